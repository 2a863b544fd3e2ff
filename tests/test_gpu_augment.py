"""Training augmentation on the GPU: yk_letterbox_augment_u8 bit for bit against the host copy (letterbox_bilinear, then
augment.warp_u8), InputPipeline(augment=True) against the host generator on every rank, and `--augmenter True` end to end."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HW = (224, 320)


def _h():
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    return Helper(None, 20, VOC_ANCHORS, [list(HW)], [[7, 10], [14, 20]])


def _host(h, img, M):
    from k210_yolo_framework_amd import augment
    from k210_yolo_framework_amd.helper import letterbox_bilinear
    s, t = h.letterbox_params(img.shape[:2])
    return augment.warp_u8(letterbox_bilinear(img, HW, float(s[0]), t), M)


@pytest.mark.parametrize('src_hw', [(224, 320), (375, 500), (333, 500), (100, 100)])
def test_fused_kernel_is_bit_exact_against_the_host_copy(src_hw):
    import torch
    from k210_yolo_framework_amd import augment, engine
    B = 16
    rng = np.random.default_rng(src_hw[0] + src_hw[1])
    frames = rng.integers(0, 256, (B, *src_hw, 3), dtype=np.uint8)
    u = augment.param_table(src_hw[0], 0, B)
    u[:, 0] = np.array([0.05, 0.4, 0.75, 0.1])[np.arange(B) % 4]                 # flip / rotate / translate / flip, in turn
    u[0::8, 1], u[4::8, 1] = 0.2, 0.8                                             # ... flip and no flip
    A, t, M = augment.matrices(u, HW)
    branch, flip = augment.decode(u)[:2]
    assert set(branch.tolist()) == {0, 1, 2} and flip[branch == 0].any() and not flip[branch == 0].all()
    out = engine.letterbox_augment_u8(torch.from_numpy(frames).cuda(), HW, torch.from_numpy(M).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    h = _h()
    for b in range(B):
        np.testing.assert_array_equal(out[b], _host(h, frames[b], M[b]), err_msg=f'image {b} branch {branch[b]}')


def test_identity_and_flip_equal_the_letterbox_and_its_mirror():
    import torch
    from k210_yolo_framework_amd import augment, engine
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (4, 375, 500, 3), dtype=np.uint8)).cuda()
    A = np.stack([np.eye(2), np.diag([-1.0, 1.0])] * 2)
    M = torch.from_numpy(augment.inverse_matrices(A, np.zeros((4, 2)), HW)).cuda()
    got = engine.letterbox_augment_u8(frames, HW, M)
    ref = engine.letterbox_u8(frames, HW)
    torch.cuda.synchronize()
    assert torch.equal(got[0::2], ref[0::2])
    assert torch.equal(got[1::2], torch.flip(ref[1::2], dims=[2]))


def test_null_inverse_maps_and_bad_arguments_are_rejected():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    src = torch.zeros((1, 10, 10, 3), dtype=torch.uint8, device='cuda')
    dst = torch.zeros((1, *HW, 3), dtype=torch.uint8, device='cuda')
    inv = torch.zeros((1, 6), dtype=torch.float64, device='cuda')
    s = engine._stream()
    P = engine._ptr
    assert L.yk_letterbox_augment_u8(P(src), 1, 10, 10, None, P(dst), HW[0], HW[1], s) == -10
    assert 'bad argument' in L.yk_last_error().decode()
    assert L.yk_letterbox_augment_u8(None, 1, 10, 10, P(inv), P(dst), HW[0], HW[1], s) == -10
    assert L.yk_letterbox_augment_u8(P(src), 0, 10, 10, P(inv), P(dst), HW[0], HW[1], s) == -10
    assert L.yk_letterbox_augment_u8(P(src), 1, 10, 10, P(inv), None, HW[0], HW[1], s) == -10
    assert L.yk_letterbox_augment_u8(P(src), 1, 10, 10, P(inv), P(dst), 0, HW[1], s) == -10
    assert L.yk_letterbox_augment_u8(P(src), 1, 10, 10, P(inv), P(dst), HW[0], HW[1], s) == 0
    torch.cuda.synchronize()


def test_augmented_pipeline_equals_the_host_generator_for_every_rank(tmp_path):
    from PIL import Image
    from k210_yolo_framework_amd import pipeline, training
    h = _h()
    rng = np.random.default_rng(6)
    items = []
    for k in range(22):
        hw = [(240, 320), (375, 500), (333, 500), (224, 320)][k % 4]
        img = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
        n = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(0.05, 0.3, (n, 2))], 1)
        if k % 3 == 0:
            p = tmp_path / f'{k}.png'
            Image.fromarray(img).save(p)
            items.append((str(p), boxes))
        else:
            items.append((img, boxes))
    GB, world, seed, epoch = 8, 2, 3, 1
    order = pipeline.epoch_order(len(items), seed=seed, epoch=epoch, shuffle=True)

    class _Fixed:
        def permutation(self, n):
            return order
    want = list(training.batches(h, items, GB, _Fixed(), shuffle=True, augment=(seed, epoch)))
    plain = list(training.batches(h, items, GB, _Fixed(), shuffle=True))
    assert len(want) == len(items) // GB
    assert any(not np.array_equal(w[0][i], p[0][i]) for w, p in zip(want, plain) for i in range(GB))
    for rank in range(world):
        pipe = pipeline.InputPipeline(h, items, GB, rank, world, seed=seed, epoch=epoch, shuffle=True, workers=4, prefetch=2, augment=True)
        got = [(x.cpu().numpy(), [y.cpu().numpy() for y in ys]) for x, ys in pipe]
        pipe.close()
        assert len(got) == len(want)
        sl = slice(rank * GB // world, (rank + 1) * GB // world)
        for (gx, gys), (wx, wys) in zip(got, want):
            np.testing.assert_array_equal(gx, wx[sl])
            for gy, wy in zip(gys, wys):
                np.testing.assert_array_equal(gy, wy[sl])
        assert pipe.producer_images_per_sec() > 0


def test_augmented_pipeline_divides_by_the_augmented_images_own_maximum(tmp_path):
    """Dark and sub-255 images, and dim ones whose only 255 is a corner pixel: the warp moves it out of the frame or blends it, so the
    divisor is the maximum of the augmented image, not of its source."""
    from PIL import Image
    from k210_yolo_framework_amd import pipeline, training
    from tests.test_gpu_pipeline import divisors
    h = _h()
    rng = np.random.default_rng(16)
    items, corner = [], []
    for k in range(12):
        hw = [(240, 320), (375, 500), (333, 500), (224, 320)][k % 4]
        if k % 3 == 2:
            img = rng.integers(0, 256, (*HW, 3), dtype=np.uint8) // 16
            img[[0, 0, -1, -1][k % 4], [0, -1, 0, -1][k % 4]] = 255
            corner.append(k)
        else:
            img = rng.integers(0, 256, (*hw, 3), dtype=np.uint8) // 16 if k % 3 == 0 else rng.integers(0, 200, (*hw, 3), dtype=np.uint8)
        n = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(0.05, 0.3, (n, 2))], 1)
        if k % 5 == 0:
            p = tmp_path / f'{k}.png'
            Image.fromarray(img).save(p)
            items.append((str(p), boxes))
        else:
            items.append((img, boxes))
    GB, seed, epoch = 4, 3, 1
    order = pipeline.epoch_order(len(items), seed=seed, epoch=epoch, shuffle=True)

    class _Fixed:
        def permutation(self, n):
            return order
    want = list(training.batches(h, items, GB, _Fixed(), shuffle=True, augment=(seed, epoch)))
    plain = list(training.batches(h, items, GB, _Fixed(), shuffle=True))
    assert len(want) == 3
    div, div_plain = np.array([divisors(wx) for wx, _ in want]), np.array([divisors(px) for px, _ in plain])
    assert all(len(set(d)) > 1 for d in div), div
    is_corner = np.isin(order[:12].reshape(3, GB), corner)
    assert (div_plain[is_corner] == 255).all() and (div[is_corner] != 255).any(), (div, div_plain)
    pipe = pipeline.InputPipeline(h, items, GB, 0, 1, seed=seed, epoch=epoch, shuffle=True, workers=4, prefetch=2, augment=True)
    got = [(x.cpu().numpy(), [y.cpu().numpy() for y in ys]) for x, ys in pipe]
    pipe.close()
    assert len(got) == len(want)
    for (gx, gys), (wx, wys) in zip(got, want):
        np.testing.assert_array_equal(gx, wx)
        for gy, wy in zip(gys, wys):
            np.testing.assert_array_equal(gy, wy)


def test_make_train_with_the_augmenter(tmp_path, capsys):
    from k210_yolo_framework_amd import training
    training.cli(['--synthetic', '64', '--augmenter', 'True', '--max_steps', '3', '--model_def', 'yolo_mobilev1', '--depth_multiplier',
                  '0.5', '--batch_size', '8', '--max_nrof_epochs', '1', '--log_dir', str(tmp_path)])
    out = capsys.readouterr().out
    assert re.search(r'data augment is\s+True', out)
    losses = [float(v) for v in re.findall(r'step \d+: loss (\S+)', out)]
    assert losses and all(np.isfinite(losses))
    ck = list(tmp_path.glob('*/yolo_model.h5'))
    assert len(ck) == 1 and (ck[0].parent / 'yolo_model.npz').exists()
