"""Mosaic augmentation on the GPU: yk_mosaic_ragged_u8 bit for bit against its host copy (mosaic.compose_u8, then augment.warp_u8),
non-mosaic samples against the plain letterbox kernels, rows the kernel must not follow, bad arguments, InputPipeline(mosaic=...) against
the host generator on every rank, and `--mosaic True` end to end."""
import ctypes as C
import re

import numpy as np
import pytest

from k210_yolo_framework_amd import draw, mosaic

pytestmark = pytest.mark.gpu

HW = (224, 320)
PICTURES = [(17, 23), (40, 31), (64, 48), (1, 1), (5, 200)]
PICKS = [[0, 1, 2, 4], [4, 3, 2, 1], [2, 4, 0, 3], [1, 1, 1, 1], [3, 0, 4, 2], [4, 2, 1, 0]]      # picture of each quadrant, per sample
GAINS = [[0.5, 1.0, 0.73, 1.0], [0.73, 0.5, 1.0, 0.5], [0.5, 1.0, 0.73, 0.5], [1.0, 0.73, 0.5, 1.0], [1.0, 1.0, 1.0, 1.0], [0.73, 0.73, 0.5, 0.5]]
GAP = 7


def _seams(dst):
    H, W = dst
    return [(0, 0), (W, H), (W // 2, H // 2), (1, H - 1), (W // 2 + 3, H // 2 - 5), (W - 1, 1)]


def _batch(dst):
    """-> (pictures, packed host bytes with 255 in the gaps, ragged table [6 * 4] for dst, seams int32 [6, 2])."""
    rng = np.random.default_rng(11)
    imgs = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in PICTURES]
    packed, ptable, _ = draw.pack_ragged(imgs, gap=GAP)
    flat = packed.numpy().copy()
    for r in ptable[:-1]:
        e = int(r['offset']) + 3 * int(r['h']) * int(r['w'])
        flat[e:e + GAP] = 255                                       # (a gap byte that leaked into a picture would show)
    assert any(int(o) % 2 for o in ptable['offset'])
    seams = np.array(_seams(dst), np.int32)
    quads = np.zeros((len(PICKS), 4), mosaic.ROW_DTYPE)
    for b, (pick, gain) in enumerate(zip(PICKS, GAINS)):
        for k in range(4):
            quads[b, k] = (pick[k], *PICTURES[pick[k]], *mosaic.quadrant_params(PICTURES[pick[k]], k, seams[b, 0], seams[b, 1], gain[k], dst))
    table = mosaic.ragged_rows(quads, lambda i: int(ptable[i]['offset']))
    return imgs, flat, table, seams


def _host(imgs, table, seams, dst):
    t = table.reshape(-1, 4)
    return np.stack([mosaic.compose_u8([imgs[i] for i in PICKS[b]], t[b], seams[b], dst) for b in range(len(PICKS))])


def _quadrant(frame, k, cx, cy):
    return frame[(slice(cy, None) if k & 2 else slice(0, cy)), (slice(cx, None) if k & 1 else slice(0, cx))]


def _maps(n, hw):
    """Inverse maps for n samples: flip, rotation, shift, no flip, in turn."""
    from k210_yolo_framework_amd import augment
    u = augment.param_table(4, 0, n)
    u[:, 0] = np.array([0.05, 0.4, 0.75, 0.1])[np.arange(n) % 4]
    u[0::4, 1], u[3::4, 1] = 0.2, 0.8
    branch, flip = augment.decode(u)[:2]
    assert set(branch.tolist()) == {0, 1, 2} and flip[branch == 0].any() and not flip[branch == 0].all()
    return augment.matrices(u, hw)[2]


@pytest.mark.parametrize('dst', [(24, 40), HW])
def test_kernel_is_bit_exact_against_the_host_copy(dst):
    import torch
    from k210_yolo_framework_amd import engine
    imgs, flat, table, seams = _batch(dst)
    assert (table['tx'] < 0).any() and (table['ty'] < 0).any()
    out = engine.mosaic_ragged_u8(torch.from_numpy(flat).cuda(), table, seams, dst)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    want = _host(imgs, table, seams, dst)
    assert out.shape == want.shape == (len(PICKS), *dst, 3)
    assert any(all(_quadrant(want[b], k, *seams[b]).any() for k in range(4)) for b in range(len(PICKS)))
    for b in range(len(PICKS)):
        np.testing.assert_array_equal(out[b], want[b], err_msg=f'sample {b} seam {seams[b]}')
    assert out[0].any() and out[1].any()                            # the degenerate seams: one picture owns the whole frame


def test_warped_kernel_equals_the_host_copy_then_the_warp():
    import torch
    from k210_yolo_framework_amd import augment, engine
    dst = (24, 40)
    imgs, flat, table, seams = _batch(dst)
    M = _maps(len(PICKS), dst)
    out = engine.mosaic_ragged_u8(torch.from_numpy(flat).cuda(), table, seams, dst, inv=torch.from_numpy(M).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    want = _host(imgs, table, seams, dst)
    for b in range(len(PICKS)):
        np.testing.assert_array_equal(out[b], augment.warp_u8(want[b], M[b]), err_msg=f'sample {b}')
    assert any(not np.array_equal(out[b], want[b]) for b in range(len(PICKS)))


def test_non_mosaic_samples_equal_the_letterbox_kernels():
    import torch
    from k210_yolo_framework_amd import augment, engine
    dst = (24, 40)
    rng = np.random.default_rng(3)
    imgs = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in PICTURES]
    packed, ptable, _ = draw.pack_ragged(imgs)
    quads = np.zeros((len(imgs), 4), mosaic.ROW_DTYPE)
    for b, hw in enumerate(PICTURES):
        quads[b, :] = (b, *hw, *mosaic.letterbox_params(hw, dst))
    table = mosaic.ragged_rows(quads, lambda i: int(ptable[i]['offset']))
    seams = np.array(_seams(dst)[:len(imgs)], np.int32)
    d_packed = packed.cuda()
    M = _maps(len(imgs), dst)
    d_M = torch.from_numpy(M).cuda()
    got = engine.mosaic_ragged_u8(d_packed, table, seams, dst)
    got_w = engine.mosaic_ragged_u8(d_packed, table, seams, dst, inv=d_M)
    eye = torch.from_numpy(augment.inverse_matrices(np.stack([np.eye(2)] * len(imgs)), np.zeros((len(imgs), 2)), dst)).cuda()
    got_i = engine.mosaic_ragged_u8(d_packed, table, seams, dst, inv=eye)
    for b, im in enumerate(imgs):
        src = torch.from_numpy(im[None]).cuda()
        assert torch.equal(got[b], engine.letterbox_u8(src, dst)[0]), b
        assert torch.equal(got_w[b], engine.letterbox_augment_u8(src, dst, d_M[b:b + 1].contiguous())[0]), b
    assert torch.equal(got_i, got)                                  # a NULL d_inv is the identity map
    _, flat, mtable, mseams = _batch(dst)                           # ... for mosaics too
    d_flat = torch.from_numpy(flat).cuda()
    eye6 = torch.from_numpy(augment.inverse_matrices(np.stack([np.eye(2)] * len(PICKS)), np.zeros((len(PICKS), 2)), dst)).cuda()
    assert torch.equal(engine.mosaic_ragged_u8(d_flat, mtable, mseams, dst, inv=eye6), engine.mosaic_ragged_u8(d_flat, mtable, mseams, dst))


def test_a_row_the_kernel_must_not_follow_zeroes_only_its_quadrant():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (24, 40)
    imgs, flat, table, seams = _batch(dst)
    d_flat = torch.from_numpy(flat).cuda()
    good = engine.mosaic_ragged_u8(d_flat, table, seams, dst).cpu().numpy()
    b = 2                                                           # the sample with the seam in the middle
    cx, cy = seams[b]
    assert all(_quadrant(good[b], k, cx, cy).any() for k in range(4))
    for k, field, value in ((1, 'offset', None), (2, 'h', 0), (0, 'w', -3), (3, 'offset', 2 ** 63)):
        bad = table.copy()
        r = bad[4 * b + k]
        r[field] = len(flat) - 3 * int(r['h']) * int(r['w']) + 1 if value is None else value      # ends one byte past the buffer
        with pytest.raises(engine.YkError):
            engine.mosaic_ragged_u8(d_flat, bad, seams, dst)        # the wrapper refuses the host table ...
        if field == 'offset' and value is not None:
            with pytest.raises(engine.YkError):
                engine.check_ragged_rows(bad, len(flat))
        d_bad = torch.from_numpy(bad.view(np.uint8).reshape(len(bad), draw.RAGGED_DTYPE.itemsize)).cuda()
        out = engine.mosaic_ragged_u8(d_flat, d_bad, torch.from_numpy(seams).cuda(), dst)     # ... the kernel reads nothing for the row
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert not _quadrant(out[b], k, cx, cy).any()
        _quadrant(out[b], k, cx, cy)[...] = _quadrant(good[b], k, cx, cy)
        np.testing.assert_array_equal(out, good)                    # the other three quadrants and the neighbouring samples are intact
    with pytest.raises(engine.YkError):
        engine.mosaic_ragged_u8(d_flat, table[:6], seams, dst)      # not four rows per sample
    # seams outside the frame are clamped: an empty quadrant is legal
    wild = np.array([(-5, -7), (10 ** 6, 10 ** 6), (-1, dst[0] + 9), (dst[1] + 1, -2), (0, dst[0]), (dst[1], 0)], np.int32)
    out = engine.mosaic_ragged_u8(d_flat, table, wild, dst).cpu().numpy()
    clamped = np.stack([np.clip(wild[:, 0], 0, dst[1]), np.clip(wild[:, 1], 0, dst[0])], 1).astype(np.int32)
    np.testing.assert_array_equal(out, _host(imgs, table, clamped, dst))


def test_recorded_in_a_graph_and_replayed_gives_the_same_bytes():
    import torch
    from k210_yolo_framework_amd import engine
    dst = (24, 40)
    _, flat, table, seams = _batch(dst)
    d_flat, d_seams = torch.from_numpy(flat).cuda(), torch.from_numpy(seams).cuda()
    d_table = torch.from_numpy(table.view(np.uint8).reshape(len(table), draw.RAGGED_DTYPE.itemsize)).cuda()
    d_M = torch.from_numpy(_maps(len(PICKS), dst)).cuda()
    eager = engine.mosaic_ragged_u8(d_flat, d_table, d_seams, dst, inv=d_M)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    issue = lambda: engine.call('yk_mosaic_ragged_u8', d_flat, d_flat.numel(), d_table, d_seams, d_M, len(PICKS), out, dst[0], dst[1], st)
    graph = engine.capture(st, issue)
    try:
        assert graph.kernel_nodes == 1                              # one launch for the batch
        stream.synchronize()
        assert not out.any().item()                                 # recorded, not executed
        graph.launch(st)
        stream.synchronize()
        assert torch.equal(out, eager)
    finally:
        graph.close()


def test_bad_arguments_are_refused_not_run():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    dst = (24, 40)
    _, flat, table, seams = _batch(dst)
    p, c = torch.from_numpy(flat).cuda(), torch.from_numpy(seams).cuda()
    t = torch.from_numpy(table.view(np.uint8).reshape(len(table), draw.RAGGED_DTYPE.itemsize)).cuda()
    o = torch.empty((len(PICKS), *dst, 3), dtype=torch.uint8, device='cuda')
    nb, n = p.numel(), len(PICKS)
    assert L.yk_mosaic_ragged_u8(p, nb, t, c, None, n, o, *dst, None) == 0
    for args in [(None, nb, t, c, None, n, o, *dst), (p, nb, None, c, None, n, o, *dst), (p, nb, t, None, None, n, o, *dst),
                 (p, nb, t, c, None, n, None, *dst), (p, nb, t, c, None, 0, o, *dst), (p, nb, t, c, None, -2, o, *dst),
                 (p, 0, t, c, None, n, o, *dst), (p, nb, t, c, None, n, o, 0, dst[1]), (p, nb, t, c, None, n, o, dst[0], -1)]:
        assert L.yk_mosaic_ragged_u8(*args, None) == -10            # YK_ERR_ARG
        assert b'yk_mosaic_ragged_u8' in L.yk_last_error()
    torch.cuda.synchronize()


def _items(tmp_path):
    from PIL import Image
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
    return items


@pytest.mark.parametrize('augmented', [False, True])
def test_mosaic_pipeline_equals_the_host_generator_for_every_rank(tmp_path, augmented):
    from k210_yolo_framework_amd import pipeline, training
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    h = Helper(None, 20, VOC_ANCHORS, [list(HW)], [[7, 10], [14, 20]])
    items = _items(tmp_path)
    GB, world, seed, epoch, prob = 8, 2, 3, 1, 0.8
    order = pipeline.epoch_order(len(items), seed=seed, epoch=epoch, shuffle=True)

    class _Fixed:
        def permutation(self, n):
            return order
    aug = (seed, epoch) if augmented else None
    want = list(training.batches(h, items, GB, _Fixed(), shuffle=True, augment=aug, mosaic=(seed, epoch, prob)))
    plain = list(training.batches(h, items, GB, _Fixed(), shuffle=True, augment=aug))
    assert len(want) == len(items) // GB
    assert any(not np.array_equal(w[0][i], p[0][i]) for w, p in zip(want, plain) for i in range(GB))
    assert any(not np.array_equal(wy, py) for w, p in zip(want, plain) for wy, py in zip(w[1], p[1]))
    # what the inputs exercise: a sample with boxes of at least two pictures, a box lost to a seam, a sample that is not a mosaic
    table = mosaic.param_table(seed, epoch, len(items))
    used = order[:len(want) * GB]
    shape_of = lambda i: [(240, 320), (375, 500), (333, 500), (224, 320)][i % 4]
    dropped = []
    quads, centres, _ = mosaic.plan(used, table, shape_of, HW, boxes_of=lambda i: items[i][1], prob=prob, dropped=dropped)
    is_m = mosaic.members(used, table, HW, prob)[1]
    assert is_m.any() and not is_m.all() and sum(dropped) > 0
    contributing = [sum(len(mosaic.quadrant_boxes(items[int(r['item'])][1], (r['h'], r['w']), float(r['scale']), int(r['tx']), int(r['ty']), k,
                                                  centres[b, 0], centres[b, 1], HW)[0]) > 0 for k, r in enumerate(quads[b])) for b in np.nonzero(is_m)[0]]
    assert max(contributing) >= 2
    for rank in range(world):
        pipe = pipeline.InputPipeline(h, items, GB, rank, world, seed=seed, epoch=epoch, shuffle=True, workers=4, prefetch=2, augment=augmented,
                                      mosaic=mosaic.MosaicConfig(prob))
        got = [(x.cpu().numpy(), [y.cpu().numpy() for y in ys]) for x, ys in pipe]
        pipe.close()
        assert len(got) == len(want)
        sl = slice(rank * GB // world, (rank + 1) * GB // world)
        for (gx, gys), (wx, wys) in zip(got, want):
            np.testing.assert_array_equal(gx, wx[sl])
            for gy, wy in zip(gys, wys):
                np.testing.assert_array_equal(gy, wy[sl])
        assert pipe.producer_images_per_sec() > 0


def test_make_train_with_mosaic(tmp_path, capsys):
    from k210_yolo_framework_amd import training
    # 58 training images in batches of 24: two steps of epoch 1 with mosaic, the third step is epoch 2, which trains without
    training.cli(['--synthetic', '64', '--mosaic', 'True', '--mosaic_off_epochs', '1', '--max_nrof_epochs', '2', '--max_steps', '3',
                  '--mosaic_prob', '0.9', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '24', '--log_dir', str(tmp_path)])
    out = capsys.readouterr().out
    assert re.search(r'mosaic is True, mosaic_prob 0\.9, mosaic_off_epochs 1', out)
    assert 'epoch 2: mosaic off from here on' in out
    losses = [float(v) for v in re.findall(r'step \d+: loss (\S+)', out)]
    assert len(losses) >= 2 and all(np.isfinite(losses))
    ck = list(tmp_path.glob('*/yolo_model.h5'))
    assert len(ck) == 1 and (ck[0].parent / 'yolo_model.npz').exists()
