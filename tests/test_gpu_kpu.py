"""The KPU-exact mode on the GPU (engine.KpuPlan, csrc/yk_kpu.hip): a kmodel v3 run on the K210 KPU's integer arithmetic,
batched.  Every output and every conv layer is compared BIT FOR BIT with oracle/kpu_ref.py (computed here on the CPU), and through it
with the board's published answer on the demo picture (bicycle + car at main.c's 0.6 / 0.3)."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import oracle
from k210_yolo_framework_amd import kmodel
from oracle import kpu_ref

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / 'golden'


@pytest.fixture(scope='module')
def km():
    return kmodel.parse((GOLD / 'yolo.kmodel').read_bytes())


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD / 'kmodel_dog_golden.npz')


def _frames(gold):
    """CHW uint8 frames: the demo picture, a shifted and a mirrored copy, seeded noise, all-0, all-255, a gradient, sparse noise."""
    img = gold['image']
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, img.shape, dtype=np.uint8)
    grad = np.broadcast_to((np.arange(320) * 255 // 319).astype(np.uint8), img.shape).copy()
    sparse = np.where(rng.random(img.shape) < 0.05, 255, 0).astype(np.uint8)
    return [img, np.roll(img, (13, -29), (1, 2)), img[:, :, ::-1].copy(), noise, np.zeros_like(img), np.full_like(img, 255), grad,
            sparse]


def _run(plan, chw, layout='nhwc'):
    import torch
    x = chw if layout == 'chw' else chw.transpose(0, 2, 3, 1)
    plan.run_u8(torch.from_numpy(np.ascontiguousarray(x)).cuda(), layout=layout)
    torch.cuda.synchronize()
    n = len(chw)
    return [o[:n].cpu().numpy().transpose(0, 3, 1, 2).copy() for o in plan.outputs()]


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_demo_picture_bit_for_bit_in_both_layouts(km, gold):
    from k210_yolo_framework_amd import engine
    with engine.KpuPlan(km, max_batch=2) as plan:
        for layout in ('chw', 'nhwc'):
            y1, y2 = _run(plan, gold['image'][None], layout)
            assert _same_bits(y1[0], gold['y1_q']), layout
            assert _same_bits(y2[0], gold['y2_q']), layout


def test_the_boards_answer_through_the_drop_in_region_layer(km, gold):
    """main.c:280-288 on the GPU outputs: the bicycle and the car of asset/k210_res.jpg, no dog."""
    from k210_yolo_framework_amd import engine
    with engine.KpuPlan(km, max_batch=1) as plan:
        outs = _run(plan, gold['image'][None], 'chw')
    dets = []
    for li, (W, H) in enumerate([(10, 7), (20, 14)]):
        res = oracle.drive_region_abi(engine.lib(), outs[li][0].reshape(3, 25, H, W).copy(), gold['anchors'][li], W, H, 3, 20, 0.6, 0.3)
        dets.append(np.asarray(res[3], np.uint32).reshape(-1, 6))
    dets = np.concatenate(dets, 0)
    np.testing.assert_array_equal(dets, gold['dets'])
    assert sorted(int(c) for c in dets[:, 4]) == [1, 6]                           # bicycle, car


def test_every_conv_layer_and_output_of_a_batch_of_eight(km, gold):
    from k210_yolo_framework_amd import engine
    frames = np.stack(_frames(gold))
    with engine.KpuPlan(km, max_batch=8) as plan:
        outs = _run(plan, frames, 'nhwc')
        for i, f in enumerate(frames):
            keep = {}
            ref = kpu_ref.run(km, f, keep)
            for li, q in keep.items():
                got = plan.read_layer(li, i)
                assert np.array_equal(got, q), (i, li, int((got != q).sum()))
            for o, r in zip(outs, ref):
                assert _same_bits(o[i], r), i


def test_results_do_not_depend_on_the_batch_and_a_replay_equals_the_eager_run(km, gold):
    import torch
    from k210_yolo_framework_amd import engine
    base = np.stack(_frames(gold))
    rng = np.random.default_rng(3)
    frames = np.concatenate([base, rng.integers(0, 256, (25, *base.shape[1:]), dtype=np.uint8)])     # 33 frames
    with engine.KpuPlan(km, max_batch=64) as plan:
        full = _run(plan, frames, 'chw')
        for n in (1, 7, 32):
            part = _run(plan, frames[:n], 'chw')
            for a, b in zip(part, full):
                assert _same_bits(a, b[:n]), n
        # graph replay on a created stream (the eager run on the same stream comes first)
        s = torch.cuda.Stream()
        x = torch.from_numpy(np.ascontiguousarray(frames[:32])).cuda()
        torch.cuda.synchronize()
        plan.run_u8(x, layout='chw', stream=s)
        s.synchronize()
        eager = [o[:32].cpu().numpy() for o in plan.outputs()]
        for o in plan.outputs():
            o.zero_()
        torch.cuda.synchronize()
        g = engine.capture(C.c_void_p(s.cuda_stream), lambda: plan.run_u8(x, layout='chw', stream=s))
        assert g.kernel_nodes == len(plan.launches())
        g.launch(C.c_void_p(s.cuda_stream))
        s.synchronize()
        replay = [o[:32].cpu().numpy() for o in plan.outputs()]
        g.close()
        for a, b, c in zip(eager, replay, full):
            assert _same_bits(a, b) and _same_bits(a, c.transpose(0, 2, 3, 1)[:32])


def _extreme(km, which):
    """A deep copy of the demo model with register fields at the ends of their bit widths (only what kpu_ref itself runs)."""
    m = copy.deepcopy(km)
    cv = m.convs
    rng = np.random.default_rng(11)
    if which == 0:
        dw, pw, dw2 = cv[1], cv[2], cv[25]
        dw.pad_value = 0
        dw.bn_mul[:] = -dw.bn_mul                                                # negative multipliers
        dw.bn_shift[:] = 15
        pw.act_shift[:] = [0, 1, 64, 255, 70, 20, 3, 0, 1, 255, 64, 20, 20, 20, 20, 20]
        pw.act_start[:] = rng.permutation(pw.act_start)                         # unsorted starts: only the scan order decides
        dw2.arg_x, dw2.arg_w, dw2.arg_add = (1 << 23) - 1, -(1 << 23), -(1 << 39)
    elif which == 1:
        a, b = cv[27], cv[30]                                                    # the 3x3 dense convs of the head (K = 6912, 4608)
        a.pad_value = 255
        a.arg_w, a.arg_x = (1 << 23) - 1, (1 << 23) - 1
        a.bn_mul[::2] = -(1 << 23)
        a.bn_shift[:] = 15
        a.act_shift[:] = np.arange(16) * 17                                      # 0 .. 255
        b.pad_value = 0
        b.weights[:] = 255
        b.arg_add = -(1 << 39)
        b.act_start[:] = rng.permutation(np.arange(-8, 8) * (1 << 31))
        b.act_shift[:] = [1, 0, 64, 63, 62, 65, 1, 0, 5, 9, 200, 2, 1, 0, 3, 4]
        b.act_mul[:] = rng.integers(-(1 << 15), 1 << 15, 16)
    elif which == 2:
        stem = cv[0]                                                             # saturates the stem: on its own, so that later cases see live frames
        stem.pad_value = 255
        stem.weights[:] = 255                                                    # all-255 weights
        stem.arg_x, stem.arg_add = -(1 << 23), (1 << 39) - 1
    else:
        _clamp_case(cv[2])
    return m


CLAMP_LAYER = 2
CLAMP_BIAS = 5 + 8 * np.arange(16)                                               # int8 biases, one per segment, 8 apart


def _clamp_case(c):
    """Every segment of a live layer shifts by 65..255 with multipliers of both signs: (z - start) * mul >> (s - 1) is then the sign fill
    (-1 / 0) under numpy's rule, while a count taken mod 64 would shift by 0..63 and give other values."""
    c.act_shift[:] = [65, 200, 255, 66, 65, 100, 127, 128, 129, 65, 200, 255, 70, 80, 90, 65]
    c.act_mul[:] = [(-1) ** s * ((1 << 15) - 1 - 37 * s) for s in range(16)]
    c.act_bias[:] = CLAMP_BIAS                                                   # the segment shows in the output: bias - 1 or bias


def _shift_mod64(m):
    """The same model with every act_shift replaced by what a kernel computing `v >> ((s - 1) & 63)` would use."""
    w = copy.deepcopy(m)
    for c in w.convs:
        s = np.asarray(c.act_shift, np.int64)
        c.act_shift[:] = np.where(s > 0, ((s - 1) & 63) + 1, s)
    return w


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_register_fields_at_the_ends_of_their_widths(km, gold, which):
    from k210_yolo_framework_amd import engine
    m = _extreme(km, which)
    rng = np.random.default_rng(5)
    frames = np.stack([np.full_like(gold['image'], 255), rng.integers(0, 256, gold['image'].shape, dtype=np.uint8)])
    with engine.KpuPlan(m, max_batch=2) as plan:
        outs = _run(plan, frames, 'chw')
        for i, f in enumerate(frames):
            keep = {}
            ref = kpu_ref.run(m, f, keep)
            for li, q in keep.items():
                assert np.array_equal(plan.read_layer(li, i), q), (which, i, li)
            for o, r in zip(outs, ref):
                assert _same_bits(o[i], r), (which, i)
            if which == 3:
                # the clamp is pinned: shift counts >= 65 are selected here, and counting them mod 64 would change the layer
                y = keep[CLAMP_LAYER]
                assert np.isin(y, CLAMP_BIAS - 1).any() and np.isin(y, CLAMP_BIAS).any(), (i, np.unique(y))
                alt = {}
                kpu_ref.run(_shift_mod64(m), f, alt)
                assert (alt[CLAMP_LAYER] != y).mean() > 0.5, i


def test_plans_beyond_32_bit_indexing_are_refused_at_create(km):
    from k210_yolo_framework_amd import engine
    with pytest.raises(engine.YkError, match='32-bit indexing'):
        engine.KpuPlan(km, max_batch=1 << 14)                                    # 48 x 112 x 160 x 16384 > 2^30 elements


def test_user_path_predict_and_detect_give_the_boards_outputs(km, gold, tmp_path):
    import torch
    from PIL import Image
    from k210_yolo_framework_amd import engine, inference, yolonet
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    infer, wrapped = yolonet.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75, precision='kpu')
    infer.load_weights(str(GOLD / 'yolo.kmodel'))
    frame = gold['image'].transpose(1, 2, 0)[None].copy()
    y1, y2 = infer.predict(frame)
    assert _same_bits(y1[0].transpose(2, 0, 1), gold['y1_q']) and _same_bits(y2[0].transpose(2, 0, 1), gold['y2_q'])
    w1, _ = wrapped.predict(frame)
    assert w1.shape == (1, 7, 10, 3, 25) and _same_bits(w1.reshape(y1.shape), y1)
    # inference.detect in kpu mode on the demo picture saved at the network's size
    path = tmp_path / 'dog_224x320.png'
    Image.fromarray(frame[0]).save(path)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    img = h._read_img(str(path))
    dets = inference.detect(h, infer, [img], 0.5, 0.3)[0]
    lb = engine.letterbox_u8(torch.from_numpy(img[None].copy()).cuda(), (224, 320)).cpu().numpy()
    assert np.array_equal(lb[0], frame[0])                                       # the letterbox is the identity at this size
    ref = kpu_ref.run(km, lb[0].transpose(2, 0, 1).copy())
    preds = [torch.from_numpy(r.transpose(1, 2, 0)[None].copy()).cuda() for r in ref]
    cfg = engine.make_decode_cfg(h.anchors, h.class_num, h.in_hw[0], h.out_hw)
    rd, rc = engine.decode_py(cfg, preds, 1, np.asarray([img.shape[:2]], np.float32), 0.5, 0.3)
    torch.cuda.synchronize()
    want = rd[0, :int(rc[0])].cpu().numpy()
    assert len(dets) > 0 and _same_bits(dets, want)


def test_kpu_mode_refuses_what_it_cannot_run(km, gold):
    from k210_yolo_framework_amd import engine, yolonet
    frame = gold['image'].transpose(1, 2, 0)[None].copy()
    infer, _ = yolonet.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75, precision='kpu')
    with pytest.raises(engine.YkError, match='kmodel'):
        infer.predict(frame)                                                     # no kmodel loaded
    infer.load_weights(str(GOLD / 'yolo.kmodel'))
    with pytest.raises(engine.YkError, match='uint8'):
        infer.predict(frame.astype(np.float32) / 255.0)                           # normalised floats
    other, _ = yolonet.yolo_mobilev1((224, 320, 3), 3, 4, alpha=0.75, precision='kpu')
    other._s['kmodel'] = km                                                      # a kmodel whose outputs do not fit this head
    with pytest.raises(engine.YkError, match='this network'):
        other.predict(frame)
    # the float weights from the same file keep working in the float modes
    infer.precision = 'f16x2'
    assert [o.shape for o in infer.predict(frame)] == [(1, 7, 10, 75), (1, 14, 20, 75)]
