"""softnms_py_kernel<1088 / 2048, linear / gaussian / diou> through yk_decode_py_nms and yk_decode_py_packed_nms against
k210_yolo_framework_amd/softnms.py on the exact heads of tests/softnms_cases.py: `linear` and `diou` bit for bit (rows, counts, box indices; padded,
indexed and packed forms), `gaussian` by box index with the scores inside softnms_cases.bound of the float64 rule.  What every case reaches, and
that the Gaussian cases meet their input condition, is asserted on the CPU by tests/test_softnms_rule.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import softnms
from tests import nms_cases as nc
from tests import softnms_cases as sc

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10                                                       # include/yolo_hip.h
SENT_F, SENT_I = 0x7FC0F00D, -7


def _cfg_dev(base):
    from k210_yolo_framework_amd import engine
    p = sc.preds(base)
    head, anchors = sc.head_of(base)
    B, Cn = p[0].shape[0], p[0].shape[-1] - 5
    cfg = engine.make_decode_cfg(anchors, Cn, (nc.S, nc.S), head.grids)
    dev = [torch.from_numpy(np.array(q).reshape(B, q.shape[1], q.shape[2], -1)).cuda() for q in p]
    arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    return cfg, dev, arr, B, Cn


@functools.lru_cache(maxsize=None)
def _device_inputs(base, obj):
    """The boxes and scores the device itself decodes from the head, read back through the existing hard decode with nothing suppressed
    (iou_thresh 1, max_out = every box): the device's sigmoid products are the oracle's to a few ulps only, and the rule is held to ITS scores.
    The boxes are the oracle's bit for bit.  -> (boxes [B, ntot, 4], scores [B, ntot, C]; a box below obj has score 0), read-only."""
    from k210_yolo_framework_amd import engine
    cfg, dev, arr, B, Cn = _cfg_dev(base)
    n = nc.ntot(sc.head_of(base)[0])
    dets, counts, index = engine.decode_py(cfg, dev, B, None, obj, 1.0, n, return_index=True)
    torch.cuda.synchronize()
    dets, counts, index = dets.cpu().numpy(), counts.cpu().numpy(), index.cpu().numpy()
    boxes, ref_scores = sc.boxes_scores(base)
    scores = np.zeros_like(ref_scores)
    for b in range(B):
        d, i = dets[b, :counts[b]], index[b, :counts[b]]
        assert counts[b] == int((ref_scores[b] >= np.float32(obj)).sum())
        assert np.array_equal(d[:, :4].view(np.int32), boxes[b, i].view(np.int32))
        scores[b, i, d[:, 5].astype(int)] = d[:, 4]
        np.testing.assert_allclose(scores[b], np.where(ref_scores[b] >= np.float32(obj), ref_scores[b], 0), rtol=1e-5, atol=0)
    scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _reference(cid, f64=False):
    """softnms.decode_image of every image of the case on the device's own scores, computed once."""
    c = sc.by_id(cid)
    boxes, scores = _device_inputs(c.base, c.obj)
    return [softnms.decode_image(boxes[b], scores[b], c.obj, c.iou, c.max_out, c.method, c.sigma, np.float64 if f64 else np.float32)
            for b in range(boxes.shape[0])]


def _sentinels(B, cap):
    dets = torch.full((B, cap, 6), SENT_F, dtype=torch.int32, device='cuda').view(torch.float32)
    index = torch.full((B, cap), SENT_I, dtype=torch.int32, device='cuda')
    counts = torch.full((B,), SENT_I, dtype=torch.int32, device='cuda')
    return dets, counts, index


def _padded(entry, cfg, arr, B, Cn, obj, iou, max_out, *rule):
    from k210_yolo_framework_amd import engine
    dets, counts, index = _sentinels(B, Cn * max_out)
    engine.call(entry, C.byref(cfg), arr, B, None, obj, iou, max_out, dets, counts, index, engine._stream(), *rule)
    torch.cuda.synchronize()
    return dets.view(torch.int32).cpu(), counts.cpu(), index.cpu()


def _packed(entry, cfg, arr, B, Cn, obj, iou, max_out, *rule):
    from k210_yolo_framework_amd import engine
    cap = Cn * max_out
    rows = torch.full((B * cap + 4, 6), SENT_F, dtype=torch.int32, device='cuda').view(torch.float32)
    offsets = torch.full((B + 1 + 4,), SENT_I, dtype=torch.int32, device='cuda')
    rindex = torch.full((B * cap + 4,), SENT_I, dtype=torch.int32, device='cuda')
    engine.call(entry, C.byref(cfg), arr, B, None, obj, iou, max_out, rows, offsets, rindex, None, None, engine._stream(), *rule)
    torch.cuda.synchronize()
    return rows.view(torch.int32).cpu(), offsets.cpu(), rindex.cpu()


def _want(ref, B, cap):
    """The reference's rows in the padded and the packed form, sentinels behind them: (dets bits, counts, index, rows bits, offsets, rows index)."""
    dets = torch.full((B, cap, 6), SENT_F, dtype=torch.int32)
    index = torch.full((B, cap), SENT_I, dtype=torch.int32)
    counts = torch.tensor([len(d) for d, _ in ref], dtype=torch.int32)
    for b, (d, i) in enumerate(ref):
        dets[b, :len(d)] = torch.from_numpy(np.ascontiguousarray(d, np.float32).view(np.int32))
        index[b, :len(d)] = torch.from_numpy(i.astype(np.int32))
    total = int(counts.sum())
    rows = torch.full((B * cap + 4, 6), SENT_F, dtype=torch.int32)
    rindex = torch.full((B * cap + 4,), SENT_I, dtype=torch.int32)
    rows[:total] = torch.cat([dets[b, :counts[b]] for b in range(B)])
    rindex[:total] = torch.cat([index[b, :counts[b]] for b in range(B)])
    offsets = torch.full((B + 1 + 4,), SENT_I, dtype=torch.int32)
    offsets[:B + 1] = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts.long(), 0)]).int()
    return dets, counts, index, rows, offsets, rindex


@pytest.mark.parametrize('cid', [sc.case_id(c) for c in sc.CASES if c.method != 'gaussian'])
def test_linear_and_diou_equal_the_rule_bit_for_bit(cid):
    from k210_yolo_framework_amd import engine
    c = sc.by_id(cid)
    cfg, dev, arr, B, Cn = _cfg_dev(c.base)
    rule = (softnms.method_id(c.method), c.sigma)
    w_dets, w_counts, w_index, w_rows, w_off, w_rindex = _want(_reference(cid), B, Cn * c.max_out)
    assert w_counts.tolist() == [len(d) for d, _ in sc.reference(cid)]         # (the table's labels were taken on the oracle's scores)
    dets, counts, index = _padded('yk_decode_py_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    assert torch.equal(counts, w_counts)
    assert torch.equal(index, w_index)
    assert torch.equal(dets, w_dets)
    rows, offsets, rindex = _packed('yk_decode_py_packed_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    assert torch.equal(offsets, w_off) and torch.equal(rindex, w_rindex) and torch.equal(rows, w_rows)
    # engine.decode_py, without the index; and a second call of everything: the same bits
    d2, c2 = engine.decode_py(cfg, dev, B, None, c.obj, c.iou, c.max_out, nms=c.method, sigma=c.sigma)
    torch.cuda.synchronize()
    assert torch.equal(c2.cpu(), w_counts)
    for b in range(B):
        assert torch.equal(d2[b, :w_counts[b]].view(torch.int32).cpu(), w_dets[b, :w_counts[b]])
    again = _padded('yk_decode_py_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    assert all(torch.equal(a, b) for a, b in zip(again, (dets, counts, index)))


@pytest.mark.parametrize('cid', [sc.case_id(c) for c in sc.CASES if c.method == 'gaussian'])
def test_gaussian_selects_the_rules_boxes_with_scores_inside_the_bound(cid):
    c = sc.by_id(cid)
    cfg, dev, arr, B, Cn = _cfg_dev(c.base)
    rule = (softnms.method_id('gaussian'), c.sigma)
    ref32, ref64 = _reference(cid), _reference(cid, True)
    assert [i.tolist() for _, i in ref32] == [i.tolist() for _, i in sc.reference(cid)]
    dets, counts, index = _padded('yk_decode_py_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    assert counts.tolist() == [len(d) for d, _ in ref32]
    worst = 0.0
    for b, ((r32, i32), (r64, i64)) in enumerate(zip(ref32, ref64)):
        k = len(r32)
        assert np.array_equal(index[b, :k].numpy(), i32) and np.array_equal(i32, i64)
        got = dets[b, :k].numpy().view(np.float32)
        assert np.array_equal(got[:, [0, 1, 2, 3, 5]], r32[:, [0, 1, 2, 3, 5]])
        assert (dets[b, k:] == SENT_F).all() and (index[b, k:] == SENT_I).all()
        if k:
            rounds = sc.rounds_of(r32)
            first = rounds == 1
            assert np.array_equal(got[first, 4], r32[first, 4])                           # undecayed: exact
            rel = np.abs(got[:, 4].astype(np.float64) - r64[:, 4]) / r64[:, 4]
            # the float64 yardstick starts from the same fp32 scores; half an ulp for the device's final rounding is inside the bound's multiply
            worst = max(worst, float((rel[~first] / sc.bound(rounds[~first])).max()) if (~first).any() else 0.0)
    print(f'{cid}: worst score error / bound = {worst:.3f}')
    assert worst <= 1.0
    rows, offsets, rindex = _packed('yk_decode_py_packed_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    total = int(counts.sum())
    assert offsets[:B + 1].tolist() == np.concatenate([[0], np.cumsum(counts.numpy())]).tolist()
    assert torch.equal(rows[:total], torch.cat([dets[b, :counts[b]] for b in range(B)])) and (rows[total:] == SENT_F).all()
    assert torch.equal(rindex[:total], torch.cat([index[b, :counts[b]] for b in range(B)]))
    again = _padded('yk_decode_py_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, *rule)
    assert all(torch.equal(a, b) for a, b in zip(again, (dets, counts, index)))           # two calls, the same bits


@pytest.mark.parametrize('cid', [nc.case_id(c) for c in nc.CASES])
def test_hard_through_the_new_entry_points_is_the_existing_decode(cid):
    c = nc.by_id(cid)
    cfg, dev, arr, B, Cn = _cfg_dev(c.name)
    old = _padded('yk_decode_py_ex', cfg, arr, B, Cn, c.obj, c.iou, c.max_out)
    new = _padded('yk_decode_py_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, 0, 0.5)
    assert old[1].tolist() == [len(d) for d, _ in nc.reference(cid)]
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    old = _packed('yk_decode_py_packed', cfg, arr, B, Cn, c.obj, c.iou, c.max_out)
    new = _packed('yk_decode_py_packed_nms', cfg, arr, B, Cn, c.obj, c.iou, c.max_out, 0, float('nan'))      # sigma is the Gaussian's alone
    assert all(torch.equal(a, b) for a, b in zip(old, new))


def test_bad_rule_arguments_are_refused_before_any_launch():
    from k210_yolo_framework_amd import engine
    c = sc.by_id('soft1040-linear-obj0.05-iou0.3-max30')
    cfg, dev, arr, B, Cn = _cfg_dev(c.base)
    lib, st = engine.lib(), engine._stream()
    cap = Cn * c.max_out
    dets, counts, index = _sentinels(B, cap)
    rows, offsets, rindex = torch.clone(dets).view(B * cap, 6), torch.full((B + 1,), SENT_I, dtype=torch.int32, device='cuda'), torch.clone(index).view(-1)

    def padded(method, sigma, dets=dets):
        return lib.yk_decode_py_nms(C.byref(cfg), arr, B, None, c.obj, c.iou, c.max_out, dets, counts, index, st, method, sigma)

    def packed(method, sigma, rows=rows):
        return lib.yk_decode_py_packed_nms(C.byref(cfg), arr, B, None, c.obj, c.iou, c.max_out, rows, offsets, rindex, None, None, st, method, sigma)

    for method, sigma, word in ((4, 0.5, 'nms_method'), (-1, 0.5, 'nms_method'), (2, 0.0, 'nms_sigma'), (2, -0.5, 'nms_sigma'),
                                (2, float('nan'), 'nms_sigma'), (2, float('inf'), 'nms_sigma')):
        for fn in (padded, packed):
            assert fn(method, sigma) == YK_ERR_ARG, (method, sigma)
            assert word in lib.yk_last_error().decode()
    assert padded(1, 0.5, dets=None) == YK_ERR_ARG and packed(3, 0.5, rows=None) == YK_ERR_ARG
    torch.cuda.synchronize()
    for t in (dets, rows):
        assert (t.view(torch.int32) == SENT_F).all().item()
    for t in (counts, index, offsets, rindex):
        assert (t == SENT_I).all().item()
    for bad in (dict(nms='soft'), dict(nms='gaussian', sigma=0.0), dict(nms='gaussian', sigma=float('nan'))):
        with pytest.raises(engine.YkError, match='nms'):
            engine.decode_py(cfg, dev, B, None, c.obj, c.iou, c.max_out, **bad)
    assert padded(1, 0.0) == 0 and packed(3, -1.0) == 0                # sigma is read by the Gaussian only
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [len(d) for d, _ in _reference(sc.case_id(c))]


def test_pipeline_replays_each_rule_and_keeps_them_apart():
    from k210_yolo_framework_amd import engine, netspec
    from k210_yolo_framework_amd.helper import VOC_ANCHORS
    spec = netspec.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    w = spec.init_weights(seed=1)
    B = 2
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, 224, 320, 3), dtype=np.uint8)).cuda()
    pipe = engine.Pipeline(spec, w, VOC_ANCHORS, max_batch=B, depth=1, max_out=100)     # (100 rows a class: room for what hard NMS deletes)
    try:
        want = {}
        for m in softnms.METHODS:
            for _ in range(2):                                         # the capture, then its replay
                dets, counts, stream, index = pipe.submit(frames, obj_thresh=0.05, iou_thresh=0.3, max_out=100, return_index=True, nms=m, sigma=0.7)
                stream.synchronize()
                e = engine.decode_py(pipe.cfg, pipe.outs[0], B, None, 0.05, 0.3, 100, return_index=True, nms=m, sigma=0.7)
                torch.cuda.synchronize()
                k = e[1].cpu().tolist()
                assert counts.cpu().tolist() == k and sum(k) > 0
                for b in range(B):
                    assert torch.equal(dets[b, :k[b]].view(torch.int32), e[0][b, :k[b]].view(torch.int32)) and torch.equal(index[b, :k[b]], e[2][b, :k[b]])
            want[m] = (torch.cat([dets[b, :k[b]] for b in range(B)]).cpu().clone(), k)
        assert not torch.equal(want['hard'][0], want['linear'][0]) and not torch.equal(want['linear'][0], want['gaussian'][0])
        for m in ('linear', 'hard', 'gaussian', 'linear', 'diou', 'hard'):                # alternating on one slot: each its own capture
            dets, counts, stream = pipe.submit(frames, obj_thresh=0.05, iou_thresh=0.3, max_out=100, nms=m, sigma=0.7)
            stream.synchronize()
            k = counts.cpu().tolist()
            assert k == want[m][1] and torch.equal(torch.cat([dets[b, :k[b]] for b in range(B)]).cpu(), want[m][0])
        assert len(pipe.slots[0].graphs) == 8                           # 4 rules x (with, without) the index
        for m in ('gaussian', 'hard', 'gaussian'):
            rows, off = pipe.submit_host(frames.cpu().numpy(), obj_thresh=0.05, iou_thresh=0.3, max_out=100, nms=m, sigma=0.7).result()
            assert off.tolist() == np.concatenate([[0], np.cumsum(want[m][1])]).tolist() and np.array_equal(rows.view(np.int32), want[m][0].numpy().view(np.int32))
        with pytest.raises(engine.YkError, match="nms 'soft'"):
            pipe.submit(frames, nms='soft')
    finally:
        pipe.close()


def test_inference_with_linear_gives_the_rule_on_the_plans_own_outputs():
    """A mini network end to end: inference.detect(..., nms='linear') against softnms.decode_image on the boxes and scores the device itself
    decoded from the plan's outputs (read back through the hard decode with nothing suppressed: iou_thresh 1, max_out = every box).
    The network is tests/plan_zoo.py::residual, the wiring of tests/mini_net.py::residual_zoo_spec with the head the inference plans accept:
    both nets of mini_net.py itself are refused by yk_plan_create_ex (an 8-filter stem; 8 channels through the upsample)."""
    from k210_yolo_framework_amd import engine, inference
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.yolonet import YoloModel
    from tests.plan_zoo import residual
    spec, weights = residual()
    H, W = spec.in_hw
    model = YoloModel(spec, {'weights': weights, 'precision': 'f16x2'}, False)
    h = Helper(None, 20, VOC_ANCHORS, np.array([[H, W]]), np.array([list(x) for x in spec.out_hw()]))
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    obj, iou = 0.02, 0.3
    got = inference.detect(h, model, [img], obj, iou, 'linear', 0.5)[0]
    hard = inference.detect(h, model, [img], obj, iou)[0]
    plan = model._plan(1)
    cfg = engine.make_decode_cfg(h.anchors, 20, (H, W), spec.out_hw())
    ntot = sum(a * b for a, b in spec.out_hw()) * 3
    dets, counts, index = engine.decode_py(cfg, plan.outputs(), 1, np.asarray([[H, W]], np.float32), obj, 1.0, ntot, return_index=True)
    torch.cuda.synchronize()
    k = int(counts[0])
    dets, index = dets[0, :k].cpu().numpy(), index[0, :k].cpu().numpy()
    boxes, scores = np.zeros((ntot, 4), np.float32), np.zeros((ntot, 20), np.float32)
    boxes[index] = dets[:, :4]
    scores[index, dets[:, 5].astype(int)] = dets[:, 4]
    want, _ = softnms.decode_image(boxes, scores, obj, iou, 30, 'linear')
    want_hard, _ = softnms.decode_image(boxes, scores, obj, iou, 30, 'hard')
    print(f'mini net: {k} candidates, {len(want)} rows, {len(hard)} under hard NMS, {int((want[:len(hard), 4] != hard[:len(want), 4]).sum())} scores differ')
    assert len(want) > 0
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert hard.shape == want_hard.shape and np.array_equal(hard.view(np.int32), want_hard.view(np.int32))       # and the default is the default
    model._drop_plan()
