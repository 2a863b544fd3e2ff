"""Every branch of nms_py_kernel<1088 / 2048> and both compactions of the Python-mode decode (yk_decode_py_ex, yk_decode_py_packed) on EXACT
heads: tests/nms_cases.py builds heads whose box arithmetic is exact in fp32 on the device and in oracle/decode_ref.py, with scores from a
handful of logit levels, so the selection is compared BOX INDEX for box index, classes and boxes bit for bit, and only the scores (the device's
sigmoid) to rtol 1e-5.  The branch, template, chunking and edge every case reaches is asserted on the CPU by tests/test_nms_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nms_cases as nc

pytestmark = pytest.mark.gpu

YK_ERR_ARG = -10                                                       # include/yolo_hip.h
SENT_F, SENT_I = 0x7FC0F00D, -7                                        # one NaN pattern (compared as int32) and an impossible index / count


def _cfg_dev(c):
    from k210_yolo_framework_amd import engine
    p = nc.preds(c.name)
    B, Cn = p[0].shape[0], p[0].shape[-1] - 5
    cfg = engine.make_decode_cfg(c.anchors, Cn, (nc.S, nc.S), c.head.grids)
    dev = [torch.from_numpy(np.array(q).reshape(B, q.shape[1], q.shape[2], -1)).cuda() for q in p]
    arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    return cfg, dev, arr, B, Cn


def _sentinels(B, cap):
    dets = torch.full((B, cap, 6), SENT_F, dtype=torch.int32, device='cuda').view(torch.float32)
    index = torch.full((B, cap), SENT_I, dtype=torch.int32, device='cuda')
    counts = torch.full((B,), SENT_I, dtype=torch.int32, device='cuda')
    return dets, counts, index


def _padded(c, cfg, arr, B, Cn):
    """yk_decode_py_ex into sentinel-filled buffers -> dets (as int32 bits and as float), counts, index on the host."""
    from k210_yolo_framework_amd import engine
    dets, counts, index = _sentinels(B, Cn * c.max_out)
    engine.call('yk_decode_py_ex', C.byref(cfg), arr, B, None, c.obj, c.iou, c.max_out, dets, counts, index, engine._stream())
    torch.cuda.synchronize()
    return dets.cpu().numpy(), counts.cpu().numpy(), index.cpu().numpy()


@pytest.mark.parametrize('cid', [nc.case_id(c) for c in nc.CASES])
def test_every_nms_path_selects_the_oracles_boxes(cid):
    from k210_yolo_framework_amd import engine
    c = nc.by_id(cid)
    ref = nc.reference(cid)
    cfg, dev, arr, B, Cn = _cfg_dev(c)
    dets, counts, index = engine.decode_py(cfg, dev, B, None, c.obj, c.iou, c.max_out, return_index=True)
    torch.cuda.synchronize()
    dets, counts, index = dets.cpu().numpy(), counts.cpu().numpy(), index.cpu().numpy()
    assert counts.tolist() == [len(d) for d, _ in ref]
    for b, (rd, ridx) in enumerate(ref):
        k = len(rd)
        bad = np.flatnonzero(index[b, :k] != ridx)
        assert bad.size == 0, (b, bad[:6], index[b, :k][bad[:6]], ridx[bad[:6]], rd[bad[:6], 5])            # the same boxes, element for element
        assert np.array_equal(dets[b, :k, 5], rd[:, 5])
        assert np.array_equal(dets[b, :k, :4].view(np.int32), rd[:, :4].view(np.int32))                     # exact boxes: bit for bit
        np.testing.assert_allclose(dets[b, :k, 4], rd[:, 4], rtol=1e-5, atol=0)
    # a second call, through yk_decode_py_ex by name, into sentinel-filled buffers: bit-identical rows, nothing written behind counts
    d2, c2, i2 = _padded(c, cfg, arr, B, Cn)
    assert np.array_equal(c2, counts)
    for b in range(B):
        k = int(counts[b])
        assert np.array_equal(d2[b, :k].view(np.int32), dets[b, :k].view(np.int32)) and np.array_equal(i2[b, :k], index[b, :k])
        assert (d2[b, k:].view(np.int32) == SENT_F).all() and (i2[b, k:] == SENT_I).all()


def _packed(c, cfg, arr, B, Cn, with_index, with_padded):
    from k210_yolo_framework_amd import engine
    cap = Cn * c.max_out
    rows = torch.full((B * cap + 4, 6), SENT_F, dtype=torch.int32, device='cuda').view(torch.float32)
    offsets = torch.full((B + 1 + 4,), SENT_I, dtype=torch.int32, device='cuda')
    rindex = torch.full((B * cap + 4,), SENT_I, dtype=torch.int32, device='cuda') if with_index else None
    dets, counts, _ = _sentinels(B, cap) if with_padded else (None, None, None)
    engine.call('yk_decode_py_packed', C.byref(cfg), arr, B, None, c.obj, c.iou, c.max_out, rows, offsets, rindex, dets, counts, engine._stream())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(rows), host(offsets), host(rindex), host(dets), host(counts)


@pytest.mark.parametrize('cid', ['many-obj0.05-iou0.3-max3', 't1088-obj0.05-iou0.3-max64', 'giants-obj0.05-iou0.5-max65'])
def test_packed_rows_equal_the_padded_rows(cid):
    """compact_packed_kernel against compact_py_kernel row for row.  'many' is batch 14 x 20 classes (280 > 256: the `before` loop takes a
    second step) with four images that have no detection."""
    c = nc.by_id(cid)
    cfg, dev, arr, B, Cn = _cfg_dev(c)
    pd, pc, pi = _padded(c, cfg, arr, B, Cn)
    assert pc.tolist() == [len(d) for d, _ in nc.reference(cid)]
    want_rows = np.concatenate([pd[b, :pc[b]] for b in range(B)]).view(np.int32)
    want_index = np.concatenate([pi[b, :pc[b]] for b in range(B)])
    want_off = np.concatenate([[0], np.cumsum(pc)]).astype(np.int32)
    total = int(want_off[-1])
    assert total > 0
    for with_index, with_padded in ((True, True), (False, False), (True, False), (False, True)):
        rows, offsets, rindex, dets, counts = _packed(c, cfg, arr, B, Cn, with_index, with_padded)
        assert np.array_equal(offsets[:B + 1], want_off) and (offsets[B + 1:] == SENT_I).all()
        assert np.array_equal(rows[:total].view(np.int32), want_rows) and (rows[total:].view(np.int32) == SENT_F).all()
        if with_index:
            assert np.array_equal(rindex[:total], want_index) and (rindex[total:] == SENT_I).all()
        if with_padded:
            assert np.array_equal(counts, pc) and np.array_equal(dets.view(np.int32), pd.view(np.int32))    # rows and the sentinels behind them


def test_decode_refuses_bad_arguments_before_any_launch():
    from k210_yolo_framework_amd import engine
    c = nc.by_id('t1088-obj0.05-iou0.5-max30')
    cfg, dev, arr, B, Cn = _cfg_dev(c)
    lib, st = engine.lib(), engine._stream()
    cap = Cn * c.max_out

    def edit(**kw):
        bad = type(cfg).from_buffer_copy(cfg)
        for k, v in kw.items():
            if k == 'out_h0':
                bad.out_h[0] = v
            else:
                setattr(bad, k, v)
        return bad

    null_layer = (C.c_void_p * len(dev))(dev[0].data_ptr(), None)
    refusals = [('cfg', dict(cfg=None)), ('preds', dict(arr=None)), ('layer', dict(arr=null_layer)), ('batch', dict(B=0)), ('max_out', dict(max_out=0)),
                ('n_layers', dict(cfg=edit(n_layers=5))), ('anchor_num', dict(cfg=edit(anchor_num=9))), ('class_num', dict(cfg=edit(class_num=0))),
                ('empty layer', dict(cfg=edit(out_h0=0)))]
    dets, counts, index = _sentinels(B, cap)
    rows, offsets, rindex = _sentinels(B, cap)
    rows, rindex = rows.view(B * cap, 6), rindex.view(-1)
    offsets = torch.full((B + 1,), SENT_I, dtype=torch.int32, device='cuda')

    def untouched():
        torch.cuda.synchronize()
        for t in (dets, rows):
            assert (t.view(torch.int32) == SENT_F).all().item()
        for t in (counts, index, offsets, rindex):
            assert (t == SENT_I).all().item()

    def padded(cfg=cfg, arr=arr, B=B, max_out=c.max_out, dets=dets, counts=counts):
        return lib.yk_decode_py_ex(None if cfg is None else C.byref(cfg), arr, B, None, c.obj, c.iou, max_out, dets, counts, index, st)

    def packed(cfg=cfg, arr=arr, B=B, max_out=c.max_out, rows=rows, offsets=offsets):
        return lib.yk_decode_py_packed(None if cfg is None else C.byref(cfg), arr, B, None, c.obj, c.iou, max_out, rows, offsets, rindex, dets, counts, st)

    for what, kw in refusals:
        assert padded(**kw) == YK_ERR_ARG, what
        assert packed(**kw) == YK_ERR_ARG, what
        assert lib.yk_last_error()
    assert padded(dets=None) == YK_ERR_ARG and padded(counts=None) == YK_ERR_ARG
    assert packed(rows=None) == YK_ERR_ARG and packed(offsets=None) == YK_ERR_ARG
    assert lib.yk_decode_py(C.byref(cfg), arr, B, None, c.obj, c.iou, c.max_out, None, counts, st) == YK_ERR_ARG
    untouched()
    assert padded() == 0 and packed() == 0                             # the same buffers, good arguments: both calls run
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [len(d) for d, _ in nc.reference(nc.case_id(c))]
