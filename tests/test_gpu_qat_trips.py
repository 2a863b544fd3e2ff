"""The quantisation-aware training kernels (csrc/yk_qat.hip) where tests/test_gpu_qat.py does not take them: activations and the weight copy past
one grid of work items, so that a workgroup goes round its grid-stride loop a second time; weight segments outside the flat buffer; and a range
table of more than 256 slots.  Cases and expected values: tests/grid_trip_cases.py (checked on their own by tests/test_grid_trip_cases.py).
Every comparison is bit for bit against tests/qat_ref.py and covers every element."""
import ctypes as C

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine
from tests import grid_trip_cases as gt
from tests import qat_ref
from tests.test_gpu_qat import RANGES, _batch_table, _bits, _cu, _range_table, _read_batch, _st

pytestmark = pytest.mark.gpu

CAL_ITEMS = gt.CAL_ITEMS                             # csrc/yk_range.h:13-15, grid_for: CAL_MAX_GRID x CAL_BLOCK = 2048 x 256 items per trip
SENTINEL = 7.0


def _up(a):
    """A device copy of a (read-only) case array."""
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize('path,shift', [('vector', 0), ('vector', 1), ('vector', 2), ('vector', 3), ('scalar', 0)])
def test_activations_past_one_grid_equal_the_restatement_bitwise(path, shift):
    """vector: y, yq, dyq and dy `shift` floats behind a 16-byte boundary (heads 0, 3, 2, 1), CAL_ITEMS + 352 float4 items and three scalars.
    scalar: yq and dy one float off y's phase, CAL_ITEMS + 352 floats, each an item."""
    L = engine.lib()
    c = gt.act_case(path, shift)
    n, shift_q, x, g = c['n'], c['shift_q'], c['x'], c['g']
    assert gt.act_items(n, shift, shift_q) > CAL_ITEMS                                            # a second trip
    slot = 0
    lo, hi = RANGES[slot]
    assert (lo, hi) == gt.QAT_RANGE
    rt = _range_table()
    xd = _cu(np.concatenate([np.zeros(shift, np.float32), x, np.float32([SENTINEL])]))
    qd = torch.full((shift_q + n + 3,), SENTINEL, dtype=torch.float32, device='cuda')
    assert xd.data_ptr() % 16 == 0 and qd.data_ptr() % 16 == 0                                     # the phases are the shifts
    bt = _batch_table(len(RANGES))
    assert L.yk_qat_act_fwd_f32(engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot), engine._ptr(qd[shift_q:]), engine._ptr(bt),
                                _st()) == 0, L.yk_last_error()
    got = qd.cpu().numpy()
    want = qat_ref.fq(x, lo, hi)
    bad = np.nonzero(_bits(got[shift_q:shift_q + n]) != _bits(want))[0]
    assert len(bad) == 0, (len(bad), bad[:8], c['second'])
    assert (got[:shift_q] == SENTINEL).all() and (got[shift_q + n:] == SENTINEL).all()             # nothing outside [0, n) is written
    blo, bhi, bfl = _read_batch(bt, len(RANGES))
    e = qat_ref.extremes(x)
    assert _bits(blo[slot:slot + 1])[0] == _bits(e[0])[0] and _bits(bhi[slot:slot + 1])[0] == _bits(e[1])[0], (blo[slot], bhi[slot], e)
    assert np.isposinf(blo[1:]).all() and np.isneginf(bhi[1:]).all() and not bfl.any()
    # backward, out of place and in place
    gd = _cu(np.concatenate([np.zeros(shift, np.float32), g, np.float32([SENTINEL])]))
    dd = torch.full((shift_q + n + 3,), SENTINEL, dtype=torch.float32, device='cuda')
    assert L.yk_qat_act_bwd_f32(engine._ptr(gd[shift:]), engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot),
                                engine._ptr(dd[shift_q:]), _st()) == 0, L.yk_last_error()
    wantg = np.where(qat_ref.ste_mask(x, lo, hi), g, np.float32(0.0)).astype(np.float32)
    gotg = dd.cpu().numpy()
    bad = np.nonzero(_bits(gotg[shift_q:shift_q + n]) != _bits(wantg))[0]
    assert len(bad) == 0, (len(bad), bad[:8], c['second'])
    assert (gotg[:shift_q] == SENTINEL).all() and (gotg[shift_q + n:] == SENTINEL).all()
    assert L.yk_qat_act_bwd_f32(engine._ptr(gd[shift:]), engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot),
                                engine._ptr(gd[shift:]), _st()) == 0
    goti = gd.cpu().numpy()
    assert _bits(goti[shift:shift + n]).tobytes() == _bits(wantg).tobytes() and (goti[:shift] == 0).all() and goti[shift + n] == SENTINEL
    back = xd.cpu().numpy()
    assert back[shift:shift + n].tobytes() == x.tobytes() and back[shift + n] == SENTINEL           # y is only read


def _run_weights(flat, offs, sizes, shift_q):
    """One yk_qat_weights_f32 call -> (Pq with its sentinels, P read back, the segments' (lo, hi, flag))."""
    L = engine.lib()
    assert L.yk_qat_tile() == gt.QAT_TILE
    total, nseg = len(flat), len(offs)
    first = gt.tile_first(sizes)
    p = _up(flat)
    pq = torch.full((total + shift_q + 2,), SENTINEL, dtype=torch.float32, device='cuda')
    wr = torch.zeros(4 * nseg, dtype=torch.int32, device='cuda')
    offd, sized, firstd = _cu(np.asarray(offs, np.int64)), _cu(np.asarray(sizes, np.int64)), _cu(first)      # (alive until the call has run)
    assert p.data_ptr() % 16 == 0 and pq.data_ptr() % 16 == 0
    rc = L.yk_qat_weights_f32(engine._ptr(p), C.c_longlong(total), engine._ptr(offd), engine._ptr(sized), engine._ptr(firstd), C.c_int(nseg),
                              C.c_int(int(first[-1])), engine._ptr(pq[shift_q:]), engine._ptr(wr), _st())
    assert rc == 0, L.yk_last_error()
    got = pq.cpu().numpy()
    assert (got[:shift_q] == SENTINEL).all() and (got[shift_q + total:] == SENTINEL).all()
    assert p.cpu().numpy().tobytes() == flat.tobytes()                                             # P is only read
    return got[shift_q:shift_q + total], _read_batch(wr, nseg)


def _check_segment(got, off, sg, slot):
    """tests/test_gpu_qat.py's criterion for one segment."""
    want = qat_ref.fq_weights(sg)
    assert _bits(got[off:off + len(sg)]).tobytes() == _bits(want).tobytes(), (off, len(sg))
    e = qat_ref.extremes(sg)
    assert slot == (e[0], e[1], 0)
    _, zp = qat_ref.qparams32(*e)
    z = sg == 0
    assert not _bits(got[off:off + len(sg)][z]).any()                                              # an exact zero stays +0.0, bit for bit,
    assert (qat_ref.codes(sg[z], *e) == zp).all()                                                  # and is the code zp
    u = qat_ref.codes(sg, *e)
    assert u.min() >= 0 and u.max() <= 255                                                         # no weight is ever clamped


@pytest.mark.parametrize('shift_q', [0, 1])
def test_weights_of_a_buffer_past_one_grid_equal_the_restatement_bitwise(shift_q):
    """shift_q 0: the copy moves CAL_ITEMS + 352 float4 and three scalars; shift_q 1: Pq one float off P's phase, every float an item of the
    copy (five trips).  Nearly all of the buffer is gap, which only the copy writes."""
    c = gt.weights_case()
    flat, offs, segs, total = c['flat'], c['offs'], c['segs'], c['total']
    assert (total // 4 if shift_q == 0 else total) > CAL_ITEMS                                     # a second trip of w_copy_reset_kernel
    got, (wlo, whi, wfl) = _run_weights(flat, offs, [len(s) for s in segs], shift_q)
    outside = np.ones(total, bool)
    for i, (off, sg) in enumerate(zip(offs, segs)):
        _check_segment(got, off, sg, (wlo[i], whi[i], wfl[i]))
        outside[off:off + len(sg)] = False
    bad = np.nonzero(_bits(got[outside]) != _bits(flat[outside]))[0]
    assert len(bad) == 0, (len(bad), np.nonzero(outside)[0][bad[:8]])                              # everything else is copied unchanged


@pytest.mark.parametrize('shift_q', [0, 1])
def test_segments_outside_the_buffer_are_skipped_and_their_neighbours_are_exact(shift_q):
    """off < 0, off + size > total and size == 0 between four good segments.  csrc/yk_qat.hip tile_of marks the first two `!ok` from off,
    size and total alone and both tile kernels return on it before any access; the third has no tile.  What lies inside the buffer of a bad
    segment is the plain copy; its range slot reads "nothing seen", flag 0."""
    c = gt.bad_segment_case()
    flat, offs, sizes, total = c['flat'], c['offs'], c['sizes'], c['total']
    got, (wlo, whi, wfl) = _run_weights(flat, offs, sizes, shift_q)
    outside = np.ones(total, bool)
    for i in range(len(offs)):
        if i in c['good']:
            _check_segment(got, offs[i], c['good'][i], (wlo[i], whi[i], wfl[i]))
            outside[offs[i]:offs[i] + sizes[i]] = False
        else:
            assert np.isposinf(wlo[i]) and np.isneginf(whi[i]) and wfl[i] == 0, (i, wlo[i], whi[i], wfl[i])
    assert _bits(got[outside]).tobytes() == _bits(flat[outside]).tobytes()


@pytest.mark.parametrize('observe', [0, 1])
def test_range_update_of_300_slots(observe):
    """update_kernel's one workgroup of 256 threads goes round its slot loop twice.  tests/test_gpu_qat.py's criterion: the table bit for bit
    tests/qat_ref.update + min / max unions, the batch extremes reset, the flags sticky."""
    L = engine.lib()
    c = gt.update_case()
    n = gt.UPDATE_SLOTS
    assert n > gt.UPDATE_BLOCK                                                                     # csrc/yk_qat.hip:117
    kd, p0d, p1d = _up(c['kind']), _up(c['p0']), _up(c['p1'])
    empty = np.tile(np.array([np.inf, -np.inf], np.float32), (n, 1))
    for r_init, m in ((c['r0'], 0.9), (empty, 0.9)) if observe else ((c['r0'], 0.9), (c['r0'], 1.0)):
        rt, bt = _up(r_init).reshape(-1), _batch_table(n)
        for slot, v in c['data'].items():
            vd = _up(v)
            assert L.yk_range_f32(engine._ptr(vd), C.c_longlong(vd.numel()), engine._ptr(bt), C.c_int(slot), _st()) == 0
        m32 = np.float32(m)
        assert L.yk_qat_update_f32(engine._ptr(rt), engine._ptr(bt), engine._ptr(kd), engine._ptr(p0d), engine._ptr(p1d), C.c_int(n), C.c_float(m32),
                                   C.c_float(np.float32(1) - m32), C.c_int(observe), _st()) == 0, L.yk_last_error()
        want, flags = gt.update_want(r_init, m, observe)
        blo, bhi, bfl = _read_batch(bt, n)
        assert np.isposinf(blo).all() and np.isneginf(bhi).all()                                   # the batch extremes start again
        assert np.array_equal(bfl, flags)                                                          # the flag is sticky
        got = rt.cpu().numpy().reshape(-1, 2)
        bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
        assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
