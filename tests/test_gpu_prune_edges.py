"""The magnitude-pruning select and mask kernels (csrc/yk_prune.hip) at the C entry on the crafted segments and tables of
tests/prune_cases.py: the digit and bin boundaries of the four-pass radix select, ties across the threshold, NaN and zero contents, the
keep clamp, segments of size 0, many segments, a recorded call replayed on changed weights, the dispatch of yk_mask_apply_f32 and the
refusals.  The expected values come from prune_cases.reference (one sort of the uint32 patterns); every comparison is exact: threshold
bits, mask bytes, kept.  tests/test_prune_cases.py shows, without a GPU, that the cases reach the boundaries they are named for."""
import ctypes as C

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine
from tests import prune_cases as pc
from tests.test_gpu_prune import _cu, _masks, _st

pytestmark = pytest.mark.gpu

U = np.uint32
YK_ERR_ARG = -10                                                  # include/yolo_hip.h
FILL, THR_FILL, KEPT_FILL = 7, -1.0, -1                           # what _masks leaves in the outputs before the call


def _run(lay):
    return _masks(lay.flat.copy(), lay.offsets, lay.sizes, lay.keeps, fill=FILL)


def _want(lay):
    """The three outputs of a call on `lay` as the reference gives them: fills outside the segments and for segments of size 0."""
    mask = np.full(lay.flat.size, FILL, np.uint8)
    thr = np.full(len(lay.sizes), THR_FILL, np.float32)
    kept = np.full(len(lay.sizes), KEPT_FILL, np.int64)
    for i, (o, n, r) in enumerate(zip(lay.offsets, lay.sizes, pc.expected(lay))):
        if r is not None:
            mask[o:o + n], thr.view(U)[i], kept[i] = r.mask, r.bits, r.kept
    return mask, thr, kept


def _check(lay, got):
    mask, thr, kept = got
    wmask, wthr, wkept = _want(lay)
    for i, (o, n, k) in enumerate(zip(lay.offsets, lay.sizes, lay.keeps)):
        what = (lay.name, i, n, k)
        assert thr.view(U)[i] == wthr.view(U)[i], what + (hex(thr.view(U)[i]), hex(wthr.view(U)[i]))
        assert kept[i] == wkept[i], what + (kept[i], wkept[i])
        assert np.array_equal(mask[o:o + n], wmask[o:o + n]), what + (int((mask[o:o + n] != wmask[o:o + n]).sum()),)
    assert mask.tobytes() == wmask.tobytes(), lay.name                    # the gaps, and the bytes of segments of size 0, hold the fill
    assert thr.tobytes() == wthr.tobytes() and kept.tobytes() == wkept.tobytes(), lay.name


@pytest.mark.parametrize('name', pc.KIND_NAMES)
def test_crafted_segments_in_one_call_and_each_alone(name):
    lay = pc.kind_layout(name)
    mask, thr, kept = _run(lay)
    _check(lay, (mask, thr, kept))
    for i, (o, n, k) in enumerate(zip(lay.offsets, lay.sizes, lay.keeps)):
        one = pc.layout(f'{name}-{n}-alone', [lay.flat[o:o + n]], [k])
        m1, t1, k1 = _run(one)
        _check(one, (m1, t1, k1))
        o1 = one.offsets[0]
        assert m1[o1:o1 + n].tobytes() == mask[o:o + n].tobytes() and t1.tobytes() == thr[i:i + 1].tobytes() and k1[0] == kept[i], (name, n)


def test_keep_is_clamped_to_1_and_n():
    lay = pc.clamp_layout()
    mask, thr, kept = _run(lay)
    _check(lay, (mask, thr, kept))
    assert kept.tolist() == [pc.clamp_keep(k, n) for n, k in zip(lay.sizes, lay.keeps)]      # distinct values: kept is the clamped keep itself


@pytest.mark.parametrize('name', sorted(pc.ZERO_PLACEMENTS))
def test_segments_of_size_0_get_no_output_and_change_nothing_for_their_neighbours(name):
    lay, bare = pc.zero_layout(name), pc.zero_layout(name, with_zeros=False)
    mask, thr, kept = _run(lay)
    _check(lay, (mask, thr, kept))
    empty = [i for i, n in enumerate(lay.sizes) if n == 0]
    assert empty and (thr[empty] == THR_FILL).all() and (kept[empty] == KEPT_FILL).all()
    bmask, bthr, bkept = _run(bare)
    _check(bare, (bmask, bthr, bkept))
    full = [i for i, n in enumerate(lay.sizes) if n]
    assert thr[full].tobytes() == bthr.tobytes() and kept[full].tobytes() == bkept.tobytes()
    for i, j in zip(full, range(len(bare.sizes))):
        n = lay.sizes[i]
        assert mask[lay.offsets[i]:lay.offsets[i] + n].tobytes() == bmask[bare.offsets[j]:bare.offsets[j] + n].tobytes(), (name, i)


@pytest.mark.parametrize('nseg', pc.NSEGS)
def test_every_tile_finds_its_segment(nseg):
    lay = pc.nseg_layout(nseg)
    _check(lay, _run(lay))


def test_a_recorded_call_replayed_on_changed_weights_equals_a_fresh_eager_call():
    """One eager call on the stream (its scratch then has its size), one recording, then replays on weights overwritten in place: the
    histogram clear is part of the recording and no pass sees the counts of the replay before."""
    L = engine.lib()
    a = pc.kind_layout('pass2-bin255-last')
    lays = {'a': a}
    for key, name in (('b', 'pass0-bin0-first'), ('c', 'ties257'), ('d', 'nan_payload')):      # the same table, other weights
        lays[key] = pc.layout(f'replay-{name}', [pc.segment(name, n)[0] for n in pc.SIZES], a.keeps)
        assert lays[key].offsets == a.offsets and lays[key].sizes == a.sizes
    nseg = len(a.sizes)
    p, off, size, keep, tf = _cu(a.flat.copy()), _cu(np.asarray(a.offsets, np.int64)), _cu(np.asarray(a.sizes, np.int64)), \
        _cu(np.asarray(a.keeps, np.int64)), _cu(a.tile_first)
    mask = torch.full((a.flat.size,), FILL, dtype=torch.uint8, device='cuda')
    thr = torch.full((nseg,), THR_FILL, dtype=torch.float32, device='cuda')
    kept = torch.full((nseg,), KEPT_FILL, dtype=torch.int64, device='cuda')
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def issue():
        engine._check(L.yk_prune_masks_f32(engine._ptr(p), engine._ptr(off), engine._ptr(size), engine._ptr(keep), engine._ptr(tf), C.c_int(nseg),
                                           C.c_int(int(a.tile_first[-1])), engine._ptr(mask), engine._ptr(thr), engine._ptr(kept), st), 'yk_prune_masks_f32')

    def outputs():
        stream.synchronize()
        return mask.cpu().numpy(), thr.cpu().numpy(), kept.cpu().numpy()

    def clear():
        mask.fill_(FILL), thr.fill_(THR_FILL), kept.fill_(KEPT_FILL)
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    issue()
    _check(a, outputs())
    clear()
    graph = engine.capture(st, issue)
    try:
        assert graph.kernel_nodes == graph.nodes == 10                                # the clear, 4 x (histogram, pick), the mask: all kernels
        got = outputs()
        assert (got[0] == FILL).all() and (got[1] == THR_FILL).all() and (got[2] == KEPT_FILL).all()      # recorded, not executed
        for key in ('b', 'a', 'c', 'd', 'd', 'a'):
            lay = lays[key]
            p.copy_(torch.from_numpy(lay.flat.copy()))
            clear()
            graph.launch(st)
            got = outputs()
            _check(lay, got)
            fresh = _run(lay)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, fresh)), key
    finally:
        graph.close()


# ------------------------------------------------------------------------------------------------ yk_mask_apply_f32
SPECIALS = np.array([0x80000000, 0x7fc12345, 0xffc54321, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x3fc00000, 0xc0100000,
                     0x00000000, 0x7f800001, 0xffffffff], U)
ALIGNMENTS = [(0, 0), (0, 1), (0, 2), (0, 3), (4, 0), (8, 0), (12, 0), (4, 1)]          # bytes that params / mask are off their 16 / 4


@pytest.mark.parametrize('n', [4, 5, 7, 1023, 1024, 1025])
@pytest.mark.parametrize('p_off,m_off', ALIGNMENTS)
def test_mask_apply_on_both_paths_at_group_and_workgroup_boundaries(n, p_off, m_off):
    L = engine.lib()
    rng = np.random.default_rng(n * 64 + p_off * 4 + m_off)
    pad = 8
    e = p_off // 4
    wu = SPECIALS[rng.integers(0, SPECIALS.size, n + pad)]
    m = (rng.uniform(size=n + pad) < 0.6).astype(np.uint8) * rng.integers(1, 256, n + pad).astype(np.uint8)      # any non-zero byte keeps
    wu[e:e + 4] = (0x80000000, 0x7fc12345, 0xffc54321, 0x807fffff)       # -0.0, NaN payloads, a denormal under four different non-zero bytes:
    m[m_off:m_off + 4] = (1, 2, 128, 255)                                # the group that is not written back
    if n >= 1023:
        g = (n // 4 - 1) * 4                                             # the same in the last full group, and a group with one zero byte
        wu[e + g:e + g + 4] = (0xffffffff, 0x80000000, 0x7f800001, 0x00000001)
        m[m_off + g:m_off + g + 4] = (255, 128, 2, 1)
        wu[e + 8:e + 12] = (0x80000000, 0x7fc12345, 0x80000000, 0xffc54321)
        m[m_off + 8:m_off + 12] = (1, 0, 0, 255)
    p, md = _cu(wu.view(np.float32)), _cu(m)
    assert p.data_ptr() % 16 == 0 and md.data_ptr() % 4 == 0
    pv, mv = p[e:], md[m_off:]
    assert pv.data_ptr() % 16 == p_off and mv.data_ptr() % 4 == m_off
    assert L.yk_mask_apply_f32(engine._ptr(pv), engine._ptr(mv), C.c_longlong(n), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    want = wu.copy()
    want[e:e + n] = np.where(m[m_off:m_off + n] != 0, wu[e:e + n], U(0))              # masked: +0.0; kept: the same bits; outside [0, n): untouched
    got = p.cpu().numpy().view(U)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    assert md.cpu().numpy().tobytes() == m.tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_the_argument_error_and_launch_nothing():
    L = engine.lib()
    lay = pc.kind_layout('zeros')
    nseg, ntiles = len(lay.sizes), int(lay.tile_first[-1])
    t = dict(params=_cu(lay.flat.copy()), off=_cu(np.asarray(lay.offsets, np.int64)), size=_cu(np.asarray(lay.sizes, np.int64)),
             keep=_cu(np.asarray(lay.keeps, np.int64)), tf=_cu(lay.tile_first),
             mask=torch.full((lay.flat.size,), FILL, dtype=torch.uint8, device='cuda'),
             thr=torch.full((nseg,), THR_FILL, dtype=torch.float32, device='cuda'), kept=torch.full((nseg,), KEPT_FILL, dtype=torch.int64, device='cuda'))

    def call(null=None, nseg=nseg, ntiles=ntiles):
        ptr = {k: C.c_void_p(None) if k == null else engine._ptr(v) for k, v in t.items()}
        return L.yk_prune_masks_f32(ptr['params'], ptr['off'], ptr['size'], ptr['keep'], ptr['tf'], C.c_int(nseg), C.c_int(ntiles), ptr['mask'], ptr['thr'],
                                    ptr['kept'], _st())

    bad = [dict(null=k) for k in t] + [dict(nseg=0), dict(nseg=-1), dict(ntiles=0), dict(ntiles=-1)]
    for kw in bad:
        assert call(**kw) == YK_ERR_ARG and b'yk_prune_masks_f32' in L.yk_last_error(), kw
        torch.cuda.synchronize()
        assert bool((t['mask'] == FILL).all()) and bool((t['thr'] == THR_FILL).all()) and bool((t['kept'] == KEPT_FILL).all()), kw
    assert call() == 0                                                   # the same arguments, none of them bad
    torch.cuda.synchronize()
    _check(lay, (t['mask'].cpu().numpy(), t['thr'].cpu().numpy(), t['kept'].cpu().numpy()))

    wu = SPECIALS[np.arange(64) % SPECIALS.size]
    p, md = _cu(wu.view(np.float32)), torch.zeros(64, dtype=torch.uint8, device='cuda')
    for args in ((None, engine._ptr(md), 64), (engine._ptr(p), None, 64), (engine._ptr(p), engine._ptr(md), 0), (engine._ptr(p), engine._ptr(md), -1)):
        assert L.yk_mask_apply_f32(args[0], args[1], C.c_longlong(args[2]), _st()) == YK_ERR_ARG and b'yk_mask_apply_f32' in L.yk_last_error(), args
        torch.cuda.synchronize()
        assert p.cpu().numpy().view(U).tobytes() == wu.tobytes(), args
