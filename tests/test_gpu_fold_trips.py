"""The folds of per-tile partials past their first trip (tests/fold_cases.py; tests/test_fold_cases.py checks the cases on the CPU):
km_update_kernel and km_score_kernel of csrc/yk_kmeans.hip at 64, 65 and 129 tiles against 64 lanes, sumsq_finish_kernel of
csrc/yk_optim.hip at 256, 257 and 513 partials against 256 threads.  The yardsticks are the numpy / math.fsum statements of
tests/fold_cases.py, not the project's own; every element is compared."""
import ctypes as C

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import datatools, engine
from tests import fold_cases as fc
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
GUARD = 64                                           # bytes behind the k-means workspace that no kernel may touch


def _worst(got, want):
    return float(np.nanmax(np.abs(got - want), initial=0))


def _same_bytes(a, b):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or (u.dtype == v.dtype and u.tobytes() == v.tobytes()), k


# ---------------------------------------------------------------------------------------------------- anchor k-means
@pytest.mark.parametrize('n,k', fc.KM_CASES)
def test_kmeans_past_64_tiles_equals_the_independent_statement(n, k):
    c = fc.km_case(n, k)
    x, inits, want = c['x'], c['inits'], c['want']
    got = datatools.run_kmeans_gpu(x, inits, c['iters'], return_counts=True)
    cent, idx, score, empty, counts = got
    assert cent.shape == (fc.KM_R, k, 2) and idx.shape == (fc.KM_R, n) and counts.shape == (fc.KM_R, k)
    bound = fc.km_bound(n)
    print(f'n {n} ({fc.tiles(n, fc.KM_TILE)} tiles) k {k}: gap {want["gap"]:.3g}, max |centroid error| {_worst(cent, want["c"]):.3g}, '
          f'max |score error| {_worst(score, want["score"]):.3g}, bound {bound:.3g}')
    assert not empty.any()
    assert np.array_equal(counts, want['counts']) and (counts.sum(axis=1) == n).all()
    assert np.array_equal(idx, want['idx'])
    assert not np.isnan(cent).any() and not np.isnan(score).any()
    assert _worst(cent, want['c']) <= bound and _worst(score, want['score']) <= bound
    _same_bytes(got, datatools.run_kmeans_gpu(x, inits, c['iters'], return_counts=True))


def test_kmeans_past_64_tiles_does_not_depend_on_a_neighbour_start_that_has_left():
    c = fc.km_twin_case()
    x, inits, want = c['x'], c['inits'], c['want']
    n = len(x)
    got = datatools.run_kmeans_gpu(x, inits, c['iters'], return_counts=True)
    cent, idx, score, empty, counts = got
    assert empty.tolist() == want['empty'].tolist() == [0, 1, 0]
    assert np.array_equal(np.isnan(cent), np.isnan(want['c'])) and np.isnan(cent[1, 2]).all() and np.isnan(cent[1]).sum() == 2
    assert np.array_equal(np.isnan(score), [False, True, False])
    assert np.array_equal(idx, want['idx']) and np.array_equal(counts, want['counts'])                   # the twin's: those of iteration 1
    assert counts[1, 2] == 0 and (counts.sum(axis=1) == n).all()
    bound = fc.km_bound(n)
    print(f'n {n}, twin start: max |centroid error| {_worst(cent, want["c"]):.3g}, max |score error| {_worst(score, want["score"]):.3g}, '
          f'bound {bound:.3g}')
    assert _worst(cent, want['c']) <= bound and _worst(score, want['score']) <= bound
    alone = datatools.run_kmeans_gpu(x, inits[[0, 2]], c['iters'], return_counts=True)
    _same_bytes([a[[0, 2]] for a in got], alone)


def _kmeans_c(x, inits, iters, with_idx=True, in_place=False):
    """yk_anchor_kmeans_f64 itself, on a workspace of exactly the queried size -> (centroids, counts, score, empty, idx or None)."""
    engine.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    (R, k, _), n = inits.shape, len(x)
    need = C.c_size_t()
    engine.call('yk_anchor_kmeans_workspace_bytes', n, k, R, C.byref(need))
    assert need.value == R * fc.tiles(n, fc.KM_TILE) * k * (16 + 4)
    work = torch.full((need.value + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_x, d_init = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(inits)).to(dev)
    d_c = d_init if in_place else torch.full((R, k, 2), -7.0, dtype=torch.float64, device=dev)
    d_counts = torch.full((R, k), -7, dtype=torch.int32, device=dev)
    d_score = torch.full((R,), -7.0, dtype=torch.float64, device=dev)
    d_empty = torch.full((R,), -7, dtype=torch.int32, device=dev)
    d_idx = torch.full((R, n), 0xEE, dtype=torch.uint8, device=dev) if with_idx else None
    engine.call('yk_anchor_kmeans_f64', d_x, n, d_init, k, R, iters, d_c, d_counts, d_score, d_empty, d_idx, work, need.value, engine._stream())
    torch.cuda.synchronize()
    assert bool((work[need.value:] == 0xA5).all()), 'written past the workspace'
    if not in_place:
        assert d_init.cpu().numpy().tobytes() == inits.tobytes()                      # the starts are only read
    return (d_c.cpu().numpy(), d_counts.cpu().numpy(), d_score.cpu().numpy(), d_empty.cpu().numpy(), d_idx.cpu().numpy() if with_idx else None)


def test_kmeans_entry_point_without_an_index_buffer_and_in_place_gives_the_same_bytes():
    c = fc.km_case(fc.KM_NS[1], 6)
    x, inits, want = c['x'], c['inits'], c['want']
    base = _kmeans_c(x, inits, c['iters'])
    assert np.array_equal(base[4], want['idx']) and np.array_equal(base[1], want['counts']) and not base[3].any()
    assert _worst(base[0], want['c']) <= fc.km_bound(len(x)) and _worst(base[2], want['score']) <= fc.km_bound(len(x))
    no_idx = _kmeans_c(x, inits, c['iters'], with_idx=False)
    assert no_idx[4] is None
    _same_bytes(no_idx[:4], base[:4])
    _same_bytes(_kmeans_c(x, inits, c['iters'], in_place=True), base)
    cent, idx, score, empty, counts = datatools.run_kmeans_gpu(x, inits, c['iters'], return_counts=True)
    _same_bytes((cent, counts, score, empty, idx), base)


# ---------------------------------------------------------------------------------------------------- yk_sumsq_f32
def _sumsq(x, n):
    """yk_sumsq_f32 on device tensor x -> the float64 result.  The workspace is exactly yk_sumsq_workspace_bytes, with one more double behind
    it that holds a NaN: a fold that reads one past n_partial returns it."""
    nb = C.c_size_t()
    engine.call('yk_sumsq_workspace_bytes', n, C.byref(nb))
    assert nb.value == 8 * fc.tiles(n, fc.SUMSQ_TILE)
    work = torch.full((nb.value // 8 + 1,), -7.0, dtype=torch.float64, device='cuda')
    work[-1] = float('nan')
    out = torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
    engine.call('yk_sumsq_f32', x, n, work, out, engine._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(work[-1])) and float(out[1]) == -7.0, 'written past the workspace or the result'
    return np.float64(out[0].item())


def _aligned_and_shifted(x):
    """The same values on a 16-byte boundary (sumsq_tile_kernel<true>) and one float behind one (sumsq_tile_kernel<false>)."""
    engine.require_gpu()
    a = torch.from_numpy(np.array(x)).cuda()
    s = torch.cat([torch.zeros(1, device='cuda'), a])[1:]
    assert a.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 4 and s.is_contiguous()
    return a, s


@pytest.mark.parametrize('n', fc.SS_NS)
def test_sumsq_past_256_partials_is_the_float64_sum(n):
    pr = fc.ss_problem(n)
    ref, bound = pr['ref'], oc.sumsq_bound(n, pr['ref'])
    aligned, shifted = _aligned_and_shifted(pr['x'])
    a, a2, s, s2 = _sumsq(aligned, n), _sumsq(aligned, n), _sumsq(shifted, n), _sumsq(shifted, n)
    print(f'sumsq n {n} ({fc.tiles(n, fc.SUMSQ_TILE)} partials): {a!r} reference {ref!r}, |error| {abs(a - ref):.3g} (shifted {abs(s - ref):.3g}), '
          f'bound {bound:.3g}')
    assert np.isfinite(a) and abs(a - ref) <= bound and abs(s - ref) <= bound
    assert a.tobytes() == a2.tobytes() and s.tobytes() == s2.tobytes()
    assert a.tobytes() == s.tobytes()                                                  # who adds what depends on n alone
    assert np.array_equal(aligned.cpu().numpy().view(np.uint32), pr['x'].view(np.uint32))          # only read


@pytest.mark.parametrize('t', sorted(fc.SS_ONE_HOT))
def test_sumsq_reaches_every_partial_exactly_once(t):
    """One 3.0 in tile t of 513, zeros elsewhere: exactly 9.0, no tolerance.  t = 256 | 257 and 512 are partials of the second and third trip."""
    n = fc.SS_ONE_HOT_N
    want = np.float64(fc.SS_ONE_HOT_SUM)
    for x in _aligned_and_shifted(fc.ss_one_hot(t)):
        got = _sumsq(x, n)
        assert got.tobytes() == want.tobytes(), (t, fc.SS_ONE_HOT[t], got)
