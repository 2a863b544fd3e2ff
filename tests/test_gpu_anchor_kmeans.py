"""csrc/yk_kmeans.hip (datatools.run_kmeans_gpu) against datatools.run_kmeans, the float64 numpy statement: the same assignments, centroids
and scores within the reordering error of a float64 mean, for every start of a call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import datatools, engine
from tests.anchor_boxes import boxes, write_ann

pytestmark = pytest.mark.gpu
SEED = 0
# a mean of <= 4099 values in (0, 1] summed in any order differs by at most (n - 1) * 2^-53 = 4.6e-13; assignments are exact, so the
# error does not grow over the iterations
TOL = 1e-12
MIN_GAP = 1e-9


@functools.lru_cache(maxsize=None)
def reference(n, k, R, iters):
    """(x, inits, per start: centroids, idx, counts, score, empty) by numpy, one iteration of run_kmeans at a time, and the smallest gap
    between the best and the second-best distance of any box at any iteration of any start.  Computed once per shape, never changed."""
    x, inits = boxes(n, SEED), datatools.anchor_inits(k, R, False, seed=SEED)
    cs, idxs, counts, score, empty, gap = [], [], [], np.full(R, np.nan), np.zeros(R, np.int32), np.inf
    for r, c in enumerate(inits):
        for it in range(iters):
            d = np.sort(datatools.fake_iou_distance(x, c), axis=1)
            if k > 1:
                gap = min(gap, float((d[:, 1] - d[:, 0]).min()))
            c, idx = datatools.run_kmeans(x, c, 1)
            if np.isnan(c).any():
                empty[r] = it + 1
                break
        if not empty[r]:
            c, idx = datatools.run_kmeans(x, inits[r], iters)                        # the oracle itself, in one call
            score[r] = np.mean(1 - datatools.fake_iou_distance(x, c).min(axis=1))
        cs.append(c), idxs.append(idx), counts.append(np.bincount(idx, minlength=k))
    for a in (x, inits):
        a.setflags(write=False)
    return x, inits, np.stack(cs), np.stack(idxs), np.stack(counts), score, empty, gap


# every n, k, R and iters of the list once, and the corner n = 4099, k = 32, R = 16.  n = 63 | 64 | 65: one wave of one tile and its
# edges; 4099: nine tiles of 512, the last one with 3 boxes
CASES = [(1, 1, 1, 1), (63, 6, 16, 10), (64, 9, 1, 10), (65, 6, 16, 1), (4099, 1, 1, 10), (4099, 6, 16, 10), (4099, 9, 16, 10), (4099, 32, 16, 10)]


@pytest.mark.parametrize('n,k,R,iters', CASES)
def test_every_start_equals_run_kmeans(n, k, R, iters):
    x, inits, want_c, want_idx, want_counts, want_score, want_empty, gap = reference(n, k, R, iters)
    assert gap >= MIN_GAP, gap                                                       # no assignment hangs on the last bit of a distance
    c, idx, score, empty, counts = datatools.run_kmeans_gpu(x, inits, iters, return_counts=True)
    assert c.shape == (R, k, 2) and idx.shape == (R, n) and score.shape == empty.shape == (R,) and counts.shape == (R, k)
    print(f'n {n} k {k} R {R} iters {iters}: gap {gap:.3g}, flagged {int((want_empty != 0).sum())}/{R}, '
          f'max |centroid error| {np.nanmax(np.abs(c - want_c), initial=0):.3g}, max |score error| {np.nanmax(np.abs(score - want_score), initial=0):.3g}')
    assert np.array_equal(empty, want_empty)
    ok = want_empty == 0
    assert np.array_equal(idx[ok], want_idx[ok]) and np.array_equal(counts[ok], want_counts[ok])
    assert np.array_equal(np.isnan(c), np.isnan(want_c)) and np.array_equal(np.isnan(score), ~ok)
    assert np.nanmax(np.abs(c - want_c), initial=0) <= TOL
    assert (np.abs(score[ok] - want_score[ok]) <= TOL).all()
    # a flagged start stops at the iteration that emptied a cluster: its assignment is that iteration's
    assert np.array_equal(idx[~ok], want_idx[~ok]) and np.array_equal(counts[~ok], want_counts[~ok])
    assert (counts.sum(axis=1) == n).all()


def test_a_twin_centroid_empties_its_cluster_and_leaves_the_other_starts_alone():
    x = boxes(600, SEED)
    good = datatools.anchor_inits(3, 2, False, seed=SEED)
    twin = good[0].copy()
    twin[2] = twin[0]                                                                # index 0 takes every tied box
    inits = np.stack([good[0], twin, good[1]])
    c, idx, score, empty, counts = datatools.run_kmeans_gpu(x, inits, 10, return_counts=True)
    assert empty.tolist() == [0, 1, 0] and np.isnan(c[1, 2]).all() and not np.isnan(c[1, :2]).any() and np.isnan(score[1])
    assert counts[1, 2] == 0 and counts[1].sum() == 600 and not (idx[1] == 2).any()
    ref1, ref_idx1 = datatools.run_kmeans(x, twin, 1)
    assert np.isnan(datatools.run_kmeans(x, twin, 10)[0]).any() and np.isnan(ref1[2]).all()
    assert np.array_equal(idx[1], ref_idx1) and np.nanmax(np.abs(c[1] - ref1)) <= TOL
    alone = datatools.run_kmeans_gpu(x, inits[[0, 2]], 10, return_counts=True)
    for got, want in zip((c, idx, score, empty, counts), alone):
        assert got[[0, 2]].tobytes() == want.tobytes()
    for r in (0, 2):
        ref_c, ref_idx = datatools.run_kmeans(x, inits[r], 10)
        assert np.array_equal(idx[r], ref_idx) and np.abs(c[r] - ref_c).max() <= TOL


def test_an_exact_tie_goes_to_the_lowest_index():
    x = np.tile([[0.3, 0.3]], (100, 1))
    inits = np.array([[0.2, 0.4], [0.4, 0.2]])                                       # w and h swapped around a square box: the same distance
    d = datatools.fake_iou_distance(x, inits)
    assert (d[:, 0] == d[:, 1]).all()
    ref_c, ref_idx = datatools.run_kmeans(x, inits, 1)
    assert not ref_idx.any() and np.isnan(ref_c[1]).all()
    c, idx, score, empty, counts = datatools.run_kmeans_gpu(x, inits, 1, return_counts=True)
    assert idx.shape == (1, 100) and not idx.any() and counts.tolist() == [[100, 0]] and empty.tolist() == [1]
    assert np.abs(c[0, 0] - [0.3, 0.3]).max() <= TOL and np.isnan(c[0, 1]).all()


def test_two_calls_give_the_same_bits():
    x, inits = reference(4099, 9, 16, 10)[:2]
    a = datatools.run_kmeans_gpu(x, inits, 10, return_counts=True)
    b = datatools.run_kmeans_gpu(x, inits, 10, return_counts=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_make_anchor_list_on_the_gpu_selects_what_the_cpu_selects(tmp_path, capsys):
    data_dir, x = write_ann(tmp_path)
    inits = datatools.anchor_inits(6, 16, True, seed=SEED)
    cpu, gpu = (datatools.run_kmeans_restarts(x, inits, 10, dev) for dev in ('cpu', 'gpu'))
    assert np.array_equal(cpu[2], gpu[2]) and (cpu[2] == 0).sum() >= 2
    assert datatools.select_anchors(*cpu)[0] == datatools.select_anchors(*gpu)[0]
    want = datatools.make_anchor_list('gen', is_random=True, seed=SEED, data_dir=data_dir, save=False, device='cpu', restarts=16)
    line_cpu = capsys.readouterr().out
    got = datatools.make_anchor_list('gen', is_random=True, seed=SEED, data_dir=data_dir, save=True, device='gpu', restarts=16)
    line_gpu = capsys.readouterr().out
    assert got.shape == (2, 3, 2) and not np.isnan(want).any() and np.abs(got - want).max() <= TOL
    assert line_gpu == line_cpu and 'mean IoU' in line_gpu
    assert np.load(tmp_path / 'data' / 'gen_anchor.npy').tobytes() == got.tobytes()


def _call(n=100, k=3, R=2, iters=1, work_bytes=None):
    """The C entry point on buffers of the sizes it is told (at least one element each), so that only the named argument is wrong."""
    dev = torch.device('cuda', torch.cuda.current_device())
    f64 = lambda *s: torch.ones([max(int(v), 1) for v in s], dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros([max(int(v), 1) for v in s], dtype=torch.int32, device=dev)
    need = C.c_size_t(1 << 20)
    if work_bytes is None:
        engine.call('yk_anchor_kmeans_workspace_bytes', n, k, R, C.byref(need))
    work = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    engine.call('yk_anchor_kmeans_f64', f64(n, 2), n, f64(R, k, 2), k, R, iters, f64(R, k, 2), i32(R, k), f64(R), i32(R), None, work,
                need.value if work_bytes is None else work_bytes, engine._stream())
    torch.cuda.synchronize()


def test_refusals_name_the_argument():
    x = boxes(100, SEED)
    with pytest.raises(engine.YkError, match=r'k = 33: must be in 1 \.\. 32'):
        datatools.run_kmeans_gpu(x, np.full((1, 33, 2), 0.5))
    with pytest.raises(engine.YkError, match=r'restarts = 0: must be in 1 \.\. 4096'):
        _call(R=0)
    with pytest.raises(engine.YkError, match=r'restarts = 4097'):
        _call(R=4097, work_bytes=1 << 20)
    with pytest.raises(engine.YkError, match=r'iters = 1001'):
        _call(iters=1001)
    need = C.c_size_t()
    engine.call('yk_anchor_kmeans_workspace_bytes', 100, 3, 2, C.byref(need))
    assert need.value == 2 * 1 * 3 * (16 + 4)                                        # restarts x tiles x k x (two float64 sums + an int32 count)
    with pytest.raises(engine.YkError, match=rf'work_bytes = {need.value - 1}: {need.value} needed'):
        _call(work_bytes=need.value - 1)
    _call()                                                                          # and with everything in range it runs
    for bad in (0.0, -0.1, np.nan, np.inf):
        y = x.copy()
        y[7, 0] = bad
        with pytest.raises(ValueError, match='x holds a box whose w or h is not finite or not positive'):
            datatools.run_kmeans_gpu(y, datatools.anchor_inits(3, 2))
