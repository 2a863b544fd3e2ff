"""The cases of tests/fold_cases.py checked on their own (no GPU): the tile sizes and fold strides are the ones the sources state, every size
gives the number of partials and the ragged end it is named for, every k-means case keeps its assignments clear of the last bits of a distance
and all of its clusters, the second statement of the k-means rule agrees with datatools.run_kmeans, and in the plain sumsq inputs every
single tile outweighs the bound by six orders of magnitude - so a fold that drops one partial cannot pass."""
import numpy as np
import pytest

from k210_yolo_framework_amd import datatools
from tests import fold_cases as fc
from tests import optim_cases as oc
from tests.test_gpu_anchor_kmeans import MIN_GAP


def test_the_tiles_and_strides_are_the_ones_the_sources_state():
    km, opt = (fc.CSRC / 'yk_kmeans.hip').read_text(), (fc.CSRC / 'yk_optim.hip').read_text()
    assert (fc.KM_THREADS, fc.KM_BOXES, fc.KM_LANES, fc.KM_TILE) == (256, 2, 64, 512)
    assert (fc.SUMSQ_TILE, fc.SUMSQ_THREADS) == (4096, 256) and fc.SUMSQ_TILE == oc.SUMSQ_TILE
    assert '#define YK_KMEANS_TILE (YK_KMEANS_THREADS * YK_KMEANS_BOXES)' in km
    assert km.count('for (long long t = lane; t < tiles; t += YK_WAVE)') == 3         # two in km_update_kernel, one in km_score_kernel
    assert 'for (size_t i = threadIdx.x; i < n_partial; i += YK_SUMSQ_THREADS)' in opt
    assert fc.MIN_GAP == MIN_GAP == 1e-9


def test_every_size_gives_the_trips_and_the_ragged_end_it_is_named_for():
    assert fc.KM_NS == (32768, 32769, 65539) and fc.SS_NS == (1048576, 1048577, 2097153)
    assert [fc.tiles(n, fc.KM_TILE) for n in fc.KM_NS] == [64, 65, 129] == [fc.KM_LANES, fc.KM_LANES + 1, 2 * fc.KM_LANES + 1]
    assert [n - (fc.tiles(n, fc.KM_TILE) - 1) * fc.KM_TILE for n in fc.KM_NS] == [fc.KM_TILE, 1, 3]          # boxes of the last tile
    assert [fc.tiles(n, fc.SUMSQ_TILE) for n in fc.SS_NS] == [256, 257, 513] == [fc.SUMSQ_THREADS, fc.SUMSQ_THREADS + 1, 2 * fc.SUMSQ_THREADS + 1]
    assert [n - (fc.tiles(n, fc.SUMSQ_TILE) - 1) * fc.SUMSQ_TILE for n in fc.SS_NS] == [fc.SUMSQ_TILE, 1, 1]
    assert fc.KM_CASES == tuple((n, k) for n in fc.KM_NS for k in (6, 32)) and set(fc.KM_SEEDS) == set(fc.KM_CASES)
    assert (fc.KM_R, fc.KM_ITERS) == (2, 3) and (fc.KM_TWIN_N, fc.KM_TWIN_K) == (fc.KM_NS[1], 6)
    n = fc.SS_ONE_HOT_N
    assert n == fc.SS_NS[-1] and sorted(fc.SS_ONE_HOT) == [0, 255, 256, 257, 511, 512]
    for t, j in fc.SS_ONE_HOT.items():
        x = fc.ss_one_hot(t)
        (at,) = np.flatnonzero(x)
        assert at == t * fc.SUMSQ_TILE + j and at // fc.SUMSQ_TILE == t and x[at] == 3.0 and x.dtype == np.float32 and len(x) == n
        assert (fc.ss_thread(j) != 0) == (t != 512) and (at == n - 1) == (t == 512)
    assert len({fc.ss_thread(j) // 64 for j in fc.SS_ONE_HOT.values()}) >= 3           # and the threads sit in different waves


def test_the_starts_are_drawn_as_anchor_inits_draws_them():
    for k, seed in ((6, 0), (32, 2)):
        assert fc.km_starts(k, fc.KM_R, seed).tobytes() == datatools.anchor_inits(k, fc.KM_R, True, seed=seed).tobytes()


@pytest.mark.parametrize('n,k', fc.KM_CASES)
def test_kmeans_cases_are_clear_of_ties_and_empty_clusters_and_both_statements_agree(n, k):
    """A condition, not a measurement: the smallest gap between the best and the second-best distance is at least MIN_GAP and no start loses
    a cluster (fold_cases.KM_SEEDS records the seed that meets both).  Then datatools.run_kmeans against the second statement: the same
    assignments, centroids within the reordering error of a float64 mean - before either judges a kernel."""
    c = fc.km_case(n, k)
    x, inits, want = c['x'], c['inits'], c['want']
    assert x.shape == (n, 2) and inits.shape == (fc.KM_R, k, 2) and c['iters'] == fc.KM_ITERS
    print(f'n {n} k {k} seed {fc.KM_SEEDS[n, k]}: gap {want["gap"]:.3g}, smallest cluster {int(want["counts"].min())}')
    assert want['gap'] >= MIN_GAP, want['gaps']
    assert not want['empty'].any() and want['counts'].min() > 0 and (want['counts'].sum(axis=1) == n).all()
    assert not np.isnan(want['c']).any() and ((want['score'] > 0) & (want['score'] <= 1)).all()
    tol = (n - 1) * 2.0 ** -53
    for r in range(fc.KM_R):
        got_c, got_idx = datatools.run_kmeans(x, inits[r], fc.KM_ITERS)
        assert np.array_equal(got_idx, want['idx'][r])
        assert (np.abs(got_c - want['c'][r]) <= tol * np.maximum(1, np.abs(want['c'][r]))).all()
        assert abs(datatools.mean_best_iou(x, got_c) - want['score'][r]) <= tol
    # the two IoU formulas give the same distances (halving is exact), so the agreement above is not luck
    assert np.array_equal(1 - fc.km_iou(x[:4099], inits[0]), datatools.fake_iou_distance(x[:4099], inits[0]))


def test_the_twin_start_loses_cluster_2_at_once_and_its_neighbours_are_the_plain_case():
    c, plain = fc.km_twin_case(), fc.km_case(fc.KM_TWIN_N, fc.KM_TWIN_K)
    x, inits, want = c['x'], c['inits'], c['want']
    n = len(x)
    assert inits.shape == (3, 6, 2) and np.array_equal(inits[1, 2], inits[1, 0]) and np.array_equal(inits[[0, 2]], plain['inits'])
    assert want['empty'].tolist() == [0, 1, 0] and np.isnan(want['score'][1])
    assert np.isnan(want['c'][1, 2]).all() and not np.isnan(np.delete(want['c'][1], 2, axis=0)).any()
    assert want['counts'][1, 2] == 0 and want['counts'][1].sum() == n and want['gaps'][1] == 0.0         # the tie is exact, index 0 takes it
    for key in ('c', 'idx', 'counts', 'score'):
        assert want[key][[0, 2]].tobytes() == plain['want'][key].tobytes()
    # among the five distinct centroids of the twin start no assignment hangs on the last bits either
    two = np.partition(1 - fc.km_iou(x, np.delete(inits[1], 2, axis=0)), 1, axis=1)
    assert (two[:, 1] - two[:, 0]).min() >= MIN_GAP
    ref_c, ref_idx = datatools.run_kmeans(x, inits[1], 1)
    assert np.array_equal(ref_idx, want['idx'][1]) and np.array_equal(np.isnan(ref_c), np.isnan(want['c'][1]))
    assert np.nanmax(np.abs(ref_c - want['c'][1])) <= (n - 1) * 2.0 ** -53


@pytest.mark.parametrize('n', fc.SS_NS)
def test_every_tile_of_the_plain_sumsq_values_outweighs_the_bound(n):
    """min over the tiles of fsum(x^2 of the tile) >= 1e6 * n 2^-53 fsum(x^2): a result that lacks any one partial is a million bounds away.
    optim_cases.sumsq_problem does not meet this: its +-1e25 put 1e50 into the total, below whose half ulp every tile without one vanishes."""
    pr = fc.ss_problem(n)
    x, ref = pr['x'], pr['ref']
    sums = fc.ss_tile_sums(x)
    bound = oc.sumsq_bound(n, ref)
    print(f'n {n}: {len(sums)} tiles, smallest tile {min(sums):.6g}, bound {bound:.3g}, ratio {min(sums) / bound:.3g}')
    assert len(x) == n and x.dtype == np.float32 and len(sums) == fc.tiles(n, fc.SUMSQ_TILE)
    assert np.abs(x).max() <= fc.SS_LONE and (x == 0).any()                            # plain values: nothing near 1e25
    assert min(sums) >= fc.SS_VISIBLE * bound
    assert abs(sum(sums) - ref) <= bound
    if n % fc.SUMSQ_TILE == 1:
        assert x[-1] == fc.SS_LONE and sums[-1] == fc.SS_LONE ** 2


def test_sumsq_problem_hides_whole_tiles_below_its_bound():
    n = oc.NS[-1]
    pr = oc.sumsq_problem(n)
    assert min(fc.ss_tile_sums(pr['x'])) < oc.sumsq_bound(n, pr['ref'])
