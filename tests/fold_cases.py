"""Inputs that make a FOLD OF PER-TILE PARTIALS take a second and a third trip, shared by tests/test_fold_cases.py (CPU: the sizes, the
conditions the cases must meet and the reference side checked on their own) and tests/test_gpu_fold_trips.py (the kernels).  Nothing here
touches a GPU or loads the library.

Two operations leave one partial per tile in a first launch and fold the partials in a second one, in a strided loop:

  csrc/yk_kmeans.hip  km_update_kernel / km_score_kernel   for (t = lane; t < tiles; t += YK_WAVE)               tiles of KM_TILE boxes
  csrc/yk_optim.hip   sumsq_finish_kernel                  for (i = tid; i < n_partial; i += YK_SUMSQ_THREADS)   tiles of SUMSQ_TILE floats

The loop takes a second trip from KM_LANES + 1 = 65 tiles (33 281 boxes) and from SUMSQ_THREADS + 1 = 257 partials (1 048 577 floats) on.
The constants are read out of the sources; tests/test_fold_cases.py compares them with the literals the sizes below were written for.

The k-means rule is stated here a second time, without datatools: float64 numpy for the IoU and the argmin, math.fsum (the correctly rounded
sum) for every mean."""
import functools
import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'k210_yolo_framework_amd' / 'csrc'


def _define(path, name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)\b', path.read_text()).group(1))


KM_THREADS = _define(CSRC / 'yk_kmeans.hip', 'YK_KMEANS_THREADS')
KM_BOXES = _define(CSRC / 'yk_kmeans.hip', 'YK_KMEANS_BOXES')            # per lane
KM_LANES = _define(CSRC / 'yk_common.h', 'YK_WAVE')                      # the stride of both k-means folds
KM_TILE = KM_THREADS * KM_BOXES                                          # YK_KMEANS_TILE
SUMSQ_TILE = _define(ROOT / 'include' / 'yolo_hip.h', 'YK_SUMSQ_TILE')
SUMSQ_THREADS = _define(CSRC / 'yk_optim.hip', 'YK_SUMSQ_THREADS')       # the stride of the sumsq fold


def _frozen(a):
    a.setflags(write=False)
    return a


def tiles(n, tile):
    return (n + tile - 1) // tile


# ---------------------------------------------------------------------------------------------------- 1. anchor k-means
# 64 tiles: the last size with one trip | 65: tile index 64 holds one box, lane 0 alone takes a second trip | 129: a third trip, 3 boxes in it
KM_NS = (KM_LANES * KM_TILE, KM_LANES * KM_TILE + 1, 2 * KM_LANES * KM_TILE + 3)
KM_KS = (6, 32)
KM_R, KM_ITERS = 2, 3                                # the smallest that reach the loops: two starts (r * tiles in every index), three updates
MIN_GAP = 1e-9                                       # tests/test_gpu_anchor_kmeans.py's: no assignment hangs on the last bits of a distance
# (n, k) -> the seed of the boxes and of the starts.  tests/test_fold_cases.py holds every case to: smallest gap >= MIN_GAP, no start
# loses a cluster.  Seeds were tried from 0 upwards.  With k = 32 uniform starts a centroid far from every box is common: seeds 0 and 1 lose
# a cluster in the first update at the two smaller sizes, seed 0 at the largest; the gap was at least 1e-7 at every seed tried.
KM_SEEDS = {(KM_NS[0], 6): 0, (KM_NS[1], 6): 0, (KM_NS[2], 6): 0, (KM_NS[0], 32): 2, (KM_NS[1], 32): 2, (KM_NS[2], 32): 1}
KM_CASES = tuple((n, k) for n in KM_NS for k in KM_KS)
KM_TWIN_N, KM_TWIN_K = KM_NS[1], 6


def km_boxes(n, seed):
    from tests.anchor_boxes import boxes
    return _frozen(boxes(n, seed))


def km_starts(k, R, seed):
    """[R, k, 2] uniform in (0, 1), drawn as datatools.anchor_inits(k, R, is_random=True, seed=seed) draws them: per start the w column,
    then the h column, of one generator."""
    rng = np.random.default_rng(seed)
    return _frozen(np.stack([np.hstack((rng.uniform(0., 1., (k, 1)), rng.uniform(0., 1., (k, 1)))) for _ in range(R)]))


def km_iou(x, c):
    """[n, 2] boxes against [k, 2] centroids, both centred at the origin -> IoU [n, k]."""
    w, h, cw, ch = x[:, 0, None], x[:, 1, None], c[None, :, 0], c[None, :, 1]
    inter = np.minimum(w, cw) * np.minimum(h, ch)
    return inter / (w * h + cw * ch - inter)


def km_statement(x, inits, iters):
    """The rule for every start of inits [R, k, 2] -> dict(c [R, k, 2], idx [R, n], counts [R, k], score [R], empty [R], gaps [R], gap).
    Per iteration: every box goes to the first minimum of 1 - IoU; a centroid is math.fsum of its members divided by their number.  A start
    that loses a cluster at iteration i stops there: empty = i + 1, that centroid row and the score NaN, idx and counts that iteration's.
    score = math.fsum of every box's IoU with its centroid (the returned ones) / n.  gaps: the smallest difference between the best and the
    second-best distance of any box at any iteration of a start (inf for k = 1); gap: the smallest of them."""
    x, inits = np.asarray(x, np.float64), np.asarray(inits, np.float64)
    (R, k, _), n = inits.shape, len(x)
    cs, idxs, counts = np.empty((R, k, 2)), np.empty((R, n), np.int64), np.empty((R, k), np.int64)
    score, empty, gaps = np.full(R, np.nan), np.zeros(R, np.int32), np.full(R, np.inf)
    for r in range(R):
        c = inits[r].copy()
        for it in range(iters):
            d = 1 - km_iou(x, c)
            idx = np.argmin(d, axis=1)
            if k > 1:
                two = np.partition(d, 1, axis=1)
                gaps[r] = min(gaps[r], float((two[:, 1] - two[:, 0]).min()))
            c = np.full((k, 2), np.nan)
            for i in range(k):
                mine = x[idx == i]
                if len(mine):
                    c[i] = math.fsum(mine[:, 0].tolist()) / len(mine), math.fsum(mine[:, 1].tolist()) / len(mine)
            if np.isnan(c).any():
                empty[r] = it + 1
                break
        if not empty[r]:
            score[r] = math.fsum(km_iou(x, c).max(axis=1).tolist()) / n
        cs[r], idxs[r], counts[r] = c, idx, np.bincount(idx, minlength=k)
    return dict(c=_frozen(cs), idx=_frozen(idxs), counts=_frozen(counts), score=_frozen(score), empty=_frozen(empty), gaps=_frozen(gaps),
                gap=float(gaps.min()))


@functools.lru_cache(maxsize=None)
def km_case(n, k):
    """-> dict(x, inits, iters, want): the boxes, the KM_R starts and km_statement of them.  Computed once, never changed."""
    seed = KM_SEEDS[n, k]
    x, inits = km_boxes(n, seed), km_starts(k, KM_R, seed)
    return dict(x=x, inits=inits, iters=KM_ITERS, want=km_statement(x, inits, KM_ITERS))


@functools.lru_cache(maxsize=None)
def km_twin_case():
    """The (KM_TWIN_N, KM_TWIN_K) case with a start between its two whose centroid 2 repeats centroid 0: index 0 takes every tied box, so
    cluster 2 is empty after the first update.  -> dict(x, inits [3, k, 2], iters, want)."""
    c = km_case(KM_TWIN_N, KM_TWIN_K)
    twin = c['inits'][0].copy()
    twin[2] = twin[0]
    inits = _frozen(np.stack([c['inits'][0], twin, c['inits'][1]]))
    return dict(x=c['x'], inits=inits, iters=KM_ITERS, want=km_statement(c['x'], inits, KM_ITERS))


def km_bound(n):
    """A mean of n values in (0, 1] summed in any order is within (n - 1) * 2^-53 of the correctly rounded one; the assignments are exact,
    so the error does not grow over the iterations (the derivation of tests/test_gpu_anchor_kmeans.py's TOL, at this n)."""
    return (n - 1) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------- 2. sum of squares
# 256 partials: the last size with one trip | 257: thread 0 alone takes a second trip, over a tile of one element | 513: a third trip, the same
SS_NS = (SUMSQ_THREADS * SUMSQ_TILE, SUMSQ_THREADS * SUMSQ_TILE + 1, 2 * SUMSQ_THREADS * SUMSQ_TILE + 1)
SS_LONE = 256.0                                      # the element that is a tile of its own (see ss_problem)
SS_VISIBLE = 1e6                                     # every tile's sum of squares is at least this many times optim_cases.sumsq_bound


@functools.lru_cache(maxsize=None)
def ss_problem(n):
    """Plain gradients as tests/optim_cases.gradient_problem draws them (train_cases.adam_gradients: normal x 10^{-4..1}, exact zeros, a
    few +-1e-20; nothing near 1e25) -> dict(x float32 [n], ref = math.fsum of the squares, which are exact in float64).  Where the last
    tile holds one element that element is SS_LONE, whose square is about a full tile's sum: one drawn value cannot outweigh the bound of
    2e6 terms, and the last partial is the one a short fold loses."""
    from tests import train_cases as tc
    x = tc.adam_gradients(np.random.default_rng(4000 + n), n)
    if n % SUMSQ_TILE == 1:
        x[n - 1] = np.float32(SS_LONE)
    sq = x.astype(np.float64) ** 2
    return dict(x=_frozen(x), ref=math.fsum(sq.tolist()))


def ss_tile_sums(x):
    """math.fsum of the squares of every tile of SUMSQ_TILE floats."""
    sq = np.asarray(x, np.float64) ** 2
    return [math.fsum(sq[i:i + SUMSQ_TILE].tolist()) for i in range(0, len(sq), SUMSQ_TILE)]


# One-hot inputs of SS_NS[-1] floats: tile -> element of the tile that holds 3.0; everything else is zero, so the sum is 9.0 whatever the
# order.  Tiles on both sides of the fold's first and second border, the first and the last; sumsq_tile_kernel gives element j of a tile to
# thread (j / 4) % SUMSQ_THREADS, and every j below but the last tile's only one belongs to another thread than 0.
SS_ONE_HOT_N = SS_NS[-1]
SS_ONE_HOT = {0: 150, 255: 4095, 256: 1029, 257: 2310, 511: 2900, 512: 0}
SS_ONE_HOT_VALUE, SS_ONE_HOT_SUM = 3.0, 9.0


def ss_thread(j):
    return (j // 4) % SUMSQ_THREADS


def ss_one_hot(t):
    x = np.zeros(SS_ONE_HOT_N, np.float32)
    x[t * SUMSQ_TILE + SS_ONE_HOT[t]] = SS_ONE_HOT_VALUE
    return x
