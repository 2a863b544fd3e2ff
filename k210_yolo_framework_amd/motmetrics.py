"""Scores of a multi-object tracker - HOTA, CLEAR-MOT and identity - and the linear assignment they rest on: the statement
of the rule that yk_lap_f64 (csrc/yk_mot.hip) is held to, and what `make trackeval` computes.

numpy, float64, no scipy; nothing here touches a GPU.  HOTA, CLEAR and Identity are restated from the TrackEval public source
  J. Luiten, A. Osep, P. Dendorfer, P. Torr, A. Geiger, L. Leal-Taixe, B. Leibe: "HOTA: A Higher Order Metric for Evaluating Multi-Object
  Tracking", IJCV 2021;  K. Bernardin, R. Stiefelhagen: "Evaluating Multiple Object Tracking Performance: The CLEAR MOT Metrics", 2008;
  E. Ristani et al.: "Performance Measures and a Data Set for Multi-Target, Multi-Camera Tracking", ECCV 2016 workshops
from memory.  PARITY UNPINNED: neither TrackEval nor py-motmetrics is on hand, so no number here is held to theirs; MOTChallenge's
preprocessing (distractor classes, visibility) is NOT applied - the one thing kept of it is that a ground-truth row whose 7th column is 0
is dropped; and no annotated real sequence has been scored.  Scoring is class-agnostic: the tracks file (track.mot_lines) carries no class.

lap(cost): rectangular minimum-cost assignment by shortest augmenting paths with dual variables u (rows) and v (columns), the
Jonker-Volgenant algorithm in D. Crouse's form ("On implementing 2D rectangular assignment algorithms", IEEE TAES 2016).  With more rows
than columns the transpose is solved.  Rows are augmented in ascending order.  For row `cur`: dist = inf and pred = -1 for every column,
none scanned, minval = 0, i = cur; then, until a free column is reached:
    every unscanned column j, in ascending order:  r = ((minval + c[i, j]) - u[i]) - v[j];  if r < dist[j]: dist[j] = r, pred[j] = i
    j = the FIRST argmin of dist among the unscanned columns;  minval = dist[j];  j is scanned;
    if j is free it is the sink, else i = the row that holds j
then u[cur] = u[cur] + minval; for every scanned column j: t = minval - dist[j], v[j] = v[j] - t and, unless j is the sink, u[row of j] =
u[row of j] + t; and the path is flipped back from the sink along pred.  Every operation is one float64 rounding in the order written, so a
kernel can be held to the result assignment for assignment.  (scipy's solver prefers a free column among equal minima; this rule does not,
so the two may pick different optimal assignments on ties - their totals agree.)  Every entry must be finite: forbidden pairs carry the
identity score's 1e10; NaN or inf is refused by name.

A sequence is two tables [frame, id, left, top, width, height], ground truth and result.  Frames count from 1; ids are arbitrary integers,
mapped to dense indices in order of first appearance (rows sorted by frame, stably).  Refused by name: an id twice in one frame, a
non-finite number, a side that is not positive, a frame below 1.  S is the IoU in float64 of two (left, top, width, height) rectangles,
0 where the union is not positive; eps = np.finfo(float).eps.  The formulas are the docstrings of hota, clear and identity below."""
from __future__ import annotations

from pathlib import Path
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

ALPHAS = np.arange(1, 20) * 0.05          # 0.05, 0.10 .. 0.95
EPS = np.finfo(float).eps
FORBIDDEN = 1e10
HOTA_FIELDS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')
INT_FIELDS = ('CLR_TP', 'CLR_FN', 'CLR_FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'IDFN', 'IDFP', 'GT_IDs', 'RES_IDs', 'Frames')


def lap(cost) -> np.ndarray:
    """cost [rows, cols] float64, finite -> int64 [rows]: the column of every row, or -1 (more rows than columns)."""
    c = np.asarray(cost, np.float64)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError(f'lap: cost of shape {c.shape}: expected [rows >= 1, cols >= 1]')
    if not np.isfinite(c).all():
        raise ValueError('lap: cost has a NaN or an infinity; a forbidden pair carries 1e10')
    tall = c.shape[0] > c.shape[1]
    if tall:
        c = c.T
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    for cur in range(nr):
        dist, pred, scanned = np.full(nc, np.inf), np.full(nc, -1, np.int64), np.zeros(nc, bool)
        minval, i, sink = 0.0, cur, -1
        while sink < 0:
            open_ = np.flatnonzero(~scanned)
            r = ((minval + c[i, open_]) - u[i]) - v[open_]
            better = r < dist[open_]
            dist[open_[better]], pred[open_[better]] = r[better], i
            j = int(open_[np.argmin(dist[open_])])
            minval = dist[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] = u[cur] + minval
        for j in np.flatnonzero(scanned):
            t = minval - dist[j]
            v[j] = v[j] - t
            if j != sink:
                u[row4col[j]] = u[row4col[j]] + t
        j = sink
        while True:
            i = int(pred[j])
            row4col[j] = i
            j, col4row[i] = int(col4row[i]), j
            if i == cur:
                break
    return row4col if tall else col4row


# ---- input ------------------------------------------------------------------------------------------------------------------------------

def load_mot_text(path, ground_truth: bool = False) -> np.ndarray:
    """MOTChallenge text (frame,id,left,top,width,height,...: what track.mot_lines writes) -> float64 [n, 6].  ground_truth: a row whose
    7th column is 0 is dropped; nothing else of MOTChallenge's preprocessing is applied."""
    rows = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        if not line.strip():
            continue
        try:
            f = [float(x) for x in line.replace(',', ' ').split()]
        except ValueError:
            raise ValueError(f'{path}:{n}: {line.strip()!r} is not a row of numbers') from None
        if len(f) < 6:
            raise ValueError(f'{path}:{n}: {len(f)} columns, a row has frame, id, left, top, width, height')
        if ground_truth and len(f) > 6 and f[6] == 0:
            continue
        rows.append(f[:6])
    return np.asarray(rows, np.float64).reshape(-1, 6)


def _table(name: str, side: str, t) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """-> (frame [n] int from 1, dense id [n], box [n, 4]) sorted by frame, and the number of ids"""
    t = np.asarray(t, np.float64).reshape(-1, 6)
    if not np.isfinite(t).all():
        raise ValueError(f'{name}: {side} row {int(np.flatnonzero(~np.isfinite(t).all(1))[0])} has a non-finite number')
    if (t[:, 4:6] <= 0).any():
        raise ValueError(f'{name}: {side} row {int(np.flatnonzero((t[:, 4:6] <= 0).any(1))[0])} has a side that is not positive')
    if (t[:, 0] < 1).any() or (t[:, :2] != np.floor(t[:, :2])).any():
        raise ValueError(f'{name}: {side} frames are whole numbers from 1 and ids whole numbers')
    t = t[np.argsort(t[:, 0], kind='stable')]
    ids, first, dense = t[:, 1].astype(np.int64), {}, np.zeros(len(t), np.int64)
    for k, i in enumerate(ids):
        dense[k] = first.setdefault(int(i), len(first))
    frame = t[:, 0].astype(np.int64)
    pair = frame * (len(first) + 1) + dense
    if len(np.unique(pair)) != len(pair):
        k = int(np.flatnonzero(np.diff(np.sort(pair)) == 0)[0])
        raise ValueError(f'{name}: {side} id appears twice in frame {int(np.sort(pair)[k] // (len(first) + 1))}')
    return frame, dense, t[:, 2:6], len(first)


def prepare(name: str, gt, res) -> dict:
    """The checked sequence: G, T, n_frames and per frame (gids, tids, S [G_t, T_t])."""
    gf, gi, gb, G = _table(name, 'ground-truth', gt)
    tf, ti, tb, T = _table(name, 'result', res)
    n_frames = int(max(gf.max(initial=0), tf.max(initial=0)))
    g0, t0 = np.searchsorted(gf, np.arange(1, n_frames + 2)), np.searchsorted(tf, np.arange(1, n_frames + 2))
    frames = []
    for f in range(n_frames):
        a, b = slice(g0[f], g0[f + 1]), slice(t0[f], t0[f + 1])
        frames.append((gi[a], ti[b], iou_ltwh(gb[a], tb[b])))
    return dict(name=name, G=G, T=T, n_frames=n_frames, frames=frames)


def iou_ltwh(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a [n, 4], b [m, 4] (left, top, width, height) -> S [n, m]: inter / ((area_a + area_b) - inter), 0 where the union is not positive."""
    a, b = np.asarray(a, np.float64).reshape(-1, 1, 4), np.asarray(b, np.float64).reshape(1, -1, 4)
    iw = np.maximum(np.minimum(a[..., 0] + a[..., 2], b[..., 0] + b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0.0)
    ih = np.maximum(np.minimum(a[..., 1] + a[..., 3], b[..., 1] + b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0.0)
    inter = iw * ih
    union = (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3]) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


# ---- the three scores of one prepared sequence ------------------------------------------------------------------------------------------

def hota(seq: dict, solver: Callable = lap) -> dict:
    """Per frame: denom = rowsum[:, None] + colsum[None, :] - S (both sums in ascending order, one addition after the other); pmc[g, t] += S / denom where denom > eps; gcount[g] += 1, tcount[t] += 1.
    gas = pmc / (gcount[:, None] + tcount[None, :] - pmc).  Per frame again: no ground truth FP[a] += T_t; no results FN[a] += G_t;
    otherwise solver(-(gas[gids, tids] * S)) and per alpha a pair counts when S >= alpha - eps: TP += n, FN += G_t - n, FP += T_t - n,
    Loc += sum S, mc[a][g, t] += 1.  Per alpha: A = mc / max(1, gcount + tcount - mc), AssA = sum mc A / max(1, TP), AssRe = sum mc mc /
    max(1, gcount) / max(1, TP), AssPr with tcount, DetA = TP / max(1, TP + FN + FP), DetRe = TP / max(1, TP + FN), DetPr = TP / max(1,
    TP + FP), LocA = max(1e-10, Loc) / max(1e-10, TP), HOTA = sqrt(DetA AssA)."""
    G, T, A = seq['G'], seq['T'], len(ALPHAS)
    pmc, gcount, tcount = np.zeros((G, T)), np.zeros(G), np.zeros(T)
    for gids, tids, S in seq['frames']:
        if len(gids) and len(tids):
            denom = np.cumsum(S, 1)[:, -1][:, None] + np.cumsum(S, 0)[-1][None, :] - S      # (the sums in ascending order, one addition after the other)
            ok = denom > EPS
            pmc[gids[:, None], tids[None, :]] += np.where(ok, S / np.where(ok, denom, 1.0), 0.0)
        gcount[gids] += 1
        tcount[tids] += 1
    gas = pmc / (gcount[:, None] + tcount[None, :] - pmc)         # (every id was seen once and pmc <= both counts: never 0 below)
    TP, FN, FP = (np.zeros(A, np.int64) for _ in range(3))
    loc, mc = np.zeros(A), np.zeros((A, G, T), np.int64)
    for gids, tids, S in seq['frames']:
        if not len(gids):
            FP += len(tids)
        elif not len(tids):
            FN += len(gids)
        else:
            col = np.asarray(solver(-(gas[gids[:, None], tids[None, :]] * S)))
            rows = np.flatnonzero(col >= 0)
            s = S[rows, col[rows]]
            for a, alpha in enumerate(ALPHAS):
                hit = s >= alpha - EPS
                n = int(hit.sum())
                TP[a], FN[a], FP[a] = TP[a] + n, FN[a] + len(gids) - n, FP[a] + len(tids) - n
                loc[a] += s[hit].sum()
                mc[a, gids[rows[hit]], tids[col[rows[hit]]]] += 1
    out = dict(HOTA_TP=TP, HOTA_FN=FN, HOTA_FP=FP, Loc=loc, MC=mc.reshape(A, -1).sum(1))
    tp1 = np.maximum(1, TP)
    both = gcount[:, None] + tcount[None, :]
    out['AssA'] = np.array([(mc[a] * (mc[a] / np.maximum(1, both - mc[a]))).sum() for a in range(A)]) / tp1
    out['AssRe'] = np.array([(mc[a] * (mc[a] / np.maximum(1, gcount[:, None]))).sum() for a in range(A)]) / tp1
    out['AssPr'] = np.array([(mc[a] * (mc[a] / np.maximum(1, tcount[None, :]))).sum() for a in range(A)]) / tp1
    return _hota_final(out)


def _hota_final(out: dict) -> dict:
    TP, FN, FP = out['HOTA_TP'], out['HOTA_FN'], out['HOTA_FP']
    out['DetA'], out['DetRe'], out['DetPr'] = TP / np.maximum(1, TP + FN + FP), TP / np.maximum(1, TP + FN), TP / np.maximum(1, TP + FP)
    out['LocA'] = np.maximum(1e-10, out['Loc']) / np.maximum(1e-10, TP)
    out['HOTA'] = np.sqrt(out['DetA'] * out['AssA'])
    return out


def clear(seq: dict, solver: Callable = lap) -> dict:
    """Threshold 0.5.  Per ground-truth id: prev (the last result id ever matched) and prev_t (matched in the previous frame, else none).
    Per frame: no ground truth FP += T_t; no results FN += G_t and the ids present count a frame as seen (prev_t stays); otherwise score
    = 1000 [tid == prev_t[g]] + S, 0 where S < 0.5 - eps, solver(-score), a pair counts when its score > eps; IDSW counts matched ids whose
    prev exists and differs; a fragment starts where an id is matched and prev_t was none; then prev, prev_t (this frame's matches only),
    seen and matched.  MOTA = (TP - FP - IDSW) / max(1, TP + FN), MOTP = sum S / max(1, TP); matched / seen > 0.8 MT, >= 0.2 PT, else ML;
    Frag = sum (fragments - 1) over ids with a fragment."""
    G = seq['G']
    prev, prev_t = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    seen, matched, frags = (np.zeros(G, np.int64) for _ in range(3))
    TP = FN = FP = IDSW = 0
    motp = 0.0
    for gids, tids, S in seq['frames']:
        if not len(gids):
            FP += len(tids)
            continue
        seen[gids] += 1
        if not len(tids):
            FN += len(gids)
            continue
        score = 1000.0 * (tids[None, :] == prev_t[gids][:, None]) + S
        score[S < 0.5 - EPS] = 0.0
        col = np.asarray(solver(-score))
        rows = np.flatnonzero(col >= 0)
        rows = rows[score[rows, col[rows]] > EPS]
        g, t = gids[rows], tids[col[rows]]
        IDSW += int(((prev[g] >= 0) & (prev[g] != t)).sum())
        frags[g[prev_t[g] < 0]] += 1
        prev[g] = t
        prev_t[:] = -1
        prev_t[g] = t
        matched[g] += 1
        TP, FN, FP = TP + len(g), FN + len(gids) - len(g), FP + len(tids) - len(g)
        motp += S[rows, col[rows]].sum()
    ratio = matched / np.maximum(1, seen)
    mt, pt = int((ratio > 0.8).sum()), int(((ratio >= 0.2) & ~(ratio > 0.8)).sum())
    return _clear_final(dict(CLR_TP=TP, CLR_FN=FN, CLR_FP=FP, IDSW=IDSW, MT=mt, PT=pt, ML=G - mt - pt,
                             Frag=int((frags[frags > 0] - 1).sum()), MOTPsum=motp))


def _clear_final(out: dict) -> dict:
    out['MOTA'] = (out['CLR_TP'] - out['CLR_FP'] - out['IDSW']) / max(1, out['CLR_TP'] + out['CLR_FN'])
    out['MOTP'] = out['MOTPsum'] / max(1, out['CLR_TP'])
    return out


def identity_costs(seq: dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> fn, fp [(G + T), (G + T)] and gcount: pm[g, t] counts the frames with S >= 0.5; fn is gcount[g] along ground-truth row g and at
    its own dummy column T + g, 1e10 at the other dummy columns; fp is tcount[t] down result column t and at its own dummy row G + t, 1e10
    at the other dummy rows; both minus pm in the real block; 0 elsewhere."""
    G, T = seq['G'], seq['T']
    pm, gcount, tcount = np.zeros((G, T)), np.zeros(G), np.zeros(T)
    for gids, tids, S in seq['frames']:
        pm[gids[:, None], tids[None, :]] += S >= 0.5
        gcount[gids] += 1
        tcount[tids] += 1
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fn[:G, T:], fp[G:, :T] = FORBIDDEN, FORBIDDEN
    fn[:G, :T], fp[:G, :T] = gcount[:, None] - pm, tcount[None, :] - pm
    fn[np.arange(G), T + np.arange(G)] = gcount
    fp[G + np.arange(T), np.arange(T)] = tcount
    return fn, fp, gcount


def identity(seq: dict, solver: Callable = lap) -> dict:
    """One solver(fn + fp) of identity_costs (every cost an integer below 2^53): IDFN = sum fn and IDFP = sum fp of the matches, IDTP =
    sum gcount - IDFN, IDF1 = IDTP / max(1, IDTP + (IDFN + IDFP) / 2), IDR = IDTP / max(1, IDTP + IDFN), IDP = IDTP / max(1, IDTP + IDFP)."""
    fn, fp, gcount = identity_costs(seq)
    out = dict(IDTP=0, IDFN=0, IDFP=0)
    if len(fn):
        col = np.asarray(solver(fn + fp))
        rows = np.arange(len(fn))
        out['IDFN'], out['IDFP'] = int(fn[rows, col].sum()), int(fp[rows, col].sum())
        out['IDTP'] = int(gcount.sum()) - out['IDFN']
    return _identity_final(out)


def _identity_final(out: dict) -> dict:
    tp, fn, fp = out['IDTP'], out['IDFN'], out['IDFP']
    out['IDF1'], out['IDR'], out['IDP'] = tp / max(1, tp + (fn + fp) / 2), tp / max(1, tp + fn), tp / max(1, tp + fp)
    return out


# ---- whole runs -------------------------------------------------------------------------------------------------------------------------

def summarise(m: dict) -> dict:
    """Adds the means over the alphas under the plain names; the per-alpha arrays move to <name>_alpha."""
    for k in HOTA_FIELDS:
        m[k + '_alpha'] = m[k]
        m[k] = float(np.mean(m[k]))
    return m


def combine(per_seq: Sequence[dict]) -> dict:
    """Several sequences: the integer counts and the sums add; AssA, AssRe, AssPr and LocA per alpha are the TP-weighted means (over
    max(1, sum TP)); the rest follows from the sums."""
    A = len(ALPHAS)
    out = {k: sum((m[k] for m in per_seq), np.zeros(A, np.int64)) for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'MC')}
    out['Loc'] = sum((m['Loc'] for m in per_seq), np.zeros(A))
    for k in ('AssA', 'AssRe', 'AssPr', 'LocA'):
        out[k] = sum((m[k + '_alpha'] * m['HOTA_TP'] for m in per_seq), np.zeros(A)) / np.maximum(1, out['HOTA_TP'])
    loc_a = out['LocA']
    _hota_final(out)
    out['LocA'] = loc_a
    for k in INT_FIELDS:
        out[k] = sum(int(m[k]) for m in per_seq)
    out['MOTPsum'] = sum((m['MOTPsum'] for m in per_seq), 0.0)
    return summarise(_identity_final(_clear_final(out)))


def evaluate(sequences, solver: Callable = lap) -> dict:
    """sequences: (name, gt, res) each, the tables [n, 6] -> {'sequences': {name: scores}, 'combined': scores}."""
    per = {}
    for name, gt, res in sequences:
        if name in per:
            raise ValueError(f'sequence {name!r} appears twice')
        seq = prepare(name, gt, res)
        m = dict(hota(seq, solver), **clear(seq, solver), **identity(seq, solver))
        m.update(GT_IDs=seq['G'], RES_IDs=seq['T'], Frames=seq['n_frames'])
        per[name] = summarise(m)
    return dict(sequences=per, combined=combine(list(per.values())))


def line(name: str, m: dict) -> str:
    """The line `make trackeval` prints for one sequence or for COMBINED."""
    return (f"{name:<16s} HOTA {100 * m['HOTA']:6.2f}  DetA {100 * m['DetA']:6.2f}  AssA {100 * m['AssA']:6.2f}  LocA {100 * m['LocA']:6.2f}  "
            f"MOTA {100 * m['MOTA']:7.2f}  MOTP {100 * m['MOTP']:6.2f}  IDF1 {100 * m['IDF1']:6.2f}  IDSW {m['IDSW']:5d}  Frag {m['Frag']:5d}  "
            f"MT/PT/ML {m['MT']}/{m['PT']}/{m['ML']}")


def synthetic_sequences(n_seq: int, n_frames: int, n_objects: int, seed: int, jitter: float = 0.04, miss: float = 0.1, extra: float = 0.3,
                        swap: bool = True, split: bool = True, size: Tuple[int, int] = (320, 224)) -> List[Tuple[str, np.ndarray, np.ndarray]]:
    """Generated sequences, no pictures and no network: n_objects rectangles (20 .. 60 pixels a side) on straight paths across a `size`
    field, each present over a span of frames of its own (they enter and leave).  The result table is the ground truth perturbed by
    np.random.default_rng(seed), in this order: every side and corner moved by a normal of sigma jitter * the side (box jitter); each row
    dropped with probability `miss` (missed frames); per frame a Poisson(extra) number of boxes with fresh ids (extra boxes); with `swap`
    the first two objects exchange ids from the middle frame on; with `split` the last object takes a fresh id from the middle frame on.
    -> (name, gt [n, 6], res [m, 6]) per sequence."""
    if min(n_seq, n_frames, n_objects) < 1:
        raise ValueError(f'synthetic_sequences: n_seq {n_seq}, n_frames {n_frames}, n_objects {n_objects}: each at least 1')
    rng, out = np.random.default_rng(seed), []
    W, H = size
    for s in range(n_seq):
        gt = []
        for o in range(n_objects):
            a = int(rng.integers(1, max(2, n_frames // 3 + 1)))
            b = int(rng.integers(max(a, 2 * n_frames // 3), n_frames + 1))
            w, h = rng.uniform(20, 60, 2)
            p0, p1 = rng.uniform(0, [W - w, H - h], (2, 2))
            for f in range(a, b + 1):
                x, y = p0 + (p1 - p0) * ((f - a) / max(1, b - a))
                gt.append([f, o + 1, x, y, w, h])
        gt = np.asarray(gt, np.float64)
        res = gt.copy()
        res[:, 2:4] += rng.normal(0, jitter, (len(gt), 2)) * gt[:, 4:6]
        res[:, 4:6] *= np.maximum(0.5, 1 + rng.normal(0, jitter, (len(gt), 2)))
        late = res[:, 0] > n_frames // 2
        if swap and n_objects >= 2:
            one, two = late & (gt[:, 1] == 1), late & (gt[:, 1] == 2)
            res[one, 1], res[two, 1] = 2, 1
        if split:
            res[late & (gt[:, 1] == n_objects), 1] = n_objects + 1
        res = res[rng.random(len(res)) >= miss]
        clutter, next_id = [], n_objects + 2
        for f in range(1, n_frames + 1):
            for _ in range(int(rng.poisson(extra))):
                w, h = rng.uniform(20, 60, 2)
                clutter.append([f, next_id, rng.uniform(0, W - w), rng.uniform(0, H - h), w, h])
                next_id += 1
        out.append((f'synthetic-{s:02d}', gt, np.concatenate([res, np.asarray(clutter, np.float64).reshape(-1, 6)])))
    return out
