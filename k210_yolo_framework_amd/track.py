"""Multi-object tracking across frames: the statement of the rule that yk_track_update (csrc/yk_track.hip) is held to.

The rows the decode leaves per frame get identities that last from frame to frame.  That is ByteTrack,
  Y. Zhang, P. Sun, Y. Jiang, D. Yu, F. Weng, Z. Yuan, P. Luo, W. Liu, X. Wang: "ByteTrack: Multi-Object Tracking by Associating Every
  Detection Box", ECCV 2022,
restated from the paper: a constant-velocity Kalman filter per track (the 8-state filter of SORT), a first association of the tracks with
the high-score boxes, a second association of the tracks still unmatched with the low-score boxes a detector normally throws away.
PARITY UNPINNED: the authors' code is not on hand and no number here is held to it or to TrackEval.  Two deliberate deviations:
  - class-aware.  A track keeps the class of the row that opened it and pairs of different classes never match (ByteTrack is written for
    one class; this detector has twenty).
  - greedy by default, not Hungarian.  In each stage the pair with the largest similarity is taken, then the next (ties: the lowest track
    index, then the lowest row index); it is what embedded ports do, and what every earlier run of this tracker did.  assign='lap' makes
    the optimal assignment ByteTrack makes, by the one solver whose order of operations is stated: motmetrics.lap.
The defaults (track_thresh 0.5, low_thresh 0.1, match_thresh 0.8, track_buffer 30) are ByteTrack's and are starting points, not findings;
its `fuse_score` is an option here too, off by default.
What is pinned: the filter against the dense 8 x 8 filter in float64 and the rule on hand cases (tests/test_track.py), the optimal
association against a brute force (tests/test_track_assign.py), and the kernel against this module, bit for bit (tests/test_gpu_track.py,
tests/test_gpu_track_assign.py).

Similarity.  s of a (track, row) pair is the float32 IoU below; in stage 1 with fuse_score it is float32(IoU * the row's score), one
rounding; stages 2 and 3 are never fused.  The gates read s: s >= 1 - match_thresh in stage 1, s >= 0.5 in stage 2, s >= 0.3 in stage 3;
a NaN meets no gate.  Fusion applies under greedy too: the pair with the largest s is taken, with the same ties.

assign='lap', per stage: for each class c in ascending order that has at least one eligible track and one eligible free row, a cost matrix
over that class only - its rows the eligible tracks of class c in track-index order, its columns the eligible rows of class c in row
order; an allowed pair (gate met) costs float64(1) - float64(s), a forbidden one LAP_FORBIDDEN = 2.0 ** 20; motmetrics.lap solves it
exactly as it is written, its transpose when there are more tracks than rows included; of the assigned pairs the allowed ones are kept
and their rows are taken before the next stage.  Why 2 ** 20: at most 1024 tracks and costs of at most 1 give any sum of allowed costs
below it, so the solver first maximises the number of allowed matches and then minimises their total cost; and a power of two that size
leaves the duals about 2e-10 of resolution, where the scores' 1e10 would leave 2e-6.  This is the "solve, then drop the pairs over the
threshold" form that scipy-based ports of ByteTrack use, not lapjv's `cost_limit` extension (which solves an extended problem and can
pick other pairs); parity with the authors' code stays unpinned.

State per track: id (from 1, ascending in order of opening), class, state (NEW seen once and not confirmed, TRACKED, LOST), the frame of its
last match, its last score, and the filter over (cx, cy, a, h), a = w / h, and their velocities.  Tracks are kept in ascending id order.

The filter.  Initial covariance, process and measurement noise are diagonal and the transition couples a coordinate only with its own
velocity, so the 8 x 8 covariance is four 2 x 2 blocks (pp, pv, vv) for all time: 8 means and 12 covariance entries, no inverse.  With
sp = h / 20 and sv = h / 160 (h the track's current height), all entering as squares:
  open     x = z, v = 0; pp = (2 sp)^2, vv = (10 sv)^2, pv = 0; for a: pp = 1e-2^2, vv = 1e-5^2
  predict  (a LOST track's h velocity is set to 0 first)  qp = sp^2, qv = sv^2 (a: 1e-2^2, 1e-5^2), from h before the step;
           x = x + v; pp = (((pp + pv) + pv) + vv) + qp; pv = pv + vv; vv = vv + qv
  update   r = sp^2 (a: 1e-1^2) from the predicted h; s = pp + r; kp = pp / s; kv = pv / s; y = z - x; x = x + kp * y; v = v + kv * y;
           pp = pp - kp * pp; pv = pv - kp * pv; vv = vv - kv * pv      (pp, pv on the right are the old ones)
A row (top, left, bottom, right) is measured as w = right - left, h = bottom - top, cx = (left + right) * 0.5, cy = (top + bottom) * 0.5,
a = w / h; a mean is a box again by w = a * h, hw = w * 0.5, hh = h * 0.5, (cy - hh, cx - hw, cy + hh, cx + hw).

One frame, in this order (frames count from 1 per sequence):
  0  gmc=True only (camera-motion compensation, gmc.py states how the motion is found): the centre (cx, cy) of every
     track's mean, live or lost, moves by the frame's motion (mx, my), one float32 add each - always, a motion of (0, 0) included.
     Velocities and covariances stay: a translation's linear part is the identity, so BoT-SORT's R P R^T leaves P alone.
  1  predict every track; its box is rebuilt from the predicted mean.
  2  rows: dropped unless the class is exactly one of 0 .. class_num - 1, score >= low_thresh (a NaN is dropped), and 0 < h < inf and
     0 < w < inf.  high: score >= track_thresh; low: the others.
  3  stage 1: TRACKED and LOST tracks x high rows at IoU >= 1 - match_thresh; stage 2: TRACKED tracks still unmatched x low rows at
     IoU >= 0.5; stage 3: NEW tracks x the high rows still free at IoU >= 0.3.  The IoU is softnms.iou_to_all's float32 expression, the
     decode's own, of the predicted box and the row's box.
  4  a matched track is updated with its row and is TRACKED, its last match this frame, its score the row's; an unmatched TRACKED track
     becomes LOST, an unmatched NEW one is deleted, a LOST one whose last match is more than track_buffer frames ago is deleted; the
     survivors are compacted in order.
  5  every still-free high row with score >= track_thresh + 0.1, in row order, opens a track with the next id - NEW, or TRACKED on a
     sequence's first frame.  With max_tracks set, a row that finds the sequence full opens nothing, takes no id and is counted in
     `overflow`.
  6  out: one row per track that is TRACKED with its last match in this frame, ascending id, at most `cap`: the filter's box, the matched
     row's score, the class; and the ids beside them.
Every step is np.float32 with one rounding per operation.  numpy only; nothing here touches a GPU."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from .motmetrics import lap

F = np.float32
NEW, TRACKED, LOST = 0, 1, 2
DEFAULTS = dict(track_thresh=0.5, low_thresh=0.1, match_thresh=0.8, track_buffer=30)
DEFAULT_MAX_TRACKS = 256
MAX_TRACKS = 1024                         # what yk_track_update holds of one sequence in LDS at the most
STAGE2_IOU, STAGE3_IOU, OPEN_MARGIN = 0.5, 0.3, 0.1
ASSIGNS = ('greedy', 'lap')               # YK_TRACK_ASSIGN_GREEDY, YK_TRACK_ASSIGN_LAP
LAP_FORBIDDEN = 2.0 ** 20


def check(track_thresh=0.5, low_thresh=0.1, match_thresh=0.8, track_buffer=30, max_tracks=DEFAULT_MAX_TRACKS, nms: str = 'hard',
          tiles=None, tta=None, assign: str = 'greedy', fuse_score: bool = False) -> dict:
    """The tracker's options, refused by name -> the four options as a dict, and `assign` / `fuse_score` where they are not the defaults."""
    if assign not in ASSIGNS:
        raise ValueError(f'track_assign {assign!r}: expected one of {", ".join(ASSIGNS)}')
    if not isinstance(fuse_score, (bool, np.bool_)):
        raise ValueError(f'track_fuse {fuse_score!r}: expected True or False')
    num = lambda v: isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool) and math.isfinite(v)
    if not (num(track_thresh) and 0.0 < track_thresh <= 1.0):
        raise ValueError(f'track_thresh {track_thresh!r}: expected a number in (0, 1]')
    if not (num(low_thresh) and 0.0 <= low_thresh < track_thresh):
        raise ValueError(f'track_low {low_thresh!r}: expected a number in [0, track_thresh {track_thresh:g})')
    if not (num(match_thresh) and 0.0 < match_thresh <= 1.0):
        raise ValueError(f'track_match {match_thresh!r}: expected a number in (0, 1]')
    if not (isinstance(track_buffer, (int, np.integer)) and not isinstance(track_buffer, bool) and 0 <= track_buffer < 2 ** 31):
        raise ValueError(f'track_buffer {track_buffer!r}: expected a whole number of frames >= 0')
    if max_tracks is not None and not (isinstance(max_tracks, (int, np.integer)) and not isinstance(max_tracks, bool)
                                       and 1 <= max_tracks <= MAX_TRACKS):
        raise ValueError(f'track_max {max_tracks!r}: expected 1 .. {MAX_TRACKS} tracks per sequence')
    if tiles is not None:
        raise ValueError('track with tiles: a sliced picture is not one frame of a sequence here; tracking takes whole pictures')
    if tta is not None:
        raise ValueError('track with tta: the fused scores are not the scores the two thresholds were set for; tracking takes one view')
    if nms != 'hard':
        raise ValueError(f"nms {nms!r} with track: the second association reads undecayed low scores; tracking needs nms 'hard'")
    out = dict(track_thresh=float(track_thresh), low_thresh=float(low_thresh), match_thresh=float(match_thresh), track_buffer=int(track_buffer))
    if assign != 'greedy':
        out['assign'] = assign
    if fuse_score:
        out['fuse_score'] = True
    return out


def add_arguments(p) -> None:
    """The command line of the tracker (keras_detect.py)."""
    p.add_argument('--track', type=str, choices=['True', 'False'], default='False',
                   help='track objects across the frames of a folder (ByteTrack restated, track.py): rows carry ids')
    p.add_argument('--track_thresh', type=float, default=DEFAULTS['track_thresh'], help='rows at or above this score take part in the first association')
    p.add_argument('--track_low', type=float, default=DEFAULTS['low_thresh'], help='rows from this score up to --track_thresh take part in the second')
    p.add_argument('--track_match', type=float, default=DEFAULTS['match_thresh'], help='the first association matches at IoU >= 1 - this')
    p.add_argument('--track_buffer', type=int, default=DEFAULTS['track_buffer'], help='frames a lost track is kept')
    p.add_argument('--track_max', type=int, default=DEFAULT_MAX_TRACKS, help=f'tracks held per sequence (at most {MAX_TRACKS})')
    p.add_argument('--track_assign', type=str, default='greedy',
                   help='greedy: the best pair first; lap: the optimal assignment per stage and class (motmetrics.lap)')
    p.add_argument('--track_fuse', type=str, choices=['True', 'False'], default='False',
                   help="ByteTrack's fuse_score: the first association compares IoU * score instead of IoU")


def parse_arguments(a) -> None:
    """Checks what add_arguments read (ValueError by name) and leaves a.track and a.track_fuse as bools."""
    a.track = a.track == 'True'
    a.track_fuse = a.track_fuse == 'True'
    if a.track:
        check(a.track_thresh, a.track_low, a.track_match, a.track_buffer, a.track_max, getattr(a, 'nms', 'hard'), getattr(a, 'tiles', None),
              getattr(a, 'tta', None), a.track_assign, a.track_fuse)


def run_options(a) -> dict:
    """The keyword arguments detect.run takes, from parsed arguments."""
    return dict(track=a.track, track_thresh=a.track_thresh, track_low=a.track_low, track_match=a.track_match, track_buffer=a.track_buffer,
                track_max=a.track_max, track_assign=a.track_assign, track_fuse=a.track_fuse)


# ---- the filter: the last axis holds the four coordinates; any leading axes are tracks --------------------------------------------------

def _noise(h, dtype, pos, vel):
    """(pos * h / 20)^2 and (vel * h / 160)^2 per coordinate, the constants of `a` in the third place."""
    sp = (h / dtype(20)).astype(dtype)
    sv = (h / dtype(160)).astype(dtype)
    if pos != 1:
        sp = (dtype(pos) * sp).astype(dtype)
    if vel != 1:
        sv = (dtype(vel) * sv).astype(dtype)
    p2, v2 = (sp * sp).astype(dtype), (sv * sv).astype(dtype)
    ap = np.full_like(p2, dtype(1e-2) * dtype(1e-2))
    av = np.full_like(v2, dtype(1e-5) * dtype(1e-5))
    return np.stack([p2, p2, ap, p2], -1), np.stack([v2, v2, av, v2], -1)


def kf_open(z: np.ndarray, dtype=F) -> Tuple[np.ndarray, np.ndarray]:
    """z [..., 4] (cx, cy, a, h) -> mean [..., 8] (x then v), cov [..., 12] (pp then pv then vv)."""
    z = np.asarray(z, dtype)
    pp, vv = _noise(z[..., 3], dtype, 2, 10)
    return np.concatenate([z, np.zeros_like(z)], -1), np.concatenate([pp, np.zeros_like(pp), vv], -1)


def kf_predict(mean: np.ndarray, cov: np.ndarray, dtype=F) -> Tuple[np.ndarray, np.ndarray]:
    x, v = mean[..., :4], mean[..., 4:]
    pp, pv, vv = cov[..., :4], cov[..., 4:8], cov[..., 8:]
    qp, qv = _noise(x[..., 3], dtype, 1, 1)
    npp = (((((pp + pv).astype(dtype) + pv).astype(dtype) + vv).astype(dtype)) + qp).astype(dtype)
    npv = (pv + vv).astype(dtype)
    nvv = (vv + qv).astype(dtype)
    return np.concatenate([(x + v).astype(dtype), v], -1), np.concatenate([npp, npv, nvv], -1)


def kf_update(mean: np.ndarray, cov: np.ndarray, z: np.ndarray, dtype=F) -> Tuple[np.ndarray, np.ndarray]:
    x, v = mean[..., :4], mean[..., 4:]
    pp, pv, vv = cov[..., :4], cov[..., 4:8], cov[..., 8:]
    r, _ = _noise(x[..., 3], dtype, 1, 1)
    r[..., 2] = dtype(1e-1) * dtype(1e-1)
    s = (pp + r).astype(dtype)
    kp, kv = (pp / s).astype(dtype), (pv / s).astype(dtype)
    y = (np.asarray(z, dtype) - x).astype(dtype)
    nx = (x + (kp * y).astype(dtype)).astype(dtype)
    nv = (v + (kv * y).astype(dtype)).astype(dtype)
    npp = (pp - (kp * pp).astype(dtype)).astype(dtype)
    npv = (pv - (kp * pv).astype(dtype)).astype(dtype)
    nvv = (vv - (kv * pv).astype(dtype)).astype(dtype)
    return np.concatenate([nx, nv], -1), np.concatenate([npp, npv, nvv], -1)


def measure(box: np.ndarray, dtype=F) -> np.ndarray:
    """(top, left, bottom, right) [..., 4] -> (cx, cy, a, h)."""
    b = np.asarray(box, dtype)
    top, left, bottom, right = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w, h = (right - left).astype(dtype), (bottom - top).astype(dtype)
    half = dtype(0.5)
    return np.stack([((left + right).astype(dtype) * half).astype(dtype), ((top + bottom).astype(dtype) * half).astype(dtype),
                     (w / h).astype(dtype), h], -1)


def box_of(mean: np.ndarray, dtype=F) -> np.ndarray:
    """mean [..., 8] -> (top, left, bottom, right) [..., 4]."""
    cx, cy, a, h = mean[..., 0], mean[..., 1], mean[..., 2], mean[..., 3]
    half = dtype(0.5)
    hw, hh = ((a * h).astype(dtype) * half).astype(dtype), (h * half).astype(dtype)
    return np.stack([(cy - hh).astype(dtype), (cx - hw).astype(dtype), (cy + hh).astype(dtype), (cx + hw).astype(dtype)], -1)


def iou_matrix(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """softnms.iou_to_all's float32 expression for every pair: a [T, 4], b [R, 4] -> [T, R]; a box whose area is NaN (a filter that left
    float32's range) has IoU NaN, as in the kernel, where iou_to_all says 0."""
    a, b = np.asarray(a, F).reshape(-1, 1, 4), np.asarray(b, F).reshape(1, -1, 4)
    ay0, ax0, ay1, ax1 = (np.minimum(a[..., 0], a[..., 2]), np.minimum(a[..., 1], a[..., 3]), np.maximum(a[..., 0], a[..., 2]),
                          np.maximum(a[..., 1], a[..., 3]))
    by0, bx0, by1, bx1 = (np.minimum(b[..., 0], b[..., 2]), np.minimum(b[..., 1], b[..., 3]), np.maximum(b[..., 0], b[..., 2]),
                          np.maximum(b[..., 1], b[..., 3]))
    with np.errstate(all='ignore'):
        area_a = ((ay1 - ay0).astype(F) * (ax1 - ax0).astype(F)).astype(F)
        area_b = ((by1 - by0).astype(F) * (bx1 - bx0).astype(F)).astype(F)
        iy0, ix0 = np.maximum(ay0, by0), np.maximum(ax0, bx0)
        iy1, ix1 = np.minimum(ay1, by1), np.minimum(ax1, bx1)
        inter = (np.maximum((iy1 - iy0).astype(F), F(0)) * np.maximum((ix1 - ix0).astype(F), F(0))).astype(F)
        union = ((area_a + area_b).astype(F) - inter).astype(F)
        none = (area_a <= 0) | (area_b <= 0)                 # as the kernel's tf_iou: an area that is NaN is not `none`, its IoU is NaN and
        return np.where(none, F(0), (inter / np.where(none, F(1), union)).astype(F)).astype(F)      # meets no threshold, not even 0


class Tracker:
    """The host form of one sequence: update(rows of a frame) -> (rows [k, 6] float32, ids [k] int32)."""

    def __init__(self, class_num: int, track_thresh=0.5, low_thresh=0.1, match_thresh=0.8, track_buffer=30, max_tracks: Optional[int] = None,
                 assign: str = 'greedy', fuse_score: bool = False, gmc: bool = False):
        cfg = check(track_thresh, low_thresh, match_thresh, track_buffer, max_tracks, assign=assign, fuse_score=fuse_score)
        if not isinstance(gmc, (bool, np.bool_)):
            raise ValueError(f'track_gmc {gmc!r}: expected True or False')
        self.gmc = bool(gmc)
        if int(class_num) < 1:
            raise ValueError(f'class_num {class_num!r}: expected at least 1')
        self.class_num, self.max_tracks = int(class_num), max_tracks
        self.assign, self.fuse_score = assign, bool(fuse_score)
        self.track_thresh, self.low_thresh = F(cfg['track_thresh']), F(cfg['low_thresh'])
        self.stage1 = F(1) - F(cfg['match_thresh'])
        self.open_thresh = self.track_thresh + F(OPEN_MARGIN)
        self.track_buffer = cfg['track_buffer']
        self.reset()

    def reset(self) -> None:
        self.frame, self.next_id, self.overflow = 0, 1, 0
        self.ids, self.cls, self.state, self.last = (np.zeros(0, np.int32) for _ in range(4))
        self.score = np.zeros(0, F)
        self.mean, self.cov = np.zeros((0, 8), F), np.zeros((0, 12), F)

    @property
    def live(self) -> int:
        return len(self.ids)

    def _rows(self, rows):
        """Step 2: -> (boxes [R, 4], scores [R], classes [R] int, high [R] bool) of the rows that take part, in row order."""
        r = np.asarray(rows, F).reshape(-1, 6)
        with np.errstate(all='ignore'):
            c = np.where(np.abs(r[:, 5]) < F(2 ** 30), r[:, 5], F(-1)).astype(np.int64)      # (a NaN or a huge class: none)
            h, w = (r[:, 2] - r[:, 0]).astype(F), (r[:, 3] - r[:, 1]).astype(F)
            ok = ((c.astype(F) == r[:, 5]) & (c >= 0) & (c < self.class_num) & (r[:, 4] >= self.low_thresh)
                  & (h > 0) & (h < np.inf) & (w > 0) & (w < np.inf))
        r, c = r[ok], c[ok]
        return r[:, :4], r[:, 4], c, r[:, 4] >= self.track_thresh

    def update(self, rows, cap: Optional[int] = None, motion=None):
        if motion is not None and not self.gmc:
            raise ValueError('motion given to a tracker opened without gmc=True')
        self.frame += 1
        if self.gmc:                                                      # step 0: the camera's translation moves every centre; v and P stay
            mx, my = (0, 0) if motion is None else motion
            self.mean[:, 0] = (self.mean[:, 0] + F(mx)).astype(F)
            self.mean[:, 1] = (self.mean[:, 1] + F(my)).astype(F)
        lost = self.state == LOST
        self.mean[lost, 7] = F(0)
        self.mean, self.cov = kf_predict(self.mean, self.cov)
        boxes, scores, classes, high = self._rows(rows)
        n_t, n_r = len(self.ids), len(boxes)
        iou = iou_matrix(box_of(self.mean), boxes) if n_t and n_r else np.zeros((n_t, n_r), F)
        same = self.cls[:, None] == classes[None, :]
        match = np.full(n_t, -1, np.int64)
        free = np.ones(n_r, bool)
        with np.errstate(all='ignore'):
            fused = (iou * scores[None, :]).astype(F) if self.fuse_score else iou
        for stage, (states, want_high, thr) in enumerate((((TRACKED, LOST), True, self.stage1), ((TRACKED,), False, F(STAGE2_IOU)),
                                                          ((NEW,), True, F(STAGE3_IOU)))):
            sim = fused if stage == 0 else iou
            t_ok = np.isin(self.state, states) & (match < 0)
            if self.assign == 'lap':
                r_ok = free & (high == want_high)
                for c in np.unique(self.cls[t_ok]):                       # ascending
                    ts, rs = np.flatnonzero(t_ok & (self.cls == c)), np.flatnonzero(r_ok & (classes == c))
                    if not len(rs):
                        continue
                    s = sim[np.ix_(ts, rs)]
                    allowed = s >= thr                                    # (a NaN meets no gate)
                    cost = np.where(allowed, np.float64(1) - s.astype(np.float64), LAP_FORBIDDEN)
                    for i, j in enumerate(lap(cost)):
                        if j >= 0 and allowed[i, j]:
                            match[ts[i]], free[rs[j]] = rs[j], False
                continue
            m = np.where(same & t_ok[:, None] & (free & (high == want_high))[None, :] & (sim >= thr), sim, F(-1))
            while m.size:
                k = int(np.argmax(m))                                     # the largest IoU; ties: the lowest track, then the lowest row
                t, r = divmod(k, n_r)
                if m[t, r] < 0:
                    break
                match[t], free[r] = r, False
                m[t, :], m[:, r] = F(-1), F(-1)
        hit = match >= 0
        if hit.any():
            self.mean[hit], self.cov[hit] = kf_update(self.mean[hit], self.cov[hit], measure(boxes[match[hit]]))
            self.score[hit] = scores[match[hit]]
        self.last[hit] = self.frame
        keep = hit | ((self.state != NEW) & (self.frame - self.last <= self.track_buffer))
        self.state = np.where(hit, TRACKED, LOST).astype(np.int32)
        for name in ('ids', 'cls', 'state', 'last', 'score', 'mean', 'cov'):
            setattr(self, name, getattr(self, name)[keep])
        opened = [r for r in np.flatnonzero(free & high) if scores[r] >= self.open_thresh]
        if self.max_tracks is not None and self.live + len(opened) > self.max_tracks:
            room = self.max_tracks - self.live
            self.overflow += len(opened) - room
            opened = opened[:room]
        if opened:
            k = len(opened)
            mean, cov = kf_open(measure(boxes[opened]))
            self.ids = np.concatenate([self.ids, np.arange(self.next_id, self.next_id + k, dtype=np.int32)])
            self.next_id += k
            self.cls = np.concatenate([self.cls, classes[opened].astype(np.int32)])
            self.state = np.concatenate([self.state, np.full(k, TRACKED if self.frame == 1 else NEW, np.int32)])
            self.last = np.concatenate([self.last, np.full(k, self.frame, np.int32)])
            self.score = np.concatenate([self.score, scores[opened]])
            self.mean, self.cov = np.concatenate([self.mean, mean]), np.concatenate([self.cov, cov])
        out = np.flatnonzero((self.state == TRACKED) & (self.last == self.frame))[:cap]
        rows_out = np.concatenate([box_of(self.mean[out]), self.score[out, None], self.cls[out, None].astype(F)], 1).astype(F)
        return rows_out.reshape(-1, 6), self.ids[out].copy()


def mot_lines(frame: int, rows: np.ndarray, ids: np.ndarray):
    """The MOTChallenge text lines of one frame's rows: frame,id,left,top,width,height,score,-1,-1,-1 (repr of the float32 values, so the
    lines parse back to the rows)."""
    for (top, left, bottom, right, score, _), i in zip(np.asarray(rows, F).reshape(-1, 6), ids):
        yield f'{int(frame)},{int(i)},{float(left)!r},{float(top)!r},{float(right - left)!r},{float(bottom - top)!r},{float(score)!r},-1,-1,-1'
