"""Options on the objectness and class terms of the YOLO loss (not in the reference, whose loss_fn, tools/utils.py:708-793,
has hard 0 / 1 targets and plain cross entropy): focal loss, label smoothing and an IoU-aware objectness target.

This module is the statement of the rule: float64, numpy only, no torch, importable without a GPU.  csrc/yk_loss.hip (yk_yolo_loss_opt) and
everything above it are held to it.  Restated from the papers and documents named below, not from anyone's code: parity with YOLOv5's or
Keras' implementation is unpinned.

Notation: x a logit, p = sigmoid(x), z in [0, 1] a target (possibly soft), bce(z, x) = max(x, 0) - x z + log(1 + exp(-|x|)).

  label smoothing   eps in [0, 1) (Zhang et al. 2019, "Bag of Freebies"; Keras BinaryCrossentropy(label_smoothing=)): every class target
                    becomes z' = z (1 - eps) + eps / 2.  Nothing else changes; eps = 0 is off.
  IoU objectness    obj_target = 'iou' (YOLOv5's gr = 1; default 'label'): in an object cell (y_true conf > obj_thresh) the objectness target
                    is z = clamp(IoU, 0, 1), IoU = I / (bw bh + tw th - I + 1e-7) between the decoded prediction b and the cell's label box
                    t, a constant in the gradient.  A cell without an object keeps its y_true conf (its label box is all zeros and is given
                    no IoU).  The weight `obj` (y_true conf), the ignore mask, the (2 - tw th) factor and the precision / recall counters
                    stay on y_true conf and the raw logit.  In the IoU box modes this is the IoU of the box term.
  focal             focal = 'obj' | 'cls' | 'all' (Lin et al. 2017; the soft-target form of YOLOv5's fl_gamma):
                        fl(z, x) = a_t (1 - p_t)^gamma bce(z, x),   p_t = z p + (1 - z)(1 - p),   a_t = z alpha + (1 - z)(1 - alpha)
                    and a_t = 1 when alpha = 0.  'obj' puts fl in place of bce in the obj and the noobj sums, 'cls' in the class sum, 'all'
                    in both.  The factor is not detached: with m = 1 - p_t = z sigmoid(-x) + (1 - z) sigmoid(x) (written without a
                    subtraction from 1, so a saturated logit keeps its bits), d m / d x = (1 - 2 z) p (1 - p) and
                        d fl / d x = a_t (gamma m^(gamma - 1) (1 - 2 z) p (1 - p) bce + m^gamma (p - z)).
                    m^0 = 1 everywhere: gamma = 0, alpha = 0 is bce.  gamma is 0 or in 1 .. 5; 0 < gamma < 1 is refused, the gradient is
                    unbounded where p_t -> 1.  alpha is 0 or inside (0, 1).

The options compose: focal sees the smoothed class targets and the IoU objectness target.  With w = y_true conf and ign the ignore mask,
    obj = obj_weight sum w t(z_o, x_o) / batch_size,  noobj = noobj_weight sum (1 - w) ign t(z_o, x_o) / batch_size,
    cls = sum w sum_c t(z'_c, x_c) / batch_size,      t = fl or bce,
the weights and the divisor where they were; no loss column is added."""
from __future__ import annotations

import numpy as np

FOCAL = {'off': 0, 'obj': 1, 'cls': 2, 'all': 3}             # YK_FOCAL_* bits (include/yolo_hip.h)
OBJ_TARGETS = {'label': 0, 'iou': 1}                         # YK_OBJ_TARGET_*
IOU_EPS = 1e-7
DEFAULTS = dict(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label')


def validate(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label') -> dict:
    """The five options as a dict, or ValueError naming the one that is out of range."""
    if focal not in FOCAL:
        raise ValueError(f'focal {focal!r}: choose one of ' + ', '.join(repr(k) for k in FOCAL))
    if obj_target not in OBJ_TARGETS:
        raise ValueError(f'obj_target {obj_target!r}: choose one of ' + ', '.join(repr(k) for k in OBJ_TARGETS))
    g, a, e = float(focal_gamma), float(focal_alpha), float(label_smooth)
    if not (g == 0.0 or 1.0 <= g <= 5.0):
        raise ValueError(f'focal_gamma {focal_gamma} must be 0 or lie in 1 .. 5 (below 1 the gradient is unbounded)')
    if not 0.0 <= a < 1.0:
        raise ValueError(f'focal_alpha {focal_alpha} must be 0 (off) or lie inside (0, 1)')
    if not 0.0 <= e < 1.0:
        raise ValueError(f'label_smooth {label_smooth} must lie in [0, 1)')
    return dict(focal=focal, focal_gamma=g, focal_alpha=a, label_smooth=e, obj_target=obj_target)


def is_off(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label') -> bool:
    """True where the loss is the one without options, whatever gamma and alpha say."""
    return focal == 'off' and float(label_smooth) == 0.0 and obj_target == 'label'


def describe(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label') -> str:
    """The options in force, for one printed line."""
    parts = []
    if focal != 'off':
        parts.append(f'focal {focal} (gamma {float(focal_gamma):g}, alpha {float(focal_alpha):g})')
    if float(label_smooth) != 0.0:
        parts.append(f'label smoothing {float(label_smooth):g}')
    if obj_target != 'label':
        parts.append(f'objectness target {obj_target}')
    return ', '.join(parts)


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce(z, x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def smooth(z, eps):
    return np.asarray(z, np.float64) * (1.0 - eps) + eps / 2.0


def focal_term(z, x, gamma=2.0, alpha=0.0):
    """-> (fl(z, x), d fl / d x), float64, elementwise."""
    z, x = np.asarray(z, np.float64), np.asarray(x, np.float64)
    p, q = sigmoid(x), sigmoid(-x)
    b = bce(z, x)
    m = z * q + (1.0 - z) * p
    at = z * alpha + (1.0 - z) * (1.0 - alpha) if alpha > 0 else np.ones_like(z)
    if gamma == 0:
        pw, dpw = np.ones_like(m), np.zeros_like(m)
    else:
        p1 = m ** (gamma - 1.0)
        pw, dpw = p1 * m, gamma * p1
    return at * pw * b, at * (dpw * (1.0 - 2.0 * z) * p * q * b + pw * (p - z))


def term(z, x, on, gamma, alpha):
    """fl where `on`, else bce, with its derivative by x."""
    if on:
        return focal_term(z, x, gamma, alpha)
    return bce(z, x), sigmoid(x) - z


def decode(y_pred, anchors):
    """Predictions in image scale, float64 [B,h,w,A,4] (cx, cy, w, h)."""
    yp = np.asarray(y_pred, np.float64)
    B, h, w, A, E = yp.shape
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    off = np.stack([gx, gy], -1)[:, :, None, :].astype(np.float64)
    xy = (sigmoid(yp[..., 0:2]) + off) / np.array([w, h], np.float64)
    return np.concatenate([xy, np.exp(yp[..., 2:4]) * np.asarray(anchors, np.float32).astype(np.float64)], -1)


def _inter(b, t):
    lo = np.maximum(b[..., 0:2] - b[..., 2:4] / 2, t[..., 0:2] - t[..., 2:4] / 2)
    hi = np.minimum(b[..., 0:2] + b[..., 2:4] / 2, t[..., 0:2] + t[..., 2:4] / 2)
    return np.clip(hi - lo, 0.0, None).prod(-1)


def box_iou(b, t):
    """IoU of boxes (cx, cy, w, h) with the 1e-7 of the box losses in the denominator."""
    i = _inter(b, t)
    return i / (b[..., 2] * b[..., 3] + t[..., 2] * t[..., 3] - i + IOU_EPS)


def ignore_mask(y_true, box, obj_thresh, iou_thresh):
    """1 where a prediction's best IoU with its image's label boxes is below iou_thresh (no label box: 1)."""
    yt = np.asarray(y_true, np.float64)
    ign = np.ones(yt.shape[:4])
    for b in range(len(yt)):
        m = yt[b, ..., 4] > obj_thresh
        if m.any():
            p, g = box[b][..., None, :], yt[b][..., 0:4][m]
            i = _inter(p, g)
            ign[b] = ((i / (p[..., 2] * p[..., 3] + g[:, 2] * g[:, 3] - i)).max(-1) < iou_thresh).astype(np.float64)
    return ign


def closed_form(y_true, y_pred, anchors, obj_thresh=0.7, iou_thresh=0.5, ow=1.0, nw=1.0, batch_size=None, focal='off', focal_gamma=2.0,
                focal_alpha=0.0, label_smooth=0.0, obj_target='label'):
    """The obj, noobj and cls terms of one layer and their gradient, derivatives written out.  y_true / y_pred [B,h,w,A,5+C].
    -> (dict(obj, noobj, cls), gradient entries 4.. as float64 [B,h,w,A,1+C], objectness target [B,h,w,A]).  The box term and gradient
    entries 0..3 are not touched by the options (the IoU target is a constant)."""
    o = validate(focal, focal_gamma, focal_alpha, label_smooth, obj_target)
    yt, yp = np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64)
    bs = batch_size or yt.shape[0]
    box = decode(yp, anchors)
    w = yt[..., 4]
    ob = w > obj_thresh
    ign = ignore_mask(yt, box, obj_thresh, iou_thresh)
    zo = w.copy()
    if o['obj_target'] == 'iou' and ob.any():
        zo[ob] = np.clip(box_iou(box[ob], yt[..., 0:4][ob]), 0.0, 1.0)
    bits = FOCAL[o['focal']]
    to, do = term(zo, yp[..., 4], bits & 1, o['focal_gamma'], o['focal_alpha'])
    zc = smooth(yt[..., 5:], o['label_smooth']) if o['label_smooth'] else yt[..., 5:]
    tc, dc = term(zc, yp[..., 5:], bits & 2, o['focal_gamma'], o['focal_alpha'])
    terms = dict(obj=float(ow * (w * to).sum() / bs), noobj=float(nw * ((1 - w) * ign * to).sum() / bs),
                 cls=float((w[..., None] * tc).sum() / bs))
    grad = np.concatenate([((ow * w + nw * (1 - w) * ign) * do)[..., None], w[..., None] * dc], -1) / bs
    return terms, grad, zo
