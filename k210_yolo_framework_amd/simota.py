"""SimOTA dynamic label assignment with anchors: the rule csrc/yk_ota.hip is held to.  numpy, float64, no torch.

Restated from the YOLOX paper (Ge et al. 2021, section 2.2 "SimOTA") and adapted to an anchor head, as YOLOv7 uses it; parity with either
code base is not pinned.  Which predictions train on which box is decided per step from the predictions themselves:

  candidates  of an image: every (layer, row, col, anchor), numbered j in the flat order of the label buffer (layer, row, col, anchor).
  boxes       of an image: its rows (cls, x, y, w, h), g in row order; x y w h clipped as min(max(v, 1e-8), 1) with C's fmax / fmin, which
              return the other operand for a NaN: a NaN goes to 1e-8 (the kernel's and yk_boxes_to_labels_f32's clip; validity does not
              look at w and h).
  validity    yk_boxes_to_labels_f32's test: the class truncated toward zero in [0, C), the centre finite, floor(x W) in [0, W) and
              floor(y H) in [0, H) in EVERY layer (on the unclipped centre); here also: the box is among the first `max_boxes` of its image.
              Nothing is written for an invalid box; status is the smallest such row of `boxes`, INT32_MAX for a clean batch.
  decode      of the fp32 row (tx, ty, tw, th, to, tc_0 ..), in float64 (the loss kernel's): bx = (s(tx) + col) / W, by = (s(ty) + row) / H,
              bw = exp(tw) aw, bh = exp(th) ah, s(v) = 1 / (1 + exp(-v)).
  geometry    px = (col + 0.5) / W, py = (row + 0.5) / H; in_box = |px - x| < w / 2 and |py - y| < h / 2; in_ctr = |px - x| < radius / W and
              |py - y| < radius / H; eligible = in_box or in_ctr.
  IoU         corners c -+ s / 2; I = max(min(x2, X2) - max(x1, X1), 0) max(min(y2, Y2) - max(y1, Y1), 0); U = (w h + bw bh) - I;
              IoU = I / U, or 0 where U is not finite or not positive.
  class cost  q_k = sqrt(s(tc_k) s(to)); L1(q) = max(log q, -100), L0(q) = max(log1p(-q), -100) (torch's BCE clamp);
              Z_j = sum_k -L0(q_k), k ascending; C_cls(g, j) = (Z_j + L0(q_c)) - L1(q_c), c the box's class.
  cost        (C_cls + iou_weight (-log(IoU + 1e-8))) + (0 if in_box and in_ctr else 1e5)
  dynamic k   E_g the eligible count; S the sum of the min(topk, E_g) largest eligible IoUs, added from the largest down;
              k_g = min(E_g, max(1, floor(S))).
  selection   a box takes its k_g eligible candidates of smallest cost, ties to the lower j.
  conflicts   a candidate chosen by several boxes goes to the one of smallest cost, ties to the lower g.
  writing     the owner writes (float32)(x, y, w, h), 1 into entries 0..4 of slot j and 1 at 5 + c; every other entry is 0.

A prediction that is not finite gives a deterministic but unspecified assignment.  `margin` is the smallest absolute gap over the batch
between the k_g-th and the (k_g + 1)-th cost of a box, between the two lowest costs contending for a candidate (bit-identical boxes left
out: the same arithmetic decides them everywhere), and between S and the integers next to it whose crossing changes k (2 .. E_g).  Only exp, log
and log1p differ between libm and the device, by ulps, so above a margin of 1e-9 a second implementation decides as this one does."""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np

STATUS_CLEAN = 2 ** 31 - 1
PENALTY = 1e5


def _clip(v):
    """min(max(v, 1e-8), 1) as C's fmax / fmin compute it: a NaN goes to 1e-8."""
    return np.fmin(np.fmax(np.asarray(v, np.float64), 1e-8), 1.0)


def grids(helper_or_cfg):
    """(out_hw [L][2] ints, anchors [L] arrays [A, 2] float64, class_num) of a Helper or of a dict with those three keys."""
    get = helper_or_cfg.get if isinstance(helper_or_cfg, dict) else lambda k: getattr(helper_or_cfg, k)
    anchors = [np.asarray(a, np.float64).reshape(-1, 2) for a in get('anchors')]
    return [(int(h), int(w)) for h, w in np.asarray(get('out_hw')).reshape(-1, 2)], anchors, int(get('class_num'))


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _candidates(preds, s, out_hw, anchors):
    """Image s: (bx, by, bw, bh, s(to), px, py, W, H per candidate in flat order; the class logits [N, C] float64)."""
    cols = []
    with np.errstate(over='ignore', invalid='ignore'):
        for p, (H, W), a in zip(preds, out_hw, anchors):
            t = np.asarray(p[s], np.float32).astype(np.float64).reshape(H, W, len(a), -1)
            row, col = np.arange(H, dtype=np.float64)[:, None, None], np.arange(W, dtype=np.float64)[None, :, None]
            full = lambda v: np.broadcast_to(v, t.shape[:3]).reshape(-1)
            cols.append((full((_sig(t[..., 0]) + col) / W), full((_sig(t[..., 1]) + row) / H), full(np.exp(t[..., 2]) * a[:, 0]),
                         full(np.exp(t[..., 3]) * a[:, 1]), full(_sig(t[..., 4])), full((col + 0.5) / W + 0 * row), full((row + 0.5) / H + 0 * col),
                         full(np.float64(W) + 0 * row + 0 * col), full(np.float64(H) + 0 * row + 0 * col), t[..., 5:].reshape(-1, t.shape[-1] - 5)))
    return [np.concatenate([c[i] for c in cols]) for i in range(10)]


def _l0(q):
    with np.errstate(divide='ignore'):
        return np.maximum(np.log1p(-q), -100.0)


def _l1(q):
    with np.errstate(divide='ignore'):
        return np.maximum(np.log(q), -100.0)


def assign(preds: Sequence[np.ndarray], boxes, first, helper_or_cfg, topk: int = 10, radius: float = 2.5, iou_weight: float = 3.0,
           max_boxes=None, detail=None):
    """-> (labels per layer [n, h, w, A, 5 + C] float32, npos [n] int32, status, margin).  preds: the raw outputs per layer,
    [n, h, w, A, 5 + C] float32; boxes [N, 5] float64 rows (cls, x, y, w, h); first [n + 1]: image s owns rows first[s] .. first[s + 1] - 1.
    detail: a list that receives one dict per valid box, in (image, row) order, of what the rule did: image, g (the row of `boxes`), E, S, k,
    el / iou / cost (every eligible j ascending, its IoU and its cost), j (the k chosen, in the order taken) with cost, in_box and in_ctr
    beside it, and per chosen j rivals (the other rows that chose it, ascending; empty: uncontested) and owner (the row that got it).
    It changes no result."""
    out_hw, anchors, C = grids(helper_or_cfg)
    boxes, first = np.asarray(boxes, np.float64).reshape(-1, 5), np.asarray(first, np.int64).reshape(-1)
    n = len(first) - 1
    labels = [np.zeros((n, H, W, len(a), 5 + C), np.float32) for (H, W), a in zip(out_hw, anchors)]
    sizes = [H * W * len(a) for (H, W), a in zip(out_hw, anchors)]
    npos, status, margin = np.zeros(n, np.int32), STATUS_CLEAN, math.inf
    for s in range(n):
        b0, b1 = max(int(first[s]), 0), min(int(first[s + 1]), len(boxes))
        if b1 <= b0:
            continue
        bx, by, bw, bh, so, px, py, gw, gh, tc = _candidates(preds, s, out_hw, anchors)
        with np.errstate(over='ignore', invalid='ignore'):
            q = np.sqrt(_sig(tc) * so[:, None])
            terms = -_l0(q)
            Z = np.zeros(len(q))
            for k in range(C):                                      # k ascending
                Z = Z + terms[:, k]
        chosen, records = {}, {}                                    # j -> [(cost, g)]; g -> its record
        for g in range(b0, b1):
            cls, x0, y0 = boxes[g, 0], boxes[g, 1], boxes[g, 2]
            ok = cls > -1.0 and cls < C and np.isfinite(x0) and np.isfinite(y0) and (max_boxes is None or g - b0 < max_boxes)
            for H, W in out_hw:
                ok = ok and 0.0 <= math.floor(x0 * W) < W and 0.0 <= math.floor(y0 * H) < H
            if not ok:
                status = min(status, g)
                continue
            c = int(cls)
            x, y, w, h = _clip(boxes[g, 1:])
            dx, dy = np.abs(px - x), np.abs(py - y)
            in_box, in_ctr = (dx < w / 2) & (dy < h / 2), (dx < radius / gw) & (dy < radius / gh)
            el = np.nonzero(in_box | in_ctr)[0]
            with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
                ow = np.maximum(np.minimum(x + w / 2, bx[el] + bw[el] / 2) - np.maximum(x - w / 2, bx[el] - bw[el] / 2), 0.0)
                oh = np.maximum(np.minimum(y + h / 2, by[el] + bh[el] / 2) - np.maximum(y - h / 2, by[el] - bh[el] / 2), 0.0)
                I = ow * oh
                U = (w * h + bw[el] * bh[el]) - I
                iou = np.where(np.isfinite(U) & (U > 0), I / np.where(U > 0, U, 1.0), 0.0)
                qc = q[el, c]
                cost = ((Z[el] + _l0(qc)) - _l1(qc)) + iou_weight * (-np.log(iou + 1e-8))
                cost = cost + np.where(in_box[el] & in_ctr[el], 0.0, PENALTY)
            S = 0.0
            for v in np.sort(iou)[::-1][:topk]:                     # from the largest down
                S = S + v
            k = min(len(el), max(1, int(math.floor(S))))
            for m in (math.floor(S), math.floor(S) + 1):
                if 2 <= m <= len(el):                             # crossing m changes k
                    margin = min(margin, abs(S - m))
            order = np.argsort(cost, kind='stable')                # ties to the lower j: el ascends
            if len(el) > k:
                margin = min(margin, float(cost[order[k]] - cost[order[k - 1]]))
            for o in order[:k]:
                chosen.setdefault(int(el[o]), []).append((float(cost[o]), g))
            if detail is not None:
                took = order[:k]
                records[g] = dict(image=s, g=g, E=len(el), S=S, k=k, el=el.copy(), iou=iou.copy(), cost=cost.copy(), j=[int(v) for v in el[took]],
                                  j_cost=[float(v) for v in cost[took]], in_box=[bool(v) for v in in_box[el[took]]],
                                  in_ctr=[bool(v) for v in in_ctr[el[took]]])
                detail.append(records[g])
        for j, takers in chosen.items():
            takers.sort()                                           # smallest cost, ties to the lower g
            for (c0, g0), (c1, g1) in zip(takers, takers[1:]):
                if not np.array_equal(boxes[g0], boxes[g1]):
                    margin = min(margin, c1 - c0)
            g = takers[0][1]
            for _, g0 in takers if detail is not None else ():
                rec = records[g0]
                rec.setdefault('rivals', {})[j] = sorted(g1 for _, g1 in takers if g1 != g0)
                rec.setdefault('owner', {})[j] = g
            l = 0
            while j >= sizes[l]:
                j -= sizes[l]
                l += 1
            slot = labels[l][s].reshape(-1, 5 + C)[j]
            slot[:4] = _clip(boxes[g, 1:]).astype(np.float32)
            slot[4] = 1.0
            slot[5 + int(boxes[g, 0])] = 1.0
            npos[s] += 1
    return labels, npos, status, margin
