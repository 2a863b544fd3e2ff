"""The rule of the IoU-family box losses (`make train BOXLOSS=giou|diou|ciou`), stated twice, and the seeded inputs the CPU
and GPU tests share.  CPU only.

For an object cell (y_true conf > obj_thresh) the prediction in image scale is b = ((sigmoid(px) + col) / w, (sigmoid(py) + row) / h,
exp(pw) anchor_w, exp(ph) anchor_h), the label box is t = y_true[0:4], edges are centre -+ size / 2, and with eps = 1e-7

    I = clamped intersection,  U = bw bh + tw th - I + eps,  IoU = I / U,  Cw, Ch = extent of the smallest enclosing box
    giou:  C = Cw Ch + eps                                   l = 1 - IoU + (C - U) / C
    diou:  c2 = Cw^2 + Ch^2 + eps, rho2 = |b - t|^2 (centres)    l = 1 - IoU + rho2 / c2
    ciou:  v = (4 / pi^2) (atan(tw / th) - atan(bw / bh))^2, alpha = v / (1 - IoU + v + eps), a constant in the gradient
                                                             l = 1 - IoU + rho2 / c2 + alpha v

The cell's term is conf (2 - tw th) box_weight l, summed over the object cells and divided by batch_size; xy and wh are then 0 and
total = obj + noobj + cls + box.  A cell without an object is skipped, not multiplied away (its label box is all zeros: atan(0 / 0)).

(a) `autograd`: the whole layer loss in torch, differentiable in y_pred - for 'mse' the loss of oracle/loss_ref.py.
(b) `closed_form`: the box term and its gradient in numpy float64, derivatives written out - the form csrc/yk_loss.hip mirrors.  At an
    exact tie of a min / max each side gets one half, as in torch."""
import numpy as np
import torch
import torch.nn.functional as TF

EPS = 1e-7
MODES = ('giou', 'diou', 'ciou')
TERMS = ('total', 'xy', 'wh', 'obj', 'noobj', 'cls', 'box')


# ---- (a) torch autograd ------------------------------------------------------------------------------------------------------------------
def _box_term_torch(b, t, mode):
    """b, t: [n,4] (cx, cy, w, h) -> l [n]."""
    b1, b2, t1, t2 = b[:, 0:2] - b[:, 2:4] / 2, b[:, 0:2] + b[:, 2:4] / 2, t[:, 0:2] - t[:, 2:4] / 2, t[:, 0:2] + t[:, 2:4] / 2
    ov = (torch.minimum(b2, t2) - torch.maximum(b1, t1)).clamp(min=0)
    inter = ov[:, 0] * ov[:, 1]
    union = b[:, 2] * b[:, 3] + t[:, 2] * t[:, 3] - inter + EPS
    iou = inter / union
    en = torch.maximum(b2, t2) - torch.minimum(b1, t1)
    if mode == 'giou':
        c = en[:, 0] * en[:, 1] + EPS
        return 1 - iou + (c - union) / c
    c2 = en[:, 0] ** 2 + en[:, 1] ** 2 + EPS
    rho2 = (b[:, 0] - t[:, 0]) ** 2 + (b[:, 1] - t[:, 1]) ** 2
    l = 1 - iou + rho2 / c2
    if mode == 'ciou':
        v = (4 / np.pi ** 2) * (torch.atan(t[:, 2] / t[:, 3]) - torch.atan(b[:, 2] / b[:, 3])) ** 2
        alpha = (v / (1 - iou + v + EPS)).detach()
        l = l + alpha * v
    return l


def layer_loss_torch(yt, yp, anchors, obj_thresh, iou_thresh, ow, nw, ww, batch_size, box_loss='mse', box_weight=1.0):
    """One output layer in torch, in the dtype of yp, differentiable in yp -> (dict of the seven terms as 0-d tensors, ignore mask)."""
    B, h, w, A, E = yp.shape
    dt = yp.dtype
    anc = torch.as_tensor(np.asarray(anchors, np.float32)).to(dt)
    gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    off = torch.stack([gx, gy], -1)[:, :, None, :].to(dt)
    whv = torch.tensor([w, h]).to(dt)
    obj = yt[..., 4:5]
    ob = yt[..., 4] > obj_thresh
    axy = (torch.sigmoid(yp[..., 0:2]) + off) / whv
    awh = torch.exp(yp[..., 2:4]) * anc
    with torch.no_grad():
        ign = torch.ones(B, h, w, A, dtype=dt)
        for b in range(B):
            gxy, gwh = yt[b][..., 0:2][ob[b]], yt[b][..., 2:4][ob[b]]
            if len(gxy):
                p1, p2 = axy[b][..., None, :] - awh[b][..., None, :] / 2, axy[b][..., None, :] + awh[b][..., None, :] / 2
                g1, g2 = gxy - gwh / 2, gxy + gwh / 2
                iw = (torch.minimum(p2, g2) - torch.maximum(p1, g1)).clamp(min=0)
                inter = iw[..., 0] * iw[..., 1]
                iou = inter / (awh[b][..., None, 0] * awh[b][..., None, 1] + gwh[:, 0] * gwh[:, 1] - inter)
                ign[b] = (iou.max(-1).values < iou_thresh).to(dt)
    cw = 2 - yt[..., 2:3] * yt[..., 3:4]
    bce = lambda z, x: TF.binary_cross_entropy_with_logits(x, z, reduction='none')
    zero = torch.zeros((), dtype=dt)
    if box_loss == 'mse':
        gtxy = yt[..., 0:2] * whv - off
        gtwh = torch.where(ob[..., None], torch.log(yt[..., 2:4].clamp(min=1e-30) / anc), torch.zeros(1, dtype=dt))
        xy = (obj * cw * bce(gtxy, yp[..., 0:2])).sum() / batch_size
        wh = (obj * cw * ww * (gtwh - yp[..., 2:4]) ** 2).sum() / batch_size
        box = zero
    else:
        xy = wh = zero
        box = zero
        if ob.any():                                                     # object cells only: the others are skipped, not weighted by 0
            l = _box_term_torch(torch.cat([axy[ob], awh[ob]], 1), yt[..., 0:4][ob], box_loss)
            box = (obj[ob][:, 0] * cw[ob][:, 0] * box_weight * l).sum() / batch_size
    bc = bce(yt[..., 4:5], yp[..., 4:5])
    ol = ow * (obj * bc).sum() / batch_size
    nl = nw * ((1 - obj) * ign[..., None] * bc).sum() / batch_size
    cl = (obj * bce(yt[..., 5:], yp[..., 5:])).sum() / batch_size
    total = ol + nl + cl + xy + wh if box_loss == 'mse' else ol + nl + cl + box
    return dict(total=total, xy=xy, wh=wh, obj=ol, noobj=nl, cls=cl, box=box), ign


def autograd(y_true, y_pred, anchors, obj_thresh=0.7, iou_thresh=0.5, ow=1.0, nw=1.0, ww=1.0, batch_size=None, box_loss='mse',
             box_weight=1.0, dtype=torch.float64):
    """(a).  -> (dict of the seven terms as floats, dL/dy_pred as float64 numpy, ignore mask)."""
    yt = torch.from_numpy(np.asarray(y_true)).to(dtype)
    yp = torch.from_numpy(np.asarray(y_pred)).to(dtype).requires_grad_(True)
    terms, ign = layer_loss_torch(yt, yp, anchors, obj_thresh, iou_thresh, ow, nw, ww, batch_size or yp.shape[0], box_loss, box_weight)
    terms['total'].backward()
    return {k: float(v.detach()) for k, v in terms.items()}, yp.grad.double().numpy(), ign.double().numpy()


# ---- (b) numpy float64, derivatives written out ------------------------------------------------------------------------------------------
def _less(u, v):
    return np.where(u < v, 1.0, np.where(u == v, 0.5, 0.0))


def _axis(bc, bs, tc, ts):
    """One axis: clamped overlap and enclosing extent with their derivatives by the prediction's centre and size."""
    b1, b2, t1, t2 = bc - bs / 2, bc + bs / 2, tc - ts / 2, tc + ts / 2
    raw = np.minimum(b2, t2) - np.maximum(b1, t1)
    on = (raw > 0).astype(np.float64)
    i2, i1 = on * _less(b2, t2), on * _less(t1, b1)
    e2, e1 = _less(t2, b2), _less(b1, t1)
    return dict(ov=np.maximum(raw, 0), ov_c=i2 - i1, ov_s=(i2 + i1) / 2, en=np.maximum(b2, t2) - np.minimum(b1, t1), en_c=e2 - e1,
                en_s=(e2 + e1) / 2, raw=raw, gaps=np.stack([np.abs(b1 - t1), np.abs(b2 - t2), np.abs(raw)]))


def box_loss_and_grad(b, t, mode):
    """b, t: float64 [n,4] (cx, cy, w, h) -> (l [n], dl/db [n,4], dict(iou, axes))."""
    bx, by, bw, bh = b.T
    tx, ty, tw, th = t.T
    X, Y = _axis(bx, bw, tx, tw), _axis(by, bh, ty, th)
    inter = X['ov'] * Y['ov']
    union = bw * bh + tw * th - inter + EPS
    iou = inter / union
    dI = np.stack([Y['ov'] * X['ov_c'], X['ov'] * Y['ov_c'], Y['ov'] * X['ov_s'], X['ov'] * Y['ov_s']])
    dU = np.stack([-dI[0], -dI[1], bh - dI[2], bw - dI[3]])
    l = 1 - iou
    g = -(dI - iou * dU) / union
    if mode == 'giou':
        c = X['en'] * Y['en'] + EPS
        dC = np.stack([Y['en'] * X['en_c'], X['en'] * Y['en_c'], Y['en'] * X['en_s'], X['en'] * Y['en_s']])
        l = l + (c - union) / c
        g = g - (dU - union / c * dC) / c
    else:
        c2 = X['en'] ** 2 + Y['en'] ** 2 + EPS
        dx, dy = bx - tx, by - ty
        r = (dx * dx + dy * dy) / c2
        dc2 = np.stack([2 * X['en'] * X['en_c'], 2 * Y['en'] * Y['en_c'], 2 * X['en'] * X['en_s'], 2 * Y['en'] * Y['en_s']])
        l = l + r
        g = g + (np.stack([2 * dx, 2 * dy, 0 * dx, 0 * dx]) - r * dc2) / c2
        if mode == 'ciou':
            k4 = 4 / np.pi ** 2
            d = np.arctan(tw / th) - np.arctan(bw / bh)
            v = k4 * d * d
            alpha = v / (1 - iou + v + EPS)
            q = alpha * 2 * k4 * d / (bw * bw + bh * bh)
            l = l + alpha * v
            g = g + np.stack([0 * q, 0 * q, -q * bh, q * bw])
    return l, g.T, dict(iou=iou, X=X, Y=Y)


def decode(y_pred, anchors):
    """Predictions in image scale, float64 [B,h,w,A,4]."""
    yp = np.asarray(y_pred, np.float64)
    B, h, w, A, E = yp.shape
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    off = np.stack([gx, gy], -1)[:, :, None, :].astype(np.float64)
    sig = 1 / (1 + np.exp(-yp[..., 0:2]))
    return np.concatenate([(sig + off) / np.array([w, h], np.float64), np.exp(yp[..., 2:4]) * np.asarray(anchors, np.float32).astype(np.float64)], -1), sig


def closed_form(y_true, y_pred, anchors, obj_thresh=0.7, batch_size=None, box_loss='giou', box_weight=1.0):
    """(b).  -> (box term, its gradient entries 0..3 as [B,h,w,A,4], dict(iou, X, Y) of the object cells)."""
    yt = np.asarray(y_true, np.float64)
    B, h, w, A, E = yt.shape
    bs = batch_size or B
    ob = yt[..., 4] > obj_thresh
    grad = np.zeros(yt.shape[:4] + (4,))
    if not ob.any():
        return 0.0, grad, None
    box, sig = decode(y_pred, anchors)
    b, t, s = box[ob], yt[..., 0:4][ob], sig[ob]
    l, g, info = box_loss_and_grad(b, t, box_loss)
    k = yt[..., 4][ob] * (2 - t[:, 2] * t[:, 3]) * box_weight
    chain = np.stack([s[:, 0] * (1 - s[:, 0]) / w, s[:, 1] * (1 - s[:, 1]) / h, b[:, 2], b[:, 3]], 1)
    grad[ob] = k[:, None] * g * chain / bs
    return float((k * l).sum() / bs), grad, info


def min_gap(y_true, y_pred, anchors, obj_thresh=0.7, iou_thresh=0.5):
    """How far the inputs are from every decision fp32 and float64 could take differently: the smallest distance between two compared
    edges of an object cell (the min / max of both axes and the clamp of the overlap at 0), and the smallest distance of a prediction's
    best IoU from the ignore threshold."""
    _, _, info = closed_form(y_true, y_pred, anchors, obj_thresh)
    edge = min(float(info['X']['gaps'].min()), float(info['Y']['gaps'].min())) if info else np.inf
    yt = np.asarray(y_true, np.float64)
    box, _ = decode(y_pred, anchors)
    thr = np.inf
    for b in range(len(yt)):
        m = yt[b, ..., 4] > obj_thresh
        if m.any():
            p, g = box[b][..., None, :], yt[b][..., 0:4][m]
            ov = np.clip(np.minimum(p[..., 0:2] + p[..., 2:4] / 2, g[:, 0:2] + g[:, 2:4] / 2) - np.maximum(p[..., 0:2] - p[..., 2:4] / 2, g[:, 0:2] - g[:, 2:4] / 2), 0, None)
            inter = ov[..., 0] * ov[..., 1]
            best = (inter / (p[..., 2] * p[..., 3] + g[:, 2] * g[:, 3] - inter)).max(-1)
            thr = min(thr, float(np.abs(best - iou_thresh).min()))
    return edge, thr


def atol_needed(got, want, rtol=2e-5):
    """The smallest atol at which np.allclose(got, want, rtol, atol) holds."""
    return float(np.clip(np.abs(np.asarray(got, np.float64) - want) - rtol * np.abs(want), 0, None).max())


# ---- the seeded inputs of tests/test_box_loss_ref.py and tests/test_gpu_box_loss.py --------------------------------------------------------
def _logit(p):
    return np.log(p / (1 - p))


def random_case(seed, B, hh, ww, A, C, n_obj=(1, 7), empty=(), garbage=False):
    """Labels written straight into the tensor: per image a few object cells (conf 1, centre inside the cell, one class) among all-zero
    ones; predictions normal(0, 1.5) with pw, ph uniform over +-4 (tiny and huge boxes).  empty: images without an object.  garbage: half
    of the cells without an object get a random box and classes under conf 0."""
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.05, 0.5, (A, 2)).astype(np.float32)
    P = hh * ww * A
    y_true = np.zeros((B, P, 5 + C), np.float32)
    for b in range(B):
        if b in empty:
            continue
        n = min(int(rng.integers(*n_obj)), P)
        slot = np.sort(rng.choice(P, n, replace=False))
        cell = slot // A
        y_true[b, slot, 0] = (cell % ww + rng.uniform(0.05, 0.95, n)) / ww
        y_true[b, slot, 1] = (cell // ww + rng.uniform(0.05, 0.95, n)) / hh
        y_true[b, slot, 2:4] = rng.uniform(0.05, 0.9, (n, 2))
        y_true[b, slot, 4] = 1
        y_true[b, slot, 5 + rng.integers(0, C, n)] = 1
    if garbage:
        free = (y_true[..., 4] == 0) & (rng.uniform(size=(B, P)) < 0.5)
        y_true[free, 0:4] = rng.uniform(0, 1, (int(free.sum()), 4))
        y_true[free, 5:] = rng.uniform(0, 1, (int(free.sum()), C))
    y_true = y_true.reshape(B, hh, ww, A, 5 + C)
    y_pred = rng.normal(0, 1.5, y_true.shape).astype(np.float32)
    y_pred[..., 2:4] = rng.uniform(-4, 4, y_pred[..., 2:4].shape)
    return anc, y_true, y_pred


def geometry_case(seed=0):
    """4x4 grid, 3 anchors, 2 classes, 2 images.  Four cells of image 0 are built by hand: the prediction disjoint from the label box,
    strictly inside it, strictly around it, and overlapping it in part; the others are random_case's."""
    anc, y_true, y_pred = random_case(100 + seed, 2, 4, 4, 3, 2, n_obj=(3, 6))
    forced = [  # (row, col, anchor), label (in-cell x, y, w, h), prediction (in-cell x, y, w, h)
        ((0, 0, 0), (0.15, 0.2, 0.05, 0.06), (0.85, 0.8, 0.05, 0.04)),       # disjoint
        ((1, 2, 1), (0.5, 0.5, 0.6, 0.5), (0.4, 0.6, 0.1, 0.12)),            # prediction inside the label
        ((2, 1, 2), (0.5, 0.4, 0.08, 0.1), (0.45, 0.5, 0.7, 0.6)),           # label inside the prediction
        ((3, 3, 0), (0.3, 0.3, 0.3, 0.2), (0.7, 0.6, 0.35, 0.3)),            # partial overlap
    ]
    cells = []
    for (r, c, a), t, p in forced:
        y_true[0, r, c, a] = 0
        y_true[0, r, c, a, 0:5] = ((c + t[0]) / 4, (r + t[1]) / 4, t[2], t[3], 1)
        y_true[0, r, c, a, 5] = 1
        y_pred[0, r, c, a, 0:4] = (_logit(p[0]), _logit(p[1]), np.log(p[2] / anc[a, 0]), np.log(p[3] / anc[a, 1]))
        cells.append((0, r, c, a))
    return anc, y_true, y_pred, cells


def geometry_of(b, t):
    """'disjoint' | 'pred_inside' | 'label_inside' | 'partial' of boxes (cx, cy, w, h), float64."""
    b1, b2, t1, t2 = b[0:2] - b[2:4] / 2, b[0:2] + b[2:4] / 2, t[0:2] - t[2:4] / 2, t[0:2] + t[2:4] / 2
    if (np.minimum(b2, t2) - np.maximum(b1, t1) <= 0).any():
        return 'disjoint'
    if (b1 > t1).all() and (b2 < t2).all():
        return 'pred_inside'
    if (t1 > b1).all() and (t2 < b2).all():
        return 'label_inside'
    return 'partial'


def equal_case():
    """4x8 grid, 3 anchors, 1 class, 2 images: in every object cell the prediction IS the label box, to the last bit in fp32 and in float64
    alike: px = py = pw = ph = 0, so sigmoid = 0.5 and exp = 1 exactly, the grid sizes are powers of two, so (0.5 + col) / w is exact, and the
    label's size is the anchor.  The anchors are large enough (area >= 0.075) for 1 - I / (I + eps) to stay below 1e-5."""
    anc = np.array([[0.25, 0.3], [0.5, 0.4], [0.8, 0.6]], np.float32)
    rng = np.random.default_rng(7)
    y_true = np.zeros((2, 4, 8, 3, 6), np.float32)
    y_pred = rng.normal(0, 1.5, y_true.shape).astype(np.float32)
    for (b, r, c, a) in [(0, 0, 0, 0), (0, 1, 2, 1), (0, 2, 7, 2), (1, 3, 1, 0), (1, 0, 5, 1)]:
        y_true[b, r, c, a] = ((0.5 + c) / 8, (0.5 + r) / 4, anc[a, 0], anc[a, 1], 1, 1)
        y_pred[b, r, c, a, 0:4] = 0
    return anc, y_true, y_pred


# name -> (B, h, w, A, C, batch_size, weights (obj, noobj, wh), box_weight, kwargs of random_case).  The grids: one cell; the 7x10 head with a
# divisor that is not the number of images, an image without objects and garbage under conf 0; h w A = 255, 256, 257 (the 256-box chunk
# of the kernel's grid, and the wide grid of its fma note)
PARITY_CASES = {
    'one_cell': (1, 1, 1, 1, 1, None, (1, 1, 1), 1.0, dict(n_obj=(1, 2))),
    'head_7x10': (4, 7, 10, 3, 20, 16, (5, 0.5, 0.5), 2.5, dict(empty=(2,), garbage=True)),
    'p255': (3, 5, 17, 3, 2, None, (1, 1, 1), 1.0, {}),
    'p256': (3, 8, 8, 4, 2, None, (1, 1, 1), 0.5, {}),
    'p257': (3, 1, 257, 1, 2, None, (1, 1, 1), 1.0, {}),
}
CASE_SEEDS = {'one_cell': 1, 'head_7x10': 2, 'p255': 3, 'p256': 4, 'p257': 5}


def parity_case(name):
    """-> (anchors, y_true, y_pred, keyword arguments of `autograd` but for box_loss)."""
    if name == 'geometry':
        anc, y_true, y_pred, _ = geometry_case()
        return anc, y_true, y_pred, dict(ow=1.0, nw=1.0, ww=1.0, batch_size=None, box_weight=1.0)
    B, hh, ww, A, C, bs, (ow, nw, whw), bw, kw = PARITY_CASES[name]
    anc, y_true, y_pred = random_case(CASE_SEEDS[name], B, hh, ww, A, C, **kw)
    return anc, y_true, y_pred, dict(ow=ow, nw=nw, ww=whw, batch_size=bs, box_weight=bw)


ALL_PARITY = tuple(PARITY_CASES) + ('geometry',)

# The gradient tolerance of tests/test_gpu_box_loss.py: rtol 2e-5 as in tests/test_gpu_loss.py, and an absolute term that is not a guess:
# (a) evaluated in torch float32 on the CPU on the inputs above needs, against (a) in float64 at rtol 2e-5, the atol below (the largest
# over ALL_PARITY and the three modes; tests/test_box_loss_ref.py measures it again and holds it to this figure); the kernel, another
# fp32 evaluation of the same expression, is given twice that.
F32_ATOL_MEASURED = 2.130e-8
