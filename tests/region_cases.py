"""Seeded inputs for the C-mode region layer (csrc/yk_region.hip: region_decode_kernel, region_nms_kernel, the region_layer_* ABI) at the places
random logits in (-6, 6) never reach, shared by tests/test_region_cases.py (CPU: the builders and the oracle checked on their own) and
tests/test_gpu_region_edges.py (the kernels, bit for bit against the oracle).  Nothing here touches a GPU.

Every builder returns a Case whose `x` is fp32 [B, A, 5 + C, H, W] (entries tx, ty, tw, th, to, classes) and FINITE: a NaN or an infinite logit
makes inf - inf, a NaN whose sign bit differs between x86 and the device, so a bit comparison would mean nothing there.  Overflow to inf from finite
logits is wanted: both sides stay free of NaN on it."""
import collections
import functools

import numpy as np

F = np.float32
YK_MAX_ANCHORS = 8
YK_NMS_MAXC = 2048                        # csrc/yk_nms.h: candidates of one (image, class) held in LDS
DEFAULT_WH = (320, 224)
ANCHOR_SMALL = (.3, .3, .2, .4, .4, .2)

Case = collections.namedtuple('Case', 'name x anchor thr nms net_wh image_wh')


def dims(case):
    """-> (B, W, H, A, C)"""
    B, A, E, H, W = case.x.shape
    return B, W, H, A, E - 5


def _case(name, x, anchor, thr, nms, net_wh=DEFAULT_WH, image_wh=DEFAULT_WH):
    x = np.ascontiguousarray(x, F)
    assert x.ndim == 5 and np.isfinite(x).all(), name
    anchor = np.asarray(anchor, F)
    assert anchor.size == 2 * x.shape[1], name
    x.setflags(write=False)
    anchor.setflags(write=False)
    return Case(name, x, anchor, float(thr), float(nms), tuple(net_wh), tuple(image_wh))


_REFERENCE = {}


def reference(case, nms=None):
    """The CPU oracle's (output, boxes, probs) of every image of the case, computed once and shared (read-only)."""
    import oracle
    key = (case.name, nms)
    if key not in _REFERENCE:
        B, W, H, A, C = dims(case)
        res = [oracle.region_run(case.x[b], case.anchor, W, H, A, C, case.thr, case.nms if nms is None else nms, case.net_wh, case.image_wh)
               for b in range(B)]
        for r in res:
            for a in r:
                a.setflags(write=False)
        _REFERENCE[key] = res
    return _REFERENCE[key]


def layout(x, kind):
    """x [B, A, E, H, W] -> the dense array yk_region_batched reads as 'chw' [B, A*E, H, W] or 'hwc' [B, H, W, A*E]."""
    B, A, E, H, W = x.shape
    if kind == 'chw':
        return x.reshape(B, A * E, H, W).copy()                   # (a writable copy: the case itself is read-only)
    return x.transpose(0, 3, 4, 1, 2).reshape(B, H, W, A * E).copy()


# ----------------------------------------------------------------------------------------------------------------- (a) expf sweep
EXPF_OVERFLOW = float.fromhex('0x1.62e42ep6')       # yk_expf_glibc: x above this -> inf
EXPF_UNDERFLOW = float.fromhex('-0x1.9fe368p6')     # x below this -> 0
EXPF_CENTRES = (EXPF_OVERFLOW, EXPF_UNDERFLOW, -87.33654,      # ln(FLT_MIN): the normal/subnormal edge
                88.0, -88.0, 0.0, 1e-8, -1e-8, -103.2789,      # ln(2^-149): the smallest subnormal
                -95.0, 1.0, -1.0)


def expf_points():
    """Each centre with its 8 fp32 neighbours on either side."""
    pts = []
    for c in EXPF_CENTRES:
        lo = hi = F(c)
        side = [F(c)]
        for _ in range(8):
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            side += [lo, hi]
        pts += sorted(side)
    return np.array(pts, F)


@functools.lru_cache(maxsize=None)
def expf_sweep():
    """52x52, A=3, C=1, B=2, anchors 1 and net == image: both scale factors are exactly 1.0f, so boxes[:, 2] IS expf(tw) and boxes[:, 3] IS
    expf(th).  thr = 2: no probability passes, NMS sees no candidate.  tx, ty, to reuse the values, so logistic sees expf(-v) over the range."""
    rng = np.random.default_rng(20240)
    B, A, C, H, W = 2, 3, 1, 52, 52
    pts = expf_points()
    x = np.empty((B, A, 5 + C, H, W), F)
    for b in range(B):
        v = rng.uniform(-110, 95, A * H * W).astype(F)
        v[rng.permutation(v.size)[:pts.size]] = pts
        w = -v[::-1]
        tw, th = v.reshape(A, H, W), w.reshape(A, H, W)
        x[b, :, 0], x[b, :, 1], x[b, :, 2], x[b, :, 3], x[b, :, 4], x[b, :, 5] = tw, th, tw, th, tw, th
    return _case('expf', x, np.ones(2 * A, F), 2.0, 0.3)


def check_expf_f64(got, t, what):
    """`got` against float32(exp(float64(t))): within 1 ulp where that is finite, infinite exactly where it is infinite, and 0 only below the
    underflow threshold.  glibc documents expf's error as under 0.502 ULP, so its result is one of the two floats that bracket the true value, and
    so is the correctly rounded one: they are equal or adjacent.  (Non-negative floats: the distance in ulps is the difference of the bit patterns.)"""
    got, t = np.asarray(got, F).ravel(), np.asarray(t, F).ravel()
    with np.errstate(over='ignore'):
        want = np.exp(t.astype(np.float64)).astype(F)
    fin = np.isfinite(want)
    assert not np.isnan(got).any(), what
    np.testing.assert_array_equal(np.isinf(got), ~fin, err_msg=what)
    ulps = np.abs(got[fin].view(np.int32).astype(np.int64) - want[fin].view(np.int32).astype(np.int64))
    worst = int(ulps.argmax())
    assert ulps[worst] <= 1, (what, float(t[fin][worst]), float(got[fin][worst]), float(want[fin][worst]), int(ulps[worst]))
    assert (t[got == 0] < F(EXPF_UNDERFLOW)).all(), what
    return int(ulps.max()), int((ulps != 0).sum())


# ----------------------------------------------------------------------------------------------------------------- (b) softmax tail
@functools.lru_cache(maxsize=None)
def softmax_tail():
    """C=3 with class logits (0, u(-103, -88), -200): e / total of the second class is subnormal, of the third 0; obj * e is subnormal
    or 0.  thr = 0: every non-zero probability, subnormal ones included, is an NMS candidate."""
    rng = np.random.default_rng(20241)
    A, C, H, W = 3, 3, 52, 52
    x = np.empty((1, A, 5 + C, H, W), F)
    x[:, :, 0:2] = rng.uniform(-1, 1, (1, A, 2, H, W))
    x[:, :, 2:4] = rng.uniform(-2, 0, (1, A, 2, H, W))
    x[:, :, 4] = 5
    x[:, :, 5] = 0
    x[:, :, 6] = rng.uniform(-103, -88, (1, A, H, W))
    x[:, :, 7] = -200
    return _case('softmax_tail', x, ANCHOR_SMALL, 0.0, 0.3, (416, 416))


# ----------------------------------------------------------------------------------------------------------------- (c) image sizes
# (net, image) -> the integer new_w, new_h of correct_region_boxes (region_layer.c:139-161)
IMAGE_SIZES = (((320, 224), (224, 320), (156, 224)), ((320, 224), (640, 480), (298, 224)), ((320, 224), (500, 333), (320, 213)),
               ((416, 416), (333, 500), (277, 416)), ((416, 416), (1920, 1080), (416, 234)))


def letterbox_dims(net_wh, image_wh):
    """new_w, new_h with the reference's float comparison and truncating integer division; also which branch and whether it truncated."""
    (nw, nh), (iw, ih) = net_wh, image_wh
    if F(nw) / F(iw) < F(nh) / F(ih):
        return nw, (ih * nw) // iw, 'fit_w', (ih * nw) % iw != 0
    return (iw * nh) // ih, nh, 'fit_h', (iw * nh) % ih != 0


@functools.lru_cache(maxsize=None)
def image_sizes():
    rng = np.random.default_rng(20242)
    B, A, C, H, W = 2, 3, 2, 7, 10
    anchor = rng.uniform(0.05, 0.9, 2 * A).astype(F)
    x = rng.uniform(-4, 4, (B, A, 5 + C, H, W)).astype(F)
    return [_case(f'image_{iw}x{ih}_in_{nw}x{nh}', x, anchor, 0.2, 0.4, (nw, nh), (iw, ih)) for (nw, nh), (iw, ih), _ in IMAGE_SIZES]


def unletterbox_f64(case):
    """float64 restatement of get_region_box + correct_region_boxes -> boxes [B, nb, 4].  The integer new_w, new_h are part of the definition."""
    B, W, H, A, C = dims(case)
    x = case.x.astype(np.float64)
    (nw, nh), (new_w, new_h) = case.net_wh, letterbox_dims(case.net_wh, case.image_wh)[:2]
    col, row = np.arange(W)[None, None, None, :], np.arange(H)[None, None, :, None]
    anc = case.anchor.astype(np.float64).reshape(A, 2)
    sig = lambda v: 1 / (1 + np.exp(-v))
    with np.errstate(over='ignore'):
        bx = ((col + sig(x[:, :, 0])) / W - (nw - new_w) / 2 / nw) / (new_w / nw)
        by = ((row + sig(x[:, :, 1])) / H - (nh - new_h) / 2 / nh) / (new_h / nh)
        bw = np.exp(x[:, :, 2]) * anc[None, :, 0, None, None] * nw / new_w
        bh = np.exp(x[:, :, 3]) * anc[None, :, 1, None, None] * nh / new_h
    return np.stack([bx, by, bw, bh], -1).reshape(B, A * H * W, 4)


# ----------------------------------------------------------------------------------------------------------------- (d) ties
@functools.lru_cache(maxsize=None)
def ties():
    """Every cell has the same logits, so every candidate of a class has the same probability: the survivors are decided by the tie-break
    (ascending box index) alone.  10x7x3 = 210 candidates (LDS path), 52x52x3 = 8112 (global-memory path)."""
    out = []
    for W, H in ((10, 7), (52, 52)):
        x = np.zeros((1, 3, 7, H, W), F)
        x[:, :, 2:4] = -0.5
        x[:, :, 4] = 3
        out.append(_case(f'ties_{W}x{H}', x, ANCHOR_SMALL, 0.3, 0.3, (416, 416)))
    return out


# ----------------------------------------------------------------------------------------------------------------- (e) LDS boundary
LDS_COUNTS = ((YK_NMS_MAXC - 1, YK_NMS_MAXC + 1), (YK_NMS_MAXC, YK_NMS_MAXC + 1), (YK_NMS_MAXC + 1, YK_NMS_MAXC + 1))


@functools.lru_cache(maxsize=None)
def lds_boundary():
    """52x52x3, C=2, B=3.  2049 boxes per image are "on" (to = 4, the rest -30), at a random permutation of the box indices; class logits
    (0, 0) make an "on" box a candidate of both classes, (-9, 9) of class 1 only.  Candidates per image: class 0 has 2047, 2048, 2049 and
    class 1 always 2049, so one launch runs both paths, and the second image fills the LDS arrays to the last slot."""
    rng = np.random.default_rng(20243)
    A, C, H, W = 3, 2, 52, 52
    nb = A * H * W
    x = np.zeros((len(LDS_COUNTS), A, 5 + C, H, W), F)
    x[:, :, 0:2] = rng.uniform(-1, 1, (len(LDS_COUNTS), A, 2, H, W))
    x[:, :, 2:4] = rng.uniform(-3, -2, (len(LDS_COUNTS), A, 2, H, W))
    for b, (n0, n1) in enumerate(LDS_COUNTS):
        to, c0, c1 = np.full(nb, -30, F), np.zeros(nb, F), np.zeros(nb, F)
        on = rng.permutation(nb)[:n1]
        to[on] = 4
        c0[on[n0:]], c1[on[n0:]] = -9, 9
        x[b, :, 4], x[b, :, 5], x[b, :, 6] = to.reshape(A, H, W), c0.reshape(A, H, W), c1.reshape(A, H, W)
    return _case('lds_boundary', x, ANCHOR_SMALL, 0.3, 0.3, (416, 416))


# ----------------------------------------------------------------------------------------------------------------- (f) small
SMALL = ((1, 1, 1, 1, 0.0), (3, 2, 1, 1, 0.0), (5, 3, YK_MAX_ANCHORS, 2, 0.05))


@functools.lru_cache(maxsize=None)
def small():
    """Grids below one wavefront, A == YK_MAX_ANCHORS, threshold 0.  Image 0 has no candidate at all (to = -200: expf overflows, objectness
    is exactly 0), image 1 exactly one, image 2 is random."""
    out = []
    for W, H, A, C, thr in SMALL:
        rng = np.random.default_rng(20244 + W)
        x = rng.uniform(-4, 4, (3, A, 5 + C, H, W)).astype(F)
        x[0:2, :, 4] = -200
        x[1, A - 1, 4, H - 1, W // 2] = 2
        out.append(_case(f'small_{W}x{H}x{A}x{C}', x, rng.uniform(0.05, 0.9, 2 * A), thr, 0.3))
    return out


# ----------------------------------------------------------------------------------------------------------------- (g) saturating boxes
@functools.lru_cache(maxsize=None)
def saturating():
    """5x3, A=2, C=2, every box detected (to = 4).  Anchor 0, row 0: tw = 100 (infinite width).  One cell of anchor 1: tw = th = 89 (both
    infinite).  Anchor 1, row 2: th = -120 (height exactly 0).  The draw casts of the ABI see -inf, +inf and huge values."""
    rng = np.random.default_rng(20245)
    A, C, H, W = 2, 2, 3, 5
    x = rng.uniform(-2, 2, (1, A, 5 + C, H, W)).astype(F)
    x[:, :, 4] = 4
    x[0, 0, 2, 0, :] = 100
    x[0, 1, 2:4, 1, 3] = 89
    x[0, 1, 3, 2, :] = -120
    return _case('saturating', x, (0.5, 0.4, 0.25, 0.6), 0.3, 0.3)
