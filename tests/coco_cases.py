"""Seeded cases for the COCO-style metric, shared by tests/test_coco_eval.py (the host statement alone) and tests/test_gpu_coco_eval.py
(map_gpu.MapEvaluator.coco_result against it).  A case is a dict: name, class_num, dets (one float32 [k,6] array per image), gts (one
float64 [g,6] array per image), diff (one bool [g] array per image), max_dets.  `reference(name)` evaluates a case once with
coco_eval.evaluate's defaults and keeps the result; nobody changes it.

What the shapes are for (csrc/yk_map.hip): an (image, class) group is matched by one wave, its ground-truth boxes 64 at a time ('lanes':
groups of 0, 1, 64, 65 and 130 boxes); a class's curve is scanned in tiles of 256 rows ('scan': classes of 0, 1, 255, 256, 257 and 1000
rows); 'mixed20' and 'one_class' are the seeded sweep with duplicated boxes (equal IoU), crowded boxes (the COCO rule falls back to the
next free box where the VOC rule gives up), difficult boxes, boxes and detections on both sides of the 32^2 and 96^2 area limits, a
handful of distinct scores (ties everywhere) and +-0.0 scores; 'cut' is 'mixed20' with max_dets = 1."""
import functools

import numpy as np

SCORES = np.array([-0.0, 0.0, 0.125, 0.25, 0.5, 0.5, 0.75, 0.875], np.float32)


def _boxes(rng, g, size):
    """g boxes: top-left anywhere, extents from a few pixels to half the picture (areas on both sides of 32^2 and 96^2)."""
    tl = rng.uniform(0, size * 0.6, (g, 2))
    ext = rng.choice([12.0, 24.0, 40.0, 70.0, 110.0, 150.0], (g, 2)) * rng.uniform(0.8, 1.2, (g, 2))
    return np.concatenate([tl, tl + ext], 1)


def random_case(rng, n_img, class_num, max_det=40, max_gt=6, size=320.0, scores=SCORES):
    dets, gts, diff = [], [], []
    for _ in range(n_img):
        g = int(rng.integers(0, max_gt + 1))
        box = _boxes(rng, g, size)
        cls = rng.integers(0, class_num, g).astype(np.float64)
        for j in range(g):                                                            # a duplicate (equal IoU with every detection) or a
            u = rng.random()                                                          # shifted neighbour of the same class (a crowd)
            if u < 0.2:
                box, cls = np.concatenate([box, box[j:j + 1]]), np.append(cls, cls[j])
            elif u < 0.4:
                shift = (box[j, 2:] - box[j, :2]) * rng.uniform(0.1, 0.3, 2)
                box, cls = np.concatenate([box, box[j:j + 1] + np.tile(shift, 2)]), np.append(cls, cls[j])
        g = len(box)
        gt = np.concatenate([box, np.ones((g, 1)), cls[:, None]], 1) if g else np.zeros((0, 6))
        n = int(rng.integers(0, max_det + 1))
        rows = []
        for _ in range(n):
            if g and rng.random() < 0.75:                                             # a jittered copy (several of one box included)
                src = gt[int(rng.integers(0, g))]
                ext = min(src[2] - src[0], src[3] - src[1])
                b = src[:4] + rng.normal(0, ext * rng.choice([0.0, 0.02, 0.06, 0.12]), 4)
                c = src[5] if rng.random() < 0.9 else rng.integers(0, class_num)
            else:                                                                     # noise of any size
                b = _boxes(rng, 1, size)[0]
                c = rng.integers(0, class_num)
            rows.append([*b, rng.choice(scores), c])
        dets.append(np.asarray(rows, np.float32).reshape(-1, 6))
        gts.append(gt)
        diff.append(rng.random(g) < 0.2)
    return dets, gts, diff


def _grid_group(rng, n_box, n_det, cls, other_cls):
    """One image: n_box boxes of class `cls` on a grid (sizes vary), two boxes of another class between them, n_det jittered detections."""
    k = np.arange(n_box)
    top, left = (k // 12) * 40.0, (k % 12) * 40.0
    ext = rng.choice([14.0, 30.0, 34.0], (n_box, 2))
    gt = np.stack([top, left, top + ext[:, 0], left + ext[:, 1], np.ones(n_box), np.full(n_box, float(cls))], 1)
    extra = np.array([[3., 3., 30., 30., 1., other_cls], [45., 45., 70., 70., 1., other_cls]])
    order = rng.permutation(n_box + 2)                                                # the class's boxes are not contiguous in the image
    gt = np.concatenate([gt, extra])[order]
    rows = []
    for _ in range(n_det):
        if n_box and rng.random() < 0.85:
            src = gt[int(rng.integers(0, len(gt)))]
            b = src[:4] + rng.normal(0, rng.choice([0.0, 0.5, 1.5]), 4)
            c = src[5]
        else:
            b, c = _boxes(rng, 1, 400.0)[0], cls
        rows.append([*b, rng.choice(SCORES), c])
    return np.asarray(rows, np.float32).reshape(-1, 6), gt, rng.random(len(gt)) < 0.15


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def put(name, class_num, dets, gts, diff, max_dets=100):
        out[name] = dict(name=name, class_num=class_num, dets=dets, gts=gts, diff=diff, max_dets=max_dets)

    d, g, h = random_case(np.random.default_rng(2014), 12, 20)
    put('mixed20', 20, d, g, h)
    put('cut', 20, d, g, h, max_dets=1)
    d, g, h = random_case(np.random.default_rng(2017), 6, 1, max_det=30)
    put('one_class', 1, d, g, h)
    # lanes: class 0 groups of 0, 1, 64, 65 and 130 boxes; an image without rows and one without boxes between them
    rng = np.random.default_rng(64)
    d, g, h = [], [], []
    for n_box in (0, 1, 64, 65, 130):
        a, b, c = _grid_group(rng, n_box, max(3, int(1.5 * n_box)), 0, 1)
        d.append(a), g.append(b), h.append(c)
        if n_box == 1:
            d.append(np.zeros((0, 6), np.float32)), g.append(b.copy()), h.append(c.copy())            # no rows
        if n_box == 64:
            d.append(a.copy()), g.append(np.zeros((0, 6))), h.append(np.zeros(0, bool))               # no boxes
    put('lanes', 2, d, g, h)
    # scan: classes of 0, 1, 255, 256, 257 and 1000 rows over 12 images (no group above max_dets)
    rng = np.random.default_rng(256)
    want = [0, 1, 255, 256, 257, 1000]
    n_img = 12
    d, g, h = [[] for _ in range(n_img)], [], []
    for i in range(n_img):
        box = _boxes(rng, 8, 320.0)
        g.append(np.concatenate([box, np.ones((8, 1)), rng.integers(0, 6, (8, 1)).astype(np.float64)], 1))
        h.append(rng.random(8) < 0.2)
    for c, n in enumerate(want):
        for k in range(n):
            i = k % n_img
            same = g[i][g[i][:, 5] == c]
            if len(same) and rng.random() < 0.7:
                src = same[int(rng.integers(0, len(same)))]
                b = src[:4] + rng.normal(0, (src[2] - src[0]) * rng.choice([0.0, 0.03, 0.1]), 4)
            else:
                b = _boxes(rng, 1, 320.0)[0]
            d[i].append([*b, rng.choice(SCORES), c])
    d = [np.asarray(rng.permutation(np.asarray(r, np.float64).reshape(-1, 6)), np.float32) for r in d]
    put('scan', 6, d, g, h)
    return out


def case(name):
    return cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name, config='default'):
    """coco_eval.evaluate of a case under a named (thresholds, ranges) configuration; computed once."""
    from k210_yolo_framework_amd import coco_eval
    c = case(name)
    thr, area = CONFIGS[config]
    return coco_eval.evaluate(c['dets'], c['gts'], c['class_num'], thr, area, c['max_dets'], c['diff'])


BOTH_ENDS = np.array([[0, 1e10]])
FOUR = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
CONFIGS = {
    'default': (None, None),                                                          # T = 10, A = 4
    't1a1': (np.array([0.5]), BOTH_ENDS),
    't16a4': (np.linspace(0.2, 0.95, 16), FOUR),                                      # T * A = 64
    't64a1': (np.linspace(0.05, 0.995, 64), BOTH_ENDS),                               # T = 64: one range fills the mask
    't13a5': (np.linspace(0.35, 0.95, 13), np.concatenate([FOUR, [[0, 50 ** 2]]])),   # T * A = 65: refused on the device
}
