"""Seeded cases for the operating points (oppoint.py), shared by tests/test_oppoint.py (the host statement alone) and tests/test_gpu_oppoint.py
(map_gpu.MapEvaluator.sweep / .confusion against it).  A case is a dict: name, class_num, dets (one float32 [k,6] array per image), gts (one
float64 [g,6] array per image), diff (one bool [g] array per image), conf (the confusion threshold: one of the scores).  `sweep_reference`
and `confusion_reference` evaluate a case once with oppoint.py and keep the result; nobody changes it.

Rows come from tests/coco_cases.random_case: jittered copies of the boxes (one in ten with another class; here every fourth row is moved
to the next class as well), noise, duplicated and crowded boxes, difficult boxes, a handful of distinct scores (ties everywhere) and +-0.0
scores.  Every score is a multiple of 1/8, so it EQUALS a
threshold of every grid k / 1000 and k / 4096 used here.

What the shapes are for (csrc/yk_map.hip): the sweep's histogram runs one thread per row in workgroups of 256, its suffix sums one wave per
class in chunks of 64 thresholds; the confusion matching runs one wave per image, 64 pairs at a time, out of LDS while the rows taking part
+ the boxes of the image are at most yk_map_confusion_lds_boxes() and out of global memory above it.

Content conditions, asserted of the reference alone when a case is built (`check_content`):
  * at least one score of every case equals a threshold of the default grid k / 1000;
  * every case's reference confusion matrix has at least 3 matches off the diagonal, at least 3 background false positives and at least 3
    background false negatives."""
import functools

import numpy as np

from tests import coco_cases as cc

LDS_BOXES = 1024                                     # yk_map_confusion_lds_boxes() of the library; tests/test_gpu_oppoint.py asserts it
GRIDS = {
    'default': np.arange(1000) / 1000,
    'one': np.array([0.25]),
    'two': np.array([0.0, 0.5]),
    'most': np.arange(4096) / 4096,
}
EMPTY_D, EMPTY_G = np.zeros((0, 6), np.float32), np.zeros((0, 6))


def _big_image(rng, n_rows, n_box=8, class_num=20):
    """n_box boxes on a row (the last two far from every detection: missed), n_rows detections: jittered or exact copies of the first
    n_box - 2 boxes, half of them with another class."""
    k = np.arange(n_box)
    ext = rng.choice([30.0, 44.0, 60.0], (n_box, 2))
    gt = np.stack([np.full(n_box, 10.0), k * 80.0, 10.0 + ext[:, 0], k * 80.0 + ext[:, 1], np.ones(n_box),
                   rng.integers(0, class_num, n_box).astype(np.float64)], 1)
    rows = np.zeros((n_rows, 6), np.float32)
    for r in range(n_rows):
        src = gt[int(rng.integers(0, n_box - 2))]
        rows[r, :4] = src[:4] + rng.normal(0, rng.choice([0.0, 1.0, 4.0, 12.0]), 4)
        rows[r, 4] = rng.choice(cc.SCORES[3:])                                       # all at or above 0.25: every row takes part
        rows[r, 5] = src[5] if rng.random() < 0.5 else (src[5] + 1 + rng.integers(0, class_num - 1)) % class_num
    return rows, gt, rng.random(n_box) < 0.15


def _one_box(rng, n_rows, n_box, class_num=20):
    """n_box copies-with-a-shift of one box, n_rows detections around the first."""
    base = np.array([20.0, 20.0, 90.0, 120.0])
    gt = np.stack([np.concatenate([base + np.tile(rng.uniform(-6, 6, 2), 2), [1.0, float(rng.integers(0, class_num))]]) for _ in range(n_box)])
    rows = np.zeros((n_rows, 6), np.float32)
    for r in range(n_rows):
        rows[r, :4] = base + rng.normal(0, rng.choice([0.0, 2.0, 8.0]), 4)
        rows[r, 4] = rng.choice(cc.SCORES[3:])
        rows[r, 5] = rng.integers(0, class_num)
    return rows, gt, np.zeros(n_box, bool)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def put(name, class_num, dets, gts, diff, conf=0.25):
        out[name] = dict(name=name, class_num=class_num, dets=[np.asarray(d, np.float32).reshape(-1, 6) for d in dets], gts=gts, diff=diff, conf=conf)

    def confused(dets, class_num):
        """Every fourth row gets the next class: matches off the diagonal."""
        dets = [np.array(x, np.float32).reshape(-1, 6) for x in dets]
        for x in dets:
            x[::4, 5] = (x[::4, 5] + 1) % class_num
        return dets

    d, g, h = cc.random_case(np.random.default_rng(2024), 12, 20)
    d = confused(d, 20)
    put('mixed20', 20, d, g, h)
    tail = (d[:8], g[:8], h[:8])                                                    # appended to the shaped cases below
    d, g, h = cc.random_case(np.random.default_rng(2025), 16, 80)
    d = confused(d, 80)
    d[0][::3, 5], d[1][::4, 5], d[2][::5, 5] = 80.0, -3.0, 85.5                      # classes outside [0, 80): they belong nowhere
    g = [x.copy() for x in g]
    if len(g[3]):
        g[3][0, 5] = 99.0
    put('wide80', 80, d, g, h)
    # gaps: images without rows and images without boxes between the others
    d, g, h = [], [], []
    for i in range(8):
        d += [tail[0][i], EMPTY_D, tail[0][i]]
        g += [tail[1][i], tail[1][i], EMPTY_G]
        h += [tail[2][i], tail[2][i], np.zeros(0, bool)]
    put('gaps', 20, [EMPTY_D] + d + [EMPTY_D], [EMPTY_G] + g + [EMPTY_G], [np.zeros(0, bool)] + h + [np.zeros(0, bool)])
    # lanes: 63 / 64 / 65 rows against one box, one row against 65 boxes
    rng = np.random.default_rng(64)
    d, g, h = list(tail[0]), list(tail[1]), list(tail[2])
    for n_rows, n_box in ((63, 1), (64, 1), (65, 1), (1, 65)):
        a, b, c = _one_box(rng, n_rows, n_box)
        d.append(a), g.append(b), h.append(c)
    put('lanes', 20, d, g, h)
    # lds: one image with exactly LDS_BOXES rows + boxes (staged), one with one more (the global path); 8 boxes each
    rng = np.random.default_rng(160)
    d, g, h = list(tail[0][:4]), list(tail[1][:4]), list(tail[2][:4])
    for n_rows in (LDS_BOXES - 8, LDS_BOXES - 7):
        a, b, c = _big_image(rng, n_rows)
        d.append(a), g.append(b), h.append(c)
    put('lds', 20, d, g, h)
    return out


SWEEP_CASES = ['mixed20', 'wide80', 'gaps', 'lanes']
CONFUSION_CASES = ['mixed20', 'wide80', 'gaps', 'lanes', 'lds']


def case(name):
    return cases()[name]


def one_class():
    """class_num 1 (no off-diagonal entry can exist: a sweep shape, not a shared confusion case)."""
    d, g, h = cc.random_case(np.random.default_rng(2017), 6, 1, max_det=30)
    return dict(name='one_class', class_num=1, dets=d, gts=g, diff=h, conf=0.25)


def head(c, n_rows):
    """The case cut to its first n_rows detection rows (images kept)."""
    dets, left = [], n_rows
    for d in c['dets']:
        dets.append(d[:max(left, 0)])
        left -= len(dets[-1])
    assert left <= 0, 'the case has fewer rows'
    return dict(c, dets=dets, name=f'{c["name"]}[:{n_rows}]')


def pack(dets):
    dets = [np.asarray(d, np.float32).reshape(-1, 6) for d in dets]
    off = np.zeros(len(dets) + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in dets])
    return (np.concatenate(dets) if dets else np.zeros((0, 6), np.float32)), off


def check_content(name):
    """The conditions of the module docstring, of the reference alone."""
    c = case(name)
    scores = np.concatenate([d[:, 4] for d in c['dets']]).astype(np.float64)
    assert np.isin(scores, GRIDS['default']).any(), f'{name}: no score equals a grid threshold'
    if name in CONFUSION_CASES:
        m, K = confusion_reference(name)['matrix'], c['class_num']
        off_diag = int(m[:K, :K].sum() - np.trace(m[:K, :K]))
        assert off_diag >= 3 and m[K, :K].sum() >= 3 and m[:K, K].sum() >= 3, (name, off_diag, m[K, :K].sum(), m[:K, K].sum())


@functools.lru_cache(maxsize=None)
def sweep_reference(name, grid='default', plus_one=False):
    from k210_yolo_framework_amd import oppoint
    c = case(name)
    return oppoint.sweep(c['dets'], c['gts'], c['class_num'], GRIDS[grid], 0.5, c['diff'], plus_one)


@functools.lru_cache(maxsize=None)
def confusion_reference(name, plus_one=False):
    from k210_yolo_framework_amd import oppoint
    c = case(name)
    return oppoint.confusion(c['dets'], c['gts'], c['class_num'], c['conf'], 0.5, c['diff'], plus_one)
