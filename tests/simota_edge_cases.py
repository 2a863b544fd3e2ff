"""The cases tests/test_gpu_simota_edges.py holds csrc/yk_ota.hip to simota.assign on, each named for the path of the kernels it is here
for; tests/test_simota_edge_cases.py proves on the CPU, from simota.assign's `detail`, that it gets there.  numpy only, no device.

`case(name)` -> dict(cfg, preds, boxes, first, opts, ties).  A case is either random (everything drawn from default_rng(seed); the seeds
were chosen on the CPU so that the rule's margin exceeds 1e-9) or crafted.  A crafted case with ties=True carries decisions at a gap of
exactly 0; they are exact on both sides because both sides compute the tied quantities with the same operations on the same inputs (all
logits 0: s = 0.5 and exp = 1 exactly, so a candidate is its cell centre with its anchor's size, and every IoU comes from + - * / min max
alone), and every other decision of such a case has a gap above 1e-9 (`nonzero_gap`).  `rule(name)` is simota.assign's answer with its
detail, computed once and shared; nobody writes into it."""
import functools
import math

import numpy as np

from k210_yolo_framework_amd import simota

TWO = [(2, 3), (4, 6)]


def net(out_hw, A, C, rng=None, anchors=None):
    """cfg of grids out_hw with A anchors each (an int, or one count per layer)"""
    A = [A] * len(out_hw) if isinstance(A, int) else list(A)
    if anchors is None:
        anchors = [rng.uniform(.05, .9, (a, 2)) for a in A]
    return dict(out_hw=list(out_hw), anchors=[np.asarray(a, np.float64).reshape(-1, 2) for a in anchors], class_num=C)


def drawn_preds(cfg, n, rng):
    C = cfg['class_num']
    return [(rng.normal(0, 1.5, (n, h, w, len(a), 5 + C)) * np.r_[1, 1, .3, .3, np.ones(1 + C)]).astype(np.float32)
            for (h, w), a in zip(cfg['out_hw'], cfg['anchors'])]


def zero_preds(cfg, n):
    return [np.zeros((n, h, w, len(a), 5 + cfg['class_num']), np.float32) for (h, w), a in zip(cfg['out_hw'], cfg['anchors'])]


def drawn_boxes(N, C, rng, lo=.05, hi=.6):
    return np.stack([rng.integers(0, C, N), rng.uniform(.1, .9, N), rng.uniform(.1, .9, N), rng.uniform(lo, hi, N), rng.uniform(lo, hi, N)], 1).astype(np.float64)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def aim(preds, cfg, boxes, first, rng, share=.5):
    """About `share` of the rows get tw = log(w / aw) + N(0, 0.05) and th likewise, (w, h) of one of the image's boxes: many high IoUs."""
    for p, a in zip(preds, cfg['anchors']):
        for s in range(p.shape[0]):
            if first[s + 1] == first[s]:
                continue
            hit = rng.random(p.shape[1:4]) < share
            g = rng.integers(first[s], first[s + 1], p.shape[1:4])
            tw = np.log(boxes[g, 3] / a[None, None, :, 0]) + rng.normal(0, .05, p.shape[1:4])
            th = np.log(boxes[g, 4] / a[None, None, :, 1]) + rng.normal(0, .05, p.shape[1:4])
            p[s, ..., 2] = np.where(hit, tw, p[s, ..., 2])
            p[s, ..., 3] = np.where(hit, th, p[s, ..., 3])


def random_case(out_hw, A, C, counts, seed, aimed=False, lo=.05, hi=.6, **opts):
    rng = np.random.default_rng(seed)
    cfg = net(out_hw, A, C, rng)
    preds = drawn_preds(cfg, len(counts), rng)
    boxes, first = drawn_boxes(sum(counts), C, rng, lo, hi), offsets(counts)
    if aimed:
        aim(preds, cfg, boxes, first, rng)
    return dict(cfg=cfg, preds=preds, boxes=boxes, first=first, opts=opts, ties=False)


def crafted(cfg, preds, boxes, counts, ties, **opts):
    return dict(cfg=cfg, preds=preds, boxes=np.asarray(boxes, np.float64).reshape(-1, 5), first=offsets(counts), opts=opts, ties=ties)


# ---- 1. many selection rounds ------------------------------------------------------------------------------------------------------------
def many_rounds(topk, radius, seed):
    return lambda: random_case([(6, 8), (12, 16)], 3, 3, [1, 4], seed, aimed=True, lo=.3, hi=.6, topk=topk, radius=radius)


# ---- 2. k_g == E_g: eight anchors that ARE the box, in the one eligible cell ----------------------------------------------------------------
def k_equals_e(topk):
    def build():
        # 4 x 4, the box on the centre of cell (row 2, col 1) and two cells wide: the neighbours' centres lie ON its edges (dx == w / 2, not
        # inside) and at exactly radius / W (not inside either), so E = 8; every IoU is 0.25 / 0.25 = 1
        cfg = net([(4, 4)], 8, 2, anchors=[[(.5, .5)] * 8])
        return crafted(cfg, zero_preds(cfg, 1), [[1, .375, .625, .5, .5]], [1], True, topk=topk, radius=1.0)
    return build


# ---- 3. the three tie levels of a round -------------------------------------------------------------------------------------------------
def tie_one_wave(topk):
    # 16 x 16, anchor (1, 1), the box on the edge between columns 7 and 8 of row 7: j = 119 and 120 tie (one wave), then 103, 104, 135, 136
    def build():
        cfg = net([(16, 16)], 1, 1, anchors=[[(1., 1.)]])
        return crafted(cfg, zero_preds(cfg, 1), [[0, .5, 7.5 / 16, 1., 1.]], [1], True, topk=topk)
    return build


def tie_two_waves(topk):
    # 16 x 16, the box on the corner of cells 119, 120 (wave 1) and 135, 136 (wave 2)
    def build():
        cfg = net([(16, 16)], 1, 1, anchors=[[(1., 1.)]])
        return crafted(cfg, zero_preds(cfg, 1), [[0, .5, .5, 1., 1.]], [1], True, topk=topk)
    return build


def tie_own_entries(topk):
    # 2 x 256: the rows mirror each other in the box's y = 0.5, and row 1 of a column is j + 256 of its row 0 - one lane's two entries
    def build():
        cfg = net([(2, 256)], 1, 1, anchors=[[(.25, 1.)]])
        return crafted(cfg, zero_preds(cfg, 1), [[0, 37.5 / 256, .5, .25, 1.]], [1], True, topk=topk)
    return build


# ---- 4. two rows of equal geometry and different class want the same candidates at bit-equal costs -----------------------------------------
def cross_box_tie(order):
    def build():
        cfg = net([(4, 4)], 2, 2, anchors=[[(.3, .3), (.2, .4)]])
        rows = np.array([[0, .375, .625, .3, .3], [1, .375, .625, .3, .3]])[list(order)]
        return crafted(cfg, zero_preds(cfg, 1), rows, [2], True)
    return build


# ---- 5. negative costs ----------------------------------------------------------------------------------------------------------------
def saturated(cfg, n):
    """objectness and class logits 80: s = 1 exactly, q = 1, Z = 100 C, and for C = 1 the class cost is (100 - 100) - 0 = 0"""
    preds = zero_preds(cfg, n)
    for p in preds:
        p[..., 4:] = 80.
    return preds


def negative_in_selection():
    # cell (0, 0) of 2 x 2 decodes to (.25, .25) with its anchors' sizes: IoUs 1, 0.875, 0.75 - k = 2 takes the costs 3 * -log(1 + 1e-8) < 0
    # and 3 * -log(0.875 + 1e-8) > 0
    cfg = net([(2, 2)], 3, 1, anchors=[[(.5, .5), (.5, .4375), (.5, .375)]])
    return crafted(cfg, saturated(cfg, 1), [[0, .25, .25, .5, .5]], [1], False)


def _near_zero_x(cfg):
    """preds whose cell (0, 0) decodes to bx of about 1e-6, where float32 still tells 1e-9 apart; -> (preds, bx)"""
    preds = saturated(cfg, 1)
    preds[0][0, 0, 0, 0, 0] = -13.
    return preds, float(simota._sig(np.float64(np.float32(-13.))) / 2)


def negative_contenders():
    # two boxes 1e-9 and 2e-9 beside the candidate: IoUs 1 - 4e-9 and 1 - 8e-9, the costs about -1.8e-8 and -6e-9; the labels tell the
    # owner by float32(x)
    cfg = net([(2, 2)], 1, 1, anchors=[[(.5, .5)]])
    preds, bx = _near_zero_x(cfg)
    return crafted(cfg, preds, [[0, bx + 2e-9, .25, .5, .5], [0, bx + 1e-9, .25, .5, .5]], [2], False, topk=1)


def negative_contenders_equal():
    # the classes -0.5 and 0 both truncate to 0: different rows, the same box, bit-equal negative costs; the lower row owns
    cfg = net([(2, 2)], 1, 1, anchors=[[(.5, .5)]])
    preds, bx = _near_zero_x(cfg)
    return crafted(cfg, preds, [[-.5, bx + 1e-9, .25, .5, .5], [0, bx + 1e-9, .25, .5, .5]], [2], True, topk=1)


# ---- 6. the workspace strip, either side of YK_OTA_LDS_CANDS = 6144 ------------------------------------------------------------------------
STRIP = [(32, 64), (1, 1)]


# ---- 7. four ragged layers ----------------------------------------------------------------------------------------------------------------
FOUR = [(3, 5), (5, 7), (7, 9), (9, 11)]
FOUR_A = [1, 8, 3, 2]


# ---- 8. tile sizes of ota_prep ----------------------------------------------------------------------------------------------------------
def tile(C, seed):
    def build():
        c = random_case([(2, 3)], 2, C, [2], seed)
        if C >= 600:
            c['boxes'][:, 0] = [0, C - 1]
        return c
    return build


def prep_tile(C):
    """tc of ota_prep"""
    return min(256, 6000 // (C + 1))


# ---- 9. ota_clear ------------------------------------------------------------------------------------------------------------------------
def big_clear():
    # 52 x 19 x 23 x 3 x 85 = 5.8M floats: past 4096 workgroups x 256 lanes x 4 floats, so the grid-stride loop runs; boxes in three images
    counts = [0] * 52
    counts[0], counts[25], counts[51] = 2, 3, 1
    return random_case([(19, 23)], 3, 80, counts, 31)


# ---- 10. the largest n -------------------------------------------------------------------------------------------------------------------
def n_65535():
    counts = np.zeros(65535, np.int64)
    counts[[0, 30000, 65534]] = 1
    return random_case([(1, 1)], 1, 1, counts, 32, max_boxes=1)


# ---- 11. hostile offsets: called with n_boxes = the row count ---------------------------------------------------------------------------------
def hostile(first, seed):
    def build():
        c = random_case(TWO, 3, 3, [5] + [0] * (len(first) - 2), seed)
        c['first'] = np.asarray(first, np.int32)
        return c
    return build


# ---- 12. status ------------------------------------------------------------------------------------------------------------------------
def with_rows(counts, rows, seed, **opts):
    """a random case on TWO with some rows of `boxes` replaced: {row: (column, value) or a whole row}"""
    def build():
        c = random_case(TWO, 3, 3, counts, seed, **opts)
        for g, what in rows.items():
            if len(what) == 2:
                c['boxes'][g, what[0]] = what[1]
            else:
                c['boxes'][g] = what
        return c
    return build


NAN, INF = math.nan, math.inf
HOSTILE_ROWS = {0: (0, -.5), 1: (0, 2.9), 2: (0, 3.), 3: (0, NAN), 4: (1, INF), 5: (1, -INF), 6: (2, NAN), 7: (2, INF), 8: (1, 1e-9),
                9: (3, 0.), 10: (3, -.2), 11: (3, 1.5), 12: (3, NAN), 13: (4, NAN), 14: (3, INF), 15: (4, -INF), 16: (3, -INF), 17: (4, INF), 18: (1, NAN)}
HOSTILE_VALID = [0, 1, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19]            # row 19 is left as drawn


# ---- 14. degenerate decodes ------------------------------------------------------------------------------------------------------------
def degenerate(seed):
    def build():
        rng = np.random.default_rng(seed)
        cfg = net([(5, 7)], 3, 4, rng)
        preds = drawn_preds(cfg, 2, rng)
        p = preds[0]
        p[0, ..., 2] = -800.                                                 # image 0: every bw is 0, every IoU 0, S = 0, k = 1
        u = rng.random(p.shape[1:4])
        p[1, ..., 2] = np.select([u < .3, u < .5, u < .6], [-800., 90., 800.], p[1, ..., 2])
        u = rng.random(p.shape[1:4])
        p[1, ..., 3] = np.select([u < .3, u < .5, u < .6], [-800., 800., 90.], p[1, ..., 3])
        # (where every IoU is 0 the cost no longer depends on the box: two boxes of one class tie bit for bit, and the lower row owns)
        return dict(cfg=cfg, preds=preds, boxes=drawn_boxes(5, 4, rng), first=offsets([2, 3]), opts={}, ties=True)
    return build


BUILDERS = {
    'rounds-topk-10': many_rounds(10, 2.5, 3),
    'rounds-topk-32-radius-16': many_rounds(32, 16., 3),
    'k-equals-E-topk-32': k_equals_e(32),
    'k-equals-E-topk-3': k_equals_e(3),
    'tie-in-one-wave-topk-1': tie_one_wave(1),
    'tie-in-one-wave-topk-4': tie_one_wave(4),
    'tie-across-waves-topk-1': tie_two_waves(1),
    'tie-across-waves-topk-4': tie_two_waves(4),
    'tie-of-one-lane-j-and-j+256-topk-1': tie_own_entries(1),
    'tie-of-one-lane-j-and-j+256-topk-4': tie_own_entries(4),
    'cross-box-tie-class-0-first': cross_box_tie((0, 1)),
    'cross-box-tie-class-1-first': cross_box_tie((1, 0)),
    'negative-cost-in-a-selection-of-2': negative_in_selection,
    'negative-costs-contend': negative_contenders,
    'negative-costs-contend-bit-equal': negative_contenders_equal,
    'N-6144-the-last-in-LDS': lambda: random_case(STRIP[:1], 3, 1, [2], 21),
    'N-6145-the-first-on-the-strip': lambda: random_case(STRIP, [3, 1], 1, [2], 22),
    'N-6147-strips-of-3-images-max_boxes-3': lambda: random_case(STRIP, 3, 2, [2, 0, 3], 23, max_boxes=3),
    'N-6147-strips-of-3-images-max_boxes-64': lambda: random_case(STRIP, 3, 2, [2, 0, 3], 23),
    'four-ragged-layers-C3': lambda: random_case(FOUR, FOUR_A, 3, [3, 2, 3], 24, aimed=True, lo=.2, hi=.6),
    'four-ragged-layers-C30': lambda: random_case(FOUR, FOUR_A, 30, [3, 2, 3], 50, aimed=True, lo=.2, hi=.6),
    'tile-C22': tile(22, 26), 'tile-C23': tile(23, 26), 'tile-C600': tile(600, 27), 'tile-C2999': tile(2999, 28), 'tile-C4096': tile(4096, 29),
    'clear-1x1': lambda: random_case([(1, 1)], 1, 1, [1], 30),
    'clear-mid': lambda: random_case(TWO, 3, 3, [2, 0, 3], 30),
    'clear-grid-stride-5.8M': big_clear,
    'n-65535': n_65535,
    'offsets-descending-then-past-the-end': hostile([0, 2, 1, 9], 33),
    'offsets-negative': hostile([-3, 2, 5], 34),
    'status-invalid-in-images-1-and-2': with_rows([2, 3, 3], {6: (0, 7.), 3: (1, 1.), 4: (2, -.01)}, 35),
    'status-overflow-in-image-0-invalid-in-image-1': with_rows([3, 2], {4: (0, -1.)}, 36, max_boxes=2),
    'status-hostile-values': with_rows([20], HOSTILE_ROWS, 64),
    'contention-256-boxes': lambda: random_case([(4, 4)], 3, 2, [256, 3], 38, max_boxes=256),
    'degenerate-decodes': degenerate(39),
}
DIRECT = ['N-6147-strips-of-3-images-max_boxes-3', 'N-6147-strips-of-3-images-max_boxes-64', 'offsets-descending-then-past-the-end',
          'offsets-negative']                                                # called through yk_assign_simota_f32 itself
LARGE = ['clear-grid-stride-5.8M', 'n-65535']                                # compared on the device, one call
ENGINE = [n for n in BUILDERS if n not in DIRECT and n not in LARGE]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def rule(name):
    """-> (labels, npos, status, margin, detail) of simota.assign on the case"""
    c, detail = case(name), []
    return simota.assign(c['preds'], c['boxes'], c['first'], c['cfg'], detail=detail, **c['opts']) + (detail,)


def n_candidates(cfg):
    return sum(h * w * len(a) for (h, w), a in zip(cfg['out_hw'], cfg['anchors']))


def layer_of(cfg, j):
    for l, ((h, w), a) in enumerate(zip(cfg['out_hw'], cfg['anchors'])):
        if j < h * w * len(a):
            return l
        j -= h * w * len(a)
    raise IndexError(j)


def nonzero_gap(detail, boxes):
    """The rule's margin over the decisions that are not exact ties: the smallest NONZERO gap between the k-th and the (k + 1)-th cost of a
    box, between the costs contending for a candidate, and between S and the integers whose crossing changes k."""
    gap, by_row = math.inf, {r['g']: r for r in detail}
    for r in detail:
        m = math.floor(r['S'])
        gap = min([gap] + [abs(r['S'] - v) for v in (m, m + 1) if 2 <= v <= r['E'] and r['S'] != v])
        cost = np.sort(r['cost'])
        if r['E'] > r['k'] and cost[r['k']] != cost[r['k'] - 1]:
            gap = min(gap, float(cost[r['k']] - cost[r['k'] - 1]))
        for j, c in zip(r['j'], r['j_cost']):
            for g in r.get('rivals', {}).get(j, []):
                other = by_row[g]['j_cost'][by_row[g]['j'].index(j)]
                if other != c:
                    gap = min(gap, abs(other - c))
    return gap


def permuted(c):
    """the same case with every image's box rows in the reverse order"""
    boxes = c['boxes'].copy()
    for s in range(len(c['first']) - 1):
        b0, b1 = int(c['first'][s]), int(c['first'][s + 1])
        boxes[b0:b1] = boxes[b0:b1][::-1]
    return dict(c, boxes=boxes)


def appended(c, seed=0):
    """the same case with one more image at the end of the batch: drawn predictions, a copy of the first image's boxes"""
    rng = np.random.default_rng(seed)
    preds = [np.concatenate([p, rng.normal(0, 1, p[:1].shape).astype(np.float32)]) for p in c['preds']]
    extra = c['boxes'][int(c['first'][0]):int(c['first'][1])]
    first = np.concatenate([c['first'], [c['first'][-1] + len(extra)]]).astype(np.int32)
    return dict(c, preds=preds, boxes=np.concatenate([c['boxes'][:int(c['first'][-1])], extra]), first=first)
