"""The cases tests/test_gpu_simota.py holds engine.assign_simota to simota.assign on: a plain table, and `build`, which fills a case's
predictions and boxes from numpy.random.default_rng(seed).  `random`: predictions and boxes are all drawn, and the test asserts the rule's
margin > 1e-9 first (the seeds were chosen on the CPU for it); the crafted cases carry exact ties, which the same arithmetic decides on
both sides.  `counts` is boxes per image; `boxes` replaces the drawn rows of the LAST image."""
import numpy as np

TWO = [(2, 3), (4, 6)]
CASES = [
    dict(id='1x1-one-box', out_hw=[(1, 1)], A=1, C=1, counts=[1], seed=1, random=True),
    dict(id='empty-image-between', out_hw=TWO, A=3, C=3, counts=[2, 0, 3], seed=2, random=True),
    dict(id='two-layers-1-to-5-boxes', out_hw=TWO, A=3, C=3, counts=[1, 5, 3], seed=3, random=True),
    dict(id='two-layers-topk-1', out_hw=TWO, A=3, C=3, counts=[4, 2], seed=4, random=True, topk=1),
    dict(id='two-layers-topk-32', out_hw=TWO, A=3, C=3, counts=[4, 2], seed=5, random=True, topk=32, radius=1.0),
    dict(id='5x7-C20-under-one-pass', out_hw=[(5, 7)], A=3, C=20, counts=[3, 4], seed=6, random=True),
    dict(id='19x23-C80-ragged-passes', out_hw=[(19, 23)], A=3, C=80, counts=[4], seed=7, random=True),
    dict(id='70-boxes-at-max_boxes', out_hw=[(13, 13)], A=3, C=2, counts=[70], seed=8, random=True, max_boxes=70),
    dict(id='70-boxes-max_boxes-plus-1', out_hw=[(13, 13)], A=3, C=2, counts=[2, 70], seed=9, random=True, max_boxes=69),
    dict(id='76x76-past-the-LDS-strip-of-6144', out_hw=[(76, 76)], A=3, C=1, counts=[3], seed=10, random=True),
    dict(id='box-smaller-than-a-cell', out_hw=[(4, 4)], A=1, C=2, counts=[1], seed=11, radius=1.0, boxes=[[1, .375, .625, .01, .01]]),
    dict(id='box-covering-the-frame', out_hw=TWO, A=3, C=3, counts=[1], seed=12, boxes=[[2, .5, .5, 1., 1.]]),
    dict(id='duplicate-boxes', out_hw=TWO, A=3, C=3, counts=[3], seed=13, boxes=[[1, .4, .6, .5, .3], [0, .7, .2, .2, .2], [1, .4, .6, .5, .3]]),
    dict(id='class-out-of-range', out_hw=TWO, A=3, C=3, counts=[2, 3], seed=14, boxes=[[0, .4, .6, .5, .3], [3, .5, .5, .2, .2], [-1.5, .5, .5, .2, .2]]),
    dict(id='centre-outside-a-grid', out_hw=TWO, A=3, C=3, counts=[3], seed=15, boxes=[[0, .4, .6, .5, .3], [1, 1., .5, .2, .2], [1, .5, -.1, .2, .2]]),
    dict(id='logits-80-tw-90-800', out_hw=[(5, 7)], A=3, C=20, counts=[3, 2], seed=16, extreme=True),
]


def build(case):
    """-> (cfg dict for simota.assign / engine.make_ota_cfg, preds per layer float32, boxes [N, 5] float64, first, the rule's options)"""
    rng = np.random.default_rng(case['seed'])
    A, C, n = case['A'], case['C'], len(case['counts'])
    cfg = dict(out_hw=case['out_hw'], anchors=rng.uniform(.05, .9, (len(case['out_hw']), A, 2)), class_num=C)
    preds = [(rng.normal(0, 1.5, (n, h, w, A, 5 + C)) * np.r_[1, 1, .3, .3, np.ones(1 + C)]).astype(np.float32) for h, w in case['out_hw']]
    if case.get('extreme'):
        for p in preds:
            p[..., 4:] = np.where(rng.random(p[..., 4:].shape) < .5, 80, -80)
            p[..., 2] = np.where(rng.random(p[..., 2].shape) < .3, 90, p[..., 2])
            p[..., 3] = np.where(rng.random(p[..., 3].shape) < .3, 800, p[..., 3])
    N = sum(case['counts'])
    boxes = np.stack([rng.integers(0, C, N), rng.uniform(.1, .9, N), rng.uniform(.1, .9, N), rng.uniform(.05, .6, N), rng.uniform(.05, .6, N)], 1).astype(np.float64)
    if 'boxes' in case:
        boxes[N - len(case['boxes']):] = case['boxes']
    opts = {k: case[k] for k in ('topk', 'radius', 'max_boxes') if k in case}
    return cfg, preds, boxes, np.concatenate([[0], np.cumsum(case['counts'])]).astype(np.int32), opts
