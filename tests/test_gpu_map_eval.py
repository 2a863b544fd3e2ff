"""map_gpu.MapEvaluator (csrc/yk_map.hip) against voc_eval.evaluate on the same inputs: flags, n_gt, n_det, tp, fp exactly equal, the
same NaN pattern in `ap`, and `ap` / `map` within 1e-12 absolute (AP is a sum of at most n_gt non-negative float64 terms that total
<= 1: any summation order differs by at most n_gt * 2^-52, below 1e-12 for n_gt <= 4096; every case here stays under 4096).

voc_eval.evaluate returns no per-row flags, so `reference_flags` restates its matching loop and returns them; every comparison first
checks that the restated loop reproduces evaluate's own tp / fp counts."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, netspec as ns, voc_eval

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / 'golden'
ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-12


def reference_flags(dets, gts, class_num, iou_thresh=0.5, difficult=None, plus_one=False):
    """voc_eval.evaluate's matching, returning one flag per row of every image (0 ignored, 1 tp, 2 fp)."""
    dets = [np.asarray(d, np.float64).reshape(-1, 6) for d in dets]
    gts = [np.asarray(g, np.float64).reshape(-1, 6) for g in gts]
    diff = [np.zeros(len(g), bool) if difficult is None else np.asarray(difficult[i], bool) for i, g in enumerate(gts)]
    flags = [np.zeros(len(d), np.uint8) for d in dets]
    for c in range(class_num):
        sel = [g[:, -1].astype(int) == c for g in gts]
        taken = [np.zeros(int(s.sum()), bool) for s in sel]
        rows = [(d[k, 4], i, k) for i, d in enumerate(dets) for k in np.nonzero(d[:, 5].astype(int) == c)[0]]
        for k in sorted(range(len(rows)), key=lambda k: -rows[k][0]):
            _, i, r = rows[k]
            g = gts[i][sel[i], :4]
            best, j = -1.0, -1
            if len(g):
                iou = voc_eval.box_iou(dets[i][r, :4], g, plus_one)
                j = int(np.argmax(iou))
                best = float(iou[j])
            if best >= iou_thresh:
                if diff[i][sel[i]][j]:
                    continue
                if not taken[i][j]:
                    flags[i][r] = 1
                    taken[i][j] = True
                else:
                    flags[i][r] = 2
            else:
                flags[i][r] = 2
    return flags


def pack(dets):
    dets = [np.asarray(d, np.float32).reshape(-1, 6) for d in dets]
    off = np.zeros(len(dets) + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in dets])
    return (np.concatenate(dets) if dets else np.zeros((0, 6), np.float32)), off


def compare(got, dets, gts, class_num, iou_thresh=0.5, use_07_metric=False, difficult=None, plus_one=False):
    dets32 = [np.asarray(d, np.float32).reshape(-1, 6) for d in dets]                 # the rows the device holds
    ref = voc_eval.evaluate(dets32, gts, class_num, iou_thresh, use_07_metric, difficult, plus_one)
    flags = reference_flags(dets32, gts, class_num, iou_thresh, difficult, plus_one)
    cat = np.concatenate(flags) if flags else np.zeros(0, np.uint8)
    cls = np.concatenate([d[:, 5].astype(int) for d in dets32]) if dets32 else np.zeros(0, int)
    for c in range(class_num):                                                         # the restated loop is evaluate's
        assert int((cat[cls == c] == 1).sum()) == ref['tp'][c] and int((cat[cls == c] == 2).sum()) == ref['fp'][c]
    assert np.array_equal(got['flags'], cat), (got['flags'], cat)
    for k in ('n_gt', 'n_det', 'tp', 'fp'):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert np.array_equal(np.isnan(got['ap']), np.isnan(ref['ap']))
    have = ~np.isnan(ref['ap'])
    err = float(np.abs(got['ap'][have] - ref['ap'][have]).max()) if have.any() else 0.0
    print('ap error', err, 'map', got['map'], ref['map'])
    assert err <= TOL
    if np.isnan(ref['map']):
        assert np.isnan(got['map'])
    else:
        assert abs(got['map'] - ref['map']) <= TOL
    return ref


def run_gpu(dets, gts, class_num, iou_thresh=0.5, use_07_metric=False, difficult=None, plus_one=False):
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    ev = MapEvaluator(class_num, iou_thresh, use_07_metric, plus_one)
    rows, off = pack(dets)
    ev.add(rows, off, gts, difficult)
    return ev.result()


def check(dets, gts, class_num, **kw):
    got = run_gpu(dets, gts, class_num, **kw)
    compare(got, dets, gts, class_num, **kw)
    return got


def D(*rows):
    return np.asarray(rows, np.float64).reshape(-1, 6)


# ---- 1. hand-made cases --------------------------------------------------------------------------------------------------------------
def test_iou_exactly_at_the_threshold_is_a_true_positive():
    got = check([D([0, 0, 2, 2, .9, 0])], [D([0, 0, 2, 1, 1, 0])], 1, iou_thresh=0.5)
    assert got['flags'].tolist() == [1] and got['ap'][0] == 1.0


def test_equal_iou_takes_the_first_box_and_a_taken_box_gives_no_second_chance():
    gts = [D([0, 0, 2, 1, 1, 0], [0, 1, 2, 2, 1, 0])]                                 # both IoU 0.5 with the detection
    got = check([D([0, 0, 2, 2, .9, 0], [0, 0, 2, 2, .8, 0])], gts, 1)
    assert got['flags'].tolist() == [1, 2]                                            # both argmax box 0; box 1 stays free
    # the second detection's best box is taken; the free box has IoU 2/3 >= 0.5 but is not the best: false positive
    got = check([D([0, 0, 10, 10, .9, 0], [0, 0, 10, 10, .8, 0])], [D([0, 0, 10, 10, 1, 0], [0, 2, 10, 12, 1, 0])], 1)
    assert got['flags'].tolist() == [1, 2] and got['tp'][0] == 1


def test_difficult_best_match_is_ignored_and_not_counted():
    gts = [D([0, 0, 10, 10, 1, 0], [20, 20, 30, 30, 1, 0])]
    got = check([D([0, 0, 10, 10, .9, 0], [20, 20, 30, 30, .8, 0])], gts, 1, difficult=[np.array([True, False])])
    assert got['flags'].tolist() == [0, 1] and got['n_gt'][0] == 1


def test_zero_area_boxes_have_union_zero():
    got = check([D([1, 1, 1, 1, .9, 0], [3, 3, 5, 5, .8, 0])], [D([1, 1, 1, 1, 1, 0])], 1)
    assert got['flags'].tolist() == [2, 2]
    got = check([D([1, 1, 1, 1, .9, 0])], [D([1, 1, 1, 1, 1, 0])], 1, plus_one=True)  # one pixel each with the devkit's convention
    assert got['flags'].tolist() == [1]


def test_classes_without_detections_or_without_ground_truth():
    dets = [D([0, 0, 10, 10, .9, 0], [0, 0, 5, 5, .7, 2])]
    gts = [D([0, 0, 10, 10, 1, 0], [5, 5, 9, 9, 1, 1])]
    got = check(dets, gts, 3)
    assert got['ap'][0] == 1.0 and got['ap'][1] == 0.0 and np.isnan(got['ap'][2]) and got['map'] == 0.5
    assert got['flags'].tolist() == [1, 2]


def test_no_detections_and_no_ground_truth():
    empty = np.zeros((0, 6))
    got = check([empty, empty], [D([0, 0, 10, 10, 1, 0]), empty], 2)
    assert got['map'] == 0.0 and len(got['flags']) == 0
    got = check([D([0, 0, 10, 10, .9, 0]), empty], [empty, empty], 2)
    assert np.isnan(got['map']) and got['flags'].tolist() == [2]
    got = check([], [], 2)
    assert np.isnan(got['map'])


def test_an_image_without_rows_between_two_others():
    dets = [D([0, 0, 10, 10, .9, 0]), np.zeros((0, 6)), D([0, 0, 10, 10, .8, 0], [50, 50, 60, 60, .95, 0])]
    gts = [D([0, 0, 10, 10, 1, 0]), D([0, 0, 10, 10, 1, 0]), D([1, 1, 10, 10, 1, 0])]
    got = check(dets, gts, 1)
    assert got['flags'].tolist() == [1, 1, 2] and got['n_gt'][0] == 3


@pytest.mark.parametrize('use_07', [False, True])
def test_score_ties_keep_row_order_inside_and_across_images(use_07):
    box, far = [0, 0, 10, 10], [50, 50, 60, 60]
    # image 0: two equal scores on one box (the first row wins), then -0.0 before +0.0 on another box (equal keys: the first row wins)
    dets = [D(box + [.5, 0], box + [.5, 0], [20, 20, 30, 30, -0.0, 0], [20, 20, 30, 30, 0.0, 0]),
            D(far + [.5, 0], box + [.5, 0]),                                          # image 1: a false positive BEFORE a true positive, same score
            D(box + [0.0, 0], box + [-0.0, 0])]
    gts = [D(box + [1, 0], [20, 20, 30, 30, 1, 0]), D(box + [1, 0]), D(box + [1, 0])]
    got = check(dets, gts, 1, use_07_metric=use_07)
    assert got['flags'].tolist() == [1, 2, 1, 2, 2, 1, 1, 2]


# ---- 2. seeded random sweep ----------------------------------------------------------------------------------------------------------
def random_case(rng, n_img, class_num, max_det=40, max_gt=6, size=100.0):
    scores = np.round(rng.uniform(0.05, 0.95, 8), 3)                                  # 8 distinct values: ties everywhere
    dets, gts, diff = [], [], []
    for _ in range(n_img):
        g = int(rng.integers(0, max_gt + 1))
        tl = rng.uniform(0, size * 0.7, (g, 2))
        gt = np.concatenate([tl, tl + rng.uniform(4, size * 0.3, (g, 2)), np.ones((g, 1)), rng.integers(0, class_num, (g, 1))], 1)
        n = int(rng.integers(0, max_det + 1))
        rows = []
        for _ in range(n):
            if g and rng.random() < 0.7:                                              # a jittered copy (duplicates of one box included)
                src = gt[int(rng.integers(0, g))]
                box = src[:4] + rng.normal(0, rng.choice([0.5, 3.0, 8.0]), 4)
                cls = src[5] if rng.random() < 0.9 else rng.integers(0, class_num)
            else:                                                                     # noise
                t = rng.uniform(0, size * 0.8, 2)
                box = np.concatenate([t, t + rng.uniform(2, size * 0.3, 2)])
                cls = rng.integers(0, class_num)
            rows.append([*box, rng.choice(scores), cls])
        dets.append(np.asarray(rows, np.float32).reshape(-1, 6))
        gts.append(gt)
        diff.append(rng.random(g) < 0.2)
    return dets, gts, diff


@pytest.mark.parametrize('class_num', [1, 3, 20])
@pytest.mark.parametrize('n_img', [1, 2, 7, 33])
def test_random_sweep(n_img, class_num):
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    rng = np.random.default_rng(1000 * n_img + class_num)
    dets, gts, diff = random_case(rng, n_img, class_num)
    rows, off = pack(dets)
    for plus_one in (False, True):
        for use_07 in (False, True):
            for iou in (0.3, 0.5):
                ev = MapEvaluator(class_num, iou, use_07, plus_one)
                ev.add(rows, off, gts, diff)
                compare(ev.result(), dets, gts, class_num, iou, use_07, diff, plus_one)


# ---- 3. size boundaries --------------------------------------------------------------------------------------------------------------
def test_one_class_of_3000_detections_over_64_images():
    rng = np.random.default_rng(5)
    dets, gts, diff = [], [], []
    for i in range(64):
        _, g, h = random_case(rng, 1, 1, max_det=0, max_gt=6)
        gts += g
        diff += h
        n = 47 if i < 56 else 46                                                      # 56 * 47 + 8 * 46 = 3000
        around = g[0][rng.integers(0, len(g[0]), n), :4] if len(g[0]) else np.tile([1., 1., 9., 9.], (n, 1))
        box = around + rng.normal(0, 4.0, (n, 4))
        dets.append(np.concatenate([box, rng.choice(np.linspace(0.1, 0.9, 8), (n, 1)), np.zeros((n, 1))], 1).astype(np.float32))
    assert sum(len(d) for d in dets) == 3000
    for use_07 in (False, True):
        got = check(dets, gts, 1, use_07_metric=use_07, difficult=diff)
        assert got['n_det'][0] == 3000 and 0 < got['tp'][0] < got['n_det'][0]


def test_one_group_of_200_detections_and_70_boxes():
    rng = np.random.default_rng(6)
    tl = rng.uniform(0, 400, (70, 2))
    gt = np.concatenate([tl, tl + rng.uniform(10, 40, (70, 2)), np.ones((70, 1)), np.zeros((70, 1))], 1)
    src = gt[rng.integers(0, 70, 200)]
    det = np.concatenate([src[:, :4] + rng.normal(0, 3.0, (200, 4)), rng.choice(np.linspace(0.1, 0.9, 8), (200, 1)), np.zeros((200, 1))], 1)
    hard = rng.random(70) < 0.2
    got = check([det.astype(np.float32)], [gt], 1, difficult=[hard])
    assert got['tp'][0] > 20 and got['fp'][0] > 20 and (got['flags'] == 0).any()


# ---- 4. accumulation and input forms --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def medium():
    dets, gts, diff = random_case(np.random.default_rng(77), 33, 5)
    return dets, gts, diff, voc_eval.evaluate(dets, gts, 5, difficult=diff)


def same(a, b):
    assert np.array_equal(a['flags'], b['flags'])
    for k in ('n_gt', 'n_det', 'tp', 'fp'):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a['ap'], b['ap'], equal_nan=True) and (a['map'] == b['map'] or (a['map'] != a['map'] and b['map'] != b['map']))


def test_uneven_batches_padded_and_device_inputs_and_reset(medium):
    import torch
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    dets, gts, diff, ref = medium
    rows, off = pack(dets)
    ev = MapEvaluator(5)
    ev.add(rows, off, gts, diff)
    whole = ev.result()
    compare(whole, dets, gts, 5, difficult=diff)
    assert abs(whole['map'] - ref['map']) <= TOL
    # five uneven batches (one of a single image, one that makes the device buffers grow)
    ev.reset()
    for lo, hi in ((0, 1), (1, 4), (4, 17), (17, 18), (18, 33)):
        r, o = pack(dets[lo:hi])
        ev.add(r, o, gts[lo:hi], diff[lo:hi])
    same(ev.result(), whole)
    # the padded form, as a device tensor, in two batches; then the packed form as device tensors
    cap = max(len(d) for d in dets) + 3
    pad = np.full((33, cap, 6), 7.0, np.float32)                                      # rows past the count must not be read as detections
    cnt = np.array([len(d) for d in dets], np.int32)
    for b, d in enumerate(dets):
        pad[b, :len(d)] = d
    ev2 = MapEvaluator(5)
    ev2.add(torch.from_numpy(pad[:20]).cuda(), torch.from_numpy(cnt[:20]).cuda(), gts[:20], diff[:20])
    ev2.add(pad[20:], cnt[20:], gts[20:], diff[20:])
    same(ev2.result(), whole)
    ev2.reset()                                                                       # reset, then reuse
    ev2.add(torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda(), gts, diff)
    same(ev2.result(), whole)
    got_rows, got_img = ev2.rows()
    assert np.array_equal(got_rows, rows) and np.array_equal(got_img, np.repeat(np.arange(33), np.diff(off)))


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(medium):
    dets, gts, diff, _ = medium
    for use_07 in (False, True):
        a = run_gpu(dets, gts, 5, use_07_metric=use_07, difficult=diff)
        b = run_gpu(dets, gts, 5, use_07_metric=use_07, difficult=diff)
        assert a['ap'].tobytes() == b['ap'].tobytes() and np.float64(a['map']).tobytes() == np.float64(b['map']).tobytes()
        assert np.array_equal(a['flags'], b['flags'])


# ---- 6. end to end: Pipeline detections scored where they are ------------------------------------------------------------------------
def views(img: np.ndarray, n: int, seed: int = 7) -> np.ndarray:
    """n seeded views [n,224,320,3] u8 of one picture (tests/test_gpu_map.py's helper, restated)."""
    rng = np.random.default_rng(seed)
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    src = img.astype(np.float64)
    for k in range(n):
        s, th = rng.uniform(0.7, 1.5), np.deg2rad(rng.uniform(-12, 12))
        tx, ty = rng.uniform(-0.15, 0.15) * W, rng.uniform(-0.15, 0.15) * H
        flip = rng.random() < 0.5
        c, sn = np.cos(th) / s, np.sin(th) / s
        u = c * (xx - W / 2) - sn * (yy - H / 2) + W / 2 - tx
        v = sn * (xx - W / 2) + c * (yy - H / 2) + H / 2 - ty
        if flip:
            u = W - 1 - u
        u0, v0 = np.floor(u).astype(int), np.floor(v).astype(int)
        fu, fv = (u - u0)[..., None], (v - v0)[..., None]
        ok = ((u0 >= 0) & (u0 < W - 1) & (v0 >= 0) & (v0 < H - 1))[..., None]
        u0, v0 = np.clip(u0, 0, W - 2), np.clip(v0, 0, H - 2)
        val = (src[v0, u0] * (1 - fu) * (1 - fv) + src[v0, u0 + 1] * fu * (1 - fv) + src[v0 + 1, u0] * (1 - fu) * fv + src[v0 + 1, u0 + 1] * fu * fv)
        val = np.where(ok, val, 127.0) * rng.uniform(0.7, 1.25) + rng.uniform(-25, 25)
        out[k] = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    out[0] = img
    return out


def test_pipeline_detections_are_scored_from_device_memory():
    import torch
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    gold = np.load(GOLD / 'kmodel_dog_golden.npz')
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    w, _ = kmodel.to_float_weights(kmodel.parse((GOLD / 'yolo.kmodel').read_bytes()))
    anchors = gold['anchors'].reshape(2, 3, 2).astype(np.float32)
    frames = torch.from_numpy(views(gold['image'].transpose(1, 2, 0).copy(), 32)).cuda()
    B = 16
    pipe = engine.Pipeline(spec, w, anchors, max_batch=B, depth=2)
    try:
        truth = []                                                                    # the f16x2 detections of a first run
        for k in range(0, 32, B):
            dets, counts, stream = pipe.submit(frames[k:k + B], obj_thresh=0.25, iou_thresh=0.5)
            stream.synchronize()
            truth += voc_eval.padded_rows(dets.cpu().numpy(), counts.cpu().numpy())
        assert sum(len(t) for t in truth) >= 32
        ev, host = MapEvaluator(20), []
        for k in range(0, 32, B):                                                     # a second run, scored straight from the slot's tensors
            dets, counts, stream = pipe.submit(frames[k:k + B], obj_thresh=0.25, iou_thresh=0.5)
            ev.add(dets, counts, truth[k:k + B], stream=stream)
            host += voc_eval.padded_rows(dets.cpu().numpy(), counts.cpu().numpy())
        got = ev.result()
    finally:
        pipe.close()
    compare(got, host, truth, 20)
    assert abs(got['map'] - 1.0) <= TOL                                               # the detections against themselves


# ---- 7. / 8. the command lines -------------------------------------------------------------------------------------------------------
NET = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5']


def train_args(tmp_path):
    return ['--synthetic', '32', '--batch_size', '4', '--max_nrof_epochs', '1', '--vaildation_split', '0.125', '--obj_weight', '1',
            '--noobj_weight', '1', '--wh_weight', '1', '--iou_thresh', '0.5', '--log_dir', str(tmp_path / 'log')] + NET


def check_dump(report, dump, class_num=20, iou=0.5):
    z = np.load(dump)
    split = lambda a, off: [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    n_img = len(z['gt_offsets']) - 1
    off = np.searchsorted(z['image'], np.arange(n_img + 1))
    dets, gts = split(z['rows'], off), split(z['gt'], z['gt_offsets'])
    ref = voc_eval.evaluate(dets, gts, class_num, iou)
    assert report['images'] == n_img and report['rows'] == len(z['rows'])
    assert report['n_gt'] == ref['n_gt'].tolist() and report['tp'] == ref['tp'].tolist() and report['fp'] == ref['fp'].tolist()
    for c in range(class_num):
        assert (report['ap'][c] is None) == bool(np.isnan(ref['ap'][c]))
        if report['ap'][c] is not None:
            assert abs(report['ap'][c] - ref['ap'][c]) <= TOL
    assert abs(report['map'] - ref['map']) <= TOL
    return ref


def test_cli_train_then_eval_writes_eval_json(tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import evaluate, training
    monkeypatch.chdir(ROOT)
    training.cli(train_args(tmp_path) + ['--max_steps', '2'])
    ck = list((tmp_path / 'log').glob('*/yolo_model.h5'))
    assert len(ck) == 1
    capsys.readouterr()
    rep = evaluate.main([str(ck[0]), '--synthetic', '32', '--obj_thresh', '0.0', '--dump_rows', str(tmp_path / 'rows.npz'), '--batch', '12'] + NET)
    text = capsys.readouterr().out
    out = ck[0].parent / 'eval.json'
    assert out.exists() and json.loads(out.read_text())['map'] == rep['map']
    assert 'mAP' in text and 'at most 30 detections per class and image' in text and 'class' in text
    assert rep['rows'] > 0                                                            # obj_thresh 0: an untrained head still gives rows
    check_dump(rep, tmp_path / 'rows.npz')


def test_cli_eval_of_a_kmodel_in_kpu_mode(tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import evaluate
    monkeypatch.chdir(ROOT)
    rep = evaluate.main([str(GOLD / 'yolo.kmodel'), '--precision', 'kpu', '--synthetic', '32', '--out', str(tmp_path / 'eval.json'),
                         '--dump_rows', str(tmp_path / 'rows.npz'), '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75'])
    assert json.loads((tmp_path / 'eval.json').read_text())['precision'] == 'kpu'
    check_dump(rep, tmp_path / 'rows.npz')


EPOCH_LINE = r'epoch 1: \d+ steps, mean loss [-\d.naif]+, val_loss [-\d.naif]+, [\d.]+s, input pipeline \d+ images/s/rank'


def test_training_cli_val_map_is_opt_in(tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import training
    monkeypatch.chdir(ROOT)
    training.cli(train_args(tmp_path) + ['--val_map', 'True'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch 1:')]
    assert len(line) == 1
    m = re.fullmatch(EPOCH_LINE + r', val_mAP (\d\.\d{4})', line[0])
    assert m, line[0]
    assert 0.0 <= float(m.group(1)) <= 1.0
    training.cli(train_args(tmp_path) + ['--val_map', 'False'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch 1:')]
    assert len(line) == 1 and re.fullmatch(EPOCH_LINE, line[0]) and 'val_mAP' not in line[0], line
