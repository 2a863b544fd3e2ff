"""Trainer(assign='simota'): the step builds its label grids from its own predictions, on tests/mini_net.py with ciou."""
import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import simota

pytestmark = pytest.mark.gpu
B, MAXB = 4, 8


def _batch(seed, counts):
    """(frames, boxes [N, 5], first) of B images with `counts` boxes each."""
    rng = np.random.default_rng(seed)
    N = sum(counts)
    boxes = np.stack([rng.integers(0, 20, N), rng.uniform(.2, .8, N), rng.uniform(.2, .8, N), rng.uniform(.1, .6, N), rng.uniform(.1, .6, N)], 1).astype(np.float64)
    return rng.uniform(0, 1, (B, 32, 32, 3)).astype(np.float32), boxes, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _box_batch(boxes, first):
    from k210_yolo_framework_amd import engine
    padded = np.zeros((B * MAXB, 5))
    padded[:len(boxes)] = boxes
    return engine.BoxBatch(torch.from_numpy(padded).cuda(), torch.from_numpy(first).cuda())


def test_step_equals_a_best_step_fed_the_rule_s_grids_bit_for_bit():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, _, _ = mini_case(6, B=B)
    x, boxes, first = _batch(21, [2, 0, 5, 1])
    xs = torch.from_numpy(x).cuda()
    tr = Trainer(spec, w, h.anchors, B, use_graph=False, box_loss='ciou', assign='simota', ota_max_boxes=MAXB)
    r = tr.loss_and_grads(xs, _box_batch(boxes, first))
    preds = [p.cpu().numpy() for p in tr.forward(xs)]                  # the same weights and frames: the step's own outputs
    labels, npos, status, margin = simota.assign(preds, boxes, first, h, max_boxes=MAXB)
    assert margin > 1e-9 and status == simota.STATUS_CLEAN and npos.sum() > 0
    assert tr._ota_out[1].cpu().numpy().tolist() == npos.tolist()
    ref = Trainer(spec, w, h.anchors, B, use_graph=False, box_loss='ciou')
    q = ref.loss_and_grads(xs, [torch.from_numpy(l).cuda() for l in labels])
    assert all(torch.equal(a, b) for a, b in zip(r['layers'], q['layers'])) and torch.equal(tr.G, ref.G)
    assert float(r['layers'][0][0]) > 0 and bool(tr.G.abs().sum() > 0)


def test_replayed_steps_equal_eager_steps_on_batches_of_different_box_counts():
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, _, _ = mini_case(7, B=B)
    batches = [_batch(30 + i, c) for i, c in enumerate([[1, 2, 3, 1], [0, 8, 0, 2], [4, 4, 4, 4], [1, 0, 0, 0]])]
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, B, use_graph=graph, box_loss='ciou', assign='simota', ota_max_boxes=MAXB, ota_topk=5)
        outs = [tr.step(torch.from_numpy(x).cuda(), _box_batch(b, f)) for x, b, f in batches]       # eager, captured + replayed, replayed ..
        assert all(o['ota_status'] == simota.STATUS_CLEAN and o['pos'] > 0 for o in outs)
        runs.append(([(o['loss'], o['pos']) for o in outs], tr.G.cpu().numpy(), tr.P.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and len({p for _, p in runs[0][0]}) > 1
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_mse_box_loss_is_refused_by_name():
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.train import Trainer
    from tests.qat_ref import mini_case
    spec, w, h, _, _ = mini_case(6, B=B)
    with pytest.raises(engine.YkError, match="assign='simota' with box_loss='mse'"):
        Trainer(spec, w, h.anchors, B, assign='simota')
