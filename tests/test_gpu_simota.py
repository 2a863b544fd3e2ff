"""engine.assign_simota (csrc/yk_ota.hip) against the rule, simota.assign, decision for decision, on tests/simota_cases.py."""
import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import simota
from tests.simota_cases import CASES, build

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_assignment_equals_the_rule_and_two_calls_give_the_same_bytes(case):
    from k210_yolo_framework_amd import engine
    cfg, preds, boxes, first, opts = build(case)
    want, npos, status, margin = simota.assign(preds, boxes, first, cfg, **opts)
    if case.get('random'):
        assert margin > 1e-9, margin                                  # a condition on the inputs: the two sides may differ by ulps of exp / log
    ocfg = engine.make_ota_cfg(cfg, **opts)
    dev = [torch.from_numpy(p).cuda() for p in preds]
    # the capacity of the box buffer is larger than the count, as in a captured step; the rows past the last offset are never read
    padded = np.concatenate([boxes, np.full((3, 5), np.nan)])
    got, gnpos, gstatus = engine.assign_simota(dev, padded, first, ocfg)
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.cpu().numpy(), w), (l, np.argwhere(g.cpu().numpy() != w)[:5])
    assert gnpos.cpu().numpy().tolist() == npos.tolist() and int(gstatus.item()) == status
    # again, into buffers full of something else
    out = (torch.full((sum(g.numel() for g in got),), 7.0, device='cuda'), torch.full((len(first) - 1,), -3, dtype=torch.int32, device='cuda'),
           torch.zeros(1, dtype=torch.int32, device='cuda'))
    again, anpos, astatus = engine.assign_simota(dev, padded, first, ocfg, out=out)
    assert all(torch.equal(a, g) for a, g in zip(again, got)) and torch.equal(anpos, gnpos) and torch.equal(astatus, gstatus)
