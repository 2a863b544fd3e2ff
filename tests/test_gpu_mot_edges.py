"""yk_mot_eval's seven launches (csrc/yk_mot.hip) held to motmetrics.evaluate on the cases of tests/mot_cases.py - more than 64 and 128
frames, more than 128 rows a side, both orientations in one sequence, the CLEAR contest, exact thresholds, duplicates, strangers, sparse
ids - under tests/test_gpu_motmetrics.same_scores' contract; the scores' symmetries on the device's own results; a poisoned workspace
passed 8 bytes off its alignment; a large call before and after a small one; yk_lap_f64 on problem tables that motmetrics_gpu.lap never
builds; and a side stream.  tests/test_mot_cases.py proves on the CPU that every case reaches what it is here for."""
import ctypes as C
import functools

import numpy as np
import pytest

from k210_yolo_framework_amd import motmetrics as mm
from tests import mot_cases as mc
from tests.test_gpu_motmetrics import CASES as FIRST_CASES, device

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def on_device(name):
    """(the evaluator of a case, its result), computed once and shared"""
    ev = device(mc.case(name))
    return ev, ev.result()


@pytest.mark.parametrize('name', sorted(mc.BUILDERS))
def test_every_case_equals_the_rule(name):
    seqs, want = mc.case(name), mc.rule(name)
    ev, got = on_device(name)
    for n in want['sequences']:
        mc.same_scores(got['sequences'][n], want['sequences'][n])
    mc.same_scores(got['combined'], want['combined'])
    mc.same_bytes(ev.result(), got)                                       # two calls: the same bytes
    if len(seqs) > 1:                                                     # every sequence alone: what it scored in the batch
        for s in seqs:
            alone = device([s]).result()['sequences'][s[0]]
            mc.same_scores(alone, got['sequences'][s[0]])
            mc.same_scores(alone, want['sequences'][s[0]])


@pytest.mark.parametrize('name', mc.GENERIC)
def test_role_swap_on_the_device(name):
    _, got = on_device(name)
    swapped = device(mc.swap_roles(mc.case(name))).result()
    for g, s in zip(mc.each(got), mc.each(swapped)):
        mc.same_scores(mc.swapped_back(s), g, keys=mc.SWAP_KEYS)


@pytest.mark.parametrize('name', mc.GENERIC)
def test_relabel_and_reorder_on_the_device(name):
    _, got = on_device(name)
    moved = device(mc.relabel_and_reorder(mc.case(name))).result()
    for g, s in zip(mc.each(got), mc.each(moved)):
        mc.same_scores(s, g)


@pytest.mark.parametrize('name', ['long_65', 'mixed_orientation'])
def test_poisoned_workspace_off_its_alignment(name):
    """Every cell a kernel reads was written in the same call: the workspace and both outputs start as 0xFF bytes (NaN, -1), the workspace
    8 bytes past an aligned address so that the entry's 256-byte slack is what it stands on; and a second call into the same buffers,
    which now hold the first call's cells, gives the same bytes again."""
    import torch
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    ev, want = on_device(name)
    sh, tables = ev._pack()
    need = C.c_size_t(0)
    engine.call('yk_mot_workspace_bytes', C.byref(sh), C.byref(need))
    n = len(ev.seqs)
    poison = lambda nbytes: torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ev.device)
    with torch.cuda.device(ev.device):
        dev = [torch.from_numpy(np.ascontiguousarray(t) if t.size else np.zeros(1, t.dtype)).to(ev.device) for t in tables]
        ws = poison(need.value + 8)
        assert ws.data_ptr() % 256 == 0
        out_i, out_d = poison(n * mg.OUT_INTS * 4).view(torch.int32), poison(n * mg.OUT_DOUBLES * 8).view(torch.float64)
        assert int(out_i[0]) == -1 and bool(torch.isnan(out_d[0]))
        for _ in range(2):
            engine.call('yk_mot_eval', C.byref(sh), *dev, ws[8:], need.value, out_i, out_d, engine._stream())
            got = ev._scores(out_i.cpu().numpy().astype(np.int64).reshape(n, mg.OUT_INTS), out_d.cpu().numpy().reshape(n, mg.OUT_DOUBLES))
            mc.same_bytes(got, want)
    assert bytes(ws[:8].cpu().numpy()) == b'\xff' * 8                    # nothing below the address that was passed


def test_large_then_small_then_large():
    small = FIRST_CASES['one_object_three_frames']()
    for seqs, want in ((mc.case('wide_129_133'), mc.rule('wide_129_133')), (small, mm.evaluate(small)),
                       (mc.case('wide_129_133'), mc.rule('wide_129_133'))):
        got = device(seqs).result()
        for g, w in zip(mc.each(got), mc.each(want)):
            mc.same_scores(g, w)


# ---- yk_lap_f64 on tables laid out by hand ------------------------------------------------------------------------------------------------

SENTINEL = -77


def lap_call(cost, rows, n_out):
    """cost: the whole d_cost (float64 [n]); rows: (rows, cols, cost_offset, out_offset) per problem -> d_out after the call, int32 [n_out]
    that started as SENTINEL"""
    import torch
    from k210_yolo_framework_amd import engine, motmetrics_gpu as mg
    table = (mg.LapProblem * len(rows))(*[mg.LapProblem(*r) for r in rows])
    d_cost = torch.from_numpy(np.ascontiguousarray(cost, np.float64)).cuda()
    d_out = torch.full((n_out,), SENTINEL, dtype=torch.int32, device=d_cost.device)
    engine.call('yk_lap_f64', d_cost, cost.size, table, len(rows), d_out, n_out, engine._stream())
    return d_out.cpu().numpy().astype(np.int64)


def draw(rng, r, c, integer):
    return rng.integers(0, 1000, (r, c)).astype(np.float64) if integer else -rng.random((r, c))


def test_lap_table_in_reverse_order_with_gaps():
    rng = np.random.default_rng(8)
    mats = [draw(rng, *s, k % 2 == 0) for k, s in enumerate(((5, 7), (64, 3), (1, 1), (65, 66), (9, 130), (3, 3)))]
    cost, rows, at_c, at_o = [], [None] * len(mats), 0, 0
    for k in reversed(range(len(mats))):                                  # the last problem first, 3 doubles and 2 ints between neighbours
        cost += [np.full(3, np.nan), mats[k].ravel()]
        rows[k] = (*mats[k].shape, at_c + 3, at_o + 2)
        at_c, at_o = at_c + 3 + mats[k].size, at_o + 2 + mats[k].shape[0]
    out = lap_call(np.concatenate(cost + [np.full(3, np.nan)]), rows, at_o + 2)
    written = np.zeros(at_o + 2, bool)
    for m, (r, _, _, o) in zip(mats, rows):
        assert np.array_equal(out[o:o + r], mm.lap(m)), m.shape
        written[o:o + r] = True
    assert (~written).sum() == 2 * (len(mats) + 1) and (out[~written] == SENTINEL).all()


def test_lap_problems_that_share_a_cost_span():
    rng = np.random.default_rng(9)
    span = draw(rng, 1, 36, True).ravel()                                 # 36 doubles read as 6 x 6 (twice), 4 x 9 and 9 x 4
    shapes = ((6, 6), (4, 9), (9, 4), (6, 6))
    rows, at = [], 0
    for r, c in shapes:
        rows.append((r, c, 0, at))
        at += r
    out = lap_call(span, rows, at)
    for r, c, _, o in rows:
        assert np.array_equal(out[o:o + r], mm.lap(span.reshape(r, c))), (r, c)
    assert np.array_equal(out[0:6], out[19:25])


def test_lap_wide_and_tall_shapes_outside_lds():
    """Neither square nor resident: 3 to 5 lane strides against 100 rows, 64 strides (YK_LAP_MAX_LONG) against 7, and 200 x 260."""
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    assert mg.limits()['MAX_LONG'] == 4096
    rng = np.random.default_rng(10)
    shapes = ((100, 300), (300, 100), (7, 4096), (4096, 7), (200, 260))
    mats = [draw(rng, r, c, k in (0, 3)) for k, (r, c) in enumerate(shapes)]
    assert not any(mg.lds_resident(*s) for s in shapes)
    for m, g in zip(mats, mg.lap(mats)):
        assert np.array_equal(g, mm.lap(m)), m.shape


def test_lap_one_problem_then_two_thousand_then_one():
    """The device copy of the table grows between the calls, and 2000 workgroups are far more than the device has compute units."""
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    rng = np.random.default_rng(11)
    one, other = draw(rng, 6, 8, True), draw(rng, 8, 6, False)
    many = [draw(rng, 5, 5, k % 2 == 0) for k in range(2000)]
    first, got, last = mg.lap([one]), mg.lap(many), mg.lap([other])
    assert np.array_equal(first[0], mm.lap(one)) and np.array_equal(last[0], mm.lap(other))
    assert len(got) == 2000
    for k, (m, g) in enumerate(zip(many, got)):
        assert np.array_equal(g, mm.lap(m)), k


def test_side_stream_gives_the_same_bytes():
    import torch
    from k210_yolo_framework_amd import motmetrics_gpu as mg
    rng = np.random.default_rng(12)
    costs = [draw(rng, *s, k % 2 == 0) for k, s in enumerate(((5, 5), (64, 129), (150, 150), (70, 3)))]
    side = torch.cuda.Stream()                                            # (default priority)
    here, there = mg.lap(costs), mg.lap(costs, stream=side)
    for c, a, b in zip(costs, here, there):
        assert np.array_equal(a, mm.lap(c)) and a.tobytes() == b.tobytes(), c.shape
    ev, got = on_device('mixed_orientation')
    mc.same_bytes(ev.result(stream=side), got)
    mc.same_bytes(ev.result(), got)
