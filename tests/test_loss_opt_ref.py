"""k210_yolo_framework_amd/lossopt.py (the closed form) against tests/loss_opt_ref.py (float64 autograd) on the inputs tests/test_gpu_loss_opt.py
holds the kernel to; the statement with every option off against tests/box_loss_ref.py; and the way of the five options through the Python
layer, the command line, the Makefile and the header.  CPU only."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import lossopt
from tests import box_loss_ref as B
from tests import loss_opt_ref as R

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_closed_form_equals_float64_autograd(name):
    """obj, noobj, cls and gradient entries 4.. of lossopt.closed_form against autograd at rtol 1e-9, for every option set; entries 0..3 and
    the box terms of the statement are those of the statement without options (the IoU target is a constant)."""
    anc, y_true, y_pred, kw = R.parity_case(name)
    for box in R.BOX_MODES:
        plain_l, plain_g, plain_i = B.autograd(y_true, y_pred, anc, box_loss=box, **kw)
        for oname in R.OPTION_SETS:
            o = R.options(oname)
            terms, grad, ign, zo = R.autograd(y_true, y_pred, anc, box_loss=box, **kw, **o)
            got, gg, gz = lossopt.closed_form(y_true, y_pred, anc, ow=kw['ow'], nw=kw['nw'], batch_size=kw['batch_size'], **o)
            for k in ('obj', 'noobj', 'cls'):
                assert abs(got[k] - terms[k]) <= 1e-9 * abs(terms[k]), (oname, box, k, got[k], terms[k])
            # atol: p - z cancels at a saturated logit, so either side carries an absolute error of an ulp of 1 (2.2e-16) times factors <= 1
            np.testing.assert_allclose(gg, grad[..., 4:], rtol=1e-9, atol=1e-15, err_msg=f'{oname} {box}')
            np.testing.assert_allclose(gz, zo, rtol=1e-12, atol=0)
            assert np.array_equal(grad[..., 0:4], plain_g[..., 0:4]) and np.array_equal(ign, plain_i)
            assert all(terms[k] == plain_l[k] for k in ('xy', 'wh', 'box'))
            assert np.isfinite(grad).all() and 0 <= zo.min() and zo.max() <= 1


@pytest.mark.parametrize('name', R.ALL_PARITY)
def test_with_every_option_off_the_statement_is_box_loss_ref(name):
    anc, y_true, y_pred, kw = R.parity_case(name)
    for box in R.BOX_MODES:
        want_l, want_g, want_i = B.autograd(y_true, y_pred, anc, box_loss=box, **kw)
        for off in (R.OFF, dict(R.OFF, focal='all', focal_gamma=0.0), dict(R.OFF, focal_gamma=1.5, focal_alpha=0.25)):
            got_l, got_g, got_i, zo = R.autograd(y_true, y_pred, anc, box_loss=box, **kw, **off)
            assert got_l == want_l and np.array_equal(got_g, want_g) and np.array_equal(got_i, want_i), off
            assert np.array_equal(zo, y_true[..., 4].astype(np.float64))


def test_float32_build_of_the_reference_meets_the_recorded_atol():
    """What the GPU test's absolute gradient tolerance rests on: the statement in torch float32 against float64 at rtol 2e-5, on the
    gradient entries the options touch (4..)."""
    worst = 0.0
    for name in R.ALL_PARITY:
        anc, y_true, y_pred, kw = R.parity_case(name)
        for box in R.BOX_MODES:
            for oname in R.OPTION_SETS:
                o = R.options(oname)
                _, g64, i64, _ = R.autograd(y_true, y_pred, anc, box_loss=box, **kw, **o)
                _, g32, i32, _ = R.autograd(y_true, y_pred, anc, box_loss=box, dtype=torch.float32, **kw, **o)
                assert np.array_equal(i64, i32)
                a = R.atol_needed(g32[..., 4:], g64[..., 4:])
                if a > worst:
                    print(name, box, oname, 'float32 build needs atol', a)
                worst = max(worst, a)
    print('largest', worst, 'recorded', R.F32_ATOL_MEASURED)
    assert worst <= R.F32_ATOL_MEASURED


# ------------------------------------------------------------------------------ what tests/test_gpu_loss_instances.py rests on (reference alone)
GPU_RTOL, GPU_ATOL = 2e-5, R.ATOL_FACTOR * R.F32_ATOL_MEASURED
SWEEPS = ((R.INSTANCE_CASES, R.INSTANCE_SETS), (R.EDGE_CASES, R.EDGE_SETS))


def test_instance_sets_are_the_27_cases_of_the_dispatch():
    """(a) INSTANCE_SETS maps one-to-one onto the OPT values loss_launch_opt's switch has a case for, written out here from the enum and read
    again from the macro list in the source; every EDGE_SETS entry runs one of them."""
    F, K, P, S, I = R.L_FOBJ, R.L_FCLS, R.L_POW, R.L_SMOOTH, R.L_IOU
    l4 = lambda o: {o, o | S, o | I, o | S | I}
    want = {S, I, S | I} | l4(F) | l4(K) | l4(F | K) | l4(F | P) | l4(K | P) | l4(F | K | P)
    bits = [R.instance_bits(**o) for o in R.INSTANCE_SETS.values()]
    assert len(bits) == 27 and len(set(bits)) == 27 and set(bits) == want
    assert all(R.instance_bits(**dict(R.OFF, **o)) in want for o in R.EDGE_SETS.values())
    assert R.instance_bits(**R.OFF) == 0 and R.instance_bits(**dict(R.OFF, focal='all', focal_gamma=0.0)) == 0
    src = (ROOT / 'k210_yolo_framework_amd' / 'csrc' / 'yk_loss.hip').read_text()
    assert 'enum { L_FOBJ = 1, L_FCLS = 2, L_POW = 4, L_SMOOTH = 8, L_IOU = 16 };' in src
    assert '#define YK_L4(o) YK_L1(o) YK_L1((o) | L_SMOOTH) YK_L1((o) | L_IOU) YK_L1((o) | L_SMOOTH | L_IOU)' in src
    body = src[src.index('switch (bits) {'):]
    cases = []
    for macro, arg in re.findall(r'YK_L([14])\(([A-Z_| ]+)\)', body[:body.index('}')]):
        o = 0
        for name in arg.split('|'):
            o |= getattr(R, name.strip())
        cases += [o] if macro == '1' else sorted(l4(o))
    assert sorted(cases) == sorted(want)                                 # each once


def test_float32_build_of_the_reference_meets_the_recorded_atol_on_both_instance_sweeps():
    """(b) A condition on the inputs of the two sweeps, not a new tolerance: the statement in torch float32 against float64 stays within the
    figures of the existing GPU test on every (case, box mode, set) - gradient entries 4.. at rtol 2e-5 need no more than F32_ATOL_MEASURED,
    every loss term is within 2e-5 of max(1, |ref|), the ignore masks are equal.  Measured: atol 2.6e-11 at most on the 27 x 4 sweep, 1.7e-10
    on the edge sets (head_7x10, label_smooth 0.999); the worst loss term 1.7e-6 relative (xy on p257)."""
    for sweep, (cases, sets) in zip(('instances', 'edges'), SWEEPS):
        worst_a, worst_t = 0.0, (0.0, None)
        for case in cases:
            for box in R.ALL_BOX_MODES:
                for oname in sets:
                    l64, g64, i64, _ = R.sweep_ref(case, box, oname)
                    l32, g32, i32, _ = R.sweep_ref(case, box, oname, torch.float32)
                    assert np.array_equal(i64, i32), (case, box, oname)
                    assert np.isfinite(g64).all() and np.isfinite(g32).all()
                    worst_a = max(worst_a, R.atol_needed(g32[..., 4:], g64[..., 4:], GPU_RTOL))
                    for term in R.TERMS:
                        e = abs(l32[term] - l64[term]) / max(1.0, abs(l64[term]))
                        assert e <= 2e-5, (case, box, oname, term, e)
                        worst_t = max(worst_t, (e, f'{term} {case} {box} {oname}'))
        print(sweep, 'float32 build needs atol', worst_a, 'recorded', R.F32_ATOL_MEASURED, 'worst loss term', worst_t)
        assert worst_a <= R.F32_ATOL_MEASURED


def _shows(bit, common):
    """Where a flipped OPT bit shows in the statement: (loss terms, slice of the gradient's last axis).  L_FOBJ and L_IOU: obj (L_FOBJ also
    noobj) and entry 4; L_FCLS and L_SMOOTH: cls and entries 5..; L_POW: those of the focal bits beside it."""
    obj, cls = (('obj', 'noobj'), slice(4, 5)), (('cls',), slice(5, None))
    if bit == R.L_POW:
        return [w for f, w in ((R.L_FOBJ, obj), (R.L_FCLS, cls)) if common & f]
    return [obj if bit in (R.L_FOBJ, R.L_IOU) else cls]


def _shown(a, b, where):
    """The largest difference of two references over `where`, in units of what the GPU test allows there."""
    (la, ga, _, _), (lb, gb, _, _) = a, b
    worst = 0.0
    for terms, sl in where:
        for t in terms:
            worst = max(worst, abs(la[t] - lb[t]) / (2e-5 * max(1.0, abs(la[t]), abs(lb[t]))))
        worst = max(worst, float((np.abs(ga[..., sl] - gb[..., sl]) / (GPU_RTOL * np.maximum(np.abs(ga[..., sl]), np.abs(gb[..., sl])) + GPU_ATOL)).max()))
    return worst


@pytest.mark.parametrize('case', R.INSTANCE_CASES)
def test_two_instances_one_bit_apart_differ_by_100_times_the_gpu_tolerance(case):
    """(c) A wrong instance cannot pass: for every box mode and every two INSTANCE_SETS entries whose OPT differ in one bit, the float64
    references differ, in a loss term or gradient entry of `_shows`, by at least 100 times what the GPU test allows there (2e-5 max(1, |ref|)
    for a term, rtol |ref| + atol for an entry).  Every bit is observable on every case: each has object cells with classes.  On `geometry`
    L_IOU alone shows at the disjoint cell, whose target falls from 1 to exactly 0."""
    names = list(R.INSTANCE_SETS)
    bits = {n: R.instance_bits(**R.INSTANCE_SETS[n]) for n in names}
    disjoint = B.geometry_case()[3][0]
    pairs, least = 0, {}
    for box in R.ALL_BOX_MODES:
        for i, u in enumerate(names):
            for v in names[i + 1:]:
                flip = bits[u] ^ bits[v]
                if flip not in R.BIT_NAMES:
                    continue
                a, b = R.sweep_ref(case, box, u), R.sweep_ref(case, box, v)
                d = _shown(a, b, _shows(flip, bits[u] & bits[v]))
                assert d >= 100, (box, u, v, R.BIT_NAMES[flip], d)
                least[R.BIT_NAMES[flip]] = min(least.get(R.BIT_NAMES[flip], np.inf), d)
                if case == 'geometry' and flip == R.L_IOU:
                    ga, gb = a[1][disjoint][4], b[1][disjoint][4]
                    assert abs(ga - gb) >= 100 * (GPU_RTOL * max(abs(ga), abs(gb)) + GPU_ATOL), (box, u, v, ga, gb)
                pairs += 1
    print(case, pairs, 'pairs; least difference / allowance per bit:', least)
    assert pairs == 4 * 60 and set(least) == set(R.BIT_NAMES.values())


def test_iou_target_on_the_forced_geometries():
    """(d) obj_target='iou' on `geometry`: the returned target is exactly 0.0 at the disjoint cell, strictly inside (0, 1) at the cells with
    the prediction inside the label box, around it and across it, and the same array in all four box modes."""
    cells = B.geometry_case()[3]
    zo = [R.sweep_ref('geometry', box, 'iou')[3] for box in R.ALL_BOX_MODES]
    assert zo[0][cells[0]] == 0.0
    assert all(0.0 < zo[0][c] < 1.0 for c in cells[1:])
    assert all(np.array_equal(z, zo[0]) for z in zo[1:])


def test_corner_case_is_disjoint_in_both_axes_with_a_product_below_the_areas():
    """What the GPU test of `corner_case` rests on: the target is exactly 0, an IoU of the unclamped overlaps would be about 0.02, and the
    float32 build of the statement stays within the recorded figures on it."""
    anc, y_true, y_pred, kw, cell = R.corner_case()
    b, t = B.decode(y_pred, anc)[0][cell], y_true[cell][0:4].astype(np.float64)
    assert B.geometry_of(b, t) == 'disjoint'
    raw = np.minimum(b[0:2] + b[2:4] / 2, t[0:2] + t[2:4] / 2) - np.maximum(b[0:2] - b[2:4] / 2, t[0:2] - t[2:4] / 2)
    assert (raw < 0).all() and 0.015 < raw.prod() / (b[2] * b[3] + t[2] * t[3] - raw.prod()) < 0.025
    for box in R.ALL_BOX_MODES:
        l64, g64, i64, zo = R.autograd(y_true, y_pred, anc, box_loss=box, **kw, obj_target='iou')
        l32, g32, i32, _ = R.autograd(y_true, y_pred, anc, box_loss=box, dtype=torch.float32, **kw, obj_target='iou')
        assert zo[cell] == 0.0 and np.array_equal(i64, i32)
        assert R.atol_needed(g32[..., 4:], g64[..., 4:], GPU_RTOL) <= R.F32_ATOL_MEASURED
        assert all(abs(l32[k] - l64[k]) <= 2e-5 * max(1.0, abs(l64[k])) for k in R.TERMS)


def test_the_inputs_are_what_they_say():
    anc, y_true, y_pred, _ = R.parity_case('saturated')
    ob = y_true[..., 4] > 0.7
    for m in (ob, ~ob):
        assert (y_pred[m][:, 4:] == 80).all(1).any() and (y_pred[m][:, 4:] == -80).all(1).any()
    anc, y_true, y_pred, _ = R.parity_case('full_20x20')
    assert (y_true[..., 4] == 1).all() and y_true[..., 4].size == 1200
    assert R.parity_case('c80')[1].shape[-1] == 85
    assert [int(np.prod(R.parity_case(n)[1].shape[1:4])) for n in ('p255', 'p256', 'p257')] == [255, 256, 257]
    assert R.parity_case('one_cell')[1].shape == (1, 1, 1, 1, 6) and R.parity_case('head_7x10')[1].shape[1:] == (7, 10, 3, 25)


def test_focal_term_limits():
    x = np.array([-80.0, -3.0, 0.0, 2.5, 80.0])
    for z in (0.0, 0.3, 1.0):
        v, d = lossopt.focal_term(z, x, 0.0, 0.0)                        # gamma = 0, alpha = 0: bce
        assert np.array_equal(v, lossopt.bce(z, x)) and np.array_equal(d, lossopt.sigmoid(x) - z)
        v, d = lossopt.focal_term(z, x, 2.0, 0.25)
        assert np.isfinite(v).all() and np.isfinite(d).all() and (v >= 0).all()
    v, _ = lossopt.focal_term(1.0, np.array([80.0]), 1.0, 0.0)           # the saturated side keeps its bits: (1 - p_t) = sigmoid(-80), not 0
    assert 0 < v[0] < 1e-60
    assert lossopt.smooth(np.array([0.0, 1.0]), 0.1) == pytest.approx([0.05, 0.95], rel=1e-15)


BAD = [dict(focal_gamma=0.5), dict(focal_gamma=5.5), dict(focal_gamma=-1.0), dict(focal_gamma=float('nan')), dict(focal_alpha=1.0),
       dict(focal_alpha=-0.1), dict(label_smooth=1.0), dict(label_smooth=-0.1), dict(focal='both'), dict(obj_target='giou')]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '-'.join(f'{k}={v}' for k, v in b.items()))
def test_options_out_of_range_are_refused_by_every_python_layer(bad):
    from k210_yolo_framework_amd import engine, helper
    field = next(iter(bad))
    t = torch.zeros(1, 1, 1, 1, 6)
    for call in (lambda: lossopt.validate(**bad),
                 lambda: lossopt.closed_form(t.numpy(), t.numpy(), [[1, 1]], **bad),
                 lambda: engine.yolo_loss(t, t, [[1, 1]], 0.7, 0.5, 1, 1, 1, **bad),
                 lambda: helper.create_loss_fn(None, 0.7, 0.5, 1, 1, 1, 0, **bad)):
        with pytest.raises(ValueError, match=field):
            call()
    for ok in (dict(focal_gamma=0.0), dict(focal_gamma=1.0), dict(focal_gamma=5.0), dict(focal_alpha=0.999), dict(label_smooth=0.0)):
        lossopt.validate(**ok)


def test_trainer_refuses_them_before_it_touches_the_gpu():
    from k210_yolo_framework_amd.train import Trainer
    with pytest.raises(ValueError, match='focal_gamma'):
        Trainer(None, {}, np.ones((1, 3, 2), np.float32), 1, focal='all', focal_gamma=0.5)


def test_parser_takes_the_five_flags(capsys):
    from k210_yolo_framework_amd import training
    a = training.parser().parse_args([])
    assert (a.focal, a.focal_gamma, a.focal_alpha, a.label_smooth, a.obj_target) == ('off', 2.0, 0.0, 0.0, 'label')
    a = training.parser().parse_args(['--focal', 'cls', '--focal_gamma', '1.5', '--focal_alpha', '0.25', '--label_smooth', '0.1', '--obj_target', 'iou'])
    assert (a.focal, a.focal_gamma, a.focal_alpha, a.label_smooth, a.obj_target) == ('cls', 1.5, 0.25, 0.1, 'iou')
    with pytest.raises(SystemExit):
        training.parser().parse_args(['--focal', 'both'])
    assert "invalid choice: 'both'" in capsys.readouterr().err
    assert lossopt.describe(**lossopt.validate('all', 2.0, 0.25, 0.1, 'iou')) == \
        'focal all (gamma 2, alpha 0.25), label smoothing 0.1, objectness target iou'
    assert lossopt.describe(**lossopt.DEFAULTS) == '' and lossopt.is_off(**lossopt.DEFAULTS)


def _make_n(*args):
    return subprocess.run(['make', '-n', 'train', *args], cwd=ROOT, capture_output=True, text=True, check=True).stdout


def test_make_train_carries_the_five_flags_and_the_default_line_has_none():
    line = _make_n('FOCAL=all', 'FOCALGAMMA=1.5', 'FOCALALPHA=0.25', 'LABELSMOOTH=0.1', 'OBJTARGET=iou')
    assert '--focal all --focal_gamma 1.5 --focal_alpha 0.25 --label_smooth 0.1 --obj_target iou' in line
    assert '--focal off --focal_gamma 2.0 --focal_alpha 0 --label_smooth 0 --obj_target iou' in _make_n('OBJTARGET=iou')
    assert '--focal off' in _make_n('LABELSMOOTH=0.1') and '--label_smooth 0.1' in _make_n('LABELSMOOTH=0.1')
    plain = _make_n()
    for flag in ('--focal', '--label_smooth', '--obj_target'):
        assert flag not in plain


def test_header_declares_the_call_and_the_structure_follows_it():
    from k210_yolo_framework_amd import abi, engine
    sigs = abi.signatures(engine.HEADER_PATH.read_text())
    assert sigs['yk_yolo_loss_opt'] == sigs['yk_yolo_loss'] == sigs['yk_yolo_loss_ex']
    names = [n for n, _ in engine.LossCfgOpt._fields_]
    assert names == [n for n, _ in engine.LossCfgEx._fields_] + ['focal', 'focal_gamma', 'focal_alpha', 'label_smooth', 'obj_target']
    assert C.sizeof(engine.LossCfgOpt) == C.sizeof(engine.LossCfgEx) + 20 and engine.LossCfgOpt.focal.offset == C.sizeof(engine.LossCfgEx)
    header = engine.HEADER_PATH.read_text()
    start = header.index('} yk_loss_cfg_ex_t;')
    body = header[start:header.index('} yk_loss_cfg_opt_t;')]
    assert [body.index(n) for n in ('int32_t focal;', 'focal_gamma, focal_alpha, label_smooth;', 'int32_t obj_target;')] == \
        sorted(body.index(n) for n in ('int32_t focal;', 'focal_gamma, focal_alpha, label_smooth;', 'int32_t obj_target;'))
    assert lossopt.FOCAL == {'off': 0, 'obj': 1, 'cls': 2, 'all': 3} and lossopt.OBJ_TARGETS == {'label': 0, 'iou': 1}
    assert 'YK_FOCAL_OBJ = 1, YK_FOCAL_CLS = 2' in header and 'YK_OBJ_TARGET_LABEL = 0, YK_OBJ_TARGET_IOU = 1' in header
