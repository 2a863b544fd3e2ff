"""Adaptive rounding (adaround.py) and quantize(weight_codes=): the rule on the CPU, with numpy-built Gram matrices.  No device needed."""
import numpy as np
import pytest

from k210_yolo_framework_amd import adaround, biascorrect, kmodel, netspec as ns, quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from tests import adaround_cases as ac
from tests import biascorrect_cases as bc

BRUTE_ITERS = 1000
SLACK = 1e-12                                              # relative: the float64 rounding of one quadratic form evaluated in two places


@pytest.fixture(scope='module')
def mini():
    spec, w, fr, fm, ranges = bc.mini_case()
    km, rep = quantize.quantize(spec, w, ranges)
    return spec, w, ranges, km, rep


def test_v_init_gives_h_equal_r():
    r = np.concatenate([np.linspace(0.0, 1.0, 1001)[:-1], [1e-12, 0.5, 1.0 - 1e-12]])
    assert np.abs(adaround.h_of(adaround.v_init(r)) - r).max() <= 4 * np.finfo(np.float64).eps


def test_rows_of_and_kern_of_are_inverse_and_in_im2col_order():
    rng = np.random.default_rng(0)
    k = rng.normal(size=(3, 3, 5, 7))
    rows = adaround.rows_of(k, False)
    assert rows.shape == (7, 45) and rows[2, (1 * 3 + 2) * 5 + 4] == k[1, 2, 4, 2]
    assert np.array_equal(adaround.kern_of(rows, k.shape, False), k)
    d = rng.normal(size=(3, 3, 6, 1))
    rows = adaround.rows_of(d, True)
    assert rows.shape == (6, 9) and rows[4, 2 * 3 + 1] == d[2, 1, 4, 0]
    assert np.array_equal(adaround.kern_of(rows, d.shape, True), d)


def test_schedule_warm_up_then_beta_from_20_to_2():
    s = [adaround.schedule(t, 50, 0.01) for t in range(50)]
    assert all(l == 0.0 for l, b in s[:10]) and all(l == 0.01 for l, b in s[10:])
    assert s[10][1] == 20.0 and s[-1][1] == 2.0
    assert all(a[1] > b[1] for a, b in zip(s[10:], s[11:]))


def test_frozen_elements_never_move_and_the_clipped_ones_have_no_gradient():
    case = ac.step_case(3, 86)
    states, _ = ac.run_steps(case, 0.01, 11.37, 3, np.float64)
    fz = case['frozen']
    for V, m, v, D in states:
        assert np.array_equal(V[fz], case['V'][fz]) and not m[fz].any() and not v[fz].any() and not D[fz].any()
        hr = adaround.sigmoid(case['V']) * (adaround.ZETA - adaround.GAMMA) + adaround.GAMMA
        clipped = (hr <= 0.0) | (hr >= 1.0)                                    # V = +-20 among them: h is clipped, the gradient is 0
        assert clipped[np.abs(case['V']) == 20.0].all() and (np.abs(case['V']) == 20.0).any() and np.array_equal(V[clipped], case['V'][clipped])
        assert np.isfinite(V).all() and np.isfinite(D).all()
    assert (states[-1][0][~fz & ~clipped] != case['V'][~fz & ~clipped]).all()


def test_the_regulariser_gives_no_nan_at_h_0_half_and_1():
    V = np.array([[adaround.v_init(np.array(0.5)), 30.0, -30.0, 0.3]])
    z = np.zeros_like(V)
    for beta in (20.0, 11.37, 2.0):
        Vc, m, v = V.copy(), z.copy(), z.copy()
        D = adaround.step(Vc, m, v, np.full_like(V, 0.25), np.zeros(V.shape, bool), np.ones_like(V), np.ones(1), 4, 0.1, 0.01, beta, 1e-2, 1)
        assert np.isfinite(Vc).all() and np.isfinite(D).all() and np.isfinite(m).all()


def test_hardening_an_untouched_v_gives_quantizes_codes(mini):
    spec, w, ranges, km, rep = mini
    _, _, _, G = ac.mini_case()
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        name, dw = op['layer'], op['type'] == ns.OP_DWCONV
        kern = np.asarray(w[name + '/kernel'], np.float64)
        rows = adaround.rows_of(kern, dw)
        codes, info = adaround.optimise_numpy(rows, G[name], iters=0)
        st = adaround.setup(rows)
        up = np.where(st['frozen'], st['nearest'], np.clip(st['down'] + (adaround.h_of(adaround.v_init(st['r'])) >= 0.5), 0, 255))
        assert (st['r'] != 0.5).all() and np.array_equal(up, st['nearest'])                  # h(V_init) = r: up iff r >= 0.5, which is rint
        assert info['flipped'] == 0 and info['rows_changed'] == 0
        layer = km.layers[rep['layers'][name]['index']]
        want = layer.weights.reshape(codes.shape[0], -1, 9 if op['k'] == 3 else 1)           # the kmodel's [Co][Ci][kk]
        got = adaround.kern_of(codes, kern.shape, dw)
        got = got[..., 0].transpose(2, 0, 1).reshape(want.shape) if dw else got.transpose(3, 2, 0, 1).reshape(want.shape)
        assert np.array_equal(got, want), name


@pytest.mark.parametrize('seed', ac.BRUTE_SEEDS)
def test_brute_force_rows_end_between_the_optimum_and_nearest(seed):
    rows, G = ac.brute_row(seed)
    assert np.linalg.eigvalsh(G).min() > 0.0
    best, near, n_free = ac.brute_force(rows, G)
    assert 6 <= n_free <= 10
    codes, info = adaround.optimise_numpy(rows, G, BRUTE_ITERS)
    e = float(adaround.row_errors(adaround.hard_error(codes, adaround.setup(rows)), G)[0])
    print(f'seed {seed}: {n_free} free, optimum {best:.6g} <= {e:.6g} <= nearest {near:.6g}, {info["flipped"]} flipped')
    assert best * (1 - SLACK) <= e <= near * (1 + SLACK)
    assert e == info['e_adaround']


def test_brute_force_at_least_one_row_is_strictly_below_nearest():
    below = []
    for seed in ac.BRUTE_SEEDS:
        rows, G = ac.brute_row(seed)
        _, info = adaround.optimise_numpy(rows, G, BRUTE_ITERS)
        below.append(info['e_adaround'] < info['e_nearest'])
    assert any(below), below


def test_mini_network_a_dense_and_a_depthwise_row_improve_strictly_and_none_gets_worse():
    spec, w, fr, G = ac.mini_case()
    res = ac.mini_optimised()
    kinds = {op['layer']: op['type'] for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)}
    improved = {ns.OP_CONV: 0, ns.OP_DWCONV: 0}
    for name, (codes, info) in res.items():
        dw = kinds[name] == ns.OP_DWCONV
        rows = adaround.rows_of(np.asarray(w[name + '/kernel'], np.float64), dw)
        st = adaround.setup(rows)
        lo, hi = adaround.allowed_codes(rows)
        assert ((codes == lo) | (codes == hi)).all() and np.array_equal(codes[st['frozen']], st['nearest'][st['frozen']]), name
        e_new = adaround.row_errors(adaround.hard_error(codes, st), G[name])
        e_near = adaround.row_errors(adaround.hard_error(st['nearest'], st), G[name])
        assert (e_new <= e_near).all(), name
        improved[kinds[name]] += int((e_new < e_near).sum())
        print(f"{name}: {info['rows_changed']}/{info['rows']} rows, {info['flipped']} flipped, ratio {info['ratio']:.4f}")
    assert improved[ns.OP_CONV] >= 1 and improved[ns.OP_DWCONV] >= 1, improved
    text = adaround.format_report(dict(layers={n: i for n, (c, i) in res.items()}, iters=ac.MINI_ITERS, lam=ac.MINI_LAMBDA, lr=ac.MINI_LR,
                                       max_gram_mb=1024))
    assert text.count('adaround ') == len(res) and 'adaptive rounding:' in text


# ---- quantize(weight_codes=) ---------------------------------------------------------------------------------------------------------------
def _nearest(w, name):
    return adaround.setup(np.asarray(w[name + '/kernel'], np.float64))['nearest']


def test_nearest_codes_none_and_empty_serialise_to_the_same_bytes(mini):
    spec, w, ranges, km, rep = mini
    want = kmodel.serialise(km)
    for codes in (None, {}, {l.name: _nearest(w, l.name) for l in spec.layers}):
        km2, rep2 = quantize.quantize(spec, w, ranges, weight_codes=codes)
        assert kmodel.serialise(km2) == want
        assert rep2['layers'] == rep['layers']


@pytest.mark.parametrize('name', ['conv_pw_2', 'conv_dw_3', 'conv1'])
def test_one_flipped_code_changes_exactly_that_weight_byte(mini, name):
    spec, w, ranges, km, rep = mini
    kern = np.asarray(w[name + '/kernel'], np.float64)
    st = adaround.setup(kern)
    at = tuple(int(v) for v in np.argwhere(~st['frozen'])[5])
    codes = st['nearest'].copy()
    lo, hi = adaround.allowed_codes(kern)
    codes[at] = hi[at] if codes[at] == lo[at] else lo[at]
    km2, rep2 = quantize.quantize(spec, w, ranges, weight_codes={name: codes})
    a, b = np.frombuffer(kmodel.serialise(km), np.uint8), np.frombuffer(kmodel.serialise(km2), np.uint8)
    assert len(a) == len(b) and (a != b).sum() == 1
    i = int(np.flatnonzero(a != b)[0])
    assert {int(a[i]), int(b[i])} == {int(lo[at]), int(hi[at])}
    idx = rep['layers'][name]['index']
    wa, wb = km.layers[idx].weights, km2.layers[idx].weights
    assert (wa != wb).sum() == 1
    assert rep2['layers'][name]['zero_share'] == float((wb == rep['layers'][name]['zp_w']).mean())


def test_a_code_two_steps_away_an_unknown_layer_and_a_wrong_shape_raise(mini):
    spec, w, ranges, km, rep = mini
    name = 'conv_pw_1'
    kern = np.asarray(w[name + '/kernel'], np.float64)
    lo, hi = adaround.allowed_codes(kern)
    at = tuple(int(v) for v in np.argwhere((lo >= 2) & (hi <= 253))[0])
    for off in (hi[at] + 1, lo[at] - 1):
        codes = _nearest(w, name)
        codes[at] = off
        with pytest.raises(KmodelError, match=name):
            quantize.quantize(spec, w, ranges, weight_codes={name: codes})
    with pytest.raises(KmodelError, match='no_such_layer'):
        quantize.quantize(spec, w, ranges, weight_codes={'no_such_layer': _nearest(w, name)})
    with pytest.raises(KmodelError, match=name):
        quantize.quantize(spec, w, ranges, weight_codes={name: _nearest(w, name)[..., :-1]})
    with pytest.raises(KmodelError, match=name):
        quantize.quantize(spec, w, ranges, weight_codes={name: _nearest(w, name).astype(np.int32)})


def test_biascorrect_passes_the_codes_to_every_quantize_call(mini, monkeypatch):
    spec, w, ranges, km, rep = mini
    _, _, fr, fm, _ = bc.mini_case()
    codes = {n: adaround.kern_of(c, np.shape(w[n + '/kernel']), n.startswith('conv_dw')) for n, (c, i) in ac.mini_optimised().items()}
    seen = []
    real = quantize.quantize

    def spy(*a, **k):
        seen.append(a[4] if len(a) > 4 else k.get('weight_codes'))
        return real(*a, **k)
    monkeypatch.setattr(quantize, 'quantize', spy)
    delta, brep = biascorrect.correct(spec, w, ranges, fm, bc.numpy_measure(fr), codes)
    assert len(seen) == len(rep['layers']) and all(s is codes for s in seen)
    km2, _ = real(spec, w, ranges, delta, codes)
    idx = rep['layers']['conv_pw_4']['index']
    assert (km2.layers[idx].weights != km.layers[idx].weights).any()


def test_cli_refuses_adaround_with_ranges(tmp_path, capsys):
    from k210_yolo_framework_amd import make_kmodel
    with pytest.raises(SystemExit):
        make_kmodel.cli(['ckpt.h5', str(tmp_path / 'o.kmodel'), '--adaround', 'True', '--ranges', 'x.npz'])
    assert 'needs calibration frames' in capsys.readouterr().err
    assert not (tmp_path / 'o.kmodel').exists()
