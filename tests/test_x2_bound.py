"""The test of the test: oracle/x2_bound.py (the float64 per-launch reference and its propagated error bound, which
tests/test_gpu_layers_x2.py holds every f16x2 launch to) against a numpy model of the kernels' arithmetic.

  * the correct three-product model is ACCEPTED on one layer of each kind with error / E <= 1/4 (the margin C_DOT was given);
  * each defect the bound exists to catch is REJECTED (error / E > 1), one at a time;
  * C_DOT is what the model says it is, and separates from a dropped cross product by a factor 8 at every K;
  * the propagated part of the bound dominates in float64; the sub-chain runner equals oracle/torch_net_ref.forward on whole networks.

What the bound cannot see (measured here, not asserted): one k-step of 32 dropped out of K = 9216 moves an element by about 0.4 x 2^-22 T,
below C_DOT; the single-k-step mutant below runs on the K = 384 layer (12 steps), the deepest the fused-block kernels have."""
import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from oracle import torch_net_ref, x2_bound as xb

B = 2


def _layer(kind, H, W, C, N, k=1, stride=1, act=ns.LEAKY03, seed=3):
    s = ns.NetSpec('one_layer', (H, W))
    x = s._new_tensor(H, W, C)
    pad = ns.K210_S2_PAD if stride == 2 else ((k - 1) // 2,) * 4
    if kind == 'conv':
        s.conv(x, N, k, stride, pad, act=act, name='l')
    else:
        s.dwconv(x, stride, pad, act=act, name='l')
    return s, s.init_weights(seed=seed)


def _run(spec, w, mutate=None, seed=11, out='split'):
    """-> (error / E, worst index, exponents of the input) of the model's launch against the float64 reference from the model's own input."""
    op = spec.ops[0]
    H, W, C = spec.tensors[0]
    ho, wo, _ = spec.tensors[op['out']]
    x, e_in = xb.model_input(np.random.default_rng(seed), B, H, W, C)
    scale, bias = xb.fold(spec.layers[0], w)
    if op['type'] == ns.OP_CONV:
        got, e_out = xb.model_conv(x, e_in, w['l/kernel'], scale, bias, op, ho, wo, out=out, mutate=mutate)
    else:
        got, e_out = xb.model_dw(x, e_in, w['l/kernel'], scale, bias, op, ho, wo)
    fmt = ('split', e_out) if out == 'split' else ('f32',)
    Y, E = xb.run_chain(spec, w, {0: x}, [0], {op['out']: fmt})
    if out == 'split':
        ok, over, msg = xb.split_health(got, e_out)
        assert ok, msg
        assert xb.is_split(got, e_out).all()
    r, idx = xb.compare(got, Y[op['out']], E[op['out']])
    return r, idx, e_in


LAYERS = {
    'stem_K27': ('conv', 9, 11, 3, 8, 3, 2),
    'pw_K384': ('conv', 4, 6, 384, 16, 1, 1),
    'conv3x3_K3456': ('conv', 4, 4, 384, 8, 3, 1),
    'conv3x3_K9216': ('conv', 3, 3, 1024, 4, 3, 1),
    'dw3x3': ('dw', 7, 6, 24, 24, 3, 2, ns.RELU),
    'pw_K124': ('conv', 4, 5, 124, 16, 1, 1),
    'conv3x3_K288': ('conv', 6, 5, 32, 8, 3, 1),
}


@pytest.mark.parametrize('name', ['stem_K27', 'pw_K384', 'conv3x3_K3456', 'conv3x3_K9216', 'dw3x3', 'pw_K124', 'conv3x3_K288'])
def test_correct_model_is_accepted_with_margin(name):
    r, idx, _ = _run(*_layer(*LAYERS[name]))
    print(f'{name}: error / E = {r:.3f} at {idx}')
    assert r <= 0.25, (name, r, idx)


def test_correct_model_fp32_output_is_accepted():
    r, idx, _ = _run(*_layer(*LAYERS['pw_K384']), out='f32')
    assert r <= 0.25, (r, idx)


@pytest.mark.parametrize('layer,mutate', [
    ('pw_K384', ('drop_lohi',)),                     # w_lo * x_hi dropped in the whole layer
    ('pw_K384', ('drop_hilo_step', 5)),              # w_hi * x_lo dropped in a single k-step of 32
    ('conv3x3_K288', ('wrap_col', 0)),               # one border column: a wrapped tap instead of the zero tap
    ('pw_K124', ('tail_nonzero',)),                  # the last partial channel group read as non-zero
    ('pw_K384', ('hi_only',)),                       # the output stored as hi only
    ('pw_K384', ('mate_exponent', 0)),               # the exponent of one image taken from its batch mate
])
def test_defect_is_rejected(layer, mutate):
    spec, w = _layer(*LAYERS[layer])
    good, _, e_in = _run(spec, w)
    bad, idx, _ = _run(spec, w, mutate)
    print(f'{layer} {mutate}: error / E = {bad:.3g} at {idx} (correct model: {good:.3f})')
    if mutate[0] == 'mate_exponent':
        assert e_in[0] != e_in[1]                    # the frames of a batch must differ in magnitude for this defect to show
    assert good <= 0.25
    assert bad > 1.0, (layer, mutate, bad)


def test_compare_leaves_no_element_out():
    ref = np.zeros((1, 2, 2, 3))
    E = np.full(ref.shape, 1e-3)
    got = ref.copy()
    assert xb.compare(got, ref, E)[0] == 0.0
    got[0, 1, 0, 2] = 2e-3
    r, idx = xb.compare(got, ref, E)
    assert abs(r - 2.0) < 1e-12 and idx == (0, 1, 0, 2)
    E[0, 1, 0, 2] = 0.0                              # a zero bound demands an exact value
    assert xb.compare(got, ref, E)[0] == np.inf
    got[0, 1, 0, 2] = np.nan
    assert xb.compare(got, ref, np.full(ref.shape, 1e-3))[0] == np.inf


def test_c_dot_is_what_the_model_gives():
    c, least = xb.derive_c()
    print(f'4 x worst ratio of the correct model {c:.2f}; smallest ratio with a cross product dropped {least:.1f}')
    assert c <= xb.C_DOT <= 1.25 * c                 # the constant is the derived figure rounded up, not a tuned one
    assert 8 * xb.C_DOT <= least


def test_split_format_helpers():
    rng = np.random.default_rng(0)
    y = rng.normal(0, 3, (2, 3, 3, 8)).astype(np.float32)
    e = xb.exp_of(np.abs(y).reshape(2, -1).max(1) * 2.0 ** 7)
    got, hi, lo = xb.store_split(y, e)
    assert (np.abs(got - y) <= 2.0 ** -22 * np.abs(y) + np.ldexp(1.0, e - 25).reshape(2, 1, 1, 1)).all()
    assert xb.is_split(got, e).all() and not xb.is_split(y, e).all()        # 24-bit values are not hi + lo
    ok, over, _ = xb.split_health(got, e)
    assert ok and 2.0 ** 7 <= over < 2.0 ** 9
    assert not xb.split_health(got, e - 20)[0]                              # scaled maximum past fp16
    assert not xb.split_health(got, e + 10)[0]                              # over-estimate 2^17
    for bound in (1.0, 1.5, 2.0 ** 13, 3e-5, 65504.0):
        s = bound * 2.0 ** -int(xb.exp_of(bound))
        assert 2.0 ** 13 <= s < 2.0 ** 14
    assert int(xb.exp_of(0.0)) == 0 and int(xb.exp_of(np.inf)) == 0


def test_propagated_bound_dominates_in_float64():
    """depthwise -> 1x1: move the inner tensor by its E with random signs; the output moves by at most the propagated part of E."""
    s = ns.NetSpec('dwpw', (6, 7))
    x = s._new_tensor(6, 7, 48)
    d = s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='dw')
    y = s.conv(d, 24, 1, act=ns.LEAKY03, name='pw')
    w = s.init_weights(seed=4)
    rng = np.random.default_rng(1)
    x0, _ = xb.model_input(rng, B, 6, 7, 48)
    Y, E = xb.run_chain(s, w, {x: x0}, [0, 1], {d: ('inner',), y: ('f32',)})
    assert (E[d] > 0).all() and (E[y] > 0).all()
    _, E_own = xb.run_chain(s, w, {d: Y[d]}, [1], {y: ('f32',)})                        # the second op's own rounding alone
    prop = E[y] - E_own[y]
    assert (prop > 0).all()
    for _ in range(8):
        moved = Y[d] + E[d] * rng.choice([-1.0, 1.0], E[d].shape)
        Ym, _ = xb.run_chain(s, w, {d: moved}, [1], bounds=False)
        assert (np.abs(Ym[y] - Y[y]) <= prop * (1 + 1e-12)).all()
    Y2, E2 = xb.run_chain(s, w, {d: Y[d]}, [1], {y: ('f32',)}, e_inputs={d: E[d]})     # the same bound from an inexact input
    np.testing.assert_allclose(E2[y], E[y], rtol=1e-12)


@pytest.mark.parametrize('net,shape,alpha', [('yolo_mobilev1', (64, 96, 3), 0.5), ('yolo_mobilev2', (64, 96, 3), 1.0),
                                             ('tiny_yolo', (64, 64, 3), 1.0), ('yolo', (64, 96, 3), 1.0)])
def test_chain_runner_equals_torch_reference_on_whole_networks(net, shape, alpha):
    spec = getattr(ns, net)(shape, 3, 20, alpha=alpha)
    w = spec.init_weights(seed=1)
    x = np.random.default_rng(2).random((2, *shape))
    want = [op['out'] for op in spec.ops]
    ref = torch_net_ref.forward(spec, w, x, want=want, keep_dtype=True)
    Y, _ = xb.run_chain(spec, w, {0: x}, bounds=False)
    for t in want:
        assert ref[t].dtype == np.float64
        assert np.abs(Y[t] - ref[t]).max() <= 1e-12 * np.abs(ref[t]).max(), (net, t)


def test_launch_chain_walks_back_to_stored_tensors():
    spec = ns.yolo_mobilev1((64, 96, 3), 3, 20, alpha=0.5)
    stored = {0, spec.ops[2]['out'], spec.ops[4]['out']}                    # the stem + dw + pw block, then dw + pw
    assert xb.launch_chain(spec, stored, spec.ops[2]['out']) == ([0, 1, 2], [0])
    assert xb.launch_chain(spec, stored, spec.ops[4]['out']) == ([3, 4], [spec.ops[2]['out']])
    y2 = spec.outputs[1]                                                    # conv1x1 <- conv3x3 <- concat <- (upsample <- conv1x1, x1)
    rows, ins = xb.launch_chain(spec, {0, spec.ops[22]['out'], spec.ops[26]['out']}, y2)
    assert [spec.ops[i]['type'] for i in rows] == [ns.OP_CONV, ns.OP_UPSAMPLE, ns.OP_CONCAT, ns.OP_CONV, ns.OP_CONV]
    assert ins == sorted([spec.ops[22]['out'], spec.ops[26]['out']])
