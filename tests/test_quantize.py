"""The quantiser (quantize.quantize) against the KPU oracle on a small graph, and its refusals.  CPU only."""
import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import kmodel, netspec as ns, quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from oracle import kpu_ref, torch_net_ref


def small_spec(hw=(32, 48)):
    """stem 3x3 s2, dw + pw pairs (two of them stride 2), the upsample + concat head, two linear outputs: yolo_mobilev1 in miniature."""
    s = ns.NetSpec('yolo_mobilev1', hw, anchor_num=3, class_num=1)
    x = s._new_tensor(hw[0], hw[1], 3)
    x = s.conv(x, 8, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    x1 = None
    for i, (f, st) in enumerate([(16, 1), (32, 2), (32, 1), (64, 2)], start=1):
        x = s.dwconv(x, st, ns.K210_S2_PAD if st == 2 else ns.SAME3, act=ns.RELU, name=f'conv_dw_{i}')
        x = s.conv(x, f, 1, act=ns.LEAKY03, name=f'conv_pw_{i}')
        if i == 3:
            x1 = x
    ns._head(s, x1, x, 24, 16, 16, 3 * 6, [0])
    return s


def frames(n, hw, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def oracle_tensors(spec, w, fr):
    x = fr.astype(np.float32) * np.float32(quantize.INPUT_SCALE)
    t = torch_net_ref.forward(spec, w, x, want=list(range(1, len(spec.tensors))), dtype=torch.float64)
    t[0] = x
    return t


def oracle_ranges(spec, w, fr):
    names = quantize.tensor_names(spec)
    return {names[i]: (float(v.min()), float(v.max())) for i, v in oracle_tensors(spec, w, fr).items()}


def error_bound(spec, w, km, rep, T):
    """Worst-case |dequantised KPU tensor - float tensor| per tensor, derived - not measured - from the number formats:

    input: 0 (q / 255 is the float input).  A conv with input error e_x, taps K, folded BatchNorm (scale_c, bias_c), weight step s_w, output
    step s_y and FINE_BITS p sees its pre-activation t_c = scale_c sum(x w) + bias_c perturbed by at most
        |scale_c| (sum|w| e_x  +  K (max|x| + e_x) s_w / 2)               input error through the layer's gain + every weight off by <= s_w / 2
      + s_y (K 255^2 / 2^(shift_c + p + 1)  +  2 / 2^p  +  1 / 2^(p + 1))  bn_mul rounded to 1/2 in its last bit on |acc| <= K 255^2, the floor of
                                                                            the shift and the slope's 2^-14 on the table, bn_add rounded
    The activation has slope <= 1 (its negative slope is stored to 2^-15: + max|t| 2^-15), then the table rounds to the output grid (s_y / 2)
    and the integer zero point moves the range's ends by at most s_y / 2, which clips by no more than that; a value pushed outside the range by
    the error above is clipped TOWARDS the true value, which lies inside.  So  e_y = max_c(...) + s_y.
    upsample copies; a concat input is re-rounded onto the union grid: e + s_u (rounding + moved ends).  DEQUANTIZE is exact in float64 up to
    fp32 rounding of (scale, bias): 256 * 2^-24 relative, added at the outputs.
    This is a worst case over every sign pattern, compounded through ~10 layers of L1 gains: it holds by construction and is far above what
    the model does (the test prints both); the assertion with teeth is the RMS one beside it."""
    names = quantize.tensor_names(spec)
    lay = {l.name: l for l in spec.layers}
    e = {0: 0.0}
    convs = {c.index: c for c in km.convs}
    for op in spec.ops:
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            l, r = lay[op['layer']], rep['layers'][op['layer']]
            c = convs[r['index']]
            k = np.asarray(w[l.name + '/kernel'], np.float64)
            absw = np.abs(k).sum((0, 1, 3)) if l.kind == 'dwconv' else np.abs(k).sum((0, 1, 2))
            K = 9 if l.kind == 'dwconv' else k.shape[0] * k.shape[1] * k.shape[2]
            scale, bias = quantize.fold_bn(l, w)
            ex, xmax = e[op['in0']], float(np.abs(T[op['in0']]).max())
            pre = np.abs(scale) * (absw * ex + K * (xmax + ex) * r['s_w'] / 2)
            p = r['fine_bits']
            fmt = r['s_y'] * (K * 255.0 ** 2 / np.exp2(c.bn_shift.astype(np.float64) + p + 1) + 2.0 / 2 ** p + 0.5 / 2 ** p)
            tmax = float(np.abs(T[op['out']]).max()) / (op['alpha'] if op['act'] == ns.ACT_LEAKY else 1.0)
            e[op['out']] = float((pre + fmt).max()) + tmax * 2.0 ** -15 + r['s_y']
        elif op['type'] == ns.OP_UPSAMPLE:
            e[op['out']] = e[op['in0']]
        else:
            lo = min(float(T[t].min()) for t in (op['in0'], op['in1']))
            hi = max(float(T[t].max()) for t in (op['in0'], op['in1']))
            s_u = (max(hi, 0) - min(lo, 0) + max(rep['layers'][names[t]]['s_y'] for t in (op['in1'],))) / 255.0   # union of the quantised ranges: at most one step wider
            e[op['out']] = max(e[op['in0']], e[op['in1']]) + s_u
    return e


@pytest.fixture(scope='module')
def small():
    spec = small_spec()
    w = spec.init_weights(seed=7)
    fr = frames(6, spec.in_hw, 11)
    ranges = oracle_ranges(spec, w, fr)
    km, rep = quantize.quantize(spec, w, ranges)
    return spec, w, fr, ranges, km, rep


def test_small_graph_packs_and_stays_within_the_derived_bound_of_the_float_network(small):
    spec, w, fr, ranges, km, rep = small
    kmodel.pack_kpu(km)                                    # accepted unchanged
    again = kmodel.parse(kmodel.serialise(km))
    T = oracle_tensors(spec, w, fr)
    bound = error_bound(spec, w, km, rep, T)
    names = quantize.tensor_names(spec)
    for b in range(len(fr)):
        chw = np.ascontiguousarray(fr[b].transpose(2, 0, 1))
        keep = {}
        outs = kpu_ref.run(km, chw, keep)
        for a, c in zip(outs, kpu_ref.run(again, chw)):
            assert a.tobytes() == c.tobytes()              # the written file computes the same
        for o, tid in zip(outs, spec.outputs):
            ref = T[tid][b].transpose(2, 0, 1)
            err = float(np.abs(o.astype(np.float64) - ref).max())
            lim = bound[tid] + 2.0 ** -16 * float(np.abs(ref).max() + 1)
            print(f'image {b} {names[tid]}: max error {err:.4f}, derived bound {lim:.4f}, output step {rep["layers"][names[tid]]["s_y"]:.4f}')
            assert err <= lim, (names[tid], err, lim)
    # and the error is of the size 8 bits promise, not merely below a loose bound: RMS within 5 % of the output's RMS - 255 steps per range
    # and ~10 layers of rounding noise, each around a third of a step, is ~1 %
    num = sum(((kpu_ref.run(km, np.ascontiguousarray(fr[0].transpose(2, 0, 1)))[i] - T[t][0].transpose(2, 0, 1)) ** 2).sum() for i, t in enumerate(spec.outputs))
    den = sum((T[t][0] ** 2).sum() for t in spec.outputs)
    print('relative RMS error', float(np.sqrt(num / den)))
    assert np.sqrt(num / den) <= 0.05


def test_layer_sequence_is_the_demos(small):
    spec, w, fr, ranges, km, rep = small
    kinds = [('conv', l.pool_type, bool(l.flags & 1)) if isinstance(l, kmodel.ConvLayer) else l.type for l in km.layers]
    K = kmodel
    assert kinds[-8:] == [K.KL_QUANTIZED_RESIZE_NN, K.KL_REQUANTIZE, K.KL_REQUANTIZE, K.KL_QUANTIZED_CONCAT, K.KL_K210_UPLOAD, ('conv', 0, False),
                          ('conv', 0, True), K.KL_DEQUANTIZE]
    by = {n: km.layers[r['index']] for n, r in rep['layers'].items()}
    assert by['conv1'].pool_type == K.POOL_LEFT_TOP_2_S2 and by['conv1'].pad_value == 0
    # a stride-2 depthwise conv runs at stride 1; its 1x1 successor pools (as nncase emits it)
    assert by['conv_dw_2'].pool_type == 0 and (by['conv_dw_2'].out_h, by['conv_dw_2'].out_w) == (16, 24)
    assert by['conv_pw_2'].pool_type == K.POOL_LEFT_TOP_2_S2 and (by['conv_pw_2'].out_h, by['conv_pw_2'].out_w) == (8, 12)
    assert by['conv_pw_3'].flags & K.KLF_MAIN_MEM_OUT           # leaves the KPU for the concat, and feeds conv_dw_4 on it
    assert len(km.outputs) == 2 and [s for _, s in km.outputs] == [4 * 18 * 4 * 6, 4 * 18 * 8 * 12]


def test_real_zero_is_the_integer_zero_point_in_every_tensor(small):
    spec, w, fr, ranges, km, rep = small
    for name, r in rep['layers'].items():
        c = km.layers[r['index']]
        for zp in (r['zp_x'], r['zp_w'], r['zp_y']):
            assert isinstance(zp, int) and 0 <= zp <= 255
        assert c.zp_x == r['zp_x'] == c.pad_value and c.zp_w == r['zp_w']          # exact: arg = -zp << 15, shr = 15
        assert c.arg_add == r['zp_x'] * r['zp_w'] * c.ksize ** 2
        lo, hi = ranges[name]
        assert -r['zp_y'] * r['s_y'] <= min(lo, 0) + r['s_y'] / 2 and (255 - r['zp_y']) * r['s_y'] >= max(hi, 0) - r['s_y'] / 2
    # an all-zero-point image region: a frame of zeros gives exactly act(bias) downstream - checked on the first layer, where the float
    # answer is known in closed form
    c = km.layers[rep['layers']['conv1']['index']]
    y = kpu_ref.conv(c, np.zeros((3, 32, 48), np.uint8))
    scale, bias = quantize.fold_bn(spec.layers[0], w)
    want = np.where(bias >= 0, bias, 0.3 * bias)
    got = (y[:, 4, 4].astype(np.float64) - rep['layers']['conv1']['zp_y']) * rep['layers']['conv1']['s_y']
    lo, hi = ranges['conv1']
    assert np.abs(got - np.clip(want, lo, hi)).max() <= rep['layers']['conv1']['s_y']


def test_pruned_weights_stay_exactly_at_the_zero_point():
    spec = small_spec()
    w = spec.init_weights(seed=7)
    rng = np.random.default_rng(3)
    masks = {}
    for l in spec.layers:
        if l.kind == 'conv':
            masks[l.name] = rng.uniform(size=l.kernel_shape) < 0.6
            w[l.name + '/kernel'] = np.where(masks[l.name], 0.0, w[l.name + '/kernel']).astype(np.float32)
    km, rep = quantize.quantize(spec, w, oracle_ranges(spec, w, frames(3, spec.in_hw, 5)))
    for name, m in masks.items():
        c = km.layers[rep['layers'][name]['index']]
        wq = c.weights.reshape(m.shape[3], m.shape[2], m.shape[0], m.shape[1]).transpose(2, 3, 1, 0)      # back to HWIO
        assert (wq[m] == rep['layers'][name]['zp_w']).all(), name
        assert rep['layers'][name]['zero_share'] >= m.mean()
    assert 'w==zp' in quantize.format_report(rep)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _any_ranges(spec):
    return {n: (-1.0, 4.0) for n in quantize.tensor_names(spec)}


def test_refuses_yolo_mobilev2_naming_add():
    spec = ns.yolo_mobilev2((224, 320, 3), 3, 20, alpha=1.0)
    with pytest.raises(KmodelError, match='`add`'):
        quantize.quantize(spec, spec.init_weights(1), _any_ranges(spec))


def test_refuses_tiny_yolo_naming_maxpool():
    spec = ns.tiny_yolo((224, 320, 3), 3, 20)
    with pytest.raises(KmodelError, match='`maxpool`'):
        quantize.quantize(spec, spec.init_weights(1), _any_ranges(spec))


def test_refuses_an_odd_input_size():
    s = ns.NetSpec('odd', (33, 48), anchor_num=3, class_num=1)
    x = s._new_tensor(33, 48, 3)
    y = s.conv(x, 8, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    s.outputs = [y]
    with pytest.raises(KmodelError, match="'conv1'.*stride 2.*33x48"):
        quantize.quantize(s, s.init_weights(1), _any_ranges(s))
    s = ns.NetSpec('pad', (32, 48), anchor_num=3, class_num=1)                   # Darknet's ((1,0),(1,0)) stride-2 padding
    y = s.conv(s._new_tensor(32, 48, 3), 8, 3, 2, (1, 0, 1, 0), act=ns.LEAKY01, name='conv2d_1')
    s.outputs = [y]
    with pytest.raises(KmodelError, match='padding \\(1, 0, 1, 0\\)'):
        quantize.quantize(s, s.init_weights(1), _any_ranges(s))
    s = ns.NetSpec('one', (32, 48), anchor_num=3, class_num=1)                   # a first layer that is not 3-channel
    y = s.conv(s._new_tensor(32, 48, 1), 8, 3, act=ns.LEAKY01, name='c')
    s.outputs = [y]
    with pytest.raises(KmodelError, match='3-channel'):
        quantize.quantize(s, s.init_weights(1), _any_ranges(s))


def test_a_range_of_zero_width_is_defined():
    """[0, 0] (a tensor that is constantly zero, e.g. a dead ReLU layer): scale 1/255, zero point 0 - nothing divides by zero, and the
    constant is exact."""
    assert quantize.qparams(0.0, 0.0) == (1.0 / 255.0, 0)
    assert quantize.qparams(2.0, 2.0) == (2.0 / 255.0, 0)                         # widened to contain zero first
    with pytest.raises(KmodelError):
        quantize.qparams(0.0, float('inf'))
    spec = small_spec()
    w = spec.init_weights(seed=7)
    w['conv_dw_2_bn/gamma'][:] = 0.0                                               # a dead layer: relu(beta) with beta <= 0
    w['conv_dw_2_bn/beta'][:] = -1.0
    fr = frames(2, spec.in_hw, 2)
    ranges = oracle_ranges(spec, w, fr)
    assert ranges['conv_dw_2'] == (0.0, 0.0)
    km, rep = quantize.quantize(spec, w, ranges)
    assert rep['layers']['conv_dw_2']['s_y'] == 1.0 / 255.0 and rep['layers']['conv_dw_2']['zp_y'] == 0
    keep = {}
    outs = kpu_ref.run(km, np.ascontiguousarray(fr[0].transpose(2, 0, 1)), keep)
    assert (keep[rep['layers']['conv_dw_2']['index']] == 0).all() and all(np.isfinite(o).all() for o in outs)


def test_refuses_a_tensor_too_large_for_kpu_ram():
    spec = ns.yolo_mobilev1((448, 640, 3), 3, 20, alpha=1.0)
    with pytest.raises(KmodelError, match="'conv1'.*KPU RAM"):
        quantize.quantize(spec, spec.init_weights(1), _any_ranges(spec))


def test_refuses_a_field_forced_past_its_width():
    spec = small_spec()
    w = spec.init_weights(seed=7)
    ranges = oracle_ranges(spec, w, frames(2, spec.in_hw, 2))
    w['head_conv_2/bias'] = w['head_conv_2/bias'].copy()
    w['head_conv_2/bias'][0] = 1e9                                                # bn_add = bias 2^10 / s_y: past 32 bits
    with pytest.raises(KmodelError, match='bn_add outside its 32-bit field'):
        quantize.quantize(spec, w, ranges)
    w = spec.init_weights(seed=7)
    w['conv_pw_1_bn/gamma'] = w['conv_pw_1_bn/gamma'] * 1e12                      # no 24-bit multiplier reaches this gain
    with pytest.raises(KmodelError, match='bn_mul'):
        quantize.quantize(spec, w, ranges)


def test_a_leaky_range_that_is_mostly_negative_is_widened_until_its_zero_point_fits_the_result_byte(small):
    """The table's result bias is a signed byte and holds the zero point at the kink: (-9, 1) would put it at 230."""
    spec, w, fr, ranges, _, _ = small
    km, rep = quantize.quantize(spec, w, dict(ranges, conv_pw_2=(-9.0, 1.0)))
    r = rep['layers']['conv_pw_2']
    assert r['zp_y'] == 127 and -127 * r['s_y'] <= -9.0 + r['s_y'] / 2 and r['range'] == (-9.0, 1.0)
    kmodel.pack_kpu(km)


def test_a_written_kmodel_of_another_depth_multiplier_loads_back_as_float_weights():
    """`load_weights('x.kmodel')` (what `keras_inference.py --precision kpu` does first) dequantises into the network it is loaded into, not
    only into the demo's alpha = 0.75.  The recovered float network differs from the original by the 8-bit rounding of the weights alone
    (uniform error of half a step on a 255-step range: ~0.1 % of the range per weight, a few per cent of a He-initialised layer's output
    over ~30 layers); 10 % relative RMS separates that from a wrong mapping, which gives ~100 %."""
    spec = ns.yolo_mobilev1((64, 96, 3), 3, 1, alpha=0.5)
    w = spec.init_weights(seed=3)
    fr = frames(2, spec.in_hw, 4)
    km, _ = quantize.quantize(spec, w, oracle_ranges(spec, w, fr))
    km = kmodel.parse(kmodel.serialise(km))
    back, rep = kmodel.to_float_weights(km, spec)
    assert abs(rep['layers']['conv_pw_1']['alpha'] - 0.3) < 1e-3 and rep['layers']['conv_dw_1']['alpha'] == 0.0
    x = fr.astype(np.float32) * np.float32(quantize.INPUT_SCALE)
    a = torch_net_ref.forward(spec, w, x, dtype=torch.float64)
    b = torch_net_ref.forward(spec, back, x, dtype=torch.float64)
    for o in spec.outputs:
        rel = float(np.sqrt(((a[o] - b[o]) ** 2).mean() / (a[o] ** 2).mean()))
        print('relative RMS', rel)
        assert rel <= 0.1
    with pytest.raises(KmodelError, match='loaded into'):
        kmodel.to_float_weights(km)                        # the demo's alpha = 0.75 is another network
    with pytest.raises(KmodelError, match='yolo_mobilev1 graph'):
        kmodel.to_float_weights(km, ns.tiny_yolo((224, 320, 3), 3, 20))
