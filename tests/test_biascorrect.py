"""Bias correction (biascorrect.py) and quantize(bn_add_delta=): the rule on the CPU, with a numpy `measure`.  No device needed."""
import numpy as np
import pytest

from k210_yolo_framework_amd import biascorrect, kmodel, quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from tests import biascorrect_cases as bc

BOUND = 0.5 + 1e-6                                         # half a unit of z (2^-p output steps), + the float64 slack of the comparison itself


@pytest.fixture(scope='module')
def mini():
    spec, w, fr, fm, ranges = bc.mini_case()
    km, rep = quantize.quantize(spec, w, ranges)
    return spec, w, fr, fm, ranges, km, rep


def test_no_delta_and_an_empty_delta_serialise_to_the_same_bytes(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    want = kmodel.serialise(km)
    for d in (None, {}):
        km2, rep2 = quantize.quantize(spec, w, ranges, bn_add_delta=d)
        assert kmodel.serialise(km2) == want
        assert not any('bias_delta_max' in r for r in rep2['layers'].values())


def test_a_delta_changes_exactly_that_layers_bn_add_by_exactly_the_delta(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    name = 'conv_pw_2'
    co = len(km.layers[rep['layers'][name]['index']].bn_add)
    d = (np.arange(co, dtype=np.int64) - 7) * 1000
    km2, rep2 = quantize.quantize(spec, w, ranges, bn_add_delta={name: d})
    assert len(km2.layers) == len(km.layers)
    for a, b in zip(km.layers, km2.layers):
        if isinstance(a, kmodel.ConvLayer):
            for f in ('weights', 'bn_mul', 'bn_shift', 'act_start', 'act_mul', 'act_shift', 'act_bias'):
                assert np.array_equal(getattr(a, f), getattr(b, f)), (a.index, f)
            for f in ('src_addr', 'dst_addr', 'pad_value', 'arg_x', 'arg_w', 'arg_add', 'shr_x', 'shr_w', 'pool_type', 'flags', 'main_mem_out'):
                assert getattr(a, f) == getattr(b, f), (a.index, f)
            want = a.bn_add + d if a.index == rep['layers'][name]['index'] else a.bn_add
            assert np.array_equal(b.bn_add, want), a.index
        else:
            assert a.type == b.type and set(a.fields) == set(b.fields)
            for k_, v in a.fields.items():
                assert np.array_equal(v, b.fields[k_]), (a.index, k_)
    assert kmodel.serialise(km2) != kmodel.serialise(km)
    p = rep2['layers'][name]['fine_bits']
    assert rep2['layers'][name]['bias_delta_max'] == float(np.abs(d).max()) / 2 ** p
    assert 'bias_delta_max' not in rep2['layers']['conv1']


def test_unknown_layer_wrong_length_and_overflow_raise(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    with pytest.raises(KmodelError, match='no_such_layer'):
        quantize.quantize(spec, w, ranges, {'no_such_layer': np.zeros(8, np.int64)})
    with pytest.raises(KmodelError, match='conv1'):
        quantize.quantize(spec, w, ranges, {'conv1': np.zeros(7, np.int64)})
    with pytest.raises(KmodelError, match='conv1'):
        quantize.quantize(spec, w, ranges, {'conv1': np.zeros(8, np.float64)})
    with pytest.raises(KmodelError, match='bn_add'):
        quantize.quantize(spec, w, ranges, {'conv1': np.full(8, 1 << 31, np.int64)})         # past the 32-bit field: conv_registers' check


def test_steps_and_counts_of_the_mini_network(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    steps = biascorrect.steps_of(km)
    by_name = {name: steps[r['index']] for name, r in rep['layers'].items()}
    assert {n for n, s in by_name.items() if s == 2} == {'conv_dw_2', 'conv_dw_4'}      # the deferred stride-2 depthwise convs, and only they
    counts = biascorrect.counted(km, len(fr))
    for name, r in rep['layers'].items():
        assert counts[r['index']] == fm[name][1], name                                      # the spec's tensor: half size for the deferred ones
    c = km.layers[rep['layers']['conv_dw_2']['index']]
    assert counts[c.index] == len(fr) * (c.out_h // 2) * (c.out_w // 2)


def test_correct_brings_every_channel_mean_within_half_a_unit(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    measure = bc.numpy_measure(fr)
    before = biascorrect.residuals(rep, fm, measure(km))
    worst = {n: float(v.max()) for n, v in before.items()}
    print('before, worst |mean z - T| per layer (units of 2^-p codes):', worst)
    assert max(worst.values()) > 0.5                       # the condition on the inputs: there is something to correct
    delta, brep = biascorrect.correct(spec, w, ranges, fm, measure)
    assert brep['passes'] == len(rep['layers']) and list(delta) == list(rep['layers'])
    km2, rep2 = quantize.quantize(spec, w, ranges, delta)
    after = biascorrect.residuals(rep2, fm, measure(km2))
    assert 'conv_dw_2' in after and 'conv_dw_4' in after
    checked = 0
    for name, v in after.items():
        keep = np.setdiff1d(np.arange(len(v)), brep['layers'][name]['limited'])
        print(f'{name}: after {float(v[keep].max()):.4f}, before {worst[name]:.1f}, limited {brep["layers"][name]["limited"]}')
        assert (v[keep] <= BOUND).all(), (name, v)
        checked += len(keep)
    assert checked >= sum(len(v) for v in after.values()) - 2          # (the limit is for broken channels: it must not hollow the check out)
    text = quantize.format_report(dict(rep2, biascorrect=brep))
    assert text.count('bias-corrected ') == len(rep['layers']) and 'bias correction:' in text


def test_the_limit_is_applied_and_reported(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    far = {n: (s.copy(), c) for n, (s, c) in fm.items()}
    r = rep['layers']['conv1']
    far['conv1'][0][3] += 1000.0 * r['s_y'] * far['conv1'][1]                               # channel 3's float mean 1000 codes away
    delta, brep = biascorrect.correct(spec, w, ranges, far, bc.numpy_measure(fr))
    assert brep['layers']['conv1']['limited'] == [3]
    assert delta['conv1'][3] == biascorrect.LIMIT_CODES << r['fine_bits']
    assert brep['layers']['conv1']['delta_max'] == float(biascorrect.LIMIT_CODES)
    assert 'LIMITED channels [3]' in biascorrect.format_report(brep)


def test_a_count_that_differs_from_the_float_side_is_refused(mini):
    spec, w, fr, fm, ranges, km, rep = mini
    with pytest.raises(KmodelError, match='conv1'):
        biascorrect.correct(spec, w, ranges, fm, bc.numpy_measure(fr[:1]))
