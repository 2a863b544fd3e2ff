"""equalize.equalize (cross-layer range equalisation) on the constructed network of tests/equalize_net.py.  CPU only.

The function and the contracts are checked on a float64 checkpoint, where the rule is exact to float64 (rtol 1e-9 leaves room for the sums
of a forward pass); a float32 checkpoint rounds every changed tensor once, so there the function is held to 2^-24 relative per tensor,
compounded over the ~6 layers of a path and their 9 .. 216-term sums: 1e-5 of the output's magnitude."""
import numpy as np
import pytest

from k210_yolo_framework_amd import equalize as eq, netspec as ns, quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from oracle import kpu_ref
from tests import equalize_net as en

MAX_GAIN = 64.0


@pytest.fixture(scope='module')
def done():
    s, w, fr, T = en.case()
    cr = en.channel_ranges(s, T)
    after_a, g, skipped = eq.equalize_activations(s, w, cr, MAX_GAIN)
    new, rep = eq.equalize(s, w, cr, MAX_GAIN)
    return s, w, fr, T, cr, after_a, g, skipped, new, rep


def _chan(l):
    return 3 if l.kind == 'conv' else 2


def test_the_function_is_kept(done):
    s, w, fr, T, cr, after_a, g, skipped, new, rep = done
    assert sorted(new) == sorted(w)
    for k in w:
        assert new[k].shape == w[k].shape and new[k].dtype == w[k].dtype, k
    held = en.frames(4, 99)
    for frames in (fr, held):
        a, b = en.forward(s, w, frames), en.forward(s, new, frames)
        for t in s.outputs:
            np.testing.assert_allclose(b[t], a[t], rtol=1e-9, atol=0)
    assert any((new[k] != w[k]).any() for k in w)                              # and it did something


def test_a_float32_checkpoint_stays_float32_and_keeps_the_function_to_its_rounding():
    s, w, fr, T = en.case('float32')
    new, _ = eq.equalize(s, w, en.channel_ranges(s, T), MAX_GAIN)
    assert all(new[k].dtype == np.float32 for k in w)
    b = en.forward(s, new, fr)
    for t in s.outputs:
        assert np.abs(b[t] - T[t]).max() <= 1e-5 * np.abs(T[t]).max()


def test_the_input_dict_is_not_mutated():
    s, w, fr, T = en.case()
    mine = {k: v.copy() for k, v in w.items()}
    before = {k: v.copy() for k, v in mine.items()}
    new, _ = eq.equalize(s, mine, en.channel_ranges(s, T), MAX_GAIN)
    for k in before:
        assert mine[k].tobytes() == before[k].tobytes(), k
        assert new[k] is not mine[k] and not np.shares_memory(new[k], mine[k])


def test_the_contract_of_step_b(done):
    """Against the weights step B is given (step A's result): step A rescales the input channels of a reader's kernel, which is that
    kernel's range from then on."""
    s, w, fr, T, cr, after_a, g, skipped, new, rep = done
    T_a = en.forward(s, after_a, fr)
    _, rep_a = quantize.quantize(s, after_a, en.tensor_ranges(s, T_a))
    T_n = en.forward(s, new, fr)
    _, rep_n = quantize.quantize(s, new, en.tensor_ranges(s, T_n))
    stretched = 0
    for l in s.layers:
        k0, k1 = after_a[l.name + '/kernel'], new[l.name + '/kernel']
        if not l.bn_name:
            assert k1.tobytes() == k0.tobytes() and new[l.name + '/bias'].tobytes() == after_a[l.name + '/bias'].tobytes()
            continue
        assert k0.min() < 0 < k0.max()
        assert k1.min() == k0.min() and k1.max() == k0.max(), l.name
        assert (rep_n['layers'][l.name]['s_w'], rep_n['layers'][l.name]['zp_w']) == (rep_a['layers'][l.name]['s_w'], rep_a['layers'][l.name]['zp_w'])
        assert ((k1 == 0) == (k0 == 0)).all(), l.name                           # zeros stay zeros, nothing else becomes one
        f = rep['gains'][l.name][1]
        assert (f >= 1.0).all() and (f <= MAX_GAIN).all()
        ax = tuple(i for i in range(4) if i != _chan(l))
        cmax, cmin = k1.max(axis=ax), k1.min(axis=ax)
        live = np.abs(k0).max(axis=ax) > 0
        for c in np.flatnonzero(live & (f < MAX_GAIN)):
            top = abs(np.float32(cmax[c]) - np.float32(k0.max())) <= 4 * np.spacing(np.float32(k0.max()))
            bot = abs(np.float32(cmin[c]) - np.float32(k0.min())) <= 4 * np.spacing(np.abs(np.float32(k0.min())))
            assert top or bot, (l.name, c, cmax[c], cmin[c], k0.max(), k0.min())
        stretched += int((f > 1.0).sum())
        # the compensation: folded scale / f, folded bias unchanged
        sc0, b0 = quantize.fold_bn(l, after_a)
        sc1, b1 = quantize.fold_bn(l, new)
        np.testing.assert_allclose(sc1 * f, sc0, rtol=1e-12)
        np.testing.assert_allclose(b1, b0, rtol=1e-9, atol=1e-12 * np.abs(b0).max())
    assert stretched > 40
    name, c = en.DEAD                                                           # the dead channel: nothing of it moved, in either step
    for key in ('/kernel', '_bn/gamma', '_bn/beta', '_bn/moving_mean', '_bn/moving_variance'):
        a, b = w[name + key], new[name + key]
        assert np.take(a, c, axis=2 if key == '/kernel' else 0).tobytes() == np.take(b, c, axis=2 if key == '/kernel' else 0).tobytes(), key
    assert rep['gains'][name][0][c] == 1.0 and rep['gains'][name][1][c] == 1.0


EQUALISED = {'conv_dw_1': 'conv_pw_1', 'conv_pw_1': 'conv_dw_2', 'conv_dw_2': 'conv_pw_2', 'head_conv_1': 'head_conv_2', 'head_conv_4': 'head_conv_5'}
SKIPPED = {'conv1': '2 readers', 'conv_pw_2': '2 readers', 'head_conv_3': 'read by `upsample`', 'head_conv_2': 'a network output',
           'head_conv_5': 'a network output'}


def test_the_contract_of_step_a(done):
    """On step A's own result.  `bit-identical` for a skipped tensor: everything that makes it - its producer's BatchNorm (or bias) and the
    output channels of its kernel - is unchanged bit for bit, and with float64 weights so is the tensor of the forward pass where its inputs
    are; the output convs keep bias and output channels (their INPUT channels are the reader side of head_conv_1 / head_conv_4)."""
    s, w, fr, T, cr, after_a, g, skipped, new, rep = done
    lay = {l.name: l for l in s.layers}
    out_of = {op['layer']: op['out'] for op in s.ops if op.get('layer')}
    assert {r['tensor']: r['reason'] for r in skipped} == SKIPPED and sorted(g) == sorted(EQUALISED)
    assert rep['skipped'] == skipped
    T_a = en.forward(s, after_a, fr)
    seen_clamp = seen_free = 0
    for name, reader in EQUALISED.items():
        gl = g[name]
        assert (gl >= 1.0 / MAX_GAIN).all() and (gl <= MAX_GAIN).all()
        t = out_of[name]
        ext0 = np.abs(T[t]).max(axis=(0, 1, 2))
        ext1 = np.abs(T_a[t]).max(axis=(0, 1, 2))
        np.testing.assert_allclose(ext1, gl * ext0, rtol=1e-9)                  # the tensor's channel c is the old one times g_c
        np.testing.assert_allclose(ext1.max(), ext0.max(), rtol=1e-9)           # the overall extent is kept
        free = (gl > 1.0 / MAX_GAIN) & (gl < MAX_GAIN) & (ext0 > 0)
        rk0, rk1 = w[reader + '/kernel'], after_a[reader + '/kernel']
        np.testing.assert_allclose(rk1 * gl.reshape(1, 1, -1, 1), rk0, rtol=1e-12)
        if lay[reader].kind == 'dwconv':
            np.testing.assert_allclose(ext1[free], ext0.max(), rtol=1e-9)       # every free channel fills the tensor's range
        else:
            r1 = np.abs(rk1).max(axis=(0, 1, 3))
            free &= np.abs(rk0).max(axis=(0, 1, 3)) > 0
            ratio = ext1[free] / r1[free]                                       # extent_c / r_c is one number: equal shares of the two ranges
            np.testing.assert_allclose(ratio, ratio[0], rtol=1e-9)
            if free[np.argmax(ext1)] and free[np.argmax(r1)]:
                np.testing.assert_allclose(ext1[free] / ext1.max(), r1[free] / r1.max(), rtol=1e-9)
        seen_clamp += int((~free & (ext0 > 0)).sum())
        seen_free += int(free.sum())
    assert seen_free > 40
    print('channels free', seen_free, 'clamped', seen_clamp)
    for name in ('conv1', 'conv_pw_2', 'head_conv_3'):                          # skipped producers with BatchNorm
        for key in ('_bn/gamma', '_bn/beta', '_bn/moving_mean', '_bn/moving_variance'):
            assert after_a[name + key].tobytes() == w[name + key].tobytes(), (name, key)
    assert after_a['conv1/kernel'].tobytes() == w['conv1/kernel'].tobytes()
    assert T_a[out_of['conv1']].tobytes() == T[out_of['conv1']].tobytes()       # feeds concat: the tensor itself, bit for bit
    for name in ('head_conv_2', 'head_conv_5'):
        assert after_a[name + '/bias'].tobytes() == w[name + '/bias'].tobytes()
        assert new[name + '/kernel'].tobytes() == after_a[name + '/kernel'].tobytes()


def test_a_clamp_that_is_active_still_keeps_the_extent():
    a = np.array([1.0, 1e-4, 0.5, 0.0, 2e-3])
    r = np.array([1e-3, 1.0, 0.5, 1.0, 0.0])
    g = eq.activation_gains(a, r, 8.0)
    assert (g >= 1 / 8.0).all() and (g <= 8.0).all() and g[3] == 1.0 and g[4] == 1.0
    assert g[1] == 8.0                                                          # wanted far more
    np.testing.assert_allclose((g * a).max(), 1.0, rtol=1e-12)
    g = eq.activation_gains(a, None, 8.0)
    assert g.tolist() == [1.0, 8.0, 2.0, 1.0, 8.0]


def _rms_error(s, w_float, T_float_outs, w_q, fr):
    Tq = en.forward(s, w_q, fr)
    km, _ = quantize.quantize(s, w_q, en.tensor_ranges(s, Tq))
    num = den = 0.0
    for b in range(len(fr)):
        outs = kpu_ref.run(km, np.ascontiguousarray(fr[b].transpose(2, 0, 1)))
        for o, ref in zip(outs, T_float_outs):
            num += float(((o.astype(np.float64) - ref[b].transpose(2, 0, 1)) ** 2).sum())
            den += float((ref[b] ** 2).sum())
    return np.sqrt(num / den)


def test_it_helps_where_it_must(done):
    """Ranges by numpy from the float64 forward (per tensor for the quantiser, per channel for the rule), both files through the CPU oracle
    on the calibration frames: RMS error of the dequantised outputs against the float forward, relative to the outputs' RMS.
    Measured when this was written: 0.071552 without, 0.029575 with equalisation."""
    s, w, fr, T, cr, after_a, g, skipped, new, rep = done
    ref = [T[t] for t in s.outputs]
    e_off, e_on = _rms_error(s, w, ref, w, fr), _rms_error(s, w, ref, new, fr)
    print(f'relative RMS error of the outputs: unequalised {e_off:.6f}, equalised {e_on:.6f}')
    assert e_off > 0.01                                                         # the constructed spread does hurt: at least 1 % of the outputs' RMS
    assert e_on < e_off


def test_the_report_is_printed_and_bn_mul_min_is_reported(done):
    s, w, fr, T, cr, after_a, g, skipped, new, rep = done
    _, qrep = quantize.quantize(s, new, en.tensor_ranges(s, en.forward(s, new, fr)))
    assert all(r['bn_mul_min'] > 0 for r in qrep['layers'].values())
    plain = quantize.format_report(qrep)
    assert 'equalised' not in plain
    qrep['equalize'] = rep
    text = quantize.format_report(qrep)
    assert text.startswith(plain[:plain.rindex('main memory')])
    assert 'equalised (max_gain 64)' in text and 'conv_dw_2' in text and 'not equalised: head_conv_3 (read by `upsample`)' in text
    r = rep['layers']['conv_pw_1']
    assert r['a_changed'] > 0 and r['g_max'] > 1.0 and rep['layers']['conv_dw_2']['f_max'] > 1.0
    assert rep['layers']['head_conv_2'] == dict(a_changed=0, g_min=1.0, g_max=1.0, b_changed=0, f_min=1.0, f_max=1.0)


@pytest.mark.parametrize('max_gain', [1.0, 0.5, 0.0, -3.0, float('nan'), float('inf')])
def test_max_gain_at_or_below_one_is_refused(max_gain):
    s, w, fr, T = en.case()
    with pytest.raises(KmodelError, match='max_gain'):
        eq.equalize(s, w, en.channel_ranges(s, T), max_gain)


def test_a_missing_layer_and_a_wrong_channel_count_are_refused_by_name():
    s, w, fr, T = en.case()
    cr = en.channel_ranges(s, T)
    less = {k: v for k, v in cr.items() if k != 'conv_dw_2'}
    with pytest.raises(KmodelError, match="conv_dw_2"):
        eq.equalize(s, w, less)
    wrong = dict(cr)
    wrong['conv_pw_1'] = (cr['conv_pw_1'][0][:-1], cr['conv_pw_1'][1][:-1])
    with pytest.raises(KmodelError, match="conv_pw_1.*16 output channels"):
        eq.equalize(s, w, wrong)
    bad = dict(cr)
    bad['head_conv_1'] = (cr['head_conv_1'][0], np.where(np.arange(16) == 2, np.inf, cr['head_conv_1'][1]))
    with pytest.raises(KmodelError, match="head_conv_1"):
        eq.equalize(s, w, bad)


def test_the_cli_refuses_equalize_with_ranges_by_name(capsys):
    from k210_yolo_framework_amd import make_kmodel
    with pytest.raises(SystemExit):
        make_kmodel.cli(['a.h5', 'b.kmodel', '--ranges', 'r.npz', '--equalize', 'True'])
    assert '--equalize cannot be combined with --ranges' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        make_kmodel.cli(['a.h5', 'b.kmodel', '--synthetic', '4', '--equalize', 'True', '--equalize_max_gain', '1'])
    assert '--equalize_max_gain' in capsys.readouterr().err
