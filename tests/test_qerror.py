"""The rule of qerror.py on closed forms (CPU, numpy): what `make kmodel ANALYZE=True` reports per conv layer."""
import json

import numpy as np
import pytest

from k210_yolo_framework_amd import qerror
from k210_yolo_framework_amd.kmodel import KmodelError

S_Y, ZP = 0.25, 7                                          # a power of two: (q - zp) * s_y is exact in fp32


def _codes(shape, seed=0, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def _exact(q):
    return ((q.astype(np.int32) - ZP) * np.float32(S_Y)).astype(np.float32)


def test_equal_tensors_give_inf_db_and_cosine_one():
    q = _codes((2, 5, 3, 4))
    f = qerror.figures(qerror.channel_sums(_exact(q), q, S_Y, ZP), S_Y)
    assert f['sqnr_db'] == np.inf and f['cosine'] == 1.0 and f['mean_err'] == 0.0 and f['max_err'] == 0.0
    assert np.all(f['channels']['sqnr_db'] == np.inf) and np.all(f['channels']['cosine'] == 1.0)
    assert f['n'] == 2 * 5 * 3 * 4 and not f['non_finite']


def test_constant_offset_is_exact():
    q = _codes((3, 4, 4, 2), seed=1)
    delta = 0.375                                          # 1.5 codes; exact in binary
    s = qerror.channel_sums(_exact(q) + np.float32(delta), q, S_Y, ZP)
    n = 3 * 4 * 4
    assert np.array_equal(s['n'], [n, n]) and np.array_equal(s['see'], [n * delta ** 2] * 2) and np.array_equal(s['se'], [n * delta] * 2)
    f = qerror.figures(s, S_Y)
    assert f['mean_err'] == delta / S_Y and f['max_err'] == delta / S_Y
    assert np.array_equal(f['channels']['mean_err'], [delta / S_Y] * 2)


def test_an_all_zero_channel_is_nan_and_not_ranked_worst():
    q = _codes((2, 4, 4, 3), seed=2)
    y = _exact(q) + np.float32(0.125)
    q[..., 1], y[..., 1] = ZP, 0.0                          # constantly zero, and exact
    f = qerror.figures(qerror.channel_sums(y, q, S_Y, ZP), S_Y, top=3)
    assert np.isnan(f['channels']['sqnr_db'][1]) and np.isnan(f['channels']['cosine'][1])
    assert [c for c, _ in f['worst']] in ([0, 2], [2, 0]) and np.isfinite(f['sqnr_db'])
    y[..., 2] = _exact(q)[..., 2]                           # an exact channel is inf dB: ranked, and last
    f = qerror.figures(qerror.channel_sums(y, q, S_Y, ZP), S_Y, top=3)
    assert [c for c, _ in f['worst']] == [0, 2] and f['worst'][1][1] == np.inf


def test_saturation_shares_on_crafted_codes():
    q = np.full((1, 2, 5, 2), 9, np.uint8)
    q[0, 0, :3, 0] = 255                                   # 3 of 10 at the top of channel 0
    q[0, 1, :, 1] = 0                                      # 5 of 10 at the bottom of channel 1
    q[0, 0, 0, 1] = 255
    f = qerror.figures(qerror.channel_sums(_exact(q), q, S_Y, ZP), S_Y)
    assert np.array_equal(f['sums']['n255'], [3, 1]) and np.array_equal(f['sums']['n0'], [0, 5])
    assert np.array_equal(f['channels']['share_255'], [0.3, 0.1]) and np.array_equal(f['channels']['share_0'], [0.0, 0.5])
    assert f['share_255'] == 4 / 20 and f['share_0'] == 5 / 20


def test_tensor_figures_are_the_figures_of_the_summed_channel_sums():
    rng = np.random.default_rng(3)
    q = _codes((2, 6, 5, 7), seed=3)
    y = (_exact(q) + rng.normal(0, 0.2, q.shape)).astype(np.float32)
    s = qerror.channel_sums(y, q, 0.1, ZP)
    f = qerror.figures(s, 0.1)
    syy, see, se, syh, shh, n = (s[k].sum() for k in ('syy', 'see', 'se', 'syh', 'shh', 'n'))
    s32 = float(np.float32(0.1))
    assert f['sqnr_db'] == 10.0 * np.log10(syy / see) and f['cosine'] == syh / np.sqrt(syy * shh)
    assert f['mean_err'] == se / n / s32 and f['max_err'] == s['emax'].max() / s32
    # and the sums are those of the definition, element by element
    yh = (q.astype(np.float64) - ZP) * s32
    assert np.array_equal(s['see'], ((y.astype(np.float64) - yh) ** 2).sum(axis=(0, 1, 2)))
    # two sets of positions add up
    both = qerror.add_sums(qerror.channel_sums(y[:1], q[:1], 0.1, ZP), qerror.channel_sums(y[1:], q[1:], 0.1, ZP))
    assert np.array_equal(both['n'], s['n']) and np.array_equal(both['emax'], s['emax']) and np.allclose(both['see'], s['see'], rtol=1e-14, atol=0)


def test_step_two_compares_every_other_code_position():
    q = _codes((1, 5, 4, 2), seed=4)                        # odd height, even width
    y = _exact(q[:, ::2, ::2])
    s = qerror.channel_sums(y, q, S_Y, ZP, step=2)
    assert np.array_equal(s['n'], [3 * 2] * 2) and np.array_equal(s['see'], [0.0, 0.0])
    with pytest.raises(KmodelError):
        qerror.channel_sums(y, q, S_Y, ZP, step=1)


def test_a_nan_or_an_infinity_is_not_added_and_flags_its_channel():
    q = _codes((2, 3, 3, 3), seed=5)
    y = _exact(q) + np.float32(0.25)
    want = qerror.channel_sums(np.delete(y.reshape(-1, 3), 4, axis=0).reshape(1, 17, 1, 3), np.delete(q.reshape(-1, 3), 4, axis=0).reshape(1, 17, 1, 3),
                               S_Y, ZP)
    bad = y.copy()
    bad.reshape(-1, 3)[4, 0], bad.reshape(-1, 3)[4, 2] = np.nan, -np.inf
    got = qerror.channel_sums(bad, q, S_Y, ZP)
    assert got['flag'].tolist() == [True, False, True]
    for k in ('n', 'n0', 'n255', 'syy', 'see', 'se', 'syh', 'shh', 'emax'):
        assert np.array_equal(got[k][[0, 2]], want[k][[0, 2]]), k
    assert got['n'].tolist() == [17, 18, 17]
    assert qerror.figures(got, S_Y)['non_finite']


def test_the_table_and_the_json_hold_every_layer():
    q = _codes((1, 4, 4, 3), seed=6)
    y = _exact(q)
    y[..., 0] += np.float32(0.5)
    f = qerror.figures(qerror.channel_sums(y, q, S_Y, ZP), S_Y, top=2)
    result = dict(images=1, layers={'conv1': dict(index=0, step=1, s_y=S_Y, zp_y=ZP, acc=f, local=f)})
    text = qerror.format_report(result)
    assert 'conv1' in text and 'reader' in text and text.count('\n') == 3
    doc = json.loads(qerror.to_json(result))
    assert doc['layers']['conv1']['acc']['worst'][0][0] == 0 and doc['layers']['conv1']['acc']['channel_sqnr_db'][1:] == ['inf', 'inf']
    assert 'sums' not in doc['layers']['conv1']['acc']
