"""quantize.clip_range (host, float64, from integer histograms) against the brute-force reference of tests/calib_ref.py, its fixed points
and edge cases, the calibration flags of the make_kmodel CLI and the report lines.  No GPU."""
import math

import numpy as np
import pytest

from k210_yolo_framework_amd import quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from tests import calib_ref


def _random_hist(nb, signed, seed, tails=False):
    """(counts uint64 [nb], lo, hi): the histogram, by the reference bin rule, of a skewed sample with a few far values.  `tails`: the range
    reaches well past the data at both ends, so the end bins are empty."""
    rng = np.random.default_rng(seed)
    n = 300 if nb == 16 else 4000
    x = rng.standard_normal(n).astype(np.float32) * np.float32(rng.uniform(0.2, 3.0))
    x[rng.integers(0, n, 3)] *= np.float32(rng.uniform(4, 30))                 # outliers
    if not signed:
        x = np.maximum(x, np.float32(0))                                       # post-ReLU: half the mass is exactly 0
    lo, hi = calib_ref.widen(x.min(), x.max())
    if tails:
        lo, hi = (np.float32(lo * 20 - 1) if signed else lo), np.float32(hi * 20 + 1)
    counts, bad = calib_ref.hist(x, lo, hi, nb)
    assert bad == 0 and counts.sum() == n
    return counts, float(lo), float(hi)


CASES = [(nb, signed, tails) for nb in (16, 2048) for signed in (True, False) for tails in (False, True)]


@pytest.mark.parametrize('nb,signed,tails', CASES)
def test_clip_range_equals_the_brute_force_reference(nb, signed, tails):
    for seed in range(6 if nb == 16 else 1):
        counts, lo, hi = _random_hist(nb, signed, 100 * nb + seed, tails)
        if tails:
            assert counts[-1] == 0 and (not signed or counts[0] == 0)
        for pct in (99.99, 99.0, 90.0, 60.0):
            got = quantize.clip_range(counts, lo, hi, 'percentile', pct)
            want = calib_ref.clip(counts, lo, hi, 'percentile', pct)
            assert got == want, (seed, pct, got, want)
            assert lo <= got[0] <= 0.0 <= got[1] <= hi                         # contains 0, inside [lo, hi]
        got = quantize.clip_range(counts, lo, hi, 'mse')
        want = calib_ref.clip(counts, lo, hi, 'mse')
        print(nb, signed, tails, seed, (lo, hi), '->', got)
        assert got == want, (seed, got, want)
        assert lo <= got[0] <= got[1] <= hi
        e_new, e_old = quantize.clip_error(counts, lo, hi, *got), quantize.clip_error(counts, lo, hi, lo, hi)
        assert e_new <= e_old
        assert math.isclose(e_new, calib_ref.err(counts, lo, hi, *got), rel_tol=1e-12)
        assert math.isclose(e_old, calib_ref.err(counts, lo, hi, lo, hi), rel_tol=1e-12)


@pytest.mark.parametrize('nb,signed,tails', CASES)
def test_percentile_100_and_minmax_return_the_range_exactly(nb, signed, tails):
    counts, lo, hi = _random_hist(nb, signed, 7, tails)
    assert quantize.clip_range(counts, lo, hi, 'percentile', 100) == (lo, hi)
    assert quantize.clip_range(counts, lo, hi, 'percentile', 100.0) == (lo, hi)
    assert quantize.clip_range(counts, lo, hi, 'minmax') == (lo, hi)
    assert quantize.clip_range(None, lo, hi, 'minmax') == (lo, hi)             # needs no histogram


def _gauss_with_outlier(nb, n, sigma=1.0):
    """Counts of round(n * P(bin)) values of max(N(0, sigma^2), 0) - a post-ReLU tensor - plus ONE value at 100 sigma, over [0, 100 sigma]:
    built from the normal distribution function, no sampling."""
    lo, hi = 0.0, 100.0 * sigma
    cdf = lambda v: 0.5 * (1.0 + math.erf(v / (sigma * math.sqrt(2.0))))       # noqa: E731
    e = [lo + b * (hi - lo) / nb for b in range(nb + 1)]
    counts = np.array([round(n * (cdf(e[b + 1]) - (cdf(e[b]) if b else 0.0))) for b in range(nb)], np.uint64)
    body = int(counts.sum())
    top = int(np.nonzero(counts)[0][-1])                                       # the last bin the Gaussian reaches
    counts[nb - 1] += np.uint64(1)                                             # 100 sigma = hi: the last bin
    return counts, lo, hi, body, top


def test_mse_clips_a_gaussian_with_one_value_at_100_sigma():
    """Why 4 million values: clipping the one outlier to d costs (100 - d)^2, and spreading the codes over [0, d] instead of [0, 100]
    saves about n_pos (100^2 - d^2) / (12 * 255^2) of rounding noise over the n_pos = n / 2 positive values (the zeros are exact).  At
    d = 25 sigma that is 5625 against 0.006 n: the rule can only prefer hi' < hi / 4 for n well above a million."""
    counts, lo, hi, body, top = _gauss_with_outlier(2048, 4_000_000)
    a, d = quantize.clip_range(counts, lo, hi, 'mse')
    e_new, e_old = quantize.clip_error(counts, lo, hi, a, d), quantize.clip_error(counts, lo, hi, lo, hi)
    print(f'mse: ({lo}, {hi}) -> ({a}, {d}); err {e_old:.6g} -> {e_new:.6g}')
    assert a == 0.0 and d < hi / 4
    assert e_new < e_old
    assert (a, d) == calib_ref.clip(counts, lo, hi, 'mse')


def test_percentile_99_9_drops_exactly_the_one_outlier():
    """1500 values: k = floor(0.001 * 1501) = 1 value may go at either end.  The upper end gives up the outlier alone; the lower end stays,
    because bin 0 holds the zeros."""
    counts, lo, hi, body, top = _gauss_with_outlier(2048, 1500)
    assert math.floor((1.0 - 99.9 / 100.0) * (body + 1)) == 1 and counts[0] > 1
    a, d = quantize.clip_range(counts, lo, hi, 'percentile', 99.9)
    w = (hi - lo) / 2048
    assert a == 0.0 and d == lo + (top + 1) * w                                # the upper edge of the last bin the Gaussian reaches
    assert quantize.outside_share(counts, lo, hi, a, d) == 1.0 / (body + 1)
    assert (a, d) == calib_ref.clip(counts, lo, hi, 'percentile', 99.9)


@pytest.mark.parametrize('method', ['minmax', 'percentile', 'mse'])
def test_zero_width_range_and_empty_histogram(method):
    counts = np.zeros(16, np.uint64)
    counts[0] = 1000                                                           # hi == lo: everything is in bin 0
    assert quantize.clip_range(counts, 0.0, 0.0, method) == (0.0, 0.0)
    assert calib_ref.clip(counts, 0.0, 0.0, method) == (0.0, 0.0)
    assert quantize.hist_inv(0.0, 0.0, 16) == 0.0 and calib_ref.inv_of(0.0, 0.0, 16) == 0.0
    assert quantize.clip_range(np.zeros(16, np.uint64), -1.0, 2.0, method) == (-1.0, 2.0)
    assert quantize.qparams(*quantize.clip_range(counts, 0.0, 0.0, method)) == (quantize.INPUT_SCALE, 0)


def test_hist_inv_is_the_references():
    for lo, hi, nb in ((0.0, 1.0, 2048), (-3.7, 11.25, 16), (-1e-3, 0.0, 4096), (0.0, 1e-37, 16), (-3e38, 3e38, 2048), (0.0, 1e-42, 2048)):
        lo, hi = np.float32(lo), np.float32(hi)
        got, want = quantize.hist_inv(lo, hi, nb), calib_ref.inv_of(lo, hi, nb)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (lo, hi, nb)


def test_bad_arguments_are_refused():
    counts, lo, hi = _random_hist(16, True, 1)
    with pytest.raises(KmodelError, match='unknown method'):
        quantize.clip_range(counts, lo, hi, 'kl')
    for pct in (50.0, 0.0, 100.5, -1.0):
        with pytest.raises(KmodelError, match='percentile'):
            quantize.clip_range(counts, lo, hi, 'percentile', pct)
    with pytest.raises(KmodelError, match='contain 0'):
        quantize.clip_range(counts, 0.5, hi, 'mse')
    with pytest.raises(KmodelError, match='counts'):
        quantize.clip_range(counts[:8], lo, hi, 'mse')


@pytest.mark.parametrize('flags,message', [
    (['--synthetic', '4', '--calib_method', 'kl'], 'calib_method'),
    (['--synthetic', '4', '--calib_method', 'percentile', '--calib_percentile', '50'], 'calib_percentile'),
    (['--synthetic', '4', '--calib_method', 'percentile', '--calib_percentile', '100.01'], 'calib_percentile'),
    (['--synthetic', '4', '--calib_method', 'mse', '--calib_bins', '8'], 'calib_bins'),
    (['--synthetic', '4', '--calib_method', 'mse', '--calib_bins', '8192'], 'calib_bins'),
    (['--ranges', 'r.npz', '--calib_method', 'mse'], '--ranges'),
    (['--ranges', 'r.npz', '--calib_method', 'minmax'], '--ranges'),
])
def test_cli_refuses_before_it_reads_anything(flags, message, capsys):
    from k210_yolo_framework_amd import make_kmodel
    with pytest.raises(SystemExit) as e:
        make_kmodel.cli(['no_such_checkpoint.h5', 'out.kmodel'] + flags)
    assert e.value.code == 2                                                   # argparse's error exit
    assert message in capsys.readouterr().err


def test_format_report_prints_one_line_per_clipped_tensor():
    report = dict(layers={}, requant=[], main_mem_usage=1024, kpu_ram_peak=2048,
                  clipped=[dict(tensor='conv_pw_3', method='mse', lo=0.0, hi=41.5, new_lo=0.0, new_hi=9.25, outside=0.000125),
                           dict(tensor='head_conv_1', method='mse', lo=-7.5, hi=3.0, new_lo=-6.0, new_hi=3.0, outside=0.5)])
    text = quantize.format_report(report).splitlines()
    assert 'clipped conv_pw_3 (mse): (0, 41.5) -> (0, 9.25), 0.0125% of the calibration values outside' in text
    assert 'clipped head_conv_1 (mse): (-7.5, 3) -> (-6, 3), 50.0000% of the calibration values outside' in text
    report.pop('clipped')                                                      # a minmax report has none and prints as before
    assert not any(line.startswith('clipped') for line in quantize.format_report(report).splitlines())
