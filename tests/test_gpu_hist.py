"""Histogram kernels of csrc/yk_calib.hip (yk_hist_*, yk_scale_act_hist_f32) count for count against the numpy bin rule of
tests/calib_ref.py; quantize.Calibrator's second pass; and the saturating ends of a kmodel quantised from clipped ranges, bit for bit between
engine.KpuPlan and oracle/kpu_ref.py."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, netspec as ns, quantize
from oracle import kpu_ref
from tests import calib_ref

pytestmark = pytest.mark.gpu


class Hists:
    """n_slots histograms of nb bins on the device, and their flags."""

    def __init__(self, nb=2048, n=3):
        import torch
        from k210_yolo_framework_amd import engine
        engine.require_gpu()
        self.torch, self.engine, self.L, self.n, self.nb = torch, engine, engine.lib(), n, nb
        self.d = torch.zeros(n * nb, dtype=torch.int64, device='cuda')
        self.f = torch.zeros(n, dtype=torch.int32, device='cuda')

    def _s(self, stream=None):
        return C.c_void_p((stream or self.torch.cuda.current_stream()).cuda_stream)

    def add(self, x, lo, hi, slot, stream=None):
        """x: device fp32; the call's return code"""
        p = self.engine._ptr
        return self.L.yk_hist_f32(p(x), C.c_longlong(x.numel()), C.c_float(lo), C.c_float(calib_ref.inv_of(lo, hi, self.nb)), self.nb, p(self.d),
                                  p(self.f), slot, self._s(stream))

    def read(self):
        counts, fl = np.empty((self.n, self.nb), np.uint64), np.empty(self.n, np.int32)
        self.torch.cuda.synchronize()
        assert self.L.yk_hist_read(self.engine._ptr(self.d), self.engine._ptr(self.f), self.n, self.nb, counts.ctypes.data_as(C.c_void_p),
                                   fl.ctypes.data_as(C.c_void_p)) == 0
        return counts, fl


def _values(n, lo, hi, seed):
    """n finite float32 values over and beyond [lo, hi], with the values the bin rule could get wrong planted where they fit."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n).astype(np.float32)      # a tenth of them below lo or above hi
    special = np.array([lo, hi, -0.0, 0.0, 1e-45, -3e-42, 2e-39, np.nextafter(np.float32(hi), np.float32(-np.inf)),
                        np.nextafter(np.float32(lo), np.float32(np.inf)), 3e38, -3e38], np.float32)
    k = min(n, len(special))
    x[rng.permutation(n)[:k]] = special[:k]
    return x


@pytest.mark.parametrize('nb', [16, 2048, 4096])
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 2048 * 256 * 4 + 5])
def test_hist_kernel_equals_the_reference_count_for_count(n, nb):
    import torch
    lo, hi = np.float32(-1.75), np.float32(5.5)
    x = _values(n + 1, lo, hi, n + nb)
    if n > 11:
        den = x[np.abs(x) < np.finfo(np.float32).tiny]
        assert (den != 0).sum() >= 3 and (x == lo).any() and (x == hi).any() and (x < lo).any() and (x > hi).any()
    xd = torch.from_numpy(x).cuda()
    H = Hists(nb)
    assert H.add(xd[:n], lo, hi, 0) == 0                                       # 16-byte aligned: float4 loads + scalar tail
    assert H.add(xd[1:], lo, hi, 2) == 0                                       # offset by one float: the scalar path
    counts, fl = H.read()
    for slot, part in ((0, x[:n]), (2, x[1:])):
        want, bad = calib_ref.hist(part, lo, hi, nb)
        assert bad == 0 and counts[slot].sum() == n                            # every finite input counted once
        assert np.array_equal(counts[slot], want), (slot, np.nonzero(counts[slot] != want)[0][:8])
    assert not counts[1].any() and not fl.any()                                # an untouched slot


def test_denormals_decide_the_bin_in_a_range_of_denormal_width():
    """[0, 1e-37] in 16 bins: the bin width is below the smallest normal float32, so a flushed denormal would land in bin 0."""
    import torch
    lo, hi = np.float32(0), np.float32(1e-37)
    x = np.array([1e-38, 7e-39, 1.1e-38, 9.9e-38, 1e-37, 0.0, 1e-45, 5e-38], np.float32)
    want, _ = calib_ref.hist(x, lo, hi, 16)
    assert want[1] == 3 and want[0] == 2                                       # 1e-38, 7e-39, 1.1e-38 are denormal and belong to bin 1
    H = Hists(16)
    assert H.add(torch.from_numpy(x).cuda(), lo, hi, 0) == 0
    assert np.array_equal(H.read()[0][0], want)


def test_zero_width_range_puts_everything_in_bin_zero():
    import torch
    H = Hists(16)
    x = np.array([0.0, -0.0, 1.0, -2.5, 3e38, 1e-45], np.float32)
    assert calib_ref.inv_of(0.0, 0.0, 16) == 0
    assert H.add(torch.from_numpy(x).cuda(), np.float32(0), np.float32(0), 1) == 0
    counts, fl = H.read()
    assert counts[1, 0] == len(x) and counts[1].sum() == len(x) and not fl.any()
    assert np.array_equal(counts[1], calib_ref.hist(x, 0.0, 0.0, 16)[0])


@pytest.mark.parametrize('poison', [np.nan, np.inf, -np.inf])
def test_a_planted_nan_or_infinity_is_not_counted_and_flags_only_its_slot(poison):
    import torch
    H = Hists(2048)
    x = np.random.default_rng(3).standard_normal(100_000).astype(np.float32)
    lo, hi = calib_ref.widen(x.min(), x.max())
    clean = x.copy()
    x[77_777] = poison
    assert H.add(torch.from_numpy(x).cuda(), lo, hi, 1) == 0
    assert H.add(torch.from_numpy(clean).cuda(), lo, hi, 2) == 0
    counts, fl = H.read()
    assert fl.tolist() == [0, 1, 0]
    assert counts[1].sum() == len(x) - 1 and np.array_equal(counts[1], calib_ref.hist(x, lo, hi, 2048)[0])
    assert np.array_equal(counts[2], calib_ref.hist(clean, lo, hi, 2048)[0])
    assert H.add(torch.from_numpy(clean[:100]).cuda(), lo, hi, 1) == 0        # sticky
    assert H.read()[1].tolist() == [0, 1, 0]


@pytest.mark.parametrize('value', [0.0, 0.75])
def test_constant_tensor_is_one_bin(value):
    """65 536 equal values: every lane of every wave on one LDS address - the zero bin through the per-wave sum, any other bin through
    per-lane atomics."""
    import torch
    H = Hists(2048)
    x = torch.full((65_536,), value, dtype=torch.float32, device='cuda')
    assert H.add(x, np.float32(-1), np.float32(1), 0) == 0
    counts, _ = H.read()
    b = int(calib_ref.bins_of(np.float32([value]), np.float32(-1), calib_ref.inv_of(-1.0, 1.0, 2048), 2048)[0])
    assert counts[0, b] == 65_536 and counts[0].sum() == 65_536


def test_counts_are_64_bit():
    import torch
    H = Hists(16)
    H.d[16 + 5] = 2 ** 32 - 1                                                  # slot 1, bin 5, seeded on the device
    x = torch.full((1,), 5.5, dtype=torch.float32, device='cuda')              # [0, 16) in 16 bins: bin 5
    assert H.add(x, np.float32(0), np.float32(16), 1) == 0
    counts, _ = H.read()
    assert int(counts[1, 5]) == 2 ** 32 and counts[1].sum() == 2 ** 32


def test_a_length_one_workgroup_could_not_count_is_refused():
    """2048 workgroups at the most: n = 2^44 would put 2^33 elements into one workgroup's uint32 bins.  Refused before any launch."""
    import torch
    H = Hists(16)
    x = torch.zeros(4, dtype=torch.float32, device='cuda')
    p = H.engine._ptr
    rc = H.L.yk_hist_f32(p(x), C.c_longlong(1 << 44), C.c_float(0.0), C.c_float(1.0), 16, p(H.d), p(H.f), 0, H._s())
    assert rc != 0 and b'yk_hist_f32' in H.L.yk_last_error()
    for nb in (8, 15, 4097):                                                   # and the bin counts outside 16..4096
        assert H.L.yk_hist_f32(p(x), C.c_longlong(4), C.c_float(0.0), C.c_float(1.0), nb, p(H.d), p(H.f), 0, H._s()) != 0
    assert not H.read()[0].any()


def test_two_halves_on_two_streams_equal_one_call():
    import torch
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(300_001) * 2).astype(np.float32)
    lo, hi = calib_ref.widen(x.min(), x.max())
    xd = torch.from_numpy(x).cuda()
    H = Hists(2048)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        assert H.add(xd[:150_000], lo, hi, 0, s1) == 0
    with torch.cuda.stream(s2):
        assert H.add(xd[150_000:], lo, hi, 0, s2) == 0
    assert H.add(xd, lo, hi, 1) == 0
    counts, _ = H.read()
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[1], calib_ref.hist(x, lo, hi, 2048)[0])


def test_reset_clears_only_the_slots_it_is_told_to():
    import torch
    H = Hists(16, n=3)
    x = torch.from_numpy(np.linspace(0, 1, 1000, dtype=np.float32)).cuda()
    for slot in range(3):
        assert H.add(x, np.float32(0), np.float32(1), slot) == 0
    before, _ = H.read()
    assert H.L.yk_hist_reset(H.engine._ptr(H.d), 2, 16, H._s()) == 0           # slots 0 and 1
    after, _ = H.read()
    assert not after[:2].any() and np.array_equal(after[2], before[2]) and before[2].sum() == 1000


def _fused_reference(M, Cn, act, alpha):
    """z, scale, bias on the device and the y of yk_scale_act_range_f32 for them (computed once per shape and activation)."""
    import torch
    from k210_yolo_framework_amd import engine
    rng = np.random.default_rng(1000 * M + 10 * Cn + act)
    z = rng.standard_normal((M, Cn)).astype(np.float32) * 3
    sc = rng.uniform(0.2, 2.0, Cn).astype(np.float32) * rng.choice([-1, 1], Cn).astype(np.float32)
    bi = rng.standard_normal(Cn).astype(np.float32)
    zd, sd, bd = (torch.from_numpy(v).cuda() for v in (z, sc, bi))
    y0 = torch.empty_like(zd)
    rngd = torch.zeros(4, dtype=torch.int32, device='cuda')
    L, p, s = engine.lib(), engine._ptr, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.yk_range_reset(p(rngd), 1, s) == 0
    assert L.yk_scale_act_range_f32(p(zd), C.c_longlong(M), Cn, p(sd), p(bd), act, C.c_float(alpha), p(y0), p(rngd), 0, s) == 0
    return zd, sd, bd, y0


@pytest.mark.parametrize('act,alpha', [(0, 0.0), (1, 0.0), (2, 6.0), (3, 0.3)])
@pytest.mark.parametrize('M,Cn', [(1, 1), (7, 3), (5, 4), (257, 24), (1031, 20)])
def test_fused_kernel_writes_the_range_kernels_y_and_histograms_it(M, Cn, act, alpha):
    import torch
    zd, sd, bd, y0 = _fused_reference(M, Cn, act, alpha)
    want_y = y0.cpu().numpy()
    lo, hi = calib_ref.widen(want_y.min(), want_y.max())
    H = Hists(2048)
    p = H.engine._ptr
    y = torch.full_like(zd, float('nan'))
    assert H.L.yk_scale_act_hist_f32(p(zd), C.c_longlong(M), Cn, p(sd), p(bd), act, C.c_float(alpha), p(y), C.c_float(lo),
                                     C.c_float(calib_ref.inv_of(lo, hi, 2048)), 2048, p(H.d), p(H.f), 1, H._s()) == 0
    counts, fl = H.read()
    got_y = y.cpu().numpy()
    assert got_y.tobytes() == want_y.tobytes()                                 # bit for bit the y of yk_scale_act_range_f32
    assert np.array_equal(counts[1], calib_ref.hist(got_y, lo, hi, 2048)[0]) and counts[1].sum() == M * Cn
    assert not counts[0].any() and not counts[2].any() and not fl.any()


# ---- the Calibrator's second pass and the quantised file -------------------------------------------------------------------------------------
W_SEED, F_SEED = 7, 11


@pytest.fixture(scope='module')
def small():
    spec = ns.yolo_mobilev1((32, 32, 3), 3, 2, alpha=0.5)
    return spec, spec.init_weights(seed=W_SEED), quantize.synthetic_frames(3, spec.in_hw, seed=F_SEED)


@pytest.fixture(scope='module')
def fed(small):
    """A Calibrator that has seen the 3 frames in both passes, and every tensor of the second pass."""
    import torch
    spec, W, fr = small
    cal = quantize.Calibrator(spec, W, max_batch=3)
    frd = torch.from_numpy(fr).cuda()
    cal.feed(frd)
    keep = {}
    cal.feed_hist(frd, keep=keep)
    return cal, {k: v.cpu().numpy() for k, v in keep.items()}


def test_calibrator_histograms_equal_the_reference_of_the_kept_tensors(small, fed):
    spec, W, fr = small
    cal, keep = fed
    counts, lo, hi = cal.histograms()
    names = quantize.tensor_names(spec)
    assert counts.shape == (len(spec.tensors), 2048) and counts.dtype == np.uint64 and sorted(keep) == sorted(names)
    mm = cal.ranges()
    for i, name in enumerate(names):
        assert (lo[i], hi[i]) == calib_ref.widen(*mm[name]), name              # the bins span the first pass's range, widened to 0
        want, bad = calib_ref.hist(keep[name], lo[i], hi[i], 2048)
        assert bad == 0 and np.array_equal(counts[i], want), name
        assert counts[i].sum() == keep[name].size


def test_feeding_three_frames_equals_two_plus_one(small, fed):
    import torch
    spec, W, fr = small
    cal, _ = fed
    frd = torch.from_numpy(fr).cuda()
    two = quantize.Calibrator(spec, W, max_batch=3)
    two.feed(frd[:2]).feed(frd[2:])
    two.feed_hist(frd[:2]).feed_hist(frd[2:])
    a, b = cal.histograms(), two.histograms()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()       # the same bins ...
    differ = np.nonzero((a[0] != b[0]).any(axis=1))[0]
    print('tensors whose histograms differ:', [quantize.tensor_names(spec)[i] for i in differ])
    assert np.array_equal(a[0], b[0])                                          # ... and the same counts
    assert two.ranges('mse') == cal.ranges('mse')


def test_percentile_100_is_minmax_and_the_order_of_the_passes_is_enforced(small, fed):
    import torch
    from k210_yolo_framework_amd import engine
    spec, W, fr = small
    cal, _ = fed
    assert cal.ranges('percentile', 100) == cal.ranges() and cal.last_clip == []
    assert cal.ranges('minmax') == cal.ranges()
    plain = cal.ranges()
    clipped = cal.ranges('percentile', 90.0)
    moved = {r['tensor']: r for r in cal.last_clip}
    assert clipped['input'] == plain['input'] and 'input' not in moved         # the input stays the raw pixel
    assert 'conv_pw_1' in moved and set(moved) <= {l.name for l in spec.layers}
    for name, r in moved.items():                                              # at most a tenth of the values cut at either end
        assert (r['lo'], r['hi']) == plain[name] and (r['new_lo'], r['new_hi']) == clipped[name]
        assert r['lo'] <= r['new_lo'] <= 0.0 <= r['new_hi'] <= r['hi'] and 0.0 <= r['outside'] <= 0.2, r
    with pytest.raises(engine.YkError, match='unknown method'):
        cal.ranges('kl')
    fresh = quantize.Calibrator(spec, W, max_batch=3)
    with pytest.raises(engine.YkError, match='feed the ranges first'):
        fresh.feed_hist(torch.from_numpy(fr).cuda())
    fresh.feed(torch.from_numpy(fr).cuda())
    with pytest.raises(engine.YkError, match='feed_hist has seen 0 of the 3'):
        fresh.ranges('mse')


def test_a_non_finite_tensor_still_raises_naming_it(small):
    import torch
    from k210_yolo_framework_amd import engine
    spec, W, fr = small
    cal = quantize.Calibrator(spec, W, max_batch=3)
    frd = torch.from_numpy(fr).cuda()
    cal.feed(frd)
    cal.P['conv_pw_2/bias'][1] = float('nan')                                  # broken between the passes
    cal.feed_hist(frd)
    with pytest.raises(engine.YkError, match='conv_pw_2'):
        cal.histograms()
    with pytest.raises(engine.YkError, match='conv_pw_2'):
        cal.ranges('mse')


@pytest.mark.parametrize('method,pct', [('percentile', 90.0), ('mse', 99.99)])
def test_saturating_ends_are_bit_identical_between_the_gpu_and_the_oracle(small, method, pct):
    """Ranges clipped inside the calibration frames' own values: the frames reach the flat q = 0 end of the activation table and the KPU's
    clamp to 255, which min / max ranges never do."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, W, fr = small
    clipped = []
    ranges = quantize.calibrate(spec, W, fr, batch=3, method=method, percentile=pct, clipped=clipped)
    km, rep = quantize.quantize(spec, W, ranges)
    assert clipped and (rep['layers']['conv1']['s_x'], rep['layers']['conv1']['zp_x']) == (quantize.INPUT_SCALE, 0)      # the raw pixel
    km = kmodel.parse(kmodel.serialise(km))
    chw = np.ascontiguousarray(fr.transpose(0, 3, 1, 2))
    refs, keeps = [], []
    for img in chw:                                                            # the oracle first: the condition on the inputs
        keep = {}
        refs.append(kpu_ref.run(km, img, keep))
        keeps.append(keep)
    both = sorted({k for keep in keeps for k, v in keep.items() if (v == 0).any() and (v == 255).any()})
    print(method, 'conv layers holding codes 0 and 255:', both)
    assert both
    with engine.KpuPlan(km, max_batch=3) as plan:
        plan.run_u8(torch.from_numpy(chw).cuda(), layout='chw')
        torch.cuda.synchronize()
        for b, (keep, ref) in enumerate(zip(keeps, refs)):
            for index, want in keep.items():
                assert plan.read_layer(index, b).tobytes() == want.tobytes(), (b, index)
            for o, want in zip(plan.outputs(), ref):
                assert o[b].cpu().numpy().transpose(2, 0, 1).tobytes() == np.ascontiguousarray(want).tobytes(), b


def test_cli_round_trip_with_mse(tmp_path, capsys, monkeypatch):
    from pathlib import Path
    from k210_yolo_framework_amd import make_kmodel, yolonet
    monkeypatch.chdir(Path(__file__).resolve().parent.parent)
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--image_size', '32', '32', '--output_size', '1', '1', '2', '2',
           '--class_num', '2']
    model, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 2, alpha=0.5)
    model.set_weights(model.spec.init_weights(seed=W_SEED))
    ck = tmp_path / 'w.npz'
    model.save_weights(str(ck))
    out = tmp_path / 'mse.kmodel'
    rep = make_kmodel.cli([str(ck), str(out), '--synthetic', '4', '--calib_method', 'mse'] + net)
    text = capsys.readouterr().out
    assert out.exists() and rep['clipped'] and 'clipped conv' in text and 'mse ranges from 2048-bin histograms' in text
    plain = tmp_path / 'minmax.kmodel'
    make_kmodel.cli([str(ck), str(plain), '--synthetic', '4'] + net)
    assert 'clipped' not in capsys.readouterr().out and plain.read_bytes() != out.read_bytes()
    fresh, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 2, alpha=0.5, precision='kpu')
    fresh.load_weights(str(out))
    got = fresh.predict(quantize.synthetic_frames(2, (32, 32), seed=1))
    assert [g.shape for g in got] == [(2, 1, 1, 21), (2, 2, 2, 21)] and all(np.isfinite(g).all() for g in got)
