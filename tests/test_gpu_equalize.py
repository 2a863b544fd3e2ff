"""The per-channel range kernel (yk_scale_act_chrange_f32, csrc/yk_calib.hip), Calibrator.feed_channels / channel_ranges and
save_kmodel(equalize=True) on the constructed network of tests/equalize_net.py."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, netspec as ns, quantize
from oracle import kpu_ref
from tests import equalize_net as en

pytestmark = pytest.mark.gpu

MS = (1, 7, 257, 4099)
ACTS = ((ns.ACT_RELU, 0.0), (ns.ACT_LEAKY, 0.1), (ns.ACT_NONE, 0.0))


class Dev:
    """One range buffer of n slots and the two kernels on torch's current stream."""

    def __init__(self, n):
        import torch
        from k210_yolo_framework_amd import engine
        engine.require_gpu()
        self.torch, self.engine, self.L, self.n = torch, engine, engine.lib(), n
        self.d = torch.zeros(4 * n, dtype=torch.int32, device='cuda')
        self.reset()

    def _s(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def reset(self):
        assert self.L.yk_range_reset(self.engine._ptr(self.d), self.n, self._s()) == 0

    def chrange(self, z, M, Cn, sc, bi, act, alpha, y, slot0):
        p = self.engine._ptr
        return self.L.yk_scale_act_chrange_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), act, C.c_float(alpha), p(y), p(self.d), slot0, self._s())

    def twin(self, z, M, Cn, sc, bi, act, alpha, y, slot):
        p = self.engine._ptr
        return self.L.yk_scale_act_range_f32(p(z), C.c_longlong(M), Cn, p(sc), p(bi), act, C.c_float(alpha), p(y), p(self.d), slot, self._s())

    def read(self):
        lo, hi, fl = np.empty(self.n, np.float32), np.empty(self.n, np.float32), np.empty(self.n, np.int32)
        self.torch.cuda.synchronize()
        assert self.L.yk_range_read(self.engine._ptr(self.d), self.n, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                    fl.ctypes.data_as(C.c_void_p)) == 0
        return lo, hi, fl


def _inputs(M, Cn, seed):
    import torch
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((M, Cn)) * 3 * np.exp(rng.uniform(-3, 3, Cn))).astype(np.float32)       # channel ranges over e^6
    sc = (rng.uniform(0.2, 2.0, Cn) * rng.choice([-1, 1], Cn)).astype(np.float32)
    bi = rng.standard_normal(Cn).astype(np.float32)
    pad = torch.zeros(M * Cn + 4, dtype=torch.float32, device='cuda')          # z again, one float off a 16-byte boundary
    pad[1:1 + M * Cn] = torch.from_numpy(z).cuda().reshape(-1)
    return torch.from_numpy(z).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(bi).cuda(), pad[1:1 + M * Cn]


@pytest.mark.parametrize('Cn', [1, 3, 5, 24, 64, 260, 1028])
def test_chrange_kernel_against_torch_and_its_twin(Cn):
    import torch
    S = 3 * Cn + 8                                                             # [0, Cn) one call, [Cn, 2 Cn) two halves, [2 Cn, 3 Cn) unaligned, then the twin
    D = Dev(S)
    for M in MS:
        z, sc, bi, z_off = _inputs(M, Cn, 1000 * Cn + M)
        assert z.data_ptr() % 16 == 0 and z_off.data_ptr() % 16 == 4
        for act, alpha in ACTS:
            D.reset()
            y0, y1, y2, y3 = (torch.full_like(z, 7.0) for _ in range(4))
            assert D.twin(z, M, Cn, sc, bi, act, alpha, y0, 3 * Cn) == 0
            assert D.chrange(z, M, Cn, sc, bi, act, alpha, y1, 0) == 0
            h = M // 2
            if h:
                assert D.chrange(z, h, Cn, sc, bi, act, alpha, y2, Cn) == 0
            assert D.chrange(z[h:], M - h, Cn, sc, bi, act, alpha, y2[h:], Cn) == 0
            assert D.chrange(z_off, M, Cn, sc, bi, act, alpha, y3, 2 * Cn) == 0
            lo, hi, fl = D.read()
            what = (Cn, M, act)
            assert torch.equal(y1, y0) and torch.equal(y2, y0) and torch.equal(y3, y0), what
            want_lo, want_hi = y0.amin(0).cpu().numpy(), y0.amax(0).cpu().numpy()
            for k in range(3):
                assert (lo[k * Cn:(k + 1) * Cn] == want_lo).all() and (hi[k * Cn:(k + 1) * Cn] == want_hi).all(), (what, k)
            assert lo[:Cn].min() == lo[3 * Cn] and hi[:Cn].max() == hi[3 * Cn], what
            assert not fl.any() and (lo[3 * Cn + 1:] == np.inf).all() and (hi[3 * Cn + 1:] == -np.inf).all(), what


@pytest.mark.parametrize('Cn,M', [(1, 257), (3, 7), (24, 4099), (260, 257), (1028, 7)])
def test_a_nan_and_an_inf_flag_their_channels_only_and_enter_no_range(Cn, M):
    import torch
    D = Dev(Cn + 2)
    z, sc, bi, _ = _inputs(M, Cn, 5 * Cn + M)
    c_nan, c_inf = Cn // 2, Cn - 1
    z[M // 3, c_nan] = float('nan')
    z[M - 1, c_inf] = float('inf')
    y = torch.empty_like(z)
    assert D.chrange(z, M, Cn, sc, bi, ns.ACT_NONE, 0.0, y, 1) == 0
    lo, hi, fl = D.read()
    assert sorted(np.flatnonzero(fl).tolist()) == sorted({1 + c_nan, 1 + c_inf})
    fin = torch.isfinite(y)
    assert int((~fin).sum()) == 2
    want_lo = torch.where(fin, y, torch.full_like(y, float('inf'))).amin(0).cpu().numpy()
    want_hi = torch.where(fin, y, torch.full_like(y, -float('inf'))).amax(0).cpu().numpy()
    assert (lo[1:1 + Cn] == want_lo).all() and (hi[1:1 + Cn] == want_hi).all()
    assert lo[0] == np.inf and lo[Cn + 1] == np.inf                             # the slots around them untouched


def test_bad_arguments_are_refused_by_name():
    import torch
    D = Dev(8)
    z = torch.zeros(16, dtype=torch.float32, device='cuda')
    ok = dict(z=z, M=4, Cn=4, sc=z, bi=z, act=0, alpha=0.0, y=torch.empty_like(z), slot0=0)
    assert D.chrange(**ok) == 0
    null = C.c_void_p(None)
    p = D.engine._ptr
    for bad in (dict(M=0), dict(M=-1), dict(Cn=0), dict(Cn=-4), dict(slot0=-1), dict(act=-1), dict(act=4),
                dict(M=1 << 62, Cn=4)):                                         # M * C past 2^63: the argument check, nothing launched
        rc = D.chrange(**{**ok, **bad})
        assert rc != 0 and b'yk_scale_act_chrange_f32' in D.L.yk_last_error(), bad
    for k in range(5):
        ptrs = [p(z), p(z), p(z), p(ok['y']), p(D.d)]
        ptrs[k] = null
        rc = D.L.yk_scale_act_chrange_f32(ptrs[0], C.c_longlong(4), 4, ptrs[1], ptrs[2], 0, C.c_float(0.0), ptrs[3], ptrs[4], 0, D._s())
        assert rc != 0 and b'yk_scale_act_chrange_f32' in D.L.yk_last_error(), k
    lo, hi, fl = D.read()
    assert (lo[:4] == 0).all() and (lo[4:] == np.inf).all()


# ---- the Calibrator ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    s, w, fr, T = en.case('float32')
    return s, w, fr.copy(), T                                                  # writable: torch.from_numpy wants that


def _np_channels(s, keeps):
    out = {}
    for op in s.ops:
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            v = np.concatenate([k[op['layer']].cpu().numpy().reshape(-1, op['cout']) for k in keeps])
            out[op['layer']] = (v.min(0), v.max(0))
    return out


def test_channel_ranges_equal_numpy_over_the_tensors_feed_keeps(net):
    import torch
    s, w, fr, T = net
    dev = torch.from_numpy(fr).cuda()
    cal = quantize.Calibrator(s, w, max_batch=8)
    keeps = []
    for a, b in ((0, 3), (3, 8)):
        keeps.append({})
        cal.feed(dev[a:b], keep=keeps[-1])
        cal.feed_channels(dev[a:b])
    got, want = cal.channel_ranges(), _np_channels(s, keeps)
    assert sorted(got) == sorted(want) == sorted(l.name for l in s.layers)
    for name in want:
        assert got[name][0].dtype == np.float32 and (got[name][0] == want[name][0]).all() and (got[name][1] == want[name][1]).all(), name
    per_tensor = cal.ranges()
    for name in want:                                                          # and the two buffers agree where they overlap
        assert (float(got[name][0].min()), float(got[name][1].max())) == per_tensor[name], name
    # the float64 forward of the helper, to the fp32 kernels' tolerance (tests/test_gpu_quantize.py: 1e-4 of the tensor's magnitude)
    ref = en.channel_ranges(s, T)
    for name in want:
        tol = 1e-4 * max(np.abs(ref[name][0]).max(), np.abs(ref[name][1]).max())
        assert np.abs(got[name][0] - ref[name][0]).max() <= tol and np.abs(got[name][1] - ref[name][1]).max() <= tol, name
    # how the frames are split: the reduction is exact, the GEMMs tile by batch size - the same tolerance
    one = quantize.calibrate_channels(s, w, fr, batch=8)
    for name in want:
        tol = 2e-4 * max(np.abs(ref[name][0]).max(), np.abs(ref[name][1]).max())
        assert np.abs(one[name][0] - got[name][0]).max() <= tol and np.abs(one[name][1] - got[name][1]).max() <= tol, name
    # the same batches in another order: bit for bit
    again = quantize.Calibrator(s, w, max_batch=8).feed_channels(dev[3:8]).feed_channels(dev[0:3]).channel_ranges()
    for name in want:
        assert again[name][0].tobytes() == got[name][0].tobytes() and again[name][1].tobytes() == got[name][1].tobytes(), name


def test_feed_and_ranges_do_not_see_feed_channels(net):
    import torch
    s, w, fr, T = net
    dev, other = torch.from_numpy(fr).cuda(), torch.from_numpy(en.frames(4, 3)).cuda()
    plain = quantize.Calibrator(s, w, max_batch=8).feed(dev[:4]).feed(dev[4:])
    mixed = quantize.Calibrator(s, w, max_batch=8).feed(dev[:4]).feed_channels(other).feed(dev[4:]).feed_channels(other[:1])
    assert mixed.ranges() == plain.ranges() and mixed.images == plain.images == 8
    for a, b in zip(mixed.read(), plain.read()):
        assert a.tobytes() == b.tobytes()
    mixed.feed_hist(dev[:4]).feed_hist(dev[4:]).feed_channels(other)
    plain.feed_hist(dev[:4]).feed_hist(dev[4:])
    assert mixed.ranges('mse') == plain.ranges('mse')
    from k210_yolo_framework_amd import engine
    with pytest.raises(engine.YkError, match='feed_channels'):
        plain.channel_ranges()


def test_a_non_finite_channel_raises_naming_the_layer(net):
    import torch
    from k210_yolo_framework_amd import engine
    s, w, fr, T = net
    w = {k: v.copy() for k, v in w.items()}
    w['conv_pw_1_bn/beta'][3] = np.nan
    cal = quantize.Calibrator(s, w, max_batch=8).feed_channels(torch.from_numpy(fr).cuda())
    with pytest.raises(engine.YkError, match='non-finite.*conv_pw_1'):
        cal.channel_ranges()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _model(s, w):
    from k210_yolo_framework_amd import yolonet
    return yolonet.YoloModel(s, {'weights': {k: np.asarray(v, np.float32) for k, v in w.items()}}, False)


def _fp32_outputs(s, w, fr):
    import torch
    keep = {}
    quantize.Calibrator(s, w, max_batch=len(fr)).feed(torch.from_numpy(fr).cuda(), keep=keep)
    names = quantize.tensor_names(s)
    return [keep[names[t]].cpu().numpy().astype(np.float64) for t in s.outputs]


def _kpu_error(km, fr, F):
    """Relative RMS error of the file on engine.KpuPlan against F, after holding the plan to the CPU oracle bit for bit."""
    import torch
    from k210_yolo_framework_amd import engine
    with engine.KpuPlan(km, max_batch=len(fr)) as plan:
        plan.run_u8(torch.from_numpy(np.ascontiguousarray(fr)).cuda())
        torch.cuda.synchronize()
        outs = [o[:len(fr)].cpu().numpy() for o in plan.outputs()]
    for b in range(len(fr)):
        for o, want in zip(outs, kpu_ref.run(km, np.ascontiguousarray(fr[b].transpose(2, 0, 1)))):
            assert o[b].transpose(2, 0, 1).tobytes() == np.ascontiguousarray(want).tobytes()
    num = sum(((o.astype(np.float64) - f) ** 2).sum() for o, f in zip(outs, F))
    return float(np.sqrt(num / sum((f ** 2).sum() for f in F)))


def test_save_kmodel_equalised_runs_as_the_oracle_and_is_closer_to_the_fp32_network(net, tmp_path, monkeypatch):
    from k210_yolo_framework_amd import engine
    s, w, fr, T = net
    calls, real = [], engine.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(engine, 'call', counting)
    m = _model(s, w)
    before = {k: v.copy() for k, v in m.get_weights().items()}
    rep_off = m.save_kmodel(str(tmp_path / 'off.kmodel'), fr, batch=8, equalize=False)
    assert 'yk_scale_act_range_f32' in calls and 'yk_scale_act_chrange_f32' not in calls and 'equalize' not in rep_off
    n = len(calls)
    rep_on = m.save_kmodel(str(tmp_path / 'on.kmodel'), fr, batch=8, equalize=True, max_gain=64.0)
    convs = len(s.layers)
    assert calls[n:].count('yk_scale_act_chrange_f32') == convs and calls[n:].count('yk_scale_act_range_f32') == convs + 2   # its input + the usual pass
    monkeypatch.undo()
    assert rep_on['equalize']['layers']['conv_dw_2']['f_max'] > 1.0 and 'equalised (max_gain 64)' in quantize.format_report(rep_on)
    assert all(m.get_weights()[k].tobytes() == before[k].tobytes() for k in before)                 # the model's float weights are its own
    # off is off: the bytes of the three calls made directly
    km, _ = quantize.quantize(s, m.get_weights(), quantize.calibrate(s, m.get_weights(), fr, 8))
    kmodel.write(str(tmp_path / 'direct.kmodel'), km)
    assert (tmp_path / 'off.kmodel').read_bytes() == (tmp_path / 'direct.kmodel').read_bytes()
    assert (tmp_path / 'on.kmodel').read_bytes() != (tmp_path / 'off.kmodel').read_bytes()
    held = en.frames(8, 23)
    F = _fp32_outputs(s, m.get_weights(), held)
    e_off = _kpu_error(kmodel.parse((tmp_path / 'off.kmodel').read_bytes()), held, F)
    e_on = _kpu_error(kmodel.parse((tmp_path / 'on.kmodel').read_bytes()), held, F)
    print(f'relative RMS error against the fp32 network on held-out frames: equalize=False {e_off:.6f}, equalize=True {e_on:.6f}')
    assert e_on < e_off
    with pytest.raises(engine.YkError, match='max_gain'):
        m.save_kmodel(str(tmp_path / 'no.kmodel'), fr, batch=8, equalize=True, max_gain=1.0)
    assert not (tmp_path / 'no.kmodel').exists()
