"""optim.py, the statement of the learning-rate schedule, the weight average and the gradient clip, by hand-computed values;
the header's declarations; and the float32 restatements against float64 on the inputs tests/test_gpu_optim.py will hold the kernels to."""
import ctypes as C
import math

import numpy as np
import pytest

from k210_yolo_framework_amd import abi, optim
from k210_yolo_framework_amd.optim import EmaConfig, LrSchedule, clip_scale
from tests import optim_cases as oc
from tests import train_cases as tc


def test_warmup_and_cosine_by_hand():
    s = LrSchedule('cosine', 1e-3, 110, warmup_steps=10, final_frac=0.01)
    assert s.lr_at(0) == 1e-3 * 1 / 10                                       # the first warmup step
    assert s.lr_at(9) == 1e-3 * 10 / 10 == 1e-3                              # the last one runs at base
    assert s.lr_at(10) == 1e-3 * (0.01 + 0.99 * 0.5 * (1.0 + math.cos(0.0))) # cosine starts at base (cos 0 = 1: 0.01 + 0.99)
    assert s.lr_at(10) == pytest.approx(1e-3, rel=1e-15)
    assert s.lr_at(60) == pytest.approx(1e-3 * (0.01 + 0.99 * 0.5), rel=1e-12)      # the midpoint: cos(pi / 2) = 0
    assert s.lr_at(109) == pytest.approx(1e-3 * (0.01 + 0.99 * 0.5 * (1 + math.cos(math.pi * 99 / 100))), rel=1e-15)   # T - 1
    assert 1e-5 < s.lr_at(109) < 1.03e-5
    assert s.lr_at(110) == s.lr_at(111) == s.lr_at(10 ** 9) == 1e-3 * 0.01   # clamped from T on
    assert all(s.lr_at(k) > s.lr_at(k + 1) for k in range(10, 110))         # monotone after the warmup
    # no warmup, T - W = 0 guarded
    assert LrSchedule('cosine', 2.0, 1).lr_at(0) == 2.0 and LrSchedule('cosine', 2.0, 1, warmup_steps=1).lr_at(0) == 2.0


def test_step_schedule_on_each_side_of_both_milestones():
    s = LrSchedule('step', 1e-2, 100, warmup_steps=4)
    assert [s.lr_at(k) for k in (0, 3)] == [1e-2 * 1 / 4, 1e-2]
    assert s.lr_at(4) == s.lr_at(79) == 1e-2
    assert s.lr_at(80) == s.lr_at(89) == 1e-2 * 0.1
    assert s.lr_at(90) == s.lr_at(99) == s.lr_at(500) == 1e-2 * 0.1 ** 2
    t = LrSchedule('step', 1.0, 10, milestones=(0.5,), gamma=0.5)
    assert [t.lr_at(k) for k in (4, 5)] == [1.0, 0.5]


def test_constant_returns_base_lr_exactly():
    for base in (5e-4, 1e-3, 0.1, float(np.float32(5e-4))):
        s = LrSchedule('constant', base, 1000)
        assert all(s.lr_at(k) == base for k in (0, 1, 999, 1000, 12345))
    w = LrSchedule('constant', 3e-3, 1000, warmup_steps=3)
    assert [w.lr_at(k) for k in range(5)] == [3e-3 * 1 / 3, 3e-3 * 2 / 3, 3e-3 * 3 / 3, 3e-3, 3e-3]


def test_ema_decay_ramp():
    e = EmaConfig(0.9999, 2000.0)
    assert e.decay_at(1) == 0.9999 * (1.0 - math.exp(-1 / 2000.0)) and 4.99e-4 < e.decay_at(1) < 5.0e-4
    assert e.decay_at(2000) == pytest.approx(0.9999 * (1 - 1 / math.e), rel=1e-15)
    assert e.decay_at(10 ** 6) == 0.9999 and all(e.decay_at(k) < e.decay_at(k + 1) for k in (1, 10, 1000, 20000))
    assert EmaConfig(0.5, 0.0).decay_at(1) == EmaConfig(0.5, 0.0).decay_at(77) == 0.5           # tau = 0: no ramp
    assert EmaConfig(0.0).decay_at(5) == 0.0
    assert e.omd_at(1) == float(np.float32(1.0 - e.decay_at(1))) and np.float32(e.omd_at(10 ** 6)) == np.float32(1e-4)


def test_clip_scale_below_at_and_above_the_threshold():
    assert clip_scale(4.0, 10.0) == 1.0                                     # norm 2 below 10
    assert clip_scale(100.0, 10.0) == 10.0 / (10.0 + 1e-6) < 1.0            # at the threshold: the epsilon keeps it just below 1
    assert clip_scale(400.0, 10.0) == 10.0 / (20.0 + 1e-6)
    assert clip_scale(0.0, 10.0) == 1.0 and clip_scale(0.0, 0.0) == 0.0
    assert clip_scale(math.inf, 10.0) == 0.0 and clip_scale(math.nan, 10.0) == 1.0      # not special-cased: see the docstring
    assert 'propagated' in clip_scale.__doc__
    assert optim.clip_coefficient_f32(400.0, 10.0) == np.float32(10.0 / (20.0 + 1e-6))


def test_refusals():
    for bad in (dict(kind='linear'), dict(base_lr=0.0), dict(base_lr=math.nan), dict(total_steps=0), dict(warmup_steps=-1), dict(warmup_steps=11),
                dict(final_frac=1.5), dict(milestones=(0.9, 0.8)), dict(milestones=(1.5,)), dict(gamma=0.0)):
        kw = dict(kind='cosine', base_lr=1e-3, total_steps=10)
        kw.update(bad)
        with pytest.raises(ValueError, match='lr schedule'):
            LrSchedule(**kw)
    with pytest.raises(ValueError, match='negative'):
        LrSchedule('cosine', 1e-3, 10).lr_at(-1)
    for bad in (dict(decay=1.0), dict(decay=-0.1), dict(decay=math.nan), dict(tau=-1.0), dict(tau=math.nan)):
        with pytest.raises(ValueError, match='ema'):
            EmaConfig(**bad)
    with pytest.raises(ValueError, match='from 1'):
        EmaConfig().decay_at(0)


def test_optim_imports_no_torch():
    import subprocess
    import sys
    code = 'import sys; import k210_yolo_framework_amd.optim; sys.exit(int("torch" in sys.modules))'
    assert subprocess.run([sys.executable, '-c', code], cwd=str(oc.HEADER.parents[1])).returncode == 0


def test_header_declares_the_new_functions():
    sigs = abi.signatures(oc.HEADER.read_text())
    ptr, f, ll = abi.DevPtr, C.c_float, C.c_longlong
    assert sigs['yk_sumsq_workspace_bytes'] == (C.c_int, [ll, ptr])
    assert sigs['yk_sumsq_f32'] == (C.c_int, [ptr, ll, ptr, ptr, ptr])
    assert sigs['yk_adam_ex_f32'] == (C.c_int, [ll, ptr, ptr, ptr, ptr, ptr, ptr, f, f, ll, f, f, f, f, f, f, ptr])
    assert sigs['yk_ema_f32'] == (C.c_int, [ll, ptr, ptr, f, ptr])
    assert sigs['yk_adam_f32'] == (C.c_int, [ll, ptr, ptr, ptr, ptr, f, f, ll, f, f, f, f, ptr])       # untouched
    assert oc.SUMSQ_TILE == 4096 and oc.NS[-1] % oc.SUMSQ_TILE == 1 and oc.NS[:-1] == tc.ADAM_NS


def test_restatement_without_options_is_train_cases_adam_step():
    """The Adam statements in optim.py are train_cases.adam_step_f32's: on every ADAM_CASES problem the same bits."""
    for case in tc.ADAM_CASES:
        n, it, gs, dc, warm = case
        pr = tc.adam_problem(case)
        pn, mn, vn, e = optim.adam_ex_step_f32(pr['p'], pr['g'], pr['m'], pr['v'], tc.ADAM_LR, dc, it, tc.ADAM_B1, tc.ADAM_B2, tc.ADAM_EPS, gs)
        assert e is None
        for a, k in ((pn, 'p32'), (mn, 'm32'), (vn, 'v32')):
            assert np.array_equal(a.view(np.uint32), pr[k].view(np.uint32)), (case, k)


def test_float32_restatements_stay_inside_their_float64_bounds():
    """The yardsticks of tests/test_gpu_optim.py, checked before they are used there.
    EMA: against e + omd (src - e) in float64, within ema_bound (three roundings).  Clipping: the clipped gradient (g gs) c is two roundings
    from its float64 value, and Adam on that float32 gradient stays within train_cases.ScaledAdamRef's per-step bounds."""
    for n in oc.NS:
        pr = oc.ema_problem(n)
        for omd in (oc.OMD, oc.OMD_LATE, 0.0, 1.0):
            got = optim.ema_step_f32(pr['e'], pr['p32'], omd)
            err = np.abs(got.astype(np.float64) - oc.ema_f64(pr['e'], pr['p32'], omd))
            assert (err <= oc.ema_bound(pr['e'], pr['p32'], omd)).all(), (n, omd)
            same = pr['e'] == pr['p32']
            assert same[::5].all() and np.array_equal(got[same].view(np.uint32), pr['e'][same].view(np.uint32))      # p_new == e keeps its bits
        assert np.array_equal(optim.ema_step_f32(pr['e'], pr['p32'], 0.0).view(np.uint32), pr['e'].view(np.uint32))   # omd = 0 is a no-op
        gp = oc.gradient_problem(n)
        norm = math.sqrt(gp['sumsq'])
        for clip in (0.5 * norm, 4.0 * norm + 1.0, 1e-44):
            c = optim.clip_coefficient_f32(gp['sumsq'], clip)
            assert (c == 1.0) == (clip > norm + 1e-6)                       # (n = 1: the gradient is 1e-20, the epsilon decides)
            gi = (gp['g'] * np.float32(0.125)) * c
            exact = gp['g'].astype(np.float64) * 0.125 * float(c)
            assert (np.abs(gi - exact) <= 2 * tc.U * np.abs(exact) + 2 * tc.TINY).all()
            pn, mn, vn, _ = optim.adam_ex_step_f32(pr['p'], gp['g'], pr['m'], pr['v'], tc.ADAM_LR, 0.0, 9, tc.ADAM_B1, tc.ADAM_B2, tc.ADAM_EPS,
                                                   0.125, c=c)
            assert np.isfinite(pn).all() and np.isfinite(mn).all() and np.isfinite(vn).all()
            p64, m64, v64, (bp, bm, bv) = tc.ScaledAdamRef(9, 1.0, 0.0, pr['m'], pr['v']).step(pr['p'], gi)
            for got, ref, b, what in ((pn, p64, bp, 'p'), (mn, m64, bm, 'm'), (vn, v64, bv, 'v')):
                assert (np.abs(got.astype(np.float64) - ref) <= b).all(), (n, clip, what)
