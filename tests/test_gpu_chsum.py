"""yk_scale_act_chsum_f32 (csrc/yk_calib.hip): the per-channel float64 sums of the pre-activation, beside the y of yk_scale_act_range_f32.

The bound: the kernel adds the M fp32 values t of a channel (exact in float64) in SOME order with M - 1 rounded additions (+ one exact addition
to the zeroed slot); any order of recursive float64 summation is within (M - 1) * 2^-53 * sum|t| of the exact sum (Rump 2012; no higher-order
term), and math.fsum is the correctly rounded exact sum.  No measured constant."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
# one pass of partials: the finishing launch walks a channel's partials with max(1, 256 // min(C, 256)) accumulators, and a workgroup covers
# ceil(YK_CHSUM_TILE / C) rows (include/yolo_hip.h).  C = 4: 64 accumulators, 4096 rows per workgroup - more than 64 * 4096 = 262144 rows take
# a second pass.  (70000, 257) has 64 rows per workgroup and ONE accumulator for the first 256 channels: 1094 passes there already.
SHAPES = [(1, 1), (255, 3), (256, 4), (257, 5), (1000, 48), (70000, 257), (300001, 4)]


class Sums:
    def __init__(self, n):
        import torch
        from k210_yolo_framework_amd import engine
        engine.require_gpu()
        self.torch, self.engine, self.n = torch, engine, n
        self.sum = torch.zeros(n, dtype=torch.float64, device='cuda')
        self.flags = torch.zeros(n, dtype=torch.int32, device='cuda')
        self.work = {}
        engine.call('yk_chsum_reset', self.sum, self.flags, n, self.stream())

    def stream(self, s=None):
        return C.c_void_p((s or self.torch.cuda.current_stream()).cuda_stream)

    def run(self, z, scale, bias, act, alpha, y, slot0, s=None):
        M, Cn = z.shape
        need = C.c_size_t()
        self.engine.call('yk_chsum_workspace_bytes', M, Cn, C.byref(need))
        assert need.value == 8 * Cn * -(-M // -(-self.tile() // Cn))
        key = (need.value, s)
        if key not in self.work:
            self.work[key] = self.torch.empty(need.value // 8, dtype=self.torch.float64, device='cuda')
        self.engine.call('yk_scale_act_chsum_f32', z, M, Cn, scale, bias, act, float(alpha), y, self.sum, self.flags, slot0, self.work[key],
                         self.stream(s))

    @staticmethod
    def tile():
        import re
        from k210_yolo_framework_amd import engine
        return int(re.search(r'#define YK_CHSUM_TILE (\d+)', engine.HEADER_PATH.read_text()).group(1))

    def read(self):
        s, f = np.empty(self.n, np.float64), np.empty(self.n, np.int32)
        self.torch.cuda.synchronize()
        self.engine.call('yk_chsum_read', self.sum, self.flags, self.n, s, f)
        return s, f


def _inputs(M, Cn, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((M, Cn)) * 3).astype(np.float32)
    sc = (rng.uniform(0.2, 2.0, Cn) * rng.choice([-1, 1], Cn)).astype(np.float32)
    bi = rng.standard_normal(Cn).astype(np.float32)
    return z, sc, bi


def _pre(z, sc, bi):
    return (z * sc + bi).astype(np.float32)                # fp32, one rounding per operation


def _reference(t):
    """(math.fsum per channel, the bound (M - 1) 2^-53 sum|t| per channel)"""
    t64 = t.astype(np.float64)
    exact = np.array([math.fsum(col) for col in t64.T])
    return exact, (t.shape[0] - 1) * U * np.array([math.fsum(col) for col in np.abs(t64).T])


@functools.lru_cache(maxsize=None)
def _case(M, Cn):
    """Inputs and reference of a shape: computed once, shared by the activations, never changed."""
    z, sc, bi = _inputs(M, Cn, M * 31 + Cn)
    return (z, sc, bi) + _reference(_pre(z, sc, bi))


def _range_y(z, sc, bi, act, alpha):
    import torch
    from k210_yolo_framework_amd import engine
    r = torch.zeros(4, dtype=torch.int32, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    engine.call('yk_range_reset', r, 1, s)
    y = torch.empty_like(z)
    engine.call('yk_scale_act_range_f32', z, z.shape[0], z.shape[1], sc, bi, act, float(alpha), y, r, 0, s)
    return y


@pytest.mark.parametrize('M,Cn', SHAPES)
@pytest.mark.parametrize('act,alpha', [(0, 0.0), (1, 0.0), (3, 0.3)])
def test_sums_within_the_float64_bound_and_y_equal_to_the_range_kernels(M, Cn, act, alpha):
    import torch
    z, sc, bi, exact, bound = _case(M, Cn)
    S = Sums(2 * Cn + 3)
    zd, sd, bd = (torch.from_numpy(v).cuda() for v in (z, sc, bi))                # (copies: the shared inputs stay as they are)
    yd = torch.empty_like(zd)
    S.run(zd, sd, bd, act, alpha, yd, 2)
    # the scalar path: every pointer 4 bytes past a 16-byte boundary
    big = [torch.empty(v.numel() + 1, dtype=torch.float32, device='cuda') for v in (zd, sd, bd, zd)]
    zo, so, bo, yo = (b[1:].view(v.shape) for b, v in zip(big, (zd, sd, bd, zd)))
    zo.copy_(zd), so.copy_(sd), bo.copy_(bd)
    assert all(v.data_ptr() % 16 == 4 for v in (zo, so, bo, yo))
    S.run(zo, so, bo, act, alpha, yo, Cn + 3)
    want_y = _range_y(zd, sd, bd, act, alpha)
    s, f = S.read()
    assert torch.equal(yd, want_y) and torch.equal(yo, want_y)
    assert not f.any() and (s[:2] == 0).all() and s[Cn + 2] == 0
    for name, got in (('vector', s[2:Cn + 2]), ('scalar', s[Cn + 3:])):
        err = np.abs(got - exact)
        print(f'{name}: max |sum - fsum| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}')
        assert (err <= bound).all(), (name, err, bound)
    assert s[2:Cn + 2].tobytes() == s[Cn + 3:].tobytes()   # the order of the additions follows from (M, C) alone, not from the alignment


def test_two_streams_give_the_same_bits_and_batches_accumulate():
    import torch
    M, Cn = 5000, 48
    z, sc, bi = _inputs(M, Cn, 5)
    t = _pre(z, sc, bi)
    exact, bound = _reference(t)
    S = Sums(3 * Cn)
    zd, sd, bd = (torch.from_numpy(v).cuda() for v in (z, sc, bi))
    ys = [torch.empty_like(zd) for _ in range(3)]
    torch.cuda.synchronize()
    for k, st in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        with torch.cuda.stream(st):
            S.run(zd, sd, bd, 1, 0.0, ys[k], k * Cn, st)
    torch.cuda.synchronize()
    cut = 1777                                             # two batches of one set, into the third run of slots
    S.run(zd[:cut], sd, bd, 1, 0.0, ys[2][:cut], 2 * Cn)
    S.run(zd[cut:], sd, bd, 1, 0.0, ys[2][cut:], 2 * Cn)
    s, f = S.read()
    assert s[:Cn].tobytes() == s[Cn:2 * Cn].tobytes() and not f.any()
    assert (np.abs(s[:Cn] - exact) <= bound).all() and (np.abs(s[2 * Cn:] - exact) <= bound).all()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


@pytest.mark.parametrize('Cn,bad_c', [(48, 17), (5, 4)])
def test_a_planted_nan_flags_its_own_channel_only(Cn, bad_c):
    import torch
    M = 300
    z, sc, bi = _inputs(M, Cn, 9)
    z[123, bad_c] = np.nan
    z[7, bad_c] = np.inf
    t = _pre(z, sc, bi)
    S = Sums(Cn)
    zd, sd, bd = (torch.from_numpy(v).cuda() for v in (z, sc, bi))
    S.run(zd, sd, bd, 0, 0.0, torch.empty_like(zd), 0)
    s, f = S.read()
    assert f.tolist() == [int(c == bad_c) for c in range(Cn)]
    keep = np.isfinite(t[:, bad_c])
    t[~keep, bad_c] = 0                                    # not added
    exact, bound = _reference(t)
    assert (np.abs(s - exact) <= bound).all()
