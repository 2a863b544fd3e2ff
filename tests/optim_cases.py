"""Inputs, references and bounds shared by tests/test_optim.py (CPU: the yardsticks themselves) and tests/test_gpu_optim.py (the kernels of
csrc/yk_optim.hip and the Trainer).  Built once, read-only."""
import functools
import math
import re
from pathlib import Path

import numpy as np

from k210_yolo_framework_amd import optim
from tests import train_cases as tc

HEADER = Path(__file__).resolve().parents[1] / 'include' / 'yolo_hip.h'
SUMSQ_TILE = int(re.search(r'#define\s+YK_SUMSQ_TILE\s+(\d+)', HEADER.read_text()).group(1))
# train_cases.ADAM_NS and one length one past a whole number of yk_sumsq_f32 tiles (three workgroups, the last with one element)
NS = list(tc.ADAM_NS) + [2 * SUMSQ_TILE + 1]
OMD = optim.EmaConfig(0.9999, 2000.0).omd_at(3)              # an ema_omd a run really passes: 1 - 0.9999 (1 - exp(-3 / 2000)), close to 1
OMD_LATE = optim.EmaConfig(0.9999, 2000.0).omd_at(10 ** 6)   # ... and the steady state, 1e-4


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def sumsq_problem(n):
    """train_cases.adam_gradients (normal x 10^{-4..1}, exact zeros, +-1e-20 whose square is subnormal in float32) with a few +-1e25 (whose
    square overflows float32); the reference is math.fsum of the squares, which are exact in float64."""
    rng = np.random.default_rng(1000 + n)
    x = tc.adam_gradients(rng, n)
    k = min(n // 8, 4)
    if k:
        x[rng.choice(n, k, replace=False)] = np.where(np.arange(k) % 2, -1e25, 1e25).astype(np.float32)
    sq = x.astype(np.float64) ** 2
    return _freeze(dict(x=x, ref=math.fsum(sq.tolist())))


def sumsq_bound(n, ref):
    """What reordering a float64 sum of n non-negative terms can move it (train_cases.colsum_bound's second term; the squares are exact)."""
    return n * 2.0 ** -53 * ref


@functools.lru_cache(maxsize=None)
def gradient_problem(n):
    """Plain gradients for the clipping tests (no 1e25: the norm is that of a training step's bucket)."""
    rng = np.random.default_rng(2000 + n)
    g = tc.adam_gradients(rng, n)
    return _freeze(dict(g=g, sumsq=math.fsum((g.astype(np.float64) ** 2).tolist())))


@functools.lru_cache(maxsize=None)
def ema_problem(n):
    """An Adam problem (warm state, the last train_cases case of this length or a fresh one) with an average e: p_old plus a perturbation,
    except every fifth element, which already equals the p the update will produce (there the average must keep its bits)."""
    case = (n, 9, 1.0, 0.0, True)
    rng = np.random.default_rng(3000 + n)
    p, m, v = tc.adam_state(rng, n, True)
    g = tc.adam_gradients(rng, n)
    pn, mn, vn = tc.adam_step_f32(p, g, m, v, 9, 1.0, 0.0)
    e = (p + rng.normal(size=n).astype(np.float32) * np.float32(1e-2)).astype(np.float32)
    e[::5] = pn[::5]
    return _freeze(dict(case=case, p=p, g=g, m=m, v=v, e=e, p32=pn, m32=mn, v32=vn))


def ema_f64(e, src, omd):
    e, src = np.asarray(e, np.float64), np.asarray(src, np.float64)
    return e + float(np.float32(omd)) * (src - e)


def ema_bound(e, src, omd):
    """Three roundings: the difference and the product carry theirs into the term omd (src - e), the sum rounds once more; a subnormal
    product is off by up to TINY whatever its size."""
    t = np.abs(float(np.float32(omd)) * (np.asarray(src, np.float64) - np.asarray(e, np.float64)))
    return tc.U * np.abs(ema_f64(e, src, omd)) + 3 * tc.U * t + 2 * tc.TINY
