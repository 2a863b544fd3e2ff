"""Independent reference for the clipped calibration: the histogram bin rule of csrc/yk_calib.hip restated in numpy, and
the two clipping rules of quantize.clip_range as brute-force loops over every candidate.  Shares no code with the package: the uint8 code
(scale, integer zero point, range widened to contain 0) is restated here too."""
import math

import numpy as np


# ---- the bin rule: float32 subtract, float32 multiply, truncate, clamp --------------------------------------------------------------------
def widen(lo, hi):
    """The float32 ends of a tensor's bins: its range widened to contain 0."""
    return np.minimum(np.float32(lo), np.float32(0)), np.maximum(np.float32(hi), np.float32(0))


def inv_of(lo, hi, nb):
    """nb / (hi - lo) in float64, rounded to float32 once; 0 for a zero-width range."""
    width = float(np.float32(hi)) - float(np.float32(lo))
    with np.errstate(over='ignore'):
        return np.float32(nb / width) if width > 0 else np.float32(0)


def bins_of(x, lo, inv, nb):
    x = np.ascontiguousarray(x, np.float32).ravel()
    with np.errstate(over='ignore', invalid='ignore'):
        d = x - np.float32(lo)                                                 # float32, rounded once
        t = d * np.float32(inv)                                                # float32, rounded once: no fused multiply-add
        assert d.dtype == np.float32 and t.dtype == np.float32
        t = np.where(np.isnan(t), np.float32(0), t)                            # 0 * inf of a degenerate range: bin 0
        b = np.clip(np.trunc(t.astype(np.float64)), 0, nb - 1)                 # truncate, then clamp (infinities clamp too)
    return b.astype(np.int64)


def hist(x, lo, hi, nb):
    """(counts uint64 [nb], number of non-finite values) of x over nb equal bins of [lo, hi]."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    fin = np.isfinite(x)
    b = bins_of(x[fin], lo, inv_of(lo, hi, nb), nb)
    return np.bincount(b, minlength=nb).astype(np.uint64), int((~fin).sum())


# ---- the clipping rules, by exhaustive search --------------------------------------------------------------------------------------------
def code(a, d):
    """(scale, zero point) of the asymmetric uint8 code over [a, d] widened to contain 0."""
    a, d = min(float(a), 0.0), max(float(d), 0.0)
    if d == a:
        return 1.0 / 255.0, 0
    s = (d - a) / 255.0
    return s, int(min(255, max(0, round(-a / s))))


def edge(lo, hi, nb, b):
    return lo if b == 0 else hi if b == nb else lo + b * ((hi - lo) / nb)


def err(counts, lo, hi, a, d):
    """sum_b counts[b] (m_b - x^(m_b))^2, exactly rounded (fsum)."""
    nb = len(counts)
    s, zp = code(a, d)
    terms = []
    for b in range(nb):
        if counts[b]:
            m = lo + (b + 0.5) * ((hi - lo) / nb)
            q = min(255.0, max(0.0, float(round(m / s)) + zp))                 # round(): half to even, as rint
            terms.append(float(counts[b]) * (m - s * (q - zp)) ** 2)
    return math.fsum(terms)


def clip(counts, lo, hi, method, percentile=99.99):
    counts = [int(c) for c in counts]
    lo, hi, nb, total = float(lo), float(hi), len(counts), sum(counts)
    if method == 'minmax' or hi == lo or total == 0 or (method == 'percentile' and percentile == 100):
        return lo, hi
    if method == 'percentile':
        k = math.floor((1.0 - percentile / 100.0) * total)
        j = next(j for j in range(nb) if sum(counts[j + 1:]) <= k)
        i = max(i for i in range(nb) if sum(counts[:i]) <= k)
        return min(edge(lo, hi, nb, i), 0.0), max(edge(lo, hi, nb, j + 1), 0.0)
    assert method == 'mse'
    best, d_star = None, None
    for j in range(1, nb + 1):
        e = err(counts, lo, hi, lo, edge(lo, hi, nb, j))
        if best is None or e <= best:                                          # a tie: the larger d
            best, d_star = e, edge(lo, hi, nb, j)
    best, a_star = None, None
    for i in range(nb):
        if edge(lo, hi, nb, i) <= 0.0:
            e = err(counts, lo, hi, edge(lo, hi, nb, i), d_star)
            if best is None or e < best:                                       # a tie: the smaller a
                best, a_star = e, edge(lo, hi, nb, i)
    return a_star, d_star
