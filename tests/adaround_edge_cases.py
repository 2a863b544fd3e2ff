"""Inputs of the kernels of csrc/yk_adaround.hip that the cases of tests/test_gpu_yolo_adaround.py do not reach, shared by
tests/test_adaround_edge_cases.py (CPU: every claim a case makes, from the constants of include/yolo_hip.h; the summation bound against damaged
references) and tests/test_gpu_yolo_adaround_edges.py (the kernels).  numpy only; the step kernel's own inputs are adaround_cases.step_edge_case.

yk_dw3x3_gram_f32 runs a grid of (chunks of rows) x (groups of 64 channels) and leaves partial [chunk][45][C]; no case so far had two chunks
and two groups at once, so the chunk stride 45 * C was never multiplied by a chunk index above 0 with a channel above 63."""
import re
from pathlib import Path

import numpy as np

from tests import biascorrect_cases as bc

HEADER = Path(__file__).resolve().parents[1] / 'include' / 'yolo_hip.h'
U64 = 2.0 ** -53

# (C, B, H, W, stride, pad_t, pad_l, pad_b, pad_r), the format of tests/test_gpu_yolo_adaround.py::GRAM_CASES, and what each is here for:
# chunks of rows, groups of channels, the rows of the last chunk (1 .. 3: row lanes idle while their LDS fold runs), rows per chunk above
# YK_DWGRAM_ROWS, and for stride 2 whether the bottom / right padding is read
GRAM_EDGES = [
    ((65, 1, 9, 9, 1, 1, 1, 1, 1), dict(M=81, chunks=2, groups=2, last=17, grown=False)),
    ((129, 1, 5, 13, 1, 1, 1, 1, 1), dict(M=65, chunks=2, groups=3, last=1, grown=False)),
    ((128, 2, 11, 6, 1, 1, 1, 1, 1), dict(M=132, chunks=3, groups=2, last=4, grown=False)),
    ((68, 3, 9, 11, 2, 1, 1, 1, 1), dict(M=90, chunks=2, groups=2, last=26, grown=False, pad_read=True)),
    ((68, 4, 9, 11, 2, 0, 0, 1, 1), dict(M=80, chunks=2, groups=2, last=16, grown=False, pad_read=False)),
    ((65, 1, 129, 128, 1, 1, 1, 1, 1), dict(M=16512, chunks=255, groups=2, last=2, grown=True)),
]
GRAM_IDS = ['C{}_B{}_{}x{}_s{}_p{}{}{}{}'.format(*c) for c, _ in GRAM_EDGES]

# (Co, K) of yk_adaround_rowerr_f64: the last partial stride of 256 threads, exactly one and two strides, more rows than one 16-bit grid dimension
ROWERR_EDGES = [(1, 255), (1, 256), (2, 512), (70000, 3)]


def define(name):
    return int(re.search(rf'#define {name} (\d+)', HEADER.read_text()).group(1))


def out_hw(case):
    Cn, B, H, W, stride, pt, pl, pb, pr = case
    return (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1


def gram_split(M):
    """gram_split of csrc/yk_adaround.hip restated: (rows per chunk, chunks)."""
    rows, most = define('YK_DWGRAM_ROWS'), define('YK_DWGRAM_MAX_CHUNKS')
    rpc = max(-(-M // most), rows)
    return rpc, -(-M // rpc)


def gram_inputs(case):
    """The two batches of a case, float32 [B][H][W][C]."""
    Cn, B, H, W = case[:4]
    rng = np.random.default_rng(Cn * 1000 + B * 100 + H)
    return [rng.normal(0.0, 1.0, (B, H, W, Cn)).astype(np.float32) for _ in range(2)]


def taps(x, stride, pt, pl, pb, pr):
    """float64 [9][M][C]: tap t of output position m = (b * Ho + oy) * Wo + ox, 0 outside the image."""
    return np.stack([w.reshape(-1, x.shape[3]) for w in bc._windows(np.asarray(x, np.float64), 3, stride, pt, pl, pb, pr)])


def gram_of_rows(win, rows):
    """float64 [C][9][9] over the output positions `rows` of taps()."""
    w = win[:, rows]
    return np.einsum('imc,jmc->cij', w, w)


def gram_in_kernel_order(win, rpc):
    """The sums in the order dw_gram_kernel and dw_gram_finish_kernel take them, in float64: per chunk the four row lanes (rows m0 + lane,
    m0 + lane + 4, ... ascending) folded 0, 1, 2, 3; then the chunks ascending."""
    M = win.shape[1]
    prod = np.einsum('imc,jmc->mcij', win, win)
    total = np.zeros(prod.shape[1:])
    for m0 in range(0, M, rpc):
        lanes = []
        for lane in range(4):
            acc = np.zeros(prod.shape[1:])
            for m in range(m0 + lane, min(m0 + rpc, M), 4):
                acc = acc + prod[m]
            lanes.append(acc)
        total = total + (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    return total


def within_bound(got, want, ab, n):
    """The assertion of test_dw_gram_against_float64_two_batches_accumulated_and_equal_bits: |G - want| <= n 2^-53 sum |x_i x_j| per entry."""
    return bool((np.abs(got - want) <= n * U64 * ab).all())


def rowerr_inputs(Co, K):
    rng = np.random.default_rng(1000 * K + Co)
    return rng.normal(0.0, 1.0, (Co, K)).astype(np.float32), rng.normal(0.0, 1.0, (Co, K)).astype(np.float32)
