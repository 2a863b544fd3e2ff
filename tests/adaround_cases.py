"""What tests/test_adaround.py (CPU) and tests/test_gpu_yolo_adaround.py (GPU) share: numpy float64 Gram matrices of the mini network of
tests/biascorrect_cases.py, the brute-force single rows, the inputs of the step kernel's test with their float32-against-float64 figure, and
the mini case both files optimise.  A helper, not a test."""
import functools
import itertools

import numpy as np

from k210_yolo_framework_amd import adaround, netspec as ns
from tests import biascorrect_cases as bc

MINI_ITERS, MINI_LAMBDA, MINI_LR = 200, 0.01, 1e-2


def dw_gram(x, stride, pt, pl, pb, pr):
    """float64 [C][9][9] of x [N][H][W][C]: sum over the output positions of tap_i tap_j, taps outside the image 0."""
    win = np.stack([w.reshape(-1, x.shape[3]) for w in bc._windows(np.asarray(x, np.float64), 3, stride, pt, pl, pb, pr)])     # [9][M][C]
    return np.einsum('imc,jmc->cij', win, win)


def dw_gram_abs(x, stride, pt, pl, pb, pr):
    """sum |tap_i tap_j|: what the summation bound multiplies."""
    return dw_gram(np.abs(np.asarray(x, np.float64)), stride, pt, pl, pb, pr)


def columns(x, k, stride, pt, pl, pb, pr):
    """[M][k * k * C] float64 in im2col order col = (ky * k + kx) * C + c."""
    win = bc._windows(np.asarray(x, np.float64), k, stride, pt, pl, pb, pr)
    return np.concatenate([w.reshape(-1, x.shape[3]) for w in win], axis=1)


def numpy_grams(spec, T):
    """{conv layer: float64 Gram matrix} from the float64 tensors T {tensor id: NHWC} of biascorrect_cases.float_means."""
    out = {}
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        pads = (op['pad_t'], op['pad_l'], op.get('pad_b', op['pad_t']), op.get('pad_r', op['pad_l']))
        x = T[op['in0']]
        if op['type'] == ns.OP_DWCONV:
            out[op['layer']] = dw_gram(x, op['stride'], *pads)
        else:
            col = columns(x, op['k'], op['stride'], *pads)
            out[op['layer']] = col.T @ col
    return out


@functools.lru_cache(maxsize=None)
def mini_case():
    """(spec, weights, frames, {layer: G float64}) of the mini network: built once per process and never changed."""
    spec, w, fr, fm, ranges = bc.mini_case()
    _, T = bc.float_means(spec, w, fr)
    return spec, w, fr, numpy_grams(spec, T)


@functools.lru_cache(maxsize=None)
def mini_optimised():
    """{layer: (codes [Co][K], entry)} of optimise_numpy on the mini case."""
    spec, w, fr, G = mini_case()
    out = {}
    for op in spec.ops:
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            name = op['layer']
            rows = adaround.rows_of(np.asarray(w[name + '/kernel'], np.float64), op['type'] == ns.OP_DWCONV)
            out[name] = adaround.optimise_numpy(rows, G[name], MINI_ITERS, MINI_LAMBDA, MINI_LR)
    return out


# ---- brute force: single rows whose every rounding can be tried --------------------------------------------------------------------------
BRUTE_SEEDS = tuple(range(12))


def brute_row(seed):
    """(rows [1][K], G [K][K] positive definite, free count): 6 .. 10 free weights besides an exact zero and the tensor's extreme whose down code is below 0."""
    rng = np.random.default_rng(1000 + seed)
    k_free = 6 + seed % 5
    row = rng.normal(0.0, 1.0, k_free + 2)
    row[0] = 0.0
    A = rng.normal(0.0, 1.0, (3 * len(row), len(row))) * rng.uniform(0.2, 3.0, len(row))
    A[:, 1:] += 0.8 * A[:, :-1]                                                 # correlated inputs: the off-diagonal of G is what nearest ignores
    return row[None, :], A.T @ A


def brute_force(rows, G):
    """(E of the best rounding, E(nearest)) over all 2^free roundings of the free weights, frozen ones at nearest."""
    st = adaround.prepare(rows, G)
    free = np.flatnonzero(~st['frozen'][0])
    base = np.clip(st['down'][0], 0, 255)
    best = np.inf
    for ups in itertools.product((0.0, 1.0), repeat=len(free)):
        codes = st['nearest'][0].astype(np.float64)
        codes[free] = base[free] + np.array(ups)
        best = min(best, float(adaround.row_errors(adaround.hard_error(codes[None, :], st), G)[0]))
    return best, float(st['e_nearest'][0]), len(free)


# ---- the step kernel's inputs -----------------------------------------------------------------------------------------------------------
STEP_SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 257), (3, 21), (3, 86))          # (Co, K): n = 1, 63, 64, 65, 257, 63, 258
STEP_MODES = {'warmup': (0.0, 20.0), 'beta20': (0.01, 20.0), 'fractional': (0.01, 11.37), 'beta2': (0.01, 2.0)}      # (lam_t, beta_t)
STEP_LR = 1e-2


def step_case(Co, K, seed=0):
    """dict of float64 inputs: V (with +-20 where h is clipped), r, frozen (some set where K allows), G [K][K], inv_e, s_w, n_free."""
    rng = np.random.default_rng(77 + 1000 * Co + K + seed)
    r = rng.uniform(0.02, 0.98, (Co, K))
    V = adaround.v_init(r) + rng.normal(0.0, 0.5, (Co, K))
    frozen = np.zeros((Co, K), bool)
    if K >= 3:
        frozen[:, 1::7] = True
        V[:, 2::11] = 20.0
        V[:, 5::13] = -20.0
    A = rng.normal(0.0, 1.0, (2 * K + 3, K))
    G = A.T @ A
    s_w = 0.013
    D = np.where(frozen, 0.0, s_w * (adaround.h_of(V) - r))
    e = adaround.row_errors(s_w * (np.rint(r) - r), G)
    return dict(V=V, r=r, frozen=frozen, G=G, inv_e=1.0 / e, s_w=s_w, n_free=int((~frozen).sum()), D=D)


STEP_EDGES = ('zeros', 'zeros_late', 'rows_of_one', 'all_frozen')


def step_edge_case(kind):
    """The step kernel's inputs step_case does not hold, as step_case's dict (+ first_t, and m, v, p_zero where set).  step_case itself stays
    as it is: step_float32_figure is measured on it.
      zeros        (3, 86) with V[0, :8] = 0.0 exactly: h = 0.5, x = 0, |x| = 0 and sign(x) = 0; P is 0 at [0, :4], so the gradient there is 0;
      zeros_late   the same from t = 10000 (c1 and c2 round to about 1), m and v as a long run leaves them: about g and g * g; the frozen
                   elements' m and v are set too, to show that nothing touches them;
      rows_of_one  (300, 1): K = 1, inv_e is one value per element across a workgroup boundary, nothing frozen;
      all_frozen   (2, 129) with every element frozen, m and v set.  n_free would be 0, which the pipeline never passes (it runs no step then)
                   and the entry point refuses; nothing reads it here, and it is 1."""
    Co, K = {'zeros': (3, 86), 'zeros_late': (3, 86), 'rows_of_one': (300, 1), 'all_frozen': (2, 129)}[kind]
    case = step_case(Co, K)
    case['first_t'] = 10000 if kind == 'zeros_late' else 1
    rng = np.random.default_rng(4321 + STEP_EDGES.index(kind))
    if kind in ('zeros', 'zeros_late'):
        case['V'][0, :8] = 0.0
        case['p_zero'] = np.zeros((Co, K), bool)
        case['p_zero'][0, :4] = True
    if kind == 'all_frozen':
        case['frozen'][:] = True
        case['n_free'] = 1
    case['D'] = np.where(case['frozen'], 0.0, case['s_w'] * (adaround.h_of(case['V']) - case['r']))
    if kind in ('zeros_late', 'all_frozen'):
        first, _ = run_steps(case, 0.0, 20.0, 1, np.float64)                    # m after one step from 0 is 0.1 g
        g = 10.0 * first[0][1]
        g = np.where(case['frozen'], 1e-3, g)
        case['m'] = g * rng.uniform(0.5, 1.5, (Co, K))
        case['v'] = g * g * rng.uniform(0.5, 2.0, (Co, K))
    return case


def run_steps(case, lam, beta, steps, dtype, products=None, first_t=1):
    """`steps` steps (t = first_t, first_t + 1, ...) of adaround.step in `dtype` from the case's state (m and v zero unless the case has them); P
    of step t is products[t] when given (the device's own), D G in float64 otherwise, 0 where the case's `p_zero` says so.
    -> ([(V, m, v, D) after every step] as float64, [P of every step])."""
    dt = dtype
    V, r = case['V'].astype(dt), case['r'].astype(dt)
    m, v = (case[k].astype(dt) if k in case else np.zeros_like(V) for k in ('m', 'v'))
    D = case['D'].astype(dt)
    inv_e = case['inv_e'].astype(dt)
    out, used = [], []
    for t in range(steps):
        P = (np.asarray(products[t], np.float64) if products is not None else adaround.quad(D.astype(np.float64), case['G'])).astype(dt)
        if products is None and 'p_zero' in case:
            P[case['p_zero']] = 0
        D = adaround.step(V, m, v, r, case['frozen'], P, inv_e, case['n_free'], case['s_w'], lam, beta, STEP_LR, first_t + t, dtype=dt)
        used.append(P.astype(np.float64))
        out.append(tuple(a.astype(np.float64).copy() for a in (V, m, v, D)))
    return out, used


def step_figure_of(case, lam, beta, steps=3, first_t=1):
    """The worst difference over `steps` steps on ONE case between the float32 numpy restatement of the step and the float64 rule fed the
    float32 run's own P, per array (V, m, v, D), each relative to the largest magnitude of that array in the float64 run."""
    a32, used = run_steps(case, lam, beta, steps, np.float32, first_t=first_t)
    a64, _ = run_steps(case, lam, beta, steps, np.float64, used, first_t=first_t)
    worst = np.zeros(4)
    for s64, s32 in zip(a64, a32):
        for k in range(4):
            scale = max(float(np.abs(s64[k]).max()), 1e-300)
            worst[k] = max(worst[k], float(np.abs(s32[k] - s64[k]).max()) / scale)
    return worst


@functools.lru_cache(maxsize=None)
def step_float32_figure(steps=3):
    """The worst difference, over STEP_SHAPES x STEP_MODES and `steps` steps, between the float32 numpy restatement of the step and the float64
    rule fed the float32 run's own P (as the GPU test feeds it the device's), per array (V, m, v, D), each relative to the largest magnitude of
    that array in the float64 run of its case."""
    worst = np.zeros(4)
    for (Co, K), (lam, beta) in itertools.product(STEP_SHAPES, STEP_MODES.values()):
        worst = np.maximum(worst, step_figure_of(step_case(Co, K), lam, beta, steps))
    return tuple(float(x) for x in worst)


@functools.lru_cache(maxsize=None)
def step_edge_figure(steps=3):
    """step_float32_figure's measurement on the inputs of step_edge_case: the worst of step_figure_of over STEP_EDGES x STEP_MODES, each case
    from its own first_t."""
    worst = np.zeros(4)
    for kind, (lam, beta) in itertools.product(STEP_EDGES, STEP_MODES.values()):
        case = step_edge_case(kind)
        worst = np.maximum(worst, step_figure_of(case, lam, beta, steps, case['first_t']))
    return tuple(float(x) for x in worst)
