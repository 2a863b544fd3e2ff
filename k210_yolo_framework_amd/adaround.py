"""Adaptive weight rounding of a quantised kmodel (`make kmodel ADAROUND=True`).

`quantize.quantize` rounds every kernel weight to the nearest of its 256 codes, which minimises each weight's own error.  The error of a conv's
OUTPUT is a quadratic form of all the rounding errors of a row (output channel) together; rounding some weights the other way lowers it.  The rule
below is restated from Nagel et al., "Up or Down? Adaptive Rounding for Post-Training Quantization", 2020 (AdaRound) - parity with the authors'
or AIMET's implementations is unpinned.  It is this project's own statement: numpy, float64, no torch; `gpu_optimise` drives the same rule
through the HIP kernels of csrc/yk_adaround.hip.

Set-up, per conv / depthwise layer.  `kern` is the kernel as quantize sees it (after equalisation if that is on), (s_w, zp_w) =
qparams(kern.min(), kern.max()), u = kern / s_w, f = floor(u), r = u - f.  A weight takes the code f + zp_w (down) or f + zp_w + 1 (up).  A
weight is FROZEN at quantize's own (nearest, clipped) code when r == 0 (it lies on the grid: a pruned zero stays exactly zp_w), when its up
code would exceed 255, or when its down code would be below 0 (the zero point is rounded, so the tensor's extreme weight can lie one step
outside the codes).

Objective.  Rows are independent.  For row c with rounding vector h in [0, 1]^K the weight error is d = s_w (h - r) and the output error over the
calibration set is E_c(h) = d^T G d, G = sum x x^T the Gram matrix of the layer's float input patches: K = 9 Ci in im2col order
k = (ky * 3 + kx) * Ci + ci for a 3x3 conv, K = Ci for a 1x1 conv, and a depthwise layer has its own 9 x 9 G_c per channel.

Two deliberate deviations from the paper:
  * the inputs are the FLOAT network's activations on frames / 255 (quantize.Calibrator's walk), not the quantised network's: the paper's
    asymmetric reconstruction feeds each layer what the quantised layers before it produce;
  * the activation function is left out of the objective.  With it out the data are touched once, to build G, and no iteration reads an
    activation again.

Relaxation.  h(V) = clip(sigmoid(V) (zeta - gamma) + gamma, 0, 1), zeta = 1.1, gamma = -0.1; V starts where h(V) = r.  The loss is
    L = (1 / Co) sum_c E_c(h) / E_c(nearest) + lam_t (1 / n) sum (1 - |2 h - 1|^beta_t)
with n the number of weights that are not frozen and E_c(nearest) evaluated at quantize's own codes.  A row with E_c(nearest) == 0 is left
alone (all its weights count as frozen).  lam_t = 0 for the first 20 % of the iterations; beta_t falls linearly from 20 to 2 over the rest.
The optimiser is Adam on V (beta1 0.9, beta2 0.999, eps 1e-8, bias-corrected); frozen elements are never updated, and in the relaxed loss their
error counts as 0 (for the at most two clipped weights of a tensor that is an approximation; the hardened check below uses the true error).

Hardening.  A weight rounds up iff h(V) >= 0.5.  Then E_c of the hard codes is evaluated in float64 on the host with every weight's true error
s_w (code - zp_w - u), and a row keeps its new codes only if E_c(new) < E_c(nearest); otherwise it keeps quantize's codes.  So no row of any
layer is worse than nearest rounding in its own objective, by construction.

A layer whose G would need more than `max_gram_mb` MiB (float64, K x K) is left at nearest and named in the report.

The defaults iters = 1000, lam = 0.01, lr = 1e-2 are starting points, not findings."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import netspec as ns
from .kmodel import KmodelError

ZETA, GAMMA = 1.1, -0.1
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
WARM_SHARE = 0.2
BETA_START, BETA_END = 20.0, 2.0
DEFAULT_ITERS, DEFAULT_LAMBDA, DEFAULT_LR, DEFAULT_MAX_GRAM_MB = 1000, 0.01, 1e-2, 1024


# ---- layout: a kernel as rows [Co][K] --------------------------------------------------------------------------------------------------
def rows_of(kern: np.ndarray, depthwise: bool) -> np.ndarray:
    """[Co][K] of a Keras kernel: conv [kh][kw][Ci][Co] -> k = (ky * kw + kx) * Ci + ci; depthwise [3][3][C][1] -> [C][9]."""
    kern = np.asarray(kern)
    if depthwise:
        return np.ascontiguousarray(kern[..., 0].reshape(9, -1).T)
    return np.ascontiguousarray(kern.transpose(3, 0, 1, 2).reshape(kern.shape[3], -1))


def kern_of(rows: np.ndarray, shape, depthwise: bool) -> np.ndarray:
    """The inverse of rows_of for a kernel of `shape`."""
    if depthwise:
        return np.ascontiguousarray(rows.T.reshape(3, 3, shape[2])[..., None])
    return np.ascontiguousarray(rows.reshape(shape[3], shape[0], shape[1], shape[2]).transpose(1, 2, 3, 0))


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def setup(kern: np.ndarray) -> dict:
    """s_w, zp_w, u, r, down (float64 code f + zp_w, before clipping), frozen, nearest (quantize's own uint8 codes), of any shape."""
    from .quantize import qparams
    kern = np.asarray(kern, np.float64)
    s_w, zp_w = qparams(kern.min(), kern.max())
    u = kern / s_w
    f = np.floor(u)
    r = u - f
    down = f + zp_w
    nearest = np.clip(np.rint(u) + zp_w, 0, 255).astype(np.uint8)
    frozen = (r == 0.0) | (down + 1.0 > 255.0) | (down < 0.0)
    return dict(s_w=s_w, zp_w=zp_w, u=u, r=r, down=down, frozen=frozen, nearest=nearest)


def allowed_codes(kern: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(down, up) uint8 codes of every weight, clipped to 0..255: the two codes quantize(weight_codes=) accepts."""
    st = setup(kern)
    return np.clip(st['down'], 0, 255).astype(np.uint8), np.clip(st['down'] + 1.0, 0, 255).astype(np.uint8)


def sigmoid(V):
    one = V.dtype.type(1)
    return one / (one + np.exp(-V))


def h_of(V: np.ndarray) -> np.ndarray:
    dt = V.dtype.type
    return np.clip(sigmoid(V) * (dt(ZETA) - dt(GAMMA)) + dt(GAMMA), dt(0), dt(1))


def v_init(r: np.ndarray) -> np.ndarray:
    """V with h(V) = r, float64."""
    p = (np.asarray(r, np.float64) - GAMMA) / (ZETA - GAMMA)
    return np.log(p / (1.0 - p))


def schedule(t: int, iters: int, lam: float) -> Tuple[float, float]:
    """(lam_t, beta_t) of iteration t = 0 .. iters - 1."""
    t0 = int(np.ceil(WARM_SHARE * iters))
    if t < t0:
        return 0.0, BETA_START
    return float(lam), BETA_START - (BETA_START - BETA_END) * (t - t0) / max(1, iters - 1 - t0)


def quad(D: np.ndarray, G: np.ndarray) -> np.ndarray:
    """P = D G per row: G [K][K] (dense) or [Co][9][9] (depthwise); G is symmetric."""
    return np.einsum('cij,cj->ci', G, D) if G.ndim == 3 else D @ G


def row_errors(D: np.ndarray, G: np.ndarray) -> np.ndarray:
    """E_c = d_c^T G d_c in float64."""
    D = np.asarray(D, np.float64)
    return (D * quad(D, np.asarray(G, np.float64))).sum(axis=1)


def hard_error(codes: np.ndarray, st: dict) -> np.ndarray:
    """The true weight error of uint8 codes: s_w (code - zp_w - u)."""
    return st['s_w'] * (codes.astype(np.float64) - st['zp_w'] - st['u'])


def step(V, m, v, r, frozen, P, inv_e, n_free: int, s_w: float, lam: float, beta: float, lr: float, t: int, dtype=np.float64) -> np.ndarray:
    """One Adam step (t = 1, 2, ...) on the free elements of V [Co][K], in place on V, m, v; returns the next D = s_w (h(V) - r), 0 at frozen
    elements.  P = D G for the D of the V given.  Every statement rounds once in `dtype`: with float32 it restates adaround_step_kernel."""
    dt = dtype
    one, two = dt(1), dt(2)
    Co = V.shape[0]
    s = dt(s_w)
    rec = dt(2.0 * float(s) / Co)
    reg = dt(2.0 * float(dt(lam)) * float(dt(beta)) / n_free)
    c1, c2 = dt(1.0 - 0.9 ** t), dt(1.0 - 0.999 ** t)
    b1, b2, eps, lr = dt(ADAM_B1), dt(ADAM_B2), dt(ADAM_EPS), dt(lr)
    span, gam = dt(ZETA) - dt(GAMMA), dt(GAMMA)
    sg = sigmoid(V)
    hr = sg * span + gam
    h = np.clip(hr, dt(0), one)
    dh = np.where((hr > 0) & (hr < 1), (sg * (one - sg)) * span, dt(0))
    g = (rec * inv_e[:, None]) * P
    if dt(lam) != 0:
        x = two * h - one
        ax = np.abs(x)
        if dt(beta) == 2:
            pw = ax
        else:
            with np.errstate(divide='ignore'):
                pw = np.where(ax == 0, dt(0), np.power(ax, dt(beta) - one))
        g = g - (reg * pw) * np.sign(x)
    g = g * dh
    mi = b1 * m + (one - b1) * g
    vv = b2 * v + ((one - b2) * g) * g
    vn = V - lr * ((mi / c1) / (np.sqrt(vv / c2) + eps))
    free = ~frozen
    m[free], v[free], V[free] = mi[free], vv[free], vn[free]
    return np.where(free, s * (h_of(V) - r), dt(0)).astype(dt)


def prepare(rows: np.ndarray, G: np.ndarray) -> dict:
    """setup(rows) + E_c(nearest) at quantize's codes and the rows left alone folded into `frozen`."""
    st = setup(rows)
    st['e_nearest'] = row_errors(hard_error(st['nearest'], st), G)
    st['frozen_weights'] = int(st['frozen'].sum())
    st['frozen'] = st['frozen'] | (st['e_nearest'] <= 0.0)[:, None]
    st['n_free'] = int((~st['frozen']).sum())
    with np.errstate(divide='ignore'):
        st['inv_e'] = np.where(st['e_nearest'] > 0.0, 1.0 / st['e_nearest'], 0.0)
    return st


def harden(V: np.ndarray, st: dict, G: np.ndarray) -> Tuple[np.ndarray, dict]:
    """uint8 codes [Co][K] from V and the layer's report entry: a row keeps its new codes only if they lower its float64 error."""
    up = h_of(np.asarray(V, np.float64)) >= 0.5
    new = np.where(st['frozen'], st['nearest'], np.clip(st['down'] + up, 0, 255).astype(np.uint8)).astype(np.uint8)
    e_new = row_errors(hard_error(new, st), G)
    better = e_new < st['e_nearest']
    codes = np.where(better[:, None], new, st['nearest']).astype(np.uint8)
    e_final = np.where(better, e_new, st['e_nearest'])
    e_n, e_a = float(st['e_nearest'].sum()), float(e_final.sum())
    info = dict(rows=int(len(better)), rows_changed=int(better.sum()), flipped=int((codes != st['nearest']).sum()), e_nearest=e_n, e_adaround=e_a,
                ratio=(e_a / e_n if e_n > 0.0 else 1.0), frozen=st['frozen_weights'], skipped=False, e_rows_nearest=st['e_nearest'], e_rows=e_final)
    return codes, info


def optimise_numpy(rows: np.ndarray, G: np.ndarray, iters: int = DEFAULT_ITERS, lam: float = DEFAULT_LAMBDA, lr: float = DEFAULT_LR):
    """The float64 host twin of the GPU loop.  rows: the layer's kernel as [Co][K] (rows_of); G: [K][K] or [Co][9][9].
    -> (uint8 codes [Co][K], the layer's report entry)."""
    rows, G = np.asarray(rows, np.float64), np.asarray(G, np.float64)
    st = prepare(rows, G)
    V = v_init(st['r'])
    if st['n_free'] and iters > 0:
        m, v = np.zeros_like(V), np.zeros_like(V)
        D = np.where(st['frozen'], 0.0, st['s_w'] * (h_of(V) - st['r']))
        for t in range(iters):
            lam_t, beta_t = schedule(t, iters, lam)
            D = step(V, m, v, st['r'], st['frozen'], quad(D, G), st['inv_e'], st['n_free'], st['s_w'], lam_t, beta_t, lr, t + 1)
    return harden(V, st, G)


def skipped_entry(kern: np.ndarray, need_mb: float) -> dict:
    return dict(rows=0, rows_changed=0, flipped=0, e_nearest=float('nan'), e_adaround=float('nan'), ratio=1.0, frozen=0, skipped=True,
                gram_mb=float(need_mb))


def format_report(rep: dict) -> str:
    rows = []
    for name, r in rep['layers'].items():
        if r['skipped']:
            rows.append(f"adaround {name}: SKIPPED, its Gram matrix needs {r['gram_mb']:.0f} MiB (cap {rep['max_gram_mb']}): left at nearest")
        else:
            rows.append(f"adaround {name}: {r['rows_changed']}/{r['rows']} rows changed, {r['flipped']} weights flipped, {r['frozen']} frozen, "
                        f"E {r['e_nearest']:.6g} -> {r['e_adaround']:.6g} (x{r['ratio']:.4f})")
    done = [r for r in rep['layers'].values() if not r['skipped']]
    rows.append(f"adaptive rounding: {len(done)} layers ({len(rep['layers']) - len(done)} skipped), {rep['iters']} iterations each, lambda "
                f"{rep['lam']:g}, lr {rep['lr']:g}, {sum(r['flipped'] for r in done)} weights flipped")
    return '\n'.join(rows)


# ---- the GPU driver --------------------------------------------------------------------------------------------------------------------
def gram_shape(op: dict) -> Tuple[int, ...]:
    """The shape of a conv op's Gram matrix: (C, 9, 9) depthwise, (K, K) dense."""
    if op['type'] == ns.OP_DWCONV:
        return (int(op['cout']), 9, 9)
    K = int(op['k']) * int(op['k']) * int(op['cin'])
    return (K, K)


def gpu_grams(spec: ns.NetSpec, weights, frames, batch: int = 32, max_gram_mb: float = DEFAULT_MAX_GRAM_MB, only=None):
    """{conv layer name: float64 device tensor G} over `frames` (uint8 [N, H, W, 3], host numpy or a device tensor) in batches of `batch`, and
    {name: MiB} of the layers the cap leaves out.  Every batch is one Calibrator walk that keeps its tensors; a depthwise layer's G is
    yk_dw3x3_gram_f32, a dense layer's one fp32 product X^T X per batch (yk_im2col3x3_f32 for 3x3, the tensor itself for 1x1, into yk_gemm_f32)
    added into the float64 accumulator.  `only`: a set of layer names (the others are not built)."""
    import ctypes as C
    from types import SimpleNamespace
    import torch
    from . import engine
    from .quantize import Calibrator, device_batches
    batch = max(1, min(int(batch), len(frames)))
    cal = Calibrator(spec, weights, max_batch=batch)
    convs_only = SimpleNamespace(conv=cal.range.conv, moved=lambda y, slot: None)      # a measure that leaves the moved tensors alone
    dev = cal.dev
    convs = [op for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV) and (only is None or op['layer'] in only)]
    G: Dict[str, "torch.Tensor"] = {}
    skipped: Dict[str, float] = {}
    for op in convs:
        shape = gram_shape(op)
        mb = float(np.prod(shape)) * 8.0 / 2.0 ** 20
        if mb > float(max_gram_mb):
            skipped[op['layer']] = mb
        else:
            G[op['layer']] = torch.zeros(shape, dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream                            # noqa: E731
    for fr in device_batches(frames, batch):
        B = int(fr.shape[0])
        keep: Dict[str, "torch.Tensor"] = {}
        cal.forward(fr, convs_only, keep, 'adaround')                                  # the float network on frames / 255
        for op in convs:
            name = op['layer']
            if name not in G:
                continue
            x = keep[cal.names[op['in0']]]
            hi, wi, ci = spec.tensors[op['in0']]
            ho, wo, _ = spec.tensors[op['out']]
            geom = [B, hi, wi, ci, ho, wo, op['stride'], op['pad_t'], op['pad_l']]
            M = B * ho * wo
            if op['type'] == ns.OP_DWCONV:
                need = C.c_size_t()
                engine.call('yk_dw3x3_gram_workspace_bytes', B, ho, wo, ci, C.byref(need))
                work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
                engine.call('yk_dw3x3_gram_f32', x, *geom, G[name], work, stream())
                del work
                continue
            K = G[name].shape[0]
            if op['k'] == 1:
                X = x
            else:
                X = torch.empty((M, K), dtype=torch.float32, device=dev)
                engine.call('yk_im2col3x3_f32', x, *geom, X, stream())
            part = torch.empty((K, K), dtype=torch.float32, device=dev)
            engine.call('yk_gemm_f32', 1, 0, K, K, M, 1.0, X, K, X, K, 0.0, part, K, stream())
            G[name] += part.double()
            del X, part
        del keep
    return G, skipped


def gpu_optimise_layer(rows: np.ndarray, G, iters: int, lam: float, lr: float, report_every: int = 0):
    """One layer on the GPU.  rows [Co][K] float64 (rows_of), G the layer's float64 device Gram matrix.  -> (uint8 codes [Co][K], entry).
    Per iteration: P = D G (yk_gemm_f32 on the fp32 copy of G, or yk_adaround_dw_quad_f32), then yk_adaround_step_f32; nothing is read back
    inside the loop - the per-row soft errors (yk_adaround_rowerr_f64) taken every `report_every` iterations stay on the device until the end."""
    import torch
    from . import engine
    Gh = G.cpu().numpy()
    st = prepare(np.asarray(rows, np.float64), Gh)
    V64 = v_init(st['r'])
    Co, K = V64.shape
    trace, loop_ms = [], 0.0
    if st['n_free'] and iters > 0:
        dev = G.device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)       # noqa: E731
        V, r = f32(V64), f32(st['r'])
        m, v, P = torch.zeros_like(V), torch.zeros_like(V), torch.empty_like(V)
        frozen = torch.from_numpy(np.ascontiguousarray(st['frozen'], np.uint8)).to(dev)
        inv_e = f32(st['inv_e'])
        V32 = V64.astype(np.float32)
        D = f32(np.where(st['frozen'], np.float32(0), np.float32(st['s_w']) * (h_of(V32) - st['r'].astype(np.float32))))
        dense = G.dim() == 2
        G32 = G.float() if dense else None
        stream = torch.cuda.current_stream().cuda_stream

        def product():
            if dense:
                engine.call('yk_gemm_f32', 0, 0, Co, K, K, 1.0, D, K, G32, K, 0.0, P, K, stream)
            else:
                engine.call('yk_adaround_dw_quad_f32', G, D, Co, P, stream)

        def soft(t):
            E = torch.empty(Co, dtype=torch.float64, device=dev)
            engine.call('yk_adaround_rowerr_f64', D, P, Co, K, E, stream)
            trace.append((t, E))

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(iters):
            lam_t, beta_t = schedule(t, iters, lam)
            product()
            if report_every and t % report_every == 0:
                soft(t)
            engine.call('yk_adaround_step_f32', V, m, v, r, frozen, P, inv_e, D, Co, K, st['n_free'], st['s_w'], lam_t, beta_t, lr, t + 1, stream)
        e1.record()
        product()
        soft(iters)
        V64 = V.cpu().numpy().astype(np.float64)
        loop_ms = float(e0.elapsed_time(e1))                                    # read after the copy above has waited for the stream
    codes, info = harden(V64, st, Gh)
    info['loop_ms'], info['free'] = loop_ms, st['n_free']
    info['soft'] = [(t, float((E.cpu().numpy() * st['inv_e']).sum() / Co)) for t, E in trace]       # the reconstruction term of L
    return codes, info


def gpu_optimise(spec: ns.NetSpec, weights, frames, batch: int = 32, iters: int = DEFAULT_ITERS, lam: float = DEFAULT_LAMBDA,
                 lr: float = DEFAULT_LR, max_gram_mb: float = DEFAULT_MAX_GRAM_MB, report_every: int = 0):
    """-> (weight_codes {conv layer name: uint8 array of kern's shape} for quantize.quantize(weight_codes=), report).  The Gram matrices of all
    layers are built first (gpu_grams: one float pass over the frames), then every layer is optimised and hardened, its Gram matrix freed as it
    goes.  report['layers'][name] = dict(rows, rows_changed, flipped, e_nearest, e_adaround, ratio, frozen, skipped, ...); a layer the cap
    skips is in the report and not in weight_codes."""
    if not (int(iters) >= 0 and float(lam) >= 0.0 and float(lr) > 0.0):
        raise KmodelError(f'adaround: iters {iters} and lambda {lam} must not be negative and lr {lr} must be positive')
    G, skipped = gpu_grams(spec, weights, frames, batch, max_gram_mb)
    codes: Dict[str, np.ndarray] = {}
    rep = {'layers': {}, 'iters': int(iters), 'lam': float(lam), 'lr': float(lr), 'max_gram_mb': max_gram_mb}
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        name, dw = op['layer'], op['type'] == ns.OP_DWCONV
        kern = np.asarray(weights[name + '/kernel'], np.float64)
        if name in skipped:
            rep['layers'][name] = skipped_entry(kern, skipped[name])
            continue
        c, info = gpu_optimise_layer(rows_of(kern, dw), G.pop(name), int(iters), float(lam), float(lr), report_every)
        codes[name] = kern_of(c, kern.shape, dw)
        rep['layers'][name] = info
    return codes, rep
