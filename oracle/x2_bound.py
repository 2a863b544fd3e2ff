"""x2_bound.py — CPU ORACLE (test infrastructure, NOT the product path): a float64 reference for ONE LAUNCH of the f16x2 mode
together with an elementwise bound on what that launch may get wrong.

Written from the arithmetic of DESIGN.md section 2; shares no code with netspec.compile_plan's folding nor with the HIP sources.

Three parts:
  * `run_chain`: a sub-chain of a NetSpec (any list of ops, started from any set of tensors) in torch-CPU float64, and for every op
    the bound `E` on |what the launch stores - exact result|, propagated through the chain;
  * `model_conv` / `model_dw`: a numpy model of the kernels' arithmetic (hi / lo splits, three products, fp32 accumulation in k-steps
    of 32, the fp32 epilogue, the split store) with switchable defects - the source of the constant `C_DOT` and of the mutants that
    tests/test_x2_bound.py holds the comparison to;
  * `compare` / `split_health`: the comparison and the format checks the GPU test and the CPU test share.

The bound
---------
Conv / depthwise with folded BatchNorm (scale_n, bias_n), T = |scale_n| * (|W| conv |x|) + |bias_n| (the same convolution on absolute
values: the yardstick of a dot product, S = sum |w||x|, carried through the epilogue):

    E_out = |scale_n| * (|W| conv E_in)  +  C_DOT * 2^-22 * T  +  storage(out)

ReLU, ReLU6 and LeakyReLU (slope <= 1) are 1-Lipschitz: E passes through them unchanged, every element is compared, no "gate flip"
exclusions.  MaxPool: window maximum of E (|max a - max b| <= max |a - b|).  UpSample / Concat: the copy / the concatenation.
Add: E_a + E_b + 2^-24 * (|a| + |b|) (one fp32 rounding of the sum).

storage(out), derived from the format.  A split tensor holds s = y * 2^-e = hi + lo, e per image.  The epilogue's order: the fp32
value v (its own rounding belongs to the C_DOT term), s = v * 2^-e (a power of two: exact, |s| < 2^14 by the choice of e),
hi = RN16(s), r = s - hi (exact in fp32: s has 24 bits, hi is its leading 11), lo = RN16(r).  fp16 has 11 significant bits, so
|s - hi| <= 2^-11 |s| when hi is normal; then |r - lo| <= 2^-11 |r| <= 2^-22 |s| when lo is normal.  The constant is 2^-22, not
2^-23: RN16's relative error reaches 2^-11 just above a power of two, twice in a row.  When lo (or hi itself) is subnormal, its
spacing is 2^-24 and the error at most 2^-25, absolute.  Hence
    split:                  2^-22 * |y| + 2^(e_b - 25)        (e_b = the stored exponent of image b, read back from the plan)
    fp32 planes, outputs:   2^-24 * |y|                       (one RN32; planes carry exponent 0)
    inner tensor of a fused launch (never stored, no exponent to read): DESIGN section 2 - its exponent comes from bounds of bounds
        that over-estimate the image's true maximum a_b by at most 2^12; e normalises the bound into [2^13, 2^14), so
        2^e <= 2^12 * a_b * 2^-13 and the floor 2^(e - 25) <= a_b * 2^-26:   2^-22 * |y| + 2^-26 * a_b   (a_b from the reference).
Read-back (hi + lo in fp32, times 2^e) is exact: hi + lo is a multiple of s's last bit and smaller than 2|s|.

C_DOT is fixed by `derive_c()` below, from the numpy model alone, before any kernel was run against this bound: 4 x the worst
error / (2^-22 * T) the correct model shows over the K values of the four reference networks.  The factor 4 pays for what the model
does not know (the summation order inside an MFMA, split-K slices, the order of the epilogue's fma).  It must stay <= 1/8 of the
smallest ratio the same model shows with one cross product dropped (`derive_c` asserts it).  It is not tuned against the kernels.
"""
import numpy as np
import torch
import torch.nn.functional as F

from k210_yolo_framework_amd import netspec as ns

# derive_c() on the K values below (seed 0, 512 dot products per K): worst ratio of the correct model 2.64 (K = 1152; the sequential fp32
# accumulation of 3K products dominates it, not the split), smallest ratio with a cross product dropped 109 (K = 9216).  4 x 2.64 = 10.6,
# rounded up; 8 x 11 = 88 <= 109.  tests/test_x2_bound.py re-derives both figures.
C_DOT = 11.0
K_VALUES = (27, 32, 124, 288, 384, 1152, 3456, 4608, 9216)     # 3x3x3 stem ... 3x3x1024: the span of the four reference networks
INNER_OVER_LOG2 = 12                                           # bounds of bounds over-estimate by at most 2^12


# ----------------------------------------------------------------------------------------------------------------------
# float64 sub-chain runner with the propagated bound
# ----------------------------------------------------------------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def fold(layer, weights):
    """Keras inference BatchNorm as y = acc * scale + bias, in float64 -> (scale, bias) per output channel."""
    c = layer.kernel_shape[3] if layer.kind == 'conv' else layer.kernel_shape[2]
    if layer.bn_name:
        g, bt, mu, var = (np.asarray(weights[layer.bn_name + s], np.float64) for s in ('/gamma', '/beta', '/moving_mean', '/moving_variance'))
        scale = g / np.sqrt(var + ns.BN_EPS)
        return scale, bt - mu * scale
    return np.ones(c), (np.asarray(weights[layer.name + '/bias'], np.float64) if layer.use_bias else np.zeros(c))


def _act(y, op):
    a = op['act']
    if a == ns.ACT_RELU:
        return F.relu(y)
    if a == ns.ACT_RELU6:
        return torch.clamp(y, 0, 6)
    if a == ns.ACT_LEAKY:
        return F.leaky_relu(y, op['alpha'])
    return y


def storage(y_abs, fmt):
    """What the stored form of a tensor may lose (module docstring).  y_abs: |reference| NCHW float64.
    fmt: None (exact: not stored by the launch under test) | ('split', e int[B]) | ('f32',) | ('inner',)."""
    if fmt is None:
        return torch.zeros_like(y_abs)
    if fmt[0] == 'f32':
        return 2.0 ** -24 * y_abs
    if fmt[0] == 'split':
        e = torch.as_tensor(np.asarray(fmt[1], np.float64)).reshape(-1, 1, 1, 1)
        return 2.0 ** -22 * y_abs + torch.exp2(e - 25)
    if fmt[0] == 'inner':
        a = y_abs.amax(dim=(1, 2, 3), keepdim=True)
        return 2.0 ** -22 * y_abs + 2.0 ** (INNER_OVER_LOG2 - 13 - 25) * a
    raise ValueError(fmt)


def run_chain(spec, weights, inputs, op_idx=None, fmt=None, c=C_DOT, bounds=True, e_inputs=None):
    """Run spec.ops[i] for i in op_idx (default: all) in float64 from `inputs` = {tensor id: NHWC array}.
    fmt: {tensor id: storage format} of the tensors the chain produces (see `storage`; missing = exact).
    e_inputs: {tensor id: NHWC bound} for inputs that are not exact (default: exact).
    -> (Y, E): {tensor id: NHWC float64} for every tensor the chain produced (E only when `bounds`)."""
    lay = {l.name: l for l in spec.layers}
    fmt = fmt or {}
    Y = {t: _nchw(v) for t, v in inputs.items()}
    E = {t: (_nchw(e_inputs[t]) if e_inputs and t in e_inputs else None) for t in inputs}      # None = exactly zero
    made = []
    with torch.no_grad():
        for i in (range(len(spec.ops)) if op_idx is None else op_idx):
            op = spec.ops[i]
            x, ex = Y[op['in0']], E[op['in0']]
            t = op['type']
            if t in (ns.OP_CONV, ns.OP_DWCONV):
                l = lay[op['layer']]
                k = torch.from_numpy(np.asarray(weights[l.name + '/kernel'], np.float64))
                w = (k.permute(3, 2, 0, 1) if t == ns.OP_CONV else k.permute(2, 3, 0, 1)).contiguous()
                scale, bias = (torch.from_numpy(v).reshape(1, -1, 1, 1) for v in fold(l, weights))
                ho, wo, _ = spec.tensors[op['out']]
                kk, st = op['k'], op['stride']
                pb = max((ho - 1) * st + kk - x.shape[2] - op['pad_t'], 0)
                pr = max((wo - 1) * st + kk - x.shape[3] - op['pad_l'], 0)
                groups = x.shape[1] if t == ns.OP_DWCONV else 1

                def conv(v, ww):
                    return F.conv2d(F.pad(v, (op['pad_l'], pr, op['pad_t'], pb)), ww, None, stride=st, groups=groups)[:, :, :ho, :wo]
                y = _act(conv(x, w) * scale + bias, op)
                e = None
                if bounds:
                    e = c * 2.0 ** -22 * (conv(x.abs(), w.abs()) * scale.abs() + bias.abs())
                    if ex is not None:
                        e = e + conv(ex, w.abs()) * scale.abs()
            elif t == ns.OP_MAXPOOL:
                ho, wo, _ = spec.tensors[op['out']]
                st = op['stride']
                pb = max((ho - 1) * st + 2 - x.shape[2], 0)
                pr = max((wo - 1) * st + 2 - x.shape[3], 0)
                y = F.max_pool2d(F.pad(x, (0, pr, 0, pb), value=float('-inf')), 2, st)
                e = None if ex is None or not bounds else F.max_pool2d(F.pad(ex, (0, pr, 0, pb)), 2, st)
            elif t == ns.OP_UPSAMPLE:
                y = F.interpolate(x, scale_factor=2, mode='nearest')
                e = None if ex is None or not bounds else F.interpolate(ex, scale_factor=2, mode='nearest')
            elif t == ns.OP_CONCAT:
                x1, e1 = Y[op['in1']], E[op['in1']]
                y = torch.cat([x, x1], 1)
                e = None
                if bounds and (ex is not None or e1 is not None):
                    e = torch.cat([torch.zeros_like(x) if ex is None else ex, torch.zeros_like(x1) if e1 is None else e1], 1)
            elif t == ns.OP_ADD:
                x1, e1 = Y[op['in1']], E[op['in1']]
                y = x + x1
                e = None
                if bounds:
                    e = 2.0 ** -24 * (x.abs() + x1.abs())
                    for q in (ex, e1):
                        if q is not None:
                            e = e + q
            else:
                raise ValueError(t)
            if bounds and op['out'] in fmt and fmt[op['out']] is not None:
                s = storage(y.abs(), fmt[op['out']])
                e = s if e is None else e + s
            Y[op['out']], E[op['out']] = y, e
            made.append(op['out'])
    Yo = {t: _nhwc(Y[t]) for t in made}
    Eo = {t: (_nhwc(E[t]) if E[t] is not None else np.zeros_like(Yo[t])) for t in made} if bounds else None
    return Yo, Eo


def launch_chain(spec, stored, tid):
    """The ops one launch ran to make stored tensor `tid`: walk back from it to the nearest tensors in `stored` (ids the plan keeps in
    memory, tensor 0 included).  -> (sorted op indices, input tensor ids)."""
    producer = {op['out']: i for i, op in enumerate(spec.ops)}
    rows, inputs = set(), set()

    def need(t, top):
        if t in stored and not top:
            inputs.add(t)
            return
        j = producer[t]
        o = spec.ops[j]
        need(o['in0'], False)
        if o['in1'] >= 0:
            need(o['in1'], False)
        rows.add(j)
    need(tid, True)
    return sorted(rows), sorted(inputs)


# ----------------------------------------------------------------------------------------------------------------------
# the comparison both suites use
# ----------------------------------------------------------------------------------------------------------------------
def compare(got, ref, E):
    """-> (worst |got - ref| / E over EVERY element, index of that element).  An element with E = 0 must be exact (ratio inf otherwise);
    a non-finite value anywhere is ratio inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / E)
    r = np.where(np.isfinite(got) & ~np.isnan(r), r, np.inf)
    i = int(np.argmax(r))
    return float(r.flat[i]), tuple(int(v) for v in np.unravel_index(i, r.shape))


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def exp_of(bound):
    """The kernels' normalisation of a storage exponent (x_exp_of): bound * 2^-e in [2^13, 2^14); 0 / inf / nan -> 0."""
    bound = np.asarray(bound, np.float32)
    ok = np.isfinite(bound) & (bound >= np.float32(2.0 ** -126))
    return np.where(ok, np.floor(np.log2(np.where(ok, bound, 1).astype(np.float64))).astype(np.int64) - 13, 0).astype(np.int32)


def is_split(v, e):
    """True where an fp32 read-back value is hi + lo of two fp16 numbers at exponent e[b] (what a split tensor can hold)."""
    s = np.ldexp(np.asarray(v, np.float32), -np.asarray(e, np.int32).reshape(-1, 1, 1, 1)).astype(np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        hi = f16(s)
        return hi + f16(s - hi) == s


def split_health(v, e):
    """Format health of one stored split tensor (read-back values v [B,H,W,C], exponents e [B]).
    The epilogue normalises e so that bound * 2^-e lies in [2^13, 2^14) (x_exp_of: e = exponent(bound) - 13): with the TRUE maximum
    amax <= bound the scaled maximum is below 2^14 < 65504 (hi is never inf), and the bound's over-estimate bound / amax lies within
    a factor 2 of 2^(e + 14) / amax, which is what is reported and held below 2^16.
    -> (ok, worst over-estimate over the images with a non-zero maximum, message)."""
    v = np.asarray(v, np.float32)
    if not np.isfinite(v).all():
        return False, np.inf, 'non-finite read-back'
    worst = 0.0
    for b in range(v.shape[0]):
        amax = float(np.abs(v[b]).max())
        if amax == 0:
            continue
        scaled = amax * 2.0 ** -int(e[b])
        if not scaled < 65504:
            return False, np.inf, f'image {b}: scaled maximum {scaled:.4g} does not fit fp16'
        worst = max(worst, 2.0 ** 14 / scaled)
    if not worst < 2.0 ** 16:
        return False, worst, f'over-estimate 2^{np.log2(worst):.1f} >= 2^16'
    return True, worst, ''


# ----------------------------------------------------------------------------------------------------------------------
# numpy model of the kernels' arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def store_split(y, e):
    """fp32 values y [B,...] -> what reading the split tensor back gives: (RN16(s) + RN16(s - RN16(s))) * 2^e, s = y * 2^-e."""
    e = np.asarray(e, np.int32).reshape((-1,) + (1,) * (np.ndim(y) - 1))
    s = np.ldexp(np.asarray(y, np.float32), -e).astype(np.float32)
    hi = f16(s)
    lo = f16(s - hi)
    return np.ldexp((hi + lo).astype(np.float32), e).astype(np.float32), hi, lo


def _apply_act(v, act, alpha):
    if act == ns.ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ns.ACT_RELU6:
        return np.clip(v, np.float32(0), np.float32(6))
    if act == ns.ACT_LEAKY:
        return np.maximum(v, v * np.float32(alpha))
    return v


def _im2col(x, k, stride, pad_t, pad_l, ho, wo, wrap_col=None):
    """x [B,H,W,C] -> [B,ho,wo,k*k,C]; taps outside the image are zero.  wrap_col=j: the defect 'one border column computed with a
    wrapped tap' - for output column j the out-of-image taps read the linear neighbour (the end of the previous row) instead."""
    B, H, W, C = x.shape
    out = np.zeros((B, ho, wo, k * k, C), x.dtype)
    flat = x.reshape(B, H * W, C)
    for oy in range(ho):
        for ox in range(wo):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * stride + ky - pad_t, ox * stride + kx - pad_l
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, oy, ox, ky * k + kx] = x[:, iy, ix]
                    elif wrap_col is not None and ox == wrap_col and 0 <= iy < H and 0 < iy * W + ix < H * W:
                        out[:, oy, ox, ky * k + kx] = flat[:, iy * W + ix]
    return out


def _dot3(A, Wm, drop_lohi=False, drop_hilo_step=None, slices=1):
    """A = (a_hi, a_lo) [M,K], Wm = (w_hi, w_lo) [N,K], fp16 values held in fp32, K a multiple of 32 -> fp32 [M,N]: per k-step of 32 the
    three products w_lo*x_hi, w_hi*x_lo, w_hi*x_hi, every product exact in fp32 (11 x 11 bits), added one at a time to an fp32
    accumulator; `slices` > 1: K cut into that many accumulators, added in z order."""
    (ah, al), (wh, wl) = A, Wm
    M, K = ah.shape
    nst = K // 32
    cut = [(z * nst) // slices for z in range(slices + 1)]
    total = None
    for z in range(slices):
        acc = np.zeros((M, wh.shape[0]), np.float32)
        for st in range(cut[z], cut[z + 1]):
            ks = range(st * 32, st * 32 + 32)
            for a, w, skip in ((ah, wl, drop_lohi), (al, wh, drop_hilo_step == st), (ah, wh, False)):
                if skip:
                    continue
                for kq in ks:
                    acc = acc + a[:, kq, None] * w[None, :, kq]
        total = acc if total is None else total + acc
    return total


def conv_gain(Wk, scale, bias):
    """The plan's a-priori bound of a conv output: |y| <= gain * amax(in) + off."""
    return float((np.abs(scale) * np.abs(Wk).reshape(-1, Wk.shape[-1]).sum(0)).max()), float(np.abs(bias).max())


def model_conv(x, e_in, Wk, scale, bias, op, ho, wo, out='split', mutate=None, slices=1):
    """One conv launch as the f16x2 kernels compute it.  x [B,H,W,C]: the stored input as read back (fp32), e_in [B] its exponents;
    Wk HWIO fp32, scale / bias float64 folded BatchNorm.  out: 'split' | 'f32'.
    mutate: None | ('drop_lohi',) | ('drop_hilo_step', step) | ('wrap_col', j) | ('tail_nonzero',) | ('hi_only',) | ('mate_exponent', b).
    -> (read-back values [B,ho,wo,N] fp32, e_out int32 [B])."""
    m = mutate or ('none',)
    B, H, W_, C = x.shape
    k, N = op['k'], Wk.shape[3]
    e_in = np.asarray(e_in, np.int32)
    _, xh, xl = store_split(x, e_in)                                          # the halves as the kernel loads them
    Cp = -(-C // 32) * 32                                                     # a k-step is 32 channels of one tap
    sexp = 13 - int(np.floor(np.log2(np.abs(Wk).max())))                      # max |w * 2^s| in [2^13, 2^14)
    ws = np.ldexp(Wk.astype(np.float32), sexp).astype(np.float32).reshape(k * k, C, N)
    wh = f16(ws)
    wl = f16(ws - wh)
    pad = lambda a, ax: np.concatenate([a, np.zeros(a.shape[:ax] + (Cp - C,) + a.shape[ax + 1:], np.float32)], ax)
    wh, wl = pad(wh, 1), pad(wl, 1)
    cols = [_im2col(h, k, op['stride'], op['pad_t'], op['pad_l'], ho, wo, m[1] if m[0] == 'wrap_col' else None) for h in (xh, xl)]
    cols = [pad(c_, 4) for c_ in cols]
    if m[0] == 'tail_nonzero' and Cp > C:                                     # the channels past the tensor arrive non-zero on both sides
        g = np.random.default_rng(5)
        cols[0][..., C:] = f16(g.uniform(0, 2.0 ** -6, cols[0][..., C:].shape) * np.abs(xh).max())
        wh[:, C:, :] = wh[:, :Cp - C, :]
    scale32 = (scale * 2.0 ** -sexp).astype(np.float32)                       # the stored scale carries 2^-s
    bias32 = bias.astype(np.float32)
    gain, off = conv_gain(Wk, scale, bias)
    amax_in = np.abs(x).reshape(B, -1).max(1)
    cap = 6.0 if op['act'] == ns.ACT_RELU6 else np.inf
    e_out = exp_of(np.minimum(np.float32(gain) * amax_in.astype(np.float32) + np.float32(off), np.float32(cap))) if out == 'split' else np.zeros(B, np.int32)
    y = np.zeros((B, ho, wo, N), np.float32)
    Wm = (wh.reshape(-1, N).T.copy(), wl.reshape(-1, N).T.copy())
    for b in range(B):
        A = tuple(c_[b].reshape(ho * wo, -1) for c_ in cols)
        acc = _dot3(A, Wm, m[0] == 'drop_lohi', m[1] if m[0] == 'drop_hilo_step' else None, slices)
        up = np.float32(2.0) ** np.float32(e_in[m[1]] if m[0] == 'mate_exponent' and b != m[1] else e_in[b])
        v = ((acc * up).astype(np.float64) * scale32.astype(np.float64) + bias32.astype(np.float64)).astype(np.float32)   # one fma
        y[b] = _apply_act(v, op['act'], op['alpha']).reshape(ho, wo, N)
    if out == 'f32':
        return y, e_out
    got, hi, _ = store_split(y, e_out)
    if m[0] == 'hi_only':
        got = np.ldexp(hi, e_out.reshape(-1, 1, 1, 1)).astype(np.float32)
    return got, e_out


def model_dw(x, e_in, Wk, scale, bias, op, ho, wo):
    """A depthwise 3x3 launch: nine fp32 fmas on x = (hi + lo) * 2^e, BatchNorm as one fma, activation, split store."""
    B, H, W_, C = x.shape
    col = _im2col(np.asarray(x, np.float32), 3, op['stride'], op['pad_t'], op['pad_l'], ho, wo)
    w = Wk[..., 0].astype(np.float32).reshape(9, C)
    acc = np.zeros((B, ho, wo, C), np.float32)
    for t in range(9):
        acc = (acc.astype(np.float64) + col[:, :, :, t].astype(np.float64) * w[t].astype(np.float64)).astype(np.float32)
    v = (acc.astype(np.float64) * scale.astype(np.float32).astype(np.float64) + bias.astype(np.float32).astype(np.float64)).astype(np.float32)
    y = _apply_act(v, op['act'], op['alpha'])
    gain = float((np.abs(scale) * np.abs(w).sum(0)).max())
    amax_in = np.abs(x).reshape(B, -1).max(1).astype(np.float32)
    e_out = exp_of(np.float32(gain) * amax_in + np.float32(np.abs(bias).max()))
    return store_split(y, e_out)[0], e_out


def model_input(rng, B, H, W, C, over_log2=7):
    """Uneven post-ReLU activations, stored split with an exponent that over-estimates each image's maximum by 2^over_log2 (DESIGN
    section 2: 2^6 - 2^8 in these nets); images of different magnitude.  -> (read-back values: exactly what the store holds, e [B])."""
    x = np.maximum(rng.normal(0.2, 1.0, (B, H, W, C)), 0) * rng.lognormal(0.0, 1.0, (1, 1, 1, C)) * (4.0 ** np.arange(B)).reshape(B, 1, 1, 1)
    x = x.astype(np.float32)
    e = exp_of(np.abs(x).reshape(B, -1).max(1) * 2.0 ** over_log2)
    return store_split(x, e)[0], e


def _dot_ratio(rng, K, rows, drop=None):
    """error / (2^-22 * S) of `rows` independent K-long dot products in the model's arithmetic; drop: None | 'lohi' | 'hilo'."""
    Kp = -(-K // 32) * 32
    x = np.zeros((rows, Kp), np.float32)
    w = np.zeros((rows, Kp), np.float32)
    x[:, :K] = np.maximum(rng.normal(0.2, 1.0, (rows, K)), 0) * rng.lognormal(0.0, 1.0, (1, K))
    w[:, :K] = rng.normal(0.0, np.sqrt(2.0 / K), (rows, K))
    e = exp_of(np.abs(x).max() * 2.0 ** 7)
    sexp = 13 - int(np.floor(np.log2(np.abs(w).max())))
    xs, ws = np.ldexp(x, -e).astype(np.float32), np.ldexp(w, sexp).astype(np.float32)
    xh, wh = f16(xs), f16(ws)
    xl, wl = f16(xs - xh), f16(ws - wh)
    acc = np.zeros(rows, np.float32)
    for st in range(Kp // 32):
        for a, b, skip in ((xh, wl, drop == 'lohi'), (xl, wh, drop == 'hilo'), (xh, wh, False)):
            if skip:
                continue
            for kq in range(st * 32, st * 32 + 32):
                acc = acc + a[:, kq] * b[:, kq]
    got = acc.astype(np.float64) * 2.0 ** (int(e) - sexp)
    ref = (x.astype(np.float64) * w.astype(np.float64)).sum(1)
    S = (np.abs(x).astype(np.float64) * np.abs(w).astype(np.float64)).sum(1)
    return float((np.abs(got - ref) / (2.0 ** -22 * S)).max())


def derive_c(seed=0, rows=512):
    """-> (4 x the worst ratio of the correct model over K_VALUES, the smallest ratio with a cross product dropped).  Asserts the condition
    under which the bound separates: at every K, C_DOT <= 1/8 of the ratio either dropped cross product gives."""
    rng = np.random.default_rng(seed)
    worst, least = 0.0, np.inf
    for K in K_VALUES:
        worst = max(worst, _dot_ratio(rng, K, rows))
        least = min(least, _dot_ratio(rng, K, rows, 'lohi'), _dot_ratio(rng, K, rows, 'hilo'))
    assert 8 * C_DOT <= least, (C_DOT, least)
    return 4 * worst, least
