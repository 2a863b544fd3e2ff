"""Cases, float64 references and tolerances for the depthwise and BatchNorm training kernels of csrc/yk_train.hip, shared by
tests/test_train_cases.py (CPU: the references and the case tables checked on their own) and tests/test_gpu_train_edges.py (the kernels).
Nothing here touches a GPU.

The host wrappers of yk_train.hip choose among several kernels by shape.  The planners below are Python copies of those choices, used
ONLY to label the cases (which path, which edge), so that tests/test_train_cases.py can assert that every path stays covered."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from k210_yolo_framework_amd import netspec as ns

EPS, MOMENTUM = 1e-3, 0.99
KINK_BAND = 1e-4                  # |pre - kink| <= this: fp32 and float64 may gate the element differently
KINK_CAP = 1e-3                   # at most this share of a column's rows may be ambiguous (a condition on the data, not a measurement)
GRAD_TOL = 2e-4                   # the project's gradient tolerance for these kernels (tests/test_gpu_train.py)


# ------------------------------------------------------------------------------------------------ host planners (labels only)
def lane_split(C):
    """lane_split(): log2 of the channel lanes per workgroup."""
    return 4 if C <= 16 else (5 if C <= 32 else 6)


def dww_planning(B, C, Ho, Wo):
    """dww_planning(): the launch geometry of dw_bwd_weight_kernel."""
    cwl = lane_split(C)
    RL = 256 >> cwl
    groups = (C + (1 << cwl) - 1) >> cwl
    segs = (1024 * RL + B * Ho * groups - 1) // (B * Ho * groups)
    segs = max(1, min(segs, min(8, Wo // 8)))
    wseg = (Wo + segs - 1) // segs
    segs = (Wo + wseg - 1) // wseg
    rows = B * Ho * segs
    rpc = ((rows + 2047) // 2048 + RL - 1) // RL * RL
    return dict(cwl=cwl, RL=RL, groups=groups, segs=segs, wseg=wseg, last_seg=Wo - (segs - 1) * wseg, rows=rows, rpc=rpc,
                chunks=(rows + rpc - 1) // rpc, cut_group=C % (1 << cwl) != 0, V=4 if C % 4 == 0 else 1)


def bn_chunking(M, C):
    """bn_chunking(): (chunks, rows per chunk, row lanes) of bn_colreduce_kernel."""
    RL = 256 >> lane_split(C)
    rpc = max(((M + 511) // 512 + RL - 1) // RL * RL, RL)
    return (M + rpc - 1) // rpc, rpc, RL


def bn_cols_ok(M, C):
    """bn_cols_ok(), for 16-byte aligned tensors: one workgroup per 8 channels does the whole chain."""
    return M <= 3 * 512 and C % 4 == 0


def bn_v4_plan(M, C):
    """The v4 branch of yk_bn_train_bwd_f32 (aligned tensors): None, or the geometry of bn_colreduce_bwd_v4_kernel."""
    if not (C % 4 == 0 and 50000 <= M < (1 << 31)):
        return None
    CV = C // 4
    CW = min(CV, 256)
    RL = 256 // CW
    groups = (CV + CW - 1) // CW
    chunks = min(2048, (M + RL * 8 - 1) // (RL * 8))
    rpc = ((M + chunks - 1) // chunks + RL - 1) // RL * RL
    return dict(CW=CW, RL=RL, groups=groups, rpc=rpc, chunks=(M + rpc - 1) // rpc)


def bn_bwd_path(M, C):
    """Which reduction yk_bn_train_bwd_f32 launches for aligned [M][C] tensors: 'cols', 'v4' or 'scalar'."""
    if bn_cols_ok(M, C):
        return 'cols'
    return 'v4' if bn_v4_plan(M, C) else 'scalar'


def bn_bwd_chain(M, C):
    """The longest sequential fp32 addition chain behind one dbeta / dgamma of yk_bn_train_bwd_f32: rows per thread, the serial sum over
    the row lanes, the chunks one lane of the finishing wave walks, and its 6-step tree (cols: 3 rows, then a 9-step tree over 512 lanes)."""
    path = bn_bwd_path(M, C)
    if path == 'cols':
        return 3 + 9
    if path == 'v4':
        p = bn_v4_plan(M, C)
        chunks, rpc, RL = p['chunks'], p['rpc'], p['RL']
    else:
        chunks, rpc, RL = bn_chunking(M, C)
    return rpc // RL + RL + (chunks + 63) // 64 + 6


# ------------------------------------------------------------------------------------------------ depthwise 3x3
# (B, Hi, Wi, C, stride, pad_t, pad_l); bottom / right padding as TF "same".  Each case is the smallest shape that reaches the edge it
# names (tests/test_train_cases.py checks the labels through dww_planning).
DW_CASES = [
    (2, 5, 7, 3, 1, 1, 1),        # V=1 (C % 4 != 0), 16 channel lanes for 3 channels, Wo < 8: one segment per row
    (1, 3, 3, 4, 1, 1, 1),        # every pixel on a border
    (2, 6, 19, 20, 1, 1, 1),      # 32 channel lanes with a cut group, 2 segments of 10: a ragged last segment of 9
    (2, 9, 39, 72, 2, 1, 1),      # stride 2, Wo = 20 -> 2 segments: the register window restarts inside a row
    (2, 10, 40, 32, 2, 0, 0),     # stride 2, asymmetric "same" padding (even input), 2 segments
    (1, 4, 70, 130, 1, 1, 1),     # V=1, 3 channel groups with the last cut to 2, 8 segments of 9, the last of 7
    (2, 8, 132, 16, 2, 0, 0),     # 16 channel lanes, Wo = 66 -> 8 segments with stride 2
    (7, 1171, 9, 40, 1, 1, 1),    # 4 row lanes and 8197 rows > 2048 * 4 -> rows per chunk (8) > row lanes, ragged last chunk of 5.  (Rows per
                                  # chunk exceed the row lanes only past 2048 * RL (image row, segment) units, and the planner spends segments
                                  # only below 1024 * RL of them: so this edge needs B * Ho > 8192 at C > 32, whatever Wo.)
]
# yk_im2col3x3_f32 / yk_col2im3x3_f32 at the asymmetric-padding geometries: C = 4 takes the float4 kernel, C = 3 the scalar one
IM2COL_CASES = [(2, 10, 40, 4, 2, 0, 0), (2, 10, 40, 3, 2, 0, 0), (2, 8, 132, 4, 2, 0, 0), (2, 8, 132, 3, 2, 0, 0)]


def dw_geom(case):
    """(B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l) as the C entry points take it, and (pad_b, pad_r)."""
    B, Hi, Wi, C, stride, pad_t, pad_l = case
    Ho, Wo = -(-Hi // stride), -(-Wi // stride)
    th, tw = max((Ho - 1) * stride + 3 - Hi, 0), max((Wo - 1) * stride + 3 - Wi, 0)
    assert (pad_t, pad_l) == (th // 2, tw // 2), case               # the table's top / left padding is TF "same"'s
    pad_b, pad_r = th - pad_t, tw - pad_l
    assert Ho == (Hi + pad_t + pad_b - 3) // stride + 1 and Wo == (Wi + pad_l + pad_r - 3) // stride + 1
    return (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r)


def dw_inputs(case, lattice):
    """x [B][Hi][Wi][C], w [3][3][C], dy [B][Ho][Wo][C] as float32: integers -3..3 (fp32 sums of them are exact in any order) or normal."""
    (B, Hi, Wi, C, Ho, Wo, *_), _ = dw_geom(case)
    rng = np.random.default_rng(17 + sum(case) + 1000 * lattice)
    draw = (lambda s: rng.integers(-3, 4, s)) if lattice else (lambda s: rng.normal(size=s))
    return draw((B, Hi, Wi, C)).astype(np.float32), draw((3, 3, C)).astype(np.float32), draw((B, Ho, Wo, C)).astype(np.float32)


def dw_ref(case, x, w, dy):
    """float64 forward, data gradient and weight gradient through torch's conv2d with explicit padding: (y, dx, dw) in NHWC / [3][3][C]."""
    (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r) = dw_geom(case)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (pad_l, pad_r, pad_t, pad_b)), wt.permute(2, 0, 1)[:, None], stride=stride, groups=C)
    assert tuple(yt.shape) == (B, C, Ho, Wo)
    yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    return yt.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy(), wt.grad.numpy()


@functools.lru_cache(maxsize=None)
def dw_problem(case, lattice):
    """Inputs and reference of one case, computed once and shared (read-only arrays).  For the lattice data also `abs_sum`: the largest sum
    of |terms| behind any output, which bounds every partial sum a kernel can form."""
    x, w, dy = dw_inputs(case, lattice)
    y, dx, dw = dw_ref(case, x, w, dy)
    out = dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw)
    if lattice:
        out['abs_sum'] = max(float(np.abs(a).max()) for a in dw_ref(case, np.abs(x), np.abs(w), np.abs(dy)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def im2col_ref(case, x):
    """col [B*Ho*Wo][9*C], k = (ky*3+kx)*C + c."""
    (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r) = dw_geom(case)
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad_t, pad_b), (pad_l, pad_r), (0, 0)))
    taps = [xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] for ky in range(3) for kx in range(3)]
    return np.stack(taps, 3).reshape(B * Ho * Wo, 9 * C)


def col2im_ref(case, col):
    """The adjoint of im2col_ref: dx [B][Hi][Wi][C], overlaps summed."""
    (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r) = dw_geom(case)
    dxp = np.zeros((B, Hi + pad_t + pad_b, Wi + pad_l + pad_r, C))
    c5 = col.astype(np.float64).reshape(B, Ho, Wo, 9, C)
    for t in range(9):
        ky, kx = divmod(t, 3)
        dxp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += c5[:, :, :, t]
    return dxp[:, pad_t:pad_t + Hi, pad_l:pad_l + Wi]


# ------------------------------------------------------------------------------------------------ BatchNorm (training) + activation
ACTS = [(ns.ACT_RELU, 0.0), (ns.ACT_RELU6, 6.0), (ns.ACT_LEAKY, 0.1), (ns.ACT_NONE, 0.0)]
_COLS_MC = [(m, 12) for m in (1, 2, 511, 512, 513, 1024, 1025, 1536)] + [(513, 4), (513, 24)]
_SCALAR_MC = [(1537, 12), (1537, 8), (300, 1), (700, 3), (900, 17), (2000, 33), (4097, 65), (49999, 24)]
_V4_MC = [(50000, 16), (50000, 24), (50001, 100), (50000, 1024), (50000, 1028)]         # the last one: two channel groups
# (M, C, act, alpha): the activation cycles inside each path, so each path sees relu, relu6, leaky and none
BN_CASES = [(m, c) + ACTS[i % 4] for mc in (_COLS_MC, _SCALAR_MC, _V4_MC) for i, (m, c) in enumerate(mc)]
# the two widest cases are generated on the GPU and compared on these columns only (BatchNorm is per column: a subset is exact)
BN_WIDE = {(50000, 1024): list(range(8)) + list(range(1008, 1024)), (50000, 1028): list(range(8)) + list(range(1012, 1028))}
BN_HOST_CASES = [c for c in BN_CASES if c[:2] not in BN_WIDE]
# Seed of each host-generated case: 0 unless that draw breaks the kink cap, then the first seed that keeps it.  Below 1000 rows the cap
# allows no ambiguous element at all, and a draw of a few thousand elements holds one about as often as not.  The choice looks at the
# float64 reference alone (tests/test_train_cases.py asserts the cap for every case), never at a kernel's output.
BN_SEEDS = {(511, 12): 1, (900, 17): 3}
# the fused forwards: (M, N, K, residual) for yk_gemm_bn_fwd_f32 - bn_fwd_cols_kernel<3> at its row edges and the first M that misses it
GEMM_BN_CASES = [(512, 8, 16, False), (513, 12, 20, True), (1536, 12, 36, True), (1537, 12, 36, False)]
DW_BN_CASES = [DW_CASES[2], DW_CASES[4]]


def bn_inputs(M, C, seed):
    """z [M][C], gamma, beta, dy as float32: the columns differ in scale and offset, as in tests/test_gpu_train.py."""
    rng = np.random.default_rng(seed)
    z = (rng.normal(size=(M, C)) * rng.uniform(0.5, 3, C) + rng.normal(size=C) * 2).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 3, C).astype(np.float32), rng.normal(size=C).astype(np.float32)
    return z, gamma, beta, rng.normal(size=(M, C)).astype(np.float32)


def act_fwd(pre, act, alpha):
    if act == ns.ACT_RELU:
        return np.maximum(pre, 0.0)
    if act == ns.ACT_RELU6:
        return np.clip(pre, 0.0, 6.0)
    if act == ns.ACT_LEAKY:
        return np.where(pre >= 0, pre, pre * alpha)
    return pre


def act_gate(pre, act, alpha):
    """The derivative at the pre-activation value, with t_act_grad's choice at the kinks themselves."""
    if act == ns.ACT_RELU:
        return (pre > 0).astype(np.float64)
    if act == ns.ACT_RELU6:
        return ((pre > 0) & (pre < 6)).astype(np.float64)
    if act == ns.ACT_LEAKY:
        return np.where(pre >= 0, 1.0, float(alpha))
    return np.ones_like(pre)


def bn_backward(ref, dy, gate):
    """The backward formulas of yk_train.hip for a given gate: g = dy * act', dbeta = sum g, dgamma = sum g * xhat,
    dz = gamma * invstd * (g - dbeta / M - xhat * dgamma / M).  Also S_dbeta / S_dgamma, the sums of |terms| the tolerance scales with."""
    M = dy.shape[0]
    g = dy * gate
    dbeta, dgamma = g.sum(0), (g * ref['xhat']).sum(0)
    dz = ref['gamma'] * ref['invstd'] * (g - dbeta / M - ref['xhat'] * dgamma / M)
    return dict(dbeta=dbeta, dgamma=dgamma, dz=dz, S_dbeta=np.abs(g).sum(0), S_dgamma=np.abs(g * ref['xhat']).sum(0))


def bn_ref(z, gamma, beta, dy, act, alpha, cols=None, res=None):
    """BatchNormalization(training) + activation in numpy float64, forward and backward, from the formulas above t_act in yk_train.hip:
    batch mean and biased variance over the M rows, y = act(gamma * (z - mean) * invstd + beta) (+ res); the moving statistics start at
    (0, 1) and take the batch mean and the UNBIASED variance (the biased one for a single row) with momentum 0.99.
    cols: compute these columns only (z, dy, res then hold just these columns; gamma and beta are full length)."""
    z, dy = np.asarray(z, np.float64), (None if dy is None else np.asarray(dy, np.float64))
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    if cols is not None:
        gamma, beta = gamma[cols], beta[cols]
    M = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + EPS)
    xhat = (z - mean) * invstd
    pre = gamma * xhat + beta
    y = act_fwd(pre, act, alpha)
    if res is not None:
        y = np.asarray(res, np.float64) + y
    uvar = var * M / (M - 1.0) if M > 1 else var
    ref = dict(M=M, mean=mean, var=var, invstd=invstd, xhat=xhat, pre=pre, y=y, gamma=gamma, beta=beta, act=act, alpha=alpha,
               moving_mean=(1 - MOMENTUM) * mean, moving_var=MOMENTUM + (1 - MOMENTUM) * uvar)
    if dy is not None:
        ref.update(bn_backward(ref, dy, act_gate(pre, act, alpha)))
    return ref


def kink_slack(ref, dy):
    """The kink rule.  An element is ambiguous when its float64 pre-activation lies within KINK_BAND of a kink (0 for relu and leaky, 0 and
    6 for relu6): fp32 may gate it the other way, which changes that element's g by at most |dy| * D (D = 1 for relu / relu6, 1 - alpha
    for leaky).  Returns (ambiguous mask, slack_dbeta[c] = sum_amb |dy| D, slack_dgamma[c] = sum_amb |dy xhat| D, dz_widen [M][C]): the
    column sums may differ from the reference by the slacks, and dz outside the mask by
    |gamma invstd| (slack_dbeta + |xhat| slack_dgamma) / M on top of its own tolerance."""
    pre, act, dy = ref['pre'], ref['act'], np.asarray(dy, np.float64)
    if act == ns.ACT_NONE:
        amb, D = np.zeros(pre.shape, bool), 0.0
    elif act == ns.ACT_RELU6:
        amb, D = (np.abs(pre) <= KINK_BAND) | (np.abs(pre - 6) <= KINK_BAND), 1.0
    else:
        amb, D = np.abs(pre) <= KINK_BAND, (1.0 if act == ns.ACT_RELU else 1.0 - float(ref['alpha']))
    s_db = (np.abs(dy) * amb).sum(0) * D
    s_dg = (np.abs(dy * ref['xhat']) * amb).sum(0) * D
    widen = np.abs(ref['gamma'] * ref['invstd']) * (s_db + np.abs(ref['xhat']) * s_dg) / ref['M']
    return amb, s_db, s_dg, widen


def kink_cap_holds(amb):
    """No column may have more than KINK_CAP of its rows ambiguous."""
    return bool((amb.sum(0) <= KINK_CAP * amb.shape[0]).all())


@functools.lru_cache(maxsize=None)
def bn_problem(case):
    """Inputs, float64 reference and kink slack of one host-generated case, computed once and shared (read-only arrays)."""
    M, C, act, alpha = case
    z, gamma, beta, dy = bn_inputs(M, C, BN_SEEDS.get((M, C), 0))
    ref = bn_ref(z, gamma, beta, dy, act, alpha)
    amb, s_db, s_dg, widen = kink_slack(ref, dy)
    out = dict(z=z, gamma=gamma, beta=beta, dy=dy, ref=ref, amb=amb, slack_dbeta=s_db, slack_dgamma=s_dg, dz_widen=widen)
    for a in list(out.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
