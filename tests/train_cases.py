"""Cases, float64 references and tolerances for the depthwise and BatchNorm training kernels of csrc/yk_train.hip and for its small calls
(max pool, upsample adjoint, bias add, column sum, axpy, Adam), shared by tests/test_train_cases.py (CPU: the references and the case
tables checked on their own), tests/test_gpu_train_edges.py and tests/test_gpu_train_small.py (the kernels).  Nothing here touches a GPU.

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
# The 16-byte rule of the host wrappers (vec4_ok in yk_train.hip): C = 4, one image of 5 x 6, stride 1 and stride 2 (asymmetric "same" padding
# along the width); called with every tensor on a 16-byte boundary and once per tensor 4 bytes past one.  BatchNorm: the 30 rows of the first.
ALIGN_DW_CASES = [(1, 5, 6, 4, 1, 1, 1), (1, 5, 6, 4, 2, 1, 0)]
ALIGN_BN_CASE = (30, 4) + ACTS[1]


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


# ------------------------------------------------------------------------------------------------ the small calls
# yk_maxpool2_{fwd,bwd}_f32, yk_upsample2x_bwd_f32, yk_bias_add_f32, yk_colsum_f32, yk_axpy_f32, yk_adam_f32 (tests/test_gpu_train_small.py).
# yk_train.o is built without FMA contraction, so every written operation of these kernels is ONE IEEE rounding: beside the float64
# reference each bitwise rule has a numpy float32 restatement, one operation per statement in the kernel's written order.
U = 2.0 ** -24                    # unit roundoff of float32
TINY = 2.0 ** -150                # half the spacing of the float32 subnormals: the most one rounding is off by below 2^-126


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# (B, Hi, Wi, C, stride): MaxPool2D 2x2, padding 'same' (bottom / right, -inf).  Odd and even sizes, a single row, a single column, one
# window that is all padding but its first tap (1 x 1), C = 1, odd C; 13 x 21 x 16 at stride 1 is several workgroups.
POOL_CASES = ([(2, hi, wi, c, s) for (hi, wi) in ((13, 20), (13, 21), (1, 7), (7, 1)) for s in (1, 2) for c in (1, 3, 16)]
              + [(2, 2, 2, 3, 1), (2, 2, 2, 3, 2), (1, 1, 1, 1, 1), (1, 1, 1, 1, 2)])
POOL_KINDS = ('a', 'b', 'c')      # a: {0, 6} (what ReLU6 leaves: ties everywhere), b: integers -3..3 with one plane of -inf, c: normal
POOL_TIE_SHARE = 0.30


def pool_geom(case):
    B, Hi, Wi, C, stride = case
    return B, Hi, Wi, C, -(-Hi // stride), -(-Wi // stride), stride


def pool_taps(case, x):
    """[4][B][Ho][Wo][C] float64: tap t = 2 * dy + dx of every window, -inf outside the input (bottom / right)."""
    B, Hi, Wi, C, Ho, Wo, s = pool_geom(case)
    xp = np.full((B, (Ho - 1) * s + 2, (Wo - 1) * s + 2, C), -np.inf)
    xp[:, :Hi, :Wi] = x
    return np.stack([xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s] for dy in (0, 1) for dx in (0, 1)])


def pool_ref(case, x):
    """(y float64, arg uint8): the maximum of each window and the FIRST tap that holds it (np.argmax returns the first; a window of
    -inf alone gives tap 0)."""
    taps = pool_taps(case, x)
    return taps.max(0), taps.argmax(0).astype(np.uint8)


def pool_bwd_ref(case, arg, dy):
    """dx float64: every dy goes to the one input its window's arg names; an input named by several windows sums them."""
    B, Hi, Wi, C, Ho, Wo, s = pool_geom(case)
    b, oy, ox, c = np.indices((B, Ho, Wo, C))
    iy, ix = oy * s + (arg >> 1), ox * s + (arg & 1)
    assert (iy < Hi).all() and (ix < Wi).all()                     # no window names a padding tap
    dx = np.zeros((B, Hi, Wi, C))
    np.add.at(dx, (b, iy, ix, c), np.asarray(dy, np.float64))
    return dx


def pool_max_wins(case):
    """How many windows one input can win: 4 at stride 1 on an input of at least 2 x 2, 2 on a single row or column, 1 otherwise."""
    B, Hi, Wi, C, stride = case
    return min(2, Hi) * min(2, Wi) if stride == 1 else 1


def pool_properties(case, x):
    """From the reference alone: the share of windows whose maximum is held by more than one tap, the largest number of windows one
    input wins, and whether some window is -inf on every tap."""
    taps = pool_taps(case, x)
    y, arg = pool_ref(case, x)
    wins = pool_bwd_ref(case, arg, np.ones(arg.shape))
    return dict(tie_share=float(((taps == y).sum(0) > 1).mean()), most_wins=int(wins.max()), all_inf=bool(np.isneginf(y).any()))


def pool_tie_floor(case):
    """The share of tied windows data (a) must reach.  A window with one valid tap cannot tie: the 1 x 1 input has no other window and is
    exempt; everywhere else the floor is the 30 % the tests ask for."""
    return 0.0 if case[1:3] == (1, 1) else POOL_TIE_SHARE


def pool_inputs(case, kind):
    """x [B][Hi][Wi][C] and dy [B][Ho][Wo][C] as float32.  Data (a) is drawn again (next seed) until the reference shows the properties
    the tests need of it - ties in 30 % of the windows and, at stride 1, an input that wins as many windows as one can; on a handful of
    windows a single draw misses them about as often as not.  The choice never looks at a kernel's output."""
    B, Hi, Wi, C, Ho, Wo, s = pool_geom(case)
    for seed in range(200):
        rng = np.random.default_rng(1000 * seed + 31 * sum(case) + ord(kind))
        if kind == 'a':
            x = rng.integers(0, 2, (B, Hi, Wi, C)) * 6.0
        elif kind == 'b':
            x = rng.integers(-3, 4, (B, Hi, Wi, C)).astype(np.float64)
            x[0, :, :, 0] = -np.inf
        else:
            x = rng.normal(size=(B, Hi, Wi, C))
        dy = rng.normal(size=(B, Ho, Wo, C)) if kind == 'c' else rng.integers(-3, 4, (B, Ho, Wo, C))
        if kind != 'a':
            break
        pr = pool_properties(case, x)
        if pr['tie_share'] >= pool_tie_floor(case) and pr['most_wins'] == pool_max_wins(case):
            break
    else:
        raise AssertionError(('no draw with the properties', case))
    return x.astype(np.float32), dy.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pool_problem(case, kind):
    """Inputs and references of one case, computed once and shared (read-only).  dx: the float64 gradient; dx_abs: the same sum over
    |dy|, which bounds every partial sum (exactness on integer dy, the rounding bound on normal dy)."""
    x, dy = pool_inputs(case, kind)
    y, arg = pool_ref(case, x)
    out = dict(x=x, dy=dy, y=y, arg=arg, dx=pool_bwd_ref(case, arg, dy), dx_abs=pool_bwd_ref(case, arg, np.abs(dy)))
    out['abs_sum'] = float(out['dx_abs'].max())
    return _freeze(out)


# (B, H, W, C) of dx; dy is [B][2H][2W][C]
UPSAMPLE_CASES = [(2, 13, 20, 16), (1, 1, 1, 1), (3, 5, 7, 3)]


def upsample_bwd_f32(dy, case):
    """The kernel's written order in float32: dy[r0] + dy[r0 + C] + dy[r0 + rs] + dy[r0 + rs + C], one rounding per +."""
    B, H, W, C = case
    t = np.asarray(dy, np.float32).reshape(B, H, 2, W, 2, C)
    s = t[:, :, 0, :, 0] + t[:, :, 0, :, 1]
    s = s + t[:, :, 1, :, 0]
    s = s + t[:, :, 1, :, 1]
    assert s.dtype == np.float32
    return s


@functools.lru_cache(maxsize=None)
def upsample_problem(case):
    B, H, W, C = case
    rng = np.random.default_rng(sum(case))
    dy = rng.normal(size=(B, 2 * H, 2 * W, C)).astype(np.float32)
    t = dy.astype(np.float64).reshape(B, H, 2, W, 2, C)
    return _freeze(dict(dy=dy, dx32=upsample_bwd_f32(dy, case), dx64=t.sum((2, 4)), dx_abs=np.abs(t).sum((2, 4))))


def colsum_chunking(M, C):
    """bn_chunking() as yk_colsum_f32 uses it: (rows per chunk, chunks, rows in the last chunk).  A label, like the planners above."""
    chunks, rpc, RL = bn_chunking(M, C)
    return rpc, chunks, M - (chunks - 1) * rpc


# (M, C): both sides of each lane_split boundary (16 | 17, 32 | 33), one column, several channel groups with a cut last one (75, 130);
# per C fewer rows than row lanes (1, RL - 1), exactly RL and RL + 1; (8193, 16): 257 chunks, the last of ONE row; (4097, 75): 342
# chunks of 12 rows, the last of 5 - both more chunks than the 64 lanes of colsum_from_stats_kernel's wave take in one pass.
COLSUM_CASES = ([(m, c) for c in (1, 16, 17, 32, 33, 75, 130) for r in (256 >> lane_split(c),) for m in (1, r - 1, r, r + 1)]
                + [(8193, 16), (4097, 75)])


@functools.lru_cache(maxsize=None)
def colsum_problem(case, lattice):
    """x [M][C] float32 (integers -3..3, or normal with a scale and an offset per column), the float64 column sums and sums of |x|."""
    M, C = case
    rng = np.random.default_rng(7 + M + 100000 * C + lattice)
    x = (rng.integers(-3, 4, (M, C)) if lattice else rng.normal(size=(M, C)) * rng.uniform(0.5, 3, C) + rng.normal(size=C)).astype(np.float32)
    return _freeze(dict(x=x, sum=x.astype(np.float64).sum(0), abs_sum=np.abs(x.astype(np.float64)).sum(0)))


def colsum_bound(M, ref, abs_sum):
    """One float32 rounding of a float64 sum, plus what reordering a float64 sum of M terms can move it."""
    return U * np.abs(ref) + M * 2.0 ** -53 * abs_sum


BIAS_CASES = [(1, 1), (255, 1), (37, 7), (520, 16), (3, 257)]                 # (M, C)
AXPY_NS = [1, 255, 256, 257, 10007]
AXPY_AS = [-0.25, 0.1]                                                        # an exact product, and one that rounds
AXPY_CASES = [(n, a) for n in AXPY_NS for a in AXPY_AS]


def bias_add_f32(y, bias):
    out = np.asarray(y, np.float32) + np.asarray(bias, np.float32)[None, :]
    assert out.dtype == np.float32
    return out


def axpy_f32(a, x, y):
    """y + a * x as the kernel writes it: the product rounded first, then the sum."""
    prod = np.float32(a) * np.asarray(x, np.float32)
    out = np.asarray(y, np.float32) + prod
    assert prod.dtype == np.float32 and out.dtype == np.float32
    return out


@functools.lru_cache(maxsize=None)
def bias_problem(case):
    M, C = case
    rng = np.random.default_rng(M + 1000 * C)
    y, bias = rng.normal(size=(M, C)).astype(np.float32), rng.normal(size=C).astype(np.float32)
    return _freeze(dict(y=y, bias=bias, out32=bias_add_f32(y, bias), out64=y.astype(np.float64) + bias.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def axpy_problem(case):
    n, a = case
    rng = np.random.default_rng(n)
    x, y = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    a64 = float(np.float32(a))
    return _freeze(dict(x=x, y=y, out32=axpy_f32(a, x, y), out64=y.astype(np.float64) + a64 * x.astype(np.float64),
                        abs64=np.abs(y.astype(np.float64)) + np.abs(a64 * x.astype(np.float64))))


# ------------------------------------------------------------------------------------------------ Adam
# The Trainer's constants (train.py: apply_update), as the float32 values the C call receives
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (float(np.float32(v)) for v in (5e-4, 0.9, 0.999, 1e-7))
ADAM_NS = [1, 255, 256, 257, 10007]
ADAM_ITERATIONS = [0, 1, 9, 999, 100000]
ADAM_GSCALES = [1.0, 0.125, float(np.float32(1.0 / 3.0))]
ADAM_DECAYS = [0.0, float(np.float32(0.01))]
# (n, iterations, grad_scale, decay, warm): every (iterations, grad_scale, decay), with the lengths and the two starting states (m = v = 0 |
# a previous state) cycling through them so that every (n, warm) pair occurs (tests/test_train_cases.py asserts it)
ADAM_CASES = [(ADAM_NS[i % 5], it, gs, dc, bool(i % 2))
              for i, (it, gs, dc) in enumerate((it, gs, dc) for it in ADAM_ITERATIONS for gs in ADAM_GSCALES for dc in ADAM_DECAYS)]
# Four consecutive steps against float64: (n, first iteration, grad_scale, decay, warm).  grad_scale is a power of two here: g * grad_scale
# is then exact and m and v each take the three roundings their bound counts (two products, one sum).  With 1/3 the rounded gradient
# enters v twice and three roundings no longer bound it; that value is held bit for bit by the single-step cases instead.
ADAM_RUN_CASES = [(10007, 0, 1.0, float(np.float32(0.01)), False), (257, 0, 0.125, 0.0, False), (10007, 999, 0.125, float(np.float32(0.01)), True),
                  (255, 100000, 1.0, 0.0, True)]
ADAM_STEPS = 4


def adam_lr_t(lr, decay, iterations, b1, b2):
    """lr_t in double exactly as yk_adam_f32 writes it (the arguments are the float32 values widened), then cast to float32.
    math.pow and math.sqrt are the C library's, as in the host code."""
    import math
    t = float(iterations) + 1.0
    lr_t = lr / (1.0 + decay * float(iterations)) * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t))
    return np.float32(lr_t)


def adam_step_f32(p, g, m, v, iterations, gscale, decay, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """adam_kernel in numpy float32, one rounding per statement, with C's left-to-right grouping of (1.f - b2) * gi * gi and of
    lr_t * mi / (...).  Needs a correctly rounded float32 divide and square root, which numpy's are.  Returns (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    lr_t, b1, b2, eps = adam_lr_t(lr, decay, iterations, b1, b2), f(b1), f(b2), f(eps)
    with np.errstate(under='ignore'):
        gi = g * f(gscale)
        c1 = f(1) - b1
        mi = b1 * m
        t1 = c1 * gi
        mi = mi + t1
        c2 = f(1) - b2
        vi = b2 * v
        t2 = c2 * gi
        t2 = t2 * gi
        vi = vi + t2
        num = lr_t * mi
        den = np.sqrt(vi)
        den = den + eps
        upd = num / den
        pn = p - upd
    assert all(a.dtype == f for a in (gi, mi, vi, upd, pn))
    return pn, mi, vi


class ScaledAdamRef:
    """oracle.train_ref.AdamRef (Keras Adam in float64) with the gradient scale of yk_adam_f32 in front, on one flat tensor, starting at
    a given iteration and state.  Also the sums of |terms| the per-step bounds scale with."""

    def __init__(self, iterations, gscale, decay, m, v):
        from oracle.train_ref import AdamRef
        self.ref = AdamRef(ADAM_LR, decay=decay, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS)
        self.ref.it, self.gscale = int(iterations), float(gscale)
        self.ref.m['p'], self.ref.v['p'] = np.asarray(m, np.float64), np.asarray(v, np.float64)

    def step(self, p, g):
        """One update; returns (p, m, v, bounds) with bounds = this step's rounding allowance for (p, m, v):
        2^-23 (|p| + 4 |update|), 3 * 2^-24 (|b1 m| + |(1 - b1) g|), 3 * 2^-24 (|b2 v| + |(1 - b2) g^2|).  The last two are three
        roundings each; a rounding in the subnormal range (the square of a gradient of 1e-20) is off by up to TINY = 2^-150 whatever
        the value, so each of the three adds that."""
        g = np.asarray(g, np.float64) * self.gscale
        m0, v0, p0 = self.ref.m['p'], self.ref.v['p'], np.asarray(p, np.float64)
        pn = self.ref.apply({'p': p0}, {'p': g})['p']
        bounds = (2 * U * (np.abs(pn) + 4 * np.abs(pn - p0)), 3 * U * (np.abs(ADAM_B1 * m0) + np.abs((1 - ADAM_B1) * g)) + 3 * TINY,
                  3 * U * (np.abs(ADAM_B2 * v0) + np.abs((1 - ADAM_B2) * g * g)) + 3 * TINY)
        return pn, self.ref.m['p'], self.ref.v['p'], bounds


def adam_gradients(rng, n):
    """normal x 10^U{-4..1} as tests/test_gpu_train.py draws them; 5 % exact zeros and a few +-1e-20 (whose squares are subnormal)."""
    g = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    k = min(n, 6)
    g[rng.choice(n, k, replace=False)] = np.where(np.arange(k) % 2, -1e-20, 1e-20).astype(np.float32)
    return g


def adam_state(rng, n, warm):
    """p, m, v float32.  warm: m and v as a few earlier steps leave them (v >= 0), with exact zeros kept where the tests need a fresh v."""
    p = rng.normal(size=n).astype(np.float32)
    if not warm:
        return p, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for it in range(3):
        _, m, v = adam_step_f32(p, adam_gradients(rng, n), m, v, it, 1.0, 0.0)
    return p, m, v


@functools.lru_cache(maxsize=None)
def adam_problem(case):
    """One step: inputs and the float32 restatement's (p, m, v)."""
    n, iterations, gscale, decay, warm = case
    rng = np.random.default_rng(n + 13 * iterations + int(1000 * gscale) + int(warm))
    p, m, v = adam_state(rng, n, warm)
    g = adam_gradients(rng, n)
    pn, mn, vn = adam_step_f32(p, g, m, v, iterations, gscale, decay)
    return _freeze(dict(p=p, g=g, m=m, v=v, p32=pn, m32=mn, v32=vn))


@functools.lru_cache(maxsize=None)
def adam_run_problem(case):
    """ADAM_STEPS consecutive steps: the gradients, and per step the float64 (p, m, v) with the ACCUMULATED bounds, and the float32
    restatement's (p, m, v)."""
    n, it0, gscale, decay, warm = case
    rng = np.random.default_rng(5 + n + it0)
    p0, m0, v0 = adam_state(rng, n, warm)
    ref = ScaledAdamRef(it0, gscale, decay, m0, v0)
    p64, acc, steps = p0.astype(np.float64), [0.0, 0.0, 0.0], []
    p32, m32, v32 = p0, m0, v0
    for k in range(ADAM_STEPS):
        g = adam_gradients(rng, n)
        p64, m64, v64, b = ref.step(p64, g)
        acc = [a + x for a, x in zip(acc, b)]
        p32, m32, v32 = adam_step_f32(p32, g, m32, v32, it0 + k, gscale, decay)
        steps.append(_freeze(dict(g=g, p64=p64, m64=m64, v64=v64, bp=acc[0], bm=acc[1], bv=acc[2], p32=p32, m32=m32, v32=v32)))
    return dict(p=p0, m=m0, v=v0, steps=steps)
