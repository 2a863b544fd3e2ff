"""Cases, float64 references and labels for the fp32 MFMA GEMM family (csrc/yk_gemm_f32.h, csrc/yk_train.hip: yk_gemm_f32, yk_gemm_f32_grouped,
yk_gemm_bn_fwd_f32) and the implicit-GEMM 3x3 convolutions (yk_conv3x3_bn_fwd_f32, yk_conv3x3_bwd_weight_f32, yk_conv3x3_bwd_data_f32), shared by
tests/test_gemm_cases.py (CPU: the tables and references checked on their own) and tests/test_gpu_gemm_edges.py (the kernels).
Nothing here touches a GPU.

The host wrappers choose among many code paths by shape, leading dimension and address.  The planners below are Python copies of those
choices, used ONLY to label the cases (layout, loader, epilogue, K slices, finishing pass), so that tests/test_gemm_cases.py can assert
that every path stays covered.

Two kinds of data.  LATTICE: integers -3..3 for A, B and C0 with (alpha, beta) in {(1, 0), (0.5, 2)}: every partial sum a kernel can form
is an integer below 9 K + 6 <= 2^24, so the fp32 result is exact in ANY summation order and must equal the float64 reference bit for bit.
NORMAL: standard normal data at K <= 320, held to the any-order fp32 summation bound gamma(K + 4) (|alpha| |A| |B| + |beta| |C0|) per
element, gamma(n) = n u / (1 - n u), u = 2^-24: what a product in a lower precision than fp32 misses by more than a factor of ten."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

NAN_BITS = 0x7FC0F00D             # the one NaN pattern of every gap, guard and beta == 0 output (compared as int32)
SPARE = 4                         # floats behind every operand; an operand may start 1 float into its buffer (off the 16-byte grid)
U = 2.0 ** -24
LAYOUTS = {'NT': (0, 1), 'NN': (0, 0), 'TN': (1, 0), 'TT': (1, 1)}          # (transA, transB): forward, data gradient, weight gradient, old kernel
ALPHA_BETA = [(1.0, 0.0), (0.5, 2.0)]
NORMAL_K_MAX = 320
YK_GROUP_MAX = 36
MAX_CASE_BYTES = 8 << 20          # "a few MB": host floats of one case (a group of 73 problems counts as one case)


def gamma(n):
    return n * U / (1.0 - n * U)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _draw(rng, shape, lattice):
    return (rng.integers(-3, 4, shape) if lattice else rng.normal(size=shape)).astype(np.float32)


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ host planners (labels only)
def gemm_splits(M, N, K):
    """gemm_splits(): K slices of a standalone problem (counted in k-steps of 16, whatever the tile walks)."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    nk = (K + 15) // 16
    s = 1
    if tiles < 512 and nk >= 8:
        s = max(1, min((1024 + tiles - 1) // tiles, nk // 4))
        s = min(s, 512)
    return s


def k_slices(K, s, bk=32):
    """The k-tile range [kb, ke) of each of the s slices as the tile code cuts them (BK = 32; 16 in the TT kernel), and how many are empty."""
    nk = (K + bk - 1) // bk
    per = (nk + s - 1) // s
    r = [(z * per, min(nk, z * per + per)) for z in range(s)]
    return r, sum(1 for kb, ke in r if kb >= ke)


def finishing_pass(M, N, s, stats=False):
    if s == 1:
        return 'none'
    if stats:
        return 'stats'
    return 'sum16' if s >= 16 and M * N <= 65536 else 'sum'


def loader_kind(layout, M, N, K, lda, ldb, off_a=0, off_b=0):
    """launch_gemm_v2: 16-byte loads ('vec') or the guarded scalar loader; off_*: floats from a 16-byte boundary.  TT: always scalar."""
    tA, tB = LAYOUTS[layout]
    if tA and tB:
        return 'scalar'
    va = (M if tA else K) % 4 == 0
    vb = (K if tB else N) % 4 == 0
    return 'vec' if va and vb and lda % 4 == 0 and ldb % 4 == 0 and off_a % 4 == 0 and off_b % 4 == 0 else 'scalar'


def epilogue_kinds(M, N, s, ldc, off_c=0):
    """The tile epilogue's store per slab: unsplit it looks at C itself, split at slab z of a 16-byte aligned workspace (ld = N)."""
    if s == 1:
        return {'vec' if ldc % 4 == 0 and N % 4 == 0 and off_c % 4 == 0 else 'scalar'}
    return {'vec' if N % 4 == 0 and (z * M * N) % 4 == 0 else 'scalar' for z in range(s)}


def group_plan(layout, shapes):
    """yk_gemm_f32_grouped for problems [(M, N, K)] (aligned operands, leading dimensions that keep 16-byte rows).
    Per problem: fallback (own yk_gemm_f32 call), the slices it would take alone, the slices re-sized for the group
    (T = max(8, units / 8192) k-tiles of 32 per slice), the slab offset in floats (rounded up to 4) and the finishing pass;
    and the number of grouped launches."""
    tA, tB = LAYOUTS[layout]
    out, grouped = [], []
    for i, (M, N, K) in enumerate(shapes):
        fb = (tA and tB) or loader_kind(layout, M, N, K, 4, 4) != 'vec'
        out.append(dict(fallback=fb, alone=gemm_splits(M, N, K)))
        if not fb:
            grouped.append(i)
    units = sum(((shapes[i][0] + 63) // 64) * ((shapes[i][1] + 63) // 64) * ((shapes[i][2] + 31) // 32) for i in grouped)
    T = max(8.0, units / 8192.0)
    off = 0
    for i in grouped:
        M, N, K = shapes[i]
        nk = (K + 31) // 32
        s = max(1, min(gemm_splits(M, N, K), int((nk + T - 1) / T)))
        out[i].update(splits=s, slab_offset=off if s > 1 else None, finish=finishing_pass(M, N, s), empty=k_slices(K, s)[1])
        if s > 1:
            off += (s * M * N + 3) // 4 * 4
    for i, p in enumerate(out):
        if p['fallback']:
            M, N, K = shapes[i]
            p.update(splits=p['alone'], slab_offset=None, finish=finishing_pass(M, N, p['alone']), empty=0)
    return out, (len(grouped) + YK_GROUP_MAX - 1) // YK_GROUP_MAX


# ------------------------------------------------------------------------------------------------ buffers
def place(mat, pad, off):
    """The matrix in a flat float32 buffer: `off` floats in front, rows of mat.shape[1] + pad, SPARE floats behind; everything that is not
    the matrix holds NAN_BITS.  Returns (buffer, leading dimension)."""
    rows, cols = mat.shape
    ld = cols + pad
    buf = np.full(off + rows * ld + SPARE, NAN_BITS, np.int32).view(np.float32)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :cols] = mat
    return buf, ld


def logical(buf, rows, cols, pad, off):
    ld = cols + pad
    return buf[off:off + rows * ld].reshape(rows, ld)[:, :cols]


def guard_mask(rows, cols, pad, off):
    """True where the buffer of place() holds no matrix element: the leading floats, the guard columns and the spare floats."""
    ld = cols + pad
    m = np.ones(off + rows * ld + SPARE, bool)
    m[off:off + rows * ld].reshape(rows, ld)[:, :cols] = False
    return m


# ------------------------------------------------------------------------------------------------ yk_gemm_f32
# pa / pb / pc: padding of lda / ldb / ldc over the row length; oa / ob / oc: floats the operand starts past a 16-byte boundary; ab: ALPHA_BETA index
GemmCase = collections.namedtuple('GemmCase', 'layout M N K pa pb pc oa ob oc ab')


def G(layout, M, N, K, pa=0, pb=0, pc=0, oa=0, ob=0, oc=0, ab=0):
    return GemmCase(layout, M, N, K, pa, pb, pc, oa, ob, oc, ab)


def a_shape(c):
    return (c.K, c.M) if LAYOUTS[c.layout][0] else (c.M, c.K)


def b_shape(c):
    return (c.N, c.K) if LAYOUTS[c.layout][1] else (c.K, c.N)


def gemm_plan(c):
    s = gemm_splits(c.M, c.N, c.K)
    slices, empty = k_slices(c.K, s, 16 if c.layout == 'TT' else 32)
    return dict(splits=s, slices=slices, empty=empty, finish=finishing_pass(c.M, c.N, s),
                loader=loader_kind(c.layout, c.M, c.N, c.K, a_shape(c)[1] + c.pa, b_shape(c)[1] + c.pb, c.oa, c.ob),
                epilogues=epilogue_kinds(c.M, c.N, s, c.N + c.pc, c.oc))


def gemm_id(c):
    p = gemm_plan(c)
    return (f'{c.layout}-{c.M}x{c.N}x{c.K}-a{c.pa}.{c.oa}-b{c.pb}.{c.ob}-c{c.pc}.{c.oc}-ab{c.ab}-ld_{p["loader"]}-st_{"+".join(sorted(p["epilogues"]))}'
            f'-{p["finish"]}-s{p["splits"]}-e{p["empty"]}')


def gemm_path(c):
    p = gemm_plan(c)
    return f'{c.layout}/{p["loader"]}/{"+".join(sorted(p["epilogues"]))}/{p["finish"]}'


TILE_EDGES = [(1, 1, 1), (64, 64, 32), (63, 65, 31), (65, 63, 33), (130, 36, 20)]
SCALAR_BY_SHAPE = {'NT': (20, 12, 23), 'TN': (17, 12, 20), 'NN': (20, 19, 24), 'TT': (17, 19, 23)}
SPLIT_SHAPES = [(5, 3, 112), (5, 3, 113), (8, 8, 288), (5, 3, 1008), (5, 3, 1009), (256, 256, 1024), (257, 256, 1024), (3, 5, 32768), (3, 5, 32752)]


def _gemm_cases():
    out = []
    for L in LAYOUTS:
        for i, mnk in enumerate(TILE_EDGES):
            out.append(G(L, *mnk, pc=4, ab=i % 2))
        # loader: vec (padded leading dimensions that keep the 16-byte rows), scalar by shape, by lda, by ldb, by A / B one float off the grid
        out += [G(L, 68, 36, 40, pa=4, pb=8, ab=1), G(L, *SCALAR_BY_SHAPE[L], pa=4, pb=4), G(L, 68, 36, 40, pa=1), G(L, 68, 36, 40, pb=2, ab=1),
                G(L, 68, 36, 40, oa=1), G(L, 68, 36, 40, ob=1, ab=1)]
        # epilogue: vec; scalar by N % 4 (N of 1..3, a last group of four cut to 1, 2, 3 columns), by ldc % 4, by C one float off; ldc > N everywhere
        for ab in (0, 1):
            out.append(G(L, 20, 8, 16, pc=4, ab=ab))
            out += [G(L, 9, n, 12, pc=3, ab=ab) for n in (1, 2, 3, 65, 66, 67)]
            out.append(G(L, 20, 8, 16, pc=1, ab=ab))
            out.append(G(L, 20, 8, 16, pc=4, oc=1, ab=ab))
        # split-K: beta == 0 over NaN, beta = 2, and a padded ldc
        for mnk in SPLIT_SHAPES:
            out += [G(L, *mnk), G(L, *mnk, ab=1), G(L, *mnk, pc=3, ab=1)]
    return out


GEMM_CASES = _gemm_cases()
GEMM_NORMAL_CASES = [c for c in GEMM_CASES if c.K <= NORMAL_K_MAX]


def _gemm_data(layout, M, N, K, ab, lattice, key):
    """A, B, C0 as stored (float32), the float64 reference, the largest sum of |terms| and the per-element normal-data bound."""
    tA, tB = LAYOUTS[layout]
    alpha, beta = ALPHA_BETA[ab]
    rng = _rng('gemm', key, lattice)
    A, B, C0 = _draw(rng, (K, M) if tA else (M, K), lattice), _draw(rng, (N, K) if tB else (K, N), lattice), _draw(rng, (M, N), lattice)
    opA, opB = (A.T if tA else A).astype(np.float64), (B.T if tB else B).astype(np.float64)
    ref = alpha * (opA @ opB) + (beta * C0.astype(np.float64) if beta != 0 else 0.0)
    mag = abs(alpha) * (np.abs(opA) @ np.abs(opB)) + abs(beta) * np.abs(C0.astype(np.float64))
    return dict(A=A, B=B, C0=C0, ref=ref, abs_sum=float((np.abs(opA) @ np.abs(opB)).max() + 6), bound=gamma(K + 4) * mag, alpha=alpha, beta=beta)


@functools.lru_cache(maxsize=None)
def gemm_problem(c, lattice):
    """One case, computed once and shared (read-only): the three flat buffers of place(), their leading dimensions, C's guard mask and the
    float64 reference.  C's buffer holds NAN_BITS everywhere for beta == 0; for beta != 0 it holds C0 in the logical region."""
    d = _gemm_data(c.layout, c.M, c.N, c.K, c.ab, lattice, tuple(c))
    bufA, lda = place(d['A'], c.pa, c.oa)
    bufB, ldb = place(d['B'], c.pb, c.ob)
    bufC, ldc = place(d['C0'], c.pc, c.oc)
    if d['beta'] == 0:
        bufC.view(np.int32)[:] = NAN_BITS
    d.update(bufA=bufA, bufB=bufB, bufC=bufC, lda=lda, ldb=ldb, ldc=ldc, guard=guard_mask(c.M, c.N, c.pc, c.oc),
             bytes=4 * (bufA.size + bufB.size + bufC.size))
    return _freeze(d)


# ------------------------------------------------------------------------------------------------ yk_gemm_f32_grouped
# (M, N, K) per layout, in an order that puts: a problem re-sized by the group first ((5, 3, 1024): 16 slices alone, 4 in a small group; NT
# with an odd M*N, so the next split problem's slabs start on the rounded offset), a one-workgroup problem, a several-tile problem right
# after it (the first[] lookup), a split problem with 16-byte slabs right after the odd one, one with 16 slices (the 16-lane sum), a problem
# in the middle that cannot take 16-byte loads (its own launch, split), another odd split one, an unsplit full tile and a ragged several-tile one.
GROUP_PATTERN = {
    'NT': [(5, 3, 1024), (8, 8, 32), (68, 132, 64), (12, 8, 1024), (8, 8, 4096), (8, 8, 290), (7, 9, 288), (64, 64, 64), (130, 36, 320)],
    'NN': [(8, 4, 1024), (8, 8, 32), (68, 132, 64), (12, 8, 1024), (8, 8, 4096), (8, 8, 290), (7, 12, 288), (64, 64, 64), (130, 36, 320)],
    'TN': [(8, 4, 1024), (8, 8, 32), (68, 132, 64), (12, 8, 1024), (8, 8, 4096), (6, 8, 288), (12, 12, 288), (64, 64, 64), (132, 36, 320)],
    'TT': [(5, 3, 113), (8, 8, 32), (65, 63, 33)],
}
GROUP_COUNTS = [1, YK_GROUP_MAX, YK_GROUP_MAX + 1, 2 * YK_GROUP_MAX + 1]       # one launch, exactly full, one over, three launches
GROUP_CASES = [(L, n) for L in ('NT', 'NN', 'TN') for n in GROUP_COUNTS] + [('TT', 3)]


def group_shapes(layout, count):
    """The pattern repeated until `count` problems that ride in grouped launches are in the list (YK_GROUP_MAX counts those); the problems
    that fall back to their own launch come along where the pattern has them.  TT: `count` problems, every one a fallback."""
    pat = GROUP_PATTERN[layout]
    if layout == 'TT':
        return [pat[i % len(pat)] for i in range(count)]
    out, grouped, i = [], 0, 0
    while grouped < count:
        out.append(pat[i % len(pat)])
        grouped += loader_kind(layout, *out[-1], 4, 4) == 'vec'
        i += 1
    return out


def group_pad_c(i):
    return (0, 4, 1, 3)[i % 4]


def group_ab(count):
    return 0 if count in (1, YK_GROUP_MAX + 1) else 1


@functools.lru_cache(maxsize=None)
def group_problem(layout, count):
    """Lattice problems of one grouped call: per problem A, B (plain, aligned), C's buffer of place() with guard columns, the reference."""
    ab = group_ab(count)
    ps = []
    for i, (M, N, K) in enumerate(group_shapes(layout, count)):
        d = _gemm_data(layout, M, N, K, ab, True, ('group', layout, count, i))
        bufC, ldc = place(d['C0'], group_pad_c(i), 0)
        if d['beta'] == 0:
            bufC.view(np.int32)[:] = NAN_BITS
        d.update(bufC=bufC, ldc=ldc, guard=guard_mask(M, N, group_pad_c(i), 0), pc=group_pad_c(i), M=M, N=N, K=K)
        ps.append(_freeze(d))
    return ps


# ------------------------------------------------------------------------------------------------ yk_gemm_bn_fwd_f32
# (M, N, K, px, pw, ox, residual): px / pw pad ldx / ldw, ox starts X one float off the grid.  K <= 112 is unsplit (the STATS epilogue).
GemmBnCase = collections.namedtuple('GemmBnCase', 'M N K px pw ox res')
GEMM_BN_CASES = [GemmBnCase(*t) for t in [
    (1, 1, 8, 0, 0, 0, False), (63, 4, 36, 0, 0, 0, True), (64, 63, 20, 0, 0, 0, False), (65, 65, 32, 0, 0, 0, True), (130, 68, 64, 0, 0, 0, False),
    (130, 1, 12, 0, 0, 0, True), (1, 68, 16, 0, 0, 0, False),                  # rows past M in every wave / a one-row batch over two column tiles
    (65, 12, 23, 0, 0, 0, True), (64, 8, 32, 0, 0, 1, False),                  # the scalar STATS kernel: K % 4 != 0, X one float off the grid
    (63, 12, 32, 4, 8, 0, True), (63, 12, 32, 1, 0, 0, False),                 # ldx > K: 16-byte rows kept / lost
    (100, 12, 288, 0, 0, 0, True), (1600, 8, 288, 4, 0, 0, False),             # split: 4 slices, one empty -> splitk_sum_stats_kernel; M > 1536
]]


def bn_finish_path(M, N):
    """bn_finish_apply for aligned tensors: one workgroup per 8 channels ('cols') or the statistics kernel + the apply pass."""
    return 'cols' if M <= 3 * 512 and N % 4 == 0 else 'finish+apply'


def gemm_bn_plan(c):
    s = gemm_splits(c.M, c.N, c.K)
    return dict(splits=s, empty=k_slices(c.K, s)[1], finish=finishing_pass(c.M, c.N, s, stats=True) if s > 1 else 'stats_epilogue',
                loader=loader_kind('NT', c.M, c.N, c.K, c.K + c.px, c.K + c.pw, c.ox, 0), bn=bn_finish_path(c.M, c.N))


def gemm_bn_id(c):
    p = gemm_bn_plan(c)
    return f'{c.M}x{c.N}x{c.K}-x{c.px}.{c.ox}-w{c.pw}-res{int(c.res)}-ld_{p["loader"]}-{p["finish"]}-s{p["splits"]}-e{p["empty"]}-{p["bn"]}'


@functools.lru_cache(maxsize=None)
def gemm_bn_problem(c):
    rng = _rng('gemm_bn', tuple(c))
    X, W = _draw(rng, (c.M, c.K), True), _draw(rng, (c.N, c.K), True)
    bufX, ldx = place(X, c.px, c.ox)
    bufW, ldw = place(W, c.pw, 0)
    z = X.astype(np.float64) @ W.astype(np.float64).T
    return _freeze(dict(bufX=bufX, ldx=ldx, bufW=bufW, ldw=ldw, z=z, abs_sum=float((np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T).max()),
                        gamma=rng.uniform(0.5, 2, c.N).astype(np.float32), beta=rng.normal(size=c.N).astype(np.float32),
                        res=rng.normal(size=(c.M, c.N)).astype(np.float32) if c.res else None))


# ------------------------------------------------------------------------------------------------ implicit 3x3 convolutions
# (B, Hi, Wi, Ci, Co, stride, padding): TF "same", or "valid" (pad_t = pad_l = 0, Ho = Hi - 2) - the entry points take Ho, Wo and the padding as given
ConvCase = collections.namedtuple('ConvCase', 'B Hi Wi Ci Co stride padding')
CONV_CASES = [ConvCase(*t) for t in [
    (1, 1, 1, 4, 4, 1, 'same'),          # one pixel: only the centre tap
    (2, 3, 3, 4, 10, 1, 'same'),         # every pixel on a border, an image boundary inside the M tile, scalar epilogue; forward only
    (3, 5, 7, 12, 8, 1, 'same'),         # tap boundaries at multiples of 12 inside the 32-wide k-tile; M = 105
    (2, 6, 5, 16, 12, 1, 'same'),        # K = 144: 2 slices
    (2, 4, 5, 32, 8, 1, 'same'),         # K = 288: 4 slices, one empty (forward)
    (2, 4, 5, 8, 32, 1, 'same'),         # the same for the data gradient (K = 9 Co)
    (2, 10, 8, 8, 20, 2, 'same'),        # stride 2, even input: top / left padding 0
    (2, 9, 7, 8, 20, 2, 'same'),         # stride 2, odd input: padding 1
    (1, 2, 130, 4, 4, 2, 'same'),        # Wo = 65
    (2, 5, 6, 4, 68, 1, 'same'),         # a second, 4-wide column tile in forward
    (2, 5, 6, 68, 4, 1, 'same'),         # ... and in the data gradient
    (4, 16, 16, 4, 4, 1, 'same'),        # weight gradient over 1024 pixels: 16 slices, the 16-lane sum
    (2, 6, 7, 8, 8, 1, 'valid'),
]]
CONV_BN_CASES = [CONV_CASES[2], CONV_CASES[3]]


def conv_geom(c):
    """(B, Hi, Wi, Ci, Ho, Wo, stride, pad_t, pad_l) as the C entry points take it, and (pad_b, pad_r)."""
    if c.padding == 'valid':
        assert c.stride == 1
        return (c.B, c.Hi, c.Wi, c.Ci, c.Hi - 2, c.Wi - 2, 1, 0, 0), (0, 0)
    Ho, Wo = -(-c.Hi // c.stride), -(-c.Wi // c.stride)
    th, tw = max((Ho - 1) * c.stride + 3 - c.Hi, 0), max((Wo - 1) * c.stride + 3 - c.Wi, 0)
    return (c.B, c.Hi, c.Wi, c.Ci, Ho, Wo, c.stride, th // 2, tw // 2), (th - th // 2, tw - tw // 2)


def conv_calls(c):
    """Which entry points accept the case: forward always (Ci % 4 == 0 in every case), the gradients with Co % 4 == 0, the data gradient at stride 1."""
    assert c.Ci % 4 == 0
    return dict(fwd=True, bwd_weight=c.Co % 4 == 0, bwd_data=c.Co % 4 == 0 and c.stride == 1)


def conv_gemm_shapes(c):
    """(M, N, K) of the implicit GEMM behind each call."""
    (B, Hi, Wi, Ci, Ho, Wo, *_), _ = conv_geom(c)
    return dict(fwd=(B * Ho * Wo, c.Co, 9 * Ci), bwd_weight=(c.Co, 9 * Ci, B * Ho * Wo), bwd_data=(B * Hi * Wi, Ci, 9 * c.Co))


def conv_plan(c, stats=False):
    out = {}
    for call, (M, N, K) in conv_gemm_shapes(c).items():
        s = gemm_splits(M, N, K)
        out[call] = dict(splits=s, empty=k_slices(K, s)[1], finish=finishing_pass(M, N, s, stats and call == 'fwd'), epilogues=epilogue_kinds(M, N, s, N),
                         tiles=((M + 63) // 64, (N + 63) // 64))
    return out


def conv_id(c):
    p = conv_plan(c)
    return '-'.join(str(v) for v in c) + '-' + '-'.join(f'{k}_{p[k]["finish"]}.s{p[k]["splits"]}.e{p[k]["empty"]}' for k, on in conv_calls(c).items() if on)


def conv_ref(c, x, w, dz):
    """float64 forward, data gradient and weight gradient through torch's conv2d with explicit padding.  x [B][Hi][Wi][Ci], w [3][3][Ci][Co],
    dz [B][Ho][Wo][Co]; returns (y NHWC, dx NHWC, dw [Co][9 Ci] with k = (ky*3 + kx) * Ci + ci: the layout of the entry points)."""
    (B, Hi, Wi, Ci, Ho, Wo, stride, pad_t, pad_l), (pad_b, pad_r) = conv_geom(c)
    xt = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (pad_l, pad_r, pad_t, pad_b)), wt.permute(3, 2, 0, 1), stride=stride)
    assert tuple(yt.shape) == (B, c.Co, Ho, Wo), (tuple(yt.shape), (B, c.Co, Ho, Wo))
    yt.backward(torch.from_numpy(np.asarray(dz, np.float64)).permute(0, 3, 1, 2))
    return (yt.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy(),
            np.ascontiguousarray(np.transpose(wt.grad.numpy(), (3, 0, 1, 2))).reshape(c.Co, 9 * Ci))


def conv_weights(w):
    """w [3][3][Ci][Co] as the entry points take it: [Co][9 Ci]."""
    return np.ascontiguousarray(np.transpose(w, (3, 0, 1, 2))).reshape(w.shape[3], 9 * w.shape[2])


@functools.lru_cache(maxsize=None)
def conv_problem(c, lattice):
    """Inputs and references of one case (read-only).  mag_*: the same three results on |x|, |w|, |dz| - for lattice data their maximum
    bounds every partial sum (`abs_sum`), for normal data gamma(reduction length + 4) times them is the per-element bound."""
    (B, Hi, Wi, Ci, Ho, Wo, *_), _ = conv_geom(c)
    rng = _rng('conv', tuple(c), lattice)
    x, w, dz = _draw(rng, (B, Hi, Wi, Ci), lattice), _draw(rng, (3, 3, Ci, c.Co), lattice), _draw(rng, (B, Ho, Wo, c.Co), lattice)
    y, dx, dw = conv_ref(c, x, w, dz)
    my, mdx, mdw = conv_ref(c, np.abs(x), np.abs(w), np.abs(dz))
    K = {k: v[2] for k, v in conv_gemm_shapes(c).items()}
    return _freeze(dict(x=x, w=w, wd=conv_weights(w), dz=dz, y=y, dx=dx, dw=dw, abs_sum=float(max(my.max(), mdx.max(), mdw.max())),
                        bound_y=gamma(K['fwd'] + 4) * my, bound_dx=gamma(K['bwd_data'] + 4) * mdx, bound_dw=gamma(K['bwd_weight'] + 4) * mdw,
                        bytes=4 * (x.size + w.size + dz.size)))


def conv_normal_calls(c):
    """Normal data runs where the reduction is short enough for the bound to separate fp32 from lower-precision products: 9 Ci <= 320
    (forward and weight gradient; the latter reduces over pixels and gets the bound of its own length), 9 Co <= 320 for the data gradient."""
    on = conv_calls(c)
    return dict(fwd=9 * c.Ci <= NORMAL_K_MAX, bwd_weight=on['bwd_weight'] and 9 * c.Ci <= NORMAL_K_MAX, bwd_data=on['bwd_data'] and 9 * c.Co <= NORMAL_K_MAX)
