"""Crafted segments, segment tables and an independent reference for the magnitude-pruning select (csrc/yk_prune.hip: prune_hist_kernel,
prune_pick_kernel x 4, prune_mask_kernel), shared by tests/test_prune_cases.py (CPU: the table checked on its own) and
tests/test_gpu_prune_edges.py (the kernels).  Nothing here touches a GPU.

REFERENCE.  reference() orders uint32 PATTERNS with one np.sort and has no radix in it: u = bits(w) & 0x7fffffff, k' = min(max(k, 1), n),
thr = sort(u)[n - k'], mask = u >= thr, kept = sum(mask).  A NaN is just a pattern above infinity's.  It is written apart from
tests/prune_ref.mask_of on purpose; tests/test_prune_cases.py checks that the two agree.

CRAFTED SEGMENTS.  Built from explicit patterns (four 8-bit digits, most significant first: the digit of pass p is bits 24 - 8p ..), then given
random signs.  A Kind builds its content at every size of SIZES; its `target` names the pass, the bin and the edge of the pick test
`above < k && k <= above + h` it is written for.

LABELS.  walk() is a host model of the four passes (per pass: the chosen bin, `above`, `h`, the rank entering the pass, the number of
non-empty bins).  It is used ONLY to label the cases, so that tests/test_prune_cases.py can assert that every boundary stays covered; it is
never the expected value."""
import collections
import functools
import pathlib
import re
import zlib

import numpy as np

U = np.uint32
HEADER = pathlib.Path(__file__).resolve().parents[1] / 'include' / 'yolo_hip.h'
TILE = int(re.search(r'#define\s+YK_PRUNE_TILE\s+(\d+)', HEADER.read_text()).group(1))
SIZES = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1)
INF, NAN_LO, NAN_HI = 0x7f800000, 0x7f800001, 0x7fffffff
GAP = 0xffffffff                          # what the gaps between segments hold: -NaN, the largest pattern there is - nobody may look at it
TOP = (127, 255, 255, 255)                # the highest bin a pass can choose
HI = (0x3f, 0x80, 0x55)                   # the digits above the targeted pass of an edge segment


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def patterns(w) -> np.ndarray:
    return np.ascontiguousarray(w, np.float32).view(U).ravel() & U(0x7fffffff)


def clamp_keep(k: int, n: int) -> int:
    return min(max(int(k), 1), int(n))


Ref = collections.namedtuple('Ref', 'bits mask kept')      # threshold as its uint32 pattern, mask uint8 [n], kept


def reference(w, k: int) -> Ref:
    u = patterns(w)
    n = u.size
    assert n >= 1
    thr = np.sort(u)[n - clamp_keep(k, n)]
    mask = u >= thr
    return Ref(int(thr), mask.astype(np.uint8), int(mask.sum()))


def threshold_float(bits: int) -> np.ndarray:
    """The float32 whose pattern is `bits`, as an array of one element (a NaN keeps its payload)."""
    return np.array([bits], U).view(np.float32)


# ------------------------------------------------------------------------------------------------ the label model
Pass = collections.namedtuple('Pass', 'bin above h k bins')


def walk(w, k: int):
    """Host model of the four passes -> [Pass] * 4.  Labels only."""
    u = patterns(w)
    k, pre, out = clamp_keep(k, u.size), 0, []
    for p in range(4):
        sh = 24 - 8 * p
        sel = u if p == 0 else u[(u >> U(sh + 8)) == U(pre >> (sh + 8))]
        hist = np.bincount(((sel >> U(sh)) & U(255)).astype(np.int64), minlength=256)
        above = hist[::-1].cumsum()[::-1] - hist
        b = int(np.flatnonzero((above < k) & (k <= above + hist))[0])
        out.append(Pass(b, int(above[b]), int(hist[b]), k, int((hist > 0).sum())))
        pre, k = pre | (b << sh), k - int(above[b])
    return out


# ------------------------------------------------------------------------------------------------ crafted contents
def _join(d) -> np.ndarray:
    d = np.asarray(d, np.int64).reshape(-1, 4)
    return ((d[:, 0] << 24) | (d[:, 1] << 16) | (d[:, 2] << 8) | d[:, 3]).astype(U)


def _digits(rng, count, fixed, lo, hi):
    """[count, 4] digits: `fixed` first, then one digit drawn from [lo, hi], then free digits."""
    d = rng.integers(0, 256, (count, 4))
    d[:, :len(fixed)] = fixed
    d[:, len(fixed)] = rng.integers(lo, hi + 1, count)
    return d


def _edge(p, b, edge, top, n, rng):
    """The k-th largest in bin `b` of pass p, at an end of the pick test.  edge: 'first' k == above + 1 with h > 1, 'last' k == above + h with
    h > 1, 'only' h == 1 (both at once).  Elements above it share the digits before p and have a larger digit p; where b is the highest bin
    of the pass they have a larger digit p - 1 instead (pass 0 then has nothing above).  Elements below likewise.  top: what fills bin 127
    of pass 0, 'inf' (infinity and the largest finite numbers) or 'nan'."""
    h = min(n, 1 if edge == 'only' else max(2, n // 3))
    can_above, can_below = b < TOP[p] or p > 0, b > 0 or p > 0
    a = (n - h) // 2 if can_above and can_below else n - h if can_above else 0
    below = n - h - a
    assert can_below or below == 0
    inb = _digits(rng, h, HI[:p] + (b,), 0, 255) if p < 3 else np.tile(HI + (b,), (h, 1))
    inb = _join(inb)
    if (p, b) == (0, 127):
        if top == 'inf':
            inb = np.where(rng.random(h) < 0.5, U(INF), U(0x7f000000) | rng.integers(0, 0x800000, h).astype(U))
            inb[0] = INF
        else:
            inb = rng.integers(NAN_LO, NAN_HI + 1, h).astype(U)
            inb[:2] = (NAN_HI, NAN_LO)[:h]
    if b < TOP[p]:
        up = _digits(rng, a, HI[:p], b + 1, TOP[p])
    else:
        up = _digits(rng, a, HI[:max(p - 1, 0)], HI[p - 1] + 1, TOP[p - 1]) if p else np.zeros((0, 4), np.int64)
    if b > 0:
        down = _digits(rng, below, HI[:p], 0, b - 1)
    else:
        down = _digits(rng, below, HI[:max(p - 1, 0)], 0, HI[p - 1] - 1) if p else np.zeros((0, 4), np.int64)
    u = np.concatenate([inb, _join(up), _join(down)])
    return u, a + (h if edge == 'last' else 1)


def _mid(n):
    return (n + 1) // 2


def _k_of(which, n):
    return {'k1': 1, 'kmid': _mid(n), 'kn': n}[which]


def _share3(which, n, rng):
    """All elements share the top three bytes: passes 0 .. 2 see one bin, only pass 3 discriminates."""
    return U(0x3fa5c300) | rng.integers(0, 256, n).astype(U), _k_of(which, n)


def _equal(which, n, rng):
    """All elements equal (-0.37 or +0.37): every pass has one bin, kept == n for any k."""
    return np.full(n, np.array([0.37], np.float32).view(U)[0], U), _k_of(which, n)


BYTE_BASE = 0x3fa5c396


def _byte(q, n, rng):
    """Patterns that differ only in byte q (the digit of pass q)."""
    sh = 24 - 8 * q
    r = rng.integers(0, TOP[q] + 1, n).astype(U)
    return (U(BYTE_BASE) & ~U(0xff << sh)) | (r << U(sh)), _mid(n)


TIE_VALUE = 0x3f000000                    # 0.5
TIE_COUNTS = (2, 255, 256, 257, TILE + 1)


def _ties(m, n, rng):
    """m copies of the threshold value straddle rank k (fewer where the segment is smaller): kept > k."""
    m = min(m, n)
    a = (n - m) // 2
    up = rng.integers(TIE_VALUE + 1, 0x7f000000, a).astype(U)
    down = rng.integers(0, TIE_VALUE, n - m - a).astype(U)
    return np.concatenate([np.full(m, TIE_VALUE, U), up, down]), a + max(1, m // 2)


def _zeros(n, rng):
    """+0.0 and -0.0 under a third of non-zero weights, k inside the zeros: threshold pattern 0, mask all ones, kept == n."""
    a = n // 3
    return np.concatenate([rng.integers(1, 0x7f000000, a).astype(U), np.zeros(n - a, U)]), a + max(1, (n - a) // 2)


def _nan_same(which, n, rng):
    return np.full(n, 0x7fc00000, U), _k_of(which, n)


def _nan_payload(n, rng):
    u = rng.integers(NAN_LO, NAN_HI + 1, n).astype(U)
    u[:2] = (NAN_HI, NAN_LO)[:n]
    return u, _mid(n)


Target = collections.namedtuple('Target', 'p bin edge')
Kind = collections.namedtuple('Kind', 'name target build')


def _kinds():
    out = []
    for p in range(4):
        for b in (0, TOP[p]):
            for top in ('inf', 'nan') if (p, b) == (0, 127) else ('inf',):
                for edge in ('first', 'last', 'only'):
                    name = f'pass{p}-bin{b}-{edge}' + ('-nan' if top == 'nan' else '')
                    out.append(Kind(name, Target(p, b, edge), functools.partial(_edge, p, b, edge, top)))
    for which in ('k1', 'kmid', 'kn'):
        out.append(Kind(f'share3-{which}', None, functools.partial(_share3, which)))
        out.append(Kind(f'equal-{which}', None, functools.partial(_equal, which)))
        out.append(Kind(f'nan_same-{which}', None, functools.partial(_nan_same, which)))
    out.append(Kind('nan_payload', None, _nan_payload))
    for q in range(4):
        out.append(Kind(f'byte{q}', None, functools.partial(_byte, q)))
    for m in TIE_COUNTS:
        out.append(Kind(f'ties{m}', None, functools.partial(_ties, m)))
    out.append(Kind('zeros', None, _zeros))
    return out


KINDS = _kinds()
KIND_NAMES = [k.name for k in KINDS]


def kind(name) -> Kind:
    return KINDS[KIND_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def segment(name, n):
    """-> (weights float32 [n], read-only; k) of kind `name` at size n: the kind's patterns, shuffled, with random signs."""
    rng = _rng(name, n)
    u, k = kind(name).build(n, rng)
    assert u.dtype == U and u.size == n and not (u >> U(31)).any() and 1 <= k <= n, (name, n)
    u = rng.permutation(u)
    sign = rng.integers(0, 2, n).astype(U)
    if n >= 2:
        z = np.flatnonzero(u == 0)[:2]                                 # both zeros, where there are two
        sign[z] = (0, 1)[:z.size]
    w = (u | (sign << U(31))).view(np.float32)
    w.setflags(write=False)
    return w, int(k)


# ------------------------------------------------------------------------------------------------ segment tables
Layout = collections.namedtuple('Layout', 'name flat offsets sizes keeps tile_first')


def tile_first(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([(n + TILE - 1) // TILE for n in sizes])]).astype(np.int32)


def layout(name, segments, keeps) -> Layout:
    """Segments in one flat buffer with gaps in front of, between and behind them (a segment of size 0 gets an offset and a gap like any
    other); some start at odd element offsets.  The gaps hold GAP."""
    offs, o = [], 5
    for i, w in enumerate(segments):
        offs.append(o)
        o += len(w) + (3, 8, 1, 13)[i % 4]
    flat = np.full(o + 9, GAP, U).view(np.float32)
    for off, w in zip(offs, segments):
        flat[off:off + len(w)] = w
    flat.setflags(write=False)
    sizes = [len(w) for w in segments]
    assert len(keeps) == len(sizes)
    return Layout(name, flat, tuple(offs), tuple(sizes), tuple(int(k) for k in keeps), tile_first(sizes))


def expected(lay: Layout):
    """reference() of every segment of the layout; None for a segment of size 0."""
    return [reference(lay.flat[o:o + n], k) if n else None for o, n, k in zip(lay.offsets, lay.sizes, lay.keeps)]


def inside(lay: Layout) -> np.ndarray:
    """bool [flat.size]: the elements that belong to a segment."""
    m = np.zeros(lay.flat.size, bool)
    for o, n in zip(lay.offsets, lay.sizes):
        m[o:o + n] = True
    return m


@functools.lru_cache(maxsize=None)
def kind_layout(name) -> Layout:
    """All sizes of one kind as the segments of one flat buffer."""
    segs = [segment(name, n) for n in SIZES]
    return layout(name, [w for w, _ in segs], [k for _, k in segs])


def _quantised(rng, n):
    """Normal weights rounded to eighths: ties, zeros of both signs, and distinct values in between."""
    return (np.round(rng.standard_normal(n) * 8) / 8).astype(np.float32)


ZERO_PLACEMENTS = {                        # 0: a segment of size 0, with the keep given to it; letters: segments with content
    'zero_first': (('0', 1), 'A', 'B'),
    'zero_last': ('A', 'B', ('0', 0)),
    'zero_between': ('A', ('0', 5), 'B'),
    'zero_pair': ('A', ('0', -1), ('0', 2 ** 40), 'B'),
    'zero_everywhere': (('0', 0), ('0', 1), 'A', ('0', 3), 'B', 'C', ('0', -2 ** 62), ('0', 7)),
}
_ZERO_CONTENT = {'A': 300, 'B': TILE + 5, 'C': 7}


@functools.lru_cache(maxsize=None)
def zero_layout(name, with_zeros=True) -> Layout:
    """A table of ZERO_PLACEMENTS; with_zeros False: the same table without its segments of size 0."""
    segs, keeps = [], []
    for e in ZERO_PLACEMENTS[name]:
        if isinstance(e, tuple):
            if with_zeros:
                segs.append(np.zeros(0, np.float32))
                keeps.append(e[1])
        else:
            n = _ZERO_CONTENT[e]
            segs.append(_quantised(_rng('zero', e), n))
            keeps.append(_mid(n))
    return layout(name + ('' if with_zeros else '-without'), segs, keeps)


NSEGS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def nseg_layout(nseg) -> Layout:
    """nseg segments, most of one tile (1 .. 47 elements), with a three-tile segment a third of the way in and a two-tile segment last."""
    rng = _rng('nseg', nseg)
    sizes = rng.integers(1, 48, nseg).tolist()
    sizes[-1] = TILE + 1
    if nseg >= 3:
        sizes[nseg // 3] = 2 * TILE + 3
    segs = [_quantised(rng, n) for n in sizes]
    return layout(f'nseg{nseg}', segs, [int(rng.integers(1, n + 1)) for n in sizes])


CLAMP_SIZES = (1, 257, TILE + 1)


def clamp_keeps(n):
    return (0, -1, -2 ** 62, n, n + 1, 2 ** 40)


@functools.lru_cache(maxsize=None)
def clamp_layout() -> Layout:
    """Every keep of clamp_keeps() at every size of CLAMP_SIZES, each on content of its own (distinct values: kept == clamp(k, 1, n))."""
    rng = _rng('clamp')
    segs, keeps = [], []
    for n in CLAMP_SIZES:
        for k in clamp_keeps(n):
            segs.append(rng.permutation(np.arange(1, n + 1)).astype(np.float32) * np.float32(0.25) * rng.choice(np.array([-1, 1], np.float32), n))
            keeps.append(k)
    return layout('clamp', segs, keeps)
