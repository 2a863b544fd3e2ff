"""tests/prune_cases.py checked on its own, without a GPU: the pattern reference against a brute-force sorted() and against
tests/prune_ref.mask_of, the crafted segments against the pass / bin / edge each one names, and the tables against every boundary that
tests/test_gpu_prune_edges.py is meant to pin.  The coverage is read from prune_cases.walk (a host model of the four passes, labels only)
and from the reference; a crafted case that stops reaching its edge after a change of a size fails here."""
import numpy as np
import pytest

from tests import prune_cases as pc
from tests import prune_ref

U = np.uint32
TARGETED = [k for k in pc.KINDS if k.target is not None]


def _cases(prefix=''):
    return [(k.name, n) + pc.segment(k.name, n) for k in pc.KINDS if k.name.startswith(prefix) for n in pc.SIZES]


def _f(*bits):
    return np.array(bits, U).view(np.float32)


# ------------------------------------------------------------------------------------------------ the reference and the label model
def test_reference_equals_a_brute_force_sort_of_patterns():
    rng = np.random.default_rng(5)
    pool = _f(0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, 0x3f800000, 0xbf800000, 0x3f800001, 0x7f7fffff, pc.INF, pc.INF | 0x80000000,
              pc.NAN_LO, 0x7fc00000, 0xffc00000, pc.NAN_HI, pc.GAP)
    for n in (1, 2, 3, 5, 17, 64):
        for _ in range(20):
            w = pool[rng.integers(0, pool.size, n)]
            for k in (-2 ** 62, -1, 0, 1, 2, n // 2, n - 1, n, n + 1, 2 ** 40):
                ints = sorted((int(x) & 0x7fffffff for x in w.view(U)), reverse=True)
                thr = ints[min(max(k, 1), n) - 1]                                        # the k'-th largest
                mask = [int((int(x) & 0x7fffffff) >= thr) for x in w.view(U)]
                r = pc.reference(w, k)
                assert (r.bits, r.mask.tolist(), r.kept) == (thr, mask, sum(mask)), (w.view(U), k)
                assert r.kept >= min(max(k, 1), n)
    assert pc.reference(_f(pc.INF, 0x7fc00000, 0x3f800000), 1).bits == 0x7fc00000       # NaN ranks above infinity
    assert pc.reference(_f(0xffc00000, pc.INF), 2).bits == pc.INF
    assert pc.threshold_float(0x7fc12345).view(U)[0] == 0x7fc12345                      # a payload survives the conversion


def test_reference_agrees_with_prune_ref_wherever_prune_ref_is_defined():
    """prune_ref.mask_of refuses k outside [1, n] and takes no size 0; everywhere else the two are the same function of the patterns, NaN
    included (prune_ref sorts patterns too, not floats)."""
    checked = 0
    lays = [pc.kind_layout(name) for name in pc.KIND_NAMES] + [pc.nseg_layout(n) for n in pc.NSEGS] + [pc.clamp_layout()] + \
        [pc.zero_layout(name) for name in pc.ZERO_PLACEMENTS]
    for lay in lays:
        for o, n, k, r in zip(lay.offsets, lay.sizes, lay.keeps, pc.expected(lay)):
            if n and 1 <= k <= n:
                thr, mask, kept = prune_ref.mask_of(lay.flat[o:o + n], k)
                assert np.array([thr], np.float32).view(U)[0] == r.bits and np.array_equal(mask.astype(np.uint8), r.mask) and kept == r.kept, (lay.name, n, k)
                checked += 1
    assert checked > 1000
    assert [1 for name in pc.KIND_NAMES if 'nan' in name]                                # ... among them NaN contents


def test_walk_model_ends_on_the_reference_threshold():
    """The labels can be trusted: the four chosen bins spell the reference's threshold, and the counts give its kept."""
    for name, n, w, k in _cases():
        ps = pc.walk(w, k)
        r = pc.reference(w, k)
        assert sum(p.bin << (24 - 8 * i) for i, p in enumerate(ps)) == r.bits, (name, n)
        assert k - (ps[3].k - ps[3].above) + ps[3].h == r.kept, (name, n)
        assert ps[0].k == k and all(1 <= p.k and p.above < p.k <= p.above + p.h for p in ps), (name, n)


def test_sizes_are_the_listed_ones_and_everything_stays_small():
    T = pc.TILE
    assert pc.SIZES == (1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T, 2 * T + 1)
    assert pc.TIE_COUNTS == (2, 255, 256, 257, 4097) and T == 4096
    for lay in [pc.kind_layout(name) for name in pc.KIND_NAMES] + [pc.nseg_layout(n) for n in pc.NSEGS] + [pc.clamp_layout()] + \
            [pc.zero_layout(name, z) for name in pc.ZERO_PLACEMENTS for z in (True, False)]:
        assert lay.flat.size < 50000, lay.name
        assert lay.tile_first[-1] <= 16 or lay.name.startswith('nseg') or lay.name == 'clamp', lay.name


# ------------------------------------------------------------------------------------------------ what the crafted segments reach
@pytest.mark.parametrize('name', [k.name for k in TARGETED])
def test_an_edge_segment_hits_the_pass_bin_and_edge_it_names(name):
    t = pc.kind(name).target
    for n in pc.SIZES:
        w, k = pc.segment(name, n)
        p = pc.walk(w, k)[t.p]
        assert p.bin == t.bin, (n, p)
        assert p.k == p.above + (p.h if t.edge == 'last' else 1), (n, p)
        if n >= 2:
            assert (p.h == 1) == (t.edge == 'only'), (n, p)
        if n >= 4 and t.p > 0:                                                           # the threshold has elements above and below it
            u, r = pc.patterns(w), pc.reference(w, k)
            assert (u > r.bits).any() and (u < r.bits).any() and r.kept < n, (n, p)


def test_every_pass_has_its_lowest_and_highest_bin_and_both_ends_of_the_pick_test():
    seen = set()
    for name, n, w, k in _cases('pass'):
        if n < 2:
            continue
        for i, p in enumerate(pc.walk(w, k)):
            if p.k == p.above + 1:
                seen.add((i, p.bin, 'first', p.h > 1))
            if p.k == p.above + p.h:
                seen.add((i, p.bin, 'last', p.h > 1))
    for i in range(4):
        for b in (0, pc.TOP[i]):
            for edge in ('first', 'last'):
                for many in (True, False):
                    assert (i, b, edge, many) in seen, (i, b, edge, many)
    assert pc.TOP == (127, 255, 255, 255)


def test_bin_127_of_pass_0_is_reached_with_infinity_and_with_nan():
    thr = {(name, n): pc.reference(w, k).bits for name, n, w, k in _cases('pass0-bin127')}
    assert [1 for (name, n), b in thr.items() if b == pc.INF and 'nan' not in name]
    assert [1 for (name, n), b in thr.items() if 0x7f000000 <= b < pc.INF]               # a finite number of bin 127
    assert [1 for (name, n), b in thr.items() if b == pc.NAN_HI] and [1 for (name, n), b in thr.items() if b == pc.NAN_LO]
    assert [1 for n in pc.SIZES if pc.NAN_LO < pc.reference(*pc.segment('nan_payload', n)).bits < pc.NAN_HI]
    for name, n, w, k in _cases('pass0-bin127'):
        if name.endswith('-nan') and n >= 4:                                             # NaNs above finite numbers: they rank first
            u, r = pc.patterns(w), pc.reference(w, k)
            assert (u > pc.INF).any() and (u < pc.INF).any() and r.bits > pc.INF and r.kept <= int((u > pc.INF).sum())


def test_degenerate_passes():
    for name, n, w, k in _cases('share3'):
        ps = pc.walk(w, k)
        assert [p.bins for p in ps[:3]] == [1, 1, 1] and (ps[3].bins > 1 or n == 1), (name, n)
    for name, n, w, k in _cases('equal'):
        assert [p.bins for p in pc.walk(w, k)] == [1, 1, 1, 1] and pc.reference(w, k).kept == n, (name, n)
        assert n < 255 or (np.signbit(w).any() and not np.signbit(w).all())
    assert {name.split('-')[1] for name, *_ in _cases('equal')} == {'k1', 'kmid', 'kn'}
    for which, want in (('k1', lambda n: 1), ('kn', lambda n: n)):
        assert all(k == want(n) for name, n, w, k in _cases('equal-' + which) + _cases('share3-' + which) + _cases('nan_same-' + which))


def test_patterns_that_differ_in_one_byte_only():
    for q in range(4):
        for name, n, w, k in _cases(f'byte{q}'):
            u = pc.patterns(w)
            assert not ((u ^ U(pc.BYTE_BASE)) & ~U(0xff << (24 - 8 * q))).any(), (q, n)
            bins = [p.bins for p in pc.walk(w, k)]
            assert all(b == 1 for i, b in enumerate(bins) if i != q), (q, n, bins)
            assert bins[q] > 1 or n == 1, (q, n, bins)
            if n >= 255:
                assert bins[q] > 64
    # every byte of the base is non-zero and differs from the others: a digit OR-ed into the wrong byte cannot go unnoticed
    assert len({(pc.BYTE_BASE >> s) & 255 for s in (0, 8, 16, 24)}) == 4 and all((pc.BYTE_BASE >> s) & 255 for s in (0, 8, 16, 24))


def test_ties_straddle_the_rank_at_every_listed_count():
    for m in pc.TIE_COUNTS:
        full = []
        for name, n, w, k in _cases(f'ties{m}'):
            if name != f'ties{m}':                                                       # (ties2 is a prefix of ties255 ...)
                continue
            u, r = pc.patterns(w), pc.reference(w, k)
            assert r.bits == pc.TIE_VALUE, (m, n)
            ties, above = int((u == r.bits).sum()), int((u > r.bits).sum())
            assert ties == min(m, n) and r.kept == above + ties
            if ties == m and above and r.kept < n:
                assert above < k < above + ties and r.kept > k, (m, n)
                full.append(n)
        assert full, m
    assert pc.TILE + 1 in pc.TIE_COUNTS and 257 in pc.TIE_COUNTS                         # past one tile; past the 256 bins' worth of one thread each


def test_zeros_of_both_signs_with_k_inside_them():
    for name, n, w, k in _cases('zeros'):
        r = pc.reference(w, k)
        assert r.bits == 0 and r.mask.all() and r.kept == n, n
        nonzero = int((pc.patterns(w) != 0).sum())
        assert nonzero < k <= n
        if n >= 255:
            z = w[pc.patterns(w) == 0]
            assert nonzero and np.signbit(z).any() and not np.signbit(z).all()


def test_the_out_of_tile_fill_case_is_there():
    """A NaN-filled segment of TILE + 1 elements: the last tile holds one element and TILE - 1 positions past the end, whose fill value has
    top byte 255 - counted with the NaNs' top digit 127 it would move `above` of pass 0."""
    T = pc.TILE
    assert T + 1 in pc.SIZES and pc.tile_first([T + 1])[-1] == 2
    for name in ('nan_same-k1', 'nan_same-kmid', 'nan_same-kn', 'nan_payload'):
        w, k = pc.segment(name, T + 1)
        u = pc.patterns(w)
        assert (u > pc.INF).all() and ((u >> U(24)) == 127).all()
        p0 = pc.walk(w, k)[0]
        assert (p0.bin, p0.above, p0.h) == (127, 0, T + 1)
    assert pc.reference(*pc.segment('nan_same-kn', T + 1)).kept == T + 1 and pc.segment('nan_same-kn', T + 1)[1] == T + 1
    assert np.unique(pc.patterns(pc.segment('nan_payload', T + 1)[0])).size > T // 2


def test_random_signs_and_shuffled_order():
    for name, n, w, k in _cases():
        if n >= 255:
            assert np.signbit(w).any() and not np.signbit(w).all(), (name, n)
    w, _ = pc.segment('pass1-bin0-first', 257)
    assert (np.diff(pc.patterns(w).astype(np.int64)) > 0).any() and (np.diff(pc.patterns(w).astype(np.int64)) < 0).any()


# ------------------------------------------------------------------------------------------------ the tables
def _check_table(lay):
    assert lay.flat.dtype == np.float32 and len(lay.offsets) == len(lay.sizes) == len(lay.keeps) == len(lay.tile_first) - 1
    ins = pc.inside(lay)
    assert (lay.flat.view(U)[~ins] == pc.GAP).all() and int(ins.sum()) == sum(lay.sizes)                  # disjoint segments, sentinel gaps
    assert not ins[0] and not ins[-1]
    assert lay.tile_first[0] == 0 and np.array_equal(np.diff(lay.tile_first), [(n + pc.TILE - 1) // pc.TILE for n in lay.sizes])
    assert all(0 <= o and o + n <= lay.flat.size for o, n in zip(lay.offsets, lay.sizes))


def test_kind_layouts_hold_every_size_between_sentinel_gaps():
    for name in pc.KIND_NAMES:
        lay = pc.kind_layout(name)
        _check_table(lay)
        assert lay.sizes == pc.SIZES
        assert [o % 4 for o in lay.offsets].count(0) < len(lay.offsets)                                   # some segments start off a 16-byte boundary
        for o, n, k in zip(lay.offsets, lay.sizes, lay.keeps):
            w, k0 = pc.segment(name, n)
            assert lay.flat[o:o + n].tobytes() == w.tobytes() and k == k0


def test_zero_size_placements():
    shape = {name: [n == 0 for n in pc.zero_layout(name).sizes] for name in pc.ZERO_PLACEMENTS}
    assert shape['zero_first'] == [True, False, False] and shape['zero_last'] == [False, False, True]
    assert shape['zero_between'] == [False, True, False] and shape['zero_pair'] == [False, True, True, False]
    assert shape['zero_everywhere'] == [True, True, False, True, False, False, True, True]
    keeps = set()
    for name in pc.ZERO_PLACEMENTS:
        lay, bare = pc.zero_layout(name), pc.zero_layout(name, False)
        _check_table(lay)
        _check_table(bare)
        tf = lay.tile_first
        assert all(tf[i] == tf[i + 1] for i, n in enumerate(lay.sizes) if n == 0) and tf[-1] == bare.tile_first[-1]
        assert [n for n in lay.sizes if n] == list(bare.sizes) and 0 not in bare.sizes
        for a, b in zip([r for r in pc.expected(lay) if r is not None], pc.expected(bare)):
            assert a.bits == b.bits and a.kept == b.kept and np.array_equal(a.mask, b.mask)
        assert any(n > pc.TILE for n in lay.sizes) and any(0 < n < pc.TILE for n in lay.sizes)            # one-tile and two-tile neighbours
        keeps |= {k for n, k in zip(lay.sizes, lay.keeps) if n == 0}
    assert keeps >= {0, 1, -1, 5, 2 ** 40, -2 ** 62}                                                      # k0 of a size 0 is 1 or 0: both


def test_nseg_sweep():
    assert set(pc.NSEGS) >= {1, 2, 3} | {p + d for p in (4, 8, 16, 32, 64, 128, 256) for d in (-1, 0, 1)} and max(pc.NSEGS) <= 300
    for nseg in pc.NSEGS:
        lay = pc.nseg_layout(nseg)
        _check_table(lay)
        assert len(lay.sizes) == nseg and min(lay.sizes) >= 1
        tiles = np.diff(lay.tile_first)
        assert (tiles > 1).sum() == (2 if nseg >= 3 else 1) and (tiles == 1).sum() == nseg - (tiles > 1).sum()
        assert all(1 <= k <= n for n, k in zip(lay.sizes, lay.keeps))
    big = pc.nseg_layout(257)
    assert any(r.kept > k for r, k in zip(pc.expected(big), big.keeps)) and any(r.kept == k for r, k in zip(pc.expected(big), big.keeps))


def test_keep_clamp_table():
    lay = pc.clamp_layout()
    _check_table(lay)
    assert pc.CLAMP_SIZES == (1, 257, pc.TILE + 1)
    i = 0
    for n in pc.CLAMP_SIZES:
        assert pc.clamp_keeps(n) == (0, -1, -2 ** 62, n, n + 1, 2 ** 40)
        for k in pc.clamp_keeps(n):
            assert lay.sizes[i] == n and lay.keeps[i] == k
            r = pc.expected(lay)[i]
            want = 1 if k < 1 else n                                                                      # distinct values: kept IS the clamped k
            assert r.kept == want == pc.clamp_keep(k, n), (n, k)
            assert r.bits == int(np.sort(pc.patterns(lay.flat[lay.offsets[i]:lay.offsets[i] + n]))[n - want])
            i += 1
    assert i == len(lay.sizes)
