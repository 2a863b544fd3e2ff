"""The case builders of tests/tile_cases.py and tiles.merge on them, checked on their own (no GPU): each case must really sit on the path or the
edge it is named after - candidates per class against the restated lds_cap, the distance of every match from the threshold, what is kept, an
add that rounds - or tests/test_gpu_tiles.py would compare the kernel with the reference somewhere harmless.  And the reference itself is held to
an independent float64 restatement of the rule (sort, then sweep), so that it is not the thing that is wrong."""
import numpy as np
import pytest

from k210_yolo_framework_amd import tiles
from tests import tile_cases as tc

F = np.float32
CASES = tc.all_cases()
BY_NAME = {c.name: c for c in CASES}


def _ids(cases):
    return [c.name for c in cases]


# ---- the rule once more, float64, sort-then-sweep; `sums`: the translation in 'float32' (the rule: one float32 add) or 'exact' (float64) ----
def _match64(k, b, metric):
    """match of box k [4] with boxes b [n, 4], float64"""
    ky0, ky1, kx0, kx1 = min(k[0], k[2]), max(k[0], k[2]), min(k[1], k[3]), max(k[1], k[3])
    y0, y1 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
    x0, x1 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
    ka, a = (ky1 - ky0) * (kx1 - kx0), (y1 - y0) * (x1 - x0)
    inter = np.maximum(np.minimum(ky1, y1) - np.maximum(ky0, y0), 0.0) * np.maximum(np.minimum(kx1, x1) - np.maximum(kx0, x0), 0.0)
    if metric == 'iou':
        ok = (ka > 0) & (a > 0)
        den = ka + a - inter
    else:
        den = np.minimum(ka, a)
        ok = den > 0
    return np.where(ok, inter / np.where(ok, den, 1.0), 0.0)


def merge64(rows_per_tile, origins, class_num, max_out, thresh, metric, sums='exact'):
    """-> (rows float64 [k, 6], candidate index [k], every match of a kept box with a candidate of its class)"""
    cand = []
    for r, o in zip(rows_per_tile, origins):
        r = np.asarray(r, F).reshape(-1, 6)
        if sums == 'float32':
            moved = (r[:, :4] + np.tile(np.asarray(o, F), 2)).astype(F).astype(np.float64)
        else:
            moved = r[:, :4].astype(np.float64) + np.tile(np.asarray(o, np.float64), 2)
        cand.append(np.concatenate([moved, r[:, 4:].astype(np.float64)], 1))
    cand = np.concatenate(cand, 0) if cand else np.zeros((0, 6))
    out, idx, seen = [], [], []
    for c in range(class_num):
        mine = [i for i in range(len(cand)) if cand[i, 5] == c and cand[i, 4] > -np.inf]
        order = sorted(mine, key=lambda i: (-cand[i, 4], i))
        kept = []
        for i in order:
            if len(kept) == max_out:
                break
            if not kept or not (_match64(cand[i, :4], cand[kept, :4], metric) > thresh).any():
                kept.append(i)
        for k in kept:
            seen.append(_match64(cand[k, :4], cand[mine, :4], metric))
        out += [cand[i] for i in kept]
        idx += kept
    return np.asarray(out, np.float64).reshape(-1, 6), np.asarray(idx, np.int64), np.concatenate(seen) if seen else np.zeros(0)


def _sums(case):
    return 'float32' if case.name.startswith('far_origin') else 'exact'


def test_names_are_unique_and_inputs_fit():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        cap = c.class_num * c.max_out
        assert all(r.dtype == F and r.shape[1] == 6 and len(r) <= cap for r in c.rows), c.name
        assert c.origins.dtype == F and c.origins.shape == (len(c.rows), 2), c.name
        assert sum(len(r) for r in c.rows) <= 8800, c.name                                    # sizes stay what keeps a GPU test to seconds


def test_lds_cap_restated():
    assert tc.lds_cap(3, 1, 8) == 64 and tc.lds_cap(2, 1, 8) == 64 and tc.lds_cap(3, 1, 32) == 128
    assert tc.lds_cap(33, 1, 64) == 2048 and tc.lds_cap(69, 3, 64) == 2048 and tc.lds_cap(65, 1, 30) == 1984
    assert tc.lds_cap(3, 5, 8) == 64 and tc.lds_cap(1, 1, 1) == 64 and tc.lds_cap(1, 1, 65) == 128


@pytest.mark.parametrize('case', CASES, ids=_ids(CASES))
def test_case_takes_the_path_it_claims(case):
    assert tc.case_lds_cap(case) == case.claims['lds_cap']
    assert tc.over(case) == case.claims['over'], tc.candidates(case)


@pytest.mark.parametrize('case', CASES, ids=_ids(CASES))
def test_reference_equals_the_float64_restatement_and_no_match_is_near_the_threshold(case):
    for (rows, origins), (got, gi) in zip(tc.pictures(case), tc.reference(case)):
        ref, ri, seen = merge64(rows, origins, case.class_num, case.max_out, case.thresh, case.metric, _sums(case))
        assert got.dtype == F and np.array_equal(gi, ri), case.name
        assert np.array_equal(got.astype(np.float64).view(np.int64), ref.view(np.int64)), case.name           # -0.0 is not 0.0 here
        assert not np.isnan(got[:, :4]).any() and not np.isnan(got[:, 4]).any() and np.all(got[:, 4] > -np.inf)
        assert np.all(got[:, 5] == np.floor(got[:, 5])) and np.all((got[:, 5] >= 0) & (got[:, 5] < case.class_num))
        if np.isfinite(case.thresh):
            away = seen[seen != case.thresh]
            assert not len(away) or np.abs(away - case.thresh).min() > 1e-5, (case.name, np.abs(away - case.thresh).min())


def _lattice(case):
    a = np.concatenate([r[:, :4].reshape(-1) for r in case.rows] + [case.origins.reshape(-1)])
    return bool(np.all(a * 4 == np.round(a * 4)) and np.abs(a).max() < 4096)


def test_coordinates_are_on_the_lattice_except_where_the_add_is_meant_to_round():
    for c in CASES:
        assert _lattice(c) == (not c.name.startswith('far_origin')), c.name


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_two_classes_global_small(metric):
    c = BY_NAME[f'two_classes_global_small-{metric}']
    per = tc.candidates(c)[0]
    assert per[:2] == [70, 70] and sum(per[2:]) == 52 and all(0 < n <= 64 for n in per[2:]) and [len(r) for r in c.rows] == [64, 64, 64]
    assert max(int((r[:, 5] == 0).sum()) for r in c.rows) > c.max_out                        # not decode-shaped
    got = tc.reference(c)[0][0]
    assert all((got[:, 5] == k).sum() >= 1 for k in range(8))
    assert (got[:, 5] == 0).sum() == (got[:, 5] == 1).sum() == 8                              # and some were retired on the way there:
    assert len(tiles.merge(c.rows, c.origins, 8, 70, 0.5, metric)[0]) < sum(per)


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_four_classes_global_stride8(metric):
    c = BY_NAME[f'four_classes_global_stride8-{metric}']
    per = tc.candidates(c)[0]
    assert [n for n in per if n > 64] == [70] * 4 and tc.over(c) == [[0, 1, 8, 9]] and sum(per) == 3 * 128 == sum(len(r) for r in c.rows)
    got = tc.reference(c)[0][0]
    assert all((got[:, 5] == k).sum() >= 1 for k in range(16)) and all((got[:, 5] == k).sum() == 8 for k in (0, 1, 8, 9))
    assert len({tuple(r) for k in (0, 1, 8, 9) for r in got[got[:, 5] == k][:, :5]}) == 32       # no two of these classes keep the same rows


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_boundary(metric):
    a, b = BY_NAME[f'boundary-64-{metric}'], BY_NAME[f'boundary-65-{metric}']
    assert tc.candidates(a)[0][0] == 64 == tc.case_lds_cap(a) and tc.candidates(b)[0][0] == 65 == tc.case_lds_cap(b) + 1
    assert all(n <= 64 for n in tc.candidates(a)[0][1:] + tc.candidates(b)[0][1:])
    last = b.rows[2][-1]
    assert last[5] == 0 and last[4] == max(r[:, 4].max() for r in b.rows)                     # position 64 of class 0, the best of the picture
    assert int((np.concatenate(b.rows)[:, 5] == 0).sum()) == 65 and [len(r) for r in b.rows] == [64, 64, 64]
    got = tc.reference(b)[0][0]
    assert np.array_equal(got[0], b.claims['first_row']) and not np.array_equal(tc.reference(a)[0][0][0], got[0])


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_decode_shaped_and_mixed(metric):
    c = BY_NAME[f'two_classes_global_decode_shaped-{metric}-3']
    assert len(c.rows) == 33 and tc.candidates(c) == [[2112, 2112]]
    for r in c.rows:
        assert r[:, 5].tolist() == [0.0] * 64 + [1.0] * 64 and np.all(np.diff(r[:64, 4]) <= 0) and np.all(np.diff(r[64:, 4]) <= 0)
    got = tc.reference(c)[0][0]
    assert (got[:, 5] == 0).sum() == (got[:, 5] == 1).sum() == c.claims['kept_per_class'] == c.max_out
    other = tc.two_classes_global_decode_shaped(metric, seed=13)
    assert not np.array_equal(tc.reference(other)[0][0], got)
    m = BY_NAME[f'three_pictures_mixed-{metric}']
    assert m.first == (0, 33, 36, 69) and tc.candidates(m) == [[2112, 2112], [100, 78], [2112, 2112]]
    assert [len(r) for r in m.rows[33:36]] == [50, 0, 128]
    res = tc.reference(m)
    assert [len(r) for r, _ in res] == [128, len(res[1][0]), 128] and 0 < len(res[1][0]) < 128
    assert not np.array_equal(res[0][0], res[2][0])


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_dropped_rows(metric):
    c = BY_NAME[f'dropped_rows-{metric}']
    allr = np.concatenate(c.rows)
    assert [len(r) for r in c.rows] == [64, 64, 64]                                           # every one of them is a counted row
    s, k = allr[:, 4], allr[:, 5]
    for cl in (0, 2):
        assert (np.isnan(s) & (k == cl)).sum() == 1 and ((s == -np.inf) & (k == cl)).sum() == 1 and ((s == np.inf) & (k == cl)).sum() == 1
        assert ((s == 0) & np.signbit(s) & (k == cl)).sum() == 1
    assert (k == -1).sum() == 2 and (k == 8).sum() == 2 and (k == 1.5).sum() == 1 and np.isnan(k).sum() == 1
    per = tc.candidates(c)[0]
    assert per[0] == c.claims['candidates0'] == 70 and per[2] == c.claims['candidates2'] == 6
    got = tc.reference(c)[0][0]
    g0, g2 = got[got[:, 5] == 0], got[got[:, 5] == 2]
    assert len(g0) == 8 and g0[0, 4] == np.inf and np.isfinite(g0[1:, 4]).all()
    want2 = np.asarray(c.claims['class2'], F)
    assert np.array_equal(g2.view(np.int32), want2.view(np.int32)) and np.signbit(g2[-1, 4]) and g2[0, 4] == np.inf
    assert np.isfinite(got[:, :4]).all() and (np.abs(got[:, 4]) != 0.99).all() and (got[:, 4] != 2.0).all()      # no row of a bad class came through


@pytest.mark.parametrize('metric', tiles.METRICS)
@pytest.mark.parametrize('kind', ['plain', 'zero', 'inf'])
def test_box_edges(metric, kind):
    c = BY_NAME[f'box_edges-{kind}-{metric}']
    got, idx = tc.reference(c)[0]
    assert idx.tolist() == c.claims['kept']
    if kind == 'plain':
        assert got[0].tolist() == [10, 10, 20, 20, 0.875, 0]
        # without the normalisation the swapped boxes have a positive or a negative area and an empty intersection: they would stay
        swapped = [r for r in np.concatenate([c.rows[0], c.rows[1]]) if r[5] == 0 and (r[0] > r[2] or r[1] > r[3])]
        assert len(swapped) == 3 and sum(r[0] > r[2] and r[1] > r[3] for r in swapped) == 1
    if kind == 'inf':
        assert c.thresh == float('inf') and len(got) == c.max_out < tc.candidates(c)[0][0] == 12 and len({tuple(r[:4]) for r in got}) == 1


@pytest.mark.parametrize('metric', tiles.METRICS)
def test_far_origin_adds_round_and_decide(metric):
    c = BY_NAME[f'far_origin-{metric}']
    got, idx = tc.reference(c)[0]
    assert len(got) == c.claims['kept_total'] == 12 and sum(len(r) for r in c.rows) == 24
    allr = np.concatenate(c.rows)
    off = np.repeat(c.origins, [len(r) for r in c.rows], 0)
    exact = allr[:, :4].astype(np.float64) + np.tile(off.astype(np.float64), 2)
    f32 = (allr[:, :4] + np.tile(off, 2)).astype(F)
    assert (f32.astype(np.float64) != exact).sum() >= 24                                      # the add really rounds, many times over
    assert np.array_equal(got[:, :4], f32[idx]) and (got[:, :4].astype(np.float64) != exact[idx]).any()
    assert len(set(idx.tolist()) & set(range(12, 24))) >= 3                                   # a later tile's copy wins somewhere
    t = BY_NAME[f'far_origin_touch-{metric}']
    rows, origins = tc.pictures(t)[0]
    assert tc.reference(t)[0][1].tolist() == t.claims['kept'] == [0, 1]
    assert merge64(rows, origins, 1, 4, 0.0, metric, 'float32')[1].tolist() == [0, 1]
    assert merge64(rows, origins, 1, 4, 0.0, metric, 'exact')[1].tolist() == t.claims['kept_if_exact'] == [0]
    a, b = tc.reference(t)[0][0]
    assert a[2] == b[0] and a[3] > b[1] and b[3] > a[1]                                        # they touch, along a stretch of the edge


@pytest.mark.parametrize('metric', tiles.METRICS)
@pytest.mark.parametrize('path', ['lds', 'global'])
def test_ties(path, metric):
    c = BY_NAME[f'ties-{path}-{metric}']
    n = c.claims['n']
    assert tc.candidates(c)[0][:2] == [n, n] and n > 64 + 32 and c.claims['stride_pair_in_two_tiles']
    allr = np.concatenate(c.rows)
    assert set(allr[allr[:, 5] < 2][:, 4].tolist()) == {0.5}
    got, idx = tc.reference(c)[0]
    pos = lambda cl: np.flatnonzero(allr[:, 5] == cl)
    assert idx[:32].tolist() == pos(0)[:32].tolist() and idx[32:64].tolist() == pos(1)[:32].tolist()      # the lowest positions, in order
    p0 = allr[pos(0)]
    assert np.array_equal(p0[64, :4], p0[0, :4] + F(0.25)) and np.array_equal(allr[pos(1)][40], allr[pos(1)][0])


def test_clamps():
    cs = tc.clamps()
    assert [c.first.tolist() for c in cs] == [[0, 5, 2], [-1, 2], [0, 7]] and [c.n_pics for c in cs] == [2, 1, 1]
    for c in cs:
        cap = c.class_num * c.max_out
        assert c.counts.tolist() == [cap + 5, -3, 7] and c.dets.shape == (3, cap, 6) and c.n_tiles == 3
        assert (c.dets[1, :, 4] == tc.POISON).all() and (c.dets[2, 7:, 4] == tc.POISON).all() and (c.dets[0, :, 4] < 1).all()
        assert all((w[:, 4] < 1).all() for w in c.want)
    assert len(cs[0].want[1]) == 0 and len(cs[0].want[0]) > len(cs[1].want[0]) > 0
    assert np.array_equal(cs[0].want[0], cs[2].want[0])
