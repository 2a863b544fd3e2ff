"""The picture cache's host side (cache.py): the planner without a device - alignment, contiguous admissions, no overlap, a full cache
stages instead of failing, a staging overflow names its flag, staging only, statistics, determinism - and the four options of `make train`."""
from pathlib import Path

import pytest

from k210_yolo_framework_amd.cache import ALIGN, PictureCache
from k210_yolo_framework_amd.engine import YkError

ROOT = Path(__file__).resolve().parents[1]
SIZES = [(1, 1), (7, 1), (33, 47), (50, 75), (33, 47), (17, 90), (64, 96), (5, 3), (120, 160), (9, 9), (31, 2), (50, 75)]


def size_of(row):
    return SIZES[row % len(SIZES)]


def nbytes(row):
    h, w = size_of(row)
    return 3 * h * w


def spans(plan, rows):
    return sorted((plan.table[r][0], plan.table[r][0] + nbytes(r)) for r in rows)


def test_offsets_are_aligned_contiguous_and_never_overlap():
    c = PictureCache(1 << 20, stage_bytes=1 << 16, prefetch=2, allocate=False)
    taken = []
    for first in range(0, 36, 6):
        rows = [first + k for k in range(6)] + [first, first + 3]             # repeats count once
        p = c.plan(rows, size_of)
        assert p.admitted == rows[:6] and not p.staged and not p.hits
        assert all(p.table[r][0] % ALIGN == 0 and p.table[r][1:] == size_of(r) for r in p.admitted)
        # one run: every picture starts at the aligned end of the one before, the first at the end of everything admitted so far
        at = p.admit_start
        assert at == c.stats().bytes_used
        for r in p.admitted:
            assert p.table[r][0] == at
            at = (at + nbytes(r) + ALIGN - 1) // ALIGN * ALIGN
        assert p.admit_end == p.table[rows[5]][0] + nbytes(rows[5]) <= c.capacity_bytes
        taken += spans(p, p.admitted)
        c.commit(p)
    taken.sort()
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))
    p = c.plan(range(36), size_of)                                             # all cached now, where they were put
    assert p.hits == list(range(36)) and not p.admitted and not p.staged and spans(p, range(36)) == taken


def test_a_full_cache_stages_the_rest_without_an_error():
    cap = sum((nbytes(r) + ALIGN - 1) // ALIGN * ALIGN for r in range(4)) + 64  # four pictures and a little
    c = PictureCache(cap, stage_bytes=1 << 17, prefetch=1, allocate=False)
    assert c.ring == 3 and c.arena_bytes == c.capacity_bytes + 3 * c.stage_bytes
    p = c.plan(range(9), size_of, region=1)
    assert p.admitted == [0, 1, 2, 3, 7] and p.staged == [4, 5, 6, 8]          # (5 x 3 still fits the little: later and smaller)
    base = c.region_base(1)
    assert base == c.capacity_bytes + c.stage_bytes and p.stage_start == base
    at = base
    for r in p.staged:
        assert p.table[r][0] == at and at % ALIGN == 0
        at = (at + nbytes(r) + ALIGN - 1) // ALIGN * ALIGN
    assert p.stage_end == p.table[8][0] + nbytes(8) <= base + c.stage_bytes
    assert all(e <= c.capacity_bytes for _, e in spans(p, p.admitted))
    c.commit(p)
    # the next epoch: the admitted rows hit, the others are staged again - never admitted, in whichever region
    for region in (2, 0):
        q = c.plan(range(9), size_of, region=region)
        assert sorted(q.hits) == [0, 1, 2, 3, 7] and not q.admitted and q.staged == [4, 5, 6, 8]
        assert q.stage_start == c.region_base(region) and q.admit_start == q.admit_end
        assert all(q.table[r] == p.table[r] for r in q.hits)
        c.commit(q)
    s = c.stats()
    assert (s.hits, s.misses, s.admitted, s.capacity) == (10, 9 + 4 + 4, 5, c.capacity_bytes)
    assert s.bytes_used == (p.admit_end + ALIGN - 1) // ALIGN * ALIGN <= c.capacity_bytes + ALIGN


def test_a_staging_overflow_names_the_flag_the_need_and_the_region():
    c = PictureCache(0, stage_bytes=8192, prefetch=2, allocate=False)
    assert c.plan([0, 1, 2], size_of).staged == [0, 1, 2]
    with pytest.raises(YkError, match=r'--cache_stage_mb.* need 11298 bytes.* holds 8192') as e:                # 48 + 3 * 50 * 75
        c.plan([0, 1, 3], lambda r: SIZES[r])
    assert 'raise --cache_stage_mb' in str(e.value)
    assert c.stats() == (0, 0, 0, 0, 0)                                        # a refused plan changes nothing


def test_capacity_zero_is_staging_only():
    c = PictureCache(0, stage_bytes=1 << 16, prefetch=2, allocate=False)
    assert c.capacity_bytes == 0 and c.ring == 4 and c.arena_bytes == 4 << 16
    for epoch in range(2):
        p = c.plan([2, 0, 1, 2], size_of, region=epoch)
        assert not p.hits and not p.admitted and p.staged == [2, 0, 1]          # the order of the rows is kept
        assert p.table[2][0] == c.region_base(epoch)
        c.commit(p)
    assert c.stats() == (0, 6, 0, 0, 0)
    assert c.lookup([0, 1, 2]) == {}


def test_the_same_inputs_give_the_same_plan_and_planning_changes_nothing():
    mk = lambda: PictureCache(40000, stage_bytes=1 << 16, prefetch=2, allocate=False)
    a, b = mk(), mk()
    for rows in ([5, 1, 8, 2], [8, 8, 3, 1], [11, 10, 9, 0]):
        pa, pa2, pb = a.plan(rows, size_of), a.plan(rows, size_of), b.plan(list(rows), size_of)
        assert pa == pa2 == pb
        a.commit(pa)
        b.commit(pb)
    assert a.stats() == b.stats() and a.lookup(range(12)) == b.lookup(range(12))
    # a decode that failed is not admitted: its bytes stay unused, the others are where the plan put them
    p = a.plan([4, 6], size_of)
    if p.admitted:
        a.commit(p, failed=[p.admitted[0]])
        assert p.admitted[0] not in a.lookup(p.admitted) and a.stats().bytes_used >= p.admit_end


def test_bad_sizes_are_refused_by_name():
    with pytest.raises(YkError, match='PictureCache'):
        PictureCache(-1, allocate=False)
    with pytest.raises(YkError, match='PictureCache'):
        PictureCache(0, stage_bytes=0, allocate=False)
    c = PictureCache(1024, stage_bytes=1024, allocate=False)
    with pytest.raises(YkError, match='row 3 is 0 x 5'):
        c.plan([3], lambda r: (0, 5))
    with pytest.raises(YkError, match='region 4 of 4'):
        c.plan([3], size_of, region=4)


def test_cli_knows_the_four_options_and_refuses_them_without_a_device(tmp_path):
    import torch
    from k210_yolo_framework_amd import training
    a = training.parser().parse_args([])
    assert (a.cache, a.cache_gb, a.cache_stage_mb, a.decode) == ('off', 8, 256, 'pil')
    a = training.parser().parse_args(['--cache', 'gpu', '--cache_gb', '0.5', '--cache_stage_mb', '64', '--decode', 'gpu'])
    assert (a.cache, a.cache_gb, a.cache_stage_mb, a.decode) == ('gpu', 0.5, 64.0, 'gpu')
    for bad in (['--cache', 'host'], ['--decode', 'turbo']):
        with pytest.raises(SystemExit):
            training.parser().parse_args(bad)
    mk = (ROOT / 'Makefile').read_text()
    assert '--cache $(CACHE) --cache_gb $(CACHEGB) --cache_stage_mb $(CACHESTAGE) --decode $(DECODE)' in mk
    for line in ('CACHE         ?= off', 'CACHEGB       ?= 8', 'CACHESTAGE    ?= 256', 'DECODE        ?= pil'):
        assert line in mk
    for flag, value in [('--cache_gb', '-1'), ('--cache_gb', 'nan'), ('--cache_stage_mb', '0'), ('--cache_stage_mb', 'inf')]:
        with pytest.raises(YkError, match=flag + ' '):              # refused by name, before anything needs a device
            training.cli(['--synthetic', '16', '--cache', 'gpu', flag, value, '--max_steps', '1', '--log_dir', str(tmp_path)])
    if not torch.cuda.is_available():
        with pytest.raises(YkError, match='--cache gpu'):
            training.cli(['--synthetic', '16', '--cache', 'gpu', '--max_steps', '1', '--log_dir', str(tmp_path)])
        with pytest.raises(YkError, match='--decode gpu'):
            training.cli(['--synthetic', '16', '--decode', 'gpu', '--max_steps', '1', '--log_dir', str(tmp_path)])
        with pytest.raises(YkError):
            PictureCache(1 << 20)                                   # an arena needs a device: never a host fallback
    assert not list(tmp_path.iterdir())
