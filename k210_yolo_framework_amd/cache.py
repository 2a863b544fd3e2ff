"""The device-resident picture cache of the training input pipeline (`make train CACHE=gpu`; not in the reference): every
picture of the training list is decoded once, kept in HBM as [h, w, 3] uint8, and every later batch is composed from there by one launch
of a ragged kernel - no file is read, nothing is decoded and no pixel crosses PCIe from the second epoch on.

The arena.  ONE device allocation of capacity_bytes + ring * stage_bytes uint8, because the ragged kernels (yk_letterbox_ragged_u8,
yk_mosaic_ragged_u8, include/yolo_hip.h) take one (d_src, src_bytes) and address pictures by 64-bit byte offsets:

  [0, capacity_bytes)                          the persistent part: a write-once bump allocator, every picture at a 16-byte aligned offset,
                                               keyed by dataset row -> (offset, h, w).  Nothing is evicted: a picture that no longer fits is
                                               never admitted (the bump pointer only grows), which is no error - it is staged every time.
  [capacity_bytes + k * stage_bytes, ... + stage_bytes), k = 0 .. ring - 1
                                               the staging ring, ring = prefetch + 2 regions: the pictures of ONE batch that are not in the
                                               persistent part live in one region, for that batch only.

Ordering.  A region is handed out again (`acquire`) only after the event recorded behind the launch that read it (`release`) has completed
- the discipline of pipeline.py's pinned slots; prefetch + 2 regions are more than the batches that can be outstanding (the queue's
`prefetch`, the one being produced, the one being consumed), so the wait is normally over before it starts.  The persistent part is
written once per picture, on the producer's stream in front of the launch that first reads it; `commit` keeps the event behind that write
and a pipeline on another stream (the next epoch's) waits for `last_write()` before it reads.

Planning is pure host arithmetic (`plan`; tests/test_cache.py runs it without a device): the same state and the same rows give the same
plan, the admissions of one batch are one contiguous run of the persistent part and the staged pictures one contiguous run of the region,
in the order of the rows given, so that one copy (or one decode call) fills each.  `plan` changes nothing; `commit` records what was
really brought in (a picture whose decode failed is left out: its bytes stay unused).

capacity_bytes = 0 is legal: staging only, what `DECODE=gpu CACHE=off` runs on.  The cache outlives the per-epoch InputPipeline objects
(the training loop owns it) and is safe against the one producer thread per pipeline.  Under data-parallel training every rank caches the
rows it meets; the rows rotate between the ranks from epoch to epoch, so the hit rate grows over the epochs instead of jumping to 1."""
from __future__ import annotations

import threading
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

from .engine import YkError

ALIGN = 16


def align(v: int) -> int:
    return (int(v) + ALIGN - 1) & ~(ALIGN - 1)


class Plan(NamedTuple):
    """What `PictureCache.plan` answers for the distinct rows of one batch."""
    hits: List[int]                             # rows found in the persistent part
    admitted: List[int]                         # rows that enter it now: back to back (16-byte aligned) in [admit_start, admit_end)
    staged: List[int]                           # rows that live in the region for this batch: likewise in [stage_start, stage_end)
    table: Dict[int, Tuple[int, int, int]]      # row -> (byte offset in the arena, h, w), for every row of the three lists
    admit_start: int
    admit_end: int
    stage_start: int
    stage_end: int


class Stats(NamedTuple):
    hits: int               # distinct pictures of a batch served from the persistent part
    misses: int             # ... that had to be brought in (admitted or staged)
    admitted: int           # pictures in the persistent part
    bytes_used: int         # its bump pointer
    capacity: int


class PictureCache:
    def __init__(self, capacity_bytes: int, stage_bytes: int = 256 << 20, prefetch: int = 2, device: Optional[int] = None,
                 allocate: bool = True, _first_offset: int = 0):
        """allocate=False: the planner alone, no device.  _first_offset (tests only): where the bump allocator starts."""
        if int(capacity_bytes) < 0 or int(stage_bytes) <= 0 or int(prefetch) < 1:
            raise YkError(f'PictureCache: capacity {capacity_bytes} bytes, staging regions of {stage_bytes} bytes, prefetch {prefetch}')
        self.capacity_bytes = align(capacity_bytes)
        self.stage_bytes = align(stage_bytes)
        self.ring = int(prefetch) + 2
        self.arena_bytes = self.capacity_bytes + self.ring * self.stage_bytes
        self._lock = threading.Lock()
        self._entries: Dict[int, Tuple[int, int, int]] = {}
        self._bump = align(_first_offset)
        self._hits = self._misses = 0
        self._events = [None] * self.ring
        self._tick = 0
        self._written = None
        self.arena = None
        self.device = None
        if allocate:
            self._allocate(device)

    def _allocate(self, device) -> None:
        import torch
        from . import engine
        engine.require_gpu()
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        free, _ = torch.cuda.mem_get_info(self.device)
        what = (f'picture cache: --cache_gb asks for {self.capacity_bytes} bytes and the {self.ring} staging regions (--cache_stage_mb) for '
                f'{self.ring * self.stage_bytes} more, {self.arena_bytes} bytes in one allocation')
        if self.arena_bytes > free:
            raise YkError(f'{what}: the device has {int(free)} bytes free')
        try:
            self.arena = torch.empty(self.arena_bytes, dtype=torch.uint8, device=self.device)
        except RuntimeError as e:                                               # (fragmentation: free in total, not in one piece)
            raise YkError(f'{what}: the device has {int(free)} bytes free and refused it ({str(e).splitlines()[0]})') from e

    # ---- host planning ---------------------------------------------------------------------------------------------------------
    def region_base(self, region: int) -> int:
        if not 0 <= int(region) < self.ring:
            raise YkError(f'PictureCache: region {region} of {self.ring}')
        return self.capacity_bytes + int(region) * self.stage_bytes

    def lookup(self, rows: Sequence[int]) -> Dict[int, Tuple[int, int, int]]:
        """The rows of `rows` that are in the persistent part -> (offset, h, w)."""
        with self._lock:
            return {int(r): self._entries[int(r)] for r in rows if int(r) in self._entries}

    def plan(self, rows: Sequence[int], size_of: Callable[[int], Tuple[int, int]], region: int = 0) -> Plan:
        """Where the pictures of dataset rows `rows` (repeats count once; order kept) are or go: size_of(row) -> (h, w) is asked for the
        rows that are not cached.  Pure: nothing changes until `commit`.  Staged pictures that exceed one region raise YkError."""
        base = self.region_base(region)
        with self._lock:
            hits, admitted, staged, table = [], [], [], {}
            bump = admit_start = self._bump
            at = base
            for r in rows:
                r = int(r)
                if r in table:
                    continue
                if r in self._entries:
                    hits.append(r)
                    table[r] = self._entries[r]
                    continue
                h, w = (int(v) for v in size_of(r)[:2])
                if h <= 0 or w <= 0:
                    raise YkError(f'PictureCache: row {r} is {h} x {w}')
                nbytes = 3 * h * w
                if bump + nbytes <= self.capacity_bytes:
                    admitted.append(r)
                    table[r] = (bump, h, w)
                    bump = align(bump + nbytes)
                else:
                    staged.append(r)
                    table[r] = (at, h, w)
                    at = align(at + nbytes)
            need = table[staged[-1]][0] + 3 * table[staged[-1]][1] * table[staged[-1]][2] - base if staged else 0
            if need > self.stage_bytes:
                raise YkError(f'--cache_stage_mb: the {len(staged)} pictures of this batch that are not in the cache need {need} bytes, a '
                              f'staging region holds {self.stage_bytes}; raise --cache_stage_mb to at least {(need + (1 << 20) - 1) >> 20}')
            admit_end = table[admitted[-1]][0] + 3 * table[admitted[-1]][1] * table[admitted[-1]][2] if admitted else admit_start
            return Plan(hits, admitted, staged, table, admit_start, admit_end, base, base + need)

    def commit(self, plan: Plan, failed: Sequence[int] = (), event=None) -> None:
        """The batch of `plan` has been brought in (its copies and decodes are queued in front of `event`): its admissions are cached from
        now on, all but the rows of `failed`, whose bytes stay unused."""
        with self._lock:
            if plan.admitted:
                if plan.admit_start != self._bump:
                    raise YkError('PictureCache: two producers planned at once (one pipeline at a time feeds a cache)')
                for r in plan.admitted:
                    if r not in failed:
                        self._entries[r] = plan.table[r]
                self._bump = align(plan.admit_end)
                if event is not None:
                    self._written = event
            self._hits += len(plan.hits)
            self._misses += len(plan.admitted) + len(plan.staged)

    def stats(self) -> Stats:
        with self._lock:
            return Stats(self._hits, self._misses, len(self._entries), self._bump, self.capacity_bytes)

    # ---- the staging ring and the device ---------------------------------------------------------------------------------------
    def acquire(self) -> int:
        """The next staging region, once the launch that last read it has completed."""
        with self._lock:
            k = self._tick % self.ring
            self._tick += 1
            ev, self._events[k] = self._events[k], None
        if ev is not None:
            ev.synchronize()
        return k

    def release(self, region: int, event) -> None:
        """`event` was recorded behind the last launch that reads `region`."""
        with self._lock:
            self._events[int(region)] = event

    def last_write(self):
        """The event behind the newest write of the persistent part (None: nothing written): a reader on another stream waits for it."""
        with self._lock:
            return self._written

    def read(self, row: int):
        """The cached picture of dataset row `row` as a device view [h, w, 3] of the arena."""
        with self._lock:
            off, h, w = self._entries[int(row)]
        return self.arena[off:off + 3 * h * w].view(h, w, 3)

    def close(self) -> None:
        """Free the arena, after everything that reads it has completed."""
        with self._lock:
            events, self._events = [e for e in self._events if e is not None], [None] * self.ring
            arena, self.arena = self.arena, None
            self._entries.clear()
        for e in events:
            e.synchronize()
        if arena is not None:
            import torch
            torch.cuda.synchronize(self.device)
            del arena

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
