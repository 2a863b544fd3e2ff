"""The five entry points that put the picture index in blockIdx.y and loop on the host past the 65535 rows of one launch -
yk_letterbox_ragged_u8, yk_letterbox_tiles_u8, yk_letterbox_views_u8, yk_mosaic_ragged_u8 (csrc/yk_pre.hip) and yk_draw_dets_u8
(csrc/yk_draw.hip) - at n = 65535 (one full launch), 65536 (a second launch of one row), 65538, and 131071 (a third launch, `base` added up
twice) for the ragged letterbox and the warped mosaic.  Every frame of every call is compared, as bytes, with the gather of
tests/grid_y_cases.py, whose frames are host references and in which a row never equals the row one or two launches before it
(tests/test_grid_y_cases.py): a `+ base` missing from any advanced pointer, or a wrong stride, shows on every row past the first launch.

The C entry points are called through engine.call on device tables built in one vectorised NumPy step.  The Python wrappers
(engine.letterbox_ragged_u8 and its kin) are bypassed on purpose: their per-row host checks would dominate the run time at 131071 rows, and
the bad rows below are exactly what they refuse.  Every output has one guard frame in front and one behind, filled with a sentinel like the
output itself; both must still hold it afterwards.

The second half feeds the two warp kernels (yk_letterbox_augment_u8, yk_mosaic_ragged_u8 with d_inv) maps no other test does: all zero,
translations of 1e12, scales of 1e-300 and 1e300, and maps that put a coordinate exactly on -1, dw - 1 and dw.  Their reference is
grid_y_cases.warp_loop, the header comment's arithmetic one pixel at a time."""
import ctypes as C

import numpy as np
import pytest

from tests import grid_y_cases as gy
from tests import letterbox_cases as lc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _rows_u8(t):
    import torch
    t = np.ascontiguousarray(t).reshape(-1)
    return torch.from_numpy(t.view(np.uint8).reshape(len(t), t.dtype.itemsize)).cuda()


class _Dev:
    """One kernel's device buffers at its largest n; a call of fewer rows reads their first n rows (row i depends on i alone)."""

    def __init__(self, kernel):
        import torch
        self.kernel, self.n = kernel, gy.LARGEST[kernel]
        self.H, self.W = gy.DST[kernel]
        self.per = 3 * self.H * self.W
        self.key = torch.from_numpy(gy.keys(self.n)).cuda()
        self.want = torch.from_numpy(gy.frames77(kernel).copy()).cuda()[self.key]               # the gather, on the device
        self.table = _rows_u8(gy.table(kernel, self.n))
        self.packed = torch.from_numpy(gy.pool()[2].copy()).cuda()
        if kernel in ('mosaic', 'mosaic_inv'):
            self.centre = torch.from_numpy(gy.centres77().copy()).cuda()[self.key].contiguous()
            self.inv = torch.from_numpy(gy.inv77().copy()).cuda()[self.key].contiguous() if kernel == 'mosaic_inv' else None
        if kernel == 'draw':
            dets, counts = gy.dets77()
            self.dets = torch.from_numpy(dets.copy()).cuda()[self.key].contiguous()
            self.counts = torch.from_numpy(counts.copy()).cuda()[self.key].contiguous()
            self.pictures = torch.from_numpy(gy.draw_pictures().copy()).cuda()[self.key // 11].contiguous()        # seven of them, by i % 7
            self.colours = torch.from_numpy(gy.COLOURS.copy()).cuda()

    def issue(self, n, out, stream=None):
        """The C call alone, writing n frames at `out` (for draw: painting the n pictures of the buffer that starts one picture before `out`)."""
        from k210_yolo_framework_amd import engine
        k, nb = self.kernel, self.packed.numel()
        if k == 'ragged':
            engine.call('yk_letterbox_ragged_u8', self.packed, nb, self.table, n, out, self.H, self.W, stream)
        elif k == 'tiles':
            engine.call('yk_letterbox_tiles_u8', self.packed, nb, self.table, n, out, self.H, self.W, stream)
        elif k == 'views':
            engine.call('yk_letterbox_views_u8', self.packed, nb, self.table, n, out, self.H, self.W, stream)
        elif k in ('mosaic', 'mosaic_inv'):
            engine.call('yk_mosaic_ragged_u8', self.packed, nb, self.table, self.centre, self.inv, n, out, self.H, self.W, stream)
        else:
            raise KeyError(k)

    def run(self, n):
        """-> the n frames [n, H, W, 3] of one call, the guards checked."""
        import torch
        from k210_yolo_framework_amd import engine
        assert 0 < n <= self.n
        buf = torch.full(((n + 2) * self.per,), SENTINEL, dtype=torch.uint8, device='cuda')
        if self.kernel == 'draw':
            buf[self.per:(n + 1) * self.per] = self.pictures[:n].reshape(-1)
            engine.call('yk_draw_dets_u8', buf, buf.numel(), self.table, n, self.dets, gy.CAP, self.counts, self.colours, len(gy.COLOURS), None, 0, 8,
                        self.H * self.W, None)
        else:
            self.issue(n, buf[self.per:])
        torch.cuda.synchronize()
        assert bool((buf[:self.per] == SENTINEL).all().item()), (self.kernel, n, 'the guard frame in front was written')
        assert bool((buf[(n + 1) * self.per:] == SENTINEL).all().item()), (self.kernel, n, 'the guard frame behind was written')
        return buf[self.per:(n + 1) * self.per].view(n, self.H, self.W, 3)


_DEVS = {}


@pytest.fixture(scope='module')
def dev():
    """kernel -> _Dev, each built once per module and dropped with it."""
    def get(kernel):
        if kernel not in _DEVS:
            _DEVS[kernel] = _Dev(kernel)
        return _DEVS[kernel]
    yield get
    _DEVS.clear()


def _where(got, want):
    """The first rows that differ, for the assertion message."""
    bad = (got != want).reshape(len(got), -1).any(1).nonzero().reshape(-1)
    return f'{bad.numel()} frames differ, the first at rows {bad[:6].tolist()}'


CALLS = [(k, n) for k in gy.KERNELS for n in gy.NS + ((gy.N_MAX,) if gy.LARGEST[k] == gy.N_MAX else ())]


@pytest.mark.parametrize('kernel,n', CALLS, ids=[f'{k}-{n}' for k, n in CALLS])
def test_every_frame_of_the_call_equals_the_gather(dev, kernel, n):
    """For draw the frames are the pictures themselves, painted in place: the whole buffer is compared, so a row painted into its neighbour's
    bytes shows."""
    import torch
    d = dev(kernel)
    got = d.run(n)
    assert torch.equal(got, d.want[:n]), (kernel, n, _where(got, d.want[:n]))


def _spoil(d, i):
    """Makes row i one the kernel must refuse (h = 0; for the mosaic kernels the row of quadrant BAD_QUADRANT) -> the bytes to put back."""
    r = 4 * i + gy.BAD_QUADRANT if d.kernel in ('mosaic', 'mosaic_inv') else i
    assert d.table.shape[1] in (40, 56)                            # yk_ragged_row_t, yk_tile_row_t, yk_view_row_t: int32 h at byte 8
    saved = d.table[r].clone()
    d.table[r, 8:12] = 0
    return r, saved


@pytest.mark.parametrize('kernel', ['ragged', 'tiles', 'views', 'mosaic', 'mosaic_inv'])
def test_a_bad_row_at_the_boundary_blanks_its_own_frame_and_no_other(dev, kernel):
    """Rows 65534 (the last of the first launch), 65535 and 65536 (the first two of the second) in turn: the bounds check reads the row the
    output belongs to."""
    import torch
    d = dev(kernel)
    n = gy.NS[-1]
    for i in gy.BAD_ROWS:
        r, saved = _spoil(d, i)
        try:
            got = d.run(n)
        finally:
            d.table[r] = saved
        want_i = torch.from_numpy(gy.slow_frame(kernel, i, bad=gy.BAD_QUADRANT)).cuda()
        assert not torch.equal(want_i, d.want[i])
        assert torch.equal(got[i], want_i), (kernel, i, got[i].cpu().tolist())
        if kernel not in ('mosaic', 'mosaic_inv'):
            assert not got[i].any().item()
        assert torch.equal(got[:i], d.want[:i]), (kernel, i, _where(got[:i], d.want[:i]))
        assert torch.equal(got[i + 1:], d.want[i + 1:n]), (kernel, i, _where(got[i + 1:], d.want[i + 1:n]))
    torch.cuda.synchronize()
    assert torch.equal(d.run(n), d.want[:n])                       # the table is whole again


def test_draw_counts_beyond_the_cap_and_below_zero_at_the_boundary(dev):
    """counts of cap + 5 at row 65535 and -3 at row 65536 are read as cap and 0.  Both rows hold two finite boxes for this, so that the clamp
    to cap paints both and the clamp to 0 paints neither; the neighbours are unchanged."""
    import torch
    d = dev('draw')
    n, (hi, lo) = gy.NS[-1], gy.BAD_ROWS[1:]
    boxes = gy.BOXES[2]
    assert len(boxes) == gy.CAP
    saved = d.dets[hi:lo + 1].clone(), d.counts[hi:lo + 1].clone()
    try:
        d.dets[hi:lo + 1] = torch.from_numpy(np.asarray(boxes, np.float32)).cuda()
        d.counts[hi:lo + 1] = torch.tensor([gy.CAP + 5, -3], dtype=torch.int32).cuda()
        got = d.run(n)
    finally:
        d.dets[hi:lo + 1], d.counts[hi:lo + 1] = saved
    want_hi = torch.from_numpy(gy.painted(hi % 7, boxes)).cuda()
    assert not torch.equal(want_hi, d.pictures[hi]) and not torch.equal(want_hi, d.want[hi])
    assert not np.array_equal(gy.painted(lo % 7, boxes), gy.draw_pictures()[lo % 7])        # painted, row 65536 would show it
    assert torch.equal(got[hi], want_hi), got[hi].cpu().tolist()
    assert torch.equal(got[lo], d.pictures[lo]), got[lo].cpu().tolist()
    assert torch.equal(got[:hi], d.want[:hi]) and torch.equal(got[lo + 1:], d.want[lo + 1:n])


def test_ragged_letterbox_of_65536_rows_recorded_in_a_graph_is_two_kernel_nodes_and_replays_on_changed_pixels(dev):
    import torch
    from k210_yolo_framework_amd import engine
    d = dev('ragged')
    n = gy.CHUNK + 1
    out = torch.zeros((n, d.H, d.W, 3), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    original = d.packed.clone()
    torch.cuda.synchronize()
    graph = engine.capture(st, lambda: d.issue(n, out, st))
    try:
        assert graph.kernel_nodes == 2
        stream.synchronize()
        assert not out.any().item()                                 # recorded, not executed
        for turn in range(2):
            eager = d.run(n).clone()
            graph.launch(st)
            stream.synchronize()
            assert eager.any().item() and torch.equal(out, eager), turn
            if turn == 0:
                assert torch.equal(out, d.want[:n])
                d.packed.copy_(255 - d.packed)                      # the replay reads the pixels that are there when it runs
                torch.cuda.synchronize()
            else:
                assert not torch.equal(out, d.want[:n])
    finally:
        graph.close()
        d.packed.copy_(original)
        torch.cuda.synchronize()


def test_two_runs_of_the_warped_mosaic_give_the_same_bytes(dev):
    import torch
    d = dev('mosaic_inv')
    a = d.run(gy.NS[-1]).clone()
    b = d.run(gy.NS[-1])
    assert torch.equal(a, b) and torch.equal(a, d.want[:gy.NS[-1]])


# ---------------------------------------------------------------------------------------------------- warp maps no other test feeds
B = 6


def _ordinary():
    from tests.test_gpu_letterbox_edges import _inverse_maps
    return _inverse_maps(gy.ROOM)[1]                                # identity, mirror, half-pixel shift, rotation, rotation x 1.25


class _Warp:
    """A batch of six 5 x 7 frames through one of the two warp kernels: `frames` are the unwarped frames from the host references."""

    def __init__(self, kernel):
        import torch
        self.kernel = kernel
        if kernel == 'augment':
            src = (3, 5)
            pics = np.stack([lc.picture(src, 'noise', v) for v in range(B)])
            self.frames = [lc.reference(p, gy.ROOM) for p in pics]
            self.src, self.d_src = src, torch.from_numpy(pics.copy()).cuda()
        else:
            first = 41                                              # six consecutive rows of the mosaic table: six seams, 24 pictures
            key = gy.keys(B, first=first)
            self.frames = list(gy.frames77('mosaic')[key])
            self.packed = torch.from_numpy(gy.pool()[2].copy()).cuda()
            self.table = _rows_u8(gy.rows77('mosaic')[key])
            self.centre = torch.from_numpy(gy.centres77()[key].copy()).cuda()
        assert all(f.any() for f in self.frames) and all(self.frames[s][0, 0].all() for s in (0, 3, 4))   # the slots whose map samples (0, 0)

    def run(self, maps):
        import torch
        from k210_yolo_framework_amd import engine
        H, W = gy.ROOM
        per = 3 * H * W
        d_inv = torch.from_numpy(np.ascontiguousarray(np.asarray(maps, np.float64).reshape(B, 6))).cuda()
        buf = torch.full(((B + 2) * per,), SENTINEL, dtype=torch.uint8, device='cuda')
        if self.kernel == 'augment':
            engine.call('yk_letterbox_augment_u8', self.d_src, B, self.src[0], self.src[1], d_inv, buf[per:], H, W, None)      # raises unless YK_OK
        else:
            engine.call('yk_mosaic_ragged_u8', self.packed, self.packed.numel(), self.table, self.centre, d_inv, B, buf[per:], H, W, None)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:per] == SENTINEL).all() and (host[(B + 1) * per:] == SENTINEL).all()
        return host[per:(B + 1) * per].reshape(B, H, W, 3)


def _batch(slot, hostile):
    """Five ordinary maps with `hostile` put in at `slot`."""
    maps = list(_ordinary())
    maps.insert(slot, np.asarray(hostile, np.float64))
    return maps


@pytest.mark.parametrize('kernel', ['augment', 'mosaic_inv'])
def test_finite_maps_far_outside_the_frame_and_exactly_on_its_edges_equal_the_stated_arithmetic(kernel):
    w = _Warp(kernel)
    for f in w.frames[:2]:                                          # the loop is the suite's warp reference on ordinary maps
        for M in _ordinary():
            assert np.array_equal(gy.warp_loop(f, M), lc.warp_reference(f, M))
    for k, (name, M) in enumerate(gy.hostile_maps().items()):
        slot = k % B
        maps = _batch(slot, M)
        got = w.run(maps)
        for j in range(B):
            want = gy.warp_loop(w.frames[j], maps[j])
            assert np.array_equal(got[j], want), (kernel, name, slot, j, got[j].tolist(), want.tolist())
            if j != slot:
                assert np.array_equal(want, lc.warp_reference(w.frames[j], maps[j]))
        f = w.frames[slot]
        if name in ('zero', 'scale_1e-300'):
            assert (got[slot] == f[0, 0]).all()                     # every output pixel samples the frame's (0, 0)
        if name in ('far', 'far_negative'):
            assert not got[slot].any()
        if name == 'scale_1e300':
            assert np.array_equal(got[slot][0, 0], f[0, 0]) and got[slot].reshape(-1, 3)[1:].max() == 0


@pytest.mark.parametrize('kernel', ['augment', 'mosaic_inv'])
def test_a_map_that_is_not_finite_is_answered_yk_ok_leaves_its_neighbours_alone_and_is_deterministic(kernel):
    """Read from the kernels: with a NaN or an infinity among the six entries every c or r of the frame is NaN or infinite (0 * inf and
    inf - inf are NaN), `tap >= 0.0 && tap < dh` is false for a NaN and for either infinity, so no tap is evaluated and (int) is applied to no
    such value; dc or dr is NaN, the blend is NaN, fmin(255.0, NaN) is 255.0 and the cast is of 255.0.  The project promises less - YK_OK, an
    unspecified but deterministic frame, nothing read - and only that is asserted.
    Observed on an MI355X: every byte of the hostile frame is 255, for every one of the five maps and both kernels."""
    w = _Warp(kernel)
    for k, (name, M) in enumerate(gy.nonfinite_maps().items()):
        slot = (k + 2) % B
        plain = w.run(_batch(slot, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
        a = w.run(_batch(slot, M))
        b = w.run(_batch(slot, M))
        print(kernel, name, 'hostile frame bytes:', np.unique(a[slot]).tolist())
        assert np.array_equal(plain[slot], w.frames[slot])
        for j in range(B):
            if j != slot:
                assert np.array_equal(a[j], plain[j]) and np.array_equal(b[j], plain[j]), (kernel, name, j)
        assert np.array_equal(a[slot], b[slot]), (kernel, name)
