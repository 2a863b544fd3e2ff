"""The four letterbox kernels of csrc/yk_pre.hip (letterbox_u8_kernel, letterbox_rows_u8_kernel<yk_ragged_row_t>, letterbox_augment_u8_kernel,
mosaic_ragged_u8_kernel: one letterbox_px behind all of them) against the host reference of tests/letterbox_cases.py at the sizes of its
table: single pixels, lines, slivers, upscales to 28-fold, exact scales 2 and 0.5, destinations smaller than a workgroup or no multiple of
one, constant-255 pictures whose blend falls an ulp short of 255, taps one past both edges, negative translations.

Every comparison is np.array_equal against reference() / warp_reference(); none is against another kernel's output, none has a tolerance.
tests/test_letterbox_cases.py holds the reference and the table's conditions on the CPU."""
import functools

import numpy as np
import pytest

from k210_yolo_framework_amd import augment, draw, mosaic
from tests import letterbox_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64


def _diff(got, want):
    """Where two pictures differ, for the assertion message."""
    bad = np.argwhere(got != want)
    return f'{len(bad)} bytes differ, first at (y, x, ch) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}' if len(bad) else ''


@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_letterbox_u8_equals_the_reference_and_stays_inside_its_destination(case):
    import torch
    from k210_yolo_framework_amd import engine
    (sh, sw), (dh, dw) = case.src, case.dst
    n = 3 * dh * dw * 3
    for content in lc.CONTENTS:
        frames = torch.from_numpy(lc.batch(case.src, content).copy()).cuda()
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
        engine.call('yk_letterbox_u8', frames, 3, sh, sw, buf[GUARD:], dh, dw, None)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), (case, content)
        got, want = host[GUARD:GUARD + n].reshape(3, dh, dw, 3), lc.expected_batch(case.src, case.dst, content)
        for b in range(3):
            assert np.array_equal(got[b], want[b]), (case, content, b, _diff(got[b], want[b]))


@pytest.mark.parametrize('dst', sorted({c.dst for c in lc.CASES}), ids=lambda d: f'{d[0]}x{d[1]}')
def test_letterbox_ragged_u8_equals_the_reference_per_picture(dst):
    """All sources of one destination, every content of each, back to back in ONE launch; each image against the reference (not against
    yk_letterbox_u8).  The rows the launch reads are the ones engine.ragged_table_to_device had yk_letterbox_ragged_params fill."""
    import torch
    from k210_yolo_framework_amd import engine
    pics = [(c.src, content) for c in lc.CASES if c.dst == dst for content in lc.CONTENTS]
    packed, table, _ = draw.pack_ragged([lc.picture(src, content) for src, content in pics])
    assert any(int(o) % 2 for o in table['offset'])                 # back to back, 3-byte pixels: odd offsets
    d_packed = packed.cuda()
    d_table = engine.ragged_table_to_device(table, dst, d_packed.numel(), d_packed.device)
    out = engine.letterbox_ragged_u8(d_packed, d_table, dst)
    torch.cuda.synchronize()
    rows = d_table.cpu().numpy().reshape(-1).view(draw.RAGGED_DTYPE)
    out = out.cpu().numpy()
    assert out.shape == (len(pics), *dst, 3) and len(rows) == len(pics)
    for i, (src, content) in enumerate(pics):
        scale, tx, ty = lc.params(src, dst)
        r = rows[i]
        assert (int(r['offset']), int(r['h']), int(r['w'])) == (int(table[i]['offset']), *src)
        assert np.float64(r['scale']).view(np.uint64) == np.float64(scale).view(np.uint64) and (int(r['tx']), int(r['ty'])) == (tx, ty), (src, r)
        want = lc.expected(src, dst, content)
        assert np.array_equal(out[i], want), (src, dst, content, _diff(out[i], want))


AUGMENT_CASES = [((1, 1), (7, 5)), ((2, 2), (56, 80)), ((9, 13), (255, 257)), ((640, 7), (56, 80))]


def _inverse_maps(dst):
    """-> (names, M [5, 2, 3]): identity, horizontal mirror, translation by (0.5, 0.25), a rotation augment.py draws from a fixed seed, and
    that rotation scaled by 1.25 about the frame's centre."""
    H, W = dst
    u = augment.param_table(7, 0, 2)
    u[0, 0], u[1, 0], u[1, 1] = 0.4, 0.05, 0.2                      # row 0: the rotation branch; row 1: the flip branch, flipping
    branch, flip = augment.decode(u)[:2]
    assert branch.tolist() == [augment.ROTATE, augment.FLIP] and flip[1]
    drawn = augment.matrices(u, dst)[2]
    rot, mirror = drawn[0], np.array([[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0]])
    assert rot[0, 1] != 0.0 and rot[0, 1] == -rot[1, 0] and np.array_equal(drawn[1], mirror)
    A = 1.25 * rot[:, :2]
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    scaled = np.concatenate([A, (c - A @ c)[:, None]], 1)
    M = np.stack([np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), mirror, np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]), rot, scaled])
    return ('identity', 'mirror', 'shift', 'rotation', 'rotation x 1.25'), np.ascontiguousarray(M)


@pytest.mark.parametrize('src,dst', AUGMENT_CASES, ids=[f'{s[0]}x{s[1]}-{d[0]}x{d[1]}' for s, d in AUGMENT_CASES])
def test_letterbox_augment_u8_equals_the_reference_then_the_warp(src, dst):
    import torch
    from k210_yolo_framework_amd import engine
    assert any(c.src == src and c.dst == dst for c in lc.CASES)
    names, M = _inverse_maps(dst)
    d_inv = torch.from_numpy(M).cuda()
    for content in lc.CONTENTS:
        img, box = lc.picture(src, content), lc.expected(src, dst, content)
        frames = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (len(M), *img.shape)))).cuda()
        out = engine.letterbox_augment_u8(frames, dst, d_inv)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert out.shape == (len(M), *dst, 3)
        for k, name in enumerate(names):
            want = lc.warp_reference(box, M[k])
            assert np.array_equal(out[k], want), (src, dst, content, name, _diff(out[k], want))
        assert np.array_equal(out[0], box) and np.array_equal(out[1], box[:, ::-1])       # exact copies of the letterbox and of its mirror
        if content != 'white' or src != (1, 1):
            assert not np.array_equal(out[2], box) and not np.array_equal(out[3], out[4])


MOSAIC_DST = (56, 80)
MOSAIC_SRC = [(1, 1), (37, 1), (3, 5), (640, 7)]                    # quadrants 0 (top left) .. 3 (bottom right)
MOSAIC_GAINS = (1.0, 0.5, 1.0, 0.75)
HALF_PIXEL = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]])


@functools.lru_cache(maxsize=None)
def _mosaic_batch():
    """Twelve samples - three contents x four seams - over twelve pictures packed back to back.  -> (packed torch uint8, the kernel's table
    [48] with rows from yk_mosaic_params, seams int32 [12, 2], the frames assembled from reference() [12, H, W, 3])."""
    from k210_yolo_framework_amd import engine
    H, W = MOSAIC_DST
    assert all(any(c.src == s for c in lc.CASES) for s in MOSAIC_SRC)
    seams = [(0, 0), (W, H), (1, H - 1), (W // 2, H // 2)]
    pics = [lc.picture(src, content) for content in lc.CONTENTS for src in MOSAIC_SRC]
    packed, ptable, _ = draw.pack_ragged(pics)
    assert any(int(o) % 2 for o in ptable['offset'])
    gains = np.array(MOSAIC_GAINS, np.float64)
    table, centres, frames = [], [], []
    for ci in range(len(lc.CONTENTS)):
        for cx, cy in seams:
            rows4 = ptable[4 * ci:4 * ci + 4].copy()
            engine.call('yk_mosaic_params', rows4, cx, cy, gains, H, W)
            frame = np.zeros((H, W, 3), np.uint8)
            for k in range(4):
                want = mosaic.quadrant_params(MOSAIC_SRC[k], k, cx, cy, gains[k], MOSAIC_DST)     # the C rows are the Python geometry's
                assert (float(rows4[k]['scale']), int(rows4[k]['tx']), int(rows4[k]['ty'])) == want, (k, rows4[k], want)
                ys, xs = (slice(cy, H) if k & 2 else slice(0, cy)), (slice(cx, W) if k & 1 else slice(0, cx))
                frame[ys, xs] = lc.reference(pics[4 * ci + k], MOSAIC_DST, float(rows4[k]['scale']), int(rows4[k]['tx']), int(rows4[k]['ty']))[ys, xs]
            table.append(rows4)
            centres.append((cx, cy))
            frames.append(frame)
    table = np.concatenate(table)
    assert (table['tx'] < 0).any() and (table['ty'] < 0).any()
    centre_seam = np.stack(frames[3::4])                             # the samples cut at the middle: every quadrant shows its picture
    assert all(centre_seam[:, ys, xs].any() for ys in (slice(0, H // 2), slice(H // 2, H)) for xs in (slice(0, W // 2), slice(W // 2, W)))
    return packed, table, np.array(centres, np.int32), np.stack(frames)


def test_mosaic_ragged_u8_quadrants_equal_the_reference_with_each_rows_parameters():
    import torch
    from k210_yolo_framework_amd import engine
    packed, table, centres, frames = _mosaic_batch()
    out = engine.mosaic_ragged_u8(packed.cuda(), table, centres, MOSAIC_DST)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == frames.shape
    for b in range(len(frames)):
        cx, cy = centres[b]
        for k in range(4):
            ys, xs = (slice(cy, None) if k & 2 else slice(0, cy)), (slice(cx, None) if k & 1 else slice(0, cx))
            assert np.array_equal(out[b][ys, xs], frames[b][ys, xs]), (b, k, centres[b].tolist(), table[4 * b + k], _diff(out[b][ys, xs], frames[b][ys, xs]))


def test_mosaic_ragged_u8_with_an_inverse_map_equals_the_warp_of_the_assembled_frame():
    import torch
    from k210_yolo_framework_amd import engine
    packed, table, centres, frames = _mosaic_batch()
    inv = np.ascontiguousarray(np.broadcast_to(HALF_PIXEL, (len(frames), 2, 3)))
    out = engine.mosaic_ragged_u8(packed.cuda(), table, centres, MOSAIC_DST, inv=torch.from_numpy(inv).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for b in range(len(frames)):
        want = lc.warp_reference(frames[b], HALF_PIXEL)
        assert np.array_equal(out[b], want), (b, centres[b].tolist(), _diff(out[b], want))
        assert not np.array_equal(want, frames[b])
