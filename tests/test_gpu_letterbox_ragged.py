"""yk_letterbox_ragged_u8: pictures of different sizes letterboxed by ONE launch.  Image i of the result equals yk_letterbox_u8 on picture i
alone, bit for bit - against the real scikit-image (tests/golden/letterbox_golden.npz, the bar of test_gpu_pre.py) and against
engine.letterbox_u8 per picture on seeded noise."""
import ctypes as C

import numpy as np
import pytest

from k210_yolo_framework_amd import draw

pytestmark = pytest.mark.gpu
DST = (224, 320)
# sizes at which the ragged launch could part from yk_letterbox_u8: single pixels and lines, one less / equal / one more than the network
# size (equal = identity), both orientations of a VOC picture, a sliver, and a picture larger than the network size in both dimensions.
# These comparisons are against yk_letterbox_u8, a kernel with the same letterbox_px: they hold the table, the offsets and the indexing, not
# the arithmetic.  The independent check of the arithmetic at such sizes is tests/test_gpu_letterbox_edges.py (table: tests/letterbox_cases.py).
SIZES = [(1, 1), (1, 37), (37, 1), (223, 319), (224, 320), (225, 321), (500, 375), (375, 500), (640, 7), (300, 400)]


def _per_image(engine, torch, imgs, dst):
    return [engine.letterbox_u8(torch.from_numpy(np.ascontiguousarray(im[None])).cuda(), dst)[0].cpu().numpy() for im in imgs]


def test_golden_pictures_in_one_ragged_batch_bit_exact_vs_skimage(golden_dir):
    import torch
    from k210_yolo_framework_amd import engine
    g = np.load(golden_dir / 'letterbox_golden.npz')
    n = 0
    while f'img{n}' in g.files:
        n += 1
    assert n >= 6
    # every source picture of the file in ONE ragged batch; the file's outputs have several network sizes, and a launch has one, so the
    # same batch is launched once per size and each picture is held to its golden output at the size the file recorded for it
    packed, table, _ = draw.pack_ragged([np.ascontiguousarray(g[f'img{i}']) for i in range(n)])
    d_packed = packed.cuda()
    checked = 0
    for dst in sorted({(int(g[f'par{i}'][3]), int(g[f'par{i}'][4])) for i in range(n)}):
        out = engine.letterbox_ragged_u8(d_packed, table, dst)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert out.shape == (n, *dst, 3)
        for i in range(n):
            if (int(g[f'par{i}'][3]), int(g[f'par{i}'][4])) == dst:
                np.testing.assert_array_equal(out[i], g[f'out{i}'], err_msg=f'case {i} {g[f"img{i}"].shape}')
                checked += 1
    assert checked == n


@pytest.mark.parametrize('case', ['n1', 'mixed', 'n33', 'gaps'])
def test_seeded_ragged_batch_equals_letterbox_u8_per_picture(case):
    import torch
    from k210_yolo_framework_amd import engine
    rng = np.random.default_rng(5)
    if case == 'n1':
        shapes, gap = [(97, 131)], 0
    elif case == 'n33':                                             # more pictures than any one size list: 33 small ones, odd sizes
        shapes, gap = [(int(rng.integers(1, 60)), int(rng.integers(1, 60))) for _ in range(33)], 0
    else:
        shapes, gap = SIZES, (7 if case == 'gaps' else 0)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    packed, table, _ = draw.pack_ragged(imgs, gap=gap)
    if gap == 0 and len(shapes) > 1:
        assert any(int(o) % 2 for o in table['offset'])             # back to back: odd offsets
    d_packed = packed.cuda()
    if gap:
        flat = packed.numpy()
        ends = [int(r['offset']) + 3 * int(r['h']) * int(r['w']) for r in table]
        for e in ends[:-1]:
            flat[e:e + gap] = 255                                   # (a gap byte that leaked into a picture would show)
        d_packed = torch.from_numpy(flat.copy()).cuda()
    out = engine.letterbox_ragged_u8(d_packed, table, DST)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (len(shapes), *DST, 3)
    for i, ref in enumerate(_per_image(engine, torch, imgs, DST)):
        assert np.array_equal(out[i], ref), (case, i, shapes[i])
    if case == 'mixed':
        assert np.array_equal(out[SIZES.index((224, 320))], imgs[SIZES.index((224, 320))])      # the identity


def test_recorded_in_a_graph_and_replayed_gives_the_same_bytes():
    import torch
    from k210_yolo_framework_amd import engine
    rng = np.random.default_rng(9)
    shapes = [(37, 1), (225, 321), (97, 131), (1, 1)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    packed, table, _ = draw.pack_ragged(imgs)
    d_packed = packed.cuda()
    d_table = engine.ragged_table_to_device(table, DST, d_packed.numel(), d_packed.device)
    eager = engine.letterbox_ragged_u8(d_packed, d_table, DST)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    issue = lambda: engine._check(engine.lib().yk_letterbox_ragged_u8(C.c_void_p(d_packed.data_ptr()), C.c_size_t(d_packed.numel()),
                                                                      C.c_void_p(d_table.data_ptr()), C.c_int(len(shapes)), C.c_void_p(out.data_ptr()),
                                                                      C.c_int(DST[0]), C.c_int(DST[1]), st), 'yk_letterbox_ragged_u8')
    graph = engine.capture(st, issue)                               # yk_graph_begin / yk_graph_end around the launch, as Pipeline records a step
    try:
        assert graph.kernel_nodes == 1
        stream.synchronize()
        assert not out.any().item()                                 # recorded, not executed
        for _ in range(2):
            graph.launch(st)
            stream.synchronize()
            assert torch.equal(out, eager)
            out.zero_()
            torch.cuda.synchronize()
    finally:
        graph.close()


def test_bad_arguments_are_refused_not_run():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    img = np.full((4, 5, 3), 9, np.uint8)
    packed, table, _ = draw.pack_ragged([img])
    d_packed = packed.cuda()
    d_table = engine.ragged_table_to_device(table, DST, d_packed.numel(), d_packed.device)
    out = torch.empty((1, *DST, 3), dtype=torch.uint8, device='cuda')
    p, t, o, nb = C.c_void_p(d_packed.data_ptr()), C.c_void_p(d_table.data_ptr()), C.c_void_p(out.data_ptr()), C.c_size_t(d_packed.numel())
    call = lambda p_, nb_, t_, n_, o_, h_, w_: L.yk_letterbox_ragged_u8(p_, nb_, t_, C.c_int(n_), o_, C.c_int(h_), C.c_int(w_), None)
    assert call(p, nb, t, 1, o, *DST) == 0
    for args in [(None, nb, t, 1, o, *DST), (p, nb, None, 1, o, *DST), (p, nb, t, 1, None, *DST), (p, nb, t, 0, o, *DST),
                 (p, nb, t, -1, o, *DST), (p, nb, t, 1, o, 0, 320), (p, nb, t, 1, o, 224, -3), (p, C.c_size_t(0), t, 1, o, *DST)]:
        assert call(*args) == -10                                   # YK_ERR_ARG
        assert b'yk_letterbox_ragged_u8' in L.yk_last_error()
    torch.cuda.synchronize()
    # what the C call cannot see - the rows of a DEVICE table - the wrapper refuses on the host table
    for field, value in (('h', 0), ('w', -2)):
        bad = table.copy()
        bad[0][field] = value
        with pytest.raises(engine.YkError):
            engine.letterbox_ragged_u8(d_packed, bad, DST)
    beyond = table.copy()
    beyond[0]['offset'] = 1                                         # the picture would end one byte past the buffer
    with pytest.raises(engine.YkError):
        engine.letterbox_ragged_u8(d_packed, beyond, DST)
    with pytest.raises(engine.YkError):
        engine.letterbox_ragged_u8(d_packed, table[:0], DST)
    host = np.zeros(1, draw.RAGGED_DTYPE)                            # the host helper itself names the row
    assert L.yk_letterbox_ragged_params(host.ctypes.data_as(C.c_void_p), C.c_int(1), C.c_int(224), C.c_int(320)) == -10
    assert L.yk_letterbox_ragged_params(None, C.c_int(1), C.c_int(224), C.c_int(320)) == -10
