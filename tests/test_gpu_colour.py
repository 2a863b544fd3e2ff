"""HSV colour jitter on the GPU: yk_hsv_jitter_u8 bit for bit against its host copy (colour.jitter_u8) on a lattice of colours and on
batches of odd shapes, the exact properties on the device output itself, the sample index past 65535, rows the kernel must not follow, bad
arguments, graph capture, InputPipeline(hsv=...) against the host generator on every rank, and `--hsv True` end to end."""
import ctypes as C
import re

import numpy as np
import pytest

from k210_yolo_framework_amd import colour, mosaic

pytestmark = pytest.mark.gpu

HW = (224, 320)
LEVELS = sorted(set(range(0, 256, 8)) | {1, 2, 127, 128, 254, 255})
ROWS = [(0.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0 / 3.0, 1.0, 1.0), (0.1, 1.5, 1.5), (-0.1, 1.0 / 1.5, 1.0 / 1.5), (0.0371, 1.234, 0.777),
        (0.5, 0.0, 1.0), (0.0, 1.0, 4.0)]
_cache = {}


def lattice_frame() -> np.ndarray:
    """Every combination of LEVELS as ONE frame [37, 37 * 37, 3] (37 levels: 128 is a multiple of 8 already): every grey level of LEVELS,
    every sector boundary of the hue circle, both ends; 1369 pixels a row, 198 blocks of 256 with a ragged last one."""
    if 'frame' not in _cache:
        a = np.array(LEVELS, np.uint8)
        _cache['frame'] = np.ascontiguousarray(np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(len(a), len(a) ** 2, 3))
        _cache['frame'].setflags(write=False)
    return _cache['frame']


def host(row) -> np.ndarray:
    """colour.jitter_u8 of the lattice frame, computed once per row and shared."""
    if row not in _cache:
        _cache[row] = colour.jitter_u8(lattice_frame(), row)
        _cache[row].setflags(write=False)
    return _cache[row]


def _device(frames: np.ndarray, params) -> np.ndarray:
    import torch
    from k210_yolo_framework_amd import engine
    d = torch.from_numpy(np.array(frames)).cuda()
    out = engine.hsv_jitter_u8(d, params)
    assert out is d                                                 # in place
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize('row', ROWS, ids=[f'{r[0]:.4g}_{r[1]:.4g}_{r[2]:.4g}' for r in ROWS])
def test_kernel_is_bit_exact_against_the_host_copy_on_the_lattice(row):
    L = lattice_frame()
    assert L.shape == (37, 1369, 3)
    got = _device(L[None], np.array([row]))[0]
    np.testing.assert_array_equal(got, host(row))
    if row == ROWS[0] or row == ROWS[1]:
        np.testing.assert_array_equal(got, L)                       # (a) neutral, (b) a whole turn: every colour unchanged
    elif row == ROWS[2]:
        np.testing.assert_array_equal(got, L[..., [2, 0, 1]])       # (c) a third of a turn: (r, g, b) -> (b, r, g)
    else:
        assert not np.array_equal(got, L)
    if row == ROWS[6]:                                              # gs = 0: the value in all three channels
        np.testing.assert_array_equal(got, np.repeat(L.max(-1, keepdims=True), 3, -1))
    grey = (L[..., 0] == L[..., 1]) & (L[..., 1] == L[..., 2])       # grey stays grey, min(255, floor(V gv + 0.5))
    want = np.minimum(255, np.floor(L[grey][:, 0].astype(np.float64) * row[2] + 0.5)).astype(np.uint8)
    np.testing.assert_array_equal(got[grey], np.repeat(want[:, None], 3, 1))


def test_a_whole_turn_backwards_on_the_device_returns_every_colour():
    L = lattice_frame()
    np.testing.assert_array_equal(_device(L[None], np.array([(-1.0, 1.0, 1.0)]))[0], L)


@pytest.mark.parametrize('n, hw', [(3, (5, 7)), (2, (1, 1)), (4, (24, 40))])
def test_every_sample_follows_its_own_row_at_sizes_that_fill_no_block(n, hw):
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, (n, *hw, 3), dtype=np.uint8)
    params = np.array([ROWS[3], ROWS[0], ROWS[5], ROWS[4]][:n])     # the second sample's row is neutral
    got = _device(frames, params)
    for k in range(n):
        np.testing.assert_array_equal(got[k], colour.jitter_u8(frames[k], params[k]), err_msg=f'sample {k}')
    np.testing.assert_array_equal(got[1], frames[1])                # between jittered neighbours, untouched
    assert not np.array_equal(got[0], frames[0])
    # a device table gives the same bytes as the host array
    import torch
    np.testing.assert_array_equal(_device(frames, torch.from_numpy(params).cuda()), got)


def test_sample_index_past_65535():
    n = 65537
    frames = np.random.default_rng(1).integers(0, 256, (n, 1, 1, 3), dtype=np.uint8)
    params = np.tile(np.array([ROWS[0], ROWS[2]]), (n // 2 + 1, 1))[:n]
    got = _device(frames, params)
    np.testing.assert_array_equal(got[0::2], frames[0::2])
    np.testing.assert_array_equal(got[1::2], frames[1::2][..., [2, 0, 1]])
    assert not np.array_equal(got[65535], frames[65535]) and np.array_equal(got[65536], frames[65536])


def test_a_row_the_kernel_must_not_follow_leaves_only_its_own_frame():
    import torch
    frames = np.random.default_rng(2).integers(1, 256, (10, 5, 7, 3), dtype=np.uint8)
    good = ROWS[3]
    bad = {1: (np.nan, 1.5, 1.5), 2: (0.1, np.inf, 1.5), 4: (0.1, 1.5, -np.inf), 5: (0.1, -0.5, 1.5), 6: (0.1, 1.5, -1e-300), 8: (-np.inf, 1.0, np.nan)}
    params = np.array([bad.get(k, good) for k in range(len(frames))])
    got = _device(frames, torch.from_numpy(params).cuda())          # a device table: the kernel's own check
    for k in range(len(frames)):
        if k in bad:
            np.testing.assert_array_equal(got[k], frames[k], err_msg=f'row {params[k]}')
        else:
            np.testing.assert_array_equal(got[k], colour.jitter_u8(frames[k], good))
            assert not np.array_equal(got[k], frames[k])


def test_bad_arguments_are_refused_not_run():
    import torch
    from k210_yolo_framework_amd import engine
    L = engine.lib()
    src = np.random.default_rng(3).integers(1, 256, (2, 5, 7, 3), dtype=np.uint8)
    f, p = torch.from_numpy(src).cuda(), torch.from_numpy(np.array([ROWS[3], ROWS[4]])).cuda()
    assert L.yk_hsv_jitter_u8(f, 0, 5, 7, p, None) == 0            # n = 0: success, nothing launched
    assert L.yk_hsv_jitter_u8(None, 0, 5, 7, None, None) == 0
    for args in [(None, 2, 5, 7, p), (f, 2, 5, 7, None), (f, -1, 5, 7, p), (f, 2, 0, 7, p), (f, 2, 5, 0, p), (f, 2, -5, 7, p)]:
        assert L.yk_hsv_jitter_u8(*args, None) == -10               # YK_ERR_ARG
        assert b'yk_hsv_jitter_u8' in L.yk_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f.cpu().numpy(), src)             # nothing ran
    empty = torch.empty((0, 5, 7, 3), dtype=torch.uint8, device='cuda')
    assert engine.hsv_jitter_u8(empty, np.zeros((0, 3))) is empty


def test_the_wrapper_refuses_what_it_cannot_pass_on():
    import torch
    from k210_yolo_framework_amd import engine
    f = torch.zeros((2, 5, 7, 3), dtype=torch.uint8, device='cuda')
    p = torch.from_numpy(np.array([ROWS[3], ROWS[4]])).cuda()
    refused = (AssertionError, engine.YkError)
    for frames, params in [(f.float(), p), (f[0], p), (f[..., :2].contiguous(), p), (f.cpu(), p), (f.permute(0, 2, 1, 3), p),
                           (torch.zeros((2, 5, 7, 6), dtype=torch.uint8, device='cuda')[..., ::2], p),
                           (f, p.float()), (f, p[:1]), (f, p.t().contiguous().t()), (f, p.cpu()), (f, p.reshape(6)),
                           (f, np.ones((3, 3))), (f, np.array([ROWS[3], (np.nan, 1.0, 1.0)])), (f, np.array([ROWS[3], (0.0, np.inf, 1.0)])),
                           (f, np.array([(0.0, 1.0, -1.0), ROWS[3]]))]:
        with pytest.raises(refused):
            engine.hsv_jitter_u8(frames, params)
    with pytest.raises(engine.YkError, match='row 1'):
        engine.hsv_jitter_u8(f, np.array([ROWS[3], (0.0, 1.0, -np.inf)]))
    torch.cuda.synchronize()
    assert not f.any().item()                                       # black stayed black, nothing else ran


def test_recorded_in_a_graph_and_replayed_gives_the_eager_bytes():
    import torch
    from k210_yolo_framework_amd import engine
    src = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (4, 24, 40, 3), dtype=np.uint8)).cuda()
    params = torch.from_numpy(np.array([ROWS[3], ROWS[0], ROWS[5], ROWS[4]])).cuda()
    eager = engine.hsv_jitter_u8(src.clone(), params)
    torch.cuda.synchronize()
    assert not torch.equal(eager, src)
    # one kernel node
    work = src.clone()
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    stream.wait_stream(torch.cuda.current_stream())
    graph = engine.capture(st, lambda: engine.call('yk_hsv_jitter_u8', work, 4, 24, 40, params, st))
    try:
        assert graph.kernel_nodes == 1 and graph.nodes == 1
        stream.synchronize()
        assert torch.equal(work, src)                               # recorded, not executed
        graph.launch(st)
        stream.synchronize()
        assert torch.equal(work, eager)
    finally:
        graph.close()
    # torch.cuda.graph: the kernel works in place, so every replay starts from a fresh copy of the input
    work = src.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
            engine.hsv_jitter_u8(work, params)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(work, src)
    for _ in range(2):
        work.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(work, eager)


def _items(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(6)
    items = []
    for k in range(18):
        hw = [(120, 160), (75, 100), (67, 100), (224, 320)][k % 4]
        img = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
        n = int(rng.integers(1, 4))
        boxes = np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(0.05, 0.3, (n, 2))], 1)
        if k % 3 == 0:
            p = tmp_path / f'{k}.png'
            Image.fromarray(img).save(p)
            items.append((str(p), boxes))
        else:
            items.append((img, boxes))
    return items


@pytest.mark.parametrize('augmented, mosaicked', [(False, False), (True, False), (False, True), (True, True)],
                         ids=['plain', 'augment', 'mosaic', 'mosaic+augment'])
def test_hsv_pipeline_equals_the_host_generator_for_every_rank(tmp_path, augmented, mosaicked):
    from k210_yolo_framework_amd import pipeline, training
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    h = Helper(None, 20, VOC_ANCHORS, [list(HW)], [[7, 10], [14, 20]])
    items = _items(tmp_path)
    GB, world, seed, epoch, cfg = 8, 2, 3, 1, colour.HsvConfig()
    order = pipeline.epoch_order(len(items), seed=seed, epoch=epoch, shuffle=True)

    class _Fixed:
        def permutation(self, n):
            return order
    kw = dict(augment=(seed, epoch) if augmented else None, mosaic=(seed, epoch, 1.0) if mosaicked else None)
    want = list(training.batches(h, items, GB, _Fixed(), shuffle=True, hsv=(seed, epoch, cfg), **kw))
    plain = list(training.batches(h, items, GB, _Fixed(), shuffle=True, **kw))
    assert len(want) == len(items) // GB == 2
    assert all(not np.array_equal(w[0][i], p[0][i]) for w, p in zip(want, plain) for i in range(GB))      # every frame is jittered ...
    for w, p in zip(want, plain):
        for wy, py in zip(w[1], p[1]):
            np.testing.assert_array_equal(wy, py)                   # ... and no label moves
    pkw = dict(seed=seed, epoch=epoch, shuffle=True, workers=4, prefetch=2, augment=augmented,
               mosaic=mosaic.MosaicConfig(1.0) if mosaicked else None)
    for rank in range(world):
        sl = slice(rank * GB // world, (rank + 1) * GB // world)
        pipe = pipeline.InputPipeline(h, items, GB, rank, world, hsv=cfg, **pkw)
        got = [(x.cpu().numpy(), [y.cpu().numpy() for y in ys]) for x, ys in pipe]
        pipe.close()
        assert len(got) == len(want)
        for (gx, gys), (wx, wys) in zip(got, want):
            np.testing.assert_array_equal(gx, wx[sl])
            for gy, wy in zip(gys, wys):
                np.testing.assert_array_equal(gy, wy[sl])
        # prob = 0: the frames of the pipeline without the option, bit for bit
        for kwargs in (dict(hsv=colour.HsvConfig(prob=0.0)), dict()):
            pipe = pipeline.InputPipeline(h, items, GB, rank, world, **kwargs, **pkw)
            off = [(x.cpu().numpy(), [y.cpu().numpy() for y in ys]) for x, ys in pipe]
            pipe.close()
            for (ox, oys), (px, pys) in zip(off, plain):
                np.testing.assert_array_equal(ox, px[sl])
                for oy, py in zip(oys, pys):
                    np.testing.assert_array_equal(oy, py[sl])


def test_make_train_with_hsv(tmp_path, capsys):
    from k210_yolo_framework_amd import engine, training
    with pytest.raises(engine.YkError, match='--hsv_sat 0.5'):
        training.cli(['--synthetic', '64', '--hsv', 'True', '--hsv_sat', '0.5', '--max_steps', '1', '--log_dir', str(tmp_path / 'refused')])
    assert not (tmp_path / 'refused').exists()
    training.cli(['--synthetic', '64', '--hsv', 'True', '--hsv_hue', '0.05', '--hsv_sat', '1.4', '--hsv_exposure', '1.3', '--hsv_prob', '0.9',
                  '--max_nrof_epochs', '1', '--max_steps', '2', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '24',
                  '--log_dir', str(tmp_path)])
    out = capsys.readouterr().out
    assert re.search(r'hsv is True, hsv_hue 0\.05, hsv_sat 1\.4, hsv_exposure 1\.3, hsv_prob 0\.9', out)
    losses = [float(v) for v in re.findall(r'step \d+: loss (\S+)', out)]
    assert len(losses) >= 1 and all(np.isfinite(losses))
    ck = list(tmp_path.glob('*/yolo_model.h5'))
    assert len(ck) == 1 and (ck[0].parent / 'yolo_model.npz').exists()
