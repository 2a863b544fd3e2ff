"""The device-resident picture cache (cache.py) behind InputPipeline(cache=..., decode=...): every batch bit for bit the
batch of the pipeline without a cache on the same (seed, epoch, items) - in every mode, on the first pass (all misses) and on the second
(all hits, no file touched), with a capacity that holds a third of the pictures, with the staging ring reused under a slow consumer, with
offsets beyond 2^32 - GPU JPEG decoding into the arena against detect.py's decode='gpu' path, and `--cache gpu` end to end."""
import re
import time
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import colour, mosaic
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS

pytestmark = pytest.mark.gpu

HW = (64, 96)
# 1 x 1, strips one pixel wide / high, odd sizes that are no multiple of 16, the network's own size, two sizes repeated
SIZES = [(1, 1), (37, 1), (33, 47), (50, 75), (33, 47), (17, 90), (64, 96), (5, 3), (61, 29), (9, 9), (1, 31), (50, 75), (23, 77), (45, 45)]
GB, SEED = 4, 5
MODES = {'plain': {}, 'augment': dict(augment=True), 'mosaic': dict(mosaic=mosaic.MosaicConfig(1.0)),
         'mosaic+augment': dict(mosaic=mosaic.MosaicConfig(0.8), augment=True),
         'mosaic+augment+hsv': dict(mosaic=mosaic.MosaicConfig(1.0), augment=True, hsv=colour.HsvConfig()),
         'plain+hsv': dict(hsv=colour.HsvConfig())}
_shared = {}


def _h():
    return Helper(None, 20, VOC_ANCHORS, [list(HW)], [[2, 3], [4, 6]])


def _pictures():
    if 'pics' not in _shared:
        rng = np.random.default_rng(11)
        _shared['pics'] = [rng.integers(1, 256, (*hw, 3), dtype=np.uint8) for hw in SIZES]
        _shared['boxes'] = [np.concatenate([rng.integers(0, 20, (m, 1)).astype(float), rng.uniform(0.2, 0.8, (m, 2)), rng.uniform(0.1, 0.4, (m, 2))], 1)
                            for m in rng.integers(1, 4, len(SIZES))]
    return _shared['pics'], _shared['boxes']


@pytest.fixture(scope='module')
def items(tmp_path_factory):
    """The pictures as PNG files (lossless: PIL's pixels are the arrays), every fourth one an array already in memory."""
    from PIL import Image
    folder = tmp_path_factory.mktemp('cache_pics')
    pics, boxes = _pictures()
    out = []
    for k, (img, b) in enumerate(zip(pics, boxes)):
        if k % 4 == 3:
            out.append((img, b))
        else:
            Image.fromarray(img).save(folder / f'{k}.png')
            out.append((str(folder / f'{k}.png'), b))
    return out


def _run(h, items, epoch=0, consumer_sleep=0.0, batch=GB, **kw):
    from k210_yolo_framework_amd import pipeline
    pipe = pipeline.InputPipeline(h, items, batch, 0, 1, seed=SEED, epoch=epoch, shuffle=True, workers=4, **kw)
    out = []
    try:
        for x, ys in pipe:
            out.append((x, list(ys)))
            if consumer_sleep:
                time.sleep(consumer_sleep)
    finally:
        pipe.close()
    return out


def _reference(h, items, mode, epoch=0):
    """The pipeline without a cache: computed once per (mode, epoch), shared and never changed."""
    key = (mode, epoch, len(items))
    if key not in _shared:
        _shared[key] = _run(h, items, epoch=epoch, **MODES[mode])
    return _shared[key]


def _assert_equal(got, want):
    import torch
    assert len(got) == len(want) > 0
    for k, ((gx, gys), (wx, wys)) in enumerate(zip(got, want)):
        assert torch.equal(gx, wx), f'batch {k}: frames'
        assert len(gys) == len(wys)
        for l, (gy, wy) in enumerate(zip(gys, wys)):
            assert torch.equal(gy, wy), f'batch {k}: labels of layer {l}'


@pytest.mark.parametrize('mode', list(MODES))
def test_both_passes_equal_the_pipeline_without_a_cache(items, mode, monkeypatch):
    from k210_yolo_framework_amd.cache import PictureCache
    h = _h()
    want = _reference(h, items, mode)
    assert len(want) == len(items) // GB == 3
    with PictureCache(1 << 20, stage_bytes=1 << 18) as cache:
        _assert_equal(_run(h, items, cache=cache, **MODES[mode]), want)        # pass 1: every picture is a miss, once
        first = cache.stats()
        assert first.hits + first.misses > 0 and first.admitted == first.misses and 0 < first.bytes_used <= first.capacity
        if 'mosaic' not in mode:
            assert (first.hits, first.misses) == (0, 3 * GB)

        def no_file(path):
            raise AssertionError(f'a hit read {path}')
        monkeypatch.setattr(h, '_read_img', no_file)
        _assert_equal(_run(h, items, cache=cache, **MODES[mode]), want)        # pass 2, a new pipeline as the training loop builds one
        second = cache.stats()
        assert second.misses == first.misses and second.admitted == first.admitted and second.bytes_used == first.bytes_used
        assert second.hits > first.hits
        pics, _ = _pictures()
        import torch
        for row in cache.lookup(range(len(items))):
            assert torch.equal(cache.read(row).cpu(), torch.from_numpy(pics[row])), row


def test_a_capacity_for_a_third_of_the_pictures_stages_the_rest_every_epoch(items):
    import torch
    from k210_yolo_framework_amd.cache import PictureCache
    h = _h()
    pics, _ = _pictures()
    third = sum(p.size for p in pics) // 3
    with PictureCache(third, stage_bytes=1 << 18) as cache:
        kept = {}
        for epoch in (0, 1):
            before = cache.stats()
            _assert_equal(_run(h, items, epoch=epoch, cache=cache, **MODES['mosaic+augment']), _reference(h, items, 'mosaic+augment', epoch))
            s = cache.stats()
            assert 0 < s.admitted < len(items) and s.bytes_used <= s.capacity == cache.capacity_bytes
            assert s.misses > before.misses                                     # what does not fit is brought in again, every epoch
            if epoch == 0:
                kept = {row: cache.read(row).clone() for row in cache.lookup(range(len(items)))}
                assert len(kept) == s.admitted
            else:
                assert s.hits > before.hits
        for row, was in kept.items():                                           # write once: the persistent bytes are still the pictures
            assert torch.equal(cache.read(row), was) and torch.equal(was.cpu(), torch.from_numpy(pics[row])), row
        entries = cache.lookup(range(len(items)))
        spans = sorted((o, o + 3 * hh * ww) for o, hh, ww in entries.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= cache.capacity_bytes


def test_the_staging_ring_is_reused_while_the_consumer_lags(items):
    from k210_yolo_framework_amd.cache import PictureCache
    h = _h()
    many = list(items) * 3                                                     # 42 rows: 20 batches of 2 and a remainder
    kw = dict(batch=2, prefetch=1, **MODES['mosaic'])
    want = _run(h, many, **kw)
    assert len(want) >= 20
    with PictureCache(0, stage_bytes=1 << 18, prefetch=1) as cache:
        assert cache.ring == 3
        got = _run(h, many, cache=cache, consumer_sleep=0.01, **kw)             # the producer runs ahead, every region serves ~7 batches
        _assert_equal(got, want)
        s = cache.stats()
        assert s.hits == 0 and s.admitted == 0 and s.bytes_used == 0 and s.misses >= 2 * len(want)
        assert cache._tick == len(want)


def test_offsets_beyond_two_to_the_32(items):
    import torch
    from k210_yolo_framework_amd.cache import PictureCache
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f'a 4 GiB + 64 MiB arena needs 8 GiB free, the device has {free >> 20} MiB')
    h = _h()
    small = [items[k] for k in (2, 3, 5)] * 2                                  # three pictures, one batch of four plus a remainder
    with PictureCache((4 << 30) + (64 << 20), stage_bytes=1 << 20, _first_offset=2 ** 32 + 16) as cache:
        for mode in ('plain', 'augment', 'mosaic'):
            want = _reference(h, small, mode)
            _assert_equal(_run(h, small, cache=cache, **MODES[mode]), want)
        entries = cache.lookup(range(len(small)))
        assert len(entries) >= 3 and min(o for o, _, _ in entries.values()) == 2 ** 32 + 16
        assert all(o > 2 ** 32 and o % 16 == 0 for o, _, _ in entries.values())
        assert cache.stats().bytes_used > 2 ** 32


def _jpeg_files(folder):
    """Written by PIL: baseline 4:2:0 / 4:4:4 / grey, one with a restart interval, a progressive JPEG and a PNG."""
    from PIL import Image
    rng = np.random.default_rng(21)
    shapes = [(50, 75), (33, 47), (64, 96), (61, 29), (40, 56), (17, 90), (24, 24), (50, 75)]
    paths = []
    for i, hw in enumerate(shapes):
        im = Image.fromarray(np.kron(rng.integers(0, 256, ((hw[0] + 3) // 4, (hw[1] + 3) // 4, 3), dtype=np.uint8),
                                     np.ones((4, 4, 1), np.uint8))[:hw[0], :hw[1]])
        p = folder / (f'p{i}.png' if i == 5 else f'p{i}.jpg')
        if i == 4:
            im.save(p, progressive=True)
        elif i == 5:
            im.save(p)
        elif i == 2:
            im.convert('L').save(p)
        elif i == 3:
            im.save(p, quality=90, subsampling=2, restart_marker_blocks=3)
        else:
            im.save(p, quality=90, subsampling=(2, 0)[i % 2])
        paths.append(str(p))
    return paths


def test_decode_gpu_writes_detects_bytes_into_the_arena(tmp_path):
    import torch
    from k210_yolo_framework_amd import detect, engine, jpeg, keras_io, netspec as ns
    from k210_yolo_framework_amd.cache import PictureCache
    from k210_yolo_framework_amd.yolonet import MODEL_DEFS
    paths = _jpeg_files(tmp_path)
    parsed = {}
    for k, f in enumerate(paths):
        try:
            parsed[k] = jpeg.parse_baseline(Path(f).read_bytes())
        except jpeg.Unsupported:
            pass
    assert sorted(parsed) == [0, 1, 2, 3, 6, 7] and parsed[3].restart > 0 and parsed[2].ncomp == 1
    assert (parsed[0].hs, parsed[0].vs, parsed[1].hs, parsed[1].vs) == (2, 2, 1, 1)
    # detect.py's decode='gpu' path on the same files: a threshold no score reaches, so the pictures come back as they were decoded
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.5)
    ck = tmp_path / 'yolo_model.h5'
    keras_io.save_keras_weights(spec, spec.init_weights(seed=1), ck)
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.5, precision='f16x2')
    model.load_weights(str(ck))
    hd = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    det = detect.run(hd, model, paths, decode='gpu', draw=True, return_arrays=True, obj_thresh=1.5, batch=4, depth=1, verbose=False)
    assert sum(len(d) for d in det['detections']) == 0 and len(det['arrays']) == len(paths)
    h = _h()
    rng = np.random.default_rng(3)
    boxes = [np.concatenate([rng.integers(0, 20, (2, 1)).astype(float), rng.uniform(0.3, 0.7, (2, 2)), rng.uniform(0.1, 0.4, (2, 2))], 1) for _ in paths]
    items = list(zip(paths, boxes))
    by_hand = [(np.ascontiguousarray(a), b) for a, b in zip(det['arrays'], boxes)]     # the same pixels as arrays: the uncached reference
    for k in (4, 5):                                                            # the parser refuses these two: PIL's pixels
        assert np.array_equal(det['arrays'][k], np.ascontiguousarray(h._read_img(paths[k])[..., :3], np.uint8))
    for mode in ('plain', 'mosaic+augment'):
        want = _run(h, by_hand, **MODES[mode])
        with PictureCache(1 << 20, stage_bytes=1 << 18) as cache:
            one = _run(h, items, cache=cache, decode='gpu', **MODES[mode])
            _assert_equal(one, want)
            first = cache.stats()
            for row, (o, hh, ww) in cache.lookup(range(len(paths))).items():    # the arena holds detect's bytes
                assert torch.equal(cache.read(row).cpu(), torch.from_numpy(np.ascontiguousarray(det['arrays'][row]))), paths[row]
            assert first.admitted == first.misses > 0
            two = _run(h, items, cache=cache, decode='gpu', **MODES[mode])      # served from the cache
            _assert_equal(two, one)
            assert cache.stats().misses == first.misses and cache.stats().hits > first.hits
        _assert_equal(_run(h, items, decode='gpu', **MODES[mode]), want)        # without a cache: staging only
    # a stream that ends early: an error naming the file, and the row is not admitted
    data = Path(paths[0]).read_bytes()
    seg = parsed[0].scan
    at = data.index(seg)
    short = tmp_path / 'short.jpg'
    short.write_bytes(data[:at + len(seg) // 2] + b'\xff\xd9')
    bad = [(str(short), boxes[0])] + items[1:4]
    with PictureCache(1 << 20, stage_bytes=1 << 18) as cache:
        with pytest.raises(engine.YkError, match='short.jpg'):
            _run(h, bad, cache=cache, decode='gpu')
        assert 0 not in cache.lookup(range(4)) and sorted(cache.lookup(range(4))) == [1, 2, 3]


LINE = r'epoch (\d+): (\d+) steps, mean loss (\d+\.\d{4}), (?:val_loss (\d+\.\d{4}), )?\d+\.\ds, input pipeline \d+ images/s/rank'


@pytest.mark.parametrize('mosaicked', ['False', 'True'], ids=['plain', 'mosaic'])
def test_make_train_with_the_cache_trains_on_the_same_batches(tmp_path, capsys, mosaicked):
    from k210_yolo_framework_amd import training
    common = ['--synthetic', '32', '--max_nrof_epochs', '2', '--mosaic', mosaicked, '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5',
              '--batch_size', '8']
    training.cli(common + ['--cache', 'off', '--log_dir', str(tmp_path / 'off')])
    off = capsys.readouterr().out
    training.cli(common + ['--cache', 'gpu', '--cache_gb', '0.25', '--cache_stage_mb', '16', '--log_dir', str(tmp_path / 'on')])
    on = capsys.readouterr().out
    off_lines = [l for l in off.splitlines() if re.match(r'epoch \d+: \d+ steps', l)]
    on_lines = [l for l in on.splitlines() if re.match(r'epoch \d+: \d+ steps', l)]
    assert len(off_lines) == len(on_lines) == 2
    assert all(re.fullmatch(LINE, l) for l in off_lines), off_lines             # off: the line as it always was
    assert 'hits/misses' not in off and 'cache is' not in off
    tail = r', cache (\d+)/(\d+) hits/misses, (\d+\.\d\d)/0\.25 GB'
    figures = [re.fullmatch(LINE + tail, l) for l in on_lines]
    assert all(figures), on_lines
    for a, b in zip(off_lines, figures):                                        # epoch, steps, mean loss and val_loss: the same figures
        assert re.fullmatch(LINE, a).groups() == b.groups()[:4]
    steps = lambda out: re.findall(r'epoch \d+ step \d+: loss (\S+)', out)
    assert steps(on) == steps(off) and len(steps(on)) >= 2
    h1, m1, h2, m2 = (int(figures[e].group(g)) for e in (0, 1) for g in (5, 6))
    assert h2 >= h1 and m2 >= m1 > 0 and h2 > 0                                 # the counts run on over the epochs
    if mosaicked == 'False':
        assert (h1, m1) == (0, 24) and h2 + m2 == 48                            # 29 training pictures, three batches of eight per epoch
    assert re.search(r'cache is gpu, cache_gb 0\.25, cache_stage_mb 16\.0, decode is pil', on)
    assert len(list(tmp_path.glob('on/*/yolo_model.h5'))) == 1


def test_a_cache_the_device_cannot_hold_is_refused_by_name():
    import torch
    from k210_yolo_framework_amd import engine
    from k210_yolo_framework_amd.cache import PictureCache
    _, total = torch.cuda.mem_get_info()
    with pytest.raises(engine.YkError, match=r'--cache_gb asks for \d+ bytes.*the device has \d+ bytes free'):
        PictureCache(2 * total)
