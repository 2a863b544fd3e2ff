"""engine.gmc_motion (yk_gmc_motion_u8) against gmc.py - every block's (dy, dx, sad, kept) and every frame's motion, exactly - at the smallest
shapes at which the kernels can go wrong; yk_track_update_gmc against track.Tracker(gmc=True), bit for bit; detect.run(gmc=True) against
the host path."""
import numpy as np
import pytest

from k210_yolo_framework_amd import gmc
from k210_yolo_framework_amd import track as tk
from tests.gmc_cases import CONTENT, view
from tests.test_gmc import pan_rows

pytestmark = pytest.mark.gpu
F = np.float32

# name -> (sequences: pictures each, options, the calls: frames per sequence in each - None: all in one)
CASES = {
    # (B + 2R) f = 128 on a side is exactly one block; a pixel less is none, which is no error
    'one_block_and_none': ([[view(h=128, w=128), view(4, 4, 128, 128)], [view(h=127, w=127), view(4, 4, 127, 127)]], dict(min_blocks=1), None),
    # sides no multiple of the scale, a width no multiple of 4 (rows of the original start at every byte alignment), B = 8
    'odd_sides_b8': ([[view(h=141, w=203), view(-8, 12, 141, 203)]], dict(block=8, step=8, min_blocks=2), None),
    # R = 1: nine candidates, one round, window rows of 18 bytes padded to 20
    'r1': ([[view(h=100, w=131), view(4, -4, 100, 131)]], dict(range=1, step=4, min_blocks=2), None),
    # a block side and a scale without a compiled-in form; 49 candidates
    'b12_f3': ([[view(h=97, w=130), view(-6, 3, 97, 130)]], dict(scale=3, block=12, range=3, step=5, min_blocks=2), None),
    # the content cases of tests/test_gmc.py, seven sequences in one call
    'content': ([frames for frames, _ in CONTENT.values()], {}, None),
    # a sequence continued across three calls beside one that pauses: the kept last picture; and a change of size in mid-sequence
    'continued': ([[view(), view(8, -4), view(20, 0), view(24, 8, h=252), view(16, 8, h=252)], [view(h=128, w=256), view(-12, 0, 128, 256)]],
                  dict(min_blocks=3), [[1, 1], [2, 0], [2, 1]]),
}


def host(seqs, cfg):
    out = []
    for frames in seqs:
        e = gmc.Estimator(**cfg)
        out.append([(e.update(p), e.blocks.copy()) for p in frames])
    return out


def device(seqs, cfg, calls=None):
    """The same through engine.gmc_motion; -> per sequence, per frame (motion, blocks), and the raw outputs of every call."""
    import torch
    from k210_yolo_framework_amd import draw as dr
    from k210_yolo_framework_amd import engine
    calls = calls or [[len(f) for f in seqs]]
    scale = cfg.get('scale', 4)
    state = engine.GmcState(len(seqs), max(sum(c) for c in calls), max((p.shape[0] // scale) * (p.shape[1] // scale) for f in seqs for p in f),
                            **cfg)
    out, done, raw = [[] for _ in seqs], [0] * len(seqs), []
    for take in calls:
        frames = [p for s, k in enumerate(take) for p in seqs[s][done[s]:done[s] + k]]
        packed, table, _ = dr.pack_ragged(frames)
        blocks = torch.full((len(frames), state.max_blocks, 4), -7, dtype=torch.int32, device='cuda')
        motion = engine.gmc_motion(state, packed.cuda(), table, np.concatenate([[0], np.cumsum(take)]), blocks=blocks)
        raw.append((motion.cpu().numpy(), blocks.cpu().numpy()))
        at = 0
        for s, k in enumerate(take):
            out[s] += [(raw[-1][0][i], raw[-1][1][i]) for i in range(at, at + k)]
            at, done[s] = at + k, done[s] + k
    return out, raw


@pytest.mark.parametrize('name', list(CASES))
def test_motion_and_blocks_equal_the_rule(name):
    seqs, cfg, calls = CASES[name]
    want = host(seqs, cfg)
    got, raw = device(seqs, cfg, calls)
    for ws, gs in zip(want, got):
        for (wm, wb), (gm, gb) in zip(ws, gs):
            assert gm.dtype == F and np.array_equal(gm, wm), (gm, wm)
            assert np.array_equal(gb[:len(wb)], wb), (gb[:len(wb)], wb)
            assert (gb[len(wb):] == -7).all()                                        # rows past the frame's blocks are not written
    assert sum(len(b) for s in want for _, b in s) > 0 and any(m.any() for s in want for m, _ in s)
    if name == 'one_block_and_none':
        assert [len(b) for _, b in want[0]] == [0, 1] and [len(b) for _, b in want[1]] == [0, 0]
    if name == 'content':                                                            # two calls give the same bytes
        again = device(seqs, cfg, calls)[1]
        assert all(np.array_equal(a, b) for x, y in zip(raw, again) for a, b in zip(x, y))


def test_bad_arguments_are_refused_by_name():
    from k210_yolo_framework_amd import draw as dr
    from k210_yolo_framework_amd import engine
    for kw, name in ((dict(block=10), 'gmc_block'), (dict(range=0), 'gmc_range'), (dict(scale=0), 'gmc_scale')):
        with pytest.raises(engine.YkError, match=name):
            engine.GmcState(1, 2, 4096, **kw)
    with pytest.raises(engine.YkError, match=r'cfg->block 10'):
        engine.call('yk_gmc_max_blocks', engine.C.byref(engine.GmcCfg(4, 10, 8, 16, 16, 8, 1, 2, 4096)))
    with pytest.raises(engine.YkError, match=r'blocks at step 1.*8192'):                 # more than the median's LDS holds: refused, not cut
        engine.GmcState(1, 2, 320 * 180, step=1)
    state = engine.GmcState(1, 2, 32 * 32)
    packed, table, _ = dr.pack_ragged([view(h=128, w=132)] * 3)
    with pytest.raises(engine.YkError, match='row 0 is 128 x 132, 1056 small pixels'):
        engine.gmc_motion(state, packed.cuda(), table, [0, 3])
    packed, table, _ = dr.pack_ragged([view(h=128, w=128)] * 3)
    with pytest.raises(engine.YkError, match=r'n_frames 3.*max_frames 2'):
        engine.gmc_motion(state, packed.cuda(), table, [0, 3])


@pytest.mark.parametrize('assign', tk.ASSIGNS)
def test_track_update_gmc_equals_the_host_tracker(assign):
    import torch
    from k210_yolo_framework_amd import engine
    frames = [np.concatenate([pan_rows(t), pan_rows(t)[:1] + F([3 * t, 2 * t, 3 * t, 2 * t, -0.5, 0])]) for t in range(8)]
    motions = np.asarray([(0, 0) if t == 0 or t % 2 else (40 if (t // 2) % 2 else -40, t) for t in range(8)], F)
    host_t = tk.Tracker(20, gmc=True, assign=assign, max_tracks=256)
    want = [host_t.update(f, cap=6, motion=m) for f, m in zip(frames, motions)]
    state = engine.TrackState(1, 20, assign=assign)
    dets = np.zeros((8, 6, 6), F)
    dets[:, :4] = np.stack(frames)
    rows, ids, n = (t.cpu().numpy() for t in state.update(torch.from_numpy(dets).cuda(), torch.full((8,), 4, dtype=torch.int32, device='cuda'),
                                                          [0, 8], motion=torch.from_numpy(motions).cuda()))
    for i, (wr, wi) in enumerate(want):
        assert np.array_equal(ids[i, :n[i]], wi) and np.array_equal(rows[i, :n[i]].view(np.int32), wr.view(np.int32))
    assert [w[1].tolist()[:3] for w in want] == [[1, 2, 3]] * 8


def test_detect_run_with_gmc_equals_the_host_path(tmp_path):
    import json
    from PIL import Image
    from k210_yolo_framework_amd import detect, engine
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from k210_yolo_framework_amd.yolonet import YoloModel
    from tests.plan_zoo import residual
    spec, weights = residual()
    model = YoloModel(spec, {'weights': weights, 'precision': 'f16x2'}, False)
    h = Helper(None, 20, VOC_ANCHORS, np.array([list(spec.in_hw)]), np.array([list(x) for x in spec.out_hw()]))
    (tmp_path / 'pan').mkdir()
    paths = []
    for t, dx in enumerate((0, 16, 28, 28, 4, -20, -8)):                                # smooth content, so that JPEG keeps it matchable
        big = np.asarray(Image.fromarray(view(dx, 2 * t)[::8, ::8]).resize((448, 256), Image.BICUBIC))
        paths.append(str(tmp_path / 'pan' / f'{t:03d}.jpg'))
        Image.fromarray(big).save(paths[-1], quality=92)
    kw = dict(draw=False, batch=3, depth=2, obj_thresh=0.5, iou_thresh=0.5, verbose=False)
    trk = dict(track_thresh=0.85, track_low=0.5, track_match=0.8, track_buffer=2, track_max=1024)
    try:
        plain = detect.run(h, model, paths, **kw)
        got = detect.run(h, model, paths, out_dir=tmp_path / 'out', track=True, gmc=True, gmc_texture=8, **trk, **kw)
        with pytest.raises(engine.YkError, match='gmc without track'):
            detect.run(h, model, paths, gmc=True, **kw)
    finally:
        model._drop_plan()
    est, host_t = gmc.Estimator(texture=8), tk.Tracker(20, *trk.values(), gmc=True)
    for path, rows, rows_got, ids, motion in zip(paths, plain['detections'], got['detections'], got['track_ids'], got['motion']):
        want_motion = est.update(h._read_img(path)[..., :3])
        assert np.array_equal(motion, want_motion), (path, motion, want_motion)
        want, want_ids = host_t.update(rows, cap=600, motion=want_motion)
        assert np.array_equal(ids, want_ids) and np.array_equal(rows_got.view(np.int32), want.view(np.int32))
    assert got['motion'].any() and sum(len(i) for i in got['track_ids']) > 0
    doc = json.loads((tmp_path / 'out' / 'detections.json').read_text())
    assert doc[0]['gmc']['gmc_texture'] == 8 and doc[0]['motion'] == got['motion'].tolist() and 'motion' not in doc[1]
