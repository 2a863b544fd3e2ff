"""engine.TrackState.update (yk_track_update) against track.Tracker: rows, ids, counts, the draw copy and read(), equal bit for bit."""
import numpy as np
import pytest

from k210_yolo_framework_amd import track as tk

pytestmark = pytest.mark.gpu
F = np.float32
NAN = float('nan')


def row(top, left, h=40, w=30, score=0.9, cls=3):
    return [top, left, top + h, left + w, score, cls]


def crossing(n, frames):
    """n boxes on a 20-pixel pitch, so that neighbours overlap: even ones move right, odd ones left, three classes, seven scores."""
    return [[row(60 * (k // 16), 20 * (k % 16) + (3 if k % 2 == 0 else -3) * t, score=0.62 + 0.05 * (k % 7), cls=k % 3) for k in range(n)]
            for t in range(frames)]


STILL = [row(10, 10)]
# name -> (sequences: frames of rows each, options of the tracker, max_tracks, the calls: frames per sequence in each)
CASES = {
    'open_confirm_update': ([[[row(10, 10 + 4 * t)] for t in range(3)]], {}, 256, None),
    'crossing_65': ([crossing(65, 5)], {}, 256, None),
    'crossing_129': ([crossing(129, 5)], {}, 256, None),
    'ties': ([[[row(10, 10), row(10, 10)], [row(10, 10, score=0.7), row(10, 10, score=0.8)], [row(11, 10), row(11, 10)]]], {}, 256, None),
    'lost_found_expired': ([[STILL] * 3 + [[]] * 3 + [STILL] * 2, [STILL] * 3 + [[]] * 4 + [STILL] * 2], dict(track_buffer=3), 256, None),
    'low_scores': ([[STILL, [row(10, 10, score=0.3)], [row(11, 10, score=0.3), row(100, 100, score=0.3)], [row(11, 11, score=0.05)]]], {}, 256,
                   None),
    'two_classes': ([[[row(10, 10 + 2 * t, score=0.9, cls=3), row(12, 8 + 2 * t, score=0.8, cls=5)][::(1 if t % 2 == 0 else -1)]
                      for t in range(5)]], {}, 256, None),
    'empty_frame_and_empty_sequence': ([[STILL, [], STILL], [], [[row(50, 50, cls=1)], [row(52, 50, cls=1)]]], {}, 256, None),
    'bad_rows': ([[[row(10, 10), row(100, 10, score=NAN), row(100, 60, cls=20), row(100, 110, h=0), row(100, 160, w=-5),
                    row(NAN, 210), row(100, 260, h=float('inf')), row(100, 310, cls=2.5)]] * 3], {}, 256, None),
    'eight_frames_as_three_and_five': ([crossing(20, 8)], {}, 256, [[3], [5]]),
    'overflow': ([[[row(60 * k, 10) for k in range(6)]] + [[row(60 * k, 10 + 2 * t) for k in range(4)] for t in (1, 2)]], {}, 4, None),
}


def host(seqs, cfg, max_tracks, cap, class_num=20):
    """-> (per sequence, per frame: (rows, ids)), live, next_id, overflow"""
    out, trackers = [], []
    for frames in seqs:
        t = tk.Tracker(class_num, max_tracks=max_tracks, **cfg)
        out.append([t.update(np.asarray(f, F).reshape(-1, 6), cap=cap) for f in frames])
        trackers.append(t)
    return out, [t.live for t in trackers], [t.next_id for t in trackers], [t.overflow for t in trackers]


def device(seqs, cfg, max_tracks, cap, calls=None, class_num=20):
    """The same through engine.TrackState, in one call or in `calls`; also checks the draw copy.  -> (frames, state)"""
    import torch
    from k210_yolo_framework_amd import engine
    state = engine.TrackState(len(seqs), class_num, max_tracks=max_tracks, **cfg)
    out, done = [[] for _ in seqs], [0] * len(seqs)
    for take in calls or [[len(f) for f in seqs]]:
        frames = [f for s, k in enumerate(take) for f in seqs[s][done[s]:done[s] + k]]
        dets, counts = np.zeros((len(frames), cap, 6), F), np.zeros(len(frames), np.int32)
        for i, f in enumerate(frames):
            counts[i] = len(f)
            dets[i, :len(f)] = np.asarray(f, F).reshape(-1, 6)
        rows, ids, n, drawn = (t.cpu().numpy() for t in state.update(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(),
                                                                      np.concatenate([[0], np.cumsum(take)]), draw=True))
        at = 0
        for s, k in enumerate(take):
            for i in range(at, at + k):
                out[s].append((rows[i, :n[i]], ids[i, :n[i]]))
                want = rows[i, :n[i]].copy()
                want[:, 5] = ids[i, :n[i]] % 100
                assert np.array_equal(drawn[i, :n[i]].view(np.int32), want.view(np.int32))
            at, done[s] = at + k, done[s] + k
    return out, state


def same_frames(got, want):
    assert [len(s) for s in got] == [len(s) for s in want]
    for gs, ws in zip(got, want):
        for (gr, gi), (wr, wi) in zip(gs, ws):
            assert np.array_equal(gi, wi), (gi, wi)
            assert gr.shape == wr.shape and np.array_equal(gr.view(np.int32), wr.view(np.int32)), (gr, wr)


@pytest.mark.parametrize('name', list(CASES))
def test_update_equals_the_host_tracker(name):
    seqs, cfg, max_tracks, calls = CASES[name]
    cap = max(len(f) for s in seqs for f in s) + 3
    want, live, next_id, overflow = host(seqs, cfg, max_tracks, cap)
    got, state = device(seqs, cfg, max_tracks, cap, calls)
    same_frames(got, want)
    assert [a.tolist() for a in state.read()] == [live, next_id, overflow]
    assert sum(len(i) for s in want for _, i in s) > 0                                   # (the case tracks something)
    if name == 'crossing_129':
        assert max(int(i.max()) for _, i in want[0]) >= 129 and live[0] > 128            # past two tracks per lane, ids past the draw's mod 100
    if name == 'overflow':                                                               # the four tracks go on as in an unbounded run
        assert overflow == [2]
        free, *_ = host(seqs, cfg, None, cap)
        same_frames(got, [[(r[i <= 4], i[i <= 4]) for r, i in free[0]]])
    if calls:                                                                            # one call leaves the bytes and the state of several
        whole, state1 = device(seqs, cfg, max_tracks, cap)
        same_frames(whole, got)
        a, b = state.state.cpu().numpy(), state1.state.cpu().numpy()
        assert np.array_equal(a[:4], b[:4]) and np.array_equal(a[4:].reshape(25, -1)[:, :live[0]], b[4:].reshape(25, -1)[:, :live[0]])


def test_the_largest_cap_is_taken_and_one_more_is_refused_by_name():
    import torch
    from k210_yolo_framework_amd import engine
    cap = engine.track_max_cap(256)
    assert cap >= 2400                                                                   # 80 classes x 30 rows fit beside 256 tracks
    state = engine.TrackState(1, 20)
    dets = torch.zeros((1, cap + 1, 6), dtype=torch.float32, device='cuda')
    dets[0, cap - 1] = torch.tensor(row(10, 10))                                         # the last row a full frame can hold
    counts = torch.tensor([cap], dtype=torch.int32, device='cuda')
    rows, ids, n = state.update(dets[:, :cap].contiguous(), counts, [0, 1])
    assert n.tolist() == [1] and ids[0, 0].item() == 1 and np.array_equal(rows[0, 0].cpu().numpy(), np.asarray(row(10, 10), F))
    with pytest.raises(engine.YkError, match=r'cap \d+'):
        state.update(dets, counts, [0, 1])
    with pytest.raises(engine.YkError, match='seq_first'):
        state.update(dets[:, :8].contiguous(), counts, [1, 0])
    with pytest.raises(engine.YkError, match='track_max'):
        engine.TrackState(1, 20, max_tracks=tk.MAX_TRACKS + 1)
    assert [a.tolist() for a in state.read()] == [[1], [2], [0]]                         # the refused calls launched nothing
