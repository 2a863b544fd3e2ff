"""engine.TrackState(assign=, fuse_score=) (yk_track_update_ex) against track.Tracker, bit for bit: rows, ids, counts, the draw copy and
read(), at the shapes where the matrix-free solver of csrc/yk_track.hip can go wrong."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_track import CASES as GREEDY_CASES, crossing, device, host, row, same_frames

pytestmark = pytest.mark.gpu
F = np.float32
OPTIONS = [('lap', False), ('lap', True), ('greedy', True), ('greedy', False)]


def crowd(n_tracks, n_rows, seed):
    """n_tracks boxes of one class on a 7-pixel pitch (30 wide: every box overlaps eight others) open tracks; two frames of n_rows jittered
    rows in a shuffled order follow, so that both orientations of the solver run and, with fewer rows than tracks, LOST tracks come back."""
    rng = np.random.default_rng(seed)
    frames = [[row(10, 7 * k, score=0.62 + 0.03 * (k % 11)) for k in range(n_tracks)]]
    for _ in range(2):
        at = rng.permutation(max(n_tracks, n_rows))[:n_rows]
        frames.append([row(10 + float(rng.integers(-6, 7)), 7 * int(k) + float(rng.integers(-9, 10)), score=float(F(rng.uniform(0.55, 0.99)))) for k in at])
    return frames


THREE = crossing(30, 4)
THREE[2] = [r for r in THREE[2] if r[5] != 2]                            # a class with tracks and no rows
STAGES = [[row(10, 10), row(10, 100), row(10, 200)], [row(12, 10), row(10, 300), row(10, 202, score=0.3)],     # 100 goes LOST, 300 is NEW,
          [row(14, 12), row(11, 101), row(12, 303), row(10, 203), row(60, 400, score=0.2)]]                    # 200 takes a low row; all return
# name -> (sequences, max_tracks)
CASES = {f'{t}x{r}': ([crowd(t, r, t + r)], 256) for t, r in [(1, 1), (2, 2), (3, 64), (64, 3), (63, 65), (65, 63), (130, 70)]}
CASES.update({
    'three_classes': ([THREE], 256),
    'duplicates': (GREEDY_CASES['ties'][0], 256),
    'all_forbidden': ([[[row(10, 40 * k) for k in range(5)], [row(300, 40 * k) for k in range(3)]]], 256),
    'all_three_stages': ([STAGES], 256),
    'four_frames_and_two_sequences': ([crossing(20, 4), crowd(9, 7, 1)[:2]], 256),
    'overflow': ([[[row(10, 40 * k) for k in range(11)], [row(12, 40 * k + 3) for k in range(11)]]], 8),
    # greedy gives the left track the row nearest to it, which is the only row the right track reaches
    'crossing': ([[[row(10, 0), row(10, 15)], [row(10, 3), row(10, -10)]]], 256),
})


@pytest.mark.parametrize('assign, fuse', OPTIONS)
@pytest.mark.parametrize('name', list(CASES))
def test_update_equals_the_host_tracker(name, assign, fuse):
    seqs, max_tracks = CASES[name]
    cfg = dict(assign=assign, fuse_score=fuse)
    cap = max(len(f) for s in seqs for f in s) + 3
    want, live, next_id, overflow = host(seqs, cfg, max_tracks, cap)
    got, state = device(seqs, cfg, max_tracks, cap)
    same_frames(got, want)
    assert [a.tolist() for a in state.read()] == [live, next_id, overflow]
    if name == 'overflow':
        assert overflow[0] >= 3 and live == [8]
    if name == 'crossing':                                               # frame 2: greedy keeps one track; lap both, track 1 on the second row
        rows, ids = got[0][1]
        assert ids.tolist() == ([1, 2] if assign == 'lap' else [1]) and (rows[0, 1] < 0) == (assign == 'lap')


def test_ex_with_the_defaults_gives_the_bytes_of_yk_track_update_and_a_cap_above_the_capacity_is_refused():
    import torch
    from k210_yolo_framework_amd import engine
    cap = 70
    dets, counts = np.zeros((3, cap, 6), F), torch.full((3,), 65, dtype=torch.int32, device='cuda')
    dets[:, :65] = np.asarray(crossing(65, 3), F)
    dets = torch.from_numpy(dets).cuda()
    state, plain = engine.TrackState(1, 20), engine.TrackState(1, 20)
    out = [torch.zeros(s, dtype=d, device='cuda') for s, d in (((3, cap, 6), torch.float32), ((3, cap), torch.int32), ((3,), torch.int32))]
    engine.call('yk_track_update_ex', state.state, 1, 256, dets, counts, cap, torch.tensor([0, 3], dtype=torch.int32, device='cuda'), 3, 20,
                C.byref(state.cfg), 0, 0, *out, None, engine._stream())
    for a, b in zip(out, plain.update(dets, counts, [0, 3])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = state.state.cpu().numpy(), plain.state.cpu().numpy()
    assert a[0] > 64 and np.array_equal(a[:4], b[:4]) and np.array_equal(a[4:].reshape(25, -1)[:, :a[0]], b[4:].reshape(25, -1)[:, :a[0]])
    most = engine.track_max_cap(256, 'lap')
    assert 600 <= most < engine.track_max_cap(256) and engine.TrackState(1, 20, assign='lap').max_cap == most
    with pytest.raises(engine.YkError, match=rf'cap {most + 1}.*{most} rows.*yk_track_max_cap_ex'):
        engine.TrackState(1, 20, assign='lap').update(torch.zeros((1, most + 1, 6), device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'), [0, 1])
    with pytest.raises(engine.YkError, match='assign 7'):
        engine.call('yk_track_max_cap_ex', 256, 7)
