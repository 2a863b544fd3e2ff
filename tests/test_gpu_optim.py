"""Weight EMA, learning-rate schedule and gradient clipping on the GPU (`make train EMA=True CLIPNORM=10 LRSCHED=cosine`; csrc/yk_optim.hip,
train.Trainer(ema=, clip_norm=, lr_schedule=), training.cli): the three kernels through the C-ABI against optim.py's float32 restatements
(tests/test_optim.py checks those first) and against yk_adam_f32, then the Trainer step by step, the replayed graph, pruning, the refusals
and the CLI with its checkpoint.  Every element is compared; nothing is sampled."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine, netspec as ns, optim
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from k210_yolo_framework_amd.optim import EmaConfig, LrSchedule
from tests import optim_cases as oc
from tests import train_cases as tc

pytestmark = pytest.mark.gpu

SENTINEL, TAIL = 12345.0, 64


def _L():
    engine.require_gpu()
    return engine.lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).cuda()                       # (a copy: the shared problems are read-only)


def _buf(init, dtype=torch.float32):
    """A device copy of `init` as a view of a sentinel-tailed buffer -> (view, whole buffer)."""
    init = np.asarray(init)
    b = torch.full((init.size + TAIL,), SENTINEL, dtype=dtype, device='cuda')
    b[:init.size].copy_(torch.from_numpy(np.array(init)))
    return b[:init.size], b


def _tails(*bufs):
    for k, b in enumerate(bufs):
        assert bool((b[-TAIL:] == SENTINEL).all()), f'buffer {k}: written past its end'


def _bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (what, int(bad.size), bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def _sumsq(L, x, n):
    """yk_sumsq_f32 on device tensor x -> the device double (a 1-element tensor).  The workspace is exactly what the query asks for."""
    nb = C.c_size_t()
    assert L.yk_sumsq_workspace_bytes(C.c_longlong(n), C.byref(nb)) == 0, L.yk_last_error()
    assert nb.value == 8 * ((n + oc.SUMSQ_TILE - 1) // oc.SUMSQ_TILE)
    work, wb = _buf(np.full(nb.value // 8, -7.0), torch.float64)
    out, ob = _buf(np.full(1, -7.0), torch.float64)
    assert L.yk_sumsq_f32(x, C.c_longlong(n), work, out, _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    _tails(wb, ob)
    return out


def _adam_ex(L, n, p, g, m, v, ema, sumsq, it, gs, dc, clip_norm=0.0, omd=0.0, lr=tc.ADAM_LR):
    rc = L.yk_adam_ex_f32(C.c_longlong(n), p, g, m, v, ema, sumsq, C.c_float(lr), C.c_float(dc), C.c_longlong(it), C.c_float(tc.ADAM_B1),
                          C.c_float(tc.ADAM_B2), C.c_float(tc.ADAM_EPS), C.c_float(gs), C.c_float(clip_norm), C.c_float(omd), _st())
    assert rc == 0, L.yk_last_error()


def _adam(L, n, p, g, m, v, it, gs, dc):
    rc = L.yk_adam_f32(C.c_longlong(n), p, g, m, v, C.c_float(tc.ADAM_LR), C.c_float(dc), C.c_longlong(it), C.c_float(tc.ADAM_B1),
                       C.c_float(tc.ADAM_B2), C.c_float(tc.ADAM_EPS), C.c_float(gs), _st())
    assert rc == 0, L.yk_last_error()


# --------------------------------------------------------------------------------------------- yk_sumsq_f32
@pytest.mark.parametrize('n', oc.NS)
def test_sumsq_is_the_float64_sum_of_exact_squares_and_reproducible(n):
    """|out - fsum(x^2)| <= n 2^-53 fsum(x^2) with +-1e-20 (square subnormal in float32) and +-1e25 (square overflows float32) among the
    inputs; a second call and a call on a pointer that does not allow the 16-byte path give the same bits; all zeros give +0.0."""
    L = _L()
    pr = oc.sumsq_problem(n)
    x = _cu(pr['x'])
    a = float(_sumsq(L, x, n).cpu().numpy()[0])
    print('sumsq', n, a, pr['ref'], 'error / bound', abs(a - pr['ref']) / oc.sumsq_bound(n, pr['ref']))
    assert math.isfinite(a) and abs(a - pr['ref']) <= oc.sumsq_bound(n, pr['ref'])
    if n >= 8:
        assert a > 1e49                                                      # the 1e25 entries are in it
    b = float(_sumsq(L, x, n).cpu().numpy()[0])
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    shifted = torch.cat([torch.zeros(1, device='cuda'), x])[1:]              # 4 bytes off a 16-byte boundary: the element-wise loads
    assert shifted.data_ptr() % 16 == 4
    c = float(_sumsq(L, shifted, n).cpu().numpy()[0])
    assert np.float64(a).tobytes() == np.float64(c).tobytes()
    assert np.array_equal(x.cpu().numpy().view(np.uint32), pr['x'].view(np.uint32))     # only read
    z = _sumsq(L, torch.zeros(n, device='cuda'), n).cpu().numpy()
    assert z[0] == 0.0 and not np.signbit(z[0])


def test_sumsq_and_friends_refuse_bad_arguments():
    L = _L()
    x, d = torch.ones(16, device='cuda'), torch.full((4,), -7.0, dtype=torch.float64, device='cuda')
    nb = C.c_size_t(77)
    ll, fl = C.c_longlong, C.c_float
    assert L.yk_sumsq_workspace_bytes(ll(0), C.byref(nb)) == -10 and L.yk_sumsq_workspace_bytes(ll(16), None) == -10 and nb.value == 77
    for args in ((None, ll(16), d, d[1:]), (x, ll(0), d, d[1:]), (x, ll(16), None, d[1:]), (x, ll(16), d, None)):
        assert L.yk_sumsq_f32(*args, _st()) == -10
    adam = lambda n=16, p=x, g=x, m=x, v=x, it=0, sq=None, clip=0.0: (ll(n), p, g, m, v, None, sq, fl(5e-4), fl(0), ll(it), fl(.9), fl(.999),
                                                                      fl(1e-7), fl(1), fl(clip), fl(0), _st())
    for args in (adam(p=None), adam(g=None), adam(m=None), adam(v=None), adam(n=0), adam(it=-1), adam(sq=d, clip=-1.0)):
        assert L.yk_adam_ex_f32(*args) == -10
    for args in ((ll(16), None, x, fl(.5)), (ll(16), x, None, fl(.5)), (ll(0), x, x, fl(.5))):
        assert L.yk_ema_f32(*args, _st()) == -10
    torch.cuda.synchronize()
    assert bool((x == 1).all()) and bool((d == -7).all())                    # nothing was launched


# --------------------------------------------------------------------------------------------- yk_adam_ex_f32
@pytest.mark.parametrize('case', tc.ADAM_CASES, ids=str)
def test_adam_ex_without_options_is_yk_adam_f32_bit_for_bit(case):
    L = _L()
    n, it, gs, dc, warm = case
    pr = tc.adam_problem(case)
    g = _cu(pr['g'])
    (p, pb), (m, mb), (v, vb) = _buf(pr['p']), _buf(pr['m']), _buf(pr['v'])
    (p2, pb2), (m2, mb2), (v2, vb2) = _buf(pr['p']), _buf(pr['m']), _buf(pr['v'])
    _adam(L, n, p, g, m, v, it, gs, dc)
    _adam_ex(L, n, p2, g, m2, v2, None, None, it, gs, dc)
    torch.cuda.synchronize()
    _tails(pb, mb, vb, pb2, mb2, vb2)
    for a, b, k in ((p, p2, 'p'), (m, m2, 'm'), (v, v2, 'v')):
        _bits(b, a.cpu().numpy(), k)
        _bits(b, pr[k + '32'], k + ' (restatement)')


@pytest.mark.parametrize('n', oc.NS)
def test_clipping_matches_the_restatement_and_leaves_g_alone(n):
    """The kernel's own sum of squares read back, c formed from it by optim.py: p, m, v bit for bit at a norm above clip_norm (grad_scale 1/8
    as well: the product is formed before c), the unclipped bits at a norm below it, g unchanged, and no NaN where c underflows."""
    L = _L()
    pr, gp = oc.ema_problem(n), oc.gradient_problem(n)
    g = _cu(gp['g'])
    sq = _sumsq(L, g, n)
    s = float(sq.cpu().numpy()[0])
    assert abs(s - gp['sumsq']) <= oc.sumsq_bound(n, gp['sumsq'])
    norm = math.sqrt(s)
    for clip, gs in ((0.5 * norm, 1.0), (0.25 * norm, 0.125), (4.0 * norm + 1.0, 1.0), (1e-44, 1.0)):
        clip = float(np.float32(clip))
        c = optim.clip_coefficient_f32(s, clip)
        (p, pb), (m, mb), (v, vb) = _buf(pr['p']), _buf(pr['m']), _buf(pr['v'])
        _adam_ex(L, n, p, g, m, v, None, sq, 9, gs, 0.0, clip_norm=clip)
        torch.cuda.synchronize()
        _tails(pb, mb, vb)
        want = optim.adam_ex_step_f32(pr['p'], gp['g'], pr['m'], pr['v'], tc.ADAM_LR, 0.0, 9, tc.ADAM_B1, tc.ADAM_B2, tc.ADAM_EPS, gs, c=c)
        for got, w, k in zip((p, m, v), want, 'pmv'):
            _bits(got, w, (k, n, clip))
            assert np.isfinite(got.cpu().numpy()).all(), (k, n, clip)
        if clip > norm + 1e-6:                                               # below the threshold: the bits of the update without clipping
            assert c == 1.0
            plain = tc.adam_step_f32(pr['p'], gp['g'], pr['m'], pr['v'], 9, gs, 0.0)
            for got, w, k in zip((p, m, v), plain, 'pmv'):
                _bits(got, w, (k, n, 'unclipped'))
        else:
            assert c < 1.0 and (n < 255 or not np.array_equal(m.cpu().numpy(), tc.adam_step_f32(pr['p'], gp['g'], pr['m'], pr['v'], 9, gs, 0.0)[1]))
    assert c < 2.0 ** -126 and np.float32(1e-44) > 0                         # the last c is subnormal (or 0): its products with g underflow
    _bits(g, gp['g'], 'g')


@pytest.mark.parametrize('n', oc.NS)
def test_ema_fused_and_alone_match_the_restatement(n):
    L = _L()
    pr = oc.ema_problem(n)
    g = _cu(pr['g'])
    for omd in (oc.OMD, oc.OMD_LATE, 0.0):
        want_e = optim.ema_step_f32(pr['e'], pr['p32'], omd)
        # fused
        (p, pb), (m, mb), (v, vb), (e, eb) = _buf(pr['p']), _buf(pr['m']), _buf(pr['v']), _buf(pr['e'])
        _adam_ex(L, n, p, g, m, v, e, None, 9, 1.0, 0.0, omd=omd)
        # yk_adam_f32 followed by yk_ema_f32
        (p2, pb2), (m2, mb2), (v2, vb2), (e2, eb2) = _buf(pr['p']), _buf(pr['m']), _buf(pr['v']), _buf(pr['e'])
        _adam(L, n, p2, g, m2, v2, 9, 1.0, 0.0)
        assert L.yk_ema_f32(C.c_longlong(n), p2, e2, C.c_float(omd), _st()) == 0, L.yk_last_error()
        torch.cuda.synchronize()
        _tails(pb, mb, vb, eb, pb2, mb2, vb2, eb2)
        for got, k in ((p, 'p32'), (m, 'm32'), (v, 'v32'), (p2, 'p32'), (m2, 'm32'), (v2, 'v32')):
            _bits(got, pr[k], (k, n, omd))                                   # p, m, v are untouched by the average's presence
        _bits(e, want_e, ('ema fused', n, omd))
        _bits(e2, want_e, ('ema alone', n, omd))
        same = pr['e'] == pr['p32']
        assert same[::5].all()
        _bits(e.cpu().numpy()[same], pr['e'][same], 'ema == p_new keeps its bits')
        if omd == 0.0:
            _bits(e, pr['e'], 'ema_omd = 0 keeps the bits')
        else:
            assert n < 255 or not np.array_equal(e.cpu().numpy(), pr['e'])
    # all three parts in one launch, and on pointers that do not allow the 16-byte path
    gp = oc.gradient_problem(n)
    g = _cu(gp['g'])
    sq = _sumsq(L, g, n)
    s = float(sq.cpu().numpy()[0])
    clip = float(np.float32(0.5 * math.sqrt(s)))
    want = optim.adam_ex_step_f32(pr['p'], gp['g'], pr['m'], pr['v'], tc.ADAM_LR, 0.0, 9, tc.ADAM_B1, tc.ADAM_B2, tc.ADAM_EPS, 1.0,
                                  c=optim.clip_coefficient_f32(s, clip), ema=pr['e'], omd=oc.OMD)
    for shift in (0, 1):
        bufs = [_buf(np.concatenate([np.zeros(shift, np.float32), pr[k]])) for k in 'pmve']
        views = [b[0][shift:] for b in bufs]
        _adam_ex(L, n, views[0], g, views[1], views[2], views[3], sq, 9, 1.0, 0.0, clip_norm=clip, omd=oc.OMD)
        torch.cuda.synchronize()
        _tails(*[b[1] for b in bufs])
        for got, w, k in zip(views, want, 'pmve'):
            _bits(got, w, (k, n, 'all parts', shift))
        assert all(float(b[0][0]) == 0.0 for b in bufs if shift)


# --------------------------------------------------------------------------------------------- Trainer
def _batches(spec, h, hw, B, seed, steps):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        ys = [[] for _ in spec.outputs]
        for b in range(B):
            k = int(rng.integers(1, 4))
            boxes = np.stack([rng.integers(0, 20, k), rng.uniform(.2, .8, k), rng.uniform(.2, .8, k), rng.uniform(.1, .6, k), rng.uniform(.1, .6, k)], 1)
            for i, lab in enumerate(h.box_to_label(boxes)):
                ys[i].append(lab)
        out.append((rng.uniform(0, 1, (B, hw[0], hw[1], 3)).astype(np.float32), [np.stack(y).astype(np.float32) for y in ys]))
    return out


@pytest.fixture(scope='module')
def mini():
    from tests.qat_ref import mini_case
    spec, w, h, _, _ = mini_case(7, B=4)
    return spec, w, h, _batches(spec, h, (32, 32), 4, 70, 5)


def _trainer(mini, **kw):
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, _ = mini
    return Trainer(spec, w, h.anchors, 4, lr=1e-3, **kw)


def _run(tr, batches, each=None):
    outs = []
    for k, (x, yt) in enumerate(batches):
        if each is not None:
            each(tr, k)
        outs.append(tr.step(_cu(x), [_cu(y) for y in yt]))
    torch.cuda.synchronize()
    return outs


def _state(tr):
    return {k: getattr(tr, k).cpu().numpy() for k in ('P', 'm', 'v', 'M')}


@pytest.fixture(scope='module')
def plain_run(mini):
    """Five plain steps, with P and the moving statistics after each: computed once, shared."""
    tr = _trainer(mini)
    start = (tr.P.cpu().numpy(), tr.M.cpu().numpy())
    snaps, outs = [], []
    for x, yt in mini[3]:
        outs.append(tr.step(_cu(x), [_cu(y) for y in yt]))
        snaps.append((tr.P.cpu().numpy(), tr.M.cpu().numpy()))
    return dict(start=start, snaps=snaps, outs=outs, state=_state(tr))


def test_default_trainer_issues_yk_adam_f32_and_allocates_no_average(mini, monkeypatch):
    names = []
    real = engine.call
    monkeypatch.setattr(engine, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    tr = _trainer(mini)
    out = _run(tr, mini[3][:3])
    assert names.count('yk_adam_f32') == 3 and not {'yk_adam_ex_f32', 'yk_sumsq_f32', 'yk_ema_f32', 'yk_sumsq_workspace_bytes'} & set(names)
    assert tr.E is None and tr.EM is None and not hasattr(tr, '_sumsq') and not hasattr(tr, 'ema_moving')
    assert all('lr' not in o and 'grad_norm' not in o for o in out)
    with pytest.raises(engine.YkError, match='ema'):
        tr.export_weights(ema=True)
    names.clear()
    tr2 = _trainer(mini, ema=EmaConfig(), clip_norm=10.0, lr_schedule=LrSchedule('constant', 1e-3, 10))
    _run(tr2, mini[3][:1])
    assert 'yk_adam_f32' not in names and [names.count(k) for k in ('yk_sumsq_f32', 'yk_adam_ex_f32', 'yk_ema_f32')] == [1, 1, 1]
    assert names.index('yk_sumsq_f32') < names.index('yk_adam_ex_f32') < names.index('yk_ema_f32')


def test_ema_does_not_disturb_training_and_follows_the_recurrence(mini, plain_run):
    cfg = EmaConfig(0.9, 3.0)                                                # a decay that moves the average visibly in five updates
    tr = _trainer(mini, ema=cfg)
    _bits(tr.E, plain_run['start'][0], 'E starts as P')
    _bits(tr.EM, plain_run['start'][1], 'the averaged statistics start as the statistics')
    outs = _run(tr, mini[3])
    assert outs == plain_run['outs'] and tr.ema_updates == 5
    for k, v in _state(tr).items():
        _bits(v, plain_run['state'][k], k)
    e, em = plain_run['start']
    for k, (p, mv) in enumerate(plain_run['snaps']):
        omd = cfg.omd_at(k + 1)
        e, em = optim.ema_step_f32(e, p, omd), optim.ema_step_f32(em, mv, omd)
    _bits(tr.E, e, 'E')
    _bits(tr.EM, em, 'averaged moving statistics')
    assert not np.array_equal(e, plain_run['snaps'][-1][0]) and not np.array_equal(em, plain_run['snaps'][-1][1])
    live, avg = tr.export_weights(), tr.export_weights(ema=True)
    assert sorted(live) == sorted(avg) and all(live[k].shape == avg[k].shape and live[k].dtype == avg[k].dtype for k in live)
    assert all(not np.array_equal(live[k], avg[k]) for k in live if k.endswith(('/kernel', '/moving_mean')))
    for nm, t in tr.ema_moving.items():                                      # the views are the flat buffer's
        o, c = tr.mslots[nm]
        assert np.array_equal(avg[nm], em[o:o + c]) and np.array_equal(live[nm], tr.moving[nm].cpu().numpy())
    tr.load_weights(live)                                                    # loading starts the average again
    _bits(tr.E, tr.P.cpu().numpy(), 'E after load_weights')
    _bits(tr.EM, tr.M.cpu().numpy(), 'EM after load_weights')


def test_replayed_graph_equals_eager_steps_with_all_options(mini):
    runs = []
    for use_graph in (False, True):
        tr = _trainer(mini, use_graph=use_graph, ema=EmaConfig(0.9, 3.0), clip_norm=0.05, lr_schedule=LrSchedule('cosine', 1e-3, 5, warmup_steps=2))
        outs = _run(tr, mini[3])
        assert (tr._graph is not None) == use_graph
        runs.append((outs, {**_state(tr), 'E': tr.E.cpu().numpy(), 'EM': tr.EM.cpu().numpy()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        _bits(runs[1][1][k], runs[0][1][k], k)
    assert any(o['grad_norm'] > 0.05 for o in runs[0][0])                    # the clip did act


def test_schedule_equals_setting_lr_by_hand(mini):
    sch = LrSchedule('cosine', 1e-3, 5, warmup_steps=2)
    a = _trainer(mini, lr_schedule=sch)
    outs = _run(a, mini[3])
    assert [o['lr'] for o in outs] == [sch.lr_at(k) for k in range(5)] and len({o['lr'] for o in outs}) >= 4
    b = _trainer(mini)
    _run(b, mini[3], each=lambda tr, k: setattr(tr, 'lr', sch.lr_at(k)))
    sa, sb = _state(a), _state(b)
    for k in sa:
        _bits(sa[k], sb[k], k)


def test_clipping_reports_the_norm_and_clips_by_the_restatement(mini, plain_run):
    x, yt = mini[3][0]
    far = _trainer(mini, clip_norm=1e9)                                      # far above the norm: the plain step's bits
    out = far.step(_cu(x), [_cu(y) for y in yt])
    torch.cuda.synchronize()
    g = far.G.cpu().numpy()
    ref = math.fsum((g.astype(np.float64) ** 2).tolist())
    norm = out['grad_norm']
    print('grad_norm', norm, 'reference', math.sqrt(ref))
    assert abs(norm * norm - ref) <= oc.sumsq_bound(g.size, ref) + 4 * 2.0 ** -53 * ref       # (the square root and its square: two roundings each way)
    _bits(far.P, plain_run['snaps'][0][0], 'P, clip_norm far above the norm')
    assert {k: v for k, v in out.items() if k != 'grad_norm'} == plain_run['outs'][0]
    half = _trainer(mini, clip_norm=0.5 * norm)
    p0 = half.P.cpu().numpy()
    out2 = half.step(_cu(x), [_cu(y) for y in yt])
    torch.cuda.synchronize()
    assert out2['grad_norm'] == norm                                         # the same gradient, the same tree
    _bits(half.G, g, 'G is not written by the clip')
    c = optim.clip_coefficient_f32(float(half._sumsq.cpu().numpy()[0]), 0.5 * norm)
    assert 0.49 < c < 0.51
    want = optim.adam_ex_step_f32(p0, g, np.zeros_like(g), np.zeros_like(g), 1e-3, 0.0, 0, c=c)
    for got, w, k in zip((half.P, half.m, half.v), want, 'Pmv'):
        _bits(got, w, k)
    assert not np.array_equal(half.P.cpu().numpy(), plain_run['snaps'][0][0])


def test_pruning_masks_the_average_too():
    from k210_yolo_framework_amd.prune import PruneSchedule
    from k210_yolo_framework_amd.train import Trainer
    spec = ns.NETWORKS['yolo_mobilev1']([64, 96, 3], 3, 20, alpha=0.75)
    h = Helper(None, 20, VOC_ANCHORS, [[64, 96]], [list(v) for v in spec.out_hw()])
    tr = Trainer(spec, spec.init_weights(43), h.anchors, 4, lr=1e-3, prune=PruneSchedule(0.5, 0.9, 4, 1), ema=EmaConfig(0.9, 0.0))
    _run(tr, _batches(spec, h, (64, 96), 4, 43, 2))
    masks = tr.prune_masks()
    before = tr.export_weights(ema=True)
    assert any((before[nm][~m] != 0).any() for nm, m in masks.items())       # the average of regrown weights is not sparse by itself
    tr.apply_masks()
    after, live = tr.export_weights(ema=True), tr.export_weights()
    for nm, m in masks.items():
        assert not m.all() and (after[nm][~m] == 0).all() and (live[nm][~m] == 0).all(), nm
        assert after[nm][m].tobytes() == before[nm][m].tobytes(), nm
    for k in after:
        if k not in masks:
            assert after[k].tobytes() == before[k].tobytes(), k


def test_refusals(mini):
    from k210_yolo_framework_amd.qat import QatConfig
    with pytest.raises(engine.YkError, match='ema= together with qat='):
        _trainer(mini, ema=EmaConfig(), qat=QatConfig(0.99))
    with pytest.raises(engine.YkError, match='two learning-rate schedules'):
        _trainer(mini, lr_schedule=LrSchedule('cosine', 1e-3, 5), decay=0.01)
    with pytest.raises(engine.YkError, match='clip_norm'):
        _trainer(mini, clip_norm=-1.0)
    with pytest.raises(engine.YkError, match='ema=None'):
        _trainer(mini, clip_norm=1.0).export_weights(ema=True)


def test_make_train_cli_saves_the_averaged_checkpoint(tmp_path, capsys):
    from k210_yolo_framework_amd import training, yolonet
    common = ['--synthetic', '32', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '4', '--max_nrof_epochs', '1',
              '--vaildation_split', '0.125', '--obj_weight', '1', '--noobj_weight', '1', '--wh_weight', '1', '--iou_thresh', '0.5', '--max_steps', '3']
    tr = training.cli(common + ['--log_dir', str(tmp_path / 'e'), '--ema', 'True', '--lr_schedule', 'cosine', '--warmup_steps', '2', '--clip_norm', '10'])
    out = capsys.readouterr().out
    ck = list((tmp_path / 'e').glob('*/yolo_ema_model.h5'))
    assert len(ck) == 1 and (ck[0].parent / 'yolo_ema_model.npz').exists() and (ck[0].parent / 'yolo_model.h5').exists()
    assert tr.iterations == 3 and tr.ema_updates == 3 and tr.lr_schedule.total_steps == 3 and tr.lr_schedule.warmup_steps == 2
    step_lines = [l for l in out.splitlines() if ' step ' in l]
    assert step_lines and all(' lr ' in l and ' gnorm ' in l for l in step_lines) and '(ema)' in out and 'Save EMA Model as' in out
    args = (ck[0].parent / 'args.txt').read_text()
    assert 'ema: True' in args and 'lr_schedule: cosine' in args and 'clip_norm: 10.0' in args and 'warmup_steps: 2' in args
    saved, avg = dict(np.load(ck[0].parent / 'yolo_ema_model.npz')), tr.export_weights(ema=True)
    assert sorted(saved) == sorted(avg) and all(np.array_equal(saved[k], avg[k]) for k in avg)
    live = dict(np.load(ck[0].parent / 'yolo_model.npz'))
    assert any(not np.array_equal(saved[k], live[k]) for k in live)
    model, wrapper = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.5)
    wrapper.load_weights(str(ck[0]))
    x = np.random.default_rng(0).uniform(0, 1, (2, 224, 320, 3)).astype(np.float32)
    y = wrapper.predict(x)
    assert [t.shape for t in y] == [(2, 7, 10, 3, 25), (2, 14, 20, 3, 25)] and all(np.isfinite(t).all() for t in y)
    # without the new flags: no such file, no new words on the step lines
    tr2 = training.cli(common + ['--log_dir', str(tmp_path / 'n')])
    out = capsys.readouterr().out
    assert len(list((tmp_path / 'n').glob('*/yolo_model.h5'))) == 1 and not list((tmp_path / 'n').glob('*/*ema*'))
    step_lines = [l for l in out.splitlines() if ' step ' in l]
    assert step_lines and not any(' lr ' in l or 'gnorm' in l for l in step_lines) and '(ema)' not in out and 'EMA' not in out
    assert tr2.E is None and tr2.lr_schedule is None and tr2.clip_norm == 0.0
