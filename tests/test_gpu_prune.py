"""Magnitude pruning on the GPU (`make train PRUNE=True`; csrc/yk_prune.hip, train.Trainer(prune=...), training.cli): the kernels
against the numpy restatement tests/prune_ref.py (a full sort), the place of the masks inside the step against the unpruned step,
graph replay, two replicas, and the CLI with its checkpoint.  Every element of every segment is compared; nothing is sampled."""
import ctypes as C

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine, netspec as ns
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from k210_yolo_framework_amd.prune import PruneSchedule, prunable_layers
from tests import prune_ref

pytestmark = pytest.mark.gpu

HEADER = __import__('pathlib').Path(__file__).resolve().parents[1] / 'include' / 'yolo_hip.h'
SIZES = [1, 2, 255, 256, 257, 648, 65537, 1327104]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _masks(flat, offs, sizes, ks, fill=7):
    """One yk_prune_masks_f32 call over all segments -> (mask bytes of the whole flat buffer, thresholds, kept)."""
    L = engine.lib()
    TILE = L.yk_prune_tile()
    assert TILE == int(__import__('re').search(r'#define\s+YK_PRUNE_TILE\s+(\d+)', HEADER.read_text()).group(1))     # the library's is the header's
    first = np.concatenate([[0], np.cumsum([(n + TILE - 1) // TILE for n in sizes])]).astype(np.int32)
    p, off, size, keep, tf = _cu(flat), _cu(np.asarray(offs, np.int64)), _cu(np.asarray(sizes, np.int64)), _cu(np.asarray(ks, np.int64)), _cu(first)
    mask = torch.full((flat.size,), fill, dtype=torch.uint8, device='cuda')
    thr = torch.full((len(sizes),), -1.0, dtype=torch.float32, device='cuda')
    kept = torch.full((len(sizes),), -1, dtype=torch.int64, device='cuda')
    rc = L.yk_prune_masks_f32(engine._ptr(p), engine._ptr(off), engine._ptr(size), engine._ptr(keep), engine._ptr(tf), C.c_int(len(sizes)),
                              C.c_int(int(first[-1])), engine._ptr(mask), engine._ptr(thr), engine._ptr(kept), _st())
    assert rc == 0, L.yk_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy().view(np.uint32), flat.view(np.uint32))          # the parameters are only read
    return mask.cpu().numpy(), thr.cpu().numpy(), kept.cpu().numpy()


def _contents(kind, n, rng):
    if kind == 'normal':
        return rng.standard_normal(n).astype(np.float32)
    if kind == 'levels16':                                                # weights quantised to 16 levels: heavy ties
        return np.linspace(-1, 1, 16).astype(np.float32)[rng.integers(0, 16, n)]
    if kind == 'equal':
        return np.full(n, -0.37, np.float32)
    if kind == 'zero':
        return np.zeros(n, np.float32)
    if kind == 'zeros_denormals':                                         # +-0.0 and denormals (and the smallest normal)
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-45, 1e-40, -1e-40, -3e-39, 1.1754942e-38, 1.17549435e-38, -1.17549435e-38], np.float32)
        return pool[rng.integers(0, len(pool), n)]
    assert kind == 'normal_inf'
    w = rng.standard_normal(n).astype(np.float32)
    w[[0, n // 2, n - 1]] = [np.inf, -np.inf, np.inf][:1] if n == 1 else [np.inf, -np.inf, np.inf]
    return w


def _layout(sizes):
    """Segments in one flat buffer with gaps in front of, between and behind them; some start at odd element offsets."""
    offs, o = [], 5
    for i, n in enumerate(sizes):
        offs.append(o)
        o += n + (3, 8, 1, 13)[i % 4]
    return offs, o + 9


@pytest.mark.parametrize('kind', ['normal', 'levels16', 'equal', 'zero', 'zeros_denormals', 'normal_inf'])
def test_masks_thresholds_and_kept_counts_equal_a_sort(kind):
    rng = np.random.default_rng(SIZES.index(648) + len(kind))
    offs, total = _layout(SIZES)
    flat = rng.standard_normal(total).astype(np.float32) * 100                         # the gaps hold large values nobody may look at
    for o, n in zip(offs, SIZES):
        flat[o:o + n] = _contents(kind, n, rng)
    sch = PruneSchedule(0.5, 0.9, 1000, 100)
    variants = {'one': [1] * len(SIZES), 'all': list(SIZES), 'half': [max(1, n // 2) for n in SIZES]}
    for s in (0, 500, 1000):                                              # the schedule's own counts; it refuses k < 1 (n = 1, 2 ...): there k = 1
        ks = []
        for n in SIZES:
            k = prune_ref.keep_count(n, prune_ref.sparsity(s, 0.5, 0.9, 1000))
            if k < 1:
                with pytest.raises(engine.YkError, match='pruning'):
                    sch.keep_counts([n], s)
                k = 1
            else:
                assert sch.keep_counts([n], s).tolist() == [k]
            ks.append(k)
        variants[f'schedule{s}'] = ks
    for name, ks in variants.items():
        mask, thr, kept = _masks(flat, offs, SIZES, ks)
        mask2, thr2, kept2 = _masks(flat, offs, SIZES, ks)
        assert mask.tobytes() == mask2.tobytes() and thr.tobytes() == thr2.tobytes() and kept.tobytes() == kept2.tobytes(), name
        outside = np.ones(total, bool)
        for i, (o, n, k) in enumerate(zip(offs, SIZES, ks)):
            rthr, rmask, rkept = prune_ref.mask_of(flat[o:o + n], k)
            assert thr[i:i + 1].view(np.uint32)[0] == np.array([rthr], np.float32).view(np.uint32)[0], (kind, name, n, k, thr[i], rthr)
            assert np.array_equal(mask[o:o + n], rmask.astype(np.uint8)), (kind, name, n, k)
            assert kept[i] == rkept and kept[i] >= k, (kind, name, n, k, kept[i], rkept)
            outside[o:o + n] = False
        assert (mask[outside] == 7).all(), (kind, name)                  # bytes outside the segments are not written


def test_mask_apply_zeroes_exactly_the_masked_elements():
    L = engine.lib()
    rng = np.random.default_rng(3)
    for n, shift in ((1, 0), (3, 0), (4099, 0), (70001, 1), (1 << 20, 0)):       # shift 1: pointers that do not allow the 16-byte path
        w = rng.standard_normal(n + shift).astype(np.float32)
        w[rng.integers(0, n + shift, 5)] = -0.0
        m = (rng.uniform(size=n + shift) < 0.4).astype(np.uint8) * rng.integers(1, 255, n + shift).astype(np.uint8)   # any non-zero byte keeps
        p, md = _cu(w), _cu(m)
        pv, mv = p[shift:], md[shift:]
        assert L.yk_mask_apply_f32(engine._ptr(pv), engine._ptr(mv), C.c_longlong(n), _st()) == 0, L.yk_last_error()
        torch.cuda.synchronize()
        want = w.copy()
        want[shift:] = np.where(m[shift:] != 0, w[shift:], np.float32(0.0))
        assert p.cpu().numpy().tobytes() == want.tobytes(), n                         # masked elements are +0.0, the others untouched bits


def _anchors(spec):
    return VOC_ANCHORS if len(spec.outputs) == 2 else np.concatenate([VOC_ANCHORS, VOC_ANCHORS[:1] * 0.5])


def _case(name, hw, B, alpha, seed, steps=1):
    spec = ns.NETWORKS[name]([hw[0], hw[1], 3], 3, 20, alpha=alpha)
    w = spec.init_weights(seed)
    h = Helper(None, 20, _anchors(spec), [list(hw)], [list(x) for x in spec.out_hw()])
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(steps):
        ys = [[] for _ in spec.outputs]
        for b in range(B):
            n = int(rng.integers(1, 5))
            boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
            for i, lab in enumerate(h.box_to_label(boxes)):
                ys[i].append(lab)
        batches.append((rng.uniform(0, 1, (B, hw[0], hw[1], 3)).astype(np.float32), [np.stack(y).astype(np.float32) for y in ys]))
    return spec, w, h, batches


def _expected(spec, weights, sch, s):
    """name -> (threshold, mask, kept, k) of every prunable kernel from Keras-layout weights, by the numpy restatement."""
    out = {}
    for nm in prunable_layers(spec):
        w = np.asarray(weights[nm + '/kernel'], np.float32)
        k = prune_ref.keep_count(w.size, prune_ref.sparsity(s, sch.initial, sch.final, sch.end_step))
        out[nm + '/kernel'] = prune_ref.mask_of(w, k) + (k,)
    return out


@pytest.mark.parametrize('name,alpha', [('yolo_mobilev2', 1.0), ('yolo', 1.0)])
def test_real_segment_tables_of_the_flagship_and_darknet53(name, alpha):
    from k210_yolo_framework_amd.train import Trainer
    spec = ns.NETWORKS[name]([64, 96, 3], 3, 20, alpha=alpha)
    w = spec.init_weights(11)
    sch = PruneSchedule(0.5, 0.9, 1000, 100)
    tr = Trainer(spec, w, _anchors(spec), 1, prune=sch)
    assert all(r['kept'] == r['n'] and r['threshold'] == 0.0 for r in tr.prune_report().values())      # before the first update: all ones
    assert all(m.all() for m in tr.prune_masks().values())
    runs = []
    for s in (300, 300, 1000):
        tr.update_masks(s)
        torch.cuda.synchronize()
        runs.append((tr._pr_mask.cpu().numpy().tobytes(), tr._pr_thr.cpu().numpy().tobytes(), tr._pr_kept.cpu().numpy().tobytes()))
        masks, rep = tr.prune_masks(), tr.prune_report()
        exp = _expected(spec, w, sch, s)
        assert sorted(masks) == sorted(exp) == sorted(rep)
        for nm, (rthr, rmask, rkept, k) in exp.items():
            assert np.float32(rep[nm]['threshold']).view(np.uint32) == np.float32(rthr).view(np.uint32), (nm, s)
            assert masks[nm].shape == rmask.shape and np.array_equal(masks[nm], rmask), (nm, s)
            assert rep[nm]['kept'] == rkept and rep[nm]['n'] == rmask.size and rkept >= k, (nm, s)
    assert runs[0] == runs[1] and runs[0] != runs[2]
    # only prunable kernels carry zeros in the flat mask
    total_masked = int((tr._pr_mask == 0).sum().item())
    assert total_masked == sum(r['n'] - r['kept'] for r in tr.prune_report().values())
    if name == 'yolo':
        assert max(r['n'] for r in tr.prune_report().values()) == 3 * 3 * 512 * 1024                      # 4.7 M weights in one kernel


def test_step_order_masks_then_forward_backward_then_adam_on_everything():
    """Trainer A prunes at every step; Trainer B is plain and starts from A's weights times the reference mask of those weights.  One
    step each on the same batch from fresh Adam state: gradients and the parameters after the step are bitwise equal (Adam is not
    masked: the masked elements of A move too)."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, batches = _case('yolo_mobilev1', (64, 96), 4, 0.5, 41)
    x, yt = batches[0]
    sch = PruneSchedule(0.5, 0.9, 4, 1)
    a = Trainer(spec, w, h.anchors, 4, prune=sch)
    w0 = a.export_weights()
    exp = _expected(spec, w0, sch, 0)
    wb = dict(w0)
    for nm, (_, rmask, _, _) in exp.items():
        wb[nm] = np.where(rmask, w0[nm], np.float32(0.0)).astype(np.float32)
    b = Trainer(spec, wb, h.anchors, 4)
    ra = a.step(_cu(x), [_cu(y) for y in yt])
    rb = b.step(_cu(x), [_cu(y) for y in yt])
    assert ra == rb
    ga, gb = a.grads(), b.grads()
    for k in ga:
        assert ga[k].tobytes() == gb[k].tobytes(), k
    assert a.P.cpu().numpy().tobytes() == b.P.cpu().numpy().tobytes()
    for nm, (_, rmask, _, _) in exp.items():
        assert np.array_equal(a.prune_masks()[nm], rmask), nm
    moved = a.export_weights()
    assert any((moved[nm][~exp[nm][1]] != 0).any() for nm in exp)          # Adam updated masked elements (gradients are not masked)
    # a plain Trainer has no pruning state and refuses the accessors
    assert b.prune is None and not hasattr(b, '_pr_mask')
    with pytest.raises(engine.YkError, match='pruning'):
        b.apply_masks()


def _multi_step(use_graph, check):
    """yolo_mobilev1-0.75 at 64x96, F = 3, E = 6, 8 steps -> (flat parameters, flat mask, Adam moments) after the run."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, batches = _case('yolo_mobilev1', (64, 96), 4, 0.75, 43, steps=8)
    sch = PruneSchedule(0.5, 0.9, 6, 3)
    tr = Trainer(spec, w, h.anchors, 4, lr=1e-3, use_graph=use_graph, prune=sch)
    prev = tr.prune_masks()
    updates = 0
    for s, (x, yt) in enumerate(batches):
        assert tr.iterations == s
        before = tr.export_weights() if check else None
        tr.step(_cu(x), [_cu(y) for y in yt])
        if not check:
            continue
        masks = tr.prune_masks()
        if s <= 6 and s % 3 == 0:
            assert sch.is_update(s)
            updates += 1
            exp = _expected(spec, before, sch, s)
            rep = tr.prune_report()
            for nm, (rthr, rmask, rkept, k) in exp.items():
                assert np.array_equal(masks[nm], rmask), (s, nm)
                assert rep[nm]['kept'] == rkept and np.float32(rep[nm]['threshold']).view(np.uint32) == np.float32(rthr).view(np.uint32), (s, nm)
            if s:
                assert any(not np.array_equal(masks[nm], prev[nm]) for nm in masks), s      # the sparsity grew: the masks did change
        else:
            assert not sch.is_update(s)
            for nm in masks:
                assert np.array_equal(masks[nm], prev[nm]), (s, nm)                         # unchanged between updates
        prev = masks
    if check:
        assert updates == 3
        w_before = tr.export_weights()
        assert any((w_before[nm][~prev[nm]] != 0).any() for nm in prev)                    # Adam regrew masked weights after the last apply
        tr.apply_masks()
        w_after = tr.export_weights()
        for nm, m in prev.items():
            assert (w_after[nm][~m] == 0).all() and not np.signbit(w_after[nm][~m]).any(), nm   # every masked element is exactly +0
            assert w_after[nm][m].tobytes() == w_before[nm][m].tobytes(), nm
        for k in w_after:                                                                   # depthwise kernels, biases, BatchNorm: no forced zero
            if k not in prev:
                assert w_after[k].tobytes() == w_before[k].tobytes(), k
        for l in spec.layers:
            if l.kind == 'dwconv':
                assert (w_after[l.name + '/kernel'] != 0).all(), l.name
        off_limits = torch.ones_like(tr._pr_mask, dtype=torch.bool)
        for nm in prev:
            o, shp = tr.slots[nm]
            off_limits[o:o + int(np.prod(shp))] = False
        assert bool((tr._pr_mask[off_limits] == 1).all())
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (tr.P, tr._pr_mask, tr.m, tr.v, tr.G)]


def test_multi_step_run_masks_follow_the_schedule():
    _multi_step(True, check=True)


def test_graph_replay_and_eager_runs_are_bitwise_equal_across_an_update_after_the_capture():
    """Steps 0 (eager) and 1 (capture + replay) come first; the updates of steps 3 and 6 rewrite the mask and P in place under the captured graph."""
    eager, graph = _multi_step(False, check=False), _multi_step(True, check=False)
    for a, b, what in zip(eager, graph, ('P', 'mask', 'm', 'v', 'G')):
        assert a == b, what


def test_two_replicas_keep_identical_masks_and_parameters():
    """Data-parallel: every rank computes the masks from its own replica; no exchange is added.  Two replicas of one process driven
    through the `reduce=` hook, like tests/test_gpu_train_dp.py."""
    from k210_yolo_framework_amd import shard
    from k210_yolo_framework_amd.train import Trainer
    GB = 8
    spec, w, h, batches = _case('yolo_mobilev1', (64, 96), GB, 0.5, 47, steps=5)
    sch = PruneSchedule(0.5, 0.9, 4, 2)
    reps = [Trainer(spec, w, h.anchors, GB // 2, lr=1e-3, world_size=2, prune=sch) for _ in range(2)]
    for x, yt in batches:
        for r, tr in enumerate(reps):
            tr.prune_step()
            idx = shard.shard_indices(GB, r, 2)
            tr._loss_and_grads_replayed(_cu(x[idx]), [_cu(y[idx]) for y in yt])
        total = reps[0].G + reps[1].G
        for tr in reps:
            tr.exchange(reduce=lambda g: g.copy_(total))
            tr.apply_update()
        torch.cuda.synchronize()
        assert reps[0]._pr_mask.cpu().numpy().tobytes() == reps[1]._pr_mask.cpu().numpy().tobytes()
        assert reps[0].P.cpu().numpy().tobytes() == reps[1].P.cpu().numpy().tobytes()
    assert reps[0].prune_report() == reps[1].prune_report()
    assert any(r['kept'] < r['n'] for r in reps[0].prune_report().values())


def test_make_train_prune_cli_saves_a_pruned_checkpoint_the_inference_model_loads(tmp_path, capsys):
    """56 training images / 4 per step = 14 steps per epoch, prune_end_epoch 1 -> end_step 14, frequency 2: the last update is step 14,
    at the final sparsity; two epochs."""
    from k210_yolo_framework_amd import training, yolonet
    common = ['--synthetic', '64', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '4', '--max_nrof_epochs', '2',
              '--vaildation_split', '0.125', '--obj_weight', '1', '--noobj_weight', '1', '--wh_weight', '1', '--iou_thresh', '0.5']
    tr = training.cli(common + ['--log_dir', str(tmp_path / 'p'), '--is_prune', 'True', '--prune_end_epoch', '1', '--prune_frequency', '2'])
    out = capsys.readouterr().out
    ck = list((tmp_path / 'p').glob('*/yolo_prune_model.h5'))
    assert len(ck) == 1 and (ck[0].parent / 'yolo_prune_model.npz').exists() and not (ck[0].parent / 'yolo_model.h5').exists()
    assert 'Save Pruned Model as' in out and out.count('target sparsity') == 2 and 'achieved' in out
    assert tr.iterations == 28 and tr.prune.end_step == 14
    spec = tr.spec
    saved = dict(np.load(ck[0].parent / 'yolo_prune_model.npz'))
    rep = tr.prune_report()
    names = [n + '/kernel' for n in prunable_layers(spec)]
    assert sorted(rep) == sorted(names)
    for nm in names:
        n = saved[nm].size
        k = prune_ref.keep_count(n, prune_ref.sparsity(14, 0.5, 0.9, 14))                  # the final sparsity, 0.9
        zeros = int((saved[nm] == 0).sum())
        print(nm, 'n', n, 'k', k, 'zeros', zeros, 'kept', rep[nm]['kept'])
        assert zeros >= n - k, (nm, zeros, n, k)
        if rep[nm]['kept'] == k and (saved[nm][tr.prune_masks()[nm]] != 0).all():          # no tie at the threshold (and no weight that is 0 by itself)
            assert zeros == n - k, (nm, zeros, n, k)
    for l in spec.layers:                                                                   # nothing else was masked
        if l.kind == 'dwconv':
            assert (saved[l.name + '/kernel'] != 0).all(), l.name
    model, wrapper = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.5)
    wrapper.load_weights(str(ck[0]))
    x = np.random.default_rng(0).uniform(0, 1, (2, 224, 320, 3)).astype(np.float32)
    y = wrapper.predict(x)
    assert [t.shape for t in y] == [(2, 7, 10, 3, 25), (2, 14, 20, 3, 25)] and all(np.isfinite(t).all() for t in y)
    _, w2 = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.5)
    w2.load_weights(str(ck[0].parent / 'yolo_prune_model.npz'))
    for a, b in zip(y, w2.predict(x)):
        np.testing.assert_array_equal(a, b)
    # without the switch: the plain checkpoint, as before
    tr2 = training.cli(common + ['--log_dir', str(tmp_path / 'n'), '--is_prune', 'False', '--max_steps', '3'])
    out = capsys.readouterr().out
    assert len(list((tmp_path / 'n').glob('*/yolo_model.h5'))) == 1 and not list((tmp_path / 'n').glob('*/yolo_prune_model.h5'))
    assert 'Save Model as' in out and 'Pruned' not in out and tr2.prune is None
