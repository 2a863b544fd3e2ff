"""Quantisation-aware training on the GPU (`make train QAT=True`; csrc/yk_qat.hip, train.Trainer(qat=...), training.cli, make_kmodel
--ranges).  The kernels against the float32 numpy restatement tests/qat_ref.py bit for bit, the wiring of the tape against
the float64 autograd restatement, graph replay, off-means-off, pruning + QAT, and the round trip through the CLI to a kmodel the KPU
runner loads.  Every comparison covers every element."""
import ctypes as C

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine, kmodel, netspec as ns, quantize
from k210_yolo_framework_amd.qat import QatConfig, SLOT_NONE, SLOT_OWNER, SLOT_UNION
from tests import qat_ref
from tests.test_gpu_train import _close, _gate_flips

pytestmark = pytest.mark.gpu

RANGES = [(-1.0, 3.0), (0.5, 2.0), (-2.0, -0.5), (0.0, 0.0)]                 # (0.5, 2) and (-2, -0.5) are widened to 0; zero width
HYPER = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _range_table():
    return _cu(np.asarray(RANGES, np.float32).reshape(-1))


def _batch_table(n_slots):
    L = engine.lib()
    t = torch.zeros(4 * n_slots, dtype=torch.int32, device='cuda')
    assert L.yk_range_reset(engine._ptr(t), C.c_int(n_slots), _st()) == 0
    return t


def _read_batch(t, n_slots):
    L = engine.lib()
    lo, hi, fl = np.empty(n_slots, np.float32), np.empty(n_slots, np.float32), np.empty(n_slots, np.int32)
    torch.cuda.synchronize()
    assert L.yk_range_read(engine._ptr(t), C.c_int(n_slots), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                           fl.ctypes.data_as(C.c_void_p)) == 0
    return lo, hi, fl


def _values(lo, hi, n, rng):
    """Beyond both ends of the range, exact k + 0.5 steps, -0.0, denormals, and values inside; the first n of a seeded shuffle."""
    s, zp = qat_ref.qparams32(lo, hi)
    ties = ((np.arange(-3, 259, dtype=np.float32) + np.float32(0.5)) - zp) * s
    pool = np.concatenate([ties, (np.arange(-6, 262, dtype=np.float32) - zp) * s, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39], np.float32),
                           np.array([-1e6, 1e6, -300 * s, 300 * s], np.float32),
                           rng.uniform(float(-zp * s) - 0.3, float((255 - zp) * s) + 0.3, 4200).astype(np.float32)]).astype(np.float32)
    pool = pool[rng.permutation(len(pool))]
    head = np.array([-0.0, 300 * s, ties[7], 1e-45], np.float32)              # the small sizes see the edge cases too
    return np.concatenate([head, pool])[:n].copy() if n > 1 else np.array([ties[7]], np.float32)


@pytest.mark.parametrize('n', [1, 3, 4, 4099])
@pytest.mark.parametrize('shift', [0, 1])
def test_activation_forward_and_backward_equal_the_restatement_bitwise(n, shift):
    """shift 1: pointers one float off a 16-byte boundary (a scalar head, or no 16-byte access at all where the two differ)."""
    L = engine.lib()
    rng = np.random.default_rng(100 * n + shift)
    rt = _range_table()
    for slot, (lo, hi) in enumerate(RANGES):
        for shift_q in (shift, 0):
            x = _values(lo, hi, n, rng)
            g = rng.standard_normal(n).astype(np.float32)
            xd = _cu(np.concatenate([np.zeros(shift, np.float32), x, np.float32([7.0])]))
            qd = torch.full((shift_q + n + 3,), 7.0, dtype=torch.float32, device='cuda')
            bt = _batch_table(len(RANGES))
            assert L.yk_qat_act_fwd_f32(engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot), engine._ptr(qd[shift_q:]),
                                        engine._ptr(bt), _st()) == 0, L.yk_last_error()
            got = qd.cpu().numpy()
            want = qat_ref.fq(x, lo, hi)
            assert _bits(got[shift_q:shift_q + n]).tobytes() == _bits(want).tobytes(), (n, shift, shift_q, slot)
            assert (got[:shift_q] == 7.0).all() and (got[shift_q + n:] == 7.0).all()                   # nothing outside [0, n) is written
            blo, bhi, bfl = _read_batch(bt, len(RANGES))
            e = qat_ref.extremes(x)                                                                    # of the UNQUANTISED values
            assert _bits(blo[slot:slot + 1])[0] == _bits(e[0])[0] and _bits(bhi[slot:slot + 1])[0] == _bits(e[1])[0], (blo[slot], bhi[slot], e)
            others = [k for k in range(len(RANGES)) if k != slot]
            assert np.isposinf(blo[others]).all() and np.isneginf(bhi[others]).all() and not bfl.any()
            # backward: dy = dyq where 0 <= u <= 255, else +0.0, out of place and in place
            gd = _cu(np.concatenate([np.zeros(shift, np.float32), g]))
            dd = torch.full((shift_q + n + 3,), 7.0, dtype=torch.float32, device='cuda')
            assert L.yk_qat_act_bwd_f32(engine._ptr(gd[shift:]), engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot),
                                        engine._ptr(dd[shift_q:]), _st()) == 0, L.yk_last_error()
            wantg = np.where(qat_ref.ste_mask(x, lo, hi), g, np.float32(0.0)).astype(np.float32)
            gotg = dd.cpu().numpy()
            assert _bits(gotg[shift_q:shift_q + n]).tobytes() == _bits(wantg).tobytes(), (n, shift, shift_q, slot)
            assert (gotg[:shift_q] == 7.0).all() and (gotg[shift_q + n:] == 7.0).all()
            assert L.yk_qat_act_bwd_f32(engine._ptr(gd[shift:]), engine._ptr(xd[shift:]), C.c_longlong(n), engine._ptr(rt), C.c_int(slot),
                                        engine._ptr(gd[shift:]), _st()) == 0
            assert _bits(gd.cpu().numpy()[shift:]).tobytes() == _bits(wantg).tobytes()
            assert xd.cpu().numpy()[shift:shift + n].tobytes() == x.tobytes()                          # y is only read


def test_activation_forward_flags_non_finite_values_and_keeps_them_out_of_the_extremes():
    L = engine.lib()
    rng = np.random.default_rng(5)
    lo, hi = RANGES[0]
    x = _values(lo, hi, 4099, rng)
    x[17], x[4001] = np.nan, np.inf
    rt, bt = _range_table(), _batch_table(len(RANGES))
    xd, qd = _cu(x), torch.empty(4099, device='cuda')
    assert L.yk_qat_act_fwd_f32(engine._ptr(xd), C.c_longlong(4099), engine._ptr(rt), C.c_int(0), engine._ptr(qd), engine._ptr(bt), _st()) == 0
    got, want = qd.cpu().numpy(), qat_ref.fq(x, lo, hi)
    fin = np.isfinite(x)
    assert _bits(got[fin]).tobytes() == _bits(want[fin]).tobytes()
    assert np.isnan(got[17]) and got[4001] == want[4001] == qat_ref.fq(np.float32(1e30), lo, hi)     # +inf clamps to the top code
    blo, bhi, bfl = _read_batch(bt, len(RANGES))
    e = qat_ref.extremes(x)
    assert bfl[0] == 1 and not bfl[1:].any() and blo[0] == e[0] and bhi[0] == e[1] and np.isfinite([blo[0], bhi[0]]).all()
    gd = _cu(np.ones(4099, np.float32))
    assert L.yk_qat_act_bwd_f32(engine._ptr(gd), engine._ptr(xd), C.c_longlong(4099), engine._ptr(rt), C.c_int(0), engine._ptr(gd), _st()) == 0
    g = gd.cpu().numpy()
    assert g[17] == 0 and g[4001] == 0 and np.array_equal(g != 0, qat_ref.ste_mask(x, lo, hi))
    # bad arguments are refused
    assert L.yk_qat_act_fwd_f32(engine._ptr(xd), C.c_longlong(0), engine._ptr(rt), C.c_int(0), engine._ptr(qd), engine._ptr(bt), _st()) == -10
    assert L.yk_qat_act_fwd_f32(engine._ptr(xd), C.c_longlong(4), engine._ptr(rt), C.c_int(-1), engine._ptr(qd), engine._ptr(bt), _st()) == -10
    assert L.yk_qat_act_fwd_f32(engine._ptr(xd), C.c_longlong(4), engine._ptr(rt), C.c_int(0), engine._ptr(xd), engine._ptr(bt), _st()) == -10
    assert L.yk_qat_act_bwd_f32(None, engine._ptr(xd), C.c_longlong(4), engine._ptr(rt), C.c_int(0), engine._ptr(gd), _st()) == -10
    assert L.yk_qat_update_f32(engine._ptr(rt), engine._ptr(bt), None, None, None, C.c_int(4), C.c_float(0.9), C.c_float(0.1), 0, _st()) == -10
    assert L.yk_qat_weights_f32(engine._ptr(xd), C.c_longlong(4099), None, None, None, C.c_int(1), C.c_int(1), engine._ptr(qd), engine._ptr(bt),
                                _st()) == -10


SEG_SIZES = [1, 216, 4097, 65537]
SEG_KINDS = ['normal', 'equal', 'zero', 'half_zero']


def _segment(kind, n, rng):
    if kind == 'normal':
        return (rng.standard_normal(n) * 0.1).astype(np.float32)
    if kind == 'equal':
        return np.full(n, -0.37, np.float32)
    if kind == 'zero':
        return np.zeros(n, np.float32)
    w = (rng.standard_normal(n) * 0.1 + 0.02).astype(np.float32)             # half exactly zero: pruned weights
    w[rng.permutation(n)[:(n + 1) // 2]] = 0.0
    return w


@pytest.mark.parametrize('shift_q', [0, 1])
def test_weights_of_all_segments_in_one_call_equal_the_restatement_bitwise(shift_q):
    """16 segments (1, 216, 4097, 65537 elements x four kinds of content) at odd offsets with gaps, in ONE call.  shift_q 1: Pq one float off
    P's position inside 16 bytes, so no 16-byte access is possible."""
    L = engine.lib()
    rng = np.random.default_rng(11)
    TILE = L.yk_qat_tile()
    segs, offs, o = [], [], 5
    for i, (kind, n) in enumerate((k, n) for k in SEG_KINDS for n in SEG_SIZES):
        offs.append(o)
        segs.append(_segment(kind, n, rng))
        o += n + (3, 8, 1, 13)[i % 4]
    total = o + 9
    flat = (rng.standard_normal(total) * 100).astype(np.float32)             # gaps: biases, gamma, beta of the real buffer
    flat[3] = -0.0
    for off, sg in zip(offs, segs):
        flat[off:off + len(sg)] = sg
    sizes = [len(sg) for sg in segs]
    first = np.concatenate([[0], np.cumsum([(n + TILE - 1) // TILE for n in sizes])]).astype(np.int32)
    p = _cu(flat)
    pq = torch.full((total + shift_q + 2,), 7.0, dtype=torch.float32, device='cuda')
    wr = torch.zeros(4 * len(segs), dtype=torch.int32, device='cuda')
    offd, sized, firstd = _cu(np.asarray(offs, np.int64)), _cu(np.asarray(sizes, np.int64)), _cu(first)      # (alive until the call has run)
    assert all(0 <= o and o + n <= total for o, n in zip(offs, sizes))
    rc = L.yk_qat_weights_f32(engine._ptr(p), C.c_longlong(total), engine._ptr(offd), engine._ptr(sized), engine._ptr(firstd), C.c_int(len(segs)),
                              C.c_int(int(first[-1])), engine._ptr(pq[shift_q:]), engine._ptr(wr), _st())
    assert rc == 0, L.yk_last_error()
    got = pq.cpu().numpy()
    assert (got[:shift_q] == 7.0).all() and (got[shift_q + total:] == 7.0).all()
    got = got[shift_q:shift_q + total]
    assert p.cpu().numpy().tobytes() == flat.tobytes()                                                # P is only read
    outside = np.ones(total, bool)
    wlo, whi, wfl = _read_batch(wr, len(segs))
    for i, (off, sg) in enumerate(zip(offs, segs)):
        want = qat_ref.fq_weights(sg)
        assert _bits(got[off:off + len(sg)]).tobytes() == _bits(want).tobytes(), (i, len(sg))
        e = qat_ref.extremes(sg)
        assert (wlo[i], whi[i], wfl[i]) == (e[0], e[1], 0)
        s, zp = qat_ref.qparams32(*e)
        z = sg == 0
        assert not _bits(got[off:off + len(sg)][z]).any()                                             # an exact zero stays +0.0, bit for bit,
        assert (qat_ref.codes(sg[z], *e) == zp).all()                                                 # and is the code zp
        u = qat_ref.codes(sg, *e)
        assert u.min() >= 0 and u.max() <= 255                                                        # no weight is ever clamped
        outside[off:off + len(sg)] = False
    assert _bits(got[outside]).tobytes() == _bits(flat[outside]).tobytes()                            # everything else is copied unchanged


def test_range_update_moving_average_observe_union_and_untouched_slot():
    L = engine.lib()
    rng = np.random.default_rng(2)
    kind = [SLOT_NONE, SLOT_OWNER, SLOT_OWNER, SLOT_UNION, SLOT_OWNER, SLOT_UNION, SLOT_OWNER]
    p0, p1 = [0, 0, 0, 1, 0, 3, 0], [0, 0, 0, 2, 0, 4, 0]                    # slot 5: a union of a union and an owner
    n = len(kind)
    data = {0: rng.standard_normal(50), 1: rng.standard_normal(777) * 3, 2: rng.standard_normal(5) - 4, 6: np.array([np.nan, np.inf])}   # 4: untouched
    r0 = np.array([[9, 9], [-1.5, 2.25], [-6.0, 0.5], [0, 0], [-0.25, 8.0], [0, 0], [-3.0, 3.0]], np.float32)
    kd, p0d, p1d = _cu(np.asarray(kind, np.int32)), _cu(np.asarray(p0, np.int32)), _cu(np.asarray(p1, np.int32))

    def run(r_init, m, observe):
        rt, bt = _cu(r_init.reshape(-1).copy()), _batch_table(n)
        for slot, v in data.items():
            vd = _cu(np.asarray(v, np.float32))
            assert L.yk_range_f32(engine._ptr(vd), C.c_longlong(vd.numel()), engine._ptr(bt), C.c_int(slot), _st()) == 0
        m32 = np.float32(m)
        assert L.yk_qat_update_f32(engine._ptr(rt), engine._ptr(bt), engine._ptr(kd), engine._ptr(p0d), engine._ptr(p1d), C.c_int(n), C.c_float(m32),
                                   C.c_float(np.float32(1) - m32), C.c_int(observe), _st()) == 0, L.yk_last_error()
        blo, bhi, bfl = _read_batch(bt, n)
        assert np.isposinf(blo).all() and np.isneginf(bhi).all()                                      # the batch extremes start again
        assert bfl.tolist() == [0, 0, 0, 0, 0, 0, 1]                                                  # the flag is sticky
        want = r_init.copy()
        for i in range(n):
            if kind[i] == SLOT_OWNER:
                want[i] = qat_ref.update(r_init[i], qat_ref.extremes(np.asarray(data[i], np.float32)) if i in data else None, m, bool(observe))
        for i in range(n):
            if kind[i] == SLOT_UNION:
                want[i] = min(want[p0[i]][0], want[p1[i]][0]), max(want[p0[i]][1], want[p1[i]][1])
        got = rt.cpu().numpy().reshape(-1, 2)
        assert _bits(got).tobytes() == _bits(want).tobytes(), (got, want)
        return got

    got = run(r0, 0.9, 0)
    assert got[0].tolist() == [9, 9] and got[4].tolist() == [-0.25, 8.0] and got[6].tolist() == [-3.0, 3.0]     # no slot, untouched, nothing finite
    assert (got[1] != r0[1]).all()
    run(r0, 1.0, 0)
    run(r0, 0.9, 1)
    empty = np.tile(np.array([np.inf, -np.inf], np.float32), (n, 1))
    got = run(empty, 0.9, 1)                                                                          # observe from "nothing seen yet"
    assert np.isfinite(got[[1, 2, 3]]).all() and np.isposinf(got[4, 0]) and np.isneginf(got[4, 1]) and got[5].tolist() == got[3].tolist()   # min / max with 'nothing'


# ---------------------------------------------------------------------------------------------------------------------------- wiring
def _trainer(spec, w, h, B=2, **kw):
    from k210_yolo_framework_amd.train import Trainer
    return Trainer(spec, w, h.anchors, B, lr=1e-3, decay=0.0, **HYPER, **kw)


def _fixed_ranges(tr, x):
    """Ranges from one qat_observe, written back through qat_set_ranges."""
    tr.qat_observe(_cu(x))
    r = tr.qat_ranges()
    tr.qat_set_ranges(r)
    assert tr.qat_ranges() == r
    return r


def _tape(tr, spec):
    """{tensor name: (unquantised y, quantised tensor)} of the last forward pass, numpy NHWC."""
    names = quantize.tensor_names(spec)
    return {names[op['out']]: (tr.saved[i]['qy'].cpu().numpy(), tr.T[op['out']].cpu().numpy())
            for i, op in enumerate(spec.ops) if 'qy' in tr.saved.get(i, ())}


def test_every_quantised_tensor_lies_on_its_grid_and_the_exported_kernels_are_the_restatement():
    spec, w, h, x, yt = qat_ref.mini_case(5)
    tr = _trainer(spec, w, h, qat=QatConfig(momentum=1.0), use_graph=False)
    ranges = _fixed_ranges(tr, x)
    assert set(ranges) == {l.name for l in spec.layers} | {'concat_1'}
    up, back = ranges['head_conv_3'], ranges['conv_pw_1']                     # the concat of mini_spec: [upsample(head_conv_3), conv_pw_1]
    assert ranges['concat_1'] == (min(up[0], back[0]), max(up[1], back[1]))
    tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
    tape = _tape(tr, spec)
    assert set(tape) == set(ranges)
    for name, (y, yq) in tape.items():
        lo, hi = ranges[name]
        assert _bits(yq).tobytes() == _bits(qat_ref.fq(y, lo, hi)).tobytes(), name                    # the hook is the kernel, on this range
        assert _bits(qat_ref.fq(yq, lo, hi)).tobytes() == _bits(yq).tobytes(), name                   # on the grid (the concat: the union grid)
    assert tr.T[0].cpu().numpy().tobytes() == x.tobytes()                                            # the input frame is not quantised
    lat, qk = tr.export_weights(), tr.export_weights(quantized=True)
    for k in lat:
        want = qat_ref.fq_weights(lat[k]) if k.endswith('/kernel') else lat[k]
        assert _bits(qk[k]).tobytes() == _bits(want).tobytes(), k
    assert np.array_equal(tr.export_weights()['conv1/kernel'], w['conv1/kernel'])                    # P itself is not touched


def test_qat_loss_and_all_gradients_vs_float64_autograd_driven_by_the_gpu_codes():
    """Loss and every gradient against tests/qat_ref.loss_and_grads_qat in float64, test_gpu_train.py's tolerances (loss 1e-4, gradients 2e-3
    of the tensor's maximum).  The reference takes the GPU's code where its own differs - under qat_ref.check_driven's two conditions
    (fewer than 1 % of a tensor, each within 255e-4 steps of a tie; held for every seed of qat_ref.WIRING_SEEDS on the CPU by tests/test_qat_ref.py)"""
    compared = 0
    for seed in qat_ref.WIRING_SEEDS:
        spec, w, h, x, yt = qat_ref.mini_case(seed)
        tr = _trainer(spec, w, h, qat=QatConfig(momentum=1.0), use_graph=False)
        ranges = _fixed_ranges(tr, x)
        r = tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
        torch.cuda.synchronize()
        drive = {name: qat_ref.codes(y, *ranges[name]) for name, (y, _) in _tape(tr, spec).items()}
        record = {}
        ref_data, ref_reg, ref_g, stats = qat_ref.loss_and_grads_qat(spec, w, x, yt, h.anchors, ranges, drive=drive, record=record, **HYPER)
        print('seed', seed, 'driven codes per tensor:', {k: (v['diff'], round(v['tie_dist'], 6)) for k, v in record.items() if v['diff']})
        qat_ref.check_driven(record)
        data = float(sum(p[0] for p in r['layers']).cpu())
        print('seed', seed, 'loss', data, ref_data)
        assert abs(data - ref_data) <= 1e-4 * abs(ref_data), (data, ref_data)
        assert abs(float(r['reg'].cpu()) - ref_reg) <= 1e-5 * abs(ref_reg)
        if _gate_flips(tr, spec, stats):                                       # an activation kink evaluated on two sides: sub-gradients differ
            continue
        got = tr.grads()
        gmax = max(np.abs(v).max() for v in ref_g.values())
        for k, rg in ref_g.items():
            if np.abs(rg).max() < 1e-9 * gmax:
                assert np.abs(got[k]).max() <= 1e-6 * gmax, k
                continue
            print('   ', k, np.abs(got[k] - rg).max() / np.abs(rg).max())
            _close(got[k], rg, 2e-3)
        compared += 1
        if compared == 2:
            break
    assert compared >= 1, 'no flip-free seed found'


def test_replayed_qat_step_equals_the_eager_step_bitwise_and_the_ranges_follow_the_batch_extremes():
    spec, w, h, x, yt = qat_ref.mini_case(6)
    names = quantize.tensor_names(spec)
    runs = []
    for graph in (False, True):
        tr = _trainer(spec, w, h, qat=QatConfig(momentum=0.9), use_graph=graph)
        r = {k: tuple(np.float32(v) for v in lohi) for k, lohi in _fixed_ranges(tr, x).items()}
        for _ in range(3):                                                     # step 1 eager, step 2 captured + replayed, step 3 replayed
            tr.step(_cu(x), [_cu(y) for y in yt])
            torch.cuda.synchronize()
            for i, op in enumerate(spec.ops):                                  # the restatement on this step's own batch extremes
                if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
                    nm = names[op['out']]
                    r[nm] = qat_ref.update(r[nm], qat_ref.extremes(tr.saved[i]['qy'].cpu().numpy()), 0.9, False)
            r['concat_1'] = (min(r['head_conv_3'][0], r['conv_pw_1'][0]), max(r['head_conv_3'][1], r['conv_pw_1'][1]))
            got = tr.qat_ranges()
            for k in r:
                assert _bits(np.array(got[k], np.float32)).tobytes() == _bits(np.array(r[k], np.float32)).tobytes(), (graph, k, got[k], r[k])
        runs.append((tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy(), tr.Pq.cpu().numpy().copy(), tr._qa_ranges.cpu().numpy().copy()))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_qat_off_means_off_and_on_changes_the_step():
    spec, w, h, x, yt = qat_ref.mini_case(7)
    state = []
    for q in (None, None, QatConfig(momentum=0.99)):
        tr = _trainer(spec, w, h, qat=q)
        if q is not None:
            _fixed_ranges(tr, x)
            tr.load_weights(w)                                                 # (the observing pass moved the BatchNorm moving statistics)
        else:
            assert not hasattr(tr, 'Pq') and not hasattr(tr, '_qa_ranges')     # nothing is allocated
            with pytest.raises(engine.YkError, match='qat=None'):
                tr.qat_ranges()
        for _ in range(2):
            tr.step(_cu(x), [_cu(y) for y in yt])
        state.append([t.cpu().numpy().copy() for t in (tr.P, tr.m, tr.v)])
    for a, b in zip(state[0], state[1]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(state[0], state[2]):
        assert not np.array_equal(a, b)
    tr = _trainer(spec, w, h, qat=QatConfig())
    with pytest.raises(engine.YkError, match='qat_observe'):                   # no ranges yet: refused, not quantised on an empty range
        tr.step(_cu(x), [_cu(y) for y in yt])
    from k210_yolo_framework_amd.train import Trainer
    v2 = ns.yolo_mobilev2((64, 96, 3), 3, 20, alpha=0.5)
    with pytest.raises(kmodel.KmodelError, match='`add`'):
        Trainer(v2, v2.init_weights(1), h.anchors, 2, qat=QatConfig())


def test_pruning_and_qat_compose_masked_weights_are_exactly_zero_in_pq():
    from k210_yolo_framework_amd.prune import PruneSchedule
    spec, w, h, x, yt = qat_ref.mini_case(8)
    tr = _trainer(spec, w, h, qat=QatConfig(momentum=0.99), prune=PruneSchedule(0.5, 0.5, 10, 1))
    _fixed_ranges(tr, x)
    for _ in range(2):
        tr.step(_cu(x), [_cu(y) for y in yt])
    masks = tr.prune_masks()
    pq = {}                                                                # Pq as the LAST step read it, Keras layout
    for l in spec.layers:
        kh, kw, ci, co = l.kernel_shape
        k = tr.view(tr.Pq, l.name + '/kernel').cpu().numpy()
        pq[l.name + '/kernel'] = np.transpose(k.reshape(co, kh, kw, ci), (1, 2, 3, 0)) if l.kind == 'conv' else k.reshape(3, 3, ci)[..., None]
    assert masks
    for nm, m in masks.items():
        assert 0.45 <= 1.0 - m.mean() <= 0.55, nm
        assert not _bits(pq[nm][~m]).any(), nm                                 # +0.0 bit for bit: real zero is the code zp
        assert (pq[nm][m] != 0).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------------- round trip
def test_make_train_qat_cli_round_trip_to_a_kmodel_the_kpu_runner_loads(tmp_path):
    from k210_yolo_framework_amd import make_kmodel, training
    from k210_yolo_framework_amd.kmodel import YOLO_MOBILEV1_ORDER
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--image_size', '64', '96', '--output_size', '2', '3', '4', '6']
    tr = training.cli(['--synthetic', '32', '--batch_size', '4', '--max_steps', '6', '--qat', 'True', '--qat_observe', '2', '--max_nrof_epochs', '3',
                       '--vaildation_split', '0.0', '--log_dir', str(tmp_path), '--obj_weight', '1', '--noobj_weight', '1', '--wh_weight', '1', *net])
    assert tr.iterations == 6
    (ck,) = list(tmp_path.glob('*/yolo_qat_model.npz'))
    assert (ck.parent / 'yolo_qat_model.h5').exists() and (ck.parent / 'yolo_qat_ranges.npz').exists()
    with np.load(ck.parent / 'yolo_qat_ranges.npz') as z:
        assert {k: tuple(float(v) for v in z[k]) for k in z.files} == tr.qat_ranges()
    out = tmp_path / 'qat.kmodel'
    make_kmodel.cli([str(ck), str(out), *net, '--ranges', str(ck.parent / 'yolo_qat_ranges.npz')])
    km = kmodel.parse(out.read_bytes())
    plan = engine.KpuPlan(kmodel.pack_kpu(km), max_batch=2)
    plan.run_u8(torch.from_numpy(quantize.synthetic_frames(2, (64, 96), 1)).cuda())
    torch.cuda.synchronize()
    outs = [o[:2].cpu().numpy() for o in plan.outputs()]
    assert [o.shape for o in outs] == [(2, 2, 3, 75), (2, 4, 6, 75)] and all(np.isfinite(o).all() for o in outs)
    plan.close()
    # the written codes are the codes the step trained on: centred code (q - zp) of every weight, float64 quantiser against the fp32 kernels
    spec = tr.spec
    lat, qk = tr.export_weights(), tr.export_weights(quantized=True)
    with np.load(ck) as z:
        for k in lat:
            assert np.array_equal(z[k], lat[k]), k                             # the checkpoint holds the latent weights
    fw, _ = kmodel.to_float_weights(km, spec)
    plain = [n for n in YOLO_MOBILEV1_ORDER if n not in ('conv1', 'head_conv_4', 'head_conv_2', 'head_conv_5')]     # to_float_weights folds gains into these
    assert len(km.convs) == len(YOLO_MOBILEV1_ORDER)
    for name, c in zip(YOLO_MOBILEV1_ORDER, km.convs):
        k = lat[name + '/kernel']
        s, zp = qat_ref.qparams32(*qat_ref.extremes(k))
        mine = np.rint(qk[name + '/kernel'] / s)                               # exact: Pq = s * (q - zp)
        assert np.array_equal((mine * s).astype(np.float32), qk[name + '/kernel'])
        wq = c.weights.astype(np.float64) - c.zp_w
        theirs = wq.reshape(c.out_ch, 3, 3).transpose(1, 2, 0)[..., None] if c.depthwise else wq.reshape(c.out_ch, c.in_ch, c.ksize, c.ksize).transpose(2, 3, 1, 0)
        if name in plain:
            assert np.array_equal(fw[name + '/kernel'], theirs.astype(np.float32)), name
        d = np.abs(mine - theirs)
        print(name, 'codes differing', int((d != 0).sum()), 'of', d.size, 'max', d.max())
        assert d.max() <= 1 and (d != 0).sum() <= 1e-3 * d.size, (name, d.max(), int((d != 0).sum()), d.size)


def test_non_finite_flags_are_named_sticky_clearable_and_momentum_changes_reach_a_captured_step():
    spec, w, h, x, yt = qat_ref.mini_case(9)
    tr = _trainer(spec, w, h, qat=QatConfig(momentum=0.9))
    ranges = _fixed_ranges(tr, x)
    yd = [_cu(y) for y in yt]
    for _ in range(3):                                                         # eager, captured, replayed
        tr.step(_cu(x), yd)
    moved = tr.qat_ranges()
    assert moved != ranges and tr.qat_flagged() == []
    tr.qat.momentum = 1.0                                                      # a launch scalar of the capture: the step is captured again
    tr.step(_cu(x), yd)
    tr.step(_cu(x), yd)
    assert tr.qat_ranges() == moved
    bad = x.copy()
    bad[0, 3, 4, 1] = np.inf
    tr.step(_cu(bad), yd)
    flagged = tr.qat_flagged()
    assert 'conv1' in flagged and all(not f.endswith('/kernel') for f in flagged)
    with pytest.raises(engine.YkError, match='conv1'):
        tr.qat_ranges()
    assert tr.qat_ranges(check=False)['conv_pw_2'] == moved['conv_pw_2']       # a batch without a finite value keeps the range
    tr.load_weights(w)
    tr.qat_clear_flags()
    assert tr.qat_flagged() == [] and tr.qat_ranges(check=False) == tr.qat_ranges()
    wn = dict(w)
    wn['conv_pw_1/kernel'] = w['conv_pw_1/kernel'].copy()
    wn['conv_pw_1/kernel'][0, 0, 1, 2] = np.nan
    tr.load_weights(wn)
    tr.export_weights(quantized=True)                                          # Pq from the current P
    assert tr.qat_flagged() == ['conv_pw_1/kernel']
