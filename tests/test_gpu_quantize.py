"""Calibration kernels (csrc/yk_calib.hip), quantize.Calibrator, and the quantised file on the KPU-exact GPU path.  fp32 tolerance: the
1e-4 of the tensor's magnitude that tests/test_gpu_train.py holds the fp32 forward kernels to."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, netspec as ns, quantize
from oracle import decode_ref, kpu_ref, torch_net_ref

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / 'golden'
FP32_TOL = 1e-4                                            # tests/test_gpu_train.py: kernels 1e-4 relative to the tensor's max magnitude


def _keys(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.uint32(k)
    b = (k ^ np.uint32(0x80000000)) if k & np.uint32(0x80000000) else ~k
    return np.array([b], np.uint32).view(np.float32)[0]


def np_min_max(a):
    """numpy's min / max, with the one thing IEEE comparison leaves open pinned: -0 orders below +0 (np.min may return either zero)."""
    a = np.asarray(a, np.float32).ravel()
    lo, hi = _unkey(_keys(a).min()), _unkey(_keys(a).max())
    assert lo == a.min() and hi == a.max()
    if a.min() != 0:
        assert lo.tobytes() == a.min().tobytes()
    if a.max() != 0:
        assert hi.tobytes() == a.max().tobytes()
    return lo, hi


class Slots:
    def __init__(self, n=4):
        import torch
        from k210_yolo_framework_amd import engine
        engine.require_gpu()
        self.torch, self.engine, self.L, self.n = torch, engine, engine.lib(), n
        self.d = torch.zeros(4 * n, dtype=torch.int32, device='cuda')
        self.reset()

    def _s(self, stream=None):
        return C.c_void_p((stream or self.torch.cuda.current_stream()).cuda_stream)

    def reset(self):
        assert self.L.yk_range_reset(self.engine._ptr(self.d), self.n, self._s()) == 0

    def fold(self, x, slot, stream=None):
        assert self.L.yk_range_f32(self.engine._ptr(x), C.c_longlong(x.numel()), self.engine._ptr(self.d), slot, self._s(stream)) == 0

    def read(self):
        lo, hi, fl = np.empty(self.n, np.float32), np.empty(self.n, np.float32), np.empty(self.n, np.int32)
        self.torch.cuda.synchronize()
        assert self.L.yk_range_read(self.engine._ptr(self.d), self.n, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                    fl.ctypes.data_as(C.c_void_p)) == 0
        return lo, hi, fl


@pytest.mark.parametrize('n', [1, 2, 3, 5, 63, 64, 65, 255, 1025, 65537, 3_000_001])
def test_range_kernel_equals_numpy_bitwise(n):
    import torch
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    S = Slots()
    S.fold(torch.from_numpy(a).cuda(), 1)
    if n > 8:                                              # a view that is not 16-byte aligned takes the scalar path
        S.fold(torch.from_numpy(a).cuda()[1:], 2)
    lo, hi, fl = S.read()
    want = np_min_max(a)
    assert (lo[1].tobytes(), hi[1].tobytes(), fl[1]) == (want[0].tobytes(), want[1].tobytes(), 0)
    if n > 8:
        w2 = np_min_max(a[1:])
        assert (lo[2].tobytes(), hi[2].tobytes()) == (w2[0].tobytes(), w2[1].tobytes())
    assert lo[0] == np.inf and hi[0] == -np.inf and fl[0] == 0     # an untouched slot


def test_signed_zeros_denormals_accumulation_and_streams():
    import torch
    S = Slots(6)
    z = np.array([0.0, -0.0, 0.0], np.float32)
    S.fold(torch.from_numpy(z).cuda(), 0)
    den = np.array([1e-45, -3e-42, 2e-39, -1e-40], np.float32)                   # all subnormal
    assert (den != 0).all() and (np.abs(den) < np.finfo(np.float32).tiny).all()
    S.fold(torch.from_numpy(den).cuda(), 1)
    rng = np.random.default_rng(0)
    parts = [rng.standard_normal(k).astype(np.float32) * s for k, s in ((1000, 1.0), (7, 50.0), (300001, 0.1))]
    for p_ in parts:
        S.fold(torch.from_numpy(p_).cuda(), 2)                                   # accumulates over calls
    whole = np.concatenate(parts)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    xd = torch.from_numpy(whole).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        S.fold(xd, 3, s1)
    with torch.cuda.stream(s2):
        S.fold(xd, 4, s2)
    lo, hi, fl = S.read()
    assert np.signbit(lo[0]) and lo[0] == 0 and not np.signbit(hi[0]) and hi[0] == 0
    w = np_min_max(den)
    assert (lo[1].tobytes(), hi[1].tobytes()) == (w[0].tobytes(), w[1].tobytes()) and lo[1] != 0 and hi[1] != 0
    w = np_min_max(whole)
    for s in (2, 3, 4):
        assert (lo[s].tobytes(), hi[s].tobytes()) == (w[0].tobytes(), w[1].tobytes()), s
    assert not fl.any()
    S.reset()
    lo, hi, fl = S.read()
    assert (lo == np.inf).all() and (hi == -np.inf).all()


@pytest.mark.parametrize('M,Cn,act,alpha', [(1, 1, 0, 0.0), (7, 3, 3, 0.3), (1000, 75, 0, 0.0), (4097, 24, 1, 0.0), (35840, 48, 3, 0.1),
                                            (3, 1024, 2, 6.0), (600_000, 5, 3, 0.3)])
def test_scale_act_range_kernel(M, Cn, act, alpha):
    import torch
    from k210_yolo_framework_amd import engine
    rng = np.random.default_rng(M + Cn)
    z = rng.standard_normal((M, Cn)).astype(np.float32) * 3
    sc = rng.uniform(0.2, 2.0, Cn).astype(np.float32) * rng.choice([-1, 1], Cn).astype(np.float32)
    bi = rng.standard_normal(Cn).astype(np.float32)
    S = Slots()
    zd, sd, bd = (torch.from_numpy(v).cuda() for v in (z, sc, bi))
    yd = torch.empty_like(zd)
    assert S.L.yk_scale_act_range_f32(engine._ptr(zd), C.c_longlong(M), Cn, engine._ptr(sd), engine._ptr(bd), act, C.c_float(alpha), engine._ptr(yd),
                                      engine._ptr(S.d), 3, S._s()) == 0
    lo, hi, fl = S.read()
    y = yd.cpu().numpy()
    v = z * sc + bi                                        # fp32, one rounding per operation
    a32 = np.float32(alpha)
    want = {0: v, 1: np.where(v > 0, v, np.float32(0)), 2: np.clip(v, 0, 6), 3: np.where(v >= 0, v, v * a32)}[act].astype(np.float32)
    err = float(np.abs(y.astype(np.float64) - want).max())
    print('max |y - numpy|', err)
    assert err <= FP32_TOL * max(1e-6, float(np.abs(want).max()))
    w = np_min_max(y)                                      # the range is that of the y it stored, bit for bit
    assert (lo[3].tobytes(), hi[3].tobytes(), fl[3]) == (w[0].tobytes(), w[1].tobytes(), 0)


MINI = None


def _mini():
    from tests.test_quantize import small_spec
    spec = small_spec()
    return spec, spec.init_weights(seed=7)


@pytest.mark.parametrize('poison', [np.nan, np.inf, -np.inf])
def test_a_planted_nan_or_inf_sets_the_flag_and_raises_through_the_calibrator(poison):
    import torch
    from k210_yolo_framework_amd import engine
    S = Slots()
    a = np.random.default_rng(1).standard_normal(100_000).astype(np.float32)
    a[77_777] = poison
    S.fold(torch.from_numpy(a).cuda(), 0)
    S.fold(torch.from_numpy(a[:1000]).cuda(), 0)           # sticky
    lo, hi, fl = S.read()
    fin = a[np.isfinite(a)]
    assert fl[0] == 1 and lo[0] == fin.min() and hi[0] == fin.max()         # the non-finite value did not enter the range
    spec, w = _mini()
    w['conv_pw_2_bn/beta'] = w['conv_pw_2_bn/beta'].copy()
    w['conv_pw_2_bn/beta'][3] = poison
    cal = quantize.Calibrator(spec, w, max_batch=2)
    cal.feed(torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)).cuda())
    with pytest.raises(engine.YkError, match='conv_pw_2'):
        cal.ranges()


def _oracle_ranges(spec, w, fr):
    import torch
    x = fr.astype(np.float32) * np.float32(quantize.INPUT_SCALE)
    names = quantize.tensor_names(spec)
    out = {'input': (float(x.min()), float(x.max()))}
    for s in range(0, len(fr), 8):
        t = torch_net_ref.forward(spec, w, x[s:s + 8], want=list(range(1, len(spec.tensors))), dtype=torch.float64)
        for i, v in t.items():
            lo, hi = out.get(names[i], (np.inf, -np.inf))
            out[names[i]] = (min(lo, float(v.min())), max(hi, float(v.max())))
    return out


@pytest.fixture(scope='module')
def demo():
    return kmodel.parse((GOLD / 'yolo.kmodel').read_bytes())


@pytest.fixture(scope='module')
def flagship(demo):
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    W, _ = kmodel.to_float_weights(demo)
    return spec, W


def test_calibrator_ranges_agree_with_the_fp32_oracle_on_the_flagship(flagship):
    import torch
    spec, W = flagship
    fr = quantize.synthetic_frames(16, spec.in_hw, seed=21)
    cal = quantize.Calibrator(spec, W, max_batch=8)
    cal.feed(torch.from_numpy(fr[:8]).cuda()).feed(torch.from_numpy(fr[8:13]).cuda()).feed(torch.from_numpy(fr[13:]).cuda())
    got = cal.ranges()
    want = _oracle_ranges(spec, W, fr)
    assert sorted(got) == sorted(want) and len(got) == len(spec.tensors)
    for name in quantize.tensor_names(spec):
        (glo, ghi), (wlo, whi) = got[name], want[name]
        tol = FP32_TOL * max(whi - wlo, 1e-6)
        print(f'{name:<12} gpu ({glo:.6g}, {ghi:.6g})  oracle ({wlo:.6g}, {whi:.6g})  tol {tol:.3g}')
        assert abs(glo - wlo) <= tol and abs(ghi - whi) <= tol, name
    # upsample / concat take their producers' ranges by construction
    assert got['upsample_1'] == got['head_conv_3']
    assert got['concat_1'] == (min(got['upsample_1'][0], got['conv_pw_11'][0]), max(got['upsample_1'][1], got['conv_pw_11'][1]))
    one = quantize.Calibrator(spec, W, max_batch=16).feed(torch.from_numpy(fr).cuda()).ranges()      # how the set is split does not matter...
    assert one['input'] == got['input']                    # ...bitwise for the reduction itself (the GEMMs tile by batch size)
    for name in got:
        assert abs(one[name][0] - got[name][0]) + abs(one[name][1] - got[name][1]) <= 2 * FP32_TOL * (want[name][1] - want[name][0] + 1e-6), name


@pytest.fixture(scope='module')
def requantised(flagship, tmp_path_factory):
    """W = the demo's own float weights, calibrated on 256 generated images (seed A = 101) and quantised."""
    import torch
    spec, W = flagship
    cal = quantize.Calibrator(spec, W, max_batch=32)
    fr = quantize.synthetic_frames(256, spec.in_hw, seed=101)
    for s in range(0, 256, 32):
        cal.feed(torch.from_numpy(fr[s:s + 32]).cuda())
    km, rep = quantize.quantize(spec, W, cal.ranges())
    path = tmp_path_factory.mktemp('q') / 'requantised.kmodel'
    kmodel.write(path, km)
    return kmodel.parse(path.read_bytes()), rep, path


def test_written_file_is_bit_identical_on_the_gpu_to_the_oracle(requantised):
    import torch
    from k210_yolo_framework_amd import engine
    km, rep, _ = requantised
    img = np.load(GOLD / 'kmodel_dog_golden.npz')['image']
    keep = {}
    ref = kpu_ref.run(km, img, keep)
    with engine.KpuPlan(km, max_batch=1) as plan:
        plan.run_u8(torch.from_numpy(np.ascontiguousarray(img[None])).cuda(), layout='chw')
        torch.cuda.synchronize()
        assert len(keep) == 32
        for index, want in keep.items():
            assert plan.read_layer(index, 0).tobytes() == want.tobytes(), index
        for o, want in zip(plan.outputs(), ref):
            assert o[0].cpu().numpy().transpose(2, 0, 1).tobytes() == np.ascontiguousarray(want).tobytes()


def _run_kpu(km, frames_nhwc):
    import torch
    from k210_yolo_framework_amd import engine
    outs = []
    with engine.KpuPlan(km, max_batch=len(frames_nhwc)) as plan:
        plan.run_u8(torch.from_numpy(np.ascontiguousarray(frames_nhwc)).cuda())
        torch.cuda.synchronize()
        outs = [o[:len(frames_nhwc)].cpu().numpy().astype(np.float64) for o in plan.outputs()]
    return outs


def _run_float(spec, W, frames_nhwc):
    import torch
    from k210_yolo_framework_amd import engine
    plan = engine.Plan(spec, W, max_batch=len(frames_nhwc))
    assert plan.precision == 'f16x2'
    plan.run_u8(torch.from_numpy(np.ascontiguousarray(frames_nhwc)).cuda())
    torch.cuda.synchronize()
    outs = [o[:len(frames_nhwc)].cpu().numpy().astype(np.float64) for o in plan.outputs()]
    plan.close()
    return outs


def _dog_nhwc():
    return np.ascontiguousarray(np.load(GOLD / 'kmodel_dog_golden.npz')['image'].transpose(1, 2, 0))


def test_accuracy_against_the_references_own_quantisation(flagship, demo, requantised):
    """e = RMS(KPU(file) - F) / RMS(F) over both outputs, F = the float network (f16x2) on W; evaluation on 64 generated images (seed B = 202)
    + the dog picture.  Pass: e_new <= 1.5 e_ref, e_ref measured here from the reference's file.
    Both figures are printed; not yet measured on an MI355X (profiles/quantize_demo_error.txt say so)."""
    spec, W = flagship
    km, rep, _ = requantised
    ev = np.concatenate([quantize.synthetic_frames(64, spec.in_hw, seed=202), _dog_nhwc()[None]])
    assert (ev.reshape(len(ev), -1).max(1) == 255).all()   # float (img / max) and KPU (img / 255) inputs coincide
    F = _run_float(spec, W, ev)
    den = np.sqrt(sum((f ** 2).sum() for f in F))
    e_ref = np.sqrt(sum(((a - f) ** 2).sum() for a, f in zip(_run_kpu(demo, ev), F))) / den
    e_new = np.sqrt(sum(((a - f) ** 2).sum() for a, f in zip(_run_kpu(km, ev), F))) / den
    print(f'e_ref {e_ref:.6f}  e_new {e_new:.6f}  ratio {e_new / e_ref:.4f}')
    assert e_new <= 1.5 * e_ref, (e_new, e_ref)


def _scores(outs, b=0):
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))              # noqa: E731
    res = []
    for o in outs:
        p = o[b].reshape(o.shape[1], o.shape[2], 3, 25)
        res.append((sig(p[..., 5:]) * sig(p[..., 4:5])).reshape(-1, 20))
    return np.concatenate(res)


def _iou(a, b):
    t, l, bo, r = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    inter = max(0.0, bo - t) * max(0.0, r - l)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def test_detections_on_the_dog_picture_at_main_c_thresholds(flagship, demo, requantised):
    """main.c: threshold 0.5, nms 0.3.  delta = the largest score difference between KPU(demo) and F on the picture: every F detection
    scoring >= 0.5 + delta must appear in KPU(new) (same class, IoU >= 0.5), and no class whose best F score is <= 0.5 - delta may."""
    spec, W = flagship
    km, rep, _ = requantised
    dog = _dog_nhwc()[None]
    from k210_yolo_framework_amd.helper import VOC_ANCHORS as anchors
    F, D, N = _run_float(spec, W, dog), _run_kpu(demo, dog), _run_kpu(km, dog)
    sF, sD, sN = _scores(F), _scores(D), _scores(N)
    delta = float(np.abs(sD - sF).max())
    thr = 0.5
    dec = lambda outs: decode_ref.decode_batch([o.astype(np.float32).reshape(1, o.shape[1], o.shape[2], 3, 25) for o in outs], anchors,   # noqa: E731
                                               (224, 320), (224, 320), thr, 0.3)[0][0]
    dF, dN = dec(F), dec(N)
    print(f'delta {delta:.4f}; F detections {dF[:, 4:].tolist()}; KPU(new) detections {dN[:, 4:].tolist()}; max |score new - F| {np.abs(sN - sF).max():.4f}')
    for row in dF:
        if row[4] >= thr + delta:
            assert any(n[5] == row[5] and _iou(n[:4], row[:4]) >= 0.5 for n in dN), row
    best = sF.max(0)
    for n in dN:
        assert best[int(n[5])] > thr - delta, n


def test_save_kmodel_then_kpu_predict_equals_loading_the_written_file(flagship, tmp_path):
    from k210_yolo_framework_amd import engine, yolonet
    spec, W = flagship
    model, _ = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.75)
    model.set_weights(W)
    fr = quantize.synthetic_frames(24, spec.in_hw, seed=5)
    rep = model.save_kmodel(str(tmp_path / 'a.kfpkg'), fr, batch=16)
    assert rep['file_bytes'] > 3_000_000 and 'conv_pw_13' in rep['layers']
    model.precision = 'kpu'
    x = np.concatenate([fr[:2], _dog_nhwc()[None]])
    got = model.predict(x)
    fresh, _ = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.75, precision='kpu')
    fresh.load_weights(str(tmp_path / 'a.kfpkg'))
    for a, b in zip(got, fresh.predict(x)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    model.precision = 'f16x2'                              # the float weights are still there beside it
    assert all(np.isfinite(o).all() for o in model.predict(x))
    for build in (yolonet.yolo_mobilev2, yolonet.tiny_yolo):
        m, _ = build([224, 320, 3], 3, 20, alpha=1.0)
        with pytest.raises(engine.YkError, match='`add`|`maxpool`'):
            m.save_kmodel(str(tmp_path / 'no.kmodel'), fr[:2])
    assert not (tmp_path / 'no.kmodel').exists()


@pytest.mark.parametrize('prune', [False, True])
def test_cli_train_then_make_kmodel_then_kpu_inference(prune, tmp_path, capsys, monkeypatch):
    from k210_yolo_framework_amd import inference, make_kmodel, training
    root = Path(__file__).resolve().parent.parent
    monkeypatch.chdir(root)
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5']
    common = ['--synthetic', '32', '--batch_size', '4', '--max_nrof_epochs', '1', '--vaildation_split', '0.125', '--obj_weight', '1',
              '--noobj_weight', '1', '--wh_weight', '1', '--iou_thresh', '0.5', '--log_dir', str(tmp_path / 'log')] + net
    extra = ['--is_prune', 'True', '--prune_end_epoch', '1', '--prune_frequency', '2'] if prune else ['--is_prune', 'False']
    tr = training.cli(common + extra)
    capsys.readouterr()
    ck = list((tmp_path / 'log').glob('*/yolo_prune_model.h5' if prune else '*/yolo_model.h5'))
    assert len(ck) == 1
    out = tmp_path / 'trained.kmodel'
    rep = make_kmodel.cli([str(ck[0]), str(out), '--synthetic', '16', '--calib_seed', '9'] + net)
    text = capsys.readouterr().out
    assert out.exists() and f'kmodel of {out.stat().st_size} bytes' in text and 'conv_pw_13' in text and 'w==zp' in text
    if prune:
        for name, r in tr.prune_report().items():
            sparsity = 1.0 - r['kept'] / r['n']
            layer = name[:-len('/kernel')]
            print(layer, 'trained sparsity', sparsity, 'w == zp share', rep['layers'][layer]['zero_share'])
            assert rep['layers'][layer]['zero_share'] >= sparsity - 1e-12, layer
    import shutil
    shutil.copy(root / 'data' / 'synthetic_320x224.jpg', tmp_path / 'picture.jpg')          # the CLI saves its drawing beside the picture
    dets = inference.cli([str(out), str(tmp_path / 'picture.jpg'), '--precision', 'kpu', '--obj_thresh', '0.0', '--iou_thresh', '0.5'] + net)
    text = capsys.readouterr().out
    assert '[top\tleft\tbottom\tright\tscore\tclass]' in text and len(dets) > 0
