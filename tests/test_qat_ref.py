"""CPU checks of quantisation-aware training: the float32 restatement tests/qat_ref.py against its own definition and
against quantize.qparams, the `--ranges` flag of make_kmodel, the refusal of networks the KPU path cannot express, and the pre-check
that the seeded inputs of tests/test_gpu_qat.py keep a float32 forward pass inside the conditions under which a float64 pass may be driven
by its codes."""
import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import netspec as ns, quantize
from k210_yolo_framework_amd.kmodel import KmodelError
from tests import qat_ref

RANGES = [(-1.0, 3.0), (0.5, 2.0), (-2.0, -0.5), (0.0, 0.0), (-1e-3, 1e-3), (-7.3, 0.0), (0.0, 6.0)]


def _values(lo, hi, rng):
    s, zp = qat_ref.qparams32(lo, hi)
    grid = (np.arange(-20, 280, dtype=np.float32) - zp) * s
    ties = ((np.arange(-3, 259, dtype=np.float32) + np.float32(0.5)) - zp) * s
    return np.concatenate([grid, ties, rng.uniform(min(lo, 0) * 2 - 1, max(hi, 0) * 2 + 1, 4000).astype(np.float32),
                           np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)])


@pytest.mark.parametrize('lo,hi', RANGES)
def test_fq_is_idempotent_keeps_zero_and_takes_at_most_256_values(lo, hi):
    x = _values(lo, hi, np.random.default_rng(1))
    y = qat_ref.fq(x, lo, hi)
    assert qat_ref.fq(y, lo, hi).tobytes() == y.tobytes()
    assert len(np.unique(y)) <= 256
    z = qat_ref.fq(np.array([0.0, -0.0], np.float32), lo, hi)
    assert z.tobytes() == np.zeros(2, np.float32).tobytes()                # +0.0, bit for bit
    s, zp = qat_ref.qparams32(lo, hi)
    assert zp == np.rint(zp) and 0 <= zp <= 255
    assert qat_ref.codes(np.zeros(1, np.float32), lo, hi)[0] == zp          # real zero is the code zp
    # the straight-through mask is 1 exactly where nothing was clamped
    u = qat_ref.codes(x, lo, hi)
    assert np.array_equal(qat_ref.ste_mask(x, lo, hi), (u >= 0) & (u <= 255))


def test_float32_rule_equals_quantize_qparams_on_a_seeded_sweep():
    rng = np.random.default_rng(7)
    n_zp = 0
    for k in range(10000):
        kind = k % 4
        a, b = np.sort(rng.standard_normal(2) * 10.0 ** rng.uniform(-4, 3))
        if kind == 1:
            a, b = abs(a), abs(a) + abs(b)                                 # lo > 0
        elif kind == 2:
            a, b = -abs(a) - abs(b), -abs(a)                               # hi < 0
        lo, hi = np.float32(a), np.float32(b)
        s32, zp32 = qat_ref.qparams32(lo, hi)
        s64, zp64 = quantize.qparams(float(lo), float(hi))
        assert abs(float(s32) - s64) <= 2.0 ** -23 * s64, (lo, hi)          # up to float32 rounding of s (difference and quotient)
        t = -min(float(lo), 0.0) / s64
        if abs(t - np.floor(t) - 0.5) > 1e-3:
            assert int(zp32) == zp64, (lo, hi, zp32, zp64)
            n_zp += 1
    assert n_zp > 9900
    assert qat_ref.qparams32(0, 0) == (np.float32(quantize.INPUT_SCALE), 0) and quantize.qparams(0, 0) == (quantize.INPUT_SCALE, 0)


def test_update_rules():
    r = (np.float32(-1.5), np.float32(2.25))
    b = (np.float32(-0.7), np.float32(3.1))
    assert qat_ref.update(r, None, 0.9, False) == r and qat_ref.update(r, None, 0.9, True) == r
    assert qat_ref.update(r, b, 1.0, False) == r
    assert qat_ref.update(r, b, 0.9, True) == (np.float32(-1.5), np.float32(3.1))
    assert qat_ref.update((np.float32(np.inf), np.float32(-np.inf)), b, 0.9, True) == b          # nothing seen yet
    lo, hi = qat_ref.update(r, b, 0.9, False)
    assert lo == np.float32(np.float32(0.9) * r[0]) + np.float32((np.float32(1) - np.float32(0.9)) * b[0]) and r[1] < hi < b[1]


def test_qat_refuses_networks_the_kpu_path_cannot_express():
    """Trainer(qat=...) builds its slot table through quantize.plan_convs: the user sees the quantiser's own KmodelError naming the op."""
    from k210_yolo_framework_amd import qat
    with pytest.raises(KmodelError, match='`add`'):
        qat.slot_table(ns.yolo_mobilev2((64, 96, 3), 3, 20, alpha=0.5))
    with pytest.raises(KmodelError, match='`maxpool`'):
        qat.slot_table(ns.tiny_yolo((64, 96, 3), 3, 20))
    spec = ns.yolo_mobilev1((64, 96, 3), 3, 20, alpha=0.5)
    kind, p0, p1 = qat.slot_table(spec)
    names = quantize.tensor_names(spec)
    assert [names[i] for i, k in enumerate(kind) if k == qat.SLOT_OWNER] == [l.name for l in spec.layers]
    (cat,) = [i for i, k in enumerate(kind) if k == qat.SLOT_UNION]
    assert names[cat] == 'concat_1' and {names[p0[cat]], names[p1[cat]]} == {'head_conv_3', 'conv_pw_11'}      # through the upsample
    assert kind[0] == qat.SLOT_NONE
    with pytest.raises(Exception, match='momentum'):
        qat.QatConfig(1.5)


def test_make_kmodel_ranges_flag(tmp_path, capsys):
    from k210_yolo_framework_amd import engine, kmodel, make_kmodel
    spec = ns.yolo_mobilev1((64, 96, 3), 3, 20, alpha=0.5)
    w = spec.init_weights(3)
    ck, out = tmp_path / 'w.npz', tmp_path / 'm.kmodel'
    np.savez(ck, **w)
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--image_size', '64', '96', '--output_size', '2', '3', '4', '6']
    rng = np.random.default_rng(0)
    relu = {op['layer'] for op in spec.ops if op.get('layer') and op['act'] == ns.ACT_RELU}          # a ReLU output never goes below zero
    ranges = {l.name: np.array([0.0 if l.name in relu else -rng.uniform(0.5, 1), rng.uniform(2, 6)], np.float32) for l in spec.layers}
    ranges['concat_1'] = np.array([-2, 6], np.float32)
    np.savez(tmp_path / 'r.npz', **ranges)
    for extra in (['--synthetic', '4'], ['--calib', 'x.npy']):                                       # replaces calibration: exclusive
        with pytest.raises(SystemExit):
            make_kmodel.cli([str(ck), str(out), *net, '--ranges', str(tmp_path / 'r.npz'), *extra])
        assert 'cannot be combined' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        make_kmodel.cli([str(ck), str(out), *net])
    rep = make_kmodel.cli([str(ck), str(out), *net, '--ranges', str(tmp_path / 'r.npz')])            # CPU only: nothing is calibrated
    km = kmodel.parse(out.read_bytes())
    assert len(km.convs) == len(spec.layers) and rep['file_bytes'] == out.stat().st_size
    for name, r in rep['layers'].items():
        assert r['range'] == tuple(float(v) for v in ranges[name])
    # the written codes against the float32 restatement of the step's kernels (what test_gpu_qat.py holds the GPU's Pq to): centred code
    # (q - zp) of every weight, float64 quantiser against float32 rule - they can part only where the two scales round a tie differently
    fw, _ = kmodel.to_float_weights(km, spec)
    folded = ('conv1', 'head_conv_4', 'head_conv_2', 'head_conv_5')                                  # to_float_weights folds gains into these kernels
    for name, c in zip(kmodel.YOLO_MOBILEV1_ORDER, km.convs):
        k = w[name + '/kernel']
        s32, _ = qat_ref.qparams32(*qat_ref.extremes(k))
        mine = np.rint(qat_ref.fq_weights(k) / s32)
        wq = c.weights.astype(np.float64) - c.zp_w
        theirs = wq.reshape(c.out_ch, 3, 3).transpose(1, 2, 0)[..., None] if c.depthwise else wq.reshape(c.out_ch, c.in_ch, c.ksize, c.ksize).transpose(2, 3, 1, 0)
        if name not in folded:
            assert np.array_equal(fw[name + '/kernel'], theirs.astype(np.float32)), name
        d = np.abs(mine - theirs)
        assert d.max() <= 1 and (d != 0).sum() <= 1e-3 * d.size, (name, d.max(), int((d != 0).sum()), d.size)
    lacking = {k: v for k, v in ranges.items() if k not in ('conv_dw_3', 'head_conv_5')}
    np.savez(tmp_path / 'r2.npz', **lacking)
    with pytest.raises(engine.YkError, match=r'conv_dw_3, head_conv_5'):
        make_kmodel.cli([str(ck), str(out), *net, '--ranges', str(tmp_path / 'r2.npz')])


@pytest.mark.parametrize('seed', qat_ref.WIRING_SEEDS)
def test_seeded_wiring_inputs_keep_a_float32_forward_inside_the_driving_conditions(seed):
    """tests/test_gpu_qat.py drives the float64 pass by the GPU's codes.  Beforehand, without a GPU, for every seed it may use: the
    float32-numpy forward (qat_ref.forward_np32) of the same inputs, over the ranges its own unquantised pass observes, differs from the
    float64 pass in fewer than 1 % of any tensor's codes, each of them within 255e-4 steps of a rounding tie."""
    spec, w, h, x, yt = qat_ref.mini_case(seed)
    observed = qat_ref.forward_np32(spec, w, x, None)
    assert set(observed) == {l.name for l in spec.layers} | {'concat_1'}
    rec32 = qat_ref.forward_np32(spec, w, x, observed)
    assert set(rec32) == set(observed)
    drive = {k: r['u'] for k, r in rec32.items()}
    p64 = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in w.items()}
    rec64 = {}
    qat_ref.forward_train_qat(spec, p64, torch.from_numpy(x).double(), observed, drive=drive, record=rec64)
    qat_ref.check_driven(rec64)
    for name, r in rec32.items():
        lo, hi = observed[name]
        assert np.abs(r['y'] - rec64[name]['y']).max() <= 1e-4 * np.abs(rec64[name]['y']).max(), name     # the two forwards are one network
        yq = qat_ref.fq(r['y'], lo, hi)
        assert qat_ref.fq(yq, lo, hi).tobytes() == yq.tobytes()                                           # every quantised tensor on its grid


def test_map_eval_takes_a_kmodel_with_precision_kpu_and_only_then(capsys):
    from tools import map_eval
    for argv in (['w.h5', '--precision', 'kpu'], ['m.kmodel'], ['m.kfpkg', '--precision', 'f16']):
        with pytest.raises(SystemExit):
            map_eval.main(argv)
        assert '--precision kpu runs a .kmodel' in capsys.readouterr().err


def test_make_train_qat_needs_at_least_one_observed_batch():
    """--qat_observe 0 is refused before anything is built or written; without a HIP device --qat True is refused by its name."""
    from k210_yolo_framework_amd import engine, training
    if not torch.cuda.is_available():
        with pytest.raises(engine.YkError, match='--qat True'):
            training.cli(['--synthetic', '8', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '4', '--qat', 'True',
                          '--log_dir', '/nonexistent/never-written'])
    with pytest.raises(engine.YkError, match='--qat_observe 0'):
        training.cli(['--synthetic', '8', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '4', '--qat', 'True',
                      '--qat_observe', '0', '--log_dir', '/nonexistent/never-written'])
