"""Bias correction end to end on the GPU: Calibrator.feed_means + KpuPlan.run_stats_u8 + biascorrect.correct, on the mini network of
tests/biascorrect_cases.py and through save_kmodel(bias_correct=True) on yolo_mobilev1-0.5 at 32 x 32 with 8 generated frames.

The file's name puts it behind tests/test_gpu_shared_weights.py in a run of the whole suite: that file compares differences of the device's free
memory that are a few 2 MiB blocks wide, and the hundred small plans made and closed here (one per conv and pass), run before it, leave the driver's
small-allocation heap packed differently - four shared plans then cost 10 MiB instead of 8 there, one block past its bound."""
import numpy as np
import pytest

from k210_yolo_framework_amd import biascorrect, kmodel, quantize
from tests import biascorrect_cases as bc

pytestmark = pytest.mark.gpu
BOUND = 0.5 + 1e-6                                         # half a unit of z (2^-p output steps) + the float64 slack of the comparison


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _worst(res, brep=None):
    out = {}
    for name, v in res.items():
        keep = np.setdiff1d(np.arange(len(v)), brep['layers'][name]['limited'] if brep else [])
        out[name] = float(v[keep].max())
    return out


def test_mini_network_gpu_statistics_equal_numpy_and_the_correction_meets_the_bound():
    import torch
    spec, w, fr, fm_np, ranges = bc.mini_case()
    km, rep = quantize.quantize(spec, w, ranges)
    measure = biascorrect.gpu_measure(np.array(fr), batch=2)                       # 3 frames in batches of 2 and 1
    got, want = measure(km), bc.numpy_measure(fr)(km)
    assert set(got) == set(want)
    for i in want:
        assert got[i][1] == want[i][1] and np.array_equal(got[i][0], want[i][0]), i      # integers: exactly
    fm = quantize.calibrate_means(spec, w, np.array(fr), batch=2)
    for name, (s, n) in fm_np.items():
        gs, gn = fm[name]
        # fp32 kernels against numpy float64: the 1e-4 of the tensor's magnitude tests/test_gpu_train.py holds the forward kernels to, per
        # element, so n times that on a sum
        assert gn == n and np.abs(gs - s).max() <= 1e-4 * n * max(1.0, float(np.abs(s).max()) / n), name
    before = _worst(biascorrect.residuals(rep, fm, got))
    assert max(before.values()) > 0.5
    delta, brep = biascorrect.correct(spec, w, ranges, fm, measure)
    km2, rep2 = quantize.quantize(spec, w, ranges, delta)
    after = _worst(biascorrect.residuals(rep2, fm, measure(km2)), brep)
    print('before', before, '\nafter', after)
    assert {'conv_dw_2', 'conv_dw_4'} <= set(after) and max(after.values()) <= BOUND
    assert sum(len(r['limited']) for r in brep['layers'].values()) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def small_yolo():
    from k210_yolo_framework_amd import yolonet
    model, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5)
    model.set_weights(model.spec.init_weights(seed=3))
    frames = quantize.synthetic_frames(8, (32, 32), seed=4)
    return model, frames


def test_save_kmodel_bias_correct_meets_the_bound_and_off_is_unchanged(small_yolo, tmp_path):
    from k210_yolo_framework_amd import yolonet
    model, frames = small_yolo
    spec, w = model.spec, model.get_weights()
    off, on, dflt = (str(tmp_path / n) for n in ('off.kmodel', 'on.kmodel', 'default.kmodel'))
    rep_off = model.save_kmodel(off, frames, batch=8, bias_correct=False)
    model.save_kmodel(dflt, frames, batch=8)
    rep_on = model.save_kmodel(on, frames, batch=8, bias_correct=True)
    # off: the bytes of the unchanged functions - calibrate, quantize without a delta, serialise
    want, _ = quantize.quantize(spec, w, quantize.calibrate(spec, w, frames, 8))
    assert open(off, 'rb').read() == kmodel.serialise(want) == open(dflt, 'rb').read()
    assert 'biascorrect' not in rep_off and 'bias-corrected' not in quantize.format_report(rep_off)
    assert open(on, 'rb').read() != open(off, 'rb').read()
    fm = quantize.calibrate_means(spec, w, frames, 8)
    measure = biascorrect.gpu_measure(frames, 8)
    brep = rep_on['biascorrect']
    res_on = biascorrect.residuals(rep_on, fm, measure(kmodel.parse(open(on, 'rb').read())))
    res_off = biascorrect.residuals(rep_off, fm, measure(kmodel.parse(open(off, 'rb').read())))
    w_on, w_off = _worst(res_on, brep), _worst(res_off)
    print('off', w_off, '\non', w_on, '\nlimited', {n: r['limited'] for n, r in brep['layers'].items() if r['limited']})
    assert set(res_on) == {l.name for l in spec.layers}
    assert max(w_off.values()) > 0.5                       # without the correction the bound is violated
    assert max(w_on.values()) <= BOUND
    n_lim = sum(len(r['limited']) for r in brep['layers'].values())
    assert n_lim <= 2, brep                                # the limit is for broken channels: it must not hollow the check out
    text = quantize.format_report(rep_on)
    assert text.count('bias-corrected ') == len(spec.layers) and 'bias correction:' in text
    assert all(rep_on['layers'][n]['bias_limited'] == len(r['limited']) for n, r in brep['layers'].items())
    fresh, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5, precision='kpu')
    fresh.load_weights(on)
    outs = fresh.predict(frames[:2])
    assert len(outs) == 2 and all(np.isfinite(o).all() for o in outs)


def test_cli_refuses_bias_correct_with_ranges(tmp_path, capsys):
    from k210_yolo_framework_amd import make_kmodel
    with pytest.raises(SystemExit):
        make_kmodel.cli(['ckpt.h5', str(tmp_path / 'o.kmodel'), '--bias_correct', 'True', '--ranges', 'x.npz'])
    assert 'needs calibration frames' in capsys.readouterr().err
    assert not (tmp_path / 'o.kmodel').exists()
