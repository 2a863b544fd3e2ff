"""The walk of qerror.analyze on the GPU: yolo_mobilev1-0.5 at 32 x 32 with 8 generated frames (the network and frames
tests/test_gpu_yolo_biascorrect.py uses; its own copy here), every row against the numpy rule applied on the host to the tensors the walk kept.

The bound is tests/test_gpu_qerr.py's: n 2^-53 sum|term| per float64 sum, the worst case of reordering it; counts and the largest |e| exact."""
import json

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, qerror, quantize

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SUMS = ('syy', 'see', 'se', 'syh', 'shh')
EXACT = ('n', 'n0', 'n255', 'emax')
CUT = 'conv_pw_5'                                          # mid-network: 10 convs upstream, 22 downstream
DEFERRED = ('conv_dw_2', 'conv_dw_4', 'conv_dw_6', 'conv_dw_12')       # stride-2 depthwise convs whose 1x1 reader pools
CONCAT_READER = 'head_conv_4'                              # reads concat(upsample(head_conv_3), conv_pw_11)


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def small_yolo():
    from k210_yolo_framework_amd import yolonet
    model, _ = yolonet.yolo_mobilev1([32, 32, 3], 3, 20, alpha=0.5)
    model.set_weights(model.spec.init_weights(seed=3))
    frames = quantize.synthetic_frames(8, (32, 32), seed=4)
    ranges = quantize.calibrate(model.spec, model.get_weights(), frames, 8)
    return model, frames, ranges


def _host_rows(rows, keep):
    """{layer: {'acc' | 'local': (sums, bounds)}} of the numpy rule on the kept tensors, batch by batch."""
    out = {}
    for name, r in rows.items():
        out[name] = {}
        for key, kept in (('acc', 'float'), ('local', 'local')):
            total, bound = None, None
            for y, q in zip(keep[name][kept], keep[name]['codes']):
                y, q = y.cpu().numpy(), q.cpu().numpy()
                s = qerror.channel_sums(y, q, r['s_y'], r['zp_y'], r['step'])
                yd, yh = y.astype(np.float64), qerror.dequantise(q[:, ::r['step'], ::r['step']], r['s_y'], r['zp_y'])
                mag = {k: np.abs(v).sum(axis=(0, 1, 2)) for k, v in dict(syy=yd * yd, see=(yd - yh) ** 2, se=yd - yh, syh=yd * yh, shh=yh * yh).items()}
                total = s if total is None else qerror.add_sums(total, s)
                bound = mag if bound is None else {k: bound[k] + mag[k] for k in mag}
            out[name][key] = (total, {k: total['n'] * U * v for k, v in bound.items()})
    return out


@pytest.fixture(scope='module')
def analysed(small_yolo):
    """The walk once with the measured ranges (two batches: 5 + 3 frames) and once with CUT's upper end cut to an eighth, each with what it kept."""
    model, frames, ranges = small_yolo
    spec, w = model.spec, model.get_weights()
    cut = dict(ranges)
    cut[CUT] = (ranges[CUT][0], ranges[CUT][1] / 8.0)
    assert ranges[CUT][1] > 0.0
    out = []
    for rg in (ranges, cut):
        km, rep = quantize.quantize(spec, w, rg)
        keep = {}
        out.append((qerror.analyze(spec, w, km, rep, frames, batch=5, keep=keep), keep, rep))
    return out


def test_every_row_equals_the_numpy_rule_on_the_kept_tensors(small_yolo, analysed):
    model = small_yolo[0]
    result, keep, rep = analysed[0]
    rows = result['layers']
    assert list(rows) == [l.name for l in model.spec.layers] and result['images'] == 8
    assert all(rows[n]['index'] == rep['layers'][n]['index'] for n in rows)
    assert all(rows[n]['step'] == (2 if n in DEFERRED else 1) for n in rows) and CONCAT_READER in rows
    assert all(len(keep[n]['codes']) == 2 for n in rows)                               # 5 + 3 frames
    host = _host_rows(rows, keep)
    worst = 0.0
    for name, r in rows.items():
        for key in ('acc', 'local'):
            got, (want, bound) = r[key]['sums'], host[name][key]
            for k in EXACT:
                assert np.array_equal(got[k], want[k]), (name, key, k)
            assert not got['flag'].any()
            for k in SUMS:
                err = np.abs(got[k] - want[k])
                worst = max(worst, float((err / np.maximum(bound[k], 1e-300)).max()))
                assert (err <= bound[k]).all(), (name, key, k, err, bound[k])
            f = qerror.figures(want, r['s_y'])
            assert r[key]['n'] == f['n'] and r[key]['share_255'] == f['share_255'] and r[key]['max_err'] == f['max_err']
    print(f'largest |gpu - numpy| / bound over all rows: {worst:.3g}')
    # the local tensor of a conv is the float conv of what the KPU handed it, not the float network's tensor: they differ past the first conv
    assert not np.array_equal(keep[CONCAT_READER]['local'][0].cpu().numpy(), keep[CONCAT_READER]['float'][0].cpu().numpy())
    text = qerror.format_report(result)
    assert text.count('\n') == len(rows) + 2 and "charged to the concat's reader" in text


def test_the_first_conv_local_row_is_its_accumulated_row_bit_for_bit(analysed):
    r = analysed[0][0]['layers']['conv1']
    for k in SUMS + EXACT:
        assert r['acc']['sums'][k].tobytes() == r['local']['sums'][k].tobytes(), k
    assert r['acc']['sqnr_db'] == r['local']['sqnr_db']


def test_a_cut_range_is_found_where_it_was_made(small_yolo, analysed):
    (before, _, _), (after, keep, rep) = analysed
    names = list(before['layers'])
    at = names.index(CUT)
    assert 5 <= at < len(names) - 5
    for name in names[:at]:                                                            # upstream: nothing changed, bit for bit
        for key in ('acc', 'local'):
            for k in SUMS + EXACT:
                assert before['layers'][name][key]['sums'][k].tobytes() == after['layers'][name][key]['sums'][k].tobytes(), (name, key, k)
    b, a = before['layers'][CUT], after['layers'][CUT]
    codes = np.concatenate([q.cpu().numpy() for q in keep[CUT]['codes']])
    assert a['acc']['share_255'] == float((codes == 255).sum()) / codes.size == a['local']['share_255']
    print(f"{CUT}: share at 255 {b['acc']['share_255']:.4f} -> {a['acc']['share_255']:.4f}, local SQNR {b['local']['sqnr_db']:.2f} -> "
          f"{a['local']['sqnr_db']:.2f} dB")
    assert a['acc']['share_255'] > b['acc']['share_255']
    assert a['local']['sqnr_db'] < b['local']['sqnr_db']


def test_save_kmodel_analyze_writes_the_same_bytes_and_off_prints_what_it_printed(small_yolo, tmp_path):
    model, frames, _ = small_yolo
    off, on, held = (str(tmp_path / n) for n in ('off.kmodel', 'on.kmodel', 'held.kmodel'))
    rep_off = model.save_kmodel(off, frames, batch=8)
    rep_on = model.save_kmodel(on, frames, batch=8, analyze=True, analyze_top=2)
    assert open(on, 'rb').read() == open(off, 'rb').read()
    want, _ = quantize.quantize(model.spec, model.get_weights(), quantize.calibrate(model.spec, model.get_weights(), frames, 8))
    assert open(off, 'rb').read() == kmodel.serialise(want)
    assert 'qerror' not in rep_off and not (tmp_path / 'off.kmodel.qerror.json').exists()
    text_off, text_on = quantize.format_report(rep_off), quantize.format_report(rep_on)
    assert 'quantisation error' not in text_off and text_off.endswith(f"KPU RAM peak {rep_off['kpu_ram_peak']} bytes")
    assert text_on == text_off + '\n' + qerror.format_report(rep_on['qerror'])          # the present lines first, unchanged
    doc = json.loads((tmp_path / 'on.kmodel.qerror.json').read_text())
    assert list(doc['layers']) == [l.name for l in model.spec.layers] and doc['images'] == 8
    assert all(len(r['acc']['worst']) <= 2 and len(r['acc']['channel_sqnr_db']) > 0 for r in doc['layers'].values())
    # held-out frames: the same file, other figures
    rep_held = model.save_kmodel(held, frames, batch=8, analyze=True, analyze_frames=quantize.synthetic_frames(4, (32, 32), seed=11))
    assert open(held, 'rb').read() == open(off, 'rb').read() and rep_held['qerror']['images'] == 4
    assert rep_held['qerror']['layers']['conv1']['acc']['sums']['see'].tobytes() != rep_on['qerror']['layers']['conv1']['acc']['sums']['see'].tobytes()


def test_cli_refuses_analyze_with_ranges(tmp_path, capsys):
    from k210_yolo_framework_amd import make_kmodel
    with pytest.raises(SystemExit):
        make_kmodel.cli(['ckpt.h5', str(tmp_path / 'o.kmodel'), '--analyze', 'True', '--ranges', 'x.npz'])
    err = capsys.readouterr().err
    assert '--analyze' in err and '--ranges' in err and 'later work' in err
    assert not (tmp_path / 'o.kmodel').exists()
