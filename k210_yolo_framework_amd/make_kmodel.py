"""`make kmodel` - quantise a trained checkpoint to a K210 kmodel (the reference leaves this step to keras_freeze.py + nncase).

    python make_kmodel.py CKPT OUT [network flags of keras_inference.py] (--calib LIST.npy | --synthetic N | --ranges FILE.npz) [--calib_seed S]
                          [--calib_method minmax|percentile|mse] [--calib_percentile P] [--calib_bins NB]
                          [--equalize True [--equalize_max_gain G]]
                          [--bias_correct True]
                          [--adaround True [--adaround_iters N] [--adaround_lambda L] [--adaround_lr R]]
                          [--analyze True [--analyze_seed S] [--analyze_top K]]

CKPT: a Keras `.h5` or `.npz` checkpoint; OUT: `.kmodel` or `.kfpkg`.  The calibration images are a list file as make_voc_list.py writes
(data/<set>_img_ann.npy) or N generated images as `make train SYNTHETIC=N` trains on; they are decoded as the input pipeline decodes them
(Helper._read_img) and letterboxed on the GPU (yk_letterbox_u8), then measured by quantize.Calibrator.  Prints the per-layer report and
the file size.  `--ranges FILE` (`make kmodel RANGES=`) quantises with the ranges a `make train QAT=True` run learned
(`yolo_qat_ranges.npz`: tensor name -> [lo, hi]) instead of calibrating; no image is read and no GPU is needed.
`--calib_method` (`make kmodel CALIBMETHOD=`): `minmax`, the default, spreads the 256 codes over each tensor's exact range; `percentile`
(`--calib_percentile`, default 99.99) and `mse` clip the range from a histogram of `--calib_bins` bins per tensor, taken on the GPU in a second
pass over the same images (quantize.clip_range).  The report then lists every clipped tensor.
`--equalize True` (`make kmodel EQUALIZE=True EQMAXGAIN=64`): cross-layer range equalisation (equalize.py) before the calibration - one more
pass over the images measures every conv output per channel, the weights are rewritten so that the channels of a tensor fill its range
(gains up to `--equalize_max_gain`), and the file written is that network: the same function, other weights.  Not with `--ranges`: QAT
ranges belong to the unequalised weights.  The report names the gains of every layer.
`--bias_correct True` (`make kmodel BIASCORRECT=True`): per-channel bias correction (biascorrect.py) after the calibration, on the same images -
one more float pass and one KPU-exact statistics pass per conv layer find the integer to add to every channel's bn_add so that the kmodel's mean
pre-activation equals the float network's.  Not with `--ranges`: it needs calibration frames.  The report gets one line per corrected layer.
`--adaround True` (`make kmodel ADAROUND=True ADAITERS=1000 ADALAMBDA=0.01 ADALR=0.01`): adaptive weight rounding (adaround.py) after the
calibration and before the bias correction, on the same images - one more float pass builds every layer's input Gram matrix, then
`--adaround_iters` Adam steps per layer on the GPU choose the lower or upper code of every weight.  Not with `--ranges`: it needs calibration
frames.  The report gets one line per layer.
`--analyze True` (`make kmodel ANALYZE=True ANALYZESEED=S ANALYZETOP=3`): after the file is written, the finished kmodel is measured against the
float network conv by conv (qerror.py) - on the calibration images, or, with `--synthetic N --analyze_seed S`, on N generated images of seed S,
which the calibration has not seen.  One table row per conv, and the same data in OUT.qerror.json.  The kmodel's bytes do not change.  Not with
`--ranges`: no frames are read then (measuring a QAT kmodel on frames of its own is later work)."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import quantize
from .helper import INFO, Helper, VOC_ANCHORS
from .yolonet import MODEL_DEFS


def calibration_frames(h: Helper, calib, synthetic: int, seed: int, class_num: int, limit: int = 0):
    """Device uint8 [N, H, W, 3] at the network's input size."""
    import torch
    from . import engine
    from .training import synthetic_list
    in_hw = tuple(int(v) for v in h.in_hw[0])
    if synthetic:
        imgs = [it[0] for it in synthetic_list(int(synthetic), in_hw, class_num, seed)]
    else:
        rows = np.load(calib, allow_pickle=True)
        order = np.random.default_rng(seed).permutation(len(rows))
        if limit:
            order = order[:limit]
        imgs = [h._read_img(str(rows[i][0])) for i in order]
    if not imgs:
        raise engine.YkError('make_kmodel: no calibration images')
    return torch.cat([engine.letterbox_u8(torch.from_numpy(np.ascontiguousarray(im[None, ..., :3], np.uint8)).cuda(), in_hw) for im in imgs])


def load_ranges(path, spec):
    """{tensor name: (lo, hi)} of a `yolo_qat_ranges.npz`; YkError naming every conv output of `spec` the file lacks."""
    from . import engine
    with np.load(str(path)) as z:
        ranges = {k: tuple(float(v) for v in np.asarray(z[k]).reshape(-1)[:2]) for k in z.files}
    missing = [l.name for l in spec.layers if l.name not in ranges]
    if missing:
        raise engine.YkError(f'make_kmodel: --ranges {path} has no range for tensor(s) {", ".join(missing)} of {spec.name}')
    return ranges


def main(ckpt, out, image_size, output_size, model_def, class_num, depth_multiplier, train_set, calib, synthetic, calib_seed, batch, limit=0,
         ranges=None, method='minmax', percentile=99.99, bins=2048, equalize=False, max_gain=64.0, bias_correct=False,
         adaround=False, ada_iters=1000, ada_lambda=0.01, ada_lr=1e-2, analyze=False, analyze_seed=None, analyze_top=3):
    from pathlib import Path
    anchor_file = Path(f'data/{train_set}_anchor.npy')
    h = Helper(None, class_num, str(anchor_file) if anchor_file.exists() else VOC_ANCHORS, np.reshape(np.array(image_size), (-1, 2)),
               np.reshape(np.array(output_size), (-1, 2)))
    model, _ = MODEL_DEFS[model_def]([image_size[0], image_size[1], 3], len(h.anchors[0]), class_num, alpha=depth_multiplier)
    model.load_weights(str(ckpt))
    print(INFO, f' Load CKPT {ckpt}')
    t0 = time.time()
    if ranges:
        from . import engine, kmodel
        try:
            km, report = quantize.quantize(model.spec, model.get_weights(), load_ranges(ranges, model.spec))
            report['file_bytes'] = kmodel.write(str(out), km)
        except kmodel.KmodelError as e:
            raise engine.YkError(f'make_kmodel: {e}') from e
        print(quantize.format_report(report))
        print(INFO, f' ranges of {ranges}, no calibration, {time.time() - t0:.2f} s')
    else:
        frames = calibration_frames(h, calib, synthetic, calib_seed, class_num, limit)
        eq = dict(equalize=True, max_gain=max_gain) if equalize else {}
        if bias_correct:
            eq['bias_correct'] = True
        if adaround:
            eq.update(adaround=True, ada_iters=ada_iters, ada_lambda=ada_lambda, ada_lr=ada_lr)
        if analyze:
            held_out = synthetic and analyze_seed is not None and int(analyze_seed) != int(calib_seed)
            eq.update(analyze=True, analyze_top=analyze_top,
                      analyze_frames=calibration_frames(h, calib, synthetic, int(analyze_seed), class_num, limit) if held_out else None)
        report = model.save_kmodel(str(out), frames, batch=batch, method=method, percentile=percentile, bins=bins, **eq)
        print(quantize.format_report(report))
        print(INFO, f' {len(frames)} calibration images{"" if method == "minmax" else f", {method} ranges from {bins}-bin histograms"}'
                    f'{f", channel ranges equalised first (max gain {max_gain:g}, one more pass)" if equalize else ""}'
                    f'{f", weights rounded adaptively ({ada_iters} steps per layer)" if adaround else ""}'
                    f'{", channel biases corrected (one statistics pass per conv)" if bias_correct else ""}'
                    f'{f", quantisation error written to {out}.qerror.json" if analyze else ""}, {time.time() - t0:.2f} s')
    print(INFO, f' wrote {out}: kmodel of {report["file_bytes"]} bytes')
    return report


def _true_or_false(p, name, value) -> bool:
    if value not in (None, 'True', 'False'):
        p.error(f'--{name} {value}: True or False')
    return value == 'True'


def cli(argv=None):
    p = argparse.ArgumentParser(description='quantise a checkpoint to a K210 kmodel, calibrated on the GPU')
    p.add_argument('--train_set', type=str, help='trian file lists', default='voc')
    p.add_argument('--class_num', type=int, help='trian class num', default=20)
    p.add_argument('--model_def', type=str, help='Model definition.', default='yolo_mobilev1')
    p.add_argument('--depth_multiplier', type=float, help='mobilenet depth_multiplier', choices=[0.5, 0.75, 1.0], default=0.75)
    p.add_argument('--image_size', type=int, help='net work input image size', default=(224, 320), nargs='+')
    p.add_argument('--output_size', type=int, help='net work output image size', default=(7, 10, 14, 20), nargs='+')
    p.add_argument('--calib', type=str, default=None, help='calibration list file as make_voc_list.py writes (data/<set>_img_ann.npy)')
    p.add_argument('--calib_limit', type=int, default=0, help='use at most this many images of --calib (0 = all)')
    p.add_argument('--synthetic', type=int, default=0, help='calibrate on N generated images instead of --calib')
    p.add_argument('--calib_seed', type=int, default=3, help='seed of the generated images / of the order --calib_limit samples in')
    p.add_argument('--calib_batch', type=int, default=32, help='images per calibration forward pass')
    p.add_argument('--ranges', type=str, default=None, help='quantise with the ranges of a QAT run (yolo_qat_ranges.npz) instead of calibrating')
    p.add_argument('--calib_method', type=str, default=None, help='minmax (default): exact ranges; percentile | mse: ranges clipped from GPU '
                                                                  'histograms (a second pass over the images)')
    p.add_argument('--calib_percentile', type=float, default=99.99, help='share of the values --calib_method percentile keeps at each end, '
                                                                         'in (50, 100]')
    p.add_argument('--calib_bins', type=int, default=2048, help='histogram bins per tensor, 16..4096')
    p.add_argument('--equalize', type=str, default=None, help='True: equalise the channel ranges before quantising (equalize.py; one more pass '
                                                              'over the images); the file is the equalised network')
    p.add_argument('--equalize_max_gain', type=float, default=64.0, help='largest gain --equalize gives a channel, > 1')
    p.add_argument('--bias_correct', type=str, default=None, help='True: correct every channel\'s bn_add after the calibration so that its mean '
                                                                  'pre-activation equals the float network\'s (biascorrect.py); needs frames')
    p.add_argument('--adaround', type=str, default=None, help='True: round every kernel weight down or up so that each output channel\'s error '
                                                              'over the calibration frames falls (adaround.py); needs frames')
    p.add_argument('--adaround_iters', type=int, default=1000, help='Adam steps per layer of --adaround')
    p.add_argument('--adaround_lambda', type=float, default=0.01, help='weight of the rounding regulariser of --adaround')
    p.add_argument('--adaround_lr', type=float, default=1e-2, help='Adam step size of --adaround')
    p.add_argument('--analyze', type=str, default=None, help='True: measure the finished kmodel against the float network, conv by conv '
                                                             '(qerror.py); prints a table and writes OUT.qerror.json; needs frames')
    p.add_argument('--analyze_seed', type=int, default=None, help='with --synthetic N: measure on N generated images of this seed instead of the '
                                                                  'calibration images')
    p.add_argument('--analyze_top', type=int, default=3, help='worst channels --analyze names per conv')
    p.add_argument('pre_ckpt', type=str, help='trained weights (.h5 / .npz)')
    p.add_argument('output', type=str, help='.kmodel or .kfpkg to write')
    a = p.parse_args(sys.argv[1:] if argv is None else argv)
    if a.ranges and (a.calib or a.synthetic):
        p.error('--ranges replaces calibration: it cannot be combined with --calib or --synthetic')
    if a.ranges and a.calib_method is not None:
        p.error('--ranges replaces calibration: it cannot be combined with --calib_method')
    if not a.calib and not a.synthetic and not a.ranges:
        p.error('give --calib LIST.npy, --synthetic N or --ranges FILE.npz')
    on = {}
    for name, why in (('equalize', 'cannot be combined with --ranges: QAT ranges belong to the unequalised weights'),
                      ('bias_correct', 'needs calibration frames: it cannot be combined with --ranges (QAT ranges, no frames)'),
                      ('adaround', 'needs calibration frames: it cannot be combined with --ranges (QAT ranges, no frames)'),
                      ('analyze', 'cannot be combined with --ranges: no frames are read then, and it measures the kmodel on frames (measuring a QAT '
                                  'kmodel on frames of its own is later work)')):
        on[name] = _true_or_false(p, name, getattr(a, name))
        if a.ranges and on[name]:
            p.error(f'--{name} {why}')
    if on['equalize'] and not a.equalize_max_gain > 1.0:
        p.error(f'--equalize_max_gain {a.equalize_max_gain} must be above 1')
    if on['adaround'] and not (a.adaround_iters >= 0 and a.adaround_lambda >= 0.0 and a.adaround_lr > 0.0):
        p.error(f'--adaround_iters {a.adaround_iters} and --adaround_lambda {a.adaround_lambda} must not be negative, --adaround_lr '
                f'{a.adaround_lr} must be positive')
    if on['analyze'] and a.analyze_top < 0:
        p.error(f'--analyze_top {a.analyze_top} must not be negative')
    method = a.calib_method or 'minmax'
    try:
        quantize.check_method(method, a.calib_percentile, a.calib_bins)
    except quantize.KmodelError as e:
        p.error({'method': f'--calib_method {method}: one of {", ".join(quantize.CALIB_METHODS)}',
                 'percentile': f'--calib_percentile {a.calib_percentile} outside (50, 100]',
                 'bins': f'--calib_bins {a.calib_bins} outside {quantize.MIN_BINS}..{quantize.MAX_BINS}'}[e.argument])
    return main(a.pre_ckpt, a.output, a.image_size, a.output_size, a.model_def, a.class_num, a.depth_multiplier, a.train_set, a.calib,
                a.synthetic, a.calib_seed, a.calib_batch, a.calib_limit, a.ranges, method, a.calib_percentile, a.calib_bins, on['equalize'],
                a.equalize_max_gain, on['bias_correct'], on['adaround'], a.adaround_iters, a.adaround_lambda, a.adaround_lr, on['analyze'],
                a.analyze_seed, a.analyze_top)


if __name__ == '__main__':
    cli()
