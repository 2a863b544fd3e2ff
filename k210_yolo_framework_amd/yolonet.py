"""Host-side mirror of the reference's model plugin API (`models/yolonet.py`).

The reference selects a network by name (`eval(model_def)`, keras_inference.py:77-78, keras_train.py:49-50)
and calls it as  net([H,W,3], anchor_num, class_num, alpha=...) -> (yolo_model, yolo_model_warpper)  where
`yolo_model` emits [N,h,w,A*(5+C)] per scale and `yolo_model_warpper` the same data reshaped to
[N,h,w,A,5+C] (yolonet.py:40-44).  The same four names are registered here; the objects returned expose
the methods the reference scripts use — `load_weights`, `predict`, `save_weights` — with numpy in / list of
numpy out and the reference's shapes and (h, w, anchor, entry) order.

All arithmetic happens in libyolo_hip.so (engine.Plan); without a GPU `predict` raises.  The models default to the 'f16x2'
precision mode (fp16 MFMA with compensated operands: the fp32-class results a Keras user expects, scores within 1e-3 and the same
boxes); pass precision='f16' (or set `model.precision`) for the throughput mode used by bench.py.
precision='kpu' runs a loaded `.kmodel` / `.kfpkg` on the K210 KPU's own integer arithmetic (engine.KpuPlan): the outputs the board
computes, bit for bit as oracle/kpu_ref.py restates them.  The KPU takes the raw 0..255 pixels of uint8 frames; the float modes divide
each image by its own maximum first (tools/utils.py:405), so for images whose maximum is below 255 the two modes see different inputs.

Weights: Keras HDF5 files (`.h5`, read and written by keras_io / h5lite without h5py: the reference's checkpoint format,
including the 255->A*(5+C) head cut of yolonet.py:146-156,182-189) or a flat `.npz` with Keras-layout arrays
(`<layer>/kernel` HWIO, `<layer>/bias`, `<bn>/gamma|beta|moving_mean|moving_variance`).
Unlike the reference (yolonet.py:16-21,146,182) building a model does NOT require pre-train files: it
starts from seeded random weights until `load_weights` is called; `load_weights(path, by_name=True)` loads a backbone-only
pre-train file the way `base_model.load_weights('data/mobilenet_v1_base_7.h5')` does.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import netspec as ns


class YoloModel:
    """`wrapped=False` -> yolo_model ([N,h,w,A*(5+C)]), `wrapped=True` -> yolo_model_warpper ([N,h,w,A,5+C])."""

    def __init__(self, spec: ns.NetSpec, shared: dict, wrapped: bool):
        self.spec = spec
        self._s = shared          # weights + lazily built engine plan, shared by both views of one network
        self.wrapped = wrapped

    @property
    def precision(self) -> str:
        return self._s.get('precision', 'f16x2')

    @precision.setter
    def precision(self, value: str) -> None:
        if value != self.precision:
            self._s['precision'] = value
            self._drop_plan()

    # -- Keras-like surface -------------------------------------------------------------------------
    @property
    def input_shape(self):
        return (None, *self.spec.in_hw, 3)

    @property
    def output_shape(self):
        e = 5 + self.spec.class_num
        a = self.spec.anchor_num
        return [(None, h, w, a, e) if self.wrapped else (None, h, w, a * e) for (h, w) in self.spec.out_hw()]

    def get_weights(self) -> Dict[str, np.ndarray]:
        return self._s['weights']

    def set_weights(self, weights: Dict[str, np.ndarray]) -> None:
        want = self.spec.init_weights(seed=0)
        for k, v in want.items():
            if k not in weights:
                raise KeyError(f'missing weight {k}')
            if tuple(weights[k].shape) != tuple(v.shape):
                raise ValueError(f'{k}: shape {weights[k].shape} != {v.shape}')
        self._s['weights'] = {k: np.asarray(weights[k], np.float32) for k in want}
        self._s.pop('kmodel', None)              # the integer model no longer describes these weights
        self._s.pop('kpu_program', None)
        self._drop_plan()

    def load_weights(self, path: str, by_name: bool = False) -> None:
        """keras_inference.py:80 / keras_train.py:52-57.  `.h5`/`.hdf5`: a Keras weight or full-model file; `.kmodel`/`.kfpkg`: a
        quantised yolo_mobilev1 - the K210 demo's, or one `save_kmodel` / `make kmodel` wrote for this network (kmodel.py); otherwise `.npz`.
        by_name=True accepts a file that covers only part of the network (backbone pre-train files, yolonet.py:16-21)."""
        path = str(path)
        if path.endswith(('.h5', '.hdf5', '.keras')):
            from . import keras_io
            w, self.last_load_report = keras_io.load_keras_weights(self.spec, path, base=self._s['weights'], strict=not by_name)
            self.set_weights(w)
            return
        if path.endswith(('.kmodel', '.kfpkg')):
            # the K210 demo's 8-bit model (yolo3_frame_test_public/kfpkg/kpu_yolov3.kfpkg -> yolo.kmodel, main.c:57,213,274), dequantised
            from . import kmodel
            data = kmodel.read_kfpkg(path) if path.endswith('.kfpkg') else open(path, 'rb').read()
            km = kmodel.parse(data)
            w, self.last_load_report = kmodel.to_float_weights(km, self.spec if self.spec.name == 'yolo_mobilev1' else None)
            self.set_weights(w)
            self._s['kmodel'] = km                   # kept beside its float weights: precision='kpu' runs it as the board does
            return
        with np.load(path) as z:
            have = {k: z[k] for k in z.files}
        if by_name:
            have = {**self._s['weights'], **have}
        self.set_weights(have)

    def save(self, path: str) -> None:
        """`keras.models.save_model(yolo_model, path)` (keras_train.py:105-109): the full-model HDF5 file - `model_config` (the
        architecture as Keras JSON) plus the weights under `/model_weights`."""
        from . import keras_io
        keras_io.save_keras_model(self.spec, self._s['weights'], str(path))

    def save_weights(self, path: str) -> None:
        """Weights only: `.h5` -> Keras `save_weights` layout (what the reference's `load_weights` reads), else `.npz`.  The full-model
        file of keras_train.py:105-109 is `save`."""
        path = str(path)
        if path.endswith(('.h5', '.hdf5')):
            from . import keras_io
            keras_io.save_keras_weights(self.spec, self._s['weights'], path)
        else:
            np.savez(path, **self._s['weights'])

    def save_kmodel(self, path: str, calibration_frames, batch: int = 32, method: str = 'minmax', percentile: float = 99.99, bins: int = 2048,
                    equalize: bool = False, max_gain: float = 64.0, bias_correct: bool = False, adaround: bool = False, ada_iters: int = 1000,
                    ada_lambda: float = 0.01, ada_lr: float = 1e-2, analyze: bool = False, analyze_frames=None, analyze_top: int = 3):
        """Quantise these weights to a K210 kmodel (quantize.py) and write it: `.kmodel`, or `.kfpkg` (model + flash list, no
        firmware).  calibration_frames: uint8 [N, H, W, 3] at the network's input size (host numpy or a device tensor); their tensor ranges
        are measured on the GPU in batches of `batch`, from the raw pixels / 255 as the KPU sees them.  The new Kmodel is kept beside the
        float weights, so precision='kpu' runs it on this object without reloading.  Returns the quantiser's report (also
        `last_quantize_report`).  A network the KPU path cannot express raises YkError with the quantiser's reason.
        method 'percentile' / 'mse' (quantize.clip_range) clips every range from a histogram of `bins` bins, taken on the GPU in a second
        pass over the frames; report['clipped'] lists the tensors it moved.  The default, 'minmax', is the exact range and one pass.
        equalize=True first equalises the channel ranges (equalize.py): one more pass over the frames measures every conv output per channel
        (Calibrator.feed_channels), equalize.equalize rewrites the weights (gains up to `max_gain`), and calibration and quantisation then run
        on THOSE weights; report['equalize'] holds the gains.  The written file is the equalised network - the same function, other weights;
        this object's float weights are not touched.
        bias_correct=True (biascorrect.py) then removes the systematic error the chosen ranges leave: on the same frames, one more float pass
        sums every channel's pre-activation (Calibrator.feed_means), and one KPU-exact statistics pass PER CONV (KpuPlan.run_stats_u8) finds the
        integer to add to each channel's bn_add so that its mean pre-activation equals the float network's within 2^-(p + 1) of a code;
        report['biascorrect'] lists the layers.
        adaround=True (adaround.py) chooses, after the calibration and on the same frames, for every kernel weight the lower or the upper of its
        two neighbouring codes so that each output channel's error over the frames falls (`ada_iters` Adam steps per layer on the GPU, rounding
        regulariser `ada_lambda`, step `ada_lr`); no row ends worse than nearest rounding in that objective; report['adaround'] lists the layers.
        Order: equalise, calibrate, adaround, bias-correct, write.
        analyze=True (qerror.py) then measures the FINISHED kmodel - whatever of the above made it - against the float network it was made of, conv
        by conv, on `analyze_frames` (as calibration_frames; None: the calibration frames): accumulated and local SQNR, cosine, mean and largest
        error in codes, the share of codes at 0 and 255 and the `analyze_top` worst channels.  report['qerror'] holds it, format_report prints
        it, and `path`.qerror.json gets the same data.  The written kmodel has the same bytes with it on and off."""
        import torch
        from . import engine, kmodel, quantize
        try:
            quantize.plan_convs(self.spec)                       # refuse before any GPU work
            if equalize and not float(max_gain) > 1.0:
                raise kmodel.KmodelError(f'equalize: max_gain {max_gain} must be above 1')
        except kmodel.KmodelError as e:
            raise engine.YkError(f'save_kmodel: {e}') from e
        frames = calibration_frames if torch.is_tensor(calibration_frames) else torch.from_numpy(np.ascontiguousarray(calibration_frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or len(frames) == 0:
            raise engine.YkError('save_kmodel: calibration_frames must be uint8 [N, H, W, 3], N >= 1')
        clipped = []
        weights, eq_report = self._s['weights'], None
        if equalize:
            from . import equalize as eq
            try:
                weights, eq_report = eq.equalize(self.spec, weights, quantize.calibrate_channels(self.spec, weights, frames, batch), max_gain)
            except kmodel.KmodelError as e:
                raise engine.YkError(f'save_kmodel: {e}') from e
        ranges = quantize.calibrate(self.spec, weights, frames, batch, method, percentile, bins, clipped)
        try:
            delta, bc_report, codes, ada_report = None, None, None, None
            if adaround:
                from . import adaround as ada
                codes, ada_report = ada.gpu_optimise(self.spec, weights, frames, batch, ada_iters, ada_lambda, ada_lr)
            if bias_correct:
                from . import biascorrect
                delta, bc_report = biascorrect.correct(self.spec, weights, ranges, quantize.calibrate_means(self.spec, weights, frames, batch),
                                                       biascorrect.gpu_measure(frames, batch), codes)
            km, report = quantize.quantize(self.spec, weights, ranges, delta, codes)
            if ada_report is not None:
                report['adaround'] = ada_report
            if bc_report is not None:
                report['biascorrect'] = bc_report
                for name, r in bc_report['layers'].items():
                    report['layers'][name]['bias_limited'] = len(r['limited'])
            if eq_report is not None:
                report['equalize'] = eq_report
            if method != 'minmax':
                report['clipped'] = clipped
            report['file_bytes'] = kmodel.write(path, km)
        except kmodel.KmodelError as e:
            raise engine.YkError(f'save_kmodel: {e}') from e
        self._s['kmodel'] = km
        self._s.pop('kpu_program', None)
        if self.precision == 'kpu':
            self._drop_plan()
        if analyze:
            from . import qerror
            report['qerror'] = qerror.analyze(self.spec, weights, km, report, frames if analyze_frames is None else analyze_frames, batch,
                                              top=analyze_top)
            with open(str(path) + '.qerror.json', 'w') as f:
                f.write(qerror.to_json(report['qerror']))
        self.last_quantize_report = report
        return report

    def _drop_plan(self):
        p = self._s.pop('plan', None)
        if p is not None:
            p.close()

    def _plan(self, batch: int):
        from . import engine
        p = self._s.get('plan')
        if p is None or p.max_batch < batch:
            self._drop_plan()
            if self.precision == 'kpu':
                p = engine.KpuPlan(self._kmodel(), max_batch=max(batch, 1))
            else:
                p = engine.Plan(self.spec, self._s['weights'], max_batch=max(batch, 1), precision=self.precision)
            self._s['plan'] = p
        return p

    def _kmodel(self):
        """The loaded kmodel packed once for the KPU-exact mode (kept beside it) and checked against this network's input and output
        shapes (precision='kpu')."""
        from . import engine, kmodel
        km = self._s.get('kmodel')
        if km is None:
            raise engine.YkError("precision='kpu' runs a K210 kmodel: load_weights a .kmodel or .kfpkg first")
        prog = self._s.get('kpu_program')
        if prog is None:
            try:
                prog = kmodel.pack_kpu(km)
            except kmodel.KmodelError as e:
                raise engine.YkError(f"precision='kpu': {e}") from e
            self._s['kpu_program'] = prog
        want_in = (3, *self.spec.in_hw)
        e = 5 + self.spec.class_num
        want_out = [(self.spec.anchor_num * e, h, w) for (h, w) in self.spec.out_hw()]
        if tuple(prog.input_chw) != want_in or prog.output_shapes() != want_out:
            raise engine.YkError(f'kmodel takes {tuple(prog.input_chw)} and gives {prog.output_shapes()} (C, H, W); this network takes '
                                 f'{want_in} and gives {want_out}')
        return prog

    def predict(self, x: np.ndarray) -> List[np.ndarray]:
        """keras_inference.py:88.  x: [N,H,W,3] float (already `img / np.max(img)`) or uint8 frames
        (then the normalisation of tools/utils.py:405 is done on the GPU).  precision='kpu': uint8 frames only, raw 0..255 pixels."""
        import torch
        x = np.asarray(x)
        if x.ndim == 3:
            x = x[None]
        n = x.shape[0]
        if self.precision == 'kpu' and x.dtype != np.uint8:
            from . import engine
            raise engine.YkError("precision='kpu' takes uint8 frames (the KPU's raw 0..255 pixels), not normalised floats")
        plan = self._plan(n)
        if x.dtype == np.uint8:
            plan.run_u8(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        else:
            plan.run_f32(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        torch.cuda.synchronize()
        outs = [o[:n].cpu().numpy() for o in plan.outputs()]
        if self.wrapped:
            e = 5 + self.spec.class_num
            outs = [o.reshape(n, o.shape[1], o.shape[2], self.spec.anchor_num, e) for o in outs]
        return outs


def _build(name: str, input_shape, anchor_num: int, class_num: int, **kwargs) -> Tuple[YoloModel, YoloModel]:
    alpha = kwargs.get('alpha', 1.0)
    spec = ns.NETWORKS[name](list(input_shape), anchor_num, class_num, alpha=alpha)
    shared = {'weights': spec.init_weights(seed=1), 'precision': kwargs.get('precision', 'f16x2')}
    return YoloModel(spec, shared, False), YoloModel(spec, shared, True)


def yolo_mobilev1(input_shape, anchor_num, class_num, **kwargs):
    """models/yolonet.py:12-46."""
    return _build('yolo_mobilev1', input_shape, anchor_num, class_num, **kwargs)


def yolo_mobilev2(input_shape, anchor_num, class_num, **kwargs):
    """models/yolonet.py:49-104."""
    return _build('yolo_mobilev2', input_shape, anchor_num, class_num, **kwargs)


def tiny_yolo(input_shape, anchor_num, class_num, **kwargs):
    """models/yolonet.py:107-158."""
    return _build('tiny_yolo', input_shape, anchor_num, class_num, **kwargs)


def yolo(input_shape, anchor_num, class_num, **kwargs):
    """models/yolonet.py:161-191."""
    return _build('yolo', input_shape, anchor_num, class_num, **kwargs)


# the reference uses eval(model_def); a dict keeps the same names without eval
MODEL_DEFS = {'yolo_mobilev1': yolo_mobilev1, 'yolo_mobilev2': yolo_mobilev2, 'tiny_yolo': tiny_yolo, 'yolo': yolo}
