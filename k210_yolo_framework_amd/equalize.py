"""Cross-layer range equalisation before quantising (`make kmodel EQUALIZE=True`): the spread BETWEEN the channels of a
tensor, which one (scale, zero point) per tensor cannot follow, is moved into the KPU's per-channel BatchNorm stage.

    new_weights, report = equalize(spec, weights, channel_ranges, max_gain=64.0)

Pure numpy, float64, no torch, no GPU: the rule.  `weights` is the Keras-layout dict quantize.quantize takes (not mutated); `new_weights`
has the same keys, shapes and dtypes and is a checkpoint like any other - the same function in real arithmetic, with other weights.
`channel_ranges` = {conv layer name: (lo[C], hi[C])}, the range of every output channel over the calibration set
(quantize.Calibrator.channel_ranges on the GPU).  Two facts carry it: the BatchNorm stage is per channel, and every activation the KPU path
takes (linear, ReLU, LeakyReLU) satisfies act(g x) = g act(x) for g > 0.

Step A, activation channels.  For every conv / depthwise output tensor with exactly one reader, that reader a conv or depthwise op, and
that is no network output: a_c = max(|lo_c|, |hi_c|), A = max_c a_c, and a gain g_c per channel -
    depthwise reader   g_c = A / a_c: the channel fills the tensor's range (the reader's own output scaling, step B, absorbs the 1 / g_c);
    full-conv reader   g_c = k sqrt(r_c / a_c), r_c the largest |w| of the reader's input-channel slice c: the balance of Nagel et al., after
                       which every channel takes the share of the tensor's range that its slice takes of the reader's; the common factor k
                       is the one that leaves max_c g_c a_c = A WITH the clamp below applied (k = A / max_c sqrt(r_c a_c) where no clamp is
                       active);
    g_c is clamped to [1 / max_gain, max_gain]; g_c = 1 where a_c or r_c is 0.
The producer's channel c is multiplied by g_c - gamma_c and beta_c with BatchNorm (folded scale and bias both scale), kernel output channel c
and bias_c for a biased conv without - and the reader's kernel input channel c is divided by g_c.  Tensors read by `upsample` or `concat`,
tensors with several readers and network outputs are left alone and listed in report['skipped'] with the reason.

Step B, weight output channels, after A, on every conv and depthwise layer with BatchNorm.  [wmin, wmax] = the kernel's range widened to
contain 0;  f_c = min(wmax / max(w_c), wmin / min(w_c)), a ratio whose denominator is 0 or of the other sign counting as +inf (that end
cannot be reached); f_c clamped to [1, max_gain], 1 for an all-zero channel.  kernel_c *= f_c, gamma_c /= f_c, moving_mean_c *= f_c: the
folded scale is divided by f_c and the folded bias is unchanged (quantize.fold_bn).  The tensor's [wmin, wmax] - so s_w and zp_w - do not
move (the result is clipped to it after the one rounding to the checkpoint's dtype), exact zeros stay exact zeros, and every live channel
now reaches an end of the weight code.  Convs without BatchNorm (the output convs) are left alone.

max_gain is a condition, not a measurement: a channel that used fewer than 256 / max_gain codes is not stretched further.  Values <= 1 are
refused.  In a float32 checkpoint every changed tensor is rounded once (2^-24 relative), so the function is kept to that; in float64, to
float64.

Restated from Nagel, van Baalen, Blankevoort, Welling, "Data-Free Quantization Through Weight Equalization and Bias Correction" (2019),
section 4.1, for asymmetric per-tensor codes and measured (not BatchNorm-predicted) activation ranges; parity with the authors' or AIMET's
code is unpinned.  Bias correction, the paper's second half, is not here."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import netspec as ns
from .kmodel import KmodelError
from .quantize import _OP_NAMES, _consumers, tensor_names

DEFAULT_MAX_GAIN = 64.0


def _chan_axis(layer: ns.Layer) -> int:
    return 3 if layer.kind == 'conv' else 2


def _per_chan(v: np.ndarray, layer: ns.Layer) -> np.ndarray:
    """A per-output-channel vector shaped to multiply the layer's kernel."""
    return v.reshape((1, 1, 1, -1) if layer.kind == 'conv' else (1, 1, -1, 1))


def activation_gains(a: np.ndarray, r, max_gain: float) -> np.ndarray:
    """g[C] of step A for channel extents `a` and, for a full-conv reader, its input-slice maxima `r` (None: a depthwise reader)."""
    a = np.asarray(a, np.float64)
    A = float(a.max()) if a.size else 0.0
    g = np.ones_like(a)
    if A == 0.0:
        return g
    if r is None:
        live = a > 0.0
        g[live] = np.minimum(A / a[live], max_gain)
        return g
    r = np.asarray(r, np.float64)
    live = (a > 0.0) & (r > 0.0)
    if not live.any():
        return g
    g0 = np.sqrt(r[live] / a[live])
    al = a[live]
    bound = al * max_gain > A                                                  # the channels that could pass A: each caps the common factor
    with np.errstate(over='ignore'):
        k = float((A / (g0[bound] * al[bound])).min()) if bound.any() else np.inf
        g[live] = np.clip(k * g0, 1.0 / max_gain, max_gain)
    return g


def weight_gains(kern: np.ndarray, layer: ns.Layer, max_gain: float) -> np.ndarray:
    """f[C] of step B for a float64 kernel."""
    ax = tuple(i for i in range(4) if i != _chan_axis(layer))
    wmin, wmax = min(float(kern.min()), 0.0), max(float(kern.max()), 0.0)
    cmax, cmin = kern.max(axis=ax), kern.min(axis=ax)
    with np.errstate(divide='ignore', invalid='ignore'):
        up = np.where(cmax > 0.0, wmax / np.where(cmax > 0.0, cmax, 1.0), np.inf)
        dn = np.where(cmin < 0.0, wmin / np.where(cmin < 0.0, cmin, 1.0), np.inf)
    f = np.minimum(up, dn)
    return np.where(np.isfinite(f), np.clip(f, 1.0, max_gain), 1.0)


def _stats(v: np.ndarray) -> Tuple[int, float, float]:
    return int((v != 1.0).sum()), float(v.min()), float(v.max())


def _check(spec, channel_ranges, max_gain) -> float:
    max_gain = float(max_gain)
    if not max_gain > 1.0 or not np.isfinite(max_gain):
        raise KmodelError(f'equalize: max_gain {max_gain} must be a finite value above 1')
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV) or channel_ranges is None:
            continue
        name, co = op['layer'], op['cout']
        if name not in channel_ranges:
            raise KmodelError(f'equalize: no per-channel range for layer {name!r}')
        lo, hi = (np.asarray(v, np.float64).reshape(-1) for v in channel_ranges[name])
        if len(lo) != co or len(hi) != co:
            raise KmodelError(f'equalize: layer {name!r} has {co} output channels, its per-channel range has {len(lo)} / {len(hi)}')
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise KmodelError(f'equalize: the per-channel range of layer {name!r} is not finite')
    return max_gain


def _finish(weights, w64, changed):
    """The changed tensors rounded once to their dtype, the others copied."""
    return {k: (w64[k].astype(np.asarray(v).dtype) if k in changed else np.array(v)) for k, v in weights.items()}


def equalize_activations(spec: ns.NetSpec, weights, channel_ranges, max_gain: float = DEFAULT_MAX_GAIN):
    """Step A alone -> (new_weights, {layer: g[C] of its output channels}, skipped)."""
    max_gain = _check(spec, channel_ranges, max_gain)
    lay = {l.name: l for l in spec.layers}
    names = tensor_names(spec)
    readers = _consumers(spec)
    w64 = {k: np.array(v, np.float64) for k, v in weights.items()}             # copies: the input is not touched
    changed, gains, skipped = set(), {}, []
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        name, t = op['layer'], op['out']
        rd = readers.get(t, [])
        why = None
        if t in spec.outputs:
            why = 'a network output'
        elif len(rd) != 1:
            why = f'{len(rd)} readers'
        elif spec.ops[rd[0]]['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            why = f"read by `{_OP_NAMES[spec.ops[rd[0]]['type']]}`"
        elif op['act'] not in (ns.ACT_NONE, ns.ACT_RELU, ns.ACT_LEAKY):
            why = 'its activation is not positively homogeneous'
        elif not lay[name].bn_name and not lay[name].use_bias:
            why = 'no BatchNorm and no bias to carry the gain'
        if why:
            skipped.append(dict(tensor=names[t], reason=why))
            continue
        l, rl = lay[name], lay[spec.ops[rd[0]]['layer']]
        lo, hi = (np.asarray(v, np.float64).reshape(-1) for v in channel_ranges[name])
        a = np.maximum(np.abs(lo), np.abs(hi))
        rk = w64[rl.name + '/kernel']
        g = activation_gains(a, None if rl.kind == 'dwconv' else np.abs(rk).max(axis=(0, 1, 3)), max_gain)
        gains[name] = g
        if not (g != 1.0).any():
            continue
        if l.bn_name:
            w64[l.bn_name + '/gamma'] *= g
            w64[l.bn_name + '/beta'] *= g
            changed.update((l.bn_name + '/gamma', l.bn_name + '/beta'))
        else:
            w64[l.name + '/kernel'] *= _per_chan(g, l)
            w64[l.name + '/bias'] *= g
            changed.update((l.name + '/kernel', l.name + '/bias'))
        rk /= g.reshape(1, 1, -1, 1)                                           # the reader's input-channel axis, conv and depthwise alike
        changed.add(rl.name + '/kernel')
    return _finish(weights, w64, changed), gains, skipped


def equalize_weights(spec: ns.NetSpec, weights, max_gain: float = DEFAULT_MAX_GAIN):
    """Step B alone -> (new_weights, {layer: f[C] of its kernel's output channels})."""
    max_gain = _check(spec, None, max_gain)
    w64 = {k: np.array(v, np.float64) for k, v in weights.items()}
    changed, gains = set(), {}
    for l in spec.layers:
        if not l.bn_name:
            continue
        kern = w64[l.name + '/kernel']
        f = weight_gains(kern, l, max_gain)
        gains[l.name] = f
        if not (f != 1.0).any():
            continue
        dt = np.asarray(weights[l.name + '/kernel']).dtype
        wmin, wmax = np.minimum(kern.min(), 0.0).astype(dt), np.maximum(kern.max(), 0.0).astype(dt)     # exact: they are values of that dtype
        w64[l.name + '/kernel'] = np.clip((kern * _per_chan(f, l)).astype(dt), wmin, wmax).astype(np.float64)    # the rounding cannot pass an end
        w64[l.bn_name + '/gamma'] /= f
        w64[l.bn_name + '/moving_mean'] *= f
        changed.update((l.name + '/kernel', l.bn_name + '/gamma', l.bn_name + '/moving_mean'))
    return _finish(weights, w64, changed), gains


def equalize(spec: ns.NetSpec, weights: Dict[str, np.ndarray], channel_ranges: Dict[str, Tuple[np.ndarray, np.ndarray]],
             max_gain: float = DEFAULT_MAX_GAIN):
    """-> (new_weights, report): step A, then step B on its result.  report = {'max_gain', 'layers': {name: dict(a_changed, g_min, g_max,
    b_changed, f_min, f_max)}, 'gains': {name: (g[C], f[C])}, 'skipped': [dict(tensor, reason)]}; g of a layer is the gain of its OUTPUT
    channels (step A), f that of its kernel's output channels (step B).  KmodelError naming the layer for a missing or mis-sized entry of
    `channel_ranges`, and for max_gain <= 1."""
    after_a, g, skipped = equalize_activations(spec, weights, channel_ranges, max_gain)
    out, f = equalize_weights(spec, after_a, max_gain)
    report = {'max_gain': float(max_gain), 'layers': {}, 'gains': {}, 'skipped': skipped}
    for l in spec.layers:
        co = l.kernel_shape[_chan_axis(l)]
        gl, fl = g.get(l.name, np.ones(co)), f.get(l.name, np.ones(co))
        (na, g0, g1), (nb, f0, f1) = _stats(gl), _stats(fl)
        report['layers'][l.name] = dict(a_changed=na, g_min=g0, g_max=g1, b_changed=nb, f_min=f0, f_max=f1)
        report['gains'][l.name] = (gl, fl)
    return out, report


def format_report(report: dict) -> str:
    """The lines quantize.format_report adds for report['equalize']."""
    rows = [f"equalised (max_gain {report['max_gain']:g}): {'layer':<14}{'out ch':>7}{'g min':>10}{'g max':>10}{'kern ch':>8}{'f min':>10}{'f max':>10}"]
    for name, r in report['layers'].items():
        rows.append(f"{'':<28}{name:<14}{r['a_changed']:>7}{r['g_min']:>10.4g}{r['g_max']:>10.4g}{r['b_changed']:>8}{r['f_min']:>10.4g}{r['f_max']:>10.4g}")
    for r in report['skipped']:
        rows.append(f"not equalised: {r['tensor']} ({r['reason']})")
    return '\n'.join(rows)
