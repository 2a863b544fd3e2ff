"""Quantise a float checkpoint to a K210 kmodel (v3): the step the reference leaves to `keras_freeze.py` + nncase.

    ranges = Calibrator(spec, weights, max_batch).feed(frames) ... .ranges()      GPU: the range of every tensor over the calibration set
    ... .feed_hist(frames) ... .ranges('mse' | 'percentile', percentile)           GPU, optional second pass: histograms -> clipped ranges
    km, report = quantize(spec, weights, ranges)                                   CPU, deterministic: KPU registers and tables
    kmodel.write('yolo.kmodel', km)

Conventions - exactly the ones `kmodel.to_float_weights` inverts and `oracle/kpu_ref.py` executes:
  * one asymmetric uint8 (scale, zero point) per weight tensor and per activation tensor, real = scale * (q - zp);
  * INTEGER zero points: a range is widened to contain 0 and zp = round(-min / scale), so real zero is exactly q = zp - zero padding is
    pad_value = zp_x, and a pruned (exactly zero) weight is exactly zp_w;
  * the input tensor is the raw pixel: scale 1/255, zero point 0;
  * the zero-point terms are exact: arg_x = -zp_w << 15 with shr_x = 15, arg_w = -zp_x << 15 with shr_w = 15, arg_add = zp_x zp_w k^2, so
    acc = sum((x - zp_x)(w - zp_w));
  * BatchNorm per channel: the pre-activation in units of 2^-p output steps is  z = (acc * bn_mul >> bn_shift) + bn_add  with
    bn_mul / 2^bn_shift = scale_c s_x s_w 2^p / s_y and bn_add = round(bias_c 2^p / s_y); every channel takes the largest shift (<= 15) that
    keeps bn_mul inside its 24 bits, p = 10 unless a channel's multiplier needs fewer;
  * the activation is a segment table over z with the kink at real zero (z = 0): slope 2^-p above it, alpha 2^-p below (LeakyReLU), 0 below
    (ReLU), or one line (linear).  Below the calibrated minimum the table is flat at q = 0; above the calibrated maximum the KPU's own
    clamp to 255 is the flat end (a segment bias is a signed byte and cannot hold 255; for the same reason a LeakyReLU tensor whose zero
    point would exceed 127 has its range widened upward until it is 127);
  * the two linear output convs carry their bias in bn_add; their DEQUANTIZE (scale s_y, bias -zp_y s_y) gives real logits.
A range of zero width ([0, 0] after widening: a tensor that is constantly zero) gets scale 1/255 and zero point 0 - no division by zero, and
the constant is represented exactly.

The layer sequence is the demo's: KPU convs (a stride-2 depthwise conv runs at stride 1 and its 1x1 successor carries the
`left_top_2_s2` pooling, as nncase emits it; a stride-2 full conv pools itself), KLF_MAIN_MEM_OUT where a tensor leaves the KPU,
QUANTIZED_RESIZE_NN for `upsample`, one REQUANTIZE per `concat` input onto the union range, QUANTIZED_CONCAT + K210_UPLOAD, DEQUANTIZE
for every network output.  What the KPU path cannot express raises `KmodelError` naming the op.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import kmodel as km_
from . import netspec as ns
from .kmodel import KmodelError

FINE_BITS = 10                   # z counts 2^-10 output steps (what the demo's tables use: y_mul 1024 >> 20)
ACT_MUL_BITS = 14                # the table's slope 2^-p is written as 2^14 >> (p + 14): alpha keeps 14 bits
INPUT_SCALE = 1.0 / 255.0

_OP_NAMES = {ns.OP_MAXPOOL: 'maxpool', ns.OP_UPSAMPLE: 'upsample', ns.OP_CONCAT: 'concat', ns.OP_ADD: 'add'}


def tensor_names(spec: ns.NetSpec) -> List[str]:
    """A name for every tensor of the spec: 'input', the layer name for a conv's output, '<op>_<n>' (n counts from 1 per op type) for
    the others."""
    names = ['?'] * len(spec.tensors)
    names[0] = 'input'
    seen: Dict[str, int] = {}
    for op in spec.ops:
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            names[op['out']] = op['layer']
        else:
            kind = _OP_NAMES[op['type']]
            seen[kind] = seen.get(kind, 0) + 1
            names[op['out']] = f'{kind}_{seen[kind]}'
    return names


def qparams(lo: float, hi: float) -> Tuple[float, int]:
    """(scale, integer zero point) of the uint8 code for the range [lo, hi] widened to contain 0."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise KmodelError(f'quantize: range ({lo}, {hi}) is not a finite interval')
    lo, hi = min(lo, 0.0), max(hi, 0.0)
    if hi == lo:
        return INPUT_SCALE, 0
    scale = (hi - lo) / 255.0
    return scale, int(min(255, max(0, round(-lo / scale))))


def fold_bn(layer: ns.Layer, weights) -> Tuple[np.ndarray, np.ndarray]:
    """Inference BatchNorm as float64 (scale, bias) per channel; a conv with bias and no BatchNorm: scale = 1."""
    c = layer.kernel_shape[3] if layer.kind == 'conv' else layer.kernel_shape[2]
    if layer.bn_name:
        g, bt, mu, var = (np.asarray(weights[layer.bn_name + s], np.float64) for s in ('/gamma', '/beta', '/moving_mean', '/moving_variance'))
        scale = g / np.sqrt(var + ns.BN_EPS)
        return scale, bt - mu * scale
    return np.ones(c), (np.asarray(weights[layer.name + '/bias'], np.float64) if layer.use_bias else np.zeros(c))


def _op_inputs(op: dict) -> List[int]:
    """The tensors an op reads."""
    return [op[key] for key in ('in0', 'in1') if op.get(key, -1) is not None and op.get(key, -1) >= 0]


def _consumers(spec: ns.NetSpec) -> Dict[int, List[int]]:
    r: Dict[int, List[int]] = {}
    for k, op in enumerate(spec.ops):
        for t in _op_inputs(op):
            r.setdefault(t, []).append(k)
    return r


def plan_convs(spec: ns.NetSpec) -> Dict[int, dict]:
    """The geometry of every conv op as the KPU runs it, {op index: dict(in_h, in_w, out_h, out_w, pool)}, and every refusal that needs
    no weights.  KmodelError names the op the KPU path here cannot express."""
    if not spec.ops or spec.ops[0]['type'] != ns.OP_CONV or spec.ops[0]['in0'] != 0 or spec.tensors[0][2] != 3:
        raise KmodelError('quantize: the first layer must be a conv of the 3-channel frame')
    readers = _consumers(spec)
    hw: Dict[int, Tuple[int, int]] = {0: spec.tensors[0][:2]}                   # what the KPU holds for a tensor (full size when the pooling is deferred)
    deferred = set()
    plan: Dict[int, dict] = {}
    for k, op in enumerate(spec.ops):
        t = op['type']
        if t in (ns.OP_ADD, ns.OP_MAXPOOL):
            raise KmodelError(f"quantize: op {k} of {spec.name} is `{_OP_NAMES[t]}` on tensor {tensor_names(spec)[op['in0']]!r}: "
                              f'the KPU path has no {_OP_NAMES[t]}')
        if t in (ns.OP_UPSAMPLE, ns.OP_CONCAT):
            hw[op['out']] = spec.tensors[op['out']][:2]
            continue
        name = op['layer']
        if op['k'] not in (1, 3):
            raise KmodelError(f"quantize: conv {name!r} has a {op['k']}x{op['k']} kernel (the KPU has 1x1 and 3x3)")
        H, W = hw[op['in0']]
        ci = spec.tensors[op['in0']][2]
        pads = (op['pad_t'], op.get('pad_b', op['pad_t']), op['pad_l'], op.get('pad_r', op['pad_l']))
        same = (op['k'] - 1) // 2
        pool, oh, ow = km_.POOL_BYPASS, H, W
        if op['in0'] in deferred:                                              # the 1x1 conv after a stride-2 depthwise conv
            pool, oh, ow = km_.POOL_LEFT_TOP_2_S2, H // 2, W // 2
        if op['stride'] == 2:
            if op['k'] != 3 or pads != (1, 1, 1, 1) or H % 2 or W % 2:
                raise KmodelError(f"quantize: conv {name!r} has stride 2 with kernel {op['k']}, padding {pads} on {H}x{W}: the KPU runs a "
                                  f'stride-2 conv as a pad-1 3x3 conv + left_top_2_s2 pooling, i.e. padding (1, 1, 1, 1) on an even size')
            nxt = [spec.ops[j] for j in readers.get(op['out'], [])]
            if (t == ns.OP_DWCONV and len(nxt) == 1 and nxt[0]['type'] == ns.OP_CONV and nxt[0]['k'] == 1 and nxt[0]['stride'] == 1
                    and op['out'] not in spec.outputs):
                deferred.add(op['out'])                                        # full size here; the successor pools
            else:
                pool, oh, ow = km_.POOL_LEFT_TOP_2_S2, H // 2, W // 2
        elif op['stride'] != 1 or pads != (same,) * 4:
            raise KmodelError(f"quantize: conv {name!r} has stride {op['stride']} and padding {pads}: the KPU pads a {op['k']}x{op['k']} "
                              f'conv by {same} on every side')
        hw[op['out']] = (oh, ow) if op['out'] not in deferred else (H, W)
        kh, kw = hw[op['out']]
        co = spec.tensors[op['out']][2]
        need = km_.kpu_tensor_units(ci, H, W) + km_.kpu_tensor_units(co, kh, kw)
        if need > km_.KPU_RAM_UNITS:
            raise KmodelError(f'quantize: conv {name!r} reads {ci}x{H}x{W} and writes {co}x{kh}x{kw}: {need * 64} bytes of KPU RAM, '
                              f'{km_.KPU_RAM_BYTES} exist')
        plan[k] = dict(in_h=H, in_w=W, out_h=kh, out_w=kw, pool=pool)
    return plan


def _act_table(act: int, alpha: float, zp_y: int, p: int):
    """(start, mul, shift, bias) x 16 over z in 2^-p output steps, kink at z = 0."""
    one, sh = 1 << ACT_MUL_BITS, p + ACT_MUL_BITS
    far = -(1 << 35)
    if act == ns.ACT_RELU:
        segs = [(far, 0, 0, zp_y), (0, one, sh, zp_y)]
    elif act == ns.ACT_LEAKY:
        if not 0.0 < alpha <= 1.0:
            raise KmodelError(f'quantize: LeakyReLU slope {alpha} outside (0, 1]')
        a_mul = int(round(alpha * one))
        z_lo = -int(round(zp_y * (1 << p) / (a_mul / one))) if a_mul else 0     # where the lower line reaches q = 0: the calibrated minimum
        segs = [(far, 0, 0, 0), (z_lo, a_mul, sh, 0), (0, one, sh, zp_y)] if zp_y and a_mul else [(far, 0, 0, zp_y), (0, one, sh, zp_y)]
    elif act == ns.ACT_NONE:
        segs = [(far, 0, 0, 0), (-(zp_y << p), one, sh, 0)]                     # one line through (0, zp_y), started where it reaches q = 0
    else:
        raise KmodelError(f'quantize: activation code {act} (ReLU6) has no KPU table here')
    top = (1 << 35) - 16
    segs += [(top + k, 0, 0, 0) for k in range(16 - len(segs))]                 # unreachable, ascending, as nncase fills the rest
    return tuple(np.array(col, np.int64) for col in zip(*segs))


def quantize(spec: ns.NetSpec, weights: Dict[str, np.ndarray], ranges: Dict[str, Tuple[float, float]],
             bn_add_delta: Optional[Dict[str, np.ndarray]] = None, weight_codes: Optional[Dict[str, np.ndarray]] = None):
    """-> (kmodel.Kmodel, report).  `ranges`: {tensor name (tensor_names): (min, max)} of the calibration set, at least for the input-side
    of every conv ('input' is fixed to the raw pixel and need not be given; upsample / concat outputs take their producers' ranges).
    report['layers'][name] = scales, zero points, FINE_BITS used, the BatchNorm shifts chosen, the share of weights equal to the zero
    point and the smallest non-zero |bn_mul| (what equalize.py's step A lowers for an amplified consumer).  CPU only, deterministic.
    `bn_add_delta` (bias correction, biascorrect.py): {conv layer name: int64 [C]} added to that layer's bn_add after its rounding, which
    moves every pre-activation z of channel c by exactly that many 2^-p output steps; None or {} changes nothing.  The report of a corrected
    layer gains `bias_delta_max` (the largest |delta| in output codes, |delta| / 2^p) and `bias_limited` (filled in by biascorrect.correct).
    `weight_codes` (adaptive rounding, adaround.py): {conv layer name: uint8 array of the kernel's shape} used in place of the nearest codes;
    every code must be the down code floor(kern / s_w) + zp_w or the up code, one above (both clipped to 0..255), of its weight; None or {}
    changes nothing.  `zero_share` is computed from the codes used."""
    plan = plan_convs(spec)
    bn_add_delta = dict(bn_add_delta or {})
    weight_codes = dict(weight_codes or {})
    convs = {op['layer'] for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)}
    for what, given in (('weight_codes', weight_codes), ('bn_add_delta', bn_add_delta)):
        unknown = sorted(set(given) - convs)
        if unknown:
            raise KmodelError(f'quantize: {what} names layer(s) {", ".join(map(repr, unknown))}, which are not conv layers of {spec.name}')
    names = tensor_names(spec)
    lay = {l.name: l for l in spec.layers}
    readers = _consumers(spec)
    leaves = {t for t in range(len(spec.tensors))
              if t in spec.outputs or any(spec.ops[j]['type'] in (ns.OP_UPSAMPLE, ns.OP_CONCAT) for j in readers.get(t, []))}
    layers: List[object] = []
    q: Dict[int, Tuple[float, int]] = {0: (INPUT_SCALE, 0)}
    rng: Dict[int, Tuple[float, float]] = {0: (0.0, 1.0)}
    kpu_of: Dict[int, int] = {}                                                # tensor -> KPU buffer
    bufs: List[dict] = []                                                      # KPU buffers: units, birth, death (layer indices)
    mem_of: Dict[int, int] = {}
    mem_top = 0
    out_entries: Dict[int, Tuple[int, int]] = {}
    report = {'layers': {}, 'requant': []}

    def mem_alloc(nbytes: int) -> int:
        nonlocal mem_top
        at = mem_top
        mem_top += (nbytes + 7) // 8 * 8
        return at

    def new_buf(c, h, w, born):
        bufs.append(dict(units=km_.kpu_tensor_units(c, h, w), birth=born, death=born))
        return len(bufs) - 1

    h0, w0, c0 = spec.tensors[0]
    kpu_of[0] = new_buf(c0, plan[0]['in_h'], plan[0]['in_w'], 0)
    for k, op in enumerate(spec.ops):
        t = op['type']
        idx = len(layers)
        if t in (ns.OP_CONV, ns.OP_DWCONV):
            l, g = lay[op['layer']], plan[k]
            tin, tout = op['in0'], op['out']
            if tin not in kpu_of:
                raise KmodelError(f"quantize: conv {l.name!r} reads tensor {names[tin]!r}, which is not in KPU RAM")
            if l.name not in ranges:
                raise KmodelError(f'quantize: no calibrated range for tensor {l.name!r}')
            dw = t == ns.OP_DWCONV
            ci, co, kk = op['cin'], op['cout'], op['k'] * op['k']
            s_x, zp_x = q[tin]
            kern = np.asarray(weights[l.name + '/kernel'], np.float64)
            s_w, zp_w = qparams(kern.min(), kern.max())
            if l.name in weight_codes:
                wq = np.asarray(weight_codes[l.name])
                down = np.floor(kern / s_w) + zp_w
                if wq.shape != kern.shape or wq.dtype != np.uint8:
                    raise KmodelError(f'quantize: weight_codes of conv {l.name!r} is {wq.dtype} {wq.shape}, uint8 {kern.shape} expected')
                off = (wq != np.clip(down, 0, 255)) & (wq != np.clip(down + 1, 0, 255))
                if off.any():
                    raise KmodelError(f'quantize: weight_codes of conv {l.name!r}: {int(off.sum())} code(s) are neither the down nor the up code '
                                      f'of their weight (the first at {tuple(int(v) for v in np.argwhere(off)[0])})')
            else:
                wq = np.clip(np.rint(kern / s_w) + zp_w, 0, 255).astype(np.uint8)
            wq = (wq[..., 0].transpose(2, 0, 1).reshape(co, 1, kk) if dw else wq.transpose(3, 2, 0, 1).reshape(co, ci, kk))
            lo, hi = (float(v) for v in ranges[l.name])
            s_y, zp_y = qparams(lo, hi)
            if op['act'] == ns.ACT_LEAKY and zp_y > 127:                        # the table holds the zero point in a signed byte (the kink's
                s_y, zp_y = qparams(lo, -lo * 128.0 / 127.0)                    # result bias): widen the range upward until it fits
            scale, bias = fold_bn(l, weights)
            m = scale * (s_x * s_w / s_y)                                       # acc -> output steps
            top = float(np.abs(m).max())
            p = FINE_BITS if top == 0.0 else int(min(FINE_BITS, np.floor(np.log2(((1 << 23) - 1) / top))))
            if p < 0:
                raise KmodelError(f'quantize: conv {l.name!r}: a channel multiplies the accumulator by {top:.3g}, beyond the 24-bit bn_mul')
            mf = m * float(1 << p)
            with np.errstate(divide='ignore'):
                shift = np.where(mf == 0.0, 15, np.floor(np.log2(((1 << 23) - 1) / np.maximum(np.abs(mf), 1e-300)))).clip(0, 15).astype(np.int64)
            bn_mul = np.rint(mf * np.exp2(shift)).astype(np.int64)
            over = np.abs(bn_mul) > (1 << 23) - 1                               # rounding pushed it past the field: one bit less
            shift = np.where(over & (shift > 0), shift - 1, shift)
            bn_mul = np.rint(mf * np.exp2(shift)).astype(np.int64)
            bn_add = np.rint(bias / s_y * float(1 << p)).astype(np.int64)
            delta = None
            if l.name in bn_add_delta:
                delta = np.asarray(bn_add_delta[l.name])
                if delta.shape != (co,) or delta.dtype.kind not in 'iu':
                    raise KmodelError(f'quantize: bn_add_delta of conv {l.name!r} is {delta.dtype} {delta.shape}, {co} integers expected')
                bn_add = bn_add + delta.astype(np.int64)
            a_start, a_mul, a_shift, a_bias = _act_table(op['act'], float(op['alpha']), zp_y, p)
            dst = new_buf(co, g['out_h'], g['out_w'], idx)
            bufs[kpu_of[tin]]['death'] = idx
            flags, mm_out = 0, 0
            if tout in leaves:
                flags, mm_out = km_.KLF_MAIN_MEM_OUT, mem_alloc(co * g['out_h'] * g['out_w'])
                mem_of[tout] = mm_out
            c = km_.ConvLayer(idx, flags, mm_out, kpu_of[tin], dst, ci, co, g['in_w'], g['in_h'], g['out_w'], g['out_h'], op['k'], g['pool'], zp_x, dw,
                              15 if zp_x else 0, 15, -(zp_x << 15), -(zp_w << 15), zp_x * zp_w * kk, wq, bn_mul, bn_add, shift,
                              a_start, a_mul, a_shift, a_bias)
            layers.append(c)
            kpu_of[tout], q[tout], rng[tout] = dst, (s_y, zp_y), (-zp_y * s_y, (255 - zp_y) * s_y)
            report['layers'][l.name] = dict(index=idx, s_x=s_x, zp_x=zp_x, s_w=s_w, zp_w=zp_w, s_y=s_y, zp_y=zp_y, fine_bits=p, pool=g['pool'],
                                            bn_shift=(int(shift.min()), int(shift.max())), zero_share=float((wq == zp_w).mean()),
                                            range=(lo, hi), bn_mul_min=int(np.abs(bn_mul[bn_mul != 0]).min()) if bn_mul.any() else 0)
            if delta is not None:
                report['layers'][l.name].update(bias_delta_max=float(np.abs(delta).max()) / float(1 << p), bias_limited=0)
            if tout in spec.outputs:
                n = co * g['out_h'] * g['out_w']
                d = mem_alloc(4 * n)
                layers.append(km_.MemLayer(len(layers), km_.KL_DEQUANTIZE, dict(flags=1, src=mm_out, dst=d, count=n,
                                                                                scale=float(np.float32(s_y)), bias=float(np.float32(-zp_y * s_y)))))
                out_entries[tout] = (d, 4 * n)
        elif t == ns.OP_UPSAMPLE:
            tin, tout = op['in0'], op['out']
            if tin not in mem_of:
                raise KmodelError(f'quantize: upsample reads tensor {names[tin]!r}, which is not in main memory')
            h, w, c = spec.tensors[tin]
            oh, ow, _ = spec.tensors[tout]
            d = mem_alloc(c * oh * ow)
            layers.append(km_.MemLayer(idx, km_.KL_QUANTIZED_RESIZE_NN, dict(flags=0, src=mem_of[tin], dst=d, in_w=w, in_h=h, channels=c, out_w=ow,
                                                                             out_h=oh, align=0)))
            mem_of[tout], q[tout], rng[tout] = d, q[tin], rng[tin]
        else:                                                                  # concat
            parts, tout = (op['in0'], op['in1']), op['out']
            for tin in parts:
                if tin not in mem_of:
                    raise KmodelError(f'quantize: concat reads tensor {names[tin]!r}, which is not in main memory')
            lo, hi = min(rng[tin][0] for tin in parts), max(rng[tin][1] for tin in parts)
            s_u, zp_u = qparams(lo, hi)
            ins = []
            for tin in parts:
                h, w, c = spec.tensors[tin]
                s_i, zp_i = q[tin]
                table = np.clip(np.rint((np.arange(256) - zp_i) * (s_i / s_u)) + zp_u, 0, 255).astype(np.uint8)
                d = mem_alloc(c * h * w)
                layers.append(km_.MemLayer(len(layers), km_.KL_REQUANTIZE, dict(flags=1, src=mem_of[tin], dst=d, count=c * h * w, table=table)))
                ins.append((d, c * h * w))
                report['requant'].append(dict(tensor=names[tin], factor=s_i / s_u, zp_in=zp_i, zp_out=zp_u))
            h, w, c = spec.tensors[tout]
            d = mem_alloc(c * h * w)
            layers.append(km_.MemLayer(len(layers), km_.KL_QUANTIZED_CONCAT, dict(flags=1, dst=d, inputs=ins)))
            up = new_buf(c, h, w, len(layers))
            layers.append(km_.MemLayer(len(layers), km_.KL_K210_UPLOAD, dict(flags=0, src=d, kpu_addr=up, width=w, height=h, channels=c)))
            kpu_of[tout], mem_of[tout], q[tout], rng[tout] = up, d, (s_u, zp_u), (-zp_u * s_u, (255 - zp_u) * s_u)
    addr = km_.allocate_kpu_ram([b['units'] for b in bufs], [b['birth'] for b in bufs], [b['death'] for b in bufs])
    for l in layers:
        if isinstance(l, km_.ConvLayer):
            l.src_addr, l.dst_addr = addr[l.src_addr], addr[l.dst_addr]
            km_.conv_registers(l)                                              # every field inside its width, or KmodelError
        elif l.type == km_.KL_K210_UPLOAD:
            l.fields['kpu_addr'] = addr[l.fields['kpu_addr']]
    missing = [names[o] for o in spec.outputs if o not in out_entries]
    if missing:
        raise KmodelError(f'quantize: network outputs {missing} are not conv outputs')
    model = km_.Kmodel(3, 0, [out_entries[o] for o in spec.outputs], layers)
    model.main_mem_usage = km_.main_mem_usage(model)
    km_.serialise(model)                                                       # the table fields too
    report['main_mem_usage'] = model.main_mem_usage
    report['kpu_ram_peak'] = max(a + b['units'] for a, b in zip(addr, bufs)) * 64
    return model, report


def format_report(report: dict) -> str:
    rows = [f"{'layer':<14}{'s_x':>11}{'zp_x':>5}{'s_w':>11}{'zp_w':>5}{'s_y':>11}{'zp_y':>5}{'p':>3}{'shift':>7}{'pool':>5}{'w==zp':>8}"]
    for name, r in report['layers'].items():
        rows.append(f"{name:<14}{r['s_x']:>11.4g}{r['zp_x']:>5}{r['s_w']:>11.4g}{r['zp_w']:>5}{r['s_y']:>11.4g}{r['zp_y']:>5}{r['fine_bits']:>3}"
                    f"{r['bn_shift'][0]:>4}-{r['bn_shift'][1]:<2}{r['pool']:>5}{100.0 * r['zero_share']:>7.2f}%")
    for r in report['requant']:
        rows.append(f"requantize {r['tensor']}: x{r['factor']:.4f}, zero point {r['zp_in']} -> {r['zp_out']}")
    for r in report.get('clipped', []):
        rows.append(f"clipped {r['tensor']} ({r['method']}): ({r['lo']:.6g}, {r['hi']:.6g}) -> ({r['new_lo']:.6g}, {r['new_hi']:.6g}), "
                    f"{100.0 * r['outside']:.4f}% of the calibration values outside")
    if report.get('equalize'):
        from . import equalize
        rows.append(equalize.format_report(report['equalize']))
    if report.get('adaround'):
        from . import adaround
        rows.append(adaround.format_report(report['adaround']))
    if report.get('biascorrect'):
        from . import biascorrect
        rows.append(biascorrect.format_report(report['biascorrect']))
    rows.append(f"main memory {report['main_mem_usage']} bytes, KPU RAM peak {report['kpu_ram_peak']} bytes")
    if report.get('qerror'):
        from . import qerror
        rows.append(qerror.format_report(report['qerror']))
    return '\n'.join(rows)


# ---- clipped calibration: a range from a histogram (host, float64, deterministic) ---------------------------------------------------------
CALIB_METHODS = ('minmax', 'percentile', 'mse')
DEFAULT_BINS = 2048
MIN_BINS, MAX_BINS = 16, 4096


def hist_inv(lo: float, hi: float, bins: int) -> np.float32:
    """The factor of the bin rule, bin(v) = trunc((v - lo) * inv) clamped to [0, bins - 1] in fp32: bins / (hi - lo) in float64, rounded to
    fp32 once; 0 for a zero-width range (everything in bin 0); +inf where the quotient exceeds fp32."""
    width = float(hi) - float(lo)
    with np.errstate(over='ignore'):
        return np.float32(bins / width) if width > 0.0 else np.float32(0.0)


def _edges(lo: float, hi: float, nb: int) -> np.ndarray:
    e = lo + np.arange(nb + 1, dtype=np.float64) * ((hi - lo) / nb)
    e[0], e[nb] = lo, hi                                                       # exactly
    return e


def _check_hist(counts, lo, hi):
    counts = np.asarray(counts)
    lo, hi = float(lo), float(hi)
    if counts.ndim != 1 or not MIN_BINS <= len(counts) <= MAX_BINS or (counts < 0).any():
        raise KmodelError(f'clip_range: a histogram is {MIN_BINS}..{MAX_BINS} non-negative counts')
    if not (np.isfinite(lo) and np.isfinite(hi)) or not lo <= 0.0 <= hi:
        raise KmodelError(f'clip_range: the histogram range ({lo}, {hi}) must be finite and contain 0')
    return counts.astype(np.float64), lo, hi


def _errors(counts: np.ndarray, mid: np.ndarray, a: np.ndarray, d: np.ndarray) -> np.ndarray:
    """err(a[k], d[k]) for every candidate k: the squared error of the uint8 code of qparams(a, d) over the bin centres, weighted by the
    counts.  Every row is reduced by the same numpy sum, so equal candidates give equal errors."""
    keep = counts > 0
    counts, mid = counts[keep], mid[keep]
    out = np.empty(len(a), np.float64)
    sz = [qparams(x, y) for x, y in zip(a, d)]
    for k0 in range(0, len(a), 256):
        s = np.array([v[0] for v in sz[k0:k0 + 256]], np.float64)[:, None]
        zp = np.array([v[1] for v in sz[k0:k0 + 256]], np.float64)[:, None]
        xq = s * (np.clip(np.rint(mid[None, :] / s) + zp, 0.0, 255.0) - zp)
        out[k0:k0 + 256] = (counts[None, :] * (mid[None, :] - xq) ** 2).sum(axis=1)
    return out


def clip_error(counts, lo: float, hi: float, a: float, d: float) -> float:
    """err(a, d) of the `mse` rule of clip_range for the histogram `counts` over [lo, hi]."""
    counts, lo, hi = _check_hist(counts, lo, hi)
    nb = len(counts)
    mid = lo + (np.arange(nb, dtype=np.float64) + 0.5) * ((hi - lo) / nb)
    return float(_errors(counts, mid, np.array([float(a)]), np.array([float(d)]))[0])


def clip_range(counts, lo: float, hi: float, method: str, percentile: float = 99.99) -> Tuple[float, float]:
    """(lo', hi') inside [lo, hi] for a tensor whose values have the histogram `counts` (NB equal bins of [lo, hi], lo <= 0 <= hi; the bin
    rule of yk_hist_f32).  Host, float64, deterministic; no GPU.  With w = (hi - lo) / NB the bin edges are e_b = lo + b w (e_0 = lo and
    e_NB = hi exactly), the centres m_b = lo + (b + 0.5) w, N the total count.

    'minmax'      (lo, hi).
    'percentile'  k = floor((1 - percentile / 100) N) values may be cut at either end: hi' = e_(j+1) for the smallest j with at most k values
                  in the bins above j, lo' = e_i for the largest i with at most k values in the bins below i; then lo' = min(lo', 0),
                  hi' = max(hi', 0).  50 < percentile <= 100; percentile = 100 is (lo, hi).
    'mse'         err(a, d) = sum_b counts[b] (m_b - x^(m_b))^2 with x^ the uint8 code of qparams(a, d) (the range widened to contain 0).
                  First d* = argmin over j = 1..NB of err(lo, e_j), the larger d on a tie; then a* = argmin over the i with e_i <= 0 of
                  err(e_i, d*), the smaller a on a tie.  err(a*, d*) <= err(lo, hi) by construction.  The search models qparams alone: the
                  upward widening quantize() applies afterwards to a LeakyReLU tensor whose zero point would exceed 127 is not in it.

    Both rules are restated from the general literature (percentile and minimum-squared-error calibrators); they are not pinned against
    nncase's or TensorRT's calibrators.  A zero-width range and an empty histogram return (lo, hi)."""
    if method not in CALIB_METHODS:
        raise KmodelError(f'clip_range: unknown method {method!r} (one of {", ".join(CALIB_METHODS)})')
    if method == 'minmax':
        return float(lo), float(hi)
    counts, lo, hi = _check_hist(counts, lo, hi)
    nb = len(counts)
    if method == 'percentile' and not 50.0 < float(percentile) <= 100.0:
        raise KmodelError(f'clip_range: percentile {percentile} outside (50, 100]')
    total = counts.sum()
    if hi == lo or total == 0 or (method == 'percentile' and float(percentile) == 100.0):
        return lo, hi
    e = _edges(lo, hi, nb)
    if method == 'percentile':
        k = np.floor((1.0 - float(percentile) / 100.0) * total)
        csum = np.concatenate([[0.0], np.cumsum(counts)])                      # csum[i] = values in the bins below i (exact: integers < 2^53)
        j = int(np.argmax(total - csum[1:] <= k))                              # values in the bins above j
        i = int(np.nonzero(csum[:nb] <= k)[0][-1])
        return min(float(e[i]), 0.0), max(float(e[j + 1]), 0.0)
    mid = lo + (np.arange(nb, dtype=np.float64) + 0.5) * ((hi - lo) / nb)
    err = _errors(counts, mid, np.full(nb, lo), e[1:])
    d = float(e[1:][nb - 1 - int(np.argmin(err[::-1]))])                       # the last of the minima: the larger d
    cand = e[:nb][e[:nb] <= 0.0]
    a = float(cand[int(np.argmin(_errors(counts, mid, cand, np.full(len(cand), d))))])    # the first of the minima: the smaller a
    return a, d


def outside_share(counts, lo: float, hi: float, new_lo: float, new_hi: float) -> float:
    """The share of a histogram's values in bins that lie wholly outside [new_lo, new_hi]."""
    counts, lo, hi = _check_hist(counts, lo, hi)
    e = _edges(lo, hi, len(counts))
    total = counts.sum()
    return float(counts[(e[1:] <= new_lo) | (e[:-1] >= new_hi)].sum() / total) if total else 0.0


# ---- calibration on the GPU -------------------------------------------------------------------------------------------------------------
class _Ranges:
    """A measure: min / max, YK_RANGE_WORDS words per slot, of every tensor - or, `per_channel`, of every output channel of
    every conv, from slot cal.ch_slot0[tensor]; the input tensor, no conv output, then goes to a last slot that nobody reads."""

    def __init__(self, cal: "Calibrator", per_channel: bool = False):
        self.cal, self.per_channel, self.n = cal, per_channel, cal.n_ch + 1 if per_channel else cal.n_slots
        self.d = cal.torch.empty(4 * self.n, dtype=cal.torch.int32, device=cal.dev)

    def clear(self):
        self.images = 0
        self.cal._ck('yk_range_reset', self.d, self.n)

    def conv(self, z, M, Cn, scale, bias, act, alpha, y, slot):
        if self.per_channel and slot:
            self.cal._ck('yk_scale_act_chrange_f32', z, M, Cn, scale, bias, act, alpha, y, self.d, self.cal.ch_slot0[slot])
        else:
            self.cal._ck('yk_scale_act_range_f32', z, M, Cn, scale, bias, act, alpha, y, self.d, self.n - 1 if self.per_channel else slot)

    def moved(self, y, slot):
        if not self.per_channel:
            self.cal._ck('yk_range_f32', y, y.numel(), self.d, slot)

    def read(self):
        return self.cal._back('yk_range_read', (self.d, self.n), (self.n, np.float32), (self.n, np.float32), (self.n, np.int32))


class _Hists:
    """uint64 counts [n_slots][bins] and a flag per slot, over the float32 spans lo .. hi (inv = bins / width) that feed_hist freezes."""

    def __init__(self, cal: "Calibrator"):
        self.cal, self.n, self.nb = cal, cal.n_slots, cal.bins
        self.d = cal.torch.empty(self.n * self.nb, dtype=cal.torch.int64, device=cal.dev)
        self.f = cal.torch.empty(self.n, dtype=cal.torch.int32, device=cal.dev)

    def clear(self):
        self.images, self.lo, self.hi, self.inv = 0, None, None, None
        self.cal._ck('yk_hist_reset', self.d, self.n, self.nb)
        self.f.zero_()

    def conv(self, z, M, Cn, scale, bias, act, alpha, y, slot):
        self.cal._ck('yk_scale_act_hist_f32', z, M, Cn, scale, bias, act, alpha, y, float(self.lo[slot]), float(self.inv[slot]), self.nb, self.d,
                     self.f, slot)

    def moved(self, y, slot):
        self.cal._ck('yk_hist_f32', y, y.numel(), float(self.lo[slot]), float(self.inv[slot]), self.nb, self.d, self.f, slot)

    def read(self):
        return self.cal._back('yk_hist_read', (self.d, self.f, self.n, self.nb), ((self.n, self.nb), np.uint64), (self.n, np.int32))


class _ChannelSums:
    """float64 sum of every output channel's pre-activation, a flag per channel, the workspace of the largest call so far, the scratch slot."""
    moved = staticmethod(lambda y, slot: None)

    def __init__(self, cal: "Calibrator"):
        self.cal, self.n, self.work = cal, cal.n_ch, None
        self.sum = cal.torch.empty(self.n, dtype=cal.torch.float64, device=cal.dev)
        self.f, self.scratch = (cal.torch.empty(n, dtype=cal.torch.int32, device=cal.dev) for n in (self.n, 4))

    def clear(self):
        self.images = 0
        self.cal._ck('yk_chsum_reset', self.sum, self.f, self.n)

    def conv(self, z, M, Cn, scale, bias, act, alpha, y, slot):
        if slot == 0:
            return self.cal._ck('yk_scale_act_range_f32', z, M, Cn, scale, bias, act, alpha, y, self.scratch, 0)
        need = C.c_size_t()
        self.cal.engine.call('yk_chsum_workspace_bytes', M, Cn, C.byref(need))
        if self.work is None or self.work.numel() * 8 < need.value:
            self.work = self.cal.torch.empty((need.value + 7) // 8, dtype=self.cal.torch.float64, device=self.cal.dev)
        self.cal._ck('yk_scale_act_chsum_f32', z, M, Cn, scale, bias, act, alpha, y, self.sum, self.f, self.cal.ch_slot0[slot], self.work)

    def read(self):
        return self.cal._back('yk_chsum_read', (self.sum, self.f, self.n), (self.n, np.float64), (self.n, np.int32))


class Calibrator:
    """The range of every tensor of `spec` over a calibration set, measured by an fp32 forward pass on the GPU.

    The pass walks the spec as train.Trainer.forward does, one device tensor per spec tensor.  Convolutions are the fp32 forward kernels of
    the training step (yk_gemm_f32 for 1x1, yk_conv3x3_bn_fwd_f32 without BatchNorm / yk_im2col3x3_f32 + yk_gemm_f32 for 3x3,
    yk_dw3x3_fwd_f32 for depthwise); inference BatchNorm (folded to scale / bias on the host) + activation + the min / max reduction are
    ONE launch of yk_scale_act_range_f32 (csrc/yk_calib.hip), so no tensor is read a second time for its range and none crosses to the host:
    `ranges()` copies 2 floats + a flag per tensor.

    `feed` normalises the uint8 frames by 255 - what the KPU sees (raw pixels, scale 1/255) - NOT by each image's own maximum as the float
    inference modes do (tools/utils.py:405).  `feed` may be called any number of times; ranges accumulate (min / max are exact and
    order-free, so the result does not depend on how the set is split into batches).

    The clipped calibrations (`ranges('percentile' | 'mse')`, clip_range) need a second pass over the same frames, `feed_hist`: the same walk
    with yk_scale_act_hist_f32 / yk_hist_f32 in place of the range launches, which count every tensor into `bins` equal bins of the range
    the first pass found (widened to contain 0, as qparams widens it).  The first `feed_hist` freezes those ranges; the counts are uint64,
    integer adds, order-free like the ranges.

    Cross-layer equalisation (equalize.py) needs the range of every CHANNEL of every conv output: `feed_channels` is the same walk with
    yk_scale_act_chrange_f32 as the epilogue, which folds channel c of a conv output into slot (the layer's first slot) + c of a second
    range buffer of sum(C over the conv outputs) slots (+ one scratch slot for the input tensor); `channel_ranges()` reads it.  It shares
    nothing with the per-tensor buffer, so `feed` / `ranges()` do not see it.  Every `feed*` is `forward`, the one walk, with its own measure."""

    def __init__(self, spec: ns.NetSpec, weights: Dict[str, np.ndarray], max_batch: int = 32, device: int = 0, bins: int = DEFAULT_BINS):
        import torch
        from . import engine
        engine.require_gpu()
        self.torch, self.engine = torch, engine
        self.spec, self.max_batch = spec, int(max_batch)
        self.dev = torch.device('cuda', device)
        self.names = tensor_names(spec)
        self.lay = {l.name: l for l in spec.layers}
        for k, op in enumerate(spec.ops):
            if op['type'] in (ns.OP_ADD, ns.OP_MAXPOOL):
                raise engine.YkError(f"Calibrator: op {k} of {spec.name} is `{_OP_NAMES[op['type']]}`, which the quantiser does not take")
            if op['type'] == ns.OP_CONV and not ((op['k'] == 1 and op['stride'] == 1) or op['k'] == 3):
                raise engine.YkError(f"Calibrator: conv {op['layer']!r}: kernel {op['k']} stride {op['stride']} has no fp32 forward kernel")
        dev = self.dev
        self.P: Dict[str, "torch.Tensor"] = {}
        for l in spec.layers:
            k = np.asarray(weights[l.name + '/kernel'], np.float32)
            k = np.transpose(k, (3, 0, 1, 2)).reshape(l.kernel_shape[3], -1) if l.kind == 'conv' else k[..., 0].reshape(9, -1)
            scale, bias = fold_bn(l, weights)
            self.P[l.name + '/w'] = torch.from_numpy(np.ascontiguousarray(k)).to(dev)
            self.P[l.name + '/scale'] = torch.from_numpy(scale.astype(np.float32)).to(dev)
            self.P[l.name + '/bias'] = torch.from_numpy(bias.astype(np.float32)).to(dev)
        self.P['input/scale'] = torch.full((3,), np.float32(INPUT_SCALE), dtype=torch.float32, device=dev)
        self.P['input/bias'] = torch.zeros(3, dtype=torch.float32, device=dev)
        self.n_slots = len(spec.tensors)
        self.bins = int(bins)
        if not MIN_BINS <= self.bins <= MAX_BINS:
            raise engine.YkError(f'Calibrator: bins = {bins} outside {MIN_BINS}..{MAX_BINS}')
        ops = [op for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)]
        ends = [sum(int(op['cout']) for op in ops[:k]) for k in range(len(ops) + 1)]                     # the first channel slot of conv k, and n_ch
        self.convs = [(op['layer'], slice(a, b), spec.tensors[op['out']]) for op, a, b in zip(ops, ends, ends[1:])]   # layer, its slots, its tensor
        self.n_ch, self.ch_slot0 = ends[-1], {op['out']: a for op, a in zip(ops, ends)}
        self._last_use = {t: k for k, op in enumerate(spec.ops) for t in _op_inputs(op)}
        self.range, self.hist, self.channels, self.means = _Ranges(self), _Hists(self), _Ranges(self, per_channel=True), _ChannelSums(self)
        self.reset()

    # the frames each measure has seen
    images, hist_images, ch_images, mean_images = (property(lambda self, m=m: getattr(self, m).images) for m in ('range', 'hist', 'channels', 'means'))

    def _ck(self, name, *args):
        """engine.call of a library function whose last parameter is the stream: torch's current one."""
        self.engine.call(name, *args, self.torch.cuda.current_stream().cuda_stream)

    def _back(self, name: str, dev: tuple, *host):
        """One synchronising copy back, `name`(*dev, *host arrays), into new numpy arrays of the (shape, dtype) pairs `host`."""
        host = tuple(np.empty(n, t) for n, t in host)
        self.torch.cuda.current_stream().synchronize()
        self.engine.call(name, *dev, *host)
        return host

    def reset(self) -> None:
        for m in (self.range, self.hist, self.channels, self.means):
            m.clear()
        self.last_clip: List[dict] = []

    def _feed(self, measure, frames_u8, keep, who: str) -> "Calibrator":
        self.forward(frames_u8, measure, keep, who)
        measure.images += int(frames_u8.shape[0])
        return self

    def _refuse_non_finite(self, bad: List[str], what: str = 'range') -> None:
        if bad:
            raise self.engine.YkError(f'Calibrator: non-finite values (NaN or infinity) in tensor(s) {", ".join(bad)}: the weights or the frames '
                                      f'are broken; no {what} is defined')

    def feed_channels(self, frames_u8, keep=None) -> "Calibrator":
        """frames_u8 as `feed` takes them: the range of every output channel of every conv layer, accumulated over calls like `feed` (and
        as independent of the batching).  Leaves the per-tensor ranges and histograms alone."""
        return self._feed(self.channels, frames_u8, keep, 'feed_channels')

    def channel_ranges(self) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        """{conv layer name: (lo[C], hi[C])} float32 over everything fed to feed_channels.  YkError naming the layer when one of its channels
        held a NaN or an infinity."""
        if not self.ch_images:
            raise self.engine.YkError('Calibrator.channel_ranges: nothing has been fed to feed_channels')
        lo, hi, fl = self.channels.read()
        self._refuse_non_finite([name for name, sl, _ in self.convs if fl[sl].any()])
        return {name: (lo[sl].copy(), hi[sl].copy()) for name, sl, _ in self.convs}

    def feed_means(self, frames_u8, keep=None) -> "Calibrator":
        """frames_u8 as `feed` takes them: the float64 sum of the fp32 PRE-activation (folded BatchNorm applied, activation not) of every output
        channel of every conv layer, accumulated over calls (yk_scale_act_chsum_f32: no floating-point atomics, the same calls give the same
        bits).  What bias correction (biascorrect.py) compares the kmodel's z against.  Leaves ranges and histograms alone."""
        return self._feed(self.means, frames_u8, keep, 'feed_means')

    def channel_means(self) -> Dict[str, Tuple[np.ndarray, int]]:
        """{conv layer name: (sum float64 [C], count)} over everything fed to feed_means; count = images x out_h x out_w of the SPEC's tensor
        (a stride-2 depthwise conv counts its half-size output).  YkError naming the layer when one of its channels held a NaN or an infinity,
        and when nothing was fed."""
        if not self.mean_images:
            raise self.engine.YkError('Calibrator.channel_means: nothing has been fed to feed_means')
        s, fl = self.means.read()
        self._refuse_non_finite([name for name, sl, _ in self.convs if fl[sl].any()], 'mean')
        return {name: (s[sl].copy(), self.mean_images * int(t[0]) * int(t[1])) for name, sl, t in self.convs}

    def feed(self, frames_u8, keep=None) -> "Calibrator":
        """frames_u8: device uint8 [B, H, W, 3], B <= max_batch, H x W = the spec's input size.  `keep`: a dict that receives every tensor
        {name: device fp32 NHWC} of this batch (tests)."""
        if self.hist.lo is not None:
            raise self.engine.YkError('Calibrator.feed: the ranges are frozen by feed_hist; reset() starts a new calibration')
        return self._feed(self.range, frames_u8, keep, 'feed')

    def feed_hist(self, frames_u8, keep=None) -> "Calibrator":
        """The second pass: `frames_u8` (as `feed` takes them - the frames the ranges came from) counted into the histogram of every tensor.
        The first call freezes the ranges fed so far, widened to contain 0, as the span of the bins.  YkError unless ranges have been fed."""
        if not self.images:
            raise self.engine.YkError('Calibrator.feed_hist: feed the ranges first (the bins span them)')
        if self.hist.lo is None:
            self.ranges()                                                                            # raises on a non-finite tensor
            lo, hi, _ = self.read()
            self.hist.lo, self.hist.hi = lo, hi = np.minimum(lo, np.float32(0)), np.maximum(hi, np.float32(0))
            self.hist.inv = np.array([hist_inv(a, b, self.bins) for a, b in zip(lo, hi)], np.float32)
        return self._feed(self.hist, frames_u8, keep, 'feed_hist')

    def frame_tensor(self, frames_u8, measure, who: str = 'forward'):
        """The input tensor of the walk, device fp32 [B, H, W, 3] = pixels / 255, made (and measured, as slot 0) by `measure.conv` from device uint8
        frames [B, H, W, 3], B <= max_batch; `who` names the caller in the refusals."""
        torch, eng = self.torch, self.engine
        H, W = self.spec.in_hw
        if not (frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and tuple(frames_u8.shape[1:]) == (H, W, 3)):
            raise eng.YkError(f'Calibrator.{who} takes device uint8 frames [B, {H}, {W}, 3]')
        B = int(frames_u8.shape[0])
        if not 1 <= B <= self.max_batch:
            raise eng.YkError(f'Calibrator.{who}: {B} frames, max_batch is {self.max_batch}')
        raw = frames_u8.contiguous().to(torch.float32)                                           # 0..255, exact
        x = torch.empty((B, H, W, 3), dtype=torch.float32, device=self.dev)
        measure.conv(raw, B * H * W, 3, self.P['input/scale'], self.P['input/bias'], ns.ACT_NONE, 0.0, x, 0)
        return x

    def conv(self, op: dict, x, B: int, measure):
        """The conv op `op` of the spec on x (device fp32 NHWC, B images) -> its output tensor: the fp32 forward launches, then `measure.conv`, which
        finishes it (folded BatchNorm, activation) and measures it."""
        new = lambda *shape: self.torch.empty(shape, dtype=self.torch.float32, device=self.dev)   # noqa: E731
        ho, wo, co = self.spec.tensors[op['out']]
        hi, wi, ci = self.spec.tensors[op['in0']]
        M = B * ho * wo
        name = op['layer']
        w = self.P[name + '/w']
        geom = [B, hi, wi, ci, ho, wo, op['stride'], op['pad_t'], op['pad_l']]
        z = new(B, ho, wo, co)
        if op['type'] == ns.OP_DWCONV:
            self._ck('yk_dw3x3_fwd_f32', x, w, *geom, z)
        elif op['k'] == 1:
            self._ck('yk_gemm_f32', 0, 1, M, co, ci, 1.0, x, ci, w, ci, 0.0, z, co)
        elif ci % 4 == 0:
            self._ck('yk_conv3x3_bn_fwd_f32', x, w, *geom, co, z, None, None, 0.0, 0, 0.0, None, None, None, None, None, 0.0, None)
        else:
            col = new(M, 9 * ci)
            self._ck('yk_im2col3x3_f32', x, *geom, col)
            self._ck('yk_gemm_f32', 0, 1, M, co, 9 * ci, 1.0, col, 9 * ci, w, 9 * ci, 0.0, z, co)
            del col
        y = new(B, ho, wo, co)
        measure.conv(z, M, co, self.P[name + '/scale'], self.P[name + '/bias'], op['act'], float(op['alpha']), y, op['out'])
        return y

    def forward(self, frames_u8, measure, keep=None, who: str = 'forward') -> None:
        """One fp32 forward pass of the spec over device uint8 frames [B, H, W, 3], B <= max_batch: `measure.conv` finishes every conv (and the
        input) and measures it, `measure.moved` measures a moved tensor.  `keep`: a dict that receives every tensor {name: device fp32 NHWC};
        `who` names the caller in the refusals."""
        torch = self.torch
        T = {0: self.frame_tensor(frames_u8, measure, who)}
        B = int(frames_u8.shape[0])
        for i, op in enumerate(self.spec.ops):
            x, t = T[op['in0']], op['type']
            if t in (ns.OP_CONV, ns.OP_DWCONV):
                y = self.conv(op, x, B, measure)
            else:
                if t == ns.OP_UPSAMPLE:                                                          # nearest x2: pure data movement
                    y = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
                else:
                    y = torch.cat([x, T[op['in1']]], dim=3)
                measure.moved(y, op['out'])
            T[op['out']] = y
            for tid in _op_inputs(op) if keep is None else ():
                if self._last_use.get(tid) == i and tid not in self.spec.outputs:
                    T.pop(tid, None)
        if keep is not None:
            keep.update({self.names[tid]: v for tid, v in T.items()})

    def read(self):
        """(min, max, flags) as numpy arrays over the spec's tensors: one device-to-host copy."""
        return self.range.read()

    def histograms(self):
        """(counts uint64 [n_slots, bins], lo, hi): the histogram of every tensor over everything fed to feed_hist, and the float32 ends of
        its bins per slot (the tensor's range widened to contain 0).  One device-to-host copy of the counts.  YkError naming the layer when
        a tensor held a NaN or an infinity."""
        if not self.hist_images:
            raise self.engine.YkError('Calibrator.histograms: nothing has been fed to feed_hist')
        counts, fl = self.hist.read()
        self._refuse_non_finite([self.names[i] for i in np.flatnonzero(fl)])
        return counts, self.hist.lo.copy(), self.hist.hi.copy()

    def ranges(self, method: str = 'minmax', percentile: float = 99.99) -> Dict[str, Tuple[float, float]]:
        """{tensor name: (min, max)} over everything fed so far.  YkError naming the layer when a tensor held a NaN or an infinity.
        method 'percentile' / 'mse': every tensor but the input (always the raw pixel) clipped by clip_range from its histogram, which
        feed_hist must have been given the same frames; an end the rule leaves where it was keeps its measured value.  `last_clip` then
        lists every conv output the rule moved (format_report prints it)."""
        if not self.images:
            raise self.engine.YkError('Calibrator.ranges: nothing has been fed')
        if method not in CALIB_METHODS:
            raise self.engine.YkError(f'Calibrator.ranges: unknown method {method!r} (one of {", ".join(CALIB_METHODS)})')
        lo, hi, fl = self.read()
        self._refuse_non_finite([self.names[i] for i in np.flatnonzero(fl)])
        out = {self.names[i]: (float(lo[i]), float(hi[i])) for i in range(self.n_slots)}
        self.last_clip = []
        if method == 'minmax':
            return out
        if self.hist_images != self.images:
            raise self.engine.YkError(f'Calibrator.ranges({method!r}): feed_hist has seen {self.hist_images} of the {self.images} frames the '
                                      f'ranges came from')
        counts, blo, bhi = self.histograms()
        for i in range(1, self.n_slots):
            try:
                a, d = clip_range(counts[i], blo[i], bhi[i], method, percentile)
            except KmodelError as e:
                raise self.engine.YkError(f'Calibrator.ranges: {e}') from e
            if (a, d) == (float(blo[i]), float(bhi[i])):
                continue
            name = self.names[i]
            new = (out[name][0] if a == float(blo[i]) else a, out[name][1] if d == float(bhi[i]) else d)
            if name in self.lay:
                self.last_clip.append(dict(tensor=name, method=method, lo=out[name][0], hi=out[name][1], new_lo=new[0], new_hi=new[1],
                                           outside=outside_share(counts[i], blo[i], bhi[i], a, d)))
            out[name] = new
        return out


def synthetic_frames(n: int, in_hw, seed: int) -> np.ndarray:
    """`n` generated calibration frames, uint8 [n, H, W, 3], every one with maximum 255 (so the float modes, which divide by the image's
    maximum, and the KPU see the same input): smooth random colour fields with rectangles, the kind of picture `make train SYNTHETIC=`
    trains on."""
    H, W = in_hw
    rng = np.random.default_rng(seed)
    out = np.empty((n, H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for i in range(n):
        img = np.zeros((H, W, 3), np.float32)
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 6.0), rng.uniform(0.5, 6.0), rng.uniform(0, 2 * np.pi)
            img[..., c] = 0.5 + 0.5 * np.sin(2 * np.pi * (fx * xx / W + fy * yy / H) + ph)
        img *= rng.uniform(0.3, 1.0, 3).astype(np.float32)
        for _ in range(int(rng.integers(1, 6))):
            h, w = int(rng.integers(H // 8, H // 2)), int(rng.integers(W // 8, W // 2))
            y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            img[y0:y0 + h, x0:x0 + w] = rng.uniform(0, 1, 3).astype(np.float32)
        img += rng.normal(0, 0.03, img.shape).astype(np.float32)
        img = np.clip(img, 0, 1)
        img /= max(float(img.max()), 1e-6)
        u8 = np.rint(img * 255).astype(np.uint8)
        u8[tuple(int(v) for v in np.unravel_index(int(np.argmax(u8)), u8.shape))] = 255
        out[i] = u8
    return out


def check_method(method: str, percentile: float, bins: int) -> None:
    """KmodelError for a calibration method, percentile or bin count the quantiser does not take."""
    for argument, ok, why in (('method', method in CALIB_METHODS, f'unknown calibration method {method!r} (one of {", ".join(CALIB_METHODS)})'),
                              ('percentile', 50.0 < float(percentile) <= 100.0, f'calibration percentile {percentile} outside (50, 100]'),
                              ('bins', MIN_BINS <= int(bins) <= MAX_BINS, f'calibration bins {bins} outside {MIN_BINS}..{MAX_BINS}')):
        if not ok:
            e = KmodelError(why)
            e.argument = argument                                                # for a caller that words the refusal itself (make_kmodel.cli)
            raise e


def device_batches(frames_u8, batch: int):
    """`frames_u8` (uint8 [N, H, W, 3], host numpy or a device tensor) in device batches of `batch`."""
    import torch
    frames = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    for i in range(0, len(frames), batch):
        yield frames[i:i + batch].cuda()


def calibrate(spec: ns.NetSpec, weights, frames_u8, batch: int = 32, method: str = 'minmax', percentile: float = 99.99,
              bins: int = DEFAULT_BINS, clipped: Optional[List[dict]] = None) -> Dict[str, Tuple[float, float]]:
    """Ranges of `frames_u8` (uint8 [N, H, W, 3], host numpy or a device tensor) in batches of `batch`.  A method other than 'minmax' walks
    the frames a second time for the histograms (`bins` bins per tensor) and clips every range by clip_range; `clipped`, a list, receives
    Calibrator.last_clip.  The input tensor's range is the raw pixel's whatever the method."""
    from . import engine
    try:
        check_method(method, percentile, bins)
    except KmodelError as e:
        raise engine.YkError(f'calibrate: {e}') from e
    cal = Calibrator(spec, weights, max_batch=max(1, min(int(batch), len(frames_u8))), bins=bins)
    for feed in (cal.feed, cal.feed_hist)[:1 if method == 'minmax' else 2]:
        for fr in device_batches(frames_u8, cal.max_batch):
            feed(fr)
    out = cal.ranges(method, percentile)
    if clipped is not None:
        clipped.extend(cal.last_clip)
    return out


def calibrate_channels(spec: ns.NetSpec, weights, frames_u8, batch: int = 32) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """{conv layer name: (lo[C], hi[C])} of `frames_u8` (as `calibrate` takes them) in batches of `batch`: what equalize.equalize needs."""
    cal = Calibrator(spec, weights, max_batch=max(1, min(int(batch), len(frames_u8))))
    for fr in device_batches(frames_u8, cal.max_batch):
        cal.feed_channels(fr)
    return cal.channel_ranges()


def calibrate_means(spec: ns.NetSpec, weights, frames_u8, batch: int = 32) -> Dict[str, Tuple[np.ndarray, int]]:
    """{conv layer name: (sum float64 [C], count)} of the pre-activations over `frames_u8` (as `calibrate` takes them) in batches of `batch`:
    what biascorrect.correct needs."""
    cal = Calibrator(spec, weights, max_batch=max(1, min(int(batch), len(frames_u8))))
    for fr in device_batches(frames_u8, cal.max_batch):
        cal.feed_means(fr)
    return cal.channel_means()
