"""Empirical bias correction of a quantised kmodel, per output channel (`make kmodel BIASCORRECT=True`).

Once a tensor's range is chosen, a systematic error is left in every conv of the kmodel: the weights are rounded to 256 codes per tensor,
`acc * bn_mul >> bn_shift` is a floor (every output element is biased downwards), and a clipped range saturates one side of a tensor.  Each
shifts the MEAN of a channel, and the shifts compound over the layers.  The KPU's arithmetic makes the correction exact:

    z = (acc * bn_mul >> bn_shift) + bn_add            bn_add an integer per output channel, z in 2^-p output steps

so adding an integer d to bn_add[c] moves every pre-activation z of channel c - and with it the channel's mean - by exactly d.

The rule (numpy float64; restated from the empirical bias correction of Nagel et al., "Data-Free Quantization through Weight Equalization and
Bias Correction", 2019, section 4.2, and Finkelstein et al., "Fighting Quantization Bias with Bias", 2019 - parity with AIMET's or nncase's
implementations is unpinned).  For the conv ops in spec order, for conv k with report entry (p, s_y):

    1. quantise with the deltas found so far;
    2. measure, on the calibration frames, zsum_c = the sum of z over the counted positions of every channel, and their count;
    3. T_c = float_sum_c / float_count * 2^p / s_y      the float network's mean pre-activation (folded BatchNorm applied, activation not), in z units;
    4. d_c = rint(T_c - zsum_c / count);
    5. d_c limited to +-255 * 2^p (a shift of more than the whole code range is meaningless; the report names every limited channel).

One pass per conv, deliberately: the network is feed-forward, so a corrected layer is never disturbed again, but it changes what its readers
see - one pass for all layers would correct them against inputs that no longer exist.  Afterwards the mean pre-activation of every unlimited
channel of every conv equals the float network's within half a unit of z: 2^-(p + 1) of an output code.

Counted positions: `quantize()` runs a stride-2 depthwise conv at stride 1 and lets its 1x1 successor pool (`left_top_2_s2`), so the KPU's tensor
is full size where the float network's is half size, and only the even positions reach a reader: `steps_of` gives such a conv step 2.

`measure(model) -> {kmodel layer index: (zsum int64 [C], count)}` is injected, so the rule runs on the CPU in tests; `gpu_measure` is the one
`save_kmodel` uses (engine.KpuPlan.run_stats_u8: the KPU-exact integer plan with the statistics kernels)."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import numpy as np

from . import kmodel as km_
from . import netspec as ns
from .kmodel import KmodelError

LIMIT_CODES = 255                # |delta| <= LIMIT_CODES * 2^p


def steps_of(model: km_.Kmodel) -> Dict[int, int]:
    """{kmodel layer index of every conv: 1 | 2}: 2 for a depthwise conv that does not pool, leaves the KPU nowhere else, and whose only reader
    is a 1x1 conv with POOL_LEFT_TOP_2_S2 reading it at the size it was written - the deferred stride 2 of quantize.plan_convs."""
    at: Dict[int, int] = {}                                # KPU address -> index of the conv whose output lies there (-1: an uploaded tensor)
    readers: Dict[int, list] = {}
    convs = {}
    first = True
    for l in model.layers:
        if isinstance(l, km_.ConvLayer):
            convs[l.index] = l
            if not first and at.get(l.src_addr, -1) >= 0:
                readers.setdefault(at[l.src_addr], []).append(l)
            first = False
            at[l.dst_addr] = l.index
        elif l.type == km_.KL_K210_UPLOAD:
            at[l.fields['kpu_addr']] = -1
    steps = {}
    for i, c in convs.items():
        r = readers.get(i, [])
        steps[i] = 2 if (c.depthwise and c.pool_type == km_.POOL_BYPASS and not c.flags & km_.KLF_MAIN_MEM_OUT and len(r) == 1
                         and not r[0].depthwise and r[0].ksize == 1 and r[0].pool_type == km_.POOL_LEFT_TOP_2_S2
                         and (r[0].in_h, r[0].in_w) == (c.out_h, c.out_w)) else 1
    return steps


def counted(model: km_.Kmodel, images: int) -> Dict[int, int]:
    """{kmodel layer index: images x ceil(out_h / step) x ceil(out_w / step)}: how many positions of a channel the statistics count."""
    st = steps_of(model)
    return {c.index: int(images) * (-(-c.out_h // st[c.index])) * (-(-c.out_w // st[c.index])) for c in model.convs}


def target(float_sum: np.ndarray, float_count: int, p: int, s_y: float) -> np.ndarray:
    """T_c: the float network's mean pre-activation in units of 2^-p output steps."""
    return np.asarray(float_sum, np.float64) / float(float_count) * float(1 << p) / float(s_y)


def mean_z(zsum: np.ndarray, count: int) -> np.ndarray:
    """zsum / count in float64 without rounding the (up to 63-bit) sums first: the integer quotient plus the remainder's share."""
    zsum = np.asarray(zsum, np.int64)
    return (zsum // count).astype(np.float64) + (zsum % count).astype(np.float64) / float(count)


def residuals(report: dict, float_means, measured) -> Dict[str, np.ndarray]:
    """{conv layer name: |zsum_c / count - T_c|} of a quantised model (its quantize() report, what `measure` returned for it)."""
    out = {}
    for name, r in report['layers'].items():
        zsum, count = measured[r['index']]
        fsum, fcount = float_means[name]
        out[name] = np.abs(mean_z(zsum, count) - target(fsum, fcount, r['fine_bits'], r['s_y']))
    return out


def correct(spec: ns.NetSpec, weights, ranges, float_means: Dict[str, Tuple[np.ndarray, int]],
            measure: Callable[[km_.Kmodel], Dict[int, Tuple[np.ndarray, int]]], weight_codes=None):
    """-> (delta {conv layer name: int64 [C]} for quantize.quantize(bn_add_delta=), report).  float_means: {conv layer name: (sum float64 [C],
    count)} of the float network's pre-activations (Calibrator.channel_means); measure: see the module's text.  report['layers'][name] =
    dict(before = the largest |mean z - T| in output codes before this layer's correction, delta_max = the largest |delta| in output codes,
    limited = [channels whose delta was limited]); report['passes'] = the number of measuring passes.  KmodelError when a layer's count
    differs from the float side's (other frames, or another geometry).  `weight_codes` (adaround.py) goes to every quantize call made here, so
    the correction is measured on the weights the file will hold."""
    from . import quantize as qz
    delta: Dict[str, np.ndarray] = {}
    rep = {'layers': {}, 'passes': 0}
    for op in spec.ops:
        if op['type'] not in (ns.OP_CONV, ns.OP_DWCONV):
            continue
        name = op['layer']
        if name not in float_means:
            raise KmodelError(f'biascorrect: no float mean for conv {name!r}')
        model, qrep = qz.quantize(spec, weights, ranges, delta, weight_codes)
        r = qrep['layers'][name]
        p = int(r['fine_bits'])
        zsum, count = measure(model)[r['index']]
        rep['passes'] += 1
        fsum, fcount = float_means[name]
        if int(count) != int(fcount) or np.shape(zsum) != np.shape(fsum):
            raise KmodelError(f'biascorrect: conv {name!r}: the kmodel counts {count} positions of {np.shape(zsum)} channels, the float network '
                              f'{fcount} of {np.shape(fsum)}: not the same frames or not the same geometry')
        diff = target(fsum, fcount, p, r['s_y']) - mean_z(zsum, int(count))
        d = np.rint(diff)
        lim = float(LIMIT_CODES << p)
        limited = np.flatnonzero(np.abs(d) > lim)
        d = np.clip(d, -lim, lim).astype(np.int64)
        delta[name] = d
        rep['layers'][name] = dict(before=float(np.abs(diff).max()) / float(1 << p), delta_max=float(np.abs(d).max()) / float(1 << p),
                                   limited=[int(c) for c in limited], fine_bits=p)
    return delta, rep


def format_report(rep: dict) -> str:
    rows = []
    for name, r in rep['layers'].items():
        rows.append(f"bias-corrected {name}: mean z off by up to {r['before']:.4f} codes before, largest delta {r['delta_max']:.4f} codes"
                    + (f", LIMITED channels {r['limited']}" if r['limited'] else ''))
    n_lim = sum(len(r['limited']) for r in rep['layers'].values())
    worst = max((r['before'] for r in rep['layers'].values()), default=0.0)
    rows.append(f"bias correction: {len(rep['layers'])} layers in {rep['passes']} passes over the calibration frames, worst channel mean was off by "
                f"{worst:.4f} codes, {n_lim} channel(s) limited to +-{LIMIT_CODES} codes")
    return '\n'.join(rows)


def gpu_measure(frames_u8, batch: int = 32) -> Callable[[km_.Kmodel], Dict[int, Tuple[np.ndarray, int]]]:
    """The `measure` of `correct` on the GPU: a KpuPlan of the model, the sums zeroed, the statistics pass over `frames_u8` (uint8 [N, H, W, 3],
    host numpy or a device tensor) in batches of `batch`."""
    import torch
    from . import engine
    frames = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    batch = max(1, min(int(batch), len(frames)))

    def measure(model):
        steps, counts = steps_of(model), counted(model, len(frames))
        with engine.KpuPlan(model, max_batch=batch) as plan:
            plan.reset_zsums()
            for i in range(0, len(frames), batch):
                plan.run_stats_u8(frames[i:i + batch].cuda().contiguous(), steps)
            sums = plan.read_zsums()
        return {i: (z, counts[i]) for i, z in sums.items()}
    return measure
