"""Where a kmodel loses the signal: the quantisation error of every conv layer (`make kmodel ANALYZE=True`).

The rule (numpy float64; the instrument every toolchain ships - AIMET's QuantAnalyzer, nncase's dump and compare - restated; parity with their
numbers is unpinned).  Per channel c of a conv output, over the compared positions, with

    y   the float network's tensor (fp32)
    q   the KPU's codes (uint8),   yh = float64(q - zp_y) * float64(float32(s_y))
    e   = float64(y) - yh                                              every product and difference rounded once, in float64

seven sums and one maximum are kept (`channel_sums`; yk_qerr_u8_f32 on the GPU):

    n, sum y^2, sum e^2, sum e, sum y yh, sum yh^2, the counts of q == 0 and of q == 255 (integers), max |e|

A position whose y is a NaN or an infinity enters none of them and raises the channel's flag; `analyze` refuses such a layer by name.  Derived
per channel, and per tensor from the channel sums added up (`figures`):

    SQNR in dB      10 log10(sum y^2 / sum e^2); inf when sum e^2 = 0, nan when both are 0 (a channel that is constantly zero and exact)
    cosine          sum y yh / sqrt(sum y^2 sum yh^2); nan when a factor is 0
    mean error      sum e / n / s_y, in output codes; largest error  max |e| / s_y, in output codes
    share at 0/255  count / n: codes at the flat ends of the activation table (saturation at 255, the calibrated minimum at 0)
    worst channels  the k channels of lowest SQNR, nan not ranked

Compared positions: `quantize()` runs a stride-2 depthwise conv at stride 1 and lets its 1x1 successor pool, so with step 2 float position
(oy, ox) is compared with code position (2 oy, 2 ox) (biascorrect.steps_of names those layers).

`analyze` measures every conv twice per batch of frames (pixels / 255, as the Calibrator feeds them):
  accumulated  the float network's tensor against the KPU's tensor of the same layer: what the layer hands on, everything inherited included;
  local        the float conv applied to the input the KPU layer actually saw - the producers' codes dequantised with their own (s_y, zp_y),
               moved in float through `upsample` / `concat` - against the KPU's tensor: the layer's own error.  A concat's requantisation
               onto the common range is thereby charged to the concat's READER.  The first conv reads the pixels in both walks: its two rows
               are equal bit for bit.
The float convs are the Calibrator's launches and its epilogue (Calibrator.conv); the comparison reads both tensors where they lie on the
device (engine.KpuPlan.layer_view), 5 bytes per element."""
from __future__ import annotations

import json
from typing import Dict, Optional

import numpy as np

from .kmodel import KmodelError

WORDS = 10                       # YK_QERR_WORDS: 4 integer words (n, n0, n255, flag) and 6 float64 words per slot
ADDED = ('n', 'n0', 'n255', 'syy', 'see', 'se', 'syh', 'shh')
DEFAULT_TOP = 3


def dequantise(q: np.ndarray, s_y: float, zp_y: int) -> np.ndarray:
    """yh: float64(q - zp_y) * float64(float32(s_y))."""
    return (np.asarray(q).astype(np.int64) - int(zp_y)).astype(np.float64) * float(np.float32(s_y))


def channel_sums(y: np.ndarray, q: np.ndarray, s_y: float, zp_y: int, step: int = 1) -> Dict[str, np.ndarray]:
    """The sums of the rule for y fp32 [B, ho, wo, C] against q uint8 [B, qH, qW, C] (ho = ceil(qH / step), wo = ceil(qW / step)):
    {n, n0, n255 int64 [C]; syy, see, se, syh, shh, emax float64 [C]; flag bool [C]}."""
    y, q = np.asarray(y), np.asarray(q)[:, ::step, ::step]
    if y.dtype != np.float32 or q.dtype != np.uint8 or y.ndim != 4 or y.shape != q.shape or step not in (1, 2):
        raise KmodelError(f'qerror: y {y.dtype} {y.shape} against codes {q.dtype} {q.shape} at step {step}')
    ok = np.isfinite(y)
    yd = np.where(ok, y, np.float32(0)).astype(np.float64)
    yh = np.where(ok, dequantise(q, s_y, zp_y), 0.0)
    e = yd - yh
    ax = (0, 1, 2)
    return dict(n=ok.sum(axis=ax, dtype=np.int64), n0=(ok & (q == 0)).sum(axis=ax, dtype=np.int64), n255=(ok & (q == 255)).sum(axis=ax, dtype=np.int64),
                syy=(yd * yd).sum(axis=ax), see=(e * e).sum(axis=ax), se=e.sum(axis=ax), syh=(yd * yh).sum(axis=ax), shh=(yh * yh).sum(axis=ax),
                emax=np.abs(e).max(axis=ax, initial=0.0), flag=~ok.all(axis=ax))


def add_sums(a: Dict[str, np.ndarray], b: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The sums of two sets of positions of the same channels."""
    out = {k: a[k] + b[k] for k in ADDED}
    out.update(emax=np.maximum(a['emax'], b['emax']), flag=a['flag'] | b['flag'])
    return out


def _derive(d: dict, s: float) -> dict:
    """The figures of the rule from sums (arrays over the channels, or scalars)."""
    n, syy, see = np.asarray(d['n'], np.float64), np.asarray(d['syy'], np.float64), np.asarray(d['see'], np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        sqnr = np.where(see == 0.0, np.where(syy == 0.0, np.nan, np.inf), 10.0 * np.log10(syy / np.where(see == 0.0, 1.0, see)))
        return dict(sqnr_db=sqnr, cosine=np.asarray(d['syh'], np.float64) / np.sqrt(syy * np.asarray(d['shh'], np.float64)),
                    mean_err=np.asarray(d['se'], np.float64) / n / s, max_err=np.asarray(d['emax'], np.float64) / s,
                    share_0=np.asarray(d['n0'], np.float64) / n, share_255=np.asarray(d['n255'], np.float64) / n)


def figures(sums: Dict[str, np.ndarray], s_y: float, top: int = DEFAULT_TOP) -> dict:
    """The tensor's figures from the channel sums added up (floats), `channels` = the same per channel (arrays [C]), `worst` = the `top`
    channels of lowest SQNR as (channel, dB) - nan is not ranked, the lower channel first on a tie - and `sums`, as given."""
    s = float(np.float32(s_y))
    total = {k: sums[k].sum() for k in ADDED}
    total['emax'] = sums['emax'].max(initial=0.0)
    ch = _derive(sums, s)
    out = {k: float(v) for k, v in _derive(total, s).items()}
    ranked = [int(c) for c in np.argsort(ch['sqnr_db'], kind='stable') if not np.isnan(ch['sqnr_db'][c])]
    out.update(n=int(total['n']), non_finite=bool(np.any(sums['flag'])), channels=ch, sums=sums,
               worst=[(c, float(ch['sqnr_db'][c])) for c in ranked[:max(0, int(top))]])
    return out


def sums_of_slots(counts: np.ndarray, sums: np.ndarray) -> Dict[str, np.ndarray]:
    """What yk_qerr_read returns for a layer's slots (int64 [C, 4], float64 [C, 6]) as `channel_sums` names it."""
    return dict(n=counts[:, 0].copy(), n0=counts[:, 1].copy(), n255=counts[:, 2].copy(), flag=counts[:, 3] != 0, syy=sums[:, 0].copy(),
                see=sums[:, 1].copy(), se=sums[:, 2].copy(), syh=sums[:, 3].copy(), shh=sums[:, 4].copy(), emax=sums[:, 5].copy())


LEGEND = ('quantisation error per conv (dB = 10 log10(sum y^2 / sum e^2) against the float network; acc: what the layer hands on, inherited error '
          'included; local: the float conv on the input the KPU layer saw, so a concat\'s requantisation is charged to the concat\'s reader; '
          'mean / max error in output codes; @0 / @255: share of codes at the ends)')


def _db(v: float) -> str:
    return f'{v:.2f}'


def format_report(result: dict) -> str:
    """One row per conv; `result` as `analyze` returns it."""
    rows = [LEGEND, f"{'layer':<14}{'idx':>4}{'acc dB':>9}{'local dB':>9}{'cos':>10}{'mean':>8}{'max':>8}{'@0':>8}{'@255':>8}  worst channels (local dB)"]
    for name, r in result['layers'].items():
        a, l = r['acc'], r['local']
        rows.append(f"{name:<14}{r['index']:>4}{_db(a['sqnr_db']):>9}{_db(l['sqnr_db']):>9}{a['cosine']:>10.6f}{a['mean_err']:>8.3f}{a['max_err']:>8.2f}"
                    f"{100.0 * a['share_0']:>7.2f}%{100.0 * a['share_255']:>7.2f}%  " + ', '.join(f'{c}: {_db(v)}' for c, v in l['worst']))
    rows.append(f"quantisation error measured on {result['images']} frames")
    return '\n'.join(rows)


def to_json(result: dict) -> str:
    """The table's data, and every channel's SQNR: the channel sums are left out."""
    def one(f):
        d = {k: v for k, v in f.items() if k not in ('channels', 'sums')}
        d['worst'] = [[c, v] for c, v in f['worst']]
        d['channel_sqnr_db'] = [float(v) for v in f['channels']['sqnr_db']]
        return d
    doc = dict(images=result['images'], layers={name: dict(index=r['index'], step=r['step'], s_y=r['s_y'], zp_y=r['zp_y'], acc=one(r['acc']),
                                                           local=one(r['local'])) for name, r in result['layers'].items()})
    return json.dumps(doc, indent=1).replace('NaN', 'null').replace('-Infinity', '"-inf"').replace('Infinity', '"inf"')


# ---- the walk on the GPU ------------------------------------------------------------------------------------------------------------------
class _Compare:
    """A measure for Calibrator.forward / Calibrator.conv: finishes every conv with the Calibrator's epilogue (its range goes to a scratch slot)
    and compares the result with the codes the KPU plan holds for that tensor, into YK_QERR_WORDS words per channel."""
    moved = staticmethod(lambda y, slot: None)

    def __init__(self, cal, layers: dict):
        self.cal, self.layers, self.work = cal, layers, None
        self.d = cal.torch.empty(cal.n_ch * WORDS, dtype=cal.torch.int64, device=cal.dev)
        cal._ck('yk_qerr_reset', self.d, cal.n_ch)
        self.scratch = cal.torch.zeros(4, dtype=cal.torch.int32, device=cal.dev)

    def conv(self, z, M, Cn, scale, bias, act, alpha, y, slot):
        import ctypes as C
        self.cal._ck('yk_scale_act_range_f32', z, M, Cn, scale, bias, act, alpha, y, self.scratch, 0)
        if slot == 0:
            return
        codes, qh, qw, step, s_y, zp_y = self.layers[slot]
        need = C.c_size_t()
        self.cal.engine.call('yk_qerr_workspace_bytes', M, Cn, C.byref(need))
        if self.work is None or self.work.numel() * 8 < need.value:
            self.work = self.cal.torch.empty((need.value + 7) // 8, dtype=self.cal.torch.int64, device=self.cal.dev)
        self.cal._ck('yk_qerr_u8_f32', codes, y, int(y.shape[0]), qh, qw, Cn, step, s_y, zp_y, self.d, self.cal.ch_slot0[slot], self.work)

    def read(self):
        return self.cal._back('yk_qerr_read', (self.d, self.cal.n_ch), ((self.cal.n_ch, 4), np.int64), ((self.cal.n_ch, 6), np.float64))


def analyze(spec, weights, model, report: dict, frames_u8, batch: int = 32, keep: Optional[dict] = None, top: int = DEFAULT_TOP) -> dict:
    """The quantisation error of `model` (a kmodel.Kmodel that quantize.quantize made of `spec` and `weights`, `report` its report) over
    `frames_u8` (uint8 [N, H, W, 3], host numpy or a device tensor) in batches of `batch`: {'images': N, 'layers': {conv layer name, in network
    order: dict(index = kmodel layer index, step, s_y, zp_y, acc = figures(...), local = figures(...))}}.  `keep`, a dict, receives for every
    layer and batch the float tensor, the local float tensor and a copy of the device codes: keep[name] = {'float': [...], 'local': [...],
    'codes': [...]}, one entry per batch (tests).  YkError naming the layers whose float tensor held a NaN or an infinity."""
    import torch
    from . import biascorrect, engine, netspec as ns, quantize as qz
    frames = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or len(frames) == 0:
        raise engine.YkError('qerror.analyze: frames_u8 must be uint8 [N, H, W, 3], N >= 1')
    batch = max(1, min(int(batch), len(frames)))
    cal = qz.Calibrator(spec, weights, max_batch=batch)
    steps = biascorrect.steps_of(model)
    conv_ops = [op for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)]
    producer = {op['out']: op for op in spec.ops}
    with engine.KpuPlan(model, max_batch=batch) as plan:
        layers, rows = {}, {}
        for op in conv_ops:
            r = report['layers'][op['layer']]
            view, step = plan.layer_view(r['index']), steps[r['index']]
            qh, qw = int(view.shape[1]), int(view.shape[2])
            ho, wo, co = spec.tensors[op['out']]
            if (-(-qh // step), -(-qw // step), int(view.shape[3])) != (ho, wo, co):
                raise engine.YkError(f"qerror.analyze: conv {op['layer']!r} is {qh}x{qw}x{int(view.shape[3])} at step {step} in the kmodel and "
                                     f'{ho}x{wo}x{co} in the float network: not a kmodel of this network')
            layers[op['out']] = (view, qh, qw, step, float(r['s_y']), int(r['zp_y']))
            rows[op['layer']] = dict(index=int(r['index']), step=step, s_y=float(r['s_y']), zp_y=int(r['zp_y']))
        acc, local = _Compare(cal, layers), _Compare(cal, layers)

        def seen(t: int, x0, B: int):
            """Tensor t as the KPU layers handed it on, in real units."""
            if t == 0:
                return x0
            op = producer[t]
            if op['type'] == ns.OP_UPSAMPLE:
                return seen(op['in0'], x0, B).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
            if op['type'] == ns.OP_CONCAT:
                return torch.cat([seen(op['in0'], x0, B), seen(op['in1'], x0, B)], dim=3)
            view, qh, qw, step, s_y, zp_y = layers[t]
            ho, wo, co = spec.tensors[t]
            y = torch.empty((B, ho, wo, co), dtype=torch.float32, device=cal.dev)
            cal._ck('yk_dequant_u8_f32', view, B, qh, qw, co, step, s_y, zp_y, y)
            return y

        for fr in qz.device_batches(frames, batch):
            fr = fr.contiguous()
            B = int(fr.shape[0])
            plan.run_u8(fr)
            kept = None if keep is None else {}
            cal.forward(fr, acc, kept, 'analyze')
            x0 = cal.frame_tensor(fr, local, 'analyze')
            for op in conv_ops:
                y = cal.conv(op, seen(op['in0'], x0, B), B, local)
                if keep is not None:
                    k = keep.setdefault(op['layer'], {'float': [], 'local': [], 'codes': []})
                    k['float'].append(kept[op['layer']])
                    k['local'].append(y)
                    k['codes'].append(layers[op['out']][0][:B].clone())
        got = [m.read() for m in (acc, local)]
    cal._refuse_non_finite([name for name, sl, _ in cal.convs if any(g[0][sl, 3].any() for g in got)], 'quantisation error')
    for name, sl, _ in cal.convs:
        for key, (counts, sums) in zip(('acc', 'local'), got):
            rows[name][key] = figures(sums_of_slots(counts[sl], sums[sl]), rows[name]['s_y'], top)
    return dict(images=int(len(frames)), layers=rows)
