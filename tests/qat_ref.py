"""Restatement of the quantisation-aware training rule (csrc/yk_qat.hip) for the tests - NOT the product path.

Part 1: the arithmetic in numpy float32, one rounding per operation (true division, np.rint = half to even, explicit np.float32):
        qparams32 / codes / fq / ste_mask / fq_weights / update.  The HIP kernels are compared with it bit for bit.
Part 2: `forward_train_qat`, oracle.train_ref.forward_train with fake-quant hooks at the places train.Trainer puts them, for torch
        autograd in any dtype (float64 as the arbiter of the gradients, float32 as a CPU stand-in of the GPU's forward pass).  The hook
        is a custom autograd.Function with the straight-through gradient; it can be DRIVEN by someone else's codes (the GPU's): where its
        own code differs it takes the given one and counts the element, so one rounding tie does not turn into a gradient difference -
        the callers bound how many such elements there are and how close to a tie each of them is."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from k210_yolo_framework_amd import netspec as ns
from k210_yolo_framework_amd import quantize
from oracle import train_ref

_F = np.float32


# ---- part 1: float32 numpy ------------------------------------------------------------------------------------------------------------
def qparams32(lo, hi):
    """(s, zp) as np.float32 for the range (lo, hi) widened to contain 0."""
    lo, hi = _F(lo), _F(hi)
    lo = lo if lo < 0 else _F(0)
    hi = hi if hi > 0 else _F(0)
    if hi == lo:
        return _F(_F(1) / _F(255)), _F(0)
    s = _F(_F(hi - lo) / _F(255))
    z = np.rint(_F(_F(_F(0) - lo) / s))
    return s, _F(min(max(z, _F(0)), _F(255)))


def codes(x, lo, hi) -> np.ndarray:
    """u = rint(x / s) + zp, unclamped, float32."""
    s, zp = qparams32(lo, hi)
    x = np.asarray(x, _F)
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.rint((x / s).astype(_F)) + zp).astype(_F)


def fq(x, lo, hi) -> np.ndarray:
    s, zp = qparams32(lo, hi)
    q = np.clip(codes(x, lo, hi), _F(0), _F(255))                     # (a NaN stays a NaN)
    return (s * (q - zp).astype(_F)).astype(_F)


def ste_mask(x, lo, hi) -> np.ndarray:
    u = codes(x, lo, hi)
    with np.errstate(invalid='ignore'):
        return (u >= 0) & (u <= 255)


def extremes(x):
    """(min, max) of the finite values of x as float32 in the total order -max < ... < -0.0 < +0.0 < ... < +max (the integer order of the
    sign-folded bit patterns, as the GPU reduces them), or None when there is no finite value."""
    b = np.ascontiguousarray(np.asarray(x, _F).ravel()).view(np.uint32)
    b = b[(b & np.uint32(0x7F800000)) != np.uint32(0x7F800000)]
    if not b.size:
        return None
    k = np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000))
    back = lambda v: np.array([(v ^ np.uint32(0x80000000)) if v & np.uint32(0x80000000) else ~v], np.uint32).view(_F)[0]     # noqa: E731
    return back(k.min()), back(k.max())


def fq_weights(w) -> np.ndarray:
    """A kernel over its own exact [min, max] (its finite values)."""
    w = np.asarray(w, _F)
    e = extremes(w)
    return w.copy() if e is None else fq(w, *e).reshape(w.shape)


def update(r, b, m, observe: bool):
    """One owner slot after a step: r = (lo, hi), b = the batch extremes or None."""
    if b is None:
        return _F(r[0]), _F(r[1])
    if observe:
        return _F(min(_F(r[0]), _F(b[0]))), _F(max(_F(r[1]), _F(b[1])))
    m = _F(m)
    om = _F(_F(1) - m)
    return tuple(_F(_F(m * _F(rv)) + _F(om * _F(bv))) for rv, bv in zip(r, b))


# ---- part 2: torch autograd ------------------------------------------------------------------------------------------------------------
class FakeQuantSTE(torch.autograd.Function):
    """out = s (clamp(u, 0, 255) - zp), u = rint(y / s) + zp or the driven code where the two differ; dy = dout where 0 <= u <= 255."""

    @staticmethod
    def forward(ctx, y, s, zp, drive):
        u = torch.round(y / s) + zp                                   # torch.round: half to even
        if drive is not None:
            u = torch.where(u != drive, drive, u)
        ctx.save_for_backward((u >= 0) & (u <= 255))
        return s * (u.clamp(0, 255) - zp)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask.to(g.dtype), None, None, None


def _hook(y_nchw, name, ranges, drive, record):
    lo, hi = ranges[name]
    s, zp = qparams32(lo, hi)
    d = None
    own = (torch.round(y_nchw.detach() / float(s)) + float(zp))
    if drive is not None:
        d = torch.from_numpy(np.ascontiguousarray(drive[name])).to(y_nchw.dtype).permute(0, 3, 1, 2)
    if record is not None:
        rec = dict(u=own.permute(0, 2, 3, 1).numpy().copy(), y=y_nchw.detach().permute(0, 2, 3, 1).numpy().copy(), n=own.numel(), diff=0,
                   tie_dist=0.0)
        if d is not None:
            differ = own != d
            rec['diff'] = int(differ.sum())
            if rec['diff']:
                t = (y_nchw.detach().double() / float(s))[differ]
                rec['tie_dist'] = float((t - torch.floor(t) - 0.5).abs().max())      # distance of x / s from a half-integer
        record[name] = rec
    return FakeQuantSTE.apply(y_nchw, float(s), float(zp), d)


def forward_train_qat(spec: ns.NetSpec, params: Dict[str, torch.Tensor], x_nhwc: torch.Tensor, ranges: Optional[dict], drive=None,
                      record=None, stats: dict = None, observed: dict = None):
    """train_ref.forward_train with the hooks of train.Trainer(qat=...): kernels fq'd over their own range (identity gradient), every conv
    output and every concat fake-quantised over ranges[name] (names of quantize.tensor_names).  ranges=None: no quantisation at all;
    `observed` then receives {name: (min, max)} of the conv outputs, the concats as the union of their parts."""
    lay = {l.name: l for l in spec.layers}
    names = quantize.tensor_names(spec)
    T = {0: x_nhwc.permute(0, 3, 1, 2)}
    src = {}
    for idx, op in enumerate(spec.ops):
        x = T[op['in0']]
        t = op['type']
        name = names[op['out']]
        if t in (ns.OP_CONV, ns.OP_DWCONV):
            l = lay[op['layer']]
            k = params[l.name + '/kernel']
            if ranges is not None:
                kq = torch.from_numpy(fq_weights(k.detach().numpy().astype(_F))).to(k.dtype)
                k = k + (kq - k).detach()                               # the float32 codes (held bitwise by the kernel tests), dL/dPq as dL/dP
            ho, wo, _ = spec.tensors[op['out']]
            kk, st = op['k'], op['stride']
            pb = (ho - 1) * st + kk - x.shape[2] - op['pad_t']
            pr = (wo - 1) * st + kk - x.shape[3] - op['pad_l']
            xp = F.pad(x, (op['pad_l'], max(pr, 0), op['pad_t'], max(pb, 0)))
            if t == ns.OP_CONV:
                y = F.conv2d(xp, k.permute(3, 2, 0, 1), params.get(l.name + '/bias') if l.use_bias else None, stride=st)
            else:
                y = F.conv2d(xp, k.permute(2, 3, 0, 1), None, stride=st, groups=x.shape[1])
            y = y[:, :, :ho, :wo]
            if l.bn_name:
                mu = y.mean((0, 2, 3), keepdim=True)
                var = ((y - mu) ** 2).mean((0, 2, 3), keepdim=True)
                y = (y - mu) / torch.sqrt(var + ns.BN_EPS) * params[l.bn_name + '/gamma'].view(1, -1, 1, 1) \
                    + params[l.bn_name + '/beta'].view(1, -1, 1, 1)
                if stats is not None:
                    stats[l.name + '/pre'] = y.detach().permute(0, 2, 3, 1).numpy()
            a = op['act']
            if a == ns.ACT_RELU:
                y = F.relu(y)
            elif a == ns.ACT_RELU6:
                y = torch.clamp(y, 0, 6)
            elif a == ns.ACT_LEAKY:
                y = F.leaky_relu(y, op['alpha'])
            if ranges is not None:
                y = _hook(y, name, ranges, drive, record)
            elif observed is not None:
                observed[name] = (float(y.min()), float(y.max()))
            src[op['out']] = name
        elif t == ns.OP_UPSAMPLE:
            y = F.interpolate(x, scale_factor=2, mode='nearest')
            src[op['out']] = src[op['in0']]
        elif t == ns.OP_CONCAT:
            y = torch.cat([x, T[op['in1']]], 1)
            if ranges is not None:
                y = _hook(y, name, ranges, drive, record)
            elif observed is not None:
                a_, b_ = observed[src[op['in0']]], observed[src[op['in1']]]
                observed[name] = (min(a_[0], b_[0]), max(a_[1], b_[1]))
            src[op['out']] = name
        else:
            raise ValueError(f'op type {t}: not a network the KPU path takes')
        T[op['out']] = y
    e = 5 + spec.class_num
    return [T[o].permute(0, 2, 3, 1).reshape(x_nhwc.shape[0], *spec.tensors[o][:2], spec.anchor_num, e) for o in spec.outputs]


def loss_and_grads_qat(spec, weights, x_nhwc, y_true: Sequence[np.ndarray], anchors, ranges, drive=None, record=None, dtype=torch.float64,
                       obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0):
    """-> (data loss, regulariser, gradients in Keras layout, stats with the pre-activations).  The loss is always float64."""
    trainable = [k for k in weights if not k.endswith(('/moving_mean', '/moving_variance'))]
    params = {k: torch.from_numpy(np.asarray(weights[k])).to(dtype).requires_grad_(True) for k in trainable}
    x = torch.from_numpy(np.asarray(x_nhwc)).to(dtype)
    stats = {}
    preds = forward_train_qat(spec, params, x, ranges, drive, record, stats)
    data = sum(train_ref.yolo_loss_torch(torch.from_numpy(np.asarray(yt, np.float64)), yp.double(), anchors[i], obj_thresh, iou_thresh, obj_weight,
                                         noobj_weight, wh_weight, x.shape[0]) for i, (yt, yp) in enumerate(zip(y_true, preds)))
    reg = sum(train_ref.L2_WEIGHT * (params[l.name + '/kernel'].double() ** 2).sum() for l in spec.layers
              if l.kind == 'conv' and train_ref._is_darknet_conv(l.name))
    (data + reg).backward()
    grads = {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in params.items()}
    return float(data.detach()), float(reg.detach()), grads, stats


# ---- the training forward in numpy float32 -----------------------------------------------------------------------------------------------
def forward_np32(spec: ns.NetSpec, weights, x_nhwc, ranges: Optional[dict]):
    """The forward pass of train.Trainer(qat=...) in numpy float32 (sums of taps, batch-statistics BatchNorm), a CPU stand-in for the GPU's.
    ranges=None: no quantisation -> {name: (min, max)} of the conv outputs and the concats (union of the parts).
    Otherwise -> {name: dict(y=unquantised tensor, u=codes)} of every quantised tensor, NHWC."""
    lay = {l.name: l for l in spec.layers}
    names = quantize.tensor_names(spec)
    T, src, out = {0: np.asarray(x_nhwc, _F)}, {}, {}
    for op in spec.ops:
        x, t, name = T[op['in0']], op['type'], names[op['out']]
        if t in (ns.OP_CONV, ns.OP_DWCONV):
            l = lay[op['layer']]
            k = np.asarray(weights[l.name + '/kernel'], _F)
            if ranges is not None:
                k = fq_weights(k)
            ho, wo, co = spec.tensors[op['out']]
            kk, st = op['k'], op['stride']
            xp = np.zeros((x.shape[0], (ho - 1) * st + kk, (wo - 1) * st + kk, x.shape[3]), _F)
            hh, ww = min(x.shape[1], xp.shape[1] - op['pad_t']), min(x.shape[2], xp.shape[2] - op['pad_l'])
            xp[:, op['pad_t']:op['pad_t'] + hh, op['pad_l']:op['pad_l'] + ww] = x[:, :hh, :ww]
            y = np.zeros((x.shape[0], ho, wo, co), _F)
            for dy in range(kk):
                for dx in range(kk):
                    tap = xp[:, dy:dy + (ho - 1) * st + 1:st, dx:dx + (wo - 1) * st + 1:st]
                    y += (tap @ k[dy, dx]).astype(_F) if t == ns.OP_CONV else tap * k[dy, dx, :, 0]
            if l.use_bias:
                y = y + np.asarray(weights[l.name + '/bias'], _F)
            if l.bn_name:
                mu = y.mean((0, 1, 2), dtype=_F)
                var = ((y - mu) ** 2).mean((0, 1, 2), dtype=_F)
                y = (y - mu) / np.sqrt(var + _F(ns.BN_EPS)) * np.asarray(weights[l.bn_name + '/gamma'], _F) + np.asarray(weights[l.bn_name + '/beta'], _F)
            a = op['act']
            if a == ns.ACT_RELU:
                y = np.maximum(y, _F(0))
            elif a == ns.ACT_RELU6:
                y = np.clip(y, _F(0), _F(6))
            elif a == ns.ACT_LEAKY:
                y = np.where(y >= 0, y, y * _F(op['alpha']))
            y = y.astype(_F)
        elif t == ns.OP_UPSAMPLE:
            T[op['out']], src[op['out']] = np.repeat(np.repeat(x, 2, 1), 2, 2), src[op['in0']]
            continue
        elif t == ns.OP_CONCAT:
            y = np.concatenate([x, T[op['in1']]], 3)
        else:
            raise ValueError(f'op type {t}: not a network the KPU path takes')
        src[op['out']] = name
        if ranges is None:
            out[name] = ((float(y.min()), float(y.max())) if t != ns.OP_CONCAT else
                         (min(out[src[op['in0']]][0], out[src[op['in1']]][0]), max(out[src[op['in0']]][1], out[src[op['in1']]][1])))
        else:
            out[name] = dict(y=y, u=codes(y, *ranges[name]))
            y = fq(y, *ranges[name])
        T[op['out']] = y
    return out


# ---- the seeded case of the wiring tests (CPU pre-check and GPU comparison use the same inputs) ----------------------------------------
def mini_case(seed: int, B: int = 2):
    """tests/mini_net.mini_spec at 32x32 (stem, depthwise, stride 2, upsample, concat, both heads), seeded weights, frames and labels."""
    from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
    from tests.mini_net import mini_spec
    spec = mini_spec()
    w = spec.init_weights(seed)
    h = Helper(None, 20, VOC_ANCHORS, [[32, 32]], [list(v) for v in spec.out_hw()])
    rng = np.random.default_rng(seed)
    ys = [[] for _ in spec.outputs]
    for _ in range(B):
        n = int(rng.integers(1, 4))
        boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
        for i, lab in enumerate(h.box_to_label(boxes)):
            ys[i].append(lab)
    yt = [np.stack(y).astype(np.float32) for y in ys]
    x = rng.uniform(0, 1, (B, 32, 32, 3)).astype(np.float32)
    return spec, w, h, x, yt


WIRING_SEEDS = (5, 6, 7, 8, 9, 10)   # the seeds tests/test_gpu_qat.py may compare gradients on; tests/test_qat_ref.py pre-checks every one of them
MAX_DIFF_SHARE = 0.01                # fewer than 1 % of a tensor's codes may differ between two evaluations of one forward pass ...
MAX_TIE_DIST = 255 * 1e-4            # ... and each of them within this of a rounding tie, in steps: test_gpu_train.py's forward tolerance (1e-4 of
                                     # the tensor's magnitude) over the 255 steps of the range


def check_driven(record):
    """The two conditions under which driving the float64 pass by another pass's codes hides nothing."""
    for name, r in record.items():
        assert r['diff'] < MAX_DIFF_SHARE * r['n'], (name, r['diff'], r['n'])
        assert r['tie_dist'] <= MAX_TIE_DIST, (name, r['tie_dist'])
