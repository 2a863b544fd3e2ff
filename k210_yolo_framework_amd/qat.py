"""Quantisation-aware fine-tuning of `make train QAT=True`: the host half.

`quantize.py` is post-training: one asymmetric uint8 (scale, zero point) per weight tensor and per activation tensor, ranges from one
calibration pass.  With `Trainer(qat=QatConfig(...))` the same codes are simulated inside the training step - every conv / depthwise
kernel over its own [min, max], every conv output (and every concat, on the union of its parts) over a range that follows the batches as
a moving average - and the backward pass takes the straight-through gradient.  This module holds the configuration and the slot table
(which tensor owns a range, which is a union); the arithmetic is HIP: csrc/yk_qat.hip, driven by train.Trainer.

  rule           quantize.qparams in float32 (one rounding per operation):  lo' = min(lo, 0), hi' = max(hi, 0);  hi' == lo': s = 1/255,
                 zp = 0;  else s = (hi' - lo') / 255, zp = clamp(rint(-lo' / s), 0, 255);  u = rint(x / s) + zp, q = clamp(u, 0, 255),
                 fq(x) = s (q - zp);  d fq / dx = 1 where 0 <= u <= 255, else 0.
  ranges         r <- momentum r + (1 - momentum) b after every step (b = the batch's own min / max of the unquantised tensor), per
                 replica like BatchNorm statistics; `Trainer.qat_observe` widens them from batches before the first step.
  slots          one per spec tensor, named by quantize.tensor_names: a conv output OWNS its range, a concat output is the UNION of its
                 parts' ranges (through `upsample`, which passes values and range on), the input frame has none.
"""
from __future__ import annotations

from typing import List, Tuple

from . import netspec as ns
from .engine import YkError

SLOT_NONE, SLOT_OWNER, SLOT_UNION = 0, 1, 2                   # YK_QAT_SLOT_* of include/yolo_hip.h


class QatConfig:
    """momentum of the range moving average (1.0 freezes the ranges).  A captured step holds it as a launch argument; changing it on a
    live Trainer makes the next step capture again."""

    def __init__(self, momentum: float = 0.99):
        self.momentum = float(momentum)
        if not 0.0 <= self.momentum <= 1.0:
            raise YkError(f'qat: momentum {momentum} must be in [0, 1]')


def slot_table(spec: ns.NetSpec) -> Tuple[List[int], List[int], List[int]]:
    """(kind, part0, part1) per spec tensor.  Refuses, through quantize.plan_convs, what the KPU path cannot express (KmodelError naming
    the op)."""
    from . import quantize
    quantize.plan_convs(spec)
    n = len(spec.tensors)
    kind, p0, p1 = [SLOT_NONE] * n, [0] * n, [0] * n
    source = list(range(n))                                    # the slot a tensor's values are quantised on
    for op in spec.ops:
        t, out = op['type'], op['out']
        if t in (ns.OP_CONV, ns.OP_DWCONV):
            kind[out] = SLOT_OWNER
        elif t == ns.OP_UPSAMPLE:
            source[out] = source[op['in0']]
        elif t == ns.OP_CONCAT:
            kind[out], p0[out], p1[out] = SLOT_UNION, source[op['in0']], source[op['in1']]
            for p in (p0[out], p1[out]):
                if kind[p] == SLOT_NONE or p >= out:
                    raise YkError(f'qat: concat input tensor {p} carries no quantised range')
    return kind, p0, p1
