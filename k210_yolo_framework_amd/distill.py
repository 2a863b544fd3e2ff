"""Knowledge distillation on the raw outputs of the network (`make train TEACHERCKPT=...`; not in the reference): the rule,
stated once in float64 numpy, and the host-side checks.  CPU only; csrc/yk_distill.hip (yk_distill_loss_f32) is the same rule in fp32 on the GPU.

Every network of the zoo at the same image size, output size, anchor count and class count writes outputs of one shape, [B, h, w, A, 5 + C],
so the student's raw outputs are compared with the teacher's directly, no adapter layers.  Per prediction row the student's raw outputs are
p = [x, y, w, h, o, c_0..c_{C-1}], the teacher's q in the same layout; the teacher is a constant.  With sigma the sigmoid and
sp(z) = log(1 + e^z) in its stable form,

    kl(q, p) = sigma(q) (sp(-p) - sp(-q)) + (1 - sigma(q)) (sp(p) - sp(q))

is the Bernoulli KL divergence from the teacher's probability to the student's: >= 0, exactly 0 where the bits of p and q are equal, and
d kl / dp = sigma(p) - sigma(q).  With a = sigma(q_o), the teacher's objectness, a row adds

    obj = kl(q_o, p_o)
    cls = a sum_c kl(q_c, p_c)
    box = a [kl(q_x, p_x) + kl(q_y, p_y) + ((p_w - q_w)^2 + (p_h - q_h)^2) / 2]

The box term mirrors the reference loss (cross-entropy on the in-cell offset, squared error on log(w / anchor)); the scaling by `a` is the
objectness-scaled distillation of Mehta & Ozturk 2018.  Per layer L = distill_weight / batch_size * sum over rows of
(obj + cls + box), batch_size the global batch - the divisor of the detection loss - and the reported loss is {total, obj, cls, box}, each
with that factor.  There is no temperature and no objectness threshold.

Known limitation: a (p_wh - q_wh)^2 is unbounded where a teacher has wild wh logits on background cells; distill_weight = 1.0 is a
starting point, not a finding."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

TERMS = ('total', 'obj', 'cls', 'box')


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    """log(1 + e^z) as max(z, 0) + log1p(e^-|z|): finite for every finite z."""
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def kl(q, p):
    """Bernoulli KL from sigmoid(q) to sigmoid(p), elementwise, float64."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    s = sigmoid(q)
    return s * (softplus(-p) - softplus(-q)) + (1.0 - s) * (softplus(p) - softplus(q))


def loss_and_grad(teacher, pred, weight: float = 1.0, batch_size=None) -> Tuple[Dict[str, float], np.ndarray]:
    """The rule for one layer.  teacher, pred: [B, ..., 5 + C] -> ({total, obj, cls, box}, dL/dpred as float64, shape of pred)."""
    q, p = np.asarray(teacher, np.float64), np.asarray(pred, np.float64)
    if q.shape != p.shape or p.ndim < 2 or p.shape[-1] < 6:
        raise ValueError(f'distill: teacher {q.shape} and student {p.shape} outputs must have one shape [B, ..., 5 + C], C >= 1')
    k = float(weight) / float(batch_size if batch_size else p.shape[0])
    a = sigmoid(q[..., 4:5])
    ds = sigmoid(p) - sigmoid(q)
    obj = kl(q[..., 4], p[..., 4]).sum()
    cls = (a * kl(q[..., 5:], p[..., 5:])).sum()
    dwh = p[..., 2:4] - q[..., 2:4]
    box = (a * kl(q[..., 0:2], p[..., 0:2])).sum() + (a * 0.5 * dwh ** 2).sum()
    grad = a * ds
    grad[..., 2:4] = a * dwh
    grad[..., 4] = ds[..., 4]
    terms = dict(total=k * (obj + cls + box), obj=k * obj, cls=k * cls, box=k * box)
    return {n: float(v) for n, v in terms.items()}, k * grad


@dataclass
class DistillConfig:
    """What Trainer(distill=...) takes: the teacher's NetSpec and weights (Keras layout, as load_weights leaves them), the weight of the
    distillation term and the precision of the teacher's inference plan (engine.Plan)."""
    spec: object
    weights: dict
    weight: float = 1.0
    precision: str = 'f16x2'


def check_teacher(student_spec, teacher_spec, anchors) -> None:
    """Host only.  The teacher's outputs must have the student's shapes: raises engine.YkError naming the first difference among input size,
    output count, each output's h x w, anchors per layer and class count.  anchors: the run's [layers, A, 2] table."""
    from .engine import YkError
    s, t = student_spec, teacher_spec
    anchors = np.asarray(anchors)
    si, ti = tuple(int(v) for v in s.in_hw), tuple(int(v) for v in t.in_hw)
    if si != ti:
        raise YkError(f'distill: input size: the teacher takes {ti[0]} x {ti[1]}, the student {si[0]} x {si[1]}')
    so, to = [tuple(v) for v in s.out_hw()], [tuple(v) for v in t.out_hw()]
    if len(so) != len(to) or len(so) != len(anchors):
        raise YkError(f'distill: output count: the teacher has {len(to)} output layers, the student {len(so)}, the anchor table {len(anchors)}')
    for i, (a, b) in enumerate(zip(so, to)):
        if a != b:
            raise YkError(f'distill: output size: output {i} of the teacher is {b[0]} x {b[1]}, of the student {a[0]} x {a[1]}')
    if not (int(s.anchor_num) == int(t.anchor_num) == int(anchors.shape[1])):
        raise YkError(f'distill: anchor count: the teacher has {t.anchor_num} anchors per layer, the student {s.anchor_num}, '
                      f'the anchor table {anchors.shape[1]}')
    if int(s.class_num) != int(t.class_num):
        raise YkError(f'distill: class count: the teacher has {t.class_num} classes, the student {s.class_num}')
