"""The distillation rule (k210_yolo_framework_amd/distill.py; `make train TEACHERCKPT=`) as a torch autograd build, its
analytic gradient, and the seeded inputs the CPU and GPU tests share.  CPU only.

(a) `autograd`: the layer's loss in torch, in any dtype, differentiable in the student's outputs; the teacher is a constant.
(b) `analytic`: distill.loss_and_grad, the numpy float64 statement with the gradient written out - the form csrc/yk_distill.hip mirrors."""
import numpy as np
import torch

from k210_yolo_framework_amd import distill

TERMS = distill.TERMS


def _sp(z):
    return torch.logaddexp(z, torch.zeros((), dtype=z.dtype))        # log(1 + e^z), stable: finite at +-80, derivative sigmoid(z)


def _kl(q, p):
    s = torch.sigmoid(q)
    return s * (_sp(-p) - _sp(-q)) + (1 - s) * (_sp(p) - _sp(q))


def loss_torch(q, p, weight, batch_size):
    """q, p: [B, ..., 5 + C] tensors of one dtype -> dict of the four terms as 0-d tensors, differentiable in p."""
    k = weight / batch_size
    a = torch.sigmoid(q[..., 4:5])
    obj = _kl(q[..., 4], p[..., 4]).sum()
    cls = (a * _kl(q[..., 5:], p[..., 5:])).sum()
    box = (a * (_kl(q[..., 0:2], p[..., 0:2]) + 0.5 * (p[..., 2:4] - q[..., 2:4]) ** 2)).sum()
    return dict(total=k * (obj + cls + box), obj=k * obj, cls=k * cls, box=k * box)


def autograd(teacher, pred, weight=1.0, batch_size=None, dtype=torch.float64):
    """(a).  -> (dict of the four terms as floats, dL/dpred as float64 numpy)."""
    q = torch.from_numpy(np.asarray(teacher)).to(dtype)
    p = torch.from_numpy(np.asarray(pred)).to(dtype).requires_grad_(True)
    terms = loss_torch(q, p, weight, batch_size or p.shape[0])
    terms['total'].backward()
    return {k: float(v.detach()) for k, v in terms.items()}, p.grad.double().numpy()


def analytic(teacher, pred, weight=1.0, batch_size=None):
    """(b).  -> (dict of the four terms, dL/dpred as float64 numpy)."""
    return distill.loss_and_grad(teacher, pred, weight, batch_size)


def atol_needed(got, want, rtol=2e-5):
    """The smallest atol at which np.allclose(got, want, rtol, atol) holds."""
    return float(np.clip(np.abs(np.asarray(got, np.float64) - want) - rtol * np.abs(want), 0, None).max())


# name -> (B, h, w, A, C, batch_size, weight).  One row; the 7x10 head with a divisor that is not the number of images; 255, 256 and 257
# rows per image (one below, at and above the 256 rows of a workgroup of csrc/yk_distill.hip); 85 floats per row (no alignment of 4);
# every logit of both tensors +-80.  All others: logits uniform over +-4.
PARITY_CASES = {
    'one': (1, 1, 1, 1, 1, None, 1.0),
    'head_7x10': (4, 7, 10, 3, 20, 16, 2.5),
    'p255': (3, 1, 85, 3, 2, None, 1.0),
    'p256': (3, 1, 256, 1, 2, None, 0.5),
    'p257': (3, 1, 257, 1, 2, None, 1.0),
    'c80': (2, 3, 4, 2, 80, None, 1.0),
    'saturated': (2, 2, 3, 3, 3, None, 1.0),
}
CASE_SEEDS = {'one': 1, 'head_7x10': 2, 'p255': 3, 'p256': 4, 'p257': 5, 'c80': 6, 'saturated': 7}
ALL_PARITY = tuple(PARITY_CASES)


def parity_case(name):
    """-> (teacher, pred as float32 [B,h,w,A,5+C], dict(weight, batch_size))."""
    B, h, w, A, C, bs, weight = PARITY_CASES[name]
    rng = np.random.default_rng(CASE_SEEDS[name])
    shape = (B, h, w, A, 5 + C)
    if name == 'saturated':
        q, p = (np.where(rng.uniform(size=shape) < 0.5, -80.0, 80.0).astype(np.float32) for _ in range(2))
    else:
        q, p = (rng.uniform(-4, 4, shape).astype(np.float32) for _ in range(2))
    return q, p, dict(weight=weight, batch_size=bs)


# The gradient tolerance of tests/test_gpu_distill.py: rtol 2e-5 as in tests/test_gpu_loss.py, and an absolute term that is not a guess:
# (a) evaluated in torch float32 on the CPU on the inputs above needs, against (a) in float64 at rtol 2e-5, the atol below (the largest
# over ALL_PARITY: 1.871e-8 on `p257`, whose factor weight / batch_size is 1 / 3; tests/test_distill_ref.py measures it again and holds it
# to this figure); the kernel, another fp32 evaluation of the same expression, is given twice that.
F32_ATOL_MEASURED = 1.871e-8
