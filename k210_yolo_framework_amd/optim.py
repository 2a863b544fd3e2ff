"""The optional parts of the update that ends a training step (not in the reference, whose step is Keras Adam(lr, decay) and
nothing else): a learning-rate schedule with linear warmup, an exponential moving average of the weights, and global-norm gradient clipping.

This module is the statement of the rule: float64, numpy and math only, no torch, importable without a GPU.  csrc/yk_optim.hip
(yk_sumsq_f32, yk_adam_ex_f32, yk_ema_f32) and train.Trainer are held to it, through the float32 restatements at the end, which round once
per statement the way the kernels (compiled without FMA contraction) do.

  lr       host side: Trainer.apply_update passes LrSchedule.lr_at(iterations) as the launch's lr; Adam's bias correction stays as it is.
  clipping c = min(1, clip_norm / (sqrt(sum g^2) + 1e-6)) over the whole flat gradient bucket, torch.nn.utils.clip_grad_norm_'s coefficient;
           the update consumes (g * grad_scale) * c, the bucket itself is not written.
  EMA      e <- e + (1 - d) (p_new - e) after every update, d = EmaConfig.decay_at(number of updates so far, from 1): YOLOv5's ramp
           d = decay (1 - exp(-updates / tau)), so that the average is not dominated by the initial weights."""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np

KINDS = ('constant', 'cosine', 'step')


class LrSchedule:
    """lr_at(step), step = Adam's `iterations` (0 for the first update), T = total_steps, W = warmup_steps, f = final_frac:
      step < W            base (step + 1) / W                                   (linear warmup: the last warmup step runs at base)
      'constant'          base
      'cosine'            base (f + (1 - f) (1 + cos(pi (step - W) / max(T - W, 1))) / 2),  base f from step T on
      'step'              base gamma^k, k = how many of the milestones (fractions of T) satisfy step >= milestone T."""

    def __init__(self, kind: str, base_lr: float, total_steps: int, warmup_steps: int = 0, final_frac: float = 0.01,
                 milestones: Sequence[float] = (0.8, 0.9), gamma: float = 0.1):
        if kind not in KINDS:
            raise ValueError(f'lr schedule {kind!r}: choose one of ' + ', '.join(repr(k) for k in KINDS))
        if not (math.isfinite(base_lr) and base_lr > 0):
            raise ValueError(f'lr schedule: base_lr {base_lr} must be positive')
        if int(total_steps) != total_steps or total_steps < 1:
            raise ValueError(f'lr schedule: total_steps {total_steps} must be a positive number of steps')
        if int(warmup_steps) != warmup_steps or not 0 <= warmup_steps <= total_steps:
            raise ValueError(f'lr schedule: warmup_steps {warmup_steps} must lie in 0 .. total_steps ({total_steps})')
        if not 0.0 <= final_frac <= 1.0:
            raise ValueError(f'lr schedule: final_frac {final_frac} must lie in [0, 1]')
        ms = tuple(float(m) for m in milestones)
        if any(not 0.0 <= m <= 1.0 for m in ms) or list(ms) != sorted(ms):
            raise ValueError(f'lr schedule: milestones {milestones} must be ascending fractions of total_steps')
        if not (math.isfinite(gamma) and gamma > 0):
            raise ValueError(f'lr schedule: gamma {gamma} must be positive')
        self.kind, self.base_lr, self.total_steps, self.warmup_steps = kind, float(base_lr), int(total_steps), int(warmup_steps)
        self.final_frac, self.milestones, self.gamma = float(final_frac), ms, float(gamma)

    def lr_at(self, step: int) -> float:
        if step < 0:
            raise ValueError(f'lr schedule: step {step} is negative')
        base, T, W, f = self.base_lr, self.total_steps, self.warmup_steps, self.final_frac
        if step < W:
            return base * (step + 1) / W
        if self.kind == 'constant':
            return base
        if self.kind == 'cosine':
            if step >= T:
                return base * f
            return base * (f + (1.0 - f) * 0.5 * (1.0 + math.cos(math.pi * (step - W) / max(T - W, 1))))
        k = sum(1 for m in self.milestones if step >= m * T)
        return base * self.gamma ** k

    def __repr__(self):
        return (f'LrSchedule({self.kind!r}, {self.base_lr}, {self.total_steps}, warmup_steps={self.warmup_steps}, final_frac={self.final_frac}, '
                f'milestones={self.milestones}, gamma={self.gamma})')


class EmaConfig:
    """decay_at(updates) = decay (1 - exp(-updates / tau)), updates counted from 1; tau = 0: no ramp, decay from the first update on."""

    def __init__(self, decay: float = 0.9999, tau: float = 2000.0):
        if not 0.0 <= decay < 1.0:
            raise ValueError(f'ema: decay {decay} must lie in [0, 1)')
        if not (math.isfinite(tau) and tau >= 0.0):
            raise ValueError(f'ema: tau {tau} must not be negative')
        self.decay, self.tau = float(decay), float(tau)

    def decay_at(self, updates: int) -> float:
        if updates < 1:
            raise ValueError(f'ema: updates {updates} is counted from 1')
        if self.tau == 0.0:
            return self.decay
        return self.decay * (1.0 - math.exp(-updates / self.tau))

    def omd_at(self, updates: int) -> float:
        """What the kernels receive as ema_omd: 1 - decay_at(updates) formed in double, rounded once to float32."""
        return float(np.float32(1.0 - self.decay_at(updates)))

    def __repr__(self):
        return f'EmaConfig(decay={self.decay}, tau={self.tau})'


def clip_scale(sumsq: float, clip_norm: float) -> float:
    """min(1.0, clip_norm / (sqrt(sumsq) + 1e-6)): the factor on every gradient, sumsq = the sum of their squares.
    A non-finite sumsq is not special-cased, it is propagated: an infinite one gives 0.0, and the infinite gradient behind it times 0 is the NaN
    that reaches the update; a NaN one compares false, which leaves 1.0 (C's fmin does the same), and the NaN gradients behind it reach the
    update unscaled.  Either way the step does not hide what the backward pass produced."""
    return min(1.0, clip_norm / (math.sqrt(sumsq) + 1e-6))


# ------------------------------------------------------------------------------------------------ float32 restatements
# One rounding per statement, in the kernels' order (csrc/yk_optim.hip; adam_kernel of csrc/yk_train.hip in between).  numpy's float32
# divide and square root are correctly rounded, as the device's are.
_f = np.float32


def clip_coefficient_f32(sumsq: float, clip_norm: float) -> np.float32:
    """c of yk_adam_ex_f32: clip_scale in double on the float32 value of clip_norm, then one rounding to float32."""
    return _f(clip_scale(float(sumsq), float(_f(clip_norm))))


def adam_lr_t_f32(lr: float, decay: float, iterations: int, b1: float, b2: float) -> np.float32:
    """lr_t as the host code of yk_adam_f32 / yk_adam_ex_f32 forms it: in double from the float32 arguments, then cast."""
    lr, decay, b1, b2 = (float(_f(x)) for x in (lr, decay, b1, b2))
    t = float(iterations) + 1.0
    return _f(lr / (1.0 + decay * float(iterations)) * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t)))


def ema_step_f32(e, src, omd: float) -> np.ndarray:
    """e + omd * (src - e): the difference, the product and the sum each rounded to float32."""
    e, src = np.asarray(e, _f), np.asarray(src, _f)
    with np.errstate(under='ignore'):
        d = src - e
        t = _f(omd) * d
        out = e + t
    assert out.dtype == _f
    return out


def adam_ex_step_f32(p, g, m, v, lr: float, decay: float, iterations: int, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-7,
                     grad_scale: float = 1.0, c=None, ema=None, omd: float = 0.0) -> Tuple[np.ndarray, ...]:
    """One yk_adam_ex_f32 launch -> (p, m, v, ema or None).  c: the clip coefficient (clip_coefficient_f32; None = no clipping)."""
    p, g, m, v = (np.asarray(a, _f) for a in (p, g, m, v))
    lr_t, b1, b2, eps = adam_lr_t_f32(lr, decay, iterations, b1, b2), _f(b1), _f(b2), _f(eps)
    with np.errstate(under='ignore'):
        gi = g * _f(grad_scale)
        if c is not None:
            gi = gi * _f(c)
        c1 = _f(1) - b1
        mi = b1 * m
        t1 = c1 * gi
        mi = mi + t1
        c2 = _f(1) - b2
        vi = b2 * v
        t2 = c2 * gi
        t2 = t2 * gi
        vi = vi + t2
        num = lr_t * mi
        den = np.sqrt(vi)
        den = den + eps
        upd = num / den
        pn = p - upd
    assert all(a.dtype == _f for a in (gi, mi, vi, upd, pn))
    return pn, mi, vi, (None if ema is None else ema_step_f32(ema, pn, omd))
