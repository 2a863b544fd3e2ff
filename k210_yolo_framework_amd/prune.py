"""Magnitude pruning schedule of `make train PRUNE=True` (reference keras_train.py:59-71,87-90,102-107).

The reference wraps the model in `tensorflow_model_optimization.sparsity.keras.prune_low_magnitude` with a `PolynomialDecay` schedule
and runs the `UpdatePruningStep` callback.  tfmot is not vendored by the reference and not installed here, so its rule is
RESTATED from its public source (pruning_schedule.PolynomialDecay, pruning_impl.Pruning._update_mask, prune_registry) and parity with
it is unpinned.  This module is the host half: which kernels are pruned, at which steps, and how many elements
each keeps.  The arithmetic on the weights (k-th largest |w| per kernel, the mask) is HIP: csrc/yk_prune.hip, driven by train.Trainer.

  prunable set   the `kernel` of every Conv2D (`Layer.kind == 'conv'`: stem, 1x1, head 3x3, the biased output convs).  Depthwise kernels
                 (tfmot's registry lists no prunable weight for DepthwiseConv2D), biases and BatchNorm parameters are never pruned.
  update steps   s <= end_step and s % frequency == 0 (begin_step 0), s = optimizer iterations, 0 at the first step.
  sparsity(s)    final + (initial - final) * (1 - p)^3 with p = clip(s / end_step, 0, 1), every operation rounded to float32.
  keep count     k = int(rint(float32(n) * (float32(1) - sparsity))), half to even; k < 1 is refused (tfmot would gather at index -1).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .engine import YkError

_F = np.float32


def prunable_layers(spec) -> List[str]:
    """Names of the layers whose `<name>/kernel` is pruned, in NetSpec order."""
    return [l.name for l in spec.layers if l.kind == 'conv']


class PruneSchedule:
    """tfmot PolynomialDecay(initial_sparsity, final_sparsity, begin_step=0, end_step, power=3, frequency)."""

    def __init__(self, initial: float, final: float, end_step: int, frequency: int):
        self.initial, self.final, self.end_step, self.frequency = float(initial), float(final), int(end_step), int(frequency)
        for nm, v in (('initial', self.initial), ('final', self.final)):
            if not 0.0 <= v < 1.0:
                raise YkError(f'pruning: {nm} sparsity {v} must be in [0, 1)')
        if self.end_step < 1:
            raise YkError(f'pruning: end_step {end_step} must be at least 1 (prune_end_epoch x steps per epoch)')
        if self.frequency < 1:
            raise YkError(f'pruning: frequency {frequency} must be at least 1')

    def is_update(self, s: int) -> bool:
        return 0 <= s <= self.end_step and s % self.frequency == 0

    def sparsity(self, s: int) -> np.float32:
        p = min(_F(1), max(_F(0), _F(_F(s) / _F(self.end_step))))
        q = _F(_F(1) - p)
        cube = _F(_F(q * q) * q)
        return _F(_F(_F(self.initial - self.final) * cube) + _F(self.final))

    def keep_counts(self, sizes: Sequence[int], s: int) -> np.ndarray:
        """k per kernel of `sizes` elements at step s (int64).  Raises YkError where a kernel would keep nothing."""
        keep = _F(_F(1) - self.sparsity(s))
        k = np.rint(np.asarray(sizes, np.int64).astype(_F) * keep).astype(np.int64)       # np.rint: half to even, like tf.math.round
        if k.size and k.min() < 1:
            i = int(np.argmin(k))
            raise YkError(f'pruning: a kernel of {int(sizes[i])} elements keeps {int(k[i])} at sparsity {float(self.sparsity(s)):.6g} (step {s}); '
                          f'tfmot has no defined mask for k < 1')
        return k

    def check(self, sizes: Sequence[int]) -> None:
        """Refuse now what some update step would refuse: the sparsity moves monotonically from initial (s = 0) to final (s = end_step)."""
        self.keep_counts(sizes, 0)
        self.keep_counts(sizes, self.end_step)
