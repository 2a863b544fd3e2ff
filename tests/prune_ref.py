"""CPU restatement of the magnitude-pruning rule (tfmot 0.1.1 PolynomialDecay + Pruning._update_mask), the checker of the HIP kernels
in csrc/yk_prune.hip and of prune.PruneSchedule.  Plain numpy and written independently of the product: the selection is a full sort of
the uint32 patterns of |w|, the schedule is spelled out a second time."""
import numpy as np

f32 = np.float32


def patterns(w) -> np.ndarray:
    """uint32 pattern of |w|: the sign bit cleared.  Orders non-negative floats (and -0.0, denormals, inf) like integers."""
    return np.ascontiguousarray(w, np.float32).view(np.uint32).ravel() & np.uint32(0x7fffffff)


def mask_of(w, k: int):
    """-> (threshold as float32, mask of w's shape, kept count): threshold = the k-th largest |w|, mask = |w| >= threshold."""
    u = patterns(w)
    assert 1 <= k <= u.size, (k, u.size)
    thr = np.sort(u)[u.size - k]
    m = u >= thr
    return np.array([thr], np.uint32).view(np.float32)[0], m.reshape(np.shape(w)), int(m.sum())


def is_update(s: int, end_step: int, frequency: int) -> bool:
    return s <= end_step and s % frequency == 0


def sparsity(s: int, initial: float, final: float, end_step: int) -> np.float32:
    p = f32(s) / f32(end_step)
    p = f32(1) if p > 1 else f32(0) if p < 0 else p
    one_minus = f32(1) - p
    return f32(initial - final) * (one_minus * one_minus * one_minus) + f32(final)      # float32 scalars: every operation rounds to float32


def keep_count(n: int, sp) -> int:
    return int(np.rint(f32(n) * (f32(1) - f32(sp))))                                     # rint: half to even
