"""HSV colour jitter (`make train HSV=True`; not in the reference): every training frame gets its own hue rotation,
saturation gain and exposure gain - Darknet's `hue=.1 saturation=1.5 exposure=1.5` recipe (`distort_image`), the HSV jitter YOLOv4 / v5
keep beside mosaic - in Smith's hexcone HSV (A. R. Smith, "Color gamut transform pairs", SIGGRAPH 1978).  The rule is restated here from
the literature; parity with Darknet's or OpenCV's bytes is unpinned.

Draws.  Per (seed, epoch, dataset row), never from a per-process stream, like augment.py and mosaic.py: a row's jitter does not depend on
the rank, the world size, the thread pool or the batch it lands in.  One table per epoch, `np.random.default_rng([seed, epoch, 3]).random(
(n_rows, 6))`, a stream of its own beside the augmentation's `[seed, epoch, 1]` and the mosaic's `[seed, epoch, 2]`, indexed by row of the
training list; from a row's uniforms u0..u5 and HsvConfig(hue, sat, exposure, prob):
  the row is jittered iff u0 < prob; otherwise its parameters are the neutral (0, 1, 1)
  dh = hue*(2*u1 - 1)                                 turns of the hue circle, |dh| <= hue
  gs = 1 + (sat - 1)*u2,      1/gs when u3 < 0.5      Darknet's rand_scale: a gain in [1/sat, sat]
  gv = 1 + (exposure - 1)*u4, 1/gv when u5 < 0.5      likewise, in [1/exposure, exposure]
-> params [n_rows, 3] = (dh, gs, gv), float64.  0 <= hue <= 0.5, sat >= 1, exposure >= 1, 0 <= prob <= 1, all finite, or ValueError.

Pixels (`jitter_u8`; yk_hsv_jitter_u8 is the same operations in the same order on the device, bit for bit).  Float64 on the u8 values
r, g, b of one pixel, only + - * / floor min max and comparisons, one rounding per operation, in this order:
  V = max(max(r, g), b);  m = min(min(r, g), b);  d = V - m
  h = 0 when d == 0; else (g - b)/d when V == r; else 2 + (b - r)/d when V == g; else 4 + (r - g)/d         h in [-1, 5]
  h = h + 6*dh;  h = h - 6*floor(h/6);  h = 0 unless 0 <= h < 6                                             wrapped into [0, 6)
  S = d/V (0 when V == 0);  S' = min(1, S*gs);  V' = min(255, V*gv)
  i = floor(h);  f = h - i;  p = V'*(1 - S');  q = V'*(1 - S'*f);  t = V'*(1 - S'*(1 - f))
  (R, G, B) = (V',t,p) (q,V',p) (p,V',t) (p,q,V') (t,p,V') (V',p,q)  for i = 0 .. 5
  each channel min(255, floor(x + 0.5)) -> u8
Exact properties (tests/test_colour.py, on the device tests/test_gpu_colour.py): (0, 1, 1) returns every colour unchanged; dh = +-1, a whole
turn, likewise; dh = 1/3 with gains 1 maps (r, g, b) to (b, r, g) for every colour; grey stays grey for any parameters and becomes
min(255, floor(V*gv + 0.5)); gs = 0 gives V' in all three channels.  A row that is not finite or has a negative gain is refused here
(ValueError); the kernel, which does not trust its table, leaves such a row's frame untouched.

Where.  On the finished u8 frame: after the letterbox, after the `IAA=True` warp, after the mosaic, before `img / np.max(img)`.  The
padding is jittered too, as in Darknet and YOLOv5: the warp's and the letterbox's zero fill stays zero (black is a fixed point), grey
padding stays grey.  Boxes and labels do not change.  Validation is never jittered.

A consequence, documented and not fixed: the normalisation that follows divides every frame by its own maximum (utils.py:405), so on the
float training path an exposure gain that does not clip - any gain below 1 included - is cancelled up to rounding; what survives of the
exposure is clipping at 255 and rounding.  Hue and saturation are not cancelled.  The KPU path sees pixel/255, so exposure does matter
for what a kmodel sees.

Out of scope: mixup, jittering each mosaic quadrant separately, colour augmentation in detect / eval / calibration."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

NEUTRAL = (0.0, 1.0, 1.0)


class HsvConfig(NamedTuple):
    """InputPipeline(hsv=HsvConfig(...)): Darknet's hue / saturation / exposure ranges and the share of the rows that are jittered."""
    hue: float = 0.1
    sat: float = 1.5
    exposure: float = 1.5
    prob: float = 1.0


def validate(cfg: HsvConfig) -> HsvConfig:
    """The configuration as floats, or ValueError naming the field that is out of range."""
    hue, sat, exposure, prob = (float(v) for v in cfg)
    for name, v, ok, want in (('hue', hue, 0.0 <= hue <= 0.5, 'in [0, 0.5] turns'), ('sat', sat, sat >= 1.0, '>= 1'),
                              ('exposure', exposure, exposure >= 1.0, '>= 1'), ('prob', prob, 0.0 <= prob <= 1.0, 'a probability')):
        if not (math.isfinite(v) and ok):
            raise ValueError(f'HsvConfig.{name} = {v}: must be finite and {want}')
    return HsvConfig(hue, sat, exposure, prob)


def uniforms(seed: int, epoch: int, n_rows: int) -> np.ndarray:
    """The epoch's [n_rows, 6] uniforms, indexed by dataset row."""
    return np.random.default_rng([int(seed), int(epoch), 3]).random((int(n_rows), 6))


def decode(u: np.ndarray, cfg: HsvConfig = HsvConfig()) -> np.ndarray:
    """Rows of uniforms [n, 6] -> params [n, 3] = (dh, gs, gv): the module docstring's draws."""
    hue, sat, exposure, prob = validate(cfg)
    u = np.asarray(u, np.float64).reshape(-1, 6)
    dh = hue * (2.0 * u[:, 1] - 1.0)
    gs = 1.0 + (sat - 1.0) * u[:, 2]
    gs = np.where(u[:, 3] < 0.5, 1.0 / gs, gs)
    gv = 1.0 + (exposure - 1.0) * u[:, 4]
    gv = np.where(u[:, 5] < 0.5, 1.0 / gv, gv)
    on = u[:, 0] < prob
    return np.stack([np.where(on, dh, NEUTRAL[0]), np.where(on, gs, NEUTRAL[1]), np.where(on, gv, NEUTRAL[2])], 1)


def param_table(seed: int, epoch: int, n_rows: int, cfg: HsvConfig = HsvConfig()) -> np.ndarray:
    """The epoch's params [n_rows, 3] = (dh, gs, gv), float64, indexed by dataset row: the same on every rank."""
    return decode(uniforms(seed, epoch, n_rows), cfg)


def check_params(params, n: int) -> np.ndarray:
    """params as a contiguous float64 [n, 3] ((3,) is one row for every frame), or ValueError: every entry finite, no negative gain."""
    p = np.asarray(params, np.float64)
    if p.shape == (3,):
        p = np.broadcast_to(p, (int(n), 3))
    if p.shape != (int(n), 3):
        raise ValueError(f'hsv params of shape {p.shape} for {int(n)} frames: want [{int(n)}, 3] = (dh, gs, gv)')
    bad = ~np.isfinite(p).all(1) | (p[:, 1] < 0.0) | (p[:, 2] < 0.0)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f'hsv params: row {i} is {tuple(p[i])}: not finite, or a negative gain')
    return np.ascontiguousarray(p)


def jitter_u8(img_u8: np.ndarray, params) -> np.ndarray:
    """Host copy of yk_hsv_jitter_u8: u8 [H, W, 3] with params (3,), or u8 [n, H, W, 3] with params [n, 3] (or (3,) for all) -> u8 of the
    same shape.  Float64, the module docstring's operations in its order."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f'jitter_u8: {img.dtype} {img.shape}, want uint8 [H, W, 3] or [n, H, W, 3]')
    single = img.ndim == 3
    frames = img[None] if single else img
    p = check_params(params, len(frames))
    out = frames.copy()
    for k in np.nonzero((p != np.array(NEUTRAL)).any(1))[0]:          # a neutral row returns every colour unchanged anyway
        out[k] = _jitter_one(frames[k], float(p[k, 0]), float(p[k, 1]), float(p[k, 2]))
    return out[0] if single else out


def _jitter_one(frame: np.ndarray, dh: float, gs: float, gv: float) -> np.ndarray:
    x = frame.astype(np.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    V = np.maximum(np.maximum(r, g), b)
    m = np.minimum(np.minimum(r, g), b)
    d = V - m
    dd = np.where(d > 0.0, d, 1.0)                                    # (the quotient is not used where d == 0)
    h = np.where(V == r, (g - b) / dd, np.where(V == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    h = np.where(d > 0.0, h, 0.0)
    h = h + 6.0 * dh
    h = h - 6.0 * np.floor(h / 6.0)
    h = np.where((h >= 0.0) & (h < 6.0), h, 0.0)
    S = np.where(V > 0.0, d / np.where(V > 0.0, V, 1.0), 0.0)
    S2 = np.minimum(1.0, S * gs)
    V2 = np.minimum(255.0, V * gv)
    i = np.floor(h)
    f = h - i
    p = V2 * (1.0 - S2)
    q = V2 * (1.0 - S2 * f)
    t = V2 * (1.0 - S2 * (1.0 - f))
    i = i.astype(int)
    R = np.choose(i, [V2, q, p, p, t, V2])
    G = np.choose(i, [t, V2, V2, q, p, p])
    B = np.choose(i, [p, p, t, V2, V2, q])
    return np.minimum(255.0, np.floor(np.stack([R, G, B], -1) + 0.5)).astype(np.uint8)
