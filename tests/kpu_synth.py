"""Small synthetic kmodels for the KPU-exact kernels (csrc/yk_kpu.hip): a builder that turns a list of layer descriptions into a
`kmodel.Kmodel`, and the models tests/test_kpu_synth.py (CPU) and tests/test_gpu_kpu_shapes.py (GPU) share.  A helper, not a test.

The builder allocates distinct KPU-RAM and main-memory addresses, fills `out_h` / `out_w` from the pool type and draws the register
fields at random inside their bit widths - but CALIBRATED on the test's own noise frame, because naive random tables saturate: it
computes the layer's `acc` and `z` here in numpy (`conv_z`, a restatement of the formula that never calls `kpu_ref.conv`), centres
`acc` with `arg_add` and `z` per channel with `bn_add`, spreads the sixteen `act_start` over the observed `z` range and picks
`act_mul` / `act_shift` / `act_bias` so that the segments cover 0..255.  It only picks constants: every expected output of a test comes
from `oracle/kpu_ref.run`.  `check_live` is the condition the inputs must meet (asserted at build time and by the CPU test), so that no
comparison can pass on a saturated layer."""
import functools

import numpy as np

from k210_yolo_framework_amd import kmodel as km_
from oracle import kpu_ref


# ---- layer descriptions ---------------------------------------------------------------------------------------------------------------
def conv(out_ch=None, k=3, dw=False, s2=False, pad=None, mem=None, src=None, weights='random', identity=False):
    """A KPU conv: dense (out_ch) or depthwise (dw), k 1 / 3, s2 = pool `left_top_2_s2`, pad = pad_value (None: random), mem = name of
    the main-memory tensor it also writes, src = name of an uploaded tensor it reads (default: the previous conv's KPU output),
    weights 'random' / 0 / 255.  identity: y = x through a 15-segment table (1x1, one channel), for a test that dictates the bytes."""
    return dict(op='conv', out_ch=out_ch, k=k, dw=dw, s2=s2, pad=pad, mem=mem, src=src, weights=weights, identity=identity)


def dequant(src, scale, bias):
    """DEQUANTIZE of main-memory tensor `src`; every one is a model output, in order."""
    return dict(op='dequant', src=src, scale=scale, bias=bias)


def requant(src, name, table):
    return dict(op='requant', src=src, name=name, table=np.asarray(table, np.uint8))


def resize(src, name, oh, ow):
    return dict(op='resize', src=src, name=name, oh=oh, ow=ow)


def concat(srcs, name):
    return dict(op='concat', srcs=list(srcs), name=name)


def upload(src, name):
    return dict(op='upload', src=src, name=name)


# ---- the arithmetic, restated (calibration and the segment count only) -----------------------------------------------------------------
def conv_z(c, x):
    """z of conv `c` at full resolution for x uint8 [N][C][H][W] -> int64 [N][OC][H][W]: tap by tap, independent of kpu_ref.conv."""
    x = np.asarray(x, np.int64)
    n, ch, h, w = x.shape
    k = c.ksize
    p = (k - 1) // 2
    xp = np.full((n, ch, h + 2 * p, w + 2 * p), int(c.pad_value), np.int64)
    xp[:, :, p:p + h, p:p + w] = x
    wt = np.asarray(c.weights, np.int64)                                          # [oc][ic|1][kk]
    sum_xw = np.zeros((n, c.out_ch, h, w), np.int64)
    sum_x = np.zeros((n, ch if c.depthwise else 1, h, w), np.int64)
    for t in range(k * k):
        win = xp[:, :, t // k:t // k + h, t % k:t % k + w]
        if c.depthwise:
            sum_xw += win * wt[None, :, 0, t, None, None]
            sum_x += win
        else:
            sum_xw += np.tensordot(win, wt[:, :, t], ([1], [1])).transpose(0, 3, 1, 2)
            sum_x += win.sum(1, keepdims=True)
    sum_w = wt.reshape(c.out_ch, -1).sum(1)[None, :, None, None]
    g_ic = 1 if c.depthwise else ch
    acc = sum_xw + ((int(c.arg_x) * sum_x) >> int(c.shr_x)) + ((int(c.arg_w) * sum_w) >> int(c.shr_w)) + int(c.arg_add) * g_ic
    bc = lambda v: np.asarray(v, np.int64)[None, :, None, None]                    # noqa: E731
    return ((acc * bc(c.bn_mul)) >> bc(c.bn_shift)) + bc(c.bn_add)


def segment_of(c, z):
    s = np.zeros(z.shape, np.int64)
    for i in range(16):
        s = np.where(z > int(c.act_start[i]), i, s)
    return s


def _activate(c, z):
    s = segment_of(c, z)
    v = (z - np.asarray(c.act_start, np.int64)[s]) * np.asarray(c.act_mul, np.int64)[s]
    sh = np.asarray(c.act_shift, np.int64)[s]
    assert sh.max() < 63                                                          # the builder never draws more (kpu_ref pins the rest)
    r = v >> np.maximum(sh - 1, 0)
    r = np.where(sh > 0, np.where(r >= 0, (r + 1) >> 1, r >> 1), v)               # round half up; a negative value keeps its floor
    return np.clip(r + np.asarray(c.act_bias, np.int64)[s], 0, 255).astype(np.uint8)


def _pooled(c, t):
    return t[:, :, ::2, ::2] if c.pool_type == km_.POOL_LEFT_TOP_2_S2 else t


def conv_forward(c, x):
    """The builder's own forward of one conv, x [N][C][H][W] uint8 (to feed the next layer's calibration)."""
    return _pooled(c, _activate(c, conv_z(c, x)))


# ---- calibration ----------------------------------------------------------------------------------------------------------------------
def _calibrate(c, x, rng):
    """Fill arg_add, bn_* and the activation table of `c` from its input x [N][C][H][W] (the noise frames)."""
    g_ic = 1 if c.depthwise else c.in_ch
    c.arg_add = 0
    c.bn_mul, c.bn_add, c.bn_shift = np.ones(c.out_ch, np.int64), np.zeros(c.out_ch, np.int64), np.zeros(c.out_ch, np.int64)
    acc = _pooled(c, conv_z(c, x))                                                # with bn = identity, z is acc
    c.arg_add = int(-np.rint(acc.mean() / g_ic)) + int(rng.integers(-3, 4))       # 40-bit field: centre the accumulator
    acc = acc + c.arg_add * g_ic
    acc = acc.transpose(1, 0, 2, 3).reshape(c.out_ch, -1)
    per = acc.astype(np.float64)
    spread = np.maximum(np.maximum(per.std(1), np.abs(per).max(1) / 64.0), 1.0)
    target = np.exp2(rng.uniform(10, 20))                                         # spread of z the table is laid over
    c.bn_shift = rng.integers(0, 16, c.out_ch).astype(np.int64)
    mul = np.clip(np.rint(target * np.exp2(c.bn_shift) / spread), 1, (1 << 23) - 1).astype(np.int64)
    c.bn_mul = mul * rng.choice([-1, 1], c.out_ch)
    z0 = (acc * c.bn_mul[:, None]) >> c.bn_shift[:, None]
    c.bn_add = (-np.rint(z0.mean(1)) + np.rint(rng.uniform(-0.5, 0.5, c.out_ch) * target)).astype(np.int64)
    z = (z0 + c.bn_add[:, None]).ravel()
    # segment 0 lies below everything observed (random constants); 1..15 split the observed range into equal shares
    start = np.empty(16, np.int64)
    start[0] = -(1 << 35)
    start[1] = z.min() - 1
    if len(np.unique(z)) >= 32:
        start[2:] = np.floor(np.quantile(z, np.arange(1, 15) / 15.0)).astype(np.int64)
    else:                                 # a handful of values (a tiny layer): equal widths, so that a value is rarely a segment's end
        start[2:] = np.floor(np.linspace(float(z.min()) - 1, float(z.max()), 16)[1:15]).astype(np.int64)
    ends = np.append(start[2:], max(int(z.max()), int(start[15]) + 1))
    width = np.maximum(ends - start[1:], 1).astype(np.float64)
    mul_, shift_, bias_ = np.zeros(16, np.int64), np.zeros(16, np.int64), np.zeros(16, np.int64)
    mul_[0], shift_[0], bias_[0] = rng.integers(-(1 << 15), 1 << 15), rng.integers(20, 41), rng.integers(-128, 128)
    for s in range(1, 16):
        if rng.random() < 0.7:                                                    # rising: from an int8 bias up to (a little past) 255
            b, e = int(rng.integers(-16, 121)), int(rng.integers(180, 291))
        else:                                                                     # falling
            b, e = int(rng.integers(60, 128)), int(rng.integers(-30, 41))
        slope = (e - b) / width[s - 1]
        sh = int(np.clip(np.floor(np.log2(16000.0 / abs(slope))), 0, 40))
        mul_[s] = int(np.clip(np.rint(slope * 2.0 ** sh), -(1 << 15), (1 << 15) - 1))
        shift_[s], bias_[s] = sh, b
    c.act_start, c.act_mul, c.act_shift, c.act_bias = start, mul_, shift_, bias_


def _identity(c):
    """y = x for a 1x1 conv of one channel: weight 1, no zero points, and fifteen segments y = (z - start) + start (start <= 127)."""
    c.weights[:] = 1
    c.arg_x = c.arg_w = c.arg_add = c.shr_x = c.shr_w = 0
    c.bn_mul, c.bn_add, c.bn_shift = np.ones(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
    start = np.array([-(1 << 35)] + [8 * s - 1 for s in range(15)], np.int64)
    c.act_start, c.act_mul, c.act_shift = start, np.ones(16, np.int64), np.zeros(16, np.int64)
    c.act_bias = np.where(start < 0, -1, start).astype(np.int64)
    c.act_bias[0] = 0


# ---- the builder ----------------------------------------------------------------------------------------------------------------------
def build(descs, in_chw, frames, seed):
    """A Kmodel from layer descriptions; `frames` uint8 [N][C][H][W] are the test's inputs, frames[0] (noise) calibrates."""
    rng = np.random.default_rng(seed)
    frames = np.asarray(frames, np.uint8)
    assert frames.shape[1:] == tuple(in_chw)
    layers, outputs = [], []
    kpu_at, mem_at = 0, 0
    kpu_cur = None                        # (address, data [N][C][H][W]) of the previous conv's output
    uploaded, mem = {}, {}                # name -> (address, data)

    def main_alloc(nbytes):
        nonlocal mem_at
        a = mem_at
        mem_at += (nbytes + 7) // 8 * 8
        return a

    for d in descs:
        i = len(layers)
        if d['op'] == 'conv':
            if not layers:
                src_addr, x = 0, frames
                kpu_at = km_.kpu_tensor_units(*in_chw)
            else:
                src_addr, x = uploaded[d['src']] if d['src'] else kpu_cur
            _, ch, h, w = x.shape
            k, dw = d['k'], d['dw']
            oc = ch if dw else d['out_ch']
            oh, ow = ((h + 1) // 2, (w + 1) // 2) if d['s2'] else (h, w)
            dst_addr = kpu_at
            kpu_at += km_.kpu_tensor_units(oc, oh, ow)
            assert kpu_at <= km_.KPU_RAM_UNITS
            wshape = (oc, 1 if dw else ch, k * k)
            wt = rng.integers(0, 256, wshape, dtype=np.uint8) if isinstance(d['weights'], str) else np.full(wshape, d['weights'], np.uint8)
            shr_x, shr_w = int(rng.integers(0, 16)), int(rng.integers(0, 16))
            zp_w, zp_x = rng.uniform(64, 192, 2)                                  # zero points inside the uint8 range, never at an end
            c = km_.ConvLayer(index=i, flags=0, main_mem_out=0, src_addr=src_addr, dst_addr=dst_addr, in_ch=ch, out_ch=oc, in_w=w, in_h=h,
                              out_w=ow, out_h=oh, ksize=k, pool_type=km_.POOL_LEFT_TOP_2_S2 if d['s2'] else km_.POOL_BYPASS,
                              pad_value=int(rng.integers(0, 256)) if d['pad'] is None else int(d['pad']), depthwise=bool(dw),
                              shr_w=shr_w, shr_x=shr_x, arg_w=int(-np.rint(zp_x * 2 ** shr_w)), arg_x=int(-np.rint(zp_w * 2 ** shr_x)),
                              arg_add=0, weights=wt, bn_mul=None, bn_add=None, bn_shift=None, act_start=None, act_mul=None,
                              act_shift=None, act_bias=None)
            if d['identity']:
                assert (k, oc, ch) == (1, 1, 1)
                _identity(c)
            else:
                _calibrate(c, x[:1], rng)
            y = conv_forward(c, x)
            kpu_cur = (dst_addr, y)
            if d['mem']:
                c.flags = km_.KLF_MAIN_MEM_OUT
                c.main_mem_out = main_alloc(y[0].size)
                mem[d['mem']] = (c.main_mem_out, y)
            layers.append(c)
            continue
        if d['op'] == 'dequant':
            a, x = mem[d['src']]
            dst = main_alloc(4 * x[0].size)
            f = dict(flags=0, src=a, dst=dst, count=x[0].size, scale=float(np.float32(d['scale'])), bias=float(np.float32(d['bias'])))
            layers.append(km_.MemLayer(i, km_.KL_DEQUANTIZE, f))
            outputs.append((dst, 4 * x[0].size))
        elif d['op'] == 'requant':
            a, x = mem[d['src']]
            dst = main_alloc(x[0].size)
            layers.append(km_.MemLayer(i, km_.KL_REQUANTIZE, dict(flags=0, src=a, dst=dst, count=x[0].size, table=d['table'].copy())))
            mem[d['name']] = (dst, d['table'][x])
        elif d['op'] == 'resize':
            a, x = mem[d['src']]
            _, ch, h, w = x.shape
            oh, ow = d['oh'], d['ow']
            dst = main_alloc(ch * oh * ow)
            layers.append(km_.MemLayer(i, km_.KL_QUANTIZED_RESIZE_NN, dict(flags=0, src=a, dst=dst, in_w=w, in_h=h, channels=ch, out_w=ow,
                                                                           out_h=oh, align=0)))
            ys, xs = [yy * h // oh for yy in range(oh)], [xx * w // ow for xx in range(ow)]
            mem[d['name']] = (dst, x[:, :, ys][:, :, :, xs])
        elif d['op'] == 'concat':
            parts = [mem[s] for s in d['srcs']]
            y = np.concatenate([p for _, p in parts], 1)
            dst = main_alloc(y[0].size)
            layers.append(km_.MemLayer(i, km_.KL_QUANTIZED_CONCAT, dict(flags=0, dst=dst, inputs=[(a, p[0].size) for a, p in parts])))
            mem[d['name']] = (dst, y)
        elif d['op'] == 'upload':
            a, x = mem[d['src']]
            _, ch, h, w = x.shape
            addr = kpu_at
            kpu_at += km_.kpu_tensor_units(ch, h, w)
            assert kpu_at <= km_.KPU_RAM_UNITS
            layers.append(km_.MemLayer(i, km_.KL_K210_UPLOAD, dict(flags=0, src=a, kpu_addr=addr, width=w, height=h, channels=ch)))
            uploaded[d['name']] = (addr, x)
        else:
            raise ValueError(d['op'])
    model = km_.Kmodel(3, 0, outputs, layers)
    model.main_mem_usage = km_.main_mem_usage(model)
    check_live(model, frames[0])
    return model


# ---- the liveness condition -----------------------------------------------------------------------------------------------------------
def trace(model, frame):
    """kpu_ref.run on one CHW frame: (float outputs, {conv index: uint8 output}, {conv index: the uint8 input kpu_ref.conv was given})."""
    keep, seen = {}, {}
    orig = kpu_ref.conv

    def spy(c, x):
        seen[c.index] = x
        return orig(c, x)
    kpu_ref.conv = spy
    try:
        outs = kpu_ref.run(model, frame, keep)
    finally:
        kpu_ref.conv = orig
    return outs, keep, seen


def check_live(model, frame):
    """The condition on a test's inputs, on kpu_ref's outputs for the noise frame.  A conv layer of at least 256 output elements: at
    least half of them strictly inside (0, 255), at least 32 distinct values, at least 4 activation segments selected.  A smaller
    layer: at least a quarter of its element count distinct.  Returns {conv index: (inside fraction, distinct, segments)}."""
    _, keep, seen = trace(model, frame)
    res = {}
    for c in model.convs:
        y = keep[c.index]
        inside = float(((y > 0) & (y < 255)).mean())
        distinct = len(np.unique(y))
        segs = len(np.unique(segment_of(c, _pooled(c, conv_z(c, seen[c.index][None])))))
        res[c.index] = (inside, distinct, segs)
        if y.size >= 256:
            assert inside >= 0.5 and distinct >= 32 and segs >= 4, (c.index, y.shape, res[c.index])
        else:
            assert 4 * distinct >= y.size, (c.index, y.shape, res[c.index])
    return res


# ---- the frames and the models of the two test files ----------------------------------------------------------------------------------
def make_frames(in_chw, seed):
    """Seeded noise, all-0, all-255 and one sparse frame, uint8 [4][C][H][W]."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, in_chw, dtype=np.uint8)
    sparse = np.where(rng.random(in_chw) < 0.1, 255, 0).astype(np.uint8)
    return np.stack([noise, np.zeros(in_chw, np.uint8), np.full(in_chw, 255, np.uint8), sparse])


def fma_sensitive_dequant():
    """A float32 (scale, bias) for which rounding q*scale before adding the bias differs, for many q in 0..255, from rounding
    q*scale + bias once (what a fused multiply-add gives): (scale, bias, the q that differ)."""
    rng = np.random.default_rng(2024)
    q = np.arange(256)
    best = None
    for _ in range(200):
        scale, bias = np.float32(rng.uniform(0.01, 0.2)), np.float32(-rng.uniform(1.0, 8.0))
        twice = (q.astype(np.float32) * scale + bias).astype(np.float32)
        once = (q.astype(np.float64) * np.float64(scale) + np.float64(bias)).astype(np.float32)
        diff = np.flatnonzero(twice.view(np.uint32) != once.view(np.uint32))
        if best is None or len(diff) > len(best[2]):
            best = (scale, bias, diff)
    return best


PERMUTATION = np.random.default_rng(31).permutation(256).astype(np.uint8)
MANY_TO_ONE = (np.arange(256) // 7 * 5 % 256).astype(np.uint8)                    # 37 distinct values, seven q to each

_last = [dequant('out', 0.037, -2.5)]

# name -> (frame C, H, W), batch of one run, layer descriptions
DENSE = {
    'm1':   ((1, 1, 1), 1, [conv(3, k=3, pad=0), conv(1, k=1, mem='out')]),
    'm63':  ((3, 7, 9), 1, [conv(15, k=3, pad=255), conv(4, k=1), conv(31, k=3, mem='out')]),
    'm64':  ((16, 8, 8), 1, [conv(17, k=1), conv(32, k=3, pad=0), conv(33, k=1, mem='out')]),
    'm65':  ((24, 5, 13), 1, [conv(48, k=3, pad=255), conv(75, k=3, mem='out')]),
    'm255': ((32, 17, 15), 1, [conv(3, k=3, pad=0), conv(16, k=3), conv(1, k=1, mem='out')]),
    'm256': ((15, 8, 16), 2, [conv(24, k=1), conv(4, k=3, pad=255), conv(32, k=3, mem='out')]),
    'm257': ((17, 1, 257), 1, [conv(31, k=3), conv(75, k=1, mem='out')]),
    'm765': ((48, 17, 15), 3, [conv(32, k=1), conv(33, k=3, pad=0), conv(3, k=3, pad=255, mem='out')]),
}
_S2 = [conv(8, k=3, s2=True), conv(dw=True, k=3, s2=True), conv(6, k=1, s2=True), conv(dw=True, k=1, s2=True, mem='out')]
STRIDE2 = {f's2_{h}x{w}': ((5, h, w), 2, _S2) for h, w in ((1, 1), (1, 6), (2, 2), (5, 7), (6, 5), (13, 19))}
# M*C of the two launches: 255 / 510 (C = 1, 5), 240 / 480 (C = 16), 231 / 462 (C = 33)
DEPTHWISE = {f'dw_c{c}': ((c, h, w), 2, [conv(dw=True, k=3), conv(dw=True, k=1), conv(dw=True, k=3, pad=255, mem='out')])
             for c, h, w in ((1, 15, 17), (5, 3, 17), (16, 3, 5), (33, 1, 7))}
LAYOUT = {f'frame_c{c}': ((c, 5, 7), 2, [conv(8, k=3, mem='out')]) for c in (1, 3, 16)}
GATHER = {'gather': ((4, 7, 9), 5, [
    conv(5, k=3, mem='a'), conv(3, k=3, mem='c'), conv(16, k=1, mem='b7'),
    resize('b7', 'b3', 3, 5), requant('b3', 'b3q', MANY_TO_ONE), resize('b3q', 'b7u', 7, 9), requant('a', 'aq', PERMUTATION),
    concat(['aq', 'b7u', 'c'], 'cat'), upload('cat', 'catk'), conv(8, k=3, src='catk', mem='out'),
    dequant('out', 0.037, -2.5), dequant('cat', 0.5, -64.0)])}
DEEP = {f'deep_c{c}_w{w}': ((c, 2, 2), 1, [conv(5, k=3, weights=w, mem='out')]) for c in (768, 3072) for w in (255, 0, 'random')}
DEQUANT = {'dequant': ((1, 1, 257), 1, [conv(1, k=1, identity=True, mem='out')])}
OVER_K = ((3073, 2, 2), 1, [conv(1, k=3, mem='out')])                             # C*k*k = 27648 + 9: packs, refused at create time

FAMILIES = dict(dense=DENSE, stride2=STRIDE2, depthwise=DEPTHWISE, layout=LAYOUT, gather=GATHER, deep=DEEP, dequant=DEQUANT)
CASES = {name: spec for fam in FAMILIES.values() for name, spec in fam.items()}


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode()))


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, frames uint8 [4][C][H][W], batch) of a named case; built once per process and never changed."""
    in_chw, batch, descs = OVER_K if name == 'over_k' else CASES[name]
    frames = make_frames(in_chw, _seed(name))
    descs = list(descs)
    if name == 'dequant':
        scale, bias, _ = fma_sensitive_dequant()
        frames[0, 0, 0] = np.random.default_rng(1).permutation(257) % 256            # every q, an odd count
        descs.append(dequant('out', scale, bias))
    elif not any(d['op'] == 'dequant' for d in descs):
        descs += _last
    frames.setflags(write=False)
    return build(descs, in_chw, frames, _seed(name) + 1), frames, batch
