"""The constructed network of tests/test_equalize.py and tests/test_gpu_equalize.py, and a float64 numpy forward of a spec.  A helper,
not a test.

yolo_mobilev1 in miniature on 16x16 frames: stem conv 3x3 s2 (8 ch, LeakyReLU) -> dw (ReLU) -> pw 16 (LeakyReLU) -> dw s2 (ReLU) -> pw 24
(LeakyReLU), the head of netspec._head on (stem output, last pw): a 3x3 conv + linear output conv, and 1x1 conv -> upsample -> concat with the
stem output -> 3x3 conv + linear output conv.  So step A of equalize.py meets a depthwise reader (conv_pw_1 -> conv_dw_2), full-conv readers
(conv_dw_1 -> conv_pw_1, conv_dw_2 -> conv_pw_2, head_conv_1 -> head_conv_2, head_conv_4 -> head_conv_5), a tensor with several readers
(conv1, conv_pw_2), one read by `upsample` (head_conv_3) and the two network outputs.

The weights are netspec.init_weights with the spread per-tensor quantisation is weak at built in: the output channels of conv_pw_1 scaled by
1 .. 100 (in its BatchNorm), the channels of conv_dw_2's kernel by 1 .. 1/100, the output channels of conv_pw_2's kernel by 1 .. 1/100 with
its BatchNorm compensating; 30 % of every pointwise kernel exactly zero (pruned); channel 5 of conv_dw_1 dead (zero kernel, zero beta and
mean: its output is exactly 0)."""
import functools

import numpy as np

from k210_yolo_framework_amd import netspec as ns, quantize

HW = (16, 16)
DEAD = ('conv_dw_1', 5)


def spec():
    s = ns.NetSpec('yolo_mobilev1', HW, anchor_num=3, class_num=1)
    x = s._new_tensor(HW[0], HW[1], 3)
    x1 = x = s.conv(x, 8, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    x = s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='conv_dw_1')
    x = s.conv(x, 16, 1, act=ns.LEAKY03, name='conv_pw_1')
    x = s.dwconv(x, 2, ns.K210_S2_PAD, act=ns.RELU, name='conv_dw_2')
    x = s.conv(x, 24, 1, act=ns.LEAKY03, name='conv_pw_2')
    ns._head(s, x1, x, 16, 12, 8, 3 * 6, [0])
    return s


def weights(dtype=np.float64, seed=5):
    s = spec()
    rng = np.random.default_rng(seed)
    w = {k: np.asarray(v, np.float64) for k, v in s.init_weights(seed=seed).items()}
    spread = lambda n: 10.0 ** rng.uniform(0.0, 2.0, n)                          # noqa: E731
    g = spread(16)
    w['conv_pw_1_bn/gamma'] *= g
    w['conv_pw_1_bn/beta'] *= g
    w['conv_dw_2/kernel'] /= spread(16).reshape(1, 1, 16, 1)
    f = spread(24)
    w['conv_pw_2/kernel'] /= f
    w['conv_pw_2_bn/gamma'] *= f
    w['conv_pw_2_bn/moving_mean'] /= f
    for name in ('conv_pw_1', 'conv_pw_2'):
        k = w[name + '/kernel']
        k[rng.random(k.shape) < 0.3] = 0.0
    name, c = DEAD
    w[name + '/kernel'][:, :, c, :] = 0.0
    w[name + '_bn/beta'][c] = 0.0
    w[name + '_bn/moving_mean'][c] = 0.0
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in w.items()}


def frames(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, HW[0], HW[1], 3), dtype=np.uint8)


def _act(v, act, alpha):
    if act == ns.ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if act == ns.ACT_LEAKY:
        return np.where(v >= 0, v, v * np.float64(np.float32(alpha)))           # the slope the fp32 kernels hold
    assert act == ns.ACT_NONE
    return v


def forward(s, w, fr_u8):
    """{tensor id: float64 NHWC} of the spec on uint8 frames / 255: every op written out here (pad, taps, BatchNorm, activation)."""
    lay = {l.name: l for l in s.layers}
    T = {0: fr_u8.astype(np.float64) / 255.0}
    for op in s.ops:
        x = T[op['in0']]
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            l = lay[op['layer']]
            k, st = op['k'], op['stride']
            ho, wo, _ = s.tensors[op['out']]
            xp = np.pad(x, ((0, 0), (op['pad_t'], op.get('pad_b', op['pad_t'])), (op['pad_l'], op.get('pad_r', op['pad_l'])), (0, 0)))
            kern = np.asarray(w[l.name + '/kernel'], np.float64)
            acc = 0.0
            for ky in range(k):
                for kx in range(k):
                    win = xp[:, ky:ky + st * (ho - 1) + 1:st, kx:kx + st * (wo - 1) + 1:st, :]
                    acc = acc + (win * kern[ky, kx, :, 0] if l.kind == 'dwconv' else win @ kern[ky, kx])
            scale, bias = quantize.fold_bn(l, w)
            T[op['out']] = _act(acc * scale + bias, op['act'], op['alpha'])
        elif op['type'] == ns.OP_UPSAMPLE:
            T[op['out']] = x.repeat(2, axis=1).repeat(2, axis=2)
        else:
            assert op['type'] == ns.OP_CONCAT
            T[op['out']] = np.concatenate([x, T[op['in1']]], axis=3)
    return T


def tensor_ranges(s, T):
    names = quantize.tensor_names(s)
    return {names[i]: (float(v.min()), float(v.max())) for i, v in T.items()}


def channel_ranges(s, T):
    return {op['layer']: (T[op['out']].min(axis=(0, 1, 2)), T[op['out']].max(axis=(0, 1, 2))) for op in s.ops
            if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)}


@functools.lru_cache(maxsize=None)
def case(dtype_name='float64'):
    """(spec, weights, calibration frames, their forward) - built once per process, never changed."""
    s, w, fr = spec(), weights(np.dtype(dtype_name)), frames(8, 17)
    for v in w.values():
        v.setflags(write=False)
    fr.setflags(write=False)
    return s, w, fr, forward(s, w, fr)
