"""What tests/test_biascorrect.py (CPU) and tests/test_gpu_yolo_biascorrect.py (GPU) share: the two-scale mini network, a numpy float64 forward
that keeps every conv's PRE-activation, and a numpy `measure` for biascorrect.correct built on kpu_synth.conv_z and oracle.kpu_ref.run.
A helper, not a test."""
import functools

import numpy as np

from k210_yolo_framework_amd import biascorrect, kmodel as km_, netspec as ns, quantize
from tests import kpu_synth


def mini_spec(hw=(32, 48)):
    """Dense 3x3 stride-2 stem, depthwise + 1x1 pairs (two depthwise convs of stride 2: their pooling is deferred to the 1x1 successor), the
    upsample + concat head, two linear outputs: yolo_mobilev1 in miniature, built as tests/test_gpu_quantize.py's mini network is."""
    s = ns.NetSpec('yolo_mobilev1', hw, anchor_num=3, class_num=1)
    x = s._new_tensor(hw[0], hw[1], 3)
    x = s.conv(x, 8, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    x1 = None
    for i, (f, st) in enumerate([(16, 1), (32, 2), (32, 1), (64, 2)], start=1):
        x = s.dwconv(x, st, ns.K210_S2_PAD if st == 2 else ns.SAME3, act=ns.RELU, name=f'conv_dw_{i}')
        x = s.conv(x, f, 1, act=ns.LEAKY03, name=f'conv_pw_{i}')
        if i == 3:
            x1 = x
    ns._head(s, x1, x, 24, 16, 16, 3 * 6, [0])
    return s


def mini_frames(n, hw, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def _windows(x, k, stride, pt, pl, pb, pr):
    """x [N][H][W][C] float64 -> the k*k shifted views [k*k][N][Ho][Wo][C] of the zero-padded tensor."""
    n, h, w, c = x.shape
    xp = np.zeros((n, h + pt + pb, w + pl + pr, c), np.float64)
    xp[:, pt:pt + h, pl:pl + w] = x
    ho, wo = (h + pt + pb - k) // stride + 1, (w + pl + pr - k) // stride + 1
    return [xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(k) for kx in range(k)]


def float_means(spec, weights, frames_u8):
    """{conv layer: (sum float64 [C] of the pre-activation t = conv(x) * scale + bias, count)} of the float network in numpy float64, over
    frames uint8 [N][H][W][3] / 255."""
    lay = {l.name: l for l in spec.layers}
    T = {0: frames_u8.astype(np.float64) * quantize.INPUT_SCALE}
    out = {}
    for op in spec.ops:
        x = T[op['in0']]
        if op['type'] in (ns.OP_CONV, ns.OP_DWCONV):
            l = lay[op['layer']]
            k = op['k']
            kern = np.asarray(weights[l.name + '/kernel'], np.float64)
            win = _windows(x, k, op['stride'], op['pad_t'], op['pad_l'], op.get('pad_b', op['pad_t']), op.get('pad_r', op['pad_l']))
            if op['type'] == ns.OP_DWCONV:
                z = sum(wv * kern[t // k, t % k, :, 0] for t, wv in enumerate(win))
            else:
                z = sum(wv @ kern[t // k, t % k] for t, wv in enumerate(win))
            scale, bias = quantize.fold_bn(l, weights)
            t = z * scale + bias
            out[l.name] = (t.sum((0, 1, 2)), int(t.shape[0] * t.shape[1] * t.shape[2]))
            a = op['act']
            T[op['out']] = t if a == ns.ACT_NONE else np.maximum(t, 0.0) if a == ns.ACT_RELU else np.where(t >= 0, t, t * float(op['alpha']))
        elif op['type'] == ns.OP_UPSAMPLE:
            T[op['out']] = x.repeat(2, 1).repeat(2, 2)
        else:
            T[op['out']] = np.concatenate([x, T[op['in1']]], 3)
    return out, T


def float_ranges(spec, T):
    names = quantize.tensor_names(spec)
    return {names[i]: (float(v.min()), float(v.max())) for i, v in T.items()}


def numpy_measure(frames_u8):
    """measure(model) of biascorrect.correct on the CPU: every conv's input from oracle.kpu_ref.run (through kpu_synth.trace), its z from
    kpu_synth.conv_z, summed over the positions biascorrect.steps_of / the conv's own pooling keep."""
    chw = [np.ascontiguousarray(f.transpose(2, 0, 1)) for f in frames_u8]

    def measure(model):
        steps, counts = biascorrect.steps_of(model), biascorrect.counted(model, len(chw))
        sums = {c.index: np.zeros(c.out_ch, np.int64) for c in model.convs}
        seen_n = {c.index: 0 for c in model.convs}
        for f in chw:
            _, _, seen = kpu_synth.trace(model, f)
            for c in model.convs:
                z = kpu_synth.conv_z(c, seen[c.index][None])[0]
                st = 2 if c.pool_type == km_.POOL_LEFT_TOP_2_S2 else steps[c.index]
                z = z[:, ::st, ::st]
                sums[c.index] += z.sum((1, 2))
                seen_n[c.index] += z.shape[1] * z.shape[2]
        assert seen_n == counts, (seen_n, counts)
        return {i: (sums[i], counts[i]) for i in sums}
    return measure


@functools.lru_cache(maxsize=None)
def mini_case():
    """(spec, weights, frames, float means, ranges) of the mini network: built once per process and never changed."""
    spec = mini_spec()
    w = spec.init_weights(seed=7)
    fr = mini_frames(3, spec.in_hw, 11)
    fr.setflags(write=False)
    fm, T = float_means(spec, w, fr)
    return spec, w, fr, fm, float_ranges(spec, T)
