"""The fused depthwise + pointwise block (csrc/yk_xblock.h) with its pointwise weight fragments requested a phase ahead: W(0) in the
prologue behind the first patch request, W(k+1) when the MFMAs of step k have been issued, and a COUNTED wait at the top of a step
(`vmcnt(2 * TNW)`: the patch has landed, the fragments stay in flight under the depthwise pass; a wave that requested none waits for
everything).  What a wrong count, a wrong k+1 address or a wrong order in the prologue would break is the VALUE of a launch, so:

Criterion: tests/layerwise.py, unchanged - every stored tensor read back and held, element by element, to oracle/x2_bound.py's float64
chain from the GPU's own inputs of the launch (error / E <= 1), as in tests/test_gpu_layers_x2.py and tests/test_gpu_plan_zoo.py.  Then
the same plan twice, bit for bit, and an image alone against the same image inside a batch.

`chain` (46x62 frame, u8 AND f32 frames - the two fused-stem kernels):
    stem 24, stride 2 -> 23x31, fused with dw s1 + pw 24->40     nk = 1 in the STEM form: no W(k+1), the prologue's frame-window loads
                                                                 sit between W(0) and the counted wait; 40 outputs in a 64-wide tile:
                                                                 wave 3 requests nothing and waits for everything beside live waves
    dw s1 + pw 40->72       nk = 2: kstep(ks + 1) wraps at once in every tile with rot = 1; five channel groups: the last step is partial
                            (three of its four groups lie past the tensor); 72 outputs in a 128-wide tile: wave 3 dead
    dw s2 + pw 72->96       nk = 3, nine groups (last step: one group); 96 outputs in a 128-wide tile: wave 3 dead
    dw s1 + pw 96->96 + Add nk = 3 with the residual (the mobilev2 form)
  every image is several tiles (asserted), so rot = tile % nk takes every value and workgroups of one launch start at different steps
`short` (16x32 frame): 8x16 = 128 output pixels, the smallest image a block is fused at
    dw s1 + pw 24->48       nk = 1 on a STORED tensor (three groups: a partial first and last step), 48 outputs in a 64-wide tile: wave 3 dead
`long` (28x40 frame -> 14x20):
    dw s1 + pw 384->384     the `wide` geometry on eight waves, 12 steps, five tiles per image: rot = 0..4

Every case asserts from the plan's launch list that each block ran as ONE fused launch with the step count, the N tile (64 * TN channels;
384 is the eight-wave tile) and the number of tiles per image the case is there for."""
import re
import time

import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from tests.layerwise import _frames, _layerwise, _report, _switches

pytestmark = pytest.mark.gpu


def _out(s, x, name):
    return s.conv(x, 18, 1, bn=False, bias=True, name=name, net_output=True)


def chain():
    s = ns.NetSpec('xbwpf_chain', (46, 62), anchor_num=3, class_num=1)
    x = s._new_tensor(46, 62, 3)
    x = s.conv(x, 24, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 23x31x24
    a = s.conv(s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='dw_a'), 40, 1, act=ns.LEAKY03, name='pw_a')
    b = s.conv(s.dwconv(a, 1, ns.SAME3, act=ns.RELU6, name='dw_b'), 72, 1, act=ns.LEAKY03, name='pw_b')
    y2 = _out(s, b, 'out_b')
    c = s.conv(s.dwconv(b, 2, ns.K210_S2_PAD, act=ns.RELU, name='dw_c'), 96, 1, act=ns.LEAKY03, name='pw_c')   # 12x16x96
    d = s.conv(s.dwconv(c, 1, ns.SAME3, act=ns.RELU6, name='dw_d'), 96, 1, act=(ns.ACT_NONE, 0.0), name='pw_d')
    y1 = _out(s, s.add(c, d), 'out_r')
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=31)


def short():
    s = ns.NetSpec('xbwpf_short', (16, 32), anchor_num=3, class_num=1)
    x = s._new_tensor(16, 32, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 8x16x16
    x = s.conv(x, 24, 1, act=ns.LEAKY03, name='widen')
    a = s.conv(s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='dw_a'), 48, 1, act=ns.LEAKY03, name='pw_a')
    s.outputs = [_out(s, a, 'out_a')]
    return s, s.init_weights(seed=32)


def long():
    s = ns.NetSpec('xbwpf_long', (28, 40), anchor_num=3, class_num=1)
    x = s._new_tensor(28, 40, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 14x20x16
    x = s.conv(x, 384, 1, act=ns.RELU6, name='expand')
    a = s.conv(s.dwconv(x, 1, ns.SAME3, act=ns.RELU6, name='dw_a'), 384, 1, act=ns.LEAKY03, name='pw_a')
    s.outputs = [_out(s, a, 'out_a')]
    return s, s.init_weights(seed=33)


SPECS = {'chain': chain, 'short': short, 'long': long}
# per block: (start of the launch name, output size (Ho, Wo), input channels, channels of the N tile, least tiles per image)
EXPECT = {
    'chain': [('x:stem3x3s2_24+dw3x3s1+conv1x1_24to40[', (23, 31), 24, 64, 2), ('x:dw3x3s1+conv1x1_40to72[', (23, 31), 40, 128, 2),
              ('x:dw3x3s2+conv1x1_72to96[', (12, 16), 72, 128, 3), ('x:dw3x3s1+conv1x1_96to96+add[', (12, 16), 96, 128, 3)],
    'short': [('x:dw3x3s1+conv1x1_24to48[', (8, 16), 24, 64, 1)],
    'long': [('x:dw3x3s1+conv1x1_384to384[', (14, 20), 384, 384, 5)],
}
NK = {24: 1, 40: 2, 72: 3, 96: 3, 384: 12}                            # steps of 32 input channels
_cache = {}


def _spec(name):
    if name not in _cache:
        _cache[name] = SPECS[name]()
    return _cache[name]


def _assert_paths(name, names):
    """Each block of the case is ONE fused launch on the tile the case is about."""
    fused = [n for n in names if 'dw3x3' in n]
    assert len(fused) == len(EXPECT[name]), names                     # no depthwise conv outside a fused launch, none twice
    for (head, (Ho, Wo), cin, ch, tiles), n in zip(EXPECT[name], fused):
        assert n.startswith(head), (head, names)
        m = re.search(r'\[(\d+)x(\d+)px,(\d+)ch,1stage\]$', n)
        assert m, n
        TH, TW, got_ch = (int(v) for v in m.groups())
        assert got_ch == ch, (n, ch)                                  # 64 * TN; 384 = the eight-wave tile
        assert -(-Ho // TH) * -(-Wo // TW) >= tiles, (n, tiles)       # tiles per image: rot = tile % nk
        assert -(-(-(-cin // 8)) // 4) == NK[cin]


@pytest.mark.parametrize('name,B,f32', [('chain', 3, False), ('chain', 2, True), ('short', 3, False), ('long', 2, False)])
def test_blocks_within_their_bound(name, B, f32):
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B, f32_entry=f32, seed=7)
    _report(f'xbwpf {name} {"f32" if f32 else "u8"} frames B={B}', names, rows, over, t0)
    _assert_paths(name, names)
    checked = {r[0] for r in rows}
    assert {n for n in names if 'dw3x3' in n} <= checked              # every block's stored output went through the bound
    assert max(r[3] for r in rows) <= 1.0


@pytest.mark.parametrize('name,f32', [('chain', False), ('chain', True), ('short', False), ('long', False)])
def test_twice_and_alone_identical_bits(name, f32):
    """Every output twice from one plan, and one image alone: an image's bits depend neither on the run nor on its batch mates."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, w = _spec(name)
    f8 = _frames(spec, 3, seed=9)
    if f32:
        frames = torch.from_numpy((f8.astype(np.float64) / f8.reshape(3, -1).max(1).astype(np.float64).reshape(3, 1, 1, 1)).astype(np.float32)).cuda()
    else:
        frames = torch.from_numpy(f8).cuda()
    with _switches(), engine.Plan(spec, w, max_batch=3, precision='f16x2', schedule='throughput') as plan:
        def run(f):
            (plan.run_f32 if f32 else plan.run_u8)(f)
            plan.check()
            return [o[:f.shape[0]].cpu().numpy().copy() for o in plan.outputs()]
        first, second = run(frames), run(frames)
        alone = run(frames[1:2].contiguous())
        _assert_paths(name, [l[0] for l in plan.launches()])
    for a, b, c in zip(first, second, alone):
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
        assert a.tobytes() == b.tobytes(), 'two runs of the same batch differ'
        assert a[1:2].tobytes() == c.tobytes(), 'image 1 alone differs from image 1 in the batch'
