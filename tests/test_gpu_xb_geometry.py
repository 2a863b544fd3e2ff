"""The fused depthwise + pointwise block (csrc/yk_xblock.h) at the shapes where per-thread item geometry computed ONCE per workgroup
(patch offset of tap (0, 0), A-tile offset, liveness - see `dsrc / dpar / ddst` there) can go wrong, through the f16x2 plan.

Criterion: tests/layerwise.py, unchanged - every stored tensor read back and held, element by element, to oracle/x2_bound.py's float64
chain from the GPU's own inputs (error / E <= 1), as in tests/test_gpu_layers_x2.py.  Then the same plan twice, bit for bit.

`narrow` (46x62 frame, four waves):
    stem 24, stride 2 -> 23x31, fused with dw s1 + pw 24->40          the STEM form fed from u8 frames (GL = 3, one step)
    dw s1 + pw 40->72     2 steps, the second with groups past the tensor (5 groups); input read by this block alone: fp32 planes
    dw s2 + pw 72->96     3 steps, stride 2 on an ODD size (23x31 -> 12x16), input with a second reader: (hi | lo)
    dw s1 + pw 96->96 + Add   3 steps, the residual path
`wide` (40x56 frame):
    dw s2 + pw 192->384   6 steps, stride 2 on an EVEN size (20x28 -> 10x14), 192-wide tiles on four waves
    dw s1 + pw 384->384   12 steps: the 384-wide geometry on eight waves, (hi | lo) input
    dw s1 + pw 384->384   the same on fp32 planes
`one_tile` (16x32 frame): 8x16 = 128 output pixels, the smallest image a block is fused at: one 128-pixel tile is the whole image, and
    24 -> 48 leaves the step's fourth group past the tensor.
23x31, 12x16 on 64-pixel tiles and 10x14 are no multiples of any tile the geometry rule picks: the last tile row and column are partly
dead, several tiles per image so that the rotated step order starts at different steps, and at B = 3 the workgroup index crosses image
boundaries.  B = 1 runs `narrow` alone."""
import re
import time

import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from tests.layerwise import _frames, _layerwise, _report, _switches

pytestmark = pytest.mark.gpu

KERAS_SAME_S2 = (0, 1, 0, 1)


def _out(s, x, name):
    return s.conv(x, 18, 1, bn=False, bias=True, name=name, net_output=True)


def narrow():
    s = ns.NetSpec('xbgeo_narrow', (46, 62), anchor_num=3, class_num=1)
    x = s._new_tensor(46, 62, 3)
    x = s.conv(x, 24, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 23x31x24
    a = s.conv(s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='dw_a'), 40, 1, act=ns.LEAKY03, name='pw_a')
    b = s.conv(s.dwconv(a, 1, ns.SAME3, act=ns.RELU6, name='dw_b'), 72, 1, act=ns.LEAKY03, name='pw_b')
    y2 = _out(s, b, 'out_b')                                                               # the second reader of b: stored as (hi | lo)
    c = s.conv(s.dwconv(b, 2, ns.K210_S2_PAD, act=ns.RELU, name='dw_c'), 96, 1, act=ns.LEAKY03, name='pw_c')   # 12x16x96
    d = s.conv(s.dwconv(c, 1, ns.SAME3, act=ns.RELU, name='dw_d'), 96, 1, act=ns.LEAKY03, name='pw_d')
    r = s.add(c, d)
    y1 = _out(s, r, 'out_r')
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=21)


def wide():
    s = ns.NetSpec('xbgeo_wide', (40, 56), anchor_num=3, class_num=1)
    x = s._new_tensor(40, 56, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 20x28x16
    x = s.conv(x, 192, 1, act=ns.LEAKY03, name='widen')
    a = s.conv(s.dwconv(x, 2, KERAS_SAME_S2, act=ns.RELU, name='dw_a'), 384, 1, act=ns.LEAKY03, name='pw_a')   # 10x14x384
    y2 = _out(s, a, 'out_a')                                                               # a: (hi | lo)
    b = s.conv(s.dwconv(a, 1, ns.SAME3, act=ns.RELU, name='dw_b'), 384, 1, act=ns.LEAKY03, name='pw_b')          # b: fp32 planes
    c = s.conv(s.dwconv(b, 1, ns.SAME3, act=ns.RELU, name='dw_c'), 384, 1, act=ns.LEAKY03, name='pw_c')
    y1 = _out(s, c, 'out_c')
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=22)


def one_tile():
    s = ns.NetSpec('xbgeo_one_tile', (16, 32), anchor_num=3, class_num=1)
    x = s._new_tensor(16, 32, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                  # 8x16x16
    x = s.conv(x, 24, 1, act=ns.LEAKY03, name='widen')
    a = s.conv(s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='dw_a'), 48, 1, act=ns.LEAKY03, name='pw_a')
    y = _out(s, a, 'out_a')
    s.outputs = [y]
    return s, s.init_weights(seed=23)


SPECS = {'narrow': narrow, 'wide': wide, 'one_tile': one_tile}
# what each launch list must contain: (regular expression, number of launches it matches)
EXPECT = {
    'narrow': [(r'^x:stem3x3s2_24\+dw3x3s1\+conv1x1_24to40\[', 1), (r'dw3x3s1\+conv1x1_40to72\[', 1), (r'dw3x3s2\+conv1x1_72to96\[', 1),
               (r'dw3x3s1\+conv1x1_96to96\+add\[', 1)],
    'wide': [(r'dw3x3s2\+conv1x1_192to384\[', 1), (r'dw3x3s1\+conv1x1_384to384\[', 2)],
    'one_tile': [(r'dw3x3s1\+conv1x1_24to48\[', 1)],
}
_cache = {}


def _spec(name):
    if name not in _cache:
        _cache[name] = SPECS[name]()
    return _cache[name]


@pytest.mark.parametrize('name,B', [('narrow', 3), ('narrow', 1), ('wide', 3), ('one_tile', 3)])
def test_fused_blocks_within_their_bound(name, B):
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B)
    _report(f'xbgeo {name} {spec.in_hw[0]}x{spec.in_hw[1]} B={B}', names, rows, over, t0)
    for pat, n in EXPECT[name]:
        assert sum(bool(re.search(pat, x)) for x in names) == n, (pat, n, names)


@pytest.mark.parametrize('name', list(SPECS))
def test_same_plan_twice_identical_bits(name):
    """Every output twice from one plan, and image 0 alone: an image's bits depend neither on the run nor on its batch mates."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, w = _spec(name)
    frames = torch.from_numpy(_frames(spec, 3, seed=5)).cuda()
    with _switches(), engine.Plan(spec, w, max_batch=3, precision='f16x2', schedule='throughput') as plan:
        def run(f):
            plan.run_u8(f)
            plan.check()
            return [o[:f.shape[0]].cpu().numpy().copy() for o in plan.outputs()]
        first, second = run(frames), run(frames)
        alone = run(frames[:1].contiguous())
    for a, b, c in zip(first, second, alone):
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
        assert a.tobytes() == b.tobytes(), 'two runs of the same batch differ'
        assert a[:1].tobytes() == c.tobytes(), 'image 0 alone differs from image 0 in the batch'
