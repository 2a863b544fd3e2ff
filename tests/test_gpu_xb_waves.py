"""The 8-wave form of the fused depthwise + pointwise block (csrc/yk_xblock.h, NW = 8), one launch at a time, against the per-element
bound of tests/test_gpu_layers_x2.py (oracle/x2_bound.py: float64 from the GPU's own stored inputs of the launch, |gpu - ref| <= E
for EVERY element).

xb_geometry (csrc/yk_exact.hip) sends a block with more than 192 output channels and more than six channel steps to the 384-wide
tile (`wide`), and that tile runs on eight waves: wave w owns 48 output channels, a depthwise item is one channel HALF of a (pixel,
group), every deposit and copy-out loop strides by 512.  The networks here are a 16-filter stem, a 1x1 conv up to the block's input
channels, the block(s), and a 1x1 output conv: the only interesting launches are the blocks.  What the shapes are for:

  384 -> 384 -> 384, 14x20      the benched network's shape.  Two blocks in a row: the first one's output has the second one's depthwise
  B = 1, B = 3                  conv as its only reader, so it leaves as fp32 planes straight from the registers and the second one's half
                                items read fp32 planes; the second block's output goes through the LDS staging passes as (hi | lo).  14x4
                                pixel tiles: rows 56..63 of every A tile are dead.  B = 3: per-image exponents and maxima
  384 -> 384, 6x23              three row blocks (TM = 3: 384 half items on 512 threads, the last two waves have none), 6x8 pixel tiles, the
                                last one partial (23 = 8 + 8 + 7)
  384 -> 384, 15x22             8x8 pixel tiles with partial tiles in both directions (15 = 8 + 7, 22 = 8 + 8 + 6)
  360 -> 392, 14x20             45 channel groups: the twelfth step holds one group of four; two N slices, the second with 8 live
                                channels: waves 1..7 dead, wave 0 with half a slab
  384 -> 384 + Add, 14x20       mobilev2-style block: the residual is read in the staging pass; the block's input has two readers (the
                                depthwise conv and the Add), so it is stored as (hi | lo) and the half items take the two 8-byte reads
  384 -> 384, (hi | lo) input   the same input format without a residual (a 1x1 conv is the second reader)

The issue that asked for these tests named a 5x7 image (one partial tile, dead rows).  decide_blocks (csrc/yk_xplan_build.h) fuses a
block from 128 output pixels per image on, so a 35-pixel image never reaches this kernel in a product build; 6x23 is the smallest
image the builder gives a tile of fewer than four row blocks, and it has the partial tile.  Dead rows are in every 14x4 case.

Every case asserts from the plan's launch list that each block ran as ONE launch on the 384-channel tile (`384ch` in the launch name is
64 * TN = 384, which only the `wide` rule selects, and the wide rule is the eight-wave rule)."""
import re
import time

import pytest

from k210_yolo_framework_amd import netspec as ns
from tests.layerwise import _layerwise, _report

pytestmark = pytest.mark.gpu

NONE = (ns.ACT_NONE, 0.0)


def _net(name, hw, cin, couts, residual=False, second_reader=False):
    """stem (stride 2) -> 1x1 up to cin -> one block per entry of couts -> 1x1 output conv; hw is the size of the blocks' tensors."""
    s = ns.NetSpec(name, (2 * hw[0], 2 * hw[1]), anchor_num=3, class_num=1)
    x = s._new_tensor(2 * hw[0], 2 * hw[1], 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')
    x = s.conv(x, cin, 1, act=ns.RELU6, name='expand')
    if second_reader:
        s.conv(x, 16, 1, act=ns.LEAKY01, name='side')
    for i, co in enumerate(couts):
        d = s.dwconv(x, 1, ns.SAME3, act=ns.RELU6, name=f'dw_{i}')
        y = s.conv(d, co, 1, act=NONE if residual else ns.LEAKY03, name=f'pw_{i}')
        x = s.add(x, y) if residual else y
    out = s.conv(x, 18, 1, bn=False, bias=True, name='out', net_output=True)
    s.outputs = [out]
    return s


CASES = {
    # name: (hw, cin, couts, B, residual, second_reader, tile)
    'benched_b1': ((14, 20), 384, [384, 384], 1, False, False, '14x4'),
    'benched_b3': ((14, 20), 384, [384, 384], 3, False, False, '14x4'),
    'three_row_blocks_6x23': ((6, 23), 384, [384], 2, False, False, '6x8'),
    'partial_tiles_15x22': ((15, 22), 384, [384], 1, False, False, '8x8'),
    'ragged_360to392': ((14, 20), 360, [392], 2, False, False, '14x4'),
    'residual_add': ((14, 20), 384, [384], 2, True, False, '14x4'),
    'hi_lo_input': ((14, 20), 384, [384], 2, False, True, '14x4'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_wide_block_on_eight_waves(case):
    t0 = time.time()
    hw, cin, couts, B, residual, second, tile = CASES[case]
    spec = _net('xbw_' + case, hw, cin, couts, residual, second)
    names, rows, over = _layerwise(spec, spec.init_weights(seed=21), B, seed=5)
    _report(f'{case} B={B}', names, rows, over, t0)
    want, ci = [], cin
    for co in couts:
        want.append(f'x:dw3x3s1+conv1x1_{ci}to{co}{"+add" if residual else ""}[{tile}px,384ch,1stage]')
        ci = co
    assert [n for n in names if re.match(r'x:dw3x3', n)] == want, names     # every depthwise conv inside a fused launch on the 384-wide tile
    checked = {r[0] for r in rows}
    assert set(want) <= checked                                       # every block's stored output went through the bound
    assert max(r[3] for r in rows) <= 1.0
