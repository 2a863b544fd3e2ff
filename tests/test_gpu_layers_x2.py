"""f16x2 parity, one launch at a time, against a per-element bound from the launch's own inputs.

For every tensor an f16x2 plan keeps in memory: walk back through spec.ops to the nearest stored tensors, recompute that chain in
float64 FROM THE GPU'S OWN VALUES of those tensors (oracle/x2_bound.py; read back exactly, with their per-image exponents), and
assert |gpu - ref| <= E for EVERY element, E being the propagated bound of that module (C_DOT * 2^-22 * sum |w||x| per dot product,
plus what the stored format can lose at the exponent the plan actually used).  tests/test_x2_bound.py shows what this accepts and
rejects.  The whole-network tests compare a handful of tensors to 1e-4 of their maximum after up to 75 layers; a dropped cross product
in one k-step, a wrong border tap in one tile shape or a ragged channel tail stays below that and shows here as error / E >> 1.

Every launch of `plan.launches()` except u8_max must have its stored outputs checked: the number of checked tensors EQUALS the number
the launch list says the plan stores (one per launch; a heads cluster launch one per phase, a persistent launch one per store phase).
A read that fails for any reason other than "not stored" fails the test.

Format health of every stored split tensor, every image with a non-zero maximum (x2_bound.split_health): the exponent is normalised
by the epilogue so that bound * 2^-e lies in [2^13, 2^14) (x_exp_of in csrc/yk_exact.hip); so amax * 2^-e fits fp16, hi is never inf,
every read-back value is finite and is the sum of two fp16 numbers at that exponent, and the over-estimate 2^(e+14) / amax stays below
the 2^16 of DESIGN section 2.

Oracle time (float64, 16 host threads; measured): the whole file 35 s; Darknet-53 at 416x416, one image, all 75 tensors 3.8 s, the
B = 32 plans 9 s each - so every tensor of every plan is checked, none sampled.  Measured worst error / E per plan (one MI355X):
yolo_mobilev1 0.12 - 0.15 (cluster launches 0.03), yolo_mobilev2 0.29, tiny_yolo 0.09, Darknet-53 0.15 / 0.17."""
import time

import pytest

from k210_yolo_framework_amd import netspec as ns
from tests.layerwise import _layerwise, _report                      # shared with tests/test_gpu_plan_zoo.py

pytestmark = pytest.mark.gpu


def _mobilev1():
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    return spec, spec.init_weights(seed=1)


@pytest.mark.parametrize('B', [2, 32])
@pytest.mark.parametrize('schedule', ['throughput', 'latency'])
def test_yolo_mobilev1_benched_network(B, schedule):
    t0 = time.time()
    spec, w = _mobilev1()
    names, rows, over = _layerwise(spec, w, B, schedule)
    _report(f'yolo_mobilev1-0.75 224x320 B={B} {schedule}', names, rows, over, t0)
    assert any(n.startswith('x:persist') for n in names) == (schedule == 'latency')
    assert any(n.startswith('x:heads') for n in names) == (schedule == 'latency')
    assert any('stem3x3s2' in n and '+dw3x3' in n for n in names)


def test_yolo_mobilev1_every_basic_kernel_unfused():
    t0 = time.time()
    spec, w = _mobilev1()
    names, rows, over = _layerwise(spec, w, 2, env={'YK_FUSE_DWPW': '0', 'YK_SPLITK': '0', 'YK_FUSE_HEAD': '0'})
    _report('yolo_mobilev1-0.75 224x320 B=2 unfused', names, rows, over, t0)
    assert len(rows) == len([op for op in spec.ops if op['type'] in (ns.OP_CONV, ns.OP_DWCONV)])     # one op per launch, all of them
    assert not any('splitk' in n for n in names)


def test_yolo_mobilev1_cluster_write_through():
    t0 = time.time()
    spec, w = _mobilev1()
    names, rows, over = _layerwise(spec, w, 2, 'latency', env={'YK_CLUSTER_WT': '1'})
    _report('yolo_mobilev1-0.75 224x320 B=2 latency YK_CLUSTER_WT=1', names, rows, over, t0)
    assert any(n.startswith('x:persist') for n in names)


def test_yolo_mobilev1_fp32_entry_valu_stem():
    t0 = time.time()
    spec, w = _mobilev1()
    names, rows, over = _layerwise(spec, w, 2, f32_entry=True)
    _report('yolo_mobilev1-0.75 224x320 B=2 run_f32', names, rows, over, t0)


@pytest.mark.parametrize('shape,alpha', [((96, 128, 3), 0.5), ((64, 96, 3), 1.0)])
def test_yolo_mobilev1_ragged_tiles_small_images(shape, alpha):
    t0 = time.time()
    spec = ns.yolo_mobilev1(shape, 3, 20, alpha=alpha)
    names, rows, over = _layerwise(spec, spec.init_weights(seed=2), 3)
    _report(f'yolo_mobilev1-{alpha} {shape[0]}x{shape[1]} B=3', names, rows, over, t0)


@pytest.mark.parametrize('fuse', [True, False])
def test_yolo_mobilev2(fuse):
    t0 = time.time()
    spec = ns.yolo_mobilev2((224, 320, 3), 3, 20, alpha=1.0)          # K = 124 padding, ReLU6, the Add folded into its producer
    names, rows, over = _layerwise(spec, spec.init_weights(seed=1), 2, env=None if fuse else {'YK_FUSE_DWPW': '0'})
    _report(f'yolo_mobilev2-1.0 224x320 B=2 fuse={fuse}', names, rows, over, t0)
    assert any('+add' in n for n in names)


def test_tiny_yolo_416():
    t0 = time.time()
    spec = ns.tiny_yolo((416, 416, 3), 3, 20)                         # max pools, split-K heads through xg_reduce_kernel
    names, rows, over = _layerwise(spec, spec.init_weights(seed=1), 2)
    _report('tiny_yolo 416x416 B=2', names, rows, over, t0)
    assert any('maxpool' in n for n in names) and any('splitk' in n for n in names)


def test_darknet53_128x160_undamped():
    t0 = time.time()
    spec = ns.yolo((128, 160, 3), 3, 20)                              # stride-2 (1, 0) pad, 23 Adds, two-exponent up+concat, ~1e6 activations
    names, rows, over = _layerwise(spec, spec.init_weights(seed=1), 2)
    _report('yolo (Darknet-53) 128x160 B=2 undamped', names, rows, over, t0)
    assert sum('+add' in n for n in names) == 23
    assert sum('+upcat' in n for n in names) == 2


def test_darknet53_416_undamped():
    t0 = time.time()
    spec = ns.yolo((416, 416, 3), 3, 20)
    names, rows, over = _layerwise(spec, spec.init_weights(seed=1), 1)
    _report('yolo (Darknet-53) 416x416 B=1 undamped', names, rows, over, t0)
    assert len(rows) == 75
