"""GPU parity of the opt-in `precision='f16'` mode ONLY (the f16x2 default and its `x:` kernels: tests/test_gpu_layers_x2.py),
one launch at a time: every materialised tensor of a plan is recomputed by the CPU oracle FROM THE
GPU'S OWN INPUT TENSORS of that launch (read back bit-exactly), so the comparison isolates each kernel from the
accumulated fp16 drift of the layers before it.  What is left is fp32 accumulation order, i.e. at most a 1-ulp
fp16 flip on a small fraction of elements:
    |gpu - ref| <= 2^-9 * |ref| + 1e-3 * rms(ref)      for every element   (1 fp16 ulp is <= 2^-10 * |ref|)
    and fewer than 2 % of the elements differ at all; fp32 network outputs: <= 1e-4*|ref| + 1e-4*rms(ref).
Covers: stem (u8 + normalise LUT), fused dw3x3+pw1x1 (all four tile configs), standalone dw, implicit-GEMM
1x1/3x3 incl. split-K, upsample+concat loader, residual Add epilogue, stride-2 top/left pad, max pools, fp32 heads."""
import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from tests.layerwise import _layerwise_f16 as _layerwise             # shared with tests/test_gpu_plan_zoo.py

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fuse,splitk', [(True, True), (False, False)])
def test_yolo_mobilev1_headline_layers(fuse, splitk):
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    n, names = _layerwise(spec, spec.init_weights(seed=1), 2, fuse, splitk)
    assert n >= (19 if fuse else 32)
    assert any('splitk' in x for x in names) == splitk


def test_yolo_mobilev1_batch32_layers_use_every_fused_config():
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    n, names = _layerwise(spec, spec.init_weights(seed=1), 32)
    for cfg in ('lr_', 'wide_'):
        assert any(cfg in x for x in names), (cfg, names)


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_yolo_mobilev1_other_widths(alpha):
    spec = ns.yolo_mobilev1((96, 128, 3), 3, 20, alpha=alpha)
    _layerwise(spec, spec.init_weights(seed=2), 3)


@pytest.mark.parametrize('fuse', [True, False])
def test_yolo_mobilev2_layers(fuse):
    spec = ns.yolo_mobilev2((224, 320, 3), 3, 20, alpha=1.0)     # K=124 padding, ReLU6, linear bottleneck + Add
    n, names = _layerwise(spec, spec.init_weights(seed=1), 2, fuse)
    assert any('+add' in x for x in names)


def test_tiny_yolo_layers():
    spec = ns.tiny_yolo((224, 320, 3), 3, 20)                    # max pools incl. the stride-1 'same' one
    _layerwise(spec, spec.init_weights(seed=1), 2)
    spec = ns.tiny_yolo((416, 416, 3), 3, 20)                    # BASELINE config 3 shape (13x13 / 26x26)
    _layerwise(spec, spec.init_weights(seed=1), 1)


def test_darknet53_layers():
    spec = ns.yolo((128, 160, 3), 3, 20)                         # stride-2 (1,0) pad, 23 residual Adds, 3 scales
    w = spec.init_weights(seed=1)
    for k in w:
        if k.endswith('/gamma'):
            w[k] = (w[k] * 0.5).astype(np.float32)               # keep random-init activations inside fp16 range
    n, names = _layerwise(spec, w, 2)
    assert sum('+add' in x for x in names) == 23
    assert sum('+upcat' in x for x in names) == 2


def test_darknet53_416_fp16_stress_config_layers():
    """BASELINE configs[4]: full YOLO (Darknet-53) 416x416, 3 scales x 3 anchors, fp16 storage — every one of the 75 convs
    at the real shape, one launch at a time (the oracle runs on the host cores of the GPU box)."""
    spec = ns.yolo((416, 416, 3), 3, 20)
    assert spec.out_hw() == [(13, 13), (26, 26), (52, 52)]
    w = spec.init_weights(seed=1)
    for k in w:
        if k.endswith('/gamma'):
            w[k] = (w[k] * 0.5).astype(np.float32)
    n, names = _layerwise(spec, w, 1)
    assert n >= 75
