"""More than 64 KB of dynamic LDS needs an attribute per (device, kernel).  One helper sets it (yk_allow_lds, csrc/yk_region.hip), and
every large-LDS launch goes through it (yk_launch_lds, csrc/yk_common.h)."""
import re
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / 'k210_yolo_framework_amd' / 'csrc'
ATTR = 'hipFuncAttributeMaxDynamicSharedMemorySize'


def test_the_lds_attribute_is_set_only_by_the_one_helper():
    sources = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in ('.h', '.hip')}
    where = [(name, txt.count('\n', 0, m.start()) + 1) for name, txt in sources.items()
             for m in re.finditer('hipFuncSetAttribute|' + ATTR, txt)]
    txt = sources['yk_region.hip']
    start = txt.index('\nvoid yk_allow_lds(const void *kern, size_t bytes) {\n')
    first, last = txt.count('\n', 0, start) + 2, txt.count('\n', 0, txt.index('\n}\n', start)) + 1
    assert where and all(name == 'yk_region.hip' and first <= line <= last for name, line in where), where
    assert sum(txt.count(ATTR) for txt in sources.values()) == 1


@pytest.mark.gpu
def test_plans_on_two_devices_of_one_process_give_identical_outputs():
    """The f16x2 throughput plan (its 192-channel fused head takes 66,880 B of LDS) and an f16 plan, on device 0 and then on device 1."""
    import torch
    from k210_yolo_framework_amd import engine, netspec as ns
    if torch.cuda.device_count() < 2:
        pytest.skip('one device visible: the per-device opt-in needs two')
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    w = spec.init_weights(seed=1)
    B = 32
    frames = np.random.default_rng(0).integers(0, 256, (B, 224, 320, 3), dtype=np.uint8)
    got = {}
    for dev in (0, 1):
        with torch.cuda.device(dev):
            for precision in ('f16x2', 'f16'):
                with engine.Plan(spec, w, max_batch=B, device=dev, precision=precision, schedule='throughput') as plan:
                    plan.run_u8(torch.from_numpy(frames).cuda(dev))
                    plan.check()
                    got[dev, precision] = [o[:B].cpu().numpy() for o in plan.outputs()]
    for precision in ('f16x2', 'f16'):
        for a, b in zip(got[0, precision], got[1, precision]):
            assert np.isfinite(a).all() and np.abs(a).max() > 0
            assert np.array_equal(a, b), precision
