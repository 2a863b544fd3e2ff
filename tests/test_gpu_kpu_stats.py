"""KpuPlan.run_stats_u8 (csrc/yk_kpu.hip, the statistics instantiations): per-channel integer sums of z, exactly those of kpu_synth.conv_z over
the counted positions, with every tensor and output bit-identical to a plain run_u8."""
import functools

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel as km_
from tests import kpu_synth as ks

pytestmark = pytest.mark.gpu

_out = [ks.dequant('out', 0.037, -2.5)]


@pytest.fixture(scope='module', autouse=True)
def _give_the_memory_back():
    """The tensors of this file are returned to the driver when it is done, so that later files meet the device as they did before it existed."""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
# name -> (frame C, H, W), layer descriptions, {conv position: step 2}
#   a: C = 3 frame (generic operand path), OC 5 / 32 / 33 / 48 / 1, a depthwise conv at step 2 on an odd 13 x 19, a self-pooling dense conv
#      (13 x 19 -> 7 x 10: M = 70 per image, so a batch of 1 leaves two of a workgroup's four waves without pixels), a depthwise conv at step 1.
#   b: C = 16 frame (the 16-byte operand path in NHWC, the generic one in CHW), 9 x 11 = 99 pixels: M = 99 / 297, never a multiple of 64;
#      a dense 3x3 conv counted at step 2, depthwise 1x1 and 3x3 with C = 48 and C = 5.
MODELS = {
    'a': ((3, 13, 19), [ks.conv(5, k=3), ks.conv(32, k=1), ks.conv(dw=True, k=3), ks.conv(33, k=3), ks.conv(48, k=1, s2=True),
                        ks.conv(dw=True, k=3), ks.conv(1, k=1, mem='out')] + _out, {2: 2}),
    'b': ((16, 9, 11), [ks.conv(48, k=3), ks.conv(dw=True, k=1), ks.conv(5, k=3, pad=0), ks.conv(dw=True, k=3, pad=255),
                        ks.conv(32, k=3, mem='out')] + _out, {0: 2, 3: 2}),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, frames uint8 [4][C][H][W], {layer index: step}, {batch: {layer index: expected int64 sums}}): built once, never changed."""
    in_chw, descs, step_at = MODELS[name]
    frames = ks.make_frames(in_chw, 77 + len(name) + ord(name[0]))
    frames.setflags(write=False)
    model = ks.build(list(descs), in_chw, frames, 5 + ord(name[0]))
    steps = {c.index: step_at.get(n, 1) for n, c in enumerate(model.convs)}
    per_frame = []
    for f in frames[:3]:
        _, _, seen = ks.trace(model, f)
        sums = {}
        for c in model.convs:
            z = ks.conv_z(c, seen[c.index][None])[0]
            st = 2 if c.pool_type == km_.POOL_LEFT_TOP_2_S2 else steps[c.index]       # a conv that pools itself computes the kept positions only
            sums[c.index] = z[:, ::st, ::st].sum((1, 2))
        per_frame.append(sums)
    want = {b: {i: sum(p[i] for p in per_frame[:b]) for i in per_frame[0]} for b in (1, 3)}
    return model, frames, steps, want


def _device_frames(frames, batch, layout):
    import torch
    f = frames[:batch] if layout == 'chw' else frames[:batch].transpose(0, 2, 3, 1)
    return torch.from_numpy(np.array(f, order='C')).cuda()                            # a copy: the shared frames are read-only


@pytest.mark.parametrize('layout', ['nhwc', 'chw'])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('name', sorted(MODELS))
def test_sums_are_exact_and_the_run_is_bit_identical(name, batch, layout):
    import torch
    from k210_yolo_framework_amd import engine
    model, frames, steps, want = _case(name)
    assert {c.out_ch for m in MODELS for c in _case(m)[0].convs} >= {1, 5, 32, 33, 48}
    fd = _device_frames(frames, batch, layout)
    with engine.KpuPlan(model, max_batch=3) as plain, engine.KpuPlan(model, max_batch=3) as stat:
        plain.run_u8(fd, layout)
        stat.reset_zsums()
        stat.run_stats_u8(fd, steps, layout)
        got = stat.read_zsums()
        assert set(got) == set(want[batch])
        for i, w in want[batch].items():
            assert got[i].dtype == np.int64 and np.array_equal(got[i], w), (i, steps[i], got[i], w)
        for c in model.convs:
            for b in range(batch):
                assert np.array_equal(stat.read_layer(c.index, b), plain.read_layer(c.index, b)), (c.index, b)
        torch.cuda.synchronize()
        for a, b_ in zip(stat.outputs(), plain.outputs()):
            assert torch.equal(a[:batch], b_[:batch])
        stat.run_stats_u8(fd, [steps[c.index] for c in model.convs], layout)          # the list form; no reset: twice the sums
        twice = stat.read_zsums()
        for i, w in want[batch].items():
            assert np.array_equal(twice[i], 2 * w), i
        stat.reset_zsums()
        assert all(not v.any() for v in stat.read_zsums().values())


def test_bad_steps_are_refused():
    import torch
    from k210_yolo_framework_amd import engine
    model, frames, steps, _ = _case('b')
    fd = _device_frames(frames, 1, 'nhwc')
    with engine.KpuPlan(model, max_batch=1) as plan:
        with pytest.raises(engine.YkError):
            plan.run_stats_u8(fd, [1, 2])
        with pytest.raises(engine.YkError):
            plan.run_stats_u8(fd, {c.index: 3 for c in model.convs})
        with pytest.raises(engine.YkError):
            plan.run_stats_u8(fd, {10 ** 6: 2})
    torch.cuda.synchronize()
