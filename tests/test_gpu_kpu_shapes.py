"""The KPU-exact integer kernels (csrc/yk_kpu.hip) at the shapes the demo kmodel does not have: tile edges of the MFMA conv (pixel and
channel tails, packed and byte stores, K chunk tails, the channel-padded loader), stride 2 on odd sides, depthwise element tails, both
frame layouts on the aligned and the unaligned loader, gathers at non-integer ratios and odd channel offsets, K at its limit with the
operands at the ends of int8, the two roundings of DEQUANTIZE, and batches on a reused arena.  Every model comes from tests/kpu_synth.py
(tests/test_kpu_synth.py holds them live on the CPU); every conv layer and every output of every frame is compared with
oracle/kpu_ref.run BIT FOR BIT: np.array_equal on uint8, uint32 views on fp32.  There is no tolerance anywhere."""
import functools

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel
from oracle import kpu_ref
from tests import kpu_synth as ks

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name, fi):
    """kpu_ref.run of frame `fi` of a case, once: (float outputs, {conv index: uint8 output})."""
    model, frames, _ = ks.case(name)
    keep = {}
    outs = kpu_ref.run(model, frames[fi], keep)
    return outs, keep


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_frames(chw, layout, misalign=False):
    """A contiguous cuda uint8 tensor of the frames; misalign: a view one byte into a larger buffer."""
    import torch
    x = torch.from_numpy(np.array(chw if layout == 'chw' else chw.transpose(0, 2, 3, 1), order='C'))      # a writable copy
    if not misalign:
        d = x.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.zeros(x.numel() + 32, dtype=torch.uint8, device='cuda')
    d = buf[1:1 + x.numel()].view(x.shape)
    d.copy_(x)
    assert d.data_ptr() % 16 == 1 and d.is_contiguous()
    return d


def _run(plan, chw, layout='nhwc', misalign=False):
    """Run a batch; returns ([per output: [n][C][H][W] fp32], [per image: {conv index: uint8 [C][H][W]}])."""
    import torch
    plan.run_u8(_device_frames(chw, layout, misalign), layout=layout)
    torch.cuda.synchronize()
    n = len(chw)
    outs = [o[:n].cpu().numpy().transpose(0, 3, 1, 2).copy() for o in plan.outputs()]
    layers = [{li: plan.read_layer(li, i) for li in plan.program.conv_values} for i in range(n)]
    return outs, layers


def _check_case(plan, name, layout='nhwc', misalign=False):
    """All four frames of a case in batches of its size (the last batch wraps round), each against the oracle.  Returns the number of
    (layer, image) tensors compared."""
    _, frames, batch = ks.case(name)
    compared = 0
    for i0 in range(0, len(frames), batch):
        idx = [(i0 + j) % len(frames) for j in range(batch)]
        outs, layers = _run(plan, frames[idx], layout, misalign)
        for j, fi in enumerate(idx):
            ref, keep = _ref(name, fi)
            assert sorted(layers[j]) == sorted(keep)
            for li, q in keep.items():
                got = layers[j][li]
                assert np.array_equal(got, q), (name, layout, fi, li, np.argwhere(got != q)[:4].tolist())
            assert len(outs) == len(ref)
            for oi, (o, r) in enumerate(zip(outs, ref)):
                assert o[j].shape == r.shape and np.array_equal(_bits(o[j]), _bits(r)), (name, layout, fi, oi)
            compared += len(keep) + len(ref)
    return compared


def _plan(name, max_batch=None):
    from k210_yolo_framework_amd import engine
    model, _, batch = ks.case(name)
    return engine.KpuPlan(model, max_batch=batch if max_batch is None else max_batch)


@pytest.mark.parametrize('name', sorted(ks.DENSE))
def test_dense_tile_edges(name):
    """M = batch x OH x OW in {1, 63, 64, 65, 255, 256, 257, 765}, OC in {1, 3, 4, 31, 32, 33, 75}, C in {1, 3, 15, 16, 17, 24, 32, 48},
    1x1 and 3x3, pad_value 0 / 255 / random: pixel tails, channel tails, both stores, chunk tails, both loaders."""
    with _plan(name) as plan:
        n = _check_case(plan, name)
    print(f'{name}: {n} tensors compared bit for bit')


@pytest.mark.parametrize('name', sorted(ks.STRIDE2))
def test_stride_2_on_odd_and_even_sides(name):
    """left_top_2_s2 on a 3x3 dense, a 3x3 depthwise, a 1x1 dense and a 1x1 depthwise conv, chained: OH = (H + 1) / 2."""
    with _plan(name) as plan:
        n = _check_case(plan, name) + _check_case(plan, name, 'chw')
    print(f'{name}: {n} tensors compared bit for bit')


@pytest.mark.parametrize('name', sorted(ks.DEPTHWISE))
def test_depthwise_element_tails(name):
    """C in {1, 5, 16, 33}, 3x3 and 1x1, odd sizes; M*C on both sides of one block of 256 (one image, then two); the first reads the frame."""
    n = 0
    for mb in (1, 2):
        with _plan(name, mb) as plan:
            _, frames, _ = ks.case(name)
            for i0 in range(0, 4, mb):
                outs, layers = _run(plan, frames[i0:i0 + mb], 'nhwc' if mb == 1 else 'chw')
                for j in range(mb):
                    ref, keep = _ref(name, i0 + j)
                    for li, q in keep.items():
                        assert np.array_equal(layers[j][li], q), (name, mb, i0 + j, li)
                    assert np.array_equal(_bits(outs[0][j]), _bits(ref[0])), (name, mb, i0 + j)
                    n += len(keep) + 1
    print(f'{name}: {n} tensors compared bit for bit')


@pytest.mark.parametrize('name', sorted(ks.LAYOUT))
def test_frame_layouts_and_both_loaders(name):
    """chw and nhwc frames of 1, 3 and 16 channels; the 16-channel NHWC frame once from a 16-byte-aligned tensor (the vector loader)
    and once from a view one byte into a buffer (the byte loader): the same bytes in every layer."""
    _, frames, _ = ks.case(name)
    with _plan(name) as plan:
        n = _check_case(plan, name, 'chw') + _check_case(plan, name, 'nhwc')
        if frames.shape[1] == 16:
            n += _check_case(plan, name, 'nhwc', misalign=True)
            a = _run(plan, frames[:2], 'nhwc')
            b = _run(plan, frames[:2], 'nhwc', misalign=True)
            for i in range(2):
                for li in a[1][i]:
                    assert np.array_equal(a[1][i][li], b[1][i][li]), (i, li)
                assert np.array_equal(_bits(a[0][0][i]), _bits(b[0][0][i]))
    print(f'{name}: {n} tensors compared bit for bit')


def test_gathers_at_odd_ratios_and_offsets():
    """RESIZE_NEAREST 7x9 -> 3x5 and 3x5 -> 7x9, REQUANTIZE through a permutation and a many-to-one table, a CONCAT of (5, 16, 3)
    channels (offsets 0, 5, 21) uploaded into a 3x3 conv; the concat itself is also dequantised, so its bytes are an output."""
    with _plan('gather') as plan:
        n = _check_case(plan, 'gather')
    print(f'gather: {n} tensors compared bit for bit')


@pytest.mark.parametrize('name', sorted(ks.DEEP))
def test_deep_k_with_the_operands_at_the_ends_of_int8(name):
    """Dense 3x3 with C = 768 (K = 6912) and C = 3072 (K = 27648, the limit), weights all 255 / all 0 / random against frames all 255 /
    all 0 / random: the int32 MFMA sum and the sum(x') reduction at their largest, on the vector (nhwc) and the byte (chw) loader."""
    with _plan(name) as plan:
        n = _check_case(plan, name) + _check_case(plan, name, 'chw')
    print(f'{name}: {n} tensors compared bit for bit')


def test_dequantize_rounds_twice():
    """Every q in 0..255 (257 elements) through a (scale, bias) for which q*scale + bias rounded once differs from the two roundings of
    kpu_ref: a build that contracts the multiply and the add into a fused multiply-add fails here."""
    scale, bias, diff = ks.fma_sensitive_dequant()
    with _plan('dequant') as plan:
        n = _check_case(plan, 'dequant')
        _, frames, _ = ks.case('dequant')
        outs, layers = _run(plan, frames[:1])
    q = layers[0][0].ravel()
    assert np.array_equal(np.unique(q), np.arange(256)) and q.size == 257
    once = (q.astype(np.float64) * np.float64(scale) + np.float64(bias)).astype(np.float32)
    assert (_bits(outs[0][0].ravel()) != _bits(once)).sum() >= len(diff) >= 1
    print(f'dequant: {n} tensors compared bit for bit, {len(diff)} of 256 q tell one rounding from two')


def test_batches_are_independent_on_a_reused_arena():
    """max_batch = 5 on the gather model: five frames, then two other frames on the same plan must equal a fresh max_batch = 2 plan's
    (nothing stale is read), and image i of the batch must equal the same image run alone."""
    model, _, _ = ks.case('gather')
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (7, 4, 7, 9), dtype=np.uint8)
    frames[3] = np.where(rng.random((4, 7, 9)) < 0.1, 255, 0)
    refs = []
    for f in frames:
        keep = {}
        refs.append((kpu_ref.run(model, f, keep), keep))

    def same(outs, layers, j, fi, tag):
        for li, q in refs[fi][1].items():
            assert np.array_equal(layers[j][li], q), (tag, fi, li)
        for o, r in zip(outs, refs[fi][0]):
            assert np.array_equal(_bits(o[j]), _bits(r)), (tag, fi)
        return len(refs[fi][1]) + len(refs[fi][0])

    n = 0
    with _plan('gather', 5) as plan, _plan('gather', 2) as fresh, _plan('gather', 1) as single:
        five = _run(plan, frames[:5])
        for j in range(5):
            n += same(*five, j, j, 'five')
        two = _run(plan, frames[5:])
        other = _run(fresh, frames[5:])
        for j in range(2):
            n += same(*two, j, 5 + j, 'two after five')
            n += same(*other, j, 5 + j, 'fresh two')
            for li in two[1][j]:
                assert np.array_equal(two[1][j][li], other[1][j][li])
            for a, b in zip(two[0], other[0]):
                assert np.array_equal(_bits(a[j]), _bits(b[j]))
        for j in range(5):
            alone = _run(single, frames[j:j + 1])
            n += same(*alone, 0, j, 'alone')
            for li in alone[1][0]:
                assert np.array_equal(alone[1][0][li], five[1][j][li]), (j, li)
            for a, b in zip(alone[0], five[0]):
                assert np.array_equal(_bits(a[0]), _bits(b[j])), j
    print(f'batches: {n} tensors compared bit for bit')


def test_the_k_limit_at_create_time():
    """C*k*k = 27648 is accepted (and runs, above); 27648 + 9 is refused."""
    from k210_yolo_framework_amd import engine
    model, _, _ = ks.case('deep_c3072_wrandom')
    assert model.convs[0].in_ch * 9 == 27648
    with engine.KpuPlan(model, max_batch=1) as plan:
        assert len(plan.launches()) == 2
    over, _, _ = ks.case('over_k')
    assert over.convs[0].in_ch * 9 == 27648 + 9
    prog = kmodel.pack_kpu(over)                                                 # the packer lays it out; the plan refuses it
    with pytest.raises(engine.YkError, match='exact int32 range'):
        engine.KpuPlan(prog, max_batch=1)
    with pytest.raises(engine.YkError, match='exact int32 range'):
        engine.KpuPlan(over, max_batch=1)
