"""CPU half of the KPU shape tests: every synthetic kmodel of tests/kpu_synth.py (the ones tests/test_gpu_kpu_shapes.py runs) packs,
survives serialise -> parse with an identical program, is live, and exercises on the oracle alone what its GPU case claims."""
import copy

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel
from oracle import kpu_ref
from tests import kpu_synth as ks

ALL = sorted(ks.CASES)
FILE_MAX_CHANNELS = 1024                                                          # i_ch_num / o_ch_num are 10-bit register fields


def _same_program(a, b):
    return (np.array_equal(a.ops, b.ops) and np.array_equal(a.values, b.values) and np.array_equal(a.outputs, b.outputs)
            and a.blob.tobytes() == b.blob.tobytes() and a.input_chw == b.input_chw and a.conv_values == b.conv_values)


@pytest.mark.parametrize('name', ALL)
def test_packs_and_survives_the_file_format(name):
    model, frames, _ = ks.case(name)
    prog = kmodel.pack_kpu(model)
    assert prog.input_chw == frames.shape[1:]
    assert sorted(prog.conv_values) == [c.index for c in model.convs]
    if max(c.in_ch for c in model.convs) > FILE_MAX_CHANNELS:
        # 3072 input channels run in the KPU-exact mode (K = 27648, the limit) but do not fit the file's 10-bit channel field
        with pytest.raises(kmodel.KmodelError, match='i_ch_num outside its 10-bit field'):
            kmodel.serialise(model)
        return
    again = kmodel.parse(kmodel.serialise(model))
    assert _same_program(kmodel.pack_kpu(again), prog)
    for f in frames:                                                             # and the parsed file computes the same thing
        for a, b in zip(kpu_ref.run(again, f), kpu_ref.run(model, f)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('name', ALL)
def test_every_layer_is_live_and_the_builders_forward_is_the_oracles(name):
    model, frames, _ = ks.case(name)
    ks.check_live(model, frames[0])                                              # asserts the condition
    # the calibrator's restatement of the arithmetic agrees with kpu_ref on every frame (two statements, one answer)
    for f in frames:
        _, keep, seen = ks.trace(model, f)
        for c in model.convs:
            assert np.array_equal(ks.conv_forward(c, seen[c.index][None])[0], keep[c.index]), (name, c.index)


def test_liveness_refuses_a_saturated_layer():
    model, frames, _ = ks.case('m255')
    dead = copy.deepcopy(model)
    dead.convs[1].act_mul[:] = 0
    dead.convs[1].act_bias[:] = 127
    with pytest.raises(AssertionError):
        ks.check_live(dead, frames[0])
    few = copy.deepcopy(model)
    few.convs[1].act_start[3:] = (1 << 35) - 1                                   # three segments only
    with pytest.raises(AssertionError):
        ks.check_live(few, frames[0])


def _border(c):
    """Output pixels of a 3x3 conv whose window reaches outside the input."""
    s = 2 if c.pool_type == kmodel.POOL_LEFT_TOP_2_S2 else 1
    oy, ox = np.arange(c.out_h) * s, np.arange(c.out_w) * s
    by, bx = (oy == 0) | (oy == c.in_h - 1), (ox == 0) | (ox == c.in_w - 1)
    return by[:, None] | bx[None, :]


@pytest.mark.parametrize('name', ALL)
def test_pad_value_reaches_the_border_and_only_the_border(name):
    model, frames, _ = ks.case(name)
    _, keep, seen = ks.trace(model, frames[0])
    for c in model.convs:
        if c.ksize != 3:
            continue
        changed = np.zeros((c.out_h, c.out_w), bool)
        for step in (-1, 1):
            if not 0 <= c.pad_value + step <= 255:
                continue
            other = copy.copy(c)
            other.pad_value = c.pad_value + step
            changed |= (kpu_ref.conv(other, seen[c.index]) != keep[c.index]).any(0)
        border = _border(c)
        assert changed[border].any() and not changed[~border].any(), (name, c.index)


@pytest.mark.parametrize('name', sorted(ks.STRIDE2))
def test_odd_sided_stride_2_layers_read_the_last_row_and_column(name):
    model, frames, _ = ks.case(name)
    _, keep, seen = ks.trace(model, frames[0])
    odd = 0
    for c in model.convs:
        assert c.pool_type == kmodel.POOL_LEFT_TOP_2_S2 and (c.out_h, c.out_w) == ((c.in_h + 1) // 2, (c.in_w + 1) // 2)
        x = seen[c.index]
        if c.in_h % 2:
            x2 = x.copy()
            x2[:, -1, :] ^= 0x80
            d = kpu_ref.conv(c, x2) != keep[c.index]
            assert d[:, -1, :].any(), (name, c.index)
            odd += 1
        if c.in_w % 2:
            x2 = x.copy()
            x2[:, :, -1] ^= 0x80
            d = kpu_ref.conv(c, x2) != keep[c.index]
            assert d[:, :, -1].any(), (name, c.index)
            odd += 1
    assert odd >= 2


def test_the_three_stride_2_forms_are_all_there():
    model, _, _ = ks.case('s2_13x19')
    assert {(c.ksize, c.depthwise) for c in model.convs} == {(3, False), (3, True), (1, False), (1, True)}
    assert [(c.in_h, c.in_w) for c in model.convs] == [(13, 19), (7, 10), (4, 5), (2, 3)]


def test_the_dequantise_case_tells_a_fused_multiply_add_from_two_roundings():
    scale, bias, diff = ks.fma_sensitive_dequant()
    assert len(diff) >= 1
    model, frames, _ = ks.case('dequant')
    deq = [l for l in model.layers if isinstance(l, kmodel.MemLayer)][-1].fields
    assert np.float32(deq['scale']) == scale and np.float32(deq['bias']) == bias
    out, keep, _ = ks.trace(model, frames[0])
    q = keep[0].ravel()
    assert q.size % 2 == 1 and np.array_equal(np.unique(q), np.arange(256))        # every q, an odd count
    assert np.array_equal(q, frames[0].ravel())                                  # the conv in front is the identity
    once = (q.astype(np.float64) * np.float64(scale) + np.float64(bias)).astype(np.float32)
    twice = out[-1].ravel()
    assert np.array_equal(twice.view(np.uint32), (q.astype(np.float32) * scale + bias).astype(np.float32).view(np.uint32))
    assert (twice.view(np.uint32) != once.view(np.uint32)).sum() >= len(diff)


def test_the_gather_case_has_the_shapes_it_claims():
    model, _, _ = ks.case('gather')
    prog = kmodel.pack_kpu(model)
    g = prog.ops[prog.ops[:, kmodel.KF_OP] == kmodel.KPU_OP_GATHER]
    shapes = [(tuple(prog.values[r[kmodel.KF_IN], :3]), tuple(prog.values[r[kmodel.KF_OUT], :3])) for r in g]
    assert ((16, 7, 9), (16, 3, 5)) in shapes and ((16, 3, 5), (16, 7, 9)) in shapes       # nearest resize down and up, no integer ratio
    assert sorted(g[:, kmodel.KF_C_OFF]) == [0, 0, 0, 0, 0, 5, 21]                      # the concat parts start at channels 0, 5, 21
    assert (g[:, kmodel.KF_TABLE_OFF] >= 0).sum() == 2
    assert len(np.unique(ks.PERMUTATION)) == 256 and len(np.unique(ks.MANY_TO_ONE)) < 64
    last = model.convs[-1]
    assert (last.in_ch, last.in_h, last.in_w) == (24, 7, 9)                            # the upload feeds the last conv


def test_the_k_limit_packs_on_both_sides():
    """C*k*k = 27648 is the deepest dense conv yk_kpu_plan_create takes; 27648 + 9 still packs (the packer only lays weights out) and is
    refused at create time, which tests/test_gpu_kpu_shapes.py checks."""
    for name, k_real in (('deep_c3072_wrandom', 27648), ('over_k', 27657)):
        model, _, _ = ks.case(name)
        c = model.convs[0]
        assert c.in_ch * c.ksize ** 2 == k_real
        prog = kmodel.pack_kpu(model)
        r = prog.ops[0]
        cq = (c.in_ch + 15) // 16
        assert r[kmodel.KF_W_BYTES] == 32 * ((9 * cq + 3) // 4 * 64)
