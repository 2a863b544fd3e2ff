"""CPU half of the KPU-exact mode: kmodel.pack_kpu lowers a parsed kmodel v3 to the program yk_kpu_plan_create takes,
resolving KPU-RAM and main-memory addresses as oracle/kpu_ref.run does, and refuses what the kernels do not implement.  The GPU run is
tests/test_gpu_kpu.py."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / 'tests' / 'golden'
LIB = ROOT / 'k210_yolo_framework_amd' / 'csrc' / 'libyolo_hip.so'


@pytest.fixture(scope='module')
def km():
    return kmodel.parse((GOLD / 'yolo.kmodel').read_bytes())


def test_packer_resolves_every_address_of_the_demo_model(km):
    prog = kmodel.pack_kpu(km)
    ops, vals = prog.ops, prog.values
    assert ops.shape[1] == kmodel.KPU_FIELDS and vals.shape[1] == 4
    assert prog.input_chw == (3, 224, 320)
    # every conv is an op whose output is a value of the layer's shape; the first one reads the frame
    convs = km.convs
    assert sorted(prog.conv_values) == [c.index for c in convs]
    for c in convs:
        v = prog.conv_values[c.index]
        assert tuple(vals[v]) == (c.out_ch, c.out_h, c.out_w, kmodel.KPU_U8)
    conv_rows = ops[np.isin(ops[:, kmodel.KF_OP], (kmodel.KPU_OP_CONV, kmodel.KPU_OP_DWCONV))]
    assert len(conv_rows) == 32 and conv_rows[0, kmodel.KF_IN] == -1 and (conv_rows[1:, kmodel.KF_IN] >= 0).all()
    assert (conv_rows[:, kmodel.KF_OP] == kmodel.KPU_OP_DWCONV).sum() == sum(c.depthwise for c in convs)
    # every op reads a value an earlier op wrote (or the frame), every value is written
    written = set()
    for r in ops:
        assert r[kmodel.KF_IN] == -1 or r[kmodel.KF_IN] in written, r
        written.add(int(r[kmodel.KF_OUT]))
    assert written == set(range(len(vals)))
    # the head: conv 36 reads the upload of the concat [requantised upsampled conv 30 | requantised conv 22] (512 channels)
    src36 = int(ops[ops[:, kmodel.KF_LAYER] == 36][0, kmodel.KF_IN])
    assert tuple(vals[src36]) == (512, 14, 20, kmodel.KPU_U8)
    parts = ops[(ops[:, kmodel.KF_OUT] == src36)]
    assert list(parts[:, kmodel.KF_C_OFF]) == [0, 128] and (parts[:, kmodel.KF_OP] == kmodel.KPU_OP_GATHER).all()
    # the two outputs are dequantised fp32 tensors of the yolo head's shape
    assert prog.output_shapes() == [(75, 7, 10), (75, 14, 20)]
    assert (vals[prog.outputs, 3] == kmodel.KPU_F32).all()
    # blob offsets: 16-byte aligned and inside the blob
    for r in conv_rows:
        for off in (kmodel.KF_W_OFF, kmodel.KF_CH_OFF, kmodel.KF_SEG_OFF):
            assert r[off] % 16 == 0 and 0 <= r[off] < prog.blob.size
        assert r[kmodel.KF_W_OFF] + r[kmodel.KF_W_BYTES] <= prog.blob.size


def test_dense_weights_are_packed_as_signed_offsets_per_tap(km):
    """Dense conv weights: int8 w' = w - 128, [oc (padded to 32)][tap][channel (padded to 16)], zero padding; the per-channel constant
    row carries (arg_w*sum(w) >> shr_w) + arg_add*in_channels and 128*sum(w)."""
    prog = kmodel.pack_kpu(km)
    c = km.convs[0]                                                          # the 3-channel stem: 9 taps x 16 channels
    r = prog.ops[prog.ops[:, kmodel.KF_LAYER] == c.index][0]
    wb = prog.blob[r[kmodel.KF_W_OFF]:r[kmodel.KF_W_OFF] + r[kmodel.KF_W_BYTES]].view(np.int8).reshape(32, -1)
    assert wb.shape[1] == 192                                                # 9*16 = 144 -> three 64-wide chunks
    t = wb[:c.out_ch, :144].reshape(c.out_ch, 9, 16).astype(np.int64)
    np.testing.assert_array_equal(t[:, :, :3], c.weights.astype(np.int64).transpose(0, 2, 1) - 128)
    assert not t[:, :, 3:].any() and not wb[c.out_ch:].any() and not wb[:, 144:].any()
    ch = prog.blob[r[kmodel.KF_CH_OFF]:r[kmodel.KF_CH_OFF] + 64 * c.out_ch].view(np.int64).reshape(c.out_ch, 8)
    sw = c.weights.astype(np.int64).reshape(c.out_ch, -1).sum(1)
    np.testing.assert_array_equal(ch[:, 0], ((c.arg_w * sw) >> c.shr_w) + c.arg_add * c.in_ch)
    np.testing.assert_array_equal(ch[:, 1], 128 * sw)
    np.testing.assert_array_equal(ch[:, 2:5], np.stack([c.bn_mul, c.bn_add, c.bn_shift], 1))


def test_unsupported_pool_type_raises(km):
    m = copy.deepcopy(km)
    m.convs[4].pool_type = 1
    with pytest.raises(kmodel.KmodelError, match='pool type'):
        kmodel.pack_kpu(m)


def test_unsupported_layer_type_raises(km):
    m = copy.deepcopy(km)
    mem = [l for l in m.layers if isinstance(l, kmodel.MemLayer)]
    mem[1].type = 2                                                          # not a layer type of the K210 runtime's v3 set here
    with pytest.raises(kmodel.KmodelError, match='does not implement'):
        kmodel.pack_kpu(m)


@pytest.mark.parametrize('field,value', [('ksize', 5), ('act_shift', 256), ('arg_add', 1 << 39), ('bn_shift', 16)])
def test_fields_the_kpu_cannot_hold_raise(km, field, value):
    m = copy.deepcopy(km)
    c = m.convs[2]
    cur = getattr(c, field)
    setattr(c, field, np.full_like(cur, value) if isinstance(cur, np.ndarray) else value)
    with pytest.raises(kmodel.KmodelError):
        kmodel.pack_kpu(m)


def test_unresolved_addresses_raise(km):
    m = copy.deepcopy(km)
    m.convs[5].src_addr = 12345                                              # no layer writes this KPU address
    with pytest.raises(kmodel.KmodelError, match='KPU address'):
        kmodel.pack_kpu(m)
    m = copy.deepcopy(km)
    m.outputs = [(99999, 4)]
    with pytest.raises(kmodel.KmodelError, match='main-memory address'):
        kmodel.pack_kpu(m)


def test_library_exports_the_kpu_entry_points():
    if not LIB.exists():
        import __graft_entry__ as g
        g.build()
    import torch  # noqa: F401  (first, as engine.lib() does)
    dll = C.CDLL(str(LIB))
    for f in ('yk_kpu_plan_create', 'yk_kpu_plan_destroy', 'yk_kpu_run_u8', 'yk_kpu_get_output', 'yk_kpu_debug_read',
              'yk_kpu_output_count', 'yk_kpu_launch_count', 'yk_kpu_profile'):
        assert hasattr(dll, f), f
