"""The kmodel v3 writer (kmodel.serialise / write / conv_registers / allocate_kpu_ram) against the K210 demo's own file, which is the same
network (yolo_mobilev1-0.75, 224x320) nncase v0.1 emitted: tests/golden/yolo.kmodel."""
import dataclasses
import json
import struct
import subprocess
import sys
import zipfile
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import kmodel, netspec as ns, quantize
from oracle import kpu_ref

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).parent / 'golden'


@pytest.fixture(scope='module')
def demo_bytes():
    return (GOLD / 'yolo.kmodel').read_bytes()


@pytest.fixture(scope='module')
def demo(demo_bytes):
    return kmodel.parse(demo_bytes)


def _same(a, b, path=''):
    if dataclasses.is_dataclass(a):
        assert type(a) is type(b), path
        for f in dataclasses.fields(a):
            _same(getattr(a, f.name), getattr(b, f.name), f'{path}.{f.name}')
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same(a[k], b[k], f'{path}[{k}]')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{path}[{i}]')
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), path
    else:
        assert a == b and type(a) is type(b), (path, a, b)


def test_round_trip_of_the_demo_is_equal_in_every_field_and_bit_identical_on_the_oracle(demo, demo_bytes):
    again_bytes = kmodel.serialise(demo)
    again = kmodel.parse(again_bytes)
    _same(demo, again)                                     # header (version, main_mem_usage, output table) and every field of every layer
    assert struct.unpack_from('<7I', again_bytes) == struct.unpack_from('<7I', demo_bytes)
    assert kmodel.main_mem_usage(demo) == demo.main_mem_usage
    assert again_bytes == demo_bytes                       # with nncase's addresses kept, the writer reproduces the file byte for byte
    img = np.load(GOLD / 'kmodel_dog_golden.npz')['image']
    for a, b in zip(kpu_ref.run(demo, img), kpu_ref.run(again, img)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _file_registers(data):
    _, _, _, nl, _, _, nout = struct.unpack_from('<7I', data, 0)
    off = 28 + 8 * nout
    pos = off + 8 * nl
    regs = {}
    for i in range(nl):
        ty, sz = struct.unpack_from('<2I', data, off + 8 * i)
        if ty == kmodel.KL_K210_CONV:
            lo = struct.unpack_from('<6I', data, pos)[2]
            regs[i] = list(struct.unpack_from('<12Q', data, lo))
        pos += sz
    return regs


def test_registers_of_every_demo_conv_are_regenerated_bit_for_bit(demo, demo_bytes):
    """Outside the KPU-RAM source / destination address fields, and outside kmodel.UNDERIVED_REGISTER_FIELDS - which is empty."""
    assert kmodel.UNDERIVED_REGISTER_FIELDS == {}
    masked = kmodel.register_field_mask({**kmodel.KPU_ADDRESS_FIELDS, **kmodel.UNDERIVED_REGISTER_FIELDS})
    assert [hex(m) for m in masked] == [hex(((1 << 15) - 1) | (((1 << 15) - 1) << 32)) if r == 1 else '0x0' for r in range(12)]
    file_regs = _file_registers(demo_bytes)
    assert len(file_regs) == len(demo.convs) == 32          # conv1, 13 dw + pw pairs, 5 head convs: every KPU conv of the file
    for c in demo.convs:
        moved = dataclasses.replace(c, src_addr=(c.src_addr * 7 + 13) % 32768, dst_addr=(c.dst_addr * 5 + 1) % 32768)   # addresses do not leak elsewhere
        for got, own in ((kmodel.conv_registers(c), True), (kmodel.conv_registers(moved), False)):
            for r in range(12):
                keep = ~masked[r] & ((1 << 64) - 1)
                assert got[r] & keep == file_regs[c.index][r] & keep, (c.index, r, hex(got[r]), hex(file_regs[c.index][r]))
                if own:
                    assert got[r] == file_regs[c.index][r]


def _check_allocation(km):
    """bounds, no input / output overlap, nothing still to be read is overwritten: replay the layers over an interval map."""
    live = {}                                              # start -> (end, tensor id)
    first = True
    convs = km.convs
    n_reads = {}
    for l in km.layers:                                    # who reads each (address, generation)
        pass
    gen = {}
    def write(addr, units, who):
        assert 0 <= addr and addr + units <= kmodel.KPU_RAM_UNITS, (who, addr, units)
        for a, (e, t) in list(live.items()):
            if a < addr + units and addr < e:
                assert t not in pending, f'layer {who} overwrites tensor {t}, which a later layer still reads'
                del live[a]
        live[addr] = (addr + units, who)
    # pending = tensors with readers still to come: computed from a forward scan of (address -> last writer)
    readers, writer_at = {}, {}
    for l in km.layers:
        if isinstance(l, kmodel.ConvLayer):
            if first:
                writer_at[l.src_addr] = 'frame'
                first = False
            readers.setdefault(writer_at[l.src_addr], []).append(l.index)
            writer_at[l.dst_addr] = l.index
        elif l.type == kmodel.KL_K210_UPLOAD:
            writer_at[l.fields['kpu_addr']] = l.index
    pending = set()
    first = True
    for l in km.layers:
        if isinstance(l, kmodel.ConvLayer):
            iu = kmodel.kpu_tensor_units(l.in_ch, l.in_h, l.in_w)
            ou = kmodel.kpu_tensor_units(l.out_ch, l.out_h, l.out_w)
            if first:
                write(l.src_addr, iu, 'frame')
                pending.add('frame')
                first = False
            assert l.src_addr in live and live[l.src_addr][0] == l.src_addr + iu, (l.index, 'its input is no longer intact')
            assert l.src_addr + iu <= l.dst_addr or l.dst_addr + ou <= l.src_addr, (l.index, 'input and output overlap')
            src_t = live[l.src_addr][1]
            write(l.dst_addr, ou, l.index)                 # the input is still pending here: overwriting it asserts
            readers[src_t].remove(l.index)
            if not readers[src_t]:
                pending.discard(src_t)
            if readers.get(l.index):
                pending.add(l.index)
        elif l.type == kmodel.KL_K210_UPLOAD:
            f = l.fields
            write(f['kpu_addr'], kmodel.kpu_tensor_units(f['channels'], f['height'], f['width']), l.index)
            if readers.get(l.index):
                pending.add(l.index)
    assert not pending


def _model(alpha, seed=5, hw=(224, 320)):
    spec = ns.yolo_mobilev1((*hw, 3), 3, 20, alpha=alpha)
    w = spec.init_weights(seed)
    names = quantize.tensor_names(spec)
    rng = np.random.default_rng(seed)
    ranges = {n: (-float(rng.uniform(0.5, 3)), float(rng.uniform(2, 9))) for n in names}
    for op in spec.ops:
        if op['act'] == ns.ACT_RELU:
            ranges[op['layer']] = (0.0, ranges[op['layer']][1])
        elif op['act'] == ns.ACT_LEAKY:                    # a LeakyReLU output reaches alpha times as far down as its input does
            ranges[op['layer']] = (-op['alpha'] * ranges[op['layer']][1] * float(rng.uniform(0.5, 1.5)), ranges[op['layer']][1])
    return spec, w, ranges


@pytest.mark.parametrize('alpha', [0.75, 0.5])
def test_kpu_ram_allocator_constraints_on_the_demo_geometry_and_depth_multiplier_half(alpha, demo):
    _check_allocation(demo)                                # the checker accepts nncase's own placement
    spec, w, ranges = _model(alpha)
    km, rep = quantize.quantize(spec, w, ranges)
    _check_allocation(km)
    assert rep['kpu_ram_peak'] <= kmodel.KPU_RAM_BYTES
    kmodel.pack_kpu(km)
    if alpha == 0.75:                                      # the same layer sequence as the demo: types, geometry, pooling, flags
        assert [type(a) for a in km.layers] == [type(a) for a in demo.layers]
        for a, b in zip(km.layers, demo.layers):
            if isinstance(a, kmodel.ConvLayer):
                for f in ('flags', 'in_ch', 'out_ch', 'in_w', 'in_h', 'out_w', 'out_h', 'ksize', 'pool_type', 'depthwise'):
                    assert getattr(a, f) == getattr(b, f), (a.index, f)
            else:
                assert a.type == b.type and a.fields['flags'] == b.fields['flags']


def test_the_allocator_catches_a_clobbered_tensor(demo):
    """The checker above is not vacuous: moving one output onto a tensor still to be read fails it."""
    bad = kmodel.parse((GOLD / 'yolo.kmodel').read_bytes())
    c28 = next(c for c in bad.convs if c.index == 28)      # head_conv_2 writes while conv_pw_13's output (at 2688) waits for head_conv_3 (layer 30)
    c28.dst_addr = 2688 + 8
    with pytest.raises(AssertionError, match='still reads'):
        _check_allocation(bad)


def test_allocator_refuses_what_does_not_fit():
    with pytest.raises(kmodel.KmodelError, match='KPU RAM'):
        kmodel.allocate_kpu_ram([20000, 20000], [0, 0], [1, 1])
    with pytest.raises(kmodel.KmodelError, match='exceeds the KPU RAM'):
        kmodel.allocate_kpu_ram([40000], [0], [0])
    assert kmodel.allocate_kpu_ram([100, 200, 100], [0, 0, 1], [0, 1, 2]) == [0, 32768 - 200, 0]


def test_kfpkg_reads_back_and_carries_the_model_at_the_demo_address(tmp_path, demo, demo_bytes):
    n = kmodel.write(tmp_path / 'm.kfpkg', demo)
    assert n == len(demo_bytes)
    assert kmodel.read_kfpkg(tmp_path / 'm.kfpkg') == demo_bytes
    with zipfile.ZipFile(tmp_path / 'm.kfpkg') as z:
        assert sorted(z.namelist()) == ['flash-list.json', 'yolo.kmodel']          # no firmware binary
        fl = json.loads(z.read('flash-list.json'))
    assert fl['files'] == [{'address': 0x00A00000, 'bin': 'yolo.kmodel', 'sha256Prefix': False}]
    assert 'firmware' in kmodel.write.__doc__
    kmodel.write(tmp_path / 'm.kmodel', demo)
    assert (tmp_path / 'm.kmodel').read_bytes() == demo_bytes


def test_make_kmodel_help_lists_the_flags():
    out = subprocess.run([sys.executable, str(ROOT / 'make_kmodel.py'), '--help'], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    for flag in ('--calib', '--synthetic', '--calib_seed', '--model_def', '--depth_multiplier', '--image_size', '--output_size', '--class_num',
                 '--train_set'):
        assert flag in out.stdout, flag


def test_a_field_forced_past_its_width_is_refused(demo):
    c = dataclasses.replace(demo.convs[3], arg_add=1 << 39)
    with pytest.raises(kmodel.KmodelError, match='arg_add outside its 40-bit field'):
        kmodel.conv_registers(c)
    c = dataclasses.replace(demo.convs[3], out_ch=1025)
    with pytest.raises(kmodel.KmodelError, match='o_ch_num'):
        kmodel.conv_registers(c)
    bad = kmodel.parse((GOLD / 'yolo.kmodel').read_bytes())
    bad.convs[0].bn_mul = bad.convs[0].bn_mul.copy()
    bad.convs[0].bn_mul[2] = 1 << 23
    with pytest.raises(kmodel.KmodelError, match='bn_mul outside its 24-bit field'):
        kmodel.serialise(bad)
