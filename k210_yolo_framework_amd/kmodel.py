"""K210 kmodel (v3) reader and writer (`parse` / `serialise`, `write`; the quantiser that fills a model is quantize.py).  Reader: recover the trained, 8-bit quantised yolo_mobilev1-0.75 of the reference's K210 demo as Keras-named
float weights this framework can run.

The only trained weights in the reference tree are inside `yolo3_frame_test_public/kfpkg/kpu_yolov3.kfpkg` (a zip): `yolo.kmodel`,
3 926 440 bytes, flashed at 0x00A00000 and run by `main.c:274,303` through the Kendryte SDK's `kpu_load_kmodel / kpu_run_kmodel`.
The container is nncase v0.1's "kmodel v3" (third party, un-vendored; restated here from the published Kendryte standalone SDK
`kpu.h` / `kpu.c` and nncase's K210 kernels):

    header   7 x u32   version(3) flags arch layers_length max_start_address main_mem_usage output_count
    outputs  output_count x (address, size)                  in main memory
    layers   layers_length x (type, body_size)               then the bodies, back to back
    K210 conv body (type 10240): flags, main_mem_out_address, layer_offset, weights_offset, bn_offset, act_offset (file offsets)
        layer:   twelve 64-bit KPU registers (kpu_layer_argument_t): channels-1, sizes-1, kernel 1x1/3x3, pool type, pad value, depthwise
                 bit, and the zero-point terms arg_x >> shr_x, arg_w >> shr_w, arg_add
        weights: uint8 [oc][ic][kh*kw] (depthwise: [c][kh*kw])
        bn:      one u64 per output channel: mul:24 add:32 shift:4
        act:     16 segments (shift:8, y_mul:16, x_start:36 signed) + 16 result biases: a piecewise-linear table in the integer domain
    main-memory layers: DEQUANTIZE(12), REQUANTIZE(13, 256-entry table), QUANTIZED_CONCAT(17), QUANTIZED_RESIZE_NEAREST_NEIGHBOR(23),
        K210_UPLOAD(10243)

The KPU computes, per output (nncase `kpu_conv2d`):
    acc = sum(x*w) + (arg_x * sum(x) >> shr_x) + (arg_w * sum(w) >> shr_w) + arg_add * in_channels_per_group     x, w uint8; pad = pad_value
    z   = (acc * bn.mul >> bn.shift) + bn.add
    y   = clamp(((z - seg.x_start) * seg.y_mul >> seg.shift) + seg.bias, 0, 255)        seg = last segment with z > x_start
which is the asymmetric-quantised form of  y_real = act(bn(sum(x_real * w_real)))  with x_real = s_x (x - zp_x), w_real = s_w (w - zp_w),
zp_x = -arg_w / 2^shr_w and zp_w = -arg_x / 2^shr_x.  `to_float_weights` re-expresses every layer in CENTRED integer units
(x~ = x - zp_x, w~ = w - zp_w: real zero is zero, so Keras zero padding is right) and folds the BN multiplier, the activation table's
slope and the requantisation factors into a per-channel (scale, bias) + LeakyReLU(alpha) - exactly the layer form of
`models/yolonet.py:12-43` / `keras_mobilenet.py:291-436`, so the result loads into `yolonet.yolo_mobilev1` under the Keras names.
What is lost: the 8-bit rounding and range clipping of every activation (the float network is the un-clipped one).

`oracle/kpu_ref.py` (test infrastructure) runs the integer pipeline above bit by bit; `tests/test_kmodel.py` checks this module
against it and against the known answer of the demo picture (`kfpkg/dog.jpg` -> dog, bicycle, car; README.md:121-128,166).
"""
from __future__ import annotations

import io
import struct
import zipfile
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

KL_DEQUANTIZE, KL_REQUANTIZE, KL_QUANTIZED_CONCAT, KL_QUANTIZED_RESIZE_NN = 12, 13, 17, 23
KL_K210_CONV, KL_K210_UPLOAD = 10240, 10243
KLF_MAIN_MEM_OUT = 1
POOL_BYPASS, POOL_LEFT_TOP_2_S2 = 0, 5


class KmodelError(ValueError):
    pass


def _bits(v: int, lo: int, n: int, signed: bool = False) -> int:
    x = (v >> lo) & ((1 << n) - 1)
    if signed and x >> (n - 1):
        x -= 1 << n
    return x


@dataclass
class ConvLayer:
    index: int
    flags: int
    main_mem_out: int
    src_addr: int
    dst_addr: int
    in_ch: int
    out_ch: int
    in_w: int
    in_h: int
    out_w: int
    out_h: int
    ksize: int                    # 1 or 3
    pool_type: int
    pad_value: int
    depthwise: bool
    shr_w: int
    shr_x: int
    arg_w: int
    arg_x: int
    arg_add: int
    weights: np.ndarray           # uint8 [oc][ic][k*k] (depthwise: [c][1][k*k])
    bn_mul: np.ndarray            # int64 [oc]
    bn_add: np.ndarray
    bn_shift: np.ndarray
    act_start: np.ndarray         # int64 [16]
    act_mul: np.ndarray
    act_shift: np.ndarray
    act_bias: np.ndarray          # int64 [16]

    @property
    def zp_x(self) -> float:
        return -self.arg_w / float(1 << self.shr_w)

    @property
    def zp_w(self) -> float:
        return -self.arg_x / float(1 << self.shr_x)


@dataclass
class MemLayer:
    index: int
    type: int
    fields: dict


@dataclass
class Kmodel:
    version: int
    main_mem_usage: int
    outputs: List[Tuple[int, int]]
    layers: List[object] = field(default_factory=list)

    @property
    def convs(self) -> List[ConvLayer]:
        return [l for l in self.layers if isinstance(l, ConvLayer)]


def read_kfpkg(path) -> bytes:
    """The `yolo.kmodel` member of a .kfpkg (a zip with flash-list.json)."""
    with zipfile.ZipFile(path) as z:
        names = [n for n in z.namelist() if n.endswith('.kmodel')]
        if not names:
            raise KmodelError(f'{path}: no .kmodel member')
        return z.read(names[0])


def parse(data: bytes) -> Kmodel:
    if len(data) < 28:
        raise KmodelError('kmodel: truncated header')
    ver, _flags, _arch, nl, _maxstart, mainmem, nout = struct.unpack_from('<7I', data, 0)
    if ver != 3:
        raise KmodelError(f'kmodel: version {ver} (only v3, nncase 0.1, is understood)')
    off = 28
    if nout > 64 or nl > 4096 or off + 8 * (nout + nl) > len(data):
        raise KmodelError(f'kmodel: header announces {nout} outputs and {nl} layers, the file has {len(data)} bytes')
    outs = [struct.unpack_from('<2I', data, off + 8 * i) for i in range(nout)]
    off += 8 * nout
    hdrs = [struct.unpack_from('<2I', data, off + 8 * i) for i in range(nl)]
    pos = off + 8 * nl
    km = Kmodel(ver, mainmem, [(int(a), int(s)) for a, s in outs])
    for i, (ty, sz) in enumerate(hdrs):
        if pos + sz > len(data):
            raise KmodelError(f'kmodel: layer {i} runs past the end of the file')
        body = data[pos:pos + sz]
        need = {KL_K210_CONV: 24, KL_DEQUANTIZE: 24, KL_REQUANTIZE: 272, KL_QUANTIZED_CONCAT: 12, KL_QUANTIZED_RESIZE_NN: 36, KL_K210_UPLOAD: 24}.get(ty)
        if need is not None and sz < need:
            raise KmodelError(f'kmodel: layer {i} (type {ty}) has a {sz}-byte body, at least {need} expected')
        if ty == KL_K210_CONV:
            km.layers.append(_parse_conv(i, data, body))
        elif ty == KL_DEQUANTIZE:
            fl, src, dst, cnt = struct.unpack_from('<4I', body, 0)
            sc, bs = struct.unpack_from('<2f', body, 16)
            km.layers.append(MemLayer(i, ty, dict(flags=fl, src=src, dst=dst, count=cnt, scale=sc, bias=bs)))
        elif ty == KL_REQUANTIZE:
            fl, src, dst, cnt = struct.unpack_from('<4I', body, 0)
            km.layers.append(MemLayer(i, ty, dict(flags=fl, src=src, dst=dst, count=cnt, table=np.frombuffer(body, np.uint8, 256, 16).copy())))
        elif ty == KL_QUANTIZED_CONCAT:
            fl, dst, n = struct.unpack_from('<3I', body, 0)
            if 12 + 8 * n > sz:
                raise KmodelError(f'kmodel: layer {i}: concat of {n} inputs does not fit its {sz}-byte body')
            ins = [struct.unpack_from('<2I', body, 12 + 8 * k) for k in range(n)]
            km.layers.append(MemLayer(i, ty, dict(flags=fl, dst=dst, inputs=[(int(a), int(s)) for a, s in ins])))
        elif ty == KL_QUANTIZED_RESIZE_NN:
            fl, src, dst, w, h, c, ow, oh, align = struct.unpack_from('<9I', body, 0)
            km.layers.append(MemLayer(i, ty, dict(flags=fl, src=src, dst=dst, in_w=w, in_h=h, channels=c, out_w=ow, out_h=oh, align=align)))
        elif ty == KL_K210_UPLOAD:
            fl, src, kpu, w, h, c = struct.unpack_from('<6I', body, 0)
            km.layers.append(MemLayer(i, ty, dict(flags=fl, src=src, kpu_addr=kpu, width=w, height=h, channels=c)))
        else:
            raise KmodelError(f'kmodel: layer {i} has type {ty}, which this reader does not know')
        pos += sz
    return km


def _parse_conv(index: int, data: bytes, body: bytes) -> ConvLayer:
    fl, mmout, lo, wo, bo, ao = struct.unpack_from('<6I', body, 0)
    # every offset comes out of an untrusted file: check each region against the file before touching it
    n = len(data)
    if lo + 96 > n:
        raise KmodelError(f'kmodel: conv layer {index}: register block at {lo} runs past the end of the file ({n} bytes)')
    if not (wo <= bo <= n):
        raise KmodelError(f'kmodel: conv layer {index}: weight / BatchNorm offsets {wo}, {bo} are out of order or past the end of the file')
    if ao + 128 + 16 > n:
        raise KmodelError(f'kmodel: conv layer {index}: activation table at {ao} runs past the end of the file')
    r = struct.unpack_from('<12Q', data, lo)
    depthwise = bool(_bits(r[0], 3, 1))
    src, dst = _bits(r[1], 0, 15), _bits(r[1], 32, 15)
    ic, oc = _bits(r[2], 0, 10) + 1, _bits(r[2], 32, 10) + 1
    iw, ih = _bits(r[3], 0, 10) + 1, _bits(r[3], 10, 9) + 1
    ow, oh = _bits(r[3], 32, 10) + 1, _bits(r[3], 42, 9) + 1
    ktype, pool, padv = _bits(r[4], 0, 3), _bits(r[4], 4, 4), _bits(r[4], 24, 8)
    ks = 3 if ktype == 1 else 1
    shr_w, shr_x = _bits(r[9], 0, 4), _bits(r[9], 4, 4)
    arg_w, arg_x = _bits(r[9], 8, 24, True), _bits(r[9], 32, 24, True)
    arg_add = _bits(r[10], 0, 40, True)
    nw = oc * ks * ks * (1 if depthwise else ic)
    # (kernel_load_cfg.para_size is the bytes of ONE parameter load; big layers are loaded in several passes of o_ch_num_coef channels)
    if bo - wo < nw:
        raise KmodelError(f'kmodel: conv layer {index}: {bo - wo} weight bytes in the file, {nw} expected (16-bit weights are not supported)')
    if bo + 8 * oc > n:
        raise KmodelError(f'kmodel: conv layer {index}: BatchNorm table of {oc} channels at {bo} runs past the end of the file')
    w = np.frombuffer(data, np.uint8, nw, wo).reshape(oc, 1 if depthwise else ic, ks * ks).copy()
    bn = np.frombuffer(data, '<u8', oc, bo)
    bn_mul = np.array([_bits(int(v), 0, 24, True) for v in bn], np.int64)
    bn_add = np.array([_bits(int(v), 24, 32, True) for v in bn], np.int64)
    bn_shift = np.array([_bits(int(v), 56, 4) for v in bn], np.int64)
    act = np.frombuffer(data, '<u8', 16, ao)
    a_shift = np.array([_bits(int(v), 0, 8) for v in act], np.int64)
    a_mul = np.array([_bits(int(v), 8, 16, True) for v in act], np.int64)
    a_start = np.array([_bits(int(v), 24, 36, True) for v in act], np.int64)
    a_bias = np.frombuffer(data, np.int8, 16, ao + 128).astype(np.int64)
    return ConvLayer(index, fl, mmout, src, dst, ic, oc, iw, ih, ow, oh, ks, pool, padv, depthwise, shr_w, shr_x, arg_w, arg_x, arg_add, w,
                     bn_mul, bn_add, bn_shift, a_start, a_mul, a_shift, a_bias)


# ---- the KPU-exact program (include/yolo_hip.h yk_kpu_plan_create) ------------------------------------------------------------------
KPU_FIELDS = 24                                       # YK_KPU_FIELDS
KPU_OP_CONV, KPU_OP_DWCONV, KPU_OP_GATHER, KPU_OP_DEQUANT = 1, 2, 3, 4
(KF_OP, KF_IN, KF_OUT, KF_K, KF_POOL, KF_PAD, KF_SHR_X, KF_ARG_X, KF_W_OFF, KF_W_BYTES, KF_CH_OFF, KF_SEG_OFF, KF_LAYER, KF_C_OFF,
 KF_TABLE_OFF, KF_SCALE_BITS, KF_BIAS_BITS, KF_IN_C, KF_IN_H, KF_IN_W) = range(20)
KPU_U8, KPU_F32 = 0, 1


@dataclass
class KpuProgram:
    """What yk_kpu_plan_create takes: op rows (int64 [n][KPU_FIELDS]), value shapes (int32 [n][4] = C, H, W, dtype), the fp32 output
    value ids and the byte blob the rows address.  `input_chw` is the frame's shape, `conv_values` maps a conv's kmodel layer index to
    its output value."""
    ops: np.ndarray
    values: np.ndarray
    outputs: np.ndarray
    blob: np.ndarray
    input_chw: Tuple[int, int, int]
    conv_values: Dict[int, int]

    def output_shapes(self) -> List[Tuple[int, int, int]]:
        """(C, H, W) of every output, in kmodel order."""
        return [tuple(int(v) for v in self.values[i, :3]) for i in self.outputs]


def _check_width(c: ConvLayer, name: str, v, bits: int, signed: bool) -> None:
    """A register field must fit the width the KPU gives it (kpu_layer_argument_t; bn / act tables)."""
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    if any(int(x) < lo or int(x) > hi for x in np.ravel(np.asarray(v, dtype=object))):
        raise KmodelError(f'kmodel: conv layer {c.index}: {name} outside its {bits}-bit field')


def pack_kpu(km: Kmodel) -> KpuProgram:
    """Lower a parsed kmodel v3 to the KPU-exact program, resolving the KPU-RAM and main-memory addresses exactly as oracle/kpu_ref.run
    does with its two dicts (a later write to an address replaces the tensor there).  Every tensor becomes a value with its own device
    buffer; KPU convs, REQUANTIZE / RESIZE_NEAREST / CONCAT (gathers) and DEQUANTIZE become ops, K210_UPLOAD only renames.  Raises
    KmodelError for anything the kernels do not implement or the oracle would not run.  CPU only."""
    values: List[Tuple[int, int, int, int]] = []
    rows: List[np.ndarray] = []
    blob = bytearray()
    conv_values: Dict[int, int] = {}

    def new_value(c_, h_, w_, dt):
        values.append((int(c_), int(h_), int(w_), dt))
        return len(values) - 1

    def put(b: bytes) -> int:
        while len(blob) % 64:
            blob.append(0)
        off = len(blob)
        blob.extend(b)
        return off

    def row(**kv):
        r = np.zeros(KPU_FIELDS, np.int64)
        r[KF_TABLE_OFF] = -1
        for k, v in kv.items():
            r[globals()['KF_' + k.upper()]] = int(v)
        rows.append(r)

    def shape(v):
        return values[v][:3]

    kpu: Dict[int, int] = {}
    mem: Dict[int, int] = {}
    first = True
    input_chw = None
    for l in km.layers:
        if isinstance(l, ConvLayer):
            c = l
            if c.ksize not in (1, 3):
                raise KmodelError(f'kmodel: conv layer {c.index}: kernel size {c.ksize} (the KPU has 1x1 and 3x3)')
            if c.pool_type not in (POOL_BYPASS, POOL_LEFT_TOP_2_S2):
                raise KmodelError(f'kmodel: conv layer {c.index}: KPU pool type {c.pool_type} is not implemented (bypass and left_top_2_s2 are)')
            for name, v, bits, signed in (('pad_value', c.pad_value, 8, False), ('shr_x', c.shr_x, 4, False), ('shr_w', c.shr_w, 4, False),
                                          ('arg_x', c.arg_x, 24, True), ('arg_w', c.arg_w, 24, True), ('arg_add', c.arg_add, 40, True),
                                          ('bn_mul', c.bn_mul, 24, True), ('bn_add', c.bn_add, 32, True), ('bn_shift', c.bn_shift, 4, False),
                                          ('act_shift', c.act_shift, 8, False), ('act_mul', c.act_mul, 16, True),
                                          ('act_start', c.act_start, 36, True), ('act_bias', c.act_bias, 8, True)):
                _check_width(c, name, v, bits, signed)
            kk = c.ksize * c.ksize
            w = np.asarray(c.weights)
            if w.dtype != np.uint8 or w.shape != (c.out_ch, 1 if c.depthwise else c.in_ch, kk):
                raise KmodelError(f'kmodel: conv layer {c.index}: weights {w.dtype} {w.shape}')
            for name in ('bn_mul', 'bn_add', 'bn_shift'):
                if np.shape(getattr(c, name)) != (c.out_ch,):
                    raise KmodelError(f'kmodel: conv layer {c.index}: {name} has {np.shape(getattr(c, name))} entries, {c.out_ch} expected')
            for name in ('act_start', 'act_mul', 'act_shift', 'act_bias'):
                if np.shape(getattr(c, name)) != (16,):
                    raise KmodelError(f'kmodel: conv layer {c.index}: {name} has {np.shape(getattr(c, name))} entries, 16 expected')
            if first:
                src = -1
                input_chw = (c.in_ch, c.in_h, c.in_w)
            else:
                if c.src_addr not in kpu:
                    raise KmodelError(f'kmodel: conv layer {c.index} reads KPU address {c.src_addr}, which no earlier layer wrote')
                src = kpu[c.src_addr]
                if values[src][3] != KPU_U8 or shape(src) != (c.in_ch, c.in_h, c.in_w):
                    raise KmodelError(f'kmodel: conv layer {c.index}: input {shape(src)} != ({c.in_ch}, {c.in_h}, {c.in_w})')
            first = False
            H, W = c.in_h, c.in_w
            oh, ow = ((H + 1) // 2, (W + 1) // 2) if c.pool_type == POOL_LEFT_TOP_2_S2 else (H, W)
            if (c.out_h, c.out_w) != (oh, ow) or (c.depthwise and c.out_ch != c.in_ch):
                raise KmodelError(f'kmodel: conv layer {c.index}: output ({c.out_ch}, {c.out_h}, {c.out_w}) does not follow from the input '
                                  f'({c.in_ch}, {H}, {W}) and pool type {c.pool_type}')
            w64 = w.astype(np.int64)
            sum_w = w64.reshape(c.out_ch, -1).sum(1)
            g_ic = 1 if c.depthwise else c.in_ch
            K = kk * g_ic
            ch = np.zeros((c.out_ch, 8), np.int64)
            ch[:, 0] = ((np.int64(c.arg_w) * sum_w) >> np.int64(c.shr_w)) + np.int64(c.arg_add * g_ic)
            if c.depthwise:
                wb = w.reshape(c.out_ch, kk).tobytes()
            else:
                ch[:, 1] = 128 * sum_w                                          # 128 sum(w') + 16384 K, with sum(w') = sum(w) - 128 K
                cp = (c.in_ch + 15) // 16 * 16
                nq = kk * cp // 16
                kw = (nq + 3) // 4 * 64
                ocp = (c.out_ch + 31) // 32 * 32
                wp = np.zeros((ocp, kw), np.int8)
                t = np.zeros((c.out_ch, kk, cp), np.int16)
                t[:, :, :c.in_ch] = w64.transpose(0, 2, 1) - 128                 # [oc][tap][c] of w' = w - 128
                wp[:c.out_ch, :kk * cp] = t.reshape(c.out_ch, kk * cp).astype(np.int8)
                wb = wp.tobytes()
            ch[:, 2], ch[:, 3], ch[:, 4] = c.bn_mul, c.bn_add, c.bn_shift
            seg = np.stack([np.asarray(c.act_start, np.int64), np.asarray(c.act_mul, np.int64), np.asarray(c.act_shift, np.int64),
                            np.asarray(c.act_bias, np.int64)], 1)
            w_off = put(wb)
            ch_off = put(ch.tobytes())
            seg_off = put(np.ascontiguousarray(seg).tobytes())
            dst = new_value(c.out_ch, c.out_h, c.out_w, KPU_U8)
            row(op=KPU_OP_DWCONV if c.depthwise else KPU_OP_CONV, **{'in': src}, out=dst, k=c.ksize, pool=c.pool_type, pad=c.pad_value,
                shr_x=c.shr_x, arg_x=c.arg_x, w_off=w_off, w_bytes=len(wb), ch_off=ch_off, seg_off=seg_off, layer=c.index,
                in_c=c.in_ch, in_h=c.in_h, in_w=c.in_w)
            conv_values[c.index] = dst
            kpu[c.dst_addr] = dst
            if c.flags & KLF_MAIN_MEM_OUT:
                mem[c.main_mem_out] = dst
            continue
        f = l.fields

        def src_of(addr, what):
            if addr not in mem:
                raise KmodelError(f'kmodel: layer {l.index} ({what}) reads main-memory address {addr}, which no earlier layer wrote')
            v = mem[addr]
            if values[v][3] != KPU_U8:
                raise KmodelError(f'kmodel: layer {l.index} ({what}) reads a dequantised (fp32) tensor; only uint8 inputs are implemented')
            return v

        def size(v):
            C_, H_, W_ = shape(v)
            return C_ * H_ * W_

        if l.type == KL_DEQUANTIZE:
            s = src_of(f['src'], 'DEQUANTIZE')
            if size(s) != f['count']:
                raise KmodelError(f'kmodel: layer {l.index}: DEQUANTIZE of {f["count"]} elements, the source has {size(s)}')
            d = new_value(*shape(s), KPU_F32)
            row(op=KPU_OP_DEQUANT, **{'in': s}, out=d, scale_bits=int(np.float32(f['scale']).view(np.uint32)),
                bias_bits=int(np.float32(f['bias']).view(np.uint32)))
            mem[f['dst']] = d
        elif l.type == KL_REQUANTIZE:
            s = src_of(f['src'], 'REQUANTIZE')
            tab = np.asarray(f['table'])
            if size(s) != f['count'] or tab.dtype != np.uint8 or tab.shape != (256,):
                raise KmodelError(f'kmodel: layer {l.index}: REQUANTIZE of {f["count"]} elements through a {tab.dtype} {tab.shape} table')
            d = new_value(*shape(s), KPU_U8)
            row(op=KPU_OP_GATHER, **{'in': s}, out=d, c_off=0, table_off=put(tab.tobytes()))
            mem[f['dst']] = d
        elif l.type == KL_QUANTIZED_RESIZE_NN:
            s = src_of(f['src'], 'RESIZE_NEAREST')
            if shape(s) != (f['channels'], f['in_h'], f['in_w']) or f['out_h'] <= 0 or f['out_w'] <= 0:
                raise KmodelError(f'kmodel: layer {l.index}: RESIZE_NEAREST of {shape(s)} as ({f["channels"]}, {f["in_h"]}, {f["in_w"]})')
            d = new_value(f['channels'], f['out_h'], f['out_w'], KPU_U8)
            row(op=KPU_OP_GATHER, **{'in': s}, out=d, c_off=0)
            mem[f['dst']] = d
        elif l.type == KL_QUANTIZED_CONCAT:
            parts = [src_of(a, 'CONCAT') for a, _ in f['inputs']]
            if not parts:
                raise KmodelError(f'kmodel: layer {l.index}: CONCAT of nothing')
            for p_, (_, sz) in zip(parts, f['inputs']):
                if size(p_) != sz or shape(p_)[1:] != shape(parts[0])[1:]:
                    raise KmodelError(f'kmodel: layer {l.index}: CONCAT parts {[shape(p) for p in parts]} (sizes {[s for _, s in f["inputs"]]})')
            d = new_value(sum(shape(p_)[0] for p_ in parts), *shape(parts[0])[1:], KPU_U8)
            off = 0
            for p_ in parts:
                row(op=KPU_OP_GATHER, **{'in': p_}, out=d, c_off=off)
                off += shape(p_)[0]
            mem[f['dst']] = d
        elif l.type == KL_K210_UPLOAD:
            s = src_of(f['src'], 'K210_UPLOAD')
            if shape(s) != (f['channels'], f['height'], f['width']):
                raise KmodelError(f'kmodel: layer {l.index}: K210_UPLOAD of {shape(s)} as ({f["channels"]}, {f["height"]}, {f["width"]})')
            kpu[f['kpu_addr']] = s
        else:
            raise KmodelError(f'kmodel: layer {l.index} has type {l.type}, which the KPU-exact mode does not implement')
    if input_chw is None:
        raise KmodelError('kmodel: no KPU conv layer reads the frame')
    outs = []
    for a, _ in km.outputs:
        if a not in mem:
            raise KmodelError(f'kmodel: output at main-memory address {a} is written by no layer')
        if values[mem[a]][3] != KPU_F32:
            raise KmodelError(f'kmodel: output at main-memory address {a} is not dequantised (uint8 outputs are not implemented)')
        outs.append(mem[a])
    if not outs:
        raise KmodelError('kmodel: no outputs')
    return KpuProgram(np.stack(rows), np.asarray(values, np.int32).reshape(-1, 4), np.asarray(outs, np.int32),
                      np.frombuffer(bytes(blob), np.uint8).copy(), input_chw, conv_values)


# ---- dequantisation into Keras-named float weights ---------------------------------------------------------------------------------
def _act_fit(c: ConvLayer) -> Tuple[float, float, float, float]:
    """The activation table as  y = y0 + s_pos * (z - z0)  for z >= z0,  y0 + s_neg * (z - z0)  below: returns (z0, y0, s_pos, s_neg).
    The table has 16 segments; nncase emits at most one kink inside the un-clamped range (ReLU / LeakyReLU / linear) plus the two
    clamping ends, which the float network does not need."""
    segs = []
    for k in range(16):
        lo = float(c.act_start[k])
        hi = float(c.act_start[k + 1]) if k + 1 < 16 else np.inf
        if hi <= lo:
            continue
        slope = float(c.act_mul[k]) / float(1 << int(c.act_shift[k]))
        segs.append((lo, hi, slope, float(c.act_bias[k])))
    # value of the table at a point
    def f(z):
        for lo, hi, s, b in reversed(segs):
            if z > lo:
                return (z - lo) * s + b
        lo, hi, s, b = segs[0]
        return (z - lo) * s + b
    live = [sg for sg in segs if sg[2] != 0.0]
    if not live:
        raise KmodelError(f'kmodel: conv layer {c.index}: activation table has no live segment')
    slopes = sorted({round(sg[2], 12) for sg in live})
    s_pos = max(slopes)
    s_neg = min(slopes) if len(slopes) > 1 else s_pos
    # the kink: where the steepest segment family starts
    pos = [sg for sg in live if abs(sg[2] - s_pos) < 1e-12]
    z0 = min(sg[0] for sg in pos)
    if s_neg == s_pos:                                         # linear, or ReLU whose flat part is the zero-slope (clamped) segment
        flat = [sg for sg in segs if sg[2] == 0.0 and sg[1] <= z0 + 1e-9]
        if flat:
            s_neg = 0.0
    return z0, f(z0 + 1e-9), s_pos, s_neg


def _requant_factor(table: np.ndarray) -> Tuple[float, float]:
    """A REQUANTIZE table is round(a * q + b) clipped to 0..255: least-squares (a, b) over its un-clipped part."""
    q = np.arange(256, dtype=np.float64)
    t = table.astype(np.float64)
    ok = (t > 0) & (t < 255)
    if ok.sum() < 8:
        ok = np.ones(256, bool)
    a, b = np.polyfit(q[ok], t[ok], 1)
    return float(a), float(b)


YOLO_MOBILEV1_ORDER = (['conv1'] + [n for i in range(1, 14) for n in (f'conv_dw_{i}', f'conv_pw_{i}')] +
                       ['head_conv_1', 'head_conv_2', 'head_conv_3', 'head_conv_4', 'head_conv_5'])


def to_float_weights(km: Kmodel, spec=None) -> Tuple[Dict[str, np.ndarray], dict]:
    """Float parameters of `yolonet.yolo_mobilev1` - `spec`, a netspec.yolo_mobilev1 of any depth multiplier and class count; by default the
    demo's (alpha=0.75, 20 classes) - under this framework's (Keras layer) names + a report (activation slopes found, zero points, the
    requantisation factors).  Conv kernels HWIO, depthwise [3,3,C,1], BatchNorm as gamma / beta / moving_mean 0 / moving_variance 1-eps
    so that Keras' inference formula reproduces (scale, bias) exactly; the two output convs carry a bias."""
    convs = km.convs
    if len(convs) != len(YOLO_MOBILEV1_ORDER):
        raise KmodelError(f'kmodel: {len(convs)} KPU conv layers; the yolo_mobilev1 graph has {len(YOLO_MOBILEV1_ORDER)}')
    # every conv against the layer of yolo_mobilev1-0.75 it is mapped onto (kernel size, depthwise, channels, no KPU pooling): a kmodel
    # of another network with the same NUMBER of convs must not be dequantised into this one's names
    from . import netspec as ns
    if spec is None:
        spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    want = {l.name: l for l in spec.layers}
    if sorted(want) != sorted(YOLO_MOBILEV1_ORDER):
        raise KmodelError(f'kmodel: dequantisation maps onto the yolo_mobilev1 graph; {spec.name} has other layers')
    for name, c in zip(YOLO_MOBILEV1_ORDER, convs):
        kh, _, ci, co = want[name].kernel_shape
        dw = want[name].kind == 'dwconv'
        exp = (kh, dw, ci, ci if dw else co)
        got = (c.ksize, bool(c.depthwise), c.in_ch, c.out_ch)
        if got != exp:
            raise KmodelError(f'kmodel: conv {c.index} is (k, depthwise, in, out) = {got}; layer {name} of the yolo_mobilev1 it is loaded into is {exp}')
        if c.pool_type not in (0, 5):          # 5 = keep the top-left sample of every 2x2 window: how the KPU runs a stride-2 conv
            raise KmodelError(f'kmodel: conv {c.index} ({name}) uses KPU pooling type {c.pool_type}; the graph has no pooling layers')
    mem = [l for l in km.layers if isinstance(l, MemLayer)]
    deq = {l.fields['src']: l.fields for l in mem if l.type == KL_DEQUANTIZE}
    req = [l.fields for l in mem if l.type == KL_REQUANTIZE]
    cat = [l.fields for l in mem if l.type == KL_QUANTIZED_CONCAT]
    if len(req) != 2 or len(cat) != 1 or len(deq) != 2:
        raise KmodelError('kmodel: expected the yolo head (two dequantised outputs, one requantised concat)')
    # which requantise feeds which half of the concat (inputs are listed in concat order: [upsampled head branch, backbone])
    (c0_addr, c0_size), (c1_addr, c1_size) = cat[0]['inputs']
    r_first = next(r for r in req if r['dst'] == c0_addr)
    r_second = next(r for r in req if r['dst'] == c1_addr)
    a_first, _ = _requant_factor(r_first['table'])
    a_second, _ = _requant_factor(r_second['table'])
    by_name = dict(zip(YOLO_MOBILEV1_ORDER, convs))
    out: Dict[str, np.ndarray] = {}
    report = {'layers': {}, 'requant': {'upsampled_branch': a_first, 'backbone_branch': a_second}}
    eps = 1e-3
    for name, c in by_name.items():
        z0, y0, s_pos, s_neg = _act_fit(c)
        alpha = s_neg / s_pos
        wq = c.weights.astype(np.float64) - c.zp_w                                   # centred weights [oc][ic][kk]
        mul = c.bn_mul.astype(np.float64) / np.exp2(c.bn_shift.astype(np.float64))
        add = c.bn_add.astype(np.float64)
        scale = s_pos * mul
        bias = s_pos * (add - z0)
        in_gain = np.ones(wq.shape[1])
        if name == 'conv1':
            if abs(c.zp_x) > 0.5:
                raise KmodelError(f'kmodel: the input zero point is {c.zp_x}, expected 0 (raw u8 pixels)')
            in_gain[:] = 255.0                                                       # the engine feeds img / max(img) in [0, 1]
        if name == 'head_conv_4':                                                    # concat input: [requantised up(head_conv_3) | requantised conv_pw_11]
            n_first = by_name['head_conv_3'].out_ch
            in_gain[n_first:] = a_second                                             # conv_pw_11 keeps its own domain (conv_dw_12 reads it too)
        if name == 'head_conv_3':
            scale, bias = scale * a_first, bias * a_first                           # LeakyReLU is positively homogeneous
        if name in ('head_conv_2', 'head_conv_5'):                                   # network outputs: dequantised to real logits
            dq = deq.get(c.main_mem_out)
            if dq is None:
                raise KmodelError(f'kmodel: output conv {name} is not followed by a DEQUANTIZE')
            # the output convs are linear in Keras; their table is the identity above z0 and flat below it, which is only the lower end
            # of the 8-bit range (real = q * scale + bias, q = 0 is the calibrated minimum): not an activation
            if abs(alpha) > 1e-6 and abs(alpha - 1.0) > 1e-6:
                raise KmodelError(f'kmodel: output conv {name} has a non-linear activation table')
            alpha = 1.0
            scale = dq['scale'] * s_pos * mul
            bias = dq['scale'] * (y0 + s_pos * (add - z0)) + dq['bias']
        wf = wq * in_gain[None, :, None]
        k = c.ksize
        if c.depthwise:
            out[f'{name}/kernel'] = wf.reshape(c.out_ch, k, k).transpose(1, 2, 0)[..., None].astype(np.float32)
        else:
            out[f'{name}/kernel'] = wf.reshape(c.out_ch, c.in_ch, k, k).transpose(2, 3, 1, 0).astype(np.float32)
        if name in ('head_conv_2', 'head_conv_5'):
            # Conv2D(use_bias=True) without BN: fold the per-channel scale into the kernel
            out[f'{name}/kernel'] = (out[f'{name}/kernel'].astype(np.float64) * scale[None, None, None, :]).astype(np.float32)
            out[f'{name}/bias'] = bias.astype(np.float32)
        else:
            bn = f'{name}_bn'
            out[f'{bn}/gamma'] = (scale * np.sqrt(1.0)).astype(np.float32)
            out[f'{bn}/beta'] = bias.astype(np.float32)
            out[f'{bn}/moving_mean'] = np.zeros(c.out_ch, np.float32)
            out[f'{bn}/moving_variance'] = np.full(c.out_ch, 1.0 - eps, np.float32)   # gamma / sqrt(var + eps) = gamma
        report['layers'][name] = dict(alpha=alpha, zp_x=c.zp_x, zp_w=c.zp_w, z0=z0, y0=y0, slope=s_pos, pool=c.pool_type, pad_value=c.pad_value)
    return out, report


# ---- writer: the inverse of parse -----------------------------------------------------------------------------------------------------
# Everything below restates the published Kendryte standalone SDK (`kpu.h`: kpu_layer_argument_t, kpu_model_header_t and the kpu_model_*
# layer bodies of `kpu.c`) and the rules nncase v0.1 applies when it emits a K210 conv; the demo file is the same network, so every rule
# is held against its 32 convs bit for bit (tests/test_kmodel_write.py).
KPU_RAM_BYTES = 2 * 1024 * 1024
KPU_RAM_UNITS = KPU_RAM_BYTES // 64                   # image_src_addr / image_dst_addr count 64-byte lines
KPU_PARAM_LOAD_BYTES = 30 * 1024                      # one weight load: nncase fills at most 30 KB of the parameter RAM at a time
KFPKG_MODEL_ADDRESS = 0x00A00000                      # where the demo flashes yolo.kmodel (flash-list.json; main.c reads it from there)
HEADER_FLAGS_8BIT = 1                                 # kpu_model_header_t.flags bit 0: eight-bit weights (the only kind read or written here)

# Register fields that could NOT be derived from the public definitions and are therefore excluded from the register check, as
# {name: (register, low bit, bits, reason)}.  Empty: every field of the demo's 32 x 12 registers is regenerated.
UNDERIVED_REGISTER_FIELDS: Dict[str, Tuple[int, int, int, str]] = {}
# The KPU-RAM addresses: allocator output, not a function of the layer (an own allocator need not place tensors where nncase did).
KPU_ADDRESS_FIELDS = {'image_src_addr': (1, 0, 15), 'image_dst_addr': (1, 32, 15)}


def kpu_row_layout(width: int) -> Tuple[int, int]:
    """How the KPU lays one image row into its 64-byte RAM lines: (channels sharing a line, lines per row).  Rows up to 16 pixels pack
    four channels into a line, up to 32 two; wider rows take ceil(width / 64) lines of their own."""
    if width <= 16:
        return 4, 1
    if width <= 32:
        return 2, 1
    return 1, (width + 63) // 64


def kpu_tensor_units(channels: int, height: int, width: int) -> int:
    """64-byte lines a [C][H][W] uint8 tensor occupies in KPU RAM."""
    groups, row_len = kpu_row_layout(width)
    return row_len * height * ((channels + groups - 1) // groups)


def _field(c: ConvLayer, regs: List[int], reg: int, lo: int, bits: int, name: str, v, signed: bool = False) -> None:
    _check_width(c, name, [v], bits, signed)
    regs[reg] |= (int(v) & ((1 << bits) - 1)) << lo


def conv_registers(c: ConvLayer) -> List[int]:
    """The twelve 64-bit registers (kpu_layer_argument_t) of a KPU conv, regenerated from its geometry and quantisation parameters.
    Pointer fields the loader fills at run time (bwsx_base_addr, para_start_addr, active_addr) and send_data_out / int_en / full_add,
    which kpu_run_kmodel sets per run, are zero in the file, as the demo has them.  KmodelError when a value does not fit its field."""
    if c.ksize not in (1, 3):
        raise KmodelError(f'kmodel: conv layer {c.index}: kernel size {c.ksize} (the KPU has 1x1 and 3x3)')
    r = [0] * 12
    f = lambda *a, **k: _field(c, r, *a, **k)                                                  # noqa: E731
    in_groups, in_row_len = kpu_row_layout(c.in_w)
    out_groups, out_row_len = kpu_row_layout(c.out_w)
    one_channel = c.ksize * c.ksize * (1 if c.depthwise else c.in_ch)                          # weight bytes of one output channel
    per_load = min(c.out_ch, KPU_PARAM_LOAD_BYTES // one_channel)
    if per_load < 1:
        raise KmodelError(f'kmodel: conv layer {c.index}: one output channel has {one_channel} weight bytes, more than one parameter load '
                          f'({KPU_PARAM_LOAD_BYTES})')
    # 0 interrupt_enabe
    f(0, 0, 1, 'int_en', 0); f(0, 1, 1, 'ram_flag', 0); f(0, 2, 1, 'full_add', 0); f(0, 3, 1, 'depth_wise_layer', int(bool(c.depthwise)))
    # 1 image_addr
    f(1, 0, 15, 'image_src_addr', c.src_addr); f(1, 32, 15, 'image_dst_addr', c.dst_addr)
    # 2 image_channel_num
    f(2, 0, 10, 'i_ch_num', c.in_ch - 1); f(2, 32, 10, 'o_ch_num', c.out_ch - 1); f(2, 48, 10, 'o_ch_num_coef', per_load - 1)
    # 3 image_size
    f(3, 0, 10, 'i_row_wid', c.in_w - 1); f(3, 10, 9, 'i_col_high', c.in_h - 1)
    f(3, 32, 10, 'o_row_wid', c.out_w - 1); f(3, 42, 9, 'o_col_high', c.out_h - 1)
    # 4 kernel_pool_type_cfg
    f(4, 0, 3, 'kernel_type', 1 if c.ksize == 3 else 0); f(4, 3, 1, 'pad_type', 0); f(4, 4, 4, 'pool_type', c.pool_type)
    f(4, 8, 1, 'first_stride', 0 if c.in_h < 256 else 1); f(4, 9, 1, 'bypass_conv', 0); f(4, 10, 1, 'load_para', 1)
    f(4, 16, 8, 'dma_burst_size', 15); f(4, 24, 8, 'pad_value', c.pad_value); f(4, 32, 32, 'bwsx_base_addr', 0)
    # 5 kernel_load_cfg
    f(5, 0, 1, 'load_coor', 1); f(5, 1, 6, 'load_time', (c.out_ch + per_load - 1) // per_load - 1)
    f(5, 15, 17, 'para_size', per_load * one_channel); f(5, 32, 32, 'para_start_addr', 0)
    # 6 kernel_offset
    f(6, 0, 4, 'coef_column_offset', 0); f(6, 4, 12, 'coef_row_offset', 0)
    # 7 kernel_calc_type_cfg
    f(7, 0, 15, 'channel_switch_addr', in_row_len * c.in_h); f(7, 16, 4, 'row_switch_addr', in_row_len); f(7, 20, 8, 'coef_size', 0)
    f(7, 28, 3, 'coef_group', in_groups); f(7, 31, 1, 'load_act', 1); f(7, 32, 32, 'active_addr', 0)
    # 8 write_back_cfg
    f(8, 0, 15, 'wb_channel_switch_addr', out_row_len * c.out_h); f(8, 16, 4, 'wb_row_switch_addr', out_row_len); f(8, 20, 3, 'wb_group', out_groups)
    # 9 conv_value, 10 conv_value2
    f(9, 0, 4, 'shr_w', c.shr_w); f(9, 4, 4, 'shr_x', c.shr_x); f(9, 8, 24, 'arg_w', c.arg_w, signed=True); f(9, 32, 24, 'arg_x', c.arg_x, signed=True)
    f(10, 0, 40, 'arg_add', c.arg_add, signed=True)
    # 11 dma_parameter
    f(11, 0, 1, 'send_data_out', 0); f(11, 16, 16, 'channel_byte_num', c.out_w * c.out_h - 1)
    f(11, 32, 32, 'dma_total_byte', c.out_w * c.out_h * c.out_ch - 1)
    return r


def register_field_mask(fields) -> List[int]:
    """Twelve masks with the bits of the given {name: (register, low bit, bits, ...)} fields set."""
    m = [0] * 12
    for reg, lo, bits, *_ in fields.values():
        m[reg] |= ((1 << bits) - 1) << lo
    return m


def main_mem_usage(km: Kmodel) -> int:
    """Bytes of main memory the layers touch: the end of the highest tensor any layer writes (kpu_model_header_t.main_mem_usage)."""
    end = 0
    for l in km.layers:
        if isinstance(l, ConvLayer):
            if l.flags & KLF_MAIN_MEM_OUT:
                end = max(end, l.main_mem_out + l.out_ch * l.out_h * l.out_w)
            continue
        f = l.fields
        if l.type == KL_DEQUANTIZE:
            end = max(end, f['dst'] + 4 * f['count'])
        elif l.type == KL_REQUANTIZE:
            end = max(end, f['dst'] + f['count'])
        elif l.type == KL_QUANTIZED_RESIZE_NN:
            end = max(end, f['dst'] + f['channels'] * f['out_h'] * f['out_w'])
        elif l.type == KL_QUANTIZED_CONCAT:
            end = max(end, f['dst'] + sum(s for _, s in f['inputs']))
    return end


def _pad_to(buf: bytearray, align: int) -> None:
    while len(buf) % align:
        buf.append(0)


def serialise(km: Kmodel) -> bytes:
    """The inverse of `parse`: a kmodel v3 file from the parsed model.  The header is rebuilt from the layers (eight-bit flag, layer count,
    main_mem_usage = `main_mem_usage(km)`, the output table; max_start_address is 0 as nncase v0.1 leaves it), every conv's registers
    by `conv_registers`, and the bodies are laid out as nncase does: registers 8-byte aligned, weights and BatchNorm table 128-byte
    aligned, activation table 256-byte aligned (file offsets, which is what the body stores), main-memory bodies padded to 8 bytes.
    For a parsed file whose addresses are kept this reproduces the demo byte for byte."""
    if km.version != 3:
        raise KmodelError(f'kmodel: version {km.version} (only v3 is written)')
    n_out, n_l = len(km.outputs), len(km.layers)
    buf = bytearray(struct.pack('<7I', 3, HEADER_FLAGS_8BIT, 0, n_l, 0, main_mem_usage(km), n_out))
    for a, s in km.outputs:
        buf += struct.pack('<2I', a, s)
    table_at = len(buf)
    buf += bytes(8 * n_l)
    for i, l in enumerate(km.layers):
        start = len(buf)
        if isinstance(l, ConvLayer):
            c = l
            regs = conv_registers(c)
            for name, v, bits, signed in (('bn_mul', c.bn_mul, 24, True), ('bn_add', c.bn_add, 32, True), ('bn_shift', c.bn_shift, 4, False),
                                          ('act_shift', c.act_shift, 8, False), ('act_mul', c.act_mul, 16, True),
                                          ('act_start', c.act_start, 36, True), ('act_bias', c.act_bias, 8, True)):
                _check_width(c, name, v, bits, signed)
            w = np.asarray(c.weights)
            if w.dtype != np.uint8 or w.shape != (c.out_ch, 1 if c.depthwise else c.in_ch, c.ksize * c.ksize):
                raise KmodelError(f'kmodel: conv layer {c.index}: weights {w.dtype} {w.shape}')
            if len(c.bn_mul) != c.out_ch or len(c.bn_add) != c.out_ch or len(c.bn_shift) != c.out_ch or any(
                    len(t) != 16 for t in (c.act_start, c.act_mul, c.act_shift, c.act_bias)):
                raise KmodelError(f'kmodel: conv layer {c.index}: BatchNorm / activation tables of the wrong length')
            buf += bytes(24)
            _pad_to(buf, 8)
            lo = len(buf)
            buf += struct.pack('<12Q', *regs)
            _pad_to(buf, 128)
            wo = len(buf)
            buf += w.tobytes()
            _pad_to(buf, 128)
            bo = len(buf)
            for m, a, s in zip(c.bn_mul, c.bn_add, c.bn_shift):
                buf += struct.pack('<Q', (int(m) & 0xFFFFFF) | ((int(a) & 0xFFFFFFFF) << 24) | ((int(s) & 0xF) << 56))
            _pad_to(buf, 256)
            ao = len(buf)
            for st, m, s in zip(c.act_start, c.act_mul, c.act_shift):
                buf += struct.pack('<Q', (int(s) & 0xFF) | ((int(m) & 0xFFFF) << 8) | ((int(st) & 0xFFFFFFFFF) << 24))
            buf += np.asarray(c.act_bias, np.int64).astype(np.int8).tobytes()
            struct.pack_into('<6I', buf, start, c.flags, c.main_mem_out, lo, wo, bo, ao)
            ty = KL_K210_CONV
        else:
            f, ty = l.fields, l.type
            if ty == KL_DEQUANTIZE:
                buf += struct.pack('<4I2f', f['flags'], f['src'], f['dst'], f['count'], f['scale'], f['bias'])
            elif ty == KL_REQUANTIZE:
                tab = np.asarray(f['table'])
                if tab.dtype != np.uint8 or tab.shape != (256,):
                    raise KmodelError(f'kmodel: layer {l.index}: REQUANTIZE table {tab.dtype} {tab.shape}')
                buf += struct.pack('<4I', f['flags'], f['src'], f['dst'], f['count']) + tab.tobytes()
            elif ty == KL_QUANTIZED_CONCAT:
                buf += struct.pack('<3I', f['flags'], f['dst'], len(f['inputs']))
                for a, s in f['inputs']:
                    buf += struct.pack('<2I', a, s)
            elif ty == KL_QUANTIZED_RESIZE_NN:
                buf += struct.pack('<9I', f['flags'], f['src'], f['dst'], f['in_w'], f['in_h'], f['channels'], f['out_w'], f['out_h'],
                                   f['align'])
            elif ty == KL_K210_UPLOAD:
                buf += struct.pack('<6I', f['flags'], f['src'], f['kpu_addr'], f['width'], f['height'], f['channels'])
            else:
                raise KmodelError(f'kmodel: layer {l.index} has type {ty}, which this writer does not know')
            buf += bytes(-(len(buf) - start) % 8)                      # every body is a multiple of 8 bytes long
        struct.pack_into('<2I', buf, table_at + 8 * i, ty, len(buf) - start)
    return bytes(buf)


def write(path, km: Kmodel) -> int:
    """Write `km` as a `.kmodel`, or - when the suffix is `.kfpkg` - as the flash package kflash takes: a zip of `yolo.kmodel` and a
    `flash-list.json` with the model at the demo's address 0x00A00000.  The package carries NO firmware binary (the demo's has one beside
    the model): flash the firmware separately.  Returns the kmodel's size in bytes."""
    import json
    data = serialise(km)
    path = str(path)
    if path.endswith('.kfpkg'):
        manifest = {'version': '0.1.0', 'files': [{'address': KFPKG_MODEL_ADDRESS, 'bin': 'yolo.kmodel', 'sha256Prefix': False}]}
        with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
            z.writestr('flash-list.json', json.dumps(manifest, indent=2))
            z.writestr('yolo.kmodel', data)
    else:
        with open(path, 'wb') as fh:
            fh.write(data)
    return len(data)


def allocate_kpu_ram(sizes: List[int], births: List[int], deaths: List[int]) -> List[int]:
    """KPU-RAM addresses (64-byte units) for tensors of `sizes` units, each alive from step births[i] to step deaths[i] inclusive (the
    step that writes it .. the last step that reads it; a conv's input and output are both alive at the conv's step, so they never
    overlap, and nothing still to be read is overwritten).  In order of birth, each tensor takes address 0 if it is free for its lifetime and
    otherwise the highest free place; not nncase's allocator, and the addresses need not equal its.  KmodelError when a tensor does not fit below 2 MB."""
    addr = [-1] * len(sizes)
    for i in sorted(range(len(sizes)), key=lambda k: (births[k], k)):
        if sizes[i] > KPU_RAM_UNITS:
            raise KmodelError(f'kmodel: a tensor of {sizes[i] * 64} bytes exceeds the KPU RAM ({KPU_RAM_BYTES} bytes)')
        busy = sorted((addr[j], addr[j] + sizes[j]) for j in range(len(sizes))
                      if addr[j] >= 0 and not (deaths[j] < births[i] or births[j] > deaths[i]))
        at = 0                                                          # lowest fit
        for lo, hi in busy:
            if at + sizes[i] <= lo:
                break
            at = max(at, hi)
        if at != 0:                                                     # the bottom is taken: highest fit instead (input and output ping-pong
            top = KPU_RAM_UNITS                                         # between the two ends, so neither fragments the other's room)
            for lo, hi in reversed(busy):
                if hi + sizes[i] <= top:
                    break
                top = min(top, lo)
            if top - sizes[i] >= 0 and not any(lo < top and top - sizes[i] < hi for lo, hi in busy):
                at = top - sizes[i]
        if at + sizes[i] > KPU_RAM_UNITS:
            raise KmodelError(f'kmodel: KPU RAM exhausted: a tensor of {sizes[i] * 64} bytes does not fit beside the '
                              f'{sum(h - l for l, h in busy) * 64} bytes alive with it ({KPU_RAM_BYTES} bytes in all)')
        addr[i] = at
    return addr
