"""ctypes binding of libyolo_hip.so (include/yolo_hip.h) — the ONLY compute path of this package.

There is no CPU fallback: if the library is missing, or no HIP device is visible, every entry point
raises.  PyTorch-ROCm is used for plumbing only (device buffers, streams, torch.distributed); it is
imported before the library so that both share one HIP runtime instance (libamdhip64.so.7).

The header is the one statement of the ABI: lib() reads its prototypes (abi.signatures) and sets argtypes / restype on every declared function.
Calls go through `call(name, *args)` with plain Python ints and floats, tensors and numpy arrays (abi.DevPtr takes their address and refuses a
non-contiguous one) and byref(...) for out-parameters; a value of the wrong kind or width raises ctypes.ArgumentError before the call.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from pathlib import Path
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import abi, draw, tiles, tta
from . import netspec as ns

# YK_LIB_PATH: the developer build of the same library (`make -C csrc dev`: tuning switches compiled in), for tools/ only
LIB_PATH = Path(os.environ.get('YK_LIB_PATH') or Path(__file__).resolve().parent / 'csrc' / 'libyolo_hip.so')
HEADER_PATH = Path(__file__).resolve().parents[1] / 'include' / 'yolo_hip.h'
YK_MAX_LAYERS, YK_MAX_ANCHORS = 4, 8
PRECISIONS = {'f16': 0, 'f16x2': 1}          # YK_PRECISION_F16 / YK_PRECISION_F16X2
SCHEDULES = {'throughput': 0x000, 'latency': 0x100}      # YK_SCHEDULE_* (include/yolo_hip.h): per-layer launches | per-image cluster launches
_lib: Optional[C.CDLL] = None

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)


class YkError(RuntimeError):
    pass


class DecodeCfg(C.Structure):
    """yk_decode_cfg_t"""
    _fields_ = [('n_layers', C.c_int32), ('anchor_num', C.c_int32), ('class_num', C.c_int32),
                ('in_h', C.c_int32), ('in_w', C.c_int32),
                ('out_h', C.c_int32 * YK_MAX_LAYERS), ('out_w', C.c_int32 * YK_MAX_LAYERS),
                ('anchors', (C.c_float * 2) * YK_MAX_ANCHORS * YK_MAX_LAYERS)]


class RegionCfg(C.Structure):
    """yk_region_cfg_t"""
    _fields_ = [('layer_w', C.c_int32), ('layer_h', C.c_int32), ('anchor_num', C.c_int32), ('classes', C.c_int32),
                ('net_w', C.c_int32), ('net_h', C.c_int32), ('image_w', C.c_int32), ('image_h', C.c_int32),
                ('threshold', C.c_float), ('nms_value', C.c_float), ('anchor', C.c_float * (2 * YK_MAX_ANCHORS)),
                ('stride_b', C.c_int64), ('stride_n', C.c_int64), ('stride_e', C.c_int64),
                ('stride_y', C.c_int64), ('stride_x', C.c_int64)]


class LossCfg(C.Structure):
    """yk_loss_cfg_t"""
    _fields_ = [('out_h', C.c_int32), ('out_w', C.c_int32), ('anchor_num', C.c_int32), ('class_num', C.c_int32),
                ('anchors', (C.c_float * 2) * YK_MAX_ANCHORS), ('obj_thresh', C.c_float), ('iou_thresh', C.c_float),
                ('obj_weight', C.c_float), ('noobj_weight', C.c_float), ('wh_weight', C.c_float), ('batch_size', C.c_int32)]


class LossCfgEx(C.Structure):
    """yk_loss_cfg_ex_t"""
    _fields_ = LossCfg._fields_ + [('box_loss', C.c_int32), ('box_weight', C.c_float)]


class LossCfgOpt(C.Structure):
    """yk_loss_cfg_opt_t"""
    _fields_ = LossCfgEx._fields_ + [('focal', C.c_int32), ('focal_gamma', C.c_float), ('focal_alpha', C.c_float),
                                     ('label_smooth', C.c_float), ('obj_target', C.c_int32)]


class LabelCfg(C.Structure):
    """yk_label_cfg_t"""
    _fields_ = [('n_layers', C.c_int32), ('class_num', C.c_int32), ('assign', C.c_int32), ('reserved', C.c_int32),
                ('out_h', C.c_int32 * YK_MAX_LAYERS), ('out_w', C.c_int32 * YK_MAX_LAYERS), ('anchor_num', C.c_int32 * YK_MAX_LAYERS),
                ('anchors', (C.c_double * 2) * YK_MAX_ANCHORS * YK_MAX_LAYERS), ('assign_iou', C.c_double)]


BOX_LOSSES = {'mse': 0, 'giou': 1, 'diou': 2, 'ciou': 3}      # YK_BOX_LOSS_* (include/yolo_hip.h)
LABEL_STATUS_CLEAN = 2 ** 31 - 1                              # what yk_boxes_to_labels_f32 leaves in its status word for a clean batch


def library_path() -> Path:
    return LIB_PATH


def lib() -> C.CDLL:
    """Load libyolo_hip.so (after torch, so the HIP runtime is shared).  Raises if absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise YkError(f'{LIB_PATH} not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                          f'(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
        if not HEADER_PATH.exists():
            raise YkError(f'{HEADER_PATH} is missing: the ctypes signatures of {LIB_PATH.name} are read from it')
        import torch  # noqa: F401  (binds libamdhip64.so.7 first)
        L = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in abi.signatures(HEADER_PATH.read_text()).items():
            fn = getattr(L, name, None)        # (a function the library exports but the header does not declare keeps ctypes' defaults)
            if fn is None:
                raise YkError(f'{LIB_PATH} does not export {name}, which {HEADER_PATH.name} declares: the library is stale, build it again')
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise YkError(f'{what} failed ({rc}): {lib().yk_last_error().decode()}')


def call(name: str, *args) -> None:
    """Call the library function `name` (an int-returning one) and raise YkError if it fails.  Arguments are converted by the signature
    lib() read from the header: plain ints and floats, tensors and numpy arrays (abi.DevPtr), byref(...) for out-parameters."""
    _check(getattr(lib(), name)(*args), name)


@functools.lru_cache(maxsize=None)
def _handles_only(name: str):
    """A second binding of `name` whose pointer parameters are plain c_void_p, converted in C: for the calls of a replayed step, the
    timed path, which pass prebuilt c_void_p handles (and byref) and nothing abi.DevPtr (a from_param written in Python) would have to look at."""
    decl, fn = getattr(lib(), name), lib()[name]
    fn.restype, fn.argtypes = decl.restype, [C.c_void_p if a is abi.DevPtr else a for a in decl.argtypes]
    return fn


def require_gpu() -> None:
    import torch
    if not torch.cuda.is_available() or lib().yk_device_count() <= 0:
        raise YkError('no MI355X / HIP device visible: the HIP path is the only path (no CPU fallback)')


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _stream(stream=None) -> C.c_void_p:
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


class _DevView:
    """Zero-copy torch view of library-owned device memory via __cuda_array_interface__."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        import weakref
        self.__cuda_array_interface__ = {'shape': tuple(int(s) for s in shape), 'typestr': typestr,
                                         'data': (int(ptr), False), 'version': 2}
        # weak: torch keeps this object alive inside the tensor's storage deleter, where Python's GC cannot see it; a strong
        # reference would tie Plan -> views -> storage -> _DevView -> Plan into a cycle that never frees the device memory.
        # The views are BORROWED (kpu_get_output semantics): they are valid until the plan is closed.
        self._owner = weakref.ref(owner)


class _PlanBase:
    """What Plan and KpuPlan share: the handle's life and the borrowed views of the outputs.  A subclass names its destroy and get-output
    functions and sets _h, _n_outputs, max_batch and device."""
    _destroy = _get_output = None

    def close(self):
        self._out_views = None
        if getattr(self, '_h', None) and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def output_ptrs(self) -> List[Tuple[int, Tuple[int, int, int]]]:
        res = []
        for i in range(self._n_outputs):
            p = f32p()
            nb = C.c_size_t()
            h, w, c = C.c_int(), C.c_int(), C.c_int()
            call(self._get_output, self._h, i, C.byref(p), C.byref(nb), C.byref(h), C.byref(w), C.byref(c))
            res.append((C.cast(p, C.c_void_p).value, (h.value, w.value, c.value)))
        return res

    def outputs(self):
        """Borrowed torch views [max_batch,h,w,c] fp32 of the network outputs (kpu_get_output; Plan: c = A*(5+C))."""
        import torch
        if self._out_views is None:
            self._out_views = [torch.as_tensor(_DevView(p, (self.max_batch, *s), '<f4', self), device=f'cuda:{self.device}')
                               for p, s in self.output_ptrs()]
        return self._out_views


class Plan(_PlanBase):
    """kpu_load_kmodel analogue (main.c:274): a compiled, device-resident network."""
    _destroy, _get_output = 'yk_plan_destroy', 'yk_get_output'

    def __init__(self, spec: ns.NetSpec, weights, max_batch: int = 32, device: Optional[int] = None, precision: str = 'f16x2',
                 schedule: str = 'latency'):
        """precision: 'f16x2' (default; activations stored as fp16 pairs hi + lo, compensated fp16 MFMA operands: the mode that meets
        BASELINE.json's 1e-3 / exact-index tolerance) or 'f16' (fp16 activations, about twice as fast, 5e-3 worst case on the
        scores); see include/yolo_hip.h YK_PRECISION_*.
        schedule (f16x2): 'latency' - the late backbone and the heads as two launches of per-image workgroup clusters, the shortest time
        for ONE batch (a Plan on its own runs one batch at a time, hence the default here) - or 'throughput' - one launch per layer,
        which overlaps better when several plans run on several streams (Pipeline picks it for depth >= 2); YK_SCHEDULE_*."""
        import torch
        require_gpu()
        if precision not in PRECISIONS:
            raise YkError(f'precision {precision!r}: expected one of {sorted(PRECISIONS)}')
        if schedule not in SCHEDULES:
            raise YkError(f'schedule {schedule!r}: expected one of {sorted(SCHEDULES)}')
        self.precision = precision
        self.schedule = schedule
        self.spec = spec
        self.max_batch = int(max_batch)
        self.device = torch.cuda.current_device() if device is None else int(device)
        ops, tens, blob = spec.compile_plan(weights)
        self._ops = np.ascontiguousarray(ops, np.int32)
        self._tens = np.ascontiguousarray(tens, np.int32)
        blob = np.ascontiguousarray(blob, np.float32)
        outs = np.ascontiguousarray(spec.outputs, np.int32)
        self._h, self._n_outputs, self._out_views = C.c_void_p(), len(outs), None
        call('yk_plan_create_ex', C.byref(self._h), self._ops, len(ops), self._tens, len(tens), blob, blob.size, outs, len(outs),
             self.max_batch, self.device, PRECISIONS[precision] | SCHEDULES[schedule])

    # -- run ---------------------------------------------------------------
    def run_u8(self, frames, stream=None) -> None:
        """frames: torch.uint8 cuda tensor [B,H,W,3] (kpu_run_kmodel analogue, async)."""
        assert frames.is_cuda and frames.dtype.__str__() == 'torch.uint8' and frames.is_contiguous()
        assert tuple(frames.shape[1:]) == (*self.spec.in_hw, 3), frames.shape
        call('yk_run_u8', self._h, frames, frames.shape[0], _stream(stream))

    def run_f32(self, x, stream=None) -> None:
        assert x.is_cuda and x.dtype.__str__() == 'torch.float32' and x.is_contiguous()
        assert tuple(x.shape[1:]) == (*self.spec.in_hw, 3), x.shape
        call('yk_run_f32', self._h, x, x.shape[0], _stream(stream))

    def check(self) -> None:
        """Wait for the device; raise if an earlier asynchronous run of this plan failed on the device (yk_plan_check)."""
        call('yk_plan_check', self._h)

    def raise_if_failed(self) -> None:
        """Raise if a run of this plan that has ALREADY finished failed on the device (yk_plan_peek_error: a read of mapped host memory,
        no synchronisation - call it after waiting for the run's stream or event).  The flag is cleared by the report."""
        e = C.c_uint()
        _check(_handles_only('yk_plan_peek_error')(self._h, 1, C.byref(e)), 'yk_plan_peek_error')      # (Ticket.result: once per timed step)
        if e.value:
            raise YkError('f16x2 cluster launch: a workgroup cluster did not assemble (its workgroups were not co-resident, e.g. another '
                          'kernel held CUs for the whole launch); the results of that run are invalid.  Use schedule=\'throughput\' when the '
                          'GPU is shared.')

    def read_tensor(self, tid: int, batch: int) -> np.ndarray:
        h, w, c = self.spec.tensors[tid]
        out = np.empty((batch, h, w, c), np.float32)
        call('yk_debug_read_tensor', self._h, tid, batch, out, out.size)
        return out

    def read_exponents(self, tid: int, batch: int) -> np.ndarray:
        """int32 [batch]: the per-image storage exponents of an f16x2 plan's stored tensor `tid` (the halves hold x * 2^-e = hi + lo; fp32
        planes: 0).  Raises for an f16 plan and for a tensor that is not stored split (yk_debug_read_exponents)."""
        e = np.empty((batch,), np.int32)
        call('yk_debug_read_exponents', self._h, tid, batch, e)
        return e

    def profile(self, frames, iters: int = 10, stream=None) -> np.ndarray:
        """Average per-launch duration (ms) measured with HIP events on the launch stream."""
        n = lib().yk_plan_launch_count(self._h)
        ms = np.zeros(n, np.float32)
        call('yk_plan_profile', self._h, frames, frames.shape[0], iters, _stream(stream), ms)
        return ms

    def launches(self):
        n = lib().yk_plan_launch_count(self._h)
        res = []
        for i in range(n):
            name = C.create_string_buffer(128)
            fl, by = C.c_double(), C.c_double()
            lib().yk_plan_launch_info(self._h, i, name, 128, C.byref(fl), C.byref(by))
            res.append((name.value.decode(), fl.value, by.value))
        return res


KPU_LAYOUTS = {'nhwc': 0, 'chw': 1}          # YK_KPU_NHWC / YK_KPU_CHW


class KpuPlan(_PlanBase):
    """The K210 KPU's integer pipeline for a parsed kmodel v3 on the GPU (yk_kpu_*, include/yolo_hip.h): outputs
    bit-identical to oracle/kpu_ref.run for every image.  The KPU takes the raw 0..255 pixels (no `img / np.max(img)`).  Duck-types Plan
    where inference.detect and yolonet use it: `max_batch`, `run_u8`, `outputs`."""
    _destroy, _get_output = 'yk_kpu_plan_destroy', 'yk_kpu_get_output'

    def __init__(self, km, max_batch: int = 32, device: Optional[int] = None):
        """km: a parsed kmodel.Kmodel (packed here) or a kmodel.KpuProgram that kmodel.pack_kpu already made."""
        import torch
        from . import kmodel
        require_gpu()
        # CPU: pack_kpu raises KmodelError for what the kernels do not implement
        prog = km if isinstance(km, kmodel.KpuProgram) else kmodel.pack_kpu(km)
        self.program = prog
        self.max_batch = int(max_batch)
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.input_chw = prog.input_chw
        self._ops = np.ascontiguousarray(prog.ops, np.int64)
        self._vals = np.ascontiguousarray(prog.values, np.int32)
        self._outs = np.ascontiguousarray(prog.outputs, np.int32)
        self._blob = np.ascontiguousarray(prog.blob, np.uint8)
        self._h, self._n_outputs, self._out_views = C.c_void_p(), len(self._outs), None
        call('yk_kpu_plan_create', C.byref(self._h), self._ops, len(self._ops), self._vals, len(self._vals), self._outs, len(self._outs),
             self._blob, self._blob.size, self.max_batch, self.device)

    def _frame_shape(self, layout: str):
        c, h, w = self.input_chw
        return (c, h, w) if layout == 'chw' else (h, w, c)

    def run_u8(self, frames, layout: str = 'nhwc', stream=None) -> None:
        """frames: torch.uint8 cuda tensor [B,H,W,C] ('nhwc', what letterbox_u8 / Plan.run_u8 use) or [B,C,H,W] ('chw', what main.c
        feeds kpu_run_kmodel), raw 0..255 pixels.  Asynchronous (kpu_run_kmodel analogue)."""
        import torch
        if layout not in KPU_LAYOUTS:
            raise YkError(f'layout {layout!r}: expected one of {sorted(KPU_LAYOUTS)}')
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()):
            raise YkError('KpuPlan.run_u8: frames must be a contiguous cuda uint8 tensor')
        if tuple(frames.shape[1:]) != self._frame_shape(layout) or not 0 < frames.shape[0] <= self.max_batch:
            raise YkError(f'KpuPlan.run_u8: frames {tuple(frames.shape)}, expected [<= {self.max_batch}, {", ".join(map(str, self._frame_shape(layout)))}]')
        call('yk_kpu_run_u8', self._h, frames, frames.shape[0], KPU_LAYOUTS[layout], _stream(stream))

    # -- statistics run (biascorrect.py): per-channel integer sums of z ------
    def _stat_layout(self):
        """[(kmodel layer index, first slot, OC)] of the conv ops in issue order, and the slot count (yk_kpu_run_stats_u8's layout)."""
        from . import kmodel as km_
        rows, at = [], 0
        for r in self.program.ops:
            if int(r[km_.KF_OP]) in (km_.KPU_OP_CONV, km_.KPU_OP_DWCONV):
                oc = int(self.program.values[int(r[km_.KF_OUT]), 0])
                rows.append((int(r[km_.KF_LAYER]), at, oc))
                at += oc
        return rows, at

    def _zsums(self):
        import torch
        if getattr(self, '_d_zsum', None) is None:
            n = self._stat_layout()[1]
            if n != lib().yk_kpu_stat_slots(self._h):
                raise YkError('KpuPlan: the library counts other statistics slots than the program has conv channels')
            self._d_zsum = torch.zeros(n, dtype=torch.int64, device=f'cuda:{self.device}')
        return self._d_zsum

    def run_stats_u8(self, frames, steps, layout: str = 'nhwc', stream=None) -> None:
        """run_u8 with the statistics kernels: the same tensors and outputs, bit for bit, and z of every counted output element added to the
        per-channel sums `read_zsums` returns.  steps: {kmodel layer index: 1 | 2} (missing: 1) or one value per conv in issue order; 2
        counts only even oy and even ox.  Sums accumulate over runs until reset_zsums."""
        import torch
        if layout not in KPU_LAYOUTS:
            raise YkError(f'layout {layout!r}: expected one of {sorted(KPU_LAYOUTS)}')
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()):
            raise YkError('KpuPlan.run_stats_u8: frames must be a contiguous cuda uint8 tensor')
        if tuple(frames.shape[1:]) != self._frame_shape(layout) or not 0 < frames.shape[0] <= self.max_batch:
            raise YkError(f'KpuPlan.run_stats_u8: frames {tuple(frames.shape)}, expected [<= {self.max_batch}, '
                          f'{", ".join(map(str, self._frame_shape(layout)))}]')
        rows = self._stat_layout()[0]
        if isinstance(steps, dict):
            unknown = sorted(set(steps) - {r[0] for r in rows})
            if unknown:
                raise YkError(f'KpuPlan.run_stats_u8: steps for layer(s) {unknown}, which are not conv layers of this kmodel')
            steps = [steps.get(r[0], 1) for r in rows]
        h_step = np.ascontiguousarray([int(s) for s in steps], np.int32)
        if len(h_step) != len(rows) or not np.isin(h_step, (1, 2)).all():
            raise YkError(f'KpuPlan.run_stats_u8: {len(rows)} steps of 1 or 2 expected, got {h_step.tolist()}')
        call('yk_kpu_run_stats_u8', self._h, frames, frames.shape[0], KPU_LAYOUTS[layout], h_step, len(h_step), self._zsums(), _stream(stream))

    def read_zsums(self):
        """{kmodel layer index: int64 [OC]}: the sums of z since the last reset_zsums (waits for the device)."""
        import torch
        torch.cuda.synchronize(self.device)
        h = self._zsums().cpu().numpy()
        return {layer: h[at:at + oc].copy() for layer, at, oc in self._stat_layout()[0]}

    def reset_zsums(self) -> None:
        self._zsums().zero_()

    def read_layer(self, index: int, image: int) -> np.ndarray:
        """uint8 [C][H][W] output of the conv at kmodel layer `index` for image `image` of the last run (waits for the device)."""
        v = self.program.conv_values.get(int(index))
        if v is None:
            raise YkError(f'layer {index} is not a KPU conv layer of this kmodel')
        c, h, w = (int(x) for x in self.program.values[v, :3])
        out = np.empty((c, h, w), np.uint8)
        call('yk_kpu_debug_read', self._h, int(index), int(image), out, out.size)
        return out

    def layer_view(self, index: int):
        """Borrowed torch view uint8 [max_batch, H, W, C] of the output of the conv at kmodel layer `index`, where the last run left it
        (yk_kpu_layer_ptr): valid until the plan is closed, rewritten by every run, and not synchronised - read it on the run's stream."""
        import torch
        p, h, w, c = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        call('yk_kpu_layer_ptr', self._h, int(index), C.byref(p), C.byref(h), C.byref(w), C.byref(c))
        return torch.as_tensor(_DevView(p.value, (self.max_batch, h.value, w.value, c.value), '|u1', self), device=f'cuda:{self.device}')

    def profile(self, frames, layout: str = 'nhwc', iters: int = 10, stream=None) -> np.ndarray:
        """Median duration (ms) of every launch of one run, HIP events around each (yk_kpu_profile)."""
        n = lib().yk_kpu_launch_count(self._h)
        ms = np.zeros(n, np.float32)
        call('yk_kpu_profile', self._h, frames, frames.shape[0], KPU_LAYOUTS[layout], iters, _stream(stream), ms)
        return ms

    def launches(self) -> List[str]:
        """Name of every launch of one run (op and kmodel layer), in issue order."""
        from . import kmodel as km_
        names = {km_.KPU_OP_CONV: 'conv', km_.KPU_OP_DWCONV: 'dwconv', km_.KPU_OP_GATHER: 'gather', km_.KPU_OP_DEQUANT: 'dequantize'}
        res = []
        for r in self.program.ops:
            n = names[int(r[km_.KF_OP])]
            res.append(f'{n}{int(r[km_.KF_K])}x{int(r[km_.KF_K])} layer {int(r[km_.KF_LAYER])}' if n.endswith('conv') else n)
        return res


def make_decode_cfg(anchors: np.ndarray, class_num: int, in_hw, out_hw) -> DecodeCfg:
    anchors = np.asarray(anchors, np.float32)
    L, A = anchors.shape[0], anchors.shape[1]
    if L > YK_MAX_LAYERS or A > YK_MAX_ANCHORS:
        raise YkError('too many layers/anchors')
    cfg = DecodeCfg()
    cfg.n_layers, cfg.anchor_num, cfg.class_num = L, A, int(class_num)
    cfg.in_h, cfg.in_w = int(in_hw[0]), int(in_hw[1])
    for l in range(L):
        cfg.out_h[l], cfg.out_w[l] = int(out_hw[l][0]), int(out_hw[l][1])
        for n in range(A):
            cfg.anchors[l][n][0] = float(anchors[l, n, 0])
            cfg.anchors[l][n][1] = float(anchors[l, n, 1])
    return cfg


def _nms_method(nms: str, sigma: float) -> int:
    """YK_NMS_* of a rule's name; an unknown name or a sigma the Gaussian cannot use is refused by name."""
    from . import softnms
    try:
        softnms.check(nms, float(sigma))
    except ValueError as e:
        raise YkError(str(e)) from None
    return softnms.method_id(nms)


def decode_py(cfg: DecodeCfg, preds: Sequence, batch: int, image_hw=None, obj_thresh: float = 0.7,
              iou_thresh: float = 0.5, max_out: int = 30, stream=None, return_index: bool = False, nms: str = 'hard', sigma: float = 0.5):
    """Batched keras_inference.py:94-135 on the GPU.  preds: cuda fp32 tensors [>=batch,h,w,A*(5+C)].
    nms: 'hard' (the reference's rule) or 'linear' / 'gaussian' / 'diou' (softnms.py: rows then carry the decayed scores); sigma: the Gaussian's.
    -> (dets [batch, C*max_out, 6] cuda fp32, counts [batch] cuda int32[, box_index [batch, C*max_out] cuda int32: each row's index
    in the reference's flattened (layer, h, w, anchor) box list])."""
    import torch
    require_gpu()
    method = _nms_method(nms, sigma)
    dev = preds[0].device
    dets = torch.empty((batch, cfg.class_num * max_out, 6), dtype=torch.float32, device=dev)
    counts = torch.empty((batch,), dtype=torch.int32, device=dev)
    arr = (C.c_void_p * len(preds))(*[p.data_ptr() for p in preds])
    ihw = None
    if image_hw is not None:
        ihw = torch.as_tensor(np.broadcast_to(np.asarray(image_hw, np.float32), (batch, 2)).copy(), device=dev)
    if method != 0:
        index = torch.full((batch, cfg.class_num * max_out), -1, dtype=torch.int32, device=dev) if return_index else None
        call('yk_decode_py_nms', C.byref(cfg), arr, batch, ihw, obj_thresh, iou_thresh, max_out, dets, counts, index, _stream(stream), method, sigma)
        return (dets, counts, index) if return_index else (dets, counts)
    if return_index:
        index = torch.full((batch, cfg.class_num * max_out), -1, dtype=torch.int32, device=dev)
        call('yk_decode_py_ex', C.byref(cfg), arr, batch, ihw, obj_thresh, iou_thresh, max_out, dets, counts, index, _stream(stream))
        return dets, counts, index
    call('yk_decode_py', C.byref(cfg), arr, batch, ihw, obj_thresh, iou_thresh, max_out, dets, counts, _stream(stream))
    return dets, counts


def region_batched(inp, W: int, H: int, A: int, Cn: int, anchor, threshold: float, nms_value: float,
                   net_wh=(320, 224), image_wh=(320, 224), layout: str = 'chw', want_output: bool = True, stream=None):
    """Batched C-mode region layer.  inp: cuda fp32 [B, A*(5+C), H, W] ('chw') or [B,H,W,A*(5+C)] ('hwc').
    -> (output|None, boxes [B,nb,4], probs [B,nb,C+1])."""
    import torch
    require_gpu()
    B = inp.shape[0]
    E, hw, nb = 5 + Cn, W * H, A * W * H
    cfg = RegionCfg()
    cfg.layer_w, cfg.layer_h, cfg.anchor_num, cfg.classes = W, H, A, Cn
    cfg.net_w, cfg.net_h, cfg.image_w, cfg.image_h = net_wh[0], net_wh[1], image_wh[0], image_wh[1]
    cfg.threshold, cfg.nms_value = threshold, nms_value
    for i, v in enumerate(np.asarray(anchor, np.float32).ravel()):
        cfg.anchor[i] = float(v)
    if layout == 'chw':
        cfg.stride_b, cfg.stride_n, cfg.stride_e, cfg.stride_y, cfg.stride_x = A * E * hw, E * hw, hw, W, 1
    else:
        cfg.stride_b, cfg.stride_n, cfg.stride_e, cfg.stride_y, cfg.stride_x = A * E * hw, E, 1, W * A * E, A * E
    out = torch.empty((B, A * E, H, W), dtype=torch.float32, device=inp.device) if want_output else None
    boxes = torch.empty((B, nb, 4), dtype=torch.float32, device=inp.device)
    probs = torch.empty((B, nb, Cn + 1), dtype=torch.float32, device=inp.device)
    call('yk_region_batched', C.byref(cfg), inp, B, out, boxes, probs, _stream(stream))
    return out, boxes, probs


def yolo_loss(y_true, y_pred, anchors_l, obj_thresh, iou_thresh, obj_weight, noobj_weight, wh_weight, batch_size=None,
              counts=None, want_grad=True, want_ignore=False, stream=None, box_loss='mse', box_weight=1.0, focal='off', focal_gamma=2.0,
              focal_alpha=0.0, label_smooth=0.0, obj_target='label'):
    """tools/utils.py:741-791 loss_fn + custom.py metrics for one layer on the GPU.
    y_true / y_pred: cuda fp32 [B,h,w,A,5+C].  -> (loss[6] = total,xy,wh,obj,noobj,cls ; grad | None ; ignore | None).
    `counts` (cuda fp32 [3], running tp/fp/fn) is updated in place when given.
    box_loss 'giou' | 'diou' | 'ciou' (DESIGN.md 3.14): the IoU-family box term, weighted by box_weight, in place of xy and wh (both then
    0); -> loss[7] = total,xy,wh,obj,noobj,cls,box (yk_yolo_loss_ex).
    focal 'obj' | 'cls' | 'all' with focal_gamma, focal_alpha; label_smooth; obj_target 'iou' (the rule is in lossopt.py):
    options on the objectness and class terms; with one of them on the call is yk_yolo_loss_opt and -> loss[7] whatever the box loss; with
    all of them off it is the call above."""
    import torch
    from . import lossopt
    if box_loss not in BOX_LOSSES:
        raise ValueError(f'box_loss {box_loss!r}: choose one of ' + ', '.join(repr(k) for k in BOX_LOSSES))
    o = lossopt.validate(focal, focal_gamma, focal_alpha, label_smooth, obj_target)
    require_gpu()
    assert y_true.is_cuda and y_pred.is_cuda and y_true.shape == y_pred.shape and y_pred.dtype == torch.float32
    y_true, y_pred = y_true.contiguous(), y_pred.contiguous()
    B, h, w, A, E = y_pred.shape
    opt = not lossopt.is_off(**o)
    ex = opt or box_loss != 'mse'
    cfg = LossCfgOpt() if opt else LossCfgEx() if ex else LossCfg()
    if ex:
        cfg.box_loss, cfg.box_weight = BOX_LOSSES[box_loss], box_weight
    if opt:
        cfg.focal, cfg.focal_gamma, cfg.focal_alpha = lossopt.FOCAL[o['focal']], o['focal_gamma'], o['focal_alpha']
        cfg.label_smooth, cfg.obj_target = o['label_smooth'], lossopt.OBJ_TARGETS[o['obj_target']]
    cfg.out_h, cfg.out_w, cfg.anchor_num, cfg.class_num = h, w, A, E - 5
    for n, (aw, ah) in enumerate(np.asarray(anchors_l, np.float32)):
        cfg.anchors[n][0], cfg.anchors[n][1] = float(aw), float(ah)
    cfg.obj_thresh, cfg.iou_thresh = obj_thresh, iou_thresh
    cfg.obj_weight, cfg.noobj_weight, cfg.wh_weight = obj_weight, noobj_weight, wh_weight
    cfg.batch_size = int(batch_size if batch_size else B)
    loss = torch.empty(7 if ex else 6, dtype=torch.float32, device=y_pred.device)
    grad = torch.empty_like(y_pred) if want_grad else None
    ign = torch.empty((B, h, w, A), dtype=torch.float32, device=y_pred.device) if want_ignore else None
    call('yk_yolo_loss_opt' if opt else 'yk_yolo_loss_ex' if ex else 'yk_yolo_loss', C.byref(cfg), y_true, y_pred, B, loss, grad, ign, counts, _stream(stream))
    return loss, grad, ign


def distill_loss(teacher, pred, weight, batch_size, grad=None, stream=None):
    """Knowledge distillation on the raw outputs of one layer (yk_distill_loss_f32; the rule is in distill.py).
    teacher / pred: cuda fp32 [B, h, w, A, 5 + C] (or [B, rows, 5 + C]), the teacher's and the student's raw outputs.  grad: dL/dpred is ADDED
    to it (same shape as pred; None to skip).  -> loss[4] = total, obj, cls, box, each weight / batch_size times its sum (cuda fp32)."""
    import torch
    require_gpu()
    for name, t in (('teacher', teacher), ('pred', pred)) + ((('grad', grad),) if grad is not None else ()):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise YkError(f'distill_loss: {name} must be a contiguous cuda float32 tensor')
        if t.shape != pred.shape or t.device != pred.device:
            raise YkError(f'distill_loss: {name} is {tuple(t.shape)} on {t.device}, pred {tuple(pred.shape)} on {pred.device}')
    if pred.dim() < 3 or pred.shape[-1] < 6 or pred.numel() == 0:
        raise YkError(f'distill_loss: pred {tuple(pred.shape)}: expected [B, ..., 5 + C] with C >= 1')
    B, E = int(pred.shape[0]), int(pred.shape[-1])
    loss = torch.empty(4, dtype=torch.float32, device=pred.device)
    call('yk_distill_loss_f32', teacher, pred, B, pred.numel() // (B * E), E - 5, float(weight), int(batch_size), loss, grad, _stream(stream))
    return loss


def letterbox_u8(frames, dst_hw, stream=None, out=None):
    """GPU Helper._process_img letterbox (tools/utils.py:378-399): cuda uint8 [B,h,w,3] -> cuda uint8 [B,H,W,3]."""
    import torch
    require_gpu()
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[-1] == 3
    B, sh, sw, _ = frames.shape
    if out is None:
        out = torch.empty((B, int(dst_hw[0]), int(dst_hw[1]), 3), dtype=torch.uint8, device=frames.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, int(dst_hw[0]), int(dst_hw[1]), 3)
    call('yk_letterbox_u8', frames, B, sh, sw, out, out.shape[1], out.shape[2], _stream(stream))
    return out


def letterbox_augment_u8(frames, dst_hw, inv, stream=None, out=None):
    """Letterbox + training augmentation in one launch (yk_letterbox_augment_u8, semantics in augment.py): cuda uint8 [B,h,w,3] and
    each image's inverse map `inv` (cuda float64 [B,2,3] or [B,6]) -> cuda uint8 [B,H,W,3]."""
    import torch
    require_gpu()
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[-1] == 3
    B, sh, sw, _ = frames.shape
    assert inv.is_cuda and inv.dtype == torch.float64 and inv.is_contiguous() and inv.numel() == 6 * B and inv.device == frames.device
    if out is None:
        out = torch.empty((B, int(dst_hw[0]), int(dst_hw[1]), 3), dtype=torch.uint8, device=frames.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, int(dst_hw[0]), int(dst_hw[1]), 3)
    call('yk_letterbox_augment_u8', frames, B, sh, sw, inv, out, out.shape[1], out.shape[2], _stream(stream))
    return out


class _RowKind(NamedTuple):
    """What tells the three per-picture tables of include/yolo_hip.h apart.  _check_rows, _table_to_device and _letterbox_rows_u8 are the one
    implementation behind the ragged, tile and view functions below."""
    label: str                      # '<label> table: ...' in every message
    dtype: np.dtype
    extra: Optional[Callable]       # t -> (the rows it refuses, i -> the rest of '<label> table: row i ...'); after the test for pixels
    end: Callable                   # (name -> that column as Python ints) -> the byte one past each row's last
    params: str                     # the C function that fills scale / tx / ty
    launch: str                     # the C function that letterboxes the rows


def _tile_stride(t):
    return (t['stride'] < 3 * t['w'].astype(np.int64),
            lambda i: f'has stride {int(t["stride"][i])}, less than the {3 * int(t["w"][i])} bytes of one of its rows')


def _view_canvas(t):
    i64 = lambda name: t[name].astype(np.int64)
    return ((t['oy'] < 0) | (t['ox'] < 0) | (i64('oy') + i64('h') > i64('ch')) | (i64('ox') + i64('w') > i64('cw')),
            lambda i: f'puts its {int(t["h"][i])} x {int(t["w"][i])} picture at ({int(t["oy"][i])}, {int(t["ox"][i])}), outside its '
                      f'canvas of {int(t["ch"][i])} x {int(t["cw"][i])}')


def _picture_end(col):
    return col('offset') + 3 * col('h') * col('w')


_RAGGED = _RowKind('ragged', draw.RAGGED_DTYPE, None, _picture_end, 'yk_letterbox_ragged_params', 'yk_letterbox_ragged_u8')
_TILE = _RowKind('tile', tiles.TILE_DTYPE, _tile_stride, lambda col: col('offset') + (col('h') - 1) * col('stride') + 3 * col('w'),
                 'yk_letterbox_tiles_params', 'yk_letterbox_tiles_u8')
_VIEW = _RowKind('view', tta.VIEW_DTYPE, _view_canvas, _picture_end, 'yk_letterbox_views_params', 'yk_letterbox_views_u8')


def _check_rows(kind: _RowKind, table, packed_bytes: int) -> np.ndarray:
    t = np.array(table, dtype=kind.dtype, copy=True).reshape(-1)
    checks = [((t['h'] <= 0) | (t['w'] <= 0), lambda i: f'is {int(t["h"][i])} x {int(t["w"][i])}')]
    if kind.extra is not None:
        checks.append(kind.extra(t))
    for bad, what in checks:
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise YkError(f'{kind.label} table: row {i} {what(i)}')
    end = kind.end(lambda name: t[name].astype(object))
    if len(t) and max(end) > int(packed_bytes):
        raise YkError(f'{kind.label} table: row {int(np.argmax(end))} ends at byte {max(end)} of a {int(packed_bytes)}-byte buffer')
    return t


def _table_to_device(kind: _RowKind, table, dst_hw, packed_bytes: int, device, stream):
    import torch
    t = _check_rows(kind, table, packed_bytes)
    if len(t) == 0:                                    # (an empty table passes _check_rows: this is the first thing said about it)
        raise YkError(f'{kind.label} table: no rows')
    if dst_hw is not None:
        call(kind.params, t, len(t), int(dst_hw[0]), int(dst_hw[1]))
    host = torch.from_numpy(t.view(np.uint8).reshape(len(t), kind.dtype.itemsize))
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        return host.to(device, non_blocking=False)


def _device_table(kind: _RowKind, packed, table, dst_hw, stream):
    """`table` as the calls on a packed buffer take it: a host table goes through _table_to_device, a device table is checked for its shape."""
    import torch
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() > 0
    if not torch.is_tensor(table):
        table = _table_to_device(kind, table, dst_hw, packed.numel(), packed.device, stream)
    assert table.is_cuda and table.dtype == torch.uint8 and table.is_contiguous() and table.dim() == 2 and table.device == packed.device
    assert table.shape[1] == kind.dtype.itemsize and table.shape[0] > 0, tuple(table.shape)
    return table


def _letterbox_rows_u8(kind: _RowKind, packed, table, dst_hw, stream, out):
    import torch
    require_gpu()
    table = _device_table(kind, packed, table, dst_hw, stream)
    n = int(table.shape[0])
    if out is None:
        out = torch.empty((n, int(dst_hw[0]), int(dst_hw[1]), 3), dtype=torch.uint8, device=packed.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, int(dst_hw[0]), int(dst_hw[1]), 3), tuple(out.shape)
    call(kind.launch, packed, packed.numel(), table, n, out, out.shape[1], out.shape[2], _stream(stream))
    return out


def ragged_table_to_device(table, dst_hw, packed_bytes: int, device, stream=None):
    """A host table of a ragged batch (draw.RAGGED_DTYPE = yk_ragged_row_t; draw.pack_ragged writes it) checked, completed and uploaded:
    every row must be a non-empty picture inside the `packed_bytes` of its buffer; scale / tx / ty are filled for the network size dst_hw
    (None: left as they are - drawing does not read them).  -> cuda uint8 [n, 40], what the ragged calls take as their table."""
    return _table_to_device(_RAGGED, table, dst_hw, packed_bytes, device, stream)


def letterbox_ragged_u8(packed, table, dst_hw, stream=None, out=None):
    """The letterbox of letterbox_u8 for pictures of DIFFERENT sizes in one launch (yk_letterbox_ragged_u8): `packed` cuda uint8 [bytes], the
    pictures of draw.pack_ragged; `table` its host table (checked here: a row without pixels, or one that leaves the buffer, is refused) or
    the device table ragged_table_to_device returned for this dst_hw.  -> cuda uint8 [n, H, W, 3]; image i is bit for bit
    letterbox_u8 of picture i alone."""
    return _letterbox_rows_u8(_RAGGED, packed, table, dst_hw, stream, out)


def check_ragged_rows(table, packed_bytes: int) -> np.ndarray:
    """The rows of a host table (draw.RAGGED_DTYPE) as one flat copy, refused with YkError unless every row is a non-empty picture inside
    the `packed_bytes` of its buffer: what the kernels would otherwise answer with zeros."""
    return _check_rows(_RAGGED, table, packed_bytes)


def check_tile_rows(table, packed_bytes: int) -> np.ndarray:
    """The rows of a host tile table (tiles.TILE_DTYPE = yk_tile_row_t) as one flat copy, refused with YkError unless every row is a non-empty
    tile whose rows do not overlap (stride >= 3 * w) and whose last byte lies inside the `packed_bytes` of its buffer: what
    yk_letterbox_tiles_u8 would otherwise answer with a zero frame."""
    return _check_rows(_TILE, table, packed_bytes)


def tile_table_to_device(table, dst_hw, packed_bytes: int, device, stream=None):
    """A host tile table (tiles.table_rows) checked (check_tile_rows), its scale / tx / ty filled for the network size dst_hw and uploaded
    -> cuda uint8 [n, 40], what letterbox_tiles_u8 takes as its table."""
    return _table_to_device(_TILE, table, dst_hw, packed_bytes, device, stream)


def letterbox_tiles_u8(packed, table, dst_hw, stream=None, out=None):
    """Tiles of the pictures of a packed buffer letterboxed into network frames in one launch (yk_letterbox_tiles_u8): `packed` cuda uint8
    [bytes]; `table` a host table of tiles.TILE_DTYPE (checked here: a row the kernel would answer with zeros is refused) or the device table
    tile_table_to_device returned for this dst_hw.  -> cuda uint8 [n, H, W, 3]; frame t is bit for bit letterbox_u8 of a contiguous copy of
    tile t."""
    return _letterbox_rows_u8(_TILE, packed, table, dst_hw, stream, out)


def merge_tiles_lds_candidates(n_tiles: int, n_pics: int, max_out: int) -> int:
    """Candidates of one (picture, class) that merge_tiles with these sizes stages in LDS on the current device; more take the global path."""
    n = lib().yk_merge_tiles_lds_candidates(int(n_tiles), int(n_pics), int(max_out))
    if n < 0:
        _check(n, 'yk_merge_tiles_lds_candidates')
    return int(n)


def merge_tiles(dets, counts, origins, first, class_num: int, max_out: int, thresh: float = 0.5, metric: str = 'ios', stream=None,
                out=None, out_counts=None):
    """The rows of tile frames merged into one padded row set per picture (yk_merge_tiles; the rule is tiles.merge): dets cuda fp32
    [n_tiles, class_num * max_out, 6] and counts cuda int32 [n_tiles] as decode_py / Pipeline.submit leave them; origins (y0, x0) per tile and
    first [n_pics + 1] (the tiles of picture p are first[p] .. first[p + 1] - 1), host arrays or cuda float32 [n_tiles, 2] / int32 [n_pics + 1].
    -> (rows cuda fp32 [n_pics, class_num * max_out, 6], counts cuda int32 [n_pics])."""
    import torch
    from . import tiles
    require_gpu()
    try:
        method = tiles.metric_id(metric)
    except ValueError as e:
        raise YkError(str(e)) from None
    cap = int(class_num) * int(max_out)
    assert dets.is_cuda and dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 3 and tuple(dets.shape[1:]) == (cap, 6), tuple(dets.shape)
    n_tiles = int(dets.shape[0])
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (n_tiles,)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        if not torch.is_tensor(origins):
            origins = torch.from_numpy(np.ascontiguousarray(origins, np.float32).reshape(-1, 2)).to(dets.device)
        if not torch.is_tensor(first):
            first = torch.from_numpy(np.ascontiguousarray(first, np.int32).reshape(-1)).to(dets.device)
    assert origins.is_cuda and origins.dtype == torch.float32 and origins.is_contiguous() and tuple(origins.shape) == (n_tiles, 2), tuple(origins.shape)
    assert first.is_cuda and first.dtype == torch.int32 and first.is_contiguous() and first.dim() == 1 and first.numel() >= 2
    n_pics = int(first.numel()) - 1
    if out is None:
        out = torch.zeros((n_pics, cap, 6), dtype=torch.float32, device=dets.device)
    if out_counts is None:
        out_counts = torch.zeros((n_pics,), dtype=torch.int32, device=dets.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_pics, cap, 6), tuple(out.shape)
    assert out_counts.is_cuda and out_counts.dtype == torch.int32 and out_counts.is_contiguous() and tuple(out_counts.shape) == (n_pics,)
    call('yk_merge_tiles', dets, counts, origins, first, n_tiles, n_pics, int(class_num), int(max_out), float(thresh), method, out, out_counts,
         _stream(stream))
    return out, out_counts


def check_view_rows(table, packed_bytes: int) -> np.ndarray:
    """The rows of a host view table (tta.VIEW_DTYPE = yk_view_row_t) as one flat copy, refused with YkError unless every row is a non-empty
    picture inside the `packed_bytes` of its buffer and inside its canvas: what yk_letterbox_views_u8 would otherwise answer with a zero
    frame."""
    return _check_rows(_VIEW, table, packed_bytes)


def view_table_to_device(table, dst_hw, packed_bytes: int, device, stream=None):
    """A host view table (tta.table_rows) checked (check_view_rows), its scale / tx / ty filled for the network size dst_hw and uploaded
    -> cuda uint8 [n, 56], what letterbox_views_u8 takes as its table."""
    return _table_to_device(_VIEW, table, dst_hw, packed_bytes, device, stream)


def letterbox_views_u8(packed, table, dst_hw, stream=None, out=None):
    """Views of the pictures of a packed buffer (test-time augmentation, tta.py) letterboxed into network frames in one launch
    (yk_letterbox_views_u8): `packed` cuda uint8 [bytes]; `table` a host table of tta.VIEW_DTYPE (checked here: a row the kernel would answer
    with zeros is refused) or the device table view_table_to_device returned for this dst_hw.  -> cuda uint8 [n, H, W, 3]; frame v is bit for
    bit letterbox_u8 of the canvas of view v (tta.canvas)."""
    return _letterbox_rows_u8(_VIEW, packed, table, dst_hw, stream, out)


def fuse_views_lds_candidates(max_out: int) -> int:
    """Candidates of one (picture, class), views * max_out, that fuse_views holds in LDS on the current device; more are refused."""
    n = lib().yk_fuse_views_lds_candidates(int(max_out))
    if n < 0:
        _check(n, 'yk_fuse_views_lds_candidates')
    return int(n)


def fuse_views(dets, counts, xforms, views: int, class_num: int, max_out: int, thresh: float = 0.55, stream=None, out=None, out_counts=None):
    """The rows of view frames fused into one padded row set per picture (yk_fuse_views; the rule is tta.fuse): dets cuda fp32
    [n_pics * views, class_num * max_out, 6] and counts cuda int32 [n_pics * views] as decode_py / Pipeline.submit leave them, the frames of
    picture p being p * views .. (p + 1) * views - 1; xforms (dy, dx, mw) per frame (tta.xforms), a host array or cuda float32
    [n_pics * views, 3].  -> (rows cuda fp32 [n_pics, class_num * max_out, 6], counts cuda int32 [n_pics])."""
    import torch
    require_gpu()
    cap = int(class_num) * int(max_out)
    views = int(views)
    assert dets.is_cuda and dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 3 and tuple(dets.shape[1:]) == (cap, 6), tuple(dets.shape)
    n_frames = int(dets.shape[0])
    if views < 1 or n_frames % views:
        raise YkError(f'fuse_views: {n_frames} frames are not whole pictures of {views} views')
    n_pics = n_frames // views
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (n_frames,)
    if not torch.is_tensor(xforms):
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            xforms = torch.from_numpy(np.ascontiguousarray(xforms, np.float32).reshape(-1, 3)).to(dets.device)
    assert xforms.is_cuda and xforms.dtype == torch.float32 and xforms.is_contiguous() and tuple(xforms.shape) == (n_frames, 3), tuple(xforms.shape)
    if out is None:
        out = torch.zeros((n_pics, cap, 6), dtype=torch.float32, device=dets.device)
    if out_counts is None:
        out_counts = torch.zeros((n_pics,), dtype=torch.int32, device=dets.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_pics, cap, 6), tuple(out.shape)
    assert out_counts.is_cuda and out_counts.dtype == torch.int32 and out_counts.is_contiguous() and tuple(out_counts.shape) == (n_pics,)
    call('yk_fuse_views', dets, counts, xforms, views, n_pics, int(class_num), int(max_out), float(thresh), out, out_counts, _stream(stream))
    return out, out_counts


def mosaic_ragged_u8(packed, table, centres, dst_hw, inv=None, stream=None, out=None):
    """One training frame from four pictures per sample, the whole batch in one launch (yk_mosaic_ragged_u8; the rule is in mosaic.py):
    `packed` cuda uint8 [bytes], the pictures of draw.pack_ragged; `table` the samples' rows in quadrant order with scale / tx / ty filled
    (mosaic.ragged_rows), either a host array of draw.RAGGED_DTYPE [n, 4] or [4n] - checked here: a row without pixels, or one that leaves
    the buffer, is refused - or cuda uint8 [4n, 40]; `centres` the seams (cx, cy), a host array or cuda int32 [n, 2]; `inv` each sample's
    inverse map of augment.py, cuda float64 [n, 6] or [n, 2, 3], or None for no warp.  -> cuda uint8 [n, H, W, 3]."""
    import torch
    from .draw import RAGGED_DTYPE
    require_gpu()
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() > 0
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        if not torch.is_tensor(table):
            t = check_ragged_rows(table, packed.numel())
            if len(t) == 0 or len(t) % 4:
                raise YkError(f'mosaic table: {len(t)} rows, a sample has four')
            table = torch.from_numpy(t.view(np.uint8).reshape(len(t), RAGGED_DTYPE.itemsize)).to(packed.device)
        if not torch.is_tensor(centres):
            centres = torch.from_numpy(np.ascontiguousarray(centres, np.int32)).to(packed.device)
    assert table.is_cuda and table.dtype == torch.uint8 and table.is_contiguous() and table.dim() == 2 and table.device == packed.device
    assert table.shape[1] == RAGGED_DTYPE.itemsize and table.shape[0] > 0 and table.shape[0] % 4 == 0, tuple(table.shape)
    n = int(table.shape[0]) // 4
    assert centres.is_cuda and centres.dtype == torch.int32 and centres.is_contiguous() and centres.numel() == 2 * n and centres.device == packed.device
    if inv is not None:
        assert inv.is_cuda and inv.dtype == torch.float64 and inv.is_contiguous() and inv.numel() == 6 * n and inv.device == packed.device
    if out is None:
        out = torch.empty((n, int(dst_hw[0]), int(dst_hw[1]), 3), dtype=torch.uint8, device=packed.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, int(dst_hw[0]), int(dst_hw[1]), 3), tuple(out.shape)
    call('yk_mosaic_ragged_u8', packed, packed.numel(), table, centres, inv, n, out, out.shape[1], out.shape[2], _stream(stream))
    return out


def hsv_jitter_u8(frames, params, stream=None):
    """HSV colour jitter of finished frames, in place (yk_hsv_jitter_u8; the rule is in colour.py): `frames` cuda uint8 [n, H, W, 3]
    contiguous; `params` each frame's (dh, gs, gv), either cuda float64 [n, 3] - the kernel leaves the frame of a row that is not finite
    or has a negative gain untouched - or a host array [n, 3], checked here (such a row is refused) and uploaded.  -> `frames`."""
    import torch
    from . import colour
    require_gpu()
    assert torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous(), 'frames: cuda uint8, contiguous'
    assert frames.dim() == 4 and frames.shape[-1] == 3 and frames.shape[1] > 0 and frames.shape[2] > 0, tuple(frames.shape)
    n = int(frames.shape[0])
    if not torch.is_tensor(params):
        try:
            host = colour.check_params(params, n)
        except ValueError as e:
            raise YkError(str(e)) from e
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            params = torch.from_numpy(host).to(frames.device)
    assert params.is_cuda and params.dtype == torch.float64 and params.is_contiguous() and params.device == frames.device
    assert tuple(params.shape) == (n, 3), tuple(params.shape)
    call('yk_hsv_jitter_u8', frames, n, frames.shape[1], frames.shape[2], params, _stream(stream))
    return frames


def make_label_cfg(helper, assign: str = 'best', assign_iou: float = 0.213) -> LabelCfg:
    """yk_label_cfg_t of a Helper: its grids, its anchors as float64 and the positive assignment (Helper.box_to_label).  CPU only."""
    from .helper import ASSIGN_MODES, Helper
    try:
        Helper.check_assign(assign, assign_iou)
    except ValueError as e:
        raise YkError(str(e)) from e
    anchors = [np.asarray(a, float).reshape(-1, 2) for a in helper.anchors]
    if not 1 <= len(anchors) <= YK_MAX_LAYERS or any(not 1 <= len(a) <= YK_MAX_ANCHORS for a in anchors):
        raise YkError(f'labels: {len(anchors)} layers of {[len(a) for a in anchors]} anchors: at most {YK_MAX_LAYERS} of {YK_MAX_ANCHORS}')
    cfg = LabelCfg()
    cfg.n_layers, cfg.class_num, cfg.assign, cfg.assign_iou = len(anchors), int(helper.class_num), ASSIGN_MODES[assign], float(assign_iou)
    for l, a in enumerate(anchors):
        cfg.out_h[l], cfg.out_w[l], cfg.anchor_num[l] = int(helper.out_hw[l][0]), int(helper.out_hw[l][1]), len(a)
        for k, (w, h) in enumerate(a):
            cfg.anchors[l][k][0], cfg.anchors[l][k][1] = float(w), float(h)
    return cfg


def boxes_to_labels(boxes, first, helper, assign: str = 'best', assign_iou: float = 0.213, stream=None, out=None, status=None):
    """The label grids of a batch, built on the device (yk_boxes_to_labels_f32; the rule is Helper.batch_box_to_label's, bit for bit):
    `boxes` [N, 5] float64 rows (cls, x, y, w, h) and `first` [n + 1] int32, sample i owning rows first[i] .. first[i + 1] - 1 - both either
    cuda tensors, or host arrays, which are checked here (rows that are not finite, offsets that do not ascend from 0 to N: refused) and
    uploaded.  -> ([one contiguous view [n, h, w, A, 5 + C] float32 per layer of ONE flat buffer], status): status is a cuda int32 [1] that
    holds INT32_MAX, or the smallest row of `boxes` that numpy could not have written (a cell outside its grid, a class outside
    [0, C)) and of which nothing was written.  out / status: buffers to reuse (cuda float32 [n * floats per sample], int32 [1]).  Does
    not synchronise."""
    import torch
    require_gpu()
    cfg = helper if isinstance(helper, LabelCfg) else make_label_cfg(helper, assign, assign_iou)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        if not torch.is_tensor(first):
            f = np.ascontiguousarray(first, np.int32).reshape(-1)
            b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 5) if not torch.is_tensor(boxes) else None
            if len(f) < 1 or f[0] != 0 or (np.diff(f) < 0).any() or (b is not None and f[-1] != len(b)):
                raise YkError(f'boxes_to_labels: first must ascend from 0 to the number of boxes, got {f.tolist()[:8]} ..')
            first = torch.from_numpy(f).cuda()
        if not torch.is_tensor(boxes):
            b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 5)
            if not np.isfinite(b).all():
                raise YkError(f'boxes_to_labels: box {int(np.nonzero(~np.isfinite(b).all(1))[0][0])} is not finite')
            boxes = torch.from_numpy(b).cuda()
        assert boxes.is_cuda and boxes.dtype == torch.float64 and boxes.is_contiguous() and boxes.dim() == 2 and boxes.shape[1] == 5, 'boxes: cuda float64 [N, 5]'
        assert first.is_cuda and first.dtype == torch.int32 and first.is_contiguous() and first.dim() == 1 and first.numel() >= 1 and first.device == boxes.device
        n = int(first.numel()) - 1
        shapes = [(n, int(cfg.out_h[l]), int(cfg.out_w[l]), int(cfg.anchor_num[l]), 5 + int(cfg.class_num)) for l in range(cfg.n_layers)]
        sizes = [int(np.prod(s, dtype=np.int64)) for s in shapes]
        if out is None:
            out = torch.empty((sum(sizes),), dtype=torch.float32, device=boxes.device)
        if status is None:
            status = torch.empty((1,), dtype=torch.int32, device=boxes.device)
        if n == 0:                                                          # (the library launches nothing)
            status.fill_(LABEL_STATUS_CLEAN)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == sum(sizes) and out.device == boxes.device
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() == 1 and status.device == boxes.device
    call('yk_boxes_to_labels_f32', C.byref(cfg), boxes if boxes.numel() else None, int(boxes.shape[0]), first, n, out, status, _stream(stream))
    views, at = [], 0
    for s, size in zip(shapes, sizes):
        views.append(out[at:at + size].view(s))
        at += size
    return views, status


def draw_detections_u8(packed, table, dets, counts, colormap, atlas, stream=None, max_pixels: Optional[int] = None):
    """Paint detections into the pictures of a ragged batch, in place and on the device (yk_draw_dets_u8; the rule is in include/yolo_hip.h):
    dets cuda fp32 [n, cap, 6] and counts cuda int32 [n] as decode_py / Pipeline.submit leave them, colormap cuda uint8 [n_colors, 3],
    atlas cuda uint8 [12, gh, gw] of 0 / 1 (draw.glyph_atlas; gh == 0 draws no label).  `table` as for letterbox_ragged_u8; with a device
    table pass max_pixels, the largest h * w of the batch."""
    import torch
    require_gpu()
    if not torch.is_tensor(table):
        t = np.asarray(table)
        max_pixels = int((t['h'].astype(np.int64) * t['w'].astype(np.int64)).max()) if len(t) else 0
    elif max_pixels is None:
        raise YkError('draw_detections_u8: a device table needs max_pixels')
    table = _device_table(_RAGGED, packed, table, None, stream)
    n = int(table.shape[0])
    assert dets.is_cuda and dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 3 and dets.shape[0] == n and dets.shape[2] == 6
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (n,)
    assert colormap.is_cuda and colormap.dtype == torch.uint8 and colormap.is_contiguous() and colormap.dim() == 2 and colormap.shape[1] == 3
    assert atlas.is_cuda and atlas.dtype == torch.uint8 and atlas.is_contiguous() and atlas.dim() == 3 and atlas.shape[0] == 12
    call('yk_draw_dets_u8', packed, packed.numel(), table, n, dets, dets.shape[1], counts, colormap, colormap.shape[0],
         atlas if atlas.numel() else None, atlas.shape[1], atlas.shape[2], int(max_pixels), _stream(stream))
    return packed


def jpeg_tables(quality: int = 75) -> np.ndarray:
    """yk_jpeg_tables: the Annex K.1 tables scaled by the IJG rule -> uint8 [2, 64], natural order (what jpeg.quant_tables states in numpy)."""
    q = np.zeros((2, 64), np.uint8)
    call('yk_jpeg_tables', int(quality), q)
    return q


def jpeg_workspace_bytes(table) -> Tuple[int, int]:
    """yk_jpeg_workspace_bytes for a host table: (bytes of scratch, capacity of the output) from the worst case per 8x8 block."""
    from .draw import RAGGED_DTYPE
    t = np.ascontiguousarray(np.asarray(table, dtype=RAGGED_DTYPE).reshape(-1))
    work, cap = C.c_size_t(0), C.c_size_t(0)
    call('yk_jpeg_workspace_bytes', t, len(t), C.byref(work), C.byref(cap))
    return int(work.value), int(cap.value)


def jpeg_encode_ragged_u8(packed, table, qtab, stream=None, sizes=None, work=None, out=None, out_off=None):
    """JPEG-encode the pictures of a ragged batch on the device (yk_jpeg_encode_ragged_u8; the rule is in include/yolo_hip.h): `packed` and
    `table` as for letterbox_ragged_u8 (a host table is checked here: a row without pixels, or one that leaves the buffer, is refused),
    qtab cuda uint8 [2, 64] (jpeg_tables).  With a device table pass sizes = jpeg_workspace_bytes(host table).  work / out / out_off: cuda
    buffers to reuse (uint8 [>= sizes[0]], uint8 [>= sizes[1]], int64 [n + 1]); allocated when None.  -> (out, out_off): the scan data of
    picture i is out[out_off[i]:out_off[i + 1]]; jpeg.assemble puts the file around it.  Does not synchronise."""
    import torch
    require_gpu()
    if not torch.is_tensor(table):
        sizes = jpeg_workspace_bytes(table)
    elif sizes is None:
        raise YkError('jpeg_encode_ragged_u8: a device table needs sizes = jpeg_workspace_bytes(host table)')
    table = _device_table(_RAGGED, packed, table, None, stream)
    n = int(table.shape[0])
    dev = packed.device
    if work is None:
        work = torch.empty(sizes[0], dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(sizes[1], dtype=torch.uint8, device=dev)
    if out_off is None:
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    assert qtab.is_cuda and qtab.dtype == torch.uint8 and qtab.is_contiguous() and tuple(qtab.shape) == (2, 64)
    assert work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    assert out_off.is_cuda and out_off.dtype == torch.int64 and out_off.is_contiguous() and out_off.numel() == n + 1
    if work.numel() < sizes[0] or out.numel() < sizes[1]:
        raise YkError(f'jpeg_encode_ragged_u8: work {work.numel()} / out {out.numel()} bytes, the batch needs {sizes[0]} / {sizes[1]}')
    call('yk_jpeg_encode_ragged_u8', packed, packed.numel(), table, n, qtab, work, work.numel(), out, out.numel(), out_off, _stream(stream))
    return out, out_off


class JpegPic(C.Structure):
    """yk_jpeg_pic_t (numpy: jpeg.PIC_DTYPE)"""
    _fields_ = [('scan_offset', C.c_uint64), ('scan_bytes', C.c_uint32), ('table_offset', C.c_uint32), ('h', C.c_int32), ('w', C.c_int32),
                ('ncomp', C.c_int32), ('hs', C.c_int32), ('vs', C.c_int32), ('restart', C.c_int32), ('tq', C.c_uint8 * 4),
                ('td', C.c_uint8 * 4), ('ta', C.c_uint8 * 4), ('reserved', C.c_uint32)]


class RaggedRow(C.Structure):
    """yk_ragged_row_t (numpy: draw.RAGGED_DTYPE)"""
    _fields_ = [('offset', C.c_uint64), ('h', C.c_int32), ('w', C.c_int32), ('scale', C.c_double), ('tx', C.c_int32), ('ty', C.c_int32),
                ('thickness', C.c_int32), ('mag', C.c_int32)]


assert C.sizeof(JpegPic) == 56 and C.sizeof(RaggedRow) == 40


def jpeg_decode_workspace_bytes(pics) -> int:
    """yk_jpeg_decode_workspace_bytes for a host table of jpeg.PIC_DTYPE rows (jpeg.plan_decode): bytes of scratch."""
    from .jpeg import PIC_DTYPE
    t = np.ascontiguousarray(np.asarray(pics, dtype=PIC_DTYPE).reshape(-1))
    work = C.c_size_t(0)
    call('yk_jpeg_decode_workspace_bytes', t, len(t), C.byref(work))
    return int(work.value)


def jpeg_decode_ragged_u8(scan, pics, tables, rows, dst, stream=None, work_bytes=None, work=None, status=None, chunk_bytes: int = 0):
    """Decode baseline JPEGs into a ragged packed buffer on the device (yk_jpeg_decode_ragged_u8; the rule is in include/yolo_hip.h): scan
    and tables cuda uint8 (jpeg.plan_decode's buffer, split at its scan_bytes), pics its host table of jpeg.PIC_DTYPE or that table on the
    device as cuda uint8 [n, 56] (then pass work_bytes = jpeg_decode_workspace_bytes(host table)), rows the destination's ragged table
    (host, or cuda uint8 [n, 40]), dst cuda uint8: picture i is written as [h, w, 3] at dst[rows[i].offset:].  work / status: cuda buffers to
    reuse (uint8 [>= work_bytes], int32 [n]).  -> status, 0 per decoded picture.  Does not synchronise."""
    import torch
    from .draw import RAGGED_DTYPE
    from .jpeg import PIC_DTYPE
    require_gpu()
    dev = dst.device
    if not torch.is_tensor(pics):
        t = np.ascontiguousarray(np.asarray(pics, dtype=PIC_DTYPE).reshape(-1))
        work_bytes = jpeg_decode_workspace_bytes(t)
        pics = torch.from_numpy(t.view(np.uint8).reshape(len(t), PIC_DTYPE.itemsize)).to(dev)
    elif work_bytes is None:
        raise YkError('jpeg_decode_ragged_u8: a device table needs work_bytes = jpeg_decode_workspace_bytes(host table)')
    if not torch.is_tensor(rows):
        t = np.ascontiguousarray(np.asarray(rows, dtype=RAGGED_DTYPE).reshape(-1))
        rows = torch.from_numpy(t.view(np.uint8).reshape(len(t), RAGGED_DTYPE.itemsize)).to(dev)
    n = int(pics.shape[0])
    for t_, width in ((pics, PIC_DTYPE.itemsize), (rows, RAGGED_DTYPE.itemsize)):
        assert t_.is_cuda and t_.dtype == torch.uint8 and t_.is_contiguous() and tuple(t_.shape) == (n, width), tuple(t_.shape)
    for t_ in (scan, tables, dst):
        assert t_.is_cuda and t_.dtype == torch.uint8 and t_.is_contiguous() and t_.numel() > 0
    if work is None:
        work = torch.empty(int(work_bytes), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    assert work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous()
    assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == n
    if work.numel() < int(work_bytes):
        raise YkError(f'jpeg_decode_ragged_u8: work {work.numel()} bytes, the batch needs {int(work_bytes)}')
    call('yk_jpeg_decode_ragged_u8', scan, scan.numel(), pics, tables, tables.numel(), rows, n, dst, dst.numel(), work, work.numel(), status,
         int(chunk_bytes), _stream(stream))
    return status


class Graph:
    """A captured step (yk_graph_*, include/yolo_hip.h): one host call replays every launch recorded between begin and end."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle

    @property
    def nodes(self) -> int:
        return int(lib().yk_graph_node_count(self._h)) if self._h else 0

    @property
    def kernel_nodes(self) -> int:
        return int(lib().yk_graph_kernel_node_count(self._h)) if self._h else 0

    def launch(self, stream_handle: C.c_void_p) -> None:
        _check(_handles_only('yk_graph_launch')(self._h, stream_handle), 'yk_graph_launch')

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib().yk_graph_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def capture(stream_handle: C.c_void_p, issue) -> Graph:
    """Record what `issue()` submits to the stream as a Graph.  The stream must have run the same step eagerly before."""
    L = lib()
    call('yk_graph_begin', stream_handle)
    try:
        issue()
    except Exception:
        h = C.c_void_p()
        L.yk_graph_end(stream_handle, C.byref(h))                  # leave capture mode whatever happened
        if h.value:
            L.yk_graph_destroy(h)
        raise
    h = C.c_void_p()
    call('yk_graph_end', stream_handle, C.byref(h))
    return Graph(h)


def _pinned(shape, dtype):
    """Pinned host tensor + the address a kernel may use for it."""
    import torch
    t = torch.empty(shape, dtype=dtype).pin_memory()
    d = C.c_void_p()
    call('yk_host_device_ptr', t, C.byref(d))
    return t, d


class Ticket:
    """One batch submitted from host memory (Pipeline.submit_host).  `result()` waits for it and returns (rows [n,6] float32 =
    top,left,bottom,right,score,class ; offsets [B+1] int32: image b owns rows[offsets[b]:offsets[b+1]]) - the concatenation of
    keras_inference.py:133-135, for every image of the batch.  Valid until the slot is reused `depth` submits later."""

    def __init__(self, slot, batch, event, with_index):
        self._slot, self.batch, self.event, self._with_index = slot, batch, event, with_index

    def result(self):
        self.event.synchronize()
        s = self._slot
        s.plan.raise_if_failed()
        off = s.h_offsets[:self.batch + 1].numpy().copy()
        n = int(off[-1])
        rows = s.h_rows[:n].numpy().copy()
        if self._with_index:
            return rows, off, s.h_index[:n].numpy().copy()
        return rows, off


class _Slot:
    pass


class Pipeline:
    """Several independent batches in flight on one GPU (the kpu_run_kmodel(async)+callback shape of main.c:303-311, widened).

    One batch alone leaves CUs idle: a step is ~27 dependent launches, most of them a single round of <= 256 workgroups.
    `depth` plans, each with its own outputs / split-K slabs, on `depth` HIP streams (decode scratch is per stream inside the
    library) let the GPU interleave workgroups of different batches; nothing is shared between them but the weight values.

    graph=True (default): a slot's step - (letterbox) -> yk_run_u8 -> decode + per-class NMS -> results - is captured once as a
    hipGraph and REPLAYED: one host call per batch instead of ~30 launches (the host -> device copy of submit_host runs in front of it on the
    pipeline's copy stream, into one of the slot's two device input buffers, under the slot's previous batch).  A captured step is bound to the
    buffers it was captured with: device frames are replayed in place when they live at an address the slot has already captured
    (the slot's own `input(i)` buffer, or up to two caller buffers - a resident ring), and are copied into `input(i)` otherwise.

    submit() returns at once; the returned (dets, counts) tensors belong to that slot and are overwritten when the slot is reused
    `depth` submits later, so consume them (or call `wait`) before that.  submit_host() takes frames from (pinned) host memory and
    delivers the detections to host memory at their live size; see Ticket."""

    def __init__(self, spec: ns.NetSpec, weights, anchors, max_batch: int = 32, depth: int = 3, device: Optional[int] = None,
                 precision: str = 'f16x2', graph: bool = True, src_hw: Optional[Tuple[int, int]] = None, max_out: int = 30,
                 schedule: str = 'auto', streams: str = 'native'):
        """schedule: 'auto' = 'latency' for depth 1 (one batch at a time: the cluster launches finish it soonest), 'throughput' for
        depth >= 2 (batches in flight on several streams: the launch-per-layer form overlaps better); see Plan.
        streams: 'native' = the slots' HIP streams are created by the library, back to back (yk_stream_create): they land on
        consecutive hardware queues whatever streams the process created before; 'torch' = streams from torch's pool."""
        import torch
        require_gpu()
        if streams not in ('native', 'torch'):
            raise YkError(f'streams {streams!r}: expected native or torch')
        self.depth = max(1, int(depth))
        self.schedule = ('latency' if self.depth == 1 else 'throughput') if schedule == 'auto' else schedule
        self.spec, self.max_batch, self.graph = spec, int(max_batch), bool(graph)
        self.src_hw = None if src_hw is None else (int(src_hw[0]), int(src_hw[1]))     # frames of this size are letterboxed on the GPU
        self.max_out = int(max_out)
        self.plans = [Plan(spec, weights, max_batch=max_batch, device=device, precision=precision, schedule=self.schedule) for _ in range(self.depth)]
        self.outs = [p.outputs() for p in self.plans]
        dev = torch.device(f'cuda:{self.plans[0].device}')
        cur = torch.cuda.current_stream()
        self._own_streams = []
        if streams == 'native':
            with torch.cuda.device(dev):
                for _ in range(self.depth):
                    h = C.c_void_p()
                    call('yk_stream_create', C.byref(h), 0)
                    self._own_streams.append(h)
            self.streams = [torch.cuda.ExternalStream(h.value, device=dev) for h in self._own_streams]
        else:
            self.streams = [torch.cuda.Stream(device=dev) for _ in range(self.depth)]
        for s in self.streams:
            s.wait_stream(cur)
        self.cfg = make_decode_cfg(anchors, spec.class_num, spec.in_hw, spec.out_hw())
        B, H, W = self.max_batch, *spec.in_hw
        nrow = spec.class_num * self.max_out
        self.slots = []
        for i in range(self.depth):
            s = _Slot()
            s.plan, s.stream, s.st = self.plans[i], self.streams[i], C.c_void_p(self.streams[i].cuda_stream)
            s.preds = (C.c_void_p * len(self.outs[i]))(*[o.data_ptr() for o in self.outs[i]])
            s.frames = torch.full((B, H, W, 3), 127, dtype=torch.uint8, device=dev)      # (defined bytes: the warm-up step reads them)
            s.src = torch.full((B, *self.src_hw, 3), 127, dtype=torch.uint8, device=dev) if self.src_hw else s.frames
            s.image_hw = torch.empty((B, 2), dtype=torch.float32, device=dev)
            s.dets = torch.zeros((B, nrow, 6), dtype=torch.float32, device=dev)
            s.counts = torch.zeros((B,), dtype=torch.int32, device=dev)
            s.index = torch.full((B, nrow), -1, dtype=torch.int32, device=dev)
            s.h_src = s.h_rows = s.h_offsets = s.h_index = None                        # pinned side, built on first submit_host
            s.graphs = {}
            s.scratch_gen, s.warm_dev, s.warm_host = 0, False, False
            s.foreign = []                                                              # caller buffers this slot has captured
            self.slots.append(s)
        self._n = 0
        self.host_us = 0.0
        self.host_wait_us = 0.0                                                         # submit_host: time the submit thread spent BLOCKED on a slot's input buffer (cumulative)
        self._copy_stream = None                                                        # submit_host: the H2D leg's own stream (created on first use)
        self._copy_st = None                                                            # ... and its handle, as the library takes it

    # -- buffers ------------------------------------------------------------------------------------
    def input(self, i: int):
        """Slot i's own device input [max_batch, h, w, 3] uint8 (camera size when src_hw is set): fill it, then submit(None)."""
        return self.slots[i % self.depth].src

    def host_input(self, i: int):
        """Slot i's pinned host input (same shape as input(i)): fill it, then submit_host(None)."""
        s = self.slots[i % self.depth]
        self._host_side(s)
        return s.h_src

    def next_slot(self) -> int:
        return self._n % self.depth

    def _host_side(self, s):
        import torch
        if s.h_src is None:
            nrow = self.max_batch * self.spec.class_num * self.max_out
            s.h_src, _ = _pinned(tuple(s.src.shape), torch.uint8)
            s.h_rows, s.d_rows = _pinned((nrow, 6), torch.float32)
            s.h_offsets, s.d_offsets = _pinned((self.max_batch + 1,), torch.int32)
            s.h_index, s.d_index = _pinned((nrow,), torch.int32)
            s.h_offsets.zero_()
            # the frames of a host batch land in one of TWO device buffers, copied on the pipeline's copy stream: the copy of this slot's
            # next batch runs under its current batch's kernels instead of in front of them on the same stream (round 5: the copy leg is
            # 125 us of a 330 us step, and a stream that copies is a stream that does not compute - from host 0.87 of resident before)
            s.h2d_bufs = [s.src, torch.full_like(s.src, 127)]
            # the copy's arguments prebuilt, like s.st: submit_host is timed, and its host thread is the busy one
            s.h2d_ptrs, s.h_src_ptr, s.frame_bytes = [C.c_void_p(t.data_ptr()) for t in s.h2d_bufs], C.c_void_p(s.h_src.data_ptr()), s.src[0].numel()
            s.h2d_next = 0
            s.h2d_copied = [torch.cuda.Event(), torch.cuda.Event()]
            s.staged = None                                         # (buffer index, batch) of a copy stage_host() has started
            s.h2d_free = [None, None]
            if self._copy_stream is None:
                if self._own_streams:                                   # library-created, like the slots' streams
                    h = C.c_void_p()
                    with torch.cuda.device(s.src.device):
                        call('yk_stream_create', C.byref(h), 0)
                    self._own_streams.append(h)
                    self._copy_stream = torch.cuda.ExternalStream(h.value, device=s.src.device)
                else:
                    self._copy_stream = torch.cuda.Stream(device=s.src.device)
                self._copy_st = C.c_void_p(self._copy_stream.cuda_stream)

    # -- the step, as the library calls it is made of (eager, or recorded by capture()) ---------------------------------
    def _h2d_start(self, s, B):
        """Issue the host -> device copy of slot `s`'s pinned frames into its other device input buffer, on the pipeline's COPY stream (the copy of
        a slot's next batch runs under its current batch's kernels).  -> the buffer's index; `s.h2d_copied[b]` fires when the frames are there."""
        import time
        b = s.h2d_next
        s.h2d_next ^= 1
        cs = self._copy_stream
        if s.h2d_free[b] is not None and not s.h2d_free[b].query():
            # the batch that last read this buffer (two submits of this slot ago) - waited for on the HOST, where it is over long ago in steady
            # state: a wait inside the copy stream would put barrier packets into a fifth hardware queue, and a fifth active queue costs the
            # four compute streams a quarter of their rate (measured 85 -> 61 k images/s)
            t0 = time.perf_counter()
            s.h2d_free[b].synchronize()
            self.host_wait_us += (time.perf_counter() - t0) * 1e6      # blocked, not busy: bench.py reports the two apart
        _check(_handles_only('yk_memcpy_async')(s.h2d_ptrs[b], s.h_src_ptr, B * s.frame_bytes, self._copy_st), 'yk_memcpy_async')
        s.h2d_copied[b].record(cs)
        return b

    def stage_host(self, i: Optional[int] = None, batch: Optional[int] = None) -> None:
        """The frames in host_input(i) are final (default: the slot of the next submit): start their copy to the device NOW, so that it runs
        while earlier batches compute and `submit_host(None)` of that slot finds it done.  A producer calls this when it has filled a slot;
        bench.py calls it one submit ahead.  Optional: without it submit_host issues the copy itself."""
        s = self.slots[(self._n if i is None else int(i)) % self.depth]
        self._host_side(s)
        B = self.max_batch if batch is None else int(batch)
        if getattr(s, 'staged', None) is None:
            s.staged = (self._h2d_start(s, B), B)

    def _h2d(self, s, B):
        """The host -> device leg, issued EAGERLY in front of the replay (measured, images/s from host with four batches in flight: copy
        engine in front of the replay 66 k; as a copy node inside the captured step 55 k; as a kernel inside it that reads the pinned
        frames through their device alias 54 k - profiles/r04_schedules.txt) on the pipeline's COPY stream into the slot's other input buffer.
        The step is launched when the HOST has seen the copy finish (round 6: tools/from_host_split.py, one box, resident 99.7 k: the slot's
        stream waiting for the copy's event 91.4 k - a cross-queue barrier packet per step; the host waiting 92.5 k; the host waiting for a copy
        that stage_host() started one submit earlier 94.8 k = what the copy traffic alone costs).  -> the device address the step reads."""
        import time
        st = getattr(s, 'staged', None)
        s.staged = None
        b = st[0] if st is not None and st[1] == B else self._h2d_start(s, B)
        if not s.h2d_copied[b].query():
            t0 = time.perf_counter()
            s.h2d_copied[b].synchronize()
            self.host_wait_us += (time.perf_counter() - t0) * 1e6
        s.h2d_last = b
        return s.h2d_bufs[b].data_ptr()

    def _h2d_done(self, s):
        """After the step has been given to the slot's stream: its input buffer is free once the stream gets here."""
        import torch
        ev = torch.cuda.Event()
        ev.record(s.stream)
        s.h2d_free[s.h2d_last] = ev

    def _issue(self, s, B, src_ptr, host, use_hw, obj, iou, max_out, want_index, nms='hard', sigma=0.5):
        H, W = self.spec.in_hw
        x = src_ptr
        if self.src_hw:
            call('yk_letterbox_u8', x, B, self.src_hw[0], self.src_hw[1], s.frames, H, W, s.st)
            x = s.frames
        call('yk_run_u8', s.plan._h, x, B, s.st)
        ihw = s.image_hw if use_hw else None
        if nms != 'hard':
            method = _nms_method(nms, sigma)
            if host:
                call('yk_decode_py_packed_nms', C.byref(self.cfg), s.preds, B, ihw, obj, iou, max_out, s.d_rows, s.d_offsets,
                     s.d_index if want_index else None, None, None, s.st, method, sigma)
            else:
                call('yk_decode_py_nms', C.byref(self.cfg), s.preds, B, ihw, obj, iou, max_out, s.dets, s.counts,
                     s.index if want_index else None, s.st, method, sigma)
        elif host:
            call('yk_decode_py_packed', C.byref(self.cfg), s.preds, B, ihw, obj, iou, max_out, s.d_rows, s.d_offsets,
                 s.d_index if want_index else None, None, None, s.st)
        else:
            call('yk_decode_py_ex', C.byref(self.cfg), s.preds, B, ihw, obj, iou, max_out, s.dets, s.counts,
                 s.index if want_index else None, s.st)

    GRAPH_CACHE = 8                     # captured steps kept per slot (one per distinct (batch, source, thresholds, ...) combination)

    def _drop_graphs(self, s):
        for g in s.graphs.values():
            g.close()
        s.graphs.clear()

    def _run(self, s, B, src_ptr, host, use_hw, obj, iou, max_out, want_index, nms='hard', sigma=0.5):
        if nms != 'hard':
            _nms_method(nms, sigma)                                # refused by name before anything is issued or captured
        if max_out > self.max_out:
            raise YkError(f'max_out {max_out} > the pipeline\'s max_out {self.max_out}')
        if host:
            src_ptr = self._h2d(s, B)
        args = (B, src_ptr, host, use_hw, float(obj), float(iou), int(max_out), bool(want_index), nms, float(sigma) if nms == 'gaussian' else 0.0)
        if not self.graph:
            self._issue(s, *args)
            if host:
                self._h2d_done(s)
            return
        # a captured step holds the address of the stream's decode scratch: if that buffer has moved since (it cannot once the slot is
        # warm - __init__ sizes it for max_batch x max_out - but another user of the same stream could grow it), every capture is stale
        gen = _handles_only('yk_scratch_generation')(s.st)
        if gen != s.scratch_gen:
            s.stream.synchronize()
            self._drop_graphs(s)
            s.scratch_gen = gen
        g = s.graphs.pop(args, None)
        if g is None:
            self._warm(s, host)
            if len(s.graphs) >= self.GRAPH_CACHE:                  # least recently used first (dicts keep insertion order)
                s.stream.synchronize()
                s.graphs.pop(next(iter(s.graphs))).close()
            g = capture(s.st, lambda: self._issue(s, *args))
        s.graphs[args] = g                                         # (re-)inserted last = most recently used
        g.launch(s.st)
        if host:
            self._h2d_done(s)

    def _warm(self, s, host):
        """One eager step at the slot's LARGEST shape (max_batch images, max_out rows per class, box indices on) for each result form the
        slot uses: sizes the library's per-stream scratch once, so that no later batch size or threshold can make it grow - and move -
        under a captured step."""
        B, did = self.max_batch, False
        if not s.warm_dev:
            self._issue(s, B, s.src.data_ptr(), False, False, 0.7, 0.5, self.max_out, True)
            s.warm_dev = did = True
        if host and not s.warm_host:
            self._issue(s, B, s.src.data_ptr(), True, False, 0.7, 0.5, self.max_out, True)
            s.warm_host = did = True
        if did:
            s.stream.synchronize()
            gen = int(lib().yk_scratch_generation(s.st))
            if gen != s.scratch_gen:                               # the warm-up itself moved a buffer older captures point into
                self._drop_graphs(s)
                s.scratch_gen = gen

    def _set_hw(self, s, B, image_hw):
        import torch
        if image_hw is None:
            return False
        hw = torch.as_tensor(np.broadcast_to(np.asarray(image_hw, np.float32), (B, 2)).copy())
        with torch.cuda.stream(s.stream):
            s.image_hw[:B].copy_(hw, non_blocking=False)
        return True

    def submit(self, frames_u8=None, image_hw=None, obj_thresh: float = 0.7, iou_thresh: float = 0.5, max_out: int = 30,
               return_index: bool = False, batch: Optional[int] = None, sync_input: bool = True, nms: str = 'hard', sigma: float = 0.5):
        """frames_u8: cuda uint8 [B,h,w,3] that stays alive until the results are consumed (None: the slot's own input(i) buffer, `batch`
        images of it).  -> (dets [B, C*max_out, 6], counts [B], stream[, box_index [B, C*max_out]]) - the slot's tensors, sliced to B."""
        import time
        import torch
        t0 = time.perf_counter()
        s = self.slots[self._n % self.depth]
        self._n += 1
        if frames_u8 is None:
            B = self.max_batch if batch is None else int(batch)
            ptr = s.src.data_ptr()
        else:
            assert frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
            assert tuple(frames_u8.shape[1:]) == tuple(s.src.shape[1:]), (frames_u8.shape, s.src.shape)
            B = int(frames_u8.shape[0])
            if sync_input:
                s.stream.wait_stream(torch.cuda.current_stream())       # the frames may have been produced on the caller's stream
            ptr = frames_u8.data_ptr()
            if self.graph and ptr != s.src.data_ptr() and ptr not in s.foreign:
                if len(s.foreign) < 2:
                    s.foreign.append(ptr)                               # a resident caller buffer: replayed in place from now on
                else:
                    with torch.cuda.stream(s.stream):
                        s.src[:B].copy_(frames_u8, non_blocking=True)
                    ptr = s.src.data_ptr()
        assert 0 < B <= self.max_batch
        use_hw = self._set_hw(s, B, image_hw)
        self._run(s, B, ptr, False, use_hw, obj_thresh, iou_thresh, max_out, return_index, nms, sigma)
        self.host_us = (time.perf_counter() - t0) * 1e6
        if return_index:
            return s.dets[:B], s.counts[:B], s.stream, s.index[:B]
        return s.dets[:B], s.counts[:B], s.stream

    def submit_host(self, frames_u8=None, image_hw=None, obj_thresh: float = 0.7, iou_thresh: float = 0.5, max_out: int = 30,
                    return_index: bool = False, batch: Optional[int] = None, nms: str = 'hard', sigma: float = 0.5) -> Ticket:
        """frames_u8: host uint8 [B,h,w,3] (numpy or torch; copied into the slot's pinned buffer) or None = `batch` images already
        written to host_input(i).  The frames cross PCIe, the detections come back to pinned host memory at their live size."""
        import time
        import torch
        t0 = time.perf_counter()
        s = self.slots[self._n % self.depth]
        self._n += 1
        self._host_side(s)
        if frames_u8 is None:
            B = self.max_batch if batch is None else int(batch)
        else:
            f = torch.as_tensor(frames_u8)
            assert f.dtype == torch.uint8 and tuple(f.shape[1:]) == tuple(s.src.shape[1:]), f.shape
            B = int(f.shape[0])
            for ev in s.h2d_copied:                                     # the slot's previous copies may still be reading h_src
                ev.synchronize()
            s.staged = None                                             # (a copy staged from the buffer's previous contents is not this batch)
            s.h_src[:B].copy_(f)
        assert 0 < B <= self.max_batch
        use_hw = self._set_hw(s, B, image_hw)
        self._run(s, B, None, True, use_hw, obj_thresh, iou_thresh, max_out, return_index, nms, sigma)
        ev = torch.cuda.Event()
        ev.record(s.stream)
        self.host_us = (time.perf_counter() - t0) * 1e6
        return Ticket(s, B, ev, return_index)

    def wait(self):
        for s in self.streams:
            s.synchronize()
        for p in self.plans:
            p.raise_if_failed()

    def close(self):
        if self._copy_stream is not None:
            self._copy_stream.synchronize()
            self._copy_stream = None
        for s in self.streams:
            s.synchronize()
        for s in self.slots:
            self._drop_graphs(s)
        for p in self.plans:
            p.close()
        self.plans = []
        self.slots = []
        self.streams = []
        for h in self._own_streams:
            lib().yk_stream_destroy(h)
        self._own_streams = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
