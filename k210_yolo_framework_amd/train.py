"""Training step on MI355X (keras_train.py:73-98).

The reference's `train_model.fit` runs, per step: forward in training mode (batch-statistics BatchNorm), the YOLO
loss of every output layer (tools/utils.py:708-793) plus the l2(5e-4) kernel regulariser of every DarknetConv2D
(models/yolonet.py:245-250), TF autodiff, and keras Adam(lr, decay) (keras_train.py:73-76).  All of that is
TensorFlow in the reference; here each arithmetic op is a HIP kernel of libyolo_hip.so (csrc/yk_train.hip,
csrc/yk_loss.hip) called through the C-ABI, and this module is only the tape: it walks the NetSpec forwards and
backwards.  torch supplies device buffers, views/concat (data movement) and the gradient all-reduce (RCCL).

Data-parallel: one process per GPU, each with `per_rank_batch` images.  The loss divisor is the GLOBAL batch (what
Helper.batch_size is in the single-process reference), gradients are SUM-all-reduced in one flat bucket, BatchNorm
statistics stay per replica.  With world_size 1 this is exactly the reference's step.

Magnitude pruning (keras_train.py:59-71, tfmot prune_low_magnitude restated in prune.py): `Trainer(prune=PruneSchedule(...))` computes the
masks of the Conv2D kernels on the schedule's update steps and zeroes the masked weights at the start of every step (csrc/yk_prune.hip),
outside the captured graph like Adam.  With prune=None the step issues exactly the launches it issued before.

Quantisation-aware fine-tuning (qat.py): `Trainer(qat=QatConfig(...))` simulates the kmodel's 8-bit codes inside the step
(csrc/yk_qat.hip): every conv / depthwise kernel is read from the shadow buffer Pq = fq(P), every conv output and every concat is
fake-quantised over a range that follows the batches, the backward pass takes the straight-through gradient, and L2 and Adam act on the
latent P.  All of it is inside the captured graph.  With qat=None nothing is allocated and nothing is launched.

IoU box losses: `Trainer(box_loss='giou' | 'diou' | 'ciou', box_weight=...)` replaces the xy / wh terms of every layer's loss
by the IoU-family term of csrc/yk_loss.hip (yk_yolo_loss_ex).  Both live in `tr.hyper`, so they are part of the captured step and of its key,
and the validation pass uses the same loss.  With box_loss='mse' the step calls yk_yolo_loss as before.

Focal loss, label smoothing, IoU objectness target (lossopt.py): `Trainer(focal='obj' | 'cls' | 'all', focal_gamma=, focal_alpha=,
label_smooth=, obj_target='iou')` change the objectness and class terms inside the same loss kernel (yk_yolo_loss_opt).  They live in
`tr.hyper` like the box loss.  With all of them off the step calls yk_yolo_loss / yk_yolo_loss_ex as before.

Knowledge distillation (distill.py): `Trainer(distill=DistillConfig(teacher_spec, teacher_weights, weight))` runs the teacher as an
inference plan (engine.Plan, f16x2) on the step's frames, outside the captured graph, copies its raw outputs into static buffers, and adds
one yk_distill_loss_f32 call per output layer (csrc/yk_distill.hip) into that layer's gradient between the detection loss and the backward
pass, inside the capture.  The validation loss stays the detection loss.  With distill=None nothing is allocated and nothing is launched.

Weight EMA, learning-rate schedule and gradient clipping (optim.py): `Trainer(ema=EmaConfig(...), clip_norm=..., lr_schedule=
LrSchedule(...))` replace the update's one yk_adam_f32 launch by yk_sumsq_f32 (clipping only) and one yk_adam_ex_f32 launch (csrc/yk_optim.hip),
outside the captured graph like Adam; the average E of P and the average of the BatchNorm moving statistics are what `export_weights(ema=True)`
returns.  With the defaults nothing is allocated and apply_update issues yk_adam_f32 as before.

fp32 storage and fp32 MFMA throughout (TF1.14's default for this model)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import engine
from . import netspec as ns

L2_WEIGHT = 5e-4                 # keras.regularizers.l2(5e-4), yolonet.py:247
BN_MOMENTUM = 0.99               # keras BatchNormalization default (v1 backbone, every DarknetConv2D_BN_Leaky)
BN_MOMENTUM_V2 = 0.999           # MobileNetV2 backbone, keras_mobilenet_v2.py:320


def _is_darknet_conv(name: str) -> bool:
    """Layers built by DarknetConv2D (yolonet.py:245) carry the l2 regulariser; the MobileNet backbones do not."""
    return name.startswith('head_conv') or name.startswith('conv2d_')


def conv_route(op: dict, layer: ns.Layer) -> str:
    """How the training step computes a Conv2D op of the NetSpec; forward and backward take the same route:
      'gemm'      1x1 stride 1: GEMMs on the activations themselves;
      'implicit'  3x3 as implicit GEMMs, no column matrix (yk_conv3x3_*; a strided data gradient still goes through a column matrix
                  folded by yk_col2im3x3_f32).  Needs Cin % 4 == 0 and Cout % 4 == 0, and BatchNorm: the step calls the forward kernel
                  fused with it;
      'im2col'    3x3 through a column matrix (yk_im2col3x3_f32 + GEMM; yk_col2im3x3_f32): every other 3x3 conv - in the networks
                  netspec builds, only the 3-channel stem."""
    if op['k'] == 1 and op['stride'] == 1:
        return 'gemm'
    assert op['k'] == 3, op
    return 'implicit' if op['cin'] % 4 == 0 and op['cout'] % 4 == 0 and layer.bn_name else 'im2col'


class Trainer:
    def __init__(self, spec: ns.NetSpec, weights: Dict[str, np.ndarray], anchors: np.ndarray, per_rank_batch: int,
                 obj_thresh: float = 0.7, iou_thresh: float = 0.5, obj_weight: float = 1.0, noobj_weight: float = 1.0,
                 wh_weight: float = 1.0, lr: float = 5e-4, decay: float = 0.0, device: int = 0, process_group=None,
                 world_size: int = 1, use_graph: bool = True, prune=None, qat=None, box_loss: str = 'mse', box_weight: float = 1.0,
                 distill=None, ema=None, clip_norm: float = 0.0, lr_schedule=None, focal: str = 'off', focal_gamma: float = 2.0,
                 focal_alpha: float = 0.0, label_smooth: float = 0.0, obj_target: str = 'label'):
        import torch
        from . import lossopt
        loss_opts = lossopt.validate(focal, focal_gamma, focal_alpha, label_smooth, obj_target)
        if box_loss not in engine.BOX_LOSSES:
            raise ValueError(f'box_loss {box_loss!r}: choose one of ' + ', '.join(repr(k) for k in engine.BOX_LOSSES))
        if ema is not None and qat is not None:
            raise engine.YkError('ema= together with qat= is not supported: the learned activation ranges belong to the live weights, not to '
                                 'their average')
        if lr_schedule is not None and float(decay) != 0.0:
            raise engine.YkError(f'lr_schedule= together with decay={decay} would be two learning-rate schedules: pass decay=0')
        if not float(clip_norm) >= 0.0:
            raise engine.YkError(f'clip_norm {clip_norm} must not be negative (0 is off)')
        engine.require_gpu()
        self.torch = torch
        self.spec, self.B = spec, int(per_rank_batch)
        self.dev = torch.device('cuda', device)
        self.anchors = np.asarray(anchors, np.float32)
        self.hyper = dict(obj_thresh=obj_thresh, iou_thresh=iou_thresh, obj_weight=obj_weight, noobj_weight=noobj_weight,
                          wh_weight=wh_weight, box_loss=box_loss, box_weight=box_weight, **loss_opts)
        self.lr, self.decay, self.iterations = float(lr), float(decay), 0
        self.pg, self.world = process_group, int(world_size)
        self.lay = {l.name: l for l in spec.layers}

        # ---- flat parameter / gradient / Adam buffers; conv kernels as [Cout][kh*kw*Cin], depthwise as [9][C]
        self.slots: Dict[str, tuple] = {}
        off = 0
        for l in spec.layers:
            kh, kw, ci, co = l.kernel_shape
            shape = (co, kh * kw * ci) if l.kind == 'conv' else (9, ci)
            items = [(l.name + '/kernel', shape)]
            if l.use_bias:
                items.append((l.name + '/bias', (co,)))
            if l.bn_name:
                c = co if l.kind == 'conv' else ci
                items += [(l.bn_name + '/gamma', (c,)), (l.bn_name + '/beta', (c,))]
            for nm, shp in items:
                n = int(np.prod(shp))
                self.slots[nm] = (off, shp)
                off += (n + 7) // 8 * 8
        self.n_params = off
        self.P = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.G = torch.zeros_like(self.P)
        self.m = torch.zeros_like(self.P)
        self.v = torch.zeros_like(self.P)
        # BatchNorm moving statistics: views of one flat buffer, padded like the parameter slots, so that one launch can cover them all.
        # The tensors of self.moving are never rebound: a captured step holds their pointers
        self.mslots: Dict[str, tuple] = {}
        off = 0
        for l in spec.layers:
            if l.bn_name:
                c = l.kernel_shape[3] if l.kind == 'conv' else l.kernel_shape[2]
                for s in ('/moving_mean', '/moving_variance'):
                    self.mslots[l.bn_name + s] = (off, c)
                    off += (c + 7) // 8 * 8
        self.M = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.moving: Dict[str, "torch.Tensor"] = {nm: self.M[o:o + c] for nm, (o, c) in self.mslots.items()}
        # the optional parts of the update (optim.py).  None / 0: nothing is allocated and nothing is launched.
        self.ema, self.clip_norm, self.lr_schedule = ema, float(clip_norm), lr_schedule
        self.E = self.EM = None
        self.ema_updates = 0
        self.load_weights(weights)
        if ema is not None:                                          # the average of the weights and of the moving statistics
            self.E, self.EM = self.P.clone(), self.M.clone()
            self.ema_moving = {nm: self.EM[o:o + c] for nm, (o, c) in self.mslots.items()}
        if self.clip_norm:
            nbytes = C.c_size_t()
            engine.call('yk_sumsq_workspace_bytes', self.n_params, C.byref(nbytes))
            self._sq_work = torch.zeros(nbytes.value // 8, dtype=torch.float64, device=self.dev)
            self._sumsq = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self.counts = [torch.zeros(3, dtype=torch.float32, device=self.dev) for _ in spec.outputs]
        self.saved: Dict[int, dict] = {}
        self.T: Dict[int, "torch.Tensor"] = {}
        # forward + loss + backward is ~800 launches whose arguments never change from step to step: after one eager step it is
        # captured as a HIP graph and replayed (same kernels, same order, same buffers -> bitwise the same results; measured 7.8 ->
        # 6.7 ms per step for yolo_mobilev2-1.0 at 16 images).  Adam stays outside: its step counter is a launch argument.
        self.use_graph = bool(use_graph)
        self._l2_seg = None
        self._fa = None
        self._graph = None
        self._gx = self._gy = self._gres = self._side = None
        self._eager_steps = 0
        self._captured_key = None
        # magnitude pruning (prune.PruneSchedule; keras_train.py:59-71).  None: nothing is allocated and nothing is launched.
        self.prune = prune
        if prune is not None:
            self._prune_init()
        # quantisation-aware training (qat.QatConfig).  None: nothing is allocated and nothing is launched.
        self.qat = qat
        if qat is not None:
            self._qat_init()
        # knowledge distillation (distill.DistillConfig).  None: nothing is allocated and nothing is launched.
        self.distill = distill
        if distill is not None:
            self._distill_init(device)

    # ------------------------------------------------------------------ parameters
    def view(self, buf, name):
        off, shp = self.slots[name]
        return buf[off:off + int(np.prod(shp))].view(*shp)

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        torch = self.torch
        for l in self.spec.layers:
            k = np.asarray(weights[l.name + '/kernel'], np.float32)
            if l.kind == 'conv':
                k = np.transpose(k, (3, 0, 1, 2)).reshape(l.kernel_shape[3], -1)          # HWIO -> O,(HWI)
            else:
                k = k[..., 0].reshape(9, -1)
            self.view(self.P, l.name + '/kernel').copy_(torch.from_numpy(np.ascontiguousarray(k)))
            if l.use_bias:
                self.view(self.P, l.name + '/bias').copy_(torch.from_numpy(np.asarray(weights[l.name + '/bias'], np.float32)))
            if l.bn_name:
                for s in ('/gamma', '/beta'):
                    self.view(self.P, l.bn_name + s).copy_(torch.from_numpy(np.asarray(weights[l.bn_name + s], np.float32)))
                for s in ('/moving_mean', '/moving_variance'):
                    # IN PLACE: a captured step holds the raw pointer of this tensor (yk_bn_train_fwd updates the moving statistics
                    # inside the replayed graph); rebinding the name would leave the graph writing a freed buffer while
                    # export_weights / validate read a tensor nobody updates
                    self.moving[l.bn_name + s].copy_(torch.from_numpy(np.asarray(weights[l.bn_name + s], np.float32).copy()))
        if self.E is not None:                                       # the average starts again from what was loaded
            self.E.copy_(self.P)
            self.EM.copy_(self.M)

    def export_weights(self, quantized: bool = False, ema: bool = False) -> Dict[str, np.ndarray]:
        """Keras-layout arrays again (what keras.models.save_model would hold, keras_train.py:107).  quantized=True (a QAT Trainer): the
        kernels as the step reads them, fq of the current P over each kernel's own range; everything else as in P.  ema=True (a Trainer
        with ema=): the averaged weights and the averaged BatchNorm moving statistics, same keys and shapes."""
        out = {}
        if ema and self.E is None:
            raise engine.YkError('this Trainer was built without a weight average (ema=None)')
        par, moving = (self.E, self.ema_moving) if ema else (self.P, self.moving)
        src = par
        if quantized:
            self._need_qat()
            self._qat_weights()
            src = self.Pq
        for l in self.spec.layers:
            kh, kw, ci, co = l.kernel_shape
            k = self.view(src, l.name + '/kernel').cpu().numpy()
            out[l.name + '/kernel'] = (np.transpose(k.reshape(co, kh, kw, ci), (1, 2, 3, 0)) if l.kind == 'conv'
                                       else k.reshape(3, 3, ci)[..., None]).copy()
            if l.use_bias:
                out[l.name + '/bias'] = self.view(par, l.name + '/bias').cpu().numpy().copy()
            if l.bn_name:
                for s in ('/gamma', '/beta'):
                    out[l.bn_name + s] = self.view(par, l.bn_name + s).cpu().numpy().copy()
                for s in ('/moving_mean', '/moving_variance'):
                    out[l.bn_name + s] = moving[l.bn_name + s].cpu().numpy().copy()
        return out

    def grads(self) -> Dict[str, np.ndarray]:
        """Gradients of the last step in Keras layout (for parity tests)."""
        out = {}
        for nm, (off, shp) in self.slots.items():
            g = self.G[off:off + int(np.prod(shp))].view(*shp).cpu().numpy()
            if nm.endswith('/kernel'):
                l = self.lay[nm[:-7]]
                kh, kw, ci, co = l.kernel_shape
                g = np.transpose(g.reshape(co, kh, kw, ci), (1, 2, 3, 0)) if l.kind == 'conv' else g.reshape(3, 3, ci)[..., None]
            out[nm] = g.copy()
        return out

    # ------------------------------------------------------------------ kernel calls
    def _ck(self, name, *args):
        """engine.call of a library function whose last parameter is the stream: torch's current one."""
        engine.call(name, *args, self.torch.cuda.current_stream().cuda_stream)

    def _new(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float32, device=self.dev)

    def gemm(self, tA, tB, M, N, K, A, lda, Bm, ldb, Cm, ldc, alpha=1.0, beta=0.0):
        self._ck('yk_gemm_f32', tA, tB, M, N, K, alpha, A, lda, Bm, ldb, beta, Cm, ldc)

    def _geom(self, op):
        hi, wi, ci = self.spec.tensors[op['in0']]
        ho, wo, _ = self.spec.tensors[op['out']]
        return [self.B, hi, wi, ci, ho, wo, op['stride'], op['pad_t'], op['pad_l']]

    def _axpy(self, a, x, y):
        self._ck('yk_axpy_f32', x.numel(), a, x, y)

    def _fused_adds(self):
        """conv op index -> (index of the Add that consumes ONLY-there its output, the Add's other input).  The Add is folded into that
        conv's BatchNorm apply pass when the conv has BatchNorm, its output has no other reader and is not a network output, and the Add
        follows before anything else needs the output (residual blocks: keras_mobilenet_v2.py:483-484, yolonet.py:194-204)."""
        if self._fa is None:
            ops, fa = self.spec.ops, {}
            readers = {}
            for k, o in enumerate(ops):
                for key in ('in0', 'in1'):
                    if o.get(key, -1) is not None and o.get(key, -1) >= 0:
                        readers.setdefault(o[key], []).append(k)
            for k, o in enumerate(ops):
                if o['type'] != ns.OP_ADD:
                    continue
                for mine, other in ((o['in1'], o['in0']), (o['in0'], o['in1'])):
                    prod = [j for j, q in enumerate(ops) if q['out'] == mine and q['type'] in (ns.OP_CONV, ns.OP_DWCONV)]
                    if (len(prod) == 1 and self.lay[ops[prod[0]]['layer']].bn_name and readers.get(mine, []) == [k] and mine not in self.spec.outputs
                            and mine != other and all(q['out'] != other for q in ops[prod[0]:k])):
                        fa[prod[0]] = (k, other)
                        break
            self._fa = fa
        return self._fa

    # ------------------------------------------------------------------ forward (training mode)
    def forward(self, x_nhwc, observe: bool = False) -> List["torch.Tensor"]:
        """x_nhwc: cuda fp32 [B,H,W,3] already normalised (Helper._process_img output).  Saves the tape.
        A QAT Trainer reads the kernels from Pq and fake-quantises every conv output and concat (the unquantised tensor stays on the tape as
        saved[i]['qy']); observe=True quantises nothing and only folds the batch extremes (qat_observe)."""
        torch = self.torch
        assert x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and tuple(x_nhwc.shape[:1]) == (self.B,)
        T, S = {0: x_nhwc.contiguous()}, {}
        fq = self.qat is not None and not observe
        if fq:
            self._qat_weights()                                      # Pq = fq(P): the first launches of the captured region
        W = self.Pq if fq else self.P
        fused_add = self._fused_adds()                               # conv op index -> (Add op index, the Add's other input)
        done = set()
        for i, op in enumerate(self.spec.ops):
            if i in done:
                continue
            x, t = T[op['in0']], op['type']
            ho, wo, co = self.spec.tensors[op['out']]
            M = self.B * ho * wo
            if t in (ns.OP_CONV, ns.OP_DWCONV):
                l = self.lay[op['layer']]
                w = self.view(W, l.name + '/kernel')
                z = self._new(self.B, ho, wo, co)
                route = conv_route(op, l) if t == ns.OP_CONV else None
                a, kk = x, op['cin']                                 # the GEMM's operand: a 1x1 conv's input, or the column matrix below
                if route == 'im2col':
                    a, kk = self._new(M, 9 * op['cin']), 9 * op['cin']
                    self._ck('yk_im2col3x3_f32', x, *self._geom(op), a)
                if l.bn_name:
                    # convolution + batch statistics + apply in one library call: the producer of z leaves the partial sums of the
                    # statistics (yk_gemm_bn_fwd_f32 / yk_dw3x3_bn_fwd_f32), z is not read a second time for them
                    y = self._new(self.B, ho, wo, co)
                    mean, invstd = self._new(co), self._new(co)
                    fa = fused_add.get(i)
                    res = T[fa[1]] if fa is not None else None       # keras Add()([res, this output]) folded into the apply pass
                    bn = (z, self.view(self.P, l.bn_name + '/gamma'), self.view(self.P, l.bn_name + '/beta'), ns.BN_EPS, op['act'], op['alpha'],
                          y, mean, invstd, self.moving[l.bn_name + '/moving_mean'], self.moving[l.bn_name + '/moving_variance'],
                          BN_MOMENTUM_V2 if self.spec.name == 'yolo_mobilev2' and not _is_darknet_conv(l.name) else BN_MOMENTUM, res)
                    if route == 'implicit':
                        self._ck('yk_conv3x3_bn_fwd_f32', x, w, *self._geom(op), co, *bn)
                    elif t == ns.OP_CONV:
                        self._ck('yk_gemm_bn_fwd_f32', M, co, kk, a, kk, w, kk, *bn)           # Z = X * W^T
                    else:
                        self._ck('yk_dw3x3_bn_fwd_f32', x, w, *self._geom(op), *bn)
                    S[i] = dict(z=z, mean=mean, invstd=invstd)
                    if fa is not None:                               # y IS the Add's output; the conv's own output tensor is never needed again
                        T[self.spec.ops[fa[0]]['out']] = y
                        done.add(fa[0])
                else:
                    assert op['act'] == ns.ACT_NONE
                    if t == ns.OP_CONV:
                        self.gemm(0, 1, M, co, kk, a, kk, w, kk, z, co)                  # Z = X * W^T
                    else:
                        self._ck('yk_dw3x3_fwd_f32', x, w, *self._geom(op), z)
                    if l.use_bias:
                        self._ck('yk_bias_add_f32', z, M, co, self.view(self.P, l.name + '/bias'))
                    y = z
                if self.qat is not None:
                    y = self._qat_out(i, op['out'], y, S, observe)
            elif t == ns.OP_MAXPOOL:
                hi, wi, ci = self.spec.tensors[op['in0']]
                y = self._new(self.B, ho, wo, co)
                arg = torch.empty((self.B, ho, wo, co), dtype=torch.uint8, device=self.dev)
                self._ck('yk_maxpool2_fwd_f32', x, self.B, hi, wi, ci, ho, wo, op['stride'], y, arg)
                S[i] = dict(arg=arg)
            elif t == ns.OP_UPSAMPLE:                                                   # nearest x2: pure data movement
                y = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
            elif t == ns.OP_CONCAT:
                y = torch.cat([x, T[op['in1']]], dim=3)
                if fq:                                               # the kmodel's REQUANTIZE onto the union of the parts' ranges
                    y = self._qat_out(i, op['out'], y, S, False)
            elif t == ns.OP_ADD:
                y = x.clone()
                self._axpy(1.0, T[op['in1']], y)
            else:
                raise engine.YkError(f'op type {t} not trainable')
            T[op['out']] = y
        self.T, self.saved = T, S
        e = 5 + self.spec.class_num
        return [T[o].view(self.B, *self.spec.tensors[o][:2], self.spec.anchor_num, e) for o in self.spec.outputs]

    # ------------------------------------------------------------------ backward
    def backward(self, out_grads: Sequence["torch.Tensor"]) -> None:
        """out_grads[i] = dL/d(output i).  Fills self.G (kernel/bias/gamma/beta gradients; regulariser added by step())."""
        self.G.zero_()
        D: Dict[int, "torch.Tensor"] = {}
        # The weight gradients of the 1x1 and depthwise convs depend on nothing the backward chain waits for: they are collected during
        # the walk and issued as grouped launches at its end, whose tiles fill the chip together (35 GEMMs + 35 slice-adding launches
        # become 2, the 17 + 17 depthwise launches 2 more).  yk_gemm_f32_grouped sizes its K slices for the group: equal to per-layer
        # yk_gemm_f32 calls within fp32 summation order, and reproducible from run to run.  yk_dw3x3_bwd_weight_grouped_f32 computes
        # every problem as yk_dw3x3_bwd_weight_f32 does.
        grouped = []                                                # (dz, x, gw, co, ci, M) of the 1x1 convs
        grouped_dw = []                                             # (x, dz, gw, geometry) of the depthwise convs

        def acc(tid, g, own):
            if tid == 0:
                return
            if tid not in D:
                D[tid] = g if own else g.clone()
            else:
                self._axpy(1.0, g, D[tid])

        for o, g in zip(self.spec.outputs, out_grads):
            acc(o, g.reshape(self.B, *self.spec.tensors[o]).contiguous(), False)
        for i in range(len(self.spec.ops) - 1, -1, -1):
            op = self.spec.ops[i]
            t = op['type']
            dy = D.pop(op['out'], None)
            if dy is None:
                continue
            if self.qat is not None and 'qy' in self.saved.get(i, ()):
                # straight-through: dy is the gradient of the fake-quantised output and nobody else holds it, masked in place
                self._ck('yk_qat_act_bwd_f32', dy, self.saved[i]['qy'], dy.numel(), self._qa_ranges, op['out'], dy)
            x = self.T.get(op['in0'])                               # (None for an Add whose conv input was folded into the producer: never stored, never read here)
            ho, wo, co = self.spec.tensors[op['out']]
            hi, wi, ci = self.spec.tensors[op['in0']]
            M = self.B * ho * wo
            if t in (ns.OP_CONV, ns.OP_DWCONV):
                l = self.lay[op['layer']]
                w = self.view(self.P if self.qat is None else self.Pq, l.name + '/kernel')     # dL/dPq is taken as dL/dP
                gw = self.view(self.G, l.name + '/kernel')
                if l.bn_name:
                    sv = self.saved[i]
                    dz = self._new(self.B, ho, wo, co)
                    self._ck('yk_bn_train_bwd_f32', sv['z'], dy, M, co, self.view(self.P, l.bn_name + '/gamma'), self.view(self.P, l.bn_name + '/beta'),
                             sv['mean'], sv['invstd'], op['act'], op['alpha'], dz, self.view(self.G, l.bn_name + '/gamma'),
                             self.view(self.G, l.bn_name + '/beta'))
                else:
                    dz = dy
                    if l.use_bias:
                        self._ck('yk_colsum_f32', dz, M, co, self.view(self.G, l.name + '/bias'))
                need_dx = op['in0'] != 0
                if t == ns.OP_CONV:
                    route = conv_route(op, l)
                    if route == 'gemm':
                        grouped.append((dz, x, gw, co, ci, M))                           # dW = dZ^T * X, with all the others below
                        if need_dx:
                            if op['in0'] in D:                                          # a second reader of the input: dX += dZ * W straight into the
                                self.gemm(0, 0, M, ci, co, dz, co, w, ci, D[op['in0']], ci, beta=1.0)   # accumulated gradient (no temporary, no axpy)
                            else:
                                dx = self._new(self.B, hi, wi, ci)
                                self.gemm(0, 0, M, ci, co, dz, co, w, ci, dx, ci)       # dX = dZ * W
                                acc(op['in0'], dx, True)
                    elif route == 'implicit':
                        geom = self._geom(op)
                        self._ck('yk_conv3x3_bwd_weight_f32', x, dz, *geom, co, gw)
                        if need_dx:
                            dx = self._new(self.B, hi, wi, ci)
                            if op['stride'] == 1:
                                self._ck('yk_conv3x3_bwd_data_f32', dz, w, *geom, co, dx)
                            else:                                           # strided: column matrix of gradients, folded by col2im
                                kk = 9 * ci
                                col = self._new(M, kk)
                                self.gemm(0, 0, M, kk, co, dz, co, w, kk, col, kk)
                                self._ck('yk_col2im3x3_f32', col, *geom, dx)
                                del col
                            acc(op['in0'], dx, True)
                    else:
                        kk = 9 * ci
                        col = self._new(M, kk)
                        self._ck('yk_im2col3x3_f32', x, *self._geom(op), col)
                        self.gemm(1, 0, co, kk, M, dz, co, col, kk, gw, kk)
                        if need_dx:
                            self.gemm(0, 0, M, kk, co, dz, co, w, kk, col, kk)          # dcol (reuses the buffer)
                            dx = self._new(self.B, hi, wi, ci)
                            self._ck('yk_col2im3x3_f32', col, *self._geom(op), dx)
                            acc(op['in0'], dx, True)
                        del col
                else:
                    grouped_dw.append((x, dz, gw, self._geom(op)))
                    if need_dx:
                        dx = self._new(self.B, hi, wi, ci)
                        self._ck('yk_dw3x3_bwd_data_f32', dz, w, *self._geom(op), dx)
                        acc(op['in0'], dx, True)
            elif t == ns.OP_MAXPOOL:
                dx = self._new(self.B, hi, wi, ci)
                self._ck('yk_maxpool2_bwd_f32', dy, self.saved[i]['arg'], self.B, hi, wi, ci, ho, wo, op['stride'], dx)
                acc(op['in0'], dx, True)
            elif t == ns.OP_UPSAMPLE:
                dx = self._new(self.B, hi, wi, ci)
                self._ck('yk_upsample2x_bwd_f32', dy, self.B, hi, wi, ci, dx)
                acc(op['in0'], dx, True)
            elif t == ns.OP_CONCAT:
                c0 = self.spec.tensors[op['in0']][2]
                acc(op['in0'], dy[..., :c0].contiguous(), True)
                acc(op['in1'], dy[..., c0:].contiguous(), True)
            elif t == ns.OP_ADD:
                # dL/d(in0) = dL/d(in1) = dy.  The two entries may SHARE dy's buffer (no clone) when nothing accumulates into either of them
                # before the other one has been consumed: every other reader of one input precedes the producer of the other input, i.e.
                # the backward loop pops the producer's entry first (the residual blocks of both networks)
                a_, b_ = op['in0'], op['in1']
                pa = max([j for j, q in enumerate(self.spec.ops) if q['out'] == a_], default=-1)
                pb = max([j for j, q in enumerate(self.spec.ops) if q['out'] == b_], default=-1)
                first, second = (a_, b_) if pa > pb else (b_, a_)     # `first` is popped first (its producer comes later in the forward order)
                pf = max(pa, pb)
                others = [j for j, q in enumerate(self.spec.ops) if j != i and (q.get('in0') == second or q.get('in1') == second)]
                lone = not [j for j, q in enumerate(self.spec.ops) if j != i and (q.get('in0') == first or q.get('in1') == first)] and first not in self.spec.outputs
                # ... and `first`'s producer must be a conv WITH BatchNorm: its backward only READS dy and writes a fresh dz.  Another Add would store
                # dy again by reference; a conv without BN hands dy on as its dz, and a 1x1 conv's dz is read again by the grouped weight-gradient
                # launch at the end of backward() - then a later accumulation into D[second] would corrupt a buffer somebody else still holds: clone.
                pq = self.spec.ops[pf] if pf >= 0 else None
                fresh = pq is not None and pq['type'] in (ns.OP_CONV, ns.OP_DWCONV) and bool(self.lay[pq['layer']].bn_name)
                share = a_ != b_ and lone and fresh and first not in D and second not in D and all(j < pf for j in others) and second != 0
                acc(second, dy, share)
                acc(first, dy, True)
        if grouped:
            n = len(grouped)
            ia = lambda v: (C.c_int * n)(*v)
            pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
            self._ck('yk_gemm_f32_grouped', n, 1, 0, ia([g[3] for g in grouped]), ia([g[4] for g in grouped]), ia([g[5] for g in grouped]), 1.0,
                     pa([g[0] for g in grouped]), ia([g[3] for g in grouped]), pa([g[1] for g in grouped]), ia([g[4] for g in grouped]), 0.0,
                     pa([g[2] for g in grouped]), ia([g[4] for g in grouped]))
        if grouped_dw:
            n = len(grouped_dw)
            pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
            geo = (C.c_int * (9 * n))(*[v for g in grouped_dw for v in g[3]])
            self._ck('yk_dw3x3_bwd_weight_grouped_f32', n, pa([g[0] for g in grouped_dw]), pa([g[1] for g in grouped_dw]), geo,
                     pa([g[2] for g in grouped_dw]))

    # ------------------------------------------------------------------ one optimisation step
    def regulariser(self, add_grad: bool) -> "torch.Tensor":
        """sum over DarknetConv2D kernels of 5e-4 * sum(w^2) (device scalar); optionally G += 2*5e-4*W.
        One pass over all of those kernels (yk_l2_segments_f32: they are segments of the flat parameter buffer) - two launches instead of
        a dot product and an axpy per layer."""
        torch = self.torch
        if self._l2_seg is None:
            segs = [(self.slots[l.name + '/kernel'][0], int(np.prod(self.slots[l.name + '/kernel'][1])))
                    for l in self.spec.layers if l.kind == 'conv' and _is_darknet_conv(l.name)]
            pre = np.concatenate([[0], np.cumsum([n for _, n in segs])]).astype(np.int64)
            self._l2_seg = (torch.from_numpy(pre).to(self.dev), torch.from_numpy(np.asarray([o for o, _ in segs], np.int64)).to(self.dev), len(segs),
                            int(pre[-1]))
        pre, off, nseg, total = self._l2_seg
        tot = torch.zeros(1, dtype=torch.float32, device=self.dev)
        if nseg:
            self._ck('yk_l2_segments_f32', self.P, self.G, pre, off, nseg, total, L2_WEIGHT, 1, int(add_grad), tot)
        return tot

    def loss_and_grads(self, x_nhwc, y_true: Sequence["torch.Tensor"]):
        """forward + loss + backward (no all-reduce, no update).  -> dict of device scalars."""
        global_batch = self.B * self.world
        preds = self.forward(x_nhwc)
        parts, grads = [], []
        for li, (yp, yt) in enumerate(zip(preds, y_true)):
            loss6, g, _ = engine.yolo_loss(yt, yp.contiguous(), self.anchors[li], batch_size=global_batch, counts=self.counts[li],
                                           **self.hyper)
            parts.append(loss6)
            grads.append(g)
        kd = None
        if self.distill is not None:                                 # g += dL_distill/dy_pred, the teacher's outputs of THIS batch in self._tq
            kd = [engine.distill_loss(tq, yp.contiguous(), self.distill_weight, global_batch, grad=g)
                  for tq, yp, g in zip(self._tq, preds, grads)]
        self.backward(grads)
        res = dict(layers=parts, reg=self.regulariser(add_grad=self.world == 1))
        if kd is not None:
            res['distill'] = kd
        if self.qat is not None:
            self._qat_update(False)                                  # after the backward pass: forward and backward saw the same ranges
        return res

    def invalidate_graph(self) -> None:
        """Forget the captured step (the next two steps run eagerly / re-capture).  Called automatically when something a capture
        bakes in as a launch scalar or a shape changes: `tr.hyper[...]`, the batch shape.  Parameters, Adam state and BatchNorm moving
        statistics live in buffers that are only ever written in place, so loading weights does not need it."""
        self._graph = None
        self._gres = self._gx = self._gy = None
        self._eager_steps = 0

    def _graph_key(self, x_nhwc, y_true):
        return (tuple(sorted(self.hyper.items())), tuple(x_nhwc.shape), tuple(tuple(y.shape) for y in y_true), self.world,
                None if self.qat is None else self.qat.momentum,           # (a launch scalar of yk_qat_update_f32 inside the capture)
                None if self.distill is None else self.distill_weight)      # (a launch scalar of yk_distill_loss_f32 inside the capture)

    def _loss_and_grads_replayed(self, x_nhwc, y_true):
        """loss_and_grads through a captured HIP graph (after one eager step that also warms allocator and scratch buffers).
        One Trainer per stream: the library's split-K workspace is keyed by the stream handle and is part of the capture."""
        torch = self.torch
        if not self.use_graph:
            return self.loss_and_grads(x_nhwc, y_true)
        key = self._graph_key(x_nhwc, y_true)
        if self._graph is not None and key != self._captured_key:
            self.invalidate_graph()                                # loss weights / thresholds / shapes are launch arguments of the capture
        if self._graph is None:
            # both the eager first step and the capture run on one dedicated stream: the library's scratch buffers are keyed by
            # stream and must already have their final size when the capture starts (an allocation would invalidate it)
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.dev)
            side, cur = self._side, torch.cuda.current_stream()
            side.wait_stream(cur)
            if self._eager_steps < 1:
                self._eager_steps += 1
                with torch.cuda.stream(side):
                    r = self.loss_and_grads(x_nhwc, y_true)
                cur.wait_stream(side)
                return r
            self._gx = x_nhwc.clone()
            self._gy = [y.clone() for y in y_true]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                g = torch.cuda.CUDAGraph()
                # thread_local: the input pipeline's producer thread allocates pinned / device buffers and copies while this thread
                # captures; in the default (global) mode any such call from another thread invalidates the capture
                with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
                    self._gres = self.loss_and_grads(self._gx, self._gy)
            cur.wait_stream(side)
            self._graph = g
            self._captured_key = key
            # the capture itself does not execute: fall through to a replay with the current batch
        self._gx.copy_(x_nhwc)
        for d, s_ in zip(self._gy, y_true):
            d.copy_(s_)
        self._graph.replay()
        return self._gres

    def exchange(self, reduce=None) -> None:
        """The data-parallel exchange of one step: SUM the flat gradient bucket over the ranks, then add the regulariser's gradient
        (identical on every rank) once.  `reduce(flat_grad)` replaces the all-reduce — tests drive several replicas of one process
        through exactly this code with it."""
        import torch.distributed as dist
        from .shard import allreduce_gradients
        # data-term gradients already carry 1/global_batch, so SUM over ranks is the global-batch gradient
        if reduce is not None:
            reduce(self.G)
        else:
            if not dist.is_initialized():
                raise engine.YkError(f'Trainer(world_size={self.world}) needs an initialised torch.distributed process group')
            allreduce_gradients(self.G, dist, self.pg)
        self.regulariser(add_grad=True)

    def apply_update(self) -> None:
        """keras Adam(lr, decay) on the flat buffers (keras_train.py:73-76); one launch.
        With ema=, clip_norm= or lr_schedule= (optim.py): the learning rate of this iteration from the schedule, the sum of squares of G as
        the update consumes it (after exchange() and the regulariser's gradient: the same on every rank), then one yk_adam_ex_f32 launch
        that clips, updates and averages in a single pass over the flat buffers, and one yk_ema_f32 over the BatchNorm moving statistics."""
        if self.ema is None and not self.clip_norm and self.lr_schedule is None:
            self._ck('yk_adam_f32', self.n_params, self.P, self.G, self.m, self.v, self.lr, self.decay, self.iterations, 0.9, 0.999, 1e-7, 1.0)
            self.iterations += 1
            return
        self.last_lr = lr = self.lr if self.lr_schedule is None else self.lr_schedule.lr_at(self.iterations)
        sumsq = None
        if self.clip_norm:
            self._ck('yk_sumsq_f32', self.G, self.n_params, self._sq_work, self._sumsq)
            sumsq = self._sumsq
        omd = 0.0
        if self.ema is not None:
            self.ema_updates += 1
            omd = self.ema.omd_at(self.ema_updates)
        self._ck('yk_adam_ex_f32', self.n_params, self.P, self.G, self.m, self.v, self.E, sumsq, lr, self.decay, self.iterations, 0.9, 0.999, 1e-7,
                 1.0, self.clip_norm, omd)
        if self.ema is not None and self.M.numel():
            self._ck('yk_ema_f32', self.M.numel(), self.M, self.EM, omd)
        self.iterations += 1

    # ------------------------------------------------------------------ knowledge distillation
    def _distill_init(self, device: int) -> None:
        """The teacher's inference plan and one static buffer per output layer for its raw outputs.  Allocated once: the captured step holds
        the buffers' pointers, every step refills them in place (the way _gx and _gy travel)."""
        from .distill import check_teacher
        d = self.distill
        check_teacher(self.spec, d.spec, self.anchors)               # YkError naming the first difference
        self.distill_weight = float(d.weight)
        # 'throughput': one launch per layer.  The cluster launches of 'latency' need their workgroups co-resident, which the input
        # pipeline's kernels on other streams can prevent, and report that through a flag the step would have to wait for
        self._teacher = engine.Plan(d.spec, d.weights, max_batch=self.B, device=device, precision=d.precision, schedule='throughput')
        e = 5 + self.spec.class_num
        self._tq = [self._new(self.B, *self.spec.tensors[o][:2], self.spec.anchor_num, e) for o in self.spec.outputs]

    def _need_distill(self):
        if self.distill is None:
            raise engine.YkError('this Trainer was built without a teacher (distill=None)')

    def teacher_forward(self, x_nhwc) -> List["torch.Tensor"]:
        """The teacher's raw outputs of these frames, [B,h,w,A,5+C] per layer, into the static buffers the step's distillation calls read.
        Runs on torch's current stream, outside the captured graph."""
        self._need_distill()
        assert tuple(x_nhwc.shape[:1]) == (self.B,)
        self._teacher.run_f32(x_nhwc.contiguous())
        for dst, o in zip(self._tq, self._teacher.outputs()):
            dst.view(self.B, -1).copy_(o[:self.B].reshape(self.B, -1))
        return self._tq

    # ------------------------------------------------------------------ magnitude pruning
    def _prune_init(self) -> None:
        """Segment tables of the prunable kernels in the flat buffer, the flat uint8 mask (1 everywhere outside them) and the outputs."""
        from .prune import prunable_layers
        torch = self.torch
        self._pr_names = [n + '/kernel' for n in prunable_layers(self.spec)]
        offs = [self.slots[n][0] for n in self._pr_names]
        self._pr_sizes = [int(np.prod(self.slots[n][1])) for n in self._pr_names]
        if not self._pr_names:
            raise engine.YkError('pruning: the network has no Conv2D kernel')
        self.prune.check(self._pr_sizes)
        tile = engine.lib().yk_prune_tile()                                      # YK_PRUNE_TILE of the loaded library
        first = np.concatenate([[0], np.cumsum([(n + tile - 1) // tile for n in self._pr_sizes])])
        assert all(o >= 0 and o + n <= self.n_params for o, n in zip(offs, self._pr_sizes)) and first[-1] < 2 ** 31
        dev = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(self.dev)
        self._pr_off, self._pr_size, self._pr_first = dev(offs, np.int64), dev(self._pr_sizes, np.int64), dev(first, np.int32)
        self._pr_ntiles = int(first[-1])
        self._pr_keep = dev(self._pr_sizes, np.int64)
        self._pr_keep_host = torch.zeros(len(offs), dtype=torch.int64).pin_memory()      # staging of the counts: the copy does not block the host
        self._pr_keep_sent = None
        self._pr_mask = torch.ones(self.n_params, dtype=torch.uint8, device=self.dev)
        self._pr_thr = torch.zeros(len(offs), dtype=torch.float32, device=self.dev)     # before the first update every mask is all ones
        self._pr_kept = dev(self._pr_sizes, np.int64)

    def _need_prune(self):
        if self.prune is None:
            raise engine.YkError('this Trainer was built without a pruning schedule (prune=None)')

    def update_masks(self, s: Optional[int] = None) -> None:
        """Masks of step s (default: the current iteration) from the CURRENT weights: per kernel the k-th largest |w| and |w| >= it.
        One library call for all kernels; the mask, the thresholds and the kept counts are written in place.
        The copy of the keep counts and the kernels that read them are ordered by torch's CURRENT stream: call it (and step()) under the same
        current stream for the whole life of the Trainer - the rule the captured step already sets (one Trainer per stream)."""
        self._need_prune()
        k = self.prune.keep_counts(self._pr_sizes, self.iterations if s is None else s)
        # n and s are host values: the counts travel as a small array, through pinned memory so that the host does not wait for the stream;
        # it only waits, before it overwrites the staging buffer, for the PREVIOUS update's copy (an update step ago: long done)
        if self._pr_keep_sent is not None:
            self._pr_keep_sent.synchronize()
        self._pr_keep_host.copy_(self.torch.from_numpy(k))
        self._pr_keep.copy_(self._pr_keep_host, non_blocking=True)
        self._pr_keep_sent = self.torch.cuda.Event()
        self._pr_keep_sent.record()
        self._ck('yk_prune_masks_f32', self.P, self._pr_off, self._pr_size, self._pr_keep, self._pr_first, len(self._pr_sizes), self._pr_ntiles,
                 self._pr_mask, self._pr_thr, self._pr_kept)

    def apply_masks(self) -> None:
        """P *= mask, in place (tfmot's weight assignment at the start of a step and its on_epoch_end)."""
        self._need_prune()
        self._ck('yk_mask_apply_f32', self.P, self._pr_mask, self.n_params)
        if self.E is not None:                                       # the exported average is as sparse as the live weights
            self._ck('yk_mask_apply_f32', self.E, self._pr_mask, self.n_params)

    def prune_step(self) -> None:
        """What pruning does at the start of step `iterations`: new masks on an update step, then P *= mask.  Outside the captured
        step, like Adam; P and the mask are only written in place, so the capture stays valid."""
        if self.prune.is_update(self.iterations):
            self.update_masks()
        self.apply_masks()

    def prune_masks(self) -> Dict[str, np.ndarray]:
        """Current mask of every pruned kernel, Keras layout (HWIO) bool arrays."""
        self._need_prune()
        out = {}
        for nm in self._pr_names:
            kh, kw, ci, co = self.lay[nm[:-7]].kernel_shape
            m = self.view(self._pr_mask, nm).cpu().numpy()
            out[nm] = np.transpose(m.reshape(co, kh, kw, ci), (1, 2, 3, 0)).astype(bool)
        return out

    def prune_report(self) -> Dict[str, dict]:
        """Per pruned kernel: n, kept (mask bytes set), threshold (the k-th largest |w| at the last update) and the achieved sparsity."""
        self._need_prune()
        kept, thr = self._pr_kept.cpu().numpy(), self._pr_thr.cpu().numpy()
        return {nm: dict(n=n, kept=int(k), threshold=float(t), sparsity=1.0 - int(k) / n)
                for nm, n, k, t in zip(self._pr_names, self._pr_sizes, kept, thr)}

    # ------------------------------------------------------------------ quantisation-aware training
    def _qat_init(self) -> None:
        """The slot table (one slot per spec tensor), the range and batch-extreme tables, the shadow parameter buffer Pq and the segment
        tables of all conv / depthwise kernels.  Allocated once: the captured step holds their pointers."""
        from . import quantize
        from .qat import slot_table
        torch = self.torch
        kind, p0, p1 = slot_table(self.spec)                        # KmodelError naming the op the KPU path cannot express
        self._qa_kind, self._qa_parts = kind, list(zip(p0, p1))
        self._qa_names = quantize.tensor_names(self.spec)
        self._qa_n = n = len(kind)
        dev = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(self.dev)
        self._qa_kind_d, self._qa_p0_d, self._qa_p1_d = dev(kind, np.int32), dev(p0, np.int32), dev(p1, np.int32)
        self._qa_ranges = dev(np.tile(np.array([np.inf, -np.inf], np.float32), n), np.float32)       # nothing seen yet
        self._qa_batch = torch.zeros(4 * n, dtype=torch.int32, device=self.dev)                      # YK_RANGE_WORDS per slot
        self._ck('yk_range_reset', self._qa_batch, n)
        self.Pq = torch.zeros_like(self.P)
        names = [l.name + '/kernel' for l in self.spec.layers]
        offs = [self.slots[nm][0] for nm in names]
        sizes = [int(np.prod(self.slots[nm][1])) for nm in names]
        tile = engine.lib().yk_qat_tile()
        first = np.concatenate([[0], np.cumsum([(s + tile - 1) // tile for s in sizes])])
        assert all(o >= 0 and s >= 1 and o + s <= self.n_params for o, s in zip(offs, sizes)) and first[-1] < 2 ** 31
        self._qa_off, self._qa_size, self._qa_first = dev(offs, np.int64), dev(sizes, np.int64), dev(first, np.int32)
        self._qa_nseg, self._qa_ntiles = len(offs), int(first[-1])
        self._qa_wrange = torch.zeros(4 * len(offs), dtype=torch.int32, device=self.dev)
        self._qa_ready = False                                       # ranges come from qat_observe or qat_set_ranges

    def _need_qat(self):
        if self.qat is None:
            raise engine.YkError('this Trainer was built without quantisation-aware training (qat=None)')

    def _qat_weights(self) -> None:
        """Pq = P with every conv / depthwise kernel replaced by fq over its own [min, max]: one library call, three launches."""
        self._ck('yk_qat_weights_f32', self.P, self.n_params, self._qa_off, self._qa_size, self._qa_first, self._qa_nseg, self._qa_ntiles, self.Pq,
                 self._qa_wrange)

    def _qat_out(self, i, slot, y, S, observe):
        """Tensor `slot`, the output of op i: folded into the batch extremes only (observe), or fake-quantised over the slot's range into a
        new tensor while y stays on the tape for the backward kernel."""
        if observe:
            self._ck('yk_range_f32', y, y.numel(), self._qa_batch, slot)
            return y
        yq = self.torch.empty_like(y)
        self._ck('yk_qat_act_fwd_f32', y, y.numel(), self._qa_ranges, slot, yq, self._qa_batch)
        S.setdefault(i, {})['qy'] = y
        return yq

    def _qat_update(self, observe: bool) -> None:
        m = np.float32(self.qat.momentum)
        self._ck('yk_qat_update_f32', self._qa_ranges, self._qa_batch, self._qa_kind_d, self._qa_p0_d, self._qa_p1_d, self._qa_n, float(m),
                 float(np.float32(1) - m), int(observe))

    def qat_observe(self, x_nhwc) -> None:
        """One training-mode forward with no quantisation at all (BatchNorm moving statistics move as in a step); every range is widened
        to the batch's extremes, starting from "nothing seen yet"."""
        self._need_qat()
        self.forward(x_nhwc, observe=True)
        self._qat_update(True)
        self._qa_ready = True

    def qat_flagged(self) -> List[str]:
        """Names of what has held a NaN or an infinity since construction or the last qat_clear_flags: tensors (conv outputs, concats) by
        their name, kernels as '<layer>/kernel' (as of the last step).  Such values enter no range; the flags are sticky."""
        self._need_qat()
        flags = self._qa_batch.cpu().numpy().reshape(-1, 4)[:, 2]
        wflags = self._qa_wrange.cpu().numpy().reshape(-1, 4)[:, 2]
        return ([self._qa_names[i] for i in range(self._qa_n) if self._qa_kind[i] and flags[i]] +
                [l.name + '/kernel' for l, f in zip(self.spec.layers, wflags) if f])

    def qat_clear_flags(self) -> None:
        """Forget the non-finite flags (in place; the ranges and the batch extremes stay)."""
        self._need_qat()
        self._qa_batch.view(-1, 4)[:, 2].zero_()

    def qat_ranges(self, check: bool = True) -> Dict[str, tuple]:
        """{tensor name (quantize.tensor_names): (lo, hi)} of every conv output and concat.  YkError naming the tensors that have no range
        yet, and (check=True) whatever qat_flagged() names: a tensor or a kernel that held a NaN or an infinity."""
        self._need_qat()
        r = self._qa_ranges.cpu().numpy().reshape(-1, 2)
        own = [i for i in range(self._qa_n) if self._qa_kind[i]]
        bad = self.qat_flagged() if check else []
        if bad:
            raise engine.YkError(f'qat: non-finite values (NaN or infinity) in {", ".join(bad)}: the weights or the frames are broken '
                                 f'(qat_clear_flags() forgets them; qat_ranges(check=False) reads the ranges of the finite values)')
        empty = [self._qa_names[i] for i in own if not r[i, 0] <= r[i, 1]]
        if empty:
            raise engine.YkError(f'qat: no range yet for tensor(s) {", ".join(empty)}: call qat_observe or qat_set_ranges first')
        return {self._qa_names[i]: (float(r[i, 0]), float(r[i, 1])) for i in own}

    def qat_set_ranges(self, ranges: Dict[str, tuple]) -> None:
        """Ranges of the conv outputs from {name: (lo, hi)}; a concat's range is derived (the union of its parts), whatever the dict holds
        for it.  Written in place: a captured step keeps reading the same table."""
        self._need_qat()
        from .qat import SLOT_OWNER, SLOT_UNION
        missing = [self._qa_names[i] for i in range(self._qa_n) if self._qa_kind[i] == SLOT_OWNER and self._qa_names[i] not in ranges]
        if missing:
            raise engine.YkError(f'qat_set_ranges: no range for tensor(s) {", ".join(missing)}')
        r = np.tile(np.array([np.inf, -np.inf], np.float32), (self._qa_n, 1))
        for i in range(self._qa_n):
            if self._qa_kind[i] == SLOT_OWNER:
                lo, hi = (np.float32(v) for v in ranges[self._qa_names[i]])
                if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                    raise engine.YkError(f'qat_set_ranges: range ({lo}, {hi}) of {self._qa_names[i]!r} is not a finite interval')
                r[i] = lo, hi
            elif self._qa_kind[i] == SLOT_UNION:
                a, b = self._qa_parts[i]
                r[i] = min(r[a, 0], r[b, 0]), max(r[a, 1], r[b, 1])
        self._qa_ranges.copy_(self.torch.from_numpy(r.reshape(-1)))
        self._qa_ready = True

    def step(self, x_nhwc, y_true: Sequence["torch.Tensor"], reduce=None, reduce_scalar=None) -> Dict[str, float]:
        """model.fit's inner step (keras_train.py:94).  Returns python floats (one device->host sync)."""
        torch = self.torch
        if self.qat is not None and not self._qa_ready:
            raise engine.YkError('qat: the activation ranges are not set: call qat_observe(x) on a few batches (or qat_set_ranges) before the first step')
        if self.prune is not None:
            self.prune_step()
        if self.distill is not None:
            self.teacher_forward(x_nhwc)                             # before the loss, outside the capture: each rank on its own shard
        r = self._loss_and_grads_replayed(x_nhwc, y_true)
        if self.world > 1:
            self.exchange(reduce)
        self.apply_update()
        iou_box = self.hyper['box_loss'] != 'mse'                     # then the layers' loss[6] is the box term (yk_yolo_loss_ex)
        data = torch.stack([p[0::6] for p in r['layers']]).sum(0)     # [total] or, of 7 entries, [total, box]
        if self.distill is not None:                                  # ... then the distillation term (each rank's carries 1 / global batch)
            data = torch.cat([data, torch.stack([d[0] for d in r['distill']]).sum().view(1)])
        if self.world > 1:
            if reduce_scalar is not None:
                reduce_scalar(data)
            else:
                import torch.distributed as dist
                dist.all_reduce(data, op=dist.ReduceOp.SUM, group=self.pg)
        tail = [r['reg'].view(1)]
        if self.clip_norm:                                            # the float64 sum of squares rides along as two float32 words: one transfer
            tail.append(self._sumsq.view(torch.float32))
        vals = torch.cat([data] + tail).cpu().numpy()
        extra = {}
        if self.lr_schedule is not None:
            extra['lr'] = self.last_lr
        if self.clip_norm:
            extra['grad_norm'] = float(np.sqrt(vals[-2:].copy().view(np.float64)[0]))      # the norm BEFORE clipping
            vals = vals[:-2]
        out = dict(loss=float(vals[0] + vals[-1]), data_loss=float(vals[0]), reg_loss=float(vals[-1]))
        if iou_box:
            out['box'] = float(vals[1])
        if self.distill is not None:                                  # loss is what the step descends: detection + distillation + regulariser
            out['distill'] = float(vals[-2])
            out['loss'] = float(vals[0] + vals[-2] + vals[-1])
        out.update(extra)
        return out

    def precision_recall(self):
        """Yolo_Precision / Yolo_Recall running values per output layer (tools/custom.py:42-44,74-75)."""
        out = []
        for c in self.counts:
            tp, fp, fn = c.cpu().numpy().tolist()
            out.append((tp / (tp + fp) if tp + fp else 0.0, tp / (tp + fn) if tp + fn else 0.0))
        return out
