"""`make train` (reference keras_train.py:27-115) on the HIP training step.

Same CLI and the same `main(...)` parameter list as the reference script.  What `train_model.fit` did inside TensorFlow
is `train.Trainer.step` here; the tf.data pipeline (tools/utils.py:417-450 `_create_dataset`: shuffle, read, letterbox,
`box_to_label`, batch) is `pipeline.InputPipeline` (row N3: per-rank shards, thread-pool decode, GPU letterbox / normalise, two batches of prefetch); the
plain-python `batches()` generator below is its host-only twin (tests compare the two bit for bit).  `--augmenter True` (`make train
IAA=True`) turns on the imgaug OneOf of tools/utils.py:84-88 for the training split: `augment.py`, fused into the GPU letterbox
(`InputPipeline(augment=True)`), parameters keyed by (rand_seed, epoch, row); validation is never augmented.  Validation runs the fp16 inference
engine on the exported weights (BatchNorm with moving statistics, like Keras' test phase).

Checkpoints: `log/<time>/yolo_model.h5` in Keras' WEIGHTS-ONLY HDF5 layout (`model.save_weights` format: readable by the reference's
`load_weights`, keras_inference.py:80; it is not a `save_model` file - no `model_config` - so `keras_freeze.py`'s `load_model` cannot
open it; keras_io / h5lite, no h5py needed) plus the same arrays as `yolo_model.npz`; `--pre_ckpt` takes either.

`--is_prune True` (`make train PRUNE=True`, keras_train.py:59-71,87-90,102-107): magnitude pruning of every Conv2D kernel on a
PolynomialDecay schedule built from the four `--prune_*` flags (`prune.PruneSchedule`, end_step = prune_end_epoch x steps per epoch);
the masks are computed and applied by HIP kernels at the start of a step (`Trainer.prune_step`), once more at the end of every epoch,
the overall and per-head sparsity is printed per epoch (the stand-in for PruningSummaries), and the checkpoint is
`yolo_prune_model.h5` / `.npz` with the masked weights.  The rule is restated from tfmot's public source; parity with it is unpinned.

`--qat True` (`make train QAT=True`; qat.py): the kmodel's 8-bit quantisation simulated in the forward pass, straight-through
gradients in the backward pass.  The first `--qat_observe` (>= 1) batches of epoch 0 only set the activation ranges (no update; an epoch 0
with fewer batches is observed whole and training starts with epoch 1); afterwards the ranges follow the batches with `--qat_momentum`.  The checkpoint is `yolo_qat_model.h5` / `.npz` (the latent float weights; with
`--is_prune True` masked) plus `yolo_qat_ranges.npz` (tensor name -> [lo, hi]), which `make kmodel RANGES=` quantises with.

`--box_loss giou | diou | ciou` (`make train BOXLOSS=ciou`; not in the reference): the IoU-family box term, weighted by
`--box_weight`, in place of the xy and wh terms, in the training step and in the validation loss alike; the step line and the epoch line
then name the box term.  The default `mse` is the reference's loss.

`--focal obj | cls | all` with `--focal_gamma`, `--focal_alpha`, `--label_smooth` and `--obj_target iou` (`make train FOCAL=all FOCALGAMMA=2.0
FOCALALPHA=0.25 LABELSMOOTH=0.1 OBJTARGET=iou`; not in the reference, lossopt.py): focal loss on the objectness and / or class
terms, smoothed class targets, and the IoU of the predicted box as the objectness target of an object cell, in the training step and in the
validation loss alike.  One line at the start names the options in force; with all of them off (the default) nothing changes.

`--mosaic True` (`make train MOSAIC=True MOSAICPROB=1.0 MOSAICOFF=0`; not in the reference, mosaic.py): a share `--mosaic_prob`
of the training samples is composed of four pictures of the training list by one HIP launch per batch (`InputPipeline(mosaic=...)`), draws keyed
by (rand_seed, epoch, row); with `--augmenter True` the augmentation acts on the mosaic.  The last `--mosaic_off_epochs` epochs train on plain
samples; validation is never mosaicked.

`--hsv True` (`make train HSV=True HSVHUE=0.1 HSVSAT=1.5 HSVEXP=1.5 HSVPROB=1.0`; not in the reference, colour.py): a share
`--hsv_prob` of the training frames gets a hue rotation of up to +-`--hsv_hue` turns and saturation and exposure gains between 1/x and x of
`--hsv_sat` and `--hsv_exposure` (Darknet's recipe), by one HIP launch per batch on the finished frame (`InputPipeline(hsv=...)`), draws
keyed by (rand_seed, epoch, row).  It acts after the letterbox, the augmentation and the mosaic, in every epoch (the `--mosaic_off_epochs`
tail included); validation is never jittered.

`--teacher_ckpt weights.h5|.npz` (`make train TEACHERCKPT=big.h5 TEACHER=yolo_mobilev2 TEACHERDEPTH=1.0 DISTILLWEIGHT=1.0`; not in the
reference, distill.py): knowledge distillation from a trained network of the zoo with the same image size, output size, anchor
count and class count (`--teacher_def` / `--teacher_depth`; by default the student's own, e.g. its float, unpruned checkpoint for a QAT or a
pruned run).  The teacher runs as an inference plan on the step's frames and one HIP launch per output layer adds the objectness-scaled
distillation term, weighted by `--distill_weight`, to the loss and its gradient; the step line and the epoch line then name the `distill`
term.  The validation loss stays the detection loss.  The empty default means off.

`--cache gpu` (`make train CACHE=gpu CACHEGB=8 CACHESTAGE=256`; not in the reference, cache.py): every training picture is
decoded once and kept in `--cache_gb` GB of device memory; what does not fit passes through staging regions of `--cache_stage_mb` MB every
time.  The loop owns the cache, every epoch's `InputPipeline(cache=...)` composes its batches from it by one launch - the batches of
`--cache off`, bit for bit - and the epoch line gains `cache hits/misses, GB used/capacity`.  `--decode gpu` (`DECODE=gpu`, with or without
the cache) has baseline JPEG files decoded on the GPU, directly into that memory: `make detect DECODE=gpu`'s pixels, not PIL's.  Validation
is not cached.

`--ema True`, `--clip_norm N`, `--lr_schedule cosine|step|constant` (`make train EMA=True EMADECAY=0.9999 EMATAU=2000 CLIPNORM=10.0
LRSCHED=cosine WARMUP=N LRFINAL=0.01`; not in the reference, optim.py): an exponential moving average of the weights and of the
BatchNorm moving statistics, which validation scores (`(ema)` on the epoch line) and rank 0 saves as `yolo_ema_model.h5` / `.npz` (with
`--is_prune True` `yolo_prune_ema_model.*`, as sparse as the live one) beside the usual checkpoint of the live weights; global-norm gradient
clipping, the step line then shows `gnorm`, the norm before clipping; a learning-rate schedule with linear warmup over the run's
`train_epoch_step x max_nrof_epochs` steps (capped by `--max_steps`), the step line then shows `lr`.  All off by default: then the update is
the reference's Adam call and no line changes.

`--labels gpu`, `--assign multi`, `--assign_iou` (`make train LABELS=gpu ASSIGN=multi ASSIGNIOU=0.213`; not in the reference): the
label grids are built on the GPU from the batch's boxes by one HIP launch (`InputPipeline(labels='gpu')`), the bits of the host's; with
`--assign multi` a box is written not only at its best-fitting (layer, anchor) but at every other whose fit exceeds `--assign_iou`
(`Helper.box_to_label`), under either `--labels` value, in training and validation alike.  One line at the start names a non-default
value; with the defaults (host, best) nothing changes."""
from __future__ import annotations

import argparse
import os
import sys
import time
from datetime import datetime
from pathlib import Path

import numpy as np

from . import engine, netspec
from .helper import ERROR, INFO, Helper, write_arguments_to_file


def synthetic_list(n: int, in_hw, class_num: int, seed: int):
    """In-memory stand-in for data/<set>_img_ann.npy: [(uint8 image, boxes[cls,x,y,w,h])]: coloured rectangles on noise."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        img = rng.integers(0, 64, (in_hw[0], in_hw[1], 3), dtype=np.uint8)
        k = int(rng.integers(1, 4))
        boxes = np.zeros((k, 5))
        for j in range(k):
            c = int(rng.integers(0, class_num))
            w, h = rng.uniform(0.15, 0.5, 2)
            x, y = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
            boxes[j] = [c, x, y, w, h]
            x0, x1 = int((x - w / 2) * in_hw[1]), int((x + w / 2) * in_hw[1])
            y0, y1 = int((y - h / 2) * in_hw[0]), int((y + h / 2) * in_hw[0])
            img[y0:y1, x0:x1] = (np.array([37, 91, 151]) * (c + 1)) % 200 + 55
        out.append((img, boxes))
    return out


def batches(h: Helper, items, batch_size: int, rng, shuffle: bool, augment=None, with_boxes: bool = False, mosaic=None, hsv=None,
            assign: str = 'best', assign_iou: float = 0.213, make_labels: bool = True):
    """tools/utils.py:417-450: (normalised image [B,H,W,3] float32, labels per layer [B,h,w,A,5+C] float32).  augment=(seed, epoch):
    every sample augmented with its row of augment.param_table(seed, epoch, len(items)), like InputPipeline(augment=True).
    with_boxes: a third element, each sample's boxes [n,5] (class, cx, cy, w, h) relative to the letterboxed frame.
    mosaic=(seed, epoch, prob): every sample composed by mosaic.py from its row of mosaic.param_table(seed, epoch, len(items)) on the host
    (mosaic.compose_u8), like InputPipeline(mosaic=MosaicConfig(prob)); the augmentation, if any, then acts on the mosaic.
    hsv=(seed, epoch, HsvConfig): the finished u8 frame of every sample jittered on the host (colour.jitter_u8) with its row of
    colour.param_table(seed, epoch, len(items), HsvConfig), like InputPipeline(hsv=HsvConfig); labels and boxes do not change.
    assign, assign_iou: the positive assignment of Helper.box_to_label, like InputPipeline(assign=, assign_iou=).
    make_labels=False: no label grid is built, the second element is None (for a caller that builds them from the boxes: with_boxes)."""
    from . import augment as aug_mod
    from . import colour as colour_mod
    from . import mosaic as mosaic_mod
    table = None if augment is None else aug_mod.param_table(augment[0], augment[1], len(items))
    mtable = None if mosaic is None else mosaic_mod.param_table(mosaic[0], mosaic[1], len(items))
    ctable = None if hsv is None else colour_mod.param_table(hsv[0], hsv[1], len(items), hsv[2])
    hw = (int(h.in_hw[0][0]), int(h.in_hw[0][1]))
    order = rng.permutation(len(items)) if shuffle else np.arange(len(items))

    def picture(i, cache):
        if i not in cache:
            img = items[i][0]
            cache[i] = np.asarray(h._read_img(str(img)) if isinstance(img, (str, os.PathLike)) else img)[..., :3]
        return cache[i]
    for s in range(0, len(order) - batch_size + 1, batch_size):             # drop_remainder=True (utils.py:447)
        xs, ys, bs = [], [[] for _ in range(len(h.anchors))], []
        rows = order[s:s + batch_size]
        if mtable is not None:
            cache = {}
            quads, centres, box_lists = mosaic_mod.plan(rows, mtable, lambda i: picture(i, cache).shape[:2], hw,
                                                        boxes_of=lambda i: items[i][1], prob=mosaic[2])
        for k, i in enumerate(rows):
            if mtable is not None:
                img = mosaic_mod.compose_u8([picture(int(j), cache) for j in quads[k]['item']], quads[k], centres[k], hw)
                boxes = box_lists[k]
            else:
                img, boxes = items[i]
                if isinstance(img, (str, os.PathLike)):
                    img = h._read_img(str(img))
                boxes = np.array(boxes, np.float64, copy=True)
            img, boxes = h._process_img(img, boxes, is_training=table is not None, is_resize=mtable is None,
                                        aug=None if table is None else table[i], hsv=None if ctable is None else ctable[i])
            xs.append(img.astype(np.float32))
            bs.append(boxes)
            if make_labels:
                for l, lab in enumerate(h.box_to_label(boxes, assign=assign, assign_iou=assign_iou)):
                    ys[l].append(lab)
        labs = [np.stack(y).astype(np.float32) for y in ys] if make_labels else None
        if with_boxes:
            yield np.stack(xs), labs, bs
        else:
            yield np.stack(xs), labs


def main(args, train_set, class_num, pre_ckpt, model_def, depth_multiplier, is_augmenter, image_size, output_size, batch_size,
         rand_seed, max_nrof_epochs, init_learning_rate, learning_rate_decay_factor, obj_weight, noobj_weight, wh_weight,
         obj_thresh, iou_thresh, vaildation_split, log_dir, is_prune, initial_sparsity=0.5, final_sparsity=0.9, end_epoch=5,
         frequency=100, synthetic=0, max_steps=0, is_qat='False', qat_momentum=0.99, qat_observe=8, val_map='False', val_map_obj=0.05,
         box_loss='mse', box_weight=1.0, is_mosaic='False', mosaic_prob=1.0, mosaic_off_epochs=0, is_hsv='False', hsv_hue=0.1, hsv_sat=1.5,
         hsv_exposure=1.5, hsv_prob=1.0, teacher_ckpt='', teacher_def=None, teacher_depth=None, distill_weight=1.0, cache='off',
         cache_gb=8.0, cache_stage_mb=256, decode='pil', is_ema='False', ema_decay=0.9999, ema_tau=2000.0, clip_norm=0.0, lr_schedule='none',
         warmup_steps=0, lr_final=0.01, focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label',
         labels='host', assign='best', assign_iou=0.213):
    import torch
    from . import lossopt
    from .train import Trainer
    try:
        loss_opts = lossopt.validate(focal, focal_gamma, focal_alpha, label_smooth, obj_target)
    except ValueError as e:
        raise engine.YkError(f'--focal / --focal_gamma / --focal_alpha / --label_smooth / --obj_target: {e}') from e
    prune = is_prune == 'True'
    qat = is_qat == 'True'
    if qat and int(qat_observe) < 1:
        raise engine.YkError(f'--qat_observe {qat_observe}: at least one batch must set the activation ranges before the first step')
    augment = is_augmenter == 'True'
    mosaic = is_mosaic == 'True'
    if mosaic and not 0.0 <= float(mosaic_prob) <= 1.0:
        raise engine.YkError(f'--mosaic_prob {mosaic_prob}: a probability')
    if mosaic and int(mosaic_off_epochs) < 0:
        raise engine.YkError(f'--mosaic_off_epochs {mosaic_off_epochs}: a number of epochs')
    hsv = is_hsv == 'True'
    hsv_cfg = None
    if hsv:
        from .colour import HsvConfig
        for flag, v, ok, want in (('--hsv_hue', float(hsv_hue), 0.0 <= float(hsv_hue) <= 0.5, 'turns of the hue circle, 0 to 0.5'),
                                  ('--hsv_sat', float(hsv_sat), float(hsv_sat) >= 1.0, 'the largest saturation gain, at least 1'),
                                  ('--hsv_exposure', float(hsv_exposure), float(hsv_exposure) >= 1.0, 'the largest exposure gain, at least 1'),
                                  ('--hsv_prob', float(hsv_prob), 0.0 <= float(hsv_prob) <= 1.0, 'a probability')):
            if not (np.isfinite(v) and ok):
                raise engine.YkError(f'{flag} {v}: {want}')
        hsv_cfg = HsvConfig(float(hsv_hue), float(hsv_sat), float(hsv_exposure), float(hsv_prob))
    if cache not in ('off', 'gpu'):
        raise engine.YkError(f'--cache {cache}: off or gpu')
    if decode not in ('pil', 'gpu'):
        raise engine.YkError(f'--decode {decode}: pil or gpu')
    cached = cache == 'gpu'
    if cached and not (np.isfinite(float(cache_gb)) and float(cache_gb) >= 0.0):
        raise engine.YkError(f'--cache_gb {cache_gb}: a size in GB, not negative')
    if (cached or decode == 'gpu') and not (np.isfinite(float(cache_stage_mb)) and float(cache_stage_mb) > 0.0):
        raise engine.YkError(f'--cache_stage_mb {cache_stage_mb}: a size in MB, positive')
    ema = is_ema == 'True'
    if ema and qat:
        raise engine.YkError('--ema True together with --qat True is not supported: the learned activation ranges belong to the live weights')
    if not (np.isfinite(float(clip_norm)) and float(clip_norm) >= 0.0):
        raise engine.YkError(f'--clip_norm {clip_norm}: the largest gradient norm, not negative (0 is off)')
    if lr_schedule not in ('none', 'constant', 'cosine', 'step'):
        raise engine.YkError(f'--lr_schedule {lr_schedule}: none, constant, cosine or step')
    scheduled = lr_schedule != 'none'
    if scheduled and float(learning_rate_decay_factor) != 0.0:
        raise engine.YkError(f'--lr_schedule {lr_schedule} together with --learning_rate_decay_factor {learning_rate_decay_factor} would be two schedules')
    distill = teacher_ckpt not in (None, 'None', '', '""')
    if labels not in ('host', 'gpu'):
        raise engine.YkError(f'--labels {labels}: host or gpu')
    try:
        Helper.check_assign(assign, float(assign_iou))
    except ValueError as e:
        raise engine.YkError(f'--assign {assign} --assign_iou {assign_iou}: {e}') from e
    label_opts = dict(labels=labels, assign=assign, assign_iou=float(assign_iou))
    if distill and not (np.isfinite(float(distill_weight)) and float(distill_weight) >= 0.0):
        raise engine.YkError(f'--distill_weight {distill_weight}: a finite weight, not negative')
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    try:
        engine.require_gpu()
    except engine.YkError as e:
        if prune:
            raise engine.YkError('--is_prune True (magnitude pruning, keras_train.py:59-71) runs in HIP kernels on the training step: '
                                 'no HIP device') from e
        if qat:
            raise engine.YkError('--qat True (quantisation-aware fine-tuning) runs in HIP kernels on the training step: no HIP device') from e
        if augment:
            raise engine.YkError('--augmenter True (imgaug OneOf, tools/utils.py:84-88) runs in the GPU input pipeline: no HIP device') from e
        if mosaic:
            raise engine.YkError('--mosaic True (four pictures per sample, mosaic.py) runs in the GPU input pipeline: no HIP device') from e
        if hsv:
            raise engine.YkError('--hsv True (HSV colour jitter, colour.py) runs in the GPU input pipeline: no HIP device') from e
        if distill:
            raise engine.YkError('--teacher_ckpt (knowledge distillation, distill.py) runs the teacher and its loss in HIP kernels: no HIP device') from e
        if cached:
            raise engine.YkError('--cache gpu (the picture cache, cache.py) keeps the decoded training pictures in device memory: no HIP device') from e
        if ema or scheduled or float(clip_norm):
            raise engine.YkError('--ema / --clip_norm / --lr_schedule (optim.py) run in HIP kernels on the training step: no HIP device') from e
        if labels == 'gpu':
            raise engine.YkError('--labels gpu (the label grids built by yk_boxes_to_labels_f32) runs in the GPU input pipeline: no HIP device') from e
        if decode == 'gpu':
            raise engine.YkError('--decode gpu (baseline JPEG files decoded by yk_jpeg_decode_ragged_u8) runs in the GPU input pipeline: no HIP device') from e
        raise
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device(f'cuda:{local}'))
    log_dir = Path(log_dir) / datetime.strftime(datetime.now(), '%Y%m%d-%H%M%S')
    if rank == 0:
        log_dir.mkdir(parents=True, exist_ok=True)
        write_arguments_to_file(args, str(log_dir / 'args.txt'))                # keras_train.py:41
    in_hw, out_hw = np.reshape(np.array(image_size), (-1, 2)), np.reshape(np.array(output_size), (-1, 2))
    anchors = f'data/{train_set}_anchor.npy'
    if synthetic:
        h = Helper(None, class_num, anchors, in_hw, out_hw, vaildation_split)
        items = synthetic_list(synthetic, in_hw[0], class_num, rand_seed)
        nval = int(len(items) * vaildation_split)
        h.test_list, h.train_list = items[:nval], items[nval:]
    else:
        ann = Path(f'data/{train_set}_img_ann.npy')
        if not ann.exists():
            raise engine.YkError(f'{ann} not found (make_voc_list.py output); pass --synthetic N for generated data')
        h = Helper(str(ann), class_num, anchors, in_hw, out_hw, vaildation_split)
        h.train_list = [(a[0], a[1]) for a in h.train_list]
        h.test_list = [(a[0], a[1]) for a in h.test_list]
    if batch_size % world:
        raise engine.YkError(f'batch_size {batch_size} must divide by the {world} ranks')
    per_rank = batch_size // world
    h.batch_size = batch_size
    spec = netspec.NETWORKS[model_def]([image_size[0], image_size[1], 3], len(h.anchors[0]), class_num, alpha=depth_multiplier)
    assert [tuple(x) for x in spec.out_hw()] == [tuple(x) for x in out_hw], (spec.out_hw(), out_hw)
    weights = spec.init_keras_default(rand_seed)
    if pre_ckpt not in (None, 'None', ''):                                       # keras_train.py:52-57
        if load_weights(spec, pre_ckpt, weights):
            print(INFO, f' Load CKPT {str(pre_ckpt)}')
        else:
            print(ERROR, ' Pre CKPT path is unvalid')
    distill_cfg = None
    if distill:
        from .distill import DistillConfig, check_teacher
        t_def = model_def if teacher_def in (None, 'None', '') else teacher_def
        t_depth = depth_multiplier if teacher_depth in (None, 'None', '') else float(teacher_depth)
        if t_def not in netspec.NETWORKS:
            raise engine.YkError(f'--teacher_def {t_def}: choose one of {", ".join(sorted(netspec.NETWORKS))}')
        t_spec = netspec.NETWORKS[t_def]([image_size[0], image_size[1], 3], len(h.anchors[0]), class_num, alpha=t_depth)
        check_teacher(spec, t_spec, h.anchors)                                   # before the file is read: names the first difference
        t_weights = t_spec.init_keras_default(rand_seed)
        if not load_weights(t_spec, teacher_ckpt, t_weights):
            raise engine.YkError(f'--teacher_ckpt {teacher_ckpt}: a .h5 or .npz checkpoint of {t_def}-{t_depth}')
        distill_cfg = DistillConfig(t_spec, t_weights, float(distill_weight))
        if rank == 0:
            print(INFO, f' Load teacher CKPT {str(teacher_ckpt)} ({t_def}-{t_depth}), distill_weight {float(distill_weight)}')
    schedule = None
    if prune:                                                                    # keras_train.py:60-66: end_step = train_epoch_step * end_epoch
        from .prune import PruneSchedule
        schedule = PruneSchedule(initial_sparsity, final_sparsity, end_epoch * (len(h.train_list) // batch_size), frequency)
    qat_cfg = None
    if qat:
        from .qat import QatConfig
        qat_cfg = QatConfig(qat_momentum)
    ema_cfg = lr_cfg = None
    try:
        if ema:
            from .optim import EmaConfig
            ema_cfg = EmaConfig(float(ema_decay), float(ema_tau))
        if scheduled:                                                            # the run's length: every epoch's steps, capped by --max_steps
            from .optim import LrSchedule
            total = (len(h.train_list) // batch_size) * max_nrof_epochs
            total = min(total, int(max_steps)) if max_steps else total
            lr_cfg = LrSchedule(lr_schedule, float(init_learning_rate), max(total, 1), warmup_steps=int(warmup_steps), final_frac=float(lr_final))
    except ValueError as e:
        raise engine.YkError(f'--ema_decay / --ema_tau / --lr_schedule / --warmup_steps / --lr_final: {e}') from e
    if rank == 0 and (ema or scheduled or float(clip_norm)):
        print(INFO, f'ema is {ema_cfg}, clip_norm {float(clip_norm)}, lr schedule {lr_cfg}')
    if rank == 0 and not lossopt.is_off(**loss_opts):
        print(INFO, f'loss options: {lossopt.describe(**loss_opts)}')
    if rank == 0 and (labels != 'host' or assign != 'best'):
        print(INFO, f'labels are built on the {labels}, assign is {assign}' + (f', assign_iou {float(assign_iou)}' if assign == 'multi' else ''))
    tr = Trainer(spec, weights, h.anchors, per_rank, obj_thresh=obj_thresh, iou_thresh=iou_thresh, obj_weight=obj_weight,
                 noobj_weight=noobj_weight, wh_weight=wh_weight, lr=init_learning_rate, decay=learning_rate_decay_factor, device=local,
                 world_size=world, prune=schedule, qat=qat_cfg, box_loss=box_loss, box_weight=box_weight, distill=distill_cfg,
                 ema=ema_cfg, clip_norm=float(clip_norm), lr_schedule=lr_cfg, **loss_opts)
    from .mosaic import MosaicConfig
    from .pipeline import InputPipeline
    if rank == 0:
        print(INFO, 'data augment is ', str(augment))                            # utils.py:418
        print(INFO, f'mosaic is {mosaic}, mosaic_prob {float(mosaic_prob)}, mosaic_off_epochs {int(mosaic_off_epochs)}')
        print(INFO, f'hsv is {hsv}, hsv_hue {float(hsv_hue)}, hsv_sat {float(hsv_sat)}, hsv_exposure {float(hsv_exposure)}, hsv_prob {float(hsv_prob)}')
        if cached or decode == 'gpu':
            print(INFO, f'cache is {cache}, cache_gb {float(cache_gb)}, cache_stage_mb {float(cache_stage_mb)}, decode is {decode}')
    # the decoded pictures stay on the device from epoch to epoch (cache.py): the loop owns the arena, every epoch's pipeline reads it;
    # --decode gpu without --cache gpu runs on its staging ring alone
    pic_cache = None
    if cached or decode == 'gpu':
        from .cache import PictureCache
        pic_cache = PictureCache(int(float(cache_gb) * (1 << 30)) if cached else 0, int(float(cache_stage_mb) * (1 << 20)), prefetch=2, device=local)
    steps, observed = 0, 0
    iou_box = box_loss != 'mse'
    for epoch in range(max_nrof_epochs):
        t0, seen, run, run_box, run_kd = time.time(), 0, 0.0, 0.0, 0.0
        if rank == 0 and mosaic and int(mosaic_off_epochs) > 0 and epoch == max(max_nrof_epochs - int(mosaic_off_epochs), 0):
            print(f'epoch {epoch + 1}: mosaic off from here on', flush=True)
        # tools/utils.py:417-450: each rank decodes only its rows of the global batch, on a thread pool, two batches ahead;
        # letterbox + normalise on the GPU (pipeline.py)
        pipe = InputPipeline(h, h.train_list, batch_size, rank, world, seed=rand_seed, epoch=epoch, shuffle=True, device=local,
                             augment=augment,                                    # the last mosaic_off_epochs epochs train on plain samples
                             mosaic=MosaicConfig(float(mosaic_prob)) if mosaic and epoch < max_nrof_epochs - int(mosaic_off_epochs) else None,
                             hsv=hsv_cfg,                                       # ... the colour jitter stays on in them
                             **({} if pic_cache is None else dict(cache=pic_cache, decode=decode)),
                             **({} if labels == 'host' and assign == 'best' else label_opts))
        try:                                                                    # an exception in the step must not leave the producer running
            for x, ys in pipe:
                if qat and epoch == 0 and observed < int(qat_observe):           # the first batches of epoch 0 only set the activation ranges
                    tr.qat_observe(x)
                    observed += 1
                    continue
                out = tr.step(x, ys)
                seen, run, steps = seen + 1, run + out['loss'], steps + 1
                run_box += out.get('box', 0.0)
                run_kd += out.get('distill', 0.0)
                if rank == 0 and (seen % 10 == 0 or seen == 1):
                    pr = tr.precision_recall()
                    print(f'epoch {epoch + 1} step {seen}: loss {out["loss"]:.4f} ' + (f'{box_loss} {out["box"]:.4f} ' if iou_box else '') +
                          (f'distill {out["distill"]:.4f} ' if distill else '') + (f'lr {out["lr"]:.3g} ' if scheduled else '') +
                          (f'gnorm {out["grad_norm"]:.4g} ' if float(clip_norm) else '') +
                          ' '.join(f'l{i + 1}_p {p:.3f} l{i + 1}_r {r:.3f}' for i, (p, r) in enumerate(pr)), flush=True)
                if max_steps and steps >= max_steps:
                    break
            pipe_rate = pipe.producer_images_per_sec()
        finally:
            pipe.close()
        if prune:
            tr.apply_masks()                                                    # tfmot on_epoch_end: validation sees masked weights
            if rank == 0:
                print(sparsity_line(tr, spec, epoch), flush=True)
        val = vmap = None
        if rank == 0 and len(h.test_list) >= per_rank:
            if val_map == 'True':                                               # opt-in: the pass also scores its detections
                val, vmap = validate(tr, h, spec, per_rank, rank, map_obj=val_map_obj, ema=ema, **label_opts)
            else:
                val = validate(tr, h, spec, per_rank, rank, ema=ema, **label_opts)
        if rank == 0:
            print(f'epoch {epoch + 1}: {seen} steps, mean loss {run / max(seen, 1):.4f}, ' +
                  (f'mean {box_loss} {run_box / max(seen, 1):.4f}, ' if iou_box else '') +
                  (f'mean distill {run_kd / max(seen, 1):.4f}, ' if distill else '') +
                  (f'val_loss {val:.4f}{" (ema)" if ema else ""}, ' if val is not None else '') + f'{time.time() - t0:.1f}s, input pipeline {pipe_rate:.0f} images/s/rank' +
                  (f', val_mAP {vmap:.4f}' if vmap is not None else '') + (cache_line(pic_cache) if cached else ''), flush=True)
        for c in tr.counts:
            c.zero_()                                                           # Keras resets metrics every epoch
        if max_steps and steps >= max_steps:
            break
    if pic_cache is not None:
        pic_cache.close()
    if rank == 0:
        from . import keras_io
        stem = 'yolo_qat_model' if qat else 'yolo_prune_model' if prune else 'yolo_model'      # keras_train.py:102-111
        ckpt = log_dir / f'{stem}.h5'
        if prune:
            tr.apply_masks()                                                    # (a run cut short by --max_steps ends inside an epoch)
        final = tr.export_weights()
        keras_io.save_keras_model(spec, final, str(ckpt))                      # save_model layout: /model_weights + model_config
        np.savez(log_dir / f'{stem}.npz', **final)
        if qat:                                                                 # this rank's ranges (per replica, like BatchNorm statistics)
            flagged = tr.qat_flagged()                                          # non-finite values never enter a range: the file is written anyway
            if flagged:
                print(ERROR, f' QAT met non-finite values (NaN or infinity) in {", ".join(flagged)}; yolo_qat_ranges.npz holds the ranges of the finite ones')
            np.savez(log_dir / 'yolo_qat_ranges.npz', **{k: np.asarray(v, np.float32) for k, v in tr.qat_ranges(check=False).items()})
        if ema:                                                                 # beside the live checkpoint: the averaged weights and statistics
            ema_stem = 'yolo_prune_ema_model' if prune else 'yolo_ema_model'
            averaged = tr.export_weights(ema=True)
            keras_io.save_keras_model(spec, averaged, str(log_dir / f'{ema_stem}.h5'))
            np.savez(log_dir / f'{ema_stem}.npz', **averaged)
        print()
        if ema:
            print(INFO, f' Save EMA Model as {str(log_dir / (ema_stem + ".h5"))}')
        print(INFO, f' Save QAT Model as {str(ckpt)} (ranges: yolo_qat_ranges.npz)' if qat else
              f' Save Pruned Model as {str(ckpt)}' if prune else f' Save Model as {str(ckpt)}')
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return tr


def cache_line(pic_cache) -> str:
    """What --cache gpu appends to the epoch line: the distinct pictures of the batches so far served from the cache / brought in, and the
    persistent part's fill."""
    s = pic_cache.stats()
    return f', cache {s.hits}/{s.misses} hits/misses, {s.bytes_used / 2 ** 30:.2f}/{s.capacity / 2 ** 30:.2f} GB'


def load_weights(spec, path, weights) -> bool:
    """A checkpoint into `weights` (Keras layout, in place), keras_train.py:52-57: a Keras .h5 file (every layer must be there) or the .npz
    written beside it.  -> False for any other path."""
    if 'h5' in str(path):
        from . import keras_io
        loaded, _ = keras_io.load_keras_weights(spec, str(path), base=weights, strict=True)
        weights.update(loaded)
        return True
    if str(path).endswith('.npz'):
        weights.update({k: v for k, v in np.load(path).items()})
        return True
    return False


def sparsity_line(tr, spec, epoch: int) -> str:
    """Achieved sparsity of the masks, overall and per scale head (the biased output convs): what PruningSummaries logs, as one line."""
    rep = tr.prune_report()
    n, kept = sum(r['n'] for r in rep.values()), sum(r['kept'] for r in rep.values())
    heads = [l.name for l in spec.layers if l.kind == 'conv' and l.use_bias]
    last = min(max(tr.iterations - 1, 0), tr.prune.end_step) // tr.prune.frequency * tr.prune.frequency      # the last update step so far
    return (f'epoch {epoch + 1}: masks of step {last}, target sparsity {float(tr.prune.sparsity(last)):.4f}, '
            f'achieved {1.0 - kept / n:.4f} over {len(rep)} kernels ({n - kept} of {n} weights masked); heads ' +
            ' '.join(f'{nm} {rep[nm + "/kernel"]["sparsity"]:.4f}' for nm in heads))


def validate(tr, h: Helper, spec, batch: int, rank: int, map_obj=None, ema: bool = False, labels: str = 'host', assign: str = 'best',
             assign_iou: float = 0.213):
    """validation_data pass (keras_train.py:96-98): inference-mode forward on the engine (the f16x2 mode, the boundary default) + the same loss.
    map_obj (`--val_map True`): the plan's outputs are also decoded on the GPU at this objectness threshold (NMS and match IoU = the run's
    iou_thresh) and scored in device memory by map_gpu.MapEvaluator against the validation boxes in network-input pixels - the letterboxed
    frame is the image; -> (val_loss, val_mAP) instead of val_loss.
    ema (`--ema True`): the plan is built from the averaged weights, tr.export_weights(ema=True), for the loss and the mAP alike.
    labels, assign, assign_iou: the run's label options (InputPipeline's): the validation labels follow the same assignment and, with
    labels='gpu', are built by the same kernel from the batch's boxes; a box it could not write raises, as in training."""
    import torch
    tot, n, statuses = 0.0, 0, []
    e = 5 + spec.class_num
    ev = cfg = None
    if map_obj is not None:
        from .evaluate import ground_truth_rows
        from .map_gpu import MapEvaluator
        ev = MapEvaluator(spec.class_num, tr.hyper['iou_thresh'], device=tr.dev.index or 0)
        cfg = engine.make_decode_cfg(h.anchors, spec.class_num, spec.in_hw, spec.out_hw())
    with engine.Plan(spec, tr.export_weights(ema=True) if ema else tr.export_weights(), max_batch=batch, device=tr.dev.index or 0) as plan:   # freed on exit, every epoch
        for x, ys, *boxes in batches(h, h.test_list, batch, np.random.default_rng(0), shuffle=False, with_boxes=ev is not None or labels == 'gpu',
                                     assign=assign, assign_iou=assign_iou, make_labels=labels != 'gpu'):
            plan.run_f32(torch.from_numpy(x).cuda())
            if labels == 'gpu':
                first = np.concatenate([[0], np.cumsum([len(b) for b in boxes[0]])])
                ys, status = engine.boxes_to_labels(np.concatenate([np.reshape(b, (-1, 5)) for b in boxes[0]]), first, h, assign, assign_iou)
                statuses.append(status)                                         # read once, after the pass
            if ev is not None:
                dets, counts = engine.decode_py(cfg, plan.outputs(), batch, None, float(map_obj), tr.hyper['iou_thresh'])
                ev.add(dets, counts, [ground_truth_rows(b, spec.in_hw) for b in boxes[0]])
            for li, (o, yt) in enumerate(zip(plan.outputs(), ys)):
                yp = o[:batch].reshape(batch, *spec.tensors[spec.outputs[li]][:2], spec.anchor_num, e).contiguous()
                loss6, _, _ = engine.yolo_loss(yt if torch.is_tensor(yt) else torch.from_numpy(yt).cuda(), yp, tr.anchors[li], batch_size=batch, want_grad=False, **tr.hyper)
                tot += float(loss6[0])
            n += 1
    for b, status in enumerate(statuses):
        if int(status.item()) != engine.LABEL_STATUS_CLEAN:
            raise engine.YkError(f'validate: box {int(status.item())} of validation batch {b} has a centre cell outside a label grid it is written to')
    if ev is not None:
        return tot / max(n, 1), ev.result()['map']
    return tot / max(n, 1)


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument('--train_set', type=str, default='voc')
    p.add_argument('--class_num', type=int, default=20)
    p.add_argument('--pre_ckpt', type=str, default='None')
    p.add_argument('--model_def', type=str, default='yolo_mobilev2')
    p.add_argument('--depth_multiplier', type=float, choices=[0.5, 0.75, 1.0], default=1.0)
    p.add_argument('--augmenter', type=str, choices=['True', 'False'], default='False')
    p.add_argument('--image_size', type=int, default=(224, 320), nargs='+')
    p.add_argument('--output_size', type=int, default=(7, 10, 14, 20), nargs='+')
    p.add_argument('--batch_size', type=int, default=16)
    p.add_argument('--rand_seed', type=int, default=6)
    p.add_argument('--max_nrof_epochs', type=int, default=10)
    p.add_argument('--init_learning_rate', type=float, default=0.001)
    p.add_argument('--learning_rate_decay_factor', type=float, default=0)
    p.add_argument('--obj_weight', type=float, default=5.0)
    p.add_argument('--noobj_weight', type=float, default=0.5)
    p.add_argument('--wh_weight', type=float, default=0.5)
    p.add_argument('--obj_thresh', type=float, default=0.7)
    p.add_argument('--iou_thresh', type=float, default=0.3)
    p.add_argument('--vaildation_split', type=float, default=0.1)
    p.add_argument('--log_dir', type=str, default='log')
    p.add_argument('--is_prune', type=str, choices=['True', 'False'], default='False')
    p.add_argument('--prune_initial_sparsity', type=float, default=0.5)
    p.add_argument('--prune_final_sparsity', type=float, default=0.9)
    p.add_argument('--prune_end_epoch', type=int, default=5)
    p.add_argument('--prune_frequency', type=int, default=100)
    p.add_argument('--qat', type=str, choices=['True', 'False'], default='False', help='quantisation-aware fine-tuning (DESIGN.md 3.10)')
    p.add_argument('--qat_momentum', type=float, default=0.99, help='moving average of the activation ranges')
    p.add_argument('--qat_observe', type=int, default=8, help='batches of epoch 0 that only set the activation ranges')
    p.add_argument('--synthetic', type=int, default=0, help='train on N generated images instead of data/<set>_img_ann.npy')
    p.add_argument('--max_steps', type=int, default=0)
    p.add_argument('--val_map', type=str, choices=['True', 'False'], default='False', help='append val_mAP (VOC, on the GPU) to the epoch line')
    p.add_argument('--val_map_obj', type=float, default=0.05, help='objectness threshold of the detections val_mAP scores')
    p.add_argument('--box_loss', type=str, choices=['mse', 'giou', 'diou', 'ciou'], default='mse',
                   help='box regression term: the xy / wh terms of the reference, or an IoU-family loss (DESIGN.md 3.14)')
    p.add_argument('--box_weight', type=float, default=1.0, help='weight of the IoU box term (not used with --box_loss mse)')
    p.add_argument('--mosaic', type=str, choices=['True', 'False'], default='False',
                   help='compose every training sample of four pictures (DESIGN.md 3.15); validation is never mosaicked')
    p.add_argument('--mosaic_prob', type=float, default=1.0, help='share of the training samples that are mosaics')
    p.add_argument('--mosaic_off_epochs', type=int, default=0, help='the last N epochs train without mosaic')
    p.add_argument('--hsv', type=str, choices=['True', 'False'], default='False',
                   help='HSV colour jitter of every training frame (DESIGN.md 3.16); validation is never jittered')
    p.add_argument('--hsv_hue', type=float, default=0.1, help='largest hue rotation, in turns of the hue circle (0 to 0.5)')
    p.add_argument('--hsv_sat', type=float, default=1.5, help='largest saturation gain x (at least 1): gains between 1/x and x')
    p.add_argument('--hsv_exposure', type=float, default=1.5, help='largest exposure gain x (at least 1): gains between 1/x and x')
    p.add_argument('--hsv_prob', type=float, default=1.0, help='share of the training frames that are jittered')
    p.add_argument('--teacher_ckpt', type=str, default='', help='.h5 / .npz checkpoint of the teacher: knowledge distillation (DESIGN.md 3.18); empty = off')
    p.add_argument('--teacher_def', type=str, default=None, help="the teacher's network (default: --model_def)")
    p.add_argument('--teacher_depth', type=float, choices=[0.5, 0.75, 1.0], default=None, help="the teacher's depth multiplier (default: --depth_multiplier)")
    p.add_argument('--distill_weight', type=float, default=1.0, help='weight of the distillation term')
    p.add_argument('--cache', type=str, choices=['off', 'gpu'], default='off',
                   help='gpu: keep the decoded training pictures in device memory and compose every batch from there (DESIGN.md 3.19)')
    p.add_argument('--cache_gb', type=float, default=8, help='size of the picture cache; pictures that no longer fit are brought in every epoch')
    p.add_argument('--cache_stage_mb', type=float, default=256, help='size of one staging region: the uncached pictures of ONE batch must fit')
    p.add_argument('--decode', type=str, choices=['pil', 'gpu'], default='pil',
                   help='who decodes the training pictures: PIL on the thread pool, or (baseline JPEG files) the GPU, into the cache')
    p.add_argument('--ema', type=str, choices=['True', 'False'], default='False',
                   help='keep an exponential moving average of the weights; it is validated and saved as yolo_ema_model (DESIGN.md 3.21)')
    p.add_argument('--ema_decay', type=float, default=0.9999, help='decay of the weight average')
    p.add_argument('--ema_tau', type=float, default=2000.0, help='updates over which the decay ramps up: decay (1 - exp(-updates / tau)); 0 = no ramp')
    p.add_argument('--clip_norm', type=float, default=0.0, help='clip the global gradient norm to this value; 0 = off')
    p.add_argument('--lr_schedule', type=str, choices=['none', 'constant', 'cosine', 'step'], default='none',
                   help='learning-rate schedule over the whole run, from --init_learning_rate; none = Keras lr / (1 + decay t) as before')
    p.add_argument('--warmup_steps', type=int, default=0, help='linear warmup over the first N steps (with --lr_schedule)')
    p.add_argument('--lr_final', type=float, default=0.01, help='cosine: the last learning rate as a fraction of the first')
    p.add_argument('--focal', type=str, choices=['off', 'obj', 'cls', 'all'], default='off',
                   help='focal loss on the objectness (obj + noobj) and / or the class term (DESIGN.md 3.25)')
    p.add_argument('--focal_gamma', type=float, default=2.0, help='focal exponent: 0 or 1 to 5')
    p.add_argument('--focal_alpha', type=float, default=0.0, help='focal balance inside (0, 1); 0 = off')
    p.add_argument('--label_smooth', type=float, default=0.0, help='class targets z -> z (1 - eps) + eps / 2, eps in [0, 1); 0 = off')
    p.add_argument('--obj_target', type=str, choices=['label', 'iou'], default='label',
                   help="iou: an object cell's objectness target is the IoU of its predicted box with the label box")
    p.add_argument('--labels', type=str, choices=['host', 'gpu'], default='host',
                   help='gpu: the label grids are built on the GPU from the boxes, only the boxes cross PCIe (DESIGN.md 3.26)')
    p.add_argument('--assign', type=str, choices=['best', 'multi'], default='best',
                   help='multi: a box also trains every other (layer, anchor) that fits it better than --assign_iou (DESIGN.md 3.26)')
    p.add_argument('--assign_iou', type=float, default=0.213, help='with --assign multi: the fit above which an anchor is also trained on a box, inside (0, 1)')
    return p


def cli(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    return main(a, a.train_set, a.class_num, a.pre_ckpt, a.model_def, a.depth_multiplier, a.augmenter, a.image_size, a.output_size,
                a.batch_size, a.rand_seed, a.max_nrof_epochs, a.init_learning_rate, a.learning_rate_decay_factor, a.obj_weight,
                a.noobj_weight, a.wh_weight, a.obj_thresh, a.iou_thresh, a.vaildation_split, a.log_dir, a.is_prune,
                a.prune_initial_sparsity, a.prune_final_sparsity, a.prune_end_epoch, a.prune_frequency, a.synthetic, a.max_steps,
                a.qat, a.qat_momentum, a.qat_observe, a.val_map, a.val_map_obj, a.box_loss, a.box_weight, a.mosaic, a.mosaic_prob,
                a.mosaic_off_epochs, a.hsv, a.hsv_hue, a.hsv_sat, a.hsv_exposure, a.hsv_prob, a.teacher_ckpt, a.teacher_def, a.teacher_depth,
                a.distill_weight, a.cache, a.cache_gb, a.cache_stage_mb, a.decode, a.ema, a.ema_decay, a.ema_tau, a.clip_norm, a.lr_schedule,
                a.warmup_steps, a.lr_final, a.focal, a.focal_gamma, a.focal_alpha, a.label_smooth, a.obj_target, a.labels, a.assign, a.assign_iou)


if __name__ == '__main__':
    cli()
