"""The training input pipeline: what tools/utils.py:417-450 builds with tf.data -

    Dataset.from_tensor_slices(list).shuffle().map(py_function(read + letterbox + box_to_label), num_parallel_calls=AUTOTUNE)
           .batch(batch_size, drop_remainder=True).prefetch(AUTOTUNE)

- rebuilt so that it can feed the HIP training step (2.5 k images/s/GPU) instead of starving it:

  * every rank decodes ONLY ITS SHARE of the global batch: the epoch order is one permutation drawn from the shared seed, global batch g
    is order[g*GB:(g+1)*GB], rank r takes rows [r*per, (r+1)*per) of it (round 2 built the whole global batch on every rank and sliced);
  * file decode (`Helper._read_img`, PIL releases the GIL) and label scatter (`Helper.box_to_label`) run on a small thread pool;
  * the letterbox (tools/utils.py:378-399) and `img / np.max(img)` (:405) run on the GPU - `yk_letterbox_u8` (bit-exact against
    scikit-image, tests/golden/letterbox_golden.npz) and `yk_normalise_u8` - on a side stream, frames travel as u8 (a quarter of the
    float bytes) from pinned buffers;
  * a producer thread keeps `prefetch` batches ahead of the consumer (`.prefetch`); the consumer gets device tensors whose producing
    stream it must wait on (`batch.ready` is a recorded event; `__iter__` does the wait for the current stream).

Images of one batch may have different sizes (VOC): they are letterboxed in groups of equal size.

augment=True adds the training augmentation (the imgaug OneOf of utils.py:84-88; semantics in augment.py): each row's parameters
come from the epoch's table (seed, epoch, row), the letterboxed boxes are augmented before `batch_box_to_label`, the per-image
inverse maps [n, 6] travel through a pinned slot like the labels, and each size group is letterboxed AND warped by one
`yk_letterbox_augment_u8` launch (no intermediate frame).  `yk_normalise_u8` then divides by the augmented image's own maximum, as
utils.py:405 does.

mosaic=MosaicConfig(prob) composes every sample of four pictures (semantics in mosaic.py): the producer decodes the batch's own rows and
their partners on the pool, each picture once however often the batch names it, packs them into ONE pinned buffer (draw.pack_ragged),
copies it with the table, the seams and - with augment=True - the inverse maps, and ONE `yk_mosaic_ragged_u8` launch writes the whole
batch, pictures of any sizes, warped or not.  Every rank computes the partners from the epoch's shared table.  Without mosaic the path
above runs untouched.

hsv=HsvConfig(hue, sat, exposure, prob) jitters the colours of every finished frame (semantics in colour.py): the batch's (dh, gs, gv)
rows of the epoch's table travel through a pinned slot, and ONE `yk_hsv_jitter_u8` launch works in place on the u8 frames of the whole
batch, on either path above, between the geometric launch and `yk_normalise_u8`.  Without hsv no call is added.

cache=PictureCache(...) (cache.py) keeps every decoded picture on the device: a batch resolves its rows, brings the pictures
the cache does not hold into its arena - decoded by the pool and copied (decode='pil'), or, baseline JPEG files, only read and parsed by the
pool and decoded there by ONE `yk_jpeg_decode_ragged_u8` (decode='gpu'; without a cache it runs on a staging ring of its own) - and ONE
ragged launch over the arena writes the whole batch, plain, warped or mosaicked; hsv, normalise and labels follow as above.  The batches are
those of the paths above, bit for bit.  Without cache and with decode='pil' the paths above run untouched.

labels='gpu'  builds the label grids on the device: letterboxing, augmentation and mosaic of the BOXES stay on the host in
float64 (a few hundred numbers), the batch's boxes [N, 5] and offsets [n + 1] travel through two pinned slots instead of the dense grids, and
ONE `yk_boxes_to_labels_f32` launch writes every layer's grid into one flat buffer - `Helper.batch_box_to_label`'s bits.  Where numpy would
raise or wrap (a centre cell outside its grid) the kernel writes nothing of the box and says so in a status word, which comes home to a
pinned int32 and is read once the batch's `ready` event has completed, at the latest when the epoch ends: the producer then raises, naming
the dataset row and the box; rows that are not finite are refused before upload.  assign='multi', assign_iou (Helper.box_to_label): a box
is also written at every other (layer, anchor) that fits it better than assign_iou, under either value of `labels`.  With labels='host',
assign='best' (the defaults) every path above runs untouched.
"""
from __future__ import annotations

import collections
import io
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np

from . import augment as aug_mod
from . import colour as colour_mod
from . import engine
from . import mosaic as mosaic_mod
from .helper import Helper


def epoch_order(n_items: int, seed: int, epoch: int, shuffle: bool) -> np.ndarray:
    """The epoch's sample order, identical on every rank (shared seed)."""
    return np.random.default_rng([seed, epoch]).permutation(n_items) if shuffle else np.arange(n_items)


def rank_rows(order: np.ndarray, global_batch: int, rank: int, world: int) -> List[np.ndarray]:
    """Per step: the dataset rows THIS rank decodes (drop_remainder=True, utils.py:447)."""
    if global_batch % world:
        raise ValueError(f'global batch {global_batch} must divide by {world} ranks')
    per = global_batch // world
    return [order[s + rank * per: s + (rank + 1) * per] for s in range(0, len(order) - global_batch + 1, global_batch)]


def letterbox_boxes(h: Helper, img_hw, boxes: np.ndarray) -> np.ndarray:
    """The box half of Helper._process_img (utils.py:386-389): centre / size fractions of the source image -> of the network tensor."""
    boxes = np.array(boxes, np.float64, copy=True)
    if boxes.size:
        scale, translation = h.letterbox_params(img_hw)
        src_wh, net_wh = np.tile(np.array(img_hw[::-1], float), 2), np.tile(h.in_hw[0][::-1].astype(float), 2)
        moved = boxes[:, 1:5] * src_wh * np.tile(scale, 2)
        moved[:, :2] += translation
        boxes[:, 1:5] = moved / net_wh
    return boxes


def letterbox_boxes_batch(h: Helper, img_hws, boxes_list) -> List[np.ndarray]:
    """`letterbox_boxes` for every sample of a batch with one pass of array arithmetic (same element-wise operations in the same order:
    bit-identical), the letterbox parameters computed once per distinct image size."""
    per = [np.array(b, np.float64, copy=True).reshape(-1, 5) for b in boxes_list]
    counts = [len(b) for b in per]
    if sum(counts) == 0:
        return per
    params = {}
    for hw in img_hws:
        if tuple(hw) not in params:
            scale, translation = h.letterbox_params(hw)
            params[tuple(hw)] = (np.tile(np.array(hw[::-1], float), 2), np.tile(scale, 2), np.asarray(translation, float))
    allb = np.concatenate(per)
    src = np.repeat(np.stack([params[tuple(hw)][0] for hw in img_hws]), counts, axis=0)
    sc = np.repeat(np.stack([params[tuple(hw)][1] for hw in img_hws]), counts, axis=0)
    tr = np.repeat(np.stack([params[tuple(hw)][2] for hw in img_hws]), counts, axis=0)
    moved = allb[:, 1:5] * src * sc
    moved[:, :2] += tr
    allb[:, 1:5] = moved / np.tile(h.in_hw[0][::-1].astype(float), 2)
    return np.split(allb, np.cumsum(counts)[:-1])


class Batch:
    __slots__ = ('x', 'labels', 'ready', 'n')

    def __init__(self, x, labels, ready, n):
        self.x, self.labels, self.ready, self.n = x, labels, ready, n


# Pinned host staging buffers, shared by the epochs' pipelines of a process (allocating pinned memory per batch costs more than the
# batch).  Keyed by CAPACITY BUCKET, not by shape: real VOC lists hold hundreds of image sizes and the count of every size varies from
# batch to batch - a ring per exact (count, h, w) would pin a new buffer for nearly every batch and never give it back.  A request takes
# a reshaped view of the prefix of a power-of-two sized byte buffer; the total is capped and the least recently used ring is released.
_PINNED: "dict" = {}          # (device, what, bucket bytes) -> {'ring': [[pinned uint8 tensor, event of its last H2D copy], ...], 'tick': last use}
_PINNED_CAP_BYTES = 1 << 30   # upper bound of page-locked staging memory per process
_pinned_clock = 0
_pinned_lock = threading.Lock()


def _bucket(nbytes: int) -> int:
    return 1 << max(12, (int(nbytes) - 1).bit_length())


def pinned_bytes() -> int:
    return sum(sl[0].numel() for e in _PINNED.values() for sl in e['ring'])


def _evict(keep_key, need: int) -> None:
    """Release least recently used rings (never `keep_key`) until `need` more bytes fit under the cap."""
    while _PINNED and pinned_bytes() + need > _PINNED_CAP_BYTES:
        victims = [k for k in _PINNED if k != keep_key]
        if not victims:
            return
        k = min(victims, key=lambda kk: _PINNED[kk]['tick'])
        for sl in _PINNED[k]['ring']:
            if sl[1] is not None:
                sl[1].synchronize()
        del _PINNED[k]


class InputPipeline:
    """Iterable over one epoch: yields (x [per_rank,H,W,3] float32 cuda, [labels per layer, float32 cuda])."""

    def __init__(self, h: Helper, items: Sequence, global_batch: int, rank: int = 0, world: int = 1, seed: int = 0, epoch: int = 0,
                 shuffle: bool = True, workers: int = 8, prefetch: int = 2, device: Optional[int] = None, augment: bool = False,
                 mosaic: Optional[mosaic_mod.MosaicConfig] = None, hsv: Optional[colour_mod.HsvConfig] = None, cache=None,
                 decode: str = 'pil', labels: str = 'host', assign: str = 'best', assign_iou: float = 0.213):
        import torch
        engine.require_gpu()
        if decode not in ('pil', 'gpu'):
            raise engine.YkError(f'InputPipeline: decode {decode!r}: expected pil or gpu')
        if labels not in ('host', 'gpu'):
            raise engine.YkError(f'InputPipeline: labels {labels!r}: expected host or gpu')
        try:
            Helper.check_assign(assign, assign_iou)
        except ValueError as e:
            raise engine.YkError(f'InputPipeline: {e}') from e
        self.labels, self.assign, self.assign_iou = labels, assign, float(assign_iou)
        self.h, self.items = h, items
        self.hsv_table = colour_mod.param_table(seed, epoch, len(items), hsv) if hsv is not None else None       # [n_rows, 3], rank-independent
        self.mosaic = mosaic
        self.mosaic_table = mosaic_mod.param_table(seed, epoch, len(items)) if mosaic is not None else None      # rank-independent too
        self.table = aug_mod.param_table(seed, epoch, len(items)) if augment else None       # per (seed, epoch, row): rank-independent
        self.rows = rank_rows(epoch_order(len(items), seed, epoch, shuffle), global_batch, rank, world)
        self.per = global_batch // world
        self.dev = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.q: "queue.Queue" = queue.Queue(maxsize=max(1, prefetch))
        self.stream = torch.cuda.Stream(device=self.dev)
        self.images = 0
        self.seconds = 0.0
        self._thread = None
        self._stop = False
        # labels='gpu': the grids are built on the device from the boxes (yk_boxes_to_labels_f32); every batch's status word comes home
        # to its own pinned int32 and is read once the batch's `ready` event has completed, at the latest when the epoch ends
        self._in_flight: "collections.deque" = collections.deque()
        self._batches = 0
        if labels == 'gpu':
            self._label_cfg = engine.make_label_cfg(h, assign, assign_iou)
            self._status_home = torch.full((max(1, len(self.rows)),), engine.LABEL_STATUS_CLEAN, dtype=torch.int32).pin_memory()
        # cache=PictureCache (cache.py) and / or decode='gpu': every batch is composed from the cache's arena by one launch
        self.decode = decode
        self._own_cache = None
        if cache is None and decode == 'gpu':                                   # staging only
            from .cache import PictureCache
            cache = self._own_cache = PictureCache(0, prefetch=self.q.maxsize, device=self.dev.index)
        self.cache = cache
        if cache is not None:
            if cache.arena is None or cache.device != self.dev:
                raise engine.YkError(f'InputPipeline: the picture cache lives on {cache.device}, the pipeline runs on {self.dev}')
            if cache.ring < self.q.maxsize + 2:
                raise engine.YkError(f'InputPipeline: prefetch {self.q.maxsize} needs a picture cache with {self.q.maxsize + 2} staging '
                                     f'regions, this one has {cache.ring}')

    def __len__(self):
        return len(self.rows)

    # one image on a worker thread (file decode releases the GIL; arrays already in memory are taken as they are)
    def _image(self, i: int):
        img = self.items[int(i)][0]
        if isinstance(img, (str, os.PathLike)):
            img = self.h._read_img(str(img))
        return np.ascontiguousarray(img[..., :3], np.uint8)

    def _slot(self, key, shape, dtype):
        """[view of a pinned host staging buffer shaped `shape`, its slot] from a small ring per capacity bucket."""
        import torch
        global _pinned_clock
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        bk = _bucket(nbytes)
        k = (self.dev.index, key, bk)
        with _pinned_lock:
            _pinned_clock += 1
            e = _PINNED.setdefault(k, {'ring': [], 'tick': 0})
            e['tick'] = _pinned_clock
            ring = e['ring']
            nslots = self.q.maxsize + 2                                     # more than the batches that can be outstanding
            if len(ring) < nslots:
                _evict(k, bk)
                ring.append([torch.empty((bk,), dtype=torch.uint8).pin_memory(), None])
                slot = ring[-1]
            else:
                slot = ring[self._tick % nslots]
        if slot[1] is not None:
            slot[1].synchronize()                                           # its last H2D copy has left the buffer
        return slot[0][:nbytes].view(dtype).view(tuple(shape)), slot

    def _produce(self):
        import torch
        H, W = int(self.h.in_hw[0][0]), int(self.h.in_hw[0][1])
        self._tick = 0
        self._batches = 0                                                       # (a second pass over the same pipeline starts its status words afresh)
        self._in_flight.clear()
        if self.labels == 'gpu':
            self.stream.synchronize()                                           # no status word of an abandoned pass is still on its way home
            self._status_home.fill_(engine.LABEL_STATUS_CLEAN)
        try:
            for rows in self.rows:
                if self._stop:
                    break
                self._check_labels(wait=False)
                t0 = time.perf_counter()
                if self.cache is not None or self.mosaic is not None:
                    batch = self._cached_batch(rows, H, W) if self.cache is not None else self._mosaic_batch(rows, H, W)
                    self.images += batch.n
                    self.seconds += time.perf_counter() - t0
                    if not self._put(batch):
                        return
                    continue
                # decode on the pool only when there is something to decode: for rows that are arrays already the pool's hand-off
                # costs more than it buys (threads of numpy work share the GIL: 1.9 vs 1.4 ms per 16 samples)
                from_files = isinstance(self.items[int(rows[0])][0], (str, os.PathLike))
                imgs = list(self.pool.map(self._image, rows)) if from_files else [self._image(i) for i in rows]
                n = len(imgs)
                self._tick += 1
                # labels of the whole batch in a handful of array operations (utils.py:207-230 on the letterboxed boxes), then ONE copy per
                # layer into the pinned staging buffer (pinned memory is slow to write piecemeal from the CPU)
                boxes = letterbox_boxes_batch(self.h, [im.shape[:2] for im in imgs], [self.items[int(i)][1] for i in rows])
                by_size = {}
                for k, img in enumerate(imgs):
                    by_size.setdefault(img.shape[:2], []).append(k)
                inv_slot = None
                if self.table is not None:
                    A, t, M = aug_mod.matrices(self.table[rows], (H, W))
                    boxes = aug_mod.augment_boxes_batch(boxes, A, t, (H, W))
                    # the inverse maps in size-group order: group g reads a contiguous run of rows
                    inv_slot = self._slot('inv', (n, 6), torch.float64)
                    inv_slot[0].numpy()[...] = M.reshape(n, 6)[np.concatenate(list(by_size.values()))]
                staged = self._stage_labels(boxes, rows)
                with torch.cuda.stream(self.stream):
                    frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.dev)
                    if inv_slot is not None:
                        inv = inv_slot[0].to(self.dev, non_blocking=True)
                        inv_slot[1][1] = torch.cuda.Event()
                        inv_slot[1][1].record(self.stream)
                    first = 0
                    for (sh, sw), idx in by_size.items():                   # equal-sized images are letterboxed in one launch
                        view, slot = self._slot('img', (len(idx), sh, sw, 3), torch.uint8)
                        hv = view.numpy()
                        for j, k in enumerate(idx):
                            hv[j] = imgs[k]
                        src = view.to(self.dev, non_blocking=True)
                        slot[1] = torch.cuda.Event()
                        slot[1].record(self.stream)
                        if inv_slot is None:
                            out = engine.letterbox_u8(src, (H, W), stream=self.stream)
                        else:
                            out = engine.letterbox_augment_u8(src, (H, W), inv[first:first + len(idx)], stream=self.stream)
                        first += len(idx)
                        if len(by_size) == 1:
                            frames = out
                        else:
                            frames[torch.as_tensor(idx, device=self.dev)] = out
                    if self.hsv_table is not None:                          # the frames are in batch order again: one launch, in place
                        engine.hsv_jitter_u8(frames, self._upload('hsv', self.hsv_table[rows], torch.float64), stream=self.stream)
                    x = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.dev)
                    engine.call('yk_normalise_u8', frames, n, H * W * 3, x, engine._stream(self.stream))
                    labels, ready = self._send_labels(staged)
                self.images += n
                self.seconds += time.perf_counter() - t0
                if not self._put(Batch(x, labels, ready, n)):
                    return
            self._check_labels(wait=not self._stop)
        except BaseException as e:                                         # surface worker errors in the consumer
            self._put(e)
            return
        self._put(None)

    def _upload(self, key, array, dtype):
        """A host array through a pinned slot to the device, on the producer's stream (call inside `torch.cuda.stream(self.stream)`)."""
        import torch
        view, slot = self._slot(key, array.shape, dtype)
        view.numpy()[...] = array
        dev = view.to(self.dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(self.stream)
        return dev

    # ---- labels: the one place the three batch builders get them from ---------------------------------------------------------------
    def _stage_labels(self, boxes, rows):
        """The host half, before anything is queued.  labels='host': the dense grids (Helper.batch_box_to_label) written into pinned
        slots, one per layer.  labels='gpu': the batch's boxes as one [N, 5] float64 array and its offsets [n + 1]; rows that are not
        finite are refused here, naming the dataset row."""
        import torch
        if self.labels == 'host':
            labs = self.h.batch_box_to_label(boxes, self.assign, self.assign_iou)
            lab_slots = [self._slot(('lab', l), labs[l].shape, torch.float32) for l in range(len(labs))]
            for (view, _), lab in zip(lab_slots, labs):
                view.numpy()[...] = lab
            return lab_slots
        per = [np.asarray(b, np.float64).reshape(-1, 5) for b in boxes]
        first = np.zeros(len(per) + 1, np.int32)
        np.cumsum([len(b) for b in per], out=first[1:])
        allb = np.concatenate(per) if first[-1] else np.zeros((0, 5), np.float64)
        if not np.isfinite(allb).all():
            raise engine.YkError(self._box_message(int(np.nonzero(~np.isfinite(allb).all(1))[0][0]), rows, first, allb, 'is not finite'))
        return allb, first, np.array(rows, np.int64, copy=True)

    def _send_labels(self, staged):
        """The device half, inside `torch.cuda.stream(self.stream)`, last of the batch: -> (labels per layer, the batch's `ready` event).
        labels='host': one copy per layer from the pinned slots.  labels='gpu': boxes and offsets through `_upload`, ONE
        yk_boxes_to_labels_f32 launch, and the status word on its way to its pinned home - read once `ready` has completed."""
        import torch
        if self.labels == 'host':
            labels = []
            for view, slot in staged:
                labels.append(view.to(self.dev, non_blocking=True))
                slot[1] = torch.cuda.Event()
                slot[1].record(self.stream)
            ready = torch.cuda.Event()
            ready.record(self.stream)
            return labels, ready
        allb, first, rows = staged
        d_boxes = self._upload('lbox', allb, torch.float64)
        d_first = self._upload('lfirst', first, torch.int32)
        labels, status = engine.boxes_to_labels(d_boxes, d_first, self._label_cfg, stream=self.stream)
        home = self._status_home[self._batches:self._batches + 1]
        home.copy_(status, non_blocking=True)
        self._batches += 1
        ready = torch.cuda.Event()
        ready.record(self.stream)
        self._in_flight.append((ready, status, home, rows, first, allb))
        return labels, ready

    def _box_message(self, g: int, rows, first, allb, what: str) -> str:
        s = int(np.searchsorted(first, g, side='right')) - 1
        return (f'InputPipeline(labels=\'gpu\'): dataset row {int(rows[s])} (sample {s} of its batch), box {g - int(first[s])} of the sample, '
                f'(cls, x, y, w, h) = {tuple(float(v) for v in allb[g])} {what}')

    def _check_labels(self, wait: bool) -> None:
        """Read the status words of the batches whose `ready` event has completed (wait: of all of them, waiting for each): a box that
        numpy could not have written either - a centre cell outside a grid it is written to, a class outside [0, class_num) - raises."""
        while self._in_flight:
            ready, _, home, rows, first, allb = self._in_flight[0]
            if wait:
                ready.synchronize()
            elif not ready.query():
                return
            self._in_flight.popleft()
            g = int(home[0])
            if g != engine.LABEL_STATUS_CLEAN:
                raise engine.YkError(self._box_message(g, rows, first, allb, 'has a centre cell outside the label grid of a layer it is written '
                                                       'to (or a class outside [0, class_num)): Helper.batch_box_to_label raises or wraps there'))

    def _mosaic_batch(self, rows, H: int, W: int) -> Batch:
        """One batch of mosaics (mosaic.py): decode each picture the batch names once, one packed pinned buffer, one launch."""
        import torch
        from .draw import RAGGED_DTYPE, pack_ragged
        n = len(rows)
        self._tick += 1
        members, _ = mosaic_mod.members(rows, self.mosaic_table, (H, W), self.mosaic.prob)
        uniq = [int(i) for i in np.unique(members)]
        from_files = any(isinstance(self.items[i][0], (str, os.PathLike)) for i in uniq)
        imgs = dict(zip(uniq, self.pool.map(self._image, uniq) if from_files else [self._image(i) for i in uniq]))
        quads, centres, boxes = mosaic_mod.plan(rows, self.mosaic_table, lambda i: imgs[i].shape[:2], (H, W),
                                                boxes_of=lambda i: self.items[i][1], prob=self.mosaic.prob)
        M = None
        if self.table is not None:
            A, t, M = aug_mod.matrices(self.table[rows], (H, W))
            boxes = aug_mod.augment_boxes_batch(boxes, A, t, (H, W))
        staged = self._stage_labels(boxes, rows)
        total = sum(im.size for im in imgs.values())
        view, slot = self._slot('mosaic', (total,), torch.uint8)
        _, ptable, _ = pack_ragged([imgs[i] for i in uniq], out=view)
        offsets = {i: int(o) for i, o in zip(uniq, ptable['offset'])}
        table = engine.check_ragged_rows(mosaic_mod.ragged_rows(quads, offsets.__getitem__), total)
        with torch.cuda.stream(self.stream):
            packed = view.to(self.dev, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(self.stream)
            d_table = self._upload('mtab', table.view(np.uint8).reshape(len(table), RAGGED_DTYPE.itemsize), torch.uint8)
            d_centres = self._upload('mcen', np.ascontiguousarray(centres, np.int32), torch.int32)
            inv = None if M is None else self._upload('inv', M.reshape(n, 6), torch.float64)
            frames = engine.mosaic_ragged_u8(packed, d_table, d_centres, (H, W), inv=inv, stream=self.stream)
            if self.hsv_table is not None:
                engine.hsv_jitter_u8(frames, self._upload('hsv', self.hsv_table[rows], torch.float64), stream=self.stream)
            x = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.dev)
            engine.call('yk_normalise_u8', frames, n, H * W * 3, x, engine._stream(self.stream))
            labels, ready = self._send_labels(staged)
        return Batch(x, labels, ready, n)

    # ---- cache= / decode='gpu': the batch is composed from the arena of cache.py -------------------------------------------------
    def _load(self, i: int):
        """decode='gpu', a row that is not cached, on a worker thread: -> a jpeg.Baseline (the file read and parsed: the device decodes
        it), or pixels - an array of the list, or a file the parser refuses (progressive, PNG ...), decoded by PIL as detect.py does."""
        from . import jpeg
        img = self.items[int(i)][0]
        if not isinstance(img, (str, os.PathLike)):
            return np.ascontiguousarray(img[..., :3], np.uint8)
        with open(img, 'rb') as f:
            data = f.read()
        try:
            return jpeg.parse_baseline(data)
        except jpeg.Unsupported:
            return np.ascontiguousarray(self.h._read_img(io.BytesIO(data))[..., :3], np.uint8)

    def _copy_run(self, key, run, plan, got):
        """The pictures of `run`, one contiguous run of `plan`, through ONE pinned slot to their arena offsets: one copy."""
        import torch
        if not run:
            return
        start = plan.table[run[0]][0]
        end = plan.table[run[-1]][0] + got[run[-1]].size
        view, slot = self._slot(key, (end - start,), torch.uint8)
        flat = view.numpy()
        for i in run:
            o = plan.table[i][0] - start
            flat[o:o + got[i].size] = got[i].reshape(-1)
        self.cache.arena[start:end].copy_(view, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(self.stream)

    def _decode_into_arena(self, jp, plan, got):
        """The parsed files of rows `jp`: their scans and tables cross PCIe and ONE yk_jpeg_decode_ragged_u8 writes the pictures at their
        arena offsets.  -> the rows whose stream did not decode, with their status (waits for the decode: only batches with misses pay)."""
        import torch
        from . import jpeg
        from .draw import RAGGED_DTYPE
        if not jp:
            return []
        parsed = [got[i] for i in jp]
        jbytes = sum((len(p.scan) + jpeg.SCAN_PAD + 3) // 4 * 4 for p in parsed) + len(jp) * jpeg.PIC_TABLE_BYTES
        view, slot = self._slot('jscan', (jbytes,), torch.uint8)
        _, pics, scan_bytes, table_bytes = jpeg.plan_decode(parsed, out=view.numpy())
        d_buf = view.to(self.dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(self.stream)
        rows = np.zeros(len(jp), RAGGED_DTYPE)
        for k, i in enumerate(jp):
            rows[k]['offset'], rows[k]['h'], rows[k]['w'] = plan.table[i]
        rows = engine.check_ragged_rows(rows, self.cache.arena_bytes)
        d_pics = self._upload('jpics', pics.view(np.uint8).reshape(len(jp), jpeg.PIC_DTYPE.itemsize), torch.uint8)
        d_rows = self._upload('jrows', rows.view(np.uint8).reshape(len(jp), RAGGED_DTYPE.itemsize), torch.uint8)
        status = engine.jpeg_decode_ragged_u8(d_buf[:scan_bytes], d_pics, d_buf[scan_bytes:scan_bytes + table_bytes], d_rows, self.cache.arena,
                                              stream=self.stream, work_bytes=engine.jpeg_decode_workspace_bytes(pics))
        return [(i, code) for i, code in zip(jp, status.cpu().tolist()) if code]

    def _cached_batch(self, rows, H: int, W: int) -> Batch:
        """One batch from the picture cache: resolve the rows, bring the misses into the arena (each distinct picture once), ONE geometric
        launch over the arena - yk_letterbox_ragged_u8 for plain samples, yk_mosaic_ragged_u8 for mosaics and, each sample four times its
        own plain letterbox row, for augmented plain samples (bit for bit yk_letterbox_augment_u8: include/yolo_hip.h) - then HSV,
        normalise and labels as on the other paths."""
        import torch
        from .draw import RAGGED_DTYPE
        cache = self.cache
        rows = np.asarray(rows, np.int64).reshape(-1)
        n = len(rows)
        self._tick += 1
        if self.mosaic is not None:
            uniq = [int(i) for i in np.unique(mosaic_mod.members(rows, self.mosaic_table, (H, W), self.mosaic.prob)[0])]
        else:
            uniq = [int(i) for i in np.unique(rows)]
        known = cache.lookup(uniq)
        missing = [i for i in uniq if i not in known]
        load = self._load if self.decode == 'gpu' else self._image
        from_files = any(isinstance(self.items[i][0], (str, os.PathLike)) for i in missing)
        got = dict(zip(missing, self.pool.map(load, missing) if from_files else [load(i) for i in missing]))
        raw = [i for i in missing if isinstance(got[i], np.ndarray)]            # pixels on the host: copied in
        jp = [i for i in missing if not isinstance(got[i], np.ndarray)]         # parsed files: decoded in
        region = cache.acquire() if missing else None
        try:
            # copied pictures first: the copied part of the admissions is one run of the persistent part, that of the staged one of the region
            plan = cache.plan(raw + jp + sorted(known), lambda i: got[i].shape[:2] if i in raw else (got[i].h, got[i].w), region or 0)
            hw_of = lambda i: plan.table[int(i)][1:]
            M = centres = None
            if self.mosaic is not None:
                quads, centres, boxes = mosaic_mod.plan(rows, self.mosaic_table, hw_of, (H, W), boxes_of=lambda i: self.items[i][1],
                                                        prob=self.mosaic.prob)
            else:
                boxes = letterbox_boxes_batch(self.h, [hw_of(i) for i in rows], [self.items[int(i)][1] for i in rows])
            if self.table is not None:
                A, t, M = aug_mod.matrices(self.table[rows], (H, W))
                boxes = aug_mod.augment_boxes_batch(boxes, A, t, (H, W))
            if self.mosaic is None and M is not None:                           # four times the sample's own plain letterbox row
                quads = np.zeros((n, 4), mosaic_mod.ROW_DTYPE)
                for b, i in enumerate(rows):
                    quads[b, :] = (int(i), *hw_of(i), *mosaic_mod.letterbox_params(hw_of(i), (H, W)))
                centres = np.zeros((n, 2), np.int32)
            if centres is not None:
                table = mosaic_mod.ragged_rows(quads, lambda i: plan.table[i][0])
            else:
                table = np.zeros(n, RAGGED_DTYPE)
                for b, i in enumerate(rows):
                    table[b]['offset'], table[b]['h'], table[b]['w'] = plan.table[int(i)]
                engine.call('yk_letterbox_ragged_params', table, n, H, W)
            table = engine.check_ragged_rows(table, cache.arena_bytes)
            staged = self._stage_labels(boxes, rows)
            with torch.cuda.stream(self.stream):
                written = cache.last_write()
                if written is not None:                                         # (a pipeline of an earlier epoch wrote on its own stream)
                    self.stream.wait_event(written)
                if missing:
                    self._copy_run('cadm', [i for i in plan.admitted if i in raw], plan, got)
                    self._copy_run('cstg', [i for i in plan.staged if i in raw], plan, got)
                    failed = self._decode_into_arena(jp, plan, got)
                    behind = torch.cuda.Event()
                    behind.record(self.stream)
                    cache.commit(plan, [i for i, _ in failed], behind)
                    if failed:
                        i, code = failed[0]
                        raise engine.YkError(f'{self.items[i][0]}: the JPEG stream does not decode (status {code}: yk_jpeg_decode_ragged_u8)')
                else:
                    cache.commit(plan)
                d_table = self._upload('mtab', table.view(np.uint8).reshape(len(table), RAGGED_DTYPE.itemsize), torch.uint8)
                if centres is not None:
                    d_centres = self._upload('mcen', np.ascontiguousarray(centres, np.int32), torch.int32)
                    inv = None if M is None else self._upload('inv', M.reshape(n, 6), torch.float64)
                    frames = engine.mosaic_ragged_u8(cache.arena, d_table, d_centres, (H, W), inv=inv, stream=self.stream)
                else:
                    frames = engine.letterbox_ragged_u8(cache.arena, d_table, (H, W), stream=self.stream)
        finally:
            if region is not None:                                              # the region is free once everything queued so far has run
                done = torch.cuda.Event()
                done.record(self.stream)
                cache.release(region, done)
        with torch.cuda.stream(self.stream):
            if self.hsv_table is not None:
                engine.hsv_jitter_u8(frames, self._upload('hsv', self.hsv_table[rows], torch.float64), stream=self.stream)
            x = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.dev)
            engine.call('yk_normalise_u8', frames, n, H * W * 3, x, engine._stream(self.stream))
            labels, ready = self._send_labels(staged)
        return Batch(x, labels, ready, n)

    def _put(self, item) -> bool:
        """queue.put that gives up when the consumer has gone away (close() after an early break): never blocks forever."""
        while not self._stop:
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def __iter__(self):
        import torch
        self._stop = False
        self._thread = threading.Thread(target=self._produce, daemon=True)
        self._thread.start()
        while True:
            b = self.q.get()
            if b is None:
                break
            if isinstance(b, BaseException):
                raise b
            cur = torch.cuda.current_stream()
            cur.wait_event(b.ready)
            # the tensors were allocated on the producer's side stream and are consumed on this one: tell the caching allocator, or a
            # block could go back to the producer while kernels queued here still read it
            b.x.record_stream(cur)
            for t in b.labels:
                t.record_stream(cur)
            yield b.x, b.labels
        self._thread.join()

    def close(self):
        """Stop the producer and wait for it: drains the queue until the thread has exited (it may be blocked in put), then the pool."""
        self._stop = True
        t = self._thread
        while t is not None and t.is_alive():
            try:
                while True:
                    self.q.get_nowait()
            except queue.Empty:
                pass
            t.join(timeout=0.05)
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
        self._thread = None
        self.pool.shutdown(wait=True)
        if self._own_cache is not None:
            self._own_cache.close()
            self._own_cache = self.cache = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def producer_images_per_sec(self) -> float:
        """Rate of the producer alone (decode + labels + H2D + GPU letterbox / normalise), not limited by the consumer."""
        return self.images / self.seconds if self.seconds else 0.0
