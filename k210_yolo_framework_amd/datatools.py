"""Offline dataset tools of the reference (row N3): `make_voc_list.py` and `make_anchor_list.py`.  numpy on the host; the anchor k-means
also runs on the GPU (`run_kmeans_gpu`, csrc/yk_kmeans.hip), many random starts in one call, with the numpy functions as its statement.

  make_voc_list.py:9-26     image list -> data/<set>_img_ann.npy rows [path, boxes[n,5] (cls,x,y,w,h), (h,w)]
  make_anchor_list.py:176-218  letterbox the boxes to the network frame, k-means on (w,h) under the centred-IoU
                               distance 1 - IoU (:10-39), 10 iterations (the reference passes a literal 10 at :207, not
                               --max_iters), centroids sorted by descending w, reshaped to [layers, anchors, 2]

The reference evaluates the distance in a TF-1 session; it is plain float64 arithmetic, restated here with numpy."""
from __future__ import annotations

import os
import re
from typing import Sequence

import numpy as np


def make_voc_list(train_file: str, output_file: str) -> np.ndarray:
    """train_file: one image path per line; labels sit beside them with JPEGImages->labels, .jpg->.txt."""
    from PIL import Image
    paths = [str(p) for p in np.atleast_1d(np.loadtxt(train_file, dtype=str))]
    rows = np.empty((len(paths), 3), dtype=object)
    for i, p in enumerate(paths):
        ann = re.sub(r'.jpg', '.txt', re.sub(r'JPEGImages', 'labels', p))
        with Image.open(p) as im:
            hw = np.array([im.height, im.width])
        rows[i, 0], rows[i, 1], rows[i, 2] = p, np.loadtxt(ann, dtype=float, ndmin=2), hw
    os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
    np.save(output_file, rows, allow_pickle=True)
    return rows


def fake_iou_distance(x: np.ndarray, centroids: np.ndarray) -> np.ndarray:
    """make_anchor_list.py:10-39: boxes centred at the origin, [m,2] vs [k,2] -> 1 - IoU, [m,k]."""
    x, c = x[:, None, :], centroids[None, :, :]
    wh = np.maximum(np.minimum(x / 2., c / 2.) - np.maximum(-x / 2., -c / 2.), 0.)
    inter = wh[..., 0] * wh[..., 1]
    return 1 - inter / (x[..., 0] * x[..., 1] + c[..., 0] * c[..., 1] - inter)


def run_kmeans(x: np.ndarray, initial_centroids: np.ndarray, iters: int = 10):
    """make_anchor_list.py:143-173 (empty clusters give NaN centroids, which the caller reports like the reference)."""
    c = np.array(initial_centroids, np.float64)
    idx = np.zeros(len(x), np.int64)
    for _ in range(iters):
        idx = np.argmin(fake_iou_distance(x, c), axis=1)
        with np.errstate(invalid='ignore'), np.testing.suppress_warnings() as sup:
            sup.filter(RuntimeWarning)
            c = np.stack([x[idx == i].mean(axis=0) if (idx == i).any() else np.full(x.shape[1], np.nan) for i in range(len(c))])
    return c, idx


def letterbox_boxes(rows: np.ndarray, in_hw: Sequence[int]) -> np.ndarray:
    """make_anchor_list.py:181-193: every annotation mapped into the network frame; returns all (w,h) stacked."""
    in_wh = np.array(in_hw[::-1], np.float64)
    out = []
    for r in rows:
        box = np.array(r[1], np.float64, copy=True)
        img_wh = np.array(r[2][::-1], np.float64)
        scale = in_wh / img_wh
        scale[:] = np.min(scale)
        translation = ((in_wh - img_wh * scale) / 2).astype(int)
        box[:, 1:3] = (box[:, 1:3] * img_wh * scale + translation) / in_wh
        box[:, 3:5] = (box[:, 3:5] * img_wh * scale) / in_wh
        out.append(box)
    return np.vstack(out)[:, 3:]


def _as_inits(inits) -> np.ndarray:
    inits = np.array(inits, np.float64, order='C')            # (a copy: C-contiguous and writable, whatever came in)
    if inits.ndim == 2:
        inits = inits[None]
    if inits.ndim != 3 or inits.shape[2] != 2 or not inits.shape[0] or not inits.shape[1]:
        raise ValueError(f'inits of shape {inits.shape}: [R, k, 2] or [k, 2] wanted')
    return inits


def _as_boxes(x) -> np.ndarray:
    x = np.array(x, np.float64, order='C')
    if x.ndim != 2 or x.shape[1] != 2 or not len(x):
        raise ValueError(f'x of shape {x.shape}: [n, 2] wanted, n >= 1')
    if not (np.isfinite(x) & (x > 0)).all():
        raise ValueError('x holds a box whose w or h is not finite or not positive (its distance to a centroid would be 0 / 0)')
    return x


def run_kmeans_gpu(x: np.ndarray, inits: np.ndarray, iters: int = 10, return_counts: bool = False):
    """`run_kmeans` for every one of the R starts `inits` [R, k, 2] (or [k, 2]: R = 1) in one call on the GPU (csrc/yk_kmeans.hip;
    DESIGN.md 3.13) -> (centroids [R, k, 2], idx [R, n] uint8, score [R], empty [R]) and, with `return_counts`, counts [R, k].
    score = the mean over the boxes of the best IoU against the returned centroids.  A start that loses a cluster at iteration i stops
    there: empty = i + 1 (else 0), that centroid row and the score are NaN.  Raises engine.YkError without a device: there is no fallback."""
    import ctypes as C
    from . import engine                    # lazily: this module imports without torch and without a device
    x, inits = _as_boxes(x), _as_inits(inits)
    if np.isnan(inits).any():
        raise ValueError('inits holds a NaN')
    engine.require_gpu()
    import torch
    (R, k, _), n = inits.shape, len(x)
    nbytes = C.c_size_t()
    engine.call('yk_anchor_kmeans_workspace_bytes', n, k, R, C.byref(nbytes))
    dev = torch.device('cuda', torch.cuda.current_device())
    d_x, d_c = torch.from_numpy(x).to(dev), torch.from_numpy(inits).to(dev)
    d_counts = torch.empty((R, k), dtype=torch.int32, device=dev)
    d_empty = torch.empty((R,), dtype=torch.int32, device=dev)
    d_score = torch.empty((R,), dtype=torch.float64, device=dev)
    d_idx = torch.empty((R, n), dtype=torch.uint8, device=dev)
    work = torch.empty((int(nbytes.value),), dtype=torch.uint8, device=dev)
    engine.call('yk_anchor_kmeans_f64', d_x, n, d_c, k, R, int(iters), d_c, d_counts, d_score, d_empty, d_idx, work, nbytes.value,
                engine._stream())
    torch.cuda.current_stream().synchronize()
    out = (d_c.cpu().numpy(), d_idx.cpu().numpy(), d_score.cpu().numpy(), d_empty.cpu().numpy())
    return out + (d_counts.cpu().numpy(),) if return_counts else out


def mean_best_iou(x: np.ndarray, centroids: np.ndarray) -> float:
    """The figure the YOLO papers judge anchors by: the mean over the boxes of the IoU with the closest centroid."""
    return float(np.mean(1 - fake_iou_distance(x, centroids).min(axis=1)))


def run_kmeans_restarts(x: np.ndarray, inits: np.ndarray, iters: int = 10, device: str = 'cpu'):
    """Every start of `inits` [R, k, 2] -> (centroids [R, k, 2], score [R], empty [R]) as `run_kmeans_gpu` defines them.  device 'cpu'
    loops `run_kmeans` one iteration at a time (the same centroids as one call of `iters` iterations) and stops a start at the iteration
    that empties a cluster: the numpy statement of what device 'gpu' computes."""
    if device == 'gpu':
        c, _, score, empty = run_kmeans_gpu(x, inits, iters)
        return c, score, empty
    if device != 'cpu':
        raise ValueError(f"device {device!r}: 'cpu' or 'gpu'")
    x, inits = _as_boxes(x), _as_inits(inits)
    out, score, empty = np.empty_like(inits), np.full(len(inits), np.nan), np.zeros(len(inits), np.int32)
    for r, c in enumerate(inits):
        for it in range(iters):
            c, _ = run_kmeans(x, c, 1)
            if np.isnan(c).any():
                empty[r] = it + 1
                break
        out[r] = c
        if not empty[r]:
            score[r] = mean_best_iou(x, c)
    return out, score, empty


def anchor_inits(k: int, restarts: int = 1, is_random: bool = False, low=(0., 0.), high=(1., 1.), seed=None) -> np.ndarray:
    """[restarts, k, 2] initial centroids.  Start 0 is the reference's: the linspace pair, or with `is_random` the first draw of
    default_rng(seed) (w column, then h column); every further start is the next such draw of the same generator."""
    rng = np.random.default_rng(seed)
    draw = lambda: np.hstack((rng.uniform(low[0], high[0], (k, 1)), rng.uniform(low[1], high[1], (k, 1))))
    first = draw() if is_random else np.vstack((np.linspace(0.05, 0.3, num=k), np.linspace(0.05, 0.5, num=k))).T
    return np.stack([first] + [draw() for _ in range(restarts - 1)])


def select_anchors(centroids: np.ndarray, score: np.ndarray, empty: np.ndarray):
    """-> (best_r, centroids[best_r]): the highest score among the starts that kept every cluster, the lowest r on a tie.  If every
    start lost one: (0, the NaN set of start 0)."""
    valid = np.flatnonzero(np.asarray(empty) == 0)
    if not len(valid):
        return 0, centroids[0]
    best = int(valid[np.argmax(np.asarray(score)[valid])])               # np.argmax: the first of equal maxima
    return best, centroids[best]


def make_anchor_list(train_set: str, in_hw=(224, 320), out_hw=(7, 10, 14, 20), anchor_num: int = 3, is_random: bool = False,
                     low=(0., 0.), high=(1., 1.), seed=None, data_dir: str = 'data', save: bool = True, device: str = 'cpu',
                     restarts: int = 1) -> np.ndarray:
    """device 'cpu', restarts 1: the reference's single run.  Otherwise `restarts` starts (anchor_inits) are run, on the GPU in one
    call with device 'gpu', and the set with the highest mean IoU over the boxes among the starts that kept every cluster is taken."""
    if device not in ('cpu', 'gpu'):
        raise ValueError(f"device {device!r}: 'cpu' or 'gpu'")
    if restarts < 1:
        raise ValueError(f'restarts = {restarts}: at least 1')
    rows = np.load(os.path.join(data_dir, f'{train_set}_img_ann.npy'), allow_pickle=True)
    x = letterbox_boxes(rows, in_hw)
    layers = len(out_hw) // 2
    k = layers * anchor_num
    inits = anchor_inits(k, restarts, is_random, low, high, seed)
    if device == 'cpu' and restarts == 1:
        centroids, _ = run_kmeans(x, inits[0], 10)
    else:
        sets, score, empty = run_kmeans_restarts(x, inits, 10, device)
        best, centroids = select_anchors(sets, score, empty)
        valid = score[empty == 0]
        if restarts > 1 and len(valid):
            print(f'mean IoU {score[best]:.6f} (of {len(valid)}/{restarts} starts; worst {valid.min():.6f})')
    centroids = np.array(sorted(centroids, key=lambda v: -v[0])).reshape(layers, anchor_num, 2)
    if np.any(np.isnan(centroids)):
        print('[ERROR] Result have NaN value please Rerun!')
    elif save:
        np.save(os.path.join(data_dir, f'{train_set}_anchor.npy'), centroids)
    return centroids
