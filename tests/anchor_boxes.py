"""Generated (w, h) boxes for the anchor k-means tests, and a <set>_img_ann.npy that holds them."""
import numpy as np

from k210_yolo_framework_amd import datatools


def boxes(n, seed):
    return np.clip(np.exp(np.random.default_rng(seed).normal(-1.6, 0.7, (n, 2))), 0.004, 1.0)


def write_ann(tmp_path, n_img=300, seed=0):
    """data/gen_img_ann.npy under tmp_path: network-sized pictures (the letterbox changes no box), 1 .. 3 generated boxes each.
    -> (data_dir, the [n, 2] boxes make_anchor_list clusters)."""
    x = boxes(3 * n_img, seed)
    rows = np.empty((n_img, 3), dtype=object)
    for i in range(n_img):
        wh = x[3 * i:3 * i + 1 + i % 3]
        rows[i, 0], rows[i, 1], rows[i, 2] = f'{i}.jpg', np.hstack([np.zeros((len(wh), 1)), np.full((len(wh), 2), 0.5), wh]), np.array([224, 320])
    (tmp_path / 'data').mkdir()
    np.save(tmp_path / 'data' / 'gen_img_ann.npy', rows, allow_pickle=True)
    return str(tmp_path / 'data'), datatools.letterbox_boxes(rows, (224, 320))
