"""Generate tests/golden/region_live_golden.npz by RUNNING THE REFERENCE's region_layer.c on the cases of
tests/test_oracle_region.py::test_live_reference_bit_exact, and on the saturating boxes of tests/region_cases.py (infinite widths, zero heights:
the reference's own draw casts see +-inf) for ::test_live_reference_saturating_boxes.

Requires oracle/_ref/libregion_ref.so (oracle/build_ref.sh, needs the reference tree).
The fixture holds only data: per case and input scale, the seeded input, the anchors and the reference's outputs
(rl->output, rl->boxes, rl->probs after NMS, and the ordered draw-callback list).
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402
from tests import region_cases  # noqa: E402

# (W, H, A, C, thr, nms, net) - the parameters of test_live_reference_bit_exact
CASES = [
    (10, 7, 3, 20, 0.6, 0.3, (320, 224)), (20, 14, 3, 20, 0.1, 0.3, (320, 224)),
    (13, 13, 3, 20, 0.2, 0.5, (416, 416)), (5, 3, 5, 2, 0.05, 0.2, (160, 224)), (1, 1, 1, 1, 0.0, 0.5, (320, 224)),
    (20, 14, 3, 1, 0.3, 0.3, (320, 224)),
]
SCALES = (6.0, 2.0)


def case_key(W, H, A, C, thr, nms, net):
    return f'{W}x{H}x{A}x{C}_{thr}_{nms}_{net[0]}x{net[1]}'


def main():
    assert oracle.have_ref(), 'run oracle/build_ref.sh first (needs the reference tree)'
    out = {}
    for W, H, A, C, thr, nms, net in CASES:
        key = case_key(W, H, A, C, thr, nms, net)
        rng = np.random.default_rng(W * 1000 + H * 10 + C)
        anchor = rng.uniform(0.05, 0.9, 2 * A).astype(np.float32)
        out[key + '/anchor'] = anchor
        for scale in SCALES:
            x = rng.uniform(-scale, scale, (A, 5 + C, H, W)).astype(np.float32)
            o, b, p, d = oracle.ref_region_run(x, anchor, W, H, A, C, thr, nms, net)
            k = f'{key}/s{scale:g}'
            out[k + '/input'] = x
            out[k + '/output'] = o
            out[k + '/boxes'] = b
            out[k + '/probs'] = p
            out[k + '/dets'] = d
            print(k, 'dets', len(d))
    c = region_cases.saturating()
    B, W, H, A, C = region_cases.dims(c)
    assert B == 1 and c.image_wh == (320, 224)      # the reference hard-codes the image size
    o, b, p, d = oracle.ref_region_run(c.x[0], c.anchor, W, H, A, C, c.thr, c.nms, c.net_wh)
    for name, a in (('input', c.x[0]), ('anchor', c.anchor), ('output', o), ('boxes', b), ('probs', p), ('dets', d)):
        out[f'{c.name}/{name}'] = a
    print(c.name, 'dets', len(d), 'infinite box fields', int(np.isinf(b).sum()))
    np.savez_compressed(Path(__file__).with_name('region_live_golden.npz'), **out)


if __name__ == '__main__':
    main()
