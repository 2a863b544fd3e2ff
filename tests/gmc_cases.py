"""Generated pictures for the camera-motion tests (tests/test_gmc.py on the host, tests/test_gpu_gmc.py on the device): views of one seeded
noise canvas, so that a view moved by (dx, dy) shows the same content moved by exactly that."""
import numpy as np

H, W = 256, 448                           # small 64 x 112 at scale 4: 3 x 6 blocks of 16 at range 8, step 16
_CANVAS = np.random.default_rng(7).integers(0, 256, (H + 400, W + 400, 3), dtype=np.uint8)


def view(dx=0, dy=0, h=H, w=W):
    """The canvas seen through an h x w window; its content sits (dx, dy) further right / down than in view(0, 0)."""
    return np.ascontiguousarray(_CANVAS[200 - dy:200 - dy + h, 200 - dx:200 - dx + w])


def periodic(dx=0):
    """Period 16 in x (4 small pixels), random down the rows."""
    return np.ascontiguousarray(np.tile(_CANVAS[:H, :16], (1, (W + 32) // 16, 1))[:, 16 - dx:16 - dx + W])


def two_motions(a, b, split=288):
    """The left part moved by a, everything from column `split` (the last two of six block columns: a third of the blocks) by b."""
    out = view(*a)
    out[:, split:] = view(*b)[:, split:]
    return out


# name -> (the two frames, the motion the rule must give or None where only "not the shift" is known)
CONTENT = {
    'inside': ([view(), view(12, -8)], (12, -8)),
    'edge': ([view(), view(32, -32)], (32, -32)),
    'edge_negative': ([view(), view(-32, 32)], (-32, 32)),
    'beyond': ([view(), view(40, 0)], None),
    'flat': ([np.full((H, W, 3), 90, np.uint8)] * 2, (0, 0)),
    'period_4_ties': ([periodic(), periodic(8)], (-8, 0)),       # dx = -2 and +2 small pixels tie in SAD and |dx|: the smaller dx wins
    'a_third_moves_away': ([view(), two_motions((-8, 4), (16, 0))], (-8, 4)),
}
