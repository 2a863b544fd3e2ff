"""The layer loss with focal loss, label smoothing and the IoU objectness target (the rule is the header of
k210_yolo_framework_amd/lossopt.py) as ONE torch expression, differentiable in y_pred, in the dtype of y_pred, and the seeded inputs the CPU
and GPU tests share.  CPU only.

`layer_loss_torch` is tests/box_loss_ref.layer_loss_torch with three changes: the class targets are smoothed, the objectness target of an
object cell is the detached, clamped IoU of box_loss_ref's box term, and bce is replaced by fl(z, x) = a_t (1 - p_t)^gamma bce(z, x) where
focal says so, (1 - p_t) = z sigmoid(-x) + (1 - z) sigmoid(x) written as the rule writes it.  With every option off it IS box_loss_ref's."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

from tests import box_loss_ref as B

TERMS = B.TERMS
OFF = dict(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label')


def _term(z, x, on, gamma, alpha):
    bce = TF.binary_cross_entropy_with_logits(x, z, reduction='none')
    if not on:
        return bce
    m = z * torch.sigmoid(-x) + (1 - z) * torch.sigmoid(x)
    at = z * alpha + (1 - z) * (1 - alpha) if alpha > 0 else 1.0
    return at * (m ** gamma if gamma != 0 else 1.0) * bce


def layer_loss_torch(yt, yp, anchors, obj_thresh, iou_thresh, ow, nw, ww, batch_size, box_loss='mse', box_weight=1.0, focal='off',
                     focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label'):
    """-> (dict of the seven terms as 0-d tensors, ignore mask, objectness target [B,h,w,A])."""
    base, ign = B.layer_loss_torch(yt, yp, anchors, obj_thresh, iou_thresh, ow, nw, ww, batch_size, box_loss, box_weight)
    Bn, h, w, A, E = yp.shape
    dt = yp.dtype
    conf = yt[..., 4]
    ob = conf > obj_thresh
    zo = conf.clone()
    if obj_target == 'iou' and ob.any():
        anc = torch.as_tensor(np.asarray(anchors, np.float32)).to(dt)
        gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        off = torch.stack([gx, gy], -1)[:, :, None, :].to(dt)
        b = torch.cat([(torch.sigmoid(yp[..., 0:2]) + off) / torch.tensor([w, h]).to(dt), torch.exp(yp[..., 2:4]) * anc], -1)[ob]
        t = yt[..., 0:4][ob]
        ov = (torch.minimum(b[:, 0:2] + b[:, 2:4] / 2, t[:, 0:2] + t[:, 2:4] / 2) - torch.maximum(b[:, 0:2] - b[:, 2:4] / 2, t[:, 0:2] - t[:, 2:4] / 2)).clamp(min=0)
        inter = ov[:, 0] * ov[:, 1]
        zo[ob] = (inter / (b[:, 2] * b[:, 3] + t[:, 2] * t[:, 3] - inter + B.EPS)).clamp(0, 1).detach()
    bits = {'off': 0, 'obj': 1, 'cls': 2, 'all': 3}[focal]
    to = _term(zo, yp[..., 4], bits & 1, focal_gamma, focal_alpha)
    zc = yt[..., 5:] * (1 - label_smooth) + label_smooth / 2 if label_smooth else yt[..., 5:]
    tc = _term(zc, yp[..., 5:], bits & 2, focal_gamma, focal_alpha)
    ol = ow * (conf * to).sum() / batch_size
    nl = nw * ((1 - conf) * ign * to).sum() / batch_size
    cl = (conf[..., None] * tc).sum() / batch_size
    total = ol + nl + cl + base['xy'] + base['wh'] if box_loss == 'mse' else ol + nl + cl + base['box']
    return dict(total=total, xy=base['xy'], wh=base['wh'], obj=ol, noobj=nl, cls=cl, box=base['box']), ign, zo


def autograd(y_true, y_pred, anchors, obj_thresh=0.7, iou_thresh=0.5, ow=1.0, nw=1.0, ww=1.0, batch_size=None, box_loss='mse',
             box_weight=1.0, dtype=torch.float64, **opts):
    """-> (dict of the seven terms as floats, dL/dy_pred as float64 numpy, ignore mask, objectness target)."""
    yt = torch.from_numpy(np.asarray(y_true)).to(dtype)
    yp = torch.from_numpy(np.asarray(y_pred)).to(dtype).requires_grad_(True)
    terms, ign, zo = layer_loss_torch(yt, yp, anchors, obj_thresh, iou_thresh, ow, nw, ww, batch_size or yp.shape[0], box_loss, box_weight, **opts)
    terms['total'].backward()
    return {k: float(v.detach()) for k, v in terms.items()}, yp.grad.double().numpy(), ign.double().numpy(), zo.detach().double().numpy()


# ---- the option sets of the parity tests: focal obj / cls / all at gamma 2 and 1.5, alpha 0 and 0.25, eps 0.1, the IoU target, all three
OPTION_SETS = {
    'obj_g2': dict(focal='obj', focal_gamma=2.0),
    'cls_g2': dict(focal='cls', focal_gamma=2.0),
    'all_g2': dict(focal='all', focal_gamma=2.0),
    'obj_g1.5': dict(focal='obj', focal_gamma=1.5),
    'cls_g1.5_a': dict(focal='cls', focal_gamma=1.5, focal_alpha=0.25),
    'all_g1.5': dict(focal='all', focal_gamma=1.5),
    'all_g2_a': dict(focal='all', focal_gamma=2.0, focal_alpha=0.25),
    'smooth': dict(label_smooth=0.1),
    'iou': dict(obj_target='iou'),
    'all_three': dict(focal='all', focal_gamma=2.0, focal_alpha=0.25, label_smooth=0.1, obj_target='iou'),
    'all_three_g1.5': dict(focal='all', focal_gamma=1.5, label_smooth=0.1, obj_target='iou'),
}
BOX_MODES = ('mse', 'ciou')


def options(name):
    return dict(OFF, **OPTION_SETS[name])


# ---- every instance (tests/test_gpu_loss_instances.py).  csrc/yk_loss.hip compiles yolo_loss_kernel<MODE, OPT> for 27 sets of L_* bits in
# each of the four box modes; `instance_bits` restates loss_launch's rule from the options to the bits, and INSTANCE_SETS holds one option set
# per compiled OPT (alpha 0; gamma 1.5 sets L_POW), all-off left out: its instances are test_gpu_loss.py's and test_gpu_box_loss.py's.
L_FOBJ, L_FCLS, L_POW, L_SMOOTH, L_IOU = 1, 2, 4, 8, 16
BIT_NAMES = {L_FOBJ: 'L_FOBJ', L_FCLS: 'L_FCLS', L_POW: 'L_POW', L_SMOOTH: 'L_SMOOTH', L_IOU: 'L_IOU'}


def instance_bits(focal='off', focal_gamma=2.0, focal_alpha=0.0, label_smooth=0.0, obj_target='label'):
    """The OPT of the instance loss_launch picks: focal counts only with gamma or alpha away from 0, L_POW only beside a focal bit."""
    bits = 0
    if focal_gamma != 0 or focal_alpha != 0:
        bits |= {'off': 0, 'obj': L_FOBJ, 'cls': L_FCLS, 'all': L_FOBJ | L_FCLS}[focal]
        if bits and focal_gamma != 2:
            bits |= L_POW
    if label_smooth > 0:
        bits |= L_SMOOTH
    if obj_target == 'iou':
        bits |= L_IOU
    return bits


def _instance_sets():
    sets = {}
    for focal, gamma in (('off', 2.0),) + tuple((f, g) for f in ('obj', 'cls', 'all') for g in (2.0, 1.5)):
        for eps in (0.0, 0.1):
            for target in ('label', 'iou'):
                name = '+'.join([f'{focal}_g{gamma:g}'] * (focal != 'off') + ['smooth'] * (eps > 0) + ['iou'] * (target == 'iou'))
                if name:                                                 # (all-off has none)
                    sets[name] = dict(focal=focal, focal_gamma=gamma, label_smooth=eps, obj_target=target)
    return sets


INSTANCE_SETS = _instance_sets()
ALL_BOX_MODES = ('mse', 'giou', 'diou', 'ciou')
# the ends of what loss_launch accepts: gamma 1 (powf(m, 0)) and 5, gamma 0 with alpha (alpha-balanced bce through the L_POW instance), alpha
# and label_smooth near 1, gamma 1 beside the IoU target
EDGE_SETS = {
    'all_g1': dict(focal='all', focal_gamma=1.0),
    'all_g5': dict(focal='all', focal_gamma=5.0),
    'all_g0_a.25': dict(focal='all', focal_gamma=0.0, focal_alpha=0.25),
    'all_g1_a.75': dict(focal='all', focal_gamma=1.0, focal_alpha=0.75),
    'cls_g5_a.999_smooth.9': dict(focal='cls', focal_gamma=5.0, focal_alpha=0.999, label_smooth=0.9),
    'smooth.999': dict(label_smooth=0.999),
    'obj_g1+iou': dict(focal='obj', focal_gamma=1.0, obj_target='iou'),
}
SWEEP_SETS = dict(INSTANCE_SETS, **EDGE_SETS)
assert len(SWEEP_SETS) == len(INSTANCE_SETS) + len(EDGE_SETS)
# the smallest inputs on which each failure exists: batch_size != batch, an image without objects and garbage under conf 0; two chunks of
# blockIdx.y, the second of one box; box_loss_ref's four forced box relations (disjoint: the IoU target is exactly 0); logits of +-80
INSTANCE_CASES = ('head_7x10', 'p257', 'geometry')
EDGE_CASES = ('head_7x10', 'saturated')


def corner_case():
    """`geometry` with the disjoint cell's prediction moved to the label box's corner: 0.0125 and 0.02 clear of it in x and in y.  Both
    overlaps are negative and their product, 0.00025, is positive and smaller than the two areas (0.01 + 0.003): an IoU built on the
    overlaps before their clamp is 0.0196 here, where `geometry`'s own disjoint cell (product 0.0125, larger than the areas) gives a
    negative quotient that the clamp of the target hides.  -> (anchors, y_true, y_pred, keywords, the cell)."""
    anc, y_true, y_pred, cells = B.geometry_case()
    b, r, c, a = cells[0]
    y_pred = y_pred.copy()
    y_pred[b, r, c, a, 0:4] = (B._logit(0.5), B._logit(0.6), np.log(0.1 / anc[a, 0]), np.log(0.1 / anc[a, 1]))
    return anc, y_true, y_pred, parity_case('geometry')[3], cells[0]


@functools.lru_cache(maxsize=None)
def sweep_ref(case, box, oname, dtype=torch.float64):
    """`autograd` of a SWEEP_SETS entry on a parity case, computed once and shared: the arrays are not to be written to."""
    anc, y_true, y_pred, kw = parity_case(case)
    return autograd(y_true, y_pred, anc, box_loss=box, dtype=dtype, **kw, **SWEEP_SETS[oname])


# ---- the seeded inputs: box_loss_ref's one cell, 7x10 head with 20 classes, 255 / 256 / 257 predictions, and three of this file's
def wide_classes_case():
    """80 classes on a 3x3 grid, 2 images."""
    anc, y_true, y_pred = B.random_case(11, 2, 3, 3, 3, 80, n_obj=(2, 5))
    return anc, y_true, y_pred, dict(ow=1.0, nw=1.0, ww=1.0, batch_size=None, box_weight=1.0)


def full_case():
    """20x20 cells, 3 anchors, 1 class, 1 image, every cell an object: 1200 label boxes, more than the kernel keeps in LDS (1024)."""
    anc, y_true, y_pred = B.random_case(12, 1, 20, 20, 3, 1, n_obj=(1200, 1201))
    assert int((y_true[..., 4] > 0.7).sum()) == 1200
    return anc, y_true, y_pred, dict(ow=1.0, nw=0.5, ww=1.0, batch_size=None, box_weight=1.0)


def saturated_case():
    """p255 of box_loss_ref with objectness and class logits of +-80: in every image the first object cell and the first cell without one
    get +80, the second of each -80, on objectness and on both classes."""
    anc, y_true, y_pred, kw = B.parity_case('p255')
    y_pred = y_pred.copy()
    flat_t, flat_p = y_true.reshape(len(y_true), -1, y_true.shape[-1]), y_pred.reshape(len(y_pred), -1, y_pred.shape[-1])
    for b in range(len(flat_t)):
        ob = np.flatnonzero(flat_t[b, :, 4] > 0.7)
        no = np.flatnonzero(flat_t[b, :, 4] <= 0.7)
        for idx, v in ((ob[0], 80.0), (no[0], 80.0), (no[1], -80.0)) + (((ob[1], -80.0),) if len(ob) > 1 else ()):
            flat_p[b, idx, 4:] = v
    return anc, y_true, y_pred, kw


EXTRA_CASES = {'c80': wide_classes_case, 'full_20x20': full_case, 'saturated': saturated_case}
ALL_PARITY = tuple(B.PARITY_CASES) + tuple(EXTRA_CASES)


def parity_case(name):
    """-> (anchors, y_true, y_pred, keyword arguments of `autograd` but for box_loss and the options)."""
    return EXTRA_CASES[name]() if name in EXTRA_CASES else B.parity_case(name)


atol_needed = B.atol_needed

# The gradient tolerance of tests/test_gpu_loss_opt.py.  Entries 0..3 (the box) are not touched by the options and are held to the bits of
# the call without options.  Entries 4.. (objectness, classes): rtol 2e-5 as in tests/test_gpu_loss.py, and an absolute term that is measured:
# `autograd` evaluated in torch float32 on the CPU needs, against float64 at that rtol, the atol below on those entries (the largest over
# ALL_PARITY, OPTION_SETS and BOX_MODES: full_20x20 with the IoU target alone, whose float32 IoU is 8.4e-7 off and whose divisor is 1;
# tests/test_loss_opt_ref.py measures it again and holds it to this figure).  The kernel is another fp32 evaluation of the same expression
# with the GPU's expf / logf / powf, a few ulp from the host's, and is given four times that.
F32_ATOL_MEASURED = 1.361e-7
ATOL_FACTOR = 4
