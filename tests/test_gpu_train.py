"""GPU parity of the training step against oracle/train_ref.py (torch-CPU float64 autograd).

Tolerances (fp32 HIP vs float64 reference): kernels 1e-4 relative to the tensor's max magnitude (fp32 sums over up to
1e5 terms); whole-step gradients 2e-3 of each tensor's max (≈60 layers of fp32 BatchNorm/ReLU chains); loss 1e-4."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from k210_yolo_framework_amd import netspec as ns
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from oracle import train_ref
from tests import train_cases
from tests.mini_net import residual_zoo_spec

pytestmark = pytest.mark.gpu


def _lib():
    from k210_yolo_framework_amd import engine
    engine.require_gpu()
    return engine, engine.lib()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _close(got, ref, tol=1e-4):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref).max()
    assert err <= tol * max(1e-6, np.abs(ref).max()), (err, np.abs(ref).max())


@pytest.mark.parametrize('tA,tB,M,N,K', [(0, 1, 300, 75, 96), (0, 0, 257, 130, 65), (1, 0, 48, 33, 20000), (1, 1, 17, 19, 23),
                                        (0, 1, 1, 1, 300000), (0, 1, 4480, 96, 16)])
def test_gemm_all_layouts_and_split_k(tA, tB, M, N, K):
    engine, L = _lib()
    rng = np.random.default_rng(M + N + K)
    A = rng.normal(size=(K, M) if tA else (M, K)).astype(np.float32)
    Bm = rng.normal(size=(N, K) if tB else (K, N)).astype(np.float32)
    C0 = rng.normal(size=(M, N)).astype(np.float32)
    ref = 0.5 * ((A.T if tA else A).astype(np.float64) @ (Bm.T if tB else Bm).astype(np.float64)) + 2.0 * C0
    a, b, c = _cu(A), _cu(Bm), _cu(C0)
    assert L.yk_gemm_f32(tA, tB, M, N, K, C.c_float(0.5), engine._ptr(a), A.shape[1], engine._ptr(b), Bm.shape[1], C.c_float(2.0),
                         engine._ptr(c), N, _st()) == 0
    _close(c.cpu().numpy(), ref, 2e-5)


@pytest.mark.parametrize('tA,tB', [(1, 0), (0, 1), (0, 0)])
def test_grouped_gemms_equal_the_separate_calls(tA, tB):
    """yk_gemm_f32_grouped: many independent problems in one grid (+ one launch for all the K-slice sums), K slices sized for the group: equal to
    the separate calls within 2e-5 of the result's magnitude, and bitwise reproducible call to call.  Shapes of the weight gradients of a
    backward pass: one-tile results over 70 000 rows (512 slices, the 16-lane sum), mid-size ones (a few slices, the plain sum), unsplit ones,
    a shape without 16-byte rows (falls back to its own launch), and more problems than one group holds."""
    engine, L = _lib()
    rng = np.random.default_rng(7 + tA * 2 + tB)
    shapes = [(96, 16, 70000), (16, 96, 70000), (144, 24, 17920), (320, 960, 1120), (24, 144, 4480), (75, 128, 1120), (64, 64, 64), (130, 36, 300)]
    shapes = shapes + [(8 + 4 * (i % 5), 12 + 4 * (i % 3), 2000 + 400 * i) for i in range(40)]       # 48 problems: two groups
    if not tA:
        shapes = [(k if k < 5000 else 4480, n, m) for (m, n, k) in shapes]                         # keep M*K moderate for the row-major A layouts
    As, Bs, Cs, refs, C0s = [], [], [], [], []
    for (M, N, K) in shapes:
        A = rng.normal(size=(K, M) if tA else (M, K)).astype(np.float32)
        Bm = rng.normal(size=(N, K) if tB else (K, N)).astype(np.float32)
        C0 = rng.normal(size=(M, N)).astype(np.float32)
        a, b, c = _cu(A), _cu(Bm), _cu(C0)
        ref = c.clone()
        assert L.yk_gemm_f32(tA, tB, M, N, K, C.c_float(0.5), engine._ptr(a), A.shape[1], engine._ptr(b), Bm.shape[1], C.c_float(2.0),
                             engine._ptr(ref), N, _st()) == 0
        As.append(a); Bs.append(b); Cs.append(c); refs.append(ref); C0s.append(c.clone())
    n = len(shapes)
    ia = lambda v: (C.c_int * n)(*v)
    pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    assert L.yk_gemm_f32_grouped(n, tA, tB, ia([s[0] for s in shapes]), ia([s[1] for s in shapes]), ia([s[2] for s in shapes]), C.c_float(0.5), pa(As),
                                 ia([a.shape[1] for a in As]), pa(Bs), ia([b.shape[1] for b in Bs]), C.c_float(2.0), pa(Cs), ia([s[1] for s in shapes]),
                                 _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    for k, (c, r) in enumerate(zip(Cs, refs)):
        _close(c.cpu().numpy(), r.cpu().numpy(), 2e-5)
    first = [c.clone() for c in Cs]
    for c, c0 in zip(Cs, C0s):                                   # (beta = 2 reads C: restore the inputs, run again, compare bit for bit)
        c.copy_(c0)
    assert L.yk_gemm_f32_grouped(n, tA, tB, ia([s[0] for s in shapes]), ia([s[1] for s in shapes]), ia([s[2] for s in shapes]), C.c_float(0.5), pa(As),
                                 ia([a.shape[1] for a in As]), pa(Bs), ia([b.shape[1] for b in Bs]), C.c_float(2.0), pa(Cs), ia([s[1] for s in shapes]),
                                 _st()) == 0
    torch.cuda.synchronize()
    for k, (c, r) in enumerate(zip(Cs, first)):
        assert torch.equal(c, r), (k, shapes[k])
    assert L.yk_gemm_f32_grouped(0, tA, tB, None, None, None, C.c_float(1), None, None, None, None, C.c_float(0), None, None, _st()) == 0


@pytest.mark.parametrize('stride,pad', [(1, (1, 1)), (2, (1, 1)), (2, (1, 0))])
def test_conv3x3_im2col_gemm_and_adjoint(stride, pad):
    engine, L = _lib()
    rng = np.random.default_rng(stride)
    B, Hi, Wi, Ci, Co = 3, 13, 18, 7, 10
    pt, pl = pad[0], pad[0]
    pb = pr = pad[1]
    Ho, Wo = (Hi + pt + pb - 3) // stride + 1, (Wi + pl + pr - 3) // stride + 1
    x = rng.normal(size=(B, Hi, Wi, Ci)).astype(np.float32)
    w = rng.normal(size=(3, 3, Ci, Co)).astype(np.float32)
    dy = rng.normal(size=(B, Ho, Wo, Co)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt.permute(3, 2, 0, 1), stride=stride)
    yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    M, KK = B * Ho * Wo, 9 * Ci
    geom = [C.c_int(v) for v in (B, Hi, Wi, Ci, Ho, Wo, stride, pt, pl)]
    xd, dyd = _cu(x), _cu(dy)
    wd = _cu(np.transpose(w, (3, 0, 1, 2)).reshape(Co, KK))
    col = torch.empty(M, KK, device='cuda')
    assert L.yk_im2col3x3_f32(engine._ptr(xd), *geom, engine._ptr(col), _st()) == 0
    y = torch.empty(M, Co, device='cuda')
    assert L.yk_gemm_f32(0, 1, M, Co, KK, C.c_float(1), engine._ptr(col), KK, engine._ptr(wd), KK, C.c_float(0), engine._ptr(y), Co, _st()) == 0
    _close(y.cpu().numpy().reshape(B, Ho, Wo, Co), yt.detach().permute(0, 2, 3, 1).numpy())
    gw = torch.empty(Co, KK, device='cuda')
    assert L.yk_gemm_f32(1, 0, Co, KK, M, C.c_float(1), engine._ptr(dyd), Co, engine._ptr(col), KK, C.c_float(0), engine._ptr(gw), KK, _st()) == 0
    _close(np.transpose(gw.cpu().numpy().reshape(Co, 3, 3, Ci), (1, 2, 3, 0)), wt.grad.numpy())
    assert L.yk_gemm_f32(0, 0, M, KK, Co, C.c_float(1), engine._ptr(dyd), Co, engine._ptr(wd), KK, C.c_float(0), engine._ptr(col), KK, _st()) == 0
    dx = torch.empty(B, Hi, Wi, Ci, device='cuda')
    assert L.yk_col2im3x3_f32(engine._ptr(col), *geom, engine._ptr(dx), _st()) == 0
    _close(dx.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize('stride,pad,B,Hi,Wi,Ci,Co', [(1, (1, 1), 3, 13, 18, 8, 12), (2, (1, 1), 2, 15, 22, 12, 20), (2, (1, 0), 2, 14, 20, 4, 8),
                                                     (1, (1, 1), 16, 7, 10, 64, 36), (1, (1, 1), 4, 14, 20, 48, 16)])
def test_conv3x3_implicit_gemm_forward_and_gradients(stride, pad, B, Hi, Wi, Ci, Co):
    """The 3x3 convolution without the column matrix (yk_conv3x3_*): against float64 autograd, and forward / weight gradient bit for bit against
    im2col + yk_gemm_f32 (same order of additions); with BatchNorm the fused call equals conv + yk_bn_train_fwd_res_f32."""
    engine, L = _lib()
    rng = np.random.default_rng(stride + Ci)
    pt, pl = pad[0], pad[0]
    pb = pr = pad[1]
    Ho, Wo = (Hi + pt + pb - 3) // stride + 1, (Wi + pl + pr - 3) // stride + 1
    x = rng.normal(size=(B, Hi, Wi, Ci)).astype(np.float32)
    w = rng.normal(size=(3, 3, Ci, Co)).astype(np.float32)
    dy = rng.normal(size=(B, Ho, Wo, Co)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt.permute(3, 2, 0, 1), stride=stride)
    yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    M, KK = B * Ho * Wo, 9 * Ci
    geom = [C.c_int(v) for v in (B, Hi, Wi, Ci, Ho, Wo, stride, pt, pl)]
    xd, dyd = _cu(x), _cu(dy)
    wd = _cu(np.transpose(w, (3, 0, 1, 2)).reshape(Co, KK))
    nobn = [None, None, C.c_float(0), 0, C.c_float(0), None, None, None, None, None, C.c_float(0), None]
    z = torch.empty(M, Co, device='cuda')
    assert L.yk_conv3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *geom, Co, engine._ptr(z), *nobn, _st()) == 0, L.yk_last_error()
    _close(z.cpu().numpy().reshape(B, Ho, Wo, Co), yt.detach().permute(0, 2, 3, 1).numpy())
    col = torch.empty(M, KK, device='cuda')
    assert L.yk_im2col3x3_f32(engine._ptr(xd), *geom, engine._ptr(col), _st()) == 0
    z2 = torch.empty(M, Co, device='cuda')
    assert L.yk_gemm_f32(0, 1, M, Co, KK, C.c_float(1), engine._ptr(col), KK, engine._ptr(wd), KK, C.c_float(0), engine._ptr(z2), Co, _st()) == 0
    assert torch.equal(z, z2)
    if Co % 4 == 0:
        gw, gw2 = torch.empty(Co, KK, device='cuda'), torch.empty(Co, KK, device='cuda')
        assert L.yk_conv3x3_bwd_weight_f32(engine._ptr(xd), engine._ptr(dyd), *geom, Co, engine._ptr(gw), _st()) == 0, L.yk_last_error()
        assert L.yk_gemm_f32(1, 0, Co, KK, M, C.c_float(1), engine._ptr(dyd), Co, engine._ptr(col), KK, C.c_float(0), engine._ptr(gw2), KK, _st()) == 0
        _close(np.transpose(gw.cpu().numpy().reshape(Co, 3, 3, Ci), (1, 2, 3, 0)), wt.grad.numpy())
        assert torch.equal(gw, gw2)
        dx = torch.empty(B, Hi, Wi, Ci, device='cuda')
        rc = L.yk_conv3x3_bwd_data_f32(engine._ptr(dyd), engine._ptr(wd), *geom, Co, engine._ptr(dx), _st())
        if stride == 1:
            assert rc == 0, L.yk_last_error()
            _close(dx.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy())
        else:
            assert rc != 0 and b'stride' in L.yk_last_error()
    # with BatchNorm: the fused call against conv + the separate BatchNorm call
    gamma, beta = _cu(rng.uniform(0.5, 2, Co)), _cu(rng.normal(size=Co))
    outs = []
    for fused in (False, True):
        zz, y = torch.empty(M, Co, device='cuda'), torch.empty(M, Co, device='cuda')
        sm, si = torch.empty(Co, device='cuda'), torch.empty(Co, device='cuda')
        mm, mv = torch.zeros(Co, device='cuda'), torch.ones(Co, device='cuda')
        bn = (engine._ptr(gamma), engine._ptr(beta), C.c_float(1e-3), ns.ACT_LEAKY, C.c_float(0.1), engine._ptr(y), engine._ptr(sm), engine._ptr(si),
              engine._ptr(mm), engine._ptr(mv), C.c_float(0.99), None, _st())
        if fused:
            assert L.yk_conv3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *geom, Co, engine._ptr(zz), *bn) == 0, L.yk_last_error()
        else:
            zz.copy_(z)
            assert L.yk_bn_train_fwd_res_f32(engine._ptr(zz), C.c_longlong(M), Co, *bn) == 0
        outs.append([t.cpu().numpy() for t in (zz, y, sm, si, mm, mv)])
    a, b = outs
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[2:], b[2:]):
        _close(v, u, 1e-6)
    assert np.abs(a[1] - b[1]).max() <= 1e-5 * np.abs(a[1]).max()
    # a 3-channel input and a tensor off the 16-byte grid are refused as unsupported (the im2col path covers them); host checks, no launch
    YK_ERR_UNSUPPORTED = -12                                                  # include/yolo_hip.h
    assert L.yk_conv3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), B, Hi, Wi, 3, Ho, Wo, stride, pt, pl, Co, engine._ptr(z), *nobn,
                                   _st()) == YK_ERR_UNSUPPORTED
    assert L.yk_conv3x3_bn_fwd_f32(C.c_void_p(xd.data_ptr() + 4), engine._ptr(wd), *geom, Co, engine._ptr(z), *nobn, _st()) == YK_ERR_UNSUPPORTED


@pytest.mark.parametrize('stride', [1, 2])
def test_depthwise_forward_and_both_gradients(stride):
    engine, L = _lib()
    rng = np.random.default_rng(10 + stride)
    B, Hi, Wi, Cc = 4, 15, 22, 72
    Ho, Wo = (Hi + 2 - 3) // stride + 1, (Wi + 2 - 3) // stride + 1
    x = rng.normal(size=(B, Hi, Wi, Cc)).astype(np.float32)
    w = rng.normal(size=(3, 3, Cc)).astype(np.float32)
    dy = rng.normal(size=(B, Ho, Wo, Cc)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    yt = F.conv2d(F.pad(xt, (1, 1, 1, 1)), wt.permute(2, 0, 1)[:, None], stride=stride, groups=Cc)
    yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    geom = [C.c_int(v) for v in (B, Hi, Wi, Cc, Ho, Wo, stride, 1, 1)]
    xd, wd, dyd = _cu(x), _cu(w.reshape(9, Cc)), _cu(dy)
    y, dx, dw = torch.empty(B, Ho, Wo, Cc, device='cuda'), torch.empty(B, Hi, Wi, Cc, device='cuda'), torch.empty(9, Cc, device='cuda')
    assert L.yk_dw3x3_fwd_f32(engine._ptr(xd), engine._ptr(wd), *geom, engine._ptr(y), _st()) == 0
    assert L.yk_dw3x3_bwd_data_f32(engine._ptr(dyd), engine._ptr(wd), *geom, engine._ptr(dx), _st()) == 0
    assert L.yk_dw3x3_bwd_weight_f32(engine._ptr(xd), engine._ptr(dyd), *geom, engine._ptr(dw), _st()) == 0
    _close(y.cpu().numpy(), yt.detach().permute(0, 2, 3, 1).numpy())
    _close(dx.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy())
    _close(dw.cpu().numpy().reshape(3, 3, Cc), wt.grad.numpy())


def test_grouped_depthwise_weight_gradients_equal_the_separate_calls_bitwise():
    engine, L = _lib()
    rng = np.random.default_rng(3)
    cases = [(4, 15, 22, 72, 1), (2, 56, 80, 24, 2), (3, 14, 20, 130, 1), (16, 7, 10, 960, 1), (2, 28, 40, 32, 2)] + [(2, 9 + i, 11, 8 + 4 * i, 1 + i % 2) for i in range(35)]
    xs, dys, refs, outs, geo = [], [], [], [], []
    for (B, Hi, Wi, Cc, stride) in cases:
        Ho, Wo = (Hi + 2 - 3) // stride + 1, (Wi + 2 - 3) // stride + 1
        x, dy = _cu(rng.normal(size=(B, Hi, Wi, Cc))), _cu(rng.normal(size=(B, Ho, Wo, Cc)))
        g = (B, Hi, Wi, Cc, Ho, Wo, stride, 1, 1)
        ref = torch.empty(9, Cc, device='cuda')
        assert L.yk_dw3x3_bwd_weight_f32(engine._ptr(x), engine._ptr(dy), *[C.c_int(v) for v in g], engine._ptr(ref), _st()) == 0
        xs.append(x); dys.append(dy); refs.append(ref); outs.append(torch.zeros(9, Cc, device='cuda')); geo += list(g)
    n = len(cases)
    pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    assert L.yk_dw3x3_bwd_weight_grouped_f32(n, pa(xs), pa(dys), (C.c_int * (9 * n))(*geo), pa(outs), _st()) == 0, L.yk_last_error()
    torch.cuda.synchronize()
    for k, (o, r) in enumerate(zip(outs, refs)):
        assert torch.equal(o, r), (k, cases[k])


@pytest.mark.parametrize('act,alpha,M,Cc', [(ns.ACT_NONE, 0.0, 1000, 24), (ns.ACT_RELU, 0.0, 4097, 96), (ns.ACT_RELU6, 6.0, 700, 130),
                                           (ns.ACT_LEAKY, 0.1, 70, 75), (ns.ACT_LEAKY, 0.3, 200000, 16)])
def test_batchnorm_training_forward_backward(act, alpha, M, Cc):
    engine, L = _lib()
    # (seed 858 for the 700 x 130 relu6 case: the first from 700 whose float64 pre-activations leave every element outside the kink band.
    # Below 1000 rows the kink cap allows no ambiguous element in a column, and 91 000 elements with two kinks hold a few in most draws.)
    rng = np.random.default_rng(858 if M == 700 else M)
    z = (rng.normal(size=(M, Cc)) * rng.uniform(0.5, 3, Cc) + rng.normal(size=Cc) * 2).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 3, Cc).astype(np.float32), rng.normal(size=Cc).astype(np.float32)
    dy = rng.normal(size=(M, Cc)).astype(np.float32)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    mu, var = zt.mean(0), ((zt - zt.mean(0)) ** 2).mean(0)
    yt = (zt - mu) / torch.sqrt(var + 1e-3) * gt + bt
    yt = {ns.ACT_NONE: lambda v: v, ns.ACT_RELU: F.relu, ns.ACT_RELU6: lambda v: v.clamp(0, 6),
          ns.ACT_LEAKY: lambda v: F.leaky_relu(v, alpha)}[act](yt)
    yt.backward(torch.from_numpy(dy).double())
    zd, gd, bd, dyd = _cu(z), _cu(gamma), _cu(beta), _cu(dy)
    y, dz = torch.empty(M, Cc, device='cuda'), torch.empty(M, Cc, device='cuda')
    sm, si, dg, db = (torch.empty(Cc, device='cuda') for _ in range(4))
    mm, mv = torch.zeros(Cc, device='cuda'), torch.ones(Cc, device='cuda')
    assert L.yk_bn_train_fwd_f32(engine._ptr(zd), C.c_longlong(M), Cc, engine._ptr(gd), engine._ptr(bd), C.c_float(1e-3), act, C.c_float(alpha),
                                 engine._ptr(y), engine._ptr(sm), engine._ptr(si), engine._ptr(mm), engine._ptr(mv), C.c_float(0.99), _st()) == 0
    assert L.yk_bn_train_bwd_f32(engine._ptr(zd), engine._ptr(dyd), C.c_longlong(M), Cc, engine._ptr(gd), engine._ptr(bd), engine._ptr(sm),
                                 engine._ptr(si), act, C.c_float(alpha), engine._ptr(dz), engine._ptr(dg), engine._ptr(db), _st()) == 0
    _close(sm.cpu().numpy(), mu.detach().numpy(), 1e-5)
    _close(si.cpu().numpy(), (1 / torch.sqrt(var + 1e-3)).detach().numpy(), 1e-5)
    _close(mm.cpu().numpy(), 0.01 * mu.detach().numpy(), 1e-5)
    # the moving variance is fed the UNBIASED batch variance (tf fused_batch_norm; keras BatchNormalization fused=True)
    _close(mv.cpu().numpy(), 0.99 + 0.01 * var.detach().numpy() * (M / (M - 1.0)), 1e-5)
    # activation kinks: an fp32 pre-activation within rounding of 0/6 may land on the other side.  Such an element is left out of the dz
    # comparison, and what its flipped gate can do to the column sums (and through them to every dz of the column) is added to the
    # tolerances: tests/train_cases.py, kink_slack.  With no element near a kink this is the plain 2e-4 comparison.
    pre = ((zt - mu) / torch.sqrt(var + 1e-3) * gt + bt).detach().numpy()
    ref = dict(pre=pre, xhat=((zt - mu) / torch.sqrt(var + 1e-3)).detach().numpy(), gamma=gamma.astype(np.float64),
               invstd=(1 / torch.sqrt(var + 1e-3)).detach().numpy(), act=act, alpha=alpha, M=M)
    amb, slack_db, slack_dg, widen = train_cases.kink_slack(ref, dy)
    assert train_cases.kink_cap_holds(amb), int(amb.sum(0).max())
    got_y, got_dz = y.cpu().numpy(), dz.cpu().numpy()
    assert np.abs(got_y - yt.detach().numpy()).max() <= 2e-5 * np.abs(pre).max()
    ref_dz, ref_dg, ref_db = zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
    assert (np.abs(got_dz - ref_dz) <= 2e-4 * max(1e-6, np.abs(ref_dz).max()) + widen)[~amb].all()
    assert (np.abs(dg.cpu().numpy() - ref_dg) <= 2e-4 * max(1e-6, np.abs(ref_dg).max()) + slack_dg).all()
    assert (np.abs(db.cpu().numpy() - ref_db) <= 2e-4 * max(1e-6, np.abs(ref_db).max()) + slack_db).all()


@pytest.mark.parametrize('M,N,K,res', [(300, 75, 96, False),        # unsplit, ragged tile edges, scalar loads (K % 4 == 0 but N odd)
                                       (4480, 96, 576, True),        # 14x20 at 16 images: K split, the slice-adding pass leaves the partials
                                       (1120, 320, 960, False),      # 7x10: split
                                       (40000, 24, 16, True),        # unsplit, 625 row tiles, one ragged column tile
                                       (70000, 16, 27, False)])      # K % 4 != 0: the unvectorised loader; > 1024 partials: the wide finish
def test_conv_bn_forward_in_one_call_equals_the_separate_calls(M, N, K, res):
    """yk_gemm_bn_fwd_f32 = yk_gemm_f32 + yk_bn_train_fwd_res_f32 with the statistics' partial sums left by the producer of z: z bitwise the
    same, mean / invstd / moving statistics / y within 1e-6 relative (the double sums are added in another order)."""
    engine, L = _lib()
    rng = np.random.default_rng(M + N)
    X = (rng.normal(size=(M, K)) + 0.3).astype(np.float32)
    W = rng.normal(size=(N, K)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 2, N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    r = rng.normal(size=(M, N)).astype(np.float32) if res else None
    xd, wd, gd, bd = _cu(X), _cu(W), _cu(gamma), _cu(beta)
    rd = _cu(r) if res else None
    outs = []
    for fused in (False, True):
        z, y = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
        sm, si = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
        mm, mv = torch.zeros(N, device='cuda'), torch.ones(N, device='cuda')
        bn = (engine._ptr(gd), engine._ptr(bd), C.c_float(1e-3), ns.ACT_RELU6, C.c_float(6.0), engine._ptr(y), engine._ptr(sm), engine._ptr(si),
              engine._ptr(mm), engine._ptr(mv), C.c_float(0.99), engine._ptr(rd) if res else None, _st())
        if fused:
            assert L.yk_gemm_bn_fwd_f32(M, N, K, engine._ptr(xd), K, engine._ptr(wd), K, engine._ptr(z), *bn) == 0, L.yk_last_error()
        else:
            assert L.yk_gemm_f32(0, 1, M, N, K, C.c_float(1), engine._ptr(xd), K, engine._ptr(wd), K, C.c_float(0), engine._ptr(z), N, _st()) == 0
            assert L.yk_bn_train_fwd_res_f32(engine._ptr(z), C.c_longlong(M), N, *bn) == 0
        outs.append([t.cpu().numpy() for t in (z, y, sm, si, mm, mv)])
    a, b = outs
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[2:], b[2:]):
        _close(v, u, 1e-6)
    assert np.abs(a[1] - b[1]).max() <= 1e-5 * np.abs(a[1]).max()
    zz = X.astype(np.float64) @ W.astype(np.float64).T
    _close(b[2], zz.mean(0), 1e-5)
    _close(b[3], 1 / np.sqrt(zz.var(0) + 1e-3), 1e-5)


@pytest.mark.parametrize('stride,Cc', [(1, 72), (2, 24), (1, 130)])
def test_depthwise_bn_forward_in_one_call_equals_the_separate_calls(stride, Cc):
    engine, L = _lib()
    rng = np.random.default_rng(20 + stride)
    B, Hi, Wi = 5, 29, 38
    Ho, Wo = (Hi + 2 - 3) // stride + 1, (Wi + 2 - 3) // stride + 1
    M = B * Ho * Wo
    x = rng.normal(size=(B, Hi, Wi, Cc)).astype(np.float32)
    w = rng.normal(size=(9, Cc)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 2, Cc).astype(np.float32), rng.normal(size=Cc).astype(np.float32)
    geom = [C.c_int(v) for v in (B, Hi, Wi, Cc, Ho, Wo, stride, 1, 1)]
    xd, wd, gd, bd = _cu(x), _cu(w), _cu(gamma), _cu(beta)
    outs = []
    for fused in (False, True):
        z, y = torch.empty(M, Cc, device='cuda'), torch.empty(M, Cc, device='cuda')
        sm, si = torch.empty(Cc, device='cuda'), torch.empty(Cc, device='cuda')
        mm, mv = torch.zeros(Cc, device='cuda'), torch.ones(Cc, device='cuda')
        bn = (engine._ptr(gd), engine._ptr(bd), C.c_float(1e-3), ns.ACT_RELU, C.c_float(0.0), engine._ptr(y), engine._ptr(sm), engine._ptr(si),
              engine._ptr(mm), engine._ptr(mv), C.c_float(0.999), None, _st())
        if fused:
            assert L.yk_dw3x3_bn_fwd_f32(engine._ptr(xd), engine._ptr(wd), *geom, engine._ptr(z), *bn) == 0, L.yk_last_error()
        else:
            assert L.yk_dw3x3_fwd_f32(engine._ptr(xd), engine._ptr(wd), *geom, engine._ptr(z), _st()) == 0
            assert L.yk_bn_train_fwd_res_f32(engine._ptr(z), C.c_longlong(M), Cc, *bn) == 0
        outs.append([t.cpu().numpy() for t in (z, y, sm, si, mm, mv)])
    a, b = outs
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[2:], b[2:]):
        _close(v, u, 1e-6)
    assert np.abs(a[1] - b[1]).max() <= 1e-5 * np.abs(a[1]).max()


@pytest.mark.parametrize('stride', [1, 2])
def test_maxpool_upsample_bias_colsum_axpy(stride):
    engine, L = _lib()
    rng = np.random.default_rng(stride)
    B, Hi, Wi, Cc = 2, 13, 20, 16
    Ho, Wo = -(-Hi // stride), -(-Wi // stride)
    x = rng.normal(size=(B, Hi, Wi, Cc)).astype(np.float32)
    dy = rng.normal(size=(B, Ho, Wo, Cc)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    pb, pr = max((Ho - 1) * stride + 2 - Hi, 0), max((Wo - 1) * stride + 2 - Wi, 0)
    yt = F.max_pool2d(F.pad(xt, (0, pr, 0, pb), value=float('-inf')), 2, stride)
    yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    xd, dyd = _cu(x), _cu(dy)
    y, dx = torch.empty(B, Ho, Wo, Cc, device='cuda'), torch.empty(B, Hi, Wi, Cc, device='cuda')
    arg = torch.empty(B, Ho, Wo, Cc, dtype=torch.uint8, device='cuda')
    assert L.yk_maxpool2_fwd_f32(engine._ptr(xd), B, Hi, Wi, Cc, Ho, Wo, stride, engine._ptr(y), engine._ptr(arg), _st()) == 0
    assert L.yk_maxpool2_bwd_f32(engine._ptr(dyd), engine._ptr(arg), B, Hi, Wi, Cc, Ho, Wo, stride, engine._ptr(dx), _st()) == 0
    assert np.array_equal(y.cpu().numpy(), yt.detach().permute(0, 2, 3, 1).float().numpy())
    _close(dx.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy(), 1e-6)
    # UpSampling2D(2) adjoint
    g = rng.normal(size=(B, 2 * Hi, 2 * Wi, Cc)).astype(np.float32)
    gd, du = _cu(g), torch.empty(B, Hi, Wi, Cc, device='cuda')
    assert L.yk_upsample2x_bwd_f32(engine._ptr(gd), B, Hi, Wi, Cc, engine._ptr(du), _st()) == 0
    _close(du.cpu().numpy(), g.reshape(B, Hi, 2, Wi, 2, Cc).astype(np.float64).sum((2, 4)), 1e-6)
    # bias / column sum / axpy
    bias = rng.normal(size=Cc).astype(np.float32)
    yb, cs = _cu(x), torch.empty(Cc, device='cuda')
    assert L.yk_bias_add_f32(engine._ptr(yb), C.c_longlong(B * Hi * Wi), Cc, engine._ptr(_cu(bias)), _st()) == 0
    assert np.array_equal(yb.cpu().numpy(), x + bias)
    assert L.yk_colsum_f32(engine._ptr(xd), C.c_longlong(B * Hi * Wi), Cc, engine._ptr(cs), _st()) == 0
    _close(cs.cpu().numpy(), x.reshape(-1, Cc).astype(np.float64).sum(0), 1e-5)
    assert L.yk_axpy_f32(C.c_longlong(x.size), C.c_float(-0.25), engine._ptr(xd), engine._ptr(yb), _st()) == 0
    _close(yb.cpu().numpy(), (x + bias) - 0.25 * x, 1e-6)


def test_adam_matches_keras_update_rule_with_decay():
    engine, L = _lib()
    rng = np.random.default_rng(0)
    n = 10007
    p0 = rng.normal(size=n).astype(np.float32)
    ref = train_ref.AdamRef(5e-4, decay=0.01)
    w = {'p': p0.astype(np.float64)}
    p, m, v = _cu(p0), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    for it in range(4):
        g = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, n)).astype(np.float32)
        w = ref.apply(w, {'p': g.astype(np.float64)})
        assert L.yk_adam_f32(C.c_longlong(n), engine._ptr(p), engine._ptr(_cu(g)), engine._ptr(m), engine._ptr(v), C.c_float(5e-4),
                             C.c_float(0.01), C.c_longlong(it), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-7), C.c_float(1.0), _st()) == 0
        assert np.abs(p.cpu().numpy() - w['p']).max() <= 2e-6


# --------------------------------------------------------------------------------------------- whole step
def _case(name, hw, B, alpha, seed):
    spec = ns.NETWORKS[name]([hw[0], hw[1], 3], 3, 20, alpha=alpha)
    w = spec.init_weights(seed)
    h = Helper(None, 20, VOC_ANCHORS if len(spec.outputs) == 2 else np.concatenate([VOC_ANCHORS, VOC_ANCHORS[:1] * 0.5]),
               [list(hw)], [list(x) for x in spec.out_hw()])
    rng = np.random.default_rng(seed)
    ys = [[] for _ in spec.outputs]
    for b in range(B):
        n = int(rng.integers(1, 5))
        boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
        for i, lab in enumerate(h.box_to_label(boxes)):
            ys[i].append(lab)
    yt = [np.stack(y).astype(np.float32) for y in ys]
    x = rng.uniform(0, 1, (B, hw[0], hw[1], 3)).astype(np.float32)
    return spec, w, h, x, yt


def _gate_flips(tr, spec, stats):
    """Elements whose activation gate (ReLU/ReLU6/LeakyReLU kink) is evaluated on different sides by the fp32 tape and the float64
    oracle.  There the two compute different — equally valid — sub-gradients, and with batch-statistics BatchNorm over a few
    dozen samples one flipped element moves every upstream gradient by ~1e-2, so the comparison is only defined for flips == 0."""
    flips = 0
    for i, op in enumerate(spec.ops):
        if op['type'] == ns.OP_MAXPOOL:                    # the winning tap of a 2x2 window is a gate too
            xin = stats[f'op{i}/pool_in']
            arg = tr.saved[i]['arg'].cpu().numpy()
            Bq, Ho, Wo, Cc = arg.shape
            st = op['stride']
            pad = np.full((Bq, (Ho - 1) * st + 2, (Wo - 1) * st + 2, Cc), -np.inf)
            pad[:, :xin.shape[1], :xin.shape[2]] = xin
            taps = np.stack([pad[:, (t >> 1):(t >> 1) + (Ho - 1) * st + 1:st, (t & 1):(t & 1) + (Wo - 1) * st + 1:st] for t in range(4)], -1)
            flips += int((taps.argmax(-1) != arg).sum())
            continue
        if i not in tr.saved or 'z' not in tr.saved[i] or op['act'] == ns.ACT_NONE:
            continue
        l = tr.lay[op['layer']]
        sv = tr.saved[i]
        pre = ((sv['z'] - sv['mean']) * sv['invstd'] * tr.view(tr.P, l.bn_name + '/gamma') + tr.view(tr.P, l.bn_name + '/beta')).cpu().numpy()
        rp = stats[l.name + '/pre']
        flips += int(((pre > 0) != (rp > 0)).sum())
        if op['act'] == ns.ACT_RELU6:
            flips += int(((pre < 6) != (rp < 6)).sum())
    return flips


@pytest.mark.parametrize('name,hw,B,alpha', [('yolo_mobilev1', (64, 96), 4, 0.5), ('yolo_mobilev2', (64, 96), 4, 0.5),
                                            ('tiny_yolo', (64, 96), 3, 1.0), ('yolo', (64, 64), 2, 1.0)])
def test_training_step_loss_and_all_gradients_vs_autograd(name, hw, B, alpha):
    from k210_yolo_framework_amd.train import Trainer
    hyper = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)
    compared = 0
    for seed in range(5, 17):                              # every kernel is deterministic, so this scan is reproducible
        spec, w, h, x, yt = _case(name, hw, B, alpha, seed)
        ref_data, ref_reg, ref_g, ref_stats, ref_pred = train_ref.loss_and_grads(spec, w, x, yt, h.anchors, want_pre=True, **hyper)
        tr = Trainer(spec, w, h.anchors, B, lr=5e-4, decay=0.0, **hyper)
        r = tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
        torch.cuda.synchronize()
        data = float(sum(p[0] for p in r['layers']).cpu())
        assert abs(data - ref_data) <= 1e-4 * abs(ref_data), (data, ref_data)          # loss: always comparable
        assert abs(float(r['reg'].cpu()) - ref_reg) <= 1e-5 * abs(ref_reg)
        flips = _gate_flips(tr, spec, ref_stats)
        if flips:
            print(name, 'seed', seed, 'gate flips', flips, '-> gradients not comparable, next seed')
            continue
        got = tr.grads()
        worst = 0.0
        gmax = max(np.abs(v).max() for v in ref_g.values())
        for k, rg in ref_g.items():
            if np.abs(rg).max() < 1e-9 * gmax:
                # a BN beta that feeds straight into another BatchNorm has an analytically ZERO gradient; fp32 leaves the
                # rounding residue of a sum of O(gmax) terms that cancel
                assert np.abs(got[k]).max() <= 1e-6 * gmax, (k, np.abs(got[k]).max(), gmax)
                continue
            scale = np.abs(rg).max()
            e = np.abs(got[k] - rg).max() / scale
            worst = max(worst, e)
            assert e <= 2e-3, (k, e, scale)
        print(name, 'seed', seed, 'worst gradient error (relative to tensor max):', worst)
        compared += 1
        if compared == (1 if name == 'yolo' else 2):
            break
    assert compared >= 1, 'no flip-free seed found'


def test_nested_and_swapped_adds_gradients_vs_autograd():
    """the Add backward may share dy between its two inputs only when the later producer is a BatchNorm conv (a fresh dz); and a
    folded Add must work whichever operand is the conv's output.  Gradients of every parameter against float64 autograd."""
    from k210_yolo_framework_amd.train import Trainer
    hyper = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)
    spec = residual_zoo_spec()
    h = Helper(None, 20, VOC_ANCHORS, [[32, 48]], [list(v) for v in spec.out_hw()])
    compared = 0
    for seed in range(3, 15):
        w = spec.init_weights(seed)
        rng = np.random.default_rng(seed)
        B = 4
        ys = [[] for _ in spec.outputs]
        for _ in range(B):
            n = int(rng.integers(1, 4))
            boxes = np.stack([rng.integers(0, 20, n), rng.uniform(.2, .8, n), rng.uniform(.2, .8, n), rng.uniform(.1, .6, n), rng.uniform(.1, .6, n)], 1)
            for i, lab in enumerate(h.box_to_label(boxes)):
                ys[i].append(lab)
        yt = [np.stack(y).astype(np.float32) for y in ys]
        x = rng.uniform(0, 1, (B, 32, 48, 3)).astype(np.float32)
        ref_data, ref_reg, ref_g, ref_stats, _ = train_ref.loss_and_grads(spec, w, x, yt, h.anchors, want_pre=True, **hyper)
        tr = Trainer(spec, w, h.anchors, B, lr=5e-4, decay=0.0, **hyper)
        r = tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
        torch.cuda.synchronize()
        data = float(sum(p[0] for p in r['layers']).cpu())
        assert abs(data - ref_data) <= 1e-4 * abs(ref_data), (data, ref_data)
        if _gate_flips(tr, spec, ref_stats):
            continue
        got = tr.grads()
        gmax = max(np.abs(v).max() for v in ref_g.values())
        for k, rg in ref_g.items():
            if np.abs(rg).max() < 1e-9 * gmax:
                assert np.abs(got[k]).max() <= 1e-6 * gmax, k
                continue
            assert np.abs(got[k] - rg).max() / np.abs(rg).max() <= 2e-3, (k, seed)
        compared += 1
        if compared == 2:
            break
    assert compared >= 1, 'no flip-free seed found'


def test_adam_step_moves_weights_like_reference_and_loss_decreases():
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev1', (64, 96), 4, 0.5, 9)
    hyper = dict(obj_thresh=0.7, iou_thresh=0.5, obj_weight=1.0, noobj_weight=1.0, wh_weight=1.0)
    tr = Trainer(spec, w, h.anchors, 4, lr=1e-3, decay=0.0, **hyper)
    xd, ytd = _cu(x), [_cu(y) for y in yt]
    ref_opt, wref = train_ref.AdamRef(1e-3), {k: np.asarray(v, np.float64) for k, v in w.items()}
    losses = []
    for it in range(3):
        _, _, g, stats, _ = train_ref.loss_and_grads(spec, wref, x, yt, h.anchors, **hyper)
        wref = ref_opt.apply(wref, g)
        losses.append(tr.step(xd, ytd)['loss'])
        got = tr.export_weights()
        for k in g:
            # Adam's first steps are ~lr*sign(g): where |g| is at rounding level the sign is arbitrary, so bound by a fraction of
            # the step size on average and by the step size itself everywhere
            d = np.abs(got[k] - wref[k])
            assert d.max() <= 2.5e-3 * (it + 1), (k, it, d.max())
            assert d.mean() <= 1e-4 * (it + 1), (k, it, d.mean())
    for k in range(8):
        losses.append(tr.step(xd, ytd)['loss'])
    assert losses[-1] < 0.7 * losses[0], losses                    # overfits one batch
    mm = tr.export_weights()['conv1_bn/moving_mean']
    assert np.isfinite(mm).all() and not np.allclose(mm, w['conv1_bn/moving_mean'])
    pr = tr.precision_recall()
    assert len(pr) == 2 and all(0.0 <= v <= 1.0 for t in pr for v in t)


def test_moving_statistics_follow_keras_momentum_rule():
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev1', (64, 96), 4, 0.5, 11)
    _, _, _, stats, preds = train_ref.loss_and_grads(spec, w, x, yt, h.anchors)
    tr = Trainer(spec, w, h.anchors, 4)
    got_preds = tr.forward(_cu(x))
    for gp, rp in zip(got_preds, preds):
        _close(gp.cpu().numpy(), rp, 2e-4)
    rows = {}
    for op in spec.ops:                                                   # samples per channel of each BatchNorm: B * h * w
        if op.get('layer'):
            ho, wo, _ = spec.tensors[op['out']]
            l = next(l for l in spec.layers if l.name == op['layer'])
            if l.bn_name:
                rows[l.bn_name] = 4 * ho * wo
    for bn, (mu, var) in stats.items():
        _close(tr.moving[bn + '/moving_mean'].cpu().numpy(), 0.99 * w[bn + '/moving_mean'] + 0.01 * mu, 1e-4)
        m = rows[bn]                                                      # fused_batch_norm feeds the moving average the unbiased variance
        _close(tr.moving[bn + '/moving_variance'].cpu().numpy(), 0.99 * w[bn + '/moving_variance'] + 0.01 * var * m / (m - 1), 1e-4)


def test_training_step_is_bitwise_reproducible():
    """No atomics anywhere in the step (split-K slabs and column sums are reduced in a fixed order)."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev2', (64, 96), 4, 0.5, 21)
    runs = []
    for _ in range(2):
        tr = Trainer(spec, w, h.anchors, 4)
        tr.step(_cu(x), [_cu(y) for y in yt])
        tr.step(_cu(x), [_cu(y) for y in yt])
        runs.append((tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_graph_replayed_step_equals_the_eager_step_bitwise():
    """Trainer(use_graph=True) captures forward + loss + backward once (after an eager first step) and replays it: the same kernels
    on the same buffers in the same order, so gradients and parameters after three steps equal the eager run bit for bit."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev1', (64, 96), 4, 0.5, 22)
    runs = []
    for graph in (False, True):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph)
        for _ in range(3):                                                    # step 1 eager, step 2 captured + replayed, step 3 replayed
            tr.step(_cu(x), [_cu(y) for y in yt])
        runs.append((tr.G.cpu().numpy().copy(), tr.P.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_reloading_weights_and_changing_hyper_parameters_after_a_replayed_step():
    """ADVICE (round 2): the captured graph bakes in raw pointers and launch scalars.  load_weights() must write the BatchNorm moving
    statistics IN PLACE (the replayed kernels keep updating the buffers export_weights() reads), and a change of tr.hyper must drop
    the capture.  Reference behaviour: keras load_weights / compile with new loss weights, then fit again (keras_train.py:52-98)."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev1', (64, 96), 4, 0.5, 23)
    xs, ys = _cu(x), [_cu(y) for y in yt]

    def run(graph, obj_weight_after):
        tr = Trainer(spec, w, h.anchors, 4, use_graph=graph)
        for _ in range(3):                                                    # eager, capture + replay, replay
            tr.step(xs, ys)
        tr.load_weights(w)                                                    # back to the start (parameters AND moving statistics)
        tr.m.zero_(); tr.v.zero_(); tr.iterations = 0
        if obj_weight_after is not None:
            tr.hyper['obj_weight'] = obj_weight_after
        out = [tr.step(xs, ys) for _ in range(2)]
        return out, tr.export_weights(), tr.G.cpu().numpy().copy()
    for ow in (None, 3.0):
        (le, we, ge), (lg, wg, gg) = run(False, ow), run(True, ow)
        assert [o['loss'] for o in le] == [o['loss'] for o in lg], ow
        assert np.array_equal(ge, gg), ow
        for k in we:
            assert np.array_equal(we[k], wg[k]), (ow, k)                      # includes every moving_mean / moving_variance
    # and the moving statistics did move after the reload (they are not the loaded values any more)
    k = spec.layers[0].bn_name + '/moving_mean'
    assert not np.array_equal(wg[k], np.asarray(w[k], np.float32))


def test_full_size_config3_step_mobilev2_b16_loss_and_gradient_direction():
    """BASELINE configs[3] at full size (yolo_mobilev2 1.0, 224x320, 16 images).  With ~1e8 activations some gates always flip
    between fp32 and float64, so gradients are compared by direction and norm per tensor instead of element-wise."""
    from k210_yolo_framework_amd.train import Trainer
    spec, w, h, x, yt = _case('yolo_mobilev2', (224, 320), 16, 1.0, 31)
    ref_data, ref_reg, ref_g, _, _ = train_ref.loss_and_grads(spec, w, x, yt, h.anchors)
    tr = Trainer(spec, w, h.anchors, 16)
    r = tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
    data = float(sum(p[0] for p in r['layers']).cpu())
    assert abs(data - ref_data) <= 1e-4 * abs(ref_data), (data, ref_data)
    assert abs(float(r['reg'].cpu()) - ref_reg) <= 1e-5 * abs(ref_reg)
    got = tr.grads()
    gmax = max(np.abs(v).max() for v in ref_g.values())
    cos_min = 1.0
    for k, rg in ref_g.items():
        if np.abs(rg).max() < 1e-9 * gmax:
            continue
        a, b = got[k].ravel().astype(np.float64), rg.ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        cos_min = min(cos_min, cos)
        assert cos >= 0.999, (k, cos)
        assert abs(np.linalg.norm(a) / np.linalg.norm(b) - 1) <= 2e-2, k
    print('config3 full size: min cosine', cos_min)


def test_rccl_allreduce_of_the_flat_gradient_bucket_single_rank_group():
    """The exchange primitive itself on the GPU: a 1-rank RCCL group all-reduces the flat bucket (identity)."""
    import torch.distributed as dist
    from k210_yolo_framework_amd import shard
    from k210_yolo_framework_amd.train import Trainer
    import os
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29571')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
    try:
        spec, w, h, x, yt = _case('yolo_mobilev1', (64, 96), 4, 0.5, 3)
        tr = Trainer(spec, w, h.anchors, 4)
        tr.loss_and_grads(_cu(x), [_cu(y) for y in yt])
        before = tr.G.clone()
        dist.all_reduce(tr.G, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        assert torch.equal(before, tr.G)
        assert shard.allreduce_gradients(tr.G, dist) is tr.G
    finally:
        dist.destroy_process_group()


def test_make_train_cli_synthetic_run_saves_a_checkpoint_the_inference_model_loads(tmp_path, monkeypatch):
    from k210_yolo_framework_amd import training, yolonet
    tr = training.cli(['--synthetic', '40', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '8',
                       '--max_nrof_epochs', '3', '--init_learning_rate', '0.001', '--vaildation_split', '0.2', '--log_dir', str(tmp_path),
                       '--obj_weight', '1', '--noobj_weight', '1', '--wh_weight', '1', '--iou_thresh', '0.5'])
    ck = list(tmp_path.glob('*/yolo_model.h5'))                           # keras_train.py:105-109: log/<time>/yolo_model.h5
    assert len(ck) == 1 and (ck[0].parent / 'args.txt').exists() and (ck[0].parent / 'yolo_model.npz').exists()
    assert tr.iterations == 12                                            # 32 training images / 8 per step * 3 epochs
    model, wrapper = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.5)
    wrapper.load_weights(str(ck[0]))                                      # the Keras-layout HDF5 file, read without h5py
    x = np.random.default_rng(0).uniform(0, 1, (2, 224, 320, 3)).astype(np.float32)
    y = wrapper.predict(x)
    assert [t.shape for t in y] == [(2, 7, 10, 3, 25), (2, 14, 20, 3, 25)] and all(np.isfinite(t).all() for t in y)
    _, w2 = yolonet.yolo_mobilev1([224, 320, 3], 3, 20, alpha=0.5)
    w2.load_weights(str(ck[0].parent / 'yolo_model.npz'))
    for a, b in zip(y, w2.predict(x)):
        np.testing.assert_array_equal(a, b)                               # both checkpoint formats hold the same arrays


def test_make_train_reports_an_unusable_pre_ckpt_like_the_reference(tmp_path, capsys):
    """keras_train.py:52-57: a --pre_ckpt that is not an .h5 file prints `[ ERROR ]  Pre CKPT path is unvalid` and training goes on."""
    from k210_yolo_framework_amd import training
    training.cli(['--synthetic', '10', '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.5', '--batch_size', '4',
                  '--max_nrof_epochs', '1', '--max_steps', '1', '--log_dir', str(tmp_path), '--pre_ckpt', 'weights.ckpt'])
    out = capsys.readouterr().out
    assert '[ ERROR ]  Pre CKPT path is unvalid' in out and 'Save Model as' in out
