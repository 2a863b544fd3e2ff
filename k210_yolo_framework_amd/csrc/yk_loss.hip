// yk_loss.hip — YOLO loss forward + dL/dy_pred + ignore mask + precision/recall counters for one output layer.
//
// Replaces, as ONE fused pass per image instead of a TF graph with a Python loop
// over the batch (tools/utils.py:698-705):
//   create_loss_fn / loss_fn        tools/utils.py:708-793
//   calc_ignore_mask, tf_iou        tools/utils.py:662-705, 617-659
//   tf_xywh_to_all / _to_grid       tools/utils.py:524-572
//   Yolo_Precision / Yolo_Recall    tools/custom.py:13-75   (raw logit vs threshold, custom.py:33)
// The gradient is TF autodiff's: ignore_mask comes from a comparison and carries none.
// One workgroup per image: (1) the image's ground-truth boxes (cells with y_true conf > obj_thresh) are
// compacted into LDS, (2) every prediction is decoded, matched against them (best IoU), contributes its five
// loss terms and writes its 5+C gradient entries, (3) a block reduction in fp64 produces per-image partials;
// a second tiny kernel adds the partials in image order (deterministic).
//
// Box term: the reference's xy / wh terms (YK_BOX_LOSS_MSE, the default) or, opt-in, one of the IoU-family losses between
// the decoded prediction and the label box: GIoU (Rezatofighi et al. 2019), DIoU / CIoU (Zheng et al. 2020).  The mode is a template
// parameter of the kernel: the MSE instance is the kernel as it was, the others replace the xy / wh arithmetic of an object cell.
//
// Options on the objectness and class terms (the rule is stated in lossopt.py; yk_yolo_loss_opt): focal loss, label smoothing
// and an IoU objectness target.  They are the second template parameter, a set of L_* bits: the instances with OPT = 0 are the kernels that
// yk_yolo_loss / yk_yolo_loss_ex launch, and an option that is off costs its instances nothing.
#include "yk_common.h"

#define YK_LOSS_MAXGT 1024
#define YK_LOSS_COLS 9   // float64 columns of a partial: xy, wh, obj, noobj, cls, tp, fp, fn, box

struct loss_args {
    int h, w, A, C, E, batch_size;
    float anchors[YK_MAX_ANCHORS][2];
    float obj_thresh, iou_thresh, obj_w, noobj_w, wh_w;
    int box_loss;
    float box_w;
    float gamma, alpha, smooth_k, smooth_h;   // focal exponent and balance; label smoothing z -> z smooth_k + smooth_h (1 - eps, eps / 2)
};

// OPT bits.  L_POW: gamma is not 2 (everyone's default, two multiplications) and the focal factor takes a powf
enum { L_FOBJ = 1, L_FCLS = 2, L_POW = 4, L_SMOOTH = 8, L_IOU = 16 };

__device__ __forceinline__ float l_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float l_bce(float z, float x) { return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x))); }

// Focal term fl(z, x) = a_t m^gamma bce(z, x) with m = 1 - p_t = z sigmoid(-x) + (1 - z) sigmoid(x), and dx = d fl / d x, the full derivative:
// d m / d x = (1 - 2 z) p (1 - p), d bce / d x = p - z.  Both sigmoids come from one expf(-|x|) with no subtraction from 1, so a saturated
// logit keeps the bits of its small side; the same expf feeds the bce.
template <bool POW>
__device__ __forceinline__ float l_focal(float z, float x, float gamma, float alpha, float &dx) {
    const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
    const float big = r, small = e * r;                                  // sigmoid(|x|), sigmoid(-|x|)
    const float p = x >= 0.f ? big : small, q = x >= 0.f ? small : big;
    const float bce = fmaxf(x, 0.f) - x * z + log1pf(e);
    const float m = z * q + (1.f - z) * p;
    const float at = alpha > 0.f ? z * alpha + (1.f - z) * (1.f - alpha) : 1.f;
    float pw, dpw;                                                       // m^gamma and its derivative by m
    if (POW) {
        const float p1 = gamma > 0.f ? powf(m, gamma - 1.f) : 0.f;       // gamma >= 1: finite at m = 0
        pw = gamma > 0.f ? p1 * m : 1.f;
        dpw = gamma * p1;
    } else {
        pw = m * m;
        dpw = 2.f * m;
    }
    dx = at * (dpw * ((1.f - 2.f * z) * p * q) * bce + pw * (p - z));
    return at * pw * bce;
}

// 0.5 at a tie: where two edges coincide the loss has a kink, and the even split is the one sub-gradient that is zero for equal boxes
__device__ __forceinline__ float l_less(float u, float v) { return u < v ? 1.f : (u == v ? 0.5f : 0.f); }

// One axis of two boxes given as centre c / size s (prediction b, label t): the clamped overlap ov and the enclosing extent en, with
// their derivatives by the prediction's centre (.._c) and size (.._s).
struct l_axis {
    float ov, ov_c, ov_s, en, en_c, en_s;
};
__device__ __forceinline__ l_axis l_box_axis(float bc, float bs, float tc, float ts) {
    const float b1 = bc - bs / 2.f, b2 = bc + bs / 2.f, t1 = tc - ts / 2.f, t2 = tc + ts / 2.f;
    const float raw = fminf(b2, t2) - fmaxf(b1, t1);
    const float on = raw > 0.f ? 1.f : 0.f;
    const float i2 = on * l_less(b2, t2), i1 = on * l_less(t1, b1);      // d ov / d b2, -d ov / d b1
    const float e2 = l_less(t2, b2), e1 = l_less(b1, t1);                // d en / d b2, -d en / d b1
    l_axis r;
    r.ov = fmaxf(raw, 0.f);
    r.ov_c = i2 - i1;
    r.ov_s = (i2 + i1) / 2.f;
    r.en = fmaxf(b2, t2) - fminf(b1, t1);
    r.en_c = e2 - e1;
    r.en_s = (e2 + e1) / 2.f;
    return r;
}

// IoU-family loss of one object cell and its gradient g = d loss / d (bx, by, bw, bh); alpha of CIoU is a constant.
// iou_out: the IoU the loss is built on (the objectness target of L_IOU).
template <int MODE>
__device__ __forceinline__ float l_box_loss(float bx, float by, float bw, float bh, float tx, float ty, float tw, float th, float g[4],
                                            float &iou_out) {
    const float eps = 1e-7f;
    const l_axis X = l_box_axis(bx, bw, tx, tw), Y = l_box_axis(by, bh, ty, th);
    const float I = X.ov * Y.ov;
    const float U = bw * bh + tw * th - I + eps;
    const float iou = I / U;
    iou_out = iou;
    const float dI[4] = {Y.ov * X.ov_c, X.ov * Y.ov_c, Y.ov * X.ov_s, X.ov * Y.ov_s};
    const float dU[4] = {-dI[0], -dI[1], bh - dI[2], bw - dI[3]};
    float l = 1.f - iou;
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = -(dI[k] - iou * dU[k]) / U;
    if (MODE == YK_BOX_LOSS_GIOU) {
        const float Cc = X.en * Y.en + eps, r = U / Cc;
        const float dC[4] = {Y.en * X.en_c, X.en * Y.en_c, Y.en * X.en_s, X.en * Y.en_s};
        l += (Cc - U) / Cc;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] -= (dU[k] - r * dC[k]) / Cc;
    } else {
        const float c2 = X.en * X.en + Y.en * Y.en + eps;
        const float dx = bx - tx, dy = by - ty, r = (dx * dx + dy * dy) / c2;
        const float dc2[4] = {2.f * X.en * X.en_c, 2.f * Y.en * Y.en_c, 2.f * X.en * X.en_s, 2.f * Y.en * Y.en_s};
        l += r;
        g[0] += (2.f * dx - r * dc2[0]) / c2;
        g[1] += (2.f * dy - r * dc2[1]) / c2;
        g[2] -= r * dc2[2] / c2;
        g[3] -= r * dc2[3] / c2;
        if (MODE == YK_BOX_LOSS_CIOU) {
            const float k4 = 0.40528473456935109f;                       // 4 / pi^2
            const float d = atanf(tw / th) - atanf(bw / bh);
            const float v = k4 * d * d;
            const float alpha = v / (1.f - iou + v + eps);
            const float q = alpha * 2.f * k4 * d / (bw * bw + bh * bh);
            l += alpha * v;
            g[2] -= q * bh;
            g[3] += q * bw;
        }
    }
    return l;
}

template <int MODE, int OPT = 0>
__global__ void __launch_bounds__(256) yolo_loss_kernel(loss_args a, const float *__restrict__ y_true,
                                                        const float *__restrict__ y_pred, float *__restrict__ grad,
                                                        float *__restrict__ ignore_out, double *__restrict__ partial) {
    __shared__ float4 gt[YK_LOSS_MAXGT];
    __shared__ int ngt;
    __shared__ double red[YK_LOSS_COLS][4];
    // grid (batch, chunks of 256 boxes): one workgroup per image left 16 workgroups on the chip for 41 us; every chunk gathers the image's
    // ground truth itself (a strided scan of P objectness values) and handles one box per thread
    const int b = blockIdx.x, tid = threadIdx.x;
    const int P = a.h * a.w * a.A;
    const float *yt = y_true + (size_t)b * P * a.E, *yp = y_pred + (size_t)b * P * a.E;
    if (tid == 0) ngt = 0;
    __syncthreads();
    for (int p = tid; p < P; p += 256) {
        const float *t = yt + (size_t)p * a.E;
        if (t[4] > a.obj_thresh) {
            const int k = atomicAdd(&ngt, 1);
            if (k < YK_LOSS_MAXGT) gt[k] = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
    __syncthreads();
    const int n = ngt;
    const float inv_bs = 1.f / (float)a.batch_size;
    double s_xy = 0, s_wh = 0, s_obj = 0, s_noobj = 0, s_cls = 0, s_box = 0;
    int tp = 0, fp = 0, fn = 0;
    for (int p = blockIdx.y * 256 + tid; p < min(P, (int)(blockIdx.y + 1) * 256); p += 256) {
        const float *t = yt + (size_t)p * a.E, *q = yp + (size_t)p * a.E;
        const int an = p % a.A, cell = p / a.A, col = cell % a.w, row = cell / a.w;
        const float px = q[0], py = q[1], pw = q[2], ph = q[3], pc = q[4];
        const float tx = t[0], ty = t[1], tw = t[2], th = t[3], tc = t[4];
        // prediction in image scale (tf_xywh_to_all)
        const float sx = l_sigmoid(px), sy = l_sigmoid(py);
        const float ax = (sx + (float)col) / (float)a.w, ay = (sy + (float)row) / (float)a.h;
        const float aw = expf(pw) * a.anchors[an][0], ah = expf(ph) * a.anchors[an][1];
        // ignore mask: best IoU against this image's ground truth (empty set -> -inf -> 1)
        float best = -INFINITY;
        if (n <= YK_LOSS_MAXGT) {
            for (int k = 0; k < n; ++k) {
                const float4 g = gt[k];
                const float iw = fmaxf(fminf(ax + aw / 2.f, g.x + g.z / 2.f) - fmaxf(ax - aw / 2.f, g.x - g.z / 2.f), 0.f);
                const float ih = fmaxf(fminf(ay + ah / 2.f, g.y + g.w / 2.f) - fmaxf(ay - ah / 2.f, g.y - g.w / 2.f), 0.f);
                const float inter = iw * ih;
                best = fmaxf(best, inter / (aw * ah + g.z * g.w - inter));
            }
        } else {   // more boxes than LDS slots: scan the label tensor directly
            for (int k = 0; k < P; ++k) {
                const float *g = yt + (size_t)k * a.E;
                if (!(g[4] > a.obj_thresh)) continue;
                const float iw = fmaxf(fminf(ax + aw / 2.f, g[0] + g[2] / 2.f) - fmaxf(ax - aw / 2.f, g[0] - g[2] / 2.f), 0.f);
                const float ih = fmaxf(fminf(ay + ah / 2.f, g[1] + g[3] / 2.f) - fmaxf(ay - ah / 2.f, g[1] - g[3] / 2.f), 0.f);
                const float inter = iw * ih;
                best = fmaxf(best, inter / (aw * ah + g[2] * g[3] - inter));
            }
        }
        const float ign = (best < a.iou_thresh) ? 1.f : 0.f;
        if (ignore_out) ignore_out[(size_t)b * P + p] = ign;
        const bool ob = tc > a.obj_thresh;
        const float obj = tc;
        // targets in grid scale.  One rounding (fma): rounding tx * w first costs the position inside the cell log2(w) bits, and with them
        // the xy gradient on a wide grid (257 columns: 5e-6 off, found by tests/test_gpu_loss.py against the float64-pinned oracle)
        const float gx = fmaf(tx, (float)a.w, -(float)col), gy = fmaf(ty, (float)a.h, -(float)row);
        const float gw = ob ? logf(tw / a.anchors[an][0]) : 0.f, gh = ob ? logf(th / a.anchors[an][1]) : 0.f;
        const float cw = 2.f - tw * th;
        float gb[4] = {0.f, 0.f, 0.f, 0.f};     // the IoU modes' gradient entries 0..3
        float iou = 0.f;                        // of an object cell's prediction with its label box (L_IOU)
        if (MODE == YK_BOX_LOSS_MSE) {
            s_xy += (double)(obj * cw * (l_bce(gx, px) + l_bce(gy, py)));
            s_wh += (double)(obj * cw * a.wh_w * ((gw - pw) * (gw - pw) + (gh - ph) * (gh - ph)));
            if ((OPT & L_IOU) && ob) {          // the IoU of l_box_loss; no box term uses it here
                const l_axis X = l_box_axis(ax, aw, tx, tw), Y = l_box_axis(ay, ah, ty, th);
                const float I = X.ov * Y.ov;
                iou = I / (aw * ah + tw * th - I + 1e-7f);
            }
        } else if (ob) {
            // skipped, not multiplied away, elsewhere: the label box of a cell without an object is all zeros (atan(0 / 0), 0 * NaN)
            const float k = obj * cw * a.box_w;
            s_box += (double)(k * l_box_loss<MODE>(ax, ay, aw, ah, tx, ty, tw, th, gb, iou));
            gb[0] = k * gb[0] * (sx * (1.f - sx) / (float)a.w) * inv_bs;
            gb[1] = k * gb[1] * (sy * (1.f - sy) / (float)a.h) * inv_bs;
            gb[2] = k * gb[2] * aw * inv_bs;
            gb[3] = k * gb[3] * ah * inv_bs;
        }
        // objectness: the target is y_true conf or, in an object cell under L_IOU, the clamped IoU, a constant in the gradient; the weights
        // (obj, the ignore mask) stay on y_true conf.  dbc = d bc / d pc
        float zo = tc;
        if ((OPT & L_IOU) && ob) zo = fminf(fmaxf(iou, 0.f), 1.f);
        float bc, dbc;
        if (OPT & L_FOBJ) {
            bc = l_focal<(OPT & L_POW) != 0>(zo, pc, a.gamma, a.alpha, dbc);
        } else {
            bc = l_bce(zo, pc);
            dbc = l_sigmoid(pc) - zo;
        }
        s_obj += (double)(obj * bc);
        s_noobj += (double)((1.f - obj) * ign * bc);
        float cls = 0.f;
        float *gr = grad ? grad + ((size_t)b * P + p) * a.E : nullptr;
        for (int c = 0; c < a.C; ++c) {
            const float x = q[5 + c];
            float z = t[5 + c];
            if (OPT & L_SMOOTH) z = z * a.smooth_k + a.smooth_h;
            if (OPT & L_FCLS) {
                float d;
                cls += l_focal<(OPT & L_POW) != 0>(z, x, a.gamma, a.alpha, d);
                if (gr) gr[5 + c] = obj * d * inv_bs;
            } else {
                cls += l_bce(z, x);
                if (gr) gr[5 + c] = obj * (l_sigmoid(x) - z) * inv_bs;
            }
        }
        s_cls += (double)(obj * cls);
        if (gr) {
            if (MODE == YK_BOX_LOSS_MSE) {
                gr[0] = obj * cw * (sx - gx) * inv_bs;
                gr[1] = obj * cw * (sy - gy) * inv_bs;
                gr[2] = obj * cw * a.wh_w * 2.f * (pw - gw) * inv_bs;
                gr[3] = obj * cw * a.wh_w * 2.f * (ph - gh) * inv_bs;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) gr[k] = gb[k];
            }
            gr[4] = (a.obj_w * obj + a.noobj_w * (1.f - obj) * ign) * dbc * inv_bs;
        }
        const bool pp = pc > a.obj_thresh;     // custom.py:33: raw logit
        tp += (ob && pp);
        fp += (!ob && pp);
        fn += (ob && !pp);
    }
    double v[YK_LOSS_COLS] = {s_xy, s_wh, s_obj, s_noobj, s_cls, (double)tp, (double)fp, (double)fn, s_box};
#pragma unroll
    for (int k = 0; k < YK_LOSS_COLS; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
    }
    __syncthreads();
    if (tid < YK_LOSS_COLS)
        partial[((size_t)b * gridDim.y + blockIdx.y) * YK_LOSS_COLS + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// out_loss = {total, xy, wh, obj, noobj, cls} and, for yk_yolo_loss_ex (n_out = 7), box; counts += {tp, fp, fn}
__global__ void yolo_loss_finish_kernel(loss_args a, int batch, const double *__restrict__ partial, float *__restrict__ out_loss,
                                        float *__restrict__ counts, int n_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[YK_LOSS_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < batch; ++b)
        for (int k = 0; k < YK_LOSS_COLS; ++k) s[k] += partial[(size_t)b * YK_LOSS_COLS + k];
    const double bs = (double)a.batch_size;
    const double xy = s[0] / bs, wh = s[1] / bs, ob = a.obj_w * s[2] / bs, no = a.noobj_w * s[3] / bs, cl = s[4] / bs, bx = s[8] / bs;
    out_loss[0] = a.box_loss == YK_BOX_LOSS_MSE ? (float)(ob + no + cl + xy + wh)   // utils.py:789
                                                : (float)(ob + no + cl + bx);        // xy and wh are not computed: both are 0
    out_loss[1] = (float)xy;
    out_loss[2] = (float)wh;
    out_loss[3] = (float)ob;
    out_loss[4] = (float)no;
    out_loss[5] = (float)cl;
    if (n_out > 6) out_loss[6] = (float)bx;
    if (counts) {
        counts[0] += (float)s[5];
        counts[1] += (float)s[6];
        counts[2] += (float)s[7];
    }
}

// The instances with options: every set of L_* bits that can be asked for (L_POW only beside a focal bit), for one box mode.
template <int MODE>
static void loss_launch_opt(int bits, dim3 grid, hipStream_t st, const loss_args &a, const float *d_y_true, const float *d_y_pred, float *d_grad,
                            float *d_ignore, double *partial) {
#define YK_L1(o)                                                                                                                          \
    case (o):                                                                                                                             \
        hipLaunchKernelGGL((yolo_loss_kernel<MODE, (o)>), grid, dim3(256), 0, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);      \
        break;
#define YK_L4(o) YK_L1(o) YK_L1((o) | L_SMOOTH) YK_L1((o) | L_IOU) YK_L1((o) | L_SMOOTH | L_IOU)
    switch (bits) {
        YK_L1(L_SMOOTH) YK_L1(L_IOU) YK_L1(L_SMOOTH | L_IOU)
        YK_L4(L_FOBJ) YK_L4(L_FCLS) YK_L4(L_FOBJ | L_FCLS)
        YK_L4(L_FOBJ | L_POW) YK_L4(L_FCLS | L_POW) YK_L4(L_FOBJ | L_FCLS | L_POW)
    }
#undef YK_L4
#undef YK_L1
}

// all entry points: `who` names the caller in the messages, n_out is the length of d_loss, opt (yk_yolo_loss_opt alone) holds the options
static int loss_launch(const char *who, const yk_loss_cfg_ex_t *cfg, const yk_loss_cfg_opt_t *opt, int n_out, const float *d_y_true,
                       const float *d_y_pred, int batch, float *d_loss, float *d_grad, float *d_ignore, float *d_counts, void *stream) {
    if (!cfg || !d_y_true || !d_y_pred || !d_loss || batch <= 0 || cfg->out_h <= 0 || cfg->out_w <= 0 || cfg->anchor_num <= 0 ||
        cfg->anchor_num > YK_MAX_ANCHORS || cfg->class_num <= 0 || cfg->batch_size <= 0) {
        yk_set_error("%s: bad argument", who);
        return YK_ERR_ARG;
    }
    const int box_loss = cfg->box_loss;
    if (box_loss != YK_BOX_LOSS_MSE && box_loss != YK_BOX_LOSS_GIOU && box_loss != YK_BOX_LOSS_DIOU && box_loss != YK_BOX_LOSS_CIOU) {
        yk_set_error("%s: box_loss %d is none of YK_BOX_LOSS_MSE (0), _GIOU (1), _DIOU (2), _CIOU (3)", who, box_loss);
        return YK_ERR_ARG;
    }
    int bits = 0;                                                       // L_*: what is on, and so which instance runs
    if (opt) {
        const float g = opt->focal_gamma, al = opt->focal_alpha, eps = opt->label_smooth;
        if (opt->focal < 0 || opt->focal > (YK_FOCAL_OBJ | YK_FOCAL_CLS)) {
            yk_set_error("%s: focal %d is no set of YK_FOCAL_OBJ (1), YK_FOCAL_CLS (2)", who, opt->focal);
            return YK_ERR_ARG;
        }
        if (!(g == 0.f || (g >= 1.f && g <= 5.f))) {                     // (a NaN fails every comparison)
            yk_set_error("%s: focal_gamma %g is neither 0 nor in 1 .. 5 (below 1 the gradient is unbounded)", who, (double)g);
            return YK_ERR_ARG;
        }
        if (!(al >= 0.f && al < 1.f)) {
            yk_set_error("%s: focal_alpha %g is neither 0 (off) nor inside (0, 1)", who, (double)al);
            return YK_ERR_ARG;
        }
        if (!(eps >= 0.f && eps < 1.f)) {
            yk_set_error("%s: label_smooth %g is not in [0, 1)", who, (double)eps);
            return YK_ERR_ARG;
        }
        if (opt->obj_target != YK_OBJ_TARGET_LABEL && opt->obj_target != YK_OBJ_TARGET_IOU) {
            yk_set_error("%s: obj_target %d is neither YK_OBJ_TARGET_LABEL (0) nor YK_OBJ_TARGET_IOU (1)", who, opt->obj_target);
            return YK_ERR_ARG;
        }
        if (g != 0.f || al != 0.f) {                                     // gamma = 0, alpha = 0: fl is bce
            bits |= (opt->focal & YK_FOCAL_OBJ ? L_FOBJ : 0) | (opt->focal & YK_FOCAL_CLS ? L_FCLS : 0);
            if (bits && g != 2.f) bits |= L_POW;
        }
        if (eps > 0.f) bits |= L_SMOOTH;
        if (opt->obj_target == YK_OBJ_TARGET_IOU) bits |= L_IOU;
    }
    int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("%s: no HIP device", who);
        return YK_ERR_NO_DEVICE;
    }
    loss_args a;
    a.h = cfg->out_h;
    a.w = cfg->out_w;
    a.A = cfg->anchor_num;
    a.C = cfg->class_num;
    a.E = 5 + cfg->class_num;
    a.batch_size = cfg->batch_size;
    for (int n = 0; n < a.A; ++n) {
        a.anchors[n][0] = cfg->anchors[n][0];
        a.anchors[n][1] = cfg->anchors[n][1];
    }
    a.obj_thresh = cfg->obj_thresh;
    a.iou_thresh = cfg->iou_thresh;
    a.obj_w = cfg->obj_weight;
    a.noobj_w = cfg->noobj_weight;
    a.wh_w = cfg->wh_weight;
    a.box_loss = box_loss;
    a.box_w = cfg->box_weight;
    a.gamma = opt ? opt->focal_gamma : 0.f;
    a.alpha = opt ? opt->focal_alpha : 0.f;
    a.smooth_k = opt ? 1.f - opt->label_smooth : 1.f;
    a.smooth_h = opt ? opt->label_smooth / 2.f : 0.f;
    const int chunks = (a.h * a.w * a.A + 255) / 256;
    double *partial = (double *)yk_scratch(dev, stream, YK_SLOT_LOSS, sizeof(double) * YK_LOSS_COLS * batch * chunks);
    if (!partial) return YK_ERR_NOMEM;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(batch, chunks);
    if (bits) {
        switch (box_loss) {
        case YK_BOX_LOSS_GIOU:
            loss_launch_opt<YK_BOX_LOSS_GIOU>(bits, grid, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
            break;
        case YK_BOX_LOSS_DIOU:
            loss_launch_opt<YK_BOX_LOSS_DIOU>(bits, grid, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
            break;
        case YK_BOX_LOSS_CIOU:
            loss_launch_opt<YK_BOX_LOSS_CIOU>(bits, grid, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
            break;
        default:
            loss_launch_opt<YK_BOX_LOSS_MSE>(bits, grid, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
        }
    } else
    switch (box_loss) {
    case YK_BOX_LOSS_GIOU:
        hipLaunchKernelGGL(yolo_loss_kernel<YK_BOX_LOSS_GIOU>, grid, dim3(256), 0, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
        break;
    case YK_BOX_LOSS_DIOU:
        hipLaunchKernelGGL(yolo_loss_kernel<YK_BOX_LOSS_DIOU>, grid, dim3(256), 0, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
        break;
    case YK_BOX_LOSS_CIOU:
        hipLaunchKernelGGL(yolo_loss_kernel<YK_BOX_LOSS_CIOU>, grid, dim3(256), 0, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
        break;
    default:
        hipLaunchKernelGGL(yolo_loss_kernel<YK_BOX_LOSS_MSE>, grid, dim3(256), 0, st, a, d_y_true, d_y_pred, d_grad, d_ignore, partial);
    }
    hipLaunchKernelGGL(yolo_loss_finish_kernel, dim3(1), dim3(64), 0, st, a, batch * chunks, partial, d_loss, d_counts, n_out);   // (image, chunk) in order
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_yolo_loss(const yk_loss_cfg_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                            float *d_grad, float *d_ignore, float *d_counts, void *stream) {
    yk_loss_cfg_ex_t ex;
    if (cfg) {
        ex.out_h = cfg->out_h;
        ex.out_w = cfg->out_w;
        ex.anchor_num = cfg->anchor_num;
        ex.class_num = cfg->class_num;
        memcpy(ex.anchors, cfg->anchors, sizeof(ex.anchors));
        ex.obj_thresh = cfg->obj_thresh;
        ex.iou_thresh = cfg->iou_thresh;
        ex.obj_weight = cfg->obj_weight;
        ex.noobj_weight = cfg->noobj_weight;
        ex.wh_weight = cfg->wh_weight;
        ex.batch_size = cfg->batch_size;
        ex.box_loss = YK_BOX_LOSS_MSE;
        ex.box_weight = 0.f;
    }
    return loss_launch("yk_yolo_loss", cfg ? &ex : nullptr, nullptr, 6, d_y_true, d_y_pred, batch, d_loss, d_grad, d_ignore, d_counts, stream);
}

extern "C" int yk_yolo_loss_ex(const yk_loss_cfg_ex_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                               float *d_grad, float *d_ignore, float *d_counts, void *stream) {
    return loss_launch("yk_yolo_loss_ex", cfg, nullptr, 7, d_y_true, d_y_pred, batch, d_loss, d_grad, d_ignore, d_counts, stream);
}

static_assert(offsetof(yk_loss_cfg_opt_t, focal) == sizeof(yk_loss_cfg_ex_t), "yk_loss_cfg_opt_t begins with yk_loss_cfg_ex_t's fields");

extern "C" int yk_yolo_loss_opt(const yk_loss_cfg_opt_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                                float *d_grad, float *d_ignore, float *d_counts, void *stream) {
    yk_loss_cfg_ex_t ex;
    if (cfg) memcpy(&ex, cfg, sizeof(ex));
    return loss_launch("yk_yolo_loss_opt", cfg ? &ex : nullptr, cfg, 7, d_y_true, d_y_pred, batch, d_loss, d_grad, d_ignore, d_counts, stream);
}
