// yk_distill.hip — knowledge distillation on the raw outputs of one layer (the rule is stated in distill.py).
//
// Student rows p = [x, y, w, h, o, c_0..c_{C-1}], teacher rows q in the same layout, the teacher a constant.  With
//   kl(q, p) = sigmoid(q) (sp(-p) - sp(-q)) + (1 - sigmoid(q)) (sp(p) - sp(q)),  sp(z) = log(1 + e^z)  (Bernoulli KL, teacher -> student)
// and a = sigmoid(q_o), a row adds  obj = kl(q_o, p_o),  cls = a sum_c kl(q_c, p_c),  box = a [kl(q_x, p_x) + kl(q_y, p_y) +
// ((p_w - q_w)^2 + (p_h - q_h)^2) / 2]  (objectness-scaled distillation, Mehta & Ozturk 2018), and the layer's loss is
// weight / batch_size times the sum over the rows.
//
// One workgroup per 256 rows of one image: (1) the rows' a into LDS (one strided float per row), (2) the 256 * (5 + C) floats of the chunk
// element by element, so a wave reads 64 consecutive floats of both tensors and writes 64 consecutive gradient entries, (3) a block
// reduction in fp64 gives the chunk's three partial sums; a second tiny kernel adds the partials in (image, chunk) order.  No atomics:
// two calls give the same bits.
#include "yk_common.h"

#define YK_DISTILL_ROWS 256   // rows of one workgroup (= its threads)
#define YK_DISTILL_COLS 3     // float64 columns of a partial: obj, cls, box

__device__ __forceinline__ float d_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// finite for every finite z: max(z, 0) + log1p(exp(-|z|))
__device__ __forceinline__ float d_softplus(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
// sigmoid(p) - sigmoid(q) without the cancellation of two rounded sigmoids: with D = p - q (exact where it matters, p close to q)
//   D >= 0:  -expm1(-D) sigmoid(p) sigmoid(-q),     D < 0:  expm1(D) sigmoid(q) sigmoid(-p)
// every factor is in [0, 1], so +-80 stays finite; p == q (the same bits) gives +0
__device__ __forceinline__ float d_sigmoid_diff(float p, float q) {
    const float D = p - q;
    return D >= 0.f ? -expm1f(-D) * (d_sigmoid(p) * d_sigmoid(-q)) : expm1f(D) * (d_sigmoid(q) * d_sigmoid(-p));
}
// p == q (the same bits): both differences are +0, the result is +0
__device__ __forceinline__ float d_kl(float q, float sq, float p) {
    return sq * (d_softplus(-p) - d_softplus(-q)) + (1.f - sq) * (d_softplus(p) - d_softplus(q));
}

__global__ void __launch_bounds__(YK_DISTILL_ROWS) distill_kernel(const float *__restrict__ teacher, const float *__restrict__ pred, int rows,
                                                                   int E, int chunks, float scale, float *__restrict__ grad,
                                                                   double *__restrict__ partial) {
    __shared__ float a_s[YK_DISTILL_ROWS];
    __shared__ double red[YK_DISTILL_COLS][YK_DISTILL_ROWS / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int row0 = chunk * YK_DISTILL_ROWS;
    const int n_rows = min(YK_DISTILL_ROWS, rows - row0);
    const size_t base = ((size_t)b * rows + row0) * E;
    const float *q = teacher + base, *p = pred + base;
    float *g = grad ? grad + base : nullptr;
    if (tid < n_rows) a_s[tid] = d_sigmoid(q[(size_t)tid * E + 4]);
    __syncthreads();
    double s_obj = 0, s_cls = 0, s_box = 0;
    const int n = n_rows * E;
    for (int i = tid; i < n; i += YK_DISTILL_ROWS) {
        const int r = i / E, e = i - r * E;
        const float qv = q[i], pv = p[i], a = a_s[r];
        float term, d;
        if (e == 2 || e == 3) {
            d = pv - qv;
            term = 0.5f * (d * d);
        } else {
            const float sq = e == 4 ? a : d_sigmoid(qv);
            d = d_sigmoid_diff(pv, qv);
            term = d_kl(qv, sq, pv);
        }
        if (e == 4) {
            s_obj += (double)term;
        } else {
            d = a * d;
            if (e < 4)
                s_box += (double)(a * term);
            else
                s_cls += (double)(a * term);
        }
        if (g) g[i] += scale * d;
    }
    double v[YK_DISTILL_COLS] = {s_obj, s_cls, s_box};
#pragma unroll
    for (int k = 0; k < YK_DISTILL_COLS; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
    }
    __syncthreads();
    if (tid < YK_DISTILL_COLS) partial[(size_t)blockIdx.x * YK_DISTILL_COLS + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// out_loss = {total, obj, cls, box}, each weight / batch_size times its sum; the partials are added in (image, chunk) order
__global__ void distill_finish_kernel(int n_partial, const double *__restrict__ partial, double scale, float *__restrict__ out_loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[YK_DISTILL_COLS] = {0, 0, 0};
    for (int i = 0; i < n_partial; ++i)
        for (int k = 0; k < YK_DISTILL_COLS; ++k) s[k] += partial[(size_t)i * YK_DISTILL_COLS + k];
    const double ob = scale * s[0], cl = scale * s[1], bx = scale * s[2];
    out_loss[0] = (float)(ob + cl + bx);
    out_loss[1] = (float)ob;
    out_loss[2] = (float)cl;
    out_loss[3] = (float)bx;
}

extern "C" int yk_distill_loss_f32(const float *d_teacher, const float *d_pred, int batch, int rows_per_image, int class_num, float weight,
                                   int batch_size, float *d_loss, float *d_grad, void *stream) {
    if (!d_teacher || !d_pred || !d_loss) {
        yk_set_error("yk_distill_loss_f32: d_teacher, d_pred and d_loss must not be NULL");
        return YK_ERR_ARG;
    }
    if (batch <= 0 || rows_per_image <= 0 || class_num < 1 || batch_size <= 0) {
        yk_set_error("yk_distill_loss_f32: batch %d, rows_per_image %d, class_num %d, batch_size %d: batch, rows_per_image and batch_size must be "
                     "positive, class_num at least 1", batch, rows_per_image, class_num, batch_size);
        return YK_ERR_ARG;
    }
    const int chunks = (rows_per_image + YK_DISTILL_ROWS - 1) / YK_DISTILL_ROWS;
    // the grid is one dimension of batch * chunks workgroups, and a chunk's elements are indexed in 32 bits
    if ((long long)batch * chunks > 0x7fffffffLL || (long long)YK_DISTILL_ROWS * (5 + (long long)class_num) > 0x7fffffffLL) {
        yk_set_error("yk_distill_loss_f32: batch %d x rows_per_image %d x class_num %d is too large", batch, rows_per_image, class_num);
        return YK_ERR_ARG;
    }
    int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("yk_distill_loss_f32: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    const int n_partial = batch * chunks;
    double *partial = (double *)yk_scratch(dev, stream, YK_SLOT_DISTILL, sizeof(double) * YK_DISTILL_COLS * (size_t)n_partial);
    if (!partial) return YK_ERR_NOMEM;
    hipStream_t st = (hipStream_t)stream;
    const float scale = weight / (float)batch_size;
    hipLaunchKernelGGL(distill_kernel, dim3(n_partial), dim3(YK_DISTILL_ROWS), 0, st, d_teacher, d_pred, rows_per_image, 5 + class_num, chunks,
                       scale, d_grad, partial);
    hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(64), 0, st, n_partial, partial, (double)weight / (double)batch_size, d_loss);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
