// yk_adaround.hip — adaptive weight rounding for `make kmodel ADAROUND=True` (the rule is stated in adaround.py):
//   yk_dw3x3_gram_f32        G_c = sum over the output positions of x x^T, x the 9 taps of channel c: the Gram matrix of a depthwise layer;
//   yk_adaround_step_f32     one Adam step of the relaxed rounding loss on every free weight, and the next weight error D;
//   yk_adaround_dw_quad_f32  P[c] = G_c D[c] for a depthwise layer (a dense layer's P = D G is yk_gemm_f32);
//   yk_adaround_rowerr_f64   E_c = sum_k D[c][k] P[c][k] per row, in float64.
// Compiled without FMA contraction: every statement of the step rounds once, as adaround.step's float32 restatement does.
//
// No floating-point atomics anywhere.  yk_dw3x3_gram_f32 is two launches: a workgroup owns a chunk of output rows (positions) and 64
// channels, its 4 row lanes add their rows in ascending order and fold in the order 0, 1, 2, 3, and it leaves 45 partials per channel
// in d_work; the finishing launch adds the chunks of an entry in ascending order and ADDS the sum to the output.  The rows of a chunk
// follow from M = B * Ho * Wo alone (YK_DWGRAM_ROWS, or more once M passes YK_DWGRAM_ROWS * YK_DWGRAM_MAX_CHUNKS rows): two calls give
// the same bits.
#include "yk_common.h"
#include <cmath>

struct gram_geom {
    int B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l;
};

static void gram_split(long long M, long long *rpc, long long *chunks) {
    long long r = (M + YK_DWGRAM_MAX_CHUNKS - 1) / YK_DWGRAM_MAX_CHUNKS;
    if (r < YK_DWGRAM_ROWS) r = YK_DWGRAM_ROWS;
    *rpc = r;
    *chunks = (M + r - 1) / r;
}

// partial [chunk][45][C]: entry e = i (i + 1) / 2 + j, j <= i
__global__ void __launch_bounds__(256) dw_gram_kernel(gram_geom q, const float *__restrict__ x, long long M, long long rpc,
                                                      double *__restrict__ partial) {
    __shared__ double red[45][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = (int)blockIdx.y * 64 + cl;
    const bool live = c < q.C;
    double acc[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) acc[e] = 0.0;
    const long long m0 = (long long)blockIdx.x * rpc, m1 = m0 + rpc < M ? m0 + rpc : M;
    if (live) {
        for (long long m = m0 + rl; m < m1; m += 4) {
            const int ox = (int)(m % q.Wo), oy = (int)((m / q.Wo) % q.Ho), b = (int)(m / ((long long)q.Wo * q.Ho));
            double xv[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = oy * q.stride - q.pad_t + t / 3, ix = ox * q.stride - q.pad_l + t % 3;
                xv[t] = ((unsigned)iy < (unsigned)q.Hi && (unsigned)ix < (unsigned)q.Wi)
                            ? (double)x[(((size_t)b * q.Hi + iy) * q.Wi + ix) * q.C + c] : 0.0;
            }
            int e = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) acc[e++] += xv[i] * xv[j];      // fp32 x fp32 is exact in float64
        }
    }
    for (int r = 1; r < 4; ++r) {                                             // the row lanes in order
        if (rl == r) {
#pragma unroll
            for (int e = 0; e < 45; ++e) red[e][cl] = acc[e];
        }
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int e = 0; e < 45; ++e) acc[e] += red[e][cl];
        }
        __syncthreads();
    }
    if (rl == 0 && live) {
#pragma unroll
        for (int e = 0; e < 45; ++e) partial[((size_t)blockIdx.x * 45 + e) * q.C + c] = acc[e];
    }
}

// G [C][9][9] += the chunks of every entry in ascending order; both halves of the symmetric matrix are written
__global__ void __launch_bounds__(256) dw_gram_finish_kernel(const double *__restrict__ partial, long long chunks, int C, double *__restrict__ G) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 45LL * C) return;
    const int e = (int)(idx / C), c = (int)(idx % C);
    double s = 0.0;
    for (long long k = 0; k < chunks; ++k) s += partial[((size_t)k * 45 + e) * C + c];
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    double *g = G + (size_t)c * 81;
    g[i * 9 + j] += s;
    if (i != j) g[j * 9 + i] += s;
}

static bool gram_sizes_ok(int B, int Hi, int Wi, int C, int Ho, int Wo, int stride) {
    return B > 0 && Hi > 0 && Wi > 0 && C > 0 && Ho > 0 && Wo > 0 && stride > 0;
}

extern "C" int yk_dw3x3_gram_workspace_bytes(int B, int Ho, int Wo, int C, size_t *bytes) {
    if (!bytes || B <= 0 || Ho <= 0 || Wo <= 0 || C <= 0) {
        yk_set_error("yk_dw3x3_gram_workspace_bytes: sizes must be positive and bytes not NULL");
        return YK_ERR_ARG;
    }
    long long rpc, chunks;
    gram_split((long long)B * Ho * Wo, &rpc, &chunks);
    *bytes = sizeof(double) * 45 * (size_t)chunks * (size_t)C;
    return YK_OK;
}

extern "C" int yk_dw3x3_gram_f32(const float *x, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t, int pad_l,
                                 double *d_gram, double *d_work, void *stream) {
    if (!x || !d_gram || !d_work || !gram_sizes_ok(B, Hi, Wi, C, Ho, Wo, stride) || pad_t < 0 || pad_l < 0) {
        yk_set_error("yk_dw3x3_gram_f32: x, d_gram and d_work must not be NULL, every size positive and the padding not negative");
        return YK_ERR_ARG;
    }
    if ((((uintptr_t)d_gram | (uintptr_t)d_work) & 7) != 0) {
        yk_set_error("yk_dw3x3_gram_f32: d_gram and d_work must be 8-byte aligned");
        return YK_ERR_ARG;
    }
    const gram_geom q = {B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l};
    const long long M = (long long)B * Ho * Wo;
    long long rpc, chunks;
    gram_split(M, &rpc, &chunks);
    const int groups = (C + 63) / 64;
    if (groups > 65535) {
        yk_set_error("yk_dw3x3_gram_f32: C %d is more than one grid dimension of channel groups", C);
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dw_gram_kernel, dim3((unsigned)chunks, (unsigned)groups), dim3(256), 0, st, q, x, M, rpc, d_work);
    hipLaunchKernelGGL(dw_gram_finish_kernel, dim3((unsigned)((45LL * C + 255) / 256)), dim3(256), 0, st, (const double *)d_work, chunks, C,
                       d_gram);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One element of the step: adaround.step's statements in its order (h = the rectified sigmoid, the gradient of the row's output error
// through P, the rounding regulariser, Adam with bias correction), then D for the next P.
struct ada_args {
    float s_w, rec_scale, reg_scale, lam, beta, lr, c1, c2;
};
#define ADA_ZETA 1.1f
#define ADA_GAMMA (-0.1f)
#define ADA_B1 0.9f
#define ADA_B2 0.999f
#define ADA_EPS 1e-8f

__device__ __forceinline__ float ada_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float ada_clip01(float h) { return fminf(fmaxf(h, 0.f), 1.f); }

__global__ void __launch_bounds__(256) adaround_step_kernel(ada_args a, size_t n, int K, float *__restrict__ V, float *__restrict__ m,
                                                            float *__restrict__ v, const float *__restrict__ r,
                                                            const uint8_t *__restrict__ frozen, const float *__restrict__ P,
                                                            const float *__restrict__ inv_e, float *__restrict__ D) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (frozen[i]) {
        D[i] = 0.f;
        return;
    }
    float vi = V[i];
    const float sg = ada_sigmoid(vi);
    const float hr = sg * (ADA_ZETA - ADA_GAMMA) + ADA_GAMMA;
    const float h = ada_clip01(hr);
    const float dh = (hr > 0.f && hr < 1.f) ? (sg * (1.f - sg)) * (ADA_ZETA - ADA_GAMMA) : 0.f;
    float g = (a.rec_scale * inv_e[i / (size_t)K]) * P[i];
    if (a.lam != 0.f) {
        const float x = 2.f * h - 1.f, ax = fabsf(x);
        // |x|^(beta - 1): beta = 2 needs no powf, and 0 stays 0 whatever the exponent (no NaN at h = 0.5, none at h in {0, 1} where ax = 1)
        const float pw = a.beta == 2.f ? ax : (ax == 0.f ? 0.f : powf(ax, a.beta - 1.f));
        const float sgn = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
        g = g - (a.reg_scale * pw) * sgn;
    }
    g = g * dh;
    const float mi = ADA_B1 * m[i] + (1.f - ADA_B1) * g;
    const float vv = ADA_B2 * v[i] + ((1.f - ADA_B2) * g) * g;
    m[i] = mi;
    v[i] = vv;
    vi = vi - a.lr * ((mi / a.c1) / (sqrtf(vv / a.c2) + ADA_EPS));
    V[i] = vi;
    const float h2 = ada_clip01(ada_sigmoid(vi) * (ADA_ZETA - ADA_GAMMA) + ADA_GAMMA);
    D[i] = a.s_w * (h2 - r[i]);
}

extern "C" int yk_adaround_step_f32(float *V, float *m, float *v, const float *r, const uint8_t *frozen, const float *P, const float *inv_e,
                                    float *D, int Co, int K, long long n_free, float s_w, float lam, float beta, float lr, int t, void *stream) {
    if (!V || !m || !v || !r || !frozen || !P || !inv_e || !D || Co <= 0 || K <= 0 || n_free <= 0 || t <= 0) {
        yk_set_error("yk_adaround_step_f32: no tensor may be NULL; Co %d, K %d, n_free %lld and t %d must be positive", Co, K, n_free, t);
        return YK_ERR_ARG;
    }
    const size_t n = (size_t)Co * (size_t)K;
    if ((n + 255) / 256 > 0x7fffffffULL) {
        yk_set_error("yk_adaround_step_f32: %d x %d weights are more than one grid dimension of workgroups", Co, K);
        return YK_ERR_ARG;
    }
    ada_args a;
    a.s_w = s_w;
    a.rec_scale = (float)(2.0 * (double)s_w / (double)Co);
    a.reg_scale = (float)(2.0 * (double)lam * (double)beta / (double)n_free);
    a.lam = lam;
    a.beta = beta;
    a.lr = lr;
    a.c1 = (float)(1.0 - pow(0.9, (double)t));
    a.c2 = (float)(1.0 - pow(0.999, (double)t));
    hipLaunchKernelGGL(adaround_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, n, K, V, m, v, r, frozen,
                       P, inv_e, D);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// P[c][i] = sum_j G_c[i][j] D[c][j], j ascending, in float64, rounded to fp32 once
__global__ void __launch_bounds__(256) adaround_dw_quad_kernel(const double *__restrict__ G, const float *__restrict__ D, int C,
                                                               float *__restrict__ P) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)C * 9) return;
    const size_t c = idx / 9;
    const double *g = G + idx * 9;                                            // row i of G_c: (c * 9 + i) * 9
    const float *d = D + c * 9;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) s += g[j] * (double)d[j];
    P[idx] = (float)s;
}

extern "C" int yk_adaround_dw_quad_f32(const double *G, const float *D, int C, float *P, void *stream) {
    if (!G || !D || !P || C <= 0) {
        yk_set_error("yk_adaround_dw_quad_f32: G, D and P must not be NULL and C %d positive", C);
        return YK_ERR_ARG;
    }
    hipLaunchKernelGGL(adaround_dw_quad_kernel, dim3((unsigned)(((size_t)C * 9 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, D, C, P);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// E[c] = sum_k D[c][k] P[c][k]: one workgroup per row, thread j adds k = j, j + 256, ... in ascending order, the 64 lanes of a wave fold
// in a fixed tree and the 4 waves in order.  fp32 x fp32 is exact in float64.
__global__ void __launch_bounds__(256) adaround_rowerr_kernel(const float *__restrict__ D, const float *__restrict__ P, int K,
                                                              double *__restrict__ E) {
    __shared__ double red[4];
    const size_t row = (size_t)blockIdx.x * (size_t)K;
    double s = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) s += (double)D[row + k] * (double)P[row + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) E[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int yk_adaround_rowerr_f64(const float *D, const float *P, int Co, int K, double *E, void *stream) {
    if (!D || !P || !E || Co <= 0 || K <= 0 || ((uintptr_t)E & 7) != 0) {
        yk_set_error("yk_adaround_rowerr_f64: D, P and E (8-byte aligned) must not be NULL; Co %d and K %d must be positive", Co, K);
        return YK_ERR_ARG;
    }
    hipLaunchKernelGGL(adaround_rowerr_kernel, dim3((unsigned)Co), dim3(256), 0, (hipStream_t)stream, D, P, K, E);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
