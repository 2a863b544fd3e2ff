// yk_optim.hip — what ends a training step when the options of DESIGN.md 3.21 are on (the rule is stated in optim.py):
//   yk_sumsq_f32     sum of squares of the flat gradient bucket in float64, for the global-norm clip;
//   yk_adam_ex_f32   adam_kernel's statements (yk_train.hip) with the clip coefficient in front and the weight average behind, one pass;
//   yk_ema_f32       the average's statement alone, for buffers Adam does not own (the BatchNorm moving statistics).
// Compiled without FMA contraction: every statement below rounds once, as optim.py's float32 restatements do.
//
// yk_sumsq_f32 is two launches: a workgroup per tile of YK_SUMSQ_TILE floats leaves one float64 partial in d_work, and a finishing launch of
// one workgroup folds the partials.  The alternative, the last-arriving workgroup folding them behind a ticket, needs an agent-scope
// release per workgroup, a counter that something zeroes before every call and an acquire in the tail; in the training graph that tail cost
// more than the finishing launch it saved, and here the fold is followed by a launch that waits for it anyway.  Who adds what
// depends on n alone: element j of a tile always belongs to thread (j / 4) % 256, whichever width loads it, every thread adds its elements in
// ascending order, the 64 lanes of a wave and then the 4 waves fold in a fixed tree, and the finishing workgroup does the same over the
// partials.  No atomics: two calls give the same bits, and so do data-parallel replicas.
#include "yk_common.h"
#include <cmath>

#define YK_SUMSQ_THREADS 256
#define YK_SUMSQ_QUADS 4                                                    // float4 groups of one thread
#define YK_SUMSQ_TILE_ (YK_SUMSQ_THREADS * YK_SUMSQ_QUADS * 4)
static_assert(YK_SUMSQ_TILE_ == YK_SUMSQ_TILE, "yolo_hip.h states the tile the tests size their lengths by");

// the workgroup's sum in thread 0: lanes by xor-shuffle (a fixed tree), then the waves in order
__device__ __forceinline__ double block_sum_256(double s, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool VEC>
__global__ void __launch_bounds__(YK_SUMSQ_THREADS) sumsq_tile_kernel(const float *__restrict__ x, size_t n, double *__restrict__ partial) {
    __shared__ double red[YK_SUMSQ_THREADS / 64];
    const size_t tile0 = (size_t)blockIdx.x * YK_SUMSQ_TILE;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < YK_SUMSQ_QUADS; ++k) {
        const size_t i = tile0 + ((size_t)k * YK_SUMSQ_THREADS + threadIdx.x) * 4;
        if (VEC && i + 4 <= n) {
            const float4 q = *reinterpret_cast<const float4 *>(x + i);
            s += (double)q.x * (double)q.x;
            s += (double)q.y * (double)q.y;
            s += (double)q.z * (double)q.z;
            s += (double)q.w * (double)q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < n) {
                    const double v = (double)x[i + e];
                    s += v * v;
                }
        }
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(YK_SUMSQ_THREADS) sumsq_finish_kernel(const double *__restrict__ partial, size_t n_partial, double *__restrict__ out) {
    __shared__ double red[YK_SUMSQ_THREADS / 64];
    double s = 0.0;
    for (size_t i = threadIdx.x; i < n_partial; i += YK_SUMSQ_THREADS) s += partial[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) *out = s;
}

extern "C" int yk_sumsq_workspace_bytes(long long n, size_t *bytes) {
    if (!bytes || n <= 0) {
        yk_set_error("yk_sumsq_workspace_bytes: n %lld must be positive and bytes not NULL", n);
        return YK_ERR_ARG;
    }
    *bytes = sizeof(double) * (size_t)((n + YK_SUMSQ_TILE - 1) / YK_SUMSQ_TILE);
    return YK_OK;
}

extern "C" int yk_sumsq_f32(const float *x, long long n, double *d_work, double *d_out, void *stream) {
    if (!x || !d_work || !d_out || n <= 0) {
        yk_set_error("yk_sumsq_f32: x, d_work and d_out must not be NULL and n %lld positive", n);
        return YK_ERR_ARG;
    }
    const long long tiles = (n + YK_SUMSQ_TILE - 1) / YK_SUMSQ_TILE;
    if (tiles > 0x7fffffffLL) {
        yk_set_error("yk_sumsq_f32: n %lld is more than one grid dimension of tiles", n);
        return YK_ERR_ARG;
    }
    if ((((uintptr_t)d_work | (uintptr_t)d_out) & 7) != 0) {
        yk_set_error("yk_sumsq_f32: d_work and d_out must be 8-byte aligned");
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (((uintptr_t)x & 15) == 0)
        hipLaunchKernelGGL(sumsq_tile_kernel<true>, dim3((unsigned)tiles), dim3(YK_SUMSQ_THREADS), 0, st, x, (size_t)n, d_work);
    else
        hipLaunchKernelGGL(sumsq_tile_kernel<false>, dim3((unsigned)tiles), dim3(YK_SUMSQ_THREADS), 0, st, x, (size_t)n, d_work);
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(YK_SUMSQ_THREADS), 0, st, (const double *)d_work, (size_t)tiles, d_out);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One element of the update.  Between the two optional parts stand adam_kernel's statements, unchanged and in its order.
struct adam_args {
    float lr_t, b1, b2, eps, gscale, omd;
};

// min(1, clip_norm / (sqrt(s) + 1e-6)) in double, then one rounding to float (torch.nn.utils.clip_grad_norm_'s coefficient).  fmin returns
// the other operand for a NaN: a NaN sum gives 1 and the NaN gradients themselves reach the update; an infinite one gives 0.
__device__ __forceinline__ float clip_coefficient(const double *d_sumsq, float clip_norm) {
    return (float)fmin(1.0, (double)clip_norm / (sqrt(*d_sumsq) + 1e-6));
}

__device__ __forceinline__ float ema_one(float e, float src, float omd) {
    const float d = src - e;
    return e + omd * d;
}

template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_one(const adam_args &a, float c, float g, float &p, float &m, float &v, float &e) {
    float gi = g * a.gscale;
    if (CLIP) gi = gi * c;
    const float mi = a.b1 * m + (1.f - a.b1) * gi, vi = a.b2 * v + (1.f - a.b2) * gi * gi;
    m = mi;
    v = vi;
    p -= a.lr_t * mi / (sqrtf(vi) + a.eps);
    if (EMA) e = ema_one(e, p, a.omd);
}

// W = 4: n % 4 == 0 and every buffer 16-byte aligned, one float4 of each buffer per thread (a wave moves 1 KiB per instruction, the widest
// access there is); W = 1: any n, any alignment
template <bool CLIP, bool EMA, int W>
__global__ void __launch_bounds__(256) adam_ex_kernel(size_t n, float *p, const float *g, float *m, float *v, float *ema, const double *d_sumsq,
                                                      float clip_norm, adam_args a) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= n) return;
    const float c = CLIP ? clip_coefficient(d_sumsq, clip_norm) : 1.f;
    if (W == 4) {
        float4 pq = *reinterpret_cast<float4 *>(p + i), mq = *reinterpret_cast<float4 *>(m + i), vq = *reinterpret_cast<float4 *>(v + i);
        const float4 gq = *reinterpret_cast<const float4 *>(g + i);
        float4 eq = EMA ? *reinterpret_cast<float4 *>(ema + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        adam_one<CLIP, EMA>(a, c, gq.x, pq.x, mq.x, vq.x, eq.x);
        adam_one<CLIP, EMA>(a, c, gq.y, pq.y, mq.y, vq.y, eq.y);
        adam_one<CLIP, EMA>(a, c, gq.z, pq.z, mq.z, vq.z, eq.z);
        adam_one<CLIP, EMA>(a, c, gq.w, pq.w, mq.w, vq.w, eq.w);
        *reinterpret_cast<float4 *>(m + i) = mq;
        *reinterpret_cast<float4 *>(v + i) = vq;
        *reinterpret_cast<float4 *>(p + i) = pq;
        if (EMA) *reinterpret_cast<float4 *>(ema + i) = eq;
    } else {
        float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.f;
        adam_one<CLIP, EMA>(a, c, g[i], pi, mi, vi, ei);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (EMA) ema[i] = ei;
    }
}

template <int W>
__global__ void __launch_bounds__(256) ema_kernel(size_t n, const float *__restrict__ src, float *__restrict__ ema, float omd) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= n) return;
    if (W == 4) {
        const float4 s = *reinterpret_cast<const float4 *>(src + i);
        float4 e = *reinterpret_cast<float4 *>(ema + i);
        e.x = ema_one(e.x, s.x, omd);
        e.y = ema_one(e.y, s.y, omd);
        e.z = ema_one(e.z, s.z, omd);
        e.w = ema_one(e.w, s.w, omd);
        *reinterpret_cast<float4 *>(ema + i) = e;
    } else {
        ema[i] = ema_one(ema[i], src[i], omd);
    }
}

static bool grid_of(const char *who, long long n, int w, unsigned *blocks) {
    const long long b = (n / w + 255) / 256;
    if (b > 0x7fffffffLL) {
        yk_set_error("%s: n %lld is more than one grid dimension of workgroups", who, n);
        return false;
    }
    *blocks = (unsigned)b;
    return true;
}

template <bool CLIP, bool EMA>
static void launch_adam_ex(int w, unsigned blocks, hipStream_t st, size_t n, float *p, const float *g, float *m, float *v, float *ema,
                           const double *d_sumsq, float clip_norm, const adam_args &a) {
    if (w == 4)
        hipLaunchKernelGGL((adam_ex_kernel<CLIP, EMA, 4>), dim3(blocks), dim3(256), 0, st, n, p, g, m, v, ema, d_sumsq, clip_norm, a);
    else
        hipLaunchKernelGGL((adam_ex_kernel<CLIP, EMA, 1>), dim3(blocks), dim3(256), 0, st, n, p, g, m, v, ema, d_sumsq, clip_norm, a);
}

extern "C" int yk_adam_ex_f32(long long n, float *p, const float *g, float *m, float *v, float *ema, const double *d_sumsq, float lr, float decay,
                              long long iterations, float beta1, float beta2, float eps, float grad_scale, float clip_norm, float ema_omd,
                              void *stream) {
    if (!p || !g || !m || !v || n <= 0 || iterations < 0) {
        yk_set_error("yk_adam_ex_f32: p, g, m and v must not be NULL, n %lld positive and iterations %lld not negative", n, iterations);
        return YK_ERR_ARG;
    }
    if (d_sumsq && (!(clip_norm >= 0.f) || ((uintptr_t)d_sumsq & 7) != 0)) {
        yk_set_error("yk_adam_ex_f32: with d_sumsq, clip_norm %g must not be negative and d_sumsq 8-byte aligned", (double)clip_norm);
        return YK_ERR_ARG;
    }
    // the 16-byte path: n % 4 == 0 and every buffer it touches aligned (a NULL ema counts as aligned)
    const int w = (n % 4 == 0 && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0)) ? 4 : 1;
    unsigned blocks;
    if (!grid_of("yk_adam_ex_f32", n, w, &blocks)) return YK_ERR_ARG;
    // lr_t as yk_adam_f32 forms it
    const double t = (double)iterations + 1.0;
    const double lr_t = (double)lr / (1.0 + (double)decay * (double)iterations) * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));
    const adam_args a = {(float)lr_t, beta1, beta2, eps, grad_scale, ema_omd};
    hipStream_t st = (hipStream_t)stream;
    if (d_sumsq && ema)
        launch_adam_ex<true, true>(w, blocks, st, (size_t)n, p, g, m, v, ema, d_sumsq, clip_norm, a);
    else if (d_sumsq)
        launch_adam_ex<true, false>(w, blocks, st, (size_t)n, p, g, m, v, ema, d_sumsq, clip_norm, a);
    else if (ema)
        launch_adam_ex<false, true>(w, blocks, st, (size_t)n, p, g, m, v, ema, d_sumsq, clip_norm, a);
    else
        launch_adam_ex<false, false>(w, blocks, st, (size_t)n, p, g, m, v, ema, d_sumsq, clip_norm, a);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_ema_f32(long long n, const float *src, float *ema, float ema_omd, void *stream) {
    if (!src || !ema || n <= 0) {
        yk_set_error("yk_ema_f32: src and ema must not be NULL and n %lld positive", n);
        return YK_ERR_ARG;
    }
    const int w = (n % 4 == 0 && ((((uintptr_t)src | (uintptr_t)ema) & 15) == 0)) ? 4 : 1;
    unsigned blocks;
    if (!grid_of("yk_ema_f32", n, w, &blocks)) return YK_ERR_ARG;
    if (w == 4)
        hipLaunchKernelGGL(ema_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (size_t)n, src, ema, ema_omd);
    else
        hipLaunchKernelGGL(ema_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (size_t)n, src, ema, ema_omd);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
