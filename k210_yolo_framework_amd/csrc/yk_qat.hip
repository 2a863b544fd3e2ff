// yk_qat.hip — quantisation-aware training (train.Trainer(qat=...)): the kmodel's 8-bit codes simulated in fp32.
//
// The rule is quantize.qparams restated in fp32, ONE rounding per operation (this file is compiled without FMA contraction).  For a
// range (lo, hi):  lo' = lo < 0 ? lo : +0,  hi' = hi > 0 ? hi : +0;  hi' == lo': s = 1 / 255, zp = 0;  otherwise s = (hi' - lo') / 255,
// zp = clamp(rintf((0 - lo') / s), 0, 255).  Then u = rintf(x / s) + zp, q = clamp(u, 0, 255), fq(x) = s * (q - zp); the straight-through
// gradient passes where 0 <= u <= 255.  Real zero is the code zp, so fq(+-0) = +0.0 exactly.  A NaN stays a NaN (and passes no gradient).
//
//   yk_qat_weights_f32   every conv / depthwise kernel of the flat parameter buffer, each over its OWN exact [min, max]: three launches
//                        whatever the number of segments (copy + reset, per-tile min / max, per-tile quantise);
//   yk_qat_act_fwd_f32   yq = fq(y) over a slot of the device range table, and the batch's own min / max of y into the batch table;
//   yk_qat_act_bwd_f32   the straight-through mask, recomputed from the saved y;
//   yk_qat_update_f32    the range table after a step: moving average / widening of every owner slot, then the union slots.
// Minima and maxima are integer reductions on the ordered key of yk_range.h: bitwise reproducible.
#include "yk_range.h"

namespace {
using namespace yk_range;

struct QP {
    float s, zp;
};

__device__ __forceinline__ QP qp_of(float lo, float hi) {
    lo = lo < 0.f ? lo : 0.f;
    hi = hi > 0.f ? hi : 0.f;
    QP p;
    if (hi == lo) {
        p.s = 1.0f / 255.0f;
        p.zp = 0.f;
        return p;
    }
    p.s = (hi - lo) / 255.0f;
    const float z = rintf((0.f - lo) / p.s);
    p.zp = z < 0.f ? 0.f : (z > 255.f ? 255.f : z);
    return p;
}
__device__ __forceinline__ float code_of(float x, QP p) { return rintf(x / p.s) + p.zp; }                  // u, unclamped
__device__ __forceinline__ float fq_of(float x, QP p) {
    const float u = code_of(x, p);
    const float q = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
    return p.s * (q - p.zp);
}
__device__ __forceinline__ float ste_of(float g, float x, QP p) {
    const float u = code_of(x, p);
    return (u >= 0.f && u <= 255.f) ? g : 0.f;
}
__device__ __forceinline__ float unkey_f(uint32_t k) { return __uint_as_float(unkey_bits(k)); }

// elements in front of the first 16-byte boundary of p (p is 4-byte aligned), at most n
inline size_t head_of(const void *p, size_t n) {
    const size_t h = ((16u - ((uintptr_t)p & 15u)) & 15u) / 4u;
    return h < n ? h : n;
}
inline bool same_phase(const void *a, const void *b) { return (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0 && ((uintptr_t)a & 3u) == 0; }

// ---- activations ----------------------------------------------------------------------------------------------------------------------
// [0, head) scalar, n4 float4 from head, the scalar tail behind them
__global__ __launch_bounds__(CAL_BLOCK) void act_fwd_kernel(const float *__restrict__ y, size_t head, size_t n4, size_t n,
                                                            const float *__restrict__ range, float *__restrict__ yq, uint32_t *batch) {
    const QP p = qp_of(range[0], range[1]);
    Acc a;
    const size_t step = (size_t)gridDim.x * CAL_BLOCK, t = (size_t)blockIdx.x * CAL_BLOCK + threadIdx.x;
    const float4 *y4 = reinterpret_cast<const float4 *>(y + head);
    float4 *q4 = reinterpret_cast<float4 *>(yq + head);
    for (size_t i = t; i < n4; i += step) {
        const float4 v = y4[i];
        a.add(v.x);
        a.add(v.y);
        a.add(v.z);
        a.add(v.w);
        float4 r;
        r.x = fq_of(v.x, p);
        r.y = fq_of(v.y, p);
        r.z = fq_of(v.z, p);
        r.w = fq_of(v.w, p);
        q4[i] = r;
    }
    const size_t tail = head + 4 * n4;
    for (size_t i = t; i < head + (n - tail); i += step) {
        const size_t e = i < head ? i : tail + (i - head);
        const float v = y[e];
        a.add(v);
        yq[e] = fq_of(v, p);
    }
    fold(a, batch);
}

// dy may be dyq (in place): no __restrict__ on the two
__global__ __launch_bounds__(CAL_BLOCK) void act_bwd_kernel(const float *dyq, const float *__restrict__ y, size_t head, size_t n4, size_t n,
                                                            const float *__restrict__ range, float *dy) {
    const QP p = qp_of(range[0], range[1]);
    const size_t step = (size_t)gridDim.x * CAL_BLOCK, t = (size_t)blockIdx.x * CAL_BLOCK + threadIdx.x;
    const float4 *g4 = reinterpret_cast<const float4 *>(dyq + head);
    const float4 *y4 = reinterpret_cast<const float4 *>(y + head);
    float4 *d4 = reinterpret_cast<float4 *>(dy + head);
    for (size_t i = t; i < n4; i += step) {
        const float4 g = g4[i], v = y4[i];
        float4 r;
        r.x = ste_of(g.x, v.x, p);
        r.y = ste_of(g.y, v.y, p);
        r.z = ste_of(g.z, v.z, p);
        r.w = ste_of(g.w, v.w, p);
        d4[i] = r;
    }
    const size_t tail = head + 4 * n4;
    for (size_t i = t; i < head + (n - tail); i += step) {
        const size_t e = i < head ? i : tail + (i - head);
        dy[e] = ste_of(dyq[e], y[e], p);
    }
}

// ---- the range table after a step -----------------------------------------------------------------------------------------------------
// One workgroup.  Owner slots first (each by one thread), then the union slots in ascending order by thread 0: a union's parts are
// produced before it, so a union of unions reads finished values.
__global__ __launch_bounds__(256) void update_kernel(float *ranges, uint32_t *batch, const int *__restrict__ kind, const int *__restrict__ part0,
                                                     const int *__restrict__ part1, int n_slots, float m, float one_minus_m, int observe) {
    for (int i = threadIdx.x; i < n_slots; i += 256) {
        uint32_t *b = batch + (size_t)YK_RANGE_WORDS * i;
        if (kind[i] == YK_QAT_SLOT_OWNER && b[0] <= b[1]) {          // (an empty batch slot - nothing finite seen - keeps r)
            const float blo = unkey_f(b[0]), bhi = unkey_f(b[1]);
            float lo = ranges[2 * i], hi = ranges[2 * i + 1];
            if (observe) {
                lo = blo < lo ? blo : lo;
                hi = bhi > hi ? bhi : hi;
            } else {
                lo = m * lo + one_minus_m * blo;
                hi = m * hi + one_minus_m * bhi;
            }
            ranges[2 * i] = lo;
            ranges[2 * i + 1] = hi;
        }
        b[0] = 0xFFFFFFFFu;                                          // the extremes start again; the flag is sticky
        b[1] = 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < n_slots; ++i)
            if (kind[i] == YK_QAT_SLOT_UNION && part0[i] >= 0 && part0[i] < n_slots && part1[i] >= 0 && part1[i] < n_slots) {
                const float l0 = ranges[2 * part0[i]], l1 = ranges[2 * part1[i]], h0 = ranges[2 * part0[i] + 1], h1 = ranges[2 * part1[i] + 1];
                ranges[2 * i] = l1 < l0 ? l1 : l0;
                ranges[2 * i + 1] = h1 > h0 ? h1 : h0;
            }
}

// ---- weights --------------------------------------------------------------------------------------------------------------------------
struct qat_seg {
    const long long *off, *size;
    const int *tile_first;
    int nseg;
    long long total;                                                 // elements of the flat buffer: a segment outside it is skipped, never touched
};

// the segment of tile `t`: last s with tile_first[s] <= t
__device__ __forceinline__ int seg_of_tile(const qat_seg &S, int t) {
    int lo = 0, hi = S.nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (S.tile_first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Pq = P over the whole buffer (what lies outside the segments stays as copied), and every segment's range slot to "nothing seen"
__global__ __launch_bounds__(CAL_BLOCK) void w_copy_reset_kernel(const float *__restrict__ P, size_t head, size_t n4, size_t n, float *__restrict__ Pq,
                                                                 uint32_t *wrange, int nseg) {
    const size_t step = (size_t)gridDim.x * CAL_BLOCK, t = (size_t)blockIdx.x * CAL_BLOCK + threadIdx.x;
    const float4 *p4 = reinterpret_cast<const float4 *>(P + head);
    float4 *q4 = reinterpret_cast<float4 *>(Pq + head);
    for (size_t i = t; i < n4; i += step) q4[i] = p4[i];
    const size_t tail = head + 4 * n4;
    for (size_t i = t; i < head + (n - tail); i += step) {
        const size_t e = i < head ? i : tail + (i - head);
        Pq[e] = P[e];
    }
    for (size_t i = t; i < (size_t)nseg; i += step) {
        wrange[YK_RANGE_WORDS * i + 0] = 0xFFFFFFFFu;
        wrange[YK_RANGE_WORDS * i + 1] = 0u;
        wrange[YK_RANGE_WORDS * i + 2] = 0u;
        wrange[YK_RANGE_WORDS * i + 3] = 0u;
    }
}

// A tile is YK_QAT_TILE elements of ONE segment, counted from the segment's first 16-byte boundary (`head` elements in); tile 0 also takes
// the elements in front of it.  vec: P and Pq share their phase inside 16 bytes, so a group of four is one 16-byte access in both.
struct tile_pos {
    const float *w;
    long long n, e0, head;
    int seg;
    bool ok;
};
__device__ __forceinline__ tile_pos tile_of(const qat_seg &S, const float *P, bool vec) {
    tile_pos t;
    t.seg = seg_of_tile(S, (int)blockIdx.x);
    t.n = S.size[t.seg];
    const long long off = S.off[t.seg];
    t.ok = off >= 0 && t.n >= 1 && off <= S.total - t.n;             // (uniform over the workgroup)
    t.w = P + off;
    const long long h = vec ? (long long)(((16u - ((uintptr_t)t.w & 15u)) & 15u) / 4u) : 0;
    t.head = h < t.n ? h : t.n;
    t.e0 = t.head + (long long)((int)blockIdx.x - S.tile_first[t.seg]) * YK_QAT_TILE;
    return t;
}

__global__ __launch_bounds__(CAL_BLOCK) void w_range_kernel(qat_seg S, const float *__restrict__ P, int vec, uint32_t *wrange) {
    const tile_pos t = tile_of(S, P, vec != 0);
    if (!t.ok) return;
    Acc a;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < YK_QAT_TILE / (4 * CAL_BLOCK); ++j) {
        const long long e = t.e0 + 4 * (j * CAL_BLOCK + tid);
        if (vec && e + 3 < t.n) {
            const float4 v = *reinterpret_cast<const float4 *>(t.w + e);
            a.add(v.x);
            a.add(v.y);
            a.add(v.z);
            a.add(v.w);
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < t.n) a.add(t.w[e + k]);
        }
    }
    if (t.e0 == t.head && tid < t.head) a.add(t.w[tid]);
    fold(a, wrange + (size_t)YK_RANGE_WORDS * t.seg);
}

__global__ __launch_bounds__(CAL_BLOCK) void w_quant_kernel(qat_seg S, const float *__restrict__ P, int vec, const uint32_t *__restrict__ wrange,
                                                            float *__restrict__ Pq) {
    const tile_pos t = tile_of(S, P, vec != 0);
    if (!t.ok) return;
    const uint32_t klo = wrange[YK_RANGE_WORDS * t.seg], khi = wrange[YK_RANGE_WORDS * t.seg + 1];
    if (klo > khi) return;                                           // nothing finite in the segment: Pq keeps the copy
    const QP p = qp_of(unkey_f(klo), unkey_f(khi));
    float *q = Pq + S.off[t.seg];
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < YK_QAT_TILE / (4 * CAL_BLOCK); ++j) {
        const long long e = t.e0 + 4 * (j * CAL_BLOCK + tid);
        if (vec && e + 3 < t.n) {
            const float4 v = *reinterpret_cast<const float4 *>(t.w + e);
            float4 r;
            r.x = fq_of(v.x, p);
            r.y = fq_of(v.y, p);
            r.z = fq_of(v.z, p);
            r.w = fq_of(v.w, p);
            *reinterpret_cast<float4 *>(q + e) = r;
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < t.n) q[e + k] = fq_of(t.w[e + k], p);
        }
    }
    if (t.e0 == t.head && tid < t.head) q[tid] = fq_of(t.w[tid], p);
}

}  // namespace

extern "C" int yk_qat_tile(void) { return YK_QAT_TILE; }

extern "C" int yk_qat_weights_f32(const float *params, long long n, const long long *d_offset, const long long *d_size, const int *d_tile_first,
                                  int nseg, int ntiles, float *params_q, uint32_t *d_wrange, void *stream) {
    if (!params || n <= 0 || !d_offset || !d_size || !d_tile_first || nseg <= 0 || ntiles <= 0 || !params_q || params_q == params || !d_wrange ||
        ((uintptr_t)params & 3u) || ((uintptr_t)params_q & 3u)) {
        yk_set_error("yk_qat_weights_f32: bad argument");
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = same_phase(params, params_q);
    const size_t head = vec ? head_of(params, (size_t)n) : (size_t)n, n4 = ((size_t)n - head) / 4;
    const size_t rest = (size_t)n - 4 * n4, items = n4 > rest ? n4 : rest;
    hipLaunchKernelGGL(w_copy_reset_kernel, dim3(grid_for(items > (size_t)nseg ? items : (size_t)nseg)), dim3(CAL_BLOCK), 0, st, params, head, n4,
                       (size_t)n, params_q, d_wrange, nseg);
    YK_HIP(hipGetLastError());
    const qat_seg S{d_offset, d_size, d_tile_first, nseg, n};
    hipLaunchKernelGGL(w_range_kernel, dim3((unsigned)ntiles), dim3(CAL_BLOCK), 0, st, S, params, vec ? 1 : 0, d_wrange);
    YK_HIP(hipGetLastError());
    hipLaunchKernelGGL(w_quant_kernel, dim3((unsigned)ntiles), dim3(CAL_BLOCK), 0, st, S, params, vec ? 1 : 0, (const uint32_t *)d_wrange, params_q);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_qat_act_fwd_f32(const float *y, long long n, const float *d_ranges, int slot, float *yq, uint32_t *d_batch, void *stream) {
    if (!y || n <= 0 || !d_ranges || slot < 0 || !yq || yq == y || !d_batch || ((uintptr_t)y & 3u) || ((uintptr_t)yq & 3u)) {
        yk_set_error("yk_qat_act_fwd_f32: bad argument");
        return YK_ERR_ARG;
    }
    const size_t head = same_phase(y, yq) ? head_of(y, (size_t)n) : (size_t)n, n4 = ((size_t)n - head) / 4;
    const size_t rest = (size_t)n - 4 * n4;
    hipLaunchKernelGGL(act_fwd_kernel, dim3(grid_for(n4 > rest ? n4 : rest)), dim3(CAL_BLOCK), 0, (hipStream_t)stream, y, head, n4, (size_t)n,
                       d_ranges + 2 * (size_t)slot, yq, d_batch + (size_t)YK_RANGE_WORDS * slot);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_qat_act_bwd_f32(const float *dyq, const float *y, long long n, const float *d_ranges, int slot, float *dy, void *stream) {
    if (!dyq || !y || n <= 0 || !d_ranges || slot < 0 || !dy || dy == y || ((uintptr_t)dyq & 3u) || ((uintptr_t)y & 3u) || ((uintptr_t)dy & 3u)) {
        yk_set_error("yk_qat_act_bwd_f32: bad argument");
        return YK_ERR_ARG;
    }
    const size_t head = same_phase(dyq, y) && same_phase(dyq, dy) ? head_of(y, (size_t)n) : (size_t)n, n4 = ((size_t)n - head) / 4;
    const size_t rest = (size_t)n - 4 * n4;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n4 > rest ? n4 : rest)), dim3(CAL_BLOCK), 0, (hipStream_t)stream, dyq, y, head, n4, (size_t)n,
                       d_ranges + 2 * (size_t)slot, dy);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_qat_update_f32(float *d_ranges, uint32_t *d_batch, const int *d_kind, const int *d_part0, const int *d_part1, int n_slots,
                                 float momentum, float one_minus_momentum, int observe, void *stream) {
    if (!d_ranges || !d_batch || !d_kind || !d_part0 || !d_part1 || n_slots <= 0) {
        yk_set_error("yk_qat_update_f32: bad argument");
        return YK_ERR_ARG;
    }
    hipLaunchKernelGGL(update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_ranges, d_batch, d_kind, d_part0, d_part1, n_slots, momentum,
                       one_minus_momentum, observe ? 1 : 0);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
