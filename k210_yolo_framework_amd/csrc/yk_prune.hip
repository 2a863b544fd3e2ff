// yk_prune.hip — magnitude pruning of the flat parameter buffer (keras_train.py:59-71: tfmot prune_low_magnitude).
//
// Per prunable segment (one Conv2D kernel) of the flat fp32 buffer: the exact k-th largest |w|, the mask |w| >= threshold and the
// number of kept elements, for ALL segments in one call.  Everything is defined on the uint32 pattern of |w| (sign bit cleared), which
// orders non-negative floats: -0.0, denormals and +-inf need no special case, and a NaN is a pattern above infinity's (top digit 127 too).
// A segment of size 0 owns no tile; its pick workgroup reads an all-zero histogram, matches no bin and writes nothing.
//
// Selection = radix select, most significant digit first, four 8-bit digits of the pattern (shift 24, 16, 8, 0; the top digit only
// reaches 127).  A pass is
//   prune_hist_kernel   one workgroup per tile of YK_PRUNE_TILE elements of ONE segment: the digit histogram of the elements whose
//                       higher digits equal the prefix chosen so far, in LDS; then one integer atomic per non-empty bin into the
//                       segment's histogram;
//   prune_pick_kernel   one workgroup per segment: walk the bins from the top, pick the digit that holds the k-th largest, shrink k.
// After four passes the prefix IS the threshold pattern.  prune_mask_kernel writes the mask; the kept count needs no second count:
// (elements above the threshold) = k - (rank left inside the last digit), (elements equal to it) = that digit's bin.
// Integer atomics only, so every result is independent of arrival order: bitwise reproducible and equal to a sort.
#include <algorithm>

#include "yk_common.h"

struct prune_seg {
    const long long *off, *size, *keep;
    const int *tile_first;
    int nseg;
};

// the segment of tile `t`: last s with tile_first[s] <= t (segments without tiles never match: their range is empty)
__device__ __forceinline__ int prune_tile_segment(const prune_seg &S, int t) {
    int lo = 0, hi = S.nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (S.tile_first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Zeroes the four histograms of a call.  A kernel of the call's own and not a hipMemsetAsync: as a node of a recorded graph the runtime's fill
// left other values than 0 in the histograms on a replay that followed unrelated launches (tests/test_gpu_prune_edges.py, the replay test).
__global__ void __launch_bounds__(256) prune_clear_kernel(uint32_t *__restrict__ hist, size_t words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) hist[i] = 0u;
}

__global__ void __launch_bounds__(256) prune_hist_kernel(prune_seg S, const float *__restrict__ P, int pass, const uint32_t *__restrict__ prefix,
                                                         uint32_t *__restrict__ hist) {
    __shared__ uint32_t bins[256];
    const int tid = threadIdx.x;
    const int seg = prune_tile_segment(S, (int)blockIdx.x);
    const long long n = S.size[seg], e0 = (long long)((int)blockIdx.x - S.tile_first[seg]) * YK_PRUNE_TILE;
    const float *w = P + S.off[seg];
    const int shift = 24 - 8 * pass;
    const uint32_t want = pass ? prefix[seg] >> (shift + 8) : 0u;
    bins[tid] = 0;
    __syncthreads();
    uint32_t u[YK_PRUNE_TILE / 256];
#pragma unroll
    for (int j = 0; j < YK_PRUNE_TILE / 256; ++j) {                   // all loads of the tile in flight before the first LDS atomic
        const long long e = e0 + j * 256 + tid;
        u[j] = e < n ? (__float_as_uint(w[e]) & 0x7fffffffu) : 0xffffffffu;       // (bit 31 set: matches no prefix, not even the empty one)
    }
#pragma unroll
    for (int j = 0; j < YK_PRUNE_TILE / 256; ++j) {
        const bool in = pass ? ((u[j] >> (shift + 8)) == want) : !(u[j] >> 31);
        if (in) atomicAdd(&bins[(u[j] >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = bins[tid];
    if (c) atomicAdd(&hist[(size_t)seg * 256 + tid], c);
}

// state: prefix[nseg] then krem[nseg] (the rank still to find among the elements that share the prefix, counted from the largest)
__global__ void __launch_bounds__(256) prune_pick_kernel(prune_seg S, int pass, const uint32_t *__restrict__ hist, uint32_t *__restrict__ prefix,
                                                         uint32_t *__restrict__ krem, float *__restrict__ threshold, long long *__restrict__ kept) {
    __shared__ uint32_t bins[256];
    const int tid = threadIdx.x, seg = blockIdx.x;
    const uint32_t h = hist[(size_t)seg * 256 + tid];
    const long long n = S.size[seg];
    const long long kq = S.keep[seg];
    const uint32_t k0 = (uint32_t)(kq < 1 ? 1 : kq > n ? n : kq);    // keep is clamped to [1, n]
    const uint32_t k = pass ? krem[seg] : k0;
    const uint32_t pre = pass ? prefix[seg] : 0u;
    bins[tid] = h;
    __syncthreads();                                                  // (also: everybody has read the state before the one writer below)
    uint32_t above = 0;
    for (int j = tid + 1; j < 256; ++j) above += bins[j];
    if (above < k && k <= above + h) {                                // exactly one bin holds the k-th largest
        const uint32_t p = pre | ((uint32_t)tid << (24 - 8 * pass));
        prefix[seg] = p;
        krem[seg] = k - above;
        if (pass == 3) {
            threshold[seg] = __uint_as_float(p);
            kept[seg] = (long long)(k0 - (k - above)) + (long long)h;
        }
    }
}

__global__ void __launch_bounds__(256) prune_mask_kernel(prune_seg S, const float *__restrict__ P, const uint32_t *__restrict__ prefix,
                                                         uint8_t *__restrict__ mask) {
    const int tid = threadIdx.x;
    const int seg = prune_tile_segment(S, (int)blockIdx.x);
    const long long n = S.size[seg], e0 = (long long)((int)blockIdx.x - S.tile_first[seg]) * YK_PRUNE_TILE;
    const long long base = S.off[seg];
    const uint32_t thr = prefix[seg];
#pragma unroll
    for (int j = 0; j < YK_PRUNE_TILE / 256; ++j) {
        const long long e = e0 + j * 256 + tid;
        if (e < n) mask[base + e] = (__float_as_uint(P[base + e]) & 0x7fffffffu) >= thr ? 1 : 0;
    }
}

extern "C" int yk_prune_tile(void) { return YK_PRUNE_TILE; }

extern "C" int yk_prune_masks_f32(const float *params, const long long *d_offset, const long long *d_size, const long long *d_keep,
                                  const int *d_tile_first, int nseg, int ntiles, uint8_t *mask, float *d_threshold, long long *d_kept,
                                  void *stream) {
    if (!params || !d_offset || !d_size || !d_keep || !d_tile_first || nseg <= 0 || ntiles <= 0 || !mask || !d_threshold || !d_kept) {
        yk_set_error("yk_prune_masks_f32: bad argument");
        return YK_ERR_ARG;
    }
    int dev = yk_current_device();
    if (dev < 0) return YK_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    const size_t hist_words = (size_t)4 * nseg * 256;                // one histogram per pass: zeroed once, no pass waits for a clear
    uint32_t *ws = (uint32_t *)yk_scratch(dev, stream, YK_SLOT_PRUNE, sizeof(uint32_t) * (hist_words + 2 * (size_t)nseg));
    if (!ws) return YK_ERR_NOMEM;
    uint32_t *prefix = ws + hist_words, *krem = prefix + nseg;
    hipLaunchKernelGGL(prune_clear_kernel, dim3((unsigned)(hist_words / 256)), dim3(256), 0, st, ws, hist_words);
    YK_HIP(hipGetLastError());
    const prune_seg S{d_offset, d_size, d_keep, d_tile_first, nseg};
    for (int pass = 0; pass < 4; ++pass) {
        uint32_t *hist = ws + (size_t)pass * nseg * 256;
        hipLaunchKernelGGL(prune_hist_kernel, dim3(ntiles), dim3(256), 0, st, S, params, pass, (const uint32_t *)prefix, hist);
        YK_HIP(hipGetLastError());
        hipLaunchKernelGGL(prune_pick_kernel, dim3(nseg), dim3(256), 0, st, S, pass, (const uint32_t *)hist, prefix, krem, d_threshold, d_kept);
        YK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(prune_mask_kernel, dim3(ntiles), dim3(256), 0, st, S, params, (const uint32_t *)prefix, mask);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// p[i] = mask[i] ? p[i] : +0.0f.  Four elements per lane (16 B of parameters, 4 B of mask) when both pointers allow it; a group whose
// four mask bytes are all set is not written back.
__global__ void __launch_bounds__(256) mask_apply_vec_kernel(size_t n4, float4 *__restrict__ p, const uint32_t *__restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const uint32_t m = mask[i];
    if ((m & 0xffu) && (m & 0xff00u) && (m & 0xff0000u) && (m & 0xff000000u)) return;
    float4 v = p[i];
    if (!(m & 0xffu)) v.x = 0.f;
    if (!(m & 0xff00u)) v.y = 0.f;
    if (!(m & 0xff0000u)) v.z = 0.f;
    if (!(m & 0xff000000u)) v.w = 0.f;
    p[i] = v;
}
__global__ void __launch_bounds__(256) mask_apply_kernel(size_t first, size_t n, float *__restrict__ p, const uint8_t *__restrict__ mask) {
    const size_t i = first + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !mask[i]) p[i] = 0.f;
}
extern "C" int yk_mask_apply_f32(float *params, const uint8_t *mask, long long n, void *stream) {
    if (!params || !mask || n <= 0) {
        yk_set_error("yk_mask_apply_f32: bad argument");
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = !((uintptr_t)params & 15) && !((uintptr_t)mask & 3);
    const size_t n4 = vec ? (size_t)n / 4 : 0, rest = (size_t)n - 4 * n4;
    if (n4) {
        hipLaunchKernelGGL(mask_apply_vec_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, n4, (float4 *)params, (const uint32_t *)mask);
        YK_HIP(hipGetLastError());
    }
    if (rest) {
        hipLaunchKernelGGL(mask_apply_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, st, 4 * n4, (size_t)n, params, mask);
        YK_HIP(hipGetLastError());
    }
    return YK_OK;
}
