// yk_range.h — the order-preserving key of a float and the min / max accumulator over it, shared by the calibration kernels
// (yk_calib.hip) and the quantisation-aware training kernels (yk_qat.hip).
//
// The key of a float is its bit pattern with the sign bit flipped (positive values) or all bits flipped (negative values): unsigned
// comparison of keys is the total order -max < ... < -0 < +0 < ... < +max, so a min / max reduction is integer min / max - associative
// and commutative, hence bitwise independent of how workgroups are scheduled, of the launch geometry and of the stream; denormals are
// never flushed because no floating-point comparison touches them.  A NaN or an infinity does not enter the range: it sets a flag.
#pragma once
#include "yk_common.h"

namespace yk_range {

constexpr int CAL_BLOCK = 256;
constexpr int CAL_WAVES = CAL_BLOCK / YK_WAVE;
constexpr unsigned CAL_MAX_GRID = 2048;                  // 8 workgroups per CU: enough in flight to stream from HBM

__host__ __device__ __forceinline__ uint32_t key_of(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t unkey_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

struct Acc {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, bad = 0u;
    __device__ __forceinline__ void add(float v) {
        const uint32_t b = __float_as_uint(v);
        if ((b & 0x7F800000u) == 0x7F800000u) {          // inf or NaN
            bad = 1u;
            return;
        }
        const uint32_t k = key_of(b);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
};

// the workgroup's result (CAL_BLOCK threads) into the slot: one atomicMin + one atomicMax
__device__ __forceinline__ void fold(Acc a, uint32_t *slot) {
    __shared__ uint32_t s_lo[CAL_WAVES], s_hi[CAL_WAVES], s_bad[CAL_WAVES];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t l = __shfl_xor(a.lo, o, 64), h = __shfl_xor(a.hi, o, 64), f = __shfl_xor(a.bad, o, 64);
        a.lo = l < a.lo ? l : a.lo;
        a.hi = h > a.hi ? h : a.hi;
        a.bad |= f;
    }
    const int wave = threadIdx.x / YK_WAVE;
    if ((threadIdx.x & (YK_WAVE - 1)) == 0) {
        s_lo[wave] = a.lo;
        s_hi[wave] = a.hi;
        s_bad[wave] = a.bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t lo = s_lo[0], hi = s_hi[0], bad = s_bad[0];
#pragma unroll
        for (int w = 1; w < CAL_WAVES; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
            bad |= s_bad[w];
        }
        atomicMin(slot + 0, lo);
        atomicMax(slot + 1, hi);
        if (bad) atomicOr(slot + 2, 1u);
    }
}

inline unsigned grid_for(size_t items) {
    const size_t g = (items + CAL_BLOCK - 1) / CAL_BLOCK;
    return (unsigned)(g < 1 ? 1 : (g > CAL_MAX_GRID ? CAL_MAX_GRID : g));
}
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace yk_range
