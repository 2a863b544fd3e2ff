// yk_common.h — shared helpers of libyolo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "yolo_hip.h"

#define YK_WAVE 64

// Tuning switches (YK_IGEMM_FORCE, YK_SPLIT_FORCE, YK_NS, YK_PIPE, ...) exist only in development builds (`make dev` or `make DEV=1`,
// -DYK_DEV): the shipped library never reads the environment on its launch path.  Rejected kernel variants are not kept here (git history).
#include <stdlib.h>
#ifdef YK_DEV
static inline const char *yk_dev_env(const char *name) { return getenv(name); }
#else
static inline const char *yk_dev_env(const char *) { return nullptr; }
#endif

// the few switches the shipped library does read, at plan creation only (README "Environment switches")
static inline bool yk_env_flag(const char *name, bool dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    return e[0] != '0';
}

void yk_set_error(const char *fmt, ...);

#define YK_HIP(call)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            yk_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));  \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? YK_ERR_NO_DEVICE  \
                                                                           : YK_ERR_HIP;      \
        }                                                                                      \
    } while (0)

// grow-only device scratch per (device, stream, slot); safe because work on one stream is ordered.  Two calls on one stream that name the
// same slot get the same buffer, so every slot of the library is named here and a new user takes a new name.  The numbers are the ones
// the callers always used.
enum yk_scratch_slot {
    YK_SLOT_DECODE = 0,           // yk_decode.hip: boxes, scores, selections and counts of one yk_decode call
    YK_SLOT_LOSS = 1,             // yk_loss.hip: the loss columns' partial sums per (image, chunk)
    YK_SLOT_DWW = 12,             // yk_train.hip: yk_dw3x3_bwd_weight_f32's partials per row chunk
    YK_SLOT_BN_PARTIAL = 13,      // yk_train.hip: BatchNorm / column-sum partials of every forward (yk_bn_train_fwd*, yk_*_bn_fwd_f32, yk_colsum_f32:
                                  // doubles) and of yk_bn_train_bwd_f32 (floats).  Shared on purpose: in stream order each call has folded its partials
                                  // before the next one writes them, and a captured step holds ONE buffer sized by its largest layer
    YK_SLOT_SPLITK = 14,          // yk_train.hip: the split-K slabs of every ungrouped GEMM (yk_gemm_f32, yk_gemm_bn_fwd_f32, yk_conv3x3_*_f32).  Shared
                                  // on purpose, for the same reason
    YK_SLOT_L2 = 15,              // yk_train.hip: yk_l2_segments_f32's partials per block
    YK_SLOT_NORMALISE = 16,       // yk_pre.hip: yk_normalise_u8's maximum per image
    YK_SLOT_SPLITK_GROUPED = 22,  // yk_train.hip: the slabs of all problems of one yk_gemm_f32_grouped call (its fallback calls use YK_SLOT_SPLITK)
    YK_SLOT_DWW_GROUPED = 23,     // yk_train.hip: the partials of all problems of one yk_dw3x3_bwd_weight_grouped_f32 call
    YK_SLOT_PRUNE = 24,           // yk_prune.hip: the histograms and thresholds of one magnitude-pruning call
    YK_SLOT_DISTILL = 25,         // yk_distill.hip: the distillation loss's partial sums per (image, chunk)
    YK_SLOT_TILES = 26,           // yk_tiles.hip: cursors, overflow lists, selections and counts of one yk_merge_tiles call
    YK_SLOT_TTA = 27,             // yk_tta.hip: the fused rows per (picture, class) and their counts of one yk_fuse_views call
};
void *yk_scratch(int device, void *stream, int slot, size_t bytes);
void yk_scratch_release_stream(void *stream);

// More than 64 KB of dynamic LDS needs the maximum-dynamic-LDS attribute on every kernel (instantiation) launched with it, on every
// device.  yk_allow_lds raises it for (current device, kern) when `bytes` exceeds what was set there; every launch whose dynamic LDS
// can exceed 64 KB goes through yk_launch_lds, which calls it.
void yk_allow_lds(const void *kern, size_t bytes);
template <typename... P, typename... A>
static inline void yk_launch_lds(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
    yk_allow_lds(reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
}

static inline int yk_current_device() {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) return -1;
    return d;
}

// Kernels that put a table row in blockIdx.y: grid.y holds at most 65535 rows, so n rows are launch(base, m) once per chunk - rows base ..
// base + m - 1, every pointer advanced by the caller - and one kernel node per chunk in a captured graph.
template <class Launch>
static inline void yk_for_grid_y(int n, Launch launch) {
    for (int base = 0; base < n; base += 65535) launch(base, n - base < 65535 ? n - base : 65535);
}

// A row whose picture has pixels and lies inside the src_bytes of its buffer.  Kernels do not trust their tables: any other row is not read.
__device__ __forceinline__ bool yk_ragged_row_inside(const yk_ragged_row_t &row, size_t src_bytes) {
    return row.h > 0 && row.w > 0 && row.offset <= src_bytes && (size_t)row.h * row.w * 3 <= src_bytes - row.offset;
}

__device__ __forceinline__ float yk_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// expf as glibc >= 2.27 computes it (sysdeps/ieee754/flt-32/e_expf.c, the ARM optimized-routines algorithm): x*32/ln2 = k + r,
// 2^(k/32) from a 32-entry table, a cubic in r, everything in double, ONE rounding to float at the end.  The reference's C path
// (region_layer.c:75,100,171-172) calls libm's expf on the host; evaluating the SAME approximation on the device makes the C-mode
// outputs bit-identical to it (the double-precision evaluation order only matters at the 2^-53 level, i.e. never for the final
// float; checked here against glibc 2.35 on 1.5e8 inputs: 0 mismatches).  Device libm's expf differs from glibc in ~1 ulp cases.
__device__ __forceinline__ float yk_expf_glibc(float x) {
    static constexpr unsigned long long T[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull,
        0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull,
        0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull,
        0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull,
        0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
        0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
    constexpr double N = 32.0, InvLn2N = 0x1.71547652b82fep+0 * N;
    constexpr double C0 = 0x1.c6af84b912394p-5 / N / N / N, C1 = 0x1.ebfce50fac4f3p-3 / N / N, C2 = 0x1.62e42ff0c52d6p-1 / N;
    if (x != x) return x + x;
    if (x > 0x1.62e42ep6f) return __builtin_huge_valf();
    if (x < -0x1.9fe368p6f) return 0.f;
    const double z = InvLn2N * (double)x;
    const double kd = rint(z);                       // round-half-even, as the 0x1.8p52 shift trick does
    const long long ki = (long long)kd;
    const double r = z - kd;
    const unsigned long long t = T[ki & 31] + ((unsigned long long)ki << 47);
    const double s = __longlong_as_double((long long)t);
    double y = C2 * r + 1.0;
    y = (C0 * r + C1) * (r * r) + y;
    return (float)(y * s);
}
