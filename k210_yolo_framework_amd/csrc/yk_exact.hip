// yk_exact.hip — the "f16x2" precision mode of the engine: fp16 MFMA arithmetic with fp32-class accuracy.
//
// Why: BASELINE.json asks for fp16-MFMA convolutions AND outputs within 1e-3 of the fp32 Keras path with exact class / box
// indices.  fp16 STORAGE alone cannot give the second (a 20-layer chain of 2^-11 roundings drifts to ~2e-3 on the scores and NMS /
// threshold decisions flip).  This mode feeds the matrix cores with compensated operands:
//     x * 2^-e = x_hi + x_lo   (two fp16 values, 22 significant bits)
//     w * 2^s  = w_hi + w_lo   (split once on the host, s per layer)
//     acc += w_lo*x_hi + w_hi*x_lo + w_hi*x_hi        three v_mfma_f32_16x16x32_f16 per product, fp32 accumulate
// (the dropped w_lo*x_lo term is 2^-22 of the product).  Depthwise convs, pooling and the residual add run in fp32 on the VALU.
//
// Round 3: the split is done ONCE, BY THE PRODUCER.  Every activation tensor lives in HBM already split, NHWC with the channel axis in
// groups of eight: [pixel][c/8][hi x8 | lo x8] fp16 (32 bytes per group, the same bytes as fp32), scaled by a per-image STORAGE
// EXPONENT e.  A consumer GEMM therefore moves its operand tiles exactly like the fp16 plan does - `buffer_load ... lds` straight
// into an NS-deep LDS ring, no staging registers, no conversion in the loop (round 2 converted fp32 -> hi/lo in every consumer
// workgroup's loader: 915 us per batch; profiles/r02_f16x2_per_launch.txt).
//
// The storage exponent of a tensor has to be known BEFORE its values are: e = exponent of an a-priori BOUND of |output|, computed by
// the producing workgroup from the MEASURED per-image max of its inputs: bound = gain * amax(in) + offset with gain = max_n |scale_n|
// * sum_k |w_nk| (fixed at plan creation).  The bound over-estimates the real maximum by 2^6..2^8 in these networks; fp16 has a
// 5-bit exponent, so hi + lo keeps its 22 bits relative to the tensor maximum as long as the over-estimate stays below 2^16.  Each
// producer also measures the true per-image max of what it wrote (atomicMax into 64 sub-slots per image) for the NEXT layer's bound.
// Exponents are per image, never per batch, and every tiling decision is fixed at plan creation for max_batch: an image's results
// do not depend on its batch mates (tests/test_gpu_net.py::test_f16x2_is_per_image_and_deterministic).
//
// Concatenate([UpSampling2D(a), b]) feeds ONE GEMM from two tensors with two exponents: the K axis is ordered source-major, the
// accumulators are multiplied by 2^(e_a - e_b) (exact) where the walk crosses from a to b.
//
// Reference layers: Conv2D / DepthwiseConv2D / BatchNormalization / LeakyReLU / ReLU / MaxPooling2D / UpSampling2D / Concatenate /
// Add as built by models/yolonet.py:12-260, models/keras_mobilenet.py:291-436, models/keras_mobilenet_v2.py:426-485.
#include <algorithm>
#include <math.h>
#include <string>
#include <vector>

#include "yk_conv.h"
#include "yk_plan_graph.h"

namespace {

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define X_OOB 0x40000000u       // an offset no tensor reaches (tensors are < 1 GiB): buffer loads past num_records return zeros
// phase knock-out bits of the developer builds (tools/xbench.py, `make DEV=1`); a constant false in the shipped kernels
#ifdef YK_DEV
#define X_DBG(a, bit) (((a).dbg & (bit)) != 0)
#else
#define X_DBG(a, bit) false
#endif

extern __shared__ __attribute__((aligned(16))) unsigned char xsm[];

// activation min(max(v, v * slope), cap) as ONE median.  Valid for the combinations the reference networks use - leaky / linear layers
// (slope in (0, 1], cap = +inf: median(v, v*slope, inf) = max) and ReLU / ReLU6 (slope 0, cap >= 0: median(v, 0, cap) = clamp) - NOT for a
// capped leaky activation (v = 20, slope 0.5, cap 6: the median is 10): yk_xplan_create refuses that combination
__device__ __forceinline__ float x_actf(float v, float slope, float cap) { return __builtin_amdgcn_fmed3f(v, v * slope, cap); }
__device__ __forceinline__ uint32_t x_div(uint32_t n, yk_fastdiv d) { return (__umulhi(n, d.mul) + n) >> d.shift; }

// exponent e with bound * 2^-e in [2^13, 2^14); bound given as float bits (0 / inf / nan -> e = 0)
__device__ __forceinline__ int x_exp_of(uint32_t bits) {
    const int be = (int)((bits >> 23) & 0xffu);
    if (be == 0 || be == 255) return 0;
    return be - 127 - 13;
}
__device__ __forceinline__ float x_pow2(int e) { return __uint_as_float((uint32_t)(127 + max(-126, min(127, e))) << 23); }

// bijective XCD-aware remap of a 1-D tile index (block b runs on XCD b % 8): consecutive tiles land on the same XCD's L2
__device__ __forceinline__ int x_xcd_tile(int bid, int nt) {
    const int q = nt >> 3, r = nt & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Per-image running maxima live in XS = 64 sub-slots per image: thousands of workgroups hitting ONE address with a device-scope atomic
// serialise at ~0.25 us each across the XCDs (measured in round 2: 3/4 of every kernel's time).  A workgroup fires one no-return
// atomic at slot blockIdx.x % 64; a reader wave loads the 64 slots of an image with one coalesced access and reduces them.
constexpr int XS = 64;
__device__ __forceinline__ void x_amax_global(uint32_t *img_slots, uint32_t bits) { atomicMax(img_slots + (blockIdx.x & (XS - 1)), bits); }
__device__ __forceinline__ float x_amax_wave(const uint32_t *base, int b) {   // whole wave: every lane returns image b's max
    uint32_t v = base[(size_t)b * XS + (threadIdx.x & 63)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return __uint_as_float(v);
}
// wave-wide max into an LDS slot: one atomic per wave when every lane targets the same slot (the common case: one image per tile)
__device__ __forceinline__ void x_amax_lds(uint32_t *simg, int slot, float v) {
    const int s0 = __builtin_amdgcn_readfirstlane(slot);
    if (__all(slot == s0)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        if ((threadIdx.x & 63) == 0 && v > 0.f) atomicMax(&simg[s0], __float_as_uint(v));
    } else if (v > 0.f) {
        atomicMax(&simg[slot], __float_as_uint(v));
    }
}

// One stored activation tensor as a kernel sees it: [B][H][W][G][hi x8 | lo x8] fp16, values = x * 2^-eexp[b]
struct xview {
    const uint8_t *p;
    const int *eexp;            // [max_batch] storage exponent per image (written by the producer)
    const uint32_t *amax;       // [max_batch][XS] float bits of the true per-image max |x| (written by the producer)
    uint32_t bytes;             // whole tensor, for the buffer descriptor
    int G, H, W;                // channel groups of 8, stored height / width
};

// acc += f16(lo | hi half of a) * w: one VALU op, fp32 accumulate, no conversion instruction
__device__ __forceinline__ void x_fma_mix_lo(float &acc, uint32_t a, float w) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(a), "v"(w));
}
__device__ __forceinline__ void x_fma_mix_hi(float &acc, uint32_t a, float w) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(a), "v"(w));
}
// f16(lo | hi halves of h) + f16(same half of l) as fp32: the stored pair (hi, lo) of one channel back in one register, one VALU op
__device__ __forceinline__ float x_mix_sum_lo(uint32_t h, uint32_t l) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    return r;
}
__device__ __forceinline__ float x_mix_sum_hi(uint32_t h, uint32_t l) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    return r;
}
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void x_split(float s, yk_half &hi, yk_half &lo) {
    hi = (yk_half)s;
    lo = (yk_half)(s - (float)hi);
}
// the same split for a pair: one packed conversion per half pair, the residual s - hi (exact in fp32) by one mixed-precision op that reads
// hi straight out of the packed register - 2 VALU ops per value instead of 4, bit-identical results
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void x_split2(float a, float b, uint32_t &hi2, uint32_t &lo2) {
    const half2v h = {(_Float16)a, (_Float16)b};
    hi2 = __builtin_bit_cast(uint32_t, h);
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(hi2), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(hi2), "v"(b));
    const half2v l = {(_Float16)ra, (_Float16)rb};
    lo2 = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ void x_split4(const float *v, half4 &hi, half4 &lo) {
    uint32_t h0, h1, l0, l1;
    x_split2(v[0], v[1], h0, l0);
    x_split2(v[2], v[3], h1, l1);
    hi = __builtin_bit_cast(half4, u32x2{h0, h1});
    lo = __builtin_bit_cast(half4, u32x2{l0, l1});
}
__device__ __forceinline__ void x_split8(const float *v, half8 &hi, half8 &lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x_split2(v[2 * j], v[2 * j + 1], h[j], l[j]);
    hi = __builtin_bit_cast(half8, u32x4{h[0], h[1], h[2], h[3]});
    lo = __builtin_bit_cast(half8, u32x4{l[0], l[1], l[2], l[3]});
}

// =====================================================================================================================
// xg_kernel: Conv2D 1x1 / 3x3 (stride 1|2, explicit top/left pad) over [up2(src0), src1] as C[M,N] = A[M,K] * W[N,K]^T with
// compensated operands.  K is walked in steps of 32 (one MFMA); a step's operand tiles are
//     A: BM/16 row blocks x {hi, lo} x [16 rows][64 B]      B: BN/16 row blocks x {hi, lo} x [16 rows][64 B]
// i.e. 1 KB pieces, each deposited by ONE `buffer_load_dwordx4 ... lds` wave-instruction (lane l -> row l>>2, 16-byte position l&3).
// The fragment read `ds_read_b128` (lane = row fr, k-chunk fq) is conflict-free with the chunk stored at position chunk ^ ((row>>1)&3)
// (tools/lds_sim.py, tests/test_lds_model.py): the A lanes apply that XOR to the chunk they FETCH, the weights are stored that way
// by the host (tile order [step][16-row block][hi|lo][16][32], so a B piece is a linear 1 KB copy).
// Pipeline as yk_igemm_pipe.h: NS stages, one raw s_barrier per step, counted vmcnt, no branches in the loop body.
// =====================================================================================================================
struct xg_args {
    xview s0, s1, res;          // s1.p / res.p null when absent
    int up0;                    // s0 is read through UpSampling2D(2)
    int Hi, Wi, Ho, Wo, ks, stride, pad_t, pad_l;
    int B, M, N, HoWo;
    int taps, nc0, nc1;         // k-steps of 32 per tap in segment 0 / 1 (ceil(G/4); nc1 = 0 without concat)
    const uint8_t *w;           // [nsteps][nslab][2][16][32] halfs (w * 2^s split, position-swizzled)
    uint32_t w_bytes;
    int nslab;                  // 16-row blocks, padded to a whole number of N tiles
    const float *scale, *bias;  // [N padded with zeros]; scale already carries 2^-s
    float slope, cap;
    float gain0, gain1, off;    // |conv output before act| <= gain0*amax(s0) + gain1*amax(s1) + off
    uint8_t *out;               // split tensor, or null for a network output
    int dst_f32;                // ... stored as fp32 planes [pixel][group][ch 0-3 | ch 4-7], exponent 0: its only reader is a depthwise conv
    int outG;
    float *out32;               // network output [M][N] fp32 (exact pitch)
    int *eexp_out;
    uint32_t *amax_out;
    yk_fastdiv fd_hw, fd_wo;
    int splitk;
    float *slab;                // split-K partial sums [z][tile][reg][thread] floatx4
    int dbg;                    // developer builds: phase knock-out bits (tools/xbench.py), 0 in production
};

template <int BM, int BN, int WM, int WN>
struct xg_cfg {
    static constexpr int NW = WM * WN, NT = 64 * NW;
    static constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    static constexpr int STAGE = (BM + BN) * 128;                 // bytes of one ring stage
    static constexpr int CPITCH = BN * 4 + 16;                    // output staging: [BM][BN/8 groups][32 B] + pad
    static constexpr int CT = BM * CPITCH;
    static constexpr int SMALL = 5 * BM * 4;                      // per-image factors of the tile
    static constexpr int lds(int ns) { return (ns * STAGE > CT ? ns * STAGE : CT) + SMALL; }
};

// per-image factors of the tile's images b0..bl -> LDS (one wave per image): operand exponents in, storage exponent out
template <int BM, int NW>
__device__ __forceinline__ void xg_prep(const xg_args &a, int b0, int bl, float *s_up, float *s_resc, float *s_down, float *s_rup,
                                        uint32_t *s_amax) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int b = b0 + wid; b <= bl; b += NW) {
        float bound = a.gain0 * x_amax_wave(a.s0.amax, b) + a.off;
        const int e0 = a.s0.eexp[b];
        int e1 = e0;
        if (a.s1.p) {
            bound += a.gain1 * x_amax_wave(a.s1.amax, b);
            e1 = a.s1.eexp[b];
        }
        bound = fminf(bound, a.cap);
        float rup = 0.f;
        if (a.res.p) {
            bound += x_amax_wave(a.res.amax, b);
            rup = x_pow2(a.res.eexp[b]);
        }
        const int eo = a.dst_f32 ? 0 : x_exp_of(__float_as_uint(bound));
        if (lane == 0) {
            s_up[b - b0] = x_pow2(e1);
            s_resc[b - b0] = x_pow2(e0 - e1);
            s_down[b - b0] = x_pow2(-eo);
            s_rup[b - b0] = rup;
            s_amax[b - b0] = 0u;
            if (a.eexp_out) a.eexp_out[b] = eo;                   // every workgroup of the image writes the same value
        }
    }
}

// epilogue: lane holds channels n..n+3 (acc regs) of GEMM row (wm*TM+i)*16 + fr
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void xg_epilogue(const xg_args &a, floatx4 (&acc)[BM / WM / 16][BN / WN / 16], int m0, int n0, int b0, int bl,
                                            const int (&rowb)[BM / WM / 16], const float4 (&sc)[BN / WN / 16], const float4 (&bs)[BN / WN / 16],
                                            const float *s_up, const float *s_down, const float *s_rup, uint32_t *s_amax) {
    typedef xg_cfg<BM, BN, WM, WN> C;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN, fr = lane & 15, nl4 = (lane >> 4) * 4;
    unsigned char *Cs = xsm;
#pragma unroll
    for (int i = 0; i < C::TM; ++i) {
        const int r = (wm * C::TM + i) * 16 + fr, m = m0 + r;
        const bool mok = m < a.M;
        const int bi = rowb[i];
        const float up = s_up[bi], down = s_down[bi], rup = s_rup[bi];
        float rmax = 0.f;
#pragma unroll
        for (int j = 0; j < C::TN; ++j) {
            const int nl = (wn * C::TN + j) * 16 + nl4, n = n0 + nl;
            float v[4];
            v[0] = x_actf(__builtin_fmaf(acc[i][j][0] * up, sc[j].x, bs[j].x), a.slope, a.cap);
            v[1] = x_actf(__builtin_fmaf(acc[i][j][1] * up, sc[j].y, bs[j].y), a.slope, a.cap);
            v[2] = x_actf(__builtin_fmaf(acc[i][j][2] * up, sc[j].z, bs[j].z), a.slope, a.cap);
            v[3] = x_actf(__builtin_fmaf(acc[i][j][3] * up, sc[j].w, bs[j].w), a.slope, a.cap);
            if (a.out32) {
                if (mok) {
                    float *o = a.out32 + (size_t)m * a.N + n;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (n + k < a.N) o[k] = v[k];
                }
                continue;
            }
            if (a.dst_f32) {                                       // 16 contiguous bytes per lane, 64 per pixel and channel block: no staging
                if (mok && (n >> 3) < a.outG) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) rmax = fmaxf(rmax, fabsf(v[k]));
                    *reinterpret_cast<u32x4 *>(a.out + ((size_t)m * a.outG + (n >> 3)) * 32 + ((n >> 2) & 1) * 16) =
                        u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
                }
                continue;
            }
            if (a.res.p && mok && (n >> 3) < a.res.G) {
                const uint8_t *q = a.res.p + ((size_t)m * a.res.G + (n >> 3)) * 32 + (n & 7) * 2;
                const half4 rh = *reinterpret_cast<const half4 *>(q), rl = *reinterpret_cast<const half4 *>(q + 16);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] += ((float)rh[k] + (float)rl[k]) * rup;
            }
            half4 hi, lo;
            float vd[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (mok) rmax = fmaxf(rmax, fabsf(v[k]));
                vd[k] = v[k] * down;
            }
            x_split4(vd, hi, lo);
            unsigned char *d = Cs + r * C::CPITCH + (nl >> 3) * 32 + (nl & 7) * 2;
            *reinterpret_cast<half4 *>(d) = hi;
            *reinterpret_cast<half4 *>(d + 16) = lo;
        }
        if (a.amax_out) x_amax_lds(s_amax, bi, rmax);
    }
    if (a.out32) return;
    __syncthreads();
    if (a.dst_f32) {
        if (a.amax_out && tid <= bl - b0 && s_amax[tid]) x_amax_global(a.amax_out + (size_t)(b0 + tid) * XS, s_amax[tid]);
        return;
    }
    // 16 bytes per lane, row-contiguous: a pixel's BN channels are BN*4 bytes in a row of the output tensor
    constexpr int VPR = BN / 4;
    for (int v = tid; v < BM * VPR; v += C::NT) {
        const int r = v / VPR, cv = v - r * VPR, m = m0 + r;
        const int g = (n0 >> 3) + (cv >> 1);
        if (m < a.M && g < a.outG)
            *reinterpret_cast<u32x4 *>(a.out + ((size_t)m * a.outG + g) * 32 + (cv & 1) * 16) =
                *reinterpret_cast<const u32x4 *>(Cs + r * C::CPITCH + cv * 16);
    }
    if (a.amax_out && tid <= bl - b0 && s_amax[tid]) x_amax_global(a.amax_out + (size_t)(b0 + tid) * XS, s_amax[tid]);
}

template <int N>
__device__ __forceinline__ void x_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

template <int BM, int BN, int WM, int WN, int NS, bool PART>
__global__ void __launch_bounds__(64 * WM * WN) xg_kernel(const xg_args a) {
    typedef xg_cfg<BM, BN, WM, WN> C;
    constexpr int NW = C::NW, TM = C::TM, TN = C::TN;
    constexpr int A_IT = (BM / 16 * 2) / NW, B_IT = (BN / 16 * 2) / NW, L = A_IT + B_IT, AR = A_IT / 2;
    static_assert((BM / 16 * 2) % NW == 0 && (BN / 16 * 2) % NW == 0 && A_IT % 2 == 0, "1 KB pieces must divide among the waves");
    static_assert(NS >= 2 && (NS - 2) * L <= 63, "vmcnt is a 6-bit counter");
    constexpr int BIG = C::lds(NS) - C::SMALL;
    float *s_up = reinterpret_cast<float *>(xsm + BIG), *s_resc = s_up + BM, *s_down = s_resc + BM, *s_rup = s_down + BM;
    uint32_t *s_amax = reinterpret_cast<uint32_t *>(s_rup + BM);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    // XCD-aware walk of the 3-D grid
    const int gx = gridDim.x, gy = gridDim.y;
    const int L0 = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int v = x_xcd_tile(L0, gx * gy * gridDim.z);
    // N tile fastest: the N tiles of one M tile run back to back on one XCD, so the A rows they all read come out of that L2 (with M
    // fastest a 384 -> 384 pointwise conv fetched its input three times from the fabric: 57 MB for 27.5)
    const int vz = v / (gx * gy), vr = v - vz * (gx * gy), vx = vr / gy, vy = vr - vx * gy;
    const int m0 = vx * BM, n0 = vy * BN;
    const int b0 = (int)x_div((uint32_t)m0, a.fd_hw), bl = (int)x_div((uint32_t)min(a.M - 1, m0 + BM - 1), a.fd_hw);
    // BatchNorm scale / bias of this lane's channels: requested first, used last (the epilogue would otherwise open with a cold miss)
    float4 sc[TN], bs[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 16 + (lane >> 4) * 4;
        sc[j] = *reinterpret_cast<const float4 *>(a.scale + n);
        bs[j] = *reinterpret_cast<const float4 *>(a.bias + n);
    }

    // K range of this split: steps [kt0, kt0 + nk) of the walk  seg 0: tap-major over s0   |   seg 1: tap-major over s1
    const int kb = a.taps * a.nc0, nk_all = kb + a.taps * a.nc1;
    const int per = (nk_all + a.splitk - 1) / a.splitk;
    const int kt0 = vz * per, nk = X_DBG(a, 1) ? 0 : max(0, min(per, nk_all - kt0));
    const int lim = kt0 + nk;

    // ---- this lane's A rows (fixed over the walk): row l>>2 of the 16-row blocks wid*AR + it, fetching chunk (l&3) ^ ((row>>1)&3)
    const int lr = lane >> 2, lc = (lane & 3) ^ ((lr >> 1) & 3);
    const int G0 = a.s0.G, G1 = a.s1.G, W0 = a.s0.W;
    uint32_t P0[AR], P1[AR], rmask[AR];
    int ry[AR], rx[AR];
#pragma unroll
    for (int it = 0; it < AR; ++it) {
        const int m = m0 + (wid * AR + it) * 16 + lr;
        const bool ok = m < a.M;
        const uint32_t mm = ok ? m : 0;
        const uint32_t b = x_div(mm, a.fd_hw), rem = mm - b * a.HoWo;
        const uint32_t oy = x_div(rem, a.fd_wo), ox = rem - oy * a.Wo;
        const int ry0 = (int)oy * a.stride - a.pad_t, rx0 = (int)ox * a.stride - a.pad_l;
        ry[it] = ry0;
        rx[it] = rx0;
        if (a.up0) P0[it] = b * (uint32_t)(a.s0.H * W0 * G0 * 32) + lc * 32u;
        else P0[it] = b * (uint32_t)(a.Hi * a.Wi * G0 * 32) + (uint32_t)((ry0 * a.Wi + rx0) * G0 * 32) + lc * 32u;
        P1[it] = b * (uint32_t)(a.Hi * a.Wi * G1 * 32) + (uint32_t)((ry0 * a.Wi + rx0) * G1 * 32) + lc * 32u;
        uint32_t msk = 0;
        for (int t = 0; t < a.taps; ++t) {
            const int ky = (a.ks == 3) ? t / 3 : 0, kx = t - ky * a.ks;
            if (ok && (unsigned)(ry0 + ky) < (unsigned)a.Hi && (unsigned)(rx0 + kx) < (unsigned)a.Wi) msk |= 1u << t;
        }
        rmask[it] = msk;
    }
    // the last step of a tap may run past the tensor's channel groups (G not a multiple of 4): those chunks are zeros
    const bool lastbad0 = ((a.nc0 - 1) * 4 + lc) >= G0, lastbad1 = a.nc1 > 0 && ((a.nc1 - 1) * 4 + lc) >= G1;
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void *)a.s0.p, 0, a.s0.bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void *)(a.s1.p ? a.s1.p : a.s0.p), 0, a.s1.p ? a.s1.bytes : a.s0.bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void *)a.w, 0, a.w_bytes, 0x00020000);

    // walk state (uniform): segment, channel step inside the segment, tap.  The TAP is the fastest index: the nine taps of a channel
    // step re-read the same 128-byte pieces of neighbouring pixels within nine consecutive steps, i.e. out of L2 / L1 (with the tap as
    // the outer index a piece came back after a whole pass over the channels and had to be fetched from the fabric again: the 3x3 head
    // convs moved 25x their algorithmic bytes, profiles/r03_x2_kernel_trace_per_launch.csv first version)
    int step = kt0, seg, tap, cs;
    if (kt0 < kb) {
        seg = 0;
        cs = kt0 / a.taps;
        tap = kt0 - cs * a.taps;
    } else {
        seg = 1;
        const int r = kt0 - kb;
        cs = r / a.taps;
        tap = r - cs * a.taps;
    }
    uint32_t aoff[AR];
    auto retap = [&]() {
        const int ky = (a.ks == 3) ? (tap * 11) >> 5 : 0, kx = tap - ky * a.ks;        // tap / 3 for tap < 9+
        const bool tlive = tap < a.taps;
#pragma unroll
        for (int it = 0; it < AR; ++it) {
            const bool ok = tlive && ((rmask[it] >> tap) & 1u);
            uint32_t o;
            if (seg) o = P1[it] + (uint32_t)((ky * a.Wi + kx) * G1 * 32);
            else if (a.up0) o = P0[it] + (uint32_t)((((ry[it] + ky) >> 1) * W0 + ((rx[it] + kx) >> 1)) * G0 * 32);
            else o = P0[it] + (uint32_t)((ky * a.Wi + kx) * G0 * 32);
            aoff[it] = ok ? o : X_OOB;
        }
    };
    retap();
    const uint32_t wbase = (uint32_t)(n0 >> 4) * 2048u + (uint32_t)(wid * B_IT) * 1024u + lane * 16u, wstep = (uint32_t)a.nslab * 2048u;
    // one step's DMA = prepare (uniform offsets) + A_IT + B_IT pieces + advance (walk state)
    uint32_t d_cso = 0, d_ws = 0;
    auto dma_prepare = [&]() {
        const bool live = step < lim;
        const int nc = seg ? a.nc1 : a.nc0;
        const bool bad = !live || (cs == nc - 1 && (seg ? lastbad1 : lastbad0));
        d_cso = bad ? X_OOB : (uint32_t)cs * 128u;
        d_ws = live ? wbase + (uint32_t)step * wstep : X_OOB;
    };
    auto dma_piece = [&](int stage, int n) {                       // n: a compile-time constant after unrolling
        unsigned char *As = xsm + stage * C::STAGE, *Bs = As + BM * 128;
        if (n < A_IT) {
            const uint32_t o = aoff[(n >> 1) < AR ? (n >> 1) : 0] + d_cso + (uint32_t)(n & 1) * 16u;
            lds_ptr_t dsta = (lds_ptr_t)(As + (wid * A_IT + n) * 1024);
            if (seg) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, dsta, 16, o, 0, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, dsta, 16, o, 0, 0, 0);
            }
        } else {
            const int it = n - A_IT;
            const uint32_t ob = d_ws + (uint32_t)it * 1024u;
            lds_ptr_t dstb = (lds_ptr_t)(Bs + (wid * B_IT + it) * 1024);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, dstb, 16, ob, 0, 0, 0);
        }
    };
    auto dma_advance = [&]() {
        ++step;
        ++tap;
        if (tap >= a.taps) {                                       // uniform
            tap = 0;
            ++cs;
            if (!seg && cs >= a.nc0 && a.nc1 > 0) {
                seg = 1;
                cs = 0;
            }
        }
        if (a.taps > 1 || cs == 0) retap();                        // 1x1: the row offsets only change with the segment
    };
    auto dma = [&](int stage) {
        dma_prepare();
#pragma unroll
        for (int n = 0; n < L; ++n) {
            dma_piece(stage, n);
        }
        dma_advance();
    };
    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    const int foff = fr * 64 + ((fq ^ ((fr >> 1) & 3)) * 16);
    auto compute = [&](int stage) {
        const unsigned char *As = xsm + stage * C::STAGE, *Bs = As + BM * 128;
        half8 xh[TM], xl[TM], wh[TN], wl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            xh[i] = *reinterpret_cast<const half8 *>(As + ((wm * TM + i) * 2) * 1024 + foff);
            xl[i] = *reinterpret_cast<const half8 *>(As + ((wm * TM + i) * 2 + 1) * 1024 + foff);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            wh[j] = *reinterpret_cast<const half8 *>(Bs + ((wn * TN + j) * 2) * 1024 + foff);
            wl[j] = *reinterpret_cast<const half8 *>(Bs + ((wn * TN + j) * 2 + 1) * 1024 + foff);
        }
        // the three products of a tile go out as three sweeps over the accumulators: consecutive MFMAs never share one
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], xh[i], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xl[i], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xh[i], acc[i][j], 0, 0, 0);
    };
    // image of each accumulator row (relative to b0)
    int rowb[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) rowb[i] = (int)x_div((uint32_t)min(a.M - 1, m0 + (wm * TM + i) * 16 + fr), a.fd_hw) - b0;

#pragma unroll
    for (int s = 0; s < NS - 1; ++s) dma(s);                       // steps past `lim` deposit zeros and keep the vmcnt arithmetic uniform
    if (!X_DBG(a, 2)) xg_prep<BM, NW>(a, b0, bl, s_up, s_resc, s_down, s_rup, s_amax);   // slot loads fly with the prologue DMAs
    bool in0 = a.nc1 > 0 && kt0 < kb;                               // accumulators still in src0's units
    auto rescale = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float f = s_resc[rowb[i]];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] *= f;
        }
    };
    int rd = 0, wr = NS - 1;
    for (int kt = 0; kt < nk; ++kt) {
        x_wait_vm<(NS - 2) * L>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (in0 && kt0 + kt == kb) {                               // uniform, at most once: the walk crosses from src0 to src1
            rescale();
            in0 = false;
        }
        dma(wr);
        if (!X_DBG(a, 16)) compute(rd);
        rd = (rd + 1 == NS) ? 0 : rd + 1;
        wr = (wr + 1 == NS) ? 0 : wr + 1;
    }
    x_wait_vm<0>();                                                // drain the dead prefetches before LDS is reused
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (in0) rescale();
    if constexpr (PART) {
        const size_t tile = (size_t)vy * gx + vx, ntile = (size_t)gx * gy;
        floatx4 *mine = reinterpret_cast<floatx4 *>(a.slab) + ((size_t)vz * ntile + tile) * (TM * TN) * C::NT + tid;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) mine[(i * TN + j) * C::NT] = acc[i][j];
    } else {
        if (!X_DBG(a, 4)) xg_epilogue<BM, BN, WM, WN>(a, acc, m0, n0, b0, bl, rowb, sc, bs, s_up, s_down, s_rup, s_amax);
    }
}

// second phase of split-K: the partial sums of a tile are added in z order (deterministic) and finished like an unsplit tile
template <int BM, int BN, int WM, int WN>
__global__ void __launch_bounds__(64 * WM * WN) xg_reduce_kernel(const xg_args a) {
    typedef xg_cfg<BM, BN, WM, WN> C;
    constexpr int TM = C::TM, TN = C::TN;
    float *s_up = reinterpret_cast<float *>(xsm + C::CT), *s_resc = s_up + BM, *s_down = s_resc + BM, *s_rup = s_down + BM;
    uint32_t *s_amax = reinterpret_cast<uint32_t *>(s_rup + BM);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid / WN, fr = lane & 15;
    const int gx = gridDim.x, gy = gridDim.y;
    const int v = x_xcd_tile(blockIdx.x + gx * blockIdx.y, gx * gy);
    const int vx = v / gy, vy = v - vx * gy;
    const int m0 = vx * BM, n0 = vy * BN;
    const int b0 = (int)x_div((uint32_t)m0, a.fd_hw), bl = (int)x_div((uint32_t)min(a.M - 1, m0 + BM - 1), a.fd_hw);
    // BatchNorm scale / bias of this lane's channels: requested first, used last (the epilogue would otherwise open with a cold miss)
    float4 sc[TN], bs[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + ((wid % WN) * TN + j) * 16 + (lane >> 4) * 4;
        sc[j] = *reinterpret_cast<const float4 *>(a.scale + n);
        bs[j] = *reinterpret_cast<const float4 *>(a.bias + n);
    }
    xg_prep<BM, C::NW>(a, b0, bl, s_up, s_resc, s_down, s_rup, s_amax);
    int rowb[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) rowb[i] = (int)x_div((uint32_t)min(a.M - 1, m0 + (wm * TM + i) * 16 + fr), a.fd_hw) - b0;
    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const size_t tile = (size_t)vy * gx + vx, ntile = (size_t)gx * gy;
    for (int z = 0; z < a.splitk; ++z) {
        const floatx4 *src = reinterpret_cast<const floatx4 *>(a.slab) + ((size_t)z * ntile + tile) * (TM * TN) * C::NT + tid;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += __builtin_nontemporal_load(src + (i * TN + j) * C::NT);
    }
    __syncthreads();
    xg_epilogue<BM, BN, WM, WN>(a, acc, m0, n0, b0, bl, rowb, sc, bs, s_up, s_down, s_rup, s_amax);
}

// =====================================================================================================================
// xdw_kernel: DepthwiseConv2D 3x3 + BN + activation, fp32 on the VALU, input PATCH staged by LDS-DMA.
// A workgroup owns TH x TW output pixels x GS channel groups of one image.  Its input patch ((TH-1)s+3 rows x (TW-1)s+3 columns x GS
// groups) arrives in ONE burst of `buffer_load ... lds`: every lane computes the source address of the 16 bytes that belong at its
// linear LDS position (hi halves in one region, lo halves in another, so a tap read is a conflict-free ds_read_b128); pixels
// outside the image get an out-of-range offset and arrive as zeros - Keras zero padding costs nothing.  A thread keeps ONE channel
// group for all of its pixels (blockDim is a multiple of GS), so the nine tap weights, scale and bias of its eight channels live in
// registers, fetched while the patch is in flight.  (Round 3, first version: one thread = one output pixel, taps by buffer loads,
// the whole [11][C] parameter table copied to LDS by every workgroup - at 384 channels that copy was most of the kernel: 16 us for
// 27.5 MB.)
// =====================================================================================================================
struct xdw_args {
    xview in;
    int B, Ho, Wo, stride, pad_t, pad_l;
    const float *par;                  // [11][Cp] fp32: nine taps, scale, bias
    float slope, cap, gain, off;       // |out| <= min(cap, gain * amax(in) + off)
    uint8_t *out;
    int *eexp_out;
    uint32_t *amax_out;
    // geometry, fixed at plan creation
    int TH, TW, PH, PW, GS, gsl, tiles_x, tiles_y, NT, n16, n16p;
    int dbg;
    int in_f32;                        // the input is stored as fp32 planes (its only reader is this kernel): the taps read floats
    yk_fastdiv fd_gsl, fd_tpi, fd_tx, fd_gs, fd_pw, fd_tw;
};
__global__ void __launch_bounds__(256, 4) xdw_kernel(const xdw_args a) {   // <= 128 registers: four workgroups per CU (the patch is <= 40 KB)
    __shared__ uint32_t smax;
    __shared__ float sf[2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, G = a.in.G, Cp = G * 8, s = a.stride;
    unsigned char *HI = xsm, *LO = xsm + (size_t)a.n16p * 16;
    // block -> (image, tile, group slice)
    const uint32_t bid = blockIdx.x;
    const uint32_t tl_all = x_div(bid, a.fd_gsl), gsi = bid - tl_all * a.gsl;
    const uint32_t b = x_div(tl_all, a.fd_tpi), tl = tl_all - b * (a.tiles_x * a.tiles_y);
    const uint32_t ty = x_div(tl, a.fd_tx), tx = tl - ty * a.tiles_x;
    const int oy0 = (int)ty * a.TH, ox0 = (int)tx * a.TW, g0 = (int)gsi * a.GS;
    const int iy0 = oy0 * s - a.pad_t, ix0 = ox0 * s - a.pad_l;
    // (1) the patch, by DMA (full waves only: an inactive lane would leave its 16 bytes unwritten)
    {
        const uint32_t img = (uint32_t)a.in.H * a.in.W * G * 32u;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.in.p + (size_t)b * img), 0, img, 0x00020000);
        const int nwf = a.NT >> 6;
        if (wid < nwf && !X_DBG(a, 1))
            for (int q0 = wid * 64; q0 < a.n16p; q0 += nwf * 64) {
                const uint32_t q = q0 + lane;
                const uint32_t pos = x_div(q, a.fd_gs), g = q - pos * a.GS;
                const uint32_t r = x_div(pos, a.fd_pw), c = pos - r * a.PW;
                const int iy = iy0 + (int)r, ix = ix0 + (int)c;
                const bool ok = (int)q < a.n16 && (unsigned)iy < (unsigned)a.in.H && (unsigned)ix < (unsigned)a.in.W;
                const uint32_t oh = ok ? (uint32_t)(((iy * a.in.W + ix) * G + g0 + (int)g) * 32) : X_OOB, ol = oh + 16u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(HI + (size_t)q0 * 16), 16, oh, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(LO + (size_t)q0 * 16), 16, ol, 0, 0, 0);
            }
    }
    // (2) this thread's channel group: weights, scale, bias -> registers (in flight with the patch)
    const int gl = tid % a.GS, p0 = tid / a.GS, PP = a.NT / a.GS;
    const float *wp = a.par + (size_t)(g0 + gl) * 8;
    float4 w0[9], w1[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        w0[t] = *reinterpret_cast<const float4 *>(wp + (size_t)t * Cp);
        w1[t] = *reinterpret_cast<const float4 *>(wp + (size_t)t * Cp + 4);
    }
    const float4 sc0 = *reinterpret_cast<const float4 *>(wp + (size_t)9 * Cp), sc1 = *reinterpret_cast<const float4 *>(wp + (size_t)9 * Cp + 4);
    const float4 bs0 = *reinterpret_cast<const float4 *>(wp + (size_t)10 * Cp), bs1 = *reinterpret_cast<const float4 *>(wp + (size_t)10 * Cp + 4);
    if (tid < 64) {
        const float bound = fminf(a.cap, a.gain * x_amax_wave(a.in.amax, (int)b) + a.off);
        const int eo = x_exp_of(__float_as_uint(bound));
        if (tid == 0) {
            smax = 0u;
            sf[0] = x_pow2(a.in.eexp[b]);
            sf[1] = x_pow2(-eo);
            a.eexp_out[b] = eo;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float up = sf[0], down = sf[1];
    const float sc[8] = {sc0.x * up, sc0.y * up, sc0.z * up, sc0.w * up, sc1.x * up, sc1.y * up, sc1.z * up, sc1.w * up};
    const float bs[8] = {bs0.x, bs0.y, bs0.z, bs0.w, bs1.x, bs1.y, bs1.z, bs1.w};
    float mx = 0.f;
    if (tid < a.NT && !X_DBG(a, 2))
        for (int p = p0; p < a.TH * a.TW; p += PP) {
            const int py = (int)x_div((uint32_t)p, a.fd_tw), px = p - py * a.TW;
            const int oy = oy0 + py, ox = ox0 + px;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const int base = ((py * s) * a.PW + px * s) * a.GS + gl;
            float2v acc2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int at = (base + ((t / 3) * a.PW + (t % 3)) * a.GS) * 16;
                const u32x4 h = *reinterpret_cast<const u32x4 *>(HI + at), l = *reinterpret_cast<const u32x4 *>(LO + at);
                const float2v w2[4] = {{w0[t].x, w0[t].y}, {w0[t].z, w0[t].w}, {w1[t].x, w1[t].y}, {w1[t].z, w1[t].w}};
                if (a.in_f32) {                                  // (h, l) are the fp32 planes: channels 0-3 | 4-7
                    acc2[0] = __builtin_elementwise_fma(float2v{__uint_as_float(h[0]), __uint_as_float(h[1])}, w2[0], acc2[0]);
                    acc2[1] = __builtin_elementwise_fma(float2v{__uint_as_float(h[2]), __uint_as_float(h[3])}, w2[1], acc2[1]);
                    acc2[2] = __builtin_elementwise_fma(float2v{__uint_as_float(l[0]), __uint_as_float(l[1])}, w2[2], acc2[2]);
                    acc2[3] = __builtin_elementwise_fma(float2v{__uint_as_float(l[2]), __uint_as_float(l[3])}, w2[3], acc2[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {                // hi + lo back in fp32 (one op per channel), packed fp32 FMA on channel pairs
                        const float2v x2 = {x_mix_sum_lo(h[j], l[j]), x_mix_sum_hi(h[j], l[j])};
                        acc2[j] = __builtin_elementwise_fma(x2, w2[j], acc2[j]);
                    }
                }
            }
            const float acc[8] = {acc2[0].x, acc2[0].y, acc2[1].x, acc2[1].y, acc2[2].x, acc2[2].y, acc2[3].x, acc2[3].y};
            half8 hi, lo;
            float vd[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = x_actf(__builtin_fmaf(acc[j], sc[j], bs[j]), a.slope, a.cap);
                mx = fmaxf(mx, fabsf(v));
                vd[j] = v * down;
            }
            x_split8(vd, hi, lo);
            uint8_t *o = a.out + ((((size_t)b * a.Ho + oy) * a.Wo + ox) * G + g0 + gl) * 32;
            if (X_DBG(a, 4)) continue;
            *reinterpret_cast<half8 *>(o) = hi;
            *reinterpret_cast<half8 *>(o + 16) = lo;
        }
    x_amax_lds(&smax, 0, mx);
    __syncthreads();
    if (tid == 0 && smax) x_amax_global(a.amax_out + (size_t)b * XS, smax);
}
// patch geometry of a depthwise layer: fewest bytes moved per output (halo) among the shapes that leave the chip at least ~2
// workgroups per CU, with the patch under 40 KB (3+ workgroups per CU)
void xdw_geometry(xdw_args &d, int max_batch) {
    const int G = d.in.G, s = d.stride;
    double best = -1.0;
    const long lds_cap = (yk_dev_env("YK_X_DWLDS") ? atoi(yk_dev_env("YK_X_DWLDS")) : 40) * 1024L;
    const double gs_pref = yk_dev_env("YK_X_DWGS") ? atof(yk_dev_env("YK_X_DWGS")) : 3.0;
    for (int GS = 1; GS <= std::min(G, 64); ++GS) {
        if (G % GS) continue;
        const int NT = 256 / GS * GS;
        if (NT < 128) continue;
        for (int TH = 1; TH <= d.Ho; ++TH)
            for (int TW = 1; TW <= d.Wo; ++TW) {
                if (TW != d.Wo && (TW & 3)) continue;
                const int PH = (TH - 1) * s + 3, PW = (TW - 1) * s + 3;
                const long n16 = (long)PH * PW * GS;
                if (n16 * 32 > lds_cap) continue;
                const long tiles = (long)((d.Ho + TH - 1) / TH) * ((d.Wo + TW - 1) / TW), wgs = tiles * (G / GS) * max_batch;
                const double cover = (double)d.Ho * d.Wo / ((double)tiles * TH * TW);        // ragged tiles waste threads
                const double halo = (double)TH * TW * s * s / ((double)PH * PW);             // bytes used / bytes staged
                const double items = (double)TH * TW * GS / NT;                              // pixels per thread
                double score = halo * cover * std::min(1.0, items / 4.0) * std::min(1.0, wgs / 512.0) * std::min(1.0, GS / gs_pref);
                if (score > best) {
                    best = score;
                    d.TH = TH; d.TW = TW; d.PH = PH; d.PW = PW; d.GS = GS; d.NT = NT;
                    d.gsl = G / GS;
                    d.tiles_x = (d.Wo + TW - 1) / TW;
                    d.tiles_y = (d.Ho + TH - 1) / TH;
                    d.n16 = (int)n16;
                    d.n16p = (int)((n16 + 63) & ~63L);
                }
            }
    }
    d.fd_gsl = yk_make_fastdiv((uint32_t)d.gsl);
    d.fd_tpi = yk_make_fastdiv((uint32_t)(d.tiles_x * d.tiles_y));
    d.fd_tx = yk_make_fastdiv((uint32_t)d.tiles_x);
    d.fd_gs = yk_make_fastdiv((uint32_t)d.GS);
    d.fd_pw = yk_make_fastdiv((uint32_t)d.PW);
    d.fd_tw = yk_make_fastdiv((uint32_t)d.TW);
}

#include "yk_xblock.h"
#include "yk_xpersist.h"
#include "yk_xheads.h"
#include "yk_xfin.h"

// =====================================================================================================================
// stem conv (Cin = 3), fp32 VALU; u8 frames are normalised as float(v)/float(max) = numpy's `img / np.max(img)` rounded once.
// The normalised image is in [0, 1], so the storage exponent of the output is a plan-time constant (xstem_args::eo).
// =====================================================================================================================
struct xstem_args {
    const void *in;
    const unsigned *img_max;           // YK_MAXP partial maxima per image (u8 path)
    int in_f32, B, Hi, Wi, Ho, Wo, stride, pad_t, pad_l, Cout, outG;
    const float *w;                    // [27][Cout]
    const float *scale, *bias;
    float slope, cap;
    int eo;                            // storage exponent of the output (same for every image)
    uint8_t *out;
    int *eexp_out;
    uint32_t *amax_out;
};
template <int COUT>
__global__ void __launch_bounds__(256) xstem_kernel(const xstem_args a) {
    // the 27 x COUT weights, scale and bias are the same for every lane: read straight from the kernel-argument pointers they become
    // scalar loads feeding v_fma's SGPR operand (through LDS every FMA paid a ds_read)
    __shared__ float lut[256];
    __shared__ uint32_t smax;
    const int tid = threadIdx.x, b = blockIdx.y;
    const float *__restrict__ wl = a.w, *__restrict__ sc = a.scale, *__restrict__ bs = a.bias;
    if (tid == 0) {
        smax = 0u;
        a.eexp_out[b] = a.eo;
    }
    if (!a.in_f32) {
        unsigned mx = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) mx = max(mx, a.img_max[b * 32 + j]);
        lut[tid] = (float)tid / (float)mx;
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + tid;
    float vmax = 0.f;
    if (pix < a.Ho * a.Wo) {
        const int oy = pix / a.Wo, ox = pix - oy * a.Wo;
        float acc[COUT];
#pragma unroll
        for (int c = 0; c < COUT; ++c) acc[c] = 0.f;
        const int iy0 = oy * a.stride - a.pad_t, ix0 = ox * a.stride - a.pad_l;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = iy0 + ky;
            if ((unsigned)iy >= (unsigned)a.Hi) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ix0 + kx;
                if ((unsigned)ix >= (unsigned)a.Wi) continue;
                const size_t off = ((size_t)(b * a.Hi + iy) * a.Wi + ix) * 3;
                float x[3];
                if (a.in_f32) {
                    const float *p = reinterpret_cast<const float *>(a.in) + off;
                    x[0] = p[0];
                    x[1] = p[1];
                    x[2] = p[2];
                } else {
                    const uint8_t *p = reinterpret_cast<const uint8_t *>(a.in) + off;
                    x[0] = lut[p[0]];
                    x[1] = lut[p[1]];
                    x[2] = lut[p[2]];
                }
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float *w = wl + ((ky * 3 + kx) * 3 + ci) * COUT;
#pragma unroll
                    for (int c = 0; c < COUT; ++c) acc[c] = fmaf(x[ci], w[c], acc[c]);
                }
            }
        }
        const float down = x_pow2(-a.eo);
        uint8_t *o = a.out + ((size_t)b * a.Ho * a.Wo + pix) * a.outG * 32;
#pragma unroll
        for (int c8 = 0; c8 < COUT; c8 += 8) {
            half8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = x_actf(acc[c8 + j] * sc[c8 + j] + bs[c8 + j], a.slope, a.cap);
                vmax = fmaxf(vmax, fabsf(v));
                yk_half h, l;
                x_split(v * down, h, l);
                hi[j] = h;
                lo[j] = l;
            }
            *reinterpret_cast<half8 *>(o + c8 * 4) = hi;
            *reinterpret_cast<half8 *>(o + c8 * 4 + 16) = lo;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    if ((tid & 63) == 0) atomicMax(&smax, __float_as_uint(vmax));
    __syncthreads();
    if (tid == 0 && smax) x_amax_global(a.amax_out + (size_t)b * XS, smax);
}

// ---- 2x2 max pool 'same' (the maximum of stored values is the stored maximum: same exponent in and out) and residual add ----------
struct xpool_args {
    xview in;
    int B, Ho, Wo, stride;
    uint8_t *out;
    int *eexp_out;
    uint32_t *amax_out;
    yk_fastdiv fd_g, fd_wo;
};
__global__ void __launch_bounds__(256) xpool_kernel(const xpool_args a) {
    __shared__ uint32_t smax;
    const int tid = threadIdx.x, b = blockIdx.y, G = a.in.G;
    const int e = a.in.eexp[b];
    if (tid == 0) {
        smax = 0u;
        a.eexp_out[b] = e;
    }
    __syncthreads();
    const uint32_t idx = blockIdx.x * 256 + tid;
    float mx = 0.f;
    if (idx < (uint32_t)(a.Ho * a.Wo * G)) {
        const uint32_t pix = x_div(idx, a.fd_g), g = idx - pix * G;
        const uint32_t oy = x_div(pix, a.fd_wo), ox = pix - oy * a.Wo;
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
#pragma unroll
        for (int ky = 0; ky < 2; ++ky)
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) {
                const int iy = (int)oy * a.stride + ky, ix = (int)ox * a.stride + kx;
                if (iy >= a.in.H || ix >= a.in.W) continue;
                const uint8_t *q = a.in.p + ((((size_t)b * a.in.H + iy) * a.in.W + ix) * G + g) * 32;
                const half8 h = *reinterpret_cast<const half8 *>(q), l = *reinterpret_cast<const half8 *>(q + 16);
#pragma unroll
                for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], (float)h[j] + (float)l[j]);
            }
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mx = fmaxf(mx, fabsf(m[j]));
            yk_half h, l;
            x_split(m[j], h, l);                                   // exact: m is one of the stored hi + lo sums
            hi[j] = h;
            lo[j] = l;
        }
        uint8_t *o = a.out + (((size_t)b * a.Ho * a.Wo + pix) * G + g) * 32;
        *reinterpret_cast<half8 *>(o) = hi;
        *reinterpret_cast<half8 *>(o + 16) = lo;
    }
    x_amax_lds(&smax, 0, mx * x_pow2(e));
    __syncthreads();
    if (tid == 0 && smax) x_amax_global(a.amax_out + (size_t)b * XS, smax);
}
struct xadd_args {
    xview x, y;
    size_t n_per_image;                // groups per image
    uint8_t *out;
    int *eexp_out;
    uint32_t *amax_out;
};
__global__ void __launch_bounds__(256) xadd_kernel(const xadd_args a) {
    __shared__ uint32_t smax;
    __shared__ float sf[3];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (tid < 64) {
        const float bound = x_amax_wave(a.x.amax, b) + x_amax_wave(a.y.amax, b);
        const int eo = x_exp_of(__float_as_uint(bound));
        if (tid == 0) {
            smax = 0u;
            sf[0] = x_pow2(a.x.eexp[b]);
            sf[1] = x_pow2(a.y.eexp[b]);
            sf[2] = x_pow2(-eo);
            a.eexp_out[b] = eo;
        }
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + tid;
    float mx = 0.f;
    if (i < a.n_per_image) {
        const size_t k = ((size_t)b * a.n_per_image + i) * 32;
        const half8 xh = *reinterpret_cast<const half8 *>(a.x.p + k), xl = *reinterpret_cast<const half8 *>(a.x.p + k + 16);
        const half8 yh = *reinterpret_cast<const half8 *>(a.y.p + k), yl = *reinterpret_cast<const half8 *>(a.y.p + k + 16);
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = ((float)xh[j] + (float)xl[j]) * sf[0] + ((float)yh[j] + (float)yl[j]) * sf[1];
            mx = fmaxf(mx, fabsf(r));
            yk_half h, l;
            x_split(r * sf[2], h, l);
            hi[j] = h;
            lo[j] = l;
        }
        *reinterpret_cast<half8 *>(a.out + k) = hi;
        *reinterpret_cast<half8 *>(a.out + k + 16) = lo;
    }
    x_amax_lds(&smax, 0, mx);
    __syncthreads();
    if (tid == 0 && smax) x_amax_global(a.amax_out + (size_t)b * XS, smax);
}

// ---- host side ------------------------------------------------------------------------------------------------
enum { XK_STEM = 1, XK_CONV, XK_DW, XK_POOL, XK_ADD, XK_U8MAX, XK_BLOCK, XK_PERSIST, XK_HEADS, XK_FIN };
// tile configurations of xg_kernel
enum { XC_64x64 = 0, XC_64x128, XC_128x64, XC_128x128, XC_NUM };
struct xc_info {
    int bm, bn, threads;
    const char *name;
};
const xc_info g_xc[XC_NUM] = {{64, 64, 256, "64x64"}, {64, 128, 256, "64x128"}, {128, 64, 256, "128x64"}, {128, 128, 512, "128x128"}};

struct xtens : yk_gtens {
    uint8_t *d = nullptr;              // split tensor
    bool f32 = false;                  // ... stored as fp32 planes instead of (hi | lo): only a fused block's depthwise conv reads it
    float *d32 = nullptr;              // network output
};
struct xlaunch {
    int kind = 0;
    xg_args c;
    xdw_args d;
    xstem_args s;
    xpool_args p;
    xadd_args ad;
    xb_args b;
    int tm = 0, tn = 0;                // xb_kernel<tm, tn>
    int Ho = 0, Wo = 0;
    int cfg = 0, ns = 2;               // xg_kernel tile configuration and ring depth
    unsigned lds = 0;
    int in_tid = -1, out_tid = -1;     // tensors of a plain depthwise / 1x1 conv launch (chain detection of the persistent stage)
    unsigned ring_lds = 0;             // fused block: dynamic LDS without the output staging area
    xp_args pa;                        // XK_PERSIST
    xh_args ha;                        // XK_HEADS
    unsigned h_lds = 0;
    xf_args f;                         // XK_FIN: conv + BN + act -> 1x1 output conv in one launch (yk_xfin.h)
    int fin_bn = 0;                    // ... its output channels (64-row tiles on four waves)
    int p_cw = 0;
    std::string name;
    double flops = 0, bytes = 0;
};

template <int BM, int BN, int WM, int WN, int NS>
int x_launch_g(const xg_args &g, hipStream_t st) {
    typedef xg_cfg<BM, BN, WM, WN> C;
    constexpr unsigned lds = (unsigned)C::lds(NS), rlds = (unsigned)(C::CT + C::SMALL);
    dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN), (unsigned)g.splitk);
    yk_launch_lds(g.splitk > 1 ? xg_kernel<BM, BN, WM, WN, NS, true> : xg_kernel<BM, BN, WM, WN, NS, false>, grid, dim3(C::NT), lds, st, g);
    if (g.splitk > 1) yk_launch_lds(xg_reduce_kernel<BM, BN, WM, WN>, dim3(grid.x, grid.y), dim3(C::NT), rlds, st, g);
    return YK_OK;
}
template <int BM, int BN, int WM, int WN>
int x_launch_g_ns(const xg_args &g, int ns, hipStream_t st) {
    if (ns <= 2) return x_launch_g<BM, BN, WM, WN, 2>(g, st);
    if (ns == 3) return x_launch_g<BM, BN, WM, WN, 3>(g, st);
    return x_launch_g<BM, BN, WM, WN, 4>(g, st);
}
int x_launch_conv(int cfg, int ns, const xg_args &g, hipStream_t st) {
    switch (cfg) {
    case XC_64x64: return x_launch_g_ns<64, 64, 2, 2>(g, ns, st);
    case XC_64x128: return x_launch_g_ns<64, 128, 2, 2>(g, ns, st);
    case XC_128x64: return x_launch_g_ns<128, 64, 2, 2>(g, ns, st);
    case XC_128x128: return x_launch_g_ns<128, 128, 2, 4>(g, std::min(ns, 3), st);
    }
    yk_set_error("f16x2: bad tile configuration %d", cfg);
    return YK_ERR_ARG;
}

// a detection head in one launch (yk_xfin.h): grid = (BM-row tiles, 1, K slices)
template <int BM, int BN, int NW>
int x_launch_fin_bn(const xf_args &f, int ns, hipStream_t st) {
    typedef xf_cfg<BM, BN, NW> C;
    const dim3 grid((unsigned)((f.c.M + BM - 1) / BM), 1u, (unsigned)f.c.splitk);
    if (ns < 3) yk_launch_lds(xf_kernel<BM, BN, 2, NW>, grid, dim3(C::NT), C::lds(2), st, f);
    else yk_launch_lds(xf_kernel<BM, BN, 3, NW>, grid, dim3(C::NT), C::lds(3), st, f);
    return YK_OK;
}
int x_launch_fin(int bn, int ns, const xf_args &f, hipStream_t st) {
    if (bn == 128) return x_launch_fin_bn<64, 128, 4>(f, ns, st);
    if (bn == 192) return x_launch_fin_bn<64, 192, 4>(f, ns, st);
    yk_set_error("f16x2: no fused head kernel for a 64 x %d tile on 4 waves", bn);
    return YK_ERR_ARG;
}

template <int TM, int TN, int SG, bool F32IN = false, int NW = 4>
int x_launch_b2(const xb_args &g, int batch, unsigned lds, hipStream_t st) {
    if constexpr (SG > 0 && !F32IN)
        if (g.in_f32) return x_launch_b2<TM, TN, SG, true>(g, batch, lds, st);
    dim3 grid((unsigned)(batch * g.tiles_x * g.tiles_y), (unsigned)((g.N + 64 * TN - 1) / (64 * TN)));
    yk_launch_lds(xb_kernel<TM, TN, SG, F32IN, NW>, grid, dim3(NW * 64), lds, st, g);
    return YK_OK;
}
template <int TM, int TN>
int x_launch_b(const xb_args &g, int batch, unsigned lds, hipStream_t st) {
    if constexpr (TN == 1) {                                       // the stem-fed block of every network here has <= 64 output channels
        if (g.stem && g.GL == 2) return x_launch_b2<TM, TN, 2>(g, batch, lds, st);   // 16 / 24 / 32 stem filters
        if (g.stem && g.GL == 3) return x_launch_b2<TM, TN, 3>(g, batch, lds, st);
        if (g.stem && g.GL == 4) return x_launch_b2<TM, TN, 4>(g, batch, lds, st);
    }
    if (g.stem) {
        yk_set_error("f16x2: stem fusion needs an N tile of 64 and 16, 24 or 32 stem filters");
        return YK_ERR_UNSUPPORTED;
    }
    if constexpr (TN == 6) {                                       // the 384-wide tile: same tile, grid and LDS on eight waves of <= 128 registers
        if (g.waves == 8) return x_launch_b2<TM, TN, 0, false, 8>(g, batch, lds, st);
    }
    if (g.waves != 4) {
        yk_set_error("f16x2: no fused block kernel <%d,%d> on %d waves", TM, TN, g.waves);
        return YK_ERR_ARG;
    }
    return x_launch_b2<TM, TN, 0>(g, batch, lds, st);
}
const int g_xb_tm[] = {2, 3, 4, 5, 8}, g_xb_tn[] = {1, 2, 3, 6};
bool xb_has(int tm, int tn) {
    if (tm * tn > 24) return false;
    bool a = false, b = false;
    for (int v : g_xb_tm) a |= v == tm;
    for (int v : g_xb_tn) b |= v == tn;
    return a && b;
}
int x_launch_block(int tm, int tn, const xb_args &g, int batch, unsigned lds, hipStream_t st) {
#define XB_CASE(M, N) \
    if (tm == M && tn == N) return x_launch_b<M, N>(g, batch, lds, st);
    XB_CASE(2, 1) XB_CASE(2, 2) XB_CASE(2, 3) XB_CASE(2, 6)
    XB_CASE(3, 1) XB_CASE(3, 2) XB_CASE(3, 3) XB_CASE(3, 6)
    XB_CASE(4, 1) XB_CASE(4, 2) XB_CASE(4, 3) XB_CASE(4, 6)
    XB_CASE(5, 1) XB_CASE(5, 2) XB_CASE(5, 3)
    XB_CASE(8, 1) XB_CASE(8, 2) XB_CASE(8, 3)
#undef XB_CASE
    yk_set_error("f16x2: no fused block kernel <%d,%d>", tm, tn);
    return YK_ERR_ARG;
}
// LDS of a fused block: patch (hi | lo planes) + depthwise parameters per stage, the A tile, or the output staging if that is larger.
// The pointwise weights are NOT staged (each wave loads its own fragments into registers): `wt` adds the tile they used to take, which
// is what the tile-selection rule below was measured with (rounds 3-4) and still uses, so that the tiles stay the measured ones
int xb_bt_bytes(int tn, int N) { return std::min(64 * tn, (N + 15) / 16 * 16) * 128; }
unsigned xb_lds(int tm, int tn, int n16p, int db, int N, bool wt = false, bool staged = true) {
    const int bm = 16 * tm, bn = 64 * tn;
    const int ipp = (tn >= 3 && tm >= 2) ? (tm + 1) / 2 : tm;
    const int ring = (db ? 2 : 1) * (n16p * 32 + 2048 + (wt ? xb_bt_bytes(tn, N) : 0)) + bm * 128, ct = staged ? ipp * 16 * (bn * 4 + 16) : 0;
    return (unsigned)(std::max(ring, ct) + 64);
}
// Tile geometry of a fused block.  Measured on K2 at B=32 (tools/xbsweep.py: every (TM, TN, tile width, stages) per block): the launch
// time moves by only a few per cent across geometries, and what wins everywhere is THREE co-resident workgroups per CU (<= 53 KB of
// LDS each; their DMA, depthwise and MFMA phases overlap) with the whole N (up to 192 channels) in one workgroup and one stage;
// two stages never paid (they halve the co-residency).  So: N tile = min(192, N rounded up to 64); among the tiles that fit 53 KB the
// one with the most pixels, then the least halo.  Returns false when nothing fits (the caller keeps the two-launch form).
bool xb_geometry(xb_args &g, int *tm_out, int *tn_out, unsigned *lds_out, int max_batch, int ordinal) {
    const int s = g.stride;
    double best = -1.0;
    const bool mine = !yk_dev_env("YK_XB_LAYER") || atoi(yk_dev_env("YK_XB_LAYER")) == ordinal;   // developer sweeps: force one block only
    const int force_tm = mine && yk_dev_env("YK_XB_TM") ? atoi(yk_dev_env("YK_XB_TM")) : 0, force_tn = mine && yk_dev_env("YK_XB_TN") ? atoi(yk_dev_env("YK_XB_TN")) : 0;
    const int force_tw = mine && yk_dev_env("YK_XB_TW") ? atoi(yk_dev_env("YK_XB_TW")) : 0;
    const int force_db = mine && yk_dev_env("YK_XB_DB") ? atoi(yk_dev_env("YK_XB_DB")) : -1;
    const bool forced = force_tm || force_tn || force_tw || force_db >= 0;
    // N tile: the whole N up to 192 channels.  A long channel walk to 384 outputs (14x20x384 -> 384: 12 steps) takes all 384 in one
    // workgroup: two 192-wide workgroups would each repeat the depthwise pass, and with four batches in flight what counts is the work,
    // not the launch's own time (41.2 against 36.8 us alone, +3.5 % images/s in flight).  The 6-step 192 -> 384 block stays at 192 (30 vs 22 us).
    const bool wide = g.N > 192 && g.nk > 6;
    const int tn_want = (wide && yk_dev_env("YK_XB_TNL")) ? atoi(yk_dev_env("YK_XB_TNL")) : (wide ? 6 : std::min(3, (g.N + 63) / 64));
    (void)max_batch;
    for (int tm : g_xb_tm)
        for (int tn : g_xb_tn) {
            if (!xb_has(tm, tn) || (force_tm && tm != force_tm) || (force_tn && tn != force_tn)) continue;
            if (!force_tn && tn != tn_want) continue;
            // measured: 64-pixel tiles from 96 output channels on, 128 below.  (The 12-step blocks at 14x20x384 alone are faster on 32-pixel
            // tiles - 30.2 against 36 us - but with four batches in flight the step loses 3 %: more workgroups, more halo, more contention)
            const int tm_long = yk_dev_env("YK_XB_TML") ? atoi(yk_dev_env("YK_XB_TML")) : 4;
            if (!force_tm && tm > (tn_want == 1 ? 8 : (g.nk > 6 ? tm_long : 4))) continue;
            const int bm = 16 * tm;
            for (int TW = 1; TW <= std::min(g.Wo, bm); ++TW) {
                if (force_tw && TW != force_tw) continue;
                const int TH = std::min(g.Ho, bm / TW);
                if (TH * TW <= 16 * (tm - 1)) continue;                 // would leave a whole row block empty
                const int PH = (TH - 1) * s + 3, PW = (TW - 1) * s + 3;
                const int n16 = PH * PW * 4, n16p = (n16 + 63) & ~63;
                if (n16p > 1536) continue;
                for (int db = 0; db <= 1; ++db) {
                    if (force_db >= 0 ? db != force_db : db != 0) continue;
                    const unsigned lds = xb_lds(tm, tn, n16p, db, g.N);
                    if (lds > 160 * 1024 || (!forced && xb_lds(tm, tn, n16p, db, g.N, !wide) > 53 * 1024 + 512)) continue;
                    const long tiles = (long)((g.Ho + TH - 1) / TH) * ((g.Wo + TW - 1) / TW);
                    const double cover = (double)g.Ho * g.Wo / ((double)tiles * bm);       // useful rows of the MFMA tiles
                    const double halo = (double)TH * TW * s * s / ((double)PH * PW);       // bytes used / bytes staged
                    const double score = bm * cover * (0.5 + 0.5 * halo) * (TW >= TH ? 1.0 : 0.999) * ((TW & 3) ? 0.98 : 1.0);
                    if (score > best) {
                        best = score;
                        *tm_out = tm; *tn_out = tn; *lds_out = lds;
                        g.TH = TH; g.TW = TW; g.PH = PH; g.PW = PW; g.n16 = n16; g.n16p = n16p; g.db = db;
                        g.lds_bytes = (int)lds;
                        // converting a stored patch to fp32 once instead of in every tap: measured slower (49.8 vs 45.3 us, 35.3 vs 32.8 us on the
                        // two stride-1 blocks: the extra barrier and LDS pass cost more than the 60 conversions per item they save); the
                        // fused stem writes its patch as fp32 directly (84 -> 78 us)
                        g.prepass = (s == 1 && yk_dev_env("YK_XB_PREPASS")) ? 1 : 0;
                        g.tiles_x = (g.Wo + TW - 1) / TW;
                        g.tiles_y = (g.Ho + TH - 1) / TH;
                    }
                }
            }
        }
    if (best < 0) return false;
    g.fd_tpi = yk_make_fastdiv((uint32_t)(g.tiles_x * g.tiles_y));
    g.fd_tx = yk_make_fastdiv((uint32_t)g.tiles_x);
    g.fd_tw = yk_make_fastdiv((uint32_t)g.TW);
    g.fd_pw = yk_make_fastdiv((uint32_t)g.PW);
    g.fd_nk = yk_make_fastdiv((uint32_t)std::max(1, g.nk));
    g.GL = 4;
    // the long channel walk on the 384-wide tile runs on eight waves (yk_xblock.h: NW); whether its input is stored as fp32 planes or as
    // (hi | lo) does not matter, the half items read either.  Developer builds can force four for A/B runs
    g.waves = (wide && *tn_out == 6 && !(yk_dev_env("YK_XB_WAVES") && atoi(yk_dev_env("YK_XB_WAVES")) == 4)) ? 8 : 4;
    return true;
}

}   // namespace

struct yk_xplan {
    int max_batch = 0, in_h = 0, in_w = 0;
    std::vector<xtens> T;
    std::vector<xlaunch> L;
    yk_dev_mem mem;
    std::vector<int> outputs;
    unsigned *d_imgmax = nullptr;
    uint32_t *d_amax = nullptr;        // [n_tensors][max_batch][XS], then [max_batch] cluster arrival counters: cleared by every step's first launch
    size_t zero_words = 0;
    uint32_t *d_err = nullptr;         // sticky device error word (a cluster barrier timed out): the device alias of ...
    uint32_t *h_err = nullptr;         // ... this word of pinned, mapped host memory: the host reads it without a copy or a sync
    int *d_eexp = nullptr;             // [n_tensors][max_batch]
    long long *d_dbg = nullptr;        // developer instrumentation (yk_xplan_phase_stamps)
    int dbg_launch = -1;
    int cluster_wt = 0;                // YK_CLUSTER_WT as it stood when the plan was created -> xp_args / xh_args::write_through
};

void yk_xplan_destroy(yk_xplan *p) {
    if (!p) return;
    p->mem.free_all();
    if (p->h_err) (void)hipHostFree(p->h_err);
    delete p;
}


// The late backbone as one persistent launch (yk_xpersist.h).  Looks for the longest run of launches
//     dw3x3 -> conv1x1 -> dw3x3 -> conv1x1 ...      (plain launches, every one the only consumer of its predecessor's output
// unless that output is also a tap - then it is additionally written in the stored layout) whose images are small enough for one
// workgroup's LDS, and replaces it.  The decision depends on the network and the image size only, never on the batch.
static int x_build_persist(yk_xplan *p, int max_batch) {
    constexpr int CW = 8;
    const unsigned ring_cap = XP_NS * 8 * 6 * 1024;
    auto pw_ok = [&](const xlaunch &l) {
        const xg_args &g = l.c;
        return l.kind == XK_CONV && g.ks == 1 && g.stride == 1 && !g.s1.p && !g.up0 && !g.res.p && g.splitk == 1 && g.out && l.in_tid >= 0 &&
               (g.N % (16 * CW)) == 0 && (g.s0.G % CW) == 0 && (g.s0.G % 4) == 0;      // whole 16-channel blocks per member
    };
    auto dw_ok = [&](const xlaunch &l) { return l.kind == XK_DW && (l.d.in.G % CW) == 0 && (l.d.in.G % 4) == 0; };
    auto y_fits = [&](int H, int W, int Gs) { return (unsigned)(2 * (H + 2) * (W + 2) * Gs * 16) <= ring_cap; };
    int best0 = -1, best1 = -1;
    const int n = (int)p->L.size();
    for (int i = 0; i < n; ++i) {
        if (!dw_ok(p->L[i])) continue;
        int k = i, blocks = 0;
        while (k + 1 < n && dw_ok(p->L[k]) && pw_ok(p->L[k + 1]) && p->L[k + 1].in_tid == p->L[k].out_tid && p->T[p->L[k].out_tid].uses == 1) {
            const xdw_args &d = p->L[k].d;
            const xg_args &g = p->L[k + 1].c;
            const int nrb = (d.Ho * d.Wo + 15) / 16, ncb = g.N / 16 / CW, nT = 2 * (nrb + ncb);
            bool ok = nT <= 48 && y_fits(d.in.H, d.in.W, d.in.G / CW) && y_fits(d.Ho, d.Wo, g.N / 8 / CW) && d.in.H * d.in.W <= 1024;
            bool tile = false;
            for (int wr = 8; wr >= 1 && !tile; wr >>= 1) tile = (nrb + wr - 1) / wr <= 3 && (ncb + 8 / wr - 1) / (8 / wr) <= 3;
            if (!ok || !tile) break;
            ++blocks;
            k += 2;
            if (!(k < n && dw_ok(p->L[k]) && p->L[k].in_tid == p->L[k - 1].out_tid)) break;
        }
        if (blocks >= 2 && blocks * 2 > best1 - best0 + 1) {
            best0 = i;
            best1 = i + 2 * blocks - 1;
        }
        if (blocks) i = i + 2 * blocks - 1;
    }
    if (best0 < 0) return YK_OK;
    std::vector<xp_phase> ph;
    std::vector<std::pair<uint32_t, const xlaunch *>> wcopy;           // arena offset <- launch weights
    uint32_t arena = 0, dmax = 0;
    double flops = 0, bytes = 0;
    int nbar = 0, dbuf = 0;
    auto zero_phase = [] {
        xp_phase q;
        memset(&q, 0, sizeof(q));
        return q;
    };
    for (int k = best0; k <= best1; k += 2) {
        const xlaunch &ld = p->L[k], &lp = p->L[k + 1];
        const xdw_args &d = ld.d;
        const xg_args &g = lp.c;
        flops += ld.flops + lp.flops;
        bytes += ld.bytes + lp.bytes;
        const int Gs_in = d.in.G / CW, Gs_out = g.N / 8 / CW;
        if (k == best0) {                                              // the chain's input: a stored tensor
            xp_phase q = zero_phase();
            q.type = XP_LOAD;
            q.H = d.in.H; q.W = d.in.W; q.Gs = Gs_in;
            q.fd_w = yk_make_fastdiv((uint32_t)q.W); q.fd_gs = yk_make_fastdiv((uint32_t)q.Gs);
            q.src = d.in.p; q.src_eexp = d.in.eexp; q.src_amax = d.in.amax; q.tG = d.in.G; q.src_f32 = d.in_f32;
            ph.push_back(q);
        }
        {
            xp_phase q = zero_phase();
            q.type = XP_DW;
            q.H = d.in.H; q.W = d.in.W; q.Gs = Gs_in;
            q.fd_w = yk_make_fastdiv((uint32_t)q.W); q.fd_gs = yk_make_fastdiv((uint32_t)q.Gs);
            q.Ho = d.Ho; q.Wo = d.Wo; q.stride = d.stride; q.pad_t = d.pad_t; q.pad_l = d.pad_l;
            q.fd_wo = yk_make_fastdiv((uint32_t)q.Wo);
            q.par = d.par; q.Cp = d.in.G * 8;
            q.slope = d.slope; q.cap = d.cap; q.gain = d.gain; q.off = d.off;
            q.nrb_out = (d.Ho * d.Wo + 15) / 16;
            q.dbuf = dbuf;
            q.barrier_after = 1;
            dmax = std::max(dmax, (uint32_t)q.nrb_out * (uint32_t)(d.in.G / 4) * 2048u);
            ph.push_back(q);
            ++nbar;
        }
        {
            xp_phase q = zero_phase();
            q.type = XP_PW;
            q.H = d.Ho; q.W = d.Wo; q.Gs = Gs_out;
            q.fd_w = yk_make_fastdiv((uint32_t)q.W); q.fd_gs = yk_make_fastdiv((uint32_t)q.Gs);
            q.nrb = (d.Ho * d.Wo + 15) / 16; q.nks = d.in.G / 4; q.ncb = g.N / 16 / CW; q.nslab = g.nslab;
            int bt = 100;
            for (int wr = 8; wr >= 1; wr >>= 1) {
                const int tr = (q.nrb + wr - 1) / wr, tc = (q.ncb + 8 / wr - 1) / (8 / wr);
                if (tr <= 3 && tc <= 3 && tr * tc < bt) {
                    bt = tr * tc;
                    q.WR = wr; q.WC = 8 / wr;
                }
            }
            q.ppw = std::max(3, (2 * (q.nrb + q.ncb) + 7) / 8);
            // one wave per 16-pixel block and the y image + a weight ring fit side by side: fragments straight to registers
            q.adirect = 0;
            if (2 * (q.H + 2) * (q.W + 2) * q.Gs * 16 <= XP_YB_BYTES) {
                if (q.nrb <= 24 && q.ncb == 3) q.adirect = 1;              // kernel instantiations: see xp_kernel
                else if (q.nrb <= 24 && q.ncb == 2) q.adirect = 3;
                if ((q.adirect == 1 || q.adirect == 3) && q.nks * q.ncb * 2048 <= 76 * 1024) q.resident = 1;
                else if (q.nrb == 5 && q.ncb <= 8) q.adirect = 2;
                else if (q.nrb == 5 && q.ncb <= 16) q.adirect = 4;
            }
            q.zero_border = 1;
            q.w_off = arena;
            wcopy.push_back({arena, &lp});
            arena += (g.w_bytes + 1023u) & ~1023u;
            q.scale = g.scale; q.bias = g.bias;
            q.pslope = g.slope; q.pcap = g.cap; q.pgain = g.gain0; q.poff = g.off;
            q.dbuf = dbuf;
            ph.push_back(q);
            dbuf ^= 1;
        }
        const bool last = k + 1 == best1;
        p->T[ld.out_tid].d = nullptr;                                  // the depthwise tensor lives in the arena, in MFMA tile order
        if (!(last || p->T[lp.out_tid].uses != 1)) p->T[lp.out_tid].d = nullptr;   // never leaves the CU
        if (last || p->T[lp.out_tid].uses != 1) {                      // other kernels read it: stored layout too
            xp_phase q = zero_phase();
            q.type = XP_STORE;
            q.H = d.Ho; q.W = d.Wo; q.Gs = Gs_out;
            q.fd_w = yk_make_fastdiv((uint32_t)q.W); q.fd_gs = yk_make_fastdiv((uint32_t)q.Gs);
            q.dst = g.out; q.dst_eexp = g.eexp_out; q.dst_amax = g.amax_out; q.tG = g.outG; q.dst_f32 = g.dst_f32;
            ph.push_back(q);
        }
    }
    if ((int)ph.size() > XP_MAXPH) return YK_OK;                       // (keeps the plain launches)
    for (size_t i = 0; i + 1 < ph.size(); ++i)                         // a depthwise phase requests the weights of a resident pointwise phase behind it
        if (ph[i].type == XP_DW && ph[i + 1].type == XP_PW && ph[i + 1].resident) {
            ph[i].nw_off = ph[i + 1].w_off;
            ph[i].nw_nks = ph[i + 1].nks;
            ph[i].nw_ncb = ph[i + 1].ncb;
            ph[i].nw_nslab = ph[i + 1].nslab;
            ph[i + 1].resident = 2;
        }
    {   // the y image's border must be cleared where its shape changes or something else has used its LDS (the LDS-ring form)
        int ph_h = -1, ph_w = -1, ph_g = -1;
        for (auto &q : ph) {
            if (q.type == XP_LOAD) { ph_h = q.H; ph_w = q.W; ph_g = q.Gs; }
            if (q.type != XP_PW) continue;
            q.zero_border = !(q.adirect && q.H == ph_h && q.W == ph_w && q.Gs == ph_g);
            ph_h = q.H; ph_w = q.W; ph_g = q.Gs;
        }
    }
    for (size_t i = 0; i < ph.size(); ++i) {                           // every LOAD / PW phase requests the parameters of the depthwise phase behind it
        if (ph[i].type != XP_LOAD && ph[i].type != XP_PW) continue;
        for (size_t k = i + 1; k < ph.size(); ++k)
            if (ph[k].type == XP_DW) {
                ph[i].nd_par = ph[k].par;
                ph[i].nd_Cp = ph[k].Cp;
                ph[i].nd_Gs = ph[k].Gs;
                break;
            } else if (ph[k].type == XP_PW || ph[k].type == XP_LOAD) {
                break;
            }
    }
    xlaunch l;
    l.kind = XK_PERSIST;
    l.p_cw = CW;
    xp_args &a = l.pa;
    memset(&a, 0, sizeof(a));
    a.d_img_stride = dmax;
    a.d_off[0] = arena;
    a.d_off[1] = arena + dmax * (uint32_t)max_batch;
    const size_t total = (size_t)arena + 2 * (size_t)dmax * max_batch;
    if (total + 65536 >= X_OOB) return YK_OK;
    void *ar = nullptr, *dph = nullptr, *px = nullptr;
    int rc = p->mem.alloc(&ar, total + 65536);
    if (rc) return rc;
    for (auto &wc : wcopy) YK_HIP(hipMemcpy((uint8_t *)ar + wc.first, wc.second->c.w, wc.second->c.w_bytes, hipMemcpyDeviceToDevice));
    if ((rc = p->mem.upload(&dph, ph.data(), ph.size() * sizeof(xp_phase)))) return rc;
    a.ph = (const xp_phase *)dph;
    a.n_phase = (int)ph.size();
    a.CW = CW;
    a.arena = (const uint8_t *)ar;
    a.arena_bytes = (uint32_t)total;
    a.gran = reinterpret_cast<unsigned long long *>(p->d_amax + (p->zero_words - 2 * (size_t)max_batch * 2 * CW * 2));
    if ((rc = p->mem.alloc(&px, sizeof(uint32_t) * (size_t)max_batch * CW))) return rc;
    a.pxcc = (uint32_t *)px;
    a.err = p->d_err;
    char nm[160];
    const xdw_args &d0 = p->L[best0].d;
    snprintf(nm, sizeof nm, "x:persist[%d blocks dw3x3+conv1x1 from %dx%dx%d,%d phases,%d cluster barriers,%d wg/image]", (best1 - best0 + 1) / 2, d0.in.H, d0.in.W,
             d0.in.G * 8, (int)ph.size(), nbar, CW);
    l.name = nm;
    l.flops = flops;
    l.bytes = bytes;
    p->L.erase(p->L.begin() + best0, p->L.begin() + best1 + 1);
    p->L.insert(p->L.begin() + best0, l);
    return YK_OK;
}


// ---- the detection heads as one launch (yk_xheads.h) ---------------------------------------------------------------------------
// Takes the plan's trailing run of stride-1 'same' convs (3x3 -> network-output 1x1 pairs and the 1x1 in front of the UpSampling2D)
// when every one of them fits a kernel instantiation; otherwise the plain launches stay.  Depends on the network and the image size only.
static int x_build_heads_from(yk_xplan *p, int max_batch, int first, bool *built);
static int x_build_heads(yk_xplan *p, int max_batch) {
    const int n = (int)p->L.size();
    int first = n;
    while (first > 0 && p->L[first - 1].kind == XK_CONV) --first;
    // the longest suffix of the trailing convs that fits (the convs in front of it, e.g. the backbone's last pointwise conv, stay launches)
    for (; n - first >= 2; ++first) {
        bool built = false;
        const int rc = x_build_heads_from(p, max_batch, first, &built);
        if (rc || built) return rc;
    }
    return YK_OK;
}
static int x_build_heads_from(yk_xplan *p, int max_batch, int first, bool *built) {
    const int n = (int)p->L.size();
    auto conv_ok = [&](const xg_args &g) {
        return g.stride == 1 && !g.res.p && g.Ho == g.Hi && g.Wo == g.Wi &&
               ((g.ks == 1 && g.pad_t == 0 && g.pad_l == 0) || (g.ks == 3 && g.pad_t == 1 && g.pad_l == 1));
    };
    struct item {
        xh_phase q;
        int out_tid;
        std::string nm;
        double flops, bytes;
    };
    std::vector<item> ph;
    unsigned lds_main = 0;
    for (int k = first; k < n; ++k) {
        const xlaunch &l = p->L[k];
        const xg_args &g = l.c;
        if (!conv_ok(g) || g.out32 || !g.out || (g.N % 16) != 0) return YK_OK;
        item it;
        xh_phase &q = it.q;
        memset(&q, 0, sizeof(q));
        auto src = [&](const xview &v, int up, int nch) {
            xh_src s;
            s.p = v.p; s.eexp = v.eexp; s.amax = v.amax; s.bytes = v.bytes; s.G = v.G; s.H = v.H; s.W = v.W; s.up = up; s.nchunk = nch;
            return s;
        };
        q.s0 = src(g.s0, g.up0, g.nc0);
        if (g.s1.p) q.s1 = src(g.s1, 0, g.nc1);
        if (g.up0 && (g.s0.H * 2 != g.Hi || g.s0.W * 2 != g.Wi)) return YK_OK;
        q.H = g.Ho; q.W = g.Wo; q.W2 = g.Wo + 2; q.PP = (g.Ho + 2) * q.W2; q.taps = g.taps;
        q.fd_w = yk_make_fastdiv((uint32_t)q.W); q.fd_w2 = yk_make_fastdiv((uint32_t)q.W2);
        q.nrb = (g.Ho * g.Wo + 15) / 16; q.ncb = g.N / 16; q.nchunk = g.nc0 + g.nc1;
        if (q.PP > 384) return YK_OK;
        if (q.taps == 9 && q.nrb <= 5 && q.ncb <= 12 && q.nchunk <= 24 && !g.s1.p) { q.variant = 1; q.WR = 1; q.WC = 4; q.WK = 2; }
        else if (q.taps == 9 && q.nrb <= 18 && q.ncb <= 8 && q.nchunk <= 16) { q.variant = 0; q.WR = 2; q.WC = 4; q.WK = 1; }
        else if (q.taps == 1 && q.nrb <= 5 && q.ncb <= 8 && q.nchunk <= 24 && !g.s1.p) { q.variant = 2; q.WR = 1; q.WC = 4; q.WK = 2; }
        else return YK_OK;
        q.plane = (uint32_t)q.PP * 64u; q.img = 2u * q.plane;
        const int nslots = std::min(XH_NCH, (q.nchunk + XH_CW - 1) / XH_CW);
        lds_main = std::max(lds_main, (unsigned)nslots * q.img);
        q.w = g.w; q.w_bytes = g.w_bytes; q.nslab = g.nslab; q.scale = g.scale; q.bias = g.bias;
        q.slope = g.slope; q.cap = g.cap; q.gain0 = g.gain0; q.gain1 = g.gain1; q.off = g.off;
        q.nslot = XH_CW;
        if (q.WK == 2) lds_main = std::max(lds_main, (unsigned)(q.nrb * q.ncb * 1024));
        it.out_tid = l.out_tid;
        it.nm = l.name.substr(2, l.name.find('[') == std::string::npos ? std::string::npos : l.name.find('[') - 2);
        it.flops = l.flops; it.bytes = l.bytes;
        const bool tail = k + 1 < n && p->L[k + 1].c.out32 && p->L[k + 1].c.ks == 1 && conv_ok(p->L[k + 1].c) && !p->L[k + 1].c.s1.p && !p->L[k + 1].c.up0 &&
                          p->L[k + 1].c.s0.p == g.out && l.out_tid >= 0 && p->T[l.out_tid].uses == 1;
        if (tail) {
            const xlaunch &lt = p->L[k + 1];
            const xg_args &t = lt.c;
            q.tw = t.w; q.tw_bytes = t.w_bytes; q.t_nslab = t.nslab; q.t_N = t.N; q.t_ncb = (t.N + 15) / 16; q.t_nks = t.nc0;
            q.t_scale = t.scale; q.t_bias = t.bias; q.t_slope = t.slope; q.t_cap = t.cap; q.out32 = t.out32;
            if (q.t_nks * 32 < q.ncb * 16 || q.t_ncb > q.t_nslab || q.t_nks > 6) return YK_OK;
            lds_main = std::max(lds_main, (unsigned)(48 * (q.ncb * 16 + 4) * 4 + 64));
            it.nm += "+" + lt.name.substr(2, lt.name.find('[') == std::string::npos ? std::string::npos : lt.name.find('[') - 2);
            it.flops += lt.flops; it.bytes += lt.bytes;
            ++k;
        } else {
            q.out = g.out; q.out_bytes = (uint32_t)((size_t)max_batch * g.Ho * g.Wo * g.outG * 32); q.outG = g.outG; q.eexp_out = g.eexp_out; q.amax_out = g.amax_out;
        }
        ph.push_back(it);
    }
    if (ph.empty() || (int)ph.size() > XH_MAXPH) return YK_OK;
    if (lds_main + 256 > 156 * 1024) return YK_OK;
    // a stored output that a later phase reads goes first: its consumer then has another phase's barrier between them
    std::stable_sort(ph.begin(), ph.end(), [&](const item &a, const item &b) {
        auto feeds = [&](const item &x) {
            if (!x.q.out) return 0;
            for (const item &y : ph)
                if (y.q.s0.p == x.q.out || y.q.s1.p == x.q.out) return 1;
            return 0;
        };
        return feeds(a) > feeds(b);
    });
    uint32_t poff = 0;
    for (size_t i = 0; i < ph.size(); ++i) {
        xh_phase &q = ph[i].q;
        q.part_off = poff;
        poff += (uint32_t)q.nslot * (uint32_t)q.nrb * (uint32_t)q.ncb * 1024u;
        // every source must be complete: produced by an earlier kernel, or by a phase with a barrier between it and this one
        for (size_t k = 0; k < ph.size(); ++k) {
            const bool reads = ph[k].q.out && (q.s0.p == ph[k].q.out || q.s1.p == ph[k].q.out);
            if (!reads) continue;
            if (k >= i) return YK_OK;                                  // (cannot happen in a feed-forward plan)
            if (k + 1 == i) q.pre_barrier = 1;
        }
    }
    if (ph.size() == 1) ph[0].q.pre_barrier = 1;                       // the partial-sum region is reused by the cluster's next image
    const size_t total = (size_t)32 * poff;
    if (total + 65536 >= X_OOB) return YK_OK;
    std::vector<xh_phase> dev;
    for (auto &it : ph) dev.push_back(it.q);
    void *dpart = nullptr, *dph = nullptr, *px = nullptr;
    int rc;
    if ((rc = p->mem.alloc(&dpart, total + 65536))) return rc;
    if ((rc = p->mem.upload(&dph, dev.data(), dev.size() * sizeof(xh_phase)))) return rc;
    if ((rc = p->mem.alloc(&px, sizeof(uint32_t) * (size_t)max_batch * XH_CW))) return rc;
    xlaunch l;
    l.kind = XK_HEADS;
    xh_args &a = l.ha;
    memset(&a, 0, sizeof(a));
    a.ph = (const xh_phase *)dph;
    a.n_phase = (int)dev.size();
    a.CW = XH_CW;
    a.part = (uint8_t *)dpart;
    a.part_stride = poff;
    a.part_bytes = (uint32_t)total;
    a.gran = reinterpret_cast<unsigned long long *>(p->d_amax + (p->zero_words - (size_t)max_batch * 2 * XH_CW * 2));
    a.pxcc = (uint32_t *)px;
    a.err = p->d_err;
    a.lds_misc = (lds_main + 63u) & ~63u;
    l.h_lds = a.lds_misc + 256;
    std::string nm = "x:heads[";
    int nbar = 0;
    for (size_t i = 0; i < ph.size(); ++i) {
        nm += (i ? " | " : "") + ph[i].nm;
        l.flops += ph[i].flops;
        l.bytes += ph[i].bytes;
        nbar += 1 + ph[i].q.pre_barrier;
        if (ph[i].q.tw && ph[i].out_tid >= 0) p->T[ph[i].out_tid].d = nullptr;        // never leaves the cluster
    }
    char tl[96];
    snprintf(tl, sizeof tl, ";K split over %d wg/image,%d cluster barriers]", XH_CW, nbar);
    l.name = nm + tl;
    p->L.erase(p->L.begin() + first, p->L.end());
    p->L.push_back(l);
    *built = true;
    return YK_OK;
}

#include "yk_xplan_build.h"

// clears the running maxima when the step has no u8_max launch to do it (fp32 frames)
__global__ void __launch_bounds__(256) xzero_kernel(uint32_t *__restrict__ z, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) z[i] = 0u;
}

int yk_xplan_run(yk_xplan *p, const void *d_in, int in_f32, int batch, hipStream_t st, hipEvent_t *ev) {
    // the per-image running maxima are cleared by the step's first launch (no fill launch, nothing but kernels in a captured step)
    const size_t amax_words = p->zero_words;
    int li = 0;
    for (xlaunch &l : p->L) {
        if (ev) YK_HIP(hipEventRecord(ev[2 * li], st));
        switch (l.kind) {
        case XK_U8MAX:
            if (!in_f32) {
                int rc = yk_launch_u8_max((const uint8_t *)d_in, (size_t)p->in_h * p->in_w * 3, batch, p->d_imgmax, st, p->d_amax, amax_words);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL(xzero_kernel, dim3(128), dim3(256), 0, st, p->d_amax, amax_words);
            }
            break;
        case XK_STEM: {
            xstem_args s = l.s;
            s.in = d_in; s.in_f32 = in_f32; s.img_max = p->d_imgmax; s.B = batch;
            dim3 grid((s.Ho * s.Wo + 255) / 256, batch);
            if (s.Cout == 16) hipLaunchKernelGGL(xstem_kernel<16>, grid, dim3(256), 0, st, s);
            else if (s.Cout == 24) hipLaunchKernelGGL(xstem_kernel<24>, grid, dim3(256), 0, st, s);
            else hipLaunchKernelGGL(xstem_kernel<32>, grid, dim3(256), 0, st, s);
        } break;
        case XK_CONV: {
            xg_args g = l.c;
            g.B = batch;
            g.M = batch * l.Ho * l.Wo;
            if (const char *e = yk_dev_env("YK_X_DBG")) g.dbg = atoi(e);
            int rc = x_launch_conv(l.cfg, l.ns, g, st);
            if (rc) return rc;
        } break;
        case XK_FIN: {
            xf_args f = l.f;
            f.c.B = batch;
            f.c.M = batch * l.Ho * l.Wo;
            int rc = x_launch_fin(l.fin_bn, l.ns, f, st);
            if (rc) return rc;
        } break;
        case XK_BLOCK: {
            xb_args g = l.b;
            g.B = batch;
            if (g.stem) {
                g.frames = d_in;
                g.in_f32 = in_f32;
                g.img_max = p->d_imgmax;
            }
            if (const char *e = yk_dev_env("YK_XB_DBG")) g.dbg = atoi(e);
            g.stamps = (li == p->dbg_launch) ? p->d_dbg : nullptr;
            int rc = x_launch_block(l.tm, l.tn, g, batch, l.lds, st);
            if (rc) return rc;
        } break;
        case XK_DW: {
            xdw_args d = l.d;
            d.B = batch;
            if (const char *e = yk_dev_env("YK_X_DWDBG")) d.dbg = atoi(e);
            hipLaunchKernelGGL(xdw_kernel, dim3((unsigned)(batch * d.tiles_x * d.tiles_y * d.gsl)), dim3((unsigned)((d.NT + 63) & ~63)), l.lds, st, d);
        } break;
        case XK_PERSIST: {
            xp_args pa = l.pa;
            pa.B = batch;
            pa.n_cluster = 8 * std::min(4, (batch + 7) / 8);           // <= 32 clusters of p_cw workgroups: one workgroup per CU
            pa.stamps = (li == p->dbg_launch) ? p->d_dbg : nullptr;
            pa.write_through = p->cluster_wt;
            if (const char *e = yk_dev_env("YK_XP_DBG")) pa.dbg = atoi(e);
            yk_launch_lds(xp_kernel, dim3((unsigned)(pa.n_cluster * l.p_cw)), dim3(XP_NT), XP_NS * 8 * 6 * 1024 + XP_MISC, st, pa);
        } break;
        case XK_HEADS: {
            xh_args ha = l.ha;
            ha.B = batch;
            ha.n_cluster = 8 * std::min(4, (batch + 7) / 8);
            ha.stamps = (li == p->dbg_launch) ? p->d_dbg : nullptr;
            ha.write_through = p->cluster_wt;
            if (const char *e = yk_dev_env("YK_XH_DBG")) ha.dbg = atoi(e);
            yk_launch_lds(xh_kernel, dim3((unsigned)(ha.n_cluster * XH_CW)), dim3(XH_NT), l.h_lds, st, ha);
        } break;
        case XK_POOL: {
            xpool_args q = l.p;
            q.B = batch;
            const unsigned per_image = (unsigned)q.Ho * q.Wo * q.in.G;
            hipLaunchKernelGGL(xpool_kernel, dim3((per_image + 255) / 256, batch), dim3(256), 0, st, q);
        } break;
        case XK_ADD:
            hipLaunchKernelGGL(xadd_kernel, dim3((unsigned)((l.ad.n_per_image + 255) / 256), batch), dim3(256), 0, st, l.ad);
            break;
        }
        if (ev) YK_HIP(hipEventRecord(ev[2 * li + 1], st));
        ++li;
    }
    YK_HIP(hipGetLastError());
    return YK_OK;
}

int yk_xplan_output(yk_xplan *p, int idx, float **d_ptr, size_t *bytes, int *h, int *w, int *c) {
    if (idx < 0 || idx >= (int)p->outputs.size()) return YK_ERR_ARG;
    const xtens &t = p->T[p->outputs[idx]];
    if (d_ptr) *d_ptr = t.d32;
    if (bytes) *bytes = (size_t)p->max_batch * t.h * t.w * t.c * sizeof(float);
    if (h) *h = t.h;
    if (w) *w = t.w;
    if (c) *c = t.c;
    return YK_OK;
}

int yk_xplan_read_tensor(yk_xplan *p, int tid, int batch, float *h_dst, size_t dst_elems) {
    if (tid <= 0 || tid >= (int)p->T.size()) return YK_ERR_ARG;
    const xtens &t = p->T[tid];
    const size_t n = (size_t)batch * t.h * t.w * t.c;
    if (dst_elems < n) return YK_ERR_ARG;
    if (!t.d && !t.d32) {
        yk_set_error("yk_debug_read_tensor: tensor %d is a view or was folded away", tid);
        return YK_ERR_UNSUPPORTED;
    }
    YK_HIP(hipDeviceSynchronize());
    if (t.d32) {
        YK_HIP(hipMemcpy(h_dst, t.d32, n * sizeof(float), hipMemcpyDeviceToHost));
        return YK_OK;
    }
    const int G = t.cp >> 3;
    std::vector<uint16_t> hbuf((size_t)batch * t.h * t.w * G * 16);
    std::vector<int> ee(batch);
    YK_HIP(hipMemcpy(hbuf.data(), t.d, hbuf.size() * 2, hipMemcpyDeviceToHost));
    YK_HIP(hipMemcpy(ee.data(), p->d_eexp + (size_t)tid * p->max_batch, sizeof(int) * batch, hipMemcpyDeviceToHost));
    const size_t hw = (size_t)t.h * t.w;
    for (int b = 0; b < batch; ++b)
        for (size_t q = 0; q < hw; ++q) {
            const uint16_t *src = hbuf.data() + ((size_t)b * hw + q) * G * 16;
            float *dst = h_dst + ((size_t)b * hw + q) * t.c;
            if (t.f32) {                                                  // fp32 planes: the group's 32 bytes are eight floats
                const float *f = reinterpret_cast<const float *>(src);
                for (int c = 0; c < t.c; ++c) dst[c] = ldexpf(f[c], ee[b]);
                continue;
            }
            for (int c = 0; c < t.c; ++c)
                dst[c] = ldexpf(yk_h2f(src[(c >> 3) * 16 + (c & 7)]) + yk_h2f(src[(c >> 3) * 16 + 8 + (c & 7)]), ee[b]);
        }
    return YK_OK;
}

// the storage exponents of a stored tensor (split halves: x * 2^-e = hi + lo; fp32 planes: 0), one per image of the last run
int yk_xplan_read_exponents(yk_xplan *p, int tid, int batch, int32_t *h_e) {
    if (tid <= 0 || tid >= (int)p->T.size()) return YK_ERR_ARG;
    if (!p->T[tid].d) {
        yk_set_error("yk_debug_read_exponents: tensor %d has no stored exponent (a view, folded away, or an fp32 network output)", tid);
        return YK_ERR_UNSUPPORTED;
    }
    YK_HIP(hipDeviceSynchronize());
    YK_HIP(hipMemcpy(h_e, p->d_eexp + (size_t)tid * p->max_batch, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
    return YK_OK;
}

// dev instrumentation: arm phase timestamps for launch `li` (a fused block), run once, copy out [n_wg][16] ticks (100 MHz)
int yk_xplan_phase_stamps(yk_xplan *p, int li, const void *d_in, int batch, hipStream_t st, long long *h_out, int max_wg) {
    if (li < 0 || li >= (int)p->L.size() || (p->L[li].kind != XK_BLOCK && p->L[li].kind != XK_PERSIST && p->L[li].kind != XK_HEADS)) return YK_ERR_ARG;
    const size_t cap = 65536;
    if (!p->d_dbg) {
        int rc = p->mem.alloc((void **)&p->d_dbg, sizeof(long long) * 16 * cap);
        if (rc) return rc;
    }
    YK_HIP(hipMemset(p->d_dbg, 0, sizeof(long long) * 16 * cap));
    p->dbg_launch = li;
    int rc = yk_xplan_run(p, d_in, 0, batch, st, nullptr);
    p->dbg_launch = -1;
    if (rc) return rc;
    YK_HIP(hipStreamSynchronize(st));
    YK_HIP(hipMemcpy(h_out, p->d_dbg, sizeof(long long) * 16 * std::min<size_t>(cap, (size_t)max_wg), hipMemcpyDeviceToHost));
    return YK_OK;
}

// sticky device-side error (a cluster barrier of the persistent stage gave up): synchronises the device
int yk_xplan_check(yk_xplan *p) {
    YK_HIP(hipDeviceSynchronize());
    if (yk_xplan_peek_error(p, 1)) {
        yk_set_error("f16x2 cluster launch: a workgroup cluster did not assemble (its workgroups were not co-resident); results of that run are invalid");
        return YK_ERR_HIP;
    }
    return YK_OK;
}
// the error word as it stands now (no synchronisation: meaningful after the caller has waited for the runs it cares about)
unsigned yk_xplan_peek_error(yk_xplan *p, int clear) {
    volatile uint32_t *w = p->h_err;
    const unsigned e = w ? *w : 0u;
    if (e && clear) *w = 0u;
    return e;
}

void yk_xplan_debug_set_error(yk_xplan *p, unsigned value) {
    if (p->h_err) *(volatile uint32_t *)p->h_err = value;
}

int yk_xplan_launch_count(const yk_xplan *p) { return (int)p->L.size(); }
int yk_xplan_launch_info(const yk_xplan *p, int i, const char **name, double *flops, double *bytes) {
    if (i < 0 || i >= (int)p->L.size()) return YK_ERR_ARG;
    *name = p->L[i].name.c_str();
    *flops = p->L[i].flops;
    *bytes = p->L[i].bytes;
    return YK_OK;
}
