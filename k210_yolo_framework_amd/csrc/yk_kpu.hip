// yk_kpu.hip — the K210 KPU's integer pipeline for a kmodel v3, batched on gfx950 (include/yolo_hip.h yk_kpu_*).
//
// The semantics are those of oracle/kpu_ref.py, element by element:
//   acc = sum(x*w) + (arg_x*sum(x) >> shr_x) + (arg_w*sum(w) >> shr_w) + arg_add*g_ic       x, w uint8, padded taps = pad_value
//   z   = (acc*bn_mul >> bn_shift) + bn_add
//   y   = clamp(carry_shift((z - start[s])*mul[s], shift[s]) + bias[s], 0, 255)           s = last segment with z > start[s]
// all in int64 with numpy's two's-complement wrap (products taken in uint64) and arithmetic >> (counts >= 64 give the sign fill).
// The host (k210_yolo_framework_amd/kmodel.py:pack_kpu) folds the per-channel constants: wconst = (arg_w*sum(w) >> shr_w) + arg_add*g_ic.
//
// Dense convs are an implicit GEMM on the int8 MFMA (v_mfma_i32_16x16x64_i8): operands x' = x ^ 0x80, w' = w ^ 0x80 (x - 128, w - 128 as
// int8) and  sum(x*w) = sum(x'w') + 128 sum(x') + 128 sum(w') + 16384 K,  exact in int32 for K <= 27648.  The K axis is (ky, kx, c) with
// the channels of one tap padded to a multiple of 16 (x' = w' = 0 there: they add nothing to any sum).  Depthwise convs run on the VALU.
// Activations are uint8 NHWC per image, each tensor in its own buffer; main-memory layers are gathers, DEQUANTIZE writes the fp32 output.
#include "yk_common.h"

#include <algorithm>
#include <vector>

namespace {

enum { OP_CONV = 1, OP_DWCONV = 2, OP_GATHER = 3, OP_DEQUANT = 4 };
enum {
    F_OP = 0, F_IN, F_OUT, F_K, F_POOL, F_PAD, F_SHR_X, F_ARG_X, F_W_OFF, F_W_BYTES, F_CH_OFF, F_SEG_OFF, F_LAYER, F_C_OFF, F_TABLE_OFF,
    F_SCALE_BITS, F_BIAS_BITS, F_IN_C, F_IN_H, F_IN_W
};
static_assert(F_IN_W < YK_KPU_FIELDS, "op row");

// per output channel (blob, 64 bytes): wconst = (arg_w*sum_w >> shr_w) + arg_add*g_ic; fix = 128*sum(w') + 16384*K (dense only)
struct KpuChan {
    int64_t wconst, fix, bn_mul, bn_add, bn_shift, pad_[3];
};
// one activation segment (blob, 32 bytes)
struct KpuSeg {
    int64_t start, mul, shift, bias;
};

// every tensor of a plan, times max_batch, stays below this many elements: pixel indices (batch * H * W), the element indices of the
// depthwise / gather / dequantize launches and their grid sizes then fit 32-bit integers with room to spare (checked at create time)
constexpr long long YK_KPU_MAX_ELEMS = 1ll << 30;

struct ConvArgs {
    const uint8_t *in;
    uint8_t *out;
    const int8_t *w;      // dense: int8 w' [OCp32][Kw]; depthwise: uint8 w [C][k*k]
    const KpuChan *ch;
    const KpuSeg *seg;
    long long in_sb, in_sy, in_sx, in_sc;      // input strides in bytes (frame: NHWC or CHW; activations: NHWC)
    int C, H, W, OC, OH, OW;
    int k, stride, pad;
    int cq;               // 16-byte channel groups per tap (Cp / 16)
    int nq;               // 16-byte groups of K (k*k*cq)
    int nchunk;           // 64-wide K chunks (ceil(nq / 4))
    int Kw;               // weight row length (nchunk * 64)
    int M;                // batch * OH * OW
    int K;                // real K = C*k*k (dense) / k*k (depthwise)
    int pad_value;
    int shr_x;
    long long arg_x;
};

__device__ __forceinline__ int64_t wrap_mul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ __forceinline__ int64_t wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t wrap_sub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
// numpy int64 `>>`: arithmetic; a count of 64 or more gives the sign fill, which is what a count of 63 gives
__device__ __forceinline__ int64_t np_shr(int64_t v, int64_t s) { return v >> (s > 63 ? 63 : (s < 0 ? 0 : s)); }

// kpu_ref._carry_shift: round half up on the value shifted by s - 1 (a negative odd value keeps its floor)
__device__ __forceinline__ int64_t carry_shift(int64_t v, int64_t s) {
    if (s <= 0) return v;
    v = np_shr(v, s - 1);
    const int64_t half = v >> 1;
    return (v & 1) ? (v < 0 ? half : half + 1) : half;
}

// THE epilogue of every KPU conv output element (dense and depthwise), in its two halves: z, the pre-activation in 2^-p output steps (what
// bn_add shifts and the statistics run sums), and the segment table over it
__device__ __forceinline__ int64_t kpu_z(int64_t sum_xw, int64_t sum_x, long long arg_x, int shr_x, const KpuChan &c) {
    const int64_t acc = wrap_add(wrap_add(sum_xw, np_shr(wrap_mul(arg_x, sum_x), shr_x)), c.wconst);
    return wrap_add(np_shr(wrap_mul(acc, c.bn_mul), c.bn_shift), c.bn_add);
}

__device__ __forceinline__ uint8_t kpu_table(int64_t z, const KpuSeg *__restrict__ seg) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (z > seg[i].start) s = i;          // linear scan: the LAST segment whose start is below z (starts need not be sorted)
    const KpuSeg g = seg[s];
    int64_t y = wrap_add(carry_shift(wrap_mul(wrap_sub(z, g.start), g.mul), g.shift), g.bias);
    y = y < 0 ? 0 : (y > 255 ? 255 : y);
    return (uint8_t)y;
}

__device__ __forceinline__ uint8_t kpu_epilogue(int64_t sum_xw, int64_t sum_x, long long arg_x, int shr_x, const KpuChan &c,
                                                const KpuSeg *__restrict__ seg) {
    return kpu_table(kpu_z(sum_xw, sum_x, arg_x, shr_x, c), seg);
}

// The statistics run (yk_kpu_run_stats_u8): sums of z per output channel, uint64 adds that wrap like everything here - so the result does not
// depend on scheduling or launch geometry.  `step` 2 counts only output pixels with even oy and even ox (a stride-2 depthwise conv the KPU
// runs at stride 1: only those positions reach its pooling reader).
struct StatArgs {
    unsigned long long *zsum;     // [OC] of this conv
    int step;
};

typedef int v4i __attribute__((ext_vector_type(4)));

// sum of the 16 signed bytes of v (x' values): sum of the unsigned bytes of v ^ 0x80.. minus 16*128
__device__ __forceinline__ int sum16_signed(v4i v) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned u = (unsigned)v[i] ^ 0x80808080u;
        const unsigned t = (u & 0x00ff00ffu) + ((u >> 8) & 0x00ff00ffu);
        s += (int)((t & 0xffffu) + (t >> 16));
    }
    return s - 16 * 128;
}

// Dense conv: a wave computes 32 output channels x 64 output pixels (2 x 4 tiles of 16 x 16); A = weights (rows = oc), B = pixels
// (columns), so a lane's four accumulator registers are four consecutive channels of one pixel (C/D: col = lane&15, row = 4(lane>>4)+r).
// Inside a 64-wide K chunk, lane group h = lane>>4 holds K entries 16h..16h+15 of both operands (the same (group, byte) -> k map for A
// and B, so the order inside the chunk is immaterial to the exact integer sum).
// STATS: the same stores, and z of every counted element added to st.zsum[oc].  A lane's eight (i, t) channels are first summed over its four
// pixels j in registers, then over the 16 lanes of its group h (the same channels, 16 pixels) by shuffles, and lane r == 0 of every group
// issues one 64-bit atomic per channel: 32 per wave.  The shuffles sit after the pixel loop, outside every per-lane condition; the one return
// above them is taken by whole waves (px0 depends on the wave alone), so no shuffle reads a lane that has left.
template <bool FAST, bool STATS>
__device__ __forceinline__ void kpu_conv_mfma_body(const ConvArgs &a, const StatArgs &st) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px0 = (blockIdx.x * 4 + wave) * 64;
    if (px0 >= a.M) return;                   // wave-uniform
    const int oc0 = blockIdx.y * 32;
    const int r = lane & 15, h = lane >> 4;
    const int ohw = a.OH * a.OW;
    int iy0[4], ix0[4];
    long long base[4];
    bool pv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = px0 + 16 * j + r;
        pv[j] = m < a.M;
        const int mm = pv[j] ? m : 0;
        const int b = mm / ohw, rem = mm - b * ohw;
        const int oy = rem / a.OW, ox = rem - oy * a.OW;
        iy0[j] = oy * a.stride - a.pad;
        ix0[j] = ox * a.stride - a.pad;
        base[j] = (long long)b * a.in_sb;
    }
    const unsigned padb = (unsigned)(a.pad_value ^ 0x80) & 0xffu;
    const v4i padv = {(int)(padb * 0x01010101u), (int)(padb * 0x01010101u), (int)(padb * 0x01010101u), (int)(padb * 0x01010101u)};
    v4i acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4i{0, 0, 0, 0};
    int sx[4] = {0, 0, 0, 0};
    const int8_t *w0 = a.w + (size_t)(oc0 + r) * a.Kw;
    const int8_t *w1 = w0 + (size_t)16 * a.Kw;
    for (int chk = 0; chk < a.nchunk; ++chk) {
        const int q = chk * 4 + h;
        const v4i A0 = *reinterpret_cast<const v4i *>(w0 + q * 16);
        const v4i A1 = *reinterpret_cast<const v4i *>(w1 + q * 16);
        v4i B[4];
        if (q < a.nq) {
            const int tap = q / a.cq, c0 = (q - tap * a.cq) * 16;
            const int ky = tap / a.k, kx = tap - ky * a.k;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = iy0[j] + ky, ix = ix0[j] + kx;
                const bool inb = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                const uint8_t *src = a.in + base[j] + (long long)iy * a.in_sy + (long long)ix * a.in_sx;
                if (FAST) {
                    if (inb) {
                        v4i v = *reinterpret_cast<const v4i *>(src + c0);
                        B[j] = v ^ (int)0x80808080u;
                    } else {
                        B[j] = padv;
                    }
                } else {
                    unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int c = c0 + t;
                        unsigned v = 0u;
                        if (c < a.C) v = ((inb ? (unsigned)src[(long long)c * a.in_sc] : (unsigned)a.pad_value) ^ 0x80u) & 0xffu;
                        d[t >> 2] |= v << (8 * (t & 3));
                    }
                    B[j] = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) B[j] = v4i{0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sx[j] += sum16_signed(B[j]);
            acc[0][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, B[j], acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B[j], acc[1][j], 0, 0, 0);
        }
    }
    // sum(x') of pixel r: the four lane groups' partial sums
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sx[j] += __shfl_xor(sx[j], 16, 64);
        sx[j] += __shfl_xor(sx[j], 32, 64);
    }
    const bool vec = (a.OC & 3) == 0;
    unsigned long long zs[2][4] = {{0ull, 0ull, 0ull, 0ull}, {0ull, 0ull, 0ull, 0ull}};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!pv[j]) continue;
        const int m = px0 + 16 * j + r;
        const int64_t sum_x = (int64_t)sx[j] + 128 * (int64_t)a.K;
        uint8_t *dst = a.out + (size_t)m * a.OC;
        bool counted = true;
        if (STATS && st.step > 1) {
            const int rem = m % ohw, oy = rem / a.OW, ox = rem - oy * a.OW;
            counted = oy % st.step == 0 && ox % st.step == 0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oc = oc0 + 16 * i + 4 * h;
            if (oc >= a.OC) continue;
            unsigned pack = 0u;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (oc + t < a.OC) {
                    const KpuChan c = a.ch[oc + t];
                    const int64_t sum_xw = (int64_t)acc[i][j][t] + 128 * (int64_t)sx[j] + c.fix;
                    if (STATS) {
                        const int64_t z = kpu_z(sum_xw, sum_x, a.arg_x, a.shr_x, c);
                        if (counted) zs[i][t] += (unsigned long long)z;
                        pack |= (unsigned)kpu_table(z, a.seg) << (8 * t);
                    } else {
                        pack |= (unsigned)kpu_epilogue(sum_xw, sum_x, a.arg_x, a.shr_x, c, a.seg) << (8 * t);
                    }
                }
            }
            if (vec) {
                *reinterpret_cast<unsigned *>(dst + oc) = pack;
            } else {
                for (int t = 0; t < 4 && oc + t < a.OC; ++t) dst[oc + t] = (uint8_t)(pack >> (8 * t));
            }
        }
    }
    if (STATS) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                unsigned long long v = zs[i][t];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d, 64);    // lanes 16 h .. 16 h + 15: every lane of the wave is here
                const int oc = oc0 + 16 * i + 4 * h + t;
                if (r == 0 && oc < a.OC && v) atomicAdd(st.zsum + oc, v);       // (adding 0 changes nothing: skipped)
            }
    }
}

template <bool FAST>
__global__ __launch_bounds__(256) void kpu_conv_mfma(ConvArgs a) {
    kpu_conv_mfma_body<FAST, false>(a, StatArgs{nullptr, 1});
}

template <bool FAST>
__global__ __launch_bounds__(256) void kpu_conv_mfma_stats(ConvArgs a, StatArgs st) {
    kpu_conv_mfma_body<FAST, true>(a, st);
}

// Depthwise conv on the VALU: one thread per output element (pixel, channel)
__device__ __forceinline__ void kpu_dw_sums(const ConvArgs &a, int oy, int ox, const uint8_t *src, const uint8_t *w, int &sum_xw, int &sum_x) {
    sum_xw = 0, sum_x = 0;
    for (int ky = 0; ky < a.k; ++ky) {
        const int iy = oy * a.stride - a.pad + ky;
        for (int kx = 0; kx < a.k; ++kx) {
            const int ix = ox * a.stride - a.pad + kx;
            const int x = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? (int)src[(long long)iy * a.in_sy + (long long)ix * a.in_sx]
                                                                         : a.pad_value;
            sum_xw += x * (int)w[ky * a.k + kx];
            sum_x += x;
        }
    }
}

__global__ __launch_bounds__(256) void kpu_dwconv(ConvArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.M * a.C) return;
    const int m = (int)(idx / a.C), c = (int)(idx - (long long)m * a.C);
    const int ohw = a.OH * a.OW;
    const int b = m / ohw, rem = m - b * ohw;
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    const uint8_t *src = a.in + (long long)b * a.in_sb + (long long)c * a.in_sc;
    const uint8_t *w = reinterpret_cast<const uint8_t *>(a.w) + (size_t)c * a.k * a.k;
    int sum_xw, sum_x;
    kpu_dw_sums(a, oy, ox, src, w, sum_xw, sum_x);
    a.out[idx] = kpu_epilogue(sum_xw, sum_x, a.arg_x, a.shr_x, a.ch[c], a.seg);
}

// The statistics twin: the same store; no thread leaves before the barriers.  Consecutive threads are consecutive channels, so with C <= 256 a
// workgroup meets every channel 256 / C times: its z are summed per channel in LDS (64-bit LDS atomics) and each channel's sum goes out as one
// global atomic per workgroup.  With C > 256 the 256 threads of a workgroup hold 256 different channels - there is nothing to fold, and an
// address is met once per workgroup as well.
__global__ __launch_bounds__(256) void kpu_dwconv_stats(ConvArgs a, StatArgs st) {
    __shared__ unsigned long long s_z[256];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = idx < (long long)a.M * a.C;
    const bool lds = a.C <= 256;
    if (lds) s_z[threadIdx.x] = 0ull;
    if (lds) __syncthreads();
    if (valid) {
        const int m = (int)(idx / a.C), c = (int)(idx - (long long)m * a.C);
        const int ohw = a.OH * a.OW;
        const int b = m / ohw, rem = m - b * ohw;
        const int oy = rem / a.OW, ox = rem - oy * a.OW;
        const uint8_t *src = a.in + (long long)b * a.in_sb + (long long)c * a.in_sc;
        const uint8_t *w = reinterpret_cast<const uint8_t *>(a.w) + (size_t)c * a.k * a.k;
        int sum_xw, sum_x;
        kpu_dw_sums(a, oy, ox, src, w, sum_xw, sum_x);
        const int64_t z = kpu_z(sum_xw, sum_x, a.arg_x, a.shr_x, a.ch[c]);
        a.out[idx] = kpu_table(z, a.seg);
        if (oy % st.step == 0 && ox % st.step == 0 && z != 0) {
            if (lds)
                atomicAdd(s_z + c, (unsigned long long)z);
            else
                atomicAdd(st.zsum + c, (unsigned long long)z);
        }
    }
    if (lds) {
        __syncthreads();
        if ((int)threadIdx.x < a.C && s_z[threadIdx.x]) atomicAdd(st.zsum + threadIdx.x, s_z[threadIdx.x]);
    }
}

// REQUANTIZE / RESIZE_NEAREST / one part of a CONCAT:  out[b][y][x][c_off + c] = T[in[b][(y*ih)/oh][(x*iw)/ow][c]]
__global__ __launch_bounds__(256) void kpu_gather(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                  const uint8_t *__restrict__ table, long long total, int ih, int iw, int ic, int oh,
                                                  int ow, int oc_total, int c_off) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    long long t = idx;
    const int c = (int)(t % ic);
    t /= ic;
    const int x = (int)(t % ow);
    t /= ow;
    const int y = (int)(t % oh);
    const long long b = t / oh;
    const int sy = (int)(((long long)y * ih) / oh), sx = (int)(((long long)x * iw) / ow);
    uint8_t v = in[((b * ih + sy) * iw + sx) * ic + c];
    if (table) v = table[v];
    out[((b * oh + y) * ow + x) * oc_total + c_off + c] = v;
}

// DEQUANTIZE: float32(q) * scale, rounded, then + bias, rounded (this file is compiled without FMA contraction)
__global__ __launch_bounds__(256) void kpu_dequant(const uint8_t *__restrict__ in, float *__restrict__ out, long long total, float scale,
                                                   float bias) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const float p = (float)in[idx] * scale;
    out[idx] = p + bias;
}

struct Value {
    int C, H, W, dtype;   // dtype 0 = uint8, 1 = fp32
    size_t off = 0;       // in the arena
    size_t per_image() const { return (size_t)C * H * W * (dtype ? 4 : 1); }
};

struct Op {
    int op, in, out, k, pool, pad, shr_x, layer, c_off;
    long long arg_x;
    size_t w_off, ch_off, seg_off;
    long long table_off;
    float scale, bias;
    // derived (dense)
    int cq, nq, nchunk, Kw;
};

}  // namespace

struct yk_kpu_plan {
    int device = 0, max_batch = 0;
    std::vector<Value> V;
    std::vector<Op> ops;
    std::vector<int> outputs;
    int in_c = 0, in_h = 0, in_w = 0;
    uint8_t *blob = nullptr;     // device copy of the weight blob
    uint8_t *arena = nullptr;    // every value, [max_batch][H][W][C]
};

static long long up(long long v, long long m) { return (v + m - 1) / m * m; }

extern "C" void yk_kpu_plan_destroy(yk_kpu_plan_t *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->blob) (void)hipFree(p->blob);
    if (p->arena) (void)hipFree(p->arena);
    delete p;
}

extern "C" int yk_kpu_plan_create(yk_kpu_plan_t **out, const int64_t *ops, int n_ops, const int32_t *values, int n_values,
                                  const int32_t *outputs, int n_outputs, const void *blob, size_t blob_len, int max_batch, int device) {
    if (!out || !ops || !values || !outputs || !blob || n_ops <= 0 || n_values <= 0 || n_outputs <= 0 || max_batch <= 0) {
        yk_set_error("yk_kpu_plan_create: bad argument");
        return YK_ERR_ARG;
    }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yk_set_error("yk_kpu_plan_create: no HIP device visible (this library has no CPU path)");
        return YK_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        yk_set_error("yk_kpu_plan_create: device %d out of range (%d visible)", device, ndev);
        return YK_ERR_NO_DEVICE;
    }
    // ---- every check happens here: a run never fails on the plan's content
    std::vector<Value> V(n_values);
    for (int i = 0; i < n_values; ++i) {
        V[i] = Value{values[4 * i], values[4 * i + 1], values[4 * i + 2], values[4 * i + 3]};
        if (V[i].C <= 0 || V[i].H <= 0 || V[i].W <= 0 || V[i].C > 4096 || V[i].H > 4096 || V[i].W > 4096 || (V[i].dtype != 0 && V[i].dtype != 1)) {
            yk_set_error("yk_kpu_plan_create: value %d has shape (%d, %d, %d) / dtype %d", i, V[i].C, V[i].H, V[i].W, V[i].dtype);
            return YK_ERR_ARG;
        }
        if ((long long)max_batch * V[i].C * V[i].H * V[i].W > YK_KPU_MAX_ELEMS) {
            yk_set_error("yk_kpu_plan_create: value %d (%d, %d, %d) x max_batch %d is beyond the kernels' 32-bit indexing (%lld elements at most)",
                         i, V[i].C, V[i].H, V[i].W, max_batch, (long long)YK_KPU_MAX_ELEMS);
            return YK_ERR_UNSUPPORTED;
        }
    }
    std::vector<Op> O(n_ops);
    std::vector<char> written(n_values, 0);
    int in_c = 0, in_h = 0, in_w = 0;
    auto bad = [&](int code, int i, const char *what) {
        yk_set_error("yk_kpu_plan_create: op %d: %s", i, what);
        return code;
    };
    auto in_blob = [&](long long off, long long bytes) { return off >= 0 && bytes >= 0 && off % 16 == 0 && (unsigned long long)(off + bytes) <= blob_len; };
    for (int i = 0; i < n_ops; ++i) {
        const int64_t *f = ops + (size_t)i * YK_KPU_FIELDS;
        Op &o = O[i];
        o = Op{};
        o.op = (int)f[F_OP];
        o.in = (int)f[F_IN];
        o.out = (int)f[F_OUT];
        if (o.op < OP_CONV || o.op > OP_DEQUANT) return bad(YK_ERR_UNSUPPORTED, i, "unknown op code");
        if (o.out < 0 || o.out >= n_values) return bad(YK_ERR_ARG, i, "output value out of range");
        if (o.in < (o.op == OP_GATHER || o.op == OP_DEQUANT ? 0 : -1) || o.in >= n_values) return bad(YK_ERR_ARG, i, "input value out of range");
        if (o.in >= 0 && !written[o.in]) return bad(YK_ERR_ARG, i, "reads a value no earlier op wrote");
        const Value &vo = V[o.out];
        if (o.op == OP_CONV || o.op == OP_DWCONV) {
            o.k = (int)f[F_K];
            o.pool = (int)f[F_POOL];
            o.pad = (int)f[F_PAD];
            o.shr_x = (int)f[F_SHR_X];
            o.arg_x = f[F_ARG_X];
            o.layer = (int)f[F_LAYER];
            o.w_off = (size_t)f[F_W_OFF];
            o.ch_off = (size_t)f[F_CH_OFF];
            o.seg_off = (size_t)f[F_SEG_OFF];
            if (o.k != 1 && o.k != 3) return bad(YK_ERR_UNSUPPORTED, i, "kernel size other than 1x1 / 3x3");
            if (o.pool != 0 && o.pool != 5) return bad(YK_ERR_UNSUPPORTED, i, "KPU pool type other than bypass / left_top_2_s2");
            if (o.pad < 0 || o.pad > 255 || o.shr_x < 0 || o.shr_x > 15) return bad(YK_ERR_ARG, i, "pad value / shr_x out of range");
            int C, H, W;
            if (o.in >= 0) {
                const Value &vi = V[o.in];
                if (vi.dtype != 0) return bad(YK_ERR_ARG, i, "conv input is not uint8");
                C = vi.C, H = vi.H, W = vi.W;
            } else {
                // the frame (kpu_run_kmodel's input): its shape is in the op row
                if (in_c) return bad(YK_ERR_ARG, i, "only the first conv reads the frame");
                C = (int)f[F_IN_C], H = (int)f[F_IN_H], W = (int)f[F_IN_W];
                if (C <= 0 || H <= 0 || W <= 0 || C > 4096 || H > 4096 || W > 4096) return bad(YK_ERR_ARG, i, "frame shape");
                if ((long long)max_batch * C * H * W > YK_KPU_MAX_ELEMS) return bad(YK_ERR_UNSUPPORTED, i, "frames beyond the kernels' 32-bit indexing");
                in_c = C, in_h = H, in_w = W;
            }
            if (vo.dtype != 0) return bad(YK_ERR_ARG, i, "conv output is not uint8");
            const int OH = o.pool == 5 ? (H + 1) / 2 : H, OW = o.pool == 5 ? (W + 1) / 2 : W;
            if (vo.H != OH || vo.W != OW) return bad(YK_ERR_ARG, i, "output size does not follow from the input and the pool type");
            if (o.op == OP_DWCONV && vo.C != C) return bad(YK_ERR_ARG, i, "depthwise conv changes the channel count");
            const int OC = vo.C;
            long long wbytes;
            if (o.op == OP_CONV) {
                o.cq = (C + 15) / 16;
                o.nq = o.k * o.k * o.cq;
                o.nchunk = (o.nq + 3) / 4;
                o.Kw = o.nchunk * 64;
                wbytes = up(OC, 32) * o.Kw;
                if ((long long)C * o.k * o.k > 6912 * 4) return bad(YK_ERR_UNSUPPORTED, i, "K beyond the exact int32 range of the MFMA path");
            } else {
                wbytes = (long long)C * o.k * o.k;
            }
            if (f[F_W_BYTES] != wbytes || !in_blob(f[F_W_OFF], wbytes)) return bad(YK_ERR_ARG, i, "weights do not fit the blob / layout");
            if (!in_blob(f[F_CH_OFF], (long long)OC * (long long)sizeof(KpuChan))) return bad(YK_ERR_ARG, i, "channel table outside the blob");
            if (!in_blob(f[F_SEG_OFF], 16 * (long long)sizeof(KpuSeg))) return bad(YK_ERR_ARG, i, "activation table outside the blob");
        } else if (o.op == OP_GATHER) {
            const Value &vi = V[o.in];
            o.c_off = (int)f[F_C_OFF];
            o.table_off = f[F_TABLE_OFF];
            if (vi.dtype != 0 || vo.dtype != 0) return bad(YK_ERR_ARG, i, "gather of a non-uint8 value");
            if (o.c_off < 0 || o.c_off + vi.C > vo.C) return bad(YK_ERR_ARG, i, "channel slice outside the output");
            if (o.c_off != 0 || vi.C != vo.C) {
                if (vi.H != vo.H || vi.W != vo.W) return bad(YK_ERR_ARG, i, "concat part of another size");
            }
            if (o.table_off != -1 && !in_blob(o.table_off, 256)) return bad(YK_ERR_ARG, i, "table outside the blob");
        } else {
            const Value &vi = V[o.in];
            if (vi.dtype != 0 || vo.dtype != 1) return bad(YK_ERR_ARG, i, "dequantize is uint8 -> fp32");
            if (vi.C != vo.C || vi.H != vo.H || vi.W != vo.W) return bad(YK_ERR_ARG, i, "dequantize changes the shape");
            uint32_t sb = (uint32_t)f[F_SCALE_BITS], bb = (uint32_t)f[F_BIAS_BITS];
            memcpy(&o.scale, &sb, 4);
            memcpy(&o.bias, &bb, 4);
        }
        written[o.out] = 1;
    }
    if (!in_c) {
        yk_set_error("yk_kpu_plan_create: no conv reads the frame");
        return YK_ERR_ARG;
    }
    std::vector<int> outs(outputs, outputs + n_outputs);
    for (int v : outs)
        if (v < 0 || v >= n_values || !written[v] || V[v].dtype != 1) {
            yk_set_error("yk_kpu_plan_create: output value %d is not an fp32 value the program writes", v);
            return YK_ERR_ARG;
        }
    YK_HIP(hipSetDevice(device));
    yk_kpu_plan *p = new yk_kpu_plan();
    p->device = device;
    p->max_batch = max_batch;
    p->in_c = in_c, p->in_h = in_h, p->in_w = in_w;
    size_t total = 0;
    for (Value &v : V) {
        v.off = total;
        total += (size_t)up((long long)(v.per_image() * (size_t)max_batch), 256);
    }
    p->V = V;
    p->ops = O;
    p->outputs = outs;
    hipError_t e = hipMalloc(&p->blob, blob_len ? blob_len : 1);
    if (e == hipSuccess) e = hipMemcpy(p->blob, blob, blob_len, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->arena, total);
    if (e == hipSuccess) e = hipMemset(p->arena, 0, total);
    if (e != hipSuccess) {
        yk_set_error("yk_kpu_plan_create: %s (%zu bytes of activations)", hipGetErrorString(e), total);
        yk_kpu_plan_destroy(p);
        return e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_HIP;
    }
    *out = p;
    return YK_OK;
}

static ConvArgs conv_args(const yk_kpu_plan *p, const Op &o, const uint8_t *d_frames, int batch, int layout) {
    ConvArgs a{};
    const Value &vo = p->V[o.out];
    if (o.in < 0) {
        a.in = d_frames;
        a.C = p->in_c, a.H = p->in_h, a.W = p->in_w;
        if (layout == YK_KPU_CHW) {
            a.in_sc = (long long)a.H * a.W, a.in_sy = a.W, a.in_sx = 1;
        } else {
            a.in_sc = 1, a.in_sy = (long long)a.W * a.C, a.in_sx = a.C;
        }
    } else {
        const Value &vi = p->V[o.in];
        a.in = p->arena + vi.off;
        a.C = vi.C, a.H = vi.H, a.W = vi.W;
        a.in_sc = 1, a.in_sy = (long long)a.W * a.C, a.in_sx = a.C;
    }
    a.in_sb = (long long)a.C * a.H * a.W;
    a.out = p->arena + vo.off;
    a.w = reinterpret_cast<const int8_t *>(p->blob + o.w_off);
    a.ch = reinterpret_cast<const KpuChan *>(p->blob + o.ch_off);
    a.seg = reinterpret_cast<const KpuSeg *>(p->blob + o.seg_off);
    a.OC = vo.C, a.OH = vo.H, a.OW = vo.W;
    a.k = o.k, a.stride = o.pool == 5 ? 2 : 1, a.pad = (o.k - 1) / 2;
    a.cq = o.cq, a.nq = o.nq, a.nchunk = o.nchunk, a.Kw = o.Kw;
    a.M = batch * vo.H * vo.W;
    a.K = (o.op == OP_CONV ? a.C : 1) * o.k * o.k;
    a.pad_value = o.pad, a.shr_x = o.shr_x, a.arg_x = o.arg_x;
    return a;
}

// One run: d_zsum == nullptr is yk_kpu_run_u8; otherwise the conv launches are the statistics instantiations (the same grids), conv number n (in
// issue order) adding into d_zsum[sum of the earlier convs' OC ..] with step h_step[n].
static int kpu_run(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, const int *h_step, unsigned long long *d_zsum, void *stream) {
    YK_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    int n_conv = 0;
    size_t slot = 0;
    for (const Op &o : p->ops) {
        const Value &vo = p->V[o.out];
        StatArgs sa{nullptr, 1};
        if (d_zsum && (o.op == OP_CONV || o.op == OP_DWCONV)) {
            sa = StatArgs{d_zsum + slot, h_step[n_conv++]};
            slot += (size_t)vo.C;
        }
        if (o.op == OP_CONV) {
            const ConvArgs a = conv_args(p, o, d_frames, batch, layout);
            const dim3 grid((a.M + 255) / 256, (unsigned)(up(a.OC, 32) / 32));
            const bool fast = a.in_sc == 1 && a.C % 16 == 0 && a.in_sx % 16 == 0 && ((uintptr_t)a.in & 15) == 0;
            if (d_zsum) {
                if (fast)
                    hipLaunchKernelGGL(kpu_conv_mfma_stats<true>, grid, dim3(256), 0, st, a, sa);
                else
                    hipLaunchKernelGGL(kpu_conv_mfma_stats<false>, grid, dim3(256), 0, st, a, sa);
            } else if (fast) {
                hipLaunchKernelGGL(kpu_conv_mfma<true>, grid, dim3(256), 0, st, a);
            } else {
                hipLaunchKernelGGL(kpu_conv_mfma<false>, grid, dim3(256), 0, st, a);
            }
        } else if (o.op == OP_DWCONV) {
            const ConvArgs a = conv_args(p, o, d_frames, batch, layout);
            const long long n = (long long)a.M * a.C;
            if (d_zsum)
                hipLaunchKernelGGL(kpu_dwconv_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, sa);
            else
                hipLaunchKernelGGL(kpu_dwconv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
        } else if (o.op == OP_GATHER) {
            const Value &vi = p->V[o.in];
            const long long n = (long long)batch * vo.H * vo.W * vi.C;
            const uint8_t *tab = o.table_off >= 0 ? p->blob + o.table_off : nullptr;
            hipLaunchKernelGGL(kpu_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->arena + vi.off, p->arena + vo.off, tab, n,
                               vi.H, vi.W, vi.C, vo.H, vo.W, vo.C, o.c_off);
        } else {
            const Value &vi = p->V[o.in];
            const long long n = (long long)batch * vi.C * vi.H * vi.W;
            hipLaunchKernelGGL(kpu_dequant, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->arena + vi.off,
                               reinterpret_cast<float *>(p->arena + vo.off), n, o.scale, o.bias);
        }
        YK_HIP(hipGetLastError());
    }
    return YK_OK;
}

static int kpu_stat_slots(const yk_kpu_plan_t *p, int *n_convs) {
    int slots = 0, n = 0;
    for (const Op &o : p->ops)
        if (o.op == OP_CONV || o.op == OP_DWCONV) slots += p->V[o.out].C, ++n;
    if (n_convs) *n_convs = n;
    return slots;
}

extern "C" int yk_kpu_run_u8(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, void *stream) {
    if (!p || !d_frames || batch <= 0 || batch > p->max_batch || (layout != YK_KPU_NHWC && layout != YK_KPU_CHW)) {
        yk_set_error("yk_kpu_run_u8: bad argument (batch %d, max_batch %d, layout %d)", batch, p ? p->max_batch : 0, layout);
        return YK_ERR_ARG;
    }
    return kpu_run(p, d_frames, batch, layout, nullptr, nullptr, stream);
}

extern "C" int yk_kpu_stat_slots(const yk_kpu_plan_t *p) { return p ? kpu_stat_slots(p, nullptr) : 0; }

extern "C" int yk_kpu_run_stats_u8(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, const int *h_step, int n_step,
                                   uint64_t *d_zsum, void *stream) {
    if (!p || !d_frames || !h_step || !d_zsum || batch <= 0 || batch > p->max_batch || (layout != YK_KPU_NHWC && layout != YK_KPU_CHW) ||
        ((uintptr_t)d_zsum & 7u) != 0) {
        yk_set_error("yk_kpu_run_stats_u8: bad argument (batch %d, max_batch %d, layout %d)", batch, p ? p->max_batch : 0, layout);
        return YK_ERR_ARG;
    }
    int n_convs = 0;
    (void)kpu_stat_slots(p, &n_convs);
    if (n_step != n_convs) {
        yk_set_error("yk_kpu_run_stats_u8: %d steps for the %d conv ops of the plan", n_step, n_convs);
        return YK_ERR_ARG;
    }
    for (int i = 0; i < n_step; ++i)
        if (h_step[i] != 1 && h_step[i] != 2) {
            yk_set_error("yk_kpu_run_stats_u8: step %d of conv op %d (1 or 2)", h_step[i], i);
            return YK_ERR_ARG;
        }
    return kpu_run(p, d_frames, batch, layout, h_step, reinterpret_cast<unsigned long long *>(d_zsum), stream);
}

extern "C" int yk_kpu_get_output(yk_kpu_plan_t *p, int idx, float **d_ptr, size_t *bytes, int *h, int *w, int *c) {
    if (!p || idx < 0 || idx >= (int)p->outputs.size()) {
        yk_set_error("yk_kpu_get_output: bad argument");
        return YK_ERR_ARG;
    }
    const Value &v = p->V[p->outputs[idx]];
    if (d_ptr) *d_ptr = reinterpret_cast<float *>(p->arena + v.off);
    if (bytes) *bytes = v.per_image() * (size_t)p->max_batch;
    if (h) *h = v.H;
    if (w) *w = v.W;
    if (c) *c = v.C;
    return YK_OK;
}

extern "C" int yk_kpu_output_count(const yk_kpu_plan_t *p) { return p ? (int)p->outputs.size() : 0; }

extern "C" int yk_kpu_launch_count(const yk_kpu_plan_t *p) { return p ? (int)p->ops.size() : 0; }

extern "C" int yk_kpu_debug_read(yk_kpu_plan_t *p, int layer_index, int image, uint8_t *h_dst, size_t n) {
    if (!p || !h_dst || image < 0 || image >= p->max_batch) {
        yk_set_error("yk_kpu_debug_read: bad argument");
        return YK_ERR_ARG;
    }
    for (const Op &o : p->ops) {
        if ((o.op != OP_CONV && o.op != OP_DWCONV) || o.layer != layer_index) continue;
        const Value &v = p->V[o.out];
        const size_t per = v.per_image();
        if (n != per) {
            yk_set_error("yk_kpu_debug_read: layer %d holds %zu bytes per image, %zu asked", layer_index, per, n);
            return YK_ERR_ARG;
        }
        YK_HIP(hipSetDevice(p->device));
        std::vector<uint8_t> hwc(per);
        YK_HIP(hipDeviceSynchronize());
        YK_HIP(hipMemcpy(hwc.data(), p->arena + v.off + per * (size_t)image, per, hipMemcpyDeviceToHost));
        for (int y = 0; y < v.H; ++y)
            for (int x = 0; x < v.W; ++x)
                for (int c = 0; c < v.C; ++c) h_dst[((size_t)c * v.H + y) * v.W + x] = hwc[((size_t)y * v.W + x) * v.C + c];
        return YK_OK;
    }
    yk_set_error("yk_kpu_debug_read: layer %d is not a conv layer of this plan", layer_index);
    return YK_ERR_ARG;
}

extern "C" int yk_kpu_layer_ptr(yk_kpu_plan_t *p, int layer_index, uint8_t **d_ptr, int *h, int *w, int *c) {
    if (!p || !d_ptr) {
        yk_set_error("yk_kpu_layer_ptr: bad argument");
        return YK_ERR_ARG;
    }
    for (const Op &o : p->ops) {
        if ((o.op != OP_CONV && o.op != OP_DWCONV) || o.layer != layer_index) continue;
        const Value &v = p->V[o.out];
        *d_ptr = p->arena + v.off;
        if (h) *h = v.H;
        if (w) *w = v.W;
        if (c) *c = v.C;
        return YK_OK;
    }
    yk_set_error("yk_kpu_layer_ptr: layer %d is not a conv layer of this plan", layer_index);
    return YK_ERR_ARG;
}

// Per-launch timing: the run replayed `iters` times with HIP events around every launch; ms_out[i] = median of launch i.
extern "C" int yk_kpu_profile(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, int iters, void *stream, float *ms_out) {
    if (!p || !ms_out || iters <= 0) {
        yk_set_error("yk_kpu_profile: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipSetDevice(p->device));
    const size_t n = p->ops.size();
    std::vector<hipEvent_t> ev(2 * n);              // start / end of every launch
    for (auto &e : ev) YK_HIP(hipEventCreate(&e));
    std::vector<std::vector<float>> t(n);
    yk_kpu_plan sub = *p;                           // one op at a time (blob and arena borrowed from p)
    int rc = YK_OK;
    for (int it = 0; it < iters && rc == YK_OK; ++it) {
        for (size_t i = 0; i < n && rc == YK_OK; ++i) {
            sub.ops.assign(p->ops.begin() + i, p->ops.begin() + i + 1);
            (void)hipEventRecord(ev[2 * i], (hipStream_t)stream);
            rc = yk_kpu_run_u8(&sub, d_frames, batch, layout, stream);
            (void)hipEventRecord(ev[2 * i + 1], (hipStream_t)stream);
        }
        if (rc != YK_OK) break;
        (void)hipEventSynchronize(ev[2 * n - 1]);
        for (size_t i = 0; i < n; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
            t[i].push_back(ms);
        }
    }
    sub.blob = sub.arena = nullptr;
    for (auto &e : ev) (void)hipEventDestroy(e);
    if (rc != YK_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
        std::vector<float> &v = t[i];
        std::sort(v.begin(), v.end());
        ms_out[i] = v[v.size() / 2];
    }
    return YK_OK;
}
