// yk_qerr.hip — the quantisation error of a KPU tensor against a float tensor, per channel (qerror.py states the rule).
//
// q = uint8 codes [B][qH][qW][C] as engine.KpuPlan keeps them, y = fp32 [B][ho][wo][C] as quantize.Calibrator makes them; step 2 compares float
// position (oy, ox) with code position (2 oy, 2 ox) - the deferred stride 2 of quantize.plan_convs.  A row is one float position, M = B ho wo.
// Per element, in float64 with one rounding per operation (this unit compiles with -ffp-contract=off, and numpy does the same):
//     yh = (double)(q - zp) * (double)s_y,  e = (double)y - yh,  the terms y y, e e, e, y yh, yh yh, and |e| for the maximum.
// A memory-bound reduction: 5 bytes read per element, nothing written per element.  Structure as scale_act_chsum_kernel of yk_calib.hip - no
// floating-point atomics, and an order that (M, C) alone fix:
//   * the channels are walked in chunks of w = min(C - c0, QE_BLOCK); a chunk has L = 4 * (QE_BLOCK / w) ROW LANES;
//   * workgroup g owns rows [g * T, (g + 1) * T), T = qe_rows(C); lane l of a chunk takes rows g * T + l, + L, + 2 L, ... in that order;
//   * each of the QE_NQ quantities of a channel - the three counts packed into one integer, five sums, one maximum - is folded over the L lanes
//     by a tree in LDS (lanes [half, n) onto [0, n - half)), one quantity after the other through the same 8 KB, and is partial[g][k][c];
//   * the finishing launch (one workgroup per chunk) walks the G partials of a channel with R = QE_BLOCK / w lanes the same way - lane r takes
//     g = r, r + R, ... : ceil(G / R) passes - folds them by the same tree and joins the result with the slot (a plain load and store).
// The two thread layouts realise the same lanes: with 16-byte loads of y (and 4-byte loads of q) a thread is one lane of four channels; without,
// a thread is one channel and walks lanes r, r + R, r + 2 R, r + 3 R one after the other.
// A non-finite y enters nothing and sets the channel's flag (an integer atomicOr from the threads that met one).
#include "yk_range.h"

namespace {
using namespace yk_range;
typedef unsigned long long u64;

constexpr int QE_BLOCK = CAL_BLOCK;
static_assert(QE_BLOCK == YK_QERR_BLOCK, "the header states the workgroup's width");
constexpr int QE_NQ = 7;                                  // quantities a workgroup leaves per channel: counts, 5 sums, max |e|
constexpr int QE_MAX = QE_NQ - 1;                         // the one that is a maximum
constexpr int QE_BITS = 21;                               // of each of the three counts packed into quantity 0
static_assert(YK_QERR_TILE < (1 << QE_BITS), "a workgroup's rows must fit a packed count");
constexpr int QE_OUT = 9;                                 // words the finishing launch writes per slot: 3 counts, 5 sums, the maximum

inline size_t qe_rows(int C) { return (size_t)((YK_QERR_TILE + C - 1) / C); }                 // T: rows of one workgroup (>= 1)
inline size_t qe_groups(size_t M, int C) { return (M + qe_rows(C) - 1) / qe_rows(C); }        // G

struct Geo {
    size_t HW;                                            // ho * wo
    int wo, qH, qW, step;
};

// the row of q that float row `row` is compared with
__device__ __forceinline__ size_t q_row(const Geo &g, size_t row) {
    if (g.step == 1) return row;
    const size_t b = row / g.HW;
    const uint32_t r = (uint32_t)(row - b * g.HW), oy = r / (uint32_t)g.wo, ox = r - oy * (uint32_t)g.wo;
    return (b * (size_t)g.qH + 2u * oy) * (size_t)g.qW + 2u * ox;
}

struct QAcc {
    u64 cnt = 0ull;                                       // n | (q == 0) << QE_BITS | (q == 255) << 2 QE_BITS
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};         // sum y^2, e^2, e, y yh, yh^2; max |e|
    uint32_t bad = 0u;
    __device__ __forceinline__ void add(float y, uint32_t q, double s, int zp) {
        if ((__float_as_uint(y) & 0x7F800000u) == 0x7F800000u) {
            bad = 1u;
            return;
        }
        const double yd = (double)y, h = (double)((int)q - zp) * s, e = yd - h;
        cnt += 1ull | ((u64)(q == 0u) << QE_BITS) | ((u64)(q == 255u) << (2 * QE_BITS));
        v[0] += yd * yd;
        v[1] += e * e;
        v[2] += e;
        v[3] += yd * h;
        v[4] += h * h;
        v[5] = fmax(v[5], fabs(e));
    }
    __device__ __forceinline__ u64 word(int k) const { return k == 0 ? cnt : (u64)__double_as_longlong(v[k - 1]); }
};

// two values of quantity k (0: integers; QE_MAX: a maximum; else a sum), a before b
__device__ __forceinline__ u64 qe_join(int k, u64 a, u64 b) {
    if (k == 0) return a + b;
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return (u64)__double_as_longlong(k == QE_MAX ? fmax(x, y) : x + y);
}

// the tree over `n` lanes of `w` channels held as s[lane * w + channel]; every thread of the workgroup calls it
__device__ __forceinline__ void qe_tree(u64 *s, int n, int w, int k) {
    while (n > 1) {
        const int half = (n + 1) / 2;
        __syncthreads();
        for (int e = threadIdx.x; e < (n - half) * w; e += QE_BLOCK) s[e] = qe_join(k, s[e], s[e + half * w]);
        n = half;
    }
    __syncthreads();
}

template <int V>
__global__ __launch_bounds__(QE_BLOCK) void qerr_kernel(const uint8_t *__restrict__ q, const float *__restrict__ y, size_t M, int C, size_t T, Geo geo,
                                                         double s, int zp, u64 *__restrict__ partial, u64 *slots) {
    __shared__ u64 s_w[4 * QE_BLOCK];
    const int t = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * T;
    const size_t row1 = row0 + T < M ? row0 + T : M;
    for (int c0 = 0; c0 < C; c0 += QE_BLOCK) {
        const int w = C - c0 < QE_BLOCK ? C - c0 : QE_BLOCK;
        const int R = QE_BLOCK / w, L = 4 * R;
        const int wq = V == 4 ? w / 4 : w, col = t % wq, r = t / wq;               // V = 4: r is the lane, col a group of four channels
        const bool works = r < (V == 4 ? L : R);                                   // wq * L = R * w <= QE_BLOCK threads work
        QAcc a[4];                                                                 // V = 4: four channels of lane r; else lanes r + j R of channel col
        if (works) {
            if constexpr (V == 4) {
                const int c = c0 + 4 * col;
                for (size_t row = row0 + r; row < row1; row += L) {
                    const float4 f = *reinterpret_cast<const float4 *>(y + row * (size_t)C + c);
                    const uint32_t b = *reinterpret_cast<const uint32_t *>(q + q_row(geo, row) * (size_t)C + c);
                    a[0].add(f.x, b & 255u, s, zp);
                    a[1].add(f.y, b >> 8 & 255u, s, zp);
                    a[2].add(f.z, b >> 16 & 255u, s, zp);
                    a[3].add(f.w, b >> 24, s, zp);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (a[j].bad) atomicOr(slots + (size_t)YK_QERR_WORDS * (c + j) + 3, 1ull);
            } else {
                const int c = c0 + col;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    for (size_t row = row0 + r + (size_t)j * R; row < row1; row += L)
                        a[j].add(y[row * (size_t)C + c], q[q_row(geo, row) * (size_t)C + c], s, zp);
                if (a[0].bad | a[1].bad | a[2].bad | a[3].bad) atomicOr(slots + (size_t)YK_QERR_WORDS * c + 3, 1ull);
            }
        }
#pragma unroll
        for (int k = 0; k < QE_NQ; ++k) {
            __syncthreads();                                                       // what was there has been read
            if (works) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s_w[V == 4 ? r * w + 4 * col + j : (r + j * R) * w + col] = a[j].word(k);
            }
            qe_tree(s_w, L, w, k);
            for (int e = t; e < w; e += QE_BLOCK) partial[((size_t)blockIdx.x * QE_NQ + k) * (size_t)C + c0 + e] = s_w[e];
        }
    }
}

// workgroup blockIdx.x = chunk c0 = blockIdx.x * QE_BLOCK of the channels
__global__ __launch_bounds__(QE_BLOCK) void qerr_finish_kernel(const u64 *__restrict__ partial, size_t G, int C, u64 *slots) {
    __shared__ u64 s_w[QE_BLOCK];
    const int t = threadIdx.x, c0 = blockIdx.x * QE_BLOCK;
    const int w = C - c0 < QE_BLOCK ? C - c0 : QE_BLOCK;
    const int R = QE_BLOCK / w, col = t % w, r = t / w;
    for (int j = 0; j < QE_OUT; ++j) {                                             // 0..2: the counts out of quantity 0; 3..8: quantities 1..6
        const int k = j < 3 ? 0 : j - 2;
        __syncthreads();
        if (r < R) {
            u64 a = 0ull;                                                          // (the bits of +0.0 too)
            for (size_t g = r; g < G; g += R) {
                u64 p = partial[(g * QE_NQ + k) * (size_t)C + c0 + col];
                if (j < 3) p = p >> (QE_BITS * j) & ((1ull << QE_BITS) - 1ull);
                a = qe_join(k, a, p);
            }
            s_w[r * w + col] = a;
        }
        qe_tree(s_w, R, w, k);
        for (int e = t; e < w; e += QE_BLOCK) {
            u64 *dst = slots + (size_t)YK_QERR_WORDS * (c0 + e) + (j < 3 ? j : j + 1);
            *dst = qe_join(k, *dst, s_w[e]);
        }
    }
}

// item i of V floats of y [M][C]; V = 4: C % 4 == 0, y 16-byte and q 4-byte aligned
template <int V>
__global__ __launch_bounds__(QE_BLOCK) void dequant_kernel(const uint8_t *__restrict__ q, size_t nv, int C, Geo geo, float s, int zp, float *__restrict__ y) {
    const size_t cw = (size_t)(C / V);
    for (size_t i = (size_t)blockIdx.x * QE_BLOCK + threadIdx.x; i < nv; i += (size_t)gridDim.x * QE_BLOCK) {
        const size_t row = i / cw, at = q_row(geo, row) * (size_t)C + (i - row * cw) * V;
        if constexpr (V == 4) {
            const uint32_t b = *reinterpret_cast<const uint32_t *>(q + at);
            reinterpret_cast<float4 *>(y)[i] = make_float4((float)((int)(b & 255u) - zp) * s, (float)((int)(b >> 8 & 255u) - zp) * s,
                                                           (float)((int)(b >> 16 & 255u) - zp) * s, (float)((int)(b >> 24) - zp) * s);
        } else {
            y[i] = (float)((int)q[at] - zp) * s;
        }
    }
}

// the geometry both entry points take; -> M = B ho wo (0: refused).  M * C is a size_t after it: past 2^31 elements is fine, past 2^62 is not
inline size_t qe_geometry(int B, int qH, int qW, int C, int step, float s_y, int zp_y, Geo *geo) {
    if (B <= 0 || qH <= 0 || qW <= 0 || C <= 0 || (step != 1 && step != 2) || !(s_y - s_y == 0.f) || zp_y < 0 || zp_y > 255) return 0;
    const long long ho = (qH + step - 1) / step, wo = (qW + step - 1) / step;
    if (ho * wo > 0x7FFFFFFFll || (long long)qH * qW > (1ll << 62) / B / C) return 0;
    *geo = Geo{(size_t)(ho * wo), (int)wo, qH, qW, step};
    return (size_t)B * geo->HW;
}

}  // namespace

extern "C" int yk_qerr_workspace_bytes(long long M, int C, size_t *bytes) {
    if (M <= 0 || C <= 0 || !bytes || M > (1ll << 62) / C) {
        yk_set_error("yk_qerr_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    *bytes = sizeof(u64) * QE_NQ * qe_groups((size_t)M, C) * (size_t)C;
    return YK_OK;
}

extern "C" int yk_qerr_reset(uint64_t *d_slots, int n_slots, void *stream) {
    if (!d_slots || n_slots <= 0) {
        yk_set_error("yk_qerr_reset: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipMemsetAsync(d_slots, 0, (size_t)n_slots * YK_QERR_WORDS * sizeof(uint64_t), (hipStream_t)stream));
    return YK_OK;
}

extern "C" int yk_qerr_u8_f32(const uint8_t *q, const float *y, int B, int qH, int qW, int C, int step, float s_y, int zp_y, uint64_t *d_slots,
                              int slot0, uint64_t *d_work, void *stream) {
    Geo geo;
    const size_t M = q && y && d_slots && d_work && slot0 >= 0 && ((uintptr_t)d_slots & 7u) == 0 && ((uintptr_t)d_work & 7u) == 0
                         ? qe_geometry(B, qH, qW, C, step, s_y, zp_y, &geo) : 0;
    if (!M) {
        yk_set_error("yk_qerr_u8_f32: bad argument (step 1 or 2, a finite s_y, 0 <= zp_y <= 255, d_slots and d_work 8-byte aligned)");
        return YK_ERR_ARG;
    }
    const size_t T = qe_rows(C), G = qe_groups(M, C);
    if (G > 0x7FFFFFFFull) {
        yk_set_error("yk_qerr_u8_f32: %zu rows are more than one grid dimension of workgroups", M);
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    u64 *slots = reinterpret_cast<u64 *>(d_slots) + (size_t)YK_QERR_WORDS * slot0, *work = reinterpret_cast<u64 *>(d_work);
    if (C % 4 == 0 && aligned16(y) && ((uintptr_t)q & 3u) == 0)
        hipLaunchKernelGGL(qerr_kernel<4>, dim3((unsigned)G), dim3(QE_BLOCK), 0, st, q, y, M, C, T, geo, (double)s_y, zp_y, work, slots);
    else
        hipLaunchKernelGGL(qerr_kernel<1>, dim3((unsigned)G), dim3(QE_BLOCK), 0, st, q, y, M, C, T, geo, (double)s_y, zp_y, work, slots);
    YK_HIP(hipGetLastError());
    hipLaunchKernelGGL(qerr_finish_kernel, dim3((unsigned)((C + QE_BLOCK - 1) / QE_BLOCK)), dim3(QE_BLOCK), 0, st, (const u64 *)work, G, C, slots);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_qerr_read(const uint64_t *d_slots, int n_slots, long long *h_counts, double *h_sums) {
    if (!d_slots || n_slots <= 0 || !h_counts || !h_sums) {
        yk_set_error("yk_qerr_read: bad argument");
        return YK_ERR_ARG;
    }
    uint64_t *h = (uint64_t *)malloc((size_t)n_slots * YK_QERR_WORDS * sizeof(uint64_t));
    if (!h) {
        yk_set_error("yk_qerr_read: out of host memory");
        return YK_ERR_NOMEM;
    }
    const hipError_t e = hipMemcpy(h, d_slots, (size_t)n_slots * YK_QERR_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost);   // one copy; synchronises
    if (e != hipSuccess) {
        free(h);
        yk_set_error("yk_qerr_read: hipMemcpy -> %s", hipGetErrorString(e));
        return YK_ERR_HIP;
    }
    for (size_t i = 0; i < (size_t)n_slots; ++i) {
        for (int k = 0; k < 4; ++k) h_counts[4 * i + k] = (long long)h[YK_QERR_WORDS * i + k];
        memcpy(h_sums + 6 * i, h + YK_QERR_WORDS * i + 4, 6 * sizeof(double));
    }
    free(h);
    return YK_OK;
}

extern "C" int yk_dequant_u8_f32(const uint8_t *q, int B, int qH, int qW, int C, int step, float s_y, int zp_y, float *y, void *stream) {
    Geo geo;
    const size_t M = q && y ? qe_geometry(B, qH, qW, C, step, s_y, zp_y, &geo) : 0;
    if (!M) {
        yk_set_error("yk_dequant_u8_f32: bad argument (step 1 or 2, a finite s_y, 0 <= zp_y <= 255)");
        return YK_ERR_ARG;
    }
    const size_t n = M * (size_t)C;
    if (C % 4 == 0 && aligned16(y) && ((uintptr_t)q & 3u) == 0)
        hipLaunchKernelGGL(dequant_kernel<4>, dim3(grid_for(n / 4)), dim3(QE_BLOCK), 0, (hipStream_t)stream, q, n / 4, C, geo, s_y, zp_y, y);
    else
        hipLaunchKernelGGL(dequant_kernel<1>, dim3(grid_for(n)), dim3(QE_BLOCK), 0, (hipStream_t)stream, q, n, C, geo, s_y, zp_y, y);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
