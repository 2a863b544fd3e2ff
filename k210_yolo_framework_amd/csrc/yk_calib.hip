// yk_calib.hip — calibration for 8-bit quantisation (quantize.py): the range of every tensor of an fp32 forward pass.
//
// The minimum and the maximum of a tensor are folded on the device into a slot of YK_RANGE_WORDS uint32 words: the smallest and the largest
// ORDER-PRESERVING KEY seen so far and a sticky flag.  The key of a float is its bit pattern with the sign bit flipped (positive values)
// or all bits flipped (negative values): unsigned comparison of keys is the total order -max < ... < -0 < +0 < ... < +max, so the whole
// reduction is integer min / max - associative and commutative, hence bitwise independent of how workgroups are scheduled, of the launch
// geometry and of the stream; denormals are never flushed because no floating-point comparison touches them.  A NaN or an infinity does
// not enter the range: it sets the flag, which the host turns into an error naming the layer.
//
// Per launch: grid-stride loop with 16-byte loads (and stores), wave reduction in registers (__shfl_xor), block reduction through 2 x 4
// words of LDS, then ONE atomicMin and ONE atomicMax per workgroup (vector atomics on global memory), and an atomicOr only from a
// workgroup that met a non-finite value.  The key, the accumulator and the workgroup fold live in yk_range.h (yk_qat.hip shares them).
//
// Every kernel that finishes a conv - y = act(z * scale + bias) - makes y in scale_act below, so all of them round y the same way; the
// per-tensor ones are ONE template, tensor_kernel, over what takes y (the Range or the Hist sink), whether there is a z to finish, and
// whether the accesses are 16 bytes wide.
//
// Per channel, for cross-layer equalisation (equalize.py): yk_scale_act_chrange_f32 stores the same y and folds channel c into slot
// slot0 + c of such a buffer - a column reduction of [M][C] with lanes along the channels (scale_act_chrange_kernel below).
//
// Per channel, for bias correction (biascorrect.py): yk_scale_act_chsum_f32 stores the same y and adds the float64 sum of the PRE-activation of
// channel c to d_sum[slot0 + c] - per-workgroup partials and a fold in a fixed order, no floating-point atomics (scale_act_chsum_kernel below).
//
// Second pass, for the clipped calibrations (quantize.clip_range): a histogram of NB equal bins per tensor over the range the first pass
// found, uint64 counts [n_slots][NB].  The bin of v is  t = (v - lo) * inv  (one rounding per operation), truncated and clamped to
// [0, NB - 1]: values outside [lo, hi] land in the end bins, a NaN or an infinity is not counted and sets the slot's flag.  Same launch shape
// as the range kernels.  Each workgroup counts into a private uint32 [NB] in LDS (LDS atomics; the bin that holds real zero - most of a
// post-ReLU tensor - is first summed over the wave with a ballot, one LDS add per wave) and at the end adds its non-zero bins to global
// memory with 64-bit vector atomics.  Integer adds only: the counts do not depend on scheduling, launch geometry or stream.
#include "yk_range.h"

namespace {
using namespace yk_range;

__device__ __forceinline__ float c_act(float v, int act, float alpha) {      // as t_act of yk_train.hip
    if (act == YK_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == YK_ACT_RELU6) return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    if (act == YK_ACT_LEAKY) return v >= 0.f ? v : v * alpha;
    return v;
}

// item i of V = 1 or 4 floats (V = 4: one 16-byte access, so p + 4 * i is 16-byte aligned)
template <int V>
__device__ __forceinline__ void load_v(const float *__restrict__ p, size_t i, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 q = reinterpret_cast<const float4 *>(p)[i];
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[i];
    }
}

// THE epilogue of a conv: item i of z to item i of y, o = y = c_act(p), p = z * s + b the pre-activation (this unit compiles with
// -ffp-contract=off: two roundings).  Every kernel below that makes a y makes it here.
template <int V>
__device__ __forceinline__ void scale_act(const float *__restrict__ z, float *__restrict__ y, size_t i, const float (&s)[V], const float (&b)[V],
                                          int act, float alpha, float (&p)[V], float (&o)[V]) {
    float v[V];
    load_v<V>(z, i, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        p[j] = v[j] * s[j] + b[j];
        o[j] = c_act(p[j], act, alpha);
    }
    if constexpr (V == 4)
        reinterpret_cast<float4 *>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
    else
        y[i] = o[0];
}

// ---- per tensor: one walk, a sink for what it yields ------------------------------------------------------------------------------------
// A sink is built from its Args by every thread of the workgroup, takes values with add(float) and ends with finish(), which every
// thread calls.  Range: the min / max slot (Acc + fold of yk_range.h).  Hist, further down: the counts of one slot.
struct Range : Acc {
    struct Args {
        uint32_t *slot;
    };
    uint32_t *slot;
    __device__ __forceinline__ Range(const Args &p) : slot(p.slot) {}
    __device__ __forceinline__ void finish() { fold(*this, slot); }
};

// nv items of V floats, then the scalar tail [V * nv, n).  EPI: x is z [M][C] and each value goes through scale_act into y first; then
// C % V == 0 (V = 4: all pointers 16-byte aligned; item i starts at channel (V * i) % C and its floats share one row) and n = V * nv, no
// tail.  Without EPI the values of x are taken as they are and C ... y are not read.
template <class Sink, bool EPI, int V>
__global__ __launch_bounds__(CAL_BLOCK) void tensor_kernel(const float *__restrict__ x, size_t nv, size_t n, int C, const float *__restrict__ scale,
                                                            const float *__restrict__ bias, int act, float alpha, float *__restrict__ y,
                                                            typename Sink::Args sink_args) {
    Sink k(sink_args);
    const size_t step = (size_t)gridDim.x * CAL_BLOCK;
    const size_t cw = EPI ? (size_t)(C / V) : 1;
    for (size_t i = (size_t)blockIdx.x * CAL_BLOCK + threadIdx.x; i < nv; i += step) {
        float o[V];
        if constexpr (EPI) {
            const size_t c = i % cw;
            float s[V], b[V], p[V];
            load_v<V>(scale, c, s);
            load_v<V>(bias, c, b);
            scale_act<V>(x, y, i, s, b, act, alpha, p, o);
        } else {
            load_v<V>(x, i, o);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) k.add(o[j]);
    }
    if constexpr (!EPI)
        for (size_t i = V * nv + (size_t)blockIdx.x * CAL_BLOCK + threadIdx.x; i < n; i += step) k.add(x[i]);
    k.finish();
}

// ---- per-channel ranges (equalize.py): the column reduction of [M][C] -------------------------------------------------
// V = 4 (C % 4 == 0, 16-byte accesses) or 1 elements per thread; cw = C / V "columns".  The columns are walked in chunks of at most CAL_BLOCK;
// in a chunk of w columns thread t holds column t % w of row t / w of a tile of R = CAL_BLOCK / w whole rows (R * w <= CAL_BLOCK threads work,
// the others idle), so a tile is one contiguous piece of memory and a thread's channels never change: scale and bias are loaded once, and the
// accumulators are per channel.  Tiles are strided over the grid.  Then the R accumulators of a column are folded by a tree over rows in LDS
// and the chunk's w * V channels go to their slots: one atomicMin / atomicMax pair per channel and workgroup, none from a workgroup that saw
// nothing finite there.
constexpr int CHR_MIN_TRIPS = 4;                          // tiles a workgroup walks at least (chrange_grid)
constexpr int CHR_MIN_FOLD = 32;                          // values a workgroup folds per channel, at least, before its pair of atomics

template <int V>
__global__ __launch_bounds__(CAL_BLOCK) void scale_act_chrange_kernel(const float *__restrict__ z, size_t M, int cw, const float *__restrict__ scale,
                                                                       const float *__restrict__ bias, int act, float alpha, float *__restrict__ y,
                                                                       uint32_t *slots) {
    __shared__ uint32_t s_lo[CAL_BLOCK * V], s_hi[CAL_BLOCK * V], s_bad[CAL_BLOCK * V];
    const int t = threadIdx.x;
    for (int c0 = 0; c0 < cw; c0 += CAL_BLOCK) {
        const int w = cw - c0 < CAL_BLOCK ? cw - c0 : CAL_BLOCK;
        const int R = CAL_BLOCK / w, r = t / w;
        const size_t col = (size_t)(c0 + t % w);
        Acc a[V];
        if (r < R) {
            float s[V], b[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s[j] = scale[col * V + j];
                b[j] = bias[col * V + j];
            }
            for (size_t row = (size_t)blockIdx.x * R + r; row < M; row += (size_t)gridDim.x * R) {
                float p[V], o[V];
                scale_act<V>(z, y, row * (size_t)cw + col, s, b, act, alpha, p, o);
#pragma unroll
                for (int j = 0; j < V; ++j) a[j].add(o[j]);
            }
        }
        __syncthreads();                                                       // the previous chunk's results have been read
#pragma unroll
        for (int j = 0; j < V; ++j) {
            s_lo[t * V + j] = a[j].lo;
            s_hi[t * V + j] = a[j].hi;
            s_bad[t * V + j] = a[j].bad;
        }
        for (int n = R; n > 1;) {                                              // rows [half, n) onto rows [0, n - half): nobody reads what is written
            const int half = (n + 1) / 2;
            __syncthreads();
            if (r + half < n) {
                const int o = (t + half * w) * V;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const uint32_t l = s_lo[o + j], h = s_hi[o + j];
                    a[j].lo = l < a[j].lo ? l : a[j].lo;
                    a[j].hi = h > a[j].hi ? h : a[j].hi;
                    a[j].bad |= s_bad[o + j];
                    s_lo[t * V + j] = a[j].lo;
                    s_hi[t * V + j] = a[j].hi;
                    s_bad[t * V + j] = a[j].bad;
                }
            }
            n = half;
        }
        __syncthreads();
        for (int e = t; e < w * V; e += CAL_BLOCK) {                           // row 0 holds channel c0 * V + e at word e
            uint32_t *slot = slots + (size_t)YK_RANGE_WORDS * ((size_t)c0 * V + e);
            // a slot's min only falls and its max only rises, so a value read here - however old - that ours cannot improve means the
            // atomic would change nothing: skipped.  (Up to 2048 workgroups share C slots; once the ranges have settled, over the batches of
            // a calibration, almost none of them has anything to add.)
            if (s_lo[e] <= s_hi[e]) {
                if (s_lo[e] < __hip_atomic_load(slot + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot + 0, s_lo[e]);
                if (s_hi[e] > __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot + 1, s_hi[e]);
            }
            if (s_bad[e]) atomicOr(slot + 2, 1u);
        }
    }
}

// workgroups for M rows of cw columns: every one walks at least CHR_MIN_TRIPS tiles and folds at least CHR_MIN_FOLD values per channel
// (workgroups x C atomics beside M x C loads)
inline unsigned chrange_grid(size_t M, int cw) {
    const size_t R = (size_t)(cw < CAL_BLOCK ? CAL_BLOCK / cw : 1);
    const size_t tiles = (M + R - 1) / R;
    size_t trips = (CHR_MIN_FOLD + R - 1) / R;
    if (trips < (size_t)CHR_MIN_TRIPS) trips = CHR_MIN_TRIPS;
    const size_t g = (tiles + trips - 1) / trips;
    return (unsigned)(g < 1 ? 1 : (g > CAL_MAX_GRID ? CAL_MAX_GRID : g));
}

// ---- per-channel sums of the pre-activation (biascorrect.py) ------------------------------------------------------------
// t = z * scale + bias (fp32, BEFORE the activation: scale_act's p) summed per channel in float64, without floating-point atomics and in an
// order that (M, C) alone fix - not the pointers' alignment, the stream or the scheduling:
//   * the channels are walked in chunks of w = min(C - c0, CAL_BLOCK); a chunk has L = 4 * (CAL_BLOCK / w) ROW LANES;
//   * workgroup g owns rows [g * T, (g + 1) * T), T = chsum_rows(C); lane l of a chunk adds rows g * T + l, + L, + 2 L, ... in that order;
//   * the L lanes of a channel are folded by a tree in LDS (lanes [half, n) onto [0, n - half)), and the result is partial[g][c];
//   * the finishing launch (one workgroup per chunk) walks the G partials of a channel with R = CAL_BLOCK / w lanes the same way - lane r adds
//     g = r, r + R, ... : ceil(G / R) passes - folds them by the same tree and adds the result to d_sum[slot0 + c] (a plain load and store: calls
//     on one buffer are ordered by their stream).
// The two thread layouts realise the same lanes: with 16-byte accesses a thread is one lane of four channels (w / 4 columns x L lanes); without,
// a thread is one channel and holds lanes r, r + R, r + 2 R, r + 3 R in four accumulators, taking rows r + k R into accumulator k % 4.
// A non-finite t is not added and sets the channel's flag (an integer atomicOr from the threads that met one).
constexpr int CHS_TILE = YK_CHSUM_TILE;                   // elements a workgroup covers, about

inline size_t chsum_rows(int C) { return (size_t)((CHS_TILE + C - 1) / C); }                  // T: rows of one workgroup (>= 1)
inline size_t chsum_groups(size_t M, int C) { return (M + chsum_rows(C) - 1) / chsum_rows(C); }   // G

__device__ __forceinline__ bool chs_finite(float t) { return (__float_as_uint(t) & 0x7F800000u) != 0x7F800000u; }

// the tree over `n` lanes of `w` channels held as s[lane * w + channel]; every thread of the workgroup calls it
__device__ __forceinline__ void chs_tree(double *s, int n, int w) {
    while (n > 1) {
        const int half = (n + 1) / 2;
        __syncthreads();
        for (int e = threadIdx.x; e < (n - half) * w; e += CAL_BLOCK) s[e] += s[e + half * w];
        n = half;
    }
    __syncthreads();
}

template <int V>
__global__ __launch_bounds__(CAL_BLOCK) void scale_act_chsum_kernel(const float *__restrict__ z, size_t M, int C, size_t T, const float *__restrict__ scale,
                                                                     const float *__restrict__ bias, int act, float alpha, float *__restrict__ y,
                                                                     double *__restrict__ partial, uint32_t *flags) {
    __shared__ double s_sum[4 * CAL_BLOCK];
    const int t = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * T;
    const size_t row1 = row0 + T < M ? row0 + T : M;
    for (int c0 = 0; c0 < C; c0 += CAL_BLOCK) {
        const int w = C - c0 < CAL_BLOCK ? C - c0 : CAL_BLOCK;
        const int R = CAL_BLOCK / w, L = 4 * R;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        float s[V], b[V], p[V], o[V];
        if constexpr (V == 4) {
            const int wq = w / 4, q = t % wq, l = t / wq;                          // wq * L = R * w <= CAL_BLOCK threads work
            if (l < L) {
                const int c = c0 + 4 * q;
                load_v<4>(scale + c, 0, s);
                load_v<4>(bias + c, 0, b);
                uint32_t bad = 0u;
                for (size_t row = row0 + l; row < row1; row += L) {
                    scale_act<4>(z, y, (row * (size_t)C + c) / 4, s, b, act, alpha, p, o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (chs_finite(p[j])) a[j] += (double)p[j]; else bad |= 1u << j;
                    }
                }
                for (int j = 0; j < 4; ++j)
                    if (bad >> j & 1u) atomicOr(flags + c + j, 1u);
            }
            __syncthreads();                                                       // the previous chunk's results have been read
            if (l < L)
                for (int j = 0; j < 4; ++j) s_sum[l * w + 4 * q + j] = a[j];
        } else {
            const int col = t % w, r = t / w;
            if (r < R) {
                const int c = c0 + col;
                s[0] = scale[c], b[0] = bias[c];
                bool bad = false;
                int k = 0;
                for (size_t row = row0 + r; row < row1; row += R, k = (k + 1) & 3) {
                    scale_act<1>(z, y, row * (size_t)C + c, s, b, act, alpha, p, o);
                    if (chs_finite(p[0])) {
                        a[0] += k == 0 ? (double)p[0] : 0.0;                       // (adding +0.0 changes no finite sum)
                        a[1] += k == 1 ? (double)p[0] : 0.0;
                        a[2] += k == 2 ? (double)p[0] : 0.0;
                        a[3] += k == 3 ? (double)p[0] : 0.0;
                    } else {
                        bad = true;
                    }
                }
                if (bad) atomicOr(flags + c, 1u);
            }
            __syncthreads();
            if (r < R)
                for (int j = 0; j < 4; ++j) s_sum[(r + j * R) * w + col] = a[j];
        }
        chs_tree(s_sum, L, w);
        for (int e = t; e < w; e += CAL_BLOCK) partial[(size_t)blockIdx.x * C + c0 + e] = s_sum[e];
    }
}

// workgroup blockIdx.x = chunk c0 = blockIdx.x * CAL_BLOCK of the channels
__global__ __launch_bounds__(CAL_BLOCK) void chsum_finish_kernel(const double *__restrict__ partial, size_t G, int C, double *d_sum) {
    __shared__ double s_sum[CAL_BLOCK];
    const int t = threadIdx.x, c0 = blockIdx.x * CAL_BLOCK;
    const int w = C - c0 < CAL_BLOCK ? C - c0 : CAL_BLOCK;
    const int R = CAL_BLOCK / w, col = t % w, r = t / w;
    if (r < R) {
        double a = 0.0;
        for (size_t g = r; g < G; g += R) a += partial[g * (size_t)C + c0 + col];
        s_sum[r * w + col] = a;
    }
    chs_tree(s_sum, R, w);
    for (int e = t; e < w; e += CAL_BLOCK) d_sum[c0 + e] += s_sum[e];
}

// ---- histograms ---------------------------------------------------------------------------------------------------------------------
constexpr int HIST_MIN_BINS = 16, HIST_MAX_BINS = 4096;
constexpr bool HIST_WAVE_ZERO = true;                     // the zero bin per wave (ballot + popcount) before the per-lane LDS atomics

// truncation and clamp written as comparisons on t, so that an overflowing or NaN t (zero-width and sub-normal-width ranges) is defined:
// t >= NB -> NB - 1, t > 0 -> (int)t, anything else (t <= 0, NaN) -> 0
__device__ __forceinline__ int bin_of(float v, float lo, float inv, int nb) {
    const float t = __fmul_rn(__fsub_rn(v, lo), inv);
    return t >= (float)nb ? nb - 1 : (t > 0.f ? (int)t : 0);
}

// the sink of tensor_kernel that counts: the workgroup's uint32 [nb] in dynamic LDS (the launch gives nb * 4 bytes)
struct Hist {
    struct Args {
        float lo, inv;
        int nb;
        unsigned long long *row;                         // the slot's counts [nb]
        uint32_t *flag;
    };
    uint32_t *s_h;                                       // LDS, [nb]
    const Args p;
    int zbin;
    uint32_t bad = 0u;
    __device__ __forceinline__ Hist(const Args &args) : p(args) {
        extern __shared__ uint32_t s_hist[];
        s_h = s_hist;
        zbin = bin_of(0.f, p.lo, p.inv, p.nb);
        for (int b = threadIdx.x; b < p.nb; b += CAL_BLOCK) s_h[b] = 0u;
        __syncthreads();
    }
    __device__ __forceinline__ void add(float v) {
        const bool ok = (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u;
        if (!ok) bad = 1u;
        const int b = bin_of(v, p.lo, p.inv, p.nb);
        if (HIST_WAVE_ZERO) {
            const bool z = ok && b == zbin;
            const unsigned long long m = __ballot(z);                          // over the lanes active here
            if (z) {
                if ((int)(threadIdx.x & (YK_WAVE - 1)) == __ffsll((long long)m) - 1) atomicAdd(s_h + zbin, (uint32_t)__popcll(m));
            } else if (ok) {
                atomicAdd(s_h + b, 1u);
            }
        } else if (ok) {
            atomicAdd(s_h + b, 1u);
        }
    }
    // the workgroup's non-zero bins into the slot's row; the flag only from a workgroup that met a non-finite value
    __device__ __forceinline__ void finish() {
        __shared__ uint32_t s_bad;
        if (threadIdx.x == 0) s_bad = 0u;
        __syncthreads();                                                       // also: every LDS count is in
        if (bad) atomicOr(&s_bad, 1u);
        for (int b = threadIdx.x; b < p.nb; b += CAL_BLOCK) {
            const uint32_t c = s_h[b];
            if (c) atomicAdd(p.row + b, (unsigned long long)c);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_bad) atomicOr(p.flag, 1u);
    }
};

// what a call may histogram: NB in range, a finite lo, inv >= 0 (+inf allowed: a range narrower than NB / FLT_MAX), and no workgroup of
// `grid` that could count 2^32 elements into one uint32 bin (a workgroup takes at most n / grid + 4 * CAL_BLOCK + 3 of them)
inline bool hist_args_ok(long long n, float lo, float inv, int nbins, int slot, unsigned grid) {
    return n > 0 && nbins >= HIST_MIN_BINS && nbins <= HIST_MAX_BINS && slot >= 0 && lo - lo == 0.f && inv >= 0.f &&
           (unsigned long long)n / grid + 4ull * CAL_BLOCK + 3ull < (1ull << 32);
}

inline Hist::Args hist_sink(float lo, float inv, int nbins, uint64_t *d_hist, uint32_t *d_flags, int slot) {
    return {lo, inv, nbins, reinterpret_cast<unsigned long long *>(d_hist) + (size_t)slot * nbins, d_flags + slot};
}

// ---- what the entry points share ----------------------------------------------------------------------------------------------------------
// a tensor taken as it is: n4 float4 (none unless x is 16-byte aligned) + the scalar tail [4 * n4, n); -> the workgroups for both loops
inline unsigned plain_grid(const float *x, long long n, size_t *n4) {
    *n4 = aligned16(x) ? (size_t)n / 4 : 0;
    const size_t tail = (size_t)n - 4 * *n4;
    return grid_for(*n4 > tail ? *n4 : tail);
}

template <class Sink>
void launch_plain(unsigned grid, size_t lds, void *stream, const float *x, size_t n4, long long n, typename Sink::Args sink) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tensor_kernel<Sink, false, 4>), dim3(grid), dim3(CAL_BLOCK), lds, (hipStream_t)stream, x, n4, (size_t)n, 0,
                       (const float *)nullptr, (const float *)nullptr, 0, 0.f, (float *)nullptr, sink);
}

// the arguments every yk_scale_act_* call takes.  M * C is a size_t after it: past 2^31 elements is fine, past 2^63 is not
inline bool scale_act_args_ok(const float *z, long long M, int C, const float *scale, const float *bias, int act, const float *y) {
    return z && scale && bias && y && M > 0 && C > 0 && act >= YK_ACT_NONE && act <= YK_ACT_LEAKY && M <= (long long)(~0ull >> 1) / C;
}

// whether a yk_scale_act_* call runs its 16-byte kernel (V = 4): four channels of one row per access
inline bool scale_act_vec(const float *z, int C, const float *scale, const float *bias, const float *y) {
    return C % 4 == 0 && aligned16(z) && aligned16(y) && aligned16(scale) && aligned16(bias);
}

template <class Sink>
void launch_scale_act(bool vec, unsigned grid, size_t lds, void *stream, const float *z, size_t n, int C, const float *scale, const float *bias, int act,
                      float alpha, float *y, typename Sink::Args sink) {
    if (vec)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tensor_kernel<Sink, true, 4>), dim3(grid), dim3(CAL_BLOCK), lds, (hipStream_t)stream, z, n / 4, n, C, scale,
                           bias, act, alpha, y, sink);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tensor_kernel<Sink, true, 1>), dim3(grid), dim3(CAL_BLOCK), lds, (hipStream_t)stream, z, n, n, C, scale, bias,
                           act, alpha, y, sink);
}

__global__ void range_reset_kernel(uint32_t *r, int n_slots) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) {
        r[YK_RANGE_WORDS * i + 0] = 0xFFFFFFFFu;
        r[YK_RANGE_WORDS * i + 1] = 0u;
        r[YK_RANGE_WORDS * i + 2] = 0u;
        r[YK_RANGE_WORDS * i + 3] = 0u;
    }
}

inline float unkey(uint32_t k) {
    const uint32_t b = unkey_bits(k);
    float f;
    memcpy(&f, &b, 4);
    return f;
}

}  // namespace

extern "C" int yk_range_reset(uint32_t *d_range, int n_slots, void *stream) {
    if (!d_range || n_slots <= 0) {
        yk_set_error("yk_range_reset: bad argument");
        return YK_ERR_ARG;
    }
    hipLaunchKernelGGL(range_reset_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_range, n_slots);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_range_f32(const float *x, long long n, uint32_t *d_range, int slot, void *stream) {
    if (!x || n <= 0 || !d_range || slot < 0) {
        yk_set_error("yk_range_f32: bad argument");
        return YK_ERR_ARG;
    }
    size_t n4;
    const unsigned grid = plain_grid(x, n, &n4);
    launch_plain<Range>(grid, 0, stream, x, n4, n, {d_range + (size_t)YK_RANGE_WORDS * slot});
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_scale_act_range_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                                      uint32_t *d_range, int slot, void *stream) {
    if (!scale_act_args_ok(z, M, C, scale, bias, act, y) || !d_range || slot < 0) {
        yk_set_error("yk_scale_act_range_f32: bad argument");
        return YK_ERR_ARG;
    }
    const size_t n = (size_t)M * (size_t)C;
    const bool vec = scale_act_vec(z, C, scale, bias, y);
    launch_scale_act<Range>(vec, grid_for(vec ? n / 4 : n), 0, stream, z, n, C, scale, bias, act, alpha, y, {d_range + (size_t)YK_RANGE_WORDS * slot});
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_scale_act_chrange_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                                        uint32_t *d_range, int slot0, void *stream) {
    if (!scale_act_args_ok(z, M, C, scale, bias, act, y) || !d_range || slot0 < 0) {
        yk_set_error("yk_scale_act_chrange_f32: bad argument");
        return YK_ERR_ARG;
    }
    uint32_t *s = d_range + (size_t)YK_RANGE_WORDS * slot0;
    if (scale_act_vec(z, C, scale, bias, y))
        hipLaunchKernelGGL(scale_act_chrange_kernel<4>, dim3(chrange_grid((size_t)M, C / 4)), dim3(CAL_BLOCK), 0, (hipStream_t)stream, z, (size_t)M, C / 4,
                           scale, bias, act, alpha, y, s);
    else
        hipLaunchKernelGGL(scale_act_chrange_kernel<1>, dim3(chrange_grid((size_t)M, C)), dim3(CAL_BLOCK), 0, (hipStream_t)stream, z, (size_t)M, C, scale,
                           bias, act, alpha, y, s);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_chsum_workspace_bytes(long long M, int C, size_t *bytes) {
    if (M <= 0 || C <= 0 || !bytes || M > (long long)(~0ull >> 1) / C) {
        yk_set_error("yk_chsum_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    *bytes = sizeof(double) * chsum_groups((size_t)M, C) * (size_t)C;
    return YK_OK;
}

extern "C" int yk_chsum_reset(double *d_sum, uint32_t *d_flags, int n_slots, void *stream) {
    if (!d_sum || !d_flags || n_slots <= 0) {
        yk_set_error("yk_chsum_reset: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipMemsetAsync(d_sum, 0, (size_t)n_slots * sizeof(double), (hipStream_t)stream));
    YK_HIP(hipMemsetAsync(d_flags, 0, (size_t)n_slots * sizeof(uint32_t), (hipStream_t)stream));
    return YK_OK;
}

extern "C" int yk_scale_act_chsum_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                                      double *d_sum, uint32_t *d_flags, int slot0, double *d_work, void *stream) {
    if (!scale_act_args_ok(z, M, C, scale, bias, act, y) || !d_sum || !d_flags || !d_work || slot0 < 0 || ((uintptr_t)d_sum & 7u) != 0 ||
        ((uintptr_t)d_work & 7u) != 0) {
        yk_set_error("yk_scale_act_chsum_f32: bad argument (d_sum and d_work 8-byte aligned)");
        return YK_ERR_ARG;
    }
    const size_t T = chsum_rows(C), G = chsum_groups((size_t)M, C);
    if (G > 0x7FFFFFFFull) {
        yk_set_error("yk_scale_act_chsum_f32: M %lld is more than one grid dimension of workgroups", M);
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (scale_act_vec(z, C, scale, bias, y))
        hipLaunchKernelGGL(scale_act_chsum_kernel<4>, dim3((unsigned)G), dim3(CAL_BLOCK), 0, st, z, (size_t)M, C, T, scale, bias, act, alpha, y, d_work,
                           d_flags + slot0);
    else
        hipLaunchKernelGGL(scale_act_chsum_kernel<1>, dim3((unsigned)G), dim3(CAL_BLOCK), 0, st, z, (size_t)M, C, T, scale, bias, act, alpha, y, d_work,
                           d_flags + slot0);
    YK_HIP(hipGetLastError());
    hipLaunchKernelGGL(chsum_finish_kernel, dim3((unsigned)((C + CAL_BLOCK - 1) / CAL_BLOCK)), dim3(CAL_BLOCK), 0, st, (const double *)d_work, G, C,
                       d_sum + slot0);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_chsum_read(const double *d_sum, const uint32_t *d_flags, int n_slots, double *h_sum, int *h_flags) {
    if (!d_sum || !d_flags || n_slots <= 0 || !h_sum || !h_flags) {
        yk_set_error("yk_chsum_read: bad argument");
        return YK_ERR_ARG;
    }
    hipError_t e = hipMemcpy(h_sum, d_sum, (size_t)n_slots * sizeof(double), hipMemcpyDeviceToHost);                         // synchronises
    if (e == hipSuccess) e = hipMemcpy(h_flags, d_flags, (size_t)n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        yk_set_error("yk_chsum_read: hipMemcpy -> %s", hipGetErrorString(e));
        return YK_ERR_HIP;
    }
    return YK_OK;
}

extern "C" int yk_range_read(const uint32_t *d_range, int n_slots, float *h_min, float *h_max, int *h_flags) {
    if (!d_range || n_slots <= 0 || !h_min || !h_max || !h_flags) {
        yk_set_error("yk_range_read: bad argument");
        return YK_ERR_ARG;
    }
    uint32_t *h = (uint32_t *)malloc((size_t)n_slots * YK_RANGE_WORDS * sizeof(uint32_t));
    if (!h) {
        yk_set_error("yk_range_read: out of host memory");
        return YK_ERR_NOMEM;
    }
    const hipError_t e = hipMemcpy(h, d_range, (size_t)n_slots * YK_RANGE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost);   // one copy; synchronises
    if (e != hipSuccess) {
        free(h);
        yk_set_error("yk_range_read: hipMemcpy -> %s", hipGetErrorString(e));
        return YK_ERR_HIP;
    }
    for (int i = 0; i < n_slots; ++i) {
        const uint32_t lo = h[YK_RANGE_WORDS * i], hi = h[YK_RANGE_WORDS * i + 1];
        const bool empty = lo > hi;                                    // nothing finite folded in yet
        h_min[i] = empty ? __builtin_huge_valf() : unkey(lo);
        h_max[i] = empty ? -__builtin_huge_valf() : unkey(hi);
        h_flags[i] = (int)h[YK_RANGE_WORDS * i + 2];
    }
    free(h);
    return YK_OK;
}

extern "C" int yk_hist_reset(uint64_t *d_hist, int n_slots, int nbins, void *stream) {
    if (!d_hist || n_slots <= 0 || nbins < HIST_MIN_BINS || nbins > HIST_MAX_BINS) {
        yk_set_error("yk_hist_reset: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipMemsetAsync(d_hist, 0, (size_t)n_slots * (size_t)nbins * sizeof(uint64_t), (hipStream_t)stream));
    return YK_OK;
}

extern "C" int yk_hist_f32(const float *x, long long n, float lo, float inv, int nbins, uint64_t *d_hist, uint32_t *d_flags, int slot,
                           void *stream) {
    if (!x || !d_hist || !d_flags || n <= 0) {
        yk_set_error("yk_hist_f32: bad argument");
        return YK_ERR_ARG;
    }
    size_t n4;
    const unsigned grid = plain_grid(x, n, &n4);
    if (!hist_args_ok(n, lo, inv, nbins, slot, grid)) {
        yk_set_error("yk_hist_f32: bad argument (16 <= nbins <= 4096, finite lo, inv >= 0, n / workgroups < 2^32)");
        return YK_ERR_ARG;
    }
    launch_plain<Hist>(grid, (size_t)nbins * sizeof(uint32_t), stream, x, n4, n, hist_sink(lo, inv, nbins, d_hist, d_flags, slot));
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_scale_act_hist_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                                     float lo, float inv, int nbins, uint64_t *d_hist, uint32_t *d_flags, int slot, void *stream) {
    if (!scale_act_args_ok(z, M, C, scale, bias, act, y) || !d_hist || !d_flags) {
        yk_set_error("yk_scale_act_hist_f32: bad argument");
        return YK_ERR_ARG;
    }
    const size_t n = (size_t)M * (size_t)C;
    const bool vec = scale_act_vec(z, C, scale, bias, y);
    const unsigned grid = grid_for(vec ? n / 4 : n);
    if (!hist_args_ok((long long)n, lo, inv, nbins, slot, grid)) {
        yk_set_error("yk_scale_act_hist_f32: bad argument (16 <= nbins <= 4096, finite lo, inv >= 0, M * C / workgroups < 2^32)");
        return YK_ERR_ARG;
    }
    launch_scale_act<Hist>(vec, grid, (size_t)nbins * sizeof(uint32_t), stream, z, n, C, scale, bias, act, alpha, y,
                           hist_sink(lo, inv, nbins, d_hist, d_flags, slot));
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_hist_read(const uint64_t *d_hist, const uint32_t *d_flags, int n_slots, int nbins, uint64_t *h_counts,
                            int *h_flags) {
    if (!d_hist || !d_flags || n_slots <= 0 || nbins < HIST_MIN_BINS || nbins > HIST_MAX_BINS || !h_counts || !h_flags) {
        yk_set_error("yk_hist_read: bad argument");
        return YK_ERR_ARG;
    }
    hipError_t e = hipMemcpy(h_counts, d_hist, (size_t)n_slots * (size_t)nbins * sizeof(uint64_t), hipMemcpyDeviceToHost);   // synchronises
    if (e == hipSuccess) e = hipMemcpy(h_flags, d_flags, (size_t)n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        yk_set_error("yk_hist_read: hipMemcpy -> %s", hipGetErrorString(e));
        return YK_ERR_HIP;
    }
    return YK_OK;
}
