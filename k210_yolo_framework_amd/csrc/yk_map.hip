// yk_map.hip — the PASCAL-VOC detection metric (per-class AP, mAP) on the device, where the detections already are.
//
// The rule is voc_eval.evaluate's (k210_yolo_framework_amd/voc_eval.py), held to it integer for integer:
//
//   keys      one pass over the rows: class = the float's truncation (`astype(int)`), score -> an order-preserving 32-bit key, complemented
//             (descending), -0.0 folded onto +0.0 first.  Two 64-bit keys per row:  A = class | score  and  B = image, class | score.
//   sort      rocPRIM's stable LSD radix sort, twice, values = row indices.  Order A is the per-class curve order (score descending, row
//             ascending); order B makes every (image, class) group contiguous in the order the devkit visits it.
//   match     one wave per (image, class) group.  The detections of a group are sequential (a taken box changes the next answer); the IoUs
//             of one detection with ALL ground-truth boxes of its image and class are parallel over the lanes, in float64, in box_iou's
//             operation order; argmax with the first index on ties; then `>= iou_thresh`, difficult -> ignored, taken -> false positive.
//   curve     one workgroup per class over order A: integer inclusive scan of tp / fp, precision and recall in float64, the monotone
//             envelope as a reverse max-scan, AP as the sum over the rows where recall steps (the true positives), or the 11-point form.
//
// The COCO rule (coco_eval.evaluate) reuses the keys, the sorts and the class offsets; its matcher keeps, per ground-truth box, one
// bit per (threshold, area range) pair, its curve kernel runs once per (class, pair) and looks the 101 recall points up: see `the COCO rule` below.
//
// Everything is integer or order-independent (max) except the AP sum, which is added in a fixed order: two runs give the same bits.
// This translation unit is compiled with -ffp-contract=off: one rounding per reference operation.
#include "yk_common.h"

#include <rocprim/rocprim.hpp>   // device radix sort (the ordering step only)

namespace {

constexpr int MAP_BLOCK = 256;
constexpr int MAP_WAVES = MAP_BLOCK / YK_WAVE;
constexpr long long MAP_MAX_ROWS = 0x7fffffffLL;

inline unsigned grid_for(long long n, int per_block) {
    long long g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > 65536) g = 65536;            // grid-stride loops
    return (unsigned)g;
}

inline unsigned bits_for(unsigned long long v) {      // bits needed to hold values 0 .. v
    unsigned b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// `a[:, 5].astype(int) == c` for c in [0, class_num): the truncation toward zero; everything else (NaN too) -> class_num, which no class owns
__device__ __forceinline__ int class_of(double c, int class_num) {
    if (!(c > -1.0 && c < (double)class_num)) return class_num;
    return (int)c;
}

// descending score, +-0 equal: a smaller key = visited earlier
__device__ __forceinline__ uint32_t desc_key(float s) {
    uint32_t b = __float_as_uint(s);
    if ((b << 1) == 0u) b = 0u;
    b ^= (b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u;
    return ~b;
}

// first index k in [0, n) with a[k] >= v
__device__ __forceinline__ long long lower_bound_u64(const uint64_t *__restrict__ a, long long n, uint64_t v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- accumulation ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_BLOCK) void append_packed_kernel(const float *__restrict__ src, const int32_t *__restrict__ offsets, int n_img,
                                                                  int img_base, long long n_new, float *__restrict__ rows, int32_t *__restrict__ img) {
    const long long off0 = offsets[0];
    for (long long r = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; r < n_new; r += (long long)gridDim.x * MAP_BLOCK) {
        int lo = 0, hi = n_img;                                  // the last image b with offsets[b] - offsets[0] <= r
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((long long)offsets[mid] - off0 <= r) lo = mid; else hi = mid;
        }
        const float *s = src + (size_t)(off0 + r) * 6;
        float *d = rows + (size_t)r * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = s[k];
        img[r] = img_base + lo;
    }
}

// one workgroup per image: its first row = the sum of the counts before it
__global__ __launch_bounds__(MAP_BLOCK) void append_padded_kernel(const float *__restrict__ dets, const int32_t *__restrict__ counts, int batch, int cap,
                                                                  int img_base, long long n_new, float *__restrict__ rows, int32_t *__restrict__ img) {
    __shared__ unsigned long long before;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        if (threadIdx.x == 0) before = 0ull;
        __syncthreads();
        unsigned long long part = 0;
        for (int j = threadIdx.x; j < b; j += MAP_BLOCK) part += (unsigned long long)min(max(counts[j], 0), cap);
        if (part) atomicAdd(&before, part);
        __syncthreads();
        const long long first = (long long)before;
        const int n = min(max(counts[b], 0), cap);
        for (int k = threadIdx.x; k < n; k += MAP_BLOCK) {
            const long long r = first + k;
            if (r < n_new) {                                      // never past what the caller made room for
                const float *s = dets + ((size_t)b * cap + k) * 6;
                float *d = rows + (size_t)r * 6;
#pragma unroll
                for (int e = 0; e < 6; ++e) d[e] = s[e];
                img[r] = img_base + b;
            }
        }
        __syncthreads();
    }
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_BLOCK) void keys_kernel(const float *__restrict__ rows, const int32_t *__restrict__ img, long long n, int class_num,
                                                         uint64_t *__restrict__ key_a, uint64_t *__restrict__ key_b, uint32_t *__restrict__ iota) {
    for (long long r = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; r < n; r += (long long)gridDim.x * MAP_BLOCK) {
        const uint64_t c = (uint64_t)class_of((double)rows[(size_t)r * 6 + 5], class_num);
        const uint64_t k = desc_key(rows[(size_t)r * 6 + 4]);
        key_a[r] = (c << 32) | k;
        key_b[r] = (((uint64_t)img[r] * (uint64_t)(class_num + 1) + c) << 32) | k;
        iota[r] = (uint32_t)r;
    }
}

__global__ void class_offsets_kernel(const uint64_t *__restrict__ key_a, long long n, int class_num, int32_t *__restrict__ cls_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= class_num) cls_off[c] = (int32_t)lower_bound_u64(key_a, n, (uint64_t)c << 32);
}

__global__ __launch_bounds__(MAP_BLOCK) void gt_count_kernel(const double *__restrict__ gt, const uint8_t *__restrict__ difficult, long long n_gt_rows,
                                                             int class_num, int32_t *__restrict__ n_gt) {
    for (long long g = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; g < n_gt_rows; g += (long long)gridDim.x * MAP_BLOCK) {
        const int c = class_of(gt[(size_t)g * 6 + 5], class_num);
        if (c < class_num && !difficult[g]) atomicAdd(&n_gt[c], 1);
    }
}

// ---- matching: one wave per (image, class) group --------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_BLOCK) void match_kernel(const float *__restrict__ rows, const uint64_t *__restrict__ key_b, const uint32_t *__restrict__ row_b,
                                                          long long n, int n_img, int class_num, const double *__restrict__ gt,
                                                          const int32_t *__restrict__ gt_off, const uint8_t *__restrict__ difficult, uint8_t *taken,
                                                          double iou_thresh, double o, uint8_t *__restrict__ flags) {
    const int lane = threadIdx.x & (YK_WAVE - 1);
    const long long n_groups = (long long)n_img * class_num;
    for (long long q = (long long)blockIdx.x * MAP_WAVES + (threadIdx.x / YK_WAVE); q < n_groups; q += (long long)gridDim.x * MAP_WAVES) {
        const int i = (int)(q / class_num), c = (int)(q % class_num);
        const uint64_t gkey = (uint64_t)i * (uint64_t)(class_num + 1) + (uint64_t)c;
        const long long lo = lower_bound_u64(key_b, n, gkey << 32);
        const long long hi = lower_bound_u64(key_b, n, (gkey + 1) << 32);
        const int g0 = gt_off[i], g1 = gt_off[i + 1];
        for (long long k = lo; k < hi; ++k) {
            const uint32_t r = row_b[k];
            const float *d = rows + (size_t)r * 6;
            const double b0 = (double)d[0], b1 = (double)d[1], b2 = (double)d[2], b3 = (double)d[3];
            const double area = (b2 - b0 + o) * (b3 - b1 + o);
            double best = -1.0;
            int j = 0x7fffffff;
            for (int g = g0 + lane; g < g1; g += YK_WAVE) {
                const double *t = gt + (size_t)g * 6;
                if (class_of(t[5], class_num) != c) continue;
                const double t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
                const double ih = fmin(b2, t2) - fmax(b0, t0) + o;
                const double iw = fmin(b3, t3) - fmax(b1, t1) + o;
                const double inter = fmax(ih, 0.0) * fmax(iw, 0.0);
                const double areas = (t2 - t0 + o) * (t3 - t1 + o);
                const double uni = area + areas - inter;
                const double iou = uni > 0.0 ? inter / uni : 0.0;
                if (iou > best) {                                 // a lane's indices ascend: the first of equal values stays
                    best = iou;
                    j = g;
                }
            }
#pragma unroll
            for (int s = YK_WAVE / 2; s > 0; s >>= 1) {
                const double ob = __shfl_xor(best, s, YK_WAVE);
                const int oj = __shfl_xor(j, s, YK_WAVE);
                if (ob > best || (ob == best && oj < j)) {
                    best = ob;
                    j = oj;
                }
            }
            if (lane == 0) {                                      // one lane reads and writes `taken`: program order is the devkit's order
                uint8_t f = 2;
                if (best >= iou_thresh && j != 0x7fffffff) {
                    if (difficult[j]) f = 0;
                    else if (!taken[j]) {
                        f = 1;
                        taken[j] = 1;
                    }
                }
                flags[r] = f;
            }
        }
    }
}

// ---- curve and AP: one workgroup per class --------------------------------------------------------------------------------------------
struct AddU64 {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
struct MaxF64 {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// inclusive scan over the workgroup (Hillis-Steele through LDS); sh is free again after the call
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, T *sh, Op op) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 1; s < MAP_BLOCK; s <<= 1) {
        const T x = t >= s ? op(sh[t - s], sh[t]) : sh[t];
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
    const T out = sh[t];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(MAP_BLOCK) void ap_kernel(const uint32_t *__restrict__ row_a, const int32_t *__restrict__ cls_off, const uint8_t *__restrict__ flags,
                                                       const int32_t *__restrict__ n_gt, int use_07, uint64_t *__restrict__ cum,
                                                       int32_t *__restrict__ n_det, int32_t *__restrict__ tp, int32_t *__restrict__ fp, double *__restrict__ ap) {
    __shared__ uint64_t sh_u[MAP_BLOCK];
    __shared__ double sh_d[MAP_BLOCK];
    __shared__ uint64_t carry_u;
    __shared__ double carry_d;
    const int c = blockIdx.x, t = threadIdx.x;
    const long long lo = cls_off[c], n = (long long)cls_off[c + 1] - lo;
    const long long tiles = (n + MAP_BLOCK - 1) / MAP_BLOCK;
    // forward: cumulative tp (high word) and fp (low word), both < 2^31
    if (t == 0) carry_u = 0ull;
    __syncthreads();
    for (long long base = 0; base < n; base += MAP_BLOCK) {
        const long long k = base + t;
        uint64_t v = 0;
        if (k < n) {
            const uint8_t f = flags[row_a[lo + k]];
            v = f == 1 ? (1ull << 32) : (f == 2 ? 1ull : 0ull);
        }
        const uint64_t inc = block_scan(v, sh_u, AddU64()) + carry_u;
        if (k < n) cum[lo + k] = inc;
        __syncthreads();
        if (t == MAP_BLOCK - 1) carry_u = inc;
        __syncthreads();
    }
    const int ngt = n_gt[c];
    if (t == 0) {
        n_det[c] = (int32_t)n;
        tp[c] = (int32_t)(carry_u >> 32);
        fp[c] = (int32_t)(carry_u & 0xffffffffull);
        if (ngt == 0) ap[c] = __builtin_nan("");
    }
    if (ngt == 0) return;
    // backward: thread 0 holds the LAST row of a tile, so an inclusive max-scan over the threads is the reverse max-scan over the rows
    const double dgt = (double)ngt;
    double sum = 0.0, m11[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) m11[q] = 0.0;
    if (t == 0) carry_d = 0.0;
    __syncthreads();
    for (long long tile = tiles - 1; tile >= 0; --tile) {
        const long long k = tile * MAP_BLOCK + (MAP_BLOCK - 1 - t);
        double prec = 0.0, ctp = 0.0;
        uint64_t cu = 0;
        if (k < n) {
            cu = cum[lo + k];
            ctp = (double)(uint32_t)(cu >> 32);
            const double cfp = (double)(uint32_t)(cu & 0xffffffffull);
            prec = ctp / fmax(ctp + cfp, 2.220446049250313e-16);
        }
        const double env = fmax(block_scan(prec, sh_d, MaxF64()), carry_d);
        if (k < n) {
            const double rec = ctp / dgt;
            if (use_07) {
#pragma unroll
                for (int q = 0; q < 11; ++q)
                    if (rec >= (0.0 + (double)q * 0.1) - 1e-12) m11[q] = fmax(m11[q], prec);
            } else {
                const uint64_t before = k > 0 ? cum[lo + k - 1] : 0ull;
                if ((before >> 32) != (cu >> 32)) sum += (rec - (ctp - 1.0) / dgt) * env;      // recall steps at a true positive only
            }
        }
        __syncthreads();
        if (t == MAP_BLOCK - 1) carry_d = env;
        __syncthreads();
    }
    if (use_07) {
        double out = 0.0;
        for (int q = 0; q < 11; ++q) {
            const double m = block_scan(m11[q], sh_d, MaxF64());
            if (t == MAP_BLOCK - 1) out += m / 11.0;              // the eleven terms in order, in one thread
        }
        if (t == MAP_BLOCK - 1) ap[c] = out;
    } else {
        sh_d[t] = sum;
        __syncthreads();
        for (int s = MAP_BLOCK / 2; s > 0; s >>= 1) {             // a fixed tree: the same bits every run
            if (t < s) sh_d[t] += sh_d[t + s];
            __syncthreads();
        }
        if (t == 0) ap[c] = sh_d[0];
    }
}

__global__ void map_mean_kernel(const double *__restrict__ ap, int class_num, double *__restrict__ map) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        int n = 0;
        for (int c = 0; c < class_num; ++c)
            if (ap[c] == ap[c]) {
                s += ap[c];
                ++n;
            }
        map[0] = n ? s / (double)n : __builtin_nan("");
    }
}

// ---- the COCO rule (coco_eval.evaluate) ---------------------------------------------------------------------------------
// T thresholds x A area ranges = at most 64 (t, a) pairs; pair (t, a) is BIT a * T + t of every 64-bit mask and PLANE a * T + t of the flags.
constexpr int COCO_MAX_BITS = 64;
constexpr int COCO_MAX_REC = 1024;

// per ground-truth box: the pairs under which it is ignored (difficult, or its area outside the range); per (class, range) the boxes that are not
__global__ __launch_bounds__(MAP_BLOCK) void coco_gt_kernel(const double *__restrict__ gt, const uint8_t *__restrict__ difficult, long long n_gt_rows,
                                                            int class_num, const double *__restrict__ area_rng, int T, int A,
                                                            uint64_t *__restrict__ ign, int32_t *__restrict__ npig) {
    const uint64_t row = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
    for (long long g = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; g < n_gt_rows; g += (long long)gridDim.x * MAP_BLOCK) {
        const double *t = gt + (size_t)g * 6;
        const int c = class_of(t[5], class_num);
        const double area = (t[2] - t[0]) * (t[3] - t[1]);
        const bool hard = difficult[g] != 0;
        uint64_t m = 0;
        for (int a = 0; a < A; ++a) {
            if (hard || area < area_rng[2 * a] || area > area_rng[2 * a + 1]) m |= row << (a * T);
            else if (c < class_num) atomicAdd(&npig[c * A + a], 1);
        }
        ign[g] = m;
    }
}

// the larger of two candidates: a non-ignored box before an ignored one (bit 63 of the key), then the IoU (its bits: IoU >= +0), then the HIGHER index
__device__ __forceinline__ bool coco_after(uint64_t ka, int ia, uint64_t kb, int ib) { return ka > kb || (ka == kb && ia > ib); }

// One wave per (image, class) group; its detections are sequential.  A chunk of 64 boxes of the image is spread over the lanes: the IoU of the
// detection with a lane's box is computed once and serves every pair.  Per pair the candidates (class, IoU >= threshold, not matched under the
// pair) are found by a ballot: none - nothing to do; one - it is the winner; more - a wave max over (key, index).  Lane b keeps the winner of pair
// b across the chunks, writes pair b's flag, and the lane that owns the winning box sets bit b of its mask (a box is always read and written
// by the same lane: program order is the matching order).  A detection none of whose boxes reaches the lowest threshold skips all of that.
__global__ __launch_bounds__(MAP_BLOCK) void coco_match_kernel(const float *__restrict__ rows, const uint64_t *__restrict__ key_b, const uint32_t *__restrict__ row_b,
                                                               long long n, int n_img, int class_num, const double *__restrict__ gt,
                                                               const int32_t *__restrict__ gt_off, const uint64_t *__restrict__ ign, uint64_t *matched,
                                                               const double *__restrict__ iou_thr, const double *__restrict__ area_rng, int T, int A,
                                                               int max_dets, uint8_t *__restrict__ flags, int32_t *__restrict__ n_det) {
    __shared__ double sh_thr[COCO_MAX_BITS], sh_a0[COCO_MAX_BITS], sh_a1[COCO_MAX_BITS];
    const int nb = T * A;
    if ((int)threadIdx.x < nb) {
        sh_thr[threadIdx.x] = fmin(iou_thr[threadIdx.x % T], 1.0 - 1e-10);
        sh_a0[threadIdx.x] = area_rng[2 * (threadIdx.x / T)];
        sh_a1[threadIdx.x] = area_rng[2 * (threadIdx.x / T) + 1];
    }
    __syncthreads();
    double thr_min = sh_thr[0];
    for (int t = 1; t < T; ++t) thr_min = fmin(thr_min, sh_thr[t]);
    const int lane = threadIdx.x & (YK_WAVE - 1);
    const bool pair = lane < nb;
    const double my_a0 = pair ? sh_a0[lane] : 0.0, my_a1 = pair ? sh_a1[lane] : 0.0;
    const long long n_groups = (long long)n_img * class_num;
    for (long long q = (long long)blockIdx.x * MAP_WAVES + (threadIdx.x / YK_WAVE); q < n_groups; q += (long long)gridDim.x * MAP_WAVES) {
        const int i = (int)(q / class_num), c = (int)(q % class_num);
        const uint64_t gkey = (uint64_t)i * (uint64_t)(class_num + 1) + (uint64_t)c;
        const long long lo = lower_bound_u64(key_b, n, gkey << 32);
        long long hi = lower_bound_u64(key_b, n, (gkey + 1) << 32);
        if (hi - lo > (long long)max_dets) hi = lo + max_dets;           // the rest takes no part: flag 0 (the memset), counted nowhere
        if (hi <= lo) continue;
        if (lane == 0) atomicAdd(&n_det[c], (int32_t)(hi - lo));
        const int g0 = gt_off[i], g1 = gt_off[i + 1];
        for (long long k = lo; k < hi; ++k) {
            const uint32_t r = row_b[k];
            const float *d = rows + (size_t)r * 6;
            const double b0 = (double)d[0], b1 = (double)d[1], b2 = (double)d[2], b3 = (double)d[3];
            const double area = (b2 - b0) * (b3 - b1);
            uint64_t win_key = 0;                                         // lane b: the winner of pair b so far
            int win = -1;
            for (int gb = g0; gb < g1; gb += YK_WAVE) {
                const int g = gb + lane;
                double iou = -1.0;
                uint64_t ig = 0, mt = 0;
                if (g < g1) {
                    const double *t = gt + (size_t)g * 6;
                    if (class_of(t[5], class_num) == c) {
                        const double t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
                        const double ih = fmin(b2, t2) - fmax(b0, t0);
                        const double iw = fmin(b3, t3) - fmax(b1, t1);
                        const double inter = fmax(ih, 0.0) * fmax(iw, 0.0);
                        const double areas = (t2 - t0) * (t3 - t1);
                        const double uni = area + areas - inter;
                        iou = uni > 0.0 ? inter / uni : 0.0;
                        if (iou == 0.0) iou = 0.0;                        // -0.0 -> +0.0: the key below is the bits of a value >= +0
                    }
                }
                const bool near = iou >= thr_min;
                if (__ballot(near) == 0ull) continue;                     // wave-uniform
                if (near) {
                    ig = ign[g];
                    mt = matched[g];
                }
                const uint64_t iou_bits = near ? (uint64_t)__double_as_longlong(iou) : 0ull;
                for (int b = 0; b < nb; ++b) {
                    const bool cand = near && iou >= sh_thr[b] && !((mt >> b) & 1ull);
                    const uint64_t who = __ballot(cand);
                    if (who == 0ull) continue;                            // wave-uniform
                    uint64_t key = cand ? (iou_bits | (((ig >> b) & 1ull) ? 0ull : (1ull << 63))) : 0ull;
                    int idx = cand ? g : -1;
                    if (who & (who - 1ull)) {
#pragma unroll
                        for (int s = YK_WAVE / 2; s > 0; s >>= 1) {
                            const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)key, s, YK_WAVE);
                            const int oi = __shfl_xor(idx, s, YK_WAVE);
                            if (coco_after(ok, oi, key, idx)) {
                                key = ok;
                                idx = oi;
                            }
                        }
                    } else {
                        const int src = __ffsll((unsigned long long)who) - 1;
                        key = (uint64_t)__shfl((unsigned long long)key, src, YK_WAVE);
                        idx = __shfl(idx, src, YK_WAVE);
                    }
                    if (lane == b && coco_after(key, idx, win_key, win)) {   // chunks ascend: a later chunk's index is higher
                        win_key = key;
                        win = idx;
                    }
                }
            }
            // lane b: pair b's outcome
            if (pair) {
                uint8_t f;
                if (win >= 0) f = (win_key >> 63) ? 1 : 0;
                else f = (area < my_a0 || area > my_a1) ? 0 : 2;
                flags[(size_t)lane * (size_t)n + r] = f;
            }
            // the owner of a winning box marks it under the pair
            uint64_t won = __ballot(win >= 0);
            while (won) {
                const int b = __ffsll((unsigned long long)won) - 1;
                won &= won - 1ull;
                const int m = __shfl(win, b, YK_WAVE);
                if (((m - g0) & (YK_WAVE - 1)) == lane) matched[m] |= 1ull << b;
            }
        }
    }
}

// One workgroup per (class, pair) over order A: the integer scan of tp / fp as ap_kernel's; per recall point the smallest integer tp with
// (double)tp / npig >= the point and the first row that reaches it (a binary search of the scan); the reverse max-scan of the precision, written
// over the scan; then the look-ups.
__global__ __launch_bounds__(MAP_BLOCK) void coco_curve_kernel(const uint32_t *__restrict__ row_a, const int32_t *__restrict__ cls_off, const uint8_t *__restrict__ flags,
                                                               long long n_rows, const int32_t *__restrict__ npig, const double *__restrict__ rec_thr, int n_rec,
                                                               int class_num, int T, int A, uint64_t *cum_all, double *__restrict__ precision,
                                                               double *__restrict__ recall) {
    __shared__ uint64_t sh_u[MAP_BLOCK];
    __shared__ double sh_d[MAP_BLOCK];
    __shared__ uint64_t carry_u;
    __shared__ double carry_d;
    __shared__ int32_t sh_row[COCO_MAX_REC];
    const int nb = T * A;
    const int c = blockIdx.x / nb, b = blockIdx.x % nb, ta = b / T, tt = b % T, t = threadIdx.x;
    const long long lo = cls_off[c], n = (long long)cls_off[c + 1] - lo;
    const uint8_t *fl = flags + (size_t)b * (size_t)n_rows;
    uint64_t *cum = cum_all + (size_t)b * (size_t)n_rows;
    const int ng = npig[c * A + ta];
    double *pout = precision + ((size_t)tt * n_rec * class_num + c) * A + ta;          // + r * class_num * A
    const size_t pstep = (size_t)class_num * A;
    if (ng == 0) {                                                                      // absent
        for (int r = t; r < n_rec; r += MAP_BLOCK) pout[(size_t)r * pstep] = -1.0;
        if (t == 0) recall[((size_t)tt * class_num + c) * A + ta] = -1.0;
        return;
    }
    if (t == 0) carry_u = 0ull;
    __syncthreads();
    for (long long base = 0; base < n; base += MAP_BLOCK) {
        const long long k = base + t;
        uint64_t v = 0;
        if (k < n) {
            const uint8_t f = fl[row_a[lo + k]];
            v = f == 1 ? (1ull << 32) : (f == 2 ? 1ull : 0ull);
        }
        const uint64_t inc = block_scan(v, sh_u, AddU64()) + carry_u;
        if (k < n) cum[lo + k] = inc;
        __syncthreads();
        if (t == MAP_BLOCK - 1) carry_u = inc;
        __syncthreads();
    }
    const double dgt = (double)ng;
    const long long total = (long long)(carry_u >> 32);
    if (t == 0) recall[((size_t)tt * class_num + c) * A + ta] = n > 0 ? (double)total / dgt : 0.0;
    // the row of every recall point: searchsorted(rc, point, 'left'), or -1 past the end
    for (int r = t; r < n_rec; r += MAP_BLOCK) {
        const double want = rec_thr[r];
        double est = ceil(want * dgt);                                                  // an estimate; the two loops make it exact
        if (!(est >= 0.0)) est = 0.0;
        if (est > dgt + 1.0) est = dgt + 1.0;
        long long tp = (long long)est;
        while (tp > 0 && (double)(tp - 1) / dgt >= want) --tp;
        while (tp <= (long long)ng && !((double)tp / dgt >= want)) ++tp;
        int32_t row = -1;
        if (tp <= total && n > 0) {
            long long a0 = 0, a1 = n;                                                   // the first row whose tp count is >= tp
            while (a0 < a1) {
                const long long mid = a0 + ((a1 - a0) >> 1);
                if ((long long)(cum[lo + mid] >> 32) < tp) a0 = mid + 1; else a1 = mid;
            }
            row = (int32_t)a0;
        }
        sh_row[r] = row;
    }
    if (t == 0) carry_d = 0.0;
    __syncthreads();
    // backward: thread 0 holds the LAST row of a tile (ap_kernel); the envelope replaces the scan
    const long long tiles = (n + MAP_BLOCK - 1) / MAP_BLOCK;
    for (long long tile = tiles - 1; tile >= 0; --tile) {
        const long long k = tile * MAP_BLOCK + (MAP_BLOCK - 1 - t);
        double prec = 0.0;
        if (k < n) {
            const uint64_t cu = cum[lo + k];
            const double ctp = (double)(uint32_t)(cu >> 32);
            const double cfp = (double)(uint32_t)(cu & 0xffffffffull);
            prec = ctp / ((cfp + ctp) + 2.220446049250313e-16);
        }
        const double env = fmax(block_scan(prec, sh_d, MaxF64()), carry_d);
        if (k < n) cum[lo + k] = (uint64_t)__double_as_longlong(env);
        __syncthreads();
        if (t == MAP_BLOCK - 1) carry_d = env;
        __syncthreads();
    }
    for (int r = t; r < n_rec; r += MAP_BLOCK) {
        const int32_t row = sh_row[r];
        pout[(size_t)r * pstep] = row >= 0 ? __longlong_as_double((long long)cum[lo + row]) : 0.0;
    }
}

// The summary: one workgroup per figure (0 ap, 1 ap50, 2 ap75, 3-5 ap small / medium / large, 6 ar, 7-9 ar small / medium / large, 10 + k
// ap_class[k]): the mean of the entries > -1 of its slice, NaN if there are none.  Every thread adds its entries in index order, then a fixed tree.
__global__ __launch_bounds__(MAP_BLOCK) void coco_summary_kernel(const double *__restrict__ precision, const double *__restrict__ recall,
                                                                 const double *__restrict__ iou_thr, int T, int n_rec, int class_num, int A,
                                                                 double *__restrict__ summary, double *__restrict__ ap_class) {
    __shared__ double sh_s[MAP_BLOCK];
    __shared__ unsigned long long sh_n[MAP_BLOCK];
    const int fig = blockIdx.x, t = threadIdx.x;
    const bool is_ar = fig >= 6 && fig < 10, one_class = fig >= 10;
    const int ta = one_class ? 0 : (fig < 3 ? 0 : (fig < 6 ? fig - 2 : fig - 6));
    const int k0 = one_class ? fig - 10 : 0, nk = one_class ? 1 : class_num;
    const double only = fig == 1 ? 0.5 : 0.75;
    const bool pick = fig == 1 || fig == 2;
    const int per_t = is_ar ? nk : n_rec * nk;
    double s = 0.0;
    unsigned long long cnt = 0;
    if (ta < A) {
        for (long long e = t; e < (long long)T * per_t; e += MAP_BLOCK) {
            const int tt = (int)(e / per_t), rest = (int)(e % per_t);
            if (pick && !(iou_thr[tt] == only)) continue;
            const int k = k0 + rest % nk, r = rest / nk;
            const double v = is_ar ? recall[((size_t)tt * class_num + k) * A + ta]
                                   : precision[(((size_t)tt * n_rec + r) * class_num + k) * A + ta];
            if (v > -1.0) {
                s += v;
                ++cnt;
            }
        }
    }
    sh_s[t] = s;
    sh_n[t] = cnt;
    __syncthreads();
    for (int w = MAP_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            sh_s[t] += sh_s[t + w];
            sh_n[t] += sh_n[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double m = sh_n[0] ? sh_s[0] / (double)sh_n[0] : __builtin_nan("");
        if (one_class) ap_class[k0] = m; else summary[fig] = m;
    }
}

// ---- operating points (oppoint.py) --------------------------------------------------------------------------------------
// sweep: the rows' flags are yk_map_eval's; a row of score s is in at the first j thresholds, j = the number of thresholds <= float64(s).  An
// integer histogram per (flag, class, j - 1), its suffix sums are tp / fp; the curves are fixed chains of float64 operations on those integers.
constexpr int SWEEP_MAX_THR = 4096;

__global__ __launch_bounds__(MAP_BLOCK) void sweep_hist_kernel(const float *__restrict__ rows, const uint8_t *__restrict__ flags, long long n, int class_num,
                                                               const double *__restrict__ thr, int n_thr, int32_t *__restrict__ hist) {
    for (long long r = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; r < n; r += (long long)gridDim.x * MAP_BLOCK) {
        const uint8_t f = flags[r];
        if (f != 1 && f != 2) continue;
        const int c = class_of((double)rows[(size_t)r * 6 + 5], class_num);
        if (c >= class_num) continue;
        const double s = (double)rows[(size_t)r * 6 + 4];
        int lo = 0, hi = n_thr;                                   // the first k with thr[k] > s = the number of thresholds <= s
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (thr[mid] <= s) lo = mid + 1; else hi = mid;
        }
        if (lo > 0) atomicAdd(&hist[((size_t)(f - 1) * class_num + c) * n_thr + (lo - 1)], 1);
    }
}

// the larger f1, then the lower index
__device__ __forceinline__ bool sweep_better(double fa, int ka, double fb, int kb) { return fa > fb || (fa == fb && ka < kb); }

// one wave per class: lane 0 holds the HIGHEST threshold of a chunk, so an inclusive scan over the lanes is the suffix sum over the thresholds
__global__ __launch_bounds__(YK_WAVE) void sweep_curve_kernel(const int32_t *__restrict__ hist, const int32_t *__restrict__ n_gt, int class_num, int n_thr,
                                                              int32_t *__restrict__ tp, int32_t *__restrict__ fp, double *__restrict__ precision,
                                                              double *__restrict__ recall, double *__restrict__ f1, int32_t *__restrict__ best) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int32_t *h_tp = hist + (size_t)c * n_thr, *h_fp = hist + ((size_t)class_num + c) * n_thr;
    const int ngt = n_gt[c];
    const double dgt = (double)ngt;
    int carry_tp = 0, carry_fp = 0, bk = 0x7fffffff;
    double bf = -1.0;
    for (int top = n_thr - 1; top >= 0; top -= YK_WAVE) {
        const int k = top - lane;
        int a = k >= 0 ? h_tp[k] : 0, b = k >= 0 ? h_fp[k] : 0;
#pragma unroll
        for (int s = 1; s < YK_WAVE; s <<= 1) {
            const int oa = __shfl_up(a, s, YK_WAVE), ob = __shfl_up(b, s, YK_WAVE);
            if (lane >= s) {
                a += oa;
                b += ob;
            }
        }
        a += carry_tp;
        b += carry_fp;
        carry_tp = __shfl(a, YK_WAVE - 1, YK_WAVE);
        carry_fp = __shfl(b, YK_WAVE - 1, YK_WAVE);
        if (k >= 0) {
            const size_t at = (size_t)c * n_thr + k;
            tp[at] = a;
            fp[at] = b;
            const double t = (double)a;
            const double p = (a + b == 0) ? 1.0 : t / (double)(a + b);
            double r = __builtin_nan(""), f = __builtin_nan("");
            if (ngt > 0) {
                r = t / dgt;
                const double pr = p + r;
                f = pr == 0.0 ? 0.0 : ((2.0 * p) * r) / pr;
                if (sweep_better(f, k, bf, bk)) {
                    bf = f;
                    bk = k;
                }
            }
            precision[at] = p;
            recall[at] = r;
            f1[at] = f;
        }
    }
#pragma unroll
    for (int s = YK_WAVE / 2; s > 0; s >>= 1) {
        const double of = __shfl_xor(bf, s, YK_WAVE);
        const int ok = __shfl_xor(bk, s, YK_WAVE);
        if (sweep_better(of, ok, bf, bk)) {
            bf = of;
            bk = ok;
        }
    }
    if (lane == 0) best[c] = ngt > 0 ? bk : -1;
}

// one thread per threshold: the classes with ground truth in ascending order, one after another
__global__ __launch_bounds__(MAP_BLOCK) void sweep_mean_kernel(const double *__restrict__ f1, const int32_t *__restrict__ n_gt, int class_num, int n_thr,
                                                               double *__restrict__ mean_f1) {
    const int k = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (k >= n_thr) return;
    double s = 0.0;
    int n = 0;
    for (int c = 0; c < class_num; ++c)
        if (n_gt[c] > 0) {
            s = s + f1[(size_t)c * n_thr + k];
            ++n;
        }
    mean_f1[k] = n ? s / (double)n : __builtin_nan("");
}

// one wave: the lowest index of the largest mean (a NaN mean = no class has ground truth = -1)
__global__ __launch_bounds__(YK_WAVE) void sweep_best_all_kernel(const double *__restrict__ mean_f1, int n_thr, int32_t *__restrict__ best_all) {
    const int lane = threadIdx.x;
    double bf = -1.0;
    int bk = 0x7fffffff;
    for (int k = lane; k < n_thr; k += YK_WAVE) {
        const double f = mean_f1[k];
        if (f == f && sweep_better(f, k, bf, bk)) {
            bf = f;
            bk = k;
        }
    }
#pragma unroll
    for (int s = YK_WAVE / 2; s > 0; s >>= 1) {
        const double of = __shfl_xor(bf, s, YK_WAVE);
        const int ok = __shfl_xor(bk, s, YK_WAVE);
        if (sweep_better(of, ok, bf, bk)) {
            bf = of;
            bk = ok;
        }
    }
    if (lane == 0) best_all[0] = bk == 0x7fffffff ? -1 : bk;
}

// confusion: one workgroup of ONE wave per image, so that __syncthreads() orders lane 0's writes of the matching state (d_match of the rows,
// `taken` of the boxes, both in global memory) before every lane's reads of the next round.  d_match doubles as the rows' state: -2 takes no
// part, -1 free, >= 0 the box.  taken: 0 free, 1 matched, 2 takes no part.  While the rows taking part + the boxes of the image fit CONF_LDS
// their coordinates are staged in LDS as float64 (rows compacted: slot -> row index); above it the same loop reads them from global memory.
constexpr int CONF_LDS = 1024;

struct ConfKey {
    double iou;
    float score;
    int row, box;
};
// the larger IoU, then the larger score (-0.0 == +0.0 as floats compare), then the lower row, then the lower box
__device__ __forceinline__ bool conf_better(const ConfKey &a, const ConfKey &b) {
    if (a.iou != b.iou) return a.iou > b.iou;
    if (a.score != b.score) return a.score > b.score;
    if (a.row != b.row) return a.row < b.row;
    return a.box < b.box;
}

__device__ __forceinline__ int lower_bound_i32(const int32_t *__restrict__ a, long long n, int v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (int)lo;
}

__global__ __launch_bounds__(YK_WAVE) void confusion_kernel(const float *__restrict__ rows, const int32_t *__restrict__ img, long long n_rows, int n_img,
                                                            const double *__restrict__ gt, const int32_t *__restrict__ gt_off,
                                                            const uint8_t *__restrict__ difficult, int class_num, double conf_thresh, double iou_thresh,
                                                            double o, uint8_t *taken, int32_t *matrix, int32_t *match) {
    __shared__ double sh_box[CONF_LDS * 4];
    __shared__ float sh_score[CONF_LDS];
    __shared__ int32_t sh_row[CONF_LDS];
    const int lane = threadIdx.x;
    const int K1 = class_num + 1;
    for (int i = blockIdx.x; i < n_img; i += gridDim.x) {
        const int r0 = lower_bound_i32(img, n_rows, i), r1 = lower_bound_i32(img, n_rows, i + 1);
        const int g0 = gt_off[i], g1 = gt_off[i + 1];
        const int nbx = g1 - g0;
        __syncthreads();                                          // the previous image's LDS is no longer read
        // who takes part; the rows that do are compacted into LDS while they fit
        int nd = 0;
        for (int base = r0; base < r1; base += YK_WAVE) {
            const int r = base + lane;
            bool part = false;
            if (r < r1) {
                const float *d = rows + (size_t)r * 6;
                part = (double)d[4] >= conf_thresh && class_of((double)d[5], class_num) < class_num;
                match[r] = part ? -1 : -2;
            }
            const unsigned long long who = __ballot(part);
            const int at = nd + __popcll(who & ((1ull << lane) - 1ull));
            if (part && at < CONF_LDS) {
                const float *d = rows + (size_t)r * 6;
#pragma unroll
                for (int e = 0; e < 4; ++e) sh_box[at * 4 + e] = (double)d[e];
                sh_score[at] = d[4];
                sh_row[at] = r;
            }
            nd += __popcll(who);
        }
        const bool staged = (long long)nd + nbx <= CONF_LDS;
        for (int g = g0 + lane; g < g1; g += YK_WAVE) {
            taken[g] = class_of(gt[(size_t)g * 6 + 5], class_num) < class_num ? 0 : 2;
            if (staged) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sh_box[(nd + (g - g0)) * 4 + e] = gt[(size_t)g * 6 + e];
            }
        }
        __syncthreads();
        // the rounds: every lane strides over the pairs (row slot, box), the wave keeps the best free pair
        const int n_slots = staged ? nd : r1 - r0;               // staged: the rows taking part; global: every row of the image
        const long long n_pairs = (long long)n_slots * nbx;
        const int max_rounds = nd < nbx ? nd : nbx;
        for (int round = 0; round < max_rounds; ++round) {
            ConfKey best = {-1.0, 0.0f, 0x7fffffff, 0x7fffffff};
            for (long long p = lane; p < n_pairs; p += YK_WAVE) {
                const int slot = (int)(p / nbx), g = g0 + (int)(p % nbx);
                const int r = staged ? sh_row[slot] : r0 + slot;
                if (match[r] != -1 || taken[g] != 0) continue;
                double b0, b1, b2, b3, t0, t1, t2, t3;
                float sc;
                if (staged) {
                    const double *b = sh_box + slot * 4, *t = sh_box + (nd + (g - g0)) * 4;
                    b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
                    sc = sh_score[slot];
                } else {
                    const float *b = rows + (size_t)r * 6;
                    const double *t = gt + (size_t)g * 6;
                    b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2], b3 = (double)b[3], t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
                    sc = b[4];
                }
                const double ih = fmin(b2, t2) - fmax(b0, t0) + o;
                const double iw = fmin(b3, t3) - fmax(b1, t1) + o;
                const double inter = fmax(ih, 0.0) * fmax(iw, 0.0);
                const double area = (b2 - b0 + o) * (b3 - b1 + o);
                const double areas = (t2 - t0 + o) * (t3 - t1 + o);
                const double uni = area + areas - inter;
                const double iou = uni > 0.0 ? inter / uni : 0.0;
                if (!(iou >= iou_thresh)) continue;
                const ConfKey key = {iou, sc, r, g};
                if (best.row == 0x7fffffff || conf_better(key, best)) best = key;
            }
#pragma unroll
            for (int s = YK_WAVE / 2; s > 0; s >>= 1) {
                ConfKey other;
                other.iou = __shfl_xor(best.iou, s, YK_WAVE);
                other.score = __shfl_xor(best.score, s, YK_WAVE);
                other.row = __shfl_xor(best.row, s, YK_WAVE);
                other.box = __shfl_xor(best.box, s, YK_WAVE);
                if (other.row != 0x7fffffff && (best.row == 0x7fffffff || conf_better(other, best))) best = other;
            }
            if (best.row == 0x7fffffff) break;                    // wave-uniform: no candidate pair is left
            if (lane == 0) {
                match[best.row] = best.box;
                taken[best.box] = 1;
            }
            __syncthreads();
        }
        __syncthreads();
        // the counts
        for (int r = r0 + lane; r < r1; r += YK_WAVE) {
            const int m = match[r];
            if (m == -2) continue;
            const int pc = class_of((double)rows[(size_t)r * 6 + 5], class_num);
            if (m == -1) atomicAdd(&matrix[class_num * K1 + pc], 1);
            else if (!difficult[m]) atomicAdd(&matrix[class_of(gt[(size_t)m * 6 + 5], class_num) * K1 + pc], 1);
        }
        for (int g = g0 + lane; g < g1; g += YK_WAVE)
            if (taken[g] == 0 && !difficult[g]) atomicAdd(&matrix[class_of(gt[(size_t)g * 6 + 5], class_num) * K1 + class_num], 1);
    }
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------
struct Work {
    size_t key_a_in, key_a, key_b_in, key_b, iota, row_a, row_b, cum, taken, cls_off, sort_tmp, sort_bytes, total;
    unsigned bits_a, bits_b;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

int layout(long long n_rows, long long n_gt_rows, int n_img, int class_num, Work *w) {
    const size_t R = (size_t)(n_rows > 0 ? n_rows : 1), G = (size_t)(n_gt_rows > 0 ? n_gt_rows : 1);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += up256(bytes);
        return o;
    };
    w->key_a_in = take(R * 8);
    w->key_a = take(R * 8);
    w->key_b_in = take(R * 8);
    w->key_b = take(R * 8);
    w->iota = take(R * 4);
    w->row_a = take(R * 4);
    w->row_b = take(R * 4);
    w->cum = take(R * 8);
    w->taken = take(G);
    w->cls_off = take((size_t)(class_num + 1) * 4);
    w->bits_a = 32 + bits_for((unsigned long long)class_num);
    w->bits_b = 32 + bits_for((unsigned long long)(n_img > 0 ? n_img : 1) * (unsigned long long)(class_num + 1));
    if (w->bits_b > 64) w->bits_b = 64;
    size_t bytes = 0;
    if (n_rows > 0) {                                             // size queries only: nothing is launched
        uint64_t *k = nullptr;
        uint32_t *v = nullptr;
        size_t a = 0, b = 0;
        if (rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, (size_t)n_rows, 0u, w->bits_a) != hipSuccess) return YK_ERR_HIP;
        if (rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, (size_t)n_rows, 0u, w->bits_b) != hipSuccess) return YK_ERR_HIP;
        bytes = a > b ? a : b;
    }
    w->sort_bytes = bytes;
    w->sort_tmp = take(bytes ? bytes : 1);
    w->total = at;
    return YK_OK;
}

int check_sizes(const char *who, long long n_rows, long long n_gt_rows, int n_img, int class_num) {
    if (n_rows < 0 || n_gt_rows < 0 || n_img < 0 || class_num <= 0) {
        yk_set_error("%s: bad argument", who);
        return YK_ERR_ARG;
    }
    if (n_rows > MAP_MAX_ROWS || n_gt_rows > MAP_MAX_ROWS) {
        yk_set_error("%s: %lld detection rows / %lld ground-truth rows: more than 2^31-1", who, n_rows, n_gt_rows);
        return YK_ERR_ARG;
    }
    if ((unsigned long long)n_img * (unsigned long long)(class_num + 1) > 0xffffffffull) {
        yk_set_error("%s: %d images x %d classes do not fit the 32-bit group key", who, n_img, class_num);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

int check_append(const char *who, const void *src, const void *cnt, long long n_new, const void *rows, const void *img, long long have, long long capacity) {
    if (!src || !cnt || !rows || !img || n_new < 0 || have < 0 || capacity < 0) {
        yk_set_error("%s: bad argument", who);
        return YK_ERR_ARG;
    }
    if (have + n_new > MAP_MAX_ROWS) {
        yk_set_error("%s: %lld + %lld rows: more than 2^31-1", who, have, n_new);
        return YK_ERR_ARG;
    }
    if (have + n_new > capacity) {
        yk_set_error("%s: %lld + %lld rows do not fit the buffer of %lld", who, have, n_new, capacity);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

// the COCO evaluation's workspace: yk_map_eval's (keys, sorts, class offsets) followed by its own
struct CocoWork {
    Work w;
    size_t ign, matched, cum, total;
};

int coco_layout(long long n_rows, long long n_gt_rows, int n_img, int class_num, int nb, CocoWork *cw) {
    const int rc = layout(n_rows, n_gt_rows, n_img, class_num, &cw->w);
    if (rc != YK_OK) return rc;
    const size_t R = (size_t)(n_rows > 0 ? n_rows : 1), G = (size_t)(n_gt_rows > 0 ? n_gt_rows : 1);
    size_t at = cw->w.total;
    cw->ign = at;
    at += up256(G * 8);
    cw->matched = at;
    at += up256(G * 8);
    cw->cum = at;
    at += up256(R * 8 * (size_t)nb);
    cw->total = at;
    return YK_OK;
}

int coco_check(const char *who, long long n_rows, long long n_gt_rows, int n_img, int class_num, int n_thr, int n_area, int n_rec) {
    const int rc = check_sizes(who, n_rows, n_gt_rows, n_img, class_num);
    if (rc != YK_OK) return rc;
    if (n_thr <= 0 || n_area <= 0 || n_rec <= 0) {
        yk_set_error("%s: bad argument", who);
        return YK_ERR_ARG;
    }
    if ((long long)n_thr * n_area > COCO_MAX_BITS) {
        yk_set_error("%s: %d IoU thresholds x %d area ranges: more than %d pairs", who, n_thr, n_area, COCO_MAX_BITS);
        return YK_ERR_ARG;
    }
    if (n_rec > COCO_MAX_REC) {
        yk_set_error("%s: %d recall points: more than %d", who, n_rec, COCO_MAX_REC);
        return YK_ERR_ARG;
    }
    if ((long long)class_num * n_thr * n_area > 0x7fffffffLL) {
        yk_set_error("%s: %d classes x %d pairs: more than 2^31-1 curves", who, class_num, n_thr * n_area);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

}  // namespace

extern "C" int yk_map_append_packed(const float *d_src, const int32_t *d_offsets, int n_img, int img_base, long long n_new, float *d_rows,
                                    int32_t *d_img, long long have, long long capacity, void *stream) {
    const int rc = check_append("yk_map_append_packed", d_src, d_offsets, n_new, d_rows, d_img, have, capacity);
    if (rc != YK_OK) return rc;
    if (n_img <= 0 || img_base < 0) {
        yk_set_error("yk_map_append_packed: bad argument");
        return YK_ERR_ARG;
    }
    if (n_new == 0) return YK_OK;
    hipLaunchKernelGGL(append_packed_kernel, dim3(grid_for(n_new, MAP_BLOCK)), dim3(MAP_BLOCK), 0, (hipStream_t)stream, d_src, d_offsets, n_img, img_base,
                       n_new, d_rows + (size_t)have * 6, d_img + have);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_map_append_padded(const float *d_dets, const int32_t *d_counts, int batch, int cap, int img_base, long long n_new, float *d_rows,
                                    int32_t *d_img, long long have, long long capacity, void *stream) {
    const int rc = check_append("yk_map_append_padded", d_dets, d_counts, n_new, d_rows, d_img, have, capacity);
    if (rc != YK_OK) return rc;
    if (batch <= 0 || cap <= 0 || img_base < 0) {
        yk_set_error("yk_map_append_padded: bad argument");
        return YK_ERR_ARG;
    }
    if (n_new == 0) return YK_OK;
    hipLaunchKernelGGL(append_padded_kernel, dim3(grid_for(batch, 1)), dim3(MAP_BLOCK), 0, (hipStream_t)stream, d_dets, d_counts, batch, cap, img_base,
                       n_new, d_rows + (size_t)have * 6, d_img + have);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_map_workspace_bytes(long long n_rows, long long n_gt_rows, int n_img, int class_num, size_t *bytes) {
    const int rc = check_sizes("yk_map_workspace_bytes", n_rows, n_gt_rows, n_img, class_num);
    if (rc != YK_OK) return rc;
    if (!bytes) {
        yk_set_error("yk_map_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    Work w;
    if (layout(n_rows, n_gt_rows, n_img, class_num, &w) != YK_OK) {
        yk_set_error("yk_map_workspace_bytes: radix sort size query failed");
        return YK_ERR_HIP;
    }
    *bytes = w.total;
    return YK_OK;
}

extern "C" int yk_map_eval(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                           const uint8_t *d_difficult, long long n_gt_rows, int class_num, double iou_thresh, int use_07_metric, int plus_one,
                           void *d_work, size_t work_bytes, uint8_t *d_flags, int32_t *d_n_gt, int32_t *d_n_det, int32_t *d_tp, int32_t *d_fp,
                           double *d_ap, double *d_map, void *stream) {
    const int rc = check_sizes("yk_map_eval", n_rows, n_gt_rows, n_img, class_num);
    if (rc != YK_OK) return rc;
    if (!d_gt_off || !d_work || !d_n_gt || !d_n_det || !d_tp || !d_fp || !d_ap || !d_map || (n_rows > 0 && (!d_rows || !d_img || !d_flags)) ||
        (n_gt_rows > 0 && (!d_gt || !d_difficult)) || !(iou_thresh == iou_thresh)) {
        yk_set_error("yk_map_eval: bad argument");
        return YK_ERR_ARG;
    }
    Work w;
    if (layout(n_rows, n_gt_rows, n_img, class_num, &w) != YK_OK) {
        yk_set_error("yk_map_eval: radix sort size query failed");
        return YK_ERR_HIP;
    }
    if (work_bytes < w.total) {
        yk_set_error("yk_map_eval: workspace of %zu bytes, %zu needed (yk_map_workspace_bytes)", work_bytes, w.total);
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)d_work;
    uint64_t *key_a_in = (uint64_t *)(base + w.key_a_in), *key_a = (uint64_t *)(base + w.key_a);
    uint64_t *key_b_in = (uint64_t *)(base + w.key_b_in), *key_b = (uint64_t *)(base + w.key_b);
    uint32_t *iota = (uint32_t *)(base + w.iota), *row_a = (uint32_t *)(base + w.row_a), *row_b = (uint32_t *)(base + w.row_b);
    uint64_t *cum = (uint64_t *)(base + w.cum);
    uint8_t *taken = (uint8_t *)(base + w.taken);
    int32_t *cls_off = (int32_t *)(base + w.cls_off);

    YK_HIP(hipMemsetAsync(d_n_gt, 0, (size_t)class_num * 4, st));
    YK_HIP(hipMemsetAsync(cls_off, 0, (size_t)(class_num + 1) * 4, st));
    if (n_gt_rows > 0) {
        YK_HIP(hipMemsetAsync(taken, 0, (size_t)n_gt_rows, st));
        hipLaunchKernelGGL(gt_count_kernel, dim3(grid_for(n_gt_rows, MAP_BLOCK)), dim3(MAP_BLOCK), 0, st, d_gt, d_difficult, n_gt_rows, class_num, d_n_gt);
    }
    if (n_rows > 0) {
        YK_HIP(hipMemsetAsync(d_flags, 0, (size_t)n_rows, st));   // rows of no class in [0, class_num) stay 0
        hipLaunchKernelGGL(keys_kernel, dim3(grid_for(n_rows, MAP_BLOCK)), dim3(MAP_BLOCK), 0, st, d_rows, d_img, n_rows, class_num, key_a_in, key_b_in, iota);
        YK_HIP(hipGetLastError());
        size_t tmp = w.sort_bytes;
        YK_HIP(rocprim::radix_sort_pairs(base + w.sort_tmp, tmp, key_a_in, key_a, iota, row_a, (size_t)n_rows, 0u, w.bits_a, st));
        tmp = w.sort_bytes;
        YK_HIP(rocprim::radix_sort_pairs(base + w.sort_tmp, tmp, key_b_in, key_b, iota, row_b, (size_t)n_rows, 0u, w.bits_b, st));
        hipLaunchKernelGGL(class_offsets_kernel, dim3((unsigned)(class_num + 1 + 63) / 64), dim3(64), 0, st, key_a, n_rows, class_num, cls_off);
        if (n_img > 0)
            hipLaunchKernelGGL(match_kernel, dim3(grid_for((long long)n_img * class_num, MAP_WAVES)), dim3(MAP_BLOCK), 0, st, d_rows, key_b, row_b, n_rows, n_img,
                               class_num, d_gt, d_gt_off, d_difficult, taken, iou_thresh, plus_one ? 1.0 : 0.0, d_flags);
    }
    hipLaunchKernelGGL(ap_kernel, dim3((unsigned)class_num), dim3(MAP_BLOCK), 0, st, row_a, cls_off, d_flags, d_n_gt, use_07_metric ? 1 : 0, cum, d_n_det,
                       d_tp, d_fp, d_ap);
    hipLaunchKernelGGL(map_mean_kernel, dim3(1), dim3(1), 0, st, d_ap, class_num, d_map);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_map_coco_workspace_bytes(long long n_rows, long long n_gt_rows, int n_img, int class_num, int n_thr, int n_area, int n_rec,
                                           size_t *bytes) {
    const int rc = coco_check("yk_map_coco_workspace_bytes", n_rows, n_gt_rows, n_img, class_num, n_thr, n_area, n_rec);
    if (rc != YK_OK) return rc;
    if (!bytes) {
        yk_set_error("yk_map_coco_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    CocoWork cw;
    if (coco_layout(n_rows, n_gt_rows, n_img, class_num, n_thr * n_area, &cw) != YK_OK) {
        yk_set_error("yk_map_coco_workspace_bytes: radix sort size query failed");
        return YK_ERR_HIP;
    }
    *bytes = cw.total;
    return YK_OK;
}

extern "C" int yk_map_coco_eval(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                                const uint8_t *d_difficult, long long n_gt_rows, int class_num, const double *d_iou_thr, int n_thr,
                                const double *d_area, int n_area, const double *d_rec_thr, int n_rec, int max_dets, void *d_work, size_t work_bytes,
                                uint8_t *d_flags, int32_t *d_npig, int32_t *d_n_det, double *d_precision, double *d_recall, double *d_summary,
                                double *d_ap_class, void *stream) {
    const int rc = coco_check("yk_map_coco_eval", n_rows, n_gt_rows, n_img, class_num, n_thr, n_area, n_rec);
    if (rc != YK_OK) return rc;
    if (!d_gt_off || !d_work || !d_iou_thr || !d_area || !d_rec_thr || !d_npig || !d_n_det || !d_precision || !d_recall || !d_summary || !d_ap_class ||
        max_dets < 0 || (n_rows > 0 && (!d_rows || !d_img || !d_flags)) || (n_gt_rows > 0 && (!d_gt || !d_difficult))) {
        yk_set_error("yk_map_coco_eval: bad argument");
        return YK_ERR_ARG;
    }
    const int nb = n_thr * n_area;
    CocoWork cw;
    if (coco_layout(n_rows, n_gt_rows, n_img, class_num, nb, &cw) != YK_OK) {
        yk_set_error("yk_map_coco_eval: radix sort size query failed");
        return YK_ERR_HIP;
    }
    if (work_bytes < cw.total) {
        yk_set_error("yk_map_coco_eval: workspace of %zu bytes, %zu needed (yk_map_coco_workspace_bytes)", work_bytes, cw.total);
        return YK_ERR_ARG;
    }
    const Work &w = cw.w;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)d_work;
    uint64_t *key_a_in = (uint64_t *)(base + w.key_a_in), *key_a = (uint64_t *)(base + w.key_a);
    uint64_t *key_b_in = (uint64_t *)(base + w.key_b_in), *key_b = (uint64_t *)(base + w.key_b);
    uint32_t *iota = (uint32_t *)(base + w.iota), *row_a = (uint32_t *)(base + w.row_a), *row_b = (uint32_t *)(base + w.row_b);
    int32_t *cls_off = (int32_t *)(base + w.cls_off);
    uint64_t *ign = (uint64_t *)(base + cw.ign), *matched = (uint64_t *)(base + cw.matched), *cum = (uint64_t *)(base + cw.cum);

    YK_HIP(hipMemsetAsync(d_npig, 0, (size_t)class_num * n_area * 4, st));
    YK_HIP(hipMemsetAsync(d_n_det, 0, (size_t)class_num * 4, st));
    YK_HIP(hipMemsetAsync(cls_off, 0, (size_t)(class_num + 1) * 4, st));
    if (n_gt_rows > 0) {
        YK_HIP(hipMemsetAsync(matched, 0, (size_t)n_gt_rows * 8, st));
        hipLaunchKernelGGL(coco_gt_kernel, dim3(grid_for(n_gt_rows, MAP_BLOCK)), dim3(MAP_BLOCK), 0, st, d_gt, d_difficult, n_gt_rows, class_num, d_area,
                           n_thr, n_area, ign, d_npig);
    }
    if (n_rows > 0) {
        YK_HIP(hipMemsetAsync(d_flags, 0, (size_t)n_rows * (size_t)nb, st));   // rows of no class, rows past max_dets: 0 under every pair
        hipLaunchKernelGGL(keys_kernel, dim3(grid_for(n_rows, MAP_BLOCK)), dim3(MAP_BLOCK), 0, st, d_rows, d_img, n_rows, class_num, key_a_in, key_b_in, iota);
        YK_HIP(hipGetLastError());
        size_t tmp = w.sort_bytes;
        YK_HIP(rocprim::radix_sort_pairs(base + w.sort_tmp, tmp, key_a_in, key_a, iota, row_a, (size_t)n_rows, 0u, w.bits_a, st));
        tmp = w.sort_bytes;
        YK_HIP(rocprim::radix_sort_pairs(base + w.sort_tmp, tmp, key_b_in, key_b, iota, row_b, (size_t)n_rows, 0u, w.bits_b, st));
        hipLaunchKernelGGL(class_offsets_kernel, dim3((unsigned)(class_num + 1 + 63) / 64), dim3(64), 0, st, key_a, n_rows, class_num, cls_off);
        if (n_img > 0 && max_dets > 0)
            hipLaunchKernelGGL(coco_match_kernel, dim3(grid_for((long long)n_img * class_num, MAP_WAVES)), dim3(MAP_BLOCK), 0, st, d_rows, key_b, row_b, n_rows,
                               n_img, class_num, d_gt, d_gt_off, ign, matched, d_iou_thr, d_area, n_thr, n_area, max_dets, d_flags, d_n_det);
    }
    hipLaunchKernelGGL(coco_curve_kernel, dim3((unsigned)(class_num * nb)), dim3(MAP_BLOCK), 0, st, row_a, cls_off, d_flags, n_rows, d_npig, d_rec_thr, n_rec,
                       class_num, n_thr, n_area, cum, d_precision, d_recall);
    hipLaunchKernelGGL(coco_summary_kernel, dim3((unsigned)(10 + class_num)), dim3(MAP_BLOCK), 0, st, d_precision, d_recall, d_iou_thr, n_thr, n_rec, class_num,
                       n_area, d_summary, d_ap_class);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---- operating points: the C-ABI ------------------------------------------------------------------------------------------------------
namespace {

int sweep_check(const char *who, long long n_rows, int class_num, int n_thr) {
    const int rc = check_sizes(who, n_rows, 0, 0, class_num);
    if (rc != YK_OK) return rc;
    if (n_thr < 1 || n_thr > SWEEP_MAX_THR) {
        yk_set_error("%s: %d thresholds: outside 1 .. %d", who, n_thr, SWEEP_MAX_THR);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

inline size_t sweep_bytes(int class_num, int n_thr) { return up256((size_t)2 * (size_t)class_num * (size_t)n_thr * 4); }

}  // namespace

extern "C" int yk_map_sweep_workspace_bytes(long long n_rows, int class_num, int n_thr, size_t *bytes) {
    const int rc = sweep_check("yk_map_sweep_workspace_bytes", n_rows, class_num, n_thr);
    if (rc != YK_OK) return rc;
    if (!bytes) {
        yk_set_error("yk_map_sweep_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    *bytes = sweep_bytes(class_num, n_thr);
    return YK_OK;
}

extern "C" int yk_map_sweep(const float *d_rows, const uint8_t *d_flags, long long n_rows, int class_num, const int32_t *d_n_gt, const double *d_thr,
                            int n_thr, void *d_work, size_t work_bytes, int32_t *d_tp, int32_t *d_fp, double *d_precision, double *d_recall,
                            double *d_f1, int32_t *d_best, double *d_mean_f1, int32_t *d_best_all, void *stream) {
    const int rc = sweep_check("yk_map_sweep", n_rows, class_num, n_thr);
    if (rc != YK_OK) return rc;
    if (!d_n_gt || !d_thr || !d_work || !d_tp || !d_fp || !d_precision || !d_recall || !d_f1 || !d_best || !d_mean_f1 || !d_best_all ||
        (n_rows > 0 && (!d_rows || !d_flags))) {
        yk_set_error("yk_map_sweep: bad argument");
        return YK_ERR_ARG;
    }
    if (work_bytes < sweep_bytes(class_num, n_thr)) {
        yk_set_error("yk_map_sweep: workspace of %zu bytes, %zu needed (yk_map_sweep_workspace_bytes)", work_bytes, sweep_bytes(class_num, n_thr));
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int32_t *hist = (int32_t *)d_work;
    YK_HIP(hipMemsetAsync(hist, 0, (size_t)2 * class_num * n_thr * 4, st));
    if (n_rows > 0)
        hipLaunchKernelGGL(sweep_hist_kernel, dim3(grid_for(n_rows, MAP_BLOCK)), dim3(MAP_BLOCK), 0, st, d_rows, d_flags, n_rows, class_num, d_thr, n_thr, hist);
    hipLaunchKernelGGL(sweep_curve_kernel, dim3((unsigned)class_num), dim3(YK_WAVE), 0, st, hist, d_n_gt, class_num, n_thr, d_tp, d_fp, d_precision, d_recall,
                       d_f1, d_best);
    hipLaunchKernelGGL(sweep_mean_kernel, dim3((unsigned)(n_thr + MAP_BLOCK - 1) / MAP_BLOCK), dim3(MAP_BLOCK), 0, st, d_f1, d_n_gt, class_num, n_thr, d_mean_f1);
    hipLaunchKernelGGL(sweep_best_all_kernel, dim3(1), dim3(YK_WAVE), 0, st, d_mean_f1, n_thr, d_best_all);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_map_confusion_lds_boxes(void) { return CONF_LDS; }

extern "C" int yk_map_confusion_workspace_bytes(long long n_gt_rows, size_t *bytes) {
    if (n_gt_rows < 0 || n_gt_rows > MAP_MAX_ROWS || !bytes) {
        yk_set_error("yk_map_confusion_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    *bytes = up256((size_t)(n_gt_rows > 0 ? n_gt_rows : 1));
    return YK_OK;
}

extern "C" int yk_map_confusion(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                                const uint8_t *d_difficult, long long n_gt_rows, int class_num, double conf_thresh, double iou_thresh, int plus_one,
                                void *d_work, size_t work_bytes, int32_t *d_matrix, int32_t *d_match, void *stream) {
    const int rc = check_sizes("yk_map_confusion", n_rows, n_gt_rows, n_img, class_num);
    if (rc != YK_OK) return rc;
    if (!d_gt_off || !d_work || !d_matrix || (n_rows > 0 && (!d_rows || !d_img || !d_match)) || (n_gt_rows > 0 && (!d_gt || !d_difficult)) ||
        !(iou_thresh == iou_thresh) || !(conf_thresh == conf_thresh)) {
        yk_set_error("yk_map_confusion: bad argument");
        return YK_ERR_ARG;
    }
    if ((long long)(class_num + 1) * (class_num + 1) > 0x7fffffffLL / 4) {
        yk_set_error("yk_map_confusion: a matrix of %d x %d classes is too large", class_num + 1, class_num + 1);
        return YK_ERR_ARG;
    }
    if (work_bytes < up256((size_t)(n_gt_rows > 0 ? n_gt_rows : 1))) {
        yk_set_error("yk_map_confusion: workspace of %zu bytes, %zu needed (yk_map_confusion_workspace_bytes)", work_bytes,
                     up256((size_t)(n_gt_rows > 0 ? n_gt_rows : 1)));
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    YK_HIP(hipMemsetAsync(d_matrix, 0, (size_t)(class_num + 1) * (class_num + 1) * 4, st));
    if (n_img > 0)
        hipLaunchKernelGGL(confusion_kernel, dim3(grid_for(n_img, 1)), dim3(YK_WAVE), 0, st, d_rows, d_img, n_rows, n_img, d_gt, d_gt_off, d_difficult, class_num,
                           conf_thresh, iou_thresh, plus_one ? 1.0 : 0.0, (uint8_t *)d_work, d_matrix, d_match);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
