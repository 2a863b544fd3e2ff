// yk_ota.hip — SimOTA dynamic label assignment: the label grids of a batch from its boxes AND the step's own predictions
// (k210_yolo_framework_amd/simota.py is the rule; include/yolo_hip.h).
//
// Everything that decides - eligibility, IoU, cost, the dynamic k, every comparison - is float64 in the rule's operation order with
// contraction off.  No floating-point atomics; the integer min atomics and the one integer add do not depend on arrival order, so two calls
// give the same bytes.  Four launches on the caller's stream, no memset node and no synchronisation:
//   ota_clear    zeroes the grids (16 bytes per lane where the address allows) and sets the status word to INT32_MAX.
//   ota_prep     grid (tiles of TC candidates, images).  Per candidate the six doubles (bx, by, bw, bh, s(to), Z_j) into the workspace.
//                The expensive part, -L0(q_k) of every (candidate, class), runs one PAIR per lane - consecutive lanes read consecutive class
//                logits of a row, so the 25- or 85-float rows are read coalesced without being aligned - into an LDS table of TC x C doubles;
//                then one lane per candidate adds its row of the table with k ascending (the rule's order; the row stride C is what it is,
//                odd for 1, 3 ... classes and conflict-free then).
//   ota_select   one workgroup per (image, box).  The image's candidates are streamed once for eligibility and IoU and once more for the
//                cost; both passes leave a 64-bit key per candidate in ONE strip of 8 bytes per candidate - in LDS up to YK_OTA_LDS_CANDS
//                candidates, past that the same code on a workspace strip.  The key is the sign-corrected integer image of the double
//                (negative values order correctly: a cost can be about -1e-8), inverted for the IoUs so that both searches are an arg-min
//                with ties to the lower j.  A lane owns the strip entries j = lane mod 256 and keeps the best of them in registers; a round
//                is a shuffle reduction of (key, j) inside each wave, one exchange of the four wave results through LDS (double-buffered:
//                one barrier per round), and a rescan by the ONE lane whose entry was taken.  min(topk, E) rounds give S, k_g rounds give
//                the box's candidates, written with their keys to the workspace.
//   ota_write    one workgroup per image.  Owners by integer atomicMin on the cost key per contested candidate, then on g among the
//                boxes that hold that key; the winners write their slots (no two share one) and the count goes to d_npos.
// There is no contraction in this problem once Z_j is factored out of the class cost, so no matrix instruction is used.
// Nothing is trusted: an image's rows are max(d_first[s], 0) .. min(d_first[s + 1], n_boxes) - 1, none where that is empty (a descending pair, a
// start past the end), an invalid box writes nothing, every candidate index comes from a loop bound.  x y w h are clipped with fmax / fmin:
// a NaN width or height becomes 1e-8 (validity looks at the class and the centre only), as simota.py states it.
#include "yk_common.h"

#pragma clang fp contract(off)

#define YK_OTA_THREADS 256
#define YK_OTA_WAVES (YK_OTA_THREADS / YK_WAVE)
#define YK_OTA_PREP_DOUBLES 6000      /* LDS of ota_prep: TC * (C + 1) doubles */
#define YK_OTA_NONE 0xffffffffffffffffull

namespace {

typedef unsigned long long u64;

struct ota_args {
    yk_ota_cfg_t cfg;
    const float *pred[YK_MAX_LAYERS];
    int cand0[YK_MAX_LAYERS + 1];     // the first candidate of layer l in an image's flat order; cand0[n_layers] = N
    size_t per[YK_MAX_LAYERS];        // floats of one image in layer l
    size_t base[YK_MAX_LAYERS];       // floats of d_labels before layer l
    int N, E, max_boxes, tc;
    double *cand;                     // [n][N][6]
    u64 *strip;                       // [n][max_boxes][N], only where N > YK_OTA_LDS_CANDS
    u64 *okey;                        // [n][N]
    u64 *sel_key;                     // [n][max_boxes][YK_OTA_MAX_TOPK]
    int *sel_j;                       // [n][max_boxes][YK_OTA_MAX_TOPK]
    int *sel_cnt;                     // [n][max_boxes]
    int *og;                          // [n][N]
};

struct ota_layout {
    size_t cand, strip, okey, sel_key, sel_j, sel_cnt, og, total;
    int N;
};

__device__ __forceinline__ double ota_sig(double v) { return 1.0 / (1.0 + exp(-v)); }
__device__ __forceinline__ double ota_l0(double q) { return fmax(log1p(-q), -100.0); }
__device__ __forceinline__ double ota_l1(double q) { return fmax(log(q), -100.0); }

// ascending unsigned order of the doubles, -0 as +0
__device__ __forceinline__ u64 ota_key(double v) {
    const u64 u = (u64)__double_as_longlong(v + 0.0);
    return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double ota_unkey(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// j of an image -> its layer and the row of d_pred[layer] it is (in floats)
__device__ __forceinline__ int ota_layer(const ota_args &a, int j) {
    int l = 0;
    while (l + 1 < a.cfg.n_layers && j >= a.cand0[l + 1]) ++l;
    return l;
}
__device__ __forceinline__ const float *ota_row(const ota_args &a, size_t image, int l, int j) {
    return a.pred[l] + (image * (size_t)(a.cand0[l + 1] - a.cand0[l]) + (size_t)(j - a.cand0[l])) * (size_t)a.E;
}

__global__ void __launch_bounds__(YK_OTA_THREADS) ota_clear(float *__restrict__ labels, size_t count, int32_t *__restrict__ status) {
    const size_t tid = (size_t)blockIdx.x * YK_OTA_THREADS + threadIdx.x, step = (size_t)gridDim.x * YK_OTA_THREADS;
    if (tid == 0) *status = 0x7fffffff;
    size_t head = ((16 - ((uintptr_t)labels & 15)) & 15) / 4;
    head = head < count ? head : count;
    const size_t vecs = (count - head) / 4, done = head + 4 * vecs;
    if (tid < head) labels[tid] = 0.f;
    float4 *l4 = reinterpret_cast<float4 *>(labels + head);
    for (size_t i = tid; i < vecs; i += step) l4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < count - done) labels[done + tid] = 0.f;
}

__global__ void __launch_bounds__(YK_OTA_THREADS) ota_prep(const ota_args a) {
    extern __shared__ double s_prep[];                      // [tc] s(to), then [tc][C] the terms
    const int tid = threadIdx.x, C = a.cfg.class_num, tc = a.tc;
    const size_t image = blockIdx.y;
    const int j0 = (int)blockIdx.x * tc;
    const int here = a.N - j0 < tc ? a.N - j0 : tc;
    double *s_so = s_prep, *s_term = s_prep + tc;
    double bx = 0, by = 0, bw = 0, bh = 0;
    if (tid < here) {
        const int j = j0 + tid, l = ota_layer(a, j);
        const float *row = ota_row(a, image, l, j);
        const int A = a.cfg.anchor_num[l], W = a.cfg.out_w[l], H = a.cfg.out_h[l];
        const int jl = j - a.cand0[l], cell = jl / A, q = jl - cell * A;
        bx = (ota_sig((double)row[0]) + (double)(cell % W)) / (double)W;
        by = (ota_sig((double)row[1]) + (double)(cell / W)) / (double)H;
        bw = exp((double)row[2]) * a.cfg.anchors[l][q][0];
        bh = exp((double)row[3]) * a.cfg.anchors[l][q][1];
        s_so[tid] = ota_sig((double)row[4]);
    }
    __syncthreads();
    for (int p = tid; p < here * C; p += YK_OTA_THREADS) {
        const int cl = p / C, k = p - cl * C, j = j0 + cl;
        const float *row = ota_row(a, image, ota_layer(a, j), j);
        s_term[p] = -ota_l0(sqrt(ota_sig((double)row[5 + k]) * s_so[cl]));
    }
    __syncthreads();
    if (tid < here) {
        double z = 0.0;
        for (int k = 0; k < C; ++k) z = z + s_term[tid * C + k];
        double *o = a.cand + (image * (size_t)a.N + (size_t)(j0 + tid)) * 6;
        o[0] = bx, o[1] = by, o[2] = bw, o[3] = bh, o[4] = s_so[tid], o[5] = z;
    }
}

struct ota_box {
    double x, y, w, h;
    int c;
};

// a box row -> valid?  (yk_boxes_to_labels_f32's test, in every layer)
__device__ __forceinline__ bool ota_load_box(const ota_args &a, const double *row, ota_box &b) {
    const double c = row[0], x = row[1], y = row[2];
    bool ok = c > -1.0 && c < (double)a.cfg.class_num;
    for (int l = 0; l < a.cfg.n_layers; ++l) {
        const double cx = floor(x * (double)a.cfg.out_w[l]), cy = floor(y * (double)a.cfg.out_h[l]);
        ok = ok && cx >= 0.0 && cx < (double)a.cfg.out_w[l] && cy >= 0.0 && cy < (double)a.cfg.out_h[l];      // (false for a NaN or an infinity)
    }
    b.x = fmin(fmax(x, 1e-8), 1.0), b.y = fmin(fmax(y, 1e-8), 1.0), b.w = fmin(fmax(row[3], 1e-8), 1.0), b.h = fmin(fmax(row[4], 1e-8), 1.0);
    b.c = ok ? (int)c : 0;
    return ok;
}

// eligibility and IoU of (box, candidate j); with_cost: also the cost.  The rule's expressions in its order.
__device__ __forceinline__ bool ota_pair(const ota_args &a, const ota_box &b, size_t image, int j, bool with_cost, double &iou, double &cost) {
    const int l = ota_layer(a, j), A = a.cfg.anchor_num[l], W = a.cfg.out_w[l], H = a.cfg.out_h[l];
    const int cell = (j - a.cand0[l]) / A;
    const double px = ((double)(cell % W) + 0.5) / (double)W, py = ((double)(cell / W) + 0.5) / (double)H;
    const double dx = fabs(px - b.x), dy = fabs(py - b.y);
    const bool in_box = dx < b.w / 2 && dy < b.h / 2, in_ctr = dx < a.cfg.radius / (double)W && dy < a.cfg.radius / (double)H;
    if (!(in_box || in_ctr)) return false;
    const double *cd = a.cand + (image * (size_t)a.N + (size_t)j) * 6;
    const double bx = cd[0], by = cd[1], bw = cd[2], bh = cd[3];
    const double ow = fmax(fmin(b.x + b.w / 2, bx + bw / 2) - fmax(b.x - b.w / 2, bx - bw / 2), 0.0);
    const double oh = fmax(fmin(b.y + b.h / 2, by + bh / 2) - fmax(b.y - b.h / 2, by - bh / 2), 0.0);
    const double I = ow * oh, U = (b.w * b.h + bw * bh) - I;
    iou = (U > 0.0 && U < __builtin_huge_val()) ? I / U : 0.0;
    if (with_cost) {
        const double q = sqrt(ota_sig((double)ota_row(a, image, l, j)[5 + b.c]) * cd[4]);
        cost = ((cd[5] + ota_l0(q)) - ota_l1(q)) + a.cfg.iou_weight * (-log(iou + 1e-8));
        cost = cost + (in_box && in_ctr ? 0.0 : 1e5);
    }
    return true;
}

// the smallest key among a lane's own strip entries (j = tid mod YK_OTA_THREADS), ties to the lower j
__device__ __forceinline__ void ota_scan(const u64 *strip, int N, int tid, u64 &lk, int &lj) {
    lk = YK_OTA_NONE, lj = 0x7fffffff;
    for (int i = tid; i < N; i += YK_OTA_THREADS) {
        const u64 k = strip[i];
        if (k < lk) lk = k, lj = i;
    }
}

// one round: the workgroup's smallest (key, j); every lane returns it.  `buf` alternates between rounds.
__device__ __forceinline__ void ota_round(u64 lk, int lj, u64 (*s_k)[YK_OTA_WAVES], int (*s_j)[YK_OTA_WAVES], int buf, u64 &wk, int &wj) {
#pragma unroll
    for (int o = YK_WAVE / 2; o > 0; o >>= 1) {
        const u64 ok = __shfl_xor(lk, o, YK_WAVE);
        const int oj = __shfl_xor(lj, o, YK_WAVE);
        if (ok < lk || (ok == lk && oj < lj)) lk = ok, lj = oj;
    }
    if ((threadIdx.x & (YK_WAVE - 1)) == 0) s_k[buf][threadIdx.x / YK_WAVE] = lk, s_j[buf][threadIdx.x / YK_WAVE] = lj;
    __syncthreads();
    wk = s_k[buf][0], wj = s_j[buf][0];
#pragma unroll
    for (int w = 1; w < YK_OTA_WAVES; ++w) {
        const u64 ok = s_k[buf][w];
        const int oj = s_j[buf][w];
        if (ok < wk || (ok == wk && oj < wj)) wk = ok, wj = oj;
    }
}

__global__ void __launch_bounds__(YK_OTA_THREADS) ota_select(const ota_args a, const double *__restrict__ boxes, int n_boxes,
                                                             const int32_t *__restrict__ first, int32_t *__restrict__ status) {
    __shared__ u64 s_strip[YK_OTA_LDS_CANDS];
    __shared__ u64 s_k[2][YK_OTA_WAVES];
    __shared__ int s_j[2][YK_OTA_WAVES];
    __shared__ int s_elig;
    const int tid = threadIdx.x, g = blockIdx.x, N = a.N;
    const size_t image = blockIdx.y;
    const size_t slot = image * (size_t)a.max_boxes + (size_t)g;
    int b0 = first[image], b1 = first[image + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > n_boxes ? n_boxes : b1;
    const int m = b1 > b0 ? b1 - b0 : 0;
    if (g == 0 && tid == 0 && m > a.max_boxes) atomicMin(status, b0 + a.max_boxes);
    ota_box b;
    const bool ok = g < m && ota_load_box(a, boxes + (size_t)(b0 + g) * 5, b);     // (uniform over the workgroup)
    if (!ok) {
        if (tid == 0) {
            a.sel_cnt[slot] = 0;
            if (g < m) atomicMin(status, b0 + g);
        }
        return;
    }
    u64 *strip = N <= YK_OTA_LDS_CANDS ? s_strip : a.strip + slot * (size_t)N;
    if (tid == 0) s_elig = 0;
    __syncthreads();
    // pass 1: inverted IoU keys of the eligible candidates
    int mine = 0;
    for (int i = tid; i < N; i += YK_OTA_THREADS) {
        double iou = 0.0, cost = 0.0;
        const bool el = ota_pair(a, b, image, i, false, iou, cost);
        strip[i] = el ? ~ota_key(iou) : YK_OTA_NONE;
        mine += el ? 1 : 0;
    }
    if (mine) atomicAdd(&s_elig, mine);
    u64 lk, wk;
    int lj, wj, buf = 0;
    ota_scan(strip, N, tid, lk, lj);
    double S = 0.0;
    for (int r = 0; r < a.cfg.topk; ++r, buf ^= 1) {
        ota_round(lk, lj, s_k, s_j, buf, wk, wj);
        if (wk == YK_OTA_NONE) break;
        S = S + ota_unkey(~wk);                                                     // from the largest down; the same in every lane
        if (wj % YK_OTA_THREADS == tid) {
            strip[wj] = YK_OTA_NONE;
            ota_scan(strip, N, tid, lk, lj);
        }
    }
    __syncthreads();                                                                // s_elig is complete (and every lane is past the rounds' buffers)
    int k = (int)floor(S);
    k = k < 1 ? 1 : k;
    k = k > s_elig ? s_elig : k;
    k = k > YK_OTA_MAX_TOPK ? YK_OTA_MAX_TOPK : k;                                  // (S <= topk; this is for the selection table's sake)
    // pass 2: cost keys
    for (int i = tid; i < N; i += YK_OTA_THREADS) {
        double iou = 0.0, cost = 0.0;
        const bool el = ota_pair(a, b, image, i, true, iou, cost);
        strip[i] = el ? ota_key(cost) : YK_OTA_NONE;
    }
    ota_scan(strip, N, tid, lk, lj);
    int taken = 0;
    for (buf = 0; taken < k; ++taken, buf ^= 1) {
        ota_round(lk, lj, s_k, s_j, buf, wk, wj);
        if (wk == YK_OTA_NONE) break;
        if (tid == 0) a.sel_key[slot * YK_OTA_MAX_TOPK + taken] = wk, a.sel_j[slot * YK_OTA_MAX_TOPK + taken] = wj;
        if (wj % YK_OTA_THREADS == tid) {
            strip[wj] = YK_OTA_NONE;
            ota_scan(strip, N, tid, lk, lj);
        }
    }
    if (tid == 0) a.sel_cnt[slot] = taken;
}

__global__ void __launch_bounds__(YK_OTA_THREADS) ota_write(const ota_args a, const double *__restrict__ boxes, int n_boxes,
                                                            const int32_t *__restrict__ first, float *__restrict__ labels,
                                                            int32_t *__restrict__ npos) {
    __shared__ int s_pos;
    const int tid = threadIdx.x;
    const size_t image = blockIdx.x;
    int b0 = first[image], b1 = first[image + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > n_boxes ? n_boxes : b1;
    int m = b1 > b0 ? b1 - b0 : 0;
    m = m > a.max_boxes ? a.max_boxes : m;
    const int entries = m * YK_OTA_MAX_TOPK;
    u64 *okey = a.okey + image * (size_t)a.N;
    int *og = a.og + image * (size_t)a.N;
    const size_t sel0 = image * (size_t)a.max_boxes;
    if (tid == 0) s_pos = 0;
    for (int phase = 0; phase < 4; ++phase) {
        for (int e = tid; e < entries; e += YK_OTA_THREADS) {
            const int g = e / YK_OTA_MAX_TOPK, r = e - g * YK_OTA_MAX_TOPK;
            if (r >= a.sel_cnt[sel0 + g]) continue;
            const int j = a.sel_j[(sel0 + g) * YK_OTA_MAX_TOPK + r];
            if (j < 0 || j >= a.N) continue;                                        // (cannot be: ota_select wrote it from a loop bound)
            const u64 key = a.sel_key[(sel0 + g) * YK_OTA_MAX_TOPK + r];
            if (phase == 0) {
                okey[j] = YK_OTA_NONE, og[j] = 0x7fffffff;                          // (every writer writes the same)
            } else if (phase == 1) {
                atomicMin(&okey[j], key);
            } else if (__hip_atomic_load(&okey[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key) {
                if (phase == 2) {
                    atomicMin(&og[j], g);
                } else if (__hip_atomic_load(&og[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) {
                    ota_box b;
                    ota_load_box(a, boxes + (size_t)(b0 + g) * 5, b);              // valid: it selected
                    const int l = ota_layer(a, j);
                    float *o = labels + a.base[l] + image * a.per[l] + (size_t)(j - a.cand0[l]) * (size_t)a.E;
                    o[0] = (float)b.x, o[1] = (float)b.y, o[2] = (float)b.w, o[3] = (float)b.h, o[4] = 1.f;
                    o[5 + b.c] = 1.f;
                    atomicAdd(&s_pos, 1);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) npos[image] = s_pos;
}

// sizes and argument checks that need no device; nullptr, or the message's tail
const char *ota_plan(const yk_ota_cfg_t *cfg, int n, int max_boxes, ota_layout &lay) {
    static thread_local char msg[160];
    if (!cfg) return "cfg is NULL";
    if (n < 0 || n > 65535) {
        snprintf(msg, sizeof msg, "n = %d: must be in 0 .. 65535", n);
        return msg;
    }
    if (max_boxes < 1 || max_boxes > YK_OTA_MAX_BOXES) {
        snprintf(msg, sizeof msg, "max_boxes = %d: must be in 1 .. %d", max_boxes, YK_OTA_MAX_BOXES);
        return msg;
    }
    if (cfg->n_layers < 1 || cfg->n_layers > YK_MAX_LAYERS) {
        snprintf(msg, sizeof msg, "cfg->n_layers = %d: must be in 1 .. %d", cfg->n_layers, YK_MAX_LAYERS);
        return msg;
    }
    if (cfg->class_num < 1 || cfg->class_num > YK_OTA_MAX_CLASSES) {
        snprintf(msg, sizeof msg, "cfg->class_num = %d: must be in 1 .. %d", cfg->class_num, YK_OTA_MAX_CLASSES);
        return msg;
    }
    if (cfg->topk < 1 || cfg->topk > YK_OTA_MAX_TOPK) {
        snprintf(msg, sizeof msg, "cfg->topk = %d: must be in 1 .. %d", cfg->topk, YK_OTA_MAX_TOPK);
        return msg;
    }
    if (!(cfg->radius >= 1.0 && cfg->radius <= 16.0)) {
        snprintf(msg, sizeof msg, "cfg->radius = %g: must be in 1 .. 16", cfg->radius);
        return msg;
    }
    if (!(cfg->iou_weight > 0.0 && cfg->iou_weight < __builtin_huge_val())) {
        snprintf(msg, sizeof msg, "cfg->iou_weight = %g: must be positive and finite", cfg->iou_weight);
        return msg;
    }
    unsigned long long N = 0;
    for (int l = 0; l < cfg->n_layers; ++l) {
        if (cfg->anchor_num[l] < 1 || cfg->anchor_num[l] > YK_MAX_ANCHORS) {
            snprintf(msg, sizeof msg, "cfg->anchor_num[%d] = %d: must be in 1 .. %d", l, cfg->anchor_num[l], YK_MAX_ANCHORS);
            return msg;
        }
        if (cfg->out_h[l] <= 0 || cfg->out_w[l] <= 0) {
            snprintf(msg, sizeof msg, "cfg->out_h[%d] x cfg->out_w[%d] = %d x %d", l, l, cfg->out_h[l], cfg->out_w[l]);
            return msg;
        }
        N += (unsigned long long)cfg->out_h[l] * (unsigned long long)cfg->out_w[l] * (unsigned)cfg->anchor_num[l];
        if (N > (1ull << 24)) {
            snprintf(msg, sizeof msg, "more than 2^24 candidates per image (layers 0 .. %d)", l);
            return msg;
        }
    }
    // n <= 2^16, N <= 2^24, max_boxes <= 2^8, 5 + C <= 2^13: every product below is under 2^62
    const size_t nn = (size_t)n, NN = (size_t)N, mb = (size_t)max_boxes;
    size_t at = 0;
    lay.N = (int)N;
    lay.cand = at, at += nn * NN * 6 * sizeof(double);
    lay.strip = at, at += N > YK_OTA_LDS_CANDS ? nn * mb * NN * sizeof(u64) : 0;
    lay.okey = at, at += nn * NN * sizeof(u64);
    lay.sel_key = at, at += nn * mb * YK_OTA_MAX_TOPK * sizeof(u64);
    lay.sel_j = at, at += nn * mb * YK_OTA_MAX_TOPK * sizeof(int);
    lay.sel_cnt = at, at += nn * mb * sizeof(int);
    lay.og = at, at += nn * NN * sizeof(int);
    lay.total = (at + 7) & ~(size_t)7;
    return nullptr;
}

}  // namespace

extern "C" int yk_simota_workspace_bytes(const yk_ota_cfg_t *cfg, int n, int max_boxes, size_t *bytes) {
    const char *who = "yk_simota_workspace_bytes";
    ota_layout lay;
    if (!bytes) {
        yk_set_error("%s: bytes is NULL", who);
        return YK_ERR_ARG;
    }
    if (const char *bad = ota_plan(cfg, n, max_boxes, lay)) {
        yk_set_error("%s: %s", who, bad);
        return YK_ERR_ARG;
    }
    *bytes = lay.total;
    return YK_OK;
}

extern "C" int yk_assign_simota_f32(const yk_ota_cfg_t *cfg, const double *d_boxes, int n_boxes, const int32_t *d_first, int n,
                                    const float *const *d_pred, float *d_labels, int32_t *d_npos, int32_t *d_status, void *d_work,
                                    size_t work_bytes, void *stream) {
    const char *who = "yk_assign_simota_f32";
    ota_layout lay;
    if (const char *bad = ota_plan(cfg, n, cfg ? cfg->max_boxes : 1, lay)) {
        yk_set_error("%s: %s%s", who, cfg && (cfg->max_boxes < 1 || cfg->max_boxes > YK_OTA_MAX_BOXES) ? "cfg->" : "", bad);
        return YK_ERR_ARG;
    }
    if (n == 0) return YK_OK;
    if (n_boxes < 0 || n_boxes >= (1 << 30)) {
        yk_set_error("%s: n_boxes = %d: must be in 0 .. 2^30 - 1", who, n_boxes);
        return YK_ERR_ARG;
    }
    const char *null = !d_first ? "d_first" : !d_pred ? "d_pred" : !d_labels ? "d_labels" : !d_npos ? "d_npos" : !d_status ? "d_status"
                       : !d_work ? "d_work" : n_boxes > 0 && !d_boxes ? "d_boxes" : nullptr;
    if (null) {
        yk_set_error("%s: %s is NULL", who, null);
        return YK_ERR_ARG;
    }
    for (int l = 0; l < cfg->n_layers; ++l)
        if (!d_pred[l] || ((uintptr_t)d_pred[l] & 3)) {
            yk_set_error("%s: d_pred[%d] is %s", who, l, d_pred[l] ? "misaligned" : "NULL");
            return YK_ERR_ARG;
        }
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_boxes & 7) || ((uintptr_t)d_first & 3) || ((uintptr_t)d_status & 3) || ((uintptr_t)d_npos & 3) ||
        ((uintptr_t)d_work & 7)) {
        yk_set_error("%s: a misaligned pointer", who);
        return YK_ERR_ARG;
    }
    if (work_bytes < lay.total) {
        yk_set_error("%s: work_bytes = %zu: yk_simota_workspace_bytes asks for %zu", who, work_bytes, lay.total);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("%s: no HIP device", who);
        return YK_ERR_NO_DEVICE;
    }
    ota_args a;
    memset(&a, 0, sizeof(a));
    a.cfg = *cfg;
    a.N = lay.N, a.E = 5 + cfg->class_num, a.max_boxes = cfg->max_boxes;
    size_t before = 0;
    for (int l = 0; l < cfg->n_layers; ++l) {
        a.pred[l] = d_pred[l];
        a.cand0[l + 1] = a.cand0[l] + cfg->out_h[l] * cfg->out_w[l] * cfg->anchor_num[l];
        a.per[l] = (size_t)(a.cand0[l + 1] - a.cand0[l]) * (size_t)a.E;
        a.base[l] = before * (size_t)n;
        before += a.per[l];
    }
    for (int l = cfg->n_layers; l < YK_MAX_LAYERS; ++l) a.cand0[l + 1] = a.cand0[l];
    const int tc_fit = YK_OTA_PREP_DOUBLES / (cfg->class_num + 1);
    a.tc = tc_fit < YK_OTA_THREADS ? tc_fit : YK_OTA_THREADS;                       // >= 1: class_num <= YK_OTA_MAX_CLASSES
    char *w = (char *)d_work;
    a.cand = (double *)(w + lay.cand), a.strip = (u64 *)(w + lay.strip), a.okey = (u64 *)(w + lay.okey), a.sel_key = (u64 *)(w + lay.sel_key);
    a.sel_j = (int *)(w + lay.sel_j), a.sel_cnt = (int *)(w + lay.sel_cnt), a.og = (int *)(w + lay.og);
    hipStream_t st = (hipStream_t)stream;
    const size_t count = before * (size_t)n;
    const size_t want = (count / 4 + YK_OTA_THREADS - 1) / YK_OTA_THREADS + 1;
    hipLaunchKernelGGL(ota_clear, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(YK_OTA_THREADS), 0, st, d_labels, count, d_status);
    hipLaunchKernelGGL(ota_prep, dim3((unsigned)((a.N + a.tc - 1) / a.tc), (unsigned)n), dim3(YK_OTA_THREADS),
                       (size_t)a.tc * (size_t)(cfg->class_num + 1) * sizeof(double), st, a);
    hipLaunchKernelGGL(ota_select, dim3((unsigned)a.max_boxes, (unsigned)n), dim3(YK_OTA_THREADS), 0, st, a, d_boxes, n_boxes, d_first, d_status);
    hipLaunchKernelGGL(ota_write, dim3((unsigned)n), dim3(YK_OTA_THREADS), 0, st, a, d_boxes, n_boxes, d_first, d_labels, d_npos);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
