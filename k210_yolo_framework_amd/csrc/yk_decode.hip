// yk_decode.hip — Python-mode decode + per-class NMS on gfx950 (batched).
//
// Replaces, for a whole batch and without host round trips,
//   keras_inference.py:94-111   sigmoid(cls)*sigmoid(conf), reshape(-1,..) in (layer,h,w,anchor) order
//   tools/utils.py:545-546      tf_xywh_to_all
//   keras_inference.py:51-72    correct_box
//   keras_inference.py:113-135  scores >= obj_thresh ; per class tf.image.non_max_suppression(…, 30, iou)
// which the reference runs as ~100 eager TF op dispatches per image.
//
// Three launches: decode (thread per box, coalesced class-major score planes) -> NMS (one
// wavefront per (image, class), yk_nms.h) -> compaction to the reference's class-major row order.
// Compiled with -ffp-contract=off: one rounding per TF op, like the eager fp32 graph.
#include <cstddef>
#include "yk_common.h"
#include "yk_nms.h"

struct decode_args {
    int L, A, C, E;
    int in_h, in_w;
    int out_h[YK_MAX_LAYERS], out_w[YK_MAX_LAYERS];
    int off[YK_MAX_LAYERS + 1];   // first global box index of each layer
    float anchors[YK_MAX_LAYERS][YK_MAX_ANCHORS][2];
    const float *pred[YK_MAX_LAYERS];
};

__device__ __forceinline__ float tf_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

__global__ void __launch_bounds__(256) decode_py_kernel(decode_args a, int batch, const float *__restrict__ image_hw,
                                                        float4 *__restrict__ boxes, float *__restrict__ scores_t) {
    const int ntot = a.off[a.L];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= batch * ntot) return;
    const int b = t / ntot, g = t - b * ntot;
    int l = 0;
    while (l + 1 < a.L && g >= a.off[l + 1]) ++l;
    const int r = g - a.off[l];
    const int cell = r / a.A, an = r - cell * a.A;
    const int h = a.out_h[l], w = a.out_w[l];
    const int row = cell / w, col = cell - row * w;
    const float *p = a.pred[l] + ((size_t)(b * h + row) * w + col) * a.A * a.E + (size_t)an * a.E;

    const float conf = tf_sigmoid(p[4]);
    for (int c = 0; c < a.C; ++c) scores_t[((size_t)b * a.C + c) * ntot + g] = tf_sigmoid(p[5 + c]) * conf;

    // tf_xywh_to_all (tools/utils.py:545-546)
    const float x = (tf_sigmoid(p[0]) + (float)col) / (float)w;
    const float y = (tf_sigmoid(p[1]) + (float)row) / (float)h;
    const float bw = expf(p[2]) * a.anchors[l][an][0];
    const float bh = expf(p[3]) * a.anchors[l][an][1];

    // correct_box (keras_inference.py:51-72), (y,x) order
    const float in_h = (float)a.in_h, in_w = (float)a.in_w;
    const float im_h = image_hw ? image_hw[2 * b] : in_h, im_w = image_hw ? image_hw[2 * b + 1] : in_w;
    const float rh = in_h / im_h, rw = in_w / im_w;
    const float m = rh < rw ? rh : rw;
    const float new_h = rintf(im_h * m), new_w = rintf(im_w * m);       // tf.round = half-to-even
    const float off_y = (in_h - new_h) / 2.f / in_h, off_x = (in_w - new_w) / 2.f / in_w;
    const float sc_y = in_h / new_h, sc_x = in_w / new_w;
    const float cy = (y - off_y) * sc_y, cx = (x - off_x) * sc_x;
    const float hh = bh * sc_y, ww = bw * sc_x;
    const float hy = hh / 2.f, hx = ww / 2.f;
    boxes[(size_t)b * ntot + g] = make_float4((cy - hy) * im_h, (cx - hx) * im_w, (cy + hy) * im_h, (cx + hx) * im_w);
}

// ---- The candidates of one (image, class) in LDS.  MAXC: LDS capacity in candidates.  1 088 (26 KB) covers the 224x320 heads (1 050 boxes)
// and leaves the CU's LDS to the conv kernels of other batches in flight; 2 048 (48 KB) otherwise.  nms_maxc() is the one place that picks it.
template <int MAXC>
struct nms_lds {
    float s[MAXC];
    int idx[MAXC];
    float4 box[MAXC];
};
// (host only; nms_path() in tests/nms_cases.py carries a copy of this line.  From outside the choice shows in the kernel's name in a trace.)
static int nms_maxc(int ntot) { return ntot <= 1088 ? 1088 : 2048; }

// What one wavefront works on: its class's score plane, its image's boxes, its output slots, and the call's thresholds.  Uniform, by value.
struct nms_job {
    float *sc;
    const float4 *bx;
    int *og;
    float *os;
    int ntot, max_out;
    float obj_thresh, iou_thresh;
};
__device__ __forceinline__ nms_job nms_job_of(int ntot, int C, float obj_thresh, float iou_thresh, int max_out, const float4 *boxes,
                                               float *scores_t, int *sel_g, float *sel_s) {
    const size_t bc = (size_t)blockIdx.y * C + blockIdx.x;
    return {scores_t + bc * ntot, boxes + (size_t)blockIdx.y * ntot, sel_g + bc * max_out, sel_s + bc * max_out, ntot, max_out, obj_thresh, iou_thresh};
}

// The 64-bit key of the fast path's rank sort and of the overflow path: (score bits, ~box index) - scores are >= 0, so the bit pattern
// orders like the float; ties fall to the lower box index
__device__ __forceinline__ unsigned long long key_of(float v, int i) { return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(~i); }

// ---- THE scan: ballot compaction of one class's score plane into L.s / L.idx, in box-index order, 8 independent loads in flight.  A box is
// a candidate when its score is >= obj_thresh (keras_inference.py:116) and take(score, box index) holds; the candidates ranked
// [first, first + MAXC) among them are stored, all are counted.  seen(score) is told every candidate (the initial scan's score range).
// RANKED = false: first is 0 by construction and the lower end of the window is not compiled (the scan as the usual path runs it).
struct take_all {
    __device__ bool operator()(float, int) const { return true; }
};
struct see_none {
    __device__ void operator()(float) const {}
};
template <int MAXC, bool RANKED = false, class Take = take_all, class Seen = see_none>
__device__ __forceinline__ int scan_scores(nms_lds<MAXC> &L, const float *sc, int ntot, float obj_thresh, int first, Take take = Take(),
                                           Seen seen = Seen()) {
    const int lane = threadIdx.x;
    int n = 0;
    for (int base0 = 0; base0 < ntot; base0 += 64 * 8) {
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base0 + u * 64 + lane;
            sv[u] = (i < ntot) ? sc[i] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base0 + u * 64 + lane;
            const bool f = (i < ntot) && (sv[u] >= obj_thresh) && take(sv[u], i);
            const unsigned long long m = __ballot(f);
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull)) - (RANKED ? first : 0);
            if (f && (!RANKED || pos >= 0) && pos < MAXC) {
                L.s[pos] = sv[u];
                L.idx[pos] = i;
            }
            if (f) seen(sv[u]);
            n += __popcll(m);
        }
    }
    return n;
}

// ---- THE fetch: the boxes of the first nc candidates, in bulk AFTER the scan: a load inside the ballot loop above would put one global
// round trip on the critical path per unrolled step (measured: 24 serialised latencies, ~40 us of a 53 us kernel)
template <int MAXC>
__device__ __forceinline__ void fetch_boxes(nms_lds<MAXC> &L, const float4 *bx, int nc) {
    const int lane = threadIdx.x;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * 64 + lane;
            t[u] = bx[c < nc ? L.idx[c] : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * 64 + lane;
            if (c < nc) L.box[c] = t[u];
        }
    }
}

// corners normalised once (tf_iou does it per call; min / max are idempotent, so the other paths are unaffected)
template <int MAXC>
__device__ __forceinline__ void normalise_box(nms_lds<MAXC> &L, int c) {
    const float4 q = L.box[c];
    L.box[c] = make_float4(fminf(q.x, q.z), fminf(q.y, q.w), fmaxf(q.x, q.z), fmaxf(q.y, q.w));
}

// ---- THE sweep.  TF's own formulation: visit the candidates in descending score order and test each against the boxes selected so far.
// The selected boxes live one per lane in registers (max_out <= 64), so a candidate costs one IoU + one ballot: no LDS writes, no barriers.
// The set lives in the kernel and is carried ACROSS calls (the chunks of the tied and overflow paths).
struct kept_set {
    float y0, x0, y1, x1, area;   // this lane's selected box (lane < kept)
    int kept;                     // uniform
};
// iou > thr is decided without the division whenever inter is clearly above / below thr*union (2e-6 guard band, 30x the rounding of the
// quotient); only the band itself takes the exact fp32 division the reference performs
struct iou_gate {
    float thr, hi, lo;
};
__device__ __forceinline__ iou_gate iou_gate_of(float iou_thresh) {
    const bool guard = iou_thresh > 0.f;
    return {iou_thresh, guard ? iou_thresh * (1.f + 2e-6f) : INFINITY, guard ? iou_thresh * (1.f - 2e-6f) : -INFINITY};
}
__device__ __forceinline__ float lane_value(float v, int t) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), t)); }

// A block of up to 64 candidates in registers (lane t holds the t-th best of the block: normalised box, score bits, box index), handed out
// with v_readlane: the serial loop has no dependent LDS read in it
__device__ __forceinline__ void sweep_block(kept_set &K, const iou_gate g, const nms_job J, const float4 bb, int sbits, int iv, int count) {
    const int lane = threadIdx.x;
    const float ar = (bb.z - bb.x) * (bb.w - bb.y);
    // the count is uniform, but behind the struct the compiler takes it for a per-lane value and runs this loop's control through exec masks
    // (measured: +0.9 us on the 20 us fast path): read it into a scalar for the loop
    int kept = __builtin_amdgcn_readfirstlane(K.kept);
    for (int t = 0; t < count && kept < J.max_out; ++t) {
        const float cy0 = lane_value(bb.x, t), cx0 = lane_value(bb.y, t), cy1 = lane_value(bb.z, t), cx1 = lane_value(bb.w, t);
        const float ca = lane_value(ar, t);
        const float inter = fmaxf(fminf(cy1, K.y1) - fmaxf(cy0, K.y0), 0.f) * fmaxf(fminf(cx1, K.x1) - fmaxf(cx0, K.x0), 0.f);
        const float uni = ca + K.area - inter;
        const bool valid = (lane < kept) && (ca > 0.f) && (K.area > 0.f);           // zero-area boxes never overlap (TF)
        unsigned long long hits = __ballot(valid && inter > g.hi * uni);
        if (hits == 0ull) {
            const bool band = valid && inter >= g.lo * uni;
            if (__ballot(band) != 0ull) hits = __ballot(band && (inter / uni > g.thr));
        }
        if (hits == 0ull) {
            if (lane == kept) {
                K.y0 = cy0;
                K.x0 = cx0;
                K.y1 = cy1;
                K.x1 = cx1;
                K.area = ca;
            }
            const int gi = __builtin_amdgcn_readlane(iv, t);
            const int gs = __builtin_amdgcn_readlane(sbits, t);
            if (lane == 0) {
                J.og[kept] = gi;
                J.os[kept] = __int_as_float(gs);
            }
            ++kept;
        }
    }
    K.kept = kept;
}

// ---- fast (the usual case: a few dozen candidates per class, n <= 512): rank sort, then the sweep
template <int MAXC>
__device__ __forceinline__ void fast_path(nms_lds<MAXC> &L, kept_set &K, const iou_gate g, const nms_job J, int n) {
    // ord[512] | key[512] alias the tail of the box array, which n <= 512 leaves free (MAXC = 1088: from byte 11264 = box 704)
    static_assert(MAXC * sizeof(float4) >= 512 * sizeof(float4) + 512 * (sizeof(int) + sizeof(unsigned long long)), "ord / key overlap boxes 0..511");
    static_assert((MAXC * sizeof(float4) - 512 * (sizeof(int) + sizeof(unsigned long long))) % 8 == 0, "key misaligned");
    const int lane = threadIdx.x;
    int *ord = reinterpret_cast<int *>(L.box + MAXC) - 512;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(ord) - 512;
    for (int c = lane; c < n; c += 64) key[c] = key_of(L.s[c], L.idx[c]);
    __syncthreads();
    for (int c = lane; c < n; c += 64) {
        const unsigned long long kc = key[c];
        int r = 0;
        for (int j = 0; j < n; ++j) r += key[j] > kc ? 1 : 0;
        ord[r] = c;
        normalise_box(L, c);
    }
    __syncthreads();
    for (int base = 0; base < n && K.kept < J.max_out; base += 64) {
        const int me = base + lane;
        const int pos = (me < n) ? ord[me] : 0;
        sweep_block(K, g, J, L.box[pos], __float_as_int(L.s[pos]), L.idx[pos], min(64, n - base));
    }
}

// ---- sorted sweep (round 6): the first nc candidates of the LDS arrays in descending (score, -index) order - a bitonic sort of one
// 64-bit key per candidate, (score bits, ~index : 20, LDS position : 12), written over L.s | L.idx - then the sweep.  One IoU + one ballot
// per candidate instead of two LDS passes over all of them per SELECTED box: 1 000 - 2 000 tied candidates per class (saturated logits)
// took ~0.5 ms per wave that way.
// presorted: the LDS arrays already ARE in key order (every score ties: order = box index = scan order): no sort, keys built in place
template <int MAXC>
__device__ __forceinline__ void sorted_sweep(nms_lds<MAXC> &L, kept_set &K, const iou_gate g, const nms_job J, int nc, bool presorted) {
    static_assert(MAXC <= 4096, "the key holds the LDS position in 12 bits (and the box index in 20: sweep_ok)");
    static_assert(offsetof(nms_lds<MAXC>, idx) == offsetof(nms_lds<MAXC>, s) + MAXC * sizeof(float) && offsetof(nms_lds<MAXC>, s) % 8 == 0 &&
                      offsetof(nms_lds<MAXC>, box) == offsetof(nms_lds<MAXC>, s) + MAXC * sizeof(unsigned long long),
                  "L.s | L.idx are not one 8-byte key per candidate");
    const int lane = threadIdx.x;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(L.s);
    int P = 64;
    while (P < nc && !presorted) P <<= 1;                                       // (callers make sure P <= MAXC)
    if (presorted) P = nc;
    constexpr int PL = (MAXC + 63) / 64;
    uint32_t sv[PL], iv[PL];
#pragma unroll
    for (int k = 0; k < PL; ++k) {
        const int c = lane + 64 * k;
        sv[k] = c < nc ? __float_as_uint(L.s[c]) : 0u;
        iv[k] = c < nc ? (uint32_t)L.idx[c] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PL; ++k) {
        const int c = lane + 64 * k;
        if (c < P) key[c] = c < nc ? (((unsigned long long)sv[k] << 32) | ((unsigned long long)((~iv[k]) & 0xfffffu) << 12) | (unsigned)c) : 0ull;
        if (c < nc) normalise_box(L, c);
    }
    __syncthreads();
    for (int k = 2; k <= P && !presorted; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = key[i], b = key[l];
                const bool desc = (i & k) == 0;
                if ((a < b) == desc) {
                    key[i] = b;
                    key[l] = a;
                }
            }
            __syncthreads();
        }
    for (int base = 0; base < nc && K.kept < J.max_out; base += 64) {
        const int me = base + lane;
        const unsigned long long kk = me < nc ? key[me] : 0ull;
        sweep_block(K, g, J, L.box[(int)(kk & 0xfffu)], (int)(uint32_t)(kk >> 32), (int)((~(uint32_t)(kk >> 12)) & 0xfffffu), min(64, nc - base));
    }
    __syncthreads();
}

// ---- tied: every candidate has the SAME score (saturated logits: what the random-init Darknet-53 of the benchmark produces, 1 000 - 10 647
// candidates per class at exactly 1.0): descending (score, -index) order is ascending box index, which is the order the scan compacted
// them in.  The LDS already holds the first chunk, sorted; later chunks are the next MAXC candidates of the same scan.
template <int MAXC>
__device__ __forceinline__ void tied_path(nms_lds<MAXC> &L, kept_set &K, const iou_gate g, const nms_job J, int n) {
    int done = 0;
    for (;;) {
        const int nc = min(n - done, MAXC);
        sorted_sweep(L, K, g, J, nc, true);
        done += nc;
        if (K.kept >= J.max_out || done >= n) break;
        __syncthreads();
        scan_scores<MAXC, true>(L, J.sc, J.ntot, J.obj_thresh, done);               // candidates ranked [done, done + MAXC) in scan order
        __syncthreads();
        fetch_boxes(L, J.bx, min(n - done, MAXC));
        __syncthreads();
    }
}

// ---- greedy: n <= MAXC candidates the sweep cannot take (max_out > 64, or 2^20 boxes and more): iterated arg-max over the LDS (yk_nms.h)
// RECORD (the overflow path's chunks): the first 256 selected box indices are also kept in selg, for the next chunk's dead pass
template <bool RECORD, int MAXC>
__device__ __forceinline__ int greedy_path(nms_lds<MAXC> &L, const nms_job J, int n, int base, int *selg) {
    return yk_wave_greedy_nms(
        n, L.s, L.idx, L.box, J.iou_thresh, J.max_out - base, [](const float4 &a, const float4 &d) { return tf_iou(d, a); },
        [&](int rank, int pos) {
            if (threadIdx.x == 0) {
                J.og[base + rank] = L.idx[pos];
                J.os[base + rank] = L.s[pos];
                if (RECORD && base + rank < 256) selg[base + rank] = L.idx[pos];
            }
        },
        [](int) {});
}

// ---- overflow: more candidates than the LDS holds (degenerate inputs: saturated logits - what 75 undamped random-init Darknet layers
// produce).  Greedy NMS only ever needs the candidates in descending (score, -index) order, and a candidate's fate depends only on the boxes
// selected before it - so the list is processed in CHUNKS of at most MAXC consecutive keys: find a key `lo` with count([lo, hi)) <= MAXC,
// gather that interval into LDS, drop what the boxes selected so far suppress, run the LDS greedy on the rest, continue below lo.
// `lo` comes from an MSD RADIX SELECT on the 64-bit key (score bits, ~index): one histogram pass (2^NBL bins in LDS) per level, the
// bin that crosses MAXC is split by the next level - 1-2 passes for distinct scores, <= 5 when thousands of scores tie (then the
// index bits decide).  Round 5 bisected on the key with one counting pass per step: ~45 passes per chunk, 1.44 ms of a 5.7 ms
// Darknet-53 step at 32 images (profiles/r06_darknet_pipeline_kernel_stats.csv); the old in-place loop before that: 10 ms.
template <int MAXC>
struct radix {
    static constexpr int NBL = MAXC >= 2048 ? 11 : 10, NB = 1 << NBL, PER = NB / 64;
    static_assert(NB % 64 == 0, "the bin walk gives every lane NB / 64 bins");
    static_assert(NB <= MAXC, "the histogram lives in L.idx");
};

// histogram of the candidates' keys in [lo_c, hi_c) over bins of 2^sh keys, in L.idx: free between chunks (the selected indices live in selg / og)
template <int MAXC>
__device__ __forceinline__ void hist_pass(nms_lds<MAXC> &L, const nms_job J, unsigned long long lo_c, unsigned long long hi_c, int sh) {
    const int lane = threadIdx.x;
    int *hist = L.idx;
    for (int q = lane; q < radix<MAXC>::NB; q += 64) hist[q] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < J.ntot; i0 += 64 * 16) {            // sixteen independent loads in flight per lane: the pass is latency-bound
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 64 + lane;
            v[u] = (i < J.ntot) ? J.sc[i] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 64 + lane;
            if (i < J.ntot && v[u] >= J.obj_thresh) {
                const unsigned long long k = key_of(v[u], i);
                if (k >= lo_c && k < hi_c) atomicAdd(&hist[(int)((k - lo_c) >> sh)], 1);
            }
        }
    }
    __syncthreads();
}

// select lo: the lowest key such that [lo, hi) holds <= MAXC candidates (a half-full chunk is good enough).  hi > key_min.
// Mirrors the inner loop of radix_chunks() in tests/nms_cases.py: keep the two together.
template <int MAXC>
__device__ __forceinline__ unsigned long long radix_select_lo(nms_lds<MAXC> &L, const nms_job J, unsigned long long key_min, unsigned long long hi) {
    constexpr int NBL = radix<MAXC>::NBL, PER = radix<MAXC>::PER;
    const int lane = threadIdx.x;
    const int *hist = L.idx;
    unsigned long long lo_c = key_min, hi_c = hi;
    int taken = 0;                                            // candidates in [hi_c, hi): already inside the chunk
    for (;;) {
        const unsigned long long range = hi_c - lo_c;                         // >= 1
        const int bits = range > 1ull ? 64 - __builtin_clzll(range - 1ull) : 0;
        const int sh = bits > NBL ? bits - NBL : 0;
        const int nb = (int)(((range - 1ull) >> sh) + 1ull);                  // <= NB
        hist_pass(L, J, lo_c, hi_c, sh);
        // walk the bins from the top: lane l owns bins nb-1-PER*l ... nb-PER-PER*l (PER = 32 or 16)
        int mine[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int q = nb - 1 - (lane * PER + j);
            mine[j] = q >= 0 ? hist[q] : 0;
            sum += mine[j];
        }
        int pre = sum;                                                        // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(pre, o, 64);
            if (lane >= o) pre += t;
        }
        const int before = pre - sum;                                         // candidates in the bins above this lane's
        const unsigned long long cross = __ballot(taken + pre > MAXC);
        if (cross == 0ull) return lo_c;                                       // 'all fits': everything down to lo_c
        const int cl = __ffsll((long long)cross) - 1;                         // the lane whose bins hold the crossing one
        int tq = 0, tk = 0;                                                   // crossing bin (counted from the top), candidates above it
        if (lane == cl) {
            int run = taken + before;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                if (run + mine[j] > MAXC) {
                    tq = lane * PER + j;
                    tk = run;
                    break;
                }
                run += mine[j];
            }
        }
        tq = __shfl(tq, cl, 64);
        tk = __shfl(tk, cl, 64);
        const int qb = nb - 1 - tq;                                           // the crossing bin's index
        const unsigned long long b_lo = lo_c + ((unsigned long long)qb << sh), b_hi = qb + 1 >= nb ? hi_c : b_lo + (1ull << sh);
        taken = tk;
        if (taken >= MAXC / 2 || sh == 0) return b_hi;                        // 'half full' / 'single keys': the chunk ends above the crossing bin
        lo_c = b_lo;                                                          // split the crossing bin
        hi_c = b_hi;
        // inside ONE score value the keys differ in ~index only, and ~i >= 2^32 - ntot: skip the empty part of the interval
        // (thousands of tied scores: the next level then bins the indices directly)
        if ((lo_c >> 32) == ((hi_c - 1ull) >> 32)) {
            const unsigned long long first = (lo_c & 0xffffffff00000000ull) | (0x100000000ull - (unsigned long long)J.ntot);
            if (first > lo_c && first < hi_c) lo_c = first;
        }
        __syncthreads();
    }
}

// the chunk loop: select lo, gather [lo, hi), consume.  'overflow-sweep' (sweep_ok, and only where MAXC holds the 2048 keys a full chunk sorts
// as): the sorted sweep, the selected boxes carry over in registers.  'overflow-greedy': the LDS greedy after the candidates a box of an earlier
// chunk overlaps are marked dead (those boxes: by index, selg for the first 256, else og).
// Mirrors the outer loop of radix_chunks() in tests/nms_cases.py.
template <int MAXC>
__device__ __forceinline__ void overflow_path(nms_lds<MAXC> &L, kept_set &K, const iou_gate g, const nms_job J, bool sweep_ok, int *selg) {
    const int lane = threadIdx.x;
    const unsigned long long key_min = (unsigned long long)__float_as_uint(fmaxf(J.obj_thresh, 0.f)) << 32;
    const int *selp = (J.max_out <= 256) ? selg : J.og;
    unsigned long long hi = ~0ull;
    while (K.kept < J.max_out) {
        if (hi <= key_min) break;
        const unsigned long long lo = radix_select_lo(L, J, key_min, hi);
        if (lo >= hi) break;                                                  // (cannot happen: a bin of one key holds at most one candidate)
        __syncthreads();
        const int nc = scan_scores(L, J.sc, J.ntot, J.obj_thresh, 0, [&](float v, int i) {
            const unsigned long long k = key_of(v, i);
            return k >= lo && k < hi;
        });
        __syncthreads();
        fetch_boxes(L, J.bx, nc);
        __syncthreads();
        bool swept = false;
        if constexpr (MAXC >= 2048) {
            if (sweep_ok) {
                sorted_sweep(L, K, g, J, min(nc, MAXC), false);
                swept = true;
            }
        }
        if (!swept) {
            for (int q = lane; q < nc; q += 64) {
                const float4 cb = L.box[q];
                bool dead = false;
                for (int k = 0; k < K.kept && !dead; ++k) dead = tf_iou(cb, J.bx[selp[k]]) > J.iou_thresh;
                if (dead) L.s[q] = -INFINITY;
            }
            __syncthreads();
            K.kept += greedy_path<true>(L, J, nc, K.kept, selg);
            __threadfence_block();
            __syncthreads();
        }
        if (lo == key_min) break;
        hi = lo;
    }
}

// grid (C, batch), one wavefront.  sel_g/sel_s: [batch][C][max_out]; cnt: [batch][C]
template <int MAXC>
__global__ void __launch_bounds__(64) nms_py_kernel(int ntot, int C, float obj_thresh, float iou_thresh, int max_out,
                                                    const float4 *__restrict__ boxes, float *__restrict__ scores_t,
                                                    int *__restrict__ sel_g, float *__restrict__ sel_s,
                                                    int *__restrict__ cnt) {
    __shared__ nms_lds<MAXC> L;
    __shared__ int selg[256];                                 // overflow, greedy consumer: global indices of the boxes selected so far
    const nms_job J = nms_job_of(ntot, C, obj_thresh, iou_thresh, max_out, boxes, scores_t, sel_g, sel_s);
    float cmin = INFINITY, cmax = -INFINITY;                  // candidate score range: all equal = the order is the box index = the scan order
    const int n = scan_scores(L, J.sc, ntot, obj_thresh, 0, take_all(), [&](float v) {
        cmin = fminf(cmin, v);
        cmax = fmaxf(cmax, v);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
    }
    const bool all_tied = n > 0 && cmin == cmax;
    __syncthreads();
    fetch_boxes(L, J.bx, min(n, MAXC));
    __syncthreads();
    kept_set K = {0.f, 0.f, 0.f, 0.f, 0.f, 0};
    const iou_gate g = iou_gate_of(iou_thresh);
    const bool sweep_ok = max_out <= 64 && ntot < (1 << 20);
    // The dispatch.  nms_path() in tests/nms_cases.py is a copy of this chain (it labels the test cases): keep the two together.
    if (n <= 512 && max_out <= 64)
        fast_path(L, K, g, J, n);
    else if (all_tied && sweep_ok)
        tied_path(L, K, g, J, n);
    else if (n <= MAXC && sweep_ok && (n <= 1024 ? 1024 : 2048) <= MAXC)
        sorted_sweep(L, K, g, J, n, false);
    else if (n <= MAXC)
        K.kept = greedy_path<false>(L, J, n, 0, nullptr);
    else
        overflow_path(L, K, g, J, sweep_ok, selg);                            // 'overflow-sweep' (sweep_ok && MAXC >= 2048) : 'overflow-greedy'
    if (threadIdx.x == 0) cnt[blockIdx.y * C + blockIdx.x] = K.kept;
}

// ---- Soft-NMS (linear, Gaussian) and DIoU-NMS: the rule of k210_yolo_framework_amd/softnms.py, operation for operation.
// The weight the selected box m puts on a live box q.  DIoU: centres and enclosing box from the min / max-normalised corners, in this order.
template <int METHOD>
__device__ __forceinline__ float soft_weight(const float4 &m, const float4 &q, float iou_thresh, float sigma) {
    const float o = tf_iou(m, q);
    if (METHOD == YK_NMS_LINEAR) return o > iou_thresh ? 1.f - o : 1.f;
    if (METHOD == YK_NMS_GAUSSIAN) return expf(-(o * o) / sigma);
    const float my0 = fminf(m.x, m.z), mx0 = fminf(m.y, m.w), my1 = fmaxf(m.x, m.z), mx1 = fmaxf(m.y, m.w);
    const float qy0 = fminf(q.x, q.z), qx0 = fminf(q.y, q.w), qy1 = fmaxf(q.x, q.z), qx1 = fmaxf(q.y, q.w);
    const float dy = (my0 + my1) * 0.5f - (qy0 + qy1) * 0.5f, dx = (mx0 + mx1) * 0.5f - (qx0 + qx1) * 0.5f;
    const float d2 = dy * dy + dx * dx;
    const float ey = fmaxf(my1, qy1) - fminf(my0, qy0), ex = fmaxf(mx1, qx1) - fminf(mx0, qx0);
    const float c2 = ey * ey + ex * ex;
    const float pen = c2 > 0.f ? d2 / c2 : 0.f;
    return o - pen > iou_thresh ? 0.f : 1.f;
}

// The rounds over `count` entries: entry i has the current score s[i] (live iff >= obj_thresh), the box box_of(i) and the box index idx_of(i),
// ascending in i.  Lane l owns the entries i = l (mod 64) and is the only one to read or write their scores, so a round needs no barrier
// and no atomic: an arg-max over (current score, lowest index) across the wave, then one decay pass.  Any max_out: rounds are sequential.
template <int METHOD, class BoxOf, class IdxOf>
__device__ __forceinline__ int soft_rounds(int count, float *s, BoxOf box_of, IdxOf idx_of, float obj_thresh, float iou_thresh, float sigma,
                                           int max_out, int *og, float *os) {
    const int lane = threadIdx.x;
    int kept = 0;
    while (kept < max_out) {
        float best = -INFINITY;
        int bidx = 0x7fffffff, bpos = -1;
        for (int i = lane; i < count; i += 64) {
            const float v = s[i];
            if (v >= obj_thresh && (bpos < 0 || v > best)) {          // ascending i: a tie stays with the lower box index
                best = v;
                bpos = i;
            }
        }
        if (bpos >= 0) bidx = idx_of(bpos);
        yk_wave_argmax(best, bidx, bpos);
        if (bpos < 0) break;
        if (lane == 0) {
            og[kept] = bidx;
            os[kept] = best;
        }
        ++kept;
        if (kept >= max_out) break;
        const float4 mb = box_of(bpos);
        for (int i = lane; i < count; i += 64) {
            const float v = s[i];
            if (i == bpos) {
                s[i] = -INFINITY;
            } else if (v >= obj_thresh) {
                const float w = soft_weight<METHOD>(mb, box_of(i), iou_thresh, sigma);
                const float nv = v * w;
                if (w == 0.f || nv < obj_thresh)
                    s[i] = -INFINITY;
                else if (METHOD != YK_NMS_DIOU)
                    s[i] = nv;
            }
        }
    }
    return kept;
}

// grid (C, batch), one wavefront, the LDS, the scan and the fetch of nms_py_kernel<MAXC>.  A class with more candidates than the LDS holds
// runs the same rounds over its score plane in global memory, decayed in place: the plane is this call's own scratch and decode_py_kernel
// rewrites it on every call.
template <int MAXC, int METHOD>
__global__ void __launch_bounds__(64) softnms_py_kernel(int ntot, int C, float obj_thresh, float iou_thresh, float sigma, int max_out,
                                                        const float4 *__restrict__ boxes, float *scores_t, int *__restrict__ sel_g,
                                                        float *__restrict__ sel_s, int *__restrict__ cnt) {
    __shared__ nms_lds<MAXC> L;
    const nms_job J = nms_job_of(ntot, C, obj_thresh, iou_thresh, max_out, boxes, scores_t, sel_g, sel_s);
    const int n = scan_scores(L, J.sc, ntot, obj_thresh, 0);
    __syncthreads();
    int kept;
    if (n <= MAXC) {
        fetch_boxes(L, J.bx, n);
        __syncthreads();
        kept = soft_rounds<METHOD>(
            n, L.s, [&](int i) { return L.box[i]; }, [&](int i) { return L.idx[i]; }, obj_thresh, iou_thresh, sigma, max_out, J.og, J.os);
    } else {
        kept = soft_rounds<METHOD>(
            ntot, J.sc, [&](int i) { return J.bx[i]; }, [](int i) { return i; }, obj_thresh, iou_thresh, sigma, max_out, J.og, J.os);
    }
    if (threadIdx.x == 0) cnt[blockIdx.y * C + blockIdx.x] = kept;
}

// ---- compaction: class-major concatenation (keras_inference.py:133-135), one thread per (class, rank) slot.
// thread 0: base[0..C] = exclusive prefix of image b's per-class counts; returns the image's row count
__device__ __forceinline__ int class_prefix(int *base, const int *__restrict__ cnt, int b, int C) {
    int acc = 0;
    for (int c = 0; c < C; ++c) {
        base[c] = acc;
        acc += cnt[b * C + c];
    }
    base[C] = acc;
    return acc;
}
// every live slot of image b: put(class, row within the image, box index, box, score)
template <class Put>
__device__ __forceinline__ void for_each_row(const int *base, int b, int ntot, int C, int max_out, const float4 *__restrict__ boxes,
                                             const int *__restrict__ sel_g, const float *__restrict__ sel_s, Put put) {
    for (int slot = threadIdx.x; slot < C * max_out; slot += 256) {
        const int c = slot / max_out, j = slot - c * max_out;
        if (j < base[c + 1] - base[c]) {
            const int g = sel_g[((size_t)b * C + c) * max_out + j];
            put(c, base[c] + j, g, boxes[(size_t)b * ntot + g], sel_s[((size_t)b * C + c) * max_out + j]);
        }
    }
}
__device__ __forceinline__ void put_row(float *d, const float4 &bb, float sv, int c) {
    d[0] = bb.x;
    d[1] = bb.y;
    d[2] = bb.z;
    d[3] = bb.w;
    d[4] = sv;
    d[5] = (float)c;
}

// grid (batch), 256 threads: rows of image b at dets[b][0 .. counts[b]), C * max_out rows per image
__global__ void __launch_bounds__(256) compact_py_kernel(int ntot, int C, int max_out, const float4 *__restrict__ boxes,
                                                         const int *__restrict__ sel_g, const float *__restrict__ sel_s,
                                                         const int *__restrict__ cnt, float *__restrict__ dets,
                                                         int *__restrict__ counts, int *__restrict__ box_index) {
    extern __shared__ int base[];                   // [C + 1]
    const int b = blockIdx.x;
    if (threadIdx.x == 0) counts[b] = class_prefix(base, cnt, b, C);
    __syncthreads();
    for_each_row(base, b, ntot, C, max_out, boxes, sel_g, sel_s, [&](int c, int row, int g, const float4 &bb, float sv) {
        put_row(dets + ((size_t)b * C * max_out + row) * 6, bb, sv, c);
        if (box_index) box_index[(size_t)b * C * max_out + row] = g;
    });
}

// The same concatenation ACROSS the batch: rows of image b start at offsets[b] (offsets[batch] = total), nothing between the images.
// `rows` / `offsets` / `box_index` may be device memory or pinned, device-mapped HOST memory: in the second case the detections land on
// the host at their live size (a few KB) with no device-to-host copy to size or to wait for.  grid (batch), 256 threads.
__global__ void __launch_bounds__(256) compact_packed_kernel(int ntot, int C, int max_out, int batch, const float4 *__restrict__ boxes,
                                                            const int *__restrict__ sel_g, const float *__restrict__ sel_s,
                                                            const int *__restrict__ cnt, float *rows, int *offsets, int *box_index,
                                                            float *__restrict__ dets, int *__restrict__ counts) {
    extern __shared__ int base[];                   // [C + 1], then [C + 1] = rows of the images before this one
    __shared__ int part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int before = 0;
    for (int i = tid; i < b * C; i += 256) before += cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = before;
    __syncthreads();
    if (tid == 0) {
        const int acc = class_prefix(base, cnt, b, C);
        const int first = part[0] + part[1] + part[2] + part[3];
        base[C + 1] = first;
        offsets[b] = first;
        if (b == batch - 1) offsets[batch] = first + acc;
        if (counts) counts[b] = acc;
    }
    __syncthreads();
    const int first = base[C + 1];
    for_each_row(base, b, ntot, C, max_out, boxes, sel_g, sel_s, [&](int c, int row, int g, const float4 &bb, float sv) {
        float2 *d = reinterpret_cast<float2 *>(rows + ((size_t)first + row) * 6);      // rows are 24 bytes: 8-byte aligned
        d[0] = make_float2(bb.x, bb.y);
        d[1] = make_float2(bb.z, bb.w);
        d[2] = make_float2(sv, (float)c);
        if (box_index) box_index[(size_t)first + row] = g;
        if (dets) put_row(dets + ((size_t)b * C * max_out + row) * 6, bb, sv, c);
    });
}

// ---- host side
template <int MAXC>
static void launch_nms(int method, dim3 grid, hipStream_t st, int ntot, int C, float obj_thresh, float iou_thresh, float sigma, int max_out,
                       const float4 *boxes, float *scores_t, int *sel_g, float *sel_s, int *cnt) {
    if (method == YK_NMS_HARD)
        hipLaunchKernelGGL(nms_py_kernel<MAXC>, grid, dim3(64), 0, st, ntot, C, obj_thresh, iou_thresh, max_out, boxes, scores_t, sel_g, sel_s, cnt);
    else if (method == YK_NMS_LINEAR)
        hipLaunchKernelGGL((softnms_py_kernel<MAXC, YK_NMS_LINEAR>), grid, dim3(64), 0, st, ntot, C, obj_thresh, iou_thresh, sigma, max_out, boxes,
                           scores_t, sel_g, sel_s, cnt);
    else if (method == YK_NMS_GAUSSIAN)
        hipLaunchKernelGGL((softnms_py_kernel<MAXC, YK_NMS_GAUSSIAN>), grid, dim3(64), 0, st, ntot, C, obj_thresh, iou_thresh, sigma, max_out, boxes,
                           scores_t, sel_g, sel_s, cnt);
    else
        hipLaunchKernelGGL((softnms_py_kernel<MAXC, YK_NMS_DIOU>), grid, dim3(64), 0, st, ntot, C, obj_thresh, iou_thresh, sigma, max_out, boxes,
                           scores_t, sel_g, sel_s, cnt);
}

// where a call's detections go: the padded layout (dets / counts / box_index), the packed one (rows / offsets / rows_index), or both
struct decode_out {
    float *dets;
    int32_t *counts, *box_index;
    float *rows;
    int32_t *offsets, *rows_index;
};

static int bad_argument(const char *who) {
    yk_set_error("%s: bad argument", who);
    return YK_ERR_ARG;
}

static int decode_impl(const char *who, const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                       float obj_thresh, float iou_thresh, int max_out, const decode_out &out, void *stream, int nms_method, float nms_sigma) {
    if (!cfg || !d_pred || batch <= 0 || max_out <= 0 || cfg->n_layers <= 0 ||
        cfg->n_layers > YK_MAX_LAYERS || cfg->anchor_num <= 0 || cfg->anchor_num > YK_MAX_ANCHORS ||
        cfg->class_num <= 0)
        return bad_argument(who);
    decode_args a;
    memset(&a, 0, sizeof(a));
    a.L = cfg->n_layers;
    a.A = cfg->anchor_num;
    a.C = cfg->class_num;
    a.E = 5 + cfg->class_num;
    a.in_h = cfg->in_h;
    a.in_w = cfg->in_w;
    int off = 0;
    for (int l = 0; l < a.L; ++l) {
        if (!d_pred[l] || cfg->out_h[l] <= 0 || cfg->out_w[l] <= 0) {
            yk_set_error("%s: layer %d null / empty", who, l);
            return YK_ERR_ARG;
        }
        a.out_h[l] = cfg->out_h[l];
        a.out_w[l] = cfg->out_w[l];
        a.off[l] = off;
        off += cfg->out_h[l] * cfg->out_w[l] * a.A;
        a.pred[l] = d_pred[l];
        for (int n = 0; n < a.A; ++n) {
            a.anchors[l][n][0] = cfg->anchors[l][n][0];
            a.anchors[l][n][1] = cfg->anchors[l][n][1];
        }
    }
    a.off[a.L] = off;
    const int ntot = off;
    int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("%s: no HIP device", who);
        return YK_ERR_NO_DEVICE;
    }
    // the scratch, carved in this order at 256-byte steps: boxes | score planes | selected indices | selected scores | per-class counts
    size_t need = 0;
    auto carve = [&need](size_t bytes) {
        const size_t at = need;
        need += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t sel_b = (size_t)batch * a.C * max_out * sizeof(int);
    const size_t at_box = carve((size_t)batch * ntot * sizeof(float4)), at_sc = carve((size_t)batch * a.C * ntot * sizeof(float));
    const size_t at_selg = carve(sel_b), at_sels = carve(sel_b), at_cnt = carve((size_t)batch * a.C * sizeof(int));
    char *ws = (char *)yk_scratch(dev, stream, YK_SLOT_DECODE, need);
    if (!ws) return YK_ERR_NOMEM;
    float4 *boxes = (float4 *)(ws + at_box);
    float *scores_t = (float *)(ws + at_sc);
    int *sel_g = (int *)(ws + at_selg);
    float *sel_s = (float *)(ws + at_sels);
    int *cnt = (int *)(ws + at_cnt);
    hipStream_t st = (hipStream_t)stream;
    const int total = batch * ntot;
    hipLaunchKernelGGL(decode_py_kernel, dim3((total + 255) / 256), dim3(256), 0, st, a, batch, d_image_hw, boxes,
                       scores_t);
    if (nms_maxc(ntot) == 1088)
        launch_nms<1088>(nms_method, dim3(a.C, batch), st, ntot, a.C, obj_thresh, iou_thresh, nms_sigma, max_out, boxes, scores_t, sel_g, sel_s, cnt);
    else
        launch_nms<2048>(nms_method, dim3(a.C, batch), st, ntot, a.C, obj_thresh, iou_thresh, nms_sigma, max_out, boxes, scores_t, sel_g, sel_s, cnt);
    if (out.rows)
        hipLaunchKernelGGL(compact_packed_kernel, dim3(batch), dim3(256), (a.C + 2) * sizeof(int), st, ntot, a.C, max_out, batch, boxes, sel_g,
                           sel_s, cnt, out.rows, out.offsets, out.rows_index, out.dets, out.counts);
    else
        hipLaunchKernelGGL(compact_py_kernel, dim3(batch), dim3(256), (a.C + 1) * sizeof(int), st, ntot, a.C, max_out, boxes, sel_g, sel_s, cnt,
                           out.dets, out.counts, out.box_index);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// the rule's own arguments, checked before anything else is looked at or launched
static int check_nms(const char *who, int nms_method, float nms_sigma) {
    if (nms_method < YK_NMS_HARD || nms_method > YK_NMS_DIOU) {
        yk_set_error("%s: nms_method %d is none of YK_NMS_HARD, _LINEAR, _GAUSSIAN, _DIOU", who, nms_method);
        return YK_ERR_ARG;
    }
    if (nms_method == YK_NMS_GAUSSIAN && !(nms_sigma > 0.f && nms_sigma < INFINITY)) {
        yk_set_error("%s: nms_sigma %g is not positive and finite", who, (double)nms_sigma);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

// The entry points: the rule's check, the pointers their layout cannot do without (padded: dets and counts; packed: rows and offsets), one call.
extern "C" int yk_decode_py(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                            float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts,
                            void *stream) {
    if (!d_dets || !d_counts) return bad_argument(__func__);
    return decode_impl(__func__, cfg, d_pred, batch, d_image_hw, obj_thresh, iou_thresh, max_out, {d_dets, d_counts, nullptr, nullptr, nullptr, nullptr},
                       stream, YK_NMS_HARD, 0.5f);
}

extern "C" int yk_decode_py_ex(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                               float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts,
                               int32_t *d_box_index, void *stream) {
    if (!d_dets || !d_counts) return bad_argument(__func__);
    return decode_impl(__func__, cfg, d_pred, batch, d_image_hw, obj_thresh, iou_thresh, max_out, {d_dets, d_counts, d_box_index, nullptr, nullptr, nullptr},
                       stream, YK_NMS_HARD, 0.5f);
}

extern "C" int yk_decode_py_packed(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                                   float obj_thresh, float iou_thresh, int max_out, float *rows, int32_t *offsets, int32_t *rows_index,
                                   float *d_dets, int32_t *d_counts, void *stream) {
    if (!rows || !offsets) return bad_argument(__func__);
    return decode_impl(__func__, cfg, d_pred, batch, d_image_hw, obj_thresh, iou_thresh, max_out, {d_dets, d_counts, nullptr, rows, offsets, rows_index},
                       stream, YK_NMS_HARD, 0.5f);
}

extern "C" int yk_decode_py_nms(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                                float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts,
                                int32_t *d_box_index, void *stream, int nms_method, float nms_sigma) {
    if (const int rc = check_nms(__func__, nms_method, nms_sigma)) return rc;
    if (!d_dets || !d_counts) return bad_argument(__func__);
    return decode_impl(__func__, cfg, d_pred, batch, d_image_hw, obj_thresh, iou_thresh, max_out, {d_dets, d_counts, d_box_index, nullptr, nullptr, nullptr},
                       stream, nms_method, nms_sigma);
}

extern "C" int yk_decode_py_packed_nms(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                                       float obj_thresh, float iou_thresh, int max_out, float *rows, int32_t *offsets, int32_t *rows_index,
                                       float *d_dets, int32_t *d_counts, void *stream, int nms_method, float nms_sigma) {
    if (const int rc = check_nms(__func__, nms_method, nms_sigma)) return rc;
    if (!rows || !offsets) return bad_argument(__func__);
    return decode_impl(__func__, cfg, d_pred, batch, d_image_hw, obj_thresh, iou_thresh, max_out, {d_dets, d_counts, nullptr, rows, offsets, rows_index},
                       stream, nms_method, nms_sigma);
}

