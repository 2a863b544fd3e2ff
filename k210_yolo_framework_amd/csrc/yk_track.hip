// yk_track.hip — identities across frames for the decode's rows (k210_yolo_framework_amd/track.py states the rule, ByteTrack restated with a
// class-aware association, greedy or optimal).
//
// Tracking is a chain over time: frame t cannot start before frame t - 1 has ended.  The parallelism there is lies across sequences, across
// the tracks of a sequence and across the rows of a frame, and that is how the work is split:
//   - one wavefront per sequence, sequences side by side on different CUs; the frames of a sequence inside one call are walked in order
//     inside the kernel;
//   - a sequence's tracks (25 words each, field-major so that lane i reads word i) are loaded into LDS once per call, stay there across all
//     of the call's frames and are written back once;
//   - per frame the rows that take part are compacted by ballot into LDS (box, score, class and kind: 24 bytes a row);
//   - lanes own tracks (lane, lane + 64, ...): predict, update, open and emit are one track (or one row) per lane;
//   - matching: every track keeps its best free row in LDS, a wave reduction picks the stage's best pair (largest IoU, lowest track, lowest
//     row), and only the tracks whose cached row was just taken look again;
//   - matching, assign = lap (a second instantiation of the kernel; the greedy one carries none of it): per stage and class the eligible
//     tracks and rows are compacted by ballot into two index lists in LDS and motmetrics.lap's shortest augmenting paths run on the dense
//     nr x nc problem, the smaller side as the solver's rows.  The solver is yk_lap.h's yk_lap_wave, the one yk_mot.hip's scores call; this
//     unit gives it its costs (track_pair_cost).  MATRIX-FREE: 1024 x cap float64 costs do not fit beside the tracks, so a cost is
//     recomputed where the solver reads it - tf_iou of two LDS-resident boxes, the optional score multiply, the gate, 1.0 - (double)s or
//     2^20 - which is LDS reads and VALU only.  The solver row's box is held in registers across the sweep.
// No atomics anywhere, so two calls give the same bytes.  A 2 x 2 filter and an arg-max have no matrix product in them: no MFMA.
// Compiled with -ffp-contract=off: one rounding per operation, as track.py's float32 steps.
#include <vector>

#include "yk_common.h"
#include "yk_lap.h"
#include "yk_nms.h"

#define YK_TRACK_WORDS 25                 // a track in the state: id, class, state, last frame | score, mean[8], cov[12]
#define YK_TRACK_HEADER 4                 // a sequence's header: live tracks, next id, frames seen, overflow
#define YK_TRACK_LDS_PER_TRACK 128        // the 25 words + predicted box (16) + matched row, best IoU, best row (12)
#define YK_TRACK_LDS_PER_ROW 24
// assign = lap, on top of the two above: a share of the solver's vectors and, per row, an entry of the class's index list (4; the tracks'
// list lies where the greedy path keeps its best IoU, which lap never reads).  lap_carve's vectors of the longer side (YK_LAP_LDS_PER_COL
// bytes an entry) are carved for max(M, cap) entries and those of the shorter (YK_LAP_LDS_PER_ROW) for min(M, cap), which 28 bytes per track
// and per row cover whichever side is longer.
#define YK_TRACK_LAP_LDS_PER_TRACK YK_LAP_LDS_PER_COL
#define YK_TRACK_LAP_LDS_PER_ROW (4 + YK_LAP_LDS_PER_COL)
#define YK_TRACK_LAP_FORBIDDEN 1048576.0  // 2^20: above any sum of 1024 allowed costs, and a power of two (track.py says why)
#define YK_TRACK_LDS_LIMIT (160 * 1024)

enum { T_NEW = 0, T_TRACKED = 1, T_LOST = 2, T_DEAD = 3 };
enum { R_TAKEN = 0, R_LOW = 1, R_HIGH = 2 };

#define TI(f, i) Ti[(f) * M + (i)]        // 0 id, 1 class, 2 state, 3 frame of the last match
#define TF(f, i) Tf[(f) * M + (i)]        // 0 score, 1..4 x (cx, cy, a, h), 5..8 v, 9..12 pp, 13..16 pv, 17..20 vv

struct track_lds {
    float4 *Pbox, *Rbox;                  // [M] the tracks' predicted boxes, [cap] the frame's rows
    float *Rs;                            // [cap] scores
    int *Ri;                              // [cap] class * 4 + kind (R_*)
    int *Ti;                              // [4][M]
    float *Tf;                            // [21][M]
    int *Tm;                              // [M] the row a track matched in this frame, or -1
    float *Tbest;                         // [M] the IoU of the track's best free row in the running stage
    int *Tbrow;                           // [M] that row, or -1
    // assign = lap only
    lap_lds S;                            // the solver's vectors: min(M, cap) rows, max(M, cap) columns
    int *Tidx, *Ridx;                     // [M], [cap] the stage's eligible tracks and rows of the running class, ascending
};

__device__ __forceinline__ void measure(const float4 &b, float z[4]) {
    const float w = b.w - b.y, h = b.z - b.x;
    z[0] = (b.y + b.w) * 0.5f;
    z[1] = (b.x + b.z) * 0.5f;
    z[2] = w / h;
    z[3] = h;
}

__device__ __forceinline__ float4 box_of(float cx, float cy, float a, float h) {
    const float hw = (a * h) * 0.5f, hh = h * 0.5f;
    return make_float4(cy - hh, cx - hw, cy + hh, cx + hw);
}

// (pos * h / 20)^2 and (vel * h / 160)^2
__device__ __forceinline__ void noise(float h, float pos, float vel, float &p2, float &v2) {
    float sp = h / 20.f, sv = h / 160.f;
    if (pos != 1.f) sp = pos * sp;
    if (vel != 1.f) sv = vel * sv;
    p2 = sp * sp;
    v2 = sv * sv;
}

// the similarity of a pair: the decode's float32 IoU, in stage 1 with fuse_score times the row's score (one rounding)
template <bool FUSE>
__device__ __forceinline__ float pair_sim(const float4 &pb, const float4 &rb, float score) {
    const float o = tf_iou(pb, rb);
    return FUSE ? o * score : o;
}

// the best free row of track i among the rows of `kind` and the track's class: the largest similarity >= thr, ties to the lowest row
template <bool FUSE>
__device__ __forceinline__ void scan_rows(const track_lds &L, int M, int i, int n_rows, int kind, float thr) {
    const float4 pb = L.Pbox[i];
    const int want = L.Ti[1 * M + i] * 4 + kind;
    float best = -INFINITY;
    int brow = -1;
    for (int r = 0; r < n_rows; ++r) {
        if (L.Ri[r] != want) continue;
        const float o = pair_sim<FUSE>(pb, L.Rbox[r], FUSE ? L.Rs[r] : 0.f);
        if (o >= thr && (brow < 0 || o > best)) {
            best = o;
            brow = r;
        }
    }
    L.Tbest[i] = best;
    L.Tbrow[i] = brow;
}

// does track i take part in a stage: unmatched in this frame, and its state in `states` (a bit set)
__device__ __forceinline__ bool eligible(const track_lds &L, int M, int i, unsigned states) {
    return L.Tm[i] < 0 && ((states >> L.Ti[2 * M + i]) & 1u);
}

// one chunk of a ballot compaction: the slot of this lane's item (`count` + the takers in the lanes below); `count` moves past the chunk's takers
__device__ __forceinline__ int ballot_slot(bool take, unsigned long long below, int &count) {
    const unsigned long long m = __ballot(take);
    const int pos = count + __popcll(m & below);
    count += __popcll(m);
    return pos;
}

// one association stage: the tracks whose state is in `states` (a bit set) and that are unmatched against the free rows of `kind`
template <bool FUSE>
__device__ __forceinline__ void match_stage(const track_lds &L, int M, int lane, int n_live, int n_rows, unsigned states, int kind, float thr) {
    for (int i = lane; i < n_live; i += 64) {
        if (eligible(L, M, i, states)) {
            scan_rows<FUSE>(L, M, i, n_rows, kind, thr);
        } else {
            L.Tbest[i] = -INFINITY;
            L.Tbrow[i] = -1;
        }
    }
    __syncthreads();
    for (;;) {
        float best = -INFINITY;
        int bidx = 0x7fffffff, bpos = -1;
        for (int i = lane; i < n_live; i += 64) {                        // ascending i: a tie stays with the lower track
            const float v = L.Tbest[i];
            if (L.Tbrow[i] >= 0 && (bpos < 0 || v > best)) {
                best = v;
                bidx = bpos = i;
            }
        }
        yk_wave_argmax(best, bidx, bpos);
        if (bpos < 0) break;
        const int r = L.Tbrow[bpos];
        __syncthreads();
        if (lane == 0) {
            L.Tm[bpos] = r;
            L.Ri[r] &= ~3;                                               // R_TAKEN
            L.Tbest[bpos] = -INFINITY;
            L.Tbrow[bpos] = -1;
        }
        __syncthreads();
        for (int i = lane; i < n_live; i += 64)
            if (L.Tbrow[i] == r) scan_rows<FUSE>(L, M, i, n_rows, kind, thr);
        __syncthreads();
    }
}

// ---- assign = lap: motmetrics.lap on the stage's pairs of one class, matrix-free ---------------------------------------------------------

// the cost of a pair: an allowed one (gate met; a NaN meets none) 1 - s in float64, a forbidden one 2^20
__device__ __forceinline__ double lap_cost(float s, float thr) { return s >= thr ? 1.0 - (double)s : YK_TRACK_LAP_FORBIDDEN; }

// yk_lap_wave's cost source: solver row i and column j are positions in rowlist and collist; the pair's cost is recomputed from the two boxes.
// The solver row's box (and its score, where the rows of the frame are the solver's rows) stay in registers for the sweep.
template <bool FUSE>
struct track_pair_cost {
    const track_lds &L;
    const int *rowlist, *collist;
    bool tall;
    float thr;
    struct row_costs {
        const track_pair_cost &P;
        float4 ob;
        float os;
        __device__ __forceinline__ double operator()(int j) const {
            const int other = P.collist[j];
            const float s = P.tall ? pair_sim<FUSE>(P.L.Pbox[other], ob, os) : pair_sim<FUSE>(ob, P.L.Rbox[other], FUSE ? P.L.Rs[other] : 0.f);
            return lap_cost(s, P.thr);
        }
    };
    __device__ __forceinline__ row_costs row(int i) const {
        const int own = rowlist[i];
        return {*this, tall ? L.Rbox[own] : L.Pbox[own], (FUSE && tall) ? L.Rs[own] : 0.f};
    }
};

// One class of one stage by the wavefront: nt tracks (L.Tidx) x nr rows (L.Ridx), both ascending.  The solver's rows are the smaller side
// (`tall`: more tracks than rows, the transpose, as motmetrics.lap); its m rows and n columns are positions in the two lists.
// Leaves the allowed pairs in L.Tm and their rows R_TAKEN.
template <bool FUSE>
__device__ __forceinline__ void lap_solve_class(const track_lds &L, int lane, int nt, int nr, float thr) {
    const bool tall = nt > nr;
    const int m = tall ? nr : nt, n = tall ? nt : nr;
    const int *rowlist = tall ? L.Ridx : L.Tidx, *collist = tall ? L.Tidx : L.Ridx;
    yk_lap_wave(track_pair_cost<FUSE>{L, rowlist, collist, tall, thr}, m, n, L.S, lane);
    // every solver row holds a column (m <= n); the pair is kept where it is allowed.  Tracks and rows of distinct pairs are distinct.
    for (int i = lane; i < m; i += 64) {
        const int a = rowlist[i], b = collist[L.S.col4row[i]];
        const int t = tall ? b : a, r = tall ? a : b;
        if (pair_sim<FUSE>(L.Pbox[t], L.Rbox[r], FUSE ? L.Rs[r] : 0.f) >= thr) {
            L.Tm[t] = r;
            L.Ri[r] &= ~3;                                               // R_TAKEN
        }
    }
    __syncthreads();
}

// one association stage under assign = lap: the classes that have an eligible track, ascending; one solve per class that has a row too
template <bool FUSE>
__device__ __forceinline__ void lap_stage(const track_lds &L, int M, int lane, unsigned long long below, int n_live, int n_rows, unsigned states,
                                          int kind, float thr) {
    int prev = -1;
    for (;;) {
        int c = 0x7fffffff;                                              // the lowest class above `prev` among the eligible tracks
        for (int i = lane; i < n_live; i += 64) {
            const int ci = L.Ti[1 * M + i];
            if (eligible(L, M, i, states) && ci > prev && ci < c) c = ci;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
        if (c == 0x7fffffff) break;
        prev = c;
        int nt = 0, nr = 0;
        for (int base = 0; base < n_live; base += 64) {
            const int i = base + lane;
            const bool take = i < n_live && eligible(L, M, i, states) && L.Ti[1 * M + i] == c;
            const int pos = ballot_slot(take, below, nt);
            if (take) L.Tidx[pos] = i;
        }
        const int want = c * 4 + kind;
        for (int base = 0; base < n_rows; base += 64) {
            const int r = base + lane;
            const bool take = r < n_rows && L.Ri[r] == want;
            const int pos = ballot_slot(take, below, nr);
            if (take) L.Ridx[pos] = r;
        }
        __syncthreads();
        if (nr > 0) lap_solve_class<FUSE>(L, lane, nt, nr, thr);
    }
}

// motion: NULL, or [n_frames][2] (mx, my) per frame, added to every track's centre before the frame's predict step.
// grid (n_seq), one wavefront; dynamic LDS: 128 bytes per track of M and 24 per row of cap, with ASSIGN = lap 28 and 32 more.
// ASSIGN (YK_TRACK_ASSIGN_*) and FUSE (stage 1's similarity is IoU * score) are compile-time: <GREEDY, false> is the kernel of before.
template <int ASSIGN, bool FUSE>
__global__ void __launch_bounds__(64) track_update_kernel(int32_t *__restrict__ state, int M, const float *__restrict__ dets,
                                                          const int32_t *__restrict__ counts, int cap, const int32_t *__restrict__ seq_first,
                                                          int n_frames, int class_num, float track_thresh, float low_thresh, float stage1,
                                                          float open_thresh, int track_buffer, float *__restrict__ out,
                                                          int32_t *__restrict__ out_ids, int32_t *__restrict__ out_counts,
                                                          float *__restrict__ draw, const float *__restrict__ motion) {
    extern __shared__ float4 lds_raw[];
    track_lds L;
    L.Pbox = lds_raw;
    L.Rbox = L.Pbox + M;
    L.Rs = reinterpret_cast<float *>(L.Rbox + cap);
    L.Ri = reinterpret_cast<int *>(L.Rs + cap);
    L.Ti = L.Ri + cap;
    L.Tf = reinterpret_cast<float *>(L.Ti + 4 * M);
    L.Tm = reinterpret_cast<int *>(L.Tf + 21 * M);
    L.Tbest = reinterpret_cast<float *>(L.Tm + M);
    L.Tbrow = reinterpret_cast<int *>(L.Tbest + M);
    if constexpr (ASSIGN == YK_TRACK_ASSIGN_LAP) {                       // (128 M + 24 cap bytes lie before: a multiple of 8)
        // lap_carve's vectors end lap_vector_bytes(shorter, longer) = 28 longer + 12 shorter bytes behind Tbrow, col4row [shorter] last:
        // with Ridx [cap] behind it that is the 28 M + 32 cap of YK_TRACK_LAP_LDS_PER_TRACK / _PER_ROW at the most
        const int shorter = min(M, cap);
        L.S = lap_carve(L.Tbrow + M, shorter, max(M, cap));
        L.Ridx = L.S.col4row + shorter;
        L.Tidx = reinterpret_cast<int *>(L.Tbest);                       // (Tbest and Tbrow are the greedy path's alone)
    }
    int *Ti = L.Ti;
    float *Tf = L.Tf;
    const int s = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const float AP2 = 1e-2f * 1e-2f, AV2 = 1e-5f * 1e-5f, AR2 = 1e-1f * 1e-1f;

    int32_t *mine = state + (size_t)s * (YK_TRACK_HEADER + YK_TRACK_WORDS * (size_t)M);
    int n_live = min(max(mine[0], 0), M), next_id = mine[1], frame = mine[2], overflow = mine[3];
    for (int f = 0; f < YK_TRACK_WORDS; ++f)                            // (Ti and Tf are adjacent: 25 fields of M words)
        for (int i = lane; i < n_live; i += 64) Ti[f * M + i] = mine[YK_TRACK_HEADER + f * M + i];
    __syncthreads();

    const int f0 = min(max(seq_first[s], 0), n_frames), f1 = min(max(seq_first[s + 1], 0), n_frames);
    for (int f = f0; f < f1; ++f) {
        ++frame;
        // 0  camera-motion compensation (yk_track_update_gmc): every centre moves by the frame's (mx, my); v and P stay
        const float mx = motion ? motion[2 * (size_t)f] : 0.f, my = motion ? motion[2 * (size_t)f + 1] : 0.f;
        // 1  predict
        for (int i = lane; i < n_live; i += 64) {
            if (motion) {
                TF(1, i) = TF(1, i) + mx;
                TF(2, i) = TF(2, i) + my;
            }
            if (TI(2, i) == T_LOST) TF(8, i) = 0.f;
            float qp, qv;
            noise(TF(4, i), 1.f, 1.f, qp, qv);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = TF(1 + k, i), v = TF(5 + k, i), pp = TF(9 + k, i), pv = TF(13 + k, i), vv = TF(17 + k, i);
                TF(1 + k, i) = x + v;
                TF(9 + k, i) = (((pp + pv) + pv) + vv) + (k == 2 ? AP2 : qp);
                TF(13 + k, i) = pv + vv;
                TF(17 + k, i) = vv + (k == 2 ? AV2 : qv);
            }
            L.Pbox[i] = box_of(TF(1, i), TF(2, i), TF(3, i), TF(4, i));
            L.Tm[i] = -1;
        }
        // 2  the rows that take part, compacted in row order
        const int k_rows = min(max(counts[f], 0), cap);
        int n_rows = 0;
        for (int base = 0; base < k_rows; base += 64) {
            const int r = base + lane;
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            float sc = 0.f, cf = -1.f;
            if (r < k_rows) {
                const float *row = dets + ((size_t)f * cap + r) * 6;
                b = make_float4(row[0], row[1], row[2], row[3]);
                sc = row[4];
                cf = row[5];
            }
            const float h = b.z - b.x, w = b.w - b.y;
            const bool take = r < k_rows && cf >= 0.f && cf < (float)class_num && cf == floorf(cf) && sc >= low_thresh && h > 0.f && h < INFINITY &&
                              w > 0.f && w < INFINITY;
            const int pos = ballot_slot(take, below, n_rows);
            if (take) {
                L.Rbox[pos] = b;
                L.Rs[pos] = sc;
                L.Ri[pos] = (int)cf * 4 + (sc >= track_thresh ? R_HIGH : R_LOW);
            }
        }
        __syncthreads();
        // 3  the three associations
        if constexpr (ASSIGN == YK_TRACK_ASSIGN_LAP) {
            lap_stage<FUSE>(L, M, lane, below, n_live, n_rows, (1u << T_TRACKED) | (1u << T_LOST), R_HIGH, stage1);
            lap_stage<false>(L, M, lane, below, n_live, n_rows, 1u << T_TRACKED, R_LOW, 0.5f);
            lap_stage<false>(L, M, lane, below, n_live, n_rows, 1u << T_NEW, R_HIGH, 0.3f);
        } else {
            match_stage<FUSE>(L, M, lane, n_live, n_rows, (1u << T_TRACKED) | (1u << T_LOST), R_HIGH, stage1);
            match_stage<false>(L, M, lane, n_live, n_rows, 1u << T_TRACKED, R_LOW, 0.5f);
            match_stage<false>(L, M, lane, n_live, n_rows, 1u << T_NEW, R_HIGH, 0.3f);
        }
        // 4  update the matched, retire the others
        for (int i = lane; i < n_live; i += 64) {
            const int r = L.Tm[i];
            if (r >= 0) {
                float z[4], r2, unused;
                measure(L.Rbox[r], z);
                noise(TF(4, i), 1.f, 1.f, r2, unused);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float x = TF(1 + k, i), v = TF(5 + k, i), pp = TF(9 + k, i), pv = TF(13 + k, i), vv = TF(17 + k, i);
                    const float sk = pp + (k == 2 ? AR2 : r2);
                    const float kp = pp / sk, kv = pv / sk, y = z[k] - x;
                    TF(1 + k, i) = x + kp * y;
                    TF(5 + k, i) = v + kv * y;
                    TF(9 + k, i) = pp - kp * pp;
                    TF(13 + k, i) = pv - kp * pv;
                    TF(17 + k, i) = vv - kv * pv;
                }
                TI(2, i) = T_TRACKED;
                TI(3, i) = frame;
                TF(0, i) = L.Rs[r];
            } else {
                TI(2, i) = (TI(2, i) != T_NEW && frame - TI(3, i) <= track_buffer) ? T_LOST : T_DEAD;
            }
        }
        __syncthreads();
        // a stable compaction in place: a chunk is read whole before any of it is written, and lands at or below where it was
        int n_kept = 0;
        for (int base = 0; base < n_live; base += 64) {
            const int i = base + lane;
            const bool alive = i < n_live && TI(2, i) != T_DEAD;
            int w[YK_TRACK_WORDS];
            if (alive) {
#pragma unroll
                for (int f2 = 0; f2 < YK_TRACK_WORDS; ++f2) w[f2] = Ti[f2 * M + i];
            }
            const unsigned long long m = __ballot(alive);
            __syncthreads();
            if (alive) {
                const int pos = n_kept + __popcll(m & below);
#pragma unroll
                for (int f2 = 0; f2 < YK_TRACK_WORDS; ++f2) Ti[f2 * M + pos] = w[f2];
            }
            n_kept += __popcll(m);
            __syncthreads();
        }
        n_live = n_kept;
        // 5  open tracks for the free high rows, in row order, while the sequence has room
        for (int base = 0; base < n_rows; base += 64) {
            const int r = base + lane;
            const bool take = r < n_rows && (L.Ri[r] & 3) == R_HIGH && L.Rs[r] >= open_thresh;
            const unsigned long long m = __ballot(take);
            const int pre = __popcll(m & below), i = n_live + pre;
            if (take && i < M) {
                float z[4], p2, v2;
                measure(L.Rbox[r], z);
                noise(z[3], 2.f, 10.f, p2, v2);
                TI(0, i) = next_id + pre;
                TI(1, i) = L.Ri[r] >> 2;
                TI(2, i) = frame == 1 ? T_TRACKED : T_NEW;
                TI(3, i) = frame;
                TF(0, i) = L.Rs[r];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    TF(1 + k, i) = z[k];
                    TF(5 + k, i) = 0.f;
                    TF(9 + k, i) = k == 2 ? AP2 : p2;
                    TF(13 + k, i) = 0.f;
                    TF(17 + k, i) = k == 2 ? AV2 : v2;
                }
            }
            const int cnt = __popcll(m), opened = min(cnt, M - n_live);
            overflow += cnt - opened;
            n_live += opened;
            next_id += opened;
        }
        __syncthreads();
        // 6  the frame's rows: the tracks matched in it, in id order
        int n_out = 0;
        for (int base = 0; base < n_live; base += 64) {
            const int i = base + lane;
            const bool emit = i < n_live && TI(2, i) == T_TRACKED && TI(3, i) == frame;
            const int pos = ballot_slot(emit, below, n_out);
            if (emit && pos < cap) {
                const float4 b = box_of(TF(1, i), TF(2, i), TF(3, i), TF(4, i));
                const size_t at = (size_t)f * cap + pos;
                float *d = out + at * 6;
                d[0] = b.x;
                d[1] = b.y;
                d[2] = b.z;
                d[3] = b.w;
                d[4] = TF(0, i);
                d[5] = (float)TI(1, i);
                out_ids[at] = TI(0, i);
                if (draw) {
                    float *g = draw + at * 6;
                    g[0] = b.x;
                    g[1] = b.y;
                    g[2] = b.z;
                    g[3] = b.w;
                    g[4] = TF(0, i);
                    g[5] = (float)(TI(0, i) % 100);
                }
            }
        }
        if (lane == 0) out_counts[f] = min(n_out, cap);
        __syncthreads();
    }

    for (int f = 0; f < YK_TRACK_WORDS; ++f)
        for (int i = lane; i < n_live; i += 64) mine[YK_TRACK_HEADER + f * M + i] = Ti[f * M + i];
    if (lane == 0) {
        mine[0] = n_live;
        mine[1] = next_id;
        mine[2] = frame;
        mine[3] = overflow;
    }
}

__global__ void __launch_bounds__(64) track_reset_kernel(int32_t *__restrict__ state, int n_seq, size_t words) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < n_seq) {
        int32_t *mine = state + (size_t)s * words;
        mine[0] = 0;
        mine[1] = 1;
        mine[2] = 0;
        mine[3] = 0;
    }
}

static size_t track_words(int max_tracks) { return YK_TRACK_HEADER + YK_TRACK_WORDS * (size_t)max_tracks; }

// what one workgroup may ask for on `dev`, never more than the architecture's 160 KB
static long long track_lds_bytes(int dev) {
    int bytes = 0;
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || bytes < 64 * 1024) bytes = 64 * 1024;
    return bytes > YK_TRACK_LDS_LIMIT ? YK_TRACK_LDS_LIMIT : bytes;
}

#define YK_TRACK_REFUSE(fn, cond, ...)          \
    if (cond) {                                 \
        yk_set_error(fn ": " __VA_ARGS__);      \
        return YK_ERR_ARG;                      \
    }
#define YK_TRACK_STATE_ARGS(fn)                                                                                                           \
    YK_TRACK_REFUSE(fn, n_seq <= 0, "n_seq %d: expected at least 1", n_seq)                                                               \
    YK_TRACK_REFUSE(fn, max_tracks <= 0 || max_tracks > YK_TRACK_MAX_TRACKS, "max_tracks %d: expected 1 .. %d (a sequence's tracks live in LDS)", \
                    max_tracks, YK_TRACK_MAX_TRACKS)

extern "C" int yk_track_state_bytes(int n_seq, int max_tracks, size_t *bytes) {
    YK_TRACK_STATE_ARGS("yk_track_state_bytes")
    YK_TRACK_REFUSE("yk_track_state_bytes", !bytes, "bytes is NULL")
    *bytes = (size_t)n_seq * track_words(max_tracks) * sizeof(int32_t);
    return YK_OK;
}

extern "C" int yk_track_reset(void *d_state, int n_seq, int max_tracks, void *stream) {
    YK_TRACK_REFUSE("yk_track_reset", !d_state, "d_state is NULL")
    YK_TRACK_STATE_ARGS("yk_track_reset")
    hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int32_t *)d_state, n_seq,
                       track_words(max_tracks));
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// LDS bytes per track and per row of a call under `assign`
static int track_per_track(int assign) { return YK_TRACK_LDS_PER_TRACK + (assign == YK_TRACK_ASSIGN_LAP ? YK_TRACK_LAP_LDS_PER_TRACK : 0); }
static int track_per_row(int assign) { return YK_TRACK_LDS_PER_ROW + (assign == YK_TRACK_ASSIGN_LAP ? YK_TRACK_LAP_LDS_PER_ROW : 0); }

// fn: the entry point the refusal names
static int track_max_cap(const char *fn, int max_tracks, int assign) {
    if (max_tracks <= 0 || max_tracks > YK_TRACK_MAX_TRACKS) {
        yk_set_error("%s: max_tracks %d: expected 1 .. %d", fn, max_tracks, YK_TRACK_MAX_TRACKS);
        return YK_ERR_ARG;
    }
    if (assign != YK_TRACK_ASSIGN_GREEDY && assign != YK_TRACK_ASSIGN_LAP) {
        yk_set_error("%s: assign %d: expected YK_TRACK_ASSIGN_GREEDY (%d) or YK_TRACK_ASSIGN_LAP (%d)", fn, assign, YK_TRACK_ASSIGN_GREEDY,
                     YK_TRACK_ASSIGN_LAP);
        return YK_ERR_ARG;
    }
    const int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("%s: no HIP device", fn);
        return YK_ERR_NO_DEVICE;
    }
    const long long room = track_lds_bytes(dev) - (long long)track_per_track(assign) * max_tracks;
    return room <= 0 ? 0 : (int)(room / track_per_row(assign));
}

extern "C" int yk_track_max_cap(int max_tracks) { return track_max_cap("yk_track_max_cap", max_tracks, YK_TRACK_ASSIGN_GREEDY); }

extern "C" int yk_track_max_cap_ex(int max_tracks, int assign) { return track_max_cap("yk_track_max_cap_ex", max_tracks, assign); }

extern "C" int yk_track_update_gmc(void *d_state, int n_seq, int max_tracks, const float *d_dets, const int32_t *d_counts, int cap,
                                   const int32_t *d_seq_first, int n_frames, int class_num, const yk_track_cfg_t *cfg, int assign,
                                   int fuse_score, const float *d_motion, float *d_out, int32_t *d_out_ids, int32_t *d_out_counts, float *d_draw,
                                   void *stream) {
#define R(cond, ...) YK_TRACK_REFUSE("yk_track_update", cond, __VA_ARGS__)
    R(!d_state, "d_state is NULL")
    YK_TRACK_STATE_ARGS("yk_track_update")
    R(assign != YK_TRACK_ASSIGN_GREEDY && assign != YK_TRACK_ASSIGN_LAP, "assign %d: expected YK_TRACK_ASSIGN_GREEDY (%d) or YK_TRACK_ASSIGN_LAP (%d)",
      assign, YK_TRACK_ASSIGN_GREEDY, YK_TRACK_ASSIGN_LAP)
    R(fuse_score != 0 && fuse_score != 1, "fuse_score %d: expected 0 or 1", fuse_score)
    R(!d_dets, "d_dets is NULL")
    R(!d_counts, "d_counts is NULL")
    R(!d_seq_first, "d_seq_first is NULL")
    R(!cfg, "cfg is NULL")
    R(!d_out, "d_out is NULL")
    R(!d_out_ids, "d_out_ids is NULL")
    R(!d_out_counts, "d_out_counts is NULL")
    R(cap <= 0, "cap %d: expected at least 1", cap)
    R(n_frames <= 0, "n_frames %d: expected at least 1", n_frames)
    R(class_num <= 0 || class_num > (1 << 24), "class_num %d: expected 1 .. 2^24", class_num)
    R(cfg->track_thresh != cfg->track_thresh, "cfg->track_thresh is NaN")
    R(cfg->low_thresh != cfg->low_thresh, "cfg->low_thresh is NaN")
    R(cfg->match_thresh != cfg->match_thresh, "cfg->match_thresh is NaN")
    R(cfg->track_buffer < 0, "cfg->track_buffer %d: expected a number of frames >= 0", cfg->track_buffer)
    R((long long)n_frames * cap > 0x7fffffffLL, "n_frames %d x cap %d: 2^31 rows or more", n_frames, cap)
    const int max_cap = track_max_cap("yk_track_update", max_tracks, assign);
    if (max_cap < 0) return max_cap;
    R(cap > max_cap, "cap %d: beside max_tracks %d the device holds %d rows of a frame in LDS (%s)", cap, max_tracks, max_cap,
      assign == YK_TRACK_ASSIGN_LAP ? "yk_track_max_cap_ex, assign lap" : "yk_track_max_cap")
#undef R
    const size_t lds = (size_t)track_per_track(assign) * max_tracks + (size_t)track_per_row(assign) * cap;
    auto go = [&](auto kern) {
        yk_launch_lds(kern, dim3((unsigned)n_seq), dim3(64), lds, (hipStream_t)stream, (int32_t *)d_state, max_tracks, d_dets, d_counts, cap,
                      d_seq_first, n_frames, class_num, cfg->track_thresh, cfg->low_thresh, 1.f - cfg->match_thresh, cfg->track_thresh + 0.1f,
                      cfg->track_buffer, d_out, d_out_ids, d_out_counts, d_draw, d_motion);
    };
    if (assign == YK_TRACK_ASSIGN_LAP) {
        if (fuse_score) go(track_update_kernel<YK_TRACK_ASSIGN_LAP, true>);
        else go(track_update_kernel<YK_TRACK_ASSIGN_LAP, false>);
    } else {
        if (fuse_score) go(track_update_kernel<YK_TRACK_ASSIGN_GREEDY, true>);
        else go(track_update_kernel<YK_TRACK_ASSIGN_GREEDY, false>);
    }
    YK_HIP(hipGetLastError());
    return YK_OK;
}

extern "C" int yk_track_update_ex(void *d_state, int n_seq, int max_tracks, const float *d_dets, const int32_t *d_counts, int cap,
                                  const int32_t *d_seq_first, int n_frames, int class_num, const yk_track_cfg_t *cfg, int assign,
                                  int fuse_score, float *d_out, int32_t *d_out_ids, int32_t *d_out_counts, float *d_draw, void *stream) {
    return yk_track_update_gmc(d_state, n_seq, max_tracks, d_dets, d_counts, cap, d_seq_first, n_frames, class_num, cfg, assign, fuse_score, nullptr,
                               d_out, d_out_ids, d_out_counts, d_draw, stream);
}

extern "C" int yk_track_update(void *d_state, int n_seq, int max_tracks, const float *d_dets, const int32_t *d_counts, int cap,
                               const int32_t *d_seq_first, int n_frames, int class_num, const yk_track_cfg_t *cfg, float *d_out,
                               int32_t *d_out_ids, int32_t *d_out_counts, float *d_draw, void *stream) {
    return yk_track_update_ex(d_state, n_seq, max_tracks, d_dets, d_counts, cap, d_seq_first, n_frames, class_num, cfg, YK_TRACK_ASSIGN_GREEDY, 0,
                              d_out, d_out_ids, d_out_counts, d_draw, stream);
}

extern "C" int yk_track_read(const void *d_state, int n_seq, int max_tracks, int32_t *h_live, int32_t *h_next_id, int32_t *h_overflow) {
    YK_TRACK_REFUSE("yk_track_read", !d_state, "d_state is NULL")
    YK_TRACK_STATE_ARGS("yk_track_read")
    YK_TRACK_REFUSE("yk_track_read", !h_live || !h_next_id || !h_overflow, "h_live, h_next_id and h_overflow are all needed")
    std::vector<int32_t> head((size_t)n_seq * YK_TRACK_HEADER);
    YK_HIP(hipDeviceSynchronize());
    YK_HIP(hipMemcpy2D(head.data(), YK_TRACK_HEADER * sizeof(int32_t), d_state, track_words(max_tracks) * sizeof(int32_t),
                       YK_TRACK_HEADER * sizeof(int32_t), (size_t)n_seq, hipMemcpyDeviceToHost));
    for (int s = 0; s < n_seq; ++s) {
        h_live[s] = head[(size_t)s * YK_TRACK_HEADER];
        h_next_id[s] = head[(size_t)s * YK_TRACK_HEADER + 1];
        h_overflow[s] = head[(size_t)s * YK_TRACK_HEADER + 3];
    }
    return YK_OK;
}
