// yk_tiles.hip — sliced inference, the cross-tile merge (k210_yolo_framework_amd/tiles.py states the rule).
//
// The decode leaves one padded row set per FRAME; with tiles a picture is several frames.  yk_merge_tiles turns the rows of a picture's
// tile frames into one padded row set per PICTURE: every row moved back by its tile's origin (one float add per coordinate), then per
// (picture, class) a greedy hard NMS over all of them, then the decode's own class-major compaction - so the draw, the evaluator and the
// copies downstream read what they always read.
//
// Two launches: merge_tiles_kernel (one wavefront per (picture, class), structured like softnms_py_kernel: iterated arg-max, lane l owns
// the entries i = l mod 64 and is the only one to touch their scores between the barriers) -> merge_compact_kernel.
// Compiled with -ffp-contract=off: one rounding per operation, as tiles.py's float32 steps.
#include "yk_common.h"
#include "yk_nms.h"

#define YK_TILES_MAXC 2048 /* candidates of one (picture, class) held in LDS (24 bytes each: 48 KB, under the default limit) */

template <int METRIC>
__device__ __forceinline__ float tile_match(const float4 &i, const float4 &j) {
    if (METRIC == YK_MATCH_IOU) return tf_iou(i, j);
    // the intersection of tf_iou over the smaller area
    const float ymin_i = fminf(i.x, i.z), xmin_i = fminf(i.y, i.w), ymax_i = fmaxf(i.x, i.z), xmax_i = fmaxf(i.y, i.w);
    const float ymin_j = fminf(j.x, j.z), xmin_j = fminf(j.y, j.w), ymax_j = fmaxf(j.x, j.z), xmax_j = fmaxf(j.y, j.w);
    const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
    const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
    const float small = fminf(area_i, area_j);
    if (!(small > 0.f)) return 0.f;
    const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
    const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
    const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
    return inter / small;
}

// row `ref` (= tile * cap + row) of d_dets moved back by its tile's origin
__device__ __forceinline__ float4 tile_box(const float *__restrict__ dets, const float *__restrict__ origin, int cap, int ref) {
    const float *r = dets + (size_t)ref * 6;
    const int t = ref / cap;
    const float y0 = origin[2 * (size_t)t], x0 = origin[2 * (size_t)t + 1];
    return make_float4(r[0] + y0, r[1] + x0, r[2] + y0, r[3] + x0);
}

// The rounds over `count` entries in ascending candidate order: score(i) the score (a reference; -inf: retired), box_of(i) the translated box.
// A tie stays with the lower position, which is the lower candidate index.  sel[k] receives ref_of(position) of the k-th kept candidate.
template <int METRIC, class ScoreOf, class BoxOf, class RefOf>
__device__ __forceinline__ int merge_rounds(int count, ScoreOf score, BoxOf box_of, RefOf ref_of, float thresh, int max_out, int *sel) {
    const int lane = threadIdx.x;
    int kept = 0;
    while (kept < max_out) {
        float best = -INFINITY;
        int bidx = 0x7fffffff, bpos = -1;
        for (int i = lane; i < count; i += 64) {
            const float v = score(i);
            if (v > -INFINITY && (bpos < 0 || v > best)) {             // ascending i: a tie stays with the lower position
                best = v;
                bpos = i;
            }
        }
        if (bpos >= 0) bidx = bpos;
        yk_wave_argmax(best, bidx, bpos);
        if (bpos < 0) break;
        if (lane == 0) sel[kept] = ref_of(bpos);
        ++kept;
        if (kept >= max_out) break;
        const float4 mb = box_of(bpos);
        for (int i = lane; i < count; i += 64) {
            float &v = score(i);
            if (i == bpos || (v > -INFINITY && tile_match<METRIC>(mb, box_of(i)) > thresh)) v = -INFINITY;
        }
    }
    return kept;
}

struct merge_entry {
    float s;
    int ref;
};

// grid (n_pics * C), one wavefront; dynamic LDS: lds_cap candidates of { float s; int ref; float4 box }.
// Pass 1 walks the rows of the picture's tiles in candidate order and compacts the ones of this class by ballot: into LDS while they fit,
// always counted.  More than lds_cap: the wave takes a segment of the picture's region of `list` (atomicAdd on the picture's cursor - the
// segments of a picture's classes are disjoint and together no longer than its rows, wherever each one lands) and pass 2 writes the same
// compaction there; the rounds then read boxes from d_dets.
template <int METRIC>
__global__ void __launch_bounds__(64) merge_tiles_kernel(const float *__restrict__ dets, const int32_t *__restrict__ counts,
                                                         const float *__restrict__ origin, const int32_t *__restrict__ first, int n_tiles, int C,
                                                         int max_out, float thresh, int lds_cap, int *cursor, merge_entry *list,
                                                         int *__restrict__ sel, int *__restrict__ cnt) {
    extern __shared__ float4 lds_raw[];
    float4 *Lbox = lds_raw;                                              // [lds_cap]
    float *Ls = reinterpret_cast<float *>(lds_raw + lds_cap);            // [lds_cap]
    int *Lref = reinterpret_cast<int *>(Ls + lds_cap);                   // [lds_cap]
    const int p = blockIdx.x / C, c = blockIdx.x - p * C, lane = threadIdx.x;
    const int cap = C * max_out;
    const int t0 = min(max(first[p], 0), n_tiles), t1 = min(max(first[p + 1], 0), n_tiles);
    const float cf = (float)c;
    int *my_sel = sel + (size_t)blockIdx.x * max_out;

    auto scan = [&](auto put) {                                          // put(position, score, ref) for every candidate of this class, in order
        int n = 0;
        for (int t = t0; t < t1; ++t) {
            const int k = min(max(counts[t], 0), cap);
            for (int base = 0; base < k; base += 64) {
                const int r = base + lane;
                float sc = -INFINITY, cl = -1.f;
                if (r < k) {
                    const float *row = dets + ((size_t)t * cap + r) * 6;
                    sc = row[4];
                    cl = row[5];
                }
                const bool f = r < k && cl == cf && sc > -INFINITY;
                const unsigned long long m = __ballot(f);
                if (f) put(n + __popcll(m & ((1ull << lane) - 1ull)), sc, t * cap + r);
                n += __popcll(m);
            }
        }
        return n;
    };

    const int n = scan([&](int pos, float sc, int ref) {
        if (pos < lds_cap) {
            Ls[pos] = sc;
            Lref[pos] = ref;
            Lbox[pos] = tile_box(dets, origin, cap, ref);
        }
    });
    int kept;
    if (n <= lds_cap) {
        __syncthreads();
        kept = merge_rounds<METRIC>(
            n, [&](int i) -> float & { return Ls[i]; }, [&](int i) { return Lbox[i]; }, [&](int i) { return Lref[i]; }, thresh, max_out, my_sel);
    } else {
        int seg = 0;
        if (lane == 0) seg = atomicAdd(cursor + p, n);
        seg = __shfl(seg, 0, 64);
        merge_entry *mine = list + (size_t)t0 * cap + seg;
        scan([&](int pos, float sc, int ref) {
            mine[pos].s = sc;
            mine[pos].ref = ref;
        });
        __threadfence_block();
        __syncthreads();
        kept = merge_rounds<METRIC>(
            n, [&](int i) -> float & { return mine[i].s; }, [&](int i) { return tile_box(dets, origin, cap, mine[i].ref); },
            [&](int i) { return mine[i].ref; }, thresh, max_out, my_sel);
    }
    if (lane == 0) cnt[blockIdx.x] = kept;
}

// grid (n_pics), 256 threads: the class-major concatenation of compact_py_kernel, rows fetched through their refs and moved back again
__global__ void __launch_bounds__(256) merge_compact_kernel(const float *__restrict__ dets, const float *__restrict__ origin, int C, int max_out,
                                                           const int *__restrict__ sel, const int *__restrict__ cnt, float *__restrict__ out,
                                                           int32_t *__restrict__ out_counts) {
    extern __shared__ int base[];                   // [C + 1] exclusive prefix of the per-class counts
    const int p = blockIdx.x, tid = threadIdx.x;
    const int cap = C * max_out;
    if (tid == 0) {
        int acc = 0;
        for (int c = 0; c < C; ++c) {
            base[c] = acc;
            acc += cnt[(size_t)p * C + c];
        }
        base[C] = acc;
        out_counts[p] = acc;
    }
    __syncthreads();
    for (int slot = tid; slot < cap; slot += 256) {
        const int c = slot / max_out, j = slot - c * max_out;
        if (j < base[c + 1] - base[c]) {
            const int ref = sel[((size_t)p * C + c) * max_out + j];
            const float4 bb = tile_box(dets, origin, cap, ref);
            const float *r = dets + (size_t)ref * 6;
            float *d = out + ((size_t)p * cap + base[c] + j) * 6;
            d[0] = bb.x;
            d[1] = bb.y;
            d[2] = bb.z;
            d[3] = bb.w;
            d[4] = r[4];
            d[5] = r[5];
        }
    }
}

static int merge_lds_candidates(int n_tiles, int n_pics, int max_out) {
    // no (picture, class) of rows as the decode leaves them has more than (tiles of the largest possible picture) * max_out candidates
    const long long most = (long long)(n_tiles - (n_pics - 1) > 1 ? n_tiles - (n_pics - 1) : 1) * max_out;
    const long long up = (most + 63) / 64 * 64;
    return (int)(up < YK_TILES_MAXC ? up : YK_TILES_MAXC);
}

extern "C" int yk_merge_tiles_lds_candidates(int n_tiles, int n_pics, int max_out) {
    if (n_tiles <= 0 || n_pics <= 0 || max_out <= 0) {
        yk_set_error("yk_merge_tiles_lds_candidates: n_tiles %d, n_pics %d, max_out %d: expected positive numbers", n_tiles, n_pics, max_out);
        return YK_ERR_ARG;
    }
    return merge_lds_candidates(n_tiles, n_pics, max_out);
}

extern "C" int yk_merge_tiles(const float *d_dets, const int32_t *d_counts, const float *d_origin, const int32_t *d_first, int n_tiles,
                              int n_pics, int class_num, int max_out, float thresh, int metric, float *d_out, int32_t *d_out_counts,
                              void *stream) {
#define YK_MERGE_REFUSE(cond, ...)                  \
    if (cond) {                                     \
        yk_set_error("yk_merge_tiles: " __VA_ARGS__); \
        return YK_ERR_ARG;                          \
    }
    YK_MERGE_REFUSE(!d_dets, "d_dets is NULL")
    YK_MERGE_REFUSE(!d_counts, "d_counts is NULL")
    YK_MERGE_REFUSE(!d_origin, "d_origin is NULL")
    YK_MERGE_REFUSE(!d_first, "d_first is NULL")
    YK_MERGE_REFUSE(!d_out, "d_out is NULL")
    YK_MERGE_REFUSE(!d_out_counts, "d_out_counts is NULL")
    YK_MERGE_REFUSE(n_tiles <= 0, "n_tiles %d: expected at least 1", n_tiles)
    YK_MERGE_REFUSE(n_pics <= 0, "n_pics %d: expected at least 1", n_pics)
    YK_MERGE_REFUSE(class_num <= 0, "class_num %d: expected at least 1", class_num)
    YK_MERGE_REFUSE(max_out <= 0, "max_out %d: expected at least 1", max_out)
    YK_MERGE_REFUSE(thresh != thresh, "thresh is not a number")
    YK_MERGE_REFUSE(metric != YK_MATCH_IOU && metric != YK_MATCH_IOS, "metric %d: expected YK_MATCH_IOU or YK_MATCH_IOS", metric)
    const long long lim = 0x7fffffffLL;
    YK_MERGE_REFUSE((long long)class_num * max_out > lim || (long long)n_tiles * class_num * max_out > lim,
                    "n_tiles %d x class_num %d x max_out %d: 2^31 input rows or more", n_tiles, class_num, max_out)
    YK_MERGE_REFUSE((long long)n_pics * class_num * max_out > lim, "n_pics %d x class_num %d x max_out %d: 2^31 output rows or more", n_pics,
                    class_num, max_out)
#undef YK_MERGE_REFUSE
    const int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("yk_merge_tiles: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    const size_t rows_in = (size_t)n_tiles * class_num * max_out;
    const size_t cur_b = (size_t)n_pics * sizeof(int), list_b = rows_in * sizeof(merge_entry);
    const size_t sel_b = (size_t)n_pics * class_num * max_out * sizeof(int), cnt_b = (size_t)n_pics * class_num * sizeof(int);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char *ws = (char *)yk_scratch(dev, stream, YK_SLOT_TILES, up(cur_b) + up(list_b) + up(sel_b) + up(cnt_b));
    if (!ws) return YK_ERR_NOMEM;
    int *cursor = (int *)ws;
    merge_entry *list = (merge_entry *)(ws + up(cur_b));
    int *sel = (int *)(ws + up(cur_b) + up(list_b));
    int *cnt = (int *)(ws + up(cur_b) + up(list_b) + up(sel_b));
    hipStream_t st = (hipStream_t)stream;
    YK_HIP(hipMemsetAsync(cursor, 0, cur_b, st));
    const int lds_cap = merge_lds_candidates(n_tiles, n_pics, max_out);
    const size_t lds = (size_t)lds_cap * (sizeof(float4) + sizeof(float) + sizeof(int));
    const dim3 grid((unsigned)(n_pics * class_num));
    if (metric == YK_MATCH_IOU)
        yk_launch_lds(merge_tiles_kernel<YK_MATCH_IOU>, grid, dim3(64), lds, st, d_dets, d_counts, d_origin, d_first, n_tiles, class_num, max_out,
                      thresh, lds_cap, cursor, list, sel, cnt);
    else
        yk_launch_lds(merge_tiles_kernel<YK_MATCH_IOS>, grid, dim3(64), lds, st, d_dets, d_counts, d_origin, d_first, n_tiles, class_num, max_out,
                      thresh, lds_cap, cursor, list, sel, cnt);
    hipLaunchKernelGGL(merge_compact_kernel, dim3((unsigned)n_pics), dim3(256), ((size_t)class_num + 1) * sizeof(int), st, d_dets, d_origin, class_num,
                       max_out, sel, cnt, d_out, d_out_counts);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
