// yk_tta.hip — test-time augmentation, the fusion of the views' rows (k210_yolo_framework_amd/tta.py states the rule).
//
// The decode leaves one padded row set per FRAME; with test-time augmentation a picture is `views` frames.  yk_fuse_views turns the rows of a
// picture's frames into one padded row set per PICTURE by Weighted Boxes Fusion: every row mapped back into the picture (un-mirrored, moved),
// then per (picture, class) the candidates walked by score against a growing list of clusters, each candidate joining the cluster whose fused
// box it overlaps most or opening its own, then the decode's own class-major compaction - so the draw, the evaluator and the copies
// downstream read what they always read.
//
// Two launches: fuse_views_kernel (one wavefront per (picture, class); everything of the class lives in LDS) -> fuse_compact_kernel.
// Compiled with -ffp-contract=off: one rounding per operation, as tta.py's float32 steps.
#include "yk_common.h"
#include "yk_nms.h"

// LDS per candidate: its mapped box (16), the box and the four weighted sums of the cluster it may open (16 + 16), its score and row before
// the sort (4 + 4), its score after (4), the cluster's weight and member count (4 + 4)
#define YK_TTA_LDS_PER_CAND 68
#define YK_TTA_LDS_LIMIT (160 * 1024)

// row `ref` (= frame * cap + row) of d_dets mapped back into its picture
__device__ __forceinline__ float4 view_box(const float *__restrict__ dets, const float *__restrict__ xform, int cap, int ref) {
    const float *r = dets + (size_t)ref * 6;
    const float *x = xform + 3 * (size_t)(ref / cap);
    const float dy = x[0], dx = x[1], mw = x[2];
    float top = r[0], left = r[1], bottom = r[2], right = r[3];
    if (mw >= 0.f) {
        const float l = mw - right, rr = mw - left;
        left = l;
        right = rr;
    }
    return make_float4(top + dy, left + dx, bottom + dy, right + dx);
}

// position of entry i of v[0 .. n) in the order (value descending, index ascending): every lane reads the same v[j], a broadcast
__device__ __forceinline__ int rank_of(const float *v, int n, int i) {
    const float s = v[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float o = v[j];
        rank += (o > s || (o == s && j < i)) ? 1 : 0;
    }
    return rank;
}

// grid (n_pics * C), one wavefront; dynamic LDS: YK_TTA_LDS_PER_CAND bytes for each of nmax = views * max_out candidates.
//   1  the rows of the picture's frames in candidate order, those of this class compacted by ballot into (Us, Uref)
//   2  in-wave rank sort: lane l ranks the entries i = l mod 64 and scatters score and mapped box to their places (Cs, Cbox)
//   3  the walk, one candidate at a time: the lanes share the clusters (k = l mod 64), a wave reduction finds (largest IoU, lowest index), lane
//      0 updates or opens the cluster; the barrier publishes it to the next candidate
//   4  final scores into Us, ranked again; the first max_out go to `stage` in their order
__global__ void __launch_bounds__(64) fuse_views_kernel(const float *__restrict__ dets, const int32_t *__restrict__ counts,
                                                        const float *__restrict__ xform, int views, int C, int max_out, float thresh, int nmax,
                                                        float *__restrict__ stage, int *__restrict__ cnt_out) {
    extern __shared__ float4 lds_raw[];
    float4 *Cbox = lds_raw;                                              // [nmax] candidates in walk order
    float4 *Kbox = Cbox + nmax;                                          // [nmax] clusters: the current fused box
    float4 *Kacc = Kbox + nmax;                                          // [nmax] st, sl, sb, sr
    float *Us = reinterpret_cast<float *>(Kacc + nmax);                  // [nmax] scores in candidate order; later the clusters' final scores
    int *Uref = reinterpret_cast<int *>(Us + nmax);                      // [nmax]
    float *Cs = reinterpret_cast<float *>(Uref + nmax);                  // [nmax] scores in walk order
    float *Ksw = Cs + nmax;                                              // [nmax] sw (ss of tta.py is the same sum)
    int *Kcnt = reinterpret_cast<int *>(Ksw + nmax);                     // [nmax]
    const int p = blockIdx.x / C, c = blockIdx.x - p * C, lane = threadIdx.x;
    const int cap = C * max_out;
    const float cf = (float)c;

    int n = 0;
    for (int v = 0; v < views; ++v) {
        const int f = p * views + v;
        const int k = min(max(counts[f], 0), cap);
        for (int base = 0; base < k; base += 64) {
            const int r = base + lane;
            float sc = 0.f, cl = -1.f;
            if (r < k) {
                const float *row = dets + ((size_t)f * cap + r) * 6;
                sc = row[4];
                cl = row[5];
            }
            const bool take = r < k && cl == cf && sc > 0.f;
            const unsigned long long m = __ballot(take);
            // a frame holds at most max_out rows of a class as the decode leaves it; rows that are not decode-shaped must not leave the arrays
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
            if (take && pos < nmax) {
                Us[pos] = sc;
                Uref[pos] = f * cap + r;
            }
            n += __popcll(m);
        }
    }
    n = min(n, nmax);
    __syncthreads();

    for (int i = lane; i < n; i += 64) {
        const int rank = rank_of(Us, n, i);
        Cs[rank] = Us[i];
        Cbox[rank] = view_box(dets, xform, cap, Uref[i]);
    }
    __syncthreads();

    int nk = 0;
    for (int i = 0; i < n; ++i) {
        const float4 b = Cbox[i];
        const float s = Cs[i];
        float best = -INFINITY;
        int bidx = 0x7fffffff, bpos = -1;
        for (int k = lane; k < nk; k += 64) {
            const float o = tf_iou(b, Kbox[k]);
            if (o > best) {                                              // ascending k: a tie stays with the lower cluster
                best = o;
                bidx = bpos = k;
            }
        }
        yk_wave_argmax(best, bidx, bpos);
        const bool join = bpos >= 0 && best > thresh;
        const int k = join ? bpos : nk;
        if (lane == 0) {
            float sw = 0.f;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            int cnt = 0;
            if (join) {
                sw = Ksw[k];
                a = Kacc[k];
                cnt = Kcnt[k];
            }
            sw = sw + s;
            a.x = a.x + s * b.x;
            a.y = a.y + s * b.y;
            a.z = a.z + s * b.z;
            a.w = a.w + s * b.w;
            ++cnt;
            Ksw[k] = sw;
            Kacc[k] = a;
            Kcnt[k] = cnt;
            Kbox[k] = cnt == 1 ? b : make_float4(a.x / sw, a.y / sw, a.z / sw, a.w / sw);
        }
        if (!join) ++nk;
        __syncthreads();
    }

    const float nf = (float)views;
    for (int k = lane; k < nk; k += 64) {
        const int cnt = Kcnt[k];
        Us[k] = ((Ksw[k] / (float)cnt) * (float)min(cnt, views)) / nf;
    }
    __syncthreads();
    float *mine = stage + (size_t)blockIdx.x * max_out * 6;
    for (int k = lane; k < nk; k += 64) {
        const int rank = rank_of(Us, nk, k);
        if (rank < max_out) {
            const float4 bb = Kbox[k];
            float *d = mine + (size_t)rank * 6;
            d[0] = bb.x;
            d[1] = bb.y;
            d[2] = bb.z;
            d[3] = bb.w;
            d[4] = Us[k];
            d[5] = cf;
        }
    }
    if (lane == 0) cnt_out[blockIdx.x] = min(nk, max_out);
}

// grid (n_pics), 256 threads: the class-major concatenation of compact_py_kernel over the staged rows
__global__ void __launch_bounds__(256) fuse_compact_kernel(const float *__restrict__ stage, const int *__restrict__ cnt, int C, int max_out,
                                                          float *__restrict__ out, int32_t *__restrict__ out_counts) {
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
            const float *s = stage + ((size_t)p * cap + slot) * 6;
            float *d = out + ((size_t)p * cap + base[c] + j) * 6;
#pragma unroll
            for (int e = 0; e < 6; ++e) d[e] = s[e];
        }
    }
}

// what one workgroup may ask for on `dev`, never more than the architecture's 160 KB
static int fuse_lds_candidates(int dev) {
    int bytes = 0;
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || bytes < 64 * 1024) bytes = 64 * 1024;
    if (bytes > YK_TTA_LDS_LIMIT) bytes = YK_TTA_LDS_LIMIT;
    return bytes / YK_TTA_LDS_PER_CAND / 64 * 64;
}

extern "C" int yk_fuse_views_lds_candidates(int max_out) {
    if (max_out <= 0) {
        yk_set_error("yk_fuse_views_lds_candidates: max_out %d: expected a positive number", max_out);
        return YK_ERR_ARG;
    }
    const int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("yk_fuse_views_lds_candidates: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    return fuse_lds_candidates(dev);
}

extern "C" int yk_fuse_views(const float *d_dets, const int32_t *d_counts, const float *d_xform, int views, int n_pics, int class_num,
                             int max_out, float thresh, float *d_out, int32_t *d_out_counts, void *stream) {
#define YK_FUSE_REFUSE(cond, ...)                    \
    if (cond) {                                      \
        yk_set_error("yk_fuse_views: " __VA_ARGS__); \
        return YK_ERR_ARG;                           \
    }
    YK_FUSE_REFUSE(!d_dets, "d_dets is NULL")
    YK_FUSE_REFUSE(!d_counts, "d_counts is NULL")
    YK_FUSE_REFUSE(!d_xform, "d_xform is NULL")
    YK_FUSE_REFUSE(!d_out, "d_out is NULL")
    YK_FUSE_REFUSE(!d_out_counts, "d_out_counts is NULL")
    YK_FUSE_REFUSE(views <= 0 || views > YK_TTA_MAX_VIEWS, "views %d: expected 1 .. %d", views, YK_TTA_MAX_VIEWS)
    YK_FUSE_REFUSE(n_pics <= 0, "n_pics %d: expected at least 1", n_pics)
    YK_FUSE_REFUSE(class_num <= 0, "class_num %d: expected at least 1", class_num)
    YK_FUSE_REFUSE(max_out <= 0, "max_out %d: expected at least 1", max_out)
    YK_FUSE_REFUSE(!(thresh >= 0.f), "thresh %g: expected a number >= 0", (double)thresh)
    const long long lim = 0x7fffffffLL;
    YK_FUSE_REFUSE((long long)class_num * max_out > lim || (long long)n_pics * views > lim ||
                       (long long)n_pics * views * ((long long)class_num * max_out) > lim,
                   "n_pics %d x views %d x class_num %d x max_out %d: 2^31 input rows or more", n_pics, views, class_num, max_out)
    const int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("yk_fuse_views: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    const int lds_cap = fuse_lds_candidates(dev);
    YK_FUSE_REFUSE((long long)views * max_out > lds_cap,
                   "views %d x max_out %d = %lld candidates per class, the device holds %d in LDS (views * max_out <= yk_fuse_views_lds_candidates)",
                   views, max_out, (long long)views * max_out, lds_cap)
#undef YK_FUSE_REFUSE
    const size_t stage_b = (size_t)n_pics * class_num * max_out * 6 * sizeof(float), cnt_b = (size_t)n_pics * class_num * sizeof(int);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    char *ws = (char *)yk_scratch(dev, stream, YK_SLOT_TTA, up(stage_b) + up(cnt_b));
    if (!ws) return YK_ERR_NOMEM;
    float *stage = (float *)ws;
    int *cnt = (int *)(ws + up(stage_b));
    hipStream_t st = (hipStream_t)stream;
    const int nmax = views * max_out;
    yk_launch_lds(fuse_views_kernel, dim3((unsigned)(n_pics * class_num)), dim3(64), (size_t)nmax * YK_TTA_LDS_PER_CAND, st, d_dets, d_counts, d_xform,
                  views, class_num, max_out, thresh, nmax, stage, cnt);
    hipLaunchKernelGGL(fuse_compact_kernel, dim3((unsigned)n_pics), dim3(256), ((size_t)class_num + 1) * sizeof(int), st, stage, cnt, class_num, max_out,
                       d_out, d_out_counts);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
