// yk_kmeans.hip — anchor k-means with many restarts in one call (datatools.run_kmeans for every restart).
//
// Boxes are (w, h) pairs centred at the origin, the distance is 1 - IoU, everything is float64 in datatools.fake_iou_distance's
// operation order with contraction off, so an assignment is the one numpy makes.  One iteration is two launches:
//   km_assign_kernel<false>  one workgroup per (tile of YK_KMEANS_TILE boxes, restart): the restart's k centroids in LDS, two boxes per
//                            lane read as double2, argmin with the lowest index winning a tie; then per cluster the tile's sum of w, of h
//                            and its member count: a butterfly over the wave, the four waves folded in wave order.  Nothing is added
//                            with an atomic, so the order of every sum is fixed by (n, k) alone.
//   km_update_kernel         one workgroup per restart: folds the tiles (lane-strided, then the same butterfly), divides, writes the
//                            centroids and the counts; a cluster without members makes its row NaN and flags the restart, whose
//                            workgroups leave at once from then on.
// After the last update km_assign_kernel<true> sums the best IoU of every box per tile and km_score_kernel folds it into the mean.
// The kernel boundary is the only synchronisation between workgroups: no workgroup ever waits for another.
//
// At the sizes of an anchor search (4e4 boxes, 6 .. 9 centroids, 256 starts, 10 iterations: 1e9 distances, 0.6 MB of boxes that stay in L2)
// the call is bound by float64 vector arithmetic - the division of every distance above all - on top of about 12 us for each of its
// 2 * iters + 2 dependent launches; with few starts those launches are all there is (profiles/anchor_kmeans_rate.txt).
#include "yk_common.h"

#pragma clang fp contract(off)

#define YK_KMEANS_MAX_K 32
#define YK_KMEANS_MAX_N (1ll << 24)
#define YK_KMEANS_MAX_RESTARTS 4096
#define YK_KMEANS_MAX_ITERS 1000
#define YK_KMEANS_THREADS 256
#define YK_KMEANS_BOXES 2 /* per lane */
#define YK_KMEANS_TILE (YK_KMEANS_THREADS * YK_KMEANS_BOXES)
#define YK_KMEANS_WAVES (YK_KMEANS_THREADS / YK_WAVE)

namespace {

// every lane receives the same bits: a + b == b + a at each of the six steps
__device__ __forceinline__ double km_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int km_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// datatools.fake_iou_distance for one box and one centroid
__device__ __forceinline__ double km_distance(double w, double h, double cw, double ch) {
    const double iw = fmax(fmin(w / 2., cw / 2.) - fmax(-w / 2., -cw / 2.), 0.);
    const double ih = fmax(fmin(h / 2., ch / 2.) - fmax(-h / 2., -ch / 2.), 0.);
    const double inter = iw * ih;
    return 1 - inter / (w * h + cw * ch - inter);
}

// SCORE false: part_sum [R][tiles][k][2], part_cnt [R][tiles][k], idx [R][n] or NULL.  SCORE true: part_sum [R][tiles], the rest unused.
template <bool SCORE>
__global__ void __launch_bounds__(YK_KMEANS_THREADS) km_assign_kernel(const double2 *__restrict__ x, long long n, const double *__restrict__ cent,
                                                                      int k, const int32_t *__restrict__ empty, double *__restrict__ part_sum,
                                                                      int32_t *__restrict__ part_cnt, uint8_t *__restrict__ idx) {
    __shared__ double s_c[YK_KMEANS_MAX_K * 2];
    __shared__ double s_sum[YK_KMEANS_WAVES][YK_KMEANS_MAX_K * 2];
    __shared__ int s_cnt[YK_KMEANS_WAVES][YK_KMEANS_MAX_K];
    const int tid = threadIdx.x, lane = tid & (YK_WAVE - 1), wave = tid / YK_WAVE;
    const size_t r = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    if (empty[r]) return;                                             // (the same answer in every lane of the workgroup)
    if (tid < 2 * k) s_c[tid] = cent[r * k * 2 + tid];
    __syncthreads();
    double w[YK_KMEANS_BOXES], h[YK_KMEANS_BOXES], best[YK_KMEANS_BOXES];
    int bi[YK_KMEANS_BOXES];
#pragma unroll
    for (int j = 0; j < YK_KMEANS_BOXES; ++j) {
        const long long i = (long long)tile * YK_KMEANS_TILE + j * YK_KMEANS_THREADS + tid;
        const bool in = i < n;
        const double2 b = in ? x[i] : make_double2(1., 1.);
        w[j] = b.x, h[j] = b.y;
        best[j] = km_distance(w[j], h[j], s_c[0], s_c[1]);
        bi[j] = 0;
        for (int c = 1; c < k; ++c) {
            const double d = km_distance(w[j], h[j], s_c[2 * c], s_c[2 * c + 1]);
            if (d < best[j]) best[j] = d, bi[j] = c;                  // np.argmin: the first of equal minima
        }
        if (!in) bi[j] = 0xff;                                        // member of no cluster
        if (!SCORE && idx && in) idx[(long long)r * n + i] = (uint8_t)bi[j];
    }
    if (SCORE) {
        double v = 0.;
#pragma unroll
        for (int j = 0; j < YK_KMEANS_BOXES; ++j) v = v + (bi[j] != 0xff ? 1 - best[j] : 0.);
        v = km_wave_sum(v);
        if (lane == 0) s_sum[wave][0] = v;
        __syncthreads();
        if (tid == 0) {
            double t = s_sum[0][0];
            for (int q = 1; q < YK_KMEANS_WAVES; ++q) t = t + s_sum[q][0];
            part_sum[r * tiles + tile] = t;
        }
        return;
    }
    for (int c = 0; c < k; ++c) {                                     // every lane of the wave takes every turn of this loop
        int m = 0;
        double sw = 0., sh = 0.;
#pragma unroll
        for (int j = 0; j < YK_KMEANS_BOXES; ++j) {
            const bool mine = bi[j] == c;
            m += mine;
            sw = sw + (mine ? w[j] : 0.);
            sh = sh + (mine ? h[j] : 0.);
        }
        if (__ballot(m != 0)) {                                       // a wave without a member adds exact zeros: the same bits, sooner
            sw = km_wave_sum(sw), sh = km_wave_sum(sh), m = km_wave_sum(m);
        }
        if (lane == 0) s_sum[wave][2 * c] = sw, s_sum[wave][2 * c + 1] = sh, s_cnt[wave][c] = m;
    }
    __syncthreads();
    if (tid < 2 * k) {
        double t = s_sum[0][tid];
        for (int q = 1; q < YK_KMEANS_WAVES; ++q) t = t + s_sum[q][tid];
        part_sum[(r * tiles + tile) * k * 2 + tid] = t;
    }
    if (tid < k) {
        int t = 0;
        for (int q = 0; q < YK_KMEANS_WAVES; ++q) t += s_cnt[q][tid];
        part_cnt[(r * tiles + tile) * k + tid] = t;
    }
}

__global__ void __launch_bounds__(YK_KMEANS_THREADS) km_update_kernel(const double *__restrict__ part_sum, const int32_t *__restrict__ part_cnt,
                                                                      long long tiles, int k, int iteration, double *__restrict__ cent,
                                                                      int32_t *__restrict__ counts, int32_t *__restrict__ empty) {
    __shared__ double s_sum[YK_KMEANS_MAX_K * 2];
    __shared__ int s_cnt[YK_KMEANS_MAX_K];
    const int tid = threadIdx.x, lane = tid & (YK_WAVE - 1), wave = tid / YK_WAVE;
    const size_t r = blockIdx.x;
    if (empty[r]) return;
    const double *ps = part_sum + r * tiles * k * 2;
    const int32_t *pc = part_cnt + r * tiles * k;
    for (int j = wave; j < 3 * k; j += YK_KMEANS_WAVES) {             // 2k sums, then k counts; a wave per value, tiles over the lanes
        if (j < 2 * k) {
            double a = 0.;
            for (long long t = lane; t < tiles; t += YK_WAVE) a = a + ps[(size_t)t * k * 2 + j];
            a = km_wave_sum(a);
            if (lane == 0) s_sum[j] = a;
        } else {
            int a = 0;
            for (long long t = lane; t < tiles; t += YK_WAVE) a += pc[(size_t)t * k + (j - 2 * k)];
            a = km_wave_sum(a);
            if (lane == 0) s_cnt[j - 2 * k] = a;
        }
    }
    __syncthreads();                                                  // (also: every lane has read empty[r] before lane 0 writes it)
    if (tid < 2 * k) {
        const int m = s_cnt[tid >> 1];
        cent[r * k * 2 + tid] = m > 0 ? s_sum[tid] / (double)m : __builtin_nan("");
    }
    if (tid < k) counts[r * k + tid] = s_cnt[tid];
    if (tid == 0) {
        bool any = false;
        for (int c = 0; c < k; ++c) any |= s_cnt[c] == 0;
        if (any) empty[r] = iteration + 1;
    }
}

__global__ void __launch_bounds__(YK_WAVE) km_score_kernel(const double *__restrict__ part, long long tiles, long long n,
                                                           const int32_t *__restrict__ empty, double *__restrict__ score) {
    const size_t r = blockIdx.x;
    const int lane = threadIdx.x;
    double a = 0.;
    if (!empty[r])
        for (long long t = lane; t < tiles; t += YK_WAVE) a = a + part[r * tiles + t];
    a = km_wave_sum(a);
    if (lane == 0) score[r] = empty[r] ? __builtin_nan("") : a / (double)n;
}

int km_check_sizes(const char *who, long long n, int k, int restarts) {
    if (k < 1 || k > YK_KMEANS_MAX_K) {
        yk_set_error("%s: k = %d: must be in 1 .. %d", who, k, YK_KMEANS_MAX_K);
        return YK_ERR_ARG;
    }
    if (n < 1 || n > YK_KMEANS_MAX_N) {
        yk_set_error("%s: n = %lld: must be in 1 .. 2^24", who, n);
        return YK_ERR_ARG;
    }
    if (restarts < 1 || restarts > YK_KMEANS_MAX_RESTARTS) {
        yk_set_error("%s: restarts = %d: must be in 1 .. %d", who, restarts, YK_KMEANS_MAX_RESTARTS);
        return YK_ERR_ARG;
    }
    return YK_OK;
}

inline long long km_tiles(long long n) { return (n + YK_KMEANS_TILE - 1) / YK_KMEANS_TILE; }
// the partial sums (16 bytes per tile and cluster), then the partial counts (4): at most 2^12 * 2^15 * 2^5 * 20 bytes < 2^42
inline size_t km_sum_bytes(long long n, int k, int restarts) { return (size_t)restarts * (size_t)km_tiles(n) * (size_t)k * 2 * sizeof(double); }
inline size_t km_work_bytes(long long n, int k, int restarts) { return km_sum_bytes(n, k, restarts) / 4 * 5; }

}  // namespace

extern "C" int yk_anchor_kmeans_workspace_bytes(long long n, int k, int restarts, size_t *bytes) {
    const int rc = km_check_sizes("yk_anchor_kmeans_workspace_bytes", n, k, restarts);
    if (rc != YK_OK) return rc;
    if (!bytes) {
        yk_set_error("yk_anchor_kmeans_workspace_bytes: bytes is NULL");
        return YK_ERR_ARG;
    }
    *bytes = km_work_bytes(n, k, restarts);
    return YK_OK;
}

extern "C" int yk_anchor_kmeans_f64(const double *d_wh, long long n, const double *d_init, int k, int restarts, int iters, double *d_centroids,
                                    int32_t *d_counts, double *d_score, int32_t *d_empty, uint8_t *d_idx, void *d_work, size_t work_bytes,
                                    void *stream) {
    const char *who = "yk_anchor_kmeans_f64";
    const int rc = km_check_sizes(who, n, k, restarts);
    if (rc != YK_OK) return rc;
    if (iters < 1 || iters > YK_KMEANS_MAX_ITERS) {
        yk_set_error("%s: iters = %d: must be in 1 .. %d", who, iters, YK_KMEANS_MAX_ITERS);
        return YK_ERR_ARG;
    }
    const struct {
        const void *p;
        const char *name;
    } ptrs[] = {{d_wh, "d_wh"}, {d_init, "d_init"}, {d_centroids, "d_centroids"}, {d_counts, "d_counts"}, {d_score, "d_score"},
                {d_empty, "d_empty"}, {d_work, "d_work"}};
    for (const auto &a : ptrs)
        if (!a.p) {
            yk_set_error("%s: %s is NULL", who, a.name);
            return YK_ERR_ARG;
        }
    if (((uintptr_t)d_wh & 15) || ((uintptr_t)d_work & 15)) {
        yk_set_error("%s: d_wh and d_work must be 16-byte aligned", who);
        return YK_ERR_ARG;
    }
    if (work_bytes < km_work_bytes(n, k, restarts)) {
        yk_set_error("%s: work_bytes = %zu: %zu needed (yk_anchor_kmeans_workspace_bytes)", who, work_bytes, km_work_bytes(n, k, restarts));
        return YK_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long tiles = km_tiles(n);
    double *part_sum = (double *)d_work;
    int32_t *part_cnt = (int32_t *)((char *)d_work + km_sum_bytes(n, k, restarts));
    const double2 *x = (const double2 *)d_wh;
    const dim3 grid((unsigned)tiles, (unsigned)restarts);
    YK_HIP(hipMemsetAsync(d_empty, 0, (size_t)restarts * sizeof(int32_t), st));
    if (d_centroids != d_init)
        YK_HIP(hipMemcpyAsync(d_centroids, d_init, (size_t)restarts * k * 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(km_assign_kernel<false>, grid, dim3(YK_KMEANS_THREADS), 0, st, x, n, d_centroids, k, d_empty, part_sum, part_cnt, d_idx);
        hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)restarts), dim3(YK_KMEANS_THREADS), 0, st, part_sum, part_cnt, tiles, k, it,
                           d_centroids, d_counts, d_empty);
    }
    hipLaunchKernelGGL(km_assign_kernel<true>, grid, dim3(YK_KMEANS_THREADS), 0, st, x, n, d_centroids, k, d_empty, part_sum, (int32_t *)nullptr,
                       (uint8_t *)nullptr);
    hipLaunchKernelGGL(km_score_kernel, dim3((unsigned)restarts), dim3(YK_WAVE), 0, st, part_sum, tiles, n, d_empty, d_score);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
