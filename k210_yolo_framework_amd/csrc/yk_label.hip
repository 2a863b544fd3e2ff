// yk_label.hip — the dense training labels of a batch from its boxes (Helper.batch_box_to_label; include/yolo_hip.h).
//
// Everything that decides anything - the fit of a box to an anchor, the first argmax, the threshold, the cell - is float64 in numpy's
// operation order with contraction off, so a candidate is the one the host statement makes; the clip and the cast to fp32 come last.
//   label_kernel   grid (chunks of a sample, samples).  A chunk is up to YK_LABEL_CHUNK consecutive floats of ONE layer of ONE sample, so it
//                  is contiguous in d_labels.  The workgroup keeps the chunk in LDS: zeroes it, builds the sample's candidate table
//                  (YK_LABEL_LDS_BOXES boxes at a time: per box its primary (layer, anchor), whether it is written at all, and for this
//                  chunk's layer the cell and the anchors it is written at), folds the largest key per slot with integer LDS atomics (a
//                  maximum: the order of arrival does not matter), then every candidate sets its class bit and the one whose key the slot
//                  holds writes x y w h and the 1.  The chunk leaves with one store per element: scalar up to the first 16-byte boundary
//                  of the ADDRESS, 16 bytes per lane from there, scalar for the rest (5 + C is 25 or 85: nothing about a chunk is aligned).
//                  A sample with more boxes than the table holds is walked in tiles of YK_LABEL_LDS_BOXES boxes, twice (keys, then
//                  values), each tile read from global memory again.
// The status word is the only thing two workgroups both touch, with an integer atomicMin by the first chunk's workgroup of a sample.
// Nothing is trusted: d_first is clamped to [0, n_boxes), a class outside [0, C) or a centre that is not finite makes the box one that is not
// written, and every LDS and global index is checked against the chunk before it is used.
#include "yk_common.h"

#pragma clang fp contract(off)

#define YK_LABEL_THREADS 256
#define YK_LABEL_MAX_SLOTS (YK_LABEL_CHUNK / 6 + 2) /* 5 + C >= 6 floats per slot; a chunk may begin and end inside one */
#define YK_LABEL_PRIMARY 0x40000000                 /* key = is_primary * 2^30 + box + 1; n_boxes < 2^30 */

namespace {

struct label_args {
    yk_label_cfg_t cfg;
    size_t per[YK_MAX_LAYERS];        // floats of one sample in layer l: h w A (5 + C)
    size_t base[YK_MAX_LAYERS];       // floats of d_labels before layer l: n * (per[0] + .. + per[l - 1])
    int chunk0[YK_MAX_LAYERS + 1];    // the first chunk of layer l among a sample's chunks
};

// Helper._fake_iou of one box and one anchor
__device__ __forceinline__ double label_fit(double w, double h, double aw, double ah) {
    const double o = fmax(fmin(w, aw), 0.0) * fmax(fmin(h, ah), 0.0);
    return o / (w * h + aw * ah - o);
}

// floor(v * cells) as a cell index, or -1 where numpy would raise or wrap (and for a NaN: every comparison with it is false)
__device__ __forceinline__ int label_cell(double v, int cells) {
    const double c = floor(v * (double)cells);
    return c >= 0.0 && c < (double)cells ? (int)c : -1;
}

__global__ void __launch_bounds__(YK_LABEL_THREADS) label_kernel(const label_args a, const double *__restrict__ boxes, int n_boxes,
                                                                 const int32_t *__restrict__ first, int sample0, float *__restrict__ labels,
                                                                 int32_t *__restrict__ status) {
    __shared__ float s_chunk[YK_LABEL_CHUNK];
    __shared__ int s_key[YK_LABEL_MAX_SLOTS];
    __shared__ float4 s_xywh[YK_LABEL_LDS_BOXES];
    __shared__ int s_cell[YK_LABEL_LDS_BOXES];              // cy * w + cx in this chunk's layer; -1: the box is not written here
    __shared__ unsigned s_mask[YK_LABEL_LDS_BOXES];         // bits 0..7: the anchors of this layer it is written at; bit 8 + a: a is its primary
    __shared__ int s_cls[YK_LABEL_LDS_BOXES];
    const int tid = threadIdx.x;
    const size_t sample = (size_t)sample0 + blockIdx.y;
    const yk_label_cfg_t &cfg = a.cfg;
    int layer = 0;
    while (layer + 1 < cfg.n_layers && (int)blockIdx.x >= a.chunk0[layer + 1]) ++layer;
    const size_t lo = (size_t)((int)blockIdx.x - a.chunk0[layer]) * YK_LABEL_CHUNK;      // the chunk is floats [lo, lo + len) of the sample's layer
    const int len = (int)(a.per[layer] - lo < (size_t)YK_LABEL_CHUNK ? a.per[layer] - lo : (size_t)YK_LABEL_CHUNK);
    const int E = 5 + cfg.class_num, A = cfg.anchor_num[layer], gw = cfg.out_w[layer], gh = cfg.out_h[layer];
    const size_t slot0 = lo / (size_t)E;                                                 // the first slot the chunk holds a float of
    for (int i = tid; i < YK_LABEL_CHUNK; i += YK_LABEL_THREADS) s_chunk[i] = 0.f;
    for (int i = tid; i < YK_LABEL_MAX_SLOTS; i += YK_LABEL_THREADS) s_key[i] = 0;
    int b0 = first[sample], b1 = first[sample + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > n_boxes ? n_boxes : b1;
    const int m = b1 > b0 ? b1 - b0 : 0;
    const int tiles = (m + YK_LABEL_LDS_BOXES - 1) / YK_LABEL_LDS_BOXES;
    const bool multi = cfg.assign == YK_ASSIGN_MULTI;
    int worst = 0x7fffffff;
    for (int pass = 0; pass < 2; ++pass) {
        for (int tile = 0; tile < tiles; ++tile) {
            const int t0 = tile * YK_LABEL_LDS_BOXES, tn = m - t0 < YK_LABEL_LDS_BOXES ? m - t0 : YK_LABEL_LDS_BOXES;
            if (pass == 0 || tiles > 1) {                                               // (one tile: the table of pass 0 still stands)
                __syncthreads();
                for (int j = tid; j < tn; j += YK_LABEL_THREADS) {
                    const double *row = boxes + (size_t)(b0 + t0 + j) * 5;
                    const double c = row[0], x = row[1], y = row[2], w = row[3], h = row[4];
                    // first argmax over the flattened (layer, anchor), numpy's: a NaN is a maximum
                    double best = 0.0;
                    int bl = 0, ba = 0;
                    bool seen = false;
                    for (int l = 0; l < cfg.n_layers; ++l)
                        for (int q = 0; q < cfg.anchor_num[l]; ++q) {
                            const double f = label_fit(w, h, cfg.anchors[l][q][0], cfg.anchors[l][q][1]);
                            if (!seen || (best == best && (f > best || f != f))) best = f, bl = l, ba = q, seen = true;
                        }
                    // written at all?  every layer it has a candidate in must hold its cell, and its class must be one
                    // (numpy's astype(int) truncates toward zero: -0.5 is class 0, and so is (int)c below)
                    bool ok = c > -1.0 && c < (double)cfg.class_num;
                    unsigned mask = 0;
                    for (int l = 0; l < cfg.n_layers; ++l) {
                        unsigned here = 0;
                        for (int q = 0; q < cfg.anchor_num[l]; ++q) {
                            const bool prim = l == bl && q == ba;
                            if (prim || (multi && label_fit(w, h, cfg.anchors[l][q][0], cfg.anchors[l][q][1]) > cfg.assign_iou))
                                here |= (1u << q) | (prim ? 0x100u << q : 0u);
                        }
                        if (here && (label_cell(x, cfg.out_w[l]) < 0 || label_cell(y, cfg.out_h[l]) < 0)) ok = false;
                        if (l == layer) mask = here;
                    }
                    if (!ok && b0 + t0 + j < worst) worst = b0 + t0 + j;
                    const int cx = label_cell(x, gw), cy = label_cell(y, gh);
                    s_cell[j] = ok && mask && cx >= 0 && cy >= 0 ? cy * gw + cx : -1;
                    s_mask[j] = mask;
                    s_cls[j] = ok ? (int)c : 0;
                    s_xywh[j] = make_float4((float)fmin(fmax(x, 1e-8), 1.0), (float)fmin(fmax(y, 1e-8), 1.0), (float)fmin(fmax(w, 1e-8), 1.0),
                                            (float)fmin(fmax(h, 1e-8), 1.0));
                }
                __syncthreads();
            }
            for (int j = tid; j < tn * A; j += YK_LABEL_THREADS) {                       // one candidate place per lane: (box, anchor of this layer)
                const int k = j / A, q = j - k * A;
                if (s_cell[k] < 0 || !(s_mask[k] >> q & 1u)) continue;
                const size_t slot = (size_t)s_cell[k] * A + q;
                const size_t f0 = slot * E;                                              // the slot is floats [f0, f0 + E) of the sample's layer
                if (f0 + E <= lo || f0 >= lo + len) continue;                            // no float of it in this chunk
                const int sl = (int)(slot - slot0);                                      // < YK_LABEL_MAX_SLOTS: the slot overlaps the chunk
                const int key = ((s_mask[k] >> (8 + q) & 1u) ? YK_LABEL_PRIMARY : 0) + t0 + k + 1;
                if (pass == 0) {
                    atomicMax(&s_key[sl], key);
                    continue;
                }
                const size_t fc = f0 + 5 + s_cls[k];
                if (fc >= lo && fc < lo + len) s_chunk[fc - lo] = 1.f;                   // (every writer of this float writes 1)
                if (s_key[sl] != key) continue;
                const float v[5] = {s_xywh[k].x, s_xywh[k].y, s_xywh[k].z, s_xywh[k].w, 1.f};
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (f0 + e >= lo && f0 + e < lo + len) s_chunk[f0 + e - lo] = v[e];
            }
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && worst != 0x7fffffff) atomicMin(status, worst);
    // the chunk leaves: one store per element
    float *dst = labels + a.base[layer] + sample * a.per[layer] + lo;
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15) / 4;
    head = head < len ? head : len;
    const int vecs = (len - head) / 4;
    if (tid < head) dst[tid] = s_chunk[tid];
    float4 *dst4 = reinterpret_cast<float4 *>(dst + head);
    for (int i = tid; i < vecs; i += YK_LABEL_THREADS) {
        const float *s = s_chunk + head + 4 * i;
        dst4[i] = make_float4(s[0], s[1], s[2], s[3]);
    }
    const int done = head + 4 * vecs;
    if (tid < len - done) dst[done + tid] = s_chunk[done + tid];
}

}  // namespace

extern "C" int yk_boxes_to_labels_f32(const yk_label_cfg_t *cfg, const double *d_boxes, int n_boxes, const int32_t *d_first, int n,
                                      float *d_labels, int32_t *d_status, void *stream) {
    const char *who = "yk_boxes_to_labels_f32";
    if (n < 0) {
        yk_set_error("%s: n = %d", who, n);
        return YK_ERR_ARG;
    }
    if (n == 0) return YK_OK;
    if (n_boxes < 0 || n_boxes >= YK_LABEL_PRIMARY) {
        yk_set_error("%s: n_boxes = %d: must be in 0 .. 2^30 - 1", who, n_boxes);
        return YK_ERR_ARG;
    }
    if (!cfg) {
        yk_set_error("%s: cfg is NULL", who);
        return YK_ERR_ARG;
    }
    if (cfg->n_layers < 1 || cfg->n_layers > YK_MAX_LAYERS) {
        yk_set_error("%s: cfg->n_layers = %d: must be in 1 .. %d", who, cfg->n_layers, YK_MAX_LAYERS);
        return YK_ERR_ARG;
    }
    if (cfg->class_num < 1 || cfg->class_num > (1 << 24)) {
        yk_set_error("%s: cfg->class_num = %d", who, cfg->class_num);
        return YK_ERR_ARG;
    }
    if (cfg->assign != YK_ASSIGN_BEST && cfg->assign != YK_ASSIGN_MULTI) {
        yk_set_error("%s: cfg->assign = %d: YK_ASSIGN_BEST or YK_ASSIGN_MULTI", who, cfg->assign);
        return YK_ERR_ARG;
    }
    if (cfg->assign == YK_ASSIGN_MULTI && !(cfg->assign_iou > 0.0 && cfg->assign_iou < 1.0)) {
        yk_set_error("%s: cfg->assign_iou = %g: must be inside (0, 1)", who, cfg->assign_iou);
        return YK_ERR_ARG;
    }
    label_args a;
    memset(&a, 0, sizeof(a));
    a.cfg = *cfg;
    unsigned long long total = 0, chunks = 0;                         // floats of one sample; its chunks
    for (int l = 0; l < cfg->n_layers; ++l) {
        if (cfg->anchor_num[l] < 1 || cfg->anchor_num[l] > YK_MAX_ANCHORS) {
            yk_set_error("%s: cfg->anchor_num[%d] = %d: must be in 1 .. %d", who, l, cfg->anchor_num[l], YK_MAX_ANCHORS);
            return YK_ERR_ARG;
        }
        if (cfg->out_h[l] <= 0 || cfg->out_w[l] <= 0) {
            yk_set_error("%s: cfg->out_h[%d] x cfg->out_w[%d] = %d x %d", who, l, l, cfg->out_h[l], cfg->out_w[l]);
            return YK_ERR_ARG;
        }
        // h w < 2^62, A (5 + C) < 2^28: the cell index must also fit an int, and the product a size_t with n of them
        unsigned long long per = (unsigned long long)cfg->out_h[l] * (unsigned long long)cfg->out_w[l];
        if (per > 0x7fffffffull || __builtin_mul_overflow(per, (unsigned long long)cfg->anchor_num[l] * (unsigned)(5 + cfg->class_num), &per) ||
            __builtin_add_overflow(total, per, &total)) {
            yk_set_error("%s: layer %d of %d x %d x %d x %d is beyond size_t", who, l, cfg->out_h[l], cfg->out_w[l], cfg->anchor_num[l],
                         5 + cfg->class_num);
            return YK_ERR_ARG;
        }
        a.per[l] = (size_t)per;
        a.chunk0[l] = (int)chunks;
        chunks += (per + YK_LABEL_CHUNK - 1) / YK_LABEL_CHUNK;
        if (chunks > 0x7fffffffull) {
            yk_set_error("%s: a sample of more than 2^31 - 1 chunks of %d floats", who, YK_LABEL_CHUNK);
            return YK_ERR_ARG;
        }
        a.chunk0[l + 1] = (int)chunks;
    }
    size_t bytes;
    if (__builtin_mul_overflow((size_t)total, (size_t)n, &bytes) || __builtin_mul_overflow(bytes, sizeof(float), &bytes)) {
        yk_set_error("%s: %d samples of %llu floats are beyond size_t", who, n, total);
        return YK_ERR_ARG;
    }
    const char *null = !d_first ? "d_first" : !d_labels ? "d_labels" : !d_status ? "d_status" : n_boxes > 0 && !d_boxes ? "d_boxes" : nullptr;
    if (null) {
        yk_set_error("%s: %s is NULL", who, null);
        return YK_ERR_ARG;
    }
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_boxes & 7) || ((uintptr_t)d_first & 3) || ((uintptr_t)d_status & 3)) {
        yk_set_error("%s: a misaligned pointer", who);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("%s: no HIP device", who);
        return YK_ERR_NO_DEVICE;
    }
    size_t before = 0;
    for (int l = 0; l < cfg->n_layers; ++l) {
        a.base[l] = before * (size_t)n;
        before += a.per[l];
    }
    hipStream_t st = (hipStream_t)stream;
    YK_HIP(hipMemsetD32Async((hipDeviceptr_t)d_status, 0x7fffffff, 1, st));
    yk_for_grid_y(n, [&](int base, int m) {
        hipLaunchKernelGGL(label_kernel, dim3((unsigned)chunks, (unsigned)m), dim3(YK_LABEL_THREADS), 0, st, a, d_boxes, n_boxes, d_first, base,
                           d_labels, d_status);
    });
    YK_HIP(hipGetLastError());
    return YK_OK;
}
