// yk_pre.hip — GPU pre-processing immediately before the path:
// Helper._process_img's letterbox (tools/utils.py:378-399): scale = min(in_wh / img_wh),
// translation = ((in_wh - img_wh*scale)/2).astype(int), then
// skimage.transform.warp(img, AffineTransform(scale, translation).inverse, output_shape=in_hw, order=1,
//                        mode='constant', cval=0, preserve_range=True).astype('uint8')
// restated with skimage's own arithmetic (float64, one rounding per operation; this file is built with -ffp-contract=off):
//   M = inv(AffineTransform.params) = [[1/s, 0, -(tx*(1/s))], [0, 1/s, -(ty*(1/s))], [0, 0, 1]]   (numpy.linalg.inv of that matrix)
//   c = M00*x + M02, r = M11*y + M12                                   (_warps_cy._transform_metric)
//   minr/minc = floor, maxr/maxc = ceil, dr = r - minr, dc = c - minc   (interpolation.pxd bilinear_interpolation)
//   top = (1-dc)*I[minr,minc] + dc*I[minr,maxc]; bottom likewise on maxr; out = (1-dr)*top + dr*bottom; pixels outside -> cval 0
//   .astype('uint8') truncation.
// Pinned: tests/golden/letterbox_golden.npz holds outputs of the real scikit-image for seven source sizes; the kernel, the host
// mirror (helper.letterbox_bilinear) and the oracle reproduce them bit for bit.
// The per-image max normalisation that follows (utils.py:405) is fused into the stem conv (yk_run_u8).
#include "yk_common.h"

// One letterboxed pixel (x, y) of the network tensor from a source of sh x sw pixels: the arithmetic above, truncating cast.  tap(yy, xx, ch)
// is the source's byte at a position inside it; a tap outside reads 0.
template <class Tap>
__device__ __forceinline__ void letterbox_px_of(Tap tap, int sh, int sw, double scale, int tx, int ty, int x, int y, uint8_t out[3]) {
    const double inv = 1.0 / scale;
    const double c = inv * (double)x + (-((double)tx * inv)), r = inv * (double)y + (-((double)ty * inv));
    const double minc_f = floor(c), minr_f = floor(r);
    const int minc = (int)minc_f, minr = (int)minr_f, maxc = (int)ceil(c), maxr = (int)ceil(r);
    const double dc = c - minc_f, dr = r - minr_f;
    auto px = [&](int yy, int xx, int ch) -> double { return (yy >= 0 && yy < sh && xx >= 0 && xx < sw) ? (double)tap(yy, xx, ch) : 0.0; };
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double top = (1.0 - dc) * px(minr, minc, ch) + dc * px(minr, maxc, ch);
        const double bottom = (1.0 - dc) * px(maxr, minc, ch) + dc * px(maxr, maxc, ch);
        out[ch] = (uint8_t)((1.0 - dr) * top + dr * bottom);    // astype('uint8'): truncation
    }
}

// ... from source frame `im`, sh rows of sw pixels `stride` bytes apart
__device__ __forceinline__ void letterbox_px(const uint8_t *__restrict__ im, int sh, int sw, size_t stride, double scale, int tx, int ty, int x,
                                             int y, uint8_t out[3]) {
    letterbox_px_of([&](int yy, int xx, int ch) { return im[(size_t)yy * stride + (size_t)xx * 3 + ch]; }, sh, sw, scale, tx, ty, x, y, out);
}

// ... from a contiguous frame [sh][sw][3]
__device__ __forceinline__ void letterbox_px(const uint8_t *__restrict__ im, int sh, int sw, double scale, int tx, int ty, int x, int y,
                                             uint8_t out[3]) {
    letterbox_px(im, sh, sw, (size_t)sw * 3, scale, tx, ty, x, y, out);
}

__global__ void __launch_bounds__(256) letterbox_u8_kernel(const uint8_t *__restrict__ src, int batch, int sh, int sw,
                                                           uint8_t *__restrict__ dst, int dh, int dw, double scale, int tx, int ty) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * dh * dw;
    if (idx >= total) return;
    const int x = (int)(idx % dw), y = (int)((idx / dw) % dh), b = (int)(idx / ((size_t)dw * dh));
    uint8_t v[3];
    letterbox_px(src + (size_t)b * sh * sw * 3, sh, sw, scale, tx, ty, x, y, v);
    uint8_t *o = dst + idx * 3;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
}

static void letterbox_params(int src_h, int src_w, int dst_h, int dst_w, double *scale, int *tx, int *ty) {
    const double sx = (double)dst_w / (double)src_w, sy = (double)dst_h / (double)src_h;
    *scale = sx < sy ? sx : sy;                                                // utils.py:381-382
    *tx = (int)(((double)dst_w - (double)src_w * *scale) / 2.0);               // .astype(int): truncation, utils.py:385
    *ty = (int)(((double)dst_h - (double)src_h * *scale) / 2.0);
}

extern "C" int yk_letterbox_u8(const uint8_t *d_src, int batch, int src_h, int src_w, uint8_t *d_dst, int dst_h, int dst_w,
                               void *stream) {
    if (!d_src || !d_dst || batch <= 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("yk_letterbox_u8: bad argument");
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_letterbox_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    double scale;
    int tx, ty;
    letterbox_params(src_h, src_w, dst_h, dst_w, &scale, &tx, &ty);
    const size_t total = (size_t)batch * dst_h * dst_w;
    hipLaunchKernelGGL(letterbox_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_src, batch,
                       src_h, src_w, d_dst, dst_h, dst_w, scale, tx, ty);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---- the same letterbox with ONE FRAME PER TABLE ROW (the three row types of yolo_hip.h), one launch: blockIdx.y is the row, so a workgroup
// reads one row (uniform loads) and every pixel goes through letterbox_px_of with that row's (scale, tx, ty) - the values letterbox_params gives
// yk_letterbox_u8 for the same sizes, hence the same bytes.  Offsets carry no alignment (3-byte pixels): sources are read a byte at a time, as
// above.  A row type states two things: row_ok(row, src_bytes), false for a row the host should have refused - nothing of src is read for it and
// its frame is zeros - and row_px(src, row, x, y, out), the source size and the tap this row hands to the arithmetic.
//
// A RAGGED batch: pictures of different sizes packed into one buffer, one row each.
__device__ __forceinline__ bool row_ok(const yk_ragged_row_t row, size_t src_bytes) { return yk_ragged_row_inside(row, src_bytes); }
__device__ __forceinline__ void row_px(const uint8_t *__restrict__ src, const yk_ragged_row_t row, int x, int y, uint8_t out[3]) {
    letterbox_px(src + row.offset, row.h, row.w, row.scale, row.tx, row.ty, x, y, out);
}

// TILES of the pictures of a ragged batch (sliced inference: k210_yolo_framework_amd/tiles.py): a tile is h rows of w pixels
// `stride` bytes apart, so letterbox_px reads it in place and its bounds are the tile's - a tap outside the tile reads 0, not the parent's
// neighbouring pixel, and frame t is yk_letterbox_u8 of a contiguous copy of the crop, bit for bit.
__device__ __forceinline__ bool row_ok(const yk_tile_row_t row, size_t src_bytes) {
    // Its last byte is offset + (h-1)*stride + 3*w - 1; tested by division, so that no product can overflow
    bool ok = row.h > 0 && row.w > 0 && row.stride >= (int64_t)3 * row.w && row.offset <= src_bytes;
    if (ok) {
        const size_t room = src_bytes - row.offset, last = (size_t)3 * row.w, st = (size_t)row.stride, rows = (size_t)(row.h - 1);
        ok = last <= room && (rows == 0 || st <= (room - last) / rows);
    }
    return ok;
}
__device__ __forceinline__ void row_px(const uint8_t *__restrict__ src, const yk_tile_row_t row, int x, int y, uint8_t out[3]) {
    letterbox_px(src + row.offset, row.h, row.w, (size_t)row.stride, row.scale, row.tx, row.ty, x, y, out);
}

// VIEWS of the pictures of a ragged batch (test-time augmentation: k210_yolo_framework_amd/tta.py): a view is a zero canvas of
// ch x cw pixels with the picture pasted at (oy, ox), mirrored or not.  The canvas is the source letterbox_px_of sees, its taps read out of the
// picture in place, so frame v is yk_letterbox_u8 of the canvas, bit for bit, and no canvas is ever written.
static_assert(sizeof(yk_view_row_t) == 56, "yk_view_row_t has no padding");
__device__ __forceinline__ bool row_ok(const yk_view_row_t row, size_t src_bytes) {
    // The sums are taken in 64 bits, so none can overflow
    return row.h > 0 && row.w > 0 && row.oy >= 0 && row.ox >= 0 && (int64_t)row.oy + row.h <= (int64_t)row.ch &&
           (int64_t)row.ox + row.w <= (int64_t)row.cw && row.offset <= src_bytes && (size_t)row.h * row.w * 3 <= src_bytes - row.offset;
}
__device__ __forceinline__ void row_px(const uint8_t *__restrict__ src, const yk_view_row_t row, int x, int y, uint8_t out[3]) {
    const uint8_t *im = src + row.offset;
    const int h = row.h, w = row.w, oy = row.oy, ox = row.ox;
    const bool mirror = row.mirror != 0;
    letterbox_px_of(
        [&](int yy, int xx, int ch) -> uint8_t {
            const int py = yy - oy, qx = xx - ox;                  // yy in [0, ch), oy in [0, ch]: no overflow
            if (py < 0 || py >= h || qx < 0 || qx >= w) return 0;
            return im[((size_t)py * w + (size_t)(mirror ? w - 1 - qx : qx)) * 3 + ch];
        },
        row.ch, row.cw, row.scale, row.tx, row.ty, x, y, out);
}

template <class Row>
__global__ void __launch_bounds__(256) letterbox_rows_u8_kernel(const uint8_t *__restrict__ src, size_t src_bytes, const Row *__restrict__ table,
                                                                uint8_t *__restrict__ dst, int dh, int dw) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)dh * dw;
    if (idx >= per) return;
    const Row row = table[blockIdx.y];
    const int x = (int)(idx % dw), y = (int)(idx / dw);
    uint8_t v[3] = {0, 0, 0};
    const bool ok = row_ok(row, src_bytes);
    if (ok) row_px(src, row, x, y, v);
    uint8_t *o = dst + ((size_t)blockIdx.y * per + idx) * 3;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
}

template <class Row>
static int letterbox_rows_u8(const char *name, const uint8_t *d_src, size_t src_bytes, const Row *d_table, int n, uint8_t *d_dst, int dst_h,
                             int dst_w, void *stream) {
    if (!d_src || !d_table || !d_dst || n <= 0 || src_bytes == 0 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("%s: bad argument", name);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("%s: no HIP device", name);
        return YK_ERR_NO_DEVICE;
    }
    const size_t per = (size_t)dst_h * dst_w;
    yk_for_grid_y(n, [&](int base, int m) {
        hipLaunchKernelGGL(letterbox_rows_u8_kernel<Row>, dim3((unsigned)((per + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream,
                           d_src, src_bytes, d_table + base, d_dst + (size_t)base * per * 3, dst_h, dst_w);
    });
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// scale, tx, ty of n host rows from the source size each row's fields sh, sw hold; `what` words the refusal of a row without one
template <class Row>
static int fill_params(const char *name, const char *what, int32_t Row::*sh, int32_t Row::*sw, Row *h_table, int n, int dst_h, int dst_w) {
    if (!h_table || n <= 0 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("%s: bad argument", name);
        return YK_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (h_table[i].*sh <= 0 || h_table[i].*sw <= 0) {
            yk_set_error("%s: row %d %s %d x %d", name, i, what, (int)(h_table[i].*sh), (int)(h_table[i].*sw));
            return YK_ERR_ARG;
        }
    for (int i = 0; i < n; ++i) {
        int tx, ty;
        letterbox_params(h_table[i].*sh, h_table[i].*sw, dst_h, dst_w, &h_table[i].scale, &tx, &ty);
        h_table[i].tx = tx;
        h_table[i].ty = ty;
    }
    return YK_OK;
}

extern "C" int yk_letterbox_ragged_params(yk_ragged_row_t *h_table, int n, int dst_h, int dst_w) {
    return fill_params("yk_letterbox_ragged_params", "is", &yk_ragged_row_t::h, &yk_ragged_row_t::w, h_table, n, dst_h, dst_w);
}
extern "C" int yk_letterbox_tiles_params(yk_tile_row_t *h_table, int n, int dst_h, int dst_w) {
    return fill_params("yk_letterbox_tiles_params", "is", &yk_tile_row_t::h, &yk_tile_row_t::w, h_table, n, dst_h, dst_w);
}
extern "C" int yk_letterbox_views_params(yk_view_row_t *h_table, int n, int dst_h, int dst_w) {
    return fill_params("yk_letterbox_views_params", "has a canvas of", &yk_view_row_t::ch, &yk_view_row_t::cw, h_table, n, dst_h, dst_w);
}

extern "C" int yk_letterbox_ragged_u8(const uint8_t *d_src, size_t src_bytes, const yk_ragged_row_t *d_table, int n, uint8_t *d_dst,
                                      int dst_h, int dst_w, void *stream) {
    return letterbox_rows_u8("yk_letterbox_ragged_u8", d_src, src_bytes, d_table, n, d_dst, dst_h, dst_w, stream);
}
extern "C" int yk_letterbox_tiles_u8(const uint8_t *d_src, size_t src_bytes, const yk_tile_row_t *d_table, int n, uint8_t *d_dst, int dst_h,
                                     int dst_w, void *stream) {
    return letterbox_rows_u8("yk_letterbox_tiles_u8", d_src, src_bytes, d_table, n, d_dst, dst_h, dst_w, stream);
}
extern "C" int yk_letterbox_views_u8(const uint8_t *d_src, size_t src_bytes, const yk_view_row_t *d_table, int n, uint8_t *d_dst, int dst_h,
                                     int dst_w, void *stream) {
    return letterbox_rows_u8("yk_letterbox_views_u8", d_src, src_bytes, d_table, n, d_dst, dst_h, dst_w, stream);
}

// ---- letterbox + training augmentation (k210_yolo_framework_amd/augment.py; the imgaug OneOf of tools/utils.py:84-88): the u8
// letterboxed frame L above, then warped by the image's inverse map inv[b] = M (2x3, float64, pixel-index coordinates, computed on
// the host; no transcendental here):
//   c = M00*x + M01*y + M02, r = M10*x + M11*y + M12; taps floor/ceil as above, taps outside [0,dh)x[0,dw) read 0;
//   out = min(255, floor((1-dr)*top + dr*bottom + 0.5)).
// Each tap's L value is computed on the fly (letterbox_px), so no intermediate frame goes to HBM and the result is bit-identical
// to yk_letterbox_u8 followed by the warp.  Identity and mirror matrices have integer entries: an exact pixel copy.
//
// The warp of output pixel (x, y) of a dh x dw frame by the map m[6], written to o[3]: frame(xx, yy, v) puts the frame's pixel at an integer
// position inside it into v, which arrives as zeros.
template <class Frame>
__device__ __forceinline__ void warp_px(Frame frame, const double *m, int dh, int dw, int x, int y, uint8_t *o) {
    const double c = m[0] * (double)x + m[1] * (double)y + m[2], r = m[3] * (double)x + m[4] * (double)y + m[5];
    const double minc_f = floor(c), minr_f = floor(r), maxc_f = ceil(c), maxr_f = ceil(r);
    const double dc = c - minc_f, dr = r - minr_f;
    const double tr[4] = {minr_f, minr_f, maxr_f, maxr_f}, tc[4] = {minc_f, maxc_f, minc_f, maxc_f};
    double t[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint8_t v[3] = {0, 0, 0};
        if (tr[k] >= 0.0 && tr[k] < (double)dh && tc[k] >= 0.0 && tc[k] < (double)dw)      // compared as doubles: any M is safe
            frame((int)tc[k], (int)tr[k], v);
        t[k][0] = v[0];
        t[k][1] = v[1];
        t[k][2] = v[2];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double top = (1.0 - dc) * t[0][ch] + dc * t[1][ch];
        const double bottom = (1.0 - dc) * t[2][ch] + dc * t[3][ch];
        o[ch] = (uint8_t)fmin(255.0, floor((1.0 - dr) * top + dr * bottom + 0.5));
    }
}

__global__ void __launch_bounds__(256) letterbox_augment_u8_kernel(const uint8_t *__restrict__ src, int batch, int sh, int sw,
                                                                   const double *__restrict__ inv, uint8_t *__restrict__ dst, int dh,
                                                                   int dw, double scale, int tx, int ty) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * dh * dw;
    if (idx >= total) return;
    const int x = (int)(idx % dw), y = (int)((idx / dw) % dh), b = (int)(idx / ((size_t)dw * dh));
    const uint8_t *im = src + (size_t)b * sh * sw * 3;
    warp_px([=](int xx, int yy, uint8_t v[3]) { letterbox_px(im, sh, sw, scale, tx, ty, xx, yy, v); }, inv + (size_t)b * 6, dh, dw, x, y,
            dst + idx * 3);
}

extern "C" int yk_letterbox_augment_u8(const uint8_t *d_src, int batch, int src_h, int src_w, const double *d_inv, uint8_t *d_dst,
                                       int dst_h, int dst_w, void *stream) {
    if (!d_src || !d_inv || !d_dst || batch <= 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("yk_letterbox_augment_u8: bad argument");
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_letterbox_augment_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    double scale;
    int tx, ty;
    letterbox_params(src_h, src_w, dst_h, dst_w, &scale, &tx, &ty);
    const size_t total = (size_t)batch * dst_h * dst_w;
    hipLaunchKernelGGL(letterbox_augment_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_src,
                       batch, src_h, src_w, d_inv, d_dst, dst_h, dst_w, scale, tx, ty);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---- mosaic (k210_yolo_framework_amd/mosaic.py): one frame from four pictures of any sizes, a whole ragged training batch
// in one launch.  Sample b has four table rows in quadrant order (0 TL, 1 TR, 2 BL, 3 BR) and a seam (cx, cy): output pixel (x, y) belongs
// to quadrant (x >= cx) + 2*(y >= cy) and is letterbox_px of that row's picture with that row's (scale, tx, ty) - the arithmetic above,
// unchanged, so a quadrant equals the letterbox of its picture restricted to it, and four equal rows give the plain letterbox wherever
// the seam is.  The table is not trusted: a row without pixels or one that leaves the buffer gives zeros and reads nothing.
__device__ __forceinline__ void mosaic_px(const uint8_t *__restrict__ src, size_t src_bytes, const yk_ragged_row_t *__restrict__ rows4, int cx,
                                          int cy, int x, int y, uint8_t out[3]) {
    const yk_ragged_row_t row = rows4[(x >= cx ? 1 : 0) + (y >= cy ? 2 : 0)];
    out[0] = out[1] = out[2] = 0;
    if (yk_ragged_row_inside(row, src_bytes)) letterbox_px(src + row.offset, row.h, row.w, row.scale, row.tx, row.ty, x, y, out);
}

// inv == NULL: the mosaic frame itself.  Otherwise the frame warped by the sample's inverse map - warp_px, as letterbox_augment_u8_kernel warps
// the letterbox: each of the four taps evaluates the mosaic pixel on the fly, no intermediate frame.
__global__ void __launch_bounds__(256) mosaic_ragged_u8_kernel(const uint8_t *__restrict__ src, size_t src_bytes,
                                                               const yk_ragged_row_t *__restrict__ table, const int32_t *__restrict__ centre,
                                                               const double *__restrict__ inv, uint8_t *__restrict__ dst, int dh, int dw) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)dh * dw;
    if (idx >= per) return;
    const yk_ragged_row_t *rows4 = table + (size_t)blockIdx.y * 4;
    const int cx = min(max(centre[(size_t)blockIdx.y * 2], 0), dw), cy = min(max(centre[(size_t)blockIdx.y * 2 + 1], 0), dh);
    const int x = (int)(idx % dw), y = (int)(idx / dw);
    uint8_t *o = dst + ((size_t)blockIdx.y * per + idx) * 3;
    if (!inv) {
        uint8_t v[3];
        mosaic_px(src, src_bytes, rows4, cx, cy, x, y, v);
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        return;
    }
    warp_px([=](int xx, int yy, uint8_t v[3]) { mosaic_px(src, src_bytes, rows4, cx, cy, xx, yy, v); }, inv + (size_t)blockIdx.y * 6, dh, dw, x, y,
            o);
}

extern "C" int yk_mosaic_params(yk_ragged_row_t *h_rows4, int cx, int cy, const double *gain4, int dst_h, int dst_w) {
    if (!h_rows4 || !gain4 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("yk_mosaic_params: bad argument");
        return YK_ERR_ARG;
    }
    for (int k = 0; k < 4; ++k)
        if (h_rows4[k].h <= 0 || h_rows4[k].w <= 0 || !(gain4[k] > 0.0) || !(gain4[k] <= 1.0e300)) {
            yk_set_error("yk_mosaic_params: row %d is %d x %d, gain %g", k, (int)h_rows4[k].h, (int)h_rows4[k].w, gain4[k]);
            return YK_ERR_ARG;
        }
    for (int k = 0; k < 4; ++k) {
        double s;
        int tx, ty;
        letterbox_params(h_rows4[k].h, h_rows4[k].w, dst_h, dst_w, &s, &tx, &ty);
        const double scale = gain4[k] * s;
        const double pw = (double)h_rows4[k].w * scale, ph = (double)h_rows4[k].h * scale;
        h_rows4[k].scale = scale;
        h_rows4[k].tx = (k & 1) ? cx : cx - (int)ceil(pw);            // the corner nearest the seam sits at the seam
        h_rows4[k].ty = (k & 2) ? cy : cy - (int)ceil(ph);
    }
    return YK_OK;
}

extern "C" int yk_mosaic_ragged_u8(const uint8_t *d_src, size_t src_bytes, const yk_ragged_row_t *d_table, const int32_t *d_centre,
                                   const double *d_inv, int n, uint8_t *d_dst, int dst_h, int dst_w, void *stream) {
    if (!d_src || !d_table || !d_centre || !d_dst || n <= 0 || src_bytes == 0 || dst_h <= 0 || dst_w <= 0) {
        yk_set_error("yk_mosaic_ragged_u8: bad argument");
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_mosaic_ragged_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    const size_t per = (size_t)dst_h * dst_w;
    yk_for_grid_y(n, [&](int base, int m) {
        hipLaunchKernelGGL(mosaic_ragged_u8_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream, d_src,
                           src_bytes, d_table + (size_t)base * 4, d_centre + (size_t)base * 2, d_inv ? d_inv + (size_t)base * 6 : nullptr,
                           d_dst + (size_t)base * per * 3, dst_h, dst_w);
    });
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---- HSV colour jitter (k210_yolo_framework_amd/colour.py): every finished u8 frame gets its own hue rotation dh (turns),
// saturation gain gs and exposure gain gv, in place, one thread per pixel, which reads its own three bytes and writes them back.  Float64,
// the operations of colour.jitter_u8 in its order (this file is built with -ffp-contract=off), so the bytes are the host function's:
//   V = max(max(r,g),b); m = min(min(r,g),b); d = V - m
//   h = 0 when d == 0; else (g-b)/d when V == r; else 2 + (b-r)/d when V == g; else 4 + (r-g)/d
//   h = h + 6*dh; h = h - 6*floor(h/6); h = 0 unless 0 <= h < 6
//   S = d/V (0 when V == 0); S' = min(1, S*gs); V' = min(255, V*gv)
//   i = floor(h); f = h - i; p = V'(1-S'); q = V'(1-S'f); t = V'(1-S'(1-f)); the six sectors; each channel min(255, floor(x + 0.5)).
// No LDS, no transcendental.  The table is not trusted: a row that is not finite or has a negative gain leaves its frame untouched (every
// comparison with a NaN is false), and no value of a row can move a thread off its own pixel.  A neutral row (0, 1, 1) returns early: the
// arithmetic gives the same bytes.  The pixel index is a size_t over the whole batch, so neither n nor n*h*w meets a 16- or 32-bit limit.
__global__ void __launch_bounds__(256) hsv_jitter_u8_kernel(uint8_t *__restrict__ frames, size_t first, size_t total, size_t per,
                                                            const double *__restrict__ params) {
    const size_t idx = first + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const double *row = params + (idx / per) * 3;
    const double dh = row[0], gs = row[1], gv = row[2];
    const double big = 1.7976931348623157e308;                      // DBL_MAX: |x| <= big is "finite"
    if (!(dh >= -big && dh <= big && gs >= 0.0 && gs <= big && gv >= 0.0 && gv <= big)) return;
    if (dh == 0.0 && gs == 1.0 && gv == 1.0) return;
    uint8_t *px = frames + idx * 3;
    const double r = (double)px[0], g = (double)px[1], b = (double)px[2];
    const double V = fmax(fmax(r, g), b), m = fmin(fmin(r, g), b), d = V - m;
    double h = 0.0;
    if (d > 0.0) h = V == r ? (g - b) / d : V == g ? 2.0 + (b - r) / d : 4.0 + (r - g) / d;
    h = h + 6.0 * dh;
    h = h - 6.0 * floor(h / 6.0);
    if (!(h >= 0.0 && h < 6.0)) h = 0.0;
    const double S = V > 0.0 ? d / V : 0.0;
    const double Sg = S * gs, Vg = V * gv;
    const double S2 = Sg < 1.0 ? Sg : 1.0, V2 = Vg < 255.0 ? Vg : 255.0;
    const double fi = floor(h), f = h - fi;
    const double p = V2 * (1.0 - S2), q = V2 * (1.0 - S2 * f), t = V2 * (1.0 - S2 * (1.0 - f));
    const int i = (int)fi;                                            // 0 .. 5
    const double R = i == 0 || i == 5 ? V2 : i == 1 ? q : i == 4 ? t : p;
    const double G = i == 1 || i == 2 ? V2 : i == 0 ? t : i == 3 ? q : p;
    const double B = i == 3 || i == 4 ? V2 : i == 2 ? t : i == 5 ? q : p;
    px[0] = (uint8_t)fmin(255.0, floor(R + 0.5));
    px[1] = (uint8_t)fmin(255.0, floor(G + 0.5));
    px[2] = (uint8_t)fmin(255.0, floor(B + 0.5));
}

extern "C" int yk_hsv_jitter_u8(uint8_t *d_frames, int n, int h, int w, const double *d_params, void *stream) {
    if (n < 0 || h <= 0 || w <= 0 || (n > 0 && (!d_frames || !d_params))) {
        yk_set_error("yk_hsv_jitter_u8: bad argument");
        return YK_ERR_ARG;
    }
    if (n == 0) return YK_OK;
    const size_t per = (size_t)h * w;                                 // < 2^62
    if ((size_t)n > (size_t)-1 / 3 / per) {                           // 3*n*h*w bytes must be addressable
        yk_set_error("yk_hsv_jitter_u8: %d frames of %d x %d overflow size_t", n, h, w);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_hsv_jitter_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    const size_t total = (size_t)n * per;
    const size_t chunk = (size_t)1 << 30;                             // pixels per launch: one launch for any batch the pipeline makes
    for (size_t first = 0; first < total; first += chunk) {
        const size_t m = total - first < chunk ? total - first : chunk;
        hipLaunchKernelGGL(hsv_jitter_u8_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_frames, first,
                           first + m, per, d_params);
    }
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// ---- `img / np.max(img)` (tools/utils.py:405) for a batch of u8 frames -> fp32, for the TRAINING input pipeline (the inference
// path fuses it into the stem conv).  numpy divides in float64 and the pipeline then casts to float32 (utils.py:436 py_function
// output type): one correctly rounded quotient per element.
__global__ void __launch_bounds__(1024) u8_image_max_kernel(const uint8_t *__restrict__ f, size_t per_image, unsigned *__restrict__ mx) {
    __shared__ unsigned part[16];
    const uint8_t *p = f + (size_t)blockIdx.x * per_image;
    unsigned m = 0;
    size_t done = 0;
    if ((((uintptr_t)p) & 15) == 0) {                              // 16 bytes per load (byte loads: 210 dependent-latency loads per thread, 28 us)
        const size_t nv = per_image / 16;
        const uint4 *v = reinterpret_cast<const uint4 *>(p);
        unsigned a = 0;                                           // byte-wise max of the four lanes of a dword, folded at the end
        for (size_t i = threadIdx.x; i < nv; i += 1024) {
            const uint4 q = v[i];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // per-byte max of a and w[k]: compare byte lanes separately (no carries between them)
                const unsigned lo_a = a & 0x00ff00ffu, lo_w = w[k] & 0x00ff00ffu, hi_a = (a >> 8) & 0x00ff00ffu, hi_w = (w[k] >> 8) & 0x00ff00ffu;
                const unsigned lo = max(lo_a & 0xffffu, lo_w & 0xffffu) | (max(lo_a >> 16, lo_w >> 16) << 16);
                const unsigned hi = max(hi_a & 0xffffu, hi_w & 0xffffu) | (max(hi_a >> 16, hi_w >> 16) << 16);
                a = lo | (hi << 8);
            }
        }
        m = max(max(a & 255u, (a >> 8) & 255u), max((a >> 16) & 255u, a >> 24));
        done = nv * 16;
    }
    for (size_t i = done + threadIdx.x; i < per_image; i += 1024) m = max(m, (unsigned)p[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = max(m, part[i]);
        mx[blockIdx.x] = m;
    }
}
__global__ void __launch_bounds__(256) u8_normalise_kernel(const uint8_t *__restrict__ f, size_t per_image, const unsigned *__restrict__ mx,
                                                           float *__restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const unsigned m = mx[i / per_image];
    out[i] = (float)((double)f[i] / (double)m);                   // max 0 -> nan/inf exactly like numpy's 0/0 (an all-black image)
}
extern "C" int yk_normalise_u8(const uint8_t *d_frames, int batch, size_t per_image, float *d_out, void *stream) {
    if (!d_frames || !d_out || batch <= 0 || per_image == 0) {
        yk_set_error("yk_normalise_u8: bad argument");
        return YK_ERR_ARG;
    }
    const int dev = yk_current_device();
    if (dev < 0) {
        yk_set_error("yk_normalise_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    unsigned *mx = (unsigned *)yk_scratch(dev, stream, YK_SLOT_NORMALISE, sizeof(unsigned) * (size_t)batch);
    if (!mx) return YK_ERR_NOMEM;
    hipLaunchKernelGGL(u8_image_max_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, d_frames, per_image, mx);
    const size_t total = (size_t)batch * per_image;
    hipLaunchKernelGGL(u8_normalise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_frames, per_image, mx,
                       d_out, total);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
