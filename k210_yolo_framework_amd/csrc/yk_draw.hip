// yk_draw.hip — detections painted into the ORIGINAL pictures while they are still in device memory (`make detect`):
// the box outlines of inference.py's ImageDraw.rectangle loop and the label of keras_inference.py:137-174 - a filled background in the
// class colour with '{:2d} {:.2f}'.format(class, score) on it - from the project's own bitmap glyphs (draw.py).  The rule is stated in
// include/yolo_hip.h (yk_draw_dets_u8); this file is built with -ffp-contract=off.
//
// Structure: GATHER per pixel.  A thread owns one pixel of one picture (blockIdx.y = picture, blockIdx.x * 256 + threadIdx.x = pixel,
// early exit past the picture's end).  The painter's rule says the LAST primitive that covers a pixel wins, so the thread walks the
// picture's rows from the last to the first - and inside a row text, background, outline - and stops at the first hit: one write per
// covered pixel, none for the others, no atomics, no ordering between workgroups, the same bytes on every run.
// A workgroup stages the rows 256 at a time in LDS as integer rectangles (one row per thread, 10 KB), from the last chunk to the first;
// a row that cannot touch the image rows of this workgroup's 256 pixels is staged empty, and a chunk without any live row is not scanned.
#include "yk_common.h"

#define DRAW_CHUNK 256
#define GLYPH_SPACE 11
#define GLYPH_DOT 10

struct draw_ent {
    int l, t, r, b;     // inclusive rectangle of ring 0; l > r: the row draws nothing here
    int rings;          // outline rings j = 0 .. rings - 1
    int lw, lh;         // label rectangle at (l, t + 1): lw x lh pixels
    unsigned colour;    // r | g << 8 | b << 16
    unsigned g03, g46;  // the 7 glyph indices, one byte each
};

// '{:2d} {:.2f}'.format(cls, score) as 7 glyph indices (0-9 digits, 10 '.', 11 ' ').  (double)score * 100.0 is exact (24 bits x 7 bits),
// so rint - half to even - of it is the correctly rounded two-decimal value of the fp32 score: Python's digits for every score in [0, 1].
__device__ __forceinline__ void label_glyphs(float cls_f, float score, unsigned *g03, unsigned *g46) {
    const int cls = cls_f >= 0.0f ? (int)fminf(cls_f, 1.0e9f) : 0;                          // negative or NaN: 0
    const double s = (score >= 0.0f && score <= 3.0e38f) ? fmin(rint((double)score * 100.0), 1.0e15) : 0.0;   // negative or non-finite: 0.00
    const long long s100 = (long long)s;
    const unsigned tens = (unsigned)((cls / 10) % 10), ones = (unsigned)(cls % 10);
    *g03 = (cls < 10 ? GLYPH_SPACE : tens) | ones << 8 | GLYPH_SPACE << 16 | (unsigned)((s100 / 100) % 10) << 24;
    *g46 = GLYPH_DOT | (unsigned)((s100 / 10) % 10) << 8 | (unsigned)(s100 % 10) << 16;
}

__global__ void __launch_bounds__(256) draw_dets_u8_kernel(uint8_t *__restrict__ buf, size_t src_bytes, const yk_ragged_row_t *__restrict__ table,
                                                           const float *__restrict__ dets, int cap, const int32_t *__restrict__ counts,
                                                           const uint8_t *__restrict__ colours, int n_colours,
                                                           const uint8_t *__restrict__ atlas, int gh, int gw, size_t max_pixels) {
    __shared__ draw_ent ents[DRAW_CHUNK];
    const int img = blockIdx.y;
    const yk_ragged_row_t row = table[img];
    const int h = row.h, w = row.w;
    if (!yk_ragged_row_inside(row, src_bytes)) return;                                                          // uniform: the whole workgroup
    size_t npx = (size_t)h * w;
    if (npx > max_pixels) npx = max_pixels;
    const size_t first = (size_t)blockIdx.x * 256;
    if (first >= npx) return;                                                                                   // uniform
    int count = counts[img];
    count = count < 0 ? 0 : (count > cap ? cap : count);
    if (count == 0) return;                                                                                     // uniform
    const size_t last = first + 255 < npx ? first + 255 : npx - 1;
    const int y_first = (int)(first / w), y_last = (int)(last / w);           // image rows this workgroup's pixels lie on
    const size_t idx = first + threadIdx.x;
    const bool live = idx < npx;
    const int x = (int)(idx % w), y = (int)(idx / w);
    const int mag = row.mag < 1 ? 1 : (row.mag > 1024 ? 1024 : row.mag), thick = row.thickness < 1 ? 1 : row.thickness;   // mag bounded: no overflow below
    const int cell = gw * mag;                                                // one glyph cell, pixels
    const int lw = gh > 0 ? 7 * cell : 0, lh = gh * mag;
    const float *drows = dets + (size_t)img * cap * 6;

    bool hit = false;
    unsigned paint = 0;
    for (int base = ((count - 1) / DRAW_CHUNK) * DRAW_CHUNK; base >= 0; base -= DRAW_CHUNK) {
        const int nk = count - base < DRAW_CHUNK ? count - base : DRAW_CHUNK;
        int touches = 0;
        if ((int)threadIdx.x < nk) {
            const float *d = drows + (size_t)(base + threadIdx.x) * 6;
            // clamped as floats first, so that no conversion overflows; t <= h and b >= 0 change no decision (such a row has b <= t)
            const int t = (int)fminf(fmaxf(0.0f, floorf(d[0] + 0.5f)), (float)h), l = (int)fminf(fmaxf(0.0f, floorf(d[1] + 0.5f)), (float)w);
            const int b = (int)fmaxf(fminf((float)h, floorf(d[2] + 0.5f)), 0.0f), r = (int)fmaxf(fminf((float)w, floorf(d[3] + 0.5f)), 0.0f);
            draw_ent e;
            e.l = 1, e.r = 0, e.t = 1, e.b = 0, e.rings = 0, e.lw = 0, e.lh = 0, e.colour = 0, e.g03 = 0, e.g46 = 0;
            const int y_end = b > t + lh ? b : t + lh;                        // last image row the row's paint can reach
            if (b > t && r > l && t <= y_last && y_end >= y_first) {
                e.l = l, e.t = t, e.r = r, e.b = b;
                const int rw = (r - l + 1) / 2, rh = (b - t + 1) / 2;         // rings with r - j > l + j, and with b - j > t + j
                e.rings = thick < rw ? (thick < rh ? thick : rh) : (rw < rh ? rw : rh);
                e.lw = lw, e.lh = lh;
                const int cls = d[5] >= 0.0f ? (int)fminf(d[5], 1.0e9f) : 0;
                const uint8_t *c = colours + (size_t)(cls % n_colours) * 3;
                e.colour = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
                label_glyphs(d[5], d[4], &e.g03, &e.g46);
                touches = 1;
            }
            ents[threadIdx.x] = e;
        }
        if (__syncthreads_or(touches)) {                                      // (also the barrier after staging)
            if (live && !hit) {
                for (int k = nk - 1; k >= 0; --k) {
                    const draw_ent &e = ents[k];                              // every lane reads the same entry: an LDS broadcast
                    const int dx = x - e.l, dy = y - e.t - 1;
                    if (dx < 0 || y < e.t) continue;
                    if (dx < e.lw && dy >= 0 && dy < e.lh) {                  // label: text over background
                        const int slot = dx / cell, gx = (dx - slot * cell) / mag, gy = dy / mag;
                        const unsigned g = ((slot < 4 ? e.g03 >> (8 * slot) : e.g46 >> (8 * (slot - 4))) & 255u);
                        paint = atlas[((size_t)g * gh + gy) * gw + gx] ? 0u : e.colour;
                        hit = true;
                        break;
                    }
                    if (x <= e.r && y <= e.b) {                               // outline: ring `depth` of the inclusive rectangle
                        const int dxr = e.r - x, dyb = e.b - y, dyt = y - e.t;
                        const int depth = min(min(dx, dxr), min(dyt, dyb));
                        if (depth < e.rings) {
                            paint = e.colour;
                            hit = true;
                            break;
                        }
                    }
                }
            }
        }
        __syncthreads();                                                      // the next chunk overwrites ents
    }
    if (hit) {
        uint8_t *o = buf + row.offset + idx * 3;
        o[0] = (uint8_t)(paint & 255u);
        o[1] = (uint8_t)((paint >> 8) & 255u);
        o[2] = (uint8_t)((paint >> 16) & 255u);
    }
}

extern "C" int yk_draw_dets_u8(uint8_t *d_buf, size_t src_bytes, const yk_ragged_row_t *d_table, int n, const float *d_dets, int cap,
                               const int32_t *d_counts, const uint8_t *d_colors, int n_colors, const uint8_t *d_atlas, int gh, int gw,
                               size_t max_pixels, void *stream) {
    if (!d_buf || !d_table || !d_dets || !d_counts || !d_colors || (!d_atlas && gh != 0) || n <= 0 || cap <= 0 || n_colors <= 0 || gh < 0 ||
        gw <= 0 || src_bytes == 0 || max_pixels == 0) {
        yk_set_error("yk_draw_dets_u8: bad argument");
        return YK_ERR_ARG;
    }
    const size_t blocks = (max_pixels + 255) / 256;
    if (blocks > 0x7fffffffu) {
        yk_set_error("yk_draw_dets_u8: max_pixels %zu is more than one launch covers", max_pixels);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_draw_dets_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    yk_for_grid_y(n, [&](int base, int m) {
        hipLaunchKernelGGL(draw_dets_u8_kernel, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, (hipStream_t)stream, d_buf, src_bytes,
                           d_table + base, d_dets + (size_t)base * cap * 6, cap, d_counts + base, d_colors, n_colors, d_atlas, gh, gw,
                           max_pixels);
    });
    YK_HIP(hipGetLastError());
    return YK_OK;
}
