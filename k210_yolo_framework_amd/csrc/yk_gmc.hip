// yk_gmc.hip — the camera's translation between consecutive frames, for the tracker (k210_yolo_framework_amd/gmc.py states the rule: block
// matching on shrunk grey pictures, integers only).  Three launches per call, no host read, no atomics, no floating point
// before the one conversion of the result:
//   gmc_shrink_kernel   one thread per small pixel: f rows of 3 f bytes of the packed original, read as the aligned dwords that cover them
//                       (rows start at any byte: a picture's width need not be a multiple of 4), grey and the rounded cell average; every
//                       small picture of the batch goes into one arena in the state.
//   gmc_match_kernel    the hot one.  ONE WAVEFRONT PER BLOCK: the block (B x B of the previous small picture) and its (B + 2R)^2 window of
//                       the current one lie in LDS; lanes own candidates (lane, lane + 64, ...: 289 of them at R = 8, five per lane), each
//                       accumulating its SAD four bytes at a time with v_sad_u8.  A candidate's window row starts at byte dx of the row, so
//                       its dwords are assembled from two aligned ones with v_alignbyte_b32 (B / 4 + 1 LDS reads per row for B / 4 SADs).
//                       WHY NOT four byte-shifted copies of the window: lanes with consecutive dx then read four different copies - 64
//                       distinct dwords per read, two passes of the 32 banks at the least - where here four consecutive lanes share one
//                       dword and a row of 17 candidates touches 6; with the window's rows 8 dwords apart the wave's 4 rows of candidates
//                       fall on banks 0-5, 8-13, 16-21, 24-29: no conflict, mostly broadcast, and 1 KB of LDS not 4.  The block's own row
//                       is read once per row (the same address in every lane) and kept in registers across the lane's candidates.
//                       WHY NOT a workgroup per strip of blocks sharing windows: the window is 1 KB read once from L2 per block against
//                       74 K byte differences; loading is not what the time goes to.  The arg-min is a wave reduction over one packed
//                       64-bit key (sad, |dy|+|dx|, dy + R, dx + R) - the tie rule is the key's order; the texture test a wave min / max.
//   gmc_median_kernel   one wavefront per frame: the frame's answers go into LDS; lane v counts the kept blocks whose dx (then dy) is v - R,
//                       a wave prefix sum ranks them and the first lane whose cumulative count passes (n - 1) / 2 is the lower median.  The
//                       wave of a sequence's last frame then copies that small picture beside the sequence's header, where the first frame
//                       of the next call finds it.
#include "yk_common.h"

#define YK_GMC_CHUNK 5                    // candidates a lane carries through one pass over the block's rows (5 x 64 >= 17^2)

struct gmc_args {
    int f, B, R, S, texture, min_blocks, n_seq, n_frames, P;
    int PS, MB, MBS;                      // a small picture's stride in bytes, the call's blocks per frame (grid), the state's stride of answers
    int32_t *head;                        // [n_seq][4] (h, w) of the sequence's last picture, (0, 0): none
    uint8_t *last, *arena;                // [n_seq][PS], [max_frames][PS]
    int32_t *res, *finfo;                 // [max_frames][MBS] (dy + R) << 8 | (dx + R) of a kept block, -1 of a dropped one; [max_frames] blocks matched
    const uint8_t *buf;
    size_t src_bytes;
    const yk_ragged_row_t *table;
    const int32_t *seq_first;
};

struct gmc_geom {
    int sh, sw, ni, nj;                   // the small picture, blocks down and across
    bool ok;                              // the row is a picture inside the buffer whose small picture fits the state
};

__device__ __forceinline__ gmc_geom gmc_geom_of(const yk_ragged_row_t &row, const gmc_args &a) {
    gmc_geom g = {0, 0, 0, 0, false};
    if (!yk_ragged_row_inside(row, a.src_bytes)) return g;
    g.sh = row.h / a.f;
    g.sw = row.w / a.f;
    if ((long long)g.sh * g.sw > a.P) return g;
    const int t = a.B + 2 * a.R;
    g.ni = g.sh >= t ? (g.sh - t) / a.S + 1 : 0;
    g.nj = g.sw >= t ? (g.sw - t) / a.S + 1 : 0;
    g.ok = true;
    return g;
}

// The sequence that owns frame f - the lowest s with first[s] <= f < first[s + 1], both clamped to [0, n_frames] as yk_track_update clamps
// them - and its frames f0 .. f1 - 1, or -1.  Called by a whole wavefront.
__device__ __forceinline__ int gmc_seq_of(const gmc_args &a, int f, int lane, int &f0, int &f1) {
    for (int base = 0; base < a.n_seq; base += 64) {
        const int s = base + lane;
        int lo = 0, hi = 0;
        if (s < a.n_seq) {
            lo = min(max(a.seq_first[s], 0), a.n_frames);
            hi = min(max(a.seq_first[s + 1], 0), a.n_frames);
        }
        const unsigned long long m = __ballot(lo <= f && f < hi);
        if (m) {
            const int src = __ffsll(m) - 1;
            f0 = __shfl(lo, src, 64);
            f1 = __shfl(hi, src, 64);
            return base + src;
        }
    }
    return -1;
}

// the small picture frame f is matched against: the frame before it in its sequence, of the same size - or NULL.  A whole wavefront.
__device__ __forceinline__ const uint8_t *gmc_prev_of(const gmc_args &a, int f, const yk_ragged_row_t &row, int lane) {
    int f0, f1;
    const int s = gmc_seq_of(a, f, lane, f0, f1);
    if (s < 0) return nullptr;
    if (f == f0) {
        const int32_t *hd = a.head + 4 * (size_t)s;
        return (hd[0] == row.h && hd[1] == row.w) ? a.last + (size_t)s * a.PS : nullptr;
    }
    const yk_ragged_row_t p = a.table[f - 1];
    return (p.h == row.h && p.w == row.w && yk_ragged_row_inside(p, a.src_bytes)) ? a.arena + (size_t)(f - 1) * a.PS : nullptr;
}

// the four bytes at `at` (a multiple of 4; buf is 4-byte aligned) of a buffer of n bytes; bytes past its end read as 0 and are not fetched
__device__ __forceinline__ uint32_t gmc_ld4(const uint8_t *buf, size_t n, size_t at) {
    if (at + 4 <= n) return *reinterpret_cast<const uint32_t *>(buf + at);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (at + k < n) v |= (uint32_t)buf[at + k] << (8 * k);
    return v;
}

// grid (n_frames * ceil(P / 256)), 256 threads: thread = small pixel
__global__ void __launch_bounds__(256) gmc_shrink_kernel(gmc_args a) {
    const int per = (a.P + 255) / 256;
    const int f = blockIdx.x / per, p = (blockIdx.x % per) * 256 + threadIdx.x;
    const yk_ragged_row_t row = a.table[f];
    const gmc_geom g = gmc_geom_of(row, a);
    if (!g.ok || p >= g.sh * g.sw) return;
    const int y = p / g.sw, x = p % g.sw, n = 3 * a.f;
    const size_t pitch = 3 * (size_t)row.w;
    uint32_t sum = 0;
    for (int r = 0; r < a.f; ++r) {
        const size_t at = row.offset + ((size_t)y * a.f + r) * pitch + (size_t)x * n;
        const int sh = (int)(at & 3);
        const size_t base = at - sh;
        uint32_t word = 0, acc = 0;
        int c = 0;
        for (int i = 0; i < n; ++i) {
            const int pos = sh + i;
            if (i == 0 || (pos & 3) == 0) word = gmc_ld4(a.buf, a.src_bytes, base + (size_t)(pos & ~3));
            const uint32_t v = (word >> (8 * (pos & 3))) & 255u;
            acc += (c == 0 ? 77u : c == 1 ? 150u : 29u) * v;
            if (++c == 3) {
                sum += (acc + 128u) >> 8;
                acc = 0;
                c = 0;
            }
        }
    }
    const uint32_t cell = (uint32_t)(a.f * a.f);
    a.arena[(size_t)f * a.PS + p] = (uint8_t)((sum + cell / 2) / cell);
}

// grid (n_frames * MB), one wavefront: workgroup = block b of frame f.  BT: the block's side at compile time (its row then lives in
// registers), 0: a.B.  Dynamic LDS: the window [W][WS] (W = B + 2R, WS = W rounded up to 4) + 4 bytes, then the block [B][B].
template <int BT>
__global__ void __launch_bounds__(64) gmc_match_kernel(gmc_args a, int32_t *__restrict__ blocks_out) {
    extern __shared__ uint32_t gmc_lds[];
    const int lane = threadIdx.x, f = blockIdx.x / a.MB, b = blockIdx.x % a.MB;
    const int B = BT ? BT : a.B, R = a.R, Bq = B >> 2;
    const yk_ragged_row_t row = a.table[f];
    const gmc_geom g = gmc_geom_of(row, a);
    const uint8_t *prev = g.ok ? gmc_prev_of(a, f, row, lane) : nullptr;
    const int nb = prev ? g.ni * g.nj : 0;
    if (b == 0 && lane == 0) a.finfo[f] = nb;
    if (b >= nb) return;
    const uint8_t *cur = a.arena + (size_t)f * a.PS;
    const int y0 = (b / g.nj) * a.S, x0 = (b % g.nj) * a.S;            // the window's corner; the block's is R further in
    const int W = B + 2 * R, WS = (W + 3) & ~3, WQ = WS >> 2;
    uint8_t *win = reinterpret_cast<uint8_t *>(gmc_lds), *blk = win + W * WS + 4;
    const uint32_t *win4 = gmc_lds, *blk4 = gmc_lds + W * WQ + 1;
    for (int i = lane; i < W * WQ + 1; i += 64) gmc_lds[i] = 0;         // (the padding is read, never used: alignbyte by 0 drops it)
    __syncthreads();
    for (int i = lane; i < W * W; i += 64) {
        const int y = i / W, x = i % W;
        win[y * WS + x] = cur[(size_t)(y0 + y) * g.sw + x0 + x];
    }
    int lo = 255, hi = 0;
    for (int i = lane; i < B * B; i += 64) {
        const int y = i / B, x = i % B, v = prev[(size_t)(y0 + R + y) * g.sw + x0 + R + x];
        blk[i] = (uint8_t)v;
        lo = min(lo, v);
        hi = max(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    __syncthreads();

    const int side = 2 * R + 1, ncand = side * side;
    unsigned long long best = ~0ull;
    for (int c0 = 0; c0 < ncand; c0 += 64 * YK_GMC_CHUNK) {
        int d0[YK_GMC_CHUNK], sh[YK_GMC_CHUNK];
        uint32_t sad[YK_GMC_CHUNK];
#pragma unroll
        for (int k = 0; k < YK_GMC_CHUNK; ++k) {                        // (a lane past the last candidate scores the last one again, unused)
            const int c = min(c0 + 64 * k + lane, ncand - 1), cy = c / side, cx = c % side;
            d0[k] = cy * WQ + (cx >> 2);
            sh[k] = cx & 3;
            sad[k] = 0;
        }
        for (int y = 0; y < B; ++y) {
            uint32_t mine[BT ? BT / 4 : 1];
            if constexpr (BT != 0) {
#pragma unroll
                for (int q = 0; q < BT / 4; ++q) mine[q] = blk4[y * Bq + q];
            }
#pragma unroll
            for (int k = 0; k < YK_GMC_CHUNK; ++k) {
                const uint32_t *w = win4 + d0[k] + y * WQ;
                uint32_t low = w[0];
                if constexpr (BT != 0) {
#pragma unroll
                    for (int q = 0; q < BT / 4; ++q) {
                        const uint32_t high = w[q + 1];
                        sad[k] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(high, low, (uint32_t)sh[k]), mine[q], sad[k]);
                        low = high;
                    }
                } else {
                    for (int q = 0; q < Bq; ++q) {
                        const uint32_t high = w[q + 1];
                        sad[k] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(high, low, (uint32_t)sh[k]), blk4[y * Bq + q], sad[k]);
                        low = high;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < YK_GMC_CHUNK; ++k) {
            const int c = c0 + 64 * k + lane;
            if (c < ncand) {
                const int cy = c / side, cx = c % side;
                const unsigned long long key = ((unsigned long long)sad[k] << 32) | ((unsigned)(abs(cy - R) + abs(cx - R)) << 16) |
                                               ((unsigned)cy << 8) | (unsigned)cx;
                best = key < best ? key : best;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if (lane == 0) {
        const int cy = (int)((best >> 8) & 255), cx = (int)(best & 255), kept = hi - lo >= a.texture;
        a.res[(size_t)f * a.MBS + b] = kept ? (cy << 8 | cx) : -1;
        if (blocks_out) {
            int32_t *o = blocks_out + ((size_t)f * a.MB + b) * 4;
            o[0] = cy - R;
            o[1] = cx - R;
            o[2] = (int32_t)(best >> 32);
            o[3] = kept;
        }
    }
}

// grid (n_frames), one wavefront; dynamic LDS: MB words
__global__ void __launch_bounds__(64) gmc_median_kernel(gmc_args a, float *__restrict__ motion) {
    extern __shared__ uint32_t gmc_lds[];
    int32_t *vals = reinterpret_cast<int32_t *>(gmc_lds);
    const int lane = threadIdx.x, f = blockIdx.x;
    const int nb = min(max(a.finfo[f], 0), a.MB);
    int kept = 0;
    for (int base = 0; base < nb; base += 64) {
        const int i = base + lane, v = i < nb ? a.res[(size_t)f * a.MBS + i] : -1;
        if (i < nb) vals[i] = v;
        kept += __popcll(__ballot(v >= 0));
    }
    __syncthreads();
    int m[2] = {0, 0};
    if (kept >= a.min_blocks) {
        const int target = (kept - 1) / 2;                               // the lower median's rank
        for (int axis = 0; axis < 2; ++axis) {                           // dx, then dy: lane v counts the value v - R (2R + 1 <= 33 lanes)
            int cnt = 0;
            for (int i = 0; i < nb; ++i) {
                const int v = vals[i];
                cnt += (v >= 0 && ((v >> (8 * axis)) & 255) == lane) ? 1 : 0;
            }
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            m[axis] = (__ffsll(__ballot(incl > target)) - 1 - a.R) * a.f;
        }
    }
    if (lane == 0) {
        motion[2 * (size_t)f] = (float)m[0];
        motion[2 * (size_t)f + 1] = (float)m[1];
    }
    // the last picture of a sequence outlives the call
    int f0, f1;
    const int s = gmc_seq_of(a, f, lane, f0, f1);
    if (s < 0 || f != f1 - 1) return;
    const yk_ragged_row_t row = a.table[f];
    const gmc_geom g = gmc_geom_of(row, a);
    if (g.ok) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.arena + (size_t)f * a.PS);
        uint32_t *dst = reinterpret_cast<uint32_t *>(a.last + (size_t)s * a.PS);
        for (int i = lane; i < (g.sh * g.sw + 3) / 4; i += 64) dst[i] = src[i];          // (PS is a multiple of 16: the tail stays inside)
    }
    if (lane == 0) {
        a.head[4 * (size_t)s] = g.ok ? row.h : 0;
        a.head[4 * (size_t)s + 1] = g.ok ? row.w : 0;
    }
}

__global__ void __launch_bounds__(64) gmc_reset_kernel(int32_t *__restrict__ head, int n_seq) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < n_seq) head[4 * (size_t)s] = head[4 * (size_t)s + 1] = head[4 * (size_t)s + 2] = head[4 * (size_t)s + 3] = 0;
}

#define YK_GMC_REFUSE(fn, cond, ...)            \
    if (cond) {                                 \
        yk_set_error(fn ": " __VA_ARGS__);      \
        return YK_ERR_ARG;                      \
    }
#define YK_GMC_STATE_ARGS(fn)                                                                                                        \
    YK_GMC_REFUSE(fn, n_seq <= 0, "n_seq %d: expected at least 1", n_seq)                                                            \
    YK_GMC_REFUSE(fn, max_frames <= 0, "max_frames %d: expected at least 1", max_frames)                                             \
    YK_GMC_REFUSE(fn, max_small_pixels <= 0 || max_small_pixels > (1 << 28), "max_small_pixels %d: expected 1 .. 2^28", max_small_pixels)

static size_t gmc_stride(int max_small_pixels) { return ((size_t)max_small_pixels + 15) & ~(size_t)15; }
static int gmc_answers(int max_small_pixels) { return max_small_pixels < YK_GMC_MAX_BLOCKS ? max_small_pixels : YK_GMC_MAX_BLOCKS; }

// the state's sections, all 16-byte aligned: headers | last pictures | arena | answers | blocks matched per frame -> its size
static size_t gmc_carve(void *state, int n_seq, int max_frames, int max_small_pixels, gmc_args *a) {
    const size_t ps = gmc_stride(max_small_pixels), mbs = (size_t)gmc_answers(max_small_pixels);
    uint8_t *at = static_cast<uint8_t *>(state);
    size_t used = 0;
    auto take = [&](size_t bytes) {
        uint8_t *p = at + used;
        used += (bytes + 15) & ~(size_t)15;
        return p;
    };
    uint8_t *head = take(16 * (size_t)n_seq), *last = take(ps * n_seq), *arena = take(ps * max_frames);
    uint8_t *res = take(4 * mbs * max_frames), *finfo = take(4 * (size_t)max_frames);
    if (a) {
        a->head = reinterpret_cast<int32_t *>(head);
        a->last = last;
        a->arena = arena;
        a->res = reinterpret_cast<int32_t *>(res);
        a->finfo = reinterpret_cast<int32_t *>(finfo);
        a->PS = (int)ps;
        a->MBS = (int)mbs;
    }
    return used;
}

extern "C" int yk_gmc_state_bytes(int n_seq, int max_frames, int max_small_pixels, size_t *bytes) {
    YK_GMC_STATE_ARGS("yk_gmc_state_bytes")
    YK_GMC_REFUSE("yk_gmc_state_bytes", !bytes, "bytes is NULL")
    *bytes = gmc_carve(nullptr, n_seq, max_frames, max_small_pixels, nullptr);
    return YK_OK;
}

extern "C" int yk_gmc_reset(void *d_state, int n_seq, void *stream) {
    YK_GMC_REFUSE("yk_gmc_reset", !d_state, "d_state is NULL")
    YK_GMC_REFUSE("yk_gmc_reset", n_seq <= 0, "n_seq %d: expected at least 1", n_seq)
    hipLaunchKernelGGL(gmc_reset_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int32_t *)d_state, n_seq);
    YK_HIP(hipGetLastError());
    return YK_OK;
}

// fn: the entry point the refusal names.  -> the most blocks a frame of cfg->max_small_pixels can have (at least 1), or an error
static int gmc_max_blocks(const char *fn, const yk_gmc_cfg_t *cfg) {
#define R(cond, ...)                            \
    if (cond) {                                 \
        yk_set_error(__VA_ARGS__);              \
        return YK_ERR_ARG;                      \
    }
    R(!cfg, "%s: cfg is NULL", fn)
    R(cfg->scale < 1 || cfg->scale > 64, "%s: cfg->scale %d: expected f in 1 .. 64", fn, cfg->scale)
    R(cfg->block < 4 || cfg->block > YK_GMC_MAX_BLOCK || cfg->block % 4, "%s: cfg->block %d: expected B, a multiple of 4 in 4 .. %d", fn, cfg->block,
      YK_GMC_MAX_BLOCK)
    R(cfg->range < 1 || cfg->range > YK_GMC_MAX_RANGE, "%s: cfg->range %d: expected R in 1 .. %d", fn, cfg->range, YK_GMC_MAX_RANGE)
    R(cfg->step < 1 || cfg->step > 4096, "%s: cfg->step %d: expected S in 1 .. 4096", fn, cfg->step)
    R(cfg->texture < 0 || cfg->texture > 256, "%s: cfg->texture %d: expected 0 .. 256", fn, cfg->texture)
    R(cfg->min_blocks < 1, "%s: cfg->min_blocks %d: expected at least 1", fn, cfg->min_blocks)
    R(cfg->max_small_pixels <= 0 || cfg->max_small_pixels > (1 << 28), "%s: cfg->max_small_pixels %d: expected 1 .. 2^28", fn, cfg->max_small_pixels)
#undef R
    // blocks down <= sh / m and across <= sw / m with m = min(S, B + 2R), and sh * sw <= max_small_pixels
    const long long m = cfg->step < cfg->block + 2 * cfg->range ? cfg->step : cfg->block + 2 * cfg->range;
    const long long n = cfg->max_small_pixels / (m * m);
    if (n > YK_GMC_MAX_BLOCKS) {
        yk_set_error("%s: a picture of cfg->max_small_pixels %d can have %lld blocks at step %d, and the median's LDS holds %d of a frame; raise "
                     "cfg->step or cfg->scale", fn, cfg->max_small_pixels, n, cfg->step, YK_GMC_MAX_BLOCKS);
        return YK_ERR_ARG;
    }
    return n < 1 ? 1 : (int)n;
}

extern "C" int yk_gmc_max_blocks(const yk_gmc_cfg_t *cfg) { return gmc_max_blocks("yk_gmc_max_blocks", cfg); }

extern "C" int yk_gmc_motion_u8(void *d_state, const uint8_t *d_buf, size_t src_bytes, const yk_ragged_row_t *d_table, const int32_t *d_seq_first,
                                int n_frames, const yk_gmc_cfg_t *cfg, float *d_motion, int32_t *d_blocks, void *stream) {
#define R(cond, ...) YK_GMC_REFUSE("yk_gmc_motion_u8", cond, __VA_ARGS__)
    R(!d_state, "d_state is NULL")
    R(!d_buf, "d_buf is NULL")
    R(((uintptr_t)d_buf & 3) != 0, "d_buf is not 4-byte aligned")
    R(src_bytes == 0, "src_bytes is 0")
    R(!d_table, "d_table is NULL")
    R(!d_seq_first, "d_seq_first is NULL")
    R(!d_motion, "d_motion is NULL")
    const int mb = gmc_max_blocks("yk_gmc_motion_u8", cfg);
    if (mb < 0) return mb;
    R(cfg->n_seq <= 0, "cfg->n_seq %d: expected at least 1", cfg->n_seq)
    R(cfg->max_frames <= 0, "cfg->max_frames %d: expected at least 1", cfg->max_frames)
    R(n_frames <= 0 || n_frames > cfg->max_frames, "n_frames %d: expected 1 .. cfg->max_frames %d", n_frames, cfg->max_frames)
    const long long per = ((long long)cfg->max_small_pixels + 255) / 256;
    R(per * n_frames > 0x7fffffffLL || (long long)mb * n_frames > 0x7fffffffLL, "n_frames %d x cfg->max_small_pixels %d: 2^31 workgroups or more",
      n_frames, cfg->max_small_pixels)
#undef R
    gmc_args a;
    gmc_carve(d_state, cfg->n_seq, cfg->max_frames, cfg->max_small_pixels, &a);
    a.f = cfg->scale;
    a.B = cfg->block;
    a.R = cfg->range;
    a.S = cfg->step;
    a.texture = cfg->texture;
    a.min_blocks = cfg->min_blocks;
    a.n_seq = cfg->n_seq;
    a.n_frames = n_frames;
    a.P = cfg->max_small_pixels;
    a.MB = mb;
    a.buf = d_buf;
    a.src_bytes = src_bytes;
    a.table = d_table;
    a.seq_first = d_seq_first;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gmc_shrink_kernel, dim3((unsigned)(per * n_frames)), dim3(256), 0, st, a);
    const int W = a.B + 2 * a.R, WS = (W + 3) & ~3;
    const size_t lds = (size_t)W * WS + 4 + (size_t)a.B * a.B;
    const dim3 grid((unsigned)((long long)mb * n_frames));
    if (a.B == 16) hipLaunchKernelGGL(gmc_match_kernel<16>, grid, dim3(64), lds, st, a, d_blocks);
    else if (a.B == 8) hipLaunchKernelGGL(gmc_match_kernel<8>, grid, dim3(64), lds, st, a, d_blocks);
    else hipLaunchKernelGGL(gmc_match_kernel<0>, grid, dim3(64), lds, st, a, d_blocks);
    hipLaunchKernelGGL(gmc_median_kernel, dim3((unsigned)n_frames), dim3(64), (size_t)mb * 4, st, a, d_motion);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
