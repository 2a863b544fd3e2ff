// yk_jpeg_dec.hip — baseline JPEG decoding of a batch of pictures into a ragged packed buffer on the device (`make detect DECODE=gpu`;
// DESIGN.md 3.12).  The host parses the files (jpeg.py: parse_baseline, plan_decode); the device gets the entropy-coded segments, one
// yk_jpeg_pic_t per picture and the decode-ready tables, and writes [h][w][3] u8 at the offsets of the yk_ragged_row_t table.  The rule
// from bit to pixel is integer and stated in include/yolo_hip.h, so tests/jpeg_dec_ref.py reproduces every byte.
//
// Structure (every launch on the caller's stream, nothing synchronises, everything can be recorded in a graph):
//   plan     one workgroup: checks every row against the capacities, blocks per picture scanned into blk_start[n + 1], d_status
//   zero     the coefficient array of the workspace: the Huffman stage stores only what the stream codes
//   huffman  one workgroup per picture, its four Huffman tables in LDS.  The stuffed stream is cut into chunks of chunk_bytes, one per
//            thread, 256 chunks per tile.  Every thread decodes from (chunk start, block 0, index 0) to the first symbol at or after the
//            next chunk's start, then takes its predecessor's exit state as its entry and decodes again until no entry changed (a Huffman
//            decoder started at a wrong place falls into step after a few symbols: Weissenberger & Schmidt); after j rounds the first j
//            chunks are right, so the loop ends after at most 256 rounds whatever the stream.  A segmented scan of (markers crossed,
//            blocks completed since the last marker) gives every chunk its first block; one more pass stores the coefficients.
//   dc       one workgroup per picture, one thread per MCU: the DC differences summed per component, segmented at restart intervals
//   idct     one wave per 8x8 block, one lane per sample: dequantise, clamp, columns, rows, level shift -> component planes (MCU-padded)
//   colour   one thread per luma sample of the padded planes: triangle upsampling of the chroma, YCbCr -> RGB, store inside h x w
// No read leaves the picture's segment, no store its blocks / planes / h*w*3 bytes: a corrupt stream gives wrong coefficients and a
// non-zero status, nothing else.
#include "yk_common.h"
#include "yk_jpeg_dec_tables.h"

#define JD_THREADS 256
#define JD_TABLE_BYTES 896u                   // one Huffman table: look u16 [256], maxcode i32 [16], delta i32 [16], vals u8 [256]
#define JD_PIC_TABLES (256u + 4u * JD_TABLE_BYTES)
#define JD_PER_BLOCK 192u                     // workspace bytes per 8x8 block: 64 int16 coefficients, 64 u8 samples
#define JD_MAX_BLOCKS (1u << 22)             // per picture
#define JD_ST_ROW 1                           // d_status bits
#define JD_ST_COUNT 2
#define JD_ST_TRAIL 4
#define JD_ST_MARKER 8
#define JD_ST_WORK 16

static inline size_t jd_a16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t jd_header_bytes(size_t n) { return jd_a16(4 * (n + 1)) + jd_a16(4 * n); }    // blk_start [n + 1], rounds [n]

// what the kernels need to know about a picture; blocks == 0: an invalid row
struct jd_geom {
    int bpm, nl, mw, mh;
    unsigned blocks;
};

__host__ __device__ static inline jd_geom jd_geometry(const yk_jpeg_pic_t &p) {
    jd_geom g = {0, 0, 0, 0, 0u};
    const bool grey = p.ncomp == 1 && p.hs == 1 && p.vs == 1;
    const bool colour = p.ncomp == 3 && ((p.hs == 1 && p.vs == 1) || (p.hs == 2 && p.vs == 1) || (p.hs == 2 && p.vs == 2));
    if (!(grey || colour) || p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535 || p.restart < 0 || p.restart > 65535) return g;
    for (int c = 0; c < p.ncomp; ++c)
        if (p.tq[c] > 3 || p.td[c] > 1 || p.ta[c] > 1) return g;
    g.nl = p.hs * p.vs;
    g.bpm = g.nl + (p.ncomp == 3 ? 2 : 0);
    g.mw = (p.w + 8 * p.hs - 1) / (8 * p.hs);
    g.mh = (p.h + 8 * p.vs - 1) / (8 * p.vs);
    const unsigned long long b = (unsigned long long)g.mw * g.mh * g.bpm;
    g.blocks = b > JD_MAX_BLOCKS ? 0u : (unsigned)b;
    return g;
}

// exclusive scan over the 256 threads of a workgroup; *total = the sum.  sh: 256 values of LDS.
__device__ __forceinline__ unsigned jd_block_scan(unsigned v, unsigned *sh, unsigned *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < JD_THREADS; o <<= 1) {
        const unsigned a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const unsigned incl = sh[t];
    *total = sh[JD_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ int jd_picture_of(const uint32_t *__restrict__ blk_start, int n, unsigned b) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(JD_THREADS) jd_plan_kernel(const yk_jpeg_pic_t *__restrict__ pics, const yk_ragged_row_t *__restrict__ rows, int n,
                                                             size_t scan_bytes, size_t table_bytes, size_t dst_bytes, unsigned cap,
                                                             uint32_t *__restrict__ blk_start, int32_t *__restrict__ status) {
    __shared__ unsigned sh[JD_THREADS];
    unsigned carry = 0;
    bool over = false;
    for (int base = 0; base < n; base += JD_THREADS) {
        const int i = base + threadIdx.x;
        unsigned cnt = 0;
        if (i < n) {
            const yk_jpeg_pic_t p = pics[i];
            const yk_ragged_row_t r = rows[i];
            const jd_geom g = jd_geometry(p);
            const size_t seg = ((size_t)p.scan_bytes + 3) & ~(size_t)3;       // whole words are loaded
            const bool ok = g.blocks > 0 && p.scan_bytes > 0 && p.scan_bytes < (1u << 28) && (p.scan_offset & 3) == 0 && p.scan_offset <= scan_bytes &&
                            seg <= scan_bytes - p.scan_offset && (p.table_offset & 3) == 0 && p.table_offset <= table_bytes &&
                            JD_PIC_TABLES <= table_bytes - p.table_offset && r.h == p.h && r.w == p.w && r.offset <= dst_bytes &&
                            (size_t)p.h * p.w * 3 <= dst_bytes - r.offset;
            if (ok) cnt = g.blocks;
            status[i] = ok ? 0 : JD_ST_ROW;
        }
        unsigned total;
        const unsigned excl = jd_block_scan(cnt, sh, &total);
        if (i < n) blk_start[i] = carry + excl;
        if (total > cap - carry) over = true;                                 // (carry <= cap <= 2^30, a group's total <= 256 * 2^22: no wrap)
        else carry += total;
    }
    __syncthreads();
    if (over) {                                                               // a workspace too small for this table: nothing is decoded
        for (int i = threadIdx.x; i <= n; i += JD_THREADS) {
            blk_start[i] = 0;
            if (i < n) status[i] |= JD_ST_WORK;
        }
    } else if (threadIdx.x == 0) {
        blk_start[n] = carry;
    }
}

__global__ void __launch_bounds__(JD_THREADS) jd_zero_kernel(uint4 *__restrict__ p, size_t count) {
    const size_t i = (size_t)blockIdx.x * JD_THREADS + threadIdx.x;
    if (i < count) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- the bit reader ---------------------------------------------------------------------------------------------------------------
// A position is a bit index into the stuffed segment; its byte is a data byte (never the 0x00 after an 0xFF), the 0xFF of a marker, or the
// end.  A window holds the next up to 5 data bytes from a byte index on: enough for one symbol (16 bits of code, 15 of value, 7 of offset).
struct jd_window {
    uint64_t bits;       // data bytes from bit 63 down, zeros beyond the barrier
    unsigned nd;         // data bytes in front of the barrier (a marker or the end of the segment), at most 5
    unsigned ffmask;     // bit b: data byte b is an 0xFF, a stuffed zero follows it
    unsigned barrier;    // its byte index, when nd < 5
};

struct jd_stream {
    const uint8_t *seg;  // 4-byte aligned
    unsigned end;        // bytes
    __device__ __forceinline__ unsigned byte(unsigned j) const { return j < end ? seg[j] : 0u; }
    __device__ __forceinline__ uint32_t word_be(unsigned k) const {          // bytes 4k .. 4k + 3, most significant first; k clamped
        const unsigned last = (end - 1) >> 2;
        return __builtin_bswap32(reinterpret_cast<const uint32_t *>(seg)[k < last ? k : last]);
    }
    __device__ __forceinline__ jd_window fetch(unsigned i) const {           // i < end
        jd_window w;
        const unsigned k = i >> 2, s = (i & 3) * 8;
        const uint32_t w0 = word_be(k), w1 = word_be(k + 1), w2 = word_be(k + 2);
        uint64_t v = ((((uint64_t)w0 << 32) | w1) << s) | ((((uint64_t)w2) << s) >> 32);       // bytes i .. i + 7
        const unsigned left = end - i;
        if (left < 8) v &= ~0ull << (8 * (8 - left));                         // nothing beyond the end is data, whatever the memory holds
        const uint64_t top = ~v | 0x0000000000FFFFFFull;                      // a zero byte here = an 0xFF among bytes i .. i + 4
        if (!((top - 0x0101010101010101ull) & ~top & 0x8080808080808080ull)) {
            w.bits = v & 0xFFFFFFFFFF000000ull;
            w.nd = left < 5 ? left : 5;
            w.ffmask = 0;
            w.barrier = end;
            return w;
        }
        w.bits = 0, w.nd = 0, w.ffmask = 0, w.barrier = end;
        unsigned j = i;
        bool open = true;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            if (open) {
                const unsigned c = byte(j), nx = byte(j + 1);
                if (j >= end || (c == 0xFFu && nx != 0u)) {
                    open = false;
                    w.barrier = j < end ? j : end;
                } else {
                    w.bits |= (uint64_t)c << (56 - 8 * b);
                    ++w.nd;
                    if (c == 0xFFu) w.ffmask |= 1u << b, j += 2;
                    else j += 1;
                }
            }
        }
        return w;
    }
};

struct jd_tables {       // LDS: DC0 DC1 AC0 AC1
    const uint32_t *words;
    __device__ __forceinline__ unsigned look(unsigned t, unsigned c) const {
        return (words[t * (JD_TABLE_BYTES / 4) + (c >> 1)] >> ((c & 1) * 16)) & 0xFFFFu;
    }
    __device__ __forceinline__ int maxcode(unsigned t, unsigned l) const { return (int)words[t * (JD_TABLE_BYTES / 4) + 128 + l - 1]; }
    __device__ __forceinline__ int delta(unsigned t, unsigned l) const { return (int)words[t * (JD_TABLE_BYTES / 4) + 144 + l - 1]; }
    __device__ __forceinline__ unsigned val(unsigned t, unsigned k) const {
        return (words[t * (JD_TABLE_BYTES / 4) + 160 + (k >> 2)] >> ((k & 3) * 8)) & 0xFFu;
    }
};

struct jd_pic {          // uniform per workgroup
    jd_stream in;
    jd_tables tab;
    unsigned sel_dc, sel_ac;     // 4 bits per block of the MCU: its table (DC: 0 / 1, AC: 2 / 3)
    int bpm, restart;
    unsigned blocks;
    int16_t *coef;               // the picture's blocks
};

struct jd_state {
    unsigned pos;        // bit position
    unsigned bk;         // block of the MCU << 8 | zigzag index
};

struct jd_counts {
    unsigned markers;    // crossed
    unsigned blocks;     // completed since the last marker crossed (all, when none was)
    unsigned flags;      // STORE: status bits
    unsigned endpos;     // STORE: the position behind the picture's last block, when this chunk completed it
};

// Decodes from st to the first symbol that starts at or after `limit` (a bit position).  STORE: gb = the picture's block index of the entry
// state's block and mk = the markers in front of it; coefficients go to their place, the DC as its difference.
template <bool STORE>
__device__ __forceinline__ jd_state jd_decode_chunk(const jd_pic &P, jd_state st, unsigned limit, unsigned gb, unsigned mk, jd_counts *out) {
    unsigned pos = st.pos, blk = st.bk >> 8, k = st.bk & 63u;
    jd_counts c = {0u, 0u, 0u, 0xFFFFFFFFu};
    const unsigned endbits = P.in.end * 8u;
    while (pos < limit) {
        if (STORE && gb >= P.blocks) break;                                   // the picture is complete: what follows is padding or trailing data
        const unsigned i = pos >> 3, off = pos & 7u;
        const jd_window w = P.in.fetch(i);
        if (w.nd == 0) {                                                      // a marker (i < end here: limit <= end)
            if (STORE) {
                ++mk;
                const unsigned want = mk * (unsigned)P.restart * (unsigned)P.bpm;
                if (P.restart == 0 || gb != want || blk != 0 || k != 0 || P.in.byte(i + 1) != 0xD0u + ((mk - 1) & 7u)) c.flags |= JD_ST_MARKER;
                if (P.restart != 0) gb = want;
            }
            if (P.restart != 0) ++c.markers, c.blocks = 0;
            pos = i + 2 < P.in.end ? (i + 2) * 8u : endbits;
            blk = 0, k = 0;
            continue;
        }
        const uint64_t x = w.bits << off;
        if (w.nd == 1) {                                                      // the last byte in front of a marker or the end: 1-bits are padding
            const unsigned r = 8u - off;
            if ((unsigned)(x >> (64 - r)) == (1u << r) - 1u) {
                pos = w.barrier * 8u;
                continue;
            }
        }
        const unsigned comp_sel = blk * 4u;
        const unsigned t = k == 0 ? (P.sel_dc >> comp_sel) & 15u : (P.sel_ac >> comp_sel) & 15u;
        const unsigned code16 = (unsigned)(x >> 48);
        unsigned len = 1, sym = 0;
        bool defined = false;
        const unsigned lk = P.tab.look(t, code16 >> 8);
        if (lk) {
            len = lk >> 8, sym = lk & 255u, defined = true;
        } else {
            for (unsigned l = 9; l <= 16; ++l) {
                const int cd = (int)(code16 >> (16 - l));
                if (cd <= P.tab.maxcode(t, l)) {
                    len = l, sym = P.tab.val(t, (unsigned)(cd + P.tab.delta(t, l)) & 255u), defined = true;
                    break;
                }
            }
        }
        unsigned used = len;
        bool done = false;                                                    // the block is complete
        if (defined) {
            const unsigned s = sym & 15u, run = k == 0 ? 0u : sym >> 4;
            const unsigned raw = s ? (unsigned)((x << len) >> (64 - s)) : 0u;
            const int value = s && raw < (1u << (s - 1)) ? (int)raw - (int)(1u << s) + 1 : (int)raw;
            used += s;
            if (k != 0 && s == 0) {
                if (run == 15) k += 16;                                       // ZRL
                else k = 64;                                                  // EOB
            } else {
                k += run;
                if (k <= 63) {
                    if (STORE) P.coef[(size_t)gb * 64 + (k == 0 ? 0u : JPEG_DEC_ZZ[k])] = (int16_t)value;     // (gb < blocks: checked above)
                    ++k;
                }
            }
            done = k > 63;                                                    // a run that passes 63 ends the block too
        }
        if (done) {
            k = 0;
            blk = blk + 1 == (unsigned)P.bpm ? 0u : blk + 1;
            ++c.blocks;
            if (STORE) ++gb;
        }
        const unsigned total = off + used, nbytes = total >> 3;
        if (w.nd < 5 && nbytes >= w.nd) pos = w.barrier * 8u;                 // (bits beyond a barrier are zeros; the position stops at it)
        else pos = (i + nbytes + __popc(w.ffmask & ((1u << nbytes) - 1u))) * 8u + (total & 7u);
        if (STORE && done && gb == P.blocks) c.endpos = pos;
    }
    *out = c;
    jd_state r;
    r.pos = pos, r.bk = (blk << 8) | k;
    return r;
}

__global__ void __launch_bounds__(JD_THREADS) jd_huffman_kernel(const uint8_t *__restrict__ scan, const yk_jpeg_pic_t *__restrict__ pics,
                                                                const uint8_t *__restrict__ tables, const uint32_t *__restrict__ blk_start,
                                                                int16_t *__restrict__ coef, int32_t *__restrict__ status, uint32_t *__restrict__ rounds, int chunk_bytes) {
    __shared__ uint32_t s_tab[JD_TABLE_BYTES];                                // 4 tables of 896 bytes
    __shared__ unsigned s_pos[JD_THREADS], s_bk[JD_THREADS], s_m[JD_THREADS], s_a[JD_THREADS];
    __shared__ unsigned s_flags, s_endpos;
    const int p = blockIdx.x, t = threadIdx.x;
    const unsigned b0 = blk_start[p], nb = blk_start[p + 1] - b0;
    if (nb == 0) {                                                            // an invalid row, or a workspace too small: uniform
        if (t == 0) rounds[p] = 0;
        return;
    }
    const yk_jpeg_pic_t &pic = pics[p];                                       // (read in place: a private copy indexed by component would live in scratch)
    const jd_geom g = jd_geometry(pic);
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tables + pic.table_offset + 256);
        for (int i = t; i < (int)JD_TABLE_BYTES; i += JD_THREADS) s_tab[i] = src[i];
    }
    if (t == 0) s_flags = 0, s_endpos = 0xFFFFFFFFu;
    jd_pic P;
    P.in.seg = scan + pic.scan_offset;
    P.in.end = pic.scan_bytes;
    P.tab.words = s_tab;
    P.sel_dc = P.sel_ac = 0;
    for (int b = 0; b < g.bpm; ++b) {
        const int c = b < g.nl ? 0 : b - g.nl + 1;
        P.sel_dc |= (unsigned)pic.td[c] << (4 * b);
        P.sel_ac |= (2u + pic.ta[c]) << (4 * b);
    }
    P.bpm = g.bpm, P.restart = pic.restart, P.blocks = nb;
    P.coef = coef + (size_t)b0 * 64;
    __syncthreads();
    const unsigned cb = (unsigned)chunk_bytes, nch = (P.in.end + cb - 1) / cb, endbits = P.in.end * 8u;
    jd_state carry = {0u, 0u};                                                // the entry of the tile's first chunk
    unsigned carry_m = 0, carry_a = 0;                                        // markers / blocks since the last one, in front of the tile
    unsigned nrounds = 0;                                                     // fixed-point rounds over all tiles (tools/detect_rate.py reads them)
    for (unsigned base = 0; base < nch; base += JD_THREADS) {
        const unsigned c = base + t;
        const bool live = c < nch;
        const unsigned limit = live ? ((c + 1) * cb < P.in.end ? (c + 1) * cb * 8u : endbits) : 0u;
        jd_state entry = carry, exit_;
        if (t > 0 && live) {                                                  // the guess: a symbol starts here, at the first index of an MCU's first block
            const unsigned at = c * cb;
            entry.pos = (at + (P.in.byte(at) == 0u && P.in.byte(at - 1) == 0xFFu ? 1u : 0u)) * 8u;
            entry.bk = 0;
        }
        jd_counts cnt = {0u, 0u, 0u, 0u};
        exit_ = entry;
        if (live) exit_ = jd_decode_chunk<false>(P, entry, limit, 0u, 0u, &cnt);
        const unsigned tile = nch - base < JD_THREADS ? nch - base : JD_THREADS;
        for (unsigned round = 0; round < tile; ++round) {                    // after j rounds the first j chunks are right
            s_pos[t] = exit_.pos, s_bk[t] = exit_.bk;
            __syncthreads();
            bool changed = false;
            if (t > 0 && live) {
                const jd_state e = {s_pos[t - 1], s_bk[t - 1]};
                changed = e.pos != entry.pos || e.bk != entry.bk;
                if (changed) {
                    entry = e;
                    exit_ = jd_decode_chunk<false>(P, entry, limit, 0u, 0u, &cnt);
                }
            }
            ++nrounds;
            if (!__syncthreads_or(changed)) break;
        }
        // the first block of every chunk: (m, a) o (m', a') = (m + m', m' ? a' : a + a'), scanned over the tile behind the carry
        s_m[t] = live ? cnt.markers : 0u, s_a[t] = live ? cnt.blocks : 0u;
        s_pos[t] = exit_.pos, s_bk[t] = exit_.bk;                            // (the break above leaves them as they are; an exhausted loop does not)
        __syncthreads();
        for (int o = 1; o < JD_THREADS; o <<= 1) {
            unsigned pm = 0, pa = 0;
            if (t >= o) pm = s_m[t - o], pa = s_a[t - o];
            const unsigned mm = s_m[t], ma = s_a[t];
            __syncthreads();
            if (t >= o) s_m[t] = pm + mm, s_a[t] = mm ? ma : pa + ma;
            __syncthreads();
        }
        unsigned em = carry_m, ea = carry_a;                                  // exclusive: everything in front of this chunk
        if (t > 0) em = carry_m + s_m[t - 1], ea = s_m[t - 1] ? s_a[t - 1] : carry_a + s_a[t - 1];
        if (live) {
            jd_counts fin;
            const unsigned gb = em * (unsigned)P.restart * (unsigned)P.bpm + ea;
            jd_decode_chunk<true>(P, entry, limit, gb, em, &fin);
            if (fin.flags) atomicOr(&s_flags, fin.flags);
            if (fin.endpos != 0xFFFFFFFFu) s_endpos = fin.endpos;             // one chunk completes the last block
        }
        const unsigned lm = s_m[JD_THREADS - 1], la = s_a[JD_THREADS - 1];
        carry.pos = s_pos[tile - 1], carry.bk = s_bk[tile - 1];
        carry_a = lm ? la : carry_a + la;
        carry_m += lm;
        __syncthreads();
    }
    if (t == 0) {
        unsigned f = s_flags;
        if (s_endpos == 0xFFFFFFFFu) f |= JD_ST_COUNT;                        // too few blocks
        else {                                                                // the stream ends inside its last byte: the rest of it is padding
            const unsigned i = s_endpos >> 3;                                 // (a last byte padded to 0xFF carries its stuffed zero behind it)
            const unsigned next = (s_endpos & 7u) ? i + 1u + (P.in.byte(i) == 0xFFu ? 1u : 0u) : i;
            if (next != P.in.end) f |= JD_ST_TRAIL;
        }
        status[p] = (int32_t)f;
        rounds[p] = nrounds;
    }
}

__global__ void __launch_bounds__(JD_THREADS) jd_dc_kernel(const yk_jpeg_pic_t *__restrict__ pics, const uint32_t *__restrict__ blk_start,
                                                           int16_t *__restrict__ coef) {
    __shared__ int s_v[3][JD_THREADS];
    __shared__ int s_f[JD_THREADS];
    const int p = blockIdx.x, t = threadIdx.x;
    const unsigned b0 = blk_start[p], nb = blk_start[p + 1] - b0;
    if (nb == 0) return;
    const yk_jpeg_pic_t pic = pics[p];
    const jd_geom g = jd_geometry(pic);
    const unsigned nmcu = nb / (unsigned)g.bpm;
    int16_t *dc = coef + (size_t)b0 * 64;
    int carry[3] = {0, 0, 0};
    for (unsigned base = 0; base < nmcu; base += JD_THREADS) {
        const unsigned m = base + t;
        const bool live = m < nmcu;
        int d[6] = {0, 0, 0, 0, 0, 0}, tot0 = 0, tot1 = 0, tot2 = 0;
        const bool first = live && pic.restart > 0 && m % (unsigned)pic.restart == 0;       // the predictors restart at this MCU
        if (live) {
#pragma unroll
            for (int b = 0; b < 6; ++b)
                if (b < g.bpm) {
                    d[b] = dc[((size_t)m * g.bpm + b) * 64];
                    tot0 += b < g.nl ? d[b] : 0, tot1 += b == g.nl ? d[b] : 0, tot2 += b == g.nl + 1 ? d[b] : 0;
                }
        }
        s_v[0][t] = tot0, s_v[1][t] = tot1, s_v[2][t] = tot2, s_f[t] = first ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < JD_THREADS; o <<= 1) {                            // inclusive segmented scan
            int a[3] = {0, 0, 0}, af = 0;
            if (t >= o) a[0] = s_v[0][t - o], a[1] = s_v[1][t - o], a[2] = s_v[2][t - o], af = s_f[t - o];
            const int mf = s_f[t];
            __syncthreads();
            if (t >= o) {
                if (!mf) s_v[0][t] += a[0], s_v[1][t] += a[1], s_v[2][t] += a[2];
                s_f[t] = mf | af;
            }
            __syncthreads();
        }
        int pred[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (first) pred[c] = 0;
            else if (t == 0) pred[c] = carry[c];
            else pred[c] = s_v[c][t - 1] + (s_f[t - 1] ? 0 : carry[c]);
        }
        if (live) {
#pragma unroll
            for (int b = 0; b < 6; ++b)
                if (b < g.bpm) {
                    int v;
                    if (b < g.nl) v = pred[0] += d[b];
                    else if (b == g.nl) v = pred[1] += d[b];
                    else v = pred[2] += d[b];
                    dc[((size_t)m * g.bpm + b) * 64] = (int16_t)v;
                }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) carry[c] = s_v[c][JD_THREADS - 1] + (s_f[JD_THREADS - 1] ? 0 : carry[c]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(JD_THREADS) jd_idct_kernel(const yk_jpeg_pic_t *__restrict__ pics, int n, const uint8_t *__restrict__ tables,
                                                             const uint32_t *__restrict__ blk_start, const int16_t *__restrict__ coef,
                                                             uint8_t *__restrict__ planes) {
    __shared__ int s_c[4][64];
    __shared__ int s_t[4][64];
    const int wv = threadIdx.x >> 6, i = threadIdx.x & 63, iy = i >> 3, ix = i & 7;
    const unsigned b = blockIdx.x * 4u + wv, total = blk_start[n];
    if (blockIdx.x * 4u >= total) return;                                     // uniform in the workgroup
    const bool live = b < total;                                              // uniform in the wave
    int pidx = 0;
    yk_jpeg_pic_t pic;
    jd_geom g = {1, 1, 1, 1, 0u};
    unsigned lb = 0;
    int comp = 0;
    if (live) {
        pidx = jd_picture_of(blk_start, n, b);
        pic = pics[pidx];
        g = jd_geometry(pic);
        lb = b - blk_start[pidx];
        const int j = (int)(lb % (unsigned)g.bpm);
        comp = j < g.nl ? 0 : j - g.nl + 1;
        const int q = tables[pic.table_offset + pic.tq[comp] * 64 + i];
        const int v = (int)coef[(size_t)b * 64 + i] * q;
        s_c[wv][i] = min(max(v, -32767), 32767);
    }
    __syncthreads();
    if (live) {                                                               // columns: lane (y = iy, u = ix)
        int a = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) a += JPEG_DEC_T[v * 8 + iy] * s_c[wv][v * 8 + ix];
        s_t[wv][i] = min(max((a + 512) >> 10, -65535), 65535);
    }
    __syncthreads();
    if (live) {                                                               // rows: lane (y = iy, x = ix)
        int a = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) a += JPEG_DEC_T[u * 8 + ix] * s_t[wv][iy * 8 + u];
        const int px = min(max(((a + 32768) >> 16) + 128, 0), 255);
        const unsigned mcu = lb / (unsigned)g.bpm, nmcu = (unsigned)g.mw * g.mh;
        const int j = (int)(lb % (unsigned)g.bpm), my = (int)(mcu / (unsigned)g.mw), mx = (int)(mcu % (unsigned)g.mw);
        size_t at;
        if (comp == 0) {
            const int by = my * pic.vs + j / pic.hs, bx = mx * pic.hs + j % pic.hs;
            at = ((size_t)(by * 8 + iy) * (g.mw * pic.hs) + bx) * 8 + ix;
        } else {
            at = (size_t)nmcu * (g.nl + comp - 1) * 64 + ((size_t)(my * 8 + iy) * g.mw + mx) * 8 + ix;
        }
        planes[(size_t)blk_start[pidx] * 64 + at] = (uint8_t)px;              // at < blocks * 64
    }
}

__global__ void __launch_bounds__(JD_THREADS) jd_colour_kernel(const yk_jpeg_pic_t *__restrict__ pics, const yk_ragged_row_t *__restrict__ rows, int n,
                                                               const uint32_t *__restrict__ blk_start, const uint8_t *__restrict__ planes,
                                                               uint8_t *__restrict__ dst) {
    const size_t gidx = (size_t)blockIdx.x * JD_THREADS + threadIdx.x;
    const unsigned b = (unsigned)(gidx >> 6);
    if (b >= blk_start[n]) return;
    const int p = jd_picture_of(blk_start, n, b);
    const yk_jpeg_pic_t pic = pics[p];
    const jd_geom g = jd_geometry(pic);
    const size_t local = gidx - (size_t)blk_start[p] * 64;
    const unsigned nmcu = (unsigned)g.mw * g.mh;
    const unsigned stride = (unsigned)g.mw * pic.hs * 8u;
    if (local >= (size_t)nmcu * g.nl * 64) return;                            // a chroma sample: its pixels are written from the luma side
    const int y = (int)(local / stride), x = (int)(local % stride);
    if (y >= pic.h || x >= pic.w) return;                                     // MCU padding
    const uint8_t *base = planes + (size_t)blk_start[p] * 64;
    const int yy = base[local];
    int r = yy, gg = yy, bb = yy;
    if (pic.ncomp == 3) {
        const unsigned cs = (unsigned)g.mw * 8u;
        const uint8_t *pb = base + (size_t)nmcu * g.nl * 64, *pr = pb + (size_t)nmcu * 64;
        int cb, cr;
        if (pic.hs == 1) {
            cb = pb[(size_t)y * cs + x], cr = pr[(size_t)y * cs + x];
        } else {
            const int cw = (pic.w + 1) >> 1, cx = x >> 1, ox = min(max((x & 1) ? cx + 1 : cx - 1, 0), cw - 1);
            if (pic.vs == 1) {
                const int rnd = (x & 1) ? 2 : 1;
                cb = (3 * pb[(size_t)y * cs + cx] + pb[(size_t)y * cs + ox] + rnd) >> 2;
                cr = (3 * pr[(size_t)y * cs + cx] + pr[(size_t)y * cs + ox] + rnd) >> 2;
            } else {
                const int ch = (pic.h + 1) >> 1, cy = y >> 1, oy = min(max((y & 1) ? cy + 1 : cy - 1, 0), ch - 1);
                const int rnd = (x & 1) ? 7 : 8;
                const size_t n0 = (size_t)cy * cs, f0 = (size_t)oy * cs;
                cb = (3 * (3 * pb[n0 + cx] + pb[f0 + cx]) + (3 * pb[n0 + ox] + pb[f0 + ox]) + rnd) >> 4;
                cr = (3 * (3 * pr[n0 + cx] + pr[f0 + cx]) + (3 * pr[n0 + ox] + pr[f0 + ox]) + rnd) >> 4;
            }
        }
        cb -= 128, cr -= 128;
        r = yy + ((JPEG_DEC_CR_R * cr + 32768) >> 16);
        gg = yy + ((-JPEG_DEC_CB_G * cb - JPEG_DEC_CR_G * cr + 32768) >> 16);
        bb = yy + ((JPEG_DEC_CB_B * cb + 32768) >> 16);
    }
    uint8_t *o = dst + rows[p].offset + ((size_t)y * pic.w + x) * 3;          // (the plan kernel checked the row against dst_bytes)
    o[0] = (uint8_t)min(max(r, 0), 255);
    o[1] = (uint8_t)min(max(gg, 0), 255);
    o[2] = (uint8_t)min(max(bb, 0), 255);
}

extern "C" int yk_jpeg_decode_workspace_bytes(const yk_jpeg_pic_t *h_pics, int n, size_t *work_bytes) {
    if (!h_pics || n <= 0 || !work_bytes) {
        yk_set_error("yk_jpeg_decode_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    uint64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const jd_geom g = jd_geometry(h_pics[i]);
        if (g.blocks == 0) {
            yk_set_error("yk_jpeg_decode_workspace_bytes: row %d (%d x %d, %d components, sampling %d x %d) is not a picture this decoder takes", i,
                         h_pics[i].h, h_pics[i].w, h_pics[i].ncomp, h_pics[i].hs, h_pics[i].vs);
            return YK_ERR_ARG;
        }
        blocks += g.blocks;
    }
    if (blocks > (1ull << 30)) {
        yk_set_error("yk_jpeg_decode_workspace_bytes: %llu blocks are more than one call decodes", (unsigned long long)blocks);
        return YK_ERR_ARG;
    }
    *work_bytes = jd_header_bytes((size_t)n) + (size_t)blocks * JD_PER_BLOCK;
    return YK_OK;
}

extern "C" int yk_jpeg_decode_ragged_u8(const uint8_t *d_scan, size_t scan_bytes, const yk_jpeg_pic_t *d_pics, const uint8_t *d_tables,
                                        size_t table_bytes, const yk_ragged_row_t *d_rows, int n, uint8_t *d_dst, size_t dst_bytes, void *d_work,
                                        size_t work_bytes, int32_t *d_status, int chunk_bytes, void *stream) {
    if (chunk_bytes == 0) chunk_bytes = YK_JPEG_DECODE_CHUNK;
    if (!d_scan || !d_pics || !d_tables || !d_rows || !d_dst || !d_work || !d_status || n <= 0 || scan_bytes == 0 || table_bytes == 0 ||
        dst_bytes == 0 || ((uintptr_t)d_scan & 3) || ((uintptr_t)d_tables & 3) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_pics & 7) ||
        chunk_bytes < 4 || chunk_bytes > 1024 || (chunk_bytes & 3)) {
        yk_set_error("yk_jpeg_decode_ragged_u8: bad argument (chunk_bytes %d)", chunk_bytes);
        return YK_ERR_ARG;
    }
    const size_t fixed = jd_header_bytes((size_t)n);
    if (work_bytes < fixed + JD_PER_BLOCK) {
        yk_set_error("yk_jpeg_decode_ragged_u8: work_bytes %zu hold no block (yk_jpeg_decode_workspace_bytes sizes them)", work_bytes);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_jpeg_decode_ragged_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    size_t cap = (work_bytes - fixed) / JD_PER_BLOCK;                         // what the workspace holds; the kernels never go beyond it
    if (cap > ((size_t)1 << 30)) cap = (size_t)1 << 30;
    uint32_t *blk_start = (uint32_t *)d_work;
    uint32_t *rounds = (uint32_t *)((char *)d_work + jd_a16(4 * ((size_t)n + 1)));
    int16_t *coef = (int16_t *)((char *)d_work + fixed);
    uint8_t *planes = (uint8_t *)(coef + cap * 64);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jd_plan_kernel, dim3(1), dim3(JD_THREADS), 0, st, d_pics, d_rows, n, scan_bytes, table_bytes, dst_bytes, (unsigned)cap,
                       blk_start, d_status);
    hipLaunchKernelGGL(jd_zero_kernel, dim3((unsigned)((cap * 8 + JD_THREADS - 1) / JD_THREADS)), dim3(JD_THREADS), 0, st, (uint4 *)coef, cap * 8);
    hipLaunchKernelGGL(jd_huffman_kernel, dim3((unsigned)n), dim3(JD_THREADS), 0, st, d_scan, d_pics, d_tables, blk_start, coef, d_status,
                       rounds, chunk_bytes);
    hipLaunchKernelGGL(jd_dc_kernel, dim3((unsigned)n), dim3(JD_THREADS), 0, st, d_pics, blk_start, coef);
    hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)((cap + 3) / 4)), dim3(JD_THREADS), 0, st, d_pics, n, d_tables, blk_start, coef, planes);
    hipLaunchKernelGGL(jd_colour_kernel, dim3((unsigned)((cap * 64 + JD_THREADS - 1) / JD_THREADS)), dim3(JD_THREADS), 0, st, d_pics, d_rows, n,
                       blk_start, planes, d_dst);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
