// yk_jpeg.hip — baseline JPEG encoding of a ragged batch of pictures on the device (`make detect ENCODE=gpu`):
// 8 bit, YCbCr 4:2:0, interleaved scan, the Annex-K Huffman tables, no restart markers.  The call produces the entropy-coded scan of every
// picture, byte-stuffed and padded, packed back to back in d_out; the host puts the JFIF headers around it (jpeg.py).  All arithmetic
// from pixel to coefficient is integer and stated in include/yolo_hip.h, so tests/jpeg_ref.py reproduces every byte.
//
// Structure (every launch on the caller's stream, nothing synchronises, everything can be recorded in a graph):
//   plan      one workgroup: MCUs per picture from the DEVICE table (an invalid row: none), scanned into mcu_start[n + 1]
//   transform one workgroup of 6 waves per 16x16 MCU, one wave per 8x8 block, one lane per coefficient: load with edge replication,
//             colour, chroma average, two 1-D DCT passes through LDS, quantise, zigzagged int16 store; the AC bit count of the block
//             by one ballot (the run before a coefficient is the distance to the previous set bit) and a wave sum; zeroes the MCU's
//             1248 bytes of the bit buffer
//   offsets   one workgroup per picture, one thread per MCU: DC differences (predictor: the previous block of the component), the bit
//             length of every block, a scan in chunks of 256 MCUs -> bit offset of every block inside its picture; the trailing 1-padding
//   emit      one thread per block walks its 63 AC coefficients and shifts codes into a 64-bit accumulator; whole words are stored, the
//             first and the last word of a block - the only ones a neighbour shares - are merged with a 32-bit atomicOr into the zeroed
//             buffer.  OR does not depend on order: the same bytes on every run.
//   stuffing  count 0xFF per 1248-byte chunk (one wave each), scan per picture, scan over pictures -> d_out_off, scatter with the 0x00s.
// Worst case: a block is at most 22 + 63 * 26 = 1660 bits; every block owns 1664 bits of the unstuffed buffer, an MCU
// 1248 bytes, and a picture's stream is at most twice that after stuffing.
#include "yk_common.h"
#include "yk_jpeg_tables.h"

#define JPEG_MCU_WORDS 312u                   // 6 blocks x 1664 bits
#define JPEG_MCU_BYTES (JPEG_MCU_WORDS * 4u)
#define JPEG_PER_MCU (768u + 12u + 12u + 48u + 4u + 8u + JPEG_MCU_BYTES)      // workspace bytes per MCU, see jpeg_layout
#define JPEG_SLACK 128u                       // alignment of the seven per-MCU arrays
#define JPEG_LANE_BYTES 20u                   // stuffing: bytes of a chunk per lane (63 lanes x 20 >= 1248)

struct jpeg_layout {
    uint64_t *mcu_start;   // [n + 1]
    uint64_t *pic_bits;    // [n] bits of the picture's scan before padding
    uint64_t *pic_len;     // [n] bytes after stuffing
    int16_t *coef;         // [M][6][64] zigzag order, the DC undifferenced
    uint16_t *acbits;      // [M][6]
    int16_t *dcdiff;       // [M][6]
    uint64_t *bitoff;      // [M][6] from the picture's first bit
    uint32_t *ffcount;     // [M] 0xFF bytes in the chunk
    uint64_t *chunkoff;    // [M] stuffed bytes of the picture in front of the chunk
    uint32_t *bitbuf;      // [M][312] unstuffed bits, MSB first, bytes in memory order; picture p begins at word mcu_start[p] * 312
};

static inline size_t jpeg_a16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t jpeg_header_bytes(size_t n) { return jpeg_a16(8 * (n + 1)) + 2 * jpeg_a16(8 * n); }

static jpeg_layout jpeg_make_layout(void *work, size_t n, size_t M) {
    char *p = (char *)work;
    jpeg_layout L;
    auto take = [&p](size_t bytes) { char *r = p; p += jpeg_a16(bytes); return r; };
    L.mcu_start = (uint64_t *)take(8 * (n + 1));
    L.pic_bits = (uint64_t *)take(8 * n);
    L.pic_len = (uint64_t *)take(8 * n);
    L.coef = (int16_t *)take(768 * M);
    L.acbits = (uint16_t *)take(12 * M);
    L.dcdiff = (int16_t *)take(12 * M);
    L.bitoff = (uint64_t *)take(48 * M);
    L.ffcount = (uint32_t *)take(4 * M);
    L.chunkoff = (uint64_t *)take(8 * M);
    L.bitbuf = (uint32_t *)take((size_t)JPEG_MCU_BYTES * M);
    return L;
}

// exclusive scan over the 256 threads of a workgroup; *total = the sum.  sh: 256 values of LDS.
__device__ __forceinline__ uint64_t jpeg_block_scan(uint64_t v, uint64_t *sh, uint64_t *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint64_t a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ unsigned jpeg_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the picture of MCU g: the largest p < n with mcu_start[p] <= g (g < mcu_start[n]; empty pictures share their start with the next one)
__device__ __forceinline__ int jpeg_picture_of(const uint64_t *__restrict__ mcu_start, int n, uint64_t g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mcu_start[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) jpeg_plan_kernel(const yk_ragged_row_t *__restrict__ table, int n, size_t src_bytes, uint64_t m_cap,
                                                        uint64_t *__restrict__ mcu_start) {
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int p = base + threadIdx.x;
        uint64_t cnt = 0;
        if (p < n) {
            const yk_ragged_row_t row = table[p];
            const bool ok = row.h > 0 && row.w > 0 && row.h <= 65535 && row.w <= 65535 && row.offset <= src_bytes &&
                            (size_t)row.h * row.w * 3 <= src_bytes - row.offset;
            if (ok) cnt = (uint64_t)((row.h + 15) >> 4) * (uint64_t)((row.w + 15) >> 4);
        }
        uint64_t total;
        const uint64_t excl = jpeg_block_scan(cnt, sh, &total);
        if (p < n) mcu_start[p] = carry + excl;
        carry += total;
    }
    __syncthreads();
    if (carry > m_cap) {                                                      // a workspace too small for this table: n empty streams
        for (int p = threadIdx.x; p <= n; p += 256) mcu_start[p] = 0;
    } else if (threadIdx.x == 0) {
        mcu_start[n] = carry;
    }
}

__global__ void __launch_bounds__(384) jpeg_transform_kernel(const uint8_t *__restrict__ buf, const yk_ragged_row_t *__restrict__ table, int n,
                                                             const uint8_t *__restrict__ qtab, const uint64_t *__restrict__ mcu_start,
                                                             int16_t *__restrict__ coef, uint16_t *__restrict__ acbits,
                                                             uint32_t *__restrict__ bitbuf) {
    __shared__ int s_px[3][256];
    __shared__ int s_blk[6][64];
    __shared__ int s_r1[6][64];
    __shared__ int s_q[128];
    const uint64_t g = blockIdx.x;
    if (g >= mcu_start[n]) return;                                            // uniform
    const int tid = threadIdx.x;
    const int p = jpeg_picture_of(mcu_start, n, g);
    const yk_ragged_row_t row = table[p];
    const int h = row.h, w = row.w, mw = (w + 15) >> 4;
    const uint64_t local = g - mcu_start[p];
    const int my = (int)(local / (uint64_t)mw), mx = (int)(local % (uint64_t)mw);
    if (tid < 128) s_q[tid] = qtab[tid];
    if (tid < (int)JPEG_MCU_WORDS) bitbuf[g * JPEG_MCU_WORDS + tid] = 0;        // the MCU's share of the bit buffer: emit ORs into zeros
    if (tid < 256) {
        const int y = min(my * 16 + (tid >> 4), h - 1), x = min(mx * 16 + (tid & 15), w - 1);       // edge replication on the RGB indices
        const uint8_t *px = buf + row.offset + ((size_t)y * w + x) * 3;
        const int r = px[0], gg = px[1], b = px[2];
        const int yy = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
        const int cb = ((-11059 * r - 21709 * gg + 32768 * b + 32768) >> 16) + 128;
        const int cr = ((32768 * r - 27439 * gg - 5329 * b + 32768) >> 16) + 128;
        s_px[0][tid] = min(max(yy, 0), 255);
        s_px[1][tid] = min(max(cb, 0), 255);
        s_px[2][tid] = min(max(cr, 0), 255);
    }
    __syncthreads();
    const int b = tid >> 6, i = tid & 63, iy = i >> 3, ix = i & 7;            // one wave per block: Y00 Y01 Y10 Y11 Cb Cr
    if (b < 4) {
        s_blk[b][i] = s_px[0][((b >> 1) * 8 + iy) * 16 + (b & 1) * 8 + ix] - 128;
    } else {
        const int *c = &s_px[b - 3][(2 * iy) * 16 + 2 * ix];
        s_blk[b][i] = ((c[0] + c[1] + c[16] + c[17] + 2) >> 2) - 128;
    }
    __syncthreads();
    {                                                                         // rows: lane (y = iy, u = ix)
        int r = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) r += JPEG_T[ix * 8 + x] * s_blk[b][iy * 8 + x];
        s_r1[b][i] = (r + 512) >> 10;
    }
    __syncthreads();
    const int nat = JPEG_ZZ[i], v = nat >> 3, u = nat & 7;                    // columns: lane = zigzag index
    int c = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) c += JPEG_T[v * 8 + y] * s_r1[b][y * 8 + u];
    const unsigned d = (unsigned)s_q[(b < 4 ? 0 : 64) + nat];
    const unsigned mag = ((unsigned)(c < 0 ? -c : c) + d * 32768u) / (d * 65536u);
    int q = c < 0 ? -(int)mag : (int)mag;
    if (i > 0) q = min(max(q, -1023), 1023);
    coef[(g * 6 + b) * 64 + i] = (int16_t)q;

    const bool nz = i > 0 && q != 0;
    const unsigned long long mask = __ballot(nz);
    unsigned bits = 0;
    const uint32_t *ac = JPEG_AC + (b < 4 ? 0 : 256);
    if (nz) {
        const unsigned long long before = (mask | 1ull) & ((1ull << i) - 1ull);
        const int run = i - (63 - __clzll((long long)before)) - 1;
        const int size = 32 - __clz(q < 0 ? -q : q);
        bits = (unsigned)(run >> 4) * (ac[0xF0] & 255u) + (ac[((run & 15) << 4) | size] & 255u) + (unsigned)size;
    }
    bits = jpeg_wave_sum(bits);
    if (i == 0) {
        if (!(mask >> 63)) bits += ac[0] & 255u;                              // EOB: the last coefficient is zero
        acbits[g * 6 + b] = (uint16_t)bits;
    }
}

__global__ void __launch_bounds__(256) jpeg_offsets_kernel(const uint64_t *__restrict__ mcu_start, const int16_t *__restrict__ coef,
                                                           const uint16_t *__restrict__ acbits, int16_t *__restrict__ dcdiff,
                                                           uint64_t *__restrict__ bitoff, uint64_t *__restrict__ pic_bits,
                                                           uint32_t *__restrict__ bitbuf) {
    __shared__ uint64_t sh[256];
    const int p = blockIdx.x;
    const uint64_t m0 = mcu_start[p], cnt = mcu_start[p + 1] - m0;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < cnt; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < cnt;
        const uint64_t g = m0 + i;
        int diff[6];
        unsigned len[6];
        uint64_t sum = 0;
        if (live) {
            int dc[6], pred[3] = {0, 0, 0};
#pragma unroll
            for (int b = 0; b < 6; ++b) dc[b] = coef[(g * 6 + b) * 64];
            if (i > 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) pred[c] = coef[((g - 1) * 6 + 3 + c) * 64];
            }
            diff[0] = dc[0] - pred[0], diff[1] = dc[1] - dc[0], diff[2] = dc[2] - dc[1], diff[3] = dc[3] - dc[2];
            diff[4] = dc[4] - pred[1], diff[5] = dc[5] - pred[2];
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                diff[b] = min(max(diff[b], -2047), 2047);
                const int size = 32 - __clz(diff[b] < 0 ? -diff[b] : diff[b]);
                len[b] = (JPEG_DC[(b < 4 ? 0 : 12) + size] & 255u) + (unsigned)size + acbits[g * 6 + b];
                sum += len[b];
            }
        }
        uint64_t total;
        uint64_t off = carry + jpeg_block_scan(sum, sh, &total);
        if (live) {
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                dcdiff[g * 6 + b] = (int16_t)diff[b];
                bitoff[g * 6 + b] = off;
                off += len[b];
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        pic_bits[p] = carry;
        const unsigned used = (unsigned)(carry & 7u);
        if (used) {                                                           // the last byte is padded with 1-bits
            const unsigned pad = 8u - used, at = (unsigned)(carry & 31u);
            const uint32_t word = ((1u << pad) - 1u) << (32u - at - pad);
            atomicOr(&bitbuf[m0 * JPEG_MCU_WORDS + (carry >> 5)], __builtin_bswap32(word));
        }
    }
}

struct jpeg_writer {
    uint32_t *words;        // the picture's region
    uint64_t nwords, at;    // its size, the next word
    uint64_t acc;
    int nacc;
    bool first;
    __device__ __forceinline__ void flush(uint32_t word, bool whole) {
        if (at < nwords) {                                                    // cannot fail (worst-case bound); never write outside
            if (whole && !first) words[at] = __builtin_bswap32(word);
            else atomicOr(&words[at], __builtin_bswap32(word));
        }
        first = false;
        ++at;
    }
    __device__ __forceinline__ void put(uint32_t v, int len) {                // len <= 26
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            nacc -= 32;
            flush((uint32_t)(acc >> nacc), true);
            acc &= (1ull << nacc) - 1ull;
        }
    }
};

__global__ void __launch_bounds__(256) jpeg_emit_kernel(const uint64_t *__restrict__ mcu_start, int n, const int16_t *__restrict__ coef,
                                                        const int16_t *__restrict__ dcdiff, const uint64_t *__restrict__ bitoff,
                                                        uint32_t *__restrict__ bitbuf) {
    const uint64_t blk = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= mcu_start[n] * 6) return;
    const uint64_t g = blk / 6;
    const int b = (int)(blk % 6);
    const int p = jpeg_picture_of(mcu_start, n, g);
    const uint64_t m0 = mcu_start[p];
    const uint64_t off = bitoff[blk];
    jpeg_writer wr;
    wr.words = bitbuf + m0 * JPEG_MCU_WORDS;
    wr.nwords = (mcu_start[p + 1] - m0) * JPEG_MCU_WORDS;
    wr.at = off >> 5;
    wr.acc = 0;
    wr.nacc = (int)(off & 31u);                                               // the bits in front belong to the neighbour: zeros here
    wr.first = true;
    const uint32_t *ac = JPEG_AC + (b < 4 ? 0 : 256);
    {
        const int diff = dcdiff[blk];
        const int size = 32 - __clz(diff < 0 ? -diff : diff);
        const uint32_t e = JPEG_DC[(b < 4 ? 0 : 12) + size];
        const uint32_t extra = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u);
        wr.put(((e >> 8) << size) | extra, (int)(e & 255u) + size);
    }
    const uint4 *c4 = reinterpret_cast<const uint4 *>(coef + blk * 64);       // 128 bytes per block, 16-byte aligned
    int run = 0;
    for (int c = 0; c < 8; ++c) {
        const uint4 q4 = c4[c];
        const uint32_t wd[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (c == 0 && j == 0) continue;
            const int v = (int)(int16_t)(wd[j >> 1] >> ((j & 1) * 16));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run >= 16) {
                wr.put(ac[0xF0] >> 8, (int)(ac[0xF0] & 255u));                // ZRL
                run -= 16;
            }
            const int size = 32 - __clz(v < 0 ? -v : v);
            const uint32_t e = ac[(run << 4) | size];
            const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
            wr.put(((e >> 8) << size) | extra, (int)(e & 255u) + size);
            run = 0;
        }
    }
    if (run) wr.put(ac[0] >> 8, (int)(ac[0] & 255u));                         // EOB
    if (wr.nacc) wr.flush((uint32_t)(wr.acc << (32 - wr.nacc)), false);
}

// One wave per 1248-byte chunk (= the region of one MCU; a picture's bits fill its chunks from the first on).  SCATTER false: counts the
// chunk's 0xFF bytes; true: writes the chunk's bytes to their final place, a 0x00 after every 0xFF.
template <bool SCATTER>
__global__ void __launch_bounds__(256) jpeg_stuff_kernel(const uint64_t *__restrict__ mcu_start, int n, const uint64_t *__restrict__ pic_bits,
                                                         const uint32_t *__restrict__ bitbuf, uint32_t *__restrict__ ffcount,
                                                         const uint64_t *__restrict__ chunkoff, const uint64_t *__restrict__ out_off,
                                                         uint8_t *__restrict__ out, size_t out_capacity) {
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63u;
    if (g >= mcu_start[n]) return;                                            // uniform in the wave
    if (SCATTER && out_off[n] == 0) return;                                   // nothing, or an output too small for this batch
    const int p = jpeg_picture_of(mcu_start, n, g);
    const uint64_t m0 = mcu_start[p];
    const uint64_t bytes = (pic_bits[p] + 7) >> 3;                            // unstuffed bytes of the picture
    const uint64_t cstart = (g - m0) * JPEG_MCU_BYTES;
    if (cstart >= bytes) {                                                    // uniform: the chunk holds no data
        if (!SCATTER && lane == 0) ffcount[g] = 0;
        return;
    }
    const uint64_t cbytes = bytes - cstart < JPEG_MCU_BYTES ? bytes - cstart : JPEG_MCU_BYTES;
    const unsigned first = lane * JPEG_LANE_BYTES;
    const unsigned mine = first >= cbytes ? 0u : (cbytes - first < JPEG_LANE_BYTES ? (unsigned)(cbytes - first) : JPEG_LANE_BYTES);
    uint32_t wd[JPEG_LANE_BYTES / 4];
    unsigned ff = 0;
#pragma unroll
    for (unsigned k = 0; k < JPEG_LANE_BYTES / 4; ++k) {
        wd[k] = 4 * k < mine ? bitbuf[g * JPEG_MCU_WORDS + first / 4 + k] : 0u;   // (first + 4k < 1248: inside the chunk)
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) ff += (4 * k + j < mine && ((wd[k] >> (8 * j)) & 255u) == 255u) ? 1u : 0u;
    }
    if (!SCATTER) {
        ff = jpeg_wave_sum(ff);
        if (lane == 0) ffcount[g] = ff;
        return;
    }
    unsigned incl = ff;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned a = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += a;
    }
    uint64_t pos = out_off[p] + chunkoff[g] + first + (incl - ff);
#pragma unroll
    for (unsigned k = 0; k < JPEG_LANE_BYTES / 4; ++k) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            if (4 * k + j < mine) {
                const uint8_t v = (uint8_t)((wd[k] >> (8 * j)) & 255u);
                if (pos < out_capacity) out[pos] = v;
                ++pos;
                if (v == 255u) {
                    if (pos < out_capacity) out[pos] = 0;
                    ++pos;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) jpeg_chunk_scan_kernel(const uint64_t *__restrict__ mcu_start, const uint64_t *__restrict__ pic_bits,
                                                              const uint32_t *__restrict__ ffcount, uint64_t *__restrict__ chunkoff,
                                                              uint64_t *__restrict__ pic_len) {
    __shared__ uint64_t sh[256];
    const int p = blockIdx.x;
    const uint64_t m0 = mcu_start[p];
    const uint64_t bytes = (pic_bits[p] + 7) >> 3;
    const uint64_t chunks = (bytes + JPEG_MCU_BYTES - 1) / JPEG_MCU_BYTES;    // <= the picture's MCUs (worst-case bound)
    uint64_t carry = 0;
    for (uint64_t base = 0; base < chunks; base += 256) {
        const uint64_t i = base + threadIdx.x;
        uint64_t v = 0;
        if (i < chunks) {
            const uint64_t left = bytes - i * JPEG_MCU_BYTES;
            v = (left < JPEG_MCU_BYTES ? left : JPEG_MCU_BYTES) + ffcount[m0 + i];
        }
        uint64_t total;
        const uint64_t excl = jpeg_block_scan(v, sh, &total);
        if (i < chunks) chunkoff[m0 + i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) pic_len[p] = carry;
}

__global__ void __launch_bounds__(256) jpeg_out_off_kernel(const uint64_t *__restrict__ pic_len, int n, size_t out_capacity,
                                                           uint64_t *__restrict__ out_off) {
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int p = base + threadIdx.x;
        uint64_t total;
        const uint64_t excl = jpeg_block_scan(p < n ? pic_len[p] : 0, sh, &total);
        if (p < n) out_off[p] = carry + excl;
        carry += total;
    }
    __syncthreads();
    if (carry > out_capacity) {                                               // an output too small for this batch: n empty streams
        for (int p = threadIdx.x; p <= n; p += 256) out_off[p] = 0;
    } else if (threadIdx.x == 0) {
        out_off[n] = carry;
    }
}

extern "C" int yk_jpeg_tables(int quality, uint8_t *h_qtab) {
    if (!h_qtab || quality < 1 || quality > 100) {
        yk_set_error("yk_jpeg_tables: bad argument (quality %d)", quality);
        return YK_ERR_ARG;
    }
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 128; ++i) {
        const int t = (YK_JPEG_BASE_Q[i] * scale + 50) / 100;
        h_qtab[i] = (uint8_t)(t < 1 ? 1 : (t > 255 ? 255 : t));
    }
    return YK_OK;
}

extern "C" int yk_jpeg_workspace_bytes(const yk_ragged_row_t *h_table, int n, size_t *work_bytes, size_t *out_capacity) {
    if (!h_table || n <= 0 || !work_bytes || !out_capacity) {
        yk_set_error("yk_jpeg_workspace_bytes: bad argument");
        return YK_ERR_ARG;
    }
    uint64_t M = 0;
    for (int i = 0; i < n; ++i) {
        const int h = h_table[i].h, w = h_table[i].w;
        if (h > 65535 || w > 65535) {
            yk_set_error("yk_jpeg_workspace_bytes: row %d is %d x %d, more than a JPEG frame header holds", i, h, w);
            return YK_ERR_ARG;
        }
        if (h > 0 && w > 0) M += (uint64_t)((h + 15) >> 4) * (uint64_t)((w + 15) >> 4);   // (a row without pixels encodes to nothing)
    }
    if (M == 0) M = 1;
    if (M > (1ull << 30)) {
        yk_set_error("yk_jpeg_workspace_bytes: %llu MCUs are more than one call encodes", (unsigned long long)M);
        return YK_ERR_ARG;
    }
    *work_bytes = jpeg_header_bytes((size_t)n) + JPEG_SLACK + (size_t)M * JPEG_PER_MCU;
    *out_capacity = (size_t)M * 2 * JPEG_MCU_BYTES;
    return YK_OK;
}

extern "C" int yk_jpeg_encode_ragged_u8(const uint8_t *d_buf, size_t src_bytes, const yk_ragged_row_t *d_table, int n, const uint8_t *d_qtab,
                                        void *d_work, size_t work_bytes, uint8_t *d_out, size_t out_capacity, uint64_t *d_out_off,
                                        void *stream) {
    if (!d_buf || !d_table || !d_qtab || !d_work || !d_out || !d_out_off || n <= 0 || src_bytes == 0 || ((uintptr_t)d_work & 15) ||
        ((uintptr_t)d_out_off & 7)) {
        yk_set_error("yk_jpeg_encode_ragged_u8: bad argument");
        return YK_ERR_ARG;
    }
    const size_t fixed = jpeg_header_bytes((size_t)n) + JPEG_SLACK;
    if (work_bytes < fixed + JPEG_PER_MCU || out_capacity < 2 * (size_t)JPEG_MCU_BYTES) {
        yk_set_error("yk_jpeg_encode_ragged_u8: work_bytes %zu / out_capacity %zu hold no MCU (yk_jpeg_workspace_bytes sizes them)", work_bytes,
                     out_capacity);
        return YK_ERR_ARG;
    }
    if (yk_current_device() < 0) {
        yk_set_error("yk_jpeg_encode_ragged_u8: no HIP device");
        return YK_ERR_NO_DEVICE;
    }
    size_t M = (work_bytes - fixed) / JPEG_PER_MCU;                           // what the workspace holds; the kernels never go beyond it
    if (M > ((size_t)1 << 30)) M = (size_t)1 << 30;
    const jpeg_layout L = jpeg_make_layout(d_work, (size_t)n, M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_plan_kernel, dim3(1), dim3(256), 0, st, d_table, n, src_bytes, (uint64_t)M, L.mcu_start);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)M), dim3(384), 0, st, d_buf, d_table, n, d_qtab, L.mcu_start, L.coef, L.acbits,
                       L.bitbuf);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((unsigned)n), dim3(256), 0, st, L.mcu_start, L.coef, L.acbits, L.dcdiff, L.bitoff, L.pic_bits,
                       L.bitbuf);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)((M * 6 + 255) / 256)), dim3(256), 0, st, L.mcu_start, n, L.coef, L.dcdiff, L.bitoff,
                       L.bitbuf);
    const dim3 chunks((unsigned)((M + 3) / 4));
    hipLaunchKernelGGL(jpeg_stuff_kernel<false>, chunks, dim3(256), 0, st, L.mcu_start, n, L.pic_bits, L.bitbuf, L.ffcount, L.chunkoff, d_out_off,
                       d_out, out_capacity);
    hipLaunchKernelGGL(jpeg_chunk_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, L.mcu_start, L.pic_bits, L.ffcount, L.chunkoff, L.pic_len);
    hipLaunchKernelGGL(jpeg_out_off_kernel, dim3(1), dim3(256), 0, st, L.pic_len, n, out_capacity, d_out_off);
    hipLaunchKernelGGL(jpeg_stuff_kernel<true>, chunks, dim3(256), 0, st, L.mcu_start, n, L.pic_bits, L.bitbuf, L.ffcount, L.chunkoff, d_out_off,
                       d_out, out_capacity);
    YK_HIP(hipGetLastError());
    return YK_OK;
}
