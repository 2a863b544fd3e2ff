// yk_xplan_build.h — the f16x2 plan builder: yk_xplan_create as a list of passes over one xbuilder.  Included by yk_exact.hip (one
// translation unit with the kernels and launch wrappers it plans for); host code only.
#pragma once
#include "yk_plan_graph.h"

namespace {

// The switches the shipped library reads (README "Environment switches"), sampled once per plan; nothing below reads the environment.
struct xopts {
    bool fuse_blocks;                  // YK_FUSE_DWPW: depthwise + pointwise (and the stem in front) as one launch
    bool persist, heads;               // YK_PERSIST / YK_HEADS: the two cluster launches (default: the latency schedule)
    bool fuse_head;                    // YK_FUSE_HEAD: head conv + its 1x1 output conv as one launch
    bool splitk;                       // YK_SPLITK
    bool cluster_wt;                   // YK_CLUSTER_WT: the cluster launches never trust their placement check
};
xopts x_read_opts(int latency_schedule) {
    xopts o;
    o.fuse_blocks = yk_env_flag("YK_FUSE_DWPW", true) && !yk_dev_env("YK_X_NOFUSE");
    o.persist = yk_env_flag("YK_PERSIST", latency_schedule != 0) && o.fuse_blocks && !yk_dev_env("YK_X_NOPERSIST");
    o.heads = yk_env_flag("YK_HEADS", latency_schedule != 0) && o.fuse_blocks && !yk_dev_env("YK_X_NOHEADS");
    o.fuse_head = yk_env_flag("YK_FUSE_HEAD", true) && o.fuse_blocks && !o.heads;       // (YK_FUSE_DWPW=0: one launch per layer, everywhere)
    o.splitk = yk_env_flag("YK_SPLITK", true);
    o.cluster_wt = yk_env_flag("YK_CLUSTER_WT", false);
    return o;
}

// tile configuration, ring depth and K split of a plain conv launch: fixed for max_batch (Mmax = max_batch x output pixels), an image's
// arithmetic never depends on the batch
struct xconv_tiling {
    int cfg, ns, splitk;
    long tiles;
};
xconv_tiling x_conv_tiling(int co, long Mmax, int nsteps, const xopts &opt) {
    xconv_tiling t;
    int cfg;
    if (co <= 64) cfg = Mmax >= 30000 ? XC_128x64 : XC_64x64;
    else if (Mmax >= 60000 && co >= 96) cfg = XC_128x128;
    else cfg = XC_64x128;
    if (co > 64 && co <= 96 && Mmax < 60000) cfg = XC_64x128;
    long tiles = ((Mmax + g_xc[cfg].bm - 1) / g_xc[cfg].bm) * ((co + g_xc[cfg].bn - 1) / g_xc[cfg].bn);
    if (cfg == XC_64x128 && tiles < 256) {             // too few workgroups for the chip: the narrow tile doubles them
        cfg = XC_64x64;
        tiles = ((Mmax + 63) / 64) * ((co + 63) / 64);
    }
    if (const char *e = yk_dev_env("YK_X_CFG")) {
        const int v = atoi(e);
        if (v >= 0 && v < XC_NUM) cfg = v;
        tiles = ((Mmax + g_xc[cfg].bm - 1) / g_xc[cfg].bm) * ((co + g_xc[cfg].bn - 1) / g_xc[cfg].bn);
    }
    t.cfg = cfg;
    t.tiles = tiles;
    // ring depth: 3 stages from K = 416 on.  (One batch in flight, K = 384 is a tie between 2 and 3; with three batches in
    // flight 2 stages are +3.5 % on the whole step (tools/sweep3.sh): 48 KB less LDS per workgroup lets another stream's
    // kernel onto the CU.)
    t.ns = nsteps >= (yk_dev_env("YK_X_NS3") ? atoi(yk_dev_env("YK_X_NS3")) : 13) ? 3 : 2;
    long sk = 1;
    if (tiles < 384 && nsteps >= 32) sk = std::min<long>(std::min<long>(7, (900 + tiles - 1) / tiles), nsteps / 8);   // measured (tools/xsweep.py): 7 slices at 105 tiles (8: +25 %), 4 at 280 (3: +9 %)
    if (!opt.splitk) sk = 1;
    if (const char *e = yk_dev_env("YK_X_SPLITK")) sk = std::max(1, std::min(atoi(e), nsteps));
    // a K-split launch is a small grid of long loops (the 3x3 head convs): two stages (32 KB) instead of three leave room on the CU
    // for the other batches' workgroups - the launch alone takes the same time (62.3 / 63.1 us), four batches in flight gain 1 %
    if (sk > 1 && !yk_dev_env("YK_X_SK_NS3")) t.ns = 2;
    if (const char *e = yk_dev_env("YK_X_NS")) t.ns = std::max(2, std::min(4, atoi(e)));
    t.splitk = (int)std::max<long>(1, sk);
    return t;
}

// K slices and ring depth of a fused head (yk_xfin.h):
// one workgroup = 64 rows x all channels, at most six K slices, about 420 workgroups (the 64x64 split-K form: 735 / 1120 workgroups
// that each re-read their operands from L2)
// The slice count follows the IMAGE size (priced for the 32-image batch of the benchmark), never max_batch: an image's
// arithmetic must not depend on how many images the plan was built for.
struct xfin_tiling {
    int splitk, ns;
};
xfin_tiling x_fin_tiling(int co, int HoWo, int nsteps, const xopts &opt) {
    const int bm = 64;
    const long tiles32 = (32L * HoWo + bm - 1) / bm;
    // measured with four batches in flight (tools/calls r6c5, developer build, one box; three-launch form 93.0 k images/s):
    // slices (192-ch head, 128-ch head) = (8, 2) 94.0 k, (4, 4) 94.3 k, (6, 3) 94.8 k, (8, 4) 93.6 k; 128-row tiles 91.0 - 93.5 k
    long sk = std::max<long>(1, std::min<long>(std::min<long>(6, (420 + tiles32 / 2) / tiles32), nsteps / 8));
    if (!opt.splitk) sk = 1;
    if (const char *e = yk_dev_env("YK_XF_SPLITK")) sk = std::max(1, std::min(atoi(e), nsteps));
    if (const char *e = yk_dev_env(co == 192 ? "YK_XF_SPLITK_192" : "YK_XF_SPLITK_128")) sk = std::max(1, std::min(atoi(e), nsteps));
    xfin_tiling t;
    t.splitk = (int)sk;
    t.ns = 2;
    if (const char *e = yk_dev_env("YK_XF_NS")) t.ns = std::max(2, std::min(3, atoi(e)));
    return t;
}

// a fused block's tile geometry, chosen when the fusion is decided
struct xfuse {
    xb_args g;
    int tm = 0, tn = 0;
    unsigned lds = 0, ring = 0;    // dynamic LDS with / without the output staging area
};

struct xbuilder {
    yk_xplan *p;
    const int32_t *ops;
    int n_ops;
    const float *blob;
    int max_batch;
    xopts opt;
    std::vector<int> add_of, dw_of, stem_of, fin_of;       // conv op i -> the Add folded into it, the depthwise conv / stem in front, the 1x1 output conv behind
    std::vector<char> skip, gone;                           // op i emits no launch of its own / tensor t is never allocated
    std::vector<xfuse> fuse;
    // [per-image running maxima][tickets of the fused heads' K-slice reduction (yk_xfin.h)][barrier granules of the persistent stage and of the heads:
    // [image][barrier parity][member] x 8 bytes each, addressed from the END] - everything the step's first launch clears
    static constexpr size_t XF_TICKETS = 8192;
    size_t ticket_base = 0, ticket_used = 0;

    const int32_t *op(int i) const { return ops + (size_t)i * YK_OP_FIELDS; }
    uint32_t *amax_of(int tid) const { return p->d_amax + (size_t)tid * max_batch * XS; }
    int *eexp_of(int tid) const { return p->d_eexp + (size_t)tid * max_batch; }
    xview view_of(int tid) const {
        const xtens &t = p->T[tid];
        xview v;
        v.p = t.d;
        v.eexp = eexp_of(tid);
        v.amax = amax_of(tid);
        v.bytes = (uint32_t)((size_t)max_batch * t.h * t.w * t.cp * 4);
        v.G = t.cp >> 3;
        v.H = t.h;
        v.W = t.w;
        return v;
    }

    int analyse(const int32_t *tensors, int n_tensors, size_t blob_len, const int32_t *outputs, int n_outputs) {
        yk_graph_tensors(p->T, tensors, n_tensors);
        p->in_h = p->T[0].h;
        p->in_w = p->T[0].w;
        for (int i = 0; i < n_outputs; ++i) p->outputs.push_back(outputs[i]);
        dw_of.assign(n_ops, -1);
        stem_of.assign(n_ops, -1);
        fin_of.assign(n_ops, -1);
        fuse.resize(n_ops);
        gone.assign(n_tensors, 0);
        return yk_graph_analyse(p->T, ops, n_ops, blob_len, p->outputs, add_of, skip);
    }

    // DepthwiseConv2D(3x3) whose only consumer is the next op, a 1x1 stride-1 Conv2D: one launch (yk_xblock.h), the depthwise
    // tensor is never allocated.  The tile geometry is chosen here, for max_batch.
    void decide_blocks() {
        int n_fused_seen = 0;
        if (!opt.fuse_blocks) return;
        for (int i = 0; i + 1 < n_ops; ++i) {
            const int32_t *o = op(i), *q = o + YK_OP_FIELDS;
            const int y = o[YK_F_OUT];
            if (o[YK_F_TYPE] != YK_OP_DWCONV || q[YK_F_TYPE] != YK_OP_CONV || q[YK_F_K] != 1 || q[YK_F_STRIDE] != 1 || q[YK_F_IN0] != y ||
                p->T[y].uses != 1 || p->T[y].kind != T_REAL || p->T[o[YK_F_IN0]].kind != T_REAL || p->T[o[YK_F_IN0]].is_input ||
                (q[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT))
                continue;
            xfuse &f = fuse[i + 1];
            memset(&f.g, 0, sizeof(f.g));
            f.g.Ho = p->T[y].h;
            f.g.Wo = p->T[y].w;
            f.g.N = q[YK_F_COUT];
            f.g.stride = o[YK_F_STRIDE];
            f.g.nk = ((p->T[y].cp >> 3) + 3) / 4;
            // measured (K2, B=32): one launch wins or ties down to 14x20 pixels per image; at 7x10 (2240 GEMM rows) the two-launch form
            // is faster (28 vs 39 us, 34 vs 60 us): too few workgroups to hide the fused pipeline's per-step DMA round trips
            // (the rule looks at the image only, not at max_batch: whether a block is fused changes its rounding, and an image's
            // results must not depend on how many images the plan was built for)
            // and up to 384 input channels (round 5, with the weight fragments out of LDS: 35.8 us against 16 + 21.5 at 14x20x384, +4.7 % images/s
            // with four batches in flight; rounds 3-4, with the weight tile in LDS, had the two-launch form ahead from 384 on).  Where the
            // persistent stage takes the 14x20x384 blocks (latency schedule) they stay separate launches for it to collect.
            const int max_nk = yk_dev_env("YK_XB_MAXNK") ? atoi(yk_dev_env("YK_XB_MAXNK")) : (opt.persist ? 6 : 12);
            const int min_px = yk_dev_env("YK_XB_MINPX") ? atoi(yk_dev_env("YK_XB_MINPX")) : 128;
            if ((f.g.Ho * f.g.Wo < min_px || f.g.nk > max_nk) && !yk_dev_env("YK_XB_ALWAYS")) continue;
            if (!xb_geometry(f.g, &f.tm, &f.tn, &f.lds, max_batch, n_fused_seen++)) continue;
            f.ring = xb_lds(f.tm, f.tn, f.g.n16p, f.g.db, f.g.N, false, false);
            dw_of[i + 1] = i;
            skip[i] = 1;
            gone[y] = 1;
        }
    }

    // The network's first conv feeding (only) a fused block: computed inside that block's kernel from the frames (yk_xblock.h), its
    // output tensor is never allocated.  Needs the frame window of a patch to fit in the block's A-tile space.
    void decide_stem() {
        if (!opt.fuse_blocks || yk_dev_env("YK_X_NOSTEMFUSE")) return;
        for (int i = 0; i + 2 < n_ops; ++i) {
            const int32_t *o = op(i);
            if (o[YK_F_TYPE] != YK_OP_CONV || !p->T[o[YK_F_IN0]].is_input) continue;
            const int y = o[YK_F_OUT], co = o[YK_F_COUT];
            const int32_t *d = o + YK_OP_FIELDS;
            if (d[YK_F_TYPE] != YK_OP_DWCONV || d[YK_F_IN0] != y || dw_of[i + 2] != i + 1 || p->T[y].uses != 1 || o[YK_F_K] != 3 ||
                (co != 16 && co != 24 && co != 32) || (o[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT))
                continue;
            xfuse &f = fuse[i + 2];
            const int st = o[YK_F_STRIDE], WR = (f.g.PH - 1) * st + 3, WC = (f.g.PW - 1) * st + 3;
            if (f.g.nk != 1 || f.tn != 1) continue;
            // the patch and the A tile of a stem-fed block hold the channel groups the stem HAS (yk_xblock.h: xb_args::GL); the A tile's
            // space first holds the frame window (fp32 frames: WR x WC x 3 floats), so it is at least that large
            const int GL = co / 8, n16 = f.g.PH * f.g.PW * GL, n16p = (n16 + 63) & ~63;
            const int abytes = std::max(16 * f.tm * GL * 32, (WR * WC * 3 * 4 + 8 + 63) & ~63);
            const int ring = n16p * 32 + 2048 + abytes, ct = f.tm * 16 * (64 * 4 + 16);
            const unsigned lds = (unsigned)(std::max(ring, ct) + 64);
            if (lds > f.lds) continue;
            f.g.GL = GL;
            f.g.n16 = n16; f.g.n16p = n16p;
            f.g.lds_bytes = (int)lds;
            f.lds = lds;
            f.ring = (unsigned)(ring + 64);
            stem_of[i + 2] = i;
            skip[i] = 1;
            gone[y] = 1;
        }
    }

    // A detection head: Conv2D (3x3 | 1x1, stride 1) + BN + act whose ONLY consumer is the next op, the 1x1 NET_OUTPUT conv (yolonet.py:27-29,
    // 35-38): one launch (yk_xfin.h), the 128- / 192-channel tensor between them is never allocated.  Not where the heads cluster launch
    // (latency schedule) collects these convs.  The rule looks at the network only, never at the batch.
    void decide_fin_heads() {
        if (!opt.fuse_head) return;
        for (int i = 0; i + 1 < n_ops; ++i) {
            const int32_t *o = op(i), *q = o + YK_OP_FIELDS;
            const int y = o[YK_F_OUT], co = o[YK_F_COUT];
            if (o[YK_F_TYPE] != YK_OP_CONV || skip[i] || dw_of[i] >= 0 || add_of[i] >= 0 || (o[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT) ||
                p->T[o[YK_F_IN0]].is_input || o[YK_F_STRIDE] != 1 || (co != 128 && co != 192))
                continue;
            if (q[YK_F_TYPE] != YK_OP_CONV || !(q[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT) || q[YK_F_K] != 1 || q[YK_F_STRIDE] != 1 || q[YK_F_IN0] != y ||
                q[YK_F_COUT] > 80 || add_of[i + 1] >= 0 || p->T[y].uses != 1 || p->T[y].kind != T_REAL)
                continue;
            fin_of[i] = i + 1;
            skip[i + 1] = 1;
            gone[y] = 1;
        }
    }

    int alloc_tensors() {
        int rc;
        for (int i = 1; i < (int)p->T.size(); ++i) {
            xtens &t = p->T[i];
            if (t.kind != T_REAL || gone[i]) continue;
            bool folded = false;
            for (int k = 0; k < n_ops; ++k)
                if (op(k)[YK_F_OUT] == i && add_of[k] >= 0) folded = true;
            if (folded) continue;
            if (t.net_out) {
                if ((rc = p->mem.alloc((void **)&t.d32, ((size_t)max_batch * t.h * t.w * t.c + 64) * sizeof(float)))) return rc;
            } else {
                const size_t bytes = (size_t)max_batch * t.h * t.w * t.cp * 4;
                if (bytes >= X_OOB) {
                    yk_set_error("tensor %d: %zu bytes >= 1 GiB; lower max_batch", i, bytes);
                    return YK_ERR_UNSUPPORTED;
                }
                if ((rc = p->mem.alloc((void **)&t.d, bytes + 256))) return rc;
            }
        }
        return YK_OK;
    }

    // per-image maxima of the frames, the region every step's first launch clears (see XF_TICKETS), the error word, the storage exponents
    int alloc_step_state() {
        const size_t n_tensors = p->T.size();
        int rc;
        if ((rc = p->mem.alloc((void **)&p->d_imgmax, sizeof(unsigned) * max_batch * 32))) return rc;
        ticket_base = n_tensors * max_batch * XS;
        p->zero_words = ticket_base + XF_TICKETS + 2 * (size_t)max_batch * 2 * 8 * 2;
        if ((rc = p->mem.alloc((void **)&p->d_amax, sizeof(uint32_t) * p->zero_words))) return rc;
        {   // the error word lives in mapped host memory: a failing cluster writes it over the link once, the host polls it for free
            void *h = nullptr, *d = nullptr;
            if (hipHostMalloc(&h, 256, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
                if (h) (void)hipHostFree(h);
                yk_set_error("yk_plan_create: pinned error word: %s", hipGetErrorString(hipGetLastError()));
                return YK_ERR_HIP;
            }
            memset(h, 0, 256);
            p->h_err = (uint32_t *)h;
            p->d_err = (uint32_t *)d;
        }
        return p->mem.alloc((void **)&p->d_eexp, sizeof(int) * n_tensors * max_batch);
    }

    // conv weights -> device, split and tile-ordered: w * 2^s = hi + lo with max |w * 2^s| in [2^13, 2^14); [step][16-row block][hi|lo][16][32],
    // the 16-byte chunk c of row r stored at position c ^ ((r >> 1) & 3); K walk: segment-major (source 0, then source 1), tap, channel.
    // Also returns the per-source gains max_n |scale_n| * sum_k |w_nk| and max |bias| for the output bound.
    int pack_w(const int32_t *o, int c0, int nc0, int nc1, int taps, int nslab, const uint8_t **dw, uint32_t *dbytes, const float **dscale,
               const float **dbias, float *gain0, float *gain1, float *off) {
        const int co = o[YK_F_COUT], cin = o[YK_F_CIN];
        const int nsteps = taps * (nc0 + nc1);
        const size_t nw = (size_t)co * taps * cin;
        // everything below the three source ranges is computed where the store has no entry for them yet: the tiles, and with them the
        // weight exponent and the gains {gain0, gain1, off, sexp}
        const std::vector<yk_wsrc> src{{blob + o[YK_F_W_OFF], nw * sizeof(float)}, {blob + o[YK_F_SCALE_OFF], (size_t)co * sizeof(float)},
                                       {blob + o[YK_F_BIAS_OFF], (size_t)co * sizeof(float)}};
        const auto pack = [&](std::vector<uint8_t> &out, std::vector<float> &aux) {
            float wmax = 0.f;
            for (size_t k = 0; k < nw; ++k) wmax = std::max(wmax, fabsf(blob[o[YK_F_W_OFF] + k]));
            const int sexp = (wmax > 0.f && std::isfinite(wmax)) ? 13 - ilogbf(wmax) : 0;
            out.assign((size_t)nsteps * nslab * 1024 * sizeof(uint16_t), 0);
            uint16_t *wt = reinterpret_cast<uint16_t *>(out.data());
            std::vector<double> sum0(co, 0.0), sum1(co, 0.0);
            for (int n = 0; n < co; ++n)
                for (int t = 0; t < taps; ++t)
                    for (int c = 0; c < cin; ++c) {
                        const float wv = blob[o[YK_F_W_OFF] + ((size_t)n * taps + t) * cin + c];
                        const bool second = c >= c0;
                        const int cc = second ? c - c0 : c;
                        const int step = second ? taps * nc0 + (cc / 32) * taps + t : (cc / 32) * taps + t;      // channel step outer, tap inner
                        const int k32 = cc % 32, chunk = k32 >> 3, e = k32 & 7, r = n & 15, pos = chunk ^ ((r >> 1) & 3);
                        const float v = ldexpf(wv, sexp);
                        const uint16_t hi = yk_f2h(v);
                        const size_t at = ((size_t)step * nslab + (n >> 4)) * 1024 + (size_t)r * 32 + pos * 8 + e;
                        wt[at] = hi;
                        wt[at + 512] = yk_f2h(v - yk_h2f(hi));
                        (second ? sum1 : sum0)[n] += fabs((double)wv);
                    }
            float g0 = 0.f, g1 = 0.f, of = 0.f;
            for (int n = 0; n < co; ++n) {
                const float sc = fabsf(blob[o[YK_F_SCALE_OFF] + n]);
                g0 = std::max(g0, (float)(sc * sum0[n]));
                g1 = std::max(g1, (float)(sc * sum1[n]));
                of = std::max(of, fabsf(blob[o[YK_F_BIAS_OFF] + n]));
            }
            aux = {g0 * 1.0001f, g1 * 1.0001f, of * 1.0001f, (float)sexp};
        };
        std::vector<float> aux;
        size_t bytes;
        int rc2 = p->mem.packed(YK_WT_XW, {co, cin, c0, nc0, nc1, taps, nslab}, src, pack, dw, &bytes, &aux);
        if (rc2) return rc2;
        *dbytes = (uint32_t)bytes;
        *gain0 = aux[0];
        *gain1 = aux[1];
        *off = aux[2];
        const int sexp = (int)aux[3];
        if ((rc2 = p->mem.upload_f(blob + o[YK_F_SCALE_OFF], co, dscale, ldexpf(1.f, -sexp)))) return rc2;
        return p->mem.upload_f(blob + o[YK_F_BIAS_OFF], co, dbias);
    }
    // [11][cp] depthwise parameters (nine taps, BN scale, BN bias) -> device; bound of the output from the input's max
    int pack_dw(const int32_t *o, int c, int cp, const float **dpar, float *gain, float *off) {
        const std::vector<yk_wsrc> src{{blob + o[YK_F_W_OFF], (size_t)9 * c * sizeof(float)}, {blob + o[YK_F_SCALE_OFF], (size_t)c * sizeof(float)},
                                       {blob + o[YK_F_BIAS_OFF], (size_t)c * sizeof(float)}};
        const auto pack = [&](std::vector<uint8_t> &out, std::vector<float> &aux) {
            std::vector<float> par((size_t)11 * cp, 0.f);
            float g = 0.f, of = 0.f;
            for (int k = 0; k < c; ++k) {
                float sw = 0.f;
                for (int t = 0; t < 9; ++t) {
                    const float w = blob[o[YK_F_W_OFF] + (size_t)t * c + k];
                    par[(size_t)t * cp + k] = w;
                    sw += fabsf(w);
                }
                const float sc = blob[o[YK_F_SCALE_OFF] + k], bs = blob[o[YK_F_BIAS_OFF] + k];
                par[(size_t)9 * cp + k] = sc;
                par[(size_t)10 * cp + k] = bs;
                g = std::max(g, fabsf(sc) * sw);
                of = std::max(of, fabsf(bs));
            }
            aux = {g * 1.0001f, of * 1.0001f};
            yk_wput(out, par);
        };
        std::vector<float> aux;
        int rc = p->mem.packed(YK_WT_XDW, {c, cp}, src, pack, dpar, nullptr, &aux);
        if (rc) return rc;
        *gain = aux[0];
        *off = aux[1];
        return YK_OK;
    }
    // the stem conv's output bound from its weights (the normalised image is in [0, 1]: the bound needs no measurement):
    // gain = max_c |scale_c| * sum_t |w_ct|, off = max |bias|, wmax = max |w|
    void stem_gain(const int32_t *so, float *gain, float *off, float *wmax) const {
        *gain = *off = *wmax = 0.f;
        for (int c = 0; c < so[YK_F_COUT]; ++c) {
            float sw = 0.f;
            for (int t = 0; t < 27; ++t) {
                const float wv = blob[so[YK_F_W_OFF] + (size_t)c * 27 + t];
                sw += fabsf(wv);
                *wmax = std::max(*wmax, fabsf(wv));
            }
            *gain = std::max(*gain, sw * fabsf(blob[so[YK_F_SCALE_OFF] + c]));
            *off = std::max(*off, fabsf(blob[so[YK_F_BIAS_OFF] + c]));
        }
    }
    // where conv op i stores: its own output, or - with a residual Add folded into it - the Add's output, `res` then views the other addend
    int residual_dst(int i, xview *res) const {
        const int yid = op(i)[YK_F_OUT];
        if (add_of[i] < 0) return yid;
        const int32_t *q = op(add_of[i]);
        *res = view_of((q[YK_F_IN0] == yid) ? q[YK_F_IN1] : q[YK_F_IN0]);
        return q[YK_F_OUT];
    }

    void emit_u8_max() {
        xlaunch l;
        l.kind = XK_U8MAX;
        l.name = "u8_max";
        l.bytes = (double)p->in_h * p->in_w * 3;
        p->L.push_back(l);
    }

    // the launch of op i, if it has one of its own
    int emit(int i) {
        if (skip[i]) return YK_OK;
        const int32_t *o = op(i);
        const int ty = o[YK_F_TYPE];
        if (ty == YK_OP_UPSAMPLE || ty == YK_OP_CONCAT) return YK_OK;
        xlaunch l;
        l.Ho = p->T[o[YK_F_OUT]].h;
        l.Wo = p->T[o[YK_F_OUT]].w;
        int rc;
        if (ty == YK_OP_CONV && p->T[o[YK_F_IN0]].is_input) rc = emit_stem(i, l);
        else if (ty == YK_OP_CONV && dw_of[i] >= 0) rc = emit_block(i, l);
        else if (ty == YK_OP_CONV) rc = emit_conv(i, l);
        else if (ty == YK_OP_DWCONV) rc = emit_dw(i, l);
        else if (ty == YK_OP_MAXPOOL) rc = emit_pool(i, l);
        else if (ty == YK_OP_ADD) rc = emit_add(i, l);
        else {
            yk_set_error("op %d: unknown op type %d", i, ty);
            rc = YK_ERR_UNSUPPORTED;
        }
        if (rc == YK_OK) p->L.push_back(l);
        return rc;
    }

    int emit_stem(int i, xlaunch &l) {
        const int32_t *o = op(i);
        const int yid = o[YK_F_OUT], co = o[YK_F_COUT];
        const xtens &X = p->T[o[YK_F_IN0]], &Y = p->T[yid];
        int rc;
        if (o[YK_F_K] != 3 || (co != 16 && co != 24 && co != 32) || Y.net_out) {
            yk_set_error("op %d: stem conv must be 3x3 with 16/24/32 filters", i);
            return YK_ERR_UNSUPPORTED;
        }
        const auto pack = [&](std::vector<uint8_t> &out, std::vector<float> &) {
            std::vector<float> w((size_t)27 * co);
            for (int c = 0; c < co; ++c)
                for (int t = 0; t < 27; ++t) w[(size_t)t * co + c] = blob[o[YK_F_W_OFF] + (size_t)c * 27 + t];
            yk_wput(out, w);
        };
        float gain, off, wmax;
        stem_gain(o, &gain, &off, &wmax);
        l.kind = XK_STEM;
        xstem_args &s = l.s;
        memset(&s, 0, sizeof(s));
        if ((rc = p->mem.packed(YK_WT_XSTEM, {co}, {{blob + o[YK_F_W_OFF], (size_t)27 * co * sizeof(float)}}, pack, &s.w))) return rc;
        s.Hi = X.h; s.Wi = X.w; s.Ho = Y.h; s.Wo = Y.w;
        s.stride = o[YK_F_STRIDE]; s.pad_t = o[YK_F_PAD_T]; s.pad_l = o[YK_F_PAD_L];
        s.Cout = co; s.outG = Y.cp >> 3;
        if ((rc = p->mem.upload_f(blob + o[YK_F_SCALE_OFF], co, &s.scale))) return rc;
        if ((rc = p->mem.upload_f(blob + o[YK_F_BIAS_OFF], co, &s.bias))) return rc;
        yk_act_params(o[YK_F_ACT], yk_op_alpha(o), &s.slope, &s.cap);
        const float bound = std::min(s.cap, (gain + off) * 1.0001f);
        s.eo = (bound > 0.f && std::isfinite(bound)) ? ilogbf(bound) - 13 : 0;
        s.out = Y.d;
        s.eexp_out = eexp_of(yid);
        s.amax_out = amax_of(yid);
        char nm[112];
        snprintf(nm, sizeof nm, "x:stem3x3s%d_%d", s.stride, co);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * 27 * co;
        l.bytes = (double)X.h * X.w * 3 * 4 + (double)Y.h * Y.w * co * 4;
        return YK_OK;
    }

    // the stem conv `so` computed inside the fused block g (decide_stem); S is the tensor between them, which does not exist
    int fuse_stem_into(xb_args &g, const int32_t *so, const xtens &S, char *stn, size_t stn_len, double *flops, double *bytes) {
        const xtens &F = p->T[so[YK_F_IN0]];
        const int sco = so[YK_F_COUT];
        int rc;
        float gain, off, wmax;
        stem_gain(so, &gain, &off, &wmax);
        // MFMA fragments of the 32 x 32 weight matrix (k = ky*8 + j for the first eight of a filter row's nine values, 24 + ky
        // for the ninth), w * 2^s = hi + lo
        const int sexp = (wmax > 0.f && std::isfinite(wmax)) ? 13 - ilogbf(wmax) : 0;
        const auto pack = [&](std::vector<uint8_t> &out, std::vector<float> &) {
            std::vector<uint16_t> wf((size_t)2 * 2 * 64 * 8, 0);
            for (int nf = 0; nf < 2; ++nf)
                for (int ln = 0; ln < 64; ++ln)
                    for (int e = 0; e < 8; ++e) {
                        const int n = nf * 16 + (ln & 15), k = (ln >> 4) * 8 + e;
                        int t = -1;
                        if (k < 24) t = (k >> 3) * 9 + (k & 7);            // tap row ky = k/8, j = kx*3 + ci
                        else if (k < 27) t = (k - 24) * 9 + 8;
                        if (n >= sco || t < 0) continue;
                        const float v = ldexpf(blob[so[YK_F_W_OFF] + (size_t)n * 27 + t], sexp);
                        const uint16_t hi = yk_f2h(v);
                        wf[((size_t)(nf * 2 + 0) * 64 + ln) * 8 + e] = hi;
                        wf[((size_t)(nf * 2 + 1) * 64 + ln) * 8 + e] = yk_f2h(v - yk_h2f(hi));
                    }
            yk_wput(out, wf);
        };
        if ((rc = p->mem.packed(YK_WT_XSTEM_FRAG, {sco}, {{blob + so[YK_F_W_OFF], (size_t)27 * sco * sizeof(float)}}, pack, &g.st_wf))) return rc;
        g.stem = 1;
        if ((rc = p->mem.upload_f(blob + so[YK_F_SCALE_OFF], sco, &g.st_scale, ldexpf(1.f, -sexp)))) return rc;
        if ((rc = p->mem.upload_f(blob + so[YK_F_BIAS_OFF], sco, &g.st_bias))) return rc;
        yk_act_params(so[YK_F_ACT], yk_op_alpha(so), &g.st_slope, &g.st_cap);
        g.st_stride = so[YK_F_STRIDE]; g.st_pad_t = so[YK_F_PAD_T]; g.st_pad_l = so[YK_F_PAD_L]; g.st_cout = sco;
        g.fH = F.h; g.fW = F.w;
        g.fd_wrow = yk_make_fastdiv((uint32_t)(((g.PW - 1) * g.st_stride + 3) * 3));
        g.fd_dpr = yk_make_fastdiv((uint32_t)((((g.PW - 1) * g.st_stride + 3) * 3 + 3) / 4));
        g.st_bound = std::min(g.st_cap, (gain + off) * 1.0001f);               // the normalised image is in [0, 1]
        g.st_e = (g.st_bound > 0.f && std::isfinite(g.st_bound)) ? ilogbf(g.st_bound) - 13 : 0;
        g.in.p = nullptr;                                                       // the tensor does not exist
        snprintf(stn, stn_len, "stem3x3s%d_%d+", g.st_stride, sco);
        *flops = 2.0 * S.h * S.w * 27 * sco;
        *bytes = (double)F.h * F.w * 3 * 4 + (double)S.h * S.w * sco * 4;
        return YK_OK;
    }

    // depthwise + pointwise (+ stem, + residual) as one launch
    int emit_block(int i, xlaunch &l) {
        const int32_t *o = op(i), *dwo = op(dw_of[i]);
        const int sid = dwo[YK_F_IN0];
        const xtens &S = p->T[sid], &Y = p->T[o[YK_F_OUT]];
        int rc;
        l.kind = XK_BLOCK;
        l.tm = fuse[i].tm;
        l.tn = fuse[i].tn;
        l.lds = fuse[i].lds;
        l.ring_lds = fuse[i].ring;
        xb_args &g = l.b;
        g = fuse[i].g;
        const int co = o[YK_F_COUT], cin = o[YK_F_CIN];
        float g1, dwgain, dwoff;
        g.in = view_of(sid);
        g.pad_t = dwo[YK_F_PAD_T];
        g.pad_l = dwo[YK_F_PAD_L];
        double st_flops = 0, st_bytes = 0;
        char stn[40] = "";
        if (stem_of[i] >= 0 && (rc = fuse_stem_into(g, op(stem_of[i]), S, stn, sizeof stn, &st_flops, &st_bytes))) return rc;
        if ((rc = pack_dw(dwo, S.c, S.cp, &g.par, &dwgain, &dwoff))) return rc;
        yk_act_params(dwo[YK_F_ACT], yk_op_alpha(dwo), &g.dw_slope, &g.dw_cap);
        g.dw_gain = dwgain;
        g.dw_off = dwoff;
        const int BN = 64 * l.tn;
        g.nslab = ((co + BN - 1) / BN) * (BN / 16);
        if ((rc = pack_w(o, cin, g.nk, 0, 1, g.nslab, &g.w, &g.w_bytes, &g.scale, &g.bias, &g.gain, &g1, &g.off))) return rc;
        yk_act_params(o[YK_F_ACT], yk_op_alpha(o), &g.slope, &g.cap);
        const int dst_id = residual_dst(i, &g.res);
        const xtens *dst = &p->T[dst_id];
        g.out = dst->d;
        g.outG = dst->cp >> 3;
        g.eexp_out = eexp_of(dst_id);
        g.amax_out = amax_of(dst_id);
        if (!g.out) {
            yk_set_error("op %d: output tensor not allocated", i);
            return YK_ERR_UNSUPPORTED;
        }
        char nm[112];
        snprintf(nm, sizeof nm, "x:%sdw3x3s%d+conv1x1_%dto%d%s[%dx%dpx,%dch,%dstage]", stn, g.stride, cin, co, g.res.p ? "+add" : "", g.TH, g.TW, 64 * l.tn, g.db ? 2 : 1);
        l.name = nm;
        // algorithmic work of everything this launch replaces, counted unfused: stem + depthwise + pointwise
        l.flops = 2.0 * Y.h * Y.w * (double)cin * co + 2.0 * Y.h * Y.w * 9 * cin + st_flops;
        l.bytes = ((double)S.h * S.w * S.c + 2.0 * Y.h * Y.w * cin + (double)Y.h * Y.w * co) * 4 + st_bytes;
        return YK_OK;
    }

    // K slices, ring depth, slabs and tile counters of a fused head
    int plan_fin(int i, xlaunch &l, long Mmax, int nsteps) {
        xg_args &g = l.c;
        const int co = g.N, bm = 64;
        const long tiles = (Mmax + bm - 1) / bm;
        const xfin_tiling t = x_fin_tiling(co, g.HoWo, nsteps, opt);
        int rc;
        g.splitk = t.splitk;
        l.ns = t.ns;
        l.fin_bn = co;
        l.f.slab_bytes = 0;
        if (g.splitk > 1) {
            void *sl;
            const size_t sb = (size_t)g.splitk * tiles * bm * co * 4;
            if ((rc = p->mem.alloc(&sl, sb))) return rc;
            g.slab = (float *)sl;
            l.f.slab_bytes = (uint32_t)sb;
        }
        // the tile counters live in the region every step's first launch clears (the last arriver also clears its own: a step that was
        // cut short cannot leave a count behind for the next one)
        if (ticket_used + (size_t)tiles > XF_TICKETS) {
            yk_set_error("op %d: %ld head tiles: more than the %zu ticket slots of a plan; lower max_batch", i, tiles, XF_TICKETS);
            return YK_ERR_UNSUPPORTED;
        }
        l.f.ticket = p->d_amax + ticket_base + ticket_used;
        ticket_used += (size_t)tiles;
        return YK_OK;
    }
    // tile configuration, ring depth, K split and slabs of a plain conv launch
    int plan_conv(xlaunch &l, long Mmax, int nsteps) {
        xg_args &g = l.c;
        const xconv_tiling t = x_conv_tiling(g.N, Mmax, nsteps, opt);
        l.cfg = t.cfg;
        l.ns = t.ns;
        g.splitk = t.splitk;
        if (g.splitk > 1) {
            void *sl;
            const int tm = g_xc[t.cfg].bm * g_xc[t.cfg].bn / 16 / (g_xc[t.cfg].threads / 64) / 16;   // floatx4 registers per thread
            int rc;
            if ((rc = p->mem.alloc(&sl, (size_t)g.splitk * t.tiles * tm * g_xc[t.cfg].threads * 16))) return rc;
            g.slab = (float *)sl;
        }
        return YK_OK;
    }

    // a conv launch; with fin_of[i], a detection head that ends in its 1x1 NET_OUTPUT conv (finish_fin)
    int emit_conv(int i, xlaunch &l) {
        const int32_t *o = op(i);
        const int xid = o[YK_F_IN0];
        const xtens &X = p->T[xid], &Y = p->T[o[YK_F_OUT]];
        int rc;
        l.kind = XK_CONV;
        xg_args &g = l.c;
        memset(&g, 0, sizeof(g));
        int s0 = xid, s1 = -1, up0 = 0;
        if (X.kind == T_CAT) {
            s0 = X.src0;
            s1 = X.src1;
        }
        if (p->T[s0].kind == T_UP) {
            up0 = 1;
            s0 = p->T[s0].src0;
        }
        const xtens &S0 = p->T[s0];
        const xtens *S1 = s1 >= 0 ? &p->T[s1] : nullptr;
        if (S0.kind != T_REAL || (S1 && S1->kind != T_REAL) || !S0.d || (S1 && !S1->d)) {
            yk_set_error("op %d: unsupported input view nesting", i);
            return YK_ERR_UNSUPPORTED;
        }
        const int ks = o[YK_F_K], co = o[YK_F_COUT], cin = o[YK_F_CIN];
        const int c0 = S0.c, G0 = S0.cp >> 3, c1 = S1 ? S1->c : 0, G1 = S1 ? S1->cp >> 3 : 0;
        if (c0 + c1 != cin || (ks != 1 && ks != 3)) {
            yk_set_error("op %d: conv shape mismatch", i);
            return YK_ERR_UNSUPPORTED;
        }
        if (S1 && (S0.cp % 32) != 0) {
            yk_set_error("op %d: f16x2 concat needs the first source's channels in multiples of 32 (got %d)", i, S0.cp);
            return YK_ERR_UNSUPPORTED;
        }
        g.s0 = view_of(s0);
        if (S1) g.s1 = view_of(s1);
        g.up0 = up0;
        g.Hi = X.h; g.Wi = X.w; g.Ho = Y.h; g.Wo = Y.w; g.HoWo = Y.h * Y.w;
        g.ks = ks; g.stride = o[YK_F_STRIDE]; g.pad_t = o[YK_F_PAD_T]; g.pad_l = o[YK_F_PAD_L];
        g.N = co;
        g.taps = ks * ks;
        g.nc0 = (G0 + 3) / 4;
        g.nc1 = S1 ? (G1 + 3) / 4 : 0;
        // tile shape and K split are fixed here, for max_batch: an image's arithmetic never depends on the batch
        const long Mmax = (long)max_batch * Y.h * Y.w;
        const int nsteps = g.taps * (g.nc0 + g.nc1);
        const bool fin = fin_of[i] >= 0;
        if ((rc = fin ? plan_fin(i, l, Mmax, nsteps) : plan_conv(l, Mmax, nsteps))) return rc;
        const int BN = fin ? co : g_xc[l.cfg].bn;
        g.nslab = ((co + BN - 1) / BN) * (BN / 16);
        if ((rc = pack_w(o, c0, g.nc0, g.nc1, g.taps, g.nslab, &g.w, &g.w_bytes, &g.scale, &g.bias, &g.gain0, &g.gain1, &g.off))) return rc;
        yk_act_params(o[YK_F_ACT], yk_op_alpha(o), &g.slope, &g.cap);
        g.fd_hw = yk_make_fastdiv((uint32_t)(Y.h * Y.w));
        g.fd_wo = yk_make_fastdiv((uint32_t)Y.w);
        l.in_tid = (S1 || up0) ? -1 : s0;
        const int dst_id = residual_dst(i, &g.res);
        const xtens *dst = &p->T[dst_id];
        const char *view = S1 ? "+upcat" : (up0 ? "+up" : "");
        const double in_elems = (double)S0.h * S0.w * c0 + (S1 ? (double)S1->h * S1->w * c1 : 0.0);
        if (fin) return finish_fin(i, l, view, in_elems);
        if (dst->net_out) {
            g.out32 = dst->d32;
        } else {
            g.out = dst->d;
            g.outG = dst->cp >> 3;
            g.eexp_out = eexp_of(dst_id);
            g.amax_out = amax_of(dst_id);
            l.out_tid = dst_id;
        }
        if (!g.out && !g.out32) {
            yk_set_error("op %d: output tensor not allocated", i);
            return YK_ERR_UNSUPPORTED;
        }
        char nm[112], tl[48];
        snprintf(tl, sizeof tl, "[%s,ring%d%s]", g_xc[l.cfg].name, l.ns, g.splitk > 1 ? ",splitk" : "");
        snprintf(nm, sizeof nm, "x:conv%dx%ds%d_%dto%d%s%s%s", ks, ks, g.stride, cin, co, g.res.p ? "+add" : "", view, tl);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * ks * ks * (double)cin * co;
        l.bytes = (in_elems + (double)Y.h * Y.w * co) * 4;
        return YK_OK;
    }
    // the conv's own output never exists; the launch ends in the 1x1 NET_OUTPUT conv
    int finish_fin(int i, xlaunch &l, const char *view, double in_elems) {
        const int32_t *o = op(i), *q = op(fin_of[i]);
        const xtens &Y = p->T[o[YK_F_OUT]], &Z = p->T[q[YK_F_OUT]];
        const xg_args &g = l.c;
        const int ks = g.ks, co = g.N, cin = o[YK_F_CIN];
        xf_args &f = l.f;
        f.N2 = q[YK_F_COUT];
        f.nslab2 = 5;
        uint32_t wb2;
        float ga, gb, go;
        int rc;
        if ((rc = pack_w(q, co, co / 32, 0, 1, f.nslab2, &f.w2, &wb2, &f.scale2, &f.bias2, &ga, &gb, &go))) return rc;
        yk_act_params(q[YK_F_ACT], yk_op_alpha(q), &f.slope2, &f.cap2);
        f.out32 = Z.d32;
        if (!f.out32) {
            yk_set_error("op %d: network output not allocated", fin_of[i]);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = XK_FIN;
        f.c = g;
        char nm[112], tl[64];
        snprintf(tl, sizeof tl, "[64x%d,4waves,ring%d%s]", co, l.ns, g.splitk > 1 ? ",splitk" : "");
        snprintf(nm, sizeof nm, "x:conv%dx%ds%d_%dto%d%s+conv1x1_%dto%d%s", ks, ks, g.stride, cin, co, view, co, f.N2, tl);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * ks * ks * (double)cin * co + 2.0 * Y.h * Y.w * (double)co * f.N2;
        l.bytes = (in_elems + 2.0 * Y.h * Y.w * co + (double)Y.h * Y.w * f.N2) * 4;
        return YK_OK;
    }

    int emit_dw(int i, xlaunch &l) {
        const int32_t *o = op(i);
        const int xid = o[YK_F_IN0], yid = o[YK_F_OUT];
        const xtens &X = p->T[xid], &Y = p->T[yid];
        if (X.kind != T_REAL || X.is_input) {
            yk_set_error("op %d: depthwise conv on a view/input", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = XK_DW;
        xdw_args &d = l.d;
        memset(&d, 0, sizeof(d));
        const int c = X.c, cp = X.cp;
        float gain, off;
        int rc;
        if ((rc = pack_dw(o, c, cp, &d.par, &gain, &off))) return rc;
        d.in = view_of(xid);
        d.Ho = Y.h; d.Wo = Y.w;
        d.stride = o[YK_F_STRIDE]; d.pad_t = o[YK_F_PAD_T]; d.pad_l = o[YK_F_PAD_L];
        yk_act_params(o[YK_F_ACT], yk_op_alpha(o), &d.slope, &d.cap);
        d.gain = gain;
        d.off = off;
        d.out = Y.d;
        d.eexp_out = eexp_of(yid);
        d.amax_out = amax_of(yid);
        xdw_geometry(d, max_batch);
        l.in_tid = xid;
        l.out_tid = yid;
        l.lds = (unsigned)((size_t)d.n16p * 32);
        char nm[112];
        snprintf(nm, sizeof nm, "x:dw3x3s%d_%d[%dx%dx%d]", d.stride, c, d.TH, d.TW, d.GS * 8);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * 9 * c;
        l.bytes = ((double)X.h * X.w * c + (double)Y.h * Y.w * c) * 4;
        return YK_OK;
    }

    int emit_pool(int i, xlaunch &l) {
        const int32_t *o = op(i);
        const int xid = o[YK_F_IN0], yid = o[YK_F_OUT];
        const xtens &X = p->T[xid], &Y = p->T[yid];
        if (X.kind != T_REAL || X.is_input) {
            yk_set_error("op %d: max pool on a view/input", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = XK_POOL;
        xpool_args &q = l.p;
        memset(&q, 0, sizeof(q));
        q.in = view_of(xid);
        q.Ho = Y.h; q.Wo = Y.w; q.stride = o[YK_F_STRIDE]; q.out = Y.d;
        q.eexp_out = eexp_of(yid);
        q.amax_out = amax_of(yid);
        q.fd_g = yk_make_fastdiv((uint32_t)(X.cp >> 3));
        q.fd_wo = yk_make_fastdiv((uint32_t)Y.w);
        char nm[112];
        snprintf(nm, sizeof nm, "x:maxpool2x2s%d_%d", q.stride, X.c);
        l.name = nm;
        l.bytes = ((double)X.h * X.w * X.c + (double)Y.h * Y.w * Y.c) * 4;
        return YK_OK;
    }

    int emit_add(int i, xlaunch &l) {
        const int32_t *o = op(i);
        const int xid = o[YK_F_IN0], yid = o[YK_F_OUT];
        const xtens &X = p->T[xid], &Y = p->T[yid], &Z = p->T[o[YK_F_IN1]];
        if (X.kind != T_REAL || Z.kind != T_REAL || !X.d || !Z.d || !Y.d) {
            yk_set_error("op %d: standalone Add on views", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = XK_ADD;
        xadd_args &ad = l.ad;
        memset(&ad, 0, sizeof(ad));
        ad.x = view_of(xid);
        ad.y = view_of(o[YK_F_IN1]);
        ad.n_per_image = (size_t)Y.h * Y.w * (Y.cp >> 3);
        ad.out = Y.d;
        ad.eexp_out = eexp_of(yid);
        ad.amax_out = amax_of(yid);
        char nm[112];
        snprintf(nm, sizeof nm, "x:add_%d", Y.c);
        l.name = nm;
        l.bytes = 3.0 * Y.h * Y.w * Y.c * 4;
        return YK_OK;
    }

    int check_activations() const {
        for (const xlaunch &l : p->L) {                                 // x_actf's one-median form (top of yk_exact.hip) does not cover a capped leaky activation
            auto bad = [](float slope, float cap) { return slope > 0.f && std::isfinite(cap); };
            if ((l.kind == XK_CONV && bad(l.c.slope, l.c.cap)) || (l.kind == XK_DW && bad(l.d.slope, l.d.cap)) || (l.kind == XK_STEM && bad(l.s.slope, l.s.cap)) ||
                (l.kind == XK_BLOCK && (bad(l.b.slope, l.b.cap) || bad(l.b.dw_slope, l.b.dw_cap) || (l.b.stem && bad(l.b.st_slope, l.b.st_cap)))) ||
                (l.kind == XK_FIN && (bad(l.f.c.slope, l.f.c.cap) || bad(l.f.slope2, l.f.cap2)))) {
                yk_set_error("f16x2: %s has a leaky activation with a finite cap (not a reference layer)", l.name.c_str());
                return YK_ERR_UNSUPPORTED;
            }
        }
        return YK_OK;
    }

    // A tensor whose ONLY reader is a depthwise conv (of a fused block, a plain depthwise launch or the persistent stage's first phase) is
    // stored as fp32 planes - the same 32 bytes per channel group as (hi | lo): its producer (fused block or conv launch without a residual)
    // skips the split and stores straight from the registers, the depthwise taps skip their conversions
    void mark_f32_planes() {
        if (yk_dev_env("YK_XB_NOF32")) return;
        for (size_t t = 1; t < p->T.size(); ++t) {
            xtens &T = p->T[t];
            if (!T.d || T.uses != 1 || T.net_out || T.is_input) continue;
            xlaunch *prod = nullptr, *cons = nullptr;
            for (xlaunch &l : p->L) {
                if (l.kind == XK_BLOCK && l.b.out == T.d && !l.b.res.p) prod = &l;
                if (l.kind == XK_CONV && l.c.out == T.d && !l.c.res.p) prod = &l;
                if (l.kind == XK_BLOCK && !l.b.stem && l.b.in.p == T.d) cons = &l;
                if (l.kind == XK_DW && l.d.in.p == T.d) cons = &l;
            }
            bool other = false;                                            // read as a matrix operand / residual somewhere: stays (hi | lo)
            for (xlaunch &l : p->L)
                other = other || (l.kind == XK_BLOCK && l.b.res.p == T.d) || (l.kind == XK_CONV && (l.c.s0.p == T.d || l.c.s1.p == T.d || l.c.res.p == T.d)) ||
                        (l.kind == XK_POOL && l.p.in.p == T.d) || (l.kind == XK_ADD && (l.ad.x.p == T.d || l.ad.y.p == T.d));
            if (other || !prod || !cons) continue;
            if (prod->kind == XK_BLOCK) {
                prod->b.dst_f32 = 1;
                // registers -> global memory, no staging area: the launch asks for the patch + A tile only (a 384-wide tile: 22 KB instead of 50)
                if (prod->ring_lds && prod->ring_lds < prod->lds && !yk_dev_env("YK_XB_NOSHRINK")) {
                    prod->lds = prod->ring_lds;
                    prod->b.lds_bytes = (int)prod->ring_lds;
                }
            } else {
                prod->c.dst_f32 = 1;
            }
            if (cons->kind == XK_BLOCK) cons->b.src_f32 = 1; else cons->d.in_f32 = 1;
            T.f32 = true;
        }
    }

    // every network output is there; then waits for the uploads
    int check_outputs() const {
        for (int t : p->outputs)
            if (!p->T[t].d32 || !p->T[t].net_out) {
                yk_set_error("yk_plan_create: output tensor %d is not produced by a NET_OUTPUT conv", t);
                return YK_ERR_UNSUPPORTED;
            }
        YK_HIP(hipDeviceSynchronize());
        return YK_OK;
    }
};

}   // namespace

int yk_xplan_create(yk_xplan **out, const int32_t *ops, int n_ops, const int32_t *tensors, int n_tensors, const float *blob,
                    size_t blob_len, const int32_t *outputs, int n_outputs, int max_batch, int latency_schedule) {
    yk_xplan *p = new yk_xplan();
    p->max_batch = max_batch;
    xbuilder b{p, ops, n_ops, blob, max_batch, x_read_opts(latency_schedule)};
    p->cluster_wt = b.opt.cluster_wt ? 1 : 0;
    int rc = b.analyse(tensors, n_tensors, blob_len, outputs, n_outputs);
    if (!rc) {
        b.decide_blocks();
        b.decide_stem();
        b.decide_fin_heads();
        rc = b.alloc_tensors();
    }
    if (!rc) rc = b.alloc_step_state();
    if (!rc) b.emit_u8_max();
    for (int i = 0; i < n_ops && !rc; ++i) rc = b.emit(i);
    if (!rc) rc = b.check_activations();
    if (!rc) b.mark_f32_planes();
    // The two cluster launches hold every CU for their whole duration: the shortest time of ONE batch (one-batch latency 669 -> 542 us of
    // kernels), but with several batches in flight on several streams the launch-per-layer form overlaps better (78 k vs 68 k images/s, four in
    // flight; profiles/r04_schedules.txt).  YK_SCHEDULE_LATENCY selects them; YK_PERSIST / YK_HEADS = 0|1 override either way.
    if (!rc && b.opt.persist) rc = x_build_persist(p, max_batch);       // (YK_FUSE_DWPW=0: one launch per layer)
    if (!rc && b.opt.heads) rc = x_build_heads(p, max_batch);
    if (!rc) rc = b.check_outputs();
    if (rc) {
        yk_xplan_destroy(p);
        return rc;
    }
    *out = p;
    return YK_OK;
}
