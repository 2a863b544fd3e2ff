// yk_plan_build.h — the f16 plan builder: the precision 'f16' path of yk_plan_create_ex as a list of passes over one builder.  Included by
// yk_engine.hip (which defines yk_plan, tinfo, launch and the K_* launch kinds in front of it); host code only.
#pragma once
#include "yk_plan_graph.h"

namespace {

// The switches the f16 builder reads (README "Environment switches"), sampled once per plan; nothing below reads the environment.
struct plan_opts {
    bool fuse_dwpw;                    // YK_FUSE_DWPW: depthwise + pointwise as one launch where yk_igemm_fused_ok
    bool splitk;                       // YK_SPLITK
    bool reduce_pw;                    // YK_REDUCE_PW: split-K finishing pass + the 1x1 fp32 head conv behind it as one launch
};
plan_opts read_plan_opts() { return {yk_env_flag("YK_FUSE_DWPW", true), yk_env_flag("YK_SPLITK", true), yk_env_flag("YK_REDUCE_PW", true)}; }

// ---- weight packers: host fp32 weights of one op -> the panel its kernel reads ----------------------------------------
// stem [co][27] -> [27][co] floats holding fp16-rounded values
std::vector<float> pack_stem(const float *w, int co) {
    std::vector<float> v((size_t)27 * co);
    for (int c = 0; c < co; ++c)
        for (int t = 0; t < 27; ++t) v[(size_t)t * co + c] = yk_h2f(yk_f2h(w[(size_t)c * 27 + t]));
    return v;
}
// stem again, in the MFMA stem's k order: [32][32] fp16, k = ky*8 + j for the first eight of a filter row's nine values, 24 + ky for the ninth
std::vector<uint16_t> pack_stem_mfma(const float *w, int co) {
    std::vector<uint16_t> v(32 * 32, 0);
    for (int n = 0; n < co; ++n)
        for (int ky = 0; ky < 3; ++ky)
            for (int j = 0; j < 9; ++j) v[(size_t)n * 32 + (j < 8 ? ky * 8 + j : 24 + ky)] = yk_f2h(w[(size_t)n * 27 + ky * 9 + j]);
    return v;
}
// conv [co][tap][c0 + c1] -> fp16 [co][tap][c0p + c1p]: the second concat source starts at c0p, the gap behind each source stays zero
std::vector<uint16_t> pack_conv(const float *w, int co, int taps, int c0, int c0p, int c1, int c1p) {
    const int cin = c0 + c1, ctp = c0p + c1p;
    std::vector<uint16_t> v((size_t)co * taps * ctp, 0);
    for (int n = 0; n < co; ++n)
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < cin; ++c) {
                const int pos = c < c0 ? c : c0p + (c - c0);
                v[((size_t)n * taps + t) * ctp + pos] = yk_f2h(w[((size_t)n * taps + t) * cin + c]);
            }
    return v;
}
// a packed 1x1 panel [co][K] in MFMA fragment order, as the LDS-DMA staged kernel and the LR kernels read it:
// [16-channel slice][k-step of 32][lane][8], element = W[slice*16 + (lane & 15)][kstep*32 + (lane >> 4)*8 + e]; one wave-load = 1 KB contiguous
std::vector<uint16_t> pack_fragments(const std::vector<uint16_t> &w, int co, int K) {
    const int nkf = ((K + 31) & ~31) / 32, nsl = (co + 15) / 16;
    std::vector<uint16_t> v((size_t)nsl * nkf * 512, 0);
    for (int sl = 0; sl < nsl; ++sl)
        for (int ks = 0; ks < nkf; ++ks)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 8; ++e) {
                    const int n = sl * 16 + (ln & 15), k = ks * 32 + (ln >> 4) * 8 + e;
                    if (n < co && k < K) v[(((size_t)sl * nkf + ks) * 64 + ln) * 8 + e] = w[(size_t)n * K + k];
                }
    return v;
}
// depthwise [9][c] -> fp16 [9][cp]
std::vector<uint16_t> pack_dw(const float *w, int c, int cp) {
    std::vector<uint16_t> v((size_t)9 * cp, 0);
    for (int t = 0; t < 9; ++t)
        for (int k = 0; k < c; ++k) v[(size_t)t * cp + k] = yk_f2h(w[(size_t)t * c + k]);
    return v;
}

// tensor table and output list: what every precision's plan keeps in yk_plan itself
int plan_read_tensors(yk_plan *p, const int32_t *tensors, int n_tensors, const int32_t *outputs, int n_outputs) {
    yk_graph_tensors(p->T, tensors, n_tensors);
    if (!p->T[0].is_input || p->T[0].c != 3) {
        yk_set_error("yk_plan_create: tensor 0 must be the 3-channel network input");
        return YK_ERR_UNSUPPORTED;
    }
    p->in_h = p->T[0].h;
    p->in_w = p->T[0].w;
    for (int i = 0; i < n_outputs; ++i) {
        if (outputs[i] < 0 || outputs[i] >= n_tensors) {
            yk_set_error("yk_plan_create: bad output id");
            return YK_ERR_ARG;
        }
        p->outputs.push_back(outputs[i]);
    }
    return YK_OK;
}

struct builder {
    yk_plan *p;
    const int32_t *ops;
    int n_ops;
    const float *blob;
    int max_batch;
    plan_opts opt;
    std::vector<int> add_of, dw_of;        // conv op i -> the Add folded into it, the depthwise conv fused in front of it
    std::vector<char> skip;                // op i emits no launch of its own

    const int32_t *op(int i) const { return ops + (size_t)i * YK_OP_FIELDS; }
    int upload_dw(const float *w, int c, int cp, const yk_half **d) {
        return p->mem.packed(YK_WT_DW, {c, cp}, {{w, (size_t)9 * c * sizeof(float)}},
                             [&](std::vector<uint8_t> &out, std::vector<float> &) { yk_wput(out, pack_dw(w, c, cp)); }, d);
    }
    int upload_scale_bias(const int32_t *o, int n, const float **scale, const float **bias) {
        int rc = p->mem.upload_f(blob + o[YK_F_SCALE_OFF], n, scale);
        return rc ? rc : p->mem.upload_f(blob + o[YK_F_BIAS_OFF], n, bias);
    }

    // views, use counts, output flags and the Adds that fold into their producing conv
    int analyse(size_t blob_len) { return yk_graph_analyse(p->T, ops, n_ops, blob_len, p->outputs, add_of, skip); }

    // DepthwiseConv2D whose only consumer is the next op, a 1x1 Conv2D: one launch where a fused kernel takes the shape
    void decide_dwpw() {
        dw_of.assign(n_ops, -1);
        if (!opt.fuse_dwpw) return;
        for (int i = 0; i + 1 < n_ops; ++i) {
            const int32_t *o = op(i), *q = o + YK_OP_FIELDS;
            if (o[YK_F_TYPE] == YK_OP_DWCONV && q[YK_F_TYPE] == YK_OP_CONV && q[YK_F_K] == 1 &&
                q[YK_F_IN0] == o[YK_F_OUT] && p->T[o[YK_F_OUT]].uses == 1 && !(q[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT) &&
                p->T[o[YK_F_IN0]].kind == T_REAL && !p->T[o[YK_F_IN0]].is_input && o[YK_F_ACT] != YK_ACT_LEAKY &&
                yk_igemm_fused_ok(yk_pad8(o[YK_F_CIN]), q[YK_F_COUT])) {
                dw_of[i + 1] = i;
                skip[i] = 1;
            }
        }
    }

    // real tensors, minus those that live only in LDS / registers (a fused depthwise conv's, a folded Add's conv operand); the frame maxima
    int allocate() {
        int rc;
        for (int i = 1; i < (int)p->T.size(); ++i) {
            tinfo &t = p->T[i];
            if (t.kind != T_REAL) continue;
            bool fused_away = false;
            for (int k = 0; k < n_ops; ++k)
                if (op(k)[YK_F_OUT] == i && ((skip[k] && op(k)[YK_F_TYPE] == YK_OP_DWCONV) || add_of[k] >= 0)) fused_away = true;
            if (fused_away) continue;
            if (t.net_out) rc = p->mem.alloc((void **)&t.d32, (size_t)max_batch * t.h * t.w * t.c * sizeof(float));
            else rc = p->mem.alloc((void **)&t.d, ((size_t)max_batch * t.h * t.w * t.cp + 64) * sizeof(yk_half));
            if (rc) return rc;
        }
        return p->mem.alloc((void **)&p->d_imgmax, sizeof(unsigned) * max_batch * 32);   // YK_MAXP partials per image
    }

    void emit_u8max() {
        launch l;
        l.kind = K_U8MAX;   // only issued by yk_run_u8: Helper._process_img's np.max(img)
        l.name = "u8_max";
        l.bytes = (double)p->in_h * p->in_w * 3;
        p->L.push_back(l);
    }

    // the launch of op i, if it has one of its own; a conv that split K is followed by its finishing pass
    int emit(int i) {
        if (skip[i]) return YK_OK;
        const int32_t *o = op(i);
        const int ty = o[YK_F_TYPE];
        if (ty == YK_OP_UPSAMPLE || ty == YK_OP_CONCAT) return YK_OK;
        launch l;
        l.Ho = p->T[o[YK_F_OUT]].h;
        l.Wo = p->T[o[YK_F_OUT]].w;
        int rc;
        if (ty == YK_OP_CONV && p->T[o[YK_F_IN0]].is_input) rc = emit_stem(i, l);
        else if (ty == YK_OP_CONV) rc = emit_conv(i, l);
        else if (ty == YK_OP_DWCONV) rc = emit_dw(i, l);
        else if (ty == YK_OP_MAXPOOL) rc = emit_pool(i, l);
        else if (ty == YK_OP_ADD) rc = emit_add(i, l);
        else {
            yk_set_error("op %d: unknown op type %d", i, ty);
            rc = YK_ERR_UNSUPPORTED;
        }
        if (rc) return rc;
        p->L.push_back(l);
        if (l.kind == K_IGEMM && l.g.split_k > 1) emit_reduce(l);
        return YK_OK;
    }

    int emit_stem(int i, launch &l) {
        const int32_t *o = op(i);
        const tinfo &X = p->T[o[YK_F_IN0]], &Y = p->T[o[YK_F_OUT]];
        if (o[YK_F_K] != 3 || add_of[i] >= 0 || Y.net_out) {
            yk_set_error("op %d: stem conv must be 3x3", i);
            return YK_ERR_UNSUPPORTED;
        }
        const int co = o[YK_F_COUT];
        const float *w = blob + o[YK_F_W_OFF];
        l.kind = K_FIRST;
        first_args &f = l.f;
        memset(&f, 0, sizeof(f));
        int rc;
        const yk_wsrc wsrc{w, (size_t)27 * co * sizeof(float)};
        if ((rc = p->mem.packed(YK_WT_STEM, {co}, {wsrc}, [&](std::vector<uint8_t> &out, std::vector<float> &) { yk_wput(out, pack_stem(w, co)); }, &f.w))) return rc;
        f.Hi = X.h; f.Wi = X.w; f.Ho = Y.h; f.Wo = Y.w;
        f.stride = o[YK_F_STRIDE]; f.pad_t = o[YK_F_PAD_T]; f.pad_l = o[YK_F_PAD_L];
        f.Cout = co; f.outp = Y.cp;
        if (co <= 32 && (rc = p->mem.packed(YK_WT_STEM_MFMA, {co}, {wsrc}, [&](std::vector<uint8_t> &out, std::vector<float> &) { yk_wput(out, pack_stem_mfma(w, co)); }, &f.wm))) return rc;
        if ((rc = upload_scale_bias(o, co, &f.scale, &f.bias))) return rc;
        f.act = o[YK_F_ACT]; f.alpha = yk_op_alpha(o); f.out = Y.d;
        yk_act_params(f.act, f.alpha, &f.slope, &f.cap);
        if (Y.cp != co) {
            yk_set_error("op %d: stem conv Cout must be a multiple of 8", i);
            return YK_ERR_UNSUPPORTED;
        }
        char nm[96];
        snprintf(nm, sizeof nm, "stem3x3s%d_%d", f.stride, co);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * 27 * co;
        l.bytes = (double)X.h * X.w * 3 * 2 + (double)Y.h * Y.w * co * 2;
        return YK_OK;
    }

    // the depthwise conv `dwo` (input dwX, output X: never stored) computed by the fused kernel in front of its 1x1 GEMM
    int fuse_dw_into(igemm_args &g, const int32_t *dwo, const tinfo &dwX, const tinfo &X, double *flops, double *bytes) {
        const int c0 = X.c;
        int rc;
        if ((rc = upload_dw(blob + dwo[YK_F_W_OFF], c0, g.c0p, &g.dw_w))) return rc;
        if ((rc = upload_scale_bias(dwo, c0, &g.dw_scale, &g.dw_bias))) return rc;
        g.dw_act = dwo[YK_F_ACT]; g.dw_stride = dwo[YK_F_STRIDE];
        g.dw_pad_t = dwo[YK_F_PAD_T]; g.dw_pad_l = dwo[YK_F_PAD_L];
        g.dw_Hi = dwX.h; g.dw_Wi = dwX.w;
        yk_act_params(g.dw_act, 0.f, &g.dw_slope, &g.dw_cap);
        g.fd_g = yk_make_fastdiv((uint32_t)(g.c0p >> 3));
        *flops = 2.0 * X.h * X.w * 9 * c0;
        *bytes = ((double)dwX.h * dwX.w * c0 + (double)X.h * X.w * c0) * 2;
        return YK_OK;
    }

    // where conv op i stores: its own output, or - with a residual Add folded into it - the Add's output, g.res then reads the other addend
    tinfo *residual_dst(int i, igemm_args &g) {
        const int32_t *o = op(i);
        if (add_of[i] < 0) return &p->T[o[YK_F_OUT]];
        const int32_t *q = op(add_of[i]);
        const int other = (q[YK_F_IN0] == o[YK_F_OUT]) ? q[YK_F_IN1] : q[YK_F_IN0];
        g.res = p->T[other].d;
        g.resp = p->T[other].cp;
        return &p->T[q[YK_F_OUT]];
    }

    // tile configuration of conv launch l, fixed here for max_batch, and its weights in the one form that configuration reads: the panel
    // (fp16 [N][K]), or for the fused kernels that read their pointwise panel in MFMA fragment order, that order; K split and slab size
    // of a plain conv
    int plan_conv(launch &l, bool fused, const std::vector<int32_t> &wpar, const yk_wsrc &wsrc, const std::function<std::vector<uint16_t>()> &pack_panel) {
        igemm_args &g = l.g;
        g.M = max_batch * g.Ho * g.Wo;   // for config choice; patched per run
        l.cfg = fused ? yk_igemm_fused_pick(g) : yk_igemm_pick(g, l.out_f32);
        const bool frag = fused && (l.cfg == FUSED_DMA || l.cfg == LR_T1 || l.cfg == LR_T2);
        if (fused && l.cfg == FUSED_DMA) yk_fdma_fill(g);
        size_t bytes;
        int rc = p->mem.packed(frag ? YK_WT_FRAG : YK_WT_CONV, wpar, {wsrc}, [&](std::vector<uint8_t> &out, std::vector<float> &) {
            yk_wput(out, frag ? pack_fragments(pack_panel(), g.N, g.K) : pack_panel());
        }, &g.w, &bytes);
        if (rc) return rc;
        g.w_bytes = (uint32_t)bytes;
        if (!fused && opt.splitk) {
            g.split_k = yk_igemm_split(l.cfg, g);
            if (g.split_k > 1) {
                g.ldn = (g.N + 15) & ~15;
                p->slab_bytes = std::max(p->slab_bytes, (size_t)g.split_k * g.M * g.ldn * sizeof(float));
            }
        }
        return YK_OK;
    }

    // implicit GEMM conv (+ folded Add, + fused depthwise producer)
    int emit_conv(int i, launch &l) {
        const int32_t *o = op(i);
        const tinfo &X = p->T[o[YK_F_IN0]], &Y = p->T[o[YK_F_OUT]];
        l.kind = K_IGEMM;
        igemm_args &g = l.g;
        memset(&g, 0, sizeof(g));
        g.lda_pad = yk_fused_pad();
        const tinfo *s0 = &X, *s1 = nullptr;
        int up0 = 0, rc;
        if (X.kind == T_CAT) {
            s0 = &p->T[X.src0];
            s1 = &p->T[X.src1];
        }
        if (s0->kind == T_UP) {
            up0 = 1;
            s0 = &p->T[s0->src0];
        }
        const int32_t *dwo = dw_of[i] >= 0 ? op(dw_of[i]) : nullptr;
        const tinfo *dwX = dwo ? &p->T[dwo[YK_F_IN0]] : nullptr;
        if (dwo) s0 = dwX;
        if (s0->kind != T_REAL || (s1 && s1->kind != T_REAL) || s0->is_input || (s1 && s1->is_input) || !s0->d || (s1 && !s1->d)) {
            yk_set_error("op %d: unsupported input view nesting", i);
            return YK_ERR_UNSUPPORTED;
        }
        const int ks = o[YK_F_K], co = o[YK_F_COUT];
        const int c0 = dwo ? X.c : s0->c, c0p = yk_pad8(c0), c1 = s1 ? s1->c : 0, c1p = s1 ? s1->cp : 0;
        if (c0 + c1 != o[YK_F_CIN] || (ks != 1 && ks != 3)) {
            yk_set_error("op %d: conv shape mismatch (cin %d vs %d+%d, k=%d)", i, o[YK_F_CIN], c0, c1, ks);
            return YK_ERR_UNSUPPORTED;
        }
        g.in0 = s0->d; g.in1 = s1 ? s1->d : nullptr;
        g.c0p = c0p; g.c1p = c1p; g.up0 = up0;
        g.Hi = X.h; g.Wi = X.w; g.Ho = Y.h; g.Wo = Y.w;
        g.ks = ks; g.stride = o[YK_F_STRIDE]; g.pad_t = o[YK_F_PAD_T]; g.pad_l = o[YK_F_PAD_L];
        g.N = co; g.K = ks * ks * (c0p + c1p);
        const yk_wsrc wsrc{blob + o[YK_F_W_OFF], (size_t)co * ks * ks * (c0 + c1) * sizeof(float)};
        const auto pack_panel = [&] { return pack_conv(blob + o[YK_F_W_OFF], co, ks * ks, c0, c0p, c1, c1p); };
        const std::vector<int32_t> wpar{co, ks * ks, c0, c0p, c1, c1p};
        if ((rc = upload_scale_bias(o, co, &g.scale, &g.bias))) return rc;
        g.act = o[YK_F_ACT]; g.alpha = yk_op_alpha(o);
        yk_act_params(g.act, g.alpha, &g.slope, &g.cap);
        g.fd_hw = yk_make_fastdiv((uint32_t)(Y.h * Y.w));
        g.fd_wo = yk_make_fastdiv((uint32_t)Y.w);
        g.fd_ctp = yk_make_fastdiv((uint32_t)(c0p + c1p));
        g.split_k = 1;
        g.in0_bytes = (uint32_t)std::min<size_t>((size_t)max_batch * s0->h * s0->w * s0->cp * 2, 0xffffffffu);
        g.in1_bytes = s1 ? (uint32_t)std::min<size_t>((size_t)max_batch * s1->h * s1->w * s1->cp * 2, 0xffffffffu) : 0u;
        if (g.in0_bytes >= 0x40000000u || g.in1_bytes >= 0x40000000u) {
            yk_set_error("op %d: activation tensor >= 1 GiB; lower max_batch", i);
            return YK_ERR_UNSUPPORTED;
        }
        const tinfo *dst = residual_dst(i, g);
        const bool f32 = dst->net_out;
        g.out = f32 ? (void *)dst->d32 : (void *)dst->d;
        g.outp = f32 ? dst->c : dst->cp;
        g.fd_vpr = yk_make_fastdiv((uint32_t)std::max(1, g.outp >> 3));
        if (!g.out) {
            yk_set_error("op %d: output tensor not allocated", i);
            return YK_ERR_UNSUPPORTED;
        }
        double dw_flops = 0, dw_bytes = 0;
        if (dwo && (rc = fuse_dw_into(g, dwo, *dwX, X, &dw_flops, &dw_bytes))) return rc;
        l.out_f32 = f32;
        if ((rc = plan_conv(l, dwo != nullptr, wpar, wsrc, pack_panel))) return rc;
        char nm[96];
        snprintf(nm, sizeof nm, "%sconv%dx%ds%d_%dto%d%s%s[%s]", dwo ? "dw3x3+" : "", ks, ks, g.stride, o[YK_F_CIN], co,
                 g.res ? "+add" : "", s1 ? "+upcat" : (up0 ? "+up" : ""), dwo ? yk_igemm_fused_name(l.cfg) : yk_igemm_name(l.cfg));
        if (g.split_k > 1) snprintf(nm + strlen(nm), sizeof nm - strlen(nm), "/splitk%d", g.split_k);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * ks * ks * (double)o[YK_F_CIN] * co + dw_flops;
        l.bytes = ((double)X.h * X.w * o[YK_F_CIN] + (double)Y.h * Y.w * co) * 2 + dw_bytes;
        return YK_OK;
    }

    // deterministic finishing pass of the split-K conv launch c
    void emit_reduce(const launch &c) {
        launch r = c;
        r.kind = K_REDUCE;
        r.name = std::string("splitk_reduce") + std::to_string(c.g.split_k) + "_" + std::to_string(c.g.N);
        r.flops = 0;
        r.bytes = ((double)c.g.split_k * 4 + 2) * c.Ho * c.Wo * c.g.ldn;   // slabs read (fp32) + tile written (fp16)
        p->L.push_back(r);
    }

    int emit_dw(int i, launch &l) {
        const int32_t *o = op(i);
        const tinfo &X = p->T[o[YK_F_IN0]], &Y = p->T[o[YK_F_OUT]];
        if (X.kind != T_REAL || X.is_input) {
            yk_set_error("op %d: depthwise conv on a view/input", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = K_DW;
        dw_args &d = l.d;
        memset(&d, 0, sizeof(d));
        const int c = X.c, cp = X.cp;
        int rc;
        if ((rc = upload_dw(blob + o[YK_F_W_OFF], c, cp, &d.w))) return rc;
        d.in = X.d; d.Hi = X.h; d.Wi = X.w; d.Ho = Y.h; d.Wo = Y.w; d.Cp = cp;
        d.stride = o[YK_F_STRIDE]; d.pad_t = o[YK_F_PAD_T]; d.pad_l = o[YK_F_PAD_L];
        if ((rc = upload_scale_bias(o, c, &d.scale, &d.bias))) return rc;
        d.act = o[YK_F_ACT]; d.alpha = yk_op_alpha(o); d.out = Y.d;
        yk_act_params(d.act, d.alpha, &d.slope, &d.cap);
        char nm[96];
        snprintf(nm, sizeof nm, "dw3x3s%d_%d", d.stride, c);
        l.name = nm;
        l.flops = 2.0 * Y.h * Y.w * 9 * c;
        l.bytes = ((double)X.h * X.w * c + (double)Y.h * Y.w * c) * 2;
        return YK_OK;
    }

    int emit_pool(int i, launch &l) {
        const int32_t *o = op(i);
        const tinfo &X = p->T[o[YK_F_IN0]], &Y = p->T[o[YK_F_OUT]];
        if (X.kind != T_REAL || X.is_input) {
            yk_set_error("op %d: max pool on a view/input", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = K_POOL;
        pool_args &q = l.p;
        memset(&q, 0, sizeof(q));
        q.in = X.d; q.Hi = X.h; q.Wi = X.w; q.Ho = Y.h; q.Wo = Y.w; q.Cp = X.cp; q.stride = o[YK_F_STRIDE]; q.out = Y.d;
        char nm[96];
        snprintf(nm, sizeof nm, "maxpool2x2s%d_%d", q.stride, X.c);
        l.name = nm;
        l.bytes = ((double)X.h * X.w * X.c + (double)Y.h * Y.w * Y.c) * 2;
        return YK_OK;
    }

    int emit_add(int i, launch &l) {
        const int32_t *o = op(i);
        const tinfo &X = p->T[o[YK_F_IN0]], &Y = p->T[o[YK_F_OUT]], &Z = p->T[o[YK_F_IN1]];
        if (X.kind != T_REAL || Z.kind != T_REAL || !X.d || !Z.d || !Y.d) {
            yk_set_error("op %d: standalone Add on views", i);
            return YK_ERR_UNSUPPORTED;
        }
        l.kind = K_ADD;
        l.add_a = X.d; l.add_b = Z.d; l.add_o = Y.d;
        l.add_n8_per_image = (size_t)Y.h * Y.w * Y.cp / 8;
        char nm[96];
        snprintf(nm, sizeof nm, "add_%d", Y.c);
        l.name = nm;
        l.bytes = 3.0 * Y.h * Y.w * Y.c * 2;
        return YK_OK;
    }

    // split-K finishing pass followed by the 1x1 fp32 head conv that reads it -> one launch (reduce_pw_kernel)
    void merge_reduce_pw() {
        if (!opt.reduce_pw) return;
        for (size_t i = 0; i + 1 < p->L.size(); ++i) {
            launch &r = p->L[i];
            launch &c = p->L[i + 1];
            if (r.kind != K_REDUCE || r.out_f32 || c.kind != K_IGEMM) continue;
            igemm_args cg = c.g;
            cg.M = r.g.M;
            if (!yk_reduce_pw_ok(r.g, cg, c.out_f32)) continue;
            r.kind = K_REDUCE_PW;
            r.g2 = c.g;
            r.Ho2 = c.Ho; r.Wo2 = c.Wo;
            r.name += "+" + c.name.substr(0, c.name.find('['));
            r.flops += c.flops;
            r.bytes += c.bytes;
            p->L.erase(p->L.begin() + i + 1);
        }
    }

    // the split-K slabs; every network output is there; then waits for the uploads
    int finish() {
        int rc;
        if (p->slab_bytes && (rc = p->mem.alloc((void **)&p->d_slab, p->slab_bytes))) return rc;
        for (int t : p->outputs)
            if (!p->T[t].d32) {
                yk_set_error("yk_plan_create: output tensor %d is not produced by a NET_OUTPUT conv", t);
                return YK_ERR_UNSUPPORTED;
            }
        YK_HIP(hipDeviceSynchronize());
        return YK_OK;
    }
};

}   // namespace
