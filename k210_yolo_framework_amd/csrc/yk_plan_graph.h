// yk_plan_graph.h — what both plan builders start from (host only): the f16 one (yk_plan_build.h) and the f16x2 one
// (yk_xplan_build.h).  The host plumbing - fp32 <-> fp16 conversion, a plan's device allocations - and the op-graph analysis: tensor
// table, op validation, use counts, UpSampling2D / Concatenate views, network-output flags and the residual Adds that fold into their
// producing conv.
#pragma once
#include <algorithm>
#include <vector>

#include "yk_conv.h"
#include "yk_wstore.h"

static inline uint16_t yk_f2h(float f) {   // round-to-nearest-even fp32 -> fp16 bits (normal / subnormal / overflow to inf)
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static inline float yk_h2f(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}

static inline float yk_op_alpha(const int32_t *o) {   // an op row's LeakyReLU slope: a float stored in an int32 field
    float a;
    memcpy(&a, &o[YK_F_ALPHA], 4);
    return a;
}

// The library's store of packed immutable buffers (yk_wstore.h; defined once, in yk_engine.hip).  The tag names the packer, so two
// packers never share an entry; each packer lists the parameters its layout depends on beside it.
yk_wstore &yk_weights();
enum yk_wtag {
    YK_WT_F32 = 1,                                                   // upload_f
    YK_WT_STEM, YK_WT_STEM_MFMA, YK_WT_CONV, YK_WT_FRAG, YK_WT_DW,   // yk_plan_build.h
    YK_WT_XW, YK_WT_XDW, YK_WT_XSTEM, YK_WT_XSTEM_FRAG,              // yk_xplan_build.h
};
template <class E>
static inline void yk_wput(std::vector<uint8_t> &packed, const std::vector<E> &v) {
    packed.resize(v.size() * sizeof(E));
    if (!v.empty()) memcpy(packed.data(), v.data(), packed.size());
}

// the device allocations of a plan, freed together by its destroy function: what a step writes is the plan's own (alloc, upload), the
// packed weights and parameter tables no kernel writes are references into the store (packed)
struct yk_dev_mem {
    std::vector<void *> ptrs;
    std::vector<yk_went *> refs;
    bool share = yk_env_flag("YK_SHARE_WEIGHTS", true);   // read where the plan is created; 0: every packed buffer is the plan's own

    int alloc(void **ptr, size_t bytes, bool zero = true) {
        YK_HIP(hipMalloc(ptr, bytes));
        ptrs.push_back(*ptr);
        if (zero) YK_HIP(hipMemset(*ptr, 0, bytes));
        return YK_OK;
    }
    int upload(void **ptr, const void *src, size_t bytes) {
        int rc = alloc(ptr, bytes, false);
        if (rc) return rc;
        YK_HIP(hipMemcpy(*ptr, src, bytes, hipMemcpyHostToDevice));
        return YK_OK;
    }
    // A packed immutable buffer, to the pointer type its kernel reads it through: `pack` turns the source ranges `src` into the packed
    // bytes and the host-side floats derived with them (`aux`); `par` lists every parameter of the packer that the result depends on.
    // Shared: the store's entry for (device, tag, par, src) - packed and uploaded only if it is not there yet.
    template <class D>
    int packed(int tag, const std::vector<int32_t> &par, const std::vector<yk_wsrc> &src, const yk_wpack_fn &pack, const D **d,
               size_t *bytes = nullptr, std::vector<float> *aux = nullptr) {
        if (!share) {
            std::vector<uint8_t> host;
            std::vector<float> a;
            pack(host, a);
            void *q;
            int rc = upload(&q, host.data(), host.size());
            if (rc) return rc;
            *d = (const D *)q;
            if (bytes) *bytes = host.size();
            if (aux) *aux = a;
            return YK_OK;
        }
        yk_went *e = yk_weights().acquire(yk_current_device(), tag, par.data(), (int)par.size(), src.data(), (int)src.size(), pack);
        if (!e) return YK_ERR_HIP;                             // (the error text is set where the upload failed)
        refs.push_back(e);
        *d = (const D *)e->d;
        if (bytes) *bytes = e->bytes;
        if (aux) *aux = e->aux;
        return YK_OK;
    }
    // n floats times `mul` (BatchNorm scale / bias), padded with 256 zeros so an epilogue may read past n unguarded
    int upload_f(const float *src, int n, const float **d, float mul = 1.f) {
        int32_t mul_bits;
        memcpy(&mul_bits, &mul, 4);
        return packed(YK_WT_F32, {n, mul_bits}, {{src, (size_t)n * sizeof(float)}}, [&](std::vector<uint8_t> &out, std::vector<float> &) {
            std::vector<float> v((size_t)n + 256, 0.f);
            for (int i = 0; i < n; ++i) v[i] = src[i] * mul;
            yk_wput(out, v);
        }, d);
    }
    void free_all() {
        for (void *q : ptrs) (void)hipFree(q);
        ptrs.clear();
        for (yk_went *e : refs) yk_weights().release(e);
        refs.clear();
    }
};

enum { T_REAL = 0, T_UP = 1, T_CAT = 2 };

// what the analysis knows of a tensor; each plan's tensor struct derives from it and adds its device pointers
struct yk_gtens {
    int h = 0, w = 0, c = 0, cp = 0;
    int kind = T_REAL, src0 = -1, src1 = -1;
    bool net_out = false, is_input = false;
    int uses = 0;
};

template <class TENS>
static void yk_graph_tensors(std::vector<TENS> &T, const int32_t *tensors, int n_tensors) {
    T.resize(n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        TENS &t = T[i];
        t.h = tensors[4 * i];
        t.w = tensors[4 * i + 1];
        t.c = tensors[4 * i + 2];
        t.cp = yk_pad8(t.c);
        t.is_input = tensors[4 * i + 3] != 0;
    }
}

// views, use counts (the network outputs count as a use), output flags; then add_of[i] = index of the Add folded into conv op i's
// epilogue and skip[that Add] = 1.  YK_ERR_ARG (with the error text set) for a bad tensor id or a weight offset outside the blob.
template <class TENS>
static int yk_graph_analyse(std::vector<TENS> &T, const int32_t *ops, int n_ops, size_t blob_len, const std::vector<int> &outputs,
                            std::vector<int> &add_of, std::vector<char> &skip) {
    const int n_tensors = (int)T.size();
    for (int i = 0; i < n_ops; ++i) {
        const int32_t *o = ops + (size_t)i * YK_OP_FIELDS;
        const int ty = o[YK_F_TYPE], in0 = o[YK_F_IN0], in1 = o[YK_F_IN1], ot = o[YK_F_OUT];
        if (in0 < 0 || in0 >= n_tensors || ot <= 0 || ot >= n_tensors || in1 >= n_tensors) {
            yk_set_error("yk_plan_create: op %d has a bad tensor id", i);
            return YK_ERR_ARG;
        }
        T[in0].uses++;
        if (in1 >= 0) T[in1].uses++;
        if (ty == YK_OP_UPSAMPLE) {
            T[ot].kind = T_UP;
            T[ot].src0 = in0;
        } else if (ty == YK_OP_CONCAT) {
            T[ot].kind = T_CAT;
            T[ot].src0 = in0;
            T[ot].src1 = in1;
        }
        if ((ty == YK_OP_CONV) && (o[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT)) T[ot].net_out = true;
        if ((ty == YK_OP_CONV || ty == YK_OP_DWCONV) &&
            ((size_t)std::max(o[YK_F_W_OFF], std::max(o[YK_F_SCALE_OFF], o[YK_F_BIAS_OFF])) >= blob_len ||
             o[YK_F_W_OFF] < 0)) {
            yk_set_error("yk_plan_create: op %d weight offset outside the blob", i);
            return YK_ERR_ARG;
        }
    }
    for (int t : outputs) T[t].uses++;
    add_of.assign(n_ops, -1);
    skip.assign(n_ops, 0);
    for (int i = 0; i + 1 < n_ops; ++i) {      // residual Add folded into the producing conv's epilogue
        const int32_t *o = ops + (size_t)i * YK_OP_FIELDS, *q = o + YK_OP_FIELDS;
        if (o[YK_F_TYPE] == YK_OP_CONV && q[YK_F_TYPE] == YK_OP_ADD && !(o[YK_F_FLAGS] & YK_FLAG_NET_OUTPUT)) {
            const int y = o[YK_F_OUT];
            const int other = (q[YK_F_IN0] == y) ? q[YK_F_IN1] : (q[YK_F_IN1] == y ? q[YK_F_IN0] : -1);
            if (other >= 0 && other != y && T[y].uses == 1 && T[other].kind == T_REAL && !T[other].is_input) {
                add_of[i] = i + 1;
                skip[i + 1] = 1;
            }
        }
    }
    return YK_OK;
}
