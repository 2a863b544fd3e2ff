// yk_engine.hip — plan compiler + executor behind yk_plan_create / yk_run_* / yk_get_output.
//
// A plan (k210_yolo_framework_amd/netspec.py) is compiled ONCE into a flat launch list:
//   * UpSampling2D / Concatenate never materialise: they become addressing modes of the consuming
//     conv's A-operand loader (yolonet.py:31-38 head pattern, Darknet FPN :167-172);
//   * Add (MobileNet-v2 / Darknet residual) is folded into the producing conv's epilogue;
//   * DepthwiseConv2D+BN+ReLU followed by its 1x1 Conv2D+BN+LeakyReLU is fused into one launch
//     where profitable (the depthwise tile lives only in LDS) — see YK_FUSE_DWPW;
//   * every weight tensor is converted to fp16 with its reduction axis padded to the activation
//     channel pitch, BatchNorm stays an fp32 (scale, bias) epilogue.
// The compiler itself - its passes and weight packers - is yk_plan_build.h; this file holds the plan, yk_plan_create_ex's pass list
// and the executor.  Running a plan replays the launch list on the caller's stream; nothing is allocated at run time.
#include <algorithm>
#include <string>
#include <vector>

#include "yk_conv.h"
#include "yk_plan_graph.h"

namespace {

enum { K_FIRST = 1, K_DW, K_IGEMM, K_POOL, K_ADD, K_U8MAX, K_REDUCE, K_REDUCE_PW };

struct tinfo : yk_gtens {
    yk_half *d = nullptr;
    float *d32 = nullptr;
};

struct launch {
    int kind = 0, cfg = 0;
    igemm_args g;
    igemm_args g2;              // K_REDUCE_PW: the 1x1 conv finished in the same launch
    int Ho2 = 0, Wo2 = 0;
    first_args f;
    dw_args d;
    pool_args p;
    const yk_half *add_a = nullptr, *add_b = nullptr;
    yk_half *add_o = nullptr;
    size_t add_n8_per_image = 0;
    int Ho = 0, Wo = 0;
    bool out_f32 = false;
    std::string name;
    double flops = 0, bytes = 0;
};

}   // namespace

struct yk_plan {
    int device = 0, max_batch = 0;
    std::vector<tinfo> T;
    std::vector<launch> L;
    yk_dev_mem mem;
    std::vector<int> outputs;
    unsigned *d_imgmax = nullptr;
    float *d_slab = nullptr;
    long long *d_dbg = nullptr;
    int dbg_launch = -1;
    size_t slab_bytes = 0;
    int in_h = 0, in_w = 0;
    int last_batch = 0;
    yk_xplan *x = nullptr;       // precision 1 ("f16x2"): the plan lives in yk_exact.hip, everything below forwards to it
};

#include "yk_plan_build.h"

// the device side of the weight store: plain device memory, written once before the entry is handed out
yk_wstore &yk_weights() {
    static const yk_wstore_dev dev = {
        nullptr,
        [](void *, int, const void *src, size_t bytes) -> void * {
            void *d = nullptr;
            hipError_t e = hipMalloc(&d, bytes ? bytes : 1);
            if (e == hipSuccess && bytes) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                yk_set_error("yk_plan_create: packed weights (%zu bytes): %s", bytes, hipGetErrorString(e));
                if (d) (void)hipFree(d);
                return nullptr;
            }
            return d;
        },
        [](void *, int, void *d) { (void)hipFree(d); }};
    static yk_wstore &store = *new yk_wstore(dev);      // never destroyed: a plan may be closed while the process exits
    return store;
}

extern "C" void yk_plan_destroy(yk_plan_t *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    p->mem.free_all();
    yk_xplan_destroy(p->x);
    delete p;
}

extern "C" int yk_plan_create(yk_plan_t **out, const int32_t *ops, int n_ops, const int32_t *tensors, int n_tensors,
                              const float *blob, size_t blob_len, const int32_t *outputs, int n_outputs, int max_batch,
                              int device) {
    return yk_plan_create_ex(out, ops, n_ops, tensors, n_tensors, blob, blob_len, outputs, n_outputs, max_batch, device, YK_PRECISION_F16X2);
}

extern "C" int yk_plan_create_ex(yk_plan_t **out, const int32_t *ops, int n_ops, const int32_t *tensors, int n_tensors,
                                 const float *blob, size_t blob_len, const int32_t *outputs, int n_outputs, int max_batch,
                                 int device, int precision) {
    if (!out || !ops || !tensors || !blob || !outputs || n_ops <= 0 || n_tensors <= 0 || max_batch <= 0) {
        yk_set_error("yk_plan_create: bad argument");
        return YK_ERR_ARG;
    }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yk_set_error("yk_plan_create: no HIP device visible (this library has no CPU path)");
        return YK_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        yk_set_error("yk_plan_create: device %d out of range (%d visible)", device, ndev);
        return YK_ERR_NO_DEVICE;
    }
    YK_HIP(hipSetDevice(device));
    yk_plan *p = new yk_plan();
    p->device = device;
    p->max_batch = max_batch;
    const int schedule = precision & YK_SCHEDULE_MASK;
    precision &= ~YK_SCHEDULE_MASK;
    int rc = plan_read_tensors(p, tensors, n_tensors, outputs, n_outputs);
    if (!rc && precision == YK_PRECISION_F16X2) {
        rc = yk_xplan_create(&p->x, ops, n_ops, tensors, n_tensors, blob, blob_len, outputs, n_outputs, max_batch, schedule == YK_SCHEDULE_LATENCY);
    } else if (!rc && precision != YK_PRECISION_F16) {
        yk_set_error("yk_plan_create_ex: unknown precision %d", precision);
        rc = YK_ERR_ARG;
    } else if (!rc) {                                        // f16: the passes of yk_plan_build.h
        builder b{p, ops, n_ops, blob, max_batch, read_plan_opts()};
        rc = b.analyse(blob_len);
        if (!rc) {
            b.decide_dwpw();
            rc = b.allocate();
        }
        if (!rc) b.emit_u8max();
        for (int i = 0; i < n_ops && !rc; ++i) rc = b.emit(i);
        if (!rc) {
            b.merge_reduce_pw();
            rc = b.finish();
        }
    }
    if (rc) {
        yk_plan_destroy(p);
        return rc;
    }
    *out = p;
    return YK_OK;
}

static int run_plan(yk_plan *p, const void *d_in, int in_f32, int batch, void *stream, hipEvent_t *ev = nullptr) {
    if (!p || !d_in || batch <= 0 || batch > p->max_batch) {
        yk_set_error("yk_run: bad plan/input/batch (max_batch=%d)", p ? p->max_batch : 0);
        return YK_ERR_ARG;
    }
    YK_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (p->x) {
        p->last_batch = batch;
        return yk_xplan_run(p->x, d_in, in_f32, batch, st, ev);
    }
    int li = 0;
    for (launch &l : p->L) {
        int rc = YK_OK;
        if (ev) YK_HIP(hipEventRecord(ev[2 * li], st));
        switch (l.kind) {
        case K_U8MAX:
            if (!in_f32) {
                rc = yk_launch_u8_max((const uint8_t *)d_in, (size_t)p->in_h * p->in_w * 3, batch, p->d_imgmax, st);
            }
            break;
        case K_FIRST: {
            first_args f = l.f;
            f.in = d_in; f.in_f32 = in_f32; f.img_max = p->d_imgmax; f.B = batch;
            rc = yk_launch_first(f, st);
        } break;
        case K_IGEMM: {
            igemm_args g = l.g;
            g.M = batch * l.Ho * l.Wo;
            g.slab = p->d_slab;
            g.dbg = (li == p->dbg_launch) ? p->d_dbg : nullptr;
            rc = g.dw_w ? yk_launch_igemm_fused(l.cfg, g, st) : yk_launch_igemm(l.cfg, g, st);
        } break;
        case K_REDUCE: {
            igemm_args g = l.g;
            g.M = batch * l.Ho * l.Wo;
            g.slab = p->d_slab;
            rc = yk_launch_splitk_reduce(g, l.out_f32, st);
        } break;
        case K_REDUCE_PW: {
            igemm_args g = l.g, g2 = l.g2;
            g.M = batch * l.Ho * l.Wo;
            g.slab = p->d_slab;
            g2.M = batch * l.Ho2 * l.Wo2;
            rc = yk_launch_reduce_pw(g, g2, st);
        } break;
        case K_DW: {
            dw_args d = l.d;
            d.B = batch;
            rc = yk_launch_dw(d, st);
        } break;
        case K_POOL: {
            pool_args q = l.p;
            q.B = batch;
            rc = yk_launch_pool(q, st);
        } break;
        case K_ADD: rc = yk_launch_add(l.add_a, l.add_b, l.add_o, l.add_n8_per_image * batch, st); break;
        }
        if (rc) return rc;
        if (ev) YK_HIP(hipEventRecord(ev[2 * li + 1], st));
        ++li;
    }
    YK_HIP(hipGetLastError());
    p->last_batch = batch;
    return YK_OK;
}

// Per-launch timing with HIP events recorded on the SAME stream the kernels run on.
// ms_out[i] = median duration of launch i over `iters` replays (i < yk_plan_launch_count).
extern "C" int yk_plan_profile(yk_plan_t *p, const uint8_t *d_frames, int batch, int iters, void *stream, float *ms_out) {
    if (!p || !ms_out || iters <= 0) {
        yk_set_error("yk_plan_profile: bad argument");
        return YK_ERR_ARG;
    }
    const int n = yk_plan_launch_count(p);
    std::vector<hipEvent_t> ev(2 * n);
    for (auto &e : ev) YK_HIP(hipEventCreate(&e));
    std::vector<std::vector<float>> samples(n);
    int rc = YK_OK;
    for (int it = -3; it < iters && rc == YK_OK; ++it) {                  // three untimed replays first (clocks, caches, allocator)
        rc = run_plan(p, d_frames, 0, batch, stream, ev.data());
        if (rc) break;
        YK_HIP(hipStreamSynchronize((hipStream_t)stream));
        if (it < 0) continue;
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            YK_HIP(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            samples[i].push_back(ms);
        }
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    for (int i = 0; i < n; ++i) {                                         // median over the replays: one slow replay (a clock dip, another
        std::vector<float> &v = samples[i];                               // process' burst) must not define a launch's duration
        std::sort(v.begin(), v.end());
        ms_out[i] = v.empty() ? 0.f : (v.size() & 1 ? v[v.size() / 2] : 0.5f * (v[v.size() / 2 - 1] + v[v.size() / 2]));
    }
    return rc;
}

extern "C" int yk_run_u8(yk_plan_t *p, const uint8_t *d_frames, int batch, void *stream) {
    return run_plan(p, d_frames, 0, batch, stream);
}
extern "C" int yk_run_f32(yk_plan_t *p, const float *d_input, int batch, void *stream) {
    return run_plan(p, d_input, 1, batch, stream);
}

extern "C" int yk_get_output(yk_plan_t *p, int idx, float **d_ptr, size_t *bytes, int *h, int *w, int *c) {
    if (!p || idx < 0 || idx >= (int)p->outputs.size()) {
        yk_set_error("yk_get_output: bad index");
        return YK_ERR_ARG;
    }
    if (p->x) return yk_xplan_output(p->x, idx, d_ptr, bytes, h, w, c);
    const tinfo &t = p->T[p->outputs[idx]];
    if (d_ptr) *d_ptr = t.d32;
    if (bytes) *bytes = (size_t)p->max_batch * t.h * t.w * t.c * sizeof(float);
    if (h) *h = t.h;
    if (w) *w = t.w;
    if (c) *c = t.c;
    return YK_OK;
}

extern "C" int yk_debug_read_tensor(yk_plan_t *p, int tid, int batch, float *h_dst, size_t dst_elems) {
    if (!p || tid <= 0 || tid >= (int)p->T.size() || batch <= 0 || batch > p->max_batch || !h_dst) {
        yk_set_error("yk_debug_read_tensor: bad argument");
        return YK_ERR_ARG;
    }
    if (p->x) {
        YK_HIP(hipSetDevice(p->device));
        return yk_xplan_read_tensor(p->x, tid, batch, h_dst, dst_elems);
    }
    const tinfo &t = p->T[tid];
    const size_t n = (size_t)batch * t.h * t.w * t.c;
    if (dst_elems < n) {
        yk_set_error("yk_debug_read_tensor: destination too small");
        return YK_ERR_ARG;
    }
    YK_HIP(hipSetDevice(p->device));
    YK_HIP(hipDeviceSynchronize());
    if (t.d32) {
        YK_HIP(hipMemcpy(h_dst, t.d32, n * sizeof(float), hipMemcpyDeviceToHost));
        return YK_OK;
    }
    if (!t.d) {
        yk_set_error("yk_debug_read_tensor: tensor %d is a view or was fused away", tid);
        return YK_ERR_UNSUPPORTED;
    }
    std::vector<uint16_t> h((size_t)batch * t.h * t.w * t.cp);
    YK_HIP(hipMemcpy(h.data(), t.d, h.size() * 2, hipMemcpyDeviceToHost));
    const size_t pix = (size_t)batch * t.h * t.w;
    for (size_t q = 0; q < pix; ++q)
        for (int c = 0; c < t.c; ++c) h_dst[q * t.c + c] = yk_h2f(h[q * t.cp + c]);
    return YK_OK;
}

extern "C" int yk_debug_read_exponents(yk_plan_t *p, int tid, int batch, int32_t *h_e) {
    if (!p || tid <= 0 || tid >= (int)p->T.size() || batch <= 0 || batch > p->max_batch || !h_e) {
        yk_set_error("yk_debug_read_exponents: bad argument");
        return YK_ERR_ARG;
    }
    if (!p->x) {
        yk_set_error("yk_debug_read_exponents: an f16 plan stores no exponents");
        return YK_ERR_UNSUPPORTED;
    }
    YK_HIP(hipSetDevice(p->device));
    return yk_xplan_read_exponents(p->x, tid, batch, h_e);
}

// dev instrumentation: arm phase timestamps for launch `li`, run once (u8 path), copy out [n_wg][8] ticks (100 MHz)
extern "C" int yk_debug_phase_stamps(yk_plan_t *p, int li, const uint8_t *d_frames, int batch, void *stream,
                                     long long *h_out, int max_wg) {
    if (p && p->x) {       // f16x2 plan: [n_wg][16] stamps of a fused block launch
        YK_HIP(hipSetDevice(p->device));
        return yk_xplan_phase_stamps(p->x, li, d_frames, batch, (hipStream_t)stream, h_out, max_wg);
    }
    if (!p || li < 0 || li >= (int)p->L.size()) return YK_ERR_ARG;
    YK_HIP(hipSetDevice(p->device));
    if (!p->d_dbg) {
        int rc = p->mem.alloc((void **)&p->d_dbg, sizeof(long long) * 8 * 65536);
        if (rc) return rc;
    }
    YK_HIP(hipMemset(p->d_dbg, 0, sizeof(long long) * 8 * 65536));
    p->dbg_launch = li;
    int rc = run_plan(p, d_frames, 0, batch, stream);
    p->dbg_launch = -1;
    if (rc) return rc;
    YK_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (max_wg > 65536) max_wg = 65536;
    YK_HIP(hipMemcpy(h_out, p->d_dbg, sizeof(long long) * 8 * max_wg, hipMemcpyDeviceToHost));
    return YK_OK;
}

// Waits for the device and reports a sticky device-side failure of an earlier run of this plan (today: the persistent late-backbone
// stage of the f16x2 mode could not assemble a workgroup cluster; see yk_xpersist.h).  YK_OK otherwise.
extern "C" int yk_plan_check(yk_plan_t *p) {
    if (!p) {
        yk_set_error("yk_plan_check: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipSetDevice(p->device));
    if (p->x) return yk_xplan_check(p->x);
    YK_HIP(hipDeviceSynchronize());
    return YK_OK;
}

// The same word WITHOUT waiting for the device: nonzero = a run that has already finished failed on the device (today: a cluster launch
// of the f16x2 latency schedule could not assemble a cluster).  The caller has synchronised with the runs it asks about (an event, a
// stream); `clear` resets the word after reading it.  Costs a host memory read: the word lives in mapped host memory.
extern "C" int yk_plan_peek_error(yk_plan_t *p, int clear, unsigned *error_out) {
    if (!p || !error_out) {
        yk_set_error("yk_plan_peek_error: bad argument");
        return YK_ERR_ARG;
    }
    *error_out = p->x ? yk_xplan_peek_error(p->x, clear) : 0u;
    return YK_OK;
}

// test hook: stores `value` into the error word the way a timed-out cluster barrier does
extern "C" int yk_plan_debug_set_error(yk_plan_t *p, unsigned value) {
    if (!p || !p->x) {
        yk_set_error("yk_plan_debug_set_error: needs an f16x2 plan");
        return YK_ERR_ARG;
    }
    yk_xplan_debug_set_error(p->x, value);
    return YK_OK;
}

extern "C" int yk_plan_launch_count(const yk_plan_t *p) { return !p ? 0 : (p->x ? yk_xplan_launch_count(p->x) : (int)p->L.size()); }

extern "C" int yk_plan_launch_info(const yk_plan_t *p, int i, char *name, size_t name_len, double *flops_per_image,
                                   double *bytes_per_image) {
    if (p && p->x) {
        const char *nm = "";
        double fl = 0, by = 0;
        int rc = yk_xplan_launch_info(p->x, i, &nm, &fl, &by);
        if (rc) return rc;
        if (name && name_len) snprintf(name, name_len, "%s", nm);
        if (flops_per_image) *flops_per_image = fl;
        if (bytes_per_image) *bytes_per_image = by;
        return YK_OK;
    }
    if (!p || i < 0 || i >= (int)p->L.size()) return YK_ERR_ARG;
    if (name && name_len) snprintf(name, name_len, "%s", p->L[i].name.c_str());
    if (flops_per_image) *flops_per_image = p->L[i].flops;
    if (bytes_per_image) *bytes_per_image = p->L[i].bytes;
    return YK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// A step as ONE hipGraph.  Everything issued on `stream` between yk_graph_begin and yk_graph_end (yk_run_*, yk_decode_py*,
// yk_letterbox_u8, yk_memcpy_async ...) is recorded instead of executed; yk_graph_launch replays it with one host call
// (the eager step is ~30 launches at 3-4 us of host time each: SURVEY 7 step 8).  The capture is thread-local: other host threads
// (an input pipeline's producer) may keep allocating and copying on their own streams meanwhile.  A replay uses the pointers and
// sizes of the capture: the step must have run once eagerly on the same stream before (the decode scratch is allocated on first use
// and is keyed by stream), the buffers it names must stay alive, and the plan must not be replayed on two streams at once.
// ---------------------------------------------------------------------------------------------------------------------
struct yk_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    size_t nodes = 0, kernels = 0;
};

extern "C" int yk_graph_begin(void *stream) {
    if (!stream) {
        yk_set_error("yk_graph_begin: the default stream cannot be captured; pass a created stream");
        return YK_ERR_ARG;
    }
    YK_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    return YK_OK;
}

extern "C" int yk_graph_end(void *stream, yk_graph_t **out) {
    if (!out) {
        yk_set_error("yk_graph_end: bad argument");
        return YK_ERR_ARG;
    }
    *out = nullptr;
    hipGraph_t g = nullptr;
    YK_HIP(hipStreamEndCapture((hipStream_t)stream, &g));
    if (!g) {
        yk_set_error("yk_graph_end: the capture was invalidated (a call that cannot be captured ran on the stream)");
        return YK_ERR_HIP;
    }
    yk_graph *r = new yk_graph();
    r->graph = g;
    hipError_t e = hipGraphInstantiate(&r->exec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        yk_set_error("yk_graph_end: hipGraphInstantiate -> %s", hipGetErrorString(e));
        (void)hipGraphDestroy(g);
        delete r;
        return YK_ERR_HIP;
    }
    if (hipGraphGetNodes(g, nullptr, &r->nodes) == hipSuccess && r->nodes) {
        std::vector<hipGraphNode_t> nd(r->nodes);
        size_t n = r->nodes;
        if (hipGraphGetNodes(g, nd.data(), &n) == hipSuccess)
            for (size_t i = 0; i < n; ++i) {
                hipGraphNodeType ty;
                if (hipGraphNodeGetType(nd[i], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel) ++r->kernels;
            }
    }
    *out = r;
    return YK_OK;
}

extern "C" int yk_graph_launch(yk_graph_t *g, void *stream) {
    if (!g || !g->exec) {
        yk_set_error("yk_graph_launch: bad graph");
        return YK_ERR_ARG;
    }
    YK_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return YK_OK;
}

extern "C" int yk_graph_node_count(const yk_graph_t *g) { return g ? (int)g->nodes : 0; }
extern "C" int yk_graph_kernel_node_count(const yk_graph_t *g) { return g ? (int)g->kernels : 0; }

extern "C" void yk_graph_destroy(yk_graph_t *g) {
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

extern "C" int yk_memcpy_async(void *dst, const void *src, size_t bytes, void *stream) {
    if (!dst || !src) {
        yk_set_error("yk_memcpy_async: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
    return YK_OK;
}

// device address of pinned host memory (hipHostMalloc / hipHostRegister'ed): what a kernel must be given to write detections
// straight into host memory (yk_decode_py_packed)
extern "C" int yk_host_device_ptr(void *h_ptr, void **d_ptr) {
    if (!h_ptr || !d_ptr) {
        yk_set_error("yk_host_device_ptr: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipHostGetDevicePointer(d_ptr, h_ptr, 0));
    return YK_OK;
}

// library-owned streams (see include/yolo_hip.h): created back to back they land on consecutive hardware queues
extern "C" int yk_stream_create(void **stream_out, int priority) {
    if (!stream_out) {
        yk_set_error("yk_stream_create: bad argument");
        return YK_ERR_ARG;
    }
    hipStream_t s = nullptr;
    YK_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
    *stream_out = (void *)s;
    return YK_OK;
}
extern "C" int yk_stream_destroy(void *stream) {
    if (!stream) return YK_OK;
    YK_HIP(hipStreamSynchronize((hipStream_t)stream));
    yk_scratch_release_stream(stream);
    YK_HIP(hipStreamDestroy((hipStream_t)stream));
    return YK_OK;
}
extern "C" int yk_stream_query_priority(void *stream, int *priority_out) {
    if (!priority_out) {
        yk_set_error("yk_stream_query_priority: bad argument");
        return YK_ERR_ARG;
    }
    YK_HIP(hipStreamGetPriority((hipStream_t)stream, priority_out));
    return YK_OK;
}
