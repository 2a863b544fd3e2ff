/* yolo_hip.h — C-ABI of libyolo_hip.so, the MI355X (gfx950) replacement for the
 * conv-backbone + region-layer hot path of zhen8838/K210_Yolo_framework.
 *
 * Two groups of entry points:
 *
 *  (1) region_layer_*  — byte-for-byte drop-in for the reference's only native
 *      operator, yolo3_frame_test_public/region_layer.h:7-48.  Same four
 *      symbols, same struct layouts, same call order and error codes, so a
 *      main.c-style caller (main.c:278-324) links against this library
 *      unchanged.  The arithmetic runs on the GPU; rl->output / boxes / probs
 *      are mirrored back to the host buffers the reference exposes.
 *
 *  (2) yk_*            — the batched engine.  The reference has no batched
 *      native API, so these mirror the call shape its edge path already uses
 *      for the model run (kendryte SDK, un-vendored):
 *        kpu_load_kmodel(&task, blob)                 main.c:274  -> yk_plan_create
 *        kpu_run_kmodel(&task, img, dma, done_cb, 0)  main.c:303  -> yk_run_u8 / yk_run_f32 (async on a stream)
 *        kpu_get_output(&task, i, &ptr, &bytes)       main.c:310  -> yk_get_output
 *      and, for the Python path, the decode + per-class NMS block of
 *      keras_inference.py:94-135 (tf_xywh_to_all tools/utils.py:524-547,
 *      correct_box keras_inference.py:32-72)            -> yk_decode_py
 *      plus a batched form of region_layer_run           -> yk_region_batched
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success and a negative code on failure (region_layer_init keeps the
 * reference's -1..-4); pointers named d_* are DEVICE pointers, h_* host.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).
 * No entry point falls back to a CPU implementation: without a usable HIP
 * device they fail with YK_ERR_NO_DEVICE.
 */
#ifndef YOLO_HIP_H_
#define YOLO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* (1) drop-in region layer — layouts from region_layer.h:7-42                */
/* ------------------------------------------------------------------------- */
typedef struct {
    uint32_t obj_number;
    struct {
        uint32_t x1;
        uint32_t y1;
        uint32_t x2;
        uint32_t y2;
        uint32_t class_id;
        float prob;
    } obj[10];
} obj_info_t;

typedef struct {
    float threshold;          /* caller sets before init (main.c:280) */
    float nms_value;          /* caller sets before init (main.c:281) */
    uint32_t coords;
    uint32_t anchor_number;   /* caller sets before init (main.c:278) */
    float *anchor;            /* borrowed, 2*anchor_number floats (w,h) */
    uint32_t image_width;
    uint32_t image_height;
    uint32_t classes;
    uint32_t net_width;
    uint32_t net_height;
    uint32_t layer_width;
    uint32_t layer_height;
    uint32_t boxes_number;
    uint32_t output_number;
    void *boxes;              /* boxes_number x {x,y,w,h} float, callee-owned */
    float *input;             /* borrowed CHW fp32 [A*(5+C), H, W], set before run (main.c:313) */
    float *output;            /* callee-owned, output_number floats */
    float *probs_buf;         /* callee-owned, boxes_number*(classes+1) floats */
    float **probs;            /* callee-owned row pointers into probs_buf */
} region_layer_t;

typedef void (*callback_draw_box)(uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2,
                                  uint32_t class_id, float prob);

/* region_layer.h:44-45 / region_layer.c:19-66.  0 ok; -1..-4 = which host buffer
 * failed to allocate (as the reference); -5 = device state could not be created. */
int region_layer_init(region_layer_t *rl, int width, int height, int channels, int origin_width,
                      int origin_height);
/* region_layer.h:46 / region_layer.c:68-73 */
void region_layer_deinit(region_layer_t *rl);
/* region_layer.h:47 / region_layer.c:378-383.  obj_info may be NULL (main.c:314);
 * like the reference (call commented out at region_layer.c:382) it is not written. */
void region_layer_run(region_layer_t *rl, obj_info_t *obj_info);
/* region_layer.h:48 / region_layer.c:385-404.  Negative float -> uint32 is UB in the
 * reference; here it is defined as (uint32_t)(int64_t)x, the x86-64 behaviour. */
void region_layer_draw_boxes(region_layer_t *rl, callback_draw_box callback);

/* ------------------------------------------------------------------------- */
/* (2) batched engine                                                         */
/* ------------------------------------------------------------------------- */
#define YK_OK 0
#define YK_ERR_ARG (-10)
#define YK_ERR_HIP (-11)
#define YK_ERR_UNSUPPORTED (-12)
#define YK_ERR_NO_DEVICE (-13)
#define YK_ERR_NOMEM (-14)

/* op codes / activation codes / field indices of one op row (int32 x YK_OP_FIELDS);
 * produced by k210_yolo_framework_amd/netspec.py:compile_plan */
enum { YK_OP_CONV = 1, YK_OP_DWCONV = 2, YK_OP_MAXPOOL = 3, YK_OP_UPSAMPLE = 4, YK_OP_CONCAT = 5, YK_OP_ADD = 6 };
enum { YK_ACT_NONE = 0, YK_ACT_RELU = 1, YK_ACT_RELU6 = 2, YK_ACT_LEAKY = 3 };
enum {
    YK_F_TYPE = 0, YK_F_IN0, YK_F_IN1, YK_F_OUT, YK_F_CIN, YK_F_COUT, YK_F_K, YK_F_STRIDE, YK_F_PAD_T,
    YK_F_PAD_L, YK_F_ACT, YK_F_ALPHA /* float bits */, YK_F_W_OFF, YK_F_SCALE_OFF, YK_F_BIAS_OFF, YK_F_FLAGS,
    YK_F_IN_H, YK_F_IN_W, YK_F_OUT_H, YK_F_OUT_W
};
#define YK_OP_FIELDS 24
#define YK_FLAG_NET_OUTPUT 1
#define YK_MAX_LAYERS 4
#define YK_MAX_ANCHORS 8

typedef struct yk_plan yk_plan_t; /* opaque */

/* Last error text of the calling thread ("" if none). */
const char *yk_last_error(void);
/* Number of visible HIP devices (0 when there is none / no driver). */
int yk_device_count(void);

/* kpu_load_kmodel analogue.  ops: [n_ops][YK_OP_FIELDS] int32; tensors: [n_tensors][4]
 * int32 (h, w, c, is_input); blob: fp32 weights/scale/bias addressed by the op rows.
 * The plan owns every device buffer (weights, activation arena sized for max_batch).
 * Arithmetic: YK_PRECISION_F16X2 below - the mode whose outputs stay within 1e-3 of the fp32 Keras path with identical
 * class / box indices (what `yolo_model.predict`, keras_inference.py:88, returns); fp32 network outputs. */
int yk_plan_create(yk_plan_t **out, const int32_t *ops, int n_ops, const int32_t *tensors, int n_tensors,
                   const float *blob, size_t blob_len, const int32_t *outputs, int n_outputs, int max_batch,
                   int device);
/* The same with a choice of arithmetic (there is no reference counterpart: Keras computes in fp32 on the CPU):
 *   YK_PRECISION_F16X2  (= yk_plan_create) activations in HBM as fp16 PAIRS, x * 2^-e = hi + lo (22 significant bits, the bytes of
 *                       fp32, per-image storage exponent e), weights split the same way once; three fp16 MFMAs per product
 *                       (w_lo*x_hi + w_hi*x_lo + w_hi*x_hi), fp32 accumulate: fp32-class results (the "within 1e-3, indices
 *                       exact" clause of the north star; measured 2e-6 of max|logit|).  Per-image operand scaling: results
 *                       never depend on the batch mates.
 *   YK_PRECISION_F16    fp16 activations in HBM, one fp16 MFMA per product, fp32 accumulate: about twice as fast, and outside
 *                       the tolerance (scores drift ~2e-4 mean / 2e-3..5e-3 max from the fp32 Keras path). */
#define YK_PRECISION_F16 0
#define YK_PRECISION_F16X2 1
/* OR-ed into `precision` (f16x2 only; ignored by f16): how the late backbone and the detection heads are launched.
 *   YK_SCHEDULE_THROUGHPUT (default)  one launch per layer: kernels of several batches in flight on several streams overlap best
 *                                      (bench.py `value`: four batches in flight);
 *   YK_SCHEDULE_LATENCY               two launches of per-image workgroup clusters (csrc/yk_xpersist.h, csrc/yk_xheads.h): every CU
 *                                      is held for their duration, the time of ONE batch is shortest (669 -> 542 us of kernels at 32 images).
 * Same arithmetic; results differ at the 2^-22 rounding level (summation order).  YK_PERSIST / YK_HEADS = 0|1 in the environment override. */
#define YK_SCHEDULE_THROUGHPUT 0x000
#define YK_SCHEDULE_LATENCY 0x100
#define YK_SCHEDULE_MASK 0xf00
int yk_plan_create_ex(yk_plan_t **out, const int32_t *ops, int n_ops, const int32_t *tensors, int n_tensors,
                      const float *blob, size_t blob_len, const int32_t *outputs, int n_outputs, int max_batch,
                      int device, int precision);
void yk_plan_destroy(yk_plan_t *p);

/* kpu_run_kmodel analogue, asynchronous on `stream`.
 * yk_run_u8: d_frames = device uint8 [batch][H][W][3]; fuses Helper._process_img's
 *            `img / np.max(img)` (tools/utils.py:405) as a per-image max reduction.
 * yk_run_f32: d_input = device float [batch][H][W][3], already normalised (what
 *            yolo_model.predict receives, keras_inference.py:88). */
int yk_run_u8(yk_plan_t *p, const uint8_t *d_frames, int batch, void *stream);
int yk_run_f32(yk_plan_t *p, const float *d_input, int batch, void *stream);

/* kpu_get_output analogue: borrowed device pointer to network output idx,
 * NHWC fp32 [max_batch][h][w][A*(5+C)] (rows beyond the last run's batch are stale). */
int yk_get_output(yk_plan_t *p, int idx, float **d_ptr, size_t *bytes, int *h, int *w, int *c);

/* Synchronises the device and returns an error if an earlier asynchronous run of this plan failed ON the device (the f16x2 mode's
 * persistent stage bounds every inter-workgroup wait and gives up rather than hang: then this call says so).  YK_OK otherwise. */
int yk_plan_check(yk_plan_t *p);
/* The same sticky word without waiting for the device (a read of mapped host memory): *error_out != 0 means a run that has already
 * FINISHED failed on the device; the caller has synchronised with the runs it asks about (event / stream).  clear != 0 resets it. */
int yk_plan_peek_error(yk_plan_t *plan, int clear, unsigned *error_out);
int yk_plan_debug_set_error(yk_plan_t *plan, unsigned value); /* test hook: what a failing cluster launch stores */

/* Debug/parity access to any intermediate activation (fp16, channel pitch padded
 * to a multiple of 8): copies tensor `tid` of the last run to host as fp32 NHWC. */
int yk_debug_read_tensor(yk_plan_t *p, int tid, int batch, float *h_dst, size_t dst_elems);
/* The per-image storage exponents of tensor `tid` in an f16x2 plan after the last run: the stored halves hold x * 2^-h_e[b] = hi + lo
 * (fp32-plane tensors: 0).  YK_ERR_UNSUPPORTED for an f16 plan and for a tensor that is not stored split (a view, folded or fused
 * away, an fp32 network output).  Debug / parity access only: synchronises the device. */
int yk_debug_read_exponents(yk_plan_t *p, int tid, int batch, int32_t *h_e);
/* Number of kernel launches one yk_run_* issues (after fusion). */
int yk_plan_launch_count(const yk_plan_t *p);
/* Name/shape of the i-th launch for bench/roofline bookkeeping. */
int yk_plan_launch_info(const yk_plan_t *p, int i, char *name, size_t name_len, double *flops_per_image,
                        double *bytes_per_image);

/* Per-launch timing: replays the plan `iters` times with HIP events recorded on `stream` around every
 * launch; ms_out[i] (i < yk_plan_launch_count) = median duration of launch i over the replays, in milliseconds. */
int yk_plan_profile(yk_plan_t *p, const uint8_t *d_frames, int batch, int iters, void *stream, float *ms_out);

/* ---- decode ---------------------------------------------------------------- */
typedef struct {
    int32_t n_layers;                       /* output scales (2 or 3) */
    int32_t anchor_num;                     /* A */
    int32_t class_num;                      /* C */
    int32_t in_h, in_w;                     /* network input size (224, 320) */
    int32_t out_h[YK_MAX_LAYERS];           /* Helper.out_hw */
    int32_t out_w[YK_MAX_LAYERS];
    float anchors[YK_MAX_LAYERS][YK_MAX_ANCHORS][2]; /* Helper.anchors (w,h), image-relative */
} yk_decode_cfg_t;

/* Python-mode decode + per-class NMS for a batch (keras_inference.py:94-135).
 * d_pred[l]: device fp32 [batch][out_h][out_w][A][5+C] (== the engine's outputs).
 * d_image_hw: device float [batch][2] original image (h,w) per image, or NULL = in_hw.
 * d_dets:   device float [batch][C*max_out][6] rows (top,left,bottom,right,score,class),
 *           class-major ascending, score-descending within a class (the reference's order).
 * d_counts: device int32 [batch].
 * Semantics restated from tensorflow 1.14 tf.image.non_max_suppression: score >= obj_thresh
 * kept, greedy, suppress iff IoU > iou_thresh, at most max_out (30) per class; equal scores
 * are ordered by ascending box index (TF leaves it unspecified). */
int yk_decode_py(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                 float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts, void *stream);
/* The same, also returning which box each row is: d_box_index [batch][C*max_out] int32 (may be NULL), the row's index into the
 * reference's flattened (layer, h, w, anchor) box list (keras_inference.py:107-114: `tf.reshape(..., (-1, 4))` per layer, concatenated) -
 * what `tf.boolean_mask` + `tf.image.non_max_suppression` + `tf.gather` select (:116-131). */
int yk_decode_py_ex(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                    float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts, int32_t *d_box_index,
                    void *stream);

/* The same selection, concatenated ACROSS the batch as well (keras_inference.py:133-135 concatenates per image): rows of image b
 * are rows[offsets[b] .. offsets[b+1]) (6 floats each, same order as d_dets), offsets[batch] = total.  `rows` (capacity
 * batch*C*max_out rows), `offsets` [batch+1] and `rows_index` (may be NULL; the box index of every row) may be device memory or
 * pinned, device-mapped HOST memory (hipHostMalloc): then the detections reach the host at their live size, with no device-to-host
 * copy whose size would have to be known first.  d_dets / d_counts (device, may be NULL) additionally receive the padded form. */
int yk_decode_py_packed(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                        float obj_thresh, float iou_thresh, int max_out, float *rows, int32_t *offsets, int32_t *rows_index,
                        float *d_dets, int32_t *d_counts, void *stream);

/* The suppression rule of the decode tail.  YK_NMS_HARD is the rule above.  The other three run Soft-NMS (Bodla et al. 2017) and
 * DIoU-NMS (Zheng et al. 2020) as k210_yolo_framework_amd/softnms.py states them: per class, the live candidate with the largest CURRENT
 * score (ties: lowest box index) is emitted with that score, then every live candidate's score is multiplied by
 *   LINEAR    1 - IoU if IoU > iou_thresh, else 1
 *   GAUSSIAN  expf(-(IoU * IoU) / nms_sigma), for every IoU
 *   DIOU      0 if IoU - d2 / c2 > iou_thresh, else 1   (d2: squared centre distance, c2: squared diagonal of the enclosing box)
 * and a candidate whose score falls below obj_thresh (or whose weight is 0) is retired.  Rows of a class are in emission order and carry
 * the decayed score. */
#define YK_NMS_HARD 0
#define YK_NMS_LINEAR 1
#define YK_NMS_GAUSSIAN 2
#define YK_NMS_DIOU 3
/* yk_decode_py_ex / yk_decode_py_packed with the rule chosen: YK_NMS_HARD runs exactly what those two run.  nms_sigma is read by
 * YK_NMS_GAUSSIAN only.  An unknown nms_method, or an nms_sigma that is not positive and finite with YK_NMS_GAUSSIAN: YK_ERR_ARG with the
 * argument named in yk_last_error, nothing launched. */
int yk_decode_py_nms(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                     float obj_thresh, float iou_thresh, int max_out, float *d_dets, int32_t *d_counts, int32_t *d_box_index,
                     void *stream, int nms_method, float nms_sigma);
int yk_decode_py_packed_nms(const yk_decode_cfg_t *cfg, const float *const *d_pred, int batch, const float *d_image_hw,
                            float obj_thresh, float iou_thresh, int max_out, float *rows, int32_t *offsets, int32_t *rows_index,
                            float *d_dets, int32_t *d_counts, void *stream, int nms_method, float nms_sigma);

/* ---- sliced inference: the rows of the tile frames of a picture merged into one row set (k210_yolo_framework_amd/tiles.py states the
 * rule).  d_dets [n_tiles][class_num*max_out][6] and d_counts [n_tiles] as yk_decode_py* leaves them (counts are clamped to
 * [0, class_num*max_out]); d_origin [n_tiles][2] float (y0, x0) of each tile in its picture; d_first [n_pics + 1] int32: the tiles of
 * picture p are d_first[p] .. d_first[p+1] - 1 (contiguous; their number may differ between pictures; a value outside [0, n_tiles] is
 * clamped, a descending pair is an empty picture).  Candidates of a picture: every row of its tiles, tile by tile, in row order, translated by
 * ONE float add per coordinate (top, bottom += y0; left, right += x0).  A row whose class is not exactly one of 0 .. class_num - 1, or whose
 * score is not above -inf, is dropped.  Per (picture, class) a greedy hard NMS: the live candidate with the largest score (ties: the lowest
 * candidate index) is kept, every live candidate whose match with it is > thresh is retired, at most max_out kept.
 *   YK_MATCH_IOU  the IoU of yk_decode_py's own NMS        YK_MATCH_IOS  the same intersection / the smaller area (not positive: no match)
 * d_out [n_pics][class_num*max_out][6] (class-major ascending, score-descending within a class) and d_out_counts [n_pics]: the padded form
 * again, so yk_draw_dets_u8, yk_map_append_padded and the copies downstream take it unchanged; rows past the count are not written.
 * One wavefront per (picture, class); a class's candidates are staged in LDS when at most yk_merge_tiles_lds_candidates(...) of them exist
 * and are walked in global memory (per-stream scratch: 8 bytes per input row) otherwise - no bound on tiles * max_out other than memory and
 * n_tiles * class_num * max_out < 2^31.  Two launches and one 4-byte-per-picture fill on `stream`; can be recorded in a graph once the
 * stream's scratch has been sized by an eager call of the same size.  The tiles of different pictures must not overlap.  A NULL pointer,
 * n_tiles <= 0, n_pics <= 0, class_num <= 0, max_out <= 0, a thresh that is NaN, an unknown metric, or 2^31 or more input or output rows:
 * YK_ERR_ARG with the argument named in yk_last_error, nothing launched. */
#define YK_MATCH_IOU 0
#define YK_MATCH_IOS 1
int yk_merge_tiles(const float *d_dets, const int32_t *d_counts, const float *d_origin, const int32_t *d_first, int n_tiles, int n_pics,
                   int class_num, int max_out, float thresh, int metric, float *d_out, int32_t *d_out_counts, void *stream);
/* Candidates of one (picture, class) that yk_merge_tiles with these sizes stages in LDS on the current device; more take the global path. */
int yk_merge_tiles_lds_candidates(int n_tiles, int n_pics, int max_out);

/* ---- test-time augmentation: the rows of the view frames of a picture fused into one row set (k210_yolo_framework_amd/tta.py states the
 * rule, Weighted Boxes Fusion).  d_dets [n_pics * views][class_num*max_out][6] and d_counts [n_pics * views] as yk_decode_py*
 * leaves them (counts are clamped to [0, class_num*max_out]); the frames of picture p are p*views .. (p+1)*views - 1 and N = views.
 * d_xform [n_pics * views][3] float (dy, dx, mw) per frame: a row is mapped back by left' = mw - right, right' = mw - left when mw >= 0, then
 * top, bottom += dy and left, right += dx, one float operation each.  Candidates of a picture: every row of its frames, frame by frame, in
 * row order, mapped back.  A row whose class is not exactly one of 0 .. class_num - 1, or whose score is not above 0 (a NaN included), is
 * dropped.  Per (picture, class) the candidates are walked by score descending (ties: the lowest candidate index) against the clusters made so
 * far, in creation order: the cluster whose current fused box has the largest IoU with the candidate (the IoU of yk_decode_py's own NMS; ties:
 * the lowest cluster index) takes it when that IoU is > thresh, otherwise the candidate opens a cluster.  A cluster accumulates, in join
 * order, sw += s and (st, sl, sb, sr) += s * (top, left, bottom, right); its box is its member's verbatim while it has one and
 * (st, sl, sb, sr) / sw afterwards; its score is ((sw / cnt) * min(cnt, N)) / N.  Every step one float operation, no contraction.
 * d_out [n_pics][class_num*max_out][6] (class-major ascending; within a class by final score descending, ties to the older cluster, at most
 * max_out) and d_out_counts [n_pics]: the decode's padded form, so yk_draw_dets_u8, yk_map_append_padded and the copies downstream take it
 * unchanged; rows past the count are not written.  One wavefront per (picture, class), candidates and clusters in LDS, no atomics: two calls
 * give the same bytes.  There is one path: views * max_out must not exceed yk_fuse_views_lds_candidates(max_out), and more is refused, never
 * truncated.  (That bound is the decode's: a frame holds at most max_out rows of a class.  Frames that are not decode-shaped may hold more; of a
 * class's candidates only the first views * max_out in candidate order are then read.)  Two launches on `stream`; can be recorded in a graph once the stream's scratch has been sized by an eager call of the same
 * size.  A NULL pointer, views <= 0 or > 8, n_pics <= 0, class_num <= 0, max_out <= 0, a thresh that is NaN or negative, 2^31 or more input
 * rows, or views * max_out above the capacity: YK_ERR_ARG with the argument named in yk_last_error, nothing launched. */
#define YK_TTA_MAX_VIEWS 8
int yk_fuse_views(const float *d_dets, const int32_t *d_counts, const float *d_xform, int views, int n_pics, int class_num, int max_out,
                  float thresh, float *d_out, int32_t *d_out_counts, void *stream);
/* Candidates of one (picture, class), views * max_out, that yk_fuse_views holds in LDS on the current device (68 bytes each); max_out <= 0:
 * YK_ERR_ARG, no device: YK_ERR_NO_DEVICE. */
int yk_fuse_views_lds_candidates(int max_out);

/* ---- a step as one hipGraph (the kpu_run_kmodel(..., dma, ai_done_cb) shape of main.c:303-311: submit once, get called back) ----
 * Everything issued on `stream` (a created stream, not NULL) between yk_graph_begin and yk_graph_end - yk_run_*, yk_decode_py*,
 * yk_letterbox_u8, yk_memcpy_async - is recorded, not executed; yk_graph_launch replays the recording with ONE host call.
 * Rules: run the step once eagerly on the same stream first (scratch is allocated on first use, per stream); the replay uses the
 * pointers, batch and thresholds of the capture; keep the named buffers alive; one replay of a plan at a time.  The capture is
 * thread-local (other host threads may use HIP meanwhile). */
typedef struct yk_graph yk_graph_t; /* opaque */
int yk_graph_begin(void *stream);
int yk_graph_end(void *stream, yk_graph_t **out);
int yk_graph_launch(yk_graph_t *g, void *stream);
int yk_graph_node_count(const yk_graph_t *g);          /* nodes of the recording */
int yk_graph_kernel_node_count(const yk_graph_t *g);   /* ... of which kernels (the rest: copies / fills) */
void yk_graph_destroy(yk_graph_t *g);
/* hipMemcpyAsync(hipMemcpyDefault) on `stream`: the host<->device legs of a captured step (pinned host memory). */
int yk_memcpy_async(void *dst, const void *src, size_t bytes, void *stream);
/* Device address of pinned host memory (hipHostGetDevicePointer): the form of a host buffer a kernel can write. */
int yk_host_device_ptr(void *h_ptr, void **d_ptr);
/* A HIP stream created by the library itself (hipStreamCreateWithPriority, non-blocking; priority 0 = default, negative = higher):
 * the ROCm runtime binds a stream to one of its GPU_MAX_HW_QUEUES hardware queues in creation order, so a pipeline that creates its
 * own streams back to back gets distinct queues whatever pooled streams the host framework handed out before.
 * yk_stream_query_priority returns the priority the runtime reports for any stream handle. */
int yk_stream_create(void **stream_out, int priority);
int yk_stream_destroy(void *stream);
int yk_stream_query_priority(void *stream, int *priority_out);
/* The library keeps per-stream scratch buffers (decode / NMS work space) that grow on demand.  A captured step holds their addresses:
 * yk_scratch_generation(stream) counts how often a buffer of `stream` (on the current device) has MOVED; the holder of captured graphs
 * compares it before a replay and re-captures when it changed (engine.Pipeline does). */
unsigned long long yk_scratch_generation(void *stream);

/* C-mode (region_layer.c:121-283) for a batch of layer outputs without host round trips.
 * d_input element (b, anchor n, entry e, row y, col x) is at
 *   b*stride_b + n*stride_n + e*stride_e + y*stride_y + x*stride_x   (floats)
 * so both the K210 CHW layout and the engine's NHWC outputs can be consumed.
 * d_boxes: [batch][A*H*W][4] (x,y,w,h), d_probs: [batch][A*H*W][C+1]; box index = n*H*W + y*W + x. */
typedef struct {
    int32_t layer_w, layer_h, anchor_num, classes;
    int32_t net_w, net_h, image_w, image_h;
    float threshold, nms_value;
    float anchor[2 * YK_MAX_ANCHORS];
    int64_t stride_b, stride_n, stride_e, stride_y, stride_x;
} yk_region_cfg_t;
int yk_region_batched(const yk_region_cfg_t *cfg, const float *d_input, int batch, float *d_output /* may be NULL */,
                      float *d_boxes, float *d_probs, void *stream);

/* ---- pre-processing (the step immediately before the path) ------------------------------
 * Helper._process_img letterbox (tools/utils.py:378-399) for a batch of equally sized u8 frames:
 * d_src [batch][src_h][src_w][3] -> d_dst [batch][dst_h][dst_w][3], bilinear, zero fill, truncating cast.
 * (The `img / np.max(img)` that follows, utils.py:405, is fused into yk_run_u8.) */
int yk_letterbox_u8(const uint8_t *d_src, int batch, int src_h, int src_w, uint8_t *d_dst, int dst_h, int dst_w,
                    void *stream);
/* The same letterbox, then the training augmentation (the imgaug OneOf of tools/utils.py:84-88; semantics in
 * k210_yolo_framework_amd/augment.py) in one launch for a batch of equally sized u8 frames.  d_inv: device float64 [batch][6],
 * each image's inverse map M (row-major 2x3, pixel-index coordinates of the dst_h x dst_w tensor, src_idx = M . (x, y, 1)), built on
 * the host.  The letterboxed image is warped bilinearly through M (taps outside the tensor read 0, round half up, capped at 255);
 * no intermediate frame is written, and the result is bit-identical to yk_letterbox_u8 followed by that warp.  Integer M (identity,
 * mirror) gives an exact pixel copy.  Any finite M is safe: the taps are tested as doubles before any conversion.  A map with an entry that
 * is not finite yields an unspecified but deterministic frame and reads nothing of d_src.  Bad arguments, a NULL d_inv included:
 * YK_ERR_ARG.  Can be recorded in a graph. */
int yk_letterbox_augment_u8(const uint8_t *d_src, int batch, int src_h, int src_w, const double *d_inv /* [batch][6] */,
                            uint8_t *d_dst, int dst_h, int dst_w, void *stream);
/* `img / np.max(img)` (tools/utils.py:405) for a batch of u8 frames of per_image bytes each -> fp32 (one correctly rounded quotient
 * per element, numpy's float64 division then the pipeline's float32 cast).  Used by the training input pipeline (N3); the inference
 * path fuses the normalisation into the stem conv (yk_run_u8). */
int yk_normalise_u8(const uint8_t *d_frames, int batch, size_t per_image, float *d_out, void *stream);

/* ---- pictures of different sizes in one buffer (`make detect`) ------------------------------
 * A ragged batch is one packed device buffer of `n` pictures, picture i = [h][w][3] u8 at byte `offset` (any value: pixels are 3 bytes,
 * no alignment is assumed; gaps between pictures are allowed), and a device table of one row per picture. */
typedef struct yk_ragged_row {
    uint64_t offset;    /* byte offset of the picture in the packed buffer */
    int32_t h, w;       /* its size */
    double scale;       /* letterbox of this picture into dst_h x dst_w: yk_letterbox_ragged_params fills these three */
    int32_t tx, ty;
    int32_t thickness;  /* yk_draw_dets_u8: rings of box outline, and the integer magnification of the glyphs (values < 1 draw as 1, mag > 1024 as 1024) */
    int32_t mag;
} yk_ragged_row_t;      /* 40 bytes, no padding */
/* HOST helper: fills scale, tx, ty of n rows in host memory with the arithmetic yk_letterbox_u8 uses for (h, w) -> (dst_h, dst_w).
 * A row with h <= 0 or w <= 0, a NULL table, n <= 0 or a non-positive dst size: YK_ERR_ARG.  Needs no device. */
int yk_letterbox_ragged_params(yk_ragged_row_t *h_table, int n, int dst_h, int dst_w);
/* One launch for the whole ragged batch: d_dst [n][dst_h][dst_w][3]; image i of the result equals yk_letterbox_u8 on picture i alone,
 * bit for bit (the same per-pixel arithmetic with the row's scale, tx, ty).  d_table is DEVICE memory, so this call cannot read it:
 * NULL pointers, n <= 0, src_bytes == 0 and non-positive dst sizes are YK_ERR_ARG here, while refusing a row whose h or w is not positive,
 * or whose picture does not lie inside the buffer, is the caller's job (engine.letterbox_ragged_u8 does it on the host table).
 * The kernel does not trust the table either: the image of a row with h <= 0, w <= 0 or offset + 3*h*w > src_bytes is written as
 * zeros and nothing of d_src is read for it.  Can be recorded in a graph. */
int yk_letterbox_ragged_u8(const uint8_t *d_src, size_t src_bytes, const yk_ragged_row_t *d_table, int n, uint8_t *d_dst, int dst_h,
                           int dst_w, void *stream);
/* ---- sliced inference: tiles of the pictures of a ragged batch as frames (k210_yolo_framework_amd/tiles.py) ------
 * A tile is a sub-rectangle of a packed picture: h rows of w pixels, the first at byte `offset` of the packed buffer, consecutive rows
 * `stride` bytes apart (3 * the parent picture's width; stride == 3*w is a whole picture). */
typedef struct yk_tile_row {
    uint64_t offset;    /* byte offset of the tile's first pixel in the packed buffer */
    int32_t h, w;       /* the tile's size */
    int64_t stride;     /* bytes per row of the parent picture */
    double scale;       /* letterbox of this tile into dst_h x dst_w: yk_letterbox_tiles_params fills these three */
    int32_t tx, ty;
} yk_tile_row_t;        /* 40 bytes, no padding */
/* HOST helper: fills scale, tx, ty of n rows in host memory with the arithmetic yk_letterbox_ragged_params uses for (h, w) -> (dst_h, dst_w).
 * A row with h <= 0 or w <= 0, a NULL table, n <= 0 or a non-positive dst size: YK_ERR_ARG.  Needs no device. */
int yk_letterbox_tiles_params(yk_tile_row_t *h_table, int n, int dst_h, int dst_w);
/* One launch for all tiles (one thread per output pixel): d_dst [n][dst_h][dst_w][3]; frame t equals yk_letterbox_u8 on a contiguous copy of
 * tile t alone, bit for bit - the same per-pixel arithmetic, and a tap outside the TILE reads 0, not the parent's neighbouring pixel.
 * d_table is DEVICE memory: NULL pointers, n <= 0, src_bytes == 0 and non-positive dst sizes are YK_ERR_ARG here, refusing bad rows is the
 * caller's job (engine.letterbox_tiles_u8 does it on the host table).  The kernel does not trust the table either: the frame of a row
 * with h <= 0, w <= 0, stride < 3*w or offset + (h-1)*stride + 3*w > src_bytes is written as zeros and nothing of d_src is read for it.
 * Can be recorded in a graph. */
int yk_letterbox_tiles_u8(const uint8_t *d_src, size_t src_bytes, const yk_tile_row_t *d_table, int n, uint8_t *d_dst, int dst_h,
                          int dst_w, void *stream);
/* ---- test-time augmentation: views of the pictures of a ragged batch as frames (k210_yolo_framework_amd/tta.py) ------
 * A view is a zero canvas of ch x cw pixels with the h x w picture at byte `offset` of the packed buffer pasted at row oy, column ox,
 * left-right mirrored when `mirror` is not 0.  The canvas is never built: its pixels are read out of the picture in place. */
typedef struct yk_view_row {
    uint64_t offset;    /* byte offset of the picture in the packed buffer */
    int32_t h, w;       /* the picture's size */
    int32_t ch, cw;     /* the canvas */
    int32_t oy, ox;     /* where the picture sits in it */
    int32_t mirror;     /* not 0: canvas pixel (y, x) inside the picture is picture pixel (y - oy, w - 1 - (x - ox)) */
    int32_t reserved;   /* 0 */
    double scale;       /* letterbox of the canvas into dst_h x dst_w: yk_letterbox_views_params fills these three */
    int32_t tx, ty;
} yk_view_row_t;        /* 56 bytes, no padding */
/* HOST helper: fills scale, tx, ty of n rows in host memory with the arithmetic yk_letterbox_ragged_params uses for (ch, cw) -> (dst_h, dst_w).
 * A row with ch <= 0 or cw <= 0, a NULL table, n <= 0 or a non-positive dst size: YK_ERR_ARG.  Needs no device. */
int yk_letterbox_views_params(yk_view_row_t *h_table, int n, int dst_h, int dst_w);
/* One launch for all views (one thread per output pixel): d_dst [n][dst_h][dst_w][3]; frame v equals yk_letterbox_u8 of the canvas of view v,
 * bit for bit - the same per-pixel arithmetic; a tap outside the pasted picture reads 0, a tap inside reads picture pixel (y - oy, x - ox),
 * or (y - oy, w - 1 - (x - ox)) when mirrored.  d_table is DEVICE memory: NULL pointers, n <= 0, src_bytes == 0 and non-positive dst sizes are
 * YK_ERR_ARG here, refusing bad rows is the caller's job (engine.letterbox_views_u8 does it on the host table).  The kernel does not trust the
 * table either: the frame of a row with h <= 0, w <= 0, a picture that is not inside its canvas (oy < 0, oy + h > ch, ox < 0, ox + w > cw) or
 * offset + 3*h*w > src_bytes is written as zeros and nothing of d_src is read for it.  Can be recorded in a graph. */
int yk_letterbox_views_u8(const uint8_t *d_src, size_t src_bytes, const yk_view_row_t *d_table, int n, uint8_t *d_dst, int dst_h,
                          int dst_w, void *stream);
/* ---- mosaic: one training frame from four pictures (k210_yolo_framework_amd/mosaic.py) ------
 * A sample is four table rows in quadrant order - 0 top left [0,cx) x [0,cy), 1 top right [cx,W) x [0,cy), 2 bottom left, 3 bottom right -
 * and a seam (cx, cy).  Output pixel (x, y) is the letterbox pixel (yk_letterbox_u8's arithmetic, unchanged: truncating cast, taps outside
 * the picture read 0) of the picture of the quadrant it falls in, with that row's scale, tx, ty; tx and ty may be negative.  Four equal rows
 * holding a picture's plain letterbox give yk_letterbox_u8's frame, bit for bit, wherever the seam is.
 * HOST helper: fills scale, tx, ty of the four rows of one sample from their (h, w), the seam and the gains: scale = gain_k * (the letterbox
 * scale of (h, w) -> (dst_h, dst_w)); left quadrants tx = cx - (int)ceil(w * scale), right quadrants tx = cx; top quadrants
 * ty = cy - (int)ceil(h * scale), bottom quadrants ty = cy - the corner of the scaled picture nearest the seam sits at the seam.  A NULL
 * pointer, a row with h <= 0 or w <= 0, a gain that is not positive and finite, or a non-positive dst size: YK_ERR_ARG.  Needs no device. */
int yk_mosaic_params(yk_ragged_row_t *h_rows4, int cx, int cy, const double *gain4, int dst_h, int dst_w);
/* One launch for the whole batch (blockIdx.y is the sample, chunked at 65535; one thread per output pixel): d_table [n][4] rows (quadrant
 * order), d_centre [n][2] = (cx, cy), d_inv [n][6] float64 or NULL (no warp), d_dst [n][dst_h][dst_w][3].  With d_inv the frame is warped
 * by each sample's inverse map as yk_letterbox_augment_u8 warps the letterbox: the four bilinear taps each evaluate the mosaic pixel on the
 * fly, no intermediate frame, bit-identical to the mosaic followed by that warp.  The kernel does not trust the table: a row with h <= 0,
 * w <= 0 or offset + 3*h*w > src_bytes makes its quadrant zeros and nothing of d_src is read for it; cx and cy are clamped to [0, dst_w] and
 * [0, dst_h] (an empty quadrant is legal).  A d_inv row with an entry that is not finite yields an unspecified but deterministic frame and
 * reads nothing of d_src.  NULL pointers other than d_inv, n <= 0, src_bytes == 0 and non-positive dst sizes: YK_ERR_ARG; no device:
 * YK_ERR_NO_DEVICE.  Can be recorded in a graph (one kernel node per 65535 samples). */
int yk_mosaic_ragged_u8(const uint8_t *d_src, size_t src_bytes, const yk_ragged_row_t *d_table, const int32_t *d_centre,
                        const double *d_inv, int n, uint8_t *d_dst, int dst_h, int dst_w, void *stream);
/* ---- HSV colour jitter of finished training frames (k210_yolo_framework_amd/colour.py) ------
 * In place on d_frames [n][h][w][3] u8: frame i gets the hue rotation dh (turns of the hue circle), the saturation gain gs and the exposure
 * gain gv of d_params [n][3] float64 = (dh, gs, gv), in Smith's hexcone HSV, float64, the operations of colour.jitter_u8 in its order - the
 * bytes are that function's, bit for bit.  One thread per pixel, which reads and writes only its own three bytes; one launch (one kernel
 * node in a graph) up to 2^30 pixels, more are chunked; the pixel index is a size_t, n is not limited by a grid dimension.  The kernel does
 * not trust the table: a row with a dh, gs or gv that is not finite, or with a negative gain, leaves its frame untouched; (0, 1, 1) changes
 * no byte.  n == 0: YK_OK, nothing launched.  A NULL pointer with n > 0, n < 0, h <= 0, w <= 0 or 3*n*h*w beyond size_t: YK_ERR_ARG;
 * no device: YK_ERR_NO_DEVICE.  Can be recorded in a graph. */
int yk_hsv_jitter_u8(uint8_t *d_frames, int n, int h, int w, const double *d_params, void *stream);
/* ---- training labels from boxes (Helper.batch_box_to_label, k210_yolo_framework_amd/helper.py) ------
 * The dense label grids of a batch, built on the device from its boxes: d_boxes [n_boxes][5] float64 rows (cls, x, y, w, h) relative to the
 * network frame, sample i owning rows d_first[i] .. d_first[i + 1] - 1 (d_first [n + 1] int32).  d_labels is ONE flat fp32 buffer: layer 0's
 * [n][out_h][out_w][A][5 + class_num], then layer 1's, and so on; every element of it is written (a buffer full of anything comes out
 * defined).  The rule is Helper.batch_box_to_label's, in float64, numpy's operation order, contraction off:
 *   fit[k][l][a] = o / (w h + aw ah - o),  o = max(min(w, aw), 0) max(min(h, ah), 0)                        (Helper._fake_iou)
 *   primary slot of box k: the first argmax of fit[k] over the flattened (l, a); YK_ASSIGN_MULTI: secondary slots, every other (l, a) with
 *   fit[k][l][a] > assign_iou; the cell of a slot in layer l is (floor(x out_w[l]), floor(y out_h[l]));
 *   a slot's first five entries are (float)clip(x y w h, 1e-8, 1) and 1 of the candidate with the largest key is_primary * n_boxes + k among
 *   those written there - the last primary box, else the last secondary box - and entry 5 + cls is 1 for every candidate written there.
 * Bit-identical to the host statement for every box whose cells lie inside the grids of all the layers it is written to.  Where numpy raises
 * (index out_w) or wraps (negative index) the kernel writes NOTHING of that box, in any layer, and records the smallest such row index of
 * d_boxes in *d_status with an integer atomicMin; the call sets *d_status to INT32_MAX first, which is what a clean batch leaves.  A row
 * whose class, truncated toward zero as numpy's astype(int) does, is not in [0, class_num), or with an x or y that is not finite, counts as such a box.  d_first is not trusted: rows outside
 * [0, n_boxes) are not read.
 * One launch (blockIdx.y the sample, chunked at 65535; blockIdx.x a chunk of YK_LABEL_CHUNK floats of one layer of that sample) after a
 * 4-byte memset node: a workgroup builds its chunk in LDS from the sample's candidate table - YK_LABEL_LDS_BOXES boxes at a time, a sample
 * with more is walked in tiles of that many, read from global memory again, by the same rule - and stores it once, 16 bytes per lane where
 * the address allows.  No workgroup waits for another and no floating-point atomics: two calls give the same bits.  Can be recorded in a graph.
 * n == 0: YK_OK, nothing launched.  NULL cfg, d_first, d_labels or d_status with n > 0, NULL d_boxes with n_boxes > 0, n < 0, n_boxes outside
 * 0 .. 2^30 - 1, n_layers outside 1 .. YK_MAX_LAYERS, an anchor_num outside 1 .. YK_MAX_ANCHORS, out_h or out_w <= 0, class_num < 1, an
 * unknown assign, an assign_iou outside (0, 1) with YK_ASSIGN_MULTI, sizes beyond size_t: YK_ERR_ARG, the message names the function and the
 * argument, nothing launched; these checks come before the device is needed.  No device: YK_ERR_NO_DEVICE. */
#define YK_LABEL_LDS_BOXES 512
#define YK_LABEL_CHUNK 4096
enum { YK_ASSIGN_BEST = 0, YK_ASSIGN_MULTI = 1 };
typedef struct {
    int32_t n_layers, class_num;
    int32_t assign;                                     /* YK_ASSIGN_* */
    int32_t reserved;                                   /* 0 */
    int32_t out_h[YK_MAX_LAYERS], out_w[YK_MAX_LAYERS]; /* Helper.out_hw */
    int32_t anchor_num[YK_MAX_LAYERS];
    double anchors[YK_MAX_LAYERS][YK_MAX_ANCHORS][2];   /* np.asarray(Helper.anchors, float): (w, h), image-relative */
    double assign_iou;                                  /* read with YK_ASSIGN_MULTI only */
} yk_label_cfg_t;                                       /* 584 bytes, no padding */
int yk_boxes_to_labels_f32(const yk_label_cfg_t *cfg, const double *d_boxes, int n_boxes, const int32_t *d_first, int n, float *d_labels,
                           int32_t *d_status, void *stream);
/* Draws detections INTO the pictures of a ragged batch, in place (inference.py's PIL loop plus keras_inference.py:137-174's label with
 * its filled background), by the painter's rule: for picture i and its rows k = 0 .. count_i - 1 in order, later paint over earlier:
 *   corners   t = max(0, floorf(top + 0.5f)), l likewise from left; b = min(h, floorf(bottom + 0.5f)), r = min(w, floorf(right + 0.5f))
 *             (fp32 arithmetic, as NumPy evaluates inference.py's expression on a float32 row); b <= t or r <= l: the row draws nothing;
 *   outline   for j = 0 .. thickness - 1 while r - j > l + j and b - j > t + j: the one-pixel outline of the inclusive rectangle
 *             [l+j, t+j, r-j, b-j] in the class colour d_colors[class mod n_colors] (ImageDraw.rectangle(outline=)); clipped to the
 *             picture, so row h and column w are simply not painted;
 *   label     the rectangle at (l, t + 1) of 7*gw*mag by gh*mag pixels filled with the class colour, clipped; on it the 7 glyphs of
 *             '{:2d} {:.2f}'.format(class, score), a glyph pixel of value 1 painted black as a mag x mag block.  The score digits are
 *             rint((double)score * 100.0), half to even: exact, so they are Python's digits for every fp32 score in [0, 1].
 *             A class >= 100 draws its low two digits, a score >= 10 the low three digits of that rint; a negative class draws as 0,
 *             a negative or non-finite score as 0.00: every input has a defined picture.  gh == 0 switches the label off.
 * Pixels that no primitive covers are not written.  d_dets [n][cap][6] fp32 rows (top, left, bottom, right, score, class) and d_counts [n]
 * (clamped to [0, cap]) as yk_decode_py leaves them; d_colors [n_colors][3] u8; d_atlas [12][gh][gw] u8 of 0 / 1 for the glyphs
 * "0123456789. " (may be NULL when gh == 0).  max_pixels >= the largest h*w of the table: it sizes the launch, and a picture with more
 * pixels is drawn only in its first max_pixels.  One thread per pixel gathers: it walks the picture's rows from the last to the first and
 * writes the first primitive that covers it, once - no atomics, no ordering between workgroups, the same bytes on every run.  Rows whose
 * picture does not lie inside src_bytes are skipped.  NULL pointers, n <= 0, cap <= 0, n_colors <= 0, gh < 0, gw <= 0, src_bytes == 0,
 * max_pixels == 0: YK_ERR_ARG.  Can be recorded in a graph. */
int yk_draw_dets_u8(uint8_t *d_buf, size_t src_bytes, const yk_ragged_row_t *d_table, int n, const float *d_dets, int cap,
                    const int32_t *d_counts, const uint8_t *d_colors, int n_colors, const uint8_t *d_atlas, int gh, int gw,
                    size_t max_pixels, void *stream);

/* ---- JPEG encoding of a ragged batch on the device (`make detect ENCODE=gpu`) ----------------
 * Baseline sequential JFIF as PIL's default save() writes it structurally: 8 bit, YCbCr, 4:2:0 (16x16 MCUs: Y00 Y01 Y10 Y11 Cb Cr), one
 * interleaved scan, the four Huffman tables of ITU-T T.81 Annex K.3, no restart markers.  The device produces the entropy-coded scan;
 * the headers and EOI are the host's (k210_yolo_framework_amd/jpeg.py).  Integer arithmetic only, so that a restatement gives the same bytes:
 *   colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *             Cb = ((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128,  Cr = ((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128
 *             (arithmetic shifts, results clamped to [0, 255]); a picture is extended to multiples of 16 by replicating its last column
 *             and row on the RGB indices (min(x, w-1), min(y, h-1)); chroma = (a + b + c + d + 2) >> 2 over each 2x2 group;
 *   DCT       s = p - 128, T[u][x] = rint(2^13 a(u) cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u>0) = 1/2 (float64, tabulated);
 *             rows r1 = (sum_x T[u][x] s[x] + 512) >> 10, columns c = sum_y T[v][y] r1[y] (the coefficient times 2^16, |c| < 1.3e8);
 *   quantise  q = sign(c) * ((|c| + d * 2^15) / (d * 2^16)), d the table entry; AC clamped to +-1023, DC differences to +-2047;
 *   coding    T.81: zigzag, DC difference to the previous block of the component (0 at the start of a picture), (run, size) symbols with
 *             ZRL and EOB, bits MSB first, the last byte padded with 1-bits, 0x00 after every 0xFF byte (a padded last byte included). */
/* HOST helper: the Annex K.1 luminance and chrominance tables scaled by the IJG rule (scale = 5000 / q for q < 50, else 200 - 2q;
 * t = clamp((base * scale + 50) / 100, 1, 255)) into h_qtab [2][64], natural order.  quality outside 1 .. 100, NULL: YK_ERR_ARG. */
int yk_jpeg_tables(int quality, uint8_t *h_qtab);
/* HOST helper: the workspace and the output capacity yk_jpeg_encode_ragged_u8 needs for the n rows of a HOST table, from the proved
 * worst case of 1660 bits per 8x8 block (1248 bytes per MCU before stuffing, twice that after).  Rows with h <= 0 or w <= 0 count
 * nothing; a row with h or w > 65535, NULL pointers, n <= 0: YK_ERR_ARG.  Needs no device. */
int yk_jpeg_workspace_bytes(const yk_ragged_row_t *h_table, int n, size_t *work_bytes, size_t *out_capacity);
/* Encodes the n pictures of a ragged batch (the buffer and table of yk_letterbox_ragged_u8 / yk_draw_dets_u8) with the quantisation
 * tables d_qtab (DEVICE, [2][64] natural order).  d_out receives the scan data of picture i at [d_out_off[i], d_out_off[i + 1]), packed
 * back to back; nothing at or beyond d_out_off[n] is written, d_buf is only read.  d_work: 16-byte aligned device scratch of work_bytes,
 * contents undefined before and after.  d_table is DEVICE memory, so this call cannot read it: NULL pointers, n <= 0, src_bytes == 0, a
 * misaligned d_work and capacities that hold not even one MCU are YK_ERR_ARG here, and checking them against yk_jpeg_workspace_bytes
 * is the caller's job (engine.jpeg_encode_ragged_u8 does it on the host table).  The kernels do not trust the table either: a row with
 * h <= 0, w <= 0, h or w > 65535 or offset + 3*h*w > src_bytes gives a zero-length stream and nothing of d_buf is read for it, and a
 * table that needs more than work_bytes or out_capacity hold gives n zero-length streams - no input writes outside the buffers.
 * The same bytes on every run.  Never synchronises; can be recorded in a graph. */
int yk_jpeg_encode_ragged_u8(const uint8_t *d_buf, size_t src_bytes, const yk_ragged_row_t *d_table, int n, const uint8_t *d_qtab,
                             void *d_work, size_t work_bytes, uint8_t *d_out, size_t out_capacity, uint64_t *d_out_off /* [n + 1] */,
                             void *stream);

/* ---- JPEG decoding of a batch into a ragged buffer on the device (`make detect DECODE=gpu`) -----------
 * Baseline sequential files (SOF0, 8 bit; grey, or YCbCr 4:4:4 / 4:2:2 / 4:2:0; one interleaved scan; any restart interval), parsed on
 * the host (k210_yolo_framework_amd/jpeg.py: parse_baseline refuses everything else by name, plan_decode builds what this call takes):
 *   d_scan    the entropy-coded segments packed in one buffer: the bytes after the SOS header up to, not including, EOI - stuffed zeros
 *             and RSTn markers left in place - each segment 4-byte aligned and followed by at least 8 zero bytes;
 *   d_pics    one yk_jpeg_pic_t per picture (below);
 *   d_tables  per picture, at table_offset (a multiple of 4): 3840 bytes = q u8 [4][64], the quantisation tables by id in natural order,
 *             then the Huffman tables DC 0, DC 1, AC 0, AC 1 of 896 bytes each: look u16 [256] (for the 8 bits c: length << 8 | symbol of
 *             the code of at most 8 bits that c begins with, 0 = none), maxcode i32 [16] (largest code of length l at [l - 1], -1 = none),
 *             delta i32 [16] (index of the length's first value - its first code), vals u8 [256] (HUFFVAL);
 *   d_rows    the yk_ragged_row_t table of the destination: picture i is written as [h][w][3] u8 at d_dst + d_rows[i].offset - the layout
 *             yk_letterbox_ragged_u8, yk_draw_dets_u8 and yk_jpeg_encode_ragged_u8 read - and only these h * w * 3 bytes are written.
 * The rule, integer only, so that a restatement (tests/jpeg_dec_ref.py) gives the same bytes:
 *   entropy   T.81 F.2.2: Huffman codes MSB first, the 0x00 after an 0xFF skipped, EXTEND as in the standard, the DC a difference to the
 *             previous block of its component (0 at the start and after every restart marker), AC (run, size) with ZRL and EOB; the
 *             position behind the k-th RSTn is block k * Ri * (blocks per MCU);
 *   dequant   c = clamp(q * Q, -32767, 32767) in int32, q the coefficient, Q the table entry;
 *   IDCT      T[u][x] = rint(2^13 a(u) cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u>0) = 1/2 (float64, tabulated; sum_u |T[u][x]| <= 21641);
 *             columns t[y][u] = clamp((sum_v T[v][y] c[v][u] + 512) >> 10, -65535, 65535)   (|sum| <= 32767 * 21641 < 2^30),
 *             rows    p[y][x] = clamp(((sum_u T[u][x] t[y][u] + 32768) >> 16) + 128, 0, 255) (|sum| <= 65535 * 21641 < 2^31 - 2^15);
 *             (the clamp of t is out of reach of any coefficients an encoder derives from 8-bit samples: there |t| < 2^16 / 1.7);
 *   upsample  chroma of 4:2:2: out[2i] = (3 C[i] + C[i-1] + 1) >> 2, out[2i+1] = (3 C[i] + C[i+1] + 2) >> 2; of 4:2:0: per column
 *             v = 3 near + far (the rows y >> 1 and, for even y, the one above it, for odd y the one below), then
 *             out[2i] = (3 v[i] + v[i-1] + 8) >> 4, out[2i+1] = (3 v[i] + v[i+1] + 7) >> 4; neighbour indices clamped to the component's
 *             real size ceil(w / 2) x ceil(h / 2), not to the MCU padding;
 *   colour    R = Y + ((91881 (Cr-128) + 32768) >> 16), G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16),
 *             B = Y + ((116130 (Cb-128) + 32768) >> 16): rint(c 2^16) of 1.40200, 0.34414, 0.71414, 1.77200, arithmetic shifts, clamped to
 *             [0, 255]; a grey picture writes Y to all three bytes.
 * Corrupt input has a defined result as well: every read is clamped to the picture's segment (bytes beyond it read 0), a code no table
 * entry matches consumes one bit, a run that passes index 63 ends its block, any 0xFF followed by a non-zero byte is a marker: once the
 * bits in front of it are used up (1-bits that fill the last byte in front of a marker or of the end are padding) decoding goes on behind
 * it at the first block of an MCU.  Such input changes coefficients and the status, never an address. */
#define YK_JPEG_DECODE_CHUNK 128    /* the default chunk_bytes */
typedef struct yk_jpeg_pic {
    uint64_t scan_offset;   /* of the picture's segment in d_scan, a multiple of 4 */
    uint32_t scan_bytes;    /* its length, 1 .. 2^28 - 1 */
    uint32_t table_offset;  /* of the picture's 3840 bytes in d_tables, a multiple of 4 */
    int32_t h, w;           /* 1 .. 65535 */
    int32_t ncomp;          /* 1 or 3 */
    int32_t hs, vs;         /* luma sampling: 1x1, 2x1 or 2x2 (chroma is 1x1; grey: 1x1) */
    int32_t restart;        /* MCUs per restart interval, 0 = none */
    uint8_t tq[4], td[4], ta[4];    /* per component: quantisation table 0 .. 3, DC and AC Huffman table 0 .. 1 */
    uint32_t reserved;
} yk_jpeg_pic_t;            /* 56 bytes, no padding */
/* HOST helper: the workspace yk_jpeg_decode_ragged_u8 needs for the n rows of a HOST table: 192 bytes per 8x8 block of the MCU-padded
 * pictures (coefficients, component planes) and a header.  A row that is not a picture the decoder takes (sizes, component count,
 * sampling, selectors), NULL pointers, n <= 0: YK_ERR_ARG.  Needs no device. */
int yk_jpeg_decode_workspace_bytes(const yk_jpeg_pic_t *h_pics, int n, size_t *work_bytes);
/* Decodes n pictures.  d_status[i] = 0 when exactly the picture's MCUs were decoded and the stream ended inside its last byte; otherwise
 * bits say why: 1 the row leaves scan_bytes / table_bytes / dst_bytes, is no picture this decoder takes or disagrees with d_rows[i] on
 * h, w (nothing is written for it); 2 too few MCUs in the stream; 4 data behind the last MCU; 8 a marker that is not the expected RSTn at
 * the end of its interval; 16 the DEVICE table needs more blocks than work_bytes hold (then every status has this bit and nothing is
 * written).  chunk_bytes: how much of the stuffed stream one thread decodes speculatively, a multiple of 4 in 4 .. 1024, 0 = the default;
 * the result does not depend on it.  d_scan and d_tables 4-byte, d_pics 8-byte, d_work 16-byte aligned; these, NULL pointers, n <= 0,
 * zero sizes and a workspace that holds not one block are YK_ERR_ARG here; checking the tables is the kernels' job, since they are DEVICE
 * memory.  d_work: contents undefined before and after, but for uint32 [n] at byte ((4 (n + 1) + 15) & ~15): the rounds the fixed-point
 * iteration of the Huffman stage took per picture, summed over its tiles of 256 chunks (a figure for tools, no part of the result).
 * The same bytes on every run.  Never synchronises; can be recorded in a graph. */
int yk_jpeg_decode_ragged_u8(const uint8_t *d_scan, size_t scan_bytes, const yk_jpeg_pic_t *d_pics, const uint8_t *d_tables,
                             size_t table_bytes, const yk_ragged_row_t *d_rows, int n, uint8_t *d_dst, size_t dst_bytes, void *d_work,
                             size_t work_bytes, int32_t *d_status, int chunk_bytes, void *stream);

/* ---- training step, loss level (tools/utils.py:708-793 create_loss_fn, :662-705 calc_ignore_mask,
 *      tools/custom.py:13-75 Yolo_Precision/Yolo_Recall) for ONE output layer.
 * d_y_true / d_y_pred: device fp32 [batch][out_h][out_w][A][5+C] (labels from Helper.box_to_label / raw outputs).
 * d_loss[6]   = {total, xy, wh, obj, noobj, cls}, each already divided by cfg->batch_size like the reference.
 * d_grad      = dL/dy_pred, same shape as d_y_pred (NULL to skip) — what TF autodiff yields for this graph.
 * d_ignore    = ignore mask [batch][out_h][out_w][A] (NULL to skip).
 * d_counts[3] = running {tp, fp, fn}; this batch's counts are ADDED (Keras metric assign_add); NULL to skip. */
typedef struct {
    int32_t out_h, out_w, anchor_num, class_num;
    float anchors[YK_MAX_ANCHORS][2];       /* Helper.anchors[layer] */
    float obj_thresh, iou_thresh, obj_weight, noobj_weight, wh_weight;
    int32_t batch_size;                     /* Helper.batch_size (the divisor in utils.py:771-787) */
} yk_loss_cfg_t;
int yk_yolo_loss(const yk_loss_cfg_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                 float *d_grad, float *d_ignore, float *d_counts, void *stream);
/* The same loss with a choice of box term.  YK_BOX_LOSS_MSE: the xy / wh terms above, the same bits as yk_yolo_loss.
 * _GIOU / _DIOU / _CIOU: for every object cell (y_true conf > obj_thresh) the IoU-family loss l between the decoded prediction and the
 * label box, weighted conf * (2 - tw * th) * box_weight; xy, wh and their gradients are then not computed: both report 0 and
 * total = obj + noobj + cls + box.  Cells without an object add exactly 0 to the box term and to gradient entries 0..3.
 * d_loss[7] = {total, xy, wh, obj, noobj, cls, box}; the other pointers as for yk_yolo_loss.  An unknown box_loss: YK_ERR_ARG. */
enum { YK_BOX_LOSS_MSE = 0, YK_BOX_LOSS_GIOU = 1, YK_BOX_LOSS_DIOU = 2, YK_BOX_LOSS_CIOU = 3 };
typedef struct {
    int32_t out_h, out_w, anchor_num, class_num;       /* yk_loss_cfg_t's fields, in its order ... */
    float anchors[YK_MAX_ANCHORS][2];
    float obj_thresh, iou_thresh, obj_weight, noobj_weight, wh_weight;
    int32_t batch_size;
    int32_t box_loss;                                   /* ... then YK_BOX_LOSS_* */
    float box_weight;                                   /* weight of the box term (wh_weight is not used by the IoU losses) */
} yk_loss_cfg_ex_t;
int yk_yolo_loss_ex(const yk_loss_cfg_ex_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                    float *d_grad, float *d_ignore, float *d_counts, void *stream);
/* The same loss with options on the objectness and class terms (the rule is stated in lossopt.py).  With p = sigmoid(x),
 * bce the cross entropy above and z a target in [0, 1]:
 *   label_smooth eps  every class target becomes z (1 - eps) + eps / 2.
 *   obj_target        YK_OBJ_TARGET_IOU: in an object cell (y_true conf > obj_thresh) the objectness target is clamp(IoU, 0, 1) of the decoded
 *                     prediction with the label box, IoU = I / (bw bh + tw th - I + 1e-7), a constant in the gradient; in the IoU box modes
 *                     it is the IoU of the box term.  The weights, the ignore mask, (2 - tw th) and the counters stay on y_true conf.
 *   focal             bit 0 (YK_FOCAL_OBJ): the obj and noobj sums, bit 1 (YK_FOCAL_CLS): the class sum take
 *                     fl(z, x) = a_t (1 - p_t)^gamma bce(z, x),  1 - p_t = z sigmoid(-x) + (1 - z) sigmoid(x),
 *                     a_t = z alpha + (1 - z)(1 - alpha), or 1 when alpha = 0, in place of bce; the gradient is the full derivative.
 * Ranges: focal 0 .. 3; focal_gamma 0 or 1 .. 5; focal_alpha 0 or inside (0, 1); label_smooth in [0, 1); obj_target YK_OBJ_TARGET_*.
 * Anything else is YK_ERR_ARG, the message names the field, nothing is launched.  gamma = 0 with alpha = 0 is bce.  With every option off
 * the call gives the bits of yk_yolo_loss_ex.  d_loss[7] and the other parameters are those of yk_yolo_loss_ex; obj, noobj and cls report
 * the new terms.  The sums are taken in the same fixed order: two calls give the same bits. */
enum { YK_FOCAL_OBJ = 1, YK_FOCAL_CLS = 2 };
enum { YK_OBJ_TARGET_LABEL = 0, YK_OBJ_TARGET_IOU = 1 };
typedef struct {
    int32_t out_h, out_w, anchor_num, class_num;       /* yk_loss_cfg_ex_t's fields, in its order ... */
    float anchors[YK_MAX_ANCHORS][2];
    float obj_thresh, iou_thresh, obj_weight, noobj_weight, wh_weight;
    int32_t batch_size;
    int32_t box_loss;
    float box_weight;
    int32_t focal;                                      /* ... then YK_FOCAL_* bits */
    float focal_gamma, focal_alpha, label_smooth;
    int32_t obj_target;                                 /* YK_OBJ_TARGET_* */
} yk_loss_cfg_opt_t;
int yk_yolo_loss_opt(const yk_loss_cfg_opt_t *cfg, const float *d_y_true, const float *d_y_pred, int batch, float *d_loss,
                     float *d_grad, float *d_ignore, float *d_counts, void *stream);

/* Knowledge distillation on the raw outputs of ONE output layer (the rule is stated in distill.py, csrc/yk_distill.hip).
 * d_teacher / d_pred: device fp32 [batch][rows_per_image][5 + class_num], the teacher's and the student's raw outputs (rows_per_image =
 * out_h * out_w * A); the teacher is a constant.  With sp(z) = log(1 + e^z) in its stable form (finite for logits of +-80 and beyond),
 *   kl(q, p) = sigmoid(q) (sp(-p) - sp(-q)) + (1 - sigmoid(q)) (sp(p) - sp(q))      (>= 0; d/dp = sigmoid(p) - sigmoid(q))
 * and a = sigmoid(q_o), a row p = [x, y, w, h, o, c..] adds
 *   obj = kl(q_o, p_o),  cls = a sum_c kl(q_c, p_c),  box = a (kl(q_x, p_x) + kl(q_y, p_y) + ((p_w - q_w)^2 + (p_h - q_h)^2) / 2).
 * d_loss[4]   = {total, obj, cls, box}: weight / batch_size times the sums over all rows (batch_size: the divisor of yk_yolo_loss).
 * d_grad      = the gradient by d_pred is ADDED to it (same shape; NULL to skip): weight / batch_size times a (sigmoid(p) - sigmoid(q)) for x,
 *               y and every class, a (p - q) for w and h, sigmoid(p_o) - sigmoid(q_o) for o.
 * Where the bits of p and q are equal every entry of d_loss is +0.0 and d_grad keeps its bits.  The sums are taken in float64 in a fixed order
 * and no float atomics are used: two calls give the same bits.  d_loss does not depend on whether d_grad is given.  A NULL d_teacher, d_pred
 * or d_loss, batch <= 0, rows_per_image <= 0, class_num < 1 or batch_size <= 0: YK_ERR_ARG, nothing launched.  Asynchronous on `stream`; can be
 * recorded in a graph once the stream has run it eagerly at its largest size. */
int yk_distill_loss_f32(const float *d_teacher, const float *d_pred, int batch, int rows_per_image, int class_num, float weight,
                        int batch_size, float *d_loss, float *d_grad, void *stream);

/* ---- training step, network level (keras_train.py:73-98: model.fit = forward in training mode + TF autodiff +
 *      Adam; the reference gets every one of these ops from TensorFlow 1.14).  All tensors are device fp32, NHWC,
 *      dense (no channel padding); "M" is batch*height*width.  k210_yolo_framework_amd/train.py strings them into
 *      the step.
 *
 * yk_gemm_f32: C[M][N] = alpha * op(A) * op(B) + beta * C, row-major, op = transpose when trans* != 0
 *   (A is [M][K] or, transposed, [K][M]; B is [K][N] or [N][K]).  Conv2D 1x1 forward  Y = X * W^T,
 *   data gradient dX = dY * W, weight gradient dW = dY^T * X (tf Conv2DBackpropInput / ...Filter). */
int yk_gemm_f32(int transA, int transB, int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb,
                float beta, float *C, int ldc, void *stream);
/* `count` independent GEMMs of one layout in as few launches as possible (the weight gradients of a whole backward pass): the problems'
 * tiles share one grid and the K slices are sized for the group (results reproducible run to run; equal to yk_gemm_f32's within fp32
 * summation-order differences). */
int yk_gemm_f32_grouped(int count, int transA, int transB, const int *M, const int *N, const int *K, float alpha, const float *const *A,
                        const int *lda, const float *const *B, const int *ldb, float beta, float *const *C, const int *ldc, void *stream);
/* 3x3 Conv2D through a column matrix and GEMM, for what the implicit GEMM below does not cover (the 3-channel stem, the strided data
 * gradient): col [B*Ho*Wo][9*C], k = (ky*3+kx)*C + c; col2im is the adjoint (sums overlaps). */
int yk_im2col3x3_f32(const float *x, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t, int pad_l,
                     float *col, void *stream);
int yk_col2im3x3_f32(const float *col, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t, int pad_l,
                     float *dx, void *stream);
/* 3x3 Conv2D as an implicit GEMM (no column matrix); weights [Co][9 * Ci] (k = (ky*3+kx)*Ci + c).  A NULL tensor or a non-positive size:
 * YK_ERR_ARG.  Needs Ci % 4 == 0 (Co % 4 == 0 too for the gradients; stride 1 for the data gradient) and 16-byte aligned tensors -
 * YK_ERR_UNSUPPORTED otherwise (yk_im2col3x3_f32 / yk_col2im3x3_f32 + yk_gemm_f32 cover those).
 * yk_conv3x3_bn_fwd_f32: z = conv(x); with gamma != NULL also BatchNormalization(training) + activation (+ residual) -> y, as yk_gemm_bn_fwd_f32.
 * Forward and weight gradient add in the order of im2col + yk_gemm_f32: bitwise the same result. */
int yk_conv3x3_bn_fwd_f32(const float *x, const float *w, int B, int Hi, int Wi, int Ci, int Ho, int Wo, int stride, int pad_t, int pad_l, int Co,
                          float *z, const float *gamma, const float *beta, float eps, int act, float alpha, float *y, float *save_mean,
                          float *save_invstd, float *moving_mean, float *moving_var, float momentum, const float *res, void *stream);
int yk_conv3x3_bwd_weight_f32(const float *x, const float *dz, int B, int Hi, int Wi, int Ci, int Ho, int Wo, int stride, int pad_t, int pad_l,
                              int Co, float *dw, void *stream);
int yk_conv3x3_bwd_data_f32(const float *dz, const float *w, int B, int Hi, int Wi, int Ci, int Ho, int Wo, int stride, int pad_t, int pad_l, int Co,
                            float *dx, void *stream);
/* DepthwiseConv2D 3x3, weights [9][C].  A NULL tensor or a non-positive size: YK_ERR_ARG, checked on the host before anything is launched
 * (yk_dw3x3_bn_fwd_f32 below too).  Any C and any 4-byte aligned address: four channels per thread when C % 4 == 0 and the call's
 * tensors are 16-byte aligned, one channel per thread otherwise - the same sums in the same order (the BatchNormalization apply passes
 * below choose by the same rule). */
int yk_dw3x3_fwd_f32(const float *x, const float *w, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t,
                     int pad_l, float *y, void *stream);
int yk_dw3x3_bwd_data_f32(const float *dy, const float *w, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride,
                          int pad_t, int pad_l, float *dx, void *stream);
int yk_dw3x3_bwd_weight_f32(const float *x, const float *dy, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride,
                            int pad_t, int pad_l, float *dw, void *stream);
/* the depthwise weight gradients of `count` layers in two launches; geom: 9 ints per problem (B, Hi, Wi, C, Ho, Wo, stride, pad_t, pad_l);
 * every problem computed exactly as by yk_dw3x3_bwd_weight_f32 (bitwise the same). */
int yk_dw3x3_bwd_weight_grouped_f32(int count, const float *const *x, const float *const *dy, const int *geom, float *const *dw, void *stream);
/* BatchNormalization(training=True) fused with the activation that follows it (act: YK_ACT_*).
 * fwd: batch mean / biased variance over M, y = act(gamma*(z-mean)*invstd + beta); saves mean and invstd and,
 *      when moving_mean/moving_var are given, updates them with `momentum` (Keras: 0.99).
 * bwd: dy is the gradient w.r.t. y; writes dz, dgamma, dbeta (all three are required).  A NULL pointer, M <= 0 or C <= 0: YK_ERR_ARG,
 *      checked on the host before anything is launched. */
int yk_bn_train_fwd_f32(const float *z, long long M, int C, const float *gamma, const float *beta, float eps, int act,
                        float alpha, float *y, float *save_mean, float *save_invstd, float *moving_mean,
                        float *moving_var, float momentum, void *stream);
/* ... with the residual of a following keras Add() folded into the apply pass: y = res + act(BN(z)) (keras_mobilenet_v2.py:483-484) */
int yk_bn_train_fwd_res_f32(const float *z, long long M, int C, const float *gamma, const float *beta, float eps, int act,
                            float alpha, float *y, float *save_mean, float *save_invstd, float *moving_mean,
                            float *moving_var, float momentum, const float *res, void *stream);
/* Conv2D / DepthwiseConv2D + BatchNormalization(training=True) + activation (+ residual) forward in ONE call: z = the convolution
 * (X [M][K] row-major with leading dimension ldx, W [N][K]: a 1x1 conv's input, or the column matrix of a 3x3 conv that
 * yk_conv3x3_bn_fwd_f32 does not take), y as yk_bn_train_fwd_res_f32.
 * The producer of z leaves the partial sums of the batch statistics, so z is not read again for them.  Same arithmetic per element as the
 * separate calls; the statistics are added in another (fixed) order in double. */
int yk_gemm_bn_fwd_f32(int M, int N, int K, const float *X, int ldx, const float *W, int ldw, float *z, const float *gamma, const float *beta,
                       float eps, int act, float alpha, float *y, float *save_mean, float *save_invstd, float *moving_mean,
                       float *moving_var, float momentum, const float *res, void *stream);
int yk_dw3x3_bn_fwd_f32(const float *x, const float *w, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t, int pad_l,
                        float *z, const float *gamma, const float *beta, float eps, int act, float alpha, float *y, float *save_mean,
                        float *save_invstd, float *moving_mean, float *moving_var, float momentum, const float *res, void *stream);
int yk_bn_train_bwd_f32(const float *z, const float *dy, long long M, int C, const float *gamma, const float *beta,
                        const float *save_mean, const float *save_invstd, int act, float alpha, float *dz, float *dgamma,
                        float *dbeta, void *stream);
int yk_bias_add_f32(float *y, long long M, int C, const float *bias, void *stream);       /* y[m][c] += bias[c] */
int yk_colsum_f32(const float *x, long long M, int C, float *out, void *stream);          /* out[c] = sum_m x[m][c] */
int yk_upsample2x_bwd_f32(const float *dy, int B, int H, int W, int C, float *dx, void *stream); /* UpSampling2D(2) adjoint */
/* MaxPooling2D(2, stride, 'same'): argmax [B][Ho][Wo][C] u8 = winning tap (first maximum, row-major window) */
int yk_maxpool2_fwd_f32(const float *x, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, float *y, uint8_t *argmax,
                        void *stream);
int yk_maxpool2_bwd_f32(const float *dy, const uint8_t *argmax, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, float *dx,
                        void *stream);
/* keras.regularizers.l2(weight) of yolonet.py:245-250 over `nseg` segments of one flat parameter buffer in one pass: *out = weight * sum w^2
 * (want_value) and / or grads[j] += 2 * weight * params[j] (want_grad).  d_prefix [nseg + 1] = running sum of the segment lengths (device,
 * int64), d_offset [nseg] = start of every segment in the flat buffer, total = d_prefix[nseg]. */
int yk_l2_segments_f32(const float *params, float *grads, const long long *d_prefix, const long long *d_offset, int nseg, long long total,
                       float weight, int want_value, int want_grad, float *out, void *stream);
int yk_axpy_f32(long long n, float a, const float *x, float *y, void *stream);            /* y += a*x */
/* keras.optimizers.Adam as keras_train.py:74-76 configures it (lr, decay; beta 0.9/0.999, eps 1e-7):
 * lr_t = lr/(1+decay*iterations) * sqrt(1-b2^t)/(1-b1^t), t = iterations+1; p -= lr_t*m/(sqrt(v)+eps).
 * g is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int yk_adam_f32(long long n, float *p, const float *g, float *m, float *v, float lr, float decay, long long iterations,
                float beta1, float beta2, float eps, float grad_scale, void *stream);
/* The optional parts of the update (the rule is stated in k210_yolo_framework_amd/optim.py).
 * yk_sumsq_f32: *d_out = sum of x[i]^2, every square (exact) and the whole sum in float64.  Workgroups own tiles of YK_SUMSQ_TILE floats and
 *   leave one partial each in d_work (yk_sumsq_workspace_bytes, needs no device; 8-byte aligned, contents undefined before and after); a
 *   finishing launch folds them.  Who adds what depends on n alone and no atomics are used: two calls give the same bits, all zeros give
 *   +0.0.  Asynchronous on `stream`, nothing allocated, nothing synchronised: capturable.
 * yk_adam_ex_f32: yk_adam_f32 with two optional parts around adam_kernel's unchanged statements, in one pass.
 *   d_sumsq (NULL: no clipping): every thread forms c = (float)fmin(1.0, clip_norm / (sqrt(*d_sumsq) + 1e-6)) in double and uses
 *            (g[i] * grad_scale) * c for the gradient; g is only read.  A NaN sum gives c = 1 (the NaN gradients reach the update), an
 *            infinite one c = 0.
 *   ema     (NULL: none): after the update, e = ema[i]; ema[i] = e + ema_omd * (p_new - e), ema_omd = 1 - decay.  Where p_new == e the average
 *            keeps its bits, and ema_omd = 0 changes nothing.
 *   With both NULL the stored p, m, v are yk_adam_f32's bit for bit.  16-byte accesses when n % 4 == 0 and every buffer is 16-byte aligned,
 *   element by element otherwise.
 * yk_ema_f32: the average's statement alone, ema[i] += ema_omd * (src[i] - ema[i]) in the written order, for buffers Adam does not own.
 * NULL required pointers, n <= 0, iterations < 0, a negative clip_norm with d_sumsq, a misaligned double pointer: YK_ERR_ARG, nothing launched. */
#define YK_SUMSQ_TILE 4096
int yk_sumsq_workspace_bytes(long long n, size_t *bytes);
int yk_sumsq_f32(const float *x, long long n, double *d_work, double *d_out, void *stream);
int yk_adam_ex_f32(long long n, float *p, const float *g, float *m, float *v, float *ema, const double *d_sumsq, float lr, float decay,
                   long long iterations, float beta1, float beta2, float eps, float grad_scale, float clip_norm, float ema_omd, void *stream);
int yk_ema_f32(long long n, const float *src, float *ema, float ema_omd, void *stream);
/* Magnitude pruning (tfmot prune_low_magnitude of keras_train.py:59-71) over `nseg` segments of one flat parameter buffer
 * in one call.  Segment s = params[d_offset[s] .. + d_size[s]) (device, int64; d_size >= 0); d_keep[s] = k, any int64, clamped to
 * [1, d_size[s]] (0, a negative k: 1; k > d_size: d_size).
 * Outputs per segment: d_threshold[s] = the exact k-th largest |w| (a radix select on the uint32 pattern of |w|: equal to a sort),
 * mask[d_offset[s] + e] = |w| >= threshold (1 / 0; ties at the threshold are all kept; bytes outside the segments are not written),
 * d_kept[s] = number of mask bytes set.  "Largest" and ">=" are those of the sign-cleared bit pattern as an unsigned integer: -0.0 equals
 * +0.0, denormals order like any number, and a NaN ranks above infinity (among NaNs the payload decides); d_threshold[s] carries that
 * pattern, payload included.  A segment of size 0 gets no output: d_threshold[s], d_kept[s] and every mask byte keep what the caller
 * left there, it owns no tile (d_tile_first[s] == d_tile_first[s + 1]) and it changes nothing for the other segments; at least one
 * segment must have a tile.  Workgroups own tiles of YK_PRUNE_TILE elements of one segment: d_tile_first [nseg + 1] (device,
 * int32) = running sum of ceil(d_size / YK_PRUNE_TILE), ntiles = d_tile_first[nseg].  Integer atomics only: bitwise reproducible.
 * The call itself does not synchronise with the host; capturable once the stream's scratch has its size (one eager call); the clear of
 * the histograms is part of the recording.  A NULL pointer, nseg <= 0 or ntiles <= 0: YK_ERR_ARG, nothing launched. */
#define YK_PRUNE_TILE 4096
int yk_prune_tile(void); /* YK_PRUNE_TILE of the loaded library: callers that build d_tile_first without this header ask here */
int yk_prune_masks_f32(const float *params, const long long *d_offset, const long long *d_size, const long long *d_keep,
                       const int *d_tile_first, int nseg, int ntiles, uint8_t *mask, float *d_threshold, long long *d_kept, void *stream);
/* params[i] = mask[i] ? params[i] : +0.0f over n elements: any non-zero byte keeps, and a kept element keeps its bits (-0.0, a NaN's
 * payload).  Any alignment of either pointer; nothing outside [0, n) is written.  A NULL pointer or n <= 0: YK_ERR_ARG, nothing launched. */
int yk_mask_apply_f32(float *params, const uint8_t *mask, long long n, void *stream);

/* ---- KPU-exact mode: a kmodel v3 on the K210 KPU's integer arithmetic (kpu_load_kmodel / kpu_run_kmodel / kpu_get_output of
 *      main.c:274,303,310, batched).  Outputs are bit-identical to oracle/kpu_ref.py (the restated KPU pipeline); DESIGN.md 3.7.
 * The program is packed by k210_yolo_framework_amd/kmodel.py:pack_kpu from the parsed file (one parser):
 *   values  int32 [n_values][4] = (C, H, W, dtype 0 = uint8 / 1 = fp32), every tensor of the run, each in its own buffer
 *           ([max_batch][H][W][C], NHWC);
 *   ops     int64 [n_ops][YK_KPU_FIELDS], issued in order: op code, input value (-1 = the frame), output value, then per op
 *           (conv: kernel, pool type, pad value, shr_x, arg_x, blob offsets of the packed weights / per-channel constants / activation
 *           segments, kmodel layer index, frame shape; gather: channel offset, 256-byte table offset or -1; dequantize: scale, bias bits);
 *   outputs int32 [n_outputs] fp32 value ids;  blob: the bytes the ops address (16-byte aligned offsets).
 * Every op, pool type and kernel size the kernels do not implement is refused here (YK_ERR_UNSUPPORTED), as is any inconsistent
 * row (YK_ERR_ARG), and any tensor whose max_batch x C x H x W exceeds 2^30 elements (YK_ERR_UNSUPPORTED: the kernels index in 32 bits);
 * yk_kpu_run_u8 never fails on the program's content. */
#define YK_KPU_FIELDS 24
#define YK_KPU_NHWC 0 /* frames uint8 [batch][H][W][C] (engine.letterbox_u8 / yk_run_u8) */
#define YK_KPU_CHW 1  /* frames uint8 [batch][C][H][W] (what main.c feeds kpu_run_kmodel) */
typedef struct yk_kpu_plan yk_kpu_plan_t; /* opaque */
int yk_kpu_plan_create(yk_kpu_plan_t **out, const int64_t *ops, int n_ops, const int32_t *values, int n_values, const int32_t *outputs,
                       int n_outputs, const void *blob, size_t blob_len, int max_batch, int device);
void yk_kpu_plan_destroy(yk_kpu_plan_t *p);
/* asynchronous on `stream`; one launch per op, no other stream touched (capturable with yk_graph_*) */
int yk_kpu_run_u8(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, void *stream);
/* The statistics run (biascorrect.py): the launches of yk_kpu_run_u8 with the conv kernels' statistics instantiations, which
 * leave every tensor and output bit-identical and add z - the int64 pre-activation (acc * bn_mul >> bn_shift) + bn_add, before the segment
 * table - of every counted output element into d_zsum[first slot of the conv + oc].  The conv ops (dense and depthwise, in issue order) own
 * consecutive runs of OC slots, yk_kpu_stat_slots in all.  h_step [n_step = number of conv ops], each 1 or 2: with 2 only output pixels with
 * even oy and even ox are counted (a stride-2 depthwise conv that runs at stride 1 and is pooled by its reader).  Integer adds that wrap (sums
 * reduced in registers / LDS, then one 64-bit atomic per channel and wave / workgroup): independent of scheduling and launch geometry.  The sums
 * accumulate over runs; the caller zeroes d_zsum (8-byte aligned).  h_step is read before the call returns. */
int yk_kpu_stat_slots(const yk_kpu_plan_t *p);
int yk_kpu_run_stats_u8(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, const int *h_step, int n_step, uint64_t *d_zsum,
                        void *stream);
/* borrowed device pointer to output idx, fp32 [max_batch][h][w][c] (the layout of yk_get_output: yk_decode_py consumes it) */
int yk_kpu_get_output(yk_kpu_plan_t *p, int idx, float **d_ptr, size_t *bytes, int *h, int *w, int *c);
int yk_kpu_output_count(const yk_kpu_plan_t *p);
/* conv layer `layer_index` (kmodel layer index) of image `image` of the last run, uint8 CHW (n = C*H*W bytes); synchronises */
int yk_kpu_debug_read(yk_kpu_plan_t *p, int layer_index, int image, uint8_t *h_dst, size_t n);
/* the device-side twin: a BORROWED pointer to that layer's uint8 output of the last run, [max_batch][h][w][c] (NHWC, images h * w * c bytes
 * apart), valid until the plan is destroyed and rewritten by every run; does not synchronise (read it on the stream the run was issued on) */
int yk_kpu_layer_ptr(yk_kpu_plan_t *p, int layer_index, uint8_t **d_ptr, int *h, int *w, int *c);
/* launches one yk_kpu_run_u8 issues, and their median durations over `iters` runs (HIP events around every launch) */
int yk_kpu_launch_count(const yk_kpu_plan_t *p);
int yk_kpu_profile(yk_kpu_plan_t *p, const uint8_t *d_frames, int batch, int layout, int iters, void *stream, float *ms_out);

/* ---- calibration for 8-bit quantisation (quantize.py): tensor ranges of an fp32 forward pass, reduced on the device.
 * d_range holds YK_RANGE_WORDS uint32 per slot: {smallest key, largest key, flag, 0}.  The key of a float is its bit pattern made
 * order-preserving for unsigned comparison (-max < ... < -0 < +0 < ... < +max), so the reduction is integer min / max: bitwise independent
 * of scheduling, launch geometry and stream, and denormals are kept.  Infinities and NaNs do not enter a range; they set the slot's sticky
 * flag.  Launches are asynchronous on `stream`: one atomicMin / atomicMax pair per workgroup.  Bad arguments: YK_ERR_ARG.
 * yk_range_reset          every slot to "nothing seen" (min key all ones, max key 0, flag 0);
 * yk_range_f32            folds min / max of x[0..n) into `slot` (accumulates over calls);
 * yk_scale_act_range_f32  y[m][c] = act(z[m][c] * scale[c] + bias[c]) (act: YK_ACT_*, one rounding per operation: no FMA contraction),
 *                         M x C row-major, any M, C >= 1 (16-byte accesses when C % 4 == 0 and the pointers allow), and folds min / max
 *                         of y into `slot`;
 * yk_scale_act_chrange_f32  the per-channel twin (equalize.py): the same y, bit for bit, and min / max of y[.][c] into slot slot0 + c of a
 *                         buffer of the same layout (C slots from slot0; reset and read by the two calls around it).  One atomicMin /
 *                         atomicMax pair per channel and workgroup; any M, C >= 1, M * C may exceed 2^31;
 * yk_range_read          ONE device-to-host copy (synchronises), decoded on the host: h_min / h_max [n_slots] (+inf / -inf for a slot that
 *                         has seen nothing finite), h_flags [n_slots]. */
#define YK_RANGE_WORDS 4
int yk_range_reset(uint32_t *d_range, int n_slots, void *stream);
int yk_range_f32(const float *x, long long n, uint32_t *d_range, int slot, void *stream);
int yk_scale_act_range_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                           uint32_t *d_range, int slot, void *stream);
int yk_scale_act_chrange_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                             uint32_t *d_range, int slot0, void *stream);
int yk_range_read(const uint32_t *d_range, int n_slots, float *h_min, float *h_max, int *h_flags);

/* ---- per-channel sums of the pre-activation, for bias correction (biascorrect.py).
 * yk_scale_act_chsum_f32  the third twin of yk_scale_act_range_f32: the same y, bit for bit, and the sum over m of the fp32 PRE-activation
 *                         t = z[m][c] * scale[c] + bias[c] (before `act`: the quantity a kmodel's bn_add shifts) added to d_sum[slot0 + c], in
 *                         float64.  No floating-point atomics: workgroups own about YK_CHSUM_TILE elements (whole rows) and leave one partial
 *                         per channel in d_work (yk_chsum_workspace_bytes; needs no device; contents undefined before and after), a finishing
 *                         launch folds them; who adds what, and in which order, follows from (M, C) alone, so the same calls give the same bits
 *                         on any stream and with any alignment of the pointers.  The finishing launch walks the partials of a channel with
 *                         max(1, 256 / min(C, 256)) accumulators: more workgroups than that take more than one pass.  Sums accumulate over calls
 *                         (calls on one d_sum are ordered by their stream).  A NaN or an infinity is not added; it sets d_flags[slot0 + c].
 *                         Any M, C >= 1, M * C may exceed 2^31; 16-byte accesses when C % 4 == 0 and the pointers allow.
 * yk_chsum_reset          sums and flags of slots [0, n_slots) to zero;  yk_chsum_read  two device-to-host copies (synchronises). */
#define YK_CHSUM_TILE 16384
int yk_chsum_workspace_bytes(long long M, int C, size_t *bytes);
int yk_chsum_reset(double *d_sum, uint32_t *d_flags, int n_slots, void *stream);
int yk_scale_act_chsum_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y,
                           double *d_sum, uint32_t *d_flags, int slot0, double *d_work, void *stream);
int yk_chsum_read(const double *d_sum, const uint32_t *d_flags, int n_slots, double *h_sum, int *h_flags);

/* ---- per-channel quantisation error of a KPU tensor against a float tensor (qerror.py, which states the rule).
 * yk_qerr_u8_f32   q = uint8 codes [B][qH][qW][C], y = fp32 [B][ho][wo][C] with ho = ceil(qH / step), wo = ceil(qW / step), step 1 or 2: float
 *                  position (oy, ox) is compared with code position (step oy, step ox).  With yh = (double)(q - zp_y) * (double)s_y and
 *                  e = (double)y - yh (one rounding per operation, no contraction), channel c adds into slot slot0 + c of d_slots:
 *                    words 0..3, uint64: n (positions), the counts of q == 0 and of q == 255, a sticky flag;
 *                    words 4..9, double: sum y^2, sum e^2, sum e, sum y yh, sum yh^2, and the largest |e| (a maximum, not a sum).
 *                  A position whose y is a NaN or an infinity enters none of them and sets the flag.  No floating-point atomics: workgroups
 *                  own about YK_QERR_TILE elements (whole rows of C) and leave one partial per channel and quantity in d_work
 *                  (yk_qerr_workspace_bytes; needs no device; contents undefined before and after), a finishing launch folds them with
 *                  max(1, YK_QERR_BLOCK / min(C, YK_QERR_BLOCK)) accumulators per channel - more workgroups than that take more than one pass -
 *                  and adds the result to the slot (a plain load and store: calls on one d_slots are ordered by their stream).  Who adds what,
 *                  and in which order, follows from (B ho wo, C) alone: the same calls give the same bits on any stream and with any alignment
 *                  of the pointers.  16-byte loads of y and 4-byte loads of q when C % 4 == 0 and the pointers allow; any C >= 1;
 *                  B ho wo C may exceed 2^31.  d_slots and d_work 8-byte aligned.
 * yk_qerr_reset    slots [0, n_slots) to zero;  yk_qerr_read  one device-to-host copy (synchronises): h_counts [n_slots][4] = words 0..3,
 *                  h_sums [n_slots][6] = words 4..9.
 * yk_dequant_u8_f32  y[b][oy][ox][c] = (float)(q[b][step oy][step ox][c] - zp_y) * s_y, one fp32 rounding: what a reader of that KPU tensor
 *                  sees, in real units (the local walk of qerror.analyze). */
#define YK_QERR_WORDS 10
#define YK_QERR_TILE 16384
#define YK_QERR_BLOCK 256
int yk_qerr_workspace_bytes(long long M, int C, size_t *bytes);
int yk_qerr_reset(uint64_t *d_slots, int n_slots, void *stream);
int yk_qerr_u8_f32(const uint8_t *q, const float *y, int B, int qH, int qW, int C, int step, float s_y, int zp_y, uint64_t *d_slots, int slot0,
                   uint64_t *d_work, void *stream);
int yk_qerr_read(const uint64_t *d_slots, int n_slots, long long *h_counts, double *h_sums);
int yk_dequant_u8_f32(const uint8_t *q, int B, int qH, int qW, int C, int step, float s_y, int zp_y, float *y, void *stream);

/* ---- adaptive weight rounding (adaround.py, which states the rule).  All calls are asynchronous on `stream`, allocate nothing
 *      and do not synchronise; no floating-point atomics: the same calls give the same bits.  A NULL tensor or a non-positive size:
 *      YK_ERR_ARG, checked on the host before anything is launched.
 * yk_dw3x3_gram_f32        d_gram[c][i][j] += sum over (b, oy, ox) of x_i x_j, x_t = tap t = ky * 3 + kx of channel c at that output position
 *                          (0 outside the image); x NHWC fp32, the geometry arguments of yk_dw3x3_fwd_f32.  d_gram is float64 [C][9][9], the
 *                          FULL symmetric matrix (both halves are written, from the same sums).  Every product is exact in float64.  It ADDS,
 *                          so batches accumulate; the caller zeroes d_gram.  Workgroups own chunks of rows (output positions) - YK_DWGRAM_ROWS
 *                          each, more once there are over YK_DWGRAM_ROWS * YK_DWGRAM_MAX_CHUNKS rows - and leave 45 partials per channel in
 *                          d_work (yk_dw3x3_gram_workspace_bytes, needs no device; 8-byte aligned; contents undefined before and after); a
 *                          finishing launch adds the chunks in ascending order.  Who adds what follows from the shape alone.  Reads are
 *                          coalesced along C.
 * yk_adaround_step_f32     one Adam step (beta1 0.9, beta2 0.999, eps 1e-8, bias-corrected, step number t >= 1) on V [Co][K] of the loss
 *                          (1 / Co) sum_c E_c / E_c(nearest) + lam (1 / n_free) sum (1 - |2 h - 1|^beta), h = clip(sigmoid(V) 1.2 - 0.1, 0, 1),
 *                          whose gradient with respect to h is (2 s_w / Co) inv_e[c] P[c][k] - (2 lam beta / n_free) |2 h - 1|^(beta - 1)
 *                          sign(2 h - 1), P = D G for the D of the V given.  Elements with frozen[i] != 0 keep V, m and v.  Writes the next
 *                          D = s_w (h(V) - r), 0 at frozen elements.  One thread per element.
 * yk_adaround_dw_quad_f32  P[c][i] = sum_j G[c][i][j] D[c][j] for a depthwise layer: G float64 [C][9][9] as yk_dw3x3_gram_f32 leaves it, D and P
 *                          fp32 [C][9]; summed in float64, j ascending, rounded once.  (A dense layer's P = D G is yk_gemm_f32.)
 * yk_adaround_rowerr_f64   E[c] = sum_k D[c][k] P[c][k], D and P fp32 [Co][K], E float64 [Co]: exact products, a fixed order. */
#define YK_DWGRAM_ROWS 64
#define YK_DWGRAM_MAX_CHUNKS 256
int yk_dw3x3_gram_workspace_bytes(int B, int Ho, int Wo, int C, size_t *bytes);
int yk_dw3x3_gram_f32(const float *x, int B, int Hi, int Wi, int C, int Ho, int Wo, int stride, int pad_t, int pad_l, double *d_gram,
                      double *d_work, void *stream);
int yk_adaround_step_f32(float *V, float *m, float *v, const float *r, const uint8_t *frozen, const float *P, const float *inv_e, float *D,
                         int Co, int K, long long n_free, float s_w, float lam, float beta, float lr, int t, void *stream);
int yk_adaround_dw_quad_f32(const double *G, const float *D, int C, float *P, void *stream);
int yk_adaround_rowerr_f64(const float *D, const float *P, int Co, int K, double *E, void *stream);

/* ---- histograms for the clipped calibrations (quantize.clip_range): a second pass over the calibration set, after the ranges.
 * d_hist holds uint64 counts [n_slots][nbins], 16 <= nbins <= 4096; d_flags one uint32 per slot.  A slot's bins are equal parts of [lo, hi],
 * the range of its tensor widened to contain 0; the caller passes lo and inv = (float)(nbins / ((double)hi - lo)), rounded once (0 for
 * hi == lo).  The bin of v:  t = (v - lo) * inv  in fp32, one rounding per operation (no FMA);  t >= nbins -> nbins - 1,  t > 0 -> (int)t
 * (truncated),  otherwise 0.  So values outside [lo, hi] land in the end bins, denormals are kept, and a zero-width range puts everything in
 * bin 0.  A NaN or an infinity is not counted: it sets the slot's sticky flag.  Each workgroup counts in LDS (uint32) and adds its non-zero
 * bins with 64-bit atomics: integer adds only, so the counts are bitwise independent of scheduling, launch geometry and stream.  Launches are
 * asynchronous on `stream`.  Bad arguments, and an n so large that one workgroup could count 2^32 elements: YK_ERR_ARG.
 * yk_hist_reset          the counts of slots [0, n_slots) to 0 (the flags are the caller's to clear);
 * yk_hist_f32            counts x[0..n) into `slot` (accumulates over calls);
 * yk_scale_act_hist_f32  the twin of yk_scale_act_range_f32: the same y, bit for bit, stored by the same launch that counts it into `slot`;
 * yk_hist_read           the counts [n_slots][nbins] in one device-to-host copy (synchronises) and the n_slots flag words in a second. */
int yk_hist_reset(uint64_t *d_hist, int n_slots, int nbins, void *stream);
int yk_hist_f32(const float *x, long long n, float lo, float inv, int nbins, uint64_t *d_hist, uint32_t *d_flags, int slot, void *stream);
int yk_scale_act_hist_f32(const float *z, long long M, int C, const float *scale, const float *bias, int act, float alpha, float *y, float lo,
                          float inv, int nbins, uint64_t *d_hist, uint32_t *d_flags, int slot, void *stream);
int yk_hist_read(const uint64_t *d_hist, const uint32_t *d_flags, int n_slots, int nbins, uint64_t *h_counts, int *h_flags);

/* ---- quantisation-aware training (train.Trainer(qat=...)): the kmodel's uint8 codes simulated in fp32 inside the step.
 * The rule, quantize.qparams in fp32 with one rounding per operation (no FMA contraction), for a range (lo, hi):
 *   lo' = lo < 0 ? lo : +0, hi' = hi > 0 ? hi : +0;  hi' == lo': s = 1.0f / 255.0f, zp = 0;  else s = (hi' - lo') / 255.0f,
 *   zp = clamp(rintf((0 - lo') / s), 0, 255);  u = rintf(x / s) + zp, q = clamp(u, 0, 255), fq(x) = s * (q - zp).
 * fq(+-0) is +0.0 for every range; a NaN stays a NaN.  Straight-through gradient: 1 where 0 <= u <= 255, else 0.
 * All calls are asynchronous on `stream` and capturable (no allocation, no host synchronisation); bad arguments: YK_ERR_ARG.  16-byte
 * accesses where the pointers of a call share their position inside 16 bytes, scalar heads and tails; any n >= 1.
 * Tables: d_ranges = float [n_slots][2] (lo, hi; "nothing seen yet" is (+inf, -inf)); d_batch / d_wrange = uint32 [.][YK_RANGE_WORDS] in the
 * layout of yk_range_f32 (ordered keys + sticky non-finite flag).
 * yk_qat_weights_f32  segments s = params[d_offset[s] .. + d_size[s]) (device int64, d_size >= 1, inside [0, n)), tiles of YK_QAT_TILE
 *                     elements as yk_prune_masks_f32 takes them (d_tile_first [nseg + 1] = running sum of ceil(d_size / YK_QAT_TILE), ntiles
 *                     = its last entry).  params_q = params over all n elements, then every segment replaced by fq over ITS OWN exact
 *                     [min, max] (left in d_wrange[s]; no weight is ever clamped).  params is only read.  Three launches.
 * yk_qat_act_fwd_f32  yq = fq(y) over d_ranges[slot]; min / max of the UNQUANTISED finite y folded into d_batch[slot], a NaN or an infinity
 *                     sets that slot's flag instead.
 * yk_qat_act_bwd_f32  dy = dyq where 0 <= u(y) <= 255 over d_ranges[slot], else +0.0.  dy may be dyq (in place).
 * yk_qat_update_f32   one launch for all slots.  d_kind[i] == YK_QAT_SLOT_OWNER and the batch saw something finite:
 *                     r = momentum * r + one_minus_momentum * b for lo and hi (b = the decoded batch extreme), or with `observe`
 *                     r = (min(r_lo, b_lo), max(r_hi, b_hi)).  Every slot's batch extremes are reset afterwards (flags stay).  Then, in
 *                     ascending order, d_kind[i] == YK_QAT_SLOT_UNION: r = (min of lo, max of hi) of slots d_part0[i], d_part1[i] (< i). */
#define YK_QAT_TILE 4096
#define YK_QAT_SLOT_NONE 0
#define YK_QAT_SLOT_OWNER 1
#define YK_QAT_SLOT_UNION 2
int yk_qat_tile(void); /* YK_QAT_TILE of the loaded library */
int yk_qat_weights_f32(const float *params, long long n, const long long *d_offset, const long long *d_size, const int *d_tile_first, int nseg,
                       int ntiles, float *params_q, uint32_t *d_wrange, void *stream);
int yk_qat_act_fwd_f32(const float *y, long long n, const float *d_ranges, int slot, float *yq, uint32_t *d_batch, void *stream);
int yk_qat_act_bwd_f32(const float *dyq, const float *y, long long n, const float *d_ranges, int slot, float *dy, void *stream);
int yk_qat_update_f32(float *d_ranges, uint32_t *d_batch, const int *d_kind, const int *d_part0, const int *d_part1, int n_slots, float momentum,
                      float one_minus_momentum, int observe, void *stream);

/* ---- the PASCAL-VOC detection metric on the device (map_gpu.MapEvaluator): per-class AP and mAP of detection rows that
 * are already in device memory, by the rule of voc_eval.evaluate, integer for integer.  All buffers are the caller's; every launch is on
 * `stream`; nothing is allocated and nothing synchronises.  Rows are (top, left, bottom, right, score, class) fp32; ground truth is the
 * same six columns in FLOAT64 (score ignored) so that every threshold decision is the one the float64 reference makes.  Scores and box
 * coordinates are assumed finite (a NaN has no place in the sort order).  A class column is read as numpy's `astype(int)` reads it
 * (truncation toward zero); a row whose class is outside [0, class_num) belongs to no class: flag 0, counted nowhere.
 * yk_map_append_packed   rows d_src[d_offsets[0] .. d_offsets[n_img]) of n_img images (d_offsets [n_img + 1], device) are copied behind the
 *                        `have` rows of d_rows [capacity][6]; d_img [capacity] receives img_base + the image of every row.  n_new is the
 *                        number of rows (the caller has read it back or knows it).
 * yk_map_append_padded   the same for the padded form yk_decode_py leaves in device memory: d_dets [batch][cap][6] + d_counts [batch]
 *                        (counts are clamped to [0, cap]; n_new = their sum; rows past n_new are not written).
 *                        Both refuse by name instead of overrunning: have + n_new > capacity or > 2^31-1 rows: YK_ERR_ARG.
 * yk_map_workspace_bytes bytes of d_work that yk_map_eval needs for these sizes (sort keys, permutations, scans, rocPRIM's scratch).
 * yk_map_eval            d_img [n_rows] ascending image index of every row (as the append calls write it); d_gt [n_gt_rows][6] float64 with
 *                        d_gt_off [n_img + 1] and d_difficult [n_gt_rows].  Per (image, class) group, detections in descending score
 *                        (-0.0 == +0.0; ties in row order) take the ground-truth box of their image and class with the largest IoU (float64,
 *                        box_iou's operation order, `plus_one` adds 1 to every extent; first index on ties): IoU >= iou_thresh on a
 *                        difficult box: ignored; on a free box: true positive, the box is taken; on a taken box or below: false positive.
 *                        -> d_flags [n_rows] (0 ignored, 1 tp, 2 fp, in row order); per class d_n_gt (non-difficult), d_n_det, d_tp, d_fp
 *                        (int32 [class_num]) and d_ap (float64 [class_num]; NaN where n_gt == 0): the area under the monotone precision
 *                        envelope, or with use_07_metric the 11-point mean (t = k * 0.1, recall >= t - 1e-12); d_map [1] = the mean of the
 *                        non-NaN APs in class order (NaN if there are none).  Deterministic: two runs give the same bits.
 *                        More than 2^31-1 rows, or n_img * (class_num + 1) >= 2^32, or a workspace that is too small: YK_ERR_ARG. */
int yk_map_append_packed(const float *d_src, const int32_t *d_offsets, int n_img, int img_base, long long n_new, float *d_rows, int32_t *d_img,
                         long long have, long long capacity, void *stream);
int yk_map_append_padded(const float *d_dets, const int32_t *d_counts, int batch, int cap, int img_base, long long n_new, float *d_rows,
                         int32_t *d_img, long long have, long long capacity, void *stream);
int yk_map_workspace_bytes(long long n_rows, long long n_gt_rows, int n_img, int class_num, size_t *bytes);
int yk_map_eval(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                const uint8_t *d_difficult, long long n_gt_rows, int class_num, double iou_thresh, int use_07_metric, int plus_one, void *d_work,
                size_t work_bytes, uint8_t *d_flags, int32_t *d_n_gt, int32_t *d_n_det, int32_t *d_tp, int32_t *d_fp, double *d_ap, double *d_map,
                void *stream);

/* ---- the COCO-style metric on the same rows (map_gpu.MapEvaluator.coco_result): AP over n_thr IoU thresholds, n_area
 * object-size ranges and n_rec recall points, by the rule of coco_eval.evaluate (restated from pycocotools' public source; parity with
 * pycocotools' own numbers is unpinned).  Conventions, row formats, class reading and finiteness as yk_map_eval: the caller's buffers,
 * every launch on `stream`, no allocation, no synchronisation, float64 without contraction, no floating-point atomics: two runs give the
 * same bits.  d_iou_thr [n_thr], d_area [n_area][2] (a0, a1), d_rec_thr [n_rec]: float64, device.
 * yk_map_coco_workspace_bytes  bytes of d_work that yk_map_coco_eval needs for these sizes.
 * yk_map_coco_eval   A ground-truth box is IGNORED under range a if it is difficult or its area (bottom - top) * (right - left) is < a0
 *                    or > a1.  Per (image, class) group, detections in descending score (-0.0 == +0.0; ties in row order); only the first
 *                    max_dets take part, the rest get flag 0 under every pair and are counted nowhere.  Per (t, a), each detection in
 *                    that order looks at the boxes of its image and class not yet matched under (t, a) with IoU >= min(t, 1 - 1e-10)
 *                    (box_iou's operation order, no plus_one): the non-ignored one with the largest IoU if any, otherwise the ignored
 *                    one with the largest IoU; the HIGHEST index on equal IoU; the chosen box is matched under (t, a), ignored or not.
 *                    Matched to a non-ignored box: flag 1; to an ignored box: flag 0; unmatched with its own area outside [a0, a1]:
 *                    flag 0; unmatched otherwise: flag 2.  (yk_map_eval's rule takes the best box, taken or not; this one falls back
 *                    to the next free box.)
 *                    Per (class k, t, a), rows of the class in descending score (ties in row order), tp / fp the running counts of
 *                    flags 1 / 2, npig the non-ignored boxes of the class under a: rc = tp / npig, pr = tp / ((fp + tp) + 2^-52),
 *                    pr <- its reverse running maximum; precision[t][r][k][a] = pr at the first row with rc >= d_rec_thr[r] (0 if
 *                    there is none), recall[t][k][a] = the last rc (0 without rows); npig == 0: both -1 (absent).
 *                    -> d_flags [n_area][n_thr][n_rows] (uint8, row order); d_npig [class_num][n_area], d_n_det [class_num] (rows that
 *                    take part), int32; d_precision [n_thr][n_rec][class_num][n_area], d_recall [n_thr][class_num][n_area], float64;
 *                    d_summary [10]: AP, AP at the thresholds == 0.5 and == 0.75, AP of ranges 1, 2, 3, AR, AR of ranges 1, 2, 3 - each
 *                    the mean of the entries > -1 of its slice (range 0 where none is named), NaN if there is none; d_ap_class
 *                    [class_num]: the same mean over t and r for range 0.  The means are added in a fixed order.
 *                    n_thr * n_area > 64, n_rec > 1024, the sizes yk_map_eval refuses, or a workspace that is too small: YK_ERR_ARG. */
int yk_map_coco_workspace_bytes(long long n_rows, long long n_gt_rows, int n_img, int class_num, int n_thr, int n_area, int n_rec, size_t *bytes);
int yk_map_coco_eval(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                     const uint8_t *d_difficult, long long n_gt_rows, int class_num, const double *d_iou_thr, int n_thr, const double *d_area,
                     int n_area, const double *d_rec_thr, int n_rec, int max_dets, void *d_work, size_t work_bytes, uint8_t *d_flags,
                     int32_t *d_npig, int32_t *d_n_det, double *d_precision, double *d_recall, double *d_summary, double *d_ap_class, void *stream);

/* ---- operating points of the same rows (map_gpu.MapEvaluator.sweep / .confusion): precision / recall / F1 over a sweep of
 * confidence thresholds and a confusion matrix at one threshold, by the rule of oppoint.py (the project's own: exact counting, parity with
 * other frameworks' interpolated curves is unpinned).  Conventions, row formats, class reading and finiteness as yk_map_eval: the caller's
 * buffers, every launch on `stream`, no allocation, no synchronisation, float64 without contraction, integer atomics only: two runs give
 * the same bytes.
 * yk_map_sweep_workspace_bytes  bytes of d_work that yk_map_sweep needs for these sizes (two integer histograms [class_num][n_thr]).
 * yk_map_sweep       d_flags [n_rows] and d_n_gt [class_num] are what yk_map_eval wrote for the same rows; d_thr [n_thr] float64, device,
 *                    finite and STRICTLY ASCENDING (the caller's promise: checking it here would need a synchronisation; MapEvaluator.sweep
 *                    checks on the host).  A row is in at threshold t if (double)score >= t.  -> d_tp, d_fp int32 [class_num][n_thr]: the
 *                    in-rows of the class with flag 1 / 2; d_precision = tp / (tp + fp), 1.0 where tp + fp == 0; d_recall = tp / n_gt, NaN
 *                    where n_gt == 0; d_f1 = ((2.0 * p) * r) / (p + r), 0.0 where p + r == 0, NaN where n_gt == 0 (float64
 *                    [class_num][n_thr]); d_best int32 [class_num]: the lowest k with the largest f1, -1 where n_gt == 0; d_mean_f1 float64
 *                    [n_thr]: the f1 of the classes with n_gt > 0 added in ascending class order, divided by their number, NaN if there are
 *                    none; d_best_all int32 [1]: the lowest k with the largest mean, -1 if there are none.
 *                    n_thr outside 1 .. 4096, the sizes yk_map_eval refuses, or a workspace that is too small: YK_ERR_ARG.
 * yk_map_confusion_lds_boxes  the largest (rows taking part + ground-truth boxes) of one image whose coordinates the matching stages in
 *                    LDS; a larger image runs the same loop on global memory: nothing is truncated.
 * yk_map_confusion_workspace_bytes  bytes of d_work that yk_map_confusion needs (one state byte per ground-truth box).
 * yk_map_confusion   d_img, d_gt, d_gt_off, d_difficult as yk_map_eval.  Per image, class-agnostic: the rows with (double)score >=
 *                    conf_thresh and a class in range and every box with a class in range (difficult or not) take part; pairs with IoU
 *                    (box_iou's operation order, `plus_one`) >= iou_thresh are candidates; repeatedly the best pair of a free row and a
 *                    free box is matched: the largest IoU, then the larger score (-0.0 == +0.0), then the lower row, then the lower box.
 *                    -> d_matrix int32 [(class_num + 1)^2], [true][predicted], index class_num = background, zeroed by the call: a pair
 *                    on a non-difficult box counts at [box class][row class], on a difficult box nowhere; an unmatched row at
 *                    [class_num][row class]; an unmatched non-difficult box at [box class][class_num]; d_match int32 [n_rows]: the row's
 *                    box (index into d_gt), -1 unmatched, -2 the row takes no part.
 *                    NaN thresholds, the sizes yk_map_eval refuses, or a workspace that is too small: YK_ERR_ARG. */
int yk_map_sweep_workspace_bytes(long long n_rows, int class_num, int n_thr, size_t *bytes);
int yk_map_sweep(const float *d_rows, const uint8_t *d_flags, long long n_rows, int class_num, const int32_t *d_n_gt, const double *d_thr, int n_thr,
                 void *d_work, size_t work_bytes, int32_t *d_tp, int32_t *d_fp, double *d_precision, double *d_recall, double *d_f1, int32_t *d_best,
                 double *d_mean_f1, int32_t *d_best_all, void *stream);
int yk_map_confusion_lds_boxes(void);
int yk_map_confusion_workspace_bytes(long long n_gt_rows, size_t *bytes);
int yk_map_confusion(const float *d_rows, const int32_t *d_img, long long n_rows, int n_img, const double *d_gt, const int32_t *d_gt_off,
                     const uint8_t *d_difficult, long long n_gt_rows, int class_num, double conf_thresh, double iou_thresh, int plus_one, void *d_work,
                     size_t work_bytes, int32_t *d_matrix, int32_t *d_match, void *stream);

/* ---- anchor k-means with many restarts in one call (datatools.run_kmeans_gpu): datatools.run_kmeans for each of
 * `restarts` initial centroid sets, independently, on boxes d_wh [n][2] (w, h; finite and > 0, which the caller has checked).  Distance
 * 1 - IoU of boxes centred at the origin, float64 in datatools.fake_iou_distance's operation order without contraction; assignment = argmin,
 * the lowest index on a tie; update = sum / count per cluster, summed in an order that (n, k) alone fix (no floating-point atomics), so two
 * calls on the same inputs give the same bits.
 * d_init [restarts][k][2] -> d_centroids [restarts][k][2] (may be the same buffer), d_counts [restarts][k] and d_idx [restarts][n] (or
 * NULL): the assignment of the last iteration, the one the returned centroids are the means of; d_score [restarts]: the mean over the boxes
 * of the best IoU against the returned centroids.  A restart in which a cluster has no member at iteration i (from 0) gets d_empty = i + 1
 * (else 0), NaN in that centroid row and a NaN score, and stops there: its other rows, counts and idx are those of iteration i (numpy
 * would go on and assign every box to the NaN column; that is not reproduced).
 * d_work: 16-byte aligned device scratch of yk_anchor_kmeans_workspace_bytes (needs no device), contents undefined before and after.
 * Every launch is on `stream`; nothing is allocated and nothing synchronises.  k outside 1 .. 32, n outside 1 .. 2^24, restarts outside
 * 1 .. 4096, iters outside 1 .. 1000, a NULL pointer, a d_wh or d_work that is not 16-byte aligned, a workspace that is too small:
 * YK_ERR_ARG, with the argument named in yk_last_error. */
int yk_anchor_kmeans_workspace_bytes(long long n, int k, int restarts, size_t *bytes);
int yk_anchor_kmeans_f64(const double *d_wh, long long n, const double *d_init, int k, int restarts, int iters, double *d_centroids,
                         int32_t *d_counts, double *d_score, int32_t *d_empty, uint8_t *d_idx, void *d_work, size_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_HIP_H_ */
