/*
 * ffp.h — C-ABI of the MI355X-native sliced-inference face pipeline (libffp.so).
 *
 * Drop-in boundary for the hot path  SAHI slice -> YOLO11-pose detect -> per-slice NMS -> SAHI merge ->
 * Real-ESRGAN x4 on crops.  The reference has no native code and no FFI: it reaches this arithmetic through four
 * pip packages called from Python.  Each entry point below names the reference interface it replaces (paths are
 * relative to /root/reference).  Binding shown in INTEGRATION.md (ctypes).
 *
 * Conventions: return 0 (FFP_OK) on success, a positive FFP_ERR_* code otherwise; ffp_last_error() returns a
 * thread-local message.  Callers own every input and output buffer; outputs are caller-allocated.  A handle is
 * bound to one HIP device and one internal stream and is NOT thread-safe (the reference wrapper is not re-entrant
 * either: utils/yolo_wrapper.py keeps per-call state in self._original_predictions).
 * No function here falls back to a CPU implementation: without a gfx950 device every compute call fails.
 */
#ifndef FFP_H
#define FFP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFP_OK 0
#define FFP_ERR_ARG 1      /* bad argument */
#define FFP_ERR_HIP 2      /* HIP runtime / no device */
#define FFP_ERR_WEIGHTS 3  /* malformed FFPW container or missing tensor */
#define FFP_ERR_NOMEM 4
#define FFP_ERR_STATE 5

/* arithmetic type of the convolution path */
#define FFP_PREC_F32 0 /* fp32 activations, v_mfma_f32_32x32x2_f32 (exact-f32 parity mode) */
#define FFP_PREC_F16 1 /* fp16 activations, v_mfma_f32_32x32x16_f16, fp32 accumulate */
#define FFP_PREC_F32X3 2 /* fp32 activations; each product computed as fp16 hi/lo split, 3 fp16 MFMAs (~2^-21 relative),
                            fp32 accumulate: fp32-grade results at ~5x the exact-fp32 MFMA rate */

/* how a caller's HxWx3 uint8 array maps to network channels.
 * AS_BGR reproduces Ultralytics' ndarray path (network channel 0 = array[...,2]) which is what the reference gets,
 * also when SAHI hands it an RGB array (docs sahi/predict.py:103-106 + utils/yolo_wrapper.py:74-80). */
#define FFP_CHAN_AS_BGR 0
#define FFP_CHAN_AS_RGB 1

/* SAHI post-process selectors (docs sahi/predict.py:44-49,150-153) */
#define FFP_PP_NMS 0
#define FFP_PP_GREEDYNMM 1
#define FFP_METRIC_IOU 0
#define FFP_METRIC_IOS 1

/* floats per detection row: x1,y1,x2,y2,score,class, then nkpt*(x,y,conf) */
#define FFP_DET_STRIDE(nkpt) (6 + 3 * (nkpt))

typedef struct ffp_det ffp_det;
typedef struct ffp_sr ffp_sr;

const char* ffp_last_error(void);
int ffp_version(void);
/* number of visible HIP devices (0 and FFP_OK when none) */
int ffp_device_count(int* out_n);
/* The environment switches of this process (csrc/switches.hpp), one line per switch, NUL-terminated:
 *   NAME=effective value <tab> env|default <tab> once|live <tab> accepted values <tab> effect
 * Needs no device. A variable whose value its rule refuses is FFP_ERR_ARG here and from every other call that reads a switch;
 * FFP_ERR_ARG also when cap is too small (the message says how many bytes are needed). */
int ffp_switches(char* out, size_t cap);

/* ---------------------------------------------------------------------------------------------------------
 * host logic
 * ------------------------------------------------------------------------------------------------------- */

/* sahi.slicing.get_slice_bboxes (called through slice_image at docs sahi/predict.py:229-238).
 * Writes up to cap [xmin,ymin,xmax,ymax] rows, row-major over the grid; *out_n = number of slices (may exceed cap,
 * in which case only cap rows were written). */
int ffp_slice_bboxes(int image_h, int image_w, int slice_h, int slice_w, float overlap_h_ratio, float overlap_w_ratio,
                     int32_t* out_xyxy, int cap, int32_t* out_n);

/* How the tile entry points (ffp_rtdetr_infer_tiles, ffp_scrfd_infer_tiles_ex, the sliced predictions) split n items into network batches
 * of at most max_batch >= 1 (a positive number: each engine resolves its own "default" / "one batch" values first): ceil(n / max_batch)
 * chunks whose sizes differ by at most one, the larger ones first (61 at 16: 16, 15, 15, 15). Writes up to cap sizes; *out_n = number of
 * chunks (may exceed cap, in which case only cap sizes were written). n < 0 or max_batch < 1 is FFP_ERR_ARG. */
int ffp_tile_chunks(int n, int max_batch, int32_t* out, int cap, int32_t* out_n);

/* Ultralytics LetterBox(new_shape=imgsz, auto=True, stride=32) geometry for one (h,w) source:
 * out[6] = {new_w, new_h, top, bottom, left, right}.  (inside YOLO.predict, utils/yolo_wrapper.py:74-80) */
int ffp_letterbox_geometry(int h, int w, int imgsz, int32_t* out6);

/* ---------------------------------------------------------------------------------------------------------
 * detector — replaces ultralytics.YOLO(model_path) + .predict(...) behind
 * YOLOv11PoseDetectionModel.load_model / perform_inference (utils/yolo_wrapper.py:47-56, 63-82)
 * ------------------------------------------------------------------------------------------------------- */

/* weights: FFPW container (see weights_io.py) holding the fused conv tensors of YOLO11{n,s,m,l}-pose.
 * arch: 'n', 's', 'm' or 'l' (YOLO11 scales; any other is FFP_ERR_ARG).  nc classes, nkpt keypoints of 3 values.  precision: FFP_PREC_*. */
int ffp_det_create(const void* weights, size_t nbytes, int arch, int nc, int nkpt, int device, int precision,
                   ffp_det** out);
void ffp_det_destroy(ffp_det* d);

/* One batched `predict` over n_tiles crops of one frame (each crop = one `model.predict(source=slice)` call of the
 * reference; the crop [0,0,W,H] is the "standard" full-frame prediction of docs sahi/predict.py:301-314).
 * frame_hwc: HxWx3 uint8 (host).  tiles_xyxy: n_tiles x [x0,y0,x1,y1] in frame pixels.
 * Each crop is letterboxed to imgsz (imgsz <= 0: native — the longer crop side rounded up to a multiple of 32),
 * run through the network, decoded, conf-filtered (score > conf), NMS'ed (IoU > iou suppressed, at most max_det
 * kept, score descending) and mapped back to crop pixels (scale_boxes / scale_coords, clipped to the crop).
 * out_dets: [n_tiles][max_det][FFP_DET_STRIDE(nkpt)] float32, crop-local coordinates, NOT truncated.
 * out_counts: [n_tiles].  round_boxes != 0 applies the `.round()` of older Ultralytics PosePredictor. */
int ffp_det_infer_tiles(ffp_det* d, const uint8_t* frame_hwc, int H, int W, int chan_order,
                        const int32_t* tiles_xyxy, int n_tiles, int imgsz, float conf, float iou, int max_det,
                        int round_boxes, float* out_dets, int32_t* out_counts);

/* Same, with the frame already resident in device memory and outputs written to device memory
 * (all three pointers are device pointers on the handle's device).  Work is enqueued on the handle's stream and
 * the call returns after the stream has drained. */
int ffp_det_infer_tiles_dev(ffp_det* d, const uint8_t* d_frame_hwc, int H, int W, int chan_order,
                            const int32_t* tiles_xyxy_host, int n_tiles, int imgsz, float conf, float iou,
                            int max_det, int round_boxes, float* d_out_dets, int32_t* d_out_counts);

/* The wrapper's conversion on the device, for the tiles of the handle's LAST infer call: boxes int-truncated and
 * clipped like sahi's ObjectAnnotation, then boxes and keypoints shifted by the tile origin
 * (utils/yolo_wrapper.py:137-162 + docs sahi/prediction.py:94-120). d_dets/d_counts as written by
 * ffp_det_infer_tiles_dev. */
int ffp_det_truncate_shift_dev(ffp_det* d, float* d_dets, const int32_t* d_counts, int n_tiles, int max_det, int full_h,
                               int full_w);

/* Raw network output for parity tests: for each tile the inference-mode Pose head output (4+nc+3*nkpt, A_t)
 * float32 = [cx,cy,w,h, class sigmoid.., kpt x,y,sigmoid(v)..] in net-input pixels, written back to back.
 * out_anchor_counts[n_tiles] receives A_t.  out_cap = capacity of out_raw in floats. */
int ffp_det_forward_raw(ffp_det* d, const uint8_t* frame_hwc, int H, int W, int chan_order,
                        const int32_t* tiles_xyxy, int n_tiles, int imgsz, float* out_raw, size_t out_cap,
                        int32_t* out_anchor_counts);

/* ---------------------------------------------------------------------------------------------------------
 * SAHI merge — replaces sahi.postprocess.combine.{NMSPostprocess,GreedyNMMPostprocess}.__call__
 * (constructed at docs sahi/predict.py:254-259, invoked :297,319)
 * ------------------------------------------------------------------------------------------------------- */

/* dets: n rows of `stride` floats (host), first six = x1,y1,x2,y2,score,class (full-frame coords, as SAHI holds
 * them: ints stored as floats).  out: up to n rows of `stride` floats, in SAHI's output order; for GREEDYNMM the box
 * is the union, the score the max, and the remaining columns come from the higher-scored source row.
 * out_src_index[k] = index of that source row.  Runs on `device`. */
int ffp_merge(int device, const float* dets, int n, int stride, int type, int metric, double thr, int class_agnostic,
              float* out, int32_t* out_src_index, int32_t* out_n);

/* Fused get_sliced_prediction (docs sahi/predict.py:142-345) for a host frame: slice grid -> batched predict ->
 * int-truncate + shift (utils/yolo_wrapper.py:137-162, docs sahi/prediction.py:94-120) -> optional full-frame
 * prediction when more than one slice -> merge when more than one box.  out rows as in ffp_merge. */
int ffp_sliced_predict(ffp_det* d, const uint8_t* frame_hwc, int H, int W, int chan_order, int slice_h, int slice_w,
                       float overlap_h_ratio, float overlap_w_ratio, int perform_standard_pred, int imgsz,
                       float conf, float iou, int max_det, int round_boxes, int pp_type, int pp_metric, double pp_thr,
                       int class_agnostic, float* out, int cap, int32_t* out_n);

/* Device-resident variant used by bench.py / multi-GPU: frame and outputs are device pointers. rank/world shard the
 * slice list contiguously (rank r takes slices [r*ceil(n/world), ...)); with world > 1 the call stops after the
 * per-rank detections are written to d_local_dets/d_local_counts (global slice order, fixed cap max_det) so that the
 * caller can all-gather them (RCCL) and finish with ffp_merge_dev. */
int ffp_det_stage_dev(ffp_det* d, const uint8_t* d_frame_hwc, int H, int W, int chan_order, int slice_h, int slice_w,
                      float overlap_h_ratio, float overlap_w_ratio, int perform_standard_pred, int imgsz, float conf,
                      float iou, int max_det, int round_boxes, int rank, int world, float* d_local_dets,
                      int32_t* d_local_counts, int32_t* out_n_local, int32_t* out_n_total);

/* Merge of fixed-cap per-slice detections already on the device: d_dets [n_slices][max_det][stride] (full-frame,
 * truncated+shifted), d_counts[n_slices].  d_out [cap][stride], d_out_n[1] device pointers.
 * *d_out_n receives the UNTRUNCATED number of merged detections; when it exceeds cap only the first cap rows were
 * written and the caller must treat the result as overflowed (ffp_sliced_predict returns FFP_ERR_ARG in that case). */
int ffp_merge_dev(ffp_det* d, const float* d_dets, const int32_t* d_counts, int n_slices, int max_det, int type,
                  int metric, double thr, int class_agnostic, float* d_out, int cap, int32_t* d_out_n);

/* ---------------------------------------------------------------------------------------------------------
 * super-resolution — replaces basicsr RRDBNet + realesrgan.RealESRGANer behind FaceEnhancer
 * (utils/enhancer.py:99-156 construction, :214 `self.upsampler.enhance(image, outscale=self.scale)`)
 * ------------------------------------------------------------------------------------------------------- */

/* weights: FFPW container with RRDBNet tensors.  scale 4 (x4plus) or 2 (x2plus, pixel-unshuffle front).
 * half != 0 -> FFP_PREC_F16 (the reference's GPU default, utils/enhancer.py:22), else fp32. */
int ffp_sr_create(const void* weights, size_t nbytes, int scale, int num_block, int device, int half, ffp_sr** out);
void ffp_sr_destroy(ffp_sr* s);

/* RealESRGANer.enhance for one 3-channel uint8 BGR image (host). out_bgr: (scale*h) x (scale*w) x 3 uint8.
 * tile <= 0: whole image in one pass; else tiles of `tile` px padded by tile_pad (clipped). */
int ffp_sr_enhance(ffp_sr* s, const uint8_t* bgr_hwc, int h, int w, int tile, int tile_pad, int pre_pad,
                   uint8_t* out_bgr);

/* The same for an image resident in device memory, output written to device memory ((scale*h) x (scale*w) x 3, tightly
 * packed): the enhance-first ordering (pipeline_v4_yolo/app_yolo_full.py:87-123 — FaceEnhancer.enhance_image on the
 * whole picture, utils/enhancer.py:189-235, then get_sliced_prediction on the result) without a host round trip. */
int ffp_sr_enhance_dev(ffp_sr* s, const uint8_t* d_bgr_hwc, int h, int w, int tile, int tile_pad, int pre_pad, uint8_t* d_out_bgr);

/* RealESRGANer.enhance(img, outscale, alpha_upsampler) of realesrgan 0.3.0 for every layout it accepts (reference call
 * utils/enhancer.py:214; the layout rules are the caller's, compat/utils/enhancer.py::enhance_layout):
 *   img: h x w x channels, 8-bit (bits 8) or 16-bit (bits 16) elements. channels 1 = mode 'L' (gray replicated to RGB,
 *        result BGR2GRAY), 3 = BGR, 4 = BGRA (mode 'RGBA': BGR through the network, alpha by alpha_mode).
 *   max_range: 255 or 65535 (the caller's `np.max(img) > 256` rule; 65535 needs bits 16). Pixels are divided by it, the
 *        result is rint(v * max_range); output elements are uint16 exactly when max_range == 65535, else uint8.
 *   alpha_mode (channels 4): FFP_SR_ALPHA_REALESRGAN = the alpha plane replicated to RGB through the network in the same
 *        batch as the colour image, result BGR2GRAY; FFP_SR_ALPHA_LINEAR = cv2.resize(alpha, INTER_LINEAR) in float32.
 *   out_h x out_w: (scale*h) x (scale*w), or any other size for cv2.resize(..., INTER_LANCZOS4) of the result (outscale).
 *   out: out_h x out_w x channels. Any other combination (channels 2, bits 8 with max_range 65535, a size of 0, ...) is
 *   FFP_ERR_ARG before anything is launched. */
#define FFP_SR_ALPHA_REALESRGAN 0
#define FFP_SR_ALPHA_LINEAR 1
int ffp_sr_enhance_ex(ffp_sr* s, const void* img, int h, int w, int channels, int bits, int max_range, int alpha_mode, int out_h,
                      int out_w, int tile, int tile_pad, int pre_pad, void* out);

/* n independent images in one ragged batch (one launch per layer for all of them). */
int ffp_sr_enhance_batch(ffp_sr* s, int n, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws, int tile,
                         int tile_pad, int pre_pad, uint8_t* const* outs);

/* Crops gathered on the device from a resident frame (utils/visualization.py:185-223 crop semantics: int box,
 * clamped to the frame, an empty crop is skipped), each enhanced like FaceEnhancer.enhance_image does
 * (utils/enhancer.py:189-235 -> RealESRGANer.enhance with the enhancer's tile setting: tile 400 / tile_pad 10 at
 * utils/enhancer.py:21,135-142; tile <= 0: one pass per crop), outputs packed back to back in d_out (device), byte
 * offsets in out_offsets (host, n+1 entries; a skipped crop has out_offsets[i+1] == out_offsets[i]).
 * frame is BGR. boxes_xyxy: host int32 [n][4]. */
int ffp_sr_enhance_crops_dev(ffp_sr* s, const uint8_t* d_frame_bgr, int H, int W, const int32_t* boxes_xyxy, int n, int tile,
                             int tile_pad, uint8_t* d_out, size_t out_cap, int64_t* out_offsets);

/* Same, but returns once the work is enqueued on the enhancer's own HIP stream; ffp_sr_wait() blocks until d_out is
 * complete. Lets a caller overlap frame i's super-resolution with frame i+1's detection (the detector handle has its
 * own stream). d_frame and d_out must stay untouched until ffp_sr_wait (or the next call on the handle) returns. */
int ffp_sr_enhance_crops_dev_async(ffp_sr* s, const uint8_t* d_frame_bgr, int H, int W, const int32_t* boxes_xyxy, int n, int tile,
                                   int tile_pad, uint8_t* d_out, size_t out_cap, int64_t* out_offsets);
int ffp_sr_wait(ffp_sr* s);
/* Crops of SEVERAL resident frames (all H x W) as one ragged batch: frame_of_box[i] selects d_frames[...] for box i
 * (boxes of one frame must be contiguous). More pixels per launch = better use of the chip when a frame yields few crops. */
int ffp_sr_enhance_crops_multi_dev_async(ffp_sr* s, int n_frames, const uint8_t* const* d_frames, const int32_t* frame_of_box,
                                         int H, int W, const int32_t* boxes_xyxy, int n, int tile, int tile_pad, uint8_t* d_out,
                                         size_t out_cap, int64_t* out_offsets);

/* Engine state for tests and monitoring. The enhancer lays its network out for a CAPACITY (pixels / tiles), not for a list
 * of crop sizes: out_plans_built counts the layouts built so far (a stream of frames with ever-changing crop sizes must
 * not grow it), out_last_graph tells whether the last call replayed a captured hipGraph (1) or launched eagerly (0). */
int ffp_sr_plan_state(ffp_sr* s, int32_t* out_plans_built, int32_t* out_last_graph);
/* The body of RRDBNet (the 345 convs of the residual dense blocks constructed at utils/enhancer.py:121-128) as ONE persistent launch
 * with per-tile dependency counters (1; fp16 only) or as one launch per layer (0, the default: the faster of the two on MI355X as
 * measured in round 4, profiles/r04_sr_batch_sweep.txt; FFP_TRUNK=1 in the environment makes 1 the default). Results are bit-identical
 * either way; each form is the other's parity oracle and A/B partner. Drops the resident plans. */
int ffp_sr_set_fused_body(ffp_sr* s, int on);
/* Device memory a handle holds: the packed weights and the resident plans (activations + tables; the detector keeps at most 8 plans
 * and FFP_DET_PLAN_GIB (default 64) GiB of them, the enhancer at most 4 capacity buckets, least recently used first out). The
 * reference holds one torch module per model (utils/yolo_wrapper.py:47-61, utils/enhancer.py:156) and lets torch's caching
 * allocator grow; here a caller that switches image_size or batch shapes can see — and bound — what stays resident. */
int ffp_sr_mem_bytes(ffp_sr* s, uint64_t* out_weight_bytes, uint64_t* out_plan_bytes, int32_t* out_plans_resident);
/* Release every resident plan of a handle now (activations, tables, captured graphs; the packed weights stay). The next call lays its plan out
 * again (tens of ms: layout, tuning, graph capture). The counterpart of `del model; torch.cuda.empty_cache()` around the reference's modules. */
int ffp_det_drop_plans(ffp_det* d);
int ffp_sr_drop_plans(ffp_sr* s);
/* The detector's plan bytes are the blocks its plans hold, not the sum of its tensors: with buffer reuse on (the default, see
 * ffp_det_set_buffer_reuse) activation tensors whose lifetimes do not overlap share bytes, and this figure is smaller by what they share. */
int ffp_det_mem_bytes(ffp_det* d, uint64_t* out_weight_bytes, uint64_t* out_plan_bytes, int32_t* out_plans_resident);
/* How the activation tensors of the detector's plans are stored. The reference holds one torch module per model
 * (utils/yolo_wrapper.py:47-61) and leaves activations to torch's caching allocator, which hands a freed tensor's block to the next
 * one; here a plan's pointers are fixed when it is laid out, so reuse is decided then, from the order the steps are built in.
 * mode 0: every tensor has its own allocation (parity oracle and A/B partner); 1 (default; env FFP_DET_ARENA=0|1|2 sets another
 * default): a tensor's bytes go back to the plan's pool behind its last reader and may back a later tensor; 2: as 1, and each
 * released range is then overwritten with 0xFF bytes (NaN in fp32 and fp16) — a diagnostic: a step that reads a tensor after its
 * declared end reads NaN, whether or not the range was reused. Results are bit-identical in all modes. Drops the cached plans.
 * FFP_ERR_ARG for any other mode. */
int ffp_det_set_buffer_reuse(ffp_det* d, int mode);
/* Activation storage of the resident detector plans, summed (the part of ffp_det_mem_bytes' plan bytes that torch's caching allocator
 * would own in the reference, utils/yolo_wrapper.py:47-61): bytes held for activation tensors; what mode 0 would hold (the sum of
 * every tensor's size); and the maximum, over the order the steps are built in, of the bytes live at once — the floor of any
 * placement. Any out pointer may be null. */
int ffp_det_mem_detail(ffp_det* d, uint64_t* out_activation_bytes, uint64_t* out_no_reuse_bytes, uint64_t* out_peak_live_bytes);
/* (test hook, no counterpart in the reference) Over the resident detector plans: the 0xFF fill steps their step lists hold, and the tensors
 * whose range reached the free list while they were built. Mode 2 holds exactly one fill per freed range, modes 0 and 1 none — what
 * makes mode 2 a diagnostic and not a second mode 1. */
int ffp_det_fill_steps(ffp_det* d, int32_t* out_fill_steps, int32_t* out_ranges_freed);
/* hipGraph state of the plan the detector's last call ran: 1 replayed a captured graph, 0 not captured yet (first runs of a
 * plan are eager), -1 capture failed and the plan keeps launching eagerly (also reported once on stderr). */
int ffp_det_graph_status(ffp_det* d, int32_t* out_state);
/* Parallel branches in the detector's captured launch graph (no counterpart in the reference, which runs one layer at a time:
 * /root/reference/utils/yolo_wrapper.py:74-80 hands the whole forward pass to one call). mode 0 (default): one stream;
 * 1: the head's nine towers and C3k's side convs run as parallel graph branches (3-5 % faster when the detector has the device
 * to itself, slower when an enhancer stream runs beside it); 2 / 3: coarser variants for A/B. Drops the cached plans. */
int ffp_det_set_lanes(ffp_det* d, int mode);
/* Skip the box and keypoint towers of the pose head for items (slices, the full-frame pass) in which no anchor's class score passes conf
 * (no counterpart in the reference, whose model.predict at /root/reference/utils/yolo_wrapper.py:74-80 runs every tower on every slice):
 * decode reads an anchor's box values only when its score passes, NMS reads keypoints only of boxes it keeps, so such an item gets
 * nothing out of those towers. Results are bit-identical with the gate on and off. on = 1 is the default (env FFP_DET_GATE=0 sets the
 * default to off). Drops the cached plans. */
int ffp_det_set_gate(ffp_det* d, int on);
/* Items whose box and keypoint towers ran in the handle's last inference call, and the items of that call (gate off, and the raw head
 * output of ffp_det_forward_raw: all of them). */
int ffp_det_last_active(ffp_det* d, int32_t* out_active, int32_t* out_items);
/* Stream interop for the multi-GPU exchange (no counterpart in the reference, which is single-device:
 * /root/reference/pipeline_v4_yolo/app_yolo_sahi.py:136): work enqueued on the handle's stream AFTER this call waits for `hip_event`
 * (a hipEvent_t of the same process, e.g. torch.cuda.Event.cuda_event recorded behind the RCCL all-gather of the boxes) — the
 * merge that follows is ordered behind the collective without the host waiting for either. */
int ffp_det_stream_wait_event(ffp_det* d, void* hip_event);

/* ---------------------------------------------------------------------------------------------------------
 * single-operator entry points (layer-wise parity tests; host NHWC fp32 in/out, computed on `device` in `precision`)
 * ------------------------------------------------------------------------------------------------------- */

/* cv2.resize(src, (out_w, out_h), interpolation=INTER_LANCZOS4) — the outscale step of RealESRGANer.enhance (reference call
 * utils/enhancer.py:214) alone. src: h x w x channels (1, 3, 4), bits 8 (uint8) or 16 (uint16); dst: out_h x out_w x channels
 * of the same type. Same size is a copy. 8-bit: int16 weights (x2048), int32 sums, (v + 2^21) >> 22 saturated; 16-bit: float
 * weights, float sums, rint saturated. Weight tables are built on the host (sin / cos in double). */
int ffp_op_resize_lanczos4(int device, const void* src, int h, int w, int channels, int bits, int out_h, int out_w, void* dst);

/* y = act(conv2d(x, w) + b) [* s1 + res]; x: [n][h][w][cin] fp32 NHWC; w: OIHW fp32 (groups: 1 or cin==cout
 * depthwise); k in {1,3}; stride in {1,2}; pad = k/2; act: 0 none, 1 SiLU, 2 LeakyReLU(0.2); up: nearest x2 of x
 * before the conv (0/1); res: optional residual [n][ho][wo][cout] (NULL: none). y: [n][ho][wo][cout] fp32. */
int ffp_op_conv2d(int device, int precision, const float* x, int n, int h, int w, int cin, const float* wt,
                  const float* bias, int cout, int k, int stride, int groups, int act, int up, const float* res,
                  float res_scale, float* y);

/* ---------------------------------------------------------------------------------------------------------
 * WIDER FACE evaluation (host arrays in, integer results out; float64 throughout like the reference's numpy code)
 * ------------------------------------------------------------------------------------------------------- */

/* "Official" protocol: /root/reference/eval/eval_official_widerface.py:302-375 (`_image_eval` + `_img_pr_info`, with the
 * WiderFace-Evaluation `bbox_overlaps` it imports at :24-33) for all images of one difficulty setting, summed as in
 * `_evaluate_setting` :397-443. preds [pred_off[n_img]][5] = x, y, w, h, score in the order the caller evaluates them; gts
 * [gt_off[n_img]][4] = x, y, w, h; evaluate[g] = 1: the setting evaluates this face (the reference's `ignore[keep_index-1] = 1`),
 * 0: a proposal matching it is dropped. Images with no prediction or no face contribute nothing (:430-431). out_counts
 * [thresh_num][2] = {valid proposals, matched faces} at the last prediction with score >= 1 - (t+1)/thresh_num — the
 * reference's pr_curve before `_dataset_pr_info` (counts are integers; precision / recall / AP are the caller's three lines). */
int ffp_eval_wider_pr(int device, const double* preds, const int64_t* pred_off, const double* gts, const int64_t* gt_off, const uint8_t* evaluate,
                      int n_img, double iou_thr, int thresh_num, int64_t* out_counts);

/* "Dual" protocol matching: /root/reference/eval/eval_dual.py:272-291 (`calculate_iou`) and :369-399 of `evaluate_single_set`.
 * faces [face_off[n_img]][4] in annotation order, valid[f] = 1: face belongs to the evaluated category set, 0: ignored face.
 * out_flags [pred_off[n_img]]: 1 true positive, 0 false positive, 2 not counted (overlaps an ignored face, or the image has no
 * valid face and is skipped :354-355). */
int ffp_eval_dual_match(int device, const double* preds, const int64_t* pred_off, const double* faces, const int64_t* face_off, const uint8_t* valid,
                        int n_img, double iou_thr, int32_t* out_flags);

/* COCO bbox evaluation: pycocotools 2.0.x `COCOeval(cocoGt, cocoDt, 'bbox')` `.evaluate()` + `.accumulate()` (cocoeval.py, with
 * maskApi.c `bbIou`) for a whole dataset, bit-identical to it; `summarize()` stays with the caller (numpy's pairwise mean). A unit is an
 * (image, category) pair; the n_cat * n_img units come in evalImgs order (category-major, image ids sorted). dets [det_off[U]][7] =
 * x, y, w, h, score, area, id in loadRes order per unit (ids > 0, scores not NaN); gts [gt_off[U]][8] = x, y, w, h, area, iscrowd,
 * ignore, id in annotation order per unit (ignore = iscrowd after _prepare; a crowd must be ignored). Params exactly as the host holds
 * them (never recomputed here): iou_thrs [T], rec_thrs [R], area_rng [A][2], max_dets [M] ascending. Outputs as accumulate builds
 * them, -1 where it leaves -1: precision / scores [T][R][K][A][M], recall [T][K][A][M]. Optional (NULL = skip), the evalImgs match
 * arrays per area a and threshold t: dt_matches / dt_ignore [A][T][ndc] (ndc = sum over units of min(#dets, max_dets[M-1]); a
 * unit's dets in score order from its cut offset), gt_matches [A][T][gt_off[U]] and gt_ignore [A][gt_off[U]] (a unit's GTs in that
 * area's "ignored last" order). Malformed offsets, sizes or ids: FFP_ERR_ARG, nothing is truncated. */
int ffp_eval_coco_bbox(int device, int n_img, int n_cat, const double* dets, const int64_t* det_off, const double* gts, const int64_t* gt_off,
                       const double* iou_thrs, int n_iou, const double* rec_thrs, int n_rec, const double* area_rng, int n_area,
                       const int32_t* max_dets, int n_max_dets, double* precision, double* recall, double* scores, double* dt_matches,
                       uint8_t* dt_ignore, double* gt_matches, uint8_t* gt_ignore);

/* ---------------------------------------------------------------------------------------------------------
 * JPEG at the file boundaries
 * ------------------------------------------------------------------------------------------------------- */

/* Replaces `cv2.imwrite(path, img)` / `cv2.imwrite(path, img, [cv2.IMWRITE_JPEG_QUALITY, q])` for .jpg paths
 * (/root/reference/utils/visualization.py:218-221 crops, utils/enhancer.py:273-278 enhanced crops, quality 95): baseline JFIF,
 * YCbCr 4:2:0, integer DCT, Annex K Huffman tables — byte-for-byte the file libjpeg-turbo (OpenCV's and Pillow's codec) writes.
 * img: h x w x 3 uint8, bgr = 1 for OpenCV's channel order (0: RGB). out: caller's buffer of `cap` bytes; *out_size = file size
 * (also set when cap is too small: FFP_ERR_ARG, call again). _dev: the image is already in device memory (row pitch in bytes),
 * e.g. a crop inside the buffer ffp_sr_enhance_crops_dev filled — only the compressed bytes cross PCIe. */
int ffp_jpeg_encode(int device, const uint8_t* img, int h, int w, int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_size);
int ffp_jpeg_encode_dev(int device, const uint8_t* d_img, int h, int w, int64_t row_stride, int bgr, int quality, uint8_t* out, int64_t cap,
                        int64_t* out_size);
/* The per-crop loop of enhance_face_crops_batch (/root/reference/utils/enhancer.py:344-391: one cv2.imwrite per enhanced crop) as ONE
 * pass over n device-resident images: image i is hs[i] x ws[i] x 3 at d_base + offsets[i] (row pitch strides[i], or ws[i]*3 when
 * strides is NULL) — e.g. the out_offsets layout of ffp_sr_enhance_crops_dev with hs/ws = 4 x the crop sizes. File i is
 * out[out_offsets[i] .. out_offsets[i+1]) (out_offsets has n+1 entries and is filled even when cap is too small: FFP_ERR_ARG). */
int ffp_jpeg_encode_batch_dev(int device, const uint8_t* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                              int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_offsets);

/* Replaces `cv2.imread(path)` for .jpg files (/root/reference/utils/enhancer.py:254, utils/visualization.py:200, and the image
 * load inside sahi's get_sliced_prediction): baseline / extended-sequential 8-bit JFIF, 4:4:4 / 4:2:2 / 4:2:0 or grayscale, restart
 * intervals; libjpeg's default reconstruction (integer IDCT, triangle chroma upsampling, fixed-point YCbCr -> RGB), pixel-identical
 * to what libjpeg-turbo returns. Huffman decoding (see ffp_jpeg_decode_stats below), IDCT, upsampling and colour conversion all run
 * on the device; the host parses the markers. Progressive / arithmetic-coded files: FFP_ERR_ARG. ffp_jpeg_info reads the header only. out: h*w*3 bytes, BGR
 * when bgr = 1 (cv2's order; grayscale files give three equal channels like IMREAD_COLOR). _dev writes into device memory (row
 * pitch in bytes): the frame is ready for ffp_det_infer_tiles_dev; what crosses PCIe is the file itself (through pinned staging kept in a
 * pool), neither coefficients nor pixels are ever materialised on the host. One file is decoded as a batch of one (the routine behind
 * ffp_jpeg_decode_batch_dev below), so the batch's rules hold: when the call fails — a file the markers refuse, a buffer that is too small, a
 * damaged stream that the host decoder refuses too — the output region (out / d_out) is untouched; and one decode costs TWO stream
 * synchronisations (the entropy decoder's verdict comes down before the reconstruction is queued). Calls on different threads run side by side. */
int ffp_jpeg_info(const uint8_t* data, int64_t n, int32_t* out_h, int32_t* out_w, int32_t* out_ncomp);
int ffp_jpeg_decode(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* out, int64_t cap);
int ffp_jpeg_decode_dev(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* d_out, int64_t row_stride, int64_t cap);
/* Since round 3 the Huffman decoding of ffp_jpeg_decode* runs on the device as well (csrc/jpeg_huff.hip: self-synchronising parallel
 * decoding; the file crosses PCIe as it is). Streams the device decoder flags — damaged data, anything libjpeg treats specially — are
 * decoded again by the host decoder (FFP_JPEG_HOST_HUFFMAN=1 forces it for every file). Counters since the library was loaded:
 * files decoded on the device, files that fell back to the host decoder, extra synchronisation rounds (beyond the one queued blindly). */
int ffp_jpeg_decode_stats(int64_t* device_decodes, int64_t* host_fallbacks, int64_t* extra_sync_rounds);
/* The read side of the per-crop loop of enhance_face_crops_batch (/root/reference/utils/enhancer.py:344-391: one cv2.imread per crop,
 * utils/enhancer.py:254) as ONE pass: n JPEG files -> n images in device memory. File i is datas[i][0 .. sizes[i]); image i is written at
 * d_base + offsets[i] with row pitch strides[i] bytes (NULL or 0: packed, ws[i]*3). hs/ws (out, n entries) are filled from the headers.
 * status (out, n entries): 0 decoded on the device, 1 decoded by the host decoder, < 0 minus the FFP_ERR_* of a file that was not decoded
 * (progressive, arithmetic, not a JPEG, damaged beyond the host decoder): its region is left untouched. The call returns FFP_OK when the
 * arguments were valid, even if files failed; ffp_last_error then names the first failed index and why. A null array, n < 0, or a readable
 * file's region that does not lie inside cap: FFP_ERR_ARG before anything is launched. n == 0: FFP_OK. The number of kernel launches and
 * stream synchronisations does not depend on n (csrc/jpeg_batch_plan.hpp: every file owns whole workgroups; one upload, one memset, one
 * launch per stage, one download of all files' scalars); batches whose streams would pass 256 MiB are cut into sub-batches.
 * ffp_jpeg_decode_batch: the same into n host buffers of caps[i] bytes (a readable file whose buffer is too small: FFP_ERR_ARG).
 * ffp_jpeg_decode_stats keeps counting files; FFP_JPEG_HOST_HUFFMAN=1 sends every file of a batch to the host decoder.
 * ffp_jpeg_decode_batch_stats: calls of these two entries since load, kernel launches and stream synchronisations of the latest one
 * (ffp_jpeg_decode / ffp_jpeg_decode_dev do not move them). Batches on different threads run side by side, each with a pooled workspace. */
int ffp_jpeg_decode_batch_dev(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr,
                              uint8_t* d_base, const int64_t* offsets, const int64_t* strides, int64_t cap,
                              int32_t* hs, int32_t* ws, int32_t* status);
int ffp_jpeg_decode_batch(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr,
                          uint8_t* const* outs, const int64_t* caps, int32_t* hs, int32_t* ws, int32_t* status);
int ffp_jpeg_decode_batch_stats(int64_t* batches, int64_t* launches_last_batch, int64_t* syncs_last_batch);

/* The EXIF orientation, applied where the pixels already are. The reference applies the tag on every read: cv2.imread does
 * (/root/reference/utils/visualization.py:95,198, utils/enhancer.py:254, every app), and so does read_image_as_pil(..., exif_fix=True) behind
 * get_sliced_prediction (sahi/predict.py:608). ffp_exif_orientation finds the tag in a file's bytes (csrc/exif.hpp; host only, no device): a
 * JPEG's first APP1 segment that starts with "Exif\0\0" in front of SOS, or a PNG's first eXIf chunk, holds a TIFF header ("II" / "MM", 42, the
 * offset of IFD0) and IFD0, whose entry 0x0112 (SHORT or LONG, count 1) is the value. *orientation is 1..8; everything that is not a well-formed
 * tag gives 1 (as stored): no tag, a value outside 1..8, a truncated segment, an IFD offset or entry count that leaves the segment, a file that is
 * neither kind. Nothing outside data[0 .. n) is read. FFP_ERR_ARG only for a null argument.
 * ffp_jpeg_decode_oriented / _oriented_dev / _batch_oriented_dev are ffp_jpeg_decode / _dev / _batch_dev with an orientation per file: 0 (or a
 * null `orientations` array) the file's own tag, 1..8 that value, anything else FFP_ERR_ARG. It is one decoding routine: a file of orientation
 * 2..8 is reconstructed into a pooled workspace image and turned into its region by the orient kernel below — at most ONE more launch per
 * sub-batch, whatever n is, none when every file is 1 (such a batch queues exactly what ffp_jpeg_decode_batch_dev queues), and
 * ffp_jpeg_decode_batch_stats counts it. row_stride / strides, cap, *out_h / *out_w, hs and ws describe the ORIENTED image (for 5..8 the file's
 * width is the image's height). The rest of the contract holds unchanged: a file that is not decoded leaves its region untouched. */
int ffp_exif_orientation(const uint8_t* data, int64_t n, int32_t* orientation);
int ffp_jpeg_decode_oriented(int device, const uint8_t* data, int64_t n, int bgr, int orientation, uint8_t* out, int64_t cap, int32_t* out_h, int32_t* out_w);
int ffp_jpeg_decode_oriented_dev(int device, const uint8_t* data, int64_t n, int bgr, int orientation, uint8_t* d_out, int64_t row_stride, int64_t cap,
                                 int32_t* out_h, int32_t* out_w);
int ffp_jpeg_decode_batch_oriented_dev(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr, const int32_t* orientations,
                                       uint8_t* d_base, const int64_t* offsets, const int64_t* strides, int64_t cap,
                                       int32_t* hs, int32_t* ws, int32_t* status);

/* ---------------------------------------------------------------------------------------------------------
 * PNG at the file boundaries (written and read on the device; palette, sub-byte, gray+alpha and interlaced files stay with the host)
 * ------------------------------------------------------------------------------------------------------- */

/* Replaces `cv2.imwrite(path, img)` for .png paths (/root/reference/pipeline_v1_detection_first/app_v1.py:39, app_sahi_detection.py:31,
 * app_enhancer.py:43 and pipeline_v2_enhancement_first/app_v2.py:82 `visual_*.png`; app_v2.py:105-106 the enhanced frame;
 * utils/enhancer.py:273-278 enhanced crops whose path is not .jpg; the 16-bit results of RealESRGANer.enhance). The file is written on
 * the device and only the file crosses PCIe: signature, IHDR, IDAT..., IEND; colour type gray (channels 1), RGB (3) or RGBA (4) at
 * bit_depth 8 or 16 (samples in host byte order in memory, big-endian in the file); no interlace, palette or ancillary chunk. bgr = 1:
 * the image is BGR(A), OpenCV's order. One filter byte per row by libpng's minimum sum of absolute differences (signed bytes; ties to the
 * lowest type). One zlib stream: the filtered bytes are cut into segments of ffp_png_segment_bytes() bytes, each compressed on its own
 * (LZ77 inside the segment; fixed or dynamic Huffman code, whichever is smaller; stored when it does not shrink) into one IDAT chunk,
 * every segment but the last ending with an empty stored block; the Adler-32 is a last 4-byte IDAT. level 0: stored blocks
 * throughout; every level >= 1 is the same one compressor. The contract is what a PNG reader decodes, not libpng's bytes; the same
 * pixels always give the same file. ffp_png_bound: worst-case file size (-1 for a geometry that is not written). *out_size is set also
 * when cap is too small (FFP_ERR_ARG, call again). _dev: the image is in device memory (row pitch in bytes). */
int64_t ffp_png_bound(int h, int w, int channels, int bit_depth);
int ffp_png_segment_bytes(void);
int ffp_png_encode(int device, const void* img, int h, int w, int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_size);
int ffp_png_encode_dev(int device, const void* d_img, int h, int w, int channels, int bit_depth, int64_t row_stride, int bgr, int level, uint8_t* out, int64_t cap,
                       int64_t* out_size);
/* The per-crop `cv2.imwrite` loop of enhance_face_crops_batch (/root/reference/utils/enhancer.py:344-391) for .png outputs as ONE pass,
 * with the layout of ffp_jpeg_encode_batch_dev: image i is hs[i] x ws[i] at d_base + offsets[i] bytes (row pitch strides[i], or the
 * packed row when strides is NULL); file i is out[out_offsets[i] .. out_offsets[i+1]) (n+1 entries, filled even when cap is too small:
 * FFP_ERR_ARG). File i is byte for byte what ffp_png_encode_dev writes for image i. */
int ffp_png_encode_batch_dev(int device, const void* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                             int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_offsets);

/* Reading PNG (csrc/png_dec.cpp, png_dec.hip): replaces `cv2.imread(path)` for .png paths (the reference's utils/enhancer.py:254 and
 * utils/visualization.py:95,198) and the read behind `get_sliced_prediction(image=temp_enhanced_path)`
 * (pipeline_v2_enhancement_first/app_v2.py:112). Decoded: colour types 0, 2 and 6 (gray, RGB, RGBA) at bit depth 8 or 16, not interlaced,
 * h, w >= 1; palette, sub-byte depths, gray with alpha, interlace and a file without IDAT are FFP_ERR_ARG naming the field, before
 * anything is launched. Ancillary chunks (tRNS, gAMA, iCCP, eXIf, ...) are skipped unread. Output: h x w x channels samples of the
 * file's depth (uint8, or uint16 in host byte order), what IMREAD_UNCHANGED gives; the first three channels are BGR when bgr = 1. cap too
 * small is FFP_ERR_ARG. A file whose IDAT chunks each inflate on their own (every file ffp_png_encode* writes: one deflate segment per
 * IDAT, the Adler-32 in a last 4-byte IDAT) is inflated on the device, one wavefront per IDAT; the verdict is taken per file from the
 * bytes alone (every chunk decodes by itself, uses exactly its bytes, no match reaches before its own output, the lengths add up and the
 * Adler-32 matches), never from a marker. Every other file is inflated on the host by the same code and unfiltered on the device.
 * flags: FFP_PNG_DEC_SERIAL forces the host inflate for every file (A/B partner, parity oracle). A wrong CRC (IHDR, IDAT, IEND), a wrong
 * Adler-32, a stream that ends early and one that ends late are FFP_ERR_ARG with the message saying which. ffp_png_info: header only,
 * no device. _dev: the frame stays in device memory (row pitch in bytes, 0 = packed) for the ffp_*_dev entries.
 * ffp_png_decode_stats: files decoded by each route since the library was loaded. ffp_png_unfilter_geometry: test hook, the rows one
 * workgroup pass covers and the pixels of one of its steps. */
#define FFP_PNG_DEC_SERIAL 1
int ffp_png_info(const uint8_t* data, int64_t n, int32_t* h, int32_t* w, int32_t* channels, int32_t* bit_depth);
int ffp_png_decode(int device, const uint8_t* data, int64_t n, int bgr, int flags, void* out, int64_t cap);
int ffp_png_decode_dev(int device, const uint8_t* data, int64_t n, int bgr, int flags, void* d_out, int64_t row_stride, int64_t cap);
int ffp_png_decode_stats(int64_t* parallel_decodes, int64_t* serial_decodes);
int ffp_png_unfilter_geometry(int32_t* rows_per_group, int32_t* cols_per_step);

/* ---------------------------------------------------------------------------------------------------------
 * Detection overlays drawn on the device (between ffp_jpeg_decode_dev / ffp_png_decode_dev and ffp_jpeg_encode_dev / ffp_png_encode_dev)
 * ------------------------------------------------------------------------------------------------------- */

/* Replaces the drawing of draw_detections / draw_detections_on_image (/root/reference/utils/visualization.py:78-183: cv2.rectangle,
 * cv2.putText, and draw_keypoints_and_skeleton's cv2.line / cv2.circle, :37-76) on a frame that stays in device memory: an ORDERED list of
 * primitives is painted in place, in list order (painter's order: where two overlap, the later one wins), into an h x w x 3 uint8 image
 * with a row pitch in bytes; the image's base may have any byte alignment (a view inside a larger buffer). Two kinds:
 *   FFP_OVERLAY_RECT   inclusive corners (x0, y0)..(x1, y1), partly or wholly outside the image if they like; width 0 fills it, width >= 1
 *                      paints the pixels within `width` of an edge (a frame; a rectangle under 2*width wide or high is therefore filled).
 *   FFP_OVERLAY_STAMP  an x1 x y1 (width x height) 8-bit mask laid with its top-left corner at (x0, y0): mask pixel (i, j) is byte
 *                      mask_off + j*width + i of the mask pool (`width` holds the mask's row pitch), and every covered pixel and channel becomes
 *                      t = dst*(255 - m) + c*m + 128; dst = ((t >> 8) + t) >> 8  — Pillow's blend: m == 0 keeps dst, m == 255 gives c.
 * color: three bytes in the image's channel order. The result is a function of the image and the list alone. Bytes between w*3 and the
 * row pitch are never written, and a tile no primitive touches is neither read nor written.
 * Everything is checked before anything is launched, and a refused call (FFP_ERR_ARG) leaves the image untouched: a null list or image,
 * n < 0 or n > FFP_OVERLAY_MAX_PRIMS, row_stride < w*3, an unknown kind, a negative frame width, a stamp with a negative size or offset or a
 * pitch below its width, a stamp whose mask does not lie inside mask_bytes (at most 2^31 - 1). n == 0: FFP_OK, nothing is launched.
 * The list and the pool go up through a pooled workspace, so calls on different threads run side by side.
 * ffp_overlay_draw: the same on a host image (its w*3 bytes of every row go up, are drawn on and come down), for tests and small callers. */
#define FFP_OVERLAY_RECT 0
#define FFP_OVERLAY_STAMP 1
#define FFP_OVERLAY_MAX_PRIMS 1048576
#define FFP_OVERLAY_PRIM_BYTES 32
typedef struct ffp_overlay_prim {
  int32_t kind;     /* FFP_OVERLAY_RECT / FFP_OVERLAY_STAMP */
  int32_t x0, y0;   /* RECT: first corner. STAMP: where the mask's top-left corner lies (may be negative) */
  int32_t x1, y1;   /* RECT: last corner, inclusive. STAMP: the mask's width and height */
  int32_t width;    /* RECT: 0 fill, >= 1 frame width. STAMP: the mask's row pitch in bytes */
  int32_t mask_off; /* STAMP: offset of the mask's first byte in the pool */
  uint8_t color[4]; /* [0..2] in the image's channel order; [3] is not read */
} ffp_overlay_prim; /* sizeof == FFP_OVERLAY_PRIM_BYTES */
int ffp_overlay_draw_dev(int device, uint8_t* d_img, int h, int w, int64_t row_stride, const ffp_overlay_prim* prims, int n, const uint8_t* masks,
                         int64_t mask_bytes);
int ffp_overlay_draw(int device, uint8_t* img, int h, int w, int64_t row_stride, const ffp_overlay_prim* prims, int n, const uint8_t* masks,
                     int64_t mask_bytes);

/* Replaces what cv2.imread does with the EXIF orientation after decoding (/root/reference/utils/visualization.py:95,198, utils/enhancer.py:254)
 * and ImageOps.exif_transpose inside read_image_as_pil (sahi/predict.py:608) on an image that stays in device memory (csrc/orient.hip): the
 * h x w image of px (1, 3 or 4) bytes per pixel at d_src (row pitch src_stride bytes) is written to d_dst (row pitch dst_stride) with
 * orientation 1 as stored (a pitched copy), 2 mirrored in x, 3 in both, 4 in y, 5 transposed, 6 transposed then mirrored in x, 7 then in both,
 * 8 then in y; for 5..8 the destination is w x h. Both bases may have any byte alignment; bytes between a row's w' * px and the pitch are never
 * written. Out of place. FFP_ERR_ARG before anything is queued, the destination untouched: source and destination byte ranges that overlap, an
 * orientation outside 1..8, px other than 1, 3, 4, a pitch smaller than a row, cap (the bytes there are from d_dst on) smaller than
 * (h' - 1) * dst_stride + w' * px. ffp_image_orient_batch_dev: n images in ONE launch, image i hs[i] x ws[i] at d_src_base + src_offsets[i]
 * to d_dst_base + dst_offsets[i] (cap: the bytes from d_dst_base on; a destination that overlaps another destination or ANY image's source is
 * FFP_ERR_ARG as well).
 * ffp_image_orient: the same through host memory (up, turned, down), for tests and small callers. ffp_image_orient_geometry: test hook, the side
 * in pixels of the square tile one workgroup moves. ffp_image_orient_stats: images turned and launches queued since the library was loaded
 * (the turned files of ffp_jpeg_decode_*oriented* count too). */
int ffp_image_orient_dev(int device, const uint8_t* d_src, int h, int w, int px, int64_t src_stride, int orientation, uint8_t* d_dst, int64_t dst_stride,
                         int64_t cap);
int ffp_image_orient_batch_dev(int device, int n, const uint8_t* d_src_base, const int64_t* src_offsets, const int32_t* hs, const int32_t* ws, int px,
                               const int64_t* src_strides, const int32_t* orientations, uint8_t* d_dst_base, const int64_t* dst_offsets,
                               const int64_t* dst_strides, int64_t cap);
int ffp_image_orient(int device, const uint8_t* src, int h, int w, int px, int64_t src_stride, int orientation, uint8_t* dst, int64_t dst_stride, int64_t cap);
/* Measurement hook (tools/orient_probe.py): `iters` (1..10000; a few hundred make a window of several milliseconds) launches of the kernel on one packed image between two events, then as many
 * device-to-device copies of the same h * w * px bytes between two more; microseconds per launch and per copy. d_dst holds the copy afterwards. */
int ffp_image_orient_time_dev(int device, const uint8_t* d_src, int h, int w, int px, int orientation, uint8_t* d_dst, int64_t cap, int iters, float* kernel_us,
                              float* copy_us);
int ffp_image_orient_geometry(int32_t* tile);
int ffp_image_orient_stats(int64_t* images, int64_t* launches);

/* 1x1 conv over the virtual concat [nearest_x2(coarse) | fine] (the YOLO neck's Upsample + Concat + C3k2.cv1 without
 * materialising the upsampled tensor: /root/reference's model graph via ultralytics' yolo11-pose.yaml layers 11-13 and 14-16).
 * coarse: [n][h/2][w/2][c_up] (c_up a multiple of 64), fine: [n][h][w][c_fine]; wt: [cout][c_up + c_fine] (input channel
 * order = concat order); y = act(conv + bias): [n][h][w][cout]. fp32 and fp32-split precisions. */
int ffp_op_conv1x1_up2(int device, int precision, const float* coarse, const float* fine, int n, int h, int w, int c_up, int c_fine,
                       const float* wt, const float* bias, int cout, int act, float* y);

/* Tuning / test hook: pin the kernel and workgroup shape ffp_op_conv2d and ffp_op_conv1x1_up2 use from now on (process-wide; -1 =
 * automatic, the default). The numbers are the ConvShape table of csrc/conv_route.hpp (ffp_op_conv2d_shape_name lists it): 0..5 the
 * generic kernel, 6..8 conv_rows, 9 / 23 conv_rows16, 24 conv_rows16pc, 10..16 and 22 conv_pw, 17..21 conv_k3d, 25 conv_trunk. A number
 * that is not in the table is FFP_ERR_ARG here and leaves the setting as it was. A shape that cannot run the op of a following call —
 * its layout or geometry, or an activation, residual or post-activation its epilogue does not implement — is that call's FFP_ERR_ARG:
 * a pinned shape runs the op or nothing does. (Image-input convs have one kernel and ignore the setting.) */
int ffp_op_conv2d_shape(int force_shape);
/* Test hook, needs no device: "<family> <variant suffix>" of a shape number, e.g. "pw pw2x2w" (the suffix is how the variant strings of
 * the profile getters end); FFP_ERR_ARG for a number that is not a shape. */
int ffp_op_conv2d_shape_name(int shape, char* out, int cap);
/* Test hook: the variant string (as the profile getters report it, e.g. "f16_k3s1_rows16") of the op that the last ffp_op_conv2d or
 * ffp_op_conv1x1_up2 call of this thread launched; empty after a call that launched no dense conv (an error, a depthwise conv). */
int ffp_op_conv2d_last_variant(char* out, int cap);
/* Test hook of the same kind and lifetime: the activation code (0 none, 1 SiLU, 2 LeakyReLU(0.2), 3 ReLU) ffp_op_conv2d applies AFTER the
 * residual term from now on (ConvOp::act_post; process-wide; 0 = none, the default). Any other code: FFP_ERR_ARG; a depthwise
 * ffp_op_conv2d call while it is set: FFP_ERR_ARG. */
int ffp_op_conv2d_act_post(int act);

/* ---- the detector's non-convolution kernels one at a time (operator parity tests) ----------------------------------------
 * A batch is n images of hs[i] x ws[i] pixels; host arrays hold them back to back as [sum hs*ws][cs] fp32 pixel records, and a
 * view is `c` channels at `coff` of records of `cs` — a channel slice of a wider buffer, as the plans use them. On the device the
 * images are laid out with every image starting at a multiple of `px_align` pixels (1: packed). precision: FFP_PREC_F32 or
 * FFP_PREC_F16 storage (values are rounded to fp16 on the way in). Output arrays are in/out: the caller's contents are uploaded
 * first, so everything outside the written slice comes back unchanged. Bad arguments: FFP_ERR_ARG, nothing is launched. */

/* Test hook: pin the kernel ffp_op_sppf_pool (family 0: 1 LDS, 2 direct), ffp_op_psa_attention (family 1: 1 MFMA, 2 VALU) or
 * ffp_op_dwconv3x3 (family 2: 1 column walk, 2 strip) launches from now on (process-wide; 0 = the automatic choice, the default).
 * A variant that cannot run the op is an error of the following op call. Engines are not affected. */
int ffp_op_variant(int family, int variant);
/* Test hook of ffp_op_cls_tower: rows = 16 or 8 pins the tile height of its two launches (0: the launcher's choice from the batch's shapes),
 * wg_cap > 0 launches at most that many workgroups, so that a small batch walks its tiles persistently (0: no cap). Process-wide. */
int ffp_op_cls_tower_variant(int rows, int wg_cap);

/* SPPF: y1, y2, y3 = three chained MaxPool2d(5, 1, 2) of x, written to the slices y*_coff of one buffer y. */
int ffp_op_sppf_pool(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, float* y, int y_cs, int y1_coff, int y2_coff, int y3_coff);

/* nearest x2: y (images of 2 hs[i] x 2 ws[i]) = upsample(x). */
int ffp_op_upsample2x(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff);

/* C2PSA attention, key_dim 32 / head_dim 64: qkv view of nh * 128 channels, per head [q(32) | k(32) | v(64)]; out view of nh * 64
 * channels = softmax(q^T k / sqrt(32)) applied to v, over the h*w pixels of each image. */
int ffp_op_psa_attention(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int nh, const float* qkv, int q_cs,
                         int q_coff, float* out, int o_cs, int o_coff);

/* depthwise 3x3, stride 1, pad 1: y = act(conv(x) + bias) [+ res]. wt: [c][3][3], bias: [c] or NULL; act: 0 none, 1 SiLU,
 * 2 LeakyReLU(0.2), 3 ReLU. grp > 0 reads input channel ch at x_coff + (ch / grp) * grp_stride + grp_off + ch % grp (the PSA
 * positional conv reading v in place from the [q|k|v] records); grp = 0: channel ch at x_coff + ch. res: optional, NULL = none. */
int ffp_op_dwconv3x3(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, int grp, int grp_stride, int grp_off, const float* wt, const float* bias, int act, const float* res, int r_cs,
                     int r_coff, float* y, int y_cs, int y_coff);

/* The YOLO11 class tower of one head level as the detector's fp32-split plan runs it fused (conv_dwpw.hip): two launches,
 *   e1 = SiLU(pw0(SiLU(dw0(x))))   and   logits = fin(SiLU(pw1(SiLU(dw1(e1))))),
 * each depthwise 3x3 inside the loader of the 1x1 behind it; with nc <= 4 the closing 1x1 runs in the second launch's epilogue, with nc > 4 as
 * the conv it is in the unfused plan. x: [pixels][cin] (cin a multiple of 16), dw0: [cin][3][3] + [cin], pw0: [128][cin] + [128], dw1: [128][3][3]
 * + [128], pw1: [128][128] + [128], fin: [nc][128] + [nc]. px_align must be a multiple of 32 (one split exponent per image). e1 (NULL = skip):
 * [pixels][128] out. head: [pixels][head_cs] in/out, the logits go to channels [head_coff, head_coff + nc). stray (NULL = skip): the number of
 * 32-bit words that changed in the padding pixels between the aligned images and behind the last one (e1, the stored second tensor when nc > 4,
 * and, with nc <= 4, the head record): the device buffers go up with a known pattern there and are read back whole. With nc > 4 the head record
 * is written by the plain 1x1 conv, whose flat-pixel kernels compute padding pixels like any pixel; it is then left out of the count. */
int ffp_op_cls_tower(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int cin, int nc, const float* x, const float* dw0_w,
                     const float* dw0_b, const float* pw0_w, const float* pw0_b, const float* dw1_w, const float* dw1_b, const float* pw1_w,
                     const float* pw1_b, const float* fin_w, const float* fin_b, float* e1, float* head, int head_cs, int head_coff, int64_t* stray);

/* One dense conv (k in {1,3}, stride in {1,2}, pad k/2, optional nearest x2 `up` in front) on the operands the plans give it:
 *   y = act_post( (act(conv(x) + bias) * s1 + res1) * s2 + res2 )
 * hs / ws: INPUT image sizes of a ragged batch; the output level is derived per image and both levels are built with px_align. x: channels
 * [x_coff, x_coff + cin) of records of x_cs; y (in/out: the caller's contents go up first), res1 and res2 (NULL = none) hold the output level's
 * images as slices of records of y_cs / r1_cs / r2_cs. wt: [cout][cin][k][k], bias: [cout] or NULL. The kernel is the one ffp_op_conv2d_shape
 * pins (ffp_op_conv2d_last_variant names it). per_image_amax = 1: n max-|value| slots per tensor (one split exponent per image), else one; the
 * input's are filled from the data, amax_out (n or 1 values, in/out) carries the output slots' initial and final bit patterns.
 * gate (NULL = every image): int32[n], nonzero = active (ConvOp::gate). gate_prev (only with gate): the op runs once under gate_prev, then y and
 * the output slots go up again, the device mask is overwritten with gate, the level's gated tile tables are compacted again and the op runs a
 * second time — two runs of one captured plan. stray (NULL = skip): the number of bytes that changed among the 256 behind y's records plus the
 * number of elements that changed in y's padding pixels (of a 1x1 conv: outside its own slice, whose padding pixels the flat-pixel kernels compute like any pixel;
 * behind an image that is inactive under gate they count too). */
int ffp_op_conv2d_views(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, const float* x, int x_cs, int x_coff,
                        int cin, const float* wt, const float* bias, int cout, int k, int stride, int act, int act_post, int up, const float* res1,
                        int r1_cs, int r1_coff, float s1, const float* res2, int r2_cs, int r2_coff, float s2, float* y, int y_cs, int y_coff,
                        int per_image_amax, uint32_t* amax_out, const int32_t* gate, const int32_t* gate_prev, int64_t* stray);

/* Pose-head post-processing on given head tensors. hs / ws: net input size per image (multiples of 32); head8 / head16 / head32:
 * [sum (hs/s)*(ws/s)][64 + nc + 3*nkpt] fp32 records (64 DFL logits | class logits | keypoint raws). gain_pad [n][3] = gain,
 * pad_x, pad_y and rects [n][4] = crop width, crop height, x0, y0: the un-letterboxing geometry of each image.
 * out_raw (NULL = skip): per image the inference-mode head output [4 + nc + 3*nkpt][anchors], images back to back.
 * out_dets / out_counts (both or neither): [n][max_det][6 + 3*nkpt] rows x1, y1, x2, y2, score, class, keypoints after decode
 * (score > conf), NMS (IoU > iou, per class) and scale_boxes / scale_coords, rows past out_counts[i] zero; round_boxes rounds the
 * box; shift = 1 also applies the wrapper's int truncation, clip to full_w / full_h and shift by (x0, y0). */
int ffp_op_det_post(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int nc, int nkpt, const float* head8, const float* head16,
                    const float* head32, const float* gain_pad, const int32_t* rects, float conf, float iou, int max_det, int round_boxes,
                    int shift, int full_h, int full_w, float* out_raw, float* out_dets, int32_t* out_counts);

/* RT-DETR query selection: per image the indices of the 300 tokens with the largest max-over-classes logit, ordered by (logit
 * descending, index ascending). scores: [n][nt][s_cs] fp32, the nc class logits at s_coff. Logits are ordered by their bit
 * patterns (+0.0 above -0.0, which float comparison calls equal). out_idx: [n][300]. */
int ffp_op_rt_topk(int device, int n, int nt, int nc, const float* scores, int s_cs, int s_coff, int32_t* out_idx);

/* ---- the RT-DETR and SCRFD non-convolution kernels one at a time (csrc/rtdetr_ops.hip, csrc/scrfd_ops.hip), fp32 ---------------------
 * The rt_* kernels address image i at i * h * w pixels without padding: one (h, w) or token count for the whole batch, host arrays
 * [n * h * w][cs]. Views are channel slices (cs, coff; multiples of 4) as above and output arrays are in/out. `amax` (NULL: the
 * kernel gets no slot): the max-|value| slot of the output buffer, in = its initial bit pattern, out = its final one. */

/* depthwise k x k, stride s, pad k / 2 (k5 s1 or k3 s2): y ([n][ho][wo], ho = (h - 1) / s + 1) = act(conv(x) + bias); wt: [c][k][k]
 * (repacked like the engine's weights), act 0 none / 3 ReLU. */
int ffp_op_rt_dwconv(int device, int n, int h, int w, int c, int k, int s, int act, const float* x, int x_cs, int x_coff, const float* wt,
                     const float* bias, float* y, int y_cs, int y_coff, uint32_t* amax);
/* HGStem's pool: F.pad(x, [0, 1, 0, 1]) then MaxPool2d(2, 1, ceil_mode=True); y has the size of x. */
int ffp_op_rt_maxpool2(int device, int n, int h, int w, int c, const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, uint32_t* amax);
/* y[p] = a[p] + b[period ? p % period : p] over npx pixel records; b has period (or npx) records of b_cs. */
int ffp_op_rt_add(int device, long long npx, int c, const float* a, int a_cs, int a_coff, const float* b, int b_cs, int b_coff, long long period,
                  float* y, int y_cs, int y_coff, uint32_t* amax);
/* LayerNorm over 256 channels, eps 1e-5. x = NULL: in place on the slice of y. */
int ffp_op_rt_layernorm(int device, long long npx, const float* x, int x_cs, int x_coff, const float* gamma, const float* beta, float* y, int y_cs,
                        int y_coff, uint32_t* amax);
/* exact (erf) GELU in place on c channels at coff of x. */
int ffp_op_rt_gelu(int device, long long npx, int c, float* x, int cs, int coff, uint32_t* amax);
/* 8 heads of 32 over the L tokens of each image: qk view of 512 channels [q 256 | k 256], v view of 256, y view of 256. */
int ffp_op_rt_attention(int device, int n, int L, const float* qk, int qk_cs, int qk_coff, const float* v, int v_cs, int v_coff, float* y, int y_cs,
                        int y_coff, uint32_t* amax);
/* encoder input: three levels of hs[l] x ws[l] pixels with 256 channels at src_coff[l] of records of src_cs[l] -> t [rows][256] tokens
 * [level 0 | 1 | 2] per image and tm = t where valid[token] != 0, else 0. rows >= n * tokens: the records behind stay untouched. */
int ffp_op_rt_enc_prep(int device, int n, const int32_t* hs, const int32_t* ws, const float* src0, const float* src1, const float* src2,
                       const int32_t* src_cs, const int32_t* src_coff, const float* valid, long long rows, float* t, float* tm, uint32_t* amax_t,
                       uint32_t* amax_tm);
/* the selected queries: q[i][j] = e[i][clamp(idx[i][j], 0, nt - 1)] (256 channels) and anc_out[i][j] = anchors[that token] (4 values,
 * copied as they are). idx: [n][300], anchors: [nt][4], anc_out: [n][300][4]. */
int ffp_op_rt_gather(int device, int n, int nt, const float* e, int e_cs, int e_coff, const int32_t* idx, const float* anchors, float* q, int q_cs,
                     int q_coff, float* anc_out, uint32_t* amax);
/* reference boxes over nq queries, 4 channels: anc ([nq][4]) given: ref = sigmoid(delta + anc); NULL: ref = sigmoid(delta +
 * inverse_sigmoid(ref, 1e-5)) in place. */
int ffp_op_rt_ref(int device, long long nq, const float* delta, int d_cs, int d_coff, const float* anc, float* ref, int r_cs, int r_coff,
                  uint32_t* amax);
/* MSDeformAttn core (8 heads, 3 levels of hs[l] x ws[l], 4 points): val [n][tokens] view of 256, oa [n][300] view of 288 (192 offsets |
 * 96 weight logits), ref [n][300] view of 4 (cx, cy, w, h) -> y [n][300] view of 256. */
int ffp_op_rt_deform(int device, int n, const int32_t* hs, const int32_t* ws, const float* val, int v_cs, int v_coff, const float* oa, int oa_cs,
                     int oa_coff, const float* ref, int r_cs, int r_coff, float* y, int y_cs, int y_coff, uint32_t* amax);
/* the predictor's outputs from ref ([n][300] view of 4) and class logits (view of nc). out_raw (NULL = skip): [n][300][4 + nc] boxes and
 * sigmoid scores. out_det / out_counts (both or neither): RTDETRPredictor.postprocess, [n][300][6] rows x1, y1, x2, y2, score, class of
 * the queries whose best score > conf, in query order, scaled by orig_wh [n][2] = (width, height); rows past out_counts[i] untouched. */
int ffp_op_rt_decode(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                     const float* orig_wh, float* out_raw, float* out_det, int32_t* out_counts);
/* rt_post_tiles: the same selection for n tiles of one full_h x full_w frame, tiles_xyxy [n][4] = x0, y0, x1, y1 in frame pixels (the scale
 * is the tile's width and height). mode FFP_RT_TILES_LOCAL: crop-local rows, as ffp_op_rt_decode. mode FFP_RT_TILES_SAHI: what sahi 0.11.x
 * UltralyticsDetectionModel._create_object_prediction_list_from_original_predictions, ObjectAnnotation and get_shifted_object_prediction do
 * to such a row, with float boxes: x1 = max(x1, 0), y1 = max(y1, 0), x2 = min(x2, full_w), y2 = min(y2, full_h) (the crop-local box against
 * the FULL shape), the row dropped unless x1 < x2 and y1 < y2, then + x0 / + y0 with no second clip. Every step is one float32 operation.
 * out_dets [n][300][6] in/out (rows past out_counts[i] untouched), out_counts [n]; rows in query order. */
int ffp_op_rt_post_tiles(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                         const int32_t* tiles_xyxy, int full_h, int full_w, int mode, float* out_dets, int32_t* out_counts);

/* SCRFD's pools on a ragged batch (px_align as above): maxpool != 0: MaxPool 3x3 / stride 2 / pad 1 (y images of (h - 1) / 2 + 1);
 * else AveragePool k x k / stride k, ceil_mode, count_include_pad = 0 (y images of ceil(h / k)). */
int ffp_op_scrfd_pool(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, int maxpool, int k, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff);
/* RetinaFace.detect's decode + NMS from head tensors. n images at net size net_h x net_w; level l has (net_h / strides[l]) x
 * (net_w / strides[l]) pixels with A anchors each. heads: 9 host arrays {score, bbox, kps} x 3 levels (kps NULL for the 6-output
 * variant), per pixel records of cs[kind] with the A / 4A / 10A values at coff[kind]; scores are logits (the decode applies the sigmoid).
 * Candidates: score >= thresh; NMS keeps a candidate whose "+1"-convention overlap with every kept one is <= nms_thresh.
 * out: [n][cap][FFP_DET_STRIDE(5)] in/out; out_counts[i] = faces KEPT for image i, which exceeds cap when the list was cut (only the
 * first cap rows are written). raw_scores (NULL = skip): [n][anchors per image] the decode's sigmoid of every anchor. */
int ffp_op_scrfd_post(int device, int n, int net_h, int net_w, int A, const int32_t* strides, int px_align, const float* const* heads,
                      const int32_t* cs, const int32_t* coff, const float* det_scale, float thresh, float nms_thresh, int cap, float* out,
                      int32_t* out_counts, float* raw_scores);
/* scrfd_sahi_rows alone: what utils/insightface_wrapper.py's conversion, sahi's ObjectAnnotation / BoundingBox and
 * get_shifted_object_prediction do to the rows of n_tiles tiles {x0, y0, x1, y1} of a full_h x full_w frame, per row and in this order:
 * (1) skipped when score < conf (strict, float32); (2) x1, y1, x2, y2 = (int) of the float32 value, toward zero (face.bbox.astype(int));
 * (3) x1 = max(x1, 0), y1 = max(y1, 0), x2 = min(x2, full_w), y2 = min(y2, full_h): the crop-local box against the FULL frame;
 * (4) x2 < 0 or y2 < 0 now: the reference raises "Box coords [minx, miny, maxx, maxy] cannot be negative" and the frame fails; here the
 * smallest tile * cap + row of such a box goes to *out_bad (-1: none) and the call returns FFP_ERR_ARG naming tile and row; (5) the tile
 * origin added to the box (integers) and to the five keypoints' x, y (floats); boxes with x1 >= x2 are kept, as the reference keeps them;
 * (6) survivors stay in their tile's order at the front of the tile. dets [n_tiles][cap][FFP_DET_STRIDE(5)] and counts [n_tiles] in/out:
 * counts above cap are read as cap; rows the survivors vacate (from the new count up to the old one) are zeroed, rows at or past the old
 * count are untouched. After an error return the outputs hold the other rows' results with the offending rows left out. */
int ffp_op_scrfd_sahi_rows(int device, int n_tiles, int cap, const int32_t* tiles_xyxy, int full_h, int full_w, float conf, float* dets,
                           int32_t* counts, int32_t* out_bad);

/* Tests only: the image-input kernels alone. frame: H x W x 3 u8 on the host; the n items are boxes {x0, y0, x1, y1} of it, turned into
 * letterbox records by the code the engines run (a box outside the frame, or a size that is no multiple of 32, is FFP_ERR_ARG). chan_order as
 * for the detectors. Every output holds the items back to back and goes up as NaN, so a pixel no kernel wrote comes back as NaN.
 *
 * ffp_op_image_input: kind 0 = the YOLO letterbox at imgsz size_a (pad 114, / 255), 1 = the RT-DETR stretch to size_a x size_a (/ 255),
 * 2 = SCRFD at det size size_a x size_b (w x h): picture at the top-left, pad 0, (v - 127.5) / 128, FFP_PREC_F32 only. out: whole pixel
 * records as float32, pad channels included — 4 per pixel, 8 for kinds 0 and 1 in FFP_PREC_F16 (values rounded to fp16 by the kernel) — sized
 * for n * size_a * size_a (kind 2: n * size_a * size_b) pixels; out_hs / out_ws [n]: the network size of every item. */
int ffp_op_image_input(int device, int kind, int precision, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy,
                       int size_a, int size_b, float* out, int32_t* out_hs, int32_t* out_ws);
/* The image-input 3x3 conv (w [cout][3][3][3], bias [cout], cout 16 / 32 / 64, stride 1 or 2, pad 1, activation code act) on the YOLO
 * letterbox of every item at imgsz: fused 0 = letterbox kernel, then the direct conv kernel; 1 = the one kernel that reads the frame through
 * the letterbox arithmetic. FFP_PREC_F32 or FFP_PREC_F16. out: [sum ho * wo][cout] float32, ho = (net_h - 1) / stride + 1. */
int ffp_op_stem(int device, int precision, int fused, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy, int imgsz,
                const float* w, const float* bias, int cout, int stride, int act, float* out);
/* model.0 computed inside model.1's loader (FFP_PREC_F32X3): stem 3x3 stride 2 SiLU to stem_cout (16 or 32) channels, then conv_w
 * [2 * stem_cout][stem_cout][3][3] stride 2 SiLU, laid out as a split plan lays it out (levels aligned to 32 pixels, one max-|value| slot per
 * image, the stem output's from the weight bound). out: [sum (net_h / 4) * (net_w / 4)][2 * stem_cout]. A pair of convs the loader
 * refuses is FFP_ERR_ARG; nothing else ever runs in its place. */
int ffp_op_stem_conv(int device, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy, int imgsz, const float* stem_w,
                     const float* stem_b, int stem_cout, const float* conv_w, const float* conv_b, float* out);

/* Tests only: the kernels around the Real-ESRGAN network alone — no weights, no plan. An image is 8 int64 {byte offset, bytes per row, h, w, channels
 * (1, 3, 4), bits (8, 16), range (255, or 65535 in 16-bit storage), selection (0 BGR, 1 gray: channel 0, 2 alpha: channel 3 of 4)} inside ONE host
 * buffer; offsets and strides are multiples of the element size, rows may be padded and images may share bytes (a colour and an alpha image over one
 * BGRA buffer). h and w are the INPUT size; a canvas is scale times as large. scale is 4 or 2. Tiles, descriptor tables and level sizes come from the
 * code the enhancer runs. cap_t16 == 0: exact levels (Level::build); cap_t16 > 0: levels reserved for that many 16x16 body tiles and assigned, as a
 * plan's are; then an earlier batch (n_first > 0, same buffer) may be assigned and run first. FFP_ERR_ARG leaves every buffer as it was.
 *
 * ffp_op_sr_tiles (no device): h and w of every padded tile in tile order -> out_hw [cap_tiles][2], their number, the 16x16 body tiles a plan's
 * capacity counts, and the channels of the network's input record in `precision` (conv_first's padded input channels).
 * ffp_op_sr_pre: flat [flat_px][channels] fp32 in/out is the body level's WHOLE buffer (flat_px: sum of h/f * w/f over the tiles, f the pixel_unshuffle
 * factor scale == 2 ? 2 : 1, or 256 * cap_t16): the caller's contents go up (rounded to fp16 in FFP_PREC_F16), the batches run, everything comes
 * back; out_off [tiles]: first record of every tile.
 * ffp_op_sr_post: net holds every tile's network output back to back, [scale * h][scale * w][cs] fp32 with RGB in channels 0-2; canvas in/out is
 * the whole buffer the images lie in. The launch is the enhancer's: total_core is the x4 level's pixel count, the tables are padded to the capacity.
 * only_tile >= 0 empties the core of every other tile of the batch, so that what one tile writes is not covered by its neighbours (-1: all tiles). */
int ffp_op_sr_tiles(int n, const int64_t* imgs, int scale, int tile, int tile_pad, int pre_pad, int precision, int cap_tiles, int32_t* out_hw,
                    int32_t* out_n, int32_t* out_t16, int32_t* out_channels);
int ffp_op_sr_pre(int device, int precision, const uint8_t* src, size_t src_bytes, int n, const int64_t* imgs, int scale, int tile, int tile_pad,
                  int pre_pad, int cap_t16, int n_first, const int64_t* imgs_first, float* flat, size_t flat_px, int64_t* out_off);
int ffp_op_sr_post(int device, int n, const int64_t* imgs, int scale, int tile, int tile_pad, int pre_pad, const float* net, int cs, int cap_t16,
                   int n_first, const int64_t* imgs_first, const float* net_first, int only_tile, uint8_t* canvas, size_t canvas_bytes);
/* The 'cv2' alpha upsampler alone: src h x w x 4 (uint8, or uint16 with src_bits 16), dst out_h x out_w x 4 in/out (dst_bits 8 or 16; 16 needs a
 * 16-bit source, range 65535 needs both): channel 3 = rint(resize_linear(src[..., 3] / range) * range), channels 0-2 stay. */
int ffp_op_alpha_linear(int device, const void* src, int h, int w, int src_bits, int range, int out_h, int out_w, int dst_bits, void* dst);
/* The crop gather alone: box i {x0, y0, w, h} of an H x W x 3 uint8 frame -> w * h * 3 bytes at out + offs[i]; out in/out. n == 0 is accepted. */
int ffp_op_crop_gather(int device, const uint8_t* frame, int H, int W, int n, const int32_t* boxes_xywh, const int64_t* offs, uint8_t* out,
                       size_t out_bytes);

/* Tuning hook: mean device time (HIP events, microseconds) of `iters` back-to-back launches of one dense convolution on
 * synthetic data. dbg_mask skips kernel phases (1 stores, 2 MFMAs, 4 chunk refetch, 8 LDS stash) to attribute time —
 * results are then wrong by construction; force_shape pins the workgroup shape (-1: automatic). */
int ffp_op_conv2d_time(int device, int precision, int n, int h, int w, int cin, int cout, int k, int stride, int up, int iters,
                       int dbg_mask, int force_shape, float* out_us);

/* timing hooks for bench.py: HIP-event milliseconds of the last call on the handle, by stage
 * stage: 0 total, 1 preprocess, 2 network, 3 decode+nms, 4 merge */
int ffp_det_last_ms(ffp_det* d, int stage, float* out_ms);
int ffp_sr_last_ms(ffp_sr* s, float* out_ms);

/* algorithmic conv FLOPs (2*MAC) of the last call, its number of convolution launches, and (profiling enabled) the
 * HIP-event time spent in convolution kernels */
int ffp_det_last_conv_stats(ffp_det* d, double* out_flops, float* out_ms, int32_t* out_launches);
int ffp_sr_last_conv_stats(ffp_sr* s, double* out_flops, float* out_ms, int32_t* out_launches);

/* Per-launch HIP-event profiling of the convolution kernels on the handle's stream. While enabled every conv launch
 * of a call is bracketed by two events; afterwards the table lists, per kernel variant ("f16_k3s1_narrow1", ...),
 * the algorithmic FLOPs, the summed event time and the launch count of the LAST call. */
int ffp_det_set_profile(ffp_det* d, int enable);
int ffp_det_profile_count(ffp_det* d, int32_t* out_n);
int ffp_det_profile_get(ffp_det* d, int i, char* name, int name_cap, double* out_flops, float* out_ms, int32_t* out_launches);
int ffp_sr_set_profile(ffp_sr* s, int enable);
int ffp_sr_profile_count(ffp_sr* s, int32_t* out_n);
int ffp_sr_profile_get(ffp_sr* s, int i, char* name, int name_cap, double* out_flops, float* out_ms, int32_t* out_launches);
/* algorithmic bytes of entry i of the same table: every input, residual and output element of the launches once (real channels, the tensors'
 * element size) + weights and bias once — the denominator for the PMC traffic of the same launches (bench.py: roofline.algorithmic_bytes) */
int ffp_det_profile_bytes(ffp_det* d, int i, double* out_bytes);
int ffp_sr_profile_bytes(ffp_sr* s, int i, double* out_bytes);
/* Process-wide lifetime totals per kernel variant over EVERY plan execution since enable(1) (eager, profiled or hipGraph replay; all handles):
 * launches, algorithmic FLOPs, algorithmic bytes. A rocprofv3 --pmc pass over a command sums its counters over all launches of a kernel; with
 * these totals printed by the same command (bench.py --conv-totals), traffic per launch and algorithmic bytes per launch describe one population.
 * Off by default. Diagnostics only: the reference has no counterpart (its torch modules are opaque to it). */
int ffp_conv_totals_enable(int on);
int ffp_conv_totals_count(int32_t* out_n);
int ffp_conv_totals_get(int i, char* name, int name_cap, double* out_flops, double* out_bytes, int64_t* out_launches);
/* per-launch entries of the last profiled call, in launch order: "<variant> <layer name>"; returns FFP_ERR_ARG past the end */
int ffp_det_profile_detail(ffp_det* d, int i, char* name, int name_cap, double* out_flops, float* out_ms);
int ffp_sr_profile_detail(ffp_sr* s, int i, char* name, int name_cap, double* out_flops, float* out_ms);

/* ---------------------------------------------------------------------------------------------------------
 * face detector of InsightFace's model packs (SCRFD, e.g. buffalo_l/det_10g.onnx) — replaces
 * insightface.model_zoo.retinaface.RetinaFace (prepare / detect / nms, insightface 0.7.3 model_zoo/retinaface.py), reached
 * through insightface.app.FaceAnalysis.get (app/face_analysis.py) behind utils/insightface_wrapper.py's InsightFaceDetectionModel
 * ------------------------------------------------------------------------------------------------------- */
typedef struct ffp_scrfd ffp_scrfd;

/* onnx_bytes: the ONNX model file (self-contained; external data is refused). The graph is lowered to the supported op subset
 * (see ffp_scrfd_describe); anything outside it fails with FFP_ERR_ARG and a message naming the node, its op and attribute.
 * n: the batch the graph is checked at on creation (plans themselves are laid out per call shape, for any batch).
 * precision: FFP_PREC_F32 or FFP_PREC_F32X3.
 * (RetinaFace.__init__ + prepare, model_zoo/retinaface.py) */
int ffp_scrfd_create(const void* onnx_bytes, size_t nbytes, int n, int device, int precision, ffp_scrfd** out);
void ffp_scrfd_destroy(ffp_scrfd* s);

/* Host only, no device needed: the lowered step list of the model for batch n at net size det_w x det_h, one line per step,
 * then one line per graph output; or the refusal message (returned as the error, and written to out as well).
 * out: NUL-terminated, truncated to cap bytes. */
int ffp_scrfd_describe(const void* onnx_bytes, size_t nbytes, int n, int det_w, int det_h, char* out, size_t cap);

/* RetinaFace.detect(img, input_size=(det_w, det_h), max_num=0) over n_tiles crops of one HxWx3 uint8 frame, batched:
 * per crop the resize into the top-left of the net size (det_scale = new_h / h), blobFromImage((v - 127.5) / 128, swapRB),
 * the network, scores >= det_thresh, distance2bbox / distance2kps, / det_scale, NMS at nms_thresh (areas with +1, kept when
 * overlap <= nms_thresh; equal scores in ascending anchor order).
 * out_dets: [n_tiles][cap][FFP_DET_STRIDE(5)] rows x1,y1,x2,y2,score,0, then 5 x (x, y, 1.0); crop-local floats, not truncated.
 * out_counts[n_tiles]: faces kept per crop, NOT capped; the call returns FFP_ERR_ARG when any exceeds cap.
 * chan_order as for the YOLO detector: SAHI hands RGB arrays and swapRB flips them, so FFP_CHAN_AS_BGR reproduces the reference.
 * A crop that resizes to zero width or height (cv2.resize raises there) returns FFP_ERR_ARG. */
int ffp_scrfd_infer_tiles(ffp_scrfd* s, const uint8_t* frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy,
                          int n_tiles, int det_w, int det_h, float det_thresh, float nms_thresh, float* out_dets, int cap,
                          int32_t* out_counts);

/* Sliced prediction. Upstream sahi and insightface were not available to run against: the rules below restate
 * utils/insightface_wrapper.py and sahi 0.11.x from their source, and only synthetic weights have been run (not the real det_10g.onnx). */
#define FFP_SCRFD_TILES_LOCAL 0 /* rows in tile-local float pixels, exactly ffp_scrfd_infer_tiles' rows */
#define FFP_SCRFD_TILES_SAHI 1  /* rows as sahi's ObjectPrediction list holds them after the wrapper: see ffp_op_scrfd_sahi_rows */
/* Items per network batch where a caller of the entries below passes max_batch < 0: the fastest measured size whose plans stay under 8 GB,
 * the rule of FFP_RT_TILES_DEFAULT_BATCH (tools/scrfd_sliced_probe.py on an MI355X, profiles/scrfd_sliced_mi355x.json: 61 items of a
 * 2160 x 3840 frame at 512 / 0.2, det size 640, the full-size synthetic model; FFP_PREC_F32 / F32X3 ms per frame of ffp_scrfd_sliced_predict
 * and the bytes held by the plans: 8: 47.4 / 37.4 ms, 2.1 GB; 16: 42.5 / 32.9 ms, 4.3 GB; 32: 40.6 / 30.0 ms, 8.4 GB; 0, i.e. one batch of
 * 61: 38.8 / 28.2 ms, 8.4 GB; min..max spread under 1 ms each. The Python path, get_sliced_prediction with InsightFaceDetectionModel on
 * the same commit in FFP_PREC_F32: median 123 to 138 ms, 77 to 203 ms over 40 samples). A caller with the memory to spare passes 32 or 0.
 * max_batch == 0 keeps ffp_scrfd_infer_tiles' behaviour: every tile in one batch. */
#define FFP_SCRFD_TILES_DEFAULT_BATCH 16
/* ffp_scrfd_infer_tiles with two additions. (1) Tiles run in ceil(n_tiles / max_batch) chunks of sizes as even as possible (13 at 5: 5, 4, 4),
 * one plan per chunk size, each chunk's decode and NMS writing its slice of the output; the engine scales every image by itself, so a
 * tile's rows do not depend on its batch mates in either precision. (2) mode FFP_SCRFD_TILES_SAHI applies ffp_op_scrfd_sahi_rows at `conf`
 * (the wrapper's confidence_threshold; the network's own filter stays score >= det_thresh) with the frame as the full shape.
 * out_dets: [n_tiles][cap][FFP_DET_STRIDE(5)], rows past out_counts[i] zero; out_counts [n_tiles]. A tile whose NMS keeps more than cap
 * faces is FFP_ERR_ARG with the uncapped NMS counts in out_counts; a negative far corner in SAHI mode is FFP_ERR_ARG naming tile and row.
 * (InsightFaceDetectionModel.perform_inference_batch -> FaceAnalysis.detect_tiles, and in SAHI mode the per-face Python behind it:
 * utils/insightface_wrapper.py:83-86 `score < confidence_threshold` / `face.bbox.astype(int)`, sahi/annotation.py ObjectAnnotation and
 * BoundingBox, sahi/prediction.py get_shifted_object_prediction) */
int ffp_scrfd_infer_tiles_ex(ffp_scrfd* s, const uint8_t* frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy, int n_tiles,
                             int det_w, int det_h, float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* out_dets,
                             int cap, int32_t* out_counts);
/* the same with the frame and both outputs on the device (tiles_xyxy stays a host pointer): a frame decoded by ffp_jpeg_decode_dev stays
 * where it is. Work is enqueued on the engine's stream and the call returns after that stream has drained, as ffp_det_infer_tiles_dev
 * does. Rows past a tile's count are untouched (LOCAL) or zero up to the tile's NMS count (SAHI). Errors as above.
 * (replaces the host round trip between cv2.imread / sahi's slice_image and FaceAnalysis.get, app_v1.py's detector stage) */
int ffp_scrfd_infer_tiles_dev(ffp_scrfd* s, const uint8_t* d_frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy, int n_tiles,
                              int det_w, int det_h, float det_thresh, float nms_thresh, float conf, int mode, int max_batch,
                              float* d_out_dets, int cap, int32_t* d_out_counts);
/* sahi.predict.get_sliced_prediction(image, InsightFaceDetectionModel, slice_height, slice_width, overlap ratios, perform_standard_pred,
 * postprocess_type / match_metric / match_threshold / class_agnostic) in one call (pipeline_v1_detection_first/app_v1.py's detector
 * stage): the grid of ffp_slice_bboxes, plus the full frame when there is more than one slice and perform_standard_pred != 0,
 * ffp_scrfd_infer_tiles_ex in FFP_SCRFD_TILES_SAHI with at most tile_cap faces per item, rows in tile order then score order (the order
 * the Python loop appends ObjectPredictions), then the merge of ffp_merge when there is more than one item and more than one row. Rows
 * keep FFP_DET_STRIDE(5): a merged detection carries the keypoints of its higher-scored source (ffp_merge), shifted to frame pixels.
 * out: [cap][FFP_DET_STRIDE(5)]; more than cap merged rows is FFP_ERR_ARG with *out_n = the full count. A box whose far corner is
 * negative after the clip fails the frame with FFP_ERR_ARG, as the reference's exception does. */
int ffp_scrfd_sliced_predict(ffp_scrfd* s, const uint8_t* frame_hwc, int H, int W, int chan_order, int slice_h, int slice_w,
                             float overlap_h_ratio, float overlap_w_ratio, int perform_standard_pred, int det_w, int det_h, float det_thresh,
                             float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric, double pp_thr,
                             int class_agnostic, float* out, int cap, int32_t* out_n);
/* the same with the frame, d_out [cap][FFP_DET_STRIDE(5)] and d_out_n[1] on the device; returns after the engine's stream has drained.
 * *d_out_n receives the UNTRUNCATED number of merged detections: when it exceeds cap only the first cap rows were written and the caller
 * must treat the result as overflowed (the rule of ffp_merge_dev).
 * (replaces the same call, between ffp_jpeg_decode_dev and ffp_sr_enhance_crops_dev with nothing going through the host) */
int ffp_scrfd_sliced_predict_dev(ffp_scrfd* s, const uint8_t* d_frame_hwc, int H, int W, int chan_order, int slice_h, int slice_w,
                                 float overlap_h_ratio, float overlap_w_ratio, int perform_standard_pred, int det_w, int det_h,
                                 float det_thresh, float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric,
                                 double pp_thr, int class_agnostic, float* d_out, int cap, int32_t* d_out_n);
/* device bytes held by the resident plans (activations and candidate lists) and how many plans are resident (at most 8);
 * ffp_scrfd_drop_plans releases them (no counterpart in the reference: onnxruntime owns its arena) */
int ffp_scrfd_mem_bytes(ffp_scrfd* s, uint64_t* out_plan_bytes, int32_t* out_plans_resident);
int ffp_scrfd_drop_plans(ffp_scrfd* s);

/* The graph outputs of every crop (net_outs of RetinaFace.forward), for parity tests: per crop, per output in file order,
 * anchors x values floats in the graph's (Transpose + Reshape) order; scores are the sigmoid values the decode thresholds.
 * out_sizes[n_outputs]: floats per crop of each output. */
int ffp_scrfd_forward_raw(ffp_scrfd* s, const uint8_t* frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy,
                          int n_tiles, int det_w, int det_h, float* out, size_t cap, int64_t* out_sizes);
/* RetinaFace.detect's resize geometry of one h x w crop at net size net_w x net_h, host only:
 * out2 = {new_w, new_h} (either may be 0: such a crop is refused by ffp_scrfd_infer_tiles), *det_scale = float32(new_h / h). */
int ffp_scrfd_geometry(int h, int w, int net_w, int net_h, int32_t* out2, float* det_scale);
/* number of graph outputs (9 with keypoints, 6 without) and the FLOPs of the convs of the last call's plan */
int ffp_scrfd_info(ffp_scrfd* s, int32_t* out_n_outputs, double* out_last_conv_flops);

/* ---------------------------------------------------------------------------------------------------------
 * Ultralytics RT-DETR-l (rtdetr-l.yaml, fine-tuned at imgsz 640 by pipeline_v3_RTDETR/train_rtdetr.py:162,183) — replaces
 * ultralytics.RTDETR (models/rtdetr/model.py, predict.py RTDETRPredictor, nn/modules/head.py RTDETRDecoder) as
 * pipeline_v3_RTDETR/inference.py uses it
 * ------------------------------------------------------------------------------------------------------- */
typedef struct ffp_rtdetr ffp_rtdetr;

/* weights: FFPW tensors from weights_io.from_ultralytics_rtdetr_state_dict (BatchNorm and RepConv folded, in_proj split); nc is read
 * from the encoder score head. precision: FFP_PREC_F32 or FFP_PREC_F32X3. (self.model = RTDETR(weights_path), inference.py:20) */
int ffp_rtdetr_create(const void* weights, size_t nbytes, int device, int precision, ffp_rtdetr** out);
void ffp_rtdetr_destroy(ffp_rtdetr* r);
/* RTDETRPredictor over n BGR uint8 images (frames[i]: hw[2i] x hw[2i+1] x 3, sizes may differ), one network batch at imgsz (a multiple
 * of 32): LetterBox(auto=False, scale_fill=True) = a cv2 INTER_LINEAR stretch, BGR -> RGB, / 255; the model; postprocess: sigmoid
 * scores, xywh -> xyxy, max over classes > conf, x * width, y * height, query order, no NMS (predict.py RTDETRPredictor.postprocess).
 * out_dets: [n][300][6] {x1, y1, x2, y2, score, cls}; out_counts[n].
 * (self.model.predict(source=image_path | frame, conf=self.conf, ...), inference.py:36-41 and 138-141, read back at :47-51) */
int ffp_rtdetr_predict(ffp_rtdetr* r, const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float conf, float* out_dets,
                       int32_t* out_counts);
/* The model output of every image (RTDETRDecoder.forward in eval: dec_bboxes ++ sigmoid(dec_scores), what the predict calls of
 * inference.py:36 post-process), for parity tests: out: [n][300][4 + nc] {cx, cy, w, h (normalised), scores};
 * out_topk (may be NULL): [n][300] encoder token of each query. */
int ffp_rtdetr_forward_raw(ffp_rtdetr* r, const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float* out, int32_t* out_topk);
/* class count (result.names of inference.py), FLOPs of the convs of the last call's plan and its hipGraph state (1 replaying, 0 not
 * captured yet, -1 eager) */
int ffp_rtdetr_info(ffp_rtdetr* r, int32_t* out_nc, double* out_last_conv_flops, int32_t* out_graph_state);
/* Profiling (no counterpart in the reference): with on != 0 later calls run their plan eagerly with HIP events around every launch;
 * entry i of the last call is "<kernel> <layer>" and its milliseconds, in launch order (FFP_ERR_ARG past the end). */
int ffp_rtdetr_set_profile(ffp_rtdetr* r, int on);
int ffp_rtdetr_profile_count(ffp_rtdetr* r, int32_t* out_n);
int ffp_rtdetr_profile_get(ffp_rtdetr* r, int i, char* name, int name_cap, float* out_ms);

/* Sliced prediction. Upstream sahi was not available to run against: the box rules below restate sahi 0.11.x from its source, and only
 * synthetic weights have been run. */
#define FFP_RT_TILES_LOCAL 0 /* rows in tile-local pixels, exactly ffp_rtdetr_predict's rows of the host crop */
#define FFP_RT_TILES_SAHI 1  /* rows as sahi's ObjectPrediction list holds them: clipped against the full shape, invalid ones dropped, shifted */
/* Items per network batch when max_batch <= 0: the fastest measured size whose plans stay under 8 GB (tools/rtdetr_sliced_probe.py on an
 * MI355X, profiles/rtdetr_sliced_mi355x.json: 61 tiles of a 2160 x 3840 frame at imgsz 640, FFP_PREC_F32 / F32X3 ms per frame and bytes held
 * by the two plans: 4: 144.0 / 102.6 ms, 2.4 GB; 8: 109.7 / 66.8 ms, 5.1 GB; 16: 88.8 / 48.5 ms, 10.5 GB; 32: 78.9 / 40.0 ms, 20.7 GB).
 * A caller with the memory to spare passes 16 or 32. */
#define FFP_RT_TILES_DEFAULT_BATCH 8
/* n_tiles crops [x0, y0, x1, y1] (frame pixels) of one H x W x 3 uint8 frame, each stretched to imgsz x imgsz exactly as
 * ffp_rtdetr_predict stretches an image, so a tile's rows in FFP_RT_TILES_LOCAL equal ffp_rtdetr_predict on the host crop (bit for bit in
 * FFP_PREC_F32). The frame goes up once. Tiles run in ceil(n_tiles / max_batch) chunks of sizes as even as possible (61 at 16: 16, 15, 15,
 * 15; at the default 8: 8, 8, 8, 8, 8, 7, 7, 7), one plan per chunk size. chan_order as for the YOLO detector (sahi hands RGB arrays: FFP_CHAN_AS_RGB). mode: see
 * ffp_op_rt_post_tiles. A tile that is empty, inverted or reaches outside the frame is FFP_ERR_ARG naming the tile.
 * out_dets: [n_tiles][300][6] {x1, y1, x2, y2, score, cls}, query order; out_counts [n_tiles].
 * (sahi.predict.get_sliced_prediction's loop of get_prediction(slice) -> UltralyticsDetectionModel.perform_inference ->
 * model(image[:, :, ::-1], imgsz=..., conf=...), sahi/models/ultralytics.py, and the conversion behind it in FFP_RT_TILES_SAHI) */
int ffp_rtdetr_infer_tiles(ffp_rtdetr* r, const uint8_t* frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy, int n_tiles,
                           int imgsz, float conf, int mode, int max_batch, float* out_dets, int32_t* out_counts);
/* the same with the frame and both outputs on the device (tiles_xyxy stays a host pointer); work is enqueued on the engine's stream and the
 * call returns after that stream has drained, as ffp_det_infer_tiles_dev does */
int ffp_rtdetr_infer_tiles_dev(ffp_rtdetr* r, const uint8_t* d_frame_hwc, int H, int W, int chan_order, const int32_t* tiles_xyxy, int n_tiles,
                               int imgsz, float conf, int mode, int max_batch, float* d_out_dets, int32_t* d_out_counts);
/* sahi.predict.get_sliced_prediction(image, RTDetrDetectionModel, slice_height, slice_width, overlap ratios, perform_standard_pred,
 * postprocess_type / match_metric / match_threshold / class_agnostic) in one call: the grid of ffp_slice_bboxes, plus the full frame when
 * there is more than one slice and perform_standard_pred != 0 (sahi/predict.py), ffp_rtdetr_infer_tiles in FFP_RT_TILES_SAHI, rows in
 * tile order then query order (the order the Python loop appends ObjectPredictions), then the merge of ffp_merge (skipped for one row or
 * fewer). pp_type: FFP_PP_NMS or FFP_PP_GREEDYNMM. out: [cap][6]; more than cap merged rows is FFP_ERR_ARG with *out_n = the full count. */
int ffp_rtdetr_sliced_predict(ffp_rtdetr* r, const uint8_t* frame_hwc, int H, int W, int chan_order, int slice_h, int slice_w,
                              float overlap_h_ratio, float overlap_w_ratio, int perform_standard_pred, int imgsz, float conf, int max_batch,
                              int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* out, int cap, int32_t* out_n);
/* device bytes held by the resident plans' activations and how many plans are resident (at most 4); ffp_rtdetr_drop_plans releases them */
int ffp_rtdetr_mem_bytes(ffp_rtdetr* r, uint64_t* out_plan_bytes, int32_t* out_plans_resident);
int ffp_rtdetr_drop_plans(ffp_rtdetr* r);

/* ---------------------------------------------------------------------------------------------------------
 * No-reference image quality: NIQE — replaces pyiqa.create_metric('niqe', device=...) and the call of the metric on an image
 * tensor (pipeline_v4_yolo/1_Inference.py:122-126 and :171-176). The algorithm is Mittal et al. 2013 with pyiqa 0.1.x's choices
 * as DESIGN.md states them; parity with pyiqa itself has not been run. BRISQUE is not built.
 * ------------------------------------------------------------------------------------------------------- */
#define FFP_IQA_F32_CHW 0 /* float32 planar C x H x W in [0,1], RGB: the tensor pyiqa's metrics are called with */
#define FFP_IQA_U8_HWC 1  /* uint8 H x W x C, channel order FFP_CHAN_AS_BGR / FFP_CHAN_AS_RGB */
#define FFP_NIQE_FEATURES 36

typedef struct ffp_iqa ffp_iqa;

/* pyiqa.create_metric(name, device=device) (1_Inference.py:124): the engine holds the device, a stream, the AGGD Gamma tables and
 * the filter taps. The pristine model (pyiqa's niqe_modelparameters.mat) is an argument of the score call, not of the engine. */
int ffp_iqa_create(int device, ffp_iqa** out);
void ffp_iqa_destroy(ffp_iqa* q);
/* Host: number of 96x96 blocks of an h x w image, floor(h / 96) * floor(w / 96), to size the buffers of the next call. */
int ffp_iqa_niqe_blocks(int h, int w, int64_t* out_blocks);
/* The feature half of pyiqa's niqe() for a ragged batch (what `metric(img_tensor)` computes before the distance, :175): image i is
 * h[i] x w[i] x c[i] (c 1 or 3) in `layout`; chan_order applies to FFP_IQA_U8_HWC with 3 channels. on_device != 0: imgs[i] are
 * device pointers whose producer the caller has synchronised. Each image is cropped to whole 96x96 blocks from its top-left
 * corner; an image with fewer than two blocks is FFP_ERR_ARG (one block has no covariance). out_feat [blocks][36] float64 (scale 1, then
 * scale 2; blocks row-major per image), out_sharp [blocks] = mean local sigma of the scale-1 block (the paper's patch selection),
 * out_block_off [n + 1]. cap_blocks: capacity of out_feat / out_sharp; more blocks than that is FFP_ERR_ARG. A flat block gives NaN
 * where its arithmetic does. */
int ffp_iqa_niqe_features(ffp_iqa* q, int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout,
                          int chan_order, int on_device, double* out_feat, double* out_sharp, int64_t cap_blocks, int64_t* out_block_off);
/* Step one of the same alone, for parity tests: the rounded luma (pyiqa's to_y_channel(img, 255, 'yiq').round()) of one host
 * image's crop, out_y [floor(h / 96) * 96][floor(w / 96) * 96] float32 holding integers 0..255. */
int ffp_iqa_niqe_luma(ffp_iqa* q, const void* img, int h, int w, int c, int layout, int chan_order, float* out_y);
/* The distance half of pyiqa's niqe() (host, float64): per image sqrt((mu - m)^T pinv((cov + C) / 2) (mu - m)) with m the
 * per-feature nanmean of the image's blocks, C their sample covariance over blocks without NaN, and singular values below
 * 36 * 2.2e-16 * the largest treated as zero. mu [36], cov [36][36]: the pristine model (mu_prisparam / cov_prisparam).
 * out_scores [n]; an image with fewer than two NaN-free blocks scores NaN. */
int ffp_iqa_niqe_score(const double* feat, const int64_t* block_off, int n, const double* mu, const double* cov, double* out_scores);

#ifdef __cplusplus
}
#endif
#endif /* FFP_H */
