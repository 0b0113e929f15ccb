// api.cpp — the C-ABI of libffp.so (include/ffp.h). Every entry point catches engine exceptions, stores a
// thread-local message and returns an error code; nothing here computes on the CPU.
#include <algorithm>
#include <climits>
#include <cmath>

#include "coco_eval.hpp"
#include "conv_route.hpp"
#include "det_post.hpp"
#include "eval.hpp"
#include "iqa.hpp"
#include "jpeg.hpp"
#include "png.hpp"
#include "sr_ops.hpp"
#include "scrfd.hpp"
#include "sliced.hpp"
#include "rtdetr.hpp"
#include "yolo11.hpp"

namespace ffp {
const std::string& last_error();
}

struct ffp_det { ffp::DetEngine eng; ffp_det(const void* w, size_t n, int a, int nc, int nk, int dev, int pr) : eng(w, n, a, nc, nk, dev, pr) {} };
struct ffp_rtdetr { ffp::RtdetrEngine eng; ffp_rtdetr(const void* b, size_t nb, int dev, int pr) : eng(b, nb, dev, pr) {} };
struct ffp_scrfd { ffp::ScrfdEngine eng; ffp_scrfd(const void* b, size_t nb, int n, int dev, int pr) : eng(b, nb, n, dev, pr) {} };
struct ffp_iqa { ffp::IqaEngine eng; explicit ffp_iqa(int dev) : eng(dev) {} };
struct ffp_sr { ffp::SrEngine eng; ffp_sr(const void* w, size_t n, int s, int nb, int dev, int h) : eng(w, n, s, nb, dev, h) {} };

using namespace ffp;

#define FFP_API_BEGIN try { ffp::ApiShared gate_share_;
#define FFP_API_END                                                              \
  return FFP_OK;                                                                 \
  }                                                                              \
  catch (const ffp::Error& e) { ffp::set_last_error(e.what()); return e.code; } \
  catch (const std::bad_alloc&) { ffp::set_last_error("host out of memory"); return FFP_ERR_NOMEM; } \
  catch (const std::exception& e) { ffp::set_last_error(e.what()); return FFP_ERR_STATE; }

namespace {

template <typename T> ffp::DevBuf upload(const T* src, size_t n) {
  ffp::DevBuf b(std::max<size_t>(n, 1) * sizeof(T));
  if (n) FFP_HIP(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return b;
}
void check_offsets(const int64_t* off, int n, const char* what) {
  FFP_CHECK(off && off[0] == 0, FFP_ERR_ARG, "%s offsets must start at 0", what);
  for (int i = 0; i < n; ++i) FFP_CHECK(off[i + 1] >= off[i], FFP_ERR_ARG, "%s offsets must not decrease (image %d)", what, i);
}

void upload_frame(DetEngine& e, const uint8_t* frame, int H, int W) {
  FFP_HIP(hipSetDevice(e.device()));
  ffp::upload_frame(e.scratch_frame, frame, H, W, e.stream());
}

// the host side of a Lanczos4 resize: tables built here, uploaded on `st` into `tab` (the host copy must outlive the upload)
void resize_lanczos4_dev(const void* d_src, int h, int w, int cn, int wide, int out_h, int out_w, void* d_dst, DevBuf& tab,
                         std::vector<uint8_t>& host_tab, hipStream_t st) {
  host_tab.resize(lanczos4_table_bytes(out_h, out_w));
  lanczos4_pack(lanczos4_axis(w, out_w), lanczos4_axis(h, out_h), wide, host_tab.data());
  tab.ensure(host_tab.size());
  FFP_HIP(hipMemcpyAsync(tab.p, host_tab.data(), host_tab.size(), hipMemcpyHostToDevice, st));
  launch_resize_lanczos4(d_src, h, w, cn, wide, tab.p, out_h, out_w, d_dst, st);
}

}  // namespace

extern "C" {

const char* ffp_last_error(void) { return ffp::last_error().c_str(); }
int ffp_version(void) { return 200; }

int ffp_device_count(int* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(out_n, FFP_ERR_ARG, "null output");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  (void)hipGetLastError();
  *out_n = n;
  FFP_API_END
}

int ffp_slice_bboxes(int H, int W, int sh, int sw, float oh, float ow, int32_t* out_xyxy, int cap, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(out_n, FFP_ERR_ARG, "null output");
  const std::vector<int32_t> b = slice_bboxes(H, W, sh, sw, oh, ow);
  const int n = (int)b.size() / 4;
  *out_n = n;
  if (out_xyxy && cap > 0) std::memcpy(out_xyxy, b.data(), sizeof(int32_t) * 4 * (size_t)std::min(n, cap));
  FFP_API_END
}

int ffp_tile_chunks(int n, int max_batch, int32_t* out, int cap, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(out_n, FFP_ERR_ARG, "null output");
  const std::vector<int> c = even_chunks(n, max_batch);
  *out_n = (int)c.size();
  if (out && cap > 0) std::copy(c.begin(), c.begin() + std::min((int)c.size(), cap), out);
  FFP_API_END
}

int ffp_letterbox_geometry(int h, int w, int imgsz, int32_t* out6) {
  FFP_API_BEGIN
  FFP_CHECK(out6 && h > 0 && w > 0 && imgsz > 0, FFP_ERR_ARG, "letterbox_geometry: bad arguments");
  ffp::letterbox_geometry(h, w, imgsz, out6);
  FFP_API_END
}

int ffp_det_create(const void* weights, size_t nbytes, int arch, int nc, int nkpt, int device, int precision, ffp_det** out) {
  FFP_API_BEGIN
  FFP_CHECK(out && weights, FFP_ERR_ARG, "null argument");
  *out = new ffp_det(weights, nbytes, arch, nc, nkpt, device, precision);
  FFP_API_END
}

void ffp_det_destroy(ffp_det* d) { delete d; }

int ffp_det_infer_tiles(ffp_det* d, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                        float conf, float iou, int max_det, int round_boxes, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(d && out_dets && out_counts, FFP_ERR_ARG, "null argument");
  DetEngine& e = d->eng;
  upload_frame(e, frame, H, W);
  FFP_CHECK(n_tiles > 0 && max_det >= 1 && max_det <= 1024, FFP_ERR_ARG, "n_tiles/max_det out of range");
  const size_t nd = (size_t)n_tiles * max_det * e.det_stride();
  e.scratch_dets.ensure(nd * 4);
  e.scratch_counts.ensure(sizeof(int32_t) * n_tiles);
  e.infer_tiles_dev(e.scratch_frame.as<uint8_t>(), H, W, chan_order, tiles, n_tiles, imgsz, conf, iou, max_det, round_boxes,
                    e.scratch_dets.as<float>(), e.scratch_counts.as<int32_t>());
  FFP_HIP(hipMemcpy(out_dets, e.scratch_dets.p, nd * 4, hipMemcpyDeviceToHost));
  FFP_HIP(hipMemcpy(out_counts, e.scratch_counts.p, sizeof(int32_t) * n_tiles, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_det_infer_tiles_dev(ffp_det* d, const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles,
                            int imgsz, float conf, float iou, int max_det, int round_boxes, float* d_out_dets, int32_t* d_out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(d && d_frame && d_out_dets && d_out_counts, FFP_ERR_ARG, "null argument");
  d->eng.infer_tiles_dev(d_frame, H, W, chan_order, tiles, n_tiles, imgsz, conf, iou, max_det, round_boxes, d_out_dets, d_out_counts);
  FFP_API_END
}

int ffp_det_truncate_shift_dev(ffp_det* d, float* d_dets, const int32_t* d_counts, int n_tiles, int max_det, int full_h, int full_w) {
  FFP_API_BEGIN
  FFP_CHECK(d && d_dets && d_counts && n_tiles > 0, FFP_ERR_ARG, "bad argument");
  d->eng.truncate_shift_dev(d_dets, d_counts, n_tiles, max_det, full_h, full_w);
  FFP_HIP(hipStreamSynchronize(d->eng.stream()));
  FFP_API_END
}

int ffp_det_forward_raw(ffp_det* d, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                        float* out_raw, size_t out_cap, int32_t* out_anchor_counts) {
  FFP_API_BEGIN
  FFP_CHECK(d && out_raw && out_anchor_counts, FFP_ERR_ARG, "null argument");
  DetEngine& e = d->eng;
  upload_frame(e, frame, H, W);
  e.forward_raw(e.scratch_frame.as<uint8_t>(), H, W, chan_order, tiles, n_tiles, imgsz, out_raw, out_cap, out_anchor_counts);
  FFP_API_END
}

int ffp_merge(int device, const float* dets, int n, int stride, int type, int metric, double thr, int class_agnostic, float* out,
              int32_t* out_src_index, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(out && out_n && n >= 0 && stride >= 6 && (dets || n == 0), FFP_ERR_ARG, "merge: bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "merge: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  if (n == 0) { *out_n = 0; return FFP_OK; }
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    MergeWork w;
    DevBuf rows(sizeof(float) * (size_t)n * stride), dn(sizeof(int)), dout(sizeof(float) * (size_t)n * stride), dsrc(sizeof(int) * (size_t)n),
        doutn(sizeof(int));
    FFP_HIP(hipMemcpyAsync(rows.p, dets, sizeof(float) * (size_t)n * stride, hipMemcpyHostToDevice, st));
    FFP_HIP(hipMemcpyAsync(dn.p, &n, sizeof(int), hipMemcpyHostToDevice, st));
    if (n > 1) run_merge(w, rows.as<float>(), dn.as<int>(), n, stride, type, metric, thr, class_agnostic, dout.as<float>(), dsrc.as<int>(),
                         doutn.as<int>(), n, st);
    else run_merge_passthrough(rows.as<float>(), dn.as<int>(), stride, dout.as<float>(), dsrc.as<int>(), doutn.as<int>(), n, st);
    int k = 0;
    FFP_HIP(hipMemcpyAsync(&k, doutn.p, sizeof(int), hipMemcpyDeviceToHost, st));
    FFP_HIP(hipStreamSynchronize(st));
    FFP_HIP(hipMemcpy(out, dout.p, sizeof(float) * (size_t)k * stride, hipMemcpyDeviceToHost));
    if (out_src_index) FFP_HIP(hipMemcpy(out_src_index, dsrc.p, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost));
    *out_n = k;
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

int ffp_merge_dev(ffp_det* d, const float* d_dets, const int32_t* d_counts, int n_slices, int max_det, int type, int metric, double thr,
                  int class_agnostic, float* d_out, int cap, int32_t* d_out_n) {
  FFP_API_BEGIN
  FFP_CHECK(d && d_dets && d_counts && d_out && d_out_n && n_slices > 0 && cap > 0, FFP_ERR_ARG, "merge_dev: bad arguments");
  d->eng.merge_dev(d_dets, d_counts, n_slices, max_det, type, metric, thr, class_agnostic, d_out, nullptr, cap, d_out_n);
  FFP_API_END
}

// shared body of ffp_sliced_predict / ffp_det_stage_dev: detections of this rank's share of [slices..., full frame]
static void stage(DetEngine& e, const uint8_t* d_frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                  int perform_standard_pred, int imgsz, float conf, float iou, int max_det, int round_boxes, int rank, int world,
                  float* d_dets, int32_t* d_counts, int* n_local, int* n_total) {
  FFP_CHECK(world >= 1 && rank >= 0 && rank < world, FFP_ERR_ARG, "rank %d of %d", rank, world);
  const std::vector<int32_t> items = sliced_items(H, W, slice_h, slice_w, oh, ow, perform_standard_pred);
  const int total = (int)items.size() / 4;
  const int per = (total + world - 1) / world;
  const int lo = std::min(rank * per, total), hi = std::min(lo + per, total);
  *n_total = total;
  *n_local = hi - lo;
  if (hi > lo) {
    e.infer_tiles_dev(d_frame, H, W, chan_order, items.data() + 4 * lo, hi - lo, imgsz, conf, iou, max_det, round_boxes, d_dets, d_counts);
    e.truncate_shift_dev(d_dets, d_counts, hi - lo, max_det, H, W);
  }
}

int ffp_sliced_predict(ffp_det* d, const uint8_t* frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                       int perform_standard_pred, int imgsz, float conf, float iou, int max_det, int round_boxes, int pp_type,
                       int pp_metric, double pp_thr, int class_agnostic, float* out, int cap, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(d && out && out_n && cap > 0, FFP_ERR_ARG, "null argument");
  DetEngine& e = d->eng;
  upload_frame(e, frame, H, W);
  const int total = (int)sliced_items(H, W, slice_h, slice_w, oh, ow, perform_standard_pred).size() / 4;
  const int stride = e.det_stride();
  e.scratch_dets.ensure(sizeof(float) * (size_t)total * max_det * stride);
  e.scratch_counts.ensure(sizeof(int32_t) * total);
  int nl = 0, nt = 0;
  stage(e, e.scratch_frame.as<uint8_t>(), H, W, chan_order, slice_h, slice_w, oh, ow, perform_standard_pred, imgsz, conf, iou, max_det,
        round_boxes, 0, 1, e.scratch_dets.as<float>(), e.scratch_counts.as<int32_t>(), &nl, &nt);
  e.tail.reserve(cap, stride);
  e.merge_dev(e.scratch_dets.as<float>(), e.scratch_counts.as<int32_t>(), total, max_det, pp_type, pp_metric, pp_thr, class_agnostic,
              e.tail.merged.as<float>(), nullptr, cap, e.tail.merged_n.as<int32_t>());
  e.tail.fetch(out, cap, stride, out_n, "sliced_predict", nullptr);      // merge_dev has drained the stream
  FFP_API_END
}

int ffp_det_stage_dev(ffp_det* d, const uint8_t* d_frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                      int perform_standard_pred, int imgsz, float conf, float iou, int max_det, int round_boxes, int rank, int world,
                      float* d_local_dets, int32_t* d_local_counts, int32_t* out_n_local, int32_t* out_n_total) {
  FFP_API_BEGIN
  FFP_CHECK(d && d_frame && d_local_dets && d_local_counts && out_n_local && out_n_total, FFP_ERR_ARG, "null argument");
  int nl = 0, nt = 0;
  stage(d->eng, d_frame, H, W, chan_order, slice_h, slice_w, oh, ow, perform_standard_pred, imgsz, conf, iou, max_det, round_boxes, rank,
        world, d_local_dets, d_local_counts, &nl, &nt);
  *out_n_local = nl;
  *out_n_total = nt;
  FFP_API_END
}

int ffp_det_set_lanes(ffp_det* d, int mode) {
  FFP_API_BEGIN
  FFP_CHECK(d && mode >= 0 && mode <= 3, FFP_ERR_ARG, "det_set_lanes: mode %d outside [0,3]", mode);
  FFP_HIP(hipSetDevice(d->eng.device()));
  FFP_HIP(hipStreamSynchronize(d->eng.stream()));
  d->eng.set_lanes(mode);
  FFP_API_END
}

int ffp_det_set_buffer_reuse(ffp_det* d, int mode) {
  FFP_API_BEGIN
  FFP_CHECK(d && mode >= 0 && mode <= 2, FFP_ERR_ARG, "det_set_buffer_reuse: mode %d outside [0,2]", mode);
  FFP_HIP(hipSetDevice(d->eng.device()));
  FFP_HIP(hipStreamSynchronize(d->eng.stream()));
  d->eng.set_buffer_reuse(mode);
  FFP_API_END
}

int ffp_det_set_gate(ffp_det* d, int on) {
  FFP_API_BEGIN
  FFP_CHECK(d, FFP_ERR_ARG, "null handle");
  d->eng.set_gate(on != 0);
  FFP_API_END
}

int ffp_det_last_active(ffp_det* d, int32_t* out_active, int32_t* out_items) {
  FFP_API_BEGIN
  FFP_CHECK(d && out_active && out_items, FFP_ERR_ARG, "null argument");
  int a = 0, n = 0;
  d->eng.last_active(&a, &n);
  *out_active = a;
  *out_items = n;
  FFP_API_END
}

int ffp_det_stream_wait_event(ffp_det* d, void* hip_event) {
  FFP_API_BEGIN
  FFP_CHECK(d && hip_event, FFP_ERR_ARG, "det_stream_wait_event: null argument");
  FFP_HIP(hipSetDevice(d->eng.device()));
  FFP_HIP(hipStreamWaitEvent(d->eng.stream(), reinterpret_cast<hipEvent_t>(hip_event), 0));
  FFP_API_END
}

int ffp_det_graph_status(ffp_det* d, int32_t* out_state) {
  FFP_API_BEGIN
  FFP_CHECK(d && out_state, FFP_ERR_ARG, "null argument");
  *out_state = d->eng.last_graph_state;
  FFP_API_END
}

int ffp_det_last_ms(ffp_det* d, int stage_id, float* out_ms) {
  FFP_API_BEGIN
  FFP_CHECK(d && out_ms && stage_id >= 0 && stage_id < 5, FFP_ERR_ARG, "bad argument");
  *out_ms = d->eng.last_ms[stage_id];
  FFP_API_END
}

int ffp_det_last_conv_stats(ffp_det* d, double* out_flops, float* out_ms, int32_t* out_launches) {
  FFP_API_BEGIN
  FFP_CHECK(d, FFP_ERR_ARG, "null handle");
  if (out_flops) *out_flops = d->eng.last_conv_flops;
  if (out_launches) *out_launches = d->eng.last_conv_launches;
  if (out_ms) { double ms = 0; for (auto& kv : d->eng.prof.table) ms += kv.second.ms; *out_ms = (float)ms; }
  FFP_API_END
}

static int profile_get(ConvProfile& p, int i, char* name, int cap, double* flops, float* ms, int32_t* launches) {
  if (i < 0 || i >= (int)p.table.size()) return FFP_ERR_ARG;
  auto it = p.table.begin();
  std::advance(it, i);
  if (name && cap > 0) { std::snprintf(name, cap, "%s", it->second.variant.c_str()); }
  if (flops) *flops = it->second.flops;
  if (ms) *ms = (float)it->second.ms;
  if (launches) *launches = it->second.launches;
  return FFP_OK;
}

static int profile_bytes(ConvProfile& p, int i, double* bytes) {
  if (i < 0 || i >= (int)p.table.size() || !bytes) return FFP_ERR_ARG;
  auto it = p.table.begin();
  std::advance(it, i);
  *bytes = it->second.bytes;
  return FFP_OK;
}

static int detail_get(ConvProfile& p, int i, char* name, int cap, double* flops, float* ms) {
  if (i < 0 || i >= (int)p.detail.size()) return FFP_ERR_ARG;
  if (name && cap > 0) std::snprintf(name, cap, "%s", p.detail[i].variant.c_str());
  if (flops) *flops = p.detail[i].flops;
  if (ms) *ms = (float)p.detail[i].ms;
  return FFP_OK;
}
int ffp_det_profile_detail(ffp_det* d, int i, char* name, int cap, double* flops, float* ms) { return d ? detail_get(d->eng.prof, i, name, cap, flops, ms) : FFP_ERR_ARG; }
int ffp_sr_profile_detail(ffp_sr* s, int i, char* name, int cap, double* flops, float* ms) { return s ? detail_get(s->eng.prof, i, name, cap, flops, ms) : FFP_ERR_ARG; }

int ffp_det_set_profile(ffp_det* d, int enable) { if (!d) return FFP_ERR_ARG; d->eng.prof.enabled = enable != 0; return FFP_OK; }
int ffp_det_profile_count(ffp_det* d, int32_t* n) { if (!d || !n) return FFP_ERR_ARG; *n = (int)d->eng.prof.table.size(); return FFP_OK; }
int ffp_det_profile_get(ffp_det* d, int i, char* name, int cap, double* flops, float* ms, int32_t* launches) {
  if (!d) return FFP_ERR_ARG;
  return profile_get(d->eng.prof, i, name, cap, flops, ms, launches);
}

// ---- super-resolution ---------------------------------------------------------------------------------------------------
int ffp_sr_create(const void* weights, size_t nbytes, int scale, int num_block, int device, int half, ffp_sr** out) {
  FFP_API_BEGIN
  FFP_CHECK(out && weights, FFP_ERR_ARG, "null argument");
  *out = new ffp_sr(weights, nbytes, scale, num_block, device, half);
  FFP_API_END
}

void ffp_sr_destroy(ffp_sr* s) { delete s; }

int ffp_sr_enhance_batch(ffp_sr* s, int n, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws, int tile, int tile_pad,
                         int pre_pad, uint8_t* const* outs) {
  FFP_API_BEGIN
  FFP_CHECK(s && n > 0 && imgs && hs && ws && outs, FFP_ERR_ARG, "bad argument");
  SrEngine& e = s->eng;
  FFP_HIP(hipSetDevice(e.device()));
  const int sc = e.scale();
  std::vector<SrImage> v(n);
  size_t in_tot = 0, out_tot = 0;
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(imgs[i] && outs[i] && hs[i] > 0 && ws[i] > 0, FFP_ERR_ARG, "image %d is null or empty", i);
    v[i].in_off = (long long)in_tot; v[i].in_stride = ws[i] * 3; v[i].h = hs[i]; v[i].w = ws[i];
    v[i].out_off = (long long)out_tot; v[i].out_stride = ws[i] * sc * 3;
    in_tot += ((size_t)hs[i] * ws[i] * 3 + 15) / 16 * 16;
    out_tot += ((size_t)hs[i] * sc * ws[i] * sc * 3 + 15) / 16 * 16;
  }
  e.scratch_in.ensure(in_tot);
  e.scratch_out.ensure(out_tot);
  for (int i = 0; i < n; ++i)
    FFP_HIP(hipMemcpyAsync(e.scratch_in.as<uint8_t>() + v[i].in_off, imgs[i], (size_t)hs[i] * ws[i] * 3, hipMemcpyHostToDevice, e.stream()));
  e.enhance_dev(e.scratch_in.as<uint8_t>(), e.scratch_out.as<uint8_t>(), v, tile, tile_pad, pre_pad);
  for (int i = 0; i < n; ++i)
    FFP_HIP(hipMemcpy(outs[i], e.scratch_out.as<uint8_t>() + v[i].out_off, (size_t)hs[i] * sc * ws[i] * sc * 3, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_sr_enhance(ffp_sr* s, const uint8_t* bgr, int h, int w, int tile, int tile_pad, int pre_pad, uint8_t* out_bgr) {
  const uint8_t* ins[1] = {bgr};
  uint8_t* outs[1] = {out_bgr};
  const int32_t hs[1] = {h}, ws[1] = {w};
  return ffp_sr_enhance_batch(s, 1, ins, hs, ws, tile, tile_pad, pre_pad, outs);
}

// realesrgan 0.3.0 RealESRGANer.enhance for every layout (reference call utils/enhancer.py:214; rules in include/ffp.h):
// the colour image and, for alpha_mode REALESRGAN, the alpha plane go through the network as ONE ragged batch (two SrImages
// over the same input / canvas, differing in their channel selection); the LINEAR alpha and the Lanczos4 outscale follow on
// the enhancer's stream, and the final buffer is copied to the host once.
int ffp_sr_enhance_ex(ffp_sr* s, const void* img, int h, int w, int channels, int bits, int max_range, int alpha_mode, int out_h, int out_w,
                      int tile, int tile_pad, int pre_pad, void* out) {
  FFP_API_BEGIN
  FFP_CHECK(s && img && out, FFP_ERR_ARG, "null argument");
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, FFP_ERR_ARG, "empty image (%dx%d -> %dx%d)", h, w, out_h, out_w);
  FFP_CHECK(channels == 1 || channels == 3 || channels == 4, FFP_ERR_ARG, "channels %d (1, 3 or 4)", channels);
  FFP_CHECK(bits == 8 || bits == 16, FFP_ERR_ARG, "bits %d (8 or 16)", bits);
  FFP_CHECK(max_range == 255 || (max_range == 65535 && bits == 16), FFP_ERR_ARG, "max_range %d with %d-bit input", max_range, bits);
  FFP_CHECK(alpha_mode == FFP_SR_ALPHA_REALESRGAN || alpha_mode == FFP_SR_ALPHA_LINEAR, FFP_ERR_ARG, "alpha_mode %d", alpha_mode);
  SrEngine& e = s->eng;
  FFP_HIP(hipSetDevice(e.device()));
  e.wait_done();                      // one enhancement in flight per handle: its scratch buffers are about to be reused
  const int sc = e.scale();
  const int ch = h * sc, cw = w * sc;
  SrFmt fin, fout;
  fin.cn = fout.cn = channels;
  fin.wide = bits == 16;
  fout.wide = max_range == 65535;
  fin.range = fout.range = (float)max_range;
  fin.sel = fout.sel = channels == 1 ? SR_SEL_GRAY : SR_SEL_BGR;
  const size_t in_bytes = (size_t)h * w * fin.px_bytes(), canvas_bytes = (size_t)ch * cw * fout.px_bytes();
  const size_t out_bytes = (size_t)out_h * out_w * fout.px_bytes();
  const bool resize = out_h != ch || out_w != cw;
  const size_t final_off = resize ? (canvas_bytes + 255) / 256 * 256 : 0;
  e.scratch_in.ensure(in_bytes);
  e.scratch_out.ensure(final_off + (resize ? out_bytes : canvas_bytes));
  FFP_HIP(hipMemcpyAsync(e.scratch_in.p, img, in_bytes, hipMemcpyHostToDevice, e.stream()));
  std::vector<SrImage> v(1);
  v[0].in_off = 0; v[0].in_stride = w * fin.px_bytes(); v[0].h = h; v[0].w = w;
  v[0].out_off = 0; v[0].out_stride = cw * fout.px_bytes();
  v[0].in_fmt = fin; v[0].out_fmt = fout;
  if (channels == 4 && alpha_mode == FFP_SR_ALPHA_REALESRGAN) {
    v.push_back(v[0]);
    v[1].in_fmt.sel = v[1].out_fmt.sel = SR_SEL_ALPHA;
  }
  e.enhance_dev(e.scratch_in.as<uint8_t>(), e.scratch_out.as<uint8_t>(), v, tile, tile_pad, pre_pad, false);
  if (channels == 4 && alpha_mode == FFP_SR_ALPHA_LINEAR)
    launch_alpha_linear(e.scratch_in.p, h, w, fin.wide, fin.range, ch, cw, e.scratch_out.p, fout.wide, e.stream());
  std::vector<uint8_t> host_tab;
  if (resize)
    resize_lanczos4_dev(e.scratch_out.p, ch, cw, channels, fout.wide, out_h, out_w, e.scratch_out.as<uint8_t>() + final_off, e.scratch_tab,
                        host_tab, e.stream());
  e.wait_done();
  FFP_HIP(hipMemcpy(out, e.scratch_out.as<uint8_t>() + final_off, out_bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

// crops of one or several resident frames (frame_of_box == nullptr: all from d_frames[0]) -> one ragged SR batch
static int sr_crops_impl(ffp_sr* s, int n_frames, const uint8_t* const* d_frames, const int32_t* frame_of_box, int H, int W,
                         const int32_t* boxes, int n, int tile, int tile_pad, uint8_t* d_out, size_t out_cap, int64_t* out_offsets, bool wait) {
  FFP_API_BEGIN
  FFP_CHECK(s && d_frames && n_frames > 0 && boxes && n > 0 && d_out && out_offsets, FFP_ERR_ARG, "bad argument");
  SrEngine& e = s->eng;
  FFP_HIP(hipSetDevice(e.device()));
  e.wait_done();                      // one enhancement in flight per handle: its scratch and plan tables are about to be reused
  const int sc = e.scale();
  std::vector<SrImage> v;
  v.reserve(n);
  // box / offset tables go through pinned staging so that the uploads are asynchronous on the enhancer's stream
  e.crop_stage.ensure((sizeof(int4) + sizeof(long long)) * (size_t)n);
  int4* hb = reinterpret_cast<int4*>(e.crop_stage.p);
  long long* offs = reinterpret_cast<long long*>(hb + n);
  std::vector<int> fidx;
  size_t in_tot = 0, out_tot = 0;
  for (int i = 0; i < n; ++i) {
    const int fi = frame_of_box ? frame_of_box[i] : 0;
    FFP_CHECK(fi >= 0 && fi < n_frames && d_frames[fi], FFP_ERR_ARG, "crop %d refers to frame %d of %d", i, fi, n_frames);
    // utils/visualization.py:204-213: int box, clamp to the frame; an empty crop is skipped (`if face_crop.size > 0`),
    // here: a zero-length entry in out_offsets
    const int x1 = std::max(0, boxes[4 * i]), y1 = std::max(0, boxes[4 * i + 1]);
    const int x2 = std::min(W, boxes[4 * i + 2]), y2 = std::min(H, boxes[4 * i + 3]);
    out_offsets[i] = (int64_t)out_tot;
    if (x2 <= x1 || y2 <= y1) continue;
    const int w = x2 - x1, h = y2 - y1;
    const int k = (int)v.size();
    hb[k] = make_int4(x1, y1, w, h);
    offs[k] = (long long)in_tot;
    fidx.push_back(fi);
    SrImage im;
    im.in_off = (long long)in_tot; im.in_stride = w * 3; im.h = h; im.w = w;
    im.out_off = (long long)out_tot; im.out_stride = w * sc * 3;
    v.push_back(im);
    in_tot += ((size_t)h * w * 3 + 15) / 16 * 16;
    out_tot += ((size_t)h * sc * w * sc * 3 + 15) / 16 * 16;
  }
  out_offsets[n] = (int64_t)out_tot;
  FFP_CHECK(out_tot <= out_cap, FFP_ERR_ARG, "output needs %zu bytes, capacity %zu", out_tot, out_cap);
  const int m = (int)v.size();
  if (m == 0) return FFP_OK;          // every crop was empty: nothing to enhance
  e.scratch_in.ensure(in_tot);
  e.scratch_boxes.ensure(sizeof(int4) * m);
  e.scratch_offs.ensure(sizeof(long long) * m);
  // the offsets sit behind n (not m) boxes in the staging block
  FFP_HIP(hipMemcpyAsync(e.scratch_boxes.p, hb, sizeof(int4) * m, hipMemcpyHostToDevice, e.stream()));
  FFP_HIP(hipMemcpyAsync(e.scratch_offs.p, offs, sizeof(long long) * m, hipMemcpyHostToDevice, e.stream()));
  // boxes are gathered frame by frame (contiguous runs of equal frame index)
  for (int i0 = 0; i0 < m;) {
    const int fi = fidx[i0];
    int i1 = i0 + 1;
    while (i1 < m && fidx[i1] == fi) ++i1;
    launch_crop_gather(d_frames[fi], W, e.scratch_boxes.as<int4>() + i0, e.scratch_offs.as<long long>() + i0, i1 - i0,
                       e.scratch_in.as<uint8_t>(), e.stream());
    i0 = i1;
  }
  // FaceEnhancer enhances every crop with its tile setting (tile 400 / pad 10: utils/enhancer.py:21,135-142,214)
  e.enhance_dev(e.scratch_in.as<uint8_t>(), d_out, v, tile, tile_pad, 0, wait);
  FFP_API_END
}

int ffp_sr_enhance_dev(ffp_sr* s, const uint8_t* d_bgr, int h, int w, int tile, int tile_pad, int pre_pad, uint8_t* d_out) {
  FFP_API_BEGIN
  FFP_CHECK(s && d_bgr && d_out, FFP_ERR_ARG, "null argument");
  FFP_CHECK(h >= 1 && w >= 1, FFP_ERR_ARG, "empty image");
  SrImage im;
  im.in_off = 0; im.in_stride = w * 3; im.h = h; im.w = w;
  im.out_off = 0; im.out_stride = w * s->eng.scale() * 3;
  s->eng.enhance_dev(d_bgr, d_out, {im}, tile, tile_pad, pre_pad);
  FFP_API_END
}

int ffp_sr_enhance_crops_dev(ffp_sr* s, const uint8_t* d_frame, int H, int W, const int32_t* boxes, int n, int tile, int tile_pad, uint8_t* d_out,
                             size_t out_cap, int64_t* out_offsets) {
  return sr_crops_impl(s, 1, &d_frame, nullptr, H, W, boxes, n, tile, tile_pad, d_out, out_cap, out_offsets, true);
}

int ffp_sr_enhance_crops_dev_async(ffp_sr* s, const uint8_t* d_frame, int H, int W, const int32_t* boxes, int n, int tile, int tile_pad,
                                   uint8_t* d_out, size_t out_cap, int64_t* out_offsets) {
  return sr_crops_impl(s, 1, &d_frame, nullptr, H, W, boxes, n, tile, tile_pad, d_out, out_cap, out_offsets, false);
}

int ffp_sr_enhance_crops_multi_dev_async(ffp_sr* s, int n_frames, const uint8_t* const* d_frames, const int32_t* frame_of_box, int H, int W,
                                         const int32_t* boxes, int n, int tile, int tile_pad, uint8_t* d_out, size_t out_cap, int64_t* out_offsets) {
  return sr_crops_impl(s, n_frames, d_frames, frame_of_box, H, W, boxes, n, tile, tile_pad, d_out, out_cap, out_offsets, false);
}

int ffp_sr_wait(ffp_sr* s) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.wait_done();
  FFP_API_END
}

int ffp_sr_plan_state(ffp_sr* s, int32_t* out_plans_built, int32_t* out_last_graph) {
  if (!s) return FFP_ERR_ARG;
  if (out_plans_built) *out_plans_built = s->eng.plans_built;
  if (out_last_graph) *out_last_graph = s->eng.last_graph ? 1 : 0;
  return FFP_OK;
}

int ffp_sr_set_fused_body(ffp_sr* s, int on) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.set_fused_body(on != 0);
  FFP_API_END
}

int ffp_sr_mem_bytes(ffp_sr* s, uint64_t* out_weight_bytes, uint64_t* out_plan_bytes, int32_t* out_plans_resident) {
  if (!s) return FFP_ERR_ARG;
  if (out_weight_bytes) *out_weight_bytes = s->eng.weight_bytes();
  if (out_plan_bytes) *out_plan_bytes = s->eng.plan_bytes();
  if (out_plans_resident) *out_plans_resident = s->eng.plans_resident();
  return FFP_OK;
}

int ffp_det_mem_bytes(ffp_det* d, uint64_t* out_weight_bytes, uint64_t* out_plan_bytes, int32_t* out_plans_resident) {
  if (!d) return FFP_ERR_ARG;
  if (out_weight_bytes) *out_weight_bytes = d->eng.weight_bytes();
  if (out_plan_bytes) *out_plan_bytes = d->eng.plan_bytes();
  if (out_plans_resident) *out_plans_resident = d->eng.plans_resident();
  return FFP_OK;
}

int ffp_det_mem_detail(ffp_det* d, uint64_t* out_activation_bytes, uint64_t* out_no_reuse_bytes, uint64_t* out_peak_live_bytes) {
  if (!d) return FFP_ERR_ARG;
  size_t a = 0, n = 0, p = 0;
  d->eng.mem_detail(&a, &n, &p);
  if (out_activation_bytes) *out_activation_bytes = a;
  if (out_no_reuse_bytes) *out_no_reuse_bytes = n;
  if (out_peak_live_bytes) *out_peak_live_bytes = p;
  return FFP_OK;
}

int ffp_det_fill_steps(ffp_det* d, int32_t* out_fill_steps, int32_t* out_ranges_freed) {
  if (!d) return FFP_ERR_ARG;
  int f = 0, r = 0;
  d->eng.fill_counts(&f, &r);
  if (out_fill_steps) *out_fill_steps = f;
  if (out_ranges_freed) *out_ranges_freed = r;
  return FFP_OK;
}

int ffp_det_drop_plans(ffp_det* d) {
  FFP_API_BEGIN
  FFP_CHECK(d, FFP_ERR_ARG, "null handle");
  d->eng.drop_plans();
  FFP_API_END
}

int ffp_sr_drop_plans(ffp_sr* s) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.drop_plans();
  FFP_API_END
}

int ffp_sr_last_ms(ffp_sr* s, float* out_ms) { if (!s || !out_ms) return FFP_ERR_ARG; *out_ms = s->eng.last_ms; return FFP_OK; }
int ffp_sr_last_conv_stats(ffp_sr* s, double* out_flops, float* out_ms, int32_t* out_launches) {
  if (!s) return FFP_ERR_ARG;
  if (out_flops) *out_flops = s->eng.last_conv_flops;
  if (out_launches) *out_launches = s->eng.last_conv_launches;
  if (out_ms) { double ms = 0; for (auto& kv : s->eng.prof.table) ms += kv.second.ms; *out_ms = (float)ms; }
  return FFP_OK;
}
int ffp_sr_set_profile(ffp_sr* s, int enable) { if (!s) return FFP_ERR_ARG; s->eng.prof.enabled = enable != 0; return FFP_OK; }
int ffp_sr_profile_count(ffp_sr* s, int32_t* n) { if (!s || !n) return FFP_ERR_ARG; *n = (int)s->eng.prof.table.size(); return FFP_OK; }
int ffp_sr_profile_get(ffp_sr* s, int i, char* name, int cap, double* flops, float* ms, int32_t* launches) {
  if (!s) return FFP_ERR_ARG;
  return profile_get(s->eng.prof, i, name, cap, flops, ms, launches);
}

int ffp_det_profile_bytes(ffp_det* d, int i, double* out_bytes) { return d ? profile_bytes(d->eng.prof, i, out_bytes) : FFP_ERR_ARG; }
int ffp_sr_profile_bytes(ffp_sr* s, int i, double* out_bytes) { return s ? profile_bytes(s->eng.prof, i, out_bytes) : FFP_ERR_ARG; }

int ffp_conv_totals_enable(int on) {
  conv_totals_enable(on != 0);
  return FFP_OK;
}

int ffp_conv_totals_count(int32_t* out_n) {
  if (!out_n) return FFP_ERR_ARG;
  *out_n = (int32_t)conv_totals().size();
  return FFP_OK;
}

int ffp_conv_totals_get(int i, char* name, int cap, double* flops, double* bytes, int64_t* launches) {
  const auto v = conv_totals();
  if (i < 0 || i >= (int)v.size()) return FFP_ERR_ARG;
  if (name && cap > 0) std::snprintf(name, cap, "%s", v[i].variant.c_str());
  if (flops) *flops = v[i].flops;
  if (bytes) *bytes = v[i].bytes;
  if (launches) *launches = v[i].launches;
  return FFP_OK;
}

// ---- single operator (parity tests) ------------------------------------------------------------------------------------------
// ---- WIDER FACE evaluation -----------------------------------------------------------------------------------
int ffp_eval_wider_pr(int device, const double* preds, const int64_t* pred_off, const double* gts, const int64_t* gt_off, const uint8_t* evaluate,
                      int n_img, double iou_thr, int thresh_num, int64_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0 && thresh_num > 0 && out_counts, FFP_ERR_ARG, "eval_wider_pr: bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "eval_wider_pr: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  check_offsets(pred_off, n_img, "prediction");
  check_offsets(gt_off, n_img, "face");
  const int64_t np = pred_off[n_img], ng = gt_off[n_img];
  FFP_CHECK((np == 0 || preds) && (ng == 0 || (gts && evaluate)), FFP_ERR_ARG, "eval_wider_pr: null data");
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    DevBuf dp = upload(preds, (size_t)np * 5), dpo = upload(pred_off, (size_t)n_img + 1), dg = upload(gts, (size_t)ng * 4), dgo = upload(gt_off, (size_t)n_img + 1),
           de = upload(evaluate, (size_t)ng), state(sizeof(int) * (size_t)(ng + 2 * np + 1)), counts(sizeof(unsigned long long) * 2 * thresh_num);
    launch_wider_pr(dp.as<double>(), dpo.as<long long>(), dg.as<double>(), dgo.as<long long>(), de.as<unsigned char>(), n_img, iou_thr, thresh_num,
                    state.as<int>(), np, ng, counts.as<unsigned long long>(), st);
    FFP_HIP(hipStreamSynchronize(st));
    FFP_HIP(hipMemcpy(out_counts, counts.p, sizeof(int64_t) * 2 * thresh_num, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

int ffp_eval_dual_match(int device, const double* preds, const int64_t* pred_off, const double* faces, const int64_t* face_off, const uint8_t* valid,
                        int n_img, double iou_thr, int32_t* out_flags) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0, FFP_ERR_ARG, "eval_dual_match: bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "eval_dual_match: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  check_offsets(pred_off, n_img, "prediction");
  check_offsets(face_off, n_img, "face");
  const int64_t np = pred_off[n_img], nf = face_off[n_img];
  FFP_CHECK((np == 0 || (preds && out_flags)) && (nf == 0 || (faces && valid)), FFP_ERR_ARG, "eval_dual_match: null data");
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    DevBuf dp = upload(preds, (size_t)np * 5), dpo = upload(pred_off, (size_t)n_img + 1), df = upload(faces, (size_t)nf * 4), dfo = upload(face_off, (size_t)n_img + 1),
           dv = upload(valid, (size_t)nf), state(sizeof(int) * (size_t)(nf + 1)), flags(sizeof(int) * (size_t)(np + 1));
    launch_dual_match(dp.as<double>(), dpo.as<long long>(), df.as<double>(), dfo.as<long long>(), dv.as<unsigned char>(), n_img, iou_thr, state.as<int>(), nf,
                      flags.as<int>(), st);
    FFP_HIP(hipStreamSynchronize(st));
    if (np) FFP_HIP(hipMemcpy(out_flags, flags.p, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

// ---- NIQE (pyiqa.create_metric('niqe')) ------------------------------------------------------------------------------------------
int ffp_iqa_create(int device, ffp_iqa** out) {
  FFP_API_BEGIN
  FFP_CHECK(out, FFP_ERR_ARG, "iqa_create: null output");
  *out = new ffp_iqa(device);
  FFP_API_END
}

void ffp_iqa_destroy(ffp_iqa* q) { delete q; }

int ffp_iqa_niqe_blocks(int h, int w, int64_t* out_blocks) {
  if (!out_blocks || h <= 0 || w <= 0) { ffp::set_last_error("iqa_niqe_blocks: bad arguments"); return FFP_ERR_ARG; }
  *out_blocks = niqe_blocks(h, w);
  return FFP_OK;
}

int ffp_iqa_niqe_features(ffp_iqa* q, int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout,
                          int chan_order, int on_device, double* out_feat, double* out_sharp, int64_t cap_blocks, int64_t* out_block_off) {
  FFP_API_BEGIN
  FFP_CHECK(q, FFP_ERR_ARG, "iqa_niqe_features: null handle");
  q->eng.niqe_features(n, imgs, h, w, c, layout, chan_order, on_device != 0, out_feat, out_sharp, cap_blocks, out_block_off);
  FFP_API_END
}

int ffp_iqa_niqe_luma(ffp_iqa* q, const void* img, int h, int w, int c, int layout, int chan_order, float* out_y) {
  FFP_API_BEGIN
  FFP_CHECK(q, FFP_ERR_ARG, "iqa_niqe_luma: null handle");
  q->eng.luma(img, h, w, c, layout, chan_order, out_y);
  FFP_API_END
}

int ffp_iqa_niqe_score(const double* feat, const int64_t* block_off, int n, const double* mu, const double* cov, double* out_scores) {
  FFP_API_BEGIN
    FFP_CHECK(n >= 0 && mu && cov && out_scores, FFP_ERR_ARG, "iqa_niqe_score: bad arguments");
    check_offsets(block_off, n, "block");
    FFP_CHECK(block_off[n] == 0 || feat, FFP_ERR_ARG, "iqa_niqe_score: null features");
    niqe_score(feat, block_off, n, mu, cov, out_scores);
  FFP_API_END
}

// ---- COCO bbox evaluation (pycocotools COCOeval.evaluate + accumulate) ----------------------------------------------------------
int ffp_eval_coco_bbox(int device, int n_img, int n_cat, const double* dets, const int64_t* det_off, const double* gts, const int64_t* gt_off,
                       const double* iou_thrs, int n_iou, const double* rec_thrs, int n_rec, const double* area_rng, int n_area,
                       const int32_t* max_dets, int n_max_dets, double* precision, double* recall, double* scores, double* dt_matches,
                       uint8_t* dt_ignore, double* gt_matches, uint8_t* gt_ignore) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0 && n_cat >= 0 && n_iou > 0 && n_rec > 0 && n_area > 0 && n_max_dets > 0, FFP_ERR_ARG, "eval_coco_bbox: bad sizes");
  FFP_CHECK(iou_thrs && rec_thrs && area_rng && max_dets && precision && recall && scores, FFP_ERR_ARG, "eval_coco_bbox: null parameter or output");
  const long long U = (long long)n_img * n_cat;
  FFP_CHECK(U <= INT_MAX && U * n_area * n_iou <= INT_MAX && (long long)n_cat * n_area * n_max_dets * n_iou <= INT_MAX, FFP_ERR_ARG,
            "eval_coco_bbox: %lld units x %d areas x %d thresholds is too large", U, n_area, n_iou);
  for (int m = 0; m < n_max_dets; ++m)
    FFP_CHECK(max_dets[m] >= 0 && (m == 0 || max_dets[m] >= max_dets[m - 1]), FFP_ERR_ARG, "eval_coco_bbox: maxDets must be ascending and >= 0");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "eval_coco_bbox: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  check_offsets(det_off, (int)U, "detection");
  check_offsets(gt_off, (int)U, "ground-truth");
  const int64_t nd = det_off[U], ng = gt_off[U];
  FFP_CHECK((nd == 0 || dets) && (ng == 0 || gts), FFP_ERR_ARG, "eval_coco_bbox: null data");
  std::vector<int64_t> cut_off((size_t)U + 1, 0);
  const int64_t max_det = max_dets[n_max_dets - 1];
  for (long long u = 0; u < U; ++u) {
    FFP_CHECK(det_off[u + 1] - det_off[u] <= INT_MAX && gt_off[u + 1] - gt_off[u] <= INT_MAX, FFP_ERR_ARG, "eval_coco_bbox: unit %lld is too large", u);
    cut_off[u + 1] = cut_off[u] + std::min<int64_t>(det_off[u + 1] - det_off[u], max_det);
  }
  const int64_t ndc = cut_off[U];
  FFP_CHECK(ndc <= (1LL << 30), FFP_ERR_ARG, "eval_coco_bbox: %lld detections after the maxDets cut is too many", (long long)ndc);
  for (int64_t i = 0; i < nd; ++i)   // loadRes numbers dets from 1: a GT is taken when gtMatches > 0, so every id must be positive
    FFP_CHECK(!std::isnan(dets[i * 7 + 4]) && dets[i * 7 + 6] > 0, FFP_ERR_ARG, "eval_coco_bbox: detection %lld has a NaN score or an id <= 0", (long long)i);
  for (int64_t g = 0; g < ng; ++g)   // _prepare sets ignore = iscrowd: a crowd GT is always ignored (at most one TP per kept GT)
    FFP_CHECK(gts[g * 8 + 5] == 0 || gts[g * 8 + 6] != 0, FFP_ERR_ARG, "eval_coco_bbox: ground truth %lld is a crowd but not ignored", (long long)g);
  const int T = n_iou, R = n_rec, A = n_area, M = n_max_dets, K = n_cat;
  const size_t n_pr = (size_t)T * R * K * A * M, n_rc = (size_t)T * K * A * M;
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    DevBuf dd = upload(dets, (size_t)nd * 7), ddo = upload(det_off, (size_t)U + 1), dg = upload(gts, (size_t)ng * 8), dgo = upload(gt_off, (size_t)U + 1),
           dco = upload(cut_off.data(), cut_off.size()), dit = upload(iou_thrs, (size_t)T), drt = upload(rec_thrs, (size_t)R),
           dar = upload(area_rng, (size_t)A * 2), dmd = upload(max_dets, (size_t)M);
    DevBuf dprec(sizeof(double) * std::max<size_t>(n_pr, 1)), drec(sizeof(double) * std::max<size_t>(n_rc, 1)), dsc(sizeof(double) * std::max<size_t>(n_pr, 1)),
           ddtm(sizeof(double) * (size_t)A * T * std::max<int64_t>(ndc, 1)), ddig((size_t)A * T * std::max<int64_t>(ndc, 1)),
           dgtm(sizeof(double) * (size_t)A * T * std::max<int64_t>(ng, 1)), dgig((size_t)A * std::max<int64_t>(ng, 1)),
           scratch(coco_eval_scratch_bytes(ndc, ng, A, M, T));
    CocoEvalArgs a{n_img, n_cat, T, R, A, M, dd.as<double>(), dg.as<double>(), ddo.as<long long>(), dgo.as<long long>(), dco.as<long long>(),
                   dit.as<double>(), drt.as<double>(), dar.as<double>(), dmd.as<int>(), nd, ng, ndc, dprec.as<double>(), drec.as<double>(),
                   dsc.as<double>(), ddtm.as<double>(), dgtm.as<double>(), ddig.as<unsigned char>(), dgig.as<unsigned char>()};
    launch_coco_eval(a, scratch.p, st);
    FFP_HIP(hipStreamSynchronize(st));
    if (n_pr) {
      FFP_HIP(hipMemcpy(precision, dprec.p, sizeof(double) * n_pr, hipMemcpyDeviceToHost));
      FFP_HIP(hipMemcpy(scores, dsc.p, sizeof(double) * n_pr, hipMemcpyDeviceToHost));
      FFP_HIP(hipMemcpy(recall, drec.p, sizeof(double) * n_rc, hipMemcpyDeviceToHost));
    }
    if (dt_matches && ndc) FFP_HIP(hipMemcpy(dt_matches, ddtm.p, sizeof(double) * (size_t)A * T * ndc, hipMemcpyDeviceToHost));
    if (dt_ignore && ndc) FFP_HIP(hipMemcpy(dt_ignore, ddig.p, (size_t)A * T * ndc, hipMemcpyDeviceToHost));
    if (gt_matches && ng) FFP_HIP(hipMemcpy(gt_matches, dgtm.p, sizeof(double) * (size_t)A * T * ng, hipMemcpyDeviceToHost));
    if (gt_ignore && ng) FFP_HIP(hipMemcpy(gt_ignore, dgig.p, (size_t)A * ng, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

// ---- JPEG at the file boundaries -----------------------------------------------------------------------------
// The file boundaries run beside the detector and the enhancer, whose persistent workgroups hold every CU for the length of a layer:
// a low-occupancy chain of small kernels (the JPEG codec) on an ordinary stream gets a turn only at kernel boundaries and stretches to
// tens of milliseconds. Its streams therefore have the highest priority the device offers.
static hipStream_t io_stream() {
  int least = 0, greatest = 0;
  FFP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
  return st;
}

int ffp_jpeg_encode_dev(int device, const uint8_t* d_img, int h, int w, int64_t row_stride, int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(out_size, FFP_ERR_ARG, "jpeg_encode: out_size is null");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "jpeg_encode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  hipStream_t st;
  st = io_stream();
  long long n = 0;
  try {
    n = jpeg_encode_device(d_img, h, w, row_stride, bgr, quality, out, cap, st);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  *out_size = n < 0 ? -n : n;
  FFP_CHECK(n >= 0, FFP_ERR_ARG, "jpeg_encode: output buffer too small (%lld bytes needed)", -n);
  FFP_API_END
}

int ffp_jpeg_encode_batch_dev(int device, const uint8_t* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                              int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && out_offsets && (n == 0 || (d_base && offsets && hs && ws)), FFP_ERR_ARG, "jpeg_encode_batch: bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "jpeg_encode_batch: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  std::vector<JpegSrc> src((size_t)n);
  for (int i = 0; i < n; ++i) src[i] = JpegSrc{d_base + offsets[i], hs[i], ws[i], strides ? strides[i] : (long long)ws[i] * 3};
  std::vector<std::vector<unsigned char>> files;
  hipStream_t st;
  st = io_stream();
  try {
    jpeg_encode_batch_device(src.data(), n, bgr, quality, files, st);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  int64_t pos = 0;
  for (int i = 0; i < n; ++i) { out_offsets[i] = pos; pos += (int64_t)files[i].size(); }
  out_offsets[n] = pos;
  FFP_CHECK(out && cap >= pos, FFP_ERR_ARG, "jpeg_encode_batch: output buffer too small (%lld bytes needed)", (long long)pos);
  for (int i = 0; i < n; ++i) std::memcpy(out + out_offsets[i], files[i].data(), files[i].size());
  FFP_API_END
}

int ffp_jpeg_encode(int device, const uint8_t* img, int h, int w, int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(img && h > 0 && w > 0 && out_size, FFP_ERR_ARG, "jpeg_encode: bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "jpeg_encode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  DevBuf d((size_t)h * w * 3);
  FFP_HIP(hipMemcpy(d.p, img, (size_t)h * w * 3, hipMemcpyHostToDevice));
  hipStream_t st;
  st = io_stream();
  long long n = 0;
  try {
    n = jpeg_encode_device(d.as<unsigned char>(), h, w, (long long)w * 3, bgr, quality, out, cap, st);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  *out_size = n < 0 ? -n : n;
  FFP_CHECK(n >= 0, FFP_ERR_ARG, "jpeg_encode: output buffer too small (%lld bytes needed)", -n);
  FFP_API_END
}

int ffp_jpeg_info(const uint8_t* data, int64_t n, int32_t* out_h, int32_t* out_w, int32_t* out_ncomp) {
  FFP_API_BEGIN
  FFP_CHECK(data && out_h && out_w, FFP_ERR_ARG, "jpeg_info: null argument");
  JpegScan s;
  jpeg_entropy_decode(data, n, s, true);
  *out_h = s.h; *out_w = s.w;
  if (out_ncomp) *out_ncomp = s.ncomp;
  FFP_API_END
}

int ffp_jpeg_decode_dev(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* d_out, int64_t row_stride, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && d_out, FFP_ERR_ARG, "jpeg_decode: null argument");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "jpeg_decode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  hipStream_t st;
  st = io_stream();
  try {
    jpeg_decode_to_device(data, n, d_out, row_stride, cap, bgr, st, nullptr, nullptr);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

int ffp_jpeg_decode(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* out, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && out, FFP_ERR_ARG, "jpeg_decode: null argument");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "jpeg_decode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  JpegScan s;
  jpeg_entropy_decode(data, n, s, true);
  const size_t bytes = (size_t)s.h * s.w * 3;
  FFP_CHECK(cap >= (int64_t)bytes, FFP_ERR_ARG, "jpeg_decode: output buffer too small for %dx%d", s.w, s.h);
  DevBuf d(bytes);
  hipStream_t st;
  st = io_stream();
  try {
    jpeg_decode_to_device(data, n, d.as<unsigned char>(), 0, (long long)bytes, bgr, st, nullptr, nullptr);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_HIP(hipMemcpy(out, d.p, bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_jpeg_decode_stats(int64_t* device_decodes, int64_t* host_fallbacks, int64_t* extra_sync_rounds) {
  FFP_API_BEGIN
  long long a = 0, b = 0, c = 0;
  jpeg_huff_stats(&a, &b, &c);
  if (device_decodes) *device_decodes = a;
  if (host_fallbacks) *host_fallbacks = b;
  if (extra_sync_rounds) *extra_sync_rounds = c;
  FFP_API_END
}

// ---- PNG at the file boundaries (png.hip) -----------------------------------------------------------------------------------------
int64_t ffp_png_bound(int h, int w, int channels, int bit_depth) {
  try {
    return png_bound(h, w, channels, bit_depth);
  } catch (const ffp::Error& e) {
    ffp::set_last_error(e.what());
    return -1;
  }
}

int ffp_png_segment_bytes(void) { return kPngSegmentBytes; }

// the three entries below: device chosen, arguments checked, one launch sequence on an I/O stream; out_offsets is filled before the
// capacity is judged
static void png_encode_any(int device, const void* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides, int channels,
                           int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_CHECK(n >= 0 && out_offsets && (n == 0 || (d_base && offsets && hs && ws)), FFP_ERR_ARG, "png_encode: bad arguments");
  FFP_CHECK((channels == 1 || channels == 3 || channels == 4) && (bit_depth == 8 || bit_depth == 16), FFP_ERR_ARG,
            "png_encode: %d channels of %d bits (gray, RGB or RGBA at depth 8 or 16 are written)", channels, bit_depth);
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "png_encode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  std::vector<PngSrc> src((size_t)n);
  for (int i = 0; i < n; ++i)
    src[i] = PngSrc{(const unsigned char*)d_base + offsets[i], hs[i], ws[i], strides ? strides[i] : (long long)ws[i] * channels * (bit_depth / 8)};
  std::vector<long long> off((size_t)n + 1, 0);
  hipStream_t st;
  st = io_stream();
  long long total = 0;
  try {
    total = png_encode_batch_device(src.data(), n, channels, bit_depth, bgr, level, off.data(), out, cap, st);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  for (int i = 0; i <= n; ++i) out_offsets[i] = off[i];
  FFP_CHECK(out && cap >= total, FFP_ERR_ARG, "png_encode: output buffer too small (%lld bytes needed)", total);
}

int ffp_png_encode_batch_dev(int device, const void* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                             int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_API_BEGIN
  png_encode_any(device, d_base, n, offsets, hs, ws, strides, channels, bit_depth, bgr, level, out, cap, out_offsets);
  FFP_API_END
}

int ffp_png_encode_dev(int device, const void* d_img, int h, int w, int channels, int bit_depth, int64_t row_stride, int bgr, int level, uint8_t* out, int64_t cap,
                       int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(out_size, FFP_ERR_ARG, "png_encode: out_size is null");
  const int64_t zero = 0;
  const int32_t hh = h, ww = w;
  int64_t oo[2] = {0, 0};
  try {
    png_encode_any(device, d_img, 1, &zero, &hh, &ww, &row_stride, channels, bit_depth, bgr, level, out, cap, oo);
  } catch (...) {
    *out_size = oo[1];
    throw;
  }
  *out_size = oo[1];
  FFP_API_END
}

int ffp_png_encode(int device, const void* img, int h, int w, int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(img && h > 0 && w > 0 && out_size, FFP_ERR_ARG, "png_encode: bad arguments");
  FFP_CHECK((channels == 1 || channels == 3 || channels == 4) && (bit_depth == 8 || bit_depth == 16), FFP_ERR_ARG,
            "png_encode: %d channels of %d bits (gray, RGB or RGBA at depth 8 or 16 are written)", channels, bit_depth);
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "png_encode: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  const int64_t row = (int64_t)w * channels * (bit_depth / 8), zero = 0;
  DevBuf d((size_t)h * (size_t)row);
  FFP_HIP(hipMemcpy(d.p, img, (size_t)h * (size_t)row, hipMemcpyHostToDevice));
  const int32_t hh = h, ww = w;
  int64_t oo[2] = {0, 0};
  try {
    png_encode_any(device, d.p, 1, &zero, &hh, &ww, &row, channels, bit_depth, bgr, level, out, cap, oo);
  } catch (...) {
    *out_size = oo[1];
    throw;
  }
  *out_size = oo[1];
  FFP_API_END
}

static int g_op_conv_shape = SHAPE_AUTO;
int ffp_op_conv2d_shape(int force_shape) {
  FFP_API_BEGIN
  FFP_CHECK(force_shape == SHAPE_AUTO || conv_shape_info(force_shape), FFP_ERR_ARG, "conv2d_shape: %d is not a shape number", force_shape);
  g_op_conv_shape = force_shape;
  FFP_API_END
}

int ffp_op_conv2d_shape_name(int shape, char* out, int cap) {
  FFP_API_BEGIN
  const ConvShapeInfo* s = conv_shape_info(shape);
  FFP_CHECK(s && out && cap > 0, FFP_ERR_ARG, "conv2d_shape_name: %d is not a shape number, or no output buffer", shape);
  std::snprintf(out, cap, "%s %s", s->family_name, s->suffix);
  FFP_API_END
}

static thread_local std::string tl_op_conv_variant;      // conv_variant of the op this thread's last ffp_op_conv2d / ffp_op_conv1x1_up2 launched; empty: none was
int ffp_op_conv2d_last_variant(char* out, int cap) {
  FFP_API_BEGIN
  FFP_CHECK(out && cap > 0, FFP_ERR_ARG, "conv2d_last_variant: no output buffer");
  std::snprintf(out, cap, "%s", tl_op_conv_variant.c_str());
  FFP_API_END
}

static int g_op_conv_act_post = ACT_NONE;
int ffp_op_conv2d_act_post(int act) {
  FFP_API_BEGIN
  FFP_CHECK(act >= ACT_NONE && act <= ACT_RELU, FFP_ERR_ARG, "conv2d_act_post: activation code %d (0..3)", act);
  g_op_conv_act_post = act;
  FFP_API_END
}

int ffp_op_conv2d(int device, int precision, const float* x, int n, int h, int w, int cin, const float* wt, const float* bias, int cout,
                  int k, int stride, int groups, int act, int up, const float* res, float res_scale, float* y) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0, FFP_ERR_ARG, "conv2d: bad arguments");
  FFP_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2), FFP_ERR_ARG, "conv2d: k in {1,3}, stride in {1,2}");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "conv2d: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  conv_kernels_init();
  tl_op_conv_variant.clear();
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  const bool split = precision == FFP_PREC_F32X3;
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    PackedConv pc;
    pack_conv(pc, "op", wt, bias, cout, cin, k, groups, T, st, split);
    const int hi = up ? h * 2 : h, wi = up ? w * 2 : w;
    const int ho = (hi + 2 * (k / 2) - k) / stride + 1, wo = (wi + 2 * (k / 2) - k) / stride + 1;
    Level lin, lout;
    lin.build(std::vector<int>(n, h), std::vector<int>(n, w), st);
    lout.build(std::vector<int>(n, ho), std::vector<int>(n, wo), st);
    const int cin_s = pc.depthwise() ? cin : pc.cin;        // stored (padded) input channels
    const size_t npx_in = (size_t)lin.total_px, npx_out = (size_t)lout.total_px;
    auto to_dev = [&](const float* src, size_t px, int c, int c_store) {
      DevBuf b(px * c_store * dsize(T) + 256);
      if (T == F32) {
        std::vector<float> t(px * c_store, 0.f);
        for (size_t p = 0; p < px; ++p) std::memcpy(&t[p * c_store], src + p * c, sizeof(float) * c);
        FFP_HIP(hipMemcpy(b.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
      } else {
        std::vector<_Float16> t(px * c_store, (_Float16)0.f);
        for (size_t p = 0; p < px; ++p) for (int q = 0; q < c; ++q) t[p * c_store + q] = (_Float16)src[p * c + q];
        FFP_HIP(hipMemcpy(b.p, t.data(), t.size() * 2, hipMemcpyHostToDevice));
      }
      return b;
    };
    DevBuf din = to_dev(x, npx_in, cin, cin_s);
    DevBuf dres;
    if (res) dres = to_dev(res, npx_out, cout, cout);
    DevBuf dout(npx_out * cout * dsize(T) + 256);
    TView vin{din.p, T, cin_s, 0, cin_s, &lin}, vout{dout.p, T, cout, 0, cout, &lout}, vres{dres.p, T, cout, 0, cout, &lout};
    DevBuf slots(2 * sizeof(unsigned));                 // max-|value| slots of the input / output buffers (scaled split, see TView::amax)
    {
      float m = 0.f;
      for (size_t i = 0; i < npx_in * (size_t)cin; ++i) m = std::max(m, std::fabs(x[i]));
      unsigned hb[2] = {0u, 0u};
      std::memcpy(&hb[0], &m, 4);
      FFP_HIP(hipMemcpy(slots.p, hb, sizeof(hb), hipMemcpyHostToDevice));
      vin.amax = slots.as<unsigned>(); vout.amax = slots.as<unsigned>() + 1;
    }
    if (pc.depthwise()) {
      FFP_CHECK(k == 3 && stride == 1 && !up, FFP_ERR_ARG, "conv2d: depthwise is 3x3 stride 1");
      FFP_CHECK(g_op_conv_act_post == ACT_NONE, FFP_ERR_ARG, "conv2d: depthwise convs have no post-activation");
      DwConvOp o;
      o.pc = &pc; o.in = vin; o.out = vout; o.out.lvl = &lin; o.act = act;
      if (res) { o.has_res = true; o.res = vres; o.res.lvl = &lin; FFP_CHECK(res_scale == 1.f, FFP_ERR_ARG, "conv2d: depthwise residual has no scale"); }
      launch_dwconv(o, st);
    } else {
      ConvOp o;
      o.pc = &pc; o.in = vin; o.out = vout; o.stride = stride; o.act = act; o.up = up;
      if (res) { o.has_res1 = true; o.res1 = vres; o.s1 = res_scale; }
      o.force_shape = g_op_conv_shape;
      o.act_post = g_op_conv_act_post;
      launch_conv(o, st);
      tl_op_conv_variant = conv_variant(o);
    }
    FFP_HIP(hipStreamSynchronize(st));
    if (T == F32) {
      FFP_HIP(hipMemcpy(y, dout.p, npx_out * cout * 4, hipMemcpyDeviceToHost));
    } else {
      std::vector<_Float16> t(npx_out * cout);
      FFP_HIP(hipMemcpy(t.data(), dout.p, t.size() * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < t.size(); ++i) y[i] = (float)t[i];
    }
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

int ffp_op_conv1x1_up2(int device, int precision, const float* coarse, const float* fine, int n, int h, int w, int c_up, int c_fine,
                       const float* wt, const float* bias, int cout, int act, float* y) {
  FFP_API_BEGIN
  FFP_CHECK(coarse && fine && wt && y && n > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c_up > 0 && c_fine > 0 && cout > 0, FFP_ERR_ARG, "conv1x1_up2: bad arguments");
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "conv1x1_up2: fp32 precisions only");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "conv1x1_up2: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  conv_kernels_init();
  tl_op_conv_variant.clear();
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    const int cin = c_up + c_fine;
    PackedConv pc;
    pack_conv(pc, "op", wt, bias, cout, cin, 1, 1, F32, st, precision == FFP_PREC_F32X3);
    FFP_CHECK(pc.cin == cin, FFP_ERR_ARG, "conv1x1_up2: channel count %d needs padding", cin);
    Level lf, lc;
    lf.build(std::vector<int>(n, h), std::vector<int>(n, w), st);
    lc.build(std::vector<int>(n, h / 2), std::vector<int>(n, w / 2), st);
    const size_t pf = (size_t)lf.total_px, pcs = (size_t)lc.total_px;
    // the concat buffer holds the fine channels at [c_up, cin); its first c_up channels are never written (filled with NaN here:
    // a kernel that read them would show)
    std::vector<float> cat(pf * cin, std::nanf(""));
    for (size_t p = 0; p < pf; ++p) std::memcpy(&cat[p * cin + c_up], fine + p * c_fine, sizeof(float) * c_fine);
    DevBuf dcat(cat.size() * 4 + 256), dco(pcs * c_up * 4 + 256), dout(pf * cout * 4 + 256), slots(3 * sizeof(unsigned));
    FFP_HIP(hipMemcpy(dcat.p, cat.data(), cat.size() * 4, hipMemcpyHostToDevice));
    FFP_HIP(hipMemcpy(dco.p, coarse, pcs * c_up * 4, hipMemcpyHostToDevice));
    float mf = 0.f, mc = 0.f;
    for (size_t i = 0; i < pf * (size_t)c_fine; ++i) mf = std::max(mf, std::fabs(fine[i]));
    for (size_t i = 0; i < pcs * (size_t)c_up; ++i) mc = std::max(mc, std::fabs(coarse[i]));
    unsigned hb[3] = {0u, 0u, 0u};
    std::memcpy(&hb[0], &mf, 4);
    std::memcpy(&hb[1], &mc, 4);
    FFP_HIP(hipMemcpy(slots.p, hb, sizeof(hb), hipMemcpyHostToDevice));
    TView vin{dcat.p, F32, cin, 0, cin, &lf}, vco{dco.p, F32, c_up, 0, c_up, &lc}, vout{dout.p, F32, cout, 0, cout, &lf};
    vin.amax = slots.as<unsigned>(); vco.amax = slots.as<unsigned>() + 1; vout.amax = slots.as<unsigned>() + 2;
    ConvOp o;
    o.pc = &pc; o.in = vin; o.out = vout; o.stride = 1; o.act = act;
    o.has_up2 = true; o.up2 = vco; o.up2_c = c_up; o.up2_map = lf.up2_map(&lc, st);
    o.force_shape = g_op_conv_shape;
    launch_conv(o, st);
    tl_op_conv_variant = conv_variant(o);
    FFP_HIP(hipStreamSynchronize(st));
    FFP_HIP(hipMemcpy(y, dout.p, pf * cout * 4, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

// ---- single-operator entry points of the detector's non-convolution kernels (tests/test_gpu_ops.py) --------------------------------
// Host arrays hold the images of a ragged batch back to back, [sum h*w][cs] fp32 — whole pixel records, so a view may be a channel
// slice of a wider buffer. On the device they sit in the layout of a Level built with `px_align` (padding pixels between images are
// NaN going in and are not copied back); output buffers are in/out: the caller's contents go up first, so bytes outside the written
// slice come back as they went in.
static int g_op_variant[3] = {0, 0, 0};
int ffp_op_variant(int family, int variant) {
  FFP_API_BEGIN
  FFP_CHECK(family >= 0 && family < 3 && variant >= 0 && variant <= 2, FFP_ERR_ARG, "op_variant: family %d / variant %d unknown", family, variant);
  g_op_variant[family] = variant;
  FFP_API_END
}
static int g_op_cls_tower_force = 0;      // ConvOp::dwpw_force of ffp_op_cls_tower's two launches
int ffp_op_cls_tower_variant(int rows, int wg_cap) {
  FFP_API_BEGIN
  FFP_CHECK((rows == 0 || rows == 8 || rows == 16) && wg_cap >= 0 && wg_cap <= 65535, FFP_ERR_ARG, "op_cls_tower_variant: rows %d (0, 8, 16) / workgroup cap %d", rows, wg_cap);
  g_op_cls_tower_force = (rows == 16 ? 1 : rows == 8 ? 2 : 0) | wg_cap << 2;
  FFP_API_END
}

namespace {

struct OpCtx {       // device + a stream of its own for one operator call
  hipStream_t st = nullptr;
  explicit OpCtx(int device, const char* what) {
    int ndev = 0;
    FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "%s: no HIP device %d (no CPU path)", what, device);
    FFP_HIP(hipSetDevice(device));
    FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  ~OpCtx() { if (st) (void)hipStreamDestroy(st); }
  OpCtx(const OpCtx&) = delete;
  OpCtx& operator=(const OpCtx&) = delete;
};

void op_check_batch(const char* what, int n, const int32_t* hs, const int32_t* ws, int px_align) {
  FFP_CHECK(n > 0 && n <= 4096 && hs && ws && px_align >= 1 && px_align <= 4096, FFP_ERR_ARG, "%s: bad batch description", what);
  for (int i = 0; i < n; ++i) FFP_CHECK(hs[i] > 0 && ws[i] > 0 && hs[i] <= 8192 && ws[i] <= 8192, FFP_ERR_ARG, "%s: image %d is %dx%d", what, i, ws[i], hs[i]);
}
void op_check_view(const char* what, int cs, int coff, int C) {
  FFP_CHECK(C > 0 && coff >= 0 && cs > 0 && coff + C <= cs, FFP_ERR_ARG, "%s: channels [%d, %d) do not fit records of %d", what, coff, coff + C, cs);
}
DType op_dtype(const char* what, int precision) {
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F16, FFP_ERR_ARG, "%s: precision must be FFP_PREC_F32 or FFP_PREC_F16", what);
  return precision == FFP_PREC_F16 ? F16 : F32;
}

DevBuf op_upload(const Level& L, DType T, const float* src, int cs) {
  const size_t tot = (size_t)L.total_px * cs;
  DevBuf b(tot * dsize(T) + 256);
  std::vector<float> t(tot, std::nanf(""));
  size_t sp = 0;
  for (int i = 0; i < L.n; ++i) {
    const size_t np = (size_t)L.h[i] * L.w[i];
    std::memcpy(&t[(size_t)L.off[i] * cs], src + sp * cs, np * cs * sizeof(float));
    sp += np;
  }
  if (T == F32) {
    FFP_HIP(hipMemcpy(b.p, t.data(), tot * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<_Float16> h(tot);
    for (size_t i = 0; i < tot; ++i) h[i] = (_Float16)t[i];
    FFP_HIP(hipMemcpy(b.p, h.data(), tot * 2, hipMemcpyHostToDevice));
  }
  return b;
}

void op_download(const Level& L, DType T, const DevBuf& b, int cs, float* dst) {
  const size_t tot = (size_t)L.total_px * cs;
  std::vector<float> t(tot);
  if (T == F32) {
    FFP_HIP(hipMemcpy(t.data(), b.p, tot * 4, hipMemcpyDeviceToHost));
  } else {
    std::vector<_Float16> h(tot);
    FFP_HIP(hipMemcpy(h.data(), b.p, tot * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tot; ++i) t[i] = (float)h[i];
  }
  size_t sp = 0;
  for (int i = 0; i < L.n; ++i) {
    const size_t np = (size_t)L.h[i] * L.w[i];
    std::memcpy(dst + sp * cs, &t[(size_t)L.off[i] * cs], np * cs * sizeof(float));
    sp += np;
  }
}

}  // namespace

int ffp_op_sppf_pool(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, float* y, int y_cs, int y1_coff, int y2_coff, int y3_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "sppf_pool: null argument");
  op_check_batch("sppf_pool", n, hs, ws, px_align);
  op_check_view("sppf_pool input", x_cs, x_coff, c);
  const int yo[3] = {y1_coff, y2_coff, y3_coff};
  for (int i = 0; i < 3; ++i) {
    op_check_view("sppf_pool output", y_cs, yo[i], c);
    for (int j = 0; j < i; ++j) FFP_CHECK(yo[i] >= yo[j] + c || yo[j] >= yo[i] + c, FFP_ERR_ARG, "sppf_pool: output slices %d and %d overlap", j + 1, i + 1);
  }
  const DType T = op_dtype("sppf_pool", precision);
  OpCtx cx(device, "sppf_pool");
  Level L;
  L.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  DevBuf din = op_upload(L, T, x, x_cs), dout = op_upload(L, T, y, y_cs);
  const TView vin{din.p, T, x_cs, x_coff, c, &L};
  const TView v1{dout.p, T, y_cs, y1_coff, c, &L}, v2{dout.p, T, y_cs, y2_coff, c, &L}, v3{dout.p, T, y_cs, y3_coff, c, &L};
  launch_sppf_pool(vin, v1, v2, v3, cx.st, g_op_variant[0]);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(L, T, dout, y_cs, y);
  FFP_API_END
}

int ffp_op_upsample2x(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "upsample2x: null argument");
  op_check_batch("upsample2x", n, hs, ws, px_align);
  op_check_view("upsample2x input", x_cs, x_coff, c);
  op_check_view("upsample2x output", y_cs, y_coff, c);
  const DType T = op_dtype("upsample2x", precision);
  OpCtx cx(device, "upsample2x");
  Level L, L2;
  std::vector<int> h2(n), w2(n);
  for (int i = 0; i < n; ++i) { h2[i] = hs[i] * 2; w2[i] = ws[i] * 2; }
  L.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  L2.build(h2, w2, cx.st, px_align);
  DevBuf din = op_upload(L, T, x, x_cs), dout = op_upload(L2, T, y, y_cs);
  launch_upsample2x(TView{din.p, T, x_cs, x_coff, c, &L}, TView{dout.p, T, y_cs, y_coff, c, &L2}, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(L2, T, dout, y_cs, y);
  FFP_API_END
}

int ffp_op_psa_attention(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int nh, const float* qkv, int q_cs,
                         int q_coff, float* out, int o_cs, int o_coff) {
  FFP_API_BEGIN
  FFP_CHECK(qkv && out && nh > 0 && nh <= 64, FFP_ERR_ARG, "psa_attention: bad arguments");
  op_check_batch("psa_attention", n, hs, ws, px_align);
  constexpr int KD = 32, HD = 64;
  op_check_view("psa_attention qkv", q_cs, q_coff, nh * (2 * KD + HD));
  op_check_view("psa_attention output", o_cs, o_coff, nh * HD);
  const DType T = op_dtype("psa_attention", precision);
  OpCtx cx(device, "psa_attention");
  Level L;
  L.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  DevBuf din = op_upload(L, T, qkv, q_cs), dout = op_upload(L, T, out, o_cs);
  launch_psa_attention(TView{din.p, T, q_cs, q_coff, nh * (2 * KD + HD), &L}, TView{dout.p, T, o_cs, o_coff, nh * HD, &L}, nh, KD, HD, cx.st,
                       g_op_variant[1]);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(L, T, dout, o_cs, out);
  FFP_API_END
}

int ffp_op_dwconv3x3(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, int grp, int grp_stride, int grp_off, const float* wt, const float* bias, int act, const float* res, int r_cs,
                     int r_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && c > 0 && act >= ACT_NONE && act <= ACT_RELU, FFP_ERR_ARG, "dwconv3x3: bad arguments");
  op_check_batch("dwconv3x3", n, hs, ws, px_align);
  FFP_CHECK(x_cs > 0 && x_coff >= 0 && grp >= 0 && grp_stride >= 0 && grp_off >= 0, FFP_ERR_ARG, "dwconv3x3: negative channel addressing");
  if (grp > 0) {      // channel ch is read at x_coff + (ch / grp) * grp_stride + grp_off + ch % grp
    FFP_CHECK(c % grp == 0 && grp_off + grp <= grp_stride, FFP_ERR_ARG, "dwconv3x3: groups of %d at offset %d do not fit records of %d (C = %d)", grp, grp_off, grp_stride, c);
    FFP_CHECK((long long)x_coff + (long long)(c / grp) * grp_stride <= x_cs, FFP_ERR_ARG, "dwconv3x3: %d group records of %d exceed the pixel record of %d", c / grp, grp_stride, x_cs);
  } else {
    FFP_CHECK(grp_stride == 0 && grp_off == 0, FFP_ERR_ARG, "dwconv3x3: grp_stride / grp_off without grp");
    op_check_view("dwconv3x3 input", x_cs, x_coff, c);
  }
  op_check_view("dwconv3x3 output", y_cs, y_coff, c);
  if (res) op_check_view("dwconv3x3 residual", r_cs, r_coff, c);
  const DType T = op_dtype("dwconv3x3", precision);
  OpCtx cx(device, "dwconv3x3");
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, c, c, 3, c, T, cx.st, false);
  Level L;
  L.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  DevBuf din = op_upload(L, T, x, x_cs), dout = op_upload(L, T, y, y_cs), dres;
  if (res) dres = op_upload(L, T, res, r_cs);
  DwConvOp o;
  o.pc = &pc;
  o.in = TView{din.p, T, x_cs, x_coff, c, &L};
  o.out = TView{dout.p, T, y_cs, y_coff, c, &L};
  o.act = act; o.grp = grp; o.grp_stride = grp_stride; o.grp_off = grp_off;
  if (res) { o.has_res = true; o.res = TView{dres.p, T, r_cs, r_coff, c, &L}; }
  o.force = g_op_variant[2];
  launch_dwconv(o, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(L, T, dout, y_cs, y);
  FFP_API_END
}

int ffp_op_cls_tower(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int cin, int nc, const float* x, const float* dw0_w,
                     const float* dw0_b, const float* pw0_w, const float* pw0_b, const float* dw1_w, const float* dw1_b, const float* pw1_w,
                     const float* pw1_b, const float* fin_w, const float* fin_b, float* e1, float* head, int head_cs, int head_coff, int64_t* stray) {
  FFP_API_BEGIN
  FFP_CHECK(x && dw0_w && dw0_b && pw0_w && pw0_b && dw1_w && dw1_b && pw1_w && pw1_b && fin_w && fin_b && head, FFP_ERR_ARG, "cls_tower: null argument");
  op_check_batch("cls_tower", n, hs, ws, px_align);
  FFP_CHECK(px_align % 32 == 0 && cin > 0 && cin % 16 == 0 && cin <= 4096 && nc >= 1 && nc <= 256, FFP_ERR_ARG, "cls_tower: px_align %d must be a multiple of 32, cin %d a multiple of 16, nc %d in [1, 256]", px_align, cin, nc);
  op_check_view("cls_tower head", head_cs, head_coff, nc);
  OpCtx cx(device, "cls_tower");
  conv_kernels_init();
  const int C3 = 128;
  PackedConv dw0, pw0, dw1, pw1, fin;
  pack_conv(dw0, "cv3.0.0", dw0_w, dw0_b, cin, cin, 3, cin, F32, cx.st, false);
  pack_conv(pw0, "cv3.0.1", pw0_w, pw0_b, C3, cin, 1, 1, F32, cx.st, true);
  pack_conv(dw1, "cv3.1.0", dw1_w, dw1_b, C3, C3, 3, C3, F32, cx.st, false);
  pack_conv(pw1, "cv3.1.1", pw1_w, pw1_b, C3, C3, 1, 1, F32, cx.st, true);
  pack_conv(fin, "cv3.2", fin_w, fin_b, nc, C3, 1, 1, F32, cx.st, true);
  DenseF32 dense;
  dense.w.alloc(sizeof(float) * nc * C3);
  dense.b.alloc(sizeof(float) * nc);
  FFP_HIP(hipMemcpy(dense.w.p, fin_w, sizeof(float) * nc * C3, hipMemcpyHostToDevice));
  FFP_HIP(hipMemcpy(dense.b.p, fin_b, sizeof(float) * nc, hipMemcpyHostToDevice));
  Level L;
  L.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  DevBuf dx = op_upload(L, F32, x, cin), dhead = op_upload(L, F32, head, head_cs);
  FFP_HIP(hipMemset(static_cast<char*>(dhead.p) + (size_t)L.total_px * head_cs * 4, 0xFF, 256));      // the slack behind the records: a known pattern too (stray)
  DevBuf de1((size_t)L.total_px * C3 * 4 + 256), de2((size_t)L.total_px * C3 * 4 + 256);
  FFP_HIP(hipMemset(de1.p, 0xFF, de1.n));      // NaN: padding pixels are never written
  FFP_HIP(hipMemset(de2.p, 0xFF, de2.n));
  // a max-|value| slot per (tensor, image): x's from the data, the others raised by their producers
  std::vector<unsigned> slots(3 * (size_t)n, 0u);
  {
    size_t sp = 0;
    for (int i = 0; i < n; ++i) {
      const size_t np = (size_t)hs[i] * ws[i] * cin;
      float m = 0.f;
      for (size_t k = 0; k < np; ++k) m = std::max(m, std::fabs(x[sp + k]));
      std::memcpy(&slots[i], &m, 4);
      sp += np;
    }
  }
  DevBuf dslots(slots.size() * 4);
  FFP_HIP(hipMemcpy(dslots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
  auto view = [&](void* p, int cs, int coff, int c, int slot) {
    TView v{p, F32, cs, coff, c, &L};
    if (slot >= 0) { v.amax = dslots.as<unsigned>() + (size_t)slot * n; v.amax_n = n; }
    return v;
  };
  const bool fuse_fin = nc <= 4;
  ConvOp t1, t2;
  t1.pc = &pw0; t1.dw = &dw0; t1.dw_act = ACT_SILU; t1.act = ACT_SILU;
  t1.in = view(dx.p, cin, 0, cin, 0); t1.out = view(de1.p, C3, 0, C3, 1);
  t2.pc = &pw1; t2.dw = &dw1; t2.dw_act = ACT_SILU; t2.act = ACT_SILU;
  t2.in = t1.out; t2.out = view(fuse_fin ? nullptr : de2.p, C3, 0, C3, 2);
  const TView logits = view(dhead.p, head_cs, head_coff, nc, -1);
  if (fuse_fin) { t2.fin = &fin; t2.fin_w = &dense; t2.fin_out = logits; }
  t1.dwpw_force = t2.dwpw_force = g_op_cls_tower_force;
  launch_conv(t1, cx.st);
  launch_conv(t2, cx.st);
  if (!fuse_fin) {
    ConvOp t3;
    t3.pc = &fin; t3.in = t2.out; t3.out = logits; t3.act = ACT_NONE;
    launch_conv(t3, cx.st);
  }
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(L, F32, dhead, head_cs, head);
  if (e1) op_download(L, F32, de1, C3, e1);
  if (stray) {
    // pixels that belong to no image (behind each aligned image, and the slack behind the buffer) must still hold what went up: 0xFF bytes in e1 / e2,
    // op_upload's NaN in the head record
    const float nanv = std::nanf("");
    unsigned nan_bits;
    std::memcpy(&nan_bits, &nanv, 4);
    auto changed = [&](const DevBuf& b, int cs, unsigned want, unsigned want_slack) {
      std::vector<unsigned> h(b.n / 4);
      FFP_HIP(hipMemcpy(h.data(), b.p, h.size() * 4, hipMemcpyDeviceToHost));
      int64_t bad = 0;
      for (int i = 0; i < n; ++i) {
        const size_t p0 = (size_t)(L.off[i] + (int64_t)hs[i] * ws[i]) * cs, p1 = (size_t)(i + 1 < n ? L.off[i + 1] : L.total_px) * cs;
        for (size_t k = p0; k < p1; ++k) bad += h[k] != want;
      }
      for (size_t k = (size_t)L.total_px * cs; k < h.size(); ++k) bad += h[k] != want_slack;
      return bad;
    };
    *stray = changed(de1, C3, 0xFFFFFFFFu, 0xFFFFFFFFu) + changed(de2, C3, 0xFFFFFFFFu, 0xFFFFFFFFu);
    // nc > 4: the head record is written by the plain 1x1 conv, and the flat-pixel 1x1 kernels compute padding pixels like any pixel (common.hpp, Level::build)
    if (fuse_fin) *stray += changed(dhead, head_cs, nan_bits, 0xFFFFFFFFu);
  }
  FFP_API_END
}

// A dense conv the way the plans run it (tests/test_gpu_conv_views.py): ragged batch, levels built with `px_align`, every operand a channel slice of a
// wider record, up to two residual terms, one max-|value| slot per buffer or per image, and the gate. hs / ws are the INPUT image sizes; y, res1 and
// res2 hold the output level's images. y is in/out. *stray: what changed where the conv may not write — bytes among the 256 behind y's records, and elements
// of y's padding pixels (a 1x1 conv computes the padding pixels of its own slice like any pixel: those channels are left out of the count, except behind an
// image that is inactive under the final gate).
int ffp_op_conv2d_views(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, const float* x, int x_cs, int x_coff,
                        int cin, const float* wt, const float* bias, int cout, int k, int stride, int act, int act_post, int up, const float* res1,
                        int r1_cs, int r1_coff, float s1, const float* res2, int r2_cs, int r2_coff, float s2, float* y, int y_cs, int y_coff,
                        int per_image_amax, uint32_t* amax_out, const int32_t* gate, const int32_t* gate_prev, int64_t* stray) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && amax_out && cin > 0 && cout > 0, FFP_ERR_ARG, "conv2d_views: null argument or no channels");
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F16 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "conv2d_views: precision %d", precision);
  FFP_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2) && (up == 0 || up == 1) && (per_image_amax == 0 || per_image_amax == 1), FFP_ERR_ARG,
            "conv2d_views: k in {1,3}, stride in {1,2}, up and per_image_amax in {0,1}");
  FFP_CHECK(act >= ACT_NONE && act <= ACT_RELU && act_post >= ACT_NONE && act_post <= ACT_RELU, FFP_ERR_ARG, "conv2d_views: activation codes %d / %d (0..3)", act, act_post);
  FFP_CHECK(!gate_prev || gate, FFP_ERR_ARG, "conv2d_views: gate_prev without gate");
  op_check_batch("conv2d_views", n, hs, ws, px_align);
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  const int epv = 16 / (int)dsize(T);
  const int cin_s = (cin + epv - 1) / epv * epv;       // the packed conv's input channels: padded to 16 bytes (an image-input conv reads 3 of 4)
  op_check_view("conv2d_views input", x_cs, x_coff, cin_s);
  FFP_CHECK(x_cs % epv == 0 && x_coff % epv == 0, FFP_ERR_ARG, "conv2d_views: input view not 16-byte aligned (cs=%d coff=%d)", x_cs, x_coff);
  op_check_view("conv2d_views output", y_cs, y_coff, cout);
  if (res1) op_check_view("conv2d_views res1", r1_cs, r1_coff, cout);
  if (res2) op_check_view("conv2d_views res2", r2_cs, r2_coff, cout);
  std::vector<int> hi(hs, hs + n), wi(ws, ws + n), ho(n), wo(n);
  for (int i = 0; i < n; ++i) {
    const int hv = up ? hi[i] * 2 : hi[i], wv = up ? wi[i] * 2 : wi[i];
    ho[i] = (hv + 2 * (k / 2) - k) / stride + 1;
    wo[i] = (wv + 2 * (k / 2) - k) / stride + 1;
  }
  OpCtx cx(device, "conv2d_views");
  conv_kernels_init();
  tl_op_conv_variant.clear();
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, cout, cin, k, 1, T, cx.st, precision == FFP_PREC_F32X3);
  FFP_CHECK(pc.cin == cin_s, FFP_ERR_STATE, "conv2d_views: packed conv reads %d channels, expected %d", pc.cin, cin_s);
  Level lin, lout;
  lin.build(hi, wi, cx.st, px_align);
  lout.build(ho, wo, cx.st, px_align);
  lout.gate_compact = &launch_gate_compact;
  const size_t esz = dsize(T), ybytes = (size_t)lout.total_px * y_cs * esz;
  DevBuf din = op_upload(lin, T, x, x_cs), dout, dr1, dr2;
  if (res1) dr1 = op_upload(lout, T, res1, r1_cs);
  if (res2) dr2 = op_upload(lout, T, res2, r2_cs);
  // max-|value| slots: [0, ns) the input's — from the data, per image over the view's own channels, NaN (an inactive image on its way up) left out —
  // and [ns, 2 ns) the output's, which start from the caller's bit patterns
  const int ns = per_image_amax ? n : 1;
  std::vector<unsigned> slots(2 * (size_t)ns, 0u);
  {
    size_t sp = 0;
    for (int i = 0; i < n; ++i) {
      const size_t np = (size_t)hi[i] * wi[i];
      float m = 0.f;
      for (size_t p = 0; p < np; ++p)
        for (int c = 0; c < cin; ++c) m = std::max(m, std::fabs(x[(sp + p) * x_cs + x_coff + c]));
      unsigned b;
      std::memcpy(&b, &m, 4);
      slots[per_image_amax ? i : 0] = std::max(slots[per_image_amax ? i : 0], b);
      sp += np;
    }
  }
  DevBuf dslots(slots.size() * 4), dgate;
  auto upload_outputs = [&]() {      // padding pixels go up as NaN (op_upload), the slack behind the records as 0xFF bytes
    dout = op_upload(lout, T, y, y_cs);
    FFP_HIP(hipMemset(static_cast<char*>(dout.p) + ybytes, 0xFF, 256));
    std::copy(amax_out, amax_out + ns, slots.begin() + ns);
    FFP_HIP(hipMemcpy(dslots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
  };
  upload_outputs();
  if (gate) dgate = upload(gate_prev ? gate_prev : gate, (size_t)n);
  auto view = [&](void* p, int cs, int coff, int c, Level* L, int slot) {
    TView v{p, T, cs, coff, c, L};
    if (slot >= 0) { v.amax = dslots.as<unsigned>() + (size_t)slot * ns; v.amax_n = ns; }
    return v;
  };
  ConvOp o;
  o.pc = &pc; o.stride = stride; o.act = act; o.act_post = act_post; o.up = up;
  o.in = view(din.p, x_cs, x_coff, cin_s, &lin, 0);
  auto bind_out = [&]() {      // dout is a new allocation after every upload
    o.out = view(dout.p, y_cs, y_coff, cout, &lout, 1);
  };
  bind_out();
  if (res1) { o.has_res1 = true; o.res1 = view(dr1.p, r1_cs, r1_coff, cout, &lout, -1); o.s1 = s1; }
  if (res2) { o.has_res2 = true; o.res2 = view(dr2.p, r2_cs, r2_coff, cout, &lout, -1); o.s2 = s2; }
  if (gate) o.gate = dgate.as<int>();
  o.force_shape = g_op_conv_shape;
  launch_conv(o, cx.st);
  tl_op_conv_variant = conv_variant(o);
  FFP_HIP(hipStreamSynchronize(cx.st));
  if (gate_prev) {      // what a captured plan does between two runs with different gates: same tables, same launches, the mask rewritten and the gated tables compacted again
    upload_outputs();
    bind_out();
    FFP_HIP(hipMemcpy(dgate.p, gate, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    lout.compact_gated(cx.st);
    launch_conv(o, cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
  }
  // one copy of the whole buffer back: the images' records for the caller, the rest for the stray count
  std::vector<unsigned char> now(ybytes + 256);
  FFP_HIP(hipMemcpy(now.data(), dout.p, now.size(), hipMemcpyDeviceToHost));
  {
    size_t sp = 0;
    for (int i = 0; i < n; ++i) {
      const size_t ne = (size_t)ho[i] * wo[i] * y_cs, e0 = (size_t)lout.off[i] * y_cs;
      if (T == F32) std::memcpy(y + sp, &now[e0 * 4], ne * 4);
      else for (size_t e = 0; e < ne; ++e) y[sp + e] = (float)reinterpret_cast<const _Float16*>(now.data())[e0 + e];
      sp += ne;
    }
  }
  FFP_HIP(hipMemcpy(slots.data(), dslots.p, slots.size() * 4, hipMemcpyDeviceToHost));
  std::copy(slots.begin() + ns, slots.end(), amax_out);
  if (stray) {
    volatile float nanv = std::nanf("");            // (volatile: the conversion op_upload ran, not a folded constant)
    const float nanf32 = nanv;
    const _Float16 nanf16 = (_Float16)nanf32;      // what op_upload stored in a padding pixel
    const void* want_pad = T == F32 ? static_cast<const void*>(&nanf32) : static_cast<const void*>(&nanf16);
    int64_t bad = 0;
    for (int i = 0; i < n; ++i) {
      const size_t p0 = (size_t)(lout.off[i] + (int64_t)ho[i] * wo[i]), p1 = (size_t)(i + 1 < n ? lout.off[i + 1] : lout.total_px);
      for (size_t p = p0; p < p1; ++p)
        for (int c = 0; c < y_cs; ++c) {
          if (k == 1 && c >= y_coff && c < y_coff + cout && (!gate || gate[i])) continue;      // (behind an inactive image they are nobody's to write)
          bad += std::memcmp(&now[(p * y_cs + c) * esz], want_pad, esz) != 0;
        }
    }
    for (size_t e = ybytes; e < now.size(); ++e) bad += now[e] != 0xFF;
    *stray = bad;
  }
  FFP_API_END
}

int ffp_op_det_post(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int nc, int nkpt, const float* head8, const float* head16,
                    const float* head32, const float* gain_pad, const int32_t* rects, float conf, float iou, int max_det, int round_boxes,
                    int shift, int full_h, int full_w, float* out_raw, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(head8 && head16 && head32 && gain_pad && rects && nc >= 1 && nc <= 1024 && nkpt >= 0 && nkpt <= 64, FFP_ERR_ARG, "det_post: bad arguments");
  FFP_CHECK((out_dets != nullptr) == (out_counts != nullptr) && (out_raw || out_dets), FFP_ERR_ARG, "det_post: dets and counts come together, and something must be asked for");
  op_check_batch("det_post", n, hs, ws, px_align);
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(hs[i] % 32 == 0 && ws[i] % 32 == 0, FFP_ERR_ARG, "det_post: net input %dx%d of image %d is not a multiple of 32", ws[i], hs[i], i);
    FFP_CHECK(gain_pad[3 * i] > 0.f && rects[4 * i] > 0 && rects[4 * i + 1] > 0, FFP_ERR_ARG, "det_post: image %d has no gain or no size", i);
  }
  if (out_dets) FFP_CHECK(max_det >= 1 && max_det <= 1024 && conf >= 0.f, FFP_ERR_ARG, "det_post: max_det %d outside [1,1024] or negative conf", max_det);
  OpCtx cx(device, "det_post");
  const int cs = 64 + nc + 3 * nkpt, no = 4 + nc + 3 * nkpt, stride = 6 + 3 * nkpt;
  Level L[3];
  DevBuf dh[3];
  const float* heads[3] = {head8, head16, head32};
  for (int l = 0; l < 3; ++l) {
    std::vector<int> h(n), w(n);
    for (int i = 0; i < n; ++i) { h[i] = hs[i] / (8 << l); w[i] = ws[i] / (8 << l); }
    L[l].build(h, w, cx.st, px_align);
    dh[l] = op_upload(L[l], F32, heads[l], cs);
  }
  std::vector<int> aoff(n + 1, 0);
  std::vector<long long> roff(n);
  long long rtot = 0;
  for (int i = 0; i < n; ++i) {
    int a = 0;
    for (int l = 0; l < 3; ++l) a += L[l].h[i] * L[l].w[i];
    aoff[i + 1] = aoff[i] + a;
    roff[i] = rtot;
    rtot += (long long)no * a;
  }
  const int total = aoff[n];
  std::vector<DetImg> di(n);
  for (int i = 0; i < n; ++i) {
    di[i].gain = gain_pad[3 * i]; di[i].pad_x = gain_pad[3 * i + 1]; di[i].pad_y = gain_pad[3 * i + 2];
    di[i].sw = rects[4 * i]; di[i].sh = rects[4 * i + 1]; di[i].x0 = rects[4 * i + 2]; di[i].y0 = rects[4 * i + 3];
  }
  DevBuf d_aoff = upload(aoff.data(), aoff.size()), d_roff = upload(roff.data(), roff.size()), d_imgs = upload(di.data(), di.size());
  DecodeArgs a{};
  for (int l = 0; l < 3; ++l) { a.head[l] = dh[l].as<float>(); a.tab[l] = L[l].d_tab.as<int4>(); }
  a.head_cs = cs; a.nc = nc; a.nkpt = nkpt; a.n_img = n; a.anchor_off = d_aoff.as<int>(); a.total_anchors = total;
  if (out_raw) {
    DevBuf d_raw(sizeof(float) * (size_t)rtot);
    launch_decode_raw(a, d_raw.as<float>(), d_roff.as<long long>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    FFP_HIP(hipMemcpy(out_raw, d_raw.p, sizeof(float) * (size_t)rtot, hipMemcpyDeviceToHost));
  }
  if (out_dets) {
    DevBuf d_boxes(sizeof(float4) * (size_t)total), d_scores(sizeof(float) * (size_t)total), d_classes(sizeof(int) * (size_t)total),
        d_cand(sizeof(int) * (size_t)total), d_cscore(sizeof(float) * (size_t)total);
    const size_t nd = (size_t)n * max_det * stride;
    DevBuf d_dets(sizeof(float) * nd), d_counts(sizeof(int) * (size_t)n);
    FFP_HIP(hipMemsetAsync(d_dets.p, 0, sizeof(float) * nd, cx.st));
    launch_decode(a, conf, d_boxes.as<float4>(), d_scores.as<float>(), d_classes.as<int>(), cx.st);
    launch_nms(a, d_boxes.as<float4>(), d_scores.as<float>(), d_classes.as<int>(), d_cand.as<int>(), d_cscore.as<float>(), d_imgs.as<DetImg>(), iou,
               max_det, round_boxes, stride, d_dets.as<float>(), d_counts.as<int>(), cx.st);
    if (shift) launch_truncate_shift(d_dets.as<float>(), d_counts.as<int>(), d_imgs.as<DetImg>(), n, max_det, stride, nkpt, full_h, full_w, cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    FFP_HIP(hipMemcpy(out_dets, d_dets.p, sizeof(float) * nd, hipMemcpyDeviceToHost));
    FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

int ffp_op_rt_topk(int device, int n, int nt, int nc, const float* scores, int s_cs, int s_coff, int32_t* out_idx) {
  FFP_API_BEGIN
  FFP_CHECK(scores && out_idx && n > 0 && n <= 4096 && nt >= RT_NQ && nt <= (1 << 22), FFP_ERR_ARG, "rt_topk: needs n in [1,4096] images of [%d, 2^22] tokens", RT_NQ);
  op_check_view("rt_topk scores", s_cs, s_coff, nc);
  OpCtx cx(device, "rt_topk");
  const size_t tok = (size_t)n * nt;
  DevBuf ds = upload(scores, tok * s_cs), keys(sizeof(unsigned) * tok), idx(sizeof(int) * (size_t)n * RT_NQ);
  Level L;
  L.build(std::vector<int>(n, 1), std::vector<int>(n, nt), cx.st);
  launch_rt_topk(TView{ds.p, F32, s_cs, s_coff, nc, &L}, nc, nt, n, keys.as<unsigned>(), idx.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(out_idx, idx.p, sizeof(int) * (size_t)n * RT_NQ, hipMemcpyDeviceToHost));
  FFP_API_END
}

// ---- single-operator entry points of the RT-DETR and SCRFD kernels (tests/test_gpu_rtdetr_ops.py, tests/test_gpu_scrfd_ops.py) -------
// The rt_* kernels address image i at i * h * w without padding, so host arrays go up as they are; the launches are the plans' own.
namespace {

struct OpSlot {       // a max-|value| slot: the caller's bit pattern goes up, the final one comes back
  DevBuf d;
  uint32_t* host;
  explicit OpSlot(uint32_t* h) : host(h) { if (h) d = upload(h, 1); }
  unsigned* ptr() const { return host ? d.as<unsigned>() : nullptr; }
  void fetch() { if (host) FFP_HIP(hipMemcpy(host, d.p, sizeof(uint32_t), hipMemcpyDeviceToHost)); }
};

void op_check_view4(const char* what, int cs, int coff, int C) {
  op_check_view(what, cs, coff, C);
  FFP_CHECK(C % 4 == 0 && cs % 4 == 0 && coff % 4 == 0, FFP_ERR_ARG, "%s: channels, offset and record size must be multiples of 4 (%d at %d of %d)", what, C, coff, cs);
}

void op_flat_level(Level& L, int n, long long per_image, hipStream_t st) {      // n images of per_image records each
  FFP_CHECK(per_image >= 1 && per_image <= INT_MAX && n >= 1 && n <= 4096 && (long long)n * per_image <= (1ll << 28), FFP_ERR_ARG,
            "op: %d images of %lld records", n, per_image);
  L.build(std::vector<int>(n, 1), std::vector<int>(n, (int)per_image), st);
}

struct OpView : TView {      // fp32 channels [coff, coff + C) of a buffer of cs-wide records
  OpView(const DevBuf& b, int cs_, int coff_, int C_, Level* L, unsigned* slot = nullptr) : TView{b.p, F32, cs_, coff_, C_, L} { amax = slot; }
};

void op_fetch(const DevBuf& b, float* dst, size_t n) { FFP_HIP(hipMemcpy(dst, b.p, n * sizeof(float), hipMemcpyDeviceToHost)); }

void op_rt_levels(const char* what, const int32_t* hs, const int32_t* ws, RtLevels& lv) {
  FFP_CHECK(hs && ws, FFP_ERR_ARG, "%s: null level sizes", what);
  lv.start[0] = 0;
  for (int l = 0; l < 3; ++l) {
    FFP_CHECK(hs[l] >= 1 && ws[l] >= 1 && hs[l] <= 4096 && ws[l] <= 4096, FFP_ERR_ARG, "%s: level %d is %dx%d", what, l, ws[l], hs[l]);
    lv.h[l] = hs[l]; lv.w[l] = ws[l];
    lv.start[l + 1] = lv.start[l] + hs[l] * ws[l];
  }
}

}  // namespace

int ffp_op_rt_dwconv(int device, int n, int h, int w, int c, int k, int s, int act, const float* x, int x_cs, int x_coff, const float* wt,
                     const float* bias, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && bias && y, FFP_ERR_ARG, "rt_dwconv: null argument");
  FFP_CHECK((k == 5 && s == 1) || (k == 3 && s == 2), FFP_ERR_ARG, "rt_dwconv: k%d s%d (k5 s1 or k3 s2)", k, s);
  FFP_CHECK(act == ACT_NONE || act == ACT_RELU, FFP_ERR_ARG, "rt_dwconv: act %d (0 none, 3 ReLU)", act);
  FFP_CHECK(n >= 1 && n <= 4096 && h >= 1 && w >= 1 && h <= 8192 && w <= 8192, FFP_ERR_ARG, "rt_dwconv: %d images of %dx%d", n, w, h);
  op_check_view4("rt_dwconv input", x_cs, x_coff, c);
  op_check_view4("rt_dwconv output", y_cs, y_coff, c);
  const int ho = (h - 1) / s + 1, wo = (w - 1) / s + 1;
  OpCtx cx(device, "rt_dwconv");
  Level Li, Lo;
  Li.build(std::vector<int>(n, h), std::vector<int>(n, w), cx.st);
  Lo.build(std::vector<int>(n, ho), std::vector<int>(n, wo), cx.st);
  const std::vector<float> wp = rtdetr_pack_depthwise(wt, c, k * k);
  DevBuf dx = upload(x, (size_t)n * h * w * x_cs), dy = upload(y, (size_t)n * ho * wo * y_cs), dw = upload(wp.data(), wp.size()), db = upload(bias, (size_t)c);
  OpSlot slot(amax);
  launch_rt_dwconv(OpView(dx, x_cs, x_coff, c, &Li), OpView(dy, y_cs, y_coff, c, &Lo, slot.ptr()), dw.as<float>(), db.as<float>(), k, s, act, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, (size_t)n * ho * wo * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_maxpool2(int device, int n, int h, int w, int c, const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "rt_maxpool2: null argument");
  FFP_CHECK(n >= 1 && n <= 4096 && h >= 1 && w >= 1 && h <= 8192 && w <= 8192, FFP_ERR_ARG, "rt_maxpool2: %d images of %dx%d", n, w, h);
  op_check_view4("rt_maxpool2 input", x_cs, x_coff, c);
  op_check_view4("rt_maxpool2 output", y_cs, y_coff, c);
  OpCtx cx(device, "rt_maxpool2");
  Level L;
  L.build(std::vector<int>(n, h), std::vector<int>(n, w), cx.st);
  const size_t px = (size_t)n * h * w;
  DevBuf dx = upload(x, px * x_cs), dy = upload(y, px * y_cs);
  OpSlot slot(amax);
  launch_rt_maxpool2(OpView(dx, x_cs, x_coff, c, &L), OpView(dy, y_cs, y_coff, c, &L, slot.ptr()), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, px * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_add(int device, long long npx, int c, const float* a, int a_cs, int a_coff, const float* b, int b_cs, int b_coff, long long period,
                  float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(a && b && y, FFP_ERR_ARG, "rt_add: null argument");
  FFP_CHECK(period >= 0 && period <= npx, FFP_ERR_ARG, "rt_add: period %lld of %lld records", period, npx);
  op_check_view4("rt_add a", a_cs, a_coff, c);
  op_check_view4("rt_add b", b_cs, b_coff, c);
  op_check_view4("rt_add output", y_cs, y_coff, c);
  OpCtx cx(device, "rt_add");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  DevBuf da = upload(a, (size_t)npx * a_cs), db = upload(b, (size_t)(period ? period : npx) * b_cs), dy = upload(y, (size_t)npx * y_cs);
  OpSlot slot(amax);
  launch_rt_add(OpView(da, a_cs, a_coff, c, &L), db.as<float>() + b_coff, b_cs, period, OpView(dy, y_cs, y_coff, c, &L, slot.ptr()), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, (size_t)npx * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_layernorm(int device, long long npx, const float* x, int x_cs, int x_coff, const float* gamma, const float* beta, float* y, int y_cs,
                        int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(gamma && beta && y, FFP_ERR_ARG, "rt_layernorm: null argument");
  if (x) op_check_view4("rt_layernorm input", x_cs, x_coff, 256);
  op_check_view4("rt_layernorm output", y_cs, y_coff, 256);
  OpCtx cx(device, "rt_layernorm");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  DevBuf dy = upload(y, (size_t)npx * y_cs), dx, dg = upload(gamma, (size_t)256), db = upload(beta, (size_t)256);
  if (x) dx = upload(x, (size_t)npx * x_cs);
  OpSlot slot(amax);
  const TView out = OpView(dy, y_cs, y_coff, 256, &L, slot.ptr());
  launch_rt_layernorm(x ? OpView(dx, x_cs, x_coff, 256, &L) : out, dg.as<float>(), db.as<float>(), out, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, (size_t)npx * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_gelu(int device, long long npx, int c, float* x, int cs, int coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x, FFP_ERR_ARG, "rt_gelu: null argument");
  op_check_view4("rt_gelu", cs, coff, c);
  OpCtx cx(device, "rt_gelu");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  DevBuf dx = upload(x, (size_t)npx * cs);
  OpSlot slot(amax);
  launch_rt_gelu(OpView(dx, cs, coff, c, &L, slot.ptr()), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dx, x, (size_t)npx * cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_attention(int device, int n, int L, const float* qk, int qk_cs, int qk_coff, const float* v, int v_cs, int v_coff, float* y, int y_cs,
                        int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(qk && v && y, FFP_ERR_ARG, "rt_attention: null argument");
  op_check_view("rt_attention qk", qk_cs, qk_coff, 512);
  op_check_view("rt_attention v", v_cs, v_coff, 256);
  op_check_view("rt_attention output", y_cs, y_coff, 256);
  OpCtx cx(device, "rt_attention");
  Level Lv;
  op_flat_level(Lv, n, L, cx.st);
  const size_t tok = (size_t)n * L;
  DevBuf dq = upload(qk, tok * qk_cs), dv = upload(v, tok * v_cs), dy = upload(y, tok * y_cs);
  OpSlot slot(amax);
  launch_rt_attention(OpView(dq, qk_cs, qk_coff, 512, &Lv), OpView(dv, v_cs, v_coff, 256, &Lv), OpView(dy, y_cs, y_coff, 256, &Lv, slot.ptr()), L, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, tok * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_enc_prep(int device, int n, const int32_t* hs, const int32_t* ws, const float* src0, const float* src1, const float* src2,
                       const int32_t* src_cs, const int32_t* src_coff, const float* valid, long long rows, float* t, float* tm, uint32_t* amax_t,
                       uint32_t* amax_tm) {
  FFP_API_BEGIN
  FFP_CHECK(src0 && src1 && src2 && src_cs && src_coff && valid && t && tm, FFP_ERR_ARG, "rt_enc_prep: null argument");
  RtLevels lv{};
  op_rt_levels("rt_enc_prep", hs, ws, lv);
  const int NT = lv.start[3];
  FFP_CHECK(n >= 1 && n <= 4096 && NT >= 1 && rows >= (long long)n * NT && rows <= (1ll << 24), FFP_ERR_ARG, "rt_enc_prep: %d images of %d tokens in %lld records", n, NT, rows);
  for (int l = 0; l < 3; ++l) op_check_view4("rt_enc_prep level", src_cs[l], src_coff[l], 256);
  OpCtx cx(device, "rt_enc_prep");
  const float* src[3] = {src0, src1, src2};
  DevBuf ds[3];
  for (int l = 0; l < 3; ++l) {
    ds[l] = upload(src[l], (size_t)n * lv.h[l] * lv.w[l] * src_cs[l]);
    lv.src[l] = ds[l].as<float>() + src_coff[l];
    lv.src_cs[l] = src_cs[l];
  }
  Level LT;
  op_flat_level(LT, n, NT, cx.st);
  DevBuf dv = upload(valid, (size_t)NT), dt = upload(t, (size_t)rows * 256), dtm = upload(tm, (size_t)rows * 256);
  OpSlot st(amax_t), stm(amax_tm);
  launch_rt_enc_prep(lv, dv.as<float>(), OpView(dt, 256, 0, 256, &LT, st.ptr()), OpView(dtm, 256, 0, 256, &LT, stm.ptr()), n, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dt, t, (size_t)rows * 256);
  op_fetch(dtm, tm, (size_t)rows * 256);
  st.fetch();
  stm.fetch();
  FFP_API_END
}

int ffp_op_rt_gather(int device, int n, int nt, const float* e, int e_cs, int e_coff, const int32_t* idx, const float* anchors, float* q, int q_cs,
                     int q_coff, float* anc_out, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(e && idx && anchors && q && anc_out, FFP_ERR_ARG, "rt_gather: null argument");
  FFP_CHECK(nt >= 1 && nt <= (1 << 22), FFP_ERR_ARG, "rt_gather: %d tokens", nt);
  op_check_view4("rt_gather tokens", e_cs, e_coff, 256);
  op_check_view4("rt_gather queries", q_cs, q_coff, 256);
  OpCtx cx(device, "rt_gather");
  Level LT, LQ;
  op_flat_level(LT, n, nt, cx.st);
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  DevBuf de = upload(e, (size_t)n * nt * e_cs), di = upload(idx, nq), da = upload(anchors, (size_t)nt * 4), dq = upload(q, nq * q_cs), dan = upload(anc_out, nq * 4);
  OpSlot slot(amax);
  // the kernel takes whole 256-channel records: the slices start at the views' pointers
  TView ve{de.as<float>() + e_coff, F32, e_cs, 0, 256, &LT}, vq{dq.as<float>() + q_coff, F32, q_cs, 0, 256, &LQ};
  vq.amax = slot.ptr();
  launch_rt_gather(ve, di.as<int>(), da.as<float>(), nt, n, vq, dan.as<float>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dq, q, nq * q_cs);
  op_fetch(dan, anc_out, nq * 4);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_ref(int device, long long nq, const float* delta, int d_cs, int d_coff, const float* anc, float* ref, int r_cs, int r_coff,
                  uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(delta && ref, FFP_ERR_ARG, "rt_ref: null argument");
  op_check_view("rt_ref delta", d_cs, d_coff, 4);
  op_check_view("rt_ref boxes", r_cs, r_coff, 4);
  OpCtx cx(device, "rt_ref");
  Level L;
  op_flat_level(L, 1, nq, cx.st);
  DevBuf dd = upload(delta, (size_t)nq * d_cs), dr = upload(ref, (size_t)nq * r_cs), da;
  if (anc) da = upload(anc, (size_t)nq * 4);
  OpSlot slot(amax);
  launch_rt_ref(OpView(dd, d_cs, d_coff, 4, &L), anc ? da.as<float>() : nullptr, OpView(dr, r_cs, r_coff, 4, &L, slot.ptr()), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dr, ref, (size_t)nq * r_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_deform(int device, int n, const int32_t* hs, const int32_t* ws, const float* val, int v_cs, int v_coff, const float* oa, int oa_cs,
                     int oa_coff, const float* ref, int r_cs, int r_coff, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(val && oa && ref && y, FFP_ERR_ARG, "rt_deform: null argument");
  RtLevels lv{};
  op_rt_levels("rt_deform", hs, ws, lv);
  const int NT = lv.start[3];
  op_check_view("rt_deform values", v_cs, v_coff, 256);
  op_check_view("rt_deform offsets and weights", oa_cs, oa_coff, 288);
  op_check_view("rt_deform boxes", r_cs, r_coff, 4);
  op_check_view("rt_deform output", y_cs, y_coff, 256);
  OpCtx cx(device, "rt_deform");
  Level LT, LQ;
  op_flat_level(LT, n, NT, cx.st);
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  DevBuf dv = upload(val, (size_t)n * NT * v_cs), doa = upload(oa, nq * oa_cs), dr = upload(ref, nq * r_cs), dy = upload(y, nq * y_cs);
  OpSlot slot(amax);
  launch_rt_deform(OpView(dv, v_cs, v_coff, 256, &LT), OpView(doa, oa_cs, oa_coff, 288, &LQ), OpView(dr, r_cs, r_coff, 4, &LQ), lv,
                   OpView(dy, y_cs, y_coff, 256, &LQ, slot.ptr()), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dy, y, nq * y_cs);
  slot.fetch();
  FFP_API_END
}

int ffp_op_rt_decode(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                     const float* orig_wh, float* out_raw, float* out_det, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(ref && scores && nc >= 1 && nc <= 4096, FFP_ERR_ARG, "rt_decode: bad arguments");
  FFP_CHECK((out_det != nullptr) == (out_counts != nullptr) && (out_raw || out_det) && (!out_det || orig_wh), FFP_ERR_ARG,
            "rt_decode: det, counts and orig_wh come together, and something must be asked for");
  op_check_view("rt_decode boxes", r_cs, r_coff, 4);
  op_check_view("rt_decode scores", s_cs, s_coff, nc);
  OpCtx cx(device, "rt_decode");
  Level LQ;
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  DevBuf dr = upload(ref, nq * r_cs), ds = upload(scores, nq * s_cs);
  const TView vr = OpView(dr, r_cs, r_coff, 4, &LQ), vs = OpView(ds, s_cs, s_coff, nc, &LQ);
  if (out_raw) {
    DevBuf d_raw = upload(out_raw, nq * (4 + nc));
    launch_rt_raw(vr, vs, nc, d_raw.as<float>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    op_fetch(d_raw, out_raw, nq * (4 + nc));
  }
  if (out_det) {
    DevBuf d_det = upload(out_det, nq * 6), d_wh = upload(orig_wh, (size_t)n * 2), d_counts = upload(out_counts, (size_t)n);
    launch_rt_post(vr, vs, nc, conf, d_wh.as<float2>(), n, d_det.as<float>(), d_counts.as<int>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    op_fetch(d_det, out_det, nq * 6);
    FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

int ffp_op_rt_post_tiles(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                         const int32_t* tiles_xyxy, int full_h, int full_w, int mode, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(ref && scores && tiles_xyxy && out_dets && out_counts && nc >= 1 && nc <= 4096, FFP_ERR_ARG, "rt_post_tiles: bad arguments");
  FFP_CHECK(full_h > 0 && full_w > 0 && (mode == FFP_RT_TILES_LOCAL || mode == FFP_RT_TILES_SAHI), FFP_ERR_ARG,
            "rt_post_tiles: full shape %d x %d, mode %d", full_w, full_h, mode);
  op_check_view("rt_post_tiles boxes", r_cs, r_coff, 4);
  op_check_view("rt_post_tiles scores", s_cs, s_coff, nc);
  OpCtx cx(device, "rt_post_tiles");
  Level LQ;
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  DevBuf dr = upload(ref, nq * r_cs), ds = upload(scores, nq * s_cs), dt = upload(tiles_xyxy, (size_t)n * 4);
  DevBuf d_det = upload(out_dets, nq * 6), d_counts = upload(out_counts, (size_t)n);
  launch_rt_post_tiles(OpView(dr, r_cs, r_coff, 4, &LQ), OpView(ds, s_cs, s_coff, nc, &LQ), nc, conf, dt.as<int4>(), n, full_h, full_w, mode,
                       d_det.as<float>(), d_counts.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(d_det, out_dets, nq * 6);
  FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_op_scrfd_pool(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, int maxpool, int k, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "scrfd_pool: null argument");
  FFP_CHECK(maxpool || (k >= 1 && k <= 8), FFP_ERR_ARG, "scrfd_pool: average window %d outside [1, 8]", k);
  op_check_batch("scrfd_pool", n, hs, ws, px_align);
  op_check_view("scrfd_pool input", x_cs, x_coff, c);
  op_check_view("scrfd_pool output", y_cs, y_coff, c);
  OpCtx cx(device, "scrfd_pool");
  std::vector<int> ho(n), wo(n);
  for (int i = 0; i < n; ++i) {
    ho[i] = maxpool ? (hs[i] - 1) / 2 + 1 : (hs[i] + k - 1) / k;
    wo[i] = maxpool ? (ws[i] - 1) / 2 + 1 : (ws[i] + k - 1) / k;
  }
  Level Li, Lo;
  Li.build(std::vector<int>(hs, hs + n), std::vector<int>(ws, ws + n), cx.st, px_align);
  Lo.build(ho, wo, cx.st, px_align);
  DevBuf dx = op_upload(Li, F32, x, x_cs), dy = op_upload(Lo, F32, y, y_cs);
  launch_scrfd_pool(OpView(dx, x_cs, x_coff, c, &Li), OpView(dy, y_cs, y_coff, c, &Lo), maxpool ? 1 : 0, k, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_download(Lo, F32, dy, y_cs, y);
  FFP_API_END
}

int ffp_op_scrfd_post(int device, int n, int net_h, int net_w, int A, const int32_t* strides, int px_align, const float* const* heads,
                      const int32_t* cs, const int32_t* coff, const float* det_scale, float thresh, float nms_thresh, int cap, float* out,
                      int32_t* out_counts, float* raw_scores) {
  FFP_API_BEGIN
  FFP_CHECK(strides && heads && cs && coff && det_scale && out && out_counts, FFP_ERR_ARG, "scrfd_post: null argument");
  FFP_CHECK(n >= 1 && n <= 4096 && A >= 1 && A <= 16 && cap >= 1 && cap <= (1 << 20) && px_align >= 1 && px_align <= 4096 && net_h >= 1 && net_w >= 1 &&
                net_h <= 8192 && net_w <= 8192, FFP_ERR_ARG, "scrfd_post: bad sizes");
  const bool use_kps = heads[6] != nullptr;
  const int per_px[3] = {A, 4 * A, 10 * A};
  for (int kind = 0; kind < 3; ++kind) {
    for (int l = 0; l < 3; ++l)
      FFP_CHECK((heads[3 * kind + l] != nullptr) == (kind < 2 || use_kps), FFP_ERR_ARG, "scrfd_post: head %d of level %d missing (kps: all three levels or none)", kind, l);
    if (kind < 2 || use_kps) op_check_view("scrfd_post head", cs[kind], coff[kind], per_px[kind]);
  }
  for (int i = 0; i < n; ++i) FFP_CHECK(det_scale[i] > 0.f, FFP_ERR_ARG, "scrfd_post: det_scale of image %d", i);
  OpCtx cx(device, "scrfd_post");
  Level L[3];
  DevBuf dh[3][3];
  ScrfdHeads h{};
  h.A = A;
  h.a_off[0] = 0;
  for (int l = 0; l < 3; ++l) {
    FFP_CHECK(strides[l] >= 1 && net_h % strides[l] == 0 && net_w % strides[l] == 0, FFP_ERR_ARG, "scrfd_post: stride %d does not divide %dx%d", strides[l], net_w, net_h);
    const int lh = net_h / strides[l], lw = net_w / strides[l];
    L[l].build(std::vector<int>(n, lh), std::vector<int>(n, lw), cx.st, px_align);
    for (int kind = 0; kind < 3; ++kind) {
      if (!heads[3 * kind + l]) continue;
      dh[kind][l] = op_upload(L[l], F32, heads[3 * kind + l], cs[kind]);
      h.cs[kind][l] = cs[kind];
      h.coff[kind][l] = coff[kind];
    }
    h.score[l] = dh[0][l].as<float>();
    h.bbox[l] = dh[1][l].as<float>();
    h.kps[l] = use_kps ? dh[2][l].as<float>() : nullptr;
    h.tab[l] = L[l].d_tab.as<int4>();
    h.stride[l] = strides[l];
    h.a_off[l + 1] = h.a_off[l] + lh * lw * A;
  }
  h.per_img = h.a_off[3];
  DevBuf d_scale = upload(det_scale, (size_t)n);
  h.det_scale = d_scale.as<float>();
  const size_t na = (size_t)n * h.per_img, no = (size_t)n * cap * FFP_DET_STRIDE(5);
  DevBuf d_cand(sizeof(ScrfdCand) * na), d_counts(sizeof(int) * (size_t)n), d_order(sizeof(int) * na), d_supp(sizeof(int) * na),
      d_out = upload(out, no), d_out_counts(sizeof(int) * (size_t)n), d_raw;
  if (raw_scores) {
    d_raw.alloc(sizeof(float) * na);
    launch_scrfd_decode(h, n, 0.f, nullptr, nullptr, d_raw.as<float>(), cx.st);
  }
  launch_scrfd_decode(h, n, thresh, d_cand.as<ScrfdCand>(), d_counts.as<int>(), nullptr, cx.st);
  launch_scrfd_nms(d_cand.as<ScrfdCand>(), d_counts.as<int>(), n, h.per_img, d_order.as<int>(), d_supp.as<int>(), nms_thresh, d_out.as<float>(), cap,
                   d_out_counts.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(d_out, out, no);
  FFP_HIP(hipMemcpy(out_counts, d_out_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  if (raw_scores) op_fetch(d_raw, raw_scores, na);
  FFP_API_END
}

int ffp_op_scrfd_sahi_rows(int device, int n_tiles, int cap, const int32_t* tiles_xyxy, int full_h, int full_w, float conf, float* dets,
                           int32_t* counts, int32_t* out_bad) {
  FFP_API_BEGIN
  FFP_CHECK(tiles_xyxy && dets && counts, FFP_ERR_ARG, "scrfd_sahi_rows: null argument");
  FFP_CHECK(n_tiles >= 1 && n_tiles <= 65536 && cap >= 1 && cap <= (1 << 20) && (long long)n_tiles * cap < (1 << 24) && full_h >= 1 && full_w >= 1, FFP_ERR_ARG,
            "scrfd_sahi_rows: bad sizes");
  if (out_bad) *out_bad = -1;
  OpCtx cx(device, "scrfd_sahi_rows");
  const size_t nd = (size_t)n_tiles * cap * FFP_DET_STRIDE(5);
  DevBuf dd = upload(dets, nd), dc = upload(counts, (size_t)n_tiles), dt = upload(tiles_xyxy, (size_t)n_tiles * 4), de(sizeof(unsigned));
  launch_scrfd_sahi_rows(dd.as<float>(), dc.as<int>(), dt.as<int4>(), n_tiles, cap, conf, full_h, full_w, de.as<unsigned>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(dd, dets, nd);
  FFP_HIP(hipMemcpy(counts, dc.p, sizeof(int) * (size_t)n_tiles, hipMemcpyDeviceToHost));
  unsigned bad = SCRFD_NO_BAD_ROW;
  FFP_HIP(hipMemcpy(&bad, de.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (bad != SCRFD_NO_BAD_ROW) {
    if (out_bad) *out_bad = (int32_t)bad;
    FFP_CHECK(false, FFP_ERR_ARG, "scrfd_sahi_rows: tile %d row %d: Box coords [minx, miny, maxx, maxy] cannot be negative", (int)(bad / (unsigned)cap),
              (int)(bad % (unsigned)cap));
  }
  FFP_API_END
}

// tuning hook: average device time (HIP events) of `iters` launches of one dense convolution on synthetic data
int ffp_op_conv2d_time(int device, int precision, int n, int h, int w, int cin, int cout, int k, int stride, int up, int iters,
                       int dbg_mask, int force_shape, float* out_us) {
  FFP_API_BEGIN
  FFP_CHECK(out_us && n > 0 && iters > 0, FFP_ERR_ARG, "bad arguments");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "no HIP device %d", device);
  FFP_HIP(hipSetDevice(device));
  conv_kernels_init();
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    std::vector<float> wt((size_t)cout * cin * k * k), bias(cout, 0.1f);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xFFFF) / 65536.0f - 0.5f; };
    for (auto& v : wt) v = rnd() * 0.1f;
    PackedConv pc;
    pack_conv(pc, "bench", wt.data(), bias.data(), cout, cin, k, 1, T, st, precision == FFP_PREC_F32X3);
    const int hi = up ? h * 2 : h, wi = up ? w * 2 : w;
    const int ho = (hi + 2 * (k / 2) - k) / stride + 1, wo = (wi + 2 * (k / 2) - k) / stride + 1;
    Level lin, lout;
    lin.build(std::vector<int>(n, h), std::vector<int>(n, w), st);
    lout.build(std::vector<int>(n, ho), std::vector<int>(n, wo), st);
    const size_t nin = (size_t)lin.total_px * pc.cin, nout = (size_t)lout.total_px * cout;
    DevBuf din(nin * dsize(T) + 256), dout(nout * dsize(T) + 256);
    {
      std::vector<float> hx(std::min(nin, (size_t)1 << 22));
      for (auto& v : hx) v = rnd();
      if (T == F32) {
        for (size_t o = 0; o < nin; o += hx.size()) FFP_HIP(hipMemcpy((float*)din.p + o, hx.data(), std::min(hx.size(), nin - o) * 4, hipMemcpyHostToDevice));
      } else {
        std::vector<_Float16> hh(hx.size());
        for (size_t i = 0; i < hx.size(); ++i) hh[i] = (_Float16)hx[i];
        for (size_t o = 0; o < nin; o += hh.size()) FFP_HIP(hipMemcpy((_Float16*)din.p + o, hh.data(), std::min(hh.size(), nin - o) * 2, hipMemcpyHostToDevice));
      }
    }
    ConvOp o;
    o.pc = &pc; o.stride = stride; o.act = precision == FFP_PREC_F16 ? ACT_LRELU : ACT_SILU; o.up = up; o.dbg = dbg_mask; o.force_shape = force_shape;   // the activation each precision's network uses
    o.in = TView{din.p, T, pc.cin, 0, pc.cin, &lin};
    o.out = TView{dout.p, T, cout, 0, cout, &lout};
    // SHAPE_TRUNK: the fused-body kernel (conv_trunk.hip) on this ONE layer, its plan built once outside the timed launches
    std::unique_ptr<TrunkPlan> tp;
    if (force_shape == SHAPE_TRUNK) tp.reset(new TrunkPlan(std::vector<ConvOp>{o}));
    auto once = [&]() { if (tp) tp->launch(st, dbg_mask); else launch_conv(o, st); };
    for (int i = 0; i < 3; ++i) once();
    hipEvent_t e0, e1;
    FFP_HIP(hipEventCreate(&e0)); FFP_HIP(hipEventCreate(&e1));
    FFP_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) once();
    FFP_HIP(hipEventRecord(e1, st));
    FFP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    FFP_HIP(hipEventElapsedTime(&ms, e0, e1));
    *out_us = ms * 1e3f / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  (void)hipStreamDestroy(st);
  FFP_API_END
}

int ffp_op_resize_lanczos4(int device, const void* src, int h, int w, int channels, int bits, int out_h, int out_w, void* dst) {
  FFP_API_BEGIN
  FFP_CHECK(src && dst, FFP_ERR_ARG, "resize_lanczos4: null argument");
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, FFP_ERR_ARG, "resize_lanczos4: empty image (%dx%d -> %dx%d)", h, w, out_h, out_w);
  FFP_CHECK(channels == 1 || channels == 3 || channels == 4, FFP_ERR_ARG, "resize_lanczos4: channels %d (1, 3 or 4)", channels);
  FFP_CHECK(bits == 8 || bits == 16, FFP_ERR_ARG, "resize_lanczos4: bits %d (8 or 16)", bits);
  const int wide = bits == 16;
  const size_t in_bytes = ((size_t)h * w * channels) << wide, out_bytes = ((size_t)out_h * out_w * channels) << wide;
  if (out_h == h && out_w == w) {     // cv::resize of the same size is a copy
    std::memcpy(dst, src, out_bytes);
    return FFP_OK;
  }
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "resize_lanczos4: no HIP device %d", device);
  FFP_HIP(hipSetDevice(device));
  hipStream_t st;
  FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  try {
    DevBuf din(in_bytes), dout(out_bytes), tab;
    std::vector<uint8_t> host_tab;
    FFP_HIP(hipMemcpyAsync(din.p, src, in_bytes, hipMemcpyHostToDevice, st));
    resize_lanczos4_dev(din.p, h, w, channels, wide, out_h, out_w, dout.p, tab, host_tab, st);
    FFP_HIP(hipStreamSynchronize(st));
    FFP_HIP(hipMemcpy(dst, dout.p, out_bytes, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    throw;
  }
  FFP_HIP(hipStreamDestroy(st));
  FFP_API_END
}

// ---- SCRFD (InsightFace RetinaFace) --------------------------------------------------------------------------------------------

int ffp_scrfd_create(const void* onnx_bytes, size_t nbytes, int n, int device, int precision, ffp_scrfd** out) {
  FFP_API_BEGIN
  FFP_CHECK(out && onnx_bytes && nbytes > 0, FFP_ERR_ARG, "null argument");
  FFP_CHECK(n >= 1, FFP_ERR_ARG, "batch hint %d", n);
  *out = new ffp_scrfd(onnx_bytes, nbytes, n, device, precision);
  FFP_API_END
}

void ffp_scrfd_destroy(ffp_scrfd* s) { delete s; }

int ffp_scrfd_describe(const void* onnx_bytes, size_t nbytes, int n, int det_w, int det_h, char* out, size_t cap) {
  std::string text;
  int rc = FFP_OK;
  try {
    text = ffp::onnx::lower(ffp::onnx::parse(onnx_bytes, nbytes), n, det_w, det_h).describe();
  } catch (const ffp::Error& e) {
    ffp::set_last_error(e.what());
    text = e.what();
    rc = e.code;
  } catch (const std::bad_alloc&) {
    ffp::set_last_error("host out of memory");
    return FFP_ERR_NOMEM;
  } catch (const std::exception& e) {
    ffp::set_last_error(e.what());
    text = e.what();
    rc = FFP_ERR_STATE;
  }
  if (out && cap > 0) {
    const size_t k = std::min(text.size(), cap - 1);
    std::memcpy(out, text.data(), k);
    out[k] = 0;
  }
  return rc;
}

int ffp_scrfd_infer_tiles(ffp_scrfd* s, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                          float det_thresh, float nms_thresh, float* out_dets, int cap, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.infer_tiles(frame, H, W, chan_order, tiles, n_tiles, det_w, det_h, det_thresh, nms_thresh, out_dets, cap, out_counts);
  FFP_API_END
}

// the batched detector call behind InsightFaceDetectionModel.perform_inference_batch, in bounded chunks, and (FFP_SCRFD_TILES_SAHI) the
// per-face Python behind it: utils/insightface_wrapper.py:83-86, sahi/annotation.py and get_shifted_object_prediction
int ffp_scrfd_infer_tiles_ex(ffp_scrfd* s, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                             float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* out_dets, int cap, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.infer_tiles_ex(frame, H, W, chan_order, tiles, n_tiles, det_w, det_h, det_thresh, nms_thresh, conf, mode, max_batch, out_dets, cap, out_counts);
  FFP_API_END
}

int ffp_scrfd_infer_tiles_dev(ffp_scrfd* s, const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w,
                              int det_h, float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* d_out_dets, int cap,
                              int32_t* d_out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.infer_tiles_dev(d_frame, H, W, chan_order, tiles, n_tiles, det_w, det_h, det_thresh, nms_thresh, conf, mode, max_batch, d_out_dets, cap,
                         d_out_counts);
  FFP_API_END
}

// sahi.predict.get_sliced_prediction over InsightFaceDetectionModel (pipeline_v1_detection_first/app_v1.py's detector stage) in one call
int ffp_scrfd_sliced_predict(ffp_scrfd* s, const uint8_t* frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                             int perform_standard_pred, int det_w, int det_h, float det_thresh, float nms_thresh, float conf, int max_batch,
                             int tile_cap, int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* out, int cap, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(s && frame && out && out_n && cap > 0, FFP_ERR_ARG, "null argument");
  s->eng.sliced_predict(frame, H, W, chan_order, sliced_items(H, W, slice_h, slice_w, oh, ow, perform_standard_pred), det_w, det_h, det_thresh,
                        nms_thresh, conf, max_batch, tile_cap, pp_type, pp_metric, pp_thr, class_agnostic, out, cap, out_n);
  FFP_API_END
}

int ffp_scrfd_sliced_predict_dev(ffp_scrfd* s, const uint8_t* d_frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                                 int perform_standard_pred, int det_w, int det_h, float det_thresh, float nms_thresh, float conf, int max_batch,
                                 int tile_cap, int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* d_out, int cap, int32_t* d_out_n) {
  FFP_API_BEGIN
  FFP_CHECK(s && d_frame && d_out && d_out_n && cap > 0, FFP_ERR_ARG, "null argument");
  s->eng.sliced_predict_dev(d_frame, H, W, chan_order, sliced_items(H, W, slice_h, slice_w, oh, ow, perform_standard_pred), det_w, det_h, det_thresh,
                            nms_thresh, conf, max_batch, tile_cap, pp_type, pp_metric, pp_thr, class_agnostic, d_out, cap, d_out_n);
  FFP_API_END
}

int ffp_scrfd_mem_bytes(ffp_scrfd* s, uint64_t* out_plan_bytes, int32_t* out_plans_resident) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  size_t b = 0;
  int n = 0;
  s->eng.mem_bytes(&b, &n);
  if (out_plan_bytes) *out_plan_bytes = b;
  if (out_plans_resident) *out_plans_resident = n;
  FFP_API_END
}

int ffp_scrfd_drop_plans(ffp_scrfd* s) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  s->eng.drop_plans();
  FFP_API_END
}

int ffp_scrfd_forward_raw(ffp_scrfd* s, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                          float* out, size_t cap, int64_t* out_sizes) {
  FFP_API_BEGIN
  FFP_CHECK(s && out && out_sizes, FFP_ERR_ARG, "null argument");
  s->eng.forward_raw(frame, H, W, chan_order, tiles, n_tiles, det_w, det_h, out, cap, out_sizes);
  FFP_API_END
}

int ffp_scrfd_geometry(int h, int w, int net_w, int net_h, int32_t* out2, float* det_scale) {
  FFP_API_BEGIN
  FFP_CHECK(out2 && det_scale && h > 0 && w > 0 && net_w > 0 && net_h > 0, FFP_ERR_ARG, "scrfd_geometry: sizes must be positive");
  int nw, nh;
  scrfd_geometry(h, w, net_w, net_h, &nw, &nh, det_scale);
  out2[0] = nw;
  out2[1] = nh;
  FFP_API_END
}

int ffp_scrfd_info(ffp_scrfd* s, int32_t* out_n_outputs, double* out_last_conv_flops) {
  FFP_API_BEGIN
  FFP_CHECK(s, FFP_ERR_ARG, "null handle");
  if (out_n_outputs) *out_n_outputs = s->eng.n_outputs();
  if (out_last_conv_flops) *out_last_conv_flops = s->eng.last_conv_flops;
  FFP_API_END
}

// ---- RT-DETR-l (ultralytics.RTDETR, pipeline_v3_RTDETR/inference.py) -----------------------------------------------------------

int ffp_rtdetr_create(const void* weights, size_t nbytes, int device, int precision, ffp_rtdetr** out) {
  FFP_API_BEGIN
  FFP_CHECK(out && weights && nbytes > 0, FFP_ERR_ARG, "null argument");
  *out = new ffp_rtdetr(weights, nbytes, device, precision);
  FFP_API_END
}

void ffp_rtdetr_destroy(ffp_rtdetr* r) { delete r; }

int ffp_rtdetr_predict(ffp_rtdetr* r, const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float conf, float* out_dets,
                       int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(r && frames && hw && out_dets && out_counts, FFP_ERR_ARG, "null argument");
  r->eng.predict(frames, hw, n, imgsz, conf, out_dets, out_counts);
  FFP_API_END
}

int ffp_rtdetr_forward_raw(ffp_rtdetr* r, const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float* out, int32_t* out_topk) {
  FFP_API_BEGIN
  FFP_CHECK(r && frames && hw && out, FFP_ERR_ARG, "null argument");
  r->eng.forward_raw(frames, hw, n, imgsz, out, out_topk);
  FFP_API_END
}

// sahi.predict.get_sliced_prediction over sahi.models.ultralytics (model_type "rtdetr"): the slices of a frame as network batches
int ffp_rtdetr_infer_tiles(ffp_rtdetr* r, const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                           float conf, int mode, int max_batch, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(r && out_dets && out_counts, FFP_ERR_ARG, "null argument");
  r->eng.infer_tiles(frame, H, W, chan_order, tiles, n_tiles, imgsz, conf, mode, max_batch, out_dets, out_counts);
  FFP_API_END
}

int ffp_rtdetr_infer_tiles_dev(ffp_rtdetr* r, const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                               float conf, int mode, int max_batch, float* d_out_dets, int32_t* d_out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(r && d_frame && d_out_dets && d_out_counts, FFP_ERR_ARG, "null argument");
  r->eng.infer_tiles_dev(d_frame, H, W, chan_order, tiles, n_tiles, imgsz, conf, mode, max_batch, d_out_dets, d_out_counts);
  FFP_API_END
}

int ffp_rtdetr_sliced_predict(ffp_rtdetr* r, const uint8_t* frame, int H, int W, int chan_order, int slice_h, int slice_w, float oh, float ow,
                              int perform_standard_pred, int imgsz, float conf, int max_batch, int pp_type, int pp_metric, double pp_thr,
                              int class_agnostic, float* out, int cap, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(r && frame && out && out_n && cap > 0, FFP_ERR_ARG, "null argument");
  r->eng.sliced_predict(frame, H, W, chan_order, sliced_items(H, W, slice_h, slice_w, oh, ow, perform_standard_pred), imgsz, conf, max_batch, pp_type,
                        pp_metric, pp_thr, class_agnostic, out, cap, out_n);
  FFP_API_END
}

int ffp_rtdetr_mem_bytes(ffp_rtdetr* r, uint64_t* out_plan_bytes, int32_t* out_plans_resident) {
  FFP_API_BEGIN
  FFP_CHECK(r, FFP_ERR_ARG, "null handle");
  size_t b = 0;
  int n = 0;
  r->eng.mem_bytes(&b, &n);
  if (out_plan_bytes) *out_plan_bytes = b;
  if (out_plans_resident) *out_plans_resident = n;
  FFP_API_END
}

int ffp_rtdetr_drop_plans(ffp_rtdetr* r) {
  FFP_API_BEGIN
  FFP_CHECK(r, FFP_ERR_ARG, "null handle");
  r->eng.drop_plans();
  FFP_API_END
}

int ffp_rtdetr_set_profile(ffp_rtdetr* r, int on) {
  FFP_API_BEGIN
  FFP_CHECK(r, FFP_ERR_ARG, "null handle");
  r->eng.profile = on != 0;
  FFP_API_END
}

int ffp_rtdetr_profile_count(ffp_rtdetr* r, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(r && out_n, FFP_ERR_ARG, "null argument");
  *out_n = (int32_t)r->eng.profile_ms.size();
  FFP_API_END
}

int ffp_rtdetr_profile_get(ffp_rtdetr* r, int i, char* name, int name_cap, float* out_ms) {
  FFP_API_BEGIN
  FFP_CHECK(r && name && name_cap > 0 && out_ms, FFP_ERR_ARG, "null argument");
  FFP_CHECK(i >= 0 && i < (int)r->eng.profile_ms.size(), FFP_ERR_ARG, "profile entry %d of %d", i, (int)r->eng.profile_ms.size());
  const auto& e = r->eng.profile_ms[i];
  const size_t k = std::min(e.first.size(), (size_t)name_cap - 1);
  std::memcpy(name, e.first.data(), k);
  name[k] = 0;
  *out_ms = e.second;
  FFP_API_END
}

int ffp_rtdetr_info(ffp_rtdetr* r, int32_t* out_nc, double* out_last_conv_flops, int32_t* out_graph_state) {
  FFP_API_BEGIN
  FFP_CHECK(r, FFP_ERR_ARG, "null handle");
  if (out_nc) *out_nc = r->eng.nc();
  if (out_last_conv_flops) *out_last_conv_flops = r->eng.last_conv_flops;
  if (out_graph_state) *out_graph_state = r->eng.last_graph_state;
  FFP_API_END
}

}  // extern "C"
