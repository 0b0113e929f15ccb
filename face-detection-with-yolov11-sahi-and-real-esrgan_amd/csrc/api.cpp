// api.cpp — the C-ABI of libffp.so (include/ffp.h), part one of four: the entries that go through a handle (detector, enhancer, SCRFD, RT-DETR, NIQE)
// and the pure host helpers. The entries that take a device number are in api_eval.cpp (merge, evaluators), api_codec.cpp (JPEG, PNG) and
// api_ops.cpp (single operators); api_util.hpp holds what the four share. Every entry point catches engine exceptions, stores a thread-local
// message and returns an error code; nothing here computes on the CPU.
#include "api_util.hpp"
#include "iqa.hpp"
#include "rtdetr.hpp"
#include "scrfd.hpp"
#include "sliced.hpp"
#include "sr_ops.hpp"
#include "yolo11.hpp"

struct ffp_det { ffp::DetEngine eng; ffp_det(const void* w, size_t n, int a, int nc, int nk, int dev, int pr) : eng(w, n, a, nc, nk, dev, pr) {} };
struct ffp_rtdetr { ffp::RtdetrEngine eng; ffp_rtdetr(const void* b, size_t nb, int dev, int pr) : eng(b, nb, dev, pr) {} };
struct ffp_scrfd { ffp::ScrfdEngine eng; ffp_scrfd(const void* b, size_t nb, int n, int dev, int pr) : eng(b, nb, n, dev, pr) {} };
struct ffp_iqa { ffp::IqaEngine eng; explicit ffp_iqa(int dev) : eng(dev) {} };
struct ffp_sr { ffp::SrEngine eng; ffp_sr(const void* w, size_t n, int s, int nb, int dev, int h) : eng(w, n, s, nb, dev, h) {} };

using namespace ffp;

namespace {

void upload_frame(DetEngine& e, const uint8_t* frame, int H, int W) {
  FFP_HIP(hipSetDevice(e.device()));
  ffp::upload_frame(e.scratch_frame, frame, H, W, e.stream());
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

int ffp_switches(char* out, size_t cap) {
  FFP_API_BEGIN
  const std::string text = ffp::switches_report(ffp::sw_live());
  FFP_CHECK(out && cap > text.size(), FFP_ERR_ARG, "ffp_switches: the report needs %zu bytes", text.size() + 1);
  memcpy(out, text.c_str(), text.size() + 1);
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
