// sr_ops.hpp — Real-ESRGAN pre/post kernels (sr_ops.hip) and the SR engine (rrdb.cpp).
#pragma once
#include "engine.hpp"
#include "plan_cache.hpp"
#include "sr_tiles.hpp"

namespace ffp {

// sr_tiles (sr_tiles.hpp) with its refusals raised as FFP_ERR_ARG (rrdb.cpp)
std::vector<SrTile> sr_tiles_checked(const std::vector<SrImage>& imgs, int scale, int tile, int tile_pad, int pre_pad);

void launch_sr_pre(const uint8_t* d_base, const SrSrc* d_srcs, const TView& out, int shuf, hipStream_t st);
void launch_sr_post(const TView& net_out, const SrDst* d_dsts, const long long* d_core_off, long long total_core, uint8_t* d_base,
                    hipStream_t st);
// realesrgan's post-resizes (resize.hip). The Lanczos4 tables are built on the host (libm sin / cos in double) and read as is.
struct Lanczos4Axis {           // one axis of cv::resize(INTER_LANCZOS4): first tap sx - 3 and 8 weights per output index
  std::vector<int> ofs;         // sx (taps sx-3 .. sx+4, clamped to [0, n_in - 1] by the kernel)
  std::vector<float> coef;      // 8 per output index (16-bit path)
  std::vector<int16_t> icoef;   // rint(coef * 2048) (8-bit path)
};
Lanczos4Axis lanczos4_axis(int n_in, int n_out);
// src: h x w x cn (u8 or u16), dst: out_h x out_w x cn. The table (lanczos4_pack) holds xofs[out_w], yofs[out_h] as int, then
// 8 coefficients per output column and per output row: float for 16-bit (wide) data, int16 for 8-bit data.
size_t lanczos4_table_bytes(int out_h, int out_w);
void lanczos4_pack(const Lanczos4Axis& ax, const Lanczos4Axis& ay, int wide, void* host_tab);
void launch_resize_lanczos4(const void* d_src, int h, int w, int cn, int wide, const void* d_tab, int out_h, int out_w, void* d_dst,
                            hipStream_t st);
// the host side of a Lanczos4 resize (rrdb.cpp): tables built here, uploaded on `st` into `tab` (the host copy must outlive the upload)
void resize_lanczos4_dev(const void* d_src, int h, int w, int cn, int wide, int out_h, int out_w, void* d_dst, DevBuf& tab,
                         std::vector<uint8_t>& host_tab, hipStream_t st);
// the 'cv2' alpha upsampler: cv2.resize(alpha / range, (out_w, out_h), INTER_LINEAR) in float32, quantised to rint(a * range)
// into channel 3 of a 4-channel canvas of 8-bit (dst_wide 0) or 16-bit elements; src is the 4-channel input
void launch_alpha_linear(const void* d_src, int h, int w, int src_wide, float range, int out_h, int out_w, void* d_dst, int dst_wide,
                         hipStream_t st);

void launch_crop_gather(const uint8_t* d_frame, int W, const int4* d_boxes, const long long* d_offs, int n, uint8_t* d_out,
                        hipStream_t st);

// A plan is laid out for a CAPACITY (16x16 tiles at the body level), not for a list of image sizes: its levels are in
// capacity mode (Level::reserve / assign), so one allocated, tuned and graph-captured plan serves every batch that fits.
struct SrPlan : Plan {
  Level* Lb = nullptr;     // body level (input res, or half res for x2)
  Level* L1 = nullptr;     // x2 of body
  Level* L2 = nullptr;     // x4 of body
  TView input, out;
  DevBuf d_srcs, d_dsts, d_core_off;
  int cap_t16 = 0;
  void* stage = nullptr;   // pinned staging of the per-batch tile descriptors
  size_t stage_bytes = 0;
  ~SrPlan();
};

class SrEngine {
 public:
  SrEngine(const void* weights, size_t nbytes, int scale, int num_block, int device, int half);
  ~SrEngine();
  int scale() const { return scale_; }
  int device() const { return device_; }
  hipStream_t stream() const { return st_; }
  // all images live in device memory: inputs at d_in + in_off (in_fmt, in_stride bytes/row), outputs at d_out + out_off (out_fmt)
  // wait = false: return as soon as the work is enqueued on the engine's stream (wait_done() completes it), so that the
  // caller can overlap the next frame's detection (own stream) with this frame's super-resolution
  void enhance_dev(const uint8_t* d_in, uint8_t* d_out, const std::vector<SrImage>& imgs, int tile, int tile_pad, int pre_pad, bool wait = true);
  void wait_done();
  // the body (every conv of the residual dense blocks) as ONE persistent launch (conv_trunk.hip) or one launch per layer; bit-identical
  // results either way. Default: per-layer launches; FFP_TRUNK=1 makes the fused launch the default of fp16 handles. Changing it drops the resident plans.
  void set_fused_body(bool on);
  bool fused_body() const { return fused_body_; }
  void drop_plans() { plans_.clear(); }      // release every resident plan (waits for the batch in flight and the stream first)
  size_t plan_bytes() const { return plans_.bytes(); }      // device memory held by the resident plans (activations, tables), without the packed weights
  size_t weight_bytes() const { return weight_bytes_; }
  int plans_resident() const { return (int)plans_.size(); }

  DevBuf scratch_in, scratch_out, scratch_boxes, scratch_offs, scratch_tab;
  HostPinned crop_stage;
  ConvProfile prof;
  float last_ms = 0.f;
  double last_conv_flops = 0;
  int last_conv_launches = 0;
  bool last_graph = false;      // the last call replayed a captured hipGraph (false: eager launches)
  int plans_built = 0;          // plans laid out so far (a steady stream of varying crop sizes must not grow this)

 private:
  void build_plan(SrPlan& P, int cap_t16);
  SrPlan& plan_for(long long t16);
  const PackedConv* conv(const std::string& name) const;
  std::map<std::string, PackedConv> convs_;
  // keyed by capacity; at most 4 buckets
  PlanCache<int, SrPlan> plans_{4, 0, [this] { FFP_HIP(hipSetDevice(device_)); if (pending_) wait_done(); FFP_HIP(hipStreamSynchronize(st_)); }};
  int scale_ = 4, num_block_ = 23, device_ = 0;
  DType dt_ = F16;
  hipStream_t st_ = nullptr;
  hipEvent_t ev_[2];
  bool pending_ = false;
  bool fused_body_ = false;
  size_t weight_bytes_ = 0;
};

}  // namespace ffp
