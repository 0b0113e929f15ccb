// rtdetr.hpp — Ultralytics RT-DETR-l (rtdetr-l.yaml, eval path) as a plan of HIP launches: every conv and every Linear over tokens on the
// shared conv kernels, everything else (LayerNorm, softmax, attention, top-k, deformable sampling) in rtdetr_ops.hip, fp32.
#pragma once
#include "engine.hpp"
#include "plan_cache.hpp"
#include "sliced.hpp"

namespace ffp {

constexpr int RT_NQ = 300;
constexpr int RT_TILES_DEFAULT_BATCH = FFP_RT_TILES_DEFAULT_BATCH;      // items per chunk when the caller passes max_batch <= 0 (include/ffp.h: measured)

// the three encoder levels: per-image token ranges [start[l], start[l + 1]) of [P3 | P4 | P5], their sizes and (enc_prep only) the
// input_proj outputs they are flattened from
struct RtLevels {
  int start[4];
  int h[3], w[3];
  const float* src[3];
  int src_cs[3];
};

void launch_rt_dwconv(const TView& in, const TView& out, const float* w, const float* b, int k, int s, int act, hipStream_t st);
void launch_rt_maxpool2(const TView& in, const TView& out, hipStream_t st);
void launch_rt_add(const TView& a, const float* b, int b_cs, long long period, const TView& out, hipStream_t st);
void launch_rt_layernorm(const TView& x, const float* gamma, const float* beta, const TView& out, hipStream_t st);
void launch_rt_gelu(const TView& x, hipStream_t st);
void launch_rt_attention(const TView& qk, const TView& v, const TView& out, int L, hipStream_t st);
void launch_rt_enc_prep(const RtLevels& lv, const float* valid, const TView& t, const TView& tm, int n, hipStream_t st);
void launch_rt_topk(const TView& s, int nc, int NT, int n, unsigned* keys, int* idx, hipStream_t st);
void launch_rt_gather(const TView& e, const int* idx, const float* anchors, int NT, int n, const TView& q, float* anc, hipStream_t st);
void launch_rt_ref(const TView& delta, const float* anc, const TView& ref, hipStream_t st);
void launch_rt_deform(const TView& val, const TView& oa, const TView& ref, const RtLevels& lv, const TView& out, hipStream_t st);
void launch_rt_raw(const TView& ref, const TView& s, int nc, float* raw, hipStream_t st);
void launch_rt_post(const TView& ref, const TView& s, int nc, float conf, const float2* orig_wh, int n, float* det, int* counts, hipStream_t st);
// rt_post for n tiles {x0, y0, x1, y1} of a full_h x full_w frame; mode FFP_RT_TILES_LOCAL (crop-local rows, as rt_post) or FFP_RT_TILES_SAHI
// (clipped against the full shape, invalid boxes dropped, shifted by the tile origin). det [n][300][6], counts [n]
void launch_rt_post_tiles(const TView& ref, const TView& s, int nc, float conf, const int4* tiles_xyxy, int n, int full_h, int full_w, int mode,
                          float* det, int* counts, hipStream_t st);

// host tables, constant per imgsz (RTDETRDecoder._generate_anchors, AIFI.build_2d_sincos_position_embedding)
void rtdetr_anchors(int imgsz, std::vector<float>& anchors, std::vector<float>& valid);
void rtdetr_pos_embed(int w, int h, std::vector<float>& pos);
// depthwise weights (C, 1, k, k) -> [tap][C], the layout rt_dwconv reads
std::vector<float> rtdetr_pack_depthwise(const float* w, int C, int taps);

// the letterbox record of one source rectangle: LetterBox(imgsz, auto=False, scale_fill=True), a stretch to imgsz x imgsz without padding
LetterboxImg rtdetr_stretch(int x0, int y0, int sw, int sh, int imgsz);
// ... of every tile {x0, y0, x1, y1} of an H x W frame (an empty, inverted or outside tile is FFP_ERR_ARG): what the sliced path runs and what
// ffp_op_image_input hands letterbox_kernel
void rtdetr_tile_records(int H, int W, const int32_t* tiles, int n_tiles, int imgsz, std::vector<LetterboxImg>& lb);

struct RtdetrPlan : Plan {
  int n = 0, imgsz = 0, NT = 0;
  void add_named(const std::string& name, std::function<void(hipStream_t)> f) { add(std::move(f)); steps.back().name = name; }
  TView input, ref, scores;
  DevBuf d_lb, d_wh, d_anchors, d_valid, d_pos, d_keys, d_idx, d_anc, d_raw, d_det, d_counts;
};

class RtdetrEngine {
 public:
  RtdetrEngine(const void* weights, size_t nbytes, int device, int precision);
  ~RtdetrEngine();
  int nc() const { return nc_; }
  // images: n host BGR u8 frames (sizes may differ); out: [n][300][6] {x1, y1, x2, y2, score, cls} in original pixels, counts[n]
  void predict(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float conf, float* out, int32_t* counts);
  // out: [n][300][4 + nc] {cx, cy, w, h (normalised), sigmoid scores}; topk (may be null): [n][300] encoder token of every query
  void forward_raw(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float* out, int32_t* topk);
  // Tiles [x0, y0, x1, y1] (frame pixels) of one H x W x 3 u8 frame, each stretched to imgsz x imgsz as predict() stretches an image, in
  // chunks of at most max_batch items (<= 0: RT_TILES_DEFAULT_BATCH) split as evenly as ceil(n / max_batch) chunks allow. out [n_tiles][300][6],
  // counts [n_tiles]; mode: launch_rt_post_tiles. The host form uploads the frame once; the device form takes device pointers throughout.
  // Both return after the engine's stream has drained.
  void infer_tiles(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf, int mode,
                   int max_batch, float* out, int32_t* counts);
  void infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf, int mode,
                       int max_batch, float* d_out, int32_t* d_counts);
  // get_sliced_prediction in one call: `items` (the slice grid and, where asked for, the full-frame tile) in FFP_RT_TILES_SAHI mode, rows in
  // tile order then query order into the SAHI merge. out [cap][6]; *out_n is the merged count even when it exceeds cap (FFP_ERR_ARG then).
  void sliced_predict(const uint8_t* frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int imgsz, float conf, int max_batch,
                      int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* out, int cap, int32_t* out_n);
  void mem_bytes(size_t* plans, int* resident) const { *plans = plans_.bytes(); *resident = (int)plans_.size(); }
  void drop_plans() { plans_.clear(); }      // waits for the stream first
  // profile: the next calls run their plan eagerly with a pair of events around every launch (no hipGraph); profile_ms holds the last call's
  // {"<kernel> <layer>", ms} per launch in issue order
  bool profile = false;
  std::vector<std::pair<std::string, float>> profile_ms;
  double last_conv_flops = 0;
  int last_graph_state = 0;

 private:
  void enqueue_tiles(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf, int mode,
                     int max_batch, float* d_out, int32_t* d_counts);
  RtdetrPlan* prepare(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz);
  RtdetrPlan* plan_for(int n, int imgsz);
  void build_plan(RtdetrPlan& P);
  const PackedConv& conv(const std::string& name);           // packed once per engine
  const HostTensor& t(const std::string& name) const { return wf_.get(name); }
  const float* dev(const std::string& name);                  // fp32 copy on the device (LayerNorm parameters, depthwise weights)

  std::vector<uint8_t> bytes_;
  WeightFile wf_;
  std::map<std::string, std::unique_ptr<PackedConv>> convs_;
  std::map<std::string, DevBuf> dev_;
  PlanCache<std::vector<int>, RtdetrPlan> plans_{4, 0, [this] { FFP_HIP(hipSetDevice(device_)); FFP_HIP(hipStreamSynchronize(st_)); }};
  int device_ = 0, nc_ = 0;
  bool split_ = false;
  hipStream_t st_ = nullptr;
  DevBuf frame_;
  // the tile path: per-call tables (host copies live until the stream has drained) and the fused call's scratch
  std::vector<LetterboxImg> h_lb_;
  DevBuf tiles_lb_, tiles_xy_, tile_dets_, tile_counts_;
  SlicedTail tail_;
};

}  // namespace ffp
