// yolo11.hpp — the detector engine: YOLO11{n,s}-pose laid out as a plan of HIP launches per ragged batch shape.
#pragma once
#include "engine.hpp"
#include "plan_cache.hpp"
#include "sliced.hpp"

namespace ffp {

struct DetPlan : Plan {
  Level* L[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // strides 1,2,4,8,16,32
  TView input;
  TView head[3];
  std::vector<int> anchor_off;
  DevBuf d_anchor_off, d_boxes, d_scores, d_classes, d_cand, d_cscore, d_lb, d_imgs;
  int total_anchors = 0;
  ConvOp stem;              // model.0 when it is fused with the letterbox (runs ahead of the captured launch sequence)
  bool fused_stem = false;
  // fp32-split plans of YOLO11s: model.0 is computed inside model.1's loader (launch_stem_conv) and its output never stored
  ConvOp stemconv;
  bool fused_stem_conv = false;
  std::string stemconv_variant;
  DevBuf stem_w[2];         // the stem's MFMA fragments per channel order (RGB, BGR frames)
  // the gate of the box and keypoint towers (build_plan): active[i] != 0 = item i has an anchor whose class score passes *d_conf. Cleared and
  // written in every run by the gate step behind the class towers, copied to the host behind decode / NMS.
  bool gate = false;
  DevBuf d_active, d_conf;
  double gate_share[3] = {1, 1, 1};      // per head level: active share of its pixels in the last profiled run (Step::share of the gated convs)
};

struct TileGeom {       // host-side geometry of one crop
  LetterboxImg lb;
  DetImg di;
};

class DetEngine {
 public:
  DetEngine(const void* weights, size_t nbytes, int arch, int nc, int nkpt, int device, int precision);
  ~DetEngine();

  int det_stride() const { return 6 + 3 * nkpt_; }
  // Plan::lanes of every plan built from now on (cached plans are dropped): parallel graph branches for the head towers and C3k
  void set_lanes(int mode) { if (mode != lanes_) { plans_.clear(); lanes_ = mode; } }
  // Plan::reuse of every plan built from now on (cached plans are dropped): 0 a device block per activation tensor, 1 (default; env
  // FFP_DET_ARENA sets another default for A/B runs) tensors whose lifetimes do not overlap share bytes, 2 as 1 with released ranges
  // overwritten by 0xFF bytes. Results are bit-identical in all three.
  void set_buffer_reuse(int mode) { plans_.clear(); reuse_ = mode; }
  int buffer_reuse() const { return reuse_; }
  // skip the box and keypoint towers of items without a class score above conf (on by default; env FFP_DET_GATE=0 sets the default to off).
  // Results are bit-identical either way. Cached plans are dropped.
  void set_gate(bool on);
  // items whose towers ran in the last infer_tiles_dev / forward_raw call, of how many (gate off: all of them)
  void last_active(int* active, int* items) const;
  // summed over the resident plans: bytes held for Plan::alloc tensors, what one block per tensor would hold, and the maximum over
  // build order of the bytes live at once (the floor of any placement)
  void mem_detail(size_t* activation, size_t* no_reuse, size_t* peak_live) const;
  void fill_counts(int* fill_steps, int* ranges_freed) const {     // summed over the resident plans (Plan::fill_steps, ranges_freed)
    *fill_steps = *ranges_freed = 0;
    plans_.for_each([&](const DetPlan& p) { *fill_steps += p.fill_steps; *ranges_freed += p.ranges_freed; });
  }
  int device() const { return device_; }
  hipStream_t stream() const { return st_; }
  int nc() const { return nc_; }
  int nkpt() const { return nkpt_; }
  // device memory: resident plans (activations + tables; one plan per batch shape, least recently used ones are dropped beyond 8 plans or
  // beyond sw().det_plan_bytes(), plan_cache.hpp) and the packed weights
  size_t plan_bytes() const { return plans_.bytes(); }
  void drop_plans() { plans_.clear(); }      // release every resident plan (the next call lays its plan out again); waits for the stream first
  size_t weight_bytes() const { return weight_bytes_; }
  int plans_resident() const { return (int)plans_.size(); }

  // crops of a device-resident frame -> per-crop detections (device), crop-local float coords
  void infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                       float conf, float iou, int max_det, int round_boxes, float* d_out_dets, int32_t* d_out_counts);
  // raw head output for parity tests, host output
  void forward_raw(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                   float* out_raw, size_t out_cap, int32_t* out_anchor_counts);
  // + int-truncate, clip, shift to frame coordinates (wrapper + SAHI shift semantics)
  void truncate_shift_dev(float* d_dets, const int32_t* d_counts, int n_tiles, int max_det, int H, int W);

  void merge_dev(const float* d_dets, const int32_t* d_counts, int n_slices, int max_det, int type, int metric, double thr,
                 int class_agnostic, float* d_out, int32_t* d_out_src, int cap, int32_t* d_out_n);

  // scratch the API layer may use (grown on demand)
  DevBuf scratch_frame, scratch_dets, scratch_counts, scratch_src;
  SlicedTail tail;
  ConvProfile prof;
  float last_ms[5] = {0, 0, 0, 0, 0};
  double last_conv_flops = 0;
  int last_conv_launches = 0;
  int last_graph_state = 0;     // Plan::graph_state() of the plan the last call ran
  hipEvent_t ev_[6];

 private:
  DetPlan* plan_for(const std::vector<TileGeom>& g);
  void build_plan(DetPlan& p, const std::vector<int>& hs, const std::vector<int>& ws);
  // conf: the gate's threshold for this call (what decode will test against; below 0: every item active)
  DetPlan* prepare(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf);
  void fetch_active(DetPlan* P, int n_tiles);
  void set_shares(DetPlan* P) const;
  const PackedConv* conv(const std::string& name) const;

  std::map<std::string, PackedConv> convs_;
  std::map<std::string, DenseF32> dense_;      // model.23.cv3.<l>.2 as plain fp32 (nc <= 4): the closing conv of the fused class tower (conv_dwpw.hip)
  PlanCache<std::vector<int>, DetPlan> plans_{8, sw().det_plan_bytes(), [this] { FFP_HIP(hipSetDevice(device_)); FFP_HIP(hipStreamSynchronize(st_)); }};
  std::vector<TileGeom> geom_last_;
  int lanes_ = 0;
  int reuse_ = sw().det_arena;      // FFP_DET_ARENA, or 1
  bool gate_ = sw().det_gate;       // FFP_DET_GATE, or on
  HostPinned h_active_;         // the gate's verdict of the last call
  bool last_gated_ = false;
  int last_items_ = 0;
  size_t weight_bytes_ = 0;
  int device_ = 0, nc_ = 1, nkpt_ = 5;
  char scale_ = 's';
  DType dt_ = F32;
  bool split_ = false;
  hipStream_t st_ = nullptr;
};

void letterbox_geometry(int h, int w, int imgsz, int32_t* out6);
// the letterbox record and the decode's gain / pad of every tile {x0, y0, x1, y1} of an H x W frame (imgsz <= 0: the first tile's long side rounded up
// to 32): what DetEngine runs, and what ffp_op_image_input / ffp_op_stem / ffp_op_stem_conv hand the image-input kernels
std::vector<TileGeom> det_tile_geometry(int H, int W, const int32_t* tiles, int n_tiles, int imgsz);

}  // namespace ffp
