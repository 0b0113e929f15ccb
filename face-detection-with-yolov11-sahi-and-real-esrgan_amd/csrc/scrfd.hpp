// scrfd.hpp — the face detector of InsightFace's model packs (SCRFD, det_*.onnx behind insightface.app.FaceAnalysis) as a plan
// of HIP launches: the ONNX graph is lowered on the host (onnx_graph.hpp) onto the shared conv kernels plus scrfd_ops.hip.
#pragma once
#include "engine.hpp"
#include "plan_cache.hpp"
#include "sliced.hpp"
#include "onnx_graph.hpp"

namespace ffp {

// one candidate of RetinaFace.detect after the score threshold: box and keypoints in crop pixels (already / det_scale)
struct ScrfdCand {
  float b[4];
  float score;
  int idx;          // anchor number within the image (level, pixel, anchor): the tie-break of the NMS order
  float k[10];
};

struct ScrfdHeads {
  const float* score[3];
  const float* bbox[3];
  const float* kps[3];          // nullptr: the 6-output variant
  int cs[3][3], coff[3][3];     // [score|bbox|kps][level]
  const int4* tab[3];           // level tables {off, h, w, 0}
  int stride[3];
  int a_off[4];                 // first anchor number of each level within an image; a_off[3] = anchors per image
  int per_img, A;
  const float* det_scale;       // [image] float32(new_h / h)
};

void launch_scrfd_preproc(const uint8_t* d_frame, int W, int flip, const LetterboxImg* d_imgs, const TView& out, hipStream_t st);
void launch_scrfd_pool(const TView& in, const TView& out, int maxpool, int k, hipStream_t st);
// raw_scores (may be null): every anchor's score; cand / counts (may be null): the candidates >= thresh
void launch_scrfd_decode(const ScrfdHeads& h, int n_img, float thresh, ScrfdCand* cand, int* counts, float* raw_scores, hipStream_t st);
void launch_scrfd_nms(const ScrfdCand* cand, const int* counts, int n_img, int per_img, int* order, int* supp, float thresh, float* out, int cap,
                      int* out_counts, hipStream_t st);

// the wrapper's conversion and sahi's clip / shift on the rows launch_scrfd_nms wrote (FFP_SCRFD_TILES_SAHI, include/ffp.h: ffp_op_scrfd_sahi_rows),
// in place: dets [n_tiles][cap][FFP_DET_STRIDE(5)], counts [n_tiles] (uncapped on entry, rewritten), tiles {x0, y0, x1, y1}. *err (device):
// SCRFD_NO_BAD_ROW, or the smallest tile * cap + row of a box whose far corner is negative after the clip
constexpr unsigned SCRFD_NO_BAD_ROW = 0xffffffffu;
constexpr int SCRFD_TILES_DEFAULT_BATCH = FFP_SCRFD_TILES_DEFAULT_BATCH;     // items per chunk when the caller passes max_batch < 0 (include/ffp.h: measured)
void launch_scrfd_sahi_rows(float* dets, int* counts, const int4* tiles_xyxy, int n_tiles, int cap, float conf, int full_h, int full_w, unsigned* err,
                            hipStream_t st);

// RetinaFace.detect geometry of one (h, w) crop at net size (W, H): {new_w, new_h}; det_scale = float32(new_h / h). new_w or new_h may be 0.
void scrfd_geometry(int h, int w, int net_w, int net_h, int* new_w, int* new_h, float* det_scale);

// the record (picture at the top-left of a net_w x net_h canvas) and det_scale of every tile {x0, y0, x1, y1} of an H x W frame; a tile outside the
// frame, or one that resizes to nothing, is FFP_ERR_ARG: what the engine runs and what ffp_op_image_input hands scrfd_preproc_kernel
void scrfd_tile_records(int net_w, int net_h, int H, int W, const int32_t* tiles, int n_tiles, std::vector<LetterboxImg>& lb, std::vector<float>& scale);

struct ScrfdPlan : Plan {
  onnx::Lowered low;
  std::vector<TView> views;                // by lowered buffer
  std::vector<std::unique_ptr<PackedConv>> convs;
  ScrfdHeads heads{};
  DevBuf d_lb, d_scale, d_cand, d_counts, d_order, d_supp, d_out, d_out_counts, d_raw_scores;
};

class ScrfdEngine {
 public:
  ScrfdEngine(const void* onnx, size_t nbytes, int n, int device, int precision);
  ~ScrfdEngine();
  int device() const { return device_; }
  hipStream_t stream() const { return st_; }
  int n_outputs() const { return (int)graph_.outputs.size(); }
  // crops of a host frame -> per-crop detections (host): FFP_DET_STRIDE(5) rows, crop-local float coordinates
  void infer_tiles(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float det_thresh,
                   float nms_thresh, float* out, int cap, int32_t* out_counts);
  // the graph outputs of every crop (host): per tile, per output, [anchors * values] in the file's NHWC-reshaped order; scores after the sigmoid
  void forward_raw(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float* out, size_t cap,
                   int64_t* out_sizes);
  // The same crops in chunks of at most max_batch items (0: one batch, as infer_tiles; < 0: FFP_SCRFD_TILES_DEFAULT_BATCH) split as evenly as
  // ceil(n / max_batch) chunks allow, one plan per chunk size; every chunk's decode and NMS write its slice of the output. mode
  // FFP_SCRFD_TILES_LOCAL: infer_tiles' rows; FFP_SCRFD_TILES_SAHI: launch_scrfd_sahi_rows over them at `conf`. Rows past a tile's count are
  // zero in the host form. The device form takes the frame and both outputs as device pointers (tiles stay on the host). Both return after
  // the engine's stream has drained; a tile with more than cap faces, or a negative far corner in SAHI mode, is FFP_ERR_ARG.
  void infer_tiles_ex(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float det_thresh,
                      float nms_thresh, float conf, int mode, int max_batch, float* out, int cap, int32_t* out_counts);
  void infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float det_thresh,
                       float nms_thresh, float conf, int mode, int max_batch, float* d_out, int cap, int32_t* d_out_counts);
  // get_sliced_prediction in one call: `items` (the slice grid and, where asked for, the full-frame tile) in FFP_SCRFD_TILES_SAHI mode with at
  // most tile_cap faces per item, rows in tile order then score order into the SAHI merge. out [cap][FFP_DET_STRIDE(5)]. Host form: *out_n is the
  // merged count even when it exceeds cap (FFP_ERR_ARG then). Device form: d_out / d_out_n on the device, the count untruncated (ffp_merge_dev).
  void sliced_predict(const uint8_t* frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int det_w, int det_h, float det_thresh,
                      float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric, double pp_thr, int class_agnostic,
                      float* out, int cap, int32_t* out_n);
  void sliced_predict_dev(const uint8_t* d_frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int det_w, int det_h,
                          float det_thresh, float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric, double pp_thr,
                          int class_agnostic, float* d_out, int cap, int32_t* d_out_n);
  void mem_bytes(size_t* plans, int* resident) const { *plans = plans_.bytes(); *resident = (int)plans_.size(); }
  void drop_plans() { plans_.clear(); }      // waits for the stream first
  double last_conv_flops = 0;
  int last_graph_state = 0;
  size_t plan_bytes() const { return plans_.bytes(); }

 private:
  ScrfdPlan* prepare(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h);
  // the geometry of every tile into h_lb_ / h_scale_ at the net size `first` was lowered for
  void tile_geometry(const ScrfdPlan& first, int H, int W, const int32_t* tiles, int n_tiles);
  // tiles [off, off + m) through P, nothing waited for: the tables, the pre-processing and the plan
  void run_chunk(ScrfdPlan* P, const uint8_t* d_frame, int W, int chan_order, int off, int m);
  // everything on st_, nothing waited for; check_tiles() after the stream has drained
  void enqueue_tiles(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float det_thresh,
                     float nms_thresh, float conf, int mode, int max_batch, float* d_out, int cap, int32_t* d_out_counts);
  void check_tiles(int n_tiles, int cap, int mode);
  // compact + merge of tile_dets_ / tile_counts_ into d_out / d_out_n (one read back of the row count in between, where check_tiles runs)
  // full_last: the last tile is sahi's full-frame prediction, whose rows keep their full_shape through the merge (run_merge's clip)
  void merge_tiles(int n_tiles, int tile_cap, bool full_last, int H, int W, int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* d_out,
                   int cap, int32_t* d_out_n);
  ScrfdPlan* plan_for(int n, int det_w, int det_h);
  void build_plan(ScrfdPlan& P, int n, int det_w, int det_h);

  onnx::Graph graph_;
  PlanCache<std::vector<int>, ScrfdPlan> plans_{8, sw().det_plan_bytes(), [this] { FFP_HIP(hipSetDevice(device_)); FFP_HIP(hipStreamSynchronize(st_)); }};
  int device_ = 0;
  bool split_ = false;
  hipStream_t st_ = nullptr;
  DevBuf frame_;
  // the tile path: per-call tables (the host copies live until the stream has drained) and the fused call's scratch
  std::vector<LetterboxImg> h_lb_;
  std::vector<float> h_scale_;
  std::vector<int32_t> h_counts_;
  unsigned h_err_ = SCRFD_NO_BAD_ROW;
  DevBuf tiles_xy_, err_, tile_dets_, tile_counts_;
  SlicedTail tail_;
};

}  // namespace ffp
