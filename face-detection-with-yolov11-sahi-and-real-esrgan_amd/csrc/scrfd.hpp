// scrfd.hpp — the face detector of InsightFace's model packs (SCRFD, det_*.onnx behind insightface.app.FaceAnalysis) as a plan
// of HIP launches: the ONNX graph is lowered on the host (onnx_graph.hpp) onto the shared conv kernels plus scrfd_ops.hip.
#pragma once
#include "engine.hpp"
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

// RetinaFace.detect geometry of one (h, w) crop at net size (W, H): {new_w, new_h}; det_scale = float32(new_h / h). new_w or new_h may be 0.
void scrfd_geometry(int h, int w, int net_w, int net_h, int* new_w, int* new_h, float* det_scale);

struct ScrfdPlan : Plan {
  unsigned long long last_use = 0;
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
  double last_conv_flops = 0;
  int last_graph_state = 0;
  size_t plan_bytes() const;

 private:
  ScrfdPlan* prepare(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h);
  ScrfdPlan* plan_for(int n, int det_w, int det_h);
  void build_plan(ScrfdPlan& P, int n, int det_w, int det_h);

  onnx::Graph graph_;
  std::map<std::vector<int>, std::unique_ptr<ScrfdPlan>> plans_;
  unsigned long long use_clock_ = 0;
  int device_ = 0;
  bool split_ = false;
  hipStream_t st_ = nullptr;
  DevBuf frame_;
};

}  // namespace ffp
