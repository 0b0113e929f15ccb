// iqa.hpp — no-reference image quality on the device (iqa.hip): NIQE (Mittal, Soundararajan, Bovik 2013) with the choices
// pyiqa 0.1.x makes, as far as they can be stated without the package. The pixel path (luma, half-size
// image, MSCN maps, the 26 running sums of a block) is fp32 HIP; the closed-form AGGD fit of a block's sums and the score
// (36-vector, 36x36 matrix) are float64.
#pragma once
#include "common.hpp"

namespace ffp {

constexpr int kNiqeBlock = 96;      // block side at scale 1 (48 at scale 2)
constexpr int kNiqeFeat = 36;       // features per block: 18 per scale
constexpr int kNiqeGam = 9801;      // AGGD shape grid 0.2, 0.201, ..., 10.0

// blocks of an h x w image: floor(h / 96) * floor(w / 96)
inline int64_t niqe_blocks(int h, int w) { return (int64_t)(h / kNiqeBlock) * (w / kNiqeBlock); }

class IqaEngine {
 public:
  explicit IqaEngine(int device);
  ~IqaEngine();
  IqaEngine(const IqaEngine&) = delete;
  IqaEngine& operator=(const IqaEngine&) = delete;
  int device() const { return dev_; }

  // n images; image i is h[i] x w[i] with c[i] (1 or 3) channels. layout FFP_IQA_F32_CHW: float32 planar in [0,1], RGB;
  // FFP_IQA_U8_HWC: uint8 interleaved, chan_order FFP_CHAN_AS_BGR / FFP_CHAN_AS_RGB. on_device: imgs[i] are device pointers
  // (the caller has synchronised their producer). out_feat [blocks][36] float64, out_sharp [blocks] (mean sigma of the scale-1 block),
  // out_off [n + 1] block offsets; cap_blocks: capacity of out_feat / out_sharp in blocks.
  void niqe_features(int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout, int chan_order,
                     bool on_device, double* out_feat, double* out_sharp, int64_t cap_blocks, int64_t* out_off);
  // the rounded luma of one host image's crop (parity tests): out_y [floor(h/96)*96][floor(w/96)*96]
  void luma(const void* img, int h, int w, int c, int layout, int chan_order, float* out_y);

 private:
  long long stage(int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout, int chan_order, bool on_device,
                  int64_t* out_off, long long* max_px);
  int dev_;
  hipStream_t st_ = nullptr;
  DevBuf tabs_;                     // double [4][kNiqeGam]: r(gam), Gamma(1/gam), Gamma(2/gam), Gamma(3/gam)
  DevBuf consts_;                   // float [10 + 10]: the ten distinct weights of the 7x7 Gaussian, the ten half-size taps
  DevBuf src_, y1_, tmp_, y2_, sums_, feat_, sharp_, imgtab_;
};

// host, float64: one NIQE score per image from its blocks' features against the pristine model (mu [36], cov [36][36])
void niqe_score(const double* feat, const int64_t* block_off, int n, const double* mu, const double* cov, double* out);

}  // namespace ffp
