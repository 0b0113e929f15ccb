// sliced.cpp — see sliced.hpp.
#include <algorithm>

#include "sliced.hpp"

namespace ffp {

std::vector<int32_t> slice_bboxes(int H, int W, int sh, int sw, float oh, float ow) {
  FFP_CHECK(H > 0 && W > 0 && sh > 0 && sw > 0, FFP_ERR_ARG, "slice_bboxes: sizes must be positive");
  FFP_CHECK(oh >= 0.f && oh < 1.f && ow >= 0.f && ow < 1.f, FFP_ERR_ARG, "slice_bboxes: overlap ratio must be in [0,1)");
  std::vector<int32_t> out;
  int y_max = 0, y_min = 0;
  const int y_overlap = (int)((double)oh * sh), x_overlap = (int)((double)ow * sw);
  while (y_max < H) {
    int x_min = 0, x_max = 0;
    y_max = y_min + sh;
    while (x_max < W) {
      x_max = x_min + sw;
      if (y_max > H || x_max > W) {
        const int xmax = std::min(W, x_max), ymax = std::min(H, y_max);
        const int xmin = std::max(0, xmax - sw), ymin = std::max(0, ymax - sh);
        out.insert(out.end(), {xmin, ymin, xmax, ymax});
      } else {
        out.insert(out.end(), {x_min, y_min, x_max, y_max});
      }
      x_min = x_max - x_overlap;
    }
    y_min = y_max - y_overlap;
  }
  return out;
}

std::vector<int32_t> sliced_items(int H, int W, int slice_h, int slice_w, float oh, float ow, int perform_standard_pred) {
  FFP_CHECK(H > 0 && W > 0, FFP_ERR_ARG, "frame is empty");
  std::vector<int32_t> items = slice_bboxes(H, W, slice_h, slice_w, oh, ow);
  if (items.size() / 4 > 1 && perform_standard_pred) items.insert(items.end(), {0, 0, W, H});   // sahi/predict.py: the full-frame pass
  return items;
}

std::vector<int> even_chunks(int n, int max_batch) {
  FFP_CHECK(n >= 0 && max_batch >= 1, FFP_ERR_ARG, "even_chunks: %d items in chunks of at most %d", n, max_batch);
  const int chunks = (n + max_batch - 1) / max_batch;
  std::vector<int> v(chunks, chunks ? n / chunks : 0);
  for (int i = 0; i < (chunks ? n % chunks : 0); ++i) ++v[i];
  return v;
}

void upload_frame(DevBuf& dst, const uint8_t* frame, int H, int W, hipStream_t st) {
  FFP_CHECK(frame && H > 0 && W > 0, FFP_ERR_ARG, "frame is null or empty");
  const size_t nb = (size_t)H * W * 3;
  dst.ensure(nb);
  FFP_HIP(hipMemcpyAsync(dst.p, frame, nb, hipMemcpyHostToDevice, st));
}

void SlicedTail::compact(const float* d_dets, const int* d_counts, int n_tiles_, int tile_cap, int stride_, hipStream_t st) {
  n_tiles = n_tiles_, stride = stride_;
  rows.ensure(sizeof(float) * (size_t)n_tiles * tile_cap * stride);
  rows_n.ensure(sizeof(int));
  prefix.ensure(sizeof(int) * (n_tiles + 1));
  launch_compact_rows(d_dets, d_counts, n_tiles, tile_cap, stride, rows.as<float>(), rows_n.as<int>(), prefix.as<int>(), st);
}

void SlicedTail::merge(MergeRule rule, int n_rows, int type, int metric, double thr, int class_agnostic, float* d_out, int* d_out_src, int* d_out_n,
                       int cap, hipStream_t st, int clip_first_row, int clip_w, int clip_h) {
  if (rule == MergeRule::Always || (n_tiles > 1 && n_rows > 1))
    run_merge(work, rows.as<float>(), rows_n.as<int>(), n_rows, stride, type, metric, thr, class_agnostic, d_out, d_out_src, d_out_n, cap, st, clip_first_row, clip_w, clip_h);
  else run_merge_passthrough(rows.as<float>(), rows_n.as<int>(), stride, d_out, d_out_src, d_out_n, cap, st);
}

void SlicedTail::fetch(float* out, int cap, int stride_, int32_t* out_n, const char* what, hipStream_t st) {
  const auto read_back = [st](void* dst, const void* src, size_t nb) {
    if (!st) { FFP_HIP(hipMemcpy(dst, src, nb, hipMemcpyDeviceToHost)); return; }
    FFP_HIP(hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToHost, st));
    FFP_HIP(hipStreamSynchronize(st));
  };
  int k = 0;
  read_back(&k, merged_n.p, sizeof(int));
  *out_n = k;
  FFP_CHECK(k <= cap, FFP_ERR_ARG, "%s: %d merged detections exceed the output capacity %d (nothing was dropped silently: call again with cap >= %d)", what, k, cap, k);
  read_back(out, merged.p, sizeof(float) * (size_t)k * stride_);
}

}  // namespace ffp
