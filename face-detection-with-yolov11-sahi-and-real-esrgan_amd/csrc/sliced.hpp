// sliced.hpp — the host side of sahi's get_sliced_prediction that the YOLO11, RT-DETR and SCRFD engines share ("Sliced prediction"):
// the items of a frame, their chunks, and the tail behind the per-tile detections. The first three functions make no HIP call.
#pragma once
#include "det_post.hpp"

namespace ffp {

// sahi.slicing.get_slice_bboxes: [xmin, ymin, xmax, ymax] per slice, row-major over the grid
std::vector<int32_t> slice_bboxes(int H, int W, int sh, int sw, float oh, float ow);
// the items of get_sliced_prediction: the slice grid, then the full frame when there is more than one slice and it is asked for
std::vector<int32_t> sliced_items(int H, int W, int slice_h, int slice_w, float oh, float ow, int perform_standard_pred);
// n items in ceil(n / max_batch) chunks (max_batch >= 1) whose sizes differ by at most one, the larger ones first: 61 at 16 is 16, 15, 15, 15
std::vector<int> even_chunks(int n, int max_batch);
// an H x W x 3 u8 host frame into dst (grown on demand) on st, not waited for; the caller has set its device
void upload_frame(DevBuf& dst, const uint8_t* frame, int H, int W, hipStream_t st);

// Always: run_merge whatever the counts are, over the grid bound `rows`, so no read back is needed. TwoOrMore: run_merge for more than one tile and
// more than one row (`rows` read back by the caller), else the rows as they are: sahi post-processes a list of two or more and keeps a list of one
enum class MergeRule { Always, TwoOrMore };

struct SlicedTail {      // what follows the per-tile detections; only fetch() waits for the stream
  DevBuf rows, rows_n, prefix, merged, merged_n;      // compact()'s rows, their count, the per-tile offsets [n_tiles + 1]; reserve()'s output rows, count
  MergeWork work;
  int n_tiles = 0, stride = 0;      // of the last compact()
  // d_dets [n_tiles][tile_cap][stride], d_counts [n_tiles] -> rows (tile order, then kept order), rows_n, prefix: launch_compact_rows
  void compact(const float* d_dets, const int* d_counts, int n_tiles, int tile_cap, int stride, hipStream_t st);
  // rows -> the caller's d_out [cap][stride], d_out_src [cap] (may be null), d_out_n[1] (the untruncated count); the clip arguments are run_merge's
  void merge(MergeRule rule, int rows, int type, int metric, double thr, int class_agnostic, float* d_out, int* d_out_src, int* d_out_n, int cap,
             hipStream_t st, int clip_first_row = 0x7fffffff, int clip_w = 0, int clip_h = 0);
  void reserve(int cap, int stride) { merged.ensure(sizeof(float) * (size_t)cap * stride); merged_n.ensure(sizeof(int)); }      // for a host entry
  // merged_n -> *out_n; FFP_ERR_ARG, its message prefixed by `what`, when the count exceeds cap; else that many rows of merged -> out. st: the stream
  // the merge is still running on, waited for after either copy; nullptr where the caller has drained it (blocking copies)
  void fetch(float* out, int cap, int stride, int32_t* out_n, const char* what, hipStream_t st);
};

}  // namespace ffp
