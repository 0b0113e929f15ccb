// coco_eval.hpp — launcher of the COCO bbox evaluation kernels (coco_eval.hip): COCOeval.evaluate + accumulate of pycocotools 2.0.x.
#pragma once
#include "common.hpp"

namespace ffp {

// All pointers are device memory. A unit is an (image, category) pair, U = n_cat * n_img units in pycocotools' evalImgs order
// (category-major, image ids sorted). d_dets [det_off[U]][7] = x, y, w, h, score, area, id in loadRes order per unit; d_gts [gt_off[U]][8]
// = x, y, w, h, area, iscrowd, ignore, id in annotation order per unit. d_cut_off [U + 1]: prefix sums of min(#dets, max_dets[M-1]).
// Parameter tables exactly as the host holds them: iou_thrs [T], rec_thrs [R], area_rng [A][2], max_dets [M] (ascending).
// Outputs precision / scores [T][R][K][A][M] and recall [T][K][A][M]; the match arrays are always produced (they are the
// accumulate stage's input): dt_matches / dt_ignore [A][T][ndc] (unit u at cut_off[u], dets in score order), gt_matches [A][T][ng]
// and gt_ignore [A][ng] (unit u at gt_off[u], GTs in the per-area "ignored last" order). The caller has checked every size.
struct CocoEvalArgs {
  int n_img, n_cat, T, R, A, M;
  const double *dets, *gts;
  const long long *det_off, *gt_off, *cut_off;
  const double *iou_thrs, *rec_thrs, *area_rng;
  const int* max_dets;
  long long nd, ng, ndc;
  double *precision, *recall, *scores;
  double *dt_matches, *gt_matches;
  unsigned char *dt_ignore, *gt_ignore;
};

// bytes of device scratch launch_coco_eval needs for these sizes
size_t coco_eval_scratch_bytes(long long ndc, long long ng, int A, int M, int T);
void launch_coco_eval(const CocoEvalArgs& a, void* d_scratch, hipStream_t st);

}  // namespace ffp
