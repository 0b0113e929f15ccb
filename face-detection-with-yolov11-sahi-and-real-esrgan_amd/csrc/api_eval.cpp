// api_eval.cpp — the C-ABI of libffp.so, part two of four (see api.cpp): merging of host rows and the evaluators. They take a device number, not a handle.
#include <climits>
#include <cmath>

#include "api_util.hpp"
#include "coco_eval.hpp"
#include "det_post.hpp"
#include "eval.hpp"

using namespace ffp;

extern "C" {

int ffp_merge(int device, const float* dets, int n, int stride, int type, int metric, double thr, int class_agnostic, float* out,
              int32_t* out_src_index, int32_t* out_n) {
  FFP_API_BEGIN
  FFP_CHECK(out && out_n && n >= 0 && stride >= 6 && (dets || n == 0), FFP_ERR_ARG, "merge: bad arguments");
  ScopedStream::use_device(device, "merge");
  if (n == 0) { *out_n = 0; return FFP_OK; }      // nothing to merge: no stream
  ScopedStream cx(device, "merge");
  MergeWork w;
  DevBuf rows(sizeof(float) * (size_t)n * stride), dn(sizeof(int)), dout(sizeof(float) * (size_t)n * stride), dsrc(sizeof(int) * (size_t)n),
      doutn(sizeof(int));
  FFP_HIP(hipMemcpyAsync(rows.p, dets, sizeof(float) * (size_t)n * stride, hipMemcpyHostToDevice, cx.st));
  FFP_HIP(hipMemcpyAsync(dn.p, &n, sizeof(int), hipMemcpyHostToDevice, cx.st));
  if (n > 1) run_merge(w, rows.as<float>(), dn.as<int>(), n, stride, type, metric, thr, class_agnostic, dout.as<float>(), dsrc.as<int>(),
                       doutn.as<int>(), n, cx.st);
  else run_merge_passthrough(rows.as<float>(), dn.as<int>(), stride, dout.as<float>(), dsrc.as<int>(), doutn.as<int>(), n, cx.st);
  int k = 0;
  FFP_HIP(hipMemcpyAsync(&k, doutn.p, sizeof(int), hipMemcpyDeviceToHost, cx.st));
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(out, dout.p, sizeof(float) * (size_t)k * stride, hipMemcpyDeviceToHost));
  if (out_src_index) FFP_HIP(hipMemcpy(out_src_index, dsrc.p, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost));
  *out_n = k;
  FFP_API_END
}

// ---- WIDER FACE evaluation -----------------------------------------------------------------------------------
int ffp_eval_wider_pr(int device, const double* preds, const int64_t* pred_off, const double* gts, const int64_t* gt_off, const uint8_t* evaluate,
                      int n_img, double iou_thr, int thresh_num, int64_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0 && thresh_num > 0 && out_counts, FFP_ERR_ARG, "eval_wider_pr: bad arguments");
  ScopedStream cx(device, "eval_wider_pr");
  check_offsets(pred_off, n_img, "prediction");
  check_offsets(gt_off, n_img, "face");
  const int64_t np = pred_off[n_img], ng = gt_off[n_img];
  FFP_CHECK((np == 0 || preds) && (ng == 0 || (gts && evaluate)), FFP_ERR_ARG, "eval_wider_pr: null data");
  DevBuf dp = upload(preds, (size_t)np * 5), dpo = upload(pred_off, (size_t)n_img + 1), dg = upload(gts, (size_t)ng * 4), dgo = upload(gt_off, (size_t)n_img + 1),
         de = upload(evaluate, (size_t)ng), state(sizeof(int) * (size_t)(ng + 2 * np + 1)), counts(sizeof(unsigned long long) * 2 * thresh_num);
  launch_wider_pr(dp.as<double>(), dpo.as<long long>(), dg.as<double>(), dgo.as<long long>(), de.as<unsigned char>(), n_img, iou_thr, thresh_num,
                  state.as<int>(), np, ng, counts.as<unsigned long long>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(out_counts, counts.p, sizeof(int64_t) * 2 * thresh_num, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_eval_dual_match(int device, const double* preds, const int64_t* pred_off, const double* faces, const int64_t* face_off, const uint8_t* valid,
                        int n_img, double iou_thr, int32_t* out_flags) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0, FFP_ERR_ARG, "eval_dual_match: bad arguments");
  ScopedStream cx(device, "eval_dual_match");
  check_offsets(pred_off, n_img, "prediction");
  check_offsets(face_off, n_img, "face");
  const int64_t np = pred_off[n_img], nf = face_off[n_img];
  FFP_CHECK((np == 0 || (preds && out_flags)) && (nf == 0 || (faces && valid)), FFP_ERR_ARG, "eval_dual_match: null data");
  DevBuf dp = upload(preds, (size_t)np * 5), dpo = upload(pred_off, (size_t)n_img + 1), df = upload(faces, (size_t)nf * 4), dfo = upload(face_off, (size_t)n_img + 1),
         dv = upload(valid, (size_t)nf), state(sizeof(int) * (size_t)(nf + 1)), flags(sizeof(int) * (size_t)(np + 1));
  launch_dual_match(dp.as<double>(), dpo.as<long long>(), df.as<double>(), dfo.as<long long>(), dv.as<unsigned char>(), n_img, iou_thr, state.as<int>(), nf,
                    flags.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  if (np) FFP_HIP(hipMemcpy(out_flags, flags.p, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost));
  FFP_API_END
}

// ---- COCO bbox evaluation (pycocotools COCOeval.evaluate + accumulate) ----------------------------------------------------------
int ffp_eval_coco_bbox(int device, int n_img, int n_cat, const double* dets, const int64_t* det_off, const double* gts, const int64_t* gt_off,
                       const double* iou_thrs, int n_iou, const double* rec_thrs, int n_rec, const double* area_rng, int n_area,
                       const int32_t* max_dets, int n_max_dets, double* precision, double* recall, double* scores, double* dt_matches,
                       uint8_t* dt_ignore, double* gt_matches, uint8_t* gt_ignore) {
  FFP_API_BEGIN
  FFP_CHECK(n_img >= 0 && n_cat >= 0 && n_iou > 0 && n_rec > 0 && n_area > 0 && n_max_dets > 0, FFP_ERR_ARG, "eval_coco_bbox: bad sizes");
  FFP_CHECK(iou_thrs && rec_thrs && area_rng && max_dets && precision && recall && scores, FFP_ERR_ARG, "eval_coco_bbox: null parameter or output");
  const long long U = (long long)n_img * n_cat;
  FFP_CHECK(U <= INT_MAX && U * n_area * n_iou <= INT_MAX && (long long)n_cat * n_area * n_max_dets * n_iou <= INT_MAX, FFP_ERR_ARG,
            "eval_coco_bbox: %lld units x %d areas x %d thresholds is too large", U, n_area, n_iou);
  for (int m = 0; m < n_max_dets; ++m)
    FFP_CHECK(max_dets[m] >= 0 && (m == 0 || max_dets[m] >= max_dets[m - 1]), FFP_ERR_ARG, "eval_coco_bbox: maxDets must be ascending and >= 0");
  ScopedStream cx(device, "eval_coco_bbox");
  check_offsets(det_off, (int)U, "detection");
  check_offsets(gt_off, (int)U, "ground-truth");
  const int64_t nd = det_off[U], ng = gt_off[U];
  FFP_CHECK((nd == 0 || dets) && (ng == 0 || gts), FFP_ERR_ARG, "eval_coco_bbox: null data");
  std::vector<int64_t> cut_off((size_t)U + 1, 0);
  const int64_t max_det = max_dets[n_max_dets - 1];
  for (long long u = 0; u < U; ++u) {
    FFP_CHECK(det_off[u + 1] - det_off[u] <= INT_MAX && gt_off[u + 1] - gt_off[u] <= INT_MAX, FFP_ERR_ARG, "eval_coco_bbox: unit %lld is too large", u);
    cut_off[u + 1] = cut_off[u] + std::min<int64_t>(det_off[u + 1] - det_off[u], max_det);
  }
  const int64_t ndc = cut_off[U];
  FFP_CHECK(ndc <= (1LL << 30), FFP_ERR_ARG, "eval_coco_bbox: %lld detections after the maxDets cut is too many", (long long)ndc);
  for (int64_t i = 0; i < nd; ++i)   // loadRes numbers dets from 1: a GT is taken when gtMatches > 0, so every id must be positive
    FFP_CHECK(!std::isnan(dets[i * 7 + 4]) && dets[i * 7 + 6] > 0, FFP_ERR_ARG, "eval_coco_bbox: detection %lld has a NaN score or an id <= 0", (long long)i);
  for (int64_t g = 0; g < ng; ++g)   // _prepare sets ignore = iscrowd: a crowd GT is always ignored (at most one TP per kept GT)
    FFP_CHECK(gts[g * 8 + 5] == 0 || gts[g * 8 + 6] != 0, FFP_ERR_ARG, "eval_coco_bbox: ground truth %lld is a crowd but not ignored", (long long)g);
  const int T = n_iou, R = n_rec, A = n_area, M = n_max_dets, K = n_cat;
  const size_t n_pr = (size_t)T * R * K * A * M, n_rc = (size_t)T * K * A * M;
  DevBuf dd = upload(dets, (size_t)nd * 7), ddo = upload(det_off, (size_t)U + 1), dg = upload(gts, (size_t)ng * 8), dgo = upload(gt_off, (size_t)U + 1),
         dco = upload(cut_off.data(), cut_off.size()), dit = upload(iou_thrs, (size_t)T), drt = upload(rec_thrs, (size_t)R),
         dar = upload(area_rng, (size_t)A * 2), dmd = upload(max_dets, (size_t)M);
  DevBuf dprec(sizeof(double) * std::max<size_t>(n_pr, 1)), drec(sizeof(double) * std::max<size_t>(n_rc, 1)), dsc(sizeof(double) * std::max<size_t>(n_pr, 1)),
         ddtm(sizeof(double) * (size_t)A * T * std::max<int64_t>(ndc, 1)), ddig((size_t)A * T * std::max<int64_t>(ndc, 1)),
         dgtm(sizeof(double) * (size_t)A * T * std::max<int64_t>(ng, 1)), dgig((size_t)A * std::max<int64_t>(ng, 1)),
         scratch(coco_eval_scratch_bytes(ndc, ng, A, M, T));
  CocoEvalArgs a{n_img, n_cat, T, R, A, M, dd.as<double>(), dg.as<double>(), ddo.as<long long>(), dgo.as<long long>(), dco.as<long long>(),
                 dit.as<double>(), drt.as<double>(), dar.as<double>(), dmd.as<int>(), nd, ng, ndc, dprec.as<double>(), drec.as<double>(),
                 dsc.as<double>(), ddtm.as<double>(), dgtm.as<double>(), ddig.as<unsigned char>(), dgig.as<unsigned char>()};
  launch_coco_eval(a, scratch.p, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  if (n_pr) {
    FFP_HIP(hipMemcpy(precision, dprec.p, sizeof(double) * n_pr, hipMemcpyDeviceToHost));
    FFP_HIP(hipMemcpy(scores, dsc.p, sizeof(double) * n_pr, hipMemcpyDeviceToHost));
    FFP_HIP(hipMemcpy(recall, drec.p, sizeof(double) * n_rc, hipMemcpyDeviceToHost));
  }
  if (dt_matches && ndc) FFP_HIP(hipMemcpy(dt_matches, ddtm.p, sizeof(double) * (size_t)A * T * ndc, hipMemcpyDeviceToHost));
  if (dt_ignore && ndc) FFP_HIP(hipMemcpy(dt_ignore, ddig.p, (size_t)A * T * ndc, hipMemcpyDeviceToHost));
  if (gt_matches && ng) FFP_HIP(hipMemcpy(gt_matches, dgtm.p, sizeof(double) * (size_t)A * T * ng, hipMemcpyDeviceToHost));
  if (gt_ignore && ng) FFP_HIP(hipMemcpy(gt_ignore, dgig.p, (size_t)A * ng, hipMemcpyDeviceToHost));
  FFP_API_END
}

}  // extern "C"
