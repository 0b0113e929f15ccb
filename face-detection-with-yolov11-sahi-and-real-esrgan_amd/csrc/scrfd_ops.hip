// scrfd_ops.hip — the SCRFD-specific device operators: InsightFace's pre-processing, the ResNet-v1e pools, and the decode / NMS of
// RetinaFace.detect (insightface/model_zoo/retinaface.py). Vector memory operations and ordinary global atomics only.
#include <algorithm>
#include <climits>

#include "letterbox.hpp"
#include "scrfd.hpp"

namespace ffp {

namespace {
unsigned blocks(long long n, int b) { return (unsigned)((n + b - 1) / b); }
}  // namespace

// RetinaFace.detect: cv2.resize to (new_w, new_h) INTER_LINEAR, the picture at the top-left of a zero (u8) canvas, then
// cv2.dnn.blobFromImage(img, 1/128, size, (127.5, 127.5, 127.5), swapRB=True): v -> (v - 127.5) / 128 (exact in fp32).
// Output NHWC fp32 with 4 channels (the 4th zero). grid (pixel blocks, image)
__global__ void scrfd_preproc_kernel(const uint8_t* __restrict__ frame, int W, int flip, const LetterboxImg* __restrict__ imgs,
                                     const int4* __restrict__ tab, float* __restrict__ out) {
  const int im = blockIdx.y;
  const int4 t = tab[im];
  const int lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= t.y * t.z) return;
  const int y = lp / t.z, x = lp - y * t.z;
  const LetterboxImg L = imgs[im];
  int px[3];
  letterbox_sample(frame, W, L, y, x, px, 0);
  const float v0 = ((float)px[flip ? 2 : 0] - 127.5f) * 0.0078125f;
  const float v1 = ((float)px[1] - 127.5f) * 0.0078125f;
  const float v2 = ((float)px[flip ? 0 : 2] - 127.5f) * 0.0078125f;
  *reinterpret_cast<float4*>(out + ((size_t)t.x + lp) * 4) = make_float4(v0, v1, v2, 0.f);
}

void launch_scrfd_preproc(const uint8_t* d_frame, int W, int flip, const LetterboxImg* d_imgs, const TView& out, hipStream_t st) {
  FFP_CHECK(out.dt == F32 && out.cs == 4 && out.coff == 0, FFP_ERR_ARG, "scrfd preproc: output must be a 4-channel fp32 buffer");
  const Level& l = *out.lvl;
  const dim3 grid(blocks((long long)l.h[0] * l.w[0], 256), l.n);
  hipLaunchKernelGGL(scrfd_preproc_kernel, grid, dim3(256), 0, st, d_frame, W, flip, d_imgs, l.d_tab.as<int4>(), (float*)out.ptr);
  FFP_HIP(hipGetLastError());
}

// MaxPool 3x3 / stride 2 / pad 1 (padding never wins, as ONNX pads with -inf) and AveragePool k x k / stride k with
// count_include_pad = 0 (ceil_mode windows clipped to the map). One thread per (output pixel, channel). grid (blocks, image)
__global__ void scrfd_pool_kernel(const float* __restrict__ in, int in_cs, int in_coff, const int4* __restrict__ in_tab, float* __restrict__ out,
                                  int out_cs, int out_coff, const int4* __restrict__ out_tab, int C, int maxpool, int k) {
  const int im = blockIdx.y;
  const int4 ti = in_tab[im], to = out_tab[im];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)to.y * to.z * C) return;
  const int c = (int)(e % C);
  const int p = (int)(e / C);
  const int oy = p / to.z, ox = p - oy * to.z;
  float acc = maxpool ? -INFINITY : 0.f;
  int cnt = 0;
  const int y0 = maxpool ? 2 * oy - 1 : k * oy, x0 = maxpool ? 2 * ox - 1 : k * ox, kk = maxpool ? 3 : k;
  for (int ky = 0; ky < kk; ++ky) {
    const int iy = y0 + ky;
    if (iy < 0 || iy >= ti.y) continue;
    for (int kx = 0; kx < kk; ++kx) {
      const int ix = x0 + kx;
      if (ix < 0 || ix >= ti.z) continue;
      const float v = in[((size_t)ti.x + (size_t)iy * ti.z + ix) * in_cs + in_coff + c];
      if (maxpool) acc = fmaxf(acc, v);
      else acc += v;
      ++cnt;
    }
  }
  if (!maxpool) acc = acc / (float)max(cnt, 1);
  out[((size_t)to.x + p) * out_cs + out_coff + c] = acc;
}

void launch_scrfd_pool(const TView& in, const TView& out, int maxpool, int k, hipStream_t st) {
  FFP_CHECK(in.dt == F32 && out.dt == F32 && in.C == out.C && in.lvl->n == out.lvl->n, FFP_ERR_ARG, "scrfd pool: view mismatch");
  const Level& lo = *out.lvl;
  long long px = 0;                                  // a ragged batch: the grid covers the largest output image
  for (int i = 0; i < lo.n; ++i) px = std::max(px, (long long)lo.h[i] * lo.w[i]);
  const dim3 grid(blocks(px * in.C, 256), lo.n);
  hipLaunchKernelGGL(scrfd_pool_kernel, grid, dim3(256), 0, st, (const float*)in.ptr, in.cs, in.coff, in.lvl->d_tab.as<int4>(), (float*)out.ptr, out.cs,
                     out.coff, lo.d_tab.as<int4>(), in.C, maxpool, k);
  FFP_HIP(hipGetLastError());
}

__device__ __forceinline__ float scrfd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// per (image, anchor): the anchor's score (sigmoid of the score conv), and for scores >= thresh its box / keypoints, appended to
// the image's candidate list. Anchors are numbered level by level, pixel by pixel, anchor by anchor (InsightFace's stacking order).
__global__ void scrfd_decode_kernel(ScrfdHeads h, float thresh, ScrfdCand* __restrict__ cand, int* __restrict__ counts, float* __restrict__ raw_scores) {
  const int im = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= h.per_img) return;
  int l = 0;
  while (l < 2 && j >= h.a_off[l + 1]) ++l;
  const int q = j - h.a_off[l];
  const int p = q / h.A, a = q - p * h.A;
  const int4 t = h.tab[l][im];
  const int y = p / t.z, x = p - y * t.z;
  const size_t rec = (size_t)t.x + p;
  const float s = scrfd_sigmoid(h.score[l][rec * h.cs[0][l] + h.coff[0][l] + a]);
  if (raw_scores) raw_scores[(size_t)im * h.per_img + j] = s;
  if (!cand || !(s >= thresh)) return;
  const float stride = (float)h.stride[l];
  const float cx = (float)x * stride, cy = (float)y * stride;
  const float ds = h.det_scale[im];
  const float* bb = h.bbox[l] + rec * h.cs[1][l] + h.coff[1][l] + 4 * a;
  ScrfdCand c;
  c.b[0] = (cx - bb[0] * stride) / ds;
  c.b[1] = (cy - bb[1] * stride) / ds;
  c.b[2] = (cx + bb[2] * stride) / ds;
  c.b[3] = (cy + bb[3] * stride) / ds;
  c.score = s;
  c.idx = j;
  if (h.kps[l]) {
    const float* kp = h.kps[l] + rec * h.cs[2][l] + h.coff[2][l] + 10 * a;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      c.k[2 * i] = (cx + kp[2 * i] * stride) / ds;
      c.k[2 * i + 1] = (cy + kp[2 * i + 1] * stride) / ds;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 10; ++i) c.k[i] = 0.f;
  }
  const int slot = atomicAdd(&counts[im], 1);
  cand[(size_t)im * h.per_img + slot] = c;
}

void launch_scrfd_decode(const ScrfdHeads& h, int n_img, float thresh, ScrfdCand* cand, int* counts, float* raw_scores, hipStream_t st) {
  if (counts) FFP_HIP(hipMemsetAsync(counts, 0, sizeof(int) * n_img, st));
  hipLaunchKernelGGL(scrfd_decode_kernel, dim3(blocks(h.per_img, 256), n_img), dim3(256), 0, st, h, thresh, cand, counts, raw_scores);
  FFP_HIP(hipGetLastError());
}

// InsightFace's RetinaFace.nms on one image per workgroup: candidates in descending score order (ties: ascending anchor number),
// a candidate is kept when its overlap with every kept one is <= thresh; areas and overlaps with the "+1" pixel convention.
// Every step in fp32 in numpy's order (-ffp-contract=off: no fused multiply-adds).
__global__ void __launch_bounds__(256) scrfd_nms_kernel(const ScrfdCand* __restrict__ cand, const int* __restrict__ counts, int per_img,
                                                        int* __restrict__ order, int* __restrict__ supp, float thresh, float* __restrict__ out,
                                                        int cap, int* __restrict__ out_counts) {
  const int im = blockIdx.x;
  const int n = counts[im];
  const ScrfdCand* c = cand + (size_t)im * per_img;
  int* ord = order + (size_t)im * per_img;
  int* sup = supp + (size_t)im * per_img;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float si = c[i].score;
    const int ii = c[i].idx;
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = c[j].score;
      r += (sj > si || (sj == si && c[j].idx < ii)) ? 1 : 0;
    }
    ord[r] = i;
    sup[r] = 0;
  }
  __shared__ int kept;
  if (threadIdx.x == 0) kept = 0;
  __syncthreads();
  for (int r = 0; r < n; ++r) {
    const bool dead = sup[r] != 0;
    __syncthreads();                    // every thread has read sup[r] before anyone writes this round
    if (dead) continue;
    const ScrfdCand ci = c[ord[r]];
    const float area_i = (ci.b[2] - ci.b[0] + 1.0f) * (ci.b[3] - ci.b[1] + 1.0f);
    if (threadIdx.x == 0) {
      if (kept < cap) {
        float* o = out + ((size_t)im * cap + kept) * FFP_DET_STRIDE(5);
        o[0] = ci.b[0]; o[1] = ci.b[1]; o[2] = ci.b[2]; o[3] = ci.b[3]; o[4] = ci.score; o[5] = 0.f;
        for (int k = 0; k < 5; ++k) { o[6 + 3 * k] = ci.k[2 * k]; o[7 + 3 * k] = ci.k[2 * k + 1]; o[8 + 3 * k] = 1.0f; }
      }
      ++kept;
    }
    for (int j = r + 1 + threadIdx.x; j < n; j += blockDim.x) {
      if (sup[j]) continue;
      const ScrfdCand cj = c[ord[j]];
      const float area_j = (cj.b[2] - cj.b[0] + 1.0f) * (cj.b[3] - cj.b[1] + 1.0f);
      const float xx1 = fmaxf(ci.b[0], cj.b[0]), yy1 = fmaxf(ci.b[1], cj.b[1]);
      const float xx2 = fminf(ci.b[2], cj.b[2]), yy2 = fminf(ci.b[3], cj.b[3]);
      const float w = fmaxf(0.0f, xx2 - xx1 + 1.0f), hh = fmaxf(0.0f, yy2 - yy1 + 1.0f);
      const float inter = w * hh;
      const float ovr = inter / (area_i + area_j - inter);
      if (!(ovr <= thresh)) sup[j] = 1;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out_counts[im] = kept;
}

void launch_scrfd_nms(const ScrfdCand* cand, const int* counts, int n_img, int per_img, int* order, int* supp, float thresh, float* out, int cap,
                      int* out_counts, hipStream_t st) {
  hipLaunchKernelGGL(scrfd_nms_kernel, dim3(n_img), dim3(256), 0, st, cand, counts, per_img, order, supp, thresh, out, cap, out_counts);
  FFP_HIP(hipGetLastError());
}

// numpy's float32 -> int conversion of face.bbox.astype(int): toward zero. A NaN is negative there (the smallest integer), and a value
// outside int32 is pinned to its end of the range: the clip that follows brings both back into the frame or flags them.
__device__ __forceinline__ int scrfd_trunc(float v) {
  if (!(v == v)) return INT_MIN;
  return (int)fminf(fmaxf(v, -2147483648.0f), 2147483520.0f);
}

constexpr int SCRFD_ROW = FFP_DET_STRIDE(5);

// utils/insightface_wrapper.py's conversion, sahi's ObjectAnnotation / BoundingBox and get_shifted_object_prediction on the rows of one
// tile per workgroup, in place: rows with score < conf skipped, the box int-truncated and clipped (x1, y1 >= 0, x2 <= full_w,
// y2 <= full_h: the crop-local box against the FULL frame), a box with x2 < 0 or y2 < 0 reported through *err (the smallest
// tile * cap + row wins; the reference raises there) and left out, then the tile origin added to the box (integers) and to the
// keypoints (floats). Survivors keep their order and move to the front; the rows they vacate are zeroed; counts[tile] is rewritten.
// Rounds of 256 rows: every row of a round sits in registers before the first survivor of that round is stored, and a survivor never
// moves past its own place, so compacting in place reads nothing that was already overwritten.
__global__ void __launch_bounds__(256) scrfd_sahi_rows_kernel(float* __restrict__ dets, int* __restrict__ counts, const int4* __restrict__ tiles,
                                                              int cap, float conf, int full_h, int full_w, unsigned* __restrict__ err) {
  const int tile = blockIdx.x;
  const int n = min(counts[tile], cap);
  float* base = dets + (size_t)tile * cap * SCRFD_ROW;
  const int4 t = tiles[tile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int wave_kept[4];
  __syncthreads();                      // counts[tile] is read by every thread before thread 0 rewrites it
  int kept = 0;
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int r = r0 + (int)threadIdx.x;
    float row[SCRFD_ROW];
    bool keep = false;
    if (r < n) {
      const float* src = base + (size_t)r * SCRFD_ROW;
#pragma unroll
      for (int i = 0; i < SCRFD_ROW; ++i) row[i] = src[i];
      if (!(row[4] < conf)) {
        const int x1 = max(scrfd_trunc(row[0]), 0), y1 = max(scrfd_trunc(row[1]), 0);
        const int x2 = min(scrfd_trunc(row[2]), full_w), y2 = min(scrfd_trunc(row[3]), full_h);
        if (x2 < 0 || y2 < 0) {
          atomicMin(err, (unsigned)(tile * cap + r));
        } else {
          keep = true;
          row[0] = (float)((long long)x1 + t.x); row[1] = (float)((long long)y1 + t.y);
          row[2] = (float)(x2 + t.x); row[3] = (float)(y2 + t.y);
#pragma unroll
          for (int k = 0; k < 5; ++k) { row[6 + 3 * k] += (float)t.x; row[7 + 3 * k] += (float)t.y; }
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_kept[wave] = __popcll(m);
    __syncthreads();
    int at = kept + __popcll(m & ((1ull << lane) - 1ull)), round = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) at += wave_kept[w];
      round += wave_kept[w];
    }
    if (keep) {
      float* dst = base + (size_t)at * SCRFD_ROW;
#pragma unroll
      for (int i = 0; i < SCRFD_ROW; ++i) dst[i] = row[i];
    }
    kept += round;
    __syncthreads();                    // wave_kept is rewritten by the next round
  }
  for (int e = kept * SCRFD_ROW + (int)threadIdx.x; e < n * SCRFD_ROW; e += 256) base[e] = 0.f;
  if (threadIdx.x == 0) counts[tile] = kept;
}

void launch_scrfd_sahi_rows(float* dets, int* counts, const int4* tiles_xyxy, int n_tiles, int cap, float conf, int full_h, int full_w, unsigned* err,
                            hipStream_t st) {
  FFP_CHECK(n_tiles >= 1 && cap >= 1 && (long long)n_tiles * cap < (1ll << 31), FFP_ERR_ARG, "scrfd sahi rows: %d tiles of %d rows", n_tiles, cap);
  FFP_HIP(hipMemsetAsync(err, 0xff, sizeof(unsigned), st));      // SCRFD_NO_BAD_ROW
  hipLaunchKernelGGL(scrfd_sahi_rows_kernel, dim3(n_tiles), dim3(256), 0, st, dets, counts, tiles_xyxy, cap, conf, full_h, full_w, err);
  FFP_HIP(hipGetLastError());
}

}  // namespace ffp
