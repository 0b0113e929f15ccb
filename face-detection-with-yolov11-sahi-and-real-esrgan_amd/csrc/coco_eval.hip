// coco_eval.hip — COCOeval (iouType 'bbox') evaluate + accumulate of pycocotools 2.0.x on the device, bit-identical to it.
// Four stages, all float64 and compiled without fp contraction (like eval.hip):
//   1. per unit (image, category), one workgroup: dets stably ranked by -score (mergesort order) and cut to maxDets[-1]; per area
//      range the GTs stably partitioned "ignored last" (evaluateImg's two argsorts). The cut dets also become the keys of stage 3.
//   2. per (unit, area, IoU threshold), one wave: evaluateImg's greedy match. The dets go in order; the lanes hold the GTs. The scan of
//      pycocotools picks, among the eligible GTs with IoU >= thr, the LAST one with the largest IoU, non-ignored GTs before ignored ones.
//   3. one bitonic sort of every cut det by (category, -score, image order, rank): accumulate's per-category mergesort of the
//      concatenated dtScores. A stable sort of a subsequence is that subsequence of the stable sort, so this one order serves every
//      area range and every maxDet (filter by rank within the image).
//   4. per (category, area, maxDet, IoU threshold), one workgroup: integer cumulative TP / FP counts, then precision / recall / scores.
//      Between two true positives precision can only fall (tp fixed, fp growing), so the envelope at a recall threshold is the suffix
//      max over the true positives from the c-th on, where c is the first count with c / npig >= recThr — searchsorted on rc.
#include <algorithm>
#include <climits>

#include "coco_eval.hpp"

namespace ffp {

namespace {

constexpr double kSpacing1 = 2.220446049250313e-16;      // np.spacing(1)

struct SortElem {                                        // one cut det in stage 3
  double score;
  unsigned cat, unit, rank, pad;
};

__device__ __forceinline__ bool elem_less(const SortElem& x, const SortElem& y) {
  if (x.cat != y.cat) return x.cat < y.cat;
  if (x.score != y.score) return x.score > y.score;     // -score ascending; +0 and -0 compare equal as in numpy
  if (x.unit != y.unit) return x.unit < y.unit;
  return x.rank < y.rank;
}

__device__ __forceinline__ bool gt_ignored(const double* Q, double lo, double hi) {
  return Q[6] != 0 || Q[4] < lo || Q[4] > hi;          // evaluateImg: g['ignore'] or area outside [lo, hi]
}

__device__ __forceinline__ long long block_sum_ll(long long v, long long* lds) {     // 256 threads; lds >= 4
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// exclusive prefix sum over a 256-thread block; *total = block sum
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) lds[w] = x;
  __syncthreads();
  int pre = 0;
  for (int i = 0; i < w; ++i) pre += lds[i];
  *total = lds[0] + lds[1] + lds[2] + lds[3];
  return pre + x - v;
}

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) coco_unit_sort_kernel(CocoEvalArgs a, int* dsort, int* gsort, SortElem* elems) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long d0 = a.det_off[u], g0 = a.gt_off[u], c0 = a.cut_off[u];
  const int D = (int)(a.det_off[u + 1] - d0), G = (int)(a.gt_off[u + 1] - g0), cut = (int)(a.cut_off[u + 1] - c0);
  const double* P = a.dets + d0 * 7;
  for (int i = tid; i < D; i += 256) {
    const double s = P[i * 7 + 4];
    int r = 0;
    for (int j = 0; j < D; ++j) {
      const double sj = P[j * 7 + 4];
      r += (sj > s || (sj == s && j < i)) ? 1 : 0;
    }
    if (r < cut) {
      dsort[c0 + r] = i;
      elems[c0 + r] = SortElem{s, (unsigned)(u / a.n_img), (unsigned)u, (unsigned)r, 0u};
    }
  }
  const double* Q = a.gts + g0 * 8;
  for (int ar = 0; ar < a.A; ++ar) {
    const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
    for (int g = tid; g < G; g += 256) {
      const bool ig = gt_ignored(Q + g * 8, lo, hi);
      int n_kept = 0, before = 0;
      for (int j = 0; j < G; ++j) {
        const bool igj = gt_ignored(Q + j * 8, lo, hi);
        n_kept += igj ? 0 : 1;
        before += (j < g && igj == ig) ? 1 : 0;
      }
      const long long pos = (long long)ar * a.ng + g0 + (ig ? n_kept : 0) + before;
      gsort[pos] = g;
      a.gt_ignore[pos] = ig ? 1 : 0;
    }
  }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_best(double& v, int& m) {        // largest IoU; ties to the later GT
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int om = __shfl_xor(m, o);
    if (ov > v || (ov == v && om > m)) { v = ov; m = om; }
  }
}

__global__ void __launch_bounds__(64) coco_match_kernel(CocoEvalArgs a, const int* __restrict__ dsort, const int* __restrict__ gsort) {
  const long long blk = blockIdx.x;
  const int t = (int)(blk % a.T), ar = (int)((blk / a.T) % a.A);
  const int u = (int)(blk / ((long long)a.T * a.A));
  const int lane = threadIdx.x;
  const long long d0 = a.det_off[u], g0 = a.gt_off[u], c0 = a.cut_off[u];
  const int G = (int)(a.gt_off[u + 1] - g0), D = (int)(a.cut_off[u + 1] - c0);
  if (D == 0) return;
  const double lim = 1 - 1e-10, t0 = a.iou_thrs[t];
  const double thr = lim < t0 ? lim : t0;                           // min([t, 1 - 1e-10])
  const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
  const int* gs = gsort + (long long)ar * a.ng + g0;
  const unsigned char* gig = a.gt_ignore + (long long)ar * a.ng + g0;
  double* gtm = a.gt_matches + ((long long)ar * a.T + t) * a.ng + g0;  // entry p is only ever touched by lane p % 64
  double* dtm = a.dt_matches + ((long long)ar * a.T + t) * a.ndc + c0;
  unsigned char* dig = a.dt_ignore + ((long long)ar * a.T + t) * a.ndc + c0;
  const double* Gt = a.gts + g0 * 8;
  for (int d = 0; d < D; ++d) {
    const double* P = a.dets + (d0 + dsort[c0 + d]) * 7;
    const double dx = P[0], dy = P[1], dw = P[2], dh = P[3];
    const double da = dw * dh;
    double b0 = -1.0, b1 = -1.0;                                     // best non-ignored / ignored candidate
    int m0 = -1, m1 = -1;
    for (int p = lane; p < G; p += 64) {
      const double* Q = Gt + (long long)gs[p] * 8;
      const bool crowd = Q[5] != 0;
      if (gtm[p] > 0 && !crowd) continue;
      // maskApi.c bbIou
      double iou = 0.0;
      const double w = fmin(dw + dx, Q[2] + Q[0]) - fmax(dx, Q[0]);
      if (w > 0) {
        const double h = fmin(dh + dy, Q[3] + Q[1]) - fmax(dy, Q[1]);
        if (h > 0) {
          const double i = w * h;
          const double un = crowd ? da : da + Q[2] * Q[3] - i;
          iou = i / un;
        }
      }
      if (iou >= thr) {
        if (gig[p] == 0) { if (iou >= b0) { b0 = iou; m0 = p; } }
        else if (iou >= b1) { b1 = iou; m1 = p; }
      }
    }
    wave_best(b0, m0);
    wave_best(b1, m1);
    const int m = m0 >= 0 ? m0 : m1;
    const bool out = P[5] < lo || P[5] > hi;
    if (m >= 0) {
      const double gid = Gt[(long long)gs[m] * 8 + 7];
      if (lane == (m & 63)) gtm[m] = P[6];
      if (lane == 0) {
        dtm[d] = gid;
        dig[d] = (m0 < 0 || (gid == 0 && out)) ? 1 : 0;
      }
    } else if (lane == 0) {
      dtm[d] = 0.0;
      dig[d] = out ? 1 : 0;
    }
  }
}

// ---- stage 3 ------------------------------------------------------------------------------------------------------------------
constexpr int kLocal = 1024;                               // elements per workgroup of the in-LDS steps

__global__ void coco_sort_pad_kernel(SortElem* e, long long n, long long N) {
  const long long i = n + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) e[i] = SortElem{0.0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u};
}

__device__ __forceinline__ void cmp_swap(SortElem& x, SortElem& y, bool asc) {
  if (elem_less(y, x) == asc) { const SortElem t = x; x = y; y = t; }
}

// k_only = 0: the whole bitonic network up to k = kLocal; otherwise steps j = kLocal/2 .. 1 of stage k_only
__global__ void __launch_bounds__(kLocal / 2) coco_sort_local_kernel(SortElem* e, long long k_only) {
  __shared__ SortElem s[kLocal];
  const long long base = (long long)blockIdx.x * kLocal;
  const int tid = threadIdx.x;
  s[tid] = e[base + tid];
  s[tid + kLocal / 2] = e[base + tid + kLocal / 2];
  __syncthreads();
  const long long k0 = k_only ? k_only : 2, k1 = k_only ? k_only : kLocal;
  for (long long k = k0; k <= k1; k <<= 1) {
    for (int j = (int)std::min<long long>(k >> 1, kLocal / 2); j > 0; j >>= 1) {
      const int lo = 2 * tid - (tid & (j - 1)), hi = lo + j;
      cmp_swap(s[lo], s[hi], ((base + lo) & k) == 0);
      __syncthreads();
    }
  }
  e[base + tid] = s[tid];
  e[base + tid + kLocal / 2] = s[tid + kLocal / 2];
}

__global__ void __launch_bounds__(256) coco_sort_global_kernel(SortElem* e, long long k, long long j, long long half) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half) return;
  const long long lo = 2 * i - (i & (j - 1)), hi = lo + j;
  SortElem x = e[lo], y = e[hi];
  const bool asc = (lo & k) == 0;
  if (elem_less(y, x) == asc) { e[lo] = y; e[hi] = x; }
}

// ---- stage 4 ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) coco_accumulate_kernel(CocoEvalArgs a, const SortElem* __restrict__ sorted, double* env_pr, double* env_sc) {
  __shared__ long long red[4];
  __shared__ int scan[4];
  __shared__ double first_score, carry_s;
  __shared__ double suf[256];
  __shared__ int first_fail;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int t = (int)(b % a.T), m = (int)((b / a.T) % a.M), ar = (int)((b / ((long long)a.T * a.M)) % a.A);
  const int k = (int)(b / ((long long)a.T * a.M * a.A));
  const int K = a.n_cat, T = a.T, R = a.R, A = a.A, M = a.M;
  const long long u0 = (long long)k * a.n_img, u1 = u0 + a.n_img;
  const long long gb = a.gt_off[u0], ge = a.gt_off[u1], cb = a.cut_off[u0], ce = a.cut_off[u1];
  auto pidx = [&](int r) { return ((((long long)t * R + r) * K + k) * A + ar) * M + m; };
  const long long ridx = (((long long)t * K + k) * A + ar) * M + m;

  long long cnt = 0;
  for (long long g = gb + tid; g < ge; g += 256) cnt += a.gt_ignore[(long long)ar * a.ng + g] == 0 ? 1 : 0;
  const long long npig = block_sum_ll(cnt, red);
  if (npig == 0) {                                       // accumulate: `if npig == 0: continue` (also: no unit of this category)
    for (int r = tid; r < R; r += 256) { a.precision[pidx(r)] = -1.0; a.scores[pidx(r)] = -1.0; }
    if (tid == 0) a.recall[ridx] = -1.0;
    return;
  }
  const unsigned max_det = (unsigned)a.max_dets[m];
  const double* dtm = a.dt_matches + ((long long)ar * T + t) * a.ndc;
  const unsigned char* dig = a.dt_ignore + ((long long)ar * T + t) * a.ndc;
  double* epr = env_pr + (((long long)ar * M + m) * T + t) * a.ng + gb;
  double* esc = env_sc + (((long long)ar * M + m) * T + t) * a.ng + gb;
  const long long cap = ge - gb;                         // >= npig >= #TP (the host guarantees one match per GT)
  if (tid == 0) first_score = 0.0;
  long long nd = 0, tp = 0, fp = 0;
  for (long long base = cb; base < ce; base += 256) {
    const long long e = base + tid;
    int inc = 0, tpf = 0, fpf = 0;
    SortElem el{};
    if (e < ce) {
      el = sorted[e];
      if (el.rank < max_det) {
        inc = 1;
        const long long pos = a.cut_off[el.unit] + el.rank;
        const bool mt = dtm[pos] != 0, ig = dig[pos] != 0;
        tpf = (mt && !ig) ? 1 : 0;
        fpf = (!mt && !ig) ? 1 : 0;
      }
    }
    int ti, fi, ii;
    const int inc_ex = block_excl_scan(inc, scan, &ii);
    const int tp_ex = block_excl_scan(tpf, scan, &ti);
    const int fp_ex = block_excl_scan(fpf, scan, &fi);
    if (inc && nd + inc_ex == 0) first_score = el.score;
    if (tpf) {
      const long long c = tp + tp_ex + 1;              // tp_sum at this det; fp_sum equals the FPs before it
      const double fc = (double)(fp + fp_ex), tc = (double)c;
      if (c - 1 < cap) { epr[c - 1] = tc / ((fc + tc) + kSpacing1); esc[c - 1] = el.score; }
    }
    nd += ii; tp += ti; fp += fi;
  }
  __syncthreads();
  const long long ntp = std::min(tp, cap);
  if (tid == 0) a.recall[ridx] = nd ? (double)tp / (double)npig : 0.0;
  // precision envelope: suffix max over the true positives, last block first
  if (tid == 0) carry_s = -1.0;
  __syncthreads();
  for (long long end = ntp; end > 0; end -= 256) {
    const long long i = end - 256 + tid;
    double v = i >= 0 ? epr[i] : -1.0;
    suf[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const double w = tid + o < 256 ? suf[tid + o] : -1.0;
      __syncthreads();
      v = fmax(v, w);
      suf[tid] = v;
      __syncthreads();
    }
    v = fmax(v, carry_s);
    if (i >= 0) epr[i] = v;
    __syncthreads();
    if (tid == 0) carry_s = fmax(carry_s, suf[0]);
    __syncthreads();
  }
  // searchsorted(rc, recThrs, 'left'); the first threshold past the last det ends the loop (pycocotools' try / except)
  if (tid == 0) first_fail = R;
  __syncthreads();
  auto first_count = [&](double x) {                     // smallest c in [0, tp] with c / npig >= x; tp + 1 when there is none
    long long lo = 0, hi = ntp + 1;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((double)mid / (double)npig >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  for (int r = tid; r < R; r += 256) {
    const long long c = first_count(a.rec_thrs[r]);
    if (c > ntp || (c == 0 && nd == 0)) atomicMin(&first_fail, r);
  }
  __syncthreads();
  for (int r = tid; r < R; r += 256) {
    double q = 0.0, ss = 0.0;
    if (r < first_fail) {
      const long long c = first_count(a.rec_thrs[r]);
      if (c == 0) { q = ntp ? epr[0] : 0.0; ss = first_score; }
      else { q = epr[c - 1]; ss = esc[c - 1]; }
    }
    a.precision[pidx(r)] = q;
    a.scores[pidx(r)] = ss;
  }
}

constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

long long sort_len(long long ndc) {
  long long N = kLocal;
  while (N < ndc) N <<= 1;
  return N;
}

}  // namespace

size_t coco_eval_scratch_bytes(long long ndc, long long ng, int A, int M, int T) {
  return align256(sizeof(int) * (size_t)std::max(ndc, 1LL)) + align256(sizeof(int) * (size_t)A * (size_t)std::max(ng, 1LL)) +
         align256(sizeof(SortElem) * (size_t)sort_len(ndc)) + 2 * align256(sizeof(double) * (size_t)A * M * T * (size_t)std::max(ng, 1LL));
}

void launch_coco_eval(const CocoEvalArgs& a, void* d_scratch, hipStream_t st) {
  const long long U = (long long)a.n_img * a.n_cat;
  const long long N = sort_len(a.ndc);
  char* s = static_cast<char*>(d_scratch);
  int* dsort = reinterpret_cast<int*>(s);
  s += align256(sizeof(int) * (size_t)std::max(a.ndc, 1LL));
  int* gsort = reinterpret_cast<int*>(s);
  s += align256(sizeof(int) * (size_t)a.A * (size_t)std::max(a.ng, 1LL));
  SortElem* elems = reinterpret_cast<SortElem*>(s);
  s += align256(sizeof(SortElem) * (size_t)N);
  const size_t env_n = (size_t)a.A * a.M * a.T * (size_t)std::max(a.ng, 1LL);
  double* env_pr = reinterpret_cast<double*>(s);
  double* env_sc = env_pr + align256(sizeof(double) * env_n) / sizeof(double);
  if (a.ndc) {
    FFP_HIP(hipMemsetAsync(a.dt_matches, 0, sizeof(double) * (size_t)a.A * a.T * a.ndc, st));
    FFP_HIP(hipMemsetAsync(a.dt_ignore, 0, (size_t)a.A * a.T * a.ndc, st));
  }
  if (a.ng) FFP_HIP(hipMemsetAsync(a.gt_matches, 0, sizeof(double) * (size_t)a.A * a.T * a.ng, st));
  if (U > 0) {
    hipLaunchKernelGGL(coco_unit_sort_kernel, dim3((unsigned)U), dim3(256), 0, st, a, dsort, gsort, elems);
    FFP_HIP(hipGetLastError());
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)(U * a.A * a.T)), dim3(64), 0, st, a, (const int*)dsort, (const int*)gsort);
    FFP_HIP(hipGetLastError());
  }
  if (a.ndc) {
    if (N > a.ndc) {
      hipLaunchKernelGGL(coco_sort_pad_kernel, dim3((unsigned)((N - a.ndc + 255) / 256)), dim3(256), 0, st, elems, a.ndc, N);
      FFP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(coco_sort_local_kernel, dim3((unsigned)(N / kLocal)), dim3(kLocal / 2), 0, st, elems, 0LL);
    FFP_HIP(hipGetLastError());
    for (long long k = 2 * kLocal; k <= N; k <<= 1) {
      for (long long j = k >> 1; j >= kLocal; j >>= 1) {
        hipLaunchKernelGGL(coco_sort_global_kernel, dim3((unsigned)(N / 2 / 256)), dim3(256), 0, st, elems, k, j, N / 2);
        FFP_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(coco_sort_local_kernel, dim3((unsigned)(N / kLocal)), dim3(kLocal / 2), 0, st, elems, k);
      FFP_HIP(hipGetLastError());
    }
  }
  const long long nacc = (long long)a.n_cat * a.A * a.M * a.T;
  if (nacc > 0) {
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)nacc), dim3(256), 0, st, a, (const SortElem*)elems, env_pr, env_sc);
    FFP_HIP(hipGetLastError());
  }
}

}  // namespace ffp
