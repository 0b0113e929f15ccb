// iqa.hip — NIQE block features on the device, the score on the host (iqa.hpp).
//
//   luma        one thread per crop pixel: fp32, the operation order of the text, no contraction, round-half-even
//   half rows / half cols   MATLAB imresize(y / 255, 0.5) bicubic with antialiasing: ten position-independent taps per axis,
//               symmetric reflection, the vertical pass first, * 255 at the end
//   block       one workgroup per 96x96 (scale 1) or 48x48 (scale 2) block: the block with its 3-pixel replicate halo in LDS,
//               the MSCN map of the block (window differences summed per weight class) in LDS, then the 26 running sums of the block and its four rolled products
//   finalize    one thread per (block, scale, map): the AGGD fit of those sums in float64 against host-built Gamma tables
//
// Every sum is taken in a fixed order that depends on the block alone, so an image's features do not depend on its batch mates.
#include <algorithm>
#include <cmath>

#include "iqa.hpp"

namespace ffp {

namespace {

constexpr int kThreads = 256;
constexpr int kSums = 26;           // 5 maps x {sum x^2 | x<0, sum x^2 | x>0, sum |x|, #x<0, #x>0}, sum sigma
constexpr int kHalo = 3;
constexpr int kClasses = 10;        // distinct weights of the 7x7 Gaussian

// class of tap (dy, dx): hi * (hi + 1) / 2 + lo over (lo, hi) = sorted(|dy - 3|, |dx - 3|)
__host__ __device__ constexpr int tap_class(int dy, int dx) {
  const int a = dy < 3 ? 3 - dy : dy - 3, b = dx < 3 ? 3 - dx : dx - 3;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return hi * (hi + 1) / 2 + lo;
}

struct IqaImg {
  const void* src;
  int h, w, c;                      // the caller's image
  int ch, cw;                       // the crop: multiples of 96
  int bcols;                        // blocks per row
  long long y1, tmp, y2;            // element offsets of the crop's luma, the half-height intermediate, the half-size image
  long long blk0;                   // first block of the image
};

__device__ __forceinline__ int reflect(int j, int n) { return j < 0 ? -j - 1 : (j >= n ? 2 * n - 1 - j : j); }

__global__ void __launch_bounds__(kThreads) iqa_luma_kernel(const IqaImg* __restrict__ tab, int layout, int as_rgb, float* __restrict__ y1) {
  const IqaImg im = tab[blockIdx.y];
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= (long long)im.ch * im.cw) return;
  const int y = (int)(p / im.cw), x = (int)(p % im.cw);
  const long long plane = (long long)im.h * im.w, at = (long long)y * im.w + x;
  float ch[3];
  if (layout == FFP_IQA_F32_CHW) {
    const float* s = (const float*)im.src;
    for (int k = 0; k < im.c; ++k) ch[k] = s[k * plane + at];
  } else {
    const unsigned char* s = (const unsigned char*)im.src;
    for (int k = 0; k < im.c; ++k) ch[k] = __fdiv_rn((float)s[at * im.c + k], 255.f);
    if (im.c == 3 && !as_rgb) { const float t = ch[0]; ch[0] = ch[2]; ch[2] = t; }
  }
  float v = ch[0];
  if (im.c == 3) v = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, ch[0]), __fmul_rn(0.587f, ch[1])), __fmul_rn(0.114f, ch[2]));
  y1[im.y1 + p] = rintf(__fmul_rn(v, 255.f));
}

// tmp [ch / 2][cw]: the vertical pass over y / 255
__global__ void __launch_bounds__(kThreads) iqa_half_rows_kernel(const IqaImg* __restrict__ tab, const float* __restrict__ taps, const float* __restrict__ y1,
                                                                 float* __restrict__ tmp) {
  const IqaImg im = tab[blockIdx.y];
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int oh = im.ch / 2;
  if (p >= (long long)oh * im.cw) return;
  const int i = (int)(p / im.cw), x = (int)(p % im.cw);
  const float* src = y1 + im.y1;
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    const int j = reflect(2 * i - 3 + t, im.ch);
    acc += taps[t] * __fdiv_rn(src[(long long)j * im.cw + x], 255.f);
  }
  tmp[im.tmp + p] = acc;
}

// y2 [ch / 2][cw / 2]: the horizontal pass, back on the 0..255 scale
__global__ void __launch_bounds__(kThreads) iqa_half_cols_kernel(const IqaImg* __restrict__ tab, const float* __restrict__ taps, const float* __restrict__ tmp,
                                                                 float* __restrict__ y2) {
  const IqaImg im = tab[blockIdx.y];
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int oh = im.ch / 2, ow = im.cw / 2;
  if (p >= (long long)oh * ow) return;
  const int i = (int)(p / ow), x = (int)(p % ow);
  const float* src = tmp + im.tmp + (long long)i * im.cw;
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < 10; ++t) acc += taps[t] * src[reflect(2 * x - 3 + t, im.cw)];
  y2[im.y2 + p] = acc * 255.f;
}

__device__ __forceinline__ void tally(float v, float* a) {   // a: {sum x^2 | x<0, sum x^2 | x>0, sum |x|, #x<0, #x>0}
  const float q = v * v;
  if (v < 0.f) { a[0] += q; a[3] += 1.f; }
  if (v > 0.f) { a[1] += q; a[4] += 1.f; }
  a[2] += fabsf(v);
}

// One workgroup per block of side B at its scale. LDS: tile [(B+6)^2] | nmap [B^2] | red [waves][26].
template <int B>
__global__ void __launch_bounds__(kThreads) iqa_block_kernel(const IqaImg* __restrict__ tab, int n_img, const float* __restrict__ gauss,
                                                             const float* __restrict__ ybuf, float* __restrict__ sums) {
  constexpr int T = B + 2 * kHalo, SCALE = B == kNiqeBlock ? 0 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* nmap = tile + T * T;
  float* red = nmap + B * B;
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x;
  int lo = 0, hi = n_img - 1;                            // last image whose first block is <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  const IqaImg im = tab[lo];
  const int b = (int)(blk - im.blk0), by = b / im.bcols, bx = b % im.bcols;
  const int H = SCALE ? im.ch / 2 : im.ch, W = SCALE ? im.cw / 2 : im.cw;
  const float* Y = ybuf + (SCALE ? im.y2 : im.y1);
  for (int i = tid; i < T * T; i += kThreads) {
    const int ty = i / T, tx = i % T;
    const int gy = min(max(by * B + ty - kHalo, 0), H - 1), gx = min(max(bx * B + tx - kHalo, 0), W - 1);   // replicate at the crop's edge
    tile[i] = Y[(long long)gy * W + gx];
  }
  float wg[kClasses];
#pragma unroll
  for (int k = 0; k < kClasses; ++k) wg[k] = gauss[k];
  __syncthreads();
  float acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.f;
  // MSCN with the window centred on its own pixel c. The differences d = y - c are summed per weight class first: exact for the integer
  // luma of scale 1, so a local mean that is zero by symmetry is exactly zero and the sign of n (which the fit counts) is not left to
  // rounding. Then m = sum_c w_c S_c, var = sum_c w_c Q_c - m^2, n = (c - (c + m)) / (sigma + 1) = -m / (sigma + 1).
  for (int p = tid; p < B * B; p += kThreads) {
    const int py = p / B, px = p % B;
    const float* t0 = tile + py * T + px;
    const float c = t0[kHalo * T + kHalo];
    float S[kClasses], Q[kClasses];
#pragma unroll
    for (int k = 0; k < kClasses; ++k) S[k] = Q[k] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy)
#pragma unroll
      for (int dx = 0; dx < 7; ++dx) {
        const float d = t0[dy * T + dx] - c;
        S[tap_class(dy, dx)] += d;
        Q[tap_class(dy, dx)] += d * d;
      }
    float m = 0.f, v = 0.f;
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
      m += wg[k] * S[k];
      v += wg[k] * Q[k];
    }
    const float sig = __fsqrt_rn(fabsf(v - m * m));
    nmap[p] = __fdiv_rn(-m, sig + 1.f);
    acc[25] += sig;
  }
  __syncthreads();
  // the block and its products with torch.roll(block, s), s = (0,1), (1,0), (1,1), (1,-1): circular inside the block
  for (int p = tid; p < B * B; p += kThreads) {
    const int py = p / B, px = p % B;
    const int pym = py == 0 ? B - 1 : py - 1, pxm = px == 0 ? B - 1 : px - 1, pxp = px == B - 1 ? 0 : px + 1;
    const float x0 = nmap[p];
    tally(x0, acc);
    tally(x0 * nmap[py * B + pxm], acc + 5);
    tally(x0 * nmap[pym * B + px], acc + 10);
    tally(x0 * nmap[pym * B + pxm], acc + 15);
    tally(x0 * nmap[pym * B + pxp], acc + 20);
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    float s = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[(tid >> 6) * kSums + k] = s;
  }
  __syncthreads();
  if (tid < kSums) {
    float s = red[tid];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += red[w * kSums + tid];
    sums[(blk * 2 + SCALE) * kSums + tid] = s;
  }
}

// One thread per (block, scale, map): the AGGD fit (float64) of the fp32 sums. tabs: [4][kNiqeGam] = r(gam), G(1/gam), G(2/gam), G(3/gam).
__global__ void __launch_bounds__(kThreads) iqa_finalize_kernel(long long n_blocks, const float* __restrict__ sums, const double* __restrict__ tabs,
                                                                double* __restrict__ feat, double* __restrict__ sharp) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_blocks * 10) return;
  const long long blk = t / 10;
  const int m = (int)(t % 10), scale = m / 5, k = m % 5;
  const float* S = sums + (blk * 2 + scale) * kSums;
  const double N = scale ? (kNiqeBlock / 2) * (kNiqeBlock / 2) : kNiqeBlock * kNiqeBlock;
  const double sneg = S[k * 5], spos = S[k * 5 + 1], sabs = S[k * 5 + 2], cneg = S[k * 5 + 3], cpos = S[k * 5 + 4];
  const double left = sqrt(sneg / cneg), right = sqrt(spos / cpos);            // 0 / 0 = NaN: a value, not an error
  const double g = left / right, ma = sabs / N, ms = (sneg + spos) / N;
  const double r = ma * ma / ms, g2 = g * g;
  const double rn = r * (g2 * g + 1) * (g + 1) / ((g2 + 1) * (g2 + 1));
  const double* rg = tabs;
  int idx = 0;                                                                 // argmin over NaN / inf differences is the first index
  if (isfinite(rn)) {
    int lo = 0, hi = kNiqeGam;                                                 // first entry >= rn (the table increases)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rg[mid] < rn) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) idx = 0;
    else if (lo == kNiqeGam) idx = kNiqeGam - 1;
    else {
      const double d0 = (rg[lo - 1] - rn) * (rg[lo - 1] - rn), d1 = (rg[lo] - rn) * (rg[lo] - rn);
      idx = d0 <= d1 ? lo - 1 : lo;
    }
  }
  const double alpha = 0.2 + 0.001 * idx;
  const double g1 = tabs[kNiqeGam + idx], gg2 = tabs[2 * kNiqeGam + idx], g3 = tabs[3 * kNiqeGam + idx];
  const double sc = sqrt(g1 / g3), bl = left * sc, br = right * sc;
  double* F = feat + blk * kNiqeFeat + scale * 18;
  if (k == 0) {
    F[0] = alpha;
    F[1] = (bl + br) / 2;
    if (scale == 0) sharp[blk] = (double)S[25] / N;
  } else {
    F += 2 + 4 * (k - 1);
    F[0] = alpha;
    F[1] = (br - bl) * (gg2 / g1);
    F[2] = bl;
    F[3] = br;
  }
}

double keys_cubic(double x) {
  x = std::fabs(x);
  if (x <= 1) return 1.5 * x * x * x - 2.5 * x * x + 1;
  if (x <= 2) return -0.5 * x * x * x + 2.5 * x * x - 4 * x + 2;
  return 0;
}

template <int B> constexpr size_t block_lds() { return sizeof(float) * ((B + 2 * kHalo) * (B + 2 * kHalo) + B * B + (kThreads / 64) * kSums); }

}  // namespace

IqaEngine::IqaEngine(int device) : dev_(device) {
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "iqa: no HIP device %d (no CPU path)", device);
  FFP_HIP(hipSetDevice(device));
  std::vector<double> tabs(4 * (size_t)kNiqeGam);
  for (int i = 0; i < kNiqeGam; ++i) {
    const double gam = 0.2 + 0.001 * i, g1 = std::tgamma(1 / gam), g2 = std::tgamma(2 / gam), g3 = std::tgamma(3 / gam);
    tabs[i] = g2 * g2 / (g1 * g3);
    tabs[kNiqeGam + i] = g1;
    tabs[2 * (size_t)kNiqeGam + i] = g2;
    tabs[3 * (size_t)kNiqeGam + i] = g3;
  }
  std::vector<float> consts(kClasses + 10);
  double g[7], gs = 0, ks = 0, kw[10];
  const double sigma = 7.0 / 6.0;
  for (int i = 0; i < 7; ++i) g[i] = std::exp(-(double)((i - 3) * (i - 3)) / (2 * sigma * sigma));
  for (int i = 0; i < 49; ++i) gs += g[i / 7] * g[i % 7];
  for (int i = 0; i < 49; ++i) consts[tap_class(i / 7, i % 7)] = (float)(g[i / 7] * g[i % 7] / gs);
  for (int t = 0; t < 10; ++t) { kw[t] = 0.5 * keys_cubic(0.5 * (3.5 - t)); ks += kw[t]; }   // u - j = 3.5 - t for tap j = 2i - 3 + t
  for (int t = 0; t < 10; ++t) consts[kClasses + t] = (float)(kw[t] / ks);
  tabs_.alloc(tabs.size() * sizeof(double));
  consts_.alloc(consts.size() * sizeof(float));
  FFP_HIP(hipMemcpy(tabs_.p, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
  FFP_HIP(hipMemcpy(consts_.p, consts.data(), consts.size() * sizeof(float), hipMemcpyHostToDevice));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&iqa_block_kernel<kNiqeBlock>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)block_lds<kNiqeBlock>()));
  FFP_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
}

IqaEngine::~IqaEngine() {
  if (st_) (void)hipStreamDestroy(st_);
}

// validates the batch, lays the crops out back to back, uploads the images (host sources) and the image table
long long IqaEngine::stage(int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout, int chan_order, bool on_device,
                           int64_t* out_off, long long* max_px) {
  FFP_CHECK(n > 0 && n <= 65535 && imgs && h && w && c, FFP_ERR_ARG, "niqe: null argument or bad image count %d", n);
  FFP_CHECK(layout == FFP_IQA_F32_CHW || layout == FFP_IQA_U8_HWC, FFP_ERR_ARG, "niqe: unknown layout %d", layout);
  FFP_CHECK(chan_order == FFP_CHAN_AS_BGR || chan_order == FFP_CHAN_AS_RGB, FFP_ERR_ARG, "niqe: unknown channel order %d", chan_order);
  const size_t esz = layout == FFP_IQA_F32_CHW ? 4 : 1;
  std::vector<IqaImg> tab(n);
  std::vector<size_t> src_off(n);
  long long y1 = 0, tmp = 0, y2 = 0, blk = 0;
  size_t src_bytes = 0;
  *max_px = 0;
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(imgs[i] && h[i] > 0 && w[i] > 0 && (c[i] == 1 || c[i] == 3), FFP_ERR_ARG, "niqe: image %d is null, empty or has %d channels (1 or 3)", i, c[i]);
    FFP_CHECK(niqe_blocks(h[i], w[i]) >= 2, FFP_ERR_ARG, "niqe: image %d (%d x %d) holds fewer than two 96x96 blocks: one block has no covariance", i, h[i],
              w[i]);
    IqaImg& im = tab[i];
    im.h = h[i]; im.w = w[i]; im.c = c[i];
    im.ch = h[i] / kNiqeBlock * kNiqeBlock; im.cw = w[i] / kNiqeBlock * kNiqeBlock;
    im.bcols = w[i] / kNiqeBlock;
    im.y1 = y1; im.tmp = tmp; im.y2 = y2; im.blk0 = blk;
    if (out_off) out_off[i] = blk;
    const long long px = (long long)im.ch * im.cw;
    y1 += px; tmp += px / 2; y2 += px / 4;
    blk += niqe_blocks(h[i], w[i]);
    *max_px = std::max(*max_px, px);
    src_off[i] = src_bytes;
    src_bytes += ((size_t)h[i] * w[i] * c[i] * esz + 15) & ~(size_t)15;
  }
  if (out_off) out_off[n] = blk;
  FFP_CHECK(blk < (1ll << 31) / 10, FFP_ERR_ARG, "niqe: too many blocks (%lld)", blk);
  FFP_HIP(hipSetDevice(dev_));
  if (!on_device) {
    src_.ensure(src_bytes);
    for (int i = 0; i < n; ++i) {
      FFP_HIP(hipMemcpyAsync((char*)src_.p + src_off[i], imgs[i], (size_t)h[i] * w[i] * c[i] * esz, hipMemcpyHostToDevice, st_));
      tab[i].src = (char*)src_.p + src_off[i];
    }
  } else {
    for (int i = 0; i < n; ++i) tab[i].src = imgs[i];
  }
  imgtab_.ensure(sizeof(IqaImg) * n);
  y1_.ensure(sizeof(float) * y1);
  tmp_.ensure(sizeof(float) * tmp);
  y2_.ensure(sizeof(float) * y2);
  FFP_HIP(hipMemcpyAsync(imgtab_.p, tab.data(), sizeof(IqaImg) * n, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipStreamSynchronize(st_));                   // `tab` is pageable host memory that ends with this call
  return blk;
}

void IqaEngine::luma(const void* img, int h, int w, int c, int layout, int chan_order, float* out_y) {
  FFP_CHECK(out_y, FFP_ERR_ARG, "niqe_luma: null output");
  long long max_px = 0;
  stage(1, &img, &h, &w, &c, layout, chan_order, false, nullptr, &max_px);
  hipLaunchKernelGGL(iqa_luma_kernel, dim3((unsigned)((max_px + kThreads - 1) / kThreads), 1), dim3(kThreads), 0, st_, imgtab_.as<IqaImg>(), layout,
                     chan_order == FFP_CHAN_AS_RGB ? 1 : 0, y1_.as<float>());
  FFP_HIP(hipGetLastError());
  FFP_HIP(hipMemcpyAsync(out_y, y1_.p, sizeof(float) * max_px, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
}

void IqaEngine::niqe_features(int n, const void* const* imgs, const int32_t* h, const int32_t* w, const int32_t* c, int layout, int chan_order,
                              bool on_device, double* out_feat, double* out_sharp, int64_t cap_blocks, int64_t* out_off) {
  FFP_CHECK(out_feat && out_sharp && out_off, FFP_ERR_ARG, "niqe_features: null output");
  if (n > 0 && h && w) {                                 // the capacity before anything is uploaded
    long long need = 0;
    for (int i = 0; i < n; ++i) need += niqe_blocks(std::max(h[i], 0), std::max(w[i], 0));
    FFP_CHECK(need <= cap_blocks, FFP_ERR_ARG, "niqe_features: %lld blocks, the output holds %lld", need, (long long)cap_blocks);
  }
  long long max_px = 0;
  const long long blk = stage(n, imgs, h, w, c, layout, chan_order, on_device, out_off, &max_px);
  sums_.ensure(sizeof(float) * blk * 2 * kSums);
  feat_.ensure(sizeof(double) * blk * kNiqeFeat);
  sharp_.ensure(sizeof(double) * blk);
  const IqaImg* d_tab = imgtab_.as<IqaImg>();
  const float* gauss = consts_.as<float>();
  const float* taps = gauss + kClasses;
  const unsigned gx = (unsigned)((max_px + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(iqa_luma_kernel, dim3(gx, n), dim3(kThreads), 0, st_, d_tab, layout, chan_order == FFP_CHAN_AS_RGB ? 1 : 0, y1_.as<float>());
  hipLaunchKernelGGL(iqa_half_rows_kernel, dim3((gx + 1) / 2, n), dim3(kThreads), 0, st_, d_tab, taps, y1_.as<float>(), tmp_.as<float>());
  hipLaunchKernelGGL(iqa_half_cols_kernel, dim3((gx + 3) / 4, n), dim3(kThreads), 0, st_, d_tab, taps, tmp_.as<float>(), y2_.as<float>());
  hipLaunchKernelGGL(iqa_block_kernel<kNiqeBlock>, dim3((unsigned)blk), dim3(kThreads), block_lds<kNiqeBlock>(), st_, d_tab, n, gauss, y1_.as<float>(),
                     sums_.as<float>());
  hipLaunchKernelGGL(iqa_block_kernel<kNiqeBlock / 2>, dim3((unsigned)blk), dim3(kThreads), block_lds<kNiqeBlock / 2>(), st_, d_tab, n, gauss, y2_.as<float>(),
                     sums_.as<float>());
  hipLaunchKernelGGL(iqa_finalize_kernel, dim3((unsigned)((blk * 10 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st_, blk, sums_.as<float>(),
                     tabs_.as<double>(), feat_.as<double>(), sharp_.as<double>());
  FFP_HIP(hipGetLastError());
  FFP_HIP(hipMemcpyAsync(out_feat, feat_.p, sizeof(double) * blk * kNiqeFeat, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(out_sharp, sharp_.p, sizeof(double) * blk, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
}

// ---- the score: host, float64 ------------------------------------------------------------------------------------------------------
namespace {

// cyclic Jacobi on a symmetric n x n matrix (row-major, destroyed): eigenvalues on the diagonal, eigenvectors in the columns of v
void jacobi_eig(std::vector<double>& a, std::vector<double>& v, int n) {
  v.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0, diag = 0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? diag : off) += a[(size_t)i * n + j] * a[(size_t)i * n + j];
    if (!(off > 1e-40 * diag)) break;                    // also leaves on NaN
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
        for (int k = 0; k < n; ++k) {                    // columns p, q
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = cs * akp - sn * akq;
          a[(size_t)k * n + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; ++k) {                    // rows p, q
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = cs * apk - sn * aqk;
          a[(size_t)q * n + k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
          v[(size_t)k * n + p] = cs * vkp - sn * vkq;
          v[(size_t)k * n + q] = sn * vkp + cs * vkq;
        }
      }
  }
}

}  // namespace

void niqe_score(const double* feat, const int64_t* block_off, int n, const double* mu, const double* cov, double* out) {
  constexpr int F = kNiqeFeat;
  const double nan = std::nan("");
  for (int img = 0; img < n; ++img) {
    const double* X = feat + block_off[img] * F;
    const int64_t nb = block_off[img + 1] - block_off[img];
    double m[F], mc[F];
    int64_t rows = 0;
    for (int f = 0; f < F; ++f) {                        // nanmean per feature
      double s = 0;
      int64_t k = 0;
      for (int64_t b = 0; b < nb; ++b)
        if (!std::isnan(X[b * F + f])) { s += X[b * F + f]; ++k; }
      m[f] = k ? s / k : nan;
      mc[f] = 0;
    }
    std::vector<char> ok(nb, 1);
    for (int64_t b = 0; b < nb; ++b) {
      for (int f = 0; f < F; ++f)
        if (std::isnan(X[b * F + f])) ok[b] = 0;
      if (ok[b]) {
        ++rows;
        for (int f = 0; f < F; ++f) mc[f] += X[b * F + f];
      }
    }
    if (rows < 2) { out[img] = nan; continue; }          // no sample covariance
    for (int f = 0; f < F; ++f) mc[f] /= rows;
    std::vector<double> a((size_t)F * F, 0.0), v;
    for (int64_t b = 0; b < nb; ++b) {
      if (!ok[b]) continue;
      for (int i = 0; i < F; ++i) {
        const double di = X[b * F + i] - mc[i];
        for (int j = i; j < F; ++j) a[(size_t)i * F + j] += di * (X[b * F + j] - mc[j]);
      }
    }
    for (int i = 0; i < F; ++i)
      for (int j = i; j < F; ++j) {
        const double cij = a[(size_t)i * F + j] / (rows - 1);
        a[(size_t)i * F + j] = a[(size_t)j * F + i] = (0.5 * (cov[i * F + j] + cov[j * F + i]) + cij) / 2;
      }
    jacobi_eig(a, v, F);
    double smax = 0;
    for (int i = 0; i < F; ++i) smax = std::max(smax, std::fabs(a[(size_t)i * F + i]));
    const double cut = F * 2.2e-16 * smax;
    double q = 0;
    for (int k = 0; k < F; ++k) {
      const double lam = a[(size_t)k * F + k];
      if (!(std::fabs(lam) > cut)) continue;             // pinv: singular values below the cut count as zero
      double proj = 0;
      for (int i = 0; i < F; ++i) proj += v[(size_t)i * F + k] * (mu[i] - m[i]);
      q += proj * proj / lam;
    }
    out[img] = std::sqrt(q);
  }
}

}  // namespace ffp
