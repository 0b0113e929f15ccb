// resize.hip — the two cv2.resize calls of RealESRGANer.enhance (realesrgan 0.3.0; reference call utils/enhancer.py:214):
//   * INTER_LANCZOS4 of the quantised result when outscale != scale (u8 / u16, 1, 3 or 4 channels);
//   * INTER_LINEAR of the float32 alpha plane for alpha_upsampler != 'realesrgan', fused with the quantisation into
//     channel 3 of the output canvas.
// Both restate OpenCV's resizeGeneric set-up: fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx, with
// scale_x = 1 / ((double)W_out / w). One thread per output pixel; taps are read through L1 / L2.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "sr_ops.hpp"

namespace ffp {

// OpenCV's interpolateLanczos4(x): the sines in double on the host (libm), so that every caller builds the same table.
// `x + 3` is formed in float, as OpenCV forms it from its float argument.
Lanczos4Axis lanczos4_axis(int n_in, int n_out) {
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  Lanczos4Axis a;
  a.ofs.resize(n_out);
  a.coef.resize((size_t)n_out * 8);
  a.icoef.resize((size_t)n_out * 8);
  const double scale = 1.0 / ((double)n_out / n_in);
  for (int d = 0; d < n_out; ++d) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    const int sx = (int)std::floor(fx);
    fx -= (float)sx;
    a.ofs[d] = sx;
    const float x3 = fx + 3.f;
    const double y0 = -(double)x3 * M_PI * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
    float c[8], sum = 0.f;
    for (int i = 0; i < 8; ++i) {
      const float t = x3 - (float)i;
      if (std::fabs(t) >= 1e-6f) {
        const double y = -(double)t * M_PI * 0.25;
        c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
      } else {
        c[i] = 1e30f;
      }
      sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; ++i) {
      c[i] *= sum;
      a.coef[(size_t)d * 8 + i] = c[i];
      a.icoef[(size_t)d * 8 + i] = (int16_t)std::lrint(c[i] * 2048.f);   // saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE)
    }
  }
  return a;
}

size_t lanczos4_table_bytes(int out_h, int out_w) { return (size_t)(out_h + out_w) * (sizeof(int) + 8 * sizeof(float)); }

void lanczos4_pack(const Lanczos4Axis& ax, const Lanczos4Axis& ay, int wide, void* host_tab) {
  const size_t ow = ax.ofs.size(), oh = ay.ofs.size();
  int* ofs = reinterpret_cast<int*>(host_tab);
  std::memcpy(ofs, ax.ofs.data(), ow * sizeof(int));
  std::memcpy(ofs + ow, ay.ofs.data(), oh * sizeof(int));
  void* c = ofs + ow + oh;
  if (wide) {
    std::memcpy(c, ax.coef.data(), ow * 8 * sizeof(float));
    std::memcpy(reinterpret_cast<float*>(c) + ow * 8, ay.coef.data(), oh * 8 * sizeof(float));
  } else {
    std::memcpy(c, ax.icoef.data(), ow * 8 * sizeof(int16_t));
    std::memcpy(reinterpret_cast<int16_t*>(c) + ow * 8, ay.icoef.data(), oh * 8 * sizeof(int16_t));
  }
}

namespace {

// 8-bit: int16 weights (x2048 per axis), int32 sums, (v + 2^21) >> 22 saturated (FixedPtCast<int, uchar, 22>).
// 16-bit: float weights, float sums left to right, rint saturated (saturate_cast<ushort>(float)).
template <typename T, int CN>
__global__ void resize_lanczos4_kernel(const T* __restrict__ src, int h, int w, const int* __restrict__ tab, int oh, int ow,
                                       T* __restrict__ dst) {
  constexpr bool kWide = sizeof(T) == 2;
  using Coef = typename std::conditional<kWide, float, int16_t>::type;
  using Acc = typename std::conditional<kWide, float, int>::type;
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)oh * ow) return;
  const int dy = (int)(g / ow), dx = (int)(g - (long long)dy * ow);
  const int* xofs = tab;
  const int* yofs = tab + ow;
  const Coef* xc = reinterpret_cast<const Coef*>(tab + ow + oh) + (size_t)dx * 8;
  const Coef* yc = reinterpret_cast<const Coef*>(tab + ow + oh) + (size_t)ow * 8 + (size_t)dy * 8;
  int xs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) xs[k] = min(max(xofs[dx] - 3 + k, 0), w - 1) * CN;
  Acc v[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) v[c] = (Acc)0;
  for (int r = 0; r < 8; ++r) {
    const T* row = src + (size_t)min(max(yofs[dy] - 3 + r, 0), h - 1) * w * CN;
    Acc hs[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) hs[c] = (Acc)0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const Acc a = (Acc)xc[k];
#pragma unroll
      for (int c = 0; c < CN; ++c) hs[c] += (Acc)row[xs[k] + c] * a;
    }
    const Acc b = (Acc)yc[r];
#pragma unroll
    for (int c = 0; c < CN; ++c) v[c] += hs[c] * b;
  }
  T* o = dst + (size_t)g * CN;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    if constexpr (kWide) o[c] = (T)fminf(fmaxf(rintf((float)v[c]), 0.f), 65535.f);
    else o[c] = (T)min(max(((int)v[c] + (1 << 21)) >> 22, 0), 255);
  }
}

// cv2.resize(alpha, (ow, oh), INTER_LINEAR) of alpha = x[..., 3] / range (float32), then rint(a * range) into channel 3.
// Horizontally a tap outside [0, w - 1] resets to the border pixel with weight 0; vertically only the rows are clamped.
template <typename TS, typename TD>
__global__ void alpha_linear_kernel(const TS* __restrict__ src, int h, int w, float range, double scale_x, double scale_y, int oh, int ow,
                                    TD* __restrict__ dst) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)oh * ow) return;
  const int dy = (int)(g / ow), dx = (int)(g - (long long)dy * ow);
  float fx = (float)((dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.f; }
  if (sx >= w - 1) { sx = w - 1; fx = 0.f; }
  const int sx1 = min(sx + 1, w - 1);
  float fy = (float)((dy + 0.5) * scale_y - 0.5);
  const int sy = (int)floorf(fy);
  fy -= (float)sy;
  const int sy0 = min(max(sy, 0), h - 1), sy1 = min(max(sy + 1, 0), h - 1);
  auto A = [&](int y, int x) { return (float)src[((size_t)y * w + x) * 4 + 3] / range; };
  const float h0 = A(sy0, sx) * (1.f - fx) + A(sy0, sx1) * fx;
  const float h1 = A(sy1, sx) * (1.f - fx) + A(sy1, sx1) * fx;
  const float v = h0 * (1.f - fy) + h1 * fy;
  dst[(size_t)g * 4 + 3] = (TD)fminf(fmaxf(rintf(v * range), 0.f), range);
}

}  // namespace

void launch_resize_lanczos4(const void* d_src, int h, int w, int cn, int wide, const void* d_tab, int out_h, int out_w, void* d_dst,
                            hipStream_t st) {
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, FFP_ERR_ARG, "resize_lanczos4: empty image");
  const long long total = (long long)out_h * out_w;
  const unsigned nb = (unsigned)((total + 255) / 256);
  const int* tab = reinterpret_cast<const int*>(d_tab);
#define FFP_RL4(T, CN) \
  hipLaunchKernelGGL((resize_lanczos4_kernel<T, CN>), dim3(nb), dim3(256), 0, st, (const T*)d_src, h, w, tab, out_h, out_w, (T*)d_dst)
  if (!wide && cn == 1) FFP_RL4(uint8_t, 1);
  else if (!wide && cn == 3) FFP_RL4(uint8_t, 3);
  else if (!wide && cn == 4) FFP_RL4(uint8_t, 4);
  else if (wide && cn == 1) FFP_RL4(uint16_t, 1);
  else if (wide && cn == 3) FFP_RL4(uint16_t, 3);
  else if (wide && cn == 4) FFP_RL4(uint16_t, 4);
  else fail(FFP_ERR_ARG, "resize_lanczos4: no kernel for %d channels, wide %d", cn, wide);
#undef FFP_RL4
  FFP_HIP(hipGetLastError());
}

void launch_alpha_linear(const void* d_src, int h, int w, int src_wide, float range, int out_h, int out_w, void* d_dst, int dst_wide,
                         hipStream_t st) {
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, FFP_ERR_ARG, "alpha_linear: empty image");
  const long long total = (long long)out_h * out_w;
  const unsigned nb = (unsigned)((total + 255) / 256);
  const double sx = 1.0 / ((double)out_w / w), sy = 1.0 / ((double)out_h / h);
  if (!src_wide && !dst_wide)
    hipLaunchKernelGGL((alpha_linear_kernel<uint8_t, uint8_t>), dim3(nb), dim3(256), 0, st, (const uint8_t*)d_src, h, w, range, sx, sy,
                       out_h, out_w, (uint8_t*)d_dst);
  else if (src_wide && !dst_wide)
    hipLaunchKernelGGL((alpha_linear_kernel<uint16_t, uint8_t>), dim3(nb), dim3(256), 0, st, (const uint16_t*)d_src, h, w, range, sx, sy,
                       out_h, out_w, (uint8_t*)d_dst);
  else if (src_wide && dst_wide)
    hipLaunchKernelGGL((alpha_linear_kernel<uint16_t, uint16_t>), dim3(nb), dim3(256), 0, st, (const uint16_t*)d_src, h, w, range, sx, sy,
                       out_h, out_w, (uint16_t*)d_dst);
  else
    fail(FFP_ERR_ARG, "alpha_linear: 8-bit input with a 16-bit canvas");
  FFP_HIP(hipGetLastError());
}

}  // namespace ffp
