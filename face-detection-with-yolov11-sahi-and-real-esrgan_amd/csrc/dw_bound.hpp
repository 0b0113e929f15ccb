// dw_bound.hpp — the exponent of the fp16 hi/lo split for a tensor that is never stored: the output of a depthwise 3x3 conv computed inside
// the loader of the conv that consumes it (conv_dwpw.hip). No kernel has seen that tensor's max |value|, so the split takes its exponent from
// a bound that follows from the input's max |value| slot and the depthwise weights alone. Plain C++ on both sides: the host packs S and B
// (weights.cpp), the kernel evaluates the bound per image, and dw_bound_host_check.cpp runs all of it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FFP_HD __host__ __device__
#else
#define FFP_HD
#endif

namespace ffp {

constexpr float kSiluMin = 0.2785f;      // |SiLU(v)| <= max(|v|, 0.27847): the activation's dip below zero

// |act(dw(x) + b)| <= max(amax(x) * S + B, 0.2785) for act in {none, SiLU}: S = max_c sum_taps |w_c,tap|, B = max_c |b_c| (dw_weight_norms).
// The rounding of the kernel's nine fp32 fmas stays below 2^-20 of the bound; the split keeps two binades of headroom above it (split_scales_hd).
FFP_HD inline float dw_out_bound(float amax_in, float S, float B) {
  const float b = __builtin_fmaf(amax_in, S, B);
  return b > kSiluMin ? b : kSiluMin;      // a NaN slot gives kSiluMin: the values are NaN whatever the scale
}

FFP_HD inline unsigned f32_bits(float f) { unsigned u; __builtin_memcpy(&u, &f, 4); return u; }
FFP_HD inline float bits_f32(unsigned u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// split_scales (conv_args.hpp) as host/device code: t = 2^(13 - e), tinv = 2^(e - 13), e = exponent of the max-|value| bit pattern; unscaled
// for zero / tiny / inf / nan patterns
FFP_HD inline void split_scales_hd(unsigned amax_bits, float* t, float* tinv) {
  const unsigned eb = (amax_bits >> 23) & 0xFFu;
  const bool ok = eb >= 14u && eb < 255u;
  *t = ok ? bits_f32((267u - eb) << 23) : 1.f;
  *tinv = ok ? bits_f32((eb - 13u) << 23) : 1.f;
}

// conv_dwpw.hip addresses a tensor through ONE buffer resource with 32-bit byte offsets: every tensor it reads or writes (total_px records of cs fp32
// values) has to end below 0x7FFFFFF0 bytes. A level that does not fit keeps the unfused launches (yolo11.cpp asks before it builds the fused ops).
constexpr long long kDwPwSpanLimit = 0x7FFFFFF0ll;
FFP_HD inline bool dwpw_span_fits(long long total_px, int cs) { return total_px >= 0 && cs > 0 && total_px <= kDwPwSpanLimit / 4 / cs && total_px * cs * 4 < kDwPwSpanLimit; }

// host, pack time: w is OIHW (C, 1, k, k) = [c][tap], b may be null. Sums in double, rounded UP to float: the results are upper bounds.
inline void dw_weight_norms(const float* w, const float* b, int C, int taps, float* S, float* B) {
  double s = 0.0, bm = 0.0;
  for (int c = 0; c < C; ++c) {
    double l1 = 0.0;
    for (int t = 0; t < taps; ++t) l1 += std::fabs((double)w[(size_t)c * taps + t]);
    if (l1 > s || std::isnan(l1)) s = l1;
    if (b && (std::fabs((double)b[c]) > bm || std::isnan(b[c]))) bm = std::fabs((double)b[c]);
  }
  auto up = [](double v) { float f = (float)v; if ((double)f < v) f = std::nextafterf(f, INFINITY); return f; };
  *S = up(s);
  *B = up(bm);
}

}  // namespace ffp
