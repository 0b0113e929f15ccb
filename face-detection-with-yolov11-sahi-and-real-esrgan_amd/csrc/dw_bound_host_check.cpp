// dw_bound_host_check.cpp — the host-side arithmetic of the depthwise-fused loader's split exponent (dw_bound.hpp), run under
// AddressSanitizer + UBSan on a CPU-only machine (build.py --dw-bound-check): S and B at pack time, the bound, the bound -> scale step.
// For seeded random depthwise convs and inputs it checks, against a double evaluation of every output:
//   * the bound is a bound: |act(dw(x) + b)| <= dw_out_bound(amax(x), S, B) for act in {none, SiLU}, zero padding included;
//   * the scales are exact powers of two with t * tinv == 1, the scaled bound lies in [2^13, 2^14), so every scaled value is below 2^14 — two
//     binades under fp16's overflow; zero, subnormal-tiny, inf and NaN slots give the unscaled branch or a finite scale, never UB;
//   * S and B are rounded up (never below the double sums);
//   * dwpw_span_fits: the size rule that sends an oversized level back to the unfused launches, at its edge and far past it (no overflow).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dw_bound.hpp"

using namespace ffp;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static double silu(double v) { return v / (1.0 + std::exp(-v)); }

int main() {
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  for (int trial = 0; trial < 200; ++trial) {
    const int C = 4 * (1 + trial % 5), H = 1 + trial % 7, W = 1 + (trial / 7) % 9;
    const float wscale = std::ldexp(1.f, (trial % 9) - 4), xscale = std::ldexp(1.f, (trial * 5) % 41 - 20);
    std::vector<float> w((size_t)C * 9), b(C), x((size_t)H * W * C);
    for (auto& v : w) v = nd(rng) * wscale;
    for (auto& v : b) v = nd(rng) * 0.1f;
    for (auto& v : x) v = nd(rng) * xscale;
    float S = 0.f, B = 0.f;
    dw_weight_norms(w.data(), trial % 3 ? b.data() : nullptr, C, 9, &S, &B);
    double s_ref = 0.0, b_ref = 0.0;
    for (int c = 0; c < C; ++c) {
      double l1 = 0.0;
      for (int t = 0; t < 9; ++t) l1 += std::fabs((double)w[(size_t)c * 9 + t]);
      s_ref = std::fmax(s_ref, l1);
      if (trial % 3) b_ref = std::fmax(b_ref, std::fabs((double)b[c]));
    }
    CHECK((double)S >= s_ref && (double)S <= s_ref * (1.0 + 1e-6) + 1e-40, "S %g against %g", S, s_ref);
    CHECK((double)B >= b_ref && (double)B <= b_ref * (1.0 + 1e-6) + 1e-40, "B %g against %g", B, b_ref);
    float amax = 0.f;
    for (float v : x) amax = std::fmax(amax, std::fabs(v));
    const float bound = dw_out_bound(amax, S, B);
    double out_max = 0.0;
    for (int y = 0; y < H; ++y)
      for (int xx = 0; xx < W; ++xx)
        for (int c = 0; c < C; ++c) {
          double acc = 0.0;
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
              const int yy = y + ky - 1, xq = xx + kx - 1;
              if (yy < 0 || yy >= H || xq < 0 || xq >= W) continue;
              acc += (double)x[((size_t)yy * W + xq) * C + c] * (double)w[(size_t)c * 9 + ky * 3 + kx];
            }
          if (trial % 3) acc += b[c];
          out_max = std::fmax(out_max, std::fmax(std::fabs(acc), std::fabs(silu(acc))));
        }
    CHECK(out_max <= (double)bound * (1.0 + 1e-6), "trial %d: |output| %g above the bound %g", trial, out_max, bound);
    float t, tinv;
    split_scales_hd(f32_bits(bound), &t, &tinv);
    CHECK(t * tinv == 1.f, "scales %g * %g", t, tinv);
    int e;
    CHECK(std::frexp(t, &e) == 0.5f, "scale %g is no power of two", t);
    if (t != 1.f) CHECK(bound * t >= 8192.f && bound * t < 16384.f, "scaled bound %g", bound * t);
    CHECK(out_max * t < 16384.0 * (1.0 + 1e-6) || t == 1.f, "scaled value %g", out_max * t);
  }
  // slots no data explains
  const unsigned odd[] = {0u, 1u, 0x007FFFFFu, 0x06800000u, 0x7F7FFFFFu, 0x7F800000u, 0x7FC00000u, 0xFFFFFFFFu};
  for (unsigned u : odd) {
    const float bound = dw_out_bound(bits_f32(u), 14.5f, 0.25f);
    float t, tinv;
    split_scales_hd(f32_bits(bound), &t, &tinv);
    CHECK(std::isfinite(t) && std::isfinite(tinv) && t > 0.f && tinv > 0.f && t * tinv == 1.f, "slot %08x: scales %g %g", u, t, tinv);
    split_scales_hd(u, &t, &tinv);
    CHECK(std::isfinite(t) && std::isfinite(tinv) && t * tinv == 1.f, "slot %08x taken as it is: scales %g %g", u, t, tinv);
  }
  {   // a zero image: the bound is the bias term or SiLU's dip, whichever is larger
    CHECK(dw_out_bound(0.f, 20.f, 0.f) == kSiluMin, "zero image, no bias");
    CHECK(dw_out_bound(0.f, 20.f, 3.f) == 3.f, "zero image, bias 3");
  }
  {   // which levels the fused kernel may address: every tensor inside one buffer resource
    CHECK(dwpw_span_fits(122ll * 4096, 128) && dwpw_span_fits(305ll * 4096, 128), "2- and 5-frame groups at net input 512 (256 / 640 MB)");
    CHECK(!dwpw_span_fits(305ll * 16384, 128), "5-frame group at net input 1024: 2.56 GB of x16 must keep the unfused launches");
    CHECK(dwpw_span_fits(122ll * 16384, 128) && !dwpw_span_fits(122ll * 16384, 512), "2-frame group at 1024: 1.02 GB fits, four times that does not");
    CHECK(dwpw_span_fits((0x7FFFFFF0ll / 4 - 1) / 128, 128) && !dwpw_span_fits(0x7FFFFFF0ll / 4 / 128 + 1, 128), "the edge");
    CHECK(!dwpw_span_fits(1ll << 62, 128) && !dwpw_span_fits(-1, 128) && !dwpw_span_fits(100, 0), "no overflow, no nonsense");
  }
  std::printf(fails ? "dw_bound_host_check: %d FAILED\n" : "dw_bound_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
