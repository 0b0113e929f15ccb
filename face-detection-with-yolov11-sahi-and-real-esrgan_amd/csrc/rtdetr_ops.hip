// rtdetr_ops.hip — the non-conv operators of Ultralytics RT-DETR-l (rtdetr.cpp), fp32 on every precision: depthwise k5 / k3 s2 convs,
// HGStem's 2x2 s1 ceil-mode max pool, position / query-pos adds, LayerNorm, GELU, multi-head attention at head dim 32, the encoder's
// token gather, the per-image top-300 radix select, box refinement, multi-scale deformable sampling and the predictor's decode.
// Every kernel that writes a tensor a conv reads raises that buffer's max-|value| slot (the exponent of FFP_PREC_F32X3's scaled split).
#include "conv_args.hpp"
#include "rtdetr.hpp"

namespace ffp {

namespace {

__device__ __forceinline__ void raise_slot(unsigned* slot, float m) {
  if (slot) raise_amax(slot, m);          // every lane of the wave reaches this (no early returns before it)
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float4 ld4f(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4f(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float amax4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// ---- depthwise KxK, stride S, pad K/2 (LightConv.conv2: k5 s1 ReLU; the stage DWConvs: k3 s2, no activation) -------------------
template <int K, int S>
__global__ void rt_dwconv_kernel(const float* __restrict__ in, int in_cs, int in_coff, float* __restrict__ out, int out_cs, int out_coff,
                                 const float* __restrict__ w, const float* __restrict__ b, int C, int n, int H, int W, int Ho, int Wo, int act,
                                 unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C >> 2;
  const long long total = (long long)n * Ho * Wo * C4;
  float m = 0.f;
  if (g < total) {
    const int c = (int)(g % C4) * 4;
    const long long px = g / C4;
    const int x = (int)(px % Wo), y = (int)((px / Wo) % Ho), im = (int)(px / ((long long)Wo * Ho));
    float4 acc = ld4f(b + c);
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = y * S + ky - K / 2;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = x * S + kx - K / 2;
        if (ix < 0 || ix >= W) continue;
        const float4 v = ld4f(in + ((size_t)im * H * W + (size_t)iy * W + ix) * in_cs + in_coff + c);
        const float4 wt = ld4f(w + (size_t)(ky * K + kx) * C + c);
        acc.x = fmaf(v.x, wt.x, acc.x); acc.y = fmaf(v.y, wt.y, acc.y); acc.z = fmaf(v.z, wt.z, acc.z); acc.w = fmaf(v.w, wt.w, acc.w);
      }
    }
    if (act == ACT_RELU) { acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f); }
    st4f(out + px * out_cs + out_coff + c, acc);
    m = amax4(acc);
  }
  raise_slot(amax, m);
}

// ---- HGStem: F.pad(x, [0, 1, 0, 1]) then MaxPool2d(2, 1, ceil_mode=True): out (H x W) = max of the 2x2 window, zeros past the edge ------
__global__ void rt_maxpool2_kernel(const float* __restrict__ in, int in_cs, int in_coff, float* __restrict__ out, int out_cs, int out_coff, int C,
                                   int n, int H, int W, unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C >> 2;
  const long long total = (long long)n * H * W * C4;
  float m = 0.f;
  if (g < total) {
    const int c = (int)(g % C4) * 4;
    const long long px = g / C4;
    const int x = (int)(px % W), y = (int)((px / W) % H);
    const long long base = px - (long long)y * W - x;
    float4 r = ld4f(in + px * in_cs + in_coff + c);
    for (int d = 1; d < 4; ++d) {
      const int yy = y + (d >> 1), xx = x + (d & 1);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (yy < H && xx < W) v = ld4f(in + (base + (long long)yy * W + xx) * in_cs + in_coff + c);
      r.x = fmaxf(r.x, v.x); r.y = fmaxf(r.y, v.y); r.z = fmaxf(r.z, v.z); r.w = fmaxf(r.w, v.w);
    }
    st4f(out + px * out_cs + out_coff + c, r);
    m = amax4(r);
  }
  raise_slot(amax, m);
}

// ---- out = a + b[px % period] (src + pos, embed + query_pos) ---------------------------------------------------------------------
__global__ void rt_add_kernel(const float* __restrict__ a, int a_cs, const float* __restrict__ b, int b_cs, long long period, float* __restrict__ out,
                              int out_cs, int C, long long npx, unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C >> 2;
  float m = 0.f;
  if (g < npx * C4) {
    const int c = (int)(g % C4) * 4;
    const long long px = g / C4;
    const float4 u = ld4f(a + px * a_cs + c), v = ld4f(b + (period ? px % period : px) * b_cs + c);
    const float4 r = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    st4f(out + px * out_cs + c, r);
    m = amax4(r);
  }
  raise_slot(amax, m);
}

// ---- LayerNorm over 256 channels (eps 1e-5, two-pass variance about a corrected mean); one wave per token, 4 channels per lane.
// The residual of every post-norm sublayer is already added in the epilogue of the conv that produces x (ConvOp::res1) ----------
__global__ void rt_layernorm_kernel(const float* __restrict__ x, int x_cs, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float* __restrict__ out, int out_cs, long long npx, unsigned* amax) {
  const long long px = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, c = lane * 4;
  float m = 0.f;
  if (px < npx) {
    float4 v = ld4f(x + px * x_cs + c);
    float s = (v.x + v.y) + (v.z + v.w);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / 256.0f);
    float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    // the sum of 256 values is rounded at the ulp of the SUM: with |mean| >> std that leaves the mean off by a visible fraction of the std.
    // The residuals are small, so their mean is accurate: one correction step
    float e = (d0 + d1) + (d2 + d3);
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    const float corr = e * (1.0f / 256.0f);
    d0 -= corr; d1 -= corr; d2 -= corr; d3 -= corr;
    float q = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rs = 1.0f / sqrtf(q * (1.0f / 256.0f) + 1e-5f);
    const float4 g = ld4f(gamma + c), b = ld4f(beta + c);
    const float4 r = make_float4(d0 * rs * g.x + b.x, d1 * rs * g.y + b.y, d2 * rs * g.z + b.z, d3 * rs * g.w + b.w);
    st4f(out + px * out_cs + c, r);
    m = amax4(r);
  }
  raise_slot(amax, m);
}

// ---- exact GELU, in place --------------------------------------------------------------------------------------------------------
__global__ void rt_gelu_kernel(float* __restrict__ x, int cs, int C, long long npx, unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C >> 2;
  float m = 0.f;
  if (g < npx * C4) {
    float* p = x + (g / C4) * cs + (g % C4) * 4;
    float4 v = ld4f(p);
    v.x = 0.5f * v.x * (1.0f + erff(v.x * 0.70710678118654752f));
    v.y = 0.5f * v.y * (1.0f + erff(v.y * 0.70710678118654752f));
    v.z = 0.5f * v.z * (1.0f + erff(v.z * 0.70710678118654752f));
    v.w = 0.5f * v.w * (1.0f + erff(v.w * 0.70710678118654752f));
    st4f(p, v);
    m = amax4(v);
  }
  raise_slot(amax, m);
}

// ---- multi-head attention, 8 heads of 32: qk [px][q 256 | k 256], v [px][256] -> out [px][256]; L tokens per image.
// One workgroup = 64 queries of one (image, head); keys / values go through LDS 64 at a time with an online softmax.
__global__ __launch_bounds__(64) void rt_attention_kernel(const float* __restrict__ qk, int qk_cs, const float* __restrict__ v, int v_cs,
                                                          float* __restrict__ out, int out_cs, int L, float scale, unsigned* amax) {
  __shared__ float ks[64][33], vs[64][33];
  const int im = blockIdx.z, h = blockIdx.y, qi = blockIdx.x * 64 + threadIdx.x;
  const long long base = (long long)im * L;
  float q[32], acc[32];
  const bool live = qi < L;
#pragma unroll
  for (int d = 0; d < 32; ++d) { q[d] = live ? qk[(base + qi) * qk_cs + h * 32 + d] * scale : 0.f; acc[d] = 0.f; }
  float mx = -INFINITY, den = 0.f;
  for (int k0 = 0; k0 < L; k0 += 64) {
    const int kn = min(64, L - k0);
    __syncthreads();
    if (threadIdx.x < kn) {
      const float* kp = qk + (base + k0 + threadIdx.x) * qk_cs + 256 + h * 32;
      const float* vp = v + (base + k0 + threadIdx.x) * v_cs + h * 32;
#pragma unroll
      for (int d = 0; d < 32; ++d) { ks[threadIdx.x][d] = kp[d]; vs[threadIdx.x][d] = vp[d]; }
    }
    __syncthreads();
    for (int j = 0; j < kn; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 32; ++d) s = fmaf(q[d], ks[j][d], s);
      if (s > mx) {
        const float c = expf(mx - s);
        den *= c;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc[d] *= c;
        mx = s;
      }
      const float p = expf(s - mx);
      den += p;
#pragma unroll
      for (int d = 0; d < 32; ++d) acc[d] = fmaf(p, vs[j][d], acc[d]);
    }
  }
  float m = 0.f;
  if (live) {
    const float r = 1.0f / den;
#pragma unroll
    for (int d = 0; d < 32; ++d) { const float o = acc[d] * r; out[(base + qi) * out_cs + h * 32 + d] = o; m = fmaxf(m, fabsf(o)); }
  }
  raise_slot(amax, m);
}

// ---- encoder input: the three input_proj outputs flattened into [image][token][256] (t) and the same times valid_mask (tm) ----------
__global__ void rt_enc_prep_kernel(RtLevels lv, const float* __restrict__ valid, float* __restrict__ t, float* __restrict__ tm, int n,
                                   unsigned* amax_t, unsigned* amax_tm) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int NT = lv.start[3];
  float m = 0.f;
  if (g < (long long)n * NT * 64) {
    const int c = (int)(g & 63) * 4;
    const long long tok = g >> 6;
    const int im = (int)(tok / NT), k = (int)(tok % NT);
    const int l = k < lv.start[1] ? 0 : k < lv.start[2] ? 1 : 2;
    const int hw = lv.start[l + 1] - lv.start[l];
    const float4 v = ld4f(lv.src[l] + ((long long)im * hw + (k - lv.start[l])) * lv.src_cs[l] + c);
    st4f(t + tok * 256 + c, v);
    const float4 z = valid[k] != 0.f ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    st4f(tm + tok * 256 + c, z);
    m = amax4(v);
  }
  raise_slot(amax_t, m);
  raise_slot(amax_tm, m);
}

// ---- per-image top-K of max-over-classes logits: radix select on order-preserving float bits, ties to the lower token index, then the
// K winners ranked by (logit descending, index ascending) — torch.topk's sorted order with a defined order among equal values.
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ int block_excl_scan(int v, int* sh, int* total) {        // 1024 threads
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int a = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const int incl = sh[t];
  *total = sh[1023];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(1024) void rt_topk_kernel(const float* __restrict__ s, int s_cs, int nc, int NT, unsigned* __restrict__ keys, int* __restrict__ idx_out) {
  __shared__ int hist[256];
  __shared__ int scan[1024];
  __shared__ unsigned c_key[RT_NQ];
  __shared__ int c_idx[RT_NQ];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_need;
  const int im = blockIdx.x, t = threadIdx.x;
  unsigned* kk = keys + (size_t)im * NT;
  for (int i = t; i < NT; i += 1024) {
    const float* p = s + ((size_t)im * NT + i) * s_cs;
    float m = p[0];
    for (int c = 1; c < nc; ++c) m = fmaxf(m, p[c]);
    kk[i] = fkey(m);
  }
  if (t == 0) { sh_prefix = 0u; sh_need = RT_NQ; }
  __syncthreads();
  unsigned mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (t < 256) hist[t] = 0;
    __syncthreads();
    const unsigned prefix = sh_prefix;
    for (int i = t; i < NT; i += 1024) {
      const unsigned k = kk[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (t == 0) {
      int need = sh_need, b = 255;
      for (; b > 0; --b) {
        if (hist[b] >= need) break;
        need -= hist[b];
      }
      sh_need = need;
      sh_prefix = prefix | ((unsigned)b << shift);
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  const unsigned T = sh_prefix;
  const int n_eq = sh_need;                 // winners equal to the threshold key: the n_eq lowest indices
  int base = 0, eq_base = 0;
  for (int i0 = 0; i0 < NT; i0 += 1024) {
    const int i = i0 + t;
    const unsigned k = i < NT ? kk[i] : 0u;
    int tot_eq;
    const int eq_before = eq_base + block_excl_scan(i < NT && k == T ? 1 : 0, scan, &tot_eq);
    const bool take = i < NT && (k > T || (k == T && eq_before < n_eq));
    int tot;
    const int pos = base + block_excl_scan(take ? 1 : 0, scan, &tot);
    if (take && pos < RT_NQ) { c_key[pos] = k; c_idx[pos] = i; }
    base += tot;
    eq_base += tot_eq;
  }
  __syncthreads();
  if (t < RT_NQ) {
    const unsigned k = c_key[t];
    const int i = c_idx[t];
    int r = 0;
    for (int j = 0; j < RT_NQ; ++j) r += (c_key[j] > k || (c_key[j] == k && c_idx[j] < i)) ? 1 : 0;
    idx_out[im * RT_NQ + r] = i;
  }
}

// ---- the selected queries: features (256) and logit anchors (4) -------------------------------------------------------------------
__global__ void rt_gather_kernel(const float* __restrict__ e, int e_cs, const int* __restrict__ idx, const float* __restrict__ anchors, int NT, int n,
                                 float* __restrict__ q, int q_cs, float* __restrict__ anc, unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.f;
  if (g < (long long)n * RT_NQ * 65) {
    const int c = (int)(g % 65);
    const long long qi = g / 65;
    const int im = (int)(qi / RT_NQ), k = min(max(idx[qi], 0), NT - 1);
    if (c < 64) {
      const float4 v = ld4f(e + ((long long)im * NT + k) * e_cs + c * 4);
      st4f(q + qi * q_cs + c * 4, v);
      m = amax4(v);
    } else {
      st4f(anc + qi * 4, ld4f(anchors + (size_t)k * 4));
    }
  }
  raise_slot(amax, m);
}

// ---- reference boxes: init  ref = sigmoid(delta + anchor);  refine  ref = sigmoid(delta + inverse_sigmoid(ref, 1e-5)) -------------------
__global__ void rt_ref_kernel(const float* __restrict__ delta, int d_cs, const float* __restrict__ anc, float* __restrict__ ref, int ref_cs, long long nq,
                              unsigned* amax) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.f;
  if (g < nq * 4) {
    const long long qi = g >> 2;
    const int c = (int)(g & 3);
    float base;
    if (anc) {
      base = anc[g];
    } else {
      const float x = fminf(fmaxf(ref[qi * ref_cs + c], 0.f), 1.f);
      base = logf(fmaxf(x, 1e-5f) / fmaxf(1.f - x, 1e-5f));
    }
    const float r = sigm(delta[qi * d_cs + c] + base);
    ref[qi * ref_cs + c] = r;
    m = r;
  }
  raise_slot(amax, m);
}

// ---- MSDeformAttn core: softmax over the 12 (level, point) weights of a head, sampling locations, bilinear gathers as
// F.grid_sample(align_corners=False, zeros), weighted sum. One thread per (query, head, channel): a head's 32 lanes read one 128-byte
// value row per corner. oa = [q][offsets 192 | weights 96] (sampling_offsets and attention_weights as one GEMM).
__global__ __launch_bounds__(256) void rt_deform_kernel(const float* __restrict__ val, int v_cs, const float* __restrict__ oa, int oa_cs,
                                                        const float* __restrict__ ref, int ref_cs, RtLevels lv, float* __restrict__ out, int out_cs,
                                                        unsigned* amax) {
  const long long qi = blockIdx.x;
  const int h = threadIdx.x >> 5, c = threadIdx.x & 31;
  const int NT = lv.start[3];
  const int im = (int)(qi / RT_NQ);
  const float* o = oa + qi * oa_cs;
  float w[12];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 12; ++j) { w[j] = o[192 + h * 12 + j]; mx = fmaxf(mx, w[j]); }
  float den = 0.f;
#pragma unroll
  for (int j = 0; j < 12; ++j) { w[j] = expf(w[j] - mx); den += w[j]; }
  const float inv = 1.0f / den;
  const float rx = ref[qi * ref_cs + 0], ry = ref[qi * ref_cs + 1], rw = ref[qi * ref_cs + 2], rh = ref[qi * ref_cs + 3];
  float acc = 0.f;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int H = lv.h[l], W = lv.w[l];
    const float* vb = val + ((long long)im * NT + lv.start[l]) * v_cs + h * 32 + c;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int j = l * 4 + p;
      const float ox = o[((h * 3 + l) * 4 + p) * 2], oy = o[((h * 3 + l) * 4 + p) * 2 + 1];
      const float lx = rx + ox / 4.0f * rw * 0.5f, ly = ry + oy / 4.0f * rh * 0.5f;
      const float x = lx * (float)W - 0.5f, y = ly * (float)H - 0.5f;
      const float fx0 = floorf(x), fy0 = floorf(y);
      const float ax = x - fx0, ay = y - fy0;
      float s = 0.f;
      if (fx0 > -2.f && fy0 > -2.f && fx0 < (float)W && fy0 < (float)H) {
        const int x0 = (int)fx0, y0 = (int)fy0;
        const bool xa = x0 >= 0, xb = x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
        const float v00 = (xa && ya) ? vb[((long long)y0 * W + x0) * v_cs] : 0.f;
        const float v01 = (xb && ya) ? vb[((long long)y0 * W + x0 + 1) * v_cs] : 0.f;
        const float v10 = (xa && yb) ? vb[((long long)(y0 + 1) * W + x0) * v_cs] : 0.f;
        const float v11 = (xb && yb) ? vb[((long long)(y0 + 1) * W + x0 + 1) * v_cs] : 0.f;
        s = (v00 * (1.f - ax) + v01 * ax) * (1.f - ay) + (v10 * (1.f - ax) + v11 * ax) * ay;
      }
      acc = fmaf(w[j] * inv, s, acc);
    }
  }
  out[qi * out_cs + h * 32 + c] = acc;
  raise_slot(amax, fabsf(acc));
}

// ---- outputs: raw [image][query][4 + nc] (boxes cxcywh, sigmoid scores) and RTDETRPredictor.postprocess -----------------------------
__global__ void rt_raw_kernel(const float* __restrict__ ref, int ref_cs, const float* __restrict__ s, int s_cs, int nc, long long nq, float* __restrict__ raw) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int no = 4 + nc;
  if (g >= nq * no) return;
  const long long qi = g / no;
  const int c = (int)(g % no);
  raw[g] = c < 4 ? ref[qi * ref_cs + c] : sigm(s[qi * s_cs + c - 4]);
}

__global__ __launch_bounds__(1024) void rt_post_kernel(const float* __restrict__ ref, int ref_cs, const float* __restrict__ s, int s_cs, int nc, float conf,
                                                       const float2* __restrict__ orig_wh, float* __restrict__ det, int* __restrict__ counts) {
  __shared__ int scan[1024];
  const int im = blockIdx.x, t = threadIdx.x;
  const long long qi = (long long)im * RT_NQ + t;
  float best = 0.f;
  int cls = 0;
  bool keep = false;
  if (t < RT_NQ) {
    const float* p = s + qi * s_cs;
    best = sigm(p[0]);
    for (int c = 1; c < nc; ++c) {
      const float v = sigm(p[c]);
      if (v > best) { best = v; cls = c; }
    }
    keep = best > conf;
  }
  int tot;
  const int pos = block_excl_scan(keep ? 1 : 0, scan, &tot);
  if (keep) {
    const float2 wh = orig_wh[im];
    const float cx = ref[qi * ref_cs], cy = ref[qi * ref_cs + 1], dw = ref[qi * ref_cs + 2] / 2, dh = ref[qi * ref_cs + 3] / 2;
    float* d = det + ((long long)im * RT_NQ + pos) * 6;
    d[0] = (cx - dw) * wh.x; d[1] = (cy - dh) * wh.y; d[2] = (cx + dw) * wh.x; d[3] = (cy + dh) * wh.y;
    d[4] = best; d[5] = (float)cls;
  }
  if (t == 0) counts[im] = tot;
}

// rt_post for tiles of one frame: workgroup b handles batch item b of the chunk, whose tile is tiles[b] = {x0, y0, x1, y1} in frame pixels.
// FFP_RT_TILES_LOCAL writes rt_post's crop-local rows. FFP_RT_TILES_SAHI restates what sahi's Ultralytics wrapper and ObjectAnnotation do
// to such a row with float boxes: clip the crop-local box against the FULL frame shape, drop it unless x1 < x2 and y1 < y2, then shift it by
// the tile origin (get_shifted_object_prediction: no second clip). Every step is one rounded fp32 operation (no contraction of the
// scale-then-shift into an FMA), so a float32 numpy restatement gives the same bits. Rows stay in query order.
__global__ __launch_bounds__(1024) void rt_post_tiles_kernel(const float* __restrict__ ref, int ref_cs, const float* __restrict__ s, int s_cs, int nc,
                                                             float conf, const int4* __restrict__ tiles, float full_w, float full_h, int mode,
                                                             float* __restrict__ det, int* __restrict__ counts) {
  __shared__ int scan[1024];
  const int im = blockIdx.x, t = threadIdx.x;
  const long long qi = (long long)im * RT_NQ + t;
  float best = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  int cls = 0;
  bool keep = false;
  if (t < RT_NQ) {
    const float* p = s + qi * s_cs;
    best = sigm(p[0]);
    for (int c = 1; c < nc; ++c) {
      const float v = sigm(p[c]);
      if (v > best) { best = v; cls = c; }
    }
    keep = best > conf;
  }
  if (keep) {
    const int4 tl = tiles[im];
    const float w = (float)(tl.z - tl.x), h = (float)(tl.w - tl.y);
    const float cx = ref[qi * ref_cs], cy = ref[qi * ref_cs + 1], dw = ref[qi * ref_cs + 2] / 2, dh = ref[qi * ref_cs + 3] / 2;
    x1 = __fmul_rn(__fsub_rn(cx, dw), w); y1 = __fmul_rn(__fsub_rn(cy, dh), h);
    x2 = __fmul_rn(__fadd_rn(cx, dw), w); y2 = __fmul_rn(__fadd_rn(cy, dh), h);
    if (mode == 1) {
      x1 = fmaxf(x1, 0.f); y1 = fmaxf(y1, 0.f);
      x2 = fminf(x2, full_w); y2 = fminf(y2, full_h);
      keep = x1 < x2 && y1 < y2;
      const float sx = (float)tl.x, sy = (float)tl.y;
      x1 = __fadd_rn(x1, sx); x2 = __fadd_rn(x2, sx); y1 = __fadd_rn(y1, sy); y2 = __fadd_rn(y2, sy);
    }
  }
  int tot;
  const int pos = block_excl_scan(keep ? 1 : 0, scan, &tot);
  if (keep) {
    float* d = det + ((long long)im * RT_NQ + pos) * 6;
    d[0] = x1; d[1] = y1; d[2] = x2; d[3] = y2; d[4] = best; d[5] = (float)cls;
  }
  if (t == 0) counts[im] = tot;
}

unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

void launch_rt_dwconv(const TView& in, const TView& out, const float* w, const float* b, int k, int s, int act, hipStream_t st) {
  const Level& li = *in.lvl;
  const Level& lo = *out.lvl;
  FFP_CHECK(in.C == out.C && in.C % 4 == 0 && in.cs % 4 == 0 && in.coff % 4 == 0 && out.cs % 4 == 0 && out.coff % 4 == 0, FFP_ERR_ARG,
            "rt_dwconv: channel views");
  const long long total = (long long)lo.n * lo.h[0] * lo.w[0] * (in.C / 4);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(nblk(total, 256)), dim3(256), 0, st, (const float*)in.ptr, in.cs, in.coff, (float*)out.ptr, out.cs, out.coff, w, b,
                       in.C, lo.n, li.h[0], li.w[0], lo.h[0], lo.w[0], act, out.amax);
  };
  if (k == 5 && s == 1) go(rt_dwconv_kernel<5, 1>);
  else if (k == 3 && s == 2) go(rt_dwconv_kernel<3, 2>);
  else FFP_CHECK(false, FFP_ERR_ARG, "rt_dwconv: k%d s%d", k, s);
  FFP_HIP(hipGetLastError());
}

void launch_rt_maxpool2(const TView& in, const TView& out, hipStream_t st) {
  const Level& l = *in.lvl;
  const long long total = (long long)l.n * l.h[0] * l.w[0] * (in.C / 4);
  hipLaunchKernelGGL(rt_maxpool2_kernel, dim3(nblk(total, 256)), dim3(256), 0, st, (const float*)in.ptr, in.cs, in.coff, (float*)out.ptr, out.cs,
                     out.coff, in.C, l.n, l.h[0], l.w[0], out.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_add(const TView& a, const float* b, int b_cs, long long period, const TView& out, hipStream_t st) {
  const long long npx = a.lvl->total_px;
  hipLaunchKernelGGL(rt_add_kernel, dim3(nblk(npx * (a.C / 4), 256)), dim3(256), 0, st, (const float*)a.ptr + a.coff, a.cs, b, b_cs, period,
                     (float*)out.ptr + out.coff, out.cs, a.C, npx, out.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_layernorm(const TView& x, const float* gamma, const float* beta, const TView& out, hipStream_t st) {
  FFP_CHECK(x.C == 256 && out.C == 256, FFP_ERR_ARG, "rt_layernorm: 256 channels");
  const long long npx = x.lvl->total_px;
  hipLaunchKernelGGL(rt_layernorm_kernel, dim3(nblk(npx, 4)), dim3(256), 0, st, (const float*)x.ptr + x.coff, x.cs, gamma, beta,
                     (float*)out.ptr + out.coff, out.cs, npx, out.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_gelu(const TView& x, hipStream_t st) {
  const long long npx = x.lvl->total_px;
  hipLaunchKernelGGL(rt_gelu_kernel, dim3(nblk(npx * (x.C / 4), 256)), dim3(256), 0, st, (float*)x.ptr + x.coff, x.cs, x.C, npx, x.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_attention(const TView& qk, const TView& v, const TView& out, int L, hipStream_t st) {
  FFP_CHECK(qk.C == 512 && v.C == 256 && out.C == 256, FFP_ERR_ARG, "rt_attention: 8 heads of 32");
  const int n = (int)(qk.lvl->total_px / L);
  hipLaunchKernelGGL(rt_attention_kernel, dim3((L + 63) / 64, 8, n), dim3(64), 0, st, (const float*)qk.ptr + qk.coff, qk.cs,
                     (const float*)v.ptr + v.coff, v.cs, (float*)out.ptr + out.coff, out.cs, L, 0.17677669529663687f, out.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_enc_prep(const RtLevels& lv, const float* valid, const TView& t, const TView& tm, int n, hipStream_t st) {
  const long long total = (long long)n * lv.start[3] * 64;
  hipLaunchKernelGGL(rt_enc_prep_kernel, dim3(nblk(total, 256)), dim3(256), 0, st, lv, valid, (float*)t.ptr, (float*)tm.ptr, n, t.amax, tm.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_topk(const TView& s, int nc, int NT, int n, unsigned* keys, int* idx, hipStream_t st) {
  FFP_CHECK(NT >= RT_NQ, FFP_ERR_ARG, "rt_topk: %d tokens < %d queries", NT, RT_NQ);
  hipLaunchKernelGGL(rt_topk_kernel, dim3(n), dim3(1024), 0, st, (const float*)s.ptr + s.coff, s.cs, nc, NT, keys, idx);
  FFP_HIP(hipGetLastError());
}

void launch_rt_gather(const TView& e, const int* idx, const float* anchors, int NT, int n, const TView& q, float* anc, hipStream_t st) {
  const long long total = (long long)n * RT_NQ * 65;
  hipLaunchKernelGGL(rt_gather_kernel, dim3(nblk(total, 256)), dim3(256), 0, st, (const float*)e.ptr, e.cs, idx, anchors, NT, n, (float*)q.ptr, q.cs,
                     anc, q.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_ref(const TView& delta, const float* anc, const TView& ref, hipStream_t st) {
  const long long nq = ref.lvl->total_px;
  hipLaunchKernelGGL(rt_ref_kernel, dim3(nblk(nq * 4, 256)), dim3(256), 0, st, (const float*)delta.ptr + delta.coff, delta.cs, anc,
                     (float*)ref.ptr + ref.coff, ref.cs, nq, ref.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_deform(const TView& val, const TView& oa, const TView& ref, const RtLevels& lv, const TView& out, hipStream_t st) {
  const long long nq = out.lvl->total_px;
  FFP_CHECK(val.C == 256 && oa.C == 288 && out.C == 256, FFP_ERR_ARG, "rt_deform: views");
  hipLaunchKernelGGL(rt_deform_kernel, dim3((unsigned)nq), dim3(256), 0, st, (const float*)val.ptr + val.coff, val.cs, (const float*)oa.ptr + oa.coff,
                     oa.cs, (const float*)ref.ptr + ref.coff, ref.cs, lv, (float*)out.ptr + out.coff, out.cs, out.amax);
  FFP_HIP(hipGetLastError());
}

void launch_rt_raw(const TView& ref, const TView& s, int nc, float* raw, hipStream_t st) {
  const long long nq = ref.lvl->total_px;
  hipLaunchKernelGGL(rt_raw_kernel, dim3(nblk(nq * (4 + nc), 256)), dim3(256), 0, st, (const float*)ref.ptr + ref.coff, ref.cs,
                     (const float*)s.ptr + s.coff, s.cs, nc, nq, raw);
  FFP_HIP(hipGetLastError());
}

void launch_rt_post(const TView& ref, const TView& s, int nc, float conf, const float2* orig_wh, int n, float* det, int* counts, hipStream_t st) {
  hipLaunchKernelGGL(rt_post_kernel, dim3(n), dim3(1024), 0, st, (const float*)ref.ptr + ref.coff, ref.cs, (const float*)s.ptr + s.coff, s.cs, nc, conf,
                     orig_wh, det, counts);
  FFP_HIP(hipGetLastError());
}

void launch_rt_post_tiles(const TView& ref, const TView& s, int nc, float conf, const int4* tiles_xyxy, int n, int full_h, int full_w, int mode,
                          float* det, int* counts, hipStream_t st) {
  FFP_CHECK(mode == 0 || mode == 1, FFP_ERR_ARG, "rt_post_tiles: mode %d (FFP_RT_TILES_LOCAL or FFP_RT_TILES_SAHI)", mode);
  hipLaunchKernelGGL(rt_post_tiles_kernel, dim3(n), dim3(1024), 0, st, (const float*)ref.ptr + ref.coff, ref.cs, (const float*)s.ptr + s.coff, s.cs, nc,
                     conf, tiles_xyxy, (float)full_w, (float)full_h, mode, det, counts);
  FFP_HIP(hipGetLastError());
}

}  // namespace ffp
