// conv_dwpw.hip — depthwise 3x3 + activation computed inside the loader of the 1x1 conv that consumes it (FFP_PREC_F32X3), optionally with a
// closing 1x1 conv to at most 4 channels in the epilogue: the YOLO11 class tower  dw3x3+SiLU -> 1x1+SiLU -> dw3x3+SiLU -> 1x1+SiLU -> 1x1
// as two launches instead of five. The depthwise outputs (and, with the closing conv, the last 128-channel tensor) never reach memory.
//
//   * work item = one 16 x 16 pixel tile of one image (the level's 16-row tile table); persistent workgroups of 4 waves stride over the tiles;
//   * per 16-channel chunk: the 18 x 18 halo of the input goes global -> registers -> LDS as fp32 (raw buffer loads; lanes outside the image
//     read zeros through the range check: the depthwise conv's own padding), requested one chunk ahead, across tiles too; thread = pixel
//     computes the 16 depthwise sums in fp32 in dwconv3x3_col_kernel's order (acc from 0, ky then kx ascending, + bias, the same SiLU), so
//     the never-stored tensor has the bits it has when it is stored; the values are split into fp16 hi + lo at the exponent of a BOUND of
//     the tensor (dw_bound.hpp: no kernel has seen its maximum) and written as MFMA A-operand fragments, lane-contiguous: [hi|lo][8 fragments
//     of 32 px][k half][pixel] x 16 B;
//   * wave w owns output channels 32 w .. 32 w + 31 for all 256 pixels (8 accumulator tiles): its B operand — the conv's packed weight
//     fragment of the chunk, the same bytes conv_pw reads — comes straight from L2 into registers, once per chunk and tile, a chunk ahead;
//     k order as in conv_pw: 16-channel group, then ah*bl, al*bh, ah*bh;
//   * epilogue as conv_pw's: inverse scales, bias, SiLU, dword stores of 128-byte channel runs, the image's max-|value| slot raised exactly.
//     FIN: instead of storing, 32 pixels x 128 channels at a time go through LDS and every pixel's logits are fp32 dot products: 8 partial
//     sums of 16 channels (fmaf, ascending), added in ascending order, + bias. No atomics: the same bytes on every run.
// LDS: 25.3 KiB halo + 16 KiB fragments + 2 KiB closing weights = 43.4 KiB, two workgroups per CU. Registers: both forms sit at 256 VGPRs and spill
// 5 / 10 of them (24 / 44 B of scratch per lane): the 128 accumulators beside the halo registers and their address tables; see profiles/cls_tower_fused_ab.txt.
#include <algorithm>

#include "conv_args.hpp"
#include "dw_bound.hpp"

namespace ffp {

namespace {

struct DwPwArgs {
  const float* in;
  const float* dw_w;      // [9][cin]
  const float* dw_b;
  const void* wpk;        // the 1x1 conv's packed fragments [4][ncg] x {hi 1 KiB, lo 1 KiB}
  const float* bias;
  const float* oscale;
  float* out;
  const float* fin_w;     // [nc][128]
  const float* fin_b;
  float* fin_out;
  const int4* tab;        // {first pixel, h, w, 0} per image
  const int4* tiles;      // {image, y0, x0, ..} per 16 x 16 tile
  const unsigned* amax_in;
  unsigned* amax_out;
  unsigned in_bytes, out_bytes, fin_bytes;
  int in_cs, in_coff, cin, ncg, out_cs, out_coff, fin_cs, fin_coff, nc, n_tiles, amax_img, dw_act, act;
  float dw_S, dw_B;
};

constexpr unsigned DP_OOB = 0x80000000u;       // beyond every num_records (< 0x7FFFFFF0), also after adding a chunk offset
constexpr int HP = 18, HPX = HP * HP;          // halo pitch and pixels
constexpr int HREC = 80;                       // bytes per halo pixel: 16 fp32 + 16 B, so that 16 lanes' b128 reads of neighbouring pixels cover all banks once
constexpr int HALO = HPX * HREC;
constexpr int NLD = (HPX * 4 + 255) / 256;     // 16-byte loads per thread and chunk
constexpr int AOFF = HALO, ALO = 8 * 1024;     // fragments: hi plane, lo plane ALO behind it
constexpr int WOFF = AOFF + 2 * ALO;
constexpr int DP_LDS = WOFF + 4 * 128 * 4;
constexpr int TROW = 132 * 4;                  // FIN: pitch of the 32 px x 128 ch transposition rows (in the halo region), 4 banks past a multiple of 64
static_assert(32 * TROW <= HALO && 4 * 32 * 8 * 4 <= 2 * ALO && HALO % 16 == 0, "epilogue scratch fits the stages");

__device__ __forceinline__ float4 sload4(const float* p, int idx) {      // wave-uniform 16-byte load through the scalar cache (see sload)
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(4))) f32x4* cptr;
  const f32x4 v = reinterpret_cast<cptr>(reinterpret_cast<unsigned long long>(p))[idx];
  return make_float4(v[0], v[1], v[2], v[3]);
}

struct DpTile { int img, y0, x0, off, H, W; };

template <bool FIN>
__global__ void __launch_bounds__(256, 2) conv_dwpw_kernel(const DwPwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 31, hh = lane >> 5;
  int t = (int)blockIdx.x;
  if (t >= a.n_tiles) return;
  const int ncg = a.ncg;

  const auto rs_in = buf_rsrc(reinterpret_cast<const unsigned char*>(a.in), a.in_bytes);
  auto load_tile = [&](int ti) {
    const int4 tl = a.tiles[ti];
    const int4 tb = a.tab[tl.x];
    DpTile T;
    T.img = __builtin_amdgcn_readfirstlane(tl.x); T.y0 = __builtin_amdgcn_readfirstlane(tl.y); T.x0 = __builtin_amdgcn_readfirstlane(tl.z);
    T.off = __builtin_amdgcn_readfirstlane(tb.x); T.H = __builtin_amdgcn_readfirstlane(tb.y); T.W = __builtin_amdgcn_readfirstlane(tb.z);
    return T;
  };
  // this thread's NLD vectors of a chunk's halo: (halo pixel, 4-channel quarter) -> LDS offset (tile independent) and byte offset in the input (per tile)
  int hy_[NLD], hx_[NLD], hq_[NLD];
  unsigned ldst[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int idx = tid + 256 * i, px = idx >> 2;
    hq_[i] = idx & 3;
    hy_[i] = px / HP;
    hx_[i] = px - hy_[i] * HP;
    ldst[i] = idx < HPX * 4 ? (unsigned)(px * HREC + hq_[i] * 16) : DP_OOB;
  }
  auto halo_off = [&](const DpTile& T, unsigned (&vo)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int y = T.y0 - 1 + hy_[i], x = T.x0 - 1 + hx_[i];
      const bool ok = ldst[i] != DP_OOB && (unsigned)y < (unsigned)T.H && (unsigned)x < (unsigned)T.W;
      vo[i] = ok ? (unsigned)((T.off + y * T.W + x) * a.in_cs + a.in_coff + hq_[i] * 4) * 4u : DP_OOB;      // < in_bytes < 2^31 (launcher)
    }
  };
  auto issue = [&](uint4 (&r)[NLD], const unsigned (&vo)[NLD], int c) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) r[i] = buf_load16(rs_in, vo[i] + (unsigned)c * 64u);
  };
  const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.wpk) + (size_t)wave * ncg * 2048 + lane * 16;
  auto load_w = [&](int c, uint4& h, uint4& l) {
    h = *reinterpret_cast<const uint4*>(wbase + (size_t)c * 2048);
    l = *reinterpret_cast<const uint4*>(wbase + (size_t)c * 2048 + 1024);
  };

  if constexpr (FIN) {      // the closing conv's weights: visible after the first barrier of the chunk loop
    float* w3 = reinterpret_cast<float*>(smem + WOFF);
    for (int i = tid; i < a.nc * 128; i += 256) w3[i] = a.fin_w[i];
  }

  const int c_out = wave * 32 + p;
  const float bias_c = a.bias[c_out], osc_c = a.oscale[c_out];
  const auto rs_out = buf_rsrc(reinterpret_cast<const unsigned char*>(FIN ? a.fin_out : a.out), FIN ? a.fin_bytes : a.out_bytes);
  const int ty = tid >> 4, tx = tid & 15;      // the pixel this thread computes the depthwise conv of: fragment tid >> 5, row tid & 31
  unsigned char* arec = smem + AOFF + (tid >> 5) * 1024 + (tid & 31) * 16;

  DpTile T = load_tile(t);
  unsigned vo[NLD], von[NLD];
  uint4 raw[NLD], wh, wl;
  halo_off(T, vo);
  issue(raw, vo, 0);
  load_w(0, wh, wl);

  for (;;) {
    float ts, tinv;
    {
      const unsigned ab = (unsigned)sload(a.amax_in, a.amax_img ? T.img : 0);
      split_scales(f32_bits(dw_out_bound(bits_f32(ab), a.dw_S, a.dw_B)), &ts, &tinv);
    }
    const int tn = t + (int)gridDim.x;
    const bool has_next = tn < a.n_tiles;
    DpTile Tn = T;
    if (has_next) { Tn = load_tile(tn); halo_off(Tn, von); }
    else {
#pragma unroll
      for (int i = 0; i < NLD; ++i) von[i] = DP_OOB;      // zeros without memory traffic, never used
    }
    f32x16 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

    for (int c = 0; c < ncg; ++c) {
#pragma unroll
      for (int i = 0; i < NLD; ++i)
        if (ldst[i] != DP_OOB) *reinterpret_cast<uint4*>(smem + ldst[i]) = raw[i];
      if (c + 1 < ncg) issue(raw, vo, c + 1);
      else issue(raw, von, 0);
      __syncthreads();                                   // halo of chunk c complete (and everyone is done with the fragments of chunk c - 1)

      unsigned hi[8], lo[8];
#pragma unroll
      for (int jq = 0; jq < 4; ++jq) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float4 x = *reinterpret_cast<const float4*>(smem + ((ty + ky) * HP + tx + kx) * HREC + jq * 16);
            const float4 w = sload4(a.dw_w, ((ky * 3 + kx) * a.cin + c * 16 + jq * 4) >> 2);
            s.x = fmaf(x.x, w.x, s.x); s.y = fmaf(x.y, w.y, s.y); s.z = fmaf(x.z, w.z, s.z); s.w = fmaf(x.w, w.w, s.w);
          }
        const float4 b = sload4(a.dw_b, (c * 16 + jq * 4) >> 2);
        const float d0 = act_fn(s.x + b.x, a.dw_act), d1 = act_fn(s.y + b.y, a.dw_act), d2 = act_fn(s.z + b.z, a.dw_act), d3 = act_fn(s.w + b.w, a.dw_act);
        split_pair(d0, d1, ts, hi[2 * jq], lo[2 * jq]);
        split_pair(d2, d3, ts, hi[2 * jq + 1], lo[2 * jq + 1]);
      }
      *reinterpret_cast<uint4*>(arec) = make_uint4(hi[0], hi[1], hi[2], hi[3]);                  // channels 0-7: the k half of lanes 0-31
      *reinterpret_cast<uint4*>(arec + 512) = make_uint4(hi[4], hi[5], hi[6], hi[7]);            // channels 8-15: lanes 32-63
      *reinterpret_cast<uint4*>(arec + ALO) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      *reinterpret_cast<uint4*>(arec + ALO + 512) = make_uint4(lo[4], lo[5], lo[6], lo[7]);
      __syncthreads();                                   // fragments of chunk c complete (and everyone is done with the halo)

      union { uint4 u; f16x8 h; } bh, bl;
      bh.u = wh; bl.u = wl;
      load_w(c + 1 < ncg ? c + 1 : 0, wh, wl);           // the next chunk's (next tile's first) weights: a chunk ahead of their MFMAs
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        union { uint4 u; f16x8 h; } ah, al;
        ah.u = *reinterpret_cast<const uint4*>(smem + AOFF + f * 1024 + lane * 16);
        al.u = *reinterpret_cast<const uint4*>(smem + AOFF + ALO + f * 1024 + lane * 16);
        acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bl.h, acc[f], 0, 0, 0);      // small terms first
        acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al.h, bh.h, acc[f], 0, 0, 0);
        acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bh.h, acc[f], 0, 0, 0);
      }
    }

    // ---- epilogue: register i of tile f = pixel 32 f + 8 (i >> 2) + 4 hh + (i & 3) of the 16 x 16 tile (row-major), this lane's channel
    const float osc = osc_c * tinv;
    auto value = [&](float s) { return apply_act(fmaf(s, osc, bias_c), a.act); };      // conv_pw's epilogue, its SiLU
    if constexpr (!FIN) {
      float am = 0.f;
#pragma unroll
      for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = f * 32 + 8 * (i >> 2) + 4 * hh + (i & 3);
          const int y = T.y0 + (q >> 4), x = T.x0 + (q & 15);
          const bool ok = y < T.H && x < T.W;
          const float v = value(acc[f][i]);
          if (ok) am = fmaxf(am, fabsf(v));                                    // pixels past the image's edge are neither stored nor counted
          const unsigned o = ok ? (unsigned)((T.off + y * T.W + x) * a.out_cs + a.out_coff + c_out) * 4u : DP_OOB;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs_out, o, 0, 0);
        }
      if (a.amax_out) raise_amax(a.amax_out + (a.amax_img ? T.img : 0), am);
    } else {
      const float* w3 = reinterpret_cast<const float*>(smem + WOFF);
      float* part = reinterpret_cast<float*>(smem + AOFF);                     // [class][pixel][8 partial sums]
      const int px = tid & 31, pt = tid >> 5;
#pragma unroll
      for (int f = 0; f < 8; ++f) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          *reinterpret_cast<float*>(smem + (8 * (i >> 2) + 4 * hh + (i & 3)) * TROW + c_out * 4) = value(acc[f][i]);
        __syncthreads();                                 // (the first one also: every wave is past its last fragment reads)
        float xv[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 x = *reinterpret_cast<const float4*>(smem + px * TROW + pt * 64 + j * 16);
          xv[4 * j] = x.x; xv[4 * j + 1] = x.y; xv[4 * j + 2] = x.z; xv[4 * j + 3] = x.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < a.nc) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) s = fmaf(xv[j], w3[k * 128 + pt * 16 + j], s);
            part[(k * 32 + px) * 8 + pt] = s;
          }
        __syncthreads();
        if (tid < 32 * a.nc) {
          const int k = tid >> 5;
          float s = part[(k * 32 + px) * 8];
#pragma unroll
          for (int m = 1; m < 8; ++m) s += part[(k * 32 + px) * 8 + m];
          s += a.fin_b[k];
          const int q = f * 32 + px;
          const int y = T.y0 + (q >> 4), x = T.x0 + (q & 15);
          if (y < T.H && x < T.W) {
            const unsigned o = (unsigned)((T.off + y * T.W + x) * a.fin_cs + a.fin_coff + k) * 4u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), rs_out, o, 0, 0);
          }
        }
      }
    }
    if (!has_next) break;
    t = tn;
    T = Tn;
#pragma unroll
    for (int i = 0; i < NLD; ++i) vo[i] = von[i];
  }
}

// bias + {none, SiLU} into fp32, nothing after it
constexpr EpiCaps kEpiDwPw{1u << ACT_NONE | 1u << ACT_SILU, false, false, false, true};

}  // namespace

void conv_dwpw_init() {
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS));
}

bool conv_dwpw_eligible(const ConvOp& op, bool need_storage) {
  if (!op.dw || !op.pc) return false;
  const PackedConv& pc = *op.pc;
  const PackedConv& dw = *op.dw;
  const Level* lv = op.out.lvl;
  if (!lv || op.in.lvl != lv || lv->capacity()) return false;
  bool ok = epilogue_fits(op, kEpiDwPw) && pc.split && pc.dt == F32 && pc.k == 1 && op.stride == 1 && !op.up && !op.has_up2 && !op.gate && pc.cout == 128 &&
            pc.cin % 16 == 0 && pc.cin_pad == pc.cin && pc.ncg == pc.cin / 16 && dw.depthwise() && dw.k == 3 && dw.dt == F32 && dw.cout == pc.cin &&
            (op.dw_act == ACT_NONE || op.dw_act == ACT_SILU) && op.in.dt == F32 && op.in.C == pc.cin && op.in.cs % 4 == 0 && op.in.coff % 4 == 0 && (op.in.ptr || !need_storage) &&
            op.in.amax && (op.in.amax_n == 1 || op.in.amax_n == lv->n) && dwpw_span_fits(lv->total_px, op.in.cs) && op.out.C == 128;
  if (op.fin) {
    ok = ok && op.fin_w && op.fin_w->w.p && op.fin_w->b.p && op.fin->k == 1 && op.fin->cin == 128 && op.fin->cout >= 1 && op.fin->cout <= 4 && op.fin_out.dt == F32 &&
         op.fin_out.C == op.fin->cout && op.fin_out.lvl == lv && (op.fin_out.ptr || !need_storage) && dwpw_span_fits(lv->total_px, op.fin_out.cs);
  } else {
    ok = ok && (op.out.ptr || !need_storage) && (!op.out.amax || op.out.amax_n == op.in.amax_n) && dwpw_span_fits(lv->total_px, op.out.cs);
  }
  return ok;
}

void launch_conv_dwpw(const ConvOp& op, hipStream_t st) {
  FFP_CHECK(conv_dwpw_eligible(op), FFP_ERR_ARG, "conv %s: not eligible for the depthwise-fused kernel", op.pc->name.c_str());
  const PackedConv& pc = *op.pc;
  Level* lv = op.out.lvl;
  DwPwArgs a{};
  a.in = static_cast<const float*>(op.in.ptr);
  a.dw_w = op.dw->w.as<float>(); a.dw_b = op.dw->bias.as<float>();
  a.wpk = pc.w.p; a.bias = pc.bias.as<float>(); a.oscale = pc.oscale.as<float>();
  a.tab = lv->d_tab.as<int4>();
  const int* d_count = nullptr;
  a.tiles = lv->tile_table(16, &a.n_tiles, &d_count, st);
  a.amax_in = op.in.amax;
  a.amax_img = op.in.amax_n > 1 ? 1 : 0;
  a.in_bytes = (unsigned)(lv->total_px * op.in.cs * 4);
  a.in_cs = op.in.cs; a.in_coff = op.in.coff; a.cin = pc.cin; a.ncg = pc.ncg;
  a.dw_act = op.dw_act; a.act = op.act;
  a.dw_S = op.dw->dw_l1; a.dw_B = op.dw->dw_bmax;
  if (a.n_tiles == 0) return;
  const int grid = std::min(a.n_tiles, 512);             // two resident workgroups per CU
  if (op.fin) {
    a.fin_w = op.fin_w->w.as<float>(); a.fin_b = op.fin_w->b.as<float>();
    a.fin_out = static_cast<float*>(op.fin_out.ptr);
    a.fin_cs = op.fin_out.cs; a.fin_coff = op.fin_out.coff; a.nc = op.fin->cout;
    a.fin_bytes = (unsigned)(lv->total_px * op.fin_out.cs * 4);
    hipLaunchKernelGGL(conv_dwpw_kernel<true>, dim3(grid), dim3(256), DP_LDS, st, a);
  } else {
    a.out = static_cast<float*>(op.out.ptr);
    a.out_cs = op.out.cs; a.out_coff = op.out.coff;
    a.out_bytes = (unsigned)(lv->total_px * op.out.cs * 4);
    a.amax_out = op.out.amax;
    hipLaunchKernelGGL(conv_dwpw_kernel<false>, dim3(grid), dim3(256), DP_LDS, st, a);
  }
}

}  // namespace ffp
