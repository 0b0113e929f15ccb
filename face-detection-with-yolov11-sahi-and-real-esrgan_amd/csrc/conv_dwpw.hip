// conv_dwpw.hip — depthwise 3x3 + activation computed inside the loader of the 1x1 conv that consumes it (FFP_PREC_F32X3), optionally with a
// closing 1x1 conv to at most 4 channels in the epilogue: the YOLO11 class tower  dw3x3+SiLU -> 1x1+SiLU -> dw3x3+SiLU -> 1x1+SiLU -> 1x1
// as two launches instead of five. The depthwise outputs (and, with the closing conv, the last 128-channel tensor) never reach memory.
//
//   * work item = one 16 x TH pixel tile of one image, TH = 8 or 16 (the level's tile table of that height); persistent workgroups of 4 waves
//     stride over the tiles. The launcher takes 8 rows on every level (see launch_conv_dwpw); the 16-row form is kept behind ConvOp::dwpw_force;
//   * depthwise stage, per 16-channel chunk: wave w computes channel quarter w. It stages the (TH + 2) x 18 halo of its 4 channels for itself,
//     global -> registers -> its own 16-byte-per-pixel LDS region as fp32 (raw buffer loads; lanes outside the image read zeros through the range
//     check: the depthwise conv's own padding), requested one chunk ahead, across tiles too — no other wave reads it, so no barrier guards it.
//     Lane = (column, strip of TH / 4 consecutive rows): a 3-row window slides down the strip, 18 (TH 16) or 12 (TH 8) b128 halo reads per lane
//     and chunk; weights and bias are wave-uniform scalar loads (10 x 16 B per chunk). The sums are fp32 in dwconv3x3_col_kernel's order (acc
//     from 0, ky then kx ascending, + bias, act_fn's SiLU), so the never-stored tensor has the bits it has when it is stored; the values are
//     split into fp16 hi + lo at the exponent of a BOUND of the tensor (dw_bound.hpp: no kernel has seen its maximum) and written as the wave's
//     8 bytes of the pixels' MFMA A-operand records, lane-contiguous: [hi|lo][TH / 2 fragments of 32 px][k half][pixel] x 16 B;
//   * wave w owns output channels 32 w .. 32 w + 31 for all pixels (TH / 2 accumulator tiles): its B operand — the conv's packed weight
//     fragment of the chunk, the same bytes conv_pw reads — comes straight from L2 into registers, once per chunk and tile, ahead of its use;
//     k order as in conv_pw: 16-channel group, then ah*bl, al*bh, ah*bh;
//   * the fragment planes are double-buffered and a chunk costs ONE barrier: behind it a wave runs, as one block of straight-line code, the
//     MFMAs of chunk c (two fragments' worth in front of each row of its strip) and the depthwise arithmetic of chunk c + 1 into the other
//     buffer, so the matrix pipe works while the wave's VALU does the next chunk. A tile's first chunk is staged alone;
//   * epilogue as conv_pw's: inverse scales, bias, SiLU, dword stores of 128-byte channel runs, the image's max-|value| slot raised exactly.
//     FIN: instead of storing, 32 pixels x 128 channels at a time go through LDS (over the halos) and every pixel's logits are fp32 dot
//     products: 8 partial sums of 16 channels (fmaf, ascending), added in ascending order, + bias. No atomics: the same bytes on every run.
// Every output has the bits the three-phase schedule before it gave (tests/test_gpu_cls_tower_bits.py against a recording of that kernel).
// LDS, TH 16 / 8: 20.3 / 16.5 KiB halos (8: the FIN transposition rows are the larger) + 32 / 16 KiB fragments + 2 KiB closing weights = 54.3 /
// 34.5 KiB. Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any of the four):
//   <false, 16> 253 VGPRs, <true, 16> 256: two workgroups per CU;   <false, 8> 164, <true, 8> 167: three (__launch_bounds__(256, 3)).
#include <algorithm>
#include <type_traits>

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
constexpr int HP = 18;                         // halo pitch in pixels
constexpr int TROW = 132 * 4;                  // FIN: pitch of the 32 px x 128 ch transposition rows (in the halo region), 4 banks past a multiple of 64
constexpr int DP_SLOTS = 512, DP_SLOTS8 = 768;  // resident workgroups on 256 CUs: two per CU with 16-row tiles, three with 8-row tiles (registers: 64 accumulators less)

// the stages of a TH-row tile in LDS: [4 waves' halos, 16 B per pixel | 2 x {hi, lo} fragment planes | closing weights]
template <int TH>
struct DpGeo {
  static constexpr int HPX = (TH + 2) * HP;                  // halo pixels
  static constexpr int NLD = (HPX + 63) / 64;                // 16-byte loads per lane and chunk
  static constexpr int WHALO = HPX * 16;                     // one wave's halo: its 4 channels of every pixel; 16 lanes' b128 reads of neighbouring pixels cover all banks once
  static constexpr int HALO = 4 * WHALO > 32 * TROW ? 4 * WHALO : 32 * TROW;
  static constexpr int NF = TH / 2;                          // fragments of 32 pixels
  static constexpr int APL = NF * 1024, ABUF = 2 * APL;      // hi plane, lo plane APL behind it
  static constexpr int AOFF = HALO, WOFF = AOFF + 2 * ABUF;
  static constexpr int LDS = WOFF + 4 * 128 * 4;
  static constexpr int RPL = TH / 4;                         // rows of a lane's strip
  static_assert(TH == 8 || TH == 16, "tile heights");
  static_assert(4 * 32 * 8 * 4 <= 2 * ABUF && HALO % 16 == 0 && WHALO % 16 == 0, "epilogue scratch fits the stages");
};

__device__ __forceinline__ float4 sload4(const float* p, int idx) {      // wave-uniform 16-byte load through the scalar cache (see sload)
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(4))) f32x4* cptr;
  const f32x4 v = reinterpret_cast<cptr>(reinterpret_cast<unsigned long long>(p))[idx];
  return make_float4(v[0], v[1], v[2], v[3]);
}

// LDS traffic inside one wave (its own halo): writes of all lanes before the reads of any, for the compiler; the hardware runs a wave's LDS
// instructions in order
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct DpTile { int img, y0, x0, off, H, W; };

template <bool FIN, int TH>
__global__ void __launch_bounds__(256, TH == 8 ? 3 : 2) conv_dwpw_kernel(const DwPwArgs a) {      // workgroups per CU: what DP_SLOTS* promise the launcher
  using G = DpGeo<TH>;
  constexpr int NLD = G::NLD, NF = G::NF;
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
  // wave w stages channel quarter w of every chunk for itself: halo pixel lane + 64 i -> its 16 bytes in the wave's own halo (tile independent)
  // and their byte offset in the input (per tile)
  unsigned char* hbase = smem + wave * G::WHALO;
  auto halo_off = [&](const DpTile& T, unsigned (&vo)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int px = lane + 64 * i, hy = px / HP, hx = px - hy * HP;
      const int y = T.y0 - 1 + hy, x = T.x0 - 1 + hx;
      const bool ok = px < G::HPX && (unsigned)y < (unsigned)T.H && (unsigned)x < (unsigned)T.W;
      vo[i] = ok ? (unsigned)((T.off + y * T.W + x) * a.in_cs + a.in_coff + wave * 4) * 4u : DP_OOB;      // < in_bytes < 2^31 (launcher)
    }
  };
  auto issue = [&](uint4 (&r)[NLD], const unsigned (&vo)[NLD], int c) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) r[i] = buf_load16(rs_in, vo[i] + (unsigned)c * 64u);
  };
  auto store_halo = [&](const uint4 (&r)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i)
      if (64 * (i + 1) <= G::HPX || lane + 64 * i < G::HPX) *reinterpret_cast<uint4*>(hbase + (lane + 64 * i) * 16) = r[i];
  };
  const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.wpk) + (size_t)wave * ncg * 2048 + lane * 16;
  auto load_w = [&](int c, uint4& h, uint4& l) {
    h = *reinterpret_cast<const uint4*>(wbase + (size_t)c * 2048);
    l = *reinterpret_cast<const uint4*>(wbase + (size_t)c * 2048 + 1024);
  };

  if constexpr (FIN) {      // the closing conv's weights: visible after the first barrier of the chunk loop
    float* w3 = reinterpret_cast<float*>(smem + G::WOFF);
    for (int i = tid; i < a.nc * 128; i += 256) w3[i] = a.fin_w[i];
  }

  const int c_out = wave * 32 + p;
  const float bias_c = a.bias[c_out], osc_c = a.oscale[c_out];
  const auto rs_out = buf_rsrc(reinterpret_cast<const unsigned char*>(FIN ? a.fin_out : a.out), FIN ? a.fin_bytes : a.out_bytes);

  // depthwise stage: lane = (column tx, strip of RPL consecutive rows), the wave's 4 channels of each of its pixels from a 3-row window that
  // slides down the strip; sums in dwconv3x3_col_kernel's order (acc from 0, ky then kx ascending, + bias, the same SiLU). The hi / lo pairs
  // are the wave's 8 bytes of the pixel's 16-byte A-fragment records.
  const int tx = lane & 15, row0 = (lane >> 4) * G::RPL;
  const unsigned char* hwin = hbase + (row0 * HP + tx) * 16;
  const int frag_off = ((row0 * 16 + tx) >> 5) * 1024 + ((row0 * 16 + tx) & 31) * 16 + (wave >> 1) * 512 + (wave & 1) * 8;      // pixel q: fragment q >> 5, row q & 31
  const bool dw_silu = a.dw_act == ACT_SILU;      // (ACT_NONE otherwise: conv_dwpw_eligible)
  auto dw_act = [&](float v) {                    // act_fn's values without a branch per element, so that the stage is one block the MFMAs can sit in
    const float sv = act_fn(v, ACT_SILU);
    return dw_silu ? sv : v;
  };

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
    f32x16 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

    // One step of the chunk pipeline, in one block of straight-line code: the MFMAs of chunk c (MMA) and beside them the depthwise stage of
    // chunk c + 1 (DW), two fragments' MFMAs in front of each row of the strip, so that the matrix pipe works while the wave's VALU does the
    // next chunk. The halo requests run one chunk ahead of the depthwise stage, across tiles too.
    auto step = [&](int c, auto mma_tag, auto dw_tag) {
      constexpr bool MMA = decltype(mma_tag)::value, DW = decltype(dw_tag)::value;
      const int cd = MMA ? c + 1 : c;                        // the chunk the depthwise stage works on: into fragment buffer cd & 1
      union { uint4 u; f16x8 h; } bh, bl;
      const unsigned char* ab = smem + G::AOFF + (c & 1) * G::ABUF + lane * 16;
      if constexpr (MMA) { bh.u = wh; bl.u = wl; }
      float4 w[9], b, win[3][3];
      unsigned char* rec = smem + G::AOFF + (cd & 1) * G::ABUF + frag_off;
      auto hld = [&](int r, int kx) {
        const uint4 u = *reinterpret_cast<const uint4*>(hwin + (r * HP + kx) * 16);
        return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
      };
      if constexpr (DW) {
        store_halo(raw);                                     // the wave's own halo: it is past its reads of the chunk before
        const bool more = cd + 1 < ncg;
#pragma unroll
        for (int i = 0; i < NLD; ++i) raw[i] = buf_load16(rs_in, more ? vo[i] + (unsigned)(cd + 1) * 64u : von[i]);
        wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = sload4(a.dw_w, (k * a.cin + cd * 16 + wave * 4) >> 2);
        b = sload4(a.dw_b, (cd * 16 + wave * 4) >> 2);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) win[r][kx] = hld(r, kx);
      }
#pragma unroll
      for (int r = 0; r < G::RPL; ++r) {
        if constexpr (MMA) {
#pragma unroll
          for (int f = r * (NF / G::RPL); f < (r + 1) * (NF / G::RPL); ++f) {
            union { uint4 u; f16x8 h; } ah, al;
            ah.u = *reinterpret_cast<const uint4*>(ab + f * 1024);
            al.u = *reinterpret_cast<const uint4*>(ab + G::APL + f * 1024);
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bl.h, acc[f], 0, 0, 0);      // small terms first
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al.h, bh.h, acc[f], 0, 0, 0);
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bh.h, acc[f], 0, 0, 0);
          }
          // the next chunk's (next tile's first) weights, into the registers the last MFMAs have just read: most of a row's arithmetic ahead of their use
          if (r == G::RPL - 1) load_w(c + 1 < ncg ? c + 1 : 0, wh, wl);
        }
        if constexpr (DW) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) win[2][kx] = hld(r + 2, kx);
          float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              const float4 x = win[ky][kx], wk = w[ky * 3 + kx];
              s.x = fmaf(x.x, wk.x, s.x); s.y = fmaf(x.y, wk.y, s.y); s.z = fmaf(x.z, wk.z, s.z); s.w = fmaf(x.w, wk.w, s.w);
            }
          const float d0 = dw_act(s.x + b.x), d1 = dw_act(s.y + b.y), d2 = dw_act(s.z + b.z), d3 = dw_act(s.w + b.w);
          unsigned h0, l0, h1, l1;
          split_pair(d0, d1, ts, h0, l0);
          split_pair(d2, d3, ts, h1, l1);
          const int ro =(r >> 1) * 1024 + (r & 1) * 256;      // row r of the strip (strips start on even rows): 16 records on, every other one in the next fragment
          *reinterpret_cast<uint2*>(rec + ro) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(rec + ro + G::APL) = make_uint2(l0, l1);
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) { win[0][kx] = win[1][kx]; win[1][kx] = win[2][kx]; }
        }
      }
    };
    step(0, std::false_type{}, std::true_type{});
    for (int c = 0; c + 1 < ncg; ++c) {
      __syncthreads();      // fragments of chunk c complete; everyone is done with the MFMAs of chunk c - 1, whose buffer chunk c + 1 takes
      step(c, std::true_type{}, std::true_type{});
    }
    __syncthreads();
    step(ncg - 1, std::true_type{}, std::false_type{});

    // ---- epilogue: register i of tile f = pixel 32 f + 8 (i >> 2) + 4 hh + (i & 3) of the 16 x TH tile (row-major), this lane's channel
    const float osc = osc_c * tinv;
    auto value = [&](float s) { return apply_act(fmaf(s, osc, bias_c), a.act); };      // conv_pw's epilogue, its SiLU
    if constexpr (!FIN) {
      float am = 0.f;
#pragma unroll
      for (int f = 0; f < NF; ++f)
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
      const float* w3 = reinterpret_cast<const float*>(smem + G::WOFF);
      float* part = reinterpret_cast<float*>(smem + G::AOFF);                  // [class][pixel][8 partial sums]
      const int px = tid & 31, pt = tid >> 5;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          *reinterpret_cast<float*>(smem + (8 * (i >> 2) + 4 * hh + (i & 3)) * TROW + c_out * 4) = value(acc[f][i]);
        __syncthreads();                                 // (the first one also: every wave is past its last fragment and halo reads)
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
    // the next tile's first chunk goes into fragment buffer 0 and the waves' halos: behind the epilogue's scratch, and behind the MFMAs of an odd last chunk
    if (FIN || (ncg & 1)) __syncthreads();
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
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<false, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, DpGeo<16>::LDS));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<true, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, DpGeo<16>::LDS));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<false, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, DpGeo<8>::LDS));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dwpw_kernel<true, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, DpGeo<8>::LDS));
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
  // tile height: 8 rows on every level. Deep levels get twice the workgroups, each with half the latency chain (P5 of a 2-frame group: 122 one-tile
  // workgroups became 244), and the 64 accumulators less let three workgroups share a CU where the 16-row form fits two, which pays at P3 too
  // (profiles/cls_tower_tail_ab.txt). Nothing is timed at run time: a plan is the same on every run and machine. Tests pin either height and cap
  // the workgroups (ConvOp::dwpw_force).
  const int force_h = op.dwpw_force & 3, cap = op.dwpw_force >> 2;
  FFP_CHECK(op.dwpw_force >= 0 && force_h <= 2, FFP_ERR_ARG, "conv %s: dwpw_force %d", pc.name.c_str(), op.dwpw_force);
  const int th = force_h == 1 ? 16 : 8;
  const int* d_count = nullptr;
  a.tiles = lv->tile_table(th, &a.n_tiles, &d_count, st);
  a.amax_in = op.in.amax;
  a.amax_img = op.in.amax_n > 1 ? 1 : 0;
  a.in_bytes = (unsigned)(lv->total_px * op.in.cs * 4);
  a.in_cs = op.in.cs; a.in_coff = op.in.coff; a.cin = pc.cin; a.ncg = pc.ncg;
  a.dw_act = op.dw_act; a.act = op.act;
  a.dw_S = op.dw->dw_l1; a.dw_B = op.dw->dw_bmax;
  if (a.n_tiles == 0) return;
  const int grid = std::min(a.n_tiles, cap > 0 ? cap : th == 8 ? DP_SLOTS8 : DP_SLOTS);
  if (op.fin) {
    a.fin_w = op.fin_w->w.as<float>(); a.fin_b = op.fin_w->b.as<float>();
    a.fin_out = static_cast<float*>(op.fin_out.ptr);
    a.fin_cs = op.fin_out.cs; a.fin_coff = op.fin_out.coff; a.nc = op.fin->cout;
    a.fin_bytes = (unsigned)(lv->total_px * op.fin_out.cs * 4);
    if (th == 16) hipLaunchKernelGGL((conv_dwpw_kernel<true, 16>), dim3(grid), dim3(256), DpGeo<16>::LDS, st, a);
    else hipLaunchKernelGGL((conv_dwpw_kernel<true, 8>), dim3(grid), dim3(256), DpGeo<8>::LDS, st, a);
  } else {
    a.out = static_cast<float*>(op.out.ptr);
    a.out_cs = op.out.cs; a.out_coff = op.out.coff;
    a.out_bytes = (unsigned)(lv->total_px * op.out.cs * 4);
    a.amax_out = op.out.amax;
    if (th == 16) hipLaunchKernelGGL((conv_dwpw_kernel<false, 16>), dim3(grid), dim3(256), DpGeo<16>::LDS, st, a);
    else hipLaunchKernelGGL((conv_dwpw_kernel<false, 8>), dim3(grid), dim3(256), DpGeo<8>::LDS, st, a);
  }
}

}  // namespace ffp
