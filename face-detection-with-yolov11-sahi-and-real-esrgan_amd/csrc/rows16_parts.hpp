// rows16_parts.hpp — the ONE copy of what conv_rows16_kernel (conv_rows16.hip), conv_rows16pc_kernel (conv_rows16pc.hip) and
// conv_trunk_kernel (conv_trunk.hip) have in common: geometry, item dealing and the register epilogue of a pixel for all three; the
// staging lane tables, the prefetch cursor, the fragment offsets and the bias start of the accumulators for the two opt-in kernels. The kernels are bit-identical because they run THIS text, not copies of it. Device-only; every function is a free
// __forceinline__ function over the caller's own registers (wrapping the lane tables in a struct, or passing kernel arguments by value,
// changes hipcc's register allocation). conv_rows16_kernel still carries its own text of the second group: there even the free-function
// form moves the shipped kernel's instruction stream (profiles/rows16_shared_parts_ab.txt), which has to be timed before it may change.
#pragma once
#include "conv_args.hpp"

namespace ffp {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct R16Geo {
  static constexpr int IN_PX = 336;                           // 18 x 18 halo pixels + 12 dummies: 21 whole wave-pieces of 64 vectors
  static constexpr int IN_BYTES = IN_PX * 64;                 // 21504
  static constexpr int W_BYTES = 9 * 2 * 1024;                // [tap][M-tile][lane] : 18 wave-pieces
  static constexpr int STAGE = IN_BYTES + W_BYTES;            // 39936
  static constexpr int NP = 10;                               // wave-pieces per wave and chunk: 5 input, 4 weight, 1 mixed (see r16_piece_fetch)
  static constexpr int TCAP = 40;                             // work items one workgroup walks (descriptor table in LDS)
};

// ---- this workgroup's items: logical ids first + j * Ws, j < J ---------------------------------------------------------------------
// Items are dealt so that each XCD (workgroups b, b + 8, ... share one) gets a contiguous run of logical ids (pixel tile x
// 32-channel block) and the workgroups of an XCD take consecutive ids at the same time: the channel blocks of a pixel tile
// and neighbouring tiles meet in that XCD's L2. The mapping only affects speed.
struct R16Deal {
  int first, J, Ws;
};
__device__ __forceinline__ R16Deal r16_deal(const ConvArgs& a, int tcap) {       // (blockIdx.x and gridDim.x are read here, after the kernel arguments, as the kernels always did)
  const int n_items = (a.n_tiles_dev ? __builtin_amdgcn_readfirstlane(*a.n_tiles_dev) : a.ntiles_host) * a.n_nblk;
  R16Deal d;
  d.Ws = (int)gridDim.x >> 3;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  int per_xcd = (n_items + 7) >> 3;
  per_xcd = (per_xcd + a.n_nblk - 1) / a.n_nblk * a.n_nblk;
  d.first = xcd * per_xcd + slot;
  const int last = min(n_items, (xcd + 1) * per_xcd);
  d.J = d.first < last ? min((last - d.first + d.Ws - 1) / d.Ws, tcap) : 0;      // the launcher sizes Ws so that J <= TCAP (rows16_grid)
  return d;
}
// int4 x 3 per item: tile {img, y0, x0}, input {base, h, w}, output {base, h, w}; visible to the workgroup after the barrier
__device__ __forceinline__ void r16_fill_desc(int4* desc, const ConvArgs& a, const R16Deal& d, int tid) {
  if (tid < d.J) {
    const int4 t = a.tiles[(d.first + tid * d.Ws) / a.n_nblk];
    desc[tid * 3] = t;
    desc[tid * 3 + 1] = a.in_tab[t.x];
    desc[tid * 3 + 2] = a.out_tab[t.x];
  }
  __syncthreads();
}

// ---- staging: a chunk = 21 input + 18 weight wave-pieces (64 lanes x 16 bytes); wave w stages, in its NP slots,
//   slots 0..4: input pieces w, w+4, .., w+16; slots 5..8: weight pieces w, w+4, w+8, w+12;
//   slot 9: wave 0 input piece 20, wave 1 / 2 weight pieces 16 / 17, wave 3 weight piece 17 again (same bytes to the same place)
// so every slot is a whole wave-instruction for every wave: no divergence, no validity tests in the pipeline.
//   idst: LDS byte offset of the slot's vector inside the stage (item independent)
//   hyx:  the slot's halo pixel and vector slot (slot << 16 | row << 8 | column): item independent, so that an item's set-up is adds and compares
//   wrel: weight pieces: byte offset inside a chunk's 18 KiB, also the LDS offset behind IN_BYTES
// weights in global memory: [32-channel tile][chunk][tap][M-tile][lane] — a chunk's 18 KiB are laid out like the LDS stage, so one
// per-lane offset serves the load (chunk offset as the instruction's scalar operand) and the LDS write
__device__ __forceinline__ void r16_stage_tables(int wave, int lane, unsigned (&idst)[6], unsigned (&hyx)[6], unsigned (&wrel)[5]) {
  const int s9_piece = wave == 0 ? 20 : wave == 1 ? 16 : 17;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int idx = (i < 5 ? wave + 4 * i : 20) * 64 + lane;
    const int px = idx >> 2, s = idx & 3;
    const int hy = px / 18, hx = px - hy * 18;
    idst[i] = (unsigned)(px * 64 + ((s ^ ((hx >> 1) & 2)) << 4));
    hyx[i] = px < 324 ? (unsigned)((s << 16) | (hy << 8) | hx) : (unsigned)((s << 16) | 0xFFFF);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) wrel[i] = (unsigned)(((i < 4 ? wave + 4 * i : s9_piece) * 64 + lane) * 16);
}

// the prefetch cursor moves to item j: its input resource and, per slot, isrc = byte offset of (pixel, slot) from the item's image base; OOB: zeros
__device__ __forceinline__ void r16_setup_pf(const ConvArgs& a, const int4* desc, int j, const unsigned (&hyx)[6], unsigned (&isrc)[6], buf_rsrc_t& rs_in) {
  const int4 t = desc[j * 3], it = desc[j * 3 + 1];
  const int oy0 = __builtin_amdgcn_readfirstlane(t.y), ox0 = __builtin_amdgcn_readfirstlane(t.z);
  const int Hi = __builtin_amdgcn_readfirstlane(it.y), Wi = __builtin_amdgcn_readfirstlane(it.z);
  const int Hv = Hi << a.up, Wv = Wi << a.up;
  const unsigned char* inb = reinterpret_cast<const unsigned char*>(a.in) + ((long long)__builtin_amdgcn_readfirstlane(it.x) * a.in_cs + a.in_coff) * 2;
  rs_in = buf_rsrc(inb);
#pragma unroll
  for (int i = 0; i < 6; ++i) {                      // hyx[i]: fixed per lane; 0xFFFF: padding pixel
    const int hy = (int)(hyx[i] >> 8) & 0xFF, hx = (int)hyx[i] & 0xFF, sl = (int)(hyx[i] >> 16) & 3;
    const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
    const bool ok = (hyx[i] & 0xFFFFu) != 0xFFFFu && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
    isrc[i] = ok ? (unsigned)(((iy >> a.up) * Wi + (ix >> a.up)) * a.in_cs * 2 + sl * 16) : BUF_OOB;
  }
}
// slot p of chunk pf_c of the prefetch cursor's item -> r
__device__ __forceinline__ void r16_piece_fetch(int p, uint4& r, buf_rsrc_t rs_in, buf_rsrc_t rs_wp, const unsigned (&isrc)[6], const unsigned (&wrel)[5], int pf_c, bool s9_in) {
  if (p < 5) {
    r = buf_load16(rs_in, isrc[p] != BUF_OOB ? isrc[p] + (unsigned)(pf_c * 64) : BUF_OOB);
  } else if (p < 9) {
    r = buf_load16(rs_wp, wrel[p - 5], pf_c * R16Geo::W_BYTES);
  } else {                                           // the mixed slot: wave-uniform choice, no branch
    const unsigned oi = isrc[5] != BUF_OOB ? isrc[5] + (unsigned)(pf_c * 64) : BUF_OOB;
    r = buf_load16(s9_in ? rs_in : rs_wp, s9_in ? oi : wrel[4], s9_in ? 0 : pf_c * R16Geo::W_BYTES);
  }
}
// slot p in r -> the LDS stage at sb
__device__ __forceinline__ void r16_piece_stash(unsigned char* sb, int p, const uint4& r, const unsigned (&idst)[6], const unsigned (&wrel)[5], bool s9_in) {
  if (p < 5) *reinterpret_cast<uint4*>(sb + idst[p]) = r;
  else if (p < 9) *reinterpret_cast<uint4*>(sb + R16Geo::IN_BYTES + wrel[p - 5]) = r;
  else *reinterpret_cast<uint4*>(sb + (s9_in ? idst[5] : R16Geo::IN_BYTES + wrel[4])) = r;
}
// after the last piece of a chunk has been requested: next chunk, next item, or the end of the stream (wb: the weights, any valid base)
__device__ __forceinline__ void r16_advance_pf(const ConvArgs& a, const int4* desc, int J, int NC, const unsigned char* wb, int& pf_item, int& pf_c,
                                               const unsigned (&hyx)[6], unsigned (&isrc)[6], buf_rsrc_t& rs_in, buf_rsrc_t& rs_wp) {
  if (pf_item >= J) return;
  if (++pf_c == NC) {
    pf_c = 0;
    if (++pf_item < J) {
      r16_setup_pf(a, desc, pf_item, hyx, isrc, rs_in);
    } else {                                         // stream exhausted: every later request is out of range (zeros, no traffic)
      rs_in = buf_rsrc(wb, 0);
      rs_wp = rs_in;
    }
  }
}

// ---- fragment read offsets: halo rows row0 + j, column pc + kx, slot g (per kx, for halo row row0; rows are 18 * 64 = 1152 bytes apart)
__device__ __forceinline__ void r16_frag_offsets(int row0, int pc, int g, unsigned (&boff)[3]) {
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int hx = pc + kx;
    boff[kx] = (unsigned)((row0 * 18 + hx) * 64 + ((g ^ ((hx >> 1) & 2)) << 4));
  }
}
// accumulation starts from the bias: nothing to add in the epilogue
template <int ROWS> __device__ __forceinline__ void r16_zero_acc(f32x4 (&acc)[ROWS][2], const float4& bias0, const float4& bias1) {
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    acc[i][0] = f32x4{bias0.x, bias0.y, bias0.z, bias0.w};
    acc[i][1] = f32x4{bias1.x, bias1.y, bias1.z, bias1.w};
  }
}

// ---- register epilogue of one pixel: the lane's 8 consecutive channels (two accumulators) -> activation -> v * s1 + res1 -> v * s2 + res2 -> 8 x fp16
// A deliberately cheaper subset of the ConvOp contract (ops.hpp), bias already in the sums: LReLU as max(x, 0.2 x), SiLU, none — no ReLU arm
// and no act_post (either would add to the shipped kernels' instruction stream). kEpiR16 says exactly that, and conv_rows16_eligible /
// conv_trunk_layer_ok start from it: an op outside it runs on conv_rows_kernel or the generic kernel.
constexpr EpiCaps kEpiR16{1u << ACT_NONE | 1u << ACT_SILU | 1u << ACT_LRELU, true, false, true, false};
template <class R> __device__ __forceinline__ u32x4 r16_finish_px(const f32x4& acc0, const f32x4& acc1, int act, bool has1, const R& r1v, float s1, bool has2, const R& r2v, float s2) {
  float v[8];
  v[0] = acc0[0]; v[1] = acc0[1]; v[2] = acc0[2]; v[3] = acc0[3];
  v[4] = acc1[0]; v[5] = acc1[1]; v[6] = acc1[2]; v[7] = acc1[3];
  if (act == ACT_LRELU) {                            // max(x, 0.2 x): two VALU ops per value
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q], v[q] * 0.2f);
  } else if (act == ACT_SILU) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = apply_act(v[q], ACT_SILU);
  }
  if (has1) {
    const _Float16* r = reinterpret_cast<const _Float16*>(&r1v);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = v[q] * s1 + (float)r[q];
  }
  if (has2) {
    const _Float16* r = reinterpret_cast<const _Float16*>(&r2v);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = v[q] * s2 + (float)r[q];
  }
  union { u32x4 u; _Float16 h[8]; } ov;
#pragma unroll
  for (int q = 0; q < 8; ++q) ov.h[q] = (_Float16)v[q];
  return ov.u;
}

}  // namespace

}  // namespace ffp
