// conv_rows16pc.hip — conv_rows16_kernel with the work of a workgroup split by ROLE: four producer waves own the global -> LDS
// staging and the epilogues, four consumer waves only read fragments and issue MFMAs. One 8-wave workgroup per CU.
//
// Why (round-3 probes of conv_rows16_kernel, profiles/r03_rows16_phase_probe.txt, r03_rows16_in_kernel_stamps.txt): with everything in
// one instruction stream per wave, MFMA-only takes 23 us, staging-only 26 us and the full kernel 44 us — the two do not overlap; a chunk
// of 1,152 MFMA cycles costs a wave ~215 cycles of exposed first fragment reads, ~2,000 of MFMA stream (its own staging waits and the
// partner wave's MFMAs inside), 480-690 of epilogue + item set-up and ~150 of barrier. Neither more prefetch distance, nor fewer bytes
// (weights resident: 0.76-0.89x), nor priorities moved it: one in-order wave cannot keep the matrix pipe fed beside its own staging,
// epilogue and set-up. Here every SIMD hosts ONE consumer wave, whose stream is fragment reads + 72 MFMAs per chunk and nothing else,
// and ONE producer wave with a load counter of its own, whose VALU / LDS / memory work fills the issue slots the MFMAs leave:
//   * producers: the staging of conv_rows16_kernel unchanged (21 input + 18 weight wave-pieces per chunk over four waves, raw buffer
//     loads, out-of-image lanes read zeros, two register sets = three chunks of prefetch distance), written into the other LDS stage
//     while the consumers multiply the current one;
//   * consumers: the MFMA stream of conv_rows16_kernel unchanged (same fragments, same order: results are bit-identical); at the end
//     of an item a consumer wave writes its 32 accumulator registers to an 8 KiB exchange block in LDS (8 ds_write_b128) and starts
//     the next item from the bias;
//   * the producer wave paired with it picks the block up after the chunk's barrier and runs the register epilogue (activation,
//     residuals, fp16 conversion, 16-byte stores) while the consumers are already multiplying the next item;
//   * one s_barrier per chunk for all eight waves, as before: the roles advance in lockstep, chunk time = the consumers' 1,152 MFMA
//     cycles + first fragment reads + barrier as long as the producers keep up (they have ~300 issue cycles of work per chunk).
// LDS: two 39 KiB stages + 32 KiB of exchange blocks + descriptors = 112 KiB.
// MEASURED (round 3, profiles/r03_rows16_role_split_probe.txt): bit-identical, and 0.73-0.94x the speed of conv_rows16_kernel — the
// hypothesis above is wrong, or incomplete: with the LDS bytes per MFMA unchanged (0.5 KiB of fragment reads + 0.135 KiB of staging
// writes) a CU with ONE tile in flight is slower than a CU with two whatever the wave roles are. What remains untested is the other
// half of the idea: consumers with 8 rows each (0.33 KiB of reads per MFMA) fed by LDS-DMA producers (no ds_write_b128 on the shared
// VGPR -> LDS path). Kept behind SHAPE_ROWS16PC / FFP_ROWS16_PC=1 as the starting point for that.
#include <algorithm>
#include <cstdlib>

#include "rows16_parts.hpp"

namespace ffp {

namespace {

struct PCGeo : R16Geo {                                       // conv_rows16_kernel's stages, then
  static constexpr int DUMP = 2 * STAGE;                      // four exchange blocks of 8 KiB: [consumer wave][row i][M-tile m][lane] x 16 B
  static constexpr int DUMP_W = 8192;
  static constexpr int DESC = DUMP + 4 * DUMP_W;
  static constexpr int LDS = DESC + TCAP * 48;                // 114560
};

template <int NS>              // staging register sets of a producer wave = chunks in flight ahead of the one being written (even)
__global__ void __launch_bounds__(512, 2) conv_rows16pc_kernel(const ConvArgs a) {
  using G = PCGeo;
  constexpr int NP = G::NP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave8 >= 4;                    // waves w and w + 4 share a SIMD (dispatch order 0 -> 2 -> 1 -> 3, twice)
  const int wave = wave8 & 3;
  const int pc = lane & 15, g = lane >> 4;

  const R16Deal deal = r16_deal(a, G::TCAP);           // conv_rows16_kernel's dealing
  const int J = deal.J;
  if (J == 0) return;                                  // whole workgroup: no barrier is skipped by part of it
  const int nt0 = deal.first % a.n_nblk;

  int4* desc = reinterpret_cast<int4*>(smem + G::DESC);
  r16_fill_desc(desc, a, deal, tid);

  auto sgpr = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
  const int NC = a.cin >> 5;
  const int Q = J * NC;                                // chunks of this workgroup: both roles run exactly Q iterations, one barrier each
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(a.wpk) + (long long)nt0 * NC * G::W_BYTES;
  const auto rs_w = buf_rsrc(wb);
  unsigned char* dump = smem + G::DUMP + wave * G::DUMP_W + lane * 16;       // this wave pair's exchange block

  if (producer) {
    // ================================================= producer: staging + epilogues ==================================================
    auto rs_in = rs_w;
    auto rs_wp = rs_w;
    const bool s9_in = wave == 0;
    unsigned isrc[6], idst[6], wrel[5], hyx[6];
    r16_stage_tables(wave, lane, idst, hyx, wrel);

    int pf_item = 0, pf_c = 0;
    uint4 sets[NS][NP];
    auto piece_fetch = [&](int p, uint4& r) { r16_piece_fetch(p, r, rs_in, rs_wp, isrc, wrel, pf_c, s9_in); };
    auto piece_stash = [&](unsigned char* sb, int p, const uint4& r) { r16_piece_stash(sb, p, r, idst, wrel, s9_in); };
    auto advance_pf = [&]() { r16_advance_pf(a, desc, J, NC, wb, pf_item, pf_c, hyx, isrc, rs_in, rs_wp); };
    auto fetch_all = [&](uint4 (&q)[NP]) {
#pragma unroll
      for (int p = 0; p < NP; ++p) piece_fetch(p, q[p]);
      advance_pf();
    };
    // the chunk in `set` goes to stage sb; each register is re-requested for the chunk two further on right after its write
    auto restage = [&](unsigned char* sb, uint4 (&set)[NP]) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        piece_stash(sb, p, set[p]);
        piece_fetch(p, set[p]);
      }
      advance_pf();
    };

    // ---- epilogue of item j from the exchange block: lane (pc, g) holds channels 8g..8g+7 of pixel (row 4*wave + i, column pc) ------------
    auto epilogue = [&](int j) {
      f32x4 acc[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[i][m] = *reinterpret_cast<const f32x4*>(dump + ((i * 2 + m) << 10));
      const int4 t = desc[j * 3], ot = desc[j * 3 + 2];
      const int oy0 = sgpr(t.y), ox0 = sgpr(t.z), Ho = sgpr(ot.y), Wo = sgpr(ot.z);
      const long long out_base = sgpr(ot.x);
      const unsigned char* r1b = a.res1 ? reinterpret_cast<const unsigned char*>(a.res1) + (out_base * a.r1_cs + a.r1_coff) * 2 : wb;
      const unsigned char* r2b = a.res2 ? reinterpret_cast<const unsigned char*>(a.res2) + (out_base * a.r2_cs + a.r2_coff) * 2 : wb;
      unsigned char* ob = reinterpret_cast<unsigned char*>(a.out) + (out_base * a.out_cs + a.out_coff) * 2;
      const auto rs_r1 = buf_rsrc(r1b), rs_r2 = buf_rsrc(r2b), rs_o = buf_rsrc(ob);
      const int ox = ox0 + pc;
      const int ch0 = nt0 * 32 + 8 * g;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int oy = oy0 + 4 * wave + i;
        const bool ok = oy < Ho && ox < Wo;
        const unsigned rel_px = (unsigned)(oy * Wo + ox);
        uint4 r1v = make_uint4(0u, 0u, 0u, 0u), r2v = r1v;
        if (a.res1) r1v = buf_load16(rs_r1, ok ? (rel_px * a.r1_cs + ch0) * 2 : BUF_OOB);
        if (a.res2) r2v = buf_load16(rs_r2, ok ? (rel_px * a.r2_cs + ch0) * 2 : BUF_OOB);
        const u32x4 ov = r16_finish_px(acc[i][0], acc[i][1], a.act, a.res1 != nullptr, r1v, a.s1, a.res2 != nullptr, r2v, a.s2);
        __builtin_amdgcn_raw_buffer_store_b128(ov, rs_o, ok ? (rel_px * a.out_cs + ch0) * 2 : BUF_OOB, 0, 0);
      }
    };

    // ---- prologue: chunks 0 .. NS-1 requested (set c holds chunk c mod NS), chunk 0 into stage 0, its set re-requested for chunk NS -------
    r16_setup_pf(a, desc, 0, hyx, isrc, rs_in);
#pragma unroll
    for (int k = 0; k < NS; ++k) fetch_all(sets[k]);
#pragma unroll
    for (int p = 0; p < NP; ++p) piece_stash(smem, p, sets[0][p]);
    fetch_all(sets[0]);
    __syncthreads();
    int cc = 0, cj = 0;                                // the chunk the consumers multiply in this iteration
    for (int q0 = 0; q0 < Q; q0 += NS) {
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        if (q0 + k >= Q) break;
        // iteration q0 + k: stage k & 1 is being multiplied; set (k + 1) % NS holds chunk q0 + k + 1 -> the other stage; the item that
        // ended at the last barrier is stored
        restage(smem + ((k + 1) & 1) * G::STAGE, sets[(k + 1) % NS]);
        if (cc == 0 && cj > 0) epilogue(cj - 1);
        if (++cc == NC) { cc = 0; ++cj; }
        __syncthreads();
      }
    }
    epilogue(J - 1);                                   // the last item's sums were written before the last barrier
    return;
  }

  // ===================================================== consumer: fragment reads + MFMAs =====================================================
  const float4 bias0 = *reinterpret_cast<const float4*>(a.bias + nt0 * 32 + 8 * g);
  const float4 bias1 = *reinterpret_cast<const float4*>(a.bias + nt0 * 32 + 8 * g + 4);
  unsigned boff[3];
  r16_frag_offsets(4 * wave, pc, g, boff);
  const unsigned aoff = G::IN_BYTES + lane * 16;
  f32x4 acc[4][2];
  auto zero_acc = [&]() { r16_zero_acc(acc, bias0, bias1); };
  zero_acc();
  // one step = one tap: 2 weight fragments x 4 output rows = 8 MFMAs; weight fragments two steps, input-row fragments one kx ahead
  auto chunk = [&](const unsigned char* sb) {
    uint4 bq[2][6], aq[3][2];
    auto ldB = [&](int kx, int q) {
#pragma unroll
      for (int j = 0; j < 6; ++j) bq[q][j] = *reinterpret_cast<const uint4*>(sb + boff[kx] + j * 1152);
    };
    auto ldA = [&](int s, int q) {
      const int tap = (s % 3) * 3 + s / 3;
#pragma unroll
      for (int m = 0; m < 2; ++m) aq[q][m] = *reinterpret_cast<const uint4*>(sb + aoff + ((tap * 2 + m) << 10));
    };
    ldB(0, 0);
    ldA(0, 0);
    ldA(1, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const int kx = s / 3, ky = s - 3 * kx;
      if (s + 2 < 9) ldA(s + 2, (s + 2) % 3);
      if (ky == 0 && kx < 2) ldB(kx + 1, (kx + 1) & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          union { uint4 u; f16x8 h; } ua, ub;
          ua.u = aq[s % 3][m]; ub.u = bq[kx & 1][i + ky];
          acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ua.h, ub.h, acc[i][m], 0, 0, 0);
        }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x7F6, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto hand_over = [&]() {                             // the item's sums to the paired producer wave, the next item starts from the bias
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int m = 0; m < 2; ++m) *reinterpret_cast<f32x4*>(dump + ((i * 2 + m) << 10)) = acc[i][m];
    zero_acc();
  };
  __syncthreads();                                     // the producers' prologue: chunk 0 sits in stage 0
  int cc = 0;
  for (int q = 0; q < Q; q += 2) {
    chunk(smem);
    if (++cc == NC) { cc = 0; hand_over(); }
    __syncthreads();
    if (q + 1 >= Q) break;
    chunk(smem + G::STAGE);
    if (++cc == NC) { cc = 0; hand_over(); }
    __syncthreads();
  }
}

}  // namespace

void conv_rows16pc_init() {
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_rows16pc_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, PCGeo::LDS));
  FFP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_rows16pc_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, PCGeo::LDS));
}

// SHAPE_ROWS16PC, or every eligible layer with FFP_ROWS16_PC=1 (A/B aid; conv_route.cpp). NOT the default: measured 0.73-0.94x of conv_rows16_kernel
// (profiles/r03_rows16_role_split_probe.txt) — with the same LDS traffic per MFMA the role split only halves the tiles in flight per CU.

void launch_conv_rows16pc(ConvArgs& a, const PackedConv& pc, Level* out_lvl, hipStream_t st) {
  using G = PCGeo;
  a.wpk = pc.w16.p;
  int n_tiles = 0;
  a.tiles = out_lvl->tile_table(16, &n_tiles, &a.n_tiles_dev, st, a.gate);
  if (n_tiles == 0) return;
  a.ntiles_host = n_tiles;
  a.n_nblk = a.ntiles32;
  const unsigned grid = rows16_grid(n_tiles, a.n_nblk, 32, G::TCAP, "rows16pc");          // 8 x 32 workgroups: one per CU
  const int ns = sw().rows16_pc_sets;       // 4 sets (five chunks ahead) measured SLOWER than 2: 0.68-0.85x vs 0.78-0.95x of conv_rows16_kernel
  if (ns == 2) hipLaunchKernelGGL(conv_rows16pc_kernel<2>, dim3(grid), dim3(512), G::LDS, st, a);
  else hipLaunchKernelGGL(conv_rows16pc_kernel<4>, dim3(grid), dim3(512), G::LDS, st, a);
}

}  // namespace ffp
