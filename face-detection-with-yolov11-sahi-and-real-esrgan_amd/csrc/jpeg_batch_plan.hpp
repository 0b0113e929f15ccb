// jpeg_batch_plan.hpp — where everything of a BATCH of JPEG decodes lives (jpeg_huff.hip / jpeg.hip, jpeg_decode_batch_to_device): plain C++,
// no HIP, because every number here is computed from the headers of untrusted files and is checked on the CPU under sanitizers
// (csrc/jpeg_batch_plan_host_check.cpp, tests/test_jpeg_batch_host.py). A single file (ffp_jpeg_decode*) is a batch of one, so this is also
// the only place where the buffers of a frame's decode are sized.
//
// A batch is cut into SUB-BATCHES of consecutive eligible files; one sub-batch is one launch sequence. Inside a sub-batch every file owns
//   * whole workgroups of the subsequence kernels (jh_sync / jh_write): [wg0, wg0 + n_wg), n_wg = ceil(t_cap / NT),
//   * whole unstuffing tiles: [tile0, tile0 + n_tiles),
//   * its own ranges of three arenas: `up` (what goes up in ONE copy: descriptors, the workgroup -> file and tile -> file tables, the
//     reconstruction tables, quantisation tables, Huffman table specs, the entropy-coded bytes), `work` (everything the kernels hand to
//     each other, the sample planes, the scalars) and `coef` (the coefficient planes: ONE memset clears them).
// No two files share a workgroup, a tile or a byte, so no decoder state can travel from one file into the next.
#pragma once
#include <cstddef>
#include <vector>

namespace ffp {
namespace jbp {

constexpr int SUB_BITS = 512, NT = 128, TILE = 1024;              // jpeg_huff.hip asserts that these are its own
constexpr int LDS_WORDS = NT * SUB_BITS / 32 + 8;
constexpr long long CLEAN_PAD = (long long)LDS_WORDS * 4 + 64;    // zeros behind a file's clean stream: the decoders look ahead
constexpr long long STREAM_LIMIT = 1ll << 28;                     // 32-bit bit offsets: a sub-batch's streams stay below 256 MiB
constexpr long long COEF_LIMIT = 1ll << 30;                       // bytes of coefficient planes per sub-batch
constexpr int IDCT_BLOCKS = 8, PX_THREADS = 64;                   // blocks per workgroup of the IDCT, pixels per workgroup of the colour stage
constexpr long long ALIGN = 256;

struct Sizes { long long desc, idct, colour, tab, spec, scal; };  // sizeof of the device structs (the planner does not see them)

struct FileIn {                                                   // from one parsed header
  long long n_raw = 0;                                            // bytes from the first entropy-coded byte to the end of the file
  int h = 0, w = 0, ncomp = 0, dri = 0;
  int hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, blocks_x[3] = {0, 0, 0}, blocks_y[3] = {0, 0, 0};
};

struct Range { long long off = 0, bytes = 0; };

struct FilePlan {
  int sub = -1;                                                   // sub-batch, -1: outside the device decoder's limits (host decoder)
  int slot = 0;                                                   // index inside the sub-batch
  int bpm = 0, mcus_x = 0, total_mcus = 0, n_seg_expected = 0, seg_cap = 0, t_cap = 0;
  int wg0 = 0, n_wg = 0, tile0 = 0, n_tiles = 0;
  int idct_wg0[3] = {0, 0, 0}, idct_n_wg[3] = {0, 0, 0}, idct_slot0 = 0, px_wg0 = 0, px_wgs_x = 0, px_n_wg = 0;
  Range raw;                                                      // `up`
  Range clean, tile_cnt, tmp, seg_start, first_sub, sub_start, sub_seg, entry, exit_, cnt, pref, tabs, scal, plane[3];   // `work`
  Range coef[3];                                                  // `coef`
};

struct SubPlan {
  std::vector<int> files;                                         // indices into the batch, ascending
  int n_wg = 0, n_tiles = 0, n_idct_wg = 0, n_idct = 0, n_px_wg = 0;
  Range desc, wg_file, tile_file, idct, colour, qt, spec;         // `up`: the tables
  long long up_bytes = 0, work_bytes = 0, coef_bytes = 0, stream_bytes = 0;
  Range scal;                                                     // `work`: the files' scalars, one array (ONE download)
};

struct Plan { std::vector<FilePlan> files; std::vector<SubPlan> subs; };

inline long long align_up(long long v, long long a = ALIGN) { return (v + a - 1) / a * a; }

// geometry of one file; false: not for the device decoder
inline bool plan_file(const FileIn& f, FilePlan& p) {
  if (f.n_raw <= 0 || f.n_raw >= STREAM_LIMIT || align_up(f.n_raw + CLEAN_PAD) >= STREAM_LIMIT) return false;
  if (f.ncomp != 1 && f.ncomp != 3) return false;
  if (f.h <= 0 || f.w <= 0 || f.h > 65535 || f.w > 65535 || f.dri < 0 || f.dri > 65535) return false;
  long long bpm = 0, coef = 0;
  for (int c = 0; c < f.ncomp; ++c) {
    if (f.hs[c] < 1 || f.hs[c] > 4 || f.vs[c] < 1 || f.vs[c] > 4) return false;
    if (f.blocks_x[c] <= 0 || f.blocks_y[c] <= 0 || f.blocks_x[c] > 8192 * 4 || f.blocks_y[c] > 8192 * 4) return false;
    if (f.blocks_x[c] % f.hs[c] || f.blocks_y[c] % f.vs[c]) return false;
    bpm += (long long)f.hs[c] * f.vs[c];
    coef += align_up((long long)f.blocks_x[c] * f.blocks_y[c] * 128);
  }
  if (bpm > 6 || coef > COEF_LIMIT) return false;
  int hmax = 1, vmax = 1;
  for (int c = 0; c < f.ncomp; ++c) { hmax = f.hs[c] > hmax ? f.hs[c] : hmax; vmax = f.vs[c] > vmax ? f.vs[c] : vmax; }
  for (int c = 0; c < f.ncomp; ++c)                               // the planes cover the image: the colour stage reads them by pixel
    if ((long long)f.blocks_x[c] * 8 * hmax < (long long)f.w * f.hs[c] || (long long)f.blocks_y[c] * 8 * vmax < (long long)f.h * f.vs[c]) return false;
  const long long mcus_x = f.blocks_x[0] / f.hs[0], mcus_y = f.blocks_y[0] / f.vs[0];
  for (int c = 1; c < f.ncomp; ++c)
    if (f.blocks_x[c] / f.hs[c] != mcus_x || f.blocks_y[c] / f.vs[c] != mcus_y) return false;
  const long long total = mcus_x * mcus_y;
  const long long n_seg = f.dri ? (total + f.dri - 1) / f.dri : 1;
  if (n_seg > f.n_raw / 2 + 1) return false;                      // every restart marker is two bytes: fewer cannot be a whole file
  p.bpm = (int)bpm; p.mcus_x = (int)mcus_x; p.total_mcus = (int)total;
  p.n_seg_expected = (int)n_seg; p.seg_cap = (int)n_seg + 1;
  p.t_cap = (int)((f.n_raw * 8 + SUB_BITS - 1) / SUB_BITS + n_seg + 1);
  p.n_wg = (p.t_cap + NT - 1) / NT;
  p.n_tiles = (int)((f.n_raw + TILE - 1) / TILE);
  return true;
}

inline Plan plan_batch(const FileIn* in, const unsigned char* readable, int n, const Sizes& sz) {
  Plan P;
  P.files.resize((size_t)(n > 0 ? n : 0));
  long long stream = 0, coef = 0;
  for (int i = 0; i < n; ++i) {
    FilePlan& p = P.files[(size_t)i];
    if ((readable && !readable[i]) || !plan_file(in[i], p)) { p = FilePlan(); continue; }
    long long fc = 0;
    for (int c = 0; c < in[i].ncomp; ++c) fc += align_up((long long)in[i].blocks_x[c] * in[i].blocks_y[c] * 128);
    const long long fs = align_up(in[i].n_raw + CLEAN_PAD);
    if (P.subs.empty() || stream + fs >= STREAM_LIMIT || coef + fc > COEF_LIMIT) { P.subs.emplace_back(); stream = 0; coef = 0; }
    stream += fs; coef += fc;
    p.sub = (int)P.subs.size() - 1;
    p.slot = (int)P.subs.back().files.size();
    P.subs.back().files.push_back(i);
  }
  for (SubPlan& S : P.subs) {
    const long long m = (long long)S.files.size();
    // counts first: the tables in front of `up` are sized by them
    for (int i : S.files) {
      FilePlan& p = P.files[(size_t)i];
      const FileIn& f = in[i];
      p.wg0 = S.n_wg; S.n_wg += p.n_wg;
      p.tile0 = S.n_tiles; S.n_tiles += p.n_tiles;
      p.idct_slot0 = S.n_idct;
      for (int c = 0; c < f.ncomp; ++c) {
        p.idct_wg0[c] = S.n_idct_wg;
        p.idct_n_wg[c] = (int)(((long long)f.blocks_x[c] * f.blocks_y[c] + IDCT_BLOCKS - 1) / IDCT_BLOCKS);
        S.n_idct_wg += p.idct_n_wg[c];
        ++S.n_idct;
      }
      p.px_wg0 = S.n_px_wg;
      p.px_wgs_x = (f.w + PX_THREADS - 1) / PX_THREADS;
      p.px_n_wg = p.px_wgs_x * f.h;
      S.n_px_wg += p.px_n_wg;
    }
    long long up = 0, work = 0, cf = 0;
    auto take = [](long long& pos, long long bytes) { Range r; r.off = pos; r.bytes = bytes; pos = align_up(pos + bytes); return r; };
    S.desc = take(up, sz.desc * m);
    S.wg_file = take(up, 4ll * S.n_wg);
    S.tile_file = take(up, 4ll * S.n_tiles);
    S.idct = take(up, sz.idct * S.n_idct);
    S.colour = take(up, sz.colour * m);
    S.qt = take(up, 2ll * 64 * 4 * m);
    S.spec = take(up, sz.spec * 6 * m);
    S.scal = take(work, sz.scal * m);
    for (int i : S.files) {
      FilePlan& p = P.files[(size_t)i];
      const FileIn& f = in[i];
      p.raw = take(up, f.n_raw + 16);
      p.scal.off = S.scal.off + sz.scal * p.slot; p.scal.bytes = sz.scal;
      p.clean = take(work, f.n_raw + CLEAN_PAD);
      p.tile_cnt = take(work, 8ll * (p.n_tiles + 1));
      p.tmp = take(work, 8ll * (p.seg_cap + 1));
      p.seg_start = take(work, 4ll * (p.seg_cap + 2));
      p.first_sub = take(work, 4ll * (p.seg_cap + 2));
      p.sub_start = take(work, 4ll * p.t_cap);
      p.sub_seg = take(work, 4ll * p.t_cap);
      p.entry = take(work, 8ll * p.t_cap);
      p.exit_ = take(work, 8ll * p.t_cap);
      p.cnt = take(work, 16ll * p.t_cap);
      p.pref = take(work, 16ll * p.t_cap);
      p.tabs = take(work, sz.tab * 6);
      for (int c = 0; c < f.ncomp; ++c) {
        const long long nb = (long long)f.blocks_x[c] * f.blocks_y[c];
        p.plane[c] = take(work, nb * 64 + 16);
        p.coef[c] = take(cf, nb * 128);
      }
      S.stream_bytes += align_up(f.n_raw + CLEAN_PAD);
    }
    S.up_bytes = up; S.work_bytes = work; S.coef_bytes = cf;
  }
  return P;
}

}  // namespace jbp
}  // namespace ffp
