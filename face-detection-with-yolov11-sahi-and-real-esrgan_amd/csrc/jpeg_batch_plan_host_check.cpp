// jpeg_batch_plan_host_check.cpp — the layout of a batch of JPEG decodes (jpeg_batch_plan.hpp, plain C++) on the CPU, built with the host
// compiler under AddressSanitizer + UBSan (build.py --jpeg-batch-plan-check) and run by tests/test_jpeg_batch_host.py. Seeded sets of headers,
// as an untrusted file could claim them, go through plan_batch(); every workgroup and tile range, every range of the three arenas and
// every capacity the kernels rely on is checked to be in bounds and disjoint, the tables are filled the way the host code fills them (so
// that an index past a table is the sanitizer's to find), and the sub-batches must cover every eligible file exactly once.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "jpeg_batch_plan.hpp"

using namespace ffp::jbp;

namespace {

int g_fail = 0;
#define EXPECT(cond, ...)                                      \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                \
      std::printf("\n");                                       \
      if (++g_fail > 20) std::exit(1);                         \
    }                                                          \
  } while (0)

const Sizes kSizes{328, 40, 88, 2448, 272, 32};               // the device structs' sizes today; any positive numbers must do

FileIn image(int h, int w, int ncomp, int hsub, int vsub, int dri, long long n_raw) {
  FileIn f;
  f.h = h; f.w = w; f.ncomp = ncomp; f.dri = dri; f.n_raw = n_raw;
  const int mx = (w + 8 * hsub - 1) / (8 * hsub), my = (h + 8 * vsub - 1) / (8 * vsub);
  for (int c = 0; c < ncomp; ++c) {
    f.hs[c] = c == 0 ? hsub : 1; f.vs[c] = c == 0 ? vsub : 1;
    f.blocks_x[c] = mx * f.hs[c]; f.blocks_y[c] = my * f.vs[c];
  }
  return f;
}

struct Span { long long off, bytes; const char* what; int file; };
void check_disjoint(std::vector<Span>& v, long long total, const char* arena) {
  std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.off < b.off; });
  long long end = 0;
  for (const Span& s : v) {
    EXPECT(s.off >= end && s.bytes >= 0 && s.off % ALIGN == 0, "%s: %s of file %d at %lld (+%lld) overlaps what ends at %lld", arena, s.what, s.file, s.off, s.bytes, end);
    end = s.off + s.bytes;
  }
  EXPECT(end <= total, "%s: ranges end at %lld, arena has %lld", arena, end, total);
}

// returns the number of sub-batches
int check(const std::vector<FileIn>& in, const std::vector<unsigned char>* readable, const char* name) {
  const int n = (int)in.size();
  const Plan P = plan_batch(in.data(), readable ? readable->data() : nullptr, n, kSizes);
  EXPECT((int)P.files.size() == n, "%s: %zu plans for %d files", name, P.files.size(), n);
  std::vector<int> seen((size_t)n, 0);
  int prev_last = -1;
  for (size_t si = 0; si < P.subs.size(); ++si) {
    const SubPlan& S = P.subs[si];
    EXPECT(!S.files.empty(), "%s: empty sub-batch", name);
    EXPECT(S.stream_bytes < STREAM_LIMIT && S.coef_bytes <= COEF_LIMIT, "%s: sub-batch %zu holds %lld stream / %lld coefficient bytes", name, si, S.stream_bytes, S.coef_bytes);
    std::vector<int> wg_file((size_t)S.n_wg, -1), tile_file((size_t)S.n_tiles, -1), idct_wg((size_t)S.n_idct_wg, -1), px_wg((size_t)S.n_px_wg, -1);
    std::vector<Span> up, work, coef;
    const long long m = (long long)S.files.size();
    up.push_back({S.desc.off, S.desc.bytes, "desc", -1}); up.push_back({S.wg_file.off, S.wg_file.bytes, "wg_file", -1});
    up.push_back({S.tile_file.off, S.tile_file.bytes, "tile_file", -1}); up.push_back({S.idct.off, S.idct.bytes, "idct", -1});
    up.push_back({S.colour.off, S.colour.bytes, "colour", -1}); up.push_back({S.qt.off, S.qt.bytes, "qt", -1}); up.push_back({S.spec.off, S.spec.bytes, "spec", -1});
    work.push_back({S.scal.off, S.scal.bytes, "scal", -1});
    EXPECT(S.desc.bytes >= kSizes.desc * m && S.wg_file.bytes >= 4ll * S.n_wg && S.tile_file.bytes >= 4ll * S.n_tiles && S.idct.bytes >= kSizes.idct * S.n_idct &&
               S.colour.bytes >= kSizes.colour * m && S.qt.bytes >= 512 * m && S.spec.bytes >= kSizes.spec * 6 * m && S.scal.bytes >= kSizes.scal * m,
           "%s: a table of sub-batch %zu is too small", name, si);
    int slot = 0, idct_slot = 0;
    for (int i : S.files) {
      EXPECT(i > prev_last && i < n, "%s: file order (%d after %d)", name, i, prev_last);
      prev_last = i;
      ++seen[(size_t)i];
      const FilePlan& p = P.files[(size_t)i];
      const FileIn& f = in[(size_t)i];
      EXPECT(p.sub == (int)si && p.slot == slot, "%s: file %d says sub %d slot %d, is %zu / %d", name, i, p.sub, p.slot, si, slot);
      ++slot;
      // workgroups and tiles: whole, consecutive, enough
      EXPECT(p.n_wg > 0 && (long long)p.n_wg * NT >= p.t_cap && p.wg0 >= 0 && p.wg0 + p.n_wg <= S.n_wg, "%s: file %d workgroups [%d, +%d) of %d", name, i, p.wg0, p.n_wg, S.n_wg);
      EXPECT(p.n_tiles > 0 && (long long)p.n_tiles * TILE >= f.n_raw && p.tile0 >= 0 && p.tile0 + p.n_tiles <= S.n_tiles, "%s: file %d tiles", name, i);
      for (int k = 0; k < p.n_wg; ++k) { EXPECT(wg_file[(size_t)(p.wg0 + k)] == -1, "%s: workgroup %d has two files", name, p.wg0 + k); wg_file[(size_t)(p.wg0 + k)] = slot; }
      for (int k = 0; k < p.n_tiles; ++k) { EXPECT(tile_file[(size_t)(p.tile0 + k)] == -1, "%s: tile %d has two files", name, p.tile0 + k); tile_file[(size_t)(p.tile0 + k)] = slot; }
      // the capacities the kernels rely on
      const long long n_seg = f.dri ? ((long long)p.total_mcus + f.dri - 1) / f.dri : 1;
      EXPECT(p.n_seg_expected == n_seg && p.seg_cap >= n_seg + 1, "%s: file %d segments", name, i);
      EXPECT(p.t_cap >= (f.n_raw * 8 + SUB_BITS - 1) / SUB_BITS + n_seg, "%s: file %d t_cap %d", name, i, p.t_cap);
      EXPECT(p.bpm >= 1 && p.bpm <= 6 && p.mcus_x >= 1 && p.total_mcus >= p.mcus_x, "%s: file %d MCU geometry", name, i);
      EXPECT(p.raw.bytes >= f.n_raw && p.clean.bytes >= f.n_raw + CLEAN_PAD, "%s: file %d stream capacity", name, i);
      EXPECT(p.tile_cnt.bytes >= 8ll * p.n_tiles && p.tmp.bytes >= 8ll * p.seg_cap && p.seg_start.bytes >= 4ll * (p.seg_cap + 1) && p.first_sub.bytes >= 4ll * (p.seg_cap + 1),
             "%s: file %d segment arrays", name, i);
      EXPECT(p.sub_start.bytes >= 4ll * p.t_cap && p.sub_seg.bytes >= 4ll * p.t_cap && p.entry.bytes >= 8ll * p.t_cap && p.exit_.bytes >= 8ll * p.t_cap &&
                 p.cnt.bytes >= 16ll * p.t_cap && p.pref.bytes >= 16ll * p.t_cap && p.tabs.bytes >= kSizes.tab * 6 && p.scal.bytes >= kSizes.scal,
             "%s: file %d subsequence arrays", name, i);
      EXPECT(p.scal.off >= S.scal.off && p.scal.off + p.scal.bytes <= S.scal.off + S.scal.bytes && (p.scal.off - S.scal.off) == kSizes.scal * p.slot, "%s: file %d scalars", name, i);
      up.push_back({p.raw.off, p.raw.bytes, "raw", i});
      const Range* wr[] = {&p.clean, &p.tile_cnt, &p.tmp, &p.seg_start, &p.first_sub, &p.sub_start, &p.sub_seg, &p.entry, &p.exit_, &p.cnt, &p.pref, &p.tabs};
      const char* wn[] = {"clean", "tile_cnt", "tmp", "seg_start", "first_sub", "sub_start", "sub_seg", "entry", "exit", "cnt", "pref", "tabs"};
      for (int k = 0; k < 12; ++k) work.push_back({wr[k]->off, wr[k]->bytes, wn[k], i});
      EXPECT(p.idct_slot0 == idct_slot, "%s: file %d IDCT slot", name, i);
      for (int c = 0; c < f.ncomp; ++c) {
        const long long nb = (long long)f.blocks_x[c] * f.blocks_y[c];
        EXPECT(p.plane[c].bytes >= nb * 64 + 8 && p.coef[c].bytes >= nb * 128, "%s: file %d planes of component %d", name, i, c);
        work.push_back({p.plane[c].off, p.plane[c].bytes, "plane", i});
        coef.push_back({p.coef[c].off, p.coef[c].bytes, "coef", i});
        EXPECT((long long)p.idct_n_wg[c] * IDCT_BLOCKS >= nb && p.idct_wg0[c] >= 0 && p.idct_wg0[c] + p.idct_n_wg[c] <= S.n_idct_wg, "%s: file %d IDCT workgroups", name, i);
        for (int k = 0; k < p.idct_n_wg[c]; ++k) { EXPECT(idct_wg[(size_t)(p.idct_wg0[c] + k)] == -1, "%s: IDCT workgroup twice", name); idct_wg[(size_t)(p.idct_wg0[c] + k)] = idct_slot; }
        ++idct_slot;
      }
      EXPECT((long long)p.px_wgs_x * PX_THREADS >= f.w && p.px_n_wg == p.px_wgs_x * f.h && p.px_wg0 >= 0 && p.px_wg0 + p.px_n_wg <= S.n_px_wg, "%s: file %d pixel workgroups", name, i);
      for (int k = 0; k < p.px_n_wg; k += std::max(1, p.px_n_wg / 64)) { EXPECT(px_wg[(size_t)(p.px_wg0 + k)] == -1, "%s: pixel workgroup twice", name); px_wg[(size_t)(p.px_wg0 + k)] = slot; }
      px_wg[(size_t)(p.px_wg0 + p.px_n_wg - 1)] = slot;
    }
    EXPECT(idct_slot == S.n_idct, "%s: %d IDCT descriptors, %d planned", name, idct_slot, S.n_idct);
    for (int v : wg_file) EXPECT(v != -1, "%s: a workgroup without a file", name);
    for (int v : tile_file) EXPECT(v != -1, "%s: a tile without a file", name);
    for (int v : idct_wg) EXPECT(v != -1, "%s: an IDCT workgroup without a component", name);
    check_disjoint(up, S.up_bytes, "up");
    check_disjoint(work, S.work_bytes, "work");
    check_disjoint(coef, S.coef_bytes, "coef");
  }
  for (int i = 0; i < n; ++i) {
    FilePlan q;
    const bool eligible = (!readable || (*readable)[(size_t)i]) && plan_file(in[(size_t)i], q);
    EXPECT(seen[(size_t)i] == (eligible ? 1 : 0) && (P.files[(size_t)i].sub >= 0) == eligible, "%s: file %d is in %d sub-batches (eligible: %d)", name, i, seen[(size_t)i], (int)eligible);
  }
  return (int)P.subs.size();
}

}  // namespace

int main() {
  // nothing at all
  EXPECT(check({}, nullptr, "empty") == 0, "empty batch");
  // the smallest images, every sampling, restart interval 1
  {
    std::vector<FileIn> v;
    for (int ncomp : {1, 3})
      for (int hsub : {1, 2})
        for (int vsub : {1, 2})
          for (int dri : {0, 1, 7}) v.push_back(image(1, 1, ncomp, ncomp == 1 ? 1 : hsub, ncomp == 1 ? 1 : vsub, dri, 3 + dri));
    EXPECT(check(v, nullptr, "1x1") == 1, "1x1 images are one sub-batch");
  }
  // the widest images a header can claim, one MCU row and many; restart interval 1 needs two bytes per marker
  {
    std::vector<FileIn> v;
    v.push_back(image(8, 65500, 3, 2, 2, 0, 4096));
    v.push_back(image(16, 65500, 3, 2, 2, 1, 4 * 4094 * 2));
    v.push_back(image(16, 65500, 3, 2, 2, 1, 100));             // claims more segments than its bytes can hold: host decoder
    v.push_back(image(65500, 65500, 3, 1, 1, 0, 1 << 20));      // planes beyond the sub-batch budget: host decoder
    v.push_back(image(65500, 8, 1, 1, 1, 1, 70000));
    v.push_back(image(2000, 65500, 1, 1, 1, 0, 1 << 16));
    check(v, nullptr, "65500");
    const Plan P = plan_batch(v.data(), nullptr, (int)v.size(), kSizes);
    EXPECT(P.files[0].sub >= 0 && P.files[1].sub >= 0 && P.files[2].sub < 0 && P.files[3].sub < 0 && P.files[4].sub >= 0, "65500: eligibility");
  }
  // totals just under and just over the 256 MiB cut
  {
    const long long quarter = STREAM_LIMIT / 4;
    auto four = [&](long long last_delta) {
      std::vector<FileIn> v;
      for (int i = 0; i < 4; ++i) v.push_back(image(64, 64, 3, 2, 2, 0, quarter - CLEAN_PAD - ALIGN + (i == 3 ? last_delta : 0)));
      return v;
    };
    EXPECT(check(four(0), nullptr, "under the cut") == 1, "4 x (64 MiB - 256) stays one sub-batch");
    EXPECT(check(four(4 * ALIGN), nullptr, "at the cut") == 2, "a total of exactly 256 MiB is cut");
    EXPECT(check(four(5 * ALIGN), nullptr, "over the cut") == 2, "a total over 256 MiB is cut");
    std::vector<FileIn> big{image(64, 64, 3, 2, 2, 0, STREAM_LIMIT - CLEAN_PAD - ALIGN), image(64, 64, 3, 2, 2, 0, STREAM_LIMIT - CLEAN_PAD), image(8, 8, 1, 1, 1, 0, 10)};
    EXPECT(check(big, nullptr, "one huge file") == 2, "a file just under the limit is a sub-batch of its own, one at the limit goes to the host");
  }
  // plans of exactly one file: what every single-file decode (ffp_jpeg_decode*) runs on — the planner sizes the buffers of a frame
  {
    struct One { const char* name; FileIn f; bool admitted; };
    const One ones[] = {
        {"one 1x1", image(1, 1, 3, 2, 2, 0, 3), true},
        {"one 4K 4:2:0", image(2160, 3840, 3, 2, 2, 0, 1100000), true},
        {"one 16K", image(8640, 15360, 3, 2, 2, 0, 30ll << 20), true},
        {"one with dri 1", image(47, 60, 3, 2, 1, 1, 4000), true},
        {"one under the limit", image(64, 64, 3, 2, 2, 0, STREAM_LIMIT - CLEAN_PAD - ALIGN), true},
        {"one whose padded stream reaches the limit", image(64, 64, 3, 2, 2, 0, STREAM_LIMIT - CLEAN_PAD), false},
        {"one at the limit", image(64, 64, 3, 2, 2, 0, STREAM_LIMIT), false},
    };
    for (const One& o : ones) {
      const std::vector<FileIn> v{o.f};
      const int subs = check(v, nullptr, o.name);
      const Plan P = plan_batch(v.data(), nullptr, 1, kSizes);
      EXPECT(subs == (o.admitted ? 1 : 0) && P.subs.size() == (size_t)subs && P.files[0].sub == (o.admitted ? 0 : -1), "%s: %d sub-batches, file in sub %d", o.name, subs,
             P.files[0].sub);
      if (o.admitted) EXPECT(P.subs[0].files.size() == 1 && P.subs[0].files[0] == 0 && P.files[0].slot == 0 && P.files[0].wg0 == 0 && P.files[0].tile0 == 0, "%s: slot", o.name);
    }
  }
  // seeded sets: plausible crops mixed with headers that claim nonsense, and unreadable files in between
  std::mt19937 rng(20240607u);
  for (int round = 0; round < 300; ++round) {
    const int n = (int)(rng() % 70);
    std::vector<FileIn> v;
    std::vector<unsigned char> readable;
    for (int i = 0; i < n; ++i) {
      const int kind = (int)(rng() % 10);
      FileIn f;
      if (kind < 7) {
        const int h = 1 + (int)(rng() % 300), w = 1 + (int)(rng() % 300), ncomp = rng() % 5 ? 3 : 1;
        const int hsub = ncomp == 3 ? 1 + (int)(rng() % 2) : 1, vsub = ncomp == 3 && hsub == 2 ? 1 + (int)(rng() % 2) : 1;
        const int dris[] = {0, 0, 1, 7, 64};
        f = image(h, w, ncomp, hsub, vsub, dris[rng() % 5], 1 + (long long)(rng() % 60000));
      } else if (kind < 9) {                       // every field from the whole range of its type
        auto any = [&]() { return (int)rng(); };
        f.h = any() % 70000; f.w = any() % 70000; f.ncomp = any() % 6; f.dri = any() % 70000; f.n_raw = (long long)(int)rng() * (long long)(rng() % 4);
        for (int c = 0; c < 3; ++c) { f.hs[c] = any() % 6; f.vs[c] = any() % 6; f.blocks_x[c] = any() % 40000; f.blocks_y[c] = any() % 40000; }
      } else {                                     // consistent but with more than six blocks per MCU
        f = image(32, 32, 3, 2, 2, 0, 500);
        f.hs[1] = 2; f.blocks_x[1] *= 2;
      }
      v.push_back(f);
      readable.push_back((unsigned char)(rng() % 8 != 0));
    }
    check(v, &readable, "seeded");
  }
  if (g_fail) { std::printf("jpeg_batch_plan_host_check: %d failures\n", g_fail); return 1; }
  std::printf("jpeg_batch_plan_host_check: ok\n");
  return 0;
}
