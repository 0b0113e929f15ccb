// sr_tiles_host_check.cpp — the tile geometry of the Real-ESRGAN path (sr_tiles.hpp) on a CPU-only machine, under AddressSanitizer + UBSan
// (build.py --sr-tiles-check). A dense grid of small cases (h, w in 1..12) and seeded random batches of one to three images (h, w in 1..40), over
// scale {2, 4}, tile {0, 2, 4, 6, 8, 16, 40} (the random cases add odd tiles), tile_pad {0, 2, 4, 10, 20} (and odd pads), pre_pad 0..h (h itself
// and beyond are refusals). For every accepted case:
//   * every source coordinate a tile asks for lands in [0, src_h) x [0, src_w) after reflect2, and equals the index an explicit
//     F.pad(reflect) by pre_pad followed by an explicit F.pad(reflect) by the mod pad gives;
//   * the cores are disjoint and cover the s*h x s*w canvas exactly once (painted into an array of exactly that size);
//   * each core lies inside its tile's network output: tx + cw <= s * tile_w, ty + ch <= s * tile_h;
//   * x2 tiles have even size and origin;
//   * tiles come image by image, row by row, and carry their image's offsets, strides and formats;
//   * the level sizes are tile / shuffle (x2, x4) and the 16x16 tile count a plan is chosen by equals the sum over the tiles;
//   * the descriptor tables hold the tiles, running core offsets, and empty padding entries up to the capacity.
// For every refused case the refusal is the stated one: pre_pad >= size, a one-pixel side under the x2 mod pad, or odd x2 geometry.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sr_tiles.hpp"

using namespace ffp;

static long long fails = 0, accepted = 0, refused = 0, tiles_seen = 0;
static long long refused_by[8] = {0};
#define CHECK(c, ...) do { if (!(c)) { if (fails < 40) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

// index into the source of position i of the twice-padded axis, by building both pads explicitly
static std::vector<int> padded_axis(int n, int pre_pad, int mod_pad) {
  std::vector<int> a(n);
  for (int i = 0; i < n; ++i) a[i] = i;
  std::vector<int> b = a;
  for (int k = 0; k < pre_pad; ++k) b.push_back(a[n - 2 - k]);            // reflect: the edge sample is not repeated
  std::vector<int> c = b;
  const int m = (int)b.size();
  for (int k = 0; k < mod_pad; ++k) c.push_back(b[m - 2 - k]);
  return c;
}

// does any tile of a padded axis of length L start or end at an odd position?
static bool axis_odd(int L, int tile, int tile_pad) {
  if (tile <= 0) return L % 2 != 0;
  for (int s0 = 0; s0 < L; s0 += tile) {
    const int e0 = std::min(s0 + tile, L);
    const int sp = std::max(s0 - tile_pad, 0), ep = std::min(e0 + tile_pad, L);
    if (sp % 2 || ep % 2) return true;
  }
  return false;
}

static SrTilesStatus expected_status(const std::vector<SrImage>& imgs, int s, int tile, int tile_pad, int pre_pad) {
  for (const SrImage& im : imgs) {
    if (pre_pad >= im.h || pre_pad >= im.w) return SR_TILES_PRE_PAD;
    int H = im.h + pre_pad, W = im.w + pre_pad;
    if (s == 2) {
      if ((H % 2 && H < 2) || (W % 2 && W < 2)) return SR_TILES_TOO_SMALL;
      H += H % 2; W += W % 2;
      const int tsz = tile > 0 ? tile : std::max(H, W);
      // tiles are walked row by row: the first odd one decides, and any odd axis makes some tile odd
      if (axis_odd(H, tile > 0 ? tsz : 0, tile_pad) || axis_odd(W, tile > 0 ? tsz : 0, tile_pad)) return SR_TILES_ODD_X2;
    }
  }
  return SR_TILES_OK;
}

static void run_case(const std::vector<SrImage>& imgs, int s, int tile, int tile_pad, int pre_pad) {
  std::vector<SrTile> tiles;
  const SrTilesStatus st = sr_tiles(imgs, s, tile, tile_pad, pre_pad, tiles);
  const SrTilesStatus want = expected_status(imgs, s, tile, tile_pad, pre_pad);
  CHECK(st == want, "status %d, expected %d (s %d tile %d pad %d pre %d, first image %dx%d of %d)", (int)st, (int)want, s, tile, tile_pad, pre_pad,
        imgs[0].h, imgs[0].w, (int)imgs.size());
  if (st != SR_TILES_OK) {
    CHECK(st == SR_TILES_PRE_PAD || st == SR_TILES_TOO_SMALL || st == SR_TILES_ODD_X2, "refusal %d is none of the stated ones", (int)st);
    ++refused;
    ++refused_by[(int)st & 7];
    return;
  }
  ++accepted;
  const int shuf = s == 2 ? 2 : 1;
  size_t k = 0;
  long long t16 = 0;
  for (size_t ii = 0; ii < imgs.size(); ++ii) {
    const SrImage& im = imgs[ii];
    const int pre_h = im.h + pre_pad, pre_w = im.w + pre_pad;
    const int mph = s == 2 ? pre_h % 2 : 0, mpw = s == 2 ? pre_w % 2 : 0;
    const std::vector<int> ay = padded_axis(im.h, pre_pad, mph), ax = padded_axis(im.w, pre_pad, mpw);
    const int H = pre_h + mph, W = pre_w + mpw, oh = s * im.h, ow = s * im.w;
    std::vector<unsigned char> canvas((size_t)oh * ow, 0);
    const int tsz = tile > 0 ? tile : std::max(H, W);
    const size_t want_tiles = (size_t)((H + tsz - 1) / tsz) * ((W + tsz - 1) / tsz);
    CHECK(k + want_tiles <= tiles.size(), "image %zu: %zu tiles expected, the list ends early", ii, want_tiles);
    if (k + want_tiles > tiles.size()) return;
    int last_oy = -1, last_ox = -1;
    for (size_t j = 0; j < want_tiles; ++j, ++k) {
      const SrTile& t = tiles[k];
      ++tiles_seen;
      CHECK(t.src.src_off == im.in_off && t.src.src_stride == im.in_stride && t.src.src_h == im.h && t.src.src_w == im.w, "tile %zu: source of another image", k);
      CHECK(t.dst.dst_off == im.out_off && t.dst.dst_stride == im.out_stride, "tile %zu: canvas of another image", k);
      CHECK(t.src.fmt.sel == im.in_fmt.sel && t.src.fmt.cn == im.in_fmt.cn && t.dst.fmt.sel == im.out_fmt.sel && t.dst.fmt.cn == im.out_fmt.cn, "tile %zu: format", k);
      CHECK(t.src.pre_h == pre_h && t.src.pre_w == pre_w, "tile %zu: pre-padded size", k);
      CHECK(t.h >= 1 && t.w >= 1 && t.src.x0 >= 0 && t.src.y0 >= 0 && t.src.y0 + t.h <= H && t.src.x0 + t.w <= W, "tile %zu: %dx%d at (%d, %d) outside the %dx%d padded image", k,
            t.h, t.w, t.src.y0, t.src.x0, H, W);
      CHECK(t.dst.oy > last_oy || (t.dst.oy == last_oy && t.dst.ox > last_ox), "tile %zu: not in row-major order", k);
      last_oy = t.dst.oy; last_ox = t.dst.ox;
      for (int y = 0; y < t.h; ++y) {
        const int sy = reflect2(t.src.y0 + y, t.src.pre_h, t.src.src_h);
        CHECK(sy >= 0 && sy < im.h, "tile %zu row %d reads source row %d of %d", k, y, sy, im.h);
        CHECK(t.src.y0 + y < (int)ay.size() && sy == ay[t.src.y0 + y], "tile %zu row %d: source row %d, the explicit pads give another", k, y, sy);
      }
      for (int x = 0; x < t.w; ++x) {
        const int sx = reflect2(t.src.x0 + x, t.src.pre_w, t.src.src_w);
        CHECK(sx >= 0 && sx < im.w, "tile %zu column %d reads source column %d of %d", k, x, sx, im.w);
        CHECK(t.src.x0 + x < (int)ax.size() && sx == ax[t.src.x0 + x], "tile %zu column %d: source column %d, the explicit pads give another", k, x, sx);
      }
      if (shuf == 2) CHECK(t.h % 2 == 0 && t.w % 2 == 0 && t.src.x0 % 2 == 0 && t.src.y0 % 2 == 0, "tile %zu: odd x2 geometry %dx%d at (%d, %d)", k, t.h, t.w, t.src.y0, t.src.x0);
      CHECK(t.dst.cw >= 0 && t.dst.ch >= 0 && t.dst.tx >= 0 && t.dst.ty >= 0, "tile %zu: negative core", k);
      CHECK(t.dst.tx + t.dst.cw <= s * t.w && t.dst.ty + t.dst.ch <= s * t.h, "tile %zu: core %dx%d at (%d, %d) leaves the %dx%d network output", k, t.dst.ch, t.dst.cw,
            t.dst.ty, t.dst.tx, s * t.h, s * t.w);
      // the core shows the canvas pixels it lands on: tile-local (ty, tx) is padded-source pixel y0 + ty / s, canvas pixel oy is padded-source pixel oy / s
      CHECK(t.dst.cw == 0 || t.dst.ch == 0 || (t.src.x0 * s + t.dst.tx == t.dst.ox && t.src.y0 * s + t.dst.ty == t.dst.oy), "tile %zu: core origin and canvas origin disagree", k);
      for (int y = 0; y < t.dst.ch; ++y)
        for (int x = 0; x < t.dst.cw; ++x) {
          const int cy = t.dst.oy + y, cx = t.dst.ox + x;
          const bool in = cy >= 0 && cy < oh && cx >= 0 && cx < ow;
          CHECK(in, "tile %zu: core pixel (%d, %d) outside the %dx%d canvas", k, cy, cx, oh, ow);
          if (in) {
            CHECK(canvas[(size_t)cy * ow + cx] == 0, "tile %zu: canvas pixel (%d, %d) written twice", k, cy, cx);
            canvas[(size_t)cy * ow + cx] = 1;
          }
        }
      t16 += (long long)((t.h / shuf + 15) / 16) * ((t.w / shuf + 15) / 16);
    }
    size_t holes = 0;
    for (unsigned char c : canvas) holes += c == 0;
    CHECK(holes == 0, "image %zu: %zu canvas pixels of %dx%d belong to no core (s %d tile %d pad %d pre %d)", ii, holes, oh, ow, s, tile, tile_pad, pre_pad);
  }
  CHECK(k == tiles.size(), "%zu tiles more than the images hold", tiles.size() - k);
  const SrLevelSizes z = sr_level_sizes(tiles, s);
  CHECK(z.t16 == t16, "16x16 tile count %lld, the tiles hold %lld", z.t16, t16);
  const size_t n = tiles.size();
  CHECK(z.hs.size() == n && z.ws.size() == n && z.h1.size() == n && z.w1.size() == n && z.h2.size() == n && z.w2.size() == n, "level size lists");
  for (size_t i = 0; i < n && z.h2.size() == n; ++i) {
    CHECK(z.hs[i] * shuf == tiles[i].h && z.ws[i] * shuf == tiles[i].w, "tile %zu: body level size", i);
    CHECK(z.h1[i] == 2 * z.hs[i] && z.w1[i] == 2 * z.ws[i] && z.h2[i] == s * tiles[i].h && z.w2[i] == s * tiles[i].w, "tile %zu: upsampled level sizes", i);
  }
  const int cap = (int)n + (int)(n % 3);
  std::vector<SrSrc> srcs(n);
  std::vector<SrDst> dsts(cap);
  std::vector<long long> coff((size_t)cap + 1);
  const long long tot = sr_fill_descriptors(tiles, cap, srcs.data(), dsts.data(), coff.data());
  long long run = 0;
  for (int i = 0; i < cap; ++i) {
    CHECK(coff[i] == run, "core offset %d", i);
    if (i < (int)n) CHECK(dsts[i].cw == tiles[i].dst.cw && dsts[i].oy == tiles[i].dst.oy && srcs[i].x0 == tiles[i].src.x0 && srcs[i].y0 == tiles[i].src.y0, "descriptor %d", i);
    else CHECK(dsts[i].cw == 0 && dsts[i].ch == 0, "padding entry %d is not empty", i);
    run += (long long)dsts[i].cw * dsts[i].ch;
  }
  CHECK(coff[cap] == run && tot == run, "core total");
  long long canvas_px = 0;
  for (const SrImage& im : imgs) canvas_px += (long long)s * im.h * s * im.w;
  CHECK(tot == canvas_px, "cores hold %lld pixels, the canvases %lld", tot, canvas_px);
}

static SrImage image(int h, int w, int idx) {
  SrImage im;
  im.h = h; im.w = w;
  im.in_off = 1000ll * idx + 3; im.in_stride = w * 4 + idx; im.out_off = 100000ll * idx + 5; im.out_stride = w * 16 + 7 * idx;
  im.in_fmt.cn = im.out_fmt.cn = idx % 2 ? 4 : 3;
  im.in_fmt.sel = im.out_fmt.sel = idx % 2 ? SR_SEL_ALPHA : SR_SEL_BGR;
  return im;
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 6000;
  const int tiles_[7] = {0, 2, 4, 6, 8, 16, 40}, pads_[5] = {0, 2, 4, 10, 20};
  // the argument checks that come before any geometry
  {
    std::vector<SrTile> t;
    CHECK(sr_tiles({}, 4, 0, 10, 0, t) == SR_TILES_EMPTY_BATCH, "empty batch");
    CHECK(sr_tiles({image(4, 4, 0)}, 4, 0, -1, 0, t) == SR_TILES_NEGATIVE_PAD && sr_tiles({image(4, 4, 0)}, 4, 0, 0, -1, t) == SR_TILES_NEGATIVE_PAD, "negative padding");
    CHECK(sr_tiles({image(0, 4, 0)}, 4, 0, 0, 0, t) == SR_TILES_EMPTY_IMAGE && sr_tiles({image(4, 0, 0)}, 2, 0, 0, 0, t) == SR_TILES_EMPTY_IMAGE, "empty image");
    CHECK(reflect2(5, 5, 4) == 3 && reflect2(7, 7, 4) == 1 && reflect2(4, 5, 4) == 2 && reflect2(3, 5, 4) == 3 && reflect2(6, 6, 5) == 4, "reflect2 by hand");
  }
  for (int h = 1; h <= 12; ++h)
    for (int w = 1; w <= 12; ++w)
      for (int s = 2; s <= 4; s += 2)
        for (int tile : tiles_)
          for (int pad : pads_)
            for (int pre = 0; pre <= h; ++pre) run_case({image(h, w, 0)}, s, tile, pad, pre);
  const long long dense = accepted + refused;
  std::mt19937 rng(20240611);
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (int c = 0; c < n_random; ++c) {
    const int n_img = pick(1, 3), s = pick(0, 1) ? 4 : 2;
    std::vector<SrImage> imgs;
    int hmin = 1 << 30;
    for (int i = 0; i < n_img; ++i) {
      imgs.push_back(image(pick(1, 40), pick(1, 40), i));
      hmin = std::min(hmin, imgs.back().h);
    }
    const int tile = pick(0, 3) ? tiles_[pick(0, 6)] : pick(1, 41);
    const int pad = pick(0, 3) ? pads_[pick(0, 4)] : pick(0, 21);
    const int pre = pick(0, 4) ? pick(0, hmin - 1) : pick(0, 41);
    run_case(imgs, s, tile, pad, pre);
  }
  std::printf("sr_tiles cases: %lld dense + %d random, %lld accepted (%lld tiles), %lld refused (pre_pad %lld, too small %lld, odd x2 %lld)\n", dense, n_random, accepted,
              tiles_seen, refused, refused_by[SR_TILES_PRE_PAD], refused_by[SR_TILES_TOO_SMALL], refused_by[SR_TILES_ODD_X2]);
  if (fails || accepted == 0 || refused == 0) {
    std::printf("sr_tiles_host_check: %lld FAILED\n", fails);
    return 1;
  }
  std::printf("sr_tiles_host_check: ok\n");
  return 0;
}
