// sr_tiles.hpp — the tile geometry of the Real-ESRGAN path: which padded tile of which image the network sees, and where the core of its output
// lands (RealESRGANer.pre_process / tile_process / post_process, realesrgan 0.3.0). Plain C++ on both sides: the engine
// (rrdb.cpp) and the operator entries (api_ops.cpp) build their descriptors here, the kernels of sr_ops.hip walk them and share reflect2, and
// sr_tiles_host_check.cpp runs all of it under the sanitizers.
#pragma once
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define FFP_HD __host__ __device__
#else
#define FFP_HD
#endif

namespace ffp {

// Pixel format of an image the SR path reads or writes (realesrgan 0.3.0 RealESRGANer.enhance, reference call
// utils/enhancer.py:214). The default is 3-channel uint8 BGR.
enum SrSel : int {
  SR_SEL_BGR = 0,        // read: BGR from channels 0-2 (3- or 4-channel pixel); write: BGR into channels 0-2
  SR_SEL_GRAY = 1,       // read: channel 0 replicated to RGB (mode 'L'); write: BGR2GRAY into channel 0 (1-channel canvas)
  SR_SEL_ALPHA = 2,      // read: channel 3 replicated to RGB (mode 'RGBA'); write: BGR2GRAY into channel 3 (4-channel canvas)
};
struct SrFmt {
  int cn = 3;            // channels per pixel (1, 3, 4)
  int wide = 0;          // 0: 8-bit storage, 1: 16-bit storage
  float range = 255.f;   // max_range: value = stored / range on read, rint(value * range) on write
  int sel = SR_SEL_BGR;
  FFP_HD int px_bytes() const { return cn << wide; }
};

struct SrSrc {          // where one network tile reads its pixels
  long long src_off;    // byte offset of the source image inside the base allocation
  int src_stride;       // bytes per source row
  int src_h, src_w;     // source size
  int pre_h, pre_w;     // size after pre_pad; rows beyond reflect about it first (mod pad), then about the source
  int x0, y0;           // tile origin in padded-source coordinates
  SrFmt fmt;
};
struct SrDst {          // where the core of one tile's output lands
  long long dst_off;    // byte offset of the output canvas inside the base allocation
  int dst_stride;       // bytes per canvas row
  int ox, oy;           // core origin in the canvas
  int cw, ch;           // core size (output pixels)
  int tx, ty;           // core origin inside the tile's network output
  SrFmt fmt;
};

struct SrImage {           // one image of a batch: offsets are relative to the in/out base allocations
  long long in_off; int in_stride; int h, w;
  long long out_off; int out_stride;
  SrFmt in_fmt, out_fmt;   // strides are in bytes; two images may share a buffer and differ in their channel selection
};

struct SrTile { SrSrc src; SrDst dst; int h, w; };      // h x w: the padded tile in padded-source pixels (the network sees h/shuf x w/shuf)

// F.pad(..., 'reflect') twice on the high side: the mod pad reflects the pre-padded image, pre_pad reflects the source
FFP_HD inline int reflect2(int i, int n_pre, int n) {
  if (i >= n_pre) i = 2 * (n_pre - 1) - i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

enum SrTilesStatus : int {
  SR_TILES_OK = 0,
  SR_TILES_EMPTY_BATCH,
  SR_TILES_NEGATIVE_PAD,
  SR_TILES_EMPTY_IMAGE,
  SR_TILES_PRE_PAD,         // pre_pad >= image size: reflect padding undefined
  SR_TILES_TOO_SMALL,       // a one-pixel side cannot take the x2 model's mod pad
  SR_TILES_ODD_X2,          // the x2 model's pixel_unshuffle needs even tile sizes and origins
};

inline int sr_shuffle(int scale) { return scale == 2 ? 2 : 1; }      // pixel_unshuffle factor in front of the network

// The tiles of every image, images in order, each image's tiles row by row. On a refusal `tiles` holds what was built so far.
inline SrTilesStatus sr_tiles(const std::vector<SrImage>& imgs, int scale, int tile, int tile_pad, int pre_pad, std::vector<SrTile>& tiles) {
  tiles.clear();
  if (imgs.empty()) return SR_TILES_EMPTY_BATCH;
  if (tile_pad < 0 || pre_pad < 0) return SR_TILES_NEGATIVE_PAD;
  const int s = scale;
  const int shuf = sr_shuffle(s);
  for (const SrImage& im : imgs) {
    if (im.h < 1 || im.w < 1) return SR_TILES_EMPTY_IMAGE;
    // pre_pad (reflect, bottom/right), then mod pad to a multiple of 2 for the x2 model (RealESRGANer.pre_process)
    if (pre_pad >= im.h || pre_pad >= im.w) return SR_TILES_PRE_PAD;
    int H = im.h + pre_pad, W = im.w + pre_pad;
    int mph = 0, mpw = 0;
    if (s == 2) { if (H % 2) mph = 2 - H % 2; if (W % 2) mpw = 2 - W % 2; }
    if ((mph != 0 && H < 2) || (mpw != 0 && W < 2)) return SR_TILES_TOO_SMALL;
    H += mph; W += mpw;
    const int out_h = im.h * s, out_w = im.w * s;     // pads are cropped off again (post_process)
    const int tsz = tile > 0 ? tile : std::max(H, W);
    const int txn = (W + tsz - 1) / tsz, tyn = (H + tsz - 1) / tsz;
    for (int ty = 0; ty < tyn; ++ty)
      for (int tx = 0; tx < txn; ++tx) {
        const int sx = tx * tsz, ex = std::min(sx + tsz, W), sy = ty * tsz, ey = std::min(sy + tsz, H);
        int sxp = sx, exp_ = ex, syp = sy, eyp = ey;
        if (tile > 0) { sxp = std::max(sx - tile_pad, 0); exp_ = std::min(ex + tile_pad, W); syp = std::max(sy - tile_pad, 0); eyp = std::min(ey + tile_pad, H); }
        SrTile t;
        t.h = eyp - syp; t.w = exp_ - sxp;
        if (shuf != 1 && (t.h % 2 != 0 || t.w % 2 != 0 || sxp % 2 != 0 || syp % 2 != 0)) return SR_TILES_ODD_X2;
        t.src.src_off = im.in_off; t.src.src_stride = im.in_stride; t.src.src_h = im.h; t.src.src_w = im.w; t.src.pre_h = im.h + pre_pad; t.src.pre_w = im.w + pre_pad;
        t.src.x0 = sxp; t.src.y0 = syp; t.src.fmt = im.in_fmt;
        // core region in output pixels, clipped to the un-padded output
        const int ox = sx * s, oy = sy * s;
        const int cw = std::min(ex * s, out_w) - ox, chh = std::min(ey * s, out_h) - oy;
        t.dst.dst_off = im.out_off; t.dst.dst_stride = im.out_stride; t.dst.fmt = im.out_fmt;
        t.dst.ox = ox; t.dst.oy = oy; t.dst.cw = std::max(cw, 0); t.dst.ch = std::max(chh, 0);
        t.dst.tx = (sx - sxp) * s; t.dst.ty = (sy - syp) * s;
        tiles.push_back(t);
      }
  }
  return SR_TILES_OK;
}

// Image sizes of the three levels a batch of tiles runs on (body, x2 of it, x4 of it) and the number of 16x16 tiles of the body level: what a plan's
// capacity is chosen by.
struct SrLevelSizes { std::vector<int> hs, ws, h1, w1, h2, w2; long long t16 = 0; };
inline SrLevelSizes sr_level_sizes(const std::vector<SrTile>& tiles, int scale) {
  const int shuf = sr_shuffle(scale), n = (int)tiles.size();
  SrLevelSizes z;
  z.hs.resize(n); z.ws.resize(n); z.h1.resize(n); z.w1.resize(n); z.h2.resize(n); z.w2.resize(n);
  for (int i = 0; i < n; ++i) {
    z.hs[i] = tiles[i].h / shuf; z.ws[i] = tiles[i].w / shuf;
    z.h1[i] = z.hs[i] * 2; z.w1[i] = z.ws[i] * 2; z.h2[i] = z.hs[i] * 4; z.w2[i] = z.ws[i] * 4;
    z.t16 += (long long)((z.hs[i] + 15) / 16) * ((z.ws[i] + 15) / 16);
  }
  return z;
}

// The descriptor tables of one launch pair: srcs[n], dsts[cap], core_off[cap + 1] with cap >= n. Entries n .. cap - 1 are padding (a capacity-mode
// batch): empty cores behind the last real one. Returns the number of core pixels.
inline long long sr_fill_descriptors(const std::vector<SrTile>& tiles, int cap, SrSrc* srcs, SrDst* dsts, long long* core_off) {
  const int n = (int)tiles.size();
  long long tot = 0;
  for (int i = 0; i < n; ++i) { srcs[i] = tiles[i].src; dsts[i] = tiles[i].dst; core_off[i] = tot; tot += (long long)dsts[i].cw * dsts[i].ch; }
  for (int i = n; i < cap; ++i) { dsts[i] = SrDst{}; core_off[i] = tot; }
  core_off[cap] = tot;
  return tot;
}

}  // namespace ffp
