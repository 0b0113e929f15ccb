// overlay.hip — detection overlays painted on the device: an ordered list of rectangles and 8-bit stamps composited in place into an
// h x w x 3 uint8 frame (replaces the ImageDraw calls of utils/visualization.py's _render, which replaced cv2.rectangle / cv2.putText /
// cv2.circle / cv2.line of the reference's draw_detections).
//
// One workgroup of four wavefronts per tile of kOverlayTileW x kOverlayTileH pixels. The workgroup walks the whole list in chunks of 256
// primitives (one per thread), tests each primitive's clipped box against its tile, and appends the hits to a list in LDS IN LIST ORDER:
// per wavefront a ballot and a prefix count, across the four wavefronts their counts in wavefront order. Each thread then applies that
// sub-list, front to back, to the bytes it owns. Nothing orders two primitives but their index: no atomics, no arrival order.
//
// Ownership. A byte belongs to the tile of its pixel, and inside the tile to the thread that holds the ALIGNED 4-byte word around it: row
// r of the tile is wavefront r % 4's on pass r / 4, and lane l takes the l-th aligned word that overlaps the row's byte range. 84 pixels
// are 252 bytes, which at any base alignment overlap at most 64 aligned words — one wave instruction of 256 contiguous bytes per row.
// A word that lies wholly inside the range is loaded and stored as one dword; a word cut by the range's ends (the image's or the tile's
// edge at an odd alignment) is loaded and stored byte by byte, and only the bytes inside. So no byte outside the w*3 bytes of a row is
// ever written, whatever the pitch and the base address are, and every byte has one owner.
//
// A tile no primitive touches ends after the walk: its pixels are neither read nor written. The LDS list holds kListCap indices; when the
// next chunk might not fit, the list so far is applied and emptied first (the same threads own the same bytes, so the order holds).
#include "overlay.hpp"

#include <atomic>

namespace ffp {
namespace {

constexpr int kThreads = 256;
constexpr int kListCap = 1024;

// what the kernel reads of a primitive. box: the painted extent clipped to the image, inclusive (the cull test and the x / y test).
struct DPrim {
  int x0, y0, x1, y1;     // clipped extent
  int a0, a1, a2, a3;     // RECT: the unpainted inside of a frame, inclusive (a0 > a2: none, a fill). STAMP: mask x0, y0 (unclipped), pitch, offset
  unsigned color_kind;    // colour bytes 0..2 | kind << 24
  unsigned pad[3];
};
static_assert(sizeof(DPrim) == 48, "DPrim is three 16-byte words");

struct OverlayArgs {
  unsigned char* img;
  long long pitch;
  int h, w;
  const int4* boxes;      // DPrim::x0..y1 again, packed: all the walk reads
  const DPrim* prims;
  int n;
  const unsigned char* masks;
  int tiles_x;
};

__device__ __forceinline__ unsigned blend(unsigned dst, unsigned c, unsigned m) {
  const unsigned t = dst * (255u - m) + c * m + 128u;
  return ((t >> 8) + t) >> 8;
}

__device__ void apply_list(const OverlayArgs& A, const int* list, int cnt, int tx0, int ty0, int wave, int lane) {
  const int tx1 = min(tx0 + kOverlayTileW, A.w);                       // exclusive
  const int ty1 = min(ty0 + kOverlayTileH, A.h);
  const long long lo = (long long)tx0 * 3, hi = (long long)tx1 * 3;      // the tile's byte range inside a row
  for (int y = ty0 + wave; y < ty1; y += kThreads / 64) {
    unsigned char* row = A.img + (long long)y * A.pitch;
    const unsigned long long first = (unsigned long long)(row + lo) & ~3ull;                 // aligned word around the range's first byte
    unsigned char* word = reinterpret_cast<unsigned char*>(first) + 4 * lane;
    const long long o0 = (long long)(word - row);                                             // byte offset in the row; -3..-1 possible at x == 0
    if (o0 >= hi) continue;
    const bool full = o0 >= lo && o0 + 4 <= hi;
    unsigned v[4];
    bool in[4];
    int px[4], ch[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long o = o0 + j;
      in[j] = o >= lo && o < hi;
      const int oo = in[j] ? (int)o : 0;
      px[j] = oo / 3;
      ch[j] = oo - 3 * px[j];
      v[j] = 0;
    }
    if (full) {
      const unsigned d = *reinterpret_cast<const unsigned*>(word);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (d >> (8 * j)) & 255u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) v[j] = word[j];
    }
    for (int k = 0; k < cnt; ++k) {
      const int idx = __builtin_amdgcn_readfirstlane(list[k]);           // the same for every lane: the primitive comes through the scalar cache
      const DPrim& p = A.prims[idx];
      if (y < p.y0 || y > p.y1) continue;
      const unsigned kind = p.color_kind >> 24;
      if (kind == FFP_OVERLAY_RECT) {
        const bool hole_row = y >= p.a1 && y <= p.a3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool hit = in[j] && px[j] >= p.x0 && px[j] <= p.x1 && !(hole_row && px[j] >= p.a0 && px[j] <= p.a2);
          if (hit) v[j] = (p.color_kind >> (8 * ch[j])) & 255u;
        }
      } else {
        const unsigned char* mrow = A.masks + (long long)(unsigned)p.a3 + (long long)(y - p.a1) * p.a2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (in[j] && px[j] >= p.x0 && px[j] <= p.x1) {
            const unsigned m = mrow[px[j] - p.a0];
            v[j] = blend(v[j], (p.color_kind >> (8 * ch[j])) & 255u, m);
          }
        }
      }
    }
    if (full) {
      *reinterpret_cast<unsigned*>(word) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) word[j] = (unsigned char)v[j];
    }
  }
}

__global__ __launch_bounds__(kThreads) void overlay_kernel(OverlayArgs A) {
  __shared__ int s_list[kListCap];
  __shared__ int s_wave[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  const int tx0 = (tile % A.tiles_x) * kOverlayTileW, ty0 = (tile / A.tiles_x) * kOverlayTileH;
  const int tx1 = min(tx0 + kOverlayTileW, A.w) - 1, ty1 = min(ty0 + kOverlayTileH, A.h) - 1;     // inclusive
  int cnt = 0;
  for (int base = 0; base < A.n; base += kThreads) {
    if (cnt + kThreads > kListCap) {                    // uniform: every thread holds the same cnt
      apply_list(A, s_list, cnt, tx0, ty0, wave, lane);
      cnt = 0;
      __syncthreads();                                  // the list is read to its end before it is written again
    }
    const int i = base + tid;
    bool hit = false;
    if (i < A.n) {
      const int4 b = A.boxes[i];
      hit = b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) {
      const int c = s_wave[wv];
      before += wv < wave ? c : 0;
      total += c;
    }
    if (hit) s_list[cnt + before + __popcll(votes & ((1ull << lane) - 1ull))] = i;
    cnt += total;
    __syncthreads();                                    // the list is complete, and s_wave may be written again
  }
  if (cnt > 0) apply_list(A, s_list, cnt, tx0, ty0, wave, lane);
}

// What one call in flight holds, borrowed from the codecs' kind of pool (ws_pool.hpp): the device copies of the list and of the mask pool and
// the pinned staging they go up through.
struct Workspace {
  int device = 0;
  DevBuf boxes, prims, masks;
  HostPinned stage;
  size_t held() const { return boxes.n + prims.n + masks.n + stage.n; }
};
// at most 8 idle ones; one that grew past 256 MiB is not kept (never destroyed: nothing is freed at exit, when the runtime may be gone)
WsPool<Workspace>& g_pool = *new WsPool<Workspace>(WsPolicy{8, 0, 256u << 20}, delete_on_owner_device<Workspace>);

inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

void overlay_check(int h, int w, long long row_stride, const ffp_overlay_prim* prims, int n, const unsigned char* masks, long long mask_bytes) {
  FFP_CHECK(h > 0 && w > 0 && row_stride >= (long long)w * 3, FFP_ERR_ARG, "overlay_draw: a %d x %d image with a row pitch of %lld bytes", w, h, row_stride);
  FFP_CHECK((long long)((h + kOverlayTileH - 1) / kOverlayTileH) * ((w + kOverlayTileW - 1) / kOverlayTileW) <= 0x7fffffffll, FFP_ERR_ARG,
            "overlay_draw: a %d x %d image has too many tiles", w, h);
  FFP_CHECK(n >= 0 && n <= kOverlayMaxPrims, FFP_ERR_ARG, "overlay_draw: %d primitives (0..%d are taken)", n, kOverlayMaxPrims);
  FFP_CHECK(n == 0 || prims, FFP_ERR_ARG, "overlay_draw: the primitive list is null");
  FFP_CHECK(mask_bytes >= 0 && mask_bytes <= 0x7fffffffll && (mask_bytes == 0 || masks), FFP_ERR_ARG, "overlay_draw: a mask pool of %lld bytes%s", mask_bytes,
            mask_bytes > 0 && !masks ? " that is null" : "");
  for (int i = 0; i < n; ++i) {
    const ffp_overlay_prim& p = prims[i];
    if (p.kind == FFP_OVERLAY_RECT) {
      FFP_CHECK(p.width >= 0, FFP_ERR_ARG, "overlay_draw: primitive %d: a frame width of %d", i, p.width);
    } else if (p.kind == FFP_OVERLAY_STAMP) {
      const long long mw = p.x1, mh = p.y1, pitch = p.width, off = p.mask_off;
      FFP_CHECK(mw >= 0 && mh >= 0 && off >= 0 && pitch >= mw, FFP_ERR_ARG, "overlay_draw: primitive %d: a %lld x %lld stamp at offset %lld with pitch %lld", i, mw, mh,
                off, pitch);
      FFP_CHECK(mw == 0 || mh == 0 || off + (mh - 1) * pitch + mw <= mask_bytes, FFP_ERR_ARG,
                "overlay_draw: primitive %d: its mask ends at byte %lld of a pool of %lld", i, off + (mh - 1) * pitch + mw, mask_bytes);
    } else {
      fail(FFP_ERR_ARG, "overlay_draw: primitive %d is of kind %d (FFP_OVERLAY_RECT and FFP_OVERLAY_STAMP are known)", i, p.kind);
    }
  }
}

void overlay_draw_device(unsigned char* d_img, int h, int w, long long row_stride, const ffp_overlay_prim* prims, int n, const unsigned char* masks,
                         long long mask_bytes, hipStream_t st) {
  // the device form, in 64-bit arithmetic so that no corner overflows: primitives that paint nothing inside the image are dropped here
  std::vector<DPrim> dp;
  dp.reserve((size_t)n);
  for (int i = 0; i < n; ++i) {
    const ffp_overlay_prim& p = prims[i];
    DPrim d{};
    long long x0 = p.x0, y0 = p.y0, x1, y1;
    if (p.kind == FFP_OVERLAY_RECT) {
      x1 = p.x1; y1 = p.y1;
      // the inside a frame leaves alone, clamped to a range every pixel coordinate lies strictly inside
      const long long big = 1ll << 30, t = p.width;
      long long ix0 = x0 + t, iy0 = y0 + t, ix1 = x1 - t, iy1 = y1 - t;
      if (t == 0 || ix0 > ix1 || iy0 > iy1) { ix0 = 1; ix1 = 0; iy0 = 1; iy1 = 0; }
      d.a0 = (int)clampll(ix0, -big, big); d.a1 = (int)clampll(iy0, -big, big);
      d.a2 = (int)clampll(ix1, -big, big); d.a3 = (int)clampll(iy1, -big, big);
    } else {
      x1 = x0 + p.x1 - 1; y1 = y0 + p.y1 - 1;
      d.a0 = p.x0; d.a1 = p.y0; d.a2 = p.width; d.a3 = p.mask_off;
    }
    if (x1 < x0 || y1 < y0 || x1 < 0 || y1 < 0 || x0 >= w || y0 >= h) continue;
    d.x0 = (int)std::max<long long>(x0, 0); d.y0 = (int)std::max<long long>(y0, 0);
    d.x1 = (int)std::min<long long>(x1, w - 1); d.y1 = (int)std::min<long long>(y1, h - 1);
    d.color_kind = (unsigned)p.color[0] | ((unsigned)p.color[1] << 8) | ((unsigned)p.color[2] << 16) | ((unsigned)p.kind << 24);
    dp.push_back(d);
  }
  const int m = (int)dp.size();
  if (m == 0) return;

  auto lease = lease_ws(g_pool, st);
  Workspace& ws = *lease;
  const size_t box_bytes = (size_t)m * sizeof(int4), prim_bytes = (size_t)m * sizeof(DPrim), mb = (size_t)mask_bytes;
  const size_t prim_at = box_bytes, mask_at = prim_at + prim_bytes;         // multiples of 16
  ws.stage.ensure(mask_at + mb + 16);
  unsigned char* stage = static_cast<unsigned char*>(ws.stage.p);
  int4* boxes = reinterpret_cast<int4*>(stage);
  for (int i = 0; i < m; ++i) boxes[i] = make_int4(dp[i].x0, dp[i].y0, dp[i].x1, dp[i].y1);
  std::memcpy(stage + prim_at, dp.data(), prim_bytes);
  if (mb) std::memcpy(stage + mask_at, masks, mb);
  ws.boxes.ensure(box_bytes);
  ws.prims.ensure(prim_bytes);
  ws.masks.ensure(mb + 16);
  FFP_HIP(hipMemcpyAsync(ws.boxes.p, stage, box_bytes, hipMemcpyHostToDevice, st));
  FFP_HIP(hipMemcpyAsync(ws.prims.p, stage + prim_at, prim_bytes, hipMemcpyHostToDevice, st));
  if (mb) FFP_HIP(hipMemcpyAsync(ws.masks.p, stage + mask_at, mb, hipMemcpyHostToDevice, st));

  OverlayArgs a;
  a.img = d_img; a.pitch = row_stride; a.h = h; a.w = w;
  a.boxes = ws.boxes.as<int4>(); a.prims = ws.prims.as<DPrim>(); a.n = m;
  a.masks = ws.masks.as<unsigned char>();
  a.tiles_x = (w + kOverlayTileW - 1) / kOverlayTileW;
  const long long tiles = (long long)a.tiles_x * ((h + kOverlayTileH - 1) / kOverlayTileH);
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, a);
  FFP_HIP(hipGetLastError());
  FFP_HIP(hipStreamSynchronize(st));            // the workspace goes back to the pool with nothing in flight
}

}  // namespace ffp
