// orient.hip — the eight EXIF orientations of an h x w image of 1, 3 or 4 bytes per pixel, out of place, between two pitch-addressed device buffers
// (replaces the numpy transpose-and-copy of the cv2 shim's _oriented and ImageOps.exif_transpose of the readers on a frame that is already on the
// device).
//
// One workgroup of four wavefronts moves one tile of kOrientTile x kOrientTile pixels, and a table of descriptors covers all images of a batch in one
// launch: a workgroup finds its image by bisection on the first-workgroup indices, as the JPEG reconstruction does.
//
// In: the tile's rows go into LDS as they lie in memory. Thread t takes the t-th (row, aligned 4-byte word) pair of the tile's byte range; all of
// a thread's words are loaded before the first is put down, as whole dwords (also a word cut by the range's ends: see the kernel). An LDS row keeps the alignment
// its source row has (the tile's first byte of row r sits at byte (address & 3) of the LDS row), so every global word goes into one LDS word.
// Out: after the barrier thread t takes the t-th (row, aligned word) pair of the DESTINATION tile's byte range, gathers the word's four bytes from LDS
// through the orientation's map and stores it whole; a word cut by the range's ends is stored byte by byte and only inside. This is overlay.hip's
// rule: nothing outside a row's w' * px bytes is ever written, at any base alignment and pitch, and a word that two tiles share is written by each
// only in its own bytes. Consecutive lanes write consecutive words of one destination row for all eight orientations; what the transposing ones pay
// is paid in LDS, where a lane's neighbour reads the next ROW: the LDS row pitch is an odd number of words (49, 65, 17 for px 3, 4, 1), so those
// reads spread over the banks instead of meeting on a few.
#include "orient.hpp"

#include <atomic>
#include <vector>

#include "ws_pool.hpp"

namespace ffp {
namespace {

constexpr int kThreads = 256;
constexpr int T = kOrientTile;
constexpr unsigned kTranspose = 1, kMirrorX = 2, kMirrorY = 4;      // of the destination, the mirrors after the transposition

struct DOrient {
  const unsigned char* src;
  unsigned char* dst;
  long long sp, dp;
  int h, w;               // the source's
  unsigned flags;
  int wg0, tiles_x, pad;
};
static_assert(sizeof(DOrient) == 56, "DOrient is seven 8-byte words");

// the images are in global memory: said to the compiler, so that it does not emit flat accesses, whose waits are shared with the LDS reads
typedef __attribute__((address_space(1))) unsigned GlobalWord;
typedef __attribute__((address_space(1))) unsigned char GlobalByte;

template <int PX>
__global__ __launch_bounds__(kThreads) void orient_kernel(const DOrient* __restrict__ D, int n) {
  constexpr int PW = T * PX / 4 + 1;                       // words of an LDS row: the tile's T * PX bytes at any of the four alignments; odd
  static_assert(PW % 2 == 1 && PW * 4 >= T * PX + 3, "an odd pitch that holds a row at byte offset 3");
  __shared__ unsigned lds[T * PW];
  int lo = 0, hi = n - 1;                                  // the last descriptor whose first workgroup is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (D[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const DOrient d = D[lo];
  const int tile = (int)blockIdx.x - d.wg0;
  const int sy0 = (tile / d.tiles_x) * T, sx0 = (tile % d.tiles_x) * T;
  const int th = min(T, d.h - sy0), tw = min(T, d.w - sx0);
  const unsigned char* const s0 = d.src + (long long)sy0 * d.sp + (long long)sx0 * PX;     // the tile's first source byte
  const int tid = threadIdx.x;

  // Every load of the tile is issued before the first LDS write waits for one: ITER independent loads in flight per thread, not a chain of them.
  // A word cut by the range's ends is read whole all the same: an aligned word that holds one byte of the row lies inside that byte's page, so the
  // read cannot fault, and the bytes of it that are not the tile's are never looked at again (nothing is WRITTEN outside a row: see below).
  constexpr int ITER = (T * PW + kThreads - 1) / kThreads;
  const int in_bytes = tw * PX;
  const unsigned char* const first_word = s0 - ((unsigned long long)s0 & 3ull);
  unsigned v[ITER];
#pragma unroll
  for (int i = 0; i < ITER; ++i) {
    const int idx = tid + i * kThreads;
    const int r = idx / PW, k = idx - r * PW;
    const unsigned char* start = s0 + (long long)r * d.sp;
    const int o0 = 4 * k - (int)((unsigned long long)start & 3ull);      // the word's first byte, counted from the tile's first byte of this row; -3..-1 possible
    const bool mine = idx < th * PW && o0 < in_bytes;                      // no branch around the load: a thread without a word reads the tile's first one
    v[i] = *(const GlobalWord*)(mine ? start + o0 : first_word);
  }
#pragma unroll
  for (int i = 0; i < ITER; ++i) {
    const int idx = tid + i * kThreads;
    if (idx < th * PW) lds[idx] = v[i];
  }
  __syncthreads();

  const bool tr = d.flags & kTranspose, fx = d.flags & kMirrorX, fy = d.flags & kMirrorY;
  const int oh = tr ? tw : th, ow = tr ? th : tw;          // the destination tile
  const int H = tr ? d.w : d.h, W = tr ? d.h : d.w;        // the destination image
  const int ry0 = tr ? sx0 : sy0, rx0 = tr ? sy0 : sx0;    // the tile's origin before the mirrors
  const int dy0 = fy ? H - ry0 - oh : ry0, dx0 = fx ? W - rx0 - ow : rx0;
  unsigned char* const d0 = d.dst + (long long)dy0 * d.dp + (long long)dx0 * PX;
  const unsigned char* const ldsb = reinterpret_cast<const unsigned char*>(lds);
  const int a_s0 = (int)((unsigned long long)s0 & 3ull), a_sp = (int)(d.sp & 3);            // source row r starts at LDS byte (a_s0 + r * a_sp) & 3 of its row
  const int out_bytes = ow * PX;
  for (int idx = tid; idx < oh * PW; idx += kThreads) {
    const int r = idx / PW, k = idx - r * PW;
    unsigned char* start = d0 + (long long)r * d.dp;
    const int a = (int)((unsigned long long)start & 3ull);
    const int o0 = 4 * k - a;
    if (o0 >= out_bytes) continue;
    const int ly = fy ? oh - 1 - r : r;
    unsigned v = 0;
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + j;
      in[j] = o >= 0 && o < out_bytes;
      const int oo = in[j] ? o : 0;
      const int p = oo / PX, ch = oo - p * PX;
      const int lx = fx ? ow - 1 - p : p;
      const int sr = tr ? lx : ly, sc = tr ? ly : lx;
      const unsigned b = ldsb[sr * (PW * 4) + ((a_s0 + sr * a_sp) & 3) + sc * PX + ch];
      v |= (in[j] ? b : 0u) << (8 * j);
    }
    unsigned char* word = start + o0;
    if (in[0] && in[3]) {
      *(GlobalWord*)word = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) ((GlobalByte*)word)[j] = (unsigned char)(v >> (8 * j));
    }
  }
}

unsigned flags_of(int o) {
  static const unsigned k[9] = {0, 0, kMirrorX, kMirrorX | kMirrorY, kMirrorY, kTranspose, kTranspose | kMirrorX, kTranspose | kMirrorX | kMirrorY, kTranspose | kMirrorY};
  return k[o];
}

// the device copy of the table and the pinned staging it goes up through, borrowed for one call (ws_pool.hpp)
struct Workspace {
  int device = 0;
  DevBuf table;
  HostPinned stage;
  size_t held() const { return table.n + stage.n; }
};
// (never destroyed: nothing is freed at exit, when the runtime may be gone)
WsPool<Workspace>& g_pool = *new WsPool<Workspace>(WsPolicy{8, 0, 16u << 20}, delete_on_owner_device<Workspace>);

std::atomic<long long> g_images{0}, g_launches{0};

// the table of jobs[0..n) in t; returns the number of workgroups
long long fill_table(const OrientJob* jobs, int n, DOrient* t) {
  long long wg = 0;
  for (int i = 0; i < n; ++i) {
    const OrientJob& j = jobs[i];
    const int tiles_x = (j.w + T - 1) / T, tiles_y = (j.h + T - 1) / T;
    t[i] = DOrient{j.src, j.dst, j.src_pitch, j.dst_pitch, j.h, j.w, flags_of(j.o), (int)wg, tiles_x, 0};
    wg += (long long)tiles_x * tiles_y;
    FFP_CHECK(wg <= 0x7fffffffll, FFP_ERR_ARG, "image_orient: the batch has too many tiles");
  }
  return wg;
}

void launch(int px, long long wg, const DOrient* dt, int n, hipStream_t st) {
  if (px == 1) hipLaunchKernelGGL(orient_kernel<1>, dim3((unsigned)wg), dim3(kThreads), 0, st, dt, n);
  else if (px == 3) hipLaunchKernelGGL(orient_kernel<3>, dim3((unsigned)wg), dim3(kThreads), 0, st, dt, n);
  else hipLaunchKernelGGL(orient_kernel<4>, dim3((unsigned)wg), dim3(kThreads), 0, st, dt, n);
  FFP_HIP(hipGetLastError());
}

}  // namespace

void orient_check(const OrientJob& j, int px, long long dst_cap) {
  FFP_CHECK(px == 1 || px == 3 || px == 4, FFP_ERR_ARG, "image_orient: %d bytes per pixel (1, 3 and 4 are taken)", px);
  FFP_CHECK(j.o >= 1 && j.o <= 8, FFP_ERR_ARG, "image_orient: orientation %d (1..8 are the EXIF values)", j.o);
  FFP_CHECK(j.src && j.dst && j.h > 0 && j.w > 0, FFP_ERR_ARG, "image_orient: a %d x %d image%s", j.w, j.h, j.src && j.dst ? "" : " at a null pointer");
  const long long oh = orient_out_h(j), ow = orient_out_w(j);
  FFP_CHECK(j.src_pitch >= (long long)j.w * px, FFP_ERR_ARG, "image_orient: a source row pitch of %lld bytes for rows of %lld", j.src_pitch, (long long)j.w * px);
  FFP_CHECK(j.dst_pitch >= ow * px, FFP_ERR_ARG, "image_orient: a destination row pitch of %lld bytes for rows of %lld", j.dst_pitch, ow * px);
  const long long src_bytes = (j.h - 1) * j.src_pitch + (long long)j.w * px, dst_bytes = (oh - 1) * j.dst_pitch + ow * px;
  FFP_CHECK(dst_cap >= dst_bytes, FFP_ERR_ARG, "image_orient: the %lld x %lld destination needs %lld bytes, %lld are there", ow, oh, dst_bytes, dst_cap);
  const unsigned long long s = reinterpret_cast<unsigned long long>(j.src), t = reinterpret_cast<unsigned long long>(j.dst);
  FFP_CHECK(s + (unsigned long long)src_bytes <= t || t + (unsigned long long)dst_bytes <= s, FFP_ERR_ARG, "image_orient: source and destination overlap (the kernel is out of place)");
  FFP_CHECK(((long long)(j.h + T - 1) / T) * ((j.w + T - 1) / T) <= 0x3fffffffll, FFP_ERR_ARG, "image_orient: a %d x %d image has too many tiles", j.w, j.h);
}

void orient_batch_device(const OrientJob* jobs, int n, int px, hipStream_t st) {
  if (n <= 0) return;
  auto lease = lease_ws(g_pool, st);
  Workspace& ws = *lease;
  const size_t bytes = (size_t)n * sizeof(DOrient);
  ws.stage.ensure(bytes);
  ws.table.ensure(bytes);
  DOrient* t = static_cast<DOrient*>(ws.stage.p);
  const long long wg = fill_table(jobs, n, t);
  FFP_HIP(hipMemcpyAsync(ws.table.p, t, bytes, hipMemcpyHostToDevice, st));
  launch(px, wg, ws.table.as<DOrient>(), n, st);
  g_images.fetch_add(n);
  g_launches.fetch_add(1);
  FFP_HIP(hipStreamSynchronize(st));            // the workspace goes back to the pool with nothing in flight
}

void orient_time_device(const OrientJob& j, int px, int iters, float* kernel_us, float* copy_us, hipStream_t st) {
  auto lease = lease_ws(g_pool, st);
  Workspace& ws = *lease;
  ws.stage.ensure(sizeof(DOrient));
  ws.table.ensure(sizeof(DOrient));
  DOrient* t = static_cast<DOrient*>(ws.stage.p);
  const long long wg = fill_table(&j, 1, t);
  FFP_HIP(hipMemcpyAsync(ws.table.p, t, sizeof(DOrient), hipMemcpyHostToDevice, st));
  const size_t bytes = (size_t)j.h * j.w * px;
  struct Events {                                  // destroyed on every exit
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    Events() { for (hipEvent_t& x : e) FFP_HIP(hipEventCreate(&x)); }
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } events;
  hipEvent_t* ev = events.e;
  for (int i = 0; i < 3; ++i) launch(px, wg, ws.table.as<DOrient>(), 1, st);
  FFP_HIP(hipEventRecord(ev[0], st));
  for (int i = 0; i < iters; ++i) launch(px, wg, ws.table.as<DOrient>(), 1, st);
  FFP_HIP(hipEventRecord(ev[1], st));
  for (int i = 0; i < 3; ++i) FFP_HIP(hipMemcpyAsync(j.dst, j.src, bytes, hipMemcpyDeviceToDevice, st));
  FFP_HIP(hipEventRecord(ev[2], st));
  for (int i = 0; i < iters; ++i) FFP_HIP(hipMemcpyAsync(j.dst, j.src, bytes, hipMemcpyDeviceToDevice, st));
  FFP_HIP(hipEventRecord(ev[3], st));
  FFP_HIP(hipStreamSynchronize(st));
  float k = 0.f, c = 0.f;
  FFP_HIP(hipEventElapsedTime(&k, ev[0], ev[1]));
  FFP_HIP(hipEventElapsedTime(&c, ev[2], ev[3]));
  *kernel_us = k * 1e3f / iters;
  *copy_us = c * 1e3f / iters;
}

void orient_stats(long long* images, long long* launches) {
  if (images) *images = g_images.load();
  if (launches) *launches = g_launches.load();
}

}  // namespace ffp
