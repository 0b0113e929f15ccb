// png_dec.hip — PNG files read on the device, the counterpart of png.hip. A file this library wrote is thousands of independent deflate pieces (every
// IDAT chunk but the Adler one inflates without any other), so the decode is speculative: every IDAT payload ("span") is taken for such a piece.
//   png_inflate_kernel<false>   one wave per span: lengths and validity only (the span rules of png_inflate.hpp: decodes, uses exactly its bytes, no match
//                               reaches before the span's own output, ends the way a segment ends)
//   png_dec_scan_kernel         64-bit exclusive scan of the lengths, first failing span
//   png_inflate_kernel<true>    the same walk again, writing at the final offset: the span's output window is a 32 KiB ring in LDS (deflate's window: a valid
//                               span never looks further back), flushed to global memory in 16 KiB pieces, so a match reads LDS and never global memory
//                               the wave has just written. One lane walks the symbols; the wave builds the tables and copies.
//   png_adler_*_kernel          the Adler-32 of the inflated bytes, in a pass over the output (the arithmetic of png_gather_kernel)
//   png_unfilter_kernel         the five filters reversed as an anti-diagonal wavefront, the output format fused into the store
// If every span is self-contained, the lengths add up to h * (1 + w * bpp) and the Adler-32 matches, the result is what a serial decoder gives (it would be
// in the same state at every span start, and the history it carries is never referenced). Otherwise nothing of the speculative output is used: the host
// inflates the file (png_dec.cpp, the same core), the filtered stream goes up, and the same unfilter kernel runs.
// No workgroup waits for another: the only synchronisation is __syncthreads() and stream order. Every loop is bounded (see each).
#include <atomic>

#include "png_dec.hpp"
#include "png_inflate.hpp"

namespace ffp {

namespace {

constexpr int kRing = 32768, kRingMask = kRing - 1;   // deflate's window
constexpr int kFlush = 16384;                          // the ring is flushed in pieces of this size: what is not yet flushed stays below kFlush + 258 + 64
constexpr int kWin = 4096, kAhead = 2048;              // staged input: at least kAhead bytes (or the rest of the span) lie ahead of the reader in every round
constexpr int kStoredPiece = 4096;
constexpr unsigned kAdlerMod = 65521u;
constexpr int kAdlerChunk = 16384;
static_assert(kFlush + kStoredPiece + 258 + 64 <= kRing, "nothing unflushed is overwritten");
static_assert(256 * 6 + 8 <= kAhead && 600 + 8 <= kAhead, "a round of 256 tokens, or a dynamic block header, fits ahead of the reader");

struct DSpan { unsigned long long lo, hi; };           // bytes [lo, hi) of the file: an IDAT payload (the first without its zlib header)

struct InfCtl {                                        // what the walking lane tells the wave after each round
  int status, kind, len, dist, blk_type, blk_final;
  unsigned stored;
  unsigned long long pos, produced;
};

__device__ void stage_window(const unsigned char* __restrict__ file, unsigned* win, unsigned long long rpos, unsigned long long end, int lane, inf::Bits& b) {
  const unsigned long long base = rpos & ~3ull;        // the file's buffer is 256-byte aligned and padded: whole words may be read
  const unsigned long long hi = end < base + kWin ? end : base + kWin;
  const int nd = (int)((hi - base + 3) >> 2);
  for (int k = lane; k < nd; k += 64) win[k] = *(const unsigned*)(file + base + 4ull * (unsigned)k);
  b.base = base;
  b.wend = hi;
}

// bytes [from, to) of the span's output: ring -> out + off, words where the destination allows
__device__ void flush_ring(const unsigned char* ring, unsigned char* __restrict__ dst, unsigned long long from, unsigned long long to, int lane) {
  unsigned long long a = from;
  unsigned head = (unsigned)((4u - (unsigned)((uintptr_t)(dst + a) & 3u)) & 3u);
  if (head > to - a) head = (unsigned)(to - a);
  if ((unsigned)lane < head) dst[a + lane] = ring[(a + lane) & kRingMask];
  a += head;
  const unsigned nd = (unsigned)((to - a) >> 2);
  for (unsigned k = lane; k < nd; k += 64) {
    const unsigned long long p = a + 4ull * k;
    const unsigned v = (unsigned)ring[p & kRingMask] | ((unsigned)ring[(p + 1) & kRingMask] << 8) | ((unsigned)ring[(p + 2) & kRingMask] << 16) |
                       ((unsigned)ring[(p + 3) & kRingMask] << 24);
    *(unsigned*)(dst + p) = v;
  }
  a += 4ull * nd;
  if ((unsigned long long)lane < to - a) dst[a + lane] = ring[(a + lane) & kRingMask];
}

// One wave per span. Loop bounds: blocks by the span's bits (every block takes at least three), token rounds by the remaining output + 1 (every round but a
// block's last adds output), a round by 64 (256 without writing) tokens, a table walk by 15 bits, a copy by 258 bytes, a stored block by its 16-bit length.
template <bool WRITE>
__global__ void __launch_bounds__(64) png_inflate_kernel(const unsigned char* __restrict__ file, const DSpan* __restrict__ spans, int n_span, unsigned long long total,
                                                         const unsigned long long* __restrict__ out_off, unsigned char* __restrict__ out,
                                                         unsigned long long* __restrict__ span_len, int* __restrict__ span_status, int* __restrict__ bad_flag) {
  __shared__ unsigned ring_[WRITE ? kRing / 4 : 1];
  __shared__ unsigned win[kWin / 4 + 4];
  __shared__ inf::HuffLit hl;
  __shared__ inf::HuffDist hd;
  __shared__ inf::HuffLen hc;
  __shared__ unsigned char lens[inf::kLens];
  __shared__ InfCtl L;
  unsigned char* ring = (unsigned char*)ring_;
  const int s = blockIdx.x, lane = threadIdx.x;
  const DSpan sp = spans[s];
  const bool last = s == n_span - 1;
  const unsigned long long off = WRITE ? out_off[s] : 0ull;
  const unsigned long long cap = off <= total ? total - off : 0ull;
  unsigned char* dst = out + off;
  unsigned long long produced = 0, flushed = 0, rpos = sp.lo;
  inf::Bits b;
  inf::bits_init(b, (const unsigned char*)win, 0, 0, sp.lo, sp.hi);
  int status = inf::kOk;
  bool ended = false;
  const unsigned long long max_blocks = (sp.hi - sp.lo) * 3ull + 2ull;

  for (unsigned long long bi = 0; bi < max_blocks && !ended; ++bi) {
    if (rpos + kAhead > b.wend && b.wend < sp.hi) {
      __syncthreads();
      stage_window(file, win, rpos, sp.hi, lane, b);
      __syncthreads();
    }
    if (lane == 0) {
      inf::Block blk;
      int st = inf::block_begin(b, blk, lens, hc);
      if (!st && blk.type != 0) {
        st = inf::huff_build(hl, lens, inf::kLitSyms, false);
        if (!st) st = inf::huff_build(hd, lens + inf::kDistAt, inf::kDistSyms, true);
      }
      L.status = st; L.blk_type = blk.type; L.blk_final = blk.final; L.stored = blk.stored; L.pos = b.pos;
    }
    __syncthreads();
    status = L.status;
    if (status) break;
    const int type = L.blk_type, final = L.blk_final;
    rpos = L.pos;
    if (type == 0) {
      const unsigned len = L.stored;
      if (rpos + len > sp.hi) { status = inf::kEndsEarly; break; }
      if (produced + len > cap) { status = inf::kEndsLate; break; }
      if (WRITE) {
        for (unsigned done = 0; done < len; done += kStoredPiece) {
          const unsigned n = len - done < (unsigned)kStoredPiece ? len - done : (unsigned)kStoredPiece;
          for (unsigned k = lane; k < n; k += 64) ring[(produced + k) & kRingMask] = file[rpos + k];
          produced += n;
          rpos += n;
          __syncthreads();
          while (produced - flushed >= (unsigned long long)kFlush) { flush_ring(ring, dst, flushed, flushed + kFlush, lane); flushed += kFlush; }
          __syncthreads();
        }
      } else {
        produced += len;
        rpos += len;
      }
      b.pos = rpos; b.acc = 0; b.n = 0;                 // (lane 0 stood at the first stored byte with nothing buffered)
      if (!final && rpos == sp.hi) {                    // the end of a segment that is not the file's last
        if (last) status = inf::kNotSegment;
        ended = true;
        break;
      }
    } else {
      inf::huff_lut_clear(hl, lane, 64);
      inf::huff_lut_clear(hd, lane, 64);
      __syncthreads();
      inf::huff_lut_fill(hl, lens, lane, 64);
      inf::huff_lut_fill(hd, lens + inf::kDistAt, lane, 64);
      __syncthreads();
      bool eob = false;
      for (unsigned long long ti = 0; ti <= cap + 1ull && !eob; ++ti) {
        if (rpos + kAhead > b.wend && b.wend < sp.hi) {
          __syncthreads();
          stage_window(file, win, rpos, sp.hi, lane, b);
          __syncthreads();
        }
        if (lane == 0) {
          constexpr int kMaxTok = WRITE ? 64 : 256;
          unsigned long long p = produced;
          inf::Token t;
          t.kind = 0; t.val = 0; t.dist = 0;
          int st = inf::kOk, k = 0;
          for (; k < kMaxTok; ++k) {
            st = inf::next_token(b, hl, hd, t);
            if (st) break;
            if (t.kind == 0) {
              if (p + 1ull > cap) { st = inf::kEndsLate; break; }
              if (WRITE) ring[p & kRingMask] = (unsigned char)t.val;
              ++p;
            } else if (t.kind == 1) {
              if ((unsigned long long)t.dist > p) st = inf::kBadDistance;
              else if (p + (unsigned long long)t.val > cap) st = inf::kEndsLate;
              if (st || WRITE) break;                    // writing: the wave copies the match
              p += (unsigned long long)t.val;
            } else {
              break;
            }
          }
          L.status = st;
          L.kind = (k < kMaxTok && !st) ? t.kind : 0;
          L.len = t.val; L.dist = t.dist; L.produced = p; L.pos = b.pos;
        }
        __syncthreads();
        status = L.status;
        if (status) break;
        produced = L.produced;
        rpos = L.pos;
        const int kind = L.kind;
        if (WRITE && kind == 1) {
          const int len = L.len, dist = L.dist;
          const unsigned long long src = produced - (unsigned long long)dist;
          for (int i = lane; i < len; i += 64)          // an overlapping copy (dist < len) repeats its first dist bytes
            ring[(produced + (unsigned)i) & kRingMask] = ring[(src + (unsigned)(dist >= len ? i : i % dist)) & kRingMask];
          produced += (unsigned long long)len;
        }
        eob = kind == 2;
        if (WRITE && produced - flushed >= (unsigned long long)kFlush) {
          __syncthreads();
          flush_ring(ring, dst, flushed, flushed + kFlush, lane);
          flushed += kFlush;
        }
        __syncthreads();
      }
      if (status) break;
      if (!eob) { status = inf::kEndsLate; break; }
    }
    if (final) {
      if (lane == 0) L.pos = inf::bits_byte_pos(b);
      __syncthreads();
      if (!last || L.pos != sp.hi) status = inf::kNotSegment;
      ended = true;
    }
  }
  if (!ended && !status) status = inf::kNotSegment;
  __syncthreads();
  if (WRITE && !status && produced > flushed) flush_ring(ring, dst, flushed, produced, lane);
  if (lane == 0) {
    span_len[s] = produced;
    span_status[s] = status;
    if (status) atomicOr(bad_flag, 1);
  }
}

// off[0..n] = exclusive 64-bit prefix sum of len (one workgroup); verdict[0] = 1 + the first span with a status, or 0; verdict[1] = that status
__global__ void __launch_bounds__(1024) png_dec_scan_kernel(const unsigned long long* __restrict__ len, const int* __restrict__ status, int n,
                                                            unsigned long long* __restrict__ off, unsigned long long* __restrict__ verdict) {
  __shared__ unsigned long long part[1024];
  __shared__ int first_bad;
  const int tid = threadIdx.x, per = (n + 1023) / 1024;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  if (tid == 0) first_bad = n;
  __syncthreads();
  unsigned long long s = 0;
  for (int k = lo; k < hi; ++k) {
    s += len[k];
    if (status[k]) atomicMin(&first_bad, k);
  }
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long t = tid >= o ? part[tid - o] : 0ull;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  unsigned long long run = part[tid] - s;
  for (int k = lo; k < hi; ++k) { off[k] = run; run += len[k]; }
  if (tid == 1023) off[n] = part[1023];
  if (tid == 0) {
    verdict[0] = first_bad < n ? (unsigned long long)first_bad + 1ull : 0ull;
    verdict[1] = first_bad < n ? (unsigned long long)status[first_bad] : 0ull;
  }
}

// Adler-32 sums (A = sum of bytes, B = sum of (n - k) * byte k, both mod 65521) of each kAdlerChunk bytes of p[0, total)
__global__ void __launch_bounds__(256) png_adler_chunk_kernel(const unsigned char* __restrict__ p, unsigned long long total, unsigned* __restrict__ sums) {
  __shared__ unsigned tri[256][3];
  const int tid = threadIdx.x;
  const unsigned long long c0 = (unsigned long long)blockIdx.x * kAdlerChunk;
  constexpr int per = kAdlerChunk / 256;
  const unsigned long long lo = c0 + (unsigned long long)tid * per;
  const int len = lo >= total ? 0 : (total - lo < (unsigned long long)per ? (int)(total - lo) : per);
  unsigned a = 0, b = 0;
  for (int k = 0; k < len; ++k) { const unsigned v = p[lo + k]; a += v; b += (unsigned)(len - k) * v; }
  tri[tid][0] = a; tri[tid][1] = b; tri[tid][2] = (unsigned)len;
  __syncthreads();
  if (tid != 0) return;
  unsigned long long A = 0, B = 0;
  for (int t = 0; t < 256; ++t) {                          // appending part t: every earlier byte gains len_t in weight
    B = (B + (unsigned long long)tri[t][2] * A + tri[t][1]) % kAdlerMod;
    A = (A + tri[t][0]) % kAdlerMod;
  }
  sums[2 * (size_t)blockIdx.x] = (unsigned)A;
  sums[2 * (size_t)blockIdx.x + 1] = (unsigned)B;
}

__global__ void __launch_bounds__(256) png_adler_final_kernel(const unsigned* __restrict__ sums, long long n_chunk, unsigned long long total, unsigned* __restrict__ adler) {
  __shared__ unsigned tri[256][3];
  const int tid = threadIdx.x;
  const long long per = (n_chunk + 255) / 256, lo = min((long long)tid * per, n_chunk), hi = min(lo + per, n_chunk);
  unsigned long long A = 0, B = 0, N = 0;
  for (long long c = lo; c < hi; ++c) {
    const unsigned long long left = total - (unsigned long long)c * kAdlerChunk;
    const unsigned long long nc = left < (unsigned long long)kAdlerChunk ? left : (unsigned long long)kAdlerChunk;
    B = (B + (nc % kAdlerMod) * A + sums[2 * c + 1]) % kAdlerMod;
    A = (A + sums[2 * c]) % kAdlerMod;
    N = (N + nc) % kAdlerMod;
  }
  tri[tid][0] = (unsigned)A; tri[tid][1] = (unsigned)B; tri[tid][2] = (unsigned)N;
  __syncthreads();
  if (tid != 0) return;
  A = 0; B = 0; N = 0;
  for (int t = 0; t < 256; ++t) {
    const unsigned long long at = tri[t][0], bt = tri[t][1], nt = tri[t][2];
    B = (B + nt * A + bt) % kAdlerMod;
    A = (A + at) % kAdlerMod;
    N = (N + nt) % kAdlerMod;
  }
  const unsigned a = (unsigned)((1 + A) % kAdlerMod), bb = (unsigned)((N + B) % kAdlerMod);      // the initial a = 1 is in every b step
  *adler = (bb << 16) | a;
}

// ---- unfiltering ---------------------------------------------------------------------------------------------------------------------
// Byte (x, y) needs the reconstructed bytes at (x - bpp, y), (x, y - 1) and (x - bpp, y - 1). One workgroup walks the image band by band, kUnfRows rows at
// a time; each thread owns a row. Lane i trails lane i - 1 by one pixel, so the pixel above arrives through __shfl_up; wave v trails wave v - 1 by
// kUnfLag = 2 * kUnfCols pixels (its lane 0 needs what lane 63 of the wave above finished at least one step ago, and that lane is 63 pixels behind its own
// lane 0); the hand-off goes through an LDS ring, one __syncthreads() per step of kUnfCols pixels. The last row of a band is handed to the next band
// through a row in global memory, read back a step ahead by wave 0 into its own ring. A pixel is kept as one 64-bit word, byte lane q = byte q of the pixel.
constexpr int kUnfRows = 256, kUnfCols = 64, kUnfLag = 2 * kUnfCols, kUnfRingPx = 4 * kUnfCols, kUnfGroup = 16;
static_assert(kUnfCols % kUnfGroup == 0 && kUnfCols >= 64, "a step is whole groups and at least a wave's skew");

struct UnfArgs {
  const unsigned char* filt;       // h rows of 1 + w * bpp bytes
  long long filt_cap;              // bytes of filt that may be read, a multiple of 4
  int h, w, bgr;
  unsigned char* out;
  long long pitch;
  unsigned long long* carry;       // w pixels: the last row of the band before
  int* bad_flag;                   // [1] |= 1 on a filter type above 4
};

__device__ __forceinline__ int paeth_pred(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the words that cover the filtered bytes of pixels [x0, x0 + kUnfGroup) of a row, whatever their alignment; returns where the first byte lies in them.
// Words outside the buffer, and groups outside the row, read as zero.
template <int NDW, int BPP> __device__ __forceinline__ int load_group(const UnfArgs& A, bool live, long long rbase, int x0, unsigned (&r)[NDW]) {
  const long long lo = rbase + 1 + (long long)x0 * BPP, al = lo - (lo & 3);
  const bool any = live && x0 + kUnfGroup > 0 && x0 < A.w;
#pragma unroll
  for (int k = 0; k < NDW; ++k) {
    const long long at = al + 4 * k;
    r[k] = (any && at >= 0 && at + 4 <= A.filt_cap) ? *(const unsigned*)(A.filt + at) : 0u;
  }
  return (int)(lo - al);
}

template <int CH, int BPS> __global__ void __launch_bounds__(256) png_unfilter_kernel(const UnfArgs A) {
  constexpr int BPP = CH * BPS;
  constexpr int NDW = (kUnfGroup * BPP + 3) / 4 + 1;            // words that cover a group's bytes at any alignment
  __shared__ unsigned long long hand[4][kUnfRingPx];
  __shared__ unsigned slot[256][NDW + (NDW % 2 == 0 ? 1 : 0)];  // each thread's group of filtered bytes (odd pitch: no bank conflicts)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long rl = 1 + (long long)A.w * BPP;
  const int n_band = (A.h + kUnfRows - 1) / kUnfRows;
  const int n_step = (A.w + 63 + 3 * kUnfLag + kUnfCols - 1) / kUnfCols;
  const unsigned char* my = (const unsigned char*)slot[tid];
  for (int band = 0; band < n_band; ++band) {
    const int row = band * kUnfRows + tid;
    const bool live = row < A.h;
    const long long rbase = (long long)row * rl;
    int type = live ? A.filt[rbase] : 0;
    if (type > 4) { atomicOr(A.bad_flag + 1, 1); type = 0; }
    unsigned char* drow = A.out + (long long)row * A.pitch;
    unsigned long long left = 0, upleft = 0, mine = 0;
    if (wv == 0) hand[0][lane] = (band > 0 && lane < A.w) ? A.carry[lane] : 0ull;
    unsigned nxt[NDW];
    int skew_next = load_group<NDW, BPP>(A, live, rbase, -lane - wv * kUnfLag, nxt);
    __syncthreads();
    for (int step = 0; step < n_step; ++step) {
      if (wv == 0) {
        const int x = (step + 1) * kUnfCols + lane;
        hand[0][x & (kUnfRingPx - 1)] = (band > 0 && x < A.w) ? A.carry[x] : 0ull;
      }
      for (int g = 0; g < kUnfCols / kUnfGroup; ++g) {
        const int x0 = step * kUnfCols + g * kUnfGroup - lane - wv * kUnfLag;      // this thread's first pixel of the group (may lie outside the row)
        const int skew = skew_next;
#pragma unroll
        for (int k = 0; k < NDW; ++k) slot[tid][k] = nxt[k];
        skew_next = load_group<NDW, BPP>(A, live, rbase, x0 + kUnfGroup, nxt);        // the next group's bytes travel while this one is computed
#pragma unroll 4
        for (int j = 0; j < kUnfGroup; ++j) {
          const int x = x0 + j;
          unsigned long long above = __shfl_up(mine, 1);
          const bool inrow = x >= 0 && x < A.w;
          if (lane == 0) above = inrow ? hand[wv][x & (kUnfRingPx - 1)] : 0ull;
          unsigned long long cur = 0;
          if (live && inrow) {
            const unsigned long long a = x > 0 ? left : 0ull, c = x > 0 ? upleft : 0ull;
#pragma unroll
            for (int q = 0; q < BPP; ++q) {
              const int f = my[skew + j * BPP + q];
              const int pa = (int)((a >> (8 * q)) & 255u), pb = (int)((above >> (8 * q)) & 255u), pc = (int)((c >> (8 * q)) & 255u);
              const int pred = type == 0 ? 0 : type == 1 ? pa : type == 2 ? pb : type == 3 ? ((pa + pb) >> 1) : paeth_pred(pa, pb, pc);
              const unsigned v = (unsigned)(f + pred) & 255u;
              cur |= (unsigned long long)v << (8 * q);
              const int ch = q / BPS, kk = q - ch * BPS;
              const int oc = (CH >= 3 && A.bgr && ch < 3) ? 2 - ch : ch;
              drow[(long long)x * BPP + oc * BPS + (BPS == 2 ? 1 - kk : kk)] = (unsigned char)v;
            }
            left = cur;
          }
          upleft = above;
          mine = cur;
          if (lane == 63 && inrow) {
            if (wv < 3) hand[wv + 1][x & (kUnfRingPx - 1)] = cur;
            else A.carry[x] = cur;
          }
        }
      }
      __syncthreads();
    }
  }
}

template <int CH, int BPS> void launch_unfilter(const UnfArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((png_unfilter_kernel<CH, BPS>), dim3(1), dim3(256), 0, st, a);
}

// What one decode in flight holds, borrowed from a pool (ws_pool.hpp: one workspace per concurrent decode and device, as the JPEG decoder keeps them):
// the device buffers and the pinned staging: the file on its way up (serial route: the filtered stream), the scalars on their way back. No lock is held
// while a file is decoded.
struct Workspace {
  int device = 0;
  DevBuf file, filt, spans, span_len, span_status, off, small, sums, carry;
  HostPinned stage;
  size_t held() const { return file.n + filt.n + spans.n + span_len.n + span_status.n + off.n + small.n + sums.n + carry.n + stage.n; }
};
// at most 8 idle ones; a 16K frame's buffers are not kept (never destroyed: nothing is freed at exit, when the runtime may be gone)
WsPool<Workspace>& g_pool = *new WsPool<Workspace>(WsPolicy{8, 0, 768u << 20}, delete_on_owner_device<Workspace>);
std::atomic<long long> g_parallel{0}, g_serial{0};

// device words of Workspace::small
struct Small {
  unsigned long long verdict[2];
  int bad[2];                      // [0] a span failed in the writing pass, [1] a filter type above 4
  unsigned adler;
  unsigned pad;
};

void run_unfilter(Workspace& ws, const PngFile& f, int bgr, void* d_out, long long stride, hipStream_t st) {
  const long long want = f.filtered_len();
  ws.carry.ensure((size_t)f.w * sizeof(unsigned long long));
  UnfArgs a;
  a.filt = ws.filt.as<unsigned char>();
  a.filt_cap = (want + 3) & ~3ll;
  a.h = f.h; a.w = f.w; a.bgr = bgr;
  a.out = static_cast<unsigned char*>(d_out);
  a.pitch = stride;
  a.carry = ws.carry.as<unsigned long long>();
  a.bad_flag = ws.small.as<Small>()->bad;
  switch (f.channels * 10 + f.bit_depth / 8) {
    case 11: launch_unfilter<1, 1>(a, st); break;
    case 12: launch_unfilter<1, 2>(a, st); break;
    case 31: launch_unfilter<3, 1>(a, st); break;
    case 32: launch_unfilter<3, 2>(a, st); break;
    case 41: launch_unfilter<4, 1>(a, st); break;
    default: launch_unfilter<4, 2>(a, st); break;
  }
}

inline unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | (unsigned)p[3]; }

// the speculative route; false: nothing of it is used (d_out may have been written and is written again by the serial route)
bool decode_parallel(Workspace& ws, const unsigned char* data, long long n, const PngFile& f, int bgr, void* d_out, long long stride, hipStream_t st) {
  const int ns = (int)(f.idat.size() - 1);
  const unsigned long long want = (unsigned long long)f.filtered_len();
  std::vector<DSpan> spans((size_t)ns);
  for (int s = 0; s < ns; ++s) spans[s] = DSpan{(unsigned long long)f.idat[s].off + (s == 0 ? 2ull : 0ull), (unsigned long long)(f.idat[s].off + f.idat[s].len)};
  ws.stage.ensure((size_t)n + 64);
  std::memcpy(ws.stage.p, data, (size_t)n);
  ws.file.ensure((size_t)n + 64);
  ws.spans.ensure((size_t)ns * sizeof(DSpan));
  ws.span_len.ensure((size_t)ns * sizeof(unsigned long long));
  ws.span_status.ensure((size_t)ns * sizeof(int));
  ws.off.ensure(((size_t)ns + 1) * sizeof(unsigned long long));
  Small* sm = ws.small.as<Small>();
  Small* back = reinterpret_cast<Small*>(static_cast<unsigned char*>(ws.stage.p) + (((size_t)n + 15) & ~(size_t)15));
  FFP_HIP(hipMemcpyAsync(ws.file.p, ws.stage.p, (size_t)n, hipMemcpyHostToDevice, st));
  FFP_HIP(hipMemcpyAsync(ws.spans.p, spans.data(), sizeof(DSpan) * (size_t)ns, hipMemcpyHostToDevice, st));
  FFP_HIP(hipMemsetAsync(ws.small.p, 0, sizeof(Small), st));
  hipLaunchKernelGGL(png_inflate_kernel<false>, dim3((unsigned)ns), dim3(64), 0, st, ws.file.as<unsigned char>(), ws.spans.as<DSpan>(), ns, want,
                     (const unsigned long long*)nullptr, (unsigned char*)nullptr, ws.span_len.as<unsigned long long>(), ws.span_status.as<int>(), sm->bad);
  hipLaunchKernelGGL(png_dec_scan_kernel, dim3(1), dim3(1024), 0, st, ws.span_len.as<unsigned long long>(), ws.span_status.as<int>(), ns,
                     ws.off.as<unsigned long long>(), sm->verdict);
  unsigned long long total = 0;
  FFP_HIP(hipMemcpyAsync(back, sm, sizeof(Small), hipMemcpyDeviceToHost, st));
  FFP_HIP(hipMemcpyAsync(&total, ws.off.as<unsigned long long>() + ns, sizeof(total), hipMemcpyDeviceToHost, st));
  FFP_HIP(hipStreamSynchronize(st));                   // (spans lives on this stack frame)
  FFP_HIP(hipGetLastError());
  if (back->verdict[0] != 0 || total != want) return false;

  ws.filt.ensure((size_t)want + 64);
  const long long n_chunk = (long long)((want + kAdlerChunk - 1) / kAdlerChunk);
  ws.sums.ensure((size_t)n_chunk * 2 * sizeof(unsigned));
  FFP_HIP(hipMemsetAsync(ws.small.p, 0, sizeof(Small), st));
  hipLaunchKernelGGL(png_inflate_kernel<true>, dim3((unsigned)ns), dim3(64), 0, st, ws.file.as<unsigned char>(), ws.spans.as<DSpan>(), ns, want,
                     ws.off.as<unsigned long long>(), ws.filt.as<unsigned char>(), ws.span_len.as<unsigned long long>(), ws.span_status.as<int>(), sm->bad);
  hipLaunchKernelGGL(png_adler_chunk_kernel, dim3((unsigned)n_chunk), dim3(256), 0, st, ws.filt.as<unsigned char>(), want, ws.sums.as<unsigned>());
  hipLaunchKernelGGL(png_adler_final_kernel, dim3(1), dim3(256), 0, st, ws.sums.as<unsigned>(), n_chunk, want, &sm->adler);
  run_unfilter(ws, f, bgr, d_out, stride, st);
  FFP_HIP(hipMemcpyAsync(back, sm, sizeof(Small), hipMemcpyDeviceToHost, st));
  FFP_HIP(hipStreamSynchronize(st));
  FFP_HIP(hipGetLastError());
  const unsigned stored = be32(data + f.idat.back().off);
  return back->bad[0] == 0 && back->bad[1] == 0 && back->adler == stored;
}

void decode_serial(Workspace& ws, const unsigned char* data, const PngFile& f, int bgr, void* d_out, long long stride, hipStream_t st) {
  const long long want = f.filtered_len();
  ws.stage.ensure((size_t)want + 64);
  png_inflate_serial(data, f, static_cast<unsigned char*>(ws.stage.p));
  ws.filt.ensure((size_t)want + 64);
  FFP_HIP(hipMemcpyAsync(ws.filt.p, ws.stage.p, (size_t)want, hipMemcpyHostToDevice, st));
  FFP_HIP(hipMemsetAsync(ws.small.p, 0, sizeof(Small), st));
  run_unfilter(ws, f, bgr, d_out, stride, st);
  FFP_HIP(hipStreamSynchronize(st));
  FFP_HIP(hipGetLastError());
}

}  // namespace

void png_unfilter_geometry(int* rows_per_group, int* cols_per_step) {
  if (rows_per_group) *rows_per_group = kUnfRows;
  if (cols_per_step) *cols_per_step = kUnfCols;
}

void png_decode_stats(long long* parallel_decodes, long long* serial_decodes) {
  if (parallel_decodes) *parallel_decodes = g_parallel.load();
  if (serial_decodes) *serial_decodes = g_serial.load();
}

void png_decode_to_device(const unsigned char* data, long long n, const PngFile& f, int bgr, int flags, void* d_out, long long stride, long long cap, hipStream_t st) {
  const long long row = f.row_bytes();
  if (stride == 0) stride = row;
  FFP_CHECK(d_out && stride >= row, FFP_ERR_ARG, "png_decode: row pitch %lld is below the row's %lld bytes", stride, row);
  FFP_CHECK(cap >= (long long)(f.h - 1) * stride + row, FFP_ERR_ARG, "png_decode: output buffer too small for %d x %d x %d at %d bits (%lld bytes needed)", f.w, f.h,
            f.channels, f.bit_depth, (long long)(f.h - 1) * stride + row);
  FFP_CHECK((flags & ~kPngDecSerial) == 0, FFP_ERR_ARG, "png_decode: unknown flags 0x%x", flags);
  auto lease = lease_ws(g_pool, st);
  Workspace& ws = *lease;
  ws.small.ensure(sizeof(Small));
  bool done = false;
  if (!(flags & kPngDecSerial) && f.adler_alone && f.zlib_header && f.idat[0].len >= 2 && f.idat.size() - 1 < (1u << 30))
    done = decode_parallel(ws, data, n, f, bgr, d_out, stride, st);
  if (done) {
    g_parallel.fetch_add(1);
  } else {
    decode_serial(ws, data, f, bgr, d_out, stride, st);
    g_serial.fetch_add(1);
  }
}

}  // namespace ffp
