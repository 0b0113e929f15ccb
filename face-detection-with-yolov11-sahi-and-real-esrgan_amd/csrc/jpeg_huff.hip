// jpeg_huff.hip — Huffman decoding of a baseline JPEG scan ON THE DEVICE (what `cv2.imread` does first,
// reference call sites pipeline_v4_yolo/1_Inference.py:328-330, pipeline_v4_yolo/app_yolo_sahi.py:35). The file crosses PCIe as it is
// (1 MB for a 4K frame instead of 37 MB of coefficients) and the host only parses the markers.
//
// An entropy-coded segment is one serial bit stream, but Huffman streams SELF-SYNCHRONISE: a decoder started at a wrong bit position
// falls into step with the true symbol boundaries after a few dozen symbols. The decoder state between two symbols is
// (bit position, block of the MCU, zigzag index). The stream is cut into subsequences of SUB_BITS bits, one thread each:
//   1. unstuff: find the end of the entropy-coded data (first marker that is not RSTn), drop the 0x00 after every 0xFF and the RSTn
//      markers themselves (flags -> scan over 1 KiB tiles -> scatter); the clean offsets of the RSTn markers start the restart
//      SEGMENTS, whose first decoder state is known exactly, as is the one at the start of the scan;
//   2. sync (jhb_sync_kernel<true>): every thread decodes its subsequence from a cold state, then, per workgroup, threads adopt their
//      predecessor's exit state as entry state and decode again until nothing changes any more (a thread whose entry did not change
//      keeps its result, so after the first pass only the few not-yet-synchronised threads work);
//   3. the same across workgroups (jhb_sync_kernel<false>, repeated until no workgroup's last exit state changed: normally once);
//   4. an exclusive segmented scan over the subsequences of (blocks completed, sum of DC differences per component) gives every
//      thread its first block's index and the DC predictors at its entry;
//   5. write (jhb_write_kernel): decode once more from the now exact entry states and store the quantised coefficients, natural order,
//      into the planes jpeg_idct_batch_kernel (jpeg.hip) reads.
// Semantics are those of jpeg_dec.cpp (jdhuff.c); anything that decoder would treat specially — a bad code, a DC category above 11,
// a coefficient index past 63, a segment that does not hold exactly its MCUs, markers out of place — raises a flag instead, and
// jpeg_decode_batch_to_device repeats the file's decode with the host decoder, which reproduces libjpeg's behaviour on damaged streams.
// There is ONE orchestration, for n files (jpeg_decode_batch_to_device, at the end of this file; the layout: jpeg_batch_plan.hpp); a single
// file (jpeg_decode_to_device, jpeg.hip) is a batch of one.
// Parallel Huffman decoding by self-synchronisation: Klein & Wiseman 2003; for JPEG on GPUs: Weissenberger & Schmidt 2021.
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "exif.hpp"
#include "jpeg.hpp"
#include "jpeg_batch_plan.hpp"
#include "orient.hpp"

namespace ffp {

namespace {

constexpr int SUB_BITS = 512;                   // bits per subsequence: ~80 symbols of a quality-95 photograph
constexpr int NT = 128;                         // subsequences per workgroup
constexpr int FB = 10;                          // index bits of the fast table
constexpr int TILE = 1024;                      // bytes per unstuffing tile (256 threads x 4 bytes)
constexpr int LDS_WORDS = NT * SUB_BITS / 32 + 8;
static_assert(SUB_BITS == jbp::SUB_BITS && NT == jbp::NT && TILE == jbp::TILE && LDS_WORDS == jbp::LDS_WORDS, "jpeg_batch_plan.hpp sizes the batch by these");

__constant__ unsigned char kZig[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTabDev {                             // one table, as the decoding loop wants it (built on the device from the DHT segment)
  unsigned short lut[1 << FB];                  // FB-bit prefix -> length << 8 | symbol; 0: a longer code (or none)
  int maxcode[18];                              // [1..16] largest code of each length, -1: none
  int valoff[18];                               // [1..16] index of the first symbol of the length - its smallest code
  unsigned char vals[256];
};
static_assert(sizeof(HuffTabDev) % 16 == 0, "HuffTabDev is copied in 16-byte pieces");

struct HuffSpecDev { unsigned char bits[16]; unsigned char vals[256]; };

struct Scal {                                   // scalars the kernels hand to each other (and, at the end, to the host)
  int end;                                      // bytes of entropy-coded data before the terminating marker
  int total_clean;                              // bytes of the unstuffed stream
  int n_seg;                                    // restart segments
  int T;                                        // subsequences
  int changed;                                  // a workgroup's last exit state changed in the latest jhb_sync_kernel<false>
  int err;                                      // bit mask, see the E_ constants
  int pad[2];
};
enum { E_SEGS = 1, E_CODE = 2, E_DCCAT = 4, E_INDEX = 8, E_COUNT = 16, E_PHASE = 32, E_CAP = 64 };

struct HuffParams {
  int ncomp, bpm;                               // components, blocks per MCU
  int blk_comp[6], blk_dx[6], blk_dy[6];        // block j of an MCU: component and position inside the MCU
  int hs[3], vs[3], blocks_x[3];
  int mcus_x, total_mcus, dri;
  int n_raw;                                    // bytes handed over (from the first entropy-coded byte to the end of the file)
  int seg_cap, t_cap;                           // capacities of the segment / subsequence arrays
  short* coef[3];
};

struct Bufs {
  const unsigned char* raw;
  unsigned char* clean;
  unsigned long long* tile_cnt;                 // kept bytes | RSTn markers << 32 per tile; after the scan: exclusive prefix
  int* seg_start;                               // [n_seg + 1] clean byte offsets
  int* first_sub;                               // [n_seg + 1]
  unsigned* sub_start;                          // [T] bit offset in the clean stream
  int* sub_seg;                                 // [T]
  unsigned long long* entry;                    // [T] packed decoder states
  unsigned long long* exit_;                    // [T]
  int4* cnt;                                    // [T] blocks completed, DC difference sums
  int4* pref;                                   // [T] exclusive prefix inside the segment
  const HuffTabDev* tabs;                       // [3 components][DC, AC]
  Scal* scal;
};

__device__ __forceinline__ bool is_rst(unsigned b) { return b >= 0xD0u && b <= 0xD7u; }

// ---- 1. unstuffing ---------------------------------------------------------------------------------------------------------------------
// Every stage is a body that takes its workgroup's index `blk` INSIDE the file; the kernels further down look the file up and pass
// blk = blockIdx.x - the file's first workgroup (or tile).
__device__ __forceinline__ void jh_end_body(const Bufs& b, const HuffParams& P, int blk) {
  const int i0 = (blk * 256 + threadIdx.x) * 4;
  for (int i = i0; i < min(i0 + 4, P.n_raw); ++i) {
    if (b.raw[i] != 0xFF) continue;
    if (i + 1 >= P.n_raw) { atomicMin(&b.scal->end, i); continue; }          // a dangling 0xFF: the host decoder stops there too
    const unsigned m = b.raw[i + 1];
    if (!(m == 0 || m == 0xFF || is_rst(m))) atomicMin(&b.scal->end, i);
  }
}

// byte i < end of the raw stream: kept in the clean stream? an RSTn code byte?
__device__ __forceinline__ void classify(const unsigned char* raw, int i, int n, bool* keep, bool* rst) {
  const unsigned v = raw[i], prev = i > 0 ? raw[i - 1] : 0u;
  if (v == 0xFF) {
    *keep = i + 1 < n && raw[i + 1] == 0;       // a data byte 0xFF is followed by a stuffed zero; otherwise it opens a marker / is a fill byte
    *rst = false;
  } else {
    *keep = prev != 0xFF;                       // the byte after an 0xFF is the stuffed zero or a marker code
    *rst = prev == 0xFF && is_rst(v);
  }
}

__device__ __forceinline__ void jh_count_body(const Bufs& b, const HuffParams& P, int blk) {
  __shared__ unsigned s_keep, s_rst;
  if (threadIdx.x == 0) { s_keep = 0; s_rst = 0; }
  __syncthreads();
  const int end = b.scal->end;
  const int i0 = blk * TILE + threadIdx.x * 4;
  unsigned k = 0, r = 0;
  for (int i = i0; i < min(i0 + 4, end); ++i) {
    bool keep, rst;
    classify(b.raw, i, P.n_raw, &keep, &rst);
    k += keep; r += rst;
  }
  if (k) atomicAdd(&s_keep, k);
  if (r) atomicAdd(&s_rst, r);
  __syncthreads();
  if (threadIdx.x == 0) b.tile_cnt[blk] = (unsigned long long)s_keep | ((unsigned long long)s_rst << 32);
}

// exclusive scan of n 64-bit values by one workgroup of 1024 threads (each thread a contiguous run); returns the total
__device__ unsigned long long block_scan_u64(unsigned long long* v, int n) {
  __shared__ unsigned long long s_part[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024, lo = min(tid * per, n), hi = min(lo + per, n);
  unsigned long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += v[i];
  s_part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long a = tid >= o ? s_part[tid - o] : 0ull;
    __syncthreads();
    s_part[tid] += a;
    __syncthreads();
  }
  unsigned long long run = s_part[tid] - sum;
  for (int i = lo; i < hi; ++i) { const unsigned long long x = v[i]; v[i] = run; run += x; }
  const unsigned long long total = s_part[1023];
  __syncthreads();
  return total;
}

__device__ __forceinline__ void jh_scan_tiles_body(const Bufs& b, const HuffParams& P, int n_tiles, int n_seg_expected) {
  const unsigned long long total = block_scan_u64(b.tile_cnt, n_tiles);
  if (threadIdx.x == 0) {
    const int kept = (int)(unsigned)total, n_seg = (int)(total >> 32) + 1;
    b.scal->total_clean = kept;
    if (n_seg != n_seg_expected || n_seg > P.seg_cap) atomicOr(&b.scal->err, E_SEGS);
    b.scal->n_seg = min(n_seg, P.seg_cap);
    b.seg_start[min(n_seg, P.seg_cap)] = kept;
  }
}

__device__ __forceinline__ void jh_scatter_body(const Bufs& b, const HuffParams& P, int blk) {
  __shared__ unsigned s_k[256], s_r[256];
  const int end = b.scal->end, tid = threadIdx.x;
  const int i0 = blk * TILE + tid * 4;
  bool keep[4], rst[4];
  unsigned k = 0, r = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    keep[j] = rst[j] = false;
    if (i0 + j < end) classify(b.raw, i0 + j, P.n_raw, &keep[j], &rst[j]);
    k += keep[j]; r += rst[j];
  }
  s_k[tid] = k; s_r[tid] = r;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned ak = tid >= o ? s_k[tid - o] : 0u, ar = tid >= o ? s_r[tid - o] : 0u;
    __syncthreads();
    s_k[tid] += ak; s_r[tid] += ar;
    __syncthreads();
  }
  const unsigned long long base = b.tile_cnt[blk];
  unsigned ko = (unsigned)base + s_k[tid] - k, ro = (unsigned)(base >> 32) + s_r[tid] - r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (keep[j]) b.clean[ko++] = b.raw[i0 + j];
    if (rst[j]) { ++ro; if ((int)ro < P.seg_cap) b.seg_start[ro] = (int)ko; }       // segment `ro` starts where the marker stood
  }
}

// ---- subsequence layout ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jh_segs_body(const Bufs& b, const HuffParams& P, unsigned long long* tmp) {
  const int n_seg = b.scal->n_seg, total_clean = b.scal->total_clean;
  for (int k = threadIdx.x; k < n_seg; k += 1024) {
    const long long bits = (long long)(b.seg_start[k + 1] - b.seg_start[k]) * 8;
    tmp[k] = (unsigned long long)((bits + SUB_BITS - 1) / SUB_BITS);
    if (bits <= 0) atomicOr(&b.scal->err, E_SEGS);          // every MCU needs bits: an empty segment is a damaged file
  }
  // the decoders look ahead of the bits they consume, and a workgroup stages a fixed window: zeros behind the stream
  for (int i = threadIdx.x; i < LDS_WORDS * 4 + 64; i += 1024) b.clean[total_clean + i] = 0;
  __syncthreads();
  const unsigned long long Tl = block_scan_u64(tmp, n_seg);
  for (int k = threadIdx.x; k < n_seg; k += 1024) b.first_sub[k] = (int)tmp[k];
  const int T = (int)min(Tl, (unsigned long long)P.t_cap);
  if (threadIdx.x == 0) {
    b.first_sub[n_seg] = (int)Tl;
    if (Tl > (unsigned long long)P.t_cap) atomicOr(&b.scal->err, E_CAP);
    b.scal->T = T;
  }
  __syncthreads();
  // every subsequence's segment and first bit
  for (int t = threadIdx.x; t < T; t += 1024) {
    int lo = 0, hi = n_seg;                      // the last segment k with first_sub[k] <= t (empty segments share their successor's value)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int)tmp[mid] <= t) lo = mid; else hi = mid;
    }
    b.sub_seg[t] = lo;
    b.sub_start[t] = (unsigned)b.seg_start[lo] * 8u + (unsigned)(t - (int)tmp[lo]) * SUB_BITS;
  }
}

// ---- tables --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jh_tables_body(const HuffSpecDev* spec, HuffTabDev* tabs, const Bufs& b, const HuffParams& P, int blk) {
  __shared__ int s_min[17], s_ptr[17], s_max[17];
  if (blk == 0 && threadIdx.x == 0) {     // the scalars of this decode
    b.scal->end = P.n_raw; b.scal->total_clean = 0; b.scal->n_seg = 1; b.scal->T = 0; b.scal->changed = 0; b.scal->err = 0;
    b.seg_start[0] = 0;
  }
  const HuffSpecDev& sp = spec[blk];
  HuffTabDev& t = tabs[blk];
  if (threadIdx.x == 0) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      s_ptr[l] = k; s_min[l] = code;
      k += sp.bits[l - 1]; code += sp.bits[l - 1];
      s_max[l] = sp.bits[l - 1] ? code - 1 : -1;
      code <<= 1;
    }
    for (int l = 1; l <= 16; ++l) { t.maxcode[l] = s_max[l]; t.valoff[l] = s_ptr[l] - s_min[l]; }
    t.maxcode[0] = -1; t.valoff[0] = 0;
  }
  __syncthreads();
  t.vals[threadIdx.x] = sp.vals[threadIdx.x];
  for (int e = threadIdx.x; e < (1 << FB); e += 256) {
    unsigned short v = 0;
    for (int l = 1; l <= FB; ++l) {
      const int code = e >> (FB - l);
      if (code <= s_max[l] && code >= s_min[l]) { v = (unsigned short)((l << 8) | sp.vals[s_ptr[l] + code - s_min[l]]); break; }
    }
    t.lut[e] = v;
  }
}

// ---- the decoding loop -----------------------------------------------------------------------------------------------------------------------
struct HuffLds {
  HuffTabDev tab[6];                             // [component][DC, AC]
  unsigned words[LDS_WORDS];                     // the workgroup's part of the clean stream, big-endian words
  unsigned long long ex[NT];
};

__device__ __forceinline__ unsigned long long pack_state(unsigned p, int c, int z) { return ((unsigned long long)p << 16) | ((unsigned)c << 8) | (unsigned)z | (1ull << 63); }

// Decodes symbols from state (p, c, z) until the position reaches sub_end or the next symbol would cross seg_end. Counts completed
// blocks and sums DC differences per component; WRITE: stores the coefficients of block index `g` onwards, DC predictors in pred.
template <bool WRITE>
__device__ __forceinline__ void decode_run(const HuffLds& L, unsigned bit0, const HuffParams& P, unsigned sub_end, unsigned seg_end, unsigned& p_io, int& c_io, int& z_io,
                                           int4& cnt, long long g, long long g_end, int* err) {
  unsigned p = p_io;
  int c = c_io, z = z_io;
  int nblk = 0, dc[3] = {0, 0, 0};
  int pred[3] = {cnt.y, cnt.z, cnt.w};          // WRITE: predictors at entry come in through cnt
  int e = 0;
  // An adopted entry state can sit BELOW the workgroup's window base (the previous workgroup's last thread stopped early at the end of a
  // segment whose final subsequence is shorter than a word): p - bit0 would wrap and index far outside L.words. Such a state decodes
  // nothing here — it is handed on unchanged and flagged, so that a stream that ends up relying on it goes to the host decoder.
  if (p < bit0) {
    cnt = make_int4(0, WRITE ? cnt.y : 0, WRITE ? cnt.z : 0, WRITE ? cnt.w : 0);
    if (WRITE && err) *err = E_PHASE;
    return;
  }
  unsigned wi = (p - bit0) >> 5;
  unsigned long long acc = L.words[wi++];
  int nb = 32 - (int)((p - bit0) & 31u);
  short* blk = nullptr;
  bool have_blk = false;                        // the address of block g is worked out when its first coefficient is stored
  auto block_ptr = [&]() -> short* {
    if (g < 0 || g >= g_end) { e |= E_COUNT; return nullptr; }
    const long long m = g / P.bpm;
    const int j = (int)(g - m * P.bpm);
    if (j != c) { e |= E_PHASE; return nullptr; }
    const int comp = P.blk_comp[j], yy = (int)(m / P.mcus_x), xx = (int)(m - (long long)yy * P.mcus_x);
    return P.coef[comp] + ((size_t)(yy * P.vs[comp] + P.blk_dy[j]) * P.blocks_x[comp] + xx * P.hs[comp] + P.blk_dx[j]) * 64;
  };
  while (p < sub_end) {
    if (nb <= 32) { acc = (acc << 32) | L.words[wi++]; nb += 32; }
    const unsigned pk = (unsigned)(acc >> (nb - 16)) & 0xFFFFu;
    const int comp = P.blk_comp[c];
    const HuffTabDev& t = L.tab[comp * 2 + (z != 0)];
    const unsigned le = t.lut[pk >> (16 - FB)];
    int l = (int)(le >> 8), sym = (int)(le & 255u);
    if (l == 0) {
      for (l = FB + 1; l <= 16; ++l) {
        const int code = (int)(pk >> (16 - l));
        if (code <= t.maxcode[l]) { sym = t.vals[(t.valoff[l] + code) & 255]; break; }
      }
      if (l > 16) {                                                          // no such code: a decoder out of step, a damaged stream — or the
        if (p + 16u > seg_end) break;                                        // padding of the segment's last byte running into what follows it
        l = 16; sym = 0; e |= E_CODE;
      }
    }
    const int s = sym & 15, r = sym >> 4;
    const int total = l + s;
    if (p + (unsigned)total > seg_end) break;                                 // what is left of the segment is padding
    const unsigned extra = s ? (unsigned)(acc >> (nb - total)) & ((1u << s) - 1u) : 0u;
    const int val = s ? (extra < (1u << (s - 1)) ? (int)extra - (1 << s) + 1 : (int)extra) : 0;
    nb -= total;
    p += (unsigned)total;
    if (z == 0) {
      if (sym > 11) e |= E_DCCAT;
      dc[comp] += val;
      if (WRITE) {
        pred[comp] += val;
        if (!have_blk) { blk = block_ptr(); have_blk = true; }
        if (blk) blk[0] = (short)pred[comp];
      }
      z = 1;
    } else if (s == 0) {
      z = r == 15 ? z + 16 : 64;
    } else {
      z += r;
      if (z > 63) { e |= E_INDEX; z = 64; }
      else {
        if (WRITE) {
          if (!have_blk) { blk = block_ptr(); have_blk = true; }
          if (blk) blk[kZig[z]] = (short)val;
        }
        ++z;
      }
    }
    if (z >= 64) {
      z = 0;
      c = c + 1 == P.bpm ? 0 : c + 1;
      ++nblk;
      if (WRITE) { ++g; have_blk = false; }
    }
  }
  p_io = p; c_io = c; z_io = z;
  cnt = make_int4(nblk, dc[0], dc[1], dc[2]);
  if (WRITE && err) *err = e;
}

struct SubCtx { int t, seg; bool active, head; unsigned sub_start, sub_end, seg_end, bit0; };

// fills the workgroup's LDS (tables + its part of the stream) and the thread's subsequence
__device__ __forceinline__ SubCtx stage(const Bufs& b, HuffLds& L, int blk) {
  const int T = b.scal->T, tid = threadIdx.x;
  SubCtx x;
  x.t = blk * NT + tid;
  x.active = x.t < T;
  const int t0 = blk * NT;
  const unsigned start0 = b.sub_start[min(t0, T - 1)];
  x.bit0 = start0 & ~31u;
  x.seg = 0; x.head = false; x.sub_start = x.sub_end = x.seg_end = 0;
  if (x.active) {
    x.seg = b.sub_seg[x.t];
    x.head = x.t == b.first_sub[x.seg];
    x.sub_start = b.sub_start[x.t];
    x.seg_end = (unsigned)b.seg_start[x.seg + 1] * 8u;
    x.sub_end = min(x.sub_start + SUB_BITS, x.seg_end);
  }
  const uint4* src = reinterpret_cast<const uint4*>(b.tabs);
  uint4* dst = reinterpret_cast<uint4*>(L.tab);
  for (int i = tid; i < (int)(sizeof(HuffTabDev) * 6 / 16); i += NT) dst[i] = src[i];
  const unsigned* cw = reinterpret_cast<const unsigned*>(b.clean) + (x.bit0 >> 5);     // the clean buffer is padded with zeros past its end
  for (int i = tid; i < LDS_WORDS; i += NT) L.words[i] = __builtin_bswap32(cw[i]);
  __syncthreads();
  return x;
}

// 2./3. synchronisation. FIRST: cold start; otherwise continue from the stored states with the predecessor WORKGROUP's last exit state.
template <bool FIRST>
__device__ __forceinline__ void jh_sync_body(const Bufs& b, const HuffParams& P, HuffLds& L, int blk) {
  const SubCtx x = stage(b, L, blk);
  const int tid = threadIdx.x;
  unsigned long long entry = 0, exit_ = 0, exit_at_load = 0;
  int4 cnt = make_int4(0, 0, 0, 0);
  auto run = [&](unsigned long long en) {
    unsigned p = (unsigned)(en >> 16);
    int c = (int)(en >> 8) & 255, z = (int)en & 255;
    cnt = make_int4(0, 0, 0, 0);
    decode_run<false>(L, x.bit0, P, x.sub_end, x.seg_end, p, c, z, cnt, 0, 0, nullptr);
    entry = en;
    exit_ = pack_state(p, c, z);
  };
  bool changed = false;
  if (x.active) {
    if (FIRST) {
      run(pack_state(x.sub_start, 0, 0));        // exact for the head of a segment, a guess for everyone else
    } else {
      entry = b.entry[x.t]; exit_ = exit_at_load = b.exit_[x.t]; cnt = b.cnt[x.t];
      if (tid == 0 && !x.head && x.t > 0) {
        const unsigned long long ne = __hip_atomic_load(&b.exit_[x.t - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ne != entry) { run(ne); changed = true; }
      }
    }
  }
  if (FIRST || __syncthreads_or(changed)) {
    for (int iter = 0; iter <= NT; ++iter) {
      L.ex[tid] = exit_;
      __syncthreads();
      changed = false;
      if (x.active && !x.head && tid > 0) {
        const unsigned long long ne = L.ex[tid - 1];
        if (ne != entry) { run(ne); changed = true; }
      }
      if (!__syncthreads_or(changed)) break;
    }
  }
  if (x.active) {
    b.entry[x.t] = entry; b.cnt[x.t] = cnt;
    __hip_atomic_store(&b.exit_[x.t], exit_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!FIRST && exit_ != exit_at_load && (tid == NT - 1 || x.t == b.scal->T - 1)) atomicOr(&b.scal->changed, 1);
  }
}
// 4. exclusive segmented scan over the subsequences: one workgroup, every thread a contiguous run
__device__ __forceinline__ void jh_prefix_body(const Bufs& b) {
  __shared__ int4 s_sum[1024];
  __shared__ int s_flag[1024];
  const int T = b.scal->T, tid = threadIdx.x, per = (T + 1023) / 1024, lo = min(tid * per, T), hi = min(lo + per, T);
  auto add = [](int4 a, int4 c) { return make_int4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w); };
  int4 sum = make_int4(0, 0, 0, 0);
  int flag = 0;
  for (int t = lo; t < hi; ++t) {
    if (t == b.first_sub[b.sub_seg[t]]) { sum = make_int4(0, 0, 0, 0); flag = 1; }
    sum = add(sum, b.cnt[t]);
  }
  s_sum[tid] = sum; s_flag[tid] = flag;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {           // segmented inclusive scan: (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2)
    int4 a = make_int4(0, 0, 0, 0);
    int af = 0;
    if (tid >= o) { a = s_sum[tid - o]; af = s_flag[tid - o]; }
    __syncthreads();
    if (tid >= o) {
      if (!s_flag[tid]) s_sum[tid] = add(a, s_sum[tid]);
      s_flag[tid] |= af;
    }
    __syncthreads();
  }
  int4 run = tid > 0 ? s_sum[tid - 1] : make_int4(0, 0, 0, 0);
  for (int t = lo; t < hi; ++t) {
    if (t == b.first_sub[b.sub_seg[t]]) run = make_int4(0, 0, 0, 0);
    b.pref[t] = run;
    run = add(run, b.cnt[t]);
  }
}

// 5. the coefficients
__device__ __forceinline__ void jh_write_body(const Bufs& b, const HuffParams& P, HuffLds& L, int blk) {
  const SubCtx x = stage(b, L, blk);
  if (!x.active) return;
  const unsigned long long en = b.entry[x.t];
  unsigned p = (unsigned)(en >> 16);
  int c = (int)(en >> 8) & 255, z = (int)en & 255;
  const int4 pre = b.pref[x.t];
  const long long seg_mcus = P.dri ? min((long long)P.dri, (long long)P.total_mcus - (long long)x.seg * P.dri) : (long long)P.total_mcus;
  const long long g0 = (long long)x.seg * P.dri * P.bpm, g_end = g0 + seg_mcus * P.bpm;
  int4 cnt = make_int4(0, pre.y, pre.z, pre.w);
  int e = 0;
  decode_run<true>(L, x.bit0, P, x.sub_end, x.seg_end, p, c, z, cnt, g0 + pre.x, g_end, &e);
  if (x.sub_end == x.seg_end) {                  // the segment's last subsequence: exactly its MCUs, and nothing but padding left
    if (g0 + pre.x + cnt.x != g_end || c != 0 || z != 0 || x.seg_end - p >= 8u) e |= E_COUNT;
  }
  if (e) atomicOr(&b.scal->err, e);
}

// ---- the kernels: a batch of files in one pass -------------------------------------------------------------------------------------------
// Every file owns whole workgroups and whole unstuffing tiles (jpeg_batch_plan.hpp), and a descriptor in device memory with its Bufs and
// HuffParams. A kernel looks its file up and hands the stage body the workgroup's index inside the file; one file is a batch of one. Because
// a file's first subsequence is a segment head (its entry state is exact and it adopts nobody's exit state) and b.exit_ is the file's own
// array, nothing travels from one file's last subsequence into the next file's first.
struct BatchFile {
  Bufs b;
  HuffParams P;
  unsigned long long* tmp;
  const HuffSpecDev* spec;
  HuffTabDev* tabs;
  int wg0, tile0, n_tiles, n_seg_expected;
};

__global__ void __launch_bounds__(256) jhb_tables_kernel(const BatchFile* __restrict__ F) {
  const BatchFile& f = F[blockIdx.x / 6];
  jh_tables_body(f.spec, f.tabs, f.b, f.P, (int)(blockIdx.x % 6));
}
__global__ void __launch_bounds__(256) jhb_end_kernel(const BatchFile* __restrict__ F, const int* __restrict__ tile_file) {
  const BatchFile& f = F[tile_file[blockIdx.x]];
  jh_end_body(f.b, f.P, (int)blockIdx.x - f.tile0);
}
__global__ void __launch_bounds__(256) jhb_count_kernel(const BatchFile* __restrict__ F, const int* __restrict__ tile_file) {
  const BatchFile& f = F[tile_file[blockIdx.x]];
  jh_count_body(f.b, f.P, (int)blockIdx.x - f.tile0);
}
__global__ void __launch_bounds__(1024) jhb_scan_tiles_kernel(const BatchFile* __restrict__ F) {
  const BatchFile& f = F[blockIdx.x];
  jh_scan_tiles_body(f.b, f.P, f.n_tiles, f.n_seg_expected);
}
__global__ void __launch_bounds__(256) jhb_scatter_kernel(const BatchFile* __restrict__ F, const int* __restrict__ tile_file) {
  const BatchFile& f = F[tile_file[blockIdx.x]];
  jh_scatter_body(f.b, f.P, (int)blockIdx.x - f.tile0);
}
__global__ void __launch_bounds__(1024) jhb_segs_kernel(const BatchFile* __restrict__ F) {
  const BatchFile& f = F[blockIdx.x];
  jh_segs_body(f.b, f.P, f.tmp);
}
__global__ void __launch_bounds__(1024) jhb_prefix_kernel(const BatchFile* __restrict__ F) { jh_prefix_body(F[blockIdx.x].b); }

// the decoding loop indexes P by the block of the MCU: the file's copy goes to LDS next to its tables
__device__ __forceinline__ void load_params(const BatchFile& f, HuffParams& sP) {
  static_assert(sizeof(HuffParams) % 4 == 0 && sizeof(HuffParams) / 4 <= NT, "one word per thread");
  if (threadIdx.x < sizeof(HuffParams) / 4) reinterpret_cast<int*>(&sP)[threadIdx.x] = reinterpret_cast<const int*>(&f.P)[threadIdx.x];
  __syncthreads();
}
template <bool FIRST>
__global__ void __launch_bounds__(NT) jhb_sync_kernel(const BatchFile* __restrict__ F, const int* __restrict__ wg_file) {
  __shared__ HuffLds L;
  __shared__ HuffParams sP;
  const BatchFile& f = F[wg_file[blockIdx.x]];
  const int blk = (int)blockIdx.x - f.wg0;
  const Bufs b = f.b;
  if (blk * NT >= b.scal->T) return;
  load_params(f, sP);
  jh_sync_body<FIRST>(b, sP, L, blk);
}
__global__ void __launch_bounds__(NT) jhb_write_kernel(const BatchFile* __restrict__ F, const int* __restrict__ wg_file) {
  __shared__ HuffLds L;
  __shared__ HuffParams sP;
  const BatchFile& f = F[wg_file[blockIdx.x]];
  const int blk = (int)blockIdx.x - f.wg0;
  const Bufs b = f.b;
  if (blk * NT >= b.scal->T) return;
  load_params(f, sP);
  jh_write_body(b, sP, L, blk);
}

std::atomic<long long> g_stat_device{0}, g_stat_fallback{0}, g_stat_rounds{0};
std::atomic<long long> g_batch_count{0}, g_batch_launches{0}, g_batch_syncs{0};

// ---- workspaces ----------------------------------------------------------------------------------------------------------------------------
// The three arenas of jpeg_batch_plan.hpp and the pinned image of `up` (with the scalars' landing place behind it). A decode borrows one for
// its length (ws_pool.hpp), so decodes on different threads run side by side, each on its own stream. What stays pooled when nobody decodes:
// at most 32 workspaces, and per device at most one that holds more than kFrameBytes (a batch of many files, a 16K frame); a second such one
// is freed when it comes back.
struct BatchWs {
  HostPinned stage;
  DevBuf up, work, coef;
  int device = 0;                                // buffers live on the device that was current when the workspace was made
  size_t held() const { return stage.n + up.n + work.n + coef.n; }
};
constexpr size_t kFrameBytes = 160u << 20;       // above what a 3840 x 2160 frame takes: ~55 MiB at 4:2:0 quality 95, ~145 MiB at 4:4:4 with an 8 MB stream
// (never destroyed: nothing is freed at exit, when the runtime may be gone)
WsPool<BatchWs>& g_batch_pool = *new WsPool<BatchWs>(WsPolicy{32, kFrameBytes, 0}, delete_on_owner_device<BatchWs>);
// the images the turned files of ONE sub-batch (or one host-decoded file) are reconstructed into before the orient launch; at most one kept per
// device that holds more than a 4K frame, none above 256 MiB
struct TurnWs {
  DevBuf img;
  int device = 0;
  size_t held() const { return img.n; }
};
WsPool<TurnWs>& g_turn_pool = *new WsPool<TurnWs>(WsPolicy{8, 32u << 20, 256u << 20}, delete_on_owner_device<TurnWs>);
WsPool<JpegDecodeWs>& g_host_pool = *new WsPool<JpegDecodeWs>(WsPolicy{32, 0, 0}, delete_on_owner_device<JpegDecodeWs>);     // the host decoder's staging

// the host decoder for one file: a stream the device decoder flagged, a file outside its limits, everything under FFP_JPEG_HOST_HUFFMAN=1.
// It reproduces libjpeg's behaviour on damaged streams, and its refusals are the error reports of the decoding entries.
void host_decode_one(const unsigned char* data, long long n, JpegScan& s, unsigned char* d_out, long long stride, int bgr, hipStream_t st, JpegBatchCost& k) {
  auto ws = lease_ws(g_host_pool, st);
  ws->ensure_host(s);
  jpeg_entropy_decode(data, n, s, false);
  jpeg_reconstruct_device(s, *ws, d_out, stride, bgr, st);
  FFP_HIP(hipStreamSynchronize(st));             // the staging planes go back to the pool after this
  k.launches += 2; k.syncs += 1;
}

// Everything the kernels are told about one file — slot j of sub-batch S — written into hp, the pinned image of the `up` arena: its descriptor
// (Bufs, HuffParams), its rows of the workgroup -> file and tile -> file tables, quantisation tables, Huffman specs, IDCT and colour
// descriptors and the entropy-coded bytes. The caller has zeroed the tables of hp.
struct Arenas { unsigned char *hp, *up, *work, *coef; };
void fill_file(const Arenas& A, const jbp::SubPlan& S, const jbp::FilePlan& p, int j, const JpegScan& s, const JpegHead& head, const unsigned char* data, long long n_raw,
               unsigned char* out, long long stride) {
  unsigned char* const work = A.work;
  BatchFile& f = reinterpret_cast<BatchFile*>(A.hp + S.desc.off)[j];
  HuffParams& P = f.P;
  P.ncomp = s.ncomp;
  for (int c = 0; c < s.ncomp; ++c) {
    P.hs[c] = s.comp[c].hs; P.vs[c] = s.comp[c].vs; P.blocks_x[c] = s.comp[c].blocks_x;
    for (int dy = 0; dy < s.comp[c].vs; ++dy)
      for (int dx = 0; dx < s.comp[c].hs; ++dx) { P.blk_comp[P.bpm] = c; P.blk_dx[P.bpm] = dx; P.blk_dy[P.bpm] = dy; ++P.bpm; }       // the planner admitted bpm <= 6
    P.coef[c] = reinterpret_cast<short*>(A.coef + p.coef[c].off);
  }
  P.mcus_x = p.mcus_x; P.total_mcus = p.total_mcus; P.dri = head.dri; P.n_raw = (int)n_raw;
  P.seg_cap = p.seg_cap; P.t_cap = p.t_cap;
  Bufs& b = f.b;
  b.raw = A.up + p.raw.off; b.clean = work + p.clean.off;
  b.tile_cnt = reinterpret_cast<unsigned long long*>(work + p.tile_cnt.off);
  b.seg_start = reinterpret_cast<int*>(work + p.seg_start.off); b.first_sub = reinterpret_cast<int*>(work + p.first_sub.off);
  b.sub_start = reinterpret_cast<unsigned*>(work + p.sub_start.off); b.sub_seg = reinterpret_cast<int*>(work + p.sub_seg.off);
  b.entry = reinterpret_cast<unsigned long long*>(work + p.entry.off); b.exit_ = reinterpret_cast<unsigned long long*>(work + p.exit_.off);
  b.cnt = reinterpret_cast<int4*>(work + p.cnt.off); b.pref = reinterpret_cast<int4*>(work + p.pref.off);
  b.tabs = reinterpret_cast<const HuffTabDev*>(work + p.tabs.off); b.scal = reinterpret_cast<Scal*>(work + p.scal.off);
  f.tmp = reinterpret_cast<unsigned long long*>(work + p.tmp.off);
  f.spec = reinterpret_cast<const HuffSpecDev*>(A.up + S.spec.off) + (size_t)j * 6;
  f.tabs = reinterpret_cast<HuffTabDev*>(work + p.tabs.off);
  f.wg0 = p.wg0; f.tile0 = p.tile0; f.n_tiles = p.n_tiles; f.n_seg_expected = p.n_seg_expected;
  int* wg_file = reinterpret_cast<int*>(A.hp + S.wg_file.off);
  int* tile_file = reinterpret_cast<int*>(A.hp + S.tile_file.off);
  std::fill(wg_file + p.wg0, wg_file + p.wg0 + p.n_wg, j);
  std::fill(tile_file + p.tile0, tile_file + p.tile0 + p.n_tiles, j);
  std::memcpy(reinterpret_cast<unsigned short*>(A.hp + S.qt.off) + (size_t)j * 256, s.qt, sizeof(unsigned short) * 256);
  HuffSpecDev* specs = reinterpret_cast<HuffSpecDev*>(A.hp + S.spec.off) + (size_t)j * 6;
  JpegBatchIdct* idct = reinterpret_cast<JpegBatchIdct*>(A.hp + S.idct.off) + p.idct_slot0;
  for (int c = 0; c < s.ncomp; ++c) {
    for (int t = 0; t < 2; ++t) {
      const JpegHuffSpec& sp = t ? head.ac[s.comp[c].ta] : head.dc[s.comp[c].td];
      std::memcpy(specs[c * 2 + t].bits, sp.bits, 16);
      std::memcpy(specs[c * 2 + t].vals, sp.vals, (size_t)sp.n);
    }
    idct[c] = JpegBatchIdct{P.coef[c], work + p.plane[c].off, reinterpret_cast<const unsigned short*>(A.up + S.qt.off) + (size_t)j * 256 + 64 * s.comp[c].tq,
                            s.comp[c].blocks_x * s.comp[c].blocks_y, s.comp[c].blocks_x, p.idct_wg0[c], 0};
  }
  const int hsub = s.ncomp == 3 ? s.hmax : 1, vsub = s.ncomp == 3 ? s.vmax : 1;
  JpegBatchColour& cd = reinterpret_cast<JpegBatchColour*>(A.hp + S.colour.off)[j];
  cd.py = work + p.plane[0].off;
  cd.pcb = s.ncomp == 3 ? work + p.plane[1].off : nullptr;
  cd.pcr = s.ncomp == 3 ? work + p.plane[2].off : nullptr;
  cd.out = out; cd.stride = stride;
  cd.h = s.h; cd.w = s.w; cd.pitch_y = s.comp[0].blocks_x * 8; cd.pitch_c = s.ncomp == 3 ? s.comp[1].blocks_x * 8 : 0;
  cd.ch = (s.h + vsub - 1) / vsub; cd.cw = (s.w + hsub - 1) / hsub; cd.hsub = hsub; cd.vsub = vsub; cd.ncomp = s.ncomp;
  cd.wg0 = p.px_wg0; cd.wgs_x = p.px_wgs_x; cd.pad = 0;
  std::memcpy(A.hp + p.raw.off, data, (size_t)n_raw);
}

}  // namespace

void jpeg_huff_stats(long long* device_decodes, long long* host_fallbacks, long long* extra_sync_rounds) {
  if (device_decodes) *device_decodes = g_stat_device.load();
  if (host_fallbacks) *host_fallbacks = g_stat_fallback.load();
  if (extra_sync_rounds) *extra_sync_rounds = g_stat_rounds.load();
}

void jpeg_batch_stats(long long* batches, long long* launches_last_batch, long long* syncs_last_batch) {
  if (batches) *batches = g_batch_count.load();
  if (launches_last_batch) *launches_last_batch = g_batch_launches.load();
  if (syncs_last_batch) *syncs_last_batch = g_batch_syncs.load();
}
void jpeg_batch_note(const JpegBatchCost& k) {
  g_batch_count.fetch_add(1);
  g_batch_launches.store(k.launches);
  g_batch_syncs.store(k.syncs);
}

void jpeg_decode_batch_to_device(int n, const unsigned char* const* datas, const long long* sizes, int bgr, unsigned char* d_base, const long long* offsets,
                                 const long long* strides, long long cap, int* hs, int* ws, int* status, std::string* why, JpegBatchCost* cost, hipStream_t st,
                                 const int* orientations) {
  if (n <= 0) return;
  for (int i = 0; orientations && i < n; ++i)
    FFP_CHECK(orientations[i] >= 0 && orientations[i] <= 8, FFP_ERR_ARG, "jpeg_decode_batch: orientation %d of file %d (0: the file's own, 1..8: forced)", orientations[i], i);
  auto refuse = [&](int i, const Error& e) {
    status[i] = -e.code;
    if (why) why[i] = e.what();
  };
  // 1. the markers of every file; an unreadable one keeps its status and is not looked at again
  std::vector<JpegScan> scans((size_t)n);
  std::vector<JpegHead> heads((size_t)n);
  std::vector<unsigned char> readable((size_t)n, 0);
  std::vector<long long> stride((size_t)n, 0);
  // a turned file (EXIF orientation 2..8) is reconstructed into a pooled workspace image and turned into its region by ONE orient launch per
  // sub-batch (orient.hip); hs / ws, the pitch and the region's bounds are the ORIENTED image's
  std::vector<int> ori((size_t)n, 1);
  std::vector<long long> turn_off((size_t)n, 0);                      // inside the turn workspace, laid out anew for every sub-batch
  auto turn_slot = [&](int i) { return ((long long)scans[i].h * scans[i].w * 3 + 255) / 256 * 256; };
  for (int i = 0; i < n; ++i) {
    hs[i] = ws[i] = 0; status[i] = 0;
    if (why) why[i].clear();
    try {
      FFP_CHECK(datas[i] && sizes[i] > 0, FFP_ERR_ARG, "jpeg_decode_batch: no data");
      jpeg_entropy_decode(datas[i], sizes[i], scans[i], true, &heads[i]);
      if (orientations) ori[i] = orientations[i] ? orientations[i] : exif::orientation(datas[i], sizes[i]);
      hs[i] = ori[i] >= 5 ? scans[i].w : scans[i].h; ws[i] = ori[i] >= 5 ? scans[i].h : scans[i].w;
      readable[i] = 1;
    } catch (const Error& e) {
      refuse(i, e);
    }
  }
  // 2. every readable file's region inside cap, before anything is queued
  for (int i = 0; i < n; ++i) {
    if (!readable[i]) continue;
    const long long oh = hs[i], ow = ws[i];
    stride[i] = strides && strides[i] ? strides[i] : ow * 3;
    FFP_CHECK(offsets[i] >= 0 && stride[i] >= ow * 3 && offsets[i] <= cap && stride[i] * (oh - 1) + ow * 3 <= cap - offsets[i], FFP_ERR_ARG,
              "jpeg_decode_batch: image %d (%lldx%lld at offset %lld, row pitch %lld) does not lie inside the %lld bytes of the output", i, ow, oh, offsets[i], stride[i], cap);
  }
  // Borrowed by every call, allocated by the ones that turn a file, and sized for one sub-batch at a time: every sub-batch (and every host-decoded
  // file) ends in a synchronisation, so the next one may lay the workspace out again, or let it grow.
  WsPool<TurnWs>::Lease turn_lease = lease_ws(g_turn_pool, st);
  DevBuf& turn_img = turn_lease->img;
  // where file i is reconstructed, and the job that turns it into its region afterwards (both read the workspace as it is when they are called)
  auto raw_out = [&](int i) { return ori[i] != 1 ? turn_img.as<unsigned char>() + turn_off[i] : d_base + offsets[i]; };
  auto raw_stride = [&](int i) { return ori[i] != 1 ? (long long)scans[i].w * 3 : stride[i]; };
  auto turn_job = [&](int i) {
    return OrientJob{turn_img.as<unsigned char>() + turn_off[i], d_base + offsets[i], (long long)scans[i].w * 3, stride[i], scans[i].h, scans[i].w, ori[i]};
  };
  // 3. the layout: every buffer of the device decoder is sized here, from header fields the planner has checked. Not an error of the file but a
  // limit of THIS decoder (the host decoder takes the file): 32-bit bit offsets (a scan + trailer of 256 MiB or more), six blocks per MCU
  std::vector<jbp::FileIn> in((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!readable[i]) continue;
    const JpegScan& s = scans[i];
    jbp::FileIn& f = in[i];
    f.n_raw = sizes[i] - heads[i].data_off; f.h = s.h; f.w = s.w; f.ncomp = s.ncomp; f.dri = heads[i].dri;
    for (int c = 0; c < s.ncomp; ++c) { f.hs[c] = s.comp[c].hs; f.vs[c] = s.comp[c].vs; f.blocks_x[c] = s.comp[c].blocks_x; f.blocks_y[c] = s.comp[c].blocks_y; }
  }
  const bool host_only = sw().jpeg_host_huffman;  // FFP_JPEG_HOST_HUFFMAN=1: entropy decoding on the host for every file (A/B and the fallback's own tests)
  std::vector<unsigned char> for_device = readable;
  if (host_only) std::fill(for_device.begin(), for_device.end(), 0);
  const jbp::Sizes sz{(long long)sizeof(BatchFile), (long long)sizeof(JpegBatchIdct), (long long)sizeof(JpegBatchColour), (long long)sizeof(HuffTabDev),
                      (long long)sizeof(HuffSpecDev), (long long)sizeof(Scal)};
  const jbp::Plan plan = jbp::plan_batch(in.data(), for_device.data(), n, sz);

  JpegBatchCost k;
  std::vector<unsigned char> to_host((size_t)n, 0);
  for (int i = 0; i < n; ++i) to_host[i] = readable[i] && plan.files[i].sub < 0;
  if (!plan.subs.empty()) {
    auto lease = lease_ws(g_batch_pool, st);
    BatchWs& W = *lease;
    for (const jbp::SubPlan& S : plan.subs) {
      const int m = (int)S.files.size();
      const size_t scal_host = (size_t)jbp::align_up(S.up_bytes);
      W.stage.ensure(scal_host + (size_t)S.scal.bytes);
      if ((size_t)S.up_bytes > W.up.n) W.up.alloc((size_t)S.up_bytes * 5 / 4);
      if ((size_t)S.work_bytes > W.work.n) W.work.alloc((size_t)S.work_bytes * 5 / 4);
      if ((size_t)S.coef_bytes > W.coef.n) W.coef.alloc((size_t)S.coef_bytes * 5 / 4);
      const Arenas A{static_cast<unsigned char*>(W.stage.p), W.up.as<unsigned char>(), W.work.as<unsigned char>(), W.coef.as<unsigned char>()};
      std::memset(A.hp, 0, (size_t)S.spec.off + (size_t)S.spec.bytes);          // the tables; the raw bytes behind them are copied in by fill_file
      long long turn_bytes = 0;
      for (int j = 0; j < m; ++j)
        if (ori[S.files[j]] != 1) { turn_off[S.files[j]] = turn_bytes; turn_bytes += turn_slot(S.files[j]); }
      if (turn_bytes > 0) turn_img.ensure((size_t)turn_bytes);
      for (int j = 0; j < m; ++j) {
        const int i = S.files[j];
        fill_file(A, S, plan.files[i], j, scans[i], heads[i], datas[i] + heads[i].data_off, in[i].n_raw, raw_out(i), raw_stride(i));
      }
      const BatchFile* dF = reinterpret_cast<const BatchFile*>(A.up + S.desc.off);
      const int* d_wg_file = reinterpret_cast<const int*>(A.up + S.wg_file.off);
      const int* d_tile_file = reinterpret_cast<const int*>(A.up + S.tile_file.off);
      JpegBatchColour* hC = reinterpret_cast<JpegBatchColour*>(A.hp + S.colour.off);
      Scal* h_scal = reinterpret_cast<Scal*>(A.hp + scal_host);
      auto download = [&]() {
        FFP_HIP(hipMemcpyAsync(h_scal, A.work + S.scal.off, (size_t)S.scal.bytes, hipMemcpyDeviceToHost, st));
        FFP_HIP(hipStreamSynchronize(st));
        k.syncs += 1;
      };
      auto scan_and_write = [&]() {
        hipLaunchKernelGGL(jhb_prefix_kernel, dim3(m), dim3(1024), 0, st, dF);
        hipLaunchKernelGGL(jhb_write_kernel, dim3(S.n_wg), dim3(NT), 0, st, dF, d_wg_file);
        k.launches += 2;
      };
      // the whole entropy decode is queued under the assumption that ONE round of synchronisation across workgroups is enough — it practically
      // always is; the scalars that come down say whether it was
      FFP_HIP(hipMemcpyAsync(A.up, A.hp, (size_t)S.up_bytes, hipMemcpyHostToDevice, st));
      FFP_HIP(hipMemsetAsync(A.coef, 0, (size_t)S.coef_bytes, st));
      hipLaunchKernelGGL(jhb_tables_kernel, dim3(m * 6), dim3(256), 0, st, dF);
      hipLaunchKernelGGL(jhb_end_kernel, dim3(S.n_tiles), dim3(256), 0, st, dF, d_tile_file);
      hipLaunchKernelGGL(jhb_count_kernel, dim3(S.n_tiles), dim3(256), 0, st, dF, d_tile_file);
      hipLaunchKernelGGL(jhb_scan_tiles_kernel, dim3(m), dim3(1024), 0, st, dF);
      hipLaunchKernelGGL(jhb_scatter_kernel, dim3(S.n_tiles), dim3(256), 0, st, dF, d_tile_file);
      hipLaunchKernelGGL(jhb_segs_kernel, dim3(m), dim3(1024), 0, st, dF);
      hipLaunchKernelGGL(jhb_sync_kernel<true>, dim3(S.n_wg), dim3(NT), 0, st, dF, d_wg_file);
      hipLaunchKernelGGL(jhb_sync_kernel<false>, dim3(S.n_wg), dim3(NT), 0, st, dF, d_wg_file);
      k.launches += 8;
      scan_and_write();
      FFP_HIP(hipGetLastError());
      // The reconstruction is NOT queued blindly: it writes into the caller's memory, and the region of a file that is not decoded in the end
      // (flagged here, then refused by the host decoder too) has to stay untouched. So the scalars come down first, and the two reconstruction
      // launches follow with the flagged files blanked out: two synchronisations per sub-batch, always.
      download();
      std::vector<int> sticky((size_t)m, 0);
      bool more = false;
      for (int j = 0; j < m; ++j) {
        sticky[j] = h_scal[j].err & (E_SEGS | E_CAP);
        if (h_scal[j].changed && !sticky[j]) more = true;
      }
      if (more) {
        // some workgroup's last exit state moved in the round that was queued blindly: rounds for the sub-batch until none moves (information
        // travels at least one workgroup per round), then the scan and the write pass again, for all files (the ones that did not move get the
        // same coefficients again)
        int rounds = 0;
        const int limit = S.n_wg + 2;
        do {
          FFP_HIP(hipMemset2DAsync(A.work + S.scal.off + offsetof(Scal, changed), sizeof(Scal), 0, sizeof(int), (size_t)m, st));
          hipLaunchKernelGGL(jhb_sync_kernel<false>, dim3(S.n_wg), dim3(NT), 0, st, dF, d_wg_file);
          k.launches += 1;
          download();
          g_stat_rounds.fetch_add(1);
          more = false;
          for (int j = 0; j < m; ++j) more = more || (h_scal[j].changed && !sticky[j]);
        } while (more && ++rounds < limit);
        for (int j = 0; j < m; ++j)
          if (h_scal[j].changed) sticky[j] |= E_CAP;                             // did not settle: the host decoder
        FFP_HIP(hipMemset2DAsync(A.work + S.scal.off + offsetof(Scal, err), sizeof(Scal), 0, sizeof(int), (size_t)m, st));     // flags of the premature write pass
        FFP_HIP(hipMemsetAsync(A.coef, 0, (size_t)S.coef_bytes, st));
        scan_and_write();
        download();
      }
      // files whose flags are set leave the batch: blank out their colour descriptors (h = 0: no pixel is written), the rest is reconstructed
      bool any_bad = false;
      for (int j = 0; j < m; ++j)
        if (h_scal[j].err | sticky[j]) { hC[j].h = 0; to_host[S.files[j]] = 1; any_bad = true; }
      if (any_bad) FFP_HIP(hipMemcpyAsync(A.up + S.colour.off, hC, (size_t)S.colour.bytes, hipMemcpyHostToDevice, st));
      jpeg_batch_reconstruct(reinterpret_cast<const JpegBatchIdct*>(A.up + S.idct.off), S.n_idct, S.n_idct_wg, reinterpret_cast<const JpegBatchColour*>(A.up + S.colour.off), m,
                             S.n_px_wg, bgr, st);
      k.launches += 2;
      std::vector<OrientJob> jobs;
      for (int j = 0; j < m; ++j)
        if (ori[S.files[j]] != 1 && !to_host[S.files[j]]) jobs.push_back(turn_job(S.files[j]));
      if (!jobs.empty()) {
        orient_batch_device(jobs.data(), (int)jobs.size(), 3, st);               // one launch for the sub-batch's turned files; waits for the stream
        k.launches += 1;
      } else {
        FFP_HIP(hipStreamSynchronize(st));
      }
      k.syncs += 1;
      for (int j = 0; j < m; ++j)
        if (!to_host[S.files[j]]) g_stat_device.fetch_add(1);
    }
  }
  // 4. the host decoder, file by file, for what the device decoder did not take or gave up on
  for (int i = 0; i < n; ++i) {
    if (!to_host[i]) continue;
    if (!host_only) g_stat_fallback.fetch_add(1);
    try {
      if (ori[i] != 1) { turn_off[i] = 0; turn_img.ensure((size_t)turn_slot(i)); }
      host_decode_one(datas[i], sizes[i], scans[i], raw_out(i), raw_stride(i), bgr, st, k);
      if (ori[i] != 1) {
        const OrientJob job = turn_job(i);
        orient_batch_device(&job, 1, 3, st);
        k.launches += 1; k.syncs += 1;
      }
      status[i] = 1;
    } catch (const Error& e) {
      refuse(i, e);
    }
  }
  if (cost) *cost = k;
}

}  // namespace ffp
