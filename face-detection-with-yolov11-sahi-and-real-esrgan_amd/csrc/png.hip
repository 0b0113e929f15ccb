// png.hip — PNG files written on the device (the half jpeg.hip does not cover): the image never crosses PCIe
// uncompressed, only the finished file does. Three stages, every one of them independent work per row / segment / image:
//   png_filter_kernel     one workgroup per row: the five PNG filters, libpng's minimum-sum-of-absolute-differences choice, the
//                         filtered row (filter byte first) into the filtered stream
//   png_deflate_kernel    one wave per kPngSegmentBytes of filtered stream: LZ77 (hash heads in LDS, matches never reach before the
//                         segment) parsed twice — once for the symbol counts, once to emit — around the choice between the fixed
//                         Huffman code, a dynamic one built from the counts, and a stored block; every segment but the last ends with
//                         an empty stored block (byte boundary, the pigz construction); the wave wraps its bytes in one IDAT chunk with
//                         its CRC-32 and leaves the segment's Adler-32 sums
//   png_scan_kernel / png_gather_kernel   prefix sum of the chunk sizes; chunks copied from their worst-case slots to their final
//                         offsets; signature, IHDR, the Adler-32 trailer (its own 4-byte IDAT) and IEND per image
// What a PNG reader decodes is the contract (tests/test_gpu_png.py), not libpng's bytes.
#include <vector>

#include "png.hpp"

namespace ffp {

namespace {

constexpr int kSeg = kPngSegmentBytes;
constexpr int kSlot = kSeg + 32;       // a chunk at its worst: length + type (8), zlib header (2), stored-block header (5), S, CRC (4); 16-byte multiple
constexpr int kHashBits = 12;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kTooFar = 4096;          // a 3-byte match further back than this costs more than three literals (zlib's TOO_FAR)
constexpr int kFileFixed = 8 + 25 + 16 + 12;   // signature, IHDR, the Adler IDAT, IEND
constexpr unsigned kAdlerMod = 65521u;
static_assert(kSeg >= 4096 && (kSeg & (kSeg - 1)) == 0 && kSeg <= 32768, "segment: a power of two, at least 4096, inside deflate's window");
static_assert(kSlot % 16 == 0, "slots keep 16-byte alignment");

struct PngImg {
  const unsigned char* src;
  long long stride;      // bytes between rows of src
  long long filt_off;    // this image's filtered stream inside the workspace (16-byte aligned)
  long long filt_len;    // h * (1 + w * bpp)
  int h, w;
  int first_seg, n_seg;
};

// ---- filtering --------------------------------------------------------------------------------------------------------------------
// byte x of a row as the file holds it: RGB(A) order, 16-bit samples big-endian
template <int CH, int BPS> __device__ __forceinline__ int raw_byte(const unsigned char* row, int x, int bgr) {
  constexpr int BPP = CH * BPS;
  const int px = x / BPP, r = x - px * BPP;
  int c = r / BPS;
  const int k = r - c * BPS;
  if (CH >= 3 && bgr && c < 3) c = 2 - c;
  return row[(long long)px * BPP + c * BPS + (BPS == 2 ? 1 - k : k)];
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

template <int CH, int BPS> __global__ void __launch_bounds__(256) png_filter_kernel(const PngImg im, int bgr, unsigned char* __restrict__ filt) {
  constexpr int BPP = CH * BPS;
  __shared__ unsigned long long red[5][4];
  __shared__ int chosen;
  const int r = blockIdx.x, tid = threadIdx.x, rb = im.w * BPP;
  const unsigned char* cur = im.src + (long long)r * im.stride;
  const unsigned char* up = r > 0 ? cur - im.stride : nullptr;   // the row above the first row is zeros
  unsigned long long s[5] = {0, 0, 0, 0, 0};
  for (int x = tid; x < rb; x += 256) {
    const int v = raw_byte<CH, BPS>(cur, x, bgr);
    const int a = x >= BPP ? raw_byte<CH, BPS>(cur, x - BPP, bgr) : 0;
    const int b = up ? raw_byte<CH, BPS>(up, x, bgr) : 0;
    const int c = (up && x >= BPP) ? raw_byte<CH, BPS>(up, x - BPP, bgr) : 0;
    const int f[5] = {v, (v - a) & 255, (v - b) & 255, (v - ((a + b) >> 1)) & 255, (v - paeth(a, b, c)) & 255};
#pragma unroll
    for (int t = 0; t < 5; ++t) s[t] += (unsigned)(f[t] < 128 ? f[t] : 256 - f[t]);
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    unsigned long long v = s[t];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red[t][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    unsigned long long bs = ~0ull;
    for (int t = 0; t < 5; ++t) {
      const unsigned long long v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
      if (v < bs) { bs = v; best = t; }      // ties: the lowest type number
    }
    chosen = best;
  }
  __syncthreads();
  const int type = chosen;
  unsigned char* dst = filt + im.filt_off + (long long)r * (rb + 1);
  if (tid == 0) dst[0] = (unsigned char)type;
  for (int x = tid; x < rb; x += 256) {
    const int v = raw_byte<CH, BPS>(cur, x, bgr);
    int pred = 0;
    if (type != 0) {
      const int a = x >= BPP ? raw_byte<CH, BPS>(cur, x - BPP, bgr) : 0;
      const int b = up ? raw_byte<CH, BPS>(up, x, bgr) : 0;
      const int c = (up && x >= BPP) ? raw_byte<CH, BPS>(up, x - BPP, bgr) : 0;
      pred = type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    }
    dst[1 + x] = (unsigned char)(v - pred);
  }
}

// ---- CRC-32 -----------------------------------------------------------------------------------------------------------------------
// The register update is linear over GF(2), so a wave splits a chunk among its lanes: lane 0 starts from the all-ones register, the
// others from zero, and each lane's register is advanced over the bytes behind its part by a multiplication with x^(8 * bytes) modulo
// the polynomial (the arithmetic of zlib's crc32_combine, reflected representation: x^k is bit 31 - k).
__device__ __forceinline__ unsigned crc_byte(unsigned c, unsigned b) {
  c ^= b;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}
__device__ unsigned crc_mul(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int k = 0; k < 32; ++k) {
    if (a & (0x80000000u >> k)) p ^= b;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}
__device__ unsigned crc_xpow8(unsigned n_bytes) {    // x^(8 * n_bytes)
  unsigned p = 0x80000000u, sq = 0x00800000u;         // 1, x^8
  for (int k = 0; k < 32 && n_bytes; ++k, n_bytes >>= 1) {
    if (n_bytes & 1u) p = crc_mul(sq, p);
    sq = crc_mul(sq, sq);
  }
  return p;
}
__device__ unsigned crc_serial(const unsigned char* p, int n) {     // short strings (IHDR, the Adler chunk, IEND): one thread
  unsigned c = 0xFFFFFFFFu;
  for (int k = 0; k < n; ++k) c = crc_byte(c, p[k]);
  return ~c;
}
__device__ __forceinline__ void put_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

// ---- deflate ----------------------------------------------------------------------------------------------------------------------
struct SegLds {
  unsigned data[kSeg / 4 + 4];          // the segment
  unsigned head[1 << kHashBits];        // hash of three bytes -> 1 + the latest position seen with it (0: none)
  unsigned out[kSlot / 4];              // the IDAT chunk under construction
  unsigned freq[320];                   // literal/length symbols 0..287, distance symbols at 288..
  unsigned code[320];                   // (code, bit-reversed for the LSB-first packer) << 4 | length
  unsigned tmp[64 * 3];
};
constexpr int kDistBase = 288;

__device__ __forceinline__ int len_sym(int len, int* extra_bits, int* extra_val) {
  const int x = len - 3;
  if (x < 8 || len == 258) { *extra_bits = 0; *extra_val = 0; return len == 258 ? 285 : 257 + x; }
  const int e = 29 - __clz(x);           // floor(log2 x) - 2
  *extra_bits = e; *extra_val = x & ((1 << e) - 1);
  return 261 + 4 * e + ((x >> e) & 3);
}
__device__ __forceinline__ int dist_sym(int dist, int* extra_bits, int* extra_val) {
  const int x = dist - 1;
  if (x < 4) { *extra_bits = 0; *extra_val = 0; return x; }
  const int n = 31 - __clz(x), e = n - 1;
  *extra_bits = e; *extra_val = x & ((1 << e) - 1);
  return 2 * n + ((x >> e) & 1);
}
__device__ __forceinline__ int len_sym_extra(int s) { return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0; }
__device__ __forceinline__ int dist_sym_extra(int t) { return t >= 4 ? (t >> 1) - 1 : 0; }
__device__ __forceinline__ int fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

__device__ __forceinline__ unsigned long long low_mask(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1ull; }

// nb <= 48 bits of v at bit position pos of the chunk (LSB first, as deflate packs). Lanes OR into shared words: order-independent.
__device__ __forceinline__ void put_bits(unsigned* out, unsigned pos, unsigned long long v, int /*nb*/) {
  const unsigned w = pos >> 5, sh = pos & 31u;
  if (w + 2 >= (unsigned)(kSlot / 4)) return;                 // never taken: the mode choice bounds the stream by the segment's size
  const unsigned a = (unsigned)(v << sh);
  const unsigned long long r = v >> (32u - sh);
  if (a) atomicOr(&out[w], a);
  if ((unsigned)r) atomicOr(&out[w + 1], (unsigned)r);
  if ((unsigned)(r >> 32)) atomicOr(&out[w + 2], (unsigned)(r >> 32));
}

// One greedy LZ77 parse of the segment, 64 positions at a time. Each lane looks for the longest match of its position among: the
// latest earlier position with the same three-byte hash (inserted by earlier rounds), and the fixed distances 1, bpp and one row,
// which the hash heads cannot give inside a round. The wave then walks the round's matches (a ballot and one shuffle per match
// taken) and the next round starts where the last token ended. EMIT = false counts symbols, EMIT = true writes the codes; both see
// the same head table history, so they take the same tokens. Every loop is bounded: rounds by n, the walk by 64, a comparison by 258.
template <bool EMIT> __device__ void png_parse(SegLds& L, int n, int bpp, int rowlen, int lane, unsigned& bitpos) {
  const unsigned char* d = (const unsigned char*)L.data;
  for (int k = lane; k < (1 << kHashBits); k += 64) L.head[k] = 0;
  __syncthreads();
  int pos0 = 0;
  while (pos0 < n) {
    const int i = pos0 + lane;
    const bool can = i + 2 < n;
    unsigned h = 0, cand = 0;
    if (can) {
      h = (((unsigned)d[i] | ((unsigned)d[i + 1] << 8) | ((unsigned)d[i + 2] << 16)) * 0x9E3779B1u) >> (32 - kHashBits);
      cand = L.head[h];
    }
    __syncthreads();
    if (can) atomicMax(&L.head[h], (unsigned)i + 1u);
    int bl = 0, bd = 0;
    if (can) {
      const int maxlen = min(kMaxMatch, n - i);
      const int cd[4] = {1, bpp, cand ? i - (int)(cand - 1u) : 0, rowlen};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int dist = cd[q];
        if (dist <= 0 || dist > i || bl == maxlen) continue;
        const unsigned char* a = d + i - dist;
        int k = 0;
        while (k < maxlen && a[k] == d[i + k]) ++k;
        if (k > bl || (k == bl && dist < bd)) { bl = k; bd = dist; }
      }
      if (bl < kMinMatch || (bl == kMinMatch && bd > kTooFar)) bl = 0;
    }
    const unsigned long long M = __ballot(bl > 0);
    const int nv = min(64, n - pos0);
    unsigned long long taken = 0;
    int p = 0;
    for (int it = 0; it < 64 && p < nv; ++it) {
      const unsigned long long rest = M >> p;
      if (!rest) { taken |= ~low_mask(p); p = nv; break; }
      const int q = p + __ffsll((long long)rest) - 1;        // the next match: literals up to it, then the match
      taken |= low_mask(q + 1) & ~low_mask(p);
      p = q + __shfl(bl, q);
    }
    taken &= low_mask(nv);
    const bool tk = (taken >> lane) & 1ull, mt = tk && bl > 0;
    if (!EMIT) {
      if (mt) {
        int eb, ev;
        atomicAdd(&L.freq[len_sym(bl, &eb, &ev)], 1u);
        atomicAdd(&L.freq[kDistBase + dist_sym(bd, &eb, &ev)], 1u);
      } else if (tk) {
        atomicAdd(&L.freq[d[i]], 1u);
      }
    } else {
      unsigned long long v = 0;
      int nb = 0;
      if (mt) {
        int eb, ev;
        const unsigned c = L.code[len_sym(bl, &eb, &ev)];
        v = c >> 4; nb = (int)(c & 15u);
        v |= (unsigned long long)ev << nb; nb += eb;
        const unsigned c2 = L.code[kDistBase + dist_sym(bd, &eb, &ev)];
        v |= (unsigned long long)(c2 >> 4) << nb; nb += (int)(c2 & 15u);
        v |= (unsigned long long)ev << nb; nb += eb;
      } else if (tk) {
        const unsigned c = L.code[d[i]];
        v = c >> 4; nb = (int)(c & 15u);
      }
      int inc = nb;
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
      }
      if (nb) put_bits(L.out, bitpos + (unsigned)(inc - nb), v, nb);
      bitpos += (unsigned)__shfl(inc, 63);
    }
    pos0 += p;
  }
  __syncthreads();
}

// lengths -> canonical codes (RFC 1951 §3.2.2) for symbols [base, base + nsym); one lane. cnt / next live in L.tmp[0..31].
__device__ void canonical_codes(SegLds& L, int base, int nsym) {
  unsigned* cnt = L.tmp;
  unsigned* next = L.tmp + 16;
  for (int b = 0; b < 16; ++b) cnt[b] = 0;
  for (int s = 0; s < nsym; ++s) cnt[L.code[base + s] & 15u]++;
  cnt[0] = 0;
  unsigned c = 0;
  for (int b = 1; b < 16; ++b) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < nsym; ++s) {
    const unsigned len = L.code[base + s] & 15u;
    if (len) L.code[base + s] = ((__brev(next[len]++) >> (32 - len)) << 4) | len;
  }
}

// Lengths from the counts: the Shannon length (the smallest l with count * 2^l >= total, so the Kraft sum is at most 1), then codes
// are shortened in symbol order while the sum allows until the code is complete, which inflate requires. Each pass shortens every
// symbol of the largest length while slack is left, so 15 passes always suffice for two or more symbols. One lane.
__device__ bool complete_lengths(SegLds& L, int base, int nsym) {
  unsigned used = 0;
  for (int s = 0; s < nsym; ++s) { const unsigned l = L.code[base + s]; if (l) used += 1u << (15 - l); }
  if (used > 32768u) return false;
  unsigned slack = 32768u - used;
  for (int pass = 0; pass < 15 && slack; ++pass)
    for (int s = 0; s < nsym; ++s) {
      const unsigned l = L.code[base + s];
      if (l > 1) { const unsigned u = 1u << (15 - l); if (u <= slack) { L.code[base + s] = l - 1; slack -= u; } }
    }
  return slack == 0;
}

__global__ void __launch_bounds__(64) png_deflate_kernel(const PngImg* __restrict__ imgs, const int* __restrict__ seg_img, const unsigned char* __restrict__ filt,
                                                         int level, int bpp, unsigned char* __restrict__ slots, unsigned* __restrict__ slot_len,
                                                         unsigned* __restrict__ seg_adler) {
  __shared__ SegLds L;
  const int seg = blockIdx.x, lane = threadIdx.x;
  const PngImg im = imgs[seg_img[seg]];
  const int ls = seg - im.first_seg;
  const long long off = (long long)ls * kSeg;
  const long long left = im.filt_len - off;
  const int n = left < (long long)kSeg ? (int)left : kSeg;
  const bool first = ls == 0, last = ls == im.n_seg - 1;
  const unsigned char* src = filt + im.filt_off + off;           // 16-byte aligned
  unsigned char* d = (unsigned char*)L.data;
  unsigned char* o = (unsigned char*)L.out;
  for (int k = lane * 16; k < n; k += 64 * 16) {
    if (k + 16 <= n) *(uint4*)(d + k) = *(const uint4*)(src + k);
    else for (int q = k; q < n; ++q) d[q] = src[q];
  }
  for (int k = lane; k < kSlot / 4; k += 64) L.out[k] = 0;
  for (int k = lane; k < 320; k += 64) { L.freq[k] = 0; L.code[k] = 0; }
  __syncthreads();

  {  // Adler-32 sums of the segment: A = sum of bytes, B = sum of (n - k) * byte k, both mod 65521; png_gather_kernel combines segments
    constexpr int per = kSeg / 64;
    const int lo = lane * per, hi = min(n, lo + per), len = max(hi - lo, 0);
    unsigned a = 0, b = 0;                                        // per <= 512 bytes: b <= 512 * 513 / 2 * 255 < 2^32
    for (int k = 0; k < len; ++k) { a += d[lo + k]; b += (unsigned)(len - k) * d[lo + k]; }
    L.tmp[lane * 3] = a % kAdlerMod; L.tmp[lane * 3 + 1] = b % kAdlerMod; L.tmp[lane * 3 + 2] = (unsigned)len;
    __syncthreads();
    if (lane == 0) {
      unsigned long long A = 0, B = 0;
      for (int l = 0; l < 64; ++l) {                              // appending part l: every earlier byte gains len_l in weight
        const unsigned long long al = L.tmp[l * 3], bl = L.tmp[l * 3 + 1], nl = L.tmp[l * 3 + 2];
        B = (B + nl * A + bl) % kAdlerMod;
        A = (A + al) % kAdlerMod;
      }
      seg_adler[seg * 2] = (unsigned)A; seg_adler[seg * 2 + 1] = (unsigned)B;
    }
    __syncthreads();
  }

  const int pre = 8 + (first ? 2 : 0);
  if (lane == 0) {
    o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
    if (first) { o[8] = 0x78; o[9] = 0x01; }
  }
  __syncthreads();

  int mode = 0;                                                   // 0 stored, 1 fixed Huffman, 2 dynamic Huffman
  unsigned bitpos = (unsigned)pre * 8u;
  const int rowlen = 1 + im.w * bpp;
  if (level > 0) {
    png_parse<false>(L, n, bpp, rowlen, lane, bitpos);
    if (lane == 0) L.freq[256] = 1;                               // end of block
    __syncthreads();
    unsigned tl = 0, td = 0;
    for (int s = lane; s < 288; s += 64) tl += L.freq[s];
    for (int o2 = 32; o2 > 0; o2 >>= 1) tl += __shfl_xor(tl, o2);
    if (lane < 30) td = max(L.freq[kDistBase + lane], lane < 2 ? 1u : 0u);   // two distance codes always exist: a complete code
    for (int o2 = 32; o2 > 0; o2 >>= 1) td += __shfl_xor(td, o2);
    for (int s = lane; s < 286; s += 64) {
      const unsigned f = L.freq[s];
      unsigned l = 0;
      if (f) { l = 1; while (l < 15 && ((unsigned long long)f << l) < tl) ++l; }
      L.code[s] = l;
    }
    if (lane < 30) {
      const unsigned f = max(L.freq[kDistBase + lane], lane < 2 ? 1u : 0u);
      unsigned l = 0;
      if (f) { l = 1; while (l < 15 && ((unsigned long long)f << l) < td) ++l; }
      L.code[kDistBase + lane] = l;
    }
    __syncthreads();
    if (lane == 0) {
      const bool ok = complete_lengths(L, 0, 286) && complete_lengths(L, kDistBase, 30);
      L.tmp[32] = ok ? 1u : 0u;
    }
    __syncthreads();
    const bool dyn_ok = L.tmp[32] != 0;
    unsigned long long cd = 0, cf = 0;                            // bits of the symbols under the dynamic and the fixed code
    int hl = 0, hd = 0;                                           // last used symbol + 1
    for (int s = lane; s < 286; s += 64) {
      const unsigned f = L.freq[s], l = L.code[s];
      cd += (unsigned long long)f * (l + len_sym_extra(s)); cf += (unsigned long long)f * (fixed_len(s) + len_sym_extra(s));
      if (l) hl = s + 1;
    }
    if (lane < 30) {
      const unsigned f = L.freq[kDistBase + lane], l = L.code[kDistBase + lane];
      cd += (unsigned long long)f * (l + dist_sym_extra(lane)); cf += (unsigned long long)f * (5 + dist_sym_extra(lane));
      if (l) hd = lane + 1;
    }
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
      cd += __shfl_xor(cd, o2); cf += __shfl_xor(cf, o2);
      hl = max(hl, __shfl_xor(hl, o2)); hd = max(hd, __shfl_xor(hd, o2));
    }
    hl = max(hl, 257);
    cd += 3 + 14 + 19 * 3 + 4ull * (unsigned)(hl + hd);
    cf += 3;
    const bool dyn = dyn_ok && cd < cf;
    const unsigned long long bits = (dyn ? cd : cf) + (last ? 0 : 3);
    const unsigned long long bytes = (bits + 7) / 8 + (last ? 0 : 4);
    if (bytes < (unsigned long long)n) mode = dyn ? 2 : 1;        // a segment that does not shrink is stored

    if (mode == 1) {
      for (int s = lane; s < 288; s += 64) L.code[s] = (unsigned)fixed_len(s);
      if (lane < 32) L.code[kDistBase + lane] = 5;
    }
    __syncthreads();
    if (mode != 0) {
      if (lane == 0) {
        canonical_codes(L, 0, 288);
        canonical_codes(L, kDistBase, 32);
        put_bits(L.out, bitpos, (last ? 1u : 0u) | (mode == 2 ? 4u : 2u), 3);
      }
      bitpos += 3;
      __syncthreads();
      if (mode == 2) {
        // HLIT, HDIST, HCLEN = 19; the code-length code gives lengths 0..15 four bits each and does not use 16, 17, 18, so a
        // code length is sent as its four bits (most significant first, as Huffman codes are)
        if (lane == 0) {
          put_bits(L.out, bitpos, (unsigned)(hl - 257) | ((unsigned)(hd - 1) << 5) | (15u << 10), 14);
          unsigned long long cl = 0;                              // order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: three zeros, sixteen fours
          for (int k = 3; k < 19; ++k) cl |= 4ull << (3 * k);
          put_bits(L.out, bitpos + 14, cl & 0xFFFFFFFFull, 32);
          put_bits(L.out, bitpos + 14 + 32, cl >> 32, 25);
        }
        bitpos += 14 + 57;
        for (int s = lane; s < hl + hd; s += 64) {
          const unsigned l = (s < hl ? L.code[s] : L.code[kDistBase + s - hl]) & 15u;
          put_bits(L.out, bitpos + 4u * (unsigned)s, __brev(l) >> 28, 4);
        }
        bitpos += 4u * (unsigned)(hl + hd);
        __syncthreads();
      }
      png_parse<true>(L, n, bpp, rowlen, lane, bitpos);
      const unsigned eob = L.code[256];
      if (lane == 0) put_bits(L.out, bitpos, eob >> 4, (int)(eob & 15u));
      bitpos += eob & 15u;
      if (!last) bitpos += 3;                                     // an empty stored block, not final: three zero bits, then to the byte
      bitpos = (bitpos + 7u) & ~7u;
      if (!last) {
        if (lane == 0) put_bits(L.out, bitpos, 0xFFFF0000ull, 32);  // LEN = 0, NLEN = 0xFFFF
        bitpos += 32;
      }
    }
  }
  __syncthreads();
  int end = (int)(bitpos >> 3);
  if (mode == 0) {
    if (lane == 0) {
      o[pre] = last ? 1 : 0;
      o[pre + 1] = (unsigned char)n; o[pre + 2] = (unsigned char)(n >> 8);
      o[pre + 3] = (unsigned char)~n; o[pre + 4] = (unsigned char)(~n >> 8);
    }
    for (int k = lane; k < n; k += 64) o[pre + 5 + k] = d[k];
    end = pre + 5 + n;
  }
  __syncthreads();
  {  // CRC-32 over the chunk type and payload, bytes [4, end)
    const int len = end - 4, per = (len + 63) / 64;
    const int lo = min(4 + lane * per, end), hi = min(lo + per, end);
    unsigned c = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (int k = lo; k < hi; ++k) c = crc_byte(c, o[k]);
    c = crc_mul(crc_xpow8((unsigned)(end - hi)), c);
    for (int o2 = 32; o2 > 0; o2 >>= 1) c ^= __shfl_xor(c, o2);
    if (lane == 0) { put_be32(o, (unsigned)(end - 8)); put_be32(o + end, ~c); }
  }
  __syncthreads();
  const int total = end + 4;                                      // <= kSlot - 13
  unsigned* slot = (unsigned*)(slots + (size_t)seg * kSlot);
  for (int k = lane; k < (total + 3) / 4; k += 64) slot[k] = L.out[k];
  if (lane == 0) slot_len[seg] = (unsigned)total;
}

// ---- compaction -------------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of the chunk sizes (64-bit), one workgroup: off[0..n], off[n] = the sum
__global__ void __launch_bounds__(1024) png_scan_kernel(const unsigned* __restrict__ len, int n, unsigned long long* __restrict__ off) {
  __shared__ unsigned long long part[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  unsigned long long s = 0;
  for (int k = lo; k < hi; ++k) s += len[k];
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
}

// blocks [0, n_seg): chunk `seg` from its slot to its place in its file. blocks [n_seg, n_seg + n_img): signature, IHDR, the Adler-32
// of the image (per-segment sums combined by the workgroup) in an IDAT of its own, IEND; file_off[i] = where file i starts.
__global__ void __launch_bounds__(256) png_gather_kernel(const PngImg* __restrict__ imgs, int n_img, const int* __restrict__ seg_img, int n_seg,
                                                         const unsigned char* __restrict__ slots, const unsigned* __restrict__ slot_len,
                                                         const unsigned long long* __restrict__ seg_off, const unsigned* __restrict__ seg_adler,
                                                         int channels, int bit_depth, unsigned char* __restrict__ out, long long* __restrict__ file_off) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n_seg) {
    const int seg = blockIdx.x, j = seg_img[seg];
    unsigned char* dst = out + seg_off[seg] + (unsigned long long)j * kFileFixed + 33;
    const unsigned char* src = slots + (size_t)seg * kSlot;
    const int len = (int)slot_len[seg];
    for (int k = tid; k < len; k += 256) dst[k] = src[k];
    return;
  }
  __shared__ unsigned tri[256][3];
  const int j = blockIdx.x - n_seg;
  const PngImg im = imgs[j];
  // sums (A, B, length) of a run of segments. B weighs a byte by its distance from the END of the data, so appending a run r to a
  // prefix p gives every byte of p len_r more: B = B_p + len_r * A_p + B_r
  const int per = (im.n_seg + 255) / 256, lo = min(tid * per, im.n_seg), hi = min(lo + per, im.n_seg);
  unsigned long long A = 0, B = 0, N = 0;
  for (int s = lo; s < hi; ++s) {
    const long long left = im.filt_len - (long long)s * kSeg;
    const unsigned long long ns = left < (long long)kSeg ? (unsigned long long)left : (unsigned long long)kSeg;
    const unsigned long long as = seg_adler[(size_t)(im.first_seg + s) * 2], bs = seg_adler[(size_t)(im.first_seg + s) * 2 + 1];
    B = (B + (ns % kAdlerMod) * A + bs) % kAdlerMod;
    A = (A + as) % kAdlerMod;
    N = (N + ns) % kAdlerMod;
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
  const unsigned adler_a = (unsigned)((1 + A) % kAdlerMod), adler_b = (unsigned)((N + B) % kAdlerMod);   // the initial a = 1 is in every b step
  const unsigned long long base = seg_off[im.first_seg] + (unsigned long long)j * kFileFixed;
  file_off[j] = (long long)base;
  if (j == n_img - 1) file_off[n_img] = (long long)(seg_off[n_seg] + (unsigned long long)n_img * kFileFixed);
  unsigned char* f = out + base;
  const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  for (int k = 0; k < 8; ++k) f[k] = sig[k];
  put_be32(f + 8, 13);
  f[12] = 'I'; f[13] = 'H'; f[14] = 'D'; f[15] = 'R';
  put_be32(f + 16, (unsigned)im.w); put_be32(f + 20, (unsigned)im.h);
  f[24] = (unsigned char)bit_depth; f[25] = (unsigned char)(channels == 1 ? 0 : channels == 3 ? 2 : 6); f[26] = 0; f[27] = 0; f[28] = 0;
  put_be32(f + 29, crc_serial(f + 12, 17));
  unsigned char* t = out + seg_off[im.first_seg + im.n_seg] + (unsigned long long)j * kFileFixed + 33;
  put_be32(t, 4);
  t[4] = 'I'; t[5] = 'D'; t[6] = 'A'; t[7] = 'T';
  put_be32(t + 8, (adler_b << 16) | adler_a);
  put_be32(t + 12, crc_serial(t + 4, 8));
  put_be32(t + 16, 0);
  t[20] = 'I'; t[21] = 'E'; t[22] = 'N'; t[23] = 'D';
  put_be32(t + 24, crc_serial(t + 20, 4));
}

// What one encode in flight holds, borrowed from a pool (ws_pool.hpp), so that encodes on different threads run side by side
struct Workspace {
  DevBuf filt, slots, out, slot_len, seg_adler, seg_off, imgs, seg_img, file_off;
  int device = 0;
  size_t held() const { return filt.n + slots.n + out.n; }     // the three that grow with the image; the rest is a few bytes per segment
};
// at most 8 idle ones; a 16K frame's gigabyte is not kept (never destroyed: nothing is freed at exit, when the runtime may be gone)
WsPool<Workspace>& g_pool = *new WsPool<Workspace>(WsPolicy{8, 0, 768u << 20}, delete_on_owner_device<Workspace>);

void ensure(DevBuf& b, size_t bytes) {
  if (b.n < bytes) b = DevBuf(bytes + bytes / 4);
}

template <int CH, int BPS> void launch_filter(const PngImg& im, int bgr, unsigned char* filt, hipStream_t st) {
  hipLaunchKernelGGL((png_filter_kernel<CH, BPS>), dim3((unsigned)im.h), dim3(256), 0, st, im, bgr, filt);
}

long long n_segments(long long filt_len) { return (filt_len + kSeg - 1) / kSeg; }

}  // namespace

long long png_bound(int h, int w, int channels, int bit_depth) {
  FFP_CHECK(h > 0 && w > 0 && (channels == 1 || channels == 3 || channels == 4) && (bit_depth == 8 || bit_depth == 16), FFP_ERR_ARG,
            "png: %dx%d with %d channels of %d bits is not a gray, RGB or RGBA image of depth 8 or 16", w, h, channels, bit_depth);
  const long long filt = (long long)h * (1 + (long long)w * channels * (bit_depth / 8));
  return kFileFixed + 2 + filt + n_segments(filt) * (12 + 5);
}

long long png_encode_batch_device(const PngSrc* src, int n_img, int channels, int bit_depth, int bgr, int level, long long* offsets, unsigned char* out,
                                  long long cap, hipStream_t st) {
  offsets[0] = 0;
  if (n_img == 0) return 0;
  FFP_CHECK((channels == 1 || channels == 3 || channels == 4) && (bit_depth == 8 || bit_depth == 16), FFP_ERR_ARG,
            "png: %d channels of %d bits (gray, RGB or RGBA at depth 8 or 16 are written)", channels, bit_depth);
  const int bps = bit_depth / 8, bpp = channels * bps;
  std::vector<PngImg> imgs((size_t)n_img);
  long long filt_total = 0, seg_total = 0;
  for (int i = 0; i < n_img; ++i) {
    const PngSrc& q = src[i];
    FFP_CHECK(q.d_img && q.h > 0 && q.w > 0 && (long long)q.w * bpp < (1ll << 30) && q.stride >= (long long)q.w * bpp, FFP_ERR_ARG,
              "png: bad geometry of image %d (%dx%d, row pitch %lld)", i, q.w, q.h, q.stride);
    const long long fl = (long long)q.h * (1 + (long long)q.w * bpp);
    imgs[i] = PngImg{q.d_img, q.stride, filt_total, fl, q.h, q.w, (int)seg_total, (int)n_segments(fl)};
    filt_total += (fl + 15) / 16 * 16;
    seg_total += n_segments(fl);
    FFP_CHECK(seg_total < (1ll << 30), FFP_ERR_ARG, "png: batch too large (%lld segments)", seg_total);
  }
  const int n_seg = (int)seg_total;
  std::vector<int> seg_img((size_t)n_seg);
  for (int i = 0; i < n_img; ++i) std::fill(seg_img.begin() + imgs[i].first_seg, seg_img.begin() + imgs[i].first_seg + imgs[i].n_seg, i);
  long long out_bound = 0;
  for (int i = 0; i < n_img; ++i) out_bound += png_bound(src[i].h, src[i].w, channels, bit_depth);

  auto lease = lease_ws(g_pool, st);
  Workspace& ws = *lease;
  ensure(ws.filt, (size_t)filt_total + 16);
  ensure(ws.slots, (size_t)n_seg * kSlot);
  ensure(ws.out, (size_t)out_bound + 16);
  ensure(ws.slot_len, (size_t)n_seg * sizeof(unsigned));
  ensure(ws.seg_adler, (size_t)n_seg * 2 * sizeof(unsigned));
  ensure(ws.seg_off, ((size_t)n_seg + 1) * sizeof(unsigned long long));
  ensure(ws.imgs, (size_t)n_img * sizeof(PngImg));
  ensure(ws.seg_img, (size_t)n_seg * sizeof(int));
  ensure(ws.file_off, ((size_t)n_img + 1) * sizeof(long long));
  FFP_HIP(hipMemcpyAsync(ws.imgs.p, imgs.data(), sizeof(PngImg) * (size_t)n_img, hipMemcpyHostToDevice, st));
  FFP_HIP(hipMemcpyAsync(ws.seg_img.p, seg_img.data(), sizeof(int) * (size_t)n_seg, hipMemcpyHostToDevice, st));
  for (int i = 0; i < n_img; ++i) {
    unsigned char* f = ws.filt.as<unsigned char>();
    switch (channels * 10 + bps) {
      case 11: launch_filter<1, 1>(imgs[i], bgr, f, st); break;
      case 12: launch_filter<1, 2>(imgs[i], bgr, f, st); break;
      case 31: launch_filter<3, 1>(imgs[i], bgr, f, st); break;
      case 32: launch_filter<3, 2>(imgs[i], bgr, f, st); break;
      case 41: launch_filter<4, 1>(imgs[i], bgr, f, st); break;
      default: launch_filter<4, 2>(imgs[i], bgr, f, st); break;
    }
  }
  hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)n_seg), dim3(64), 0, st, ws.imgs.as<PngImg>(), ws.seg_img.as<int>(), ws.filt.as<unsigned char>(), level, bpp,
                     ws.slots.as<unsigned char>(), ws.slot_len.as<unsigned>(), ws.seg_adler.as<unsigned>());
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(1024), 0, st, ws.slot_len.as<unsigned>(), n_seg, ws.seg_off.as<unsigned long long>());
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)(n_seg + n_img)), dim3(256), 0, st, ws.imgs.as<PngImg>(), n_img, ws.seg_img.as<int>(), n_seg,
                     ws.slots.as<unsigned char>(), ws.slot_len.as<unsigned>(), ws.seg_off.as<unsigned long long>(), ws.seg_adler.as<unsigned>(), channels, bit_depth,
                     ws.out.as<unsigned char>(), ws.file_off.as<long long>());
  FFP_HIP(hipMemcpyAsync(offsets, ws.file_off.p, sizeof(long long) * ((size_t)n_img + 1), hipMemcpyDeviceToHost, st));
  FFP_HIP(hipStreamSynchronize(st));                   // (imgs and seg_img live on this stack frame)
  FFP_HIP(hipGetLastError());
  const long long total = offsets[n_img];
  FFP_CHECK(total > 0 && total <= out_bound, FFP_ERR_STATE, "png: the encoder reported %lld bytes (bound %lld)", total, out_bound);
  if (out && cap >= total) FFP_HIP(hipMemcpy(out, ws.out.p, (size_t)total, hipMemcpyDeviceToHost));
  return total;
}

}  // namespace ffp
