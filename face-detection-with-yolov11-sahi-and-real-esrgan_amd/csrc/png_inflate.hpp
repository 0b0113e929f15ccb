// png_inflate.hpp — the inflate core of the PNG decoder (RFC 1951), plain C++ compiled on both sides: png_inflate_kernel (png_dec.hip) runs it with
// one lane walking the symbols and the wave building tables and copying; png_dec.cpp runs it serially over the joined IDAT payloads and, for
// asan_host_check.cpp, span by span as the kernel does. No HIP types, no assertion: every function returns a status, every read is bounded by the end
// of the span (and by the part of it that is staged, on the device), every table walk by 15 bits. What is written is the caller's business: the core
// hands out tokens (a literal, a match, the end of a block) and the caller bounds its output.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FFP_HD __host__ __device__
#else
#define FFP_HD
#endif

namespace ffp {
namespace inf {

enum Status : int {
  kOk = 0,
  kEndsEarly = 1,     // the bytes ran out inside a block
  kBadBlockType = 2,  // BTYPE 3
  kBadStoredLen = 3,  // LEN != ~NLEN
  kBadLengths = 4,    // over-subscribed or incomplete code, bad repeat, no end-of-block code, too many symbols
  kBadSymbol = 5,     // length symbol 286 / 287, distance symbol 30 / 31, or a bit pattern no code has
  kBadDistance = 6,   // a match that reaches before the first output byte
  kEndsLate = 7,      // more output than the image holds
  kNotStaged = 8,     // device only: the staged window did not cover a read (never expected; the span then takes the serial route)
  kNotSegment = 9,    // span rules: the span does not end the way a self-contained segment does
};

constexpr int kLitLutBits = 10, kDistLutBits = 8;
constexpr int kLitSyms = 288, kDistSyms = 32, kDistAt = 288, kLens = 320;

// LSB-first bit reader over bytes [pos, end) of a buffer; byte k of the buffer is p[k - base], staged up to wend (host: base 0, wend = end)
struct Bits {
  const unsigned char* p;
  unsigned long long base, wend, pos, end;
  unsigned long long acc;
  int n;
  bool starved;
};
FFP_HD inline void bits_init(Bits& b, const unsigned char* p, unsigned long long base, unsigned long long wend, unsigned long long pos, unsigned long long end) {
  b.p = p; b.base = base; b.wend = wend; b.pos = pos; b.end = end; b.acc = 0; b.n = 0; b.starved = false;
}
FFP_HD inline void bits_fill(Bits& b) {
  while (b.n <= 56 && b.pos < b.end) {
    if (b.pos >= b.wend || b.pos < b.base) { b.starved = true; return; }
    b.acc |= (unsigned long long)b.p[b.pos - b.base] << b.n;
    ++b.pos;
    b.n += 8;
  }
}
FFP_HD inline int bits_take(Bits& b, int k, unsigned* v) {      // k <= 32
  if (b.n < k) bits_fill(b);
  if (b.n < k) return b.starved ? kNotStaged : kEndsEarly;
  *v = (unsigned)(b.acc & ((1ull << k) - 1ull));
  b.acc >>= k;
  b.n -= k;
  return kOk;
}
// the first byte not yet touched: whole bytes still in the accumulator are given back, a byte used in part counts as used
FFP_HD inline unsigned long long bits_byte_pos(const Bits& b) { return b.pos - (unsigned long long)(b.n >> 3); }
FFP_HD inline void bits_to_byte(Bits& b) {                       // drop the rest of the current byte and restart at a byte position
  b.pos = bits_byte_pos(b);
  b.acc = 0;
  b.n = 0;
}

// One canonical Huffman code: symbols sorted by code, codes of each length counted; the short codes also sit in a table indexed by the next
// LB bits of the stream.
template <int NSYM, int LB> struct Huff {
  unsigned short count[16], first[16], offs[16];
  unsigned short symbol[NSYM];
  unsigned short lut[1 << LB];      // sym << 4 | length; 0: a longer code, or none
  int nsym;
};

// Serial part of the construction. sparse_ok: the code may be empty (its use is then an error) or hold one code of length 1, which deflate allows
// for distances; every other incomplete code, and every over-subscribed one, is refused.
template <int NSYM, int LB> FFP_HD inline int huff_build(Huff<NSYM, LB>& h, const unsigned char* len, int n, bool sparse_ok) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) h.count[len[s] & 15]++;
  h.nsym = n;
  int left = 1, used = 0, maxlen = 0;
  for (int l = 1; l < 16; ++l) {
    left <<= 1;
    left -= (int)h.count[l];
    if (left < 0) return kBadLengths;
    if (h.count[l]) maxlen = l;
    used += h.count[l];
  }
  if (left > 0 && !(sparse_ok && (used == 0 || (used == 1 && maxlen == 1)))) return kBadLengths;
  unsigned code = 0, off = 0;
  h.first[0] = 0; h.offs[0] = 0;
  for (int l = 1; l < 16; ++l) {
    code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
    h.first[l] = (unsigned short)code;
    h.offs[l] = (unsigned short)off;
    off += h.count[l];
  }
  unsigned short next[16];
  for (int l = 0; l < 16; ++l) next[l] = h.offs[l];
  for (int s = 0; s < n; ++s) {
    const int l = len[s] & 15;
    if (l) h.symbol[next[l]++] = (unsigned short)s;
  }
  return kOk;
}
template <int NSYM, int LB> FFP_HD inline void huff_lut_clear(Huff<NSYM, LB>& h, int lane, int nlanes) {
  for (int k = lane; k < (1 << LB); k += nlanes) h.lut[k] = 0;
}
// after huff_build and huff_lut_clear (a barrier between them on the device): every symbol fills its own entries
template <int NSYM, int LB> FFP_HD inline void huff_lut_fill(Huff<NSYM, LB>& h, const unsigned char* len, int lane, int nlanes) {
  for (int s = lane; s < h.nsym; s += nlanes) {
    const int l = len[s] & 15;
    if (l == 0 || l > LB) continue;
    // the symbol's rank among the codes of its length = how many smaller symbols share the length; found from the sorted list
    int lo = h.offs[l], hi = lo + h.count[l];        // symbol[lo, hi) ascending
    for (int it = 0; it < 10 && lo + 1 < hi; ++it) {
      const int mid = (lo + hi) >> 1;
      if (h.symbol[mid] <= s) lo = mid; else hi = mid;
    }
    const unsigned code = (unsigned)h.first[l] + (unsigned)(lo - h.offs[l]);
    unsigned rc = 0;
    for (int k = 0; k < l; ++k) rc |= ((code >> k) & 1u) << (l - 1 - k);
    for (unsigned j = rc; j < (1u << LB); j += 1u << l) h.lut[j] = (unsigned short)((s << 4) | l);
  }
}

// one symbol; *sym is set on kOk
template <int NSYM, int LB> FFP_HD inline int huff_decode(Bits& b, const Huff<NSYM, LB>& h, int* sym) {
  if (b.n < 15) bits_fill(b);
  const unsigned e = h.lut[b.acc & ((1u << LB) - 1u)];
  if (e) {
    const int l = (int)(e & 15u);
    if (l > b.n) return b.starved ? kNotStaged : kEndsEarly;
    b.acc >>= l; b.n -= l;
    *sym = (int)(e >> 4);
    return kOk;
  }
  int code = 0;
  for (int l = 1; l < 16; ++l) {
    if (l > b.n) return b.starved ? kNotStaged : kEndsEarly;
    code |= (int)((b.acc >> (l - 1)) & 1ull);
    const int k = code - (int)h.first[l];
    if (k >= 0 && k < (int)h.count[l]) {
      b.acc >>= l; b.n -= l;
      *sym = h.symbol[h.offs[l] + k];
      return kOk;
    }
    code <<= 1;
  }
  return kBadSymbol;
}

typedef Huff<kLitSyms, kLitLutBits> HuffLit;
typedef Huff<kDistSyms, kDistLutBits> HuffDist;
typedef Huff<19, 7> HuffLen;

struct Block {
  int final, type;
  unsigned stored;       // type 0: bytes that follow at bits_byte_pos
};

// The header of the next block. Type 0: the reader stands at the first stored byte (byte aligned, nothing buffered). Types 1 and 2: lens[0, 288) are the
// literal/length code lengths and lens[288, 320) the distance code lengths, ready for huff_build. Needs at most 600 bytes of the stream.
FFP_HD inline int block_begin(Bits& b, Block& blk, unsigned char* lens, HuffLen& hl) {
  unsigned v = 0;
  int st = bits_take(b, 3, &v);
  if (st) return st;
  blk.final = (int)(v & 1u);
  blk.type = (int)(v >> 1);
  blk.stored = 0;
  if (blk.type == 3) return kBadBlockType;
  if (blk.type == 0) {
    b.acc >>= (b.n & 7); b.n -= (b.n & 7);
    st = bits_take(b, 32, &v);
    if (st) return st;
    if ((v & 0xFFFFu) != ((~v >> 16) & 0xFFFFu)) return kBadStoredLen;
    blk.stored = v & 0xFFFFu;
    bits_to_byte(b);
    return kOk;
  }
  if (blk.type == 1) {
    for (int s = 0; s < kLitSyms; ++s) lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < kDistSyms; ++s) lens[kDistAt + s] = 5;
    return kOk;
  }
  st = bits_take(b, 14, &v);
  if (st) return st;
  const int hlit = (int)(v & 31u) + 257, hdist = (int)((v >> 5) & 31u) + 1, hclen = (int)(v >> 10) + 4;
  if (hlit > 286 || hdist > 30) return kBadLengths;
  unsigned char cl[19];
  for (int k = 0; k < 19; ++k) cl[k] = 0;
  for (int k = 0; k < hclen; ++k) {
    st = bits_take(b, 3, &v);
    if (st) return st;
    const int order = k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 8 - (k - 3) / 2 : 8 + (k - 4) / 2;     // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    cl[order] = (unsigned char)v;
  }
  st = huff_build(hl, cl, 19, false);
  if (st) return st;
  huff_lut_clear(hl, 0, 1);
  huff_lut_fill(hl, cl, 0, 1);
  const int total = hlit + hdist;
  int k = 0;
  while (k < total) {                                    // every round adds at least one length: at most 316 rounds
    int sym = 0;
    st = huff_decode(b, hl, &sym);
    if (st) return st;
    if (sym < 16) { lens[k++] = (unsigned char)sym; continue; }
    int rep = 0;
    unsigned char what = 0;
    if (sym == 16) {
      if (k == 0) return kBadLengths;
      what = lens[k - 1];
      st = bits_take(b, 2, &v); rep = 3 + (int)v;
    } else if (sym == 17) {
      st = bits_take(b, 3, &v); rep = 3 + (int)v;
    } else {
      st = bits_take(b, 7, &v); rep = 11 + (int)v;
    }
    if (st) return st;
    if (k + rep > total) return kBadLengths;
    for (int q = 0; q < rep; ++q) lens[k++] = what;
  }
  if (lens[256] == 0) return kBadLengths;
  for (int s = hdist - 1; s >= 0; --s) lens[kDistAt + s] = lens[hlit + s];      // kDistAt >= hlit: moving upward, last first
  for (int s = hdist; s < kDistSyms; ++s) lens[kDistAt + s] = 0;
  for (int s = hlit; s < kLitSyms; ++s) lens[s] = 0;
  return kOk;
}

struct Token {
  int kind;        // 0 literal, 1 match, 2 end of block
  int val;         // the literal, or the match length (3..258)
  int dist;        // 1..32768
};

// the next token of a Huffman block; needs at most 6 bytes of the stream
FFP_HD inline int next_token(Bits& b, const HuffLit& hl, const HuffDist& hd, Token& t) {
  int s = 0;
  int st = huff_decode(b, hl, &s);
  if (st) return st;
  if (s < 256) { t.kind = 0; t.val = s; t.dist = 0; return kOk; }
  if (s == 256) { t.kind = 2; t.val = 0; t.dist = 0; return kOk; }
  if (s > 285) return kBadSymbol;
  unsigned v = 0;
  int len;
  if (s < 265) len = s - 254;
  else if (s == 285) len = 258;
  else {
    const int e = (s - 261) >> 2;
    st = bits_take(b, e, &v);
    if (st) return st;
    len = 3 + ((4 + ((s - 261) & 3)) << e) + (int)v;
  }
  int d = 0;
  st = huff_decode(b, hd, &d);
  if (st) return st;
  if (d > 29) return kBadSymbol;
  int dist;
  if (d < 4) dist = d + 1;
  else {
    const int e = (d >> 1) - 1;
    st = bits_take(b, e, &v);
    if (st) return st;
    dist = 1 + ((2 + (d & 1)) << e) + (int)v;
  }
  t.kind = 1; t.val = len; t.dist = dist;
  return kOk;
}

// How a run of blocks over bytes [pos, end) has to end. Stream: with its final block, wherever that stops. The spans of a segmented file: every span
// but the last with a stored block that is not final and takes the span's last byte (the empty one of a sync flush, or a segment that is itself stored:
// either leaves a serial decoder on a byte boundary, waiting for a block header); the last with its final block inside its last byte.
enum Ending : int { kStream = 0, kSpanInner = 1, kSpanLast = 2 };

// The host's inflate: the same block and token steps in a plain loop. out may be null (lengths and validity only). *produced and *used (bytes of input
// consumed) are set on every return.
inline int inflate_host(const unsigned char* src, unsigned long long pos, unsigned long long end, Ending how, unsigned char* out, unsigned long long cap,
                        unsigned long long* produced, unsigned long long* used) {
  Bits b;
  bits_init(b, src, 0, end, pos, end);
  static thread_local HuffLit hl;
  static thread_local HuffDist hd;
  static thread_local HuffLen hc;
  unsigned char lens[kLens];
  unsigned long long n = 0;
  int st = kOk;
  *produced = 0; *used = 0;
  for (;;) {
    Block blk;
    st = block_begin(b, blk, lens, hc);
    if (st) break;
    if (blk.type == 0) {
      const unsigned long long at = bits_byte_pos(b);
      if (at + blk.stored > end) { st = kEndsEarly; break; }
      if (n + blk.stored > cap) { st = kEndsLate; break; }
      if (out) for (unsigned k = 0; k < blk.stored; ++k) out[n + k] = src[at + k];
      n += blk.stored;
      b.pos = at + blk.stored;
      if (how != kStream && !blk.final && b.pos == end) {
        st = how == kSpanInner ? kOk : kNotSegment;
        break;
      }
    } else {
      st = huff_build(hl, lens, kLitSyms, false);
      if (!st) st = huff_build(hd, lens + kDistAt, kDistSyms, true);
      if (st) break;
      huff_lut_clear(hl, 0, 1); huff_lut_fill(hl, lens, 0, 1);
      huff_lut_clear(hd, 0, 1); huff_lut_fill(hd, lens + kDistAt, 0, 1);
      for (;;) {                                       // every token but the last adds output: bounded by cap - n + 1
        Token t;
        st = next_token(b, hl, hd, t);
        if (st || t.kind == 2) break;
        if (t.kind == 0) {
          if (n + 1 > cap) { st = kEndsLate; break; }
          if (out) out[n] = (unsigned char)t.val;
          ++n;
        } else {
          if ((unsigned long long)t.dist > n) { st = kBadDistance; break; }
          if (n + (unsigned long long)t.val > cap) { st = kEndsLate; break; }
          if (out) for (int k = 0; k < t.val; ++k) out[n + k] = out[n + k - t.dist];
          n += (unsigned long long)t.val;
        }
      }
      if (st) break;
    }
    if (blk.final) {
      if (how == kSpanInner) st = kNotSegment;
      else if (how == kSpanLast && bits_byte_pos(b) != end) st = kNotSegment;
      break;
    }
    if (how != kStream && bits_byte_pos(b) >= end && b.n == 0) { st = kNotSegment; break; }      // the span ended on another block boundary
  }
  *produced = n;
  *used = bits_byte_pos(b) - pos;
  return st;
}

FFP_HD inline const char* status_text(int st) {
  switch (st) {
    case kOk: return "ok";
    case kEndsEarly: return "the deflate stream ends early";
    case kBadBlockType: return "deflate block type 3";
    case kBadStoredLen: return "stored block with LEN != ~NLEN";
    case kBadLengths: return "bad Huffman code lengths (over-subscribed, incomplete or malformed)";
    case kBadSymbol: return "invalid Huffman symbol";
    case kBadDistance: return "match distance reaches before the first byte";
    case kEndsLate: return "the deflate stream ends late: it holds more bytes than the image";
    case kNotStaged: return "staging window missed";
    default: return "not a self-contained segment";
  }
}

}  // namespace inf
}  // namespace ffp
