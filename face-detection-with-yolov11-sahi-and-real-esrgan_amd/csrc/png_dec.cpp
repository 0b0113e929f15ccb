// png_dec.cpp — the host half of PNG decoding: the chunk walk over untrusted bytes and the serial inflate of files that are one zlib stream (every
// writer but this library's). The inflate itself is png_inflate.hpp, the code png_inflate_kernel compiles too; what the kernel decides about a file's
// spans is restated here on the host (png_spans_self_contained) so that asan_host_check.cpp can run it under the sanitizers.
#include <cstring>

#include "png_dec.hpp"
#include "png_inflate.hpp"

namespace ffp {

namespace {

const unsigned char kSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

struct CrcTable {
  unsigned t[256];
  CrcTable() {
    for (unsigned i = 0; i < 256; ++i) {
      unsigned c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
      t[i] = c;
    }
  }
};
unsigned crc32(const unsigned char* p, size_t n) {
  static const CrcTable T;
  unsigned c = 0xFFFFFFFFu;
  for (size_t k = 0; k < n; ++k) c = T.t[(c ^ p[k]) & 255u] ^ (c >> 8);
  return ~c;
}
inline unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | (unsigned)p[3]; }

// byte k of the joined IDAT payloads
struct Joined {
  const unsigned char* d;
  const PngFile& f;
  long long total() const { long long t = 0; for (const PngSpan& s : f.idat) t += s.len; return t; }
  void copy(std::vector<unsigned char>& out) const {
    out.resize((size_t)total());
    size_t at = 0;
    for (const PngSpan& s : f.idat) { if (s.len) std::memcpy(out.data() + at, d + s.off, (size_t)s.len); at += (size_t)s.len; }
  }
};

void check_filter_types(const unsigned char* filtered, const PngFile& f) {
  const long long rl = 1 + f.row_bytes();
  for (int r = 0; r < f.h; ++r)
    FFP_CHECK(filtered[(long long)r * rl] <= 4, FFP_ERR_ARG, "png: filter type %d in row %d", (int)filtered[(long long)r * rl], r);
}

}  // namespace

unsigned png_adler32(const unsigned char* p, size_t n) {
  unsigned a = 1, b = 0;
  while (n) {
    const size_t k = n < 5552 ? n : 5552;              // the largest run before b can pass 2^32
    for (size_t q = 0; q < k; ++q) { a += p[q]; b += a; }
    a %= 65521u; b %= 65521u;
    p += k; n -= k;
  }
  return (b << 16) | a;
}

void png_parse(const unsigned char* d, long long n, PngFile& out, bool header_only) {
  FFP_CHECK(d && n >= 8 && std::memcmp(d, kSig, 8) == 0, FFP_ERR_ARG, "png: not a PNG file (signature)");
  out = PngFile();
  long long pos = 8;
  bool first = true, idat_done = false, end_seen = false;
  while (!end_seen) {
    FFP_CHECK(pos + 12 <= n, FFP_ERR_ARG, "png: the file ends inside a chunk header at byte %lld", pos);
    const unsigned len = be32(d + pos);
    const unsigned char* type = d + pos + 4;
    FFP_CHECK(len <= 0x7FFFFFFFu && (long long)len <= n - pos - 12, FFP_ERR_ARG, "png: chunk %.4s at byte %lld runs past the end of the file", (const char*)type, pos);
    const unsigned char* payload = d + pos + 8;
    const bool is_ihdr = std::memcmp(type, "IHDR", 4) == 0, is_idat = std::memcmp(type, "IDAT", 4) == 0, is_iend = std::memcmp(type, "IEND", 4) == 0;
    FFP_CHECK(first == is_ihdr, FFP_ERR_ARG, first ? "png: the first chunk is not IHDR" : "png: a second IHDR chunk");
    if (is_ihdr || is_idat || is_iend)
      FFP_CHECK(crc32(type, (size_t)len + 4) == be32(payload + len), FFP_ERR_ARG, "png: CRC mismatch in the %.4s chunk at byte %lld", (const char*)type, pos);
    if (is_ihdr) {
      FFP_CHECK(len == 13, FFP_ERR_ARG, "png: IHDR of %u bytes", len);
      const unsigned w = be32(payload), h = be32(payload + 4);
      const int depth = payload[8], ctype = payload[9];
      FFP_CHECK(w >= 1 && h >= 1 && w <= 0x7FFFFFFFu && h <= 0x7FFFFFFFu, FFP_ERR_ARG, "png: width %u, height %u", w, h);
      FFP_CHECK(ctype == 0 || ctype == 2 || ctype == 6, FFP_ERR_ARG, "png: colour type %d (%s) is not decoded; gray, RGB and RGBA are", ctype,
                ctype == 3 ? "palette" : ctype == 4 ? "gray with alpha" : "unknown");
      FFP_CHECK(depth == 8 || depth == 16, FFP_ERR_ARG, "png: bit depth %d is not decoded; 8 and 16 are", depth);
      FFP_CHECK(payload[10] == 0 && payload[11] == 0, FFP_ERR_ARG, "png: compression method %d, filter method %d", (int)payload[10], (int)payload[11]);
      FFP_CHECK(payload[12] == 0, FFP_ERR_ARG, "png: interlace method %d: interlaced files are not decoded", (int)payload[12]);
      out.h = (int)h; out.w = (int)w; out.bit_depth = depth; out.channels = ctype == 0 ? 1 : ctype == 2 ? 3 : 4;
      FFP_CHECK(out.row_bytes() < (1ll << 31) && out.filtered_len() < (1ll << 40), FFP_ERR_ARG, "png: %u x %u is too large", w, h);
      if (header_only) return;
    } else if (is_idat) {
      FFP_CHECK(!idat_done, FFP_ERR_ARG, "png: IDAT chunks are not consecutive (byte %lld)", pos);
      out.idat.push_back(PngSpan{pos + 8, (long long)len});
    } else if (is_iend) {
      end_seen = true;
    } else {
      FFP_CHECK((type[0] & 0x20) != 0 || std::memcmp(type, "PLTE", 4) == 0, FFP_ERR_ARG, "png: unknown critical chunk at byte %lld", pos);
      if (!out.idat.empty()) idat_done = true;
    }
    first = false;
    pos += 12 + (long long)len;
  }
  FFP_CHECK(!out.idat.empty(), FFP_ERR_ARG, "png: no IDAT chunk");
  // deflate expands at most 1032 : 1 (a 258-byte match in two bits): an IHDR that asks for more than the IDAT data can hold is refused here, before
  // anybody allocates width x height bytes on the word of a small crafted file
  long long idat_bytes = 0;
  for (const PngSpan& s : out.idat) idat_bytes += s.len;
  FFP_CHECK(out.filtered_len() <= idat_bytes * 1032, FFP_ERR_ARG, "png: the deflate stream ends early: %lld bytes of IDAT data cannot hold the %lld bytes of a %d x %d image",
            idat_bytes, out.filtered_len(), out.w, out.h);
  // the first two bytes of the joined payloads (they may lie in different chunks)
  int got = 0;
  unsigned char zh[2] = {0, 0};
  for (const PngSpan& s : out.idat)
    for (long long k = 0; k < s.len && got < 2; ++k) zh[got++] = d[s.off + k];
  out.zlib_header = got == 2 && (zh[0] & 15) == 8 && (zh[0] >> 4) <= 7 && ((zh[0] << 8) | zh[1]) % 31 == 0 && (zh[1] & 0x20) == 0;
  out.adler_alone = out.idat.size() >= 2 && out.idat.back().len == 4;
}

void png_inflate_serial(const unsigned char* d, const PngFile& f, unsigned char* filtered) {
  FFP_CHECK(f.zlib_header, FFP_ERR_ARG, "png: the IDAT data does not start with a zlib header (deflate, window up to 32 KiB, no preset dictionary)");
  std::vector<unsigned char> joined;
  const unsigned char* z = d + f.idat[0].off;
  long long zn = f.idat[0].len;
  if (f.idat.size() > 1) {
    Joined{d, f}.copy(joined);
    z = joined.data();
    zn = (long long)joined.size();
  }
  FFP_CHECK(zn >= 6, FFP_ERR_ARG, "png: the deflate stream ends early (%lld bytes of IDAT data)", zn);
  const unsigned long long want = (unsigned long long)f.filtered_len();
  unsigned long long produced = 0, used = 0;
  const int st = inf::inflate_host(z, 2, (unsigned long long)zn - 4, inf::kStream, filtered, want, &produced, &used);
  FFP_CHECK(st == inf::kOk, FFP_ERR_ARG, "png: %s (after %llu of %llu bytes)", inf::status_text(st), produced, want);
  FFP_CHECK(produced == want, FFP_ERR_ARG, "png: the deflate stream ends early (%llu of %llu bytes)", produced, want);
  FFP_CHECK(2 + used == (unsigned long long)zn - 4, FFP_ERR_ARG, "png: the deflate stream ends late: %llu bytes follow its final block", (unsigned long long)zn - 4 - 2 - used);
  const unsigned stored = be32(z + zn - 4), have = png_adler32(filtered, (size_t)want);
  FFP_CHECK(stored == have, FFP_ERR_ARG, "png: Adler-32 mismatch (the file says %08x, the data gives %08x)", stored, have);
  check_filter_types(filtered, f);
}

bool png_spans_self_contained(const unsigned char* d, const PngFile& f, unsigned char* filtered, unsigned* adler) {
  if (!f.adler_alone || !f.zlib_header || f.idat[0].len < 2) return false;
  const size_t ns = f.idat.size() - 1;
  const unsigned long long want = (unsigned long long)f.filtered_len();
  unsigned long long at = 0;
  for (size_t s = 0; s < ns; ++s) {
    const unsigned long long lo = (unsigned long long)f.idat[s].off + (s == 0 ? 2 : 0), hi = (unsigned long long)(f.idat[s].off + f.idat[s].len);
    unsigned long long produced = 0, used = 0;
    const int st = inf::inflate_host(d, lo, hi, s + 1 == ns ? inf::kSpanLast : inf::kSpanInner, filtered ? filtered + at : nullptr, want - at, &produced, &used);
    if (st != inf::kOk || used != hi - lo) return false;
    at += produced;
  }
  if (at != want) return false;
  if (filtered && adler) *adler = png_adler32(filtered, (size_t)want);
  return true;
}

}  // namespace ffp
