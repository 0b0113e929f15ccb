// png_dec.hpp — PNG decoding (png_dec.cpp: chunks and the host inflate; png_dec.hip: one wave per IDAT span, then the five filters reversed). The
// writing half is png.hpp.
#pragma once
#include <vector>

#include "common.hpp"

namespace ffp {

struct PngSpan { long long off, len; };          // one IDAT payload inside the file
struct PngFile {
  int h = 0, w = 0, channels = 0, bit_depth = 0;
  std::vector<PngSpan> idat;
  bool zlib_header = false;                      // the IDAT data starts with a valid two-byte zlib header, no preset dictionary
  bool adler_alone = false;                      // the last IDAT payload is exactly the four bytes of the Adler-32 and at least one IDAT precedes it
  int bpp() const { return channels * (bit_depth / 8); }
  long long row_bytes() const { return (long long)w * bpp(); }
  long long filtered_len() const { return (long long)h * (1 + row_bytes()); }
};

// Signature, chunk walk (bounds and the CRC-32 of IHDR, every IDAT and IEND checked; ancillary chunks skipped unread), IHDR validated: gray, RGB or RGBA
// at depth 8 or 16, not interlaced. header_only stops behind IHDR. Throws ffp::Error(FFP_ERR_ARG) naming the field or chunk.
void png_parse(const unsigned char* d, long long n, PngFile& out, bool header_only);

unsigned png_adler32(const unsigned char* p, size_t n);

// The serial route's host half: the joined IDAT payloads as one zlib stream through the shared inflate core into `filtered` (filtered_len() bytes), the
// Adler-32 and every row's filter type checked. Throws FFP_ERR_ARG saying what is wrong (ends early, ends late, Adler-32, ...).
void png_inflate_serial(const unsigned char* d, const PngFile& f, unsigned char* filtered);

// What png_inflate_kernel decides, on the host and with the same core (asan_host_check.cpp): true when every span decodes on its own by the span rules
// and the lengths add up; `filtered` (may be null) receives the bytes, *adler their Adler-32 (only when filtered is given).
bool png_spans_self_contained(const unsigned char* d, const PngFile& f, unsigned char* filtered, unsigned* adler);

constexpr int kPngDecSerial = 1;                 // FFP_PNG_DEC_SERIAL
// File in host memory -> h x w x channels samples (uint8, or uint16 in host order; first three channels BGR when bgr) at d_out, row pitch `stride` bytes
// (0: packed), `cap` bytes available. Synchronises `st`. Segmented files are inflated on the device, one wave per IDAT; others on the host.
void png_decode_to_device(const unsigned char* data, long long n, const PngFile& f, int bgr, int flags, void* d_out, long long stride, long long cap, hipStream_t st);
void png_decode_stats(long long* parallel_decodes, long long* serial_decodes);
void png_unfilter_geometry(int* rows_per_group, int* cols_per_step);

}  // namespace ffp
