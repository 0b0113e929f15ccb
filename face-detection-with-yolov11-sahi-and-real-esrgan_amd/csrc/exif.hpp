// exif.hpp — the EXIF orientation of a JPEG or PNG file, found in its bytes (replaces a second Image.open(path).getexif() per read in the shims;
// what cv2.imread and read_image_as_pil(..., exif_fix=True) of the reference apply). No HIP in here and no allocation, so the same code runs under
// the host sanitizers (exif_host_check.cpp).
//
// JPEG: the marker segments up to SOS; the first APP1 whose payload starts with "Exif\0\0" holds a TIFF header ("II" or "MM", 42, the offset
// of IFD0) and IFD0, whose entry 0x0112 is the tag (SHORT or LONG, count 1). PNG: the first eXIf chunk holds the same TIFF header and IFD. The
// chunks are walked by their lengths to IEND, through the IDATs: the format lets eXIf stand on either side of them, and Pillow's getexif(), which
// the shims used until now, finds it on either side (it reads the file to its end when the chunks in front of IDAT had none).
//
// THE RULE: every answer but a well-formed tag of 1..8 is 1 (as stored): no tag, a value outside 1..8, a truncated segment, an IFD offset or an
// entry count that leaves the segment, a file of neither kind. Every read goes through Span::at / u16 / u32, which see the segment's own length:
// nothing outside [data, data + n) is read, whatever the lengths inside the file say.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ffp {
namespace exif {

struct Span {
  const unsigned char* p;
  long long n;
  bool has(long long off, long long len) const { return off >= 0 && len >= 0 && off <= n && len <= n - off; }
  unsigned at(long long off) const { return p[off]; }                                       // callers check has() first
  unsigned u16(long long off, bool le) const { return le ? at(off) | (at(off + 1) << 8) : (at(off) << 8) | at(off + 1); }
  unsigned long u32(long long off, bool le) const {
    return le ? (unsigned long)u16(off, true) | ((unsigned long)u16(off + 2, true) << 16) : ((unsigned long)u16(off, false) << 16) | (unsigned long)u16(off + 2, false);
  }
  Span sub(long long off, long long len) const { return Span{p + off, len}; }               // callers check has() first
};

// the TIFF header and IFD0 of an Exif body (after "Exif\0\0" in a JPEG, the whole chunk body in a PNG)
inline int tiff_orientation(Span t) {
  if (!t.has(0, 8)) return 1;
  bool le;
  if (t.at(0) == 'I' && t.at(1) == 'I') le = true;
  else if (t.at(0) == 'M' && t.at(1) == 'M') le = false;
  else return 1;
  if (t.u16(2, le) != 42) return 1;
  const long long ifd = (long long)t.u32(4, le);
  if (!t.has(ifd, 2)) return 1;
  const long long count = t.u16(ifd, le);
  if (!t.has(ifd + 2, count * 12)) return 1;                 // an entry count that leaves the segment: the directory is not believed at all
  for (long long i = 0; i < count; ++i) {
    const long long e = ifd + 2 + 12 * i;
    if (t.u16(e, le) != 0x0112) continue;
    const unsigned type = t.u16(e + 2, le);
    if (t.u32(e + 4, le) != 1) return 1;
    unsigned long v;
    if (type == 3) v = t.u16(e + 8, le);
    else if (type == 4) v = t.u32(e + 8, le);
    else return 1;
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

inline int jpeg_orientation(Span f) {
  long long i = 2;                                           // behind SOI
  while (f.has(i, 2)) {
    if (f.at(i) != 0xFF) return 1;
    const unsigned m = f.at(i + 1);
    if (m == 0xFF) { ++i; continue; }                        // a fill byte
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) { i += 2; continue; }      // markers that stand alone
    if (m == 0xDA || m == 0xD9 || m == 0x00) return 1;       // the scan starts (or the file ends): no Exif segment came before it
    if (!f.has(i + 2, 2)) return 1;
    const long long L = f.u16(i + 2, false);
    if (L < 2 || !f.has(i + 2, L)) return 1;                 // the segment runs past the file
    if (m == 0xE1 && L >= 8) {
      const Span s = f.sub(i + 4, L - 2);
      if (s.at(0) == 'E' && s.at(1) == 'x' && s.at(2) == 'i' && s.at(3) == 'f' && s.at(4) == 0 && s.at(5) == 0) return tiff_orientation(s.sub(6, s.n - 6));
    }
    i += 2 + L;
  }
  return 1;
}

inline int png_orientation(Span f) {
  long long i = 8;                                           // behind the signature
  while (f.has(i, 8)) {
    const long long L = (long long)f.u32(i, false);
    const bool is_iend = f.at(i + 4) == 'I' && f.at(i + 5) == 'E' && f.at(i + 6) == 'N' && f.at(i + 7) == 'D';
    const bool is_exif = f.at(i + 4) == 'e' && f.at(i + 5) == 'X' && f.at(i + 6) == 'I' && f.at(i + 7) == 'f';
    if (is_iend) return 1;
    if (!f.has(i + 8, L)) return 1;
    if (is_exif) return tiff_orientation(f.sub(i + 8, L));
    if (!f.has(i + 8, L + 4)) return 1;
    i += 12 + L;
  }
  return 1;
}

// 1..8; 1 for everything that is not a well-formed tag (THE RULE above)
inline int orientation(const unsigned char* data, long long n) {
  static const unsigned char kPng[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (!data || n < 4) return 1;
  const Span f{data, n};
  if (f.at(0) == 0xFF && f.at(1) == 0xD8) return jpeg_orientation(f);
  if (n >= 8) {
    bool png = true;
    for (int k = 0; k < 8; ++k) png = png && f.at(k) == kPng[k];
    if (png) return png_orientation(f);
  }
  return 1;
}

}  // namespace exif
}  // namespace ffp
