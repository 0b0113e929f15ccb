// exif_host_check.cpp — csrc/exif.hpp on the CPU under AddressSanitizer + UBSan (build.py --exif-check). Every file is handed to the parser in a heap
// block of exactly its own length, so a read one byte past the end is a sanitizer report. Three parts: the corpus of tests/test_exif_host.py built
// again here with its expected answers; every prefix of every corpus file; seeded single-byte corruptions. A prefix or a corrupted file has no
// expected tag, only the rule that the answer is one of 1..8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "exif.hpp"

namespace {

using Bytes = std::vector<unsigned char>;

void put16(Bytes& b, unsigned v, bool le) {
  if (le) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
  else { b.push_back((v >> 8) & 255); b.push_back(v & 255); }
}
void put32(Bytes& b, unsigned long v, bool le) {
  if (le) { put16(b, v & 0xFFFF, true); put16(b, (v >> 16) & 0xFFFF, true); }
  else { put16(b, (v >> 16) & 0xFFFF, false); put16(b, v & 0xFFFF, false); }
}
void append(Bytes& b, const Bytes& s) { b.insert(b.end(), s.begin(), s.end()); }
void append(Bytes& b, const char* s, size_t n) { b.insert(b.end(), s, s + n); }

// a TIFF header and an IFD0 of `extra` unrelated entries around the orientation entry (type 3 SHORT or 4 LONG); value < 0: no such entry
Bytes tiff(bool le, int type, long value, unsigned long ifd_off = 8, int claimed_count = -1) {
  Bytes t;
  append(t, le ? "II" : "MM", 2);
  put16(t, 42, le);
  put32(t, ifd_off, le);
  const int count = value < 0 ? 1 : 2;
  put16(t, claimed_count >= 0 ? (unsigned)claimed_count : (unsigned)count, le);
  put16(t, 0x0100, le); put16(t, 4, le); put32(t, 1, le); put32(t, 640, le);                   // ImageWidth
  if (value >= 0) {
    put16(t, 0x0112, le); put16(t, (unsigned)type, le); put32(t, 1, le);
    if (type == 3) { put16(t, (unsigned)value, le); put16(t, 0, le); }
    else put32(t, (unsigned long)value, le);
  }
  put32(t, 0, le);                                                                             // no next IFD
  return t;
}

Bytes segment(unsigned marker, const Bytes& payload) {
  Bytes s{0xFF, (unsigned char)marker};
  put16(s, (unsigned)payload.size() + 2, false);
  append(s, payload);
  return s;
}
Bytes exif_app1(const Bytes& t) {
  Bytes p;
  append(p, "Exif\0\0", 6);
  append(p, t);
  return segment(0xE1, p);
}
Bytes jfif_app0() {
  Bytes p;
  append(p, "JFIF\0\1\1\0\0\1\0\1\0\0", 14);
  return segment(0xE0, p);
}
Bytes xmp_app1() {
  Bytes p;
  const char* ns = "http://ns.adobe.com/xap/1.0/";
  append(p, ns, std::strlen(ns) + 1);
  const char* body = "<x:xmpmeta xmlns:x=\"adobe:ns:meta/\"></x:xmpmeta>";
  append(p, body, std::strlen(body));
  return segment(0xE1, p);
}
// what follows the application segments: a quantisation table, a frame header, the start of a scan, a few entropy-coded bytes, EOI
Bytes jpeg_tail() {
  Bytes t = segment(0xDB, Bytes(65, 1));
  append(t, segment(0xC0, Bytes{8, 0, 8, 0, 8, 1, 1, 0x11, 0}));
  append(t, segment(0xDA, Bytes{1, 1, 0, 0, 63, 0}));
  append(t, Bytes{0x12, 0x34, 0xFF, 0x00, 0x56, 0xFF, 0xD9});
  return t;
}
Bytes jpeg(const std::vector<Bytes>& segs) {
  Bytes f{0xFF, 0xD8};
  for (const Bytes& s : segs) append(f, s);
  append(f, jpeg_tail());
  return f;
}
Bytes chunk(const char* type, const Bytes& body) {
  Bytes c;
  put32(c, (unsigned long)body.size(), false);
  append(c, type, 4);
  append(c, body);
  put32(c, 0, false);                                                                          // the parser does not look at the CRC
  return c;
}
Bytes png(const Bytes* exif_before, const Bytes* exif_after) {
  Bytes f{0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  append(f, chunk("IHDR", Bytes{0, 0, 0, 1, 0, 0, 0, 1, 8, 2, 0, 0, 0}));
  if (exif_before) append(f, chunk("eXIf", *exif_before));
  append(f, chunk("IDAT", Bytes{0x78, 0x01, 0x01, 0x04, 0x00, 0xFB, 0xFF, 0x00, 0x01, 0x02, 0x03, 0x00, 0x0D, 0x00, 0x07}));
  if (exif_after) append(f, chunk("eXIf", *exif_after));
  append(f, chunk("IEND", Bytes{}));
  return f;
}

struct Case { std::string name; Bytes file; int want; };

int failures = 0;

// the parser on a heap block of exactly n bytes
int run(const unsigned char* d, size_t n) {
  unsigned char* blk = static_cast<unsigned char*>(std::malloc(n ? n : 1));
  if (n) std::memcpy(blk, d, n);
  const int o = ffp::exif::orientation(blk, (long long)n);
  std::free(blk);
  return o;
}

}  // namespace

int main() {
  std::vector<Case> corpus;
  for (int le = 0; le < 2; ++le)
    for (int type = 3; type <= 4; ++type)
      for (long v = 0; v <= 9; ++v)
        corpus.push_back({"app1 " + std::string(le ? "II" : "MM") + " type " + std::to_string(type) + " value " + std::to_string(v),
                          jpeg({exif_app1(tiff(le, type, v))}), v >= 1 && v <= 8 ? (int)v : 1});
  corpus.push_back({"no tag", jpeg({exif_app1(tiff(true, 3, -1))}), 1});
  corpus.push_back({"no app1", jpeg({jfif_app0()}), 1});
  corpus.push_back({"app1 after app0", jpeg({jfif_app0(), exif_app1(tiff(false, 3, 6))}), 6});
  corpus.push_back({"xmp app1 first", jpeg({jfif_app0(), xmp_app1(), exif_app1(tiff(true, 3, 8))}), 8});
  corpus.push_back({"ifd behind a gap", jpeg({exif_app1([] { Bytes t = tiff(true, 3, 3, 8); Bytes g(t.begin(), t.begin() + 8); g[4] = 12; append(g, Bytes(4, 0)); g.insert(g.end(), t.begin() + 8, t.end()); return g; }())}), 3});
  corpus.push_back({"tag of type BYTE", jpeg({exif_app1(tiff(true, 1, 6))}), 1});
  {
    const Bytes t6 = tiff(true, 3, 6), t3 = tiff(false, 4, 3);
    corpus.push_back({"png eXIf before IDAT", png(&t6, nullptr), 6});
    corpus.push_back({"png eXIf before IDAT, MM LONG", png(&t3, nullptr), 3});
    corpus.push_back({"png eXIf after IDAT", png(nullptr, &t6), 6});
    corpus.push_back({"png no chunk", png(nullptr, nullptr), 1});
  }
  // damaged files
  {
    Bytes f = jpeg({exif_app1(tiff(true, 3, 6))});
    f[4] = 0xFF; f[5] = 0xF0;                                // the segment's length runs past the file
    corpus.push_back({"segment past the file", f, 1});
    corpus.push_back({"ifd offset 0xFFFFFFF0", jpeg({exif_app1(tiff(true, 3, 6, 0xFFFFFFF0ul))}), 1});
    corpus.push_back({"ifd offset 0xFFFFFFF0 MM", jpeg({exif_app1(tiff(false, 3, 6, 0xFFFFFFF0ul))}), 1});
    Bytes t = tiff(true, 3, 6, 8, 0xFFFF);
    t.resize(20);                                            // a 20-byte body that claims 65535 entries
    corpus.push_back({"entry count 0xFFFF in 20 bytes", jpeg({exif_app1(t)}), 1});
    Bytes cut = jpeg({exif_app1(tiff(true, 3, 6))});
    cut.resize(2 + 4 + 6 + 8 + 2 + 12 + 5);                  // SOI, the segment's head, "Exif\0\0", the TIFF header, the count, one entry, five bytes of the tag's
    corpus.push_back({"cut inside the entry", cut, 1});
    corpus.push_back({"not an image", Bytes{'G', 'I', 'F', '8', '9', 'a', 0, 0, 0, 0}, 1});
    corpus.push_back({"empty", Bytes{}, 1});
  }

  for (const Case& c : corpus) {
    const int got = run(c.file.data(), c.file.size());
    if (got != c.want) { std::printf("FAIL %s: got %d, want %d\n", c.name.c_str(), got, c.want); ++failures; }
  }
  long long prefixes = 0;
  for (const Case& c : corpus)
    for (size_t n = 0; n <= c.file.size(); ++n, ++prefixes) {
      const int got = run(c.file.data(), n);
      if (got < 1 || got > 8) { std::printf("FAIL prefix %zu of %s: %d\n", n, c.name.c_str(), got); ++failures; }
    }
  unsigned long long seed = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  const int kCorruptions = 6000;
  for (int k = 0; k < kCorruptions; ++k) {
    const Case& c = corpus[next() % corpus.size()];
    if (c.file.empty()) continue;
    Bytes f = c.file;
    f[next() % f.size()] = (unsigned char)(next() & 255);
    const int got = run(f.data(), f.size());
    if (got < 1 || got > 8) { std::printf("FAIL corruption %d of %s: %d\n", k, c.name.c_str(), got); ++failures; }
  }
  if (ffp::exif::orientation(nullptr, 100) != 1) { std::printf("FAIL null data\n"); ++failures; }
  std::printf("%zu files, %lld prefixes, %d corruptions\n", corpus.size(), prefixes, kCorruptions);
  if (failures) { std::printf("exif_host_check: %d failures\n", failures); return 1; }
  std::printf("exif_host_check: ok\n");
  return 0;
}
