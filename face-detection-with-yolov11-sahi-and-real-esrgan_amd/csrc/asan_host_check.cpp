// asan_host_check.cpp — host-side robustness driver for the parsers of untrusted bytes (host ASan/UBSan build).
// Built by `build.py --asan` with the host compiler only (-fsanitize=address,undefined; no device code, no GPU needed) from
// common.cpp + weights.cpp + jpeg_dec.cpp + this file. It feeds jpeg_entropy_decode and WeightFile::parse
//   * every file given on the command line, unchanged (must parse),
//   * truncations of it at every length in the header region and at a stride through the body,
//   * seeded byte / bit mutations, with extra weight on the marker segments (DHT, DQT, SOF, SOS, DRI),
//   * hand-made malformed streams (over-subscribed DHT, all-ones codes, fill bytes at the end, zero-length segments, RGB-coded files),
// and expects each call to either succeed or throw ffp::Error — any out-of-bounds access, overflow or undefined shift aborts the
// process through the sanitizer runtime. ONNX models (onnx_graph.cpp) are parsed and lowered (SCRFD subset) under the same cases:
// every truncation of the first 4 KiB and at a stride through the body, and seeded byte / bit mutations.
// PNG files (png_dec.cpp; the inflate core of png_inflate.hpp, the code png_inflate_kernel compiles): each file is parsed, inflated serially and span by
// span under the kernel's rules (length, Adler-32 and the verdict "segmented" / "serial" are printed), then truncated at every length of the first 4 KiB
// and at a stride through the body, and hit by seeded byte / bit mutations, raw and inside chunk payloads with the CRCs made right again. `pngbad` files
// must be refused; the reason is printed.
// Usage: asan_host_check jpeg <file>... ffpw <file>... onnx <file>... png <file>... pngbad <file>...
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "jpeg.hpp"
#include "onnx_graph.hpp"
#include "png_dec.hpp"
#include "weights.hpp"

using namespace ffp;
typedef std::vector<unsigned char> Bytes;

static long long g_ok = 0, g_rejected = 0;

static Bytes slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the same two passes jpeg_decode_to_device makes: header -> planes sized from it -> full entropy decode
static bool try_jpeg(const Bytes& b) {
  // exact-size heap copy: one byte past the stream is a redzone
  std::unique_ptr<unsigned char[]> d(new unsigned char[b.size() ? b.size() : 1]);
  if (!b.empty()) memcpy(d.get(), b.data(), b.size());
  try {
    JpegScan s;
    jpeg_entropy_decode(d.get(), (long long)b.size(), s, true);
    std::vector<short> planes[3];
    for (int c = 0; c < s.ncomp; ++c) {
      planes[c].resize((size_t)s.comp[c].blocks_x * s.comp[c].blocks_y * 64);
      s.coef[c] = planes[c].data();
    }
    jpeg_entropy_decode(d.get(), (long long)b.size(), s, false);
    ++g_ok;
    return true;
  } catch (const Error&) {
    ++g_rejected;
    return false;
  }
}

static bool try_ffpw(const Bytes& b) {
  std::unique_ptr<unsigned char[]> d(new unsigned char[b.size() ? b.size() : 1]);
  if (!b.empty()) memcpy(d.get(), b.data(), b.size());
  try {
    WeightFile wf;
    wf.parse(d.get(), b.size());
    double acc = 0;                                       // touch the first and last element of every tensor the parser accepted
    for (auto& kv : wf.t)
      if (kv.second.numel()) acc += kv.second.data[0] + kv.second.data[kv.second.numel() - 1];
    (void)acc;
    ++g_ok;
    return true;
  } catch (const Error&) {
    ++g_rejected;
    return false;
  }
}

static void put_segment(Bytes& o, int marker, const Bytes& payload) {
  o.push_back(0xFF); o.push_back((unsigned char)marker);
  const int L = (int)payload.size() + 2;
  o.push_back((unsigned char)(L >> 8)); o.push_back((unsigned char)(L & 255));
  o.insert(o.end(), payload.begin(), payload.end());
}

// end of the header region = offset just past the first SOS segment
static size_t header_end(const Bytes& b) {
  size_t i = 2;
  while (i + 4 <= b.size() && b[i] == 0xFF) {
    const int m = b[i + 1], L = (b[i + 2] << 8) | b[i + 3];
    i += 2 + L;
    if (m == 0xDA) break;
  }
  return i < b.size() ? i : b.size();
}

static void jpeg_cases(const Bytes& good, unsigned seed) {
  if (!try_jpeg(good)) { fprintf(stderr, "a valid file was rejected\n"); exit(3); }
  const size_t he = header_end(good);
  for (size_t n = 0; n <= he && n <= good.size(); ++n) try_jpeg(Bytes(good.begin(), good.begin() + n));
  for (size_t n = he; n < good.size(); n += 1 + (good.size() - he) / 97) try_jpeg(Bytes(good.begin(), good.begin() + n));
  std::mt19937 rng(seed);
  for (int it = 0; it < 3000; ++it) {
    Bytes m = good;
    const int k = 1 + (int)(rng() % 4);
    for (int q = 0; q < k; ++q) {
      const size_t pos = (rng() % 3) ? rng() % he : rng() % m.size();      // two thirds of the hits land in the header
      switch (rng() % 4) {
        case 0: m[pos] = (unsigned char)rng(); break;
        case 1: m[pos] ^= (unsigned char)(1u << (rng() % 8)); break;
        case 2: m[pos] = 0xFF; break;
        default: m[pos] = 0; break;
      }
    }
    try_jpeg(m);
  }
  // hand-made streams: the valid file's segments with one DHT replaced
  auto with_dht = [&](const Bytes& dht_payload) {
    Bytes o = {0xFF, 0xD8};
    put_segment(o, 0xC4, dht_payload);
    o.insert(o.end(), good.begin() + 2, good.end());       // the file's own tables follow and may override: also put ours last
    Bytes o2(good.begin(), good.begin() + he);
    // insert in front of SOS: find the SOS marker start
    size_t i = 2, sos = 2;
    while (i + 4 <= good.size() && good[i] == 0xFF) { const int mk = good[i + 1], L = (good[i + 2] << 8) | good[i + 3]; if (mk == 0xDA) { sos = i; break; } i += 2 + L; }
    Bytes o3(good.begin(), good.begin() + sos);
    put_segment(o3, 0xC4, dht_payload);
    o3.insert(o3.end(), good.begin() + sos, good.end());
    try_jpeg(o);
    try_jpeg(o3);
  };
  for (int tc = 0; tc < 2; ++tc) {
    Bytes p(17 + 200, 0);                                  // 200 codes of length 1
    p[0] = (unsigned char)(tc << 4); p[1] = 200;
    for (int i = 0; i < 200; ++i) p[17 + i] = (unsigned char)i;
    with_dht(p);
    Bytes q(17 + 3, 0);                                    // three codes of length 1
    q[0] = (unsigned char)(tc << 4); q[1] = 3; q[17] = 1; q[18] = 2; q[19] = 3;
    with_dht(q);
    Bytes r(17 + 2, 0);                                    // two codes of length 1: complete, but uses the all-ones code
    r[0] = (unsigned char)(tc << 4); r[1] = 2; r[17] = 0; r[18] = 1;
    with_dht(r);
    Bytes s(17 + 256, 0);                                  // 256 codes of length 8 (all-ones used), then nothing
    s[0] = (unsigned char)(tc << 4); s[8] = 255; s[9] = 1;
    for (int i = 0; i < 256; ++i) s[17 + i] = (unsigned char)i;
    with_dht(s);
    Bytes t(17 + 255, 0);                                  // over-subscribed only at length 16
    t[0] = (unsigned char)(tc << 4); t[1] = 1; t[16] = 254;
    for (int i = 0; i < 255; ++i) t[17 + i] = (unsigned char)i;
    with_dht(t);
    Bytes u(17 + 12, 0);                                   // every symbol is category 15: shifts in receive_extend
    u[0] = (unsigned char)(tc << 4); u[4] = 12;
    for (int i = 0; i < 12; ++i) u[17 + i] = 0xFF;
    with_dht(u);
  }
  {
    Bytes o(good.begin(), good.begin() + 2);                // fill bytes running into the end of the stream
    for (int i = 0; i < 9; ++i) o.push_back(0xFF);
    try_jpeg(o);
    o.push_back(0xDB);
    try_jpeg(o);
    o.push_back(0x00);
    try_jpeg(o);
    Bytes z = {0xFF, 0xD8, 0xFF, 0xDB, 0x00, 0x00};          // segment length below 2
    try_jpeg(z);
    Bytes a = {0xFF, 0xD8};
    Bytes ad = {'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0, 0, 0};   // APP14, transform 0: RGB-coded
    put_segment(a, 0xEE, ad);
    a.insert(a.end(), good.begin() + 2, good.end());
    const bool three = [&] { try { JpegScan s; jpeg_entropy_decode(good.data(), (long long)good.size(), s, true); return s.ncomp == 3; } catch (const Error&) { return false; } }();
    if (try_jpeg(a) && three) { fprintf(stderr, "an Adobe transform-0 file was accepted as YCbCr\n"); exit(3); }
  }
}

static void ffpw_cases(const Bytes& good, unsigned seed) {
  if (!try_ffpw(good)) { fprintf(stderr, "a valid container was rejected\n"); exit(3); }
  const size_t he = good.size() < 4096 ? good.size() : 4096;
  for (size_t n = 0; n <= he; ++n) try_ffpw(Bytes(good.begin(), good.begin() + n));
  std::mt19937 rng(seed);
  for (int it = 0; it < 4000; ++it) {
    Bytes m = good;
    const int k = 1 + (int)(rng() % 3);
    for (int q = 0; q < k; ++q) {
      const size_t pos = rng() % he;
      switch (rng() % 3) {
        case 0: m[pos] = (unsigned char)rng(); break;
        case 1: m[pos] = 0xFF; break;
        default: m[pos] ^= (unsigned char)(1u << (rng() % 8)); break;
      }
    }
    if (rng() % 4 == 0) m.resize(rng() % m.size());
    try_ffpw(m);
  }
}

static bool try_onnx(const Bytes& b) {
  std::unique_ptr<unsigned char[]> d(new unsigned char[b.size() ? b.size() : 1]);     // exact-size copy: a redzone right behind it
  if (!b.empty()) memcpy(d.get(), b.data(), b.size());
  try {
    const onnx::Graph g = onnx::parse(d.get(), b.size());
    (void)onnx::lower(g, 2, 64, 64).describe();
    ++g_ok;
    return true;
  } catch (const Error&) {
    ++g_rejected;
    return false;
  }
}

static void onnx_cases(const Bytes& good, unsigned seed) {
  if (!try_onnx(good)) { fprintf(stderr, "a valid model was rejected\n"); exit(3); }
  const size_t he = good.size() < 4096 ? good.size() : 4096;
  for (size_t n = 0; n <= he; ++n) try_onnx(Bytes(good.begin(), good.begin() + n));
  for (size_t n = he; n < good.size(); n += 1 + good.size() / 512) try_onnx(Bytes(good.begin(), good.begin() + n));
  std::mt19937 rng(seed);
  for (int it = 0; it < 3000; ++it) {
    Bytes m = good;
    const int k = 1 + (int)(rng() % 4);
    for (int q = 0; q < k; ++q) {
      const size_t pos = rng() % m.size();
      switch (rng() % 4) {
        case 0: m[pos] = (unsigned char)rng(); break;
        case 1: m[pos] = 0xFF; break;
        case 2: m[pos] = 0x80; break;
        default: m[pos] ^= (unsigned char)(1u << (rng() % 8)); break;
      }
    }
    if (rng() % 4 == 0) m.resize(rng() % m.size());
    try_onnx(m);
  }
}

// ---- png: the chunk walk (png_dec.cpp) and the inflate core the kernel compiles too (png_inflate.hpp) -------------------------------------------
static unsigned png_crc(const unsigned char* p, size_t n) {
  unsigned c = 0xFFFFFFFFu;
  for (size_t k = 0; k < n; ++k) {
    c ^= p[k];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}
struct PngChunk { Bytes type, payload; };
static std::vector<PngChunk> png_chunks(const Bytes& b) {          // of a file the parser accepted
  std::vector<PngChunk> out;
  size_t pos = 8;
  while (pos + 12 <= b.size()) {
    const size_t len = ((size_t)b[pos] << 24) | ((size_t)b[pos + 1] << 16) | ((size_t)b[pos + 2] << 8) | b[pos + 3];
    if (len > b.size() - pos - 12) break;
    out.push_back(PngChunk{Bytes(b.begin() + pos + 4, b.begin() + pos + 8), Bytes(b.begin() + pos + 8, b.begin() + pos + 8 + len)});
    pos += 12 + len;
  }
  return out;
}
static Bytes png_join(const Bytes& sig, const std::vector<PngChunk>& ch) {   // lengths and CRCs made right again
  Bytes o(sig.begin(), sig.begin() + 8);
  for (const PngChunk& c : ch) {
    const unsigned len = (unsigned)c.payload.size();
    for (int s = 24; s >= 0; s -= 8) o.push_back((unsigned char)(len >> s));
    Bytes body(c.type);
    body.insert(body.end(), c.payload.begin(), c.payload.end());
    o.insert(o.end(), body.begin(), body.end());
    const unsigned crc = png_crc(body.data(), body.size());
    for (int s = 24; s >= 0; s -= 8) o.push_back((unsigned char)(crc >> s));
  }
  return o;
}

// Both routes over one file: the spans one by one under the kernel's rules, and the joined stream. 1 accepted, 0 rejected (why: the serial route's
// message). The routes must agree wherever the span route accepts: exit 3 otherwise.
static int try_png(const Bytes& b, const char* print_as, std::string* why = nullptr) {
  std::unique_ptr<unsigned char[]> d(new unsigned char[b.size() ? b.size() : 1]);      // exact-size copy: a redzone right behind it
  if (!b.empty()) memcpy(d.get(), b.data(), b.size());
  try {
    PngFile f;
    png_parse(d.get(), (long long)b.size(), f, false);
    if (f.filtered_len() > (64ll << 20)) { ++g_rejected; if (why) *why = "too large for the driver"; return 0; }      // a mutated IHDR must not exhaust the host
    const size_t want = (size_t)f.filtered_len();
    std::unique_ptr<unsigned char[]> a(new unsigned char[want]), s(new unsigned char[want]);
    unsigned adler = 0;
    const unsigned char* tail = d.get() + f.idat.back().off;
    bool seg = png_spans_self_contained(d.get(), f, a.get(), &adler);
    if (seg) {
      const unsigned stored = ((unsigned)tail[0] << 24) | ((unsigned)tail[1] << 16) | ((unsigned)tail[2] << 8) | tail[3];
      seg = stored == adler;
    }
    png_inflate_serial(d.get(), f, s.get());
    if (seg && memcmp(a.get(), s.get(), want) != 0) { fprintf(stderr, "png: the span route and the serial route disagree\n"); exit(3); }
    if (print_as) printf("png %s: length %zu adler %08x verdict %s\n", print_as, want, png_adler32(s.get(), want), seg ? "segmented" : "serial");
    ++g_ok;
    return 1;
  } catch (const Error& e) {
    if (why) *why = e.what();
    ++g_rejected;
    return 0;
  }
}

static void png_cases(const Bytes& good, const char* path, unsigned seed) {
  if (!try_png(good, path)) { fprintf(stderr, "a valid file was rejected\n"); exit(3); }
  const size_t he = good.size() < 4096 ? good.size() : 4096;
  for (size_t n = 0; n <= he; ++n) try_png(Bytes(good.begin(), good.begin() + n), nullptr);
  for (size_t n = he; n < good.size(); n += 1 + (good.size() - he) / 97) try_png(Bytes(good.begin(), good.begin() + n), nullptr);
  const std::vector<PngChunk> ch = png_chunks(good);
  std::mt19937 rng(seed);
  for (int it = 0; it < 3000; ++it) {
    if (it % 3 == 0) {                                       // raw hits: mostly the chunk walk and the CRCs answer
      Bytes m = good;
      const int k = 1 + (int)(rng() % 4);
      for (int q = 0; q < k; ++q) {
        const size_t pos = rng() % m.size();
        if (rng() % 2) m[pos] = (unsigned char)rng(); else m[pos] ^= (unsigned char)(1u << (rng() % 8));
      }
      try_png(m, nullptr);
      continue;
    }
    std::vector<PngChunk> c = ch;                            // hits inside payloads with the CRCs made right: the header checks and the inflate core answer
    const int k = 1 + (int)(rng() % 3);
    for (int q = 0; q < k; ++q) {
      PngChunk& t = c[rng() % c.size()];
      if (t.payload.empty()) continue;
      const size_t pos = (rng() % 4 == 0) ? rng() % (t.payload.size() < 16 ? t.payload.size() : 16) : rng() % t.payload.size();   // extra weight on block headers
      switch (rng() % 5) {
        case 0: t.payload[pos] = (unsigned char)rng(); break;
        case 1: t.payload[pos] ^= (unsigned char)(1u << (rng() % 8)); break;
        case 2: t.payload[pos] = 0xFF; break;
        case 3: t.payload[pos] = 0; break;
        default: t.payload.resize(pos); break;               // a chunk cut short
      }
    }
    try_png(png_join(good, c), nullptr);
  }
}

// files that must be refused: prints the reason
static void png_bad_case(const Bytes& bad, const char* path) {
  std::string why;
  if (try_png(bad, nullptr, &why)) { fprintf(stderr, "png %s: an invalid file was accepted\n", path); exit(3); }
  printf("png %s: rejected: %s\n", path, why.c_str());
}

int main(int argc, char** argv) {
  enum { NONE, JPEG, FFPW, ONNX, PNG, PNGBAD } mode = NONE;
  unsigned seed = 1;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "jpeg") { mode = JPEG; continue; }
    if (a == "ffpw") { mode = FFPW; continue; }
    if (a == "onnx") { mode = ONNX; continue; }
    if (a == "png") { mode = PNG; continue; }
    if (a == "pngbad") { mode = PNGBAD; continue; }
    const Bytes b = slurp(argv[i]);
    if (mode == PNG) png_cases(b, argv[i], seed++);
    else if (mode == PNGBAD) png_bad_case(b, argv[i]);
    else if (mode == JPEG) jpeg_cases(b, seed++);
    else if (mode == FFPW) ffpw_cases(b, seed++);
    else if (mode == ONNX) onnx_cases(b, seed++);
    else { fprintf(stderr, "usage: %s jpeg <file>... ffpw <file>... onnx <file>... png <file>... pngbad <file>...\n", argv[0]); return 2; }
  }
  printf("asan_host_check: %lld inputs parsed, %lld rejected, no sanitizer report\n", g_ok, g_rejected);
  return 0;
}
