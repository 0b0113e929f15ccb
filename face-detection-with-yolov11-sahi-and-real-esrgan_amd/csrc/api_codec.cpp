// api_codec.cpp — the C-ABI of libffp.so, part three of four (see api.cpp): JPEG and PNG at the file boundaries, and the overlay drawing between a decode and an
// encode. They take a device number, not a handle.
#include "api_util.hpp"
#include "exif.hpp"
#include "jpeg.hpp"
#include "orient.hpp"
#include "overlay.hpp"
#include "png.hpp"
#include "png_dec.hpp"

using namespace ffp;

extern "C" {

// ---- JPEG at the file boundaries -----------------------------------------------------------------------------
// Every entry runs on a stream of its own of the I/O kind (api_util.hpp, ScopedStream::Io).
int ffp_jpeg_encode_dev(int device, const uint8_t* d_img, int h, int w, int64_t row_stride, int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(out_size, FFP_ERR_ARG, "jpeg_encode: out_size is null");
  ScopedStream cx(device, "jpeg_encode", ScopedStream::Io);
  const long long n = jpeg_encode_device(d_img, h, w, row_stride, bgr, quality, out, cap, cx.st);
  *out_size = n < 0 ? -n : n;
  FFP_CHECK(n >= 0, FFP_ERR_ARG, "jpeg_encode: output buffer too small (%lld bytes needed)", -n);
  FFP_API_END
}

int ffp_jpeg_encode_batch_dev(int device, const uint8_t* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                              int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && out_offsets && (n == 0 || (d_base && offsets && hs && ws)), FFP_ERR_ARG, "jpeg_encode_batch: bad arguments");
  ScopedStream cx(device, "jpeg_encode_batch", ScopedStream::Io);
  std::vector<JpegSrc> src((size_t)n);
  for (int i = 0; i < n; ++i) src[i] = JpegSrc{d_base + offsets[i], hs[i], ws[i], strides ? strides[i] : (long long)ws[i] * 3};
  std::vector<std::vector<unsigned char>> files;
  jpeg_encode_batch_device(src.data(), n, bgr, quality, files, cx.st);
  int64_t pos = 0;
  for (int i = 0; i < n; ++i) { out_offsets[i] = pos; pos += (int64_t)files[i].size(); }
  out_offsets[n] = pos;
  FFP_CHECK(out && cap >= pos, FFP_ERR_ARG, "jpeg_encode_batch: output buffer too small (%lld bytes needed)", (long long)pos);
  for (int i = 0; i < n; ++i) std::memcpy(out + out_offsets[i], files[i].data(), files[i].size());
  FFP_API_END
}

int ffp_jpeg_encode(int device, const uint8_t* img, int h, int w, int bgr, int quality, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(img && h > 0 && w > 0 && out_size, FFP_ERR_ARG, "jpeg_encode: bad arguments");
  ScopedStream cx(device, "jpeg_encode", ScopedStream::Io);
  DevBuf d((size_t)h * w * 3);
  FFP_HIP(hipMemcpy(d.p, img, (size_t)h * w * 3, hipMemcpyHostToDevice));
  const long long n = jpeg_encode_device(d.as<unsigned char>(), h, w, (long long)w * 3, bgr, quality, out, cap, cx.st);
  *out_size = n < 0 ? -n : n;
  FFP_CHECK(n >= 0, FFP_ERR_ARG, "jpeg_encode: output buffer too small (%lld bytes needed)", -n);
  FFP_API_END
}

int ffp_jpeg_info(const uint8_t* data, int64_t n, int32_t* out_h, int32_t* out_w, int32_t* out_ncomp) {
  FFP_API_BEGIN
  FFP_CHECK(data && out_h && out_w, FFP_ERR_ARG, "jpeg_info: null argument");
  JpegScan s;
  jpeg_entropy_decode(data, n, s, true);
  *out_h = s.h; *out_w = s.w;
  if (out_ncomp) *out_ncomp = s.ncomp;
  FFP_API_END
}

int ffp_jpeg_decode_dev(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* d_out, int64_t row_stride, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && d_out, FFP_ERR_ARG, "jpeg_decode: null argument");
  ScopedStream cx(device, "jpeg_decode", ScopedStream::Io);
  jpeg_decode_to_device(data, n, d_out, row_stride, cap, bgr, cx.st);
  FFP_API_END
}

int ffp_jpeg_decode(int device, const uint8_t* data, int64_t n, int bgr, uint8_t* out, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && out, FFP_ERR_ARG, "jpeg_decode: null argument");
  ScopedStream cx(device, "jpeg_decode", ScopedStream::Io);
  JpegScan s;
  jpeg_entropy_decode(data, n, s, true);
  const size_t bytes = (size_t)s.h * s.w * 3;
  FFP_CHECK(cap >= (int64_t)bytes, FFP_ERR_ARG, "jpeg_decode: output buffer too small for %dx%d", s.w, s.h);
  DevBuf d(bytes);
  jpeg_decode_to_device(data, n, d.as<unsigned char>(), 0, (long long)bytes, bgr, cx.st);
  FFP_HIP(hipMemcpy(out, d.p, bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_jpeg_decode_stats(int64_t* device_decodes, int64_t* host_fallbacks, int64_t* extra_sync_rounds) {
  FFP_API_BEGIN
  long long a = 0, b = 0, c = 0;
  jpeg_huff_stats(&a, &b, &c);
  if (device_decodes) *device_decodes = a;
  if (host_fallbacks) *host_fallbacks = b;
  if (extra_sync_rounds) *extra_sync_rounds = c;
  FFP_API_END
}

// n files in one pass (jpeg_huff.hip, jpeg_decode_batch_to_device). The call succeeds when its arguments were valid; what became of file i is status[i],
// and ffp_last_error names the first file that failed. What only a batch entry reports is done here, after the routine the single-file entries share:
// the batch counters, and that name.
static void decode_batch(int n, const uint8_t* const* datas, const int64_t* sizes, int bgr, uint8_t* d_base, const long long* offsets, const int64_t* strides,
                         int64_t cap, int32_t* hs, int32_t* ws, int32_t* status, hipStream_t st, const int32_t* orientations = nullptr) {
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the ABI's integer types are the library's");
  std::vector<std::string> why((size_t)n);
  JpegBatchCost cost;
  jpeg_decode_batch_to_device(n, datas, reinterpret_cast<const long long*>(sizes), bgr, d_base, offsets, reinterpret_cast<const long long*>(strides), cap, hs, ws, status,
                              why.data(), &cost, st, orientations);
  jpeg_batch_note(cost);
  for (int i = 0; i < n; ++i)
    if (status[i] < 0) {
      set_last_error("jpeg_decode_batch: file " + std::to_string(i) + ": " + why[(size_t)i]);
      break;
    }
}

int ffp_jpeg_decode_batch_dev(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr, uint8_t* d_base, const int64_t* offsets,
                              const int64_t* strides, int64_t cap, int32_t* hs, int32_t* ws, int32_t* status) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && (n == 0 || (datas && sizes && d_base && offsets && hs && ws && status)), FFP_ERR_ARG, "jpeg_decode_batch: bad arguments");
  if (n > 0) {
    ScopedStream cx(device, "jpeg_decode_batch", ScopedStream::Io);
    decode_batch(n, datas, sizes, bgr, d_base, reinterpret_cast<const long long*>(offsets), strides, cap, hs, ws, status, cx.st);
  }
  FFP_API_END
}

int ffp_jpeg_decode_batch(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr, uint8_t* const* outs, const int64_t* caps, int32_t* hs,
                          int32_t* ws, int32_t* status) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && (n == 0 || (datas && sizes && outs && caps && hs && ws && status)), FFP_ERR_ARG, "jpeg_decode_batch: bad arguments");
  if (n > 0) {
    // the headers first: the images are packed into one device buffer, 256-byte aligned; an unreadable file gets an empty region
    std::vector<long long> off((size_t)n, 0);
    long long total = 0;
    for (int i = 0; i < n; ++i) {
      off[i] = total;
      JpegScan s;
      try {
        FFP_CHECK(datas[i] && sizes[i] > 0, FFP_ERR_ARG, "jpeg_decode_batch: no data");
        jpeg_entropy_decode(datas[i], sizes[i], s, true);
      } catch (const ffp::Error&) {
        continue;                                            // the batch call reports it in status[i]
      }
      const long long bytes = (long long)s.h * s.w * 3;
      FFP_CHECK(outs[i] && caps[i] >= bytes, FFP_ERR_ARG, "jpeg_decode_batch: output buffer %d too small for %dx%d", i, s.w, s.h);
      total += (bytes + 255) / 256 * 256;
    }
    ScopedStream cx(device, "jpeg_decode_batch", ScopedStream::Io);
    DevBuf d((size_t)std::max<long long>(total, 16));
    decode_batch(n, datas, sizes, bgr, d.as<unsigned char>(), off.data(), nullptr, total, hs, ws, status, cx.st);
    for (int i = 0; i < n; ++i)
      if (status[i] >= 0) FFP_HIP(hipMemcpy(outs[i], d.as<unsigned char>() + off[i], (size_t)hs[i] * ws[i] * 3, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

// ---- the same with the EXIF orientation applied on the device (exif.hpp, orient.hip) ------------------------------------------------------
int ffp_exif_orientation(const uint8_t* data, int64_t n, int32_t* orientation) {
  FFP_API_BEGIN
  FFP_CHECK(data && orientation, FFP_ERR_ARG, "exif_orientation: null argument");
  *orientation = exif::orientation(data, n);
  FFP_API_END
}

int ffp_jpeg_decode_oriented_dev(int device, const uint8_t* data, int64_t n, int bgr, int orientation, uint8_t* d_out, int64_t row_stride, int64_t cap, int32_t* out_h,
                                 int32_t* out_w) {
  FFP_API_BEGIN
  FFP_CHECK(data && d_out, FFP_ERR_ARG, "jpeg_decode_oriented: null argument");
  ScopedStream cx(device, "jpeg_decode_oriented", ScopedStream::Io);
  jpeg_decode_to_device(data, n, d_out, row_stride, cap, bgr, cx.st, orientation, out_h, out_w);
  FFP_API_END
}

int ffp_jpeg_decode_oriented(int device, const uint8_t* data, int64_t n, int bgr, int orientation, uint8_t* out, int64_t cap, int32_t* out_h, int32_t* out_w) {
  FFP_API_BEGIN
  FFP_CHECK(data && out, FFP_ERR_ARG, "jpeg_decode_oriented: null argument");
  ScopedStream cx(device, "jpeg_decode_oriented", ScopedStream::Io);
  JpegScan s;
  jpeg_entropy_decode(data, n, s, true);
  const size_t bytes = (size_t)s.h * s.w * 3;              // the same for both shapes
  FFP_CHECK(cap >= (int64_t)bytes, FFP_ERR_ARG, "jpeg_decode_oriented: output buffer too small for %dx%d", s.w, s.h);
  DevBuf d(bytes);
  jpeg_decode_to_device(data, n, d.as<unsigned char>(), 0, (long long)bytes, bgr, cx.st, orientation, out_h, out_w);
  FFP_HIP(hipMemcpy(out, d.p, bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_jpeg_decode_batch_oriented_dev(int device, int n, const uint8_t* const* datas, const int64_t* sizes, int bgr, const int32_t* orientations, uint8_t* d_base,
                                       const int64_t* offsets, const int64_t* strides, int64_t cap, int32_t* hs, int32_t* ws, int32_t* status) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && (n == 0 || (datas && sizes && d_base && offsets && hs && ws && status)), FFP_ERR_ARG, "jpeg_decode_batch_oriented: bad arguments");
  if (n > 0) {
    const std::vector<int32_t> own((size_t)n, 0);            // a null array: every file's own tag
    ScopedStream cx(device, "jpeg_decode_batch_oriented", ScopedStream::Io);
    decode_batch(n, datas, sizes, bgr, d_base, reinterpret_cast<const long long*>(offsets), strides, cap, hs, ws, status, cx.st, orientations ? orientations : own.data());
  }
  FFP_API_END
}

int ffp_jpeg_decode_batch_stats(int64_t* batches, int64_t* launches_last_batch, int64_t* syncs_last_batch) {
  FFP_API_BEGIN
  long long a = 0, b = 0, c = 0;
  jpeg_batch_stats(&a, &b, &c);
  if (batches) *batches = a;
  if (launches_last_batch) *launches_last_batch = b;
  if (syncs_last_batch) *syncs_last_batch = c;
  FFP_API_END
}

// ---- PNG at the file boundaries (png.hip) -----------------------------------------------------------------------------------------
int64_t ffp_png_bound(int h, int w, int channels, int bit_depth) {
  try {
    return png_bound(h, w, channels, bit_depth);
  } catch (const ffp::Error& e) {
    ffp::set_last_error(e.what());
    return -1;
  }
}

int ffp_png_segment_bytes(void) { return kPngSegmentBytes; }

// the three entries below: arguments checked, device chosen, one launch sequence on an I/O stream; out_offsets is filled before the
// capacity is judged. on_host: `base` is host memory (one image, n == 1) and goes up first.
static void png_encode_any(int device, const void* base, bool on_host, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                           int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_CHECK(n >= 0 && out_offsets && (n == 0 || (base && offsets && hs && ws)), FFP_ERR_ARG, "png_encode: bad arguments");
  FFP_CHECK((channels == 1 || channels == 3 || channels == 4) && (bit_depth == 8 || bit_depth == 16), FFP_ERR_ARG,
            "png_encode: %d channels of %d bits (gray, RGB or RGBA at depth 8 or 16 are written)", channels, bit_depth);
  ScopedStream cx(device, "png_encode", ScopedStream::Io);
  DevBuf up;
  if (on_host) {
    up = upload(static_cast<const unsigned char*>(base), (size_t)hs[0] * (size_t)strides[0]);
    base = up.p;
  }
  std::vector<PngSrc> src((size_t)n);
  for (int i = 0; i < n; ++i)
    src[i] = PngSrc{(const unsigned char*)base + offsets[i], hs[i], ws[i], strides ? strides[i] : (long long)ws[i] * channels * (bit_depth / 8)};
  std::vector<long long> off((size_t)n + 1, 0);
  const long long total = png_encode_batch_device(src.data(), n, channels, bit_depth, bgr, level, off.data(), out, cap, cx.st);
  for (int i = 0; i <= n; ++i) out_offsets[i] = off[i];
  FFP_CHECK(out && cap >= total, FFP_ERR_ARG, "png_encode: output buffer too small (%lld bytes needed)", total);
}

// one image: *out_size is the file's size also when the capacity was the trouble
static void png_encode_one(int device, const void* img, bool on_host, int h, int w, int channels, int bit_depth, int64_t row_stride, int bgr, int level, uint8_t* out,
                           int64_t cap, int64_t* out_size) {
  const int64_t zero = 0;
  const int32_t hh = h, ww = w;
  int64_t oo[2] = {0, 0};
  try {
    png_encode_any(device, img, on_host, 1, &zero, &hh, &ww, &row_stride, channels, bit_depth, bgr, level, out, cap, oo);
  } catch (...) {
    *out_size = oo[1];
    throw;
  }
  *out_size = oo[1];
}

int ffp_png_encode_batch_dev(int device, const void* d_base, int n, const int64_t* offsets, const int32_t* hs, const int32_t* ws, const int64_t* strides,
                             int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_offsets) {
  FFP_API_BEGIN
  png_encode_any(device, d_base, false, n, offsets, hs, ws, strides, channels, bit_depth, bgr, level, out, cap, out_offsets);
  FFP_API_END
}

int ffp_png_encode_dev(int device, const void* d_img, int h, int w, int channels, int bit_depth, int64_t row_stride, int bgr, int level, uint8_t* out, int64_t cap,
                       int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(out_size, FFP_ERR_ARG, "png_encode: out_size is null");
  png_encode_one(device, d_img, false, h, w, channels, bit_depth, row_stride, bgr, level, out, cap, out_size);
  FFP_API_END
}

int ffp_png_encode(int device, const void* img, int h, int w, int channels, int bit_depth, int bgr, int level, uint8_t* out, int64_t cap, int64_t* out_size) {
  FFP_API_BEGIN
  FFP_CHECK(img && h > 0 && w > 0 && out_size, FFP_ERR_ARG, "png_encode: bad arguments");
  png_encode_one(device, img, true, h, w, channels, bit_depth, (int64_t)w * channels * (bit_depth / 8), bgr, level, out, cap, out_size);
  FFP_API_END
}

// ---- reading PNG (png_dec.cpp, png_dec.hip) -----------------------------------------------------------------------------------------
int ffp_png_info(const uint8_t* data, int64_t n, int32_t* h, int32_t* w, int32_t* channels, int32_t* bit_depth) {
  FFP_API_BEGIN
  FFP_CHECK(data && h && w, FFP_ERR_ARG, "png_info: null argument");
  PngFile f;
  png_parse(data, n, f, true);
  *h = f.h; *w = f.w;
  if (channels) *channels = f.channels;
  if (bit_depth) *bit_depth = f.bit_depth;
  FFP_API_END
}

int ffp_png_decode_dev(int device, const uint8_t* data, int64_t n, int bgr, int flags, void* d_out, int64_t row_stride, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && d_out, FFP_ERR_ARG, "png_decode: null argument");
  PngFile f;
  png_parse(data, n, f, false);                          // every refusal of the file's layout comes before the device is touched
  ScopedStream cx(device, "png_decode", ScopedStream::Io);
  png_decode_to_device(data, n, f, bgr, flags, d_out, row_stride, cap, cx.st);
  FFP_API_END
}

int ffp_png_decode(int device, const uint8_t* data, int64_t n, int bgr, int flags, void* out, int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(data && out, FFP_ERR_ARG, "png_decode: null argument");
  PngFile f;
  png_parse(data, n, f, false);
  const long long bytes = (long long)f.h * f.row_bytes();
  FFP_CHECK(cap >= bytes, FFP_ERR_ARG, "png_decode: output buffer too small for %d x %d x %d at %d bits (%lld bytes needed)", f.w, f.h, f.channels, f.bit_depth, bytes);
  ScopedStream cx(device, "png_decode", ScopedStream::Io);
  DevBuf d((size_t)bytes);
  png_decode_to_device(data, n, f, bgr, flags, d.p, 0, bytes, cx.st);
  FFP_HIP(hipMemcpy(out, d.p, (size_t)bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_png_decode_stats(int64_t* parallel_decodes, int64_t* serial_decodes) {
  FFP_API_BEGIN
  long long a = 0, b = 0;
  png_decode_stats(&a, &b);
  if (parallel_decodes) *parallel_decodes = a;
  if (serial_decodes) *serial_decodes = b;
  FFP_API_END
}

int ffp_png_unfilter_geometry(int32_t* rows_per_group, int32_t* cols_per_step) {
  FFP_API_BEGIN
  int r = 0, c = 0;
  png_unfilter_geometry(&r, &c);
  if (rows_per_group) *rows_per_group = r;
  if (cols_per_step) *cols_per_step = c;
  FFP_API_END
}

// ---- detection overlays on a frame that stays on the device (overlay.hip) ------------------------------------------------------------
// Every refusal comes from overlay_check, before the device is chosen: a refused call has touched nothing.
int ffp_overlay_draw_dev(int device, uint8_t* d_img, int h, int w, int64_t row_stride, const ffp_overlay_prim* prims, int n, const uint8_t* masks,
                         int64_t mask_bytes) {
  FFP_API_BEGIN
  static_assert(sizeof(ffp_overlay_prim) == FFP_OVERLAY_PRIM_BYTES && FFP_OVERLAY_MAX_PRIMS == kOverlayMaxPrims, "include/ffp.h states the struct's size and the cap");
  FFP_CHECK(d_img, FFP_ERR_ARG, "overlay_draw: the image is null");
  overlay_check(h, w, row_stride, prims, n, masks, mask_bytes);
  if (n > 0) {
    ScopedStream cx(device, "overlay_draw", ScopedStream::Io);
    overlay_draw_device(d_img, h, w, row_stride, prims, n, masks, mask_bytes, cx.st);
  }
  FFP_API_END
}

int ffp_overlay_draw(int device, uint8_t* img, int h, int w, int64_t row_stride, const ffp_overlay_prim* prims, int n, const uint8_t* masks,
                     int64_t mask_bytes) {
  FFP_API_BEGIN
  FFP_CHECK(img, FFP_ERR_ARG, "overlay_draw: the image is null");
  overlay_check(h, w, row_stride, prims, n, masks, mask_bytes);
  if (n > 0) {
    ScopedStream cx(device, "overlay_draw", ScopedStream::Io);
    const size_t row = (size_t)w * 3;
    DevBuf d((size_t)h * row);
    FFP_HIP(hipMemcpy2D(d.p, row, img, (size_t)row_stride, row, (size_t)h, hipMemcpyHostToDevice));
    overlay_draw_device(d.as<unsigned char>(), h, w, (long long)row, prims, n, masks, mask_bytes, cx.st);
    FFP_HIP(hipMemcpy2D(img, (size_t)row_stride, d.p, row, row, (size_t)h, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

// ---- the EXIF orientation of an image that stays on the device (orient.hip) -----------------------------------------------------------
// Every refusal comes from orient_check, before the device is chosen: a refused call has touched nothing.
int ffp_image_orient_dev(int device, const uint8_t* d_src, int h, int w, int px, int64_t src_stride, int orientation, uint8_t* d_dst, int64_t dst_stride, int64_t cap) {
  FFP_API_BEGIN
  const OrientJob j{d_src, d_dst, src_stride, dst_stride, h, w, orientation};
  orient_check(j, px, cap);
  ScopedStream cx(device, "image_orient", ScopedStream::Io);
  orient_batch_device(&j, 1, px, cx.st);
  FFP_API_END
}

int ffp_image_orient_batch_dev(int device, int n, const uint8_t* d_src_base, const int64_t* src_offsets, const int32_t* hs, const int32_t* ws, int px,
                               const int64_t* src_strides, const int32_t* orientations, uint8_t* d_dst_base, const int64_t* dst_offsets, const int64_t* dst_strides,
                               int64_t cap) {
  FFP_API_BEGIN
  FFP_CHECK(n >= 0 && (n == 0 || (d_src_base && src_offsets && hs && ws && src_strides && orientations && d_dst_base && dst_offsets && dst_strides)), FFP_ERR_ARG,
            "image_orient_batch: bad arguments");
  std::vector<OrientJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(src_offsets[i] >= 0 && dst_offsets[i] >= 0 && dst_offsets[i] <= cap, FFP_ERR_ARG, "image_orient_batch: image %d lies outside its buffer", i);
    jobs[i] = OrientJob{d_src_base + src_offsets[i], d_dst_base + dst_offsets[i], src_strides[i], dst_strides[i], hs[i], ws[i], orientations[i]};
    orient_check(jobs[i], px, cap - dst_offsets[i]);
  }
  // destinations that overlap one another would be written by two workgroups in no order, and a destination that overlaps ANY image's source
  // would be written while another workgroup reads it
  auto dst_lo = [&](int i) { return reinterpret_cast<uintptr_t>(jobs[i].dst); };
  auto dst_hi = [&](int i) { return dst_lo(i) + (uintptr_t)((int64_t)(orient_out_h(jobs[i]) - 1) * dst_strides[i] + (int64_t)orient_out_w(jobs[i]) * px); };
  auto src_lo = [&](int i) { return reinterpret_cast<uintptr_t>(jobs[i].src); };
  auto src_hi = [&](int i) { return src_lo(i) + (uintptr_t)((int64_t)(hs[i] - 1) * src_strides[i] + (int64_t)ws[i] * px); };
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) {
      FFP_CHECK(k <= i || dst_hi(i) <= dst_lo(k) || dst_hi(k) <= dst_lo(i), FFP_ERR_ARG, "image_orient_batch: the destinations of images %d and %d overlap", i, k);
      FFP_CHECK(dst_hi(i) <= src_lo(k) || src_hi(k) <= dst_lo(i), FFP_ERR_ARG, "image_orient_batch: the destination of image %d overlaps the source of image %d", i, k);
    }
  if (n > 0) {
    ScopedStream cx(device, "image_orient_batch", ScopedStream::Io);
    orient_batch_device(jobs.data(), n, px, cx.st);
  }
  FFP_API_END
}

int ffp_image_orient(int device, const uint8_t* src, int h, int w, int px, int64_t src_stride, int orientation, uint8_t* dst, int64_t dst_stride, int64_t cap) {
  FFP_API_BEGIN
  const OrientJob host{src, dst, src_stride, dst_stride, h, w, orientation};
  orient_check(host, px, cap);
  ScopedStream cx(device, "image_orient", ScopedStream::Io);
  const size_t srow = (size_t)w * px, drow = (size_t)orient_out_w(host) * px, dh = (size_t)orient_out_h(host);
  DevBuf ds((size_t)h * srow), dd(dh * drow);
  FFP_HIP(hipMemcpy2D(ds.p, srow, src, (size_t)src_stride, srow, (size_t)h, hipMemcpyHostToDevice));
  const OrientJob j{ds.as<unsigned char>(), dd.as<unsigned char>(), (long long)srow, (long long)drow, h, w, orientation};
  orient_batch_device(&j, 1, px, cx.st);
  FFP_HIP(hipMemcpy2D(dst, (size_t)dst_stride, dd.p, drow, drow, dh, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_image_orient_time_dev(int device, const uint8_t* d_src, int h, int w, int px, int orientation, uint8_t* d_dst, int64_t cap, int iters, float* kernel_us,
                              float* copy_us) {
  FFP_API_BEGIN
  FFP_CHECK(iters >= 1 && iters <= 10000 && kernel_us && copy_us, FFP_ERR_ARG, "image_orient_time: %d iterations (1..10000), or a null result", iters);
  const OrientJob j{d_src, d_dst, (int64_t)w * px, (int64_t)(orientation >= 5 && orientation <= 8 ? h : w) * px, h, w, orientation};
  orient_check(j, px, cap);
  ScopedStream cx(device, "image_orient_time", ScopedStream::Io);
  orient_time_device(j, px, iters, kernel_us, copy_us, cx.st);
  FFP_API_END
}

int ffp_image_orient_geometry(int32_t* tile) {
  FFP_API_BEGIN
  if (tile) *tile = kOrientTile;
  FFP_API_END
}

int ffp_image_orient_stats(int64_t* images, int64_t* launches) {
  FFP_API_BEGIN
  long long a = 0, b = 0;
  orient_stats(&a, &b);
  if (images) *images = a;
  if (launches) *launches = b;
  FFP_API_END
}

}  // extern "C"
