// png.hpp — PNG encoding of device-resident images (png.hip): the other half of SURVEY.md §8 row f2 (JPEG: jpeg.hpp).
#pragma once
#include "common.hpp"

namespace ffp {

// bytes of filtered stream one workgroup compresses on its own (one deflate block, one IDAT chunk): ffp_png_segment_bytes()
constexpr int kPngSegmentBytes = 16384;

// worst-case size of the file of an h x w image with `channels` samples of `bit_depth` bits per pixel (every segment stored)
long long png_bound(int h, int w, int channels, int bit_depth);

// One launch sequence for a whole batch of device-resident images (gray, RGB(A) or BGR(A); 8- or 16-bit samples in host byte order;
// row pitch `stride` bytes): file i = out[offsets[i] .. offsets[i + 1]). offsets (n + 1 entries) is always filled; the files are
// copied to `out` (host) only when it holds them all. Returns the total size. Synchronises `st`.
struct PngSrc { const unsigned char* d_img; int h, w; long long stride; };
long long png_encode_batch_device(const PngSrc* src, int n_img, int channels, int bit_depth, int bgr, int level, long long* offsets, unsigned char* out,
                                  long long cap, hipStream_t st);

}  // namespace ffp
