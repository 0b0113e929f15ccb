// overlay.hpp — ordered compositing of detection overlays into a device-resident frame (overlay.hip): the drawing between the detector and
// the file writers, so that a frame decoded by ffp_jpeg_decode_dev / ffp_png_decode_dev is drawn on and encoded without leaving the device.
#pragma once
#include "common.hpp"

namespace ffp {

constexpr int kOverlayMaxPrims = 1 << 20;      // FFP_OVERLAY_MAX_PRIMS
constexpr int kOverlayTileW = 84;              // pixels: 252 bytes, at most 64 aligned 4-byte words at any base alignment — one wavefront per row
constexpr int kOverlayTileH = 16;

// Every argument of ffp_overlay_draw_dev but the device image pointer is judged here, before anything is allocated, uploaded or launched:
// throws Error(FFP_ERR_ARG) naming the primitive. Host code only.
void overlay_check(int h, int w, long long row_stride, const ffp_overlay_prim* prims, int n, const unsigned char* masks, long long mask_bytes);

// Paints prims[0..n) in list order into the h x w x 3 image at d_img (row pitch in bytes, any base alignment). The arguments have passed
// overlay_check. The list and the mask pool go up through a pooled workspace; synchronises `st`. n == 0: nothing is launched.
void overlay_draw_device(unsigned char* d_img, int h, int w, long long row_stride, const ffp_overlay_prim* prims, int n, const unsigned char* masks,
                         long long mask_bytes, hipStream_t st);

}  // namespace ffp
