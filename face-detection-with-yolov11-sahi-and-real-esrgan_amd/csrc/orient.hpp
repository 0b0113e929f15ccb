// orient.hpp — the EXIF orientation applied to device-resident images (orient.hip): what cv2.imread and read_image_as_pil(..., exif_fix=True) do to
// a frame on the host, done where a decoded frame already is, so that a turned file keeps the device routes of the readers, the overlays and the crops.
#pragma once
#include "common.hpp"

namespace ffp {

constexpr int kOrientTile = 64;                // pixels: one workgroup moves a 64 x 64 pixel tile through LDS

// One image: h x w pixels (the SOURCE's size) of px bytes at src (row pitch src_pitch) into dst (row pitch dst_pitch) with orientation o:
// 1 as stored, 2 mirror x, 3 mirror both, 4 mirror y, 5 transpose, 6 transpose then mirror x, 7 transpose then mirror both, 8 transpose then mirror y.
// For 5..8 the destination is w x h. Any base alignment, any pitch of at least a row.
struct OrientJob {
  const unsigned char* src;
  unsigned char* dst;
  long long src_pitch, dst_pitch;
  int h, w, o;
};
inline int orient_out_h(const OrientJob& j) { return j.o >= 5 ? j.w : j.h; }
inline int orient_out_w(const OrientJob& j) { return j.o >= 5 ? j.h : j.w; }

// Every argument is judged here, before anything is allocated, uploaded or launched: throws Error(FFP_ERR_ARG) for px other than 1, 3, 4, o outside
// 1..8, a pitch smaller than a row, dst_cap (bytes from j.dst on) smaller than (h' - 1) * dst_pitch + w' * px, and source and destination byte
// ranges that overlap. Host code only.
void orient_check(const OrientJob& j, int px, long long dst_cap);

// jobs[0..n) in ONE launch (a workgroup finds its image by bisection on first-workgroup indices). The jobs have passed orient_check and their
// destinations do not overlap one another. The table goes up through a pooled workspace; synchronises `st`. n == 0: nothing is launched.
void orient_batch_device(const OrientJob* jobs, int n, int px, hipStream_t st);

// The launch alone, for tools/orient_probe.py: `iters` launches of the packed image j between two events, and as many device-to-device copies of the
// same h * w * px bytes from j.src to j.dst between two more (what the memory system allows). j has passed orient_check with both pitches packed.
// Leaves the copy in j.dst; moves no counter; synchronises `st`.
void orient_time_device(const OrientJob& j, int px, int iters, float* kernel_us, float* copy_us, hipStream_t st);

// images turned and launches queued since load
void orient_stats(long long* images, long long* launches);

}  // namespace ffp
