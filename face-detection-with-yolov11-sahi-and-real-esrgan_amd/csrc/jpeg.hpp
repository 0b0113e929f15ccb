// jpeg.hpp — baseline JPEG at the file boundaries: encoding of device-resident images (jpeg.hip) and decoding into
// device memory (jpeg_dec.cpp: markers and the host decoder; jpeg_huff.hip: entropy decoding on the device; jpeg.hip: reconstruction).
// Both directions have one routine for n images; the single-image entries call it with n == 1.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace ffp {

// SOI .. SOS of the file libjpeg writes for an h x w three-component 4:2:0 baseline image at `quality`
std::vector<unsigned char> jpeg_header(int h, int w, int quality);

// One launch sequence for a whole batch of device-resident images (e.g. the enhanced crops of a frame in the SR output buffer):
// files[i] = the JFIF file of src[i]. Two stream synchronisations per batch, whatever its size.
struct JpegSrc { const unsigned char* d_img; int h, w; long long stride; };
void jpeg_encode_batch_device(const JpegSrc* src, int n_img, int bgr, int quality, std::vector<std::vector<unsigned char>>& files, hipStream_t st);

// Encodes the h x w x 3 uint8 image at d_img (row pitch `stride` bytes, channel order RGB or BGR) into `out` (host, `cap` bytes):
// the whole JFIF file. Returns its size, or minus the size needed when out is null or too small. Synchronises `st`.
long long jpeg_encode_device(const unsigned char* d_img, int h, int w, long long stride, int bgr, int quality, unsigned char* out, long long cap, hipStream_t st);

// ---- decoding: the markers (jpeg_dec.cpp) ------------------------------------------------------------------------------------------------
struct JpegComp { int hs = 1, vs = 1, tq = 0, td = 0, ta = 0, blocks_x = 0, blocks_y = 0; };
struct JpegScan {
  int h = 0, w = 0, ncomp = 0, hmax = 1, vmax = 1;
  JpegComp comp[3];
  unsigned short qt[4][64];                     // natural order
  short* coef[3] = {nullptr, nullptr, nullptr}; // [blocks_y][blocks_x][64] natural order, quantised: caller's (pinned) memory, zeroed by the decoder
};
// what the device entropy decoder (jpeg_huff.hip) needs from the markers: the raw Huffman tables, the restart interval and where
// the entropy-coded segment starts
struct JpegHuffSpec { bool present = false; int n = 0; unsigned char bits[16]; unsigned char vals[256]; };
struct JpegHead { JpegHuffSpec dc[4], ac[4]; int dri = 0; long long data_off = 0; };
// markers + Huffman decoding of a baseline / extended-sequential 8-bit JFIF file (one interleaved scan, 1 or 3 components, chroma
// at full, half-width or half-width-half-height resolution; restart intervals). Throws ffp::Error on anything else.
void jpeg_entropy_decode(const unsigned char* data, long long n, JpegScan& out, bool header_only, JpegHead* head = nullptr);

// ---- decoding: n files in one pass (jpeg_huff.hip; the layout: jpeg_batch_plan.hpp; reconstruction: jpeg.hip) -----------------------------
// The one decoding routine. n files -> n images at d_base + offsets[i] (row pitch strides[i], 0 or strides == nullptr: packed). status[i]: 0
// decoded on the device, 1 by the host decoder, < 0 the FFP_ERR_* of a file that was not decoded: its region is untouched, and why[i] (n
// strings, or nullptr) is the text of the ffp::Error that refused it. A fixed number of launches, ONE upload, ONE memset, ONE download and
// TWO stream synchronisations per sub-batch, whatever n is; a file whose stream needs further rounds of synchronisation adds rounds for the
// sub-batch; a flagged file, a file outside the device decoder's limits (a scan of 256 MiB or more, more than six blocks per MCU) and every
// file under FFP_JPEG_HOST_HUFFMAN=1 goes to the host decoder alone. Throws FFP_ERR_ARG, before anything is queued, when a readable file's
// region does not lie inside cap. Calls on different threads run side by side: each borrows a workspace from a pool and uses its own `st`.
// cost (or nullptr): what the call queued, for the batch entries' counters (jpeg_batch_note).
struct JpegBatchCost { long long launches = 0, syncs = 0; };
void jpeg_decode_batch_to_device(int n, const unsigned char* const* datas, const long long* sizes, int bgr, unsigned char* d_base, const long long* offsets,
                                 const long long* strides, long long cap, int* hs, int* ws, int* status, std::string* why, JpegBatchCost* cost, hipStream_t st,
                                 const int* orientations = nullptr);
// orientations (n entries, or nullptr: every file as stored): the EXIF orientation applied to file i — 0 the file's own tag (exif.hpp), 1..8 that
// value. A turned file (2..8) is reconstructed into a pooled workspace image and turned into its region by the orient kernel (orient.hip): at most
// ONE more launch per sub-batch, whatever n is, and none when every file is 1; offsets, strides, cap, hs and ws then describe the ORIENTED image,
// and a file that is not decoded still leaves its region untouched. A value outside 0..8: FFP_ERR_ARG before anything is queued.
// One file is a batch of one: throws what the markers refuse and "output buffer too small" before anything is queued, and the recorded
// ffp::Error of a file that was not decoded (d_out is untouched then). stride 0: packed. Two stream synchronisations.
// orientation: as above (0: the file's own); stride, cap and out_h / out_w (or nullptr) are the oriented image's.
void jpeg_decode_to_device(const unsigned char* data, long long n, unsigned char* d_out, long long stride, long long cap, int bgr, hipStream_t st, int orientation = 1,
                           int* out_h = nullptr, int* out_w = nullptr);
// counters: files (both kinds of entry) decoded on the device / by the host decoder after the device decoder gave up / extra rounds of
// synchronisation; batches (ffp_jpeg_decode_batch* only: jpeg_batch_note) and the latest one's launches and synchronisations
void jpeg_huff_stats(long long* device_decodes, long long* host_fallbacks, long long* extra_sync_rounds);
void jpeg_batch_stats(long long* batches, long long* launches_last_batch, long long* syncs_last_batch);
void jpeg_batch_note(const JpegBatchCost& k);

// Reconstruction of a batch: per-component and per-image descriptors in device memory, sorted by their first workgroup (wg0), so that a
// workgroup finds its own by bisection. One launch per stage, whatever the number of images (jpeg.hip).
struct JpegBatchIdct { const short* coef; unsigned char* plane; const unsigned short* qt; int n_blocks, blocks_x, wg0, pad; };
struct JpegBatchColour {
  const unsigned char *py, *pcb, *pcr;
  unsigned char* out;
  long long stride;
  int h, w, pitch_y, pitch_c, ch, cw, hsub, vsub, ncomp, wg0, wgs_x, pad;
};
void jpeg_batch_reconstruct(const JpegBatchIdct* d_idct, int n_idct, int n_idct_wg, const JpegBatchColour* d_colour, int n_img, int n_px_wg, int bgr, hipStream_t st);

// ---- decoding: the host decoder's staging (jpeg.hip) ------------------------------------------------------------------------------------
// One host-decoded file in flight: pinned host coefficient planes (the entropy decoder writes them, the copies to the device run at full
// PCIe rate) and their device twins + sample planes; kept in a pool (jpeg_huff.hip) so that concurrent decodes neither allocate nor free
struct JpegDecodeWs {
  HostPinned host[3];                           // allocated on first use
  DevBuf coef_all, plane[3], qt;                // the three coefficient planes are one allocation
  short* dev[3] = {nullptr, nullptr, nullptr};  // component c's plane inside coef_all
  size_t cap[3] = {0, 0, 0};
  int device = 0;                               // the pool hands a workspace out only on the device it was made on
  JpegDecodeWs() = default;
  JpegDecodeWs(const JpegDecodeWs&) = delete;
  JpegDecodeWs& operator=(const JpegDecodeWs&) = delete;
  void ensure(const JpegScan& s);               // sizes the device planes for the scan
  void ensure_host(const JpegScan& s);          // ... and the pinned host planes, and points s.coef at them
  size_t held() const { return host[0].n + host[1].n + host[2].n + coef_all.n + plane[0].n + plane[1].n + plane[2].n + qt.n; }
};
// the coefficients in s.coef (host decoder) go up; dequantisation + integer IDCT + upsampling + colour conversion into d_out (h x w x 3
// uint8, row pitch `stride`, RGB or BGR). Queues on `st`, no synchronisation: the caller waits for `st` before ws goes back to its pool.
void jpeg_reconstruct_device(const JpegScan& s, JpegDecodeWs& ws, unsigned char* d_out, long long stride, int bgr, hipStream_t st);

}  // namespace ffp

