// api_util.hpp — what the C-ABI files (api.cpp, api_eval.cpp, api_codec.cpp, api_ops.cpp) share: the entry-point frame, small upload helpers and the
// scoped holders of a per-call stream and of HIP events. Host code only: no .hip kernel file includes this header.
#pragma once
#include <algorithm>
#include <utility>

#include "engine.hpp"

namespace ffp {

const std::string& last_error();

#define FFP_API_BEGIN try { ffp::ApiShared gate_share_;
#define FFP_API_END                                                              \
  return FFP_OK;                                                                 \
  }                                                                              \
  catch (const ffp::Error& e) { ffp::set_last_error(e.what()); return e.code; } \
  catch (const std::bad_alloc&) { ffp::set_last_error("host out of memory"); return FFP_ERR_NOMEM; } \
  catch (const std::exception& e) { ffp::set_last_error(e.what()); return FFP_ERR_STATE; }

template <typename T> DevBuf upload(const T* src, size_t n) {
  DevBuf b(std::max<size_t>(n, 1) * sizeof(T));
  if (n) FFP_HIP(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return b;
}
// A fill that has run when this returns. hipMemset queues the fill on the null stream and returns before it has run, and the streams the entries
// work on are non-blocking (ScopedStream): nothing orders a kernel on one of them behind such a fill. With other work on the card the 0xFF fill of
// an output buffer landed on top of what the kernel had written: ffp_op_image_input on one 64 x 64 box returned all NaN in 872 of 4000 calls while
// another thread kept the card busy, and in none with this wait (tests/test_gpu_image_input.py failed that way once in a while on a shared card).
inline void fill_bytes(void* p, int value, size_t n) {
  FFP_HIP(hipMemset(p, value, n));
  FFP_HIP(hipStreamSynchronize(nullptr));
}
inline void check_offsets(const int64_t* off, int n, const char* what) {
  FFP_CHECK(off && off[0] == 0, FFP_ERR_ARG, "%s offsets must start at 0", what);
  for (int i = 0; i < n; ++i) FFP_CHECK(off[i + 1] >= off[i], FFP_ERR_ARG, "%s offsets must not decrease (image %d)", what, i);
}

// The device and a stream of its own for one call of an entry that takes a device number instead of a handle: the device is checked and made current,
// the stream is of the kind asked for, and on every exit — return or throw — it is waited for and destroyed. Declare it before the call's DevBuf, Level and
// PackedConv objects, so that they are released first. Every entry drains the stream before it returns, so the wait only matters on a throw: uploads
// from host tables (hipMemcpyAsync) may still be in flight then.
struct ScopedStream {
  enum Kind {
    Plain,      // non-blocking
    // The file boundaries run beside the detector and the enhancer, whose persistent workgroups hold every CU for the length of a layer: a low-occupancy
    // chain of small kernels (the JPEG / PNG codecs) on an ordinary stream gets a turn only at kernel boundaries and stretches to tens of milliseconds.
    // Their streams therefore have the highest priority the device offers.
    Io,
  };
  hipStream_t st = nullptr;
  static void use_device(int device, const char* what) {      // the constructor's first step, for an entry that may return before it needs a stream
    int ndev = 0;
    FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev, FFP_ERR_HIP, "%s: no HIP device %d (no CPU path)", what, device);
    FFP_HIP(hipSetDevice(device));
  }
  ScopedStream(int device, const char* what, Kind kind = Plain) {
    use_device(device, what);
    if (kind == Io) {
      int least = 0, greatest = 0;
      FFP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      FFP_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
    } else {
      FFP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
  }
  ~ScopedStream() {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  ScopedStream(const ScopedStream&) = delete;
  ScopedStream& operator=(const ScopedStream&) = delete;
};

// One HIP event, destroyed on every exit.
struct ScopedEvent {
  hipEvent_t ev = nullptr;
  ScopedEvent() { FFP_HIP(hipEventCreate(&ev)); }
  ~ScopedEvent() { if (ev) (void)hipEventDestroy(ev); }
  ScopedEvent(ScopedEvent&& o) noexcept : ev(std::exchange(o.ev, nullptr)) {}
  ScopedEvent(const ScopedEvent&) = delete;
  ScopedEvent& operator=(const ScopedEvent&) = delete;
  operator hipEvent_t() const { return ev; }
};

}  // namespace ffp
