// scrfd.cpp — InsightFace's SCRFD face detector (model_zoo/retinaface.py, class RetinaFace) over a batch of crops of one frame.
//
// The ONNX graph is lowered once per (batch, net size) into a plan: convs (BatchNormalization and the bbox Scale folded in, ReLU and
// residual Add fused into the epilogue) on the shared MFMA kernels, pools and x2 upsamples in between, and the heads read in place by
// the decode. Every crop of a call is resized into the top-left of the same net size, so one plan serves the whole batch.
#include "scrfd.hpp"

#include <cmath>
#include <cstdlib>

namespace ffp {

void scrfd_geometry(int h, int w, int net_w, int net_h, int* new_w, int* new_h, float* det_scale) {
  const double im_ratio = (double)h / (double)w, model_ratio = (double)net_h / (double)net_w;
  int nw, nh;
  if (im_ratio > model_ratio) { nh = net_h; nw = (int)((double)nh / im_ratio); }
  else { nw = net_w; nh = (int)((double)nw * im_ratio); }
  *new_w = nw; *new_h = nh;
  *det_scale = (float)((double)nh / (double)h);
}

ScrfdEngine::ScrfdEngine(const void* onnx_bytes, size_t nbytes, int n, int device, int precision) {
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "scrfd: precision %d (FFP_PREC_F32 or FFP_PREC_F32X3)", precision);
  graph_ = onnx::parse(onnx_bytes, nbytes);
  (void)onnx::lower(graph_, n, 640, 640);       // refuse a graph outside the subset (at the expected batch) before touching the device
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, FFP_ERR_HIP, "no HIP device available (the detector has no CPU path)");
  FFP_CHECK(device >= 0 && device < ndev, FFP_ERR_ARG, "device %d of %d", device, ndev);
  device_ = device;
  split_ = precision == FFP_PREC_F32X3;
  FFP_HIP(hipSetDevice(device_));
  st_ = create_engine_stream(sw().det_cu_mask);
  conv_kernels_init();
}

ScrfdEngine::~ScrfdEngine() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  plans_.clear_nothrow();
  if (st_) (void)hipStreamDestroy(st_);
}

void ScrfdEngine::build_plan(ScrfdPlan& P, int n, int det_w, int det_h) {
  P.low = onnx::lower(graph_, n, det_w, det_h);
  const onnx::Lowered& L = P.low;
  P.per_image_amax = split_;                   // an image's exponent of the scaled split depends on that image alone
  P.px_align = split_ ? 32 : 1;
  std::map<int, Level*> lv;
  for (const onnx::LBuf& b : L.bufs)
    if (!lv.count(b.stride)) lv[b.stride] = P.add_level(std::vector<int>(n, L.det_h / b.stride), std::vector<int>(n, L.det_w / b.stride), st_);
  for (const onnx::LBuf& b : L.bufs) P.views.push_back(P.alloc(lv.at(b.stride), b.C, F32));
  for (DevBuf& b : P.bufs) FFP_HIP(hipMemsetAsync(b.p, 0, b.n, st_));     // padding channels are read (times zero weights): never garbage
  P.set_amax_bound(P.views[L.input_buf], 1.0f);                            // |(v - 127.5) / 128| < 1
  auto view = [&](const onnx::LView& v, int C) {
    const TView& b = P.views.at(v.buf);
    FFP_CHECK(v.coff + C <= b.cs, FFP_ERR_STATE, "scrfd: view of %d channels at %d outside a %d-channel buffer", C, v.coff, b.cs);
    return b.slice(v.coff, C);
  };
  auto pad4 = [](int c) { return (c + 3) / 4 * 4; };
  for (const onnx::LStep& s : L.steps) {
    if (s.kind == onnx::ST_CONV) {
      P.convs.emplace_back(new PackedConv());
      PackedConv& pc = *P.convs.back();
      pack_conv(pc, s.node, s.w.data(), s.b.data(), s.cout, s.cin, s.k, 1, F32, st_, split_);
      ConvOp o;
      o.pc = &pc;
      o.in = view(s.in, pc.cin);
      o.out = view(s.out, s.cout);
      o.stride = s.stride;
      o.act = s.act;
      o.act_post = s.act_post;
      if (s.res.buf >= 0) { o.has_res1 = true; o.res1 = view(s.res, s.cout); o.s1 = 1.f; }
      P.add_conv(o);
    } else if (s.kind == onnx::ST_UP2) {
      const TView in = view(s.in, pad4(s.cin)), out = view(s.out, pad4(s.cin));
      P.add([in, out](hipStream_t q) { launch_upsample2x(in, out, q); launch_amax_max(out.amax, in.amax, q, out.amax_n); });
    } else {
      const TView in = view(s.in, s.cin), out = view(s.out, s.cin);
      const int mx = s.kind == onnx::ST_MAXPOOL ? 1 : 0, k = s.k;
      P.add([in, out, mx, k](hipStream_t q) { launch_scrfd_pool(in, out, mx, k, q); launch_amax_max(out.amax, in.amax, q, out.amax_n); });
    }
  }
  P.add_amax_reset(st_);      // first step of every run
  // ---- decode of the three levels ---------------------------------------------------------------------------------------------
  ScrfdHeads& h = P.heads;
  h.A = L.num_anchors;
  h.a_off[0] = 0;
  for (int l = 0; l < 3; ++l) {
    const onnx::LOutput& os = L.outs[l];
    const onnx::LOutput& ob = L.outs[3 + l];
    const TView& vs = P.views[os.v.buf];
    const TView& vb = P.views[ob.v.buf];
    h.score[l] = (const float*)vs.ptr; h.cs[0][l] = vs.cs; h.coff[0][l] = os.v.coff;
    h.bbox[l] = (const float*)vb.ptr; h.cs[1][l] = vb.cs; h.coff[1][l] = ob.v.coff;
    h.kps[l] = nullptr; h.cs[2][l] = 0; h.coff[2][l] = 0;
    if (L.use_kps) {
      const onnx::LOutput& ok = L.outs[6 + l];
      const TView& vk = P.views[ok.v.buf];
      h.kps[l] = (const float*)vk.ptr; h.cs[2][l] = vk.cs; h.coff[2][l] = ok.v.coff;
    }
    h.tab[l] = vs.lvl->d_tab.as<int4>();
    h.stride[l] = os.stride;
    h.a_off[l + 1] = h.a_off[l] + (L.det_h / os.stride) * (L.det_w / os.stride) * h.A;
  }
  h.per_img = h.a_off[3];
  P.d_lb.alloc(sizeof(LetterboxImg) * n);
  P.d_scale.alloc(sizeof(float) * n);
  h.det_scale = P.d_scale.as<float>();
  P.d_cand.alloc(sizeof(ScrfdCand) * (size_t)n * h.per_img);    // no candidate cap: every anchor of every image fits
  P.d_counts.alloc(sizeof(int) * n);
  P.d_order.alloc(sizeof(int) * (size_t)n * h.per_img);
  P.d_supp.alloc(sizeof(int) * (size_t)n * h.per_img);
  P.d_out_counts.alloc(sizeof(int) * n);
  P.bytes += P.d_cand.n + P.d_order.n + P.d_supp.n;
  FFP_HIP(hipStreamSynchronize(st_));
}

ScrfdPlan* ScrfdEngine::plan_for(int n, int det_w, int det_h) {
  return &plans_.get({n, det_w, det_h}, [&] {
    std::unique_ptr<ScrfdPlan> p(new ScrfdPlan());
    build_plan(*p, n, det_w, det_h);
    return p;
  });
}

ScrfdPlan* ScrfdEngine::prepare(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h) {
  FFP_CHECK(frame && H > 0 && W > 0 && tiles && n_tiles > 0, FFP_ERR_ARG, "scrfd: empty frame or tile list");
  FFP_CHECK(det_w % 32 == 0 && det_h % 32 == 0 && det_w >= 32 && det_h >= 32, FFP_ERR_ARG, "scrfd: det size %dx%d must be multiples of 32", det_w, det_h);
  FFP_HIP(hipSetDevice(device_));
  ScrfdPlan* P = plan_for(n_tiles, det_w, det_h);
  tile_geometry(*P, H, W, tiles, n_tiles);
  upload_frame(frame_, frame, H, W, st_);
  run_chunk(P, frame_.as<uint8_t>(), W, chan_order, 0, n_tiles);
  FFP_HIP(hipStreamSynchronize(st_));
  return P;
}

void scrfd_tile_records(int net_w, int net_h, int H, int W, const int32_t* tiles, int n_tiles, std::vector<LetterboxImg>& lb, std::vector<float>& scale) {
  lb.resize(n_tiles);
  scale.resize(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    const int x0 = tiles[4 * i], y0 = tiles[4 * i + 1], x1 = tiles[4 * i + 2], y1 = tiles[4 * i + 3];
    FFP_CHECK(x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x1 > x0 && y1 > y0, FFP_ERR_ARG, "tile %d [%d,%d,%d,%d] outside %dx%d frame", i, x0, y0,
              x1, y1, W, H);
    LetterboxImg& L = lb[i];
    L.x0 = x0; L.y0 = y0; L.sw = x1 - x0; L.sh = y1 - y0;
    scrfd_geometry(L.sh, L.sw, net_w, net_h, &L.new_w, &L.new_h, &scale[i]);
    FFP_CHECK(L.new_w > 0 && L.new_h > 0, FFP_ERR_ARG, "tile %d (%dx%d) resizes to %dx%d at net size %dx%d (cv2.resize would raise)", i, L.sw, L.sh,
              L.new_w, L.new_h, net_w, net_h);
    L.top = 0; L.left = 0; L.net_h = net_h; L.net_w = net_w;
  }
}

void ScrfdEngine::tile_geometry(const ScrfdPlan& first, int H, int W, const int32_t* tiles, int n_tiles) {
  scrfd_tile_records(first.low.det_w, first.low.det_h, H, W, tiles, n_tiles, h_lb_, h_scale_);     // a fixed input size of the file wins
}

void ScrfdEngine::run_chunk(ScrfdPlan* P, const uint8_t* d_frame, int W, int chan_order, int off, int m) {
  FFP_HIP(hipMemcpyAsync(P->d_lb.p, h_lb_.data() + off, sizeof(LetterboxImg) * m, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(P->d_scale.p, h_scale_.data() + off, sizeof(float) * m, hipMemcpyHostToDevice, st_));
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  launch_scrfd_preproc(d_frame, W, flip, P->d_lb.as<LetterboxImg>(), P->views[P->low.input_buf], st_);
  P->execute(st_, nullptr);
  last_conv_flops = P->conv_flops;
  last_graph_state = P->graph_state();
}

void ScrfdEngine::infer_tiles(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                              float det_thresh, float nms_thresh, float* out, int cap, int32_t* out_counts) {
  FFP_CHECK(cap >= 1 && out && out_counts, FFP_ERR_ARG, "scrfd: cap must be >= 1 and outputs non-null");
  ScrfdPlan* P = prepare(frame, H, W, chan_order, tiles, n_tiles, det_w, det_h);
  const ScrfdHeads& h = P->heads;
  const size_t ob = sizeof(float) * (size_t)n_tiles * cap * FFP_DET_STRIDE(5);
  P->d_out.ensure(ob);
  launch_scrfd_decode(h, n_tiles, det_thresh, P->d_cand.as<ScrfdCand>(), P->d_counts.as<int>(), nullptr, st_);
  launch_scrfd_nms(P->d_cand.as<ScrfdCand>(), P->d_counts.as<int>(), n_tiles, h.per_img, P->d_order.as<int>(), P->d_supp.as<int>(), nms_thresh,
                   P->d_out.as<float>(), cap, P->d_out_counts.as<int>(), st_);
  FFP_HIP(hipMemcpyAsync(out, P->d_out.p, ob, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(out_counts, P->d_out_counts.p, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
  for (int i = 0; i < n_tiles; ++i)
    FFP_CHECK(out_counts[i] <= cap, FFP_ERR_ARG, "scrfd: tile %d kept %d faces, the output holds %d per tile", i, out_counts[i], cap);
}

void ScrfdEngine::forward_raw(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h, float* out,
                              size_t cap, int64_t* out_sizes) {
  ScrfdPlan* P = prepare(frame, H, W, chan_order, tiles, n_tiles, det_w, det_h);
  const ScrfdHeads& h = P->heads;
  const onnx::Lowered& L = P->low;
  const int no = (int)L.outs.size();
  size_t per_tile = 0;
  for (int k = 0; k < no; ++k) {
    const int hw = (L.det_h / L.outs[k].stride) * (L.det_w / L.outs[k].stride);
    out_sizes[k] = (int64_t)hw * L.outs[k].v.C;
    per_tile += (size_t)out_sizes[k];
  }
  FFP_CHECK(per_tile * n_tiles <= cap, FFP_ERR_ARG, "scrfd forward_raw: output needs %zu floats, capacity %zu", per_tile * n_tiles, cap);
  P->d_raw_scores.ensure(sizeof(float) * (size_t)n_tiles * h.per_img);
  launch_scrfd_decode(h, n_tiles, 0.f, nullptr, nullptr, P->d_raw_scores.as<float>(), st_);     // the decode's own sigmoid
  std::vector<float> sc((size_t)n_tiles * h.per_img);
  FFP_HIP(hipMemcpyAsync(sc.data(), P->d_raw_scores.p, sizeof(float) * sc.size(), hipMemcpyDeviceToHost, st_));
  std::vector<std::vector<float>> host(P->views.size());
  for (int k = no / 3; k < no; ++k) {        // distance outputs: the conv buffers as stored (NHWC == the graph's Transpose + Reshape)
    const int b = L.outs[k].v.buf;
    if (!host[b].empty()) continue;
    const TView& v = P->views[b];
    host[b].resize((size_t)v.lvl->total_px * v.cs);
    FFP_HIP(hipMemcpyAsync(host[b].data(), v.ptr, sizeof(float) * host[b].size(), hipMemcpyDeviceToHost, st_));
  }
  FFP_HIP(hipStreamSynchronize(st_));
  float* o = out;
  for (int i = 0; i < n_tiles; ++i) {
    for (int k = 0; k < no; ++k) {
      const onnx::LOutput& ou = L.outs[k];
      const int l = k % 3;
      if (ou.kind == 0) {
        const float* s = sc.data() + (size_t)i * h.per_img + h.a_off[l];
        std::copy(s, s + out_sizes[k], o);
      } else {
        const TView& v = P->views[ou.v.buf];
        const Level& lv = *v.lvl;
        const int hw = lv.h[i] * lv.w[i];
        for (int p = 0; p < hw; ++p)
          for (int c = 0; c < ou.v.C; ++c) o[(size_t)p * ou.v.C + c] = host[ou.v.buf][((size_t)lv.off[i] + p) * v.cs + ou.v.coff + c];
      }
      o += out_sizes[k];
    }
  }
}

// ---- tiles of one frame in chunks, and sahi's get_sliced_prediction over InsightFaceDetectionModel in one call ------------------------

void ScrfdEngine::enqueue_tiles(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                                float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* d_out, int cap, int32_t* d_out_counts) {
  FFP_CHECK(d_frame && H > 0 && W > 0 && tiles && n_tiles > 0, FFP_ERR_ARG, "scrfd: empty frame or tile list");
  FFP_CHECK(d_out && d_out_counts && cap >= 1, FFP_ERR_ARG, "scrfd: cap must be >= 1 and outputs non-null");
  FFP_CHECK((long long)n_tiles * cap < (1ll << 31) / FFP_DET_STRIDE(5), FFP_ERR_ARG, "scrfd: %d tiles of %d rows", n_tiles, cap);
  FFP_CHECK(det_w % 32 == 0 && det_h % 32 == 0 && det_w >= 32 && det_h >= 32, FFP_ERR_ARG, "scrfd: det size %dx%d must be multiples of 32", det_w, det_h);
  FFP_CHECK(chan_order == FFP_CHAN_AS_BGR || chan_order == FFP_CHAN_AS_RGB, FFP_ERR_ARG, "scrfd: chan_order %d", chan_order);
  FFP_CHECK(mode == FFP_SCRFD_TILES_LOCAL || mode == FFP_SCRFD_TILES_SAHI, FFP_ERR_ARG, "scrfd: tile mode %d (FFP_SCRFD_TILES_LOCAL or FFP_SCRFD_TILES_SAHI)",
            mode);
  FFP_HIP(hipSetDevice(device_));
  // this engine's sentinels: below 0 asks for the default, 0 (or more than there are) for one batch, as infer_tiles runs them
  max_batch = max_batch < 0 ? SCRFD_TILES_DEFAULT_BATCH : max_batch == 0 || max_batch > n_tiles ? n_tiles : max_batch;
  const std::vector<int> chunks = even_chunks(n_tiles, max_batch);      // 13 at 5: 5, 4, 4
  tile_geometry(*plan_for(chunks[0], det_w, det_h), H, W, tiles, n_tiles);
  int off = 0;
  for (int m : chunks) {
    ScrfdPlan* P = plan_for(m, det_w, det_h);        // an eviction waits for the stream first
    run_chunk(P, d_frame, W, chan_order, off, m);
    const ScrfdHeads& h = P->heads;
    launch_scrfd_decode(h, m, det_thresh, P->d_cand.as<ScrfdCand>(), P->d_counts.as<int>(), nullptr, st_);
    // straight into the call-wide buffers at the chunk's tile offset
    launch_scrfd_nms(P->d_cand.as<ScrfdCand>(), P->d_counts.as<int>(), m, h.per_img, P->d_order.as<int>(), P->d_supp.as<int>(), nms_thresh,
                     d_out + (size_t)off * cap * FFP_DET_STRIDE(5), cap, d_out_counts + off, st_);
    off += m;
  }
  h_counts_.assign(n_tiles, 0);                       // the NMS counts (not capped), before the SAHI rule rewrites them
  FFP_HIP(hipMemcpyAsync(h_counts_.data(), d_out_counts, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st_));
  h_err_ = SCRFD_NO_BAD_ROW;
  if (mode == FFP_SCRFD_TILES_SAHI) {
    tiles_xy_.ensure(sizeof(int4) * n_tiles);
    err_.ensure(sizeof(unsigned));
    FFP_HIP(hipMemcpyAsync(tiles_xy_.p, tiles, sizeof(int4) * n_tiles, hipMemcpyHostToDevice, st_));
    launch_scrfd_sahi_rows(d_out, d_out_counts, tiles_xy_.as<int4>(), n_tiles, cap, conf, H, W, err_.as<unsigned>(), st_);
    FFP_HIP(hipMemcpyAsync(&h_err_, err_.p, sizeof(unsigned), hipMemcpyDeviceToHost, st_));
  }
}

void ScrfdEngine::check_tiles(int n_tiles, int cap, int mode) {
  for (int i = 0; i < n_tiles; ++i)
    FFP_CHECK(h_counts_[i] <= cap, FFP_ERR_ARG, "scrfd: tile %d kept %d faces, the output holds %d per tile", i, h_counts_[i], cap);
  if (mode == FFP_SCRFD_TILES_SAHI && h_err_ != SCRFD_NO_BAD_ROW)
    FFP_CHECK(false, FFP_ERR_ARG, "scrfd: tile %d row %d: Box coords [minx, miny, maxx, maxy] cannot be negative (the box's far corner is negative after "
              "the clip; sahi's BoundingBox raises here and the frame fails)", (int)(h_err_ / (unsigned)cap), (int)(h_err_ % (unsigned)cap));
}

void ScrfdEngine::infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                                  float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* d_out, int cap, int32_t* d_out_counts) {
  enqueue_tiles(d_frame, H, W, chan_order, tiles, n_tiles, det_w, det_h, det_thresh, nms_thresh, conf, mode, max_batch, d_out, cap, d_out_counts);
  FFP_HIP(hipStreamSynchronize(st_));
  check_tiles(n_tiles, cap, mode);
}

void ScrfdEngine::infer_tiles_ex(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int det_w, int det_h,
                                 float det_thresh, float nms_thresh, float conf, int mode, int max_batch, float* out, int cap, int32_t* out_counts) {
  FFP_CHECK(frame && H > 0 && W > 0 && tiles && n_tiles > 0, FFP_ERR_ARG, "scrfd: empty frame or tile list");
  FFP_CHECK(cap >= 1 && out && out_counts, FFP_ERR_ARG, "scrfd: cap must be >= 1 and outputs non-null");
  FFP_CHECK((long long)n_tiles * cap < (1ll << 31) / FFP_DET_STRIDE(5), FFP_ERR_ARG, "scrfd: %d tiles of %d rows", n_tiles, cap);
  FFP_HIP(hipSetDevice(device_));
  upload_frame(frame_, frame, H, W, st_);
  const size_t ob = sizeof(float) * (size_t)n_tiles * cap * FFP_DET_STRIDE(5);
  tile_dets_.ensure(ob);
  tile_counts_.ensure(sizeof(int) * n_tiles);
  FFP_HIP(hipMemsetAsync(tile_dets_.p, 0, ob, st_));       // rows past a tile's count read as zeros
  enqueue_tiles(frame_.as<uint8_t>(), H, W, chan_order, tiles, n_tiles, det_w, det_h, det_thresh, nms_thresh, conf, mode, max_batch,
                tile_dets_.as<float>(), cap, tile_counts_.as<int>());
  FFP_HIP(hipMemcpyAsync(out, tile_dets_.p, ob, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(out_counts, tile_counts_.p, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
  for (int i = 0; i < n_tiles; ++i)
    if (h_counts_[i] > cap) {            // the caller sizes its retry by the NMS counts (not capped), as with infer_tiles
      std::copy(h_counts_.begin(), h_counts_.end(), out_counts);
      break;
    }
  check_tiles(n_tiles, cap, mode);
}

void ScrfdEngine::merge_tiles(int n_tiles, int tile_cap, bool full_last, int H, int W, int pp_type, int pp_metric, double pp_thr, int class_agnostic,
                              float* d_out, int cap, int32_t* d_out_n) {
  constexpr int S = FFP_DET_STRIDE(5);
  const int n_max = n_tiles * tile_cap;
  tail_.compact(tile_dets_.as<float>(), tile_counts_.as<int>(), n_tiles, tile_cap, S, st_);
  int rows = 0, full_first = 0;              // the merge's grid follows the row count: one small read back between the two halves
  FFP_HIP(hipMemcpyAsync(&rows, tail_.rows_n.p, sizeof(int), hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(&full_first, tail_.prefix.as<int>() + (n_tiles - 1), sizeof(int), hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
  check_tiles(n_tiles, tile_cap, FFP_SCRFD_TILES_SAHI);
  FFP_CHECK(rows >= 0 && rows <= n_max, FFP_ERR_STATE, "scrfd: %d rows from %d tiles", rows, n_tiles);
  // one slice: its rows as they are, in score order; with more tiles sahi post-processes a list of two or more (sahi/predict.py)
  // the full-frame prediction is the one sahi does not shift, so it keeps its full_shape: a union it keeps is clipped to the frame
  tail_.merge(MergeRule::TwoOrMore, rows, pp_type, pp_metric, pp_thr, class_agnostic, d_out, nullptr, d_out_n, cap, st_,
              full_last ? full_first : 0x7fffffff, W, H);
}

void ScrfdEngine::sliced_predict_dev(const uint8_t* d_frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int det_w, int det_h,
                                     float det_thresh, float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric,
                                     double pp_thr, int class_agnostic, float* d_out, int cap, int32_t* d_out_n) {
  FFP_CHECK(d_out && d_out_n && cap > 0 && tile_cap > 0, FFP_ERR_ARG, "scrfd: sliced_predict needs an output of cap > 0 rows and tile_cap > 0");
  const int n_tiles = (int)items.size() / 4;
  FFP_CHECK(n_tiles > 0 && (long long)n_tiles * tile_cap < (1 << 24), FFP_ERR_ARG, "scrfd: no tile to run, or too many rows (%d tiles of %d)", n_tiles, tile_cap);
  FFP_HIP(hipSetDevice(device_));
  tile_dets_.ensure(sizeof(float) * (size_t)n_tiles * tile_cap * FFP_DET_STRIDE(5));
  tile_counts_.ensure(sizeof(int) * n_tiles);
  enqueue_tiles(d_frame, H, W, chan_order, items.data(), n_tiles, det_w, det_h, det_thresh, nms_thresh, conf, FFP_SCRFD_TILES_SAHI, max_batch,
                tile_dets_.as<float>(), tile_cap, tile_counts_.as<int>());
  const int32_t* last = items.data() + 4 * (n_tiles - 1);          // more than one slice: none of them is the whole frame
  const bool full_last = n_tiles > 1 && last[0] == 0 && last[1] == 0 && last[2] == W && last[3] == H;
  merge_tiles(n_tiles, tile_cap, full_last, H, W, pp_type, pp_metric, pp_thr, class_agnostic, d_out, cap, d_out_n);
  FFP_HIP(hipStreamSynchronize(st_));
}

void ScrfdEngine::sliced_predict(const uint8_t* frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int det_w, int det_h,
                                 float det_thresh, float nms_thresh, float conf, int max_batch, int tile_cap, int pp_type, int pp_metric, double pp_thr,
                                 int class_agnostic, float* out, int cap, int32_t* out_n) {
  FFP_CHECK(frame && H > 0 && W > 0 && out && out_n && cap > 0, FFP_ERR_ARG, "scrfd: sliced_predict needs a frame and an output of cap > 0 rows");
  constexpr int S = FFP_DET_STRIDE(5);
  FFP_HIP(hipSetDevice(device_));
  upload_frame(frame_, frame, H, W, st_);
  tail_.reserve(cap, S);
  sliced_predict_dev(frame_.as<uint8_t>(), H, W, chan_order, items, det_w, det_h, det_thresh, nms_thresh, conf, max_batch, tile_cap, pp_type, pp_metric,
                     pp_thr, class_agnostic, tail_.merged.as<float>(), cap, tail_.merged_n.as<int>());
  tail_.fetch(out, cap, S, out_n, "scrfd: sliced_predict", nullptr);      // sliced_predict_dev has drained the stream
}

}  // namespace ffp
