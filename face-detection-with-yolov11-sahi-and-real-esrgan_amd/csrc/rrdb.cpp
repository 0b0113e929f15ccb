// rrdb.cpp — Real-ESRGAN: RRDBNet as a plan of MFMA convolutions over a ragged batch of tiles.
//
// Network: basicsr RRDBNet(3, 3, 64, num_block, 32, scale) as the reference builds it at utils/enhancer.py:99-128
// (SURVEY.md Appendix D.1). Dense-block concatenations are virtual: each RDB works inside one [pixel][192] buffer
// (x | x1 | x2 | x3 | x4), conv5 writes the next RDB's x slot with the `*0.2 + x` residual(s) fused in its epilogue;
// nearest x2 upsampling is folded into the loader of conv_up1/conv_up2.
// Tiling: RealESRGANer.tile_process (Appendix D.2) — every padded tile of every image becomes one image of the ragged batch.
#include "sr_ops.hpp"

#include <cmath>

namespace ffp {

void resize_lanczos4_dev(const void* d_src, int h, int w, int cn, int wide, int out_h, int out_w, void* d_dst, DevBuf& tab,
                         std::vector<uint8_t>& host_tab, hipStream_t st) {
  host_tab.resize(lanczos4_table_bytes(out_h, out_w));
  lanczos4_pack(lanczos4_axis(w, out_w), lanczos4_axis(h, out_h), wide, host_tab.data());
  tab.ensure(host_tab.size());
  FFP_HIP(hipMemcpyAsync(tab.p, host_tab.data(), host_tab.size(), hipMemcpyHostToDevice, st));
  launch_resize_lanczos4(d_src, h, w, cn, wide, tab.p, out_h, out_w, d_dst, st);
}

SrEngine::SrEngine(const void* weights, size_t nbytes, int scale, int num_block, int device, int half) {
  FFP_CHECK(scale == 4 || scale == 2, FFP_ERR_ARG, "scale must be 4 or 2");
  FFP_CHECK(num_block >= 1 && num_block <= 64, FFP_ERR_ARG, "num_block");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, FFP_ERR_HIP, "no HIP device available (the enhancer has no CPU path)");
  FFP_CHECK(device >= 0 && device < ndev, FFP_ERR_ARG, "device %d of %d", device, ndev);
  scale_ = scale; num_block_ = num_block; device_ = device; dt_ = half ? F16 : F32;
  FFP_HIP(hipSetDevice(device_));
  st_ = create_engine_stream(sw().sr_cu_mask);
  for (auto& e : ev_) FFP_HIP(hipEventCreate(&e));
  conv_kernels_init();
  WeightFile wf;
  wf.parse(weights, nbytes);
  auto add = [&](const std::string& n) { pack_conv(convs_[n], wf, n, 3, 1, dt_, st_); };
  add("conv_first");
  for (int b = 0; b < num_block_; ++b)
    for (int r = 1; r <= 3; ++r)
      for (int c = 1; c <= 5; ++c) add("body." + std::to_string(b) + ".rdb" + std::to_string(r) + ".conv" + std::to_string(c));
  add("conv_body"); add("conv_up1"); add("conv_up2"); add("conv_hr"); add("conv_last");
  const int cin_first = 3 * (scale_ == 2 ? 4 : 1);
  FFP_CHECK(conv("conv_first")->cin_real == cin_first && conv("conv_first")->cout == 64, FFP_ERR_WEIGHTS,
            "conv_first is %d->%d, scale %d expects %d->64", conv("conv_first")->cin_real, conv("conv_first")->cout, scale_, cin_first);
  // opt-in (FFP_TRUNK=1 or ffp_sr_set_fused_body): measured on MI355X it is bit-identical to, and 6 % slower than, the per-layer launches at 320 crops
  // and 2x slower at 32 (profiles/r04_sr_batch_sweep.txt) — the shipped default stays the faster path
  fused_body_ = dt_ == F16 && sw().trunk;
  for (const auto& kv : convs_) weight_bytes_ += kv.second.w.n + kv.second.w16.n + kv.second.bias.n + kv.second.w_direct.n;
}

void SrEngine::set_fused_body(bool on) {
  on = on && dt_ == F16;
  if (on == fused_body_) return;
  plans_.clear();
  fused_body_ = on;
}

SrEngine::~SrEngine() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  plans_.clear_nothrow();
  convs_.clear();
  for (auto& e : ev_) (void)hipEventDestroy(e);
  if (st_) (void)hipStreamDestroy(st_);
}

const PackedConv* SrEngine::conv(const std::string& name) const {
  auto it = convs_.find(name);
  FFP_CHECK(it != convs_.end(), FFP_ERR_WEIGHTS, "conv '%s' missing from the weight container", name.c_str());
  return &it->second;
}

// capacity buckets: 64 * {1, 1.5, 2, 3, 4, 6, ...} 16x16 tiles at the body level (at most 1.5x the batch)
static int capacity_bucket(long long t16) {
  long long b = 64;
  for (;;) {
    if (t16 <= b) return (int)b;
    if (t16 <= b + b / 2) return (int)(b + b / 2);
    b *= 2;
    FFP_CHECK(b < (1ll << 22), FFP_ERR_ARG, "enhance: batch of %lld tiles is too large", t16);
  }
}

void SrEngine::build_plan(SrPlan& P, int cap_t16) {
  // every image has at least one tile and a tile at most 256 pixels; x2 / x4 levels scale by 4 / 16
  P.cap_t16 = cap_t16;
  P.Lb = P.add_level_capacity(cap_t16, 256ll * cap_t16, cap_t16, st_);
  P.L1 = P.add_level_capacity(cap_t16, 1024ll * cap_t16, 4 * cap_t16, st_);
  P.L2 = P.add_level_capacity(cap_t16, 4096ll * cap_t16, 16 * cap_t16, st_);
  const DType T = dt_;
  const int cin = conv("conv_first")->cin;     // padded to the vector width
  P.input = P.alloc(P.Lb, cin, T);
  TView feat = P.alloc(P.Lb, 64, T);
  TView ring[4];
  for (auto& r : ring) r = P.alloc(P.Lb, 192, T);

  // the body's convs are collected and added as ONE fused step (conv_trunk.hip) when the engine runs the fused body
  std::vector<ConvOp> body;
  bool collect = false;
  auto cv = [&](const std::string& name, const TView& in, const TView& out, int act, int up = 0, const TView* r1 = nullptr, float s1 = 1.f,
                const TView* r2 = nullptr, float s2 = 1.f) {
    ConvOp o;
    o.pc = conv(name); o.in = in; o.out = out; o.stride = 1; o.act = act; o.up = up;
    if (r1) { o.has_res1 = true; o.res1 = *r1; o.s1 = s1; }
    if (r2) { o.has_res2 = true; o.res2 = *r2; o.s2 = s2; }
    FFP_CHECK(o.pc->cin == in.C && o.pc->cout == out.C, FFP_ERR_WEIGHTS, "%s: weights are %d->%d, graph expects %d->%d", name.c_str(),
              o.pc->cin, o.pc->cout, in.C, out.C);
    if (collect) {
      FFP_CHECK(conv_trunk_layer_ok(o), FFP_ERR_STATE, "%s: not a layer the fused body launch can run", name.c_str());
      body.push_back(o);
    } else {
      P.add_conv(o);
    }
  };

  cv("conv_first", P.input, feat, ACT_NONE);
  cv("conv_first", P.input, ring[0].slice(0, 64), ACT_NONE);   // second copy inside the first dense buffer (3->64: negligible)
  int cur = 0;
  collect = fused_body_;
  for (int b = 0; b < num_block_; ++b) {
    const TView rrdb_in = ring[cur].slice(0, 64);
    for (int r = 1; r <= 3; ++r) {
      const std::string p = "body." + std::to_string(b) + ".rdb" + std::to_string(r);
      const TView& buf = ring[cur];
      const TView x = buf.slice(0, 64);
      for (int c = 1; c <= 4; ++c)
        cv(p + ".conv" + std::to_string(c), buf.slice(0, 64 + 32 * (c - 1)), buf.slice(64 + 32 * (c - 1), 32), ACT_LRELU);
      const int nxt = (cur + 1) & 3;
      const TView y = ring[nxt].slice(0, 64);
      if (r < 3) cv(p + ".conv5", buf, y, ACT_NONE, 0, &x, 0.2f);                       // x5*0.2 + x
      else cv(p + ".conv5", buf, y, ACT_NONE, 0, &x, 0.2f, &rrdb_in, 0.2f);             // (x5*0.2 + x)*0.2 + rrdb_in
      cur = nxt;
    }
    // ring[cur] now holds the RRDB output; the RRDB input slot (3 steps back == (cur+1)&3) is free again
  }
  collect = false;
  if (!body.empty()) P.add_trunk(body);
  TView feat2 = P.alloc(P.Lb, 64, T);
  cv("conv_body", ring[cur].slice(0, 64), feat2, ACT_NONE, 0, &feat, 1.0f);            // feat + conv_body(body)
  TView u1 = P.alloc(P.L1, 64, T);
  cv("conv_up1", feat2, u1, ACT_LRELU, 1);
  TView u2 = P.alloc(P.L2, 64, T);
  cv("conv_up2", u1, u2, ACT_LRELU, 1);
  TView hr = P.alloc(P.L2, 64, T);
  cv("conv_hr", u2, hr, ACT_LRELU);
  P.out = P.alloc(P.L2, 4, F32);
  cv("conv_last", hr, P.out.slice(0, 3), ACT_NONE);
  const size_t n = (size_t)cap_t16;
  P.d_srcs.alloc(sizeof(SrSrc) * n);
  P.d_dsts.alloc(sizeof(SrDst) * n);
  P.d_core_off.alloc(sizeof(long long) * (n + 1));
  P.stage_bytes = (sizeof(SrSrc) + sizeof(SrDst) + sizeof(long long)) * (n + 1);
  FFP_HIP(hipHostMalloc(&P.stage, P.stage_bytes, hipHostMallocDefault));
}

SrPlan::~SrPlan() {
  if (stage) (void)hipHostFree(stage);
}

SrPlan& SrEngine::plan_for(long long t16) {
  // smallest resident plan that holds the batch; else a new one at the next capacity bucket (least recently used one evicted)
  SrPlan* best = nullptr;
  plans_.for_each([&](SrPlan& p) { if (p.cap_t16 >= t16 && (!best || p.cap_t16 < best->cap_t16)) best = &p; });
  if (best) {
    plans_.touch(*best);
    return *best;
  }
  const int cap = capacity_bucket(t16);
  return plans_.get(cap, [&] {
    std::unique_ptr<SrPlan> p(new SrPlan());
    build_plan(*p, cap);
    ++plans_built;
    return p;
  });
}

void SrEngine::wait_done() {
  FFP_HIP(hipSetDevice(device_));
  FFP_HIP(hipStreamSynchronize(st_));
  if (pending_) {
    if (prof.enabled) prof.collect();
    FFP_HIP(hipEventElapsedTime(&last_ms, ev_[0], ev_[1]));
    pending_ = false;
  }
}

std::vector<SrTile> sr_tiles_checked(const std::vector<SrImage>& imgs, int scale, int tile, int tile_pad, int pre_pad) {
  std::vector<SrTile> tiles;
  switch (sr_tiles(imgs, scale, tile, tile_pad, pre_pad, tiles)) {
    case SR_TILES_OK: break;
    case SR_TILES_EMPTY_BATCH: fail(FFP_ERR_ARG, "enhance: empty batch");
    case SR_TILES_NEGATIVE_PAD: fail(FFP_ERR_ARG, "enhance: negative padding");
    case SR_TILES_EMPTY_IMAGE: fail(FFP_ERR_ARG, "enhance: empty image");
    case SR_TILES_PRE_PAD: fail(FFP_ERR_ARG, "enhance: pre_pad %d >= image size (reflect padding undefined)", pre_pad);
    case SR_TILES_TOO_SMALL: fail(FFP_ERR_ARG, "enhance: image too small for reflect padding");
    case SR_TILES_ODD_X2: fail(FFP_ERR_ARG, "enhance: x2 model needs even tile geometry (tile %d, pad %d)", tile, tile_pad);
  }
  return tiles;
}

void SrEngine::enhance_dev(const uint8_t* d_in, uint8_t* d_out, const std::vector<SrImage>& imgs, int tile, int tile_pad, int pre_pad, bool wait) {
  FFP_HIP(hipSetDevice(device_));
  if (pending_) wait_done();
  const int shuf = sr_shuffle(scale_);
  const std::vector<SrTile> tiles = sr_tiles_checked(imgs, scale_, tile, tile_pad, pre_pad);
  const int n = (int)tiles.size();
  const SrLevelSizes z = sr_level_sizes(tiles, scale_);
  // The plan depends on a CAPACITY, not on the sizes: a new multiset of crop sizes (every frame of a real stream) costs table
  // uploads only — no allocation, no tuning, no graph capture (the reference enhances arbitrary crops back to back,
  // utils/enhancer.py:344-391).
  SrPlan& P = plan_for(z.t16);
  P.Lb->assign(z.hs, z.ws, st_);
  P.L1->assign(z.h1, z.w1, st_);
  P.L2->assign(z.h2, z.w2, st_);
  const int cap = P.cap_t16;
  SrSrc* srcs = reinterpret_cast<SrSrc*>(P.stage);
  SrDst* dsts = reinterpret_cast<SrDst*>(srcs + cap);
  long long* coff = reinterpret_cast<long long*>(dsts + cap);
  sr_fill_descriptors(tiles, cap, srcs, dsts, coff);      // with padding entries: empty cores behind the last real one
  FFP_HIP(hipMemcpyAsync(P.d_srcs.p, srcs, sizeof(SrSrc) * n, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(P.d_dsts.p, dsts, sizeof(SrDst) * cap, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(P.d_core_off.p, coff, sizeof(long long) * (cap + 1), hipMemcpyHostToDevice, st_));
  FFP_HIP(hipEventRecord(ev_[0], st_));
  launch_sr_pre(d_in, P.d_srcs.as<SrSrc>(), P.input, shuf, st_);
  if (prof.enabled) prof.begin();
  P.execute(st_, &prof);
  launch_sr_post(P.out, P.d_dsts.as<SrDst>(), P.d_core_off.as<long long>(), P.L2->total_px, d_out, st_);
  FFP_HIP(hipEventRecord(ev_[1], st_));
  last_conv_flops = P.actual_conv_flops();
  last_graph = P.gexec != nullptr;
  last_conv_launches = P.conv_launches;
  pending_ = true;
  if (wait) wait_done();
}

}  // namespace ffp
