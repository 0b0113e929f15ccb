// yolo11.cpp — YOLO11{n,s,m,l}-pose as a plan of HIP launches over a ragged batch of crops.
//
// Graph: Ultralytics `yolo11-pose.yaml`; the reference reaches it through
// `self.model.predict(...)` at utils/yolo_wrapper.py:74-80. Every Concat is virtual: producers write straight into
// channel slices of the consumer's buffer; Upsample is a copy into such a slice.
#include "yolo11.hpp"

#include "conv_args.hpp"

#include <cmath>
#include <cstdlib>

namespace ffp {

namespace {
int make_div8(double x) { return (int)std::ceil(x / 8.0) * 8; }
}  // namespace

static DecodeArgs decode_args(const DetPlan& P, int nc, int nkpt);

void letterbox_geometry(int h, int w, int imgsz, int32_t* o) {
  // Ultralytics LetterBox(new_shape=imgsz, auto=True, scaleup=True, center=True, stride=32); Python round() is
  // round-half-even, as is nearbyint() under the default rounding mode.
  const double r = std::min((double)imgsz / h, (double)imgsz / w);
  const int new_w = (int)std::nearbyint(w * r), new_h = (int)std::nearbyint(h * r);
  double dw = (double)((imgsz - new_w) % 32), dh = (double)((imgsz - new_h) % 32);
  if (dw < 0) dw += 32;
  if (dh < 0) dh += 32;
  dw /= 2; dh /= 2;
  o[0] = new_w; o[1] = new_h;
  o[2] = (int)std::nearbyint(dh - 0.1); o[3] = (int)std::nearbyint(dh + 0.1);
  o[4] = (int)std::nearbyint(dw - 0.1); o[5] = (int)std::nearbyint(dw + 0.1);
}

DetEngine::DetEngine(const void* weights, size_t nbytes, int arch, int nc, int nkpt, int device, int precision) {
  FFP_CHECK(arch == 'n' || arch == 's' || arch == 'm' || arch == 'l', FFP_ERR_ARG,
            "arch '%c': the detector is built for YOLO11 scales n, s, m and l", arch > 32 && arch < 127 ? (char)arch : '?');
  FFP_CHECK(nc >= 1 && nc <= 256 && nkpt >= 0 && nkpt <= 32, FFP_ERR_ARG, "nc/nkpt out of range");
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F16 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "precision");
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, FFP_ERR_HIP, "no HIP device available (the detector has no CPU path)");
  FFP_CHECK(device >= 0 && device < ndev, FFP_ERR_ARG, "device %d of %d", device, ndev);
  device_ = device; nc_ = nc; nkpt_ = nkpt; scale_ = (char)arch; dt_ = precision == FFP_PREC_F16 ? F16 : F32;
  split_ = precision == FFP_PREC_F32X3;
  FFP_HIP(hipSetDevice(device_));
  st_ = create_engine_stream(sw().det_cu_mask);
  for (auto& e : ev_) FFP_HIP(hipEventCreate(&e));
  conv_kernels_init();
  WeightFile wf;
  wf.parse(weights, nbytes);
  for (const auto& kv : wf.t) {
    const std::string& nm = kv.first;
    if (nm.size() < 7 || nm.compare(nm.size() - 7, 7, ".weight") != 0) continue;
    const std::string base = nm.substr(0, nm.size() - 7);
    const HostTensor& w = kv.second;
    FFP_CHECK(w.dims.size() == 4 && w.dims[2] == w.dims[3], FFP_ERR_WEIGHTS, "%s: not a conv weight", nm.c_str());
    const int k = w.dims[2];
    const int groups = (w.dims[1] == 1 && w.dims[0] > 1 && k == 3) ? w.dims[0] : 1;
    pack_conv(convs_[base], wf, base, k, groups, dt_, st_, split_);   // input channels are zero-padded to a 16-byte multiple
  }
  FFP_CHECK(convs_.count("model.0.conv") && convs_.count("model.23.cv2.0.2"), FFP_ERR_WEIGHTS,
            "container does not hold YOLO11-pose tensors");
  FFP_CHECK(conv("model.23.cv3.0.2")->cout == nc_ && conv("model.23.cv4.0.2")->cout == 3 * nkpt_, FFP_ERR_WEIGHTS,
            "head shapes (%d classes, %d kpt values) differ from nc=%d nkpt=%d", conv("model.23.cv3.0.2")->cout,
            conv("model.23.cv4.0.2")->cout, nc_, nkpt_);
  if (split_ && nc_ <= 4 && conv("model.23.cv3.0.1.1.conv")->cout == 128)      // where a plan can fuse the class tower (build_plan)
    for (int l = 0; l < 3; ++l) {
      const std::string nm = "model.23.cv3." + std::to_string(l) + ".2";
      if (!wf.has(nm + ".weight") || !wf.has(nm + ".bias")) continue;
      const HostTensor& w = wf.get(nm + ".weight");
      const HostTensor& b = wf.get(nm + ".bias");
      DenseF32& d = dense_[nm];
      d.w.alloc(w.numel() * 4);
      d.b.alloc(b.numel() * 4);
      FFP_HIP(hipMemcpyAsync(d.w.p, w.data, w.numel() * 4, hipMemcpyHostToDevice, st_));
      FFP_HIP(hipMemcpyAsync(d.b.p, b.data, b.numel() * 4, hipMemcpyHostToDevice, st_));
      FFP_HIP(hipStreamSynchronize(st_));
      weight_bytes_ += d.w.n + d.b.n;
    }
  for (const auto& kv : convs_) weight_bytes_ += kv.second.w.n + kv.second.w16.n + kv.second.bias.n + kv.second.w_direct.n + kv.second.oscale.n;
}

DetEngine::~DetEngine() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  plans_.clear_nothrow();
  convs_.clear();
  for (auto& e : ev_) (void)hipEventDestroy(e);
  if (st_) (void)hipStreamDestroy(st_);
}

const PackedConv* DetEngine::conv(const std::string& name) const {
  auto it = convs_.find(name);
  FFP_CHECK(it != convs_.end(), FFP_ERR_WEIGHTS, "conv '%s' missing from the weight container", name.c_str());
  return &it->second;
}

void DetEngine::build_plan(DetPlan& P, const std::vector<int>& hs, const std::vector<int>& ws) {
  const int n = (int)hs.size();
  // scaled split: a max-|value| slot per (buffer, image), so that an item's bits do not depend on its batch mates (FFP_AMAX_PER_BUFFER=1:
  // round 2's one slot per buffer, A/B aid); the 1x1 kernels find a fragment's image through Level::frag_img, hence the 32-pixel alignment
  P.per_image_amax = split_ && !sw().amax_per_buffer;
  P.px_align = (P.per_image_amax || P.gate) ? 32 : 1;        // the gated 1x1 convs find a fragment's image the same way
  for (int l = 0; l < 6; ++l) {
    std::vector<int> h(n), w(n);
    for (int i = 0; i < n; ++i) { h[i] = hs[i] >> l; w[i] = ws[i] >> l; }
    P.L[l] = P.add_level(h, w, st_);
  }
  // [depth, width, max_channels] of yolo11-pose.yaml; scales m and l also force C3k inside every C3k2 (Ultralytics parse_model)
  const double width = scale_ == 'n' ? 0.25 : scale_ == 's' ? 0.50 : 1.00;
  const int max_ch = (scale_ == 'n' || scale_ == 's') ? 1024 : 512;
  const int reps = scale_ == 'l' ? 2 : 1;                  // max(round(2 * depth), 1): C3k2 and C2PSA repeats
  const bool force_c3k = scale_ == 'm' || scale_ == 'l';
  auto ch = [&](int c) { return make_div8(std::min(c, max_ch) * width); };
  const int c64 = ch(64), c128 = ch(128), c256 = ch(256), c512 = ch(512), c1024 = ch(1024);
  const DType T = dt_;

  const bool fold_up = !sw().no_upfold;
  auto cv = [&](const std::string& name, const TView& in, const TView& out, int stride, int act, const TView* res = nullptr, const TView* up2 = nullptr,
                const int* gate = nullptr) {
    ConvOp o;
    o.pc = conv(name); o.in = in; o.out = out; o.stride = stride; o.act = act; o.gate = gate;
    const double* share = nullptr;
    for (int l = 0; l < 3; ++l) if (gate && out.lvl == P.L[3 + l]) share = &P.gate_share[l];
    if (res) { o.has_res1 = true; o.res1 = *res; o.s1 = 1.f; }
    if (up2) { o.has_up2 = true; o.up2 = *up2; o.up2_c = up2->C; o.up2_map = in.lvl->up2_map(up2->lvl, st_); }
    FFP_CHECK(o.pc->cin == in.C && o.pc->cout == out.C, FFP_ERR_WEIGHTS, "%s: weights are %d->%d, graph expects %d->%d",
              name.c_str(), o.pc->cin, o.pc->cout, in.C, out.C);
    P.add_conv(o);
    P.steps.back().share = share;
  };
  auto dw = [&](const std::string& name, const TView& in, const TView& out, int act) {
    DwConvOp o;
    o.pc = conv(name); o.in = in; o.out = out; o.act = act;
    P.add([o](hipStream_t s) { launch_dwconv(o, s); });
  };
  // Bottleneck(c, c, shortcut, k=(3,3)): out = x + cv2(cv1(x))
  auto bottleneck = [&](const std::string& p, const TView& x, const TView& out, int chid) {
    Plan::Scope tmp(P);                                 // t
    TView t = P.alloc(x.lvl, chid, T);
    cv(p + ".cv1.conv", x, t, 1, ACT_SILU);
    cv(p + ".cv2.conv", t, out, 1, ACT_SILU, &x);
  };
  // C3k(c, c, n=2) on view b into view mo: cv3(cat(m(cv1(b)), cv2(b)))
  auto c3k = [&](const std::string& p, const TView& b, const TView& mo, int c) {
    const int c_ = c / 2;
    Plan::Scope tmp(P);                                 // cat2, a0, a1 (released at the join when the side lane is on)
    TView cat2 = P.alloc(b.lvl, 2 * c_, T);
    TView a0 = P.alloc(b.lvl, c_, T), a1 = P.alloc(b.lvl, c_, T);
    const int side = 10;                               // C3k's second branch (one 1x1 conv over b) runs beside the bottleneck chain
    if (P.lane_mode() == 1) P.fork(side);
    P.cur_lane = P.lane_mode() == 1 ? side : 0;
    cv(p + ".cv2.conv", b, cat2.slice(c_, c_), 1, ACT_SILU);
    P.cur_lane = 0;
    cv(p + ".cv1.conv", b, a0, 1, ACT_SILU);
    bottleneck(p + ".m.0", a0, a1, c_);
    bottleneck(p + ".m.1", a1, cat2.slice(0, c_), c_);
    if (P.lane_mode() == 1) P.join(side);              // each C3k joins its side lane before the next one forks it again
    cv(p + ".cv3.conv", cat2, mo, 1, ACT_SILU);
  };
  // C3k2(c1, c2, n, c3k, e): cat = [a | b | m.0(b) | m.1(m.0(b)) ...]; out = cv2(cat)
  auto c3k2 = [&](const std::string& p, const TView& in, const TView& out, int c2, bool use_c3k, double e, const TView* up2 = nullptr) {
    const int c = (int)(c2 * e);
    use_c3k = use_c3k || force_c3k;
    Plan::Scope tmp(P);                                 // cat
    TView cat = P.alloc(in.lvl, (2 + reps) * c, T);
    cv(p + ".cv1.conv", in, cat.slice(0, 2 * c), 1, ACT_SILU, nullptr, up2);
    for (int i = 0; i < reps; ++i) {
      const TView b = cat.slice((1 + i) * c, c), mo = cat.slice((2 + i) * c, c);
      const std::string pm = p + ".m." + std::to_string(i);
      if (!use_c3k) bottleneck(pm, b, mo, c / 2);
      else c3k(pm, b, mo, c);
    }
    cv(p + ".cv2.conv", cat, out, 1, ACT_SILU);
  };

  // ---- buffers that realise the Concat layers --------------------------------------------------------------------
  const int cin0 = T == F16 ? 8 : 4;
  P.input = TView{};
  P.input.dt = T; P.input.cs = cin0; P.input.C = cin0; P.input.lvl = P.L[0];     // storage only if the stem is not fused (below)
  // Each is allocated where its first slice is written and released behind the C3k2 that reads it whole: the skip tensors x4, x6,
  // x10 and x13 live in them from the backbone to the neck. Everything else is released behind its last reader (Plan::release,
  // Plan::Scope for a block's temporaries), so a later tensor may reuse its bytes. Never released: P.input, the tensor the stem launch
  // writes before execute() (x1, or x0 on the two-kernel path: the tuner's timing launches run after that launch and write every
  // conv's output) and P.head[l], which decode reads after the plan.

  // ---- backbone --------------------------------------------------------------------------------------------------------
  TView x0 = P.alloc_virtual(P.L[1], c64, T);      // stored only if a kernel reads it (not when model.1's loader computes it)
  TView x1 = P.alloc(P.L[2], c128, T);
  {   // stem: fused with the letterbox when the direct image-input kernel applies (always, for 3-channel frames)
    ConvOp o, m1;
    o.pc = conv("model.0.conv"); o.in = P.input; o.out = x0; o.stride = 2; o.act = ACT_SILU;
    FFP_CHECK(o.pc->cin == cin0 && o.pc->cout == c64, FFP_ERR_WEIGHTS, "model.0.conv: weights are %d->%d, graph expects %d->%d", o.pc->cin,
              o.pc->cout, cin0, c64);
    m1.pc = conv("model.1.conv"); m1.in = x0; m1.out = x1; m1.stride = 2; m1.act = ACT_SILU;
    FFP_CHECK(m1.pc->cin == x0.C && m1.pc->cout == x1.C, FFP_ERR_WEIGHTS, "model.1.conv: weights are %d->%d, graph expects %d->%d", m1.pc->cin,
              m1.pc->cout, x0.C, x1.C);
    const bool direct = conv_direct_eligible(o) && !sw().no_fused_stem;
    // the image-input conv's output bound is known from the weights alone (inputs in [0, 1], |SiLU(v)| <= max(|v|, 0.279)), so the
    // first MFMA conv finds its input's exponent without a pass over the data
    P.set_amax_bound(x0, std::max(o.pc->out_bound, 0.3f));
    // YOLO11m/l (64 stem channels) keep the two-kernel path: a four-chunk form of the fused loader lost to it at imgsz 1024 and tied at
    // 512 (profiles/r05_stem_ab_yolo11m.txt)
    if (direct && stem_conv_eligible(o, m1)) {
      // fp32-split YOLO11s: model.0 runs inside model.1's loader on the matrix cores; x0 is never stored
      o.flops = conv_flops_of(*o.pc, x0.lvl->actual_px());
      m1.flops = conv_flops_of(*m1.pc, x1.lvl->actual_px());
      P.stem = o; P.fused_stem = true;
      P.stemconv = m1; P.fused_stem_conv = true;
      P.stemconv_variant = "f32x3_k3s2_stem_fused";
      P.conv_flops += o.flops + m1.flops; P.conv_launches += 1;
      P.reset_outside = true;                          // the fused launch raises x1's max-|value| slot before execute()
      for (int f = 0; f < 2; ++f) stem_conv_pack(o, f, P.stem_w[f], st_);
    } else {
      P.materialize(x0);
      o.out = x0; m1.in = x0;
      if (direct) {
        o.flops = conv_flops_of(*o.pc, x0.lvl->actual_px());
        P.stem = o; P.fused_stem = true;
        P.conv_flops += o.flops; P.conv_launches += 1;
      } else {
        P.input = P.alloc(P.L[0], cin0, T);
        P.set_amax_bound(P.input, 1.0f);                 // pixels / 255
        cv("model.0.conv", P.input, x0, 2, ACT_SILU);   // reads the 4/8-channel padded image (weights zero padded at pack)
      }
      P.add_conv(m1);
    }
  }
  TView x2 = P.alloc(P.L[2], c256, T);
  c3k2("model.2", x1, x2, c256, false, 0.25);
  if (!P.fused_stem_conv) P.release(x1);
  TView x3 = P.alloc(P.L[3], c256, T);
  cv("model.3.conv", x2, x3, 2, ACT_SILU);
  P.release(x2);
  TView cat15 = P.alloc(P.L[3], c512 + c512, T);    // [up(x13) | x4]
  const TView x4 = cat15.slice(c512, c512);
  c3k2("model.4", x3, x4, c512, false, 0.25);
  P.release(x3);
  TView x5 = P.alloc(P.L[4], c512, T);
  cv("model.5.conv", x4, x5, 2, ACT_SILU);
  TView cat12 = P.alloc(P.L[4], c1024 + c512, T);   // [up(x10) | x6]
  const TView x6 = cat12.slice(c1024, c512);
  c3k2("model.6", x5, x6, c512, true, 0.5);
  P.release(x5);
  TView x7 = P.alloc(P.L[5], c1024, T);
  cv("model.7.conv", x6, x7, 2, ACT_SILU);
  TView x8 = P.alloc(P.L[5], c1024, T);
  c3k2("model.8", x7, x8, c1024, true, 0.5);
  P.release(x7);
  TView cat21 = P.alloc(P.L[5], c512 + c1024, T);   // [conv20(x19) | x10]
  const TView x10 = cat21.slice(c512, c1024);
  // SPPF
  {
    const int c_ = c1024 / 2;
    TView cat9 = P.alloc(P.L[5], 4 * c_, T);
    cv("model.9.cv1.conv", x8, cat9.slice(0, c_), 1, ACT_SILU);
    P.release(x8);
    const TView y0 = cat9.slice(0, c_), y1 = cat9.slice(c_, c_), y2 = cat9.slice(2 * c_, c_), y3 = cat9.slice(3 * c_, c_);
    P.add([y0, y1, y2, y3](hipStream_t s) { launch_sppf_pool(y0, y1, y2, y3, s); });
    TView x9 = P.alloc(P.L[5], c1024, T);
    cv("model.9.cv2.conv", cat9, x9, 1, ACT_SILU);
    P.release(cat9);
    // C2PSA
    const int h = c1024 / 2, nh = h / 64, hd = h / nh, kd = hd / 2;
    TView pb = P.alloc(P.L[5], 2 * h, T);
    cv("model.10.cv1.conv", x9, pb, 1, ACT_SILU);
    P.release(x9);
    const TView b = pb.slice(h, h);
    for (int i = 0; i < reps; ++i) {                  // PSABlocks m.0, m.1, ... each in place on b
      const std::string pm = "model.10.m." + std::to_string(i);
      Plan::Scope tmp(P);                             // qkv, ao, xa, b2, f1
      TView qkv = P.alloc(P.L[5], nh * (2 * kd + hd), T);
      cv(pm + ".attn.qkv.conv", b, qkv, 1, ACT_NONE);
      TView ao = P.alloc(P.L[5], h, T);
      P.add([qkv, ao, nh, kd, hd](hipStream_t s) { launch_psa_attention(qkv, ao, nh, kd, hd, s); });
      TView xa = P.alloc(P.L[5], h, T);
      {
        DwConvOp o;
        o.pc = conv(pm + ".attn.pe.conv");
        o.in = qkv; o.in.C = h; o.out = xa; o.act = ACT_NONE;
        o.grp = hd; o.grp_stride = 2 * kd + hd; o.grp_off = 2 * kd;
        o.has_res = true; o.res = ao;
        P.add([o](hipStream_t s) { launch_dwconv(o, s); });
      }
      TView b2 = P.alloc(P.L[5], h, T);
      cv(pm + ".attn.proj.conv", xa, b2, 1, ACT_NONE, &b);
      TView f1 = P.alloc(P.L[5], 2 * h, T);
      cv(pm + ".ffn.0.conv", b2, f1, 1, ACT_SILU);
      cv(pm + ".ffn.1.conv", f1, b, 1, ACT_NONE, &b2);
    }
    cv("model.10.cv2.conv", pb, x10, 1, ACT_SILU);
    P.release(pb);
  }
  // ---- neck ------------------------------------------------------------------------------------------------------------
  // Upsample + Concat feed a 1x1 conv only: its loader reads the coarse tensor through the x2 pixel map (no upsampled copy)
  const bool fold12 = fold_up && c1024 % 64 == 0, fold15 = fold_up && c512 % 64 == 0;
  if (!fold12) {
    const TView up = cat12.slice(0, c1024);
    P.add([x10, up](hipStream_t s) { launch_upsample2x(x10, up, s); launch_amax_max(up.amax, x10.amax, s, up.amax_n); });
  }
  TView cat18 = P.alloc(P.L[4], c256 + c512, T);    // [conv17(x16) | x13]
  const TView x13 = cat18.slice(c256, c512);
  c3k2("model.13", cat12, x13, c512, false, 0.5, fold12 ? &x10 : nullptr);
  P.release(cat12);
  if (!fold15) {
    const TView up = cat15.slice(0, c512);
    P.add([x13, up](hipStream_t s) { launch_upsample2x(x13, up, s); launch_amax_max(up.amax, x13.amax, s, up.amax_n); });
  }
  const int chs[3] = {c256, c512, c1024};
  const int nk = 3 * nkpt_;
  const int no = 64 + nc_ + nk;
  const int head_cs = (no + 3) / 4 * 4;
  const int c2 = std::max(std::max(16, chs[0] / 4), 64);
  const int c3 = std::max(chs[0], std::min(nc_, 100));
  const int c4 = std::max(chs[0] / 4, nk);
  // One head level = three independent towers (box, class, keypoints) over one feature map. decode reads an anchor's box values only when
  // its best class score passes conf, and NMS reads keypoints only of boxes it keeps: an item (slice) without any such anchor gets nothing
  // out of its box and keypoint towers. So the class tower of a level is forked as soon as its map exists, the gate (det_post.hip) marks
  // the items with a passing anchor once all three class towers are done, and the 3x3 convs of the box and keypoint towers of all levels
  // then walk tile tables that hold the active items only (ConvOp::gate). Exact: with per-image exponent slots an item's bits do not
  // depend on its batch mates. Each tower is a lane of its own where lanes are on.
  const std::string hp = "model.23";
  const int lm = P.lane_mode();
  auto tower_lane = [&](int l, int k) { return lm == 1 ? 3 * l + k : lm == 2 ? 3 * l + 1 : (lm == 3 && l == 0) ? 1 : 0; };
  const int* gate = nullptr;
  if (P.gate) {
    P.d_active.alloc(sizeof(int) * n);
    P.d_conf.alloc(sizeof(float));
    gate = P.d_active.as<int>();
    for (int l = 3; l < 6; ++l) P.L[l]->gate_compact = &launch_gate_compact;
  }
  auto class_tower = [&](int l, const TView& x) {
    Level* lv = P.L[3 + l];
    const std::string ls = std::to_string(l);
    P.head[l] = P.alloc(lv, head_cs, F32);              // never released: decode reads it after the plan
    P.fork(tower_lane(l, 2));
    // Two launches instead of five (conv_dwpw.hip): each depthwise conv runs inside the loader of the 1x1 conv behind it, and with nc <= 4 the closing 1x1
    // inside the second one's epilogue; d1, d2 and e2 are never stored. A never-stored tensor has no max-|value| slot: its split takes its exponent from a
    // per-image bound (dw_bound.hpp). FFP_CLS_FUSE=0: the five ops. Read per plan, so that one process can build both.
    const bool cls_fuse = sw_live().cls_fuse;
    const std::string n0 = hp + ".cv3." + ls + ".0", n1 = hp + ".cv3." + ls + ".1", n2 = hp + ".cv3." + ls + ".2";
    // e1 and e2 start without storage: the fused ops are described first and the kernel is asked (its layout, and that x, e1 and the head record each fit
    // one buffer resource: a level past 2 GiB, e.g. 5-frame groups at imgsz 1024, does not); a level it cannot run gets the five ops below, unchanged
    TView e1 = P.alloc_virtual(lv, c3, T), e2 = P.alloc_virtual(lv, c3, T);
    bool fused = false;
    if (split_ && P.per_image_amax && cls_fuse && chs[l] % 16 == 0 && c3 == 128) {
      const bool fin = dense_.count(n2) != 0;
      ConvOp t1, t2;
      t1.pc = conv(n0 + ".1.conv"); t1.dw = conv(n0 + ".0.conv"); t1.dw_act = ACT_SILU;
      t1.in = x; t1.out = e1; t1.act = ACT_SILU; t1.label = n0;
      t2.pc = conv(n1 + ".1.conv"); t2.dw = conv(n1 + ".0.conv"); t2.dw_act = ACT_SILU;
      t2.in = e1; t2.out = e2; t2.act = ACT_SILU; t2.label = fin ? n1 + "+2" : n1;
      if (fin) { t2.fin = conv(n2); t2.fin_w = &dense_.at(n2); t2.fin_out = P.head[l].slice(64, nc_); }
      if (conv_dwpw_eligible(t1, false) && conv_dwpw_eligible(t2, false)) {
        fused = true;
        P.materialize(e1);
        if (!fin) P.materialize(e2);
        t1.out = e1; t2.in = e1; t2.out = e2;
        P.cur_lane = tower_lane(l, 2);
        P.add_conv(t1);
        P.add_conv(t2);
        if (!fin) cv(n2, e2, P.head[l].slice(64, nc_), 1, ACT_NONE);
        P.release(e1);
        if (!fin) P.release(e2);
        P.cur_lane = 0;
      }
    }
    if (fused) return;
    TView d1 = P.alloc(lv, chs[l], T);
    P.materialize(e1);
    TView d2 = P.alloc(lv, c3, T);
    P.materialize(e2);
    P.cur_lane = tower_lane(l, 2);
    dw(hp + ".cv3." + ls + ".0.0.conv", x, d1, ACT_SILU);
    cv(hp + ".cv3." + ls + ".0.1.conv", d1, e1, 1, ACT_SILU);
    dw(hp + ".cv3." + ls + ".1.0.conv", e1, d2, ACT_SILU);
    cv(hp + ".cv3." + ls + ".1.1.conv", d2, e2, 1, ACT_SILU);
    cv(hp + ".cv3." + ls + ".2", e2, P.head[l].slice(64, nc_), 1, ACT_NONE);
    P.release(d1);
    P.release(e1);
    P.release(d2);
    P.release(e2);
    P.cur_lane = 0;
  };
  // the 3x3 convs walk the gated tile tables; the closing 1x1 leaves out the 32-pixel fragments of inactive items, so it reads nothing that
  // was not written in this run. The head records of a skipped item keep whatever an earlier run left there; nobody reads them.
  auto box_kpt_towers = [&](int l, const TView& x) {
    Level* lv = P.L[3 + l];
    const std::string ls = std::to_string(l);
    TView t1 = P.alloc(lv, c2, T), t2 = P.alloc(lv, c2, T);
    P.cur_lane = tower_lane(l, 1);
    cv(hp + ".cv2." + ls + ".0.conv", x, t1, 1, ACT_SILU, nullptr, nullptr, gate);
    cv(hp + ".cv2." + ls + ".1.conv", t1, t2, 1, ACT_SILU, nullptr, nullptr, gate);
    cv(hp + ".cv2." + ls + ".2", t2, P.head[l].slice(0, 64), 1, ACT_NONE, nullptr, nullptr, gate);
    P.release(t1);
    P.release(t2);
    if (nk > 0) {
      TView k1 = P.alloc(lv, c4, T), k2 = P.alloc(lv, c4, T);
      P.cur_lane = tower_lane(l, 3);
      cv(hp + ".cv4." + ls + ".0.conv", x, k1, 1, ACT_SILU, nullptr, nullptr, gate);
      cv(hp + ".cv4." + ls + ".1.conv", k1, k2, 1, ACT_SILU, nullptr, nullptr, gate);
      cv(hp + ".cv4." + ls + ".2", k2, P.head[l].slice(64 + nc_, nk), 1, ACT_NONE, nullptr, nullptr, gate);
      P.release(k1);
      P.release(k2);
    }
    P.cur_lane = 0;
  };

  TView x16 = P.alloc(P.L[3], c256, T);
  c3k2("model.16", cat15, x16, c256, false, 0.5, fold15 ? &x13 : nullptr);
  P.release(cat15);
  class_tower(0, x16);
  cv("model.17.conv", x16, cat18.slice(0, c256), 2, ACT_SILU);
  TView x19 = P.alloc(P.L[4], c512, T);
  c3k2("model.19", cat18, x19, c512, false, 0.5);
  P.release(cat18);
  class_tower(1, x19);
  cv("model.20.conv", x19, cat21.slice(0, c512), 2, ACT_SILU);
  TView x22 = P.alloc(P.L[5], c1024, T);
  c3k2("model.22", cat21, x22, c1024, true, 0.5);
  P.release(cat21);
  class_tower(2, x22);
  for (int l = 0; l < 3; ++l) P.join(tower_lane(l, 2));
  if (gate) {
    DetPlan* pp = &P;
    const int nc = nc_, nkpt = nkpt_;
    P.add([pp, nc, nkpt](hipStream_t s) {
      launch_det_gate(decode_args(*pp, nc, nkpt), pp->d_conf.as<float>(), pp->d_active.as<int>(), s);
      Level::compact_gated(&pp->L[3], 3, s);      // tables the first run's launchers created (they compact what they create): one scan and one scatter for all of them
    });
  }
  // x16, x19 and x22 live until their towers have been issued
  const TView* xs[3] = {&x16, &x19, &x22};
  for (int l = 0; l < 3; ++l)
    for (int k = 1; k <= 3; k += 2) if (lm == 1 || k == 1) P.fork(tower_lane(l, k));
  for (int l = 0; l < 3; ++l) box_kpt_towers(l, *xs[l]);
  P.release(x16);
  P.release(x19);
  P.release(x22);

  // ---- Pose head: per level one fp32 record [64 DFL | nc | 3*nkpt] per pixel ---------------------------------------------
  for (int l = 0; l < 3; ++l)                       // lane 0 continues (decode, NMS) after every tower of every level
    for (int k = 1; k <= 3; k += 2) if (lm == 1 || k == 1) P.join(tower_lane(l, k));

  P.add_amax_reset(st_);      // first step of every run: max-|value| slots back to their static bounds / zero

  // ---- anchors -----------------------------------------------------------------------------------------------------------
  P.anchor_off.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    int a = 0;
    for (int l = 3; l < 6; ++l) a += P.L[l]->h[i] * P.L[l]->w[i];
    P.anchor_off[i + 1] = P.anchor_off[i] + a;
  }
  P.total_anchors = P.anchor_off[n];
  P.d_anchor_off.alloc(sizeof(int) * (n + 1));
  FFP_HIP(hipMemcpyAsync(P.d_anchor_off.p, P.anchor_off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, st_));
  FFP_HIP(hipStreamSynchronize(st_));
  P.d_boxes.alloc(sizeof(float4) * (size_t)P.total_anchors);
  P.d_scores.alloc(sizeof(float) * (size_t)P.total_anchors);
  P.d_classes.alloc(sizeof(int) * (size_t)P.total_anchors);
  P.d_cand.alloc(sizeof(int) * (size_t)P.total_anchors);
  P.d_cscore.alloc(sizeof(float) * (size_t)P.total_anchors);
  P.d_lb.alloc(sizeof(LetterboxImg) * n);
  P.d_imgs.alloc(sizeof(DetImg) * n);
}

std::vector<TileGeom> det_tile_geometry(int H, int W, const int32_t* tiles, int n_tiles, int imgsz) {
  FFP_CHECK(H > 0 && W > 0 && n_tiles > 0 && tiles, FFP_ERR_ARG, "empty frame or tile list");
  std::vector<TileGeom> g(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    const int x0 = tiles[4 * i], y0 = tiles[4 * i + 1], x1 = tiles[4 * i + 2], y1 = tiles[4 * i + 3];
    FFP_CHECK(x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x1 > x0 && y1 > y0, FFP_ERR_ARG, "tile %d [%d,%d,%d,%d] outside %dx%d frame",
              i, x0, y0, x1, y1, W, H);
    const int sw = x1 - x0, sh = y1 - y0;
    int sz = imgsz;
    if (sz <= 0) sz = (std::max(tiles[2] - tiles[0], tiles[3] - tiles[1]) + 31) / 32 * 32;
    FFP_CHECK(sz % 32 == 0 && sz >= 32 && sz <= 4096, FFP_ERR_ARG, "imgsz %d must be a multiple of 32 in [32,4096]", sz);
    int32_t lg[6];
    letterbox_geometry(sh, sw, sz, lg);
    FFP_CHECK(lg[0] > 0 && lg[1] > 0, FFP_ERR_ARG, "tile %d (%dx%d) resizes to %dx%d at imgsz %d (cv2.resize would raise)", i, sw, sh, lg[0], lg[1], sz);
    TileGeom& t = g[i];
    t.lb.x0 = x0; t.lb.y0 = y0; t.lb.sw = sw; t.lb.sh = sh;
    t.lb.new_w = lg[0]; t.lb.new_h = lg[1]; t.lb.top = lg[2]; t.lb.left = lg[4];
    t.lb.net_h = lg[1] + lg[2] + lg[3]; t.lb.net_w = lg[0] + lg[4] + lg[5];
    FFP_CHECK(t.lb.net_h % 32 == 0 && t.lb.net_w % 32 == 0, FFP_ERR_STATE, "letterboxed size %dx%d not a multiple of 32", t.lb.net_w, t.lb.net_h);
    // ultralytics scale_boxes: gain = min(h1/h0, w1/w0); pad = round((w1 - w0*gain)/2 - 0.1), ...
    const double gain = std::min((double)t.lb.net_h / sh, (double)t.lb.net_w / sw);
    t.di.gain = (float)gain;
    t.di.pad_x = (float)std::nearbyint((t.lb.net_w - sw * gain) / 2 - 0.1);
    t.di.pad_y = (float)std::nearbyint((t.lb.net_h - sh * gain) / 2 - 0.1);
    t.di.sw = sw; t.di.sh = sh; t.di.x0 = x0; t.di.y0 = y0;
  }
  return g;
}

DetPlan* DetEngine::plan_for(const std::vector<TileGeom>& g) {
  std::vector<int> key;
  key.reserve(g.size() * 2);
  for (const TileGeom& t : g) { key.push_back(t.lb.net_h); key.push_back(t.lb.net_w); }
  // bounded by count and by bytes (a caller alternating between image_size 512 and 1024, or between group sizes, keeps what it uses)
  return &plans_.get(key, [&] {
    std::unique_ptr<DetPlan> p(new DetPlan());
    p->lanes = lanes_;
    p->reuse = reuse_;
    p->gate = gate_;
    std::vector<int> hs, ws;
    for (const TileGeom& t : g) { hs.push_back(t.lb.net_h); ws.push_back(t.lb.net_w); }
    build_plan(*p, hs, ws);
    return p;
  });
}

void DetEngine::mem_detail(size_t* activation, size_t* no_reuse, size_t* peak_live) const {
  *activation = *no_reuse = *peak_live = 0;
  plans_.for_each([&](const DetPlan& p) {
    *activation += p.activation_bytes();
    *no_reuse += p.no_reuse_bytes();
    *peak_live += p.peak_live_bytes();
  });
}

void DetEngine::set_gate(bool on) {
  if (on == gate_) return;
  drop_plans();
  gate_ = on;
}

// the gate's verdict of the run just issued, on its way to the host: valid once the caller has waited for the stream
void DetEngine::fetch_active(DetPlan* P, int n_tiles) {
  last_items_ = n_tiles;
  last_gated_ = P->gate;
  if (!P->gate) return;
  h_active_.ensure(sizeof(int) * n_tiles);
  FFP_HIP(hipMemcpyAsync(h_active_.p, P->d_active.p, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st_));
}

// after the stream has drained: per head level, the share of its pixels that belongs to active items
void DetEngine::set_shares(DetPlan* P) const {
  if (!P->gate) return;
  const int* act = static_cast<const int*>(h_active_.p);
  for (int l = 0; l < 3; ++l) {
    const Level& lv = *P->L[3 + l];
    double on = 0, all = 0;
    for (int i = 0; i < lv.n; ++i) { const double px = (double)lv.h[i] * lv.w[i]; all += px; if (act[i]) on += px; }
    P->gate_share[l] = all > 0 ? on / all : 1.0;
  }
}

void DetEngine::last_active(int* active, int* items) const {
  *items = last_items_;
  *active = last_items_;
  if (!last_gated_) return;
  *active = 0;
  for (int i = 0; i < last_items_; ++i) *active += static_cast<const int*>(h_active_.p)[i] != 0;
}

DetPlan* DetEngine::prepare(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf) {
  FFP_HIP(hipSetDevice(device_));
  geom_last_ = det_tile_geometry(H, W, tiles, n_tiles, imgsz);
  DetPlan* P = plan_for(geom_last_);
  std::vector<LetterboxImg> lb(n_tiles);
  std::vector<DetImg> di(n_tiles);
  for (int i = 0; i < n_tiles; ++i) { lb[i] = geom_last_[i].lb; di[i] = geom_last_[i].di; }
  FFP_HIP(hipMemcpyAsync(P->d_lb.p, lb.data(), sizeof(LetterboxImg) * n_tiles, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(P->d_imgs.p, di.data(), sizeof(DetImg) * n_tiles, hipMemcpyHostToDevice, st_));
  // the gate's threshold: uploaded here, outside the captured steps, so that a replayed graph honours the conf of every call
  if (P->gate) FFP_HIP(hipMemcpyAsync(P->d_conf.p, &conf, sizeof(float), hipMemcpyHostToDevice, st_));
  FFP_HIP(hipStreamSynchronize(st_));   // lb/di are stack vectors
  FFP_HIP(hipEventRecord(ev_[0], st_));
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  if (prof.enabled) prof.begin();
  if (P->fused_stem_conv) {
    if (!P->tuned) P->tune(st_);      // the tuner's timing launches raise max-|value| slots from stale buffers: before the reset, never after it
    P->reset_fn(st_);
    const int slot = prof.enabled ? prof.open(st_) : -1;
    launch_stem_conv(d_frame, H, W, P->d_lb, P->stem_w[flip], P->stem, P->stemconv, st_);
    if (slot >= 0) prof.close(slot, st_, P->stemconv_variant, P->stem.flops + P->stemconv.flops, "model.0.conv+model.1.conv");
  } else if (P->fused_stem) {
    launch_stem_from_frame(d_frame, H, W, flip, P->d_lb, P->stem, st_);
  } else {
    launch_letterbox(d_frame, H, W, flip, P->d_lb, P->input, st_);
  }
  FFP_HIP(hipEventRecord(ev_[1], st_));
  P->execute(st_, &prof);
  FFP_HIP(hipEventRecord(ev_[2], st_));
  last_conv_flops = P->conv_flops;
  last_conv_launches = P->conv_launches;
  last_graph_state = P->graph_state();
  return P;
}

static DecodeArgs decode_args(const DetPlan& P, int nc, int nkpt) {
  DecodeArgs a{};
  for (int l = 0; l < 3; ++l) {
    a.head[l] = (const float*)P.head[l].ptr;
    a.tab[l] = P.L[3 + l]->d_tab.as<int4>();
  }
  a.head_cs = P.head[0].cs; a.nc = nc; a.nkpt = nkpt; a.n_img = P.L[0]->n;
  a.anchor_off = P.d_anchor_off.as<int>(); a.total_anchors = P.total_anchors;
  return a;
}

void DetEngine::infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                                float conf, float iou, int max_det, int round_boxes, float* d_out_dets, int32_t* d_out_counts) {
  FFP_CHECK(max_det >= 1 && max_det <= 1024, FFP_ERR_ARG, "max_det %d outside [1,1024]", max_det);
  DetPlan* P = prepare(d_frame, H, W, chan_order, tiles, n_tiles, imgsz, conf);
  const DecodeArgs a = decode_args(*P, nc_, nkpt_);
  launch_decode(a, conf, P->d_boxes.as<float4>(), P->d_scores.as<float>(), P->d_classes.as<int>(), st_);
  launch_nms(a, P->d_boxes.as<float4>(), P->d_scores.as<float>(), P->d_classes.as<int>(), P->d_cand.as<int>(),
             P->d_cscore.as<float>(), P->d_imgs.as<DetImg>(), iou, max_det, round_boxes, det_stride(), d_out_dets, d_out_counts, st_);
  FFP_HIP(hipEventRecord(ev_[3], st_));
  fetch_active(P, n_tiles);
  FFP_HIP(hipStreamSynchronize(st_));
  if (prof.enabled) { set_shares(P); prof.collect(); }
  FFP_HIP(hipEventElapsedTime(&last_ms[1], ev_[0], ev_[1]));
  FFP_HIP(hipEventElapsedTime(&last_ms[2], ev_[1], ev_[2]));
  FFP_HIP(hipEventElapsedTime(&last_ms[3], ev_[2], ev_[3]));
  FFP_HIP(hipEventElapsedTime(&last_ms[0], ev_[0], ev_[3]));
  last_ms[4] = 0.f;
}

void DetEngine::forward_raw(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz,
                            float* out_raw, size_t out_cap, int32_t* out_anchor_counts) {
  DetPlan* P = prepare(d_frame, H, W, chan_order, tiles, n_tiles, imgsz, -1.f);      // the raw output needs every anchor: sigmoid > -1, every item active
  const DecodeArgs a = decode_args(*P, nc_, nkpt_);
  const int no = 4 + nc_ + 3 * nkpt_;
  std::vector<long long> off(n_tiles);
  long long tot = 0;
  for (int i = 0; i < n_tiles; ++i) {
    off[i] = tot;
    const int A = P->anchor_off[i + 1] - P->anchor_off[i];
    out_anchor_counts[i] = A;
    tot += (long long)no * A;
  }
  FFP_CHECK((size_t)tot <= out_cap, FFP_ERR_ARG, "forward_raw: output needs %lld floats, capacity %zu", tot, out_cap);
  DevBuf d_off(sizeof(long long) * n_tiles), d_out(sizeof(float) * (size_t)tot);
  FFP_HIP(hipMemcpyAsync(d_off.p, off.data(), sizeof(long long) * n_tiles, hipMemcpyHostToDevice, st_));
  launch_decode_raw(a, d_out.as<float>(), d_off.as<long long>(), st_);
  FFP_HIP(hipMemcpyAsync(out_raw, d_out.p, sizeof(float) * (size_t)tot, hipMemcpyDeviceToHost, st_));
  fetch_active(P, n_tiles);
  FFP_HIP(hipStreamSynchronize(st_));
  if (prof.enabled) { set_shares(P); prof.collect(); }
}

void DetEngine::truncate_shift_dev(float* d_dets, const int32_t* d_counts, int n_tiles, int max_det, int H, int W) {
  FFP_CHECK((int)geom_last_.size() == n_tiles, FFP_ERR_STATE, "truncate_shift: no matching infer call");
  DetPlan* P = plan_for(geom_last_);
  launch_truncate_shift(d_dets, d_counts, P->d_imgs.as<DetImg>(), n_tiles, max_det, det_stride(), nkpt_, H, W, st_);
}

void DetEngine::merge_dev(const float* d_dets, const int32_t* d_counts, int n_slices, int max_det, int type, int metric, double thr,
                          int class_agnostic, float* d_out, int32_t* d_out_src, int cap, int32_t* d_out_n) {
  FFP_HIP(hipSetDevice(device_));
  const int stride = det_stride();
  FFP_HIP(hipEventRecord(ev_[4], st_));
  tail.compact(d_dets, d_counts, n_slices, max_det, stride, st_);
  // always the merge, over the grid bound: no read back of the row count between the two (the benchmarked ffp_merge_dev path)
  tail.merge(MergeRule::Always, n_slices * max_det, type, metric, thr, class_agnostic, d_out, d_out_src, d_out_n, cap, st_);
  FFP_HIP(hipEventRecord(ev_[5], st_));
  FFP_HIP(hipStreamSynchronize(st_));
  FFP_HIP(hipEventElapsedTime(&last_ms[4], ev_[4], ev_[5]));
}

}  // namespace ffp
