// rtdetr.cpp — Ultralytics RT-DETR-l (models/rtdetr, nn/modules/{block,transformer,head}.py) over a batch of images, eval path.
//
// One plan per (batch, imgsz): every tensor is a buffer at one of the pyramid levels, the encoder's tokens a level of n images of
// 1 x tokens and the decoder's 300 queries a level of n images of 1 x 300, so that each Linear is a 1x1 conv on the shared MFMA kernels.
// HGBlock concats are buffers the block's convs write slices of; HGStem's 2x2 convs (zero pad right / bottom) are 3x3 convs whose
// first row and column of taps are zero. The plan is captured into a hipGraph after its first run.
#include "rtdetr.hpp"

#include <cmath>

#include "api_util.hpp"

namespace ffp {

namespace {
constexpr int HD = 256;
struct HgCfg { int li, c1, cm, c2, k; bool light, shortcut; };
const HgCfg kHg[6] = {{1, 48, 48, 128, 3, false, false}, {3, 128, 96, 512, 3, false, false}, {5, 512, 192, 1024, 5, true, false},
                      {6, 1024, 192, 1024, 5, true, true}, {7, 1024, 192, 1024, 5, true, true}, {9, 1024, 384, 2048, 5, true, false}};
}  // namespace

void rtdetr_anchors(int imgsz, std::vector<float>& anchors, std::vector<float>& valid) {
  anchors.clear();
  valid.clear();
  for (int l = 0; l < 3; ++l) {
    const int h = imgsz / (8 << l), w = h;
    const float wh = (float)(0.05 * std::pow(2.0, l));
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const float a[4] = {((float)x + 0.5f) / (float)w, ((float)y + 0.5f) / (float)h, wh, wh};
        bool ok = true;
        for (float v : a) ok = ok && v > 0.01f && v < 0.99f;
        for (float v : a) anchors.push_back(ok ? std::log(v / (1.0f - v)) : INFINITY);
        valid.push_back(ok ? 1.f : 0.f);
      }
  }
}

void rtdetr_pos_embed(int w, int h, std::vector<float>& pos) {
  // torch.meshgrid(grid_w, grid_h, indexing="ij") flattened: token t (row-major over h x w) gets (t / h, t % h)
  const int pd = HD / 4;
  pos.assign((size_t)w * h * HD, 0.f);
  for (int t = 0; t < w * h; ++t) {
    const float gw = (float)(t / h), gh = (float)(t % h);
    for (int i = 0; i < pd; ++i) {
      const float omega = 1.0f / std::pow(10000.0f, (float)i / (float)pd);
      const float ow = gw * omega, oh = gh * omega;
      float* p = pos.data() + (size_t)t * HD;
      p[i] = std::sin(ow); p[pd + i] = std::cos(ow); p[2 * pd + i] = std::sin(oh); p[3 * pd + i] = std::cos(oh);
    }
  }
}

RtdetrEngine::RtdetrEngine(const void* weights, size_t nbytes, int device, int precision) {
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "rtdetr: precision %d (FFP_PREC_F32 or FFP_PREC_F32X3)", precision);
  FFP_CHECK(weights && nbytes > 0, FFP_ERR_ARG, "rtdetr: empty weights");
  bytes_.assign((const uint8_t*)weights, (const uint8_t*)weights + nbytes);
  wf_.parse(bytes_.data(), bytes_.size());
  FFP_CHECK(wf_.has("model.28.enc_score_head.weight") && wf_.has("model.0.stem1.conv.weight"), FFP_ERR_ARG,
            "rtdetr: not RT-DETR-l FFPW tensors (convert the checkpoint with weights_io.from_ultralytics_rtdetr_state_dict)");
  FFP_CHECK(!wf_.has("model.0.stem1.bn.weight") && !wf_.has("model.11.ma.in_proj_weight"), FFP_ERR_ARG,
            "rtdetr: unfused tensors (BatchNorm / in_proj): convert with weights_io.from_ultralytics_rtdetr_state_dict");
  nc_ = t("model.28.enc_score_head.weight").dims[0];
  int ndev = 0;
  FFP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, FFP_ERR_HIP, "no HIP device available (the detector has no CPU path)");
  FFP_CHECK(device >= 0 && device < ndev, FFP_ERR_ARG, "device %d of %d", device, ndev);
  device_ = device;
  split_ = precision == FFP_PREC_F32X3;
  FFP_HIP(hipSetDevice(device_));
  st_ = create_engine_stream(sw().det_cu_mask);
  conv_kernels_init();
}

RtdetrEngine::~RtdetrEngine() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  plans_.clear_nothrow();
  convs_.clear();
  dev_.clear();
  if (st_) (void)hipStreamDestroy(st_);
}

std::vector<float> rtdetr_pack_depthwise(const float* w, int C, int taps) {
  std::vector<float> v((size_t)C * taps);
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < taps; ++j) v[(size_t)j * C + c] = w[(size_t)c * taps + j];
  return v;
}

const float* RtdetrEngine::dev(const std::string& name) {
  auto it = dev_.find(name);
  if (it == dev_.end()) {
    const HostTensor& h = t(name);
    DevBuf b(h.numel() * 4);
    if (h.dims.size() == 4 && h.dims[1] == 1 && h.dims[0] > 1) {         // depthwise (C, 1, k, k) -> [tap][C]
      const std::vector<float> v = rtdetr_pack_depthwise(h.data, h.dims[0], h.dims[2] * h.dims[3]);
      FFP_HIP(hipMemcpy(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    } else {
      FFP_HIP(hipMemcpy(b.p, h.data, h.numel() * 4, hipMemcpyHostToDevice));
    }
    it = dev_.emplace(name, std::move(b)).first;
  }
  return it->second.as<float>();
}

const PackedConv& RtdetrEngine::conv(const std::string& name) {
  auto it = convs_.find(name);
  if (it != convs_.end()) return *it->second;
  std::vector<float> w, b;
  int cout = 0, cin = 0, k = 1;
  auto take = [&](const std::string& wn, const std::string& bn) {
    const HostTensor& W = t(wn);
    const HostTensor& B = t(bn);
    FFP_CHECK(W.dims.size() == 2 || W.dims.size() == 4, FFP_ERR_ARG, "rtdetr: %s has %d dims", wn.c_str(), (int)W.dims.size());
    const int co = W.dims[0], ci = W.dims[1], kk = W.dims.size() == 4 ? W.dims[2] : 1;
    FFP_CHECK(cout == 0 || (ci == cin && kk == k), FFP_ERR_ARG, "rtdetr: %s does not stack", wn.c_str());
    FFP_CHECK((int)B.numel() == co, FFP_ERR_ARG, "rtdetr: %s has %zu values for %d outputs", bn.c_str(), B.numel(), co);
    cin = ci; k = kk; cout += co;
    w.insert(w.end(), W.data, W.data + W.numel());
    b.insert(b.end(), B.data, B.data + B.numel());
  };
  const auto dot = name.rfind('.');
  const std::string stem = name.substr(0, dot), tail = name.substr(dot + 1);
  if (tail == "qk") {                       // q_proj and k_proj of one attention as one GEMM: [q 256 | k 256]
    take(stem + ".q_proj.weight", stem + ".q_proj.bias");
    take(stem + ".k_proj.weight", stem + ".k_proj.bias");
  } else if (tail == "oa") {                // MSDeformAttn sampling_offsets (192) and attention_weights (96) as one GEMM
    take(stem + ".sampling_offsets.weight", stem + ".sampling_offsets.bias");
    take(stem + ".attention_weights.weight", stem + ".attention_weights.bias");
  } else {
    take(name + ".weight", name + ".bias");
  }
  if (k == 2) {                             // HGStem 2x2 conv behind F.pad(x, [0, 1, 0, 1]): taps (1..2, 1..2) of a padded 3x3
    std::vector<float> w3((size_t)cout * cin * 9, 0.f);
    for (size_t oc = 0; oc < (size_t)cout * cin; ++oc)
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) w3[oc * 9 + (1 + dy) * 3 + 1 + dx] = w[oc * 4 + dy * 2 + dx];
    w.swap(w3);
    k = 3;
  }
  FFP_CHECK(k == 1 || k == 3, FFP_ERR_ARG, "rtdetr: %s is a %dx%d conv", name.c_str(), k, k);
  std::unique_ptr<PackedConv> pc(new PackedConv());
  pack_conv(*pc, name, w.data(), b.data(), cout, cin, k, 1, F32, st_, split_);
  FFP_HIP(hipStreamSynchronize(st_));
  return *convs_.emplace(name, std::move(pc)).first->second;
}

void RtdetrEngine::build_plan(RtdetrPlan& P) {
  const int n = P.n, S = P.imgsz;
  hipStream_t st = st_;
  P.per_image_amax = false;                  // F32X3: one exponent slot per buffer (F32 results do not depend on the batch either way)
  P.px_align = 1;
  auto lvl = [&](int s) { return P.add_level(std::vector<int>(n, S / s), std::vector<int>(n, S / s), st); };
  Level* L2 = lvl(2); Level* L4 = lvl(4); Level* L8 = lvl(8); Level* L16 = lvl(16); Level* L32 = lvl(32);
  P.NT = (S / 8) * (S / 8) + (S / 16) * (S / 16) + (S / 32) * (S / 32);
  Level* LT = P.add_level(std::vector<int>(n, 1), std::vector<int>(n, P.NT), st);
  Level* LQ = P.add_level(std::vector<int>(n, 1), std::vector<int>(n, RT_NQ), st);
  auto buf = [&](Level* l, int C) { return P.alloc(l, C, F32); };
  auto cv = [&](const std::string& name, const TView& in, const TView& out, int stride, int act, const TView* res = nullptr) {
    ConvOp o;
    o.pc = &conv(name);
    o.in = in; o.out = out; o.stride = stride; o.act = act;
    if (res) { o.has_res1 = true; o.res1 = *res; o.s1 = 1.f; }
    P.add_conv(o);
  };
  auto ln = [&](const std::string& p, const TView& x) {
    const float* g = dev(p + ".weight");
    const float* b = dev(p + ".bias");
    P.add_named("rt_layernorm " + p, [x, g, b](hipStream_t q) { launch_rt_layernorm(x, g, b, x, q); });
  };
  auto dw = [&](const std::string& p, const TView& in, const TView& out, int k, int s, int act) {
    const float* w = dev(p + ".conv.weight");
    const float* b = dev(p + ".conv.bias");
    P.add_named("rt_dwconv " + p, [in, out, w, b, k, s, act](hipStream_t q) { launch_rt_dwconv(in, out, w, b, k, s, act, q); });
  };
  auto up2 = [&](const TView& in, const TView& out) {
    P.add_named("upsample2x", [in, out](hipStream_t q) { launch_upsample2x(in, out, q); launch_amax_max(out.amax, in.amax, q, out.amax_n); });
  };
  auto attn = [&](const TView& qk, const TView& v, const TView& out, int L) { P.add_named("rt_attention", [qk, v, out, L](hipStream_t q) { launch_rt_attention(qk, v, out, L, q); }); };

  // ---- HGStem ----
  Level* L1 = lvl(1);
  P.input = buf(L1, 4);
  P.set_amax_bound(P.input, 1.0f);
  const TView a2 = buf(L2, 32), b2 = buf(L2, 16), c2 = buf(L2, 64), a4 = buf(L4, 32);
  cv("model.0.stem1.conv", P.input, a2, 2, ACT_RELU);
  cv("model.0.stem2a.conv", a2, b2, 1, ACT_RELU);
  cv("model.0.stem2b.conv", b2, c2.slice(32, 32), 1, ACT_RELU);
  {
    const TView in = a2, out = c2.slice(0, 32);
    P.add_named("rt_maxpool2 model.0.pool", [in, out](hipStream_t q) { launch_rt_maxpool2(in, out, q); });
  }
  cv("model.0.stem3.conv", c2, a4, 2, ACT_RELU);
  // ---- HGBlocks and the stage DWConvs ----
  Level* hl[6] = {L4, L8, L16, L16, L16, L32};
  std::vector<TView> cat(6);
  for (int i = 0; i < 6; ++i) cat[i] = buf(hl[i], kHg[i].c1 + 6 * kHg[i].cm);
  cv("model.0.stem4.conv", a4, cat[0].slice(0, 48), 1, ACT_RELU);
  const TView o1 = buf(L4, 128), p3 = buf(L8, 512), p4 = buf(L16, 1024), p5 = buf(L32, 2048);
  const TView outs[6] = {o1, p3, cat[3].slice(0, 1024), cat[4].slice(0, 1024), p4, p5};
  for (int i = 0; i < 6; ++i) {
    const HgCfg& h = kHg[i];
    const std::string p = "model." + std::to_string(h.li);
    const TView tmp = buf(hl[i], h.cm), sc = buf(hl[i], h.c2 / 2);
    for (int j = 0; j < 6; ++j) {
      const TView src = j == 0 ? cat[i].slice(0, h.c1) : cat[i].slice(h.c1 + (j - 1) * h.cm, h.cm);
      const TView dst = cat[i].slice(h.c1 + j * h.cm, h.cm);
      const std::string m = p + ".m." + std::to_string(j);
      if (h.light) {
        cv(m + ".conv1.conv", src, tmp, 1, ACT_NONE);
        dw(m + ".conv2", tmp, dst, h.k, 1, ACT_RELU);
      } else {
        cv(m + ".conv", src, dst, 1, ACT_RELU);
      }
    }
    cv(p + ".sc.conv", cat[i], sc, 1, ACT_RELU);
    const TView res = cat[i].slice(0, h.c1);
    cv(p + ".ec.conv", sc, outs[i], 1, ACT_RELU, h.shortcut && h.c1 == h.c2 ? &res : nullptr);
    if (i == 0) dw("model.2", o1, cat[1].slice(0, 128), 3, 2, ACT_NONE);
    if (i == 1) dw("model.4", p3, cat[2].slice(0, 512), 3, 2, ACT_NONE);
    if (i == 4) dw("model.8", p4, cat[5].slice(0, 1024), 3, 2, ACT_NONE);
  }
  // ---- AIFI on P5 ----
  const int L5 = (S / 32) * (S / 32);
  std::vector<float> pos;
  rtdetr_pos_embed(S / 32, S / 32, pos);
  P.d_pos.alloc(pos.size() * 4);
  FFP_HIP(hipMemcpy(P.d_pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
  const TView src = buf(L32, HD), x5 = buf(L32, HD), qk5 = buf(L32, 2 * HD), v5 = buf(L32, HD), a5 = buf(L32, HD), s1 = buf(L32, HD),
              h5 = buf(L32, 1024), s2 = buf(L32, HD);
  cv("model.10.conv", p5, src, 1, ACT_NONE);
  {
    const float* pp = P.d_pos.as<float>();
    P.add_named("rt_add model.11.pos", [src, pp, L5, x5](hipStream_t q) { launch_rt_add(src, pp, HD, L5, x5, q); });
  }
  cv("model.11.ma.qk", x5, qk5, 1, ACT_NONE);
  cv("model.11.ma.v_proj", src, v5, 1, ACT_NONE);
  attn(qk5, v5, a5, L5);
  cv("model.11.ma.out_proj", a5, s1, 1, ACT_NONE, &src);
  ln("model.11.norm1", s1);
  cv("model.11.fc1", s1, h5, 1, ACT_NONE);
  P.add_named("rt_gelu model.11", [h5](hipStream_t q) { launch_rt_gelu(h5, q); });
  cv("model.11.fc2", h5, s2, 1, ACT_NONE, &s1);
  ln("model.11.norm2", s2);
  // ---- neck ----
  const TView c15 = buf(L16, 512), c20 = buf(L8, 512), c23 = buf(L16, 512), c26 = buf(L32, 512);
  const TView y5 = c26.slice(256, 256), y4 = c23.slice(256, 256);
  cv("model.12.conv", s2, y5, 1, ACT_SILU);
  up2(y5, c15.slice(0, 256));
  cv("model.14.conv", p4, c15.slice(256, 256), 1, ACT_NONE);
  auto repc3 = [&](int li, const TView& in, const TView& out) {
    const std::string p = "model." + std::to_string(li);
    Level* l = in.lvl;
    const TView a = buf(l, HD), b = buf(l, HD), c = buf(l, HD);
    cv(p + ".cv1.conv", in, a, 1, ACT_SILU);
    cv(p + ".cv2.conv", in, b, 1, ACT_SILU);
    cv(p + ".m.0.conv", a, c, 1, ACT_SILU);
    cv(p + ".m.1.conv", c, a, 1, ACT_SILU);
    cv(p + ".m.2.conv", a, out, 1, ACT_SILU, &b);
  };
  const TView x16 = buf(L16, HD), x21 = buf(L8, HD), x24 = buf(L16, HD), x27 = buf(L32, HD);
  repc3(16, c15, x16);
  cv("model.17.conv", x16, y4, 1, ACT_SILU);
  up2(y4, c20.slice(0, 256));
  cv("model.19.conv", p3, c20.slice(256, 256), 1, ACT_NONE);
  repc3(21, c20, x21);
  cv("model.22.conv", x21, c23.slice(0, 256), 2, ACT_SILU);
  repc3(24, c23, x24);
  cv("model.25.conv", x24, c26.slice(0, 256), 2, ACT_SILU);
  repc3(27, c26, x27);
  // ---- RTDETRDecoder: encoder input, anchors, top-300 ----
  const std::string d = "model.28";
  const TView f[3] = {buf(L8, HD), buf(L16, HD), buf(L32, HD)};
  const TView xs[3] = {x21, x24, x27};
  RtLevels lv{};
  lv.start[0] = 0;
  for (int l = 0; l < 3; ++l) {
    cv(d + ".input_proj." + std::to_string(l) + ".0", xs[l], f[l], 1, ACT_NONE);
    lv.h[l] = lv.w[l] = S / (8 << l);
    lv.start[l + 1] = lv.start[l] + lv.h[l] * lv.w[l];
    lv.src[l] = (const float*)f[l].ptr;
    lv.src_cs[l] = f[l].cs;
  }
  std::vector<float> anc, valid;
  rtdetr_anchors(S, anc, valid);
  P.d_anchors.alloc(anc.size() * 4);
  P.d_valid.alloc(valid.size() * 4);
  FFP_HIP(hipMemcpy(P.d_anchors.p, anc.data(), anc.size() * 4, hipMemcpyHostToDevice));
  FFP_HIP(hipMemcpy(P.d_valid.p, valid.data(), valid.size() * 4, hipMemcpyHostToDevice));
  const TView tok = buf(LT, HD), tokm = buf(LT, HD), enc = buf(LT, HD), vt = buf(LT, HD);
  const int ncp = (nc_ + 3) / 4 * 4;
  const TView es = buf(LT, ncp).slice(0, nc_);
  {
    const float* vd = P.d_valid.as<float>();
    P.add_named("rt_enc_prep model.28", [lv, vd, tok, tokm, n](hipStream_t q) { launch_rt_enc_prep(lv, vd, tok, tokm, n, q); });
  }
  cv(d + ".enc_output.0", tokm, enc, 1, ACT_NONE);
  ln(d + ".enc_output.1", enc);
  cv(d + ".enc_score_head", enc, es, 1, ACT_NONE);
  P.d_keys.alloc(sizeof(unsigned) * (size_t)n * P.NT);
  P.d_idx.alloc(sizeof(int) * (size_t)n * RT_NQ);
  FFP_HIP(hipMemsetAsync(P.d_idx.p, 0, P.d_idx.n, st));
  P.d_anc.alloc(sizeof(float) * 4 * (size_t)n * RT_NQ);
  const TView qa = buf(LQ, HD), qb = buf(LQ, HD), qc = buf(LQ, HD), xq = buf(LQ, HD), qkq = buf(LQ, 2 * HD), vq = buf(LQ, HD), aq = buf(LQ, HD),
              oa = buf(LQ, 288), dq = buf(LQ, HD), hq = buf(LQ, 1024), m1 = buf(LQ, HD), m2 = buf(LQ, HD), delta = buf(LQ, 4), pm = buf(LQ, 512),
              posq = buf(LQ, HD);
  P.ref = buf(LQ, 4);
  {
    unsigned* keys = P.d_keys.as<unsigned>();
    int* idx = P.d_idx.as<int>();
    float* an = P.d_anc.as<float>();
    const float* anchors = P.d_anchors.as<float>();
    const int nc = nc_, NT = P.NT;
    P.add_named("rt_topk model.28", [es, nc, NT, n, keys, idx](hipStream_t q) { launch_rt_topk(es, nc, NT, n, keys, idx, q); });
    P.add_named("rt_gather model.28", [enc, idx, anchors, NT, n, qa, an](hipStream_t q) { launch_rt_gather(enc, idx, anchors, NT, n, qa, an, q); });
  }
  auto mlp3 = [&](const std::string& p, const TView& in) {
    cv(p + ".layers.0", in, m1, 1, ACT_RELU);
    cv(p + ".layers.1", m1, m2, 1, ACT_RELU);
    cv(p + ".layers.2", m2, delta, 1, ACT_NONE);
  };
  mlp3(d + ".enc_bbox_head", qa);
  {
    const float* an = P.d_anc.as<float>();
    const TView ref = P.ref;
    P.add_named("rt_ref model.28.enc", [delta, an, ref](hipStream_t q) { launch_rt_ref(delta, an, ref, q); });
  }
  // ---- six decoder layers: q = qa, then qb / qc within a layer, back to qa ----
  for (int i = 0; i < 6; ++i) {
    const std::string p = d + ".decoder.layers." + std::to_string(i);
    const TView ref = P.ref;
    cv(d + ".query_pos_head.layers.0", ref, pm, 1, ACT_RELU);
    cv(d + ".query_pos_head.layers.1", pm, posq, 1, ACT_NONE);
    P.add_named("rt_add " + p + ".pos1", [qa, posq, xq](hipStream_t q) { launch_rt_add(qa, (const float*)posq.ptr, posq.cs, 0, xq, q); });
    cv(p + ".self_attn.qk", xq, qkq, 1, ACT_NONE);
    cv(p + ".self_attn.v_proj", qa, vq, 1, ACT_NONE);
    attn(qkq, vq, aq, RT_NQ);
    cv(p + ".self_attn.out_proj", aq, qb, 1, ACT_NONE, &qa);
    ln(p + ".norm1", qb);
    P.add_named("rt_add " + p + ".pos2", [qb, posq, xq](hipStream_t q) { launch_rt_add(qb, (const float*)posq.ptr, posq.cs, 0, xq, q); });
    cv(p + ".cross_attn.value_proj", tok, vt, 1, ACT_NONE);
    cv(p + ".cross_attn.oa", xq, oa, 1, ACT_NONE);
    P.add_named("rt_deform " + p, [vt, oa, ref, lv, dq](hipStream_t q) { launch_rt_deform(vt, oa, ref, lv, dq, q); });
    cv(p + ".cross_attn.output_proj", dq, qc, 1, ACT_NONE, &qb);
    ln(p + ".norm2", qc);
    cv(p + ".linear1", qc, hq, 1, ACT_RELU);
    cv(p + ".linear2", hq, qa, 1, ACT_NONE, &qc);
    ln(p + ".norm3", qa);
    mlp3(d + ".dec_bbox_head." + std::to_string(i), qa);
    P.add_named("rt_ref " + p, [delta, ref](hipStream_t q) { launch_rt_ref(delta, nullptr, ref, q); });
  }
  P.scores = buf(LQ, ncp).slice(0, nc_);
  cv(d + ".dec_score_head.5", qa, P.scores, 1, ACT_NONE);
  P.add_amax_reset(st);
  P.d_lb.alloc(sizeof(LetterboxImg) * n);
  P.d_wh.alloc(sizeof(float2) * n);
  P.d_raw.alloc(sizeof(float) * (size_t)n * RT_NQ * (4 + nc_));
  P.d_det.alloc(sizeof(float) * (size_t)n * RT_NQ * 6);
  P.d_counts.alloc(sizeof(int) * n);
  for (DevBuf& b : P.bufs) FFP_HIP(hipMemsetAsync(b.p, 0, b.n, st));    // padding channels are read (times zero weights): never garbage
  FFP_HIP(hipStreamSynchronize(st));
}

RtdetrPlan* RtdetrEngine::plan_for(int n, int imgsz) {
  return &plans_.get({n, imgsz}, [&] {
    std::unique_ptr<RtdetrPlan> p(new RtdetrPlan());
    p->n = n;
    p->imgsz = imgsz;
    build_plan(*p);
    return p;
  });
}

static void check_imgsz(int imgsz) {
  FFP_CHECK(imgsz >= 32 && imgsz % 32 == 0 && imgsz <= 4096, FFP_ERR_ARG, "rtdetr: imgsz %d must be a multiple of 32 in [32, 4096]", imgsz);
  FFP_CHECK((imgsz / 8) * (imgsz / 8) + (imgsz / 16) * (imgsz / 16) + (imgsz / 32) * (imgsz / 32) >= RT_NQ, FFP_ERR_ARG,
            "rtdetr: imgsz %d gives fewer encoder tokens than the decoder's %d queries", imgsz, RT_NQ);
}

LetterboxImg rtdetr_stretch(int x0, int y0, int sw, int sh, int imgsz) {
  LetterboxImg L;
  L.x0 = x0; L.y0 = y0; L.sw = sw; L.sh = sh;
  L.new_w = imgsz; L.new_h = imgsz; L.top = 0; L.left = 0; L.net_h = imgsz; L.net_w = imgsz;    // LetterBox(scale_fill=True): a stretch
  return L;
}

void rtdetr_tile_records(int H, int W, const int32_t* tiles, int n_tiles, int imgsz, std::vector<LetterboxImg>& lb) {
  lb.resize(n_tiles);
  for (int i = 0; i < n_tiles; ++i) {
    const int32_t* t = tiles + 4 * i;
    FFP_CHECK(t[0] >= 0 && t[1] >= 0 && t[2] > t[0] && t[3] > t[1] && t[2] <= W && t[3] <= H, FFP_ERR_ARG,
              "rtdetr: tile %d [%d, %d, %d, %d] is empty, inverted or outside the %d x %d frame", i, t[0], t[1], t[2], t[3], W, H);
    lb[i] = rtdetr_stretch(t[0], t[1], t[2] - t[0], t[3] - t[1], imgsz);      // the stretch prepare() builds
  }
}

RtdetrPlan* RtdetrEngine::prepare(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz) {
  FFP_CHECK(frames && hw && n > 0, FFP_ERR_ARG, "rtdetr: empty batch");
  check_imgsz(imgsz);
  int Wmax = 0;
  long long rows = 0;
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(frames[i] && hw[2 * i] > 0 && hw[2 * i + 1] > 0, FFP_ERR_ARG, "rtdetr: image %d is empty", i);
    Wmax = std::max(Wmax, (int)hw[2 * i + 1]);
    rows += hw[2 * i];
  }
  FFP_HIP(hipSetDevice(device_));
  RtdetrPlan* P = plan_for(n, imgsz);
  // the batch as one u8 canvas: image i at rows [y_i, y_i + h_i), columns [0, w_i)
  frame_.ensure((size_t)rows * Wmax * 3);
  std::vector<LetterboxImg> lb(n);
  std::vector<float2> wh(n);
  long long y = 0;
  for (int i = 0; i < n; ++i) {
    const int h = hw[2 * i], w = hw[2 * i + 1];
    FFP_HIP(hipMemcpy2DAsync((uint8_t*)frame_.p + (size_t)y * Wmax * 3, (size_t)Wmax * 3, frames[i], (size_t)w * 3, (size_t)w * 3, h,
                             hipMemcpyHostToDevice, st_));
    lb[i] = rtdetr_stretch(0, (int)y, w, h, imgsz);
    wh[i] = make_float2((float)w, (float)h);
    y += h;
  }
  FFP_HIP(hipMemcpyAsync(P->d_lb.p, lb.data(), sizeof(LetterboxImg) * n, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(P->d_wh.p, wh.data(), sizeof(float2) * n, hipMemcpyHostToDevice, st_));
  launch_letterbox(frame_.as<uint8_t>(), (int)rows, Wmax, 1, P->d_lb, P->input, st_);      // BGR -> RGB, / 255
  if (profile) {
    if (P->runs == 0) P->execute(st_, nullptr);           // the first run tunes the convs and builds lazily created tables
    profile_ms.clear();
    std::vector<std::pair<ScopedEvent, ScopedEvent>> ev;
    std::vector<std::string> names;
    for (Step& s : P->steps) {
      if (s.kind != 0) continue;
      ev.emplace_back();
      FFP_HIP(hipEventRecord(ev.back().first, st_));
      s.run(st_);
      FFP_HIP(hipEventRecord(ev.back().second, st_));
      names.push_back(s.is_conv ? "conv " + s.variant + " " + s.name : s.name.empty() ? std::string("amax_init") : s.name);
    }
    FFP_HIP(hipStreamSynchronize(st_));
    for (size_t i = 0; i < ev.size(); ++i) {
      float ms = 0.f;
      FFP_HIP(hipEventElapsedTime(&ms, ev[i].first, ev[i].second));
      profile_ms.emplace_back(names[i], ms);
    }
  } else {
    P->execute(st_, nullptr);
  }
  last_conv_flops = P->conv_flops;
  last_graph_state = P->graph_state();
  FFP_HIP(hipStreamSynchronize(st_));        // lb / wh are stack vectors
  return P;
}

void RtdetrEngine::predict(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float conf, float* out, int32_t* counts) {
  FFP_CHECK(out && counts, FFP_ERR_ARG, "rtdetr: null output");
  RtdetrPlan* P = prepare(frames, hw, n, imgsz);
  launch_rt_post(P->ref, P->scores, nc_, conf, P->d_wh.as<float2>(), n, P->d_det.as<float>(), P->d_counts.as<int>(), st_);
  FFP_HIP(hipMemcpyAsync(out, P->d_det.p, sizeof(float) * (size_t)n * RT_NQ * 6, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(counts, P->d_counts.p, sizeof(int) * n, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
}

void RtdetrEngine::forward_raw(const uint8_t* const* frames, const int32_t* hw, int n, int imgsz, float* out, int32_t* topk) {
  FFP_CHECK(out, FFP_ERR_ARG, "rtdetr: null output");
  RtdetrPlan* P = prepare(frames, hw, n, imgsz);
  launch_rt_raw(P->ref, P->scores, nc_, P->d_raw.as<float>(), st_);
  FFP_HIP(hipMemcpyAsync(out, P->d_raw.p, sizeof(float) * (size_t)n * RT_NQ * (4 + nc_), hipMemcpyDeviceToHost, st_));
  if (topk) FFP_HIP(hipMemcpyAsync(topk, P->d_idx.p, sizeof(int) * (size_t)n * RT_NQ, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
}

// ---- tiles of one frame (sahi's get_sliced_prediction over an Ultralytics RT-DETR model) ---------------------------------------------

// everything on st_, nothing waited for: the caller drains the stream (h_lb_ and the caller's `tiles` are read by the copies until then)
void RtdetrEngine::enqueue_tiles(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf,
                                 int mode, int max_batch, float* d_out, int32_t* d_counts) {
  FFP_CHECK(d_frame && H > 0 && W > 0 && d_out && d_counts, FFP_ERR_ARG, "rtdetr: tiles need a frame and outputs");
  FFP_CHECK(tiles && n_tiles > 0, FFP_ERR_ARG, "rtdetr: no tile to run (n_tiles %d)", n_tiles);
  FFP_CHECK(n_tiles <= 65536, FFP_ERR_ARG, "rtdetr: %d tiles exceed 65536", n_tiles);
  FFP_CHECK(chan_order == FFP_CHAN_AS_BGR || chan_order == FFP_CHAN_AS_RGB, FFP_ERR_ARG, "rtdetr: chan_order %d", chan_order);
  FFP_CHECK(mode == FFP_RT_TILES_LOCAL || mode == FFP_RT_TILES_SAHI, FFP_ERR_ARG, "rtdetr: tile mode %d (FFP_RT_TILES_LOCAL or FFP_RT_TILES_SAHI)", mode);
  check_imgsz(imgsz);
  rtdetr_tile_records(H, W, tiles, n_tiles, imgsz, h_lb_);
  FFP_HIP(hipSetDevice(device_));
  tiles_lb_.ensure(sizeof(LetterboxImg) * n_tiles);
  tiles_xy_.ensure(sizeof(int4) * n_tiles);
  FFP_HIP(hipMemcpyAsync(tiles_lb_.p, h_lb_.data(), sizeof(LetterboxImg) * n_tiles, hipMemcpyHostToDevice, st_));
  FFP_HIP(hipMemcpyAsync(tiles_xy_.p, tiles, sizeof(int4) * n_tiles, hipMemcpyHostToDevice, st_));
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  int off = 0;
  if (max_batch <= 0) max_batch = RT_TILES_DEFAULT_BATCH;      // this engine's sentinel: no positive size asks for the default
  for (int m : even_chunks(n_tiles, max_batch)) {
    RtdetrPlan* P = plan_for(m, imgsz);        // an eviction waits for the stream first
    FFP_HIP(hipMemcpyAsync(P->d_lb.p, tiles_lb_.as<LetterboxImg>() + off, sizeof(LetterboxImg) * m, hipMemcpyDeviceToDevice, st_));
    launch_letterbox(d_frame, H, W, flip, P->d_lb, P->input, st_);
    P->execute(st_, nullptr);
    // straight into the call-wide buffers at the chunk's tile offset: nothing to copy between the chunks and the merge
    launch_rt_post_tiles(P->ref, P->scores, nc_, conf, tiles_xy_.as<int4>() + off, m, H, W, mode, d_out + (size_t)off * RT_NQ * 6, d_counts + off, st_);
    last_conv_flops = P->conv_flops;
    last_graph_state = P->graph_state();
    off += m;
  }
}

void RtdetrEngine::infer_tiles_dev(const uint8_t* d_frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf,
                                   int mode, int max_batch, float* d_out, int32_t* d_counts) {
  enqueue_tiles(d_frame, H, W, chan_order, tiles, n_tiles, imgsz, conf, mode, max_batch, d_out, d_counts);
  FFP_HIP(hipStreamSynchronize(st_));
}

void RtdetrEngine::infer_tiles(const uint8_t* frame, int H, int W, int chan_order, const int32_t* tiles, int n_tiles, int imgsz, float conf, int mode,
                               int max_batch, float* out, int32_t* counts) {
  FFP_CHECK(out && counts, FFP_ERR_ARG, "rtdetr: null output");
  FFP_CHECK(n_tiles > 0 && n_tiles <= 65536, FFP_ERR_ARG, "rtdetr: no tile to run, or too many (n_tiles %d)", n_tiles);
  FFP_HIP(hipSetDevice(device_));
  upload_frame(frame_, frame, H, W, st_);
  const size_t nd = sizeof(float) * (size_t)n_tiles * RT_NQ * 6;
  tile_dets_.ensure(nd);
  tile_counts_.ensure(sizeof(int) * n_tiles);
  FFP_HIP(hipMemsetAsync(tile_dets_.p, 0, nd, st_));       // rows past a tile's count read as zeros
  enqueue_tiles(frame_.as<uint8_t>(), H, W, chan_order, tiles, n_tiles, imgsz, conf, mode, max_batch, tile_dets_.as<float>(), tile_counts_.as<int>());
  FFP_HIP(hipMemcpyAsync(out, tile_dets_.p, nd, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipMemcpyAsync(counts, tile_counts_.p, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
}

void RtdetrEngine::sliced_predict(const uint8_t* frame, int H, int W, int chan_order, const std::vector<int32_t>& items, int imgsz, float conf,
                                  int max_batch, int pp_type, int pp_metric, double pp_thr, int class_agnostic, float* out, int cap, int32_t* out_n) {
  FFP_CHECK(out && out_n && cap > 0, FFP_ERR_ARG, "rtdetr: sliced_predict needs an output of cap > 0 rows");
  const int n_tiles = (int)items.size() / 4;
  FFP_CHECK(n_tiles > 0 && n_tiles <= 65536, FFP_ERR_ARG, "rtdetr: no tile to run, or too many (n_tiles %d)", n_tiles);
  FFP_HIP(hipSetDevice(device_));
  upload_frame(frame_, frame, H, W, st_);
  tile_dets_.ensure(sizeof(float) * (size_t)n_tiles * RT_NQ * 6);
  tile_counts_.ensure(sizeof(int) * n_tiles);
  enqueue_tiles(frame_.as<uint8_t>(), H, W, chan_order, items.data(), n_tiles, imgsz, conf, FFP_RT_TILES_SAHI, max_batch, tile_dets_.as<float>(),
                tile_counts_.as<int>());
  const int n_max = n_tiles * RT_NQ;
  tail_.reserve(cap, 6);
  tail_.compact(tile_dets_.as<float>(), tile_counts_.as<int>(), n_tiles, RT_NQ, 6, st_);
  int rows = 0;                              // the merge's grid follows the row count: one small read back between the two halves
  FFP_HIP(hipMemcpyAsync(&rows, tail_.rows_n.p, sizeof(int), hipMemcpyDeviceToHost, st_));
  FFP_HIP(hipStreamSynchronize(st_));
  FFP_CHECK(rows >= 0 && rows <= n_max, FFP_ERR_STATE, "rtdetr: %d rows from %d tiles", rows, n_tiles);
  // one slice: its rows as they are, in query order, like the other engines' fused calls; with more tiles sahi post-processes a list of two or more
  tail_.merge(MergeRule::TwoOrMore, rows, pp_type, pp_metric, pp_thr, class_agnostic, tail_.merged.as<float>(), nullptr, tail_.merged_n.as<int>(), cap, st_);
  tail_.fetch(out, cap, 6, out_n, "rtdetr: sliced_predict", st_);      // the merge is still in flight: both copies on st_, each waited for
}

}  // namespace ffp
