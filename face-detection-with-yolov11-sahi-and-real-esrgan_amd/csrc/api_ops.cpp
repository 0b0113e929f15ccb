// api_ops.cpp — the C-ABI of libffp.so, part four of four (see api.cpp): the single-operator entries of the parity tests and the tuning hooks, with
// their process-wide test knobs. They take a device number, not a handle; each call runs on a stream of its own (api_util.hpp, ScopedStream).
#include <climits>
#include <cmath>

#include "api_util.hpp"
#include "conv_route.hpp"
#include "rtdetr.hpp"
#include "scrfd.hpp"
#include "sr_ops.hpp"
#include "yolo11.hpp"

using namespace ffp;

// ---- the operand stager of the op entries ---------------------------------------------------------------------------------------------
// Host arrays hold the images of a batch back to back, [sum h*w][cs] fp32 — whole pixel records, so a view may be a channel slice of a
// wider buffer. On the device they sit in the layout of their Level (padding pixels between aligned images are NaN going in and are not
// copied back), in the element type of the op. Output buffers are in/out: the caller's contents go up first, so bytes outside the written
// slice come back as they went in. An entry declares its ScopedStream first, stages with blocking copies, launches, and fetches after
// op_finish has drained the stream.
namespace {

void op_check_batch(const char* what, int n, const int32_t* hs, const int32_t* ws, int px_align) {
  FFP_CHECK(n > 0 && n <= 4096 && hs && ws && px_align >= 1 && px_align <= 4096, FFP_ERR_ARG, "%s: bad batch description", what);
  for (int i = 0; i < n; ++i) FFP_CHECK(hs[i] > 0 && ws[i] > 0 && hs[i] <= 8192 && ws[i] <= 8192, FFP_ERR_ARG, "%s: image %d is %dx%d", what, i, ws[i], hs[i]);
}
void op_check_view(const char* what, int cs, int coff, int C) {
  FFP_CHECK(C > 0 && coff >= 0 && cs > 0 && coff + C <= cs, FFP_ERR_ARG, "%s: channels [%d, %d) do not fit records of %d", what, coff, coff + C, cs);
}
void op_check_view4(const char* what, int cs, int coff, int C) {
  op_check_view(what, cs, coff, C);
  FFP_CHECK(C % 4 == 0 && cs % 4 == 0 && coff % 4 == 0, FFP_ERR_ARG, "%s: channels, offset and record size must be multiples of 4 (%d at %d of %d)", what, C, coff, cs);
}
DType op_dtype(const char* what, int precision) {
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F16, FFP_ERR_ARG, "%s: precision must be FFP_PREC_F32 or FFP_PREC_F16", what);
  return precision == FFP_PREC_F16 ? F16 : F32;
}

// output-size rules, per image side
int op_conv_out(int v, int k, int stride) { return (v + 2 * (k / 2) - k) / stride + 1; }      // padding k / 2
int op_avg_out(int v, int k) { return (v + k - 1) / k; }                                       // windows of k, the last one partial

// the level of a ragged batch; `size` maps every side (an output-size rule)
template <class F> void op_level(Level& L, const int32_t* hs, const int32_t* ws, int n, hipStream_t st, int px_align, F size) {
  std::vector<int> h(n), w(n);
  for (int i = 0; i < n; ++i) { h[i] = size(hs[i]); w[i] = size(ws[i]); }
  L.build(h, w, st, px_align);
}
void op_level(Level& L, const int32_t* hs, const int32_t* ws, int n, hipStream_t st, int px_align = 1) {
  op_level(L, hs, ws, n, st, px_align, [](int v) { return v; });
}
void op_level_same(Level& L, int n, int h, int w, hipStream_t st) { L.build(std::vector<int>(n, h), std::vector<int>(n, w), st); }      // n images of h x w
void op_flat_level(Level& L, int n, long long per_image, hipStream_t st) {      // n images of per_image records each
  FFP_CHECK(per_image >= 1 && per_image <= INT_MAX && n >= 1 && n <= 4096 && (long long)n * per_image <= (1ll << 28), FFP_ERR_ARG,
            "op: %d images of %lld records", n, per_image);
  op_level_same(L, n, 1, (int)per_image, st);
}

// fp32 host values <-> `count` elements of type T: the one place where a host array changes its element type
void op_narrow(DType T, const float* src, size_t count, void* dst) {
  if (T == F32) { std::memcpy(dst, src, count * sizeof(float)); return; }
  _Float16* h = static_cast<_Float16*>(dst);
  for (size_t i = 0; i < count; ++i) h[i] = (_Float16)src[i];
}
void op_widen(DType T, const void* src, size_t count, float* dst) {
  if (T == F32) { std::memcpy(dst, src, count * sizeof(float)); return; }
  const _Float16* h = static_cast<const _Float16*>(src);
  for (size_t i = 0; i < count; ++i) dst[i] = (float)h[i];
}
// `count` fp32 host values as elements of type T at the head of a device buffer with `slack` bytes behind them, and back
DevBuf op_put(DType T, const float* src, size_t count, size_t slack = 0) {
  std::vector<unsigned char> raw(count * dsize(T));
  op_narrow(T, src, count, raw.data());
  DevBuf b(raw.size() + slack);
  if (count) FFP_HIP(hipMemcpy(b.p, raw.data(), raw.size(), hipMemcpyHostToDevice));
  return b;
}
void op_get(DType T, const DevBuf& b, size_t count, float* dst) {
  std::vector<unsigned char> raw(count * dsize(T));
  if (count) FFP_HIP(hipMemcpy(raw.data(), b.p, raw.size(), hipMemcpyDeviceToHost));
  op_widen(T, raw.data(), count, dst);
}

constexpr size_t kOpSlack = 256;      // bytes behind the records of every staged tensor
// the bits of the element op_stage stores where no image has a pixel
uint32_t op_pad_value(DType T) {
  volatile float nanv = std::nanf("");      // (volatile: the conversion op_stage runs, not a folded constant)
  const float nan = nanv;
  uint32_t bits = 0;
  op_narrow(T, &nan, 1, &bits);
  return bits;
}

// max-|value| slots of one buffer, one or one per image. From the caller: its bit patterns go up and the final ones come back (fetch). From data: up only.
struct OpSlot {
  DevBuf d;
  uint32_t* host = nullptr;
  int n = 1;
  explicit OpSlot(uint32_t* h, int n_ = 1) : host(h), n(n_) { if (h) d = upload(h, (size_t)n); }
  explicit OpSlot(const std::vector<unsigned>& bits) : n((int)bits.size()) { d = upload(bits.data(), bits.size()); }
  unsigned* ptr() const { return d.as<unsigned>(); }      // null without slots
  void fetch() { if (host) FFP_HIP(hipMemcpy(host, d.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost)); }
};

// One host array of whole pixel records on the device.
struct OpTensor {
  DevBuf buf;      // the level's records, then kOpSlack bytes
  Level* lvl = nullptr;
  DType T = F32;
  int cs = 0;
  size_t elems() const { return (size_t)lvl->total_px * cs; }
  TView view(int coff, int C, const OpSlot* slot = nullptr) const {      // channels [coff, coff + C), raising `slot`
    TView v{buf.p, T, cs, coff, C, lvl};
    if (slot) { v.amax = slot->ptr(); v.amax_n = slot->n; }
    return v;
  }
  void fetch(float* dst) const {      // the images' records back to back; call after the stream has drained
    std::vector<float> t(elems());
    op_get(T, buf, t.size(), t.data());
    size_t sp = 0;
    for (int i = 0; i < lvl->n; ++i) {
      const size_t np = (size_t)lvl->h[i] * lvl->w[i];
      std::memcpy(dst + sp * cs, &t[(size_t)lvl->off[i] * cs], np * cs * sizeof(float));
      sp += np;
    }
  }
};

// src: [sum h*w][src_cs] (0: cs; fewer: channels [src_cs, cs) of a record are zero), or null: no contents, every element is the padding value.
// slack_ff: the kOpSlack bytes behind the records are 0xFF, a known pattern for op_stray.
OpTensor op_stage(Level& L, DType T, const float* src, int cs, bool slack_ff = false, int src_cs = 0) {
  if (!src_cs) src_cs = cs;
  OpTensor t;
  t.lvl = &L; t.T = T; t.cs = cs;
  std::vector<float> h(t.elems(), std::nanf(""));
  size_t sp = 0;
  for (int i = 0; src && i < L.n; ++i) {
    const size_t np = (size_t)L.h[i] * L.w[i];
    float* rec = &h[(size_t)L.off[i] * cs];
    if (src_cs == cs) std::memcpy(rec, src + sp * cs, np * cs * sizeof(float));
    else for (size_t p = 0; p < np; ++p, rec += cs) {
      std::memcpy(rec, src + (sp + p) * src_cs, src_cs * sizeof(float));
      std::fill(rec + src_cs, rec + cs, 0.f);
    }
    sp += np;
  }
  t.buf = op_put(T, h.data(), h.size(), kOpSlack);
  if (slack_ff) fill_bytes(t.buf.as<char>() + h.size() * dsize(T), 0xFF, kOpSlack);
  return t;
}

// max |value| over channels [coff, coff + C) of a host array of cs-wide records as fp32 bits, NaN left out: one per image of L, or one for the buffer
std::vector<unsigned> op_amax_bits(const float* x, const Level& L, int cs, int coff, int C, bool per_image) {
  std::vector<unsigned> bits(per_image ? L.n : 1, 0u);
  size_t sp = 0;
  for (int i = 0; i < L.n; ++i) {
    const size_t np = (size_t)L.h[i] * L.w[i];
    float m = 0.f;
    for (size_t p = 0; p < np; ++p)
      for (int c = 0; c < C; ++c) m = std::max(m, std::fabs(x[(sp + p) * cs + coff + c]));      // (max(m, NaN) is m)
    unsigned b;
    std::memcpy(&b, &m, 4);
    unsigned& slot = bits[per_image ? i : 0];
    slot = std::max(slot, b);      // non-negative floats order like their bits
    sp += np;
  }
  return bits;
}

// What changed where no kernel may write: elements of the padding pixels behind each aligned image, against the value op_stage stored, and bytes of the
// slack behind the records, against 0xFF (op_stage with slack_ff). may_write(image, channel): an element of that image's padding pixels is the kernel's to write.
template <class F> int64_t op_stray(const OpTensor& t, F may_write) {
  const Level& L = *t.lvl;
  const size_t esz = dsize(t.T), rec_bytes = t.elems() * esz;
  std::vector<unsigned char> now(rec_bytes + kOpSlack);
  FFP_HIP(hipMemcpy(now.data(), t.buf.p, now.size(), hipMemcpyDeviceToHost));
  const uint32_t pad = op_pad_value(t.T);
  int64_t bad = 0;
  for (int i = 0; i < L.n; ++i) {
    const size_t p0 = (size_t)(L.off[i] + (int64_t)L.h[i] * L.w[i]), p1 = (size_t)(i + 1 < L.n ? L.off[i + 1] : L.total_px);
    for (size_t p = p0; p < p1; ++p)
      for (int c = 0; c < t.cs; ++c) bad += !may_write(i, c) && std::memcmp(&now[(p * t.cs + c) * esz], &pad, esz) != 0;
  }
  for (size_t e = rec_bytes; e < now.size(); ++e) bad += now[e] != 0xFF;
  return bad;
}
int64_t op_stray(const OpTensor& t) { return op_stray(t, [](int, int) { return false; }); }

// the tail of an entry: drain the stream, then the blocking copies back
void op_finish(const ScopedStream& cx, std::initializer_list<std::pair<const OpTensor*, float*>> outs, std::initializer_list<OpSlot*> slots = {}) {
  FFP_HIP(hipStreamSynchronize(cx.st));
  for (const auto& o : outs) if (o.second) o.first->fetch(o.second);
  for (OpSlot* s : slots) s->fetch();
}

}  // namespace

extern "C" {

static int g_op_conv_shape = SHAPE_AUTO;
int ffp_op_conv2d_shape(int force_shape) {
  FFP_API_BEGIN
  FFP_CHECK(force_shape == SHAPE_AUTO || conv_shape_info(force_shape), FFP_ERR_ARG, "conv2d_shape: %d is not a shape number", force_shape);
  g_op_conv_shape = force_shape;
  FFP_API_END
}

int ffp_op_conv2d_shape_name(int shape, char* out, int cap) {
  FFP_API_BEGIN
  const ConvShapeInfo* s = conv_shape_info(shape);
  FFP_CHECK(s && out && cap > 0, FFP_ERR_ARG, "conv2d_shape_name: %d is not a shape number, or no output buffer", shape);
  std::snprintf(out, cap, "%s %s", s->family_name, s->suffix);
  FFP_API_END
}

static thread_local std::string tl_op_conv_variant;      // conv_variant of the op this thread's last ffp_op_conv2d / ffp_op_conv1x1_up2 launched; empty: none was
int ffp_op_conv2d_last_variant(char* out, int cap) {
  FFP_API_BEGIN
  FFP_CHECK(out && cap > 0, FFP_ERR_ARG, "conv2d_last_variant: no output buffer");
  std::snprintf(out, cap, "%s", tl_op_conv_variant.c_str());
  FFP_API_END
}

static int g_op_conv_act_post = ACT_NONE;
int ffp_op_conv2d_act_post(int act) {
  FFP_API_BEGIN
  FFP_CHECK(act >= ACT_NONE && act <= ACT_RELU, FFP_ERR_ARG, "conv2d_act_post: activation code %d (0..3)", act);
  g_op_conv_act_post = act;
  FFP_API_END
}

int ffp_op_conv2d(int device, int precision, const float* x, int n, int h, int w, int cin, const float* wt, const float* bias, int cout,
                  int k, int stride, int groups, int act, int up, const float* res, float res_scale, float* y) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0, FFP_ERR_ARG, "conv2d: bad arguments");
  FFP_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2), FFP_ERR_ARG, "conv2d: k in {1,3}, stride in {1,2}");
  ScopedStream cx(device, "conv2d");
  conv_kernels_init();
  tl_op_conv_variant.clear();
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  const bool split = precision == FFP_PREC_F32X3;
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, cout, cin, k, groups, T, cx.st, split);
  Level lin, lout;
  op_level_same(lin, n, h, w, cx.st);
  op_level_same(lout, n, op_conv_out(up ? h * 2 : h, k, stride), op_conv_out(up ? w * 2 : w, k, stride), cx.st);
  const int cin_s = pc.depthwise() ? cin : pc.cin;        // stored (padded) input channels
  const OpTensor tin = op_stage(lin, T, x, cin_s, false, cin), tout = op_stage(lout, T, nullptr, cout);
  OpTensor tres;
  if (res) tres = op_stage(lout, T, res, cout);
  OpSlot sin(op_amax_bits(x, lin, cin, 0, cin, false)), sout(std::vector<unsigned>(1, 0u));      // max-|value| slots of the input / output buffers (scaled split, see TView::amax)
  const TView vin = tin.view(0, cin_s, &sin), vout = tout.view(0, cout, &sout), vres = res ? tres.view(0, cout) : TView{};
  if (pc.depthwise()) {
    FFP_CHECK(k == 3 && stride == 1 && !up, FFP_ERR_ARG, "conv2d: depthwise is 3x3 stride 1");
    FFP_CHECK(g_op_conv_act_post == ACT_NONE, FFP_ERR_ARG, "conv2d: depthwise convs have no post-activation");
    DwConvOp o;
    o.pc = &pc; o.in = vin; o.out = vout; o.out.lvl = &lin; o.act = act;
    if (res) { o.has_res = true; o.res = vres; o.res.lvl = &lin; FFP_CHECK(res_scale == 1.f, FFP_ERR_ARG, "conv2d: depthwise residual has no scale"); }
    launch_dwconv(o, cx.st);
  } else {
    ConvOp o;
    o.pc = &pc; o.in = vin; o.out = vout; o.stride = stride; o.act = act; o.up = up;
    if (res) { o.has_res1 = true; o.res1 = vres; o.s1 = res_scale; }
    o.force_shape = g_op_conv_shape;
    o.act_post = g_op_conv_act_post;
    launch_conv(o, cx.st);
    tl_op_conv_variant = conv_variant(o);
  }
  op_finish(cx, {{&tout, y}});
  FFP_API_END
}

int ffp_op_conv1x1_up2(int device, int precision, const float* coarse, const float* fine, int n, int h, int w, int c_up, int c_fine,
                       const float* wt, const float* bias, int cout, int act, float* y) {
  FFP_API_BEGIN
  FFP_CHECK(coarse && fine && wt && y && n > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c_up > 0 && c_fine > 0 && cout > 0, FFP_ERR_ARG, "conv1x1_up2: bad arguments");
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "conv1x1_up2: fp32 precisions only");
  ScopedStream cx(device, "conv1x1_up2");
  conv_kernels_init();
  tl_op_conv_variant.clear();
  const int cin = c_up + c_fine;
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, cout, cin, 1, 1, F32, cx.st, precision == FFP_PREC_F32X3);
  FFP_CHECK(pc.cin == cin, FFP_ERR_ARG, "conv1x1_up2: channel count %d needs padding", cin);
  Level lf, lc;
  op_level_same(lf, n, h, w, cx.st);
  op_level_same(lc, n, h / 2, w / 2, cx.st);
  // the concat buffer holds the fine channels at [c_up, cin); its first c_up channels are never written (filled with NaN here:
  // a kernel that read them would show)
  std::vector<float> cat((size_t)lf.total_px * cin, std::nanf(""));
  for (size_t p = 0; p < (size_t)lf.total_px; ++p) std::memcpy(&cat[p * cin + c_up], fine + p * c_fine, sizeof(float) * c_fine);
  const OpTensor tcat = op_stage(lf, F32, cat.data(), cin), tco = op_stage(lc, F32, coarse, c_up), tout = op_stage(lf, F32, nullptr, cout);
  OpSlot sfine(op_amax_bits(fine, lf, c_fine, 0, c_fine, false)), sco(op_amax_bits(coarse, lc, c_up, 0, c_up, false)), sout(std::vector<unsigned>(1, 0u));
  const TView vin = tcat.view(0, cin, &sfine), vco = tco.view(0, c_up, &sco), vout = tout.view(0, cout, &sout);
  ConvOp o;
  o.pc = &pc; o.in = vin; o.out = vout; o.stride = 1; o.act = act;
  o.has_up2 = true; o.up2 = vco; o.up2_c = c_up; o.up2_map = lf.up2_map(&lc, cx.st);
  o.force_shape = g_op_conv_shape;
  launch_conv(o, cx.st);
  tl_op_conv_variant = conv_variant(o);
  op_finish(cx, {{&tout, y}});
  FFP_API_END
}

// ---- single-operator entry points of the detector's non-convolution kernels (tests/test_gpu_ops.py) --------------------------------
static int g_op_variant[3] = {0, 0, 0};
int ffp_op_variant(int family, int variant) {
  FFP_API_BEGIN
  FFP_CHECK(family >= 0 && family < 3 && variant >= 0 && variant <= 2, FFP_ERR_ARG, "op_variant: family %d / variant %d unknown", family, variant);
  g_op_variant[family] = variant;
  FFP_API_END
}
static int g_op_cls_tower_force = 0;      // ConvOp::dwpw_force of ffp_op_cls_tower's two launches
int ffp_op_cls_tower_variant(int rows, int wg_cap) {
  FFP_API_BEGIN
  FFP_CHECK((rows == 0 || rows == 8 || rows == 16) && wg_cap >= 0 && wg_cap <= 65535, FFP_ERR_ARG, "op_cls_tower_variant: rows %d (0, 8, 16) / workgroup cap %d", rows, wg_cap);
  g_op_cls_tower_force = (rows == 16 ? 1 : rows == 8 ? 2 : 0) | wg_cap << 2;
  FFP_API_END
}

int ffp_op_sppf_pool(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, float* y, int y_cs, int y1_coff, int y2_coff, int y3_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "sppf_pool: null argument");
  op_check_batch("sppf_pool", n, hs, ws, px_align);
  op_check_view("sppf_pool input", x_cs, x_coff, c);
  const int yo[3] = {y1_coff, y2_coff, y3_coff};
  for (int i = 0; i < 3; ++i) {
    op_check_view("sppf_pool output", y_cs, yo[i], c);
    for (int j = 0; j < i; ++j) FFP_CHECK(yo[i] >= yo[j] + c || yo[j] >= yo[i] + c, FFP_ERR_ARG, "sppf_pool: output slices %d and %d overlap", j + 1, i + 1);
  }
  const DType T = op_dtype("sppf_pool", precision);
  ScopedStream cx(device, "sppf_pool");
  Level L;
  op_level(L, hs, ws, n, cx.st, px_align);
  const OpTensor tx = op_stage(L, T, x, x_cs), ty = op_stage(L, T, y, y_cs);
  launch_sppf_pool(tx.view(x_coff, c), ty.view(y1_coff, c), ty.view(y2_coff, c), ty.view(y3_coff, c), cx.st, g_op_variant[0]);
  op_finish(cx, {{&ty, y}});
  FFP_API_END
}

int ffp_op_upsample2x(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "upsample2x: null argument");
  op_check_batch("upsample2x", n, hs, ws, px_align);
  op_check_view("upsample2x input", x_cs, x_coff, c);
  op_check_view("upsample2x output", y_cs, y_coff, c);
  const DType T = op_dtype("upsample2x", precision);
  ScopedStream cx(device, "upsample2x");
  Level L, L2;
  op_level(L, hs, ws, n, cx.st, px_align);
  op_level(L2, hs, ws, n, cx.st, px_align, [](int v) { return v * 2; });
  const OpTensor tx = op_stage(L, T, x, x_cs), ty = op_stage(L2, T, y, y_cs);
  launch_upsample2x(tx.view(x_coff, c), ty.view(y_coff, c), cx.st);
  op_finish(cx, {{&ty, y}});
  FFP_API_END
}

int ffp_op_psa_attention(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int nh, const float* qkv, int q_cs,
                         int q_coff, float* out, int o_cs, int o_coff) {
  FFP_API_BEGIN
  FFP_CHECK(qkv && out && nh > 0 && nh <= 64, FFP_ERR_ARG, "psa_attention: bad arguments");
  op_check_batch("psa_attention", n, hs, ws, px_align);
  constexpr int KD = 32, HD = 64;
  op_check_view("psa_attention qkv", q_cs, q_coff, nh * (2 * KD + HD));
  op_check_view("psa_attention output", o_cs, o_coff, nh * HD);
  const DType T = op_dtype("psa_attention", precision);
  ScopedStream cx(device, "psa_attention");
  Level L;
  op_level(L, hs, ws, n, cx.st, px_align);
  const OpTensor tq = op_stage(L, T, qkv, q_cs), to = op_stage(L, T, out, o_cs);
  launch_psa_attention(tq.view(q_coff, nh * (2 * KD + HD)), to.view(o_coff, nh * HD), nh, KD, HD, cx.st, g_op_variant[1]);
  op_finish(cx, {{&to, out}});
  FFP_API_END
}

int ffp_op_dwconv3x3(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, const float* x, int x_cs,
                     int x_coff, int grp, int grp_stride, int grp_off, const float* wt, const float* bias, int act, const float* res, int r_cs,
                     int r_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && c > 0 && act >= ACT_NONE && act <= ACT_RELU, FFP_ERR_ARG, "dwconv3x3: bad arguments");
  op_check_batch("dwconv3x3", n, hs, ws, px_align);
  FFP_CHECK(x_cs > 0 && x_coff >= 0 && grp >= 0 && grp_stride >= 0 && grp_off >= 0, FFP_ERR_ARG, "dwconv3x3: negative channel addressing");
  if (grp > 0) {      // channel ch is read at x_coff + (ch / grp) * grp_stride + grp_off + ch % grp
    FFP_CHECK(c % grp == 0 && grp_off + grp <= grp_stride, FFP_ERR_ARG, "dwconv3x3: groups of %d at offset %d do not fit records of %d (C = %d)", grp, grp_off, grp_stride, c);
    FFP_CHECK((long long)x_coff + (long long)(c / grp) * grp_stride <= x_cs, FFP_ERR_ARG, "dwconv3x3: %d group records of %d exceed the pixel record of %d", c / grp, grp_stride, x_cs);
  } else {
    FFP_CHECK(grp_stride == 0 && grp_off == 0, FFP_ERR_ARG, "dwconv3x3: grp_stride / grp_off without grp");
    op_check_view("dwconv3x3 input", x_cs, x_coff, c);
  }
  op_check_view("dwconv3x3 output", y_cs, y_coff, c);
  if (res) op_check_view("dwconv3x3 residual", r_cs, r_coff, c);
  const DType T = op_dtype("dwconv3x3", precision);
  ScopedStream cx(device, "dwconv3x3");
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, c, c, 3, c, T, cx.st, false);
  Level L;
  op_level(L, hs, ws, n, cx.st, px_align);
  const OpTensor tx = op_stage(L, T, x, x_cs), ty = op_stage(L, T, y, y_cs);
  OpTensor tres;
  if (res) tres = op_stage(L, T, res, r_cs);
  DwConvOp o;
  o.pc = &pc;
  o.in = tx.view(x_coff, c);
  o.out = ty.view(y_coff, c);
  o.act = act; o.grp = grp; o.grp_stride = grp_stride; o.grp_off = grp_off;
  if (res) { o.has_res = true; o.res = tres.view(r_coff, c); }
  o.force = g_op_variant[2];
  launch_dwconv(o, cx.st);
  op_finish(cx, {{&ty, y}});
  FFP_API_END
}

int ffp_op_cls_tower(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int cin, int nc, const float* x, const float* dw0_w,
                     const float* dw0_b, const float* pw0_w, const float* pw0_b, const float* dw1_w, const float* dw1_b, const float* pw1_w,
                     const float* pw1_b, const float* fin_w, const float* fin_b, float* e1, float* head, int head_cs, int head_coff, int64_t* stray) {
  FFP_API_BEGIN
  FFP_CHECK(x && dw0_w && dw0_b && pw0_w && pw0_b && dw1_w && dw1_b && pw1_w && pw1_b && fin_w && fin_b && head, FFP_ERR_ARG, "cls_tower: null argument");
  op_check_batch("cls_tower", n, hs, ws, px_align);
  FFP_CHECK(px_align % 32 == 0 && cin > 0 && cin % 16 == 0 && cin <= 4096 && nc >= 1 && nc <= 256, FFP_ERR_ARG, "cls_tower: px_align %d must be a multiple of 32, cin %d a multiple of 16, nc %d in [1, 256]", px_align, cin, nc);
  op_check_view("cls_tower head", head_cs, head_coff, nc);
  ScopedStream cx(device, "cls_tower");
  conv_kernels_init();
  const int C3 = 128;
  PackedConv dw0, pw0, dw1, pw1, fin;
  pack_conv(dw0, "cv3.0.0", dw0_w, dw0_b, cin, cin, 3, cin, F32, cx.st, false);
  pack_conv(pw0, "cv3.0.1", pw0_w, pw0_b, C3, cin, 1, 1, F32, cx.st, true);
  pack_conv(dw1, "cv3.1.0", dw1_w, dw1_b, C3, C3, 3, C3, F32, cx.st, false);
  pack_conv(pw1, "cv3.1.1", pw1_w, pw1_b, C3, C3, 1, 1, F32, cx.st, true);
  pack_conv(fin, "cv3.2", fin_w, fin_b, nc, C3, 1, 1, F32, cx.st, true);
  DenseF32 dense;
  dense.w.alloc(sizeof(float) * nc * C3);
  dense.b.alloc(sizeof(float) * nc);
  FFP_HIP(hipMemcpy(dense.w.p, fin_w, sizeof(float) * nc * C3, hipMemcpyHostToDevice));
  FFP_HIP(hipMemcpy(dense.b.p, fin_b, sizeof(float) * nc, hipMemcpyHostToDevice));
  Level L;
  op_level(L, hs, ws, n, cx.st, px_align);
  // e1 / e2 have no contents going up: padding pixels are never written, and the slack behind every record buffer is a known pattern too (stray)
  const OpTensor tx = op_stage(L, F32, x, cin), thead = op_stage(L, F32, head, head_cs, true), te1 = op_stage(L, F32, nullptr, C3, true),
                 te2 = op_stage(L, F32, nullptr, C3, true);
  // a max-|value| slot per (tensor, image): x's from the data, the others raised by their producers
  OpSlot sx(op_amax_bits(x, L, cin, 0, cin, true)), s1(std::vector<unsigned>(n, 0u)), s2(std::vector<unsigned>(n, 0u));
  const bool fuse_fin = nc <= 4;
  ConvOp t1, t2;
  t1.pc = &pw0; t1.dw = &dw0; t1.dw_act = ACT_SILU; t1.act = ACT_SILU;
  t1.in = tx.view(0, cin, &sx); t1.out = te1.view(0, C3, &s1);
  t2.pc = &pw1; t2.dw = &dw1; t2.dw_act = ACT_SILU; t2.act = ACT_SILU;
  t2.in = t1.out; t2.out = te2.view(0, C3, &s2);
  if (fuse_fin) t2.out.ptr = nullptr;      // never stored
  const TView logits = thead.view(head_coff, nc);
  if (fuse_fin) { t2.fin = &fin; t2.fin_w = &dense; t2.fin_out = logits; }
  t1.dwpw_force = t2.dwpw_force = g_op_cls_tower_force;
  launch_conv(t1, cx.st);
  launch_conv(t2, cx.st);
  if (!fuse_fin) {
    ConvOp t3;
    t3.pc = &fin; t3.in = t2.out; t3.out = logits; t3.act = ACT_NONE;
    launch_conv(t3, cx.st);
  }
  op_finish(cx, {{&thead, head}, {&te1, e1}});
  if (stray) {
    *stray = op_stray(te1) + op_stray(te2);
    // nc > 4: the head record is written by the plain 1x1 conv, and the flat-pixel 1x1 kernels compute padding pixels like any pixel (common.hpp, Level::build)
    if (fuse_fin) *stray += op_stray(thead);
  }
  FFP_API_END
}

// A dense conv the way the plans run it (tests/test_gpu_conv_views.py): ragged batch, levels built with `px_align`, every operand a channel slice of a
// wider record, up to two residual terms, one max-|value| slot per buffer or per image, and the gate. hs / ws are the INPUT image sizes; y, res1 and
// res2 hold the output level's images. y is in/out. *stray: what changed where the conv may not write — bytes among the 256 behind y's records, and elements
// of y's padding pixels (a 1x1 conv computes the padding pixels of its own slice like any pixel: those channels are left out of the count, except behind an
// image that is inactive under the final gate).
int ffp_op_conv2d_views(int device, int precision, int n, const int32_t* hs, const int32_t* ws, int px_align, const float* x, int x_cs, int x_coff,
                        int cin, const float* wt, const float* bias, int cout, int k, int stride, int act, int act_post, int up, const float* res1,
                        int r1_cs, int r1_coff, float s1, const float* res2, int r2_cs, int r2_coff, float s2, float* y, int y_cs, int y_coff,
                        int per_image_amax, uint32_t* amax_out, const int32_t* gate, const int32_t* gate_prev, int64_t* stray) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && y && amax_out && cin > 0 && cout > 0, FFP_ERR_ARG, "conv2d_views: null argument or no channels");
  FFP_CHECK(precision == FFP_PREC_F32 || precision == FFP_PREC_F16 || precision == FFP_PREC_F32X3, FFP_ERR_ARG, "conv2d_views: precision %d", precision);
  FFP_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2) && (up == 0 || up == 1) && (per_image_amax == 0 || per_image_amax == 1), FFP_ERR_ARG,
            "conv2d_views: k in {1,3}, stride in {1,2}, up and per_image_amax in {0,1}");
  FFP_CHECK(act >= ACT_NONE && act <= ACT_RELU && act_post >= ACT_NONE && act_post <= ACT_RELU, FFP_ERR_ARG, "conv2d_views: activation codes %d / %d (0..3)", act, act_post);
  FFP_CHECK(!gate_prev || gate, FFP_ERR_ARG, "conv2d_views: gate_prev without gate");
  op_check_batch("conv2d_views", n, hs, ws, px_align);
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  const int epv = 16 / (int)dsize(T);
  const int cin_s = (cin + epv - 1) / epv * epv;       // the packed conv's input channels: padded to 16 bytes (an image-input conv reads 3 of 4)
  op_check_view("conv2d_views input", x_cs, x_coff, cin_s);
  FFP_CHECK(x_cs % epv == 0 && x_coff % epv == 0, FFP_ERR_ARG, "conv2d_views: input view not 16-byte aligned (cs=%d coff=%d)", x_cs, x_coff);
  op_check_view("conv2d_views output", y_cs, y_coff, cout);
  if (res1) op_check_view("conv2d_views res1", r1_cs, r1_coff, cout);
  if (res2) op_check_view("conv2d_views res2", r2_cs, r2_coff, cout);
  ScopedStream cx(device, "conv2d_views");
  conv_kernels_init();
  tl_op_conv_variant.clear();
  PackedConv pc;
  pack_conv(pc, "op", wt, bias, cout, cin, k, 1, T, cx.st, precision == FFP_PREC_F32X3);
  FFP_CHECK(pc.cin == cin_s, FFP_ERR_STATE, "conv2d_views: packed conv reads %d channels, expected %d", pc.cin, cin_s);
  Level lin, lout;
  op_level(lin, hs, ws, n, cx.st, px_align);
  op_level(lout, hs, ws, n, cx.st, px_align, [&](int v) { return op_conv_out(up ? v * 2 : v, k, stride); });
  lout.gate_compact = &launch_gate_compact;
  const OpTensor tin = op_stage(lin, T, x, x_cs);
  OpTensor tout, tr1, tr2;
  if (res1) tr1 = op_stage(lout, T, res1, r1_cs);
  if (res2) tr2 = op_stage(lout, T, res2, r2_cs);
  // max-|value| slots: the input's from the data, per image over the view's own channels, NaN (an inactive image on its way up) left out; the
  // output's start from the caller's bit patterns
  const int ns = per_image_amax ? n : 1;
  OpSlot sin(op_amax_bits(x, lin, x_cs, x_coff, cin, per_image_amax != 0)), sout(nullptr);
  DevBuf dgate;
  ConvOp o;
  auto stage_outputs = [&]() {      // a new allocation every time: the view is bound again
    tout = op_stage(lout, T, y, y_cs, true);
    sout = OpSlot(amax_out, ns);
    o.out = tout.view(y_coff, cout, &sout);
  };
  stage_outputs();
  if (gate) dgate = upload(gate_prev ? gate_prev : gate, (size_t)n);
  o.pc = &pc; o.stride = stride; o.act = act; o.act_post = act_post; o.up = up;
  o.in = tin.view(x_coff, cin_s, &sin);
  if (res1) { o.has_res1 = true; o.res1 = tr1.view(r1_coff, cout); o.s1 = s1; }
  if (res2) { o.has_res2 = true; o.res2 = tr2.view(r2_coff, cout); o.s2 = s2; }
  if (gate) o.gate = dgate.as<int>();
  o.force_shape = g_op_conv_shape;
  launch_conv(o, cx.st);
  tl_op_conv_variant = conv_variant(o);
  FFP_HIP(hipStreamSynchronize(cx.st));
  if (gate_prev) {      // what a captured plan does between two runs with different gates: same tables, same launches, the mask rewritten and the gated tables compacted again
    stage_outputs();
    FFP_HIP(hipMemcpy(dgate.p, gate, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    lout.compact_gated(cx.st);
    launch_conv(o, cx.st);
  }
  op_finish(cx, {{&tout, y}}, {&sout});
  // (a 1x1 conv computes the padding pixels of its own slice like any pixel; behind an inactive image they are nobody's to write)
  if (stray) *stray = op_stray(tout, [&](int i, int c) { return k == 1 && c >= y_coff && c < y_coff + cout && (!gate || gate[i]); });
  FFP_API_END
}

int ffp_op_det_post(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int nc, int nkpt, const float* head8, const float* head16,
                    const float* head32, const float* gain_pad, const int32_t* rects, float conf, float iou, int max_det, int round_boxes,
                    int shift, int full_h, int full_w, float* out_raw, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(head8 && head16 && head32 && gain_pad && rects && nc >= 1 && nc <= 1024 && nkpt >= 0 && nkpt <= 64, FFP_ERR_ARG, "det_post: bad arguments");
  FFP_CHECK((out_dets != nullptr) == (out_counts != nullptr) && (out_raw || out_dets), FFP_ERR_ARG, "det_post: dets and counts come together, and something must be asked for");
  op_check_batch("det_post", n, hs, ws, px_align);
  for (int i = 0; i < n; ++i) {
    FFP_CHECK(hs[i] % 32 == 0 && ws[i] % 32 == 0, FFP_ERR_ARG, "det_post: net input %dx%d of image %d is not a multiple of 32", ws[i], hs[i], i);
    FFP_CHECK(gain_pad[3 * i] > 0.f && rects[4 * i] > 0 && rects[4 * i + 1] > 0, FFP_ERR_ARG, "det_post: image %d has no gain or no size", i);
  }
  if (out_dets) FFP_CHECK(max_det >= 1 && max_det <= 1024 && conf >= 0.f, FFP_ERR_ARG, "det_post: max_det %d outside [1,1024] or negative conf", max_det);
  ScopedStream cx(device, "det_post");
  const int cs = 64 + nc + 3 * nkpt, no = 4 + nc + 3 * nkpt, stride = 6 + 3 * nkpt;
  Level L[3];
  OpTensor th[3];
  const float* heads[3] = {head8, head16, head32};
  for (int l = 0; l < 3; ++l) {
    op_level(L[l], hs, ws, n, cx.st, px_align, [l](int v) { return v / (8 << l); });
    th[l] = op_stage(L[l], F32, heads[l], cs);
  }
  std::vector<int> aoff(n + 1, 0);
  std::vector<long long> roff(n);
  long long rtot = 0;
  for (int i = 0; i < n; ++i) {
    int a = 0;
    for (int l = 0; l < 3; ++l) a += L[l].h[i] * L[l].w[i];
    aoff[i + 1] = aoff[i] + a;
    roff[i] = rtot;
    rtot += (long long)no * a;
  }
  const int total = aoff[n];
  std::vector<DetImg> di(n);
  for (int i = 0; i < n; ++i) {
    di[i].gain = gain_pad[3 * i]; di[i].pad_x = gain_pad[3 * i + 1]; di[i].pad_y = gain_pad[3 * i + 2];
    di[i].sw = rects[4 * i]; di[i].sh = rects[4 * i + 1]; di[i].x0 = rects[4 * i + 2]; di[i].y0 = rects[4 * i + 3];
  }
  DevBuf d_aoff = upload(aoff.data(), aoff.size()), d_roff = upload(roff.data(), roff.size()), d_imgs = upload(di.data(), di.size());
  DecodeArgs a{};
  for (int l = 0; l < 3; ++l) { a.head[l] = th[l].buf.as<float>(); a.tab[l] = L[l].d_tab.as<int4>(); }
  a.head_cs = cs; a.nc = nc; a.nkpt = nkpt; a.n_img = n; a.anchor_off = d_aoff.as<int>(); a.total_anchors = total;
  if (out_raw) {
    DevBuf d_raw(sizeof(float) * (size_t)rtot);
    launch_decode_raw(a, d_raw.as<float>(), d_roff.as<long long>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    FFP_HIP(hipMemcpy(out_raw, d_raw.p, sizeof(float) * (size_t)rtot, hipMemcpyDeviceToHost));
  }
  if (out_dets) {
    DevBuf d_boxes(sizeof(float4) * (size_t)total), d_scores(sizeof(float) * (size_t)total), d_classes(sizeof(int) * (size_t)total),
        d_cand(sizeof(int) * (size_t)total), d_cscore(sizeof(float) * (size_t)total);
    const size_t nd = (size_t)n * max_det * stride;
    DevBuf d_dets(sizeof(float) * nd), d_counts(sizeof(int) * (size_t)n);
    FFP_HIP(hipMemsetAsync(d_dets.p, 0, sizeof(float) * nd, cx.st));
    launch_decode(a, conf, d_boxes.as<float4>(), d_scores.as<float>(), d_classes.as<int>(), cx.st);
    launch_nms(a, d_boxes.as<float4>(), d_scores.as<float>(), d_classes.as<int>(), d_cand.as<int>(), d_cscore.as<float>(), d_imgs.as<DetImg>(), iou,
               max_det, round_boxes, stride, d_dets.as<float>(), d_counts.as<int>(), cx.st);
    if (shift) launch_truncate_shift(d_dets.as<float>(), d_counts.as<int>(), d_imgs.as<DetImg>(), n, max_det, stride, nkpt, full_h, full_w, cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    FFP_HIP(hipMemcpy(out_dets, d_dets.p, sizeof(float) * nd, hipMemcpyDeviceToHost));
    FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

int ffp_op_rt_topk(int device, int n, int nt, int nc, const float* scores, int s_cs, int s_coff, int32_t* out_idx) {
  FFP_API_BEGIN
  FFP_CHECK(scores && out_idx && n > 0 && n <= 4096 && nt >= RT_NQ && nt <= (1 << 22), FFP_ERR_ARG, "rt_topk: needs n in [1,4096] images of [%d, 2^22] tokens", RT_NQ);
  op_check_view("rt_topk scores", s_cs, s_coff, nc);
  ScopedStream cx(device, "rt_topk");
  const size_t tok = (size_t)n * nt;
  DevBuf keys(sizeof(unsigned) * tok), idx(sizeof(int) * (size_t)n * RT_NQ);
  Level L;
  op_level_same(L, n, 1, nt, cx.st);
  const OpTensor ts = op_stage(L, F32, scores, s_cs);
  launch_rt_topk(ts.view(s_coff, nc), nc, nt, n, keys.as<unsigned>(), idx.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(out_idx, idx.p, sizeof(int) * (size_t)n * RT_NQ, hipMemcpyDeviceToHost));
  FFP_API_END
}

// ---- single-operator entry points of the RT-DETR and SCRFD kernels (tests/test_gpu_rtdetr_ops.py, tests/test_gpu_scrfd_ops.py) -------
// The rt_* kernels address image i at i * h * w without padding: their levels are built without alignment, where staging is a plain copy; the
// launches are the plans' own.
namespace {

void op_fetch(const DevBuf& b, float* dst, size_t n) { FFP_HIP(hipMemcpy(dst, b.p, n * sizeof(float), hipMemcpyDeviceToHost)); }      // a flat fp32 array

void op_rt_levels(const char* what, const int32_t* hs, const int32_t* ws, RtLevels& lv) {
  FFP_CHECK(hs && ws, FFP_ERR_ARG, "%s: null level sizes", what);
  lv.start[0] = 0;
  for (int l = 0; l < 3; ++l) {
    FFP_CHECK(hs[l] >= 1 && ws[l] >= 1 && hs[l] <= 4096 && ws[l] <= 4096, FFP_ERR_ARG, "%s: level %d is %dx%d", what, l, ws[l], hs[l]);
    lv.h[l] = hs[l]; lv.w[l] = ws[l];
    lv.start[l + 1] = lv.start[l] + hs[l] * ws[l];
  }
}

}  // namespace

int ffp_op_rt_dwconv(int device, int n, int h, int w, int c, int k, int s, int act, const float* x, int x_cs, int x_coff, const float* wt,
                     const float* bias, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x && wt && bias && y, FFP_ERR_ARG, "rt_dwconv: null argument");
  FFP_CHECK((k == 5 && s == 1) || (k == 3 && s == 2), FFP_ERR_ARG, "rt_dwconv: k%d s%d (k5 s1 or k3 s2)", k, s);
  FFP_CHECK(act == ACT_NONE || act == ACT_RELU, FFP_ERR_ARG, "rt_dwconv: act %d (0 none, 3 ReLU)", act);
  FFP_CHECK(n >= 1 && n <= 4096 && h >= 1 && w >= 1 && h <= 8192 && w <= 8192, FFP_ERR_ARG, "rt_dwconv: %d images of %dx%d", n, w, h);
  op_check_view4("rt_dwconv input", x_cs, x_coff, c);
  op_check_view4("rt_dwconv output", y_cs, y_coff, c);
  ScopedStream cx(device, "rt_dwconv");
  Level Li, Lo;
  op_level_same(Li, n, h, w, cx.st);
  op_level_same(Lo, n, op_conv_out(h, k, s), op_conv_out(w, k, s), cx.st);
  const std::vector<float> wp = rtdetr_pack_depthwise(wt, c, k * k);
  const OpTensor tx = op_stage(Li, F32, x, x_cs), ty = op_stage(Lo, F32, y, y_cs);
  DevBuf dw = upload(wp.data(), wp.size()), db = upload(bias, (size_t)c);
  OpSlot slot(amax);
  launch_rt_dwconv(tx.view(x_coff, c), ty.view(y_coff, c, &slot), dw.as<float>(), db.as<float>(), k, s, act, cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_maxpool2(int device, int n, int h, int w, int c, const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "rt_maxpool2: null argument");
  FFP_CHECK(n >= 1 && n <= 4096 && h >= 1 && w >= 1 && h <= 8192 && w <= 8192, FFP_ERR_ARG, "rt_maxpool2: %d images of %dx%d", n, w, h);
  op_check_view4("rt_maxpool2 input", x_cs, x_coff, c);
  op_check_view4("rt_maxpool2 output", y_cs, y_coff, c);
  ScopedStream cx(device, "rt_maxpool2");
  Level L;
  op_level_same(L, n, h, w, cx.st);
  const OpTensor tx = op_stage(L, F32, x, x_cs), ty = op_stage(L, F32, y, y_cs);
  OpSlot slot(amax);
  launch_rt_maxpool2(tx.view(x_coff, c), ty.view(y_coff, c, &slot), cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_add(int device, long long npx, int c, const float* a, int a_cs, int a_coff, const float* b, int b_cs, int b_coff, long long period,
                  float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(a && b && y, FFP_ERR_ARG, "rt_add: null argument");
  FFP_CHECK(period >= 0 && period <= npx, FFP_ERR_ARG, "rt_add: period %lld of %lld records", period, npx);
  op_check_view4("rt_add a", a_cs, a_coff, c);
  op_check_view4("rt_add b", b_cs, b_coff, c);
  op_check_view4("rt_add output", y_cs, y_coff, c);
  ScopedStream cx(device, "rt_add");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  const OpTensor ta = op_stage(L, F32, a, a_cs), ty = op_stage(L, F32, y, y_cs);
  DevBuf db = upload(b, (size_t)(period ? period : npx) * b_cs);
  OpSlot slot(amax);
  launch_rt_add(ta.view(a_coff, c), db.as<float>() + b_coff, b_cs, period, ty.view(y_coff, c, &slot), cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_layernorm(int device, long long npx, const float* x, int x_cs, int x_coff, const float* gamma, const float* beta, float* y, int y_cs,
                        int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(gamma && beta && y, FFP_ERR_ARG, "rt_layernorm: null argument");
  if (x) op_check_view4("rt_layernorm input", x_cs, x_coff, 256);
  op_check_view4("rt_layernorm output", y_cs, y_coff, 256);
  ScopedStream cx(device, "rt_layernorm");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  const OpTensor ty = op_stage(L, F32, y, y_cs);
  OpTensor tx;
  if (x) tx = op_stage(L, F32, x, x_cs);
  DevBuf dg = upload(gamma, (size_t)256), db = upload(beta, (size_t)256);
  OpSlot slot(amax);
  const TView out = ty.view(y_coff, 256, &slot);
  launch_rt_layernorm(x ? tx.view(x_coff, 256) : out, dg.as<float>(), db.as<float>(), out, cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_gelu(int device, long long npx, int c, float* x, int cs, int coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(x, FFP_ERR_ARG, "rt_gelu: null argument");
  op_check_view4("rt_gelu", cs, coff, c);
  ScopedStream cx(device, "rt_gelu");
  Level L;
  op_flat_level(L, 1, npx, cx.st);
  const OpTensor tx = op_stage(L, F32, x, cs);
  OpSlot slot(amax);
  launch_rt_gelu(tx.view(coff, c, &slot), cx.st);
  op_finish(cx, {{&tx, x}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_attention(int device, int n, int L, const float* qk, int qk_cs, int qk_coff, const float* v, int v_cs, int v_coff, float* y, int y_cs,
                        int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(qk && v && y, FFP_ERR_ARG, "rt_attention: null argument");
  op_check_view("rt_attention qk", qk_cs, qk_coff, 512);
  op_check_view("rt_attention v", v_cs, v_coff, 256);
  op_check_view("rt_attention output", y_cs, y_coff, 256);
  ScopedStream cx(device, "rt_attention");
  Level Lv;
  op_flat_level(Lv, n, L, cx.st);
  const OpTensor tq = op_stage(Lv, F32, qk, qk_cs), tv = op_stage(Lv, F32, v, v_cs), ty = op_stage(Lv, F32, y, y_cs);
  OpSlot slot(amax);
  launch_rt_attention(tq.view(qk_coff, 512), tv.view(v_coff, 256), ty.view(y_coff, 256, &slot), L, cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_enc_prep(int device, int n, const int32_t* hs, const int32_t* ws, const float* src0, const float* src1, const float* src2,
                       const int32_t* src_cs, const int32_t* src_coff, const float* valid, long long rows, float* t, float* tm, uint32_t* amax_t,
                       uint32_t* amax_tm) {
  FFP_API_BEGIN
  FFP_CHECK(src0 && src1 && src2 && src_cs && src_coff && valid && t && tm, FFP_ERR_ARG, "rt_enc_prep: null argument");
  RtLevels lv{};
  op_rt_levels("rt_enc_prep", hs, ws, lv);
  const int NT = lv.start[3];
  FFP_CHECK(n >= 1 && n <= 4096 && NT >= 1 && rows >= (long long)n * NT && rows <= (1ll << 24), FFP_ERR_ARG, "rt_enc_prep: %d images of %d tokens in %lld records", n, NT, rows);
  for (int l = 0; l < 3; ++l) op_check_view4("rt_enc_prep level", src_cs[l], src_coff[l], 256);
  ScopedStream cx(device, "rt_enc_prep");
  const float* src[3] = {src0, src1, src2};
  DevBuf ds[3];
  for (int l = 0; l < 3; ++l) {
    ds[l] = upload(src[l], (size_t)n * lv.h[l] * lv.w[l] * src_cs[l]);
    lv.src[l] = ds[l].as<float>() + src_coff[l];
    lv.src_cs[l] = src_cs[l];
  }
  Level LT, LR;      // the tokens the kernel writes, and the `rows` records the caller's buffers hold
  op_flat_level(LT, n, NT, cx.st);
  op_flat_level(LR, 1, rows, cx.st);
  DevBuf dv = upload(valid, (size_t)NT);
  const OpTensor tt = op_stage(LR, F32, t, 256), ttm = op_stage(LR, F32, tm, 256);
  OpSlot st(amax_t), stm(amax_tm);
  TView vt = tt.view(0, 256, &st), vtm = ttm.view(0, 256, &stm);
  vt.lvl = vtm.lvl = &LT;
  launch_rt_enc_prep(lv, dv.as<float>(), vt, vtm, n, cx.st);
  op_finish(cx, {{&tt, t}, {&ttm, tm}}, {&st, &stm});
  FFP_API_END
}

int ffp_op_rt_gather(int device, int n, int nt, const float* e, int e_cs, int e_coff, const int32_t* idx, const float* anchors, float* q, int q_cs,
                     int q_coff, float* anc_out, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(e && idx && anchors && q && anc_out, FFP_ERR_ARG, "rt_gather: null argument");
  FFP_CHECK(nt >= 1 && nt <= (1 << 22), FFP_ERR_ARG, "rt_gather: %d tokens", nt);
  op_check_view4("rt_gather tokens", e_cs, e_coff, 256);
  op_check_view4("rt_gather queries", q_cs, q_coff, 256);
  ScopedStream cx(device, "rt_gather");
  Level LT, LQ;
  op_flat_level(LT, n, nt, cx.st);
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  const OpTensor te = op_stage(LT, F32, e, e_cs), tq = op_stage(LQ, F32, q, q_cs);
  DevBuf di = upload(idx, nq), da = upload(anchors, (size_t)nt * 4), dan = upload(anc_out, nq * 4);
  OpSlot slot(amax);
  // the kernel takes whole 256-channel records: the slices start at the views' pointers
  TView ve = te.view(0, 256), vq = tq.view(0, 256, &slot);
  ve.ptr = te.buf.as<float>() + e_coff;
  vq.ptr = tq.buf.as<float>() + q_coff;
  launch_rt_gather(ve, di.as<int>(), da.as<float>(), nt, n, vq, dan.as<float>(), cx.st);
  op_finish(cx, {{&tq, q}}, {&slot});
  op_fetch(dan, anc_out, nq * 4);
  FFP_API_END
}

int ffp_op_rt_ref(int device, long long nq, const float* delta, int d_cs, int d_coff, const float* anc, float* ref, int r_cs, int r_coff,
                  uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(delta && ref, FFP_ERR_ARG, "rt_ref: null argument");
  op_check_view("rt_ref delta", d_cs, d_coff, 4);
  op_check_view("rt_ref boxes", r_cs, r_coff, 4);
  ScopedStream cx(device, "rt_ref");
  Level L;
  op_flat_level(L, 1, nq, cx.st);
  const OpTensor td = op_stage(L, F32, delta, d_cs), tr = op_stage(L, F32, ref, r_cs);
  DevBuf da;
  if (anc) da = upload(anc, (size_t)nq * 4);
  OpSlot slot(amax);
  launch_rt_ref(td.view(d_coff, 4), anc ? da.as<float>() : nullptr, tr.view(r_coff, 4, &slot), cx.st);
  op_finish(cx, {{&tr, ref}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_deform(int device, int n, const int32_t* hs, const int32_t* ws, const float* val, int v_cs, int v_coff, const float* oa, int oa_cs,
                     int oa_coff, const float* ref, int r_cs, int r_coff, float* y, int y_cs, int y_coff, uint32_t* amax) {
  FFP_API_BEGIN
  FFP_CHECK(val && oa && ref && y, FFP_ERR_ARG, "rt_deform: null argument");
  RtLevels lv{};
  op_rt_levels("rt_deform", hs, ws, lv);
  const int NT = lv.start[3];
  op_check_view("rt_deform values", v_cs, v_coff, 256);
  op_check_view("rt_deform offsets and weights", oa_cs, oa_coff, 288);
  op_check_view("rt_deform boxes", r_cs, r_coff, 4);
  op_check_view("rt_deform output", y_cs, y_coff, 256);
  ScopedStream cx(device, "rt_deform");
  Level LT, LQ;
  op_flat_level(LT, n, NT, cx.st);
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const OpTensor tv = op_stage(LT, F32, val, v_cs), toa = op_stage(LQ, F32, oa, oa_cs), tr = op_stage(LQ, F32, ref, r_cs), ty = op_stage(LQ, F32, y, y_cs);
  OpSlot slot(amax);
  launch_rt_deform(tv.view(v_coff, 256), toa.view(oa_coff, 288), tr.view(r_coff, 4), lv, ty.view(y_coff, 256, &slot), cx.st);
  op_finish(cx, {{&ty, y}}, {&slot});
  FFP_API_END
}

int ffp_op_rt_decode(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                     const float* orig_wh, float* out_raw, float* out_det, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(ref && scores && nc >= 1 && nc <= 4096, FFP_ERR_ARG, "rt_decode: bad arguments");
  FFP_CHECK((out_det != nullptr) == (out_counts != nullptr) && (out_raw || out_det) && (!out_det || orig_wh), FFP_ERR_ARG,
            "rt_decode: det, counts and orig_wh come together, and something must be asked for");
  op_check_view("rt_decode boxes", r_cs, r_coff, 4);
  op_check_view("rt_decode scores", s_cs, s_coff, nc);
  ScopedStream cx(device, "rt_decode");
  Level LQ;
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  const OpTensor tr = op_stage(LQ, F32, ref, r_cs), ts = op_stage(LQ, F32, scores, s_cs);
  const TView vr = tr.view(r_coff, 4), vs = ts.view(s_coff, nc);
  if (out_raw) {
    DevBuf d_raw = upload(out_raw, nq * (4 + nc));
    launch_rt_raw(vr, vs, nc, d_raw.as<float>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    op_fetch(d_raw, out_raw, nq * (4 + nc));
  }
  if (out_det) {
    DevBuf d_det = upload(out_det, nq * 6), d_wh = upload(orig_wh, (size_t)n * 2), d_counts = upload(out_counts, (size_t)n);
    launch_rt_post(vr, vs, nc, conf, d_wh.as<float2>(), n, d_det.as<float>(), d_counts.as<int>(), cx.st);
    FFP_HIP(hipStreamSynchronize(cx.st));
    op_fetch(d_det, out_det, nq * 6);
    FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  }
  FFP_API_END
}

int ffp_op_rt_post_tiles(int device, int n, int nc, const float* ref, int r_cs, int r_coff, const float* scores, int s_cs, int s_coff, float conf,
                         const int32_t* tiles_xyxy, int full_h, int full_w, int mode, float* out_dets, int32_t* out_counts) {
  FFP_API_BEGIN
  FFP_CHECK(ref && scores && tiles_xyxy && out_dets && out_counts && nc >= 1 && nc <= 4096, FFP_ERR_ARG, "rt_post_tiles: bad arguments");
  FFP_CHECK(full_h > 0 && full_w > 0 && (mode == FFP_RT_TILES_LOCAL || mode == FFP_RT_TILES_SAHI), FFP_ERR_ARG,
            "rt_post_tiles: full shape %d x %d, mode %d", full_w, full_h, mode);
  op_check_view("rt_post_tiles boxes", r_cs, r_coff, 4);
  op_check_view("rt_post_tiles scores", s_cs, s_coff, nc);
  ScopedStream cx(device, "rt_post_tiles");
  Level LQ;
  op_flat_level(LQ, n, RT_NQ, cx.st);
  const size_t nq = (size_t)n * RT_NQ;
  const OpTensor tr = op_stage(LQ, F32, ref, r_cs), ts = op_stage(LQ, F32, scores, s_cs);
  DevBuf dt = upload(tiles_xyxy, (size_t)n * 4), d_det = upload(out_dets, nq * 6), d_counts = upload(out_counts, (size_t)n);
  launch_rt_post_tiles(tr.view(r_coff, 4), ts.view(s_coff, nc), nc, conf, dt.as<int4>(), n, full_h, full_w, mode,
                       d_det.as<float>(), d_counts.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(d_det, out_dets, nq * 6);
  FFP_HIP(hipMemcpy(out_counts, d_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_op_scrfd_pool(int device, int n, const int32_t* hs, const int32_t* ws, int px_align, int c, int maxpool, int k, const float* x, int x_cs,
                      int x_coff, float* y, int y_cs, int y_coff) {
  FFP_API_BEGIN
  FFP_CHECK(x && y, FFP_ERR_ARG, "scrfd_pool: null argument");
  FFP_CHECK(maxpool || (k >= 1 && k <= 8), FFP_ERR_ARG, "scrfd_pool: average window %d outside [1, 8]", k);
  op_check_batch("scrfd_pool", n, hs, ws, px_align);
  op_check_view("scrfd_pool input", x_cs, x_coff, c);
  op_check_view("scrfd_pool output", y_cs, y_coff, c);
  ScopedStream cx(device, "scrfd_pool");
  Level Li, Lo;
  op_level(Li, hs, ws, n, cx.st, px_align);
  op_level(Lo, hs, ws, n, cx.st, px_align, [&](int v) { return maxpool ? op_conv_out(v, 3, 2) : op_avg_out(v, k); });
  const OpTensor tx = op_stage(Li, F32, x, x_cs), ty = op_stage(Lo, F32, y, y_cs);
  launch_scrfd_pool(tx.view(x_coff, c), ty.view(y_coff, c), maxpool ? 1 : 0, k, cx.st);
  op_finish(cx, {{&ty, y}});
  FFP_API_END
}

int ffp_op_scrfd_post(int device, int n, int net_h, int net_w, int A, const int32_t* strides, int px_align, const float* const* heads,
                      const int32_t* cs, const int32_t* coff, const float* det_scale, float thresh, float nms_thresh, int cap, float* out,
                      int32_t* out_counts, float* raw_scores) {
  FFP_API_BEGIN
  FFP_CHECK(strides && heads && cs && coff && det_scale && out && out_counts, FFP_ERR_ARG, "scrfd_post: null argument");
  FFP_CHECK(n >= 1 && n <= 4096 && A >= 1 && A <= 16 && cap >= 1 && cap <= (1 << 20) && px_align >= 1 && px_align <= 4096 && net_h >= 1 && net_w >= 1 &&
                net_h <= 8192 && net_w <= 8192, FFP_ERR_ARG, "scrfd_post: bad sizes");
  const bool use_kps = heads[6] != nullptr;
  const int per_px[3] = {A, 4 * A, 10 * A};
  for (int kind = 0; kind < 3; ++kind) {
    for (int l = 0; l < 3; ++l)
      FFP_CHECK((heads[3 * kind + l] != nullptr) == (kind < 2 || use_kps), FFP_ERR_ARG, "scrfd_post: head %d of level %d missing (kps: all three levels or none)", kind, l);
    if (kind < 2 || use_kps) op_check_view("scrfd_post head", cs[kind], coff[kind], per_px[kind]);
  }
  for (int i = 0; i < n; ++i) FFP_CHECK(det_scale[i] > 0.f, FFP_ERR_ARG, "scrfd_post: det_scale of image %d", i);
  ScopedStream cx(device, "scrfd_post");
  Level L[3];
  OpTensor th[3][3];
  ScrfdHeads h{};
  h.A = A;
  h.a_off[0] = 0;
  for (int l = 0; l < 3; ++l) {
    FFP_CHECK(strides[l] >= 1 && net_h % strides[l] == 0 && net_w % strides[l] == 0, FFP_ERR_ARG, "scrfd_post: stride %d does not divide %dx%d", strides[l], net_w, net_h);
    const int lh = net_h / strides[l], lw = net_w / strides[l];
    L[l].build(std::vector<int>(n, lh), std::vector<int>(n, lw), cx.st, px_align);
    for (int kind = 0; kind < 3; ++kind) {
      if (!heads[3 * kind + l]) continue;
      th[kind][l] = op_stage(L[l], F32, heads[3 * kind + l], cs[kind]);
      h.cs[kind][l] = cs[kind];
      h.coff[kind][l] = coff[kind];
    }
    h.score[l] = th[0][l].buf.as<float>();
    h.bbox[l] = th[1][l].buf.as<float>();
    h.kps[l] = th[2][l].buf.as<float>();      // null without keypoints
    h.tab[l] = L[l].d_tab.as<int4>();
    h.stride[l] = strides[l];
    h.a_off[l + 1] = h.a_off[l] + lh * lw * A;
  }
  h.per_img = h.a_off[3];
  DevBuf d_scale = upload(det_scale, (size_t)n);
  h.det_scale = d_scale.as<float>();
  const size_t na = (size_t)n * h.per_img, no = (size_t)n * cap * FFP_DET_STRIDE(5);
  DevBuf d_cand(sizeof(ScrfdCand) * na), d_counts(sizeof(int) * (size_t)n), d_order(sizeof(int) * na), d_supp(sizeof(int) * na),
      d_out = upload(out, no), d_out_counts(sizeof(int) * (size_t)n), d_raw;
  if (raw_scores) {
    d_raw.alloc(sizeof(float) * na);
    launch_scrfd_decode(h, n, 0.f, nullptr, nullptr, d_raw.as<float>(), cx.st);
  }
  launch_scrfd_decode(h, n, thresh, d_cand.as<ScrfdCand>(), d_counts.as<int>(), nullptr, cx.st);
  launch_scrfd_nms(d_cand.as<ScrfdCand>(), d_counts.as<int>(), n, h.per_img, d_order.as<int>(), d_supp.as<int>(), nms_thresh, d_out.as<float>(), cap,
                   d_out_counts.as<int>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_fetch(d_out, out, no);
  FFP_HIP(hipMemcpy(out_counts, d_out_counts.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  if (raw_scores) op_fetch(d_raw, raw_scores, na);
  FFP_API_END
}

int ffp_op_scrfd_sahi_rows(int device, int n_tiles, int cap, const int32_t* tiles_xyxy, int full_h, int full_w, float conf, float* dets,
                           int32_t* counts, int32_t* out_bad) {
  FFP_API_BEGIN
  FFP_CHECK(tiles_xyxy && dets && counts, FFP_ERR_ARG, "scrfd_sahi_rows: null argument");
  FFP_CHECK(n_tiles >= 1 && n_tiles <= 65536 && cap >= 1 && cap <= (1 << 20) && (long long)n_tiles * cap < (1 << 24) && full_h >= 1 && full_w >= 1, FFP_ERR_ARG,
            "scrfd_sahi_rows: bad sizes");
  if (out_bad) *out_bad = -1;
  ScopedStream cx(device, "scrfd_sahi_rows");
  Level L;
  op_flat_level(L, 1, (long long)n_tiles * cap, cx.st);
  const OpTensor td = op_stage(L, F32, dets, FFP_DET_STRIDE(5));
  DevBuf dc = upload(counts, (size_t)n_tiles), dt = upload(tiles_xyxy, (size_t)n_tiles * 4), de(sizeof(unsigned));
  launch_scrfd_sahi_rows(td.buf.as<float>(), dc.as<int>(), dt.as<int4>(), n_tiles, cap, conf, full_h, full_w, de.as<unsigned>(), cx.st);
  op_finish(cx, {{&td, dets}});
  FFP_HIP(hipMemcpy(counts, dc.p, sizeof(int) * (size_t)n_tiles, hipMemcpyDeviceToHost));
  unsigned bad = SCRFD_NO_BAD_ROW;
  FFP_HIP(hipMemcpy(&bad, de.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (bad != SCRFD_NO_BAD_ROW) {
    if (out_bad) *out_bad = (int32_t)bad;
    FFP_CHECK(false, FFP_ERR_ARG, "scrfd_sahi_rows: tile %d row %d: Box coords [minx, miny, maxx, maxy] cannot be negative", (int)(bad / (unsigned)cap),
              (int)(bad % (unsigned)cap));
  }
  FFP_API_END
}

// ---- single-operator entry points of the image-input kernels (tests/test_gpu_image_input.py) -----------------------------------------
// The frame is H x W x 3 u8 on the host, the items are boxes {x0, y0, x1, y1} of it; their LetterboxImg records come from the functions
// the engines call (det_tile_geometry, rtdetr_tile_records, scrfd_tile_records), so a geometry mistake shows as well. Outputs hold the
// items back to back; every output tensor goes up without contents (all NaN), so a pixel no kernel wrote comes back as NaN.
namespace {

void op_check_frame(const char* what, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes) {
  FFP_CHECK(frame && boxes, FFP_ERR_ARG, "%s: null frame or boxes", what);
  FFP_CHECK(H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && n >= 1 && n <= 4096, FFP_ERR_ARG, "%s: %d boxes of a %d x %d frame", what, n, W, H);
  FFP_CHECK(chan_order == FFP_CHAN_AS_BGR || chan_order == FFP_CHAN_AS_RGB, FFP_ERR_ARG, "%s: chan_order %d", what, chan_order);
}

// the frame on the device; the 256 bytes behind it are 0xFF, so a kernel that used a byte past the frame would not match a reference that never saw one
DevBuf op_upload_frame(const uint8_t* frame, int H, int W) {
  const size_t nb = (size_t)H * W * 3;
  DevBuf b(nb + 256);
  FFP_HIP(hipMemcpy(b.p, frame, nb, hipMemcpyHostToDevice));
  fill_bytes(static_cast<char*>(b.p) + nb, 0xFF, 256);
  return b;
}

std::vector<LetterboxImg> op_det_records(int H, int W, const int32_t* boxes, int n, int imgsz) {
  FFP_CHECK(imgsz > 0, FFP_ERR_ARG, "imgsz %d must be a multiple of 32 in [32,4096]", imgsz);      // (0 would ask det_tile_geometry for the first box's own size)
  const std::vector<TileGeom> g = det_tile_geometry(H, W, boxes, n, imgsz);
  std::vector<LetterboxImg> lb(n);
  for (int i = 0; i < n; ++i) lb[i] = g[i].lb;
  return lb;
}

}  // namespace

int ffp_op_image_input(int device, int kind, int precision, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy,
                       int size_a, int size_b, float* out, int32_t* out_hs, int32_t* out_ws) {
  FFP_API_BEGIN
  FFP_CHECK(out && out_hs && out_ws, FFP_ERR_ARG, "image_input: null output");
  op_check_frame("image_input", frame, H, W, chan_order, n, boxes_xyxy);
  FFP_CHECK(kind >= 0 && kind <= 2, FFP_ERR_ARG, "image_input: kind %d (0 YOLO letterbox, 1 RT-DETR stretch, 2 SCRFD)", kind);
  const DType T = op_dtype("image_input", precision);
  FFP_CHECK(kind != 2 || T == F32, FFP_ERR_ARG, "image_input: the SCRFD pre-processing writes fp32 only");
  std::vector<LetterboxImg> lb;
  std::vector<float> scale;
  if (kind == 0) {
    lb = op_det_records(H, W, boxes_xyxy, n, size_a);
  } else if (kind == 1) {
    FFP_CHECK(size_a >= 32 && size_a % 32 == 0 && size_a <= 4096, FFP_ERR_ARG, "image_input: imgsz %d must be a multiple of 32 in [32, 4096]", size_a);
    rtdetr_tile_records(H, W, boxes_xyxy, n, size_a, lb);
  } else {
    FFP_CHECK(size_a % 32 == 0 && size_b % 32 == 0 && size_a >= 32 && size_b >= 32 && size_a <= 4096 && size_b <= 4096, FFP_ERR_ARG,
              "image_input: det size %dx%d must be multiples of 32 in [32, 4096]", size_a, size_b);
    scrfd_tile_records(size_a, size_b, H, W, boxes_xyxy, n, lb, scale);
  }
  std::vector<int> hs(n), ws(n);
  for (int i = 0; i < n; ++i) { hs[i] = lb[i].net_h; ws[i] = lb[i].net_w; }
  ScopedStream cx(device, "image_input");
  const int cs = T == F16 ? 8 : 4;
  Level L;
  op_level(L, hs.data(), ws.data(), n, cx.st);
  DevBuf d_frame = op_upload_frame(frame, H, W), d_imgs = upload(lb.data(), lb.size());
  const OpTensor tout = op_stage(L, T, nullptr, cs, true);
  const TView vout = tout.view(0, cs);
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  if (kind == 2) launch_scrfd_preproc(d_frame.as<uint8_t>(), W, flip, d_imgs.as<LetterboxImg>(), vout, cx.st);
  else launch_letterbox(d_frame.as<uint8_t>(), H, W, flip, d_imgs, vout, cx.st);
  op_finish(cx, {{&tout, out}});
  std::copy(hs.begin(), hs.end(), out_hs);
  std::copy(ws.begin(), ws.end(), out_ws);
  FFP_API_END
}

int ffp_op_stem(int device, int precision, int fused, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy, int imgsz,
                const float* w, const float* bias, int cout, int stride, int act, float* out) {
  FFP_API_BEGIN
  FFP_CHECK(w && bias && out, FFP_ERR_ARG, "stem: null argument");
  op_check_frame("stem", frame, H, W, chan_order, n, boxes_xyxy);
  FFP_CHECK((fused == 0 || fused == 1) && (cout == 16 || cout == 32 || cout == 64) && (stride == 1 || stride == 2) && act >= ACT_NONE && act <= ACT_RELU,
            FFP_ERR_ARG, "stem: fused %d (0, 1), cout %d (16, 32, 64), stride %d (1, 2), activation code %d (0..3)", fused, cout, stride, act);
  const DType T = op_dtype("stem", precision);
  const std::vector<LetterboxImg> lb = op_det_records(H, W, boxes_xyxy, n, imgsz);
  std::vector<int> hi(n), wi(n);
  for (int i = 0; i < n; ++i) { hi[i] = lb[i].net_h; wi[i] = lb[i].net_w; }
  ScopedStream cx(device, "stem");
  PackedConv pc;
  pack_conv(pc, "op_stem", w, bias, cout, 3, 3, 1, T, cx.st, false);
  Level lin, lout;
  op_level(lin, hi.data(), wi.data(), n, cx.st);
  op_level(lout, hi.data(), wi.data(), n, cx.st, 1, [&](int v) { return op_conv_out(v, 3, stride); });
  const int cin0 = T == F16 ? 8 : 4;
  DevBuf d_frame = op_upload_frame(frame, H, W), d_imgs = upload(lb.data(), lb.size());
  const OpTensor tout = op_stage(lout, T, nullptr, cout, true);
  OpTensor tin;
  if (!fused) tin = op_stage(lin, T, nullptr, cin0, true);
  ConvOp o;
  o.pc = &pc; o.stride = stride; o.act = act;
  o.in = TView{tin.buf.p, T, cin0, 0, cin0, &lin};      // fused: the level and the channel padding only
  o.out = tout.view(0, cout);
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  if (fused) {
    launch_stem_from_frame(d_frame.as<uint8_t>(), H, W, flip, d_imgs, o, cx.st);
  } else {
    launch_letterbox(d_frame.as<uint8_t>(), H, W, flip, d_imgs, o.in, cx.st);
    launch_conv_direct(o, cx.st);
  }
  op_finish(cx, {{&tout, out}});
  FFP_API_END
}

int ffp_op_stem_conv(int device, const uint8_t* frame, int H, int W, int chan_order, int n, const int32_t* boxes_xyxy, int imgsz, const float* stem_w,
                     const float* stem_b, int stem_cout, const float* conv_w, const float* conv_b, float* out) {
  FFP_API_BEGIN
  FFP_CHECK(stem_w && stem_b && conv_w && conv_b && out, FFP_ERR_ARG, "stem_conv: null argument");
  op_check_frame("stem_conv", frame, H, W, chan_order, n, boxes_xyxy);
  FFP_CHECK(stem_cout == 16 || stem_cout == 32, FFP_ERR_ARG, "stem_conv: %d stem channels (16 or 32: the loader holds one or two 16-channel chunks)", stem_cout);
  const std::vector<LetterboxImg> lb = op_det_records(H, W, boxes_xyxy, n, imgsz);
  std::vector<int> h0(n), w0(n);
  for (int i = 0; i < n; ++i) { h0[i] = lb[i].net_h; w0[i] = lb[i].net_w; }
  ScopedStream cx(device, "stem_conv");
  conv_kernels_init();
  const int cc = 2 * stem_cout;
  PackedConv ps, pc;
  pack_conv(ps, "model.0.conv", stem_w, stem_b, stem_cout, 3, 3, 1, F32, cx.st, true);
  pack_conv(pc, "model.1.conv", conv_w, conv_b, cc, stem_cout, 3, 1, F32, cx.st, true);
  // as a split plan lays it out: levels aligned to 32 pixels, one max-|value| slot per (buffer, image); the stem output's slots hold the bound the
  // plan knows from the weights alone, the conv output's start at zero
  Level L0, L1, L2;
  const auto half = [](int v) { return op_conv_out(v, 3, 2); };
  op_level(L0, h0.data(), w0.data(), n, cx.st, 32);
  op_level(L1, h0.data(), w0.data(), n, cx.st, 32, half);
  op_level(L2, h0.data(), w0.data(), n, cx.st, 32, [&](int v) { return half(half(v)); });
  const float bound = std::max(ps.out_bound, 0.3f);
  unsigned bound_bits;
  std::memcpy(&bound_bits, &bound, 4);
  OpSlot s_stem(std::vector<unsigned>(n, bound_bits)), s_conv(std::vector<unsigned>(n, 0u));
  DevBuf d_frame = op_upload_frame(frame, H, W), d_imgs = upload(lb.data(), lb.size()), d_stem_w;
  const OpTensor tout = op_stage(L2, F32, nullptr, cc, true);
  ConvOp stem, conv;
  stem.pc = &ps; stem.stride = 2; stem.act = ACT_SILU;
  stem.in = TView{nullptr, F32, 4, 0, 4, &L0};
  stem.out = TView{nullptr, F32, stem_cout, 0, stem_cout, &L1};      // never stored
  stem.out.amax = s_stem.ptr(); stem.out.amax_n = n;
  conv.pc = &pc; conv.stride = 2; conv.act = ACT_SILU;
  conv.in = stem.out;
  conv.out = tout.view(0, cc, &s_conv);
  FFP_CHECK(stem_conv_eligible(stem, conv), FFP_ERR_ARG, "stem_conv: the stem-fused loader refuses this pair of convs");
  const int flip = chan_order == FFP_CHAN_AS_BGR ? 1 : 0;
  stem_conv_pack(stem, flip, d_stem_w, cx.st);
  launch_stem_conv(d_frame.as<uint8_t>(), H, W, d_imgs, d_stem_w, stem, conv, cx.st);
  op_finish(cx, {{&tout, out}});
  FFP_API_END
}

// tuning hook: average device time (HIP events) of `iters` launches of one dense convolution on synthetic data
int ffp_op_conv2d_time(int device, int precision, int n, int h, int w, int cin, int cout, int k, int stride, int up, int iters,
                       int dbg_mask, int force_shape, float* out_us) {
  FFP_API_BEGIN
  FFP_CHECK(out_us && n > 0 && iters > 0, FFP_ERR_ARG, "bad arguments");
  ScopedStream cx(device, "conv2d_time");
  conv_kernels_init();
  const DType T = precision == FFP_PREC_F16 ? F16 : F32;
  std::vector<float> wt((size_t)cout * cin * k * k), bias(cout, 0.1f);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xFFFF) / 65536.0f - 0.5f; };
  for (auto& v : wt) v = rnd() * 0.1f;
  PackedConv pc;
  pack_conv(pc, "bench", wt.data(), bias.data(), cout, cin, k, 1, T, cx.st, precision == FFP_PREC_F32X3);
  Level lin, lout;
  op_level_same(lin, n, h, w, cx.st);
  op_level_same(lout, n, op_conv_out(up ? h * 2 : h, k, stride), op_conv_out(up ? w * 2 : w, k, stride), cx.st);
  const size_t nin = (size_t)lin.total_px * pc.cin, nout = (size_t)lout.total_px * cout;
  DevBuf din(nin * dsize(T) + 256), dout(nout * dsize(T) + 256);
  {
    std::vector<float> hx(std::min(nin, (size_t)1 << 22));
    for (auto& v : hx) v = rnd();
    std::vector<unsigned char> raw(hx.size() * dsize(T));
    op_narrow(T, hx.data(), hx.size(), raw.data());
    for (size_t o = 0; o < nin; o += hx.size())
      FFP_HIP(hipMemcpy(din.as<char>() + o * dsize(T), raw.data(), std::min(hx.size(), nin - o) * dsize(T), hipMemcpyHostToDevice));
  }
  ConvOp o;
  o.pc = &pc; o.stride = stride; o.act = precision == FFP_PREC_F16 ? ACT_LRELU : ACT_SILU; o.up = up; o.dbg = dbg_mask; o.force_shape = force_shape;   // the activation each precision's network uses
  o.in = TView{din.p, T, pc.cin, 0, pc.cin, &lin};
  o.out = TView{dout.p, T, cout, 0, cout, &lout};
  // SHAPE_TRUNK: the fused-body kernel (conv_trunk.hip) on this ONE layer, its plan built once outside the timed launches
  std::unique_ptr<TrunkPlan> tp;
  if (force_shape == SHAPE_TRUNK) tp.reset(new TrunkPlan(std::vector<ConvOp>{o}));
  auto once = [&]() { if (tp) tp->launch(cx.st, dbg_mask); else launch_conv(o, cx.st); };
  for (int i = 0; i < 3; ++i) once();
  ScopedEvent e0, e1;
  FFP_HIP(hipEventRecord(e0, cx.st));
  for (int i = 0; i < iters; ++i) once();
  FFP_HIP(hipEventRecord(e1, cx.st));
  FFP_HIP(hipStreamSynchronize(cx.st));
  float ms = 0.f;
  FFP_HIP(hipEventElapsedTime(&ms, e0, e1));
  *out_us = ms * 1e3f / iters;
  FFP_API_END
}

int ffp_op_resize_lanczos4(int device, const void* src, int h, int w, int channels, int bits, int out_h, int out_w, void* dst) {
  FFP_API_BEGIN
  FFP_CHECK(src && dst, FFP_ERR_ARG, "resize_lanczos4: null argument");
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, FFP_ERR_ARG, "resize_lanczos4: empty image (%dx%d -> %dx%d)", h, w, out_h, out_w);
  FFP_CHECK(channels == 1 || channels == 3 || channels == 4, FFP_ERR_ARG, "resize_lanczos4: channels %d (1, 3 or 4)", channels);
  FFP_CHECK(bits == 8 || bits == 16, FFP_ERR_ARG, "resize_lanczos4: bits %d (8 or 16)", bits);
  const int wide = bits == 16;
  const size_t in_bytes = ((size_t)h * w * channels) << wide, out_bytes = ((size_t)out_h * out_w * channels) << wide;
  if (out_h == h && out_w == w) {     // cv::resize of the same size is a copy
    std::memcpy(dst, src, out_bytes);
    return FFP_OK;
  }
  std::vector<uint8_t> host_tab;      // uploaded asynchronously: it outlives the stream
  ScopedStream cx(device, "resize_lanczos4");
  DevBuf din(in_bytes), dout(out_bytes), tab;
  FFP_HIP(hipMemcpyAsync(din.p, src, in_bytes, hipMemcpyHostToDevice, cx.st));
  resize_lanczos4_dev(din.p, h, w, channels, wide, out_h, out_w, dout.p, tab, host_tab, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(dst, dout.p, out_bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

}  // extern "C"

// ---- single-operator entry points of the Real-ESRGAN pre/post kernels (tests/test_gpu_sr_ops.py) --------------------------------------
// An image is eight int64: byte offset and row stride inside the caller's buffer, h, w (the INPUT size: a canvas is scale times as large), channels,
// bits, range, selection. The tiles and the descriptor tables come from the functions the engine calls (sr_tiles.hpp), the levels from Level::build
// or — capacity mode — Level::reserve / assign with the capacities SrEngine::build_plan gives them. No weights, no plan.
namespace {

constexpr int kSrImgFields = 8;

SrFmt op_sr_fmt(const char* what, int i, const int64_t* d) {
  const int64_t cn = d[4], bits = d[5], range = d[6], sel = d[7];
  FFP_CHECK(cn == 1 || cn == 3 || cn == 4, FFP_ERR_ARG, "%s: image %d has %lld channels (1, 3 or 4)", what, i, (long long)cn);
  FFP_CHECK(bits == 8 || bits == 16, FFP_ERR_ARG, "%s: image %d has %lld bits (8 or 16)", what, i, (long long)bits);
  FFP_CHECK(range == 255 || (range == 65535 && bits == 16), FFP_ERR_ARG, "%s: image %d has range %lld in %lld-bit storage", what, i, (long long)range, (long long)bits);
  FFP_CHECK((sel == SR_SEL_BGR && cn >= 3) || sel == SR_SEL_GRAY || (sel == SR_SEL_ALPHA && cn == 4), FFP_ERR_ARG, "%s: image %d selects %lld of %lld channels", what, i,
            (long long)sel, (long long)cn);
  SrFmt f;
  f.cn = (int)cn; f.wide = bits == 16; f.range = (float)range; f.sel = (int)sel;
  return f;
}

// the images of one batch; canvas = false: the descriptions are sources of sr_pre, true: canvases of sr_post. Every byte a kernel may touch lies in [0, bytes).
std::vector<SrImage> op_sr_images(const char* what, int n, const int64_t* imgs, int scale, bool canvas, size_t bytes) {
  FFP_CHECK(imgs && n >= 1 && n <= 256, FFP_ERR_ARG, "%s: %d images", what, n);
  std::vector<SrImage> v(n);
  for (int i = 0; i < n; ++i) {
    const int64_t* d = imgs + (size_t)i * kSrImgFields;
    const SrFmt f = op_sr_fmt(what, i, d);
    const int64_t off = d[0], stride = d[1], h = d[2], w = d[3];
    FFP_CHECK(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, FFP_ERR_ARG, "%s: image %d is %lldx%lld", what, i, (long long)w, (long long)h);
    const int64_t k = canvas ? scale : 1, row = w * k * f.px_bytes(), es = 1 << f.wide;
    FFP_CHECK(off >= 0 && stride >= row && stride <= (1 << 24) && off % es == 0 && stride % es == 0, FFP_ERR_ARG, "%s: image %d at offset %lld with rows of %lld bytes (%lld used)",
              what, i, (long long)off, (long long)stride, (long long)row);
    FFP_CHECK((uint64_t)(off + (h * k - 1) * stride + row) <= bytes, FFP_ERR_ARG, "%s: image %d ends behind the buffer of %zu bytes", what, i, bytes);
    SrImage& im = v[i];
    im = SrImage{};
    im.h = (int)h; im.w = (int)w;
    if (canvas) { im.out_off = off; im.out_stride = (int)stride; im.out_fmt = f; }
    else { im.in_off = off; im.in_stride = (int)stride; im.in_fmt = f; }
  }
  return v;
}

void op_sr_scale(const char* what, int scale) { FFP_CHECK(scale == 4 || scale == 2, FFP_ERR_ARG, "%s: scale %d (no kernel: 4 or 2)", what, scale); }

// the network's input record of a (precision, scale) pair: conv_first's padded input channels, as SrEngine::build_plan takes them from the packed conv
int op_sr_in_channels(DType T, int scale) { return conv_cin_aligned(3 * sr_shuffle(scale) * sr_shuffle(scale), T); }

// One level the way the engine has it: exact (cap_t16 == 0) or reserved for cap_t16 body tiles of 16x16, `up` = 1 (body) or 4 (the x4 level).
struct OpSrLevel {
  Level L;
  int cap_t16;
  OpSrLevel(int cap, int up) : cap_t16(cap) {
    if (cap > 0) L.reserve(cap, 256ll * up * up * cap, up * up * cap, nullptr);
  }
  void set(const std::vector<int>& hs, const std::vector<int>& ws, hipStream_t st) {
    if (cap_t16 > 0) L.assign(hs, ws, st);
    else L.build(hs, ws, st);
  }
};

void op_sr_check_cap(const char* what, int cap_t16, const SrLevelSizes& z) {
  FFP_CHECK(cap_t16 >= 0 && cap_t16 <= 4096, FFP_ERR_ARG, "%s: capacity %d", what, cap_t16);
  FFP_CHECK(cap_t16 == 0 || z.t16 <= cap_t16, FFP_ERR_ARG, "%s: batch of %lld 16x16 tiles exceeds the capacity of %d", what, z.t16, cap_t16);
}

}  // namespace

extern "C" {

int ffp_op_sr_tiles(int n, const int64_t* imgs, int scale, int tile, int tile_pad, int pre_pad, int precision, int cap_tiles, int32_t* out_hw,
                    int32_t* out_n, int32_t* out_t16, int32_t* out_channels) {
  FFP_API_BEGIN
  FFP_CHECK(imgs && out_hw && out_n && out_t16 && out_channels && cap_tiles >= 0, FFP_ERR_ARG, "sr_tiles: null argument");
  op_sr_scale("sr_tiles", scale);
  const DType T = op_dtype("sr_tiles", precision);
  const std::vector<SrImage> v = op_sr_images("sr_tiles", n, imgs, 1, false, SIZE_MAX);
  const std::vector<SrTile> tiles = sr_tiles_checked(v, scale, tile, tile_pad, pre_pad);
  FFP_CHECK((int)tiles.size() <= cap_tiles, FFP_ERR_ARG, "sr_tiles: %d tiles, room for %d", (int)tiles.size(), cap_tiles);
  for (size_t i = 0; i < tiles.size(); ++i) { out_hw[2 * i] = tiles[i].h; out_hw[2 * i + 1] = tiles[i].w; }
  *out_n = (int32_t)tiles.size();
  *out_t16 = (int32_t)sr_level_sizes(tiles, scale).t16;
  *out_channels = op_sr_in_channels(T, scale);
  FFP_API_END
}

int ffp_op_sr_pre(int device, int precision, const uint8_t* src, size_t src_bytes, int n, const int64_t* imgs, int scale, int tile, int tile_pad,
                  int pre_pad, int cap_t16, int n_first, const int64_t* imgs_first, float* flat, size_t flat_px, int64_t* out_off) {
  FFP_API_BEGIN
  FFP_CHECK(src && flat && out_off && src_bytes > 0, FFP_ERR_ARG, "sr_pre: null argument");
  FFP_CHECK(n_first == 0 || (n_first > 0 && imgs_first && cap_t16 > 0), FFP_ERR_ARG, "sr_pre: an earlier batch needs a capacity-mode level");
  op_sr_scale("sr_pre", scale);
  const DType T = op_dtype("sr_pre", precision);
  const int C = op_sr_in_channels(T, scale), shuf = sr_shuffle(scale);
  std::vector<std::vector<SrTile>> batches;
  if (n_first > 0) batches.push_back(sr_tiles_checked(op_sr_images("sr_pre", n_first, imgs_first, scale, false, src_bytes), scale, tile, tile_pad, pre_pad));
  batches.push_back(sr_tiles_checked(op_sr_images("sr_pre", n, imgs, scale, false, src_bytes), scale, tile, tile_pad, pre_pad));
  std::vector<SrLevelSizes> sizes;
  for (const auto& b : batches) {
    sizes.push_back(sr_level_sizes(b, scale));
    op_sr_check_cap("sr_pre", cap_t16, sizes.back());
  }
  long long px = 0;
  for (size_t i = 0; i < batches.back().size(); ++i) px += (long long)sizes.back().hs[i] * sizes.back().ws[i];
  const long long want_px = cap_t16 > 0 ? 256ll * cap_t16 : px;
  FFP_CHECK((long long)flat_px == want_px, FFP_ERR_ARG, "sr_pre: the level holds %lld pixel records, the buffer %zu", want_px, flat_px);
  ScopedStream cx(device, "sr_pre");
  OpSrLevel lb(cap_t16, 1);
  // the caller's contents go up once, every record of the level: a later batch runs over what the earlier one left
  DevBuf d_src = upload(src, src_bytes), d_flat = op_put(T, flat, flat_px * C, kOpSlack), d_srcs;      // the level's whole flat buffer, padding and unused capacity included
  for (size_t b = 0; b < batches.size(); ++b) {
    const std::vector<SrTile>& tiles = batches[b];
    const int nt = (int)tiles.size(), cap = cap_t16 > 0 ? cap_t16 : nt;
    FFP_HIP(hipStreamSynchronize(cx.st));      // the earlier batch has read its tables
    lb.set(sizes[b].hs, sizes[b].ws, cx.st);
    std::vector<SrSrc> srcs(nt);
    std::vector<SrDst> dsts(cap);
    std::vector<long long> coff((size_t)cap + 1);
    sr_fill_descriptors(tiles, cap, srcs.data(), dsts.data(), coff.data());
    d_srcs = upload(srcs.data(), srcs.size());
    const TView vout{d_flat.p, T, C, 0, C, &lb.L};
    launch_sr_pre(d_src.as<uint8_t>(), d_srcs.as<SrSrc>(), vout, shuf, cx.st);
  }
  FFP_HIP(hipStreamSynchronize(cx.st));
  op_get(T, d_flat, flat_px * C, flat);
  for (size_t i = 0; i < batches.back().size(); ++i) out_off[i] = lb.L.off[i];
  FFP_API_END
}

int ffp_op_sr_post(int device, int n, const int64_t* imgs, int scale, int tile, int tile_pad, int pre_pad, const float* net, int cs, int cap_t16,
                   int n_first, const int64_t* imgs_first, const float* net_first, int only_tile, uint8_t* canvas, size_t canvas_bytes) {
  FFP_API_BEGIN
  FFP_CHECK(net && canvas && canvas_bytes > 0, FFP_ERR_ARG, "sr_post: null argument");
  FFP_CHECK(cs >= 3 && cs <= 64, FFP_ERR_ARG, "sr_post: network output records of %d channels", cs);
  FFP_CHECK(n_first == 0 || (n_first > 0 && imgs_first && net_first && cap_t16 > 0), FFP_ERR_ARG, "sr_post: an earlier batch needs a capacity-mode level");
  op_sr_scale("sr_post", scale);
  std::vector<std::vector<SrTile>> batches;
  std::vector<const float*> nets;
  if (n_first > 0) {
    batches.push_back(sr_tiles_checked(op_sr_images("sr_post", n_first, imgs_first, scale, true, canvas_bytes), scale, tile, tile_pad, pre_pad));
    nets.push_back(net_first);
  }
  batches.push_back(sr_tiles_checked(op_sr_images("sr_post", n, imgs, scale, true, canvas_bytes), scale, tile, tile_pad, pre_pad));
  nets.push_back(net);
  std::vector<SrLevelSizes> sizes;
  for (const auto& b : batches) {
    sizes.push_back(sr_level_sizes(b, scale));
    op_sr_check_cap("sr_post", cap_t16, sizes.back());
  }
  FFP_CHECK(only_tile >= -1 && only_tile < (int)batches.back().size(), FFP_ERR_ARG, "sr_post: tile %d of %d", only_tile, (int)batches.back().size());
  ScopedStream cx(device, "sr_post");
  OpSrLevel l2(cap_t16, 4);
  DevBuf d_canvas = upload(canvas, canvas_bytes), d_dsts, d_coff;
  OpTensor t_net;
  for (size_t b = 0; b < batches.size(); ++b) {
    const std::vector<SrTile>& tiles = batches[b];
    const int nt = (int)tiles.size(), cap = cap_t16 > 0 ? cap_t16 : nt;
    FFP_HIP(hipStreamSynchronize(cx.st));      // the earlier batch has read its tables and its network output
    l2.set(sizes[b].h2, sizes[b].w2, cx.st);
    t_net = op_stage(l2.L, F32, nets[b], cs);      // NaN behind the batch's last pixel
    std::vector<SrSrc> srcs(nt);
    std::vector<SrDst> dsts(cap);
    std::vector<long long> coff((size_t)cap + 1);
    sr_fill_descriptors(tiles, cap, srcs.data(), dsts.data(), coff.data());
    if (only_tile >= 0 && b + 1 == batches.size()) {      // every other core emptied: what this tile writes is not covered by its neighbours
      long long tot = 0;
      for (int i = 0; i < cap; ++i) {
        if (i != only_tile) dsts[i].cw = dsts[i].ch = 0;
        coff[i] = tot;
        tot += (long long)dsts[i].cw * dsts[i].ch;
      }
      coff[cap] = tot;
    }
    d_dsts = upload(dsts.data(), dsts.size());
    d_coff = upload(coff.data(), coff.size());
    launch_sr_post(t_net.view(0, cs), d_dsts.as<SrDst>(), d_coff.as<long long>(), l2.L.total_px, d_canvas.as<uint8_t>(), cx.st);      // as SrEngine::enhance_dev launches it
  }
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(canvas, d_canvas.p, canvas_bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_op_alpha_linear(int device, const void* src, int h, int w, int src_bits, int range, int out_h, int out_w, int dst_bits, void* dst) {
  FFP_API_BEGIN
  FFP_CHECK(src && dst, FFP_ERR_ARG, "alpha_linear: null argument");
  FFP_CHECK(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1 && h <= 8192 && w <= 8192 && out_h <= 8192 && out_w <= 8192, FFP_ERR_ARG,
            "alpha_linear: %dx%d -> %dx%d", h, w, out_h, out_w);
  FFP_CHECK((src_bits == 8 || src_bits == 16) && (dst_bits == 8 || dst_bits == 16), FFP_ERR_ARG, "alpha_linear: bits %d -> %d (8 or 16)", src_bits, dst_bits);
  FFP_CHECK(src_bits == 16 || dst_bits == 8, FFP_ERR_ARG, "alpha_linear: 8-bit input with a 16-bit canvas");
  FFP_CHECK(range == 255 || (range == 65535 && src_bits == 16 && dst_bits == 16), FFP_ERR_ARG, "alpha_linear: range %d in %d-bit -> %d-bit storage", range, src_bits, dst_bits);
  const size_t in_bytes = ((size_t)h * w * 4) << (src_bits == 16), out_bytes = ((size_t)out_h * out_w * 4) << (dst_bits == 16);
  ScopedStream cx(device, "alpha_linear");
  DevBuf d_src = upload(static_cast<const uint8_t*>(src), in_bytes), d_dst = upload(static_cast<const uint8_t*>(dst), out_bytes);
  launch_alpha_linear(d_src.p, h, w, src_bits == 16, (float)range, out_h, out_w, d_dst.p, dst_bits == 16, cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(dst, d_dst.p, out_bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

int ffp_op_crop_gather(int device, const uint8_t* frame, int H, int W, int n, const int32_t* boxes_xywh, const int64_t* offs, uint8_t* out,
                       size_t out_bytes) {
  FFP_API_BEGIN
  FFP_CHECK(frame && out && out_bytes > 0 && (n == 0 || (boxes_xywh && offs)), FFP_ERR_ARG, "crop_gather: null argument");
  FFP_CHECK(H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && n >= 0 && n <= 4096, FFP_ERR_ARG, "crop_gather: %d boxes of a %d x %d frame", n, W, H);
  std::vector<int4> hb(n);
  std::vector<long long> ho(n);
  for (int i = 0; i < n; ++i) {
    const int x0 = boxes_xywh[4 * i], y0 = boxes_xywh[4 * i + 1], w = boxes_xywh[4 * i + 2], h = boxes_xywh[4 * i + 3];
    FFP_CHECK(x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && w <= W - x0 && h <= H - y0, FFP_ERR_ARG, "crop_gather: box %d (%d, %d, %dx%d) leaves the frame", i, x0, y0, w, h);
    FFP_CHECK(offs[i] >= 0 && (uint64_t)offs[i] + (uint64_t)w * h * 3 <= out_bytes, FFP_ERR_ARG, "crop_gather: box %d ends behind the output of %zu bytes", i, out_bytes);
    hb[i] = make_int4(x0, y0, w, h);
    ho[i] = offs[i];
  }
  ScopedStream cx(device, "crop_gather");
  DevBuf d_frame = op_upload_frame(frame, H, W), d_out = upload(out, out_bytes), d_boxes = upload(hb.data(), hb.size()), d_offs = upload(ho.data(), ho.size());
  launch_crop_gather(d_frame.as<uint8_t>(), W, d_boxes.as<int4>(), d_offs.as<long long>(), n, d_out.as<uint8_t>(), cx.st);
  FFP_HIP(hipStreamSynchronize(cx.st));
  FFP_HIP(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
  FFP_API_END
}

}  // extern "C"
