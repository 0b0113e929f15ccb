// conv_route.cpp — the table of shape numbers and the one decision of which kernel runs a ConvOp (see conv_route.hpp).
#include "conv_route.hpp"

#include <algorithm>

#include "api_util.hpp"
#include "conv_args.hpp"
#include "engine.hpp"
#include "trunk.hpp"

namespace ffp {

namespace {

using F = ConvFamily;
constexpr ConvShapeInfo kShapes[SHAPE_COUNT] = {
    {SHAPE_WIDE, F::GENERIC, "generic", "wide"},         {SHAPE_WIDE_H, F::GENERIC, "generic", "wideH"},
    {SHAPE_NARROW2, F::GENERIC, "generic", "narrow2"},   {SHAPE_NARROW2_H, F::GENERIC, "generic", "narrow2H"},
    {SHAPE_NARROW1, F::GENERIC, "generic", "narrow1"},   {SHAPE_NARROW1_H, F::GENERIC, "generic", "narrow1H"},
    {SHAPE_ROWS, F::ROWS, "rows", "rows"},               {SHAPE_ROWS_3STAGE, F::ROWS, "rows", "rows"},
    {SHAPE_ROWS_2TILE, F::ROWS, "rows", "rows"},         {SHAPE_ROWS16, F::ROWS16, "rows16", "rows16"},
    {SHAPE_PW_1X4, F::PW, "pw", "pw1x4"},                {SHAPE_PW_2X2, F::PW, "pw", "pw2x2"},
    {SHAPE_PW_2X1, F::PW, "pw", "pw2x1"},                {SHAPE_PW_1X4W, F::PW, "pw", "pw1x4w"},
    {SHAPE_PW_2X2W, F::PW, "pw", "pw2x2w"},              {SHAPE_PW_2X1W, F::PW, "pw", "pw2x1w"},
    {SHAPE_PW_1X4S, F::PW, "pw", "pw1x4s"},              {SHAPE_K3D_128, F::K3D, "k3d", "d128"},
    {SHAPE_K3D_64, F::K3D, "k3d", "d64"},                {SHAPE_K3D_32, F::K3D, "k3d", "d32"},
    {SHAPE_K3D_128X256, F::K3D, "k3d", "d128x256"},      {SHAPE_K3D_64X256, F::K3D, "k3d", "d64x256"},
    {SHAPE_PW_2X2S, F::PW, "pw", "pw2x2s"},              {SHAPE_ROWS16_RES, F::ROWS16, "rows16", "rows16"},
    {SHAPE_ROWS16PC, F::ROWS16PC, "rows16pc", "rows16pc"}, {SHAPE_TRUNK, F::TRUNK, "trunk", "trunk"},
};
constexpr ConvShapeInfo kDwPw{SHAPE_DWPW, F::DWPW, "dwpw", "dw3"};
constexpr bool table_in_order() {
  for (int i = 0; i < SHAPE_COUNT; ++i) if (kShapes[i].shape != i) return false;
  return true;
}
static_assert(table_in_order(), "conv shape table: row i holds shape i");
static_assert(SHAPE_COUNT <= 32 && SHAPE_DWPW >= 32, "forceable shapes fit a 32-bit candidate mask; route-only numbers lie above them");

// can `family` run the op at `shape` (a number of that family)
bool family_runs(ConvFamily family, int shape, const ConvOp& op, const ConvArgs& a) {
  switch (family) {
    case F::GENERIC: return true;      // any generic shape launches its Cfg; one whose stage does not fit the LDS is the launcher's FFP_ERR_STATE
    case F::ROWS: return conv_rows_eligible(op, a, shape);
    case F::ROWS16:
    case F::ROWS16PC: return conv_rows16_eligible(op, a, shape);
    case F::PW: return conv_pw_mask(op, a) & shape_bit(shape);
    case F::K3D: return conv_k3d_mask(op, a) & shape_bit(shape);
    case F::TRUNK: return conv_trunk_layer_ok(op);
    case F::DWPW: return conv_dwpw_eligible(op);
    case F::DIRECT: break;
  }
  return false;
}

}  // namespace

const ConvShapeInfo* conv_shape_info(int shape) {
  if (shape < 0 || shape >= SHAPE_COUNT) return nullptr;
  return &kShapes[shape];
}

const ConvShapeInfo* conv_route_info(int shape) { return shape == SHAPE_DWPW ? &kDwPw : conv_shape_info(shape); }

ConvArgs conv_route_args(const ConvOp& op) { return op.dw || conv_direct_eligible(op) ? ConvArgs{} : make_conv_args(op); }      // the depthwise-fused launcher builds its own block

ConvRoute conv_route(const ConvOp& op, const ConvArgs& a) {
  if (op.dw) {      // one kernel, one shape: nothing else computes the depthwise conv on the way in
    FFP_CHECK((op.force_shape < 0 || op.force_shape == SHAPE_DWPW) && conv_dwpw_eligible(op), FFP_ERR_ARG, "conv %s: the depthwise-fused kernel cannot run this op", op.pc->name.c_str());
    return {F::DWPW, SHAPE_DWPW};
  }
  if (conv_direct_eligible(op)) {      // the flat-pixel VALU kernel knows no gate: a gated image-input conv is refused, not computed on every image
    FFP_CHECK(!op.gate, FFP_ERR_ARG, "conv %s: the image-input kernel cannot honour a gate", op.pc->name.c_str());
    return {F::DIRECT, SHAPE_AUTO};
  }
  if (op.force_shape >= 0) {
    const ConvShapeInfo* s = conv_shape_info(op.force_shape);
    FFP_CHECK(s, FFP_ERR_ARG, "conv %s: %d is not a shape number", op.pc->name.c_str(), op.force_shape);
    FFP_CHECK(family_runs(s->family, s->shape, op, a), FFP_ERR_ARG, "conv %s: %s shape %d cannot run this op", op.pc->name.c_str(), s->family_name, s->shape);
    return {s->family, s->shape};
  }
  if (sw().rows16 && conv_rows16_eligible(op, a, SHAPE_ROWS16)) {
    if (sw().rows16_pc && a.dbg == 0) return {F::ROWS16PC, SHAPE_ROWS16PC};
    if (sw().rows16_res && conv_rows16_eligible(op, a, SHAPE_ROWS16_RES)) return {F::ROWS16, SHAPE_ROWS16_RES};
    return {F::ROWS16, SHAPE_ROWS16};
  }
  if (conv_rows_eligible(op, a, SHAPE_ROWS)) return {F::ROWS, SHAPE_ROWS};
  return {F::GENERIC, conv_generic_choose(op, a)};
}

unsigned conv_candidates(const ConvOp& op, const ConvArgs& a) {
  return conv_generic_mask(op, a) | (sw().pw ? conv_pw_mask(op, a) : 0u) | (sw().k3d ? conv_k3d_mask(op, a) : 0u);
}

void launch_conv(const ConvOp& op, hipStream_t st) {
  ConvArgs a = conv_route_args(op);
  const ConvRoute r = conv_route(op, a);
  switch (r.family) {
    case F::DIRECT: launch_conv_direct(op, st); return;
    case F::GENERIC: launch_conv_generic(a, r.shape, op, st); break;
    case F::ROWS: launch_conv_rows(a, r.shape, op.out.lvl, st); break;
    case F::ROWS16: launch_conv_rows16(a, r.shape, *op.pc, op.out.lvl, st); break;
    case F::ROWS16PC: launch_conv_rows16pc(a, *op.pc, op.out.lvl, st); break;
    case F::PW: launch_conv_pw(a, r.shape, st); break;
    case F::K3D: launch_conv_k3d(a, r.shape, op.stride, op.out.lvl, st); break;
    case F::DWPW: launch_conv_dwpw(op, st); break;
    case F::TRUNK: {                               // the fused-body kernel on ONE layer (tests, probes): a throw-away single-layer plan
      TrunkPlan tp(std::vector<ConvOp>{op});
      tp.launch(st, op.dbg);
      FFP_HIP(hipStreamSynchronize(st));           // the plan's tables die with it
      return;
    }
  }
  FFP_HIP(hipGetLastError());
}

std::string conv_variant(const ConvOp& op) {
  const PackedConv& pc = *op.pc;
  const ConvRoute r = conv_route(op, conv_route_args(op));
  if (r.family == F::DIRECT) return std::string(pc.dt == F32 ? "f32" : "f16") + "_k3_direct";
  char buf[64];
  snprintf(buf, sizeof(buf), "%s_k%ds%d_%s", pc.dt == F16 ? "f16" : pc.split ? "f32x3" : "f32", pc.k, op.stride, conv_route_info(r.shape)->suffix);
  return buf;
}

int conv_tune(const ConvOp& op, hipStream_t st) {
  const PackedConv& pc = *op.pc;
  const ConvArgs a = conv_route_args(op);
  const ConvRoute r = conv_route(op, a);
  if (op.force_shape >= 0 || r.family != F::GENERIC) return -1;
  const unsigned mask = conv_candidates(op, a);
  if (__builtin_popcount(mask) < 2) return -1;
  const int heur = r.shape;
  ScopedEvent e0, e1;
  auto time_shape = [&](int shape, int iters) {
    ConvOp o = op;
    o.force_shape = shape;
    o.gate = nullptr;                      // shapes are chosen on the whole batch
    FFP_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) launch_conv(o, st);
    FFP_HIP(hipEventRecord(e1, st));
    FFP_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FFP_HIP(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e3f / iters;
  };
  float best_t = 0.f, heur_t = 0.f;
  int best = -1;
  for (int shape = 0; shape < SHAPE_COUNT; ++shape) {
    if (!(mask & shape_bit(shape))) continue;
    const float t1 = time_shape(shape, 2);                              // also builds the shape's tile table
    const int iters = std::min(24, std::max(3, (int)(300.f / std::max(t1, 1.f))));
    const float t = time_shape(shape, iters);
    if (shape == heur) heur_t = t;
    if (best < 0 || t < best_t) { best = shape; best_t = t; }
    if (sw().tune_log) {      // every candidate's time, one line per (layer, shape)
      ConvOp o = op;
      o.force_shape = shape;
      fprintf(stderr, "[tune] %-28s %4d->%4d k%d s%d px %9lld  shape %2d %-22s %9.1f us%s\n", pc.name.c_str(), pc.cin_real, pc.cout, pc.k, op.stride,
              (long long)op.out.lvl->actual_px(), shape, conv_variant(o).c_str(), t, shape == heur ? "  (heuristic)" : "");
    }
  }
  // keep the heuristic's choice unless another shape is clearly (> 3 %) faster: timing noise must not flip plans
  if (heur_t > 0.f && best_t > 0.97f * heur_t) return heur;
  return best;
}

}  // namespace ffp
