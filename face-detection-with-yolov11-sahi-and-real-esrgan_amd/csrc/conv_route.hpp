// conv_route.hpp — which kernel runs a ConvOp: the shape numbers by name, the table of their families and variant suffixes, and the one
// decision (conv_route.cpp) that launch_conv, conv_variant and conv_tune all go through.
#pragma once
#include "ops.hpp"

namespace ffp {

struct ConvArgs;

// ConvOp::force_shape. The values are ABI: ffp_op_conv2d_shape, ffp_op_conv2d_time, the probes under tools/, tests/golden/make_rows16_pins.py.
enum ConvShape : int {
  SHAPE_AUTO = -1,
  SHAPE_WIDE = 0, SHAPE_WIDE_H, SHAPE_NARROW2, SHAPE_NARROW2_H, SHAPE_NARROW1, SHAPE_NARROW1_H,      // conv_mfma_kernel: {128, 64, 32 channels} x {full, half pixel tile}
  SHAPE_ROWS = 6, SHAPE_ROWS_3STAGE, SHAPE_ROWS_2TILE,                                               // conv_rows_kernel <1, 2>, <1, 3>, <2, 2>
  SHAPE_ROWS16 = 9,                                                                                  // conv_rows16_kernel, weights streamed
  SHAPE_PW_1X4 = 10, SHAPE_PW_2X2, SHAPE_PW_2X1, SHAPE_PW_1X4W, SHAPE_PW_2X2W, SHAPE_PW_2X1W,        // conv_pw_kernel: pixel fragments x channel tiles per wave, 4 / 8 (W) waves
  SHAPE_PW_1X4S = 16,                                                                                // ... with a weight-producer wave
  SHAPE_K3D_128 = 17, SHAPE_K3D_64, SHAPE_K3D_32, SHAPE_K3D_128X256, SHAPE_K3D_64X256,               // conv_k3d_kernel: channels [x pixels] per workgroup
  SHAPE_PW_2X2S = 22,
  SHAPE_ROWS16_RES = 23,                                                                             // conv_rows16_kernel, weights resident in LDS
  SHAPE_ROWS16PC = 24,                                                                               // conv_rows16pc_kernel
  SHAPE_TRUNK = 25,                                                                                  // conv_trunk_kernel on one layer
  SHAPE_COUNT,                                                                                       // the numbers above: what ConvOp::force_shape and ffp_op_conv2d_shape take
  SHAPE_DWPW = 64                                                                                    // conv_dwpw_kernel: only ever the route of an op with ConvOp::dw set, never forced onto another; 64: out of reach of the numbers appended above (static_assert in conv_route.cpp)
};
constexpr unsigned shape_bit(int shape) { return 1u << shape; }      // candidate masks: bit s = shape s

enum class ConvFamily { DIRECT, GENERIC, ROWS, ROWS16, ROWS16PC, PW, K3D, TRUNK, DWPW };

// One row per shape number. A step's variant string is "<precision>_k<k>s<stride>_<suffix>" (conv_variant): bench.py parses it and
// profiles/*pmc_traffic.json is keyed by it, so 6 / 7 / 8 all say "rows" and 9 / 23 both say "rows16", as they always have.
struct ConvShapeInfo { int shape; ConvFamily family; const char* family_name; const char* suffix; };
const ConvShapeInfo* conv_shape_info(int shape);      // nullptr: not a shape number an op can be forced to (0 .. SHAPE_COUNT - 1)
const ConvShapeInfo* conv_route_info(int shape);      // ... and SHAPE_DWPW: every number conv_route returns

// The kernel that runs `op`, and the shape number it runs at (DIRECT: SHAPE_AUTO, the image-input kernel has one shape).
//   op.dw set: the depthwise-fused 1x1 kernel (SHAPE_DWPW) or FFP_ERR_ARG; the plan asks conv_dwpw_eligible before it builds such an op.
//   force_shape < 0: direct -> rows16 (rows16pc / its resident form by switch) -> rows -> the generic kernel at its heuristic's shape.
//     pw and k3d shapes are only ever picked by measurement: conv_candidates() offers them to conv_tune.
//   force_shape >= 0: that shape's family at that shape, or FFP_ERR_ARG when the number is no shape or the family cannot run the op; only
//     direct-eligible ops ignore the number. Nothing falls through to another family.
// Environment, read here and nowhere else: FFP_ROWS16=0 (no rows16), FFP_ROWS16_RES=1 (resident form where it fits), FFP_ROWS16_PC=1
// (rows16pc for ops without a phase-skip mask), FFP_PW=0 / FFP_K3D=0 (keep those shapes from the tuner).
struct ConvRoute { ConvFamily family; int shape; };
ConvRoute conv_route(const ConvOp& op, const ConvArgs& a);
ConvArgs conv_route_args(const ConvOp& op);      // make_conv_args(op); direct-eligible ops have no MFMA argument block and get an empty one
// shapes conv_tune times, in increasing number, for an op the automatic route gives to the generic kernel (the other routes have nothing to tune)
unsigned conv_candidates(const ConvOp& op, const ConvArgs& a);

}  // namespace ffp
