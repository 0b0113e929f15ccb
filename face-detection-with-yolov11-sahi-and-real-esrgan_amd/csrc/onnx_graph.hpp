// onnx_graph.hpp — a reader of ONNX ModelProto bytes (protobuf wire format, no onnx / protobuf library) and the lowering of an
// SCRFD face detector (InsightFace det_*.onnx) to a list of steps the engine (scrfd.cpp) lays out as a plan.
// Host code only: no device calls, so the host sanitizer driver (asan_host_check.cpp) links it.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace ffp {
namespace onnx {

enum DataType : int { DT_FLOAT = 1, DT_INT32 = 6, DT_INT64 = 7, DT_DOUBLE = 11 };

struct Tensor {
  std::string name;
  int dtype = 0;
  std::vector<int64_t> dims;
  std::vector<float> f;        // DT_FLOAT / DT_DOUBLE
  std::vector<int64_t> i;      // DT_INT64 / DT_INT32
  bool external = false;       // data_location EXTERNAL or external_data entries: refused by the lowering
  size_t numel() const { size_t n = 1; for (int64_t d : dims) n *= (size_t)d; return n; }
};

struct Attr {
  std::string name;
  int type = 0;
  float f = 0.f;
  int64_t i = 0;
  std::string s;
  std::vector<float> floats;
  std::vector<int64_t> ints;
  bool has_t = false;
  Tensor t;
};

struct Node {
  std::string name, op;
  std::vector<std::string> in, out;
  std::vector<Attr> attrs;
  const Attr* attr(const char* n) const {
    for (const Attr& a : attrs) if (a.name == n) return &a;
    return nullptr;
  }
};

struct ValueInfo {
  std::string name;
  std::vector<int64_t> dims;   // -1: symbolic or absent
};

struct Graph {
  std::vector<Node> nodes;
  std::map<std::string, Tensor> init;
  std::vector<ValueInfo> inputs, outputs;
};

// Parses ModelProto bytes; malformed input raises ffp::Error(FFP_ERR_ARG) and never reads outside [p, p + n).
Graph parse(const void* p, size_t n);

// ---- lowering -----------------------------------------------------------------------------------------------------------
enum StepKind : int { ST_CONV = 0, ST_MAXPOOL = 1, ST_AVGPOOL = 2, ST_UP2 = 3 };

struct LBuf { int C = 0, stride = 1; };     // NHWC storage of C channels at 1/stride of the network size
struct LView { int buf = -1, coff = 0, C = 0; };

struct LStep {
  int kind = ST_CONV;
  std::string node;                 // name of the ONNX node the step came from (its last fused node for a conv)
  LView in, out, res;               // res.buf >= 0: residual added in the epilogue
  int k = 1, stride = 1;
  int act = 0, act_post = 0;        // Act codes (common.hpp): before / after the residual
  int cin = 0, cout = 0;
  std::vector<float> w, b;          // conv: OIHW fp32 with BatchNormalization and scalar Mul folded in, bias (zeros when absent)
  std::vector<std::string> fused;   // ONNX nodes folded into this step (BatchNormalization, Mul, Add, Relu)
  bool ceil_mode = false;           // avgpool
};

struct LOutput { LView v; int stride = 0; int kind = 0; /* 0 score, 1 bbox, 2 kps */ bool sigmoid = false; std::string name; };

struct Lowered {
  int n = 1, det_w = 0, det_h = 0;
  int input_buf = -1;
  std::vector<LBuf> bufs;
  std::vector<LStep> steps;
  std::vector<LOutput> outs;        // the graph outputs in file order
  int fmc = 3, num_anchors = 2;
  bool use_kps = true;
  int strides[3] = {8, 16, 32};
  double conv_flops() const;        // 2 * MAC of every conv over the whole batch
  std::string describe() const;
};

// det_w / det_h: the requested network size; a graph input with fixed spatial dims overrides it (InsightFace's _init_vars)
Lowered lower(const Graph& g, int n, int det_w, int det_h);

}  // namespace onnx
}  // namespace ffp
