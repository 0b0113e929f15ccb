// onnx_graph.cpp — ONNX ModelProto wire-format reader and the SCRFD lowering (onnx_graph.hpp).
//
// Field numbers are those of onnx/onnx.proto (ModelProto.graph = 7; GraphProto node 1, initializer 5, input 11, output 12;
// NodeProto input 1, output 2, name 3, op_type 4, attribute 5; AttributeProto name 1, f 2, i 3, s 4, t 5, floats 7, ints 8, type 20;
// TensorProto dims 1, data_type 2, float_data 4, int32_data 5, int64_data 7, name 8, raw_data 9, double_data 10, external_data 13,
// data_location 14; ValueInfoProto name 1, type 2; TypeProto tensor_type 1; Tensor shape 2; Shape dim 1; Dimension dim_value 1).
#include "onnx_graph.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <set>
#include <sstream>

#include "common.hpp"

namespace ffp {
namespace onnx {

namespace {

// ---- protobuf wire format ---------------------------------------------------------------------------------------------
struct Reader {
  const uint8_t* p;
  const uint8_t* e;
  bool done() const { return p >= e; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int sh = 0; sh < 64; sh += 7) {
      FFP_CHECK(p < e, FFP_ERR_ARG, "onnx: truncated varint");
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7F) << sh;
      if (!(b & 0x80)) return v;
    }
    fail(FFP_ERR_ARG, "onnx: varint longer than 10 bytes");
  }
  Reader sub() {
    const uint64_t n = varint();
    FFP_CHECK(n <= (uint64_t)(e - p), FFP_ERR_ARG, "onnx: length-delimited field of %llu bytes overruns its message", (unsigned long long)n);
    Reader r{p, p + n};
    p += n;
    return r;
  }
  std::string str() { Reader r = sub(); return std::string((const char*)r.p, (size_t)(r.e - r.p)); }
  uint32_t fixed32() {
    FFP_CHECK(e - p >= 4, FFP_ERR_ARG, "onnx: truncated fixed32");
    uint32_t v;
    std::memcpy(&v, p, 4);
    p += 4;
    return v;
  }
  uint64_t fixed64() {
    FFP_CHECK(e - p >= 8, FFP_ERR_ARG, "onnx: truncated fixed64");
    uint64_t v;
    std::memcpy(&v, p, 8);
    p += 8;
    return v;
  }
  void skip(int wt) {
    if (wt == 0) varint();
    else if (wt == 1) fixed64();
    else if (wt == 2) sub();
    else if (wt == 5) fixed32();
    else fail(FFP_ERR_ARG, "onnx: unsupported wire type %d", wt);
  }
  // one key: field number and wire type
  bool key(int& field, int& wt) {
    if (done()) return false;
    const uint64_t k = varint();
    field = (int)(k >> 3);
    wt = (int)(k & 7);
    FFP_CHECK(field > 0, FFP_ERR_ARG, "onnx: field number 0");
    return true;
  }
};

float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
double as_double(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }

// repeated scalar fields arrive packed (wire type 2) or one per key
void rep_int64(Reader& r, int wt, std::vector<int64_t>& out) {
  if (wt == 2) { Reader s = r.sub(); while (!s.done()) out.push_back((int64_t)s.varint()); }
  else { FFP_CHECK(wt == 0, FFP_ERR_ARG, "onnx: integer field with wire type %d", wt); out.push_back((int64_t)r.varint()); }
}
void rep_float(Reader& r, int wt, std::vector<float>& out) {
  if (wt == 2) {
    Reader s = r.sub();
    FFP_CHECK((s.e - s.p) % 4 == 0, FFP_ERR_ARG, "onnx: packed floats of %lld bytes", (long long)(s.e - s.p));
    while (!s.done()) out.push_back(as_float(s.fixed32()));
  } else { FFP_CHECK(wt == 5, FFP_ERR_ARG, "onnx: float field with wire type %d", wt); out.push_back(as_float(r.fixed32())); }
}
void rep_double(Reader& r, int wt, std::vector<float>& out) {
  if (wt == 2) {
    Reader s = r.sub();
    FFP_CHECK((s.e - s.p) % 8 == 0, FFP_ERR_ARG, "onnx: packed doubles of %lld bytes", (long long)(s.e - s.p));
    while (!s.done()) out.push_back((float)as_double(s.fixed64()));
  } else { FFP_CHECK(wt == 1, FFP_ERR_ARG, "onnx: double field with wire type %d", wt); out.push_back((float)as_double(r.fixed64())); }
}

Tensor read_tensor(Reader r) {
  Tensor t;
  std::string raw;
  bool has_raw = false;
  std::vector<int64_t> i32;
  int f, wt;
  while (r.key(f, wt)) {
    if (f == 1) rep_int64(r, wt, t.dims);
    else if (f == 2 && wt == 0) t.dtype = (int)r.varint();
    else if (f == 4) rep_float(r, wt, t.f);
    else if (f == 5) rep_int64(r, wt, i32);
    else if (f == 7) rep_int64(r, wt, t.i);
    else if (f == 8 && wt == 2) t.name = r.str();
    else if (f == 9 && wt == 2) { raw = r.str(); has_raw = true; }
    else if (f == 10) rep_double(r, wt, t.f);
    else if (f == 13 && wt == 2) { r.sub(); t.external = true; }
    else if (f == 14 && wt == 0) { if (r.varint() == 1) t.external = true; }
    else r.skip(wt);
  }
  for (int64_t d : t.dims) FFP_CHECK(d >= 0 && d < (1ll << 31), FFP_ERR_ARG, "onnx: tensor '%s' has dimension %lld", t.name.c_str(), (long long)d);
  size_t n = 1;
  for (int64_t d : t.dims) {
    FFP_CHECK(d == 0 || n <= ((size_t)1 << 40) / (size_t)d, FFP_ERR_ARG, "onnx: tensor '%s' is too large", t.name.c_str());
    n *= (size_t)d;
  }
  if (t.external) return t;
  if (t.dtype == DT_INT32) for (int64_t v : i32) t.i.push_back((int32_t)v);
  if (has_raw) {
    const size_t es = (t.dtype == DT_FLOAT || t.dtype == DT_INT32) ? 4 : (t.dtype == DT_INT64 || t.dtype == DT_DOUBLE) ? 8 : 0;
    FFP_CHECK(es != 0, FFP_ERR_ARG, "onnx: tensor '%s' has data type %d (float, double, int32 and int64 are read)", t.name.c_str(), t.dtype);
    FFP_CHECK(raw.size() == n * es, FFP_ERR_ARG, "onnx: tensor '%s' raw_data holds %zu bytes, its dims need %zu", t.name.c_str(), raw.size(), n * es);
    const char* q = raw.data();
    for (size_t k = 0; k < n; ++k) {
      if (t.dtype == DT_FLOAT) { uint32_t u; std::memcpy(&u, q + 4 * k, 4); t.f.push_back(as_float(u)); }
      else if (t.dtype == DT_DOUBLE) { uint64_t u; std::memcpy(&u, q + 8 * k, 8); t.f.push_back((float)as_double(u)); }
      else if (t.dtype == DT_INT32) { int32_t v; std::memcpy(&v, q + 4 * k, 4); t.i.push_back(v); }
      else { int64_t v; std::memcpy(&v, q + 8 * k, 8); t.i.push_back(v); }
    }
  }
  const size_t have = (t.dtype == DT_FLOAT || t.dtype == DT_DOUBLE) ? t.f.size() : t.i.size();
  FFP_CHECK(have == n || (n == 0 && have == 0), FFP_ERR_ARG, "onnx: tensor '%s' holds %zu values, its dims need %zu", t.name.c_str(), have, n);
  return t;
}

Attr read_attr(Reader r) {
  Attr a;
  int f, wt;
  while (r.key(f, wt)) {
    if (f == 1 && wt == 2) a.name = r.str();
    else if (f == 2 && wt == 5) a.f = as_float(r.fixed32());
    else if (f == 3 && wt == 0) a.i = (int64_t)r.varint();
    else if (f == 4 && wt == 2) a.s = r.str();
    else if (f == 5 && wt == 2) { a.t = read_tensor(r.sub()); a.has_t = true; }
    else if (f == 7) rep_float(r, wt, a.floats);
    else if (f == 8) rep_int64(r, wt, a.ints);
    else if (f == 20 && wt == 0) a.type = (int)r.varint();
    else r.skip(wt);
  }
  return a;
}

Node read_node(Reader r) {
  Node n;
  int f, wt;
  while (r.key(f, wt)) {
    if (f == 1 && wt == 2) n.in.push_back(r.str());
    else if (f == 2 && wt == 2) n.out.push_back(r.str());
    else if (f == 3 && wt == 2) n.name = r.str();
    else if (f == 4 && wt == 2) n.op = r.str();
    else if (f == 5 && wt == 2) n.attrs.push_back(read_attr(r.sub()));
    else r.skip(wt);
  }
  return n;
}

ValueInfo read_value_info(Reader r) {
  ValueInfo v;
  int f, wt;
  while (r.key(f, wt)) {
    if (f == 1 && wt == 2) { v.name = r.str(); continue; }
    if (!(f == 2 && wt == 2)) { r.skip(wt); continue; }
    Reader ty = r.sub();
    int f2, w2;
    while (ty.key(f2, w2)) {
      if (!(f2 == 1 && w2 == 2)) { ty.skip(w2); continue; }
      Reader tt = ty.sub();
      int f3, w3;
      while (tt.key(f3, w3)) {
        if (!(f3 == 2 && w3 == 2)) { tt.skip(w3); continue; }
        Reader sh = tt.sub();
        int f4, w4;
        while (sh.key(f4, w4)) {
          if (!(f4 == 1 && w4 == 2)) { sh.skip(w4); continue; }
          Reader dm = sh.sub();
          int64_t d = -1;
          int f5, w5;
          while (dm.key(f5, w5)) {
            if (f5 == 1 && w5 == 0) d = (int64_t)dm.varint();
            else dm.skip(w5);
          }
          v.dims.push_back(d);
        }
      }
    }
  }
  return v;
}

}  // namespace

Graph parse(const void* p, size_t n) {
  FFP_CHECK(p && n > 0, FFP_ERR_ARG, "onnx: empty model");
  Reader m{(const uint8_t*)p, (const uint8_t*)p + n};
  Graph g;
  bool has_graph = false;
  int f, wt;
  while (m.key(f, wt)) {
    if (!(f == 7 && wt == 2)) { m.skip(wt); continue; }
    has_graph = true;
    Reader r = m.sub();
    int f2, w2;
    while (r.key(f2, w2)) {
      if (f2 == 1 && w2 == 2) g.nodes.push_back(read_node(r.sub()));
      else if (f2 == 5 && w2 == 2) { Tensor t = read_tensor(r.sub()); g.init[t.name] = std::move(t); }
      else if (f2 == 11 && w2 == 2) g.inputs.push_back(read_value_info(r.sub()));
      else if (f2 == 12 && w2 == 2) g.outputs.push_back(read_value_info(r.sub()));
      else r.skip(w2);
    }
  }
  FFP_CHECK(has_graph, FFP_ERR_ARG, "onnx: no graph in the model (not an ONNX ModelProto?)");
  return g;
}

// ---- lowering ---------------------------------------------------------------------------------------------------------------

namespace {

struct Val {
  enum Kind { NONE, CONST, ACT, PEND } kind = NONE;
  Tensor c;                 // CONST (int64 in c.i, float in c.f; dtype says which)
  LView v;                  // ACT
  int stride = 1;           // ACT / PEND: 1/stride of the network size
  int pend = -1;            // PEND: index into pending
  bool sigmoid = false, nhwc = false;
};

const char* act_name(int a) { return a == 3 ? "relu" : a == 1 ? "silu" : a == 2 ? "lrelu" : "-"; }

struct Lowerer {
  const Graph& g;
  Lowered L;
  std::map<std::string, Val> vals;
  std::map<std::string, int> uses;
  std::vector<LStep> pending;
  std::map<int, std::string> pend_name;        // pending conv -> name of the value that currently holds it
  const std::map<std::string, int>* chans;     // pass 2: channels of every activation value (pass 1), for Concat slices
  std::map<std::string, std::pair<std::string, int>> concat_dst;     // value -> (Concat output, channel offset)
  std::map<std::string, int> concat_buf;
  std::map<std::string, int> chan_out;         // pass 1 result

  explicit Lowerer(const Graph& gr) : g(gr), chans(nullptr) {}

  [[noreturn]] void refuse(const Node& nd, const char* what, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fail(FFP_ERR_ARG, "onnx: node '%s' (%s): %s %s", nd.name.c_str(), nd.op.c_str(), what, buf);
  }

  static int pad4(int c) { return (c + 3) / 4 * 4; }

  int new_buf(int C, int stride) {
    L.bufs.push_back(LBuf{pad4(C), stride});
    return (int)L.bufs.size() - 1;
  }
  // storage for the value `name` of C channels: its own buffer, or its slice of a Concat's buffer
  LView storage(const std::string& name, int C, int stride) {
    auto it = concat_dst.find(name);
    if (it != concat_dst.end() && chans) {
      const std::string& cn = it->second.first;
      auto bt = concat_buf.find(cn);
      int b;
      if (bt == concat_buf.end()) { b = new_buf(chans->at(cn), stride); concat_buf[cn] = b; }
      else b = bt->second;
      FFP_CHECK(L.bufs[b].stride == stride, FFP_ERR_ARG, "onnx: Concat '%s' joins tensors of different sizes", cn.c_str());
      return LView{b, it->second.second, C};
    }
    return LView{new_buf(C, stride), 0, C};
  }

  const Val& get(const Node& nd, size_t k) {
    FFP_CHECK(k < nd.in.size() && !nd.in[k].empty(), FFP_ERR_ARG, "onnx: node '%s' (%s): input %zu missing", nd.name.c_str(), nd.op.c_str(), k);
    auto it = vals.find(nd.in[k]);
    if (it == vals.end()) {
      auto jt = g.init.find(nd.in[k]);
      FFP_CHECK(jt != g.init.end(), FFP_ERR_ARG, "onnx: node '%s' (%s): input '%s' is produced by no earlier node", nd.name.c_str(), nd.op.c_str(),
                nd.in[k].c_str());
      FFP_CHECK(!jt->second.external, FFP_ERR_ARG, "onnx: node '%s' (%s): initializer '%s' uses external data (refused: pass a self-contained file)",
                nd.name.c_str(), nd.op.c_str(), nd.in[k].c_str());
      Val v;
      v.kind = Val::CONST;
      v.c = jt->second;
      it = vals.emplace(nd.in[k], std::move(v)).first;
    }
    return it->second;
  }
  bool has_in(const Node& nd, size_t k) const { return k < nd.in.size() && !nd.in[k].empty(); }

  // a pending conv becomes a step with an output buffer
  void emit(const std::string& name) {
    Val& v = vals.at(name);
    if (v.kind != Val::PEND) return;
    LStep s = std::move(pending[v.pend]);
    pend_name.erase(v.pend);
    s.out = storage(name, s.cout, v.stride);
    L.steps.push_back(std::move(s));
    v.kind = Val::ACT;
    v.v = L.steps.back().out;
    chan_out[name] = v.v.C;
  }
  // an activation input of a compute node (no Sigmoid / Transpose in between)
  const Val& act_in(const Node& nd, size_t k) {
    get(nd, k);
    emit(nd.in[k]);
    const Val& v = vals.at(nd.in[k]);
    if (v.kind != Val::ACT || v.sigmoid || v.nhwc) refuse(nd, "input", "'%s' must be a feature map (not a constant, a Sigmoid or a Transpose output)", nd.in[k].c_str());
    return v;
  }
  bool fusable(const Node& nd, size_t k) {
    if (!has_in(nd, k)) return false;
    auto it = vals.find(nd.in[k]);
    return it != vals.end() && it->second.kind == Val::PEND && uses[nd.in[k]] == 1;
  }
  void set_pend(const Node& nd, int pi, int stride) {
    Val v;
    v.kind = Val::PEND;
    v.pend = pi;
    v.stride = stride;
    vals[nd.out.at(0)] = v;
    pend_name[pi] = nd.out.at(0);
  }
  std::vector<int64_t> ints_attr(const Node& nd, const char* n, std::vector<int64_t> dflt) {
    const Attr* a = nd.attr(n);
    return a ? a->ints : dflt;
  }
  void set_const(const Node& nd, Tensor t) {
    Val v;
    v.kind = Val::CONST;
    v.c = std::move(t);
    vals[nd.out.at(0)] = std::move(v);
  }
  const Tensor& cst(const Node& nd, size_t k) {
    const Val& v = get(nd, k);
    if (v.kind != Val::CONST) refuse(nd, "input", "'%s' must be a constant (or a shape computation folded on the host)", nd.in[k].c_str());
    return v.c;
  }
  static bool is_int(const Tensor& t) { return t.dtype == DT_INT64 || t.dtype == DT_INT32; }
  static std::vector<double> num(const Tensor& t) {
    std::vector<double> r;
    if (is_int(t)) for (int64_t x : t.i) r.push_back((double)x);
    else for (float x : t.f) r.push_back(x);
    return r;
  }

  void node(const Node& nd) {
    const std::string& op = nd.op;
    FFP_CHECK(!nd.out.empty(), FFP_ERR_ARG, "onnx: node '%s' (%s) has no output", nd.name.c_str(), op.c_str());
    if (op == "Conv") return conv(nd);
    if (op == "BatchNormalization") return batchnorm(nd);
    if (op == "Relu") return relu(nd);
    if (op == "Add") return add(nd);
    if (op == "MaxPool" || op == "AveragePool") return pool(nd);
    if (op == "Resize" || op == "Upsample") return resize(nd);
    if (op == "Sigmoid") {                      // before or after the head's Transpose + Reshape: it commutes with both
      const Val& x0 = get(nd, 0);
      if (x0.kind == Val::CONST) refuse(nd, "input", "is a constant");
      emit(nd.in[0]);
      const Val& x = vals.at(nd.in[0]);
      if (x.sigmoid) refuse(nd, "input", "'%s' is already a Sigmoid output", nd.in[0].c_str());
      Val v = x;
      v.sigmoid = true;
      vals[nd.out[0]] = v;
      return;
    }
    if (op == "Transpose") {
      const Val& x = get(nd, 0);
      if (x.kind == Val::CONST) refuse(nd, "input", "is a constant");
      emit(nd.in[0]);
      // (0,2,3,1): the batched export; (2,3,0,1): the batch-1 export, the same layout for one image (InsightFace runs one image per call,
      // and each tile here is such a run)
      const std::vector<int64_t> perm = ints_attr(nd, "perm", {});
      if (perm != std::vector<int64_t>{0, 2, 3, 1} && perm != std::vector<int64_t>{2, 3, 0, 1})
        refuse(nd, "attribute 'perm'", "must be (0,2,3,1) or (2,3,0,1): only the head outputs' channel-last transpose is lowered");
      Val v = vals.at(nd.in[0]);
      v.nhwc = true;
      vals[nd.out[0]] = v;
      return;
    }
    if (op == "Reshape" || op == "Flatten") {
      const Val& x = get(nd, 0);
      if (x.kind == Val::CONST && op == "Reshape") {       // reshape of a folded shape tensor
        Tensor t = x.c;
        t.dims = {(int64_t)(is_int(t) ? t.i.size() : t.f.size())};
        return set_const(nd, t);
      }
      if (!(x.kind == Val::ACT && x.nhwc)) refuse(nd, "input", "'%s' must be a head output after Transpose(0,2,3,1)", nd.in[0].c_str());
      vals[nd.out[0]] = x;
      return;
    }
    if (op == "Mul") return mul(nd);
    if (op == "Concat") return concat(nd);
    shape_op(nd);
  }

  void conv(const Node& nd) {
    const Val& x = act_in(nd, 0);
    const Tensor& w = cst(nd, 1);
    if (w.dtype != DT_FLOAT || w.dims.size() != 4) refuse(nd, "input", "weight '%s' must be a float OIHW tensor", nd.in[1].c_str());
    const int cout = (int)w.dims[0], cin = (int)w.dims[1], k = (int)w.dims[2];
    const int64_t group = nd.attr("group") ? nd.attr("group")->i : 1;
    if (group != 1) refuse(nd, "attribute 'group'", "= %lld: only dense convolutions (group 1) are lowered", (long long)group);
    const std::vector<int64_t> ks = ints_attr(nd, "kernel_shape", {w.dims[2], w.dims[3]});
    if (ks.size() != 2 || ks[0] != ks[1] || ks[0] != w.dims[2] || ks[1] != w.dims[3] || (k != 1 && k != 3))
      refuse(nd, "attribute 'kernel_shape'", "must be 1x1 or 3x3 (got %lldx%lld)", (long long)w.dims[2], (long long)w.dims[3]);
    const std::vector<int64_t> st = ints_attr(nd, "strides", {1, 1});
    if (st.size() != 2 || st[0] != st[1] || (st[0] != 1 && st[0] != 2)) refuse(nd, "attribute 'strides'", "must be (1,1) or (2,2)");
    const std::vector<int64_t> pads = ints_attr(nd, "pads", {0, 0, 0, 0});
    if (pads != std::vector<int64_t>(4, k / 2)) refuse(nd, "attribute 'pads'", "must be %d on every side (kernel %d)", k / 2, k);
    const std::vector<int64_t> dil = ints_attr(nd, "dilations", {1, 1});
    if (dil != std::vector<int64_t>{1, 1}) refuse(nd, "attribute 'dilations'", "must be (1,1)");
    if (nd.attr("auto_pad") && nd.attr("auto_pad")->s != "NOTSET") refuse(nd, "attribute 'auto_pad'", "must be NOTSET");
    if (cin != x.v.C) refuse(nd, "input", "weight has %d input channels, the feature map %d", cin, x.v.C);
    const int s = (int)st[0];
    if (s == 2 && (L.det_h % (2 * x.stride) || L.det_w % (2 * x.stride))) refuse(nd, "attribute 'strides'", "halves a map of odd size");
    LStep c;
    c.kind = ST_CONV;
    c.node = nd.name;
    c.in = x.v;
    c.k = k; c.stride = s; c.cin = cin; c.cout = cout;
    c.w = w.f;
    c.b.assign(cout, 0.f);
    if (has_in(nd, 2)) {
      const Tensor& b = cst(nd, 2);
      if (b.dtype != DT_FLOAT || b.numel() != (size_t)cout) refuse(nd, "input", "bias '%s' must hold %d floats", nd.in[2].c_str(), cout);
      c.b = b.f;
    }
    pending.push_back(std::move(c));
    set_pend(nd, (int)pending.size() - 1, x.stride * s);
  }

  LStep& pend_of(const Node& nd, size_t k) { return pending[vals.at(nd.in[k]).pend]; }

  void batchnorm(const Node& nd) {
    get(nd, 0);
    if (!fusable(nd, 0)) refuse(nd, "input", "'%s': BatchNormalization is folded into the Conv it follows, and that Conv feeds nothing else", nd.in[0].c_str());
    LStep& c = pend_of(nd, 0);
    if (c.act || c.res.buf >= 0 || !c.fused.empty()) refuse(nd, "input", "BatchNormalization after an activation, a residual or a scale is not folded");
    const float eps = nd.attr("epsilon") ? nd.attr("epsilon")->f : 1e-5f;
    const Tensor *t[4];
    for (int i = 0; i < 4; ++i) {
      t[i] = &cst(nd, 1 + i);
      if (t[i]->dtype != DT_FLOAT || t[i]->numel() != (size_t)c.cout) refuse(nd, "input", "'%s' must hold %d floats", nd.in[1 + i].c_str(), c.cout);
    }
    const size_t per = (size_t)c.cin * c.k * c.k;
    for (int o = 0; o < c.cout; ++o) {
      const double sc = (double)t[0]->f[o] / std::sqrt((double)t[3]->f[o] + (double)eps);
      for (size_t j = 0; j < per; ++j) c.w[o * per + j] = (float)((double)c.w[o * per + j] * sc);
      c.b[o] = (float)(((double)c.b[o] - (double)t[2]->f[o]) * sc + (double)t[1]->f[o]);
    }
    c.fused.push_back("BatchNormalization:" + nd.name);
    const Val v = vals.at(nd.in[0]);
    vals[nd.out[0]] = v;
    pend_name[v.pend] = nd.out[0];
  }

  void mul(const Node& nd) {
    const Val& a = get(nd, 0);
    const Val& b = get(nd, 1);
    if (a.kind == Val::CONST && b.kind == Val::CONST) return shape_op(nd);
    const size_t ci = a.kind == Val::CONST ? 0 : 1, xi = 1 - ci;
    const Val& s = ci == 0 ? a : b;
    if (s.kind != Val::CONST || s.c.dtype != DT_FLOAT || s.c.numel() != 1)
      refuse(nd, "input", "a Mul is lowered only as a scalar float initializer times a Conv output (the bbox branch's Scale)");
    if (!fusable(nd, xi)) refuse(nd, "input", "'%s': the scaled tensor must be a Conv output that feeds nothing else", nd.in[xi].c_str());
    LStep& c = pend_of(nd, xi);
    if (c.act || c.res.buf >= 0) refuse(nd, "input", "a Scale after an activation or a residual is not folded");
    const float m = s.c.f[0];
    for (float& x : c.w) x *= m;        // the Scale folded into the conv (fp32, exact for a power of two)
    for (float& x : c.b) x *= m;
    c.fused.push_back("Mul:" + nd.name);
    const Val v = vals.at(nd.in[xi]);
    vals[nd.out[0]] = v;
    pend_name[v.pend] = nd.out[0];
  }

  void relu(const Node& nd) {
    get(nd, 0);
    if (!fusable(nd, 0)) refuse(nd, "input", "'%s': Relu is fused into the epilogue of the Conv (or Conv + Add) it follows", nd.in[0].c_str());
    LStep& c = pend_of(nd, 0);
    if (c.res.buf >= 0) {
      if (c.act_post) refuse(nd, "input", "two activations after one residual");
      c.act_post = ACT_RELU;
    } else {
      if (c.act) refuse(nd, "input", "two activations after one Conv");
      c.act = ACT_RELU;
    }
    c.fused.push_back("Relu:" + nd.name);
    const Val v = vals.at(nd.in[0]);
    vals[nd.out[0]] = v;
    pend_name[v.pend] = nd.out[0];
  }

  void add(const Node& nd) {
    const Val& a = get(nd, 0);
    const Val& b = get(nd, 1);
    if (a.kind == Val::CONST && b.kind == Val::CONST) return shape_op(nd);
    size_t fi;
    if (fusable(nd, 0) && pending[a.pend].res.buf < 0 && !pending[a.pend].act_post) fi = 0;
    else if (fusable(nd, 1) && pending[b.pend].res.buf < 0 && !pending[b.pend].act_post) fi = 1;
    else refuse(nd, "input", "an Add is fused as the residual of a Conv that feeds nothing else; neither '%s' nor '%s' is one", nd.in[0].c_str(),
                nd.in[1].c_str());
    const Val& r = act_in(nd, 1 - fi);
    const Val cv = vals.at(nd.in[fi]);
    LStep& c = pending[cv.pend];
    if (r.v.C != c.cout || r.stride != cv.stride) refuse(nd, "input", "residual '%s' has %d channels at 1/%d, the Conv %d at 1/%d", nd.in[1 - fi].c_str(),
                                                         r.v.C, r.stride, c.cout, cv.stride);
    c.res = r.v;
    c.fused.push_back("Add:" + nd.name);
    vals[nd.out[0]] = cv;
    pend_name[cv.pend] = nd.out[0];
  }

  void pool(const Node& nd) {
    const Val x = act_in(nd, 0);
    const bool mx = nd.op == "MaxPool";
    const std::vector<int64_t> ks = ints_attr(nd, "kernel_shape", {}), st = ints_attr(nd, "strides", {1, 1}), pads = ints_attr(nd, "pads", {0, 0, 0, 0});
    const int64_t ceil = nd.attr("ceil_mode") ? nd.attr("ceil_mode")->i : 0;
    LStep s;
    s.node = nd.name;
    s.in = x.v;
    if (mx) {
      if (ks != std::vector<int64_t>{3, 3}) refuse(nd, "attribute 'kernel_shape'", "must be 3x3");
      if (st != std::vector<int64_t>{2, 2}) refuse(nd, "attribute 'strides'", "must be (2,2)");
      if (pads != std::vector<int64_t>(4, 1)) refuse(nd, "attribute 'pads'", "must be 1 on every side");
      if (ceil) refuse(nd, "attribute 'ceil_mode'", "must be 0");
      if (ints_attr(nd, "dilations", {1, 1}) != std::vector<int64_t>{1, 1}) refuse(nd, "attribute 'dilations'", "must be (1,1)");
      if (nd.attr("storage_order") && nd.attr("storage_order")->i) refuse(nd, "attribute 'storage_order'", "must be 0");
      if (nd.out.size() > 1) refuse(nd, "output", "Indices are not produced");
      s.kind = ST_MAXPOOL; s.k = 3; s.stride = 2;
    } else {
      if (ks.size() != 2 || ks[0] != ks[1] || st != ks || ks[0] < 1 || ks[0] > 8) refuse(nd, "attribute 'kernel_shape'", "must be square and equal to 'strides'");
      if (pads != std::vector<int64_t>(4, 0)) refuse(nd, "attribute 'pads'", "must be 0");
      if (nd.attr("count_include_pad") && nd.attr("count_include_pad")->i) refuse(nd, "attribute 'count_include_pad'", "must be 0");
      s.kind = ST_AVGPOOL; s.k = (int)ks[0]; s.stride = (int)ks[0]; s.ceil_mode = ceil != 0;
    }
    if (L.det_h % (x.stride * s.stride) || L.det_w % (x.stride * s.stride)) refuse(nd, "attribute 'strides'", "does not divide the feature map");
    s.cin = s.cout = x.v.C;
    s.out = storage(nd.out[0], x.v.C, x.stride * s.stride);
    L.steps.push_back(s);
    Val v;
    v.kind = Val::ACT; v.v = s.out; v.stride = x.stride * s.stride;
    vals[nd.out[0]] = v;
    chan_out[nd.out[0]] = v.v.C;
  }

  void resize(const Node& nd) {
    const Val x = act_in(nd, 0);
    const Attr* mode = nd.attr("mode");
    if (mode && mode->s != "nearest") refuse(nd, "attribute 'mode'", "is '%s': only nearest is lowered", mode->s.c_str());
    // the plan's x2 upsample reads source pixel floor(x / 2): accept only the coordinate / rounding pairs that reduce to it at scale 2
    // (opset 11+ Resize defaults: half_pixel + round_prefer_floor; opset 10 Resize and Upsample: asymmetric + floor)
    const bool v11 = nd.op == "Resize" && nd.in.size() > 2;
    const Attr* ctm_a = nd.attr("coordinate_transformation_mode");
    const Attr* nm_a = nd.attr("nearest_mode");
    const std::string ctm = ctm_a ? ctm_a->s : v11 ? "half_pixel" : "asymmetric";
    const std::string nm = nm_a ? nm_a->s : v11 ? "round_prefer_floor" : "floor";
    bool floor2 = false;
    if (ctm == "asymmetric") floor2 = nm == "floor" || nm == "round_prefer_floor";
    else if (ctm == "half_pixel" || ctm == "pytorch_half_pixel") floor2 = nm == "round_prefer_floor" || nm == "round_prefer_ceil";
    else if (ctm == "tf_half_pixel_for_nn") floor2 = nm == "floor";
    if (ctm == "align_corners" || ctm == "tf_crop_and_resize") refuse(nd, "attribute 'coordinate_transformation_mode'", "'%s' is refused", ctm.c_str());
    if (!floor2) refuse(nd, "attribute 'nearest_mode'", "'%s' with coordinate_transformation_mode '%s' does not sample pixel floor(x / 2)", nm.c_str(), ctm.c_str());
    std::vector<double> sc;
    if (nd.op == "Upsample") {
      if (has_in(nd, 1)) sc = num(cst(nd, 1));
      else if (nd.attr("scales")) for (float f : nd.attr("scales")->floats) sc.push_back(f);
    } else {
      const size_t si = nd.in.size() == 2 ? 1 : 2;     // opset 10: (X, scales); 11+: (X, roi, scales, sizes)
      if (has_in(nd, si) && cst(nd, si).numel() > 0) sc = num(cst(nd, si));
      if (sc.empty() && has_in(nd, 3)) {
        const std::vector<double> sz = num(cst(nd, 3));
        const int h = L.det_h / x.stride, w = L.det_w / x.stride;
        if (sz.size() != 4 || sz[2] != 2.0 * h || sz[3] != 2.0 * w || sz[1] != x.v.C)
          refuse(nd, "input", "'sizes' must double the map (%dx%d -> %dx%d)", h, w, 2 * h, 2 * w);
        sc = {1, 1, 2, 2};
      }
    }
    if (sc.size() != 4 || sc[0] != 1 || sc[1] != 1 || sc[2] != 2 || sc[3] != 2) refuse(nd, "input", "scales must be exactly (1,1,2,2)");
    if (x.stride % 2) refuse(nd, "input", "upsamples a map beyond the network size");
    LStep s;
    s.kind = ST_UP2; s.node = nd.name; s.in = x.v; s.cin = s.cout = x.v.C; s.stride = 2;
    s.out = storage(nd.out[0], x.v.C, x.stride / 2);
    L.steps.push_back(s);
    Val v;
    v.kind = Val::ACT; v.v = s.out; v.stride = x.stride / 2;
    vals[nd.out[0]] = v;
    chan_out[nd.out[0]] = v.v.C;
  }

  void concat(const Node& nd) {
    bool all_const = true;
    for (size_t k = 0; k < nd.in.size(); ++k) all_const = all_const && get(nd, k).kind == Val::CONST;
    if (all_const) return shape_op(nd);
    const int64_t axis = nd.attr("axis") ? nd.attr("axis")->i : 0;
    if (axis != 1) refuse(nd, "attribute 'axis'", "= %lld: feature maps are concatenated on channels only", (long long)axis);
    int C = 0, buf = -1, stride = 0;
    for (size_t k = 0; k < nd.in.size(); ++k) {
      const Val& x = act_in(nd, k);
      if (x.v.C % 4) refuse(nd, "input", "'%s' has %d channels (a multiple of 4 is needed for a channel slice)", nd.in[k].c_str(), x.v.C);
      if (chans) {
        if (k == 0) buf = x.v.buf;
        if (x.v.buf != buf || x.v.coff != C) refuse(nd, "input", "'%s' is not written in place into the concatenation (it has another consumer or is a graph input)", nd.in[k].c_str());
      }
      if (k == 0) stride = x.stride;
      if (x.stride != stride) refuse(nd, "input", "joins maps of different sizes");
      C += x.v.C;
    }
    Val v;
    v.kind = Val::ACT; v.stride = stride;
    v.v = chans ? LView{buf, 0, C} : LView{new_buf(C, stride), 0, C};
    vals[nd.out[0]] = v;
    chan_out[nd.out[0]] = C;
  }

  // shape subgraphs folded on the host
  void shape_op(const Node& nd) {
    const std::string& op = nd.op;
    Tensor t;
    if (op == "Shape") {
      const Val& x = get(nd, 0);
      if (x.kind == Val::CONST) { t.dtype = DT_INT64; for (int64_t d : x.c.dims) t.i.push_back(d); }
      else {
        const int C = x.kind == Val::PEND ? pending[x.pend].cout : x.v.C;
        t.dtype = DT_INT64;
        t.i = {L.n, C, L.det_h / x.stride, L.det_w / x.stride};
      }
      t.dims = {(int64_t)t.i.size()};
      return set_const(nd, t);
    }
    if (op == "Constant") {
      const Attr* a = nd.attr("value");
      if (!a || !a->has_t) refuse(nd, "attribute 'value'", "must be a tensor");
      if (a->t.external) refuse(nd, "attribute 'value'", "uses external data");
      return set_const(nd, a->t);
    }
    if (op == "ConstantOfShape") {
      const Tensor& s = cst(nd, 0);
      const Attr* a = nd.attr("value");
      t.dtype = a && a->has_t ? a->t.dtype : DT_FLOAT;
      for (int64_t d : s.i) if (d < 0 || d > (1 << 20)) refuse(nd, "input", "shape dimension %lld", (long long)d);
      if (s.i.size() > 4) refuse(nd, "input", "rank %zu", s.i.size());
      t.dims = s.i;
      const size_t n = t.numel();
      if (n > (1u << 20)) refuse(nd, "input", "shape too large");
      if (is_int(t)) t.i.assign(n, a && a->has_t && !a->t.i.empty() ? a->t.i[0] : 0);
      else t.f.assign(n, a && a->has_t && !a->t.f.empty() ? a->t.f[0] : 0.f);
      return set_const(nd, t);
    }
    if (op == "Cast") {
      t = cst(nd, 0);
      const int64_t to = nd.attr("to") ? nd.attr("to")->i : 0;
      const std::vector<double> v = num(t);
      t.f.clear(); t.i.clear();
      if (to == DT_INT64 || to == DT_INT32) {
        t.dtype = DT_INT64;
        for (double d : v) {
          if (!(std::fabs(d) < 9.0e18)) refuse(nd, "input", "value %g does not fit int64", d);
          t.i.push_back((int64_t)d);
        }
      }
      else if (to == DT_FLOAT || to == DT_DOUBLE) { t.dtype = DT_FLOAT; for (double d : v) t.f.push_back((float)d); }
      else refuse(nd, "attribute 'to'", "= %lld: casts to float or int64 only", (long long)to);
      return set_const(nd, t);
    }
    if (op == "Unsqueeze" || op == "Squeeze") {
      t = cst(nd, 0);
      const size_t n = t.numel();
      t.dims = n == 1 && op == "Squeeze" ? std::vector<int64_t>{} : std::vector<int64_t>{(int64_t)n};
      return set_const(nd, t);
    }
    if (op == "Floor") {
      t = cst(nd, 0);
      for (float& f : t.f) f = std::floor(f);
      return set_const(nd, t);
    }
    if (op == "Gather") {
      const Tensor& d = cst(nd, 0);
      const Tensor& ix = cst(nd, 1);
      const int64_t axis = nd.attr("axis") ? nd.attr("axis")->i : 0;
      if (axis != 0 || d.dims.size() != 1 || !is_int(ix)) refuse(nd, "input", "Gather is folded on 1-D shape tensors only");
      t.dtype = d.dtype;
      t.dims = ix.dims;
      const int64_t n = (int64_t)(is_int(d) ? d.i.size() : d.f.size());
      for (int64_t j : ix.i) {
        if (j < 0) j += n;
        if (j < 0 || j >= n) refuse(nd, "input", "index %lld outside %lld", (long long)j, (long long)n);
        if (is_int(d)) t.i.push_back(d.i[j]); else t.f.push_back(d.f[j]);
      }
      return set_const(nd, t);
    }
    if (op == "Concat") {
      t.dtype = cst(nd, 0).dtype;
      for (size_t k = 0; k < nd.in.size(); ++k) {
        const Tensor& p = cst(nd, k);
        if (is_int(p) != is_int(t)) refuse(nd, "input", "mixes integer and float constants");
        t.i.insert(t.i.end(), p.i.begin(), p.i.end());
        t.f.insert(t.f.end(), p.f.begin(), p.f.end());
      }
      t.dims = {(int64_t)(is_int(t) ? t.i.size() : t.f.size())};
      return set_const(nd, t);
    }
    if (op == "Slice") {
      const Tensor& d = cst(nd, 0);
      std::vector<int64_t> starts, ends, axes, steps;
      if (nd.in.size() >= 3) {
        starts = cst(nd, 1).i; ends = cst(nd, 2).i;
        if (has_in(nd, 3)) axes = cst(nd, 3).i;
        if (has_in(nd, 4)) steps = cst(nd, 4).i;
      } else {
        starts = ints_attr(nd, "starts", {}); ends = ints_attr(nd, "ends", {}); axes = ints_attr(nd, "axes", {});
      }
      if (starts.size() != 1 || ends.size() != 1 || (!axes.empty() && axes[0] != 0) || (!steps.empty() && steps[0] != 1))
        refuse(nd, "input", "Slice is folded on 1-D shape tensors with step 1 only");
      const int64_t n = (int64_t)(is_int(d) ? d.i.size() : d.f.size());
      int64_t b = starts[0], e = ends[0];
      if (b < 0) b += n;
      if (e < 0) e += n;
      b = std::max<int64_t>(0, std::min(b, n));
      e = std::max<int64_t>(0, std::min(e, n));
      t.dtype = d.dtype;
      for (int64_t j = b; j < e; ++j) { if (is_int(d)) t.i.push_back(d.i[j]); else t.f.push_back(d.f[j]); }
      t.dims = {(int64_t)(is_int(t) ? t.i.size() : t.f.size())};
      return set_const(nd, t);
    }
    if (op == "Div" || op == "Mul" || op == "Add" || op == "Sub") {
      const Tensor& a = cst(nd, 0);
      const Tensor& b = cst(nd, 1);
      if (is_int(a) != is_int(b)) refuse(nd, "input", "mixes integer and float constants");
      const size_t nx = is_int(a) ? a.i.size() : a.f.size(), ny = is_int(b) ? b.i.size() : b.f.size();
      if (!(nx == ny || ny == 1 || nx == 1) || nx == 0 || ny == 0) refuse(nd, "input", "shapes do not broadcast");
      const size_t n = std::max(nx, ny);
      t.dtype = a.dtype;
      t.dims = nx >= ny ? a.dims : b.dims;
      for (size_t j = 0; j < n; ++j) {
        const size_t jx = nx == 1 ? 0 : j, jy = ny == 1 ? 0 : j;
        if (is_int(t)) {                        // int64 arithmetic, overflow refused (ONNX integer Div truncates)
          const int64_t p = a.i[jx], q = b.i[jy];
          int64_t r = 0;
          bool ovf = false;
          if (op == "Mul") ovf = __builtin_mul_overflow(p, q, &r);
          else if (op == "Add") ovf = __builtin_add_overflow(p, q, &r);
          else if (op == "Sub") ovf = __builtin_sub_overflow(p, q, &r);
          else {
            if (q == 0) refuse(nd, "input", "division by zero");
            ovf = p == INT64_MIN && q == -1;
            if (!ovf) r = p / q;
          }
          if (ovf) refuse(nd, "input", "int64 overflow");
          t.i.push_back(r);
        } else {
          const float p = a.f[jx], q = b.f[jy];
          t.f.push_back(op == "Mul" ? p * q : op == "Add" ? p + q : op == "Sub" ? p - q : p / q);
        }
      }
      return set_const(nd, t);
    }
    refuse(nd, "op type", "'%s' is outside the lowered subset", op.c_str());
  }

  void run(int n, int det_w, int det_h) {
    L.n = n;
    // the image input: the one graph input that is not an initializer
    const ValueInfo* in = nullptr;
    for (const ValueInfo& v : g.inputs)
      if (!g.init.count(v.name)) {
        FFP_CHECK(!in, FFP_ERR_ARG, "onnx: the graph has more than one image input ('%s', '%s')", in->name.c_str(), v.name.c_str());
        in = &v;
      }
    FFP_CHECK(in, FFP_ERR_ARG, "onnx: the graph has no image input");
    FFP_CHECK(in->dims.size() == 4 && in->dims[1] == 3, FFP_ERR_ARG, "onnx: input '%s' must be N x 3 x H x W", in->name.c_str());
    if (in->dims[2] > 0 && in->dims[3] > 0) { det_h = (int)in->dims[2]; det_w = (int)in->dims[3]; }     // a fixed input size wins over det_size
    FFP_CHECK(det_w >= 32 && det_h >= 32 && det_w % 32 == 0 && det_h % 32 == 0 && det_w <= 4096 && det_h <= 4096, FFP_ERR_ARG,
              "onnx: det size %dx%d must be multiples of 32 in [32, 4096]", det_w, det_h);
    FFP_CHECK(n >= 1 && n <= 4096, FFP_ERR_ARG, "onnx: batch %d outside [1, 4096]", n);
    L.det_w = det_w; L.det_h = det_h;
    for (const Node& nd : g.nodes)                     // a Shape reads no values: it does not keep a conv from fusing into its consumer
      if (nd.op != "Shape") for (const std::string& s : nd.in) if (!s.empty()) ++uses[s];
    for (const ValueInfo& o : g.outputs) ++uses[o.name];
    L.input_buf = new_buf(3, 1);
    Val x;
    x.kind = Val::ACT; x.v = LView{L.input_buf, 0, 3}; x.stride = 1;
    vals[in->name] = x;
    for (const Node& nd : g.nodes) node(nd);
    // outputs: 9 (scores, bbox distances, keypoint distances at strides 8/16/32) or 6 (no keypoints), in InsightFace's order
    const int no = (int)g.outputs.size();
    FFP_CHECK(no == 9 || no == 6, FFP_ERR_ARG,
              "onnx: %d graph outputs: an SCRFD detector with 3 strides has 9 (or 6 without keypoints); the 5-stride variants (10 / 15) are refused", no);
    L.fmc = 3;
    L.use_kps = no == 9;
    for (int k = 0; k < no; ++k) {
      const std::string& nm = g.outputs[k].name;
      auto it = vals.find(nm);
      FFP_CHECK(it != vals.end(), FFP_ERR_ARG, "onnx: output '%s' is produced by no node", nm.c_str());
      emit(nm);
      const Val& v = vals.at(nm);
      FFP_CHECK(v.kind == Val::ACT, FFP_ERR_ARG, "onnx: output '%s' is not a feature map", nm.c_str());
      LOutput o;
      o.v = v.v; o.stride = v.stride; o.kind = k / 3; o.sigmoid = v.sigmoid; o.name = nm;
      const int want_s = 8 << (k % 3);
      const int per = o.kind == 0 ? 1 : o.kind == 1 ? 4 : 10;
      FFP_CHECK(o.stride == want_s, FFP_ERR_ARG, "onnx: output %d '%s' is at stride %d, InsightFace reads it as stride %d", k, nm.c_str(), o.stride, want_s);
      FFP_CHECK(o.v.C == per * L.num_anchors, FFP_ERR_ARG, "onnx: output %d '%s' has %d channels, %d anchors x %d values expected", k, nm.c_str(), o.v.C,
                L.num_anchors, per);
      FFP_CHECK(o.kind != 0 || o.sigmoid, FFP_ERR_ARG, "onnx: score output '%s' does not end in a Sigmoid", nm.c_str());
      FFP_CHECK(o.kind == 0 || !o.sigmoid, FFP_ERR_ARG, "onnx: distance output '%s' ends in a Sigmoid", nm.c_str());
      L.outs.push_back(o);
    }
    FFP_CHECK(pend_name.empty(), FFP_ERR_ARG, "onnx: conv '%s' feeds no output", pending[pend_name.begin()->first].node.c_str());
  }
};

}  // namespace

double Lowered::conv_flops() const {
  double f = 0;
  for (const LStep& s : steps)
    if (s.kind == ST_CONV) {
      const double px = (double)(det_h / bufs[s.out.buf].stride) * (det_w / bufs[s.out.buf].stride) * n;
      f += 2.0 * s.cin * s.k * s.k * s.cout * px;
    }
  return f;
}

std::string Lowered::describe() const {
  std::ostringstream o;
  o << "scrfd n=" << n << " det=" << det_w << "x" << det_h << " outputs=" << outs.size() << " fmc=" << fmc << " anchors=" << num_anchors
    << " kps=" << (use_kps ? 1 : 0) << " steps=" << steps.size() << " gflops=" << conv_flops() / 1e9 << "\n";
  static const char* kinds[] = {"conv", "maxpool", "avgpool", "upsample2x"};
  for (const LStep& s : steps) {
    o << kinds[s.kind] << " node=" << s.node << " k=" << s.k << " s=" << s.stride << " cin=" << s.cin << " cout=" << s.cout
      << " in_stride=" << bufs[s.in.buf].stride << " out_stride=" << bufs[s.out.buf].stride;
    if (s.kind == ST_CONV) {
      o << " act=" << act_name(s.act) << " res=" << (s.res.buf >= 0 ? "yes" : "-") << " act_post=" << act_name(s.act_post) << " fused=";
      for (size_t i = 0; i < s.fused.size(); ++i) o << (i ? "," : "") << s.fused[i];
      if (s.fused.empty()) o << "-";
    }
    o << "\n";
  }
  static const char* ok[] = {"score", "bbox", "kps"};
  for (size_t i = 0; i < outs.size(); ++i)
    o << "output " << i << " " << ok[outs[i].kind] << " name=" << outs[i].name << " stride=" << outs[i].stride << " C=" << outs[i].v.C
      << (outs[i].sigmoid ? " sigmoid" : "") << "\n";
  return o.str();
}

Lowered lower(const Graph& g, int n, int det_w, int det_h) {
  // pass 1: channels of every value; pass 2: the same walk with Concat inputs written in place into their slices
  Lowerer p1(g);
  p1.run(n, det_w, det_h);
  Lowerer p2(g);
  for (const Node& nd : g.nodes) {
    if (nd.op != "Concat" || nd.out.empty() || !p1.chan_out.count(nd.out[0])) continue;
    int c = 0;
    for (const std::string& s : nd.in) { p2.concat_dst[s] = {nd.out[0], c}; c += p1.chan_out.count(s) ? p1.chan_out.at(s) : 0; }
  }
  p2.chans = &p1.chan_out;
  p2.run(n, det_w, det_h);
  return std::move(p2.L);
}

}  // namespace onnx
}  // namespace ffp
