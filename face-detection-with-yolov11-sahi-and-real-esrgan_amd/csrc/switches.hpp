// switches.hpp — the library's environment switches: ONE table, one parser. Plain C++ with no HIP in it (like arena.hpp and plan_cache.hpp), so that
// common.hpp can include it and csrc/switches_host_check.cpp can run it under AddressSanitizer + UBSan on a machine without a GPU.
//
// A row is: the field call sites read, the variable's name, its value rule with default and range, when it is read, and the effect text that
// DESIGN.md (Measurement -> Switches) prints; ffp_switches() reports the same rows with their effective values. getenv appears in this file and
// nowhere else under csrc/.
//
// Value rules. An unset or EMPTY variable keeps the default. Otherwise the whole value must match the row's rule:
//   flag_off / flag_on   exactly "0" or "1" (default off / default on)
//   integer              a decimal integer in [lo, hi] on the row's step
//   real                 a plain decimal number (digits and at most one point) in [0, hi]
//   cu_range             "lo-hi" with 0 <= lo < hi <= 32: CUs lo..hi-1 of every XCD
// Anything else ("10", "1x", "0 ", "on") is a SwitchError that names the variable, the value and what is accepted; the library's sw() (common.hpp)
// turns it into FFP_ERR_ARG. A failed parse is not cached: every later call that reads a switch fails the same way while the environment stays bad.
//
// When. ONCE rows are read at the first library call that reads any switch and hold for the process (switches_once()). LIVE rows are read again by
// every switches_now(): one process can then run both settings (tests/test_gpu_cls_tower_plan.py builds both class-tower plans).
//
// Names. At the first parse every environment variable that begins with FFP_ and is neither a row nor one of kReadElsewhere earns one line on stderr:
// a misspelt switch otherwise measures A against A without a word.
#pragma once
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace ffp {

struct SwitchError : std::invalid_argument { using std::invalid_argument::invalid_argument; };
struct CuRange { int lo = 0, hi = 0; };      // hi == 0: no mask

enum class SwitchRule { FLAG_OFF, FLAG_ON, INTEGER, REAL, CU_RANGE };
enum SwitchWhen { ONCE, LIVE };
struct SwitchRow {
  const char* name;
  SwitchRule rule;
  SwitchWhen when;
  double def;            // INTEGER, REAL (flags: 0 / 1; CU_RANGE: unused, the default is "no mask")
  int lo, hi, step;      // INTEGER; REAL: hi alone
  const char* effect;
};
constexpr SwitchRow flag_off(const char* name, SwitchWhen when, const char* effect) { return {name, SwitchRule::FLAG_OFF, when, 0, 0, 1, 1, effect}; }
constexpr SwitchRow flag_on(const char* name, SwitchWhen when, const char* effect) { return {name, SwitchRule::FLAG_ON, when, 1, 0, 1, 1, effect}; }
constexpr SwitchRow integer(const char* name, int def, int lo, int hi, int step, const char* effect) { return {name, SwitchRule::INTEGER, ONCE, (double)def, lo, hi, step, effect}; }
constexpr SwitchRow real(const char* name, double def, int hi, const char* effect) { return {name, SwitchRule::REAL, ONCE, def, 0, hi, 1, effect}; }
constexpr SwitchRow cu_range(const char* name, const char* effect) { return {name, SwitchRule::CU_RANGE, ONCE, 0, 0, 32, 1, effect}; }

// X(type of the field, field, row). The effect text is DESIGN.md's: tests/test_switches_host.py holds the two sets of names equal.
#define FFP_SWITCH_TABLE(X)                                                                                                                                         \
  X(bool, no_graph, flag_off("FFP_NO_GRAPH", ONCE, "launch every plan eagerly (no hipGraph capture/replay)"))                                                       \
  X(bool, trunk, flag_off("FFP_TRUNK", ONCE, "default of `ffp_sr_set_fused_body` for every new handle: RRDBNet's 345 body convs as ONE persistent launch (`conv_trunk_kernel`); bit-identical, slower than the per-layer launches as measured in round 4: off by default")) \
  X(bool, trunk_dump, flag_off("FFP_TRUNK_DUMP", ONCE, "after every `conv_trunk_kernel` launch, wait for it and print its queue head, error word and debug words to stderr (diagnostic)")) \
  X(double, det_plan_gib, real("FFP_DET_PLAN_GIB", 64.0, 1 << 20, "byte budget in GiB of the resident plans of one YOLO11 (`ffp_det`) or SCRFD (`ffp_scrfd`) handle (`csrc/plan_cache.hpp`); at least one byte: 0 keeps only the plan in use. RT-DETR and the enhancer have no byte budget")) \
  X(bool, det_gate, flag_on("FFP_DET_GATE", ONCE, "default that `ffp_det_set_gate` overrides: 0 runs the pose head's box and keypoint towers for every item instead of only for items with a class score above `conf`; bit-identical results; `ffp_det_last_active` reports active / items of the last call")) \
  X(int, det_arena, integer("FFP_DET_ARENA", 1, 0, 2, 1, "default that `ffp_det_set_buffer_reuse` overrides, activation storage of detector plans: 0 one allocation per tensor, 1 reuse by tensor lifetime, 2 reuse with released ranges overwritten by 0xFF bytes (diagnostic); bit-identical results")) \
  X(int, rows16_ws, integer("FFP_ROWS16_WS", 0, 0, 1024, 1, "workgroups per XCD of `conv_rows16_kernel` (64 = two per CU, 32 = one per CU); 0: the kernel's own choice, 64, or 32 for the weight-resident form")) \
  X(int, k3d_ws, integer("FFP_K3D_WS", 0, 0, 1024, 1, "workgroups per XCD of `conv_k3d_kernel` (32 = one per CU: half of every CU's LDS stays free); 0: the kernel's own choice, 32 times its occupancy")) \
  X(bool, no_tune, flag_off("FFP_NO_TUNE", ONCE, "keep the heuristic workgroup shape instead of timing the valid shapes per plan"))                                 \
  X(bool, tune_log, flag_off("FFP_TUNE_LOG", ONCE, "the plan tuner prints every candidate's time to stderr, one `[tune]` line per (layer, shape)"))                 \
  X(bool, no_fused_stem, flag_off("FFP_NO_FUSED_STEM", ONCE, "separate letterbox kernel + direct stem conv"))                                                       \
  X(bool, no_upfold, flag_off("FFP_NO_UPFOLD", ONCE, "materialise the neck's upsampled tensors (`upsample2x_kernel`) instead of the two-source 1×1 loader"))         \
  X(bool, attn_valu, flag_off("FFP_ATTN_VALU", ONCE, "VALU attention kernel instead of the MFMA one"))                                                              \
  X(bool, dw_strip, flag_off("FFP_DW_STRIP", ONCE, "depthwise 3×3 on the strip kernel instead of the column walk (bit-identical)"))                                 \
  X(bool, rows16, flag_on("FFP_ROWS16", ONCE, "0: Real-ESRGAN body on round 1's `conv_rows_kernel` instead of `conv_rows16_kernel`"))                               \
  X(int, lanes, integer("FFP_LANES", -1, -1, 3, 1, "overrides `ffp_det_set_lanes`: 0 one stream, 1 every branch a lane, 2 one lane per head level, 3 head level 0 only; -1: no override")) \
  X(bool, no_stem_fuse, flag_off("FFP_NO_STEM_FUSE", ONCE, "YOLO11s f32x3 plans keep `stem_from_frame_kernel` + a separate `model.1` launch (stem output stored)")) \
  X(bool, pw, flag_on("FFP_PW", ONCE, "0: the plan tuner does not consider the `conv_pw` shapes (1×1 layers stay on the generic kernel)"))                          \
  X(bool, cls_fuse, flag_on("FFP_CLS_FUSE", LIVE, "0: the class towers run their five launches (`dwconv3x3_col_kernel` + 1×1 convs) instead of the two `conv_dwpw` launches; read at every detector plan build, so one process can hold both plans")) \
  X(bool, k3d, flag_on("FFP_K3D", ONCE, "0: the plan tuner does not consider the `conv_k3d` shapes (3×3 split layers stay on the generic kernel)"))                 \
  X(bool, jpeg_host_huffman, flag_off("FFP_JPEG_HOST_HUFFMAN", ONCE, "every JPEG file is entropy-decoded by the host decoder (`jpeg_dec.cpp`; round-2 behaviour, also the path of streams the device decoder flags)")) \
  X(bool, amax_per_buffer, flag_off("FFP_AMAX_PER_BUFFER", ONCE, "one max-|value| slot per buffer instead of one per image (round-2 behaviour; `f32x3` results then depend on the batch mates in the last bits)")) \
  X(bool, rows16_res, flag_off("FFP_ROWS16_RES", ONCE, "Real-ESRGAN body on the weight-resident form of `conv_rows16_kernel` (one workgroup per CU; measured 0.76–0.89×)")) \
  X(bool, rows16_pc, flag_off("FFP_ROWS16_PC", ONCE, "Real-ESRGAN body on `conv_rows16pc_kernel` (producer / consumer waves, one 8-wave workgroup per CU; measured 0.73–0.95×)")) \
  X(int, rows16_pc_sets, integer("FFP_ROWS16_PC_SETS", 2, 2, 4, 2, "LDS chunk sets of `conv_rows16pc_kernel`: 2 or 4 (4, five chunks ahead, measured slower)")) \
  X(int, alloc_flags, integer("FFP_ALLOC_FLAGS", 0, 0, 3, 1, "`hipExtMallocWithFlags` flags of device buffers of at least 1 MiB (experiment): 0 plain `hipMalloc`, 1 fine-grained, 3 uncached")) \
  X(CuRange, det_cu_mask, cu_range("FFP_DET_CU_MASK", "`lo-hi`: the detector engines' streams (YOLO11, SCRFD, RT-DETR) run on CUs lo..hi-1 of every XCD only (`hipExtStreamCreateWithCUMask`; experiment: a spatial split of the card)")) \
  X(CuRange, sr_cu_mask, cu_range("FFP_SR_CU_MASK", "`lo-hi`: the enhancer's stream runs on CUs lo..hi-1 of every XCD only (the detector's partner in the spatial split)")) \
  X(bool, cu_mask_order, flag_off("FFP_CU_MASK_ORDER", ONCE, "the two CU masks assume the runtime enumerates CUs CU-major (CU i of the mask = CU i / 8 of its XCD) instead of XCD-major"))

// FFP_ names that other parts of the project read (the Python package, bench.py, tools/): no switch of the library, and no warning
constexpr const char* kReadElsewhere[] = {"FFP_LIB", "FFP_LIB_B", "FFP_EXTRA_FLAGS", "FFP_NIQE_PARAMS", "FFP_BENCH_BACKEND", "FFP_BENCH_ONE_DEVICE", "FFP_NONE"};

#define FFP_SWITCH_ROW(type, field, row) row,
constexpr SwitchRow kSwitchRows[] = {FFP_SWITCH_TABLE(FFP_SWITCH_ROW)};
#undef FFP_SWITCH_ROW
constexpr int kSwitchCount = (int)(sizeof(kSwitchRows) / sizeof(kSwitchRows[0]));

struct Switches {
#define FFP_SWITCH_FIELD(type, field, row) type field{};
  FFP_SWITCH_TABLE(FFP_SWITCH_FIELD)
#undef FFP_SWITCH_FIELD
  bool from_env[kSwitchCount] = {};      // per row, in table order: set in the environment (and not empty)
  size_t det_plan_bytes() const { return det_plan_gib * (double)(1ull << 30) < 1.0 ? 1 : (size_t)(det_plan_gib * (double)(1ull << 30)); }
};

inline std::string switch_accepts(const SwitchRow& r) {
  char buf[96];
  switch (r.rule) {
    case SwitchRule::FLAG_OFF: return "0 or 1 (default 0)";
    case SwitchRule::FLAG_ON: return "0 or 1 (default 1)";
    case SwitchRule::INTEGER:
      if (r.step == 1) snprintf(buf, sizeof(buf), "an integer %d..%d (default %d)", r.lo, r.hi, (int)r.def);
      else snprintf(buf, sizeof(buf), "an integer %d..%d in steps of %d (default %d)", r.lo, r.hi, r.step, (int)r.def);
      return buf;
    case SwitchRule::REAL: snprintf(buf, sizeof(buf), "a plain decimal number 0..%d (default %g)", r.hi, r.def); return buf;
    case SwitchRule::CU_RANGE: return "lo-hi with 0 <= lo < hi <= 32 (default: no mask)";
  }
  return "";
}

[[noreturn]] inline void switch_refuse(const SwitchRow& r, const char* e) {
  throw SwitchError(std::string("environment variable ") + r.name + "=\"" + e + "\" is not accepted: " + r.name + " takes " + switch_accepts(r));
}
// a decimal integer that fills the whole of [s, end) and fits [lo, hi]
inline bool switch_int(const char* s, const char* end, int lo, int hi, int* out) {
  const char* p = s;
  if (p < end && *p == '-') ++p;
  if (p == end || end - p > 9) return false;
  for (const char* q = p; q < end; ++q) if (*q < '0' || *q > '9') return false;
  const long v = strtol(s, nullptr, 10);
  if (v < lo || v > hi) return false;
  *out = (int)v;
  return true;
}
inline void switch_parse(const SwitchRow& r, const char* e, bool* v) {
  if (!e[0] || e[1] || (e[0] != '0' && e[0] != '1')) switch_refuse(r, e);
  *v = e[0] == '1';
}
inline void switch_parse(const SwitchRow& r, const char* e, int* v) {
  if (!switch_int(e, e + strlen(e), r.lo, r.hi, v) || (*v - r.lo) % r.step) switch_refuse(r, e);
}
inline void switch_parse(const SwitchRow& r, const char* e, double* v) {
  char* end = nullptr;
  const bool plain = strspn(e, "0123456789.") == strlen(e);      // no sign, space, exponent, "inf", "nan" or hex
  const double d = plain ? strtod(e, &end) : 0.0;
  if (!plain || end == e || *end || !(d <= r.hi)) switch_refuse(r, e);
  *v = d;
}
inline void switch_parse(const SwitchRow& r, const char* e, CuRange* v) {
  const char* dash = strchr(e, '-');
  if (!dash || !switch_int(e, dash, 0, 31, &v->lo) || !switch_int(dash + 1, e + strlen(e), 1, 32, &v->hi) || v->hi <= v->lo) switch_refuse(r, e);
}
inline void switch_default(const SwitchRow& r, bool* v) { *v = r.def != 0; }
inline void switch_default(const SwitchRow& r, int* v) { *v = (int)r.def; }
inline void switch_default(const SwitchRow& r, double* v) { *v = r.def; }
inline void switch_default(const SwitchRow&, CuRange* v) { *v = CuRange{}; }

// every FFP_ name of the environment that is neither a row nor read elsewhere, in the environment's order
inline std::vector<std::string> unknown_switch_names() {
  std::vector<std::string> out;
  for (char** e = environ; e && *e; ++e) {
    if (strncmp(*e, "FFP_", 4) != 0) continue;
    const char* eq = strchr(*e, '=');
    const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
    bool known = false;
    for (const SwitchRow& r : kSwitchRows) known = known || name == r.name;
    for (const char* k : kReadElsewhere) known = known || name == k;
    if (!known) out.push_back(name);
  }
  return out;
}
inline int warn_unknown_switches(FILE* to) {
  const std::vector<std::string> names = unknown_switch_names();
  for (const std::string& n : names) fprintf(to, "libffp: environment variable %s is not a switch of this library\n", n.c_str());
  return (int)names.size();
}

// A fresh parse of the whole table; only_live: the LIVE rows alone, the others keep what `s` holds.
inline void read_switches(Switches& s, bool only_live = false) {
  static std::atomic<bool> warned{false};
  if (!warned.exchange(true)) warn_unknown_switches(stderr);
  int i = 0;
#define FFP_SWITCH_READ(type, field, row)                             \
  if (!only_live || kSwitchRows[i].when == LIVE) {                    \
    const char* e = getenv(kSwitchRows[i].name);                      \
    s.from_env[i] = e && e[0];                                        \
    if (s.from_env[i]) switch_parse(kSwitchRows[i], e, &s.field);     \
    else switch_default(kSwitchRows[i], &s.field);                    \
  }                                                                   \
  ++i;
  FFP_SWITCH_TABLE(FFP_SWITCH_READ)
#undef FFP_SWITCH_READ
}
inline Switches read_switches() { Switches s; read_switches(s); return s; }

// The process's switches as first read. A parse that throws leaves the static uninitialised (C++ retries it at the next call), so nothing bad is cached.
// A LIVE row holds its value at that first read here: its call sites use switches_now().
inline const Switches& switches_once() {
  static const Switches s = read_switches();
  return s;
}
// switches_once() with every LIVE row read again: what a plan build that honours a LIVE row, and ffp_switches(), look at.
inline Switches switches_now() {
  Switches s = switches_once();
  read_switches(s, true);
  return s;
}

inline std::string switch_value(bool v) { return v ? "1" : "0"; }
inline std::string switch_value(int v) { return std::to_string(v); }
inline std::string switch_value(double v) { char b[32]; snprintf(b, sizeof(b), "%g", v); return b; }
inline std::string switch_value(const CuRange& v) { return v.hi ? std::to_string(v.lo) + "-" + std::to_string(v.hi) : "none"; }

// One line per row: NAME=value <tab> env|default <tab> once|live <tab> accepted values <tab> effect
inline std::string switches_report(const Switches& s) {
  std::string out;
  int i = 0;
#define FFP_SWITCH_LINE(type, field, row)                                                                                             \
  out += std::string(kSwitchRows[i].name) + "=" + switch_value(s.field) + "\t" + (s.from_env[i] ? "env" : "default") + "\t" +         \
         (kSwitchRows[i].when == LIVE ? "live" : "once") + "\t" + switch_accepts(kSwitchRows[i]) + "\t" + kSwitchRows[i].effect + "\n"; \
  ++i;
  FFP_SWITCH_TABLE(FFP_SWITCH_LINE)
#undef FFP_SWITCH_LINE
  return out;
}

}  // namespace ffp
