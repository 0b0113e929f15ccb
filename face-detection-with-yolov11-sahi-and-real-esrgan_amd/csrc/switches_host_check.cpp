// switches_host_check.cpp — the environment-switch table (switches.hpp) run under AddressSanitizer + UBSan on a CPU-only machine
// (build.py --switches-check). The driver starts from an environment without FFP_ names and checks, for EVERY row of the table:
//   * unset and empty keep the default and report "not from the environment";
//   * every accepted value of the row's rule sets the field: flags 0 and 1; integers lo, hi, the default and one step above lo; the real row 0, a
//     fraction, its default and its upper bound; CU ranges 0-32, 12-32, 0-1 and 31-32;
//   * three refused values raise a SwitchError whose text names the variable and the value: "1x", "0 " (a digit and a space), and "2" — for a row
//     whose rule ACCEPTS 2 (an integer row with 2 in its range, the real row) the third is the first value above its range instead; integer rows
//     are also refused one below lo and, on a coarser step, between two steps; CU ranges with hi > 32, hi <= lo or a negative bound;
// and for the table as a whole:
//   * a parse that fails is not cached: switches_once() throws again while the value stays, and succeeds once it is gone;
//   * a LIVE row follows a setenv between two switches_now(), a ONCE row does not;
//   * FFP_DET_PLAN_GIB=0 still leaves one byte of budget;
//   * an unknown FFP_ZZZ earns exactly one warning line, FFP_LIB none, and the parses of this whole run print that line once;
//   * the report has one line per row, in table order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "switches.hpp"

using namespace ffp;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

// a field as one number (CU range: lo * 100 + hi), and the same number worked out from the text by other means than the parser's
static double as_number(bool v) { return v ? 1 : 0; }
static double as_number(int v) { return v; }
static double as_number(double v) { return v; }
static double as_number(const CuRange& v) { return v.lo * 100 + v.hi; }
static double field_number(const Switches& s, int row) {
  int i = 0;
#define FIELD(type, field, r) if (i++ == row) return as_number(s.field);
  FFP_SWITCH_TABLE(FIELD)
#undef FIELD
  return -1e300;
}
static double text_number(const SwitchRow& r, const char* text) {
  if (r.rule == SwitchRule::CU_RANGE) {
    int lo = 0, hi = 0;
    std::sscanf(text, "%d-%d", &lo, &hi);
    return lo * 100 + hi;
  }
  return std::atof(text);
}
static double default_number(const SwitchRow& r) { return r.rule == SwitchRule::CU_RANGE ? 0 : r.def; }

static void accepts(int row, const std::string& text) {
  const SwitchRow& r = kSwitchRows[row];
  setenv(r.name, text.c_str(), 1);
  try {
    const Switches s = read_switches();
    CHECK(field_number(s, row) == text_number(r, text.c_str()), "%s=\"%s\" read as %g", r.name, text.c_str(), field_number(s, row));
    CHECK(s.from_env[row], "%s=\"%s\" not reported as set", r.name, text.c_str());
    for (int j = 0; j < kSwitchCount; ++j) if (j != row) CHECK(field_number(s, j) == default_number(kSwitchRows[j]) && !s.from_env[j], "%s moved with %s", kSwitchRows[j].name, r.name);
  } catch (const SwitchError& e) {
    CHECK(false, "%s=\"%s\" refused: %s", r.name, text.c_str(), e.what());
  }
  unsetenv(r.name);
}
static void refuses(int row, const std::string& text) {
  const SwitchRow& r = kSwitchRows[row];
  setenv(r.name, text.c_str(), 1);
  try {
    (void)read_switches();
    CHECK(false, "%s=\"%s\" accepted", r.name, text.c_str());
  } catch (const SwitchError& e) {
    const std::string what = e.what();
    CHECK(what.find(std::string(r.name) + "=\"" + text + "\"") != std::string::npos && what.find("takes") != std::string::npos, "%s=\"%s\": message \"%s\"", r.name, text.c_str(), e.what());
  }
  unsetenv(r.name);
}
static void keeps_default(int row) {
  const SwitchRow& r = kSwitchRows[row];
  for (int empty = 0; empty < 2; ++empty) {
    if (empty) setenv(r.name, "", 1);
    else unsetenv(r.name);
    try {
      const Switches s = read_switches();
      CHECK(field_number(s, row) == default_number(r) && !s.from_env[row], "%s %s: %g", r.name, empty ? "empty" : "unset", field_number(s, row));
    } catch (const SwitchError& e) {
      CHECK(false, "%s %s refused: %s", r.name, empty ? "empty" : "unset", e.what());
    }
  }
  unsetenv(r.name);
}

static std::vector<std::string> warning_lines() {
  std::vector<std::string> lines;
  FILE* f = std::tmpfile();
  if (!f) { CHECK(false, "no temporary file"); return lines; }
  warn_unknown_switches(f);
  std::rewind(f);
  char buf[512];
  while (std::fgets(buf, sizeof(buf), f)) lines.push_back(buf);
  std::fclose(f);
  return lines;
}

int main() {
  {      // a clean slate: whatever FFP_ names the caller's environment holds
    std::vector<std::string> names;
    for (char** e = environ; e && *e; ++e)
      if (!std::strncmp(*e, "FFP_", 4)) names.push_back(std::string(*e, std::strcspn(*e, "=")));
    for (const std::string& n : names) unsetenv(n.c_str());
  }

  // unknown names: one line for FFP_ZZZ, none for a name read elsewhere or for a row. The first parse below prints that line to stderr, once.
  CHECK(warning_lines().empty(), "warning in a clean environment");
  setenv("FFP_ZZZ", "1", 1);
  setenv("FFP_LIB", "/nowhere/libffp.so", 1);
  setenv("FFP_NO_TUNE", "1", 1);
  {
    const std::vector<std::string> w = warning_lines();
    CHECK(w.size() == 1 && w[0] == "libffp: environment variable FFP_ZZZ is not a switch of this library\n", "%zu warning lines, first \"%s\"", w.size(), w.empty() ? "" : w[0].c_str());
    const std::vector<std::string> u = unknown_switch_names();
    CHECK(u.size() == 1 && u[0] == "FFP_ZZZ", "%zu unknown names", u.size());
  }
  unsetenv("FFP_NO_TUNE");

  // a failed parse is not cached
  setenv("FFP_PW", "2", 1);
  for (int i = 0; i < 2; ++i) {
    try {
      (void)switches_once();
      CHECK(false, "switches_once() accepted FFP_PW=2 (call %d)", i);
    } catch (const SwitchError& e) {
      CHECK(std::strstr(e.what(), "FFP_PW") != nullptr, "message \"%s\"", e.what());
    }
  }
  unsetenv("FFP_PW");
  unsetenv("FFP_ZZZ");
  unsetenv("FFP_LIB");

  // read once / read live
  bool any_live = false;
  try {
    CHECK(switches_once().pw && switches_once().cls_fuse && !switches_once().no_tune, "defaults at the first read");
    setenv("FFP_PW", "0", 1);
    setenv("FFP_NO_TUNE", "1", 1);
    setenv("FFP_CLS_FUSE", "0", 1);
    CHECK(switches_once().pw && !switches_once().no_tune, "a ONCE row followed the environment");
    Switches now = switches_now();
    CHECK(now.pw && !now.no_tune, "a ONCE row followed the environment in switches_now()");
    CHECK(!now.cls_fuse, "the LIVE row FFP_CLS_FUSE did not follow the environment");
    setenv("FFP_CLS_FUSE", "1", 1);
    CHECK(switches_now().cls_fuse, "the LIVE row did not follow the environment back");
    setenv("FFP_CLS_FUSE", "1x", 1);
    try { (void)switches_now(); CHECK(false, "switches_now() accepted FFP_CLS_FUSE=1x"); } catch (const SwitchError&) {}
    unsetenv("FFP_CLS_FUSE");
    unsetenv("FFP_PW");
    unsetenv("FFP_NO_TUNE");
    // every LIVE row of the table, generically: set to the opposite of its default, it shows in switches_now() and not in switches_once()
    for (int row = 0; row < kSwitchCount; ++row) {
      const SwitchRow& r = kSwitchRows[row];
      const bool flag = r.rule == SwitchRule::FLAG_OFF || r.rule == SwitchRule::FLAG_ON;
      if (!flag) { CHECK(r.when == ONCE, "%s: a LIVE row that is no flag is not covered here", r.name); continue; }
      setenv(r.name, r.def != 0 ? "0" : "1", 1);
      const double once = field_number(switches_once(), row), live = field_number(switches_now(), row);
      CHECK(once == r.def, "%s: switches_once() moved", r.name);
      CHECK(live == (r.when == LIVE ? 1 - r.def : r.def), "%s (%s): switches_now() reads %g", r.name, r.when == LIVE ? "live" : "once", live);
      any_live = any_live || r.when == LIVE;
      unsetenv(r.name);
    }
  } catch (const SwitchError& e) {
    CHECK(false, "clean environment refused: %s", e.what());
  }
  CHECK(any_live, "the table has no LIVE row");

  // every row: defaults, accepted values, refused values
  for (int row = 0; row < kSwitchCount; ++row) {
    const SwitchRow& r = kSwitchRows[row];
    keeps_default(row);
    refuses(row, "1x");
    refuses(row, "0 ");
    switch (r.rule) {
      case SwitchRule::FLAG_OFF:
      case SwitchRule::FLAG_ON:
        accepts(row, "0");
        accepts(row, "1");
        refuses(row, "2");
        refuses(row, "10");
        refuses(row, "01");
        refuses(row, "on");
        break;
      case SwitchRule::INTEGER:
        accepts(row, std::to_string(r.lo));
        accepts(row, std::to_string(r.hi));
        accepts(row, std::to_string((int)r.def));
        accepts(row, std::to_string(r.lo + r.step));
        refuses(row, 2 >= r.lo && 2 <= r.hi && (2 - r.lo) % r.step == 0 ? std::to_string(r.hi + 1) : "2");
        refuses(row, std::to_string(r.lo - 1));
        refuses(row, std::to_string(r.hi + 1));
        if (r.step > 1) refuses(row, std::to_string(r.lo + 1));
        refuses(row, "abc");
        refuses(row, "99999999999999999999");
        break;
      case SwitchRule::REAL:
        accepts(row, "0");
        accepts(row, "0.5");
        accepts(row, "12");
        accepts(row, "100");
        accepts(row, std::to_string(r.hi));
        refuses(row, std::to_string(r.hi + 1));      // in place of "2", which this rule accepts
        refuses(row, "-1");
        refuses(row, "1e3");
        refuses(row, "nan");
        refuses(row, ".");
        break;
      case SwitchRule::CU_RANGE:
        accepts(row, "0-32");
        accepts(row, "12-32");
        accepts(row, "0-1");
        accepts(row, "31-32");
        refuses(row, "2");
        refuses(row, "0-33");
        refuses(row, "5-5");
        refuses(row, "7-3");
        refuses(row, "-1-4");
        refuses(row, "12-32:");
        break;
    }
  }

  // the floor of the plan budget
  setenv("FFP_DET_PLAN_GIB", "0", 1);
  CHECK(read_switches().det_plan_bytes() == 1, "FFP_DET_PLAN_GIB=0: %zu bytes", read_switches().det_plan_bytes());
  setenv("FFP_DET_PLAN_GIB", "100", 1);
  CHECK(read_switches().det_plan_bytes() == (size_t)100 << 30, "FFP_DET_PLAN_GIB=100: %zu bytes", read_switches().det_plan_bytes());
  unsetenv("FFP_DET_PLAN_GIB");
  CHECK(read_switches().det_plan_bytes() == (size_t)64 << 30, "default plan budget: %zu bytes", read_switches().det_plan_bytes());

  // the report: one line per row, in table order, "NAME=value\tsource\twhen\taccepts\teffect"
  {
    setenv("FFP_ROWS16_WS", "32", 1);
    const std::string rep = switches_report(read_switches());
    unsetenv("FFP_ROWS16_WS");
    size_t pos = 0;
    int row = 0;
    while (pos < rep.size() && row < kSwitchCount) {
      const size_t nl = rep.find('\n', pos);
      const std::string line = rep.substr(pos, nl - pos);
      const std::string head = std::string(kSwitchRows[row].name) + "=";
      CHECK(line.compare(0, head.size(), head) == 0, "report line %d: \"%s\"", row, line.c_str());
      int tabs = 0;
      for (char c : line) tabs += c == '\t';
      CHECK(tabs == 4, "report line %d has %d tabs", row, tabs);
      if (!std::strcmp(kSwitchRows[row].name, "FFP_ROWS16_WS")) CHECK(line.compare(0, 21, "FFP_ROWS16_WS=32\tenv\t") == 0, "\"%s\"", line.c_str());
      if (!std::strcmp(kSwitchRows[row].name, "FFP_CLS_FUSE")) CHECK(line.compare(0, 28, "FFP_CLS_FUSE=1\tdefault\tlive\t") == 0, "\"%s\"", line.c_str());
      pos = nl + 1;
      ++row;
    }
    CHECK(row == kSwitchCount && pos == rep.size(), "report has %d lines for %d rows", row, kSwitchCount);
  }

  if (fails) {
    std::printf("switches_host_check: %d FAILED\n", fails);
    return 1;
  }
  std::printf("switches_host_check: %d rows ok\n", kSwitchCount);
  return 0;
}
