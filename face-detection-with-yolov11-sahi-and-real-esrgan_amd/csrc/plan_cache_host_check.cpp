// plan_cache_host_check.cpp — the engines' plan cache (plan_cache.hpp) run under AddressSanitizer + UBSan on a CPU-only machine
// (build.py --plan-cache-check): seeded random get / find / touch / clear sequences, some builds throwing, against a shadow model that
// is a plain vector kept in use order (front: least recently used). After every step:
//   * size() and bytes() equal the shadow's, size() <= max_plans, and bytes() <= max_bytes unless only the fresh plan is resident;
//   * the plans destroyed by the step are exactly the shadow's victims, least recently used first, never the plan the step returned;
//   * every plan is destroyed after a quiesce of the same cache call (FakePlan's destructor looks); a hit, a touch and a clear() of an
//     empty cache do not quiesce;
//   * after a build that throws the key is absent and the evictions made for it stand;
//   * every pointer handed out since the last miss or clear() is written through (a stale one is an ASan report);
//   * a cache that goes out of scope with plans in it destroys each exactly once.
#include <cstdio>
#include <memory>
#include <random>
#include <set>
#include <stdexcept>
#include <vector>

#include "plan_cache.hpp"

using namespace ffp;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static std::set<int> g_live;              // ids of the plans that exist
static std::vector<int> g_destroyed;      // ids destroyed since the current cache call began, in order
static int g_quiesced = 0;                // quiesce calls since the current cache call began
static int g_next_id = 0;

struct FakePlan {
  size_t bytes;
  int id;
  int scribble = 0;
  explicit FakePlan(size_t b) : bytes(b), id(g_next_id++) { g_live.insert(id); }
  ~FakePlan() {
    CHECK(g_quiesced > 0, "plan %d destroyed with no quiesce since the call began", id);
    CHECK(g_live.erase(id) == 1, "plan %d destroyed twice", id);
    g_destroyed.push_back(id);
  }
};

struct Shadow { int key, id; size_t bytes; };

static std::vector<int> make_key(int k, const std::vector<int>*) { return {k % 4, k / 4, 64}; }
static int make_key(int k, const int*) { return k; }

static void begin_call() { g_destroyed.clear(); g_quiesced = 0; }

template <class Key>
static void run(unsigned seed, size_t max_plans, size_t max_bytes, int steps) {
  std::mt19937 rng(seed);
  std::vector<Shadow> sh;                 // use order: front is the least recently used
  std::vector<FakePlan*> handed;          // handed out since the last miss or clear()
  auto sh_bytes = [&] { size_t b = 0; for (const Shadow& s : sh) b += s.bytes; return b; };
  auto sh_find = [&](int k) { for (size_t i = 0; i < sh.size(); ++i) if (sh[i].key == k) return (int)i; return -1; };
  auto sh_use = [&](int i) { const Shadow s = sh[i]; sh.erase(sh.begin() + i); sh.push_back(s); };
  {
    PlanCache<Key, FakePlan> cache(max_plans, max_bytes, [] { ++g_quiesced; });
    for (int step = 0; step < steps; ++step) {
      const int op = (int)(rng() % 100), k = (int)(rng() % 12);
      const Key key = make_key(k, (const Key*)nullptr);
      std::vector<int> victims;
      FakePlan* got = nullptr;
      bool fresh = false;
      begin_call();
      if (op < 60) {                      // get
        const size_t nb = 1 + rng() % 100;
        const bool throws = rng() % 8 == 0;
        const int at = sh_find(k);
        bool built = false;
        auto build = [&] {
          built = true;
          if (throws) throw std::runtime_error("build");
          return std::unique_ptr<FakePlan>(new FakePlan(nb));
        };
        if (at < 0) {
          handed.clear();
          while (sh.size() >= max_plans) { victims.push_back(sh.front().id); sh.erase(sh.begin()); }
        }
        try {
          got = &cache.get(key, build);
          CHECK(!(at < 0 && throws), "step %d: a throwing build returned a plan", step);
        } catch (const std::runtime_error&) {
          CHECK(at < 0 && throws, "step %d: get threw without a throwing build", step);
        }
        CHECK(built == (at < 0), "step %d: build ran %d on a %s", step, (int)built, at < 0 ? "miss" : "hit");
        if (at >= 0) {
          CHECK(got && got->id == sh[at].id, "step %d: the hit is another plan", step);
          sh_use(at);
        } else if (got) {
          fresh = true;
          CHECK(got->bytes == nb, "step %d: the fresh plan is not what build returned", step);
          sh.push_back(Shadow{k, got->id, nb});
          while (max_bytes && sh_bytes() > max_bytes && sh.size() > 1) { victims.push_back(sh.front().id); sh.erase(sh.begin()); }
        } else {
          CHECK(cache.find(key) == nullptr, "step %d: the key of a failed build is resident", step);
        }
      } else if (op < 80) {               // find
        got = cache.find(key);
        const int at = sh_find(k);
        CHECK((got != nullptr) == (at >= 0), "step %d: find of key %d", step, k);
        if (got && at >= 0) { CHECK(got->id == sh[at].id, "step %d: find gave another plan", step); sh_use(at); }
      } else if (op < 95) {               // touch of some resident plan, looked up as an owner would
        if (!sh.empty()) {
          const int at = (int)(rng() % sh.size());
          cache.for_each([&](FakePlan& p) { if (p.id == sh[at].id) got = &p; });
          CHECK(got != nullptr, "step %d: for_each misses plan %d", step, sh[at].id);
          if (got) { cache.touch(*got); sh_use(at); }
        }
      } else {                            // clear
        handed.clear();
        for (const Shadow& s : sh) victims.push_back(s.id);
        sh.clear();
        cache.clear();
        CHECK(g_quiesced == (victims.empty() ? 0 : 1), "step %d: clear() of %zu plans quiesced %d times", step, victims.size(), g_quiesced);
        std::multiset<int> a(victims.begin(), victims.end()), b(g_destroyed.begin(), g_destroyed.end());
        CHECK(a == b, "step %d: clear() destroyed %zu of %zu plans", step, b.size(), a.size());
        victims = g_destroyed;            // any order
      }
      CHECK(g_destroyed == victims, "step %d (op %d): %zu plans destroyed, the shadow evicts %zu (or in another order)", step, op, g_destroyed.size(),
            victims.size());
      CHECK((g_quiesced > 0) == !victims.empty(), "step %d (op %d): %d quiesce calls for %zu destructions", step, op, g_quiesced, victims.size());
      if (got) {
        for (int id : g_destroyed) CHECK(id != got->id, "step %d: the returned plan was destroyed by its own call", step);
        handed.push_back(got);
      }
      for (FakePlan* p : handed) p->scribble += step;
      CHECK(cache.size() == sh.size() && cache.bytes() == sh_bytes(), "step %d: %zu plans / %zu bytes, shadow %zu / %zu", step, cache.size(),
            cache.bytes(), sh.size(), sh_bytes());
      CHECK(cache.size() <= max_plans, "step %d: %zu plans above the limit %zu", step, cache.size(), max_plans);
      // a lone plan above the budget was the fresh one when it went over, and stays (nothing is evicted on a hit)
      CHECK(max_bytes == 0 || cache.bytes() <= max_bytes || cache.size() == 1, "step %d: %zu bytes above the budget %zu", step, cache.bytes(), max_bytes);
      if (fresh) CHECK(cache.find(key) == got, "step %d: the fresh plan is not resident under its key", step);
      CHECK(g_live.size() == sh.size(), "step %d: %zu plans alive, %zu resident", step, g_live.size(), sh.size());
      size_t seen = 0;
      cache.for_each([&](const FakePlan& p) { for (const Shadow& s : sh) seen += s.id == p.id; });
      CHECK(seen == sh.size(), "step %d: for_each visits %zu of %zu plans", step, seen, sh.size());
    }
    // leave through the destructor with plans resident
    begin_call();
    if (sh.empty()) { cache.get(make_key(0, (const Key*)nullptr), [] { return std::unique_ptr<FakePlan>(new FakePlan(1)); }); sh.push_back(Shadow{0, 0, 1}); }
  }
  CHECK(g_live.empty(), "seed %u: %zu plans outlive their cache", seed, g_live.size());
  CHECK(g_destroyed.size() == sh.size(), "seed %u: the destructor destroyed %zu of %zu plans", seed, g_destroyed.size(), sh.size());
}

int main() {
  // {max_plans, max_bytes}: the engines' two policies (8 plans under a budget; 4 plans, no budget), one plan, a budget below a single plan
  const size_t cfg[][2] = {{8, 0}, {4, 0}, {1, 0}, {8, 300}, {8, 120}, {3, 50}, {1, 10}, {8, 1}};
  for (const auto& c : cfg)
    for (unsigned seed = 1; seed <= 4; ++seed) {
      run<std::vector<int>>(seed, c[0], c[1], 3000);
      run<int>(seed + 100, c[0], c[1], 3000);
    }
  std::printf(fails ? "plan_cache_host_check: %d FAILED\n" : "plan_cache_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
