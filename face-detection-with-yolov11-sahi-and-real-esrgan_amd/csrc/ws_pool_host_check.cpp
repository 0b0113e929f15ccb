// ws_pool_host_check.cpp — the codecs' workspace pool (ws_pool.hpp) on a CPU-only machine (build.py --ws-pool-check builds this driver twice:
// under AddressSanitizer + UBSan and under ThreadSanitizer).
// 1. Seeded single-thread sequences of acquire / resize / release over three fake devices against a shadow model (the kept workspaces in the
//    pool's order), for the library's five policies and a few small ones; some constructors throw, some quiesce calls throw, some releases
//    happen through unwinding. After every step:
//      * the kept workspaces are exactly the shadow's; at most max_kept; per device at most one above one_big_above; none above drop_above;
//      * a lease for device d yields a workspace of device d: the first kept one of d, a fresh one only when none is kept;
//      * destroy ran exactly once for the workspace the step did not keep, and for no other;
//      * a release through unwinding ran quiesce before the pool looked at the workspace; a release on the normal path did not run it;
//      * a workspace whose quiesce threw was destroyed, not kept; a throwing constructor left kept and leased sets unchanged;
//      * made - destroyed == kept + leased.
// 2. Eight threads, 2 000 acquire / touch / release rounds each over two fake devices and a policy that keeps three: a workspace's holder
//    count only ever goes 0 -> 1 -> 0, and at the end made - destroyed == kept <= max_kept.
#include <atomic>
#include <cstdio>
#include <deque>
#include <memory>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "ws_pool.hpp"

using namespace ffp;

static std::atomic<int> fails{0};
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static std::atomic<long long> g_made{0}, g_destroyed{0};
static std::atomic<int> g_next_id{0};
static bool g_ctor_throws = false;         // single-thread phase only
static std::vector<int> g_destroyed_ids;   // single-thread phase only: ids destroyed since the step began

struct FakeWs {
  int device = -1;
  size_t bytes = 0;
  int id;
  std::atomic<int> holders{0};
  int scribble = 0;
  const int* quiesced_first = nullptr;     // set for a release through unwinding: the pool may look at the workspace only after quiesce ran
  FakeWs() {
    if (g_ctor_throws) throw std::runtime_error("constructor");
    id = g_next_id++;
    ++g_made;
  }
  size_t held() const {
    if (quiesced_first) CHECK(*quiesced_first > 0, "workspace %d went back before its quiesce", id);
    return bytes;
  }
};
using Pool = WsPool<FakeWs>;

struct Shadow { int id, device; size_t bytes; };
struct Held {
  std::unique_ptr<Pool::Lease> lease;
  int id, device;
  int* quiesced;                           // how often this lease's quiesce ran
  bool* quiesce_throws;
};

static void run(unsigned seed, WsPolicy pol, const std::vector<size_t>& sizes, int steps) {
  std::mt19937 rng(seed);
  std::vector<Shadow> kept;                // the pool's order: a return goes to the back, a lease takes the first of its device
  std::vector<Held> leased;
  std::set<int> live;
  std::deque<int> counters;                // one per acquire, alive for the whole run: FakeWs::quiesced_first may point at one
  std::deque<bool> throw_flags;
  const size_t max_out = pol.max_kept + 4;
  {
    Pool pool(pol, [&](FakeWs* w) {
      CHECK(w->holders.load() == 0, "workspace %d destroyed while held", w->id);
      CHECK(live.erase(w->id) == 1, "workspace %d destroyed twice", w->id);
      g_destroyed_ids.push_back(w->id);
      ++g_destroyed;
      delete w;
    });
    bool grow = true;
    for (int step = 0; step < steps; ++step) {
      if (step % 97 == 0) grow = rng() % 2;
      const int op = (int)(rng() % 100);
      g_destroyed_ids.clear();
      std::vector<int> victims;
      const long long made0 = g_made.load();
      if (op < (grow ? 55 : 20) && leased.size() < max_out) {          // acquire
        const int d = (int)(rng() % 3);
        g_ctor_throws = rng() % 6 == 0;
        int at = -1;
        for (size_t i = 0; i < kept.size() && at < 0; ++i)
          if (kept[i].device == d) at = (int)i;
        Held h;
        counters.push_back(0);
        throw_flags.push_back(false);
        int* q = h.quiesced = &counters.back();
        bool* qt = h.quiesce_throws = &throw_flags.back();
        bool threw = false;
        try {
          h.lease.reset(new Pool::Lease(pool.acquire(d, [q, qt] { ++*q; if (*qt) throw std::runtime_error("quiesce"); })));
        } catch (const std::runtime_error&) {
          threw = true;
        }
        CHECK(threw == (at < 0 && g_ctor_throws), "step %d: acquire threw %d (kept one at %d, constructor throws %d)", step, (int)threw, at, (int)g_ctor_throws);
        g_ctor_throws = false;
        if (!threw) {
          FakeWs& w = **h.lease;
          w.quiesced_first = nullptr;
          CHECK(w.device == d, "step %d: a lease for device %d gave a workspace of device %d", step, d, w.device);
          if (at >= 0) {
            CHECK(w.id == kept[at].id && g_made.load() == made0, "step %d: workspace %d kept for device %d, the lease gave %d (%lld made)", step, kept[at].id, d, w.id,
                  g_made.load() - made0);
            kept.erase(kept.begin() + at);
          } else {
            CHECK(g_made.load() == made0 + 1 && live.insert(w.id).second, "step %d: a miss made %lld workspaces", step, g_made.load() - made0);
          }
          CHECK(w.holders.fetch_add(1) == 0, "step %d: workspace %d handed out twice", step, w.id);
          h.id = w.id; h.device = d;
          leased.push_back(std::move(h));
        } else {
          CHECK(g_made.load() == made0, "step %d: a throwing constructor made a workspace", step);
        }
      } else if (op < 70) {                                             // resize
        if (!leased.empty()) {
          FakeWs& w = **leased[rng() % leased.size()].lease;
          w.bytes = sizes[rng() % sizes.size()];
          w.scribble += step;
        }
      } else if (!leased.empty()) {                                     // release
        const size_t i = rng() % leased.size();
        Held h = std::move(leased[i]);
        leased.erase(leased.begin() + i);
        FakeWs& w = **h.lease;
        const size_t b = w.bytes;
        const bool unwind = rng() % 3 == 0;
        *h.quiesce_throws = unwind && rng() % 3 == 0;
        bool keep = !*h.quiesce_throws && !(pol.drop_above && b > pol.drop_above) && kept.size() < pol.max_kept;
        if (pol.one_big_above && b > pol.one_big_above)
          for (const Shadow& s : kept) keep = keep && !(s.device == h.device && s.bytes > pol.one_big_above);
        if (keep) kept.push_back(Shadow{h.id, h.device, b}); else victims.push_back(h.id);
        CHECK(w.holders.fetch_sub(1) == 1, "step %d: workspace %d released while not held once", step, h.id);
        if (unwind) {
          w.quiesced_first = h.quiesced;
          try {
            std::unique_ptr<Pool::Lease> going = std::move(h.lease);
            throw std::runtime_error("caller");
          } catch (const std::runtime_error& e) {
            CHECK(e.what() == std::string("caller"), "step %d: the quiesce's exception escaped the lease", step);
          }
          CHECK(*h.quiesced == 1, "step %d: a release through unwinding ran quiesce %d times", step, *h.quiesced);
        } else {
          h.lease.reset();
          CHECK(*h.quiesced == 0, "step %d: a release on the normal path ran quiesce", step);
        }
      }
      CHECK(g_destroyed_ids == victims, "step %d (op %d): %zu workspaces destroyed, the shadow frees %zu", step, op, g_destroyed_ids.size(), victims.size());
      std::vector<Shadow> seen;
      pool.for_each_kept([&](const FakeWs& k) { seen.push_back(Shadow{k.id, k.device, k.bytes}); });
      CHECK(pool.kept() == kept.size() && seen.size() == kept.size(), "step %d: %zu kept, shadow %zu", step, pool.kept(), kept.size());
      for (size_t i = 0; i < seen.size() && i < kept.size(); ++i)
        CHECK(seen[i].id == kept[i].id && seen[i].device == kept[i].device && seen[i].bytes == kept[i].bytes, "step %d: kept workspace %zu is %d, shadow %d", step, i,
              seen[i].id, kept[i].id);
      CHECK(seen.size() <= pol.max_kept, "step %d: %zu kept above the limit %zu", step, seen.size(), pol.max_kept);
      int big[3] = {0, 0, 0};
      for (const Shadow& s : seen) {
        CHECK(!(pol.drop_above && s.bytes > pol.drop_above), "step %d: workspace %d of %zu bytes is kept above %zu", step, s.id, s.bytes, pol.drop_above);
        if (pol.one_big_above && s.bytes > pol.one_big_above) ++big[s.device];
      }
      for (int d = 0; d < 3; ++d) CHECK(big[d] <= 1, "step %d: %d big workspaces kept for device %d", step, big[d], d);
      CHECK(g_made.load() - g_destroyed.load() == (long long)(kept.size() + leased.size()) && live.size() == kept.size() + leased.size(),
            "step %d: %lld alive, %zu kept + %zu leased", step, g_made.load() - g_destroyed.load(), kept.size(), leased.size());
    }
    // leave with leases out and workspaces kept: the leases go first, then the pool destroys what it keeps
    for (Held& h : leased) (*h.lease)->holders.fetch_sub(1);
    leased.clear();
  }
  CHECK(live.empty() && g_made.load() == g_destroyed.load(), "seed %u: %zu workspaces outlive their pool", seed, live.size());
}

static void threaded() {
  const WsPolicy pol{3, 50, 100};
  const long long made0 = g_made.load(), destroyed0 = g_destroyed.load();
  {
    Pool pool(pol, [](FakeWs* w) {
      CHECK(w->holders.load() == 0, "workspace %d destroyed while held", w->id);
      ++g_destroyed;
      delete w;
    });
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t)
      ts.emplace_back([&pool, t] {
        std::mt19937 rng(1000u + (unsigned)t);
        for (int round = 0; round < 2000; ++round) {
          const int d = (int)(rng() % 2);
          const bool unwind = rng() % 5 == 0, q_throws = rng() % 11 == 0;
          int quiesced = 0;
          try {
            auto lease = pool.acquire(d, [&quiesced, q_throws] { ++quiesced; if (q_throws) throw std::runtime_error("quiesce"); });
            CHECK(lease->device == d, "a lease for device %d gave a workspace of device %d", d, lease->device);
            CHECK(lease->holders.fetch_add(1) == 0, "workspace %d has two holders", lease->id);
            lease->scribble += round;
            lease->bytes = rng() % 130;
            if (rng() % 4 == 0) std::this_thread::yield();
            CHECK(lease->holders.fetch_sub(1) == 1, "workspace %d lost its holder", lease->id);
            if (unwind) throw std::runtime_error("caller");
          } catch (const std::runtime_error&) {
          }
          CHECK(quiesced == (unwind ? 1 : 0), "quiesce ran %d times (unwinding %d)", quiesced, (int)unwind);
        }
      });
    for (std::thread& t : ts) t.join();
    const long long alive = (g_made.load() - made0) - (g_destroyed.load() - destroyed0);
    CHECK(alive == (long long)pool.kept() && pool.kept() <= pol.max_kept, "threads done: %lld alive, %zu kept (limit %zu)", alive, pool.kept(), pol.max_kept);
    int big[2] = {0, 0};
    pool.for_each_kept([&](const FakeWs& k) {
      CHECK(k.bytes <= pol.drop_above && k.holders.load() == 0, "workspace %d kept with %zu bytes, %d holders", k.id, k.bytes, k.holders.load());
      if (k.bytes > pol.one_big_above) ++big[k.device];
    });
    CHECK(big[0] <= 1 && big[1] <= 1, "threads done: %d + %d big workspaces kept", big[0], big[1]);
  }
  CHECK(g_made.load() - made0 == g_destroyed.load() - destroyed0, "threads done: %lld workspaces outlive their pool",
        (g_made.load() - made0) - (g_destroyed.load() - destroyed0));
}

int main() {
  const size_t MB = 1000u * 1000u, MiB = 1u << 20;
  // the library's five policies (batch JPEG decode; the host decoder's staging; PNG decode, JPEG encode, PNG encode), with sizes around their limits ...
  const std::vector<size_t> real = {0, 1 * MiB, 100 * MiB, 160 * MiB, 160 * MiB + 1, 500 * MiB, 768 * MiB, 768 * MiB + 1, 3000 * MB};
  const WsPolicy lib[] = {{32, 160 * MiB, 0}, {32, 0, 0}, {8, 0, 768 * MiB}, {8, 0, 768 * MiB}, {8, 0, 768 * MiB}};
  // ... and small ones, so that every rule decides often
  const std::vector<size_t> small = {0, 3, 5, 6, 9, 10, 11, 20, 21, 40};
  const WsPolicy tiny[] = {{3, 10, 0}, {3, 0, 20}, {2, 5, 9}, {1, 0, 0}, {4, 5, 20}};
  int steps = 0;
  for (unsigned seed = 1; seed <= 2; ++seed) {
    for (const WsPolicy& p : lib) { run(seed, p, real, 1500); steps += 1500; }
    for (const WsPolicy& p : tiny) { run(seed + 100, p, small, 1500); steps += 1500; }
  }
  threaded();
  std::printf("%d single-thread steps, 8 x 2000 threaded rounds\n", steps);
  std::printf(fails ? "ws_pool_host_check: %d FAILED\n" : "ws_pool_host_check: ok\n", fails.load());
  return fails ? 1 : 0;
}
