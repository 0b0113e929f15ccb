// arena_host_check.cpp — host driver of the lifetime pool (arena.hpp) for a build with -fsanitize=address,undefined. No HIP.
//
// Blocks are real host memory, so a range outside its block is a sanitizer report as well as a failed check: every tensor's bytes are
// written with a tag at alloc and read back at release. A shadow model kept beside the pool (what is live, what is held back by an
// open fork, the peak of the live bytes) is compared with it after every operation. Exit status 0 and the line "arena ok" only if
// nothing was violated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "arena.hpp"

namespace {

using ffp::Arena;

struct Tally { long held = 0, flushing_joins = 0, refused_joins = 0, bad = 0; int max_depth = 0; } tally;

struct Shadow { uintptr_t addr; size_t nb; int state; unsigned char tag; };    // state as Arena::Tensor::state

[[noreturn]] void fail(unsigned seed, long op, const char* what) {
  std::printf("arena check FAILED (seed %u, operation %ld): %s\n", seed, op, what);
  std::exit(1);
}

struct Host {
  std::vector<void*> mem;
  std::vector<size_t> sizes;
  size_t total = 0;
  ~Host() { for (void* p : mem) std::free(p); }
  uintptr_t get(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, Arena::ALIGN, n) != 0) return 0;
    mem.push_back(p); sizes.push_back(n); total += n;
    return reinterpret_cast<uintptr_t>(p);
  }
};

// Shares of the operations per hundred: 40 alloc, 40 release (`releases` = false: none, the share goes to bad releases), 5 bad releases,
// 7 fork, 8 join (`lanes` = false: neither, the share goes to bad releases). The open-fork count is a random walk held at zero: forks
// nest, stay open for stretches of hundreds of operations, and come back to zero (where a join must be refused) again and again.
long run(unsigned seed, long n_ops, bool reuse, bool releases, bool lanes) {
  Host host;
  Arena a([&host](size_t n) { return host.get(n); }, reuse);
  std::mt19937 rng(seed);
  std::vector<Shadow> sh;
  std::vector<int> live, held_order;
  int forks = 0;
  size_t live_bytes = 0, peak = 0, sum = 0;
  long op = 0;
  auto rnd = [&](unsigned n) { return (unsigned)(rng() % n); };
  for (; op < n_ops; ++op) {
    const unsigned k = rnd(100);
    if (k < 40 || (live.empty() && k < 80)) {                                                 // ---- alloc
      size_t nb;
      switch (rnd(4)) {
        case 0: nb = 1 + rnd(700); break;
        case 1: nb = 256 * (1 + rnd(64)); break;
        case 2: nb = 256 * (1 + rnd(64)) + 256; break;                            // the plan's shape: payload + 256 slack
        default: nb = 1 + rnd(70000); break;
      }
      const int blocks_before = a.blocks();
      const int id = a.alloc(nb);
      if (id != (int)sh.size()) fail(seed, op, "alloc did not return the next id");
      const uintptr_t p = a.addr(id);
      if (p % Arena::ALIGN != 0) fail(seed, op, "range not 256-byte aligned");
      const Arena::Tensor& t = a.tensor(id);
      if (t.nb != nb || t.span < nb || t.state != 0) fail(seed, op, "tensor record wrong");
      if (t.block < 0 || t.block >= a.blocks()) fail(seed, op, "block index out of range");
      const uintptr_t b0 = a.block_base(t.block), b1 = b0 + a.block_size(t.block);
      if (p < b0 || p + t.span > b1) fail(seed, op, "range outside its block");
      if (!reuse && a.blocks() != blocks_before + 1) fail(seed, op, "reuse off: tensor without a block of its own");
      for (const Shadow& s : sh)
        if (s.state != 2 && p < s.addr + s.nb && s.addr < p + nb)
          fail(seed, op, s.state == 1 ? "range released under an open fork handed out before the last join" : "two live ranges overlap");
      const unsigned char tag = (unsigned char)(1 + id % 250);
      std::memset(reinterpret_cast<void*>(p), tag, nb);
      sh.push_back(Shadow{p, nb, 0, tag});
      live.push_back(id);
      live_bytes += nb; sum += nb;
      if (live_bytes > peak) peak = live_bytes;
    } else if (k < 80 && releases) {                                 // ---- release
      const unsigned j = rnd((unsigned)live.size());
      const int id = live[j];
      live[j] = live.back(); live.pop_back();
      const unsigned char* q = reinterpret_cast<const unsigned char*>(sh[id].addr);
      for (size_t i = 0; i < sh[id].nb; ++i) if (q[i] != sh[id].tag) fail(seed, op, "a live tensor's bytes were overwritten");
      const Arena::Release r = a.release(id);
      if (forks > 0) {
        if (r != Arena::HELD) fail(seed, op, "release under an open fork was not held back");
        sh[id].state = 1; held_order.push_back(id); ++tally.held;
      } else {
        if (r != Arena::FREED) fail(seed, op, "release without an open fork did not free");
        sh[id].state = 2; live_bytes -= sh[id].nb;
      }
      if (a.release(id) != Arena::REJECTED) fail(seed, op, "second release accepted");
    } else if (k < 85 || !lanes) {                                                // ---- bad releases
      ++tally.bad;
      if (a.release(-1) != Arena::REJECTED || a.release((int)sh.size()) != Arena::REJECTED) fail(seed, op, "release of an unknown id accepted");
      if (!sh.empty()) {
        const int id = (int)rnd((unsigned)sh.size());
        if (sh[id].state != 0 && a.release(id) != Arena::REJECTED) fail(seed, op, "second release accepted");
      }
    } else if (k < 92) {                                                          // ---- fork
      a.fork(); ++forks;
      if (forks > tally.max_depth) tally.max_depth = forks;
    } else {                                                                      // ---- join
      std::vector<int> flushed;
      const bool ok = a.join(&flushed);
      if (forks == 0) {
        if (ok) fail(seed, op, "join without an open fork accepted");
        ++tally.refused_joins;
      } else {
        if (!ok) fail(seed, op, "join refused");
        if (--forks == 0) {
          if (flushed != held_order) fail(seed, op, "the last join did not let go exactly the held ranges, in release order");
          for (int id : held_order) { sh[id].state = 2; live_bytes -= sh[id].nb; }
          held_order.clear(); ++tally.flushing_joins;
        } else if (!flushed.empty()) {
          fail(seed, op, "a join let ranges go while another fork was open");
        }
      }
    }
    // ---- invariants after every operation
    if (a.forks_open() != forks) fail(seed, op, "fork count");
    if (a.held_bytes() != host.total) fail(seed, op, "held bytes differ from the blocks handed over");
    if (a.sum_sizes() != sum) fail(seed, op, "sum of sizes");
    if (a.live_bytes() != live_bytes) fail(seed, op, "live bytes differ from the shadow model");
    if (a.peak_live_bytes() != peak) fail(seed, op, "peak-live bytes differ from the shadow model");
    if (a.held_bytes() < a.peak_live_bytes()) fail(seed, op, "held bytes below peak-live bytes");
    if (!reuse && a.held_bytes() != sum) fail(seed, op, "reuse off: held bytes differ from the sum of the sizes");
    if (!releases && a.held_bytes() != sum) fail(seed, op, "no release: held bytes differ from the sum of the sizes");
    if (a.tensors() != (int)sh.size()) fail(seed, op, "tensor count");
    if (op % 64 == 0 || op + 1 == n_ops)                                          // every tensor, not only the one just touched
      for (int i = 0; i < (int)sh.size(); ++i)
        if (a.tensor(i).state != sh[i].state) fail(seed, op, "tensor state differs from the shadow model");
  }
  // the closing balance, from the tensors' final states alone
  size_t still = 0;
  for (const Shadow& s : sh) if (s.state != 2) still += s.nb;
  if (still != a.live_bytes()) fail(seed, op, "closing balance of live bytes");
  return (long)sh.size();
}

void fixed_cases() {
  const unsigned S = 0;
  {   // split, coalesce in every order, best fit
    Host host;
    Arena a([&host](size_t n) { return host.get(n); }, true);
    const int big = a.alloc(4096), mid = a.alloc(1024);
    if (a.release(big) != Arena::FREED || a.release(mid) != Arena::FREED) fail(S, 0, "fixed: release");
    const int x = a.alloc(1000);                                  // best fit: the 1024 block, not the 4096 one
    if (a.tensor(x).block != a.tensor(mid).block) fail(S, 1, "fixed: not best fit");
    const int p = a.alloc(256), q = a.alloc(300), r = a.alloc(3000);      // 256 + 512 + 3072 of the 4096 block, 256 left
    if (a.blocks() != 2 || a.tensor(p).block != 0 || a.tensor(q).off != 256 || a.tensor(r).off != 768) fail(S, 2, "fixed: split");
    if (a.release(p) != Arena::FREED || a.release(r) != Arena::FREED || a.release(q) != Arena::FREED) fail(S, 3, "fixed: release");
    const int w = a.alloc(4096);                                  // only fits if the four pieces coalesced
    if (a.blocks() != 2 || a.tensor(w).block != 0 || a.tensor(w).off != 0) fail(S, 4, "fixed: free neighbours did not coalesce");
    if (a.held_bytes() != 4096 + 1024 || a.peak_live_bytes() != 4096 + 1024) fail(S, 5, "fixed: counters");
  }
  {   // a range released under a fork stays out of reach until the LAST join
    Host host;
    Arena a([&host](size_t n) { return host.get(n); }, true);
    const int t = a.alloc(2048);
    a.fork(); a.fork();
    if (a.release(t) != Arena::HELD) fail(S, 10, "fixed: not held");
    const int u = a.alloc(2048);
    if (a.tensor(u).block == a.tensor(t).block) fail(S, 11, "fixed: held range handed out");
    std::vector<int> fl;
    if (!a.join(&fl) || !fl.empty()) fail(S, 12, "fixed: first join");
    const int v = a.alloc(2048);
    if (a.tensor(v).block == a.tensor(t).block) fail(S, 13, "fixed: held range handed out after the first of two joins");
    if (!a.join(&fl) || fl.size() != 1 || fl[0] != t) fail(S, 14, "fixed: last join");
    const int w = a.alloc(2048);
    if (a.tensor(w).block != a.tensor(t).block) fail(S, 15, "fixed: range not reusable after the last join");
    if (a.join(nullptr)) fail(S, 16, "fixed: join without fork");
  }
  {   // a block whose base is not aligned is refused
    Arena a([](size_t) { return (uintptr_t)0x1010; }, true);
    if (a.alloc(64) != -1) fail(S, 20, "fixed: unaligned block accepted");
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long n_ops = argc > 1 ? std::atol(argv[1]) : 12000;
  fixed_cases();
  long tensors = 0, ops = 0;
  for (unsigned seed = 1; seed <= 6; ++seed) {
    tensors += run(seed, n_ops, true, true, true);          // reuse, forks and joins
    tensors += run(seed + 100, n_ops, true, true, false);   // reuse, lanes off: nothing is ever held back
    tensors += run(seed + 200, n_ops / 4, false, true, true);       // reuse off: a block per tensor, lifetimes still counted
    tensors += run(seed + 300, n_ops / 8, true, false, true);         // never released: held == sum of sizes
    ops += 2 * n_ops + n_ops / 4 + n_ops / 8;
  }
  std::printf("arena ok: %ld operations, %ld tensors, 24 seeded runs; %ld releases held back, %ld joins that let ranges go, %ld joins refused, "
              "%ld rounds of bad releases, forks nested %d deep\n", ops, tensors, tally.held, tally.flushing_joins, tally.refused_joins, tally.bad, tally.max_depth);
  if (tally.held < 1000 || tally.flushing_joins < 100 || tally.refused_joins < 100 || tally.bad < 1000 || tally.max_depth < 3) {
    std::printf("arena check FAILED: the sequences did not cover the held-back path\n");
    return 1;
  }
  return 0;
}
