// ws_pool.hpp — the one pool of scratch workspaces behind the JPEG and PNG encoders and decoders. A call borrows a workspace of the current
// device for its length (a Lease), so calls on different threads run side by side, and idle workspaces are kept for the next call under a
// policy of three numbers. No HIP in here, so the same code runs under the host sanitizers (ws_pool_host_check.cpp); what is HIP about it —
// freeing with the owner device current, waiting for the stream — comes in as the two callables (common.hpp: lease_ws, delete_on_owner_device).
//
// THE RULE: no workspace returns to the pool with work in flight. The next borrower would overwrite staging that queued copies still read.
// A caller's straight-line path ends in its own stream synchronisation; a Lease that is left by an exception runs `quiesce` (wait for the
// stream) before it gives the workspace back, and a workspace whose quiesce throws is destroyed, never kept.
#pragma once
#include <cstddef>
#include <exception>
#include <functional>
#include <mutex>
#include <utility>
#include <vector>

namespace ffp {

struct WsPolicy {
  size_t max_kept;        // idle workspaces kept, over all devices
  size_t one_big_above;   // per device at most one kept workspace holds more than this many bytes; 0: no such rule
  size_t drop_above;      // a workspace that holds more than this many bytes is never kept; 0: no such rule
};

template <class W>        // W needs: a default constructor, int device, size_t held() const (bytes it holds, device plus pinned)
class WsPool {
 public:
  // destroy(w) runs outside the lock for every workspace the pool does not keep; it must not throw
  WsPool(WsPolicy policy, std::function<void(W*)> destroy) : policy_(policy), destroy_(std::move(destroy)) {
    free_.reserve(policy_.max_kept);      // a return to the pool never allocates
  }
  WsPool(const WsPool&) = delete;
  WsPool& operator=(const WsPool&) = delete;
  ~WsPool() {
    for (W* w : free_) destroy_(w);
  }

  class Lease {
   public:
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    ~Lease() {
      bool settled = true;
      if (std::uncaught_exceptions() > entered_) {       // the scope is being left by an exception: work may still be queued
        try { quiesce_(); } catch (...) { settled = false; }
      }
      pool_.give_back(w_, settled);
    }
    W* operator->() const { return w_; }
    W& operator*() const { return *w_; }

   private:
    friend class WsPool;
    Lease(WsPool& pool, W* w, std::function<void()> quiesce)
        : pool_(pool), w_(w), quiesce_(std::move(quiesce)), entered_(std::uncaught_exceptions()) {}
    WsPool& pool_;
    W* const w_;
    std::function<void()> quiesce_;
    const int entered_;
  };

  // a kept workspace of `device`, or a fresh W with `device` set. A W constructor that throws leaves the pool as it was.
  Lease acquire(int device, std::function<void()> quiesce) {
    W* w = nullptr;
    {
      std::lock_guard<std::mutex> lock(mu_);
      for (size_t i = 0; i < free_.size() && !w; ++i)
        if (free_[i]->device == device) { w = free_[i]; free_.erase(free_.begin() + i); }
    }
    if (!w) { w = new W(); w->device = device; }
    return Lease(*this, w, std::move(quiesce));
  }

  size_t kept() const {
    std::lock_guard<std::mutex> lock(mu_);
    return free_.size();
  }
  template <class F>
  void for_each_kept(F&& f) const {       // f(const W&) under the lock
    std::lock_guard<std::mutex> lock(mu_);
    for (const W* w : free_) f(*w);
  }

 private:
  void give_back(W* w, bool settled) {
    const size_t held = w->held();
    bool keep = settled && !(policy_.drop_above && held > policy_.drop_above);
    if (keep) {
      std::lock_guard<std::mutex> lock(mu_);
      keep = free_.size() < policy_.max_kept;
      if (keep && policy_.one_big_above && held > policy_.one_big_above)
        for (const W* f : free_) keep = keep && !(f->device == w->device && f->held() > policy_.one_big_above);
      if (keep) free_.push_back(w);
    }
    if (!keep) destroy_(w);
  }

  const WsPolicy policy_;
  std::function<void(W*)> destroy_;
  mutable std::mutex mu_;
  std::vector<W*> free_;
};

}  // namespace ffp
