// plan_cache.hpp — the engines' cache of laid-out plans: least recently used plans go first, beyond a count or beyond a byte budget,
// and the owner's `quiesce` (set the device, wait for the stream) runs before any plan is destroyed. No HIP in here, so the same code
// runs under the host sanitizers (plan_cache_host_check.cpp).
//
// A pointer or reference handed out stays valid until the next get() that misses, or clear().
#pragma once
#include <cstddef>
#include <functional>
#include <map>
#include <memory>
#include <utility>

namespace ffp {

template <class Key, class P>      // P needs: size_t bytes
class PlanCache {
 public:
  // max_plans >= 1; max_bytes 0: no byte budget
  PlanCache(size_t max_plans, size_t max_bytes, std::function<void()> quiesce)
      : max_plans_(max_plans), max_bytes_(max_bytes), quiesce_(std::move(quiesce)) {}
  PlanCache(const PlanCache&) = delete;
  PlanCache& operator=(const PlanCache&) = delete;
  ~PlanCache() { clear_nothrow(); }

  // nullptr, or the plan, marked most recently used
  P* find(const Key& k) {
    auto it = plans_.find(k);
    if (it == plans_.end()) return nullptr;
    it->second.last_use = ++use_clock_;
    return it->second.plan.get();
  }

  // find(k), or: evict down to max_plans - 1, build() -> std::unique_ptr<P>, insert, then evict plans other than the fresh one while the
  // budget is exceeded. A build() that throws inserts nothing; the evictions before it stand.
  template <class Build>
  P& get(const Key& k, Build&& build) {
    if (P* hit = find(k)) return *hit;
    while (plans_.size() >= max_plans_ && evict_lru(nullptr)) {}
    std::unique_ptr<P> p = build();
    P* fresh = p.get();
    plans_[k] = Entry{std::move(p), ++use_clock_};
    while (max_bytes_ && bytes() > max_bytes_ && evict_lru(fresh)) {}
    return *fresh;
  }

  // marks a resident plan most recently used, for an owner that looks plans up by something other than the key (for_each)
  void touch(P& p) {
    for (auto& kv : plans_)
      if (kv.second.plan.get() == &p) kv.second.last_use = ++use_clock_;
  }

  template <class F>
  void for_each(F&& f) const {       // f(P&) over the resident plans, in no particular order
    for (const auto& kv : plans_) f(*kv.second.plan);
  }

  void clear() {                     // a quiesce that throws leaves every plan resident
    if (!plans_.empty()) quiesce_();
    plans_.clear();
  }
  // for destructors, which cannot report a failed wait: the plans go regardless
  void clear_nothrow() noexcept {
    try { clear(); } catch (...) { plans_.clear(); }
  }

  size_t size() const { return plans_.size(); }
  size_t bytes() const {
    size_t b = 0;
    for (const auto& kv : plans_) b += kv.second.plan->bytes;
    return b;
  }

 private:
  struct Entry {
    std::unique_ptr<P> plan;
    unsigned long long last_use = 0;
  };

  bool evict_lru(const P* keep) {
    auto victim = plans_.end();
    for (auto it = plans_.begin(); it != plans_.end(); ++it)
      if (it->second.plan.get() != keep && (victim == plans_.end() || it->second.last_use < victim->second.last_use)) victim = it;
    if (victim == plans_.end()) return false;
    quiesce_();
    plans_.erase(victim);
    return true;
  }

  size_t max_plans_, max_bytes_;
  std::function<void()> quiesce_;
  std::map<Key, Entry> plans_;
  unsigned long long use_clock_ = 0;
};

}  // namespace ffp
