// arena.hpp — byte ranges of a plan's activation tensors, reused by tensor lifetime. No HIP in here: blocks come from a callback
// (the plan backs them with DevBuf), so the same code runs under the host sanitizers (arena_host_check.cpp).
//
// Addresses are final when alloc() returns (closures and ConvOps capture them by value), so placement is online: best fit over the
// free ranges in build order, a new block of exactly the tensor's size when nothing fits. Free ranges split at 256-byte multiples and
// coalesce with free neighbours of the same block. Build order equals issue order, so "released" means "free for every step added
// later" — on lane 0. Between a fork and its join other lanes may still be running earlier steps: a range released while any fork is
// open is held back and reaches the free list when the last open fork has been joined.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace ffp {

class Arena {
 public:
  static constexpr size_t ALIGN = 256;
  using BlockFn = std::function<uintptr_t(size_t bytes)>;     // -> base address of a new block of `bytes` bytes, ALIGN-aligned
  enum Release { FREED = 0, HELD = 1, REJECTED = 2 };         // REJECTED: unknown id or second release
  struct Tensor { int block; size_t off, span, nb; int state; };     // span: bytes of the block the tensor owns (>= nb); state: 0 live, 1 held, 2 free

  // reuse = false: every tensor gets a block of its own and release() only closes the lifetime (the layout without this class)
  Arena(BlockFn get_block, bool reuse) : get_block_(std::move(get_block)), reuse_(reuse) {}

  int alloc(size_t nb) {
    if (nb == 0) nb = 1;
    const size_t need = (nb + ALIGN - 1) / ALIGN * ALIGN;
    int best = -1;
    for (int i = 0; i < (int)free_.size(); ++i)
      if (free_[i].size >= nb && (best < 0 || free_[i].size < free_[best].size)) best = i;      // ties: lowest (block, offset), free_ is sorted
    Tensor t{};
    t.nb = nb;
    if (best >= 0) {
      Range& r = free_[best];
      t.block = r.block; t.off = r.off;
      if (r.size > need) { t.span = need; r.off += need; r.size -= need; }
      else { t.span = r.size; free_.erase(free_.begin() + best); }
    } else {
      const uintptr_t base = get_block_(nb);
      if (base == 0 || base % ALIGN != 0) return -1;
      blocks_.push_back(Block{base, nb});
      held_bytes_ += nb;
      t.block = (int)blocks_.size() - 1; t.off = 0; t.span = nb;
    }
    sum_sizes_ += nb;
    live_bytes_ += nb;
    if (live_bytes_ > peak_live_) peak_live_ = live_bytes_;
    tensors_.push_back(t);
    return (int)tensors_.size() - 1;
  }

  Release release(int id) {
    if (id < 0 || id >= (int)tensors_.size() || tensors_[id].state != 0) return REJECTED;
    if (forks_open_ > 0) { tensors_[id].state = 1; held_.push_back(id); return HELD; }
    to_free(id);
    return FREED;
  }

  void fork() { ++forks_open_; }
  // -> false without an open fork. The ids whose ranges this join let go (in release order) are appended to `flushed`.
  bool join(std::vector<int>* flushed = nullptr) {
    if (forks_open_ <= 0) return false;
    if (--forks_open_ > 0) return true;
    for (int id : held_) { to_free(id); if (flushed) flushed->push_back(id); }
    held_.clear();
    return true;
  }

  uintptr_t addr(int id) const { return blocks_[tensors_[id].block].base + tensors_[id].off; }
  const Tensor& tensor(int id) const { return tensors_[id]; }
  int tensors() const { return (int)tensors_.size(); }
  int blocks() const { return (int)blocks_.size(); }
  uintptr_t block_base(int b) const { return blocks_[b].base; }
  size_t block_size(int b) const { return blocks_[b].size; }
  int forks_open() const { return forks_open_; }
  size_t held_bytes() const { return held_bytes_; }       // bytes of every block obtained
  size_t sum_sizes() const { return sum_sizes_; }         // what one block per tensor would hold
  size_t live_bytes() const { return live_bytes_; }       // tensors not yet back on the free list (held-back ones included)
  size_t peak_live_bytes() const { return peak_live_; }   // maximum of live_bytes() over build order: the floor of any placement

 private:
  struct Block { uintptr_t base; size_t size; };
  struct Range { int block; size_t off, size; };

  void to_free(int id) {
    Tensor& t = tensors_[id];
    t.state = 2;
    live_bytes_ -= t.nb;
    if (!reuse_) return;
    Range r{t.block, t.off, t.span};
    size_t i = 0;
    while (i < free_.size() && (free_[i].block < r.block || (free_[i].block == r.block && free_[i].off < r.off))) ++i;
    if (i < free_.size() && free_[i].block == r.block && r.off + r.size == free_[i].off) { r.size += free_[i].size; free_.erase(free_.begin() + i); }
    if (i > 0 && free_[i - 1].block == r.block && free_[i - 1].off + free_[i - 1].size == r.off) { free_[i - 1].size += r.size; return; }
    free_.insert(free_.begin() + i, r);
  }

  BlockFn get_block_;
  bool reuse_;
  std::vector<Block> blocks_;
  std::vector<Range> free_;            // sorted by (block, offset), no two adjacent
  std::vector<Tensor> tensors_;
  std::vector<int> held_;
  int forks_open_ = 0;
  size_t held_bytes_ = 0, sum_sizes_ = 0, live_bytes_ = 0, peak_live_ = 0;
};

}  // namespace ffp
