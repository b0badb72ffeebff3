// The combining queue of emqx_gm_combiner (include/emqx_gpu_match.h): callers
// that arrive while earlier groups are on the device are coalesced into one
// group, run by one of them (the leader) through an executor callback.  No HIP
// here: the queue compiles and runs without a device (tests/asan/tsan_combiner.cpp
// drives it with a stub executor under ThreadSanitizer).
//
// Policy: a caller enqueues its window; while fewer than max_in_flight groups
// are out, a queued caller becomes a leader: it takes its own window and, in
// arrival order, every queued window compatible with it (same key: index,
// flags, deliveries or not, call kind and a publish window's opts) up to max_windows windows, max_topics topics and
// max_bytes of text, runs them, and hands every member its return code.
// Incompatible or surplus windows stay queued; when a group comes back, the
// waiters are woken and the first still-queued one leads the next group.  With
// min_windows > 1 a leader first waits (at most linger_us) until that many
// compatible windows have arrived -- for tests and tuning; the defaults
// (1, 0) never wait, so coalescing comes only from what queued meanwhile.
//
// One mutex and one condition variable, woken with notify_all: the waiters
// are a NIF's dirty schedulers (tens of threads), each wake-up re-checks its
// own predicate under the mutex.
#ifndef GM_COMBINE_H
#define GM_COMBINE_H

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <vector>

namespace gm {

// one caller's window in the queue (on the caller's stack for the length of its call)
struct CombWindow {
  // compatibility key
  const void* index = nullptr;
  uint32_t flags = 0;
  bool want_deliveries = false;
  // ... of a whole publish window (emqx_gm_combiner_publish): the call kind and the opts every
  // window of a group shares (defaulted: a match window's key is what it was)
  uint32_t kind = 0;  // 0: match / match + fan-out, 1: publish window
  const void* shared = nullptr;
  const void* dests = nullptr;
  uint32_t strategy = 0, seed = 0, skip_node = 0;
  // size, for the group limits
  uint64_t n_topics = 0;
  uint64_t n_bytes = 0;
  // the caller's own arguments and outputs (the executor's business)
  void* user = nullptr;
  // set by the executor (or, when it fails as a whole, by the queue)
  int rc = 0;
  // queue state (under the queue's mutex)
  bool leading = false;
  bool done = false;
};

struct CombinerLimits {
  uint32_t max_windows = 64;
  uint64_t max_topics = uint64_t(256) << 10;
  uint64_t max_bytes = uint64_t(1) << 20;
  uint32_t max_in_flight = 2;
  uint32_t min_windows = 1;
  uint32_t linger_us = 0;
};

struct CombinerCounts {
  uint64_t windows = 0;    // calls enqueued
  uint64_t groups = 0;     // executor runs
  uint64_t max_group = 0;  // windows of the largest group
  uint64_t solo = 0;       // groups of one window
};

class Combiner {
 public:
  // Runs one group: w[0] is the leader's window.  It sets each w[k]->rc and
  // the members' outputs and returns 0, or returns a non-zero code that the
  // queue hands to every member of the group.  Called without the queue's mutex.
  using Executor = std::function<int(CombWindow* const* w, uint32_t n)>;
  static constexpr int kClosed = -1;  // submit after close (EMQX_GM_EINVAL)

  Combiner(const CombinerLimits& lim, Executor ex) : lim_(lim), exec_(std::move(ex)) {
    lim_.max_windows = std::max<uint32_t>(1, lim_.max_windows);
    lim_.max_in_flight = std::max<uint32_t>(1, lim_.max_in_flight);
    lim_.min_windows = std::min(std::max<uint32_t>(1, lim_.min_windows), lim_.max_windows);
  }

  // Blocking: returns the window's own return code once its group has run.
  int submit(CombWindow* w) {
    std::unique_lock<std::mutex> lk(mu_);
    if (closed_) return kClosed;
    w->leading = w->done = false;
    q_.push_back(w);
    ++counts_.windows;
    cv_.notify_all();  // (a lingering leader counts the arrivals)
    for (;;) {
      if (w->done) return w->rc;
      // (a compatible leader still gathering will take this window: it does not lead a group of its own)
      if (!w->leading && in_flight_ < lim_.max_in_flight && !gathering_for(w)) {
        lead(w, lk);
        continue;
      }
      cv_.wait(lk);
    }
  }

  CombinerCounts counts() const {
    std::lock_guard<std::mutex> lk(mu_);
    return counts_;
  }

  // No new calls from here on; returns once every queued window has run.
  void close() {
    std::unique_lock<std::mutex> lk(mu_);
    closed_ = true;
    cv_.notify_all();  // (a lingering leader stops waiting for more)
    cv_.wait(lk, [&] { return q_.empty() && in_flight_ == 0; });
  }

 private:
  static bool compatible(const CombWindow* a, const CombWindow* b) {
    return a->index == b->index && a->flags == b->flags && a->want_deliveries == b->want_deliveries &&
           a->kind == b->kind && a->shared == b->shared && a->dests == b->dests && a->strategy == b->strategy &&
           a->seed == b->seed && a->skip_node == b->skip_node;
  }

  bool gathering_for(const CombWindow* w) const {
    for (const CombWindow* l : gathering_)
      if (compatible(l, w)) return true;
    return false;
  }

  // (entered and left with lk held; w is queued and not yet leading)
  void lead(CombWindow* w, std::unique_lock<std::mutex>& lk) {
    ++in_flight_;
    w->leading = true;
    if (lim_.min_windows > 1 && lim_.linger_us) {
      // (system_clock: the wait is pthread_cond_timedwait, which gcc 11's ThreadSanitizer runtime follows;
      // steady_clock's pthread_cond_clockwait it does not, and it then takes the mutex as held across the wait)
      const auto deadline = std::chrono::system_clock::now() + std::chrono::microseconds(lim_.linger_us);
      auto enough = [&] {
        uint32_t c = 0;
        for (const CombWindow* x : q_) c += (x == w || (!x->leading && compatible(w, x))) ? 1 : 0;
        return closed_ || c >= lim_.min_windows;
      };
      gathering_.push_back(w);
      while (!enough())
        if (cv_.wait_until(lk, deadline) == std::cv_status::timeout) break;
      gathering_.erase(std::find(gathering_.begin(), gathering_.end(), w));
    }
    // the group: the leader, then the compatible windows in arrival order, within the limits
    std::vector<CombWindow*> g{w};
    uint64_t topics = w->n_topics, bytes = w->n_bytes;
    for (CombWindow* x : q_) {
      if (g.size() >= lim_.max_windows) break;
      if (x == w || x->leading || !compatible(w, x)) continue;
      if (topics + x->n_topics > lim_.max_topics || bytes + x->n_bytes > lim_.max_bytes) continue;
      x->leading = true;  // (taken: no other leader picks it, and it does not lead itself)
      topics += x->n_topics;
      bytes += x->n_bytes;
      g.push_back(x);
    }
    q_.erase(std::remove_if(q_.begin(), q_.end(),
                            [&](CombWindow* x) { return std::find(g.begin(), g.end(), x) != g.end(); }),
             q_.end());
    ++counts_.groups;
    counts_.max_group = std::max<uint64_t>(counts_.max_group, g.size());
    if (g.size() == 1) ++counts_.solo;
    if (!q_.empty()) cv_.notify_all();  // (what stays queued: one of its owners leads the next group)
    lk.unlock();
    int rc = 0;
    try {
      rc = exec_(g.data(), uint32_t(g.size()));
    } catch (...) {
      rc = kClosed;  // (an executor must not throw; every member still gets an answer)
    }
    lk.lock();
    for (CombWindow* x : g) {  // (a follower's window is its own again once done is set)
      if (rc) x->rc = rc;
      x->done = true;
    }
    --in_flight_;
    cv_.notify_all();  // the members; and a queued window's owner, to lead the next group
  }

  CombinerLimits lim_;
  Executor exec_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::vector<CombWindow*> q_;
  std::vector<CombWindow*> gathering_;  // leaders waiting for min_windows (linger)
  uint32_t in_flight_ = 0;
  bool closed_ = false;
  CombinerCounts counts_;
};

}  // namespace gm

#endif
