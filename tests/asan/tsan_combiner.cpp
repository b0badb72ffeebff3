// The combining queue (emqx_amd/csrc/gm_combine.h) alone, under ThreadSanitizer,
// with a stub executor: a window's "rows" are its own bytes, handed back after
// a short sleep (the device round trip).  Exits non-zero on the first failed
// check.  Built and run by tests/test_windows_cpu.py (make tsan-combiner).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "../../emqx_amd/csrc/gm_combine.h"

namespace {

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

constexpr int kFail = -3;

struct Call {  // a caller's window: its bytes in, its "rows" out
  uint64_t id = 0;
  std::vector<uint8_t> in, out;
  bool poison = false;
};

struct Stub {  // what the executor saw (under mu)
  std::mutex mu;
  std::vector<uint32_t> group_sizes;
  std::set<uint64_t> failed;
  uint64_t executed = 0;
  bool mixed = false, over = false;
  std::atomic<int> running{0};
  std::atomic<bool> started{false};
  gm::CombinerLimits lim;
  int sleep_us = 200;

  int run(gm::CombWindow* const* w, uint32_t n) {
    ++running;
    started = true;
    std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
    bool bad = false;
    uint64_t topics = 0, bytes = 0;
    for (uint32_t k = 0; k < n; ++k) {
      Call* c = static_cast<Call*>(w[k]->user);
      bad = bad || c->poison;
      topics += w[k]->n_topics;
      bytes += w[k]->n_bytes;
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      group_sizes.push_back(n);
      executed += n;
      for (uint32_t k = 1; k < n; ++k)
        if (w[k]->index != w[0]->index || w[k]->flags != w[0]->flags ||
            w[k]->want_deliveries != w[0]->want_deliveries)
          mixed = true;
      if (n > lim.max_windows || (n > 1 && (topics > lim.max_topics || bytes > lim.max_bytes))) over = true;
      if (bad)
        for (uint32_t k = 0; k < n; ++k) failed.insert(static_cast<Call*>(w[k]->user)->id);
    }
    if (!bad)
      for (uint32_t k = 0; k < n; ++k) {
        Call* c = static_cast<Call*>(w[k]->user);
        c->out = c->in;
        w[k]->rc = 0;
      }
    --running;
    return bad ? kFail : 0;
  }
};

int one_call(gm::Combiner& q, Call& c, const void* index, uint64_t n_topics = 1, uint32_t flags = 0,
             bool deliveries = true) {
  gm::CombWindow w;
  w.index = index;
  w.flags = flags;
  w.want_deliveries = deliveries;
  w.n_topics = n_topics;
  w.n_bytes = c.in.size();
  w.user = &c;
  return q.submit(&w);
}

Call make_call(uint64_t id) {
  Call c;
  c.id = id;
  c.in.resize(1 + id % 37);
  for (size_t i = 0; i < c.in.size(); ++i) c.in[i] = uint8_t(id * 131 + i);
  return c;
}

// 8 threads x 200 calls, two "indexes": every caller gets its own bytes back, no group is mixed
void test_own_results() {
  Stub s;
  gm::Combiner q(s.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s.run(w, n); });
  static const int idx_a = 0, idx_b = 0;
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (int i = 0; i < 200; ++i) {
        Call c = make_call(uint64_t(t) * 1000 + i);
        CHECK(one_call(q, c, (t + i) & 1 ? &idx_a : &idx_b, 1, (i >> 3) & 1, (i >> 4) & 1) == 0);
        CHECK(c.out == c.in);
      }
    });
  for (auto& x : th) x.join();
  const gm::CombinerCounts c = q.counts();
  CHECK(c.windows == 1600 && s.executed == 1600);
  CHECK(!s.mixed && !s.over);
  uint64_t sum = 0, solo = 0, mx = 0;
  for (uint32_t g : s.group_sizes) sum += g, solo += g == 1, mx = std::max<uint64_t>(mx, g);
  CHECK(sum == 1600 && c.groups == s.group_sizes.size() && c.solo == solo && c.max_group == mx);
  q.close();
}

// min_windows = 4 and a long linger: four callers form one group of four (and none waits the linger out)
void test_group_of_four() {
  Stub s;
  s.lim.min_windows = 4;
  s.lim.linger_us = 20 * 1000 * 1000;
  gm::Combiner q(s.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s.run(w, n); });
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      Call c = make_call(t);
      CHECK(one_call(q, c, &s) == 0 && c.out == c.in);
    });
  for (auto& x : th) x.join();
  CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));
  const gm::CombinerCounts c = q.counts();
  CHECK(c.windows == 4 && c.groups == 1 && c.max_group == 4 && c.solo == 0);
  q.close();
}

// groups respect max_windows and max_topics: windows of 4 topics under a limit of 10 go two by two
void test_limits() {
  Stub s;
  s.lim.max_windows = 3;
  s.lim.max_topics = 10;
  s.lim.min_windows = 2;
  s.lim.linger_us = 200 * 1000;
  s.lim.max_in_flight = 1;
  gm::Combiner q(s.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s.run(w, n); });
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (int i = 0; i < 25; ++i) {
        Call c = make_call(uint64_t(t) * 100 + i);
        CHECK(one_call(q, c, &s, 4) == 0 && c.out == c.in);
      }
    });
  for (auto& x : th) x.join();
  CHECK(!s.over && !s.mixed);
  CHECK(q.counts().max_group == 2);
  // ... and max_windows, with windows of one topic
  Stub s2;
  s2.lim.max_windows = 3;
  s2.lim.min_windows = 3;
  s2.lim.linger_us = 200 * 1000;
  s2.lim.max_in_flight = 1;
  gm::Combiner q2(s2.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s2.run(w, n); });
  th.clear();
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (int i = 0; i < 25; ++i) {
        Call c = make_call(uint64_t(t) * 100 + i);
        CHECK(one_call(q2, c, &s2) == 0 && c.out == c.in);
      }
    });
  for (auto& x : th) x.join();
  CHECK(!s2.over && q2.counts().max_group == 3);
  q.close();
  q2.close();
}

// an executor error reaches exactly the members of its group
void test_error_reaches_its_group() {
  Stub s;
  gm::Combiner q(s.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s.run(w, n); });
  std::atomic<int> n_fail{0}, n_ok{0};
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (int i = 0; i < 100; ++i) {
        Call c = make_call(uint64_t(t) * 1000 + i);
        c.poison = (t * 7 + i) % 23 == 0;
        const int rc = one_call(q, c, &s);
        bool in_failed;
        {
          std::lock_guard<std::mutex> lk(s.mu);
          in_failed = s.failed.count(c.id) != 0;
        }
        CHECK(rc == (in_failed ? kFail : 0));
        CHECK(!c.poison || in_failed);
        if (rc == 0) CHECK(c.out == c.in);
        else CHECK(c.out.empty());
        ++(rc ? n_fail : n_ok);
      }
    });
  for (auto& x : th) x.join();
  CHECK(n_fail > 0 && n_ok > 0 && n_fail + n_ok == 800);
  q.close();
}

// close with calls in flight returns after them; calls after it are refused
void test_close() {
  Stub s;
  s.sleep_us = 50 * 1000;
  gm::Combiner q(s.lim, [&](gm::CombWindow* const* w, uint32_t n) { return s.run(w, n); });
  std::vector<std::thread> th;
  for (int t = 0; t < 6; ++t)
    th.emplace_back([&, t] {
      Call c = make_call(t);
      const int rc = one_call(q, c, &s);
      CHECK(rc == 0 || rc == gm::Combiner::kClosed);
      if (rc == 0) CHECK(c.out == c.in);
    });
  while (!s.started) std::this_thread::yield();
  q.close();
  CHECK(s.running == 0);
  {
    std::lock_guard<std::mutex> lk(s.mu);
    CHECK(s.executed == q.counts().windows);  // every window queued before the close has run
  }
  Call late = make_call(99);
  CHECK(one_call(q, late, &s) == gm::Combiner::kClosed && late.out.empty());
  for (auto& x : th) x.join();
}

}  // namespace

int main() {
  test_own_results();
  test_group_of_four();
  test_limits();
  test_error_reaches_its_group();
  test_close();
  std::puts("tsan_combiner ok");
  return 0;
}
