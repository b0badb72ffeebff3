// tests/asan/asan_batches.cpp — TEST ONLY: the host walk of the session
// batches (emqx_amd/csrc/gm_batches.cpp) and the call checks it shares with the
// option table (gm_subopts.cpp) built as host C++ with AddressSanitizer + UBSan.
// It compiles random tables, walks random windows in FLAG, DROP and LEAD mode and
// checks every array against a brute-force restatement (per-subscriber lists
// filled in window order, then dropwhile); then empty windows and tables, a
// filter listed twice in a row, and refused calls.  Never touches a device.
// Built by `make -C emqx_amd/csrc asan-batches`, run by
// tests/test_batches_cpu.py::test_host_walk_under_asan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_batches.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
void so_free_device(emqx_gm_subopts*) {}  // gm_subopts.hip's: a host-only table never gets there
}  // namespace gm
extern "C" int emqx_gm_index_release(emqx_gm_index*) { return 0; }  // (a host-only table retains no snapshot)

namespace {

int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++fails;                                                    \
    }                                                             \
  } while (0)

struct World {
  std::vector<std::string> filters;          // distinct, sorted: id = position
  std::vector<std::vector<uint32_t>> lists;  // per filter, each subscriber once
  std::map<std::pair<uint32_t, uint32_t>, uint8_t> opt;  // (filter id, subscriber) -> byte
};

emqx_gm_subopts* compile(const World& w) {
  std::vector<uint8_t> fb, eb;
  std::vector<uint64_t> fo{0}, eo{0}, so{0};
  std::vector<uint32_t> si, esub;
  std::vector<uint8_t> eopt;
  for (size_t f = 0; f < w.filters.size(); ++f) {
    fb.insert(fb.end(), w.filters[f].begin(), w.filters[f].end());
    fo.push_back(fb.size());
    si.insert(si.end(), w.lists[f].begin(), w.lists[f].end());
    so.push_back(si.size());
  }
  for (auto& e : w.opt) {
    const std::string& s = w.filters[e.first.first];
    eb.insert(eb.end(), s.begin(), s.end());
    eo.push_back(eb.size());
    esub.push_back(e.first.second);
    eopt.push_back(e.second);
  }
  if (fb.empty()) fb.push_back(0);
  if (eb.empty()) eb.push_back(0);
  if (si.empty()) si.push_back(0);
  if (esub.empty()) esub.push_back(0), eopt.push_back(0);
  emqx_gm_subopts* t = nullptr;
  const int rc = emqx_gm_subopts_compile_host(fb.data(), fo.data(), w.filters.size(), so.data(), si.data(), eb.data(),
                                              eo.data(), esub.data(), eopt.data(), w.opt.size(), 0, 0, &t);
  CHECK(rc == EMQX_GM_OK && t);
  return t;
}

struct Window {
  std::vector<uint64_t> ro{0};
  std::vector<uint32_t> ids, from;
  std::vector<uint8_t> flags;
  emqx_gm_csr csr() {
    emqx_gm_csr m{};
    m.n_rows = ro.size() - 1;
    m.nnz = ids.size();
    m.row_off = ro.data();
    m.ids = ids.empty() ? nullptr : ids.data();
    return m;
  }
};

struct Entry {
  uint32_t row, fil;
  uint8_t byte;
  bool operator==(const Entry& o) const { return row == o.row && fil == o.fil && byte == o.byte; }
};

// the restatement: mailboxes filled in window order, then the mode's removal
void expect(const World& w, Window& win, uint32_t mode, const emqx_gm_batches& got) {
  std::map<uint32_t, std::vector<Entry>> box;
  for (size_t r = 0; r + 1 < win.ro.size(); ++r)
    for (uint64_t j = win.ro[r]; j < win.ro[r + 1]; ++j) {
      const uint32_t f = win.ids[j];
      for (uint32_t s : w.lists[f]) {
        const auto it = w.opt.find({f, s});
        const uint8_t o = it == w.opt.end() ? 0 : it->second;
        const bool hit = (o & 4) && win.from[r] != EMQX_GM_SO_NO_PUBLISHER && win.from[r] == s;
        box[s].push_back(Entry{uint32_t(r), f, uint8_t(gm::so_byte(o, win.flags[r]) | (hit ? 16 : 0))});
      }
    }
  CHECK(got.n_batches == box.size() && got.n_rows == win.ro.size() - 1);
  CHECK((got.batch_dropped == nullptr) == (mode == EMQX_GM_SO_FLAG));
  uint64_t j = 0, at = 0, gone_all = 0;
  for (auto& b : box) {
    std::vector<Entry> keep;
    uint32_t gone = 0;
    size_t i = 0;
    if (mode == EMQX_GM_SO_LEAD)
      while (i < b.second.size() && (b.second[i].byte & 16)) ++i, ++gone;
    for (; i < b.second.size(); ++i) {
      Entry e = b.second[i];
      if (mode == EMQX_GM_SO_DROP && (e.byte & 16)) {
        ++gone;
        continue;
      }
      if (mode == EMQX_GM_SO_LEAD) e.byte &= uint8_t(~16);
      keep.push_back(e);
    }
    if (j >= got.n_batches) break;
    CHECK(got.subs[j] == b.first && got.batch_off[j] == at && got.batch_off[j + 1] == at + keep.size());
    if (got.batch_dropped) CHECK(got.batch_dropped[j] == gone);
    if (got.batch_off[j + 1] == at + keep.size() && at + keep.size() <= got.n_deliveries)
      for (size_t k = 0; k < keep.size(); ++k)
        CHECK((keep[k] == Entry{got.rows[at + k], got.filters[at + k], got.dopt[at + k]}));
    at += keep.size();
    gone_all += gone;
    ++j;
  }
  CHECK(got.n_deliveries == at && got.n_dropped == gone_all && got.batch_off[got.n_batches] == at);
}

void run(const World& w, emqx_gm_subopts* t, Window& win) {
  for (uint32_t mode : {EMQX_GM_SO_FLAG, EMQX_GM_SO_DROP, EMQX_GM_SO_LEAD}) {
    emqx_gm_batches out{};
    emqx_gm_csr m = win.csr();
    const uint8_t zf = 0;
    const uint32_t zu = 0;
    const int rc = emqx_gm_deliver_batches_host(t, &m, win.flags.empty() ? &zf : win.flags.data(),
                                                win.from.empty() ? &zu : win.from.data(), mode, &out);
    CHECK(rc == EMQX_GM_OK);
    if (rc) continue;
    expect(w, win, mode, out);
    CHECK(emqx_gm_batches_free_host(&out) == EMQX_GM_OK && !out.subs && !out.batch_off);
  }
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  for (int round = 0; round < 30; ++round) {
    World w;
    const uint32_t nf = 1 + rng() % 12, ns = 1 + rng() % 20;
    for (uint32_t f = 0; f < nf; ++f) {
      char name[16];
      std::snprintf(name, sizeof name, "t/%03u/+", f);
      w.filters.push_back(name);
      std::vector<uint32_t> all(ns);
      for (uint32_t s = 0; s < ns; ++s) all[s] = s * 1000003u % 70000u;  // ids past one and two digits
      std::shuffle(all.begin(), all.end(), rng);
      all.resize(rng() % (ns + 1));
      w.lists.push_back(all);
      for (uint32_t s : all)
        if (rng() % 3) w.opt[{f, s}] = uint8_t((rng() % 3) | ((rng() & 1) << 2) | ((rng() & 1) << 3) | ((rng() & 1) << 4));
    }
    emqx_gm_subopts* t = compile(w);
    if (!t) continue;
    for (int k = 0; k < 6; ++k) {
      Window win;
      const uint32_t rows = rng() % 40;
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t c = rng() % 4;
        for (uint32_t i = 0; i < c; ++i) win.ids.push_back(rng() % nf);  // (a filter may be listed twice in a row)
        win.ro.push_back(win.ids.size());
        uint32_t from = EMQX_GM_SO_NO_PUBLISHER;
        if (c && rng() % 4) {
          auto& l = w.lists[win.ids.back()];
          from = l.empty() ? rng() % 70000u : l[rng() % l.size()];
        }
        win.from.push_back(from);
        win.flags.push_back(uint8_t((rng() % 3) | ((rng() & 1) << 2) | ((rng() & 1) << 3)));
      }
      run(w, t, win);
    }
    // refused calls leave the output untouched
    Window win;
    win.ids = {0, 0};
    win.ro = {0, 1, 2};
    win.from = {1, 2};
    win.flags = {0, 0};
    emqx_gm_csr m = win.csr();
    emqx_gm_batches out;
    std::memset(&out, 0xAB, sizeof out);
    emqx_gm_batches before = out;
    CHECK(emqx_gm_deliver_batches_host(t, &m, win.flags.data(), win.from.data(), 3, &out) == EMQX_GM_EINVAL);
    win.flags[1] = 0x13;
    CHECK(emqx_gm_deliver_batches_host(t, &m, win.flags.data(), win.from.data(), 2, &out) == EMQX_GM_EINVAL);
    win.flags[1] = 0;
    win.ids[1] = nf;
    CHECK(emqx_gm_deliver_batches_host(t, &m, win.flags.data(), win.from.data(), 2, &out) == EMQX_GM_EINVAL);
    win.ids[1] = 0;
    win.ro = {0, 2, 1};
    m = win.csr();
    CHECK(emqx_gm_deliver_batches_host(t, &m, win.flags.data(), win.from.data(), 0, &out) == EMQX_GM_EINVAL);
    CHECK(emqx_gm_deliver_batches_host(t, &m, nullptr, win.from.data(), 0, &out) == EMQX_GM_EINVAL);
    CHECK(emqx_gm_deliver_batches_host(nullptr, &m, win.flags.data(), win.from.data(), 0, &out) == EMQX_GM_EINVAL);
    CHECK(std::memcmp(&out, &before, sizeof out) == 0);
    emqx_gm_deliveries d{};
    win.ro = {0, 1, 2};
    m = win.csr();
    CHECK(emqx_gm_deliver_host(t, &m, win.flags.data(), win.from.data(), EMQX_GM_SO_LEAD, &d) == EMQX_GM_EINVAL);
    emqx_gm_subopts_release(t);
  }
  // a table without subscribers, an empty window
  {
    World w;
    w.filters = {"a", "b"};
    w.lists = {{}, {}};
    emqx_gm_subopts* t = compile(w);
    Window win;
    win.ids = {0, 1};
    win.ro = {0, 2};
    win.from = {5};
    win.flags = {1};
    run(w, t, win);
    Window none;
    run(w, t, none);
    emqx_gm_subopts_release(t);
  }
  if (fails) {
    std::printf("asan_batches: %d failures\n", fails);
    return 1;
  }
  std::printf("asan_batches ok\n");
  return 0;
}
