// tests/asan/asan_subopts.cpp — TEST ONLY: the subscription-option table
// compiler and the host walk (emqx_amd/csrc/gm_subopts.cpp) built as host C++
// with AddressSanitizer + UBSan.  It compiles random tables (filters given
// twice, empty lists, a long list, pairs with and without entries), walks
// random rows in FLAG and DROP mode and checks every array against a
// brute-force restatement (a std::map of options walked pair by pair); then
// empty tables and rows, the SKIP_UNKNOWN flag, malformed offsets, entries
// past the lists and refused calls.  Never touches a device.  Built by
// `make -C emqx_amd/csrc asan-subopts`, run by
// tests/test_subopts_cpu.py::test_compiler_and_host_walk_under_asan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_subopts.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
void so_free_device(emqx_gm_subopts*) {}  // gm_subopts.hip's: a host-only table never gets there
}  // namespace gm
extern "C" int emqx_gm_index_release(emqx_gm_index*) { return 0; }  // (a host-only table retains no snapshot)

namespace {

struct Packed {
  std::vector<uint8_t> b;
  std::vector<uint64_t> o{0};
  explicit Packed(const std::vector<std::string>& v) {
    for (auto& s : v) {
      b.insert(b.end(), s.begin(), s.end());
      o.push_back(b.size());
    }
    if (b.empty()) b.push_back(0);
  }
};

struct Entry {
  std::string f;
  uint32_t sub;
  uint8_t opt;
};

struct World {
  std::vector<std::string> filters;          // input order, duplicates allowed
  std::vector<std::vector<uint32_t>> lists;  // per input filter
  std::vector<std::string> names;            // distinct, sorted: id = position
  std::vector<std::vector<uint32_t>> by_id;  // per id: the lists concatenated in input order
  void finish() {
    names = filters;
    std::sort(names.begin(), names.end());
    names.erase(std::unique(names.begin(), names.end()), names.end());
    by_id.assign(names.size(), {});
    for (size_t i = 0; i < filters.size(); ++i) {
      auto& l = by_id[std::lower_bound(names.begin(), names.end(), filters[i]) - names.begin()];
      l.insert(l.end(), lists[i].begin(), lists[i].end());
    }
  }
};

emqx_gm_subopts* compile(const World& w, const std::vector<Entry>& es, uint8_t def, uint32_t flags = 0,
                         int* rc_out = nullptr) {
  Packed pf(w.filters);
  std::vector<uint64_t> so{0};
  std::vector<uint32_t> si;
  for (auto& l : w.lists) {
    si.insert(si.end(), l.begin(), l.end());
    so.push_back(si.size());
  }
  if (si.empty()) si.push_back(0);
  std::vector<std::string> ef;
  std::vector<uint32_t> esub;
  std::vector<uint8_t> eopt;
  for (auto& e : es) {
    ef.push_back(e.f);
    esub.push_back(e.sub);
    eopt.push_back(e.opt);
  }
  Packed pe(ef);
  if (esub.empty()) esub.push_back(0), eopt.push_back(0);
  emqx_gm_subopts* t = nullptr;
  const int rc = emqx_gm_subopts_compile_host(pf.b.data(), pf.o.data(), w.filters.size(), so.data(), si.data(),
                                              pe.b.data(), pe.o.data(), esub.data(), eopt.data(), es.size(), def, flags,
                                              &t);
  if (rc_out) *rc_out = rc;
  return rc ? nullptr : t;
}

uint8_t ref_byte(uint8_t o, uint8_t m) {  // enrich_subopts/3, clause by clause
  unsigned q = o & 3, pq = m & 3;
  q = (o & 0x10) ? std::max(q, pq) : std::min(q, pq);
  bool retain = m & 4;
  if (!(o & 8) && !(m & 8)) retain = false;
  return uint8_t(q | (retain ? 4 : 0) | ((o & 4) ? 8 : 0));
}

// the option map walked pair by pair; 0 = the result equals it
int check(emqx_gm_subopts* t, const World& w, const std::vector<Entry>& es, uint8_t def,
          const std::vector<std::vector<uint32_t>>& rows, const std::vector<uint8_t>& mf,
          const std::vector<uint32_t>& from, uint32_t mode) {
  std::map<std::pair<uint32_t, uint32_t>, uint8_t> opts;
  for (auto& e : es) {
    const auto it = std::lower_bound(w.names.begin(), w.names.end(), e.f);
    if (it != w.names.end() && *it == e.f) opts[{uint32_t(it - w.names.begin()), e.sub}] = e.opt;
  }
  std::vector<uint64_t> want_ro{0};
  std::vector<uint32_t> want_ids, want_drop;
  std::vector<uint8_t> want_opt;
  for (size_t r = 0; r < rows.size(); ++r) {
    uint32_t nd = 0;
    for (uint32_t f : rows[r])
      for (uint32_t s : w.by_id[f]) {
        const auto it = opts.find({f, s});
        const uint8_t o = it == opts.end() ? def : it->second;
        const bool hit = (o & 4) && from[r] != EMQX_GM_SO_NO_PUBLISHER && s == from[r];
        if (hit && mode == EMQX_GM_SO_DROP) {
          ++nd;
          continue;
        }
        want_ids.push_back(s);
        want_opt.push_back(uint8_t(ref_byte(o, mf[r]) | (hit ? 16 : 0)));
      }
    want_ro.push_back(want_ids.size());
    want_drop.push_back(nd);
  }
  std::vector<uint64_t> ro{0};
  std::vector<uint32_t> ids;
  for (auto& r : rows) {
    ids.insert(ids.end(), r.begin(), r.end());
    ro.push_back(ids.size());
  }
  if (ids.empty()) ids.push_back(0);
  std::vector<uint8_t> mfv = mf;
  std::vector<uint32_t> frv = from;
  if (mfv.empty()) mfv.push_back(0), frv.push_back(0);
  emqx_gm_csr m{};
  m.n_rows = rows.size();
  m.nnz = ro.back();
  m.row_off = ro.data();
  m.ids = ids.data();
  emqx_gm_deliveries d;
  if (emqx_gm_deliver_host(t, &m, mfv.data(), frv.data(), mode, &d)) return 1;
  int bad = 0;
  if (d.deliveries.n_rows != rows.size() || d.deliveries.nnz != want_ids.size() || d.deliveries.on_device) bad = 2;
  for (size_t r = 0; r <= rows.size() && !bad; ++r)
    if (d.deliveries.row_off[r] != want_ro[r]) bad = 3;
  for (size_t k = 0; k < want_ids.size() && !bad; ++k)
    if (d.deliveries.ids[k] != want_ids[k] || d.dopt[k] != want_opt[k]) bad = 4;
  uint64_t sum = 0;
  if (mode == EMQX_GM_SO_DROP) {
    for (size_t r = 0; r < rows.size() && !bad; ++r) {
      if (d.row_dropped[r] != want_drop[r]) bad = 5;
      sum += want_drop[r];
    }
  } else if (d.row_dropped) {
    bad = 6;
  }
  if (!bad && d.n_dropped != sum) bad = 7;
  emqx_gm_deliveries_free_host(&d);
  if (bad) std::printf("deliver: %d (mode %u)\n", bad, mode);
  return bad;
}

}  // namespace

int main() {
  std::mt19937 rng(11);
  auto pick = [&](size_t n) { return uint32_t(rng() % n); };
  for (int round = 0; round < 6; ++round) {
    World w;
    for (int i = 0; i < 60; ++i) w.filters.push_back("f/" + std::to_string(1000 + i) + (i % 3 ? "/+" : "/#"));
    w.filters.push_back(std::string("nul\0in", 6));
    w.filters.push_back("\xff\xfe/+");
    w.filters.push_back("");
    w.filters.push_back(w.filters[3]);  // a filter given twice: its lists are concatenated
    for (size_t i = 0; i < w.filters.size(); ++i) {
      std::vector<uint32_t> l;
      const uint32_t c = std::vector<uint32_t>{0, 1, 1, 3, 4, 5, 17}[pick(7)];
      for (uint32_t k = 0; k < c; ++k) l.push_back(uint32_t(i) * 100 + k);  // distinct within and across the two lists
      w.lists.push_back(l);
    }
    w.lists[1].clear();
    for (uint32_t k = 0; k < 3000; ++k) w.lists[1].push_back(500000 + k * 7);  // a long list
    w.finish();
    std::vector<Entry> es;
    for (size_t i = 0; i < w.filters.size(); ++i)
      for (uint32_t s : w.lists[i])
        if (pick(3)) es.push_back({w.filters[i], s, uint8_t(pick(3) | (pick(2) << 2) | (pick(2) << 3) | (pick(2) << 4))});
    for (int i = 0; i < 30; ++i) es.push_back(es[pick(es.size())]);  // pairs given twice, the same byte
    const uint8_t def = round % 2 ? uint8_t(0x0D) : uint8_t(0);        // (a default with nl = 1 too)
    emqx_gm_subopts* t = compile(w, es, def);
    if (!t) return std::printf("compile %d\n", round), 1;
    emqx_gm_subopts_info_t info;
    if (emqx_gm_subopts_info(t, &info) || info.device_bytes || info.n_skipped_unknown || !info.n_entries) return 1;
    std::vector<std::vector<uint32_t>> rows;
    std::vector<uint8_t> mf;
    std::vector<uint32_t> from;
    for (int r = 0; r < 400; ++r) {
      std::vector<uint32_t> row;
      for (uint32_t k = 0, c = std::vector<uint32_t>{0, 1, 1, 2, 3, 6}[pick(6)]; k < c; ++k)
        row.push_back(pick(w.names.size()));
      uint32_t f = EMQX_GM_SO_NO_PUBLISHER;
      if (!row.empty() && pick(4)) {
        const auto& l = w.by_id[row[pick(row.size())]];
        f = l.empty() || !pick(5) ? pick(100000) : l[pick(l.size())];
      }
      rows.push_back(row);
      mf.push_back(uint8_t(pick(3) | (pick(2) << 2) | (pick(2) << 3)));
      from.push_back(f);
    }
    for (uint32_t mode : {EMQX_GM_SO_FLAG, EMQX_GM_SO_DROP})
      if (check(t, w, es, def, rows, mf, from, mode)) return 1;
    if (check(t, w, es, def, {}, {}, {}, EMQX_GM_SO_DROP)) return std::printf("empty rows\n"), 1;
    if (check(t, w, es, def, {{}, {}, {}}, {0, 1, 2}, {1, 2, 3}, EMQX_GM_SO_DROP)) return std::printf("all-empty rows\n"), 1;
    double ms[3];
    if (emqx_gm_subopts_last_times(t, ms) || ms[2] != 0) return 1;
    emqx_gm_subopts_release(t);
  }
  // the four-at-once byte rule against the scalar one: every (opt, msg), in every lane beside every neighbour
  for (uint32_t o = 0; o < 32; ++o)
    for (uint32_t m = 0; m < 16; ++m)
      for (uint32_t n = 0; n < 32; ++n)
        for (int lane = 0; lane < 4; ++lane) {
          uint32_t w = n * 0x01010101u;
          w = (w & ~(0xFFu << (8 * lane))) | (o << (8 * lane));
          const uint32_t got = gm::so_byte4(w, uint8_t(m));
          for (int k = 0; k < 4; ++k)
            if (((got >> (8 * k)) & 0xFF) != gm::so_byte(uint8_t(k == lane ? o : n), uint8_t(m)))
              return std::printf("so_byte4 %u %u %u %d\n", o, m, n, lane), 1;
        }
  // empty tables
  {
    World w0;
    w0.finish();
    emqx_gm_subopts* t0 = compile(w0, {}, 0);
    if (!t0 || check(t0, w0, {}, 0, {{}, {}}, {0, 0}, {1, 2}, EMQX_GM_SO_FLAG)) return std::printf("empty index\n"), 1;
    emqx_gm_subopts_release(t0);
    World w1;
    w1.filters = {"a", "b"};
    w1.lists = {{}, {}};
    w1.finish();
    emqx_gm_subopts* t1 = compile(w1, {}, 4);
    if (!t1 || check(t1, w1, {}, 4, {{0, 1}, {1}}, {1, 2}, {1, 2}, EMQX_GM_SO_DROP)) return std::printf("no subscribers\n"), 1;
    emqx_gm_subopts_release(t1);
  }
  // refused inputs
  {
    World w;
    w.filters = {"a/#", "b/+", "a/#"};
    w.lists = {{1, 2}, {3}, {2, 4}};
    w.finish();
    int rc = 0;
    if (compile(w, {{"not/in/the/snapshot", 1, 0}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {{"b/+", 1, 0}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;  // an entry past the list
    if (compile(w, {{"b/+", 0xFFFFFFFFu, 0}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {{"a/#", 1, 3}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {{"a/#", 1, 0x20}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {}, 3, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {}, 0, 0x8, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {{"a/#", 1, 1}, {"a/#", 1, 2}}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(w, {{"a/#", 2, 4}}, 0, 0, &rc) || rc != EMQX_GM_EUNSUPPORTED) return 1;  // listed twice, nl = 1
    if (compile(w, {}, 4, 0, &rc) || rc != EMQX_GM_EUNSUPPORTED) return 1;
    const std::vector<Entry> some{{"nope", 1, 1}, {"a/#", 1, 5}, {"b/+", 9, 1}, {"a/#", 2, 1}};
    emqx_gm_subopts* sk = compile(w, some, 0, EMQX_GM_SO_SKIP_UNKNOWN, &rc);
    emqx_gm_subopts_info_t info;
    if (!sk || emqx_gm_subopts_info(sk, &info) || info.n_entries != 2 || info.n_skipped_unknown != 2 ||
        info.n_nl != 1 || info.n_defaulted != 2)
      return std::printf("skip_unknown\n"), 1;
    if (check(sk, w, {{"a/#", 1, 5}, {"a/#", 2, 1}}, 0, {{0, 1}, {1}, {0}}, {6, 1, 2}, {1, 3, 4}, EMQX_GM_SO_DROP))
      return 1;
    // malformed offsets through the C entry point
    Packed pf(w.filters);
    const uint64_t so[4] = {0, 2, 3, 5}, so_down[4] = {0, 2, 1, 5}, so_off[4] = {1, 2, 3, 5};
    const uint32_t si[5] = {1, 2, 3, 2, 4};
    const uint8_t b[8] = {'a', '/', '#', 'b', '/', '+', 0, 0};
    const uint64_t down[3] = {0, 6, 3}, far[2] = {0, uint64_t(1) << 40}, fine[3] = {0, 3, 6};
    const uint32_t es2[2] = {1, 3};
    const uint8_t eo2[2] = {0, 0};
    emqx_gm_subopts* t = nullptr;
    auto call = [&](const uint64_t* sub_off, const uint64_t* fo, uint64_t n, const uint32_t* es, const uint8_t* eo) {
      return emqx_gm_subopts_compile_host(pf.b.data(), pf.o.data(), 3, sub_off, si, b, fo, es, eo, n, 0, 0, &t);
    };
    if (call(so, fine, 2, es2, eo2) != EMQX_GM_OK || !t) return 1;
    emqx_gm_subopts_release(t);
    if (call(so, down, 2, es2, eo2) != EMQX_GM_EINVAL || t) return 1;
    if (call(so, far, 1, es2, eo2) != EMQX_GM_EINVAL || t) return 1;
    if (call(so_down, fine, 2, es2, eo2) != EMQX_GM_EINVAL || t) return 1;
    if (call(so_off, fine, 2, es2, eo2) != EMQX_GM_EINVAL || t) return 1;
    if (call(nullptr, fine, 2, es2, eo2) != EMQX_GM_EUNSUPPORTED || t) return 1;
    if (call(so, fine, 2, nullptr, eo2) != EMQX_GM_EINVAL || t) return 1;
    if (call(so, fine, 2, es2, nullptr) != EMQX_GM_EINVAL || t) return 1;
    // rows: an id past the snapshot, descending offsets, offsets that do not span the ids, bad bytes, device rows
    uint64_t ro[3] = {0, 1, 2};
    uint32_t ids[2] = {0, 2};
    uint8_t mf[2] = {0, 0};
    uint32_t from[2] = {1, EMQX_GM_SO_NO_PUBLISHER};
    emqx_gm_csr m{};
    m.n_rows = 2, m.nnz = 2, m.row_off = ro, m.ids = ids;
    emqx_gm_deliveries d;
    std::memset(&d, 0x5A, sizeof(d));
    const emqx_gm_deliveries before = d;
    auto refused = [&](uint32_t mode = 0) {
      return emqx_gm_deliver_host(sk, &m, mf, from, mode, &d) == EMQX_GM_EINVAL && !std::memcmp(&d, &before, sizeof(d));
    };
    if (!refused()) return 1;  // id 2 of 2 filters
    ids[1] = 0;
    ro[1] = 2, ro[2] = 1;
    if (!refused()) return 1;
    ro[1] = 1, ro[2] = 1;
    if (!refused()) return 1;
    ro[2] = 2;
    mf[1] = 3;
    if (!refused()) return 1;
    mf[1] = 0x10;
    if (!refused()) return 1;
    mf[1] = 0;
    if (!refused(2)) return 1;
    m.on_device = 1;
    if (!refused()) return 1;
    m.on_device = 0;
    if (emqx_gm_deliver_host(sk, &m, nullptr, from, 0, &d) != EMQX_GM_EINVAL) return 1;
    if (emqx_gm_deliver_host(sk, &m, mf, nullptr, 0, &d) != EMQX_GM_EINVAL) return 1;
    if (emqx_gm_deliver_host(sk, &m, mf, from, 0, &d) != EMQX_GM_OK || emqx_gm_deliveries_free_host(&d)) return 1;
    if (emqx_gm_deliveries_free_host(nullptr) != EMQX_GM_EINVAL) return 1;
    emqx_gm_subopts_release(sk);
  }
  std::printf("asan_subopts ok\n");
  return 0;
}
