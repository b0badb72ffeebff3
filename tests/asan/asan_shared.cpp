// tests/asan/asan_shared.cpp — TEST ONLY: the shared-subscription table compiler
// and the host walk (emqx_amd/csrc/gm_shared.cpp) built as host C++ with
// AddressSanitizer + UBSan.  It compiles a random slot set (duplicate pairs,
// duplicate members, empty slots), walks random rows with every strategy over
// three calls and checks every pick against a brute-force restatement of
// emqx_shared_sub:pick/6 (apps/emqx/src/emqx_shared_sub.erl:234-288) kept in
// std::map state; then a rebuild with prev under shifted filter ids, empty
// tables and rows, and refused inputs.  Never touches a device.  Built by
// `make -C emqx_amd/csrc asan-shared`, run by
// tests/test_shared_cpu.py::test_compiler_and_host_walk_under_asan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_shared.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
void sh_free_device(emqx_gm_shared*) {}  // gm_shared.hip's: a host-only table never gets there
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

struct Slot {
  std::string f;
  uint32_t g;
  std::vector<uint32_t> mem;
};

using Key = std::pair<std::string, uint32_t>;  // {Topic, Group}
struct Ref {
  std::vector<std::string> names;                 // filter id -> bytes
  std::vector<std::pair<Key, std::vector<uint32_t>>> slots;  // sorted by (filter id, group)
  std::map<Key, uint32_t> rr, st;                 // the process dictionary

  Ref(std::vector<std::string> filters, const std::vector<Slot>& in, const Ref* prev) {
    std::sort(filters.begin(), filters.end());
    filters.erase(std::unique(filters.begin(), filters.end()), filters.end());
    names = filters;
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> merged;
    for (auto& s : in) {
      const uint32_t id = uint32_t(std::lower_bound(names.begin(), names.end(), s.f) - names.begin());
      auto& l = merged[{id, s.g}];
      for (uint32_t m : s.mem)
        if (std::find(l.begin(), l.end(), m) == l.end()) l.push_back(m);
    }
    for (auto& kv : merged)
      if (!kv.second.empty()) slots.push_back({Key{names[kv.first.first], kv.first.second}, kv.second});
    if (prev)
      for (auto& s : slots) {
        bool had = false;
        for (auto& p : prev->slots) had |= p.first == s.first;
        if (!had) continue;
        if (prev->rr.count(s.first)) rr[s.first] = prev->rr.at(s.first);
        if (prev->st.count(s.first) &&
            std::find(s.second.begin(), s.second.end(), prev->st.at(s.first)) != s.second.end())
          st[s.first] = prev->st.at(s.first);
      }
  }
  uint32_t fid(uint32_t s) const {
    return uint32_t(std::lower_bound(names.begin(), names.end(), slots[s].first.first) - names.begin());
  }
  uint32_t pick(uint32_t strategy, uint32_t s, uint32_t row, uint32_t h, uint32_t seed) {
    const Key& k = slots[s].first;
    const auto& mem = slots[s].second;
    const uint32_t count = uint32_t(mem.size());
    if (strategy == EMQX_GM_SHARE_STICKY) {
      if (st.count(k) && std::find(mem.begin(), mem.end(), st[k]) != mem.end()) return st[k];
      return st[k] = count == 1 ? mem[0] : mem[gm::sh_mix(seed, s) % count];
    }
    if (count == 1) return mem[0];
    if (strategy == EMQX_GM_SHARE_HASH) return mem[h % count];
    if (strategy == EMQX_GM_SHARE_RANDOM) return mem[gm::sh_mix3(seed, row, s) % count];
    const uint32_t rem = rr.count(k) ? (rr[k] + 1) % count : gm::sh_mix(seed, s) % count;
    rr[k] = rem;
    return mem[rem];
  }
};

emqx_gm_shared* compile(const std::vector<std::string>& filters, const std::vector<Slot>& in,
                        const emqx_gm_shared* prev) {
  std::vector<std::string> sf;
  std::vector<uint32_t> g, mi;
  std::vector<uint64_t> mo{0};
  for (auto& s : in) {
    sf.push_back(s.f);
    g.push_back(s.g);
    mi.insert(mi.end(), s.mem.begin(), s.mem.end());
    mo.push_back(mi.size());
  }
  Packed pf(filters), ps(sf);
  if (g.empty()) g.push_back(0);
  if (mi.empty()) mi.push_back(0);
  emqx_gm_shared* sh = nullptr;
  if (emqx_gm_shared_compile_host(pf.b.data(), pf.o.data(), filters.size(), ps.b.data(), ps.o.data(), g.data(),
                                  in.size(), mo.data(), mi.data(), prev, &sh))
    return nullptr;
  return sh;
}

// every strategy over `calls` calls on the rows; 0 = all equal
int check_calls(emqx_gm_shared* sh, Ref& ref, const std::vector<std::vector<uint32_t>>& rows, int calls,
                uint32_t seed0) {
  std::vector<uint64_t> ro{0};
  std::vector<uint32_t> ids, hash;
  for (auto& r : rows) {
    ids.insert(ids.end(), r.begin(), r.end());
    ro.push_back(ids.size());
    hash.push_back(uint32_t(ro.size() * 2654435761u));
  }
  if (ids.empty()) ids.push_back(0);
  if (hash.empty()) hash.push_back(0);
  emqx_gm_csr m{};
  m.n_rows = rows.size();
  m.nnz = ro.back();
  m.row_off = ro.data();
  m.ids = ids.data();
  for (int c = 0; c < calls; ++c)
    for (uint32_t strategy = 0; strategy < 4; ++strategy) {
      const uint32_t seed = seed0 + uint32_t(c);
      emqx_gm_csr om, os;
      if (emqx_gm_shared_pick_host(sh, &m, strategy, hash.data(), seed, &om, &os)) return 1;
      uint64_t k = 0;
      int bad = 0;
      for (uint64_t r = 0; r < rows.size() && !bad; ++r) {
        if (om.row_off[r] != k || os.row_off[r] != k) bad = 2;
        for (uint32_t f : rows[r])
          for (uint32_t s = 0; s < ref.slots.size() && !bad; ++s) {
            if (ref.fid(s) != f) continue;
            if (k >= om.nnz || os.ids[k] != s || om.ids[k] != ref.pick(strategy, s, uint32_t(r), hash[r], seed))
              bad = 3;
            ++k;
          }
      }
      if (!bad && (k != om.nnz || om.row_off[rows.size()] != k)) bad = 4;
      emqx_gm_shared_csr_free_host(&om);
      emqx_gm_shared_csr_free_host(&os);
      if (bad) return std::printf("strategy %u call %d: %d\n", strategy, c, bad), bad;
    }
  return 0;
}

}  // namespace

int main() {
  std::mt19937 rng(5);
  auto pick = [&](size_t n) { return uint32_t(rng() % n); };
  std::vector<std::string> filters;
  for (int i = 0; i < 200; ++i) filters.push_back("f/" + std::to_string(1000 + i) + (i % 3 ? "/+" : "/#"));
  filters.push_back(std::string("nul\0in", 6));
  filters.push_back("\xff\xfe/+");
  filters.push_back("");
  auto gen_slots = [&](int n) {
    std::vector<Slot> v;
    for (int i = 0; i < n; ++i) {
      Slot s{filters[pick(filters.size() / 2) * 2 % filters.size()], pick(4), {}};
      const uint32_t cnt = std::vector<uint32_t>{0, 1, 1, 2, 3, 5, 64, 65, 70}[pick(9)], base = pick(5000);
      for (uint32_t k = 0; k < cnt; ++k) s.mem.push_back(base + pick(2 * cnt));
      v.push_back(s);
    }
    v.push_back(Slot{std::string("nul\0in", 6), 1, {1, 2, 3}});
    v.push_back(Slot{"", 0, {4, 4, 5}});
    return v;
  };
  auto gen_rows = [&](size_t nf, int n) {
    std::vector<std::vector<uint32_t>> rows;
    for (int i = 0; i < n; ++i) {
      std::vector<uint32_t> r;
      for (uint32_t k = 0, c = std::vector<uint32_t>{0, 1, 1, 2, 3, 6}[pick(6)]; k < c; ++k) r.push_back(pick(nf));
      std::sort(r.begin(), r.end());
      rows.push_back(r);
    }
    return rows;
  };
  const auto s1 = gen_slots(180);
  emqx_gm_shared* t1 = compile(filters, s1, nullptr);
  if (!t1) return std::printf("compile 1\n"), 1;
  Ref r1(filters, s1, nullptr);
  emqx_gm_shared_info_t info;
  emqx_gm_shared_info(t1, &info);
  if (info.n_slots != r1.slots.size()) return std::printf("slots %llu\n", (unsigned long long)info.n_slots), 1;
  for (uint32_t s = 0; s < r1.slots.size(); ++s) {
    uint32_t f, g;
    const uint32_t* mem;
    uint64_t nm;
    if (emqx_gm_shared_slot(t1, s, &f, &g, &mem, &nm) || f != r1.fid(s) || g != r1.slots[s].first.second ||
        std::vector<uint32_t>(mem, mem + nm) != r1.slots[s].second)
      return std::printf("slot %u\n", s), 1;
  }
  if (emqx_gm_shared_slot(t1, uint32_t(r1.slots.size()), nullptr, nullptr, nullptr, nullptr) != EMQX_GM_EINVAL) return 1;
  if (check_calls(t1, r1, gen_rows(r1.names.size(), 600), 3, 100)) return 1;
  // a rebuild with prev: other members, filters added in front (every id shifts)
  std::vector<std::string> filters2 = filters;
  for (int i = 0; i < 30; ++i) filters2.push_back("a/" + std::to_string(i));
  const auto s2 = gen_slots(160);
  emqx_gm_shared* t2 = compile(filters2, s2, t1);
  if (!t2) return std::printf("compile 2\n"), 1;
  Ref r2(filters2, s2, &r1);
  if (check_calls(t2, r2, gen_rows(r2.names.size(), 600), 2, 200)) return 1;
  // empty table, empty rows
  emqx_gm_shared* t0 = compile(filters, {}, t2);
  Ref r0(filters, {}, &r2);
  if (!t0 || check_calls(t0, r0, gen_rows(r0.names.size(), 20), 1, 1)) return std::printf("empty table\n"), 1;
  if (check_calls(t2, r2, {}, 1, 1)) return std::printf("empty rows\n"), 1;
  // refused inputs
  {
    emqx_gm_shared* bad = compile(filters, {Slot{"not/in/the/snapshot", 0, {1}}}, nullptr);
    if (bad) return 1;
    bad = compile(filters, {Slot{filters[0], 0, {0xFFFFFFFFu}}}, nullptr);
    if (bad) return 1;
    Packed pf(filters);
    const uint8_t b[8] = {'f', '/', '1', '0', '0', '0', '/', '#'};
    const uint64_t down[3] = {0, 8, 4}, far[2] = {0, uint64_t(1) << 40}, mo[3] = {0, 1, 2}, mdown[3] = {0, 2, 1};
    const uint32_t g[2] = {0, 0}, mi[2] = {1, 2};
    emqx_gm_shared* sh = nullptr;
    if (emqx_gm_shared_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, down, g, 2, mo, mi, nullptr, &sh) !=
            EMQX_GM_EINVAL || sh)
      return 1;
    if (emqx_gm_shared_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, far, g, 1, mo, mi, nullptr, &sh) !=
            EMQX_GM_EINVAL || sh)
      return 1;
    const uint64_t one[2] = {0, 8};
    if (emqx_gm_shared_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, one, g, 1, mdown + 1, mi, nullptr,
                                    &sh) != EMQX_GM_EINVAL || sh)
      return 1;
    // rows: an id past the snapshot, descending offsets, HASH without hashes
    uint64_t ro[3] = {0, 1, 2};
    uint32_t ids[2] = {0, uint32_t(r1.names.size())};
    emqx_gm_csr m{};
    m.n_rows = 2, m.nnz = 2, m.row_off = ro, m.ids = ids;
    emqx_gm_csr om, os;
    if (emqx_gm_shared_pick_host(t1, &m, EMQX_GM_SHARE_RANDOM, nullptr, 0, &om, &os) != EMQX_GM_EINVAL) return 1;
    ids[1] = 0;
    ro[1] = 2, ro[2] = 1;
    if (emqx_gm_shared_pick_host(t1, &m, EMQX_GM_SHARE_RANDOM, nullptr, 0, &om, &os) != EMQX_GM_EINVAL) return 1;
    ro[1] = 1, ro[2] = 2;
    if (emqx_gm_shared_pick_host(t1, &m, EMQX_GM_SHARE_HASH, nullptr, 0, &om, &os) != EMQX_GM_EINVAL) return 1;
    if (emqx_gm_shared_pick_host(t1, &m, 9, nullptr, 0, &om, &os) != EMQX_GM_EINVAL) return 1;
  }
  emqx_gm_shared_release(t0);
  emqx_gm_shared_release(t1);
  emqx_gm_shared_release(t2);
  std::printf("asan_shared ok\n");
  return 0;
}
