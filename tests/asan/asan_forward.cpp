// tests/asan/asan_forward.cpp — TEST ONLY: the route-destination table compiler
// and the host walk (emqx_amd/csrc/gm_dests.cpp) built as host C++ with
// AddressSanitizer + UBSan.  It compiles random route sets (duplicate pairs,
// filters without routes, 1 to 4096 nodes), walks random rows with and without
// a skipped node and checks every list against a brute-force restatement
// (a std::map bag walked row by row); then empty tables and rows, the
// SKIP_UNKNOWN flag, and refused inputs.  Never touches a device.  Built by
// `make -C emqx_amd/csrc asan-forward`, run by
// tests/test_forward_cpu.py::test_compiler_and_host_walk_under_asan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_dests.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
void dt_free_device(emqx_gm_dests*) {}  // gm_dests.hip's: a host-only table never gets there
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

using Route = std::pair<std::string, uint32_t>;

emqx_gm_dests* compile(const std::vector<std::string>& filters, const std::vector<Route>& routes, uint32_t n_nodes,
                       uint32_t flags = 0, int* rc_out = nullptr) {
  std::vector<std::string> rf;
  std::vector<uint32_t> nodes;
  for (auto& r : routes) {
    rf.push_back(r.first);
    nodes.push_back(r.second);
  }
  Packed pf(filters), pr(rf);
  if (nodes.empty()) nodes.push_back(0);
  emqx_gm_dests* dt = nullptr;
  const int rc = emqx_gm_dests_compile_host(pf.b.data(), pf.o.data(), filters.size(), pr.b.data(), pr.o.data(),
                                            nodes.data(), routes.size(), n_nodes, flags, &dt);
  if (rc_out) *rc_out = rc;
  return rc ? nullptr : dt;
}

// the bag walked row by row; 0 = the plan equals it
int check_plan(emqx_gm_dests* dt, std::vector<std::string> names, const std::vector<Route>& routes, uint32_t n_nodes,
               const std::vector<std::vector<uint32_t>>& rows, uint32_t skip) {
  std::sort(names.begin(), names.end());
  names.erase(std::unique(names.begin(), names.end()), names.end());
  std::map<uint32_t, std::set<uint32_t>> bag;  // filter id -> nodes
  for (auto& r : routes) {
    const auto it = std::lower_bound(names.begin(), names.end(), r.first);
    if (it != names.end() && *it == r.first) bag[uint32_t(it - names.begin())].insert(r.second);
  }
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> want(n_nodes);
  std::vector<uint32_t> counts;
  for (uint32_t r = 0; r < rows.size(); ++r) {
    uint32_t all = 0;
    for (uint32_t f : rows[r])
      if (bag.count(f))
        for (uint32_t node : bag[f]) {
          ++all;
          if (node != skip) want[node].push_back({r, f});
        }
    counts.push_back(all);
  }
  std::vector<uint64_t> ro{0};
  std::vector<uint32_t> ids;
  for (auto& r : rows) {
    ids.insert(ids.end(), r.begin(), r.end());
    ro.push_back(ids.size());
  }
  if (ids.empty()) ids.push_back(0);
  emqx_gm_csr m{};
  m.n_rows = rows.size();
  m.nnz = ro.back();
  m.row_off = ro.data();
  m.ids = ids.data();
  emqx_gm_forwards fw;
  if (emqx_gm_forward_plan_host(dt, &m, skip, &fw)) return 1;
  int bad = 0;
  if (fw.n_nodes != n_nodes || fw.n_rows != rows.size() || fw.on_device || fw.node_off[0] != 0) bad = 2;
  for (uint32_t k = 0; k < n_nodes && !bad; ++k) {
    if (fw.node_off[k + 1] - fw.node_off[k] != want[k].size()) bad = 3;
    for (uint64_t i = 0; i < want[k].size() && !bad; ++i)
      if (fw.rows[fw.node_off[k] + i] != want[k][i].first || fw.filters[fw.node_off[k] + i] != want[k][i].second)
        bad = 4;
  }
  if (!bad && fw.node_off[n_nodes] != fw.n_pairs) bad = 5;
  for (uint32_t r = 0; r < rows.size() && !bad; ++r)
    if (fw.row_routes[r] != counts[r]) bad = 6;
  emqx_gm_forwards_free_host(&fw);
  if (bad) std::printf("plan: %d (n_nodes %u skip %u)\n", bad, n_nodes, skip);
  return bad;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  auto pick = [&](size_t n) { return uint32_t(rng() % n); };
  std::vector<std::string> filters;
  for (int i = 0; i < 200; ++i) filters.push_back("f/" + std::to_string(1000 + i) + (i % 3 ? "/+" : "/#"));
  filters.push_back(std::string("nul\0in", 6));
  filters.push_back("\xff\xfe/+");
  filters.push_back("");
  filters.push_back(filters[3]);  // a duplicate in the index's filter set
  const size_t n_ids = filters.size() - 1;
  auto gen_rows = [&](int n) {
    std::vector<std::vector<uint32_t>> rows;
    for (int i = 0; i < n; ++i) {
      std::vector<uint32_t> r;
      for (uint32_t k = 0, c = std::vector<uint32_t>{0, 1, 1, 2, 3, 6}[pick(6)]; k < c; ++k) r.push_back(pick(n_ids));
      rows.push_back(r);
    }
    return rows;
  };
  for (uint32_t n_nodes : {1u, 2u, 9u, 64u, 65u, 4096u}) {
    std::vector<Route> routes;
    for (int i = 0; i < 400; ++i) routes.push_back({filters[pick(filters.size() / 2) * 2 % filters.size()], pick(n_nodes)});
    for (int i = 0; i < 40; ++i) routes.push_back(routes[pick(routes.size())]);  // pairs given twice
    for (uint32_t k = 0; k < std::min(n_nodes, 300u); ++k) routes.push_back({filters[1], n_nodes - 1 - k});  // a long list
    routes.push_back({std::string("nul\0in", 6), 0});
    routes.push_back({"", n_nodes - 1});
    emqx_gm_dests* dt = compile(filters, routes, n_nodes);
    if (!dt) return std::printf("compile %u\n", n_nodes), 1;
    std::set<Route> distinct(routes.begin(), routes.end());
    emqx_gm_dests_info_t info;
    emqx_gm_dests_info(dt, &info);
    if (info.n_routes != distinct.size() || info.n_nodes != n_nodes || info.device_bytes || info.n_skipped_unknown)
      return std::printf("info %u\n", n_nodes), 1;
    const auto rows = gen_rows(500);
    for (uint32_t skip : {EMQX_GM_DESTS_NO_SKIP, 0u, n_nodes - 1, n_nodes + 5})
      if (check_plan(dt, filters, routes, n_nodes, rows, skip)) return 1;
    if (check_plan(dt, filters, routes, n_nodes, {}, 0)) return std::printf("empty rows\n"), 1;
    if (check_plan(dt, filters, routes, n_nodes, {{}, {}, {}}, 0)) return std::printf("all-empty rows\n"), 1;
    double ms[4];
    if (emqx_gm_dests_last_times(dt, ms) || ms[3] != 0) return 1;
    emqx_gm_dests_release(dt);
  }
  // an empty table
  {
    emqx_gm_dests* t0 = compile(filters, {}, 3);
    if (!t0 || check_plan(t0, filters, {}, 3, gen_rows(20), 1)) return std::printf("empty table\n"), 1;
    emqx_gm_dests_release(t0);
    emqx_gm_dests* t1 = compile({}, {}, 1);
    if (!t1 || check_plan(t1, {}, {}, 1, {{}, {}}, 0)) return std::printf("empty index\n"), 1;
    emqx_gm_dests_release(t1);
  }
  // refused inputs
  {
    int rc = 0;
    if (compile(filters, {{"not/in/the/snapshot", 0}}, 2, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    emqx_gm_dests* sk = compile(filters, {{"not/in/the/snapshot", 0}, {filters[0], 1}, {"nor/this", 1}}, 2,
                                EMQX_GM_DESTS_SKIP_UNKNOWN, &rc);
    emqx_gm_dests_info_t info;
    if (!sk || emqx_gm_dests_info(sk, &info) || info.n_routes != 1 || info.n_skipped_unknown != 2) return 1;
    if (check_plan(sk, filters, {{filters[0], 1}}, 2, gen_rows(50), EMQX_GM_DESTS_NO_SKIP)) return 1;
    if (compile(filters, {{filters[0], 2}}, 2, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(filters, {}, 0, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(filters, {}, 4097, 0, &rc) || rc != EMQX_GM_EINVAL) return 1;
    if (compile(filters, {}, 2, 0x8, &rc) || rc != EMQX_GM_EINVAL) return 1;
    Packed pf(filters);
    const uint8_t b[8] = {'f', '/', '1', '0', '0', '0', '/', '#'};
    const uint64_t down[3] = {0, 8, 4}, far[2] = {0, uint64_t(1) << 40};
    const uint32_t nodes[2] = {0, 0};
    emqx_gm_dests* dt = nullptr;
    if (emqx_gm_dests_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, down, nodes, 2, 1, 0, &dt) !=
            EMQX_GM_EINVAL || dt)
      return 1;
    if (emqx_gm_dests_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, far, nodes, 1, 1, 0, &dt) !=
            EMQX_GM_EINVAL || dt)
      return 1;
    if (emqx_gm_dests_compile_host(pf.b.data(), pf.o.data(), filters.size(), b, down, nullptr, 1, 1, 0, &dt) !=
            EMQX_GM_EINVAL || dt)
      return 1;
    // rows: an id past the snapshot, descending offsets, offsets that do not span the ids, device rows
    uint64_t ro[3] = {0, 1, 2};
    uint32_t ids[2] = {0, uint32_t(n_ids)};
    emqx_gm_csr m{};
    m.n_rows = 2, m.nnz = 2, m.row_off = ro, m.ids = ids;
    emqx_gm_forwards fw;
    if (emqx_gm_forward_plan_host(sk, &m, 0, &fw) != EMQX_GM_EINVAL || fw.node_off) return 1;
    ids[1] = 0;
    ro[1] = 2, ro[2] = 1;
    if (emqx_gm_forward_plan_host(sk, &m, 0, &fw) != EMQX_GM_EINVAL) return 1;
    ro[1] = 1, ro[2] = 1;
    if (emqx_gm_forward_plan_host(sk, &m, 0, &fw) != EMQX_GM_EINVAL) return 1;
    ro[2] = 2;
    m.on_device = 1;
    if (emqx_gm_forward_plan_host(sk, &m, 0, &fw) != EMQX_GM_EINVAL) return 1;
    m.on_device = 0;
    if (emqx_gm_forward_plan_host(sk, &m, 0, &fw) != EMQX_GM_OK || emqx_gm_forwards_free_host(&fw)) return 1;
    if (emqx_gm_forwards_free_host(nullptr) != EMQX_GM_EINVAL) return 1;
    emqx_gm_dests_release(sk);
  }
  std::printf("asan_forward ok\n");
  return 0;
}
