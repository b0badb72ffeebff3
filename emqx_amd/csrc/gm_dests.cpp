// gm_dests.cpp — host compiler of the route-destination table, the host walk
// over it, and the host-only part of the emqx_gm_dests_* / emqx_gm_forward_*
// boundary (layout and the chunk rule: gm_dests.h; kernels and the device entry
// points: gm_dests.hip).  Replaces lookup_routes/1 + one forward/3 per (message,
// route) (apps/emqx/src/emqx_router.erl:136, emqx_broker.erl:245-293) by one
// forward list per node per window.
// Plain host C++: it also builds under a sanitizer without a device
// (tests/asan/asan_forward.cpp).
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "gm_dests.h"

namespace gm {

int dt_compile(const DtInput& in, uint64_t n_filters,
               const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve, emqx_gm_dests** out,
               std::string* why) {
  const uint64_t n = in.n_routes;
  if (in.n_nodes < 1 || in.n_nodes > EMQX_GM_DESTS_MAX_NODES) {
    *why = "n_nodes " + std::to_string(in.n_nodes) + " is outside [1, " + std::to_string(EMQX_GM_DESTS_MAX_NODES) + "]";
    return EMQX_GM_EINVAL;
  }
  if (in.flags & ~EMQX_GM_DESTS_SKIP_UNKNOWN) {
    *why = "flags";
    return EMQX_GM_EINVAL;
  }
  if (const int rc = check_offsets(in.fb, in.fo, n, why)) return rc;
  if (n && !in.node_ids) {
    *why = "NULL buffer";
    return EMQX_GM_EINVAL;
  }
  if (n_filters >= 0xFFFFFFFFull) {
    *why = "a snapshot of 2^32 - 1 filters or more";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (in.node_ids[i] >= in.n_nodes) {
      *why = "route " + std::to_string(i) + ": node " + std::to_string(in.node_ids[i]) + " >= n_nodes";
      return EMQX_GM_EINVAL;
    }
  // 1. each route's filter id in the bound snapshot
  std::vector<std::pair<uint32_t, uint16_t>> pairs;
  pairs.reserve(n);
  uint64_t skipped = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* p = in.fb + in.fo[i];
    const uint64_t len = in.fo[i + 1] - in.fo[i];
    uint32_t f = 0;
    if (!resolve(p, len, &f) || f >= n_filters) {
      if (in.flags & EMQX_GM_DESTS_SKIP_UNKNOWN) {
        ++skipped;
        continue;
      }
      *why = "filter '" + std::string(reinterpret_cast<const char*>(p), std::min<uint64_t>(len, 200)) +
             "' is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
    pairs.emplace_back(f, uint16_t(in.node_ids[i]));
  }
  // 2. the bag: by (filter id, node), a pair given twice stored once
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  const uint64_t R = pairs.size();
  // 3. the arrays
  const size_t o_nodes = al16((n_filters + 1) * 4);
  const size_t at = al16(o_nodes + (R + 1) * 2);
  auto* dt = new emqx_gm_dests;
  dt->blob.resize(at);
  std::memset(dt->blob.data(), 0, at);
  dt->bytes = at;
  auto* d_off = reinterpret_cast<uint32_t*>(dt->blob.data());
  auto* nodes = reinterpret_cast<uint16_t*>(dt->blob.data() + o_nodes);
  uint64_t r = 0, with_routes = 0;
  for (uint64_t f = 0; f <= n_filters; ++f) {
    while (r < R && pairs[r].first < f) ++r;
    d_off[f] = uint32_t(r);
  }
  for (uint64_t k = 0; k < R; ++k) {
    nodes[k] = pairs[k].second;
    with_routes += !k || pairs[k].first != pairs[k - 1].first;
  }
  dt->hv = DtView{d_off, nodes, uint32_t(n_filters), uint32_t(R), in.n_nodes};
  dt->dv = dt->hv;  // (dt_upload rebases the pointers onto the device allocation)
  dt->info.n_routes = R;
  dt->info.n_filters_with_routes = with_routes;
  dt->info.n_skipped_unknown = skipped;
  dt->info.device_bytes = 0;
  dt->info.n_nodes = in.n_nodes;
  *out = dt;
  return EMQX_GM_OK;
}

int dt_check_rows(const emqx_gm_dests* dt, const emqx_gm_csr* m, std::string* why) {
  if (m->n_rows >= 0xFFFFFFFFull) {
    *why = "n_rows of 2^32 - 1 or more";
    return EMQX_GM_EINVAL;
  }
  if (!m->row_off || (m->nnz && !m->ids)) {
    *why = "NULL rows";
    return EMQX_GM_EINVAL;
  }
  if (m->on_device) return EMQX_GM_OK;  // (device rows: the kernels skip what they cannot index)
  if (m->row_off[0] != 0 || m->row_off[m->n_rows] != m->nnz) {
    *why = "row offsets do not span the ids";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t r = 0; r < m->n_rows; ++r)
    if (m->row_off[r + 1] < m->row_off[r]) {
      *why = "row offsets not ascending at " + std::to_string(r);
      return EMQX_GM_EINVAL;
    }
  for (uint64_t j = 0; j < m->nnz; ++j)
    if (m->ids[j] >= dt->hv.n_filters) {
      *why = "filter id " + std::to_string(m->ids[j]) + " is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
  return EMQX_GM_OK;
}

// route(aggre(match_routes(Topic))) -> forward/3 for every row in window order:
// a counting pass (per node, and per row), then the fill in batch order
int dt_plan_host(const emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node, emqx_gm_forwards* out) {
  const DtView& v = dt->hv;
  const uint64_t n = m->n_rows, N = v.n_nodes;
  std::vector<uint64_t> at(N + 1, 0);
  std::vector<uint32_t> rr(n, 0);
  uint64_t hits = 0;
  for (uint64_t r = 0; r < n; ++r) {
    uint64_t all = 0;
    for (uint64_t j = m->row_off[r]; j < m->row_off[r + 1]; ++j) {
      const uint32_t f = m->ids[j];
      all += v.d_off[f + 1] - v.d_off[f];
      for (uint32_t k = v.d_off[f]; k < v.d_off[f + 1]; ++k)
        if (v.nodes[k] != skip_node) {
          ++at[v.nodes[k] + 1];
          ++hits;
        }
    }
    rr[r] = uint32_t(std::min<uint64_t>(all, 0xFFFFFFFFull));
  }
  if (hits >= 0xFFFFFFFFull) return EMQX_GM_EOVERFLOW;
  for (uint64_t k = 0; k < N; ++k) at[k + 1] += at[k];
  out->node_off = static_cast<uint64_t*>(malloc((N + 1) * 8));
  out->rows = static_cast<uint32_t*>(malloc(std::max<uint64_t>(hits, 1) * 4));
  out->filters = static_cast<uint32_t*>(malloc(std::max<uint64_t>(hits, 1) * 4));
  out->row_routes = static_cast<uint32_t*>(malloc(std::max<uint64_t>(n, 1) * 4));
  if (!out->node_off || !out->rows || !out->filters || !out->row_routes) {
    fw_free_malloc(out);
    return EMQX_GM_ENOMEM;
  }
  std::memcpy(out->node_off, at.data(), (N + 1) * 8);
  if (n) std::memcpy(out->row_routes, rr.data(), n * 4);
  for (uint64_t r = 0; r < n; ++r)
    for (uint64_t j = m->row_off[r]; j < m->row_off[r + 1]; ++j) {
      const uint32_t f = m->ids[j];
      for (uint32_t k = v.d_off[f]; k < v.d_off[f + 1]; ++k) {
        const uint32_t node = v.nodes[k];
        if (node == skip_node) continue;
        const uint64_t p = at[node]++;
        out->rows[p] = uint32_t(r);
        out->filters[p] = f;
      }
    }
  out->n_rows = n;
  out->n_pairs = hits;
  out->n_nodes = uint32_t(N);
  out->on_device = 0;
  out->priv = nullptr;
  return EMQX_GM_OK;
}

}  // namespace gm

extern "C" {

int emqx_gm_dests_compile_host(const uint8_t* ifb, const uint64_t* ifo, uint64_t n_index, const uint8_t* fb,
                               const uint64_t* fo, const uint32_t* node_ids, uint64_t n_routes, uint32_t n_nodes,
                               uint32_t flags, emqx_gm_dests** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(ifb, ifo, n_index, &why))
    return gm::set_err(nullptr, rc, "dests_compile_host: index filters: " + why);
  // filter ids as emqx_gm_index_compile_host assigns them: the rank among the distinct filters
  std::vector<gm::WordRef> fs(n_index);
  for (uint64_t i = 0; i < n_index; ++i) fs[i] = gm::WordRef{ifb + ifo[i], ifo[i + 1] - ifo[i]};
  std::sort(fs.begin(), fs.end(), gm::word_less);
  fs.erase(std::unique(fs.begin(), fs.end(), gm::word_eq), fs.end());
  auto resolve = [&](const uint8_t* p, uint64_t len, uint32_t* id) {
    const gm::WordRef key{p, len};
    const auto it = std::lower_bound(fs.begin(), fs.end(), key, gm::word_less);
    if (it == fs.end() || gm::word_less(key, *it)) return false;
    *id = uint32_t(it - fs.begin());
    return true;
  };
  const gm::DtInput in{fb, fo, node_ids, n_routes, n_nodes, flags};
  const int rc = gm::dt_compile(in, fs.size(), resolve, out, &why);
  return rc ? gm::set_err(nullptr, rc, "dests_compile_host: " + why) : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_forward_plan_host(const emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node,
                              emqx_gm_forwards* out) {
  if (!dt || !m || !out) return EMQX_GM_EINVAL;
  std::memset(out, 0, sizeof(*out));
  if (m->on_device) return gm::set_err(nullptr, EMQX_GM_EINVAL, "forward_plan_host: device rows");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::dt_check_rows(dt, m, &why)) return gm::set_err(nullptr, rc, "forward_plan_host: " + why);
  const int rc = gm::dt_plan_host(dt, m, skip_node, out);
  if (rc)
    return gm::set_err(nullptr, rc, rc == EMQX_GM_EOVERFLOW ? "forward_plan_host: 2^32 - 1 hits or more"
                                                           : "forward_plan_host: result");
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_forwards_free_host(emqx_gm_forwards* fw) {
  if (!fw || fw->priv || fw->on_device) return EMQX_GM_EINVAL;
  return gm::fw_free_malloc(fw);
}

int emqx_gm_dests_info(const emqx_gm_dests* dt, emqx_gm_dests_info_t* info) {
  if (!dt || !info) return EMQX_GM_EINVAL;
  *info = dt->info;
  return EMQX_GM_OK;
}

int emqx_gm_dests_release(emqx_gm_dests* dt) {
  if (!dt) return EMQX_GM_EINVAL;
  if (dt->dev_base) gm::dt_free_device(dt);
  if (dt->idx) emqx_gm_index_release(dt->idx);
  delete dt;
  return EMQX_GM_OK;
}

int emqx_gm_dests_last_times(const emqx_gm_dests* dt, double* ms4) {
  if (!dt || !ms4) return EMQX_GM_EINVAL;
  std::lock_guard<std::mutex> lk(const_cast<emqx_gm_dests*>(dt)->mu);
  for (int k = 0; k < 4; ++k) ms4[k] = dt->last_ms[k];
  return EMQX_GM_OK;
}

}  // extern "C"
