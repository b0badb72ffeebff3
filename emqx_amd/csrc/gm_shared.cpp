// gm_shared.cpp — host compiler of the shared-subscription table, the host walk
// over it, and the host-only part of the emqx_gm_shared_* boundary (layout and
// the mix functions: gm_shared.h; kernels and the device entry points:
// gm_shared.hip).  Replaces the member selection of emqx_shared_sub:dispatch/3
// (pick/6 .. do_pick_subscriber/6, apps/emqx/src/emqx_shared_sub.erl:234-288).
// Plain host C++: it also builds under a sanitizer without a device
// (tests/asan/asan_shared.cpp).
#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "gm_shared.h"

namespace gm {

namespace {

std::string slot_key(const uint8_t* p, uint64_t len, uint32_t group) {
  std::string k(reinterpret_cast<const char*>(&group), 4);
  if (len) k.append(reinterpret_cast<const char*>(p), len);
  return k;
}

void set_views(emqx_gm_shared* sh, const size_t* o) {
  uint8_t* base = sh->blob.data();
  ShView& v = sh->hv;
  v.sh_off = reinterpret_cast<const uint32_t*>(base + o[0]);
  v.mem_off = reinterpret_cast<const uint32_t*>(base + o[1]);
  v.filter = reinterpret_cast<const uint32_t*>(base + o[2]);
  v.group = reinterpret_cast<const uint32_t*>(base + o[3]);
  v.mem_ids = reinterpret_cast<const uint32_t*>(base + o[4]);
  v.rr = reinterpret_cast<uint32_t*>(base + o[5]);
  v.st = reinterpret_cast<uint32_t*>(base + o[6]);
  sh->dv = sh->hv;  // (sh_upload rebases the pointers onto the device allocation)
}

}  // namespace

int sh_compile(const ShInput& in, uint64_t n_filters,
               const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve, const emqx_gm_shared* prev,
               const uint32_t* prev_rr, const uint32_t* prev_st, emqx_gm_shared** out, std::string* why) {
  const uint64_t n = in.n_slots;
  if (const int rc = check_offsets(in.fb, in.fo, n, why)) return rc;
  if (n && (!in.group_ids || !in.mem_off)) {
    *why = "NULL buffer";
    return EMQX_GM_EINVAL;
  }
  if (n_filters >= 0xFFFFFFFFull) {
    *why = "a snapshot of 2^32 - 1 filters or more";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (in.mem_off[i + 1] < in.mem_off[i]) {
      *why = "member offsets not ascending at " + std::to_string(i);
      return EMQX_GM_EINVAL;
    }
  const uint64_t n_mem_in = n ? in.mem_off[n] - in.mem_off[0] : 0;
  if (n_mem_in >= 0xFFFFFFFFull || (n_mem_in && !in.mem_ids)) {
    *why = n_mem_in && !in.mem_ids ? "NULL buffer" : "more than 2^32 - 2 members";
    return EMQX_GM_EINVAL;
  }
  // 1. each input's filter id in the bound snapshot
  std::vector<uint32_t> fid(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* p = in.fb + in.fo[i];
    const uint64_t len = in.fo[i + 1] - in.fo[i];
    if (!resolve(p, len, &fid[i]) || fid[i] >= n_filters) {
      *why = "filter '" + std::string(reinterpret_cast<const char*>(p), std::min<uint64_t>(len, 200)) +
             "' is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
  }
  // 2. slots by (filter id, group id); equal pairs merged in input order
  std::vector<uint64_t> ord(n);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
    return fid[a] != fid[b] ? fid[a] < fid[b] : in.group_ids[a] < in.group_ids[b];
  });
  std::vector<uint32_t> s_filter, s_group, s_moff{0}, mem;
  std::vector<uint64_t> s_input;  // slot -> an input carrying its filter bytes
  std::unordered_set<uint32_t> seen;
  for (uint64_t k = 0; k < n;) {
    uint64_t e = k;
    seen.clear();
    const size_t m0 = mem.size();
    while (e < n && fid[ord[e]] == fid[ord[k]] && in.group_ids[ord[e]] == in.group_ids[ord[k]]) {
      const uint64_t i = ord[e];
      for (uint64_t q = in.mem_off[i]; q < in.mem_off[i + 1]; ++q) {
        const uint32_t id = in.mem_ids[q];
        if (id == SH_UNSET) {
          *why = "member id 2^32 - 1 is reserved";
          return EMQX_GM_EINVAL;
        }
        if (seen.insert(id).second) mem.push_back(id);  // an identical member is stored once (the first)
      }
      ++e;
    }
    if (mem.size() > m0) {  // a slot with no members does not exist
      s_filter.push_back(fid[ord[k]]);
      s_group.push_back(in.group_ids[ord[k]]);
      s_moff.push_back(uint32_t(mem.size()));
      s_input.push_back(ord[k]);
    }
    k = e;
  }
  const uint64_t S = s_filter.size(), M = mem.size();
  // 3. the arrays
  size_t o[7], at = 0;
  o[0] = at, at = al16(at + (n_filters + 1) * 4);
  o[1] = at, at = al16(at + (S + 1) * 4);
  o[2] = at, at = al16(at + (S + 1) * 4);
  o[3] = at, at = al16(at + (S + 1) * 4);
  o[4] = at, at = al16(at + (M + 1) * 4);
  o[5] = at, at = al16(at + (S + 1) * 4);
  o[6] = at, at = al16(at + (S + 1) * 4);
  auto* sh = new emqx_gm_shared;
  sh->blob.resize(at);
  std::memset(sh->blob.data(), 0, at);
  sh->bytes = at;
  set_views(sh, o);
  uint8_t* base = sh->blob.data();
  auto* sh_off = reinterpret_cast<uint32_t*>(base + o[0]);
  {
    uint64_t s = 0;
    for (uint64_t f = 0; f <= n_filters; ++f) {
      while (s < S && s_filter[s] < f) ++s;
      sh_off[f] = uint32_t(s);
    }
  }
  std::memcpy(base + o[1], s_moff.data(), (S + 1) * 4);
  if (S) std::memcpy(base + o[2], s_filter.data(), S * 4);
  if (S) std::memcpy(base + o[3], s_group.data(), S * 4);
  if (M) std::memcpy(base + o[4], mem.data(), M * 4);
  for (uint64_t s = 0; s <= S; ++s) sh->hv.rr[s] = sh->hv.st[s] = SH_UNSET;
  sh->foff.assign(1, 0);
  for (uint64_t s = 0; s < S; ++s) {
    const uint64_t i = s_input[s];
    sh->fbytes.insert(sh->fbytes.end(), in.fb + in.fo[i], in.fb + in.fo[i + 1]);
    sh->foff.push_back(sh->fbytes.size());
  }
  // 4. carry-over by (filter bytes, group id): filter ids shift between snapshots
  if (prev && prev->hv.n_slots && prev_rr && prev_st) {
    std::unordered_map<std::string, uint32_t> at_prev;
    for (uint32_t s = 0; s < prev->hv.n_slots; ++s)
      at_prev.emplace(slot_key(prev->fbytes.data() + prev->foff[s], prev->foff[s + 1] - prev->foff[s], prev->hv.group[s]), s);
    for (uint64_t s = 0; s < S; ++s) {
      const auto it = at_prev.find(slot_key(sh->fbytes.data() + sh->foff[s], sh->foff[s + 1] - sh->foff[s], s_group[s]));
      if (it == at_prev.end()) continue;
      sh->hv.rr[s] = prev_rr[it->second];
      const uint32_t st = prev_st[it->second];
      if (st != SH_UNSET && std::find(mem.begin() + s_moff[s], mem.begin() + s_moff[s + 1], st) != mem.begin() + s_moff[s + 1])
        sh->hv.st[s] = st;  // (a member that left the list loses stickiness here)
    }
  }
  uint64_t with_slots = 0;
  for (uint64_t s = 0; s < S; ++s) with_slots += !s || s_filter[s] != s_filter[s - 1];
  for (ShView* v : {&sh->hv, &sh->dv}) {
    v->n_filters = uint32_t(n_filters);
    v->n_slots = uint32_t(S);
    v->n_members = uint32_t(M);
  }
  sh->info.n_slots = S;
  sh->info.n_members = M;
  sh->info.n_filters_with_slots = with_slots;
  sh->info.device_bytes = 0;
  *out = sh;
  return EMQX_GM_OK;
}

int sh_check_rows(const emqx_gm_shared* sh, const emqx_gm_csr* m, std::string* why) {
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
    if (m->ids[j] >= sh->hv.n_filters) {
      *why = "filter id " + std::to_string(m->ids[j]) + " is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
  return EMQX_GM_OK;
}

// pick/6 + do_pick_subscriber/6 hit by hit in batch order over the host state
int sh_pick_host(emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy, const uint32_t* msg_hash, uint32_t seed,
                 std::vector<uint64_t>& row_off, std::vector<uint32_t>& members, std::vector<uint32_t>& slots) {
  const ShView& v = sh->hv;
  row_off.assign(m->n_rows + 1, 0);
  members.clear();
  slots.clear();
  for (uint64_t r = 0; r < m->n_rows; ++r) {
    row_off[r] = members.size();
    for (uint64_t j = m->row_off[r]; j < m->row_off[r + 1]; ++j) {
      const uint32_t f = m->ids[j];
      for (uint32_t s = v.sh_off[f]; s < v.sh_off[f + 1]; ++s) {
        const uint32_t* mem = v.mem_ids + v.mem_off[s];
        const uint32_t count = v.mem_off[s + 1] - v.mem_off[s];
        uint32_t got;
        if (strategy == EMQX_GM_SHARE_STICKY) {  // pick(sticky, ...), :234-247: whatever is picked is stored
          if (v.st[s] == SH_UNSET) v.st[s] = mem[count == 1 ? 0 : sh_mix(seed, s) % count];
          got = v.st[s];
        } else if (count == 1) {  // pick_subscriber/6, first clause: no state read or written
          got = mem[0];
        } else if (strategy == EMQX_GM_SHARE_HASH) {
          got = mem[msg_hash[r] % count];
        } else if (strategy == EMQX_GM_SHARE_ROUND_ROBIN) {
          const uint32_t rem = v.rr[s] == SH_UNSET ? sh_mix(seed, s) % count : uint32_t((uint64_t(v.rr[s]) + 1) % count);
          v.rr[s] = rem;
          got = mem[rem];
        } else {
          got = mem[sh_mix3(seed, uint32_t(r), s) % count];
        }
        if (members.size() >= 0xFFFFFFFEull) return EMQX_GM_EOVERFLOW;
        members.push_back(got);
        slots.push_back(s);
      }
    }
  }
  row_off[m->n_rows] = members.size();
  return EMQX_GM_OK;
}

}  // namespace gm

extern "C" {

int emqx_gm_shared_compile_host(const uint8_t* ifb, const uint64_t* ifo, uint64_t n_index, const uint8_t* fb,
                                const uint64_t* fo, const uint32_t* group_ids, uint64_t n_slots,
                                const uint64_t* mem_off, const uint32_t* mem_ids, const emqx_gm_shared* prev,
                                emqx_gm_shared** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(ifb, ifo, n_index, &why))
    return gm::set_err(nullptr, rc, "shared_compile_host: index filters: " + why);
  if (prev && prev->dev_base)
    return gm::set_err(nullptr, EMQX_GM_EUNSUPPORTED, "shared_compile_host: prev is a device table");
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
  const gm::ShInput in{fb, fo, group_ids, n_slots, mem_off, mem_ids};
  const int rc = gm::sh_compile(in, fs.size(), resolve, prev, prev ? prev->hv.rr : nullptr,
                                prev ? prev->hv.st : nullptr, out, &why);
  return rc ? gm::set_err(nullptr, rc, "shared_compile_host: " + why) : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_shared_pick_host(emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy, const uint32_t* msg_hash,
                             uint32_t seed, emqx_gm_csr* out_members, emqx_gm_csr* out_slots) {
  if (!sh || !m || !out_members || !out_slots) return EMQX_GM_EINVAL;
  std::memset(out_members, 0, sizeof(*out_members));
  std::memset(out_slots, 0, sizeof(*out_slots));
  if (sh->dev_base)
    return gm::set_err(nullptr, EMQX_GM_EUNSUPPORTED, "shared_pick_host: a device table (its state lives there)");
  if (m->on_device) return gm::set_err(nullptr, EMQX_GM_EINVAL, "shared_pick_host: device rows");
  if (strategy > EMQX_GM_SHARE_RANDOM) return gm::set_err(nullptr, EMQX_GM_EINVAL, "shared_pick_host: strategy");
  if (strategy == EMQX_GM_SHARE_HASH && !msg_hash && m->n_rows)
    return gm::set_err(nullptr, EMQX_GM_EINVAL, "shared_pick_host: msg_hash is required for EMQX_GM_SHARE_HASH");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::sh_check_rows(sh, m, &why)) return gm::set_err(nullptr, rc, "shared_pick_host: " + why);
  std::lock_guard<std::mutex> lk(sh->mu);
  std::vector<uint64_t> ro;
  std::vector<uint32_t> mem, slots;
  if (const int rc = gm::sh_pick_host(sh, m, strategy, msg_hash, seed, ro, mem, slots))
    return gm::set_err(nullptr, rc, "shared_pick_host: 2^32 - 1 hits or more");
  int rc = gm::csr_to_malloc(ro, mem, out_members);
  if (!rc) rc = gm::csr_to_malloc(ro, slots, out_slots);
  if (rc) {
    gm::csr_free_malloc(out_members);
    gm::csr_free_malloc(out_slots);
    return gm::set_err(nullptr, rc, "shared_pick_host: result");
  }
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_shared_csr_free_host(emqx_gm_csr* csr) { return gm::csr_free_malloc(csr); }

int emqx_gm_shared_slot(const emqx_gm_shared* sh, uint32_t slot, uint32_t* filter_id, uint32_t* group_id,
                        const uint32_t** members, uint64_t* n_members) {
  if (!sh || slot >= sh->hv.n_slots) return EMQX_GM_EINVAL;
  if (filter_id) *filter_id = sh->hv.filter[slot];
  if (group_id) *group_id = sh->hv.group[slot];
  if (members) *members = sh->hv.mem_ids + sh->hv.mem_off[slot];
  if (n_members) *n_members = sh->hv.mem_off[slot + 1] - sh->hv.mem_off[slot];
  return EMQX_GM_OK;
}

int emqx_gm_shared_info(const emqx_gm_shared* sh, emqx_gm_shared_info_t* info) {
  if (!sh || !info) return EMQX_GM_EINVAL;
  *info = sh->info;
  return EMQX_GM_OK;
}

int emqx_gm_shared_release(emqx_gm_shared* sh) {
  if (!sh) return EMQX_GM_EINVAL;
  if (sh->dev_base) gm::sh_free_device(sh);
  if (sh->idx) emqx_gm_index_release(sh->idx);
  delete sh;
  return EMQX_GM_OK;
}

int emqx_gm_shared_last_times(const emqx_gm_shared* sh, double* ms4) {
  if (!sh || !ms4) return EMQX_GM_EINVAL;
  for (int k = 0; k < 4; ++k) ms4[k] = sh->last_ms[k];
  return EMQX_GM_OK;
}

}  // extern "C"
