// gm_subopts.cpp — host compiler of the subscription-option table, the host
// walk over it, and the host-only part of the emqx_gm_subopts_* /
// emqx_gm_deliver* boundary (layout and the byte rules: gm_subopts.h; kernels
// and the device entry points: gm_subopts.hip).  Replaces ignore_local/4 and
// enrich_deliver/2 per delivery (apps/emqx/src/emqx_session.erl:279-291,
// 560-602) by one option byte streamed beside each subscriber id.
// Plain host C++: it also builds under a sanitizer without a device
// (tests/asan/asan_subopts.cpp).
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gm_subopts.h"

namespace gm {

namespace {
bool bad_opt(uint8_t o) { return (o & 3u) == 3u || (o & 0xE0u); }
bool bad_msg(uint8_t b) { return gm::so_bad_msg(b); }
std::string shown(const uint8_t* p, uint64_t len) {
  return std::string(reinterpret_cast<const char*>(p), std::min<uint64_t>(len, 200));
}
}  // namespace

int so_compile(const SoInput& in, uint64_t n_filters, const uint64_t* sub_off, const uint32_t* sub_ids,
               const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve, emqx_gm_subopts** out,
               std::string* why) {
  const uint64_t n = in.n_entries;
  const bool skip = in.flags & EMQX_GM_SO_SKIP_UNKNOWN;
  if (in.flags & ~EMQX_GM_SO_SKIP_UNKNOWN) {
    *why = "flags";
    return EMQX_GM_EINVAL;
  }
  if (bad_opt(in.default_opt)) {
    *why = "default_opt " + std::to_string(in.default_opt);
    return EMQX_GM_EINVAL;
  }
  if (const int rc = check_offsets(in.fb, in.fo, n, why)) return rc;
  if (n && (!in.subs || !in.opts)) {
    *why = "NULL buffer";
    return EMQX_GM_EINVAL;
  }
  if (n_filters >= 0xFFFFFFFFull) {
    *why = "a snapshot of 2^32 - 1 filters or more";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (bad_opt(in.opts[i])) {
      *why = "entry " + std::to_string(i) + ": opt byte " + std::to_string(in.opts[i]);
      return EMQX_GM_EINVAL;
    }
  const uint64_t n_subs = sub_off[n_filters];
  // 1. the entries by (filter id, subscriber): a pair given twice is stored once
  struct Ent {
    uint64_t first;  // the input entry that made it
    uint32_t hits;   // positions of the lists it met
    uint8_t opt;
  };
  std::vector<Ent> ents;
  std::unordered_map<uint64_t, uint32_t> at;  // (f << 32 | sub) -> its Ent
  ents.reserve(n);
  at.reserve(n);
  uint64_t skipped = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* p = in.fb + in.fo[i];
    const uint64_t len = in.fo[i + 1] - in.fo[i];
    uint32_t f = 0;
    if (!resolve(p, len, &f) || f >= n_filters) {
      if (skip) {
        ++skipped;
        continue;
      }
      *why = "entry " + std::to_string(i) + ": filter '" + shown(p, len) + "' is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
    const uint64_t key = (uint64_t(f) << 32) | in.subs[i];
    const auto ins = at.emplace(key, uint32_t(ents.size()));
    if (ins.second) {
      ents.push_back(Ent{i, 0, in.opts[i]});
    } else if (ents[ins.first->second].opt != in.opts[i]) {
      *why = "entry " + std::to_string(i) + ": the pair ('" + shown(p, len) + "', " + std::to_string(in.subs[i]) +
             ") is given twice with different bytes";
      return EMQX_GM_EINVAL;
    }
  }
  // 2. one pass over the lists: every pair's byte, and each filter's nl pairs
  std::vector<uint8_t> opt(n_subs);
  std::vector<uint64_t> nl_off(n_filters + 1, 0);
  std::vector<std::pair<uint32_t, uint32_t>> nl;  // (subscriber, position in the segment)
  uint64_t defaulted = 0;
  for (uint64_t f = 0; f < n_filters; ++f) {
    const uint64_t a = sub_off[f], b = sub_off[f + 1], nl0 = nl.size();
    nl_off[f] = nl0;
    if (b - a >= 0xFFFFFFFFull) {
      *why = "a filter of 2^32 - 1 subscribers or more";
      return EMQX_GM_EINVAL;
    }
    for (uint64_t k = a; k < b; ++k) {
      uint8_t o = in.default_opt;
      if (!at.empty()) {
        const auto it = at.find((f << 32) | sub_ids[k]);
        if (it != at.end()) {
          o = ents[it->second].opt;
          ++ents[it->second].hits;
        } else {
          ++defaulted;
        }
      } else {
        ++defaulted;
      }
      opt[k] = o;
      if (o & SO_NL) nl.emplace_back(sub_ids[k], uint32_t(k - a));
    }
    if (nl.size() - nl0 > 1) {
      std::sort(nl.begin() + nl0, nl.end());
      for (uint64_t k = nl0 + 1; k < nl.size(); ++k)
        if (nl[k].first == nl[k - 1].first) {
          *why = "filter id " + std::to_string(f) + " lists subscriber " + std::to_string(nl[k].first) +
                 " twice and the pair has nl = 1";
          return EMQX_GM_EUNSUPPORTED;
        }
    }
  }
  nl_off[n_filters] = nl.size();
  // 3. an entry that met no position: its pair is not in the filter's list
  uint64_t stored = 0;
  for (const Ent& e : ents) {
    if (e.hits) {
      ++stored;
      continue;
    }
    if (skip) {
      ++skipped;
      continue;
    }
    const uint64_t i = e.first;
    *why = "entry " + std::to_string(i) + ": subscriber " + std::to_string(in.subs[i]) + " is not in the list of '" +
           shown(in.fb + in.fo[i], in.fo[i + 1] - in.fo[i]) + "'";
    return EMQX_GM_EINVAL;
  }
  // 4. the arrays: the device part, then the host copy of the lists
  const uint64_t n_nl = nl.size();
  const size_t o_nloff = al16(n_subs + 16);  // (a copy thread reads 4 option bytes at once: room behind the last)
  const size_t o_nlsub = o_nloff + al16((n_filters + 1) * 8);
  const size_t o_nlpos = o_nlsub + al16(n_nl * 4 + 4);
  const size_t dev_bytes = o_nlpos + al16(n_nl * 4 + 4);
  const size_t o_soff = dev_bytes;
  const size_t o_sids = o_soff + al16((n_filters + 1) * 8);
  const size_t total = o_sids + al16(n_subs * 4 + 4);
  auto* so = new emqx_gm_subopts;
  so->blob.resize(total);
  std::memset(so->blob.data(), 0, total);
  so->bytes = dev_bytes;
  uint8_t* B = so->blob.data();
  if (n_subs) std::memcpy(B, opt.data(), n_subs);
  std::memcpy(B + o_nloff, nl_off.data(), (n_filters + 1) * 8);
  auto* nl_sub = reinterpret_cast<uint32_t*>(B + o_nlsub);
  auto* nl_pos = reinterpret_cast<uint32_t*>(B + o_nlpos);
  for (uint64_t k = 0; k < n_nl; ++k) {
    nl_sub[k] = nl[k].first;
    nl_pos[k] = nl[k].second;
  }
  std::memcpy(B + o_soff, sub_off, (n_filters + 1) * 8);
  if (n_subs) std::memcpy(B + o_sids, sub_ids, n_subs * 4);
  so->hv = SoView{reinterpret_cast<const uint64_t*>(B + o_soff),
                  reinterpret_cast<const uint32_t*>(B + o_sids),
                  B,
                  reinterpret_cast<const uint64_t*>(B + o_nloff),
                  nl_sub,
                  nl_pos,
                  n_subs,
                  n_nl,
                  uint32_t(n_filters)};
  for (uint64_t k = 0; k < n_subs; ++k) so->max_sub = std::max(so->max_sub, sub_ids[k]);
  so->dv = so->hv;  // (so_upload rebases the table's pointers and takes the lists from the snapshot)
  so->info.n_entries = stored;
  so->info.n_defaulted = defaulted;
  so->info.n_nl = n_nl;
  so->info.n_skipped_unknown = skipped;
  so->info.device_bytes = 0;
  *out = so;
  return EMQX_GM_OK;
}

int so_check_call(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags, const uint32_t* msg_from,
                  uint32_t mode, std::string* why, bool lead_ok) {
  if (mode != EMQX_GM_SO_FLAG && mode != EMQX_GM_SO_DROP && !(lead_ok && mode == EMQX_GM_SO_LEAD)) {
    *why = "mode";
    return EMQX_GM_EINVAL;
  }
  if (m->n_rows >= 0xFFFFFFFFull) {
    *why = "n_rows of 2^32 - 1 or more";
    return EMQX_GM_EINVAL;
  }
  if (!m->row_off || (m->nnz && !m->ids) || (m->n_rows && (!msg_flags || !msg_from))) {
    *why = "NULL argument";
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
    if (m->ids[j] >= so->hv.n_filters) {
      *why = "filter id " + std::to_string(m->ids[j]) + " is not in the snapshot";
      return EMQX_GM_EINVAL;
    }
  for (uint64_t r = 0; r < m->n_rows; ++r)
    if (bad_msg(msg_flags[r])) {
      *why = "msg_flags[" + std::to_string(r) + "] = " + std::to_string(msg_flags[r]);
      return EMQX_GM_EINVAL;
    }
  return EMQX_GM_OK;
}

// ignore_local's fun and enrich_subopts/3 for every delivery of every row in
// window order: the plain walk, one (filter, subscriber) pair at a time
int so_deliver_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                    const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out) {
  const SoView& v = so->hv;
  const uint64_t n = m->n_rows;
  const bool drop = mode == EMQX_GM_SO_DROP;
  std::vector<uint64_t> ro(n + 1, 0);
  std::vector<uint32_t> ids, dropped(drop ? n : 0, 0);
  std::vector<uint8_t> dopt;
  uint64_t n_dropped = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const uint8_t mf = msg_flags[r];
    const uint32_t from = msg_from[r];
    for (uint64_t j = m->row_off[r]; j < m->row_off[r + 1]; ++j) {
      const uint32_t f = m->ids[j];
      for (uint64_t k = v.sub_off[f]; k < v.sub_off[f + 1]; ++k) {
        const uint32_t s = v.sub_ids[k];
        const uint8_t o = v.opt[k];
        const bool hit = (o & SO_NL) && from != EMQX_GM_SO_NO_PUBLISHER && s == from;
        if (hit && drop) {
          ++dropped[r];
          ++n_dropped;
          continue;
        }
        ids.push_back(s);
        dopt.push_back(uint8_t(so_byte(o, mf) | (hit ? SO_HIT : 0)));
      }
    }
    ro[r + 1] = ids.size();
  }
  if (csr_to_malloc(ro, ids, &out->deliveries)) {
    so_free_malloc(out);
    return EMQX_GM_ENOMEM;
  }
  out->dopt = static_cast<uint8_t*>(malloc(std::max<size_t>(dopt.size(), 1)));
  if (drop) out->row_dropped = static_cast<uint32_t*>(malloc(std::max<uint64_t>(n, 1) * 4));
  if (!out->dopt || (drop && !out->row_dropped)) {
    so_free_malloc(out);
    return EMQX_GM_ENOMEM;
  }
  if (!dopt.empty()) std::memcpy(out->dopt, dopt.data(), dopt.size());
  if (drop && n) std::memcpy(out->row_dropped, dropped.data(), n * 4);
  out->n_dropped = n_dropped;
  out->deliveries.on_device = 0;
  out->deliveries.priv = nullptr;
  return EMQX_GM_OK;
}

}  // namespace gm

extern "C" {

int emqx_gm_subopts_compile_host(const uint8_t* ifb, const uint64_t* ifo, uint64_t n_index, const uint64_t* sub_off,
                                 const uint32_t* sub_ids, const uint8_t* fb, const uint64_t* fo,
                                 const uint32_t* entry_subs, const uint8_t* opts, uint64_t n_entries,
                                 uint8_t default_opt, uint32_t flags, emqx_gm_subopts** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(ifb, ifo, n_index, &why))
    return gm::set_err(nullptr, rc, "subopts_compile_host: index filters: " + why);
  if (!sub_off) return gm::set_err(nullptr, EMQX_GM_EUNSUPPORTED, "subopts_compile_host: an index without subscriber lists");
  if (sub_off[0] != 0) return gm::set_err(nullptr, EMQX_GM_EINVAL, "subopts_compile_host: sub_off");
  for (uint64_t i = 0; i < n_index; ++i)
    if (sub_off[i + 1] < sub_off[i]) return gm::set_err(nullptr, EMQX_GM_EINVAL, "subopts_compile_host: sub_off not ascending");
  if (n_index && sub_off[n_index] && !sub_ids) return gm::set_err(nullptr, EMQX_GM_EINVAL, "subopts_compile_host: sub_ids is NULL");
  // filter ids as emqx_gm_index_compile_host assigns them: the rank among the
  // distinct filters; the lists of a filter given twice concatenated in input order
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
  const uint64_t nf = fs.size();
  std::vector<uint32_t> id_of(n_index);
  std::vector<uint64_t> soff(nf + 1, 0);
  for (uint64_t i = 0; i < n_index; ++i) {
    resolve(ifb + ifo[i], ifo[i + 1] - ifo[i], &id_of[i]);
    soff[id_of[i] + 1] += sub_off[i + 1] - sub_off[i];
  }
  for (uint64_t f = 0; f < nf; ++f) soff[f + 1] += soff[f];
  std::vector<uint32_t> sids(soff[nf]);
  std::vector<uint64_t> cur(soff.begin(), soff.end() - 1);
  for (uint64_t i = 0; i < n_index; ++i) {
    const uint64_t c = sub_off[i + 1] - sub_off[i];
    if (c) std::memcpy(&sids[cur[id_of[i]]], sub_ids + sub_off[i], c * 4);
    cur[id_of[i]] += c;
  }
  const gm::SoInput in{fb, fo, entry_subs, opts, n_entries, default_opt, flags};
  const int rc = gm::so_compile(in, nf, soff.data(), sids.data(), resolve, out, &why);
  return rc ? gm::set_err(nullptr, rc, "subopts_compile_host: " + why) : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_deliver_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                         const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out) {
  if (!so || !m || !out) return EMQX_GM_EINVAL;
  if (m->on_device) return gm::set_err(nullptr, EMQX_GM_EINVAL, "deliver_host: device rows");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::so_check_call(so, m, msg_flags, msg_from, mode, &why))
    return gm::set_err(nullptr, rc, "deliver_host: " + why);
  std::memset(out, 0, sizeof(*out));
  const int rc = gm::so_deliver_host(so, m, msg_flags, msg_from, mode, out);
  return rc ? gm::set_err(nullptr, rc, "deliver_host: result") : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_deliveries_free_host(emqx_gm_deliveries* d) {
  if (!d || d->deliveries.priv || d->deliveries.on_device) return EMQX_GM_EINVAL;
  return gm::so_free_malloc(d);
}

int emqx_gm_subopts_info(const emqx_gm_subopts* so, emqx_gm_subopts_info_t* info) {
  if (!so || !info) return EMQX_GM_EINVAL;
  *info = so->info;
  return EMQX_GM_OK;
}

const emqx_gm_index* emqx_gm_subopts_index(const emqx_gm_subopts* so) { return so ? so->idx : nullptr; }

int emqx_gm_subopts_release(emqx_gm_subopts* so) {
  if (!so) return EMQX_GM_EINVAL;
  if (so->dev_base) gm::so_free_device(so);
  if (so->idx) emqx_gm_index_release(so->idx);
  delete so;
  return EMQX_GM_OK;
}

int emqx_gm_subopts_last_times(const emqx_gm_subopts* so, double* ms3) {
  if (!so || !ms3) return EMQX_GM_EINVAL;
  std::lock_guard<std::mutex> lk(const_cast<emqx_gm_subopts*>(so)->mu);
  for (int k = 0; k < 3; ++k) ms3[k] = so->last_ms[k];
  return EMQX_GM_OK;
}

}  // extern "C"
