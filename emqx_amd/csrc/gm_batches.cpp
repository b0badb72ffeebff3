// gm_batches.cpp — the host walk of the session batches and the host-only part
// of the emqx_gm_deliver_batches* boundary (semantics: gm_batches.h; kernels
// and the device entry points: gm_batches.hip).  The walk is the reference's
// own shape: dispatch the window in order into per-subscriber lists
// (emqx_misc:drain_deliver/1, emqx_misc.erl:159-173), then ignore_local/4 and
// enrich_deliver/2 over each list (emqx_session.erl:279-291, 560-602).
// Plain host C++: it also builds under a sanitizer without a device
// (tests/asan/asan_batches.cpp).
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "gm_batches.h"

namespace gm {

int sb_batches_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                    const uint32_t* msg_from, uint32_t mode, emqx_gm_batches* out) {
  const SoView& v = so->hv;
  const uint64_t n = m->n_rows;
  // 0. the counting pass decides the overflow before anything is sized (as the device path does)
  uint64_t total = 0;
  for (uint64_t j = 0; j < m->nnz; ++j) {
    total += v.sub_off[m->ids[j] + 1] - v.sub_off[m->ids[j]];
    if (total >= 0xFFFFFFFFull) return EMQX_GM_EOVERFLOW;
  }
  // 1. the deliveries in window order: k -> (subscriber, row, filter, FLAG byte)
  std::vector<uint32_t> sub, row, fil;
  std::vector<uint8_t> byte;
  sub.reserve(total), row.reserve(total), fil.reserve(total), byte.reserve(total);
  for (uint64_t r = 0; r < n; ++r) {
    const uint8_t mf = msg_flags[r];
    const uint32_t from = msg_from[r];
    for (uint64_t j = m->row_off[r]; j < m->row_off[r + 1]; ++j) {
      const uint32_t f = m->ids[j];
      for (uint64_t k = v.sub_off[f]; k < v.sub_off[f + 1]; ++k) {
        const uint32_t s = v.sub_ids[k];
        const uint8_t o = v.opt[k];
        const bool hit = (o & SO_NL) && from != EMQX_GM_SO_NO_PUBLISHER && s == from;
        sub.push_back(s);
        row.push_back(uint32_t(r));
        fil.push_back(f);
        byte.push_back(uint8_t(so_byte(o, mf) | (hit ? SO_HIT : 0)));
      }
    }
  }
  // 2. each subscriber's mailbox: a stable grouping by subscriber id
  const uint64_t T = sub.size();
  std::vector<uint32_t> ord(T);
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return sub[a] < sub[b]; });
  // 3. per batch the mode's removal
  std::vector<uint32_t> subs, o_row, o_fil, dropped;
  std::vector<uint64_t> off{0};
  std::vector<uint8_t> o_opt;
  uint64_t n_dropped = 0;
  for (uint64_t a = 0; a < T;) {
    uint64_t b = a;
    while (b < T && sub[ord[b]] == sub[ord[a]]) ++b;
    uint64_t i = a;
    uint32_t gone = 0;
    if (mode == EMQX_GM_SO_LEAD)  // lists:dropwhile: the leading run alone
      while (i < b && (byte[ord[i]] & SO_HIT)) ++i, ++gone;
    for (; i < b; ++i) {
      const uint32_t k = ord[i];
      if (mode == EMQX_GM_SO_DROP && (byte[k] & SO_HIT)) {
        ++gone;
        continue;
      }
      o_row.push_back(row[k]);
      o_fil.push_back(fil[k]);
      o_opt.push_back(mode == EMQX_GM_SO_LEAD ? uint8_t(byte[k] & ~SO_HIT) : byte[k]);
    }
    subs.push_back(sub[ord[a]]);
    off.push_back(o_row.size());
    dropped.push_back(gone);
    n_dropped += gone;
    a = b;
  }
  // 4. the arrays
  const uint64_t nb = subs.size(), kept = o_row.size();
  emqx_gm_batches res{};
  auto take = [](const void* src, size_t bytes) -> void* {
    void* p = malloc(std::max<size_t>(bytes, 1));
    if (p && bytes) std::memcpy(p, src, bytes);
    return p;
  };
  res.subs = static_cast<uint32_t*>(take(subs.data(), nb * 4));
  res.batch_off = static_cast<uint64_t*>(take(off.data(), (nb + 1) * 8));
  res.rows = static_cast<uint32_t*>(take(o_row.data(), kept * 4));
  res.filters = static_cast<uint32_t*>(take(o_fil.data(), kept * 4));
  res.dopt = static_cast<uint8_t*>(take(o_opt.data(), kept));
  if (mode != EMQX_GM_SO_FLAG) res.batch_dropped = static_cast<uint32_t*>(take(dropped.data(), nb * 4));
  if (!res.subs || !res.batch_off || !res.rows || !res.filters || !res.dopt ||
      (mode != EMQX_GM_SO_FLAG && !res.batch_dropped)) {
    sb_free_malloc(&res);
    return EMQX_GM_ENOMEM;
  }
  res.n_rows = n;
  res.n_deliveries = kept;
  res.n_batches = nb;
  res.n_dropped = n_dropped;
  *out = res;  // (the caller's struct is written only on success)
  return EMQX_GM_OK;
}

}  // namespace gm

extern "C" {

int emqx_gm_deliver_batches_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                                 const uint32_t* msg_from, uint32_t mode, emqx_gm_batches* out) {
  if (!so || !m || !out) return EMQX_GM_EINVAL;
  if (m->on_device) return gm::set_err(nullptr, EMQX_GM_EINVAL, "deliver_batches_host: device rows");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::so_check_call(so, m, msg_flags, msg_from, mode, &why, true))
    return gm::set_err(nullptr, rc, "deliver_batches_host: " + why);
  const int rc = gm::sb_batches_host(so, m, msg_flags, msg_from, mode, out);
  return rc ? gm::set_err(nullptr, rc, rc == EMQX_GM_EOVERFLOW ? "deliver_batches_host: 2^32 - 1 deliveries or more"
                                                               : "deliver_batches_host: result")
            : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_batches_free_host(emqx_gm_batches* b) {
  if (!b || b->priv || b->on_device) return EMQX_GM_EINVAL;
  return gm::sb_free_malloc(b);
}

}  // extern "C"
