// gm_authz.cpp — host compiler of the authorization table, the host walk over
// its tables, and the emqx_gm_authz_* boundary (layout: gm_authz.h; kernel:
// gm_authz.hip).  Replaces the per-packet rule scans of
// emqx_authz:do_authorize/4 (apps/emqx_authz/src/emqx_authz.erl:307-317):
// emqx_authz_rule:matches/4 (emqx_authz_rule.erl:110-125) for a file source and
// emqx_authz_mnesia:authorize/4 (emqx_authz_mnesia.erl:95-111, 212-218) for the
// built-in database.  Plain host C++: every device call is in gm_authz.hip, so
// this file also builds under a sanitizer without a device
// (tests/asan/asan_authz.cpp).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "gm_authz.h"

namespace gm {

namespace {

// offsets from 0, ascending, entries under 2 GiB (the boundary carries no byte count)
int check_off(const char* name, const uint64_t* o, uint64_t n, const void* bytes, std::string* why) {
  if (!o) {
    *why = std::string(name) + ": NULL offsets";
    return EMQX_GM_EINVAL;
  }
  if (o[0] != 0) {
    *why = std::string(name) + ": offsets do not start at 0";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (o[i + 1] < o[i] || o[i + 1] - o[i] >= (1ull << 31)) {
      *why = std::string(name) + ": offsets not ascending (or an entry of 2 GiB) at " + std::to_string(i);
      return EMQX_GM_EINVAL;
    }
  if (!bytes && o[n]) {
    *why = std::string(name) + ": NULL buffer";
    return EMQX_GM_EINVAL;
  }
  return EMQX_GM_OK;
}

struct WordHash {
  size_t operator()(const WordRef& s) const { return hash_word_host(s.p, s.len); }
};

const char* const kReserved[AZ_RESERVED_WORDS] = {"", "+", "#", "${clientid}", "${username}"};

// the rule range under a key of a keyed segment (empty: no such key)
void host_key_find(const AzView& v, const AzSeg& sg, const uint8_t* p, uint64_t len, uint32_t* lo, uint32_t* hi) {
  *lo = *hi = 0;
  const uint32_t h = dict_hash_host(p, len);
  const uint64_t head = word_head_host(p, len);
  for (uint32_t s = h & sg.key_mask;; s = (s + 1) & sg.key_mask) {
    const AzKeySlot& e = v.keys[sg.key_lo + s];
    if (e.len == DICT_EMPTY_LEN) return;
    if (e.len != len || e.hash != h || e.head != head) continue;
    if (len <= 8 || !std::memcmp(v.words.arena + e.off + 8, p + 8, len - 8)) {
      *lo = e.r_lo, *hi = e.r_hi;
      return;
    }
  }
}

}  // namespace

int az_compile(const emqx_gm_authz_desc* d, emqx_gm_authz** out, std::string* why) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!d) {
    *why = "NULL description";
    return EMQX_GM_EINVAL;
  }
  if (d->n_segments > AZ_MAX_SEGS) {
    *why = "more than 64 segments";
    return EMQX_GM_EINVAL;
  }
  if (d->n_rules >= 0x7FFFFFFFull || d->n_ranges >= 0x7FFFFFFFull || d->n_leaves >= 0x7FFFFFFFull ||
      d->n_filters >= 0x7FFFFFFFull) {
    *why = "2^31 - 1 entries or more";
    return EMQX_GM_EINVAL;
  }
  if (d->n_segments && !d->seg_kind) {
    *why = "NULL seg_kind";
    return EMQX_GM_EINVAL;
  }
  if (d->n_rules && (!d->rule_id || !d->rule_perm || !d->rule_action || !d->rule_who_op)) {
    *why = "NULL rule array";
    return EMQX_GM_EINVAL;
  }
  if ((d->n_leaves && !d->leaf_kind) || (d->n_filters && !d->filter_kind)) {
    *why = "NULL kind array";
    return EMQX_GM_EINVAL;
  }
  // ---- the offset arrays, each closed by the next array's count
  static const uint8_t nothing = 0;
  if (const int rc = check_off("seg_range_off", d->seg_range_off, d->n_segments, &nothing, why)) return rc;
  if (const int rc = check_off("range_rule_off", d->range_rule_off, d->n_ranges, &nothing, why)) return rc;
  if (const int rc = check_off("key_off", d->key_off, d->n_ranges, d->key_bytes, why)) return rc;
  if (const int rc = check_off("rule_who_off", d->rule_who_off, d->n_rules, &nothing, why)) return rc;
  if (const int rc = check_off("rule_filter_off", d->rule_filter_off, d->n_rules, &nothing, why)) return rc;
  if (const int rc = check_off("leaf_off", d->leaf_off, d->n_leaves, d->leaf_bytes, why)) return rc;
  if (const int rc = check_off("filter_off", d->filter_off, d->n_filters, d->filter_bytes, why)) return rc;
  if (d->seg_range_off[d->n_segments] != d->n_ranges || d->range_rule_off[d->n_ranges] != d->n_rules ||
      d->rule_who_off[d->n_rules] != d->n_leaves || d->rule_filter_off[d->n_rules] != d->n_filters) {
    *why = "offsets do not end at the next array's count";
    return EMQX_GM_EINVAL;
  }
  if (d->key_off[d->n_ranges] >= 0xFFFFFFFFull || d->leaf_off[d->n_leaves] >= 0xFFFFFFFFull) {
    *why = "4 GiB of keys or leaf values";
    return EMQX_GM_EINVAL;
  }
  // ---- rules
  std::vector<AzRule> rules(d->n_rules + 1);
  for (uint64_t r = 0; r < d->n_rules; ++r) {
    const uint32_t perm = d->rule_perm[r], act = d->rule_action[r], op = d->rule_who_op[r];
    if (perm != EMQX_GM_AUTHZ_ALLOW && perm != EMQX_GM_AUTHZ_DENY) {
      *why = "a permission outside 1..2 at rule " + std::to_string(r);
      return EMQX_GM_EINVAL;
    }
    if (act < EMQX_GM_AUTHZ_PUBLISH || act > EMQX_GM_AUTHZ_ALL) {
      *why = "an action outside 1..3 at rule " + std::to_string(r);
      return EMQX_GM_EINVAL;
    }
    if (op > 1) {
      *why = "a who operator outside 0..1 at rule " + std::to_string(r);
      return EMQX_GM_EINVAL;
    }
    rules[r] = AzRule{d->rule_id[r], perm | (act << 2) | (op ? AZ_M_OR : 0u), uint32_t(d->rule_who_off[r]),
                      uint32_t(d->rule_filter_off[r])};
  }
  rules[d->n_rules] = AzRule{NONE, 0, uint32_t(d->n_leaves), uint32_t(d->n_filters)};
  // ---- who leaves; their values go behind the words in the arena (offsets patched below)
  std::vector<AzLeaf> leaves(d->n_leaves);
  std::vector<AzCidr> cidrs;
  std::vector<uint8_t> tail;  // key and leaf-value bytes
  for (uint64_t l = 0; l < d->n_leaves; ++l) {
    const uint8_t* p = d->leaf_bytes + d->leaf_off[l];
    const uint64_t len = d->leaf_off[l + 1] - d->leaf_off[l];
    const uint32_t kind = d->leaf_kind[l];
    AzLeaf lf{kind, 0, 0, 0};
    if (kind == EMQX_GM_AUTHZ_WHO_USERNAME || kind == EMQX_GM_AUTHZ_WHO_CLIENTID) {
      lf.a = uint32_t(tail.size());
      lf.b = uint32_t(len);
      tail.insert(tail.end(), p, p + len);
    } else if (kind == EMQX_GM_AUTHZ_WHO_IPADDR) {
      if (len % EMQX_GM_AUTHZ_CIDR_BYTES) {
        *why = "an ipaddr leaf that is no list of 33-byte CIDRs at leaf " + std::to_string(l);
        return EMQX_GM_EINVAL;
      }
      lf.a = uint32_t(cidrs.size());
      lf.b = uint32_t(len / EMQX_GM_AUTHZ_CIDR_BYTES);
      for (uint64_t k = 0; k < lf.b; ++k) {
        const uint8_t* c = p + k * EMQX_GM_AUTHZ_CIDR_BYTES;
        if (c[0] != 4 && c[0] != 6) {
          *why = "a CIDR family that is neither 4 nor 6 at leaf " + std::to_string(l);
          return EMQX_GM_EINVAL;
        }
        AzCidr cd{};
        cd.v6 = c[0] == 6;
        az_peer_words(c + 1, cd.v6, cd.lo);
        az_peer_words(c + 17, cd.v6, cd.hi);
        cidrs.push_back(cd);
      }
    } else if (kind == EMQX_GM_AUTHZ_WHO_REGEX) {
      if (len != 1) {
        *why = "a regex leaf without its one byte at leaf " + std::to_string(l);
        return EMQX_GM_EINVAL;
      }
      if (p[0] >= 32) {
        *why = "more than 32 distinct regexes (bit " + std::to_string(p[0]) + ")";
        return EMQX_GM_EUNSUPPORTED;
      }
      lf.a = p[0];
    } else if (kind == EMQX_GM_AUTHZ_WHO_AND || kind == EMQX_GM_AUTHZ_WHO_OR) {
      *why = "a nested and / or at leaf " + std::to_string(l) + " (the reference's who() allows leaves only)";
      return EMQX_GM_EUNSUPPORTED;
    } else {
      *why = "an unknown leaf kind at leaf " + std::to_string(l);
      return EMQX_GM_EINVAL;
    }
    leaves[l] = lf;
  }
  // ---- filters: words interned in first-seen order behind the reserved ids
  std::unordered_map<WordRef, uint32_t, WordHash> ids;
  std::vector<WordRef> dw;
  for (uint32_t k = 0; k < AZ_RESERVED_WORDS; ++k) {
    const WordRef s{reinterpret_cast<const uint8_t*>(kReserved[k]), std::strlen(kReserved[k])};
    ids.emplace(s, k);
    dw.push_back(s);
  }
  std::vector<AzFilter> filters(d->n_filters);
  std::vector<uint32_t> fwords;
  uint64_t deepest = 0;
  for (uint64_t f = 0; f < d->n_filters; ++f) {
    const uint32_t kind = d->filter_kind[f];
    if (kind != EMQX_GM_AUTHZ_FILTER_PLAIN && kind != EMQX_GM_AUTHZ_FILTER_EQ) {
      *why = "an unknown filter kind at filter " + std::to_string(f);
      return EMQX_GM_EINVAL;
    }
    const uint8_t* p = d->filter_bytes + d->filter_off[f];
    const uint64_t len = d->filter_off[f + 1] - d->filter_off[f];
    const uint64_t w_lo = fwords.size();
    bool pattern = false;
    uint64_t s = 0;
    for (uint64_t e = 0; e <= len; ++e)
      if (e == len || p[e] == '/') {
        const WordRef w{p + s, e - s};
        auto it = ids.find(w);
        if (it == ids.end()) {
          it = ids.emplace(w, uint32_t(dw.size())).first;
          dw.push_back(w);
        }
        pattern |= it->second == AZ_W_PH_CLIENTID || it->second == AZ_W_PH_USERNAME;
        fwords.push_back(it->second);
        s = e + 1;
      }
    const uint64_t n = fwords.size() - w_lo;
    if (n > AZ_F_N_MASK || fwords.size() >= 0xFFFFFFFFull || dw.size() >= 0x7FFFFFFFull) {
      *why = "too many filter words";
      return EMQX_GM_EINVAL;
    }
    deepest = std::max(deepest, n);
    const uint32_t k = kind == EMQX_GM_AUTHZ_FILTER_EQ ? AZ_F_EQ : (pattern ? AZ_F_PATTERN : AZ_F_PLAIN);
    filters[f] = AzFilter{uint32_t(w_lo), uint32_t(n) | (k << 30)};
  }
  uint64_t word_bytes = 0;
  for (const WordRef& w : dw) word_bytes += w.len;
  // ---- segments and key tables
  std::vector<AzSeg> segs(d->n_segments);
  std::vector<AzKeySlot> keys;
  uint64_t n_keys = 0, longest = 0;
  for (uint32_t s = 0; s < d->n_segments; ++s) {
    const uint32_t kind = d->seg_kind[s];
    const uint64_t k0 = d->seg_range_off[s], k1 = d->seg_range_off[s + 1];
    AzSeg sg{};
    sg.kind = kind;
    if (kind == EMQX_GM_AUTHZ_GLOBAL) {
      if (k1 - k0 != 1) {
        *why = "a GLOBAL segment must own exactly one range (segment " + std::to_string(s) + ")";
        return EMQX_GM_EINVAL;
      }
      sg.r_lo = uint32_t(d->range_rule_off[k0]);
      sg.r_hi = uint32_t(d->range_rule_off[k1]);
      longest = std::max<uint64_t>(longest, sg.r_hi - sg.r_lo);
    } else if (kind == EMQX_GM_AUTHZ_BY_CLIENTID || kind == EMQX_GM_AUTHZ_BY_USERNAME) {
      uint64_t cap = 4;
      while (cap < 2 * (k1 - k0)) cap <<= 1;
      if (keys.size() + cap >= 0xFFFFFFFFull) {
        *why = "too many keys";
        return EMQX_GM_EINVAL;
      }
      sg.key_lo = uint32_t(keys.size());
      sg.key_mask = uint32_t(cap - 1);
      keys.resize(keys.size() + cap, AzKeySlot{0, DICT_EMPTY_LEN, 0, 0, 0, 0, 0});
      AzKeySlot* tab = keys.data() + sg.key_lo;
      for (uint64_t k = k0; k < k1; ++k) {
        const uint8_t* p = d->key_bytes + d->key_off[k];
        const uint64_t len = d->key_off[k + 1] - d->key_off[k];
        const uint32_t h = dict_hash_host(p, len);
        const uint64_t head = word_head_host(p, len);
        uint32_t at = h & sg.key_mask;
        for (; tab[at].len != DICT_EMPTY_LEN; at = (at + 1) & sg.key_mask) {
          const AzKeySlot& e = tab[at];
          if (e.len == len && e.hash == h && e.head == head && (!len || !std::memcmp(tail.data() + e.off, p, len))) {
            *why = "a key listed twice in segment " + std::to_string(s);
            return EMQX_GM_EINVAL;
          }
        }
        tab[at] = AzKeySlot{head, uint32_t(len), h, uint32_t(tail.size()), uint32_t(d->range_rule_off[k]),
                            uint32_t(d->range_rule_off[k + 1]), 0};
        tail.insert(tail.end(), p, p + len);
        longest = std::max<uint64_t>(longest, d->range_rule_off[k + 1] - d->range_rule_off[k]);
      }
      n_keys += k1 - k0;
    } else {
      *why = "an unknown segment kind at segment " + std::to_string(s);
      return EMQX_GM_EINVAL;
    }
    segs[s] = sg;
  }
  if (word_bytes + tail.size() >= 0xFFFFFFFFull) {
    *why = "4 GiB of word, key and value bytes";
    return EMQX_GM_EINVAL;
  }
  // ---- the blob
  const uint64_t dict_cap = dict_capacity(dw.size());
  size_t o[10];
  size_t at = 0;
  o[0] = at, at = al32(at + (segs.size() + 1) * sizeof(AzSeg));
  o[1] = at, at = al32(at + rules.size() * sizeof(AzRule));
  o[2] = at, at = al32(at + (leaves.size() + 1) * sizeof(AzLeaf));
  o[3] = at, at = al32(at + (cidrs.size() + 1) * sizeof(AzCidr));
  o[4] = at, at = al32(at + (filters.size() + 1) * sizeof(AzFilter));
  o[5] = at, at = al32(at + (fwords.size() + 1) * 4);
  o[6] = at, at = al32(at + (keys.size() + 1) * sizeof(AzKeySlot));
  o[7] = at, at = al32(at + dict_cap * sizeof(DictSlot));
  o[8] = at, at = al32(at + (dw.size() + 1) * 4);
  o[9] = at, at = al32(at + word_bytes + tail.size() + 16);
  auto* t = new emqx_gm_authz;
  t->blob.resize(at);
  std::memset(t->blob.data(), 0, at);
  uint8_t* base = t->blob.data();
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) std::memcpy(base + off, src, bytes);
  };
  put(o[0], segs.data(), segs.size() * sizeof(AzSeg));
  put(o[1], rules.data(), rules.size() * sizeof(AzRule));
  put(o[3], cidrs.data(), cidrs.size() * sizeof(AzCidr));
  put(o[4], filters.data(), filters.size() * sizeof(AzFilter));
  put(o[5], fwords.data(), fwords.size() * 4);
  // key and leaf-value offsets become arena offsets: the words come first
  for (AzLeaf& lf : leaves)
    if (lf.kind == EMQX_GM_AUTHZ_WHO_USERNAME || lf.kind == EMQX_GM_AUTHZ_WHO_CLIENTID) lf.a += uint32_t(word_bytes);
  for (AzKeySlot& k : keys)
    if (k.len != DICT_EMPTY_LEN) k.off += uint32_t(word_bytes);
  put(o[2], leaves.data(), leaves.size() * sizeof(AzLeaf));
  put(o[6], keys.data(), keys.size() * sizeof(AzKeySlot));
  auto* dict = reinterpret_cast<DictSlot*>(base + o[7]);
  auto* woff = reinterpret_cast<uint32_t*>(base + o[8]);
  uint8_t* arena = base + o[9];
  dict_fill(dw.data(), dw.size(), dict, dict_cap, woff, arena);
  put(o[9] + word_bytes, tail.data(), tail.size());
  t->bytes = at;
  AzView& v = t->hv;
  v.segs = reinterpret_cast<const AzSeg*>(base + o[0]);
  v.rules = reinterpret_cast<const AzRule*>(base + o[1]);
  v.leaves = reinterpret_cast<const AzLeaf*>(base + o[2]);
  v.cidrs = reinterpret_cast<const AzCidr*>(base + o[3]);
  v.filters = reinterpret_cast<const AzFilter*>(base + o[4]);
  v.fwords = reinterpret_cast<const uint32_t*>(base + o[5]);
  v.keys = reinterpret_cast<const AzKeySlot*>(base + o[6]);
  v.words = DictView{dict, woff, arena, dict_cap - 1};
  v.n_segs = d->n_segments;
  v.n_rules = uint32_t(d->n_rules);
  v.n_words = uint32_t(dw.size());
  t->dv = t->hv;  // (az_upload rebases the pointers onto the device allocation)
  t->info.device_bytes = 0;
  t->info.n_rules = d->n_rules;
  t->info.n_keys = n_keys;
  t->info.n_words = dw.size();
  t->info.n_filters = d->n_filters;
  t->info.n_leaves = d->n_leaves;
  t->info.n_segments = d->n_segments;
  t->info.deepest_filter = uint32_t(deepest);
  t->info.longest_range = longest;
  t->info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = t;
  return EMQX_GM_OK;
}

int az_check_batch(const emqx_gm_authz_batch* b, std::string* why) {
  if (!b) {
    *why = "NULL batch";
    return EMQX_GM_EINVAL;
  }
  if (b->n >= 0xFFFFFFFFull) {
    *why = "more than 2^32 - 2 requests";
    return EMQX_GM_EINVAL;
  }
  if (b->n && (!b->flags || !b->peerhost || !b->action || !b->re_mask)) {
    *why = "NULL request array";
    return EMQX_GM_EINVAL;
  }
  const struct {
    const char* name;
    const uint8_t* bytes;
    const uint64_t* off;
  } cols[3] = {{"topic_off", b->topic_bytes, b->topic_off},
               {"clientid_off", b->clientid_bytes, b->clientid_off},
               {"username_off", b->username_bytes, b->username_off}};
  for (const auto& c : cols) {
    if (!c.off) {
      *why = std::string(c.name) + ": NULL offsets";
      return EMQX_GM_EINVAL;
    }
    for (uint64_t i = 0; i < b->n; ++i)
      if (c.off[i + 1] < c.off[i] || c.off[i + 1] - c.off[i] >= (1ull << 31)) {
        *why = std::string(c.name) + ": offsets not ascending (or an entry of 2 GiB) at " + std::to_string(i);
        return EMQX_GM_EINVAL;
      }
    if (!c.bytes && b->n && c.off[b->n] != c.off[0]) {
      *why = std::string(c.name) + ": NULL buffer";
      return EMQX_GM_EINVAL;
    }
  }
  for (uint64_t i = 0; i < b->n; ++i)
    if (b->action[i] != EMQX_GM_AUTHZ_PUBLISH && b->action[i] != EMQX_GM_AUTHZ_SUBSCRIBE) {
      *why = "an action outside 1..2 at request " + std::to_string(i);
      return EMQX_GM_EINVAL;
    }
  return EMQX_GM_OK;
}

namespace {

// One request as the host walk sees it: the topic's word ids at any depth and,
// per level, whether the word equals the client's substituted placeholder word.
struct HostReq {
  std::vector<uint32_t> w;
  std::vector<uint8_t> is_cid, is_un;
  const uint8_t *cid, *un;
  uint64_t cid_len, un_len;
  bool has_cid, has_un, has_peer, v6;
  uint32_t peer[4];
  uint32_t action, re_mask;
};

// emqx_topic:match/2, the list clauses (emqx_topic.erl:74-87) in their order,
// name and filter advancing together; `eq(i)`: do the heads at position i equal
bool host_filter_match(const AzView& v, const HostReq& q, const AzFilter& f) {
  const uint32_t n = f.n_kind & AZ_F_N_MASK, kind = f.n_kind >> 30;
  const uint32_t* fw = v.fwords + f.w_lo;
  const size_t L = q.w.size();
  auto eq = [&](uint32_t i) {
    if (kind == AZ_F_PATTERN && fw[i] == AZ_W_PH_CLIENTID) return q.is_cid[i] != 0;
    if (kind == AZ_F_PATTERN && fw[i] == AZ_W_PH_USERNAME) return q.is_un[i] != 0;
    return q.w[i] == fw[i];
  };
  if (kind == AZ_F_EQ) {  // match_topic/2, first clause: Topic =:= TopicFilter
    if (L != n) return false;
    for (uint32_t i = 0; i < n; ++i)
      if (q.w[i] != fw[i]) return false;
    return true;
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (i < L && (eq(i) || fw[i] == AZ_W_PLUS)) continue;  // [H|T1],[H|T2] and [_|T1],['+'|T2]
    return i == n - 1 && fw[i] == AZ_W_HASH;               // _, ['#']; every other clause is false
  }
  return L == n;  // [],[] against [_|_],[]
}

bool host_rule_match(const AzView& v, const HostReq& q, uint32_t r) {
  const AzRule &ru = v.rules[r], &nx = v.rules[r + 1];
  if (!((ru.meta >> 2) & 3u & q.action)) return false;  // match_action/2
  const bool is_or = ru.meta & AZ_M_OR;
  bool acc = !is_or;  // the foldl identities: AND [] is true, OR [] is false
  for (uint32_t l = ru.who_lo; l < nx.who_lo; ++l) {
    const AzLeaf& lf = v.leaves[l];
    bool m = false;
    if (lf.kind == EMQX_GM_AUTHZ_WHO_USERNAME)
      m = q.has_un && q.un_len == lf.b && (!lf.b || !std::memcmp(q.un, v.words.arena + lf.a, lf.b));
    else if (lf.kind == EMQX_GM_AUTHZ_WHO_CLIENTID)
      m = q.has_cid && q.cid_len == lf.b && (!lf.b || !std::memcmp(q.cid, v.words.arena + lf.a, lf.b));
    else if (lf.kind == EMQX_GM_AUTHZ_WHO_IPADDR) {
      for (uint32_t c = 0; c < lf.b && !m && q.has_peer; ++c) m = az_cidr_match(v.cidrs[lf.a + c], q.peer, q.v6);
    } else
      m = (q.re_mask >> lf.a) & 1u;
    acc = is_or ? (acc || m) : (acc && m);
  }
  if (!acc) return false;
  for (uint32_t f = ru.filt_lo; f < nx.filt_lo; ++f)
    if (host_filter_match(v, q, v.filters[f])) return true;
  return false;
}

}  // namespace

void az_check_host(const emqx_gm_authz* t, const emqx_gm_authz_batch* b, uint8_t* verdict, uint32_t* rule) {
  const AzView& v = t->hv;
  HostReq q;
  for (uint64_t i = 0; i < b->n; ++i) {
    const uint8_t fl = b->flags[i];
    q.has_cid = fl & EMQX_GM_AUTHZ_F_CLIENTID;
    q.has_un = fl & EMQX_GM_AUTHZ_F_USERNAME;
    q.has_peer = fl & EMQX_GM_AUTHZ_F_PEERHOST;
    q.v6 = fl & EMQX_GM_AUTHZ_F_IPV6;
    q.cid = b->clientid_bytes ? b->clientid_bytes + b->clientid_off[i] : nullptr;
    q.cid_len = b->clientid_off[i + 1] - b->clientid_off[i];
    q.un = b->username_bytes ? b->username_bytes + b->username_off[i] : nullptr;
    q.un_len = b->username_off[i + 1] - b->username_off[i];
    az_peer_words(b->peerhost + 16 * i, q.v6, q.peer);
    q.action = b->action[i];
    q.re_mask = b->re_mask[i];
    const uint8_t* p = b->topic_bytes ? b->topic_bytes + b->topic_off[i] : nullptr;
    const uint64_t len = b->topic_off[i + 1] - b->topic_off[i];
    q.w.clear(), q.is_cid.clear(), q.is_un.clear();
    uint64_t s = 0;
    for (uint64_t e = 0; e <= len; ++e)
      if (e == len || p[e] == '/') {
        const uint64_t wl = e - s;
        const uint32_t id = dict_find_host(v.words, p + s, wl);
        q.w.push_back(id);
        // feed_var/3: the value as one binary word, or the placeholder's own text when undefined
        const bool bin = az_is_binary_word(p + s, uint32_t(std::min<uint64_t>(wl, 0x7FFFFFFF)));
        q.is_cid.push_back(q.has_cid ? (bin && wl == q.cid_len && !std::memcmp(p + s, q.cid, wl))
                                     : id == AZ_W_PH_CLIENTID);
        q.is_un.push_back(q.has_un ? (bin && wl == q.un_len && !std::memcmp(p + s, q.un, wl))
                                   : id == AZ_W_PH_USERNAME);
        s = e + 1;
      }
    uint8_t vd = EMQX_GM_AUTHZ_NOMATCH;
    uint32_t rid = EMQX_GM_AUTHZ_NO_RULE;
    for (uint32_t sgi = 0; sgi < v.n_segs && !vd; ++sgi) {
      const AzSeg& sg = v.segs[sgi];
      uint32_t lo = sg.r_lo, hi = sg.r_hi;
      if (sg.kind == EMQX_GM_AUTHZ_BY_CLIENTID) {
        lo = hi = 0;
        if (q.has_cid) host_key_find(v, sg, q.cid, q.cid_len, &lo, &hi);
      } else if (sg.kind == EMQX_GM_AUTHZ_BY_USERNAME) {
        lo = hi = 0;
        if (q.has_un) host_key_find(v, sg, q.un, q.un_len, &lo, &hi);
      }
      for (uint32_t r = lo; r < hi; ++r)
        if (host_rule_match(v, q, r)) {
          vd = uint8_t(v.rules[r].meta & 3u);
          rid = v.rules[r].id;
          break;
        }
    }
    verdict[i] = vd;
    rule[i] = rid;
  }
}

}  // namespace gm

extern "C" {

int emqx_gm_authz_compile_host(const emqx_gm_authz_desc* desc, emqx_gm_authz** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  std::string why;
  const int rc = gm::az_compile(desc, out, &why);
  return rc ? gm::set_err(nullptr, rc, "authz_build: " + why) : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_authz_build(emqx_gm_ctx* ctx, const emqx_gm_authz_desc* desc, uint32_t flags, emqx_gm_authz** out) {
  if (!ctx || !out) return EMQX_GM_EINVAL;
  *out = nullptr;
  if (flags) return gm::set_err(ctx, EMQX_GM_EINVAL, "authz_build: flags");
  GM_GUARD_BEGIN
  const auto t0 = std::chrono::steady_clock::now();
  std::string why;
  emqx_gm_authz* t = nullptr;
  int rc = gm::az_compile(desc, &t, &why);
  if (rc) return gm::set_err(ctx, rc, "authz_build: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  rc = gm::az_upload(ctx, t);
  if (rc) {
    delete t;
    return rc;
  }
  t->info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = t;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_authz_check(emqx_gm_ctx* ctx, const emqx_gm_authz* tab, const emqx_gm_authz_batch* batch, uint32_t flags,
                        uint8_t* verdict, uint32_t* rule) {
  if (!ctx || !tab || !batch) return EMQX_GM_EINVAL;
  if (flags & ~EMQX_GM_AUTHZ_TIMED) return gm::set_err(ctx, EMQX_GM_EINVAL, "authz_check: flags");
  if (!tab->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "authz_check: a host-only table");
  if (tab->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "authz_check: the table is on another device");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::az_check_batch(batch, &why)) return gm::set_err(ctx, rc, "authz_check: " + why);
  if (!batch->n) return EMQX_GM_OK;
  if (!verdict || !rule) return gm::set_err(ctx, EMQX_GM_EINVAL, "authz_check: NULL result");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::az_check_device(ctx, const_cast<emqx_gm_authz*>(tab), batch, (flags & EMQX_GM_AUTHZ_TIMED) != 0, verdict,
                             rule);
  GM_GUARD_END(ctx)
}

int emqx_gm_authz_check_host(const emqx_gm_authz* tab, const emqx_gm_authz_batch* batch, uint8_t* verdict,
                             uint32_t* rule) {
  if (!tab || !batch) return EMQX_GM_EINVAL;
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::az_check_batch(batch, &why)) return gm::set_err(nullptr, rc, "authz_check_host: " + why);
  if (!batch->n) return EMQX_GM_OK;
  if (!verdict || !rule) return gm::set_err(nullptr, EMQX_GM_EINVAL, "authz_check_host: NULL result");
  gm::az_check_host(tab, batch, verdict, rule);
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_authz_info(const emqx_gm_authz* tab, emqx_gm_authz_info_t* info) {
  if (!tab || !info) return EMQX_GM_EINVAL;
  *info = tab->info;
  return EMQX_GM_OK;
}

int emqx_gm_authz_release(emqx_gm_authz* tab) {
  if (!tab) return EMQX_GM_EINVAL;
  if (tab->dev_base) gm::az_free_device(tab);
  delete tab;
  return EMQX_GM_OK;
}

int emqx_gm_authz_last_kernel_ms(const emqx_gm_authz* tab, double* ms) {
  if (!tab || !ms) return EMQX_GM_EINVAL;
  *ms = tab->last_kernel_ms;
  return EMQX_GM_OK;
}

}  // extern "C"
