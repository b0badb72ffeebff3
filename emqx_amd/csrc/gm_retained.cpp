// gm_retained.cpp — host compiler of the retained-topic index, the host walk
// over its tables, and the emqx_gm_retained_* boundary (layout: gm_retained.h;
// kernels: gm_retained.hip).  Replaces the table scan of
// emqx_retainer_mnesia:match_messages/1 + condition/1
// (apps/emqx_retainer/src/emqx_retainer_mnesia.erl:210-244).  Plain host C++:
// every device call is in gm_retained.hip, so this file also builds under a
// sanitizer without a device (tests/asan/asan_retained.cpp).
#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "gm_retained.h"

namespace gm {

namespace {

// the child of `parent` through word id w: a binary search over its contiguous, ascending children
uint32_t host_child(const RetView& v, uint32_t parent, uint32_t w) {
  uint32_t a = v.nodes[parent].child_lo, b = v.nodes[parent + 1].child_lo;
  while (a < b) {
    const uint32_t m = a + (b - a) / 2, x = v.nodes[m].word & RET_WORD_MASK;
    if (x == w) return m;
    if (x < w) a = m + 1;
    else b = m;
  }
  return NONE;
}

void set_views(emqx_gm_retained* r, const size_t* o, uint64_t dict_cap) {
  auto fill = [&](RetView& v, uint8_t* base) {
    v.nodes = reinterpret_cast<const RetNode*>(base + o[0]);
    v.depth_ends = reinterpret_cast<const uint32_t*>(base + o[1]);
    v.words = DictView{reinterpret_cast<const DictSlot*>(base + o[2]), reinterpret_cast<const uint32_t*>(base + o[3]),
                       base + o[4], dict_cap - 1};
    v.ids = reinterpret_cast<const uint32_t*>(base + o[5]);
    v.expiry = reinterpret_cast<uint64_t*>(base + o[6]);
  };
  fill(r->hv, r->blob.data());
  r->dv = r->hv;  // (ret_upload rebases the pointers onto the device allocation)
}

}  // namespace

int ret_compile(const uint8_t* tb, const uint64_t* to, uint64_t n, const uint32_t* ids, const uint64_t* expiry,
                emqx_gm_retained** out, std::string* why) {
  if (const int rc = check_offsets(tb, to, n, why)) return rc;
  // 1. words of every topic (emqx_topic:words/1: split on '/', empty words kept)
  std::vector<uint64_t> wo(n + 1, 0);  // topic -> its first word in `words`
  std::vector<WordRef> words;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* p = tb + to[i];
    const uint64_t len = to[i + 1] - to[i];
    uint64_t s = 0;
    for (uint64_t e = 0; e <= len; ++e)
      if (e == len || p[e] == '/') {
        words.push_back(WordRef{p + s, e - s});
        s = e + 1;
      }
    wo[i + 1] = words.size();
  }
  // 2. word ids = rank among the distinct words (sibling order by id = by bytes)
  std::vector<uint64_t> ord(words.size());
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return word_less(words[a], words[b]); });
  std::vector<uint32_t> wid(words.size());
  std::vector<WordRef> dw;  // distinct words in id order
  for (uint64_t k = 0; k < ord.size(); ++k) {
    if (!k || !word_eq(words[ord[k]], words[ord[k - 1]])) dw.push_back(words[ord[k]]);
    wid[ord[k]] = uint32_t(dw.size() - 1);
  }
  if (dw.size() >= RET_WORD_MASK) {
    *why = "too many distinct words";
    return EMQX_GM_EINVAL;
  }
  std::vector<uint64_t>().swap(ord);
  // 3. topics in word-list order; of equal topics the last input wins
  auto tlen = [&](uint64_t t) { return wo[t + 1] - wo[t]; };
  auto cmp = [&](uint64_t a, uint64_t b) {  // <0, 0, >0
    const uint64_t la = tlen(a), lb = tlen(b), m = std::min(la, lb);
    for (uint64_t k = 0; k < m; ++k) {
      const uint32_t x = wid[wo[a] + k], y = wid[wo[b] + k];
      if (x != y) return x < y ? -1 : 1;
    }
    return la == lb ? 0 : (la < lb ? -1 : 1);
  };
  std::vector<uint64_t> tord(n);
  std::iota(tord.begin(), tord.end(), 0);
  std::sort(tord.begin(), tord.end(), [&](uint64_t a, uint64_t b) {
    const int c = cmp(a, b);
    return c ? c < 0 : a < b;
  });
  std::vector<uint64_t> rank_t;  // rank -> input topic
  for (uint64_t k = 0; k < n; ++k) {
    if (k && cmp(tord[k], tord[k - 1]) == 0) rank_t.back() = tord[k];  // (ascending input position among equals)
    else rank_t.push_back(tord[k]);
  }
  std::vector<uint64_t>().swap(tord);
  const uint64_t nt = rank_t.size();
  // lcp[r]: words topic r shares with topic r - 1
  std::vector<uint32_t> lcp(nt, 0);
  uint64_t depth_max = 0;
  for (uint64_t r = 0; r < nt; ++r) {
    const uint64_t t = rank_t[r], l = tlen(t);
    depth_max = std::max(depth_max, l);
    if (!r) continue;
    const uint64_t q = rank_t[r - 1], m = std::min(l, tlen(q));
    uint64_t k = 0;
    while (k < m && wid[wo[t] + k] == wid[wo[q] + k]) ++k;
    lcp[r] = uint32_t(std::min<uint64_t>(k, 0xFFFFFFFFu));
  }
  if (depth_max >= (1u << 24)) {
    *why = "a topic of 2^24 words or more";
    return EMQX_GM_EINVAL;
  }
  // 4. the levels.  The topics of more than d words, in rank order, shrink from
  // level to level; consecutive ones share their first d+1 words iff they are
  // adjacent ranks with lcp > d (a rank between them is a shallower topic).
  std::vector<RetNode> nodes;
  nodes.push_back(RetNode{0, 0, 0, uint32_t(nt)});  // the root; child_lo patched below
  nodes.push_back(RetNode{0, 0, uint32_t(nt), uint32_t(nt)});
  std::vector<uint32_t> depth_ends(depth_max + 1, 0);
  std::vector<uint32_t> act(nt), next;
  std::iota(act.begin(), act.end(), 0u);
  uint64_t prev_lo = 0, prev_n = 1, widest = 0;  // the level above: its first node and node count
  for (uint64_t d = 0; d < depth_max; ++d) {
    const uint64_t lo = nodes.size();
    next.clear();
    for (uint64_t k = 0; k < act.size(); ++k) {
      const uint32_t r = act[k];
      const uint64_t t = rank_t[r];
      if (!(k && act[k - 1] + 1 == r && lcp[r] > d)) {
        const bool ends = tlen(t) == d + 1;
        if (ends) ++depth_ends[d + 1];
        nodes.push_back(RetNode{wid[wo[t] + d] | (ends ? RET_ENDS : 0u), 0, r, r + 1});
      } else {
        nodes.back().topic_hi = r + 1;
      }
      if (tlen(t) > d + 1) next.push_back(r);
    }
    const uint64_t cnt = nodes.size() - lo;
    widest = std::max(widest, cnt);
    if (nodes.size() + 1 + (depth_max - d) >= 0xFFFFFFFFull) {
      *why = "more than 2^32 trie nodes";
      return EMQX_GM_EINVAL;
    }
    nodes.push_back(RetNode{0, 0, uint32_t(nt), uint32_t(nt)});  // sentinel
    // child_lo of the level above: the first node here at or past the parent's first rank
    uint64_t c = lo;
    for (uint64_t p = prev_lo; p < prev_lo + prev_n; ++p) {
      while (c < lo + cnt && nodes[c].topic_lo < nodes[p].topic_lo) ++c;
      nodes[p].child_lo = uint32_t(c);
    }
    nodes[prev_lo + prev_n].child_lo = uint32_t(lo + cnt);
    prev_lo = lo;
    prev_n = cnt;
    act.swap(next);
  }
  // the deepest level (or the root of an empty table) has no children: an empty level of one sentinel
  {
    const uint32_t end = uint32_t(nodes.size());
    nodes.push_back(RetNode{0, end, uint32_t(nt), uint32_t(nt)});
    for (uint64_t p = prev_lo; p <= prev_lo + prev_n; ++p) nodes[p].child_lo = end;
  }
  // 5. dictionary (open addressing, load <= 1/2), word offsets, arena
  const uint64_t dict_cap = dict_capacity(dw.size());
  uint64_t arena_bytes = 0;
  for (const WordRef& w : dw) arena_bytes += w.len;
  if (arena_bytes >= 0xFFFFFFFFull) {
    *why = "4 GiB of distinct words";
    return EMQX_GM_EINVAL;
  }
  size_t o[8];
  size_t at = 0;
  o[0] = at, at = al16(at + nodes.size() * sizeof(RetNode));
  o[1] = at, at = al16(at + depth_ends.size() * 4);
  o[2] = at, at = al16(at + dict_cap * sizeof(DictSlot));
  o[3] = at, at = al16(at + (dw.size() + 1) * 4);
  o[4] = at, at = al16(at + arena_bytes + 16);
  o[5] = at, at = al16(at + (nt + 1) * 4);
  o[6] = at, at = al16(at + (nt + 1) * 8);
  auto* r = new emqx_gm_retained;
  r->blob.resize(at);
  std::memset(r->blob.data(), 0, at);
  uint8_t* base = r->blob.data();
  std::memcpy(base + o[0], nodes.data(), nodes.size() * sizeof(RetNode));
  std::memcpy(base + o[1], depth_ends.data(), depth_ends.size() * 4);
  dict_fill(dw.data(), dw.size(), reinterpret_cast<DictSlot*>(base + o[2]), dict_cap,
            reinterpret_cast<uint32_t*>(base + o[3]), base + o[4]);
  auto* rid = reinterpret_cast<uint32_t*>(base + o[5]);
  auto* rex = reinterpret_cast<uint64_t*>(base + o[6]);
  bool any_expiry = false;
  for (uint64_t k = 0; k < nt; ++k) {
    rid[k] = ids ? ids[rank_t[k]] : uint32_t(rank_t[k]);
    rex[k] = expiry ? expiry[rank_t[k]] : 0;
    any_expiry |= rex[k] != 0;
  }
  r->bytes = at;
  set_views(r, o, dict_cap);
  for (RetView* v : {&r->hv, &r->dv}) {
    v->n_topics = uint32_t(nt);
    v->n_nodes = uint32_t(nodes.size());
    v->n_words = uint32_t(dw.size());
    v->depth_max = uint32_t(depth_max);
    v->flags = any_expiry ? RET_HAS_EXPIRY : 0u;
  }
  const uint64_t wave_bytes = uint64_t(ret_wave_words(uint32_t(depth_max))) * 4;
  r->info.n_topics = nt;
  r->info.n_nodes = nodes.size();
  r->info.n_words = dw.size();
  r->info.device_bytes = 0;
  r->info.widest_level = widest;
  r->info.depth_max = uint32_t(depth_max);
  r->info.lds_frames = wave_bytes <= RET_LDS_WAVE_BYTES ? 1 : 0;
  r->info.walk_ws_bytes = 0;  // (set per grid by the device side when the frames do not fit LDS)
  *out = r;
  return EMQX_GM_OK;
}

uint32_t ret_find_host(const emqx_gm_retained* r, const uint8_t* p, uint64_t len) {
  const RetView& v = r->hv;
  uint32_t node = 0;
  uint64_t s = 0;
  for (uint64_t e = 0; e <= len; ++e)
    if (e == len || p[e] == '/') {
      const uint32_t w = dict_find_host(v.words, p + s, e - s);
      if (w == NONE) return NONE;
      node = host_child(v, node, w);
      if (node == NONE) return NONE;
      s = e + 1;
    }
  return (v.nodes[node].word & RET_ENDS) ? node : NONE;
}

// The walk of k_ret_walk over the host tables, level by level: the matched
// nodes of a level stay in node order, which is rank order, so a row comes out
// ascending without the kernel's chunked descent (the host has the memory).
void ret_match_host(const emqx_gm_retained* r, const uint8_t* fb, const uint64_t* fo, uint64_t n, uint64_t now,
                    std::vector<uint64_t>& row_off, std::vector<uint32_t>& ids) {
  const RetView& v = r->hv;
  row_off.assign(n + 1, 0);
  ids.clear();
  std::vector<uint32_t> fw;
  std::vector<std::pair<uint32_t, uint32_t>> cur, nxt;  // node ranges [lo, hi)
  const bool expiring = v.flags & RET_HAS_EXPIRY;
  auto emit = [&](uint32_t rank) {
    if (expiring) {
      const uint64_t x = v.expiry[rank];
      if (x != 0 && x <= now) return;
    }
    ids.push_back(v.ids[rank]);
  };
  for (uint64_t f = 0; f < n; ++f) {
    row_off[f] = ids.size();
    const uint8_t* p = fb + fo[f];
    const uint64_t len = fo[f + 1] - fo[f];
    fw.clear();
    bool ok = true, hash = false;
    uint64_t s = 0;
    for (uint64_t e = 0; e <= len && ok; ++e)
      if (e == len || p[e] == '/') {
        const uint64_t wl = e - s;
        if (wl == 1 && p[s] == '+') {
          fw.push_back(RET_PLUS);
        } else if (wl == 1 && p[s] == '#') {
          if (e == len) hash = true;
          else ok = false;  // '#' before the last word: no stored word equals it
        } else {
          const uint32_t w = dict_find_host(v.words, p + s, wl);
          if (w == NONE) ok = false;
          fw.push_back(w);
        }
        s = e + 1;
        if (fw.size() > v.depth_max) ok = false;  // more words before a '#' than any topic has
      }
    if (!ok) continue;
    const uint64_t P = fw.size();
    if (P > v.depth_max || (!hash && v.depth_ends[P] == 0)) continue;
    cur.assign(1, {0u, 1u});
    for (uint64_t d = 0; d < P && !cur.empty(); ++d) {
      nxt.clear();
      for (const auto& it : cur) {
        if (fw[d] == RET_PLUS) {
          const uint32_t a = v.nodes[it.first].child_lo, b = v.nodes[it.second].child_lo;
          if (a < b) nxt.emplace_back(a, b);
        } else {
          for (uint32_t q = it.first; q < it.second; ++q) {
            const uint32_t c = host_child(v, q, fw[d]);
            if (c != NONE) nxt.emplace_back(c, c + 1);
          }
        }
      }
      cur.swap(nxt);
    }
    for (const auto& it : cur)
      for (uint32_t q = it.first; q < it.second; ++q) {
        const RetNode& nd = v.nodes[q];
        if (hash) {
          for (uint32_t k = nd.topic_lo; k < nd.topic_hi; ++k) emit(k);
        } else if (nd.word & RET_ENDS) {
          emit(nd.topic_lo);
        }
      }
  }
  row_off[n] = ids.size();
}

}  // namespace gm

extern "C" {

int emqx_gm_retained_compile_host(const uint8_t* tb, const uint64_t* to, uint64_t n, const uint32_t* ids,
                                  const uint64_t* expiry, emqx_gm_retained** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  std::string why;
  const int rc = gm::ret_compile(tb, to, n, ids, expiry, out, &why);
  return rc ? gm::set_err(nullptr, rc, "retained_build: " + why) : rc;
  GM_GUARD_END(nullptr)
}

int emqx_gm_retained_build(emqx_gm_ctx* ctx, const uint8_t* tb, const uint64_t* to, uint64_t n, const uint32_t* ids,
                           const uint64_t* expiry, uint32_t flags, emqx_gm_retained** out) {
  if (!ctx || !out) return EMQX_GM_EINVAL;
  *out = nullptr;
  if (flags) return gm::set_err(ctx, EMQX_GM_EINVAL, "retained_build: flags");
  GM_GUARD_BEGIN
  std::string why;
  emqx_gm_retained* r = nullptr;
  int rc = gm::ret_compile(tb, to, n, ids, expiry, &r, &why);
  if (rc) return gm::set_err(ctx, rc, "retained_build: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  rc = gm::ret_upload(ctx, r);
  if (rc) {
    delete r;
    return rc;
  }
  *out = r;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_retained_match(emqx_gm_ctx* ctx, const emqx_gm_retained* idx, const uint8_t* fb, const uint64_t* fo,
                           uint64_t n, uint64_t now_ms, uint32_t flags, emqx_gm_csr* out) {
  if (!ctx || !idx || !out) return EMQX_GM_EINVAL;
  std::memset(out, 0, sizeof(*out));
  if (flags & ~EMQX_GM_RET_TIMED) return gm::set_err(ctx, EMQX_GM_EINVAL, "retained_match: flags");
  if (!idx->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "retained_match: a host-only index");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "retained_match: the index is on another device");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(fb, fo, n, &why)) return gm::set_err(ctx, rc, "retained_match: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::ret_match_device(ctx, const_cast<emqx_gm_retained*>(idx), fb, fo, n, now_ms,
                              (flags & EMQX_GM_RET_TIMED) != 0, out);
  GM_GUARD_END(ctx)
}

int emqx_gm_retained_expire(emqx_gm_ctx* ctx, emqx_gm_retained* idx, const uint8_t* tb, const uint64_t* to,
                            uint64_t n, const uint64_t* expiry, uint64_t* n_found) {
  if (!ctx || !idx) return EMQX_GM_EINVAL;
  if (n_found) *n_found = 0;
  if (n && !expiry) return gm::set_err(ctx, EMQX_GM_EINVAL, "retained_expire: NULL expiry");
  if (!idx->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "retained_expire: a host-only index");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "retained_expire: the index is on another device");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(tb, to, n, &why)) return gm::set_err(ctx, rc, "retained_expire: " + why);
  if (!n) return EMQX_GM_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  uint64_t found = 0;
  if (const int rc = gm::ret_expire_device(ctx, idx, tb, to, n, expiry, &found)) return rc;
  // the host copy follows (the host walk of emqx_gm_retained_match_host reads it)
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t node = gm::ret_find_host(idx, tb + to[i], to[i + 1] - to[i]);
    if (node != gm::NONE) idx->hv.expiry[idx->hv.nodes[node].topic_lo] = expiry[i];
  }
  idx->hv.flags |= gm::RET_HAS_EXPIRY;
  idx->dv.flags |= gm::RET_HAS_EXPIRY;
  if (n_found) *n_found = found;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_retained_info(const emqx_gm_retained* idx, emqx_gm_retained_info_t* info) {
  if (!idx || !info) return EMQX_GM_EINVAL;
  *info = idx->info;
  return EMQX_GM_OK;
}

int emqx_gm_retained_release(emqx_gm_retained* idx) {
  if (!idx) return EMQX_GM_EINVAL;
  if (idx->dev_base) gm::ret_free_device(idx);
  delete idx;
  return EMQX_GM_OK;
}

int emqx_gm_retained_match_host(const emqx_gm_retained* idx, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                                uint64_t now_ms, emqx_gm_csr* out) {
  if (!idx || !out) return EMQX_GM_EINVAL;
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::check_offsets(fb, fo, n, &why))
    return gm::set_err(nullptr, rc, "retained_match_host: " + why);
  std::vector<uint64_t> ro;
  std::vector<uint32_t> ids;
  gm::ret_match_host(idx, fb, fo, n, now_ms, ro, ids);
  if (const int rc = gm::csr_to_malloc(ro, ids, out)) {
    gm::csr_free_malloc(out);
    return gm::set_err(nullptr, rc, "retained_match_host: result");
  }
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_retained_csr_free_host(emqx_gm_csr* csr) { return gm::csr_free_malloc(csr); }

int emqx_gm_retained_last_times(const emqx_gm_retained* idx, double* ms3) {
  if (!idx || !ms3) return EMQX_GM_EINVAL;
  for (int k = 0; k < 3; ++k) ms3[k] = idx->last_ms[k];
  return EMQX_GM_OK;
}

}  // extern "C"
