// gm_shard.cpp — a prefix-sharded index behind the C ABI (emqx_gm_index_build_sharded):
// SURVEY.md §8e C5's sharded form for a filter set too large for one GPU,
// reachable from ONE multi-device context -- the NIF's form -- instead of
// only from Python over torch.distributed (emqx_amd/sharded.py).
//
// The reference keeps one routing table per node and has no sharded trie
// (apps/emqx/src/emqx_router.erl:75-84); what makes sharding exact here is
// emqx_topic:match/2 (apps/emqx/src/emqx_topic.erl:65-87): a topic can only
// match filters whose first word is its own first word, '+' or '#'.  So
// emqx_gm_prefix_plan (gm_route.hip) partitions the filters by first word (a
// hot first word by its first two) over the context's devices, puts the
// filters beginning with '+' / '#' on every device, and routes each topic to
// the ONE device that holds every filter it can match:
//   build   the shards compiled at once (one host thread and one device each),
//           each with the global ids of its filters (rows come out in global
//           order: a shard's local order is the global one);
//   match   host buffers: every topic routed (all threads), each device's
//           topics gathered into a batch of its own, matched there (the
//           host-buffer pipeline of gm_host.cpp, all devices at once), and every
//           row put back at its topic's place in ONE result CSR -- nothing is
//           merged: a row comes from one shard whole;
//   fan-out host rows: each row goes to the shard of its filters (all on the
//           row's topic's shard, or on every shard), its global ids mapped to
//           that shard's local ones, fanned out there, and put back in order.
//   update  (an index built without subscriber lists) the route of a snapshot
//           line is fixed: a new filter goes to the shard its matching topics
//           are routed to (route_filter_shard), a shard with local changes is
//           patched in place like a plain index, and EVERY shard gets a new
//           local-to-global id map from one device pass (k_gmap_shift) -- a
//           global id shifts on every shard when any filter is added; a shard
//           that cannot be patched is rebuilt alone (update_sharded).
// Images, device-buffer calls, emqx_gm_index_update_subs and updates of a
// sharded index built with subscriber lists are refused
// (EMQX_GM_EUNSUPPORTED): such a set is rebuilt.
#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <set>
#include <string>
#include <thread>

#include "gm_internal.h"

namespace gm {

namespace {

unsigned host_threads() { return std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// f(a, b) over [0, n) in up to host_threads() ranges at once
template <class F> void parallel_ranges(uint64_t n, uint64_t min_per, F f) {
  const unsigned T = n < 2 * min_per ? 1u : unsigned(std::min<uint64_t>(host_threads(), n / min_per));
  std::vector<std::thread> th;
  for (unsigned r = 1; r < T; ++r) th.emplace_back([&, r] { f(n * r / T, n * (r + 1) / T); });
  f(0, n / T);
  for (auto& t : th) t.join();
}

// emqx_topic:wildcard/1 on the filter bytes
bool is_wild(const uint8_t* p, uint64_t len) {
  uint64_t ws = 0;
  for (uint64_t i = 0; i <= len; ++i) {
    if (i < len && p[i] != '/') continue;
    if (i - ws == 1 && (p[ws] == '+' || p[ws] == '#')) return true;
    ws = i + 1;
  }
  return false;
}

std::vector<emqx_gm_ctx*> devices_of(emqx_gm_ctx* ctx) {
  std::vector<emqx_gm_ctx*> mem{ctx};
  for (emqx_gm_ctx* m : ctx->members) mem.push_back(m);
  return mem;
}

// a device's lock while its shard works (the first device's is the caller's)
struct MemberLock {
  std::unique_lock<std::recursive_mutex> lk;
  explicit MemberLock(emqx_gm_ctx* c) : lk(c->mu, std::defer_lock) {
    if (c->parent) lk.lock();
    hipSetDevice(c->device);
  }
};

}  // namespace

int build_sharded(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n, const uint64_t* sub_off,
                  const uint32_t* sub_ids, uint32_t* perm_out, emqx_gm_index** out) {
  if (!out) return set_err(ctx, EMQX_GM_EINVAL, "index_build_sharded: out is NULL");
  if (n && (!fb || !fo)) return set_err(ctx, EMQX_GM_EINVAL, "index_build_sharded: NULL filter buffers");
  if (n >= 0x7FFFFFFFull) return set_err(ctx, EMQX_GM_EINVAL, "index_build_sharded: too many filters");
  if (sub_off && !sub_ids && n && sub_off[n] > 0)
    return set_err(ctx, EMQX_GM_EINVAL, "index_build_sharded: sub_ids is NULL");
  for (uint64_t i = 0; i < n; ++i)
    if (fo[i + 1] < fo[i] || (sub_off && sub_off[i + 1] < sub_off[i]))
      return set_err(ctx, EMQX_GM_EINVAL, "index_build_sharded: offsets not monotone");
  const std::vector<emqx_gm_ctx*> mem = devices_of(ctx);
  const int K = int(mem.size());
  // ---- global ids: the rank of each unique filter (what an unsharded build assigns)
  std::vector<uint32_t> ord(n);
  std::iota(ord.begin(), ord.end(), 0u);
  sort_filters(ord, fb, fo);
  std::vector<uint32_t> gid(n);
  auto sf = std::make_shared<SortedFilters>();  // (off starts as {0})
  for (uint64_t k = 0; k < n; ++k) {
    const uint32_t i = ord[k];
    const uint64_t li = fo[i + 1] - fo[i];
    bool dup = false;
    if (k) {
      const uint32_t p = ord[k - 1];
      dup = fo[p + 1] - fo[p] == li && std::memcmp(fb + fo[p], fb + fo[i], li) == 0;
    }
    if (!dup) {
      sf->bytes.insert(sf->bytes.end(), fb + fo[i], fb + fo[i] + li);
      sf->off.push_back(sf->bytes.size());
    }
    gid[i] = uint32_t(sf->off.size() - 2);
  }
  const uint64_t nf = sf->off.size() - 1;
  std::vector<uint32_t>().swap(ord);
  if (perm_out)
    for (uint64_t i = 0; i < n; ++i) perm_out[i] = gid[i];
  // ---- the plan: each filter's device (EMQX_GM_ALL_SHARDS: every one)
  std::vector<uint32_t> shard(n ? n : 1);
  emqx_gm_route* route = nullptr;
  if (const int rc = route_plan(fb, fo, n, uint32_t(K), shard.data(), &route)) return set_err(ctx, rc, "index_build_sharded: prefix plan");
  std::unique_ptr<emqx_gm_index> idx(new emqx_gm_index);
  idx->device = ctx->device;
  idx->route = route;
  idx->fshard.assign(nf, 0);
  for (uint64_t i = 0; i < n; ++i) idx->fshard[gid[i]] = shard[i];
  // ---- the shards, compiled and placed at once (each its own host thread and device)
  idx->shards.assign(K, nullptr);
  const int rc = run_all(K, [&](int k) -> int {
    MemberLock lk(mem[k]);
    std::vector<uint8_t> b;
    std::vector<uint64_t> o{0}, so{0};
    std::vector<uint32_t> g, si;
    for (uint64_t i = 0; i < n; ++i) {
      if (shard[i] != uint32_t(k) && shard[i] != EMQX_GM_ALL_SHARDS) continue;
      b.insert(b.end(), fb + fo[i], fb + fo[i + 1]);
      o.push_back(b.size());
      g.push_back(gid[i]);
      if (sub_off) {
        si.insert(si.end(), sub_ids + sub_off[i], sub_ids + sub_off[i + 1]);
        so.push_back(si.size());
      }
    }
    b.resize(b.size() + 64, 0);
    if (si.empty()) si.push_back(0);
    std::vector<uint32_t> perm(g.size() + 1);
    return build_index(mem[k], b.data(), o.data(), g.size(), sub_off ? so.data() : nullptr, sub_off ? si.data() : nullptr,
                       perm.data(), &idx->shards[k], nullptr, g.empty() ? nullptr : g.data(), true);
  });
  hipSetDevice(ctx->device);
  if (rc) {
    free_index(idx.release());
    return rc;
  }
  // ---- the host side: the global filter table and counts
  idx->ft.set_base(sf);
  emqx_gm_index_info_t& in = idx->info;
  in.n_filters = nf;
  for (uint64_t f = 0; f < nf; ++f) in.n_wildcard += is_wild(sf->bytes.data() + sf->off[f], sf->off[f + 1] - sf->off[f]);
  in.trie_empty = in.n_wildcard == 0;
  for (emqx_gm_index* s : idx->shards) {
    in.n_nodes += s->info.n_nodes;
    in.n_edges += s->info.n_edges;
    in.n_words = std::max(in.n_words, s->info.n_words);
    in.device_bytes += s->info.device_bytes;
    in.max_depth = std::max(in.max_depth, s->info.max_depth);
  }
  if (sub_off) {  // per global id: its subscribers (duplicates' lists concatenated), as a build counts them
    std::vector<uint64_t> so(nf + 1, 0);
    for (uint64_t i = 0; i < n; ++i) so[gid[i] + 1] += sub_off[i + 1] - sub_off[i];
    for (uint64_t f = 0; f < nf; ++f) so[f + 1] += so[f];
    in.n_subs = so[nf];
    idx->subs = SubTable(std::move(so), {});
  }
  *out = idx.release();
  return EMQX_GM_OK;
}

// ---------------------------------------------------------------------------
// emqx_gm_index_update on a sharded index (built without subscriber lists).
// The reference applies a route delta on every node to its own tables in a
// constant number of key writes (apps/emqx/src/emqx_router_utils.erl:33-38,
// 74-125, emqx_trie.erl:107-136); here every shard applies its share of the
// delta at once (one host thread and one device each):
//   host plan  O(delta log n): the ops folded against the global filter table,
//              the global id shift G, each op's shard under the fixed route;
//   per shard  PATCH   local changes that fit: patch_update on the shard (its
//                      mirror) + its new id map in the same device step;
//              SHIFT   no local change: the previous shard's tables shared
//                      (blob_owner), a new id map only;
//              REBUILD no room / delta past max(4096, n_local / 8) / a '#'
//                      before a new filter's last word / the mirror moved on:
//                      build_index of this shard's updated filters alone;
//   host side  one merge pass per shard over its u32 id map (its own thread),
//              one over the top-level fshard (a thread of its own): 4 B read
//              and written per filter; no filter bytes of unchanged filters
//              are walked.
// The balance of the shards drifts with the updates until a rebuild re-plans.
// ---------------------------------------------------------------------------
namespace {
thread_local std::vector<uint32_t> tl_shard_kinds;

struct ShardPlan {
  std::set<uint32_t> tomb;        // local ids deleted
  std::set<std::string> dset;     // filters gained
  std::vector<uint32_t> add_gid;  // ... their final global ids (byte order)
  bool well_formed = true;
};

// The shard's id map after the update: survivors G(old id), merged with the
// new filters' ids.  G's shift is constant between two of its list entries, so
// the old map is cut where the shift or the kept set changes (O(delta log n)
// searches) and every piece is copied with one constant added: a streaming
// pass over the u32 map, no search per element.
std::vector<uint32_t> next_gmap(const std::vector<uint32_t>& old, const ShardPlan& p, const IdShift& G) {
  const uint64_t nl = old.size();
  auto pos = [&](uint64_t g) { return uint64_t(std::lower_bound(old.begin(), old.end(), g) - old.begin()); };
  std::vector<uint64_t> cut{0, nl};
  for (uint64_t d : G.dels) cut.push_back(pos(d + 1));  // ids past d lose one more
  for (uint64_t a : G.addpos) cut.push_back(pos(a));    // ids from a on gain one more (a local insert lands here)
  for (uint32_t t : p.tomb) {
    cut.push_back(t);
    cut.push_back(uint64_t(t) + 1);
  }
  std::sort(cut.begin(), cut.end());
  cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
  std::vector<uint32_t> ng(nl - p.tomb.size() + p.add_gid.size());
  uint64_t w = 0;
  size_t ai = 0;
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const uint64_t b = cut[k], e = cut[k + 1];
    if (p.tomb.count(uint32_t(b))) continue;  // (a deleted filter is a piece of its own)
    const uint32_t g = old[b];
    const int64_t c = int64_t(std::upper_bound(G.addpos.begin(), G.addpos.end(), uint64_t(g)) - G.addpos.begin()) -
                      int64_t(std::lower_bound(G.dels.begin(), G.dels.end(), uint64_t(g)) - G.dels.begin());
    while (ai < p.add_gid.size() && int64_t(p.add_gid[ai]) < int64_t(g) + c) ng[w++] = p.add_gid[ai++];
    const uint32_t* src = old.data() + b;
    uint32_t* dst = ng.data() + w;
    const uint32_t cc = uint32_t(c);  // (mod 2^32: the sum is exact)
    for (uint64_t t = 0; t < e - b; ++t) dst[t] = src[t] + cc;
    w += e - b;
  }
  while (ai < p.add_gid.size()) ng[w++] = p.add_gid[ai++];
  return ng;
}
}  // namespace

const std::vector<uint32_t>& last_shard_kinds() { return tl_shard_kinds; }

int update_sharded(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo, const uint8_t* ops,
                   uint64_t n_ops, emqx_gm_index** out) {
  tl_shard_kinds.clear();
  if (!prev || !out) return set_err(ctx, EMQX_GM_EINVAL, "index_update: NULL argument");
  if (n_ops && (!fb || !fo || !ops)) return set_err(ctx, EMQX_GM_EINVAL, "index_update: NULL op buffers");
  if (!prev->subs.empty())
    return set_err(ctx, EMQX_GM_EUNSUPPORTED, "index_update: sharded index with subscriber lists (rebuild it)");
  const std::vector<emqx_gm_ctx*> mem = devices_of(ctx);
  const int K = int(prev->shards.size());
  if (K > int(mem.size()) || route_n_shards(prev->route) != uint32_t(K))
    return set_err(ctx, EMQX_GM_EINVAL, "index_update: a sharded index of another context");
  tl_ustats.replica_mode = EMQX_GM_REP_SHARDED;
  tl_ustats.replicas = uint32_t(K - 1);
  // ---- the ops folded against the global filter table (update_index's rules)
  std::set<uint32_t> tomb;
  std::set<std::string> dset;
  for (uint64_t i = 0; i < n_ops; ++i) {
    if (fo[i + 1] < fo[i]) return set_err(ctx, EMQX_GM_EINVAL, "index_update: offsets not monotone");
    const uint8_t* f = fb + fo[i];
    const uint64_t len = fo[i + 1] - fo[i];
    if (len >= (1ull << 31)) return set_err(ctx, EMQX_GM_EINVAL, "index_update: filter too long");
    bool found;
    const uint64_t b = prev->ft.rank_of(f, len, &found);
    if (ops[i]) {  // insert (idempotent)
      if (found) tomb.erase(uint32_t(b));
      else dset.emplace(reinterpret_cast<const char*>(f), len);
    } else {  // delete (only if present)
      if (found) tomb.insert(uint32_t(b));
      else dset.erase(std::string(reinterpret_cast<const char*>(f), len));
    }
  }
  if (tomb.empty() && dset.empty()) {
    prev->refs.fetch_add(1);
    *out = prev;
    tl_ustats.kind = EMQX_GM_UPD_NONE;
    return EMQX_GM_OK;
  }
  // ---- the global id shift and each new filter's final id and shard
  const uint64_t nb = prev->info.n_filters, na = dset.size();
  if (nb + na >= 0x7FFFFFFFull) return set_err(ctx, EMQX_GM_EINVAL, "index_update: too many filters");
  IdShift G;
  G.nb = nb;
  G.dels.assign(tomb.begin(), tomb.end());
  G.addpos.reserve(na);
  uint64_t twild = 0, dwild = 0;
  for (const std::string& d : dset) {
    bool found;
    G.addpos.push_back(prev->ft.rank_of(reinterpret_cast<const uint8_t*>(d.data()), d.size(), &found));
    dwild += is_wild(reinterpret_cast<const uint8_t*>(d.data()), d.size());
  }
  std::vector<ShardPlan> P(K);
  auto each_shard = [&](uint32_t s, auto f) -> bool {
    if (s == EMQX_GM_ALL_SHARDS) {
      for (int k = 0; k < K; ++k) f(k);
      return true;
    }
    if (s >= uint32_t(K)) return false;
    f(int(s));
    return true;
  };
  bool ok = true, stray = false;  // stray: a deleted filter missing from its shard's id map
  for (uint32_t g : tomb) {
    uint64_t l;
    const uint8_t* p = prev->ft.at(g, &l);
    twild += is_wild(p, l);
    ok = ok && each_shard(prev->fshard[g], [&](int k) {
      const std::vector<uint32_t>& gm = prev->shards[k]->gmap;
      auto it = std::lower_bound(gm.begin(), gm.end(), g);
      if (it == gm.end() || *it != g) stray = true;
      else P[k].tomb.insert(uint32_t(it - gm.begin()));
    });
  }
  std::vector<uint32_t> add_shard(na);
  {
    uint64_t j = 0;
    for (const std::string& d : dset) {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(d.data());
      const uint32_t gid = G.map(nb + j), s = route_filter_shard(prev->route, p, d.size());
      const bool wf = well_formed_filter(p, d.size());
      add_shard[j++] = s;
      ok = ok && each_shard(s, [&](int k) {
        P[k].dset.insert(d);
        P[k].add_gid.push_back(gid);
        P[k].well_formed = P[k].well_formed && wf;
      });
    }
  }
  if (!ok || stray) return set_err(ctx, EMQX_GM_EINVAL, "index_update: the sharded index's shard tables disagree");
  // ---- the top-level filter -> shard table, merged on a thread of its own
  const uint64_t nf_new = nb - tomb.size() + na;
  std::vector<uint32_t> nfshard;
  std::thread fshard_thread([&] {  // (pieces between two changes copied whole)
    nfshard.resize(nf_new);
    const uint32_t* src = prev->fshard.data();
    uint32_t* dst = nfshard.data();
    uint64_t g = 0, w = 0, d = 0, a = 0;
    const uint64_t nd = G.dels.size();
    auto copy_to = [&](uint64_t end) {
      if (end > g) std::memcpy(dst + w, src + g, (end - g) * 4);
      w += end - g;
      g = end;
    };
    while (d < nd || a < na) {
      copy_to(std::min(d < nd ? G.dels[d] : nb, a < na ? G.addpos[a] : nb));
      while (a < na && G.addpos[a] == g) dst[w++] = add_shard[a++];
      if (d < nd && G.dels[d] == g) {
        ++d;
        ++g;
      }
    }
    copy_to(nb);
  });
  struct Joiner {
    std::thread& t;
    ~Joiner() {
      if (t.joinable()) t.join();
    }
  } fshard_join{fshard_thread};
  // ---- every shard at once: patch, shift or rebuild
  std::vector<emqx_gm_index*> ns(K, nullptr);
  std::vector<uint32_t> kinds(K, EMQX_GM_UPD_SHIFT);
  std::vector<emqx_gm_update_stats> st(K);
  auto shard_step = [&](int k) -> int {
    emqx_gm_ctx* c = mem[k];
    emqx_gm_index* s = prev->shards[k];
    const ShardPlan& p = P[k];
    const uint64_t nl = s->info.n_filters, delta = p.tomb.size() + p.dset.size();
    std::vector<uint32_t> ng = next_gmap(s->gmap, p, G);
    emqx_gm_index* o = nullptr;
    if (!delta) {
      // no local change: the previous shard's tables shared, a new id map only
      o = new emqx_gm_index;
      o->device = s->device;
      emqx_gm_index* owner = s->blob_owner ? s->blob_owner : s;
      owner->refs.fetch_add(1);
      o->blob_owner = owner;
      o->dev_base = s->dev_base;
      o->dev_bytes = s->dev_bytes;
      o->view = s->view;
      o->dev_flen = s->dev_flen;
      o->flen_stale = s->flen_stale.load();
      o->ft = s->ft;
      o->level_nodes = s->level_nodes;
      o->info = s->info;
      {  // the mirror follows the newest snapshot of the shard's line
        std::lock_guard<std::mutex> ml(s->mirror_mu);
        o->mirror = s->mirror;
        s->mirror = nullptr;
      }
      const double t0 = now_ms();
      const hipError_t e = hipMalloc(&o->dev_gmap, (nl + 1) * 4);
      if (e != hipSuccess) {
        o->dev_gmap = nullptr;
        free_index(o);
        return set_err(c, EMQX_GM_ENOMEM, std::string("index_update: hipMalloc (id map): ") + hipGetErrorString(e));
      }
      const std::vector<uint32_t> none;
      GmapJob job;
      job.old_gmap = s->view.gmap;
      job.nb = nl;
      job.sh = GmapShift{&G, &none};
      job.new_gmap = static_cast<uint32_t*>(o->dev_gmap);
      job.n_new = nl;
      if (const int rc = shift_gmap_device(c, job)) {
        free_index(o);
        return rc;
      }
      o->view.gmap = job.new_gmap;
      tl_ustats.device_ms = now_ms() - t0;
      kinds[k] = EMQX_GM_UPD_SHIFT;
    } else {
      bool patched = false;
      if (delta <= std::max<uint64_t>(4096, nl / 8) && p.well_formed) {
        std::lock_guard<std::mutex> ml(s->mirror_mu);
        if (s->mirror) {
          const GmapShift gs{&G, &p.add_gid};
          const int rc = patch_update(c, s, p.tomb, p.dset, &o, nullptr, false, nullptr, &gs);
          if (rc < 0) return rc;
          patched = rc == 0;  // (1: a table has no room, nothing changed)
        }
      }
      if (patched) {
        kinds[k] = EMQX_GM_UPD_PATCH;
      } else {
        // this shard alone recompiled, with its filters' new global ids
        std::vector<uint8_t> b;
        std::vector<uint64_t> off{0};
        auto dit = p.dset.begin();
        auto tit = p.tomb.begin();
        auto put = [&](const uint8_t* q, uint64_t l) {
          b.insert(b.end(), q, q + l);
          off.push_back(b.size());
        };
        s->ft.for_each([&](uint64_t i, const uint8_t* bp, uint64_t bl) {
          while (dit != p.dset.end() &&
                 cmp_filter(reinterpret_cast<const uint8_t*>(dit->data()), dit->size(), bp, bl) < 0) {
            put(reinterpret_cast<const uint8_t*>(dit->data()), dit->size());
            ++dit;
          }
          if (tit != p.tomb.end() && *tit == i) {
            ++tit;
            return;
          }
          put(bp, bl);
        });
        for (; dit != p.dset.end(); ++dit) put(reinterpret_cast<const uint8_t*>(dit->data()), dit->size());
        b.resize(b.size() + 64, 0);
        const uint64_t n = off.size() - 1;
        if (n != ng.size()) return set_err(c, EMQX_GM_EINVAL, "index_update: shard id map out of step");
        std::vector<uint32_t> perm(n + 1);
        const double t0 = now_ms();
        if (const int rc = build_index(c, b.data(), off.data(), n, nullptr, nullptr, perm.data(), &o, nullptr,
                                       n ? ng.data() : nullptr, true))
          return rc;
        tl_ustats.device_ms = now_ms() - t0;
        kinds[k] = EMQX_GM_UPD_REBUILD;
      }
    }
    if (o->dev_gmap) {
      o->gmap = std::move(ng);
      o->info.device_bytes = o->dev_bytes + (o->gmap.size() + 1) * 4;
    }
    ns[k] = o;
    return 0;
  };
  const int rc = run_all(K, [&](int k) -> int {
    MemberLock lk(mem[k]);
    const emqx_gm_update_stats saved = tl_ustats;  // (shard 0 runs on the calling thread)
    tl_ustats = emqx_gm_update_stats{};
    const int r = shard_step(k);
    st[k] = tl_ustats;
    tl_ustats = saved;
    return r;
  });
  fshard_thread.join();
  hipSetDevice(ctx->device);
  if (rc) {  // (a shard patched before another failed took its line's mirror with it: prev's next update rebuilds that shard)
    for (emqx_gm_index* o : ns) free_index(o);
    return rc;
  }
  // ---- the host side of the new snapshot
  std::unique_ptr<emqx_gm_index> idx(new emqx_gm_index);
  idx->device = ctx->device;
  retain_route(prev->route);
  idx->route = prev->route;
  idx->shards = ns;
  idx->fshard = std::move(nfshard);
  idx->ft = prev->ft.apply(G.dels, dset);
  emqx_gm_index_info_t& in = idx->info;
  in.n_filters = nf_new;
  in.n_wildcard = prev->info.n_wildcard - twild + dwild;
  in.trie_empty = in.n_wildcard == 0;
  bool rebuilt = false;
  for (int k = 0; k < K; ++k) {
    const emqx_gm_index* s = ns[k];
    in.n_nodes += s->info.n_nodes;
    in.n_edges += s->info.n_edges;
    in.n_words = std::max(in.n_words, s->info.n_words);
    in.device_bytes += s->info.device_bytes;
    in.max_depth = std::max(in.max_depth, s->info.max_depth);
    rebuilt = rebuilt || kinds[k] == EMQX_GM_UPD_REBUILD;
    tl_ustats.device_ms = std::max(tl_ustats.device_ms, st[k].device_ms);
    tl_ustats.blobs_reused += st[k].blobs_reused;
    tl_ustats.blobs_fresh += st[k].blobs_fresh;
    tl_ustats.mirror_loaded = tl_ustats.mirror_loaded || st[k].mirror_loaded;
    tl_ustats.mirror_bytes += st[k].mirror_bytes;
    tl_ustats.mirror_ms = std::max(tl_ustats.mirror_ms, st[k].mirror_ms);
  }
  tl_ustats.kind = rebuilt ? EMQX_GM_UPD_REBUILD : EMQX_GM_UPD_PATCH;
  tl_shard_kinds = kinds;
  *out = idx.release();
  return EMQX_GM_OK;
}

int run_match_sharded(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                      uint32_t flags, emqx_gm_csr* out) {
  const std::vector<emqx_gm_ctx*> mem = devices_of(ctx);
  const int K = int(idx->shards.size());
  if (K > int(mem.size())) return set_err(ctx, EMQX_GM_EINVAL, "match: a sharded index of another context");
  // ---- every topic's device (offsets checked first: the route reads each topic)
  std::atomic<int> bad{0};
  parallel_ranges(n, 1 << 16, [&](uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; ++i)
      if (to[i + 1] < to[i]) bad.store(1);
  });
  if (bad.load()) return set_err(ctx, EMQX_GM_EINVAL, "match: topic offsets not monotone");
  std::vector<uint32_t> dest(n);
  parallel_ranges(n, 1 << 16, [&](uint64_t a, uint64_t b) { route_topics_host(idx->route, tb, to + a, b - a, dest.data() + a); });
  // ---- each device's topics, in batch order (a stable counting sort)
  std::vector<uint64_t> cnt(K + 1, 0);
  for (uint64_t i = 0; i < n; ++i) ++cnt[dest[i] + 1];
  for (int k = 0; k < K; ++k) cnt[k + 1] += cnt[k];
  std::vector<uint64_t> pos(n), fill(cnt.begin(), cnt.end() - 1);
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t p = fill[dest[i]]++;
    order[p] = uint32_t(i);
    pos[i] = p - cnt[dest[i]];  // its row in its device's result
  }
  // ---- each device gathers and matches its batch (all at once)
  struct Part {
    std::vector<uint8_t> b;
    std::vector<uint64_t> o;
    emqx_gm_csr res{};
    emqx_gm_match_stats st{};
  };
  std::vector<Part> P(K);
  const int rc = run_all(K, [&](int k) -> int {
    MemberLock lk(mem[k]);
    Part& p = P[k];
    const uint64_t a = cnt[k], m = cnt[k + 1] - a;
    p.o.resize(m + 1);
    p.o[0] = 0;
    for (uint64_t j = 0; j < m; ++j) p.o[j + 1] = p.o[j] + (to[order[a + j] + 1] - to[order[a + j]]);
    p.b.resize(p.o[m] + 64);
    for (uint64_t j = 0; j < m; ++j) {
      const uint32_t i = order[a + j];
      if (to[i + 1] > to[i]) std::memcpy(p.b.data() + p.o[j], tb + to[i], to[i + 1] - to[i]);
    }
    const int r = run_match_host(mem[k], idx->shards[k], p.b.data(), p.o.data(), m, flags & ~EMQX_GM_DEVICE_IO, &p.res);
    p.st = mem[k]->stats;
    return r;
  });
  hipSetDevice(ctx->device);
  auto drop = [&]() {
    for (int k = 0; k < K; ++k)
      if (P[k].res.row_off || P[k].res.ids) {
        MemberLock lk(mem[k]);
        mem[k]->hpool->release(P[k].res.row_off);
        mem[k]->hpool->release(P[k].res.ids);
      }
    hipSetDevice(ctx->device);
  };
  if (rc) {
    drop();
    return rc;
  }
  // ---- every row back at its topic's place
  uint64_t total = 0;
  for (auto& p : P) total += p.res.nnz;
  uint64_t* r_off = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8));
  uint32_t* r_ids = static_cast<uint32_t*>(ctx->hpool->alloc(total * 4 + 16));
  if (!r_off || !r_ids) {
    ctx->hpool->release(r_off);
    ctx->hpool->release(r_ids);
    drop();
    return set_err(ctx, EMQX_GM_ENOMEM, "match: host result");
  }
  r_off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* ro = P[dest[i]].res.row_off;
    r_off[i + 1] = r_off[i] + (ro[pos[i] + 1] - ro[pos[i]]);
  }
  parallel_ranges(n, 1 << 16, [&](uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; ++i) {
      const emqx_gm_csr& s = P[dest[i]].res;
      const uint64_t l = r_off[i + 1] - r_off[i];
      if (l) std::memcpy(r_ids + r_off[i], s.ids + s.row_off[pos[i]], l * 4);
    }
  });
  drop();
  emqx_gm_match_stats tot{};
  tot.n_topics = n;
  tot.nnz = total;
  for (auto& p : P) {
    tot.n_overflow += p.st.n_overflow;
    tot.n_wildcard_topics += p.st.n_wildcard_topics;
    tot.probes += p.st.probes;
    tot.match_kernel_ms = std::max(tot.match_kernel_ms, p.st.match_kernel_ms);
    tot.total_device_ms = std::max(tot.total_device_ms, p.st.total_device_ms);
  }
  ctx->stats = tot;
  out->n_rows = n;
  out->nnz = total;
  out->row_off = r_off;
  out->ids = r_ids;
  out->on_device = 0;
  out->priv = ctx;
  return EMQX_GM_OK;
}

int run_fanout_sharded(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
                       emqx_gm_csr* out) {
  const std::vector<emqx_gm_ctx*> mem = devices_of(ctx);
  const int K = int(idx->shards.size());
  if (K > int(mem.size())) return set_err(ctx, EMQX_GM_EINVAL, "fanout: a sharded index of another context");
  const uint64_t n = m->n_rows, nnz = m->nnz, nf = idx->info.n_filters;
  if (m->row_off[0] != 0 || m->row_off[n] != nnz) return set_err(ctx, EMQX_GM_EINVAL, "fanout: row offsets");
  for (uint64_t i = 0; i < n; ++i)
    if (m->row_off[i + 1] < m->row_off[i]) return set_err(ctx, EMQX_GM_EINVAL, "fanout: row offsets not monotone");
  for (uint64_t j = 0; j < nnz; ++j)
    if (m->ids[j] >= nf) return set_err(ctx, EMQX_GM_EINVAL, "fanout: filter id out of range");
  // ---- each row's shard: that of its first filter held by one shard (a row's
  // filters all live on its topic's shard, or on every shard)
  std::vector<uint32_t> dest(n);
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t s = 0;
    for (uint64_t j = m->row_off[i]; j < m->row_off[i + 1]; ++j)
      if (idx->fshard[m->ids[j]] != EMQX_GM_ALL_SHARDS) {
        s = idx->fshard[m->ids[j]];
        break;
      }
    dest[i] = s;
  }
  std::vector<uint64_t> cnt(K + 1, 0);
  for (uint64_t i = 0; i < n; ++i) ++cnt[dest[i] + 1];
  for (int k = 0; k < K; ++k) cnt[k + 1] += cnt[k];
  std::vector<uint64_t> pos(n), fill(cnt.begin(), cnt.end() - 1);
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t p = fill[dest[i]]++;
    order[p] = uint32_t(i);
    pos[i] = p - cnt[dest[i]];
  }
  struct Part {
    std::vector<uint64_t> o;
    std::vector<uint32_t> ids;
    emqx_gm_csr res{};
  };
  std::vector<Part> P(K);
  const int rc = run_all(K, [&](int k) -> int {
    MemberLock lk(mem[k]);
    Part& p = P[k];
    const emqx_gm_index* s = idx->shards[k];
    const uint64_t a = cnt[k], r = cnt[k + 1] - a;
    p.o.assign(1, 0);
    for (uint64_t q = 0; q < r; ++q) {
      const uint32_t i = order[a + q];
      for (uint64_t j = m->row_off[i]; j < m->row_off[i + 1]; ++j) {  // global id -> the shard's local id
        auto it = std::lower_bound(s->gmap.begin(), s->gmap.end(), m->ids[j]);
        if (it == s->gmap.end() || *it != m->ids[j])
          return set_err(mem[k], EMQX_GM_EINVAL, "fanout: a row's filters are not on one shard");
        p.ids.push_back(uint32_t(it - s->gmap.begin()));
      }
      p.o.push_back(p.ids.size());
    }
    if (p.ids.empty()) p.ids.push_back(0);
    emqx_gm_csr sub{};
    sub.n_rows = r;
    sub.nnz = p.o.back();
    sub.row_off = p.o.data();
    sub.ids = p.ids.data();
    sub.on_device = 0;
    return run_fanout(mem[k], s, &sub, flags & EMQX_GM_WITH_EXACT, &p.res);
  });
  hipSetDevice(ctx->device);
  auto drop = [&]() {
    for (int k = 0; k < K; ++k)
      if (P[k].res.row_off || P[k].res.ids) {
        MemberLock lk(mem[k]);
        mem[k]->hpool->release(P[k].res.row_off);
        mem[k]->hpool->release(P[k].res.ids);
      }
    hipSetDevice(ctx->device);
  };
  if (rc) {
    drop();
    return rc;
  }
  uint64_t total = 0;
  for (auto& p : P) total += p.res.nnz;
  uint64_t* r_off = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8));
  uint32_t* r_ids = static_cast<uint32_t*>(ctx->hpool->alloc(total * 4 + 16));
  if (!r_off || !r_ids) {
    ctx->hpool->release(r_off);
    ctx->hpool->release(r_ids);
    drop();
    return set_err(ctx, EMQX_GM_ENOMEM, "fanout: host result");
  }
  r_off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* ro = P[dest[i]].res.row_off;
    r_off[i + 1] = r_off[i] + (ro[pos[i] + 1] - ro[pos[i]]);
  }
  parallel_ranges(n, 1 << 16, [&](uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; ++i) {
      const emqx_gm_csr& s = P[dest[i]].res;
      const uint64_t l = r_off[i + 1] - r_off[i];
      if (l) std::memcpy(r_ids + r_off[i], s.ids + s.row_off[pos[i]], l * 4);
    }
  });
  drop();
  emqx_gm_match_stats tot{};
  tot.n_topics = n;
  tot.nnz = total;
  ctx->stats = tot;
  out->n_rows = n;
  out->nnz = total;
  out->row_off = r_off;
  out->ids = r_ids;
  out->on_device = 0;
  out->priv = ctx;
  return EMQX_GM_OK;
}

}  // namespace gm
