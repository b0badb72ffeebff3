// gm_authz.hip — the gfx950 kernel of the authorization check (layout and
// semantics: gm_authz.h; the reference path it replaces:
// emqx_authz:do_authorize/4, apps/emqx_authz/src/emqx_authz.erl:307-317, over
// emqx_authz_rule:matches/4 and emqx_authz_mnesia:authorize/4).  No '$'-rule
// here: '#' and '+/x' authorize '$SYS/x' (emqx_topic:match/2's list clauses).
//
// k_authz_check: one request per lane.  The lane tokenizes its topic, looks
// each word up in the dictionary (an absent word gets NONE, which only '+' and
// '#' accept) and keeps the ids of its first AZ_LEVELS words as a column of an
// LDS array [level][lane] -- the filter loop indexes them at run time, which a
// per-lane register array could only do through scratch -- plus two bit masks:
// at which levels the word equals the client's substituted '${clientid}' /
// '${username}' word.  A topic of more than AZ_LEVELS words compares bytes
// against the word arena instead (az_filter_bytes), at any depth.
// Then the segments in order.  A GLOBAL segment is scanned by the whole wave in
// step: every lane reads the same rule at the same step (wave-uniform loads), a
// lane that has its hit drops out, and the wave leaves the scan when all its
// lanes are done.  A keyed segment is one probe of its key table per lane and
// a scan of the lane's own short range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gm_authz.h"
#include "gm_device.h"

namespace gm {
namespace {

struct AzReq {
  const uint8_t *p, *cid, *un;  // topic, clientid, username bytes
  uint32_t len, clen, ulen;
  uint32_t L;             // words of the topic
  uint32_t cmask, umask;  // bit i: word i equals the substituted ${clientid} / ${username} word (levels < AZ_LEVELS)
  uint32_t peer[4];
  uint32_t re_mask;
  uint32_t action;
  bool has_cid, has_un, has_peer, v6;
};

struct AzBatchDev {
  const uint8_t *tb, *cb, *ub;
  const uint32_t *to, *co, *uo;  // [n + 1] each
  const uint8_t *flags, *peer, *action;
  const uint32_t* re_mask;
  uint8_t* verdict;
  uint32_t* rule;
  uint32_t n;
};

// the slot of a key in a keyed segment's table (absolute index), or NONE.  The
// rule range is read from the slot afterwards, by the caller: the lookup hands
// back one value, as dict_find (gm_device.h) does.  (With the range written through two
// out-parameters inside this loop, the gfx950 code lost it for every key longer
// than 8 bytes: after the tail compare the registers holding it were restored
// to the "no key" values.  tests/test_gpu_authz.py covers key lengths 0-255.)
__device__ uint32_t az_key_find(const AzView& v, const AzSeg& sg, const uint8_t* p, uint32_t len) {
  uint64_t head;
  const uint32_t h = dict_hash_bytes(p, len, &head);
  for (uint32_t s = h & sg.key_mask;; s = (s + 1) & sg.key_mask) {
    const uint32_t at = sg.key_lo + s;
    const AzKeySlot* e = v.keys + at;
    const uint32_t elen = e->len;
    if (elen == DICT_EMPTY_LEN) return NONE;
    if (elen != len || e->hash != h || e->head != head) continue;
    if (len <= 8 || bytes_eq(v.words.arena + e->off + 8, p + 8, len - 8)) return at;
  }
}

// emqx_topic:match/2, the list clauses (emqx_topic.erl:74-87) in their order,
// over the lane's word-id column; name and filter advance together, so position
// i of one always meets position i of the other.
__device__ __forceinline__ bool az_filter_ids(const uint32_t* fw, uint32_t n, uint32_t kind, const uint32_t* col,
                                              const AzReq& q) {
  if (kind == AZ_F_EQ) {  // match_topic/2, first clause: Topic =:= TopicFilter
    if (q.L != n) return false;
    bool ok = true;
    for (uint32_t i = 0; i < n && ok; ++i) ok = col[i * AZ_BLOCK] == fw[i];
    return ok;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t f = fw[i];
    if (i < q.L) {
      bool eq;
      if (kind == AZ_F_PATTERN && f == AZ_W_PH_CLIENTID) eq = (q.cmask >> i) & 1u;
      else if (kind == AZ_F_PATTERN && f == AZ_W_PH_USERNAME) eq = (q.umask >> i) & 1u;
      else eq = col[i * AZ_BLOCK] == f;
      if (eq || f == AZ_W_PLUS) continue;  // [H|T1],[H|T2] and [_|T1],['+'|T2]
    }
    return i == n - 1 && f == AZ_W_HASH;  // _, ['#']; every other clause is false
  }
  return q.L == n;  // [],[] against [_|_],[]
}

// does the name word p[0, wl) equal the client's value as ONE binary word (feed_var/3)
__device__ __forceinline__ bool az_is_value(const uint8_t* p, uint32_t wl, const uint8_t* val, uint32_t vlen) {
  return wl == vlen && az_is_binary_word(p, wl) && bytes_eq(p, val, wl);
}

// The same clauses for a topic of any depth: the name's words compared as bytes
// with the filter words' bytes in the arena (the reserved ids' bytes are there
// too, so an atom equals only the same atom).
__device__ bool az_filter_bytes(const AzView& v, const uint32_t* fw, uint32_t n, uint32_t kind, const AzReq& q) {
  uint32_t pos = 0;
  bool have = true;  // the name has a word at pos
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t f = fw[i];
    if (have) {
      uint32_t e = pos;
      while (e < q.len && q.p[e] != '/') ++e;
      const uint32_t wl = e - pos;
      bool eq;
      if (kind == AZ_F_PATTERN && f == AZ_W_PH_CLIENTID && q.has_cid) {
        eq = az_is_value(q.p + pos, wl, q.cid, q.clen);
      } else if (kind == AZ_F_PATTERN && f == AZ_W_PH_USERNAME && q.has_un) {
        eq = az_is_value(q.p + pos, wl, q.un, q.ulen);
      } else {
        const uint32_t a = v.words.word_off[f];
        eq = wl == v.words.word_off[f + 1] - a && bytes_eq(q.p + pos, v.words.arena + a, wl);
      }
      if (eq || (kind != AZ_F_EQ && f == AZ_W_PLUS)) {
        have = e < q.len;
        pos = e + 1;
        continue;
      }
    }
    return kind != AZ_F_EQ && i == n - 1 && f == AZ_W_HASH;
  }
  return !have;
}

// emqx_authz_rule:match/4 (emqx_authz_rule.erl:119-125) of rule r for the lane's request
__device__ __forceinline__ bool az_rule_match(const AzView& v, uint32_t r, const AzReq& q, const uint32_t* col) {
  const AzRule ru = v.rules[r];
  const uint32_t who_hi = v.rules[r + 1].who_lo, filt_hi = v.rules[r + 1].filt_lo;
  if (!((ru.meta >> 2) & 3u & q.action)) return false;  // match_action/2
  const bool is_or = ru.meta & AZ_M_OR;
  bool acc = !is_or;  // the foldl identities: AND [] is true, OR [] is false
  for (uint32_t l = ru.who_lo; l < who_hi; ++l) {
    const AzLeaf lf = v.leaves[l];
    bool m = false;
    if (lf.kind == EMQX_GM_AUTHZ_WHO_USERNAME) {
      m = q.has_un && q.ulen == lf.b && bytes_eq(q.un, v.words.arena + lf.a, lf.b);
    } else if (lf.kind == EMQX_GM_AUTHZ_WHO_CLIENTID) {
      m = q.has_cid && q.clen == lf.b && bytes_eq(q.cid, v.words.arena + lf.a, lf.b);
    } else if (lf.kind == EMQX_GM_AUTHZ_WHO_IPADDR) {
      if (q.has_peer)
        for (uint32_t c = 0; c < lf.b && !m; ++c) m = az_cidr_match(v.cidrs[lf.a + c], q.peer, q.v6);
    } else {
      m = (q.re_mask >> lf.a) & 1u;
    }
    acc = is_or ? (acc || m) : (acc && m);
  }
  if (!acc) return false;
  for (uint32_t f = ru.filt_lo; f < filt_hi; ++f) {
    const AzFilter fl = v.filters[f];
    const uint32_t n = fl.n_kind & AZ_F_N_MASK, kind = fl.n_kind >> 30;
    const uint32_t* fw = v.fwords + fl.w_lo;
    if (q.L <= AZ_LEVELS ? az_filter_ids(fw, n, kind, col, q) : az_filter_bytes(v, fw, n, kind, q)) return true;
  }
  return false;
}

__global__ __launch_bounds__(AZ_BLOCK) void k_authz_check(AzView v, AzBatchDev b) {
  __shared__ uint32_t s_w[AZ_LEVELS * AZ_BLOCK];  // [level][lane] word ids
  const uint32_t i = blockIdx.x * AZ_BLOCK + threadIdx.x;
  const bool live = i < b.n;
  uint32_t* col = s_w + threadIdx.x;
  AzReq q{};
  if (live) {
    const uint32_t t0 = b.to[i], c0 = b.co[i], u0 = b.uo[i];
    const uint8_t fl = b.flags[i];
    q.p = b.tb + t0, q.len = b.to[i + 1] - t0;
    q.cid = b.cb + c0, q.clen = b.co[i + 1] - c0;
    q.un = b.ub + u0, q.ulen = b.uo[i + 1] - u0;
    q.has_cid = fl & EMQX_GM_AUTHZ_F_CLIENTID;
    q.has_un = fl & EMQX_GM_AUTHZ_F_USERNAME;
    q.has_peer = fl & EMQX_GM_AUTHZ_F_PEERHOST;
    q.v6 = fl & EMQX_GM_AUTHZ_F_IPV6;
    az_peer_words(b.peer + 16ull * i, q.v6, q.peer);
    q.action = b.action[i];
    q.re_mask = b.re_mask[i];
    // ---- tokenize (emqx_topic:words/1: split on '/', empty words kept)
    uint32_t s = 0;
    for (uint32_t e = 0; e <= q.len; ++e)
      if (e == q.len || q.p[e] == '/') {
        if (q.L < AZ_LEVELS) {
          const uint32_t wl = e - s;
          const uint32_t id = dict_find(v.words, q.p + s, wl);
          col[q.L * AZ_BLOCK] = id;
          // feed_var/3: the value as one binary word, or the placeholder's own text when undefined
          const bool ic = q.has_cid ? az_is_value(q.p + s, wl, q.cid, q.clen) : id == AZ_W_PH_CLIENTID;
          const bool iu = q.has_un ? az_is_value(q.p + s, wl, q.un, q.ulen) : id == AZ_W_PH_USERNAME;
          q.cmask |= uint32_t(ic) << q.L;
          q.umask |= uint32_t(iu) << q.L;
        }
        ++q.L;
        s = e + 1;
      }
  }
  // (each lane reads only its own column: no barrier is needed)
  uint32_t verdict = EMQX_GM_AUTHZ_NOMATCH, rid = EMQX_GM_AUTHZ_NO_RULE;
  bool done = !live;
  for (uint32_t sgi = 0; sgi < v.n_segs; ++sgi) {
    if (__all(done)) break;
    const AzSeg sg = v.segs[sgi];
    if (sg.kind == EMQX_GM_AUTHZ_GLOBAL) {
      for (uint32_t r = sg.r_lo; r < sg.r_hi; ++r) {
        if (__all(done)) break;
        if (!done && az_rule_match(v, r, q, col)) {
          const AzRule ru = v.rules[r];
          verdict = ru.meta & 3u, rid = ru.id;
          done = true;
        }
      }
    } else if (!done) {
      uint32_t slot = NONE, lo = 0, hi = 0;
      if (sg.kind == EMQX_GM_AUTHZ_BY_CLIENTID) {
        if (q.has_cid) slot = az_key_find(v, sg, q.cid, q.clen);
      } else if (q.has_un) {
        slot = az_key_find(v, sg, q.un, q.ulen);
      }
      if (slot != NONE) lo = v.keys[slot].r_lo, hi = v.keys[slot].r_hi;
      for (uint32_t r = lo; r < hi; ++r)
        if (az_rule_match(v, r, q, col)) {
          const AzRule ru = v.rules[r];
          verdict = ru.meta & 3u, rid = ru.id;
          done = true;
          break;
        }
    }
  }
  if (live) {
    b.verdict[i] = uint8_t(verdict);
    b.rule[i] = rid;
  }
}

constexpr uint64_t AZ_CHUNK_REQS = 1ull << 20;   // requests of one device round trip
constexpr uint64_t AZ_CHUNK_BYTES = 1ull << 30;  // ... and the bytes of each of its three text columns (u32 offsets)

}  // namespace

int az_upload(emqx_gm_ctx* ctx, emqx_gm_authz* t) {
  if (const int rc = table_upload(ctx, t->blob, t->bytes, "authz_build", &t->dev_base)) return rc;
  const AzView& h = t->hv;
  const void* hb = t->blob.data();
  void* db = t->dev_base;
  t->dv.segs = rebase(h.segs, hb, db);
  t->dv.rules = rebase(h.rules, hb, db);
  t->dv.leaves = rebase(h.leaves, hb, db);
  t->dv.cidrs = rebase(h.cidrs, hb, db);
  t->dv.filters = rebase(h.filters, hb, db);
  t->dv.fwords = rebase(h.fwords, hb, db);
  t->dv.keys = rebase(h.keys, hb, db);
  t->dv.words = DictView{rebase(h.words.dict, hb, db), rebase(h.words.word_off, hb, db), rebase(h.words.arena, hb, db),
                         h.words.dict_mask};
  t->device = ctx->device;
  t->info.device_bytes = t->bytes;
  return EMQX_GM_OK;
}

void az_free_device(emqx_gm_authz* t) {
  table_free(t->device, t->dev_base);  // (waits for the device: no queued check still reads the tables)
  t->dev_base = nullptr;
}

// One chunk: every input staged into one page-locked buffer and sent with one
// copy, the kernel, one copy back, one wait -- a single device round trip.
static int az_check_chunk(emqx_gm_ctx* ctx, emqx_gm_authz* t, const emqx_gm_authz_batch* b, uint64_t at, uint64_t m,
                          bool timed, uint8_t* verdict, uint32_t* rule) {
  hipStream_t st = ctx->stream;
  const uint64_t tb = b->topic_off[at + m] - b->topic_off[at], cb = b->clientid_off[at + m] - b->clientid_off[at],
                 ub = b->username_off[at + m] - b->username_off[at];
  size_t o[10], sz = 0;
  o[0] = sz, sz = al16(sz + (m + 1) * 4);  // topic offsets
  o[1] = sz, sz = al16(sz + (m + 1) * 4);  // clientid offsets
  o[2] = sz, sz = al16(sz + (m + 1) * 4);  // username offsets
  o[3] = sz, sz = al16(sz + m * 4);        // re_mask
  o[4] = sz, sz = al16(sz + m * 16);       // peerhost
  o[5] = sz, sz = al16(sz + m);            // flags
  o[6] = sz, sz = al16(sz + m);            // action
  o[7] = sz, sz = al16(sz + tb + 16);
  o[8] = sz, sz = al16(sz + cb + 16);
  o[9] = sz, sz = al16(sz + ub + 16);
  const size_t out_rule = 0, out_verdict = al16(m * 4), out_sz = al16(out_verdict + m);
  PinBuf pin(ctx->pins, sz + out_sz);
  PoolBuf d_in(ctx->pool, sz), d_out(ctx->pool, out_sz);
  if (!pin.p || !d_in.p || !d_out.p) return set_err(ctx, EMQX_GM_ENOMEM, "authz_check: staging buffers");
  uint8_t* h = static_cast<uint8_t*>(pin.p);
  auto rebase = [&](size_t off, const uint64_t* src) {
    auto* dst = reinterpret_cast<uint32_t*>(h + off);
    for (uint64_t k = 0; k <= m; ++k) dst[k] = uint32_t(src[at + k] - src[at]);
  };
  rebase(o[0], b->topic_off);
  rebase(o[1], b->clientid_off);
  rebase(o[2], b->username_off);
  std::memcpy(h + o[3], b->re_mask + at, m * 4);
  std::memcpy(h + o[4], b->peerhost + 16 * at, m * 16);
  std::memcpy(h + o[5], b->flags + at, m);
  std::memcpy(h + o[6], b->action + at, m);
  if (tb) std::memcpy(h + o[7], b->topic_bytes + b->topic_off[at], tb);
  if (cb) std::memcpy(h + o[8], b->clientid_bytes + b->clientid_off[at], cb);
  if (ub) std::memcpy(h + o[9], b->username_bytes + b->username_off[at], ub);
  GM_HIP(ctx, hipMemcpyAsync(d_in.p, h, sz, hipMemcpyHostToDevice, st));
  uint8_t* di = d_in.as<uint8_t>();
  uint8_t* dout = d_out.as<uint8_t>();
  AzBatchDev db{};
  db.to = reinterpret_cast<const uint32_t*>(di + o[0]);
  db.co = reinterpret_cast<const uint32_t*>(di + o[1]);
  db.uo = reinterpret_cast<const uint32_t*>(di + o[2]);
  db.re_mask = reinterpret_cast<const uint32_t*>(di + o[3]);
  db.peer = di + o[4];
  db.flags = di + o[5];
  db.action = di + o[6];
  db.tb = di + o[7];
  db.cb = di + o[8];
  db.ub = di + o[9];
  db.rule = reinterpret_cast<uint32_t*>(dout + out_rule);
  db.verdict = dout + out_verdict;
  db.n = uint32_t(m);
  EventSet<2> ev;
  if (timed) {
    if (const int rc = ev.create(ctx)) return rc;
    GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  }
  hipLaunchKernelGGL(k_authz_check, dim3(uint32_t((m + AZ_BLOCK - 1) / AZ_BLOCK)), dim3(AZ_BLOCK), 0, st, t->dv, db);
  GM_HIP(ctx, hipGetLastError());
  if (timed) GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  GM_HIP(ctx, hipMemcpyAsync(h + sz, dout, out_sz, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  std::memcpy(rule + at, h + sz + out_rule, m * 4);
  std::memcpy(verdict + at, h + sz + out_verdict, m);
  if (timed) {
    float ms = 0;
    GM_HIP(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    t->last_kernel_ms += ms;
  }
  return EMQX_GM_OK;
}

int az_check_device(emqx_gm_ctx* ctx, emqx_gm_authz* t, const emqx_gm_authz_batch* b, bool timed, uint8_t* verdict,
                    uint32_t* rule) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  if (timed) t->last_kernel_ms = 0;
  for (uint64_t at = 0; at < b->n;) {
    // the next chunk: up to AZ_CHUNK_REQS requests whose text columns each stay under AZ_CHUNK_BYTES
    uint64_t m = std::min<uint64_t>(AZ_CHUNK_REQS, b->n - at);
    auto fits = [&](uint64_t k) {
      return b->topic_off[at + k] - b->topic_off[at] < AZ_CHUNK_BYTES &&
             b->clientid_off[at + k] - b->clientid_off[at] < AZ_CHUNK_BYTES &&
             b->username_off[at + k] - b->username_off[at] < AZ_CHUNK_BYTES;
    };
    while (m > 1 && !fits(m)) m /= 2;
    if (!fits(m)) return set_err(ctx, EMQX_GM_EINVAL, "authz_check: a request of 1 GiB");
    if (const int rc = az_check_chunk(ctx, t, b, at, m, timed, verdict, rule)) return rc;
    at += m;
  }
  return EMQX_GM_OK;
}

}  // namespace gm
