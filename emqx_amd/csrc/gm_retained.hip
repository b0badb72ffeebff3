// gm_retained.hip — gfx950 kernels of the retained-topic lookup (layout and
// semantics: gm_retained.h; the reference path it replaces:
// emqx_retainer_mnesia:match_messages/1 + condition/1,
// apps/emqx_retainer/src/emqx_retainer_mnesia.erl:210-244).  No '$'-rule here:
// '#' and '+/x' match '$SYS/...' topics, unlike the publish-side walk.
//
// k_ret_walk: one wave per filter, run twice per call (count, then fill, with
// the library's scan between).  The wave walks the trie as an ordered, chunked
// descent: frame d holds the matched nodes of the filter's first d words as up
// to 64 (lo, hi) node ranges; the wave takes the next chunk of the deepest
// frame that has work -- up to 64 ranges for a '+' step (range -> the one range
// of its children), up to 64 nodes for a literal step (one binary search over
// the parent's children per lane) or the emit step -- and compacts the hits in
// lane order into the next frame.  Everything below a chunk is finished before
// the next chunk of the same frame is taken, and subtrees are rank ordered, so
// ids come out ascending without a sort.  The state is depth_max + 1 frames and
// their cursors whatever the fan-out: no truncation, no overflow path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_device.h"
#include "gm_retained.h"

namespace gm {
namespace {

// the child of `parent` through word id w: binary search over its contiguous, ascending children
__device__ uint32_t ret_child(const RetView& v, uint32_t parent, uint32_t w) {
  uint32_t a = v.nodes[parent].child_lo, b = v.nodes[parent + 1].child_lo;
  while (a < b) {
    const uint32_t m = a + (b - a) / 2, x = v.nodes[m].word & RET_WORD_MASK;
    if (x == w) return m;
    if (x < w) a = m + 1;
    else b = m;
  }
  return NONE;
}

// Emit ranks [rlo, rhi) of filter row f (wave-uniform arguments): the lanes
// stride over the range, so expiry[] and ids[] are read coalesced.
__device__ __forceinline__ void emit_range(const RetView& v, uint32_t rlo, uint32_t rhi, uint64_t now, bool fill,
                                           uint32_t* out, uint64_t row_at, uint64_t row_end, uint64_t& total,
                                           uint32_t lane) {
  const bool expiring = v.flags & RET_HAS_EXPIRY;
  if (!expiring && !fill) {
    total += rhi - rlo;
    return;
  }
  for (uint64_t b = rlo; b < rhi; b += 64) {
    const uint64_t r = b + lane;
    bool e = r < rhi;
    if (e && expiring) {
      const uint64_t x = v.expiry[r];
      e = x == 0 || x > now;
    }
    const uint64_t m = __ballot(e);
    if (e && fill) {
      const uint64_t o = row_at + total + lanes_below(m, lane);
      if (o < row_end) out[o] = v.ids[r];  // (the row is as long as the count pass found it)
    }
    total += __popcll(m);
  }
}

// GWS: the per-wave state lives in a global workspace (ws) instead of LDS.
template <bool GWS>
__global__ __launch_bounds__(RET_WAVES_PER_BLOCK * 64) void k_ret_walk(RetView v, const uint8_t* __restrict__ fb,
                                                                      const uint64_t* __restrict__ fo, uint64_t nf,
                                                                      uint64_t now, int fill, uint64_t* row_len,
                                                                      const uint64_t* row_off, uint32_t* out_ids,
                                                                      uint32_t* ws, uint32_t wave_words) {
  extern __shared__ __align__(16) uint32_t s_ret[];
  const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const uint64_t wave = uint64_t(blockIdx.x) * RET_WAVES_PER_BLOCK + wib;
  const uint64_t n_waves = uint64_t(gridDim.x) * RET_WAVES_PER_BLOCK;
  uint32_t* st = GWS ? ws + wave * wave_words : s_ret + wib * wave_words;
  const uint32_t D = v.depth_max + 1;
  uint2* frames = reinterpret_cast<uint2*>(st);  // [D][64]
  uint32_t* cnt = st + D * 128;                  // items of frame d
  uint32_t* pos = cnt + D;                       // its cursor: the next item
  uint32_t* sub = pos + D;                       // nodes of that item already taken
  uint32_t* wid = sub + D;                       // word starts, then word ids
  uint32_t* scr = wid + D;                       // [64]

  for (uint64_t f = wave; f < nf; f += n_waves) {
    const uint8_t* p = fb + fo[f];
    const uint32_t len = uint32_t(fo[f + 1] - fo[f]);
    uint64_t total = 0;
    const uint64_t row_at = fill ? row_off[f] : 0, row_end = fill ? row_off[f + 1] : 0;
    if (fill && row_at == row_end) continue;  // an empty row: nothing to write
    // ---- tokenize: word k starts behind the k-th '/'
    wave_sync();
    if (lane == 0) wid[0] = 0;
    uint32_t ns = 0;
    for (uint32_t base = 0; base < len; base += 64) {
      const uint32_t i = base + lane;
      const bool sl = i < len && p[i] == '/';
      const uint64_t m = __ballot(sl);
      if (sl) {
        const uint32_t j = ns + lanes_below(m, lane) + 1;
        if (j < D) wid[j] = i + 1;
      }
      ns += __popcll(m);
    }
    const uint32_t L = ns + 1;  // words of the filter
    bool ok = L <= D;           // more words than the deepest topic (plus a '#'): nothing can match
    bool hash = false;
    uint32_t P = L;             // words before the final '#'
    wave_sync();
    if (ok) {
      const uint32_t ls = uni(wid[L - 1]);
      hash = len - ls == 1 && p[ls] == '#';
      P = hash ? L - 1 : L;
      if (P > v.depth_max) ok = false;
      else if (!hash && v.depth_ends[P] == 0) ok = false;  // no stored topic has that many words
    }
    if (ok) {
      bool bad = false;
      for (uint32_t base = 0; base < P; base += 64) {
        const uint32_t k = base + lane;
        uint32_t s = 0, e = 0;
        if (k < P) {
          s = wid[k];
          e = k + 1 < L ? wid[k + 1] - 1 : len;
        }
        wave_sync();  // every start is read before an id replaces it
        if (k < P) {
          const uint32_t wl = e - s;
          uint32_t id;
          if (wl == 1 && p[s] == '+') id = RET_PLUS;
          else if (wl == 1 && p[s] == '#') id = NONE;  // '#' before the last word: no stored word equals it
          else id = dict_find<true>(v.words, p + s, wl);  // an unknown word ends the row empty
          wid[k] = id;
          bad |= id == NONE;
        }
      }
      if (__any(bad)) ok = false;
    }
    if (ok) {
      // ---- the descent
      if (lane == 0) {
        frames[0] = make_uint2(0u, 1u);  // the root
        cnt[0] = 1;
        pos[0] = 0;
        sub[0] = 0;
      }
      wave_sync();
      int d = 0;
      while (d >= 0) {
        const uint32_t c = uni(cnt[d]), ps = uni(pos[d]), sb = uni(sub[d]);
        if (ps >= c) {
          --d;
          continue;
        }
        const uint32_t w = uint32_t(d) < P ? uni(wid[d]) : 0u;
        const uint32_t i = ps + lane;
        const bool have = i < c;
        uint2 it = make_uint2(0u, 0u);
        if (have) it = frames[d * 64 + i];
        if (lane == 0) it.x += sb;
        if (uint32_t(d) < P && w == RET_PLUS) {
          // '+': each range of parents is one range of children
          uint32_t lo = 0, hi = 0;
          if (have) {
            lo = v.nodes[it.x].child_lo;
            hi = v.nodes[it.y].child_lo;
          }
          const bool keep = lo < hi;
          const uint64_t m = __ballot(keep);
          if (keep) frames[(d + 1) * 64 + lanes_below(m, lane)] = make_uint2(lo, hi);
          if (lane == 0) {
            pos[d] = min(c, ps + 64u);
            sub[d] = 0;
            cnt[d + 1] = __popcll(m);
            pos[d + 1] = 0;
            sub[d + 1] = 0;
          }
          wave_sync();
          ++d;
          continue;
        }
        // ---- take the next up to 64 NODES of the frame, one per lane
        const uint32_t sz = have ? min(it.y - it.x, 65u) : 0u;  // (65: a longer item is never taken whole)
        uint32_t incl = sz;
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = __shfl_up(incl, o, 64);
          if (lane >= uint32_t(o)) incl += t;
        }
        scr[lane] = incl;
        wave_sync();
        const uint32_t T = min(64u, uni(scr[63]));
        uint32_t t = 0;  // the item of this lane's node: the first whose inclusive sum passes the lane
        for (uint32_t step = 32; step; step >>= 1)
          if (scr[t + step - 1] <= lane) t += step;
        const uint32_t t_lo = __shfl(it.x, int(t), 64), t_excl = __shfl(incl - sz, int(t), 64);
        const bool act = lane < T;
        const uint32_t node = t_lo + (lane - t_excl);
        // the cursor moves past the items taken whole and into the one taken in part
        const uint32_t nfull = __popcll(__ballot(have && incl <= T));
        const uint32_t taken = nfull ? uni(scr[nfull - 1]) : 0u;
        wave_sync();  // scr is read before the next round writes it
        if (lane == 0) {
          pos[d] = ps + nfull;
          sub[d] = ps + nfull < c ? (nfull ? 0u : sb) + (T - taken) : 0u;
        }
        if (uint32_t(d) < P) {
          // a literal word: one binary search over the parent's children per lane
          uint32_t child = NONE;
          if (act) child = ret_child(v, node, w);
          const bool hit = child != NONE;
          const uint64_t m = __ballot(hit);
          if (hit) frames[(d + 1) * 64 + lanes_below(m, lane)] = make_uint2(child, child + 1);
          if (lane == 0) {
            cnt[d + 1] = __popcll(m);
            pos[d + 1] = 0;
            sub[d + 1] = 0;
          }
          wave_sync();
          ++d;
          continue;
        }
        // ---- emit (d == P): the nodes reached by the whole filter
        RetNode nd{0, 0, 0, 0};
        if (act) nd = v.nodes[node];
        if (!hash) {
          // the topic equal to the prefix, if stored
          bool e = act && (nd.word & RET_ENDS);
          if (e && (v.flags & RET_HAS_EXPIRY)) {
            const uint64_t x = v.expiry[nd.topic_lo];
            e = x == 0 || x > now;
          }
          const uint64_t m = __ballot(e);
          if (e && fill) {
            const uint64_t o = row_at + total + lanes_below(m, lane);
            if (o < row_end) out_ids[o] = v.ids[nd.topic_lo];
          }
          total += __popcll(m);
        } else {
          // every topic under each node, PER NODE: shallower topics lie between two
          // subtrees of one level.  Adjacent lanes whose rank ranges touch are one run.
          const uint32_t prev_hi = __shfl_up(nd.topic_hi, 1, 64);
          const bool head = act && (lane == 0 || nd.topic_lo != prev_hi);
          uint64_t hm = __ballot(head);
          while (hm) {
            const uint32_t h = __ffsll((unsigned long long)hm) - 1;
            hm &= hm - 1;
            const uint32_t h2 = hm ? uint32_t(__ffsll((unsigned long long)hm) - 1) : T;
            const uint32_t rlo = __shfl(nd.topic_lo, int(h), 64), rhi = __shfl(nd.topic_hi, int(h2 - 1), 64);
            emit_range(v, rlo, rhi, now, fill != 0, out_ids, row_at, row_end, total, lane);
          }
        }
        wave_sync();
      }
    }
    if (!fill && lane == 0) row_len[f] = total;
  }
}

// One lane per topic: the topic walked as an all-literal filter ('+' and '#'
// are ordinary words of a stored topic); the stored ones get their new expiry.
__global__ __launch_bounds__(256) void k_ret_expire(RetView v, const uint8_t* __restrict__ tb,
                                                    const uint64_t* __restrict__ to, uint64_t n,
                                                    const uint64_t* __restrict__ expiry,
                                                    unsigned long long* n_found) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool found = false;
  if (i < n) {
    const uint8_t* p = tb + to[i];
    const uint32_t len = uint32_t(to[i + 1] - to[i]);
    uint32_t node = 0, s = 0;
    for (uint32_t e = 0; e <= len && node != NONE; ++e)
      if (e == len || p[e] == '/') {
        const uint32_t w = dict_find<true>(v.words, p + s, e - s);
        node = w == NONE ? NONE : ret_child(v, node, w);
        s = e + 1;
      }
    if (node != NONE) {
      const RetNode nd = v.nodes[node];
      if (nd.word & RET_ENDS) {
        v.expiry[nd.topic_lo] = expiry[i];
        found = true;
      }
    }
  }
  const uint64_t m = __ballot(found);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_found, (unsigned long long)__popcll(m));
}

}  // namespace

int ret_upload(emqx_gm_ctx* ctx, emqx_gm_retained* r) {
  if (const int rc = table_upload(ctx, r->blob, r->bytes, "retained_build", &r->dev_base)) return rc;
  const RetView& h = r->hv;
  const void* hb = r->blob.data();
  void* db = r->dev_base;
  r->dv.nodes = rebase(h.nodes, hb, db);
  r->dv.depth_ends = rebase(h.depth_ends, hb, db);
  r->dv.words = DictView{rebase(h.words.dict, hb, db), rebase(h.words.word_off, hb, db), rebase(h.words.arena, hb, db),
                         h.words.dict_mask};
  r->dv.ids = rebase(h.ids, hb, db);
  r->dv.expiry = rebase(h.expiry, hb, db);
  r->device = ctx->device;
  r->info.device_bytes = r->bytes;
  if (!r->info.lds_frames) {
    const uint64_t wave_bytes = uint64_t(ret_wave_words(r->hv.depth_max)) * 4;
    const uint64_t blocks =
        std::max<uint64_t>(1, std::min<uint64_t>(1024, RET_WS_BUDGET / (wave_bytes * RET_WAVES_PER_BLOCK)));
    r->info.walk_ws_bytes = blocks * RET_WAVES_PER_BLOCK * wave_bytes;
  }
  return EMQX_GM_OK;
}

void ret_free_device(emqx_gm_retained* r) {
  table_free(r->device, r->dev_base);  // (waits for the device: no queued walk still reads the tables)
  r->dev_base = nullptr;
}

int ret_match_device(emqx_gm_ctx* ctx, emqx_gm_retained* r, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                     uint64_t now, bool timed, emqx_gm_csr* out) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t nbytes = n ? fo[n] : 0;
  auto* h_ro = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8));
  if (!h_ro) return set_err(ctx, EMQX_GM_ENOMEM, "retained_match: result offsets");
  out->priv = ctx;  // the owning context (emqx_gm_csr_free checks it)
  out->row_off = h_ro;
  out->n_rows = n;
  h_ro[0] = 0;
  if (!n) return EMQX_GM_OK;
  struct Undo {  // a failing call hands back no buffers
    emqx_gm_ctx* c;
    emqx_gm_csr* o;
    bool armed = true;
    ~Undo() {
      if (!armed) return;
      c->hpool->release(o->row_off);
      c->hpool->release(o->ids);
      *o = emqx_gm_csr{};
    }
  } undo{ctx, out};
  // the walk's grid: one wave per filter, capped; the global-workspace branch also by its budget
  const uint32_t wave_words = ret_wave_words(r->hv.depth_max);
  const bool gws = !r->info.lds_frames;
  uint64_t blocks = std::min<uint64_t>(1024, (n + RET_WAVES_PER_BLOCK - 1) / RET_WAVES_PER_BLOCK);
  if (gws)
    blocks = std::min<uint64_t>(blocks, r->info.walk_ws_bytes / (uint64_t(wave_words) * 4 * RET_WAVES_PER_BLOCK));
  PoolBuf d_fb(ctx->pool, nbytes + 64), d_fo(ctx->pool, (n + 1) * 8), d_len(ctx->pool, n * 8),
      d_ro(ctx->pool, (n + 1) * 8), d_ws;
  if (gws) d_ws = PoolBuf(ctx->pool, blocks * RET_WAVES_PER_BLOCK * uint64_t(wave_words) * 4);
  if (!d_fb.p || !d_fo.p || !d_len.p || !d_ro.p || (gws && !d_ws.p))
    return set_err(ctx, EMQX_GM_ENOMEM, "retained_match: device buffers");
  // the filters' offsets rebased to the copied bytes
  std::vector<uint64_t> off(n + 1);
  for (uint64_t i = 0; i <= n; ++i) off[i] = fo[i] - fo[0];
  if (nbytes - fo[0]) GM_HIP(ctx, hipMemcpyAsync(d_fb.p, fb + fo[0], nbytes - fo[0], hipMemcpyHostToDevice, st));
  GM_HIP(ctx, hipMemcpyAsync(d_fo.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  EventSet<4> ev;
  if (timed)
    if (const int rc = ev.create(ctx)) return rc;
  const size_t lds = gws ? 0 : size_t(wave_words) * 4 * RET_WAVES_PER_BLOCK;
  auto walk = [&](int fill, uint32_t* d_ids) {
    if (gws)
      hipLaunchKernelGGL(k_ret_walk<true>, dim3(uint32_t(blocks)), dim3(RET_WAVES_PER_BLOCK * 64), 0, st, r->dv,
                         d_fb.as<uint8_t>(), d_fo.as<uint64_t>(), n, now, fill, d_len.as<uint64_t>(),
                         d_ro.as<uint64_t>(), d_ids, d_ws.as<uint32_t>(), wave_words);
    else
      hipLaunchKernelGGL(k_ret_walk<false>, dim3(uint32_t(blocks)), dim3(RET_WAVES_PER_BLOCK * 64), lds, st, r->dv,
                         d_fb.as<uint8_t>(), d_fo.as<uint64_t>(), n, now, fill, d_len.as<uint64_t>(),
                         d_ro.as<uint64_t>(), d_ids, static_cast<uint32_t*>(nullptr), wave_words);
  };
  if (ev.on) GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  walk(0, nullptr);
  GM_HIP(ctx, hipGetLastError());
  if (ev.on) GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  if (const int rc = scan_lengths(ctx, d_len.as<uint64_t>(), n, d_ro.as<uint64_t>())) return rc;
  if (ev.on) GM_HIP(ctx, hipEventRecord(ev.e[2], st));
  GM_HIP(ctx, hipMemcpyAsync(h_ro, d_ro.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  const uint64_t nnz = h_ro[n];
  out->nnz = nnz;
  if (nnz) {
    auto* h_ids = static_cast<uint32_t*>(ctx->hpool->alloc(nnz * 4));
    out->ids = h_ids;
    PoolBuf d_ids(ctx->pool, nnz * 4);
    if (!h_ids || !d_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "retained_match: result ids");
    walk(1, d_ids.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
    if (ev.on) GM_HIP(ctx, hipEventRecord(ev.e[3], st));
    GM_HIP(ctx, hipMemcpyAsync(h_ids, d_ids.p, nnz * 4, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipStreamSynchronize(st));
  } else if (ev.on) {
    GM_HIP(ctx, hipEventRecord(ev.e[3], st));
    GM_HIP(ctx, hipStreamSynchronize(st));
  }
  if (ev.on) {
    for (int k = 0; k < 3; ++k) {
      float ms = 0;
      GM_HIP(ctx, hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
      r->last_ms[k] = ms;
    }
  }
  undo.armed = false;
  return EMQX_GM_OK;
}

int ret_expire_device(emqx_gm_ctx* ctx, emqx_gm_retained* r, const uint8_t* tb, const uint64_t* to, uint64_t n,
                      const uint64_t* expiry, uint64_t* n_found) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t nbytes = to[n] - to[0];
  PoolBuf d_tb(ctx->pool, nbytes + 64), d_to(ctx->pool, (n + 1) * 8), d_ex(ctx->pool, n * 8), d_cnt(ctx->pool, 16);
  if (!d_tb.p || !d_to.p || !d_ex.p || !d_cnt.p) return set_err(ctx, EMQX_GM_ENOMEM, "retained_expire: device buffers");
  std::vector<uint64_t> off(n + 1);
  for (uint64_t i = 0; i <= n; ++i) off[i] = to[i] - to[0];
  if (nbytes) GM_HIP(ctx, hipMemcpyAsync(d_tb.p, tb + to[0], nbytes, hipMemcpyHostToDevice, st));
  GM_HIP(ctx, hipMemcpyAsync(d_to.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  GM_HIP(ctx, hipMemcpyAsync(d_ex.p, expiry, n * 8, hipMemcpyHostToDevice, st));
  GM_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, 8, st));
  hipLaunchKernelGGL(k_ret_expire, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, st, r->dv, d_tb.as<uint8_t>(),
                     d_to.as<uint64_t>(), n, d_ex.as<uint64_t>(), d_cnt.as<unsigned long long>());
  GM_HIP(ctx, hipGetLastError());
  uint64_t found = 0;
  GM_HIP(ctx, hipMemcpyAsync(&found, d_cnt.p, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  *n_found = found;
  return EMQX_GM_OK;
}

}  // namespace gm
