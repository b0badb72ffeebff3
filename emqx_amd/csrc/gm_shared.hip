// gm_shared.hip — gfx950 kernels of the shared-subscription pick and the device
// entry points (layout, mix functions and the chunk rule: gm_shared.h; the
// reference path it replaces: emqx_shared_sub:dispatch/3's pick/6 ..
// do_pick_subscriber/6, apps/emqx/src/emqx_shared_sub.erl:234-288).
//
// A call runs on the context stream:
//   enumerate  k_sh_count (one lane per matched id: its slot count), the
//              library's scan (hit offsets), k_sh_rowoff (output row offsets);
//   expand     k_sh_expand (one lane per matched id): the slot of each of its
//              hits, and for hash / sticky / random the picked member;
//   round robin only, over the flat hit array in batch order, cut into C
//   chunks of L consecutive hits:
//     k_sh_hist    every hit counted into hist[chunk][slot] (integer atomics);
//     k_sh_column  one lane per slot: the exclusive prefix over the C rows in
//                  place, as "next member index" (first + hits before, mod
//                  Count), and the slot's new rr;
//     k_sh_rank    one wave per chunk walks its hits 64 at a time in order; a
//                  lane's rank among the equal-slot lanes below it comes from a
//                  ballot loop over the step's distinct slots; the chunk's
//                  running index lives in its own hist row.
// No workgroup waits on another: every dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_device.h"
#include "gm_shared.h"

namespace gm {
namespace {

// nnz_p (optional, speculative rows: nnz is their capacity): the rows' own count
// on the device; an entry past it counts 0 (the buffer holds stale words there)
__global__ __launch_bounds__(256) void k_sh_count(ShView v, const uint32_t* __restrict__ ids, uint64_t nnz,
                                                  const uint64_t* __restrict__ nnz_p, uint64_t* __restrict__ cnt) {
  const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= nnz) return;
  if (nnz_p && j >= *nnz_p) {
    cnt[j] = 0;
    return;
  }
  const uint32_t f = ids[j];
  cnt[j] = f < v.n_filters ? v.sh_off[f + 1] - v.sh_off[f] : 0;  // (an id past the snapshot is skipped)
}

// out[r] = the hit offset at the row's first matched id, r = 0 .. n_rows
__global__ __launch_bounds__(256) void k_sh_rowoff(const uint64_t* __restrict__ m_ro, uint64_t n_rows, uint64_t nnz,
                                                   const uint64_t* __restrict__ hoff, uint64_t* __restrict__ out,
                                                   uint64_t* __restrict__ out2) {
  const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r > n_rows) return;
  const uint64_t at = m_ro[r];
  const uint64_t x = hoff[at < nnz ? at : nnz];  // (a device row offset past the ids is clamped)
  out[r] = x;
  if (out2) out2[r] = x;
}

__global__ __launch_bounds__(256) void k_sh_expand(ShView v, const uint64_t* __restrict__ m_ro, uint64_t n_rows,
                                                   const uint32_t* __restrict__ ids, uint64_t nnz,
                                                   const uint64_t* __restrict__ hoff, uint64_t hits, uint32_t strategy,
                                                   const uint32_t* __restrict__ msg_hash, uint32_t seed,
                                                   uint32_t* __restrict__ out_slots,
                                                   uint32_t* __restrict__ out_members,
                                                   uint32_t* st_out, const uint32_t* __restrict__ win_row0,
                                                   uint32_t n_win) {
  const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= nnz) return;
  const uint32_t f = ids[j];
  if (f >= v.n_filters) return;
  const uint32_t s0 = v.sh_off[f], s1 = v.sh_off[f + 1];
  uint64_t h = hoff[j];
  if (s0 == s1 || hoff[j + 1] == h) return;  // (no hit counted: no slot, or an entry past speculative rows' count)
  uint64_t row = 0;
  if (strategy == EMQX_GM_SHARE_HASH || strategy == EMQX_GM_SHARE_RANDOM) {
    // the row of matched id j: the last r < n_rows with m_ro[r] <= j
    uint64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (m_ro[mid] <= j) lo = mid;
      else hi = mid;
    }
    row = lo;
    // a group of windows (gm_publish.hip): random's row is the message's row in its OWN window --
    // the last window w with win_row0[w] <= row (windows without a topic repeat a first row)
    if (win_row0 && strategy == EMQX_GM_SHARE_RANDOM) {
      uint32_t a = 0, b = n_win;
      while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (win_row0[mid] <= row) a = mid;
        else b = mid;
      }
      row -= win_row0[a];
    }
  }
  for (uint32_t s = s0; s < s1 && h < hits; ++s, ++h) {
    out_slots[h] = s;
    if (strategy == EMQX_GM_SHARE_ROUND_ROBIN) continue;  // (k_sh_rank writes the members)
    const uint32_t m0 = v.mem_off[s], count = v.mem_off[s + 1] - m0;
    uint32_t got;
    if (strategy == EMQX_GM_SHARE_STICKY) {
      got = v.st[s];
      if (got == SH_UNSET) {  // every hit of the slot computes the same value: identical plain stores
        got = v.mem_ids[m0 + (count == 1 ? 0 : sh_mix(seed, s) % count)];
        st_out[s] = got;  // (the table's st, or a speculative window's shadow of it)
      }
    } else if (count == 1) {
      got = v.mem_ids[m0];
    } else if (strategy == EMQX_GM_SHARE_HASH) {
      got = v.mem_ids[m0 + msg_hash[row] % count];
    } else {
      got = v.mem_ids[m0 + sh_mix3(seed, uint32_t(row), s) % count];
    }
    out_members[h] = got;
  }
}

__global__ __launch_bounds__(256) void k_sh_hist(const uint32_t* __restrict__ slots, uint64_t hits, uint64_t chunk_len,
                                                 uint32_t n_slots, uint32_t* __restrict__ hist) {
  const uint64_t h = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (h >= hits) return;
  const uint32_t s = slots[h];
  if (s >= n_slots) return;
  atomicAdd(&hist[(h / chunk_len) * uint64_t(n_slots) + s], 1u);
}

// One lane per slot (coalesced across slots): hist[c][s] becomes the member
// index the chunk's first hit on s takes, (first + hits of s in chunks < c) rem
// Count, and rr[s] the index of the call's last hit on s.
// rr_out: the table's rr, or a speculative window's shadow of it.
__global__ __launch_bounds__(256) void k_sh_column(ShView v, uint32_t* __restrict__ hist, uint32_t n_chunks,
                                                   uint32_t seed, uint32_t* rr_out) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= v.n_slots) return;
  const uint32_t count = v.mem_off[s + 1] - v.mem_off[s];
  const uint32_t old = v.rr[s];
  const uint32_t first =
      count <= 1 ? 0 : (old == SH_UNSET ? sh_mix(seed, s) % count : uint32_t((uint64_t(old) + 1) % count));
  uint64_t next = first;  // < count
  bool any = false;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    uint32_t* p = hist + uint64_t(c) * v.n_slots + s;
    const uint32_t t = *p;
    *p = uint32_t(next);
    any |= t != 0;
    if (count > 1) next = (next + t) % count;
  }
  // next is the index after the last hit; a slot of one member reads and writes no state
  if (any && count > 1) rr_out[s] = uint32_t((next + count - 1) % count);
}

// A speculative window's state made the table's (gm_publish.hip): the slots its
// shadow arrays hold a value for, one lane per slot.
__global__ __launch_bounds__(256) void k_sh_commit(uint32_t* __restrict__ rr, const uint32_t* __restrict__ sh_rr,
                                                   uint32_t* __restrict__ st, const uint32_t* __restrict__ sh_st,
                                                   uint32_t n_slots) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  if (sh_rr && sh_rr[s] != SH_UNSET) rr[s] = sh_rr[s];
  if (sh_st && sh_st[s] != SH_UNSET) st[s] = sh_st[s];
}

__global__ __launch_bounds__(64) void k_sh_rank(ShView v, const uint32_t* __restrict__ slots, uint64_t hits,
                                                uint64_t chunk_len, uint32_t* __restrict__ hist,
                                                uint32_t* __restrict__ out_members) {
  const uint32_t lane = threadIdx.x;
  const uint64_t begin = uint64_t(blockIdx.x) * chunk_len;
  const uint64_t end = begin + chunk_len < hits ? begin + chunk_len : hits;
  uint32_t* row = hist + uint64_t(blockIdx.x) * v.n_slots;  // only this wave touches it
  for (uint64_t base = begin; base < end; base += 64) {
    const uint64_t h = base + lane;
    uint32_t s = SH_UNSET;
    if (h < end) s = slots[h];
    const bool active = s < v.n_slots;
    uint32_t rank = 0, n = 0;
    uint64_t todo = __ballot(active);
    while (todo) {  // one round per distinct slot of the step
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint32_t ls = __shfl(s, leader);
      const uint64_t m = __ballot(active && s == ls);
      if (active && s == ls) {
        rank = __popcll(m & ((1ull << lane) - 1ull));
        n = __popcll(m);
      }
      todo &= ~m;
    }
    uint32_t m0 = 0, count = 1, next = 0;
    if (active) {
      m0 = v.mem_off[s];
      count = v.mem_off[s + 1] - m0;
      next = row[s];
    }
    wave_sync();  // every lane has read the row before any lane writes it
    if (active) {
      out_members[h] = v.mem_ids[m0 + uint32_t((uint64_t(next) + rank) % count)];
      if (rank == 0) row[s] = uint32_t((uint64_t(next) + n) % count);
    }
    wave_sync();  // the next step's lanes see this step's writes
  }
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + 255) / 256); }

}  // namespace

int sh_upload(emqx_gm_ctx* ctx, emqx_gm_shared* sh) {
  if (const int rc = table_upload(ctx, sh->blob, sh->bytes, "shared_build", &sh->dev_base)) return rc;
  const ShView& h = sh->hv;
  const void* hb = sh->blob.data();
  void* db = sh->dev_base;
  sh->dv.sh_off = rebase(h.sh_off, hb, db);
  sh->dv.mem_off = rebase(h.mem_off, hb, db);
  sh->dv.filter = rebase(h.filter, hb, db);
  sh->dv.group = rebase(h.group, hb, db);
  sh->dv.mem_ids = rebase(h.mem_ids, hb, db);
  sh->dv.rr = rebase(h.rr, hb, db);
  sh->dv.st = rebase(h.st, hb, db);
  sh->device = ctx->device;
  sh->info.device_bytes = sh->bytes;
  return EMQX_GM_OK;
}

void sh_free_device(emqx_gm_shared* sh) {
  table_free(sh->device, sh->dev_base);  // (waits for the device: no queued pick still reads the tables)
  sh->dev_base = nullptr;
}

int sh_read_state(emqx_gm_ctx* ctx, const emqx_gm_shared* sh, std::vector<uint32_t>& rr, std::vector<uint32_t>& st) {
  const uint64_t S = sh->hv.n_slots;
  rr.assign(S + 1, SH_UNSET);
  st.assign(S + 1, SH_UNSET);
  if (!sh->dev_base) {
    std::copy(sh->hv.rr, sh->hv.rr + S, rr.begin());
    std::copy(sh->hv.st, sh->hv.st + S, st.begin());
    return EMQX_GM_OK;
  }
  if (!S) return EMQX_GM_OK;
  GM_HIP(ctx, hipSetDevice(ctx->device));
  GM_HIP(ctx, hipMemcpyAsync(rr.data(), sh->dv.rr, S * 4, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(ctx, hipMemcpyAsync(st.data(), sh->dv.st, S * 4, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (stream order: after every queued pick)
  return EMQX_GM_OK;
}

int sh_pick_device(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy,
                   const uint32_t* msg_hash, uint32_t seed, uint32_t n_chunks, emqx_gm_csr* out_members,
                   emqx_gm_csr* out_slots, bool host_out, uint32_t* waits, const uint32_t* d_win_row0, uint32_t n_win) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // (host_out: device rows, but host hashes and a host result -- a publish window's rerun, gm_publish.hip)
  const bool dev_in = m->on_device != 0, dev = dev_in && !host_out;
  auto waited = [&]() {
    if (waits) ++*waits;
  };
  const uint64_t n = m->n_rows, nnz = m->nnz;
  emqx_gm_csr* outs[2] = {out_members, out_slots};
  struct Undo {  // a failing call hands back no buffers
    emqx_gm_ctx* c;
    emqx_gm_csr** o;
    bool dev, armed = true;
    ~Undo() {
      if (!armed) return;
      for (int k = 0; k < 2; ++k) {
        if (dev) {
          hipStreamSynchronize(c->stream);  // (a queued kernel may still write them)
          c->pool->release(o[k]->row_off);
          c->pool->release(o[k]->ids);
        } else {
          c->hpool->release(o[k]->row_off);
          c->hpool->release(o[k]->ids);
        }
        *o[k] = emqx_gm_csr{};
      }
    }
  } undo{ctx, outs, dev};
  for (emqx_gm_csr* o : outs) {
    o->priv = ctx;  // the owning context (emqx_gm_csr_free checks it)
    o->n_rows = n;
    o->on_device = dev ? 1 : 0;
    o->row_off = static_cast<uint64_t*>(dev ? ctx->pool->alloc((n + 1) * 8) : ctx->hpool->alloc((n + 1) * 8));
    if (!o->row_off) return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: result offsets");
  }
  if (!nnz || !n || !sh->hv.n_slots) {  // no hit
    for (emqx_gm_csr* o : outs) {
      if (dev) GM_HIP(ctx, hipMemsetAsync(o->row_off, 0, (n + 1) * 8, st));
      else std::fill(o->row_off, o->row_off + n + 1, uint64_t(0));
    }
    if (dev) {
      GM_HIP(ctx, hipStreamSynchronize(st));
      waited();
    }
    undo.armed = false;
    return EMQX_GM_OK;
  }
  // the rows (and hashes) on the device
  PoolBuf b_ro, b_ids, b_hash;
  const uint64_t* d_mro = m->row_off;
  const uint32_t* d_mids = m->ids;
  const uint32_t* d_hash = msg_hash;
  const bool need_hash = strategy == EMQX_GM_SHARE_HASH;
  if (!dev_in) {
    b_ro = PoolBuf(ctx->pool, (n + 1) * 8);
    b_ids = PoolBuf(ctx->pool, nnz * 4);
    if (!b_ro.p || !b_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: device buffers");
    GM_HIP(ctx, hipMemcpyAsync(b_ro.p, m->row_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_ids.p, m->ids, nnz * 4, hipMemcpyHostToDevice, st));
    d_mro = b_ro.as<uint64_t>();
    d_mids = b_ids.as<uint32_t>();
  }
  if (!dev) {
    if (need_hash) {
      b_hash = PoolBuf(ctx->pool, n * 4);
      if (!b_hash.p) return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: device buffers");
      GM_HIP(ctx, hipMemcpyAsync(b_hash.p, msg_hash, n * 4, hipMemcpyHostToDevice, st));
    }
    d_hash = need_hash ? b_hash.as<uint32_t>() : nullptr;
  }
  PoolBuf d_cnt(ctx->pool, nnz * 8), d_hoff(ctx->pool, (nnz + 1) * 8), d_ro;
  if (!dev) d_ro = PoolBuf(ctx->pool, (n + 1) * 8);
  if (!d_cnt.p || !d_hoff.p || (!dev && !d_ro.p)) return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: device buffers");
  EventSet<5> ev;
  if (const int rc = ev.create(ctx)) return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  // enumerate
  hipLaunchKernelGGL(k_sh_count, dim3(blocks_of(nnz)), dim3(256), 0, st, sh->dv, d_mids, nnz,
                     static_cast<const uint64_t*>(nullptr), d_cnt.as<uint64_t>());
  GM_HIP(ctx, hipGetLastError());
  if (const int rc = scan_lengths(ctx, d_cnt.as<uint64_t>(), nnz, d_hoff.as<uint64_t>())) return rc;
  uint64_t* ro_a = dev ? out_members->row_off : d_ro.as<uint64_t>();
  uint64_t* ro_b = dev ? out_slots->row_off : nullptr;
  hipLaunchKernelGGL(k_sh_rowoff, dim3(blocks_of(n + 1)), dim3(256), 0, st, d_mro, n, nnz, d_hoff.as<uint64_t>(), ro_a,
                     ro_b);
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  uint64_t hits = 0;
  GM_HIP(ctx, hipMemcpyAsync(&hits, d_hoff.as<uint64_t>() + nnz, 8, hipMemcpyDeviceToHost, st));
  if (!dev) GM_HIP(ctx, hipMemcpyAsync(out_members->row_off, d_ro.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  if (!dev) std::copy(out_members->row_off, out_members->row_off + n + 1, out_slots->row_off);
  if (hits >= 0xFFFFFFFFull) return set_err(ctx, EMQX_GM_EOVERFLOW, "shared_pick: 2^32 - 1 hits or more in one call");
  out_members->nnz = out_slots->nnz = hits;
  if (!hits) {
    undo.armed = false;
    return EMQX_GM_OK;
  }
  // the round-robin workspace, sized before anything changes state
  const uint64_t S = sh->hv.n_slots;
  uint32_t C = 1;
  uint64_t L = hits;
  PoolBuf d_hist;
  if (strategy == EMQX_GM_SHARE_ROUND_ROBIN) {
    C = n_chunks ? n_chunks : sh_rr_chunks(hits, S);
    C = uint32_t(std::min<uint64_t>(C, hits));
    if (uint64_t(C) * S * 4 > SH_RR_WS_CAP && C > 1)
      return set_err(ctx, EMQX_GM_EINVAL, "shared_pick: chunk count past the workspace cap");
    L = (hits + C - 1) / C;
    C = uint32_t((hits + L - 1) / L);
    d_hist = PoolBuf(ctx->pool, uint64_t(C) * S * 4);
    if (!d_hist.p) return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: round-robin workspace");
  }
  PoolBuf d_mem, d_slot;  // host rows: the device side of the two id arrays
  uint32_t *o_mem, *o_slot;
  if (dev) {
    out_members->ids = o_mem = static_cast<uint32_t*>(ctx->pool->alloc(hits * 4));
    out_slots->ids = o_slot = static_cast<uint32_t*>(ctx->pool->alloc(hits * 4));
  } else {
    d_mem = PoolBuf(ctx->pool, hits * 4);
    d_slot = PoolBuf(ctx->pool, hits * 4);
    o_mem = d_mem.as<uint32_t>();
    o_slot = d_slot.as<uint32_t>();
    out_members->ids = static_cast<uint32_t*>(ctx->hpool->alloc(hits * 4));
    out_slots->ids = static_cast<uint32_t*>(ctx->hpool->alloc(hits * 4));
  }
  if (!o_mem || !o_slot || !out_members->ids || !out_slots->ids)
    return set_err(ctx, EMQX_GM_ENOMEM, "shared_pick: result ids");
  // expand (and pick, but for round robin)
  hipLaunchKernelGGL(k_sh_expand, dim3(blocks_of(nnz)), dim3(256), 0, st, sh->dv, d_mro, n, d_mids, nnz,
                     d_hoff.as<uint64_t>(), hits, strategy, d_hash, seed, o_slot, o_mem, sh->dv.st, d_win_row0, n_win);
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipEventRecord(ev.e[2], st));
  if (strategy == EMQX_GM_SHARE_ROUND_ROBIN) {
    GM_HIP(ctx, hipMemsetAsync(d_hist.p, 0, uint64_t(C) * S * 4, st));
    hipLaunchKernelGGL(k_sh_hist, dim3(blocks_of(hits)), dim3(256), 0, st, o_slot, hits, L, uint32_t(S),
                       d_hist.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sh_column, dim3(blocks_of(S)), dim3(256), 0, st, sh->dv, d_hist.as<uint32_t>(), C, seed,
                       sh->dv.rr);
    GM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sh_rank, dim3(C), dim3(64), 0, st, sh->dv, o_slot, hits, L, d_hist.as<uint32_t>(), o_mem);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ev.e[3], st));
  if (!dev) {
    GM_HIP(ctx, hipMemcpyAsync(out_members->ids, o_mem, hits * 4, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipMemcpyAsync(out_slots->ids, o_slot, hits * 4, hipMemcpyDeviceToHost, st));
  }
  GM_HIP(ctx, hipEventRecord(ev.e[4], st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  // (a publish window's rerun of a stateless strategy does not hold sh->mu, which guards last_ms)
  for (int k = 0; k < 3 && !host_out; ++k) {
    float ms = 0;
    GM_HIP(ctx, hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
    sh->last_ms[k] = ms;
  }
  if (!host_out) {
    float ms = 0;
    GM_HIP(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[4]));
    sh->last_ms[3] = ms;
  }
  undo.armed = false;
  return EMQX_GM_OK;
}


// The pick of a small call's SPECULATIVE rows (gm_publish.hip), queued on the
// context stream with no wait and no read-back: the counts run over the ids'
// capacity `cap` with the rows' own count read on the device (d_ro + n), the
// expansion into cap_hits entries (slots pre-filled SH_UNSET, so the round-robin
// passes skip the unused ones; their chunking is fixed from cap_hits).  The
// table's state is read but not written: the new round-robin index and the
// first sticky pick go to shadow arrays (SH_UNSET: untouched) that
// sh_queue_commit applies once the host knows the run holds.  1: not queued
// (no room, or a workspace past the cap).
int sh_queue_spec(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_hits, uint32_t strategy, const uint32_t* d_hash, uint32_t seed,
                  ShSpec* out, const uint32_t* d_win_row0, uint32_t n_win) {
  hipStream_t st = ctx->stream;
  const uint64_t S = sh->hv.n_slots;
  if (!S || !cap || !cap_hits) return 1;  // (a table without slots: the exact call answers without device work)
  const bool rr = strategy == EMQX_GM_SHARE_ROUND_ROBIN, sticky = strategy == EMQX_GM_SHARE_STICKY;
  uint32_t C = 1;
  uint64_t L = cap_hits;
  if (rr) {
    C = uint32_t(std::min<uint64_t>(sh_rr_chunks(cap_hits, S), cap_hits));
    L = (cap_hits + C - 1) / C;
    C = uint32_t((cap_hits + L - 1) / L);
    if (uint64_t(C) * S * 4 > SH_RR_WS_CAP) return 1;
  }
  // one workspace: cnt | hoff | row offsets | slots | members | hist | shadow
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(std::max<size_t>(bytes, 16), 256);
    return at;
  };
  const size_t o_cnt = take(cap * 8), o_hoff = take((cap + 1) * 8), o_ro = take((n + 1) * 8);
  const size_t o_slot = take(cap_hits * 4), o_mem = take(cap_hits * 4);
  const size_t o_hist = rr ? take(uint64_t(C) * S * 4) : 0, o_sh = rr || sticky ? take(S * 4) : 0;
  uint8_t* w = static_cast<uint8_t*>(ctx->pool->alloc(o));
  if (!w) return 1;
  auto at = [&](size_t off) { return static_cast<void*>(w + off); };
  uint64_t* cnt = static_cast<uint64_t*>(at(o_cnt));
  uint64_t* hoff = static_cast<uint64_t*>(at(o_hoff));
  out->ws = w;
  out->row_off = static_cast<uint64_t*>(at(o_ro));
  out->slots = static_cast<uint32_t*>(at(o_slot));
  out->members = static_cast<uint32_t*>(at(o_mem));
  out->total = hoff + cap;
  out->sh_rr = rr ? static_cast<uint32_t*>(at(o_sh)) : nullptr;
  out->sh_st = sticky ? static_cast<uint32_t*>(at(o_sh)) : nullptr;
  auto fail = [&](int rc) {
    hipStreamSynchronize(st);  // (a queued kernel may still write the workspace)
    ctx->pool->release(w);
    *out = ShSpec{};
    return rc;
  };
#define SH_Q(expr)                                                                    \
  do {                                                                                \
    if ((expr) != hipSuccess) return fail(set_err(ctx, EMQX_GM_EDEVICE, "publish_window: " #expr)); \
  } while (0)
  SH_Q(hipMemsetAsync(out->slots, 0xFF, cap_hits * 4, st));
  if (rr || sticky) SH_Q(hipMemsetAsync(at(o_sh), 0xFF, S * 4, st));
  hipLaunchKernelGGL(k_sh_count, dim3(blocks_of(cap)), dim3(256), 0, st, sh->dv, d_ids, cap, d_ro + n, cnt);
  SH_Q(hipGetLastError());
  if (const int rc = scan_lengths(ctx, cnt, cap, hoff)) return fail(rc);
  hipLaunchKernelGGL(k_sh_rowoff, dim3(blocks_of(n + 1)), dim3(256), 0, st, d_ro, n, cap, hoff, out->row_off,
                     static_cast<uint64_t*>(nullptr));
  SH_Q(hipGetLastError());
  hipLaunchKernelGGL(k_sh_expand, dim3(blocks_of(cap)), dim3(256), 0, st, sh->dv, d_ro, n, d_ids, cap, hoff, cap_hits,
                     strategy, d_hash, seed, out->slots, out->members, out->sh_st, d_win_row0, n_win);
  SH_Q(hipGetLastError());
  if (rr) {
    uint32_t* hist = static_cast<uint32_t*>(at(o_hist));
    SH_Q(hipMemsetAsync(hist, 0, uint64_t(C) * S * 4, st));
    hipLaunchKernelGGL(k_sh_hist, dim3(blocks_of(cap_hits)), dim3(256), 0, st, out->slots, cap_hits, L, uint32_t(S), hist);
    SH_Q(hipGetLastError());
    hipLaunchKernelGGL(k_sh_column, dim3(blocks_of(S)), dim3(256), 0, st, sh->dv, hist, C, seed, out->sh_rr);
    SH_Q(hipGetLastError());
    hipLaunchKernelGGL(k_sh_rank, dim3(C), dim3(64), 0, st, sh->dv, out->slots, cap_hits, L, hist, out->members);
    SH_Q(hipGetLastError());
  }
#undef SH_Q
  return 0;
}

int sh_queue_commit(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const ShSpec& run) {
  const uint32_t S = sh->hv.n_slots;
  if (!S || (!run.sh_rr && !run.sh_st)) return 0;
  hipLaunchKernelGGL(k_sh_commit, dim3(blocks_of(S)), dim3(256), 0, ctx->stream, sh->dv.rr, run.sh_rr, sh->dv.st,
                     run.sh_st, S);
  GM_HIP(ctx, hipGetLastError());
  return 0;
}

}  // namespace gm

extern "C" {

int emqx_gm_shared_build(emqx_gm_ctx* ctx, emqx_gm_index* idx, const uint8_t* fb, const uint64_t* fo,
                         const uint32_t* group_ids, uint64_t n_slots, const uint64_t* mem_off,
                         const uint32_t* mem_ids, const emqx_gm_shared* prev, uint32_t flags, emqx_gm_shared** out) {
  if (!ctx || !out) return EMQX_GM_EINVAL;
  *out = nullptr;
  if (!idx) return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_build: NULL index");
  if (flags) return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_build: flags");
  if (idx->route || !idx->shards.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "shared_build: a sharded index");
  if (idx->view.gmap || !idx->gmap.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "shared_build: a shard index");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "shared_build: an overlay snapshot");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_build: the index is on another device");
  if (prev && prev->dev_base && prev->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_build: prev is on another device");
  GM_GUARD_BEGIN
  std::string why;
  // (prev is read, not modified; its lock -- taken before the context's, as a pick does -- keeps a
  // concurrent pick from queueing between the reads of its two state arrays)
  std::unique_lock<std::mutex> pl;
  if (prev) pl = std::unique_lock<std::mutex>(const_cast<emqx_gm_shared*>(prev)->mu);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  std::vector<uint32_t> prr, pst;
  if (prev)
    if (const int rc = gm::sh_read_state(ctx, prev, prr, pst)) return rc;
  auto resolve = [&](const uint8_t* p, uint64_t len, uint32_t* id) {
    bool found = false;
    const uint64_t r = gm::filter_rank(idx, p, len, &found);
    *id = uint32_t(r);
    return found;
  };
  const gm::ShInput in{fb, fo, group_ids, n_slots, mem_off, mem_ids};
  emqx_gm_shared* sh = nullptr;
  int rc = gm::sh_compile(in, idx->info.n_filters, resolve, prev, prev ? prr.data() : nullptr,
                          prev ? pst.data() : nullptr, &sh, &why);
  if (rc) return gm::set_err(ctx, rc, "shared_build: " + why);
  rc = gm::sh_upload(ctx, sh);
  if (rc) {
    delete sh;
    return rc;
  }
  emqx_gm_index_retain(idx);
  sh->idx = idx;
  *out = sh;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_shared_pick_chunked(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy,
                                const uint32_t* msg_hash, uint32_t seed, uint32_t n_chunks,
                                emqx_gm_csr* out_members, emqx_gm_csr* out_slots) {
  if (!ctx || !sh || !m || !out_members || !out_slots) return EMQX_GM_EINVAL;
  std::memset(out_members, 0, sizeof(*out_members));
  std::memset(out_slots, 0, sizeof(*out_slots));
  if (strategy > EMQX_GM_SHARE_RANDOM) return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_pick: strategy");
  if (!sh->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "shared_pick: a host-only table");
  if (sh->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_pick: the table is on another device");
  if (strategy == EMQX_GM_SHARE_HASH && !msg_hash && m->n_rows)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_pick: msg_hash is required for EMQX_GM_SHARE_HASH");
  if (n_chunks > gm::SH_RR_MAX_CHUNKS) return gm::set_err(ctx, EMQX_GM_EINVAL, "shared_pick: chunk count");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::sh_check_rows(sh, m, &why)) return gm::set_err(ctx, rc, "shared_pick: " + why);
  std::lock_guard<std::mutex> tl(sh->mu);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::sh_pick_device(ctx, sh, m, strategy, msg_hash, seed, n_chunks, out_members, out_slots, false, nullptr);
  GM_GUARD_END(ctx)
}

int emqx_gm_shared_pick(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy,
                        const uint32_t* msg_hash, uint32_t seed, emqx_gm_csr* out_members, emqx_gm_csr* out_slots) {
  return emqx_gm_shared_pick_chunked(ctx, sh, m, strategy, msg_hash, seed, 0, out_members, out_slots);
}

}  // extern "C"
