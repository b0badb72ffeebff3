// gm_batches.hip — gfx950 kernels of the session batches and the device entry
// points (semantics, the chunk rule: gm_batches.h; the reference path it
// replaces: every connection process draining its mailbox into one list,
// emqx_connection.erl:516-520, emqx_misc.erl:159-173, then ignore_local/4 and
// enrich_deliver/2 over it, emqx_channel.erl:830-842, emqx_session.erl:279-291).
//
// A call runs on the context stream:
//   count      gm_subopts.hip's k_so_seglen (FLAG form: segment lengths, the
//              hits) and the library's scan; one 8-byte read back gives the
//              pre-removal total T (2^32 - 1 or more: EMQX_GM_EOVERFLOW);
//   expand     k_sb_expand, k_so_copy's shape (every workgroup owns a fixed
//              range of deliveries, a thread moves 4): per delivery k its key
//              (the subscriber), val = k, and the payload row / filter / byte;
//   partition  a stable LSD radix partition of the (key, val) pairs, one pass
//              per 8-bit digit of the table's largest subscriber id, the pairs
//              ping-ponging between two workspaces; per pass over C chunks of
//              L consecutive pairs:
//     k_sb_hist     one block per chunk counts its digits in 256 LDS bins
//                   (integer atomics: the order is irrelevant) and stores its
//                   row hist[chunk][bin];
//     k_sb_column   one lane per bin: the exclusive prefix over the C rows in
//                   place, and the bin's total;
//     the library's scan over the totals: bin_off;
//     k_sb_scatter  one block per chunk keeps next[bin] = bin_off[bin] +
//                   hist[chunk][bin] in LDS and walks its pairs 256 at a time
//                   in order; a pair's rank among the equal-digit lanes below
//                   it comes from ballots over the 8 digit bits (lane order),
//                   and the block's four waves take their turns in wave order;
//   heads      a scan of the head flags (position 0, or the key changes) gives
//              every position's batch index; k_sb_heads writes each batch's
//              first position;
//   removal    LEAD: an exclusive scan P of the non-hit flags -- a hit at i of
//              the batch starting at s is in the leading run iff P[i] = P[s];
//              DROP and LEAD: a scan Q of the kept flags; one 16-byte read
//              back gives the batch count and the kept total;
//   emit       k_sb_batches (subs, batch_off, batch_dropped from the scans at
//              the heads) and k_sb_emit (rows, filters, bytes gathered through
//              val to Q's positions; LEAD clears bit 4).
// No arrival-order atomics, no workgroup waits on another: every dependency is
// a kernel boundary, and the result is the same whatever C is.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_batches.h"
#include "gm_device.h"
#include "gm_scan.h"

namespace gm {
namespace {

// the row of match entry j: the last r < n_rows with m_off[r] <= j (n_rows >= 1)
__device__ __forceinline__ uint64_t sb_row_of(const uint64_t* __restrict__ m_off, uint64_t n_rows, uint64_t j) {
  uint64_t lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (m_off[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// last segment in [a, b] whose start <= p
__device__ __forceinline__ uint64_t sb_seg(const uint64_t* __restrict__ seg_dst, uint64_t a, uint64_t b, uint64_t p) {
  if (a == b) return a;
  ++b;
  while (b - a > 1) {
    const uint64_t m = (a + b) >> 1;
    if (seg_dst[m] <= p) a = m;
    else b = m;
  }
  return a;
}

struct SbRows {  // the window on the device
  const uint64_t* seg_dst;  // [nseg + 1] the segments' first deliveries
  uint64_t nseg;
  const uint64_t* m_off;
  uint64_t n_rows;
  const uint32_t* m_ids;
  const uint32_t* seg_hit;
  const uint8_t* msg_flags;
};

struct SbExp {  // what the expansion writes, [T] each (opt with 16 B of slack)
  uint32_t *key, *val, *row, *fil;
  uint8_t* opt;
};

struct SbSeg {
  uint64_t dst, src;
  uint32_t hit, row, fil;
  uint8_t msg;
};
__device__ __forceinline__ SbSeg sb_seg_load(const SoView& v, const SbRows& w, uint64_t s) {
  SbSeg g;
  g.dst = w.seg_dst[s];
  g.fil = w.m_ids[s];
  g.src = v.sub_off[g.fil];  // (a segment that holds a delivery has an id of the snapshot)
  g.hit = w.seg_hit[s];
  g.row = uint32_t(sb_row_of(w.m_off, w.n_rows, s));
  g.msg = w.msg_flags[g.row] & 0x0Fu;
  return g;
}

// delivery q of segment g
__device__ __forceinline__ void sb_one(const SoView& v, const SbSeg& g, uint64_t q, const SbExp& o) {
  const uint64_t t = q - g.dst;
  o.key[q] = v.sub_ids[g.src + t];
  o.val[q] = uint32_t(q);
  o.row[q] = g.row;
  o.fil[q] = g.fil;
  o.opt[q] = uint8_t(so_byte(v.opt[g.src + t], g.msg) | (t == g.hit ? SO_HIT : 0));
}

// deliveries q .. q + 3, all of segment g; q is a multiple of 4
__device__ __forceinline__ void sb_four(const SoView& v, const SbSeg& g, uint64_t q, const SbExp& o) {
  const uint64_t t = q - g.dst, k = g.src + t, h = g.hit;
  uint32_t ow;
  __builtin_memcpy(&ow, v.opt + k, 4);  // (one dword load at any alignment)
  uint32_t w = so_byte4(ow, g.msg);
  if (g.hit != SO_NONE && h - t < 4) w |= uint32_t(SO_HIT) << (8 * (h - t));  // (h < t wraps far past 4)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o.key[q + e] = v.sub_ids[k + e];
    o.val[q + e] = uint32_t(q + e);
    o.row[q + e] = g.row;
    o.fil[q + e] = g.fil;
  }
  *reinterpret_cast<uint32_t*>(o.opt + q) = w;
}

// Every workgroup owns per_block (a multiple of 1,024) consecutive deliveries
// [lo, hi) of [0, total); a thread moves 4 at a time.
__global__ __launch_bounds__(256) void k_sb_expand(SoView v, SbRows w, uint64_t total, uint64_t per_block, SbExp o) {
  total = min(total, w.seg_dst[w.nseg]);  // (never past the device's own total)
  const uint64_t lo = uint64_t(blockIdx.x) * per_block;
  if (lo >= total) return;
  const uint64_t hi = min(total, lo + per_block);
  __shared__ uint64_t s_seg[2];
  if (threadIdx.x < 2) {
    // last segment whose start <= x (segments may be empty)
    const uint64_t x = threadIdx.x == 0 ? lo : hi - 1;
    uint64_t a = 0, b = w.nseg;  // seg_dst[a] <= x < seg_dst[b]
    while (b - a > 1) {
      const uint64_t m = (a + b) >> 1;
      if (w.seg_dst[m] <= x) a = m;
      else b = m;
    }
    s_seg[threadIdx.x] = a;
  }
  __syncthreads();
  const uint64_t s0 = s_seg[0], s1 = s_seg[1];
  for (uint64_t q = lo + uint64_t(threadIdx.x) * 4; q < hi; q += 256 * 4) {
    const uint64_t s = sb_seg(w.seg_dst, s0, s1, q);
    if (q + 4 <= hi && q + 4 <= w.seg_dst[s + 1]) {
      sb_four(v, sb_seg_load(v, w, s), q, o);
    } else {
      for (uint64_t p = q; p < q + 4 && p < hi; ++p) sb_one(v, sb_seg_load(v, w, sb_seg(w.seg_dst, s0, s1, p)), p, o);
    }
  }
}

// hist[chunk][bin] = the chunk's keys whose digit (key >> shift) & 255 is bin
__global__ __launch_bounds__(SB_BLOCK) void k_sb_hist(const uint32_t* __restrict__ key, uint64_t n, uint64_t chunk_len,
                                                      uint32_t shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[SB_BINS];
  s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t begin = uint64_t(blockIdx.x) * chunk_len;
  const uint64_t end = begin + chunk_len < n ? begin + chunk_len : n;
  for (uint64_t i = begin + threadIdx.x; i < end; i += SB_BLOCK) atomicAdd(&s_cnt[(key[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[uint64_t(blockIdx.x) * SB_BINS + threadIdx.x] = s_cnt[threadIdx.x];
}

// One lane per bin (coalesced across bins): hist[c][bin] becomes the pairs of
// the bin in chunks < c, total[bin] the bin's pairs.
__global__ __launch_bounds__(SB_BINS) void k_sb_column(uint32_t* __restrict__ hist, uint32_t n_chunks,
                                                       uint64_t* __restrict__ total) {
  const uint32_t bin = threadIdx.x;
  uint32_t sum = 0;  // (the call's deliveries are below 2^32 - 1)
  for (uint32_t c = 0; c < n_chunks; ++c) {
    uint32_t* p = hist + uint64_t(c) * SB_BINS + bin;
    const uint32_t t = *p;
    *p = sum;
    sum += t;
  }
  total[bin] = sum;
}

// One block per chunk: the pairs to their digit's bin, in lane, wave and chunk order.
__global__ __launch_bounds__(SB_BLOCK) void k_sb_scatter(const uint32_t* __restrict__ key_in,
                                                         const uint32_t* __restrict__ val_in, uint64_t n,
                                                         uint64_t chunk_len, uint32_t shift,
                                                         const uint32_t* __restrict__ hist,
                                                         const uint64_t* __restrict__ bin_off,
                                                         uint32_t* __restrict__ key_out,
                                                         uint32_t* __restrict__ val_out) {
  __shared__ uint32_t s_next[SB_BINS];  // where the bin's next pair of this chunk goes
  s_next[threadIdx.x] = uint32_t(bin_off[threadIdx.x]) + hist[uint64_t(blockIdx.x) * SB_BINS + threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t begin = uint64_t(blockIdx.x) * chunk_len;
  const uint64_t end = begin + chunk_len < n ? begin + chunk_len : n;
  for (uint64_t base = begin; base < end; base += SB_BLOCK) {  // (the trip count is the same for every thread)
    const uint64_t i = base + threadIdx.x;
    const bool active = i < end;
    uint32_t k = 0, x = 0;
    if (active) {
      k = key_in[i];
      x = val_in[i];
    }
    const uint32_t d = (k >> shift) & 255u;
    // the lanes of this wave holding the same digit: one ballot per bit
    uint64_t peers = __ballot(active);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const uint64_t set = __ballot(active && ((d >> b) & 1u));
      peers &= ((d >> b) & 1u) ? set : ~set;
    }
    const uint32_t rank = lanes_below(peers, lane), cnt = __popcll(peers);
    for (uint32_t w = 0; w < SB_BLOCK / 64; ++w) {  // the waves in order: wave w's pairs come before wave w + 1's
      if (wave == w) {
        uint32_t next = 0;
        if (active) next = s_next[d];
        wave_sync();  // every lane has read its slot before a leader writes it
        if (active) {
          const uint32_t pos = next + rank;
          if (pos < n) {
            key_out[pos] = k;
            val_out[pos] = x;
          }
          if (rank == 0) s_next[d] = next + cnt;
        }
      }
      __syncthreads();
    }
  }
}

// position i of the sorted order starts a batch iff i = 0 or the key changes
struct LoadHead {
  const uint32_t* key;
  __device__ uint64_t operator()(uint64_t i) const { return (i == 0 || key[i] != key[i - 1]) ? 1 : 0; }
};
struct LoadNonHit {
  const uint32_t* val;
  const uint8_t* opt;
  __device__ uint64_t operator()(uint64_t i) const { return (opt[val[i]] & SO_HIT) ? 0 : 1; }
};
// !remove: E the heads' scan (E[i + 1] - 1 is i's batch), first the batches' first positions
struct LoadKeep {
  const uint32_t* val;
  const uint8_t* opt;
  const uint64_t *E, *first, *P;
  bool lead;
  __device__ uint64_t operator()(uint64_t i) const {
    if (!(opt[val[i]] & SO_HIT)) return 1;
    if (!lead) return 0;
    return P[i] != P[first[E[i + 1] - 1]] ? 1 : 0;  // a non-hit lies between the head and i: dropwhile has stopped
  }
};

// first[j] = batch j's first position of the sorted order; first[n_batches] = n (cap: first's entries - 1)
__global__ __launch_bounds__(256) void k_sb_heads(const uint32_t* __restrict__ key, const uint64_t* __restrict__ E,
                                                  uint64_t n, uint64_t cap, uint64_t* __restrict__ first) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0 || key[i] != key[i - 1]) {
    const uint64_t j = E[i];
    if (j < cap) first[j] = i;
  }
  if (i == n - 1 && E[n] <= cap) first[E[n]] = n;
}

// one lane per batch (and one for the closing offset); Q: the kept flags' scan (nullptr: nothing is removed)
__global__ __launch_bounds__(256) void k_sb_batches(const uint32_t* __restrict__ key, const uint64_t* __restrict__ first,
                                                    const uint64_t* __restrict__ Q, uint64_t n_batches, uint64_t n,
                                                    uint32_t* __restrict__ subs, uint64_t* __restrict__ batch_off,
                                                    uint32_t* __restrict__ batch_dropped) {
  const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j > n_batches) return;
  if (j == n_batches) {
    batch_off[j] = Q ? Q[n] : n;
    return;
  }
  const uint64_t s = min(first[j], n - 1), e = min(first[j + 1], n);
  subs[j] = key[s];
  batch_off[j] = Q ? Q[s] : s;
  if (batch_dropped) batch_dropped[j] = uint32_t((e - s) - (Q[e] - Q[s]));
}

// one lane per position of the sorted order: the kept deliveries' payload to its place
__global__ __launch_bounds__(256) void k_sb_emit(const uint32_t* __restrict__ val, const uint32_t* __restrict__ h_row,
                                                 const uint32_t* __restrict__ h_fil, const uint8_t* __restrict__ h_opt,
                                                 const uint64_t* __restrict__ Q, uint64_t n, uint64_t kept,
                                                 uint8_t mask, uint32_t* __restrict__ rows,
                                                 uint32_t* __restrict__ filters, uint8_t* __restrict__ dopt) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t o = i;
  if (Q) {
    o = Q[i];
    if (Q[i + 1] == o) return;  // removed
  }
  if (o >= kept) return;
  const uint32_t k = val[i];
  rows[o] = h_row[k];
  filters[o] = h_fil[k];
  dopt[o] = h_opt[k] & mask;
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + 255) / 256); }

void* const* sb_ptrs(emqx_gm_batches* b, void** ps) {
  ps[0] = b->subs, ps[1] = b->batch_off, ps[2] = b->rows, ps[3] = b->filters, ps[4] = b->dopt, ps[5] = b->batch_dropped;
  return ps;
}

struct SbUndo {  // a failing call hands back no buffers
  emqx_gm_ctx* c;
  emqx_gm_batches* o;
  bool dev, armed = true;
  ~SbUndo() {
    if (!armed) return;
    void* ps[6];
    sb_ptrs(o, ps);
    if (dev) hipStreamSynchronize(c->stream);  // (a queued kernel may still write them)
    for (void* p : ps) {
      if (!p) continue;
      if (dev) c->pool->release(p);
      else c->hpool->release(p);
    }
    *o = emqx_gm_batches{};
  }
};

}  // namespace

int sb_batches_device(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                      const uint32_t* msg_from, uint32_t mode, uint32_t n_chunks, emqx_gm_batches* out) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool dev = m->on_device != 0, flag = mode == EMQX_GM_SO_FLAG, lead = mode == EMQX_GM_SO_LEAD;
  struct Waits {  // the call's host-blocking waits, left with the table however the call ends
    emqx_gm_subopts* so;
    uint32_t n = 0;
    ~Waits() {
      std::lock_guard<std::mutex> lk(so->mu);
      so->sb_ms[6] = n;
    }
  } waits{so};
  auto waited = [&]() { ++waits.n; };
  const uint64_t n = m->n_rows, nnz = m->nnz;
  auto res_alloc = [&](size_t bytes) -> void* {
    bytes = std::max<size_t>(bytes, 16);
    return dev ? ctx->pool->alloc(bytes) : ctx->hpool->alloc(bytes);
  };
  emqx_gm_batches res{};  // (the caller's struct is written only on success)
  SbUndo undo{ctx, &res, dev};
  res.priv = ctx;  // the owning context (emqx_gm_batches_free checks it)
  res.n_rows = n;
  res.on_device = dev ? 1 : 0;
  // the result's arrays for nb batches of `kept` deliveries
  auto res_arrays = [&](uint64_t nb, uint64_t kept) -> int {
    res.n_batches = nb;
    res.n_deliveries = kept;
    res.subs = static_cast<uint32_t*>(res_alloc(nb * 4));
    res.batch_off = static_cast<uint64_t*>(res_alloc((nb + 1) * 8));
    res.rows = static_cast<uint32_t*>(res_alloc(kept * 4));
    res.filters = static_cast<uint32_t*>(res_alloc(kept * 4));
    res.dopt = static_cast<uint8_t*>(res_alloc(kept));
    if (!flag) res.batch_dropped = static_cast<uint32_t*>(res_alloc(nb * 4));
    if (!res.subs || !res.batch_off || !res.rows || !res.filters || !res.dopt || (!flag && !res.batch_dropped))
      return set_err(ctx, EMQX_GM_ENOMEM, "deliver_batches: result arrays");
    return EMQX_GM_OK;
  };
  auto no_batches = [&]() -> int {
    if (const int rc = res_arrays(0, 0)) return rc;
    if (dev) {
      GM_HIP(ctx, hipMemsetAsync(res.batch_off, 0, 8, st));
      GM_HIP(ctx, hipStreamSynchronize(st));
      waited();
    } else {
      res.batch_off[0] = 0;
    }
    undo.armed = false;
    *out = res;
    return EMQX_GM_OK;
  };
  if (!n || !nnz || !so->hv.n_subs) return no_batches();  // no delivery at all
  // the rows and the messages on the device
  PoolBuf b_ro, b_ids, b_mf, b_from;
  const uint64_t* d_mro = m->row_off;
  const uint32_t* d_mids = m->ids;
  const uint8_t* d_mf = msg_flags;
  const uint32_t* d_from = msg_from;
  if (!dev) {
    b_ro = PoolBuf(ctx->pool, (n + 1) * 8);
    b_ids = PoolBuf(ctx->pool, nnz * 4);
    b_mf = PoolBuf(ctx->pool, n);
    b_from = PoolBuf(ctx->pool, n * 4);
    if (!b_ro.p || !b_ids.p || !b_mf.p || !b_from.p)
      return set_err(ctx, EMQX_GM_ENOMEM, "deliver_batches: device buffers");
    GM_HIP(ctx, hipMemcpyAsync(b_ro.p, m->row_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_ids.p, m->ids, nnz * 4, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_mf.p, msg_flags, n, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_from.p, msg_from, n * 4, hipMemcpyHostToDevice, st));
    d_mro = b_ro.as<uint64_t>();
    d_mids = b_ids.as<uint32_t>();
    d_mf = b_mf.as<uint8_t>();
    d_from = b_from.as<uint32_t>();
  }
  PoolBuf d_len(ctx->pool, nnz * 8), d_hit(ctx->pool, nnz * 4), d_dst(ctx->pool, (nnz + 1) * 8);
  if (!d_len.p || !d_hit.p || !d_dst.p) return set_err(ctx, EMQX_GM_ENOMEM, "deliver_batches: device buffers");
  EventSet<9> ev;
  if (const int rc = ev.create(ctx)) return rc;
  // count
  GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  if (so_launch_seglen(st, so->dv, d_mro, n, d_mids, nnz, d_from, d_len.as<uint64_t>(), d_hit.as<uint32_t>()))
    return set_err(ctx, EMQX_GM_EDEVICE, "deliver_batches: segment lengths");
  if (const int rc = scan_lengths(ctx, d_len.as<uint64_t>(), nnz, d_dst.as<uint64_t>())) return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  uint64_t T = 0;
  GM_HIP(ctx, hipMemcpyAsync(&T, d_dst.as<uint64_t>() + nnz, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  if (T >= 0xFFFFFFFFull)
    return set_err(ctx, EMQX_GM_EOVERFLOW, "deliver_batches: 2^32 - 1 deliveries or more in one call");
  if (!T) return no_batches();
  // the chunks and the workspace
  const uint64_t c_max = (T + SB_BLOCK - 1) / SB_BLOCK;
  uint32_t C = uint32_t(std::min<uint64_t>(n_chunks ? n_chunks : sb_chunks(T), c_max));
  const uint64_t L = (T + C - 1) / C;
  C = uint32_t((T + L - 1) / L);
  const uint32_t passes = sb_passes(so->max_sub);
  const uint64_t cap = std::min<uint64_t>(T, so->hv.n_subs);  // batches at the most: the table's pairs
  PoolBuf d_key[2] = {PoolBuf(ctx->pool, T * 4), PoolBuf(ctx->pool, T * 4)};
  PoolBuf d_val[2] = {PoolBuf(ctx->pool, T * 4), PoolBuf(ctx->pool, T * 4)};
  PoolBuf d_hrow(ctx->pool, T * 4), d_hfil(ctx->pool, T * 4), d_hopt(ctx->pool, T + 16);
  PoolBuf d_hist(ctx->pool, uint64_t(C) * SB_BINS * 4), d_tot(ctx->pool, SB_BINS * 8), d_boff(ctx->pool, (SB_BINS + 1) * 8);
  PoolBuf d_E(ctx->pool, (T + 1) * 8), d_first(ctx->pool, (cap + 1) * 8), d_P, d_Q;
  if (lead) d_P = PoolBuf(ctx->pool, (T + 1) * 8);
  if (!flag) d_Q = PoolBuf(ctx->pool, (T + 1) * 8);
  if (!d_key[0].p || !d_key[1].p || !d_val[0].p || !d_val[1].p || !d_hrow.p || !d_hfil.p || !d_hopt.p || !d_hist.p ||
      !d_tot.p || !d_boff.p || !d_E.p || !d_first.p || (lead && !d_P.p) || (!flag && !d_Q.p))
    return set_err(ctx, EMQX_GM_ENOMEM, "deliver_batches: partition workspace");
  // expand
  GM_HIP(ctx, hipEventRecord(ev.e[2], st));
  {
    const SbRows w{d_dst.as<uint64_t>(), nnz, d_mro, n, d_mids, d_hit.as<uint32_t>(), d_mf};
    const SbExp o{d_key[0].as<uint32_t>(), d_val[0].as<uint32_t>(), d_hrow.as<uint32_t>(), d_hfil.as<uint32_t>(),
                  d_hopt.as<uint8_t>()};
    const uint64_t per = fan_per_block(T);
    hipLaunchKernelGGL(k_sb_expand, dim3((T + per - 1) / per), dim3(256), 0, st, so->dv, w, T, per, o);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ev.e[3], st));
  // partition: one stable pass per digit, least significant first
  int cur = 0;
  for (uint32_t p = 0; p < passes; ++p, cur ^= 1) {
    const uint32_t shift = 8 * p;
    hipLaunchKernelGGL(k_sb_hist, dim3(C), dim3(SB_BLOCK), 0, st, d_key[cur].as<uint32_t>(), T, L, shift,
                       d_hist.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sb_column, dim3(1), dim3(SB_BINS), 0, st, d_hist.as<uint32_t>(), C, d_tot.as<uint64_t>());
    GM_HIP(ctx, hipGetLastError());
    if (const int rc = scan_lengths(ctx, d_tot.as<uint64_t>(), SB_BINS, d_boff.as<uint64_t>())) return rc;
    hipLaunchKernelGGL(k_sb_scatter, dim3(C), dim3(SB_BLOCK), 0, st, d_key[cur].as<uint32_t>(),
                       d_val[cur].as<uint32_t>(), T, L, shift, d_hist.as<uint32_t>(), d_boff.as<uint64_t>(),
                       d_key[cur ^ 1].as<uint32_t>(), d_val[cur ^ 1].as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ev.e[4], st));
  const uint32_t* s_key = d_key[cur].as<uint32_t>();
  const uint32_t* s_val = d_val[cur].as<uint32_t>();
  // heads and removal
  if (const int rc = scan_excl(ctx, LoadHead{s_key}, T, d_E.as<uint64_t>())) return rc;
  hipLaunchKernelGGL(k_sb_heads, dim3(blocks_of(T)), dim3(256), 0, st, s_key, d_E.as<uint64_t>(), T, cap,
                     d_first.as<uint64_t>());
  GM_HIP(ctx, hipGetLastError());
  if (lead)
    if (const int rc = scan_excl(ctx, LoadNonHit{s_val, d_hopt.as<uint8_t>()}, T, d_P.as<uint64_t>())) return rc;
  if (!flag)
    if (const int rc = scan_excl(ctx, LoadKeep{s_val, d_hopt.as<uint8_t>(), d_E.as<uint64_t>(), d_first.as<uint64_t>(),
                                               d_P.as<uint64_t>(), lead},
                                 T, d_Q.as<uint64_t>()))
      return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[5], st));
  uint64_t nb = 0, kept = T;
  GM_HIP(ctx, hipMemcpyAsync(&nb, d_E.as<uint64_t>() + T, 8, hipMemcpyDeviceToHost, st));
  if (!flag) GM_HIP(ctx, hipMemcpyAsync(&kept, d_Q.as<uint64_t>() + T, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  if (!nb || nb > cap || kept > T) return set_err(ctx, EMQX_GM_EDEVICE, "deliver_batches: batch count");
  if (const int rc = res_arrays(nb, kept)) return rc;
  res.n_dropped = T - kept;
  // emit
  PoolBuf o_sub, o_off, o_row, o_fil, o_opt, o_drp;  // host rows: the device side of the result
  uint32_t *p_sub = res.subs, *p_row = res.rows, *p_fil = res.filters, *p_drp = res.batch_dropped;
  uint64_t* p_off = res.batch_off;
  uint8_t* p_opt = res.dopt;
  if (!dev) {
    o_sub = PoolBuf(ctx->pool, nb * 4);
    o_off = PoolBuf(ctx->pool, (nb + 1) * 8);
    o_row = PoolBuf(ctx->pool, std::max<uint64_t>(kept, 4) * 4);
    o_fil = PoolBuf(ctx->pool, std::max<uint64_t>(kept, 4) * 4);
    o_opt = PoolBuf(ctx->pool, std::max<uint64_t>(kept, 16));
    if (!flag) o_drp = PoolBuf(ctx->pool, nb * 4);
    if (!o_sub.p || !o_off.p || !o_row.p || !o_fil.p || !o_opt.p || (!flag && !o_drp.p))
      return set_err(ctx, EMQX_GM_ENOMEM, "deliver_batches: device buffers");
    p_sub = o_sub.as<uint32_t>(), p_off = o_off.as<uint64_t>(), p_row = o_row.as<uint32_t>();
    p_fil = o_fil.as<uint32_t>(), p_opt = o_opt.as<uint8_t>(), p_drp = o_drp.as<uint32_t>();
  }
  GM_HIP(ctx, hipEventRecord(ev.e[6], st));
  hipLaunchKernelGGL(k_sb_batches, dim3(blocks_of(nb + 1)), dim3(256), 0, st, s_key, d_first.as<uint64_t>(),
                     flag ? static_cast<const uint64_t*>(nullptr) : d_Q.as<uint64_t>(), nb, T, p_sub, p_off, p_drp);
  GM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_sb_emit, dim3(blocks_of(T)), dim3(256), 0, st, s_val, d_hrow.as<uint32_t>(),
                     d_hfil.as<uint32_t>(), d_hopt.as<uint8_t>(),
                     flag ? static_cast<const uint64_t*>(nullptr) : d_Q.as<uint64_t>(), T, kept,
                     uint8_t(lead ? 0xFF & ~SO_HIT : 0xFF), p_row, p_fil, p_opt);
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipEventRecord(ev.e[7], st));
  if (!dev) {
    GM_HIP(ctx, hipMemcpyAsync(res.subs, p_sub, nb * 4, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipMemcpyAsync(res.batch_off, p_off, (nb + 1) * 8, hipMemcpyDeviceToHost, st));
    if (kept) {
      GM_HIP(ctx, hipMemcpyAsync(res.rows, p_row, kept * 4, hipMemcpyDeviceToHost, st));
      GM_HIP(ctx, hipMemcpyAsync(res.filters, p_fil, kept * 4, hipMemcpyDeviceToHost, st));
      GM_HIP(ctx, hipMemcpyAsync(res.dopt, p_opt, kept, hipMemcpyDeviceToHost, st));
    }
    if (!flag) GM_HIP(ctx, hipMemcpyAsync(res.batch_dropped, p_drp, nb * 4, hipMemcpyDeviceToHost, st));
  }
  GM_HIP(ctx, hipEventRecord(ev.e[8], st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  float ms[6] = {0, 0, 0, 0, 0, 0}, tail = 0;
  GM_HIP(ctx, hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[1], ev.e[2], ev.e[3]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[2], ev.e[3], ev.e[4]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[3], ev.e[4], ev.e[5]));
  GM_HIP(ctx, hipEventElapsedTime(&tail, ev.e[6], ev.e[7]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[4], ev.e[0], ev.e[8]));
  ms[3] += tail;
  {
    std::lock_guard<std::mutex> lk(so->mu);
    for (int k = 0; k < 5; ++k) so->sb_ms[k] = ms[k];
    so->sb_ms[5] = passes;
  }
  undo.armed = false;
  *out = res;
  return EMQX_GM_OK;
}

}  // namespace gm

extern "C" {

int emqx_gm_deliver_batches_chunked(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m,
                                    const uint8_t* msg_flags, const uint32_t* msg_from, uint32_t mode,
                                    uint32_t n_chunks, emqx_gm_batches* out) {
  if (!ctx || !so || !m || !out) return EMQX_GM_EINVAL;
  if (!so->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "deliver_batches: a host-only table");
  if (so->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "deliver_batches: the table is on another device");
  if (n_chunks > gm::SB_MAX_CHUNKS) return gm::set_err(ctx, EMQX_GM_EINVAL, "deliver_batches: chunk count");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::so_check_call(so, m, msg_flags, msg_from, mode, &why, true))
    return gm::set_err(ctx, rc, "deliver_batches: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::sb_batches_device(ctx, so, m, msg_flags, msg_from, mode, n_chunks, out);
  GM_GUARD_END(ctx)
}

int emqx_gm_deliver_batches(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                            const uint32_t* msg_from, uint32_t mode, emqx_gm_batches* out) {
  return emqx_gm_deliver_batches_chunked(ctx, so, m, msg_flags, msg_from, mode, 0, out);
}

int emqx_gm_batches_free(emqx_gm_ctx* ctx, emqx_gm_batches* b) {
  if (!b) return EMQX_GM_EINVAL;
  if (!b->priv) return b->on_device ? EMQX_GM_EINVAL : gm::sb_free_malloc(b);  // (the host walk's)
  if (!ctx || b->priv != ctx) return EMQX_GM_EINVAL;
  void* ps[6];
  gm::sb_ptrs(b, ps);
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (b->on_device) {
      // (later calls may be queued behind a reader of these buffers)
      hipSetDevice(ctx->device);
      ctx->pool->release_after(ps, 4, ctx->stream);
      ctx->pool->release_after(ps + 4, 2, ctx->stream);
    } else {
      for (void* p : ps) ctx->hpool->release(p);
    }
  }
  std::memset(b, 0, sizeof(*b));
  return EMQX_GM_OK;
}

int emqx_gm_batches_last_times(const emqx_gm_subopts* so, double* ms7) {
  if (!so || !ms7) return EMQX_GM_EINVAL;
  std::lock_guard<std::mutex> lk(const_cast<emqx_gm_subopts*>(so)->mu);
  for (int k = 0; k < 7; ++k) ms7[k] = so->sb_ms[k];
  return EMQX_GM_OK;
}

}  // extern "C"
