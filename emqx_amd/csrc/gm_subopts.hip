// gm_subopts.hip — gfx950 kernels of the deliver call and the device entry
// points (layout and the byte rules: gm_subopts.h; the reference path it
// replaces: ignore_local/4 and enrich_deliver/2 per delivery, apps/emqx/src/
// emqx_session.erl:279-291, 560-602).
//
// A call runs on the context stream:
//   k_so_seglen   one lane per match entry: the filter's segment length, and
//                 -- when the row has a publisher and the filter has No-Local
//                 pairs -- a binary search of the publisher in the filter's
//                 ascending nl_sub: seg_hit = the pair's position in the
//                 segment, or none.  DROP mode: the length minus the hit.
//   the library's scan (lengths -> seg_dst), the fan-out's k_fanout_rowoff
//   (row offsets); DROP mode: k_so_rowdrop, one lane per row, counts the hits
//   of its entries, and a scan of the counts gives their sum;
//   one 16-byte read back gives the delivery total and the dropped total;
//   k_so_copy     k_fanout_copy's shape: every workgroup owns a fixed range of
//                 OUTPUT elements (a fast path when the range is one segment);
//                 a thread moves 4 ids and writes their 4 option bytes as one
//                 dword when the 4 lie in one segment.
// No atomics, no sort, no compaction pass: a dropped delivery is skipped by
// the source index (t + 1 from the hit on), so the output order is the
// fan-out's.
//
// A publish window (emqx_gm_publish_window_deliver, gm_publish.hip) queues the
// same kernels over its SPECULATIVE rows without the read back (so_queue_spec):
// k_so_seglen / k_so_rowdrop over the ids' capacity with the rows' own count
// read on the device, k_so_copy over a capacity of deliveries, and k_so_pack,
// one launch that carries the result and the two true totals to mapped
// page-locked buffers.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_scan.h"
#include "gm_subopts.h"

namespace gm {
namespace {

// the row of match entry j: the last r < n_rows with m_off[r] <= j (n_rows >= 1)
__device__ __forceinline__ uint64_t so_row_of(const uint64_t* __restrict__ m_off, uint64_t n_rows, uint64_t j) {
  uint64_t lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (m_off[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// nnz_p (optional, a publish window's speculative rows: nnz is their ids'
// capacity): the rows' own count on the device; an entry past it is an empty
// segment without a hit -- its id, its row and the table are not read (the
// buffer's tail is uninitialised pool memory)
__global__ __launch_bounds__(256) void k_so_seglen(SoView v, const uint64_t* __restrict__ m_off, uint64_t n_rows,
                                                   const uint32_t* __restrict__ m_ids, uint64_t nnz,
                                                   const uint64_t* __restrict__ nnz_p,
                                                   const uint32_t* __restrict__ from, bool drop,
                                                   uint64_t* __restrict__ seg_len, uint32_t* __restrict__ seg_hit) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  if (nnz_p && i >= *nnz_p) {
    seg_hit[i] = SO_NONE;
    seg_len[i] = 0;
    return;
  }
  const uint32_t f = m_ids[i];
  uint64_t len = 0;
  uint32_t hit = SO_NONE;
  if (f < v.n_filters) {  // (an id past the snapshot is skipped: an empty segment)
    len = v.sub_off[f + 1] - v.sub_off[f];
    uint64_t a = v.nl_off[f], b = v.nl_off[f + 1];
    if (b > a && b <= v.n_nl) {
      const uint32_t x = from[so_row_of(m_off, n_rows, i)];
      if (x != SO_NONE) {
        while (a < b) {
          const uint64_t mid = a + (b - a) / 2;
          const uint32_t y = v.nl_sub[mid];
          if (y == x) {
            hit = v.nl_pos[mid];
            break;
          }
          if (y < x) a = mid + 1;
          else b = mid;
        }
      }
    }
    if (hit != SO_NONE && hit >= len) hit = SO_NONE;  // (never, by the table's construction)
  }
  seg_hit[i] = hit;
  seg_len[i] = len - ((drop && hit != SO_NONE) ? 1 : 0);
}

// DROP mode: the hits of a row's entries (a row holds few matched filters)
// nnz_p (optional): as k_so_seglen's -- the offsets are clamped to the device's count too
__global__ __launch_bounds__(256) void k_so_rowdrop(const uint64_t* __restrict__ m_off, uint64_t n_rows, uint64_t nnz,
                                                    const uint64_t* __restrict__ nnz_p,
                                                    const uint32_t* __restrict__ seg_hit,
                                                    uint32_t* __restrict__ row_dropped) {
  const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  if (nnz_p) nnz = min(nnz, *nnz_p);
  uint64_t a = m_off[r], b = m_off[r + 1];
  if (a > nnz) a = nnz;  // (a device row offset past the ids is clamped)
  if (b > nnz) b = nnz;
  uint32_t c = 0;
  for (uint64_t j = a; j < b; ++j) c += seg_hit[j] != SO_NONE;
  row_dropped[r] = c;
}

struct LoadU32 {
  const uint32_t* p;
  __device__ uint64_t operator()(uint64_t i) const { return p[i]; }
};

// last segment in [a, b] whose start <= p (as gm_csr.hip's fan_seg)
__device__ __forceinline__ uint64_t so_seg(const uint64_t* __restrict__ seg_dst, uint64_t a, uint64_t b, uint64_t p) {
  if (a == b) return a;
  ++b;
  while (b - a > 1) {
    const uint64_t m = (a + b) >> 1;
    if (seg_dst[m] <= p) a = m;
    else b = m;
  }
  return a;
}

// What a thread needs of one segment: where it starts in the output and in
// sub_ids, its hit, and its row's message byte.
struct SoSeg {
  uint64_t dst, src;
  uint32_t hit;
  uint8_t msg;
};
__device__ __forceinline__ SoSeg so_seg_load(const SoView& v, const uint64_t* __restrict__ seg_dst,
                                             const uint64_t* __restrict__ m_off, uint64_t n_rows,
                                             const uint32_t* __restrict__ m_ids,
                                             const uint32_t* __restrict__ seg_hit,
                                             const uint8_t* __restrict__ msg_flags, uint64_t s) {
  SoSeg g;
  g.dst = seg_dst[s];
  g.src = v.sub_off[m_ids[s]];  // (a segment that holds an output element has an id of the snapshot)
  g.hit = seg_hit[s];
  g.msg = msg_flags[so_row_of(m_off, n_rows, s)] & 0x0Fu;
  return g;
}

// output element q of segment g: its id and delivery byte
__device__ __forceinline__ void so_one(const SoView& v, const SoSeg& g, bool drop, uint64_t q,
                                       uint32_t* __restrict__ out_ids, uint8_t* __restrict__ dopt) {
  const uint64_t t = q - g.dst;
  const uint64_t k = t + ((drop && t >= g.hit) ? 1 : 0);
  out_ids[q] = v.sub_ids[g.src + k];
  dopt[q] = uint8_t(so_byte(v.opt[g.src + k], g.msg) | ((!drop && k == g.hit) ? SO_HIT : 0));
}

// output elements q .. q + 3, all of segment g; q is a multiple of 4
__device__ __forceinline__ void so_four(const SoView& v, const SoSeg& g, bool drop, uint64_t q,
                                        uint32_t* __restrict__ out_ids, uint8_t* __restrict__ dopt) {
  const uint64_t t = q - g.dst;
  const uint64_t h = g.hit;  // (SO_NONE: past every position)
  uint32_t id[4], ow;
  if (!drop || t + 3 < h || t >= h) {  // one run of the source: 4 consecutive pairs
    const uint64_t k = g.src + t + ((drop && t >= h) ? 1 : 0);
    const uint32_t* si = v.sub_ids + k;
#pragma unroll
    for (int e = 0; e < 4; ++e) id[e] = si[e];
    __builtin_memcpy(&ow, v.opt + k, 4);  // (one dword load at any alignment: four byte loads cost four address slots)
  } else {  // the dropped pair lies among them
    ow = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint64_t k = g.src + t + e + ((t + e >= h) ? 1 : 0);
      id[e] = v.sub_ids[k];
      ow |= uint32_t(v.opt[k]) << (8 * e);
    }
  }
  uint32_t w = so_byte4(ow, g.msg);
  if (!drop && g.hit != SO_NONE && h - t < 4) w |= uint32_t(SO_HIT) << (8 * (h - t));  // (h < t wraps far past 4)
#pragma unroll
  for (int e = 0; e < 4; ++e) __builtin_nontemporal_store(id[e], out_ids + q + e);
  __builtin_nontemporal_store(w, reinterpret_cast<uint32_t*>(dopt + q));
}

// Every workgroup owns per_block (a multiple of 1,024) consecutive output
// elements [lo, hi) of [0, total); a thread moves 4 at a time.
__global__ __launch_bounds__(256) void k_so_copy(SoView v, const uint64_t* __restrict__ seg_dst, uint64_t nseg,
                                                 const uint64_t* __restrict__ m_off, uint64_t n_rows,
                                                 const uint32_t* __restrict__ m_ids,
                                                 const uint32_t* __restrict__ seg_hit,
                                                 const uint8_t* __restrict__ msg_flags, uint64_t total,
                                                 uint64_t per_block, bool drop, uint32_t* __restrict__ out_ids,
                                                 uint8_t* __restrict__ dopt) {
  total = min(total, seg_dst[nseg]);  // (never past the device's own total)
  const uint64_t lo = uint64_t(blockIdx.x) * per_block;
  if (lo >= total) return;
  const uint64_t hi = min(total, lo + per_block);
  __shared__ uint64_t s_seg[2];
  if (threadIdx.x < 2) {
    // last segment whose start <= x (segments may be empty)
    const uint64_t x = threadIdx.x == 0 ? lo : hi - 1;
    uint64_t a = 0, b = nseg;  // seg_dst[a] <= x < seg_dst[b]
    while (b - a > 1) {
      const uint64_t m = (a + b) >> 1;
      if (seg_dst[m] <= x) a = m;
      else b = m;
    }
    s_seg[threadIdx.x] = a;
  }
  __syncthreads();
  const uint64_t s0 = s_seg[0], s1 = s_seg[1];
  if (s0 == s1) {
    // the whole range lies in one segment (a hot row): the segment, its hit and
    // its row's message byte are loop invariant
    const SoSeg g = so_seg_load(v, seg_dst, m_off, n_rows, m_ids, seg_hit, msg_flags, s0);
    uint64_t q = lo + uint64_t(threadIdx.x) * 4;
    for (; q + 4 <= hi; q += 256 * 4) so_four(v, g, drop, q, out_ids, dopt);
    for (uint64_t p = q; p < hi; ++p) so_one(v, g, drop, p, out_ids, dopt);  // q + 4 > hi here: at most 3 left
    return;
  }
  for (uint64_t q = lo + uint64_t(threadIdx.x) * 4; q < hi; q += 256 * 4) {
    const uint64_t s = so_seg(seg_dst, s0, s1, q);
    if (q + 4 <= hi && q + 4 <= seg_dst[s + 1]) {
      so_four(v, so_seg_load(v, seg_dst, m_off, n_rows, m_ids, seg_hit, msg_flags, s), drop, q, out_ids, dopt);
    } else {
      for (uint64_t p = q; p < q + 4 && p < hi; ++p) {
        const uint64_t sp = so_seg(seg_dst, s0, s1, p);
        so_one(v, so_seg_load(v, seg_dst, m_off, n_rows, m_ids, seg_hit, msg_flags, sp), drop, p, out_ids, dopt);
      }
    }
  }
}

// A publish window's speculative deliveries to their mapped page-locked result
// in one launch (as gm_publish.hip's k_pw_pack for the picks and the plan):
// plain vector stores, no atomics; the ids' and bytes' lengths are the device's
// own total clamped to the capacity, and the two true totals travel along.
struct SoPack {
  const uint64_t* ro;  // [n_ro] row offsets
  uint64_t* o_ro;
  uint64_t n_ro;
  const uint32_t* ids;  // [cap] + slack
  uint32_t* o_ids;
  const uint32_t* opt;  // [cap] bytes + slack, moved as words
  uint32_t* o_opt;
  uint64_t cap;
  const uint32_t* rd;  // [n_rd] DROP mode (n_rd = 0: none)
  uint32_t* o_rd;
  uint64_t n_rd;
  const uint64_t *total, *dropped;  // (dropped: nullptr in FLAG mode)
  uint64_t* o_meta;                 // [0] the true deliveries, [1] the true dropped
};

// n u32 words, 16 B at a time (every buffer here is 16-B aligned)
__device__ __forceinline__ void so_pack_copy(uint32_t* __restrict__ d, const uint32_t* __restrict__ s, uint64_t n,
                                             uint64_t t, uint64_t stride) {
  const uint64_t q = n / 4;
  for (uint64_t i = t; i < q; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
  if (t < (n & 3)) d[q * 4 + t] = s[q * 4 + t];
}

__global__ __launch_bounds__(256) void k_so_pack(SoPack a) {
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x, stride = uint64_t(gridDim.x) * 256u;
  const uint64_t total = *a.total, k = min(total, a.cap);
  so_pack_copy(reinterpret_cast<uint32_t*>(a.o_ro), reinterpret_cast<const uint32_t*>(a.ro), a.n_ro * 2, t, stride);
  so_pack_copy(a.o_ids, a.ids, k, t, stride);
  so_pack_copy(a.o_opt, a.opt, (k + 3) / 4, t, stride);  // (the bytes' buffers end in 16 B of slack)
  if (a.n_rd) so_pack_copy(a.o_rd, a.rd, a.n_rd, t, stride);
  if (t == 0) {
    a.o_meta[0] = total;
    a.o_meta[1] = a.dropped ? *a.dropped : 0;
  }
  __threadfence_system();  // (host-bound stores visible before the call's end event)
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + 255) / 256); }

struct SoUndo {  // a failing call hands back no buffers
  emqx_gm_ctx* c;
  emqx_gm_deliveries* o;
  bool dev, armed = true;
  ~SoUndo() {
    if (!armed) return;
    void* ps[4] = {o->deliveries.row_off, o->deliveries.ids, o->dopt, o->row_dropped};
    if (dev) hipStreamSynchronize(c->stream);  // (a queued kernel may still write them)
    for (void* p : ps) {
      if (!p) continue;
      if (dev) c->pool->release(p);
      else c->hpool->release(p);
    }
    *o = emqx_gm_deliveries{};
  }
};

}  // namespace

// (gm_batches.hip counts a window's deliveries with the same kernel)
int so_launch_seglen(hipStream_t st, const SoView& dv, const uint64_t* d_mro, uint64_t n_rows, const uint32_t* d_mids,
                     uint64_t nnz, const uint32_t* d_from, uint64_t* seg_len, uint32_t* seg_hit) {
  hipLaunchKernelGGL(k_so_seglen, dim3(blocks_of(nnz)), dim3(256), 0, st, dv, d_mro, n_rows, d_mids, nnz,
                     static_cast<const uint64_t*>(nullptr), d_from, false, seg_len, seg_hit);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

int so_upload(emqx_gm_ctx* ctx, emqx_gm_subopts* so) {
  if (const int rc = table_upload(ctx, so->blob, so->bytes, "subopts_build", &so->dev_base)) return rc;
  const void* hb = so->blob.data();
  so->dv.opt = rebase(so->hv.opt, hb, so->dev_base);
  so->dv.nl_off = rebase(so->hv.nl_off, hb, so->dev_base);
  so->dv.nl_sub = rebase(so->hv.nl_sub, hb, so->dev_base);
  so->dv.nl_pos = rebase(so->hv.nl_pos, hb, so->dev_base);
  so->dv.sub_off = so->idx->view.sub_off;  // the bound snapshot's own lists
  so->dv.sub_ids = so->idx->view.sub_ids;
  so->device = ctx->device;
  so->info.device_bytes = so->bytes;
  return EMQX_GM_OK;
}

void so_free_device(emqx_gm_subopts* so) {
  table_free(so->device, so->dev_base);  // (waits for the device: no queued call still reads the tables)
  so->dev_base = nullptr;
}

int so_deliver_device(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                      const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out, bool host_out, uint32_t* waits,
                      const uint8_t* d_flags_up, const uint32_t* d_from_up) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // (host_out: device rows, but host messages -- or their uploaded copies -- and a host result: a publish
  // window's rerun, gm_publish.hip)
  const bool dev_in = m->on_device != 0, dev = dev_in && !host_out, drop = mode == EMQX_GM_SO_DROP;
  const bool msgs_up = host_out && d_flags_up && d_from_up;
  auto waited = [&]() {
    if (waits) ++*waits;
  };
  const uint64_t n = m->n_rows, nnz = m->nnz;
  auto res_alloc = [&](size_t bytes) -> void* {
    bytes = std::max<size_t>(bytes, 16);
    return dev ? ctx->pool->alloc(bytes) : ctx->hpool->alloc(bytes);
  };
  emqx_gm_deliveries res{};  // (the caller's struct is written only on success)
  SoUndo undo{ctx, &res, dev};
  res.deliveries.priv = ctx;  // the owning context (emqx_gm_deliveries_free checks it)
  res.deliveries.n_rows = n;
  res.deliveries.on_device = dev ? 1 : 0;
  res.deliveries.row_off = static_cast<uint64_t*>(res_alloc((n + 1) * 8));
  if (drop) res.row_dropped = static_cast<uint32_t*>(res_alloc(n * 4));
  if (!res.deliveries.row_off || (drop && !res.row_dropped))
    return set_err(ctx, EMQX_GM_ENOMEM, "deliver: result arrays");
  if (!n || !nnz || !so->hv.n_subs) {  // no delivery at all
    res.deliveries.ids = static_cast<uint32_t*>(res_alloc(0));
    res.dopt = static_cast<uint8_t*>(res_alloc(0));
    if (!res.deliveries.ids || !res.dopt) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: result arrays");
    if (dev) {
      GM_HIP(ctx, hipMemsetAsync(res.deliveries.row_off, 0, (n + 1) * 8, st));
      if (drop && n) GM_HIP(ctx, hipMemsetAsync(res.row_dropped, 0, n * 4, st));
      GM_HIP(ctx, hipStreamSynchronize(st));
    } else {
      std::fill(res.deliveries.row_off, res.deliveries.row_off + n + 1, uint64_t(0));
      if (drop) std::fill(res.row_dropped, res.row_dropped + n, 0u);
    }
    undo.armed = false;
    *out = res;
    return EMQX_GM_OK;
  }
  // the rows and the messages on the device
  PoolBuf b_ro, b_ids, b_mf, b_from;
  const uint64_t* d_mro = m->row_off;
  const uint32_t* d_mids = m->ids;
  const uint8_t* d_mf = msg_flags;
  const uint32_t* d_from = msg_from;
  if (!dev_in) {
    b_ro = PoolBuf(ctx->pool, (n + 1) * 8);
    b_ids = PoolBuf(ctx->pool, nnz * 4);
    if (!b_ro.p || !b_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: device buffers");
    GM_HIP(ctx, hipMemcpyAsync(b_ro.p, m->row_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_ids.p, m->ids, nnz * 4, hipMemcpyHostToDevice, st));
    d_mro = b_ro.as<uint64_t>();
    d_mids = b_ids.as<uint32_t>();
  }
  if (msgs_up) {
    d_mf = d_flags_up;
    d_from = d_from_up;
  } else if (!dev) {
    b_mf = PoolBuf(ctx->pool, n);
    b_from = PoolBuf(ctx->pool, n * 4);
    if (!b_mf.p || !b_from.p) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: device buffers");
    GM_HIP(ctx, hipMemcpyAsync(b_mf.p, msg_flags, n, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_from.p, msg_from, n * 4, hipMemcpyHostToDevice, st));
    d_mf = b_mf.as<uint8_t>();
    d_from = b_from.as<uint32_t>();
  }
  PoolBuf d_len(ctx->pool, nnz * 8), d_hit(ctx->pool, nnz * 4), d_dst(ctx->pool, (nnz + 1) * 8);
  PoolBuf d_ro, d_rd, d_rdsum;  // host rows: the device side of the result
  uint64_t* o_ro = res.deliveries.row_off;
  uint32_t* o_rd = res.row_dropped;
  if (!dev) {
    d_ro = PoolBuf(ctx->pool, (n + 1) * 8);
    if (drop) d_rd = PoolBuf(ctx->pool, n * 4);
    if (!d_ro.p || (drop && !d_rd.p)) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: device buffers");
    o_ro = d_ro.as<uint64_t>();
    o_rd = d_rd.as<uint32_t>();
  }
  if (drop) d_rdsum = PoolBuf(ctx->pool, (n + 1) * 8);
  if (!d_len.p || !d_hit.p || !d_dst.p || (drop && !d_rdsum.p))
    return set_err(ctx, EMQX_GM_ENOMEM, "deliver: device buffers");
  EventSet<4> ev;
  if (const int rc = ev.create(ctx)) return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(k_so_seglen, dim3(blocks_of(nnz)), dim3(256), 0, st, so->dv, d_mro, n, d_mids, nnz,
                     static_cast<const uint64_t*>(nullptr), d_from, drop, d_len.as<uint64_t>(), d_hit.as<uint32_t>());
  GM_HIP(ctx, hipGetLastError());
  if (const int rc = scan_lengths(ctx, d_len.as<uint64_t>(), nnz, d_dst.as<uint64_t>())) return rc;
  if (launch_fanout_rowoff(st, d_mro, n, d_dst.as<uint64_t>(), o_ro, nnz))
    return set_err(ctx, EMQX_GM_EDEVICE, "deliver: row offsets");
  if (drop) {
    hipLaunchKernelGGL(k_so_rowdrop, dim3(blocks_of(n)), dim3(256), 0, st, d_mro, n, nnz,
                       static_cast<const uint64_t*>(nullptr), d_hit.as<uint32_t>(), o_rd);
    GM_HIP(ctx, hipGetLastError());
    if (const int rc = scan_excl(ctx, LoadU32{o_rd}, n, d_rdsum.as<uint64_t>())) return rc;
  }
  GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  uint64_t total = 0, n_dropped = 0;
  GM_HIP(ctx, hipMemcpyAsync(&total, d_dst.as<uint64_t>() + nnz, 8, hipMemcpyDeviceToHost, st));
  if (drop) GM_HIP(ctx, hipMemcpyAsync(&n_dropped, d_rdsum.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  res.deliveries.nnz = total;
  res.n_dropped = n_dropped;
  res.deliveries.ids = static_cast<uint32_t*>(res_alloc(total * 4 + 16));
  res.dopt = static_cast<uint8_t*>(res_alloc(total + 16));
  if (!res.deliveries.ids || !res.dopt) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: result arrays");
  PoolBuf d_ids, d_opt;
  uint32_t* o_ids = res.deliveries.ids;
  uint8_t* o_opt = res.dopt;
  if (!dev) {
    d_ids = PoolBuf(ctx->pool, total * 4 + 16);
    d_opt = PoolBuf(ctx->pool, total + 16);
    if (!d_ids.p || !d_opt.p) return set_err(ctx, EMQX_GM_ENOMEM, "deliver: device buffers");
    o_ids = d_ids.as<uint32_t>();
    o_opt = d_opt.as<uint8_t>();
  }
  if (total) {
    const uint64_t per = fan_per_block(total);
    hipLaunchKernelGGL(k_so_copy, dim3((total + per - 1) / per), dim3(256), 0, st, so->dv, d_dst.as<uint64_t>(), nnz,
                       d_mro, n, d_mids, d_hit.as<uint32_t>(), d_mf, total, per, drop, o_ids, o_opt);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ev.e[2], st));
  if (!dev) {
    GM_HIP(ctx, hipMemcpyAsync(res.deliveries.row_off, o_ro, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) {
      GM_HIP(ctx, hipMemcpyAsync(res.deliveries.ids, o_ids, total * 4, hipMemcpyDeviceToHost, st));
      GM_HIP(ctx, hipMemcpyAsync(res.dopt, o_opt, total, hipMemcpyDeviceToHost, st));
    }
    if (drop) GM_HIP(ctx, hipMemcpyAsync(res.row_dropped, o_rd, n * 4, hipMemcpyDeviceToHost, st));
  }
  GM_HIP(ctx, hipEventRecord(ev.e[3], st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  float ms[3] = {0, 0, 0};
  GM_HIP(ctx, hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[1], ev.e[1], ev.e[2]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[2], ev.e[0], ev.e[3]));
  {
    std::lock_guard<std::mutex> lk(so->mu);
    for (int k = 0; k < 3; ++k) so->last_ms[k] = ms[k];
  }
  undo.armed = false;
  *out = res;
  return EMQX_GM_OK;
}

// The deliveries of a small call's SPECULATIVE rows (gm_publish.hip), queued on
// the context stream with no wait and no read-back: the lengths run over the
// ids' capacity `cap` with the rows' own count read on the device (d_ro + n),
// the copy over cap_d output elements (k_so_copy clamps to the device's total).
// msgs: the call's page-locked [publishers | flags] (so_msgs_bytes), up in one
// launch.  1: not queued.
int so_queue_spec(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_d, uint32_t mode, const void* msgs, SoSpec* out) {
  hipStream_t st = ctx->stream;
  if (!n || !cap || !cap_d || !msgs || !so->hv.n_subs) return 1;  // (the exact call answers without device work)
  const bool drop = mode == EMQX_GM_SO_DROP;
  // one workspace: messages | len | hit | dst | row offsets | row drops | their scan | ids | bytes
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(std::max<size_t>(bytes, 16), 256);
    return at;
  };
  const size_t o_from = take(so_msgs_bytes(n)), o_flags = o_from + al16(n * 4);
  const size_t o_len = take(cap * 8), o_hit = take(cap * 4), o_dst = take((cap + 1) * 8), o_ro = take((n + 1) * 8);
  const size_t o_rd = drop ? take(n * 4) : 0, o_rds = drop ? take((n + 1) * 8) : 0;
  const size_t o_ids = take(cap_d * 4 + 16), o_opt = take(cap_d + 16);
  uint8_t* w = static_cast<uint8_t*>(ctx->pool->alloc(o));
  if (!w) return 1;
  uint64_t* len = reinterpret_cast<uint64_t*>(w + o_len);
  uint32_t* hit = reinterpret_cast<uint32_t*>(w + o_hit);
  uint64_t* dst = reinterpret_cast<uint64_t*>(w + o_dst);
  out->ws = w;
  out->d_from = reinterpret_cast<uint32_t*>(w + o_from);
  out->d_flags = w + o_flags;
  out->row_off = reinterpret_cast<uint64_t*>(w + o_ro);
  out->ids = reinterpret_cast<uint32_t*>(w + o_ids);
  out->dopt = w + o_opt;
  out->row_dropped = drop ? reinterpret_cast<uint32_t*>(w + o_rd) : nullptr;
  out->total = dst + cap;
  out->dropped = drop ? reinterpret_cast<uint64_t*>(w + o_rds) + n : nullptr;
  auto fail = [&](int rc) {
    hipStreamSynchronize(st);  // (a queued kernel may still write the workspace)
    ctx->pool->release(w);
    *out = SoSpec{};
    return rc;
  };
#define SO_Q(expr)                                                                                   \
  do {                                                                                               \
    if ((expr) != hipSuccess) return fail(set_err(ctx, EMQX_GM_EDEVICE, "publish_window: " #expr)); \
  } while (0)
  // the publishers and the flags (padded to words) up in ONE launch
  void* mdev = nullptr;
  if (so_msgs_bytes(n) <= (size_t(1) << 20) && hipHostGetDevicePointer(&mdev, const_cast<void*>(msgs), 0) == hipSuccess) {
    const uint8_t* md = static_cast<const uint8_t*>(mdev);
    if (launch_copy_u32x2(st, reinterpret_cast<const uint32_t*>(md), reinterpret_cast<uint32_t*>(w + o_from), n,
                          reinterpret_cast<const uint32_t*>(md + al16(n * 4)), reinterpret_cast<uint32_t*>(w + o_flags),
                          (n + 3) / 4))
      return fail(set_err(ctx, EMQX_GM_EDEVICE, "publish_window: messages to device"));
  } else {
    SO_Q(hipMemcpyAsync(w + o_from, msgs, so_msgs_bytes(n), hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(k_so_seglen, dim3(blocks_of(cap)), dim3(256), 0, st, so->dv, d_ro, n, d_ids, cap, d_ro + n,
                     out->d_from, drop, len, hit);
  SO_Q(hipGetLastError());
  if (const int rc = scan_lengths(ctx, len, cap, dst)) return fail(rc);
  if (launch_fanout_rowoff(st, d_ro, n, dst, out->row_off, cap))
    return fail(set_err(ctx, EMQX_GM_EDEVICE, "publish_window: delivery row offsets"));
  if (drop) {
    hipLaunchKernelGGL(k_so_rowdrop, dim3(blocks_of(n)), dim3(256), 0, st, d_ro, n, cap, d_ro + n, hit,
                       out->row_dropped);
    SO_Q(hipGetLastError());
    if (const int rc = scan_excl(ctx, LoadU32{out->row_dropped}, n, reinterpret_cast<uint64_t*>(w + o_rds)))
      return fail(rc);
  }
  // the small fan-out's cut: 1,024 output elements a workgroup at the least
  const uint64_t per = fan_per_block(cap_d);
  hipLaunchKernelGGL(k_so_copy, dim3((cap_d + per - 1) / per), dim3(256), 0, st, so->dv, dst, cap, d_ro, n, d_ids, hit,
                     out->d_flags, cap_d, per, drop, out->ids, out->dopt);
  SO_Q(hipGetLastError());
#undef SO_Q
  return 0;
}

// the queued deliveries to their mapped page-locked result (device addresses), one launch
int so_queue_pack(emqx_gm_ctx* ctx, const SoSpec& run, uint64_t n, uint64_t cap_d, uint64_t* o_ro, uint32_t* o_ids,
                  uint8_t* o_opt, uint32_t* o_rd, uint64_t* o_meta) {
  SoPack k{};
  k.ro = run.row_off;
  k.o_ro = o_ro;
  k.n_ro = n + 1;
  k.ids = run.ids;
  k.o_ids = o_ids;
  k.opt = reinterpret_cast<const uint32_t*>(run.dopt);
  k.o_opt = reinterpret_cast<uint32_t*>(o_opt);
  k.cap = cap_d;
  k.rd = run.row_dropped;
  k.o_rd = o_rd;
  k.n_rd = run.row_dropped ? n : 0;
  k.total = run.total;
  k.dropped = run.dropped;
  k.o_meta = o_meta;
  const uint64_t words = std::max((n + 1) * 2, cap_d);
  const uint64_t g = std::min<uint64_t>(1024, ((words + 3) / 4 + 255) / 256);
  hipLaunchKernelGGL(k_so_pack, dim3(g ? g : 1), dim3(256), 0, ctx->stream, k);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

}  // namespace gm

extern "C" {

int emqx_gm_subopts_build(emqx_gm_ctx* ctx, emqx_gm_index* idx, const uint8_t* fb, const uint64_t* fo,
                          const uint32_t* sub_ids, const uint8_t* opts, uint64_t n_entries, uint8_t default_opt,
                          uint32_t flags, emqx_gm_subopts** out) {
  if (!ctx || !out) return EMQX_GM_EINVAL;
  *out = nullptr;
  if (!idx) return gm::set_err(ctx, EMQX_GM_EINVAL, "subopts_build: NULL index");
  if (idx->route || !idx->shards.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "subopts_build: a sharded index");
  if (idx->view.gmap || !idx->gmap.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "subopts_build: a shard index");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "subopts_build: an overlay snapshot");
  if (idx->subs.empty() || !idx->view.sub_off)
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "subopts_build: an index without subscriber lists");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "subopts_build: the index is on another device");
  GM_GUARD_BEGIN
  std::string why;
  // the snapshot's lists, read back once (as gm_subs.cpp's rebuild does)
  const std::vector<uint64_t> soff = idx->subs.offsets();
  const uint64_t nf = idx->info.n_filters;
  if (soff.size() != nf + 1) return gm::set_err(ctx, EMQX_GM_EINVAL, "subopts_build: subscriber table");
  std::vector<uint32_t> sids(soff[nf]);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!sids.empty()) {
    GM_HIP(ctx, hipSetDevice(ctx->device));
    GM_HIP(ctx, hipMemcpy(sids.data(), idx->view.sub_ids, sids.size() * 4, hipMemcpyDeviceToHost));
  }
  auto resolve = [&](const uint8_t* p, uint64_t len, uint32_t* id) {
    bool found = false;
    const uint64_t r = gm::filter_rank(idx, p, len, &found);
    *id = uint32_t(r);
    return found;
  };
  const gm::SoInput in{fb, fo, sub_ids, opts, n_entries, default_opt, flags};
  emqx_gm_subopts* so = nullptr;
  int rc = gm::so_compile(in, nf, soff.data(), sids.data(), resolve, &so, &why);
  if (rc) return gm::set_err(ctx, rc, "subopts_build: " + why);
  so->idx = idx;
  rc = gm::so_upload(ctx, so);
  if (rc) {
    delete so;
    return rc;
  }
  emqx_gm_index_retain(idx);
  *out = so;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_deliver(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                    const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out) {
  if (!ctx || !so || !m || !out) return EMQX_GM_EINVAL;
  if (!so->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "deliver: a host-only table");
  if (so->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "deliver: the table is on another device");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::so_check_call(so, m, msg_flags, msg_from, mode, &why))
    return gm::set_err(ctx, rc, "deliver: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::so_deliver_device(ctx, so, m, msg_flags, msg_from, mode, out);
  GM_GUARD_END(ctx)
}

int emqx_gm_deliveries_free(emqx_gm_ctx* ctx, emqx_gm_deliveries* d) {
  if (!d) return EMQX_GM_EINVAL;
  if (!d->deliveries.priv) return d->deliveries.on_device ? EMQX_GM_EINVAL : gm::so_free_malloc(d);  // (the host walk's)
  if (!ctx || d->deliveries.priv != ctx) return EMQX_GM_EINVAL;
  void* ps[4] = {d->deliveries.row_off, d->deliveries.ids, d->dopt, d->row_dropped};
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (d->deliveries.on_device) {
      // (later calls may be queued behind a reader of these buffers)
      hipSetDevice(ctx->device);
      ctx->pool->release_after(ps, 4, ctx->stream);
    } else {
      for (void* p : ps) ctx->hpool->release(p);
    }
  }
  std::memset(d, 0, sizeof(*d));
  return EMQX_GM_OK;
}

}  // extern "C"
