// gm_dests.hip — gfx950 kernels of the forward plan and the device entry points
// (layout and the chunk rule: gm_dests.h; the reference path it replaces:
// lookup_routes/1 per matched filter and forward/3 per (message, route),
// apps/emqx/src/emqx_router.erl:136, emqx_broker.erl:245-293).
//
// A call runs on the context stream:
//   enumerate  k_fw_row_routes (one lane per row: its {To, Node} route count,
//              skip_node's included), k_fw_count (one lane per matched id: its
//              hits), the library's scan (hit offsets); one 8-byte read back
//              gives the hit total;
//   expand     k_fw_expand (one lane per matched id): (row, filter, node) of
//              each of its hits into the flat hit array, in batch order;
//   partition  stable, by node, over the flat hit array cut into C chunks of L
//              consecutive hits:
//     k_fw_hist     one block per chunk counts its hits per node in LDS
//                   (integer atomics: the order is irrelevant) and stores its
//                   row hist[chunk][node];
//     k_fw_column   one lane per node: the exclusive prefix over the C rows in
//                   place, and the node's total;
//     the library's scan over the totals: node_off;
//     k_fw_scatter  one block per chunk keeps next[node] = node_off[node] +
//                   hist[chunk][node] in LDS and walks its hits 256 at a time
//                   in order; a hit's rank among the equal-node lanes below it
//                   comes from ballots over the node id's bits (lane order),
//                   and the block's four waves take their turns in wave order.
// No workgroup waits on another: every dependency is a kernel boundary.  The
// order of each node's list is the batch order whatever C is.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_device.h"
#include "gm_dests.h"

namespace gm {
namespace {

constexpr uint32_t FW_NONE = 0xFFFFFFFFu;

// whether the ascending list nodes[a, b) holds x
__device__ __forceinline__ bool fw_has(const uint16_t* __restrict__ nodes, uint32_t a, uint32_t b, uint32_t x) {
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    const uint32_t y = nodes[mid];
    if (y == x) return true;
    if (y < x) a = mid + 1;
    else b = mid;
  }
  return false;
}

__global__ __launch_bounds__(256) void k_fw_row_routes(DtView v, const uint64_t* __restrict__ m_ro, uint64_t n_rows,
                                                       const uint32_t* __restrict__ ids, uint64_t nnz,
                                                       uint32_t* __restrict__ row_routes) {
  const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  uint64_t a = m_ro[r], b = m_ro[r + 1];
  if (a > nnz) a = nnz;  // (a device row offset past the ids is clamped)
  if (b > nnz) b = nnz;
  uint64_t all = 0;
  for (uint64_t j = a; j < b; ++j) {
    const uint32_t f = ids[j];
    if (f < v.n_filters) all += v.d_off[f + 1] - v.d_off[f];  // (an id past the snapshot is skipped)
  }
  row_routes[r] = all < 0xFFFFFFFFull ? uint32_t(all) : 0xFFFFFFFFu;
}

// nnz_p (optional, speculative rows: nnz is their capacity): the rows' own count
// on the device; an entry past it counts 0, so k_fw_expand skips it too
__global__ __launch_bounds__(256) void k_fw_count(DtView v, const uint32_t* __restrict__ ids, uint64_t nnz,
                                                  const uint64_t* __restrict__ nnz_p, uint32_t skip_node,
                                                  uint64_t* __restrict__ cnt) {
  const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= nnz) return;
  if (nnz_p && j >= *nnz_p) {
    cnt[j] = 0;
    return;
  }
  const uint32_t f = ids[j];
  uint32_t c = 0;
  if (f < v.n_filters) {
    const uint32_t a = v.d_off[f], b = v.d_off[f + 1];
    c = b - a;
    if (c && skip_node < v.n_nodes && fw_has(v.nodes, a, b, skip_node)) --c;
  }
  cnt[j] = c;
}

__global__ __launch_bounds__(256) void k_fw_expand(DtView v, const uint64_t* __restrict__ m_ro, uint64_t n_rows,
                                                   const uint32_t* __restrict__ ids, uint64_t nnz,
                                                   const uint64_t* __restrict__ hoff, uint64_t hits,
                                                   uint32_t skip_node, uint32_t* __restrict__ h_row,
                                                   uint32_t* __restrict__ h_filter, uint32_t* __restrict__ h_node) {
  const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= nnz) return;
  const uint32_t f = ids[j];
  if (f >= v.n_filters) return;
  const uint32_t a = v.d_off[f], b = v.d_off[f + 1];
  uint64_t h = hoff[j];
  if (a == b || hoff[j + 1] == h) return;
  // the row of matched id j: the last r < n_rows with m_ro[r] <= j
  uint64_t lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (m_ro[mid] <= j) lo = mid;
    else hi = mid;
  }
  for (uint32_t k = a; k < b; ++k) {
    const uint32_t node = v.nodes[k];
    if (node == skip_node) continue;
    if (h >= hits) return;
    h_row[h] = uint32_t(lo);
    h_filter[h] = f;
    h_node[h] = node;
    ++h;
  }
}

// hist[chunk][node] = the chunk's hits on the node
__global__ __launch_bounds__(FW_BLOCK) void k_fw_hist(const uint32_t* __restrict__ h_node, uint64_t hits,
                                                      uint64_t chunk_len, uint32_t n_nodes,
                                                      uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t s_cnt[];  // [n_nodes]
  for (uint32_t k = threadIdx.x; k < n_nodes; k += FW_BLOCK) s_cnt[k] = 0;
  __syncthreads();
  const uint64_t begin = uint64_t(blockIdx.x) * chunk_len;
  const uint64_t end = begin + chunk_len < hits ? begin + chunk_len : hits;
  for (uint64_t h = begin + threadIdx.x; h < end; h += FW_BLOCK) {
    const uint32_t node = h_node[h];
    if (node < n_nodes) atomicAdd(&s_cnt[node], 1u);
  }
  __syncthreads();
  uint32_t* row = hist + uint64_t(blockIdx.x) * n_nodes;
  for (uint32_t k = threadIdx.x; k < n_nodes; k += FW_BLOCK) row[k] = s_cnt[k];
}

// One lane per node (coalesced across nodes): hist[c][node] becomes the hits on
// the node in chunks < c, total[node] the node's hits.
__global__ __launch_bounds__(256) void k_fw_column(uint32_t* __restrict__ hist, uint32_t n_chunks, uint32_t n_nodes,
                                                   uint64_t* __restrict__ total) {
  const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n_nodes) return;
  uint32_t sum = 0;  // (the call's hits are below 2^32 - 1)
  for (uint32_t c = 0; c < n_chunks; ++c) {
    uint32_t* p = hist + uint64_t(c) * n_nodes + node;
    const uint32_t t = *p;
    *p = sum;
    sum += t;
  }
  total[node] = sum;
}

// One block per chunk.  bits = the bits a node id below n_nodes needs.
__global__ __launch_bounds__(FW_BLOCK) void k_fw_scatter(const uint32_t* __restrict__ h_row,
                                                         const uint32_t* __restrict__ h_filter,
                                                         const uint32_t* __restrict__ h_node, uint64_t hits,
                                                         uint64_t chunk_len, uint32_t n_nodes, uint32_t bits,
                                                         const uint32_t* __restrict__ hist,
                                                         const uint64_t* __restrict__ node_off,
                                                         uint32_t* __restrict__ out_rows,
                                                         uint32_t* __restrict__ out_filters) {
  extern __shared__ uint32_t s_next[];  // [n_nodes]: where the node's next hit of this chunk goes
  const uint32_t* row = hist + uint64_t(blockIdx.x) * n_nodes;
  for (uint32_t k = threadIdx.x; k < n_nodes; k += FW_BLOCK) s_next[k] = uint32_t(node_off[k]) + row[k];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t begin = uint64_t(blockIdx.x) * chunk_len;
  const uint64_t end = begin + chunk_len < hits ? begin + chunk_len : hits;
  for (uint64_t base = begin; base < end; base += FW_BLOCK) {  // (the trip count is the same for every thread)
    const uint64_t h = base + threadIdx.x;
    uint32_t node = FW_NONE, r = 0, f = 0;
    if (h < end) {
      node = h_node[h];
      r = h_row[h];
      f = h_filter[h];
    }
    const bool active = node < n_nodes;
    // the lanes of this wave holding the same node: one ballot per bit of the id
    uint64_t peers = __ballot(active);
    for (uint32_t b = 0; b < bits; ++b) {
      const uint64_t set = __ballot(active && ((node >> b) & 1u));
      peers &= ((node >> b) & 1u) ? set : ~set;
    }
    const uint32_t rank = lanes_below(peers, lane), n = __popcll(peers);
    for (uint32_t w = 0; w < FW_BLOCK / 64; ++w) {  // the waves in order: wave w's hits come before wave w + 1's
      if (wave == w) {
        uint32_t next = 0;
        if (active) next = s_next[node];
        wave_sync();  // every lane has read its slot before a leader writes it
        if (active) {
          const uint32_t pos = next + rank;
          if (pos < hits) {
            out_rows[pos] = r;
            out_filters[pos] = f;
          }
          if (rank == 0) s_next[node] = next + n;
        }
      }
      __syncthreads();
    }
  }
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + 255) / 256); }

struct FwUndo {  // a failing call hands back no buffers
  emqx_gm_ctx* c;
  emqx_gm_forwards* o;
  bool dev, armed = true;
  ~FwUndo() {
    if (!armed) return;
    void* ps[4] = {o->node_off, o->rows, o->filters, o->row_routes};
    if (dev) hipStreamSynchronize(c->stream);  // (a queued kernel may still write them)
    for (void* p : ps) {
      if (!p) continue;
      if (dev) c->pool->release(p);
      else c->hpool->release(p);
    }
    *o = emqx_gm_forwards{};
  }
};

}  // namespace

int dt_upload(emqx_gm_ctx* ctx, emqx_gm_dests* dt) {
  if (const int rc = table_upload(ctx, dt->blob, dt->bytes, "dests_build", &dt->dev_base)) return rc;
  const void* hb = dt->blob.data();
  dt->dv.d_off = rebase(dt->hv.d_off, hb, dt->dev_base);
  dt->dv.nodes = rebase(dt->hv.nodes, hb, dt->dev_base);
  dt->device = ctx->device;
  dt->info.device_bytes = dt->bytes;
  return EMQX_GM_OK;
}

void dt_free_device(emqx_gm_dests* dt) {
  table_free(dt->device, dt->dev_base);  // (waits for the device: no queued plan still reads the tables)
  dt->dev_base = nullptr;
}

int dt_plan_device(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node, uint32_t n_chunks,
                   emqx_gm_forwards* out, bool host_out, uint32_t* waits) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // (host_out: device rows, but a host result -- a publish window's rerun, gm_publish.hip)
  const bool dev_in = m->on_device != 0, dev = dev_in && !host_out;
  auto waited = [&]() {
    if (waits) ++*waits;
  };
  const uint64_t n = m->n_rows, nnz = m->nnz;
  const uint32_t N = dt->hv.n_nodes;
  auto res_alloc = [&](size_t bytes) -> void* {
    bytes = std::max<size_t>(bytes, 16);
    return dev ? ctx->pool->alloc(bytes) : ctx->hpool->alloc(bytes);
  };
  FwUndo undo{ctx, out, dev};
  out->priv = ctx;  // the owning context (emqx_gm_forwards_free checks it)
  out->n_rows = n;
  out->n_nodes = N;
  out->on_device = dev ? 1 : 0;
  out->node_off = static_cast<uint64_t*>(res_alloc((uint64_t(N) + 1) * 8));
  out->row_routes = static_cast<uint32_t*>(res_alloc(n * 4));
  if (!out->node_off || !out->row_routes) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: result arrays");
  auto no_pairs = [&]() -> int {  // node_off all zero; rows / filters hold no entry
    out->n_pairs = 0;
    out->rows = static_cast<uint32_t*>(res_alloc(0));
    out->filters = static_cast<uint32_t*>(res_alloc(0));
    if (!out->rows || !out->filters) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: result arrays");
    if (dev) {
      GM_HIP(ctx, hipMemsetAsync(out->node_off, 0, (uint64_t(N) + 1) * 8, st));
      GM_HIP(ctx, hipStreamSynchronize(st));
      waited();
    } else {
      std::fill(out->node_off, out->node_off + N + 1, uint64_t(0));
    }
    undo.armed = false;
    return EMQX_GM_OK;
  };
  if (!nnz || !n || !dt->hv.n_routes) {  // no route at all
    if (dev) {
      if (n) GM_HIP(ctx, hipMemsetAsync(out->row_routes, 0, n * 4, st));
    } else {
      std::fill(out->row_routes, out->row_routes + n, 0u);
    }
    return no_pairs();
  }
  // the rows on the device
  PoolBuf b_ro, b_ids, b_rr;
  const uint64_t* d_mro = m->row_off;
  const uint32_t* d_mids = m->ids;
  uint32_t* d_rr = out->row_routes;
  if (!dev_in) {
    b_ro = PoolBuf(ctx->pool, (n + 1) * 8);
    b_ids = PoolBuf(ctx->pool, nnz * 4);
    if (!b_ro.p || !b_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: device buffers");
    GM_HIP(ctx, hipMemcpyAsync(b_ro.p, m->row_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemcpyAsync(b_ids.p, m->ids, nnz * 4, hipMemcpyHostToDevice, st));
    d_mro = b_ro.as<uint64_t>();
    d_mids = b_ids.as<uint32_t>();
  }
  if (!dev) {
    b_rr = PoolBuf(ctx->pool, n * 4);
    if (!b_rr.p) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: device buffers");
    d_rr = b_rr.as<uint32_t>();
  }
  PoolBuf d_cnt(ctx->pool, nnz * 8), d_hoff(ctx->pool, (nnz + 1) * 8);
  if (!d_cnt.p || !d_hoff.p) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: device buffers");
  EventSet<5> ev;
  if (const int rc = ev.create(ctx)) return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[0], st));
  // enumerate
  hipLaunchKernelGGL(k_fw_row_routes, dim3(blocks_of(n)), dim3(256), 0, st, dt->dv, d_mro, n, d_mids, nnz, d_rr);
  GM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_fw_count, dim3(blocks_of(nnz)), dim3(256), 0, st, dt->dv, d_mids, nnz,
                     static_cast<const uint64_t*>(nullptr), skip_node, d_cnt.as<uint64_t>());
  GM_HIP(ctx, hipGetLastError());
  if (const int rc = scan_lengths(ctx, d_cnt.as<uint64_t>(), nnz, d_hoff.as<uint64_t>())) return rc;
  GM_HIP(ctx, hipEventRecord(ev.e[1], st));
  uint64_t hits = 0;
  GM_HIP(ctx, hipMemcpyAsync(&hits, d_hoff.as<uint64_t>() + nnz, 8, hipMemcpyDeviceToHost, st));
  if (!dev) GM_HIP(ctx, hipMemcpyAsync(out->row_routes, d_rr, n * 4, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  if (hits >= 0xFFFFFFFFull) return set_err(ctx, EMQX_GM_EOVERFLOW, "forward_plan: 2^32 - 1 hits or more in one call");
  if (!hits) return no_pairs();  // (every route of the window is skip_node's: row_routes still counts them)
  out->n_pairs = hits;
  // the chunks and the partition's workspace
  uint32_t C = n_chunks ? n_chunks : fw_chunks(hits, N);
  C = uint32_t(std::min<uint64_t>(C, hits));
  const uint64_t L = (hits + C - 1) / C;
  C = uint32_t((hits + L - 1) / L);
  PoolBuf d_hrow(ctx->pool, hits * 4), d_hfil(ctx->pool, hits * 4), d_hnode(ctx->pool, hits * 4);
  PoolBuf d_hist(ctx->pool, uint64_t(C) * N * 4), d_tot(ctx->pool, uint64_t(N) * 8);
  if (!d_hrow.p || !d_hfil.p || !d_hnode.p || !d_hist.p || !d_tot.p)
    return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: partition workspace");
  PoolBuf d_noff, d_orow, d_ofil;  // host rows: the device side of the result
  uint64_t* o_noff;
  uint32_t *o_row, *o_fil;
  out->rows = static_cast<uint32_t*>(res_alloc(hits * 4));
  out->filters = static_cast<uint32_t*>(res_alloc(hits * 4));
  if (!out->rows || !out->filters) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: result arrays");
  if (dev) {
    o_noff = out->node_off;
    o_row = out->rows;
    o_fil = out->filters;
  } else {
    d_noff = PoolBuf(ctx->pool, (uint64_t(N) + 1) * 8);
    d_orow = PoolBuf(ctx->pool, hits * 4);
    d_ofil = PoolBuf(ctx->pool, hits * 4);
    if (!d_noff.p || !d_orow.p || !d_ofil.p) return set_err(ctx, EMQX_GM_ENOMEM, "forward_plan: device buffers");
    o_noff = d_noff.as<uint64_t>();
    o_row = d_orow.as<uint32_t>();
    o_fil = d_ofil.as<uint32_t>();
  }
  // expand
  hipLaunchKernelGGL(k_fw_expand, dim3(blocks_of(nnz)), dim3(256), 0, st, dt->dv, d_mro, n, d_mids, nnz,
                     d_hoff.as<uint64_t>(), hits, skip_node, d_hrow.as<uint32_t>(), d_hfil.as<uint32_t>(),
                     d_hnode.as<uint32_t>());
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipEventRecord(ev.e[2], st));
  // partition
  uint32_t bits = 0;
  while ((1u << bits) < N) ++bits;
  const size_t lds = size_t(N) * 4;
  hipLaunchKernelGGL(k_fw_hist, dim3(C), dim3(FW_BLOCK), lds, st, d_hnode.as<uint32_t>(), hits, L, N,
                     d_hist.as<uint32_t>());
  GM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_fw_column, dim3(blocks_of(N)), dim3(256), 0, st, d_hist.as<uint32_t>(), C, N,
                     d_tot.as<uint64_t>());
  GM_HIP(ctx, hipGetLastError());
  if (const int rc = scan_lengths(ctx, d_tot.as<uint64_t>(), N, o_noff)) return rc;
  hipLaunchKernelGGL(k_fw_scatter, dim3(C), dim3(FW_BLOCK), lds, st, d_hrow.as<uint32_t>(), d_hfil.as<uint32_t>(),
                     d_hnode.as<uint32_t>(), hits, L, N, bits, d_hist.as<uint32_t>(), o_noff, o_row, o_fil);
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipEventRecord(ev.e[3], st));
  if (!dev) {
    GM_HIP(ctx, hipMemcpyAsync(out->node_off, o_noff, (uint64_t(N) + 1) * 8, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipMemcpyAsync(out->rows, o_row, hits * 4, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipMemcpyAsync(out->filters, o_fil, hits * 4, hipMemcpyDeviceToHost, st));
  }
  GM_HIP(ctx, hipEventRecord(ev.e[4], st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  waited();
  float ms[4] = {0, 0, 0, 0};
  for (int k = 0; k < 3; ++k) GM_HIP(ctx, hipEventElapsedTime(&ms[k], ev.e[k], ev.e[k + 1]));
  GM_HIP(ctx, hipEventElapsedTime(&ms[3], ev.e[0], ev.e[4]));
  {
    std::lock_guard<std::mutex> lk(dt->mu);
    for (int k = 0; k < 4; ++k) dt->last_ms[k] = ms[k];
  }
  undo.armed = false;
  return EMQX_GM_OK;
}


// The plan of a small call's SPECULATIVE rows (gm_publish.hip), queued on the
// context stream with no wait and no read-back: the counts run over the ids'
// capacity `cap` with the rows' own count read on the device (d_ro + n), the
// expansion into cap_pairs hits (h_node pre-filled FW_NONE, so the partition
// skips the unused ones; its chunking is fixed from cap_pairs).  1: not queued.
int dt_queue_spec(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_pairs, uint32_t skip_node, DtSpec* out) {
  hipStream_t st = ctx->stream;
  const uint32_t N = dt->hv.n_nodes;
  if (!N || !n || !cap || !cap_pairs) return 1;  // (nothing to plan: the exact call answers without a kernel)
  uint32_t C = uint32_t(std::min<uint64_t>(fw_chunks(cap_pairs, N), cap_pairs));
  const uint64_t L = (cap_pairs + C - 1) / C;
  C = uint32_t((cap_pairs + L - 1) / L);
  // one workspace: cnt | hoff | row routes | hit rows | hit filters | hit nodes | hist | totals | node_off | rows | filters
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(std::max<size_t>(bytes, 16), 256);
    return at;
  };
  const size_t o_cnt = take(cap * 8), o_hoff = take((cap + 1) * 8), o_rr = take(n * 4);
  const size_t o_hrow = take(cap_pairs * 4), o_hfil = take(cap_pairs * 4), o_hnode = take(cap_pairs * 4);
  const size_t o_hist = take(uint64_t(C) * N * 4), o_tot = take(uint64_t(N) * 8), o_noff = take((uint64_t(N) + 1) * 8);
  const size_t o_orow = take(cap_pairs * 4), o_ofil = take(cap_pairs * 4);
  uint8_t* w = static_cast<uint8_t*>(ctx->pool->alloc(o));
  if (!w) return 1;
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(w + off); };
  auto u64 = [&](size_t off) { return reinterpret_cast<uint64_t*>(w + off); };
  out->ws = w;
  out->row_routes = u32(o_rr);
  out->node_off = u64(o_noff);
  out->rows = u32(o_orow);
  out->filters = u32(o_ofil);
  out->total = u64(o_hoff) + cap;
  auto fail = [&](int rc) {
    hipStreamSynchronize(st);  // (a queued kernel may still write the workspace)
    ctx->pool->release(w);
    *out = DtSpec{};
    return rc;
  };
#define FW_Q(expr)                                                                    \
  do {                                                                                \
    if ((expr) != hipSuccess) return fail(set_err(ctx, EMQX_GM_EDEVICE, "publish_window: " #expr)); \
  } while (0)
  FW_Q(hipMemsetAsync(u32(o_hnode), 0xFF, cap_pairs * 4, st));
  hipLaunchKernelGGL(k_fw_row_routes, dim3(blocks_of(n)), dim3(256), 0, st, dt->dv, d_ro, n, d_ids, cap,
                     out->row_routes);
  FW_Q(hipGetLastError());
  hipLaunchKernelGGL(k_fw_count, dim3(blocks_of(cap)), dim3(256), 0, st, dt->dv, d_ids, cap, d_ro + n, skip_node,
                     u64(o_cnt));
  FW_Q(hipGetLastError());
  if (const int rc = scan_lengths(ctx, u64(o_cnt), cap, u64(o_hoff))) return fail(rc);
  hipLaunchKernelGGL(k_fw_expand, dim3(blocks_of(cap)), dim3(256), 0, st, dt->dv, d_ro, n, d_ids, cap, u64(o_hoff),
                     cap_pairs, skip_node, u32(o_hrow), u32(o_hfil), u32(o_hnode));
  FW_Q(hipGetLastError());
  uint32_t bits = 0;
  while ((1u << bits) < N) ++bits;
  const size_t lds = size_t(N) * 4;
  hipLaunchKernelGGL(k_fw_hist, dim3(C), dim3(FW_BLOCK), lds, st, u32(o_hnode), cap_pairs, L, N, u32(o_hist));
  FW_Q(hipGetLastError());
  hipLaunchKernelGGL(k_fw_column, dim3(blocks_of(N)), dim3(256), 0, st, u32(o_hist), C, N, u64(o_tot));
  FW_Q(hipGetLastError());
  if (const int rc = scan_lengths(ctx, u64(o_tot), N, out->node_off)) return fail(rc);
  hipLaunchKernelGGL(k_fw_scatter, dim3(C), dim3(FW_BLOCK), lds, st, u32(o_hrow), u32(o_hfil), u32(o_hnode), cap_pairs,
                     L, N, bits, u32(o_hist), out->node_off, out->rows, out->filters);
  FW_Q(hipGetLastError());
#undef FW_Q
  return 0;
}

}  // namespace gm

extern "C" {

int emqx_gm_dests_build(emqx_gm_ctx* ctx, emqx_gm_index* idx, const uint8_t* fb, const uint64_t* fo,
                        const uint32_t* node_ids, uint64_t n_routes, uint32_t n_nodes, uint32_t flags,
                        emqx_gm_dests** out) {
  if (!ctx || !out) return EMQX_GM_EINVAL;
  *out = nullptr;
  if (!idx) return gm::set_err(ctx, EMQX_GM_EINVAL, "dests_build: NULL index");
  if (idx->route || !idx->shards.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "dests_build: a sharded index");
  if (idx->view.gmap || !idx->gmap.empty())
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "dests_build: a shard index");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "dests_build: an overlay snapshot");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "dests_build: the index is on another device");
  GM_GUARD_BEGIN
  std::string why;
  auto resolve = [&](const uint8_t* p, uint64_t len, uint32_t* id) {
    bool found = false;
    const uint64_t r = gm::filter_rank(idx, p, len, &found);
    *id = uint32_t(r);
    return found;
  };
  const gm::DtInput in{fb, fo, node_ids, n_routes, n_nodes, flags};
  emqx_gm_dests* dt = nullptr;
  int rc = gm::dt_compile(in, idx->info.n_filters, resolve, &dt, &why);  // (every input check: before any device work)
  if (rc) return gm::set_err(ctx, rc, "dests_build: " + why);
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    rc = gm::dt_upload(ctx, dt);
  }
  if (rc) {
    delete dt;
    return rc;
  }
  emqx_gm_index_retain(idx);
  dt->idx = idx;
  *out = dt;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_forward_plan_chunked(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node,
                                 uint32_t n_chunks, emqx_gm_forwards* out) {
  if (!ctx || !dt || !m || !out) return EMQX_GM_EINVAL;
  std::memset(out, 0, sizeof(*out));
  if (!dt->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "forward_plan: a host-only table");
  if (dt->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "forward_plan: the table is on another device");
  if (n_chunks > gm::FW_MAX_CHUNKS) return gm::set_err(ctx, EMQX_GM_EINVAL, "forward_plan: chunk count");
  GM_GUARD_BEGIN
  std::string why;
  if (const int rc = gm::dt_check_rows(dt, m, &why)) return gm::set_err(ctx, rc, "forward_plan: " + why);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return gm::dt_plan_device(ctx, dt, m, skip_node, n_chunks, out, false, nullptr);
  GM_GUARD_END(ctx)
}

int emqx_gm_forward_plan(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node,
                         emqx_gm_forwards* out) {
  return emqx_gm_forward_plan_chunked(ctx, dt, m, skip_node, 0, out);
}

int emqx_gm_forwards_free(emqx_gm_ctx* ctx, emqx_gm_forwards* fw) {
  if (!fw) return EMQX_GM_EINVAL;
  if (!fw->priv) return fw->on_device ? EMQX_GM_EINVAL : gm::fw_free_malloc(fw);  // (the host walk's)
  if (!ctx || fw->priv != ctx) return EMQX_GM_EINVAL;
  void* ps[4] = {fw->node_off, fw->rows, fw->filters, fw->row_routes};
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (fw->on_device) {
      // (later calls may be queued behind a reader of these buffers)
      hipSetDevice(ctx->device);
      ctx->pool->release_after(ps, 4, ctx->stream);
    } else {
      for (void* p : ps) ctx->hpool->release(p);
    }
  }
  std::memset(fw, 0, sizeof(*fw));
  return EMQX_GM_OK;
}

}  // extern "C"
