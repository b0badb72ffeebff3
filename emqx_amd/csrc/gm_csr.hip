// gm_csr.hip — CDNA4 (gfx950) kernels and host drivers for everything that
// consumes finished match rows (a CSR: row_off u64, ids u32).
//
// Fan-out (replaces emqx_broker:dispatch/2 + do_dispatch, emqx_broker.erl:
// 296-322, 506-530): scan of the matches' subscriber counts -> k_fanout_rowoff
// -> k_fanout_copy, a load-balanced CSR gather in which every workgroup owns a
// fixed range of OUTPUT elements, so a 1M-subscriber row is split across many
// workgroups (run_fanout, and queue_fanout_small / _spec for the small calls
// that queue it without a wait).
//
// Row utilities: the sharded index's row merge (k_merge_rows) and row
// lengths, the overlay snapshot merge (k_ov_merge, run_match_overlay), the
// row un-permute after a prefix-routed exchange (unpermute_rows), the
// host-buffer path's offset conversions and copies (launch_*), the length
// scans other files reach (scan_lengths, scan_len16) and the matched-filter
// length sum of the stats (sum_filter_lengths).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "gm_gather.h"
#include "gm_internal.h"
#include "gm_scan.h"

namespace gm {

// ---------------------------------------------------------------------------
// fan-out
// ---------------------------------------------------------------------------
struct LoadSegLen {  // subscriber count of the filter of match entry i
  const uint32_t* ids;
  const uint64_t* sub_off;
  __device__ uint64_t operator()(uint64_t i) const {
    const uint32_t f = ids[i];
    return sub_off[f + 1] - sub_off[f];
  }
};

// LoadSegLen over a small call's SPECULATIVE rows (emqx_gm_match_fanout): the
// fan-out is queued before the host knows the match count, so entries past the
// device's own count (*nnz, the rows' row_off[n]) and ids out of range (an
// overflowed speculative buffer holds stale words) count 0 -- such a fan-out
// is discarded, but it reads nothing out of bounds
struct LoadSegLenSpec {
  const uint32_t* ids;
  const uint64_t* sub_off;
  const uint64_t* nnz;
  uint32_t nf;
  __device__ uint64_t operator()(uint64_t i) const {
    if (i >= *nnz) return 0;
    const uint32_t f = ids[i];
    return f < nf ? sub_off[f + 1] - sub_off[f] : 0;
  }
};

// (nseg: the segments seg_dst holds -- a speculative call's row offsets may point past them)
__global__ __launch_bounds__(256) void k_fanout_rowoff(const uint64_t* __restrict__ m_off, uint64_t n,
                                                       const uint64_t* __restrict__ seg_dst,
                                                       uint64_t* __restrict__ out_off, uint64_t nseg) {
  const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (i <= n) out_off[i] = seg_dst[min(m_off[i], nseg)];
}

// Segment of output element p: the last segment whose start <= p, searched in
// [a, b] (the block's first and last segments).
__device__ __forceinline__ uint64_t fan_seg(const uint64_t* __restrict__ seg_dst, uint64_t a, uint64_t b, uint64_t p) {
  if (a == b) return a;
  ++b;
  while (b - a > 1) {
    const uint64_t m = (a + b) >> 1;
    if (seg_dst[m] <= p) a = m;
    else b = m;
  }
  return a;
}

// Every workgroup owns per_block consecutive output elements; a thread
// moves 4 consecutive elements at a time, as one 16-B non-temporal store (the
// output is streamed out once) when they lie in one segment -- the usual case,
// a hot row being one long segment -- and element by element across a
// segment boundary.
__global__ __launch_bounds__(256) void k_fanout_copy(const uint64_t* __restrict__ seg_dst, uint64_t nseg,
                                                     const uint32_t* __restrict__ m_ids,
                                                     const uint64_t* __restrict__ sub_off,
                                                     const uint32_t* __restrict__ sub_ids, uint64_t glo,
                                                     uint64_t total, uint64_t per_block, uint32_t* __restrict__ out0,
                                                     bool clamp) {
  // this launch produces the global delivery range [glo, total); out0[0] is delivery glo
  // (clamp: never past the device's own total -- a small host fan-out sizes
  // the launch by a speculative capacity, gm_host.cpp run_fanout_small)
  if (clamp) total = min(total, seg_dst[nseg]);
  const uint64_t lo = glo + uint64_t(blockIdx.x) * per_block;
  if (lo >= total) return;
  const uint64_t hi = min(total, lo + per_block);
  uint32_t* const out = out0 - glo;  // indexed by global delivery number
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
    // the whole range lies in one segment (a hot row): the source offset is
    // loop invariant, so each step is an independent load + store with no
    // dependent segment lookups in between
    const uint64_t off = sub_off[m_ids[s0]] - seg_dst[s0];  // element q comes from sub_ids[off + q] (mod 2^64)
    uint64_t q = lo + uint64_t(threadIdx.x) * 4;
    for (; q + 4 <= hi; q += 256 * 4) {
      const uint32_t* src = sub_ids + (off + q);
      const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
      __builtin_nontemporal_store(v.x, out + q);
      __builtin_nontemporal_store(v.y, out + q + 1);
      __builtin_nontemporal_store(v.z, out + q + 2);
      __builtin_nontemporal_store(v.w, out + q + 3);
    }
    for (uint64_t p = q; p < hi; ++p) out[p] = sub_ids[off + p];  // q + 4 > hi here: at most 3 left
    return;
  }
  for (uint64_t q = lo + uint64_t(threadIdx.x) * 4; q < hi; q += 256 * 4) {
    const uint64_t s = fan_seg(seg_dst, s0, s1, q);
    const uint64_t sd = seg_dst[s];
    if (q + 4 <= hi && q + 4 <= seg_dst[s + 1]) {
      const uint32_t* src = sub_ids + sub_off[m_ids[s]] + (q - sd);
      const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
      __builtin_nontemporal_store(v.x, out + q);
      __builtin_nontemporal_store(v.y, out + q + 1);
      __builtin_nontemporal_store(v.z, out + q + 2);
      __builtin_nontemporal_store(v.w, out + q + 3);
    } else {
      for (uint64_t p = q; p < q + 4 && p < hi; ++p) {
        const uint64_t sp = fan_seg(seg_dst, s0, s1, p);
        out[p] = sub_ids[sub_off[m_ids[sp]] + (p - seg_dst[sp])];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// stats helper: sum of matched filter lengths (for algorithmic bytes)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (a[m] < x) lo = m + 1;
    else hi = m;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_sum_flen(const uint32_t* __restrict__ ids, uint64_t nnz,
                                                  const uint16_t* __restrict__ flen,
                                                  const uint32_t* __restrict__ gmap, uint32_t nf,
                                                  unsigned long long* __restrict__ acc) {
  uint64_t s = 0;
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < nnz; i += uint64_t(gridDim.x) * 256u)
    s += flen[gmap ? lower_bound_u32(gmap, nf, ids[i]) : ids[i]];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(acc, (unsigned long long)s);
}

// ---------------------------------------------------------------------------
// row merge (sharded index)
// ---------------------------------------------------------------------------
// Pieces p = 0..P-1 each hold, for the same n rows, a sorted list of filter
// ids; the lists of one row are disjoint (filters are partitioned over the
// shards).  lens is [P][stride] (rows >= n have length 0), ids the pieces'
// rows concatenated piece-major, row-minor (the all-to-all's output), so an
// exclusive scan of lens gives every (piece, row) list's offset in ids.  Each
// element's rank in its merged row = its index in its own list + its
// lower_bound in every other list of the row.
struct LoadU32 {
  const uint32_t* p;
  __device__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
struct LoadRowSum {  // merged row length
  const uint32_t* lens;
  uint64_t stride;
  uint32_t pieces;
  __device__ uint64_t operator()(uint64_t t) const {
    uint64_t s = 0;
    for (uint32_t p = 0; p < pieces; ++p) s += lens[p * stride + t];
    return s;
  }
};

__global__ __launch_bounds__(256) void k_merge_rows(const uint32_t* __restrict__ lens, const uint64_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ ids, uint64_t n, uint64_t stride,
                                                    uint32_t pieces, const uint64_t* __restrict__ row_off,
                                                    uint32_t* __restrict__ out) {
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (t >= n) return;
  const uint64_t o = row_off[t];
  for (uint32_t p = 0; p < pieces; ++p) {
    const uint64_t src = pos[p * stride + t];
    const uint32_t len = lens[p * stride + t];
    for (uint32_t j = 0; j < len; ++j) {
      const uint32_t x = ids[src + j];
      uint64_t r = j;
      for (uint32_t q = 0; q < pieces; ++q)
        if (q != p) r += lower_bound_u32(ids + pos[q * stride + t], lens[q * stride + t], x);
      out[o + r] = x;
    }
  }
}

__global__ __launch_bounds__(256) void k_row_lengths(const uint64_t* __restrict__ row_off, uint64_t n,
                                                     uint32_t* __restrict__ out) {
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (t < n) out[t] = uint32_t(row_off[t + 1] - row_off[t]);
}

// ---------------------------------------------------------------------------
// overlay snapshot merge (incremental updates, gm_overlay.cpp)
// ---------------------------------------------------------------------------
struct OvView {
  const uint32_t* tbm;   // tombstone bitmap over base ids
  const uint32_t* tpre;  // tombstones in the words before each bitmap word
  const uint32_t* ins;   // insertion point of each delta filter, ascending
  uint32_t n_ins;
};
__device__ __forceinline__ bool ov_dead(const OvView& o, uint32_t b) { return (o.tbm[b >> 5] >> (b & 31)) & 1u; }
// final id of a surviving base id: + delta filters sorting before it - tombstones below it
__device__ __forceinline__ uint32_t ov_remap(const OvView& o, uint32_t b) {
  uint32_t lo = 0, hi = o.n_ins;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (o.ins[m] <= b) lo = m + 1;
    else hi = m;
  }
  const uint32_t w = b >> 5;
  return b + lo - (o.tpre[w] + __popc(o.tbm[w] & ((1u << (b & 31)) - 1u)));
}
struct LoadOvLen {  // merged row length: surviving base ids + delta ids
  const uint64_t* bo;
  const uint32_t* bi;
  const uint64_t* dof;
  OvView o;
  __device__ uint64_t operator()(uint64_t t) const {
    uint64_t c = dof ? dof[t + 1] - dof[t] : 0;
    for (uint64_t k = bo[t]; k < bo[t + 1]; ++k) c += ov_dead(o, bi[k]) ? 0 : 1;
    return c;
  }
};
__global__ __launch_bounds__(256) void k_ov_merge(const uint64_t* __restrict__ bo, const uint32_t* __restrict__ bi,
                                                  const uint64_t* __restrict__ dof, const uint32_t* __restrict__ di,
                                                  OvView o, uint64_t n, const uint64_t* __restrict__ row_off,
                                                  uint32_t* __restrict__ out) {
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (t >= n) return;
  uint64_t i = bo[t], w = row_off[t];
  const uint64_t ie = bo[t + 1];
  uint64_t j = dof ? dof[t] : 0;
  const uint64_t je = dof ? dof[t + 1] : 0;
  auto next_base = [&]() -> uint32_t {
    while (i < ie && ov_dead(o, bi[i])) ++i;
    return i < ie ? ov_remap(o, bi[i]) : 0xFFFFFFFFu;
  };
  uint32_t b = next_base(), d = j < je ? di[j] : 0xFFFFFFFFu;
  while (b != 0xFFFFFFFFu || d != 0xFFFFFFFFu) {
    if (b < d) {
      out[w++] = b;
      ++i;
      b = next_base();
    } else {
      out[w++] = d;
      ++j;
      d = j < je ? di[j] : 0xFFFFFFFFu;
    }
  }
}

// Offsets of the host-buffer path: topics cross PCIe with u32 chunk-relative
// offsets (4 B per topic instead of 8) and rows come back the same way.
__global__ __launch_bounds__(256) void k_off32_to_64(const uint32_t* __restrict__ in, uint64_t n1,
                                                     uint64_t* __restrict__ out) {
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n1; i += uint64_t(gridDim.x) * 256u) out[i] = in[i];
}
__global__ __launch_bounds__(256) void k_off64_to_32(const uint64_t* __restrict__ in, uint64_t n1,
                                                     uint32_t* __restrict__ out) {
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n1; i += uint64_t(gridDim.x) * 256u)
    out[i] = uint32_t(in[i]);
}
int launch_off32_to_64(hipStream_t st, const uint32_t* in, uint64_t n1, uint64_t* out) {
  const uint64_t g = std::min<uint64_t>(2048, (n1 + 255) / 256);
  hipLaunchKernelGGL(k_off32_to_64, dim3(g ? g : 1), dim3(256), 0, st, in, n1, out);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}
int launch_off64_to_32(hipStream_t st, const uint64_t* in, uint64_t n1, uint32_t* out) {
  const uint64_t g = std::min<uint64_t>(2048, (n1 + 255) / 256);
  hipLaunchKernelGGL(k_off64_to_32, dim3(g ? g : 1), dim3(256), 0, st, in, n1, out);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}
// Small host-buffer calls (gm_host.cpp run_host_small): inputs in and rows out
// through page-locked host memory the device addresses directly -- two copies
// in one launch on the call's own queue, so no copy engine has to hand over to
// the compute queue between the call's kernels (~10 us a hand-over).  n1_max
// (optional): the second copy stops at the count the device wrote there (a
// result's row_off[n]: the rows' true length inside a speculative capacity)
__global__ __launch_bounds__(256) void k_copy_u32x2(const uint32_t* __restrict__ s0, uint32_t* __restrict__ d0,
                                                    uint64_t n0, const uint32_t* __restrict__ s1,
                                                    uint32_t* __restrict__ d1, uint64_t n1,
                                                    const uint64_t* __restrict__ n1_max) {
  if (n1_max) n1 = min(n1, *n1_max);
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x, stride = uint64_t(gridDim.x) * 256u;
  const uint64_t q0 = n0 / 4, q1 = n1 / 4;  // (16-B units; every buffer here is 16-B aligned)
  for (uint64_t i = t; i < q0; i += stride)
    reinterpret_cast<uint4*>(d0)[i] = reinterpret_cast<const uint4*>(s0)[i];
  for (uint64_t i = t; i < q1; i += stride)
    reinterpret_cast<uint4*>(d1)[i] = reinterpret_cast<const uint4*>(s1)[i];
  if (t < (n0 & 3)) d0[q0 * 4 + t] = s0[q0 * 4 + t];
  if (t < (n1 & 3)) d1[q1 * 4 + t] = s1[q1 * 4 + t];
  __threadfence_system();  // (host-bound stores visible before the call's end event)
}
int launch_copy_u32x2(hipStream_t st, const uint32_t* s0, uint32_t* d0, uint64_t n0, const uint32_t* s1, uint32_t* d1,
                      uint64_t n1, const uint64_t* n1_max) {
  const uint64_t q = (std::max(n0, n1) + 3) / 4;
  const uint64_t g = std::min<uint64_t>(1024, (q + 255) / 256);
  hipLaunchKernelGGL(k_copy_u32x2, dim3(g ? g : 1), dim3(256), 0, st, s0, d0, n0, s1, d1, n1, n1_max);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}
// p[0..n1) += add, in place (a chunk's row offsets rebased to the whole call's rows)
__global__ __launch_bounds__(256) void k_add_u64(uint64_t* __restrict__ p, uint64_t n1, uint64_t add) {
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n1; i += uint64_t(gridDim.x) * 256u) p[i] += add;
}
int launch_add_u64(hipStream_t st, uint64_t* p, uint64_t n1, uint64_t add) {
  if (!n1) return 0;
  const uint64_t g = std::min<uint64_t>(2048, (n1 + 255) / 256);
  hipLaunchKernelGGL(k_add_u64, dim3(g), dim3(256), 0, st, p, n1, add);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

int scan_lengths(emqx_gm_ctx* ctx, const uint64_t* len, uint64_t n, uint64_t* out) {
  return scan_excl(ctx, LoadU64{len}, n, out);
}

namespace {
struct LoadU16 {
  const uint16_t* p;
  __device__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
}  // namespace
int scan_len16(emqx_gm_ctx* ctx, hipStream_t st, const uint16_t* len, uint64_t n, uint64_t* out) {
  return scan_excl(ctx, LoadU16{len}, n, out, SideSum{}, nullptr, st);
}

int sum_filter_lengths(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint32_t* d_ids, uint64_t nnz,
                       uint64_t* out) {
  if (idx->flen_stale) {  // after an in-place update: the lengths in this snapshot's ids, once
    std::lock_guard<std::mutex> lk(idx->flen_mu);
    if (idx->flen_stale) {
      const uint64_t nf = idx->info.n_filters;
      std::vector<uint16_t> fl(nf + 1, 0);
      idx->ft.for_each([&](uint64_t f, const uint8_t*, uint64_t l) { fl[f] = uint16_t(std::min<uint64_t>(l, 65535)); });
      GM_HIP(ctx, hipMemcpyAsync(idx->dev_flen, fl.data(), nf * 2, hipMemcpyHostToDevice, ctx->stream));
      GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
      idx->flen_stale = false;
    }
  }
  PoolBuf acc(ctx->pool, 16);
  if (!acc.p) return set_err(ctx, EMQX_GM_ENOMEM, "sum_flen");
  GM_HIP(ctx, hipMemsetAsync(acc.p, 0, 8, ctx->stream));
  if (nnz) {
    const uint64_t blocks = std::min<uint64_t>(4096, (nnz + 255) / 256);
    hipLaunchKernelGGL(k_sum_flen, dim3(blocks), dim3(256), 0, ctx->stream, d_ids, nnz, idx->dev_flen,
                       idx->view.gmap, idx->view.n_filters, acc.as<unsigned long long>());
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipMemcpyAsync(out, acc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int run_fanout(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
               emqx_gm_csr* out, uint32_t part, uint32_t n_parts, uint64_t* first_out) {
  const bool dev_out = flags & EMQX_GM_DEVICE_IO;
  hipStream_t st = ctx->stream;
  const uint64_t n = m->n_rows, nnz = m->nnz;
  ctx->stats = emqx_gm_match_stats{};
  ctx->stats.n_topics = n;
  PoolBuf own_off, own_ids;
  const uint64_t* m_off = m->row_off;
  const uint32_t* m_ids = m->ids;
  if (!m->on_device) {
    for (uint64_t i = 0; i < nnz; ++i)
      if (m->ids[i] >= idx->view.n_filters) return set_err(ctx, EMQX_GM_EINVAL, "fanout: filter id out of range");
    own_off = PoolBuf(ctx->pool, (n + 1) * 8);
    own_ids = PoolBuf(ctx->pool, nnz * 4 + 16);
    if (!own_off.p || !own_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "fanout: input workspace");
    GM_HIP(ctx, hipMemcpyAsync(own_off.p, m->row_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz) GM_HIP(ctx, hipMemcpyAsync(own_ids.p, m->ids, nnz * 4, hipMemcpyHostToDevice, st));
    m_off = own_off.as<uint64_t>();
    m_ids = own_ids.as<uint32_t>();
  }
  PoolBuf seg_dst(ctx->pool, (nnz + 1) * 8);
  PoolBuf row_off(ctx->pool, (n + 1) * 8);
  if (!seg_dst.p || !row_off.p) return set_err(ctx, EMQX_GM_ENOMEM, "fanout: workspace");
  GM_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  int rc = scan_excl(ctx, LoadSegLen{m_ids, idx->view.sub_off}, nnz, seg_dst.as<uint64_t>());
  if (rc) return rc;
  hipLaunchKernelGGL(k_fanout_rowoff, dim3((n + 1 + 255) / 256), dim3(256), 0, st, m_off, n, seg_dst.as<uint64_t>(),
                     row_off.as<uint64_t>(), nnz);
  GM_HIP(ctx, hipGetLastError());
  uint64_t total = 0;
  GM_HIP(ctx, hipMemcpyAsync(&total, seg_dst.as<uint64_t>() + nnz, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  // part `part` of n_parts: the contiguous delivery range [glo, ghi) of the
  // whole fan-out (rows and wide rows alike are cut wherever the range ends)
  // (the deliveries per match a small host fan-out sizes its speculative capacity by)
  if (nnz) ctx->subs_per_match = std::max(1.0, double(total) / double(nnz));
  const uint64_t glo = uint64_t((unsigned __int128)total * part / n_parts);
  const uint64_t ghi = uint64_t((unsigned __int128)total * (part + 1) / n_parts);
  const uint64_t cnt = ghi - glo;
  if (first_out) *first_out = glo;
  PoolBuf ids(ctx->pool, cnt * 4 + 16);
  if (!ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "fanout: output");
  GM_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  if (cnt) {
    const uint64_t per = fan_per_block(cnt);
    const uint64_t blocks = (cnt + per - 1) / per;
    hipLaunchKernelGGL(k_fanout_copy, dim3(blocks), dim3(256), 0, st, seg_dst.as<uint64_t>(), nnz, m_ids,
                       idx->view.sub_off, idx->view.sub_ids, glo, ghi, per, ids.as<uint32_t>(), false);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  GM_HIP(ctx, hipEventSynchronize(ctx->ev[2]));
  ctx->stats.nnz = cnt;
  ctx->stats.match_kernel_ms = ev_ms(ctx->ev[1], ctx->ev[2]);
  ctx->stats.total_device_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
  return finish_csr(ctx, n, cnt, row_off, ids, dev_out, out);
}

// A small host fan-out's device work (gm_host.cpp run_fanout_small), queued
// without a wait: the deliveries' offsets, the rows' offsets and the delivery
// lists of [0, min(total, the device's count)) -- total: the call's capacity.
int queue_fanout_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint64_t* d_off, const uint32_t* d_ids,
                       uint64_t n, uint64_t nnz, uint64_t total, uint64_t* seg_dst, uint64_t* row_off, uint32_t* ids) {
  hipStream_t st = ctx->stream;
  if (nnz + 1 <= SCAN_LOOP_MAX) {
    hipLaunchKernelGGL(k_scan_loop<LoadSegLen>, dim3(1), dim3(SCAN1_T), 0, st, LoadSegLen{d_ids, idx->view.sub_off},
                       nnz, nnz + 1, seg_dst);
    GM_HIP(ctx, hipGetLastError());
  } else if (int rc = scan_excl(ctx, LoadSegLen{d_ids, idx->view.sub_off}, nnz, seg_dst)) {
    return rc;
  }
  hipLaunchKernelGGL(k_fanout_rowoff, dim3((n + 1 + 255) / 256), dim3(256), 0, st, d_off, n, seg_dst, row_off, nnz);
  GM_HIP(ctx, hipGetLastError());
  if (total) {
    const uint64_t per = fan_per_block(total);
    hipLaunchKernelGGL(k_fanout_copy, dim3((total + per - 1) / per), dim3(256), 0, st, seg_dst, nnz, d_ids,
                       idx->view.sub_off, idx->view.sub_ids, uint64_t(0), total, per, ids, true);
    GM_HIP(ctx, hipGetLastError());
  }
  return 0;
}

// The fan-out of a small host call's speculative rows, queued right behind its
// assembly (emqx_gm_match_fanout, gm_host.cpp run_host_small): d_ro/d_ids the
// speculative CSR (cap_m ids), the deliveries into cap_f -- both counts checked
// by the host after the call's one wait.
int queue_fanout_spec(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint64_t* d_ro, const uint32_t* d_ids,
                      uint64_t n, uint64_t cap_m, uint64_t cap_f, uint64_t* seg_dst, uint64_t* row_off, uint32_t* ids) {
  hipStream_t st = ctx->stream;
  const LoadSegLenSpec ld{d_ids, idx->view.sub_off, d_ro + n, uint32_t(idx->view.n_filters)};
  if (cap_m + 1 <= SCAN_LOOP_MAX) {
    hipLaunchKernelGGL(k_scan_loop<LoadSegLenSpec>, dim3(1), dim3(SCAN1_T), 0, st, ld, cap_m, cap_m + 1, seg_dst);
    GM_HIP(ctx, hipGetLastError());
  } else if (int rc = scan_excl(ctx, ld, cap_m, seg_dst)) {
    return rc;
  }
  hipLaunchKernelGGL(k_fanout_rowoff, dim3((n + 1 + 255) / 256), dim3(256), 0, st, d_ro, n, seg_dst, row_off, cap_m);
  GM_HIP(ctx, hipGetLastError());
  const uint64_t per = fan_per_block(cap_f);
  hipLaunchKernelGGL(k_fanout_copy, dim3((cap_f + per - 1) / per), dim3(256), 0, st, seg_dst, cap_m, d_ids,
                     idx->view.sub_off, idx->view.sub_ids, uint64_t(0), cap_f, per, ids, true);
  GM_HIP(ctx, hipGetLastError());
  return 0;
}

// k_fanout_rowoff for another file's segment offsets (gm_subopts.hip: a deliver
// call cuts its rows the way the fan-out does)
int launch_fanout_rowoff(hipStream_t st, const uint64_t* m_off, uint64_t n, const uint64_t* seg_dst, uint64_t* out_off,
                         uint64_t nseg) {
  hipLaunchKernelGGL(k_fanout_rowoff, dim3((n + 1 + 255) / 256), dim3(256), 0, st, m_off, n, seg_dst, out_off, nseg);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

// Rows back in their batch order after a prefix-routed exchange (sharded.py,
// gm_route.hip): out row perm[i] = input row i, the input rows packed in send
// order with u32 lengths lens[i].
__global__ __launch_bounds__(256) void k_unperm_lens(const uint32_t* __restrict__ lens, const uint32_t* __restrict__ perm,
                                                     uint64_t n, uint64_t* __restrict__ lens_out,
                                                     uint64_t* __restrict__ lens_in, uint32_t* __restrict__ inv) {
  const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (i < n) {
    lens_out[perm[i]] = lens[i];
    lens_in[i] = lens[i];
    inv[perm[i]] = uint32_t(i);
  }
}
// output row j = input row inv[j] (k_gather_segs, output-driven: one coalesced write)
struct UnpermSeg {
  const uint64_t* in_off;
  const uint32_t* inv;
  __device__ __forceinline__ SegSpan at(uint64_t j) const {
    const uint64_t a = in_off[inv[j]];
    return {a, in_off[inv[j] + 1] - a};
  }
};
int unpermute_rows(emqx_gm_ctx* ctx, uint64_t n, const uint32_t* d_perm, const uint32_t* d_lens, const uint32_t* d_ids,
                   uint32_t flags, emqx_gm_csr* out) {
  hipStream_t st = ctx->stream;
  PoolBuf row_off(ctx->pool, (n + 1) * 8), in_off(ctx->pool, (n + 1) * 8), l_out(ctx->pool, n * 8 + 8),
      l_in(ctx->pool, n * 8 + 8), inv(ctx->pool, n * 4 + 4);
  if (!row_off.p || !in_off.p || !l_out.p || !l_in.p || !inv.p)
    return set_err(ctx, EMQX_GM_ENOMEM, "unpermute_rows: workspace");
  if (n) {
    hipLaunchKernelGGL(k_unperm_lens, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, st, d_lens, d_perm, n,
                       l_out.as<uint64_t>(), l_in.as<uint64_t>(), inv.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
  }
  if (int rc = scan_lengths(ctx, l_out.as<uint64_t>(), n, row_off.as<uint64_t>())) return rc;
  if (int rc = scan_lengths(ctx, l_in.as<uint64_t>(), n, in_off.as<uint64_t>())) return rc;
  uint64_t nnz = 0;
  GM_HIP(ctx, hipMemcpyAsync(&nnz, row_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  PoolBuf ids(ctx->pool, nnz * 4 + 16);
  if (!ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "unpermute_rows: ids");
  if (n) {
    hipLaunchKernelGGL((k_gather_segs<uint32_t, UnpermSeg>), dim3(gather_blocks(n)), dim3(256), 0, st, d_ids,
                       UnpermSeg{in_off.as<uint64_t>(), inv.as<uint32_t>()}, n, row_off.as<uint64_t>(),
                       ids.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
  }
  return finish_csr(ctx, n, nnz, row_off, ids, flags & EMQX_GM_DEVICE_IO, out);
}

int run_merge_rows(emqx_gm_ctx* ctx, uint64_t n, uint64_t stride, uint32_t pieces, const uint32_t* d_lens,
                   const uint32_t* d_ids, uint32_t flags, emqx_gm_csr* out) {
  hipStream_t st = ctx->stream;
  ctx->stats = emqx_gm_match_stats{};
  ctx->stats.n_topics = n;
  const uint64_t nl = uint64_t(pieces) * stride;
  PoolBuf pos(ctx->pool, (nl + 1) * 8), row_off(ctx->pool, (n + 1) * 8);
  if (!pos.p || !row_off.p) return set_err(ctx, EMQX_GM_ENOMEM, "merge_rows: workspace");
  GM_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  int rc = scan_excl(ctx, LoadU32{d_lens}, nl, pos.as<uint64_t>());
  if (rc) return rc;
  rc = scan_excl(ctx, LoadRowSum{d_lens, stride, pieces}, n, row_off.as<uint64_t>());
  if (rc) return rc;
  uint64_t nnz = 0;
  GM_HIP(ctx, hipMemcpyAsync(&nnz, row_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  PoolBuf ids(ctx->pool, nnz * 4 + 16);
  if (!ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "merge_rows: output");
  GM_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  if (n) {
    hipLaunchKernelGGL(k_merge_rows, dim3((n + 255) / 256), dim3(256), 0, st, d_lens, pos.as<uint64_t>(), d_ids, n,
                       stride, pieces, row_off.as<uint64_t>(), ids.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  GM_HIP(ctx, hipEventSynchronize(ctx->ev[2]));
  ctx->stats.nnz = nnz;
  ctx->stats.match_kernel_ms = ev_ms(ctx->ev[1], ctx->ev[2]);
  ctx->stats.total_device_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
  return finish_csr(ctx, n, nnz, row_off, ids, flags & EMQX_GM_DEVICE_IO, out);
}

int run_row_lengths(emqx_gm_ctx* ctx, const emqx_gm_csr* csr, uint32_t* d_out) {
  if (csr->n_rows) {
    hipLaunchKernelGGL(k_row_lengths, dim3((csr->n_rows + 255) / 256), dim3(256), 0, ctx->stream, csr->row_off,
                       csr->n_rows, d_out);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// Match on an overlay snapshot: the base and the delta snapshots each match
// the batch (inputs copied to the device once), then one pass drops
// tombstoned base ids, remaps the survivors to final ids and merges the delta
// row in (both rows sorted, disjoint).
int run_match_overlay(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb_in, const uint64_t* to_in,
                      uint64_t n, uint32_t flags, emqx_gm_csr* out) {
  const OverlayState& ov = *idx->ov;
  const bool dev_io = flags & EMQX_GM_DEVICE_IO;
  hipStream_t st = ctx->stream;
  PoolBuf d_tb_own, d_to_own;
  const uint8_t* tb = tb_in;
  const uint64_t* to = to_in;
  if (!dev_io && n) {
    const uint64_t bytes = to_in[n];
    for (uint64_t i = 0; i < n; ++i)
      if (to_in[i + 1] < to_in[i]) return set_err(ctx, EMQX_GM_EINVAL, "match: topic offsets not monotone");
    d_tb_own = PoolBuf(ctx->pool, bytes + 64);
    d_to_own = PoolBuf(ctx->pool, (n + 1) * 8);
    if (!d_tb_own.p || !d_to_own.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: input workspace");
    if (bytes) GM_HIP(ctx, hipMemcpyAsync(d_tb_own.p, tb_in, bytes, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemsetAsync(static_cast<uint8_t*>(d_tb_own.p) + bytes, 0, 64, st));
    GM_HIP(ctx, hipMemcpyAsync(d_to_own.p, to_in, (n + 1) * 8, hipMemcpyHostToDevice, st));
    tb = d_tb_own.as<uint8_t>();
    to = d_to_own.as<uint64_t>();
  }
  const uint32_t sub_flags = (flags & EMQX_GM_WITH_EXACT) | EMQX_GM_DEVICE_IO;
  emqx_gm_csr cb{}, cd{};
  int rc = run_match(ctx, ov.base, tb, to, n, sub_flags, &cb);
  if (rc) return rc;
  PoolBuf b_off, b_ids, d_off, d_ids;  // adopt the sub-results' pool buffers
  b_off.pool = b_ids.pool = d_off.pool = d_ids.pool = ctx->pool;
  b_off.p = cb.row_off;
  b_ids.p = cb.ids;
  emqx_gm_match_stats st_b = ctx->stats, st_d{};
  if (ov.delta) {
    rc = run_match(ctx, ov.delta, tb, to, n, sub_flags, &cd);
    if (rc) return rc;
    d_off.p = cd.row_off;
    d_ids.p = cd.ids;
    st_d = ctx->stats;
  }
  PoolBuf row_off(ctx->pool, (n + 1) * 8);
  if (!row_off.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: row_off");
  const OvView o{ov.d_tbm, ov.d_tpre, ov.d_ins, uint32_t(ov.ins.size())};
  rc = scan_excl(ctx, LoadOvLen{cb.row_off, cb.ids, ov.delta ? cd.row_off : nullptr, o}, n, row_off.as<uint64_t>());
  if (rc) return rc;
  uint64_t nnz = 0;
  GM_HIP(ctx, hipMemcpyAsync(&nnz, row_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  PoolBuf ids(ctx->pool, nnz * 4 + 16);
  if (!ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: ids");
  if (n) {
    hipLaunchKernelGGL(k_ov_merge, dim3((n + 255) / 256), dim3(256), 0, st, cb.row_off, cb.ids,
                       ov.delta ? cd.row_off : nullptr, ov.delta ? cd.ids : nullptr, o, n, row_off.as<uint64_t>(),
                       ids.as<uint32_t>());
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipStreamSynchronize(st));
  ctx->stats = st_b;
  ctx->stats.nnz = nnz;
  ctx->stats.probes += st_d.probes;
  ctx->stats.n_overflow += st_d.n_overflow;
  ctx->stats.match_kernel_ms += st_d.match_kernel_ms;
  ctx->stats.total_device_ms += st_d.total_device_ms;
  return finish_csr(ctx, n, nnz, row_off, ids, dev_io, out);
}

}  // namespace gm
