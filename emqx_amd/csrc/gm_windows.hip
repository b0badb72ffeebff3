// gm_windows.hip — k_rows_split: a group of publish windows matched as one
// device batch (gm_host.cpp run_host_windows), its CSR cut back into one
// result per window, straight into each window's page-locked host result.
//
// Inputs: the group's device CSR (row_off u64[n + 1], ids within a speculative
// capacity), or two of them -- matches and deliveries, blockIdx.z picks, as
// k_copy_u32x2 does two copies in one launch -- and the window table: per
// window and CSR a WinSlice {row0, n_rows, ids_cap, dst_row_off, dst_ids}, the
// destinations as the device addresses the windows' host results.
//
// Mapping: one grid row per window (blockIdx.y), blockIdx.x strides over that
// window's offsets and ids.  The slice is uniform per workgroup, so it comes in
// through scalar loads and no lane searches for its window; the other choice,
// a flat element index searched in an LDS copy of the table, balances uneven
// windows better but pays a 6..8-step search per element for groups whose
// windows are, on the NIF's path, of one size (a scheduler's publish window).
// Grid rows of short windows end after one bounds check.
//
// A window's ids start at an arbitrary 4-B offset of the group's array, so the
// source is not 16-B aligned: a lane reads its four ids with dword loads (the
// four of a wave fall into the same lines) and writes them as ONE 16-B store
// -- the destination is 16-B aligned, and the host-bound side is the one that
// pays per store.  Plain vector stores only, no atomics, no waits between
// workgroups; __threadfence_system() before the end, as in k_copy_u32x2.
//
// A group of WHOLE publish windows (emqx_gm_publish_windows, gm_publish.hip)
// cuts its side results here too: the picks' two CSRs, members and slots over
// one shared row_off, are k_rows_split's two planes as they are; the forward
// plan, one list per node, is cut by k_plan_bounds + k_plan_cut below.  The
// reference does this work per message in each publisher's process
// (emqx_broker:publish/1 -> route/2, apps/emqx/src/emqx_broker.erl:204-215,
// 245-293; emqx_shared_sub:dispatch/3, emqx_shared_sub.erl:113-130).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_internal.h"

namespace gm {
namespace {

__global__ __launch_bounds__(256) void k_rows_split(const WinSlice* __restrict__ tab,
                                                    const uint64_t* __restrict__ ro0, const uint32_t* __restrict__ ids0,
                                                    uint64_t cap0, const uint64_t* __restrict__ ro1,
                                                    const uint32_t* __restrict__ ids1, uint64_t cap1) {
  const WinSlice s = tab[blockIdx.y * 2u + blockIdx.z];
  const uint64_t* __restrict__ ro = blockIdx.z ? ro1 : ro0;
  const uint32_t* __restrict__ ids = blockIdx.z ? ids1 : ids0;
  const uint64_t cap = blockIdx.z ? cap1 : cap0;  // the group's own speculative capacity
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x, stride = uint64_t(gridDim.x) * 256u;
  const uint64_t base = ro[s.row0];
  // the offsets rebased to the window, all n_rows + 1 of them: the last one is
  // the window's true length whatever fits, so the host sees an overflow
  for (uint64_t i = t; i <= s.n_rows; i += stride) s.dst_row_off[i] = ro[s.row0 + i] - base;
  // the ids the window's capacity holds, never one at or past the group's
  uint64_t m = min(ro[s.row0 + s.n_rows] - base, s.ids_cap);
  m = base < cap ? min(m, cap - base) : 0;
  const uint32_t* __restrict__ src = ids + base;
  const uint64_t q = m / 4;
  for (uint64_t i = t; i < q; i += stride) {
    const uint32_t* p = src + 4 * i;
    reinterpret_cast<uint4*>(s.dst_ids)[i] = make_uint4(p[0], p[1], p[2], p[3]);
  }
  if (t < (m & 3)) s.dst_ids[q * 4 + t] = src[q * 4 + t];
  __threadfence_system();  // (host-bound stores visible before the call's end event)
}

// ---- the cut of a group's forward plan (gm_publish.hip, emqx_gm_publish_windows) ----
// The group's plan lists each node's (row, filter) pairs in batch order, and a
// window is a contiguous range of the group's rows: window w's pairs on node k
// are ONE run of node k's list, the entries with row0[w] <= row < row0[w + 1].
//
// k_plan_bounds: one lane per (window boundary b, node k) finds by binary search
// how many entries of node k's list have a row below row0[b]: lb[b][k] (a lower
// bound on the row, so a row with several filters on one node lands whole in its
// window).  lb[0][k] = 0 and lb[g][k] = the list's length.
__global__ __launch_bounds__(256) void k_plan_bounds(const uint32_t* __restrict__ win_row0, uint32_t g,
                                                     const uint64_t* __restrict__ node_off,
                                                     const uint32_t* __restrict__ rows, uint32_t n_nodes,
                                                     uint64_t cap_pairs, uint32_t* __restrict__ lb) {
  const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (i >= (uint64_t(g) + 1) * n_nodes) return;
  const uint32_t b = uint32_t(i / n_nodes), k = uint32_t(i % n_nodes);
  const uint64_t a = min(node_off[k], cap_pairs), e = max(a, min(node_off[k + 1], cap_pairs));
  const uint32_t want = win_row0[b];
  uint64_t lo = a, hi = e;  // the first entry of [a, e) with rows[] >= want
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (rows[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  lb[i] = uint32_t(lo - a);
}

// k_plan_cut: grid (x, window).  Every workgroup builds its window's node
// offsets in LDS -- an exclusive scan over lb[w + 1][k] - lb[w][k], n_nodes <=
// 4096: 16 KiB, what k_fw_hist uses -- and workgroup x = 0 stores them, as u64,
// to the window's host node_off (the last one is the window's true pair count,
// whatever fits).  Then the lanes stride over the window's pairs four at a
// time: the node of the first by a search in the LDS offsets, the next three by
// stepping on; a pair's source is node_off[k] + lb[w][k] + its place in the run,
// its row rebased by row0[w]; one 16-B store each to the window's rows and
// filters.  The window's row_routes are a plain slice, copied as k_rows_split
// copies ids.  The order depends on indices only: no atomics, no wait between
// workgroups, plain vector stores, __threadfence_system() before the end.
__global__ __launch_bounds__(256) void k_plan_cut(const PlanSlice* __restrict__ tab, const uint32_t* __restrict__ lb,
                                                  const uint64_t* __restrict__ node_off,
                                                  const uint32_t* __restrict__ rows,
                                                  const uint32_t* __restrict__ filters,
                                                  const uint32_t* __restrict__ row_routes, uint32_t n_nodes,
                                                  uint64_t cap_pairs, const uint64_t* __restrict__ total_p,
                                                  uint64_t* __restrict__ total_out) {
  extern __shared__ uint32_t s_off[];  // [n_nodes + 1], then the waves' sums [4]
  uint32_t* s_w = s_off + n_nodes + 1;
  const PlanSlice s = tab[blockIdx.y];
  const uint32_t* __restrict__ lb0 = lb + uint64_t(blockIdx.y) * n_nodes;
  const uint32_t* __restrict__ lb1 = lb0 + n_nodes;
  // the scan: a thread's consecutive nodes, the waves' lanes, the four waves
  const uint32_t per = (n_nodes + 255u) / 256u, k0 = min(threadIdx.x * per, n_nodes), k1 = min(k0 + per, n_nodes);
  uint32_t run = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t a = lb0[k], b = lb1[k];
    run += b > a ? b - a : 0;
  }
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t x = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  uint32_t pre = x - run;
  for (uint32_t k = 0; k < wv; ++k) pre += s_w[k];
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t a = lb0[k], b = lb1[k];
    s_off[k] = pre;
    pre += b > a ? b - a : 0;
  }
  if (threadIdx.x == 255) s_off[n_nodes] = pre;  // (the last thread's nodes end the list: the total)
  __syncthreads();
  if (blockIdx.x == 0) {
    for (uint32_t k = threadIdx.x; k <= n_nodes; k += 256u) s.dst_node_off[k] = s_off[k];
    if (blockIdx.y == 0 && threadIdx.x == 0) *total_out = *total_p;  // the group's true pair count
  }
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x, stride = uint64_t(gridDim.x) * 256u;
  const uint32_t total = s_off[n_nodes];
  const uint32_t m = uint32_t(min(uint64_t(total), s.pairs_cap));
  const uint32_t row0 = uint32_t(s.row0);
  const uint64_t last = cap_pairs - 1;  // (m > 0 only with cap_pairs > 0)
  const uint32_t q = m / 4;
  for (uint64_t i = t; i < q + ((m & 3) ? 1u : 0u); i += stride) {
    const uint32_t e0 = uint32_t(i) * 4u, cnt = i < q ? 4u : (m & 3u);
    uint32_t lo = 0, hi = n_nodes;  // the last node k with s_off[k] <= e0
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (s_off[mid] <= e0) lo = mid;
      else hi = mid;
    }
    uint32_t r[4] = {0, 0, 0, 0}, f[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (j < cnt) {
        const uint32_t e = e0 + j;
        while (e >= s_off[lo + 1]) ++lo;  // (e < total = s_off[n_nodes]: lo stays below n_nodes)
        const uint64_t src = min(node_off[lo] + lb0[lo] + (e - s_off[lo]), last);
        r[j] = rows[src] - row0;
        f[j] = filters[src];
      }
    }
    if (cnt == 4) {
      reinterpret_cast<uint4*>(s.dst_rows)[i] = make_uint4(r[0], r[1], r[2], r[3]);
      reinterpret_cast<uint4*>(s.dst_filters)[i] = make_uint4(f[0], f[1], f[2], f[3]);
    } else {
      for (uint32_t j = 0; j < cnt; ++j) {
        s.dst_rows[e0 + j] = r[j];
        s.dst_filters[e0 + j] = f[j];
      }
    }
  }
  // the window's row_routes: a slice at an arbitrary 4-B offset, dword loads and one 16-B store
  const uint32_t* __restrict__ src = row_routes + s.row0;
  const uint64_t rq = s.n_rows / 4;
  for (uint64_t i = t; i < rq; i += stride) {
    const uint32_t* p = src + 4 * i;
    reinterpret_cast<uint4*>(s.dst_row_routes)[i] = make_uint4(p[0], p[1], p[2], p[3]);
  }
  if (t < (s.n_rows & 3)) s.dst_row_routes[rq * 4 + t] = src[rq * 4 + t];
  __threadfence_system();  // (host-bound stores visible before the call's end event)
}

}  // namespace

int launch_plan_cut(hipStream_t st, const PlanSlice* tab, uint32_t n_windows, uint64_t max_work,
                    const uint32_t* win_row0, uint32_t* lb, bool bounds, const uint64_t* node_off, const uint32_t* rows,
                    const uint32_t* filters, const uint32_t* row_routes, uint32_t n_nodes, uint64_t cap_pairs,
                    const uint64_t* total_p, uint64_t* total_out) {
  if (!n_windows || !n_nodes) return 0;
  if (bounds) {
    const uint64_t lanes = (uint64_t(n_windows) + 1) * n_nodes;
    hipLaunchKernelGGL(k_plan_bounds, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, st, win_row0, n_windows,
                       node_off, rows, n_nodes, cap_pairs, lb);
    if (hipGetLastError() != hipSuccess) return EMQX_GM_EDEVICE;
  }
  // blocks per window: enough for the largest window's 16-B units, at most 8 (each repeats the window's scan)
  const uint32_t gx = uint32_t(std::min<uint64_t>(8, std::max<uint64_t>(1, (max_work + 255) / 256)));
  hipLaunchKernelGGL(k_plan_cut, dim3(gx, n_windows), dim3(256), (size_t(n_nodes) + 1 + 4) * 4, st, tab, lb, node_off,
                     rows, filters, row_routes, n_nodes, cap_pairs, total_p, total_out);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

int launch_rows_split(hipStream_t st, const WinSlice* tab, uint32_t n_windows, uint64_t max_work, const uint64_t* ro0,
                      const uint32_t* ids0, uint64_t cap0, const uint64_t* ro1, const uint32_t* ids1, uint64_t cap1) {
  if (!n_windows) return 0;
  // blocks per window: enough for the largest window's offsets or 16-B id units, at most 32
  const uint32_t gx = uint32_t(std::min<uint64_t>(32, std::max<uint64_t>(1, (max_work + 255) / 256)));
  hipLaunchKernelGGL(k_rows_split, dim3(gx, n_windows, ro1 ? 2 : 1), dim3(256), 0, st, tab, ro0, ids0, cap0, ro1, ids1,
                     cap1);
  return hipGetLastError() == hipSuccess ? 0 : EMQX_GM_EDEVICE;
}

}  // namespace gm
