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

}  // namespace

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
