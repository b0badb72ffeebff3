// gm_scan.h — the exclusive u64 scan every count -> scan -> write step uses
// (a match call's tile sums in gm_match.hip; segment, row and length scans in
// gm_csr.hip): scan_excl over a caller's LOAD functor (value i of the input).
// The functors live with their callers; LoadU64 is here because scan_excl's
// own second level uses it.
//
// HIP only, like gm_gather.h, and included from more than one .hip.  The
// kernels are templates except k_scan_add, which has internal linkage
// (static): each including file carries its own copy, so no file has to be
// the kernel's home and the header needs no companion .hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "gm_internal.h"

namespace gm {

// ---------------------------------------------------------------------------
// scan (u64, exclusive, n+1 outputs: out[n] = total)
// ---------------------------------------------------------------------------
constexpr int SCAN_T = 256, SCAN_V = 4, SCAN_B = SCAN_T * SCAN_V;
// one-launch form for short inputs (up to 4,096 values: a match call of up to
// 262,144 topics): one workgroup of SCAN1_T threads, SCAN1_V per thread.  (16
// per thread, 16,384 values, took 25.6 us against 14 us for the three-launch
// form at C1's 15,625 tiles: one CU's address unit serializes the lanes'
// separate lines.)
constexpr int SCAN1_T = 1024, SCAN1_V = 4, SCAN1_B = SCAN1_T * SCAN1_V;

// A second array summed alongside the scan (the main pass's per-tile probe
// counts -> the probe counter), one atomic add per workgroup: saves the
// separate reduction launch of a match call.
struct SideSum {
  const unsigned long long* a = nullptr;
  uint64_t n = 0;
  unsigned long long* acc = nullptr;
};

// Scan of one workgroup's T*V inputs (exclusive, from `pre`); returns the
// workgroup's total to every thread.  s_w: T/64 + 1 words of LDS.
template <int T, int V, class LOAD>
__device__ __forceinline__ uint64_t block_scan(LOAD load, uint64_t base, uint64_t n_in, uint64_t n_out, uint64_t pre,
                                               uint64_t* __restrict__ out, uint64_t* s_w, const SideSum& side) {
  uint64_t v[V];
  uint64_t run = 0, ssum = 0;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const uint64_t i = base + k;
    const uint64_t x = i < n_in ? load(i) : 0;
    v[k] = run;
    run += x;
    if (side.a && i < side.n) ssum += side.a[i];
  }
  // wave inclusive scan of per-thread totals
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t x = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (side.a) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ssum += __shfl_down(ssum, d, 64);
  }
  if (lane == 63) s_w[wv] = x;
  if (side.a && lane == 0) s_w[T / 64 + wv] = ssum;
  __syncthreads();
  uint64_t wpre = 0, tot = 0;
  for (int k = 0; k < T / 64; ++k) {
    wpre += k < wv ? s_w[k] : 0;
    tot += s_w[k];
  }
  const uint64_t tpre = pre + wpre + x - run;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const uint64_t i = base + k;
    if (i < n_out) out[i] = tpre + v[k];
  }
  if (side.a && threadIdx.x == 0) {
    uint64_t st = 0;
    for (int k = 0; k < T / 64; ++k) st += s_w[T / 64 + k];
    if (st) atomicAdd(side.acc, (unsigned long long)st);
  }
  return tot;
}

template <class LOAD>
__global__ __launch_bounds__(SCAN_T) void k_scan_local(LOAD load, uint64_t n_in, uint64_t n_out,
                                                        uint64_t* __restrict__ out,
                                                        uint64_t* __restrict__ block_sums, SideSum side) {
  __shared__ uint64_t s_w[2 * (SCAN_T / 64)];
  const uint64_t base = uint64_t(blockIdx.x) * SCAN_B + threadIdx.x * SCAN_V;
  const uint64_t tot = block_scan<SCAN_T, SCAN_V>(load, base, n_in, n_out, 0, out, s_w, side);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

template <class LOAD>
__global__ __launch_bounds__(SCAN1_T) void k_scan_one(LOAD load, uint64_t n_in, uint64_t n_out,
                                                       uint64_t* __restrict__ out, SideSum side,
                                                       uint64_t* __restrict__ mirror) {
  __shared__ uint64_t s_w[2 * (SCAN1_T / 64)];
  const uint64_t tot = block_scan<SCAN1_T, SCAN1_V>(load, uint64_t(threadIdx.x) * SCAN1_V, n_in, n_out, 0, out, s_w,
                                                    side);
  if (mirror && threadIdx.x == 0) *mirror = tot;  // the grand total, also at the caller's out[n]
}

// A small call's scan of up to 8 x SCAN1_B values in ONE launch: the workgroup
// walks the chunks with a running carry (a publish window's fan-out: ~5-15k
// matches, where the three-launch form idled the queue ~20 us between launches)
template <class LOAD>
__global__ __launch_bounds__(SCAN1_T) void k_scan_loop(LOAD load, uint64_t n_in, uint64_t n_out,
                                                        uint64_t* __restrict__ out) {
  __shared__ uint64_t s_w[2 * (SCAN1_T / 64)];
  uint64_t pre = 0;
  for (uint64_t b0 = 0; b0 < n_out; b0 += SCAN1_B) {
    pre += block_scan<SCAN1_T, SCAN1_V>(load, b0 + uint64_t(threadIdx.x) * SCAN1_V, n_in, n_out, pre, out, s_w,
                                        SideSum{});
    __syncthreads();  // (s_w is rewritten by the next chunk)
  }
}
constexpr uint64_t SCAN_LOOP_MAX = 8ull * SCAN1_B;

static __global__ __launch_bounds__(SCAN_T) void k_scan_add(uint64_t* __restrict__ out, uint64_t n_out,
                                                      const uint64_t* __restrict__ block_off) {
  const uint64_t base = uint64_t(blockIdx.x) * SCAN_B;
  const uint64_t add = block_off[blockIdx.x];
  for (int k = threadIdx.x; k < SCAN_B; k += SCAN_T) {
    const uint64_t i = base + k;
    if (i < n_out) out[i] += add;
  }
}

struct LoadU64 {
  const uint64_t* p;
  __device__ uint64_t operator()(uint64_t i) const { return p[i]; }
};

// Exclusive scan of n_in loaded values into out[0..n_in] (out[n_in] = total).
// split (optional): for a two-level scan, leave out[0..n_in) block-local and
// hand back the blocks' offsets in *split (out[i] + (*split)[i / SCAN_B] is the
// scan; out[n_in] is the grand total) -- the consumer adds them, one launch
// (k_scan_add) fewer.  split->p stays null when the scan was not split.
// st: the stream (default: the context's).  On another stream the scan's
// workspace goes back to the pool behind an event on that stream (the pool's
// immediate reuse assumes the context stream's order).
// split_sums (optional, with split): a scan of at most 64 blocks may hand
// back the blocks' SUMS instead (*split_sums = their count): no second launch;
// the consumer (k_assemble_c) sums the prefixes and writes out[n_in] itself.
template <class LOAD>
int scan_excl(emqx_gm_ctx* ctx, LOAD load, uint64_t n_in, uint64_t* out, SideSum side = SideSum{},
              PoolBuf* split = nullptr, hipStream_t st = nullptr, uint32_t* split_sums = nullptr) {
  if (split_sums) *split_sums = 0;
  if (!st) st = ctx->stream;
  const uint64_t n_out = n_in + 1;
  if (n_out <= uint64_t(SCAN1_B)) {  // one launch
    hipLaunchKernelGGL(k_scan_one<LOAD>, dim3(1), dim3(SCAN1_T), 0, st, load, n_in, n_out, out, side,
                       static_cast<uint64_t*>(nullptr));
    GM_HIP(ctx, hipGetLastError());
    return 0;
  }
  const uint64_t nb = (n_out + SCAN_B - 1) / SCAN_B;
  PoolBuf sums(ctx->pool, nb * 8 + 8), offs(ctx->pool, (nb + 1) * 8 + 8);
  if (!sums.p || !offs.p) return set_err(ctx, EMQX_GM_ENOMEM, "scan: workspace");
  struct Later {  // (another stream: release the workspace behind that stream's work)
    emqx_gm_ctx* c;
    hipStream_t s;
    PoolBuf* b[2];
    ~Later() {
      if (s == c->stream) return;
      for (PoolBuf* x : b)
        if (x->p) c->pool->release_after(x->release_ownership(), s);
    }
  } later{ctx, st, {&sums, &offs}};
  hipLaunchKernelGGL(k_scan_local<LOAD>, dim3(nb), dim3(SCAN_T), 0, st, load, n_in, n_out, out,
                     sums.as<uint64_t>(), side);
  if (split && split_sums && nb <= 64) {
    GM_HIP(ctx, hipGetLastError());
    *split = std::move(sums);
    *split_sums = uint32_t(nb);
    return 0;
  }
  if (split && nb + 1 <= uint64_t(SCAN1_B)) {  // the blocks' offsets, and the total into out[n_in]
    hipLaunchKernelGGL(k_scan_one<LoadU64>, dim3(1), dim3(SCAN1_T), 0, st, LoadU64{sums.as<uint64_t>()}, nb,
                       nb + 1, offs.as<uint64_t>(), SideSum{}, out + n_in);
    GM_HIP(ctx, hipGetLastError());
    *split = std::move(offs);
    return 0;
  }
  if (nb > 1) {
    int rc = scan_excl(ctx, LoadU64{sums.as<uint64_t>()}, nb, offs.as<uint64_t>(), SideSum{}, nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(SCAN_T), 0, st, out, n_out, offs.as<uint64_t>());
  }
  GM_HIP(ctx, hipGetLastError());
  return 0;
}
}  // namespace gm
