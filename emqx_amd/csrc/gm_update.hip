// gm_update.hip — CDNA4 (gfx950) kernels and host drivers for the device side
// of in-place index updates.
//
//   patch_update (gm_overlay.cpp) -> apply_patch_device / _gmap: the new blob =
//                  the old one with the host-patched byte ranges scattered in
//                  (k_patch_scatter), flag bits set or cleared (k_patch_or) and
//                  every filter-id field renumbered by the update's id shift
//                  (k_shift_table builds its table; k_renumber_copy renumbers
//                  while copying, k_renumber in place).
//   a sharded update (gm_shard.cpp) -> k_gmap_shift: a shard's new
//                  local-to-global id map (shift_gmap_device, or queued behind
//                  the patch).
//   update_subs (gm_subs.cpp) -> the new subscriber CSR: k_soff_shift and
//                  k_subs_copy (shift_subs_device, rebuild_subs_device), and
//                  gather_segments for lists read back by the host.
//
// None of this runs during a match call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "gm_internal.h"

namespace gm {

// ---- in-place update (gm_overlay.cpp, patch_update) -----------------------
// The host-patched byte ranges, cut into pieces of <= PATCH_PIECE bytes, one
// workgroup per piece: desc[3b..3b+2] = (offset in the blob, offset in the
// payload, bytes).
constexpr uint32_t PATCH_PIECE = 4096;
__global__ __launch_bounds__(256) void k_patch_scatter(uint8_t* __restrict__ dst, const uint64_t* __restrict__ desc,
                                                       const uint8_t* __restrict__ pay) {
  const uint64_t d = desc[3 * blockIdx.x], p = desc[3 * blockIdx.x + 1], n = desc[3 * blockIdx.x + 2];
  for (uint64_t i = threadIdx.x; i < n; i += 256) dst[d + i] = pay[p + i];
}
// The id table of an in-place update (IdShift::map, gm_internal.h), built on
// the device from the O(delta) lists: dels (prev ids deleted, ascending) and
// addpos (per new filter, byte order: prev filters sorting before it).
__device__ __forceinline__ uint32_t count_below(const uint32_t* a, uint32_t n, uint32_t x) {  // a[i] < x
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (a[m] < x) lo = m + 1;
    else hi = m;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_shift_table(uint32_t* __restrict__ rmap, uint64_t nb,
                                                     const uint32_t* __restrict__ dels, uint32_t nd,
                                                     const uint32_t* __restrict__ addpos, uint32_t na) {
  const uint64_t id = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (id >= nb + na) return;
  if (id >= nb) {
    const uint32_t k = uint32_t(id - nb), p = addpos[k];
    rmap[id] = p - count_below(dels, nd, p) + k;
    return;
  }
  const uint32_t x = uint32_t(id), below = count_below(dels, nd, x);
  if (below < nd && dels[below] == x) {
    rmap[id] = NONE;
    return;
  }
  rmap[id] = x - below + count_below(addpos, na, x + 1);  // inserts at or before it
}
// A shard's new local-to-global id map after a sharded update (gm_shard.cpp,
// GmapJob): rows leave the device through view.gmap[local id], and one insert
// anywhere shifts global ids on every shard.  For every old or temporary local
// id i < nb + na: j = rmap[i] (the shard's local shift, k_shift_table's table;
// nullptr: the identity; NONE: deleted), new_gmap[j] = G(old_gmap[i]) for a
// surviving filter, add_gid[i - nb] for a new one, with G(g) = g - (gdels < g)
// + (gadds <= g) the GLOBAL shift.  old_gmap ascends, so the 256 elements of a
// tile bracket a narrow window of gdels / gadds: four lanes find it with full
// searches on the tile's first and last element, the windows are staged in LDS
// when they fit, and each lane searches only inside them.  A streaming pass:
// 4 B read and 4 B written per filter (writes monotone in i).
constexpr uint32_t GMAP_WIN = 1024;
__global__ __launch_bounds__(256) void k_gmap_shift(const uint32_t* __restrict__ old_gmap, uint32_t nb, uint32_t na,
                                                    const uint32_t* __restrict__ rmap,
                                                    const uint32_t* __restrict__ add_gid,
                                                    const uint32_t* __restrict__ gdels, uint32_t gnd,
                                                    const uint32_t* __restrict__ gadds, uint32_t gna,
                                                    uint32_t* __restrict__ new_gmap, uint32_t n_new) {
  __shared__ uint32_t s_d[GMAP_WIN], s_a[GMAP_WIN];
  __shared__ uint32_t s_w[4];  // dels window [0], [1]; adds window [2], [3]
  const uint64_t n_map = uint64_t(nb) + na;
  for (uint64_t base = uint64_t(blockIdx.x) * 256u; base < n_map; base += uint64_t(gridDim.x) * 256u) {
    uint32_t d_lo = 0, d_hi = 0, a_lo = 0, a_hi = 0;
    bool ld = false, la = false;
    if (base < nb) {  // (block-uniform) the tile's old ids: [base, hi)
      const uint32_t hi = uint32_t(min(base + 256u, uint64_t(nb)));
      if (threadIdx.x < 4) {
        const uint32_t g = old_gmap[(threadIdx.x & 1) ? hi - 1 : uint32_t(base)];
        s_w[threadIdx.x] = threadIdx.x < 2 ? count_below(gdels, gnd, g) : count_below(gadds, gna, g + 1);
      }
      __syncthreads();
      d_lo = s_w[0], d_hi = max(s_w[0], s_w[1]), a_lo = s_w[2], a_hi = max(s_w[2], s_w[3]);
      ld = d_hi - d_lo <= GMAP_WIN;
      la = a_hi - a_lo <= GMAP_WIN;
      if (ld)
        for (uint32_t k = threadIdx.x; k < d_hi - d_lo; k += 256) s_d[k] = gdels[d_lo + k];
      if (la)
        for (uint32_t k = threadIdx.x; k < a_hi - a_lo; k += 256) s_a[k] = gadds[a_lo + k];
      __syncthreads();
    }
    const uint64_t i = base + threadIdx.x;
    if (i < n_map) {
      const uint32_t j = rmap ? rmap[i] : uint32_t(i);
      if (j != NONE && j < n_new) {
        if (i >= nb) {
          new_gmap[j] = add_gid[i - nb];
        } else {
          const uint32_t g = old_gmap[i];
          const uint32_t below = d_lo + (ld ? count_below(s_d, d_hi - d_lo, g) : count_below(gdels + d_lo, d_hi - d_lo, g));
          const uint32_t ins =
              a_lo + (la ? count_below(s_a, a_hi - a_lo, g + 1) : count_below(gadds + a_lo, a_hi - a_lo, g + 1));
          new_gmap[j] = g - below + ins;
        }
      }
    }
    __syncthreads();  // (the next tile restages the windows)
  }
}
// Flag bits set on words whose other bits are filter ids (HOT_PLUS on hf /
// p_hf): the host mirror's ids are stale (not renumbered), so these go as ORs.
__global__ __launch_bounds__(256) void k_patch_or(uint32_t* __restrict__ dst, const uint64_t* __restrict__ ops,
                                                  uint64_t n) {
  const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = ops[2 * i];
  if (off & PATCH_AND) atomicAnd(dst + ((off & ~PATCH_AND) >> 2), ~uint32_t(ops[2 * i + 1]));
  else atomicOr(dst + (off >> 2), uint32_t(ops[2 * i + 1]));
}
// Every filter-id field renumbered (renum_field, the device twin of
// gm_overlay.cpp's renumber_host): hot slots [0, n_hot), nodes [0, n_nodes).
__global__ __launch_bounds__(256) void k_renumber(HotSlot* __restrict__ hot, uint64_t n_hot, Node* __restrict__ nodes,
                                                  uint64_t n_nodes, const uint32_t* __restrict__ rmap) {
  const uint64_t stride = uint64_t(gridDim.x) * 256u;
  for (uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x; s < n_hot; s += stride) {
    HotSlot h = hot[s];
    if (h.key == EDGE_EMPTY) continue;
    h.hf = renum_field(h.hf, HF_NONE, HF_FLAGS, rmap);
    h.end_filter = renum_field(h.end_filter, NONE, END_WILD, rmap);
    h.p_hf = renum_field(h.p_hf, HF_NONE, HF_FLAGS, rmap);
    h.p_end = renum_field(h.p_end, NONE, END_WILD, rmap);
    hot[s] = h;
  }
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n_nodes; i += stride) {
    Node nd = nodes[i];
    nd.hash_filter = renum_field(nd.hash_filter, NONE, 0, rmap);
    nd.end_filter = renum_field(nd.end_filter, NONE, 0, rmap);
    nodes[i] = nd;
  }
}

// k_renumber fused with the blob copy: dst's hot slots and nodes = src's,
// renumbered (every slot written, empty ones as they are), so an update reads
// and writes the id-bearing tables once instead of copying them and then
// renumbering them in place (C5: ~26 of the 38 GB blob)
__global__ __launch_bounds__(256) void k_renumber_copy(const HotSlot* __restrict__ shot, HotSlot* __restrict__ hot,
                                                       uint64_t n_hot, const Node* __restrict__ snodes,
                                                       Node* __restrict__ nodes, uint64_t n_nodes,
                                                       const uint32_t* __restrict__ rmap) {
  const uint64_t stride = uint64_t(gridDim.x) * 256u;
  for (uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x; s < n_hot; s += stride) {
    HotSlot h = shot[s];
    if (h.key != EDGE_EMPTY) {
      h.hf = renum_field(h.hf, HF_NONE, HF_FLAGS, rmap);
      h.end_filter = renum_field(h.end_filter, NONE, END_WILD, rmap);
      h.p_hf = renum_field(h.p_hf, HF_NONE, HF_FLAGS, rmap);
      h.p_end = renum_field(h.p_end, NONE, END_WILD, rmap);
    }
    hot[s] = h;
  }
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n_nodes; i += stride) {
    Node nd = snodes[i];
    nd.hash_filter = renum_field(nd.hash_filter, NONE, 0, rmap);
    nd.end_filter = renum_field(nd.end_filter, NONE, 0, rmap);
    nodes[i] = nd;
  }
}

namespace {
// The filter-id fields of the records k_renumber rewrites: (offset, empty value, flag bits)
struct IdField {
  uint32_t off, none, flag;
};
constexpr IdField kHotIds[] = {{offsetof(HotSlot, hf), HF_NONE, HF_FLAGS},
                               {offsetof(HotSlot, end_filter), NONE, END_WILD},
                               {offsetof(HotSlot, p_hf), HF_NONE, HF_FLAGS},
                               {offsetof(HotSlot, p_end), NONE, END_WILD}};
constexpr IdField kNodeIds[] = {{offsetof(Node, hash_filter), NONE, 0u}, {offsetof(Node, end_filter), NONE, 0u}};
// The id fields of the table [o, o + n * rec) lying inside the patched range
// [a, b) (buf = its bytes), renumbered in place by the shift (IdShift::map:
// O(log delta) per field).  false: a field holds an id outside the shift.
template <size_t K>
bool renum_payload(uint8_t* buf, uint64_t a, uint64_t b, uint64_t o, uint64_t n, uint64_t rec,
                   const IdField (&fs)[K], const IdShift& sh, uint64_t n_map) {
  const uint64_t lo = std::max(a, o), hi = std::min(b, o + n * rec);
  for (uint64_t r = lo < hi ? (lo - o) / rec : 0, re = lo < hi ? (hi - o + rec - 1) / rec : 0; r < re; ++r)
    for (const IdField& f : fs) {
      const uint64_t at = o + r * rec + f.off;
      if (at < a || at + 4 > b) continue;  // (the patcher writes id fields whole)
      uint32_t x;
      std::memcpy(&x, buf + (at - a), 4);
      const uint32_t id = x & ~f.flag;
      if (x != f.none && id != (f.none & ~f.flag) && id >= n_map) return false;
      x = renum_field(x, f.none, f.flag, sh);
      std::memcpy(buf + (at - a), &x, 4);
    }
  return true;
}
}  // namespace

namespace {
// k_gmap_shift queued on ctx's stream: the global shift's lists and the new
// filters' ids go up in one copy (stage / dbuf: kept by the caller until it has
// synchronized the stream); rmap: the local shift's device table (n_map
// entries), or nullptr for a shard without local changes.
int queue_gmap_shift(emqx_gm_ctx* ctx, const GmapJob& job, const uint32_t* rmap, uint64_t n_map,
                     std::vector<uint32_t>& stage, PoolBuf& dbuf) {
  const IdShift& G = *job.sh.G;
  const std::vector<uint32_t>& ag = *job.sh.add_gid;
  const uint64_t gnd = G.dels.size(), gna = G.addpos.size(), na = ag.size();
  if (job.nb + na != n_map || (!rmap && na) || (job.nb && !job.old_gmap) || !job.new_gmap ||
      job.nb + na >= 0xFFFFFFFFull || G.nb + gna >= 0xFFFFFFFFull)
    return set_err(ctx, EMQX_GM_EINVAL, "index_update: id map job");
  if (!n_map) return EMQX_GM_OK;
  stage.resize(gnd + gna + na + 1);
  for (uint64_t k = 0; k < gnd; ++k) stage[k] = uint32_t(G.dels[k]);
  for (uint64_t k = 0; k < gna; ++k) stage[gnd + k] = uint32_t(G.addpos[k]);
  for (uint64_t k = 0; k < na; ++k) stage[gnd + gna + k] = ag[k];
  dbuf = PoolBuf(ctx->pool, stage.size() * 4);
  if (!dbuf.p) return set_err(ctx, EMQX_GM_ENOMEM, "index_update: id map staging");
  hipStream_t s = ctx->stream;
  GM_HIP(ctx, hipMemcpyAsync(dbuf.p, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, s));
  const uint32_t* D = dbuf.as<uint32_t>();
  const uint64_t g = std::min<uint64_t>(4096, (n_map + 255) / 256);
  hipLaunchKernelGGL(k_gmap_shift, dim3(uint32_t(g)), dim3(256), 0, s, job.old_gmap, uint32_t(job.nb), uint32_t(na),
                     rmap, D + gnd + gna, D, uint32_t(gnd), D + gnd, uint32_t(gna), job.new_gmap, uint32_t(job.n_new));
  GM_HIP(ctx, hipGetLastError());
  return EMQX_GM_OK;
}
}  // namespace

int shift_gmap_device(emqx_gm_ctx* ctx, const GmapJob& job) {
  std::vector<uint32_t> stage;
  PoolBuf dbuf;
  if (const int rc = queue_gmap_shift(ctx, job, nullptr, job.nb, stage, dbuf)) return rc;
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return EMQX_GM_OK;
}

int apply_patch_device(emqx_gm_ctx* ctx, void* dst, const void* src, size_t bytes,
                       const std::vector<std::pair<uint64_t, uint32_t>>& ranges, const uint8_t* host,
                       const IndexView& v, uint64_t o_hot, uint64_t o_nodes, uint64_t n_nodes,
                       const IdShift& shift, const std::vector<std::pair<uint64_t, uint32_t>>& orops) {
  return apply_patch_device_gmap(ctx, dst, src, bytes, ranges, host, v, o_hot, o_nodes, n_nodes, shift, orops, nullptr);
}

int apply_patch_device_gmap(emqx_gm_ctx* ctx, void* dst, const void* src, size_t bytes,
                            const std::vector<std::pair<uint64_t, uint32_t>>& ranges, const uint8_t* host,
                            const IndexView& v, uint64_t o_hot, uint64_t o_nodes, uint64_t n_nodes,
                            const IdShift& shift, const std::vector<std::pair<uint64_t, uint32_t>>& orops,
                            const GmapJob* gmap) {
  uint64_t n_hot = 0;
  for (int t = 0; t < HOT_TABLES; ++t) n_hot = std::max<uint64_t>(n_hot, v.hot_off[t] + v.hot_cap[t]);
  const uint64_t hot_end = o_hot + n_hot * sizeof(HotSlot), nodes_end = o_nodes + n_nodes * sizeof(Node);
  if (hot_end > bytes || nodes_end > bytes) return set_err(ctx, EMQX_GM_EINVAL, "index_update: tables outside the blob");
  const bool unfused = knob("GM_UPDATE_UNFUSED") != nullptr;
  // fused (one pass): the two id-bearing tables must not overlap
  const bool fused = !unfused && (hot_end <= o_nodes || nodes_end <= o_hot);
  // coalesce overlapping / adjacent ranges only (the bytes between two written
  // fields may differ: the host mirror's untouched filter ids are stale), then
  // cut into pieces
  std::vector<std::pair<uint64_t, uint64_t>> seg;  // [begin, end)
  {
    std::vector<std::pair<uint64_t, uint32_t>> r(ranges);
    std::sort(r.begin(), r.end());
    for (const auto& x : r) {
      if (!x.second) continue;
      if (x.first + x.second > bytes) return set_err(ctx, EMQX_GM_EINVAL, "index_update: patch outside the blob");
      if (!seg.empty() && x.first <= seg.back().second) seg.back().second = std::max(seg.back().second, x.first + x.second);
      else seg.emplace_back(x.first, x.first + x.second);
    }
  }
  for (const auto& o : orops)
    if ((o.first & 3) || (o.first & ~PATCH_AND) + 4 > bytes)
      return set_err(ctx, EMQX_GM_EINVAL, "index_update: OR/AND op outside the blob");
  std::vector<uint64_t> desc;
  uint64_t pay_n = 0;
  for (const auto& g : seg) {
    for (uint64_t b = g.first; b < g.second; b += PATCH_PIECE) {
      const uint64_t n = std::min<uint64_t>(PATCH_PIECE, g.second - b);
      desc.insert(desc.end(), {b, pay_n + (b - g.first), n});
    }
    pay_n += g.second - g.first;
  }
  const uint64_t n_pieces = desc.size() / 3;
  if (n_pieces > 0x7FFFFFFFull) return set_err(ctx, EMQX_GM_EINVAL, "index_update: patch too large");
  // staging: desc | payload | dels | addpos | OR ops (one upload); the id table after them (device-built)
  const uint64_t nd = shift.dels.size(), na = shift.addpos.size(), n_map = shift.nb + na;
  const size_t o_pay = (desc.size() * 8 + 255) & ~size_t(255);
  const size_t o_dels = (o_pay + pay_n + 255) & ~size_t(255);
  const size_t o_adds = (o_dels + nd * 4 + 4 + 255) & ~size_t(255);
  const size_t o_ors = (o_adds + na * 4 + 4 + 255) & ~size_t(255);
  const size_t up = o_ors + orops.size() * 16 + 16;
  const size_t o_rmap = (up + 255) & ~size_t(255);
  const size_t total = o_rmap + n_map * 4 + 4;
  std::vector<uint8_t> st(up, 0);
  if (!desc.empty()) std::memcpy(st.data(), desc.data(), desc.size() * 8);
  {
    uint64_t q = o_pay;
    for (const auto& g : seg) {
      uint8_t* const pb = st.data() + q;
      std::memcpy(pb, host + g.first, g.second - g.first);
      // fused: the range's filter ids (this update's temporary numbering) go up final
      if (fused && !(renum_payload(pb, g.first, g.second, o_hot, n_hot, sizeof(HotSlot), kHotIds, shift, n_map) &&
                     renum_payload(pb, g.first, g.second, o_nodes, n_nodes, sizeof(Node), kNodeIds, shift, n_map)))
        return set_err(ctx, EMQX_GM_EINVAL, "index_update: a patched filter id outside the update's ids");
      q += g.second - g.first;
    }
  }
  for (uint64_t k = 0; k < nd; ++k) reinterpret_cast<uint32_t*>(st.data() + o_dels)[k] = uint32_t(shift.dels[k]);
  for (uint64_t k = 0; k < na; ++k) reinterpret_cast<uint32_t*>(st.data() + o_adds)[k] = uint32_t(shift.addpos[k]);
  for (size_t k = 0; k < orops.size(); ++k) {
    const uint64_t w[2] = {orops[k].first, orops[k].second};
    std::memcpy(st.data() + o_ors + 16 * k, w, 16);
  }
  PoolBuf dbuf(ctx->pool, total);
  if (!dbuf.p) return set_err(ctx, EMQX_GM_ENOMEM, "index_update: staging buffer");
  hipStream_t s = ctx->stream;
  uint8_t* D = static_cast<uint8_t*>(dst);
  const uint8_t* S = dbuf.as<uint8_t>();
  uint32_t* const RM = reinterpret_cast<uint32_t*>(dbuf.as<uint8_t>() + o_rmap);
  auto shift_table = [&]() -> int {
    if (n_map) {
      hipLaunchKernelGGL(k_shift_table, dim3(uint32_t((n_map + 255) / 256)), dim3(256), 0, s, RM, shift.nb,
                         reinterpret_cast<const uint32_t*>(S + o_dels), uint32_t(nd),
                         reinterpret_cast<const uint32_t*>(S + o_adds), uint32_t(na));
      GM_HIP(ctx, hipGetLastError());
    }
    return 0;
  };
  const uint64_t g = std::min<uint64_t>(8192, (std::max(n_hot, n_nodes) + 255) / 256);
  if (fused) {
    GM_HIP(ctx, hipMemcpyAsync(dbuf.p, st.data(), up, hipMemcpyHostToDevice, s));
    if (const int rc = shift_table()) return rc;
    // the bytes around the two tables as they are, the tables renumbered on the way
    const uint64_t a0 = std::min(o_hot, o_nodes), a1 = std::min(hot_end, nodes_end);
    const uint64_t b0 = std::max(o_hot, o_nodes), b1 = std::max(hot_end, nodes_end);
    const uint64_t gaps[3][2] = {{0, a0}, {a1, b0}, {b1, bytes}};
    for (const auto& gp : gaps)
      if (gp[1] > gp[0])
        GM_HIP(ctx, hipMemcpyAsync(D + gp[0], static_cast<const uint8_t*>(src) + gp[0], gp[1] - gp[0],
                                   hipMemcpyDeviceToDevice, s));
    const uint8_t* SRC = static_cast<const uint8_t*>(src);
    hipLaunchKernelGGL(k_renumber_copy, dim3(uint32_t(g ? g : 1)), dim3(256), 0, s,
                       reinterpret_cast<const HotSlot*>(SRC + o_hot), reinterpret_cast<HotSlot*>(D + o_hot), n_hot,
                       reinterpret_cast<const Node*>(SRC + o_nodes), reinterpret_cast<Node*>(D + o_nodes), n_nodes, RM);
    GM_HIP(ctx, hipGetLastError());
  } else {
    GM_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    GM_HIP(ctx, hipMemcpyAsync(dbuf.p, st.data(), up, hipMemcpyHostToDevice, s));
  }
  if (n_pieces) {
    hipLaunchKernelGGL(k_patch_scatter, dim3(uint32_t(n_pieces)), dim3(256), 0, s, D,
                       reinterpret_cast<const uint64_t*>(S), S + o_pay);
    GM_HIP(ctx, hipGetLastError());
  }
  if (!orops.empty()) {
    hipLaunchKernelGGL(k_patch_or, dim3(uint32_t((orops.size() + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<uint32_t*>(D), reinterpret_cast<const uint64_t*>(S + o_ors),
                       uint64_t(orops.size()));
    GM_HIP(ctx, hipGetLastError());
  }
  if (!fused) {
    if (const int rc = shift_table()) return rc;
    hipLaunchKernelGGL(k_renumber, dim3(uint32_t(g ? g : 1)), dim3(256), 0, s, reinterpret_cast<HotSlot*>(D + o_hot),
                       n_hot, reinterpret_cast<Node*>(D + o_nodes), n_nodes, RM);
    GM_HIP(ctx, hipGetLastError());
  }
  // a shard's new id map, behind the patch on the same stream (it reads the shift's table)
  std::vector<uint32_t> gm_stage;
  PoolBuf gm_dbuf;
  if (gmap)
    if (const int rc = queue_gmap_shift(ctx, *gmap, RM, n_map, gm_stage, gm_dbuf)) {
      (void)hipStreamSynchronize(s);
      return rc;
    }
  GM_HIP(ctx, hipStreamSynchronize(s));  // the staging buffers go back to the pool / the host
  return EMQX_GM_OK;
}

// ---- the new subscriber CSR of emqx_gm_index_update_subs (gm_subs.cpp) ----
// Output element p of the new CSR belongs to filter f (the last segment whose
// start <= p); its source is f's edited list from the host (f in aff_ids) or
// element p - nsoff[f] of the previous list of f's old id inv[f].  Every
// workgroup owns per_block consecutive outputs, as k_fanout_copy does.
__device__ __forceinline__ uint64_t seg_of(const uint64_t* __restrict__ s, uint64_t a, uint64_t b, uint64_t p) {
  // s[a] <= p < s[b]: the last segment of [a, b) starting at or before p
  while (b - a > 1) {
    const uint64_t m = (a + b) >> 1;
    if (s[m] <= p) a = m;
    else b = m;
  }
  return a;
}
__global__ __launch_bounds__(256) void k_subs_copy(const uint64_t* __restrict__ nsoff, uint64_t nf,
                                                   const uint32_t* __restrict__ inv, const uint64_t* __restrict__ osoff,
                                                   const uint32_t* __restrict__ oids, const uint32_t* __restrict__ aff_ids,
                                                   uint64_t n_aff, const uint64_t* __restrict__ aff_off,
                                                   const uint32_t* __restrict__ aff_buf, uint64_t total,
                                                   uint64_t per_block, uint32_t* __restrict__ out) {
  const uint64_t lo = uint64_t(blockIdx.x) * per_block;
  if (lo >= total) return;
  const uint64_t hi = min(total, lo + per_block);
  __shared__ uint64_t s_seg[2];
  if (threadIdx.x < 2) s_seg[threadIdx.x] = seg_of(nsoff, 0, nf, threadIdx.x == 0 ? lo : hi - 1);
  __syncthreads();
  const uint64_t s0 = s_seg[0], s1 = s_seg[1] + 1;
  for (uint64_t p = lo + threadIdx.x; p < hi; p += 256) {
    const uint64_t f = seg_of(nsoff, s0, s1, p);
    const uint64_t q = p - nsoff[f];
    uint64_t a = 0, b = n_aff;  // is f a touched filter?
    while (a < b) {
      const uint64_t m = (a + b) >> 1;
      if (aff_ids[m] < f) a = m + 1;
      else b = m;
    }
    out[p] = (a < n_aff && aff_ids[a] == f) ? aff_buf[aff_off[a] + q] : oids[osoff[inv ? inv[f] : f] + q];
  }
}

// A subscriber-only batch (ids unchanged): new sub_off[i] = old sub_off[i] +
// the count changes of the touched filters below i (tid ascending, tcum their
// running sum) -- the host uploads only the touched ids
__global__ __launch_bounds__(256) void k_soff_shift(const uint64_t* __restrict__ osoff, uint64_t n1,
                                                    const uint32_t* __restrict__ tid, const int64_t* __restrict__ tcum,
                                                    uint64_t nt, uint64_t* __restrict__ nsoff) {
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n1; i += uint64_t(gridDim.x) * 256u) {
    uint64_t a = 0, b = nt;  // touched ids below i
    while (a < b) {
      const uint64_t m = (a + b) >> 1;
      if (tid[m] < i) a = m + 1;
      else b = m;
    }
    nsoff[i] = uint64_t(int64_t(osoff[i]) + (a ? tcum[a - 1] : 0));
  }
}

__global__ __launch_bounds__(256) void k_gather_segments(const uint32_t* __restrict__ src,
                                                         const uint64_t* __restrict__ src_off,
                                                         const uint64_t* __restrict__ dst_off, uint64_t m,
                                                         uint64_t total, uint64_t per_block,
                                                         uint32_t* __restrict__ out) {
  const uint64_t lo = uint64_t(blockIdx.x) * per_block;
  if (lo >= total) return;
  const uint64_t hi = min(total, lo + per_block);
  __shared__ uint64_t s_seg[2];
  if (threadIdx.x < 2) s_seg[threadIdx.x] = seg_of(dst_off, 0, m, threadIdx.x == 0 ? lo : hi - 1);
  __syncthreads();
  const uint64_t s0 = s_seg[0], s1 = s_seg[1] + 1;
  for (uint64_t p = lo + threadIdx.x; p < hi; p += 256) {
    const uint64_t j = seg_of(dst_off, s0, s1, p);
    out[p] = src[src_off[j] + (p - dst_off[j])];
  }
}

int gather_segments(emqx_gm_ctx* ctx, const uint32_t* src, const std::vector<uint64_t>& src_off,
                    const std::vector<uint64_t>& dst_off, uint32_t* out) {
  const uint64_t m = src_off.size(), total = dst_off.back();
  if (!total) return EMQX_GM_OK;
  hipStream_t st = ctx->stream;
  PoolBuf so(ctx->pool, m * 8 + 8), dof(ctx->pool, (m + 1) * 8), buf(ctx->pool, total * 4 + 16);
  if (!so.p || !dof.p || !buf.p) return set_err(ctx, EMQX_GM_ENOMEM, "gather_segments: workspace");
  GM_HIP(ctx, hipMemcpyAsync(so.p, src_off.data(), m * 8, hipMemcpyHostToDevice, st));
  GM_HIP(ctx, hipMemcpyAsync(dof.p, dst_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
  const uint64_t per = fan_per_block(total);
  hipLaunchKernelGGL(k_gather_segments, dim3((total + per - 1) / per), dim3(256), 0, st, src, so.as<uint64_t>(),
                     dof.as<uint64_t>(), m, total, per, buf.as<uint32_t>());
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipMemcpyAsync(out, buf.p, total * 4, hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  return EMQX_GM_OK;
}

// The new subscriber CSR of a subscriber-only emqx_gm_index_update_subs batch
// (gm_subs.cpp; filter ids unchanged): O(delta) host work -- the touched
// filters' ids, count changes and lists go up -- and the device derives the
// offsets (k_soff_shift) and copies every other filter's segment from prev's
// CSR (k_subs_copy with the identity id map).
int shift_subs_device(emqx_gm_ctx* ctx, const emqx_gm_index* prev, emqx_gm_index* idx,
                      const std::vector<uint32_t>& aff_ids, const std::vector<uint64_t>& aff_off,
                      const std::vector<uint32_t>& aff_buf) {
  const uint64_t nf = prev->info.n_filters, na = aff_ids.size();
  std::vector<int64_t> tcum(na + 1, 0);
  int64_t cum = 0;
  for (uint64_t k = 0; k < na; ++k) {
    if (aff_ids[k] >= nf || (k && aff_ids[k] <= aff_ids[k - 1]))
      return set_err(ctx, EMQX_GM_EINVAL, "index_update_subs: touched ids");
    cum += int64_t(aff_off[k + 1] - aff_off[k]) - int64_t(prev->subs.count(aff_ids[k]));
    tcum[k] = cum;
  }
  const uint64_t total = uint64_t(int64_t(prev->subs.total()) + cum);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_ids = al((nf + 1) * 8);
  GM_HIP(ctx, hipMalloc(&idx->dev_subs, o_ids + total * 4 + 16));
  idx->subs_bytes = o_ids + total * 4 + 16;
  uint8_t* D = static_cast<uint8_t*>(idx->dev_subs);
  hipStream_t st = ctx->stream;
  // staging: tid | tcum | aff_off | aff_buf
  const size_t o_cum = al(na * 4 + 4), o_aoff = o_cum + al((na + 1) * 8), o_abuf = o_aoff + al(aff_off.size() * 8),
               n_st = o_abuf + aff_buf.size() * 4 + 4;
  std::vector<uint8_t> h(n_st, 0);
  if (na) std::memcpy(h.data(), aff_ids.data(), na * 4);
  std::memcpy(h.data() + o_cum, tcum.data(), (na + 1) * 8);
  std::memcpy(h.data() + o_aoff, aff_off.data(), aff_off.size() * 8);
  if (!aff_buf.empty()) std::memcpy(h.data() + o_abuf, aff_buf.data(), aff_buf.size() * 4);
  PoolBuf sbuf(ctx->pool, n_st);
  if (!sbuf.p) return set_err(ctx, EMQX_GM_ENOMEM, "index_update_subs: staging");
  GM_HIP(ctx, hipMemcpyAsync(sbuf.p, h.data(), n_st, hipMemcpyHostToDevice, st));
  const uint8_t* S = sbuf.as<uint8_t>();
  const uint64_t g = std::min<uint64_t>(4096, (nf + 1 + 255) / 256);
  hipLaunchKernelGGL(k_soff_shift, dim3(g), dim3(256), 0, st, prev->view.sub_off, nf + 1,
                     reinterpret_cast<const uint32_t*>(S), reinterpret_cast<const int64_t*>(S + o_cum), na,
                     reinterpret_cast<uint64_t*>(D));
  GM_HIP(ctx, hipGetLastError());
  if (total) {
    const uint64_t per = fan_per_block(total);
    hipLaunchKernelGGL(k_subs_copy, dim3((total + per - 1) / per), dim3(256), 0, st,
                       reinterpret_cast<const uint64_t*>(D), nf, static_cast<const uint32_t*>(nullptr),
                       prev->view.sub_off, prev->view.sub_ids, reinterpret_cast<const uint32_t*>(S), na,
                       reinterpret_cast<const uint64_t*>(S + o_aoff), reinterpret_cast<const uint32_t*>(S + o_abuf),
                       total, per, reinterpret_cast<uint32_t*>(D + o_ids));
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipStreamSynchronize(st));  // the staging goes back to the pool / the host
  idx->view.sub_off = reinterpret_cast<const uint64_t*>(D);
  idx->view.sub_ids = reinterpret_cast<const uint32_t*>(D + o_ids);
  idx->info.device_bytes += o_ids + total * 4 + 16;
  return EMQX_GM_OK;
}

int rebuild_subs_device(emqx_gm_ctx* ctx, const emqx_gm_index* prev, emqx_gm_index* idx,
                        const std::vector<uint64_t>& new_soff, const std::vector<uint32_t>& inv,
                        const std::vector<uint32_t>& aff_ids, const std::vector<uint64_t>& aff_off,
                        const std::vector<uint32_t>& aff_buf) {
  const uint64_t nf = new_soff.size() - 1, total = new_soff.back();
  for (uint64_t f = 0; f < nf; ++f)  // host-side check of what the kernel will index
    if (inv[f] == NONE && !std::binary_search(aff_ids.begin(), aff_ids.end(), uint32_t(f)) &&
        new_soff[f + 1] != new_soff[f])
      return set_err(ctx, EMQX_GM_EINVAL, "index_update_subs: a new filter without its list");
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_ids = al((nf + 1) * 8);
  GM_HIP(ctx, hipMalloc(&idx->dev_subs, o_ids + total * 4 + 16));
  idx->subs_bytes = o_ids + total * 4 + 16;
  uint8_t* D = static_cast<uint8_t*>(idx->dev_subs);
  hipStream_t st = ctx->stream;
  GM_HIP(ctx, hipMemcpyAsync(D, new_soff.data(), (nf + 1) * 8, hipMemcpyHostToDevice, st));
  // staging: inv | aff_ids | aff_off | aff_buf
  const size_t o_aid = al(nf * 4 + 4), o_aoff = o_aid + al(aff_ids.size() * 4 + 4),
               o_abuf = o_aoff + al(aff_off.size() * 8), n_st = o_abuf + aff_buf.size() * 4 + 4;
  std::vector<uint8_t> h(n_st, 0);
  std::memcpy(h.data(), inv.data(), nf * 4);
  if (!aff_ids.empty()) std::memcpy(h.data() + o_aid, aff_ids.data(), aff_ids.size() * 4);
  std::memcpy(h.data() + o_aoff, aff_off.data(), aff_off.size() * 8);
  if (!aff_buf.empty()) std::memcpy(h.data() + o_abuf, aff_buf.data(), aff_buf.size() * 4);
  PoolBuf sbuf(ctx->pool, n_st);
  if (!sbuf.p) return set_err(ctx, EMQX_GM_ENOMEM, "index_update_subs: staging");
  GM_HIP(ctx, hipMemcpyAsync(sbuf.p, h.data(), n_st, hipMemcpyHostToDevice, st));
  if (total) {
    const uint8_t* S = sbuf.as<uint8_t>();
    const uint64_t per = fan_per_block(total);
    hipLaunchKernelGGL(k_subs_copy, dim3((total + per - 1) / per), dim3(256), 0, st,
                       reinterpret_cast<const uint64_t*>(D), nf, reinterpret_cast<const uint32_t*>(S),
                       prev->view.sub_off, prev->view.sub_ids, reinterpret_cast<const uint32_t*>(S + o_aid),
                       uint64_t(aff_ids.size()), reinterpret_cast<const uint64_t*>(S + o_aoff),
                       reinterpret_cast<const uint32_t*>(S + o_abuf), total, per,
                       reinterpret_cast<uint32_t*>(D + o_ids));
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipStreamSynchronize(st));  // the staging goes back to the pool / the host
  idx->view.sub_off = reinterpret_cast<const uint64_t*>(D);
  idx->view.sub_ids = reinterpret_cast<const uint32_t*>(D + o_ids);
  idx->info.device_bytes += o_ids + total * 4 + 16;
  return EMQX_GM_OK;
}

}  // namespace gm
