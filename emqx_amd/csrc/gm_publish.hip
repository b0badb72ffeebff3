// gm_publish.hip — a whole publish window in one device round trip
// (emqx_gm_publish_window): the shared picks and the forward plan of a window
// queued behind its match's speculative rows and fan-out, before the call's one
// wait (gm_host.cpp run_host_small, SmallSide).
//
// The reference does all of it per message in the publisher's process:
// route(aggre(match_routes(Topic))), forward/3 per node route and
// emqx_shared_sub:dispatch/3 per group (apps/emqx/src/emqx_broker.erl:204-215,
// 245-293, emqx_shared_sub.erl:113-130).
//
// queue()   under the context lock, behind the rows and the fan-out:
//             gm_shared.hip sh_queue_spec   the picks into cap_hits entries
//             gm_dests.hip  dt_queue_spec   the plan into cap_pairs entries
//             k_pw_pack                     ONE launch copies every side result
//                                           and the two true totals into mapped
//                                           page-locked result buffers
//           Neither stage reads a count back: both run over the ids' capacity
//           and read the rows' own count on the device (row_off[n]).  The
//           shared table's state is not written: the picks leave their new
//           round-robin index / first sticky member in shadow arrays.
// finish()  after the wait, under the lock, the true rows still on the device:
//           a part holds if the rows were the speculative ones and its total
//           fits its capacity; a held pick queues k_sh_commit (no wait).  A part
//           that does not hold is run again at its exact size on the device
//           rows (sh_pick_device / dt_plan_device, host_out).
// emqx_gm_publish_window_deliver: the deliveries with their option bytes are a
// THIRD speculative part, in place of the plain fan-out (gm_subopts.hip
// so_queue_spec into cap_deliveries entries, k_so_pack: one more copy-out
// launch).  finish() settles them after the plan and before the picks'
// commit, so the shared state is unchanged on every error of the call; a part
// that does not hold: so_deliver_device (host_out) on the device rows and the
// messages already uploaded.
// Capacities: the fan-out's rule -- 1024 + the ids past the slack x this
// context's recent hits (pairs) per match, rounded up to a power of two.
//
// emqx_gm_publish_windows runs a GROUP of such windows as one batch (the
// reference's many publisher processes at once, emqx_broker.erl:296-322): the
// same two stages ONCE over the group's rows, then a cut into each window's own
// result (PwGroupStage below; the cut's kernels: gm_windows.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gm_dests.h"
#include "gm_publish.h"
#include "gm_shared.h"
#include "gm_subopts.h"

namespace gm {
namespace {

// a speculative part larger than this many entries is not queued (its page-locked result)
constexpr uint64_t kPwMaxCap = uint64_t(16) << 20;

struct PwPack {
  // picks (n_ro = 0: none): row offsets to both result CSRs, members and slots up to min(*p_total, cap_hits)
  const uint64_t* p_ro;
  uint64_t *o_ro0, *o_ro1;
  uint64_t n_ro;
  const uint32_t *p_mem, *p_slot;
  uint32_t *o_mem, *o_slot;
  const uint64_t* p_total;
  uint64_t cap_hits;
  // forwards (n_noff = 0: none): node offsets, rows and filters up to min(*f_total, cap_pairs), row routes
  const uint64_t* f_noff;
  uint64_t* o_noff;
  uint64_t n_noff;
  const uint32_t *f_rows, *f_fil;
  uint32_t *o_rows, *o_fil;
  const uint64_t* f_total;
  uint64_t cap_pairs;
  const uint32_t* f_rr;
  uint32_t* o_rr;
  uint64_t n_rr;
  uint64_t* o_meta;  // [0] the true hits, [1] the true pairs
};

// n u32 words, 16 B at a time (every buffer here is 16-B aligned)
__device__ __forceinline__ void pw_copy(uint32_t* __restrict__ d, const uint32_t* __restrict__ s, uint64_t n, uint64_t t,
                                        uint64_t stride) {
  const uint64_t q = n / 4;
  for (uint64_t i = t; i < q; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
  if (t < (n & 3)) d[q * 4 + t] = s[q * 4 + t];
}

// Every side result of a window to its page-locked result buffer in one launch
// (after k_copy_u32x2 / k_rows_split): plain vector stores, no atomics, no wait
// between workgroups; the copy lengths are the device's own totals, clamped to
// the capacities, and the totals travel with the results.
__global__ __launch_bounds__(256) void k_pw_pack(PwPack a) {
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x, stride = uint64_t(gridDim.x) * 256u;
  uint64_t hits = 0, pairs = 0;
  if (a.n_ro) {
    hits = *a.p_total;
    const uint64_t k = min(hits, a.cap_hits);
    pw_copy(reinterpret_cast<uint32_t*>(a.o_ro0), reinterpret_cast<const uint32_t*>(a.p_ro), a.n_ro * 2, t, stride);
    pw_copy(reinterpret_cast<uint32_t*>(a.o_ro1), reinterpret_cast<const uint32_t*>(a.p_ro), a.n_ro * 2, t, stride);
    pw_copy(a.o_mem, a.p_mem, k, t, stride);
    pw_copy(a.o_slot, a.p_slot, k, t, stride);
  }
  if (a.n_noff) {
    pairs = *a.f_total;
    const uint64_t k = min(pairs, a.cap_pairs);
    pw_copy(reinterpret_cast<uint32_t*>(a.o_noff), reinterpret_cast<const uint32_t*>(a.f_noff), a.n_noff * 2, t, stride);
    pw_copy(a.o_rows, a.f_rows, k, t, stride);
    pw_copy(a.o_fil, a.f_fil, k, t, stride);
    pw_copy(a.o_rr, a.f_rr, a.n_rr, t, stride);
  }
  if (t == 0) {
    a.o_meta[0] = hits;
    a.o_meta[1] = pairs;
  }
  __threadfence_system();  // (host-bound stores visible before the call's end event)
}

template <class T> T* dev_ptr(T* h) {  // a page-locked buffer as the device addresses it (nullptr: not mapped)
  void* d = nullptr;
  return h && hipHostGetDevicePointer(&d, h, 0) == hipSuccess ? static_cast<T*>(d) : nullptr;
}

size_t pow2_bytes(uint64_t entries) {  // (a power of two: the buffer comes back from the host pool's cache)
  size_t b = 4096;
  while (b < entries * 4 + 16) b <<= 1;
  return b;
}

// the speculative capacity of a part: the A/B knob's value as it is, else the rule (0: do not speculate)
uint64_t spec_cap(const char* forced, uint64_t cap_ids, double per_match) {
  if (const char* e = forced) return std::min<uint64_t>(strtoull(e, nullptr, 10), kPwMaxCap);
  const double want = 1024.0 + double(cap_ids > 1024 ? cap_ids - 1024 : 1) * per_match;
  if (want > double(kPwMaxCap)) return 0;
  uint64_t c = 1024;
  while (double(c) < want) c <<= 1;
  return c;
}

struct PwStage {
  emqx_gm_ctx* ctx;
  const PwArgs& a;
  uint64_t n;
  emqx_gm_publish_stats st{};
  bool q_pick = false, q_plan = false, q_del = false, del_spec = false;
  ShSpec ps;
  DtSpec fs;
  SoSpec ds;
  void* d_hash = nullptr;
  uint64_t cap_hits = 0, cap_pairs = 0, cap_del = 0;
  // the page-locked results of the speculative run
  uint64_t* h_pro[2] = {nullptr, nullptr};
  uint64_t *h_noff = nullptr, *h_meta = nullptr;
  uint32_t *h_mem = nullptr, *h_slot = nullptr, *h_rows = nullptr, *h_fil = nullptr, *h_rr = nullptr;
  uint64_t *h_dro = nullptr, *h_dmeta = nullptr;
  uint32_t *h_dids = nullptr, *h_drd = nullptr;
  uint8_t* h_dopt = nullptr;
  // what the call returns
  emqx_gm_csr members{}, slots{};
  emqx_gm_forwards fw{};
  emqx_gm_deliveries deliv{};

  PwStage(emqx_gm_ctx* c, const PwArgs& args, uint64_t n_topics) : ctx(c), a(args), n(n_topics) {}

  bool stateful() const {
    return a.sh && (a.strategy == EMQX_GM_SHARE_ROUND_ROBIN || a.strategy == EMQX_GM_SHARE_STICKY);
  }
  // (all under ctx->mu)
  void drop_pick_host() {
    for (void* p : {static_cast<void*>(h_pro[0]), static_cast<void*>(h_pro[1]), static_cast<void*>(h_mem),
                    static_cast<void*>(h_slot)})
      ctx->hpool->release(p);
    h_pro[0] = h_pro[1] = nullptr;
    h_mem = h_slot = nullptr;
  }
  void drop_plan_host() {
    for (void* p : {static_cast<void*>(h_noff), static_cast<void*>(h_rows), static_cast<void*>(h_fil),
                    static_cast<void*>(h_rr)})
      ctx->hpool->release(p);
    h_noff = nullptr;
    h_rows = h_fil = h_rr = nullptr;
  }
  void drop_del_host() {
    for (void* p : {static_cast<void*>(h_dro), static_cast<void*>(h_dids), static_cast<void*>(h_dopt),
                    static_cast<void*>(h_drd)})
      ctx->hpool->release(p);
    h_dro = nullptr;
    h_dids = h_drd = nullptr;
    h_dopt = nullptr;
  }
  void drop_device() {  // the workspaces back to the pool behind the work queued so far
    void* ps4[4] = {ps.ws, fs.ws, d_hash, ds.ws};
    for (void* p : ps4)
      if (p) ctx->pool->release_after(p, ctx->stream);
    ps = ShSpec{};
    fs = DtSpec{};
    ds = SoSpec{};
    d_hash = nullptr;
    q_pick = q_plan = q_del = false;
  }
  // a failed call: nothing is held
  void drop_all() {
    drop_device();
    drop_pick_host();
    drop_plan_host();
    drop_del_host();
    ctx->hpool->release(h_meta);
    ctx->hpool->release(h_dmeta);
    h_meta = h_dmeta = nullptr;
    for (void* p : {static_cast<void*>(deliv.deliveries.row_off), static_cast<void*>(deliv.deliveries.ids),
                    static_cast<void*>(deliv.dopt), static_cast<void*>(deliv.row_dropped)})
      ctx->hpool->release(p);
    deliv = emqx_gm_deliveries{};
    for (emqx_gm_csr* c : {&members, &slots}) {
      ctx->hpool->release(c->row_off);
      ctx->hpool->release(c->ids);
      *c = emqx_gm_csr{};
    }
    for (void* p : {static_cast<void*>(fw.node_off), static_cast<void*>(fw.rows), static_cast<void*>(fw.filters),
                    static_cast<void*>(fw.row_routes)})
      ctx->hpool->release(p);
    fw = emqx_gm_forwards{};
  }

  // the deliveries with their option bytes: the fan-out's own capacity and rule, one copy-out launch of their own
  void queue_deliv(const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap, const void* msgs_pin) {
    if (!a.so || !n || !(cap_del = spec_cap(so_cap_knob(), cap, ctx->subs_per_match))) return;
    if (so_queue_spec(ctx, a.so, d_ro, d_ids, n, cap, cap_del, a.so_mode, msgs_pin, &ds)) return;
    const bool drop = a.so_mode == EMQX_GM_SO_DROP;
    h_dmeta = static_cast<uint64_t*>(ctx->hpool->alloc(64, true));
    h_dro = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8, true));
    h_dids = static_cast<uint32_t*>(ctx->hpool->alloc(pow2_bytes(cap_del), true));
    h_dopt = static_cast<uint8_t*>(ctx->hpool->alloc(pow2_bytes((cap_del + 3) / 4), true));
    if (drop) h_drd = static_cast<uint32_t*>(ctx->hpool->alloc(std::max<size_t>(n * 4, 16), true));
    uint64_t *o_meta = dev_ptr(h_dmeta), *o_ro = dev_ptr(h_dro);
    uint32_t *o_ids = dev_ptr(h_dids), *o_rd = drop ? dev_ptr(h_drd) : nullptr;
    uint8_t* o_opt = dev_ptr(h_dopt);
    // (no room, or nothing comes back: this part runs after the wait, on the messages already up)
    q_del = o_meta && o_ro && o_ids && o_opt && (!drop || o_rd) &&
            so_queue_pack(ctx, ds, n, cap_del, o_ro, o_ids, o_opt, o_rd, o_meta) == 0;
    if (!q_del) drop_del_host();
  }

  void queue(const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap, const uint32_t* hash_pin,
             const void* msgs_pin) {
    hipStream_t s = ctx->stream;
    queue_deliv(d_ro, d_ids, cap, msgs_pin);
    const uint32_t N = a.dt ? a.dt->hv.n_nodes : 0;
    if (a.sh && (cap_hits = spec_cap(knob("GM_PW_CAP_HITS"), cap, ctx->hits_per_match))) {
      bool ok = true;
      if (a.strategy == EMQX_GM_SHARE_HASH && n) {  // the hashes up, from the call's page-locked copy
        d_hash = ctx->pool->alloc(n * 4);
        const uint32_t* hm = n * 4 <= (size_t(1) << 20) ? dev_ptr(const_cast<uint32_t*>(hash_pin)) : nullptr;
        ok = d_hash && hash_pin &&
             (hm ? launch_copy_u32x2(s, hm, static_cast<uint32_t*>(d_hash), n, nullptr, nullptr, 0) == 0
                 : hipMemcpyAsync(d_hash, hash_pin, n * 4, hipMemcpyHostToDevice, s) == hipSuccess);
      }
      q_pick = ok && sh_queue_spec(ctx, a.sh, d_ro, d_ids, n, cap, cap_hits, a.strategy,
                                   static_cast<const uint32_t*>(d_hash), a.seed, &ps) == 0;
    }
    if (a.dt && (cap_pairs = spec_cap(knob("GM_PW_CAP_PAIRS"), cap, ctx->pairs_per_match)))
      q_plan = dt_queue_spec(ctx, a.dt, d_ro, d_ids, n, cap, cap_pairs, a.skip_node, &fs) == 0;
    if (!q_pick && !q_plan) return;
    // the page-locked results, and the one launch that fills them
    PwPack k{};
    h_meta = static_cast<uint64_t*>(ctx->hpool->alloc(64, true));
    k.o_meta = dev_ptr(h_meta);
    if (q_pick) {
      h_pro[0] = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8, true));
      h_pro[1] = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8, true));
      h_mem = static_cast<uint32_t*>(ctx->hpool->alloc(pow2_bytes(cap_hits), true));
      h_slot = static_cast<uint32_t*>(ctx->hpool->alloc(pow2_bytes(cap_hits), true));
      k.p_ro = ps.row_off;
      k.o_ro0 = dev_ptr(h_pro[0]);
      k.o_ro1 = dev_ptr(h_pro[1]);
      k.n_ro = n + 1;
      k.p_mem = ps.members;
      k.p_slot = ps.slots;
      k.o_mem = dev_ptr(h_mem);
      k.o_slot = dev_ptr(h_slot);
      k.p_total = ps.total;
      k.cap_hits = cap_hits;
      if (!k.o_meta || !k.o_ro0 || !k.o_ro1 || !k.o_mem || !k.o_slot) {  // (no room: this part runs after the wait)
        q_pick = false;
        k.n_ro = 0;
        drop_pick_host();
      }
    }
    if (q_plan) {
      h_noff = static_cast<uint64_t*>(ctx->hpool->alloc((uint64_t(N) + 1) * 8, true));
      h_rows = static_cast<uint32_t*>(ctx->hpool->alloc(pow2_bytes(cap_pairs), true));
      h_fil = static_cast<uint32_t*>(ctx->hpool->alloc(pow2_bytes(cap_pairs), true));
      h_rr = static_cast<uint32_t*>(ctx->hpool->alloc(std::max<size_t>(n * 4, 16), true));
      k.f_noff = fs.node_off;
      k.o_noff = dev_ptr(h_noff);
      k.n_noff = uint64_t(N) + 1;
      k.f_rows = fs.rows;
      k.f_fil = fs.filters;
      k.o_rows = dev_ptr(h_rows);
      k.o_fil = dev_ptr(h_fil);
      k.f_total = fs.total;
      k.cap_pairs = cap_pairs;
      k.f_rr = fs.row_routes;
      k.o_rr = dev_ptr(h_rr);
      k.n_rr = n;
      if (!k.o_meta || !k.o_noff || !k.o_rows || !k.o_fil || !k.o_rr) {
        q_plan = false;
        k.n_noff = 0;
        drop_plan_host();
      }
    }
    if (!q_pick && !q_plan) return;
    const uint64_t words = std::max({(n + 1) * 2, q_pick ? cap_hits : 0, q_plan ? cap_pairs : 0,
                                     q_plan ? (uint64_t(N) + 1) * 2 : 0});
    const uint64_t g = std::min<uint64_t>(1024, ((words + 3) / 4 + 255) / 256);
    hipLaunchKernelGGL(k_pw_pack, dim3(g ? g : 1), dim3(256), 0, s, k);
    if (hipGetLastError() != hipSuccess) {  // (nothing comes back: both parts run after the wait)
      q_pick = q_plan = false;
      drop_pick_host();
      drop_plan_host();
    }
  }

  int finish(bool rows_spec, const emqx_gm_csr* rows) {
    st.rows_spec = rows_spec;
    st.cap_hits = cap_hits;
    st.cap_pairs = cap_pairs;
    const uint64_t hits = h_meta ? h_meta[0] : 0, pairs = h_meta ? h_meta[1] : 0;
    const uint32_t N = a.dt ? a.dt->hv.n_nodes : 0;
    int rc = EMQX_GM_OK;
    // the plan first: the picks' commit is the only step that changes state, and it comes last
    if (a.dt) {
      if (q_plan && rows_spec && pairs <= cap_pairs) {
        fw.n_rows = n;
        fw.n_pairs = pairs;
        fw.node_off = h_noff;
        fw.rows = h_rows;
        fw.filters = h_fil;
        fw.row_routes = h_rr;
        fw.n_nodes = N;
        fw.on_device = 0;
        fw.priv = ctx;
        h_noff = nullptr;
        h_rows = h_fil = h_rr = nullptr;
        st.forwards_spec = 1;
      } else {
        drop_plan_host();
        rc = dt_plan_device(ctx, a.dt, rows, a.skip_node, 0, &fw, true, &st.device_waits);
        if (rc) return rc;
      }
      st.n_pairs = fw.n_pairs;
      if (rows_spec && rows->nnz) ctx->pairs_per_match = std::max(1.0 / 64, double(fw.n_pairs) / double(rows->nnz));
    }
    // the deliveries: settled before the picks' commit
    if (a.so) {
      const uint64_t tot = h_dmeta ? h_dmeta[0] : 0, dropped = h_dmeta ? h_dmeta[1] : 0;
      if (q_del && rows_spec && tot <= cap_del) {
        deliv.deliveries.n_rows = n;
        deliv.deliveries.nnz = tot;
        deliv.deliveries.row_off = h_dro;
        deliv.deliveries.ids = h_dids;
        deliv.deliveries.on_device = 0;
        deliv.deliveries.priv = ctx;
        deliv.dopt = h_dopt;
        deliv.row_dropped = h_drd;  // (nullptr in FLAG mode)
        deliv.n_dropped = dropped;
        h_dro = nullptr;
        h_dids = h_drd = nullptr;
        h_dopt = nullptr;
        del_spec = true;
      } else {
        drop_del_host();
        rc = so_deliver_device(ctx, a.so, rows, a.msg_flags, a.msg_from, a.so_mode, &deliv, true, &st.device_waits,
                               ds.d_flags, ds.d_from);
        if (rc) return rc;
      }
      // (the plain fan-out's figure, whichever kind of window ran last)
      if (rows_spec && rows->nnz)
        ctx->subs_per_match = std::max(1.0, double(deliv.deliveries.nnz + deliv.n_dropped) / double(rows->nnz));
    }
    if (a.sh) {
      if (q_pick && rows_spec && hits <= cap_hits) {
        emqx_gm_csr* outs[2] = {&members, &slots};
        uint32_t* ids[2] = {h_mem, h_slot};
        for (int k = 0; k < 2; ++k) {
          outs[k]->n_rows = n;
          outs[k]->nnz = hits;
          outs[k]->row_off = h_pro[k];
          outs[k]->ids = ids[k];
          outs[k]->on_device = 0;
          outs[k]->priv = ctx;
          if (!hits) {  // (as emqx_gm_shared_pick: no ids without a hit)
            ctx->hpool->release(ids[k]);
            outs[k]->ids = nullptr;
          }
        }
        h_pro[0] = h_pro[1] = nullptr;
        h_mem = h_slot = nullptr;
        if (hits && (rc = sh_queue_commit(ctx, a.sh, ps))) return rc;  // (queued under sh->mu: no wait of its own)
        st.picks_spec = 1;
      } else {
        drop_pick_host();
        rc = sh_pick_device(ctx, a.sh, rows, a.strategy, a.msg_hash, a.seed, 0, &members, &slots, true,
                            &st.device_waits);
        if (rc) return rc;
      }
      st.n_hits = members.nnz;
      if (rows_spec && rows->nnz) ctx->hits_per_match = std::max(1.0 / 64, double(members.nnz) / double(rows->nnz));
    }
    drop_device();
    ctx->hpool->release(h_meta);
    ctx->hpool->release(h_dmeta);
    h_meta = h_dmeta = nullptr;
    return EMQX_GM_OK;
  }
};

// ---- the group stage (emqx_gm_publish_windows): PwStage for a group of windows
// run as one batch (gm_host.cpp run_host_windows, WindowsSide).
// stage()    outside the lock: the windows' hashes, concatenated in window
//            order, and their first rows into the side's room behind the
//            group's staged text (up with the group's one input copy).
// prepare()  under the lock: each window's own capacities (spec_cap's rule on
//            the window's rows capacity), its page-locked results, and the two
//            window tables (picks: WinSlice x 2, plan: PlanSlice).
// queue()    sh_queue_spec / dt_queue_spec ONCE over the group's rows and
//            capacity (random: with the first-row table), then the cut:
//            k_rows_split over the two pick CSRs (one shared row_off), and
//            k_plan_bounds + k_plan_cut (gm_windows.hip).
// finish()   the plan first, then the picks, the commit last.  A part the group
//            held: a window past its own capacity gets a result of exact size
//            (the plan's cut relaunched for it, the picks copied from the
//            group's arrays), one more wait for all of them.  A part it did
//            not hold: the exact call over the group's true device rows, its
//            host result cut per window on the host by the same rule.
struct PwGroupStage {
  emqx_gm_ctx* ctx;
  const PwArgs& a;
  const emqx_gm_publish_win* w;
  uint32_t g;
  uint64_t n = 0;
  uint32_t N = 0;
  bool hash = false;
  std::vector<uint32_t> row0;  // [g + 1]
  size_t o_row0 = 0, o_ptab = 0, o_ftab = 0, extra = 0;  // (the hashes at 0)
  uint8_t* h_x = nullptr;
  const uint8_t* d_x = nullptr;
  struct Win {
    uint64_t n = 0;
    uint64_t* p_off[2] = {nullptr, nullptr};
    uint32_t* p_ids[2] = {nullptr, nullptr};
    size_t p_ib = 0;  // bytes of each p_ids[]
    uint64_t cap_hits = 0, hits = 0;
    bool p_exact = false;
    uint64_t* f_noff = nullptr;
    uint32_t *f_rows = nullptr, *f_fil = nullptr, *f_rr = nullptr;
    size_t f_ib = 0;  // bytes of f_rows / f_fil
    uint64_t cap_pairs = 0, pairs = 0;
    bool f_exact = false;
  };
  std::vector<Win> win;
  bool tabs_pick = false, tabs_plan = false, q_pick = false, q_plan = false;
  bool held_pick = false, held_plan = false, rows_spec = false;
  ShSpec ps;
  DtSpec fs;
  uint32_t* d_lb = nullptr;
  uint64_t* h_meta = nullptr;
  uint64_t cap_hits = 0, cap_pairs = 0, hits_g = 0, pairs_g = 0, work_p = 0, work_f = 0;
  uint32_t waits = 0;

  PwGroupStage(emqx_gm_ctx* c, const PwArgs& args, const emqx_gm_publish_win* wins, uint32_t n_win)
      : ctx(c), a(args), w(wins), g(n_win), row0(size_t(n_win) + 1, 0), win(n_win) {
    for (uint32_t k = 0; k < g; ++k) {
      win[k].n = w[k].w.n_topics;
      row0[k] = uint32_t(n);
      n += win[k].n;
    }
    row0[g] = uint32_t(n);
    N = a.dt ? a.dt->hv.n_nodes : 0;
    hash = a.sh && a.strategy == EMQX_GM_SHARE_HASH;
    o_row0 = hash ? al16(n * 4) : 0;
    o_ptab = al16(o_row0 + (size_t(g) + 1) * 4);
    o_ftab = al16(o_ptab + size_t(g) * 2 * sizeof(WinSlice));
    extra = al16(o_ftab + size_t(g) * sizeof(PlanSlice));
  }

  bool stateful() const {
    return a.sh && (a.strategy == EMQX_GM_SHARE_ROUND_ROBIN || a.strategy == EMQX_GM_SHARE_STICKY);
  }
  const uint32_t* d_row0() const { return reinterpret_cast<const uint32_t*>(d_x + o_row0); }

  void stage(uint8_t* host) {
    if (hash)
      for (uint32_t k = 0; k < g; ++k)
        if (win[k].n) std::memcpy(host + size_t(row0[k]) * 4, w[k].msg_hash, win[k].n * 4);
    std::memcpy(host + o_row0, row0.data(), (size_t(g) + 1) * 4);
  }

  // (all below under ctx->mu)
  void drop_pick(Win& x) {
    for (int c = 0; c < 2; ++c) {
      ctx->hpool->release(x.p_off[c]);
      ctx->hpool->release(x.p_ids[c]);
      x.p_off[c] = nullptr;
      x.p_ids[c] = nullptr;
    }
    x.p_ib = 0;
  }
  void drop_plan(Win& x) {
    for (void* p : {static_cast<void*>(x.f_noff), static_cast<void*>(x.f_rows), static_cast<void*>(x.f_fil),
                    static_cast<void*>(x.f_rr)})
      ctx->hpool->release(p);
    x.f_noff = nullptr;
    x.f_rows = x.f_fil = x.f_rr = nullptr;
    x.f_ib = 0;
  }
  void drop_device() {  // the workspaces back to the pool behind the work queued so far
    void* ps3[3] = {ps.ws, fs.ws, d_lb};
    for (void* p : ps3)
      if (p) ctx->pool->release_after(p, ctx->stream);
    ps = ShSpec{};
    fs = DtSpec{};
    d_lb = nullptr;
    ctx->hpool->release(h_meta);
    h_meta = nullptr;
  }
  void drop_all() {  // a failed group: nothing is held
    drop_device();
    for (Win& x : win) {
      drop_pick(x);
      drop_plan(x);
    }
  }

  void prepare(uint8_t* host, const uint8_t* dev) {
    h_x = host;
    d_x = dev;
    WinSlice* ptab = reinterpret_cast<WinSlice*>(host + o_ptab);
    PlanSlice* ftab = reinterpret_cast<PlanSlice*>(host + o_ftab);
    std::memset(host + o_ptab, 0, extra - o_ptab);
    const double ipt = std::min(ctx->ids_per_topic, double(FAST_MC));
    tabs_pick = a.sh != nullptr;
    tabs_plan = a.dt != nullptr && N != 0;
    for (uint32_t k = 0; k < g; ++k) {
      Win& x = win[k];
      const uint64_t cap_rows = 1024 + uint64_t(double(x.n) * ipt);  // (run_host_windows' rule for the window's ids)
      if (tabs_pick) {
        x.cap_hits = spec_cap(nullptr, cap_rows, ctx->hits_per_match);
        x.p_ib = pow2_bytes(x.cap_hits);
        for (int c = 0; c < 2 && x.cap_hits; ++c) {
          x.p_off[c] = static_cast<uint64_t*>(ctx->hpool->alloc((x.n + 1) * 8, true));
          x.p_ids[c] = static_cast<uint32_t*>(ctx->hpool->alloc(x.p_ib, true));
          ptab[k * 2 + c] = WinSlice{row0[k], x.n, x.cap_hits, dev_ptr(x.p_off[c]), dev_ptr(x.p_ids[c])};
          if (!ptab[k * 2 + c].dst_row_off || !ptab[k * 2 + c].dst_ids) tabs_pick = false;
        }
        if (!x.cap_hits) tabs_pick = false;
        work_p = std::max({work_p, x.n + 1, (x.cap_hits + 3) / 4});
      }
      if (tabs_plan) {
        x.cap_pairs = spec_cap(nullptr, cap_rows, ctx->pairs_per_match);
        x.f_ib = pow2_bytes(x.cap_pairs);
        if (x.cap_pairs) {
          x.f_noff = static_cast<uint64_t*>(ctx->hpool->alloc((uint64_t(N) + 1) * 8, true));
          x.f_rows = static_cast<uint32_t*>(ctx->hpool->alloc(x.f_ib, true));
          x.f_fil = static_cast<uint32_t*>(ctx->hpool->alloc(x.f_ib, true));
          x.f_rr = static_cast<uint32_t*>(ctx->hpool->alloc(std::max<size_t>(x.n * 4, 16), true));
          ftab[k] = PlanSlice{row0[k],          x.n,
                              x.cap_pairs,      dev_ptr(x.f_noff),
                              dev_ptr(x.f_rows), dev_ptr(x.f_fil),
                              dev_ptr(x.f_rr)};
          if (!ftab[k].dst_node_off || !ftab[k].dst_rows || !ftab[k].dst_filters || !ftab[k].dst_row_routes)
            tabs_plan = false;
        } else {
          tabs_plan = false;
        }
        work_f = std::max({work_f, (x.cap_pairs + 3) / 4, (x.n + 3) / 4});
      }
    }
    // (no room for a part's results: nothing of it is queued, it runs after the wait)
    if (!tabs_pick)
      for (Win& x : win) drop_pick(x);
    if (!tabs_plan)
      for (Win& x : win) drop_plan(x);
  }

  void queue(const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap) {
    hipStream_t s = ctx->stream;
    if (tabs_pick && (cap_hits = spec_cap(knob("GM_PW_CAP_HITS"), cap, ctx->hits_per_match))) {
      const uint32_t* d_hash = hash ? reinterpret_cast<const uint32_t*>(d_x) : nullptr;
      q_pick = sh_queue_spec(ctx, a.sh, d_ro, d_ids, n, cap, cap_hits, a.strategy, d_hash, a.seed, &ps, d_row0(), g) == 0;
      // the two pick CSRs share one row_off: k_rows_split's two planes, members and slots
      if (q_pick && launch_rows_split(s, reinterpret_cast<const WinSlice*>(d_x + o_ptab), g, work_p, ps.row_off,
                                      ps.members, cap_hits, ps.row_off, ps.slots, cap_hits))
        q_pick = false;
    }
    if (tabs_plan && (cap_pairs = spec_cap(knob("GM_PW_CAP_PAIRS"), cap, ctx->pairs_per_match))) {
      q_plan = dt_queue_spec(ctx, a.dt, d_ro, d_ids, n, cap, cap_pairs, a.skip_node, &fs) == 0;
      if (q_plan) {
        d_lb = static_cast<uint32_t*>(ctx->pool->alloc((size_t(g) + 1) * N * 4));
        h_meta = static_cast<uint64_t*>(ctx->hpool->alloc(64, true));
        uint64_t* meta = dev_ptr(h_meta);
        if (!d_lb || !meta ||
            launch_plan_cut(s, reinterpret_cast<const PlanSlice*>(d_x + o_ftab), g, work_f, d_row0(), d_lb, true,
                            fs.node_off, fs.rows, fs.filters, fs.row_routes, N, cap_pairs, fs.total, meta))
          q_plan = false;
      }
    }
  }

  // a window's pick ids again with room for `hits` (not mapped: filled by a copy or on the host)
  bool pick_room(Win& x, uint64_t hits) {
    for (int c = 0; c < 2; ++c)
      if (!x.p_off[c] && !(x.p_off[c] = static_cast<uint64_t*>(ctx->hpool->alloc((x.n + 1) * 8)))) return false;
    if (x.p_ids[0] && hits * 4 + 4 <= x.p_ib) return true;
    for (int c = 0; c < 2; ++c) {
      ctx->hpool->release(x.p_ids[c]);
      x.p_ids[c] = static_cast<uint32_t*>(ctx->hpool->alloc(hits * 4 + 16));
    }
    x.p_ib = hits * 4 + 16;
    return x.p_ids[0] && x.p_ids[1];
  }
  bool plan_room(Win& x, uint64_t pairs, bool mapped) {
    if (!x.f_noff && !(x.f_noff = static_cast<uint64_t*>(ctx->hpool->alloc((uint64_t(N) + 1) * 8)))) return false;
    if (!x.f_rr && !(x.f_rr = static_cast<uint32_t*>(ctx->hpool->alloc(std::max<size_t>(x.n * 4, 16))))) return false;
    if (x.f_rows && pairs * 4 + 4 <= x.f_ib) return true;
    ctx->hpool->release(x.f_rows);
    ctx->hpool->release(x.f_fil);
    x.f_ib = mapped ? pow2_bytes(pairs) : pairs * 4 + 16;
    x.f_rows = static_cast<uint32_t*>(ctx->hpool->alloc(x.f_ib, mapped));
    x.f_fil = static_cast<uint32_t*>(ctx->hpool->alloc(x.f_ib, mapped));
    return x.f_rows && x.f_fil;
  }

  int finish_plan(const emqx_gm_csr* rows) {
    pairs_g = h_meta ? h_meta[0] : 0;
    held_plan = q_plan && rows_spec && pairs_g <= cap_pairs;
    if (held_plan) {
      bool again = false;
      for (uint32_t k = 0; k < g; ++k) {
        Win& x = win[k];
        x.pairs = x.f_noff[N];
        if (x.pairs <= x.cap_pairs) continue;
        // this window alone past its own capacity: a result of exact size, its cut relaunched into it
        x.f_exact = true;
        if (!plan_room(x, x.pairs, true)) return set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
        PlanSlice* ft = reinterpret_cast<PlanSlice*>(h_x + o_ftab) + k;
        ft->pairs_cap = x.pairs;
        ft->dst_rows = dev_ptr(x.f_rows);
        ft->dst_filters = dev_ptr(x.f_fil);
        const PlanSlice* d_ft = reinterpret_cast<const PlanSlice*>(d_x + o_ftab) + k;
        if (!ft->dst_rows || !ft->dst_filters ||
            hipMemcpyAsync(const_cast<PlanSlice*>(d_ft), ft, sizeof(PlanSlice), hipMemcpyHostToDevice, ctx->stream) !=
                hipSuccess ||
            launch_plan_cut(ctx->stream, d_ft, 1, (x.pairs + 3) / 4, d_row0(), d_lb + size_t(k) * N, false, fs.node_off,
                            fs.rows, fs.filters, fs.row_routes, N, cap_pairs, fs.total, dev_ptr(h_meta)))
          return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: a window's plan again");
        again = true;
      }
      if (again) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess)
          return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: a window's plan again");
        ++waits;
      }
      return EMQX_GM_OK;
    }
    // the group's plan at its exact size on the true device rows, cut on the host by the same rule
    if (q_plan && hipStreamSynchronize(ctx->stream) != hipSuccess)  // (nothing queued still writes the windows' results)
      return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: device");
    emqx_gm_forwards gf{};
    if (const int rc = dt_plan_device(ctx, a.dt, rows, a.skip_node, 0, &gf, true, &waits)) return rc;
    pairs_g = gf.n_pairs;
    int rc = EMQX_GM_OK;
    std::vector<uint64_t> lb((size_t(g) + 1) * N);
    for (uint32_t k = 0; k < N; ++k) {
      const uint32_t* lo = gf.rows + gf.node_off[k];
      const uint32_t* hi = gf.rows + gf.node_off[k + 1];
      for (uint32_t b = 0; b <= g; ++b) lb[size_t(b) * N + k] = uint64_t(std::lower_bound(lo, hi, row0[b]) - lo);
    }
    for (uint32_t wk = 0; wk < g && rc == EMQX_GM_OK; ++wk) {
      Win& x = win[wk];
      const uint64_t *l0 = lb.data() + size_t(wk) * N, *l1 = l0 + N;
      x.pairs = 0;
      for (uint32_t k = 0; k < N; ++k) x.pairs += l1[k] - l0[k];
      if (!plan_room(x, x.pairs, false)) {
        rc = set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
        break;
      }
      uint64_t at = 0;
      for (uint32_t k = 0; k < N; ++k) {
        x.f_noff[k] = at;
        const uint64_t src = gf.node_off[k] + l0[k], cnt = l1[k] - l0[k];
        for (uint64_t i = 0; i < cnt; ++i) x.f_rows[at + i] = gf.rows[src + i] - row0[wk];
        if (cnt) std::memcpy(x.f_fil + at, gf.filters + src, cnt * 4);
        at += cnt;
      }
      x.f_noff[N] = at;
      if (x.n) std::memcpy(x.f_rr, gf.row_routes + row0[wk], x.n * 4);
    }
    for (void* p : {static_cast<void*>(gf.node_off), static_cast<void*>(gf.rows), static_cast<void*>(gf.filters),
                    static_cast<void*>(gf.row_routes)})
      ctx->hpool->release(p);
    return rc;
  }

  int finish_picks(const emqx_gm_csr* rows) {
    hits_g = 0;
    if (q_pick && rows_spec)
      for (Win& x : win) hits_g += (x.hits = x.p_off[0][x.n]);
    held_pick = q_pick && rows_spec && hits_g <= cap_hits;
    if (held_pick) {
      bool again = false;
      uint64_t base = 0;
      for (Win& x : win) {
        if (x.hits > x.cap_hits) {  // this window alone past its own capacity: its ids from the group's arrays
          x.p_exact = true;
          if (!pick_room(x, x.hits)) return set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
          if (hipMemcpyAsync(x.p_ids[0], ps.members + base, x.hits * 4, hipMemcpyDeviceToHost, ctx->stream) !=
                  hipSuccess ||
              hipMemcpyAsync(x.p_ids[1], ps.slots + base, x.hits * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: a window's picks again");
          again = true;
        }
        base += x.hits;
      }
      if (again) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess)
          return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: a window's picks again");
        ++waits;
      }
      // (queued under sh->mu: no wait of its own; ONE commit for the group)
      return hits_g ? sh_queue_commit(ctx, a.sh, ps) : EMQX_GM_OK;
    }
    // the group's picks at their exact size on the true device rows (the call writes the table's state itself)
    if (q_pick && hipStreamSynchronize(ctx->stream) != hipSuccess)
      return set_err(ctx, EMQX_GM_EDEVICE, "publish_windows: device");
    emqx_gm_csr gm{}, gsl{};
    if (const int rc = sh_pick_device(ctx, a.sh, rows, a.strategy, hash ? reinterpret_cast<const uint32_t*>(h_x) : nullptr,
                                      a.seed, 0, &gm, &gsl, true, &waits, d_row0(), g))
      return rc;
    hits_g = gm.nnz;
    int rc = EMQX_GM_OK;
    for (uint32_t k = 0; k < g; ++k) {
      Win& x = win[k];
      const uint64_t* ro = gm.row_off + row0[k];
      x.hits = ro[x.n] - ro[0];
      if (!pick_room(x, x.hits)) {
        rc = set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
        break;
      }
      for (int c = 0; c < 2; ++c) {
        for (uint64_t i = 0; i <= x.n; ++i) x.p_off[c][i] = ro[i] - ro[0];
        if (x.hits) std::memcpy(x.p_ids[c], (c ? gsl.ids : gm.ids) + ro[0], x.hits * 4);
      }
    }
    for (emqx_gm_csr* c : {&gm, &gsl}) {
      ctx->hpool->release(c->row_off);
      ctx->hpool->release(c->ids);
    }
    return rc;
  }

  int finish(bool spec, const emqx_gm_csr* rows) {
    rows_spec = spec;
    // the plan first: the picks' commit is the only step that changes state, and it comes last
    if (a.dt) {
      if (const int rc = finish_plan(rows)) return rc;
      if (rows_spec && rows->nnz) ctx->pairs_per_match = std::max(1.0 / 64, double(pairs_g) / double(rows->nnz));
    }
    if (a.sh) {
      if (const int rc = finish_picks(rows)) return rc;
      if (rows_spec && rows->nnz) ctx->hits_per_match = std::max(1.0 / 64, double(hits_g) / double(rows->nnz));
    }
    drop_device();
    return EMQX_GM_OK;
  }

  // a group without a topic: every window's empty side results, no device work
  int empty() {
    for (Win& x : win) {
      if (a.sh) {
        if (!pick_room(x, 0)) return set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
        x.p_off[0][0] = x.p_off[1][0] = 0;
      }
      if (a.dt) {
        if (!plan_room(x, 0, false)) return set_err(ctx, EMQX_GM_ENOMEM, "publish_windows: host result");
        std::fill(x.f_noff, x.f_noff + N + 1, uint64_t(0));
      }
    }
    return EMQX_GM_OK;
  }
};

}  // namespace

int run_publish_windows(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win* w, uint32_t g,
                        uint32_t flags, const PwArgs& a, emqx_gm_publish_result* res, emqx_gm_publish_stats* st_out,
                        emqx_gm_publish_group_stats* gst, uint8_t* fan_ok, emqx_gm_match_stats* mst) {
  std::vector<emqx_gm_window> mw(g);
  for (uint32_t k = 0; k < g; ++k) mw[k] = w[k].w;
  std::vector<emqx_gm_csr> m(g), d(g);
  PwGroupStage stage(ctx, a, w, g);
  const bool sides = a.sh || a.dt;
  WindowsSide side;
  side.extra_bytes = stage.extra;
  side.stage = [&](uint8_t* host) { stage.stage(host); };
  side.prepare = [&](uint8_t* host, const uint8_t* dev) { stage.prepare(host, dev); };
  side.queue = [&](const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap) { stage.queue(d_ro, d_ids, cap); };
  side.finish = [&](bool rows_spec, const emqx_gm_csr* rows) { return stage.finish(rows_spec, rows); };
  // the table's own serialisation, ONCE for the group, from the moment the stage
  // is queued until the commit is queued (as run_publish_window's for a window)
  std::unique_lock<std::mutex> tl;
  if (stage.stateful()) tl = std::unique_lock<std::mutex>(a.sh->mu);
  int rc = run_host_windows(ctx, idx, mw.data(), g, flags, m.data(), d.data(), fan_ok, mst, sides ? &side : nullptr);
  if (rc == EMQX_GM_OK && sides && stage.n == 0) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    rc = stage.empty();
  }
  if (rc) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (stage.q_pick || stage.q_plan) hipStreamSynchronize(ctx->stream);  // (a queued kernel may still write the results)
    stage.drop_all();
    for (uint32_t k = 0; k < g; ++k) {
      ctx->hpool->release(m[k].row_off);
      ctx->hpool->release(m[k].ids);
      ctx->hpool->release(d[k].row_off);
      ctx->hpool->release(d[k].ids);
    }
    return rc;
  }
  tl = std::unique_lock<std::mutex>();
  // the group's round trip; rows past their capacity: their copy
  const uint32_t waits = stage.n ? stage.waits + 1 + (stage.rows_spec ? 0 : 1) : 0;
  for (uint32_t k = 0; k < g; ++k) {
    const PwGroupStage::Win& x = stage.win[k];
    res[k] = emqx_gm_publish_result{};
    res[k].matches = m[k];
    if (fan_ok[k]) res[k].deliveries = d[k];
    emqx_gm_publish_stats s{};
    emqx_gm_publish_group_stats q{};
    s.device_waits = q.device_waits = waits;
    s.rows_spec = q.rows_spec = stage.rows_spec;
    s.fanout_spec = fan_ok[k];
    q.position = k;
    q.n_windows = g;
    q.grouped = 1;
    if (a.sh) {
      emqx_gm_csr* outs[2] = {&res[k].pick_members, &res[k].pick_slots};
      for (int c = 0; c < 2; ++c) {
        outs[c]->n_rows = x.n;
        outs[c]->nnz = x.hits;
        outs[c]->row_off = x.p_off[c];
        outs[c]->ids = x.p_ids[c];
        outs[c]->on_device = 0;
        outs[c]->priv = ctx;
      }
      q.picks_spec = stage.held_pick;
      q.window_picks_exact = x.p_exact;
      s.picks_spec = stage.held_pick && !x.p_exact;
      s.n_hits = x.hits;
      s.cap_hits = x.cap_hits;
      q.cap_hits = stage.cap_hits;
      q.n_hits = stage.hits_g;
    }
    if (a.dt) {
      emqx_gm_forwards& fw = res[k].forwards;
      fw.n_rows = x.n;
      fw.n_pairs = x.pairs;
      fw.node_off = x.f_noff;
      fw.rows = x.f_rows;
      fw.filters = x.f_fil;
      fw.row_routes = x.f_rr;
      fw.n_nodes = stage.N;
      fw.on_device = 0;
      fw.priv = ctx;
      q.forwards_spec = stage.held_plan;
      q.window_forwards_exact = x.f_exact;
      s.forwards_spec = stage.held_plan && !x.f_exact;
      s.n_pairs = x.pairs;
      s.cap_pairs = x.cap_pairs;
      q.cap_pairs = stage.cap_pairs;
      q.n_pairs = stage.pairs_g;
    }
    st_out[k] = s;
    gst[k] = q;
  }
  return EMQX_GM_OK;
}

int run_publish_window(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                       uint32_t flags, const PwArgs& a, emqx_gm_publish_result* res, emqx_gm_publish_stats* st_out,
                       emqx_gm_match_stats* mst, SmallFan* fan, PwDeliv* dl) {
  PwStage stage(ctx, a, n);
  // the messages' flags and publishers likewise: [publishers | flags], up in one launch
  PinBuf mpin(ctx->pins);
  if (a.so && n) {
    fan = nullptr;  // (the deliveries run in place of the plain fan-out)
    if ((mpin.p = ctx->pins->get(so_msgs_bytes(n)))) {
      uint8_t* mp = static_cast<uint8_t*>(mpin.p);
      std::memset(mp, 0, so_msgs_bytes(n));
      std::memcpy(mp, a.msg_from, n * 4);
      std::memcpy(mp + al16(n * 4), a.msg_flags, n);
    }
  } else if (a.so) {
    fan = nullptr;
  }
  // the hashes in a page-locked copy of the call's own (staged outside the lock, like the topics)
  PinBuf hpin(ctx->pins);
  if (a.sh && a.strategy == EMQX_GM_SHARE_HASH && n) {
    if ((hpin.p = ctx->pins->get(al16(n * 4)))) std::memcpy(hpin.p, a.msg_hash, n * 4);
  }
  SmallSide side;
  side.queue = [&](const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap) {
    stage.queue(d_ro, d_ids, cap, static_cast<const uint32_t*>(hpin.p), mpin.p);
  };
  side.finish = [&](bool rows_spec, const emqx_gm_csr* rows) { return stage.finish(rows_spec, rows); };
  // the table's own serialisation from the moment the stage is queued until the
  // commit is queued: a second window on the table cannot read its state
  // between the two (taken before the context's lock, as a pick does).  A
  // stateless strategy reads and writes no state, so its windows overlap.
  std::unique_lock<std::mutex> tl;
  if (stage.stateful()) tl = std::unique_lock<std::mutex>(a.sh->mu);
  emqx_gm_csr m{};
  const int rc = run_host_small(ctx, idx, tb, to, n, flags, &m, mst, fan, &side);
  if (rc) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (stage.q_pick || stage.q_plan || stage.q_del || stage.ds.ws)
      hipStreamSynchronize(ctx->stream);  // (a queued kernel may still write the results)
    stage.drop_all();
    return rc;
  }
  if (dl) {
    dl->out = stage.deliv;
    dl->spec = stage.del_spec;
    dl->cap = stage.cap_del;
  }
  res->matches = m;
  res->pick_members = stage.members;
  res->pick_slots = stage.slots;
  res->forwards = stage.fw;
  stage.st.device_waits += 1 + (stage.st.rows_spec ? 0 : 1);  // the call's round trip; rows past their capacity: their copy
  *st_out = stage.st;
  return EMQX_GM_OK;
}

}  // namespace gm
