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
// Capacities: the fan-out's rule -- 1024 + the ids past the slack x this
// context's recent hits (pairs) per match, rounded up to a power of two.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "gm_dests.h"
#include "gm_publish.h"
#include "gm_shared.h"

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
  bool q_pick = false, q_plan = false;
  ShSpec ps;
  DtSpec fs;
  void* d_hash = nullptr;
  uint64_t cap_hits = 0, cap_pairs = 0;
  // the page-locked results of the speculative run
  uint64_t* h_pro[2] = {nullptr, nullptr};
  uint64_t *h_noff = nullptr, *h_meta = nullptr;
  uint32_t *h_mem = nullptr, *h_slot = nullptr, *h_rows = nullptr, *h_fil = nullptr, *h_rr = nullptr;
  // what the call returns
  emqx_gm_csr members{}, slots{};
  emqx_gm_forwards fw{};

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
  void drop_device() {  // the workspaces back to the pool behind the work queued so far
    void* ps3[3] = {ps.ws, fs.ws, d_hash};
    for (void* p : ps3)
      if (p) ctx->pool->release_after(p, ctx->stream);
    ps = ShSpec{};
    fs = DtSpec{};
    d_hash = nullptr;
    q_pick = q_plan = false;
  }
  // a failed call: nothing is held
  void drop_all() {
    drop_device();
    drop_pick_host();
    drop_plan_host();
    ctx->hpool->release(h_meta);
    h_meta = nullptr;
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

  void queue(const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap, const uint32_t* hash_pin) {
    hipStream_t s = ctx->stream;
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
    h_meta = nullptr;
    return EMQX_GM_OK;
  }
};

}  // namespace

int run_publish_window(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                       uint32_t flags, const PwArgs& a, emqx_gm_publish_result* res, emqx_gm_publish_stats* st_out,
                       emqx_gm_match_stats* mst, SmallFan* fan) {
  PwStage stage(ctx, a, n);
  // the hashes in a page-locked copy of the call's own (staged outside the lock, like the topics)
  PinBuf hpin(ctx->pins);
  if (a.sh && a.strategy == EMQX_GM_SHARE_HASH && n) {
    if ((hpin.p = ctx->pins->get(al16(n * 4)))) std::memcpy(hpin.p, a.msg_hash, n * 4);
  }
  SmallSide side;
  side.queue = [&](const uint64_t* d_ro, const uint32_t* d_ids, uint64_t cap) {
    stage.queue(d_ro, d_ids, cap, static_cast<const uint32_t*>(hpin.p));
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
    if (stage.q_pick || stage.q_plan) hipStreamSynchronize(ctx->stream);  // (a queued kernel may still write the results)
    stage.drop_all();
    return rc;
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
