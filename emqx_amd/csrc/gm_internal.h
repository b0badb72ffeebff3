// gm_internal.h — context, index snapshot and device memory pool.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstdint>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <functional>
#include <vector>

#include "../../include/emqx_gpu_match.h"
#include "../../include/emqx_gm_ext.h"
#include "gm_common.h"
#include "gm_dict.h"
#include "gm_filters.h"

namespace gm {

// An allocator that default-initialises: a vector of PODs is left unwritten
// by resize() until its owner fills it (GBs of index tables filled by all
// threads, or by a copy, instead of first zeroed by one).
template <class T> struct DefaultInit : std::allocator<T> {
  template <class U> struct rebind {
    using other = DefaultInit<U>;
  };
  DefaultInit() = default;
  template <class U> DefaultInit(const DefaultInit<U>&) {}
  template <class U> void construct(U* p) { ::new (static_cast<void*>(p)) U; }
  template <class U, class... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};
using HostBytes = std::vector<uint8_t, DefaultInit<uint8_t>>;

// Caching device allocator: buffers are returned to a size-keyed free list and
// reused, so steady-state batches do no hipMalloc/hipFree.
class DevPool {
 public:
  explicit DevPool(int device) : device_(device) {}
  ~DevPool();
  void* alloc(size_t bytes);           // nullptr on failure
  void release(void* p);
  // Release once the work queued on `s` so far is done (a result CSR the
  // caller frees while later calls may still be queued behind its readers):
  // an event marks the point, alloc() reclaims the buffer once it has passed,
  // and nothing waits.
  void release_after(void* p, hipStream_t s);
  void release_after(void* const* ps, int np, hipStream_t s);  // one event for up to 4 buffers
  void trim();
  size_t cached_bytes() const { return cached_; }

 private:
  int device_;
  std::multimap<size_t, void*> free_;  // rounded size -> ptr
  std::map<void*, size_t> live_;       // ptr -> rounded size
  std::vector<std::pair<void*, hipEvent_t>> deferred_;
  std::vector<hipEvent_t> ev_idle_;
  size_t cached_ = 0;
  void reclaim(bool wait);
};

// Host result buffers (the CSRs emqx_gm_match / emqx_gm_fanout return in host
// memory): emqx_gm_csr_free hands them back and the next call reuses them, so a
// steady stream of calls does no first-touch page faults on fresh pages (2 GB
// per 100M-topic call).  Large buffers are 2 MiB aligned and advised as huge
// pages.  At most kCap bytes stay cached.
// pinned: page-locked (hipHostMalloc, portable to every device) buffers that
// the device writes by DMA -- the multi-chunk host-buffer match copies its rows
// straight into them (gm_host.cpp) instead of through a bounce buffer.
class HostPool {
 public:
  ~HostPool();
  void* alloc(size_t bytes, bool pinned = false);  // nullptr on failure
  void release(void* p);      // a buffer of this pool (any other pointer: free())
  size_t cached_bytes() const { return cached_; }

 private:
  static constexpr size_t kCap = 8ull << 30;
  struct Buf {
    size_t bytes;
    bool pinned;
  };
  std::multimap<size_t, void*> free_[2];  // [pinned] rounded size -> ptr
  std::map<void*, Buf> live_;
  size_t cached_ = 0;
  void drop(void* p, bool pinned);
};

// Page-locked staging buffers of the small host-buffer calls (gm_host.cpp
// run_host_small): each call in flight owns its own, so concurrent calls on
// one context overlap; a thread-safe size-keyed free list (at most kCap cached).
class PinPool {
 public:
  ~PinPool();
  void* get(size_t bytes);  // nullptr on failure
  void put(void* p);
 private:
  static constexpr size_t kCap = 512ull << 20;
  std::mutex mu_;
  std::multimap<size_t, void*> free_;
  std::map<void*, size_t> size_;
  size_t cached_ = 0;
};

// Page-locked host buffers handed out by emqx_gm_host_alloc: the host-buffer
// match sends topic text that lies in one of them by DMA, without staging it
// (gm_host.cpp).  Process-wide, so a buffer is found from any context.
bool host_pinned_range(const void* p, size_t bytes);
void host_pinned_add(void* p, size_t bytes);
bool host_pinned_remove(void* p);

// RAII handle on a pool buffer.
struct PoolBuf {
  DevPool* pool = nullptr;
  void* p = nullptr;
  PoolBuf() = default;
  PoolBuf(DevPool* pl, size_t bytes) : pool(pl), p(pl->alloc(bytes)) {}
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
  PoolBuf(PoolBuf&& o) noexcept : pool(o.pool), p(o.p) { o.p = nullptr; }
  PoolBuf& operator=(PoolBuf&& o) noexcept {
    reset();
    pool = o.pool;
    p = o.p;
    o.p = nullptr;
    return *this;
  }
  ~PoolBuf() { reset(); }
  void reset() {
    if (p && pool) pool->release(p);
    p = nullptr;
  }
  void* release_ownership() {
    void* q = p;
    p = nullptr;
    return q;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// RAII handle on a page-locked staging buffer of a PinPool (empty until get()).
struct PinBuf {
  PinPool* pool;
  void* p = nullptr;
  explicit PinBuf(PinPool* pl) : pool(pl) {}
  PinBuf(PinPool* pl, size_t bytes) : pool(pl), p(pl->get(bytes)) {}
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() {
    if (p) pool->put(p);
  }
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }  // a: a power of two
inline size_t al16(size_t x) { return align_up(x, 16); }
inline size_t al32(size_t x) { return align_up(x, 32); }

// Per-call scratch sizes of the match pipeline.
constexpr int FAST_FC = 8;    // frontier capacity per lane (LDS)
constexpr int FAST_MC = 16;   // match capacity per lane (LDS)
constexpr uint32_t OVF_BIT = 0x80000000u;
constexpr uint32_t LIST_BIT = 0x40000000u;  // compact staging: the row is listed-pass row (cnt & ~LIST_BIT)
constexpr uint32_t CNT_MASK = 0x7FFFFFFFu;

}  // namespace gm

namespace gm {
struct HostPipe;  // gm_host.cpp: pinned staging + copy streams + worker threads of the host-buffer path
}

struct emqx_gm_ctx {
  int device = 0;
  uint32_t open_flags = 0;  // emqx_gm_opts.flags (EMQX_GM_OPEN_*)
  gm::HostPipe* host = nullptr;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // assembly stream (gm_match.hip MatchCall): a large device-buffer call's
  // scan + assembly run here behind its main pass, so the next call's main
  // pass (context stream) overlaps them
  hipStream_t stream_asm = nullptr;
  std::recursive_mutex mu;
  gm::DevPool* pool = nullptr;
  gm::HostPool* hpool = nullptr;
  gm::PinPool* pins = nullptr;  // (thread safe: small host calls stage outside mu)
  emqx_gm_match_stats stats{};
  hipEvent_t ev[6]{};
  // per match call (gm_match.hip MatchCall, under mu): reusable events and
  // 64-B pinned read-back slots, so several calls can be in flight
  std::vector<hipEvent_t> ev_free;
  std::vector<void*> pin_free, pin_all;
  double ids_per_topic = 4.0;  // speculative ids capacity of a match call (run_match), from recent calls
  double subs_per_match = 16.0;  // speculative deliveries capacity of a small host fan-out, from recent calls
  // speculative pick / plan capacities of a publish window (gm_publish.hip), from recent windows
  double hits_per_match = 1.0, pairs_per_match = 1.0;
  // A ring of 64-B pass-counter blocks (gm_match.hip MatchCall): a call takes
  // the next block, already zeroed -- the previous call's assembly kernel zeroes
  // it -- so a call needs no zeroing launch of its own.  State per block: 0 ready
  // (zero, or zeroed by a kernel queued before any later use), 1 held by a call,
  // 2 dirty (its call is done).
  static constexpr int CTR_RING = 16;
  void* ctr_ring = nullptr;
  uint8_t ctr_state[CTR_RING] = {};
  int ctr_next = 0;
  // A multi-device context (emqx_gm_opts.n_devices > 1): this context is the
  // first listed device; members[k - 1] serves devices[k] (its own stream,
  // pools and host pipeline; used only under this context's lock).  Every
  // index made through this context carries a replica per member
  // (emqx_gm_index::reps).
  std::vector<emqx_gm_ctx*> members;
  emqx_gm_ctx* parent = nullptr;    // a member: its multi-device context
  std::atomic<uint32_t> rr{0};      // round-robin start of the next small host-buffer call (gm_api.cpp)
  std::vector<struct emqx_gm_combiner*> combiners;  // opened on this context (gm_api.cpp): freed with it
};

namespace gm {
struct OverlayState;

// The library's A/B and diagnostic knobs (GM_* environment variables: table
// layout, load factor, walk form, staging, update path, host pipeline) are
// read only when EMQX_GM_AB is set (non-empty, not "0"), so a library loaded
// into a BEAM runs its one default layout and walk whatever else the host's
// environment holds (the list: emqx_gpu_match.h).  Read per call, so a test
// or an A/B script sets it beside the knob.
inline const char* knob(const char* name) {
  const char* ab = getenv("EMQX_GM_AB");
  if (!ab || !*ab || (ab[0] == '0' && !ab[1])) return nullptr;
  return getenv(name);
}

// Whether a match call on view v takes the flat instantiations of the walk
// kernels: a table the buffer form could not address with 32-bit byte offsets
// under a 2 GiB descriptor (a hot table: IX_HOT_FLAT, set at build; the word
// dictionary, an MPH table's bucket words, an exact-edge filter), or the
// GM_HOT_FLAT test knob.
inline bool view_flat(const IndexView& v) {
  constexpr uint64_t LIM = 1ull << 31;
  if (v.flags & IX_HOT_FLAT) return true;
  if ((v.dict_mask + 1) * sizeof(DictSlot) >= LIM) return true;
  for (int t = 0; t < HOT_TABLES; ++t)
    if (v.hot_cap[t] * sizeof(HotSlot) >= LIM || uint64_t(v.mph_nb[t]) * 8 >= LIM ||
        (uint64_t(v.efilt_mask[t]) + 1) * 4 >= LIM)
      return true;
  return false;
}

// What the calling thread's last index call did (emqx_gm_last_update_stats):
// the entry points reset it, the update paths fill it in.
extern thread_local emqx_gm_update_stats tl_ustats;
double now_ms();

// The id change of an in-place update, from O(delta) lists: prev ids `dels`
// deleted (ascending), new filter k (byte order) inserted with addpos[k] prev
// filters sorting before it and temporary id nb + k.  map(): prev id -> new id
// (NONE: deleted) = id - (dels below it) + (inserts at or before it); a
// temporary nb + k -> addpos[k] - (dels below addpos[k]) + k.  The device
// builds the whole table with a kernel (apply_patch_device); table() is the
// host twin, materialized only where the host needs it.
struct IdShift {
  uint64_t nb = 0;
  std::vector<uint64_t> dels, addpos;
  uint32_t map(uint64_t id) const {
    if (id >= nb) {
      const uint64_t k = id - nb, p = addpos[k];
      return uint32_t(p - (std::lower_bound(dels.begin(), dels.end(), p) - dels.begin()) + k);
    }
    if (std::binary_search(dels.begin(), dels.end(), id)) return NONE;
    return uint32_t(id - (std::lower_bound(dels.begin(), dels.end(), id) - dels.begin()) +
                    (std::upper_bound(addpos.begin(), addpos.end(), id) - addpos.begin()));
  }
  // indexed like the table (renum_field): map() without materializing it
  uint32_t operator[](uint64_t id) const { return map(id); }
  std::vector<uint32_t> table() const {
    std::vector<uint32_t> r(nb + addpos.size());
    uint64_t d = 0, a = 0;
    for (uint64_t id = 0; id < nb; ++id) {
      while (a < addpos.size() && addpos[a] <= id) ++a;
      if (d < dels.size() && dels[d] == id) {
        r[id] = NONE;
        ++d;
        continue;
      }
      r[id] = uint32_t(id - d + a);
    }
    for (uint64_t k = 0; k < addpos.size(); ++k) r[nb + k] = map(nb + k);
    return r;
  }
};

// Host copy of a plain index's device blob (no shard ids, no subscriber
// lists), byte for byte, with the headroom an in-place update may use
// (gm_overlay.cpp, patch_update): appended trie nodes, new words in the
// arena, more filter lengths.  It belongs to the newest snapshot of its line:
// an update moves it from the old snapshot (which stays valid for its readers)
// to the new one.
struct Mirror {
  HostBytes blob;                        // empty until the first update when built lazily (load_mirror_blob)
  size_t blob_size = 0;                  // bytes of the blob: the device tables up to the subscriber CSR
  size_t o_nodes = 0, o_dict = 0, o_edges = 0, o_hot = 0, o_arena = 0, o_flen = 0, o_efilt = 0, o_mph = 0;
  uint64_t nodes_n = 0, nodes_cap = 0;   // v1 level-trie nodes used / capacity
  uint64_t arena_n = 0, arena_cap = 0;   // word bytes used / capacity
  uint64_t flen_cap = 0;                 // filter-length entries available
  uint64_t dict_used = 0;
  uint64_t edge_used[EDGE_DEPTHS] = {};
  uint64_t hot_used[HOT_TABLES] = {};
  uint64_t mph_ovf_used[HOT_TABLES] = {};  // keys in each MPH table's overflow region
};
}

struct emqx_gm_index {
  std::atomic<int> refs{1};
  int device = 0;
  void* dev_base = nullptr;     // one allocation holding every table
  void* dev_subs = nullptr;     // a subscriber CSR of its own (after emqx_gm_index_update_subs), or nullptr
  size_t subs_bytes = 0;        // ... its bytes
  emqx_gm_index* blob_owner = nullptr;  // set: dev_base is that (retained) snapshot's blob, shared
  void* dev_gmap = nullptr;     // a shard's id map of its own (after a sharded update, gm_shard.cpp): view.gmap, or nullptr
  size_t dev_bytes = 0;
  gm::IndexView view{};
  uint16_t* dev_flen = nullptr; // filter lengths (stats only), inside dev_base
  mutable std::atomic<bool> flen_stale{false};  // dev_flen not yet rewritten after an in-place update
  mutable std::mutex flen_mu;
  // host copies
  gm::FilterTable ft;           // the sorted unique filters (id = rank), gm_filters.h
  std::vector<uint32_t> gmap;   // shard index: global id of each local filter (ascending); empty otherwise
  gm::SubTable subs;            // per filter id: subscriber CSR offset and route mark (emqx_gm_index_update_subs
                                // ROUTE_ADD); empty without subscriber lists.  gm_filters.h
  gm::OverlayState* ov = nullptr;  // overlay snapshot (emqx_gm_index_update); tables above unused then
  uint64_t level_nodes = 0;        // an upper bound on the trie nodes of any one depth (the slow path's frontier); 0: unknown
  gm::Mirror* mirror = nullptr;    // host copy of the blob (updatable plain index), see gm::Mirror
  std::mutex mirror_mu;            // an in-place update holds it while it patches and hands the mirror on
  emqx_gm_index_info_t info{};
  // made through a multi-device context: reps[k - 1] = this snapshot on that
  // context's members[k - 1] (same rows; its own device tables, or the tables
  // of an older replica it shares as this snapshot shares its owner's).  Owned:
  // released with this snapshot.
  std::vector<emqx_gm_index*> reps;
  bool reused_blob = false;  // (replicate_index: dev_base was a released snapshot's blob)
  // a prefix-sharded index (emqx_gm_index_build_sharded, gm_shard.cpp): shards[k]
  // on the context's k-th device (a shard index with global ids), route sends a
  // topic to its one shard, fshard[global id] = a filter's shard (or
  // EMQX_GM_ALL_SHARDS).  This object holds only the host side (ft, subs, info).
  std::vector<emqx_gm_index*> shards;
  emqx_gm_route* route = nullptr;
  std::vector<uint32_t> fshard;
};

namespace gm {
// gm_index.cpp
int build_index(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n, const uint64_t* sub_off,
                const uint32_t* sub_ids, uint32_t* perm_out, emqx_gm_index** out,
                emqx_gm_index_info_t* host_only = nullptr, const uint32_t* gids = nullptr,
                bool shard_mirror = false);  // shard_mirror: a shard index (gids) built updatable (build_sharded)
void sort_filters(std::vector<uint32_t>& ord, const uint8_t* fb, const uint64_t* fo);
void free_index(emqx_gm_index* idx);
// gm_index.cpp: a freed snapshot's device blob kept, one per device, for the
// next in-place update of that size (a large fresh hipMalloc after a few
// update / free cycles stalls: C5's 38 GB blob took ~1 s from the 7th update on,
// 0.3 ms before).  take: a spare of at least `bytes` (at most 1.25x), or null;
// give: keeps p (the device synchronized first, as hipFree does) or frees it;
// trim: frees the device's spare (emqx_gm_pool_trim, emqx_gm_close).
void* take_spare_blob(int device, size_t bytes);
void give_spare_blob(int device, void* p, size_t bytes);
void trim_spare_blob(int device);
// open contexts per device (emqx_gm_open / _close): a blob freed while none is
// open on its device is not kept (nothing would trim it)
void note_ctx_open(int device);
void note_ctx_close(int device);
// gm_match.hip
// A caller's work queued on the context stream right behind the speculative
// assembly of a DEVICE_IO match, before run_match's one host round trip (the
// host path queues the rows' copy-out there).  enqueue(row_off, ids, cap) gets
// the device rows and the ids capacity; `used` says whether those rows are the
// call's result (no reassembly happened).
struct MatchTail {
  std::function<int(const uint64_t* row_off, const uint32_t* ids, uint64_t cap)> enqueue;
  bool used = false;
};
int run_match(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
              uint32_t flags, emqx_gm_csr* out, MatchTail* tail = nullptr);
// the two halves of run_match (emqx_gm_match_submit / _wait): submit under
// ctx->mu; wait without it (it takes the lock after the device wait)
// tail (optional): as run_match's, kept by the caller until match_wait;
// st_out (optional): the call's own stats (ctx->stats may belong to a later call by then)
int match_submit(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                 uint32_t flags, void** ticket, MatchTail* tail = nullptr);
int match_wait(emqx_gm_ctx* ctx, void* ticket, emqx_gm_csr* out, MatchTail* tail = nullptr,
               emqx_gm_match_stats* st_out = nullptr);
// write the root's '+' record (IndexView::d0_root) from view v's
// depth-1 hot table on the device; d0 is the region's device address (v's own
// pointer is const).  0: written (the caller sets IX_D0), 1: not wanted
// (GM_D0=0), <0: error.
int refresh_d0(emqx_gm_ctx* ctx, const IndexView& v, void* d0);
// a call's device rows handed out as its result (device_out: the pool buffers
// themselves; else copied into host buffers of the context's pool), and the
// time between two events (0 when either was not recorded); also used by gm_csr.hip
int finish_csr(emqx_gm_ctx* ctx, uint64_t n, uint64_t nnz, PoolBuf& row_off, PoolBuf& ids, bool device_out,
               emqx_gm_csr* out);
float ev_ms(hipEvent_t a, hipEvent_t b);
// gm_csr.hip: what consumes finished rows
int run_fanout(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
               emqx_gm_csr* out, uint32_t part = 0, uint32_t n_parts = 1, uint64_t* first_out = nullptr);
// the device work of a small host fan-out (gm_host.cpp run_fanout_small) and of
// the fan-out behind a small host call's speculative rows (run_host_small), queued without a wait
int queue_fanout_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint64_t* d_off, const uint32_t* d_ids,
                       uint64_t n, uint64_t nnz, uint64_t total, uint64_t* seg_dst, uint64_t* row_off, uint32_t* ids);
int queue_fanout_spec(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint64_t* d_ro, const uint32_t* d_ids,
                      uint64_t n, uint64_t cap_m, uint64_t cap_f, uint64_t* seg_dst, uint64_t* row_off, uint32_t* ids);
// Output elements per workgroup: from 1,024 (a publish window's ~100k
// deliveries in ~100 workgroups, not 30: 63 -> ~20 us) up to 65,536 for large
// fan-outs (C4: 0.94 -> 0.81 ms against 4,096, fewer per-block segment
// searches), a multiple of 1,024 (4 per thread step).  Also used by
// gm_update.hip (its segment copies cut their output the same way).
inline uint64_t fan_per_block(uint64_t total) {
  uint64_t per = total / 2048;  // ~8 workgroups per CU
  per = per < 1024 ? 1024 : per > 65536 ? 65536 : per;
  return (per + 1023) & ~uint64_t(1023);
}
int run_merge_rows(emqx_gm_ctx* ctx, uint64_t n_rows, uint64_t stride, uint32_t n_pieces, const uint32_t* d_lens,
                   const uint32_t* d_ids, uint32_t flags, emqx_gm_csr* out);
int run_row_lengths(emqx_gm_ctx* ctx, const emqx_gm_csr* csr, uint32_t* d_out);
int run_match_overlay(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                      uint32_t flags, emqx_gm_csr* out);
int unpermute_rows(emqx_gm_ctx* ctx, uint64_t n, const uint32_t* d_perm, const uint32_t* d_lens, const uint32_t* d_ids,
                   uint32_t flags, emqx_gm_csr* out);
int scan_lengths(emqx_gm_ctx* ctx, const uint64_t* len, uint64_t n, uint64_t* out);
// the host path's u16 topic lengths -> u64 offsets (n + 1 entries, an exclusive scan) on stream st
int scan_len16(emqx_gm_ctx* ctx, hipStream_t st, const uint16_t* len, uint64_t n, uint64_t* out);
// offset conversions of the host-buffer path (n1 = entries)
int launch_off32_to_64(hipStream_t st, const uint32_t* in, uint64_t n1, uint64_t* out);
int launch_off64_to_32(hipStream_t st, const uint64_t* in, uint64_t n1, uint32_t* out);
int launch_copy_u32x2(hipStream_t st, const uint32_t* s0, uint32_t* d0, uint64_t n0, const uint32_t* s1, uint32_t* d1,
                      uint64_t n1, const uint64_t* n1_max = nullptr);
int launch_add_u64(hipStream_t st, uint64_t* p, uint64_t n1, uint64_t add);
// the fan-out's row offsets from segment offsets: out_off[i] = seg_dst[min(m_off[i], nseg)], i in [0, n]
int launch_fanout_rowoff(hipStream_t st, const uint64_t* m_off, uint64_t n, const uint64_t* seg_dst, uint64_t* out_off,
                         uint64_t nseg);
// prefix sharding (gm_route.hip) and the exchange's device steps
int route_plan(const uint8_t* fb, const uint64_t* fo, uint64_t n, uint32_t n_shards, uint32_t* shard_out,
               emqx_gm_route** out);
int route_topics_host(const emqx_gm_route* r, const uint8_t* tb, const uint64_t* to, uint64_t n, uint32_t* dest);
int route_topics_device(emqx_gm_ctx* ctx, emqx_gm_route* r, const uint8_t* d_tb, const uint64_t* d_to, uint64_t n,
                        uint32_t* d_dest);
int route_partition(emqx_gm_ctx* ctx, emqx_gm_route* r, const uint8_t* d_tb, const uint64_t* d_to, uint64_t n,
                    uint32_t* d_perm, uint32_t* d_plen, uint64_t* d_split);
void free_route(emqx_gm_route* r);  // drops one reference
void retain_route(emqx_gm_route* r);
uint32_t route_n_shards(const emqx_gm_route* r);
// the shard of a filter under a fixed route (EMQX_GM_ALL_SHARDS: every one), gm_route.hip
uint32_t route_filter_shard(const emqx_gm_route* r, const uint8_t* f, uint64_t len);
int route_filter_shards_host(const emqx_gm_route* r, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                             uint32_t* shard_out);
int permute_topics(emqx_gm_ctx* ctx, const uint8_t* d_tb, const uint64_t* d_to, uint64_t n, const uint32_t* d_perm,
                   uint8_t* d_out, uint64_t* d_out_off);

// A replica an update makes on member context m from prev's replica `prev`
// (gm_overlay.cpp patch_update, gm_subs.cpp update_subs): each member applies
// the same O(delta) plan to its own device copy at the same time as the first
// device -- the reference's every-node-applies-the-delta replication
// (apps/emqx/src/emqx_router_utils.erl:33-38, emqx_trie.erl:114-136).
struct RepTarget {
  emqx_gm_ctx* m = nullptr;
  emqx_gm_index* prev = nullptr;
  emqx_gm_index* out = nullptr;  // made by the update (owned by the caller until attached)
};
// gm_overlay.cpp — incremental index maintenance.  An
// overlay snapshot = an immutable base snapshot (shared, retained) minus
// tombstoned base filters plus a small delta index over the inserted filters.
// Final filter ids are ranks in the updated set: a surviving base id b maps to
// b + (delta filters sorting before b) - (tombstones below b); delta filters
// carry their final ids directly (shard-style global ids).
struct OverlayState {
  emqx_gm_index* base = nullptr;     // retained flat snapshot
  emqx_gm_index* delta = nullptr;    // flat snapshot over the inserted filters, or nullptr
  std::vector<uint32_t> tomb;        // deleted base ids, ascending
  std::vector<uint32_t> ins;         // per delta filter (byte order): base filters sorting before it
  std::vector<uint32_t> dgid;        // per delta filter: final id
  std::vector<uint8_t> dbytes;       // delta filters, byte order
  std::vector<uint64_t> doff;
  void* dev = nullptr;               // tomb bitmap | its word prefix counts | ins
  const uint32_t* d_tbm = nullptr;
  const uint32_t* d_tpre = nullptr;
  const uint32_t* d_ins = nullptr;
};
int update_index(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo, const uint8_t* ops,
                 uint64_t n_ops, emqx_gm_index** out);
// The in-place patch of update_index (prev must hold the mirror and a write
// lock on it): deletes base ids `tomb`, inserts the filters `dset`.  Returns 1
// when a table lacks room (nothing changed), <0 on error.  rmap_out (optional)
// receives old id -> new id for prev's filters (NONE: deleted) followed by the
// new ids of dset's filters in byte order.
// trie_only: the new blob holds the tables up to the subscriber CSR only (the
// caller gives the snapshot a CSR of its own).
// reps (optional): the member replicas to patch alongside (RepTarget::out set on success).
// gs (optional, a shard of a sharded index): the new snapshot gets an id map
// of its own (dev_gmap), written in the same device step.
struct GmapShift;
int patch_update(emqx_gm_ctx* ctx, emqx_gm_index* prev, const std::set<uint32_t>& tomb,
                 const std::set<std::string>& dset, emqx_gm_index** out, std::vector<uint32_t>* rmap_out = nullptr,
                 bool trie_only = false, std::vector<RepTarget>* reps = nullptr, const GmapShift* gs = nullptr);
bool well_formed_filter(const uint8_t* p, uint64_t len);
int overlay_filter(const emqx_gm_index* idx, uint32_t id, const uint8_t** bytes, uint64_t* len);
void free_overlay(emqx_gm_index* idx);
// gm_image.cpp: index images (emqx_gm_index_export / _import) and the lazy host mirror
int index_export(emqx_gm_ctx* ctx, const emqx_gm_index* idx, uint32_t flags, uint8_t* buf, uint64_t* size);
int index_import(emqx_gm_ctx* ctx, const uint8_t* img, uint64_t size, const void* d_blob, emqx_gm_index** out);
int load_mirror_blob(emqx_gm_ctx* ctx, emqx_gm_index* idx);
// an image's every count and offset checked against its own bytes (no device);
// EMQX_GM_EINVAL with the reason in *why
int validate_image(const uint8_t* img, uint64_t size, bool have_blob, std::string* why);
// the host half of an import (validate_image, then the host tables into idx;
// its view's pointer fields hold blob offsets + 1, 0 = null)
int import_host_part(const uint8_t* img, uint64_t size, bool have_blob, emqx_gm_index* idx, std::string* why);
// test support (tests/asan): a named u64 header field of an image (nullptr:
// unknown name), a u32 count of its view (0 n_nodes, 1 efilt_mask[t], 2
// mph_nb[t]), and the checksum recomputed after a change
uint64_t* image_field(uint8_t* img, const std::string& name);
uint32_t image_view_u32(uint8_t* img, int which, int t);
void image_view_set_u32(uint8_t* img, int which, int t, uint32_t x);
void image_reseal(uint8_t* img, uint64_t size);
// a plain index's host mirror is kept from the build when its tables are at most this big
// (C3's 4.6 GB tables keep theirs: a lazy first update downloads the tables,
// 0.8 s at C3 over pageable copies; the 38 GB C5 index does not)
constexpr size_t kEagerMirrorBytes = size_t(8) << 30;
// rank of f among idx's filters; *found = exact hit
uint64_t filter_rank(const emqx_gm_index* idx, const uint8_t* f, uint64_t len, bool* found);
// gm_subs.cpp: emqx_gm_index_update_subs
int update_subs(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo, const uint32_t* subs,
                const uint8_t* ops, uint64_t n_ops, emqx_gm_index** out);
bool is_pinned(const emqx_gm_index* idx, uint64_t f);
// gm_update.hip: the device side of in-place updates (to the next file heading)
// segments [src_off[j], src_off[j] + (dst_off[j+1] - dst_off[j])) of
// the device array src gathered into host `out` (dst_off[m] elements), one
// device gather + one copy back
int gather_segments(emqx_gm_ctx* ctx, const uint32_t* src, const std::vector<uint64_t>& src_off,
                    const std::vector<uint64_t>& dst_off, uint32_t* out);
// the new subscriber CSR of a subscriber-only update_subs batch
// (ids unchanged; O(delta) host work, see there)
int shift_subs_device(emqx_gm_ctx* ctx, const emqx_gm_index* prev, emqx_gm_index* idx,
                      const std::vector<uint32_t>& aff_ids, const std::vector<uint64_t>& aff_off,
                      const std::vector<uint32_t>& aff_buf);
// the new subscriber CSR of update_subs (see there)
int rebuild_subs_device(emqx_gm_ctx* ctx, const emqx_gm_index* prev, emqx_gm_index* idx,
                        const std::vector<uint64_t>& new_soff, const std::vector<uint32_t>& inv,
                        const std::vector<uint32_t>& aff_ids, const std::vector<uint64_t>& aff_off,
                        const std::vector<uint32_t>& aff_buf);
// An op of Patcher::orops whose offset carries PATCH_AND clears its bits
// instead of setting them (an op never sets a bit another op clears, so the
// device applies them in any order).
constexpr uint64_t PATCH_AND = 1ull << 63;
// the device side of an in-place update (patch_update): dst =
// src (bytes), then the host-patched byte ranges (offset, length) of `host`
// written over it, the OR / AND ops (offset of a word, bits) applied, then every
// filter-id field of the hot slots and of nodes [0, n_nodes) renumbered by
// the shift (its table built on the device).  Done in one pass over the blob:
// the hot slots and nodes are renumbered while copied and the patched ranges
// go up already renumbered (GM_UPDATE_UNFUSED: copy, patch, then renumber in
// place -- the A/B twin).
int apply_patch_device(emqx_gm_ctx* ctx, void* dst, const void* src, size_t bytes,
                       const std::vector<std::pair<uint64_t, uint32_t>>& ranges, const uint8_t* host,
                       const IndexView& v, uint64_t o_hot, uint64_t o_nodes, uint64_t n_nodes,
                       const IdShift& shift, const std::vector<std::pair<uint64_t, uint32_t>>& orops);
// ... of a shard of a sharded index: gmap (nullptr: none) is the shard's new id
// map, queued behind the patch on the same stream (k_gmap_shift reads the
// shift's device table); one synchronize covers both.
struct GmapJob;
int apply_patch_device_gmap(emqx_gm_ctx* ctx, void* dst, const void* src, size_t bytes,
                            const std::vector<std::pair<uint64_t, uint32_t>>& ranges, const uint8_t* host,
                            const IndexView& v, uint64_t o_hot, uint64_t o_nodes, uint64_t n_nodes,
                            const IdShift& shift, const std::vector<std::pair<uint64_t, uint32_t>>& orops,
                            const GmapJob* gmap);
// The id change of a sharded update as one shard sees it (gm_shard.cpp): G is
// the GLOBAL shift (old global id -> new), add_gid the final global ids of the
// filters this shard gains, in byte order.
struct GmapShift {
  const IdShift* G = nullptr;
  const std::vector<uint32_t>* add_gid = nullptr;
};
// k_gmap_shift: a shard's new local-to-global id map.  For every
// old or temporary local id i < nb + add_gid.size(): j = L(i) (rmap on the
// device, the shard's local shift; nullptr: the identity, no local change;
// NONE: deleted), new_gmap[j] = G(old_gmap[i]) for i < nb, else add_gid[i - nb].
struct GmapJob {
  const uint32_t* old_gmap = nullptr;  // device, nb entries ascending (may be null when nb == 0)
  uint64_t nb = 0;
  GmapShift sh;
  uint32_t* new_gmap = nullptr;  // device, n_new entries
  uint64_t n_new = 0;
};
// a shard without local changes: its new map alone (queued and waited for on ctx's stream)
int shift_gmap_device(emqx_gm_ctx* ctx, const GmapJob& job);
// gm_api.cpp
int set_err(emqx_gm_ctx* ctx, int code, const std::string& msg);
// gm_host.cpp: emqx_gm_match on host buffers, chunked and pipelined (H2D / match / D2H overlap)
int run_match_host(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                   uint32_t flags, emqx_gm_csr* out);
void free_host_pipe(emqx_gm_ctx* ctx);
// the topics of one host-pipeline chunk at most (a call this small runs whole on one device)
uint64_t host_chunk_topics();
// A host-buffer call of at most one chunk, entered WITHOUT ctx->mu: staged into
// the call's own page-locked buffer outside the lock, queued under it (inputs
// up, the match, the rows' copy-out behind its speculative assembly straight
// into the page-locked result; copies up to 1 MiB as kernels over mapped
// memory), waited for outside it -- so concurrent small calls on one device
// overlap one another's host work and device round trips
// fan (optional, emqx_gm_match_fanout): the call's fan-out queued behind its
// speculative rows in the same round trip; fan->ok says whether it held (the
// match's rows and the deliveries both within their capacities)
struct SmallFan {
  emqx_gm_csr out{};
  bool ok = false;
  // (why not, for the tests' message: queued, the rows were the speculative ones, deliveries vs capacity)
  bool queued = false, rows_spec = false;
  uint64_t total = 0, cap = 0;
};
// side (optional, emqx_gm_publish_window): a stage of the caller's behind the
// speculative rows and fan-out, in the same round trip.  queue(row_off, ids,
// cap) runs under ctx->mu before the call's one wait, with the device rows and
// their ids capacity; it keeps its own failures (it then queued nothing).
// finish(rows_spec, rows) runs under ctx->mu after the wait, while the call's
// true device rows are still held: rows_spec says whether they are the ones
// queue() saw.  A finish() that fails fails the call, which then returns nothing.
struct SmallSide {
  std::function<void(const uint64_t* row_off, const uint32_t* ids, uint64_t cap)> queue;
  std::function<int(bool rows_spec, const emqx_gm_csr* rows)> finish;
};
int run_host_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                   uint32_t flags, emqx_gm_csr* out, emqx_gm_match_stats* st_out, SmallFan* fan = nullptr,
                   SmallSide* side = nullptr);
// A host-row fan-out of a publish window, the same way (entered WITHOUT
// ctx->mu): the rows staged outside the lock, the deliveries written into a
// speculative capacity, one device round trip.  idx: the snapshot on this
// device (a replica), host: the primary (its filter count).  Returns 1 --
// nothing delivered -- for rows that are not a plain CSR, a fan-out whose
// expected size is past kFanSmallDeliveries, or one past its capacity: the
// caller takes the ordinary path.
int run_fanout_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_index* host, const emqx_gm_csr* m,
                     emqx_gm_csr* out, emqx_gm_match_stats* st_out);
// A group of publish windows as ONE device batch (emqx_gm_match_windows; entered
// WITHOUT ctx->mu, like run_host_small): the windows' text and u16 lengths
// concatenated in one page-locked staging buffer with the window table behind
// them, one input copy, one scan, one match, the fan-out behind its
// speculative rows when deliveries are wanted, then ONE k_rows_split launch
// (gm_windows.hip) that cuts the group's CSRs into each window's own
// page-locked result.  The caller has checked: every window small-call
// eligible with monotone offsets and no topic past 65,535 B, the group within
// host_chunk_topics() topics and host_window_text_max() bytes of text.
// matches[k] always comes back; deliveries[k] where fan_ok[k] (else zeroed:
// the caller fans that window's rows out itself).  On error nothing is returned.
struct WinSlice {  // one window's part of one of the group's CSRs (the window table: [window][CSR])
  uint64_t row0, n_rows;  // its rows in the group
  uint64_t ids_cap;       // ids its result holds
  uint64_t* dst_row_off;  // its result as the device addresses it: n_rows + 1 offsets from 0
  uint32_t* dst_ids;
};
int launch_rows_split(hipStream_t st, const WinSlice* tab, uint32_t n_windows, uint64_t max_work, const uint64_t* ro0,
                      const uint32_t* ids0, uint64_t cap0, const uint64_t* ro1, const uint32_t* ids1, uint64_t cap1);
// The cut of a group's forward plan into the windows' own (gm_windows.hip
// k_plan_bounds, k_plan_cut; emqx_gm_publish_windows).  tab[w]: window w's rows
// in the group and its result as the device addresses it; win_row0: the
// windows' first rows, n_windows + 1 ascending entries; lb: (n_windows + 1) x
// n_nodes u32 of workspace, written when `bounds` (a relaunch for one window
// passes tab + w, lb + w * n_nodes and bounds = false).  node_off / rows /
// filters / row_routes: the group's plan within cap_pairs entries; *total_p,
// the group's true pair count, is copied to *total_out.
struct PlanSlice {
  uint64_t row0, n_rows;   // its rows in the group
  uint64_t pairs_cap;      // pairs its result holds
  uint64_t* dst_node_off;  // n_nodes + 1 offsets from 0 (the last: its true pair count)
  uint32_t *dst_rows, *dst_filters, *dst_row_routes;
};
int launch_plan_cut(hipStream_t st, const PlanSlice* tab, uint32_t n_windows, uint64_t max_work,
                    const uint32_t* win_row0, uint32_t* lb, bool bounds, const uint64_t* node_off, const uint32_t* rows,
                    const uint32_t* filters, const uint32_t* row_routes, uint32_t n_nodes, uint64_t cap_pairs,
                    const uint64_t* total_p, uint64_t* total_out);
uint64_t host_window_text_max();
void free_combiners(emqx_gm_ctx* ctx);  // gm_api.cpp: closes and frees the context's combiners (emqx_gm_close)
// side (optional, emqx_gm_publish_windows): the group analogue of SmallSide.
// extra_bytes of room behind the group's staged input travel up with the same
// copy: stage(host) fills what is known outside the lock (the windows' hashes);
// prepare(host, dev) runs under ctx->mu before the input copy is queued (the
// windows' tables: their capacities come from the context's state).  queue()
// runs from the match's tail behind the group's speculative rows and fan-out,
// finish() after the wait, under the lock, while the true device rows are held;
// a finish() that fails fails the group.  A group without a topic calls none.
struct WindowsSide {
  size_t extra_bytes = 0;
  std::function<void(uint8_t* host)> stage;
  std::function<void(uint8_t* host, const uint8_t* dev)> prepare;
  std::function<void(const uint64_t* row_off, const uint32_t* ids, uint64_t cap)> queue;
  std::function<int(bool rows_spec, const emqx_gm_csr* rows)> finish;
};
int run_host_windows(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_window* w, uint32_t g, uint32_t flags,
                     emqx_gm_csr* matches, emqx_gm_csr* deliveries, uint8_t* fan_ok, emqx_gm_match_stats* st_out,
                     WindowsSide* side = nullptr);
// gm_multi.cpp: multi-device contexts (emqx_gm_opts.n_devices).
// A copy of flat snapshot `src` (any device) on member context m's device:
// the host tables shared or copied, the device tables copied device to device
// (peer copy across devices) -- or, with `share` (a replica on m whose device
// tables hold the bytes src's own tables hold: src shares its owner's blob and
// share is that owner's replica), those tables shared.  No host mirror (the
// primary snapshot's line owns it).
int replicate_index(emqx_gm_ctx* m, const emqx_gm_index* src, emqx_gm_index* share, emqx_gm_index** out);
// f(k) for k = 0..K-1 at once, one thread each (k = 0 on the calling thread);
// the first failure's code, its message set on the calling thread
int run_all(int K, const std::function<int(int)>& f);
// the targets of an update of `prev` through ctx: one per member when prev has
// its replicas there, else none (the result is copied by replicate_result)
std::vector<RepTarget> rep_targets(emqx_gm_ctx* ctx, emqx_gm_index* prev);
// a new replica on m carrying src's host fields (filter table, subscriber
// table, info; shared bases) and no device tables yet
emqx_gm_index* replica_shell(emqx_gm_ctx* m, const emqx_gm_index* src);
// attach the targets' replicas to out (all made), or free them (rc != 0)
int attach_replicas(emqx_gm_index* out, std::vector<RepTarget>& t, int rc);
// After an index call on a multi-device context made `out` from `prev` (NULL
// for a build / import): give `out` its replicas unless the update already
// made them (an in-place patch or update_subs applies its delta on every
// device, RepTarget).  A flat result is copied device to device in a tree
// (sharing prev's replica's tables when out shares prev's); an overlay stays
// on the first device.  On failure `out` is released and *out_p cleared.
int replicate_result(emqx_gm_ctx* ctx, emqx_gm_index* prev, emqx_gm_index** out_p);
// gm_shard.cpp: the prefix-sharded index of a multi-device context
int build_sharded(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n, const uint64_t* sub_off,
                  const uint32_t* sub_ids, uint32_t* perm_out, emqx_gm_index** out);
int run_match_sharded(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                      uint32_t flags, emqx_gm_csr* out);
int run_fanout_sharded(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
                       emqx_gm_csr* out);
// emqx_gm_index_update on a sharded index built without subscriber lists: each
// shard patched, given a new id map only, or rebuilt alone (all at once)
int update_sharded(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo, const uint8_t* ops,
                   uint64_t n_ops, emqx_gm_index** out);
// what each shard of the calling thread's last sharded update did (EMQX_GM_UPD_PATCH / _SHIFT / _REBUILD)
const std::vector<uint32_t>& last_shard_kinds();
// emqx_gm_fanout of host rows over a multi-device context's replicas (one
// slice per device, one page-locked result); small batches: run_fanout
int run_fanout_multi(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
                     emqx_gm_csr* out);
}  // namespace gm

#define GM_HIP(ctx, expr)                                                                     \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return gm::set_err((ctx), EMQX_GM_EDEVICE,                                              \
                         std::string(#expr) + ": " + hipGetErrorString(_e));                  \
  } while (0)

// The extern "C" entry points let no exception out: GM_GUARD_BEGIN ... GM_GUARD_END(ctx).
#define GM_GUARD_BEGIN try {
#define GM_GUARD_END(ctx)                                                  \
  }                                                                        \
  catch (const std::bad_alloc&) {                                          \
    return gm::set_err((ctx), EMQX_GM_ENOMEM, "host allocation failed");   \
  }                                                                        \
  catch (const std::exception& e) {                                        \
    return gm::set_err((ctx), EMQX_GM_EINVAL, e.what());                   \
  }                                                                        \
  catch (...) {                                                            \
    return gm::set_err((ctx), EMQX_GM_EINVAL, "unknown error");            \
  }

namespace gm {

// N events of one call, destroyed with it; `on` once create() made them all
template <int N> struct EventSet {
  hipEvent_t e[N] = {};
  bool on = false;
  int create(emqx_gm_ctx* ctx) {
    for (hipEvent_t& x : e) GM_HIP(ctx, hipEventCreate(&x));
    on = true;
    return EMQX_GM_OK;
  }
  ~EventSet() {
    for (hipEvent_t x : e)
      if (x) hipEventDestroy(x);
  }
};

// ---- the side tables (gm_retained / gm_shared / gm_authz): one blob compiled
// on the host, one device allocation holding a copy of it, a view over each.
// gm_api.cpp: table_upload copies the blob's first `bytes` bytes into a fresh
// allocation on ctx's device (*dev_base, set on success; errors read
// "<what>: device tables" and "<what>: upload: <hip error>"); table_free waits
// for the device, so no queued kernel still reads the tables.
int table_upload(emqx_gm_ctx* ctx, const HostBytes& blob, size_t bytes, const char* what, void** dev_base);
void table_free(int device, void* dev_base);
// a pointer into the host blob as the same place of the device allocation
template <class T> T* rebase(T* p, const void* host_base, void* dev_base) {
  return reinterpret_cast<T*>(static_cast<uint8_t*>(dev_base) +
                              (reinterpret_cast<const uint8_t*>(p) - static_cast<const uint8_t*>(host_base)));
}

// a batch of n byte strings b[o[i], o[i + 1]): fewer than 2^32 - 1 of them, ascending, each under 2 GiB
inline int check_offsets(const uint8_t* b, const uint64_t* o, uint64_t n, std::string* why) {
  if (n >= 0xFFFFFFFFull) {
    *why = "more than 2^32 - 2 entries";
    return EMQX_GM_EINVAL;
  }
  if (!o || (!b && n && o[n])) {
    *why = "NULL buffer";
    return EMQX_GM_EINVAL;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (o[i + 1] < o[i] || o[i + 1] - o[i] >= (1ull << 31)) {
      *why = "offsets not ascending (or an entry of 2 GiB) at " + std::to_string(i);
      return EMQX_GM_EINVAL;
    }
  return EMQX_GM_OK;
}

// a host walk's rows as a malloc'ed CSR (EMQX_GM_ENOMEM: the caller frees what was made), and its release
inline int csr_to_malloc(const std::vector<uint64_t>& row_off, const std::vector<uint32_t>& ids, emqx_gm_csr* out) {
  const uint64_t n = row_off.size() - 1;
  out->row_off = static_cast<uint64_t*>(malloc((n + 1) * 8));
  out->ids = static_cast<uint32_t*>(malloc(std::max<size_t>(ids.size(), 1) * 4));
  if (!out->row_off || !out->ids) return EMQX_GM_ENOMEM;
  std::memcpy(out->row_off, row_off.data(), (n + 1) * 8);
  if (!ids.empty()) std::memcpy(out->ids, ids.data(), ids.size() * 4);
  out->n_rows = n;
  out->nnz = ids.size();
  return EMQX_GM_OK;
}
inline int csr_free_malloc(emqx_gm_csr* csr) {
  if (!csr) return EMQX_GM_EINVAL;
  free(csr->row_off);
  free(csr->ids);
  std::memset(csr, 0, sizeof(*csr));
  return EMQX_GM_OK;
}

}  // namespace gm
