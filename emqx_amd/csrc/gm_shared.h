// gm_shared.h — the shared-subscription table: layout and pick rules shared by
// the host compiler and host walk (gm_shared.cpp) and the gfx950 kernels
// (gm_shared.hip).
//
// It answers emqx_shared_sub:dispatch/3's member selection (pick/6,
// do_pick/6, pick_subscriber/6, do_pick_subscriber/6,
// apps/emqx/src/emqx_shared_sub.erl:113-130, 234-288) for a whole publish
// window at once.  A SLOT is one {Group, Filter} pair with its member list
// (subscribers(Group, Topic), :287-288: an ets bag, insertion order, an
// identical member stored once).  Slots are sorted by (filter id, group id);
// sh_off maps a filter id of the bound snapshot to its slots.
//
// One allocation of u32 arrays, in this order:
//   sh_off  [n_filters + 1]  filter id -> its slots [sh_off[f], sh_off[f + 1])
//   mem_off [n_slots + 1]    slot -> its members in mem_ids
//   filter  [n_slots]        slot -> filter id
//   group   [n_slots]        slot -> the caller's group id
//   mem_ids [n_members]      the caller's member ids
//   rr      [n_slots]        round_robin state: the last Rem, or SH_UNSET
//   st      [n_slots]        sticky state: a member id, or SH_UNSET
// A built table holds in st only SH_UNSET or a member that IS in the slot's
// list (a member that left loses stickiness at the build), so the kernels need
// no membership search.
//
// The mix functions (one definition for the kernels, the host walk and the
// test restatement tests/_shared_ref.py), all arithmetic mod 2^32:
//   fmix(h):  h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
//   mix(a, b)     = fmix(fmix(a + 0x9E3779B9) + b)
//   mix3(a, r, s) = mix(mix(a, r), s)
// round_robin's unset start is r0(s) = mix(seed, s) rem Count, sticky's first
// pick members[mix(seed, s) rem Count], random's Nth - 1 = mix3(seed, row, s)
// rem Count (s the slot index, row the message row).
#pragma once

#include <mutex>

#include "gm_internal.h"

namespace gm {

constexpr uint32_t SH_UNSET = 0xFFFFFFFFu;

// (fmix is gm_common.h's fmix32)
GM_HD uint32_t sh_mix(uint32_t a, uint32_t b) { return fmix32(fmix32(a + 0x9E3779B9u) + b); }
GM_HD uint32_t sh_mix3(uint32_t a, uint32_t r, uint32_t s) { return sh_mix(sh_mix(a, r), s); }

struct ShView {
  const uint32_t* sh_off;
  const uint32_t* mem_off;
  const uint32_t* filter;
  const uint32_t* group;
  const uint32_t* mem_ids;
  uint32_t* rr;
  uint32_t* st;
  uint32_t n_filters, n_slots, n_members;
};

// The round-robin chunk rule: the hits are cut into C chunks of
// L = ceil(hits / C) consecutive hits; the workspace is C rows of n_slots u32.
// C is the largest count whose workspace stays within max(16 bytes per hit,
// SH_RR_WS_SMALL) -- proportional to the hits, with a small allowance so a
// publish window over a few thousand slots still gets one chunk per step --
// at least 1 (one row: 4 bytes per slot), at most SH_RR_MAX_CHUNKS waves, at
// most one chunk per 64-hit step, and within SH_RR_WS_CAP bytes.
constexpr uint32_t SH_RR_MAX_CHUNKS = 1024;
constexpr uint64_t SH_RR_WS_SMALL = 1ull << 20;
constexpr uint64_t SH_RR_WS_CAP = 256ull << 20;
inline uint32_t sh_rr_chunks(uint64_t hits, uint64_t n_slots) {
  if (!hits || !n_slots) return 1;
  uint64_t c = std::max<uint64_t>(16 * hits, SH_RR_WS_SMALL) / (4 * n_slots);
  c = std::min<uint64_t>(c, SH_RR_MAX_CHUNKS);
  c = std::min<uint64_t>(c, (hits + 63) / 64);
  c = std::min<uint64_t>(c, SH_RR_WS_CAP / (4 * n_slots));
  return uint32_t(std::max<uint64_t>(c, 1));
}

}  // namespace gm

struct emqx_gm_shared {
  int device = 0;
  emqx_gm_index* idx = nullptr;  // the bound snapshot, retained (nullptr: a host-only table)
  void* dev_base = nullptr;      // one allocation holding every array
  size_t bytes = 0;
  gm::HostBytes blob;            // host copy (the state arrays of a device table stay at their built values here)
  gm::ShView hv{}, dv{};
  // for the carry-over by bytes: slot -> its filter's bytes
  std::vector<uint8_t> fbytes;
  std::vector<uint64_t> foff;    // [n_slots + 1]
  emqx_gm_shared_info_t info{};
  std::mutex mu;                 // calls on one table are serialized
  double last_ms[4] = {0, 0, 0, 0};  // enumerate (count + scan + row offsets), expand/pick, round-robin passes, total
};

namespace gm {
// gm_shared.cpp (host only).  resolve(bytes, len, &id): the filter's id in the bound snapshot, false if absent.
struct ShInput {
  const uint8_t* fb;
  const uint64_t* fo;
  const uint32_t* group_ids;
  uint64_t n_slots;
  const uint64_t* mem_off;
  const uint32_t* mem_ids;
};
int sh_compile(const ShInput& in, uint64_t n_filters, const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve,
               const emqx_gm_shared* prev, const uint32_t* prev_rr, const uint32_t* prev_st, emqx_gm_shared** out,
               std::string* why);
int sh_check_rows(const emqx_gm_shared* sh, const emqx_gm_csr* m, std::string* why);
// the single-threaded walk over the host tables and host state (EMQX_GM_EOVERFLOW at 2^32 - 1 hits)
int sh_pick_host(emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy, const uint32_t* msg_hash, uint32_t seed,
                 std::vector<uint64_t>& row_off, std::vector<uint32_t>& members, std::vector<uint32_t>& slots);
// gm_shared.hip (device)
int sh_upload(emqx_gm_ctx* ctx, emqx_gm_shared* sh);
void sh_free_device(emqx_gm_shared* sh);
int sh_read_state(emqx_gm_ctx* ctx, const emqx_gm_shared* sh, std::vector<uint32_t>& rr, std::vector<uint32_t>& st);
// host_out: device rows in, but msg_hash and the result on the host (a publish
// window's rerun); waits (optional): += the host-blocking device waits made
// d_win_row0 (optional, device; a group of publish windows): the windows' first
// rows, n_win ascending entries -- EMQX_GM_SHARE_RANDOM then mixes a message's
// row in its own window, as a call on that window alone does
int sh_pick_device(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const emqx_gm_csr* m, uint32_t strategy,
                   const uint32_t* msg_hash, uint32_t seed, uint32_t n_chunks, emqx_gm_csr* out_members,
                   emqx_gm_csr* out_slots, bool host_out = false, uint32_t* waits = nullptr,
                   const uint32_t* d_win_row0 = nullptr, uint32_t n_win = 0);
// A pick queued over a small call's speculative rows (emqx_gm_publish_window):
// device pointers into one workspace `ws` of the context's pool, which the
// caller releases behind the stream; *total is the true hit count.
struct ShSpec {
  void* ws = nullptr;
  uint64_t* row_off = nullptr;  // [n + 1]
  uint32_t* slots = nullptr;    // [cap_hits]
  uint32_t* members = nullptr;  // [cap_hits]
  const uint64_t* total = nullptr;
  uint32_t* sh_rr = nullptr;    // round robin: the shadow of rr[] (SH_UNSET: untouched)
  uint32_t* sh_st = nullptr;    // sticky: the shadow of st[]
};
int sh_queue_spec(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_hits, uint32_t strategy, const uint32_t* d_hash, uint32_t seed,
                  ShSpec* out, const uint32_t* d_win_row0 = nullptr, uint32_t n_win = 0);
// the shadow state written into the table (queued, no wait; under sh->mu)
int sh_queue_commit(emqx_gm_ctx* ctx, emqx_gm_shared* sh, const ShSpec& run);
}  // namespace gm
