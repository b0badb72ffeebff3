// gm_subopts.h — the subscription-option table: layout and rules shared by the
// host compiler and host walk (gm_subopts.cpp) and the gfx950 kernels
// (gm_subopts.hip).
//
// It is the options half of emqx_broker:subscribe/3 (apps/emqx/src/
// emqx_broker.erl:126-145: the ?SUBOPTION table keyed {SubPid, Topic}) for the
// (filter, subscriber) pairs of one snapshot, and a deliver call does, for every
// delivery of a publish window, the work of emqx_session:ignore_local/4 and
// enrich_deliver/2 (apps/emqx/src/emqx_session.erl:279-291, 560-602).
//
// The table is bound to ONE plain snapshot built with subscriber lists and is
// immutable: following emqx_gm_index_update_subs incrementally is out of scope
// (a new snapshot or a changed option means a new build).  rh is not carried
// (it belongs to the subscribe-time retained dispatch), nor is subid (the
// Subscription-Identifier stays with the session).
//
// Device allocation, in this order:
//   opt    [n_subs]        u8   entry for entry with the snapshot's sub_ids
//   nl_off [n_filters + 1] u64  filter id -> its No-Local pairs [nl_off[f], nl_off[f + 1])
//   nl_sub [n_nl]          u32  their subscriber ids, ascending within a filter, each once
//   nl_pos [n_nl]          u32  the pair's position in the filter's segment of sub_ids
// The subscriber lists themselves (sub_off, sub_ids) are the bound snapshot's
// own on the device; the host blob keeps a copy behind the arrays above (not
// uploaded) so that the host walk runs over any table.
//
// OPT byte: bits 0-1 SubQoS, 2 nl, 3 rap, 4 the session's upgrade_qos.
// MSG byte: bits 0-1 PubQoS, 2 retain, 3 headers.retained.
// DELIVERY byte: bits 0-1 QoS, 2 retain, 3 the nl flag, 4 the No-Local hit (FLAG mode).
#pragma once

#include <mutex>

#include "gm_internal.h"

namespace gm {

constexpr uint32_t SO_NONE = 0xFFFFFFFFu;
constexpr uint8_t SO_NL = 0x04, SO_RAP = 0x08, SO_UPG = 0x10;
constexpr uint8_t SO_HIT = 0x10;

// enrich_subopts/3 over [{nl, _}, {qos, _}, {rap, _}] (emqx_session.erl:582-598)
GM_HD uint8_t so_byte(uint8_t opt, uint8_t msg) {
  const uint32_t sq = opt & 3u, pq = msg & 3u;
  const uint32_t q = (opt & SO_UPG) ? (sq > pq ? sq : pq) : (sq < pq ? sq : pq);
  // {rap, 1}: kept; {rap, 0} with headers.retained: kept; {rap, 0}: cleared
  const uint32_t keep = ((opt & SO_RAP) | (msg & 0x08u)) ? 1u : 0u;
  const uint32_t retain = keep & ((msg >> 2) & 1u);
  const uint32_t nl = (opt >> 2) & 1u;
  return uint8_t(q | (retain << 2) | (nl << 3));
}

// so_byte of four option bytes at once (byte k of `opts` -> byte k of the result), for one
// message: every field is at most 2 bits wide inside its byte, so the
// per-byte compare runs under a guard bit and nothing crosses a byte.
GM_HD uint32_t so_byte4(uint32_t opts, uint8_t msg) {
  constexpr uint32_t ONES = 0x01010101u;
  const uint32_t sq = opts & (3u * ONES), pq = (msg & 3u) * ONES;
  const uint32_t ge = (((sq | (4u * ONES)) - pq) >> 2) & ONES;  // SubQoS >= PubQoS, per byte
  const uint32_t gm = ge * 0xFFu;
  const uint32_t lo = (pq & gm) | (sq & ~gm), hi = (sq & gm) | (pq & ~gm);
  const uint32_t um = ((opts >> 4) & ONES) * 0xFFu;  // upgrade_qos: max, else min
  const uint32_t q = (hi & um) | (lo & ~um);
  const uint32_t keep = ((opts >> 3) & ONES) | (((msg >> 3) & 1u) * ONES);
  const uint32_t retain = keep & (((msg >> 2) & 1u) * ONES);
  const uint32_t nl = (opts >> 2) & ONES;
  return q | (retain << 2) | (nl << 3);
}

struct SoView {
  const uint64_t* sub_off;
  const uint32_t* sub_ids;
  const uint8_t* opt;
  const uint64_t* nl_off;
  const uint32_t* nl_sub;
  const uint32_t* nl_pos;
  uint64_t n_subs, n_nl;
  uint32_t n_filters;
};

// a result held in malloc'ed arrays (the host walk): its release
inline int so_free_malloc(emqx_gm_deliveries* d) {
  if (!d) return EMQX_GM_EINVAL;
  free(d->deliveries.row_off);
  free(d->deliveries.ids);
  free(d->dopt);
  free(d->row_dropped);
  std::memset(d, 0, sizeof(*d));
  return EMQX_GM_OK;
}

}  // namespace gm

struct emqx_gm_subopts {
  int device = 0;
  emqx_gm_index* idx = nullptr;  // the bound snapshot, retained (nullptr: a host-only table)
  void* dev_base = nullptr;      // one allocation holding opt and the nl arrays
  size_t bytes = 0;              // ... its bytes (the head of blob)
  gm::HostBytes blob;            // host copy: the device arrays, then sub_off and sub_ids
  gm::SoView hv{}, dv{};
  uint32_t max_sub = 0;          // the lists' largest subscriber id (gm_batches.hip: its 8-bit digits are the radix passes)
  emqx_gm_subopts_info_t info{};
  std::mutex mu;                 // guards last_ms
  double last_ms[3] = {0, 0, 0};  // lengths + scan + row offsets, copy, total
  // a batches call: count, expand, partition, heads..emit, total (ms; of the last call that had deliveries); its
  // passes; the host-blocking waits of the last call
  double sb_ms[7] = {0, 0, 0, 0, 0, 0, 0};
};

namespace gm {
// gm_subopts.cpp (host only).  resolve(bytes, len, &id): the filter's id in the bound snapshot, false if absent.
struct SoInput {
  const uint8_t* fb;
  const uint64_t* fo;
  const uint32_t* subs;
  const uint8_t* opts;
  uint64_t n_entries;
  uint8_t default_opt;
  uint32_t flags;
};
// sub_off [n_filters + 1] / sub_ids: the snapshot's lists on the host (copied into the table)
int so_compile(const SoInput& in, uint64_t n_filters, const uint64_t* sub_off, const uint32_t* sub_ids,
               const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve, emqx_gm_subopts** out,
               std::string* why);
// every check of a deliver call's inputs that needs no device
// lead_ok: EMQX_GM_SO_LEAD is a mode of this call (emqx_gm_deliver_batches alone)
int so_check_call(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags, const uint32_t* msg_from,
                  uint32_t mode, std::string* why, bool lead_ok = false);
int so_deliver_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                    const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out);
// gm_subopts.hip (device)
int so_upload(emqx_gm_ctx* ctx, emqx_gm_subopts* so);
void so_free_device(emqx_gm_subopts* so);
// host_out: device rows in, but the messages and the result on the host (a
// publish window's rerun); d_flags_up / d_from_up (optional, with host_out): the
// messages already on the device; waits (optional): += the host-blocking
// device waits made
int so_deliver_device(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                      const uint32_t* msg_from, uint32_t mode, emqx_gm_deliveries* out, bool host_out = false,
                      uint32_t* waits = nullptr, const uint8_t* d_flags_up = nullptr,
                      const uint32_t* d_from_up = nullptr);
// a bad message byte (so_check_call's rule)
inline bool so_bad_msg(uint8_t b) { return (b & 3u) == 3u || (b & 0xF0u); }
// the A/B knob of a publish window's speculative deliveries capacity (as given; "0": not speculated)
inline const char* so_cap_knob() { return knob("GM_PW_CAP_DELIVERIES"); }
// A window's messages as one page-locked block: [publishers n x u32 | flags n x u8], each part 16-B aligned
inline size_t so_msgs_bytes(uint64_t n) { return al16(al16(n * 4) + n); }
// Deliveries queued over a small call's speculative rows
// (emqx_gm_publish_window_deliver): device pointers into one workspace `ws` of
// the context's pool, which the caller releases behind the stream; *total is
// the true (post-drop) delivery count, *dropped the true dropped count.
struct SoSpec {
  void* ws = nullptr;
  uint64_t* row_off = nullptr;      // [n + 1]
  uint32_t* ids = nullptr;          // [cap_d] + 16 B
  uint8_t* dopt = nullptr;          // [cap_d] + 16 B
  uint32_t* row_dropped = nullptr;  // [n], EMQX_GM_SO_DROP
  const uint64_t* total = nullptr;
  const uint64_t* dropped = nullptr;  // EMQX_GM_SO_DROP
  const uint8_t* d_flags = nullptr;   // the uploaded messages (a rerun reads them)
  const uint32_t* d_from = nullptr;
};
int so_queue_spec(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_d, uint32_t mode, const void* msgs, SoSpec* out);
// k_so_seglen over nnz entries in FLAG form (the lengths, the hits) on stream st: gm_batches.hip counts a
// window's deliveries with the same kernel
int so_launch_seglen(hipStream_t st, const SoView& dv, const uint64_t* d_mro, uint64_t n_rows, const uint32_t* d_mids,
                     uint64_t nnz, const uint32_t* d_from, uint64_t* seg_len, uint32_t* seg_hit);
int so_queue_pack(emqx_gm_ctx* ctx, const SoSpec& run, uint64_t n, uint64_t cap_d, uint64_t* o_ro, uint32_t* o_ids,
                  uint8_t* o_opt, uint32_t* o_rd, uint64_t* o_meta);
}  // namespace gm
