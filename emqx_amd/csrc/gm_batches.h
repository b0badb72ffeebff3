// gm_batches.h — session batches: a window's deliveries grouped by subscriber
// (rules shared by the host walk, gm_batches.cpp, and the gfx950 kernels,
// gm_batches.hip; the option table and the byte rules: gm_subopts.h).
//
// It is the transpose the reference makes with mailboxes: a connection process
// drains every {deliver, Filter, Msg} into one list (apps/emqx/src/
// emqx_connection.erl:516-520, emqx_misc:drain_deliver/1, emqx_misc.erl:159-173)
// and hands it to emqx_channel:handle_deliver/2 (emqx_channel.erl:830-842),
// which runs emqx_session:ignore_local/4 -- a lists:dropwhile, emqx_session.erl:
// 279-291 -- and enriches what remains.
//
// Delivery k = 0, 1, ... is the k-th delivery emqx_gm_deliver emits in FLAG
// mode; a subscriber's batch is its deliveries in ascending k; batches are
// listed by ascending subscriber id.  Removal per mode: FLAG none, DROP every
// No-Local hit, LEAD the leading run of hits of each batch (bit 4 cleared in
// what is kept).
//
// Device: expand (key = subscriber, payload row / filter / byte per k), a
// stable LSD radix partition of (key, k) over 8-bit digits -- per pass
// hist / column / scan / scatter over C chunks, as gm_dests.hip's partition
// with 256 bins -- then heads, the removal scans and the gather.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gm_subopts.h"

namespace gm {

// The partition's chunk rule, after fw_chunks (gm_dests.h) with 256 bins: the
// flat pair array is cut into C chunks of L = ceil(n / C) consecutive pairs and
// a pass's workspace is C rows of 256 u32.  C is the largest count whose
// workspace stays within max(16 bytes per delivery, SB_WS_SMALL), at least 1,
// at most SB_MAX_CHUNKS blocks, and at most one chunk per SB_BLOCK-pair step.
constexpr uint32_t SB_BLOCK = 256, SB_BINS = 256;
constexpr uint32_t SB_MAX_CHUNKS = 1024;
constexpr uint64_t SB_WS_SMALL = 1ull << 20;
inline uint32_t sb_chunks(uint64_t n) {
  if (!n) return 1;
  uint64_t c = std::max<uint64_t>(16 * n, SB_WS_SMALL) / (4 * SB_BINS);
  c = std::min<uint64_t>(c, SB_MAX_CHUNKS);
  c = std::min<uint64_t>(c, (n + SB_BLOCK - 1) / SB_BLOCK);
  return uint32_t(std::max<uint64_t>(c, 1));
}
// the 8-bit digits of the table's largest subscriber id, at least 1
inline uint32_t sb_passes(uint32_t max_sub) {
  uint32_t p = 1;
  while (p < 4 && (max_sub >> (8 * p))) ++p;
  return p;
}

// a result held in malloc'ed arrays (the host walk): its release
inline int sb_free_malloc(emqx_gm_batches* b) {
  if (!b) return EMQX_GM_EINVAL;
  free(b->subs);
  free(b->batch_off);
  free(b->rows);
  free(b->filters);
  free(b->dopt);
  free(b->batch_dropped);
  std::memset(b, 0, sizeof(*b));
  return EMQX_GM_OK;
}

// gm_batches.cpp (host only)
int sb_batches_host(const emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                    const uint32_t* msg_from, uint32_t mode, emqx_gm_batches* out);
// gm_batches.hip (device).  n_chunks: 0 for the library's rule.  The host-blocking waits a call makes are
// counted into the table's sb_ms[6] (emqx_gm_batches_last_times).
int sb_batches_device(emqx_gm_ctx* ctx, emqx_gm_subopts* so, const emqx_gm_csr* m, const uint8_t* msg_flags,
                      const uint32_t* msg_from, uint32_t mode, uint32_t n_chunks, emqx_gm_batches* out);
}  // namespace gm
