// gm_dests.h — the route-destination table: layout and rules shared by the
// host compiler and host walk (gm_dests.cpp) and the gfx950 kernels
// (gm_dests.hip).
//
// It is the node part of the emqx_route bag (apps/emqx/src/emqx_router.erl:
// do_add_route/2, :112-116; lookup_routes/1, :136) for the filters of one
// snapshot: a set of (filter, node) pairs, node a caller-assigned dense id
// below n_nodes <= EMQX_GM_DESTS_MAX_NODES.  A forward plan turns a publish
// window's matched rows into one (row, filter) list per node, the work of
// route(aggre(match_routes(Topic))) -> forward/3 (apps/emqx/src/
// emqx_broker.erl:214, 245-293) for every message of the window.
//
// One allocation, in this order:
//   d_off [n_filters + 1] u32  filter id -> its nodes [d_off[f], d_off[f + 1])
//   nodes [n_routes]      u16  node ids, ascending within a filter, each once
// (n_nodes <= 4096, so a node id fits 16 bits: half the bytes of the list the
// expand kernel streams.)
//
// HIT: (window row, matched filter id, node of that filter) with node !=
// skip_node.  BATCH ORDER: rows ascending, filter ids in the order the row
// holds them, nodes ascending.  The plan lists each node's hits in batch order.
#pragma once

#include <mutex>

#include "gm_internal.h"

namespace gm {

struct DtView {
  const uint32_t* d_off;
  const uint16_t* nodes;
  uint32_t n_filters, n_routes, n_nodes;
};

// The partition's chunk rule, after sh_rr_chunks: the flat hit
// array is cut into C chunks of L = ceil(hits / C) consecutive hits and the
// workspace is C rows of n_nodes u32.  C is the largest count whose workspace
// stays within max(16 bytes per hit, FW_WS_SMALL) -- proportional to the hits
// -- at least 1, at most FW_MAX_CHUNKS blocks, and at most one chunk per
// FW_BLOCK-hit step.  With n_nodes <= 4096 the workspace never passes 16 MiB.
constexpr uint32_t FW_BLOCK = 256;
constexpr uint32_t FW_MAX_CHUNKS = 1024;
constexpr uint64_t FW_WS_SMALL = 1ull << 20;
inline uint32_t fw_chunks(uint64_t hits, uint64_t n_nodes) {
  if (!hits || !n_nodes) return 1;
  uint64_t c = std::max<uint64_t>(16 * hits, FW_WS_SMALL) / (4 * n_nodes);
  c = std::min<uint64_t>(c, FW_MAX_CHUNKS);
  c = std::min<uint64_t>(c, (hits + FW_BLOCK - 1) / FW_BLOCK);
  return uint32_t(std::max<uint64_t>(c, 1));
}

// a result held in malloc'ed arrays (the host walk): its release
inline int fw_free_malloc(emqx_gm_forwards* fw) {
  if (!fw) return EMQX_GM_EINVAL;
  free(fw->node_off);
  free(fw->rows);
  free(fw->filters);
  free(fw->row_routes);
  std::memset(fw, 0, sizeof(*fw));
  return EMQX_GM_OK;
}

}  // namespace gm

struct emqx_gm_dests {
  int device = 0;
  emqx_gm_index* idx = nullptr;  // the bound snapshot, retained (nullptr: a host-only table)
  void* dev_base = nullptr;      // one allocation holding both arrays
  size_t bytes = 0;
  gm::HostBytes blob;            // host copy: _info and the host walk
  gm::DtView hv{}, dv{};
  emqx_gm_dests_info_t info{};
  std::mutex mu;                 // guards last_ms
  double last_ms[4] = {0, 0, 0, 0};  // enumerate (row routes + count + scan), expand, partition, total
};

namespace gm {
// gm_dests.cpp (host only).  resolve(bytes, len, &id): the filter's id in the bound snapshot, false if absent.
struct DtInput {
  const uint8_t* fb;
  const uint64_t* fo;
  const uint32_t* node_ids;
  uint64_t n_routes;
  uint32_t n_nodes, flags;
};
int dt_compile(const DtInput& in, uint64_t n_filters,
               const std::function<bool(const uint8_t*, uint64_t, uint32_t*)>& resolve, emqx_gm_dests** out,
               std::string* why);
int dt_check_rows(const emqx_gm_dests* dt, const emqx_gm_csr* m, std::string* why);
// the single-threaded walk over the host tables into malloc'ed arrays (EMQX_GM_EOVERFLOW at 2^32 - 1 hits)
int dt_plan_host(const emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node, emqx_gm_forwards* out);
// gm_dests.hip (device)
int dt_upload(emqx_gm_ctx* ctx, emqx_gm_dests* dt);
void dt_free_device(emqx_gm_dests* dt);
// host_out: device rows in, the result on the host (a publish window's
// rerun); waits (optional): += the host-blocking device waits made
int dt_plan_device(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const emqx_gm_csr* m, uint32_t skip_node, uint32_t n_chunks,
                   emqx_gm_forwards* out, bool host_out = false, uint32_t* waits = nullptr);
// A plan queued over a small call's speculative rows (emqx_gm_publish_window):
// device pointers into one workspace `ws` of the context's pool, which the
// caller releases behind the stream; *total is the true pair count.
struct DtSpec {
  void* ws = nullptr;
  uint32_t* row_routes = nullptr;  // [n]
  uint64_t* node_off = nullptr;    // [n_nodes + 1]
  uint32_t* rows = nullptr;        // [cap_pairs]
  uint32_t* filters = nullptr;     // [cap_pairs]
  const uint64_t* total = nullptr;
};
int dt_queue_spec(emqx_gm_ctx* ctx, emqx_gm_dests* dt, const uint64_t* d_ro, const uint32_t* d_ids, uint64_t n,
                  uint64_t cap, uint64_t cap_pairs, uint32_t skip_node, DtSpec* out);
}  // namespace gm
