// gm_publish.h — emqx_gm_publish_window's stage (gm_publish.hip), called by the
// entry point (gm_api.cpp) once every argument is checked.
#pragma once

#include "gm_internal.h"

namespace gm {

struct PwArgs {
  emqx_gm_shared* sh = nullptr;  // nullptr: no picks
  uint32_t strategy = 0, seed = 0;
  const uint32_t* msg_hash = nullptr;  // host, one per topic (EMQX_GM_SHARE_HASH)
  emqx_gm_dests* dt = nullptr;   // nullptr: no plan
  uint32_t skip_node = 0;
  // emqx_gm_publish_window_deliver (nullptr: the plain fan-out)
  emqx_gm_subopts* so = nullptr;
  const uint8_t* msg_flags = nullptr;  // host, one per topic
  const uint32_t* msg_from = nullptr;  // host, one per topic
  uint32_t so_mode = 0;
};

// what a window with a.so returns beside res: the deliveries with their bytes (host pool arrays)
struct PwDeliv {
  emqx_gm_deliveries out{};
  bool spec = false;  // they came from the first round trip
  uint64_t cap = 0;   // the speculative capacity used (0: not speculated)
};

// A window run_host_small serves, whole on ctx's device (entered WITHOUT
// ctx->mu): the match, its fan-out (fan, as run_host_small's), the picks and the
// plan in one device round trip where the speculation holds.  res->deliveries
// is left to the caller (fan->ok: fan->out).  With a.so the deliveries with
// their option bytes run as a third part in place of the fan-out (fan is not
// used) and come back in dl.  On an error nothing is held and the shared
// table's state is unchanged.
int run_publish_window(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                       uint32_t flags, const PwArgs& a, emqx_gm_publish_result* res, emqx_gm_publish_stats* st_out,
                       emqx_gm_match_stats* mst, SmallFan* fan, PwDeliv* dl = nullptr);

// A GROUP of such windows as one device batch (emqx_gm_publish_windows; entered
// WITHOUT ctx->mu; the caller has checked what run_host_windows asks for): one
// match, one fan-out, one pick stage and one plan stage over the group's rows
// (a.msg_hash is not read: the windows bring their own), each result cut into
// the windows' own.  res[k].deliveries is set where fan_ok[k] (else the caller
// fans that window's rows out); st_out[k] / gst[k] are window k's figures (the
// caller sets gst[k].seq).  On an error nothing is held and the shared table's
// state is unchanged.
int run_publish_windows(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win* w, uint32_t g,
                        uint32_t flags, const PwArgs& a, emqx_gm_publish_result* res, emqx_gm_publish_stats* st_out,
                        emqx_gm_publish_group_stats* gst, uint8_t* fan_ok, emqx_gm_match_stats* mst);

}  // namespace gm
