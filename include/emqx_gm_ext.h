/*
 * emqx_gm_ext.h — extensions of libemqx_gpu_match.so that are NOT part of the
 * reference-facing boundary (emqx_gpu_match.h): the seeded synthetic workload
 * of SURVEY.md §8d (generated on the device for the bench), device-buffer
 * helpers for the Python host layer and bench, and roofline accounting.
 */
#ifndef EMQX_GM_EXT_H
#define EMQX_GM_EXT_H

#include "emqx_gpu_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workload generator (spec: DESIGN.md "Workload generator").  codes: n x 5
 * int16 per filter: word index, -1 '+', -2 '#', -3 absent level. */
int emqx_gm_gen_filter_codes(uint64_t seed, uint64_t n, int wildcard_only, int16_t *codes);
/* Render codes to bytes + offsets[n+1]; returns the byte count (pass NULL
 * buffers to size). */
uint64_t emqx_gm_render_codes(const int16_t *codes, uint64_t n, uint8_t *bytes, uint64_t *off);
/* Generate topics [start, start+n) on the device; buffers come from the
 * context pool (free with emqx_gm_dev_free).  The byte buffer is padded. */
int emqx_gm_gen_topics(emqx_gm_ctx *ctx, const int16_t *filter_codes, uint64_t n_filters, uint64_t seed,
                       uint64_t start, uint64_t n, uint8_t **d_bytes, uint64_t **d_off, uint64_t *total_bytes);

/* Device buffers from the context pool. kind: 0 H2D, 1 D2H, 2 D2D. */
int emqx_gm_dev_alloc(emqx_gm_ctx *ctx, uint64_t bytes, void **out);
int emqx_gm_dev_free(emqx_gm_ctx *ctx, void *p);
int emqx_gm_memcpy(emqx_gm_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind);
/* Returns the context's cached device buffers to the runtime, and the device
 * blob kept from the last released index snapshot of 256 MiB or more (reused
 * by the next in-place update of its size; emqx_gm_close frees it too). */
int emqx_gm_pool_trim(emqx_gm_ctx *ctx);

/* Host-only self check of the index compiler (no device needed): compiles the
 * filter set into the flat tables and reports their sizes; perm_out as in
 * emqx_gm_index_build. */
int emqx_gm_index_compile_host(const uint8_t *filter_bytes, const uint64_t *filter_off, uint64_t n_filters,
                               const uint64_t *sub_off, const uint32_t *sub_ids, uint32_t *perm_out,
                               emqx_gm_index_info_t *info);

/* The filters with shard[i] == want, packed (two-call sizing: pass NULL
 * out_bytes/out_off to get *n_out and *bytes_out). */
int emqx_gm_select_filters(const uint8_t *filter_bytes, const uint64_t *filter_off, uint64_t n_filters,
                           const uint32_t *shard, uint32_t want, uint8_t *out_bytes, uint64_t *out_off,
                           uint64_t *n_out, uint64_t *bytes_out);

/* Sum of the byte lengths of the filters referenced by a device CSR (the
 * Σ len(f) term of the algorithmic-bytes formula). */
int emqx_gm_matched_filter_bytes(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const emqx_gm_csr *csr,
                                 uint64_t *out);

/* One part of a fan-out split over n_parts devices ("split
 * rows and split wide rows across GPUs").  The deliveries emqx_gm_fanout would
 * return are numbered 0..T-1 in its order; part p produces the contiguous range
 * [T*p/n_parts, T*(p+1)/n_parts), so every row -- a 1M-subscriber row too -- is
 * cut wherever a range ends and the parts are disjoint and cover all T.  out:
 * row_off = the n_rows+1 GLOBAL delivery offsets (as emqx_gm_fanout's), nnz =
 * the part's length, ids = its deliveries; *first = its first global number.
 * This mirrors the reference's own split of a hot topic's subscribers into
 * shards dispatched independently (emqx_broker_helper.erl:82-91,
 * emqx_broker.erl:526-530). */
int emqx_gm_fanout_part(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const emqx_gm_csr *matches, uint32_t part,
                        uint32_t n_parts, uint32_t flags, emqx_gm_csr *out, uint64_t *first);

/* What the calling thread's last index call (build, import, update,
 * update_subs) did -- observed, not inferred from sizes: the path it took,
 * whether it had to download the snapshot line's host mirror first (a lazy
 * mirror's first update: its bytes and time), and how the replicas of a
 * multi-device context were made. */
#define EMQX_GM_UPD_NONE 0      /* no change (the same snapshot retained)              */
#define EMQX_GM_UPD_PATCH 1     /* in-place patch of a device copy, O(delta)           */
#define EMQX_GM_UPD_OVERLAY 2   /* base + tombstones + delta index                     */
#define EMQX_GM_UPD_REBUILD 3   /* the updated set recompiled                          */
#define EMQX_GM_UPD_SUBS_ONLY 4 /* update_subs without a route change: tables shared   */
#define EMQX_GM_UPD_BUILD 5
#define EMQX_GM_UPD_IMPORT 6
#define EMQX_GM_UPD_SHIFT 7     /* a shard of a sharded update: ids only, tables shared */
#define EMQX_GM_REP_NONE 0      /* no replicas (single device, or left on the first)   */
#define EMQX_GM_REP_PATCHED 1   /* every member applied the same delta to its replica  */
#define EMQX_GM_REP_COPIED 2    /* device tables copied device to device (tree order)  */
#define EMQX_GM_REP_SHARED 3    /* members share their replica's tables + own new CSR  */
#define EMQX_GM_REP_SHARDED 4  /* a sharded index: every shard applied its share (replicas = shards - 1) */
typedef struct {
  uint32_t kind;          /* EMQX_GM_UPD_*                                        */
  uint32_t replica_mode;  /* EMQX_GM_REP_*                                        */
  uint32_t replicas;      /* member replicas made                                 */
  int32_t mirror_loaded;  /* 1: the host mirror was loaded by this call           */
  uint64_t mirror_bytes;  /* ... its bytes                                        */
  double mirror_ms;       /* ... its time                                         */
  double device_ms;       /* the device part (every device at once), wall         */
  double replicate_ms;    /* replica copies after the first device's result, wall */
  double total_ms;        /* the whole call, wall                                 */
  uint32_t blobs_reused;  /* device tables placed in a released snapshot's blob   */
  uint32_t blobs_fresh;   /* ... in a fresh allocation (every device counted)     */
} emqx_gm_update_stats;
int emqx_gm_last_update_stats(const emqx_gm_ctx *ctx, emqx_gm_update_stats *stats);
/* What each shard of the calling thread's last emqx_gm_index_update on a
 * sharded index did: EMQX_GM_UPD_PATCH (patched in place), EMQX_GM_UPD_SHIFT
 * (no local change: the previous tables shared, a new id map only) or
 * EMQX_GM_UPD_REBUILD (this shard recompiled alone).  The stats of such an
 * update: kind PATCH when no shard was recompiled, REBUILD when any was, NONE
 * for no change; replica_mode EMQX_GM_REP_SHARDED, replicas = shards - 1.
 * In: *n = the entries `kinds` holds (kinds may be NULL); out: *n = the
 * shards (0: the thread has made no sharded update, or its last one changed
 * nothing). */
int emqx_gm_last_shard_update(const emqx_gm_ctx *ctx, uint32_t *kinds, uint32_t *n);
/* shard_out[i] = the shard a filter goes to under a FIXED route (what a
 * sharded update does with a new filter; no re-plan, no newly split word):
 * EMQX_GM_ALL_SHARDS for a first word '+' / '#', and under a split (hot)
 * first word for the word alone or a '+' / '#' second word; else the shard
 * emqx_gm_route_topics_host gives the filter's own bytes read as a topic.
 * For every filter the plan was made from this is the plan's shard_out; for
 * any other it is the shard every topic able to match the filter is routed
 * to.  Host buffers. */
int emqx_gm_route_filter_shards_host(const emqx_gm_route *route, const uint8_t *filter_bytes,
                                     const uint64_t *filter_off, uint64_t n_filters, uint32_t *shard_out);

/* Test support: FNV-1a digests of replica k's device tables (k = 0: the
 * snapshot itself, k >= 1: its replica on the context's k-th member) and of
 * its subscriber CSR (offsets + ids; 0 without one).  Replicas of one snapshot
 * hold byte-identical tables. */
int emqx_gm_index_replica_digest(emqx_gm_ctx *ctx, const emqx_gm_index *idx, uint32_t k, uint64_t *tables,
                                 uint64_t *subs);

/* Test and measurement support for the retained-topic index (no product path
 * uses these).  compile_host: the index compiled on the host alone (no device,
 * no context); emqx_gm_retained_match and _expire refuse it.  match_host: the
 * walk of emqx_gm_retained_match over the host copy of the tables, single
 * threaded, no device call; the CSR is malloc'd (free with
 * emqx_gm_retained_csr_free_host).  last_times: device ms of the count pass,
 * the scan and the fill pass of the index's last EMQX_GM_RET_TIMED match. */
int emqx_gm_retained_compile_host(const uint8_t *topic_bytes, const uint64_t *topic_off, uint64_t n_topics,
                                  const uint32_t *ids, const uint64_t *expiry_ms, emqx_gm_retained **out);
int emqx_gm_retained_match_host(const emqx_gm_retained *idx, const uint8_t *filter_bytes,
                                const uint64_t *filter_off, uint64_t n_filters, uint64_t now_ms, emqx_gm_csr *out);
int emqx_gm_retained_csr_free_host(emqx_gm_csr *csr);
int emqx_gm_retained_last_times(const emqx_gm_retained *idx, double *ms3);

/* Test and measurement support for the shared-subscription table (no product
 * path uses these).  compile_host: the table compiled on the host alone against
 * the filter set index_filter_* as emqx_gm_index_compile_host compiles it (ids
 * = ranks among the distinct filters; no device, no context); prev must be a
 * host-only table too; emqx_gm_shared_pick refuses the result.  pick_host: the
 * single-threaded walk of emqx_gm_shared_pick over the same tables and the
 * host-only table's own state (host rows; refused on a device table, whose
 * state lives on the device); the CSRs are malloc'd (free with
 * emqx_gm_shared_csr_free_host).  pick_chunked: emqx_gm_shared_pick with the
 * round-robin chunk count forced (0: the library's rule, at most 1024).
 * last_times: device ms of the last pick's enumerate, expand and round-robin
 * passes, and of the whole call on the stream. */
int emqx_gm_shared_compile_host(const uint8_t *index_filter_bytes, const uint64_t *index_filter_off,
                                uint64_t n_index_filters, const uint8_t *filter_bytes, const uint64_t *filter_off,
                                const uint32_t *group_ids, uint64_t n_slots, const uint64_t *mem_off,
                                const uint32_t *mem_ids, const emqx_gm_shared *prev, emqx_gm_shared **out);
int emqx_gm_shared_pick_host(emqx_gm_shared *sh, const emqx_gm_csr *matches, uint32_t strategy,
                             const uint32_t *msg_hash, uint32_t seed, emqx_gm_csr *out_members,
                             emqx_gm_csr *out_slots);
int emqx_gm_shared_csr_free_host(emqx_gm_csr *csr);
int emqx_gm_shared_pick_chunked(emqx_gm_ctx *ctx, emqx_gm_shared *sh, const emqx_gm_csr *matches,
                                uint32_t strategy, const uint32_t *msg_hash, uint32_t seed, uint32_t n_chunks,
                                emqx_gm_csr *out_members, emqx_gm_csr *out_slots);
int emqx_gm_shared_last_times(const emqx_gm_shared *sh, double *ms4);

/* Test and measurement support for the route-destination table (no product
 * path uses these).  compile_host: the table compiled on the host alone against
 * the filter set index_filter_* as emqx_gm_index_compile_host compiles it (ids
 * = ranks among the distinct filters; no device, no context);
 * emqx_gm_forward_plan refuses the result.  plan_host: the single-threaded walk
 * of emqx_gm_forward_plan over the table's host copy (host rows; any table);
 * the arrays are malloc'd (free with emqx_gm_forwards_free, or, in a build
 * without the device half, emqx_gm_forwards_free_host).  plan_chunked:
 * emqx_gm_forward_plan with the partition's chunk count forced (0: the
 * library's rule, at most 1024).  last_times: device ms of the last plan's
 * enumerate, expand and partition passes, and of the whole call on the stream. */
int emqx_gm_dests_compile_host(const uint8_t *index_filter_bytes, const uint64_t *index_filter_off,
                               uint64_t n_index_filters, const uint8_t *filter_bytes, const uint64_t *filter_off,
                               const uint32_t *node_ids, uint64_t n_routes, uint32_t n_nodes, uint32_t flags,
                               emqx_gm_dests **out);
int emqx_gm_forward_plan_host(const emqx_gm_dests *dt, const emqx_gm_csr *matches, uint32_t skip_node,
                              emqx_gm_forwards *out);
int emqx_gm_forwards_free_host(emqx_gm_forwards *fw);
int emqx_gm_forward_plan_chunked(emqx_gm_ctx *ctx, emqx_gm_dests *dt, const emqx_gm_csr *matches,
                                 uint32_t skip_node, uint32_t n_chunks, emqx_gm_forwards *out);
int emqx_gm_dests_last_times(const emqx_gm_dests *dt, double *ms4);

/* Test and measurement support for the subscription-option table (no product
 * path uses these).  compile_host: the table compiled on the host alone against
 * the filter set index_filter_* with the subscriber lists sub_off / sub_ids as
 * emqx_gm_index_compile_host takes them (ids = ranks among the distinct
 * filters, the lists of a filter given twice concatenated in input order; no
 * device, no context); emqx_gm_deliver refuses the result.  deliver_host: the
 * plain single-threaded walk of emqx_gm_deliver over the table's host copy
 * (host rows; any table): the walk a caller would otherwise run per delivery,
 * and the A/B baseline.  Its arrays are malloc'd (free with
 * emqx_gm_deliveries_free, or, in a build without the device half,
 * emqx_gm_deliveries_free_host).  last_times: device ms of the last
 * emqx_gm_deliver's lengths + scan, its copy kernel, and the whole call on the
 * stream. */
int emqx_gm_subopts_compile_host(const uint8_t *index_filter_bytes, const uint64_t *index_filter_off,
                                 uint64_t n_index_filters, const uint64_t *sub_off, const uint32_t *sub_ids,
                                 const uint8_t *filter_bytes, const uint64_t *filter_off, const uint32_t *entry_subs,
                                 const uint8_t *opts, uint64_t n_entries, uint8_t default_opt, uint32_t flags,
                                 emqx_gm_subopts **out);
int emqx_gm_deliver_host(const emqx_gm_subopts *so, const emqx_gm_csr *matches, const uint8_t *msg_flags,
                         const uint32_t *msg_from, uint32_t mode, emqx_gm_deliveries *out);
int emqx_gm_deliveries_free_host(emqx_gm_deliveries *d);
int emqx_gm_subopts_last_times(const emqx_gm_subopts *so, double *ms3);
/* Session batches (emqx_gm_deliver_batches).  batches_host: the plain
 * single-threaded walk over the table's host copy (host rows; any table; no
 * device): dispatch in window order into per-subscriber lists, then the
 * mode's removal.  Its arrays are malloc'd (free with emqx_gm_batches_free and
 * a NULL ctx, or, in a build without the device half,
 * emqx_gm_batches_free_host).  batches_chunked: the device call with the radix
 * partition's chunk count forced (0: the library's rule; clamped to one chunk
 * per 256 deliveries; more than 1024: EMQX_GM_EINVAL).  batches_last_times:
 * device ms of the last call's count, expand, partition (all passes) and
 * heads + removal + emit steps, the whole call on the stream, the number of
 * radix passes (all six of the last call that had deliveries), and ms7[6]: the
 * host-blocking waits the last call made. */
int emqx_gm_deliver_batches_host(const emqx_gm_subopts *so, const emqx_gm_csr *matches, const uint8_t *msg_flags,
                                 const uint32_t *msg_from, uint32_t mode, emqx_gm_batches *out);
int emqx_gm_batches_free_host(emqx_gm_batches *b);
int emqx_gm_deliver_batches_chunked(emqx_gm_ctx *ctx, emqx_gm_subopts *so, const emqx_gm_csr *matches,
                                    const uint8_t *msg_flags, const uint32_t *msg_from, uint32_t mode,
                                    uint32_t n_chunks, emqx_gm_batches *out);
int emqx_gm_batches_last_times(const emqx_gm_subopts *so, double *ms7);

/* Test and measurement support for the authorization table (no product path
 * uses these).  compile_host: the table compiled on the host alone (no device,
 * no context); emqx_gm_authz_check refuses it.  check_host: the walk of
 * emqx_gm_authz_check over the host copy of the tables, single threaded, no
 * device call.  last_kernel_ms: device ms of k_authz_check in the table's last
 * EMQX_GM_AUTHZ_TIMED check (summed over a large window's chunks). */
int emqx_gm_authz_compile_host(const emqx_gm_authz_desc *desc, emqx_gm_authz **out);
int emqx_gm_authz_check_host(const emqx_gm_authz *tab, const emqx_gm_authz_batch *batch, uint8_t *verdict,
                             uint32_t *rule);
int emqx_gm_authz_last_kernel_ms(const emqx_gm_authz *tab, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* EMQX_GM_EXT_H */
