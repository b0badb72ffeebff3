/*
 * emqx_gpu_match.h — C ABI of libemqx_gpu_match.so, the MI355X batch
 * topic-matching engine for EMQX's publish routing hot path.
 *
 * This is the drop-in boundary that a thin Erlang NIF (`emqx_gpu_match`,
 * nif/emqx_gpu_match_nif.c) binds.  Each entry point replaces one reference
 * interface (paths relative to the reference repo root):
 *
 *   emqx_gm_index_build   <- the emqx_trie / emqx_route tables as maintained by
 *                            emqx_router:do_add_route/2 + emqx_trie:insert/1
 *                            (apps/emqx/src/emqx_router.erl:112-125,
 *                             apps/emqx/src/emqx_trie.erl:107-119) and the
 *                            emqx_subscriber bag written by
 *                            emqx_broker:do_subscribe/4 (emqx_broker.erl:147-165)
 *   emqx_gm_index_info    <- emqx_trie:empty/0 (emqx_trie.erl:165-170)
 *   emqx_gm_match         <- emqx_trie:match/1 (emqx_trie.erl:139-161) with
 *                            flags = 0, or emqx_router:match_routes/1
 *                            (emqx_router.erl:128-145) with
 *                            EMQX_GM_WITH_EXACT; batched over many topics
 *   emqx_gm_fanout        <- emqx_broker:dispatch/2 + do_dispatch/2,3 +
 *                            subscribers/1 (emqx_broker.erl:296-322, 506-530)
 *   emqx_gm_match_fanout  <- emqx_broker:publish/1's route/2 + dispatch/2 of a
 *                            batch (emqx_broker.erl:204-215, 245-322)
 *
 * Result semantics (bit-exact with the reference, compared as sets):
 *   - filter ids are the lexicographic rank of the filter bytes (Erlang binary
 *     order = unsigned bytewise, prefix first), so each result row, sorted
 *     ascending by id, is `lists:sort/1` of the reference's result list;
 *   - flags = 0: row = emqx_trie:match(Topic) over the indexed filters that the
 *     trie holds (wildcard filters; a single-word '$X' topic also returns a
 *     non-wildcard '$X' filter, emqx_trie.erl:271-278); a wildcard topic gives
 *     an empty row (emqx_trie.erl:149-158);
 *   - EMQX_GM_WITH_EXACT: row = the distinct filters whose routes
 *     match_routes(Topic) returns: the literal filter == Topic (also for a
 *     wildcard Topic) plus the trie matches;
 *   - fan-out rows are multisets: a subscriber of two matching filters is
 *     delivered twice (emqx_persistent_session_SUITE.erl:705).
 *
 * Ownership: input buffers are borrowed for the duration of a call.  Result
 * CSR buffers belong to the library until emqx_gm_csr_free().  Indexes are
 * immutable and reference counted (RCU-style snapshot swap by the caller).
 * Threading: a context may be used from several threads; calls on one context
 * are serialised onto its HIP stream.  Errors: every call returns 0 or a
 * negative EMQX_GM_E* code; nothing aborts the process; the message is in
 * emqx_gm_last_error(), which is kept per calling thread (a failing call's
 * message cannot be replaced by a concurrent call on another thread).
 *
 * Device topic buffers (EMQX_GM_DEVICE_IO): the tokenizer reads whole aligned
 * 8-byte words, so at least 64 readable bytes must follow topic_bytes[toff[n]]
 * (the library pads its own copies of host buffers the same way).
 *
 * Environment: the default library reads ONE variable, EMQX_GM_AB.  Unless it
 * is set (non-empty, not "0"), every GM_* knob below is ignored, so a library
 * loaded into a BEAM runs one table layout and one walk whatever else the
 * host's environment holds.  With EMQX_GM_AB set (A/B scripts, the test
 * suite) the library reads, per call:
 *   layout (at build):  GM_HOT_LOAD_PCT, GM_HOT_LOAD_PCT_UPPER, GM_HOT_FLAT,
 *     GM_HOT_SPARSE, GM_HOT_RH_INSERT, GM_NO_RH_EXIT, GM_NO_MPH, GM_MPH_TABLES,
 *     GM_MPH_SLACK, GM_MPH_LAMBDA, GM_MPH_MIN_KEYS, GM_MPH_MAX_KEYS,
 *     GM_MPH_NO_FILTERED, GM_CHAIN, GM_NO_CHAIN, GM_NO_EDGE_FILTER,
 *     GM_EFILT_ALL, GM_EFILT_DIV, GM_EFILT_MAX_KB, GM_DICT_MUL, GM_L1_BYPASS,
 *     GM_TRIE_RUNS, GM_MIRROR, GM_NO_MIRROR;
 *   walk and staging:   GM_FUSED_PRIO, GM_HOT_POLICY, GM_NT, GM_D0,
 *     GM_STAGE_COMPACT, GM_STAGE_SC1, GM_LISTED_CAP, GM_LISTED_DEFER,
 *     GM_SCAN_SPLIT, GM_SCAN_SUMS, GM_NO_SPEC_IDS, GM_ASM_STREAM, GM_HOT_FLAT
 *     (per call too: the walk's flat-load instantiation);
 *   host path:          GM_HOST_SIMPLE, GM_HOST_PIPE, GM_HOST_CHUNK,
 *     GM_HOST_THREADS, GM_HOST_BOUNCE, GM_HOST_WIDE_ROWS, GM_HOST_OFF32,
 *     GM_FANOUT_MULTI_MIN, GM_FANOUT_SIMPLE, GM_FANOUT_FUSED_ONLY;
 *   publish window:     GM_PW_CAP_HITS, GM_PW_CAP_PAIRS, GM_PW_CAP_DELIVERIES
 *     (the speculative pick / plan / deliveries capacities as given; 0: that
 *     part is not speculated);
 *   updates:            GM_UPDATE_OVERLAY, GM_UPDATE_UNFUSED, GM_SPARE_BLOB_MIN;
 *   diagnostics:        GM_UPDATE_TIMING, GM_INDEX_STATS, GM_INDEX_VERIFY.
 */
#ifndef EMQX_GPU_MATCH_H
#define EMQX_GPU_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMQX_GM_ABI_VERSION 1

#define EMQX_GM_OK            0
#define EMQX_GM_EINVAL       -1 /* bad argument (badarg / function_clause)     */
#define EMQX_GM_ENOMEM       -2 /* host or device allocation failed            */
#define EMQX_GM_EDEVICE      -3 /* HIP runtime / device fault                  */
#define EMQX_GM_EOVERFLOW    -4 /* a row exceeded the device result capacity    */
#define EMQX_GM_EUNSUPPORTED -5 /* operation not available on this build       */

/* emqx_gm_match / emqx_gm_fanout flags */
#define EMQX_GM_WITH_EXACT 0x1u /* emqx_router:match_routes/1 semantics        */
#define EMQX_GM_DEVICE_IO  0x2u /* inputs are device pointers; result stays on
                                   the device (bench / multi-GPU path)         */
#define EMQX_GM_NO_TIMING  0x4u /* emqx_gm_match / _submit on device buffers:
                                   do not time this call's main pass
                                   (stats.match_kernel_ms and total_device_ms
                                   read 0).  A timed call puts the kernel's
                                   start/stop timestamps on the stream, which
                                   costs the device ~5 us of idle each; a
                                   serving loop times one call in a few      */

typedef struct emqx_gm_ctx emqx_gm_ctx;
typedef struct emqx_gm_index emqx_gm_index;
typedef struct emqx_gm_call emqx_gm_call;

/* Device list (the opts "select the device list (1-8)").  A BEAM
 * node loads its NIF once, so one context must be able to serve the whole
 * node's GPUs, as the reference's match_routes/1 runs in every publisher
 * process on all schedulers at once (apps/emqx/src/emqx_trie.erl:66-70,
 * emqx_router.erl:75-84, 128-145).  With n_devices = k > 0 the context owns
 * one replica of every index per listed device (a device may be listed more
 * than once: several replicas, e.g. a one-GPU rehearsal):
 *   - an index is compiled ONCE on the host and its device tables are copied
 *     to the other devices device to device (peer copies over xGMI, in a tree:
 *     every replica made is the source of another, so 8 devices take 3 rounds
 *     of copies and every device's links carry them);
 *   - an update is applied on every device at once, each from its own replica
 *     of the predecessor, as every EMQX node applies the same route delta to
 *     its own tables (emqx_router_utils.erl:33-38, emqx_trie.erl:114-136): the
 *     in-place patch's host plan is made once and each device runs its own
 *     one-pass patch; a subscriber-only emqx_gm_index_update_subs shares each
 *     replica's tables and writes each device's new subscriber CSR there;
 *     rebuilds and imports are copied as at a build; an overlay result (a
 *     filter with '#' inside) stays on the first device and is matched there;
 *   - emqx_gm_match on host buffers: a batch of more than one chunk (256K
 *     topics) is cut into chunks that run on all the devices at once (one host
 *     pipeline per device), the rows back in the caller's ONE CSR in batch
 *     order; a smaller batch runs whole on ONE device, the next one
 *     round-robin, so concurrent callers (dirty schedulers) run on different
 *     GPUs at once (on any context, such a call stages its topics into
 *     page-locked buffers of its own and waits for the device without the
 *     context lock: concurrent small calls overlap on one GPU too);
 *   - emqx_gm_fanout on host rows (65,536 rows or more) cuts them into one
 *     slice per device, balanced by matches, into the caller's ONE result;
 *     fewer rows (a publish window's, at most 16M deliveries) run whole on
 *     ONE device, round-robin like a small match, and -- on any context --
 *     hold its lock only to queue their work, so concurrent fan-outs overlap;
 *   - device-buffer calls (EMQX_GM_DEVICE_IO, emqx_gm_match_submit, a
 *     device-row fan-out), the sharding helpers, emqx_gm_set_stream and
 *     emqx_gm_index_device_blob / _export use the first listed device; so
 *     does any call on an index made through another context (it has no
 *     replicas here).
 * n_devices = 0 is the single-device context on `device`. */
#define EMQX_GM_MAX_DEVICES 8
typedef struct {
  int32_t device;        /* HIP device ordinal (n_devices == 0)                 */
  uint32_t flags;        /* EMQX_GM_OPEN_* (0: defaults)                        */
  uint32_t n_devices;    /* 0: `device` alone; 1..EMQX_GM_MAX_DEVICES: devices[] */
  int32_t devices[EMQX_GM_MAX_DEVICES];
  uint32_t reserved0;
  uint64_t reserved[2];
} emqx_gm_opts;

/* emqx_gm_opts.flags: the host copy of a plain index's device tables that an
 * in-place emqx_gm_index_update patches (host RAM ~ the tables' size).  By
 * default it is kept from the build for tables up to 8 GiB and downloaded from
 * the device on a snapshot line's first update above that (a 100M-filter index
 * holds no 53 GB host copy unless it is updated; an import follows the same
 * policy, its copy made from the image when it carries the tables). */
#define EMQX_GM_OPEN_MIRROR_EAGER 0x1u /* always keep it from the build            */
#define EMQX_GM_OPEN_MIRROR_LAZY  0x2u /* never at build: on the first update      */

/* CSR result: row i = ids[row_off[i] .. row_off[i+1]) */
typedef struct {
  uint64_t n_rows;
  uint64_t nnz;
  uint64_t *row_off;     /* n_rows + 1 entries                                 */
  uint32_t *ids;         /* nnz entries (filter ids or subscriber ids)          */
  int32_t on_device;     /* 1: device pointers, 0: host pointers                */
  int32_t reserved0;
  void *priv;            /* library bookkeeping; do not touch                   */
} emqx_gm_csr;

typedef struct {
  uint64_t n_filters;    /* unique filters; ids 0..n_filters-1                  */
  uint64_t n_wildcard;   /* filters the trie holds (emqx_topic:wildcard/1)      */
  uint64_t n_nodes;      /* level-trie nodes                                    */
  uint64_t n_edges;      /* exact/'+'/'#' edges                                 */
  uint64_t n_words;      /* distinct words                                      */
  uint64_t n_subs;       /* subscriber entries (fan-out CSR)                    */
  uint64_t device_bytes; /* resident index bytes in HBM                         */
  uint32_t max_depth;    /* deepest filter (levels)                             */
  int32_t trie_empty;    /* emqx_trie:empty/0 (no wildcard filter)              */
} emqx_gm_index_info_t;

/* probes: the probes the reference NFA makes for the batch (SURVEY.md 8d's P),
 * not a count of loads: per topic 1 (the exact-route probe) + 3 per frontier
 * node and level + 2 per node reached at the last level; 0 for a wildcard
 * publish topic.  Exact when no row leaves a pass for capacity (a row of more
 * than 16 matches, a frontier past a pass's capacity, a full tile list);
 * otherwise each such row may be counted by up to two passes: the main pass
 * and the listed pass each add what they walked of it before giving it up, the
 * slow path adds nothing.  Topics of more than 8 levels are counted by the
 * listed pass alone.  (tests/test_gpu_probe_count.py) */
typedef struct {
  uint64_t n_topics;
  uint64_t nnz;
  uint64_t n_overflow;       /* rows completed by the device slow path        */
  uint64_t n_wildcard_topics; /* publish topics with a '+' or '#' word (each once) */
  double match_kernel_ms;    /* device time of the fast match kernel          */
  double total_device_ms;    /* device time of all kernels of the call         */
  uint64_t algo_bytes;       /* algorithmic bytes of the fast kernel */
  uint64_t probes;           /* NFA edge probes of the batch (see above)       */
} emqx_gm_match_stats;

/* ---- context ---- */
int emqx_gm_open(const emqx_gm_opts *opts, emqx_gm_ctx **out);
int emqx_gm_close(emqx_gm_ctx *ctx);
/* Message of the calling thread's last failing call (valid until that
 * thread's next call into the library). */
const char *emqx_gm_last_error(const emqx_gm_ctx *ctx);
int emqx_gm_abi_version(void);
/* Use an external HIP stream (e.g. torch's current stream); NULL = own. */
int emqx_gm_set_stream(emqx_gm_ctx *ctx, void *hip_stream);
int emqx_gm_synchronize(emqx_gm_ctx *ctx);

/* ---- index (emqx_trie / emqx_route / emqx_subscriber snapshot) ---- */
/* filters in any order (duplicates allowed: one id, subscriber lists are
 * concatenated).  perm_out (optional, n_filters entries) receives the id of
 * each input filter.  sub_off/sub_ids (optional) give each input filter's
 * subscriber ids (CSR with n_filters+1 offsets). */
int emqx_gm_index_build(emqx_gm_ctx *ctx, const uint8_t *filter_bytes, const uint64_t *filter_off,
                        uint64_t n_filters, const uint64_t *sub_off, const uint32_t *sub_ids,
                        uint32_t *perm_out, emqx_gm_index **out);
/* Incremental maintenance (emqx_router:do_add_route/2 / do_delete_route/2 ->
 * emqx_trie:insert/1, delete/1, apps/emqx/src/emqx_router.erl:112-125,
 * 164-172, emqx_trie.erl:107-136).  Applies n_ops filter inserts (ops[i] = 1,
 * idempotent) and deletes (ops[i] = 0, only if present), in order, to `prev`
 * and returns a NEW snapshot; `prev` is unchanged (readers holding it keep
 * it: RCU).  The newest snapshot of a line is patched in place on a device
 * copy of its tables: the result is a flat snapshot, a match on it costs what
 * a match on a rebuilt index costs, and the update costs O(delta) host work +
 * one device pass over the index (read once, written once into the new
 * snapshot's tables; those of the last released snapshot of the same size are
 * reused when there are any -- emqx_gm_pool_trim frees them).  A plain index keeps a host copy of its device
 * tables for this (host RAM ~ emqx_gm_index_info().device_bytes), handed on
 * to each newer snapshot.  Otherwise -- a filter with '#' before its last
 * word, or an update of a snapshot that is no longer the newest -- the new
 * snapshot shares prev's tables (tombstones + a delta index; emqx_gm_fanout
 * refuses it).  Past 1/8 of the set, or when the tables run out of headroom,
 * the set is rebuilt.  Ids in rows of the new snapshot are ranks in the
 * updated set, as a full rebuild would give.
 * A prefix-sharded index (emqx_gm_index_build_sharded) built WITHOUT
 * subscriber lists is updated the same way, shard by shard and all devices at
 * once: the route is fixed, so a new filter goes to the shard its matching
 * topics are routed to; a shard with changes is patched in place (or, without
 * room or mirror, recompiled alone), a shard without any shares its previous
 * tables, and every shard gets a new local-to-global id map from one device
 * pass.  Rows of the result are bit-equal to a fresh sharded or unsharded
 * build of the updated set; a batch with no net change returns `prev`
 * retained.  Not available for stand-alone shard indexes
 * (emqx_gm_index_build_shard) or indexes -- sharded ones included -- with
 * subscriber lists (EMQX_GM_EUNSUPPORTED: rebuild those, or use
 * emqx_gm_index_update_subs on a plain one). */
int emqx_gm_index_update(emqx_gm_ctx *ctx, emqx_gm_index *prev, const uint8_t *filter_bytes,
                         const uint64_t *filter_off, const uint8_t *ops, uint64_t n_ops, emqx_gm_index **out);
/* Subscriber maintenance on an index built with subscriber lists
 * (emqx_broker:subscribe/2, unsubscribe/1 with the route added on a filter's
 * first subscriber and deleted after its last: apps/emqx/src/
 * emqx_broker.erl:147-165, 445-454, emqx_router.erl:112-125, 164-172).
 * Applies n_ops ops in order: ops[i] = EMQX_GM_SUB_SUBSCRIBE subscribes
 * sub_ids[i] to filter i (idempotent per pair), EMQX_GM_SUB_UNSUBSCRIBE
 * unsubscribes it (only if present).  A subscribe appends to the filter's
 * list, an unsubscribe keeps the others' order.  EMQX_GM_SUB_ROUTE_ADD /
 * ROUTE_DELETE (sub_ids[i] ignored) mark / unmark filter i as routed to
 * another destination (a remote node or a shared group: do_add_route/2 with
 * a dest other than the local node): a filter is in the index while it has a
 * local subscriber OR that mark, so its matches still come back (with an
 * empty subscriber segment) for the caller's lookup_routes/1 -- or, for node
 * destinations, for emqx_gm_forward_plan below.  In a built
 * index, a filter given no subscribers carries the mark.
 * Returns a NEW snapshot (RCU, as emqx_gm_index_update): route changes are
 * patched into a device copy of the newest snapshot's tables and the new
 * snapshot gets a subscriber CSR of its own; what the patch cannot take is
 * rebuilt.  EMQX_GM_EUNSUPPORTED for indexes without subscriber lists (use
 * emqx_gm_index_update), overlay snapshots and shard indexes. */
#define EMQX_GM_SUB_UNSUBSCRIBE 0u
#define EMQX_GM_SUB_SUBSCRIBE 1u
#define EMQX_GM_SUB_ROUTE_ADD 2u
#define EMQX_GM_SUB_ROUTE_DELETE 3u
int emqx_gm_index_update_subs(emqx_gm_ctx *ctx, emqx_gm_index *prev, const uint8_t *filter_bytes,
                              const uint64_t *filter_off, const uint32_t *sub_ids, const uint8_t *ops,
                              uint64_t n_ops, emqx_gm_index **out);
/* Index images: one snapshot compiled once and replicated (the reference's
 * routing tables are ONE copy that mria replicates to every node, not a
 * per-node recomputation: apps/emqx/src/emqx_router.erl:75-84, 136).
 * export: the snapshot as a self-contained host image -- the host tables
 * (layout, sorted filter table, shard ids, subscriber offsets, route marks)
 * and, unless EMQX_GM_IMAGE_NO_BLOB, the device tables; two-call sizing (buf
 * NULL sets *size).  device_blob: the device tables of a snapshot (read-only;
 * e.g. the source of an RCCL broadcast to the other GPUs).  import: a new
 * snapshot on ctx's device from an image, its device tables from the image or,
 * when d_blob is not NULL, copied from d_blob (device memory of ctx's device,
 * device_blob's bytes).  An imported plain index keeps its in-place update
 * line: its host mirror loads on the first update.  Overlay snapshots and
 * emqx_gm_index_update_subs results: EMQX_GM_EUNSUPPORTED (export a rebuilt
 * or emqx_gm_index_update'd snapshot).  An image is accepted only by a library
 * of the same table layout (EMQX_GM_EINVAL otherwise). */
#define EMQX_GM_IMAGE_NO_BLOB 0x1u
int emqx_gm_index_export(emqx_gm_ctx *ctx, const emqx_gm_index *idx, uint32_t flags, uint8_t *buf,
                         uint64_t *size);
int emqx_gm_index_device_blob(const emqx_gm_index *idx, const void **d_blob, uint64_t *bytes);
int emqx_gm_index_import(emqx_gm_ctx *ctx, const uint8_t *image, uint64_t size, const void *d_blob,
                         emqx_gm_index **out);
int emqx_gm_index_retain(emqx_gm_index *idx);
int emqx_gm_index_release(emqx_gm_index *idx);
int emqx_gm_index_info(const emqx_gm_index *idx, emqx_gm_index_info_t *info);
/* bytes of filter `id` (host memory owned by the index) */
int emqx_gm_index_filter(const emqx_gm_index *idx, uint32_t id, const uint8_t **bytes, uint64_t *len);
/* Number of subscribers of filter `id` (0 for an index built without
 * subscriber lists): the length of that filter's segment in a fan-out row,
 * which lets a caller split a row back into (filter, subscribers) groups --
 * do_dispatch/2 sends {deliver, Filter, Msg} per filter (emqx_broker.erl:
 * 506-525). */
int emqx_gm_index_subscriber_count(const emqx_gm_index *idx, uint32_t id, uint64_t *n);

/* ---- hot path ---- */
int emqx_gm_match(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                  const uint64_t *topic_off, uint64_t n_topics, uint32_t flags, emqx_gm_csr *out);
/* emqx_gm_match in two halves, for device buffers (EMQX_GM_DEVICE_IO
 * required): submit queues the call's kernels on the context stream and
 * returns at once; wait blocks until that call is done, hands out its rows
 * (exactly what emqx_gm_match returns) and frees the call.  Several calls may
 * be in flight on one context, from one thread or many (the reference matches
 * in every publisher's own process, lock-free: emqx_trie.erl:68-70,
 * emqx_router.erl:128-145): a batch's launches queue behind the previous
 * one's while the host still finishes that one, so the device does not idle
 * between small batches.  The inputs (and the index, which the call retains)
 * must stay valid until wait returns.  Overlay snapshots: EMQX_GM_EUNSUPPORTED
 * (use emqx_gm_match).  emqx_gm_match itself waits without the context lock
 * for device buffers. */
int emqx_gm_match_submit(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                         const uint64_t *topic_off, uint64_t n_topics, uint32_t flags, emqx_gm_call **call);
int emqx_gm_match_wait(emqx_gm_ctx *ctx, emqx_gm_call *call, emqx_gm_csr *out);
/* Pinned host buffers for the host-buffer emqx_gm_match: topic text (and
 * offsets) that a caller packs straight into memory from emqx_gm_host_alloc
 * crosses PCIe by DMA from where it lies, with no staging copy by the
 * library's workers (the NIF packs a publish batch's binaries here).  The
 * memory is page-locked and visible to every device of the context; free it
 * with emqx_gm_host_free on the same context. */
int emqx_gm_host_alloc(emqx_gm_ctx *ctx, uint64_t bytes, void **p);
int emqx_gm_host_free(emqx_gm_ctx *ctx, void *p);
/* The devices of a context, in emqx_gm_opts order (*n = 1 for a single-device
 * context); devices may be NULL to ask for the count. */
int emqx_gm_devices(const emqx_gm_ctx *ctx, int32_t *devices, uint32_t *n);
int emqx_gm_fanout(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const emqx_gm_csr *matches,
                   uint32_t flags, emqx_gm_csr *out_subs);
/* emqx_broker:publish/1's route + dispatch of a batch in one call
 * (emqx_broker.erl:204-215, 245-322): the rows of emqx_gm_match(flags) into
 * *matches and their fan-out, as emqx_gm_fanout gives it, into *deliveries
 * (host buffers only; flags: EMQX_GM_WITH_EXACT or 0).  A publish window (a
 * batch of at most one chunk, 256K topics) makes ONE device round trip for
 * both: the fan-out is queued right behind the match's speculative rows and
 * kept when the rows and the deliveries fit their capacities (else the
 * fan-out runs after the match, as the two calls would).  On error nothing is
 * returned; both results are freed with emqx_gm_csr_free.  The NIF's
 * fanout_batch/2. */
int emqx_gm_match_fanout(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                         const uint64_t *topic_off, uint64_t n_topics, uint32_t flags, emqx_gm_csr *matches,
                         emqx_gm_csr *deliveries);

/* ---- publish windows coalesced into one device round trip ----
 * Every scheduler of a broker node publishes at once: emqx_broker:publish/1
 * routes and dispatches in the caller's own process
 * (apps/emqx/src/emqx_broker.erl:204-215, 296-322) and emqx_trie:match/1 reads
 * the shared tables from all of them concurrently (emqx_trie.erl:66-70).  Here
 * each such caller brings one small window, and a window alone keeps the
 * device busy for a fraction of what its chain of launches costs; the calls
 * below run many windows as ONE device batch and hand each window its own
 * result.
 *
 * emqx_gm_match_windows: n_windows host-buffer windows in one call.
 * matches[k] -- and deliveries[k], unless deliveries is NULL (match only) -- are
 * CSRs of their own (host pointers, row_off[0] == 0), bit-equal to what
 * emqx_gm_match_fanout (emqx_gm_match) returns for window k alone, each freed
 * on its own with emqx_gm_csr_free, in any order, from any thread.  flags:
 * EMQX_GM_WITH_EXACT or 0.  Windows are grouped in order, a group being at
 * most 64 windows, one chunk of topics (256K) and 1 MiB of text; a group makes
 * one device round trip (one input copy, one match, the fan-out behind it, one
 * launch that cuts the rows into the windows' results) on one device of the
 * context, round-robin.  A window that a single call would not serve whole on
 * one device (an overlay or sharded index, more than one chunk), one holding a
 * topic longer than 65,535 B or more than 1 MiB of text runs alone through
 * the ordinary call, in its place.  A NULL argument, bad flags or a window
 * with non-monotone offsets: EMQX_GM_EINVAL before any device work, no output
 * touched.  On any later error every output is zeroed and nothing is held. */
typedef struct {
  const uint8_t *topic_bytes;
  const uint64_t *topic_off; /* n_topics + 1 entries */
  uint64_t n_topics;
} emqx_gm_window;
int emqx_gm_match_windows(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const emqx_gm_window *windows,
                          uint32_t n_windows, uint32_t flags, emqx_gm_csr *matches, emqx_gm_csr *deliveries);

/* emqx_gm_combiner: the same for callers that do not know of one another (a
 * NIF's dirty schedulers).  emqx_gm_combiner_match is emqx_gm_match_fanout
 * (deliveries != NULL) or emqx_gm_match (NULL) of the caller's window,
 * blocking and thread safe, with the same results and errors.  A caller
 * checks its own window (EMQX_GM_EINVAL fails that call alone) and queues it;
 * while fewer than max_in_flight groups are on the device it becomes a
 * leader, takes every queued window of the same index, flags and
 * deliveries-or-not up to the group limits, runs them through
 * emqx_gm_match_windows and hands each caller its own CSRs and return code; a
 * leader's failure reaches every member of its group.  What stays queued is
 * led by one of its owners next.  With the defaults a lone caller never
 * waits: coalescing comes only from what queued while earlier groups were on
 * the device.  Every setting is in the opts (0: the default); there is no
 * environment knob.
 *   max_windows   windows per group (default 64, at most 256)
 *   max_topics    topics per group (default and most: one chunk, 256K)
 *   max_in_flight groups on the device at once (default 2)
 *   min_windows, linger_us   a leader waits until min_windows windows have
 *                 arrived or linger_us has passed (defaults 1 and 0: no wait;
 *                 for tests and tuning)
 * After a combiner call emqx_gm_last_stats(ctx) reports, to the calling
 * thread, the figures of the GROUP its window ran in (n_topics and nnz of the
 * whole group), not of the window alone.  emqx_gm_combiner_close waits for
 * the calls in flight; calls after it return EMQX_GM_EINVAL (close it before
 * the context, and let no call start once it returns). */
typedef struct emqx_gm_combiner emqx_gm_combiner;
typedef struct {
  uint32_t max_windows;
  uint64_t max_topics;
  uint32_t max_in_flight;
  uint32_t min_windows;
  uint32_t linger_us;
  uint64_t reserved[2];
} emqx_gm_combiner_opts;
typedef struct {
  uint64_t windows;   /* calls queued                                        */
  uint64_t groups;    /* groups run                                          */
  uint64_t max_group; /* windows of the largest group                        */
  uint64_t solo;      /* groups of one window                                */
} emqx_gm_combiner_stats_t;
int emqx_gm_combiner_open(emqx_gm_ctx *ctx, const emqx_gm_combiner_opts *opts, emqx_gm_combiner **out);
int emqx_gm_combiner_match(emqx_gm_combiner *cb, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                           const uint64_t *topic_off, uint64_t n_topics, uint32_t flags, emqx_gm_csr *matches,
                           emqx_gm_csr *deliveries);
int emqx_gm_combiner_stats(const emqx_gm_combiner *cb, emqx_gm_combiner_stats_t *stats);
int emqx_gm_combiner_close(emqx_gm_combiner *cb);

int emqx_gm_csr_free(emqx_gm_ctx *ctx, emqx_gm_csr *csr);
int emqx_gm_last_stats(const emqx_gm_ctx *ctx, emqx_gm_match_stats *stats);

/* ---- sharded index (BASELINE configs[4]) ----
 * For filter sets too large to replicate, filters are hash-partitioned over
 * devices (emqx_gm_shard_of), every device matches the whole publish batch
 * against its shard, rows are exchanged (RCCL all-to-all: device q receives
 * topic slice q from every shard) and merged by global filter id.  The
 * reference has no sharded trie (every node replicates emqx_route/emqx_trie
 * through mria, emqx_router.erl:75-84); the merged rows equal the unsharded
 * match_routes/1 rows. */
/* Global id of each filter: its lexicographic rank among the unique filters
 * (the id an unsharded emqx_gm_index_build would assign). */
int emqx_gm_filter_ranks(const uint8_t *filter_bytes, const uint64_t *filter_off, uint64_t n_filters,
                         uint32_t *rank_out, uint64_t *n_unique);
/* Shard of each filter: fmix64(word hash of the filter bytes) mod n_shards. */
int emqx_gm_shard_of(const uint8_t *filter_bytes, const uint64_t *filter_off, uint64_t n_filters,
                     uint32_t n_shards, uint32_t *shard_out);
/* Index over one shard whose result rows carry the given global ids (which
 * must ascend with the filter bytes).  emqx_gm_fanout is not available on a
 * shard index (subscribers live with their shard: fan out before merging). */
int emqx_gm_index_build_shard(emqx_gm_ctx *ctx, const uint8_t *filter_bytes, const uint64_t *filter_off,
                              uint64_t n_filters, const uint32_t *global_ids, const uint64_t *sub_off,
                              const uint32_t *sub_ids, uint32_t *perm_out, emqx_gm_index **out);
/* Row lengths of a device CSR into device memory (u32 per row). */
int emqx_gm_csr_row_lengths(emqx_gm_ctx *ctx, const emqx_gm_csr *csr, uint32_t *d_lens);
/* Merge n_pieces per-shard results for the same n_rows rows.  d_lens: device
 * u32 [n_pieces][stride] (stride >= n_rows, padding rows 0); d_ids: device
 * u32, the pieces' rows concatenated piece-major.  Rows are disjoint sorted
 * id lists; the result rows are their sorted unions (flags: DEVICE_IO keeps
 * the CSR on the device). */
int emqx_gm_merge_rows(emqx_gm_ctx *ctx, uint64_t n_rows, uint64_t stride, uint32_t n_pieces,
                       const uint32_t *d_lens, const uint32_t *d_ids, uint32_t flags, emqx_gm_csr *out);

/* ---- prefix sharding (gm_route.hip): each topic needs ONE shard ----
 * A topic can only match filters whose first word is its own first word, '+'
 * or '#' (emqx_topic:match/2, emqx_topic.erl:65-87).  emqx_gm_prefix_plan
 * partitions filters by first word (a hot first word -- over 1/(2N) of the
 * filters -- by its first two words) over n_shards, greedily by size; filters
 * whose first word is '+' / '#' (and a hot word's 'w', 'w/#', 'w/+/...') go to
 * every shard (shard_out = EMQX_GM_ALL_SHARDS).  The returned route maps each
 * topic to the one shard that holds every filter it can match, so a batch is
 * routed (all-to-all of topic bytes), each rank walks only its share, and the
 * rows go back to the topics' ranks (emqx_gm_unpermute_rows) -- no merge. */
#define EMQX_GM_ALL_SHARDS 0xFFFFFFFFu
typedef struct emqx_gm_route emqx_gm_route;
int emqx_gm_prefix_plan(const uint8_t *filter_bytes, const uint64_t *filter_off, uint64_t n_filters,
                        uint32_t n_shards, uint32_t *shard_out, emqx_gm_route **route);
/* The prefix-sharded index behind ONE multi-device context (the NIF's form of
 * this plan, for a filter set that does not fit one GPU): the filters are
 * partitioned as emqx_gm_prefix_plan does over the context's devices (one
 * shard per listed device; '+' / '#'-first filters on every one), each shard
 * compiled and placed on its device at once.  The returned index is used like
 * any other: emqx_gm_match on host buffers routes each topic to its one shard,
 * matches every device's topics there at the same time and returns the rows in
 * batch order (global ids, bit-exact with an unsharded index); emqx_gm_fanout
 * on host rows fans each row out on its shard; emqx_gm_index_info / _filter /
 * _subscriber_count answer for the whole set.  emqx_gm_index_update takes a
 * sharded index built without subscriber lists (see there); on such an index
 * emqx_gm_fanout gives no deliveries.  Still EMQX_GM_EUNSUPPORTED on a sharded
 * index: emqx_gm_index_update when it was built with subscriber lists,
 * emqx_gm_index_update_subs (out of scope: subscriber changes of a sharded set
 * need a rebuild), images and device-buffer calls.  Arguments as
 * emqx_gm_index_build. */
int emqx_gm_index_build_sharded(emqx_gm_ctx *ctx, const uint8_t *filter_bytes, const uint64_t *filter_off,
                                uint64_t n_filters, const uint64_t *sub_off, const uint32_t *sub_ids,
                                uint32_t *perm_out, emqx_gm_index **out);
/* dest[i] = the shard of topic i (host buffers / device buffers, n_topics entries) */
int emqx_gm_route_topics_host(const emqx_gm_route *route, const uint8_t *topic_bytes, const uint64_t *topic_off,
                              uint64_t n_topics, uint32_t *dest);
int emqx_gm_route_topics(emqx_gm_ctx *ctx, emqx_gm_route *route, const uint8_t *d_topic_bytes,
                         const uint64_t *d_topic_off, uint64_t n_topics, uint32_t *d_dest);
int emqx_gm_route_release(emqx_gm_route *route);
/* The send order of a routed device batch in one call (the step's route, sort
 * and split sizes): d_perm[i] = the batch index of the i-th topic in order of
 * (shard, batch index), d_plen[i] = its length in bytes, d_split[2 s] / [2 s + 1]
 * = the topics / bytes bound for shard s (n_shards <= 256).  Device buffers:
 * n_topics u32 each, 2 * n_shards u64.  Stream-ordered like the other calls. */
int emqx_gm_route_partition(emqx_gm_ctx *ctx, emqx_gm_route *route, const uint8_t *d_topic_bytes,
                            const uint64_t *d_topic_off, uint64_t n_topics, uint32_t *d_perm, uint32_t *d_plen,
                            uint64_t *d_split);
/* (route_topics / route_partition / permute_topics / unpermute_rows index the
 * batch with u32: n_topics / n_rows < 2^32 - 1, else EMQX_GM_EINVAL) */
/* The exchange's device steps.  permute: out topic i = topic perm[i] (d_out
 * holds as many bytes as the input, d_out_off n+1 entries).  unpermute: row
 * perm[i] of the result = input row i, the input rows packed with u32 lengths
 * d_lens[i] (flags: EMQX_GM_DEVICE_IO keeps the CSR on the device). */
int emqx_gm_permute_topics(emqx_gm_ctx *ctx, const uint8_t *d_topic_bytes, const uint64_t *d_topic_off,
                           uint64_t n_topics, const uint32_t *d_perm, uint8_t *d_out, uint64_t *d_out_off);
int emqx_gm_unpermute_rows(emqx_gm_ctx *ctx, uint64_t n_rows, const uint32_t *d_perm, const uint32_t *d_lens,
                           const uint32_t *d_ids, uint32_t flags, emqx_gm_csr *out);

/* ---- retained-message lookup (gm_retained.cpp / gm_retained.hip): the subscribe direction ----
 * When a client subscribes, the broker hands it every retained message whose
 * topic the filter matches.  The reference scans the whole table per
 * subscription: emqx_retainer_mnesia:match_messages/1 turns the filter into a
 * match-spec (condition/1) and runs mnesia:dirty_select over it
 * (apps/emqx_retainer/src/emqx_retainer_mnesia.erl:210-244).  Here the stored
 * topics are compiled once into a level trie in HBM and a batch of filters is
 * walked against it, one wave per filter.
 * Semantics (bit-exact with condition/1, emqx_retainer_mnesia.erl:225-230): topics
 * and filters are split on '/', empty words kept; '+' matches any one word; a
 * final '#' matches any number of further words, none included ('a/#' matches
 * 'a'); without it the word counts must be equal; a '#' before the last word
 * matches nothing (the row is empty, the call does not fail); 'a+' is a
 * literal.  There is NO '$'-rule: '#' and '+/x' match '$SYS/...' topics, unlike
 * emqx_gm_match.  A topic is returned if its expiry is 0 or > now_ms
 * (make_match_spec/1, :232-244); the library reads no clock.
 * A result row holds the caller's ids of the matching topics in word-list order
 * of the topics (word by word as unsigned bytes, a proper prefix first); the
 * reference's sort by timestamp (sort_retained/1) is the caller's.
 * On a multi-device context the index lives on the first listed device and the
 * calls run there (no replication). */
typedef struct emqx_gm_retained emqx_gm_retained;
typedef struct {
  uint64_t n_topics;      /* distinct stored topics                              */
  uint64_t n_nodes;       /* level-trie nodes, root and sentinels included       */
  uint64_t n_words;       /* distinct words                                      */
  uint64_t device_bytes;  /* resident index bytes in HBM (0: a host-only index)  */
  uint64_t widest_level;  /* nodes of the widest level                           */
  uint64_t walk_ws_bytes; /* global workspace a match call takes (0: LDS frames) */
  uint32_t depth_max;     /* words of the deepest topic                          */
  int32_t lds_frames;     /* 1: the walk's frames fit LDS, 0: global workspace   */
} emqx_gm_retained_info_t;
/* The table as emqx_retainer_mnesia:store_retained/2 leaves it (:74-104; mria:
 * dirty_write overwrites): duplicates allowed, the LAST one's id and expiry
 * are kept.  ids NULL: the position in the input; expiry_ms NULL: none expires.
 * flags: 0.  n_topics < 2^32 - 1; offsets must ascend and each topic be under
 * 2 GiB -- the boundary carries no byte count, so that is how far an offset
 * past the buffer can be told (EMQX_GM_EINVAL, before any device work). */
int emqx_gm_retained_build(emqx_gm_ctx *ctx, const uint8_t *topic_bytes, const uint64_t *topic_off,
                           uint64_t n_topics, const uint32_t *ids, const uint64_t *expiry_ms, uint32_t flags,
                           emqx_gm_retained **out);
/* emqx_retainer_mnesia:match_messages/1 (:210-214) batched over n_filters
 * subscriptions: host buffers in, a host CSR out exactly as the host-buffer
 * emqx_gm_match returns one (free with emqx_gm_csr_free).  flags: 0, or
 * EMQX_GM_RET_TIMED (the call's passes are timed, emqx_gm_retained_last_times). */
#define EMQX_GM_RET_TIMED 0x1u
int emqx_gm_retained_match(emqx_gm_ctx *ctx, const emqx_gm_retained *idx, const uint8_t *filter_bytes,
                           const uint64_t *filter_off, uint64_t n_filters, uint64_t now_ms, uint32_t flags,
                           emqx_gm_csr *out);
/* Sets the expiry of the stored topics among n_topics literal topics (absent
 * ones are skipped); *n_found = the stored ones.  NOT a snapshot: the expiry
 * array is mutated in place, in stream order with matches.  Covers
 * emqx_retainer_mnesia:delete_message/2 of a literal topic (:117-128: set
 * expiry 1), a refreshed message on an existing topic (store_retained/2), and
 * clear_expired/1 (:106-115), which needs no call: a match already hides expired
 * topics.  A topic listed twice in one call gets one of its expiries. */
int emqx_gm_retained_expire(emqx_gm_ctx *ctx, emqx_gm_retained *idx, const uint8_t *topic_bytes,
                            const uint64_t *topic_off, uint64_t n_topics, const uint64_t *expiry_ms,
                            uint64_t *n_found);
/* emqx_retainer_mnesia:size/1 (:164-165) and the table's shape */
int emqx_gm_retained_info(const emqx_gm_retained *idx, emqx_gm_retained_info_t *info);
/* emqx_retainer_mnesia:clean/1 of this table (:160-162) */
int emqx_gm_retained_release(emqx_gm_retained *idx);

/* ---- shared-subscription dispatch (gm_shared.cpp / gm_shared.hip): one group member per match ----
 * A filter routed to a shared group ('$share/Group/Filter', dest {Group, Node})
 * comes back from a match as a route mark only; the reference then calls
 * emqx_shared_sub:dispatch/3 once per message and group, which picks ONE member
 * of the group (pick/6, do_pick/6, pick_subscriber/6, do_pick_subscriber/6,
 * apps/emqx/src/emqx_shared_sub.erl:113-130, 234-288).  Here the picks of a
 * whole publish window are computed in one device call, bit-equal to running
 * pick/6 hit by hit in batch order in one publisher process.
 * A SLOT is one {Group, Filter} pair with its member list (subscribers/2,
 * :287-288: an ets bag -- insertion order, an identical member stored once).
 * A HIT is a (message row, matched filter id, slot of that filter) triple;
 * BATCH ORDER is rows ascending, filter ids in the order the row holds them,
 * then the filter's slots ascending by group id.  For a hit on slot s with
 * Count members (state per slot, kept in the table; mix / mix3 as defined in
 * gm_shared.h: fmix(h) is the 32-bit finalizer h ^= h >> 16, h *= 0x85EBCA6B,
 * h ^= h >> 13, h *= 0xC2B2AE35, h ^= h >> 16; mix(a, b) = fmix(fmix(a +
 * 0x9E3779B9) + b); mix3(a, r, s) = mix(mix(a, r), s); all mod 2^32):
 *   EMQX_GM_SHARE_HASH (hash_clientid, hash_topic, hash; :272-278):
 *     members[msg_hash[row] rem Count]; the caller computes erlang:phash2/1 of
 *     the client id or the source topic per message.
 *   EMQX_GM_SHARE_ROUND_ROBIN (:279-285): Rem = rr[s] unset ? mix(seed, s) rem
 *     Count : (rr[s] + 1) rem Count with the CURRENT Count; rr[s] = Rem; pick
 *     members[Rem].  The reference draws the unset start with rand:uniform/1.
 *   EMQX_GM_SHARE_STICKY (:234-247): st[s] while set, else members[mix(seed, s)
 *     rem Count], which is stored (also for Count = 1, as :245 does).
 *     Deviation: the reference keeps a sticky pid while its PROCESS is alive,
 *     even after it unsubscribed (:236, is_active_sub); the table knows
 *     membership, not liveness, so a member that left the list loses
 *     stickiness at the next build.
 *   EMQX_GM_SHARE_RANDOM (:270-271): members[mix3(seed, row, s) rem Count]:
 *     counter based and stateless, equal arguments give equal picks (any
 *     in-range choice is a valid outcome of rand:uniform/1).
 *   Count = 1 picks that member; hash, round_robin and random read and write
 *   no state then (pick_subscriber/6, first clause, :265).
 * FailedSubs, the ack / nack retry loop of dispatch/4 (:118-130) and {error,
 * no_subscribers} stay with the caller, which reads a slot's member list with
 * emqx_gm_shared_slot.  A slot without members does not exist (the reference
 * deletes the route). */
typedef struct emqx_gm_shared emqx_gm_shared;
#define EMQX_GM_SHARE_HASH 0u
#define EMQX_GM_SHARE_ROUND_ROBIN 1u
#define EMQX_GM_SHARE_STICKY 2u
#define EMQX_GM_SHARE_RANDOM 3u
typedef struct {
  uint64_t n_slots;              /* {Group, Filter} pairs with members               */
  uint64_t n_members;            /* member entries over all slots                    */
  uint64_t n_filters_with_slots; /* distinct filters that carry a slot               */
  uint64_t device_bytes;         /* resident table bytes in HBM (0: host-only table) */
} emqx_gm_shared_info_t;
/* The emqx_shared_subscription table (emqx_shared_sub.erl:287-288) bound to ONE
 * plain snapshot `idx`, which it retains.  Input slot i is filter
 * filter_bytes[filter_off[i] .. filter_off[i+1]) -- it must be a filter of the
 * snapshot, else EMQX_GM_EINVAL with the filter named in emqx_gm_last_error --
 * with the caller's group id group_ids[i] and members mem_ids[mem_off[i] ..
 * mem_off[i+1]), ids in the same space as emqx_gm_index_build's subscriber ids
 * (2^32 - 1 is reserved).  Slots are sorted by (filter id, group id); inputs
 * with equal (filter, group) are merged in input order; a member listed twice
 * is kept once, at its first place; empty slots are dropped.  prev (optional,
 * not modified): rr / st are carried over for every slot whose (filter bytes,
 * group id) exists in both -- filter ids shift between snapshots -- st only if
 * that member is still listed.  flags: 0.  Sharded, shard and overlay
 * snapshots: EMQX_GM_EUNSUPPORTED.  Offsets are checked as
 * emqx_gm_retained_build checks them.  On a multi-device context the table
 * lives on the first listed device. */
int emqx_gm_shared_build(emqx_gm_ctx *ctx, emqx_gm_index *idx, const uint8_t *filter_bytes,
                         const uint64_t *filter_off, const uint32_t *group_ids, uint64_t n_slots,
                         const uint64_t *mem_off, const uint32_t *mem_ids, const emqx_gm_shared *prev,
                         uint32_t flags, emqx_gm_shared **out);
/* emqx_shared_sub:pick/6 (:234-288) for every hit of `matches`, rows of the
 * bound snapshot as emqx_gm_match returns them: a host CSR, or a device CSR
 * (on_device; msg_hash is then a device pointer too).  The results come back on
 * the same side, with identical row_off and one entry per hit in batch order:
 * out_members->ids the picked member, out_slots->ids the slot (free both with
 * emqx_gm_csr_free).  msg_hash (n_rows entries) is required for
 * EMQX_GM_SHARE_HASH and ignored otherwise.  Host rows are checked before any
 * device work (n_rows < 2^32 - 1, row_off from 0 to nnz ascending, every id <
 * n_filters: else EMQX_GM_EINVAL); for device rows the kernels skip an id >=
 * n_filters and clamp an offset past nnz.  2^32 - 1 hits or more in one call:
 * EMQX_GM_EOVERFLOW (no state changed).  Calls on one table are serialized
 * and its state changes in stream order. */
int emqx_gm_shared_pick(emqx_gm_ctx *ctx, emqx_gm_shared *sh, const emqx_gm_csr *matches, uint32_t strategy,
                        const uint32_t *msg_hash, uint32_t seed, emqx_gm_csr *out_members,
                        emqx_gm_csr *out_slots);
/* subscribers(Group, Topic) of slot `slot` (:287-288; host memory owned by the
 * table) for the caller's FailedSubs loop (dispatch/4, :118-130), and the
 * slot's filter id in the bound snapshot and group id.  Any out pointer may be
 * NULL. */
int emqx_gm_shared_slot(const emqx_gm_shared *sh, uint32_t slot, uint32_t *filter_id, uint32_t *group_id,
                        const uint32_t **members, uint64_t *n_members);
int emqx_gm_shared_info(const emqx_gm_shared *sh, emqx_gm_shared_info_t *info);
/* drops the table and its reference on the snapshot */
int emqx_gm_shared_release(emqx_gm_shared *sh);

/* ---- cluster forwards (gm_dests.cpp / gm_dests.hip): a window's remote routes, one list per node ----
 * A filter whose destination is another node comes back from a match as a route
 * mark only; the reference then reads the emqx_route bag per matched filter
 * (lookup_routes/1, apps/emqx/src/emqx_router.erl:136) and calls forward/3 once
 * per (message, route) (route/2, do_route/2, aggre/1, apps/emqx/src/
 * emqx_broker.erl:214, 245-293).  Here the NODE destinations of emqx_route live
 * in HBM and one call turns a publish window's matched rows into one forward
 * list per node, so the caller sends one RPC per node per window.  Group
 * destinations ({Group, Node}) stay with the shared-subscription table, whose
 * slots are aggre/1's deduplicated {To, Group} entries.
 * TABLE: a set of (filter, node) routes bound to ONE plain snapshot; node is a
 * caller-assigned dense id < n_nodes, 1 <= n_nodes <= EMQX_GM_DESTS_MAX_NODES
 * (the cap bounds the per-chunk histogram of the partition: one workgroup keeps
 * a whole node histogram in 16 KiB of LDS).  A pair given twice is stored once
 * (do_add_route/2 checks lists:member, emqx_router.erl:112-116); a filter's
 * nodes are stored ascending.  The table is immutable: a changed route set or a
 * new snapshot (filter ids shift) means a new build.
 * HIT: a (window row, matched filter id, node of that filter) triple with
 * node != skip_node.  The caller passes its own node id as skip_node (the local
 * dispatch is the fan-out's job); EMQX_GM_DESTS_NO_SKIP skips nothing.
 * BATCH ORDER: rows ascending, then filter ids in the order the row holds them,
 * then nodes ascending.
 * RESULT (emqx_gm_forwards): node k's forwards are the entries [node_off[k],
 * node_off[k + 1]) of rows / filters, IN BATCH ORDER: emqx_rpc keys its channel
 * by topic, so the forwards of one filter to one node must arrive in publish
 * order (a stable partition keeps it; an arrival-order ticket would not).
 * row_routes[r] is the number of {To, Node} routes of row r, skip_node's
 * included (saturating at 2^32 - 1): a row with 0 here and no shared slot is
 * route([], _), the dropped / no_subscribers case (emqx_broker.erl:245-248).
 * EQUIVALENCE: run, per message in window order, match_routes/1 over the row
 * (emqx_router.erl:128-134), lookup_routes/1 over the bag, aggre/1 clause by
 * clause (its lists:usort on meeting a group route included: node entries are
 * distinct terms and never equal a group entry, so every one survives it) and
 * route/2 with node() = skip_node, recording every forward(Node, To, Delivery):
 * per node, the recorded (row, To) sequence equals the plan's list -- rows in
 * window order; within one row as a set (the reference's order inside one
 * message follows the trie's match order). */
typedef struct emqx_gm_dests emqx_gm_dests;
#define EMQX_GM_DESTS_MAX_NODES 4096u
#define EMQX_GM_DESTS_NO_SKIP 0xFFFFFFFFu
#define EMQX_GM_DESTS_SKIP_UNKNOWN 0x1u /* build flag: drop (and count) routes of filters not in the snapshot */
typedef struct {
  uint64_t n_routes;              /* distinct (filter, node) pairs stored                          */
  uint64_t n_filters_with_routes; /* distinct filters that carry a route                           */
  uint64_t n_skipped_unknown;     /* input routes dropped under EMQX_GM_DESTS_SKIP_UNKNOWN          */
  uint64_t device_bytes;          /* resident table bytes in HBM (0: host-only table)              */
  uint32_t n_nodes;
  uint32_t reserved0;
} emqx_gm_dests_info_t;
typedef struct {
  uint64_t n_rows;      /* rows of the window                                     */
  uint64_t n_pairs;     /* hits = entries of rows / filters (< 2^32 - 1)          */
  uint64_t *node_off;   /* [n_nodes + 1]                                          */
  uint32_t *rows;       /* [n_pairs] window row of each forward                   */
  uint32_t *filters;    /* [n_pairs] its filter id (the forward's To)             */
  uint32_t *row_routes; /* [n_rows] node routes of the row, skip_node's included  */
  uint32_t n_nodes;
  int32_t on_device;    /* the arrays are device pointers                         */
  void *priv;           /* the owning context (NULL: malloc'ed by the host walk)  */
} emqx_gm_forwards;
/* The node routes of emqx_route bound to ONE plain snapshot `idx`, which the
 * table retains.  Route i is filter filter_bytes[filter_off[i] ..
 * filter_off[i+1]) -> node_ids[i].  A filter that is not in the snapshot:
 * EMQX_GM_EINVAL with the filter named in emqx_gm_last_error, or, with
 * EMQX_GM_DESTS_SKIP_UNKNOWN, dropped and counted.  node_ids[i] >= n_nodes,
 * n_nodes outside [1, EMQX_GM_DESTS_MAX_NODES], an unknown flag and bad
 * offsets (checked as emqx_gm_retained_build checks them): EMQX_GM_EINVAL
 * before any device work.  Sharded, shard and overlay snapshots:
 * EMQX_GM_EUNSUPPORTED.  On a multi-device context the table lives on the
 * first listed device. */
int emqx_gm_dests_build(emqx_gm_ctx *ctx, emqx_gm_index *idx, const uint8_t *filter_bytes,
                        const uint64_t *filter_off, const uint32_t *node_ids, uint64_t n_routes,
                        uint32_t n_nodes, uint32_t flags, emqx_gm_dests **out);
/* The forward plan of `matches`, rows of the bound snapshot as emqx_gm_match
 * returns them: a host CSR, or a device CSR (on_device).  The result comes
 * back on the same side (free it with emqx_gm_forwards_free).  Host rows are
 * checked before any device work (n_rows < 2^32 - 1, row_off from 0 to nnz
 * ascending, every id < n_filters: else EMQX_GM_EINVAL); for device rows the
 * kernels skip an id >= n_filters and clamp an offset past nnz.  skip_node >=
 * n_nodes other than EMQX_GM_DESTS_NO_SKIP skips nothing either.  2^32 - 1
 * hits or more in one call: EMQX_GM_EOVERFLOW, detected after the counting
 * pass, before any output is sized; nothing is returned.  The result does not
 * depend on how the library cuts the hits into chunks. */
int emqx_gm_forward_plan(emqx_gm_ctx *ctx, emqx_gm_dests *dt, const emqx_gm_csr *matches, uint32_t skip_node,
                         emqx_gm_forwards *out);
/* frees a plan (ctx may be NULL for a result of emqx_gm_forward_plan_host) */
int emqx_gm_forwards_free(emqx_gm_ctx *ctx, emqx_gm_forwards *fw);
int emqx_gm_dests_info(const emqx_gm_dests *dt, emqx_gm_dests_info_t *info);
/* drops the table and its reference on the snapshot */
int emqx_gm_dests_release(emqx_gm_dests *dt);

/* ---- subscription options at dispatch (gm_subopts.cpp / gm_subopts.hip): one option byte per delivery ----
 * A delivery {deliver, Filter, Msg} is not yet what the subscriber gets: the
 * reference passes it through the subscription's options, keyed by (Filter,
 * Subscriber) -- emqx_session:ignore_local/4 (apps/emqx/src/emqx_session.erl:
 * 279-291, from emqx_channel:handle_deliver/2, emqx_channel.erl:806-842) drops a
 * delivery whose subscription has nl = 1 when the subscriber is the publisher,
 * and enrich_deliver/2 -> get_subopts/2 -> enrich_subopts/3 (emqx_session.erl:
 * 560-602) sets the nl flag, the effective QoS and the retain flag.  Here the
 * options of emqx_broker:subscribe/3 (emqx_broker.erl:126-145) live in HBM,
 * one byte beside every subscriber id of the snapshot, and emqx_gm_deliver
 * turns a window's matched rows into deliveries with one option byte each.
 * TABLE: bound to ONE plain snapshot built with subscriber lists, which the
 * table retains.  Immutable, as emqx_gm_dests is: a new snapshot or a changed
 * option means a new build; following emqx_gm_index_update_subs incrementally
 * is out of scope.
 * OPT BYTE (input): bits 0-1 the subscription QoS (3: EMQX_GM_EINVAL), bit 2 nl,
 * bit 3 rap, bit 4 the subscriber session's upgrade_qos, bits 5-7 zero (else
 * EMQX_GM_EINVAL).  rh is not carried (it belongs to the subscribe-time retained
 * dispatch), nor is subid (the Subscription-Identifier stays with the session).
 * A pair of the snapshot without an entry gets the build's default_opt
 * (?DEFAULT_SUBOPTS, include/emqx_mqtt.hrl:193-197, is 0).
 * MESSAGE FLAGS (msg_flags[r], per row): bits 0-1 the publish QoS (3:
 * EMQX_GM_EINVAL), bit 2 the retain flag, bit 3 headers.retained =:= true, bits
 * 4-7 zero (else EMQX_GM_EINVAL).  msg_from[r]: the publisher's subscriber id,
 * or EMQX_GM_SO_NO_PUBLISHER.
 * DELIVERY BYTE (dopt[k], beside deliveries.ids[k]): bits 0-1 the effective QoS
 * (min(SubQoS, PubQoS), max under upgrade_qos), bit 2 the retain flag (cleared
 * unless rap = 1 or headers.retained), bit 3 the nl message flag ({nl, 1}), bit 4
 * the No-Local hit (EMQX_GM_SO_FLAG only).
 * NO LOCAL: the reference applies lists:dropwhile over whatever batch a channel
 * drained from its mailbox (emqx_session.erl:281): it drops only the LEADING
 * run of hits.  Batch boundaries are mailbox timing no window can know, so
 * emqx_gm_deliver evaluates the predicate per delivery (emqx_gm_deliver_batches
 * below delivers the window as ONE batch per subscriber and applies dropwhile
 * itself: EMQX_GM_SO_LEAD).  EMQX_GM_SO_FLAG removes
 * nothing and marks (bit 4) every delivery for which ignore_local's fun returns
 * true: a session has all it needs to reproduce dropwhile bit for bit.
 * EMQX_GM_SO_DROP removes those deliveries (the order otherwise kept) and counts
 * them per row (row_dropped: the delivery.dropped.no_local metric): MQTT 5
 * section 3.8.3.1 applied to every delivery, equal to the reference whenever a
 * subscriber's hits lead its batch.
 * EQUIVALENCE: for row r with message M, over each matched filter F in the row's
 * order and each subscriber S of F in list order: the delivery's hit is
 * opts(F, S).nl == 1 andalso S =:= from(M); its byte is enrich_subopts([{nl, _},
 * {qos, _}, {rap, _}], M, #session{upgrade_qos}) clause by clause. */
typedef struct emqx_gm_subopts emqx_gm_subopts;
#define EMQX_GM_SO_SKIP_UNKNOWN 0x1u       /* build flag: drop (and count) entries whose pair is not in the snapshot */
#define EMQX_GM_SO_NO_PUBLISHER 0xFFFFFFFFu
#define EMQX_GM_SO_FLAG 0u /* emqx_gm_deliver mode: mark No-Local hits (bit 4), remove nothing */
#define EMQX_GM_SO_DROP 1u /* ... remove them, count them per row                             */
typedef struct {
  uint64_t n_entries;         /* input entries stored (distinct pairs)                        */
  uint64_t n_defaulted;       /* pairs of the snapshot without an entry (default_opt)         */
  uint64_t n_nl;              /* pairs with nl = 1                                            */
  uint64_t n_skipped_unknown; /* input entries dropped under EMQX_GM_SO_SKIP_UNKNOWN          */
  uint64_t device_bytes;      /* resident table bytes in HBM (0: host-only table)             */
} emqx_gm_subopts_info_t;
typedef struct {
  emqx_gm_csr deliveries; /* row r's subscriber ids, as emqx_gm_fanout (minus the dropped)    */
  uint8_t *dopt;          /* [deliveries.nnz] the delivery bytes                              */
  uint32_t *row_dropped;  /* [n_rows] EMQX_GM_SO_DROP: the row's removed deliveries; else NULL */
  uint64_t n_dropped;     /* their sum                                                        */
} emqx_gm_deliveries;
/* Entry i is (filter filter_bytes[filter_off[i] .. filter_off[i+1]), sub_ids[i],
 * opts[i]).  An entry whose filter is not in the snapshot, or whose subscriber
 * is not in that filter's list: EMQX_GM_EINVAL naming it, or, with
 * EMQX_GM_SO_SKIP_UNKNOWN, dropped and counted.  A pair given twice with
 * different bytes, a bad opt byte (default_opt too), an unknown flag, bad
 * offsets: EMQX_GM_EINVAL.  A filter whose list holds one subscriber twice
 * (built from duplicate input filters) while that pair has nl = 1:
 * EMQX_GM_EUNSUPPORTED (the reference's bag holds a pair once; the hot path
 * relies on at most one hit per filter).  Sharded, shard and overlay snapshots,
 * and an index without subscriber lists: EMQX_GM_EUNSUPPORTED.  The build reads
 * the lists back once and is O(entries + n_subs) (expected; plus a sort of each
 * filter's nl pairs): no list is scanned per entry.  On a multi-device context
 * the table lives on the first listed device. */
int emqx_gm_subopts_build(emqx_gm_ctx *ctx, emqx_gm_index *idx, const uint8_t *filter_bytes,
                          const uint64_t *filter_off, const uint32_t *sub_ids, const uint8_t *opts,
                          uint64_t n_entries, uint8_t default_opt, uint32_t flags, emqx_gm_subopts **out);
/* The deliveries of `matches`, rows of the bound snapshot: a host CSR, or a
 * device CSR (on_device); msg_flags / msg_from (n_rows entries each) live on the
 * side the rows live on and the result comes back on that side (free it with
 * emqx_gm_deliveries_free).  A NULL argument, an unknown mode, n_rows >= 2^32 - 1,
 * and for host inputs a non-monotone row_off, an id >= n_filters or a bad
 * msg_flags byte: EMQX_GM_EINVAL before any device work, no output touched.  For
 * device rows the kernels skip an id >= n_filters, clamp an offset past nnz and
 * mask msg_flags to its low 4 bits.  The rows must be rows of the table's bound
 * snapshot (emqx_gm_subopts_index names it): a CSR does not record its snapshot,
 * so the callers that know it -- the Python binding and the NIF -- compare the
 * two and refuse another snapshot's rows with EMQX_GM_EINVAL before this call.
 * In EMQX_GM_SO_FLAG mode `deliveries` is bit-equal to emqx_gm_fanout of the
 * same rows. */
int emqx_gm_deliver(emqx_gm_ctx *ctx, emqx_gm_subopts *so, const emqx_gm_csr *matches, const uint8_t *msg_flags,
                    const uint32_t *msg_from, uint32_t mode, emqx_gm_deliveries *out);
/* the bound snapshot (NULL: a host-only table); not retained for the caller */
const emqx_gm_index *emqx_gm_subopts_index(const emqx_gm_subopts *so);
/* frees a result (ctx may be NULL for a result of emqx_gm_deliver_host) */
int emqx_gm_deliveries_free(emqx_gm_ctx *ctx, emqx_gm_deliveries *d);
int emqx_gm_subopts_info(const emqx_gm_subopts *so, emqx_gm_subopts_info_t *info);
/* drops the table and its reference on the snapshot */
int emqx_gm_subopts_release(emqx_gm_subopts *so);

/* SESSION BATCHES (gm_batches.hip): the same deliveries ordered by SUBSCRIBER.
 * In the reference every subscriber's connection process drains all
 * {deliver, Filter, Msg} of its mailbox into one list (emqx_connection.erl:
 * 516-520, emqx_misc:drain_deliver/1, emqx_misc.erl:159-173) and hands it to
 * emqx_channel:handle_deliver/2 (emqx_channel.erl:830-842), which runs
 * emqx_session:ignore_local/4 (emqx_session.erl:279-291) over the list and
 * enriches what remains.  emqx_gm_deliver_batches gives a window as those lists.
 * Number the window's deliveries k = 0, 1, ... in the order emqx_gm_deliver
 * emits them in EMQX_GM_SO_FLAG mode (rows ascending, a row's filters in row
 * order, a filter's subscribers in list order).  Subscriber S's BATCH is the
 * deliveries with subscriber S in ascending k -- the order in which one
 * dispatching process's sends reach S's mailbox; a subscriber under two
 * filters of one row appears twice, adjacent, in the row's filter order.
 * Batches are listed by ascending subscriber id; a subscriber is listed when
 * it has a delivery BEFORE any removal.  Batch j is subs[j] with entries
 * [batch_off[j], batch_off[j + 1]) of rows / filters / dopt: the window row,
 * the filter id (the deliver's Topic) and the delivery byte.
 * MODES: EMQX_GM_SO_FLAG removes nothing (bit 4 marks a hit); EMQX_GM_SO_DROP
 * removes every hit (emqx_gm_deliver's rule); EMQX_GM_SO_LEAD -- valid for this
 * call only -- removes from each batch exactly its LEADING run of hits and
 * clears bit 4 in what it keeps: the window delivered as one batch per
 * subscriber is a batch the library does know, and the result is bit-equal to
 * ignore_local/4 followed by enrich_deliver/2 over it.  A batch emptied by
 * removal stays listed (equal offsets) with its count in batch_dropped (the
 * delivery.dropped.no_local metric).
 * Inputs and refusals as emqx_gm_deliver's (host inputs fully checked before
 * any device work; device rows skipped / clamped / masked); the result lives on
 * the rows' side.  2^32 - 1 deliveries or more before removal:
 * EMQX_GM_EOVERFLOW, decided by the counting pass before any output is sized.
 * A failing call leaves `out` untouched.  An empty window, all-empty rows or a
 * table without subscribers: a valid result with zero batches.  The result is
 * deterministic.  The table lives on the first listed device of a multi-device
 * context and the call runs there. */
#define EMQX_GM_SO_LEAD 2u /* emqx_gm_deliver_batches only: remove each batch's leading run of hits */
typedef struct {
  uint64_t n_rows, n_deliveries /* kept, < 2^32 - 1 */, n_batches, n_dropped;
  uint32_t *subs;          /* [n_batches] ascending, distinct                    */
  uint64_t *batch_off;     /* [n_batches + 1]                                    */
  uint32_t *rows;          /* [n_deliveries] window row                          */
  uint32_t *filters;       /* [n_deliveries] filter id: the deliver's Topic      */
  uint8_t  *dopt;          /* [n_deliveries] delivery byte                       */
  uint32_t *batch_dropped; /* [n_batches] removed from the batch; NULL in FLAG   */
  int32_t on_device; void *priv;
} emqx_gm_batches;
int emqx_gm_deliver_batches(emqx_gm_ctx *ctx, emqx_gm_subopts *so, const emqx_gm_csr *matches,
                            const uint8_t *msg_flags, const uint32_t *msg_from, uint32_t mode,
                            emqx_gm_batches *out);
/* frees a result (ctx may be NULL for a result of emqx_gm_deliver_batches_host) */
int emqx_gm_batches_free(emqx_gm_ctx *ctx, emqx_gm_batches *b);

/* ---- a whole publish window in one device round trip (gm_publish.hip) ----
 * A broker node's unit of work is a publish window, and for every message of
 * it the node needs the matched route filters, their local subscribers, one
 * member per matched shared group and the remote nodes to forward to
 * (emqx_broker:publish/1 .. route/2, apps/emqx/src/emqx_broker.erl:204-215,
 * 245-293; emqx_shared_sub:dispatch/3).  emqx_gm_publish_window computes all
 * four in ONE call: the picks and the plan are queued on the device behind the
 * match's speculative rows and fan-out, before the call's one host-blocking
 * wait, and one kernel copies every side result to page-locked host memory.
 * CONTRACT: the result is bit-equal to, on the same tables and in this order,
 *   emqx_gm_match_fanout(topics, flags), emqx_gm_shared_pick on the returned
 *   host rows with (strategy, msg_hash, seed), emqx_gm_forward_plan on the same
 *   rows with skip_node -- every array, n_pairs, and the shared table's
 *   round-robin / sticky state afterwards.
 * Every array is a host pointer from the context's host pool; free the result
 * with emqx_gm_publish_result_free, or each member on its own with
 * emqx_gm_csr_free / emqx_gm_forwards_free.  With both tables NULL the call is
 * emqx_gm_match_fanout.
 * SPECULATION: the picks run into a capacity of hits, the plan into a capacity
 * of pairs (this context's recent hits / pairs per match x 1.25, a power of
 * two, at least 1024); the shared table's state is not written until the host
 * has seen that the run holds (a small kernel then commits it, without a wait).
 * What did not hold runs again at its exact size on the rows still in HBM:
 * both side results when the rows were not the speculative ones, only the
 * picks (the plan) when the hits (pairs) passed their capacity; deliveries
 * past theirs follow emqx_gm_match_fanout's rule.  emqx_gm_publish_stats says
 * which part came from the first round trip.
 * A window emqx_gm_match_fanout would not serve in one round trip (more than
 * one host chunk, an overlay or sharded snapshot, an index without subscriber
 * lists) takes the three calls in sequence: correct, with more waits
 * (device_waits is then 0: not counted).  On a multi-device context the window
 * runs whole on the first listed device, which holds the side tables.
 * ERRORS: a NULL argument, unknown flags, non-monotone offsets, a strategy past
 * EMQX_GM_SHARE_RANDOM, EMQX_GM_SHARE_HASH without msg_hash, a table bound to a
 * snapshot other than idx or living on another device: EMQX_GM_EINVAL (a
 * host-only table: EMQX_GM_EUNSUPPORTED) before any device work, no output
 * touched, no state changed.  On any later error every output is zeroed and
 * nothing is held; the shared state is unchanged unless the error is the
 * deliveries' rerun failing after the picks were committed.
 * THREADS: windows with a stateful strategy (round robin, sticky) on one table
 * are serialised from queueing to commit; hash and random windows overlap. */
typedef struct {
  uint32_t flags;            /* EMQX_GM_WITH_EXACT or 0, as emqx_gm_match_fanout           */
  emqx_gm_shared *shared;    /* NULL: no picks                                             */
  uint32_t strategy, seed;   /* as emqx_gm_shared_pick                                     */
  const uint32_t *msg_hash;  /* host, n_topics entries; required for EMQX_GM_SHARE_HASH    */
  emqx_gm_dests *dests;      /* NULL: no forward plan                                      */
  uint32_t skip_node;        /* as emqx_gm_forward_plan                                    */
  uint64_t reserved[2];
} emqx_gm_publish_opts;
typedef struct {
  emqx_gm_csr matches, deliveries;      /* as emqx_gm_match_fanout                          */
  emqx_gm_csr pick_members, pick_slots; /* as emqx_gm_shared_pick on host rows (zeroed without `shared`) */
  emqx_gm_forwards forwards;            /* as emqx_gm_forward_plan on host rows (zeroed without `dests`) */
} emqx_gm_publish_result;
typedef struct {
  uint32_t device_waits;   /* host-blocking waits on the device made by this call          */
  uint8_t rows_spec, fanout_spec, picks_spec, forwards_spec; /* 1: that part came from the first round trip */
  uint64_t n_hits, n_pairs;       /* shared hits, forward pairs                            */
  uint64_t cap_hits, cap_pairs;   /* the speculative capacities used (0: not speculated)   */
} emqx_gm_publish_stats;
int emqx_gm_publish_window(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                           const uint64_t *topic_off, uint64_t n_topics, const emqx_gm_publish_opts *opts,
                           emqx_gm_publish_result *out, emqx_gm_publish_stats *stats /* may be NULL */);
/* frees every member of a result and zeroes it */
int emqx_gm_publish_result_free(emqx_gm_ctx *ctx, emqx_gm_publish_result *res);

/* ---- a publish window whose deliveries carry their option bytes ----
 * A window's local deliveries are not finished until each one has its
 * delivery byte (emqx_gm_deliver above).  emqx_gm_publish_window_deliver queues
 * that work as a THIRD speculative part behind the window's rows, beside the
 * picks and the plan and in place of the plain fan-out (in EMQX_GM_SO_FLAG mode
 * the ids are the fan-out's), so the window still needs one wait in total.
 * CONTRACT: on the same tables the result is bit-equal to
 *   emqx_gm_publish_window(opts) followed by emqx_gm_deliver(subopts,
 *   &out->matches, msg_flags, msg_from, mode):
 * out->matches, pick_members, pick_slots, forwards and the shared table's
 * state afterwards are the window call's; out->deliveries is zeroed; `deliv` is
 * the deliver call's, array for array (deliveries.row_off, deliveries.ids,
 * dopt, row_dropped -- NULL in FLAG mode -- and n_dropped).  deliv's arrays are
 * host pointers from the context's host pool: free them with
 * emqx_gm_deliveries_free.
 * SPECULATION: the deliveries run into the fan-out's own capacity (this
 * context's recent deliveries per match; GM_PW_CAP_DELIVERIES gives it as it
 * is, 0: not speculated).  They hold if the rows were the speculative ones and
 * the (post-drop) total fits; else they run again at exact size on the rows
 * still in HBM, before the picks are committed.
 * A window emqx_gm_publish_window would not serve in one round trip takes
 * emqx_gm_match, the pick, the plan and emqx_gm_deliver in sequence
 * (device_waits is then 0: not counted).
 * ERRORS: every refusal of emqx_gm_publish_window; a NULL dopts, deliv or
 * subopts, NULL msg_flags / msg_from with n_topics > 0, an unknown mode, a
 * msg_flags byte with bits 4-7 set or QoS 3, a table on another device or bound
 * to a snapshot other than idx: EMQX_GM_EINVAL (a host-only table:
 * EMQX_GM_EUNSUPPORTED) -- all before any device work, no output touched, no
 * state changed.  On any later error every output is zeroed, nothing is held
 * and the shared state is unchanged. */
typedef struct {
  emqx_gm_subopts *subopts;  /* required; bound to idx, on the window's device        */
  const uint8_t *msg_flags;  /* host, n_topics entries, as emqx_gm_deliver             */
  const uint32_t *msg_from;  /* host, n_topics entries (EMQX_GM_SO_NO_PUBLISHER: none) */
  uint32_t mode;             /* EMQX_GM_SO_FLAG / EMQX_GM_SO_DROP                      */
} emqx_gm_publish_deliver_opts;
typedef struct {
  emqx_gm_publish_stats window;  /* fanout_spec stays 0: no plain fan-out is made */
  uint8_t deliveries_spec;       /* 1: the deliveries came from the first round trip */
  uint64_t n_deliveries, n_dropped, cap_deliveries; /* cap 0: not speculated */
} emqx_gm_publish_deliver_stats;
int emqx_gm_publish_window_deliver(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                                   const uint64_t *topic_off, uint64_t n_topics, const emqx_gm_publish_opts *opts,
                                   const emqx_gm_publish_deliver_opts *dopts, emqx_gm_publish_result *out,
                                   emqx_gm_deliveries *deliv, emqx_gm_publish_deliver_stats *stats /* may be NULL */);

/* ---- whole publish windows coalesced into one device round trip (gm_publish.hip) ----
 * Every scheduler of a node runs emqx_broker:publish/1 -> route/2 per message
 * at once (apps/emqx/src/emqx_broker.erl:204-215, 245-293, 296-322;
 * emqx_shared_sub:dispatch/3, emqx_shared_sub.erl:113-130), so a node has many
 * small windows in flight, each needing rows, deliveries, picks and forwards.
 * emqx_gm_publish_windows runs a GROUP of them as one match, one fan-out, one
 * pick stage and one plan stage over the group's rows, and cuts every result
 * back into the windows' own, with ONE host-blocking wait per held group and
 * the shared table's lock taken once per group.
 * CONTRACT: out[k] is bit-equal to what emqx_gm_publish_window returns for
 * window k when the windows are run one after another, in order, on the same
 * tables with the same (flags, shared, strategy, seed, dests, skip_node) --
 * every array, n_pairs, row_routes, and the shared table's round-robin / sticky
 * state afterwards.  Round robin: the concatenated rows' hits take consecutive
 * ranks per slot; sticky: every hit of a slot computes the same first member;
 * hash: the windows' msg_hash arrays are concatenated in window order; random
 * mixes a message's row in its OWN window (the kernel subtracts the window's
 * first row); a node's forwards of a window are one contiguous run of the
 * node's group list, cut at a lower bound on the row.  Each out[k] is freed on
 * its own with emqx_gm_publish_result_free, from any thread.
 * GROUPS as emqx_gm_match_windows: at most 64 windows, one chunk of topics and
 * 1 MiB of text (the hashes travel beside the text and do not count); more
 * windows run as groups one after another, state carried from group to group.
 * A window a group cannot hold (an overlay or sharded snapshot, an index
 * without subscriber lists, a topic past 65,535 B, more than 1 MiB of text)
 * runs alone through emqx_gm_publish_window, in its place.  A group runs on
 * the first listed device, which holds the side tables.  With both tables NULL
 * the call is emqx_gm_match_windows with deliveries.
 * FALLBACKS, each visible in the stats: a group whose rows were not the
 * speculative ones, or whose hits (pairs) pass the GROUP's capacity, has that
 * side result run again at its exact size on the true device rows (a second
 * round trip) and cut on the host; a window past its OWN capacity while the
 * group held gets a result of exact size and its cut again, the others pay
 * nothing; deliveries follow emqx_gm_match_windows' rule.  The plan is settled
 * before the picks and the commit of the shared state comes last.
 * ERRORS: a NULL argument, unknown flags, non-monotone offsets in any window, a
 * strategy out of range, EMQX_GM_SHARE_HASH with a window lacking msg_hash,
 * opts->msg_hash non-NULL, a table bound elsewhere: EMQX_GM_EINVAL /
 * EMQX_GM_EUNSUPPORTED before any device work, no output touched, no state
 * changed.  On a later error every output is zeroed and nothing is held.
 *
 * emqx_gm_combiner_publish: emqx_gm_publish_window through a combiner.  Publish
 * windows group only with publish windows of the same (index, flags, shared,
 * strategy, seed, dests, skip_node); a caller's bad window fails that call
 * alone.  Stateful strategies make the order of the groups observable, so it is
 * reported: `where` carries the combiner's group sequence number and the
 * window's position in its group, and groups with a stateful strategy are
 * serialised in sequence order.  Replaying all windows through
 * emqx_gm_publish_window in (seq, position) order gives the same results and
 * the same final state. */
typedef struct {
  emqx_gm_window w;
  const uint32_t *msg_hash; /* host, w.n_topics entries; required for EMQX_GM_SHARE_HASH */
} emqx_gm_publish_win;
typedef struct {
  uint64_t seq;           /* the group's sequence number: per combiner, or per call (from 0)     */
  uint32_t position;      /* the window's place in its group                                     */
  uint32_t n_windows;     /* windows of the group (1: also a window that ran alone)              */
  uint32_t device_waits;  /* host-blocking waits the whole group made (0: alone, not counted)    */
  uint8_t grouped;        /* 1: run by the group stage; 0: alone through emqx_gm_publish_window  */
  uint8_t rows_spec, picks_spec, forwards_spec; /* 1: the GROUP's part came from the first round trip */
  uint8_t window_picks_exact, window_forwards_exact; /* 1: the group held, this window passed its own capacity */
  uint8_t reserved8[6];
  uint64_t cap_hits, cap_pairs; /* the group's speculative capacities (0: not speculated)        */
  uint64_t n_hits, n_pairs;     /* the group's hits and pairs                                    */
} emqx_gm_publish_group_stats;
int emqx_gm_publish_windows(emqx_gm_ctx *ctx, const emqx_gm_index *idx, const emqx_gm_publish_win *windows,
                            uint32_t n_windows, const emqx_gm_publish_opts *opts /* msg_hash must be NULL */,
                            emqx_gm_publish_result *out /* [n_windows] */,
                            emqx_gm_publish_stats *stats /* [n_windows] or NULL */,
                            emqx_gm_publish_group_stats *gstats /* [n_windows] or NULL */);
int emqx_gm_combiner_publish(emqx_gm_combiner *cb, const emqx_gm_index *idx, const uint8_t *topic_bytes,
                             const uint64_t *topic_off, uint64_t n_topics, const emqx_gm_publish_opts *opts,
                             emqx_gm_publish_result *out, emqx_gm_publish_stats *stats /* may be NULL */,
                             emqx_gm_publish_group_stats *where /* may be NULL */);

/* ---- authorization check (gm_authz.cpp / gm_authz.hip): the first matching ACL rule per request ----
 * Every PUBLISH and SUBSCRIBE passes emqx_authz:authorize/5 before the router;
 * the reference scans its rule lists per packet (emqx_authz:do_authorize/4,
 * apps/emqx_authz/src/emqx_authz.erl:307-317; the file source,
 * emqx_authz_rule:matches/4, emqx_authz_rule.erl:110-125; the built-in database,
 * emqx_authz_mnesia:authorize/4, emqx_authz_mnesia.erl:95-111, 212-218).  Here
 * the chain of file and built-in-database sources is compiled once into one table
 * in HBM and a window of requests (clientinfo, action, topic) is answered in
 * one device call, bit-equal to do_authorize/4 over that chain.
 * The table is an ordered list of SEGMENTS; a request's evaluation order is the
 * concatenation, in segment order, of the one rule range each segment yields
 * for that client: a GLOBAL segment's one range for every client (a file
 * source; the built-in database's `all` record), a BY_CLIENTID / BY_USERNAME
 * segment's range under the request's own clientid / username (the keyed
 * records; an undefined or absent key yields no rule).  [file,
 * built_in_database] is GLOBAL, BY_CLIENTID, BY_USERNAME, GLOBAL.
 * A RULE is {permission, who, action, topic filters} (emqx_authz_rule.erl:49)
 * and the caller's u32 id.  match/4 (:119-125) = match_action/2 (:127-130) and
 * match_who/2 (:132-165) and match_topics/3 (:167-180):
 *   who: AND or OR over leaves (all = AND of none; the foldl identities make
 *     AND [] true and OR [] false).  Leaves: username / clientid equal to given
 *     bytes (an undefined username or clientid matches none); ipaddr / ipaddrs:
 *     CIDRs as esockd_cidr:parse/2 compiles them, a family and an inclusive
 *     [lo, hi] -- the families equal and lo <= peerhost <= hi, an undefined
 *     peerhost matches none; regex k (k < 32): bit k of the request's re_mask --
 *     the library runs no regex, the caller evaluates the table's at most 32
 *     distinct {re, _} predicates once per client.  A nested and / or and a 33rd
 *     regex are refused (EMQX_GM_EUNSUPPORTED).
 *   topic filters (compile_topic/1, :82-91): any filter matching is enough, a
 *     rule without filters never matches.  Words are split on '/', empty words
 *     kept.  A plain filter is matched by the LIST clauses of emqx_topic:match/2
 *     (apps/emqx/src/emqx_topic.erl:74-87) in their order -- NO '$'-rule, so '#'
 *     authorizes '$SYS/x'; the request topic's words are opaque ('a/#' as a
 *     SUBSCRIBE name matches the filter 'a/+', not 'a/b'; '#' before a filter's
 *     last word equals only a name word '#').  EMQX_GM_AUTHZ_FILTER_EQ ({eq, T}
 *     or "eq T"): equality of the word lists, placeholders not substituted.  A
 *     plain filter holding '${clientid}' or '${username}' as a whole word is a
 *     pattern (feed_var/3, :182-195): the word is replaced by the client's value
 *     as ONE binary word -- a value "", "+", "#" or one holding '/' therefore
 *     equals no name word -- and stays literal when the value is undefined.
 * On a multi-device context the table lives on the first listed device.  A
 * table is immutable: a changed ACL is a new build the caller swaps in. */
typedef struct emqx_gm_authz emqx_gm_authz;
#define EMQX_GM_AUTHZ_GLOBAL 0u
#define EMQX_GM_AUTHZ_BY_CLIENTID 1u
#define EMQX_GM_AUTHZ_BY_USERNAME 2u
#define EMQX_GM_AUTHZ_ALLOW 1u /* rule_perm, and a verdict */
#define EMQX_GM_AUTHZ_DENY 2u
#define EMQX_GM_AUTHZ_NOMATCH 0u
#define EMQX_GM_AUTHZ_PUBLISH 1u /* rule_action, and a request's action */
#define EMQX_GM_AUTHZ_SUBSCRIBE 2u
#define EMQX_GM_AUTHZ_ALL 3u /* rule_action only */
#define EMQX_GM_AUTHZ_WHO_USERNAME 0u
#define EMQX_GM_AUTHZ_WHO_CLIENTID 1u
#define EMQX_GM_AUTHZ_WHO_IPADDR 2u /* ipaddr and ipaddrs: one or more CIDRs */
#define EMQX_GM_AUTHZ_WHO_REGEX 3u
#define EMQX_GM_AUTHZ_WHO_AND 4u /* a nested list: refused */
#define EMQX_GM_AUTHZ_WHO_OR 5u
#define EMQX_GM_AUTHZ_FILTER_PLAIN 0u /* a pattern if it holds a placeholder word */
#define EMQX_GM_AUTHZ_FILTER_EQ 1u
#define EMQX_GM_AUTHZ_CIDR_BYTES 33u /* family (4 | 6), lo[16], hi[16]; an IPv4 address in the first 4 of its 16 */
#define EMQX_GM_AUTHZ_NO_RULE 0xFFFFFFFFu
/* The table to compile.  Segment s owns ranges [seg_range_off[s], seg_range_off[s+1]):
 * exactly one for a GLOBAL segment, one per key for a keyed one (a key listed
 * twice in one segment: EMQX_GM_EINVAL).  Range k holds rules [range_rule_off[k],
 * range_rule_off[k+1]) in evaluation order under the key key_bytes[key_off[k] ..
 * key_off[k+1]) (ignored for a GLOBAL segment's).  Rule r: who leaves
 * [rule_who_off[r], rule_who_off[r+1]) joined by rule_who_op[r] (0 AND, 1 OR),
 * filters [rule_filter_off[r], rule_filter_off[r+1]).  Leaf l's argument is
 * leaf_bytes[leaf_off[l] .. leaf_off[l+1]): the value's bytes (username,
 * clientid), k * EMQX_GM_AUTHZ_CIDR_BYTES (ipaddr), or one byte k (regex). */
typedef struct {
  uint32_t n_segments;
  const uint32_t *seg_kind;
  const uint64_t *seg_range_off; /* [n_segments + 1] */
  uint64_t n_ranges;
  const uint64_t *range_rule_off; /* [n_ranges + 1] */
  const uint8_t *key_bytes;
  const uint64_t *key_off; /* [n_ranges + 1] */
  uint64_t n_rules;
  const uint32_t *rule_id;
  const uint8_t *rule_perm;   /* EMQX_GM_AUTHZ_ALLOW / _DENY */
  const uint8_t *rule_action; /* EMQX_GM_AUTHZ_PUBLISH / _SUBSCRIBE / _ALL */
  const uint8_t *rule_who_op;
  const uint64_t *rule_who_off;    /* [n_rules + 1] */
  const uint64_t *rule_filter_off; /* [n_rules + 1] */
  uint64_t n_leaves;
  const uint8_t *leaf_kind; /* EMQX_GM_AUTHZ_WHO_* */
  const uint8_t *leaf_bytes;
  const uint64_t *leaf_off; /* [n_leaves + 1] */
  uint64_t n_filters;
  const uint8_t *filter_kind; /* EMQX_GM_AUTHZ_FILTER_* */
  const uint8_t *filter_bytes;
  const uint64_t *filter_off; /* [n_filters + 1] */
} emqx_gm_authz_desc;
/* A window of requests, host buffers.  flags[i]: which of the clientinfo's
 * fields are defined (an undefined one's bytes are ignored). */
#define EMQX_GM_AUTHZ_F_CLIENTID 0x1u
#define EMQX_GM_AUTHZ_F_USERNAME 0x2u
#define EMQX_GM_AUTHZ_F_PEERHOST 0x4u
#define EMQX_GM_AUTHZ_F_IPV6 0x8u
typedef struct {
  uint64_t n;
  const uint8_t *topic_bytes;
  const uint64_t *topic_off; /* [n + 1] */
  const uint8_t *clientid_bytes;
  const uint64_t *clientid_off; /* [n + 1] */
  const uint8_t *username_bytes;
  const uint64_t *username_off; /* [n + 1] */
  const uint8_t *flags;         /* [n] EMQX_GM_AUTHZ_F_* */
  const uint8_t *peerhost;      /* [n][16] network order, an IPv4 address in the first 4 */
  const uint8_t *action;        /* [n] EMQX_GM_AUTHZ_PUBLISH / _SUBSCRIBE */
  const uint32_t *re_mask;      /* [n] bit k: the table's regex k matches this client */
} emqx_gm_authz_batch;
typedef struct {
  double build_ms;         /* host compile (and upload) of this table           */
  uint64_t device_bytes;   /* resident table bytes in HBM (0: host-only table)  */
  uint64_t n_rules;
  uint64_t n_keys;         /* keys over all keyed segments                      */
  uint64_t n_words;        /* distinct filter words, the 5 reserved included    */
  uint64_t n_filters;
  uint64_t n_leaves;
  uint32_t n_segments;
  uint32_t deepest_filter; /* words of the deepest filter                       */
  uint64_t longest_range;  /* rules of the longest range                        */
} emqx_gm_authz_info_t;
/* emqx_authz_rule:compile/1 (:55-94) of every rule and emqx_authz_mnesia:
 * store_rules/2 (emqx_authz_mnesia.erl:123-132) of every record, into one device
 * allocation.  Every offset array is checked as emqx_gm_retained_build checks
 * its own (from 0, ascending, entries under 2 GiB, the last equal to the next
 * array's count) and every code against its range (EMQX_GM_EINVAL) before any
 * device work.  At most 64 segments.  flags: 0. */
int emqx_gm_authz_build(emqx_gm_ctx *ctx, const emqx_gm_authz_desc *desc, uint32_t flags, emqx_gm_authz **out);
/* emqx_authz:do_authorize/4 (emqx_authz.erl:307-317) for every request of the
 * window: verdict[i] = EMQX_GM_AUTHZ_NOMATCH / _ALLOW / _DENY and rule[i] = the
 * first matching rule's id (EMQX_GM_AUTHZ_NO_RULE on nomatch).  The default for
 * nomatch (authorization.no_match, emqx_authz.erl:297-304) is the caller's.
 * Host buffers; a window of up to 2^20 requests takes one device round trip.
 * flags: 0 or EMQX_GM_AUTHZ_TIMED (the kernel is timed by device events). */
#define EMQX_GM_AUTHZ_TIMED 0x1u
int emqx_gm_authz_check(emqx_gm_ctx *ctx, const emqx_gm_authz *tab, const emqx_gm_authz_batch *batch,
                        uint32_t flags, uint8_t *verdict, uint32_t *rule);
/* emqx_authz_mnesia:record_count/0 (emqx_authz_mnesia.erl:175-177) and the table's shape */
int emqx_gm_authz_info(const emqx_gm_authz *tab, emqx_gm_authz_info_t *info);
/* emqx_authz_mnesia:purge_rules/0 (:135-141) of this table */
int emqx_gm_authz_release(emqx_gm_authz *tab);

#ifdef __cplusplus
}
#endif
#endif /* EMQX_GPU_MATCH_H */
