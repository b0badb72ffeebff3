/*
 * emqx_gpu_match_nif.c — thin Erlang NIF over libemqx_gpu_match.so.
 *
 * Erlang module `emqx_gpu_match` (nif/emqx_gpu_match.erl).  All calls run on
 * dirty CPU schedulers (a batch takes > 1 ms).  Non-binary input -> badarg;
 * device faults -> {error, Reason} so the Erlang wrapper can fall back to
 * emqx_trie:match/1.  An index is an enif resource whose
 * destructor releases the device snapshot (emqx_gm_index_release).
 *
 * Build (only where erl_nif.h exists; this container has no Erlang):
 *   cc -O2 -fPIC -shared -I$ERL_ROOT/usr/include -I../include \
 *      emqx_gpu_match_nif.c -L../emqx_amd -lemqx_gpu_match -o emqx_gpu_match_nif.so
 */
#include <erl_nif.h>
#include <stdlib.h>
#include <string.h>

#include "emqx_gpu_match.h"

/* An index snapshot.  Result rows are binaries that point straight into the
 * snapshot's host copy of the filter bytes (emqx_gm_index_filter) and keep
 * this resource -- hence the snapshot -- alive: no per-snapshot copy of the
 * filter set is made, so an incremental update_index costs O(delta), not
 * O(filters). */
typedef struct {
  emqx_gm_index *idx;
} gm_index_res;

typedef struct {
  emqx_gm_retained *idx;
} gm_retained_res;

typedef struct {
  emqx_gm_shared *sh; /* retains its snapshot: filter binaries made over this resource stay valid */
  emqx_gm_index *idx;
} gm_shared_res;

typedef struct {
  emqx_gm_authz *tab;
} gm_authz_res;

typedef struct {
  emqx_gm_subopts *so; /* retains its snapshot */
  emqx_gm_index *idx;
} gm_subopts_res;

static ErlNifResourceType *INDEX_RT, *RETAINED_RT, *SHARED_RT, *AUTHZ_RT, *SUBOPTS_RT;
static emqx_gm_ctx *CTX;
/* LoadInfo {coalesce, Devices}: the context's one combining queue -- the
 * windows of dirty schedulers calling at once run as one device batch
 * (emqx_gm_combiner, defaults); NULL: every call makes its own round trip */
static emqx_gm_combiner *COMB;
static ERL_NIF_TERM A_OK, A_ERROR, A_BADARG, A_INSERT, A_DELETE, A_SUBSCRIBE, A_UNSUBSCRIBE, A_ROUTE_ADD,
    A_ROUTE_DELETE, A_UNDEFINED;

static void index_dtor(ErlNifEnv *env, void *obj) {
  gm_index_res *r = (gm_index_res *)obj;
  (void)env;
  if (r->idx) emqx_gm_index_release(r->idx);
}

static void retained_dtor(ErlNifEnv *env, void *obj) {
  gm_retained_res *r = (gm_retained_res *)obj;
  (void)env;
  if (r->idx) emqx_gm_retained_release(r->idx);
}

static void shared_dtor(ErlNifEnv *env, void *obj) {
  gm_shared_res *r = (gm_shared_res *)obj;
  (void)env;
  if (r->sh) emqx_gm_shared_release(r->sh);
}

static void subopts_dtor(ErlNifEnv *env, void *obj) {
  gm_subopts_res *r = (gm_subopts_res *)obj;
  (void)env;
  if (r->so) emqx_gm_subopts_release(r->so);
}

static void authz_dtor(ErlNifEnv *env, void *obj) {
  gm_authz_res *r = (gm_authz_res *)obj;
  (void)env;
  if (r->tab) emqx_gm_authz_release(r->tab);
}

/* LoadInfo (erlang:load_nif/2): a device ordinal, or the node's device list
 * [D0, D1, ...] (1..EMQX_GM_MAX_DEVICES entries; repeats give several replicas
 * on one GPU).  With a list, the ONE context of this node replicates every
 * index to all listed GPUs and each match_*_batch / fanout_batch spreads its
 * batch over them (emqx_gm_opts.n_devices), as the reference's match_routes/1
 * runs on all schedulers at once (emqx_trie.erl:66-70, emqx_router.erl:128-145). */
static int load(ErlNifEnv *env, void **priv, ERL_NIF_TERM info) {
  int device = 0, arity = 0, coalesce = 0;
  unsigned nl = 0;
  const ERL_NIF_TERM *tup;
  emqx_gm_opts o;
  (void)priv;
  memset(&o, 0, sizeof(o));
  /* {coalesce, Devices}: Devices as below, the calls through one combiner */
  if (enif_get_tuple(env, info, &arity, &tup)) {
    if (arity != 2 || !enif_is_identical(tup[0], enif_make_atom(env, "coalesce"))) return 1;
    coalesce = 1;
    info = tup[1];
  }
  if (enif_get_list_length(env, info, &nl) && nl > 0) {
    ERL_NIF_TERM h, t = info;
    if (nl > EMQX_GM_MAX_DEVICES) return 1;
    while (enif_get_list_cell(env, t, &h, &t)) {
      if (!enif_get_int(env, h, &device)) return 1;
      o.devices[o.n_devices++] = device;
    }
  } else {
    enif_get_int(env, info, &device);
    o.device = device;
  }
  INDEX_RT = enif_open_resource_type(env, NULL, "emqx_gm_index", index_dtor, ERL_NIF_RT_CREATE, NULL);
  RETAINED_RT = enif_open_resource_type(env, NULL, "emqx_gm_retained", retained_dtor, ERL_NIF_RT_CREATE, NULL);
  SHARED_RT = enif_open_resource_type(env, NULL, "emqx_gm_shared", shared_dtor, ERL_NIF_RT_CREATE, NULL);
  AUTHZ_RT = enif_open_resource_type(env, NULL, "emqx_gm_authz", authz_dtor, ERL_NIF_RT_CREATE, NULL);
  SUBOPTS_RT = enif_open_resource_type(env, NULL, "emqx_gm_subopts", subopts_dtor, ERL_NIF_RT_CREATE, NULL);
  A_UNDEFINED = enif_make_atom(env, "undefined");
  A_OK = enif_make_atom(env, "ok");
  A_ERROR = enif_make_atom(env, "error");
  A_BADARG = enif_make_atom(env, "badarg");
  A_INSERT = enif_make_atom(env, "insert");
  A_DELETE = enif_make_atom(env, "delete");
  A_SUBSCRIBE = enif_make_atom(env, "subscribe");
  A_UNSUBSCRIBE = enif_make_atom(env, "unsubscribe");
  A_ROUTE_ADD = enif_make_atom(env, "route_add");
  A_ROUTE_DELETE = enif_make_atom(env, "route_delete");
  if (emqx_gm_open(&o, &CTX) != EMQX_GM_OK || !INDEX_RT || !RETAINED_RT || !SHARED_RT || !AUTHZ_RT ||
      !SUBOPTS_RT)
    return 1;
  if (coalesce && emqx_gm_combiner_open(CTX, NULL, &COMB) != EMQX_GM_OK) return 1;
  return 0;
}

static void unload(ErlNifEnv *env, void *priv) {
  (void)env;
  (void)priv;
  if (COMB) emqx_gm_combiner_close(COMB); /* (waits for the calls in flight; the context frees it) */
  if (CTX) emqx_gm_close(CTX);
}

/* The failing call's own message: emqx_gm_last_error() is per calling thread,
 * and this NIF call runs start to end on one dirty scheduler thread. */
static ERL_NIF_TERM error_tuple(ErlNifEnv *env, int rc) {
  const char *m = emqx_gm_last_error(CTX);
  (void)rc;
  return enif_make_tuple2(env, A_ERROR, enif_make_string(env, m && *m ? m : "device", ERL_NIF_LATIN1));
}

/* Pack a list of binaries into (bytes, offsets). */
static int pack_list(ErlNifEnv *env, ERL_NIF_TERM list, uint8_t **bytes, uint64_t **off, uint64_t *n) {
  unsigned len;
  ERL_NIF_TERM h, t = list;
  ErlNifBinary b;
  uint64_t total = 0, i = 0;
  if (!enif_get_list_length(env, list, &len)) return 0;
  while (enif_get_list_cell(env, t, &h, &t)) {
    if (!enif_inspect_binary(env, h, &b)) return 0;
    total += b.size;
  }
  *bytes = enif_alloc(total + 64);
  *off = enif_alloc((len + 1) * sizeof(uint64_t));
  (*off)[0] = 0;
  t = list;
  while (enif_get_list_cell(env, t, &h, &t)) {
    enif_inspect_binary(env, h, &b);
    memcpy(*bytes + (*off)[i], b.data, b.size);
    (*off)[i + 1] = (*off)[i] + b.size;
    ++i;
  }
  memset(*bytes + total, 0, 64);
  *n = len;
  return 1;
}

/* A publish batch packed straight into page-locked memory (emqx_gm_host_alloc):
 * the library then sends the text to the GPUs by DMA from here, with no
 * staging copy of its own.  One buffer per dirty scheduler thread, grown as
 * batches grow; the offsets stay in ordinary memory (the library validates and
 * rebases them anyway). */
static __thread uint8_t *PIN_BUF;
static __thread uint64_t PIN_CAP;

static int pack_topics(ErlNifEnv *env, ERL_NIF_TERM list, uint8_t **bytes, uint64_t **off, uint64_t *n) {
  unsigned len;
  ERL_NIF_TERM h, t = list;
  ErlNifBinary b;
  uint64_t total = 0, i = 0;
  if (!enif_get_list_length(env, list, &len)) return 0;
  while (enif_get_list_cell(env, t, &h, &t)) {
    if (!enif_inspect_binary(env, h, &b)) return 0;
    total += b.size;
  }
  if (PIN_CAP < total + 64) {
    void *p = NULL;
    uint64_t cap = PIN_CAP ? PIN_CAP : (1u << 20);
    while (cap < total + 64) cap *= 2;
    if (PIN_BUF) emqx_gm_host_free(CTX, PIN_BUF);
    PIN_BUF = NULL;
    PIN_CAP = 0;
    if (emqx_gm_host_alloc(CTX, cap, &p) == EMQX_GM_OK) {
      PIN_BUF = p;
      PIN_CAP = cap;
    }
  }
  if (!PIN_BUF) return pack_list(env, list, bytes, off, n);  /* (no page-locked memory: the plain way) */
  *bytes = PIN_BUF;
  *off = enif_alloc((len + 1) * sizeof(uint64_t));
  (*off)[0] = 0;
  t = list;
  while (enif_get_list_cell(env, t, &h, &t)) {
    enif_inspect_binary(env, h, &b);
    memcpy(*bytes + (*off)[i], b.data, b.size);
    (*off)[i + 1] = (*off)[i] + b.size;
    ++i;
  }
  memset(*bytes + total, 0, 64);
  *n = len;
  return 1;
}
static void free_topics(uint8_t *bytes, uint64_t *off) {
  if (bytes != PIN_BUF) enif_free(bytes);
  enif_free(off);
}

static ERL_NIF_TERM make_index_term(ErlNifEnv *env, emqx_gm_index *idx) {
  gm_index_res *r = enif_alloc_resource(INDEX_RT, sizeof(*r));
  ERL_NIF_TERM term;
  r->idx = idx;
  term = enif_make_resource(env, r);
  enif_release_resource(r);
  return enif_make_tuple2(env, A_OK, term);
}

/* Subscriber lists [[SubId :: non_neg_integer()]] -> CSR (n+1 offsets); one
 * list per filter. */
static int pack_subs(ErlNifEnv *env, ERL_NIF_TERM lists, uint64_t n, uint64_t **off, uint32_t **ids) {
  unsigned len, k;
  ERL_NIF_TERM h, t = lists, e, u;
  uint64_t total = 0, i = 0;
  if (!enif_get_list_length(env, lists, &len) || len != n) return 0;
  while (enif_get_list_cell(env, t, &h, &t)) {
    if (!enif_get_list_length(env, h, &k)) return 0;
    total += k;
  }
  *off = enif_alloc((n + 1) * sizeof(uint64_t));
  *ids = enif_alloc((total ? total : 1) * sizeof(uint32_t));
  (*off)[0] = 0;
  t = lists;
  while (enif_get_list_cell(env, t, &h, &t)) {
    uint64_t o = (*off)[i];
    u = h;
    while (enif_get_list_cell(env, u, &e, &u)) {
      unsigned v;
      if (!enif_get_uint(env, e, &v)) {
        enif_free(*off);
        enif_free(*ids);
        return 0;
      }
      (*ids)[o++] = v;
    }
    (*off)[++i] = o;
  }
  return 1;
}

/* load_index([Filter :: binary()]) -> {ok, Index} | {error, Reason}
 * load_index([Filter :: binary()], [[SubId :: non_neg_integer()]]) -> idem,
 *   with each filter's subscriber ids (the emqx_subscriber bag of
 *   emqx_broker.erl:147-165 with its {shard, I} buckets flattened), which
 *   fanout_batch/2 returns per topic. */
static ERL_NIF_TERM do_load(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[], int sharded) {
  uint8_t *fb;
  uint64_t *fo, n, *so = NULL;
  uint32_t *si = NULL;
  emqx_gm_index *idx = NULL;
  int rc;
  if (!pack_list(env, argv[0], &fb, &fo, &n)) return enif_make_badarg(env);
  if (argc == 2 && !pack_subs(env, argv[1], n, &so, &si)) {
    enif_free(fb);
    enif_free(fo);
    return enif_make_badarg(env);
  }
  rc = sharded ? emqx_gm_index_build_sharded(CTX, fb, fo, n, so, si, NULL, &idx)
               : emqx_gm_index_build(CTX, fb, fo, n, so, si, NULL, &idx);
  enif_free(fb);
  enif_free(fo);
  if (so) enif_free(so);
  if (si) enif_free(si);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return make_index_term(env, idx);
}

static ERL_NIF_TERM load_index(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  return do_load(env, argc, argv, 0);
}

/* load_index_sharded/1,2: as load_index/1,2, for a route table too large for
 * one GPU: the filters partitioned by first word over the context's devices
 * (emqx_gm_index_build_sharded), each topic matched on its one device.
 * match_batch/2, match_routes_batch/2 and fanout_batch/2 take the result like
 * any index.  update_index/2 works on a table from load_index_sharded/1 (no
 * subscriber ids): every device patches its share of the batch at once.  A
 * table from load_index_sharded/2 (with subscriber ids) is rebuild-only:
 * update_index/2 and update_subs/2 return {error, Reason} for it, as
 * update_subs/2 and export_index/1 do for any sharded table
 * (EMQX_GM_EUNSUPPORTED). */
static ERL_NIF_TERM load_index_sharded(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  return do_load(env, argc, argv, 1);
}

/* update_index(Index, [{Filter :: binary(), insert | delete}]) -> {ok, NewIndex} | {error, Reason}
 * emqx_gm_index_update: a new snapshot; Index stays valid for its readers. */
static ERL_NIF_TERM update_index(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *r;
  unsigned len, i = 0;
  ERL_NIF_TERM h, t = argv[1], fl = enif_make_list(env, 0);
  uint8_t *fb, *ops;
  uint64_t *fo, n;
  emqx_gm_index *idx = NULL;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r) || !enif_get_list_length(env, argv[1], &len))
    return enif_make_badarg(env);
  ops = enif_alloc(len + 1);
  while (enif_get_list_cell(env, t, &h, &t)) {
    const ERL_NIF_TERM *tup;
    int arity;
    if (!enif_get_tuple(env, h, &arity, &tup) || arity != 2) {
      enif_free(ops);
      return enif_make_badarg(env);
    }
    if (!enif_is_identical(tup[1], A_INSERT) && !enif_is_identical(tup[1], A_DELETE)) {
      enif_free(ops);
      return enif_make_badarg(env);  /* only insert | delete */
    }
    fl = enif_make_list_cell(env, tup[0], fl);
    ops[i++] = enif_is_identical(tup[1], A_INSERT) ? 1 : 0;
  }
  /* fl was built by prepending: reverse it back to the ops' order */
  if (!enif_make_reverse_list(env, fl, &fl) || !pack_list(env, fl, &fb, &fo, &n)) {
    enif_free(ops);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_index_update(CTX, r->idx, fb, fo, ops, n, &idx);
  enif_free(fb);
  enif_free(fo);
  enif_free(ops);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return make_index_term(env, idx);
}

/* update_subs(Index, [{Filter :: binary(), SubId :: non_neg_integer(),
 *                       subscribe | unsubscribe | route_add | route_delete}])
 *   -> {ok, NewIndex} | {error, Reason}
 * emqx_gm_index_update_subs on an index from load_index/2: emqx_broker's
 * subscribe/unsubscribe, with the route added on a filter's first subscriber
 * and deleted after its last; route_add / route_delete (SubId ignored) mark a
 * filter routed to another destination (a remote node, a shared group), which
 * keeps it in the index without a local subscriber. */
static ERL_NIF_TERM update_subs(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *r;
  unsigned len, i = 0;
  ERL_NIF_TERM h, t = argv[1], fl = enif_make_list(env, 0);
  uint8_t *fb, *ops;
  uint32_t *subs;
  uint64_t *fo, n;
  emqx_gm_index *idx = NULL;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r) || !enif_get_list_length(env, argv[1], &len))
    return enif_make_badarg(env);
  ops = enif_alloc(len + 1);
  subs = enif_alloc((len + 1) * sizeof(uint32_t));
  while (enif_get_list_cell(env, t, &h, &t)) {
    const ERL_NIF_TERM *tup;
    int arity;
    unsigned s;
    uint8_t kind;
    if (!enif_get_tuple(env, h, &arity, &tup) || arity != 3 || !enif_get_uint(env, tup[1], &s)) goto bad;
    if (enif_is_identical(tup[2], A_SUBSCRIBE)) kind = EMQX_GM_SUB_SUBSCRIBE;
    else if (enif_is_identical(tup[2], A_UNSUBSCRIBE)) kind = EMQX_GM_SUB_UNSUBSCRIBE;
    else if (enif_is_identical(tup[2], A_ROUTE_ADD)) kind = EMQX_GM_SUB_ROUTE_ADD;
    else if (enif_is_identical(tup[2], A_ROUTE_DELETE)) kind = EMQX_GM_SUB_ROUTE_DELETE;
    else goto bad;
    fl = enif_make_list_cell(env, tup[0], fl);
    subs[i] = s;
    ops[i++] = kind;
    continue;
  bad:
    enif_free(ops);
    enif_free(subs);
    return enif_make_badarg(env);
  }
  if (!enif_make_reverse_list(env, fl, &fl) || !pack_list(env, fl, &fb, &fo, &n)) {
    enif_free(ops);
    enif_free(subs);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_index_update_subs(CTX, r->idx, fb, fo, subs, ops, n, &idx);
  enif_free(fb);
  enif_free(fo);
  enif_free(ops);
  enif_free(subs);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return make_index_term(env, idx);
}

static ERL_NIF_TERM do_match(ErlNifEnv *env, const ERL_NIF_TERM argv[], uint32_t flags) {
  gm_index_res *r;
  uint8_t *tb;
  uint64_t *to, n, i, k;
  emqx_gm_csr out;
  ERL_NIF_TERM bin, result, *rows;
  int rc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r)) return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  rc = COMB ? emqx_gm_combiner_match(COMB, r->idx, tb, to, n, flags, &out, NULL)
            : emqx_gm_match(CTX, r->idx, tb, to, n, flags, &out);
  free_topics(tb, to);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  /* each filter is a binary over the snapshot's own host bytes, kept alive by the resource */
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    for (k = out.row_off[i + 1]; k > out.row_off[i]; --k) {
      const uint8_t *p;
      uint64_t l;
      emqx_gm_index_filter(r->idx, out.ids[k - 1], &p, &l);
      bin = enif_make_resource_binary(env, r, p, l);
      row = enif_make_list_cell(env, bin, row);
    }
    rows[i] = row;
  }
  result = enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_csr_free(CTX, &out);
  return result;
}

/* match_batch(Index, [Topic]) -> [[Filter]]   (emqx_trie:match/1 per topic) */
static ERL_NIF_TERM match_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return do_match(env, argv, 0);
}

/* match_routes_batch(Index, [Topic]) -> [[Filter]]  (emqx_router:match_routes/1 filters) */
static ERL_NIF_TERM match_routes_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return do_match(env, argv, EMQX_GM_WITH_EXACT);
}

/* fanout_batch(Index, [Topic]) -> [[{Filter, [SubId]}]]
 * emqx_broker:publish/1's route + dispatch for each topic: its matched filters
 * (match_routes/1) in ascending order, each with the subscribers do_dispatch/2
 * folds over (emqx_broker.erl:296-322, 506-530) -- the order of the GPU
 * fan-out row, cut back into one segment per filter so the caller can send
 * {deliver, Filter, Msg}.  The index must come from load_index/2. */
static ERL_NIF_TERM fanout_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *r;
  uint8_t *tb;
  uint64_t *to, n, i, k, d_pos;
  emqx_gm_csr m, d;
  ERL_NIF_TERM result, *rows;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r)) return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  /* the match and its fan-out in one call: one device round trip per window,
   * or (coalesce) per group of the windows that call at once */
  rc = COMB ? emqx_gm_combiner_match(COMB, r->idx, tb, to, n, EMQX_GM_WITH_EXACT, &m, &d)
            : emqx_gm_match_fanout(CTX, r->idx, tb, to, n, EMQX_GM_WITH_EXACT, &m, &d);
  free_topics(tb, to);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    d_pos = d.row_off[i + 1];
    for (k = m.row_off[i + 1]; k > m.row_off[i]; --k) {  /* filters back to front */
      const uint8_t *p;
      uint64_t l, c, j;
      ERL_NIF_TERM subs = enif_make_list(env, 0);
      const uint32_t f = m.ids[k - 1];
      if (emqx_gm_index_filter(r->idx, f, &p, &l) != EMQX_GM_OK ||
          emqx_gm_index_subscriber_count(r->idx, f, &c) != EMQX_GM_OK || c > d_pos - d.row_off[i]) {
        enif_free(rows);
        emqx_gm_csr_free(CTX, &m);
        emqx_gm_csr_free(CTX, &d);
        return error_tuple(env, EMQX_GM_EINVAL);
      }
      for (j = 0; j < c; ++j) subs = enif_make_list_cell(env, enif_make_uint(env, d.ids[d_pos - 1 - j]), subs);
      d_pos -= c;
      row = enif_make_list_cell(env, enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l), subs), row);
    }
    rows[i] = row;
  }
  result = enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_csr_free(CTX, &m);
  emqx_gm_csr_free(CTX, &d);
  return result;
}

/* empty(Index) -> boolean()  (emqx_trie:empty/0) */
static ERL_NIF_TERM empty(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *r;
  emqx_gm_index_info_t info;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r)) return enif_make_badarg(env);
  emqx_gm_index_info(r->idx, &info);
  return enif_make_atom(env, info.trie_empty ? "true" : "false");
}

/* export_index(Index) -> {ok, Image :: binary()} | {error, Reason}
 * emqx_gm_index_export with the device tables: the snapshot as one binary a
 * joining node imports instead of recompiling the route table (the reference
 * replicates its routing tables through mria, emqx_router.erl:75-84). */
static ERL_NIF_TERM export_index(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *r;
  ErlNifBinary bin;
  uint64_t size = 0;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&r)) return enif_make_badarg(env);
  rc = emqx_gm_index_export(CTX, r->idx, 0, NULL, &size);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  if (!enif_alloc_binary((size_t)size, &bin))
    return enif_make_tuple2(env, A_ERROR, enif_make_string(env, "enomem", ERL_NIF_LATIN1));
  rc = emqx_gm_index_export(CTX, r->idx, 0, bin.data, &size);
  if (rc != EMQX_GM_OK) {
    enif_release_binary(&bin);
    return error_tuple(env, rc);
  }
  return enif_make_tuple2(env, A_OK, enif_make_binary(env, &bin));
}

/* import_index(Image :: binary()) -> {ok, Index} | {error, Reason}
 * emqx_gm_index_import on this node's device (an image of another layout or
 * a truncated one: {error, _}). */
static ERL_NIF_TERM import_index(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  ErlNifBinary bin;
  emqx_gm_index *idx = NULL;
  int rc;
  (void)argc;
  if (!enif_inspect_binary(env, argv[0], &bin)) return enif_make_badarg(env);
  rc = emqx_gm_index_import(CTX, bin.data, bin.size, NULL, &idx);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return make_index_term(env, idx);
}

/* ---- retained-message lookup (emqx_gm_retained_*): the emqx_retainer backend's table ----
 * NowMs and expiries are milliseconds since the epoch: past 32 bits, read with
 * enif_get_ulong (64-bit on the platforms this library runs on). */
#ifdef EMQX_TEST_ERL_NIF_STUB_H /* the syntax-check stub lists only what the shim used before; the real header has it */
int enif_get_ulong(ErlNifEnv *, ERL_NIF_TERM, unsigned long *);
#endif

static ERL_NIF_TERM make_retained_term(ErlNifEnv *env, emqx_gm_retained *idx) {
  gm_retained_res *r = enif_alloc_resource(RETAINED_RT, sizeof(*r));
  ERL_NIF_TERM term;
  r->idx = idx;
  term = enif_make_resource(env, r);
  enif_release_resource(r);
  return enif_make_tuple2(env, A_OK, term);
}

/* load_retained([Topic]) | load_retained([Topic], [ExpiryMs]) -> {ok, Index}
 * the table store_retained/2 maintains (emqx_retainer_mnesia.erl:74-104); ids
 * in match_retained/3 rows are positions in [Topic] (of equal topics the last) */
static ERL_NIF_TERM load_retained(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  uint8_t *tb;
  uint64_t *to, n, i = 0, *ex = NULL;
  emqx_gm_retained *idx = NULL;
  int rc;
  if (!pack_list(env, argv[0], &tb, &to, &n)) return enif_make_badarg(env);
  if (argc > 1) {
    unsigned len;
    unsigned long v;
    ERL_NIF_TERM h, t = argv[1];
    if (!enif_get_list_length(env, t, &len) || len != n) goto badarg;
    ex = enif_alloc(sizeof(uint64_t) * (n ? n : 1));
    while (enif_get_list_cell(env, t, &h, &t)) {
      if (!enif_get_ulong(env, h, &v)) goto badarg;
      ex[i++] = v;
    }
  }
  rc = emqx_gm_retained_build(CTX, tb, to, n, NULL, ex, 0, &idx);
  enif_free(tb);
  enif_free(to);
  if (ex) enif_free(ex);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return make_retained_term(env, idx);
badarg:
  enif_free(tb);
  enif_free(to);
  if (ex) enif_free(ex);
  return enif_make_badarg(env);
}

/* match_retained(Index, [Filter], NowMs) -> [[Id]]
 * emqx_retainer_mnesia:match_messages/1 per filter (:210-214), each row in
 * topic order; the caller reads its messages by id and sorts them by timestamp
 * (sort_retained/1) */
static ERL_NIF_TERM match_retained(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_retained_res *r;
  uint8_t *fb;
  uint64_t *fo, n, i, k;
  unsigned long now;
  emqx_gm_csr out;
  ERL_NIF_TERM result, *rows;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], RETAINED_RT, (void **)&r) || !enif_get_ulong(env, argv[2], &now))
    return enif_make_badarg(env);
  if (!pack_list(env, argv[1], &fb, &fo, &n)) return enif_make_badarg(env);
  rc = emqx_gm_retained_match(CTX, r->idx, fb, fo, n, now, 0, &out);
  enif_free(fb);
  enif_free(fo);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    for (k = out.row_off[i + 1]; k > out.row_off[i]; --k)
      row = enif_make_list_cell(env, enif_make_uint(env, out.ids[k - 1]), row);
    rows[i] = row;
  }
  result = enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_csr_free(CTX, &out);
  return result;
}

/* expire_retained(Index, [{Topic, ExpiryMs}]) -> {ok, NFound}
 * delete_message/2 of a literal topic (ExpiryMs = 1, :117-128) or a refreshed
 * message on a stored topic; mutates the table in place (emqx_gm_retained_expire) */
static ERL_NIF_TERM expire_retained(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_retained_res *r;
  unsigned len, i = 0;
  ERL_NIF_TERM h, t, *topics, list;
  uint8_t *tb;
  uint64_t *to, n, *ex, found = 0;
  int rc, ok = 1;
  (void)argc;
  if (!enif_get_resource(env, argv[0], RETAINED_RT, (void **)&r) || !enif_get_list_length(env, argv[1], &len))
    return enif_make_badarg(env);
  topics = enif_alloc(sizeof(ERL_NIF_TERM) * (len ? len : 1));
  ex = enif_alloc(sizeof(uint64_t) * (len ? len : 1));
  t = argv[1];
  while (ok && enif_get_list_cell(env, t, &h, &t)) {
    const ERL_NIF_TERM *tup;
    int arity;
    unsigned long v;
    ok = enif_get_tuple(env, h, &arity, &tup) && arity == 2 && enif_get_ulong(env, tup[1], &v);
    if (ok) {
      topics[i] = tup[0];
      ex[i++] = v;
    }
  }
  list = enif_make_list_from_array(env, topics, i);
  enif_free(topics);
  if (!ok || !pack_list(env, list, &tb, &to, &n)) {
    enif_free(ex);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_retained_expire(CTX, r->idx, tb, to, n, ex, &found);
  enif_free(tb);
  enif_free(to);
  enif_free(ex);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  return enif_make_tuple2(env, A_OK, enif_make_uint(env, (unsigned)found));
}

/* ---- shared-subscription dispatch (emqx_gm_shared_*): emqx_shared_sub's member selection ----
 * load_shared(Index, [{Filter, GroupId}], [[MemberId]]) | load_shared(.., Prev) -> {ok, Table}
 * the emqx_shared_subscription table (emqx_shared_sub.erl:287-288) bound to the
 * snapshot Index: one member list per {Filter, GroupId}, in subscription order;
 * Prev hands on the round_robin / sticky state (emqx_gm_shared_build) */
static ERL_NIF_TERM load_shared(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *ix;
  gm_shared_res *prev = NULL, *res;
  unsigned len, i = 0;
  ERL_NIF_TERM h, t, *filters, list, term;
  uint8_t *fb;
  uint64_t *fo, n, *mo = NULL;
  uint32_t *gids, *mi = NULL;
  emqx_gm_shared *sh = NULL;
  int rc, ok = 1;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&ix) || !enif_get_list_length(env, argv[1], &len))
    return enif_make_badarg(env);
  if (argc == 4 && !enif_get_resource(env, argv[3], SHARED_RT, (void **)&prev)) return enif_make_badarg(env);
  filters = enif_alloc(sizeof(ERL_NIF_TERM) * (len ? len : 1));
  gids = enif_alloc(sizeof(uint32_t) * (len ? len : 1));
  t = argv[1];
  while (ok && enif_get_list_cell(env, t, &h, &t)) {
    const ERL_NIF_TERM *tup;
    int arity;
    unsigned g;
    ok = enif_get_tuple(env, h, &arity, &tup) && arity == 2 && enif_get_uint(env, tup[1], &g);
    if (ok) {
      filters[i] = tup[0];
      gids[i++] = g;
    }
  }
  list = enif_make_list_from_array(env, filters, i);
  enif_free(filters);
  if (!ok || !pack_list(env, list, &fb, &fo, &n)) {
    enif_free(gids);
    return enif_make_badarg(env);
  }
  if (!pack_subs(env, argv[2], n, &mo, &mi)) {
    enif_free(gids);
    enif_free(fb);
    enif_free(fo);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_shared_build(CTX, ix->idx, fb, fo, gids, n, mo, mi, prev ? prev->sh : NULL, 0, &sh);
  enif_free(gids);
  enif_free(fb);
  enif_free(fo);
  enif_free(mo);
  enif_free(mi);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  res = enif_alloc_resource(SHARED_RT, sizeof(*res));
  res->sh = sh;
  res->idx = ix->idx; /* (kept alive by the table's own reference) */
  term = enif_make_resource(env, res);
  enif_release_resource(res);
  return enif_make_tuple2(env, A_OK, term);
}

/* pick_shared_nif(Table, [Topic], Strategy :: 0..3, [Hash], Seed) -> [[{Filter, {GroupId, MemberId}}]]
 * per topic, in batch order, the member emqx_shared_sub:pick/6 (:234-288) picks
 * for every {Group, Filter} the topic matches: the match (match_routes/1) and
 * the picks of the whole window, one emqx_gm_shared_pick.  Hashes (one per topic,
 * erlang:phash2/1 of the client id or source topic, computed by the Erlang
 * wrapper pick_shared/4) are read for Strategy 0 only. */
static ERL_NIF_TERM pick_shared_nif(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_shared_res *r;
  uint8_t *tb;
  uint64_t *to, n, i, k;
  unsigned strategy, seed, nh = 0, v;
  uint32_t *hash = NULL;
  emqx_gm_csr m, om, os;
  ERL_NIF_TERM result, *rows, h, t;
  int rc;
  (void)argc;
  if (!enif_get_resource(env, argv[0], SHARED_RT, (void **)&r) || !enif_get_uint(env, argv[2], &strategy) ||
      !enif_get_list_length(env, argv[3], &nh) || !enif_get_uint(env, argv[4], &seed))
    return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  if (strategy == EMQX_GM_SHARE_HASH) {
    if (nh != n) {
      free_topics(tb, to);
      return enif_make_badarg(env);
    }
    hash = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
    t = argv[3];
    i = 0;
    while (enif_get_list_cell(env, t, &h, &t)) {
      if (!enif_get_uint(env, h, &v)) {
        enif_free(hash);
        free_topics(tb, to);
        return enif_make_badarg(env);
      }
      hash[i++] = v;
    }
  }
  rc = emqx_gm_match(CTX, r->idx, tb, to, n, EMQX_GM_WITH_EXACT, &m);
  free_topics(tb, to);
  if (rc == EMQX_GM_OK) {
    rc = emqx_gm_shared_pick(CTX, r->sh, &m, strategy, hash, seed, &om, &os);
    emqx_gm_csr_free(CTX, &m);
  }
  if (hash) enif_free(hash);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    for (k = om.row_off[i + 1]; k > om.row_off[i]; --k) {
      const uint8_t *p = NULL;
      uint64_t l = 0;
      uint32_t f = 0, g = 0;
      if (emqx_gm_shared_slot(r->sh, os.ids[k - 1], &f, &g, NULL, NULL) != EMQX_GM_OK ||
          emqx_gm_index_filter(r->idx, f, &p, &l) != EMQX_GM_OK) {
        enif_free(rows);
        emqx_gm_csr_free(CTX, &om);
        emqx_gm_csr_free(CTX, &os);
        return error_tuple(env, EMQX_GM_EINVAL);
      }
      row = enif_make_list_cell(
          env,
          enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l),
                           enif_make_tuple2(env, enif_make_uint(env, g), enif_make_uint(env, om.ids[k - 1]))),
          row);
    }
    rows[i] = row;
  }
  result = enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_csr_free(CTX, &om);
  emqx_gm_csr_free(CTX, &os);
  return result;
}

/* publish_window_nif(Table, [Topic], Strategy :: 0..3, [Hash], Seed) ->
 *     [{[{Filter, [SubId]}], [{Filter, {GroupId, MemberId}}]}]
 * per topic, in batch order, what fanout_batch/2 and pick_shared_nif/5 give for
 * it -- the matched filters with their local subscribers, and the member picked
 * for every {Group, Filter} the topic matches -- from ONE emqx_gm_publish_window:
 * one device round trip for the window instead of the match, the fan-out and
 * the pick one after the other.  The table's snapshot must come from
 * load_index/2.  (The node destinations have no table in this shim yet, so the
 * window carries no forward plan.) */
static ERL_NIF_TERM publish_window_nif(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_shared_res *r;
  uint8_t *tb;
  uint64_t *to, n, i, k, d_pos;
  unsigned strategy, seed, nh = 0, v;
  uint32_t *hash = NULL;
  emqx_gm_publish_opts o;
  emqx_gm_publish_result w;
  ERL_NIF_TERM result, *rows, h, t;
  int rc, bad = 0;
  (void)argc;
  if (!enif_get_resource(env, argv[0], SHARED_RT, (void **)&r) || !enif_get_uint(env, argv[2], &strategy) ||
      !enif_get_list_length(env, argv[3], &nh) || !enif_get_uint(env, argv[4], &seed))
    return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  if (strategy == EMQX_GM_SHARE_HASH) {
    if (nh != n) {
      free_topics(tb, to);
      return enif_make_badarg(env);
    }
    hash = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
    t = argv[3];
    i = 0;
    while (enif_get_list_cell(env, t, &h, &t)) {
      if (!enif_get_uint(env, h, &v)) {
        enif_free(hash);
        free_topics(tb, to);
        return enif_make_badarg(env);
      }
      hash[i++] = v;
    }
  }
  memset(&o, 0, sizeof(o));
  o.flags = EMQX_GM_WITH_EXACT;
  o.shared = r->sh;
  o.strategy = strategy;
  o.seed = seed;
  o.msg_hash = hash;
  rc = emqx_gm_publish_window(CTX, r->idx, tb, to, n, &o, &w, NULL);
  free_topics(tb, to);
  if (hash) enif_free(hash);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n && !bad; ++i) {
    ERL_NIF_TERM fan = enif_make_list(env, 0), picks = enif_make_list(env, 0);
    d_pos = w.deliveries.row_off[i + 1];
    for (k = w.matches.row_off[i + 1]; k > w.matches.row_off[i] && !bad; --k) { /* filters back to front */
      const uint8_t *p;
      uint64_t l, c, j;
      ERL_NIF_TERM subs = enif_make_list(env, 0);
      const uint32_t f = w.matches.ids[k - 1];
      if (emqx_gm_index_filter(r->idx, f, &p, &l) != EMQX_GM_OK ||
          emqx_gm_index_subscriber_count(r->idx, f, &c) != EMQX_GM_OK || c > d_pos - w.deliveries.row_off[i]) {
        bad = 1;
        break;
      }
      for (j = 0; j < c; ++j)
        subs = enif_make_list_cell(env, enif_make_uint(env, w.deliveries.ids[d_pos - 1 - j]), subs);
      d_pos -= c;
      fan = enif_make_list_cell(env, enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l), subs), fan);
    }
    for (k = w.pick_members.row_off[i + 1]; k > w.pick_members.row_off[i] && !bad; --k) {
      const uint8_t *p = NULL;
      uint64_t l = 0;
      uint32_t f = 0, g = 0;
      if (emqx_gm_shared_slot(r->sh, w.pick_slots.ids[k - 1], &f, &g, NULL, NULL) != EMQX_GM_OK ||
          emqx_gm_index_filter(r->idx, f, &p, &l) != EMQX_GM_OK) {
        bad = 1;
        break;
      }
      picks = enif_make_list_cell(
          env,
          enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l),
                           enif_make_tuple2(env, enif_make_uint(env, g), enif_make_uint(env, w.pick_members.ids[k - 1]))),
          picks);
    }
    rows[i] = enif_make_tuple2(env, fan, picks);
  }
  result = bad ? error_tuple(env, EMQX_GM_EINVAL) : enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_publish_result_free(CTX, &w);
  return result;
}

/* ---- authorization check (emqx_gm_authz_*): emqx_authz:do_authorize/4 over file + built-in-database sources ----
 * Growable arrays for the flat description / request batch. */
typedef struct {
  uint8_t *p;
  uint64_t n, cap;
} az_buf;

static void az_put(az_buf *b, const void *src, uint64_t bytes) {
  if (b->n + bytes + 64 > b->cap) {
    uint64_t cap = b->cap ? b->cap : 256;
    uint8_t *q;
    while (cap < b->n + bytes + 64) cap *= 2;
    q = enif_alloc(cap);
    if (b->n) memcpy(q, b->p, b->n);
    if (b->p) enif_free(b->p);
    b->p = q;
    b->cap = cap;
  }
  if (bytes) memcpy(b->p + b->n, src, bytes);
  b->n += bytes;
}
static void az_put_u64(az_buf *b, uint64_t v) { az_put(b, &v, 8); }
static void az_put_u32(az_buf *b, uint32_t v) { az_put(b, &v, 4); }
static void az_put_u8(az_buf *b, unsigned v) {
  uint8_t x = (uint8_t)v;
  az_put(b, &x, 1);
}
static void az_free(az_buf *b, int n) {
  int i;
  for (i = 0; i < n; ++i)
    if (b[i].p) enif_free(b[i].p);
}

/* load_authz([Segment]) -> {ok, Table}
 * Segment = {Kind, [{Key, [Rule]}]}: Kind 0 a GLOBAL segment (one {<<>>, Rules}: a
 * file source's rules, or the built-in database's `all` record), 1 / 2 the
 * clientid / username records (emqx_authz_mnesia.erl:123-132), in chain order.
 * Rule = {Id, Perm, Action, WhoOp, [{LeafKind, Arg}], [{FilterKind, Filter}]} with
 * the codes of emqx_gpu_match.h (EMQX_GM_AUTHZ_*); emqx_gpu_match:authz_rule/2
 * makes one from the reference's rule tuple (emqx_authz_rule.erl:49). */
enum { AZ_SEG_KIND, AZ_SEG_OFF, AZ_RANGE_OFF, AZ_KEYS, AZ_KEY_OFF, AZ_RULE_ID, AZ_PERM, AZ_ACTION, AZ_OP, AZ_WHO_OFF,
       AZ_FILT_OFF, AZ_LEAF_KIND, AZ_LEAF_BYTES, AZ_LEAF_OFF, AZ_FILT_KIND, AZ_FILT_BYTES, AZ_FILT_BOFF, AZ_NBUF };

static ERL_NIF_TERM load_authz(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  az_buf b[AZ_NBUF];
  ERL_NIF_TERM seg, segs = argv[0], h, t, rh, rt, lh, lt, term;
  const ERL_NIF_TERM *tup, *kt, *ru, *lf;
  int arity, rc, ok = 1;
  unsigned kind, u;
  uint64_t n_segs = 0, n_ranges = 0, n_rules = 0, n_leaves = 0, n_filters = 0;
  ErlNifBinary bin;
  emqx_gm_authz_desc d;
  emqx_gm_authz *tab = NULL;
  gm_authz_res *res;
  (void)argc;
  memset(b, 0, sizeof(b));
  az_put_u64(&b[AZ_SEG_OFF], 0), az_put_u64(&b[AZ_RANGE_OFF], 0), az_put_u64(&b[AZ_KEY_OFF], 0);
  az_put_u64(&b[AZ_WHO_OFF], 0), az_put_u64(&b[AZ_FILT_OFF], 0), az_put_u64(&b[AZ_LEAF_OFF], 0);
  az_put_u64(&b[AZ_FILT_BOFF], 0);
  az_put(&b[AZ_SEG_KIND], NULL, 0), az_put(&b[AZ_KEYS], NULL, 0), az_put(&b[AZ_RULE_ID], NULL, 0);
  az_put(&b[AZ_PERM], NULL, 0), az_put(&b[AZ_ACTION], NULL, 0), az_put(&b[AZ_OP], NULL, 0);
  az_put(&b[AZ_LEAF_KIND], NULL, 0), az_put(&b[AZ_LEAF_BYTES], NULL, 0), az_put(&b[AZ_FILT_KIND], NULL, 0);
  az_put(&b[AZ_FILT_BYTES], NULL, 0);
  while (ok && enif_get_list_cell(env, segs, &seg, &segs)) {
    ok = enif_get_tuple(env, seg, &arity, &tup) && arity == 2 && enif_get_uint(env, tup[0], &kind);
    if (!ok) break;
    az_put_u32(&b[AZ_SEG_KIND], kind);
    ++n_segs;
    t = tup[1];
    while (ok && enif_get_list_cell(env, t, &h, &t)) {
      ok = enif_get_tuple(env, h, &arity, &kt) && arity == 2 && enif_inspect_binary(env, kt[0], &bin);
      if (!ok) break;
      az_put(&b[AZ_KEYS], bin.data, bin.size);
      az_put_u64(&b[AZ_KEY_OFF], b[AZ_KEYS].n);
      rt = kt[1];
      while (ok && enif_get_list_cell(env, rt, &rh, &rt)) {
        ok = enif_get_tuple(env, rh, &arity, &ru) && arity == 6 && enif_get_uint(env, ru[0], &u);
        if (!ok) break;
        az_put_u32(&b[AZ_RULE_ID], u);
        ok = enif_get_uint(env, ru[1], &u);
        az_put_u8(&b[AZ_PERM], u);
        ok = ok && enif_get_uint(env, ru[2], &u);
        az_put_u8(&b[AZ_ACTION], u);
        ok = ok && enif_get_uint(env, ru[3], &u);
        az_put_u8(&b[AZ_OP], u);
        lt = ru[4];
        while (ok && enif_get_list_cell(env, lt, &lh, &lt)) {
          ok = enif_get_tuple(env, lh, &arity, &lf) && arity == 2 && enif_get_uint(env, lf[0], &u) &&
               enif_inspect_binary(env, lf[1], &bin);
          if (!ok) break;
          az_put_u8(&b[AZ_LEAF_KIND], u);
          az_put(&b[AZ_LEAF_BYTES], bin.data, bin.size);
          az_put_u64(&b[AZ_LEAF_OFF], b[AZ_LEAF_BYTES].n);
          ++n_leaves;
        }
        lt = ru[5];
        while (ok && enif_get_list_cell(env, lt, &lh, &lt)) {
          ok = enif_get_tuple(env, lh, &arity, &lf) && arity == 2 && enif_get_uint(env, lf[0], &u) &&
               enif_inspect_binary(env, lf[1], &bin);
          if (!ok) break;
          az_put_u8(&b[AZ_FILT_KIND], u);
          az_put(&b[AZ_FILT_BYTES], bin.data, bin.size);
          az_put_u64(&b[AZ_FILT_BOFF], b[AZ_FILT_BYTES].n);
          ++n_filters;
        }
        az_put_u64(&b[AZ_WHO_OFF], n_leaves);
        az_put_u64(&b[AZ_FILT_OFF], n_filters);
        ++n_rules;
      }
      az_put_u64(&b[AZ_RANGE_OFF], n_rules);
      ++n_ranges;
    }
    az_put_u64(&b[AZ_SEG_OFF], n_ranges);
  }
  if (!ok) {
    az_free(b, AZ_NBUF);
    return enif_make_badarg(env);
  }
  memset(&d, 0, sizeof(d));
  d.n_segments = (uint32_t)n_segs;
  d.seg_kind = (const uint32_t *)b[AZ_SEG_KIND].p;
  d.seg_range_off = (const uint64_t *)b[AZ_SEG_OFF].p;
  d.n_ranges = n_ranges;
  d.range_rule_off = (const uint64_t *)b[AZ_RANGE_OFF].p;
  d.key_bytes = b[AZ_KEYS].p;
  d.key_off = (const uint64_t *)b[AZ_KEY_OFF].p;
  d.n_rules = n_rules;
  d.rule_id = (const uint32_t *)b[AZ_RULE_ID].p;
  d.rule_perm = b[AZ_PERM].p;
  d.rule_action = b[AZ_ACTION].p;
  d.rule_who_op = b[AZ_OP].p;
  d.rule_who_off = (const uint64_t *)b[AZ_WHO_OFF].p;
  d.rule_filter_off = (const uint64_t *)b[AZ_FILT_OFF].p;
  d.n_leaves = n_leaves;
  d.leaf_kind = b[AZ_LEAF_KIND].p;
  d.leaf_bytes = b[AZ_LEAF_BYTES].p;
  d.leaf_off = (const uint64_t *)b[AZ_LEAF_OFF].p;
  d.n_filters = n_filters;
  d.filter_kind = b[AZ_FILT_KIND].p;
  d.filter_bytes = b[AZ_FILT_BYTES].p;
  d.filter_off = (const uint64_t *)b[AZ_FILT_BOFF].p;
  rc = emqx_gm_authz_build(CTX, &d, 0, &tab);
  az_free(b, AZ_NBUF);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  res = enif_alloc_resource(AUTHZ_RT, sizeof(*res));
  res->tab = tab;
  term = enif_make_resource(env, res);
  enif_release_resource(res);
  return enif_make_tuple2(env, A_OK, term);
}

/* authorize_batch(Table, [{Topic, ClientId, Username, Peerhost, Action, ReMask}]) -> [{Verdict, RuleId}]
 * emqx_authz:do_authorize/4 (emqx_authz.erl:307-317) per request, in order:
 * ClientId / Username a binary or `undefined`; Peerhost the address's 4 or 16
 * bytes or `undefined`; Action 1 publish, 2 subscribe; ReMask the client's regex
 * bits.  Verdict 0 nomatch (RuleId 16#FFFFFFFF), 1 allow, 2 deny. */
enum { AQ_TOPICS, AQ_TOFF, AQ_CIDS, AQ_COFF, AQ_UNS, AQ_UOFF, AQ_FLAGS, AQ_PEER, AQ_ACTION, AQ_MASK, AQ_NBUF };

static ERL_NIF_TERM authorize_batch(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_authz_res *r;
  az_buf b[AQ_NBUF];
  ERL_NIF_TERM h, t = argv[1], result;
  const ERL_NIF_TERM *q;
  int arity, rc, ok = 1;
  unsigned u;
  uint64_t n = 0, i;
  ErlNifBinary bin;
  emqx_gm_authz_batch batch;
  uint8_t *verdict, peer[16];
  uint32_t *rule;
  (void)argc;
  if (!enif_get_resource(env, argv[0], AUTHZ_RT, (void **)&r)) return enif_make_badarg(env);
  memset(b, 0, sizeof(b));
  az_put_u64(&b[AQ_TOFF], 0), az_put_u64(&b[AQ_COFF], 0), az_put_u64(&b[AQ_UOFF], 0);
  az_put(&b[AQ_TOPICS], NULL, 0), az_put(&b[AQ_CIDS], NULL, 0), az_put(&b[AQ_UNS], NULL, 0);
  az_put(&b[AQ_FLAGS], NULL, 0), az_put(&b[AQ_PEER], NULL, 0), az_put(&b[AQ_ACTION], NULL, 0);
  az_put(&b[AQ_MASK], NULL, 0);
  while (ok && enif_get_list_cell(env, t, &h, &t)) {
    unsigned flags = 0;
    ok = enif_get_tuple(env, h, &arity, &q) && arity == 6 && enif_inspect_binary(env, q[0], &bin);
    if (!ok) break;
    az_put(&b[AQ_TOPICS], bin.data, bin.size);
    az_put_u64(&b[AQ_TOFF], b[AQ_TOPICS].n);
    if (!enif_is_identical(q[1], A_UNDEFINED)) {
      ok = enif_inspect_binary(env, q[1], &bin);
      if (!ok) break;
      az_put(&b[AQ_CIDS], bin.data, bin.size);
      flags |= EMQX_GM_AUTHZ_F_CLIENTID;
    }
    az_put_u64(&b[AQ_COFF], b[AQ_CIDS].n);
    if (!enif_is_identical(q[2], A_UNDEFINED)) {
      ok = enif_inspect_binary(env, q[2], &bin);
      if (!ok) break;
      az_put(&b[AQ_UNS], bin.data, bin.size);
      flags |= EMQX_GM_AUTHZ_F_USERNAME;
    }
    az_put_u64(&b[AQ_UOFF], b[AQ_UNS].n);
    memset(peer, 0, sizeof(peer));
    if (!enif_is_identical(q[3], A_UNDEFINED)) {
      ok = enif_inspect_binary(env, q[3], &bin) && (bin.size == 4 || bin.size == 16);
      if (!ok) break;
      memcpy(peer, bin.data, bin.size);
      flags |= EMQX_GM_AUTHZ_F_PEERHOST | (bin.size == 16 ? EMQX_GM_AUTHZ_F_IPV6 : 0u);
    }
    az_put(&b[AQ_PEER], peer, 16);
    az_put_u8(&b[AQ_FLAGS], flags);
    ok = enif_get_uint(env, q[4], &u);
    az_put_u8(&b[AQ_ACTION], u);
    ok = ok && enif_get_uint(env, q[5], &u);
    az_put_u32(&b[AQ_MASK], u);
    ++n;
  }
  if (!ok) {
    az_free(b, AQ_NBUF);
    return enif_make_badarg(env);
  }
  memset(&batch, 0, sizeof(batch));
  batch.n = n;
  batch.topic_bytes = b[AQ_TOPICS].p;
  batch.topic_off = (const uint64_t *)b[AQ_TOFF].p;
  batch.clientid_bytes = b[AQ_CIDS].p;
  batch.clientid_off = (const uint64_t *)b[AQ_COFF].p;
  batch.username_bytes = b[AQ_UNS].p;
  batch.username_off = (const uint64_t *)b[AQ_UOFF].p;
  batch.flags = b[AQ_FLAGS].p;
  batch.peerhost = b[AQ_PEER].p;
  batch.action = b[AQ_ACTION].p;
  batch.re_mask = (const uint32_t *)b[AQ_MASK].p;
  verdict = enif_alloc(n ? n : 1);
  rule = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
  rc = emqx_gm_authz_check(CTX, r->tab, &batch, 0, verdict, rule);
  az_free(b, AQ_NBUF);
  if (rc != EMQX_GM_OK) {
    enif_free(verdict);
    enif_free(rule);
    return error_tuple(env, rc);
  }
  result = enif_make_list(env, 0);
  for (i = n; i > 0; --i)
    result = enif_make_list_cell(
        env, enif_make_tuple2(env, enif_make_uint(env, verdict[i - 1]), enif_make_uint(env, rule[i - 1])), result);
  enif_free(verdict);
  enif_free(rule);
  return result;
}

/* ---- subscription options at dispatch (emqx_gm_subopts_*, emqx_gm_deliver) ----
 * load_subopts(Index, [{Filter, SubId, Opt}], DefaultOpt) -> {ok, Table}
 * the ?SUBOPTION rows of emqx_broker:subscribe/3 (emqx_broker.erl:126-145) for
 * the pairs of the snapshot Index (from load_index/2): Opt is QoS bor (nl bsl 2)
 * bor (rap bsl 3) bor (upgrade_qos bsl 4); a pair without an entry gets
 * DefaultOpt.  An entry whose pair the snapshot does not hold is an error. */
static ERL_NIF_TERM load_subopts(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_index_res *ix;
  gm_subopts_res *res;
  unsigned len, i = 0, def;
  ERL_NIF_TERM h, t, *filters, list, term;
  uint8_t *fb, *opts;
  uint64_t *fo, n;
  uint32_t *subs;
  emqx_gm_subopts *so = NULL;
  int rc, ok = 1;
  (void)argc;
  if (!enif_get_resource(env, argv[0], INDEX_RT, (void **)&ix) || !enif_get_list_length(env, argv[1], &len) ||
      !enif_get_uint(env, argv[2], &def) || def > 255)
    return enif_make_badarg(env);
  filters = enif_alloc(sizeof(ERL_NIF_TERM) * (len ? len : 1));
  subs = enif_alloc(sizeof(uint32_t) * (len ? len : 1));
  opts = enif_alloc(len ? len : 1);
  t = argv[1];
  while (ok && enif_get_list_cell(env, t, &h, &t)) {
    const ERL_NIF_TERM *tup;
    int arity;
    unsigned s = 0, o = 0;
    /* (an Opt or DefaultOpt with bits 5-7 or QoS 3 fits a byte here and is refused by the library) */
    ok = enif_get_tuple(env, h, &arity, &tup) && arity == 3 && enif_get_uint(env, tup[1], &s) &&
         enif_get_uint(env, tup[2], &o) && o <= 255;
    if (ok) {
      filters[i] = tup[0];
      subs[i] = s;
      opts[i++] = (uint8_t)o;
    }
  }
  list = enif_make_list_from_array(env, filters, i);
  enif_free(filters);
  if (!ok || !pack_list(env, list, &fb, &fo, &n)) {
    enif_free(subs);
    enif_free(opts);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_subopts_build(CTX, ix->idx, fb, fo, subs, opts, n, (uint8_t)def, 0, &so);
  enif_free(subs);
  enif_free(opts);
  enif_free(fb);
  enif_free(fo);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  res = enif_alloc_resource(SUBOPTS_RT, sizeof(*res));
  res->so = so;
  res->idx = ix->idx; /* (kept alive by the table's own reference) */
  term = enif_make_resource(env, res);
  enif_release_resource(res);
  return enif_make_tuple2(env, A_OK, term);
}

/* deliver(Table, [Topic], [MsgFlags], [From], Mode :: 0 | 1) -> [{[{SubId, Byte}], Dropped}]
 * per topic, in batch order: the local deliveries of fanout_batch/2 over the
 * table's snapshot, each with the byte emqx_session:enrich_deliver/2 would
 * compute (QoS, retain bsl 2, nl bsl 3) -- so emqx_channel:handle_deliver/2
 * takes the bytes instead of calling ignore_local/4 and enrich_deliver/2 per
 * delivery.  MsgFlags: PubQoS bor (retain bsl 2) bor (retained-header bsl 3);
 * From: the publisher's SubId, or 16#FFFFFFFF.  Mode 0 marks a No-Local hit
 * with bit 4; Mode 1 removes it and counts it in Dropped
 * ('delivery.dropped.no_local').  The rows are matched on the table's own
 * snapshot, so they are always rows of the snapshot it is bound to. */
static ERL_NIF_TERM deliver_nif(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_subopts_res *r;
  uint8_t *tb, *mf;
  uint64_t *to, n, i, k;
  unsigned nf = 0, nfr = 0, mode, v = 0;
  uint32_t *from;
  emqx_gm_csr m;
  emqx_gm_deliveries d;
  ERL_NIF_TERM result, *rows, h, t;
  int rc, ok = 1;
  (void)argc;
  if (!enif_get_resource(env, argv[0], SUBOPTS_RT, (void **)&r) || !enif_get_list_length(env, argv[2], &nf) ||
      !enif_get_list_length(env, argv[3], &nfr) || !enif_get_uint(env, argv[4], &mode))
    return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  if (nf != n || nfr != n) {
    free_topics(tb, to);
    return enif_make_badarg(env);
  }
  mf = enif_alloc(n ? n : 1);
  from = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
  for (i = 0, t = argv[2]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v) && v <= 255; /* (bits 4-7 and QoS 3: refused by the library) */
    if (ok) mf[i] = (uint8_t)v;
  }
  for (i = 0, t = argv[3]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v);
    if (ok) from[i] = v;
  }
  if (!ok) {
    enif_free(mf);
    enif_free(from);
    free_topics(tb, to);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_match(CTX, r->idx, tb, to, n, EMQX_GM_WITH_EXACT, &m);
  free_topics(tb, to);
  if (rc == EMQX_GM_OK) {
    rc = emqx_gm_deliver(CTX, r->so, &m, mf, from, mode, &d);
    emqx_gm_csr_free(CTX, &m);
  }
  enif_free(mf);
  enif_free(from);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    for (k = d.deliveries.row_off[i + 1]; k > d.deliveries.row_off[i]; --k)
      row = enif_make_list_cell(
          env, enif_make_tuple2(env, enif_make_uint(env, d.deliveries.ids[k - 1]), enif_make_uint(env, d.dopt[k - 1])),
          row);
    rows[i] = enif_make_tuple2(env, row, enif_make_uint(env, d.row_dropped ? d.row_dropped[i] : 0));
  }
  result = enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_deliveries_free(CTX, &d);
  return result;
}

/* deliver_batches(Table, [Topic], [MsgFlags], [From], Mode :: 0 | 1 | 2) -> [{SubId, [{Filter, {Row, Byte}}]}]
 * by ascending SubId: the window's local deliveries grouped by subscriber
 * (emqx_gm_deliver_batches), each subscriber's in window order -- the list its
 * connection process would drain from its mailbox (emqx_misc:drain_deliver/1)
 * and hand to emqx_channel:handle_deliver/2.  Filter is the deliver's Topic,
 * Row the 0-based position of the message in [Topic], Byte as deliver/5 gives
 * it.  Mode 2 removes each list's leading run of No-Local hits, as
 * emqx_session:ignore_local/4 does over a drained batch, and clears bit 4; a
 * list it empties stays in the result as {SubId, []}.  Arguments otherwise as
 * deliver/5 takes them. */
static ERL_NIF_TERM deliver_batches_nif(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_subopts_res *r;
  uint8_t *tb, *mf;
  uint64_t *to, n, i, j, k;
  unsigned nf = 0, nfr = 0, mode, v = 0;
  uint32_t *from;
  emqx_gm_csr m;
  emqx_gm_batches b;
  ERL_NIF_TERM result, h, t;
  int rc, ok = 1;
  (void)argc;
  if (!enif_get_resource(env, argv[0], SUBOPTS_RT, (void **)&r) || !enif_get_list_length(env, argv[2], &nf) ||
      !enif_get_list_length(env, argv[3], &nfr) || !enif_get_uint(env, argv[4], &mode))
    return enif_make_badarg(env);
  if (!pack_topics(env, argv[1], &tb, &to, &n)) return enif_make_badarg(env);
  if (nf != n || nfr != n) {
    free_topics(tb, to);
    return enif_make_badarg(env);
  }
  mf = enif_alloc(n ? n : 1);
  from = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
  for (i = 0, t = argv[2]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v) && v <= 255; /* (bits 4-7 and QoS 3: refused by the library) */
    if (ok) mf[i] = (uint8_t)v;
  }
  for (i = 0, t = argv[3]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v);
    if (ok) from[i] = v;
  }
  if (!ok) {
    enif_free(mf);
    enif_free(from);
    free_topics(tb, to);
    return enif_make_badarg(env);
  }
  rc = emqx_gm_match(CTX, r->idx, tb, to, n, EMQX_GM_WITH_EXACT, &m);
  free_topics(tb, to);
  if (rc == EMQX_GM_OK) {
    rc = emqx_gm_deliver_batches(CTX, r->so, &m, mf, from, mode, &b);
    emqx_gm_csr_free(CTX, &m);
  }
  enif_free(mf);
  enif_free(from);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  result = enif_make_list(env, 0);
  for (j = b.n_batches; j > 0; --j) { /* (built back to front: the result ascends) */
    ERL_NIF_TERM list = enif_make_list(env, 0);
    for (k = b.batch_off[j]; k > b.batch_off[j - 1]; --k) {
      const uint8_t *p = NULL;
      uint64_t l = 0;
      if (emqx_gm_index_filter(r->idx, b.filters[k - 1], &p, &l) != EMQX_GM_OK) {
        emqx_gm_batches_free(CTX, &b);
        return error_tuple(env, EMQX_GM_EINVAL);
      }
      list = enif_make_list_cell(env,
                                 enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l),
                                                  enif_make_tuple2(env, enif_make_uint(env, b.rows[k - 1]),
                                                                   enif_make_uint(env, b.dopt[k - 1]))),
                                 list);
    }
    result = enif_make_list_cell(env, enif_make_tuple2(env, enif_make_uint(env, b.subs[j - 1]), list), result);
  }
  emqx_gm_batches_free(CTX, &b);
  return result;
}

/* publish_window_deliver_nif(Shared, SubOpts, [Topic], Strategy :: 0..3, [Hash], Seed, [MsgFlags], [From],
 *                            Mode :: 0 | 1) -> [{{[{SubId, Byte}], Dropped}, [{Filter, {GroupId, MemberId}}]}]
 * per topic, in batch order: what deliver/5 gives for it and what pick_shared_nif/5
 * gives for it, from ONE emqx_gm_publish_window_deliver -- the deliveries with
 * their option bytes run as a third part of the window's one device round trip,
 * in place of the plain fan-out.  Both tables must be bound to the same snapshot
 * (from load_index/2); the library refuses another pairing. */
static ERL_NIF_TERM publish_window_deliver_nif(ErlNifEnv *env, int argc, const ERL_NIF_TERM argv[]) {
  gm_shared_res *r;
  gm_subopts_res *so;
  uint8_t *tb, *mf;
  uint64_t *to, n, i, k;
  unsigned strategy, seed, nh = 0, nf = 0, nfr = 0, mode, v = 0;
  uint32_t *hash, *from;
  emqx_gm_publish_opts o;
  emqx_gm_publish_deliver_opts dopts;
  emqx_gm_publish_result w;
  emqx_gm_deliveries d;
  ERL_NIF_TERM result, *rows, h, t;
  int rc, ok = 1, bad = 0;
  (void)argc;
  if (!enif_get_resource(env, argv[0], SHARED_RT, (void **)&r) ||
      !enif_get_resource(env, argv[1], SUBOPTS_RT, (void **)&so) || !enif_get_uint(env, argv[3], &strategy) ||
      !enif_get_list_length(env, argv[4], &nh) || !enif_get_uint(env, argv[5], &seed) ||
      !enif_get_list_length(env, argv[6], &nf) || !enif_get_list_length(env, argv[7], &nfr) ||
      !enif_get_uint(env, argv[8], &mode))
    return enif_make_badarg(env);
  if (!pack_topics(env, argv[2], &tb, &to, &n)) return enif_make_badarg(env);
  if (nf != n || nfr != n || (strategy == EMQX_GM_SHARE_HASH && nh != n)) {
    free_topics(tb, to);
    return enif_make_badarg(env);
  }
  hash = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
  mf = enif_alloc(n ? n : 1);
  from = enif_alloc(sizeof(uint32_t) * (n ? n : 1));
  if (strategy == EMQX_GM_SHARE_HASH)
    for (i = 0, t = argv[4]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
      ok = enif_get_uint(env, h, &v);
      if (ok) hash[i] = v;
    }
  for (i = 0, t = argv[6]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v) && v <= 255; /* (bits 4-7 and QoS 3: refused by the library) */
    if (ok) mf[i] = (uint8_t)v;
  }
  for (i = 0, t = argv[7]; ok && enif_get_list_cell(env, t, &h, &t); ++i) {
    ok = enif_get_uint(env, h, &v);
    if (ok) from[i] = v;
  }
  rc = EMQX_GM_OK;
  if (ok) {
    memset(&o, 0, sizeof(o));
    o.flags = EMQX_GM_WITH_EXACT;
    o.shared = r->sh;
    o.strategy = strategy;
    o.seed = seed;
    o.msg_hash = strategy == EMQX_GM_SHARE_HASH ? hash : NULL;
    memset(&dopts, 0, sizeof(dopts));
    dopts.subopts = so->so;
    dopts.msg_flags = mf;
    dopts.msg_from = from;
    dopts.mode = mode;
    rc = emqx_gm_publish_window_deliver(CTX, r->idx, tb, to, n, &o, &dopts, &w, &d, NULL);
  }
  free_topics(tb, to);
  enif_free(hash);
  enif_free(mf);
  enif_free(from);
  if (!ok) return enif_make_badarg(env);
  if (rc != EMQX_GM_OK) return error_tuple(env, rc);
  rows = enif_alloc(sizeof(ERL_NIF_TERM) * (n ? n : 1));
  for (i = 0; i < n && !bad; ++i) {
    ERL_NIF_TERM row = enif_make_list(env, 0), picks = enif_make_list(env, 0);
    for (k = d.deliveries.row_off[i + 1]; k > d.deliveries.row_off[i]; --k)
      row = enif_make_list_cell(
          env, enif_make_tuple2(env, enif_make_uint(env, d.deliveries.ids[k - 1]), enif_make_uint(env, d.dopt[k - 1])),
          row);
    for (k = w.pick_members.row_off[i + 1]; k > w.pick_members.row_off[i] && !bad; --k) {
      const uint8_t *p = NULL;
      uint64_t l = 0;
      uint32_t f = 0, g = 0;
      if (emqx_gm_shared_slot(r->sh, w.pick_slots.ids[k - 1], &f, &g, NULL, NULL) != EMQX_GM_OK ||
          emqx_gm_index_filter(r->idx, f, &p, &l) != EMQX_GM_OK) {
        bad = 1;
        break;
      }
      picks = enif_make_list_cell(
          env,
          enif_make_tuple2(env, enif_make_resource_binary(env, r, p, l),
                           enif_make_tuple2(env, enif_make_uint(env, g), enif_make_uint(env, w.pick_members.ids[k - 1]))),
          picks);
    }
    rows[i] = enif_make_tuple2(
        env, enif_make_tuple2(env, row, enif_make_uint(env, d.row_dropped ? d.row_dropped[i] : 0)), picks);
  }
  result = bad ? error_tuple(env, EMQX_GM_EINVAL) : enif_make_list_from_array(env, rows, (unsigned)n);
  enif_free(rows);
  emqx_gm_publish_result_free(CTX, &w);
  emqx_gm_deliveries_free(CTX, &d);
  return result;
}

static ErlNifFunc funcs[] = {
    {"load_index", 1, load_index, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_index", 2, load_index, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_index_sharded", 1, load_index_sharded, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_index_sharded", 2, load_index_sharded, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"update_index", 2, update_index, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"update_subs", 2, update_subs, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"match_batch", 2, match_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"match_routes_batch", 2, match_routes_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"fanout_batch", 2, fanout_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"empty", 1, empty, 0},
    {"export_index", 1, export_index, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"import_index", 1, import_index, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_retained", 1, load_retained, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_retained", 2, load_retained, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"match_retained", 3, match_retained, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"expire_retained", 2, expire_retained, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_shared", 3, load_shared, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_shared", 4, load_shared, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"pick_shared_nif", 5, pick_shared_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"publish_window_nif", 5, publish_window_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_subopts", 3, load_subopts, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"deliver", 5, deliver_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"deliver_batches", 5, deliver_batches_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"publish_window_deliver_nif", 9, publish_window_deliver_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"load_authz", 1, load_authz, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"authorize_batch", 2, authorize_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
};

ERL_NIF_INIT(emqx_gpu_match, funcs, load, NULL, NULL, unload)
