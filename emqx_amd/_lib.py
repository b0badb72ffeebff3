"""ctypes binding of libemqx_gpu_match.so (include/emqx_gpu_match.h + emqx_gm_ext.h).

The HIP library is the only compute path: if it is missing, or no device is
visible, every compute call raises :class:`GpuMatchError` — there is no CPU
fallback.
"""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EMQX_GM_LIB") or os.path.join(_HERE, "libemqx_gpu_match.so")

OK, EINVAL, ENOMEM, EDEVICE, EOVERFLOW, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
WITH_EXACT = 0x1
DEVICE_IO = 0x2
NO_TIMING = 0x4
RET_TIMED = 0x1
AUTHZ_TIMED = 0x1
SHARE_HASH, SHARE_ROUND_ROBIN, SHARE_STICKY, SHARE_RANDOM = 0, 1, 2, 3
DESTS_MAX_NODES = 4096
DESTS_NO_SKIP = 0xFFFFFFFF
DESTS_SKIP_UNKNOWN = 0x1
SO_SKIP_UNKNOWN = 0x1
SO_NO_PUBLISHER = 0xFFFFFFFF
SO_FLAG, SO_DROP = 0, 1
SO_LEAD = 2  # emqx_gm_deliver_batches only
OPEN_MIRROR_EAGER = 0x1
OPEN_MIRROR_LAZY = 0x2
IMAGE_NO_BLOB = 0x1

ERRNAMES = {EINVAL: "EINVAL", ENOMEM: "ENOMEM", EDEVICE: "EDEVICE", EOVERFLOW: "EOVERFLOW",
            EUNSUPPORTED: "EUNSUPPORTED"}


class GpuMatchError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"{ERRNAMES.get(code, code)}: {msg}")


MAX_DEVICES = 8


class Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("n_devices", C.c_uint32),
                ("devices", C.c_int32 * MAX_DEVICES), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class Csr(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("nnz", C.c_uint64), ("row_off", C.POINTER(C.c_uint64)),
                ("ids", C.POINTER(C.c_uint32)), ("on_device", C.c_int32), ("reserved0", C.c_int32),
                ("priv", C.c_void_p)]


class Window(C.Structure):
    _fields_ = [("topic_bytes", C.c_void_p), ("topic_off", C.c_void_p), ("n_topics", C.c_uint64)]


class CombinerOpts(C.Structure):
    _fields_ = [("max_windows", C.c_uint32), ("max_topics", C.c_uint64), ("max_in_flight", C.c_uint32),
                ("min_windows", C.c_uint32), ("linger_us", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class CombinerStats(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("groups", C.c_uint64), ("max_group", C.c_uint64), ("solo", C.c_uint64)]


class IndexInfo(C.Structure):
    _fields_ = [("n_filters", C.c_uint64), ("n_wildcard", C.c_uint64), ("n_nodes", C.c_uint64),
                ("n_edges", C.c_uint64), ("n_words", C.c_uint64), ("n_subs", C.c_uint64),
                ("device_bytes", C.c_uint64), ("max_depth", C.c_uint32), ("trie_empty", C.c_int32)]


class MatchStats(C.Structure):
    _fields_ = [("n_topics", C.c_uint64), ("nnz", C.c_uint64), ("n_overflow", C.c_uint64),
                ("n_wildcard_topics", C.c_uint64), ("match_kernel_ms", C.c_double),
                ("total_device_ms", C.c_double), ("algo_bytes", C.c_uint64), ("probes", C.c_uint64)]


class UpdateStats(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("replica_mode", C.c_uint32), ("replicas", C.c_uint32),
                ("mirror_loaded", C.c_int32), ("mirror_bytes", C.c_uint64), ("mirror_ms", C.c_double),
                ("device_ms", C.c_double), ("replicate_ms", C.c_double), ("total_ms", C.c_double),
                ("blobs_reused", C.c_uint32), ("blobs_fresh", C.c_uint32)]


class RetainedInfo(C.Structure):
    _fields_ = [("n_topics", C.c_uint64), ("n_nodes", C.c_uint64), ("n_words", C.c_uint64),
                ("device_bytes", C.c_uint64), ("widest_level", C.c_uint64), ("walk_ws_bytes", C.c_uint64),
                ("depth_max", C.c_uint32), ("lds_frames", C.c_int32)]


class SharedInfo(C.Structure):
    _fields_ = [("n_slots", C.c_uint64), ("n_members", C.c_uint64), ("n_filters_with_slots", C.c_uint64),
                ("device_bytes", C.c_uint64)]


class DestsInfo(C.Structure):
    _fields_ = [("n_routes", C.c_uint64), ("n_filters_with_routes", C.c_uint64), ("n_skipped_unknown", C.c_uint64),
                ("device_bytes", C.c_uint64), ("n_nodes", C.c_uint32), ("reserved0", C.c_uint32)]


class Forwards(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_pairs", C.c_uint64), ("node_off", C.POINTER(C.c_uint64)),
                ("rows", C.POINTER(C.c_uint32)), ("filters", C.POINTER(C.c_uint32)),
                ("row_routes", C.POINTER(C.c_uint32)), ("n_nodes", C.c_uint32), ("on_device", C.c_int32),
                ("priv", C.c_void_p)]


class SubOptsInfo(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_defaulted", C.c_uint64), ("n_nl", C.c_uint64),
                ("n_skipped_unknown", C.c_uint64), ("device_bytes", C.c_uint64)]


class Deliveries(C.Structure):
    _fields_ = [("deliveries", Csr), ("dopt", C.POINTER(C.c_uint8)), ("row_dropped", C.POINTER(C.c_uint32)),
                ("n_dropped", C.c_uint64)]


class Batches(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_deliveries", C.c_uint64), ("n_batches", C.c_uint64),
                ("n_dropped", C.c_uint64), ("subs", C.POINTER(C.c_uint32)), ("batch_off", C.POINTER(C.c_uint64)),
                ("rows", C.POINTER(C.c_uint32)), ("filters", C.POINTER(C.c_uint32)), ("dopt", C.POINTER(C.c_uint8)),
                ("batch_dropped", C.POINTER(C.c_uint32)), ("on_device", C.c_int32), ("priv", C.c_void_p)]


class PublishOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("shared", C.c_void_p), ("strategy", C.c_uint32), ("seed", C.c_uint32),
                ("msg_hash", C.c_void_p), ("dests", C.c_void_p), ("skip_node", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


class PublishResult(C.Structure):
    _fields_ = [("matches", Csr), ("deliveries", Csr), ("pick_members", Csr), ("pick_slots", Csr),
                ("forwards", Forwards)]


class PublishStats(C.Structure):
    _fields_ = [("device_waits", C.c_uint32), ("rows_spec", C.c_uint8), ("fanout_spec", C.c_uint8),
                ("picks_spec", C.c_uint8), ("forwards_spec", C.c_uint8), ("n_hits", C.c_uint64),
                ("n_pairs", C.c_uint64), ("cap_hits", C.c_uint64), ("cap_pairs", C.c_uint64)]


class PublishDeliverOpts(C.Structure):
    _fields_ = [("subopts", C.c_void_p), ("msg_flags", C.c_void_p), ("msg_from", C.c_void_p), ("mode", C.c_uint32)]


class PublishDeliverStats(C.Structure):
    _fields_ = [("window", PublishStats), ("deliveries_spec", C.c_uint8), ("n_deliveries", C.c_uint64),
                ("n_dropped", C.c_uint64), ("cap_deliveries", C.c_uint64)]


class PublishWin(C.Structure):
    _fields_ = [("w", Window), ("msg_hash", C.c_void_p)]


class PublishGroupStats(C.Structure):
    _fields_ = [("seq", C.c_uint64), ("position", C.c_uint32), ("n_windows", C.c_uint32),
                ("device_waits", C.c_uint32), ("grouped", C.c_uint8), ("rows_spec", C.c_uint8),
                ("picks_spec", C.c_uint8), ("forwards_spec", C.c_uint8), ("window_picks_exact", C.c_uint8),
                ("window_forwards_exact", C.c_uint8), ("reserved8", C.c_uint8 * 6), ("cap_hits", C.c_uint64),
                ("cap_pairs", C.c_uint64), ("n_hits", C.c_uint64), ("n_pairs", C.c_uint64)]


class AuthzDesc(C.Structure):
    _fields_ = [("n_segments", C.c_uint32), ("seg_kind", C.c_void_p), ("seg_range_off", C.c_void_p),
                ("n_ranges", C.c_uint64), ("range_rule_off", C.c_void_p), ("key_bytes", C.c_void_p),
                ("key_off", C.c_void_p), ("n_rules", C.c_uint64), ("rule_id", C.c_void_p),
                ("rule_perm", C.c_void_p), ("rule_action", C.c_void_p), ("rule_who_op", C.c_void_p),
                ("rule_who_off", C.c_void_p), ("rule_filter_off", C.c_void_p), ("n_leaves", C.c_uint64),
                ("leaf_kind", C.c_void_p), ("leaf_bytes", C.c_void_p), ("leaf_off", C.c_void_p),
                ("n_filters", C.c_uint64), ("filter_kind", C.c_void_p), ("filter_bytes", C.c_void_p),
                ("filter_off", C.c_void_p)]


class AuthzBatch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("topic_bytes", C.c_void_p), ("topic_off", C.c_void_p),
                ("clientid_bytes", C.c_void_p), ("clientid_off", C.c_void_p), ("username_bytes", C.c_void_p),
                ("username_off", C.c_void_p), ("flags", C.c_void_p), ("peerhost", C.c_void_p),
                ("action", C.c_void_p), ("re_mask", C.c_void_p)]


class AuthzInfo(C.Structure):
    _fields_ = [("build_ms", C.c_double), ("device_bytes", C.c_uint64), ("n_rules", C.c_uint64),
                ("n_keys", C.c_uint64), ("n_words", C.c_uint64), ("n_filters", C.c_uint64),
                ("n_leaves", C.c_uint64), ("n_segments", C.c_uint32), ("deepest_filter", C.c_uint32),
                ("longest_range", C.c_uint64)]


UPD_KINDS = {0: "none", 1: "patch", 2: "overlay", 3: "rebuild", 4: "subs_only", 5: "build", 6: "import", 7: "shift"}
REP_MODES = {0: "none", 1: "patched", 2: "copied", 3: "shared", 4: "sharded"}


# Every symbol declared in include/emqx_gpu_match.h and include/emqx_gm_ext.h.
_vp, _u64, _i32, _u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32
SIGNATURES = {
    # emqx_gpu_match.h
    "emqx_gm_open": (_i32, [C.POINTER(Opts), C.POINTER(_vp)]),
    "emqx_gm_close": (_i32, [_vp]),
    "emqx_gm_last_error": (C.c_char_p, [_vp]),
    "emqx_gm_abi_version": (_i32, []),
    "emqx_gm_set_stream": (_i32, [_vp, _vp]),
    "emqx_gm_synchronize": (_i32, [_vp]),
    "emqx_gm_index_build": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "emqx_gm_index_update": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp)]),
    "emqx_gm_index_update_subs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp)]),
    "emqx_gm_index_export": (_i32, [_vp, _vp, _u32, _vp, C.POINTER(_u64)]),
    "emqx_gm_index_device_blob": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    "emqx_gm_index_import": (_i32, [_vp, _vp, _u64, _vp, C.POINTER(_vp)]),
    "emqx_gm_index_retain": (_i32, [_vp]),
    "emqx_gm_index_release": (_i32, [_vp]),
    "emqx_gm_index_info": (_i32, [_vp, C.POINTER(IndexInfo)]),
    "emqx_gm_index_filter": (_i32, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u64)]),
    "emqx_gm_index_subscriber_count": (_i32, [_vp, _u32, C.POINTER(_u64)]),
    "emqx_gm_match": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(Csr)]),
    "emqx_gm_match_submit": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(_vp)]),
    "emqx_gm_match_wait": (_i32, [_vp, _vp, C.POINTER(Csr)]),
    "emqx_gm_host_alloc": (_i32, [_vp, _u64, C.POINTER(_vp)]),
    "emqx_gm_host_free": (_i32, [_vp, _vp]),
    "emqx_gm_devices": (_i32, [_vp, _vp, C.POINTER(_u32)]),
    "emqx_gm_fanout": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, C.POINTER(Csr)]),
    "emqx_gm_match_fanout": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(Csr), C.POINTER(Csr)]),
    "emqx_gm_match_windows": (_i32, [_vp, _vp, C.POINTER(Window), _u32, _u32, C.POINTER(Csr), C.POINTER(Csr)]),
    "emqx_gm_combiner_open": (_i32, [_vp, C.POINTER(CombinerOpts), C.POINTER(_vp)]),
    "emqx_gm_combiner_match": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(Csr), C.POINTER(Csr)]),
    "emqx_gm_combiner_stats": (_i32, [_vp, C.POINTER(CombinerStats)]),
    "emqx_gm_combiner_close": (_i32, [_vp]),
    "emqx_gm_csr_free": (_i32, [_vp, C.POINTER(Csr)]),
    "emqx_gm_last_stats": (_i32, [_vp, C.POINTER(MatchStats)]),
    "emqx_gm_filter_ranks": (_i32, [_vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "emqx_gm_shard_of": (_i32, [_vp, _vp, _u64, _u32, _vp]),
    "emqx_gm_index_build_shard": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "emqx_gm_index_build_sharded": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "emqx_gm_csr_row_lengths": (_i32, [_vp, C.POINTER(Csr), _vp]),
    "emqx_gm_merge_rows": (_i32, [_vp, _u64, _u64, _u32, _vp, _vp, _u32, C.POINTER(Csr)]),
    "emqx_gm_prefix_plan": (_i32, [_vp, _vp, _u64, _u32, _vp, C.POINTER(_vp)]),
    "emqx_gm_route_topics_host": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "emqx_gm_route_topics": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "emqx_gm_route_release": (_i32, [_vp]),
    "emqx_gm_route_partition": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "emqx_gm_permute_topics": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "emqx_gm_unpermute_rows": (_i32, [_vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(Csr)]),
    "emqx_gm_retained_build": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u32, C.POINTER(_vp)]),
    "emqx_gm_retained_match": (_i32, [_vp, _vp, _vp, _vp, _u64, _u64, _u32, C.POINTER(Csr)]),
    "emqx_gm_retained_expire": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "emqx_gm_retained_info": (_i32, [_vp, C.POINTER(RetainedInfo)]),
    "emqx_gm_retained_release": (_i32, [_vp]),
    "emqx_gm_shared_build": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_vp)]),
    "emqx_gm_shared_pick": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, _vp, _u32, C.POINTER(Csr), C.POINTER(Csr)]),
    "emqx_gm_shared_slot": (_i32, [_vp, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_vp), C.POINTER(_u64)]),
    "emqx_gm_shared_info": (_i32, [_vp, C.POINTER(SharedInfo)]),
    "emqx_gm_shared_release": (_i32, [_vp]),
    "emqx_gm_dests_build": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, C.POINTER(_vp)]),
    "emqx_gm_forward_plan": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, C.POINTER(Forwards)]),
    "emqx_gm_forwards_free": (_i32, [_vp, C.POINTER(Forwards)]),
    "emqx_gm_dests_info": (_i32, [_vp, C.POINTER(DestsInfo)]),
    "emqx_gm_dests_release": (_i32, [_vp]),
    "emqx_gm_subopts_build": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, C.c_uint8, _u32, C.POINTER(_vp)]),
    "emqx_gm_deliver": (_i32, [_vp, _vp, C.POINTER(Csr), _vp, _vp, _u32, C.POINTER(Deliveries)]),
    "emqx_gm_subopts_index": (_vp, [_vp]),
    "emqx_gm_deliveries_free": (_i32, [_vp, C.POINTER(Deliveries)]),
    "emqx_gm_subopts_info": (_i32, [_vp, C.POINTER(SubOptsInfo)]),
    "emqx_gm_deliver_batches": (_i32, [_vp, _vp, C.POINTER(Csr), _vp, _vp, _u32, C.POINTER(Batches)]),
    "emqx_gm_batches_free": (_i32, [_vp, C.POINTER(Batches)]),
    "emqx_gm_subopts_release": (_i32, [_vp]),
    "emqx_gm_publish_window": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(PublishOpts), C.POINTER(PublishResult),
                                      C.POINTER(PublishStats)]),
    "emqx_gm_publish_result_free": (_i32, [_vp, C.POINTER(PublishResult)]),
    "emqx_gm_publish_window_deliver": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(PublishOpts),
                                              C.POINTER(PublishDeliverOpts), C.POINTER(PublishResult),
                                              C.POINTER(Deliveries), C.POINTER(PublishDeliverStats)]),
    "emqx_gm_publish_windows": (_i32, [_vp, _vp, C.POINTER(PublishWin), _u32, C.POINTER(PublishOpts),
                                       C.POINTER(PublishResult), C.POINTER(PublishStats),
                                       C.POINTER(PublishGroupStats)]),
    "emqx_gm_combiner_publish": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(PublishOpts), C.POINTER(PublishResult),
                                        C.POINTER(PublishStats), C.POINTER(PublishGroupStats)]),
    "emqx_gm_authz_build": (_i32, [_vp, C.POINTER(AuthzDesc), _u32, C.POINTER(_vp)]),
    "emqx_gm_authz_check": (_i32, [_vp, _vp, C.POINTER(AuthzBatch), _u32, _vp, _vp]),
    "emqx_gm_authz_info": (_i32, [_vp, C.POINTER(AuthzInfo)]),
    "emqx_gm_authz_release": (_i32, [_vp]),
    # emqx_gm_ext.h
    "emqx_gm_gen_filter_codes": (_i32, [_u64, _u64, _i32, _vp]),
    "emqx_gm_render_codes": (_u64, [_vp, _u64, _vp, _vp]),
    "emqx_gm_gen_topics": (_i32, [_vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(_vp), C.POINTER(_vp),
                                  C.POINTER(_u64)]),
    "emqx_gm_dev_alloc": (_i32, [_vp, _u64, C.POINTER(_vp)]),
    "emqx_gm_dev_free": (_i32, [_vp, _vp]),
    "emqx_gm_memcpy": (_i32, [_vp, _vp, _vp, _u64, _i32]),
    "emqx_gm_pool_trim": (_i32, [_vp]),
    "emqx_gm_index_compile_host": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(IndexInfo)]),
    "emqx_gm_matched_filter_bytes": (_i32, [_vp, _vp, C.POINTER(Csr), C.POINTER(_u64)]),
    "emqx_gm_fanout_part": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, _u32, _u32, C.POINTER(Csr), C.POINTER(_u64)]),
    "emqx_gm_select_filters": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "emqx_gm_last_update_stats": (_i32, [_vp, C.POINTER(UpdateStats)]),
    "emqx_gm_index_replica_digest": (_i32, [_vp, _vp, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "emqx_gm_last_shard_update": (_i32, [_vp, _vp, C.POINTER(_u32)]),
    "emqx_gm_route_filter_shards_host": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "emqx_gm_retained_compile_host": (_i32, [_vp, _vp, _u64, _vp, _vp, C.POINTER(_vp)]),
    "emqx_gm_retained_match_host": (_i32, [_vp, _vp, _vp, _u64, _u64, C.POINTER(Csr)]),
    "emqx_gm_retained_csr_free_host": (_i32, [C.POINTER(Csr)]),
    "emqx_gm_retained_last_times": (_i32, [_vp, C.POINTER(C.c_double)]),
    "emqx_gm_shared_compile_host": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "emqx_gm_shared_pick_host": (_i32, [_vp, C.POINTER(Csr), _u32, _vp, _u32, C.POINTER(Csr), C.POINTER(Csr)]),
    "emqx_gm_shared_csr_free_host": (_i32, [C.POINTER(Csr)]),
    "emqx_gm_shared_pick_chunked": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, _vp, _u32, _u32, C.POINTER(Csr),
                                           C.POINTER(Csr)]),
    "emqx_gm_shared_last_times": (_i32, [_vp, C.POINTER(C.c_double)]),
    "emqx_gm_dests_compile_host": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _u32, _u32, C.POINTER(_vp)]),
    "emqx_gm_forward_plan_host": (_i32, [_vp, C.POINTER(Csr), _u32, C.POINTER(Forwards)]),
    "emqx_gm_forwards_free_host": (_i32, [C.POINTER(Forwards)]),
    "emqx_gm_forward_plan_chunked": (_i32, [_vp, _vp, C.POINTER(Csr), _u32, _u32, C.POINTER(Forwards)]),
    "emqx_gm_dests_last_times": (_i32, [_vp, C.POINTER(C.c_double)]),
    "emqx_gm_subopts_compile_host": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.c_uint8, _u32,
                                            C.POINTER(_vp)]),
    "emqx_gm_deliver_host": (_i32, [_vp, C.POINTER(Csr), _vp, _vp, _u32, C.POINTER(Deliveries)]),
    "emqx_gm_deliveries_free_host": (_i32, [C.POINTER(Deliveries)]),
    "emqx_gm_subopts_last_times": (_i32, [_vp, C.POINTER(C.c_double)]),
    "emqx_gm_deliver_batches_host": (_i32, [_vp, C.POINTER(Csr), _vp, _vp, _u32, C.POINTER(Batches)]),
    "emqx_gm_batches_free_host": (_i32, [C.POINTER(Batches)]),
    "emqx_gm_deliver_batches_chunked": (_i32, [_vp, _vp, C.POINTER(Csr), _vp, _vp, _u32, _u32, C.POINTER(Batches)]),
    "emqx_gm_batches_last_times": (_i32, [_vp, C.POINTER(C.c_double)]),
    "emqx_gm_authz_compile_host": (_i32, [C.POINTER(AuthzDesc), C.POINTER(_vp)]),
    "emqx_gm_authz_check_host": (_i32, [_vp, C.POINTER(AuthzBatch), _vp, _vp]),
    "emqx_gm_authz_last_kernel_ms": (_i32, [_vp, C.POINTER(C.c_double)]),
}

_LIB = None


def _one_hip_runtime():
    """torch-ROCm ships its own HIP / HSA runtime (torch/lib/libamdhip64.so,
    SONAME libamdhip64.so.7, the same as /opt/rocm's).  Loaded before it, the
    library would pull /opt/rocm's copy in and torch would still load its own
    by path: two HSA runtimes in one process, and whichever initialises second
    finds no device (round 5: a host-only call such as gen_filter_codes before
    the first Context, then torch.cuda, then emqx_gm_open -> EDEVICE;
    scripts/smoke_order_diag.py).  Importing torch first makes the library
    bind to torch's runtime by SONAME: one runtime.  A process without torch
    loads /opt/rocm's."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    """Load the HIP library; raise loudly if it is not built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GpuMatchError(EUNSUPPORTED, f"{LIB_PATH} is not built (run __graft_entry__.build() "
                                              f"or `make -C emqx_amd/csrc`)")
        _one_hip_runtime()
        L = C.CDLL(LIB_PATH)
        # an older build loaded for a same-box A/B (EMQX_GM_LIB) may lack the newest
        # entry points: those stay unbound there; the shipped library must have them all
        ab = bool(os.environ.get("EMQX_GM_LIB"))
        for name, (res, args) in SIGNATURES.items():
            if ab and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def check(rc: int, ctx=None, what: str = ""):
    if rc != OK:
        msg = ""
        if ctx:
            m = lib().emqx_gm_last_error(ctx)
            msg = m.decode(errors="replace") if m else ""
        raise GpuMatchError(rc, f"{what}: {msg}")
    return rc
