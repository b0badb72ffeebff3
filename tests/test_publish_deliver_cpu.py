"""The publish window with option bytes without a device: the library exports
emqx_gm_publish_window_deliver, the header declares it with its structs and
lists its knob, and PublishBatcher(one_call=True, subopts=True, shared=,
cluster=) over a stand-in ``routes.window`` makes one window call per window
with the messages' bytes and publishers, hands the bytes to ``deliver``, counts
the No-Local drops, and treats picks and forwards as it does without
``subopts`` (the device path: tests/test_gpu_publish_deliver.py)."""

import os
import re

import numpy as np
import pytest

from emqx_amd import _lib
from emqx_amd.batcher import PublishBatcher, _IdsOpts
from emqx_amd.subopts import pack_msg
from tests.test_publish_window_cpu import (FILTERS, GROUPS, LOCAL, NODE_ROUTES, NODES, _Cluster, _Index, _match,
                                           _Shared)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_header_and_knob():
    L = _lib.lib()
    assert hasattr(L, "emqx_gm_publish_window_deliver") and "emqx_gm_publish_window_deliver" in _lib.SIGNATURES
    h = open(os.path.join(ROOT, "include", "emqx_gpu_match.h")).read()
    assert re.search(r"\bint emqx_gm_publish_window_deliver\(", h)
    for struct in ("emqx_gm_publish_deliver_opts", "emqx_gm_publish_deliver_stats"):
        assert re.search(r"\}\s*%s;" % struct, h), struct
    env = h[h.index(" * Environment:"):h.index("*/", h.index(" * Environment:"))]
    assert "GM_PW_CAP_DELIVERIES" in set(re.findall(r"\bGM_[A-Z0-9_]+", env))
    srcs = "".join(open(os.path.join(ROOT, "emqx_amd", "csrc", f)).read()
                   for f in os.listdir(os.path.join(ROOT, "emqx_amd", "csrc")) if f.endswith((".hip", ".cpp", ".h")))
    assert 'knob("GM_PW_CAP_DELIVERIES")' in srcs
    # the ctypes mirror of the two structs: the layout the header gives on LP64
    O, S = _lib.PublishDeliverOpts, _lib.PublishDeliverStats
    assert (O.subopts.offset, O.msg_flags.offset, O.msg_from.offset, O.mode.offset, _lib.C.sizeof(O)) == (0, 8, 16, 24, 32)
    w = _lib.C.sizeof(_lib.PublishStats)
    assert (S.window.offset, S.deliveries_spec.offset, S.n_deliveries.offset, S.n_dropped.offset,
            S.cap_deliveries.offset, _lib.C.sizeof(S)) == (0, w, w + 8, w + 16, w + 24, w + 32)
    # the NIF shim and its Erlang module carry the call
    nif = open(os.path.join(ROOT, "nif", "emqx_gpu_match_nif.c")).read()
    erl = open(os.path.join(ROOT, "nif", "emqx_gpu_match.erl")).read()
    assert "emqx_gm_publish_window_deliver(CTX" in nif and '{"publish_window_deliver_nif", 9,' in nif
    assert "publish_window_deliver/7" in erl and "publish_window_deliver_nif/9" in erl


# ---- the stand-in world of test_publish_window_cpu.py, its local subscribers with a No-Local rule:
# a delivery to the message's own publisher is a No-Local hit (bit 4); the byte's low bits are the message's
SUBS = {0: "local0", 1: "local1", 2: "local2"}


class _Routes:
    """Stand-in for GpuRoutes: ``window`` with ``opts`` and the two-call path's ``groups_opts``."""

    def __init__(self):
        self.index, self.subs = _Index(), dict(SUBS)
        self.ids = {v: k for k, v in SUBS.items()}
        self.other = {FILTERS[f]: 1 for f in set(NODE_ROUTES) | set(GROUPS)}
        self.window_calls, self.opts_calls = [], 0

    def _csr(self, topics):
        rows = [_match(t) for t in topics]
        ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        return rows, (ro, np.array([f for r in rows for f in r], np.uint32))

    def _cut(self, rows, flags, froms, drop):
        out = []
        for r, row in enumerate(rows):
            cut = []
            for f in row:
                ids = np.array(LOCAL.get(f, []), np.uint32)
                dopt = np.array([flags[r] | (0x10 if froms[r] is not None and int(s) == froms[r] else 0) for s in ids],
                                np.uint8)
                gone = 0
                if drop:
                    keep = (dopt & 0x10) == 0
                    gone, ids, dopt = int(len(ids) - keep.sum()), ids[keep], dopt[keep]
                cut.append((FILTERS[f], _IdsOpts(ids, dopt, gone)))
            out.append(cut)
        return out

    def groups_opts(self, topics, flags, froms, drop=False):
        self.opts_calls += 1
        return self._cut(self._csr(topics)[0], flags, froms, drop)

    def groups_rows(self, topics):
        rows, csr = self._csr(topics)
        return [[(FILTERS[f], np.array(LOCAL.get(f, []), np.uint32)) for f in r] for r in rows], self.index, csr

    def groups(self, topics):
        return self.groups_rows(topics)[0]

    def window(self, topics, shared=None, strategy="round_robin", hashes=None, cluster=None, opts=None, drop=False):
        self.window_calls.append((list(topics), opts, drop))
        rows, csr = self._csr(topics)
        picks = shared.dispatch_batch(self.index, csr, strategy, hashes) if shared is not None else None
        plan = cluster.plan(self.index, csr) if cluster is not None else None
        out = self._cut(rows, opts[0], opts[1], drop) if opts is not None else self.groups_rows(topics)[0]
        return out, self.index, csr, picks, plan, {"device_waits": 1}


def _msg(k, qos=0, retain=False, frm=None, retained=False):
    return {"k": k, "qos": qos, "retain": retain, "from": frm, "retained": retained}


TRACE = [(b"loc/1", _msg("a", 1, True, "local0")), (b"rem/7", _msg("b", 2)), (b"sh/1/x", _msg("c")),
         (b"none/at/all", _msg("d")), (b"mix/9", _msg("e", 2, False, "local2")), (b"sh/2/x", _msg("f", 1)),
         (b"$SYS/broker", _msg("g")), (b"mix", _msg("h", 0, True, None, True)), (b"rem/8", _msg("i")),
         (b"sh/1/x", _msg("j", 2, True)), (b"loc", _msg("k", 1, False, "local1")), (b"zz", _msg("l")),
         (b"loc/2", _msg("m", 0, False, "someone-else"))]


def _world(subopts, drop=False, use_shared=True, use_cluster=True):
    routes, shared, cluster = _Routes(), _Shared() if use_shared else None, _Cluster() if use_cluster else None
    log = {"deliver": [], "batches": []}
    dests = {FILTERS[f]: [NODES[k] for k in ns] for f, ns in NODE_ROUTES.items()}
    for f, gs in GROUPS.items():
        dests.setdefault(FILTERS[f], []).extend((g, b"n1") for g, _ in gs)

    def deliver(sub, f, m, byte=None):
        log["deliver"].append((sub, f, m["k"], byte))
        return True
    pb = PublishBatcher(routes=routes, timer=False, node=b"n1", lookup_routes=lambda f: dests.get(f, []),
                        deliver=deliver, shared=shared, cluster=cluster, one_call=True, subopts=subopts,
                        drop_no_local=drop,
                        forward_batch=lambda node, pairs: log["batches"].append((node, [(f, m["k"]) for f, m in pairs]))
                        or ("ok", "fwd"))
    out = [pb.publish_batch(TRACE[:7]), pb.publish_batch(TRACE[7:])]
    return out, log, dict(pb.metrics), routes


@pytest.mark.parametrize("drop", [False, True], ids=["flag", "drop"])
@pytest.mark.parametrize("use_shared,use_cluster", [(True, True), (True, False), (False, True), (False, False)])
def test_one_call_batcher_carries_the_option_bytes(use_shared, use_cluster, drop):
    out, log, metrics, routes = _world(True, drop, use_shared, use_cluster)
    # exactly one window call per window, with the messages' pack_msg bytes and the publishers' routes.ids
    assert len(routes.window_calls) == 2 and routes.opts_calls == 0
    for (topics, opts, d), part in zip(routes.window_calls, (TRACE[:7], TRACE[7:])):
        assert topics == [t for t, _ in part] and d == drop
        assert list(opts[0]) == [pack_msg(m["qos"], m["retain"], m["retained"]) for _, m in part]
        assert list(opts[1]) == [routes.ids.get(m["from"]) if m["from"] is not None else None for _, m in part]
    # deliver gets the byte with every local delivery; the No-Local hit is flagged, or dropped and counted
    local = [x for x in log["deliver"] if x[0] in SUBS.values()]
    assert local and all(b is not None for *_, b in local)
    want, hits = [], 0
    for t, m in TRACE:
        for f in _match(t):
            for s in LOCAL.get(f, []):
                hit = SUBS[s] == m["from"]
                hits += hit
                if not (hit and drop):
                    want.append((SUBS[s], FILTERS[f], m["k"], pack_msg(m["qos"], m["retain"], m["retained"])
                                 | (0x10 if hit else 0)))
    assert local == want and hits == 3
    assert metrics["delivery.dropped.no_local"] == (hits if drop else 0)
    # picks and forwards: what the one-call batcher does without subopts
    plain, plog, pmetrics, proutes = _world(False, False, use_shared, use_cluster)
    assert [x[:3] for x in log["deliver"] if x[0] not in SUBS.values()] == \
        [x[:3] for x in plog["deliver"] if x[0] not in SUBS.values()]
    assert log["batches"] == plog["batches"] and bool(log["batches"]) == use_cluster
    if not drop:
        assert out == plain
    assert [x[:3] for x in plog["deliver"] if x[0] in SUBS.values()] == [x[:3] for x in want] or drop
    for name in ("messages.publish", "messages.dropped"):
        assert metrics[name] == pmetrics[name] or drop
    if use_shared or use_cluster:
        assert all(c[1] is None for c in proutes.window_calls)  # without subopts the window call carries no opts


def test_subopts_alone_and_without_one_call():
    routes = _Routes()
    got = []
    pb = PublishBatcher(routes=routes, timer=False, one_call=True, subopts=True,
                        deliver=lambda sub, f, m, b: got.append((sub, f, m["k"], b)) or True)
    pb.publish_batch(TRACE)
    assert len(routes.window_calls) == 1 and routes.opts_calls == 0 and got  # one_call + subopts alone: the window call
    routes2, got2 = _Routes(), []
    pb2 = PublishBatcher(routes=routes2, timer=False, subopts=True,
                         deliver=lambda sub, f, m, b: got2.append((sub, f, m["k"], b)) or True)
    pb2.publish_batch(TRACE)
    assert not routes2.window_calls and routes2.opts_calls == 1 and got2 == got  # ... what the two-call path gives
    for kw in (dict(shared=_Shared()), dict(cluster=_Cluster()), dict(shared=_Shared(), cluster=_Cluster())):
        with pytest.raises(TypeError, match="one_call"):
            PublishBatcher(routes=_Routes(), timer=False, subopts=True, **kw)
        PublishBatcher(routes=_Routes(), timer=False, subopts=True, one_call=True, **kw)
    with pytest.raises(TypeError):
        PublishBatcher(groups_fn=lambda ts: [], timer=False, subopts=True, one_call=True)
