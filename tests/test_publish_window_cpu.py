"""The one-call publish window without a device: the library exports the new
entry points and lists their knobs, and PublishBatcher(one_call=True) over a
stand-in ``routes.window`` gives exactly what the default three-call batcher
gives over equivalent stand-ins (the device path: tests/test_gpu_publish_window.py)."""

import os
import re
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _lib
from emqx_amd.batcher import GpuRoutes, PublishBatcher
from emqx_amd.cluster import ForwardPlan
from emqx_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_knobs():
    L = _lib.lib()
    for name in ("emqx_gm_publish_window", "emqx_gm_publish_result_free"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    h = open(os.path.join(ROOT, "include", "emqx_gpu_match.h")).read()
    env = h[h.index(" * Environment:"):h.index("*/", h.index(" * Environment:"))]
    assert {"GM_PW_CAP_HITS", "GM_PW_CAP_PAIRS"} <= set(re.findall(r"\bGM_[A-Z0-9_]+", env))
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "gm_publish.hip")).read()
    assert set(re.findall(r'knob\("(GM_[A-Z0-9_]+)"', src)) == {"GM_PW_CAP_HITS", "GM_PW_CAP_PAIRS"}
    assert callable(Context.publish_window) and callable(GpuRoutes.window)
    # the ctypes mirror of the C structs: the sizes the header's layout gives on LP64
    assert (_lib.PublishOpts.shared.offset, _lib.PublishOpts.msg_hash.offset, _lib.PublishOpts.skip_node.offset) == \
        (8, 24, 40)
    assert _lib.PublishStats.n_hits.offset == 8 and _lib.PublishResult.forwards.offset == 4 * _lib.C.sizeof(_lib.Csr)


# ---- a small world: filter ids by position
FILTERS = [b"loc/#", b"rem/+", b"sh/+/x", b"mix/#", b"$SYS/#"]
LOCAL = {0: [0, 1], 3: [2]}                      # filter -> local subscriber ids
NODES = [b"n1", b"n2", b"n3"]                    # n1 is the local node
NODE_ROUTES = {1: [1, 2], 3: [0, 2], 4: [1]}     # filter -> node ids
GROUPS = {2: [(b"g0", [10, 11, 12]), (b"g1", [13])], 3: [(b"g0", [14, 15])]}  # filter -> [(group, members)]


def _match(topic):
    t = topic.split(b"/")
    out = []
    for f, name in enumerate(FILTERS):
        w = name.split(b"/")
        if w[-1] == b"#":
            ok = t[:len(w) - 1] == w[:-1]
        else:
            ok = len(t) == len(w) and all(a == b or b == b"+" for a, b in zip(t, w))
        if ok and not (topic.startswith(b"$") and w[0] in (b"+", b"#")):
            out.append(f)
    return out


class _Index:
    h = object()

    def filter(self, f):
        return FILTERS[f]


class _Shared:
    """Stand-in for SharedSub: round robin per (filter, group), state carried from call to call."""

    def __init__(self):
        self.next, self.calls = {}, 0

    def dispatch_batch(self, index, rows, strategy, hashes=None):
        self.calls += 1
        ro, ids = rows
        out = []
        for r in range(len(ro) - 1):
            row = []
            for f in ids[int(ro[r]):int(ro[r + 1])].tolist():
                for g, mem in GROUPS.get(f, []):
                    k = self.next.get((f, g), 0)
                    self.next[(f, g)] = k + 1
                    if hashes is not None:
                        k = hashes[r]
                    row.append((g, FILTERS[f], "sub%d" % mem[k % len(mem)]))
            out.append(row)
        return out

    def subscribers(self, group, f):
        return ["sub%d" % m for g, mem in GROUPS[FILTERS.index(f)] if g == group for m in mem]


class _Cluster:
    """Stand-in for ClusterRoutes: the plan in batch order, the local node skipped."""
    nodes, self_id = NODES, 0

    def __init__(self):
        self.calls = 0

    def plan(self, index, rows):
        self.calls += 1
        ro, ids = rows
        per = [[] for _ in NODES]
        rr = np.zeros(len(ro) - 1, np.uint32)
        for r in range(len(ro) - 1):
            for f in ids[int(ro[r]):int(ro[r + 1])].tolist():
                for node in NODE_ROUTES.get(f, []):
                    rr[r] += 1
                    if node != self.self_id:
                        per[node].append((r, f))
        flat = [p for node in per for p in node]
        off = np.cumsum([0] + [len(node) for node in per]).astype(np.uint64)
        return ForwardPlan(off, np.array([r for r, _ in flat], np.uint32), np.array([f for _, f in flat], np.uint32), rr)


class _Routes:
    """Stand-in for GpuRoutes: the three calls' ``groups_rows`` and the one call's ``window``."""

    def __init__(self, fail=False):
        self.index, self.subs, self.fail = _Index(), {}, fail
        self.other = {FILTERS[f]: 1 for f in set(NODE_ROUTES) | set(GROUPS)}
        self.window_calls = self.rows_calls = 0

    def _rows(self, topics):
        rows = [_match(t) for t in topics]
        ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        ids = np.array([f for r in rows for f in r], np.uint32)
        return [[(FILTERS[f], np.array(LOCAL.get(f, []), np.uint32)) for f in r] for r in rows], (ro, ids)

    def groups_rows(self, topics):
        self.rows_calls += 1
        out, csr = self._rows(topics)
        return out, self.index, csr

    def groups(self, topics):
        return self.groups_rows(topics)[0]

    def window(self, topics, shared=None, strategy="round_robin", hashes=None, cluster=None):
        self.window_calls += 1
        if self.fail:
            raise RuntimeError("device lost")
        out, csr = self._rows(topics)
        picks = shared.dispatch_batch(self.index, csr, strategy, hashes) if shared is not None else None
        plan = cluster.plan(self.index, csr) if cluster is not None else None
        return out, self.index, csr, picks, plan, {"device_waits": 1}


TRACE = [(b"loc/1", "a"), (b"rem/7", "b"), (b"sh/1/x", "c"), (b"none/at/all", "d"), (b"mix/9", "e"), (b"sh/2/x", "f"),
         (b"$SYS/broker", "g"), (b"mix", "h"), (b"rem/8", "i"), (b"sh/1/x", "j"), (b"loc", "k"), (b"zz", "l")]


def _world(one_call, use_shared=True, use_cluster=True, fail=False, strategy="round_robin"):
    routes, shared, cluster = _Routes(fail), _Shared() if use_shared else None, _Cluster() if use_cluster else None
    log = {"deliver": [], "batches": [], "forward": [], "shared": [], "dropped": [], "fallback": []}
    dests = {FILTERS[f]: [NODES[k] for k in ns] for f, ns in NODE_ROUTES.items()}
    for f, gs in GROUPS.items():
        dests.setdefault(FILTERS[f], []).extend((g, b"n1") for g, _ in gs)

    def deliver(sub, f, m):
        log["deliver"].append((sub, f, m))
        return sub != "sub13"  # one member is down: the FailedSubs walk

    def fallback(t):
        log["fallback"].append(t)
        return [(FILTERS[f], b"n2") for f in _match(t)]
    pb = PublishBatcher(routes=routes, timer=False, node=b"n1", lookup_routes=lambda f: dests.get(f, []),
                        subscribers={k: "local%d" % k for k in range(3)}, deliver=deliver,
                        forward=lambda node, f, m: log["forward"].append((node, f, m)) or ("ok", "fwd"),
                        forward_batch=lambda node, pairs: log["batches"].append((node, list(pairs))) or ("ok", "fwd"),
                        shared_dispatch=lambda g, f, m: log["shared"].append((g, f, m)) or ("ok", 1),
                        on_dropped=log["dropped"].append, fallback=fallback, shared=shared, shared_strategy=strategy,
                        cluster=cluster, one_call=one_call)
    out = [pb.publish_batch(TRACE[:7]), pb.publish_batch(TRACE[7:])]
    futs = [pb.submit(pb.prepare(t, m), m) for t, m in TRACE[:5]]  # the submit path carries the message into its window
    assert pb.flush() == 5
    out.append([pb.route_row(f.result(), t, m) for f, (t, m) in zip(futs, TRACE)])
    return out, log, dict(pb.metrics), (pb.batches, pb.messages), routes, shared, cluster


@pytest.mark.parametrize("use_shared,use_cluster,strategy", [(True, True, "round_robin"), (True, True, "hash_topic"),
                                                             (True, False, "round_robin"),
                                                             (False, True, "round_robin")])
def test_one_call_batcher_equals_the_three_calls(use_shared, use_cluster, strategy):
    a = _world(True, use_shared, use_cluster, strategy=strategy)
    b = _world(False, use_shared, use_cluster, strategy=strategy)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    # the trace covered every kind of message
    kinds = Counter(x[0] if isinstance(x[0], str) else "node" for batch in a[0][:2] for r in batch for x in r)
    assert kinds["node"] > 4 and kinds["share"] > 3
    assert (not a[1]["shared"]) == use_shared  # every group has a pick: no per-message shared_dispatch
    assert a[2]["messages.dropped"] >= 2 and a[1]["dropped"] and a[2]["messages.publish"] == len(TRACE) - 1 + 5
    if use_cluster:
        assert a[1]["batches"] and not a[1]["forward"]
        assert {node for node, _ in a[1]["batches"]} == {b"n2", b"n3"}
    if use_shared:
        assert ("sub13", b"sh/+/x", "c") in a[1]["deliver"]  # the down member was tried first, then the rest
    # one window call per batch on the one side, the three calls on the other
    assert a[4].window_calls == 3 and a[4].rows_calls == 0 and b[4].window_calls == 0 and b[4].rows_calls == 3
    for w in (a, b):
        assert w[5] is None or w[5].calls == 3
        assert w[6] is None or w[6].calls == 3


def test_a_failing_window_call_sends_every_caller_down_the_reference_path():
    out, log, metrics, _, routes, shared, cluster = _world(True, fail=True)
    assert routes.window_calls == 3 and shared.calls == 0 and cluster.calls == 0
    assert log["fallback"] == [t for t, _ in TRACE] + [t for t, _ in TRACE[:5]]
    assert not log["batches"] and not log["deliver"]
    assert out[0][0] == [(b"n2", b"loc/#", ("ok", "fwd"))]  # match_routes/1 -> forward, as without the device
    assert out[0][3] == [] and log["dropped"] == ["d", "l", "d"]


def test_one_call_needs_routes_and_is_off_by_default():
    with pytest.raises(TypeError):
        PublishBatcher(groups_fn=lambda ts: [], timer=False, one_call=True)
    r = _Routes()
    pb = PublishBatcher(routes=r, timer=False, shared=_Shared())
    pb.publish_batch(TRACE[:3])
    assert pb.one_call is False and r.window_calls == 0 and r.rows_calls == 1
    pb = PublishBatcher(routes=r, timer=False, one_call=True)  # neither table: the plain groups call, as before
    pb.publish_batch(TRACE[:3])
    assert r.window_calls == 0
