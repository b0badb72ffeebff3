"""The route-destination table on the host alone: the compiler
(emqx_amd/csrc/gm_dests.cpp) and the host walk (emqx_gm_forward_plan_host)
against the restatement of route(aggre(match_routes(Topic)))
(tests/_forward_ref.py), and PublishBatcher(cluster=...) over stand-in
collaborators.  No device is needed.  All comparisons are exact."""

import json
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import _forward_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(filters, routes, n_nodes, skip_unknown=False):
    from emqx_amd import DestTable
    return DestTable.compile_host(filters, routes, n_nodes, skip_unknown)


def _node_routes(routes):
    return [(f, d) for f, d in routes if isinstance(d, int)]


def _host_plan(t, rows, skip):
    return R.plan_lists(t.plan_host(R.csr_of(rows), skip))


def test_build_rules_dedupe_sort_info():
    filters = [b"b/+", b"a/#", b"c", b"a/#"]  # ids: a/# 0, b/+ 1, c 2
    routes = [(b"c", 3), (b"a/#", 2), (b"a/#", 0), (b"c", 3), (b"a/#", 2), (b"c", 1)]
    t = _table(filters, routes, 4)
    i = t.info()
    assert (i.n_routes, i.n_filters_with_routes, i.n_nodes, i.n_skipped_unknown, i.device_bytes) == (4, 2, 4, 0, 0)
    p = t.plan_host(R.csr_of([[2, 0], [], [1], [0]]), None)
    # a pair given twice is stored once; a filter's nodes ascending; each node's list in batch order
    assert p.node_off.tolist() == [0, 2, 3, 5, 6]
    assert list(zip(p.rows.tolist(), p.filters.tolist())) == [(0, 0), (3, 0), (0, 2), (0, 0), (3, 0), (0, 2)]
    assert p.row_routes.tolist() == [4, 0, 0, 2]
    q = t.plan_host(R.csr_of([[2, 0], [], [1], [0]]), 2)  # node 2 is local: skipped, still counted
    assert q.node_off.tolist() == [0, 2, 3, 3, 4] and q.row_routes.tolist() == [4, 0, 0, 2]
    from emqx_amd import GpuMatchError, _lib
    with pytest.raises(GpuMatchError) as e:
        t.plan(R.csr_of([[0]]))  # a host-only table has no device half
    assert e.value.code == _lib.EUNSUPPORTED
    t.release()
    empty = _table(filters, [], 1)
    assert empty.info().n_routes == 0
    p = empty.plan_host(R.csr_of([[0, 1], []]), None)
    assert p.node_off.tolist() == [0, 0] and len(p.rows) == 0 and p.row_routes.tolist() == [0, 0]
    empty.release()


def test_refusals():
    import ctypes as C
    from emqx_amd import GpuMatchError, _lib, pack
    filters = [b"a/#", b"b/+"]
    with pytest.raises(GpuMatchError) as e:
        _table(filters, [(b"a/#", 0), (b"nope/+", 1)], 2)
    assert e.value.code == _lib.EINVAL and "nope/+" in str(e.value)
    t = _table(filters, [(b"a/#", 0), (b"nope/+", 1), (b"b/+", 1), (b"nope/+", 0)], 2, skip_unknown=True)
    i = t.info()
    assert (i.n_routes, i.n_filters_with_routes, i.n_skipped_unknown) == (2, 2, 2)
    for bad_nodes, routes in ((2, [(b"a/#", 2)]), (0, []), (4097, []), (0, [(b"a/#", 0)])):
        with pytest.raises(GpuMatchError) as e:
            _table(filters, routes, bad_nodes)
        assert e.value.code == _lib.EINVAL, (bad_nodes, routes)
    _table(filters, [(b"a/#", 4095)], 4096).release()
    # non-monotone offsets and an unknown flag, through the C entry point
    ifb, ifo = pack(filters)
    fb = np.frombuffer(b"a/#b/+" + b"\0" * 58, np.uint8).copy()
    nodes = np.zeros(2, np.uint32)
    h = C.c_void_p()

    def call(fo, flags=0):
        fo = np.array(fo, np.uint64)
        return _lib.lib().emqx_gm_dests_compile_host(C.c_void_p(ifb.ctypes.data), C.c_void_p(ifo.ctypes.data), 2,
                                                     C.c_void_p(fb.ctypes.data), C.c_void_p(fo.ctypes.data),
                                                     C.c_void_p(nodes.ctypes.data), 2, 1, flags, C.byref(h))
    assert call([0, 3, 6]) == _lib.OK and h.value
    _lib.lib().emqx_gm_dests_release(h)
    assert call([0, 6, 3]) == _lib.EINVAL and not h.value
    assert call([0, 3, 6], flags=0x2) == _lib.EINVAL and not h.value
    # rows: an id past the snapshot, descending offsets
    for rows in (([0, 1, 2], [0, 2]), ([0, 2, 1], [0, 1])):
        with pytest.raises(GpuMatchError) as e:
            t.plan_host(rows, None)
        assert e.value.code == _lib.EINVAL
    t.release()


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "forward_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _golden(), ids=lambda c: c["name"][:40])
def test_golden_vectors(case):
    filters = [f.encode() for f in case["filters"]]
    routes = [(f.encode(), (d[0].encode(), d[1]) if isinstance(d, list) else d) for f, d in case["routes"]]
    ref = R.Routes(filters, routes)
    rows = [ref.match_ids(t.encode()) for t in case["topics"]]
    want = [[] for _ in range(case["n_nodes"])]
    for k, pairs in case["forwards"].items():
        want[int(k)] = [(r, ref.fid[f.encode()]) for r, f in pairs]
    groups = [[(f.encode(), g.encode()) for f, g in row] for row in case["groups"]]
    # the restatement reproduces the hand-written expectation ...
    assert R.plan(ref, rows, case["self"], case["n_nodes"]) == (want, case["row_routes"], groups)
    # ... and so does the host walk over the node routes
    t = _table(filters, _node_routes(routes), case["n_nodes"])
    assert _host_plan(t, rows, case["self"]) == (want, case["row_routes"])
    t.release()


@pytest.mark.parametrize("n_nodes", [1, 2, 9])
@pytest.mark.parametrize("skip", [None, 0])
def test_random_sets_host_walk_equals_the_restatement(n_nodes, skip):
    filters, routes, topics, rows, ref = R.random_world(n_nodes)
    want_nodes, want_counts, _ = R.plan(ref, rows, skip, n_nodes)
    t = _table(filters, _node_routes(routes), n_nodes)
    got_nodes, got_counts = _host_plan(t, rows, skip)
    t.release()
    assert got_nodes == want_nodes
    assert got_counts == want_counts
    # the window does have forwards (none, by construction, when the one node is the local one)
    total = sum(len(x) for x in want_nodes)
    assert total == 0 if (n_nodes, skip) == (1, 0) else total > 1000
    assert sum(want_counts) > 1000
    for r, row in enumerate(rows):  # 0 exactly where the restatement lists no node route
        node_list = [d for i in row for _, d in ref.lookup_routes(ref.names[i]) if isinstance(d, int)]
        assert (got_counts[r] == 0) == (not node_list)


def test_compiler_and_host_walk_under_asan():
    """tests/asan/asan_forward.cpp: gm_dests.cpp as host C++ under
    AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-forward"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_forward")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_forward ok" in p.stdout


def test_cluster_routes_host_mirror():
    """add_route / delete_route / cleanup_routes / lookup_routes and the node id map (no table is built)."""
    from emqx_amd import ClusterRoutes
    c = ClusterRoutes(None, node=b"n1")
    assert c.self_id == 0 and c.nodes == [b"n1"]
    c.add_route(b"a/#", b"n2")
    c.add_route("a/#", "n3")
    c.add_route(b"a/#", b"n2")  # do_add_route/2: a pair is stored once
    c.add_route(b"b/+", b"n3")
    c.add_route(b"c", b"n1")
    assert c.node_id == {b"n1": 0, b"n2": 1, b"n3": 2}
    assert c.lookup_routes(b"a/#") == [b"n2", b"n3"] and c.lookup_routes(b"zz") == []
    assert sorted(c.routes()) == [(b"a/#", 1), (b"a/#", 2), (b"b/+", 2), (b"c", 0)]
    c.delete_route(b"a/#", b"n2")
    c.delete_route(b"a/#", b"n9")  # not there: nothing happens, no id is made
    assert c.lookup_routes(b"a/#") == [b"n3"] and b"n9" not in c.node_id
    assert c.cleanup_routes(b"n3") == 2 and c.cleanup_routes(b"n3") == 0 and c.cleanup_routes(b"n9") == 0
    assert c.routes() == [(b"c", 0)]
    assert c.id_of(b"n3") == 2  # a node that went down keeps its id


class _Index:
    def __init__(self, names):
        self.names, self.h = names, object()

    def filter(self, f):
        return self.names[f]


class _Routes:
    """Stand-in for GpuRoutes: matched rows from the restatement, no local subscribers."""

    def __init__(self, ref, others):
        self.ref, self.other, self.subs = ref, others, {}
        self.index = _Index(ref.names)

    def groups_rows(self, topics):
        rows = [self.ref.match_ids(t) for t in topics]
        out = [[(self.ref.names[i], np.zeros(0, np.uint32)) for i in row] for row in rows]
        ro, ids = R.csr_of(rows)
        return out, self.index, (np.array(ro, np.uint64), np.array(ids, np.uint32))

    def groups(self, topics):
        return self.groups_rows(topics)[0]


class _Cluster:
    """Stand-in for ClusterRoutes over a host-only table: the plan by the host walk."""

    def __init__(self, filters, node_routes, nodes, self_id):
        self.nodes, self.self_id = nodes, self_id
        self.t = _table(filters, node_routes, len(nodes))
        self.calls = 0

    def plan(self, index, rows):
        self.calls += 1
        return self.t.plan_host(rows, self.self_id)


def test_batcher_cluster_argument_with_stand_in_collaborators():
    """PublishBatcher(cluster=...) against the same batcher without it: equal per-message results, equal
    multiset of forwards, per node the forwards in window order, one forward_batch per node with work.
    (Stand-ins for GpuRoutes and ClusterRoutes: the device path is tests/test_gpu_forward.py's.)"""
    from emqx_amd.batcher import PublishBatcher
    n_nodes = 4
    filters, routes, topics, rows, ref = R.random_world(n_nodes, n_filters=120, n_topics=300)
    names = [b"n%d" % k for k in range(n_nodes)]  # n0 is the local node
    dests = {}
    for f, d in routes:
        d = (d[0], names[d[1]]) if isinstance(d, tuple) else names[d]
        if d not in dests.setdefault(f, []):
            dests[f].append(d)
    others = {f: len(d) for f, d in dests.items()}
    items = [(t, ("msg", k)) for k, t in enumerate(topics)]

    def make(**kw):
        sent, shared = [], []
        b = PublishBatcher(routes=_Routes(ref, others), timer=False, node=b"n0",
                           lookup_routes=lambda f: dests.get(f, []),
                           forward=lambda node, f, m: sent.append((node, f, m)) or ("ok", "fwd"),
                           shared_dispatch=lambda g, f, m: shared.append((g, f, m)) or ("ok", 1), **kw)
        return b, sent, shared

    plain, sent0, shared0 = make()
    want = plain.publish_batch(items)
    batches = []
    cluster = _Cluster(filters, _node_routes(routes), names, 0)
    b, sent1, shared1 = make(cluster=cluster, forward_batch=lambda node, pairs: batches.append((node, pairs)) or
                             ("ok", "fwd"))
    got = b.publish_batch(items)
    key = repr
    assert [sorted(r, key=key) for r in got] == [sorted(r, key=key) for r in want]
    assert not sent1 and cluster.calls == 1  # no per-route forward, one plan for the window
    flat = [(node, f, m) for node, pairs in batches for f, m in pairs]
    assert Counter(flat) == Counter(sent0) and len(flat) > 100
    assert Counter(map(key, shared1)) == Counter(map(key, shared0)) and shared0
    assert len({node for node, _ in batches}) == len(batches)  # one forward_batch per node ...
    assert {node for node, _ in batches} == {node for node, _, _ in sent0}  # ... exactly the nodes with work
    assert b"n0" not in {node for node, _ in batches}
    for node, pairs in batches:  # window order per node
        order = [m[1] for _, m in pairs]
        assert order == sorted(order)
        # and, per (filter, node), the publish order of the per-message path
        per_f0, per_f1 = {}, {}
        for n2, f, m in sent0:
            if n2 == node:
                per_f0.setdefault(f, []).append(m)
        for f, m in pairs:
            per_f1.setdefault(f, []).append(m)
        assert per_f0 == per_f1
    assert b.metrics == plain.metrics
    # the submit path carries the message into its window
    batches.clear()
    futs = [b.submit(t, m) for t, m in items[:50]]
    assert b.flush() == 50 and cluster.calls == 2
    assert [sorted(b.route_row(f.result(), t, m), key=key) for f, (t, m) in zip(futs, items)] == \
        [sorted(r, key=key) for r in want[:50]]
    assert len({node for node, _ in batches}) == len(batches)
    # a failing RPC is the result of each of its pairs
    bad, _, _ = make(cluster=cluster, forward_batch=lambda node, pairs: 1 / 0)
    res = bad.publish_batch(items[:50])
    assert {x[2] for r in res for x in r if x[0] not in (b"n0", "share")} == {("error", "badrpc")}
    with pytest.raises(TypeError):
        PublishBatcher(groups_fn=lambda ts: [], timer=False, cluster=cluster)
    cluster.t.release()
