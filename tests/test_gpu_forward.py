"""The forward plan on the device (emqx_gm_dests_*, emqx_gm_forward_plan,
emqx_amd/csrc/gm_dests.hip) against the host walk over a host-only twin of the
same table and the restatement of route(aggre(match_routes(Topic)))
(tests/_forward_ref.py).  Device and host walk are compared array for array
(both list every node's forwards in batch order); the restatement within one
row as a set.  The partition is run at forced chunk counts 1, 2, 3, 7 and the
library's own, over node counts around a wave (63, 64, 65) and at the cap."""

import ctypes as C
import random
from collections import Counter

import numpy as np
import pytest

from tests import _forward_ref as R

pytestmark = pytest.mark.gpu

CHUNKS = [1, 2, 3, 7, 0]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


class World:
    """One route set three ways: the device table, a host-only twin, the restatement."""

    def __init__(self, ctx, index, filters, routes, n_nodes):
        from emqx_amd import DestTable
        node_routes = [(f, d) for f, d in routes if isinstance(d, int)]
        self.ctx, self.index, self.n_nodes = ctx, index, n_nodes
        self.dev = ctx.build_dests(index, node_routes, n_nodes)
        self.twin = DestTable.compile_host(filters, node_routes, n_nodes)
        self.ref = R.Routes(filters, routes)
        a, b = self.dev.info(), self.twin.info()
        assert (a.n_routes, a.n_filters_with_routes, a.n_nodes) == (b.n_routes, b.n_filters_with_routes, b.n_nodes)
        assert a.device_bytes > 0 and b.device_bytes == 0

    def plan(self, rows, skip=None, n_chunks=None, check_ref=True):
        """Device == host walk (twin, and the device table's own host copy) == restatement."""
        csr = R.csr_of(rows)
        got = self.dev.plan(csr, skip, n_chunks)
        assert _same(got, self.twin.plan_host(csr, skip))
        assert _same(got, self.dev.plan_host(csr, skip))
        if check_ref:
            assert R.plan_lists(got) == R.plan(self.ref, rows, skip, self.n_nodes)[:2]
        return got

    def release(self):
        self.dev.release()
        self.twin.release()


def _device_rows(ctx, index, topics):
    from emqx_amd import pack
    tb, to = pack(topics)
    d_b, d_o = ctx.dev_alloc(tb.nbytes), ctx.dev_alloc(to.nbytes)
    ctx.memcpy_h2d(d_b, tb, tb.nbytes)
    ctx.memcpy_h2d(d_o, to, to.nbytes)
    res = ctx.match_device(index, d_b, d_o, len(topics))
    ctx.dev_free(d_b)
    ctx.dev_free(d_o)
    return res


class RawRows:
    """A device CSR made by the test (not a match result): rows the host never validated."""

    def __init__(self, ctx, row_off, ids, nnz=None):
        from emqx_amd import _lib
        from emqx_amd.engine import DeviceCsr
        ro = np.ascontiguousarray(row_off, np.uint64)
        ii = np.ascontiguousarray(ids, np.uint32)
        self.ctx = ctx
        self.d_ro, self.d_ids = ctx.dev_alloc(ro.nbytes), ctx.dev_alloc(max(ii.nbytes, 4))
        ctx.memcpy_h2d(self.d_ro, ro, ro.nbytes)
        if ii.nbytes:
            ctx.memcpy_h2d(self.d_ids, ii, ii.nbytes)
        m = _lib.Csr()
        m.n_rows, m.nnz, m.on_device = len(ro) - 1, len(ii) if nnz is None else nnz, 1
        m.row_off = C.cast(C.c_void_p(self.d_ro), C.POINTER(C.c_uint64))
        m.ids = C.cast(C.c_void_p(self.d_ids), C.POINTER(C.c_uint32))
        self.m, self.csr = m, DeviceCsr(ctx, m)

    def free(self):
        self.m.row_off = self.m.ids = None  # (the buffers are this test's, not a result's)
        self.ctx.dev_free(self.d_ro)
        self.ctx.dev_free(self.d_ids)


def _plan_device(table, res, skip=None, n_chunks=None):
    fw = table.plan_device(res, skip, n_chunks)
    out = fw.to_host()
    fw.free()
    return out


# ------------------------------------------------------------------ parity on matched rows
def test_parity_on_matched_rows_host_and_device(ctx):
    filters, routes, topics, _, _ = _world(5, 200, 1000)
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, routes, 5)
    ro, ids = ctx.match(index, topics)  # emqx_gm_match(WITH_EXACT)
    rows = [ids[int(ro[r]):int(ro[r + 1])].tolist() for r in range(len(topics))]
    assert [sorted(r) for r in rows] == [sorted(w.ref.match_ids(t)) for t in topics]
    res = _device_rows(ctx, index, topics)
    for skip in (None, 0):
        got = w.plan(rows, skip)
        assert len(got.rows) > 1000
        assert _same(_plan_device(w.dev, res, skip), got)  # device rows, the same result
        for c in CHUNKS:
            assert _same(w.dev.plan(R.csr_of(rows), skip, c), got), c
    assert all(t > 0 for t in w.dev.last_times()[:3])
    res.free()
    w.release()
    index.release()


def _world(n_nodes, n_filters, n_topics):
    return R.random_world(n_nodes, seed=23, n_filters=n_filters, n_topics=n_topics)


# ------------------------------------------------------------------ the partition's edges
@pytest.mark.parametrize("n_nodes", [1, 2, 63, 64, 65, 4096])
def test_node_counts_around_a_wave_and_at_the_cap(ctx, n_nodes):
    rnd = random.Random(n_nodes)
    filters = [b"n/%03d" % k for k in range(60)]
    routes = [(f, rnd.randrange(n_nodes)) for f in filters for _ in range(rnd.choice([0, 1, 2, 3]))]
    routes += [(filters[7], k) for k in range(min(n_nodes, 130))]  # one list longer than two waves
    routes += [(filters[9], n_nodes - 1), (filters[9], 0)]
    rows = [[rnd.randrange(60) for _ in range(rnd.choice([0, 1, 2, 5]))] for _ in range(400)]
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, routes, n_nodes)
    for skip in (None, n_nodes - 1):
        got = w.plan(rows, skip)
        for c in CHUNKS:
            assert _same(w.dev.plan(R.csr_of(rows), skip, c), got), c
    w.release()
    index.release()


def test_one_filter_on_every_node_matched_by_70_consecutive_rows(ctx):
    N = 4096
    filters = [b"all/#", b"few/+", b"none"]
    routes = [(b"all/#", k) for k in range(N)] + [(b"few/+", 5), (b"few/+", 4000)]
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, routes, N)
    topics = [b"few/a", b"none", b"zzz"] + [b"all/%d" % k for k in range(70)] + [b"few/b", b"zzz"]
    ro, ids = ctx.match(index, topics)
    rows = [ids[int(ro[r]):int(ro[r + 1])].tolist() for r in range(len(topics))]
    assert rows[2] == [] and rows[3:73] == [[0]] * 70
    got = w.plan(rows, None, check_ref=False)
    assert len(got.rows) == 286720 + 4
    for k in range(N):  # every node's list: exactly those 70 rows ascending (nodes 5 and 4000: few/+ around them)
        r, f = got.node(k)
        want = list(range(3, 73))
        if k in (5, 4000):
            want = [0] + want + [73]
        assert r.tolist() == want, k
        assert f.tolist() == [1 if x in (0, 73) else 0 for x in want]
    assert got.row_routes.tolist() == [2, 0, 0] + [N] * 70 + [2, 0]
    for c in (1, 7, 0):
        assert _same(w.dev.plan(R.csr_of(rows), None, c), got), c
    res = _device_rows(ctx, index, topics)
    assert _same(_plan_device(w.dev, res, None), got)
    skipped = w.plan(rows, 5, check_ref=False)
    assert len(skipped.node(5)[0]) == 0 and len(skipped.rows) == 286720 + 4 - 72
    assert np.array_equal(skipped.row_routes, got.row_routes)
    res.free()
    w.release()
    index.release()


def test_one_row_holding_256_plus_substitutions(ctx):
    words = [b"w%d" % k for k in range(8)]
    filters = sorted(b"/".join(b"+" if (mask >> k) & 1 else words[k] for k in range(8)) for mask in range(256))
    rnd = random.Random(4)
    routes = [(f, n) for f in filters for n in rnd.sample(range(5), rnd.choice([1, 2, 3]))]
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, routes, 5)
    topics = [b"zz", b"/".join(words), b"zz", b"zz", b"/".join(words), b"zz"]
    ro, ids = ctx.match(index, topics)
    rows = [ids[int(ro[r]):int(ro[r + 1])].tolist() for r in range(len(topics))]
    assert [len(r) for r in rows] == [0, 256, 0, 0, 256, 0]
    for skip in (None, 2):
        got = w.plan(rows, skip)
        assert len(got.rows) > 512  # the row spans several 256-hit steps of a block and, chunked, chunk boundaries
        for c in CHUNKS + [64, 1024]:
            assert _same(w.dev.plan(R.csr_of(rows), skip, c), got), c
    w.release()
    index.release()


# ------------------------------------------------------------------ empties
def test_empties(ctx):
    filters = [b"a/#", b"b/+", b"c"]
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, [(b"a/#", 2), (b"c", 2), (b"c", ("g", 1))], 3)
    zeros = [0, 0, 0, 0]
    for rows in ([], [[], [], []]):  # a 0-row window; all-empty rows
        got = w.plan(rows, None)
        assert got.node_off.tolist() == zeros and len(got.rows) == 0 and got.row_routes.tolist() == [0] * len(rows)
    got = w.plan([[0], [1], [2, 0]], 2)  # every hit on skip_node: nothing to forward, the rows still count
    assert got.node_off.tolist() == zeros and len(got.rows) == len(got.filters) == 0
    assert got.row_routes.tolist() == [1, 0, 2]
    raw = RawRows(ctx, [0, 1, 2, 4], [0, 1, 2, 0])
    dev = _plan_device(w.dev, raw.csr, 2)
    assert _same(dev, got)
    raw.free()
    raw = RawRows(ctx, [0], [])
    dev = _plan_device(w.dev, raw.csr, None)
    assert dev.node_off.tolist() == zeros and len(dev.rows) == 0 and len(dev.row_routes) == 0
    raw.free()
    w.release()
    none = World(ctx, index, filters, [], 2)  # a table with no routes
    got = none.plan([[0, 1], [2]], None)
    assert got.node_off.tolist() == [0, 0, 0] and got.row_routes.tolist() == [0, 0]
    raw = RawRows(ctx, [0, 2, 3], [0, 1, 2])
    assert _same(_plan_device(none.dev, raw.csr, None), got)
    raw.free()
    none.release()
    index.release()


# ------------------------------------------------------------------ device-row guards, refusals, overflow
def test_device_rows_with_ids_past_the_snapshot_and_an_offset_past_nnz(ctx):
    filters = [b"a/#", b"b/+", b"c"]
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, [(b"a/#", 1), (b"a/#", 3), (b"c", 0), (b"b/+", 2)], 4)
    # ids 3 (= n_filters) and 2^32 - 1 are skipped; the last offset (9) is clamped to nnz (5)
    raw = RawRows(ctx, [0, 3, 3, 9], [0, 3, 0xFFFFFFFF, 2, 0])
    for skip in (None, 1):
        want = w.plan([[0], [], [2, 0]], skip)
        assert len(want.rows) and _same(_plan_device(w.dev, raw.csr, skip), want)
        assert _same(_plan_device(w.dev, raw.csr, skip, 3), want)
    raw.free()
    w.release()
    index.release()


def test_refusals(ctx):
    from emqx_amd import Context, GpuMatchError, _lib
    filters = [b"a/#", b"b/+", b"c"]
    routes = [(b"a/#", 0), (b"c", 1)]
    index = ctx.build_index(filters)
    with pytest.raises(GpuMatchError) as e:
        ctx.build_dests(index, routes + [(b"not/there", 0)], 2)
    assert e.value.code == _lib.EINVAL and "not/there" in str(e.value)
    t = ctx.build_dests(index, routes + [(b"not/there", 0)], 2, skip_unknown=True)
    assert (t.info().n_routes, t.info().n_skipped_unknown) == (2, 1)
    for n_nodes, rs in ((0, []), (4097, []), (1, [(b"c", 1)])):
        with pytest.raises(GpuMatchError) as e:
            ctx.build_dests(index, rs, n_nodes)
        assert e.value.code == _lib.EINVAL
    shard = ctx.build_index_shard(filters, np.array([0, 1, 2], np.uint32))
    with pytest.raises(GpuMatchError) as e:
        ctx.build_dests(shard, routes, 2)
    assert e.value.code == _lib.EUNSUPPORTED
    shard.release()
    with Context(devices=[0, 0]) as c2:
        sharded = c2.build_index_sharded(filters)
        with pytest.raises(GpuMatchError) as e:
            c2.build_dests(sharded, routes, 2)
        assert e.value.code == _lib.EUNSUPPORTED
        sharded.release()
    for rows in (([0, 1], [3]), ([0, 2, 1, 2], [0, 0]), ([0, 1, 1], [0, 0])):
        with pytest.raises(GpuMatchError) as e:  # an id >= n_filters; descending offsets; offsets short of the ids
            t.plan(rows)
        assert e.value.code == _lib.EINVAL
    with pytest.raises(GpuMatchError) as e:
        t.plan(([0, 1], [0]), None, 1025)
    assert e.value.code == _lib.EINVAL
    t.release()
    index.release()


def test_overflow_is_detected_after_the_counting_pass(ctx):
    from emqx_amd import GpuMatchError, _lib
    N = 4096
    filters = [b"all/#", b"x"]
    index = ctx.build_index(filters)
    t = ctx.build_dests(index, [(b"all/#", k) for k in range(N)], N)
    n_ids = 1 << 20  # x 4096 nodes = 2^32 hits
    raw = RawRows(ctx, np.arange(0, n_ids + 1, 1024, dtype=np.uint64), np.zeros(n_ids, np.uint32))
    fw = _lib.Forwards()
    rc = _lib.lib().emqx_gm_forward_plan(ctx.h, t.h, C.byref(raw.m), _lib.DESTS_NO_SKIP, C.byref(fw))
    assert rc == _lib.EOVERFLOW
    assert not fw.node_off and not fw.rows and not fw.filters and not fw.row_routes and fw.n_pairs == 0
    with pytest.raises(GpuMatchError) as e:
        t.plan_device(raw.csr)
    assert e.value.code == _lib.EOVERFLOW
    raw.free()
    # the table still serves a window after the refusal
    small = RawRows(ctx, [0, 2, 3], [0, 1, 0])
    got = _plan_device(t, small.csr, 7)
    assert len(got.rows) == 2 * (N - 1) and got.row_routes.tolist() == [N, N]
    small.free()
    t.release()
    index.release()


# ------------------------------------------------------------------ batcher
class _Box:
    """A subscriber with an inbox; hashable by identity."""

    def __init__(self):
        self.box = []

    def append(self, x):
        self.box.append(x)


def _publish_world(ctx, use_cluster):
    from emqx_amd import ClusterRoutes
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    cluster = ClusterRoutes(ctx, node=b"n1") if use_cluster else None
    routes = GpuRoutes(ctx, node=b"n1", cluster=cluster) if use_cluster else GpuRoutes(ctx, node=b"n1")
    local = [_Box() for _ in range(3)]
    for k, box in enumerate(local):
        routes.subscribe(b"loc/%d/#" % k, box)
    dests = {b"job/+/run": [b"n2", (b"g0", b"n1"), b"n3"], b"job/#": [b"n3", (b"g0", b"n2"), (b"g0", b"n3")],
             b"loc/1/#": [b"n2", b"n1"], b"far/+": [b"n4"], b"gone/#": [b"n2"]}
    for f, ds in dests.items():
        for d in ds:
            routes.route_add(f, d)
    routes.route_delete(b"gone/#", b"n2")  # and gone again
    del dests[b"gone/#"]
    sent, shared = [], []
    items = [(b"job/%d/run" % (i % 5), "m%d" % i) for i in range(240)] + [(b"loc/1/x", "l1"), (b"none", "x"),
                                                                         (b"job/9", "j9"), (b"loc/1/y", "l2"),
                                                                         (b"far/1", "f1"), (b"gone/1", "g1")]
    kw = dict(routes=routes, timer=False, node=b"n1", lookup_routes=lambda f: dests.get(f, []),
              forward=lambda node, f, m: sent.append((node, f, m)) or ("ok", "fwd"),
              shared_dispatch=lambda g, f, m: shared.append((g, f, m)) or ("ok", 1))
    batches = []
    if use_cluster:
        pb = PublishBatcher(cluster=cluster, forward_batch=lambda node, pairs: batches.append((node, pairs)) or
                            ("ok", "fwd"), **kw)
    else:
        pb = PublishBatcher(**kw)
    out = pb.publish_batch(items)
    if use_cluster:
        assert not sent and cluster.builds == 1
        cluster.release()
    return out, [b.box for b in local], shared, sent, batches, pb.metrics


def test_batcher_with_cluster_equals_per_message_forwards(ctx):
    a = _publish_world(ctx, True)
    b = _publish_world(ctx, False)
    assert [sorted(r, key=repr) for r in a[0]] == [sorted(r, key=repr) for r in b[0]]
    assert a[1] == b[1] and Counter(map(repr, a[2])) == Counter(map(repr, b[2])) and a[5] == b[5]
    flat = [(node, f, m) for node, pairs in a[4] for f, m in pairs]
    assert Counter(flat) == Counter(b[3]) and len(flat) == 240 * 3 + 2 + 1 + 1
    assert sorted(node for node, _ in a[4]) == [b"n2", b"n3", b"n4"]  # one forward_batch per node with work
    for node, pairs in a[4]:  # per (node, filter): the publish order of the per-message path
        for f in {f for f, _ in pairs}:
            assert [m for ff, m in pairs if ff == f] == [m for n2, ff, m in b[3] if (n2, ff) == (node, f)]


def test_cluster_routes_rebuild_lazily_and_purge_a_node(ctx):
    from emqx_amd import ClusterRoutes
    filters = [b"a/#", b"b/+", b"c"]
    index = ctx.build_index(filters)
    c = ClusterRoutes(ctx, node=b"n1")
    for f, node in ((b"a/#", b"n2"), (b"a/#", b"n3"), (b"c", b"n1"), (b"c", b"n3"), (b"later/#", b"n2")):
        c.add_route(f, node)
    rows = R.csr_of([[0, 2], [1], [2]])
    p = c.plan(index, rows)  # 'later/#' is not in this snapshot: left out, not refused
    assert [list(zip(*p.node(k))) for k in range(3)] == [[], [(0, 0)], [(0, 0), (0, 2), (2, 2)]]
    assert p.row_routes.tolist() == [4, 0, 2] and c.table(index).info().n_skipped_unknown == 1
    c.plan(index, rows)
    assert c.builds == 1
    assert c.cleanup_routes(b"n3") == 2  # nodedown
    p = c.plan(index, rows)
    assert c.builds == 2 and [len(p.node(k)[0]) for k in range(3)] == [0, 1, 0] and p.row_routes.tolist() == [2, 0, 1]
    other = ctx.build_index(filters + [b"later/#"])  # another snapshot: ids shift, a new table
    p = c.plan(other, R.csr_of([[3], [0]]))
    assert c.builds == 3 and list(zip(*p.node(1))) == [(0, 3), (1, 0)]
    c.release()
    other.release()
    index.release()


# ------------------------------------------------------------------ multi-device context
def test_multi_device_context_serves_from_the_first_device():
    from emqx_amd import Context
    c = Context(devices=[0, 0])
    try:
        filters, routes, topics, _, _ = _world(5, 200, 1000)
        index = c.build_index(filters)
        w = World(c, index, filters, routes, 5)
        ro, ids = c.match(index, topics[:300])
        rows = [ids[int(ro[r]):int(ro[r + 1])].tolist() for r in range(300)]
        for skip in (None, 3):
            assert len(w.plan(rows, skip).rows) > 300
        w.release()
        index.release()
    finally:
        c.close()
