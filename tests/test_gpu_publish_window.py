"""A whole publish window in one call (emqx_gm_publish_window,
emqx_amd/csrc/gm_publish.hip) against the three calls it replaces: two
identical sets of tables, A and B; the window call runs on A,
emqx_gm_match_fanout + emqx_gm_shared_pick + emqx_gm_forward_plan on B, and
every output array must be equal, window by window.  Round robin and sticky
carry state from window to window, so the equality of a later window proves
the state after the earlier ones was equal too."""

import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IDS = 2000
MEMBER_COUNTS = (1, 2, 3, 64)
GROUP_COUNTS = (1, 2, 5)


def _filters():
    lits = [b"t/%d/x/%d" % (i, i % 7) for i in range(N_IDS)]
    wild = [b"t/%d/+/%d" % (i, i % 7) for i in range(0, N_IDS, 4)] + [b"t/%d/#" % i for i in range(0, N_IDS, 10)]
    return sorted(set(lits + wild + [b"t/+/x/3", b"w/#", b"lonely/1"]))


def _slots(filters):
    """Every 5th filter carries 1, 2 or 5 groups of 1, 2, 3 or 64 members."""
    out, k = [], 0
    for j, f in enumerate(filters):
        if j % 5:
            continue
        for g in range(GROUP_COUNTS[(j // 5) % 3]):
            m = MEMBER_COUNTS[k % 4]
            out.append((f, g, [1000 * (k % 50) + x for x in range(m)]))
            k += 1
    return out


def _routes(filters, n_nodes):
    """Every 3rd filter carries 1, 2 or 3 nodes, the local node 0 among them."""
    out = []
    for j, f in enumerate(filters):
        if j % 3:
            continue
        for x in range(1 + (j // 3) % 3):
            out.append((f, 0 if x == 0 and (j // 3) % 2 == 0 else (j * 7 + x * 13) % n_nodes))
    return out


def _topics(n, seed=0, hit=True):
    rng = np.random.default_rng(seed)
    if not hit:
        return [b"zz/%d" % i for i in range(n)]
    return [b"t/%d/x/%d" % (i, i % 7) for i in rng.integers(0, N_IDS, n).tolist()]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base(ctx):
    filters = _filters()
    index = ctx.build_index(filters, subs=[[j, j + 1, j + 2][:1 + j % 3] for j in range(len(filters))])
    yield filters, index
    index.release()


class Pair:
    """Tables A (the window call) and B (the three calls) over one snapshot."""

    def __init__(self, ctx, index, filters, n_nodes=65, shared=True, dests=True):
        self.ctx, self.index, self.filters = ctx, index, filters
        self.slots = _slots(filters)
        self.sh = [ctx.build_shared(index, self.slots) for _ in range(2)] if shared else [None, None]
        self.dt = [ctx.build_dests(index, _routes(filters, n_nodes), n_nodes) for _ in range(2)] if dests else [None, None]

    def rebuild(self):
        """Both shared tables rebuilt with their own predecessor as prev: the state carries over."""
        new = [self.ctx.build_shared(self.index, self.slots, prev=t) for t in self.sh]
        for t in self.sh:
            t.release()
        self.sh = new

    def ref(self, topics, strategy="round_robin", hashes=None, seed=0, skip=0):
        m, d = self.ctx.match_fanout(self.index, topics)
        picks = self.sh[1].pick(m, strategy, hashes, seed) if self.sh[1] is not None else None
        plan = self.dt[1].plan(m, skip) if self.dt[1] is not None else None
        return m, d, picks, plan

    def got(self, topics, strategy="round_robin", hashes=None, seed=0, skip=0):
        return self.ctx.publish_window(self.index, topics, shared=self.sh[0], strategy=strategy, hashes=hashes,
                                       seed=seed, dests=self.dt[0], skip_node=skip)

    def check(self, topics, **kw):
        want = self.ref(topics, **kw)
        got = self.got(topics, **kw)
        assert_same(got, want)
        return got

    def release(self):
        for t in self.sh + self.dt:
            if t is not None:
                t.release()


def assert_same(got, want):
    (m, d, picks, plan) = got[:4]
    (wm, wd, wpicks, wplan) = want
    for a, b, what in ((m, wm, "matches"), (d, wd, "deliveries"), (picks, wpicks, "picks"), (plan, wplan, "plan")):
        assert (a is None) == (b is None), what
        if a is None:
            continue
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)


@pytest.fixture
def pair(ctx, base):
    p = Pair(ctx, base[1], base[0])
    yield p
    p.release()


def _hashes(n, seed=5):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1024])
def test_window_sizes(pair, n):
    got = pair.check(_topics(n, seed=n), seed=n)
    if n:
        assert int(got[2][0][-1]) > 0 or n < 8  # the fixture gives the picks work
    pair.check(_topics(n, seed=n + 1), seed=n + 1)  # ... and the state after the first window was equal


def test_window_of_16384(pair):
    got = pair.check(_topics(16384, seed=3), seed=9)
    assert int(got[2][0][-1]) > 1000 and len(got[3].rows) > 1000
    pair.check(_topics(300, seed=4), seed=10)


def test_special_windows(ctx, base, pair):
    pair.check(_topics(200, hit=False))  # matches nothing
    got = pair.check([b"t/+/x/3", b"t/8/x/1", b"w/a/b", b"", b"lonely/1"] + _topics(60))  # a wildcard publish topic
    assert int(got[0][0][-1]) > 0
    pair.check(_topics(300, seed=7), skip=None)  # EMQX_GM_DESTS_NO_SKIP
    pair.check(_topics(300, seed=8), skip=9999)  # a skip_node past the table's nodes skips nothing either


@pytest.mark.parametrize("n_nodes", [1, 2, 65, 4096])
def test_node_counts(ctx, base, n_nodes):
    p = Pair(ctx, base[1], base[0], n_nodes=n_nodes)
    try:
        got = p.check(_topics(500, seed=n_nodes), skip=0)
        if n_nodes == 1:  # every route is skip_node's: no pair, but the rows still count their routes
            assert len(got[3].rows) == 0 and int(got[3].row_routes.sum()) > 0 and got[4]["n_pairs"] == 0
        else:
            assert len(got[3].rows) > 0
        p.check(_topics(500, seed=n_nodes), skip=None)
    finally:
        p.release()


@pytest.mark.parametrize("strategy", ["hash", "round_robin", "sticky", "random"])
def test_strategies_over_consecutive_windows(pair, strategy):
    for w in range(6):
        if w == 3:
            pair.rebuild()  # prev hands the state on, on both sides
        n = (257, 64, 1024, 300, 65, 500)[w]
        topics = _topics(n, seed=w % 2)  # the same slots again and again
        pair.check(topics, strategy=strategy, hashes=_hashes(n, w) if strategy == "hash" else None, seed=100 + w)


def test_one_round_trip_on_a_warm_context(pair):
    topics = _topics(1024, seed=11)
    for w in range(3):  # the context learns the window's hits and pairs per match
        pair.check(topics, seed=w)
    st = pair.check(topics, seed=3)[4]
    assert st["device_waits"] == 1, st
    assert (st["rows_spec"], st["fanout_spec"], st["picks_spec"], st["forwards_spec"]) == (1, 1, 1, 1), st
    assert st["n_hits"] > 0 and st["n_pairs"] > 0 and st["cap_hits"] >= st["n_hits"] and st["cap_pairs"] >= st["n_pairs"]


def test_fallbacks(pair, monkeypatch):
    topics = _topics(1024, seed=12)
    st = pair.check(topics, seed=1)[4]
    hits, pairs = st["n_hits"], st["n_pairs"]
    assert hits > 8 and pairs > 8
    monkeypatch.setenv("EMQX_GM_AB", "1")
    # the rows not speculative: both side results rerun on the true device rows
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    st = pair.check(topics, seed=2)[4]
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"]) == (0, 0, 0) and st["device_waits"] > 1, st
    monkeypatch.delenv("GM_NO_SPEC_IDS")
    # hits past the capacity: only the picks rerun
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits // 2))
    st = pair.check(topics, seed=3)[4]
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"]) == (1, 0, 1) and st["cap_hits"] == hits // 2, st
    pair.check(topics, seed=4)  # the next window after a failed speculation: the shadow state was discarded
    # hits exactly the capacity hold; one entry less does not
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits))
    st = pair.check(topics, seed=5)[4]
    assert st["picks_spec"] == 1 and st["n_hits"] == hits == st["cap_hits"], st
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits - 1))
    st = pair.check(topics, seed=6)[4]
    assert st["picks_spec"] == 0 and st["n_hits"] == hits == st["cap_hits"] + 1, st
    pair.check(topics, seed=7)
    monkeypatch.delenv("GM_PW_CAP_HITS")
    # pairs past the capacity: only the plan reruns
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(pairs // 2))
    st = pair.check(topics, seed=8)[4]
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"]) == (1, 1, 0), st
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(pairs))
    assert pair.check(topics, seed=9)[4]["forwards_spec"] == 1
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(pairs - 1))
    assert pair.check(topics, seed=10)[4]["forwards_spec"] == 0
    monkeypatch.setenv("GM_PW_CAP_PAIRS", "0")  # not speculated at all
    st = pair.check(topics, seed=11)[4]
    assert st["forwards_spec"] == 0 and st["cap_pairs"] == 0
    monkeypatch.delenv("GM_PW_CAP_PAIRS")
    for strategy in ("sticky", "round_robin"):  # the state is still the reference's
        pair.check(topics, strategy=strategy, seed=12)


def test_option_combinations(ctx, base):
    topics = _topics(300, seed=13)
    for shared, dests in ((True, False), (False, True), (False, False)):
        p = Pair(ctx, base[1], base[0], shared=shared, dests=dests)
        try:
            for w in range(2):
                got = p.check(topics, seed=w)
            assert (got[2] is None) == (not shared) and (got[3] is None) == (not dests)
        finally:
            p.release()


def test_errors_leave_outputs_and_state_alone(ctx, base, pair):
    from emqx_amd import _lib, pack
    from emqx_amd._lib import GpuMatchError
    topics = _topics(200, seed=14)
    pair.check(topics, seed=1)
    other = ctx.build_index(base[0], subs=[[j] for j in range(len(base[0]))])  # the same filters, another snapshot
    try:
        with pytest.raises(GpuMatchError) as e:
            ctx.publish_window(other, topics, shared=pair.sh[0], dests=None)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(GpuMatchError) as e:
            ctx.publish_window(other, topics, shared=None, dests=pair.dt[0])
        assert e.value.code == _lib.EINVAL
    finally:
        other.release()
    with pytest.raises(GpuMatchError) as e:
        pair.got(topics, strategy="hash", hashes=None)
    assert e.value.code == _lib.EINVAL
    # the C boundary: a refused call touches no output
    tb, to = pack(topics)
    o = _lib.PublishOpts()
    o.flags, o.shared, o.strategy = _lib.WITH_EXACT, pair.sh[0].h, 17  # a bad strategy
    res = _lib.PublishResult()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    before = bytes(res)
    rc = _lib.lib().emqx_gm_publish_window(ctx.h, pair.index.h, tb.ctypes.data, to.ctypes.data, len(topics),
                                           C.byref(o), C.byref(res), None)
    assert rc == _lib.EINVAL and bytes(res) == before
    pair.check(topics, seed=2)  # the state did not move
    pair.check(topics, strategy="sticky", seed=3)


def test_four_threads_through_one_context(pair):
    windows = [_topics(100 + 7 * k, seed=20 + k) for k in range(10)]
    hashes = [_hashes(len(w), k) for k, w in enumerate(windows)]
    want = [pair.ref(w, strategy="hash", hashes=h) for w, h in zip(windows, hashes)]
    bad = []

    def run(t):
        try:
            for k in range(50):
                j = (k + 3 * t) % len(windows)
                assert_same(pair.got(windows[j], strategy="hash", hashes=hashes[j]), want[j])
        except BaseException as e:  # noqa: BLE001
            bad.append(repr(e))

    ts = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:2]


def test_multi_device_context_equals_single_device(pair):
    from emqx_amd import Context
    windows = [_topics(n, seed=30 + n) for n in (65, 1024, 300)]
    want = [pair.ref(w, seed=k) for k, w in enumerate(windows)]
    with Context(devices=[0, 0]) as c2:
        index = c2.build_index(pair.filters, subs=[[j, j + 1, j + 2][:1 + j % 3] for j in range(len(pair.filters))])
        sh = c2.build_shared(index, pair.slots)
        dt = c2.build_dests(index, _routes(pair.filters, 65), 65)
        try:
            for k, w in enumerate(windows):
                assert_same(c2.publish_window(index, w, shared=sh, seed=k, dests=dt, skip_node=0), want[k])
        finally:
            sh.release()
            dt.release()
            index.release()


class _Box:
    def __init__(self):
        self.box = []

    def append(self, x):
        self.box.append(x)


def _batcher_world(ctx, one_call):
    from emqx_amd import ClusterRoutes
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    from emqx_amd.shared import SharedSub
    cluster = ClusterRoutes(ctx, node=b"n1")
    routes = GpuRoutes(ctx, node=b"n1", cluster=cluster)
    sh = SharedSub(ctx, seed=77)
    local = [_Box() for _ in range(3)]
    for k, box in enumerate(local):
        routes.subscribe(b"loc/%d/#" % k, box)
    members = [_Box() for _ in range(5)]
    dests = {b"job/+/run": [b"n2", (b"g0", b"n1"), b"n3"], b"job/#": [b"n3", (b"g1", b"n1")],
             b"loc/1/#": [b"n2", b"n1"], b"far/+": [b"n4"]}
    for f, ds in dests.items():
        for d in ds:
            routes.route_add(f, d)
    for k, m in enumerate(members):
        sh.subscribe(b"g0" if k < 3 else b"g1", b"job/+/run" if k < 3 else b"job/#", m)
    items = [(b"job/%d/run" % (i % 5), "m%d" % i) for i in range(200)] + [(b"loc/1/x", "l1"), (b"none", "x"),
                                                                         (b"job/9", "j9"), (b"far/1", "f1")]
    batches = []
    pb = PublishBatcher(routes=routes, timer=False, node=b"n1", lookup_routes=lambda f: dests.get(f, []),
                        shared=sh, shared_strategy="round_robin", cluster=cluster, one_call=one_call,
                        forward_batch=lambda node, pairs: batches.append((node, pairs)) or ("ok", "fwd"))
    out = [pb.publish_batch(items[:120]), pb.publish_batch(items[120:])]
    res = out, [b.box for b in local], [b.box for b in members], batches, dict(pb.metrics)
    sh.release()
    cluster.release()
    return res


def test_batcher_one_call_equals_the_three_calls(ctx):
    a = _batcher_world(ctx, True)
    b = _batcher_world(ctx, False)
    assert a == b
    assert sum(len(m) for m in a[2]) == 200 + 200 + 1 and len(a[3]) >= 3
