"""A publish window whose deliveries carry their option bytes, in the window's
one round trip (emqx_gm_publish_window_deliver, emqx_amd/csrc/gm_publish.hip and
gm_subopts.hip so_queue_spec) against the two calls it replaces: twin tables A
and B over one snapshot; the new call runs on A, ``Context.publish_window``
followed by ``SubOptTable.deliver`` on B, and every array must be equal, window
by window.  Round robin and sticky carry state from window to window, so the
equality of a later window proves the state after the earlier ones was equal.
The deliveries are also held against the host walk (emqx_gm_deliver_host) and,
for the small windows, the restatement of ignore_local/4 + enrich_subopts/3
(tests/_subopts_ref.py).

The filter set is small and crafted: ~40 ``s/<k>/#`` overlapped by ``s/+/x`` and
``#`` (rows of 1 to 3 filters), subscriber lists around k_so_copy's boundaries
(a thread moves 4, a workgroup owns 1,024 output elements at these sizes)."""

import ctypes as C
import threading

import numpy as np
import pytest

from tests import _subopts_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 1025, 3000)
N_K = 40
HIT_POS = (0, 3, 4, 5, 1023, 1024)  # first, around a 4-group, the 1,024-element workgroup boundary (and last, below)
N_NODES = 9
K_OF_LEN = {n: [k for k in range(N_K) if LENGTHS[k % len(LENGTHS)] == n] for n in LENGTHS}


def _world():
    filters = [b"s/%02d/#" % k for k in range(N_K)] + [b"s/+/x", b"#"]
    lists = [[10000 * (k + 1) + 3 * p for p in range(LENGTHS[k % len(LENGTHS)])] for k in range(N_K)]
    lists += [[900001, 900002, 900003], [800001, 800002, 800003, 800004, 800005]]
    opts, upgrade = {}, {}
    for i, lst in enumerate(lists):
        for p, s in enumerate(lst):  # every QoS x rap x upgrade_qos within 12 positions; nl at the hit positions
            nl = 1 if p in HIT_POS or p == len(lst) - 1 else 0
            opts[(i, s)] = R.subscribe_opts({"qos": p % 3, "nl": nl, "rap": (p // 3) % 2})
            upgrade[s] = bool((p // 6) % 2)
    return R.World(filters, lists, opts, upgrade)


def _slots(filters):
    """Every 3rd filter carries 1, 2 or 5 groups of 1, 2, 3 or 64 members."""
    out, k = [], 0
    for j, f in enumerate(filters):
        if j % 3:
            continue
        for g in range((1, 2, 5)[(j // 3) % 3]):
            out.append((f, g, [1000 * (k % 50) + x for x in range((1, 2, 3, 64)[k % 4])]))
            k += 1
    return out


def _routes(filters):
    """Every 2nd filter carries 1, 2 or 3 nodes, the local node 0 among them."""
    out = []
    for j, f in enumerate(filters):
        if j % 2:
            continue
        for x in range(1 + (j // 2) % 3):
            out.append((f, 0 if x == 0 and (j // 2) % 2 == 0 else (j * 7 + x * 13) % N_NODES))
    return out


def _window(w, n, seed=0, ks=None, publishers=True):
    """n topics: ``s/<k>/x`` (3 filters), ``s/<k>/y`` (2) or ``q/<i>`` (1), and their messages.  The publisher of a
    row is a subscriber of its ``s/<k>/#`` at one of the hit positions, another subscriber, or nobody."""
    rng = np.random.default_rng(seed)
    topics, msgs = [], []
    for i in range(n):
        k = int(ks[i % len(ks)]) if ks is not None else int(rng.integers(0, N_K))
        kind = int(rng.integers(0, 8))
        topics.append(b"q/%d" % i if kind == 0 else b"s/%02d/%s" % (k, b"x" if kind < 5 else b"y"))
        lst, frm, c = w.lists[k], None, int(rng.integers(0, 10))
        if publishers and c < 7 and lst and kind:
            pos = [p for p in HIT_POS + (len(lst) - 1,) if p < len(lst)]
            frm = lst[pos[(i + c) % len(pos)]]
        elif publishers and c == 7:
            frm = 800001 if i % 2 else 123  # a subscriber of '#' (its nl position 0), or of nothing
        msgs.append({"qos": i % 3, "retain": bool(i & 1), "retained": bool(i & 4) and not i & 2, "from": frm})
    return topics, msgs


def _flags_froms(msgs):
    return [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base(ctx):
    w = _world()
    index = ctx.build_index(w.filters, subs=w.lists)
    yield w, index
    index.release()


class Pair:
    """Tables A (the new call) and B (publish_window, then deliver) over one snapshot."""

    def __init__(self, ctx, w, index, shared=True, dests=True):
        self.ctx, self.w, self.index = ctx, w, index
        self.slots = _slots(sorted(w.filters))
        self.sh = [ctx.build_shared(index, self.slots) for _ in range(2)] if shared else [None, None]
        self.dt = [ctx.build_dests(index, _routes(sorted(w.filters)), N_NODES) for _ in range(2)] if dests else [None, None]
        self.so = [ctx.build_subopts(index, w.entries(), w.default_byte()) for _ in range(2)]

    def ref(self, topics, msgs, drop=False, strategy="round_robin", hashes=None, seed=0, skip=0):
        m, d, picks, plan, _ = self.ctx.publish_window(self.index, topics, shared=self.sh[1], strategy=strategy,
                                                       hashes=hashes, seed=seed, dests=self.dt[1], skip_node=skip)
        flags, froms = _flags_froms(msgs)
        return m, d, picks, plan, self.so[1].deliver(m, flags, froms, drop, index=self.index)

    def got(self, topics, msgs, drop=False, strategy="round_robin", hashes=None, seed=0, skip=0, ctx=None, tabs=None):
        flags, froms = _flags_froms(msgs)
        sh, dt, so = tabs or (self.sh[0], self.dt[0], self.so[0])
        return (ctx or self.ctx).publish_window(so.index, topics, shared=sh, strategy=strategy, hashes=hashes,
                                                seed=seed, dests=dt, skip_node=skip, subopts=so, msg_flags=flags,
                                                msg_from=froms, drop=drop)

    def check(self, topics, msgs, drop=False, walk=False, **kw):
        want = self.ref(topics, msgs, drop, **kw)
        got = self.got(topics, msgs, drop, **kw)
        assert_same(got, want, drop)
        flags, froms = _flags_froms(msgs)
        host = self.so[0].deliver_host(got[0], flags, froms, drop)
        assert_delivered(got[1], host, drop, "host walk")
        if walk:  # the restatement, row by row (small windows: it is a Python walk per delivery)
            ro, ids = got[0]
            rows = [ids[int(ro[r]):int(ro[r + 1])].tolist() for r in range(len(ro) - 1)]
            wro, wids, wopt, wdropped = self.w.walk(rows, msgs, drop)
            d = got[1]
            assert (d.row_off.tolist(), d.ids.tolist(), d.dopt.tolist()) == (wro, wids, wopt), "restatement"
            assert (d.row_dropped.tolist() if drop else [0] * len(rows)) == wdropped and d.n_dropped == sum(wdropped)
        return got

    def release(self):
        for t in self.sh + self.dt + self.so:
            if t is not None:
                t.release()


def assert_delivered(a, b, drop, what):
    for k, name in enumerate(("row_off", "ids", "dopt")):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, name)
    assert (a.row_dropped is None) == (not drop) and (b.row_dropped is None) == (not drop), what
    if drop:
        assert a.row_dropped.dtype == b.row_dropped.dtype and np.array_equal(a.row_dropped, b.row_dropped), what
    assert a.n_dropped == b.n_dropped, what


def assert_same(got, want, drop):
    (m, d, picks, plan) = got[:4]
    (wm, wfan, wpicks, wplan, wd) = want
    for a, b, what in ((m, wm, "matches"), (picks, wpicks, "picks"), (plan, wplan, "plan")):
        assert (a is None) == (b is None), what
        if a is None:
            continue
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
    assert_delivered(d, wd, drop, "deliveries")
    if not drop:  # FLAG mode: the ids are the plain fan-out's
        assert np.array_equal(d.row_off, wfan[0]) and np.array_equal(d.ids, wfan[1])
    st = got[4]
    assert st["fanout_spec"] == 0 and st["n_deliveries"] == len(d.ids) and st["n_dropped"] == d.n_dropped


@pytest.fixture
def pair(ctx, base):
    p = Pair(ctx, base[0], base[1])
    yield p
    p.release()


def _hashes(n, seed=5):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("drop", [False, True], ids=["flag", "drop"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1024])
def test_window_sizes(pair, n, drop):
    # (the large windows keep to the short lists: the long ones have windows of their own below)
    ks = None if n <= 65 else [k for k in range(N_K) if LENGTHS[k % len(LENGTHS)] <= 5] + K_OF_LEN[1024][:1]
    topics, msgs = _window(pair.w, n, seed=n, ks=ks)
    got = pair.check(topics, msgs, drop, walk=n <= 65, seed=n)
    if n >= 63:
        assert len(got[1].ids) > n and (got[1].n_dropped > 0) == drop
        assert drop or (got[1].dopt & 0x10).any()
    pair.check(*_window(pair.w, n, seed=n + 1, ks=ks), drop=drop, seed=n + 1)  # the state after the first window was equal


@pytest.mark.parametrize("shared,dests", [(True, True), (True, False), (False, True), (False, False)])
def test_option_combinations(ctx, base, shared, dests):
    p = Pair(ctx, base[0], base[1], shared=shared, dests=dests)
    try:
        for w in range(2):
            topics, msgs = _window(p.w, 65, seed=40 + w)
            got = p.check(topics, msgs, drop=bool(w), seed=w)
        assert (got[2] is None) == (not shared) and (got[3] is None) == (not dests)
    finally:
        p.release()


def test_windows_without_publishers_and_mixed(pair):
    topics, msgs = _window(pair.w, 65, seed=50, publishers=False)  # EMQX_GM_SO_NO_PUBLISHER in every row
    for drop in (False, True):
        got = pair.check(topics, msgs, drop, walk=True)
        assert got[1].n_dropped == 0 and not (got[1].dopt & 0x10).any()
    topics, msgs = _window(pair.w, 65, seed=51)
    for m in msgs[::2]:
        m["from"] = None
    for drop in (False, True):
        pair.check(topics, msgs, drop, walk=True)
    pair.check([b"zz/%d" % i for i in range(70)][:64] + [b""], _window(pair.w, 65, seed=52)[1])  # only '#' matches


def test_segment_starts_at_every_offset_mod_4(pair):
    ks = K_OF_LEN[1] + K_OF_LEN[3] + K_OF_LEN[5] + K_OF_LEN[4] + K_OF_LEN[0]
    topics, msgs = _window(pair.w, 64, seed=60, ks=ks)
    for drop in (False, True):
        got = pair.check(topics, msgs, drop, walk=True)
    (ro, ids), d = got[0], pair.check(topics, msgs, False)[1]
    starts, pos = set(), 0
    for f in ids.tolist():  # FLAG mode: a segment per matched filter, in order
        starts.add(pos % 4)
        pos += pair.index.subscriber_count(f)
    assert pos == len(d.ids) and starts == {0, 1, 2, 3}


def test_one_segment_spans_workgroups(pair):
    k = K_OF_LEN[3000][0]
    lst = pair.w.lists[k]
    topics = [b"s/%02d/y" % k] * 5
    msgs = [{"qos": i % 3, "retain": bool(i & 1), "retained": False,
             "from": (lst[0], lst[1023], lst[1024], lst[-1], None)[i]} for i in range(5)]
    for drop in (False, True):
        got = pair.check(topics, msgs, drop, walk=True)
        assert len(got[1].ids) == 5 * 3005 - (4 if drop else 0)
    ks = K_OF_LEN[1023] + K_OF_LEN[1024] + K_OF_LEN[1025] + K_OF_LEN[3000]
    for drop in (False, True):  # the hit on either side of the 1,024-element boundary, segments back to back
        pair.check(*_window(pair.w, 63, seed=61, ks=ks), drop=drop)


@pytest.mark.parametrize("strategy", ["hash", "round_robin", "sticky", "random"])
def test_strategies_over_three_consecutive_windows(pair, strategy):
    for w in range(3):
        n = (257, 64, 65)[w]
        topics, msgs = _window(pair.w, n, seed=w % 2, ks=list(range(0, N_K, 9)) + list(range(1, N_K, 9)))
        pair.check(topics, msgs, drop=bool(w & 1), strategy=strategy,
                   hashes=_hashes(n, w) if strategy == "hash" else None, seed=100 + w)


def _warm(pair, topics, msgs, drop=False, rounds=3):
    for w in range(rounds):  # the context learns the window's rows, hits, pairs and deliveries per match
        pair.check(topics, msgs, drop, seed=w)


@pytest.mark.parametrize("drop", [False, True], ids=["flag", "drop"])
def test_one_round_trip_on_a_warm_context(pair, drop):
    topics, msgs = _window(pair.w, 257, seed=70, ks=list(range(0, 5)) + K_OF_LEN[1024][:1])
    _warm(pair, topics, msgs, drop)
    st = pair.check(topics, msgs, drop, seed=3)[4]
    assert st["device_waits"] == 1, st
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"], st["deliveries_spec"]) == (1, 1, 1, 1), st
    assert st["n_hits"] > 0 and st["n_pairs"] > 0 and st["cap_deliveries"] >= st["n_deliveries"] > 257


def test_fallbacks(pair, monkeypatch):
    topics, msgs = _window(pair.w, 257, seed=71, ks=list(range(0, 5)) + K_OF_LEN[1024][:1])
    _warm(pair, topics, msgs)
    st = pair.check(topics, msgs, seed=1)[4]
    total, hits = st["n_deliveries"], st["n_hits"]
    std = pair.check(topics, msgs, True, seed=1)[4]
    kept, dropped = std["n_deliveries"], std["n_dropped"]
    assert total > 1024 and hits > 8 and dropped > 8 and kept + dropped == total
    monkeypatch.setenv("EMQX_GM_AB", "1")
    # the deliveries exactly at the capacity hold; one entry less does not: the exact rerun, the same result
    monkeypatch.setenv("GM_PW_CAP_DELIVERIES", str(total))
    st = pair.check(topics, msgs, seed=2)[4]
    assert (st["rows_spec"], st["deliveries_spec"], st["cap_deliveries"], st["device_waits"]) == (1, 1, total, 1), st
    monkeypatch.setenv("GM_PW_CAP_DELIVERIES", str(total - 1))
    st = pair.check(topics, msgs, seed=3)[4]
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"], st["deliveries_spec"]) == (1, 1, 1, 0), st
    assert st["cap_deliveries"] == total - 1 and st["device_waits"] > 1
    pair.check(topics, msgs, seed=4)
    # DROP mode: what counts is the total after the drop
    monkeypatch.setenv("GM_PW_CAP_DELIVERIES", str(kept))
    st = pair.check(topics, msgs, True, seed=5)[4]
    assert (st["deliveries_spec"], st["n_deliveries"], st["n_dropped"]) == (1, kept, dropped) and kept < total, st
    monkeypatch.setenv("GM_PW_CAP_DELIVERIES", str(kept - 1))
    assert pair.check(topics, msgs, True, seed=6)[4]["deliveries_spec"] == 0
    # not speculated at all
    monkeypatch.setenv("GM_PW_CAP_DELIVERIES", "0")
    st = pair.check(topics, msgs, seed=7)[4]
    assert (st["deliveries_spec"], st["cap_deliveries"], st["picks_spec"], st["forwards_spec"]) == (0, 0, 1, 1), st
    monkeypatch.delenv("GM_PW_CAP_DELIVERIES")
    # the rows not speculative: all three parts rerun on the true device rows
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    for drop in (False, True):
        st = pair.check(topics, msgs, drop, seed=8)[4]
        assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"], st["deliveries_spec"]) == (0, 0, 0, 0), st
        assert st["device_waits"] > 1
    monkeypatch.delenv("GM_NO_SPEC_IDS")
    # hits past their capacity while the deliveries hold: only the pick reruns
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits // 2))
    st = pair.check(topics, msgs, seed=9)[4]
    assert (st["rows_spec"], st["picks_spec"], st["forwards_spec"], st["deliveries_spec"]) == (1, 0, 1, 1), st
    monkeypatch.delenv("GM_PW_CAP_HITS")
    # a window the one-round-trip path does not serve: the calls in sequence
    monkeypatch.setenv("GM_FANOUT_SIMPLE", "1")
    for drop in (False, True):
        st = pair.check(topics, msgs, drop, seed=10)[4]
        assert st["device_waits"] == 0 and st["deliveries_spec"] == 0, st
    monkeypatch.delenv("GM_FANOUT_SIMPLE")
    for strategy in ("sticky", "round_robin"):  # the state is still the reference's
        pair.check(topics, msgs, strategy=strategy, seed=11)


def test_refusals_leave_outputs_and_state_alone(ctx, base, pair):
    from emqx_amd import SubOptTable, _lib, pack
    from emqx_amd._lib import GpuMatchError
    w = pair.w
    topics, msgs = _window(w, 64, seed=80)
    pair.check(topics, msgs, seed=1)
    n = len(topics)
    tb, to = pack(topics)
    flags = np.array(_flags_froms(msgs)[0], np.uint8)
    froms = np.array([0xFFFFFFFF if f is None else f for f in _flags_froms(msgs)[1]], np.uint32)
    other = ctx.build_index(w.filters, subs=w.lists)  # the same filters, another snapshot
    so_other = ctx.build_subopts(other, w.entries(), w.default_byte())
    host_only = SubOptTable.compile_host(w.filters, w.lists, w.entries(), w.default_byte())

    def call(shared=pair.sh[0].h, strategy=1, so=pair.so[0].h, mf=flags.ctypes.data, fr=froms.ctypes.data, mode=0,
             dopts=True, deliv=True, index=pair.index):
        o = _lib.PublishOpts()
        o.flags, o.shared, o.strategy, o.dests, o.skip_node = _lib.WITH_EXACT, shared, strategy, pair.dt[0].h, 0
        do = _lib.PublishDeliverOpts()
        do.subopts, do.msg_flags, do.msg_from, do.mode = so, mf, fr, mode
        res, dl, st = _lib.PublishResult(), _lib.Deliveries(), _lib.PublishDeliverStats()
        C.memset(C.byref(res), 0xAB, C.sizeof(res))
        C.memset(C.byref(dl), 0xAB, C.sizeof(dl))
        before = bytes(res), bytes(dl)
        rc = _lib.lib().emqx_gm_publish_window_deliver(ctx.h, index.h, tb.ctypes.data, to.ctypes.data, n, C.byref(o),
                                                       C.byref(do) if dopts else None, C.byref(res),
                                                       C.byref(dl) if deliv else None, C.byref(st))
        assert (bytes(res), bytes(dl)) == before  # byte-untouched
        return rc

    try:
        assert call(dopts=False) == _lib.EINVAL
        assert call(deliv=False) == _lib.EINVAL
        assert call(so=None) == _lib.EINVAL
        assert call(mf=None) == _lib.EINVAL
        assert call(fr=None) == _lib.EINVAL
        assert call(mode=2) == _lib.EINVAL
        for bad in (0x10, 0x80, 0x03):  # bits 4-7, QoS 3
            f2 = flags.copy()
            f2[n - 1] = bad
            assert call(mf=f2.ctypes.data) == _lib.EINVAL
        assert call(so=so_other.h) == _lib.EINVAL            # bound to another snapshot
        assert call(index=other) == _lib.EINVAL              # ... and the window's own refusals: the shared table's
        assert call(strategy=17) == _lib.EINVAL
        assert call(so=host_only.h) == _lib.EUNSUPPORTED
        with pytest.raises(GpuMatchError) as e:              # the binding checks the snapshot itself, as deliver does
            ctx.publish_window(pair.index, topics, subopts=so_other, msg_flags=flags, msg_from=froms)
        assert e.value.code == _lib.EINVAL
    finally:
        so_other.release()
        host_only.release()
        other.release()
    pair.check(topics, msgs, seed=2)  # the round-robin state did not move: the next window's picks say so
    pair.check(topics, msgs, strategy="sticky", seed=3)


def test_four_threads_through_one_context(pair):
    windows = [_window(pair.w, 40 + 7 * k, seed=20 + k, ks=list(range(0, 5)) + K_OF_LEN[1024][:1]) for k in range(6)]
    hashes = [_hashes(len(w[0]), k) for k, w in enumerate(windows)]
    want = [pair.ref(t, m, bool(k & 1), strategy="hash", hashes=h) for k, ((t, m), h) in enumerate(zip(windows, hashes))]
    bad = []

    def run(t):
        try:
            for k in range(24):
                j = (k + 3 * t) % len(windows)
                got = pair.got(*windows[j], drop=bool(j & 1), strategy="hash", hashes=hashes[j])
                assert_same(got, want[j], bool(j & 1))
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
    w = pair.w
    windows = [_window(w, n, seed=30 + n, ks=list(range(0, 5)) + K_OF_LEN[1024][:1]) for n in (65, 257, 64)]
    want = [pair.ref(t, m, bool(k & 1), seed=k) for k, (t, m) in enumerate(windows)]
    with Context(devices=[0, 0]) as c2:
        index = c2.build_index(w.filters, subs=w.lists)
        tabs = (c2.build_shared(index, pair.slots), c2.build_dests(index, _routes(sorted(w.filters)), N_NODES),
                c2.build_subopts(index, w.entries(), w.default_byte()))
        try:
            for k, (t, m) in enumerate(windows):
                assert_same(pair.got(t, m, bool(k & 1), seed=k, ctx=c2, tabs=tabs), want[k], bool(k & 1))
        finally:
            for t in tabs:
                t.release()
            index.release()


class _Box:
    def __init__(self):
        self.box = []

    def append(self, x):
        self.box.append(x)


def _batcher_world(ctx, one_call, drop):
    """The same world through PublishBatcher(one_call=True, subopts=True, shared=, cluster=) -- and, as the present
    code has no single path for all three, through its separate paths: a subopts batcher for the local deliveries
    and a shared + cluster batcher for the picks and forwards."""
    from emqx_amd import ClusterRoutes
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    from emqx_amd.shared import SharedSub
    cluster = ClusterRoutes(ctx, node=b"n1")
    routes = GpuRoutes(ctx, node=b"n1", cluster=cluster)
    sh = SharedSub(ctx, seed=77)
    local = [_Box() for _ in range(4)]
    for k, box in enumerate(local):
        routes.subscribe(b"loc/%d/#" % (k % 3), box, opts={"qos": k % 3, "nl": k & 1, "rap": k >> 1})
    members = [_Box() for _ in range(5)]
    dests = {b"job/+/run": [b"n2", (b"g0", b"n1"), b"n3"], b"job/#": [b"n3", (b"g1", b"n1")],
             b"loc/1/#": [b"n2", b"n1"], b"far/+": [b"n4"]}
    for f, ds in dests.items():
        for d in ds:
            routes.route_add(f, d)
    for k, m in enumerate(members):
        sh.subscribe(b"g0" if k < 3 else b"g1", b"job/+/run" if k < 3 else b"job/#", m)

    def msg(i, frm=None):
        return {"k": "m%d" % i, "qos": i % 3, "retain": bool(i & 1), "from": frm}
    items = [(b"job/%d/run" % (i % 5), msg(i)) for i in range(100)]
    items += [(b"loc/%d/x" % (i % 3), msg(100 + i, local[i % 4] if i % 2 else None)) for i in range(40)]
    items += [(b"none", msg(200)), (b"job/9", msg(201)), (b"far/1", msg(202))]
    batches, log = [], []

    def deliver(sub, f, m, byte=None):
        log.append(((local + members).index(sub), f, m["k"], byte))
        return True
    kw = dict(routes=routes, timer=False, node=b"n1", lookup_routes=lambda f: dests.get(f, []), deliver=deliver,
              forward_batch=lambda node, pairs: batches.append((node, [(f, m["k"]) for f, m in pairs])) or ("ok", "fwd"))
    halves = [items[:80], items[80:]]
    if one_call:
        pb = PublishBatcher(shared=sh, shared_strategy="round_robin", cluster=cluster, one_call=True, subopts=True,
                            drop_no_local=drop, **kw)
        out = [pb.publish_batch(h) for h in halves]
        no_local = pb.metrics["delivery.dropped.no_local"]
        local_log = sorted(x for x in log if x[3] is not None)
        picked = [x[:3] for x in log if x[3] is None]
    else:
        po = PublishBatcher(subopts=True, drop_no_local=drop, **kw)
        [po.publish_batch(h) for h in halves]
        no_local = po.metrics["delivery.dropped.no_local"]
        local_log = sorted(x for x in log if x[3] is not None)
        del log[:], batches[:]
        pb = PublishBatcher(shared=sh, shared_strategy="round_robin", cluster=cluster, one_call=True, **kw)
        out = [pb.publish_batch(h) for h in halves]
        picked = [x[:3] for x in log if x[0] >= len(local)]
    res = out, local_log, picked, batches, no_local
    sh.release()
    cluster.release()
    return res


@pytest.mark.parametrize("drop", [False, True], ids=["flag", "drop"])
def test_batcher_one_call_with_subopts_equals_the_separate_paths(ctx, drop):
    a = _batcher_world(ctx, True, drop)
    b = _batcher_world(ctx, False, drop)
    assert a[1] == b[1] and len(a[1]) > 40          # the local deliveries, each with its byte
    assert a[2] == b[2] and len(a[2]) == 100 + 100 + 1  # the shared picks' deliveries
    assert a[3] == b[3] and len(a[3]) >= 3          # the forwards
    assert a[4] == b[4] and (a[4] > 0) == drop      # delivery.dropped.no_local
    if not drop:
        assert a[0] == b[0]                         # the publish results (a dropped hit counts differently only in n)
