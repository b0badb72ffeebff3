"""Whole publish windows coalesced into one device round trip
(emqx_gm_publish_windows / emqx_gm_combiner_publish, emqx_amd/csrc/gm_publish.hip
and gm_windows.hip) against emqx_gm_publish_window run window after window:
two identical sets of tables, A and B; the grouped call runs on A, the
sequential calls on B, and every output array must be equal, window by window.
Then one more sequential window runs on both sides: round robin and sticky
carry state, so its equality proves the state after the group was equal too.
(The helpers restate tests/test_gpu_publish_window.py's shapes.)"""

import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IDS = 2000
MEMBER_COUNTS = (1, 2, 3, 64)
GROUP_COUNTS = (1, 2, 5)
STRATEGIES = ("hash", "round_robin", "sticky", "random")


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


def _routes(filters, n_nodes, one_node=None):
    """Every 3rd filter carries 1, 2 or 3 nodes, the local node 0 among them
    (one_node: every route on that node instead)."""
    out = []
    for j, f in enumerate(filters):
        if j % 3:
            continue
        if one_node is not None:
            out.append((f, one_node))
            continue
        for x in range(1 + (j // 3) % 3):
            out.append((f, 0 if x == 0 and (j // 3) % 2 == 0 else (j * 7 + x * 13) % n_nodes))
    return out


def _topics(n, seed=0, hit=True):
    rng = np.random.default_rng(seed)
    if not hit:
        return [b"zz/%d" % i for i in range(n)]
    return [b"t/%d/x/%d" % (i, i % 7) for i in rng.integers(0, N_IDS, n).tolist()]


def _hashes(n, seed=5):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def _windows(sizes, seed=0):
    return [_topics(n, seed=seed * 131 + k) for k, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _subs(filters):
    return [[j, j + 1, j + 2][:1 + j % 3] for j in range(len(filters))]


@pytest.fixture(scope="module")
def base(ctx):
    filters = _filters()
    index = ctx.build_index(filters, subs=_subs(filters))
    yield filters, index
    index.release()


def assert_same(got, want):
    (m, d, picks, plan) = got[:4]
    (wm, wd, wpicks, wplan) = want[:4]
    for a, b, what in ((m, wm, "matches"), (d, wd, "deliveries"), (picks, wpicks, "picks"), (plan, wplan, "plan")):
        assert (a is None) == (b is None), what
        if a is None:
            continue
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)


class Pair:
    """Tables A (the grouped call) and B (publish_window, window after window) over one snapshot."""

    def __init__(self, ctx, index, filters, n_nodes=65, shared=True, dests=True, one_node=None):
        self.ctx, self.index, self.filters = ctx, index, filters
        self.slots = _slots(filters)
        self.sh = [ctx.build_shared(index, self.slots) for _ in range(2)] if shared else [None, None]
        self.dt = ([ctx.build_dests(index, _routes(filters, n_nodes, one_node), n_nodes) for _ in range(2)]
                   if dests else [None, None])

    def solo(self, side, topics, strategy="round_robin", hashes=None, seed=0, skip=0, via=None):
        return (via or self.ctx).publish_window(self.index, topics, shared=self.sh[side], strategy=strategy,
                                                hashes=hashes, seed=seed, dests=self.dt[side], skip_node=skip)

    def group(self, windows, strategy="round_robin", hashes=None, seed=0, skip=0):
        return self.ctx.publish_windows(self.index, windows, hashes=hashes, shared=self.sh[0], strategy=strategy,
                                        seed=seed, dests=self.dt[0], skip_node=skip, group_stats=True)

    def check(self, windows, strategy="round_robin", seed=0, skip=0, hseed=0):
        """The grouped call on A against the sequence on B, then one more window on both."""
        hashes = None
        if strategy == "hash" and self.sh[0] is not None:
            hashes = [_hashes(len(w), hseed + 17 * k) for k, w in enumerate(windows)]  # a different array per window
        got = self.group(windows, strategy, hashes, seed, skip)
        assert len(got) == len(windows)
        for k, w in enumerate(windows):
            want = self.solo(1, w, strategy, None if hashes is None else hashes[k], seed, skip)
            try:
                assert_same(got[k], want)
            except AssertionError as e:
                raise AssertionError(f"window {k} of {len(windows)}: {e} ({got[k][4]})") from None
        after = _topics(90, seed=seed + 4242)
        ha = _hashes(90, 3) if hashes is not None else None
        assert_same(self.solo(0, after, strategy, ha, seed + 1, skip), self.solo(1, after, strategy, ha, seed + 1, skip))
        return got

    def release(self):
        for t in self.sh + self.dt:
            if t is not None:
                t.release()


@pytest.fixture(scope="module")
def pairs(ctx, base):
    """(shared + dests, shared only, dests only): module-wide, A and B move in step."""
    ps = [Pair(ctx, base[1], base[0]), Pair(ctx, base[1], base[0], dests=False), Pair(ctx, base[1], base[0], shared=False)]
    yield ps
    for p in ps:
        p.release()


@pytest.fixture
def pair(pairs):
    return pairs[0]


def _lit(filters, step):
    """A literal filter (usable as a topic) at a position that is a multiple of `step`."""
    for j in range(0, len(filters), step):
        if b"+" not in filters[j] and b"#" not in filters[j] and filters[j].startswith(b"t/"):
            return filters[j]
    raise AssertionError("no such filter")


def _size_lists(filters):
    t = _lit(filters, 15)  # a filter with slots (every 5th) and routes (every 3rd)
    return {
        "empty": [[]],
        "one": _windows([1]),
        "64_0_65": _windows([64, 0, 65], 1),
        "63_1_1_257": _windows([63, 1, 1, 257], 2),
        "4x1024": _windows([1024] * 4, 3),
        "64x16": _windows([16] * 64, 4),
        "65x16": _windows([16] * 65, 5),  # two groups
        "no_hit_middle": [_topics(64, 6), _topics(40, hit=False), _topics(65, 7)],
        # a window's last row and the next window's first row hit the same filter, node and slot
        "boundary": [_topics(30, 8) + [t, t], [t] + _topics(30, 9), [t], [t, t]],
    }


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", ["empty", "one", "64_0_65", "63_1_1_257", "4x1024", "64x16", "65x16", "no_hit_middle",
                                  "boundary"])
def test_window_size_lists(pairs, base, name, strategy):
    windows = _size_lists(base[0])[name]
    for p in pairs if strategy == "round_robin" else pairs[:2]:  # (without a shared table the strategy is not read)
        got = p.check(windows, strategy=strategy, seed=len(name))
        seqs = [g[4]["group"]["seq"] for g in got]
        assert seqs == sorted(seqs) and seqs[0] == 0
        assert (seqs[-1] == 1) == (name == "65x16"), seqs
        if name == "boundary":
            if p.sh[0] is not None:
                assert all(int(g[2][0][-1]) > 0 for g in got)
            if p.dt[0] is not None:
                assert all(len(g[3].rows) > 0 for g in got)


def test_random_mixes_the_row_in_its_own_window(pair):
    """Two windows of identical topics in one group get identical picks, each equal to the call alone."""
    w = _topics(300, seed=21)
    got = pair.group([w, w], strategy="random", seed=9)
    alone = pair.solo(1, w, strategy="random", seed=9)
    assert int(alone[2][0][-1]) > 100
    for k in range(2):
        assert_same(got[k], alone)
        assert got[k][4]["group"]["n_windows"] == 2


def test_round_robin_runs_on_across_the_windows_of_a_group(base, pair):
    """A 64-member slot hit in three consecutive windows of one group, then once more after it."""
    f = next(f for f, g, mem in _slots(base[0]) if len(mem) == 64 and b"+" not in f and b"#" not in f)
    windows = [[f] * 3, [f] * 2, [f] * 5]
    got = pair.group(windows, seed=5) + [pair.solo(0, [f] * 2, seed=5)]
    want = [pair.solo(1, w, seed=5) for w in windows + [[f] * 2]]
    per_slot = {}
    for g, w in zip(got, want):
        assert_same(g, w)
        ro, mem, sl = g[2]
        for m, s in zip(mem.tolist(), sl.tolist()):
            per_slot.setdefault(s, []).append(m)
    assert all(len(v) == 12 for v in per_slot.values())
    wide = [v for v in per_slot.values() if len(set(v)) == 12]  # twelve members in a row: no restart, no repeat
    assert wide
    for v in wide:
        idx = [m % 1000 for m in v]
        assert all((y - x) % 64 == 1 for x, y in zip(idx, idx[1:])), idx


@pytest.mark.parametrize("n_nodes", [1, 2, 65, 4096])
def test_node_counts(ctx, base, n_nodes):
    p = Pair(ctx, base[1], base[0], n_nodes=n_nodes, shared=False)
    try:
        windows = _windows([63, 257, 0, 16, 300], n_nodes)
        got = p.check(windows, skip=0)
        if n_nodes == 1:  # every route is skip_node's: no pair, but the rows still count their routes
            assert all(len(g[3].rows) == 0 for g in got) and int(got[1][3].row_routes.sum()) > 0
        else:
            assert len(got[1][3].rows) > 0
            assert any(int(a) == int(b) for a, b in zip(got[1][3].node_off, got[1][3].node_off[1:]))  # an empty list
        p.check(windows, skip=None)  # EMQX_GM_DESTS_NO_SKIP
    finally:
        p.release()


def test_all_pairs_on_one_node(ctx, base):
    p = Pair(ctx, base[1], base[0], n_nodes=65, shared=False, one_node=7)
    try:
        got = p.check(_windows([64, 65, 300], 3), skip=0)
        no = got[2][3].node_off
        assert int(no[7]) == 0 and int(no[8]) == len(got[2][3].rows) > 0
    finally:
        p.release()


def _warm(pair, windows, **kw):
    for w in range(3):  # the context learns the windows' hits and pairs per match
        got = pair.check(windows, seed=w, **kw)
    return got


def _flags(g):
    q = g[4]["group"]
    return q["rows_spec"], q["picks_spec"], q["forwards_spec"]


def test_one_wait_for_a_held_group(pair):
    windows = _windows([128] * 8, 11)
    _warm(pair, windows)
    got = pair.check(windows, seed=3)
    for k, g in enumerate(got):
        q = g[4]["group"]
        assert q["device_waits"] == 1 and q["n_windows"] == 8 and q["position"] == k and q["grouped"] == 1, q
        assert _flags(g) == (1, 1, 1) and (q["window_picks_exact"], q["window_forwards_exact"]) == (0, 0), q
        assert g[4]["fanout_spec"] == 1 and g[4]["picks_spec"] == 1 and g[4]["forwards_spec"] == 1, g[4]
    assert sum(g[4]["n_hits"] for g in got) == got[0][4]["group"]["n_hits"] > 0
    assert sum(g[4]["n_pairs"] for g in got) == got[0][4]["group"]["n_pairs"] > 0


def test_group_fallbacks(pair, monkeypatch):
    windows = _windows([200, 64, 0, 300], 12)
    q = _warm(pair, windows)[0][4]["group"]
    hits, npairs = q["n_hits"], q["n_pairs"]
    assert hits > 8 and npairs > 8
    monkeypatch.setenv("EMQX_GM_AB", "1")
    # the rows not speculative: both side results rerun on the true device rows
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    for strategy in STRATEGIES:
        got = pair.check(windows, strategy=strategy, seed=2)
        assert _flags(got[0]) == (0, 0, 0) and got[0][4]["group"]["device_waits"] > 1, got[0][4]
    monkeypatch.delenv("GM_NO_SPEC_IDS")
    # the group's total exactly its capacity: held in one round trip
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits))
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(npairs))
    got = pair.check(windows, seed=3)
    q = got[0][4]["group"]
    assert _flags(got[0]) == (1, 1, 1) and q["device_waits"] == 1, q
    assert (q["cap_hits"], q["cap_pairs"]) == (hits, npairs) == (q["n_hits"], q["n_pairs"]), q
    # one hit past it: only the picks rerun
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits - 1))
    for strategy in STRATEGIES:
        got = pair.check(windows, strategy=strategy, seed=4)
        assert _flags(got[0]) == (1, 0, 1) and got[0][4]["group"]["n_hits"] == hits, got[0][4]
    pair.check(windows, seed=5)  # the next group after a failed speculation: the shadow state was discarded
    # one pair past it: only the plan reruns
    monkeypatch.setenv("GM_PW_CAP_HITS", str(hits))
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(npairs - 1))
    got = pair.check(windows, seed=6)
    assert _flags(got[0]) == (1, 1, 0) and got[0][4]["group"]["n_pairs"] == npairs, got[0][4]
    monkeypatch.setenv("GM_PW_CAP_PAIRS", "0")  # not speculated at all
    monkeypatch.setenv("GM_PW_CAP_HITS", "0")
    got = pair.check(windows, strategy="sticky", seed=7)
    assert _flags(got[0]) == (1, 0, 0) and got[0][4]["group"]["cap_pairs"] == 0
    monkeypatch.delenv("GM_PW_CAP_PAIRS")
    monkeypatch.delenv("GM_PW_CAP_HITS")
    for strategy in ("sticky", "round_robin"):  # the state is still the sequence's
        pair.check(windows, strategy=strategy, seed=8)


def test_one_window_past_its_own_capacity(ctx, base, pair, monkeypatch):
    """The context has learnt few hits and pairs per match; then one window of a
    group holds nearly all of them: its own capacity is exceeded while the
    group's (forced wide) holds.  Only that window gets a result of exact size."""
    cand = _topics(20000, seed=77)
    ro, ids = ctx.match(base[1], cand)
    cold, hot = [], []
    for k, t in enumerate(cand):
        row = ids[int(ro[k]):int(ro[k + 1])]
        if not ((row % 5 == 0) | (row % 3 == 0)).any():
            cold.append(t)  # no matched filter carries a slot or a route
        elif (row % 15 == 0).any():
            hot.append(t)  # a matched filter carries both
    assert len(cold) > 600 and len(hot) > 1000
    hot = (hot * 10)[:8000]
    warm = [cold[:300], cold[300:600]]
    for w in range(2):  # (the sequence on B last: hits and pairs per match end at their floor)
        got = pair.group(warm, seed=w, skip=None)
        for k in range(2):
            assert_same(got[k], pair.solo(1, warm[k], seed=w, skip=None))
    monkeypatch.setenv("EMQX_GM_AB", "1")
    monkeypatch.setenv("GM_PW_CAP_HITS", str(1 << 20))
    monkeypatch.setenv("GM_PW_CAP_PAIRS", str(1 << 20))
    windows = [cold[:50], hot, cold[50:90]]
    got = pair.group(windows, seed=3, skip=None)
    monkeypatch.delenv("GM_PW_CAP_HITS")
    monkeypatch.delenv("GM_PW_CAP_PAIRS")
    for k, g in enumerate(got):
        assert_same(g, pair.solo(1, windows[k], seed=3, skip=None))
        q = g[4]["group"]
        assert _flags(g) == (1, 1, 1), q
        assert (q["window_picks_exact"], q["window_forwards_exact"]) == ((1, 1) if k == 1 else (0, 0)), (k, q, g[4])
        assert (g[4]["picks_spec"], g[4]["forwards_spec"]) == ((0, 0) if k == 1 else (1, 1)), (k, g[4])
    assert got[1][4]["n_hits"] > got[1][4]["cap_hits"] and got[1][4]["n_pairs"] > got[1][4]["cap_pairs"]
    _state(ctx, pair)


def test_limits(ctx, base, pair):
    from emqx_amd._lib import GpuMatchError
    # more than 1 MiB of text: cut into groups, the state carried across
    pad = [b"q/" + b"a" * 1000] * 30
    got = pair.check([_topics(20, 40 + k) + pad for k in range(40)], seed=1)
    assert got[-1][4]["group"]["seq"] >= 1 and all(g[4]["group"]["grouped"] for g in got)
    # a topic past 65,535 B: that window runs alone, in its place
    long_w = _topics(10, 50) + [b"t/1/" + b"b" * 70000]
    got = pair.check([_topics(30, 51), long_w, _topics(31, 52)], seed=2)
    assert [g[4]["group"]["grouped"] for g in got] == [1, 0, 1]
    assert [g[4]["group"]["seq"] for g in got] == [0, 1, 2]
    # an overlay snapshot takes the ordinary path: the error of the call alone
    plain = ctx.build_index(base[0])
    ov = ctx.update_index(plain, [(b"a/#/b", True)])
    try:
        with pytest.raises(GpuMatchError) as direct:
            ctx.publish_window(ov, _topics(5))
        with pytest.raises(GpuMatchError) as grouped:
            ctx.publish_windows(ov, _windows([5, 6]))
        assert grouped.value.code == direct.value.code and "overlay" in str(grouped.value)
    finally:
        ov.release()
        plain.release()


def test_two_member_context_equals_the_single_device(ctx, base):
    from emqx_amd import Context
    windows = _windows([65, 1024, 0, 300], 30)
    ref = Pair(ctx, base[1], base[0])  # fresh tables: the state the two-member context's own start from
    try:
        want = [ref.solo(1, w, seed=7) for w in windows] + [ref.solo(1, windows[0], seed=8)]
    finally:
        ref.release()
    with Context(devices=[0, 0]) as c2:
        index = c2.build_index(base[0], subs=_subs(base[0]))
        sh = c2.build_shared(index, _slots(base[0]))
        dt = c2.build_dests(index, _routes(base[0], 65), 65)
        try:
            got = c2.publish_windows(index, windows, shared=sh, seed=7, dests=dt, skip_node=0, group_stats=True)
            got.append(c2.publish_window(index, windows[0], shared=sh, seed=8, dests=dt, skip_node=0))
            for k in range(len(want)):
                assert_same(got[k], want[k])
            assert got[0][4]["group"]["n_windows"] == 4
        finally:
            sh.release()
            dt.release()
            index.release()


def _state(ctx, pair):
    after = _topics(64, seed=99)
    for strategy in ("round_robin", "sticky"):
        assert_same(pair.solo(0, after, strategy, None, 3), pair.solo(1, after, strategy, None, 3))


def test_errors_leave_outputs_and_state_alone(ctx, base, pair):
    from emqx_amd import _lib, pack
    from emqx_amd._lib import GpuMatchError
    windows = _windows([50, 60], 14)
    pair.check(windows, seed=1)
    L = _lib.lib()
    packed = [pack(w) for w in windows]

    def call(opts, hashes=(None, None), break_offsets=False, wins=True, out=True):
        w = (_lib.PublishWin * 2)()
        keep = []
        for k, (tb, to) in enumerate(packed):
            if break_offsets and k == 1:
                to = to.copy()
                to[3] = to[2] - 1
            keep.append(to)
            w[k].w.topic_bytes, w[k].w.topic_off, w[k].w.n_topics = tb.ctypes.data, to.ctypes.data, len(to) - 1
            w[k].msg_hash = hashes[k].ctypes.data if hashes[k] is not None else None
        res = (_lib.PublishResult * 2)()
        C.memset(res, 0xAB, C.sizeof(res))
        before = bytes(res)
        rc = L.emqx_gm_publish_windows(ctx.h, pair.index.h, w if wins else None, 2, C.byref(opts) if opts else None,
                                       res if out else None, None, None)
        assert bytes(res) == before  # a refused call touches no output
        return rc

    def opts(strategy=1, flags=None, msg_hash=None, shared=True, dests=True):
        o = _lib.PublishOpts()
        o.flags = _lib.WITH_EXACT if flags is None else flags
        o.shared = pair.sh[0].h if shared else None
        o.dests = pair.dt[0].h if dests else None
        o.strategy, o.msg_hash = strategy, msg_hash
        return o

    h = _hashes(60)
    assert call(None) == _lib.EINVAL
    assert call(opts(), wins=False) == _lib.EINVAL
    assert call(opts(), out=False) == _lib.EINVAL
    assert call(opts(flags=0x40000000)) == _lib.EINVAL
    assert call(opts(), break_offsets=True) == _lib.EINVAL
    assert call(opts(strategy=17)) == _lib.EINVAL
    assert call(opts(strategy=_lib_strategy("hash")), hashes=(_hashes(50), None)) == _lib.EINVAL  # a window lacks its hashes
    assert call(opts(msg_hash=h.ctypes.data)) == _lib.EINVAL
    assert L.emqx_gm_publish_windows(None, pair.index.h, None, 0, None, None, None, None) == _lib.EINVAL
    other = ctx.build_index(base[0], subs=[[j] for j in range(len(base[0]))])  # the same filters, another snapshot
    try:
        for kw in (dict(shared=pair.sh[0]), dict(dests=pair.dt[0])):
            with pytest.raises(GpuMatchError) as e:
                ctx.publish_windows(other, windows, **kw)
            assert e.value.code == _lib.EINVAL
    finally:
        other.release()
    _state(ctx, pair)  # the state did not move


def _lib_strategy(name):
    from emqx_amd.shared import _strategy
    return _strategy(name)


# ---------------------------------------------------------------- the combiner
def _threads(fns):
    bad = []

    def run(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001
            bad.append(repr(e))

    ts = [threading.Thread(target=run, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:2]


def test_combiner_forms_one_group_of_four(ctx, pair):
    windows = _windows([40, 50, 60, 70], 60)
    got = [None] * 4
    with ctx.combiner(min_windows=4, linger_us=5_000_000) as cb:
        _threads([lambda k=k: got.__setitem__(k, pair.solo(0, windows[k], "hash", _hashes(len(windows[k]), k), 0, 0, cb))
                  for k in range(4)])
        st = cb.stats()
    assert st["groups"] == 1 and st["max_group"] == 4, st
    for k in range(4):
        q = got[k][4]["group"]
        assert q["n_windows"] == 4 and q["seq"] == 0 and q["grouped"] == 1, q
        assert_same(got[k], pair.solo(1, windows[k], "hash", _hashes(len(windows[k]), k)))
    assert sorted(g[4]["group"]["position"] for g in got) == [0, 1, 2, 3]


def test_combiner_round_robin_order_is_the_reported_one(ctx, pair):
    """8 threads x round robin: replaying the windows through publish_window on B
    in (sequence, position) order gives the same results and the same final state."""
    per = 6
    windows = {(t, k): _topics(40 + 3 * t + k, seed=200 + 10 * t + k) for t in range(8) for k in range(per)}
    got = {}
    with ctx.combiner() as cb:
        def run(t):
            for k in range(per):
                got[(t, k)] = pair.solo(0, windows[(t, k)], "round_robin", None, 11, 0, cb)
        _threads([lambda t=t: run(t) for t in range(8)])
    order = sorted(got, key=lambda key: (got[key][4]["group"]["seq"], got[key][4]["group"]["position"]))
    assert len({(got[k][4]["group"]["seq"], got[k][4]["group"]["position"]) for k in order}) == len(order)
    for key in order:
        assert_same(got[key], pair.solo(1, windows[key], "round_robin", None, 11))
    _state(ctx, pair)


def test_combiner_keeps_kinds_and_opts_apart(ctx, pair):
    """Publish windows and match windows on one combiner never share a group, nor do windows of differing opts."""
    w = _windows([30, 31, 32, 33], 70)
    out = [None] * 4
    with ctx.combiner(min_windows=4, linger_us=50_000) as cb:
        _threads([lambda: out.__setitem__(0, pair.solo(0, w[0], "random", None, 1, 0, cb)),
                  lambda: out.__setitem__(1, pair.solo(0, w[1], "random", None, 2, 0, cb)),  # another seed
                  lambda: out.__setitem__(2, cb.match_fanout(pair.index, w[2])),
                  lambda: out.__setitem__(3, cb.match_fanout(pair.index, w[3]))])
        st = cb.stats()
    assert st["windows"] == 4 and st["groups"] >= 3, st
    assert out[0][4]["group"]["n_windows"] == 1 and out[1][4]["group"]["n_windows"] == 1
    assert_same(out[0], pair.solo(1, w[0], "random", None, 1))
    assert_same(out[1], pair.solo(1, w[1], "random", None, 2))
    for k in (2, 3):
        m, d = ctx.match_fanout(pair.index, w[k])
        assert all(np.array_equal(a, b) for a, b in zip(out[k][0] + out[k][1], m + d))


def test_combiner_bad_window_fails_alone(ctx, pair):
    from emqx_amd import _lib
    from emqx_amd._lib import GpuMatchError
    w = _windows([30, 31], 80)
    out = [None, None]

    def bad():
        with pytest.raises(GpuMatchError) as e:
            pair.solo(0, w[0], "hash", None, 0, 0, cb)  # no hashes
        out[0] = e.value.code

    with ctx.combiner(min_windows=2, linger_us=50_000) as cb:
        _threads([bad, lambda: out.__setitem__(1, pair.solo(0, w[1], "hash", _hashes(31), 0, 0, cb))])
    assert out[0] == _lib.EINVAL
    assert_same(out[1], pair.solo(1, w[1], "hash", _hashes(31)))
    _state(ctx, pair)


class _Box:
    def __init__(self):
        self.box = []

    def append(self, x):
        self.box.append(x)


def _batcher_world(ctx, cb):
    from emqx_amd import ClusterRoutes
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    from emqx_amd.shared import SharedSub
    cluster = ClusterRoutes(ctx, node=b"n1")
    routes = GpuRoutes(ctx, node=b"n1", cluster=cluster, combiner=cb)
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
                        shared=sh, shared_strategy="round_robin", cluster=cluster, one_call=True,
                        forward_batch=lambda node, pairs: batches.append((node, pairs)) or ("ok", "fwd"))
    out = [pb.publish_batch(items[:120]), pb.publish_batch(items[120:])]
    res = out, [b.box for b in local], [b.box for b in members], batches, dict(pb.metrics)
    sh.release()
    cluster.release()
    return res


def test_batcher_one_call_through_a_combiner_equals_one_call(ctx):
    with ctx.combiner() as cb:
        a = _batcher_world(ctx, cb)
        assert cb.stats()["windows"] == 2
    b = _batcher_world(ctx, None)
    assert a == b
    assert sum(len(m) for m in a[2]) == 200 + 200 + 1 and len(a[3]) >= 3
