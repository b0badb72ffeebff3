"""GPU parity: the HIP hot path (through the C ABI) vs the CPU oracle.

Bit-exact for every row: filter ids are lexicographic ranks, rows sorted, so
equality of (row_off, ids) is equality of lists:sort/1 of the reference result.
"""

import os
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _oracle_rows(orc, filters, topics, mode, compact=True):
    r = orc.Router(compact)
    for f in filters:
        if mode == 1:
            r.add_route(f)
        else:  # emqx_trie semantics: the index holds exactly what was inserted
            r.trie.insert(f)
    ro, ids, _ = r.match_batch(topics, filters, mode=mode)
    return ro, ids


def _check(ctx, orc, filters, topics, exact=True):
    filters = sorted(set(f if isinstance(f, bytes) else f.encode() for f in filters))
    topics = [t if isinstance(t, bytes) else t.encode() for t in topics]
    idx = ctx.build_index(filters)
    ro, ids = ctx.match(idx, topics, exact=exact)
    oro, oids = _oracle_rows(orc, filters, topics, 1 if exact else 0)
    if not (np.array_equal(ro, oro) and np.array_equal(ids, oids)):
        for i in range(len(topics)):
            g = ids[ro[i]:ro[i + 1]].tolist()
            e = oids[oro[i]:oro[i + 1]].tolist()
            assert g == e, (topics[i], [filters[x] for x in g], [filters[x] for x in e])
    idx.release()
    return ro, ids


# ------------------------------------------------------------------ reference suite vectors
def test_trie_suite_vectors(ctx, golden):
    from emqx_amd import Trie
    for case in golden["trie_cases"]:
        t = Trie(ctx)
        for op, arg in case["ops"]:
            getattr(t, op)(arg)
        for q in case["queries"]:
            got = sorted(t.match(q["topic"]))
            if "expect_len" in q:
                assert len(got) == q["expect_len"], case["name"]
            else:
                assert got == sorted(x.encode() for x in q["expect"]), (case["name"], q, got)


def test_router_match_routes_vector(ctx, golden):
    from emqx_amd import Router
    g = golden["router_match_routes"]
    r = Router(ctx)
    for f in g["routes"]:
        r.add_route(f)
    got = sorted(f for f, _ in r.match_routes(g["topic"]))
    assert got == sorted(x.encode() for x in g["expect"])
    for f in g["routes"]:
        r.delete_route(f)
    assert r.match_routes(g["topic"]) == []


def test_broker_vectors(ctx, golden):
    from emqx_amd import Broker
    for case in golden["broker_cases"]:
        if case.get("force_shard"):
            continue
        b = Broker(ctx)
        for topic, pid in case["subs"]:
            b.subscribe(topic, pid)
        if not case["subs"]:
            b.router.add_route("unrelated/+")
        assert sorted(b.publish(case["publish"])) == sorted(case["expect_deliveries"]), case["name"]


def test_broker_shard_path(ctx):
    """More than 1,024 subscribers: the shard indirection is flattened and every
    subscriber is delivered exactly once (t_shard, emqx_broker_SUITE.erl:311-330)."""
    from emqx_amd import Broker
    b = Broker(ctx, schedulers=2)
    for p in range(1, 3001):
        b.subscribe("topic", p)
    b.subscribe("top/+", 9)
    assert sorted(b.publish("topic")) == list(range(1, 3001))
    assert b.publish("top/x") == [9]


# ------------------------------------------------------------------ randomised vs oracle
ALPH = ["a", "b", "c", "", "$x", "$SYS", "dd", "l0w1"]


def _rand_filter(rng):
    n = rng.randint(1, 5)
    ws = [rng.choice(ALPH) for _ in range(n)]
    k = rng.random()
    if k < 0.2:
        return "/".join(ws)
    if k < 0.6:
        return "/".join("+" if rng.random() < 1 / 3 else w for w in ws)
    if k < 0.8:
        return "/".join(ws[: rng.randint(0, n)] + ["#"])
    return "/".join(["+" if rng.random() < 1 / 3 else w for w in ws] + ["#"])


def _rand_topic(rng):
    n = rng.randint(1, 6)
    ws = [rng.choice(ALPH) for _ in range(n)]
    if rng.random() < 0.05:
        ws[rng.randrange(n)] = rng.choice(["+", "#"])
    return "/".join(ws)


def _layout_env(monkeypatch, layout):
    if layout == "mph_all_tables":  # every per-depth hot table placed by hash-and-displace (default: 4k..128k keys)
        monkeypatch.setenv("GM_MPH_MIN_KEYS", "1")
        monkeypatch.setenv("GM_CHAIN", "1")  # and chain nodes (default: past 256 MiB of hot tables)
    elif layout == "dense":
        # the dictionary at one slot per word and the hot tables at load 0.9, not
        # spread out: words and keys off their home slots, the probe loops the
        # sparse defaults make rare
        monkeypatch.setenv("GM_DICT_MUL", "1")
        monkeypatch.setenv("GM_HOT_SPARSE", "0")
        monkeypatch.setenv("GM_HOT_LOAD_PCT", "90")


LAYOUTS = ["open_addressing", "mph_all_tables", "dense"]


@pytest.mark.parametrize("mph", LAYOUTS)
@pytest.mark.parametrize("exact", [True, False], ids=["match_routes", "trie_match"])
def test_random_small_sets(ctx, orc, exact, mph, monkeypatch):
    _layout_env(monkeypatch, mph)
    rng = random.Random(11)
    for _ in range(40):
        filters = [_rand_filter(rng) for _ in range(rng.randint(1, 60))]
        topics = [_rand_topic(rng) for _ in range(300)]
        _check(ctx, orc, filters, topics, exact)


@pytest.mark.parametrize("mph", LAYOUTS)
def test_edge_cases(ctx, orc, mph, monkeypatch):
    _layout_env(monkeypatch, mph)
    filters = ["#", "+", "+/+", "/#", "/+", "$SYS/#", "$SYS/+", "$SYS", "sport/", "sport/+", "sport/#", "a/+/#",
               "", "+/#", "a//b", "a/+/b", "x/y", "a/+", "a/#/b", "é/+"]
    topics = ["", "/", "//", "sport", "sport/", "sport/x", "$SYS", "$SYS/", "$SYS/a", "$SYS/a/b", "a", "a/b",
              "a//b", "a/x/b", "x/y", "+", "#", "a/+", "a/#", "a/#/b", "sport/+", "$x", "é/1", "a/b/c/d/e/f"]
    for exact in (True, False):
        _check(ctx, orc, filters, topics, exact)


# ------------------------------------------------------------------ chain nodes (path compression)
CHAIN_FILTERS = [
    "a/b/c/d", "a/b/c/e/f", "a/b/x/y/z",        # chains of 1 and 2 words under a/b/c and a/b/x
    "a/b/c/#", "a/b/x/y", "a/b/x",              # a chain node's own '#' and end filters
    "p/+/q/r/s", "p/+/q/t",                     # under an inline '+' node (no chain there) and a slot '+'
    "+/k/l/m", "$SYS/s/t/u", "m/n/o/p/q/r/s",   # root '+' child, '$' words, a longer tail (chain at its last two)
    "w/1", "w/2/3", "w/2/4",                    # a depth-1 chain, a branching node
]
CHAIN_TOPICS = [
    "a/b/c/d", "a/b/c/d/e", "a/b/c", "a/b/c/e", "a/b/c/e/f", "a/b/c/e/g", "a/b/c/f/f", "a/b/x/y/z", "a/b/x/y",
    "a/b/x", "a/b/x/y/z/w", "a/b/x/q/z", "p/1/q/r/s", "p/1/q/t", "p/1/q/r", "z/k/l/m", "$SYS/k/l/m",
    "$SYS/s/t/u", "$SYS/s/t", "m/n/o/p/q/r/s", "m/n/o/p/q/r", "m/n/o/p/q/r/t", "w/1", "w/1/2", "w/2/3", "w/2",
    "w/2/4/5", "a/b/c/#", "a/b/+/d",
]


def test_chain_nodes_vs_oracle_and_no_chain(ctx, orc, monkeypatch):
    """Chain nodes (gm_common.h) take a filter's single-word or two-word tail
    out of the walk: the main pass checks the topic's next words at the chain
    node and emits the tail's filter there.  Rows equal the oracle and an
    index built without chains (GM_CHAIN=0), in both modes, for every topic
    length around each chain, '#' / end filters on the chain node, '+' paths
    and '$' topics."""
    topics = CHAIN_TOPICS + [t + "/x" for t in CHAIN_TOPICS]
    for exact in (True, False):
        monkeypatch.setenv("GM_CHAIN", "1")  # (by default only indexes past 256 MiB of hot tables get chains)
        ro, ids = _check(ctx, orc, CHAIN_FILTERS, topics, exact)
        monkeypatch.setenv("GM_CHAIN", "0")
        ro2, ids2 = _check(ctx, orc, CHAIN_FILTERS, topics, exact)
        assert np.array_equal(ro, ro2) and np.array_equal(ids, ids2)


def test_chain_nodes_random_deep(ctx, orc, monkeypatch):
    """Random filter sets with long unique tails (most deep nodes are chain
    nodes) against the oracle."""
    monkeypatch.setenv("GM_CHAIN", "1")
    rng = random.Random(7)
    words = ["a", "b", "c", "dd", "", "$e", "f1"]
    for _ in range(20):
        filters = set()
        for _ in range(rng.randint(5, 80)):
            n = rng.randint(1, 7)
            ws = [rng.choice(words) for _ in range(n)]
            if rng.random() < 0.3:
                ws[rng.randrange(n)] = "+"
            if rng.random() < 0.15:
                ws.append("#")
            filters.add("/".join(ws))
        topics = []
        for f in sorted(filters):  # every filter's path with its words (+ -> a word), cut and extended
            ws = [rng.choice(words) if w == "+" else w for w in f.split("/") if w != "#"]
            for cut in range(max(0, len(ws) - 3), len(ws) + 3):
                topics.append("/".join((ws + [rng.choice(words) for _ in range(3)])[:max(cut, 1)]))
        for exact in (True, False):
            _check(ctx, orc, sorted(filters), topics, exact)


def test_deep_and_long_topics(ctx, orc):
    deep = "/".join("abcdefghijklmnopqrstuvwxyz")
    filters = ["#", deep + "/#", deep + "/+", "+/" * 26 + "#", "/".join(["+"] * 1000), "/".join(["x"] * 999) + "/#",
               "w" * 5000 + "/+", "w" * 5000]
    topics = [deep, deep + "/1", "/".join(["x"] * 1000), "/".join(["x"] * 5000), "w" * 5000 + "/q", "w" * 5000,
              "w" * 4999 + "/q", "/".join(["y"] * 1000)]
    for exact in (True, False):
        _check(ctx, orc, filters, topics, exact)


def test_overflow_slow_path(ctx, orc):
    """Frontier > LDS capacity and > 16 matches per row go through the device
    slow path; results stay exact."""
    lv = ["a", "b", "c", "d", "e", "f"]
    filters = set()
    for m in range(1 << 6):  # every '+'/word mix over 6 levels, plus '#' tails
        ws = ["+" if (m >> i) & 1 else lv[i] for i in range(6)]
        filters.add("/".join(ws))
        filters.add("/".join(ws[:3]) + "/#")
        filters.add("/".join(ws[:5]) + "/#")
    topics = ["a/b/c/d/e/f", "a/b/c/d/e", "a/b/c", "a/x/c/d/e/f", "q/b/c/d/e/f", "a/b/c/d/e/f/g", "+/b"] * 20
    ro, ids = _check(ctx, orc, sorted(filters), topics, True)
    st = ctx.stats()
    assert int(np.max(np.diff(ro))) > 16
    _check(ctx, orc, sorted(filters), topics, False)


def test_hash_collision_safety(ctx, orc):
    """Words that share prefixes / lengths / 8-byte chunks never alias."""
    ws = ["a" * k for k in range(1, 20)] + ["ab" * k for k in range(1, 12)] + ["\x00", "\x00\x00", "a\x00", "\xff"]
    filters = [w + "/+" for w in ws] + [w + "/#" for w in ws[::2]] + ws
    topics = [w + "/z" for w in ws] + ws + [w + "b/z" for w in ws]
    _check(ctx, orc, filters, topics, True)


def test_empty_index_and_empty_batch(ctx, orc):
    idx = ctx.build_index([])
    ro, ids = ctx.match(idx, ["a/b", "", "#"], exact=True)
    assert ro.tolist() == [0, 0, 0, 0] and len(ids) == 0
    assert idx.empty()
    ro, ids = ctx.match(idx, [], exact=True)
    assert ro.tolist() == [0]
    idx.release()


# ------------------------------------------------------------------ workload configs
def test_device_topic_generator_matches_oracle(ctx, orc):
    from emqx_amd.engine import gen_filter_codes
    codes = gen_filter_codes(1, 1000)
    n = 20000
    db, do, tot = ctx.gen_topics_device(codes, 5, 1234, n)
    off = np.zeros(n + 1, np.uint64)
    ctx.memcpy_d2h(off, do, (n + 1) * 8)
    data = np.zeros(tot, np.uint8)
    ctx.memcpy_d2h(data, db, tot)
    ob, oo = orc.render_codes(orc.gen_topic_codes(5, 1234, n, codes))
    assert np.array_equal(off, oo) and bytes(data) == bytes(ob[:oo[-1]])
    ctx.dev_free(db)
    ctx.dev_free(do)


@pytest.mark.parametrize("wild_only,flat", [(False, False), (True, False), (True, True)],
                         ids=["C1-mix", "C2-wildcard", "C2-wildcard-flat-loads"])
def test_config_subsample_vs_oracle(ctx, orc, wild_only, flat, monkeypatch):
    """C1 (10k mixed filters) and C2-shaped (wildcard-only) filter sets, 200k
    seeded topics generated on the device, every row vs the oracle.  flat: the
    index is built with GM_HOT_FLAT, so the walk uses the flat-load path that
    an index with a >= 2 GiB hot table takes instead of buffer loads."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(1, 10_000 if not wild_only else 50_000, wildcard_only=wild_only)
    fb, fo = render_codes(codes)
    filters = sorted(set(orc.unpack(fb, fo)))
    if flat:
        monkeypatch.setenv("GM_HOT_FLAT", "1")
    idx = ctx.build_index(filters)
    monkeypatch.delenv("GM_HOT_FLAT", raising=False)
    n = 200_000
    db, do, tot = ctx.gen_topics_device(codes, 1, 0, n)
    res = ctx.match_device(idx, db, do, n, exact=True)
    ro, ids = res.to_host()
    tb, to = orc.render_codes(orc.gen_topic_codes(1, 0, n, codes))
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    oro, oids, _ = r.match_batch((tb, to), filters, mode=1, nthreads=8)
    assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
    res.free()
    ctx.dev_free(db)
    ctx.dev_free(do)
    idx.release()


def test_large_batch_properties(ctx, orc):
    """A 4M-topic batch at C2 shape: sorted unique rows, ids in range, every
    derived topic matches >= 1 filter, and a strided sample equals the oracle."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(2, 200_000, wildcard_only=True)
    fb, fo = render_codes(codes)
    filters = sorted(set(orc.unpack(fb, fo)))
    idx = ctx.build_index(filters)
    n = 4_000_000
    db, do, tot = ctx.gen_topics_device(codes, 2, 0, n)
    res = ctx.match_device(idx, db, do, n, exact=True)
    ro, ids = res.to_host()
    d = np.diff(ro.astype(np.int64))
    assert (d >= 0).all() and int(ro[-1]) == len(ids)
    assert (ids < len(filters)).all()
    # rows strictly increasing
    inner = np.ones(len(ids), bool)
    inner[ro[:-1][d > 0].astype(np.int64)] = False
    assert (np.diff(ids.astype(np.int64))[inner[1:]] > 0).all()
    # sample vs oracle
    sample = np.arange(0, n, 997)
    tc = np.concatenate([orc.gen_topic_codes(2, int(i), 1, codes) for i in sample])
    tb, to = orc.render_codes(tc)
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    oro, oids, _ = r.match_batch((tb, to), filters, mode=1)
    for k, i in enumerate(sample):
        assert ids[ro[i]:ro[i + 1]].tolist() == oids[oro[k]:oro[k + 1]].tolist()
    res.free()
    ctx.dev_free(db)
    ctx.dev_free(do)
    idx.release()


# ------------------------------------------------------------------ fan-out
def test_fanout_vs_oracle(ctx, orc):
    rng = np.random.default_rng(3)
    filters = sorted({b"a/#", b"a/+", b"a/b", b"+/b", b"#", b"c/d", b"a/+/c"})
    subs = [rng.integers(0, 1 << 20, size=int(rng.integers(0, 3000))).astype(np.uint32).tolist() for _ in filters]
    idx = ctx.build_index(filters, subs=subs)
    topics = [b"a/b", b"a/x", b"c/d", b"q", b"a/b/c", b"$SYS/a"] * 50
    ro, ids = ctx.match(idx, topics, exact=True)
    fro, fids = ctx.fanout(idx, ro, ids)
    so = np.zeros(len(filters) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in subs])
    si = np.array([x for s in subs for x in s], np.uint32)
    ero, eids = orc.fanout(ro, ids, so, si)
    assert np.array_equal(fro, ero) and np.array_equal(fids, eids)
    idx.release()


def test_hot_fanout_c4_small(ctx, orc):
    """C4 shape at 1/10 scale: 100 hot topics x 100k deliveries each."""
    K, S = 100, 100_000
    filters = [b"hot/#", b"hot/+/x/#"] + [b"hot/%d/x/y/z" % k for k in range(K)]
    subs = [list(range(0, 60_000)), list(range(60_000, S - 10 * K))] + \
           [list(range(S - 10 * K + 10 * k, S - 10 * K + 10 * k + 10)) for k in range(K)]
    idx = ctx.build_index(filters, subs=subs)
    topics = [b"hot/%d/x/y/z" % k for k in range(K)]
    ro, ids = ctx.match(idx, topics, exact=True)
    fro, fids = ctx.fanout(idx, ro, ids)
    assert np.all(np.diff(fro) == 60_000 + (S - 10 * K - 60_000) + 10)
    perm = idx.perm
    so = np.zeros(len(filters) + 1, np.uint64)
    order = np.argsort(perm)
    ssorted = [subs[i] for i in order]
    so[1:] = np.cumsum([len(s) for s in ssorted])
    si = np.array([x for s in ssorted for x in s], np.uint32)
    ero, eids = orc.fanout(ro, ids, so, si)
    assert np.array_equal(fro, ero) and np.array_equal(fids, eids)
    idx.release()


def test_small_fanout_equals_locked_path(ctx, orc, monkeypatch):
    """Host-row fan-outs of publish windows (gm_host.cpp run_fanout_small: the
    deliveries into a speculative capacity, one device round trip,
    the context lock held only to queue) give the rows of the one-at-a-time
    path (GM_FANOUT_SIMPLE) and the oracle's: on a built index and after
    update_subs deltas, with empty rows, filters without subscribers, a
    fan-out past the call's speculative capacity (the ordinary path) and one
    past 1 MiB of deliveries (copy-engine rows), from four threads at once;
    rows that are not a plain CSR over [0, nnz) take the ordinary path, and a
    filter id out of range is EINVAL."""
    import threading
    from emqx_amd._lib import GpuMatchError
    rng = np.random.default_rng(5)
    filters = sorted({b"a/#", b"a/+", b"a/b", b"+/b", b"#", b"c/d", b"a/+/c", b"none/+"})
    subs = [rng.integers(0, 1 << 20, size=int(rng.integers(1, 400))).astype(np.uint32).tolist() for _ in filters]
    subs[filters.index(b"none/+")] = []
    idx = ctx.build_index(filters, subs=subs)
    idx2 = ctx.update_subs(idx, [(b"a/b", 7, True), (b"#", int(subs[filters.index(b"#")][0]), False),
                                 (b"zz/+", 9, True), (b"c/d", 11, True)])
    topics = [b"a/b", b"a/x", b"c/d", b"q", b"a/b/c", b"$SYS/a", b"none/x", b"zz/q"] * 40
    for ix in (idx, idx2):
        ro, ids = ctx.match(ix, topics, exact=True)
        one_row = np.array([0, len(ids)], np.uint64)  # every match in one row
        monkeypatch.setenv("GM_FANOUT_SIMPLE", "1")
        want = ctx.fanout(ix, ro, ids)
        want_one = ctx.fanout(ix, one_row, ids)
        monkeypatch.delenv("GM_FANOUT_SIMPLE")
        got = ctx.fanout(ix, ro, ids)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got_one = ctx.fanout(ix, one_row, ids)
        assert np.array_equal(got_one[0], want_one[0]) and np.array_equal(got_one[1], want_one[1])
        assert ctx.fanout(ix, np.zeros(1, np.uint64), np.zeros(0, np.uint32))[0].tolist() == [0]
        # (a slice whose offsets start past 0: the ordinary path, same rows as that path gives)
        sl = ro[3:10].copy()
        monkeypatch.setenv("GM_FANOUT_SIMPLE", "1")
        want_sl = ctx.fanout(ix, sl - sl[0], ids[int(sl[0]):int(sl[-1])])
        monkeypatch.delenv("GM_FANOUT_SIMPLE")
        got_sl = ctx.fanout(ix, sl - sl[0], ids[int(sl[0]):int(sl[-1])])
        assert np.array_equal(got_sl[1], want_sl[1])
        errs, outs = [], [None] * 4

        def one(k):
            try:
                for _ in range(25):
                    outs[k] = ctx.fanout(ix, ro, ids)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=one, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[0]
        for o in outs:
            assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1])
    # the built index against the oracle
    ro, ids = ctx.match(idx, topics, exact=True)
    fro, fids = ctx.fanout(idx, ro, ids)
    so = np.zeros(len(filters) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in subs])
    si = np.array([x for s in subs for x in s], np.uint32)
    ero, eids = orc.fanout(ro, ids, so, si)
    assert np.array_equal(fro, ero) and np.array_equal(fids, eids)
    # past the speculative capacity (the first call: the ordinary path), then
    # past 1 MiB of deliveries within it (the second: rows back on the copy engine)
    big = ctx.build_index([b"x/#"], subs=[list(range(300_000))])
    for _ in range(2):
        fro, fids = ctx.fanout(big, np.array([0, 1, 1, 2], np.uint64), np.zeros(2, np.uint32))
        assert fro.tolist() == [0, 300_000, 300_000, 600_000]
        assert np.array_equal(fids[:300_000], np.arange(300_000)) and np.array_equal(fids[300_000:], np.arange(300_000))
    with pytest.raises(GpuMatchError) as e:
        ctx.fanout(big, np.array([0, 1], np.uint64), np.array([5], np.uint32))
    assert "out of range" in str(e.value)
    big.release()
    idx2.release()
    idx.release()


def test_match_fanout_one_round_trip(ctx, orc, monkeypatch):
    """emqx_gm_match_fanout (the NIF's fanout_batch: route + dispatch of a
    publish window) equals emqx_gm_match followed by emqx_gm_fanout, and the
    oracle's rows and deliveries: with the fan-out fused into the match's round
    trip (GM_FANOUT_FUSED_ONLY: an error unless it held), and when it cannot
    hold -- the first wide fan-out past its capacity, no speculative match
    buffer (GM_NO_SPEC_IDS), a batch of more than one chunk, an overlay
    snapshot (EUNSUPPORTED, nothing leaked) -- in both match modes, from four
    threads at once, the empty batch included."""
    import threading
    from emqx_amd._lib import GpuMatchError
    from emqx_amd.engine import pack
    rng = np.random.default_rng(9)
    filters = sorted({b"a/#", b"a/+", b"a/b", b"+/b", b"#", b"c/d", b"a/+/c", b"none/+", b"x/y/z"})
    subs = [rng.integers(0, 1 << 20, size=int(rng.integers(1, 300))).astype(np.uint32).tolist() for _ in filters]
    subs[filters.index(b"none/+")] = []
    idx = ctx.build_index(filters, subs=subs)
    so = np.zeros(len(filters) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in subs])
    si = np.array([x for s in subs for x in s], np.uint32)
    topics = [b"a/b", b"a/x", b"c/d", b"q", b"a/b/c", b"$SYS/a", b"none/x", b"x/y/z"] * 64

    def want(ix, tps, exact=True):
        ro, ids = ctx.match(ix, tps, exact=exact)
        monkeypatch.setenv("GM_FANOUT_SIMPLE", "1")
        d = ctx.fanout(ix, ro, ids)
        monkeypatch.delenv("GM_FANOUT_SIMPLE")
        return (ro, ids), d

    def same(a, b):
        return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))

    for exact in (True, False):
        got = ctx.match_fanout(idx, topics, exact=exact)  # (warms the context's deliveries per match)
        assert same(got, want(idx, topics, exact))
        monkeypatch.setenv("GM_FANOUT_FUSED_ONLY", "1")
        got = ctx.match_fanout(idx, topics, exact=exact)
        monkeypatch.delenv("GM_FANOUT_FUSED_ONLY")
        assert same(got, want(idx, topics, exact))
    (ro, ids), (fro, fids) = ctx.match_fanout(idx, topics)
    oro, oids = _oracle_rows(orc, filters, topics, 1)
    ero, eids = orc.fanout(oro, oids, so, si)
    assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
    assert np.array_equal(fro, ero) and np.array_equal(fids, eids)
    assert same(ctx.match_fanout(idx, []), want(idx, []))
    # after update_subs (the device subscriber CSR replaced)
    idx2 = ctx.update_subs(idx, [(b"a/b", 7, True), (b"zz/+", 9, True), (b"c/d", 11, True)])
    t2 = topics + [b"zz/q"] * 5
    assert same(ctx.match_fanout(idx2, t2), want(idx2, t2))
    # no speculative match buffer: the fan-out after the match
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    assert same(ctx.match_fanout(idx, topics), want(idx, topics))
    monkeypatch.delenv("GM_NO_SPEC_IDS")
    # a wide fan-out: past the capacity the first time, fused (copy-engine rows) after
    big = ctx.build_index([b"x/#", b"y"], subs=[list(range(300_000)), [5]])
    bt = [b"x/1", b"y", b"x/2/3", b"q"]
    assert same(ctx.match_fanout(big, bt), want(big, bt))
    monkeypatch.setenv("GM_FANOUT_FUSED_ONLY", "1")
    assert same(ctx.match_fanout(big, bt), want(big, bt))
    monkeypatch.delenv("GM_FANOUT_FUSED_ONLY")
    # more than one chunk: the two calls in turn
    monkeypatch.setenv("GM_HOST_CHUNK", "1024")
    many = topics * 4
    assert same(ctx.match_fanout(idx, many), want(idx, many))
    monkeypatch.delenv("GM_HOST_CHUNK")
    # concurrent callers
    errs, outs = [], [None] * 4
    ref = want(idx, topics)

    def one(k):
        try:
            for _ in range(20):
                outs[k] = ctx.match_fanout(idx, topics)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=one, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs[0]
    assert all(same(o, ref) for o in outs)
    # an overlay snapshot (a filter with '#' inside): the fan-out refuses it, nothing is returned
    plain = ctx.build_index(filters)
    ov = ctx.update_index(plain, [(b"a/#/b", True)])
    with pytest.raises(GpuMatchError) as e:
        ctx.match_fanout(ov, topics)
    assert "overlay" in str(e.value)
    tb, to = pack(topics)
    assert same(ctx.match_fanout(idx, (tb, to)), ref)
    for x in (ov, plain, big, idx2, idx):
        x.release()


def test_tokenizer_alignments_and_bytes(ctx, orc):
    """Words of every length 0..19 at every byte alignment, with bytes next to
    '/' in value ('.', '0', 0x2E, 0x30, NUL, 0xFF) right after separators: the
    staged 8-byte (SWAR) word scan must cut and hash exactly like the oracle."""
    rng = random.Random(17)
    alphabet = [b".", b"0", b"a", b"\x00", b"\xff", b"\x2e", b"\x30", b"z"]
    words = [b"".join(rng.choice(alphabet) for _ in range(k)) for k in range(20) for _ in range(3)]
    filters = set()
    for w in words:
        filters.add(w + b"/+")
        filters.add(b"+/" + w)
        filters.add(w + b"/#")
        filters.add(w)
    topics = []
    for pad in range(9):  # shift the topic start through all 8-byte alignments
        for _ in range(40):
            a, b = rng.choice(words), rng.choice(words)
            topics.append(b"p" * pad + b"/" + a + b"/" + b)
            topics.append(a + b"/" + b)
            topics.append(a)
    _check(ctx, orc, sorted(filters), topics, True)
    _check(ctx, orc, sorted(filters), topics, False)


@pytest.mark.gpu
def test_tokenizer_group_and_depth_boundaries(ctx, orc):
    """k_match_fused's tokenizer resolves a topic's words into registers three
    levels at a time, eight levels at the most: wildcard words, '$' first
    words, empty levels and a trailing '/' on either side of a group boundary,
    and topics deeper than the 8 tokenized levels (finished by the listed
    pass), must give the same rows as the oracle."""
    rng = random.Random(23)
    words = [b"a", b"b", b"", b"cc", b"longword_over_8_bytes", b"$SYS", b"d"]
    filters = {b"#", b"+", b"+/+", b"a/#", b"$SYS/#", b"+/b/#", b"a/b/cc", b"/#", b"a//cc", b"a/b/"}
    for _ in range(200):
        n = rng.randint(1, 12)
        lev = [rng.choice(words + [b"+"]) for _ in range(n)]
        if rng.random() < 0.5:
            lev[-1] = b"#"
        filters.add(b"/".join(lev))
    topics = [b"", b"/", b"a/", b"$SYS/x", b"a/b/cc", b"a//cc", b"a/b/"]
    for _ in range(1500):
        n = rng.randint(1, 14)
        lev = [rng.choice(words) for _ in range(n)]
        if rng.random() < 0.1:  # a wildcard word at any level, including past the group / 8-level bounds
            lev[rng.randrange(n)] = rng.choice([b"+", b"#"])
        topics.append(b"/".join(lev))
    _check(ctx, orc, sorted(filters), topics, True)
    _check(ctx, orc, filters, topics, False)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [1, 3, 4097, 65_539, 200_003])
def test_fanout_long_rows_ragged(ctx, orc, row):
    """Fan-out rows of ragged lengths (not multiples of 4, shorter and longer
    than a workgroup's output range): workgroups inside one long row take the
    hoisted single-segment copy with a 1-3 element tail, the others the
    per-segment path; the result must equal the oracle's multiset rows."""
    filters = [b"a/#", b"a/+", b"a/b", b"c"]
    subs = [list(range(7, 7 + row)), [5, 3, 1], list(range(1000, 1000 + row // 3 + 1)), [9]]
    idx = ctx.build_index(filters, subs=subs)
    topics = [b"a/b", b"a/x", b"c", b"a/b", b"a", b"zz"]
    ro, ids = ctx.match(idx, topics, exact=True)
    fro, fids = ctx.fanout(idx, ro, ids)
    order = np.argsort(idx.perm)
    ssorted = [subs[i] for i in order]
    so = np.zeros(len(filters) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in ssorted])
    si = np.array([x for s in ssorted for x in s], np.uint32)
    ero, eids = orc.fanout(ro, ids, so, si)
    assert np.array_equal(fro, ero) and np.array_equal(fids, eids)
    idx.release()


# ------------------------------------------------------------------ fan-out split over devices (C4)
@pytest.mark.parametrize("n_parts", [1, 2, 3, 8])
def test_fanout_parts_cover_disjointly(ctx, orc, n_parts):
    """emqx_gm_fanout_part: the parts are contiguous, disjoint, carry the
    global row offsets, and concatenated equal the whole fan-out (1/10-scale C4:
    every part cuts through 100k-wide rows)."""
    from tests._fanout_part_worker import c4_small
    from emqx_amd.engine import pack
    filters, subs, topics = c4_small()
    idx = ctx.build_index(filters, subs=subs)
    tb, to = pack(topics)
    d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
    ctx.memcpy_h2d(d_tb, tb, len(tb))
    ctx.memcpy_h2d(d_to, to, len(to) * 8)
    m = ctx.match_device(idx, d_tb, d_to, len(topics), exact=True)
    whole = ctx.fanout_device(idx, m)
    w_ro, w_ids = whole.rows(0, len(topics))
    pos, got = 0, []
    for p in range(n_parts):
        part, first = ctx.fanout_part(idx, m, p, n_parts)
        assert first == pos
        g_ro = np.zeros(len(topics) + 1, np.uint64)
        ctx.memcpy_d2h(g_ro, ctypes.cast(part.csr.row_off, ctypes.c_void_p).value,
                       g_ro.nbytes)
        assert np.array_equal(g_ro, w_ro)
        if part.nnz:
            ids = np.zeros(part.nnz, np.uint32)
            ctx.memcpy_d2h(ids, ctypes.cast(part.csr.ids, ctypes.c_void_p).value,
                           part.nnz * 4)
            got.append(ids)
        pos += part.nnz
        part.free()
    assert pos == len(w_ids) == 100 * 99_010  # 60,000 + 39,000 + 10 per hot topic
    assert np.array_equal(np.concatenate(got), w_ids)
    mro, mids = m.to_host()
    order = np.argsort(idx.perm)
    ssorted = [subs[i] for i in order]
    so = np.zeros(len(filters) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in ssorted])
    si = np.array([x for s in ssorted for x in s], np.uint32)
    ero, eids = orc.fanout(mro, mids, so, si)
    assert np.array_equal(w_ro, ero) and np.array_equal(w_ids, eids)
    for x in (whole, m):
        x.free()
    ctx.dev_free(d_tb)
    ctx.dev_free(d_to)
    idx.release()


@pytest.mark.timeout(300)
def test_fanout_split_two_ranks():
    """The C4 split as two processes (gloo rank plumbing, both on device 0):
    rank 0 gathers both parts and checks disjoint, complete coverage against
    the oracle (tests/_fanout_part_worker.py)."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "tests", "_fanout_part_worker.py")]
    p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "FANOUT_SPLIT_OK world=2 deliveries=9901000" in p.stdout


# ------------------------------------------------------------------ host-buffer path (gm_host.cpp)
@pytest.mark.parametrize("chunk,wide", [("1024", "0"), ("5000", "0"), ("4194304", "0"), ("5000", "1")])
def test_host_path_chunks_equal_device_path(ctx, orc, monkeypatch, chunk, wide):
    """emqx_gm_match on host buffers -- chunked (GM_HOST_CHUNK topics), staged
    through pinned memory with u16 topic lengths (the device scans them into
    offsets), three chunks in flight -- gives the rows of one DEVICE_IO call over the same batch, which
    a strided sample ties to the oracle.  Small chunks put many chunk
    boundaries (and partial last chunks) in one call.  wide: the row offsets
    return as u64 (the form a chunk of 2^32 ids or more takes)."""
    monkeypatch.setenv("GM_HOST_WIDE_ROWS", wide)
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(7, 20_000)
    fb, fo = render_codes(codes)
    filters = sorted(set(orc.unpack(fb, fo)))
    idx = ctx.build_index(filters)
    n = 300_007
    tb, to = orc.render_codes(orc.gen_topic_codes(7, 0, n, codes))
    tb = np.concatenate([tb, np.zeros(64, np.uint8)])
    monkeypatch.setenv("GM_HOST_CHUNK", chunk)
    ro, ids = ctx.match(idx, (tb, to), exact=True)
    d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
    ctx.memcpy_h2d(d_tb, tb, len(tb))
    ctx.memcpy_h2d(d_to, to, len(to) * 8)
    res = ctx.match_device(idx, d_tb, d_to, n, exact=True)
    dro, dids = res.to_host()
    assert np.array_equal(ro, dro) and np.array_equal(ids, dids)
    sample = list(range(0, n, 1009)) + [n - 1]
    topics = orc.unpack(tb, to)
    oro, oids = _oracle_rows(orc, filters, [topics[i] for i in sample], 1)
    for j, i in enumerate(sample):
        assert ids[ro[i]:ro[i + 1]].tolist() == oids[oro[j]:oro[j + 1]].tolist()
    res.free()
    ctx.dev_free(d_tb)
    ctx.dev_free(d_to)
    idx.release()


@pytest.mark.parametrize("chunk", ["1024", "default"])
def test_host_path_long_topics_take_u32_offsets(ctx, orc, monkeypatch, chunk):
    """The host path sends topic lengths as u16 (MQTT caps a topic at 65,535
    bytes, emqx_topic.erl:45), but the ABI takes any length: a chunk holding a
    longer topic goes up as u32 offsets instead.  Topics of 65,535, 65,536,
    70,000 and 200,000 bytes (one deep, one one long word) among 50k ordinary
    ones: rows equal the oracle's, with the default
    staging and with every chunk forced to u32 offsets (GM_HOST_OFF32)."""
    if chunk != "default":
        monkeypatch.setenv("GM_HOST_CHUNK", chunk)
    filters = [b"l0w1/+/#", b"#", b"x/+", b"+/+/+", b"deep/#", b"long"]
    idx = ctx.build_index(filters)
    topics = [b"l0w1/a/b", b"x/y", b"a/b/c"] * 16_000
    for n_bytes, at in ((65_535, 100), (65_536, 2_000), (70_000, 30_000), (200_000, 47_999)):
        # (hundreds of 299-byte levels: the oracle restates the reference's recursion, so
        # its stack bounds the depth a CPU check can take)
        deep = b"deep/" + b"/".join([b"w" * 299] * (n_bytes // 300 + 1))
        topics.insert(at, deep[:n_bytes])
        topics.insert(at + 1, b"x/" + b"z" * (n_bytes - 2))
    assert max(len(t) for t in topics) == 200_000 and len(topics) == 48_008
    want_ro, want_ids = _oracle_rows(orc, sorted(filters), topics, 1)
    for off32 in ("0", "1"):
        monkeypatch.setenv("GM_HOST_OFF32", off32)
        ro, ids = ctx.match(idx, topics, exact=True)
        assert np.array_equal(ro, want_ro) and np.array_equal(ids, want_ids), off32
    idx.release()


@pytest.mark.parametrize("spec", ["on", "off"])
def test_small_host_calls_every_staging_branch(ctx, orc, monkeypatch, spec):
    """Small host-buffer calls (gm_host.cpp run_host_small): copies of up to
    1 MiB run as kernels over mapped page-locked memory, larger ones on the copy
    engine (and page-locked caller text goes up from the caller's buffer); the
    rows land in the caller's result straight from the device when the call's
    speculative ids buffer held them, and are copied out at their exact size
    when it did not (a context primed on rowless topics, then heavy rows; or no
    speculative buffer at all: GM_NO_SPEC_IDS).  Every form gives the oracle's
    rows, the empty call included."""
    from emqx_amd.engine import pack
    if spec == "off":
        monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    filters = sorted({b"#", b"a/#", b"a/+", b"a/+/#", b"+/+", b"+/+/+", b"+/b/#", b"a/b", b"a/b/c", b"q/#"})
    idx = ctx.build_index(filters)
    rowless = [b"$SYS/x/%d" % i for i in range(3_000)]  # ('#' does not match '$' topics)
    heavy = [b"a/b/c", b"a/b", b"a/x/y", b"q/b/z", b"zz/b"] * 600
    big = heavy * 12  # 48k topics with the long ones below: 1.2 MB of text, past the mapped-copy limit
    big += [b"a/" + b"w" * 80 + b"/%d" % i for i in range(12_000)]
    for topics in ([], rowless, heavy, rowless, big, heavy[:7]):
        want_ro, want_ids = _oracle_rows(orc, filters, topics, 1)
        tb, to = pack(topics)
        ro, ids = ctx.match(idx, (tb, to), exact=True)
        assert np.array_equal(ro, want_ro) and np.array_equal(ids, want_ids), len(topics)
        pb = ctx.host_alloc(len(tb) + 64)  # the caller's text page-locked
        pb[:len(tb)] = tb
        ro, ids = ctx.match(idx, (pb, to), exact=True)
        ctx.host_free(pb)
        assert np.array_equal(ro, want_ro) and np.array_equal(ids, want_ids), ("pinned", len(topics))
    idx.release()


def test_host_path_rejects_bad_offsets_and_survives(ctx):
    """Non-monotone host offsets -> EINVAL with a message (no GPU fault, no
    partial result), and the context keeps working afterwards."""
    from emqx_amd._lib import GpuMatchError
    idx = ctx.build_index([b"a/+", b"b/#"])
    tb = np.frombuffer(b"a/xb/yb" + b"\0" * 64, np.uint8).copy()
    bad = np.array([0, 3, 2, 7], np.uint64)
    with pytest.raises(GpuMatchError) as e:
        ctx.match(idx, (tb, bad), exact=True)
    assert "monotone" in str(e.value)
    ro, ids = ctx.match(idx, (tb, np.array([0, 3, 6, 7], np.uint64)), exact=True)
    assert ro.tolist() == [0, 1, 2, 3] and ids.tolist() == [0, 1, 1]  # a/x; b/y, b via b/#
    idx.release()


@pytest.mark.timeout(300)
def test_adversarial_plus_chains_all_rows(ctx, orc):
    """Every word sequence of depth 1..8 over {w, +} (each also with '/#'),
    plus '#': a topic 'w/.../w' matches hundreds of filters, so almost every
    row overflows the main and listed passes into the device slow path
    (frontier bounded by the widest trie level, chunks of up to 16,384
    topics).  60k topics, every row against the oracle, in both modes."""
    import itertools
    fs = {b"#"}
    for d in range(1, 9):
        for ws in itertools.product([b"w", b"+"], repeat=d):
            fs.add(b"/".join(ws))
            fs.add(b"/".join(ws) + b"/#")
    filters = sorted(fs)
    rng = random.Random(31)
    topics = [b"/".join(rng.choice([b"w", b"w", b"w", b"x", b"$x"]) for _ in range(rng.randint(1, 10)))
              for _ in range(60_000)]
    idx = ctx.build_index(filters)
    for exact in (True, False):
        ro, ids = ctx.match(idx, topics, exact=exact)
        oro, oids = _oracle_rows(orc, filters, topics, 1 if exact else 0)
        assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
        assert ctx.stats()["n_overflow"] > 10_000  # the slow path really ran
    idx.release()


def test_broker_incremental_snapshots(ctx):
    """Broker snapshots between publishes come from emqx_gm_index_update_subs:
    subscribes past the 1,024-subscriber shard threshold, unsubscribes, a
    filter's last subscriber leaving (its route goes), wildcard filters;
    deliveries as multisets against the bookkeeping's subscribers/1."""
    from emqx_amd.routing import Broker
    rng = random.Random(8)
    b = Broker(ctx, schedulers=2)
    filters = ["hot/t", "hot/+", "hot/#", "a/b", "a/+/c", "#"]
    truth = {f: [] for f in filters}
    topics = ["hot/t", "hot/x", "a/b", "a/q/c", "z"]

    def expect(t):
        from emqx_amd import topic as T
        return sorted(s for f, l in truth.items() for s in l if T.match(t, f))

    hot = iter(range(10_000, 20_000))
    for rnd in range(8):
        for _ in range(250):  # hot/t grows past the shard threshold
            s = next(hot)
            b.subscribe("hot/t", s)
            truth["hot/t"].append(s)
        for _ in range(rng.randint(50, 700)):
            f = rng.choice(filters)
            if truth[f] and rng.random() < 0.3:
                s = rng.choice(truth[f])
                b.unsubscribe(f, s)
                truth[f].remove(s)
            else:
                s = rng.randrange(1, 5000)
                b.subscribe(f, s)
                if s not in truth[f]:
                    truth[f].append(s)
        if rnd == 5:  # every subscriber of a/b leaves: its route goes
            for s in list(truth["a/b"]):
                b.unsubscribe("a/b", s)
            truth["a/b"] = []
        for t in topics:
            assert sorted(b.publish(t)) == expect(t), (rnd, t)
        assert b.router.has_routes("a/b") == bool(truth["a/b"])
    assert len(truth["hot/t"]) > 1024  # the shard buckets were exercised


@pytest.mark.timeout(300)
def test_concurrent_calls_one_context(ctx, orc):
    """SURVEY §8b threading: one context, 8 threads at once (ctypes drops the
    GIL, so the library's calls really overlap and serialize on the context):
    host-buffer and device-buffer matches, fan-out, in-place updates and
    failing calls, each thread's results equal to a single-threaded run, and
    each failing call's message its own (emqx_gm_last_error is per thread)."""
    import threading
    from emqx_amd import GpuMatchError
    from emqx_amd.engine import pack
    rng = random.Random(99)
    filters = sorted({_rand_filter(rng).encode() for _ in range(400)})
    subs = [rng.sample(range(10_000), rng.randint(0, 5)) for _ in filters]
    topics = [_rand_topic(rng).encode() for _ in range(20_000)]
    idx = ctx.build_index(filters, subs=subs)
    plain = ctx.build_index(filters)
    want_ro, want_ids = ctx.match(idx, topics, exact=True)
    want_fro, want_fids = ctx.fanout(idx, want_ro, want_ids)
    tb, to = pack(topics)
    d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
    ctx.memcpy_h2d(d_tb, tb, len(tb))
    ctx.memcpy_h2d(d_to, to, len(to) * 8)
    errors, done = [], []

    def worker(k):
        try:
            r = random.Random(k)
            for it in range(12):
                kind = (k + it) % 4
                if kind == 0:
                    ro, ids = ctx.match(idx, topics, exact=True)
                    assert np.array_equal(ro, want_ro) and np.array_equal(ids, want_ids)
                elif kind == 1:
                    fro, fids = ctx.fanout(idx, want_ro, want_ids)
                    assert np.array_equal(fro, want_fro) and np.array_equal(fids, want_fids)
                    # and overlapping submits of device-buffer calls from this thread
                    pend = [ctx.match_submit(idx, d_tb, d_to, len(topics)) for _ in range(3)]
                    for pm in pend:
                        res = pm.wait()
                        ro, ids = res.to_host()
                        res.free()
                        assert np.array_equal(ro, want_ro) and np.array_equal(ids, want_ids)
                elif kind == 2:  # an update of the shared plain index (overlay or patch) and a match on it
                    new_f = b"k%d/%d/+" % (k, it)
                    t = b"k%d/%d/x" % (k, it)
                    new = ctx.update_index(plain, [(new_f, True)])
                    _, ids0 = ctx.match(plain, [t], exact=True)
                    _, ids = ctx.match(new, [t], exact=True)
                    assert [new.filter(i) for i in ids] == sorted([plain.filter(i) for i in ids0] + [new_f])
                    new.release()
                else:  # a failing call: bad offsets, this thread's own message
                    bad = (np.zeros(8, np.uint8), np.array([0, 5, 2], np.uint64))
                    with pytest.raises(GpuMatchError) as ei:
                        ctx.match(idx, bad, exact=True)
                    assert "offset" in str(ei.value) or "EINVAL" in str(ei.value)
            done.append(k)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((k, repr(e)))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:3]
    assert sorted(done) == list(range(8))
    ctx.dev_free(d_tb)
    ctx.dev_free(d_to)
    idx.release()
    plain.release()


@pytest.mark.parametrize("asm_stream", [None, "1"])
def test_submit_wait_pipelined_vs_oracle(ctx, orc, monkeypatch, asm_stream):
    """emqx_gm_match_submit / _wait: four batches of different sizes (one with
    listed- and slow-path rows, one empty) in flight at once on one context,
    waited for out of order; every result equals its own single emqx_gm_match
    and the oracle; the index may be released while calls are in flight (a call
    retains its snapshot).  GM_ASM_STREAM=1: every device-buffer call's scan
    and assembly on the assembly stream, overlapping the next call's walk."""
    if asm_stream:
        monkeypatch.setenv("GM_ASM_STREAM", asm_stream)
    from emqx_amd.engine import pack
    lv = ["a", "b", "c", "d", "e", "f"]
    heavy = set()
    for m in range(1 << 6):  # slow-path rows: every '+'/word mix over 6 levels
        ws = ["+" if (m >> i) & 1 else lv[i] for i in range(6)]
        heavy.add("/".join(ws))
        heavy.add("/".join(ws[:3]) + "/#")
    rng = random.Random(5)
    filters = sorted({f.encode() for f in heavy} | {_rand_filter(rng).encode() for _ in range(500)})
    batches = [[_rand_topic(rng).encode() for _ in range(n)] for n in (1, 5000, 70_000)]
    batches.append([b"a/b/c/d/e/f"] * 300 + [b"a/x/c/d/e/f"] * 300)
    batches.append([])
    idx = ctx.build_index(filters)
    bufs, pend = [], []
    for topics in batches:
        tb, to = pack(topics) if topics else (np.zeros(64, np.uint8), np.zeros(1, np.uint64))
        d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
        ctx.memcpy_h2d(d_tb, tb, len(tb))
        ctx.memcpy_h2d(d_to, to, len(to) * 8)
        bufs += [d_tb, d_to]
        pend.append(ctx.match_submit(idx, d_tb, d_to, len(topics)))
    want = [ctx.match(idx, t, exact=True) if t else (np.zeros(1, np.uint64), np.zeros(0, np.uint32)) for t in batches]
    idx.release()  # the calls in flight keep the snapshot
    for k in (3, 0, 4, 2, 1):  # out of submission order
        res = pend[k].wait()
        ro, ids = res.to_host()
        res.free()
        assert np.array_equal(ro, want[k][0]) and np.array_equal(ids, want[k][1]), k
        if batches[k]:
            oro, oids = _oracle_rows(orc, filters, batches[k], 1)
            assert np.array_equal(ro, oro) and np.array_equal(ids, oids), k
    for b in bufs:
        ctx.dev_free(b)


def test_fused_priority_knob_same_rows(ctx, orc, monkeypatch):
    """GM_FUSED_PRIO=0 (every phase at wave priority 0) and the default
    (staging + tokenizer at priority 1) give the same rows, which equal the oracle."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(6, 30_000, wildcard_only=True)
    fb, fo = render_codes(codes)
    filters = sorted(set(orc.unpack(fb, fo)))
    idx = ctx.build_index(filters)
    n = 100_000
    db, do, tot = ctx.gen_topics_device(codes, 6, 0, n)
    rows = []
    for prio in ("0", "1"):
        monkeypatch.setenv("GM_FUSED_PRIO", prio)
        res = ctx.match_device(idx, db, do, n, exact=True)
        rows.append(res.to_host())
        res.free()
    assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
    tb, to = orc.render_codes(orc.gen_topic_codes(6, 0, n, codes))
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    oro, oids, _ = r.match_batch((tb, to), filters, mode=1, nthreads=8)
    assert np.array_equal(rows[1][0], oro) and np.array_equal(rows[1][1], oids)
    ctx.dev_free(db)
    ctx.dev_free(do)
    idx.release()


def test_config_c1_fixture(ctx, orc):
    """The committed C1 fixture (tests/golden/config_c1.json: 2,000 topics over
    the 1M-topic stream, rows as filter strings) against the full C1 index."""
    import json
    import os
    from emqx_amd.engine import gen_filter_codes, render_codes
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_c1.json")) as f:
        fx = json.load(f)
    codes = gen_filter_codes(fx["seed"], fx["filters"], wildcard_only=fx["wildcard_only"])
    filters = sorted(set(orc.unpack(*render_codes(codes))))
    idx = ctx.build_index(filters)
    ro, ids = ctx.match(idx, [t.encode() for t in fx["topics"]], exact=True)
    got = [[filters[k].decode() for k in ids[ro[i]:ro[i + 1]]] for i in range(len(fx["topics"]))]
    assert got == fx["matches"]
    idx.release()


@pytest.mark.parametrize("n,listed_cap", [(100_000, None), (300_000, None), (300_000, "3")])
def test_speculative_ids_capacity_redo(ctx, orc, monkeypatch, n, listed_cap):
    """run_match writes the rows before the host reads the match total, into an
    ids buffer sized from the context's recent matches per topic.  A batch
    after a match-free one (capacity ~1 id per topic) with ~8 matches per topic
    overflows it and is assembled again; both calls equal the oracle, and so
    does a third call (capacity grown).  At 300k topics (4,688 tiles) the tile
    scan is left split and k_assemble_c adds the block offsets, on the first
    assembly and on the redo; with GM_LISTED_CAP=3 the 10-level topics past
    the listed pass's cap take the slow path, whose rescan is whole."""
    if listed_cap:
        monkeypatch.setenv("GM_LISTED_CAP", listed_cap)
    filters = sorted({b"a/#", b"a/+/#", b"+/b/#", b"a/b/#", b"+/+/#", b"a/+/c", b"+/b/c", b"a/b/c", b"#"})
    idx = ctx.build_index(filters)
    none = [b"$x/%d" % i for i in range(n)]   # '$' topics: no root '#' or '+', nothing else matches
    many = [b"a/b/c" if i % 3 else b"a/b/c/%d" % i for i in range(n)]
    if listed_cap:
        many[-10:] = [b"a/b/c/d/e/f/g/h/i/%d" % i for i in range(10)]
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    for topics in (none, many, many):
        ro, ids = ctx.match(idx, topics, exact=True)
        oro, oids, _ = r.match_batch(topics, filters, mode=1, nthreads=8)
        assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
    assert int(oro[-1]) > 7 * n
    idx.release()


@pytest.mark.parametrize("listed_cap", [None, "3"])
def test_compact_staging_vs_columns(ctx, orc, monkeypatch, listed_cap):
    """GM_STAGE_COMPACT: the fused main pass stages each tile's matches as one
    list (filter id | lane) and k_assemble_c sorts them into rows; the listed
    pass keeps its rows apart (past GM_LISTED_CAP of them: the slow path).
    Both layouts give the oracle's rows on: a C2-shaped sample; 10-level topics
    (listed-pass rows); and tiles of 32 topics with 16 matches beside 32 with
    33 (their list passes 64 x 16 entries: every topic of the tile is re-walked
    by the listed pass, the 33-match rows finish on the slow path)."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    import itertools
    if listed_cap:
        monkeypatch.setenv("GM_LISTED_CAP", listed_cap)
    codes = gen_filter_codes(8, 20_000, wildcard_only=True)
    filters = set(orc.unpack(*render_codes(codes)))
    deep = ["/".join(["d%d" % i] + ["x"] * 9) for i in range(3)]
    filters |= {d.encode() for d in deep} | {b"d0/+/x/#", b"d1/x/+/x/x/#"}
    a16 = ["m/a/b", "m/+/b", "m/a/+", "m/#", "m/+/+", "+/a/b", "+/+/b", "+/a/+", "#", "+/#", "m/a/#", "+/+/+",
           "m/a/b/#", "+/a/#", "m/+/b/#", "+/+/b/#"]
    b33 = ["n/%s/%s/%s" % c for c in itertools.product(["3", "+"], ["x", "+"], ["y", "+"])]
    b33 += [f + "/#" for f in b33] + ["+/%s/%s/%s" % c for c in itertools.product(["3", "+"], ["x", "+"], ["y", "+"])]
    b33 += ["n/#", "n/3/#", "n/+/#", "n/3/x/#", "n/+/x/#", "n/3/+/#", "n/+/+/#"]
    filters = sorted(filters | {f.encode() for f in a16 + b33})
    tb, to = orc.render_codes(orc.gen_topic_codes(8, 0, 40_000, codes))
    topics = orc.unpack(tb, to) + [d.encode() for d in deep] * 50
    topics += [b"z/z"] * (-len(topics) % 64)  # the next tiles start on a 64-topic boundary
    topics += [b"m/a/b", b"n/3/x/y"] * 32 + [b"m/a/b"] * 32 + [b"n/3/x/y"] * 32
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    assert len(r.match_routes(b"m/a/b")) == 16 and len(r.match_routes(b"n/3/x/y")) == 33
    oro, oids, _ = r.match_batch(topics, filters, mode=1, nthreads=8)
    idx = ctx.build_index(filters)
    # compact staging with the listed pass deferred to the read-back (default)
    # or launched with the main pass (GM_LISTED_DEFER=0), and the columns
    for mode, defer in (("1", "1"), ("1", "0"), ("0", "1")):
        monkeypatch.setenv("GM_STAGE_COMPACT", mode)
        monkeypatch.setenv("GM_LISTED_DEFER", defer)
        ro, ids = ctx.match(idx, topics, exact=True)
        assert np.array_equal(ro, oro) and np.array_equal(ids, oids), (mode, defer)
        # a batch with no listed rows right after one with them (the fast path again)
        ro2, ids2 = ctx.match(idx, topics[:40_000], exact=True)
        assert np.array_equal(ro2, oro[:40_001]) and np.array_equal(ids2, oids[:oro[40_000]]), (mode, defer)
    idx.release()


def test_untimed_submits_same_rows(ctx, orc):
    """EMQX_GM_NO_TIMING: calls without the main pass's timestamps return the
    same rows; their stats read 0 (not an older call's stamps); a timed call
    after them is timed again."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(3, 10_000)
    idx = ctx.build_index(render_codes(codes))
    n = 200_000
    db, do, _ = ctx.gen_topics_device(codes, 3, 0, n)
    ref = ctx.match_device(idx, db, do, n)
    assert ctx.stats()["match_kernel_ms"] > 0
    ro0, ids0 = ref.to_host()
    ref.free()
    pend = [ctx.match_submit(idx, db, do, n, timed=(k == 3)) for k in range(4)]
    for k, p in enumerate(pend):
        r = p.wait()
        st = ctx.stats()
        assert (st["match_kernel_ms"] > 0) == (k == 3), (k, st["match_kernel_ms"])
        ro, ids = r.to_host()
        assert np.array_equal(ro, ro0) and np.array_equal(ids, ids0)
        r.free()
    idx.release()


@pytest.mark.parametrize("asm_stream", [None, "1"])
def test_many_calls_in_flight_counter_ring(ctx, orc, monkeypatch, asm_stream):
    """More calls in flight than the context's ring of pre-zeroed pass-counter
    blocks (16): the calls past it take counters behind their own workspace;
    every call's rows equal a lone call's, also for a batch whose rows go
    through the listed pass (its counters are read after the ring moved on).
    GM_ASM_STREAM=1: the assemblies on their own stream (no ring block is then
    zeroed by an assembly), mixed with host-buffer calls on the context stream."""
    if asm_stream:
        monkeypatch.setenv("GM_ASM_STREAM", asm_stream)
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(4, 10_000)
    filters = sorted(set(orc.unpack(*render_codes(codes))) | {("/".join(["d"] + ["x"] * 9)).encode()})
    idx = ctx.build_index(filters)
    n = 50_000
    db, do, _ = ctx.gen_topics_device(codes, 4, 0, n)
    ref = ctx.match_device(idx, db, do, n)
    ro0, ids0 = ref.to_host()
    ref.free()
    pend = [ctx.match_submit(idx, db, do, n, timed=(k % 5 == 0)) for k in range(24)]
    for p in pend:
        r = p.wait()
        ro, ids = r.to_host()
        assert np.array_equal(ro, ro0) and np.array_equal(ids, ids0)
        r.free()
    # listed-pass rows (10-level topics) between fast-path calls
    deep = [("/".join(["d"] + ["x"] * 9)).encode()] * 300 + [b"z"] * 100
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    oro, oids, _ = r.match_batch(deep, filters, mode=1)
    for _ in range(3):
        g_ro, g_ids = ctx.match(idx, deep, exact=True)
        assert np.array_equal(g_ro, oro) and np.array_equal(g_ids, oids)
        rr = ctx.match_device(idx, db, do, n)
        ro, ids = rr.to_host()
        assert np.array_equal(ro, ro0) and np.array_equal(ids, ids0)
        rr.free()
    idx.release()


def test_host_csr_ownership_across_contexts(ctx, orc):
    """A result CSR records its context: freeing it through another context is
    refused (its buffers belong to the first context's pool), and host rows
    still held after emqx_gm_close stay readable (the pool detaches them)."""
    import ctypes as C
    from emqx_amd import Context
    from emqx_amd._lib import Csr, lib, WITH_EXACT, EINVAL
    from emqx_amd.engine import pack, _ptr
    filters = [b"a/+", b"a/#", b"b/c"]
    topics = [b"a/x", b"b/c", b"q"] * 100
    other = Context(0)
    try:
        idx = other.build_index(filters)
        tb, to = pack(topics)
        csr = Csr()
        assert lib().emqx_gm_match(other.h, idx.h, _ptr(tb), _ptr(to), len(topics), WITH_EXACT, C.byref(csr)) == 0
        assert lib().emqx_gm_csr_free(ctx.h, C.byref(csr)) == EINVAL  # not this context's CSR
        ro = np.ctypeslib.as_array(csr.row_off, shape=(len(topics) + 1,)).copy()
        idx.release()
    finally:
        other.close()
    # after close the rows are detached, not freed: still readable and unchanged
    ro2 = np.ctypeslib.as_array(csr.row_off, shape=(len(topics) + 1,)).copy()
    ids = np.ctypeslib.as_array(csr.ids, shape=(int(csr.nnz),)).copy()
    assert np.array_equal(ro, ro2)
    oro, oids = _oracle_rows(orc, sorted(filters), topics, 1)
    assert np.array_equal(ro2, oro) and np.array_equal(ids, oids)


def test_c_abi_smoke_program():
    """The C ABI from a plain C program (tests/c_abi_smoke.c, built by
    __graft_entry__.build()): emqx_router_SUITE's t_match_routes filters in both
    match modes, fan-out with a duplicate filter's lists concatenated, a
    snapshot replicated through an image, a corrupt image and bad arguments
    refused with error codes."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c_abi_smoke")
    if not os.path.exists(exe):  # (normally prebuilt by __graft_entry__.build())
        subprocess.run(["gcc", "-O2", "-std=c11", "-I", os.path.join(root, "include"), exe + ".c", "-L",
                        os.path.join(root, "emqx_amd"), "-l:libemqx_gpu_match.so",
                        "-Wl,-rpath," + os.path.join(root, "emqx_amd"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "C_ABI_SMOKE_OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("n", [1_000_000, 3_000_000])
def test_no_speculative_ids_split_scan(ctx, orc, monkeypatch, n):
    """with compact staging the tile scan of a 2..64-block call hands
    back block SUMS, which only the speculative assembly turns into the grand
    total.  When the speculative ids buffer cannot be allocated
    (GM_NO_SPEC_IDS=1 forces that), the scan must write its offsets and total
    itself: the rows equal the default path's and the oracle's."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(9, 50_000, wildcard_only=True)
    fpack = render_codes(codes)
    idx = ctx.build_index(fpack)
    db, do, _ = ctx.gen_topics_device(codes, 9, 0, n)
    ref = ctx.match_device(idx, db, do, n, exact=True)
    ro0, ids0 = ref.to_host()
    ref.free()
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    res = ctx.match_device(idx, db, do, n, exact=True)
    ro, ids = res.to_host()
    res.free()
    assert np.array_equal(ro, ro0) and np.array_equal(ids, ids0)
    filters = sorted(set(orc.unpack(*fpack)))
    tb, to = orc.render_codes(orc.gen_topic_codes(9, 0, 20_000, codes))
    oro, oids = _oracle_rows(orc, filters, orc.unpack(tb, to), 1)
    assert np.array_equal(ro[:20_001], oro) and np.array_equal(ids[:int(oro[-1])], oids)
    ctx.dev_free(db)
    ctx.dev_free(do)
    idx.release()
