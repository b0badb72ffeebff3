"""emqx_gm_index_update on a prefix-sharded index (gm_shard.cpp update_sharded):
every shard patched in place, given a new id map only (k_gmap_shift), or
rebuilt alone.  The expected rows are always those of the same update on the
unsharded single-device index, plus the CPU oracle on a sample of the topics
and a fresh sharded build of the updated set."""

import bisect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE_TOPICS = [b"$SYS/broker", b"", b"/", b"a/+", b"solo/word", b"solo/x/y", b"nosuch/1", b"+/x", b"l0w1"]


@pytest.fixture(scope="module")
def ctx1():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base(orc):
    """About 30k filters: generated ones, a HOT first word (split by its second
    word at 2 and 3 shards) and the forms that live on every shard; 100k
    generated topics, topics under the hot word and the literal edge topics."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(5, 15_000)
    gen = sorted(set(orc.unpack(*render_codes(codes))))
    hot = [b"hot/%d/x%d" % (i % 40, i) for i in range(14_000)]
    extra = [b"hot", b"hot/#", b"hot/+/y", b"#", b"+/x", b"$SYS/#", b"/a", b"solo"]
    filters = sorted(set(gen) | set(hot) | set(extra))
    topics = orc.unpack(*orc.render_codes(orc.gen_topic_codes(5, 0, 100_000, codes)))
    topics += [b"hot/%d/x%d" % (i % 40, i) for i in range(0, 14_000, 7)]
    topics += [b"hot", b"hot/3", b"hot/3/q", b"hot/nv3/x", b"hot/nv3/y", b"zz4/a", b"q", b"q/r/s", b"p/new", b"!a", b"a/b/b"]
    topics += EDGE_TOPICS
    return {"gen": gen, "filters": filters, "topics": topics}


def _oracle_rows(orc, filters, topics):
    r = orc.Router(True)
    for f in filters:
        r.add_route(f)
    ro, ids, _ = r.match_batch(topics, filters, mode=1, nthreads=8)
    return ro, ids


def _eq(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


def _apply(filters, ops):
    s = set(filters)
    for f, ins in ops:
        (s.add if ins else s.discard)(f)
    return sorted(s)


def _check(c, ix, ctx1, e1, topics, orc, filters, what, both_modes=True, oracle=True):
    """ix (sharded, context c) against e1 (unsharded, ctx1), the oracle and the set itself."""
    got = c.match(ix, topics, exact=True)
    _eq(got, ctx1.match(e1, topics, exact=True), what + ": match_routes rows")
    if both_modes:
        _eq(c.match(ix, topics, exact=False), ctx1.match(e1, topics, exact=False), what + ": trie rows")
    if oracle:
        oro, oids = _oracle_rows(orc, filters, topics[::97])
        sub = [got[1][got[0][i]:got[0][i + 1]].tolist() for i in range(0, len(topics), 97)]
        assert sub == [oids[oro[j]:oro[j + 1]].tolist() for j in range(len(oro) - 1)], what + ": oracle"
    assert ix.n_filters == len(filters) == e1.n_filters, what
    assert ix.info.n_wildcard == e1.info.n_wildcard and bool(ix.info.trie_empty) == bool(e1.info.trie_empty), what
    return got


def _ids_around(ix, filters, changed):
    """filter(id) of every changed filter's place in the set and its neighbours."""
    for f in changed:
        p = bisect.bisect_left(filters, f)
        for i in range(max(0, p - 1), min(len(filters), p + 2)):
            assert ix.filter(i) == filters[i], (f, i)


def _mixed_ops(base):
    gen = base["gen"]
    w0 = next(f for f in gen if b"/" in f and not f.startswith((b"+", b"#"))).split(b"/")[0]
    ops = [(w0 + b"/newA%d/b" % i, True) for i in range(60)]       # under a known first word
    ops += [(b"zz%d/a" % i, True) for i in range(40)]               # new first words
    ops += [(b"hot/nv%d/x" % i, True) for i in range(40)]           # new second words under the split word
    ops += [(b"hot/+/q", True), (b"+/new", True), (b"q/#", True)]   # ... and filters for every shard
    plain = [f for f in gen if not f.startswith((b"+", b"#"))]
    ops += [(f, False) for f in plain[5:5 + 40]]                    # deletes, one of each kind
    ops += [(b"hot/3/x3", False), (b"#", False), (b"hot", False), (b"hot/+/y", False), (b"+/x", False),
            (b"$SYS/#", False)]
    ops += [(b"absent/x", False), (b"solo", True), (b"tmp/x", True), (b"tmp/x", False),  # no-ops, cancelling ops
            (plain[100], False), (plain[100], True)]
    ops += [(b"zz%d/b/+" % i, True) for i in range(200 - len(ops))]
    assert len(ops) == 200
    return ops


def _mixed_case(c, ctx1, orc, base):
    filters, topics = base["filters"], base["topics"]
    n_dev = len(c.devices)
    i1 = ctx1.build_index(filters)
    ix = c.build_index_sharded(filters)
    old = _check(c, ix, ctx1, i1, topics, orc, filters, "built")
    ops = _mixed_ops(base)
    new = _apply(filters, ops)
    e1 = ctx1.update_index(i1, ops)
    ix2 = c.update_index(ix, ops)
    st = c.last_update_stats()
    assert st["kind"] == "patch" and st["replica_mode"] == "sharded" and st["replicas"] == n_dev - 1, st
    kinds = c.last_shard_update()
    assert len(kinds) == n_dev and set(kinds) <= {"patch"}, kinds  # (filters for every shard: each one patched)
    got = _check(c, ix2, ctx1, e1, topics, orc, new, "200 mixed ops")
    fresh = c.build_index_sharded(new)
    _eq(got, c.match(fresh, topics, exact=True), "fresh sharded build of the new set")
    _eq(c.match(ix2, topics, exact=False), c.match(fresh, topics, exact=False), "fresh sharded build, trie rows")
    fresh.release()
    _ids_around(ix2, new, [f for f, _ in ops])
    assert ix2.subscriber_count(0) == 0
    dro, dids = c.fanout(ix2, *got)  # no subscriber lists: no deliveries, no error
    assert len(dro) == len(topics) + 1 and not dro.any() and len(dids) == 0
    _eq(c.match(ix, topics, exact=True), old, "the previous snapshot still serves its readers")
    # a chain of updates on the result
    ops2 = [(b"zz1/a", False), (b"chain/+/x", True), (b"hot/nv3/y", True), (b"#", True)]
    ops3 = [(b"chain/+/x", False), (b"hot/5/x5", False), (b"hot/nv3/x", False), (b"+/+/+", True)]
    e2, ix3 = ctx1.update_index(e1, ops2), c.update_index(ix2, ops2)
    new2 = _apply(new, ops2)
    _check(c, ix3, ctx1, e2, topics, orc, new2, "chain 1")
    e3, ix4 = ctx1.update_index(e2, ops3), c.update_index(ix3, ops3)
    new3 = _apply(new2, ops3)
    _check(c, ix4, ctx1, e3, topics, orc, new3, "chain 2")
    _ids_around(ix4, new3, [f for f, _ in ops2 + ops3])
    _eq(c.match(ix2, topics, exact=True), got, "an older snapshot of the chain")
    for x in (ix4, ix3, ix2, ix, e3, e2, e1, i1):
        x.release()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_mixed_ops_patch_every_shard(ctx1, orc, base, devices):
    from emqx_amd import Context
    with Context(devices=devices) as c:
        _mixed_case(c, ctx1, orc, base)


@pytest.mark.skipif("not __import__('torch').cuda.device_count() >= 2", reason="needs two GPUs")
def test_mixed_ops_two_gpus(ctx1, orc, base):
    from emqx_amd import Context
    with Context(devices=[0, 1]) as c:
        _mixed_case(c, ctx1, orc, base)


def _word_on_shard(base, n_shards, probe):
    """A plain (unsplit) first word of the generated filters whose partition is
    the shard `probe` (a filter with a new first word) is routed to."""
    from emqx_amd.engine import ALL_SHARDS, pack, prefix_plan
    filters = base["filters"]
    sh, route = prefix_plan(*pack(filters), n_shards)
    s = int(route.filter_shards(*pack([probe]))[0])
    assert s != ALL_SHARDS
    w = None
    for f, x in zip(filters, sh):
        if int(x) == s and b"/" in f and not f.startswith((b"hot", b"$", b"/")):
            w = f.split(b"/")[0]
            break
    assert w is not None
    on = [f for f in filters if f.startswith(w + b"/")]
    route.release()
    return w, s, on


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_shift_only_shards_share_their_tables(ctx1, orc, base, devices):
    """Ops confined to one shard: that shard is patched, every other one keeps
    its tables and gets a new id map -- and b'!a' sorts before every filter,
    so every global id in every row moves."""
    from emqx_amd import Context
    filters, topics = base["filters"], base["topics"]
    K = len(devices)
    w, _, on = _word_on_shard(base, K, b"!a")
    ops = [(b"!a", True), (w + b"/s1/x", True), (w + b"/s2", True), (on[0], False)]
    new = _apply(filters, ops)
    i1 = ctx1.build_index(filters)
    e1 = ctx1.update_index(i1, ops)
    with Context(devices=devices) as c:
        ix = c.build_index_sharded(filters)
        old = c.match(ix, topics, exact=True)
        ix2 = c.update_index(ix, ops)
        assert sorted(c.last_shard_update()) == ["patch"] + ["shift"] * (K - 1)
        assert c.last_update_stats()["kind"] == "patch"
        got = _check(c, ix2, ctx1, e1, topics, orc, new, "shift only")
        # id 0 is b"!a" now (only its own literal topic matches it): every other id moved up
        assert new[0] == b"!a" and int((got[1] == 0).sum()) == topics.count(b"!a") == 1
        # rows of topics under other first words hold no changed filter: old ids through the global shift
        dels = np.array(sorted(filters.index(f) for f, ins in ops if not ins), np.int64)
        adds = np.array(sorted(bisect.bisect_left(filters, f) for f, ins in ops if ins), np.int64)
        keep = np.array([not t.startswith((w + b"/", b"!a")) and t != w for t in topics])
        lens_old, lens_new = np.diff(old[0].astype(np.int64)), np.diff(got[0].astype(np.int64))
        assert np.array_equal(lens_old[keep], lens_new[keep])
        o_ids = old[1][np.repeat(keep, lens_old)].astype(np.int64)
        n_ids = got[1][np.repeat(keep, lens_new)].astype(np.int64)
        shifted = o_ids - np.searchsorted(dels, o_ids, side="left") + np.searchsorted(adds, o_ids, side="right")
        assert np.array_equal(shifted, n_ids) and (n_ids > o_ids).all()
        # no table was copied for the shift-only shards (and the patched shard's new tables have the old size):
        # the snapshot grew by its id maps alone, 4 B per local filter
        grew = int(ix2.info.device_bytes) - int(ix.info.device_bytes)
        assert 0 < grew <= 4 * K * (len(new) + 1), grew
        ix2.release()
        ix.release()
    e1.release()
    i1.release()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_fallbacks_rebuild_one_shard(ctx1, orc, base, devices):
    """What cannot be patched in place recompiles ONE shard; the others still
    get their new id maps only."""
    from emqx_amd import Context
    filters, topics = base["filters"], base["topics"]
    K = len(devices)
    w, _, _ = _word_on_shard(base, K, b"!a")
    i1 = ctx1.build_index(filters)

    def run(c, ix, b1, bf, ops, what):
        new = _apply(bf, ops)
        e1 = ctx1.update_index(b1, ops)
        ix2 = c.update_index(ix, ops)
        assert sorted(c.last_shard_update()) == ["rebuild"] + ["shift"] * (K - 1), (what, c.last_shard_update())
        st = c.last_update_stats()
        assert st["kind"] == "rebuild" and st["replica_mode"] == "sharded", (what, st)
        _check(c, ix2, ctx1, e1, topics, orc, new, what, both_modes=False)
        e1.release()
        ix2.release()

    with Context(devices=devices) as c:
        ix = c.build_index_sharded(filters)
        # a no-change batch: the same snapshot
        same = c.update_index(ix, [(b"absent/x", False), (b"solo", True), (b"t/x", True), (b"t/x", False)])
        st = c.last_update_stats()
        assert same.h.value == ix.h.value and st["kind"] == "none" and st["replica_mode"] == "sharded", st
        same.release()
        # a snapshot that is no longer the newest of its line: its mirrors have moved on
        ops_n = [(w + b"/n1", True)]
        newer = c.update_index(ix, ops_n)
        assert sorted(c.last_shard_update()) == ["patch"] + ["shift"] * (K - 1)
        run(c, ix, i1, filters, [(w + b"/n2", True), (w + b"/n3/+", True)], "superseded snapshot")
        # (the newest one from here on)
        f_n, e_n = _apply(filters, ops_n), ctx1.update_index(i1, ops_n)
        # a '#' before the last word: not patched in place
        run(c, newer, e_n, f_n, [(b"a/#/b", True)], "'#' inside")
        # a 5,000-op batch onto one shard: past max(4096, n_local / 8)
        run(c, newer, e_n, f_n, [(w + b"/big%d" % i, True) for i in range(5000)], "large batch")
        e_n.release()
        newer.release()
        ix.release()
    i1.release()


def _small_sets():
    """(name, filters): shards of 0, 1, 255, 256 and 257 filters at 3 shards --
    one first word whose filters share their second word is ONE partition, so
    two shards hold nothing but the filters that live on every shard."""
    out = []
    for n in (1, 255, 256, 257):
        one = [b"w/a/x%03d" % i for i in range(n)]
        out.append(("n%d_no_all" % n, one))
        out.append(("n%d_all" % n, one + [b"#", b"+/a/+", b"w/+"]))
    return out


@pytest.mark.parametrize("name,filters", _small_sets(), ids=[n for n, _ in _small_sets()])
def test_smallest_shapes(ctx1, name, filters):
    """The id-map kernel and the plan at their edges: empty shards, one filter,
    a map of exactly one workgroup and one element more; only deletes, only
    inserts, every filter of a shard deleted, inserts at the first and the
    last global rank, a delta across a 256-element boundary of a shard's map."""
    from emqx_amd import Context
    filters = sorted(filters)
    n = sum(f.startswith(b"w/a/") for f in filters)
    steps = [
        ("only deletes", [(f, False) for f in {filters[0], filters[-1], b"w/a/x%03d" % (n // 2)}]),
        ("only inserts", [(b"!a", True), (b"~z", True), (b"w/a/x1005", True), (b"w/b/y", True)]),
        ("across a workgroup boundary", [(b"w/a/x%03d" % i, False) for i in (253, 254, 255, 256)] +
         [(b"w/a/x2535", True), (b"w/a/x2545", True), (b"w/a/x2555", True), (b"w/a/x2565", True), (b"w/a/x2575", True)]),
        ("a shard emptied", [(b"w/a/x%03d" % i, False) for i in range(n)] +
         [(b"w/a/x%04d" % i, False) for i in (1005, 2535, 2545, 2555, 2565, 2575)]),
        ("filled again", [(b"w/a/x%03d" % i, True) for i in range(0, n, 2)] + [(b"#", True), (b"!a", False)]),
    ]
    with Context(devices=[0, 0, 0]) as c:
        ix = c.build_index_sharded(filters)
        cur = filters
        for what, ops in steps:
            cur = _apply(cur, ops)
            nxt = c.update_index(ix, ops)
            kinds = c.last_shard_update()
            assert len(kinds) == 3 and c.last_update_stats()["replica_mode"] == "sharded"
            if all(not ins for _, ins in ops):  # deletes need no room: never a rebuild
                assert set(kinds) <= {"patch", "shift"}, (name, what, kinds)
            topics = cur + [b"w/a/zz", b"w/a", b"w", b"!a", b"~z", b"x/y", b"w/b/y", b"", b"w/a/x000"]
            got, got_t = c.match(nxt, topics, exact=True), c.match(nxt, topics, exact=False)
            if cur:
                e = ctx1.build_index(cur)
                _eq(got, ctx1.match(e, topics, exact=True), (name, what))
                _eq(got_t, ctx1.match(e, topics, exact=False), (name, what, "trie"))
                assert nxt.info.n_wildcard == e.info.n_wildcard, (name, what)
                e.release()
            else:  # every filter gone
                assert not got[0].any() and not got_t[0].any() and nxt.info.n_wildcard == 0, (name, what)
            assert nxt.n_filters == len(cur) and nxt.filters() == cur, (name, what)
            ix.release()
            ix = nxt
        ix.release()


def test_refusals_kept(ctx1, base):
    from emqx_amd import Context, GpuMatchError
    from emqx_amd._lib import EUNSUPPORTED
    filters = base["filters"][:2000] + [b"#", b"+/x"]
    filters = sorted(set(filters))
    with Context(devices=[0, 0]) as c:
        with_subs = c.build_index_sharded(filters, subs=[[i] for i in range(len(filters))])
        plain = c.build_index_sharded(filters)
        for bad in (lambda: c.update_index(with_subs, [(b"q/+", True)]),
                    lambda: c.update_subs(with_subs, [(b"q/+", 7, True)]),
                    lambda: c.update_subs(plain, [(b"q/+", 7, True)]),
                    lambda: with_subs.export(), lambda: plain.export()):
            with pytest.raises(GpuMatchError) as ei:
                bad()
            assert ei.value.code == EUNSUPPORTED
        with_subs.release()
        plain.release()
    shard = ctx1.build_index_shard(filters[:100], np.arange(100, dtype=np.uint32) * 3)
    with pytest.raises(GpuMatchError):
        ctx1.update_index(shard, [(b"q/+", True)])
    shard.release()
