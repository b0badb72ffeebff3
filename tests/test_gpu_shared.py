"""The shared-subscription pick on the device (emqx_gm_shared_*,
emqx_amd/csrc/gm_shared.hip) against the restatement of emqx_shared_sub:pick/6
applied hit by hit (tests/_shared_ref.py) and the host walk over a host-only
twin of the same table.  All comparisons are exact.  The round-robin batch is
laid out so that 64-hit steps hold one slot only, 64 distinct slots and two
alternating slots, and is run at forced chunk counts 1, 2, 3, 7 and the
library's own."""

import numpy as np
import pytest

from tests import _shared_ref as R

pytestmark = pytest.mark.gpu

STRATEGIES = ["hash", "round_robin", "sticky", "random"]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


class World:
    """One slot set three ways: the device table, a host-only twin, the restatement."""

    def __init__(self, ctx, index, filters, slots, prev=None):
        from emqx_amd import SharedTable
        self.ctx, self.index, self.filters = ctx, index, filters
        self.dev = ctx.build_shared(index, slots, prev.dev if prev else None)
        self.twin = SharedTable.compile_host(filters, slots, prev.twin if prev else None)
        self.ref = R.Table(filters, slots, prev.ref if prev else None)
        assert self.dev.slots() == self.twin.slots() == self.ref.slot_list()
        assert self.dev.info().device_bytes > 0

    def pick(self, rows, strategy, hashes=None, seed=0, n_chunks=None):
        """Device == host walk == restatement; returns (row_off, members, slots)."""
        csr = R.csr_of(rows)
        hs = hashes if strategy == "hash" else None
        got = tuple([int(x) for x in a] for a in self.dev.pick(csr, strategy, hs, seed, n_chunks))
        host = tuple([int(x) for x in a] for a in self.twin.pick_host(csr, strategy, hs, seed))
        want = tuple(self.ref.pick(rows, strategy, hashes, seed))
        assert got[0] == want[0] and got[2] == want[2]
        assert got[1] == want[1]
        assert host == want
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


def _pick_device_rows(ctx, table, res, strategy, hashes, seed):
    d_h = None
    if strategy == "hash":
        hs = np.ascontiguousarray(hashes, np.uint32)
        d_h = ctx.dev_alloc(hs.nbytes)
        ctx.memcpy_h2d(d_h, hs, hs.nbytes)
    om, os_ = table.pick_device(res, strategy, d_h, seed)
    ro, mem = om.to_host()
    ro2, slots = os_.to_host()
    om.free()
    os_.free()
    if d_h:
        ctx.dev_free(d_h)
    assert np.array_equal(ro, ro2)
    return [int(x) for x in ro], [int(x) for x in mem], [int(x) for x in slots]


# ------------------------------------------------------------------ hash
def test_hash_over_matched_rows_host_and_device(ctx):
    counts = [1, 2, 3, 64, 65, 2, 3, 1, 5, 2, 3, 4]
    filters = [b"h/%02d/#" % k for k in range(12)]
    slots = [(filters[k], 0, list(range(100 * k, 100 * k + counts[k]))) for k in range(12)]
    slots.append((filters[4], 1, [900, 901, 902]))  # one filter carries two groups
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, slots)
    topics = [b"h/%02d/x" % (i % 12) for i in range(30)] + [b"nothing/here", b"h/+/x", b"h/04", b"h/03/a/b"]
    ro, ids = ctx.match(index, topics)
    rows = R.rows_of(ro, ids)
    assert rows[30] == [] and rows[31] == [] and rows[32] == [4]  # no hit; a wildcard publish topic; 'h/04/#' ~ 'h/04'
    res = _device_rows(ctx, index, topics)
    assert R.rows_of(*res.to_host()) == rows
    for h in (0, 1, 2, 3, 4, 5, 63, 64, 65, 2**27 - 1, 2**32 - 1):  # 0, Count - 1 and Count of every slot, large
        hs = [h] * len(topics)
        got = w.pick(rows, "hash", hs)
        assert tuple(_pick_device_rows(ctx, w.dev, res, "hash", hs, 0)) == got  # device rows, the same result
        # slot order within a row: filter 4's two groups ascending
        k = got[0][4]
        assert got[2][k:got[0][5]] == [4, 5]
    hs = [(i * 2654435761) & R.M32 for i in range(len(topics))]
    got = w.pick(rows, "hash", hs)
    assert tuple(_pick_device_rows(ctx, w.dev, res, "hash", hs, 0)) == got
    res.free()
    w.release()
    index.release()


# ------------------------------------------------------------------ round-robin ordinals
def _rr_batch():
    d = [b"r/d/%02d" % k for k in range(64)]
    filters = d + [b"r/h64", b"r/h65", b"r/t", b"r/z"]  # already in byte order: id = position
    D, H64, H65, T, A = list(range(64)), 64, 65, 66, 67
    slots = [(d[k], 0, list(range(10 * k, 10 * k + [1, 2, 3][k % 3]))) for k in range(64)]
    slots += [(b"r/h64", 0, list(range(1000, 1064))), (b"r/h65", 2, [1100, 1101, 1102]),
              (b"r/t", 0, [1200, 1201]), (b"r/t", 1, [1300]), (b"r/z", 0, [1400, 1401, 1402, 1403, 1404])]
    rows = [[A] for _ in range(64)]            # hits 0..63: one slot only
    rows.append(D + [A])                       # hits 64..127: 64 distinct slots, each hit exactly once
    rows += [[H64, A] for _ in range(64)]      # hits 129..256: two alternating slots; h64 hit 64 times
    rows += [[H65, T, A] for _ in range(65)]   # a filter with two groups; h65 hit 65 times
    rows += [[A] for _ in range(6)]
    assert len(rows) == 200
    return filters, slots, rows


def test_round_robin_ordinals_at_every_chunk_count(ctx):
    filters, slots, rows = _rr_batch()
    index = ctx.build_index(filters)
    assert index.filters() == filters
    outs = []
    for n_chunks in (1, 2, 3, 7, None):
        w = World(ctx, index, filters, slots)
        outs.append(w.pick(rows, "round_robin", seed=31, n_chunks=n_chunks))
        # a second call continues every slot where the first ended, at another chunk count
        outs.append(w.pick(rows[::-1], "round_robin", seed=99, n_chunks=None if n_chunks == 3 else 3))
        w.release()
    assert all(o == outs[0] for o in outs[0::2]) and all(o == outs[1] for o in outs[1::2])
    ro, mem, sl = outs[0]
    steps = [sl[k:k + 64] for k in range(0, len(sl) - 63, 64)]
    assert len(set(steps[0])) == 1 and len(set(steps[1])) == 64          # one slot only; 64 distinct
    assert len(set(steps[3])) == 2 and steps[3][0::2] == [steps[3][0]] * 32  # two alternating
    assert sl.count(64) == 64 and sl.count(65) == 65 and sl.count(0) == 1 and sl.count(68) == 200
    # the slot hit by every row: first + k rem 5 over all 200 hits
    a = [m for m, s in zip(mem, sl) if s == 68]
    first = R.mix(31, 68) % 5
    assert a == [1400 + (first + k) % 5 for k in range(200)]
    index.release()


# ------------------------------------------------------------------ state
def test_round_robin_state_across_calls_and_rebuilds(ctx):
    f1 = [b"m/+", b"n/#", b"z"]
    s1 = [(b"m/+", 0, [1, 2, 3, 4, 5]), (b"n/#", 3, [7, 8, 9]), (b"z", 1, [20, 21])]
    i1 = ctx.build_index(f1)
    w = World(ctx, i1, f1, s1)
    rows = [[0, 1, 2], [0], [0, 1], [0]]
    got = w.pick(rows, "round_robin", seed=11)
    assert got[1][0] == 1 + R.mix(11, 0) % 5  # the unset start comes from the seed
    for seed in (12, 13):  # three consecutive calls continue the sequence (the seed no longer matters)
        nxt = w.pick(rows, "round_robin", seed=seed)
        assert nxt[1][0] == 1 + (got[1][0] - 1 + 4) % 5
        got = nxt
    while w.ref.pd[("rr", (0, b"m/+"))] != 4:
        w.pick([[0]], "round_robin", seed=0)
    # members removed so that rr >= Count, a member added to n/#, z dropped, ids shifted by new filters
    f2 = [b"a/0", b"a/1"] + f1
    s2 = [(b"m/+", 0, [1, 2]), (b"n/#", 3, [7, 8, 9, 10])]
    i2 = ctx.build_index(f2)
    w2 = World(ctx, i2, f2, s2, prev=w)
    got = w2.pick([[2, 3], [2], [3, 2]], "round_robin", seed=14)
    assert got[1][0] == 2  # (4 + 1) rem 2 with the current Count
    # prev itself is not modified
    assert w.pick([[0]], "round_robin", seed=0)[1] == [1]
    s3 = s2 + [(b"z", 1, [20, 21])]  # z re-added: unset again
    w3 = World(ctx, i2, f2, s3, prev=w2)
    got = w3.pick([[4], [4], [2, 3, 4]], "round_robin", seed=15)
    assert got[1][0] == [20, 21][R.mix(15, 2) % 2]
    for x in (w, w2, w3):
        x.release()
    i1.release()
    i2.release()


def test_sticky_is_stable_and_dropped_when_its_member_leaves(ctx):
    f = [b"s/#", b"t/+"]
    s1 = [(b"s/#", 0, [5, 6, 7]), (b"t/+", 0, [9]), (b"t/+", 4, [30, 31, 32, 33])]
    index = ctx.build_index(f)
    w = World(ctx, index, f, s1)
    rows = [[0, 1], [0], [1, 0]] * 30  # many hits of one unset slot in one call: one value for all
    got = w.pick(rows, "sticky", seed=21)
    assert set(m for m, s in zip(got[1], got[2]) if s == 0) == {[5, 6, 7][R.mix(21, 0) % 3]}
    assert w.pick(rows, "sticky", seed=22)[1] == got[1]  # stable across calls and seeds
    stuck = got[1][0]
    rest = [m for m in (5, 6, 7) if m != stuck]
    w2 = World(ctx, index, f, [(b"s/#", 0, rest), (b"t/+", 0, [9, 10]), (b"t/+", 4, [30, 31, 32, 33])], prev=w)
    got2 = w2.pick(rows, "sticky", seed=23)
    assert got2[1][0] == rest[R.mix(23, 0) % 2]  # its member left: a new pick from the seed
    assert got2[1][1] == 9                        # stored while it was the only member, kept
    assert got2[1][2] == got[1][2]                # still listed: kept
    w.release()
    w2.release()
    index.release()


# ------------------------------------------------------------------ random
def test_random_in_range_reproducible_and_equal_to_the_restatement(ctx):
    filters, slots, rows, _ = R.random_case(8)
    index = ctx.build_index(filters)
    w = World(ctx, index, filters, slots)
    a = w.pick(rows, "random", seed=5)
    assert w.pick(rows, "random", seed=5) == a  # equal arguments, equal picks
    assert w.pick(rows, "random", seed=6)[1] != a[1]
    table = w.ref.slot_list()
    assert len(a[1]) > 300 and all(m in table[s][2] for m, s in zip(a[1], a[2]))
    w.release()
    index.release()


# ------------------------------------------------------------------ larger
def test_larger_generated_set_all_strategies(ctx):
    from emqx_amd import gen_filter_codes, render_codes
    import random
    codes = gen_filter_codes(7, 2000)
    fb, fo = render_codes(codes)
    filters = [bytes(fb[int(fo[i]):int(fo[i + 1])]) for i in range(2000)]
    index = ctx.build_index((fb, fo))
    names = sorted(set(filters))
    n = 20_000
    d_b, d_o, _ = ctx.gen_topics_device(codes, 7, 0, n)
    res = ctx.match_device(index, d_b, d_o, n)
    rows = R.rows_of(*res.to_host())
    # 300 slots over the filters the topics hit most, so the picks are many
    hit = {}
    for r in rows:
        for f in r:
            hit[f] = hit.get(f, 0) + 1
    top = sorted(hit, key=lambda f: (-hit[f], f))[:220]
    rng = random.Random(3)
    slots, seen = [], set()
    while len(seen) < 300:
        f, g = rng.choice(top), rng.randrange(3)
        if (f, g) in seen:
            continue
        seen.add((f, g))
        c = rng.choice([1, 2, 3, 7, 64, 65, 200])
        slots.append((names[f], g, [rng.randrange(100_000) for _ in range(c)]))
    w = World(ctx, index, filters, slots)
    assert w.dev.info().n_slots == 300
    hashes = [(i * 2654435761 + 7) & R.M32 for i in range(n)]
    for strategy in STRATEGIES:
        for seed in (41, 42):
            got = w.pick(rows, strategy, hashes, seed)
            assert len(got[1]) > 1000
    # device rows: the same picks, results left on the device (state continues from the calls above)
    for strategy in STRATEGIES:
        want = tuple(w.ref.pick(rows, strategy, hashes, 43))
        assert tuple(_pick_device_rows(ctx, w.dev, res, strategy, hashes, 43)) == want
    res.free()
    ctx.dev_free(d_b)
    ctx.dev_free(d_o)
    w.release()
    index.release()


# ------------------------------------------------------------------ batcher
def _publish_world(ctx, use_shared):
    from emqx_amd import SharedSub
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    routes = GpuRoutes(ctx, node=b"n1")
    local = [_Box([]) for _ in range(3)]
    for k, box in enumerate(local):
        routes.subscribe(b"loc/%d/#" % k, box)
    groups = {b"job/+/run": [(b"g0", 3), (b"g1", 2)], b"job/#": [(b"g0", 4)], b"loc/1/#": [(b"g1", 1)]}
    sh = SharedSub(ctx, seed=1234)
    boxes = {}
    for f, gs in groups.items():
        for g, cnt in gs:
            routes.route_add(f, (g, b"n1"))
            for m in range(cnt):
                box = boxes.setdefault((g, f, m), [])
                sh.subscribe(g, f, _Box(box))
    lookup = lambda f: [(g, b"n1") for g, _ in groups.get(f, [])]  # noqa: E731
    items = [(b"job/%d/run" % (i % 5), "m%d" % i) for i in range(40)] + [(b"loc/1/x", "l1"), (b"none", "x"),
                                                                        (b"job/9", "j9"), (b"loc/1/y", "l2")]
    if use_shared:
        pb = PublishBatcher(routes=routes, timer=False, node=b"n1", lookup_routes=lookup, shared=sh,
                            shared_strategy="round_robin")
    else:
        ref_state = {}

        def shared_dispatch(group, f, msg):
            # the restatement, hit by hit in the order publish/1 reaches the groups
            if "t" not in ref_state:
                names = routes.index.filters()
                slots = [(ff, sh.group_id[g], [sh.sub_id[s] for s in sh.subscribers(g, ff)]) for (g, ff) in
                         sorted(sh._members)]
                ref_state["t"] = R.Table(names, slots)
                ref_state["names"] = names
            t = ref_state["t"]
            s = [k for k, (fid, g, _) in enumerate(t.slots) if t.names[fid] == f and g == sh.group_id[group]][0]
            m = t.pick_one("round_robin", s, 0, 0, (1234 + 0x9E3779B9) & R.M32)
            sh.subs[m].append((f, msg))
            return ("ok", 1)
        pb = PublishBatcher(routes=routes, timer=False, node=b"n1", lookup_routes=lookup,
                            shared_dispatch=shared_dispatch)
    out = pb.publish_batch(items)
    sh.release()
    return out, [b.box for b in local], [boxes[k] for k in sorted(boxes)]


class _Box:
    """A subscriber with an inbox; hashable by identity."""

    def __init__(self, box):
        self.box = box

    def append(self, x):
        self.box.append(x)


def test_batcher_with_shared_equals_per_message_dispatch(ctx):
    a = _publish_world(ctx, True)
    b = _publish_world(ctx, False)
    assert a[0] == b[0]
    assert a[1] == b[1] and a[2] == b[2]
    assert sum(len(x) for x in a[2]) == 40 * 3 + 2 + 1  # every message reached one member per group


# ------------------------------------------------------------------ multi-device context
def test_multi_device_context_serves_from_the_first_device():
    from emqx_amd import Context, SharedTable
    c = Context(devices=[0, 0])
    try:
        filters, slots, rows, _ = R.random_case(12, n_rows=100)
        index = c.build_index(filters)
        t = c.build_shared(index, slots)
        ref = R.Table(filters, slots)
        twin = SharedTable.compile_host(filters, slots)
        for strategy in STRATEGIES:
            hs = list(range(len(rows)))
            got = tuple([int(x) for x in a] for a in
                        t.pick(R.csr_of(rows), strategy, hs if strategy == "hash" else None, 3))
            assert got == tuple(ref.pick(rows, strategy, hs, 3))
            assert got == tuple([int(x) for x in a] for a in
                                twin.pick_host(R.csr_of(rows), strategy, hs if strategy == "hash" else None, 3))
        t.release()
        twin.release()
        index.release()
    finally:
        c.close()


# ------------------------------------------------------------------ refusals and device-row guards
def test_refusals_and_ids_past_the_snapshot_in_device_rows(ctx):
    import ctypes as C
    from emqx_amd import Context, GpuMatchError, _lib
    from emqx_amd.engine import DeviceCsr
    filters = [b"a/#", b"b/+", b"c"]
    slots = [(b"a/#", 0, [1, 2, 3]), (b"c", 0, [7, 8])]
    index = ctx.build_index(filters)
    with pytest.raises(GpuMatchError) as e:
        ctx.build_shared(index, slots + [(b"not/there", 0, [1])])
    assert e.value.code == _lib.EINVAL and "not/there" in str(e.value)
    shard = ctx.build_index_shard(filters, np.array([0, 1, 2], np.uint32))
    with pytest.raises(GpuMatchError) as e:
        ctx.build_shared(shard, slots)
    assert e.value.code == _lib.EUNSUPPORTED
    shard.release()
    with Context(devices=[0, 0]) as c2:
        sharded = c2.build_index_sharded(filters)
        with pytest.raises(GpuMatchError) as e:
            c2.build_shared(sharded, slots)
        assert e.value.code == _lib.EUNSUPPORTED
        sharded.release()
    t = ctx.build_shared(index, slots)
    for rows, strategy in ((([0, 1], [3]), "random"), (([0, 2, 1, 2], [0, 0]), "random"), (([0, 1], [0]), "hash")):
        with pytest.raises(GpuMatchError) as e:  # an id >= n_filters; descending offsets; HASH without msg_hash
            t.pick(rows, strategy)
        assert e.value.code == _lib.EINVAL
    # device rows are not validated on the host: the kernels skip ids past the snapshot
    ro = np.array([0, 3, 3, 5], np.uint64)
    ids = np.array([0, 3, 0xFFFFFFFF, 2, 0], np.uint32)
    d_ro, d_ids = ctx.dev_alloc(ro.nbytes), ctx.dev_alloc(ids.nbytes)
    ctx.memcpy_h2d(d_ro, ro, ro.nbytes)
    ctx.memcpy_h2d(d_ids, ids, ids.nbytes)
    m = _lib.Csr()
    m.n_rows, m.nnz, m.on_device = 3, 5, 1
    m.row_off = C.cast(C.c_void_p(d_ro), C.POINTER(C.c_uint64))
    m.ids = C.cast(C.c_void_p(d_ids), C.POINTER(C.c_uint32))
    res = DeviceCsr(ctx, m)
    got = _pick_device_rows(ctx, t, res, "round_robin", None, 4)
    want = R.Table(filters, slots).pick([[0], [], [2, 0]], "round_robin", None, 4)
    assert tuple(got) == tuple(want) and got[0] == [0, 1, 1, 3]
    m.row_off = m.ids = None  # (the buffers are this test's, not a result's)
    ctx.dev_free(d_ro)
    ctx.dev_free(d_ids)
    t.release()
    index.release()
