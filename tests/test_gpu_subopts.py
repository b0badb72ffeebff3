"""Subscription options at dispatch on the device (emqx_gm_subopts_*,
emqx_gm_deliver, emqx_amd/csrc/gm_subopts.hip) against the host walk over a
host-only twin of the same table, the device table's own host copy, and the
restatement of ignore_local/4 + enrich_subopts/3 (tests/_subopts_ref.py) --
array for array, in FLAG and DROP mode, on host rows and on device rows the
test made itself.  The shapes are the smallest that cross every boundary of
k_so_copy: a workgroup owns 1,024 output elements at these sizes and a thread
moves 4."""

import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import _subopts_ref as R

pytestmark = pytest.mark.gpu

PER_BLOCK = 1024  # fan_per_block() for every total up to 2M deliveries (1,024 * 2,048)
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2047, 2049]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


class RawRows:
    """A device CSR made by the test (not a match result) with the messages' bytes and publishers beside it."""

    def __init__(self, ctx, row_off, ids, flags, froms, nnz=None):
        from emqx_amd import _lib
        from emqx_amd.engine import DeviceCsr
        arrs = [np.ascontiguousarray(row_off, np.uint64), np.ascontiguousarray(ids, np.uint32),
                np.ascontiguousarray(flags, np.uint8), np.ascontiguousarray(froms, np.uint32)]
        self.ctx, self.ptrs = ctx, []
        for a in arrs:
            p = ctx.dev_alloc(max(a.nbytes, 16))
            if a.nbytes:
                ctx.memcpy_h2d(p, a, a.nbytes)
            self.ptrs.append(p)
        m = _lib.Csr()
        m.n_rows, m.nnz, m.on_device = len(arrs[0]) - 1, len(arrs[1]) if nnz is None else nnz, 1
        m.row_off = C.cast(C.c_void_p(self.ptrs[0]), C.POINTER(C.c_uint64))
        m.ids = C.cast(C.c_void_p(self.ptrs[1]), C.POINTER(C.c_uint32))
        self.m, self.csr = m, DeviceCsr(ctx, m)
        self.d_flags, self.d_from = self.ptrs[2], self.ptrs[3]

    def free(self):
        self.m.row_off = self.m.ids = None  # (the buffers are this test's, not a result's)
        for p in self.ptrs:
            self.ctx.dev_free(p)


def _lists(d, drop):
    return (d.row_off.tolist(), d.ids.tolist(), d.dopt.tolist(),
            d.row_dropped.tolist() if drop else [0] * (len(d.row_off) - 1))


def _from_word(f):
    return 0xFFFFFFFF if f is None else f


class Tri:
    """One option set three ways: the device table, a host-only twin, the restatement."""

    def __init__(self, ctx, world, index=None):
        from emqx_amd import SubOptTable
        self.ctx, self.w = ctx, world
        self.index = index or ctx.build_index(world.filters, subs=world.lists)
        self.dev = ctx.build_subopts(self.index, world.entries(), world.default_byte())
        self.twin = SubOptTable.compile_host(world.filters, world.lists, world.entries(), world.default_byte())
        a, b = self.dev.info(), self.twin.info()
        assert (a.n_entries, a.n_defaulted, a.n_nl, a.n_skipped_unknown) == \
            (b.n_entries, b.n_defaulted, b.n_nl, b.n_skipped_unknown)
        assert a.device_bytes > 0 and b.device_bytes == 0

    def check(self, rows, msgs, want=None):
        """Device (host rows, raw device rows) == host walk (twin, own copy) == restatement, both modes."""
        csr = R.csr_of(rows)
        flags, froms = [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]
        want = want or self.w.walk_both(rows, msgs)
        raw = RawRows(self.ctx, csr[0], csr[1], flags, [_from_word(f) for f in froms])
        out = []
        for drop in (False, True):
            ref = tuple(want[1 if drop else 0])
            got = self.dev.deliver(csr, flags, froms, drop, index=self.index)
            assert _lists(got, drop) == ref, "host rows, drop=%s" % drop
            assert got.n_dropped == sum(ref[3])
            assert _lists(self.twin.deliver_host(csr, flags, froms, drop), drop) == ref
            assert _lists(self.dev.deliver_host(csr, flags, froms, drop), drop) == ref
            dd = self.dev.deliver_device(raw.csr, raw.d_flags, raw.d_from, drop, index=self.index)
            back = dd.to_host()
            dd.free()
            assert _lists(back, drop) == ref, "device rows, drop=%s" % drop
            assert back.n_dropped == sum(ref[3])
            out.append(got)
        raw.free()
        return out

    def release(self):
        self.dev.release()
        self.twin.release()
        self.index.release()


def _msg(frm, k=0):
    return {"qos": k % 3, "retain": bool(k & 1), "retained": bool(k & 4) and not k & 2, "from": frm}


# ------------------------------------------------------------------ segment lengths x hit positions
@pytest.fixture(scope="module")
def lengths_world(ctx):
    """One filter per length; every pair has nl = 1 (so the publisher's position IS the hit), options vary by position."""
    filters = [b"len/%04d" % n for n in LENGTHS]
    lists = [[1000 * (i + 1) + 7 * k for k in range(n)][::-1] for i, n in enumerate(LENGTHS)]  # descending ids: the
    # segment order is not the nl list's order
    opts = {(i, s): R.subscribe_opts({"qos": (s + k) % 3, "nl": 1, "rap": k & 1})
            for i, lst in enumerate(lists) for k, s in enumerate(lst)}
    upgrade = {s: (s % 5 == 0) for lst in lists for s in lst}
    t = Tri(ctx, R.World(filters, lists, opts, upgrade))
    yield t
    t.release()


@pytest.mark.parametrize("kind", ["first", "last", "group3", "group4", "block", "none"])
def test_segment_lengths_and_hit_positions(lengths_world, kind):
    """Every length in one 64-row window (rows of one or two segments, so 4-element groups straddle segment and
    workgroup boundaries); the No-Local hit first, last, either side of a 4-group boundary, and on the output
    element that starts a workgroup's range."""
    t, w = lengths_world, lengths_world.w
    rows, msgs, start = [], [], 0
    nl = len(LENGTHS)
    for r in range(64):
        row = [r % nl] if r % 3 else [r % nl, (r * 5 + 1) % nl]
        # the publisher: a subscriber of the row's last non-empty segment, at the position `kind` names
        frm = None
        seg0 = start
        for fid in row:
            lst = w.lists[w.by_id[fid]]
            if lst and kind != "none":
                pos = {"first": 0, "last": len(lst) - 1, "group3": min(3, len(lst) - 1), "group4": min(4, len(lst) - 1),
                       "block": min((-seg0) % PER_BLOCK, len(lst) - 1)}[kind]
                frm = lst[pos]
            seg0 += len(lst)
        start = seg0
        rows.append(row)
        msgs.append(_msg(frm, r))
    flag, drop = t.check(rows, msgs)
    assert len(flag.ids) > 30 * PER_BLOCK
    hits = int(sum(1 for b in flag.dopt if b & 16))
    assert hits == drop.n_dropped and (hits > 40) == (kind != "none")


def test_block_boundary_hits_exact(lengths_world):
    """Rows in a fixed order, so the hit of each row IS the output element that begins a workgroup's range in
    FLAG mode (and the element before / after it in the neighbouring rows)."""
    t, w = lengths_world, lengths_world.w
    big = [LENGTHS.index(n) for n in (1023, 1025, 2047, 2049, 1024)]
    rows, msgs, start = [], [], 0
    for r in range(64):
        fid = big[r % len(big)]
        lst = w.lists[w.by_id[fid]]
        pos = (-start) % PER_BLOCK + (r % 3 - 1)  # the boundary element, the one before, the one after
        pos = min(max(pos, 0), len(lst) - 1)
        rows.append([fid])
        msgs.append(_msg(lst[pos], r))
        start += len(lst)
    flag, drop = t.check(rows, msgs)
    where = np.flatnonzero(flag.dopt & 16)
    assert len(where) == 64 and drop.n_dropped == 64
    at = [int(x) % PER_BLOCK for x in where]  # (a boundary at a segment's own start has no element before it)
    assert at.count(0) == 34 and at.count(1) == 21 and at.count(PER_BLOCK - 1) == 9


# ------------------------------------------------------------------ emptied segments
def test_emptied_segment_and_a_row_all_dropped(ctx):
    filters = [b"solo/a", b"solo/b", b"pair", b"none"]
    lists = [[5], [6], [5, 9], []]
    opts = {(0, 5): R.subscribe_opts({"nl": 1, "qos": 2}), (1, 6): R.subscribe_opts({"nl": 1}),
            (2, 5): R.subscribe_opts({"nl": 1, "rap": 1}), (2, 9): R.subscribe_opts({"qos": 1})}
    t = Tri(ctx, R.World(filters, lists, opts))
    fid = {f: t.w.id_of[i] for i, f in enumerate(filters)}
    rows = [[fid[b"solo/a"]],                       # its one delivery is the publisher's: the row empties
            [fid[b"solo/a"], fid[b"pair"]],         # two segments lose their hit, one empties
            [fid[b"pair"], fid[b"solo/a"], fid[b"none"], fid[b"solo/b"]],
            [fid[b"solo/b"]], [fid[b"solo/a"]], [fid[b"none"]]]
    msgs = [_msg(5, 1), _msg(5, 2), _msg(5, 3), _msg(6, 4), _msg(6, 5), _msg(5, 6)]
    flag, drop = t.check(rows, msgs)
    assert drop.row_off.tolist() == [0, 0, 1, 3, 3, 4, 4] and drop.ids.tolist() == [9, 9, 6, 5]
    assert drop.row_dropped.tolist() == [1, 2, 2, 1, 0, 0] and drop.n_dropped == 6
    assert flag.ids.tolist() == [5, 5, 5, 9, 5, 9, 5, 6, 6, 5]
    # a window all of whose deliveries are dropped
    flag, drop = t.check([[fid[b"solo/a"]], [fid[b"solo/b"]]], [_msg(5), _msg(6)])
    assert len(drop.ids) == 0 and drop.row_off.tolist() == [0, 0, 0] and drop.n_dropped == 2
    t.release()


# ------------------------------------------------------------------ one hot row
@pytest.fixture(scope="module")
def hot_world(ctx):
    n = 300_002  # 293 workgroups: 292 of 1,024 and a tail of 994; the last pair is a defaulted one
    rnd = np.random.RandomState(3)
    subs = (rnd.permutation(n).astype(np.int64) * 3 + 11).tolist()
    opts = {(0, s): R.subscribe_opts({"qos": s % 3, "nl": 1 if s % 2 else 0, "rap": (s >> 1) & 1}) for s in subs[::2]}
    upgrade = {s: s % 7 == 0 for s in subs[::2]}
    # (every other pair is defaulted: default nl = 1, so every position can be a hit)
    t = Tri(ctx, R.World([b"hot/#", b"cold"], [subs, [1]], opts, upgrade, default=R.subscribe_opts({"nl": 1, "qos": 1})))
    yield t
    t.release()


def _nl_pos(w, lo, hi):
    lst = w.lists[0]
    return next(k for k in range(lo, hi) if w.opts.get((0, lst[k]), w.default)["nl"] == 1)


@pytest.mark.parametrize("where", ["first", "middle", "last", "none"])
def test_one_hot_row_across_many_workgroups(hot_world, where):
    t, w = hot_world, hot_world.w
    lst = w.lists[0]
    pos = {"first": _nl_pos(w, 0, 1024), "middle": _nl_pos(w, 150 * PER_BLOCK + 1021, 151 * PER_BLOCK),
           "last": len(lst) - 1, "none": None}[where]
    if where == "last":
        assert w.opts.get((0, lst[pos]), w.default)["nl"] == 1
    frm = lst[pos] if pos is not None else 2  # (2 is no subscriber)
    hot = w.id_of[0]
    flag, drop = t.check([[hot]], [_msg(frm, 5)])
    assert len(flag.ids) == len(lst) and drop.n_dropped == (0 if where == "none" else 1)
    if pos is not None:
        assert np.flatnonzero(flag.dopt & 16).tolist() == [pos]


def test_hot_rows_past_two_million_deliveries_wider_workgroup_ranges(hot_world):
    """Eight hot rows, 2.4M deliveries: a workgroup owns 2,048 output elements, not 1,024.  Device (host rows and
    raw device rows) against the host walk, whose equality with the restatement the tests above establish."""
    t, w = hot_world, hot_world.w
    lst, hot, cold = w.lists[0], w.id_of[0], w.id_of[1]
    pos = [_nl_pos(w, 0, 8), _nl_pos(w, 2047, 2060), _nl_pos(w, 2048 * 70 - 3, 2048 * 70), len(lst) - 1]
    rows = [[hot], [cold, hot], [hot], [hot, cold], [hot], [], [hot], [hot], [hot]]
    froms = [lst[pos[0]], lst[pos[1]], None, lst[pos[2]], lst[pos[3]], 5, 2, lst[pos[1]], lst[pos[0]]]
    csr, flags = R.csr_of(rows), [R.msg_byte(_msg(None, k)) for k in range(len(rows))]
    raw = RawRows(t.ctx, csr[0], csr[1], flags, [_from_word(f) for f in froms])
    for drop in (False, True):
        want = t.twin.deliver_host(csr, flags, froms, drop)
        assert len(want.ids) > 2_400_000 - 8 and want.n_dropped == (6 if drop else 0)
        got = t.dev.deliver(csr, flags, froms, drop, index=t.index)
        dd = t.dev.deliver_device(raw.csr, raw.d_flags, raw.d_from, drop, index=t.index)
        back = dd.to_host()
        dd.free()
        for x in (got, back):
            assert np.array_equal(x.row_off, want.row_off) and np.array_equal(x.ids, want.ids)
            assert np.array_equal(x.dopt, want.dopt) and x.n_dropped == want.n_dropped
            assert not drop or np.array_equal(x.row_dropped, want.row_dropped)
    raw.free()


# ------------------------------------------------------------------ the nl lists
@pytest.mark.parametrize("n_nl", [0, 1, 2, 63, 64, 65])
def test_nl_list_lengths_and_the_search(ctx, n_nl):
    n = 70
    subs = [100 + 10 * k for k in range(n)]
    rnd = random.Random(n_nl)
    order = subs[:]
    rnd.shuffle(order)  # list order is not id order
    with_nl = sorted(rnd.sample(subs, n_nl))
    opts = {(0, s): R.subscribe_opts({"nl": 1 if s in with_nl else 0, "qos": s // 10 % 3}) for s in subs}
    # the same subscribers under a second filter with nl flipped for a few: nl on one of the two only
    opts.update({(1, s): R.subscribe_opts({"nl": 0 if s in with_nl else 1, "qos": 2}) for s in subs[:8]})
    t = Tri(ctx, R.World([b"nl/a", b"nl/b", b"nl/c"], [order, subs[:8], []], opts))
    a, b = t.w.id_of[0], t.w.id_of[1]
    froms = [None, 0, 99, 100, 105, 100 + 10 * (n - 1), 100 + 10 * n, 0xFFFFFFFE]     # below, between, above, ends
    froms += with_nl[:3] + with_nl[-3:] + [s + 5 for s in with_nl[:3]]                # equal to entries, between them
    froms += [s for s in subs if s not in with_nl][:3]                                # present in the filter, nl = 0
    rows = [[a] if k % 2 else [a, b] for k in range(len(froms))] + [[b, a]] * 8
    froms += subs[:8]  # one subscriber under both matched filters
    msgs = [_msg(f, k) for k, f in enumerate(froms)]
    flag, drop = t.check(rows, msgs)
    assert t.dev.info().n_nl == n_nl + sum(1 for s in subs[:8] if s not in with_nl)
    t.release()


# ------------------------------------------------------------------ empty inputs
def test_empty_rows_empty_window_and_no_publisher(lengths_world):
    t = lengths_world
    five, one = LENGTHS.index(5), LENGTHS.index(1)
    rows = [[], [], [five], [], [one, five], [], []]
    lst = t.w.lists[t.w.by_id[five]]
    flag, drop = t.check(rows, [_msg(lst[2], k) for k in range(7)])
    assert drop.row_dropped.tolist() == [0, 0, 1, 0, 1, 0, 0]
    flag, drop = t.check(rows, [_msg(None, k) for k in range(7)])       # from = NONE everywhere
    assert drop.n_dropped == 0 and not (flag.dopt & 16).any() and np.array_equal(flag.ids, drop.ids)
    flag, drop = t.check([], [])                                         # an empty window
    assert flag.row_off.tolist() == [0] and len(flag.ids) == 0
    flag, drop = t.check([[], [], []], [_msg(lst[0], k) for k in range(3)])  # rows, no match at all
    assert flag.row_off.tolist() == [0, 0, 0, 0] and drop.row_dropped.tolist() == [0, 0, 0]


def test_unvalidated_device_rows_are_skipped_and_clamped(lengths_world):
    """Device rows the host never saw: an id past the snapshot is an empty segment, the last offset past the ids
    is clamped, and the high bits of msg_flags are masked."""
    t, w = lengths_world, lengths_world.w
    nf = len(LENGTHS)
    five, big = LENGTHS.index(5), LENGTHS.index(1025)
    rows = [[five, nf + 3, big], [0xFFFFFFFF], [big, five]]
    clean = [[five, big], [], [big, five]]
    frm = [w.lists[w.by_id[big]][700], None, w.lists[w.by_id[five]][4]]
    msgs = [_msg(f, k + 1) for k, f in enumerate(frm)]
    want = w.walk_both(clean, msgs)
    ro, ids = R.csr_of(rows)
    for drop in (False, True):
        ref = want[1 if drop else 0]
        raw = RawRows(t.ctx, ro[:-1] + [ro[-1] + 9], ids, [R.msg_byte(m) | 0xF0 for m in msgs],
                      [_from_word(f) for f in frm], nnz=len(ids))
        dd = t.dev.deliver_device(raw.csr, raw.d_flags, raw.d_from, drop)
        back = dd.to_host()
        dd.free()
        raw.free()
        assert (back.ids.tolist(), back.dopt.tolist()) == (ref[1], ref[2])
        assert back.row_off.tolist() == ref[0]
        if drop:
            assert back.row_dropped.tolist() == ref[3]


# ------------------------------------------------------------------ FLAG deliveries == the fan-out, C2 fixture
@pytest.fixture(scope="module")
def c2(ctx):
    """C2's filter set (1M wildcard filters of the bench generator) with 0-3 subscribers per filter; options
    for the pairs of every third filter, the rest defaulted."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(1, 1_000_000, wildcard_only=True)
    fb, fo = render_codes(codes)
    n = len(fo) - 1
    cnt = (np.arange(n) * 2654435761 >> 7) % 4
    so = np.zeros(n + 1, np.uint64)
    np.cumsum(cnt, out=so[1:])
    si = (np.arange(int(so[-1]), dtype=np.uint64) * 48271 % 200_000).astype(np.uint32)
    # (a filter given twice may then list one subscriber twice: nl stays 0 here, the table's rule)
    index = ctx.build_index((fb, fo), subs=(so, si))
    pick = np.flatnonzero((np.arange(n) % 3 == 0) & (cnt > 0))[:50_000]
    entries = []
    for i in pick.tolist():
        f = bytes(fb[int(fo[i]):int(fo[i + 1])])
        for s in set(si[int(so[i]):int(so[i + 1])].tolist()):
            entries.append((f, s, (s % 3) | (0x08 if s & 8 else 0) | (0x10 if s & 16 else 0)))
    table = ctx.build_subopts(index, entries, default=1)
    yield ctx, index, table, codes
    table.release()
    index.release()


@pytest.mark.parametrize("n_topics", [1024, 16384])
def test_flag_deliveries_equal_the_fanout_on_c2(c2, n_topics):
    ctx, index, table, codes = c2
    d_b, d_o, _ = ctx.gen_topics_device(codes, 2, 0, n_topics)
    m = ctx.match_device(index, d_b, d_o, n_topics)
    ro, ids = m.to_host()
    ctx.dev_free(d_b)
    ctx.dev_free(d_o)
    fro, fids = ctx.fanout(index, ro, ids)
    flags = (np.arange(n_topics) % 12).astype(np.uint8)
    flags[flags % 4 == 3] = 0
    froms = fids[np.minimum(fro[:-1], max(len(fids) - 1, 0)).astype(np.int64)] if len(fids) else np.zeros(n_topics, np.uint32)
    got = table.deliver((ro, ids), flags, froms, index=index)
    assert got.row_off.tobytes() == fro.tobytes() and got.ids.tobytes() == fids.tobytes() and len(fids) > n_topics
    host = table.deliver_host((ro, ids), flags, froms)
    assert got.dopt.tobytes() == host.dopt.tobytes()
    assert not (got.dopt & 16).any()  # (no pair has nl here)
    # the same rows as the match left them in HBM
    d_f, d_fr = ctx.dev_alloc(n_topics), ctx.dev_alloc(n_topics * 4)
    ctx.memcpy_h2d(d_f, flags, n_topics)
    ctx.memcpy_h2d(d_fr, np.ascontiguousarray(froms, np.uint32), n_topics * 4)
    dd = table.deliver_device(m, d_f, d_fr, index=index)
    back = dd.to_host()
    dd.free()
    m.free()
    ctx.dev_free(d_f)
    ctx.dev_free(d_fr)
    assert back.ids.tobytes() == fids.tobytes() and back.dopt.tobytes() == host.dopt.tobytes()
    assert back.row_off.tobytes() == fro.tobytes()


# ------------------------------------------------------------------ table lifetime
def test_table_keeps_its_snapshot_and_refuses_another(ctx):
    from emqx_amd import GpuMatchError, _lib
    w = R.random_world(6, n_filters=30, n_subs=40, max_list=9)
    index = ctx.build_index(w.filters, subs=w.lists)
    other = ctx.build_index(w.filters, subs=w.lists)
    table = ctx.build_subopts(index, w.entries(), w.default_byte())
    rows, msgs = R.random_window(w, 12, n_rows=64)
    csr, flags, froms = R.csr_of(rows), [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]
    want = w.walk_both(rows, msgs)
    assert _lists(ctx.deliver(index, table, csr, flags, froms), False) == tuple(want[0])
    with pytest.raises(GpuMatchError) as e:
        ctx.deliver(other, table, csr, flags, froms)  # rows of another snapshot
    assert e.value.code == _lib.EINVAL
    assert _lib.lib().emqx_gm_subopts_index(table.h) == index.h.value
    index.release()  # the caller lets go: the table holds the snapshot
    other.release()
    assert _lists(table.deliver(csr, flags, froms, drop=True), True) == tuple(want[1])
    table.release()


def _refused(ctx, index, code, entries=(), word="", **kw):
    """The build fails with `code`, names `word`, and hands back no table."""
    from emqx_amd import _lib
    from emqx_amd.subopts import _entry_args
    fb, fo, es, eo, ne = _entry_args(list(entries))
    h = C.c_void_p(0xDEAD)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _lib.lib().emqx_gm_subopts_build(ctx.h, index.h, p(fb), p(fo), p(es), p(eo), ne, kw.get("default", 0),
                                          kw.get("flags", 0), C.byref(h))
    msg = (_lib.lib().emqx_gm_last_error(ctx.h) or b"").decode(errors="replace")
    assert rc == code and not h.value and word in msg, (rc, h.value, msg)


def test_build_refusals_on_the_device_entry_point(ctx):
    """Every refusal of emqx_gm_subopts_build: an index without subscriber lists, a shard index, a sharded
    index, an overlay snapshot (EUNSUPPORTED); unknown pairs, bad bytes, a pair twice (EINVAL); a subscriber
    listed twice under nl (EUNSUPPORTED).  No table comes back."""
    from emqx_amd import Context, _lib
    filters, lists = [b"a/#", b"b/+", b"c"], [[1, 2], [3], [4]]
    bare = ctx.build_index(filters)  # no subscriber lists
    _refused(ctx, bare, _lib.EUNSUPPORTED, word="without subscriber lists")
    # an overlay snapshot: an update that inserts a filter with '#' inside stays an overlay (no subscriber lists either)
    ov = ctx.update_index(bare, [(b"x/#/y", True)])
    _refused(ctx, ov, _lib.EUNSUPPORTED, word="overlay")
    ov.release()
    bare.release()
    shard = ctx.build_index_shard(filters, np.array([0, 1, 2], np.uint32))
    _refused(ctx, shard, _lib.EUNSUPPORTED, word="a shard index")
    shard.release()
    with Context(devices=[0, 0]) as c2:
        sharded = c2.build_index_sharded(filters, subs=lists)
        _refused(c2, sharded, _lib.EUNSUPPORTED, word="a sharded index")
        sharded.release()
    index = ctx.build_index(filters, subs=lists)
    _refused(ctx, index, _lib.EINVAL, [(b"not/there", 1, 0)])
    _refused(ctx, index, _lib.EINVAL, [(b"b/+", 1, 0)])            # the pair is not in the filter's list
    _refused(ctx, index, _lib.EINVAL, [(b"a/#", 1, 3)])            # QoS 3
    _refused(ctx, index, _lib.EINVAL, [(b"a/#", 1, 0x20)])         # a high bit
    _refused(ctx, index, _lib.EINVAL, [(b"a/#", 1, 1), (b"a/#", 1, 2)])
    _refused(ctx, index, _lib.EINVAL, default=3)
    _refused(ctx, index, _lib.EINVAL, flags=0x2)
    t = ctx.build_subopts(index, [(b"not/there", 1, 0), (b"b/+", 1, 0), (b"a/#", 2, 5)], skip_unknown=True)
    i = t.info()
    assert (i.n_entries, i.n_skipped_unknown, i.n_nl, i.n_defaulted) == (1, 2, 1, 3)
    # refused calls: an id >= n_filters, descending offsets, a bad message byte, an unknown mode, n_rows of 2^32 - 1
    from emqx_amd import GpuMatchError
    for rows, flags in ((([0, 1], [3]), [0]), (([0, 2, 1], [0, 0]), [0, 0]), (([0, 1], [0]), [3]), (([0, 1], [0]), [0x10])):
        with pytest.raises(GpuMatchError) as e:
            t.deliver(rows, flags, [1] * len(flags))
        assert e.value.code == _lib.EINVAL
    from emqx_amd._lib import Csr, Deliveries
    ro, ids, mf, fr = np.array([0, 1], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.ones(1, np.uint32)
    m = Csr()
    m.nnz, m.row_off, m.ids = 1, ro.ctypes.data_as(C.POINTER(C.c_uint64)), ids.ctypes.data_as(C.POINTER(C.c_uint32))
    for n_rows, mode in ((0xFFFFFFFF, 0), (1, 2)):
        m.n_rows = n_rows
        d = Deliveries()
        C.memset(C.byref(d), 0xAB, C.sizeof(d))
        before = bytes(d)
        assert _lib.lib().emqx_gm_deliver(ctx.h, t.h, C.byref(m), C.c_void_p(mf.ctypes.data),
                                          C.c_void_p(fr.ctypes.data), mode, C.byref(d)) == _lib.EINVAL
        assert bytes(d) == before  # no output touched
    t.release()
    index.release()
    dup = ctx.build_index([b"a/#", b"b/+", b"a/#"], subs=[[1, 2], [3], [2, 4]])  # a/# lists 2 twice
    _refused(ctx, dup, _lib.EUNSUPPORTED, [(b"a/#", 2, 0x04)])
    _refused(ctx, dup, _lib.EUNSUPPORTED, default=0x04)
    ok = ctx.build_subopts(dup, [(b"a/#", 2, 0x01), (b"a/#", 1, 0x04)])  # the duplicate without nl is fine
    ok.release()
    dup.release()


def test_two_listed_devices_table_on_the_first():
    from emqx_amd import Context
    w = R.random_world(7, n_filters=30, n_subs=40, max_list=9)
    rows, msgs = R.random_window(w, 13, n_rows=64)
    want = w.walk_both(rows, msgs)
    with Context(devices=[0, 0]) as c2:
        t = Tri(c2, w)
        assert t.dev.info().device_bytes > 0
        t.check(rows, msgs, want)
        t.release()


# ------------------------------------------------------------------ GpuRoutes + PublishBatcher
def test_gpu_routes_and_batcher_hand_out_the_bytes(ctx):
    """GpuRoutes.subscribe(.., opts) rebuilds the table beside the snapshot; PublishBatcher(subopts=True) hands
    deliver() the byte with the subscriber; without subopts the same routes deliver as before."""
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    routes = GpuRoutes(ctx)
    routes.subscribe(b"t/+", "a", {"qos": 1, "nl": 1})
    routes.subscribe(b"t/+", "b", {"qos": 2, "rap": 1, "upgrade_qos": True})
    routes.subscribe(b"t/1", "c")
    routes.subscribe(b"t/1", "a", {"qos": 0})
    items = [(b"t/1", {"qos": 1, "retain": True, "from": "a", "k": 0}), (b"t/2", {"qos": 2, "from": "c", "k": 1}),
             (b"zz", {"k": 2})]
    want = {False: [("a", b"t/+", 0, 1 | 8 | 16), ("b", b"t/+", 0, 2 | 4), ("c", b"t/1", 0, 0), ("a", b"t/1", 0, 0),
                    ("a", b"t/+", 1, 1 | 8), ("b", b"t/+", 1, 2)]}
    want[True] = [x for x in want[False] if not x[3] & 16]
    for drop in (False, True):
        got = []
        b = PublishBatcher(routes=routes, timer=False, subopts=True, drop_no_local=drop,
                           deliver=lambda sub, f, m, byte: got.append((sub, f, m["k"], byte)) or True)
        res = b.publish_batch(items)
        assert sorted(got) == sorted(want[drop]), drop
        assert res[2] == [] and b.metrics["messages.dropped.no_subscribers"] == 1
        assert b.metrics["delivery.dropped.no_local"] == (1 if drop else 0)
    assert routes.subopts_builds == 1  # one snapshot, one table
    routes.subscribe(b"t/2", "c", {"qos": 1})  # a new snapshot: the table is rebuilt beside it
    got = []
    PublishBatcher(routes=routes, timer=False, subopts=True,
                   deliver=lambda sub, f, m, byte: got.append((sub, f, byte)) or True).publish_batch(items[1:2])
    assert sorted(got) == [("a", b"t/+", 9), ("b", b"t/+", 2), ("c", b"t/2", 1)] and routes.subopts_builds == 2
    plain = []
    PublishBatcher(routes=routes, timer=False,
                   deliver=lambda sub, f, m: plain.append((sub, f, m["k"])) or True).publish_batch(items)
    assert sorted(plain) == sorted([(s, f, k) for s, f, k, _ in want[False]] + [("c", b"t/2", 1)])
