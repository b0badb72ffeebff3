"""The subscription-option table on the host alone: the compiler
(emqx_amd/csrc/gm_subopts.cpp) and the host walk (emqx_gm_deliver_host) against
the restatement of ignore_local/4, get_subopts/2 and enrich_subopts/3
(tests/_subopts_ref.py), Broker.subscribe's option merge, and
PublishBatcher(subopts=True) over a stand-in for GpuRoutes.  No device is
needed.  All comparisons are exact."""

import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

from tests import _subopts_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(world, skip_unknown=False, entries=None):
    from emqx_amd import SubOptTable
    return SubOptTable.compile_host(world.filters, world.lists, world.entries() if entries is None else entries,
                                    world.default_byte(), skip_unknown)


def _froms(msgs):
    return [m["from"] for m in msgs]


def _deliver(t, rows, msgs, drop):
    d = t.deliver_host(R.csr_of(rows), [R.msg_byte(m) for m in msgs], _froms(msgs), drop)
    return (d.row_off.tolist(), d.ids.tolist(), d.dopt.tolist(),
            d.row_dropped.tolist() if drop else [0] * len(rows)), d


def _exhaustive_world():
    # one subscriber per (SubQoS, upgrade_qos, rap, nl): 24 of them under one filter
    combos = list(itertools.product(range(3), (False, True), (0, 1), (0, 1)))
    lst = list(range(10, 10 + len(combos)))
    opts = {(0, s): R.subscribe_opts({"qos": q, "rap": rap, "nl": nl}) for s, (q, _, rap, nl) in zip(lst, combos)}
    upgrade = {s: u for s, (_, u, _, _) in zip(lst, combos)}
    return R.World([b"x/+"], [lst], opts, upgrade), lst


@pytest.mark.parametrize("drop", [False, True])
def test_every_option_combination_against_the_restatement(drop):
    """3 x 3 QoS pairs x upgrade_qos x rap x retain x retained-header x nl x (from =
    the subscriber / another / none): every combination, in FLAG and in DROP mode."""
    w, lst = _exhaustive_world()
    msgs = [{"qos": pq, "retain": rt, "retained": hd, "from": frm}
            for pq in range(3) for rt in (False, True) for hd in (False, True) for frm in lst + [99, None]]
    rows = [[0]] * len(msgs)
    t = _table(w)
    got, d = _deliver(t, rows, msgs, drop)
    want = w.walk(rows, msgs, drop)
    assert got == tuple(want)
    hits = sum(1 for m in msgs if m["from"] in lst and w.opts[(0, m["from"])]["nl"] == 1)
    assert hits == 12 * 12  # every nl subscriber publishing every message kind
    if drop:
        assert d.n_dropped == hits and not any(b & 16 for b in got[2])
    else:
        assert sum(1 for b in got[2] if b & 16) == hits and d.n_dropped == 0
    t.release()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_windows_flag_drop_and_the_plain_fanout(seed):
    w = R.random_world(seed)
    rows, msgs = R.random_window(w, seed + 100)
    t = _table(w)
    flag, _ = _deliver(t, rows, msgs, False)
    drop, dd = _deliver(t, rows, msgs, True)
    assert flag == tuple(w.walk(rows, msgs, False))
    assert drop == tuple(w.walk(rows, msgs, True))
    # FLAG deliveries are the plain fan-out rows
    fan_ro, fan = [0], []
    for row in rows:
        for fid in row:
            fan.extend(w.lists[w.by_id[fid]])
        fan_ro.append(len(fan))
    assert flag[0] == fan_ro and flag[1] == fan
    # DROP is FLAG with the bit-4 deliveries deleted
    keep = [k for k, b in enumerate(flag[2]) if not b & 16]
    assert drop[1] == [flag[1][k] for k in keep] and drop[2] == [flag[2][k] for k in keep]
    per_row = [sum(1 for k in range(flag[0][r], flag[0][r + 1]) if flag[2][k] & 16) for r in range(len(rows))]
    assert drop[3] == per_row and sum(per_row) == dd.n_dropped and dd.n_dropped > 0
    assert drop[0] == np.cumsum([0] + [flag[0][r + 1] - flag[0][r] - per_row[r] for r in range(len(rows))]).tolist()
    t.release()


def test_dropwhile_over_flag_output_equals_the_session():
    """FLAG mode gives a session what it needs to reproduce lists:dropwhile: for random
    batch boundaries per subscriber, dropping the leading bit-4 run of a batch and
    taking the other bytes equals ignore_local + enrich_deliver of the restatement."""
    w = R.random_world(5, n_filters=12, n_subs=10, max_list=8)
    rows, msgs = R.random_window(w, 77, n_rows=800)
    t = _table(w)
    flag, _ = _deliver(t, rows, msgs, False)
    t.release()
    # every delivery's (row, filter) in output order
    where = [(r, fid) for r, row in enumerate(rows) for fid in row for _ in w.lists[w.by_id[fid]]]
    assert len(where) == len(flag[1])
    rng = random.Random(9)
    checked = led = mid = 0
    for s in range(10):
        mine = [k for k, x in enumerate(flag[1]) if x == s]
        sess = w.session(s)
        while mine:
            n = rng.randint(1, 6)
            batch, mine = mine[:n], mine[n:]
            delivers = [("deliver", w.filters[w.by_id[where[k][1]]], dict(msgs[where[k][0]], nl=False)) for k in batch]
            want = [R.dopt_byte(m) for m in R.session_deliver(delivers, s, sess)]
            lead = 0
            while lead < len(batch) and flag[2][batch[lead]] & 16:
                lead += 1
            got = [flag[2][k] & ~16 for k in batch[lead:]]
            assert got == want
            checked += 1
            led += lead > 0
            mid += any(flag[2][k] & 16 for k in batch[lead:])
    assert checked > 50 and led > 3 and mid > 0  # hits leading a batch, and hits dropwhile keeps


def _compile(filters, lists, entries, default=0, flags=0):
    from emqx_amd import _lib, pack
    from emqx_amd.subopts import _entry_args
    ifb, ifo = pack(filters)
    so = np.zeros(len(filters) + 1, np.uint64)
    np.cumsum([len(x) for x in lists], out=so[1:])
    si = np.array([x for lst in lists for x in lst] or [0], np.uint32)
    fb, fo, es, eo, ne = _entry_args(entries)
    h = C.c_void_p()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _lib.lib().emqx_gm_subopts_compile_host(p(ifb), p(ifo), len(filters), p(so), p(si), p(fb), p(fo), p(es), p(eo),
                                                 ne, default, flags, C.byref(h))
    msg = _lib.lib().emqx_gm_last_error(None)
    return rc, h, (msg or b"").decode(errors="replace")


def test_build_refusals_name_the_entry_and_return_no_table():
    from emqx_amd import _lib
    filters, lists = [b"a/#", b"b/+"], [[1, 2], [3]]
    ok = [(b"a/#", 1, 1)]
    cases = {
        "unknown filter": ([(b"nope/+", 1, 0)], 0, 0, _lib.EINVAL, "nope/+"),
        "pair not in the list": ([(b"b/+", 1, 0)], 0, 0, _lib.EINVAL, "subscriber 1"),
        "qos 3": ([(b"a/#", 1, 3)], 0, 0, _lib.EINVAL, "opt byte"),
        "high bits": ([(b"a/#", 1, 0x20)], 0, 0, _lib.EINVAL, "opt byte"),
        "default qos 3": (ok, 3, 0, _lib.EINVAL, "default_opt"),
        "default high bits": (ok, 0x40, 0, _lib.EINVAL, "default_opt"),
        "flags": (ok, 0, 0x2, _lib.EINVAL, "flags"),
        "pair twice, different bytes": ([(b"a/#", 1, 1), (b"a/#", 1, 2)], 0, 0, _lib.EINVAL, "twice"),
    }
    for name, (entries, default, flags, code, word) in cases.items():
        rc, h, msg = _compile(filters, lists, entries, default, flags)
        assert rc == code and not h.value and word in msg, (name, rc, msg)
    rc, h, _ = _compile(filters, lists, [(b"a/#", 1, 1), (b"a/#", 1, 1)])  # twice, the same byte: stored once
    assert rc == _lib.OK
    _lib.lib().emqx_gm_subopts_release(h)
    # one subscriber twice in a list (duplicate input filters) with nl = 1: by an entry, and by the default
    dup_f, dup_l = [b"a/#", b"b/+", b"a/#"], [[1, 2], [3], [2, 4]]
    rc, h, msg = _compile(dup_f, dup_l, [(b"a/#", 2, 0x04)])
    assert rc == _lib.EUNSUPPORTED and not h.value and "twice" in msg
    rc, h, msg = _compile(dup_f, dup_l, [], default=0x04)
    assert rc == _lib.EUNSUPPORTED and not h.value
    rc, h, _ = _compile(dup_f, dup_l, [(b"a/#", 2, 0x01), (b"a/#", 1, 0x04)])  # the duplicate without nl is fine
    assert rc == _lib.OK
    _lib.lib().emqx_gm_subopts_release(h)
    # an index without subscriber lists; offsets that go down
    from emqx_amd import pack
    ifb, ifo = pack(filters)
    h = C.c_void_p()
    p = lambda a: C.c_void_p(a.ctypes.data)
    z8, z32 = np.zeros(1, np.uint8), np.zeros(1, np.uint32)
    fo0 = np.zeros(1, np.uint64)
    assert _lib.lib().emqx_gm_subopts_compile_host(p(ifb), p(ifo), 2, None, None, p(z8), p(fo0), p(z32), p(z8), 0, 0,
                                                   0, C.byref(h)) == _lib.EUNSUPPORTED and not h.value
    so, si = np.array([0, 2, 3], np.uint64), np.array([1, 2, 3], np.uint32)
    down = np.array([0, 3, 1], np.uint64)
    fb = np.frombuffer(b"a/#" + b"\0" * 61, np.uint8).copy()
    two = np.zeros(2, np.uint32)
    assert _lib.lib().emqx_gm_subopts_compile_host(p(ifb), p(ifo), 2, p(so), p(si), p(fb), p(down), p(two),
                                                   np.zeros(2, np.uint8).ctypes.data_as(C.c_void_p), 2, 0, 0,
                                                   C.byref(h)) == _lib.EINVAL and not h.value


def test_skip_unknown_counts_and_info():
    from emqx_amd import SubOptTable
    filters, lists = [b"b/+", b"a/#", b"c"], [[3], [1, 2], []]
    entries = [(b"a/#", 1, 0x05), (b"nope", 1, 1), (b"b/+", 9, 2), (b"a/#", 1, 0x05), (b"c", 1, 1), (b"b/+", 3, 0x0A)]
    t = SubOptTable.compile_host(filters, lists, entries, 0, skip_unknown=True)
    i = t.info()
    # stored: (a/#, 1) once and (b/+, 3); dropped: the unknown filter, two pairs not in their lists
    assert (i.n_entries, i.n_defaulted, i.n_nl, i.n_skipped_unknown, i.device_bytes) == (2, 1, 1, 3, 0)
    d = t.deliver_host(([0, 3], [0, 1, 2]), [0x06], [1])  # ids: a/# 0, b/+ 1, c 2
    assert d.ids.tolist() == [1, 2, 3] and d.dopt.tolist() == [1 | 8 | 16, 0, 2 | 4]
    from emqx_amd import GpuMatchError, _lib
    with pytest.raises(GpuMatchError) as e:
        t.deliver(([0, 1], [0]), [0], [1])  # a host-only table has no device half
    assert e.value.code == _lib.EUNSUPPORTED
    t.release()


def test_call_refusals_touch_no_output():
    from emqx_amd import _lib
    from emqx_amd._lib import Csr, Deliveries
    w = R.random_world(4, n_filters=6, n_subs=8, max_list=4)
    t = _table(w)

    def call(ro, ids, flags, froms, mode=0, null=(), n_rows=None, nnz=None):
        ro, ids = np.array(ro, np.uint64), np.array(ids or [0], np.uint32)
        mf, fr = np.array(flags or [0], np.uint8), np.array(froms or [0], np.uint32)
        m = Csr()
        m.n_rows, m.nnz = len(ro) - 1, int(ro[-1]) if len(ro) else 0
        if n_rows is not None:
            m.n_rows = n_rows
        if nnz is not None:
            m.nnz = nnz
        m.row_off = None if "row_off" in null else ro.ctypes.data_as(C.POINTER(C.c_uint64))
        m.ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
        d = Deliveries()
        C.memset(C.byref(d), 0xAB, C.sizeof(d))
        before = bytes(d)
        rc = _lib.lib().emqx_gm_deliver_host(None if "table" in null else t.h, None if "rows" in null else C.byref(m),
                                             None if "flags" in null else C.c_void_p(mf.ctypes.data),
                                             None if "from" in null else C.c_void_p(fr.ctypes.data), mode,
                                             None if "out" in null else C.byref(d))
        if rc != _lib.OK:
            assert bytes(d) == before
        else:
            _lib.lib().emqx_gm_deliveries_free_host(C.byref(d))
        return rc
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2]) == _lib.OK
    assert call([0, 1, 2], [0, 6], [0, 0], [1, 2]) == _lib.EINVAL       # an id >= n_filters
    assert call([0, 2, 1], [0, 1], [0, 0], [1, 2]) == _lib.EINVAL       # row_off goes down
    assert call([1, 1, 2], [0, 1], [0, 0], [1, 2]) == _lib.EINVAL       # does not start at 0
    assert call([0, 1, 2], [0, 1], [3, 0], [1, 2]) == _lib.EINVAL       # publish QoS 3
    assert call([0, 1, 2], [0, 1], [0, 0x10], [1, 2]) == _lib.EINVAL    # a high bit
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], mode=2) == _lib.EINVAL
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], null=("flags",)) == _lib.EINVAL
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], null=("from",)) == _lib.EINVAL
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], null=("row_off",)) == _lib.EINVAL
    for one in ("table", "rows", "out"):  # each NULL argument alone
        assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], null=(one,)) == _lib.EINVAL, one
    # n_rows of 2^32 - 1 (and more): refused before anything is read through the row pointers
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], n_rows=0xFFFFFFFF) == _lib.EINVAL
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], n_rows=1 << 40) == _lib.EINVAL
    assert call([0, 1, 1], [0, 1], [0, 0], [1, 2], nnz=2) == _lib.EINVAL  # the last offset is not nnz
    assert call([0, 1, 2], [0, 1], [0, 0], [1, 2], nnz=1) == _lib.EINVAL
    assert _lib.lib().emqx_gm_deliver_host(None, None, None, None, 0, None) == _lib.EINVAL
    assert call([0], [], [], []) == _lib.OK  # an empty window
    t.release()


def test_pack_helpers_and_package_exports():
    import emqx_amd
    from emqx_amd import pack_msg, pack_opt, unpack_dopt
    assert pack_opt() == 0 and pack_opt(2, nl=1, rap=1, upgrade_qos=True) == 0x1E
    assert pack_msg(1, retain=True, retained_header=True) == 0x0D
    assert unpack_dopt(0x1E) == (2, True, True, True) and unpack_dopt(1) == (1, False, False, False)
    with pytest.raises(ValueError):
        pack_opt(3)
    for name in ("SubOptTable", "build_subopts", "pack_opt", "pack_msg", "unpack_dopt"):
        assert name in emqx_amd.__all__
    assert hasattr(emqx_amd.Context, "build_subopts") and hasattr(emqx_amd.Context, "deliver")


def test_broker_subscribe_merges_the_default_subopts():
    from emqx_amd import Broker
    b = Broker(ctx=None, schedulers=2)
    b.subscribe(b"a/+", 1)
    b.subscribe(b"a/+", 2, {"qos": 2, "nl": 1})
    assert b.get_subopts(b"a/+", 1) == R.DEFAULT_SUBOPTS == R.subscribe_opts({})
    assert b.get_subopts(b"a/+", 2) == R.subscribe_opts({"qos": 2, "nl": 1}) == {"rh": 0, "rap": 0, "nl": 1, "qos": 2}
    b.subscribe(b"a/+", 2)  # a call that passes none changes nothing
    assert b.get_subopts(b"a/+", 2)["qos"] == 2 and b.subscribers(b"a/+") == [1, 2]
    b.subscribe(b"a/+", 2, {"rap": 1})  # Existed: set_subopts, merged over the defaults again
    assert b.get_subopts(b"a/+", 2) == {"rh": 0, "rap": 1, "nl": 0, "qos": 0}
    assert b.subscribers(b"a/+") == [1, 2]
    b.unsubscribe(b"a/+", 2)
    assert b.get_subopts(b"a/+", 2) is None and b.get_subopts(b"zz", 1) is None


class _Routes:
    """Stand-in for GpuRoutes over a host-only table: every topic matches the
    filter equal to it; the deliveries come from the host walk."""

    def __init__(self, world):
        from emqx_amd.batcher import _IdsOpts
        self.w, self.t, self.cls = world, _table(world), _IdsOpts
        self.other = {}
        self.subs = {s: ("client", s) for lst in world.lists for s in lst}
        self.ids = {v: k for k, v in self.subs.items()}
        self.fid = {f: world.id_of[i] for i, f in enumerate(world.filters)}

    def _rows(self, topics):
        return [[self.fid[t]] if t in self.fid else [] for t in topics]

    def groups(self, topics):
        return [[(self.w.filters[self.w.by_id[f]], np.array(self.w.lists[self.w.by_id[f]], np.uint32)) for f in row]
                for row in self._rows(topics)]

    def groups_opts(self, topics, flags, froms, drop):
        rows = self._rows(topics)
        d = self.t.deliver_host(R.csr_of(rows), flags, froms, drop)
        out = []
        for r, row in enumerate(rows):
            a, b = int(d.row_off[r]), int(d.row_off[r + 1])
            gone = int(d.row_dropped[r]) if drop else 0
            out.append([(self.w.filters[self.w.by_id[f]], self.cls(d.ids[a:b], d.dopt[a:b], gone)) for f in row])
        return out


@pytest.mark.parametrize("drop", [False, True])
def test_batcher_hands_the_option_bytes_to_deliver(drop):
    from emqx_amd.batcher import PublishBatcher
    w = R.random_world(8, n_filters=10, n_subs=12, max_list=6)
    routes = _Routes(w)
    rng = random.Random(3)
    items = []
    for k in range(120):
        i = rng.randrange(len(w.filters))
        frm = rng.choice(w.lists[i]) if w.lists[i] and rng.random() < 0.6 else None
        items.append((w.filters[i], {"qos": rng.randrange(3), "retain": rng.random() < 0.5,
                                     "retained": rng.random() < 0.3, "from": ("client", frm) if frm is not None else None,
                                     "k": k}))
    got = []
    b = PublishBatcher(routes=routes, timer=False, subopts=True, drop_no_local=drop,
                       deliver=lambda sub, f, m, byte: got.append((sub, f, m["k"], byte)) or True)
    res = b.publish_batch(items)
    want, n_local = [], 0
    for t, m in items:
        fid = routes.fid[t]
        ref_m = {"qos": m["qos"], "retain": m["retain"], "retained": m["retained"],
                 "from": m["from"][1] if m["from"] else None}
        ro, ids, dopt, dropped = w.walk([[fid]], [ref_m], drop)
        want += [(("client", s), t, m["k"], o) for s, o in zip(ids, dopt)]
        n_local += dropped[0]
    assert got == want and len(got) > 200
    assert any(o & 16 for *_, o in got) != drop
    assert b.metrics["delivery.dropped.no_local"] == n_local and (n_local > 0) == drop
    # a message whose every delivery was dropped as no_local is not a no_subscribers drop
    assert b.metrics["messages.dropped.no_subscribers"] == sum(1 for t, _ in items if not w.lists[w.filters.index(t)])
    assert len(res) == len(items)
    # subopts=False: the delivered tuples are what they were
    plain = []
    p = PublishBatcher(routes=routes, timer=False, deliver=lambda sub, f, m: plain.append((sub, f, m["k"])) or True)
    p.publish_batch(items)
    fan = [(("client", s), t, m["k"]) for t, m in items for s in w.lists[w.filters.index(t)]]
    assert plain == fan and "delivery.dropped.no_local" not in p.metrics
    if not drop:
        assert [x[:3] for x in got] == plain
    with pytest.raises(TypeError):
        PublishBatcher(groups_fn=lambda ts: [], timer=False, subopts=True)
    routes.t.release()


def test_compiler_and_host_walk_under_asan():
    """tests/asan/asan_subopts.cpp: gm_subopts.cpp as host C++ under
    AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-subopts"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_subopts")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_subopts ok" in p.stdout
