"""Session batches on the host alone: the host walk
(emqx_gm_deliver_batches_host, emqx_amd/csrc/gm_batches.cpp) against the
restatement of the reference's drained mailboxes (tests/_batches_ref.py over
tests/_subopts_ref.py), the relations between the three modes, the refusals,
and PublishBatcher(batches=True) over a stand-in for GpuRoutes.  No device is
needed.  All comparisons are exact."""

import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import _batches_ref as B
from tests import _subopts_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (B.FLAG, B.DROP, B.LEAD)


def _table(world):
    from emqx_amd import SubOptTable
    return SubOptTable.compile_host(world.filters, world.lists, world.entries(), world.default_byte())


def _args(rows, msgs):
    return R.csr_of(rows), [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]


def _host(t, rows, msgs, mode):
    return t.deliver_batches_host(*_args(rows, msgs), mode)


def _check(t, w, rows, msgs):
    """The three modes against the restatement; returns the three results."""
    out = []
    for mode in MODES:
        got = _host(t, rows, msgs, mode)
        want = B.batches(w, rows, msgs, mode)
        assert got.as_lists() == want, mode
        assert got.n_dropped == sum(g for _, _, g in want)
        assert (got.batch_dropped is None) == (mode == B.FLAG)
        assert got.batch_off[0] == 0 if len(got.batch_off) else True
        assert int(got.batch_off[-1]) == len(got.rows) == len(got.filters) == len(got.dopt)
        if mode == B.LEAD:
            assert not (got.dopt & 16).any()
        out.append(got)
    return out


@pytest.fixture(scope="module")
def world():
    w = R.random_world(1, 40, 60, 12)
    t = _table(w)
    yield w, t
    t.release()


def test_three_modes_equal_the_restatement_on_random_windows(world):
    w, t = world
    led = mid = emptied = 0
    for seed in range(100, 140):
        rows, msgs = R.random_window(w, seed, n_rows=8)
        _check(t, w, rows, msgs)
        a, b, c = B.census(w, rows, msgs)
        led, mid, emptied = led + a, mid + b, emptied + c
    assert led >= 20      # batches with a leading run
    assert mid >= 5       # batches with a hit that dropwhile keeps
    assert emptied >= 10  # batches LEAD empties
    rows, msgs = R.random_window(w, 3, n_rows=80)
    _check(t, w, rows, msgs)
    assert B.census(w, rows, msgs)[:2] == (3, 9)


def _small():
    """Filters a, b, c; subscriber 7 has nl under a and b, not under c; 9 is plain."""
    filters = [b"k/a", b"k/b", b"k/c"]
    lists = [[7, 9], [7], [9, 7]]
    opts = {(0, 7): R.subscribe_opts({"nl": 1, "qos": 1}), (1, 7): R.subscribe_opts({"nl": 1, "qos": 2}),
            (2, 7): R.subscribe_opts({"qos": 1, "rap": 1}), (0, 9): R.subscribe_opts({"qos": 2})}
    w = R.World(filters, lists, opts, {7: True})
    return w, {f: w.id_of[i] for i, f in enumerate(filters)}


def _m(frm, k=0):
    return {"qos": k % 3, "retain": bool(k & 1), "retained": False, "from": frm}


def test_constructed_cases():
    w, fid = _small()
    t = _table(w)
    a, b, c = fid[b"k/a"], fid[b"k/b"], fid[b"k/c"]
    # a leading run of length 3 (rows 0-2), a non-hit (row 3), then a hit dropwhile keeps (row 4)
    rows = [[a], [b], [a], [c], [a], [c]]
    msgs = [_m(7, 1), _m(7, 2), _m(7, 0), _m(7, 1), _m(7, 2), _m(None, 1)]
    flag, drop, lead = _check(t, w, rows, msgs)
    seven = {s: (e, g) for s, e, g in lead.as_lists()}[7]
    assert seven[1] == 3 and [r for r, _, _ in seven[0]] == [3, 4, 5]
    assert {s: g for s, _, g in drop.as_lists()}[7] == 4
    assert [bool(x & 16) for _, _, x in {s: e for s, e, _ in flag.as_lists()}[7]] == [True, True, True, False, True, False]
    # a publisher of None never hits
    flag, drop, lead = _check(t, w, [[a, b]] * 3, [_m(None, k) for k in range(3)])
    assert drop.n_dropped == lead.n_dropped == 0 and not (flag.dopt & 16).any()
    # a subscriber under two filters of one row: twice, adjacent, in the row's filter order
    flag, _, _ = _check(t, w, [[c, a], [a, c]], [_m(9, 1), _m(9, 2)])
    seven = {s: e for s, e, _ in flag.as_lists()}[7]
    assert [(r, f) for r, f, _ in seven] == [(0, c), (0, a), (1, a), (1, c)]
    # a filter listed twice in a row: its subscribers twice (the multiset rule)
    flag, drop, lead = _check(t, w, [[a, a]], [_m(7, 1)])
    assert flag.subs.tolist() == [7, 9] and flag.batch_off.tolist() == [0, 2, 4]
    assert lead.batch_off.tolist() == [0, 0, 2] and lead.batch_dropped.tolist() == [2, 0]  # emptied, still listed
    # an empty window, an all-empty window
    for rows, msgs in (([], []), ([[], [], []], [_m(7), _m(None), _m(9)])):
        for got in _check(t, w, rows, msgs):
            assert len(got.subs) == 0 and got.batch_off.tolist() == [0] and got.n_dropped == 0
    t.release()
    # a table with no subscribers
    w0 = R.World([b"k/a", b"k/b"], [[], []], {})
    t0 = _table(w0)
    for got in _check(t0, w0, [[0, 1], [1]], [_m(3), _m(None)]):
        assert len(got.subs) == 0 and got.batch_off.tolist() == [0]
    t0.release()


def test_relations_across_modes(world):
    w, t = world
    rows, msgs = R.random_window(w, 3, n_rows=80)
    flag, drop, lead = (_host(t, rows, msgs, m) for m in MODES)
    d = t.deliver_host(*_args(rows, msgs), False)
    # FLAG concatenated == a stable sort by subscriber of deliver_host's FLAG output
    order = np.argsort(d.ids, kind="stable")
    assert np.array_equal(np.repeat(flag.subs, np.diff(flag.batch_off).astype(np.int64)), d.ids[order])
    assert np.array_equal(flag.dopt, d.dopt[order])
    where_r = np.repeat(np.arange(len(rows)), np.diff(d.row_off).astype(np.int64))
    assert np.array_equal(flag.rows, where_r[order])
    where_f = np.array([fid for row in rows for fid in row for _ in w.lists[w.by_id[fid]]], np.uint32)
    assert np.array_equal(flag.filters, where_f[order])
    # DROP == FLAG minus the bit-4 entries
    keep = (flag.dopt & 16) == 0
    assert np.array_equal(drop.rows, flag.rows[keep]) and np.array_equal(drop.filters, flag.filters[keep])
    assert np.array_equal(drop.dopt, flag.dopt[keep]) and np.array_equal(drop.subs, flag.subs)
    gone = np.add.reduceat((~keep).astype(np.int64), flag.batch_off[:-1].astype(np.int64))
    assert np.array_equal(drop.batch_dropped, gone) and drop.n_dropped == int(gone.sum()) > 0
    # LEAD removes no more than DROP from any batch, and lists the same subscribers
    assert np.array_equal(lead.subs, flag.subs) and (lead.batch_dropped <= drop.batch_dropped).all()
    assert 0 < lead.n_dropped < drop.n_dropped


def _raw_call(t, fn, ro, ids, flags, froms, mode=0, null=()):
    from emqx_amd import _lib
    from emqx_amd._lib import Batches, Csr
    ro, ids = np.array(ro, np.uint64), np.array(ids or [0], np.uint32)
    mf, fr = np.array(flags or [0], np.uint8), np.array(froms or [0], np.uint32)
    m = Csr()
    m.n_rows, m.nnz = len(ro) - 1, int(ro[-1])
    m.row_off = None if "row_off" in null else ro.ctypes.data_as(C.POINTER(C.c_uint64))
    m.ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    out = Batches()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    rc = fn(None if "table" in null else t.h, None if "rows" in null else C.byref(m),
            None if "flags" in null else C.c_void_p(mf.ctypes.data),
            None if "from" in null else C.c_void_p(fr.ctypes.data), mode, None if "out" in null else C.byref(out))
    if rc != _lib.OK:
        assert bytes(out) == before  # a failing call leaves `out` untouched
    else:
        assert _lib.lib().emqx_gm_batches_free(None, C.byref(out)) == _lib.OK
    return rc


def test_refusals_touch_no_output():
    from emqx_amd import GpuMatchError, _lib
    w = R.random_world(4, n_filters=6, n_subs=8, max_list=4)
    t = _table(w)
    fn = _lib.lib().emqx_gm_deliver_batches_host
    ok = ([0, 1, 2], [0, 1], [0, 0], [1, 2])
    for mode in (0, 1, 2):
        assert _raw_call(t, fn, *ok, mode=mode) == _lib.OK
    assert _raw_call(t, fn, *ok, mode=3) == _lib.EINVAL
    for one in ("table", "rows", "out", "flags", "from", "row_off"):
        assert _raw_call(t, fn, *ok, null=(one,)) == _lib.EINVAL, one
    assert _raw_call(t, fn, [0, 1, 2], [0, 1], [3, 0], [1, 2]) == _lib.EINVAL     # publish QoS 3
    assert _raw_call(t, fn, [0, 1, 2], [0, 1], [0, 0x10], [1, 2]) == _lib.EINVAL  # a high bit
    assert _raw_call(t, fn, [0, 2, 1], [0, 1], [0, 0], [1, 2]) == _lib.EINVAL     # offsets go down
    assert _raw_call(t, fn, [0, 1, 2], [0, 6], [0, 0], [1, 2]) == _lib.EINVAL     # an id >= n_filters
    assert _raw_call(t, fn, [0], [], [], []) == _lib.OK                           # an empty window
    # mode 2 stays refused by the per-delivery calls
    from emqx_amd.shared import _host_csr
    m, keep = _host_csr([0, 1, 2], [0, 1])
    mf, fr, d = np.zeros(2, np.uint8), np.array([1, 2], np.uint32), _lib.Deliveries()
    assert _lib.lib().emqx_gm_deliver_host(t.h, C.byref(m), C.c_void_p(mf.ctypes.data), C.c_void_p(fr.ctypes.data), 2,
                                           C.byref(d)) == _lib.EINVAL
    # a device call on a host-only table
    with pytest.raises(GpuMatchError) as e:
        t.deliver_batches(([0, 1], [0]), [0], [1])
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(GpuMatchError) as e:
        t.deliver_batches_device(None, 0, 0)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ValueError):
        t.deliver_batches_host(([0, 1], [0]), [0], [1], "first")

    # another snapshot's rows: refused through the binding (a host-only table is bound to none)
    class _Index:
        h = C.c_void_p(0x1000)
    with pytest.raises(GpuMatchError) as e:
        t.deliver_batches_host(([0, 1], [0]), [0], [1], "lead", index=_Index())
    assert e.value.code == _lib.EINVAL
    t.release()


def test_package_exports():
    import emqx_amd
    from emqx_amd import _lib
    assert _lib.SO_LEAD == 2
    for name in ("SessionBatches", "DeviceBatches"):
        assert name in emqx_amd.__all__
    for name in ("deliver_batches", "deliver_batches_device", "deliver_batches_host"):
        assert hasattr(emqx_amd.SubOptTable, name)


class _Routes:
    """Stand-in for GpuRoutes over a host-only table: every topic matches the
    filter equal to it; deliveries and batches come from the host walks."""

    def __init__(self, world):
        from emqx_amd.batcher import _IdsOpts
        self.w, self.t, self.cls = world, _table(world), _IdsOpts
        self.other = {}
        self.subs = {s: ("client", s) for lst in world.lists for s in lst}
        self.ids = {v: k for k, v in self.subs.items()}
        self.fid = {f: world.id_of[i] for i, f in enumerate(world.filters)}

    def _rows(self, topics):
        return [[self.fid[t]] if t in self.fid else [] for t in topics]

    def _name(self, f):
        return self.w.filters[self.w.by_id[f]]

    def groups(self, topics):
        return [[(self._name(f), np.array(self.w.lists[self.w.by_id[f]], np.uint32)) for f in row]
                for row in self._rows(topics)]

    def groups_opts(self, topics, flags, froms, drop):
        rows = self._rows(topics)
        d = self.t.deliver_host(R.csr_of(rows), flags, froms, drop)
        out = []
        for r, row in enumerate(rows):
            a, b = int(d.row_off[r]), int(d.row_off[r + 1])
            out.append([(self._name(f), self.cls(d.ids[a:b], d.dopt[a:b], int(d.row_dropped[r]) if drop else 0))
                        for f in row])
        return out

    def groups_batches(self, topics, flags, froms, mode="flag"):
        rows = self._rows(topics)
        sb = self.t.deliver_batches_host(R.csr_of(rows), flags, froms, mode)
        names = {f: self._name(f) for row in rows for f in row}
        return [[(names[f], f, len(self.w.lists[self.w.by_id[f]])) for f in row] for row in rows], names, sb


@pytest.mark.parametrize("drop", [False, True])
def test_batcher_gives_each_subscriber_one_call_per_window(drop):
    from emqx_amd.batcher import PublishBatcher
    w = R.random_world(8, n_filters=10, n_subs=12, max_list=6)
    routes = _Routes(w)
    rng = random.Random(3)
    items = []
    nl_of = {i: [s for s in lst if w.opts.get((i, s), w.default)["nl"]] for i, lst in enumerate(w.lists)}
    for k in range(120):
        i = rng.randrange(len(w.filters))
        frm = rng.choice(w.lists[i]) if w.lists[i] and rng.random() < 0.6 else None
        if k < 10 and nl_of[k]:  # the window opens with No-Local hits: they lead their subscribers' batches
            i, frm = k, nl_of[k][0]
        items.append((w.filters[i], {"qos": rng.randrange(3), "retain": rng.random() < 0.5,
                                     "retained": rng.random() < 0.3, "from": ("client", frm) if frm is not None else None,
                                     "k": k}))
    calls = []
    b = PublishBatcher(routes=routes, timer=False, subopts=True, batches=True, drop_no_local=drop,
                       deliver_batch=lambda sub, lst: calls.append((sub, [(f, m["k"], o) for f, m, o in lst])) or True)
    res = b.publish_batch(items)
    assert len(res) == len(items)
    assert len({sub for sub, _ in calls}) == len(calls) > 5  # one call per subscriber per window
    rows = [[routes.fid[t]] for t, _ in items]
    ref_msgs = [{"qos": m["qos"], "retain": m["retain"], "retained": m["retained"],
                 "from": m["from"][1] if m["from"] else None} for _, m in items]
    want = B.batches(w, rows, ref_msgs, B.LEAD if drop else B.FLAG)
    assert calls == [(("client", s), [(w.filters[w.by_id[f]], r, o) for r, f, o in e]) for s, e, _ in want if e]
    assert b.metrics["delivery.dropped.no_local"] == sum(g for _, _, g in want) and (sum(g for _, _, g in want) > 0) == drop
    # the per-delivery form of the same window (FLAG: nothing removed; its drop rule is DROP, not dropwhile)
    got = []
    p = PublishBatcher(routes=routes, timer=False, subopts=True,
                       deliver=lambda sub, f, m, byte: got.append((sub, f, m["k"], byte)) or True)
    res_p = p.publish_batch(items)
    if not drop:
        by_sub = sorted(range(len(got)), key=lambda i: got[i][0][1])  # (a stable sort by subscriber id)
        assert [(s, x) for s, lst in calls for x in lst] == [(got[i][0], got[i][1:]) for i in by_sub]
        assert b.metrics == p.metrics and res == res_p
    assert b.metrics["messages.dropped.no_subscribers"] == p.metrics["messages.dropped.no_subscribers"]
    assert b.metrics["messages.publish"] == p.metrics["messages.publish"] == len(items)
    with pytest.raises(TypeError):
        PublishBatcher(routes=routes, timer=False, subopts=True, batches=True, one_call=True,
                       deliver_batch=lambda sub, lst: True)
    with pytest.raises(TypeError):
        PublishBatcher(routes=routes, timer=False, subopts=True, batches=True)  # no deliver_batch
    routes.t.release()


def test_host_walk_under_asan():
    """tests/asan/asan_batches.cpp: gm_batches.cpp and gm_subopts.cpp as host C++
    under AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-batches"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_batches")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_batches ok" in p.stdout
