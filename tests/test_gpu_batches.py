"""Session batches on the device (emqx_gm_deliver_batches,
emqx_amd/csrc/gm_batches.hip) against the restatement of the reference's
drained mailboxes (tests/_batches_ref.py) and the host walk over the device
table's own host copy -- array for array, in FLAG, DROP and LEAD mode, on host
rows and on device rows the test made itself.  The shapes are the smallest
that cross each boundary of the path: the radix passes (one per 8-bit digit of
the largest subscriber id), a chunk's 256-pair step, a wave's 64 lanes, and
the scans' 1,024-value blocks and 4,096-value one-launch form."""

import ctypes as C

import numpy as np
import pytest

from tests import _batches_ref as B
from tests import _subopts_ref as R

pytestmark = pytest.mark.gpu

MODES = (B.FLAG, B.DROP, B.LEAD)


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


def _word(f):
    return 0xFFFFFFFF if f is None else f


def _same(a, b):
    assert np.array_equal(a.subs, b.subs) and np.array_equal(a.batch_off, b.batch_off)
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.filters, b.filters) and np.array_equal(a.dopt, b.dopt)
    assert (a.batch_dropped is None) == (b.batch_dropped is None) and a.n_dropped == b.n_dropped
    assert a.batch_dropped is None or np.array_equal(a.batch_dropped, b.batch_dropped)


class Dev:
    """One option set on the device, with its index."""

    def __init__(self, ctx, world):
        self.ctx, self.w = ctx, world
        self.index = ctx.build_index(world.filters, subs=world.lists)
        self.t = ctx.build_subopts(self.index, world.entries(), world.default_byte())

    def check(self, rows, msgs, chunks=(0,), device_rows=True, restate=True):
        """Device (host rows; raw device rows) == host walk (== the restatement), the three modes, every chunk count."""
        csr, flags, froms = R.csr_of(rows), [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]
        raw = RawRows(self.ctx, csr[0], csr[1], flags, [_word(f) for f in froms]) if device_rows else None
        out = {}
        for mode in MODES:
            host = self.t.deliver_batches_host(csr, flags, froms, mode)
            if restate:
                want = B.batches(self.w, rows, msgs, mode)
                assert host.as_lists() == want, mode
            for c in chunks:
                _same(self.t.deliver_batches(csr, flags, froms, mode, index=self.index, n_chunks=c), host)
                if raw is not None:
                    dd = self.t.deliver_batches_device(raw.csr, raw.d_flags, raw.d_from, mode, index=self.index,
                                                       n_chunks=c)
                    back = dd.to_host()
                    dd.free()
                    _same(back, host)
            out[mode] = host
        if raw is not None:
            raw.free()
        return out

    def release(self):
        self.t.release()
        self.index.release()


def _m(frm, k=0):
    return {"qos": k % 3, "retain": bool(k & 1), "retained": bool(k & 4) and not k & 2, "from": frm}


# ------------------------------------------------------------------ random worlds
@pytest.fixture(scope="module")
def base():
    w = R.random_world(1, 40, 60, 12)
    rows, msgs = R.random_window(w, 3, n_rows=80)
    return w, rows, msgs


def test_random_world_three_modes_host_and_device_rows(ctx, base):
    w, rows, msgs = base
    d = Dev(ctx, w)
    out = d.check(rows, msgs)
    assert B.census(w, rows, msgs)[:2] == (3, 9)
    assert 0 < out[B.LEAD].n_dropped < out[B.DROP].n_dropped
    assert d.t.batches_last_times()[5] == 1  # ids below 256: one pass
    d.release()


def test_a_call_makes_three_host_blocking_waits(ctx, base):
    """the pre-removal total, the batch count with the kept total, the end of the call -- from host
    rows and from device rows, in every mode; a window whose rows are all empty makes none from host rows."""
    w, rows, msgs = base
    d = Dev(ctx, w)
    csr, flags, froms = R.csr_of(rows), [R.msg_byte(m) for m in msgs], [m["from"] for m in msgs]
    raw = RawRows(ctx, csr[0], csr[1], flags, [_word(f) for f in froms])
    for mode in MODES:
        d.t.deliver_batches(csr, flags, froms, mode)
        assert d.t.batches_last_times()[6] == 3, mode
        d.t.deliver_batches_device(raw.csr, raw.d_flags, raw.d_from, mode).free()
        assert d.t.batches_last_times()[6] == 3, mode
    raw.free()
    d.t.deliver_batches(([0, 0, 0], []), [0, 0], None, "lead")
    assert d.t.batches_last_times()[6] == 0
    d.release()


# ------------------------------------------------------------------ radix passes and per-pass stability
@pytest.mark.parametrize("largest,passes", [(255, 1), (256, 2), (65535, 2), (65536, 3), ((1 << 24) - 1, 3),
                                            (1 << 24, 4), (0xFFFFFFFE, 4)])
def test_largest_id_sets_the_passes(ctx, base, largest, passes):
    w0, rows, msgs0 = base
    used = sorted({s for lst in w0.lists for s in lst})
    step = max(1, largest // 64)  # the ids spread over every digit the largest has
    rank = {s: k for k, s in enumerate(used)}
    fn = lambda s: largest - (len(used) - 1 - rank[s]) * step
    w = B.map_world(w0, fn)
    msgs = [dict(m, **{"from": fn(m["from"]) if m["from"] in rank else None}) for m in msgs0]
    d = Dev(ctx, w)
    out = d.check(rows, msgs)
    assert int(out[B.FLAG].subs.max()) == largest and d.t.batches_last_times()[5] == passes
    assert out[B.DROP].n_dropped > 0
    d.release()


def test_equal_low_digits_only_a_later_pass_separates(ctx):
    ids = [5, 5 + (1 << 8), 5 + (1 << 16), 5 + (1 << 24), 6]
    filters = [b"d/a", b"d/b", b"d/c"]
    lists = [[ids[3], ids[0], ids[4], ids[2], ids[1]], [ids[1], ids[3]], [ids[4], ids[0], ids[2]]]
    opts = {(i, s): R.subscribe_opts({"nl": (i + s) & 1, "qos": s % 3}) for i, lst in enumerate(lists) for s in lst}
    w = R.World(filters, lists, opts)
    rows = [[k % 3] if k % 4 else [(k + 1) % 3, k % 3] for k in range(150)]
    msgs = [_m(ids[k % 5] if k % 3 else None, k) for k in range(150)]
    d = Dev(ctx, w)
    out = d.check(rows, msgs)
    assert out[B.FLAG].subs.tolist() == sorted(ids) and d.t.batches_last_times()[5] == 4
    assert len(out[B.FLAG].rows) > 512
    d.release()


# ------------------------------------------------------------------ chunking
def test_forced_chunk_counts_give_one_result(ctx, base):
    w, _, _ = base
    rows, msgs = R.random_window(w, 11, n_rows=400)
    d = Dev(ctx, w)
    n = sum(len(w.lists[w.by_id[f]]) for row in rows for f in row)
    assert n > 1500
    d.check(rows, msgs, chunks=(0, 1, 2, 3, 7, n // 256 + 1, n // 256 + 2))  # (the last: clamped)
    from emqx_amd import GpuMatchError, _lib
    with pytest.raises(GpuMatchError) as e:
        d.t.deliver_batches(R.csr_of(rows), [0] * len(rows), None, "lead", n_chunks=1025)
    assert e.value.code == _lib.EINVAL
    d.release()


@pytest.fixture(scope="module")
def five(ctx):
    """Filter A with five subscribers (three with nl), B with one: any delivery count is some rows of each."""
    filters, lists = [b"n/a", b"n/b"], [[300, 7, 70000, 12, 9], [8]]
    opts = {(0, 300): R.subscribe_opts({"nl": 1, "qos": 1}), (0, 7): R.subscribe_opts({"nl": 1}),
            (0, 12): R.subscribe_opts({"nl": 1, "qos": 2, "rap": 1}), (1, 8): R.subscribe_opts({"nl": 1})}
    d = Dev(ctx, R.World(filters, lists, opts, {7: True}))
    yield d
    d.release()


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513])
def test_windows_of_exact_delivery_counts(five, n):
    w = five.w
    a, b = w.id_of[0], w.id_of[1]
    rows = [[a]] * (n // 5) + [[b]] * (n % 5)
    msgs = [_m([300, 7, 9, None, 12, 8][k % 6], k) for k in range(len(rows))]
    out = five.check(rows, msgs, chunks=(0, 2))
    assert int(out[B.FLAG].batch_off[-1]) == n


# ------------------------------------------------------------------ lane and wave ranking
@pytest.fixture(scope="module")
def lanes(ctx):
    filters = [b"w/hot", b"w/x", b"w/pair", b"w/first", b"w/last"]
    lists = [[9], [4, 9, 2], [3, 4], [1], [0]]
    opts = {(0, 9): R.subscribe_opts({"nl": 1, "qos": 1}), (2, 3): R.subscribe_opts({"nl": 1})}
    d = Dev(ctx, R.World(filters, lists, opts))
    yield d
    d.release()


@pytest.mark.parametrize("count", [64, 65, 256])
def test_one_subscriber_holding_consecutive_deliveries(lanes, count):
    w = lanes.w
    hot, x = w.id_of[0], w.id_of[1]
    rows = [[x]] + [[hot]] * count + [[x]]
    msgs = [_m(9 if k % 5 == 0 else None, k) for k in range(len(rows))]
    out = lanes.check(rows, msgs)
    nine = {s: e for s, e, _ in out[B.FLAG].as_lists()}[9]
    assert [r for r, _, _ in nine] == list(range(0, count + 2))


def test_two_subscribers_alternating_across_a_256_step(lanes):
    w = lanes.w
    rows = [[w.id_of[2]]] * 300  # deliveries 3, 4, 3, 4, ...: 600 of them
    msgs = [_m(3 if k in (0, 1, 127, 128, 299) else None, k) for k in range(300)]
    out = lanes.check(rows, msgs, chunks=(0, 1, 2))
    assert out[B.FLAG].batch_off.tolist() == [0, 300, 600] and out[B.LEAD].batch_dropped.tolist() == [2, 0]
    assert out[B.DROP].batch_dropped.tolist() == [5, 0]


def test_hot_subscriber_in_every_row_with_heads_at_both_ends(lanes):
    w = lanes.w
    hot, first, last = w.id_of[0], w.id_of[3], w.id_of[4]
    rows = [[first, hot]] + [[hot]] * 1998 + [[hot, last]]
    msgs = [_m(9 if k < 3 or k % 400 == 0 else None, k) for k in range(2000)]
    out = lanes.check(rows, msgs, chunks=(0, 3))
    flag = out[B.FLAG]
    assert flag.subs.tolist() == [0, 1, 9] and flag.batch_off.tolist() == [0, 1, 2, 2002]
    assert flag.rows[0] == 1999 and flag.rows[1] == 0  # the single deliveries at the last k and at k = 0
    assert out[B.LEAD].batch_dropped.tolist() == [0, 0, 3]


# ------------------------------------------------------------------ LEAD across boundaries
def test_leading_run_across_steps_chunks_and_scan_blocks(five):
    """Subscriber 7's leading run is 1,500 deliveries long: it crosses the 256-pair steps, the forced chunk
    boundaries and the scans' 1,024-value blocks (4,545 deliveries: the scans take their two-level form)."""
    w = five.w
    a = w.id_of[0]
    rows = [[a]] * 1515
    msgs = [_m(7 if k < 1500 or k >= 1510 else None, k) for k in range(1515)]
    out = five.check(rows, msgs, chunks=(0, 2, 3))
    lead = {s: (e, g) for s, e, g in out[B.LEAD].as_lists()}
    assert lead[7][1] == 1500 and [r for r, _, _ in lead[7][0]] == list(range(1500, 1515))
    assert {s: g for s, _, g in out[B.DROP].as_lists()}[7] == 1505


def test_emptied_batch_between_kept_ones_and_a_hit_at_the_end(five):
    w = five.w
    a, b = w.id_of[0], w.id_of[1]
    # 8's every delivery is its own (emptied; between 7 and 9); 12's only hit is its last delivery (kept by LEAD)
    rows = [[a], [b], [a], [b], [a]]
    msgs = [_m(None, 1), _m(8, 2), _m(None, 3), _m(8, 4), _m(12, 5)]
    out = five.check(rows, msgs)
    lead = out[B.LEAD]
    assert lead.subs.tolist() == [7, 8, 9, 12, 300, 70000]
    assert lead.batch_off.tolist() == [0, 3, 3, 6, 9, 12, 15] and lead.batch_dropped.tolist() == [0, 2, 0, 0, 0, 0]
    assert out[B.DROP].batch_dropped.tolist() == [0, 2, 0, 1, 0, 0]


# ------------------------------------------------------------------ device rows the host never saw
def test_unvalidated_device_rows_are_skipped_and_clamped(five):
    t, w = five.t, five.w
    a, b = w.id_of[0], w.id_of[1]
    rows = [[a, 2 + 3, b], [0xFFFFFFFF], [b, a]]
    clean = [[a, b], [], [b, a]]
    msgs = [_m(7, 1), _m(None, 2), _m(8, 3)]
    ro, ids = R.csr_of(rows)
    for mode in MODES:
        want = B.batches(w, clean, msgs, mode)
        raw = RawRows(five.ctx, ro[:-1] + [ro[-1] + 9], ids, [R.msg_byte(m) | 0xF0 for m in msgs],
                      [_word(m["from"]) for m in msgs], nnz=len(ids))
        dd = t.deliver_batches_device(raw.csr, raw.d_flags, raw.d_from, mode)
        back = dd.to_host()
        dd.free()
        raw.free()
        assert back.as_lists() == want, mode


# ------------------------------------------------------------------ refusals
def test_overflow_is_decided_by_the_counting_pass(ctx):
    from emqx_amd import GpuMatchError, _lib
    n = 1 << 20
    index = ctx.build_index([b"big/#"], subs=(np.array([0, n], np.uint64), np.arange(n, dtype=np.uint32)))
    t = ctx.build_subopts(index, [], default=0)
    rows = (np.arange(4097, dtype=np.uint64), np.zeros(4096, np.uint32))  # 4,096 rows x 2^20: 2^32 deliveries
    for mode in MODES:
        with pytest.raises(GpuMatchError) as e:
            t.deliver_batches(rows, np.zeros(4096, np.uint8), None, mode, index=index)
        assert e.value.code == _lib.EOVERFLOW
    t.release()
    index.release()


def test_refused_calls_touch_no_output_and_mode_2_stays_refused_elsewhere(five):
    from emqx_amd import _lib
    from emqx_amd._lib import Batches, Csr, Deliveries
    ctx, t = five.ctx, five.t
    ro, ids = np.array([0, 1], np.uint64), np.zeros(1, np.uint32)
    mf, fr = np.zeros(1, np.uint8), np.ones(1, np.uint32)
    m = Csr()
    m.n_rows, m.nnz = 1, 1
    m.row_off, m.ids = ro.ctypes.data_as(C.POINTER(C.c_uint64)), ids.ctypes.data_as(C.POINTER(C.c_uint32))
    p = lambda a: C.c_void_p(a.ctypes.data)
    L = _lib.lib()
    for kw in ({"mode": 3}, {"ids": 2}, {"flags": 3}, {"n_rows": 0xFFFFFFFF}):
        ids[0], mf[0], m.n_rows = kw.get("ids", 0), kw.get("flags", 0), kw.get("n_rows", 1)
        out = Batches()
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        before = bytes(out)
        assert L.emqx_gm_deliver_batches(ctx.h, t.h, C.byref(m), p(mf), p(fr), kw.get("mode", 2),
                                         C.byref(out)) == _lib.EINVAL, kw
        assert bytes(out) == before
    ids[0], mf[0], m.n_rows = 0, 0, 1
    assert L.emqx_gm_deliver_batches(ctx.h, t.h, C.byref(m), p(mf), p(fr), 2, None) == _lib.EINVAL
    d = Deliveries()
    assert L.emqx_gm_deliver(ctx.h, t.h, C.byref(m), p(mf), p(fr), 2, C.byref(d)) == _lib.EINVAL
    assert L.emqx_gm_deliver_host(t.h, C.byref(m), p(mf), p(fr), 2, C.byref(d)) == _lib.EINVAL
    # another snapshot's rows: refused through the binding
    from emqx_amd import GpuMatchError
    other = ctx.build_index(five.w.filters, subs=five.w.lists)
    with pytest.raises(GpuMatchError) as e:
        t.deliver_batches(([0, 1], [0]), [0], [1], "lead", index=other)
    assert e.value.code == _lib.EINVAL
    other.release()


# ------------------------------------------------------------------ against the existing kernel, moderate size
def test_flag_batches_are_a_stable_sort_of_the_deliver_call(ctx):
    rnd = np.random.RandomState(5)
    nf, ns, n_rows = 200, 5000, 2000
    filters = [b"m/%03d/#" % i for i in range(nf)]
    lists = [rnd.choice(ns, size=rnd.randint(0, 26), replace=False).astype(np.uint32) * 13 + 1 for _ in range(nf)]
    index = ctx.build_index(filters, subs=[x.tolist() for x in lists])
    entries = [(filters[i], int(s), int((s % 3) | (4 if s % 5 == 0 else 0) | (8 if s & 8 else 0)))
               for i in range(nf) for s in lists[i][::2]]
    t = ctx.build_subopts(index, entries, default=1)
    rows = [sorted(rnd.choice(nf, size=rnd.randint(0, 9), replace=False).tolist()) for _ in range(n_rows)]
    ro, ids = R.csr_of(rows)
    flags = (np.arange(n_rows) % 3 | (np.arange(n_rows) & 4)).astype(np.uint8)
    froms = np.array([int(lists[r[0]][0]) if r and len(lists[r[0]]) else 0xFFFFFFFF for r in rows], np.uint32)
    d = t.deliver((ro, ids), flags, froms, index=index)
    assert len(d.ids) > 80_000
    order = np.argsort(d.ids, kind="stable")
    where_r = np.repeat(np.arange(n_rows), np.diff(d.row_off).astype(np.int64)).astype(np.uint32)
    where_f = np.array([f for row in rows for f in row for _ in range(len(lists[f]))], np.uint32)
    got = t.deliver_batches((ro, ids), flags, froms, "flag", index=index)
    assert np.array_equal(np.repeat(got.subs, np.diff(got.batch_off).astype(np.int64)), d.ids[order])
    assert np.array_equal(got.dopt, d.dopt[order]) and (got.dopt & 16).sum() > 100
    assert np.array_equal(got.rows, where_r[order]) and np.array_equal(got.filters, where_f[order])
    assert (np.diff(got.subs.astype(np.int64)) > 0).all() and t.batches_last_times()[5] == 2
    for mode in (B.DROP, B.LEAD):
        _same(t.deliver_batches((ro, ids), flags, froms, mode, index=index),
              t.deliver_batches_host((ro, ids), flags, froms, mode))
    t.release()
    index.release()


# ------------------------------------------------------------------ a multi-device context
def test_two_listed_devices_the_call_runs_on_the_tables_device(base):
    from emqx_amd import Context
    w, rows, msgs = base
    with Context(devices=[0, 0]) as c2:
        d = Dev(c2, w)
        d.check(rows, msgs)
        d.release()


# ------------------------------------------------------------------ GpuRoutes + PublishBatcher
def test_gpu_routes_and_batcher_deliver_by_subscriber(ctx):
    from emqx_amd.batcher import GpuRoutes, PublishBatcher
    routes = GpuRoutes(ctx)
    routes.subscribe(b"t/+", "a", {"qos": 1, "nl": 1})
    routes.subscribe(b"t/+", "b", {"qos": 2, "rap": 1, "upgrade_qos": True})
    routes.subscribe(b"t/1", "c")
    routes.subscribe(b"t/1", "a", {"qos": 0})
    items = [(b"t/1", {"qos": 1, "retain": True, "from": "a", "k": 0}), (b"t/2", {"qos": 2, "from": "c", "k": 1}),
             (b"t/3", {"qos": 1, "from": "a", "k": 2}), (b"zz", {"k": 3})]
    flag = {"a": [(b"t/+", 0, 1 | 8 | 16), (b"t/1", 0, 0), (b"t/+", 1, 1 | 8), (b"t/+", 2, 1 | 8 | 16)],
            "b": [(b"t/+", 0, 2 | 4), (b"t/+", 1, 2), (b"t/+", 2, 2)], "c": [(b"t/1", 0, 0)]}
    lead = dict(flag, a=[(f, k, o & ~16) for f, k, o in flag["a"][1:]])  # only the leading hit goes; k = 2's stays
    for drop, want in ((False, flag), (True, lead)):
        calls = []
        b = PublishBatcher(routes=routes, timer=False, subopts=True, batches=True, drop_no_local=drop,
                           deliver_batch=lambda sub, lst: calls.append((sub, [(f, m["k"], o) for f, m, o in lst])) or True)
        res = b.publish_batch(items)
        assert dict(calls) == want and len(calls) == 3, drop
        assert res[3] == [] and b.metrics["messages.dropped.no_subscribers"] == 1
        assert b.metrics["delivery.dropped.no_local"] == (1 if drop else 0)
    rows, names, sb = routes.groups_batches([b"t/1", b"zz"], [1, 0], [None, None])
    assert [[(f, n) for f, _, n in row] for row in rows] == [[(b"t/+", 2), (b"t/1", 2)], []]
    assert len(sb.subs) == 3 and int(sb.batch_off[-1]) == 4
