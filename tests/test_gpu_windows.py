"""Publish windows coalesced into one device round trip (emqx_gm_match_windows,
emqx_gm_combiner; gm_host.cpp run_host_windows, gm_windows.hip k_rows_split).

The reference is the unchanged direct path: ctx.match_fanout (ctx.match for
match-only) of each window alone.  Every assertion is array equality."""

import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILTERS = sorted({b"a/#", b"a/+", b"a/b", b"+/b", b"#", b"c/d", b"a/+/c", b"none/+", b"x/y/z"})
CYCLE = [b"a/b", b"a/x", b"c/d", b"q", b"a/b/c", b"$SYS/a", b"none/x", b"x/y/z"]
MAX_WINDOWS = 64  # emqx_gm_match_windows' group limit (include/emqx_gpu_match.h)

SIZES = [
    [1], [0], [0, 0, 1, 0],
    [63, 1], [64, 64], [65, 63],  # window edges inside and on a 64-topic wave tile
    [255, 1, 257, 3],             # the 256-topic block
    [1] * 64,
    [1024] * 8,
    [2] * MAX_WINDOWS, [2] * (MAX_WINDOWS + 1),  # the call runs a second group
]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _subs():
    rng = np.random.default_rng(9)
    subs = [rng.integers(0, 1 << 20, size=int(rng.integers(1, 300))).astype(np.uint32).tolist() for _ in FILTERS]
    subs[FILTERS.index(b"none/+")] = []
    return subs


@pytest.fixture(scope="module")
def idx(ctx):
    ix = ctx.build_index(FILTERS, subs=_subs())
    yield ix
    ix.release()


def _windows(sizes, shift=3):
    """Consecutive slices of the eight-topic cycle, each window starting where the last ended."""
    out, pos = [], shift
    for n in sizes:
        out.append([CYCLE[(pos + i) % len(CYCLE)] for i in range(n)])
        pos += n
    return out


def _same(a, b):
    """a, b: (row_off, ids) or ((row_off, ids), (row_off, ids))."""
    if isinstance(a[0], tuple):
        return _same(a[0], b[0]) and _same(a[1], b[1])
    return (a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype and np.array_equal(a[0], b[0])
            and np.array_equal(a[1], b[1]))


_REF = {}


def _ref(ctx, ix, topics, exact=True, fanout=True):
    """The direct call of one window alone, computed once per distinct window."""
    key = (id(ix), tuple(topics), exact, fanout)
    if key not in _REF:
        _REF[key] = ctx.match_fanout(ix, topics, exact=exact) if fanout else ctx.match(ix, topics, exact=exact)
    return _REF[key]


def _check(ctx, ix, windows, exact=True, fanout=True, ref_ctx=None, ref_ix=None):
    got = ctx.match_windows(ix, windows, exact=exact, fanout=fanout)
    assert len(got) == len(windows)
    for k, (g, w) in enumerate(zip(got, windows)):
        want = _ref(ref_ctx or ctx, ref_ix or ix, w, exact, fanout)
        assert _same(g, want), f"window {k} of {len(windows)} ({len(w)} topics)"
        ro = g[0][0] if fanout else g[0]
        assert ro[0] == 0 and len(ro) == len(w) + 1
    return got


@pytest.mark.parametrize("fanout", [True, False], ids=["deliveries", "match_only"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "trie"])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)) if len(s) < 5 else f"{s[0]}x{len(s)}")
def test_window_sizes(ctx, idx, sizes, exact, fanout):
    _check(ctx, idx, _windows(sizes), exact, fanout)
    _check(ctx, idx, _windows(sizes), exact, fanout)  # (again, with the capacities the first call left)


def test_base_case_equals_the_oracle(ctx, idx, orc):
    subs = _subs()
    so = np.zeros(len(FILTERS) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in subs])
    si = np.array([x for s in subs for x in s], np.uint32)
    windows = _windows([65, 63, 8])
    got = _check(ctx, idx, windows)
    r = orc.Router(True)
    for f in FILTERS:
        r.add_route(f)
    for (m, d), w in zip(got, windows):
        oro, oids, _ = r.match_batch(w, FILTERS, mode=1)
        ero, eids = orc.fanout(oro, oids, so, si)
        assert np.array_equal(m[0], oro) and np.array_equal(m[1], oids)
        assert np.array_equal(d[0], ero) and np.array_equal(d[1], eids)


def test_window_without_a_match_between_two(ctx, idx):
    windows = [[b"a/b"] * 3, [b"$SYS/a", b"$SYS/q", b"$SYS/a"], [b"c/d", b"a/b/c"]]
    got = _check(ctx, idx, windows)
    assert got[1][0][0].tolist() == [0, 0, 0, 0] and got[1][1][0].tolist() == [0, 0, 0, 0]
    _check(ctx, idx, windows, fanout=False)


def test_wide_fanout_in_the_middle_window(ctx):
    """x/# with 300,000 subscribers, hit by the middle window only: the first
    call (its deliveries outgrow the speculative capacity of a fresh context)
    and the second are both equal, the other windows unaffected."""
    from emqx_amd import Context
    filters, subs = [b"x/#", b"y"], [list(range(300_000)), [5]]
    windows = [[b"y", b"q"], [b"x/1", b"y", b"x/2/3"], [b"y"]]
    ref_ix = ctx.build_index(filters, subs=subs)
    with Context(0) as fresh:
        big = fresh.build_index(filters, subs=subs)
        for _ in range(2):
            _check(fresh, big, windows, ref_ctx=ctx, ref_ix=ref_ix)
        _check(fresh, big, windows, fanout=False, ref_ctx=ctx, ref_ix=ref_ix)
        big.release()
    ref_ix.release()


def test_no_speculative_ids(ctx, idx, monkeypatch):
    windows = _windows([65, 0, 63, 300])
    want = [_ref(ctx, idx, w) for w in windows]
    want_m = [_ref(ctx, idx, w, fanout=False) for w in windows]
    monkeypatch.setenv("EMQX_GM_AB", "1")
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    got = ctx.match_windows(idx, windows)
    got_m = ctx.match_windows(idx, windows, fanout=False)
    monkeypatch.delenv("GM_NO_SPEC_IDS")
    assert all(_same(g, w) for g, w in zip(got, want))
    assert all(_same(g, w) for g, w in zip(got_m, want_m))


def test_long_topic_runs_alone(ctx, idx):
    long_topic = b"a/" + b"x" * 70_000
    windows = [[b"a/b"] * 5, [b"c/d", long_topic, b"a/b"], [b"c/d"] * 3, [b"a/b/c", b"q"]]
    for fanout in (True, False):
        _check(ctx, idx, windows, fanout=fanout)


def test_text_past_the_limit_is_cut_into_groups(ctx, idx):
    # 40 windows x 8 topics x ~5 KB: 1.6 MB of text, more than one group's 1 MiB
    windows = [[t + b"/" + bytes([97 + k % 26]) * 5000 for t in CYCLE] for k in range(40)]
    assert sum(len(t) for w in windows for t in w) > (1 << 20)
    _check(ctx, idx, windows)
    _check(ctx, idx, windows, exact=False, fanout=False)


def test_after_update_subs(ctx, idx):
    idx2 = ctx.update_subs(idx, [(b"a/b", 7, True), (b"zz/+", 9, True), (b"c/d", 11, True)])
    windows = _windows([9, 70]) + [[b"zz/q"] * 5]
    _check(ctx, idx2, windows)
    idx2.release()


def test_overlay_snapshot_takes_the_ordinary_path(ctx):
    from emqx_amd._lib import GpuMatchError
    plain = ctx.build_index(FILTERS)
    ov = ctx.update_index(plain, [(b"a/#/b", True)])
    windows = _windows([5, 70, 1])
    _check(ctx, ov, windows, fanout=False)
    with pytest.raises(GpuMatchError) as direct:
        ctx.match_fanout(ov, windows[0])
    with pytest.raises(GpuMatchError) as grouped:
        ctx.match_windows(ov, windows)
    assert grouped.value.code == direct.value.code and "overlay" in str(grouped.value)
    ov.release()
    plain.release()


def test_two_member_context(ctx, idx):
    """A context over devices [0, 0]: groups run whole on one member, round-robin;
    every CSR is freed through the top context (match_windows does)."""
    from emqx_amd import Context
    with Context(devices=[0, 0]) as c2:
        ix = c2.build_index(FILTERS, subs=_subs())
        for _ in range(4):  # (both members serve)
            _check(c2, ix, _windows([65, 63, 1, 0, 300]), ref_ctx=ctx, ref_ix=idx)
            _check(c2, ix, _windows([2] * (MAX_WINDOWS + 1)), fanout=False, ref_ctx=ctx, ref_ix=idx)
        ix.release()


def test_bad_arguments(ctx, idx):
    from emqx_amd import _lib
    from emqx_amd.engine import pack
    from emqx_amd._lib import GpuMatchError
    tb, to = pack(CYCLE)
    bad = to.copy()
    bad[3] = bad[5] + 1  # not monotone
    with pytest.raises(GpuMatchError) as e:
        ctx.match_windows(idx, [CYCLE, (tb, bad), CYCLE])
    assert e.value.code == _lib.EINVAL and "monotone" in str(e.value)
    L = _lib.lib()
    w = (_lib.Window * 1)()
    m = (_lib.Csr * 1)()
    m[0].n_rows = 77
    assert L.emqx_gm_match_windows(ctx.h, idx.h, w, 1, 0x2, m, None) == _lib.EINVAL  # flags
    assert L.emqx_gm_match_windows(ctx.h, None, w, 1, 0, m, None) == _lib.EINVAL
    assert m[0].n_rows == 77  # no output touched
    assert ctx.match_windows(idx, []) == []


def _run_threads(n, fn):
    errs = []

    def one(k):
        try:
            fn(k)
        except Exception as e:  # noqa: BLE001
            errs.append((k, e))
    th = [threading.Thread(target=one, args=(k,)) for k in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return errs


def test_combiner_forms_one_group_of_four(ctx, idx):
    windows = _windows([65, 1, 300, 64])
    want = [_ref(ctx, idx, w) for w in windows]
    outs = [None] * 4
    cb = ctx.combiner(min_windows=4, linger_us=5_000_000)

    def call(k):
        outs[k] = cb.match_fanout(idx, windows[k])
    errs = _run_threads(4, call)
    st = cb.stats()
    cb.close()
    assert not errs, errs
    assert all(_same(o, w) for o, w in zip(outs, want))
    assert st == {"windows": 4, "groups": 1, "max_group": 4, "solo": 0}


def test_combiner_concurrent_callers(ctx, idx):
    from emqx_amd import _lib
    from emqx_amd._lib import GpuMatchError
    windows = _windows([64, 1, 129, 7, 300, 2, 65, 33])
    want = [_ref(ctx, idx, w) for w in windows]
    want_m = [_ref(ctx, idx, w, exact=False, fanout=False) for w in windows]
    bad = [0] * 8
    cb = ctx.combiner()

    def call(k):
        for i in range(20):
            if i % 2:
                got, ref = cb.match(idx, windows[k], exact=False), want_m[k]
            else:
                got, ref = cb.match_fanout(idx, windows[k]), want[k]
            bad[k] += not _same(got, ref)
    errs = _run_threads(8, call)
    st = cb.stats()
    assert not errs, errs
    assert bad == [0] * 8
    assert st["windows"] == 160 and st["groups"] <= 160 and st["max_group"] >= 1
    # a caller's figures after its call: its group's (a group holds at least its own window)
    cb.match_fanout(idx, windows[4])
    assert ctx.stats()["n_topics"] >= len(windows[4])
    cb.close()
    with pytest.raises(GpuMatchError) as e:
        cb.match_fanout(idx, windows[0])
    assert e.value.code == _lib.EINVAL


def test_batcher_through_a_combiner(ctx):
    """GpuRoutes(..., combiner=cb): the fanout_batch path goes through the combiner, same groups."""
    from emqx_amd.batcher import GpuRoutes
    cb = ctx.combiner()
    plain, via = GpuRoutes(ctx, node=b"n1"), GpuRoutes(ctx, node=b"n1", combiner=cb)
    for r in (plain, via):
        r.subscribe(b"a/+", "s1")
        r.subscribe(b"a/b", "s2")
        r.subscribe(b"#", "s1")
    topics = [b"a/b", b"q", b"a/x/y", b"$SYS/x"]
    want = plain.groups(topics)
    assert cb.stats()["windows"] == 0
    assert via.groups(topics) == want and any(want)
    assert cb.stats()["windows"] == 1
    cb.close()


def test_combiner_bad_offsets_fail_that_call_alone(ctx, idx):
    from emqx_amd import _lib
    from emqx_amd.engine import pack
    from emqx_amd._lib import GpuMatchError
    windows = _windows([65, 1, 300, 64])
    want = [_ref(ctx, idx, w) for w in windows]
    tb, to = pack(windows[2])
    bad = to.copy()
    bad[3] = bad[5] + 1
    outs = [None] * 4
    cb = ctx.combiner(min_windows=3, linger_us=5_000_000)

    def call(k):
        outs[k] = cb.match_fanout(idx, (tb, bad) if k == 2 else windows[k])
    errs = _run_threads(4, call)
    st = cb.stats()
    cb.close()
    assert [k for k, _ in errs] == [2]
    assert isinstance(errs[0][1], GpuMatchError) and errs[0][1].code == _lib.EINVAL
    assert all(_same(outs[k], want[k]) for k in (0, 1, 3))
    assert st["windows"] == 3 and st["groups"] == 1  # (the bad window never queued)
