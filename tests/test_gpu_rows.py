"""The row consumers of emqx_amd/csrc/gm_csr.hip (k_fanout_copy, k_fanout_rowoff,
k_merge_rows, k_row_lengths, k_ov_merge) and the scan they share (gm_scan.h:
scan_excl's forms, k_scan_loop) at their boundaries, integer array against
integer array: the cases and plain references of tests/_rows_ref.py, whose
coverage of the boundaries tests/test_rows_ref_cpu.py establishes without a
device (the references against the oracle, the case list against classify).

The match lists are the test's own, not match results: the number of entries
picks the scan form, the segment lengths pick the copy path.  The shapes are
the smallest that cross each boundary."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import _rows_ref as R

pytestmark = pytest.mark.gpu

SMALL_CASES = [n for n in R.FAN_CASES if n not in R.BIG_CASES]


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fan(ctx):
    """The fan-out index (one filter per length) and each case's reference, computed once."""
    idx = ctx.build_index(R.FILTERS, subs=R.LISTS)
    perm = idx.perm.copy()
    assert sorted(perm.tolist()) == list(range(len(R.FILTERS)))
    so, si = R.world_csr(perm)
    refs = {}

    def ref(name):
        if name not in refs:
            case = R.fan_case(name)
            ro, ids = R.fanout_ref(case.m_off, case.ids(perm), so, si)
            ro.setflags(write=False)
            ids.setflags(write=False)
            refs[name] = (ro, ids)
        return refs[name]
    yield SimpleNamespace(idx=idx, perm=perm, ref=ref)
    idx.release()


def _device_rows(ctx, row_off, ids):
    """A device CSR the test makes itself (the RawRows of the subscription-option tests, without messages)."""
    from tests.test_gpu_subopts import RawRows
    return RawRows(ctx, row_off, ids, np.zeros(1, np.uint8), np.zeros(1, np.uint32))


def _same(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]), what + ": row_off"
    assert len(got[1]) == len(want[1]), what + ": %d ids, want %d" % (len(got[1]), len(want[1]))
    if not np.array_equal(got[1], want[1]):
        at = int(np.flatnonzero(got[1] != want[1])[0])
        raise AssertionError("%s: ids differ first at delivery %d: %d, want %d" % (what, at, got[1][at], want[1][at]))


# ------------------------------------------------------------------ fan-out
@pytest.mark.parametrize("name", SMALL_CASES)
def test_fanout_host_rows_default_path_twice(ctx, fan, name, monkeypatch):
    """emqx_gm_fanout of host rows, twice.  The first call sizes its speculative capacity by whatever
    the context's last fan-out left and may overflow it (then the ordinary path serves it); it leaves the
    deliveries per match exact, so the second call is the small host driver (run_fanout_small ->
    queue_fanout_small: k_scan_loop up to 32,767 entries, scan_excl above) -- its stats carry no device
    time.  By design a call of 65,536 rows or more (scan_4097_wide) and one expected past 16M deliveries
    (no case here; the two ~4.19M-entry lists are left to the tests below) take the ordinary path,
    which the stats show as well."""
    monkeypatch.delenv("GM_FANOUT_SIMPLE", raising=False)
    case = R.fan_case(name)
    ids = case.ids(fan.perm)
    for call in ("first call", "second call"):
        _same(ctx.fanout(fan.idx, case.m_off, ids), fan.ref(name), call)
    st = ctx.stats()
    assert st["n_topics"] == case.n_rows and st["nnz"] == case.total
    small = R.classify(case)["small"] is not None
    assert (st["total_device_ms"] == 0.0) == small, st


@pytest.mark.parametrize("name", R.FAN_CASES)
def test_fanout_host_rows_ordinary_path(ctx, fan, name, monkeypatch):
    """GM_FANOUT_SIMPLE=1: run_fanout on host rows (scan_excl in every form, the two ~4.19M-entry lists included)."""
    monkeypatch.setenv("GM_FANOUT_SIMPLE", "1")
    case = R.fan_case(name)
    _same(ctx.fanout(fan.idx, case.m_off, case.ids(fan.perm)), fan.ref(name), "host rows")
    assert ctx.stats()["total_device_ms"] > 0.0 and ctx.stats()["nnz"] == case.total


@pytest.mark.parametrize("name", R.FAN_CASES)
def test_fanout_device_rows(ctx, fan, name):
    case = R.fan_case(name)
    raw = _device_rows(ctx, case.m_off, case.ids(fan.perm))
    out = ctx.fanout_device(fan.idx, raw.csr)
    got, n_rows = out.to_host(), out.n_rows
    out.free()
    raw.free()
    assert n_rows == case.n_rows
    _same(got, fan.ref(name), "device rows")


@pytest.mark.parametrize("name,n_parts", R.PART_CASES)
def test_fanout_parts(ctx, fan, name, n_parts):
    """emqx_gm_fanout_part cut anywhere: inside a segment at every residue mod 4, on a segment start that
    a run of zero-length segments precedes, and more parts than deliveries (empty parts)."""
    case = R.fan_case(name)
    ids = case.ids(fan.perm)
    w_ro, w_ids = fan.ref(name)
    raw = _device_rows(ctx, case.m_off, ids)
    pos, got = 0, []
    for p in range(n_parts):
        part, first = ctx.fanout_part(fan.idx, raw.csr, p, n_parts)
        (ro, pids), n_rows = part.to_host(), part.n_rows
        part.free()
        want_first, want = R.fanout_part_ref(case.m_off, ids, None, None, p, n_parts, whole=(w_ro, w_ids))
        assert first == pos == want_first, "part %d" % p
        assert n_rows == case.n_rows and len(pids) == len(want)  # (an empty part: nnz == 0)
        _same((ro, pids), (w_ro, want), "part %d of %d" % (p, n_parts))
        pos += len(pids)
        got.append(pids)
    raw.free()
    assert pos == case.total
    assert np.array_equal(np.concatenate(got), w_ids)
    if name == "tiny":
        assert sum(1 for g in got if len(g) == 0) == 3


# ------------------------------------------------------------------ row merge, row lengths
def _upload(ctx, a):
    p = ctx.dev_alloc(max(a.nbytes, 16))
    if a.nbytes:
        ctx.memcpy_h2d(p, np.ascontiguousarray(a), a.nbytes)
    return p


@pytest.mark.parametrize("n,stride,pieces", R.MERGE_WORLDS)
def test_merge_rows_synthetic(ctx, n, stride, pieces):
    """emqx_gm_merge_rows on lists the test dealt: one piece, stride > n, no rows, a piece that is empty for
    a row, all pieces empty, ids 0 and 0xFFFFFFFF, one 5,000-id row, P * stride either side of 4,095."""
    w = R.merge_world(n, stride, pieces)
    d_lens, d_ids = _upload(ctx, w.lens), _upload(ctx, w.ids)
    out = ctx.merge_rows(n, stride, pieces, d_lens, d_ids)
    got, n_rows = out.to_host(), out.n_rows
    out.free()
    ctx.dev_free(d_lens)
    ctx.dev_free(d_ids)
    want = R.merge_rows_ref(w.lens, w.ids, n)
    assert n_rows == n and len(got[0]) == n + 1
    _same(got, want, w.name)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_row_lengths(ctx, n):
    rng = np.random.RandomState(n)
    ro = np.concatenate([[0], np.cumsum(rng.randint(0, 9, size=n))]).astype(np.uint64)
    raw = _device_rows(ctx, ro, np.zeros(int(ro[-1]), np.uint32))
    guard = np.full(n + 3, 0xDEADBEEF, np.uint32)
    d_out = _upload(ctx, guard)
    ctx.csr_row_lengths(raw.csr, d_out)
    got = np.zeros(n + 3, np.uint32)
    ctx.memcpy_d2h(got, d_out, got.nbytes)
    ctx.dev_free(d_out)
    raw.free()
    assert np.array_equal(got[:n], R.row_lengths_ref(ro)) and np.array_equal(got[:n], np.diff(ro).astype(np.uint32))
    assert (got[n:] == 0xDEADBEEF).all()  # (nothing written past row n - 1)


# ------------------------------------------------------------------ overlay remap edges
def _ov_ops(current, before, tag, after):
    """Delete the filters at ids 0, 31, 32, 33, 63, 64 and the last of the sorted set `current`; insert
    `before` (sorts before the first), one filter between ids 32 and 33, and `after` (sorts after the last)."""
    cur = sorted(current)
    dels = [cur[i] for i in (0, 31, 32, 33, 63, 64, len(cur) - 1)]
    between = cur[32] + b"/" + tag + b"/#"  # (cur[32] ends in "/+": the filter below it sorts right after it)
    assert cur[32] < between < cur[33] and before < cur[0] and after > cur[-1]
    return [(f, False) for f in dels] + [(f, True) for f in (before, between, after)]


def test_overlay_remap_at_bitmap_word_edges(ctx, orc, monkeypatch):
    """k_ov_merge / ov_remap with tombstones at bit 31 of a bitmap word, bits 0 and 1 of the next, the last
    base id, and insertion points before the first, between two tombstones and after the last base filter:
    rows equal a rebuilt index's and the oracle's, both with and without exact filters; then the same
    edit again on top of that overlay (an update of a superseded snapshot: the same base, more tombstones
    and a larger delta) -- which also deletes delta filters of the first edit, tombstones base ids 95 and
    96 (the next word edge) and brings base id 32 back."""
    from tests.test_gpu_parity import _oracle_rows
    monkeypatch.setenv("GM_UPDATE_OVERLAY", "1")
    current = {b"w%03d/+" % i for i in range(200)}
    topics = [b"w%03d/x" % i for i in range(200)] + [b"zzx/q", b"zzy/q", b"x/x", b"x/q", b"w032/q/x", b"w032/q/x/r",
                                                      b"w034/q/y", b"w034/q/y/r", b"w032/q", b"w095/q", b"w096/q"]
    idx = ctx.build_index(sorted(current))
    snaps = [idx]
    edits = [(b"+/x", b"x", b"zzx/+", []),
             (b"+/q", b"y", b"zzy/+", [(b"w095/+", False), (b"w096/+", False), (b"w032/+", True)])]
    for (before, tag, after, more), n_final in zip(edits, (196, 191)):
        if tag == b"x":  # the first edit's deletes are the base ids themselves
            assert [sorted(current)[i] for i in (0, 31, 32, 33, 63, 64, 199)] == \
                [b"w%03d/+" % i for i in (0, 31, 32, 33, 63, 64, 199)]
        ops = _ov_ops(current, before, tag, after) + more
        for f, ins in ops:
            (current.add if ins else current.discard)(f)
        new = ctx.update_index(snaps[-1], ops)
        snaps.append(new)
        assert ctx.update_stats()["kind"] == "overlay"
        final = sorted(current)
        assert new.n_filters == len(final) == n_final
        assert [new.filter(i) for i in range(new.n_filters)] == final
        rebuilt = ctx.build_index(final)
        for exact in (True, False):
            got = ctx.match(new, topics, exact=exact)
            _same(got, ctx.match(rebuilt, topics, exact=exact), "rebuilt, exact=%s" % exact)
            _same(got, _oracle_rows(orc, final, topics, 1 if exact else 0), "oracle, exact=%s" % exact)
            assert len(got[1]) > 190
        rebuilt.release()
    for s in snaps:
        s.release()
