"""The match statistics against a plain reference (tests/_nfa_ref.py).

stats()["probes"] is SURVEY.md section 8d's P summed over the batch -- the
probes the reference NFA makes, not a count of loads: the kernels book virtual
probes for work they skip (the push filter, chain nodes, the level-0 round
from registers, the exact-route probe), and several host paths decide whether
a per-tile side sum is added once, twice or not at all.  bench.py builds the
roofline's numerator from it, so it is checked here as an exact integer, with
n_wildcard_topics, for every index form, kernel form and call path; the rows
are checked against the oracle as everywhere else.

The contract (include/emqx_gpu_match.h): exact when no row leaves a pass for
capacity; otherwise each such row may be counted by up to two passes.  The
batches of the equality tests are built so that no row does -- at most 8
matches per row (FAST_MC = 16) and a frontier of at most 3 per topic (64 x 3 <
CW_CAP) -- which each test checks on the CPU with the reference.  test_overflow_rows_* assert the bounds for rows that do.
"""

import itertools
import random

import numpy as np
import pytest

from tests import _nfa_ref as R
from tests.test_gpu_parity import CHAIN_FILTERS, CHAIN_TOPICS, _layout_env, _oracle_rows

pytestmark = pytest.mark.gpu

MAX_ROW, MAX_FRONTIER = 8, 3


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the filter sets and their topics
VOCAB = [b"a", b"b", b"c", b"dd", b"", b"$SYS", b"$x", b"longword_over_8_bytes", b"l0w1", b"e", b"f1", b"g"]
ABSENT = b"zz_in_no_filter"
# a filter that is also a 10-level publish topic with '+' as its last word (levels counted from 0: level 9)
DEEP_WILD_LITERAL = b"a/b/c/dd/e/f1/g/a/b/+"


def _base_filters():
    """~600 filters of 1..12 levels over a small vocabulary (dense first levels,
    long unique tails: chain nodes under GM_CHAIN), 8 % '+' words, 25 % '#' tails."""
    rng = random.Random(41)
    fs = {b"#", b"+", b"$SYS/#", b"", b"/", b"a/", b"$x", b"$SYS/+", DEEP_WILD_LITERAL}
    while len(fs) < 600:
        n = rng.choice([1, 2, 2, 3, 3, 3, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12])
        ws = [b"+" if rng.random() < 0.08 else rng.choice(VOCAB) for _ in range(n)]
        if ws[:2] == [b"+", b"+"]:  # (no '+/+' prefix: a/x, a/+ and +/x keep a level-1 frontier at 3)
            ws[1] = rng.choice(VOCAB)
        if rng.random() < 0.25:
            ws.append(b"#")
        fs.add(b"/".join(ws))
    return sorted(fs)


def _kinds(filters, rng):
    """The topic kinds of the issue, each derived from the filters."""
    def fill(f, lo=0, hi=2):
        ws = f.split(b"/")
        if ws[-1] == b"#":
            ws = ws[:-1] + [rng.choice(VOCAB) for _ in range(rng.randint(lo, hi))]
        return [rng.choice(VOCAB[:4]) if w == b"+" else w for w in ws] or [b""]

    shallow = [f for f in filters if f.count(b"/") < 8]
    deepf = [f for f in filters if 8 <= f.count(b"/") <= 11 and not f.endswith(b"#")]
    k = {n: [] for n in ("match", "absent", "empty", "dollar", "one", "wild", "deep", "deepwild")}
    for f in rng.sample(shallow, 260):
        ws = fill(f)
        if len(ws) <= 8:
            k["match"].append(ws)
    for ws in rng.sample(k["match"], 50):  # an absent word at each level
        for lv in range(len(ws)):
            k["absent"].append(ws[:lv] + [ABSENT] + ws[lv + 1:])
    k["empty"] = [[b""], [b"", b""], [b"", b"", b""], [b"a", b""], [b"", b"a"], [b"a", b"", b"b"]]
    for ws in rng.sample(k["match"], 40):
        lv = rng.randrange(len(ws))
        k["empty"].append(ws[:lv] + [b""] + ws[lv + 1:])
    k["dollar"] = [[b"$SYS"], [b"$SYS", b"a"], [b"$x"], [b"$x", b"a", b"b"], [b"$nope"], [b"$nope", b"a"], [b"$SYS", b""]]
    k["dollar"] += [fill(f) for f in shallow if f.startswith(b"$")][:60]
    k["one"] = [[w] for w in VOCAB] + [[ABSENT]]
    for ws in rng.sample(k["match"], 40):  # wildcard publish topics; some are filters themselves (the literal route)
        lv = rng.randrange(len(ws))
        k["wild"].append(ws[:lv] + [rng.choice([b"+", b"#"])] + ws[lv + 1:])
    k["wild"] += [f.split(b"/") for f in rng.sample([f for f in shallow if R.is_wildcard(f)], 25)]
    for f in deepf:  # 9..12 levels: the listed pass walks them, the main pass counts 0
        k["deep"].append(fill(f))
        ws = fill(f)
        ws[rng.randrange(len(ws))] = ABSENT
        k["deep"].append(ws)
    for f in rng.sample([f for f in shallow if f.endswith(b"/#")], 40):  # a '#' filter's topic, 9..12 levels long
        ws = fill(f, 0, 0)
        k["deep"].append(ws + [rng.choice(VOCAB) for _ in range(rng.randint(9, 12) - len(ws))])
    # a wildcard word past the 8 tokenized levels: at level 9 (the topic is then both deep and a
    # wildcard topic: the main pass counts it in n_wildcard_topics and queues it, the listed pass
    # must add neither probes nor a second count), at level 8 (8 levels counted: not deep) and later
    for ws in [w for w in k["deep"] if len(w) == 10][:12]:
        k["deepwild"].append(ws[:9] + [rng.choice([b"+", b"#"])])
        k["deepwild"].append(ws[:8] + [rng.choice([b"+", b"#"])] + ws[9:])
    for ws in [w for w in k["deep"] if len(w) == 12][:6]:
        k["deepwild"].append(ws[:10] + [rng.choice([b"+", b"#"])] + ws[11:])
    k["deepwild"].append(DEEP_WILD_LITERAL.split(b"/"))
    return {n: [b"/".join(ws) for ws in v] for n, v in k.items()}


def _pool(ref, kinds, n):
    """n topics, the kinds in turn (every prefix of 8 or more holds all of them),
    only topics that cannot leave a pass for capacity."""
    ok = {kn: [t for t in v if len(ref.walk(t)[1]) <= MAX_ROW and ref.walk(t)[3] <= MAX_FRONTIER]
          for kn, v in kinds.items()}
    for kn, v in ok.items():
        assert len(v) >= min(6, len(kinds[kn])), (kn, len(v), len(kinds[kn]))
    out = []
    for i in itertools.count():
        for kn in ok:
            out.append(ok[kn][i % len(ok[kn])])
        if len(out) >= n:
            return out[:n]


class Case:
    """A filter set, its reference and a topic pool (built once per module)."""

    def __init__(self, filters, pool=None, n=1000):
        self.ref = R.Ref(filters)
        self.filters = self.ref.filters
        self.pool = pool if pool is not None else _pool(self.ref, _kinds(self.filters, random.Random(43)), n)
        self.check_capacity(self.pool)

    def check_capacity(self, topics):
        assert self.ref.max_row(topics) <= MAX_ROW and self.ref.max_frontier(topics) <= MAX_FRONTIER


@pytest.fixture(scope="module")
def base():
    c = Case(_base_filters())
    assert 200 <= len(c.filters) <= 2000
    # the pool really holds what the tests are about
    deep = [t for t in c.pool if t.count(b"/") >= 8]
    for lv in (8, 9, 10):  # wildcard words at, and past, the last tokenized level
        assert sum(1 for t in deep if len(t.split(b"/")) > lv and t.split(b"/")[lv] in (b"+", b"#")) >= 5, lv
    assert DEEP_WILD_LITERAL in c.pool
    assert sum(1 for t in deep if not R.is_wildcard(t)) > 50
    return c


@pytest.fixture(scope="module")
def chain():
    """The chain filter set of test_gpu_parity and every topic length around each chain."""
    topics = [t.encode() for t in CHAIN_TOPICS + [t + "/x" for t in CHAIN_TOPICS]]
    topics += [t + b"/x/y" for t in topics[:len(CHAIN_TOPICS)]] + [b"m/n/o/p/q/r/s/t/u", b"m/n/o/p/q/r/s/+/u/v",
                                                                   b"m/n/o/p/q/r/s/t/u/+", b"m/n/o/p/q/r/s/t/u/v/#"]
    return Case([f.encode() for f in CHAIN_FILTERS], pool=topics)


# ------------------------------------------------------------------ one call, every counter
def _call(ctx, idx, topics, exact, how):
    from emqx_amd.engine import pack
    if how == "host":
        return ctx.match(idx, topics, exact=exact)
    tb, to = pack(topics)
    d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
    ctx.memcpy_h2d(d_tb, tb, len(tb))
    ctx.memcpy_h2d(d_to, to, len(to) * 8)
    try:
        res = ctx.match_device(idx, d_tb, d_to, len(topics), exact=exact)
        out = res.to_host()
        res.free()
        return out
    finally:
        ctx.dev_free(d_tb)
        ctx.dev_free(d_to)


def _check_stats(ctx, case, topics, what):
    p_ref, wild_ref, _ = case.ref.batch(topics)
    st = ctx.stats()
    print(f"{what}: n={len(topics)} probes={st['probes']} P_ref={p_ref} wild={st['n_wildcard_topics']} "
          f"wild_ref={wild_ref} n_overflow={st['n_overflow']}")
    assert st["n_topics"] == len(topics), what
    assert st["probes"] == p_ref, (what, st["probes"], p_ref)
    assert st["n_wildcard_topics"] == wild_ref, (what, st["n_wildcard_topics"], wild_ref)
    assert st["n_overflow"] == 0, what  # no row of these batches takes the slow path


def _check(ctx, orc, idx, case, topics, how="host", modes=(True, False), what=""):
    for exact in modes:
        ro, ids = _call(ctx, idx, topics, exact, how)
        oro, oids = _oracle_rows(orc, case.filters, topics, 1 if exact else 0)
        assert np.array_equal(ro, oro) and np.array_equal(ids, oids), (what, exact)
        _check_stats(ctx, case, topics, f"{what} exact={exact} {how}")


SIZES = [63, 64, 65, 257, 1000]


# ------------------------------------------------------------------ index forms
def _build_form(ctx, case, form, monkeypatch):
    if form == "chain":
        monkeypatch.setenv("GM_CHAIN", "1")
    elif form == "mph":
        monkeypatch.setenv("GM_MPH_MIN_KEYS", "1")
    elif form == "no_mph":
        monkeypatch.setenv("GM_NO_MPH", "1")
    elif form == "dense":
        _layout_env(monkeypatch, "dense")
    if form != "patched":
        return ctx.build_index(case.filters)
    # the same set reached by an in-place patch: built without every 7th filter and
    # with strangers, which one update inserts and deletes
    monkeypatch.delenv("GM_UPDATE_OVERLAY", raising=False)
    late = case.filters[3::7]
    strangers = [b"zq/%d/+" % i for i in range(20)] + [b"a/zq/#", b"+/zq"]
    first = ctx.build_index(sorted((set(case.filters) - set(late)) | set(strangers)))
    idx = ctx.update_index(first, [(f, True) for f in late] + [(f, False) for f in strangers])
    assert ctx.update_stats()["kind"] == "patch"
    first.release()
    assert [idx.filter(i) for i in range(idx.n_filters)] == case.filters
    return idx


FORMS = ["default", "chain", "mph", "no_mph", "dense", "patched"]


@pytest.mark.parametrize("form", FORMS)
def test_index_forms(ctx, orc, base, form, monkeypatch):
    """P and the wildcard count are the reference's on every index layout the
    walk reads differently: open addressing, chain nodes, hash-and-displace
    tables (every table / none), the dense dictionary and hot tables, and a
    snapshot patched in place.  Batches of 1, 63, 64, 65, 257 and 1,000 topics."""
    idx = _build_form(ctx, base, form, monkeypatch)
    for t in base.pool[:8] + [DEEP_WILD_LITERAL]:  # one topic of each kind alone
        _check(ctx, orc, idx, base, [t], what=f"{form} single")
    for n in SIZES:
        _check(ctx, orc, idx, base, base.pool[:n], what=form)
    idx.release()


@pytest.mark.parametrize("form", ["chain", "no_chain", "chain_mph"])
def test_chain_nodes_every_length(ctx, orc, chain, form, monkeypatch):
    """The chain set of test_gpu_parity: every topic length around each chain
    (the vx / vp arithmetic of coop_walk_tile books the probes the reference
    makes along a chain the walk does not follow)."""
    monkeypatch.setenv("GM_CHAIN", "0" if form == "no_chain" else "1")
    if form == "chain_mph":
        monkeypatch.setenv("GM_MPH_MIN_KEYS", "1")
    idx = ctx.build_index(chain.filters)
    for how in ("host", "device"):
        _check(ctx, orc, idx, chain, chain.pool, how=how, what=form)
    for t in chain.pool:  # each topic alone: a miscount cannot hide in a sum
        ro, ids = ctx.match(idx, [t], exact=True)
        assert ctx.stats()["probes"] == chain.ref.walk(t)[0], (form, t)
    idx.release()


# ------------------------------------------------------------------ kernel forms
KERNEL_FORMS = [{}, {"GM_STAGE_COMPACT": "0"}, {"GM_D0": "0"}, {"GM_STAGE_SC1": "1"}, {"GM_HOT_FLAT": "1"},
                {"GM_FUSED_PRIO": "0"}, {"GM_NT": "0"}, {"GM_NT": "0", "GM_STAGE_COMPACT": "0"}]


def _form_id(env):
    return "-".join(f"{k[3:].lower()}={v}" for k, v in env.items()) or "default"


@pytest.mark.parametrize("env", KERNEL_FORMS, ids=_form_id)
@pytest.mark.parametrize("chains", [False, True], ids=["plain", "chains"])
def test_kernel_forms(ctx, orc, base, env, chains, monkeypatch):
    """Every instantiation of the main pass: k_match_fused with each A/B form,
    nt and plain streams; rows against the oracle and the counters against the
    reference."""
    if chains:
        monkeypatch.setenv("GM_CHAIN", "1")
    idx = ctx.build_index(base.filters)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n in (65, 1000):
        _check(ctx, orc, idx, base, base.pool[:n], what=_form_id(env))
    _check(ctx, orc, idx, base, base.pool[:257], how="device", what=_form_id(env))
    idx.release()


# ------------------------------------------------------------------ call paths
def test_small_host_and_device_paths(ctx, orc, base):
    idx = ctx.build_index(base.filters)
    for how in ("host", "device"):
        for n in (1, 64, 1000):
            _check(ctx, orc, idx, base, base.pool[:n], how=how, what="path")
    idx.release()


def test_chunked_host_path_sums_chunks(ctx, orc, base, monkeypatch):
    """GM_HOST_CHUNK=1024 over 5,000 topics: five chunks, P their sum."""
    monkeypatch.setenv("GM_HOST_CHUNK", "1024")
    idx = ctx.build_index(base.filters)
    topics = (base.pool * 5)[:5000]
    _check(ctx, orc, idx, base, topics, what="chunked")
    idx.release()


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("compact", ["0", "1"])
def test_listed_pass_deferred_or_not(ctx, orc, base, defer, compact, monkeypatch):
    """Deep topics present: the listed pass launched with the main pass or left
    to the read-back (where the main pass's side sum must not be added again);
    then a batch without listed rows on the same context."""
    monkeypatch.setenv("GM_LISTED_DEFER", defer)
    monkeypatch.setenv("GM_STAGE_COMPACT", compact)
    idx = ctx.build_index(base.filters)
    deep = [t for t in base.pool if t.count(b"/") >= 8]
    shallow = [t for t in base.pool if t.count(b"/") < 8]
    for how in ("host", "device"):
        _check(ctx, orc, idx, base, base.pool, how=how, what=f"defer={defer}")
        _check(ctx, orc, idx, base, deep, how=how, modes=(True,), what=f"defer={defer} deep only")
        _check(ctx, orc, idx, base, shallow[:300], how=how, modes=(True,), what=f"defer={defer} none listed")
    idx.release()


def test_no_speculative_ids(ctx, orc, base, monkeypatch):
    monkeypatch.setenv("GM_NO_SPEC_IDS", "1")
    idx = ctx.build_index(base.filters)
    for how in ("host", "device"):
        _check(ctx, orc, idx, base, base.pool, how=how, what="no spec ids")
    idx.release()


def test_speculative_redo_counts_once(ctx, orc):
    """The redo of test_speculative_ids_capacity_redo: after a match-free batch
    the speculative ids buffer is too small for ~8 matches per topic and the
    rows are assembled again; the probes are not counted again."""
    filters = [b"#", b"a/#", b"a/b/#", b"a/b/c/#", b"a/b/c/d/#", b"a/b/c/d", b"a/+/c/d", b"a/b/c/+"]
    n = 20_000
    none = [b"$x/%d" % (i % 50) for i in range(n)]  # '$' topics: no root '#', nothing else matches
    many = [b"a/b/c/d" if i % 3 else b"a/b/c/d/%d" % (i % 7) for i in range(n)]  # 8 and 5 matches
    case = Case(filters, pool=none[:4] + many[:8])
    filters = case.filters
    case.check_capacity(none + many)
    idx = ctx.build_index(filters)
    for how in ("host", "device"):
        for topics in (none, many, many):
            ro, ids = _call(ctx, idx, topics, True, how)
            oro, oids = _oracle_rows(orc, filters, topics, 1)
            assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
            st = ctx.stats()
            p_ref, wild_ref, _ = case.ref.batch(topics)
            assert (st["probes"], st["n_wildcard_topics"], st["n_overflow"]) == (p_ref, wild_ref, 0), how
        assert int(oro[-1]) > 6 * n  # (past the capacity a match-free batch leaves: 1,024 + n ids)
    idx.release()


@pytest.mark.parametrize("asm_stream", [None, "1"])
def test_calls_in_flight_each_its_own_counters(ctx, orc, base, monkeypatch, asm_stream):
    """24 match_submit calls in flight (more than the ring of 16 pre-zeroed
    counter blocks), two different batches in turn -- one with deep topics, so
    its listed pass runs at the read-back, after the ring has moved on: each
    call's counters are its own."""
    from emqx_amd.engine import pack
    if asm_stream:
        monkeypatch.setenv("GM_ASM_STREAM", asm_stream)
    idx = ctx.build_index(base.filters)
    batches = [base.pool[:700], [t for t in base.pool if t.count(b"/") < 8][:333]]
    want, bufs = [], []
    for topics in batches:
        tb, to = pack(topics)
        d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
        ctx.memcpy_h2d(d_tb, tb, len(tb))
        ctx.memcpy_h2d(d_to, to, len(to) * 8)
        bufs.append((d_tb, d_to))
        want.append(_oracle_rows(orc, base.filters, topics, 1))
    pend = [ctx.match_submit(idx, *bufs[k % 2], len(batches[k % 2]), timed=(k % 5 == 0)) for k in range(24)]
    for k, p in enumerate(pend):
        res = p.wait()
        _check_stats(ctx, base, batches[k % 2], f"in flight {k}")
        ro, ids = res.to_host()
        res.free()
        assert np.array_equal(ro, want[k % 2][0]) and np.array_equal(ids, want[k % 2][1]), k
    for d_tb, d_to in bufs:
        ctx.dev_free(d_tb)
        ctx.dev_free(d_to)
    idx.release()


@pytest.mark.parametrize("env", [{}, {"GM_SCAN_SPLIT": "0"}, {"GM_SCAN_SUMS": "0"}], ids=_form_id)
def test_large_batch_split_scan(ctx, orc, base, env, monkeypatch):
    """One 300,000-topic call (4,688 tiles: the split tile scan and its sums
    mode) of 40 distinct topics, deep ones among them."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    idx = ctx.build_index(base.filters)
    rng = random.Random(47)
    distinct = base.pool[:40]
    topics = [distinct[rng.randrange(40)] for _ in range(300_000)]
    _check(ctx, orc, idx, base, topics, how="device", modes=(True,), what="300k")
    idx.release()


# ------------------------------------------------------------------ rows that leave a pass for capacity
NARROW = b"$n/b/c/d/e/f/g/h"

def _overflow_case():
    lv = [b"a", b"b", b"c", b"d", b"e", b"f"]
    filters = set()
    for m in range(1 << 6):  # the filters of test_overflow_slow_path
        ws = [b"+" if (m >> i) & 1 else lv[i] for i in range(6)]
        filters.add(b"/".join(ws))
        filters.add(b"/".join(ws[:3]) + b"/#")
        filters.add(b"/".join(ws[:5]) + b"/#")
    deep1 = b"$t/0/1/2/3/4/5/6/7/8"  # a 10-level topic with one match: listed, never slow
    filters.add(deep1)
    # a narrow heavy topic: 17 matches along two paths (frontier 2), so the main and the listed
    # pass both walk it to its end before its row turns out too long
    path = NARROW.split(b"/")
    for alt in (path, path[:1] + [b"+"] + path[2:]):
        filters.add(b"/".join(alt))
        filters.update(b"/".join(alt[:k]) + b"/#" for k in range(1 if alt is path else 2, 9))
    ref = R.Ref(filters)
    heavy = [b"a/b/c/d/e/f", b"a/x/c/d/e/f", b"q/b/c/d/e/f", b"a/b/c/d/e/f/g", b"a/b/c/d/e"]
    light = [b"x/y/z", b"a/x", b"x", b"$q/b/c", b"x/y/z/w/v/u", b"a/+", b"", b"x/y/z/w/v/u/t/s"]
    deep = [deep1, b"$t/0/1/2/3/4/5/6/7/9", b"$t/0/1/2/3/4/5/6/7/8/9"]
    assert all(len(ref.walk(t)[1]) > 16 for t in heavy + [NARROW])  # past FAST_MC: only the slow path can finish them
    assert ref.walk(NARROW)[3] == 2 and len(ref.walk(NARROW)[1]) == 17
    assert ref.max_row(light + deep) <= MAX_ROW and ref.max_frontier(light + deep) <= MAX_FRONTIER
    assert len(ref.walk(deep1)[1]) == 1
    rng = random.Random(53)
    tiles = []
    for kind in (light, heavy, deep, heavy, light, light, deep, heavy, light):  # 64-aligned, never mixed
        tiles.append([rng.choice(kind) for _ in range(64)])
    tiles.append([rng.choice(heavy) for _ in range(37)])  # a partial last tile
    return ref, tiles, set(heavy) | {NARROW}


@pytest.mark.parametrize("main", ["fused", "fused_columns"])
def test_overflow_rows_bounds_and_slow_count(ctx, orc, main, monkeypatch):
    """Tiles of light topics beside tiles of topics with more than 16 matches
    (past FAST_MC: the main and the listed pass give them up, the slow path
    finishes them) and tiles of 10-level single-match topics (listed, never
    slow).  The contract: the light and listed rows are counted exactly once, a
    row that leaves a pass for capacity by at most two passes --
        sum P(light) <= probes <= sum P(light) + 2 sum P(heavy)
    -- and n_overflow is the rows the slow path completed: the heavy ones.

    Measured on an MI355X, this batch (613 topics, sum P(light) = 6,760, sum
    P(heavy) = 54,264): probes = 55,865 with the fused main pass.  (The
    since-removed split walk, which zeroed the count of a topic it gave up,
    measured 37,477; the 18,388 between them are what coop_walk_tile keeps of
    the heavy rows: it accumulates per entry lane and cannot take a topic's
    count back.)  That is under sum P = 61,024: these wide rows are cut short
    in both passes."""
    if main == "fused_columns":
        monkeypatch.setenv("GM_STAGE_COMPACT", "0")
    ref, tiles, heavy = _overflow_case()
    topics = [t for tile in tiles for t in tile]
    idx = ctx.build_index(ref.filters)
    for how in ("host", "device"):
        for exact in (True, False):
            ro, ids = _call(ctx, idx, topics, exact, how)
            oro, oids = _oracle_rows(orc, ref.filters, topics, 1 if exact else 0)
            assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
            st = ctx.stats()
            p_light = sum(ref.walk(t)[0] for t in topics if t not in heavy)
            p_heavy = sum(ref.walk(t)[0] for t in topics if t in heavy)
            print(f"overflow rows [{main} {how} exact={exact}]: probes={st['probes']} P_ref={p_light + p_heavy} "
                  f"P_light={p_light} P_heavy={p_heavy} n_overflow={st['n_overflow']}")
            assert p_light <= st["probes"] <= p_light + 2 * p_heavy
            assert st["n_overflow"] == sum(1 for t in topics if t in heavy)
            assert st["n_wildcard_topics"] == sum(1 for t in topics if R.is_wildcard(t))
    idx.release()


@pytest.mark.parametrize("main", ["fused"])
def test_overflow_narrow_rows_counted_by_up_to_two_passes(ctx, orc, main):
    """The upper bound is reached: a topic with 17 matches and a frontier of 2
    is walked to its end by the main pass and again by the listed pass before
    the slow path finishes it.  Measured on an MI355X: sum P(light) = 2,679, sum
    P(heavy) = 3,478; the fused main pass gives probes = 9,635 = 2,679 + 2 x
    3,478 (more than sum P = 6,157).  (The since-removed split walk gave
    6,157: the listed pass alone counted a topic that walk gave up.)"""
    ref, tiles, heavy = _overflow_case()
    topics = tiles[0] + [NARROW] * 64 + tiles[2] + [NARROW] * 10
    idx = ctx.build_index(ref.filters)
    for how in ("host", "device"):
        ro, ids = _call(ctx, idx, topics, True, how)
        oro, oids = _oracle_rows(orc, ref.filters, topics, 1)
        assert np.array_equal(ro, oro) and np.array_equal(ids, oids)
        st = ctx.stats()
        p_light = sum(ref.walk(t)[0] for t in topics if t != NARROW)
        p_heavy = 74 * ref.walk(NARROW)[0]
        print(f"narrow overflow rows [{main} {how}]: probes={st['probes']} P_ref={p_light + p_heavy} "
              f"P_light={p_light} P_heavy={p_heavy} n_overflow={st['n_overflow']}")
        assert p_light <= st["probes"] <= p_light + 2 * p_heavy
        assert st["n_overflow"] == 74
    idx.release()
