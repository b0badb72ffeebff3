"""k_match_fused's table addressing (gm_match.hip TabRef): buffer resources of
each table's real byte size, loads predicated by the hardware range check, the
default instantiation without the A/B forms and the flat instantiation.

Every row is compared with the CPU oracle, in both `exact` modes: a wrong
descriptor size or predicate shows up as missing or extra matches."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("GM_HOT_FLAT", "GM_STAGE_SC1", "GM_HOT_POLICY", "GM_L1_BYPASS", "GM_D0", "GM_MPH_MIN_KEYS", "GM_NO_MPH")


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _filters(orc, seed, n, wild_only):
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(seed, n, wildcard_only=wild_only)
    return codes, sorted(set(orc.unpack(*render_codes(codes))))


def _derived(orc, codes, seed, n):
    return orc.unpack(*orc.render_codes(orc.gen_topic_codes(seed, 0, n, codes)))


def _oracle(orc, filters, topics, exact):
    from tests.test_gpu_parity import _oracle_rows
    return _oracle_rows(orc, sorted(filters), topics, 1 if exact else 0)


def _assert_rows(got, want, topics, what):
    (ro, ids), (oro, oids) = got, want
    if np.array_equal(ro, oro) and np.array_equal(ids, oids):
        return
    for i in range(len(topics)):
        g, e = ids[ro[i]:ro[i + 1]].tolist(), oids[oro[i]:oro[i + 1]].tolist()
        assert g == e, (what, i, topics[i], g, e)
    raise AssertionError((what, "row offsets differ"))


# the index forms: (name, filters, wildcard-only, knobs at build)
FORMS = [
    ("mixed", 2000, False, {}),
    ("wildcard", 2000, True, {}),
    ("small-no-mph", 300, False, {}),                       # < 4k depth-2 keys and no filtered table: open addressing
    ("mixed-all-mph", 2000, False, {"GM_MPH_MIN_KEYS": "1"}),  # every per-depth table hash-and-displace placed
    ("wildcard-no-mph", 2000, True, {"GM_NO_MPH": "1"}),    # open addressing + exact-edge filters
]


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def world(request, ctx, orc):
    """One index form, its 1,000 edge-case topics (probing and non-probing lanes
    in every 64-topic tile) and the oracle's rows for them, computed once."""
    import os
    name, nf, wild_only, knobs = request.param
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(knobs)
    try:
        codes, filters = _filters(orc, 11, nf, wild_only)
        idx = ctx.build_index(filters)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    topics = _edge_topics(orc, codes, 1000)
    want = {ex: _oracle(orc, filters, topics, ex) for ex in (True, False)}
    yield idx, filters, codes, topics, want
    idx.release()


def _edge_topics(orc, codes, n):
    """n topics: derived (matching) topics interleaved 1:1 with lanes that must
    not probe somewhere -- a word absent from the dictionary at one level or at
    all of them, empty words, '$' topics, wildcard publish topics, deep topics."""
    rng = random.Random(5)
    real = _derived(orc, codes, 3, n)
    out = []
    for i, t in enumerate(real):
        if i % 2 == 0:
            out.append(t)
            continue
        ws = t.split(b"/")
        k = (i // 2) % 12
        if k < 5:      # an absent word at level k (or the last level)
            ws[min(k, len(ws) - 1)] = b"zzq%d" % i
        elif k == 5:   # absent at every level
            ws = [b"nope%d" % j for j in range(len(ws))]
        elif k == 6:   # empty words: inside, leading, trailing, the empty topic
            ws = [[b"a", b"", b"b"], [b""] + ws, ws + [b""], [b""]][(i // 24) % 4]
        elif k == 7:   # '$' topics
            ws = [b"$SYS"] + ws if (i // 24) % 2 else [b"$" + ws[0]] + ws[1:]
        elif k == 8:   # wildcard publish topics: the literal route only
            ws = [ws[:1] + [b"+"], [b"#"], [b"+"] + ws[1:] + [b"#"], ws + [b"+"]][(i // 24) % 4]
        elif k == 9:   # deep: 9 levels and more (the listed pass)
            ws = (ws * 9)[:9 + (i // 24) % 4]
        elif k == 10:  # a word longer than the dictionary's 8-byte head
            ws[rng.randrange(len(ws))] = b"long-word-over-8-bytes"
        else:          # one level only
            ws = ws[:1]
        out.append(b"/".join(ws))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tile_and_block_edges(ctx, orc, world, n):
    """Batches that end inside a tile, at a tile edge and at a block edge; the
    lanes past the batch and the lanes that do not probe read nothing."""
    idx, filters, codes, topics, want = world
    for exact in (True, False):
        ro, ids = ctx.match(idx, topics[:n], exact=exact)
        oro, oids = want[exact]
        _assert_rows((ro, ids), (oro[:n + 1], oids[:int(oro[n])]), topics[:n], (n, exact))


def test_non_probing_lanes_every_level(ctx, orc, world):
    """Absent words level by level over the SAME matching topic, so the lanes of
    a tile stop probing at different levels; plus the whole edge-case list."""
    idx, filters, codes, topics, want = world
    real = _derived(orc, codes, 9, 64)
    batch = []
    for t in real:
        ws = t.split(b"/")
        batch.append(t)
        for lv in range(len(ws)):
            batch.append(b"/".join(ws[:lv] + [b"absent"] + ws[lv + 1:]))
            batch.append(b"/".join(ws[:lv] + [b""] + ws[lv + 1:]))
    for exact in (True, False):
        _assert_rows(ctx.match(idx, batch, exact=exact), _oracle(orc, filters, batch, exact), batch, exact)


@pytest.fixture(scope="module")
def big(ctx, orc):
    """A 2,000-filter wildcard index and a 20,000-topic batch with its oracle rows."""
    codes, filters = _filters(orc, 4, 2000, True)
    idx = ctx.build_index(filters)
    topics = _derived(orc, codes, 8, 19_000) + _edge_topics(orc, codes, 1000)
    want = {ex: _oracle(orc, filters, topics, ex) for ex in (True, False)}
    yield idx, filters, topics, want
    idx.release()


def test_buffer_and_flat_forms_agree(ctx, orc, big, monkeypatch):
    """The default (buffer) instantiation and the flat one, forced per call by
    GM_HOT_FLAT, give the same CSR (and the oracle's)."""
    idx, filters, topics, want = big
    for exact in (True, False):
        monkeypatch.delenv("GM_HOT_FLAT", raising=False)
        buf = ctx.match(idx, topics, exact=exact)
        monkeypatch.setenv("GM_HOT_FLAT", "1")
        flat = ctx.match(idx, topics, exact=exact)
        monkeypatch.delenv("GM_HOT_FLAT", raising=False)
        assert np.array_equal(buf[0], flat[0]) and np.array_equal(buf[1], flat[1])
        _assert_rows(buf, want[exact], topics, exact)


@pytest.mark.parametrize("knobs", [{"GM_STAGE_SC1": "1"}, {"GM_HOT_POLICY": "1", "GM_L1_BYPASS": "0xffff"},
                                   {"GM_D0": "0"}], ids=["stage-sc1", "hot-policy", "no-d0"])
def test_instantiation_choice(ctx, orc, big, monkeypatch, knobs):
    """A call whose knobs ask for an A/B form runs the general instantiation;
    its rows equal the default instantiation's."""
    idx, filters, topics, want = big
    for exact in (True, False):
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        default = ctx.match(idx, topics, exact=exact)
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        ab = ctx.match(idx, topics, exact=exact)
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        assert np.array_equal(default[0], ab[0]) and np.array_equal(default[1], ab[1])
        _assert_rows(default, want[exact], topics, exact)


def test_descriptors_after_in_place_update(ctx, orc, monkeypatch):
    """The per-level descriptors follow an in-place update: 300 ops (24 new
    filters, the rest deletes) patched into hash-and-displace tables (inserted
    keys go to the tables' overflow regions, IndexView::mph_ovf), then a delta past the tables' headroom (the rebuild
    path, larger tables).  4,096 topics after each, derived from the filters of
    both updates."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    monkeypatch.setenv("GM_MPH_MIN_KEYS", "1")
    monkeypatch.delenv("GM_UPDATE_OVERLAY", raising=False)
    codes, filters = _filters(orc, 21, 2000, False)
    current = set(filters)
    idx = ctx.build_index(filters)
    rng = random.Random(3)
    # (an MPH table's overflow region takes max(64, keys / 16) / 2 keys: a few
    # new filters, whose keys collide in the ~0.94-full perfect-hash regions)
    c1 = gen_filter_codes(22, 24)
    c2 = gen_filter_codes(23, 9000)
    topics = (_derived(orc, codes, 1, 2048) + _derived(orc, c1, 2, 1024) + _derived(orc, c2, 3, 1024))
    assert len(topics) == 4096
    ins1 = sorted(set(orc.unpack(*render_codes(c1))) - current)
    ops1 = [(f, True) for f in ins1] + [(f, False) for f in rng.sample(filters, 300 - len(ins1))]
    assert len(ops1) == 300
    ops2 = [(f, True) for f in orc.unpack(*render_codes(c2))]
    for ops, kind in ((ops1, "patch"), (ops2, "rebuild")):
        for f, ins in ops:
            (current.add if ins else current.discard)(f)
        new = ctx.update_index(idx, ops)
        assert ctx.update_stats()["kind"] == kind
        for exact in (True, False):
            _assert_rows(ctx.match(new, topics, exact=exact), _oracle(orc, current, topics, exact), topics,
                         (kind, exact))
        idx.release()
        idx = new
    idx.release()
