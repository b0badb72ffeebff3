"""The retained-message lookup on the device (emqx_gm_retained_*,
emqx_amd/csrc/gm_retained.hip) against the Python restatement of the
reference's condition/1 + expiry rule (tests/_retained_ref.py) and the host walk
over the same tables.  Shapes sit where the walk's chunked descent can go
wrong: 63 / 64 / 65 / 129 siblings, two literal levels with more than 64
pending nodes each, rows around the wave width, a 40-level topic (the
global-workspace branch), batches around the block's four waves."""

import json
import os

import numpy as np
import pytest

from tests import _retained_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _rows(csr):
    ro, ids = csr
    assert len(ids) == int(ro[-1])
    return [[int(x) for x in ids[int(ro[i]):int(ro[i + 1])]] for i in range(len(ro) - 1)]


def _check(ctx, topics, filters, now_ms=0, ids=None, expiry_ms=None, want=None, lds=True):
    """Device rows == reference rows == host-walk rows; returns them."""
    ix = ctx.build_retained(topics, ids, expiry_ms)
    try:
        info = ix.info()
        assert bool(info.lds_frames) == lds and (info.walk_ws_bytes == 0) == lds and info.device_bytes > 0
        got = _rows(ix.match(filters, now_ms))
        host = _rows(ix.match_host(filters, now_ms))
    finally:
        ix.release()
    if want is None:
        want = R.match_rows(R.build_table(topics, ids, expiry_ms), filters, now_ms)
    for f, g, h, w in zip(filters, got, host, want):
        assert g == w, (f, len(g), len(w))
        assert h == w, f
    assert len(got) == len(filters)
    return got


# ------------------------------------------------------------------ reference parity
def test_golden_vectors(ctx):
    with open(os.path.join(ROOT, "tests", "golden", "retainer_vectors.json")) as f:
        cases = json.load(f)["cases"]
    t0 = 1_700_000_000_000
    for c in cases:
        topics = [t.encode() for t, _ in c["topics"]]
        expiry = [t0 + 1000 * s if s else 0 for _, s in c["topics"]]
        got = _check(ctx, topics, [f.encode() for f in c["filters"]], t0 + 1000 * c["at_s"], expiry_ms=expiry)
        assert [len(r) for r in got] == c["received"], c["name"]
        assert got == [[topics.index(t.encode()) for t in row] for row in c["rows"]], c["name"]


def test_edge_set(ctx):
    got = _check(ctx, R.EDGE_TOPICS, R.EDGE_FILTERS)
    by = dict(zip(R.EDGE_FILTERS, got))
    assert len(by[b"#"]) == len(R.EDGE_TOPICS) and by[b"#/a"] == [] and by[b"a/#"][0] == R.EDGE_TOPICS.index(b"a")


def test_random_set(ctx):
    topics, filters, expiry, ids, want = R.random_case(10)
    _check(ctx, topics, filters, 10, ids, expiry, want=want)


def test_empty_index_and_empty_batch(ctx):
    assert _check(ctx, [], [b"#", b"+", b"a", b""]) == [[], [], [], []]
    assert _check(ctx, R.EDGE_TOPICS, []) == []


# ------------------------------------------------------------------ the word lookup
# words on both sides of the dictionary slot's 8-byte head, and words that share a whole head
WORD_TOPICS = [b"w/" + b"k" * n for n in (0, 1, 7, 8, 9, 16, 17, 255)]
WORD_TOPICS += [b"prefix00-tailA/x", b"prefix00-tailB/x", b"prefix00/x"]
WORD_ABSENT = [b"w/" + b"k" * n for n in (2, 10, 254, 256)] + [b"prefix00-tailC/x", b"prefix00-tail/x"]
WORD_FILTERS = WORD_TOPICS + WORD_ABSENT + [b"prefix00-tailA/+", b"+/x", b"w/#"]


def test_word_lengths_and_equal_heads(ctx):
    """The device word lookup (dict_find, gm_device.h) in k_ret_walk and
    k_ret_expire: a literal filter finds its own topic and nothing else, a word
    one byte shorter or longer or with another tail finds nothing."""
    got = _check(ctx, WORD_TOPICS, WORD_FILTERS)
    for i, t in enumerate(WORD_TOPICS):
        assert got[i] == [i], t
    assert got[len(WORD_TOPICS):len(WORD_TOPICS) + len(WORD_ABSENT)] == [[]] * len(WORD_ABSENT)
    assert [len(r) for r in got[-3:]] == [1, 3, 8]
    # expire: one expiry per listed topic, so a hit on the wrong topic would show
    listed = WORD_TOPICS[::-1] + WORD_ABSENT
    new = [1000 + k for k in range(len(listed))]
    stored = [t for t in listed if t in WORD_TOPICS]
    expiry = [dict(zip(listed, new))[t] for t in WORD_TOPICS]
    ix = ctx.build_retained(WORD_TOPICS)
    try:
        assert ix.expire(listed, new) == len(stored) == len(WORD_TOPICS)
        table = R.build_table(WORD_TOPICS, None, expiry)
        for now in (999, 1000 + len(stored) // 2, max(new)):
            want = R.match_rows(table, WORD_FILTERS, now)
            assert _rows(ix.match(WORD_FILTERS, now)) == want, now
            assert _rows(ix.match_host(WORD_FILTERS, now)) == want, now
        dropped = {i for i, e in enumerate(expiry) if e <= 1000 + len(stored) // 2}
        assert 0 < len(dropped) < len(stored)
        assert _rows(ix.match([b"#"], 1000 + len(stored) // 2))[0] == sorted(
            set(range(len(WORD_TOPICS))) - dropped, key=lambda i: WORD_TOPICS[i].split(b"/"))
        assert _rows(ix.match(WORD_FILTERS, max(new))) == [[]] * len(WORD_FILTERS)
    finally:
        ix.release()


# ------------------------------------------------------------------ chunk boundaries
@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_sibling_counts_around_the_wave(ctx, k):
    topics = [b"w%03d/%s" % (i, c) for i in range(k) for c in (b"x", b"y")]
    got = _check(ctx, topics, [b"+/x", b"+/+", b"+/x/#", b"+/#", b"+/y", b"#"])
    assert [len(r) for r in got] == [k, 2 * k, k, 2 * k, k, 2 * k]


def test_two_literal_levels_past_64_pending(ctx):
    """'+/x/+/y' over 130 x 1 x 130 prefixes: the literal steps at levels 1 and
    3 each see more than 64 pending nodes, so several chunks are live at two
    levels at once."""
    topics = [b"p%03d/x/q%03d/%s" % (i, j, c) for i in range(130) for j in range(130) for c in (b"y",)]
    topics += [b"p%03d/x/q%03d/z" % (i, i) for i in range(130)] + [b"p%03d/u" % i for i in range(130)]
    got = _check(ctx, topics, [b"+/x/+/y", b"+/x/+/z", b"+/+/+/y", b"+/x/+/#", b"+/u", b"p007/x/+/y", b"+/x/q064/y"])
    assert [len(r) for r in got] == [16900, 130, 16900, 17030, 130, 130, 130]


def test_row_lengths_around_the_wave(ctx):
    topics = [b"g%d/%03d" % (k, i) for k in (1, 63, 64, 65) for i in range(k)]
    topics += [b"t/%04d" % i for i in range(5000 - len(topics))]
    filters = [b"g0/+", b"g1/+", b"g63/+", b"g64/#", b"g65/+", b"#", b"g63/#", b"g64/+", b"t/#"]
    got = _check(ctx, topics, filters)
    assert [len(r) for r in got] == [0, 1, 63, 64, 65, 5000, 63, 64, 5000 - 193]
    order = {i: tuple(t.split(b"/")) for i, t in enumerate(topics)}
    for row in got:  # ascending in topic order
        keys = [order[i] for i in row]
        assert keys == sorted(keys)


# ------------------------------------------------------------------ deep: the global-workspace branch
def test_deep_topic_uses_the_global_workspace(ctx):
    deep = b"/".join([b"w"] * 40)
    topics = [deep, b"w", b"w/w", b"x/y", b"/".join([b"w"] * 39) + b"/v"]
    plus40 = b"/".join([b"+"] * 40)
    filters = [plus40, b"/".join([b"+"] * 39) + b"/#", plus40 + b"/+", deep, deep + b"/#", b"#", b"+/+", b"w/#"]
    got = _check(ctx, topics, filters, lds=False)
    assert [len(r) for r in got] == [2, 2, 0, 1, 1, 5, 2, 4]
    # the same rows with chunks past 64 nodes in the workspace branch
    wide = [b"a%03d/%s" % (i, c) for i in range(130) for c in (b"x", b"y")] + [deep]
    got = _check(ctx, wide, [b"+/x", b"+/#", b"+/+", plus40], lds=False)
    assert [len(r) for r in got] == [130, 261, 260, 1]


# ------------------------------------------------------------------ batch sizes
def test_batch_sizes(ctx):
    topics, filters, expiry, ids, _ = R.random_case(10)
    ix = ctx.build_retained(topics, ids, expiry)
    try:
        base = filters[:65]
        single = [_rows(ix.match([f], 10))[0] for f in base]
        for n in (1, 63, 64, 65, 1000):
            batch = [base[i % 65] for i in range(n)]
            got = _rows(ix.match(batch, 10))
            assert got == [single[i % 65] for i in range(n)], n
    finally:
        ix.release()


# ------------------------------------------------------------------ expiry
def test_expiry_rule_and_expire_calls(ctx):
    now = 1_000_000
    topics = [b"e/never", b"e/past", b"e/now", b"e/future", b"f/x"]
    expiry = [0, now - 1, now, now + 1, 0]
    ix = ctx.build_retained(topics, expiry_ms=expiry)
    try:
        # expiry == now is expired: the rule is >
        assert _rows(ix.match([b"e/+", b"#", b"e/now"], now)) == [[3, 0], [3, 0, 4], []]
        assert _rows(ix.match([b"e/+"], now - 1)) == [[3, 0, 2]]
        assert _rows(ix.match([b"e/+"], 0)) == [[3, 0, 2, 1]]
        # expire: present and absent topics; the next match reflects it
        assert ix.expire([b"e/past", b"e/absent", b"f/x", b"e", b"e/past/deeper"], [0, 5, now, 5, 5]) == 2
        assert _rows(ix.match([b"#"], now)) == [[3, 0, 1]]
        assert _rows(ix.match_host([b"#"], now)) == [[3, 0, 1]]
        assert ix.expire([b"e/never"], 1) == 1  # a delete sets expiry 1
        assert _rows(ix.match([b"#"], now)) == [[3, 1]]
        assert _rows(ix.match([b"#"], 1)) == [[3, 2, 1, 4]]
        assert ix.expire([], 1) == 0
    finally:
        ix.release()


def test_index_without_expiries_skips_the_reads_until_one_is_set(ctx):
    topics = [b"n/%02d" % i for i in range(70)]
    ix = ctx.build_retained(topics)
    try:
        assert _rows(ix.match([b"n/#", b"n/+"], 10**15)) == [list(range(70))] * 2
        assert ix.expire([b"n/05", b"n/66"], 1) == 2
        left = [i for i in range(70) if i not in (5, 66)]
        assert _rows(ix.match([b"n/#", b"n/+", b"n/05"], 7)) == [left, left, []]
    finally:
        ix.release()


# ------------------------------------------------------------------ caller ids
def test_caller_ids_permutation_with_gaps(ctx):
    topics = [b"c/%03d" % i for i in range(200)] + [b"c"]
    rng = np.random.default_rng(3)
    ids = (rng.permutation(201).astype(np.uint32) * 7 + 1_000_000).tolist()
    got = _check(ctx, topics, [b"c/#", b"c/+", b"c/017", b"c"], ids=ids)
    assert got[0] == [ids[200]] + ids[:200] and got[2] == [ids[17]]


# ------------------------------------------------------------------ Retainer
def test_retainer_sequence(ctx):
    from emqx_amd import Retainer
    import random
    rng = random.Random(5)
    words = [b"a", b"b", b"c", b"d", b"", b"$SYS", b"e"]
    now = 10_000

    def topic(i):
        return b"%s/%s/n%d" % (words[i % 7], words[(i // 7) % 7], i)

    filters = [b"#", b"+/+/+", b"a/#", b"+/b/+", b"$SYS/#", b"a/b/n7", b"nope/#", b"+/+", b"a/+/n0", b"/+/#"]
    filters += [b"%s/%s/#" % (rng.choice(words), rng.choice(words)) for _ in range(20)]
    filters += [b"+/%s/+" % w for w in words] + [b"%s/+/n%d" % (words[i % 7], i) for i in range(0, 3500, 270)]
    filters = filters[:50]
    assert len(filters) == 50
    table = {}
    r = Retainer(ctx)

    def check():
        got = r.match_messages(filters, now)
        for f, row in zip(filters, got):
            want = sorted((tuple(t.split(b"/")), m) for t, (m, e) in table.items()
                          if R.matches(f, t) and R.alive(e, now))
            keys = [(tuple(t.split(b"/")), m) for t, m in row]
            assert sorted(keys) == want, f
            # the main part then the delta part, each in topic order
            assert sum(1 for a, b in zip(keys, keys[1:]) if b < a) <= 1, f
        assert r.size() == len(table)

    def store(t, m, e):
        r.store_retained(t, m, e)
        table[t] = (m, e)

    for i in range(2000):
        store(topic(i), "m%d" % i, rng.choice([0, 0, now - 5, now + 5]))
    check()
    before = r.compactions
    for i in range(2000, 3500):
        store(topic(i), "m%d" % i, rng.choice([0, now + 1]))
    assert r.compactions > before  # the delta crossed max(1024, main / 8)
    check()
    r.delete_message(b"a/b/#")
    r.delete_message(b"+//+")
    r.delete_message(topic(3))
    r.delete_message(b"not/stored")
    for t in [t for t in table if R.matches(b"a/b/#", t) or R.matches(b"+//+", t) or t == topic(3)]:
        del table[t]
    check()
    for i in (1, 3, 8, 2500, 3499):  # overwrite: live and deleted topics, main and delta
        store(topic(i), "again%d" % i, 0 if i % 2 else now + 100)
    store(topic(5), "expired", now - 1)
    check()
    assert r.read_message(topic(1)) == ["again1"] and r.read_message(b"not/stored") == []
    r.clean()
    table.clear()
    check()
    store(b"a/b/n7", "after clean", 0)
    check()
    r.clean()


# ------------------------------------------------------------------ coexistence
def test_filter_index_and_retained_index_on_one_context():
    """Interleaved emqx_gm_match and emqx_gm_retained_match on one context; the
    library's last error is kept per thread, so the sequence runs on a fresh
    thread and must leave it empty."""
    import threading
    from emqx_amd import Context, _lib
    result = {}

    def body():
        c = Context(0)
        filt = [b"a/+", b"a/#", b"b/c", b"+/c", b"#"]
        idx = c.build_index(filt)
        ret = c.build_retained([b"a/b", b"a/c", b"b/c", b"$SYS/c"])
        topics = [b"a/b", b"b/c", b"x"]
        first = _rows(c.match(idx, topics))
        for _ in range(3):
            assert _rows(ret.match([b"+/c", b"a/#", b"#"])) == [[3, 1, 2], [0, 1], [3, 0, 1, 2]]
            assert _rows(c.match(idx, topics)) == first
        assert ret.expire([b"a/c"], 1) == 1
        assert _rows(c.match(idx, topics)) == first
        assert _rows(ret.match([b"+/c"], 1)) == [[3, 2]]
        ret.release()
        idx.release()
        c.close()
        result["err"] = _lib.lib().emqx_gm_last_error(None)

    def run():
        try:
            body()
        except BaseException as e:  # noqa: BLE001 -- handed to the test's thread
            result["exc"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "exc" in result:
        raise result["exc"]
    assert result["err"] in (b"", None)
