"""The plain probe-count reference (tests/_nfa_ref.py) checked on its own: hand
counts of P, and its matches against the CPU oracle's
rows in both match modes, so the reference is tied to the oracle before the
GPU's counters are tied to it (tests/test_gpu_probe_count.py)."""

import random

import numpy as np

from tests import _nfa_ref as R


def test_worked_example():
    p, m, wild = R.walk(["#", "a/+", "a/b"], "a/b")
    assert (p, m, wild) == (1 + 3 + 3 + 2 * 2, [b"#", b"a/+", b"a/b"], False)


def test_hand_counts():
    # a '$' topic: the root's '+' and '#' children are not followed (1 + 3 + 3 + 2)
    f = ["#", "+/x", "$SYS/#", "$SYS/x", "+/#"]
    assert R.walk(f, "$SYS/x") == (9, [b"$SYS/#", b"$SYS/x"], False)
    # ... but an inner '+' is (level 1: $SYS/x and $SYS/+ both reached)
    assert R.walk(f + ["$SYS/+"], "$SYS/x") == (1 + 3 + 3 + 2 * 2, [b"$SYS/#", b"$SYS/+", b"$SYS/x"], False)
    # a '$' one-word topic: only the exact child
    assert R.walk(["+", "$x", "#"], "$x") == (1 + 3 + 2, [b"$x"], False)
    # the frontier dies at level 0, at level 1, and survives to the end without a filter there
    assert R.walk(["a/b/c"], "x/y/z") == (1 + 3, [], False)
    assert R.walk(["a/b/c"], "a/x/c") == (1 + 3 + 3, [], False)
    assert R.walk(["a/b/c"], "a/b") == (1 + 3 + 3 + 2, [], False)
    assert R.walk(["a/b/c"], "a/b/c/d") == (1 + 3 + 3 + 3 + 3, [], False)
    # two live paths: a and + at level 0, then b under each
    assert R.walk(["a/b", "+/b", "a/#"], "a/b") == (1 + 3 + 3 * 2 + 2 * 2, [b"+/b", b"a/#", b"a/b"], False)
    # the empty topic is one empty word; the empty word is a word like any other
    assert R.walk(["", "+", "#", "/a"], "") == (1 + 3 + 2 * 2, [b"", b"#", b"+"], False)
    assert R.walk(["", "+", "#", "/a", "/+"], "/a") == (1 + 3 + 3 * 2 + 2 * 2, [b"#", b"/+", b"/a"], False)
    assert R.walk([], "a") == (1 + 3, [], False)
    # a wildcard publish topic: no walk, the literal route only
    assert R.walk(["a/+", "#"], "a/+") == (0, [b"a/+"], True)
    assert R.walk(["a/+", "#"], "a/#") == (0, [], True)
    assert R.walk(["a/+", "#"], "a/b/+/c") == (0, [], True)
    assert R.trie_subset([b"a/+"], b"a/+") == []
    assert R.trie_subset([b"$x"], b"$x") == [b"$x"]
    assert R.trie_subset([b"a", b"+"], b"a") == [b"+"]


def test_batch_memoises_and_sums():
    f = ["#", "a/+", "a/b"]
    tot, wild, per = R.batch(f, ["a/b", "a/+", "x", "a/b"] * 1000)
    assert per[:4] == [11, 0, 1 + 3 + 2 * 0, 11] and tot == 1000 * 26 and wild == 1000
    ref = R.Ref(f)
    ref.batch(["a/b"] * 10)
    assert list(ref._memo) == [b"a/b"]
    assert ref.max_row(["a/b", "x"]) == 3 and ref.max_frontier(["a/b", "x"]) == 2


def _vs_oracle(orc, filters, topics):
    filters = sorted({f.encode() for f in filters})
    topics = [t.encode() for t in topics]
    ref = R.Ref(filters)
    for exact in (True, False):
        r = orc.Router(True)
        for f in filters:
            if exact:
                r.add_route(f)
            else:
                r.trie.insert(f)
        oro, oids, _ = r.match_batch(topics, filters, mode=1 if exact else 0)
        rows = ref.rows(topics, exact)
        assert np.array_equal(oro, np.concatenate([[0], np.cumsum([len(x) for x in rows])]))
        for i, row in enumerate(rows):
            assert row == oids[oro[i]:oro[i + 1]].tolist(), (exact, topics[i])


def test_matches_equal_oracle_random_sets(orc):
    from tests.test_gpu_parity import _rand_filter, _rand_topic
    rng = random.Random(11)  # the sets of test_random_small_sets
    for _ in range(40):
        filters = [_rand_filter(rng) for _ in range(rng.randint(1, 60))]
        topics = [_rand_topic(rng) for _ in range(300)]
        _vs_oracle(orc, filters, topics)


def test_matches_equal_oracle_chain_sets(orc):
    from tests.test_gpu_parity import CHAIN_FILTERS, CHAIN_TOPICS
    _vs_oracle(orc, CHAIN_FILTERS, CHAIN_TOPICS + [t + "/x" for t in CHAIN_TOPICS])
