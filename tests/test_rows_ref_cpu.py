"""The references of tests/_rows_ref.py against independent ones (the oracle's
fan-out, a per-row sorted()), and the coverage ledger: the case list that
tests/test_gpu_rows.py runs on the device reaches every boundary of the row
consumers (gm_csr.hip) and of the scan under them (gm_scan.h).  The ledger is
the argument that the device tests would notice a kernel that is wrong at one
of these boundaries; a case list that misses one is extended, the ledger is
not relaxed."""

import numpy as np
import pytest

from tests import _rows_ref as R


@pytest.fixture(scope="module")
def world():
    perm = R.host_perm()
    return (perm,) + R.world_csr(perm)


def test_world_lists_are_distinct_and_not_ascending():
    flat = [x for lst in R.LISTS for x in lst]
    assert len(set(flat)) == len(flat) == sum(R.LENGTHS)
    assert all(lst != sorted(lst) for lst in R.LISTS if len(lst) > 1)
    assert [len(lst) for lst in R.LISTS] == R.LENGTHS


@pytest.mark.parametrize("name", R.FAN_CASES)
def test_fanout_ref_equals_the_oracle(orc, world, name):
    perm, so, si = world
    case = R.fan_case(name)
    ids = case.ids(perm)
    got = R.fanout_ref(case.m_off, ids, so, si)
    want = orc.fanout(case.m_off, ids, so, si)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(got[1]) == case.total and got[0].dtype == np.uint64 and got[1].dtype == np.uint32


def test_fanout_ref_through_a_shuffled_perm(orc):
    """Filter ids that are not the filters' input order: the world's lists follow the ids."""
    perm = np.random.RandomState(4).permutation(len(R.LENGTHS)).astype(np.uint32)
    so, si = R.world_csr(perm)
    case = R.fan_case("pairs_3")
    got = R.fanout_ref(case.m_off, case.ids(perm), so, si)
    want = orc.fanout(case.m_off, case.ids(perm), so, si)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    base = R.fanout_ref(case.m_off, case.ids(R.host_perm()), *R.world_csr(R.host_perm()))
    assert np.array_equal(got[1], base[1])  # (the deliveries do not depend on how the ids are numbered)


@pytest.mark.parametrize("name,n_parts", R.PART_CASES)
def test_fanout_part_ref_tiles_the_whole(world, name, n_parts):
    perm, so, si = world
    case = R.fan_case(name)
    whole = R.fanout_ref(case.m_off, case.ids(perm), so, si)
    pos, got = 0, []
    for p in range(n_parts):
        first, ids = R.fanout_part_ref(case.m_off, case.ids(perm), so, si, p, n_parts, whole=whole)
        assert first == pos == case.total * p // n_parts
        pos += len(ids)
        got.append(ids)
    assert pos == case.total and np.array_equal(np.concatenate(got), whole[1])


def test_part_range_uses_python_integers():
    big = (1 << 63) + 12345  # total * part passes 2^64
    assert R.part_range(big, 6, 7) == (big * 6 // 7, big)
    assert R.part_range(np.uint64(1 << 62), np.uint32(7), np.uint32(8)) == ((1 << 62) * 7 // 8, 1 << 62)


@pytest.mark.parametrize("n,stride,pieces", R.MERGE_WORLDS)
def test_merge_rows_ref_equals_sorted(n, stride, pieces):
    w = R.merge_world(n, stride, pieces)
    ro, ids = R.merge_rows_ref(w.lens, w.ids, n)
    rows = [sorted(int(x) for p in range(pieces) for x in w.lists[p][t]) for t in range(n)]
    assert ro.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64).tolist()
    assert ids.tolist() == [x for r in rows for x in r]
    assert np.array_equal(R.row_lengths_ref(ro), np.array([len(r) for r in rows], np.uint32))
    # the world keeps the kernel's contract: sorted, disjoint lists; padding rows of length 0
    for t in range(n):
        assert all(np.all(np.diff(w.lists[p][t]) > 0) for p in range(pieces))
        assert len(set(rows[t])) == len(rows[t])
    assert w.lens.shape == (pieces, stride) and not w.lens[:, n:].any()
    assert len(w.ids) == int(w.lens.sum())


# ------------------------------------------------------------------ the coverage ledger
def test_scan_form_boundaries():
    """The forms at the sizes the sources state: one launch up to 4,095 inputs (4,096 outputs), three
    launches up to 4,095 blocks of 1,024 outputs, a three-launch scan of the block sums past that;
    k_scan_loop for the small driver up to 32,767."""
    assert [R.scan_form(n) for n in (0, 4095, 4096, 4_193_279, 4_193_280)] == \
        ["one", "one", "three", "three", "recursive"]
    assert [R.scan_form_small(n) for n in (0, 4095, 4096, 32767, 32768)] == ["loop", "loop", "loop", "loop", "three"]
    assert [R.fan_per_block(t) for t in (0, 1, 2_097_152, 2_099_199, 2_099_200, 1 << 40)] == \
        [1024, 1024, 1024, 1024, 2048, 65536]


@pytest.fixture(scope="module")
def ledger():
    whole = {name: R.classify(R.fan_case(name)) for name in R.FAN_CASES}
    parts = {(name, n, p): R.classify(R.fan_case(name), p, n) for name, n in R.PART_CASES for p in range(n)}
    return whole, parts


def _union(ledger_items, key):
    out = set()
    for c in ledger_items:
        if c is not None:
            out |= c["launch"][key]
    return out


def test_ledger_scan_forms(ledger):
    whole, _ = ledger
    # the ordinary driver (run_fanout: GM_FANOUT_SIMPLE host rows, device rows) takes every form of
    # scan_excl, at the two entry counts on either side of each change
    form = {n: {whole["scan_%d_%s" % (n, r)]["scan"] for r in ("one", "cut")} for n in R.SCAN_NNZ}
    assert form[4095] == {"one"} and form[4096] == {"three"}
    assert form[4_193_279] == {"three"} and form[4_193_280] == {"recursive"}
    assert form[0] == form[1] == {"one"}
    # ... and the block count of the three-launch form on either side of a whole block (5 and 6 blocks)
    assert [(n + 1 + R.SCAN_B - 1) // R.SCAN_B for n in (5119, 5120)] == [5, 6]
    # the small driver (queue_fanout_small): k_scan_loop up to 32,767 entries, scan_excl past it;
    # the loop's chunk count on either side of one chunk (4,095 / 4,096) and at its last chunk
    small = {n: {whole["scan_%d_%s" % (n, r)]["small"]["scan"] for r in ("one", "cut")}
             for n in R.SCAN_NNZ if n not in R.BIG_NNZ}
    assert small[32766] == small[32767] == {"loop"} and small[32768] == {"three"}
    assert small[4095] == small[4096] == small[4097] == {"loop"}
    # the four forms between the two drivers
    assert {c["scan"] for c in whole.values()} | {c["small"]["scan"] for c in whole.values() if c["small"]} == \
        {"one", "loop", "three", "recursive"}
    # by design on the ordinary path whatever the knob: 65,536 rows
    assert whole["scan_4097_wide"]["small"] is None and whole["scan_4097_wide"]["n_rows"] == 65536
    assert whole["scan_4097_wide"]["scan"] == "three"
    assert all(whole[n]["n_rows"] < 65536 for n in R.FAN_CASES if n != "scan_4097_wide")
    # the two largest lists are single-row and cut-into-rows alike, ~4M deliveries each
    for n in R.BIG_CASES:
        assert 3_900_000 < whole[n]["total"] < 4_500_000


def test_ledger_empty_segment_runs(ledger):
    whole, parts = ledger
    for run in (1, 2, 300):
        c = whole["empties_%d" % run]
        assert c["launch"]["empties"] == {"start", "end", "before_boundary", "after_boundary"}
        assert c["small"]["launch"]["empties"] == {"start", "end", "before_boundary", "after_boundary"}
        assert c["total"] == 2048 and c["launch"]["n_ranges"] == 2
    c = whole["empties_only"]
    assert c["total"] == 0 and c["nnz"] == 7 and c["n_rows"] > 1 and c["launch"]["n_ranges"] == 0
    # the random lists have them too (two in five entries are of the zero-length filter)
    assert "start" in _union(whole.values(), "empties") and "end" in _union(whole.values(), "empties")


def test_ledger_copy_paths(ledger):
    whole, parts = ledger
    pairs = [whole["pairs_%d" % k] for k in range(4)]
    # the k prefix moves every later segment start through the residues mod 4
    assert [(c["total"] - pairs[0]["total"]) % 4 for c in pairs] == [0, 1, 2, 3]
    # single-segment (hoisted) ranges with every tail, on both drivers
    assert _union(pairs, "single_tails") == {0, 1, 2, 3}
    assert _union([c["small"] for c in pairs], "single_tails") == {0, 1, 2, 3}
    # a 4-element group across a segment start at every residue; across the end of the deliveries
    for c in pairs:
        assert c["launch"]["cross_seg"] == {1, 2, 3} and c["small"]["launch"]["cross_seg"] == {1, 2, 3}
        assert c["launch"]["n_ranges"] > 180
    assert whole["tiny"]["launch"]["cross_end"] == {1} and whole["tiny"]["total"] == 5
    assert _union(whole.values(), "cross_end") == {1, 2, 3}
    # workgroup ranges of 1,024 and of 2,048 deliveries
    assert pairs[0]["launch"]["per_block"] == 1024
    assert whole["wide"]["launch"]["per_block"] == 2048 and whole["wide"]["total"] > 2_097_152
    assert whole["wide"]["small"]["launch"]["per_block"] == 2048  # (its capacity is 4M deliveries)
    assert {c["small"]["launch"]["per_block"] for c in pairs} == {1024}
    # past the small driver's 16M deliveries: no case (the ordinary path by design, see test_gpu_rows)
    assert all(c["small"] is not None for n, c in whole.items() if n not in R.BIG_CASES + ["scan_4097_wide"])


def test_ledger_part_cuts(ledger):
    _, parts = ledger
    cut = [c["cut"] for (name, n, p), c in parts.items() if p > 0]
    assert {c["glo_mod"] for c in cut if not c["empty_part"]} == {0, 1, 2, 3}
    assert any(c["on_seg_start"] and c["empties_at_cut"] for c in cut)
    assert any(not c["on_seg_start"] for c in cut)
    # a cut through a single-segment range leaves it a tail; a part of the wide case keeps 1,024 per workgroup
    assert _union([c for k, c in parts.items() if k[0] == "pairs_1"], "single_tails") == {0, 1, 2, 3}
    assert {c["launch"]["per_block"] for k, c in parts.items() if k[0] == "wide"} == {1024, 2048}
    # empty parts: more parts than deliveries, and a fan-out of no deliveries at all
    tiny = [c for k, c in parts.items() if k[0] == "tiny"]
    assert len(tiny) == 8 and sum(c["cut"]["empty_part"] for c in tiny) == 3
    assert {c["cut"]["glo_mod"] for c in tiny} == {0, 1, 2, 3}
    assert all(c["cut"]["empty_part"] for k, c in parts.items() if k[0] == "empties_only")
    # the cut at delivery 1,024 of 2,048: a segment start with the run of zero-length segments before it
    for run in (1, 2, 300):
        c = parts[("empties_%d" % run, 2, 1)]
        assert c["cut"]["on_seg_start"] and c["cut"]["empties_at_cut"] and c["launch"]["empties"] >= {"after_boundary"}
        assert parts[("empties_%d" % run, 2, 0)]["launch"]["empties"] == {"start", "before_boundary"}


def test_ledger_merge_worlds():
    cl = {w: R.merge_world(*w).classify() for w in R.MERGE_WORLDS}
    # P * stride on either side of the one-launch scan's 4,095 inputs; n likewise
    assert cl[(1365, 1365, 3)]["n_lists"] == 4095 and cl[(1365, 1365, 3)]["scan_lists"] == "one"
    assert cl[(2048, 2048, 2)]["n_lists"] == 4096 and cl[(2048, 2048, 2)]["scan_lists"] == "three"
    assert cl[(4097, 4097, 1)]["scan_rows"] == "three" and cl[(2048, 2048, 2)]["scan_rows"] == "one"
    assert {c["scan_lists"] for c in cl.values()} == {"one", "three"}
    # one piece, stride > n, no rows at all, rows on either side of one workgroup of 256 threads
    assert {w[2] for w in R.MERGE_WORLDS} == {1, 2, 3, 8}
    assert all(cl[(256, 259, p)]["padded"] for p in (1, 2, 3, 8))
    assert [cl[(n, n, 2)]["blocks"] for n in (0, 1, 255, 257)] == [0, 1, 1, 2] and cl[(256, 259, 2)]["blocks"] == 1
    for w, c in cl.items():
        if w[0] >= 255:
            assert c["shapes"] >= {"empty", "only", "round_robin", "blocks", "ends"}, w
        if w[0] == 257:
            assert "long" in c["shapes"]
            long_row = sum(len(R.merge_world(*w).lists[p][128]) for p in range(w[2]))
            assert long_row == R.LONG_ROW
    # every piece is in turn the only non-empty one
    w = R.merge_world(255, 255, 8)
    assert {s for s in w.shapes if s.startswith("only_")} == {"only_%d" % p for p in range(8)}
    ends = [t for t, s in enumerate(w.shapes) if s == "ends"]
    got = np.concatenate([w.lists[p][ends[0]] for p in range(8)])
    assert got.min() == 0 and got.max() == 0xFFFFFFFF
