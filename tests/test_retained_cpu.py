"""The retained-topic index on the host alone: the compiler
(emqx_amd/csrc/gm_retained.cpp) and the walk over its tables
(emqx_gm_retained_match_host) against the Python restatement of the reference's
condition/1 (tests/_retained_ref.py).  No device is needed."""

import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _retained_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(csr):
    ro, ids = csr
    return [[int(x) for x in ids[int(ro[i]):int(ro[i + 1])]] for i in range(len(ro) - 1)]


def _host_rows(topics, filters, now_ms=0, ids=None, expiry_ms=None):
    from emqx_amd import RetainedIndex
    ix = RetainedIndex.compile_host(topics, ids, expiry_ms)
    try:
        return _rows(ix.match_host(filters, now_ms))
    finally:
        ix.release()


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "retainer_vectors.json")) as f:
        cases = json.load(f)["cases"]
    out = []
    for c in cases:
        t0 = 1_700_000_000_000  # the publishes' instant in ms
        topics = [t.encode() for t, _ in c["topics"]]
        expiry = [t0 + 1000 * s if s else 0 for _, s in c["topics"]]
        out.append((c["name"], topics, expiry, [f.encode() for f in c["filters"]], t0 + 1000 * c["at_s"],
                    c["received"], [[topics.index(t.encode()) for t in row] for row in c["rows"]]))
    return out


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_golden_suite_vectors(case):
    _, topics, expiry, filters, now, received, rows = case
    got = _host_rows(topics, filters, now, expiry_ms=expiry)
    assert [len(r) for r in got] == received
    assert got == rows
    assert got == R.match_rows(R.build_table(topics, None, expiry), filters, now)


def test_edge_topics_and_filters():
    got = _host_rows(R.EDGE_TOPICS, R.EDGE_FILTERS)
    want = R.match_rows(R.build_table(R.EDGE_TOPICS), R.EDGE_FILTERS)
    for f, g, w in zip(R.EDGE_FILTERS, got, want):
        assert g == w, f
    by = dict(zip(R.EDGE_FILTERS, got))
    t = R.EDGE_TOPICS.index
    assert len(by[b"#"]) == len(R.EDGE_TOPICS)            # '$SYS/x' included: no '$'-rule
    assert by[b"a/#"][0] == t(b"a")                       # 'a/#' returns 'a' itself
    assert by[b"#/a"] == [] and by[b"a/#/#"] == []        # a '#' before the last word matches nothing
    assert by[b"a+"] == [t(b"a+")]                        # a literal
    assert by[b"unknown"] == [] and by[b"a/b/c/d"] == []  # an unknown word; one level deeper than any topic
    # byte order and word-list order at odds: 'a/b' before 'a!'
    assert by[b"#"].index(t(b"a/b")) < by[b"#"].index(t(b"a!"))
    # words sharing their first 8 bytes
    assert by[b"longword_0001/+"] == [t(b"longword_0001/x")]
    assert by[b"longword_0002/#"] == [t(b"longword_0002"), t(b"longword_0002/x")]
    assert by[b"longword_0003/#"] == []


def test_empty_batch_and_empty_index():
    assert _host_rows(R.EDGE_TOPICS, []) == []
    assert _host_rows([], [b"#", b"+", b"a", b""]) == [[], [], [], []]
    assert _host_rows([], []) == []


def test_duplicate_topics_last_one_wins():
    topics = [b"a/b", b"c", b"a/b", b"c", b"a/b"]
    ids = [10, 11, 12, 13, 14]
    expiry = [0, 5, 5, 0, 100]
    from emqx_amd import RetainedIndex
    ix = RetainedIndex.compile_host(topics, ids, expiry)
    assert ix.info().n_topics == 2
    assert _rows(ix.match_host([b"#"], 50)) == [[14, 13]]
    assert _rows(ix.match_host([b"#"], 100)) == [[13]]  # 100 > 100 is false: expired
    ix.release()


def test_index_shape():
    from emqx_amd import RetainedIndex
    ix = RetainedIndex.compile_host([b"a/b/c", b"a/b", b"a/x", b"d"])
    i = ix.info()
    # root + sentinel, then levels of 2, 2, 1 nodes each with a sentinel, then the empty level's sentinel
    assert (i.n_topics, i.depth_max, i.widest_level, i.n_words, i.n_nodes) == (4, 3, 2, 5, 2 + 3 + 3 + 2 + 1)
    assert i.device_bytes == 0 and i.lds_frames == 1
    deep = RetainedIndex.compile_host([b"/".join([b"w"] * 40)])
    assert deep.info().depth_max == 40 and deep.info().lds_frames == 0
    ix.release()
    deep.release()


def test_random_set_equals_reference():
    topics, filters, expiry, ids, want = R.random_case(10)  # (expiries 5 and 10 are past at 10, 11 and 50 are not)
    got = _host_rows(topics, filters, 10, ids, expiry)
    assert sum(map(len, want)) > 10_000
    for f, g, w in zip(filters, got, want):
        assert g == w, f


def test_bad_offsets_are_refused():
    from emqx_amd import _lib
    L = _lib.lib()
    tb = np.frombuffer(b"a/bc/d" + b"\0" * 64, np.uint8).copy()
    h = C.c_void_p()
    for off in ([0, 4, 2, 6], [0, 3, 2**40]):  # non-monotone; an entry far past the buffer
        to = np.array(off, np.uint64)
        rc = L.emqx_gm_retained_compile_host(C.c_void_p(tb.ctypes.data), C.c_void_p(to.ctypes.data), len(off) - 1,
                                             None, None, C.byref(h))
        assert rc == _lib.EINVAL and not h.value
        assert b"offsets" in L.emqx_gm_last_error(None)
    ix = C.c_void_p()
    good = np.array([0, 3, 6], np.uint64)
    assert L.emqx_gm_retained_compile_host(C.c_void_p(tb.ctypes.data), C.c_void_p(good.ctypes.data), 2, None, None,
                                           C.byref(ix)) == 0
    csr = _lib.Csr()
    bad = np.array([0, 4, 2], np.uint64)
    assert L.emqx_gm_retained_match_host(ix, C.c_void_p(tb.ctypes.data), C.c_void_p(bad.ctypes.data), 2, 0,
                                         C.byref(csr)) == _lib.EINVAL
    L.emqx_gm_retained_release(ix)


def test_compiler_and_host_walk_under_asan():
    """tests/asan/asan_retained.cpp: gm_retained.cpp as host C++ under
    AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-retained"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_retained")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_retained ok" in p.stdout
