"""The authorization table on the host alone: the compiler
(emqx_amd/csrc/gm_authz.cpp) and the walk over its tables
(emqx_gm_authz_check_host) against the Python restatement of the reference
(tests/_authz_ref.py), itself checked against the reference suites' vectors
(tests/golden/authz_vectors.json).  No device is needed."""

import json
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import _authz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"nomatch": 0, "allow": 1, "deny": 2}


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "authz_vectors.json")) as f:
        return json.load(f)


def host_answers(chain, requests):
    from emqx_amd import Authz
    a = Authz.compile_host(chain.table)
    try:
        v, r = a.check_host(requests)
        return [int(x) for x in v], [int(x) for x in r]
    finally:
        a.release()


def assert_host_equals_ref(chain, requests):
    want_v, want_r, _ = chain.expect(requests)
    got_v, got_r = host_answers(chain, requests)
    for q, gv, gr, wv, wr in zip(requests, got_v, got_r, want_v, want_r):
        assert (gv, gr) == (wv, wr), q
    return want_v, want_r


def rule_suite_cases():
    g = golden()["rule_suite"]
    return [(exp, dict(g["clients"][c]), act, topic, R.from_json_rule(g["sources"][src]), src)
            for exp, c, act, topic, src in g["t_match"]]


def test_restatement_on_rule_suite_vectors():
    for exp, client, act, topic, rule, src in rule_suite_cases():
        assert R.match(client, act, topic, R.compile_rule(rule)) == exp, (src, client, act, topic)


def test_host_walk_on_rule_suite_vectors():
    g = golden()["rule_suite"]
    for exp, client, act, topic, rule, src in rule_suite_cases():
        ch = R.Chain().file([rule])
        # the regex leaves travel as re_mask bits: the table's own evaluation agrees with the recorded ones
        if src == "SOURCE5":
            assert [list(map(str, (f, p.decode()))) for f, p in ch.table.regexes] == g["regex_bits"]
            assert ch.table.re_mask(client) == client["re_mask"]
        v, r = host_answers(ch, [(client, act, topic)])
        assert v == [CODE[exp]] and r == [0 if exp != "nomatch" else 0xFFFFFFFF], (src, client, act, topic)


def _lib_cases():
    g = golden()["test_lib"]
    out = []
    for name, tab in g["tables"].items():
        rules = [(s["permission"], s["action"], t) for s in tab["samples"] for t in s["topics"]]
        for key in g["keys"]:
            out.append((name, key, rules, tab["no_match"], tab["expected"], dict(g["client"])))
    return out


@pytest.mark.parametrize("case", _lib_cases(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_builtin_database_sample_tables(case):
    """emqx_authz_test_lib's sample tables stored under the client's clientid,
    its username and `all` in turn (emqx_authz_mnesia_SUITE:57-82)."""
    _, key, rules, no_match, expected, client = case
    ch = R.Chain().db(**{key: rules if key == "all" else {client[key]: rules}})
    requests = [(client, act, topic) for _, act, topic in expected]
    want_v, _ = assert_host_equals_ref(ch, requests)
    names = {0: no_match, 1: "allow", 2: "deny"}
    assert [names[v] for v in want_v] == [e for e, _, _ in expected]


def test_acl_conf_default_rules():
    rules = [R.from_json_rule(r) for r in golden()["acl_conf"]["rules"]]
    ch = R.Chain().file(rules)
    reqs = [({"clientid": "c", "username": "^dashboard?", "peerhost": "1.2.3.4"}, "subscribe", "$SYS/brokers"),
            ({"clientid": "c", "username": "dashboard", "peerhost": "1.2.3.4"}, "subscribe", "$SYS/brokers"),
            ({"clientid": "c", "username": "u", "peerhost": "127.0.0.1"}, "publish", "$SYS/x"),
            ({"clientid": "c", "username": "u", "peerhost": "127.0.0.1"}, "subscribe", "#"),
            ({"clientid": "c", "username": "u", "peerhost": "127.0.0.2"}, "publish", "t")]
    want_v, want_r = assert_host_equals_ref(ch, reqs)
    assert (want_v, want_r) == ([1, 0, 1, 1, 0], [0, 0xFFFFFFFF, 1, 1, 0xFFFFFFFF])  # the username is no regex here


def test_edge_set():
    ch, requests = R.edge_case()
    want_v, want_r = assert_host_equals_ref(ch, requests)
    by = {(c["clientid"], a, t): (v, r) for (c, a, t), v, r in zip(requests, want_v, want_r)}
    last = ch.n - 1  # the `all` record's closing deny '#'
    assert by[("c2", "subscribe", "$SYS/x")][0] == 2            # '$SYS/#' reaches it: rule 12, not the '$'-rule
    assert by[("c2", "publish", "$SYS/x")] == (1, 13)           # '+/x' authorizes '$SYS/x': no '$'-rule
    assert by[("c2", "subscribe", "a/#")] == (1, 8)             # the name 'a/#' matches the filter 'a/+'
    assert by[("c2", "subscribe", "#")] == (1, 9)               # eq '#'
    assert by[("c2", "subscribe", "+")] == (2, last)            # eq '#' is not '+'
    assert by[("c2", "publish", "a/#/c")] == (1, 8)             # a '#' before the last word equals the name word '#'
    assert by[("c2", "publish", "a/x/c")] == (2, last)
    assert by[("c2", "publish", "cid/c2/m")] == (1, 10)
    assert by[("+", "publish", "cid/+/m")] == (2, last)         # the value '+' is a binary, the name word an atom
    assert by[("", "publish", "cid//m")][1] != 10               # the value '' likewise
    assert by[("a/b", "publish", "cid/a/b/m")] == (2, last)
    assert by[(None, "publish", "cid/${clientid}/m")] == (1, 10)  # undefined: the placeholder stays literal
    assert by[("c2", "publish", "cid/${clientid}/m")] == (2, last)
    assert by[("c2", "subscribe", "e/${clientid}")] == (1, 9)   # eq filters are not substituted
    assert by[("c2", "subscribe", "e/c2")] == (2, last)


def test_random_set_is_balanced_and_equal():
    """On the restatement alone: each verdict is at least 10 % of the answers and
    each segment kind at least 20 % of the hits, so no comparison can pass on
    a set that is nearly all nomatch.  Then the host walk against it."""
    ch, requests = R.random_case()
    assert ch.n == 2000 and len(ch.segments) == 4 and len(requests) == 20000
    assert all(len(body) == 500 for kind, body in ch.segments if kind != "global")
    want_v, want_r, kinds = ch.expect(requests)
    verdicts = Counter(want_v)
    hits = Counter(k for k in kinds if k)
    print(verdicts, hits)
    for v in (0, 1, 2):
        assert verdicts[v] >= 0.10 * len(requests), verdicts
    for k in ("global", "clientid", "username"):
        assert hits[k] >= 0.20 * sum(hits.values()), hits
    got_v, got_r = host_answers(ch, requests)
    assert got_v == want_v and got_r == want_r


def test_empty_tables_and_batches():
    from emqx_amd import Authz, AuthzTable
    c = {"clientid": "c", "username": "u", "peerhost": "1.1.1.1"}
    reqs = [(c, "publish", "a"), (c, "subscribe", "")]
    assert host_answers(R.Chain(), reqs) == ([0, 0], [0xFFFFFFFF] * 2)            # no segment at all
    assert host_answers(R.Chain().file([]), reqs) == ([0, 0], [0xFFFFFFFF] * 2)   # an empty segment
    ch = R.Chain().by_clientid({"c": [("deny", "all", "a")]}).by_username({})    # only keyed segments
    assert host_answers(ch, reqs) == ([2, 0], [0, 0xFFFFFFFF])
    assert host_answers(ch, []) == ([], [])
    a = Authz.compile_host(ch.table)
    i = a.info()
    assert (i.n_rules, i.n_keys, i.n_segments, i.n_words, i.deepest_filter, i.longest_range, i.device_bytes) == \
        (1, 1, 2, 6, 1, 1, 0)
    a.release()
    assert isinstance(AuthzTable().desc().struct().n_rules, int)


def test_build_refusals():
    from emqx_amd import Authz, AuthzTable, GpuMatchError, _lib
    from emqx_amd.authz import DescArrays
    t = AuthzTable()
    t.add_file([("allow", ("and", [("username", "u"), ("or", [("clientid", "c")])]), "all", ["#"])])
    with pytest.raises(GpuMatchError) as e:
        Authz.compile_host(t)
    assert e.value.code == _lib.EUNSUPPORTED and "nested" in str(e.value)
    t = AuthzTable()
    t.add_file([("allow", ("username", ("re", "^u%d" % k)), "all", ["#"]) for k in range(32)])
    Authz.compile_host(t).release()  # 32 distinct regexes are fine
    t.add_file([("allow", ("username", ("re", "^u1")), "all", ["#"]), ("allow", ("clientid", ("re", "^u1")), "all", ["#"])])
    with pytest.raises(GpuMatchError) as e:
        Authz.compile_host(t)  # ... the 33rd is not (a repeated one is not a new one)
    assert e.value.code == _lib.EUNSUPPORTED and "32 distinct regexes" in str(e.value)

    def desc(**change):
        t = AuthzTable()
        t.add_file([("allow", ("username", "u"), "publish", ["a/b", "c"]), ("deny", "all")])
        t.add_by_clientid({"k1": [("allow", "all", "x")], "k2": [("deny", "all", "y")]})
        d = t.desc()
        names = ["seg_kind", "seg_range_off", "range_rule_off", "key_bytes", "key_off", "rule_id", "rule_perm",
                 "rule_action", "rule_who_op", "rule_who_off", "rule_filter_off", "leaf_kind", "leaf_bytes", "leaf_off",
                 "filter_kind", "filter_bytes", "filter_off"]
        for k, (pos, val) in change.items():
            d.a[names.index(k)][pos] = val
        return d

    def refused(code, text, **change):
        with pytest.raises(GpuMatchError) as e:
            Authz.compile_host(desc(**change))
        assert e.value.code == code and text in str(e.value), str(e.value)

    Authz.compile_host(desc()).release()
    refused(_lib.EINVAL, "action outside 1..3", rule_action=(0, 0))
    refused(_lib.EINVAL, "action outside 1..3", rule_action=(1, 4))
    refused(_lib.EINVAL, "permission", rule_perm=(0, 3))
    refused(_lib.EINVAL, "filter_off: offsets not ascending", filter_off=(1, 7))
    refused(_lib.EINVAL, "filter_off: offsets not ascending", filter_off=(2, 2**40))
    refused(_lib.EINVAL, "key_off: offsets do not start at 0", key_off=(0, 1))
    refused(_lib.EINVAL, "next array's count", rule_filter_off=(4, 4))
    refused(_lib.EINVAL, "next array's count", range_rule_off=(3, 3))
    refused(_lib.EINVAL, "exactly one range", seg_kind=(1, 0))
    refused(_lib.EINVAL, "unknown segment kind", seg_kind=(0, 9))
    refused(_lib.EINVAL, "unknown leaf kind", leaf_kind=(0, 77))
    d = desc()
    d.a[3][:2] = np.frombuffer(b"k2", np.uint8)  # both keys 'k2'
    with pytest.raises(GpuMatchError) as e:
        Authz.compile_host(d)
    assert "listed twice" in str(e.value)
    # a batch with bad offsets or an action outside 1..2 is refused before the walk
    from emqx_amd.authz import RequestBatch
    a = Authz.compile_host(desc())
    b = RequestBatch.from_requests([({"clientid": "k1"}, "publish", "x"), ({}, "subscribe", "y")])
    assert [int(x) for x in a.check_host(b)[0]] == [2, 2]  # the file segment's {deny, all}
    b.a[1][1] = 9
    with pytest.raises(GpuMatchError) as e:
        a.check_host(b)
    assert e.value.code == _lib.EINVAL and "topic_off" in str(e.value)
    b = RequestBatch.from_requests([({"clientid": "k1"}, 3, "x")])
    with pytest.raises(GpuMatchError) as e:
        a.check_host(b)
    assert e.value.code == _lib.EINVAL and "action outside 1..2" in str(e.value)
    a.release()
    assert isinstance(d, DescArrays)


def test_device_check_needs_a_device_table():
    from emqx_amd import Authz, GpuMatchError
    a = Authz.compile_host(R.Chain().file([("allow", "all")]).table)
    with pytest.raises(GpuMatchError):
        a.authorize({"clientid": "c"}, "publish", "t")
    a.release()


def test_compiler_and_host_walk_under_asan():
    """tests/asan/asan_authz.cpp: gm_authz.cpp as host C++ under
    AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-authz"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_authz")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_authz ok" in p.stdout
