"""The authorization check on the device (k_authz_check, emqx_amd/csrc/gm_authz.hip):
device answers against the Python restatement of the reference
(tests/_authz_ref.py) and against the library's host walk, on the reference
suites' vectors, the edge and random sets of the CPU tests, and shapes where
the kernel can go wrong: GLOBAL range lengths and hit positions around the
wave, lanes hitting at different steps, batch sizes around the block, key
lengths around the inline prefix, depths around the LDS levels."""

import functools
import json
import os

import pytest

from tests import _authz_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = 0xFFFFFFFF
C0 = {"clientid": "c", "username": "u", "peerhost": "10.0.0.1"}


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _check(ctx, chain, requests, want=None):
    """Device answers == restatement == host walk; returns (verdicts, rule ids)."""
    a = ctx.build_authz(chain.table)
    try:
        assert a.info().device_bytes > 0
        got_v, got_r = a.authorize_batch(requests)
        host_v, host_r = a.check_host(requests)
    finally:
        a.release()
    want_v, want_r, _ = want if want is not None else chain.expect(requests)
    assert len(got_v) == len(requests) == len(got_r)
    bad = [i for i in range(len(requests)) if (int(got_v[i]), int(got_r[i])) != (want_v[i], want_r[i])]
    assert not bad, (len(bad), requests[bad[0]], int(got_v[bad[0]]), int(got_r[bad[0]]), want_v[bad[0]], want_r[bad[0]])
    assert [int(x) for x in host_v] == want_v and [int(x) for x in host_r] == want_r
    return want_v, want_r


@functools.lru_cache(maxsize=None)
def _random():
    ch, requests = R.random_case()
    return ch, requests, ch.expect(requests)


# ------------------------------------------------------------------ reference parity
def test_golden_vectors(ctx):
    with open(os.path.join(ROOT, "tests", "golden", "authz_vectors.json")) as f:
        g = json.load(f)
    code = {"nomatch": 0, "allow": 1, "deny": 2}
    rs = g["rule_suite"]
    for exp, c, act, topic, src in rs["t_match"]:
        ch = R.Chain().file([R.from_json_rule(rs["sources"][src])])
        v, r = _check(ctx, ch, [(dict(rs["clients"][c]), act, topic)])
        assert v == [code[exp]], (src, c, act, topic)
    tl = g["test_lib"]
    client = dict(tl["client"])
    for name, tab in tl["tables"].items():
        rules = [(s["permission"], s["action"], t) for s in tab["samples"] for t in s["topics"]]
        for key in tl["keys"]:
            ch = R.Chain().db(**{key: rules if key == "all" else {client[key]: rules}})
            v, _ = _check(ctx, ch, [(client, act, topic) for _, act, topic in tab["expected"]])
            names = {0: tab["no_match"], 1: "allow", 2: "deny"}
            assert [names[x] for x in v] == [e for e, _, _ in tab["expected"]], (name, key)
    ch = R.Chain().file([R.from_json_rule(r) for r in g["acl_conf"]["rules"]])
    _check(ctx, ch, [({"clientid": "c", "username": "dashboard", "peerhost": "127.0.0.1"}, a, t)
                     for a in ("publish", "subscribe") for t in ("$SYS/x", "t", "#")])


def test_edge_set(ctx):
    ch, requests = R.edge_case()
    _check(ctx, ch, requests)


def test_random_set(ctx):
    ch, requests, want = _random()
    _check(ctx, ch, requests, want)


# ------------------------------------------------------------------ the GLOBAL scan
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_global_range_length_only_the_last_rule_matches(ctx, n):
    rules = [("deny", "all", "publish", ["miss/%d" % i]) for i in range(n - 1)] + [("allow", "all", "publish", ["hit"])]
    reqs = [(C0, "publish", "hit")] * 70 + [(C0, "publish", "none"), (C0, "subscribe", "hit")]
    v, r = _check(ctx, R.Chain().file(rules), reqs)
    assert v == [1] * 70 + [0, 0] and r[:70] == [n - 1] * 70


@pytest.mark.parametrize("pos", [0, 63, 64, 128])
def test_global_first_hit_position(ctx, pos):
    rules = [("deny", "all", "all", ["r/%d" % i, "r/+/after/%d" % i]) for i in range(129)]
    reqs = [(C0, "publish", "r/%d" % pos), (C0, "subscribe", "r/x/after/%d" % pos)]
    v, r = _check(ctx, R.Chain().file(rules), reqs)
    assert (v, r) == ([2, 2], [pos, pos])


def test_lanes_hit_at_different_steps(ctx):
    """One wave: lane i first hits rule (7 * i) % 129, so lanes drop out of the
    GLOBAL scan at different steps while the others go on."""
    rules = [("allow" if i % 2 else "deny", "all", "all", ["s/%d" % i]) for i in range(129)]
    reqs = [(C0, "publish", "s/%d" % ((7 * i) % 129)) for i in range(64)]
    v, r = _check(ctx, R.Chain().file(rules).file([("allow", "all")]), reqs)
    assert r == [(7 * i) % 129 for i in range(64)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_batch_sizes(ctx, n):
    ch, requests, (wv, wr, wk) = _random()
    _check(ctx, ch, requests[:n], (wv[:n], wr[:n], wk[:n]))


# ------------------------------------------------------------------ keyed segments
def test_many_keys_and_key_lengths(ctx):
    lens = [0, 1, 7, 8, 9, 16, 17, 255]
    cids = {"k" * n: [("allow", "all", "len/%d" % n)] for n in lens}
    cids.update({"cid%05d" % i: [("deny", "publish", "t/%d" % (i % 7)), ("allow", "all", "t/#")] for i in range(5000)})
    # equal in their first 8 bytes and their length, differing in the tail
    cids["prefix00-tailA"] = [("allow", "all", "tail")]
    cids["prefix00-tailB"] = [("deny", "all", "tail")]
    uns = {"un%05d" % i: [("allow", "subscribe", "u/%d" % (i % 5))] for i in range(5000)}
    uns[""] = [("deny", "all", "empty/username")]
    ch = R.Chain().db(clientid=cids, username=uns, all=[("deny", "all", "t/1")])
    reqs = [({"clientid": "k" * n, "username": None, "peerhost": None}, "publish", "len/%d" % m)
            for n in lens + [2, 10, 254] for m in lens]
    reqs += [({"clientid": "cid%05d" % i, "username": "un%05d" % (i + 3)}, a, t)
             for i in range(0, 5004, 3) for a, t in (("publish", "t/%d" % (i % 7)), ("subscribe", "u/%d" % ((i + 3) % 5)))]
    reqs += [({"clientid": c}, "publish", "tail") for c in ("prefix00-tailA", "prefix00-tailB", "prefix00-tailC",
                                                            "prefix00", "prefix00-tail")]
    # defined-but-empty against undefined, for both keys
    reqs += [({"clientid": "", "username": ""}, "publish", t) for t in ("len/0", "empty/username")]
    reqs += [({"clientid": None, "username": None}, "publish", t) for t in ("len/0", "empty/username")]
    reqs += [({"clientid": "absent", "username": "absent"}, "publish", "t/1")]
    v, r = _check(ctx, ch, reqs)
    assert v[-5:] == [1, 2, 0, 0, 2]


@pytest.mark.parametrize("deny_at", ["clientid", "username", "all"])
def test_precedence_between_the_segments(ctx, deny_at):
    """One deny and two allows on one topic among the clientid record, the
    username record and the `all` record, the deny in each place in turn, with a
    file segment in front and behind: the first segment holding a match wins."""
    front = [("allow", ("username", "vip"), "all", ["p"])]
    behind = [("deny", "all", "all", ["#"])]
    perm = {k: ("deny" if k == deny_at else "allow") for k in ("clientid", "username", "all")}
    ch = R.Chain().file(front).db(clientid={"c": [(perm["clientid"], "all", "p")]},
                                  username={"u": [(perm["username"], "all", "p")]},
                                  all=[(perm["all"], "all", "p")]).file(behind)
    reqs = [({"clientid": c, "username": u}, "publish", "p")
            for c, u in (("c", "u"), ("x", "u"), ("x", "y"), ("c", "vip"), (None, None), ("c", None), (None, "u"))]
    reqs.append(({"clientid": "x", "username": "y"}, "publish", "other"))
    v, r = _check(ctx, ch, reqs)
    assert r == [1, 2, 3, 0, 3, 1, 2, 4]
    code = {1: perm["clientid"], 2: perm["username"], 3: perm["all"], 0: "allow", 4: "deny"}
    assert v == [{"allow": 1, "deny": 2}[code[x]] for x in r]


# ------------------------------------------------------------------ topics, words, depth
def _deep(n, word="d"):
    return "/".join("%s%d" % (word, i) for i in range(n))


def test_depths_around_the_lds_levels(ctx):
    depths = [1, 8, 9, 16, 17, 40]
    rules = [("allow", "all", "publish", [_deep(n)]) for n in depths]
    rules += [("deny", "all", "subscribe", ["/".join(["+"] * n)]) for n in depths]
    rules += [("allow", "all", "all", [_deep(16, "h") + "/#", _deep(39, "g") + "/#"])]
    rules += [("deny", "all", "publish", [_deep(15) + "/+/" + "d16", "${clientid}/" + _deep(20, "q"),
                                          _deep(20, "q") + "/${username}"])]
    topics = [_deep(n) for n in depths + [2, 15, 18, 39, 41]]
    topics += [_deep(n, "x") for n in depths]
    topics += [_deep(16, "h"), _deep(16, "h") + "/a", _deep(16, "h") + "/a/b/c", _deep(15, "h"), _deep(17, "h")[:-1],
               _deep(39, "g"), _deep(39, "g") + "/z", _deep(38, "g"), _deep(39, "g") + "/" + _deep(30, "t"),
               _deep(15) + "/zz/d16", _deep(15) + "/zz/d17", "c/" + _deep(20, "q"), "u/" + _deep(20, "q"),
               _deep(20, "q") + "/u", _deep(20, "q") + "/c", _deep(20, "q") + "/${username}"]
    reqs = [(C0, a, t) for a in ("publish", "subscribe") for t in topics]
    reqs += [({"clientid": "c", "username": None}, "publish", _deep(20, "q") + "/${username}")]
    _check(ctx, R.Chain().file(rules), reqs)


def test_words(ctx):
    long_word = "L" * 300
    rules = [("allow", "all", "all", ["known/+", "", "/", "/a", "a/", "a//b", long_word, long_word + "/x", "+/" + long_word])]
    topics = ["known/unknown", "unknown/known", "unknown", "", "/", "//", "/a", "a/", "a", "a//b", "a/b", long_word,
              long_word[:-1], long_word + "x", long_word + "/x", "q/" + long_word, "q/" + long_word[:299] + "M"]
    _check(ctx, R.Chain().file(rules), [(C0, "publish", t) for t in topics])


def test_placeholders(ctx):
    rules = [("allow", "all", "publish", ["${clientid}/first", "mid/${clientid}/x", "last/${username}",
                                          "both/${clientid}/${username}", "both2/${username}/+/${clientid}"]),
             ("deny", "all", "publish", ["eq e/${clientid}"])]
    long_cid = "c" * 300
    clients = [{"clientid": c, "username": u} for c, u in
               (("c", "u"), ("", ""), ("+", "#"), ("#", "+"), ("a/b", "a/b"), (None, None), ("c", None), (None, "u"),
                (long_cid, long_cid[:299]), ("${clientid}", "${username}"))]
    topics = ["c/first", "/first", "+/first", "#/first", "a/b/first", "${clientid}/first", "mid/c/x", "mid//x", "mid/+/x",
              "mid/#/x", "mid/a/b/x", "mid/${clientid}/x", "last/u", "last/", "last/#", "last/+", "last/${username}",
              "both/c/u", "both/${clientid}/u", "both/c/${username}", "both/${clientid}/${username}", "both2/u/z/c",
              long_cid + "/first", long_cid[:299] + "/first", "last/" + long_cid[:299], "last/" + long_cid,
              "e/${clientid}", "e/c"]
    _check(ctx, R.Chain().file(rules), [(c, "publish", t) for c in clients for t in topics])


def test_eq_filters_and_subscribe_names(ctx):
    rules = [("allow", "all", "subscribe", [("eq", "#")]), ("deny", "all", "subscribe", ["eq a/b", ("eq", "p/${clientid}")]),
             ("allow", "all", "subscribe", ["a/+"]), ("deny", "all", "subscribe", ["a/b"]),
             ("allow", "all", "subscribe", ["a/#"]), ("allow", "all", "subscribe", ["+/b"])]
    names = ["#", "a", "+", "a/b", "a/b/", "p/${clientid}", "p/c", "a/#", "a/+", "#/b", "+/b", "a/#/c", "x/b", "a/+/c"]
    v, r = _check(ctx, R.Chain().file(rules), [(C0, "subscribe", t) for t in names])
    by = dict(zip(names, zip(v, r)))
    assert by["#"] == (1, 0) and by["a"] == (1, 4) and by["+"] == (0, NO)  # eq '#'; the name '#' does not match 'a/#'
    assert by["a/b"] == (2, 1) and by["a/b/"] == (1, 4) and by["p/${clientid}"] == (2, 1) and by["p/c"] == (0, NO)
    assert by["a/#"] == (1, 2) and by["a/+"] == (1, 2) and by["x/b"] == (1, 5) and by["+/b"] == (1, 5)
    # 'a/#' against 'a/b' alone, and against 'a/#' alone
    # ... the name '#' against 'a/#', and '+/b' against 'a/b'
    v, r = _check(ctx, R.Chain().file([rules[3], rules[4]]), [(C0, "subscribe", t) for t in ("a/#", "#", "+/b")])
    assert (v, r) == ([1, 0, 0], [1, NO, NO])


def test_dollar_topics_have_no_dollar_rule(ctx):
    rules = [("allow", "all", "publish", ["#"]), ("allow", "all", "subscribe", ["+/x"])]
    v, r = _check(ctx, R.Chain().file(rules), [(C0, "publish", "$SYS/x"), (C0, "subscribe", "$SYS/x"),
                                                (C0, "subscribe", "$SYS/y"), (C0, "publish", "$share/g/t")])
    assert (v, r) == ([1, 1, 0, 1], [0, 1, NO, 0])


# ------------------------------------------------------------------ who
def test_who_ip_ranges(ctx):
    many = ["172.16.%d.0/24" % i for i in range(64)] + ["8.8.8.8"]
    rules = [("allow", ("ipaddr", "10.1.2.0/24"), "all", ["v4"]), ("allow", ("ipaddr", "0.0.0.0/0"), "all", ["v4any"]),
             ("allow", ("ipaddr", "1.2.3.4/32"), "all", ["v4one"]), ("allow", ("ipaddr", "fe80::/10"), "all", ["v6"]),
             ("allow", ("ipaddr", "::/0"), "all", ["v6any"]), ("allow", ("ipaddr", "2001:db8::1/128"), "all", ["v6one"]),
             ("allow", ("ipaddrs", ["9.9.9.9"]), "all", ["n1"]), ("allow", ("ipaddrs", ["9.9.9.9", "7.0.0.0/8"]), "all", ["n2"]),
             ("allow", ("ipaddrs", many), "all", ["n65"])]
    peers = ["10.1.1.255", "10.1.2.0", "10.1.2.255", "10.1.3.0", "0.0.0.0", "255.255.255.255", "1.2.3.3", "1.2.3.4", "1.2.3.5",
             "fe7f:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fe80::", "febf:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fec0::",
             "::", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "2001:db8::", "2001:db8::1", "2001:db8::2", "::10.1.2.3",
             "9.9.9.9", "7.255.255.255", "8.0.0.0", "8.8.8.8", "172.16.63.255", "172.16.64.0", "172.15.255.255", None]
    topics = ["v4", "v4any", "v4one", "v6", "v6any", "v6one", "n1", "n2", "n65"]
    reqs = [({"clientid": "c", "username": "u", "peerhost": p}, "publish", t) for p in peers for t in topics]
    _check(ctx, R.Chain().file(rules), reqs)


def test_who_and_or_regex(ctx):
    three = [("clientid", "c"), ("username", "u"), ("ipaddr", "10.0.0.0/8")]
    rules = [("allow", ("and", []), "all", ["and0"]), ("allow", ("or", []), "all", ["or0"]),
             ("allow", ("and", three), "all", ["and3"]), ("allow", ("or", three), "all", ["or3"]),
             ("allow", ("username", ("re", "^r0")), "all", ["re0"])]
    rules += [("deny", ("clientid", ("re", "x%d$" % k)), "all", ["fill"]) for k in range(30)]
    rules += [("allow", ("clientid", ("re", "31$")), "all", ["re31"]), ("deny", ("username", "u"), "all", ["un"]),
              ("deny", ("clientid", "c"), "all", ["cid"])]
    clients = [{"clientid": c, "username": u, "peerhost": p} for c, u, p in
               (("c", "u", "10.1.1.1"), ("x", "u", "10.1.1.1"), ("c", "x", "10.1.1.1"), ("c", "u", "11.1.1.1"),
                ("x", "x", "11.1.1.1"), (None, None, None), ("c", None, "10.1.1.1"), ("id31", "r0x", None),
                ("id3", "xr0", None), ("", "", "10.0.0.0"))]
    ch = R.Chain().file(rules)
    assert len(ch.table.regexes) == 32 and ch.table.re_mask({"clientid": "id31", "username": "r0x"}) == (1 << 31) | 1
    topics = ["and0", "or0", "and3", "or3", "re0", "re31", "un", "cid"]
    _check(ctx, ch, [(c, "publish", t) for c in clients for t in topics])


# ------------------------------------------------------------------ rules and actions
def test_rule_without_filters_many_filters_and_actions(ctx):
    rules = [("deny", "all", "all", []), ("allow", "all", "publish", ["m/%d" % i for i in range(64)] + ["hit"]),
             ("allow", "all", "publish", ["pub"]), ("allow", "all", "subscribe", ["sub"]), ("deny", "all", "all", ["any"])]
    reqs = [(C0, a, t) for a in ("publish", "subscribe") for t in ("hit", "m/63", "pub", "sub", "any", "none")]
    v, r = _check(ctx, R.Chain().file(rules), reqs)
    assert (v, r) == ([1, 1, 1, 0, 2, 0, 0, 0, 0, 1, 2, 0], [1, 1, 2, NO, 4, NO, NO, NO, NO, 3, 4, NO])


def test_empty_tables(ctx):
    reqs = [(C0, "publish", "a"), (C0, "subscribe", "")]
    assert _check(ctx, R.Chain(), reqs) == ([0, 0], [NO, NO])
    assert _check(ctx, R.Chain().file([]).db(), reqs) == ([0, 0], [NO, NO])
    ch = R.Chain().by_username({"u": [("deny", "all", "a")]}).by_clientid({})
    assert _check(ctx, ch, reqs) == ([2, 0], [0, NO])


def test_single_request_api_and_info(ctx):
    ch = R.Chain().file([("deny", ("username", "blocked"), "all", ["#"])]).db(all=[("allow", "publish", "t/${clientid}")])
    a = ctx.build_authz(ch.table)
    try:
        assert a.authorize({"clientid": "c", "username": "blocked"}, "publish", "t/c") == ("deny", 0)
        assert a.authorize({"clientid": "c", "username": "u"}, "publish", "t/c") == ("allow", 1)
        assert a.authorize({"clientid": "c", "username": "u"}, "subscribe", "t/c") == ("nomatch", None)
        i = a.info()
        assert (i.n_rules, i.n_keys, i.n_segments, i.deepest_filter, i.longest_range) == (2, 0, 4, 2, 1)
        assert i.device_bytes > 0 and i.build_ms > 0
        v, r = a.authorize_batch([({"clientid": "c"}, "publish", "t/c")] * 300, timed=True)
        assert set(v) == {1} and a.last_kernel_ms() > 0
    finally:
        a.release()


def test_release_after_check_and_coexistence(ctx):
    """A released table takes its allocation with it; the context, a filter
    index on it and a second table go on working, and the handle is gone."""
    from emqx_amd import GpuMatchError
    idx = ctx.build_index([b"a/+", b"#"])
    first = [x.tolist() for x in ctx.match(idx, [b"a/b", b"x"])]
    ch = R.Chain().file([("allow", "all")])
    for _ in range(3):
        a = ctx.build_authz(ch.table)
        assert a.authorize(C0, "publish", "a/b") == ("allow", 0)
        a.release()
        assert a.h is None
        assert [x.tolist() for x in ctx.match(idx, [b"a/b", b"x"])] == first
    with pytest.raises(GpuMatchError):
        a.authorize(C0, "publish", "a/b")
    b = ctx.build_authz(R.Chain().file([("deny", "all")]).table)
    assert b.authorize(C0, "publish", "a/b") == ("deny", 0)
    b.release()
    idx.release()
