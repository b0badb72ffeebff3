"""A plain restatement of the reference's authorization check, clause by
clause, as the yardstick of the authz tests (no cleverness, no sharing with
emqx_amd/authz.py):

* emqx_authz_rule:compile/1, match/4, matches/4, feed_var/3
  (apps/emqx_authz/src/emqx_authz_rule.erl:55-195);
* the LIST clauses of emqx_topic:match/2 (apps/emqx/src/emqx_topic.erl:74-87)
  and words/1 (:158-164);
* emqx_authz_mnesia:authorize/4 and do_authorize/4 (emqx_authz_mnesia.erl:95-111,
  212-218), emqx_authz:do_authorize/4 over a chain (emqx_authz.erl:307-317).

Erlang atoms are Python ``str`` and binaries ``bytes``, so ``'+' != b'+'``
exactly as the atom differs from the binary.  ``undefined`` is ``None``.
Rules carry an id beside them: a compiled rule is (id, permission, who, action,
filters).  Also here: the edge set and the seeded random set the CPU, sanitizer
and GPU tests share.
"""

import ipaddress
import random
import re

PH_CLIENTID = b"${clientid}"
PH_USERNAME = b"${username}"


def _bin(x):
    return x.encode() if isinstance(x, str) else bytes(x)


# ---- emqx_topic:words/1
def word(w):
    if w == b"":
        return ""
    if w == b"+":
        return "+"
    if w == b"#":
        return "#"
    return w


def words(topic):
    return [word(w) for w in _bin(topic).split(b"/")]


# ---- emqx_topic:match/2, the list clauses in their order
def topic_match(name, filt):
    if name == [] and filt == []:
        return True
    if name != [] and filt != [] and type(name[0]) is type(filt[0]) and name[0] == filt[0]:
        return topic_match(name[1:], filt[1:])
    if name != [] and filt != [] and filt[0] == "+" and isinstance(filt[0], str):
        return topic_match(name[1:], filt[1:])
    if len(filt) == 1 and filt[0] == "#" and isinstance(filt[0], str):
        return True
    if name != [] and filt != []:
        return False
    if name != [] and filt == []:
        return False
    return False  # match([], [_H | _T2])


# ---- emqx_authz_rule:compile/1
def compile_rule(rule):
    if len(rule) == 2 and rule[1] == "all":
        return (rule[0], "all", "all", [compile_topic(b"#")])
    permission, who, action, topic_filters = rule
    return (permission, compile_who(who), action, [compile_topic(t) for t in topic_filters])


def parse_cidr(cidr):
    net = ipaddress.ip_network(cidr, strict=False)
    return (net.version, int(net.network_address), int(net.broadcast_address))


def compile_who(who):
    if who == "all":
        return "all"
    kind, arg = who
    if kind == "user":
        return compile_who(("username", arg))
    if kind == "client":
        return compile_who(("clientid", arg))
    if kind in ("username", "clientid"):
        if isinstance(arg, tuple) and arg[0] == "re":
            return (kind, ("re_pattern", re.compile(_bin(arg[1]))))
        return (kind, ("eq", _bin(arg)))
    if kind == "ipaddr":
        return ("ipaddr", parse_cidr(arg))
    if kind == "ipaddrs":
        return ("ipaddrs", [parse_cidr(c) for c in arg])
    if kind in ("and", "or"):
        return (kind, [compile_who(w) for w in arg])
    raise ValueError(who)


def compile_topic(topic):
    if isinstance(topic, tuple) and topic[0] == "eq":
        return ("eq", words(topic[1]))
    t = _bin(topic)
    if t.startswith(b"eq "):
        return ("eq", words(t[3:]))
    ws = words(t)
    if PH_USERNAME in ws or PH_CLIENTID in ws:
        return ("pattern", ws)
    return ws


# ---- emqx_authz_rule:match/4
def match(client, pubsub, topic, rule):
    permission, who, action, topic_filters = rule
    if match_action(pubsub, action) and match_who(client, who) and match_topics(client, topic, topic_filters):
        return permission
    return "nomatch"


def match_action(pubsub, action):
    if pubsub == "publish" and action == "publish":
        return True
    if pubsub == "subscribe" and action == "subscribe":
        return True
    if action == "all":
        return True
    return False


def cidr_match(peer, cidr):
    ip = ipaddress.ip_address(peer)
    version, lo, hi = cidr
    return ip.version == version and lo <= int(ip) <= hi


def match_who(client, who):
    if who == "all":
        return True
    kind, arg = who
    if kind == "username" and client.get("username") is None:
        return False
    if kind == "username" and arg[0] == "eq":
        return _bin(client["username"]) == arg[1]
    if kind == "username":
        return arg[1].search(_bin(client["username"])) is not None
    if kind == "clientid" and arg[0] == "eq":
        return client.get("clientid") is not None and _bin(client["clientid"]) == arg[1]
    if kind == "clientid":
        return client.get("clientid") is not None and arg[1].search(_bin(client["clientid"])) is not None
    if kind == "ipaddr":
        return client.get("peerhost") is not None and cidr_match(client["peerhost"], arg)
    if kind == "ipaddrs":
        return client.get("peerhost") is not None and any(cidr_match(client["peerhost"], c) for c in arg)
    if kind == "and":
        acc = True
        for p in arg:
            acc = match_who(client, p) and acc
        return acc
    if kind == "or":
        acc = False
        for p in arg:
            acc = match_who(client, p) or acc
        return acc
    return False


def match_topics(client, topic, filters):
    for f in filters:
        if isinstance(f, tuple) and f[0] == "pattern":
            if match_topic(words(topic), feed_var(client, f[1])):
                return True
        elif match_topic(words(topic), f):
            return True
    return False


def match_topic(topic, filt):
    if isinstance(filt, tuple) and filt[0] == "eq":
        return len(topic) == len(filt[1]) and all(type(a) is type(b) and a == b for a, b in zip(topic, filt[1]))
    return topic_match(topic, filt)


def feed_var(client, pattern):
    acc = []
    for w in pattern:
        if isinstance(w, bytes) and w == PH_CLIENTID:
            acc.append(PH_CLIENTID if client.get("clientid") is None else _bin(client["clientid"]))
        elif isinstance(w, bytes) and w == PH_USERNAME:
            acc.append(PH_USERNAME if client.get("username") is None else _bin(client["username"]))
        else:
            acc.append(w)
    return acc


# ---- a chain of sources: segments as the table models them
def authorize(segments, client, pubsub, topic):
    """segments: ("global", [(id, rule)]) | ("clientid" | "username", {key: [(id, rule)]}); rules
    compiled.  -> (verdict, id, segment kind) of the first matching rule, or ("nomatch", None, None)."""
    for kind, body in segments:
        if kind == "global":
            rules = body
        else:
            key = client.get(kind)
            rules = body.get(_bin(key), []) if key is not None else []
        for rid, rule in rules:
            v = match(client, pubsub, topic, rule)
            if v != "nomatch":
                return v, rid, kind
    return "nomatch", None, None


def db_rule(r):
    """emqx_authz_mnesia:do_authorize/4: compile({Permission, all, Action, [TopicFilter]})"""
    return compile_rule((r[0], "all", r[1], [r[2]]))


class Chain:
    """One chain built twice from the same tuples: the restatement's segments and
    an emqx_amd AuthzTable (ids = positions among all rules)."""

    def __init__(self):
        from emqx_amd import AuthzTable
        self.table = AuthzTable()
        self.segments = []
        self.n = 0

    def file(self, rules):
        self.table.add_file(rules)
        self.segments.append(("global", [(self.n + i, compile_rule(r)) for i, r in enumerate(rules)]))
        self.n += len(rules)
        return self

    def _keyed(self, kind, records):
        body = {}
        for k, rs in records.items():
            body[_bin(k)] = [(self.n + i, db_rule(r)) for i, r in enumerate(rs)]
            self.n += len(rs)
        self.segments.append((kind, body))

    def db(self, clientid=None, username=None, all=None):  # noqa: A002
        self.table.add_builtin_db(clientid, username, all)
        self._keyed("clientid", clientid or {})
        self._keyed("username", username or {})
        self.segments.append(("global", [(self.n + i, db_rule(r)) for i, r in enumerate(all or [])]))
        self.n += len(all or [])
        return self

    def by_clientid(self, records):
        self.table.add_by_clientid(records)
        self._keyed("clientid", records)
        return self

    def by_username(self, records):
        self.table.add_by_username(records)
        self._keyed("username", records)
        return self

    def expect(self, requests):
        """-> (verdict codes, rule ids, segment kinds) of the restatement"""
        code = {"nomatch": 0, "allow": 1, "deny": 2}
        out = [authorize(self.segments, c, a, t) for c, a, t in requests]
        return [code[v] for v, _, _ in out], [0xFFFFFFFF if r is None else r for _, r, _ in out], [k for _, _, k in out]


def from_json_rule(r):
    """A rule of tests/golden/authz_vectors.json (lists) as the tuples above."""
    def who(w):
        if w == "all":
            return w
        k, a = w
        if k in ("and", "or"):
            return (k, [who(x) for x in a])
        if isinstance(a, list) and a and a[0] == "re":
            return (k, ("re", a[1]))
        return (k, a)
    if len(r) == 2:
        return tuple(r)
    return (r[0], who(r[1]), r[2], [tuple(t) if isinstance(t, list) else t for t in r[3]])


# ---- the edge set: one chain [file, built_in_database] and requests at every corner
def edge_case():
    long_word = "w" * 300
    long_cid = "c" * 300
    deep = lambda n, last=None: "/".join(["d%d" % i for i in range(n - (1 if last else 0))] + ([last] if last else []))  # noqa: E731
    file_rules = [
        ("deny", ("username", "blocked"), "all", ["#"]),
        ("allow", ("ipaddr", "10.1.2.0/24"), "publish", ["net/+/x"]),
        ("allow", ("ipaddrs", ["192.168.0.1", "fe80::/10"]), "subscribe", ["v6/#"]),
        ("allow", ("and", []), "publish", ["and/none"]),
        ("allow", ("or", []), "publish", ["or/none"]),
        ("deny", ("and", [("clientid", "c1"), ("username", "u1"), ("ipaddr", "10.0.0.0/8")]), "publish", ["three"]),
        ("allow", ("or", [("username", ("re", "^adm")), ("clientid", ("re", "bot$"))]), "all", ["re/#"]),
        ("allow", "all", "publish", []),
        ("allow", "all", "all", ["a/+", "a/#/c", "#/b", "+/b/", "/lead", "trail/", "", "x//y"]),
        ("allow", "all", "subscribe", [("eq", "#"), "eq a/b", ("eq", "e/${clientid}")]),
        ("allow", "all", "publish", ["cid/${clientid}/m", "${username}/first", "last/${username}",
                                     "both/${clientid}/${username}"]),
        ("allow", "all", "all", [long_word + "/+", deep(8), deep(9), deep(16), deep(17), deep(40),
                                 deep(17, "#"), "p/" + deep(40, "#"), "/".join(["+"] * 16)]),
        ("deny", "all", "subscribe", ["$SYS/#"]),
        ("allow", "all", "all", ["+/x"]),
    ]
    ch = Chain().file(file_rules).db(
        clientid={"c1": [("deny", "publish", "k/c"), ("allow", "all", "k/#")], "": [("allow", "all", "empty/key")],
                  long_cid: [("allow", "publish", "long/${clientid}")],
                  "sameprefix-A": [("allow", "all", "tail/a")], "sameprefix-B": [("deny", "all", "tail/a")]},
        username={"u1": [("allow", "subscribe", "k/c")], "c1": [("deny", "all", "cross")]},
        all=[("allow", "all", "k/c"), ("deny", "all", "#")])
    clients = [
        {"clientid": "c1", "username": "u1", "peerhost": "10.1.2.3"},
        {"clientid": "c2", "username": "blocked", "peerhost": "10.1.2.3"},
        {"clientid": "c2", "username": None, "peerhost": None},
        {"clientid": None, "username": None, "peerhost": "fe80::1"},
        {"clientid": "", "username": "", "peerhost": "192.168.0.1"},
        {"clientid": "+", "username": "#", "peerhost": "10.1.3.0"},
        {"clientid": "a/b", "username": "adm1", "peerhost": "10.1.1.255"},
        {"clientid": "robot", "username": "x", "peerhost": "::ffff:10.1.2.3"},
        {"clientid": long_cid, "username": "u1", "peerhost": "9.255.255.255"},
        {"clientid": "sameprefix-A", "username": "c1", "peerhost": "10.0.0.0"},
        {"clientid": "sameprefix-B", "username": "nobody", "peerhost": "10.255.255.255"},
        {"clientid": "sameprefix-C", "username": "u1", "peerhost": "11.0.0.0"},
    ]
    topics = ["#", "+", "a", "a/b", "a/b/", "a/+", "a/#", "a/#/c", "a/x/c", "#/b", "x/b", "+/b", "q/b/", "/lead", "trail/",
              "", "/", "x//y", "x/y", "e/${clientid}", "e/c1", "e/c2", "cid/c1/m", "cid/c2/m", "cid/${clientid}/m", "cid/+/m", "cid//m",
              "cid/a/b/m", "u1/first", "${username}/first", "#/first", "last/u1", "last/", "last/#", "both/c1/u1",
              "both/${clientid}/${username}", "both/c2/${username}", "net/q/x", "v6/z", "and/none", "or/none", "three",
              "re/1", "$SYS/x", "$SYS/x/y", "k/c", "k/d", "empty/key", "cross", "tail/a", "long/" + long_cid,
              long_word + "/z", long_word[:-1] + "/z", "unknownword", "unknown/x", deep(8), deep(9), deep(16),
              deep(17), deep(40), deep(18), deep(16) + "/zz", deep(39), "p/" + deep(39) + "/more/words",
              "p/" + deep(39), "p/" + deep(38), "/".join(["z"] * 16), "/".join(["z"] * 15), "/".join(["z"] * 17)]
    requests = [(c, a, t) for c in clients for a in ("publish", "subscribe") for t in topics]
    return ch, requests


# ---- the random set: 2,000 rules over 4 segments, 500 keys per keyed segment, 20,000 requests
def random_case(seed=7, n_requests=20000):
    rng = random.Random(seed)
    w = ["w%d" % i for i in range(30)]

    def filt():
        r = rng.random()
        n = rng.randint(2, 4)  # (no lone '#' or '+': one such rule would answer everything)
        ws = [rng.choice(w) for _ in range(n)]
        if r < 0.15:
            ws[rng.randrange(1, n)] = "+"
        elif r < 0.25:
            ws[-1] = "#"
        elif r < 0.33:
            ws[rng.randrange(n)] = rng.choice(["${clientid}", "${username}"])
        elif r < 0.38:
            return ("eq", "/".join(ws))
        return "/".join(ws)

    def who():
        r = rng.random()
        if r < 0.4:
            return "all"
        if r < 0.55:
            return ("ipaddr", "10.%d.0.0/16" % rng.randrange(4))
        if r < 0.65:
            return ("username", "user%d" % rng.randrange(600))
        if r < 0.75:
            return ("clientid", ("re", "^client%d" % rng.randrange(10)))
        if r < 0.9:
            return ("or", [("ipaddr", "10.%d.0.0/16" % rng.randrange(4)), ("username", ("re", "%d$" % rng.randrange(10)))])
        return ("and", [("ipaddrs", ["10.0.0.0/15", "fe80::/10"]), ("clientid", ("re", "%d$" % rng.randrange(10)))])

    perm = lambda: rng.choice(["allow", "deny"])  # noqa: E731
    act = lambda: rng.choice(["publish", "subscribe", "all"])  # noqa: E731
    file_rules = [(perm(), who(), act(), [filt() for _ in range(rng.randint(1, 2))]) for _ in range(40)]
    cids = {"client%d" % i: [(perm(), act(), filt()) for _ in range(2)] for i in range(500)}   # 1,000 rules
    uns = {"user%d" % i: [(perm(), act(), filt()) for _ in range(rng.randint(1, 2))] for i in range(500)}
    n_all = 2000 - 40 - 1000 - sum(len(v) for v in uns.values())
    all_rules = [(perm(), act(), filt()) for _ in range(n_all)]
    ch = Chain().file(file_rules).db(clientid=cids, username=uns, all=all_rules)
    assert ch.n == 2000

    def concretize(f, c):
        """a topic the filter can match for this client: '+' and '#' made words, placeholders the client's values"""
        f = f[1] if isinstance(f, tuple) else f
        out = []
        for x in f.split("/"):
            if x == "+":
                out.append(rng.choice(w))
            elif x == "#":
                out.extend(rng.choice(w) for _ in range(rng.randrange(3)))
            elif x == "${clientid}" and c["clientid"] is not None and rng.random() < 0.9:
                out.append(c["clientid"])
            elif x == "${username}" and c["username"] is not None and rng.random() < 0.9:
                out.append(c["username"])
            else:
                out.append(x)
        return "/".join(out) if out else rng.choice(w)

    requests = []
    for _ in range(n_requests):
        c = {"clientid": "client%d" % rng.randrange(700) if rng.random() < 0.97 else None,
             "username": "user%d" % rng.randrange(700) if rng.random() < 0.9 else None,
             "peerhost": rng.choice(["10.%d.%d.1" % (rng.randrange(6), rng.randrange(256)), "fe80::%x" % rng.randrange(99),
                                     None])}
        r = rng.random()
        own_c, own_u = cids.get(c["clientid"]), uns.get(c["username"])
        if r < 0.34 and own_c:
            topic = concretize(rng.choice(own_c)[2], c)
        elif r < 0.64 and own_u:
            topic = concretize(rng.choice(own_u)[2], c)
        elif r < 0.85:
            g = rng.choice(file_rules) if rng.random() < 0.3 else None
            topic = concretize(rng.choice(g[3]) if g else rng.choice(all_rules)[2], c)
        else:
            n = rng.randint(1, 4)
            ws = [rng.choice(w) for _ in range(n)]
            if rng.random() < 0.3:
                ws[rng.randrange(n)] = rng.choice([c["clientid"] or "x", c["username"] or "y", "+", "#", "zz"])
            topic = "/".join(ws)
        requests.append((c, rng.choice(["publish", "subscribe"]), topic))
    return ch, requests
