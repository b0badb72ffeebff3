"""A plain restatement of what the forward plan answers (include/
emqx_gpu_match.h, "cluster forwards"), written from the reference and sharing no
code with the library.

For each message of a window, in window order, the reference runs
route(aggre(emqx_router:match_routes(Topic)), Delivery)
(apps/emqx/src/emqx_broker.erl:214):

  match_routes/1 (emqx_router.erl:128-134): lookup_routes/1 of the literal
      topic first, then of every filter the trie matched, appended;
  lookup_routes/1 (:136): the routes of one topic in an ets bag -- insertion
      order, an identical route stored once (do_add_route/2, :112-116);
  aggre/1 (emqx_broker.erl:262-273): no route -> []; exactly one route -> that
      one entry; otherwise a left fold that PREPENDS {To, Node} for a node
      route and, for a group route {Group, _Node}, replaces the accumulator
      with lists:usort([{To, Group} | Acc]);
  route/2, do_route/2 (:245-260): [] is the dropped case; an entry whose Node
      is node() is dispatched locally, any other node entry is forwarded
      (forward(Node, To, Delivery)), a group entry goes to emqx_shared_sub.

Here a node is an int (the caller's dense node id), a group is bytes, and a dest
is either an int or a (group, node) tuple.  Erlang orders an atom before a
binary, so in usort a node entry {To, Node} sorts before a group entry {To,
Group} of the same To; equal terms collapse.

``plan`` records every forward and returns, per node, the (row, filter id)
pairs in window order -- within one row sorted by filter id, because the order
of the matches inside one message follows the trie's match order, which the
project treats as a set -- plus, per row, the number of node entries of the
aggregated list (node() included) and its group entries.
"""

import random


def words(t):
    return t.split(b"/")


def topic_match(topic, filt):
    """emqx_topic:match/2 (a '$'-topic is not matched by a leading wildcard)."""
    tw, fw = words(topic), words(filt)
    if topic.startswith(b"$") and fw[0] in (b"+", b"#"):
        return False
    i = 0
    for i, f in enumerate(fw):
        if f == b"#":
            return True
        if i >= len(tw):
            return False
        if f != b"+" and f != tw[i]:
            return False
    return len(tw) == len(fw)


def is_wildcard(filt):
    return any(w in (b"+", b"#") for w in words(filt))


class Routes:
    """The emqx_route bag over the filter set ``index_filters`` (ids = ranks
    among the distinct filters)."""

    def __init__(self, index_filters, routes=()):
        self.names = sorted(set(index_filters))
        self.fid = {f: i for i, f in enumerate(self.names)}
        self.bag = {}
        for f, dest in routes:
            self.add_route(f, dest)

    def add_route(self, f, dest):
        lst = self.bag.setdefault(f, [])
        if dest not in lst:  # lists:member(Route, lookup_routes(Topic))
            lst.append(dest)

    def lookup_routes(self, f):
        return [(f, d) for d in self.bag.get(f, [])]

    def match_ids(self, topic):
        """The row emqx_gm_match(WITH_EXACT) holds: the literal topic if it is a
        filter, then the wildcard filters that match, as ids."""
        row = [self.fid[topic]] if topic in self.fid and not is_wildcard(topic) else []
        row += [i for i, f in enumerate(self.names) if is_wildcard(f) and topic_match(topic, f)]
        return row

    def match_routes(self, row):
        """match_routes/1 over a row of filter ids: the appended lookups."""
        out = []
        for i in row:
            out += self.lookup_routes(self.names[i])
        return out


def _term_key(entry):
    to, x = entry
    return (to, 0, x, b"") if isinstance(x, int) else (to, 1, 0, x)


def usort(entries):
    return sorted(set(entries), key=_term_key)


def aggre(routes):
    if not routes:
        return []
    if len(routes) == 1:
        to, d = routes[0]
        return [(to, d[0])] if isinstance(d, tuple) else [(to, d)]
    acc = []
    for to, d in routes:
        if isinstance(d, tuple):
            acc = usort([(to, d[0])] + acc)
        else:
            acc = [(to, d)] + acc
    return acc


def plan(table, rows, self_node=None, n_nodes=None):
    """rows: per message, the matched filter ids.  Returns (per_node, node_routes,
    groups): per_node[k] = [(row, filter id)] forwarded to node k; node_routes[r]
    = the row's {To, Node} entries, node() included; groups[r] = its sorted
    {To, Group} entries."""
    n_nodes = n_nodes if n_nodes is not None else 1 + max(
        [d for l in table.bag.values() for d in l if isinstance(d, int)] + [0])
    per_node = [[] for _ in range(n_nodes)]
    node_routes, groups = [], []
    for r, row in enumerate(rows):
        entries = aggre(table.match_routes(row))
        fwd = {}
        count, grp = 0, []
        for to, x in entries:  # route/2 folds over every entry; do_route/2 picks the clause
            if not isinstance(x, int):
                grp.append((to, x))
                continue
            count += 1
            if x != self_node:
                fwd.setdefault(x, []).append((r, table.fid[to]))
        for node, pairs in fwd.items():
            per_node[node] += sorted(pairs, key=lambda p: p[1])
        node_routes.append(count)
        groups.append(sorted(grp))
    return per_node, node_routes, groups


def csr_of(rows):
    ro, ids = [0], []
    for r in rows:
        ids += list(r)
        ro.append(len(ids))
    return ro, ids


def plan_lists(p):
    """A library ForwardPlan as plan()'s first two results (within one row
    sorted by filter id)."""
    per_node = []
    for k in range(len(p.node_off) - 1):
        a, b = int(p.node_off[k]), int(p.node_off[k + 1])
        pairs = list(zip(p.rows[a:b].tolist(), p.filters[a:b].tolist()))
        rows_seen = [r for r, _ in pairs]
        assert rows_seen == sorted(rows_seen), "node %d: rows out of window order" % k
        per_node.append(sorted(pairs))
    return per_node, p.row_routes.tolist()


WORDS = [b"a", b"b", b"c", b"dev", b"x1"]
_RANDOM = {}


def random_world(n_nodes, seed=11, n_filters=300, n_topics=2000):
    """(filters, routes with node and group dests, topics, their matched rows), made once per n_nodes."""
    key = (n_nodes, seed, n_filters, n_topics)
    if key not in _RANDOM:
        rnd = random.Random(seed * 1000 + n_nodes)
        filters = set()
        while len(filters) < n_filters:
            w = [rnd.choice(WORDS + [b"+"] * 2) for _ in range(rnd.randint(1, 4))]
            if rnd.random() < 0.3:
                w.append(b"#")
            filters.add(b"/".join(w))
        filters = sorted(filters)
        routes = []
        for f in filters:
            for _ in range(rnd.choice([0, 1, 1, 2, 3])):
                routes.append((f, rnd.randrange(n_nodes)))
            if rnd.random() < 0.25:
                for _ in range(rnd.randint(1, 3)):
                    routes.append((f, (rnd.choice([b"g1", b"g2"]), rnd.randrange(n_nodes))))
        rnd.shuffle(routes)
        topics = [b"/".join(rnd.choice(WORDS) for _ in range(rnd.randint(1, 4))) for _ in range(n_topics)]
        ref = Routes(filters, routes)
        rows = [ref.match_ids(t) for t in topics]
        _RANDOM[key] = (filters, routes, topics, rows, ref)
    return _RANDOM[key]
