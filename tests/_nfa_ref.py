"""A plain reference for the match statistics: the level trie as a dict of
dicts and the NFA walk of SURVEY.md section 8d over it, counting P, the probes
the reference implementation makes for one topic (emqx_trie.erl:139-161,
255-333; emqx_router.erl:128-134).

Pure Python, no code shared with emqx_amd or oracle.  Filters with '#' before
their last word are not handled (the overlay's business).

The index holds every filter in both match modes, so P does not depend on the
mode; only which of the visited filters count as matches does (trie_subset).
"""

_END = 0    # key of a node's own filter (bytes keys are child words)
_HASH = 1   # key of the filter of a node's '#' child


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def build(filters):
    """The level trie: node = {word: child, _END: filter, _HASH: filter}."""
    root = {}
    for f in filters:
        f = _b(f)
        ws = f.split(b"/")
        assert b"#" not in ws[:-1], f
        node = root
        hash_tail = ws[-1] == b"#"
        for w in (ws[:-1] if hash_tail else ws):
            node = node.setdefault(w, {})
        node[_HASH if hash_tail else _END] = f
    return root


def is_wildcard(topic):
    return any(w in (b"+", b"#") for w in _b(topic).split(b"/"))


def walk(filters, topic, _root=None, _set=None, _widths=None):
    """(P, matched_filters, is_wild) of one topic with match_routes semantics
    (sorted list of filter bytes)."""
    topic = _b(topic)
    root = build(filters) if _root is None else _root
    ws = topic.split(b"/")
    if is_wildcard(topic):  # no walk: the literal route only
        fset = {_b(f) for f in filters} if _set is None else _set
        return 0, ([topic] if topic in fset else []), True
    dollar = ws[0].startswith(b"$")
    out = []
    p = 1  # the exact-route probe
    if not dollar and _HASH in root:
        out.append(root[_HASH])
    frontier = [root]
    for lv, w in enumerate(ws):
        if not frontier:
            break
        if _widths is not None:
            _widths.append(len(frontier))
        p += 3 * len(frontier)
        nxt = []
        for node in frontier:
            kids = [node.get(w)]
            if not (dollar and lv == 0):
                kids.append(node.get(b"+"))
            for c in kids:
                if c is not None:
                    if _HASH in c:
                        out.append(c[_HASH])
                    nxt.append(c)
        frontier = nxt
    else:
        p += 2 * len(frontier)
        if _widths is not None:
            _widths.append(len(frontier))
        out.extend(c[_END] for c in frontier if _END in c)
    return p, sorted(out), False


def trie_subset(matched, topic):
    """What emqx_trie:match/1 returns of walk()'s matches: the wildcard filters,
    and a one-word '$' topic's own filter (do_match/2, emqx_trie.erl:271-278)."""
    topic = _b(topic)
    if is_wildcard(topic):
        return []
    quirk = topic.startswith(b"$") and b"/" not in topic
    return [f for f in matched if is_wildcard(f) or (quirk and f == topic)]


class Ref:
    """walk() over one filter set, memoised on the topic bytes."""

    def __init__(self, filters):
        self.filters = sorted({_b(f) for f in filters})
        self._set = set(self.filters)
        self._root = build(self.filters)
        self._memo = {}

    def walk(self, topic):
        """(P, matched_filters, is_wild, widest frontier)"""
        topic = _b(topic)
        r = self._memo.get(topic)
        if r is None:
            widths = []
            p, m, w = walk(self.filters, topic, self._root, self._set, widths)
            r = self._memo[topic] = (p, m, w, max(widths, default=0))
        return r

    def batch(self, topics):
        """(sum of P, wildcard topics, per-topic P)"""
        per = [self.walk(t)[0] for t in topics]
        return sum(per), sum(1 for t in topics if self.walk(t)[2]), per

    def rows(self, topics, exact=True):
        """The batch's rows as lists of filter ids (ranks in the sorted set)."""
        rank = {f: i for i, f in enumerate(self.filters)}
        out = []
        for t in topics:
            m = self.walk(t)[1]
            if not exact:
                m = trie_subset(m, t)
            out.append([rank[f] for f in m])
        return out

    def max_row(self, topics):
        return max((len(self.walk(t)[1]) for t in topics), default=0)

    def max_frontier(self, topics):
        return max((self.walk(t)[3] for t in topics), default=0)


def batch(filters, topics):
    """(sum of P, wildcard-topic count, per-topic P) of a batch."""
    return Ref(filters).batch(topics)
