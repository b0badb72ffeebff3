"""Where a sharded update puts a filter (gm_route.hip route_filter_shard,
emqx_gm_route_filter_shards_host): the route of a snapshot line is fixed, so a
new filter must land on the shard that every topic able to match it is routed
to (or on every shard).  No GPU: the plan, the route and the rule are host code;
emqx_topic:match/2 comes from the CPU oracle."""

import numpy as np
import pytest


def _base_set(orc, n_gen=5000, n_hot=4000):
    """Generated filters plus one HOT first word (split by its second word at 2
    and 3 shards) and the filters that go to every shard."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(5, n_gen)
    gen = orc.unpack(*render_codes(codes))
    hot = [b"hot/%d/x%d" % (i % 40, i) for i in range(n_hot)]
    extra = [b"hot", b"hot/#", b"hot/+/y", b"#", b"+/x", b"$SYS/#", b"/a", b"solo"]
    return codes, sorted(set(gen) | set(hot) | set(extra))


def _new_filters(orc, have, n=2000):
    """Filters not in the set: generated ones under known first words, new first
    words, new and known second words under the split word, and the edge forms."""
    from emqx_amd.engine import gen_filter_codes, render_codes
    new = [b"hot/+/z", b"+/+", b"oneword", b"", b"hot/+", b"hot/nv0", b"+", b"nw0", b"hot/#/x", b"hot/7", b"/", b"//"]
    for i in range(300):
        new += [b"nw%d/a/b" % i, b"nw%d/+/c" % i, b"nw%d/#" % i]
        new += [b"hot/nv%d/x" % i, b"hot/nv%d/+" % i, b"hot/%d/zz%d" % (i % 40, i)]
    new += [b"hot/%d/#" % i for i in range(40)] + [b"hot/%d/+" % i for i in range(40)]
    new += orc.unpack(*render_codes(gen_filter_codes(9, 4 * n)))
    out, seen = [], set(have)
    for f in new:
        if f not in seen:
            seen.add(f)
            out.append(f)
    assert len(out) >= n
    return out[:n]


def _topics_for(orc, codes, new):
    """Oracle-sampled topics of the set plus, per new filter, topics built to
    match it ('+' -> a word, '#' -> nothing / one word / two words)."""
    topics = orc.unpack(*orc.render_codes(orc.gen_topic_codes(5, 0, 4000, codes)))
    for f in new:
        ws = f.split(b"/")
        lit = [b"p" if w == b"+" else w for w in ws]
        if ws[-1] == b"#":
            topics += [b"/".join(lit[:-1]), b"/".join(lit[:-1] + [b"h"]), b"/".join(lit[:-1] + [b"h", b"k"])]
        else:
            topics.append(b"/".join(lit))
    topics += [b"hot", b"hot/3", b"hot/3/x3", b"hot/nv1/x", b"", b"/a", b"solo", b"$SYS/broker", b"a/b"]
    return topics


@pytest.mark.parametrize("n_shards", [2, 3])
def test_filter_shards_follow_the_fixed_route(orc, n_shards):
    from emqx_amd.engine import ALL_SHARDS, pack, prefix_plan
    codes, filters = _base_set(orc)
    fb, fo = pack(filters)
    sh, route = prefix_plan(fb, fo, n_shards)
    # the hot word is split: its filters lie on several shards, its own forms on every one
    at = {f: int(s) for f, s in zip(filters, sh)}
    assert len({at[f] for f in filters if f.startswith(b"hot/") and f[4:5].isdigit()}) > 1
    assert at[b"hot"] == at[b"hot/#"] == at[b"hot/+/y"] == at[b"#"] == at[b"+/x"] == ALL_SHARDS
    # (i) every filter the plan was made from: the plan's own shard, entry for entry
    assert np.array_equal(route.filter_shards(fb, fo), sh)
    # (ii) filters the plan has never seen: every matching topic is routed to the filter's shard
    new = _new_filters(orc, filters)
    nfb, nfo = pack(new)
    fs = route.filter_shards(nfb, nfo)
    assert all(s == ALL_SHARDS or s < n_shards for s in fs)
    where = {f: int(s) for f, s in zip(new, fs)}
    assert where[b"hot/+/z"] == where[b"+/+"] == where[b"hot/+"] == where[b"+"] == where[b"hot/#/x"] == ALL_SHARDS
    assert where[b"oneword"] != ALL_SHARDS and where[b""] != ALL_SHARDS and where[b"hot/nv0"] != ALL_SHARDS
    assert where[b"hot/7"] == at[b"hot/7/x7"]  # a known second word under the split word: its partition
    topics = _topics_for(orc, codes, new)
    tb, to = pack(topics)
    dest = route.route_host(tb, to)
    order = sorted(range(len(new)), key=lambda i: new[i])
    ro, ids = orc.bruteforce(topics, [new[i] for i in order], mode=1)
    hit = np.zeros(len(new), bool)
    pairs = 0
    for t in range(len(topics)):
        for k in ids[int(ro[t]):int(ro[t + 1])]:
            i = order[int(k)]
            hit[i] = True
            pairs += 1
            assert fs[i] == ALL_SHARDS or fs[i] == dest[t], (n_shards, topics[t], new[i], int(fs[i]), int(dest[t]))
    # the check has teeth: all but the '$'-rooted corner cases were matched by some topic
    assert pairs > len(new) and hit.mean() > 0.95, (pairs, hit.mean())
    route.release()
