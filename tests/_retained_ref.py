"""Plain Python restatement of the reference's retained-message match, the
expected value of the retained-lookup tests.

condition/1 (apps/emqx_retainer/src/emqx_retainer_mnesia.erl:225-230) turns the
filter's words into an ETS pattern: '+' -> '_', and with '#' as the LAST word
the first '#' is dropped and the list's tail becomes '_' (any further words,
none included).  Any '#' left in the pattern is an atom no stored word equals.
make_match_spec/1 (:232-244) keeps a row if expiry_time is 0 or > NowMs.  Rows
are ordered by the topics' word lists (Python's tuple order of the split
bytes: word by word as unsigned bytes, a proper prefix first).
"""


def match_words(fw: list, tw: list) -> bool:
    open_tail = fw[-1] == b"#"
    if open_tail:
        fw = list(fw)
        fw.remove(b"#")          # Ws1 -- ['#'] drops the FIRST '#'
    if len(tw) < len(fw) or (not open_tail and len(tw) != len(fw)):
        return False
    return all(f == b"+" or (f != b"#" and f == t) for f, t in zip(fw, tw))


def matches(filt: bytes, topic: bytes) -> bool:
    return match_words(filt.split(b"/"), topic.split(b"/"))


def alive(expiry_ms: int, now_ms: int) -> bool:
    return expiry_ms == 0 or expiry_ms > now_ms


def build_table(topics, ids=None, expiry_ms=None) -> dict:
    """topic -> (id, expiry); of equal topics the last one wins (mria:dirty_write)."""
    tab = {}
    for i, t in enumerate(topics):
        tab[t] = (i if ids is None else int(ids[i]), 0 if expiry_ms is None else int(expiry_ms[i]))
    return tab


def match_rows(table: dict, filters, now_ms: int = 0) -> list:
    """Per filter: the ids of the matching, unexpired topics in word-list order."""
    order = sorted((tuple(t.split(b"/")), v) for t, v in table.items())
    live = [(tw, i) for tw, (i, e) in order if alive(e, now_ms)]
    rows = []
    for f in filters:
        fw = f.split(b"/")
        rows.append([i for tw, i in live if match_words(fw, tw)])
    return rows


# ---- the shared sets of tests/test_retained_cpu.py and tests/test_gpu_retained.py
EDGE_TOPICS = [b"", b"/", b"a", b"a/", b"a//b", b"$SYS/x", b"a!", b"a/b",
               b"longword_0001/x", b"longword_0002/x", b"longword_0002", b"a/b/c", b"+/lit", b"a+"]
EDGE_FILTERS = [b"#", b"+", b"+/#", b"a/#", b"#/a", b"a/+/#", b"a+", b"unknown", b"a/unknown", b"a/b/c/d",
                b"a/b/c/d/#", b"+/+/+/+", b"", b"/", b"+/", b"/+", b"a/+/b", b"longword_0001/+", b"longword_0002/#",
                b"longword_0003/#", b"$SYS/+", b"+/x", b"#/#", b"a/#/#", b"+/lit", b"a/b/c/#", b"a/b/c/+"]

VOCAB = [b"a", b"b", b"c", b"dd", b"", b"$SYS", b"e!", b"longword_over_8_a", b"longword_over_8_b", b"f", b"g1", b"h"]


def random_set(seed: int = 7, n_topics: int = 3000, n_filters: int = 2000):
    """3,000 topics over a 12-word vocabulary, depth 1 to 6 (duplicates as they
    fall), and 2,000 filters, 40 % of them with a final '#'."""
    import random
    rng = random.Random(seed)
    topics = [b"/".join(rng.choice(VOCAB) for _ in range(rng.randint(1, 6))) for _ in range(n_topics)]
    filters = []
    for _ in range(n_filters):
        tail = rng.random() < 0.4
        n_words = rng.randint(0 if tail else 1, 5 if tail else 6)
        ws = [b"+" if rng.random() < 0.3 else rng.choice(VOCAB) for _ in range(n_words)]
        if tail:
            ws.append(b"#")
        if rng.random() < 0.02:
            ws[rng.randrange(len(ws))] = b"nowhere"
        filters.append(b"/".join(ws))
    expiry = [rng.choice([0, 0, 5, 10, 11, 50]) for _ in range(n_topics)]
    return topics, filters, expiry


_RANDOM = {}


def random_case(now_ms: int = 10):
    """random_set() with caller ids 3 i + 1 and its reference rows at now_ms, computed once per process."""
    if now_ms not in _RANDOM:
        topics, filters, expiry = random_set()
        ids = [3 * i + 1 for i in range(len(topics))]
        _RANDOM[now_ms] = (topics, filters, expiry, ids, match_rows(build_table(topics, ids, expiry), filters, now_ms))
    return _RANDOM[now_ms]
