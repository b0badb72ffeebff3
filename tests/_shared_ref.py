"""A plain restatement of emqx_shared_sub's member selection (pick/6,
do_pick/6, pick_subscriber/6, do_pick_subscriber/6,
apps/emqx/src/emqx_shared_sub.erl:234-288) applied hit by hit in batch order,
with a dict as the publisher's process dictionary, and of the table's build
rules (include/emqx_gpu_match.h, emqx_gm_shared_build: sort, merge, dedupe,
carry-over).  The tests compare the library with it; it shares no code with the
library.  rand:uniform/1 is replaced by the library's documented mix functions
(gm_shared.h)."""

import random

M32 = 0xFFFFFFFF


def fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def mix(a, b):
    return fmix((fmix((a + 0x9E3779B9) & M32) + b) & M32)


def mix3(a, r, s):
    return mix(mix(a, r), s)


class Table:
    """slots: [(filter bytes, group id, [member ids])] in any order, against the
    filter set ``index_filters`` (ids = ranks among the distinct filters)."""

    def __init__(self, index_filters, slots, prev=None):
        self.names = sorted(set(index_filters))
        fid = {f: i for i, f in enumerate(self.names)}
        merged = {}
        for f, g, mem in slots:
            if f not in fid:
                raise KeyError(f)
            lst = merged.setdefault((fid[f], g), [])
            for m in mem:
                if m not in lst:  # an ets bag stores an identical object once
                    lst.append(m)
        self.slots = [(k[0], k[1], merged[k]) for k in sorted(merged) if merged[k]]  # no empty slot
        self.of_filter = {}
        for s, (f, _, _) in enumerate(self.slots):
            self.of_filter.setdefault(f, []).append(s)
        # the process dictionary, keyed as the reference keys it: {Kind, Group, Topic}
        self.pd = {}
        if prev is not None:
            for f, g, mem in self.slots:
                key = (g, self.names[f])
                if ("rr", key) in prev.pd and prev.has_slot(key):
                    self.pd[("rr", key)] = prev.pd[("rr", key)]
                if prev.pd.get(("st", key)) in mem and prev.has_slot(key):
                    self.pd[("st", key)] = prev.pd[("st", key)]

    def has_slot(self, key):
        return any((g, self.names[f]) == key for f, g, _ in self.slots)

    def slot_list(self):
        return [(f, g, list(mem)) for f, g, mem in self.slots]

    # do_pick_subscriber/6 (:270-285); Nth is 1-based
    def _nth(self, strategy, key, s, row, h, seed, count):
        if strategy == "random":
            return 1 + mix3(seed, row, s) % count
        if strategy == "hash":
            return 1 + h % count
        assert strategy == "round_robin"
        n = self.pd.get(("rr", key))
        rem = mix(seed, s) % count if n is None else (n + 1) % count
        self.pd[("rr", key)] = rem
        return rem + 1

    # pick_subscriber/6 (:265-268)
    def _pick_subscriber(self, strategy, key, s, row, h, seed, subs):
        if len(subs) == 1:
            return subs[0]
        return subs[self._nth(strategy, key, s, row, h, seed, len(subs)) - 1]

    # pick/6 (:234-249) with FailedSubs = []
    def pick_one(self, strategy, s, row, h, seed):
        f, g, mem = self.slots[s]
        key = (g, self.names[f])
        if strategy == "sticky":
            sub0 = self.pd.get(("st", key))
            if sub0 is not None and sub0 in mem:
                return sub0
            # do_pick(random, ...): the one member, else the "random" first pick mix(seed, s)
            sub = mem[0] if len(mem) == 1 else mem[mix(seed, s) % len(mem)]
            self.pd[("st", key)] = sub  # "stick to whatever pick result" (:245)
            return sub
        return self._pick_subscriber(strategy, key, s, row, h, seed, mem)

    def pick(self, rows, strategy, hashes=None, seed=0):
        """rows: a list of lists of filter ids.  -> (row_off, members, slots)."""
        ro, members, slots = [0], [], []
        for r, row in enumerate(rows):
            for f in row:
                for s in self.of_filter.get(f, []):
                    members.append(self.pick_one(strategy, s, r, hashes[r] if hashes is not None else 0, seed))
                    slots.append(s)
            ro.append(len(members))
        return ro, members, slots


def rows_of(ro, ids):
    return [[int(x) for x in ids[int(ro[i]):int(ro[i + 1])]] for i in range(len(ro) - 1)]


def csr_of(rows):
    ro, ids = [0], []
    for r in rows:
        ids.extend(r)
        ro.append(len(ids))
    return ro, ids


def random_case(seed, n_filters=120, n_slots=150, n_rows=400):
    """(index filters, slots, rows): some filters with several groups, member
    counts 1..70, duplicate (filter, group) inputs and duplicate members, rows of
    0..6 filter ids, some without any slot."""
    rng = random.Random(seed)
    filters = [b"f/%04d/%s" % (i, rng.choice([b"+", b"#", b"x"])) for i in range(n_filters)]
    shared = rng.sample(filters, n_filters // 2)
    slots = []
    for _ in range(n_slots):
        f = rng.choice(shared)
        g = rng.randrange(4)
        n = rng.choice([1, 1, 2, 3, 5, 8, 64, 65, 70])
        base = rng.randrange(10_000)
        mem = [base + rng.randrange(2 * n) for _ in range(n)]
        slots.append((f, g, mem))
    names = sorted(set(filters))
    fid = {f: i for i, f in enumerate(names)}
    rows = []
    for _ in range(n_rows):
        k = rng.choice([0, 1, 1, 2, 3, 6])
        rows.append(sorted(rng.sample(range(len(names)), k)))
    return filters, slots, rows, fid
