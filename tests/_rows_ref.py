"""Plain references and the case list for the kernels that consume finished
rows (emqx_amd/csrc/gm_csr.hip) and the scan under them (gm_scan.h): the
fan-out and its delivery-range parts, the sharded index's row merge and the
row lengths.  numpy only, no library calls: tests/test_rows_ref_cpu.py holds
the references against the oracle and a per-row sorted(), and holds the case
list against the boundaries of the kernels (classify, the coverage ledger);
tests/test_gpu_rows.py runs the same cases on the device.

The constants are the sources': gm_scan.h (SCAN1_B, SCAN_B, SCAN_LOOP_MAX),
gm_internal.h (fan_per_block), gm_host.cpp (the small host fan-out's
capacity and its 16M-delivery limit), gm_api.cpp (its 65,536-row limit)."""

import functools

import numpy as np

SCAN1_B = 4096          # k_scan_one / one chunk of k_scan_loop: outputs per launch (inputs + 1)
SCAN_B = 1024           # k_scan_local: values per workgroup
SCAN_LOOP_MAX = 32768   # k_scan_loop: 8 chunks of SCAN1_B outputs
GROUP = 4               # elements a thread of k_fanout_copy moves at a time
SMALL_MAX_ROWS = 65536
SMALL_MAX_DELIVERIES = 16 << 20

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2047, 2049]
SCAN_NNZ = [0, 1, 4095, 4096, 4097, 5119, 5120, 32766, 32767, 32768, 4_193_279, 4_193_280]
BIG_NNZ = (4_193_279, 4_193_280)  # (the GM_FANOUT_SIMPLE and device-row paths only)


def fan_per_block(total):
    per = total // 2048
    per = 1024 if per < 1024 else 65536 if per > 65536 else per
    return (per + 1023) & ~1023


def scan_form(n_in):
    """The form scan_excl takes for n_in inputs: one launch, three launches
    (local, a one-launch scan of the block sums, add), or a block-sum scan that
    is itself three launches."""
    n_out = n_in + 1
    if n_out <= SCAN1_B:
        return "one"
    nb = (n_out + SCAN_B - 1) // SCAN_B
    return "three" if nb + 1 <= SCAN1_B else "recursive"


def scan_form_small(n_in):
    """queue_fanout_small: k_scan_loop while the outputs fit its 8 chunks."""
    return "loop" if n_in + 1 <= SCAN_LOOP_MAX else scan_form(n_in)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def _seg_dst(m_ids, sub_off):
    so = np.asarray(sub_off, np.int64)
    f = np.asarray(m_ids, np.int64)
    lens = so[f + 1] - so[f]
    dst = np.zeros(len(f) + 1, np.int64)
    np.cumsum(lens, out=dst[1:])
    return so, f, lens, dst


def fanout_ref(m_off, m_ids, sub_off, sub_ids):
    """(row_off, ids): the delivery lists of the matched filters concatenated in match order;
    row_off[i] = seg_dst[m_off[i]], seg_dst the exclusive scan of the lists' lengths."""
    so, f, lens, dst = _seg_dst(m_ids, sub_off)
    total = int(dst[-1])
    # delivery p of segment s comes from sub_ids[sub_off[f[s]] + (p - dst[s])]
    src = np.repeat(so[f] - dst[:-1], lens) + np.arange(total, dtype=np.int64)
    ids = np.asarray(sub_ids, np.uint32)[src] if total else np.zeros(0, np.uint32)
    return dst[np.asarray(m_off, np.int64)].astype(np.uint64), ids


def part_range(total, part, n_parts):
    total, part, n_parts = int(total), int(part), int(n_parts)  # (Python integers: no 64-bit wrap)
    return total * part // n_parts, total * (part + 1) // n_parts


def fanout_part_ref(m_off, m_ids, sub_off, sub_ids, part, n_parts, whole=None):
    """(first, ids_slice): deliveries [glo, ghi) of the whole fan-out (`whole`: fanout_ref's result, if at hand)."""
    _, ids = whole if whole is not None else fanout_ref(m_off, m_ids, sub_off, sub_ids)
    glo, ghi = part_range(len(ids), part, n_parts)
    return glo, ids[glo:ghi]


def merge_rows_ref(lens, ids, n):
    """lens [P][stride] (u32), ids the (piece, row) lists piece-major, row-minor: row t of the
    result is the sorted concatenation of the P lists of row t."""
    lens = np.asarray(lens, np.int64)
    pos = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens.ravel(), out=pos[1:])
    pos = pos[:-1].reshape(lens.shape)
    ids = np.asarray(ids, np.uint32)
    row_off, out = np.zeros(n + 1, np.uint64), []
    for t in range(n):
        row = np.concatenate([ids[pos[p, t]:pos[p, t] + lens[p, t]] for p in range(lens.shape[0])])
        out.append(np.sort(row))
        row_off[t + 1] = row_off[t] + np.uint64(len(row))
    return row_off, np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def row_lengths_ref(row_off):
    return np.diff(np.asarray(row_off, np.uint64)).astype(np.uint32)


# ---------------------------------------------------------------------------
# the fan-out world: one filter per length
# ---------------------------------------------------------------------------
FILTERS = [b"len/%04d" % n for n in LENGTHS]
# subscriber ids distinct across the lists and descending inside one (a list is not in id order)
LISTS = [[100_000 * (i + 1) + 7 * k for k in range(n)][::-1] for i, n in enumerate(LENGTHS)]


def host_perm():
    """The id an index gives input filter i (its rank among the sorted filters): what idx.perm holds."""
    order = sorted(range(len(FILTERS)), key=lambda i: FILTERS[i])
    perm = np.zeros(len(FILTERS), np.uint32)
    perm[order] = np.arange(len(FILTERS), dtype=np.uint32)
    return perm


def world_csr(perm):
    """(sub_off, sub_ids) in the index's id order."""
    by_id = np.argsort(np.asarray(perm, np.int64))
    so = np.zeros(len(FILTERS) + 1, np.uint64)
    so[1:] = np.cumsum([len(LISTS[i]) for i in by_id])
    si = np.array([x for i in by_id for x in LISTS[i]], np.uint32)
    return so, si


class FanCase:
    """A match list the test makes itself: m_off (u64 row offsets) over m_fi, each entry the
    POSITION in LENGTHS of a filter (ids(perm) maps it to the index's ids)."""

    def __init__(self, name, m_off, m_fi, seed=None):
        self.name, self.seed = name, seed
        self.m_off = np.ascontiguousarray(m_off, np.uint64)
        self.m_fi = np.ascontiguousarray(m_fi, np.uint32)
        assert self.m_off[0] == 0 and int(self.m_off[-1]) == len(self.m_fi)
        assert (np.diff(self.m_off.astype(np.int64)) >= 0).all()

    @property
    def n_rows(self):
        return len(self.m_off) - 1

    @property
    def nnz(self):
        return len(self.m_fi)

    def seg_lens(self):
        return np.asarray(LENGTHS, np.int64)[self.m_fi.astype(np.int64)]

    @property
    def total(self):
        return int(self.seg_lens().sum())

    def ids(self, perm):
        return np.asarray(perm, np.uint32)[self.m_fi.astype(np.int64)]


def _from_rows(name, rows, seed=None):
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return FanCase(name, off, [LENGTHS.index(n) for r in rows for n in r], seed)


def _pairs_rows(k):
    """k one-subscriber segments (every later segment start moves by k), a row [a, b] for every
    ordered pair of LENGTHS, a row [a] for every length; an empty row after every seventh row."""
    rows = ([[1] * k] if k else []) + [[a, b] for a in LENGTHS for b in LENGTHS] + [[a] for a in LENGTHS]
    out = []
    for r in rows:
        out.append(r)
        if len(out) % 8 == 7:
            out.append([])
    return out


def _empties_rows(run):
    """`run` zero-length segments at the start of the list, at delivery 1,024 (where one
    workgroup's range ends and the next one's starts; also where 2 parts cut) and at the end."""
    segs = [0] * run + [1023, 1] + [0] * run + [1024] + [0] * run
    assert sum(segs) == 2048
    # rows of three segments: some rows are all zero-length segments, some mix them
    return [segs[i:i + 3] for i in range(0, len(segs), 3)] + [[]]


def _scan_case(nnz, rows):
    """nnz ids of the filters of length 0..3, mean length 1 (so ~nnz deliveries); rows: "one"
    (a single row), "cut" (cut at random, empty rows allowed) or "wide" (65,536 rows of 0 or 1)."""
    seed = nnz * 3 + {"one": 0, "cut": 1, "wide": 2}[rows]
    rng = np.random.RandomState(seed % (1 << 31))
    fi = rng.choice(4, size=nnz, p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint32)  # (LENGTHS[0..3] = 0, 1, 2, 3)
    if rows == "one":
        off = np.array([0, nnz], np.uint64)
    elif rows == "cut":
        n_rows = min(max(nnz // 3, 3), 5000)
        off = np.concatenate([[0], np.sort(rng.randint(0, nnz + 1, size=n_rows - 1)), [nnz]]).astype(np.uint64)
    else:
        has = np.zeros(SMALL_MAX_ROWS, np.int64)
        has[rng.choice(SMALL_MAX_ROWS, size=nnz, replace=False)] = 1
        off = np.concatenate([[0], np.cumsum(has)]).astype(np.uint64)
    name = "scan_%d_%s" % (nnz, rows)
    return FanCase(name, off, fi, seed)


def _builders():
    b = {}
    for k in range(4):
        b["pairs_%d" % k] = functools.partial(lambda k: _from_rows("pairs_%d" % k, _pairs_rows(k)), k)
    for run in (1, 2, 300):
        b["empties_%d" % run] = functools.partial(lambda r: _from_rows("empties_%d" % r, _empties_rows(r)), run)
    b["empties_only"] = lambda: _from_rows("empties_only", [[0, 0], [], [0, 0, 0], [0], [0]])
    for nnz in SCAN_NNZ:
        for rows in ("one", "cut"):
            b["scan_%d_%s" % (nnz, rows)] = functools.partial(_scan_case, nnz, rows)
    b["scan_4097_wide"] = functools.partial(_scan_case, 4097, "wide")

    def wide():
        rows, one = [], _pairs_rows(0)
        per_copy = sum(sum(r) for r in one)
        while fan_per_block(per_copy * (len(rows) // len(one))) < 2048:
            rows += one
        return _from_rows("wide", rows)
    b["wide"] = wide
    b["tiny"] = lambda: _from_rows("tiny", [[2], [], [0, 3]])
    return b


_BUILDERS = _builders()
FAN_CASES = list(_BUILDERS)
BIG_CASES = [n for n in FAN_CASES if n.startswith(tuple("scan_%d_" % x for x in BIG_NNZ))]
PART_CASES = [("pairs_1", n) for n in (1, 2, 3, 7, 8)] + [("wide", n) for n in (1, 2, 3, 7, 8)] + \
             [(c, n) for c in FAN_CASES if c.startswith("empties_") for n in (1, 2, 3, 7, 8)] + [("tiny", 5 + 3)]


@functools.lru_cache(maxsize=None)
def fan_case(name):
    return _BUILDERS[name]()


# ---------------------------------------------------------------------------
# merge worlds
# ---------------------------------------------------------------------------
MERGE_WORLDS = [(n, s, p) for n, s in ((0, 0), (1, 1), (255, 255), (256, 259), (257, 257)) for p in (1, 2, 3, 8)] + \
               [(1365, 1365, 3), (2048, 2048, 2), (4097, 4097, 1)]
LONG_ROW = 5000  # one row of the 257-row worlds


class MergeWorld:
    """lens [P][stride] (rows t >= n: 0) and the (piece, row) lists piece-major, row-minor; the
    lists of one row are sorted and disjoint.  shapes[t]: how row t was dealt."""

    def __init__(self, n, stride, pieces):
        self.name = "n%d_s%d_p%d" % (n, stride, pieces)
        self.n, self.stride, self.pieces = n, stride, pieces
        self.seed = n * 31 + stride * 7 + pieces
        rng = np.random.RandomState(self.seed)
        kinds = ["empty"] + ["only_%d" % p for p in range(pieces)] + ["round_robin", "blocks", "ends"]
        self.shapes, lists = [], [[None] * n for _ in range(pieces)]
        for t in range(n):
            kind = "long" if (n == 257 and t == 128) else kinds[t % len(kinds)]
            self.shapes.append(kind)
            k = LONG_ROW if kind == "long" else int(rng.randint(1, 13))
            ids = np.unique(rng.randint(1, 0xFFFFFFFF, size=k + 8, dtype=np.int64))[:k]
            if kind == "ends":
                ids = np.unique(np.concatenate([[0, 0xFFFFFFFF], ids]))
            if kind == "empty":
                ids = ids[:0]
            if kind.startswith("only_"):
                deal = [ids if p == int(kind[5:]) else ids[:0] for p in range(pieces)]
            elif kind == "blocks":
                cut = [len(ids) * p // pieces for p in range(pieces + 1)]
                deal = [ids[cut[p]:cut[p + 1]] for p in range(pieces)]
            else:  # round robin (an empty list deals empty lists)
                deal = [ids[p::pieces] for p in range(pieces)]
            for p in range(pieces):
                lists[p][t] = deal[p]
        self.lens = np.zeros((pieces, stride), np.uint32)
        for p in range(pieces):
            self.lens[p, :n] = [len(x) for x in lists[p]]
        flat = [x for p in range(pieces) for x in lists[p]]
        self.ids = np.concatenate(flat).astype(np.uint32) if flat else np.zeros(0, np.uint32)
        self.lists = lists

    def classify(self):
        """The scan forms run_merge_rows takes (the (piece, row) offsets over P * stride lengths,
        the merged rows' offsets over n) and the row shapes present."""
        return {"scan_lists": scan_form(self.pieces * self.stride), "scan_rows": scan_form(self.n),
                "n_lists": self.pieces * self.stride, "padded": self.stride > self.n,
                "shapes": set(s if not s.startswith("only_") else "only" for s in self.shapes),
                "blocks": (self.n + 255) // 256}


@functools.lru_cache(maxsize=None)
def merge_world(n, stride, pieces):
    return MergeWorld(n, stride, pieces)


# ---------------------------------------------------------------------------
# classify: which paths of the kernels a case takes, from its arrays alone
# ---------------------------------------------------------------------------
def small_capacity(nnz, total):
    """The speculative capacity of a small host fan-out once the context's deliveries per
    match are this case's own (its second call): None when the call takes the ordinary path."""
    spm = max(1.0, total / nnz) if nnz else 1.0
    want = 1024.0 + nnz * spm * 1.25
    if want > SMALL_MAX_DELIVERIES:
        return None
    cap = 1024
    while cap < want:
        cap <<= 1
    return cap


def classify_launch(lens, glo, ghi, per):
    """One k_fanout_copy launch over deliveries [glo, ghi), `per` per workgroup."""
    lens = np.asarray(lens, np.int64)
    nseg = len(lens)
    dst = np.zeros(nseg + 1, np.int64)
    np.cumsum(lens, out=dst[1:])
    total = int(dst[-1])
    out = {"per_block": per, "empties": set(), "single_tails": set(), "cross_seg": set(), "cross_end": set(),
           "n_ranges": 0}
    if ghi <= glo:
        return out
    los = np.arange(glo, ghi, per, dtype=np.int64)
    his = np.minimum(los + per, ghi)
    out["n_ranges"] = len(los)
    # the workgroup's search: the last segment whose start <= x
    s0 = np.searchsorted(dst, los, side="right") - 1
    s1 = np.searchsorted(dst, his - 1, side="right") - 1
    assert (lens[s0] > 0).all() and (lens[s1] > 0).all()
    # ... which has to step over a run of zero-length segments with the same start
    first = (dst[s0] == los) & (s0 > 0) & (lens[np.maximum(s0 - 1, 0)] == 0)
    nxt = np.minimum(s1 + 1, nseg - 1)
    last = (s1 + 1 < nseg) & (dst[nxt] == his) & (lens[nxt] == 0)
    if (first & (los == 0)).any():
        out["empties"].add("start")
    if (first & (los > 0)).any():
        out["empties"].add("after_boundary")
    if (last & (his == total)).any():
        out["empties"].add("end")
    if (last & (his < total)).any():
        out["empties"].add("before_boundary")
    single = s0 == s1
    out["single_tails"] = set(((his - los)[single] % GROUP).tolist())
    out["cross_end"] = set(((his - los)[~single] % GROUP).tolist()) - {0}
    # a 4-element group of a many-segment range with a segment start inside it
    b = np.unique(dst[1:nseg])
    b = b[(b > glo) & (b < ghi)]
    lo_of = glo + (b - glo) // per * per
    out["cross_seg"] = set(((b - lo_of) % GROUP).tolist()) - {0}
    return out


def classify(case, part=0, n_parts=1):
    """The paths `case` takes: the scan form of each driver, and for part `part` of `n_parts`
    of the ordinary driver (the whole fan-out by default) and for the small host driver's one
    launch: the workgroup ranges' searches next to zero-length segments, the single-segment
    ranges' tails, the 4-element groups across a segment start or the end, and the cut."""
    lens = case.seg_lens()
    nnz, total = case.nnz, int(lens.sum())
    glo, ghi = part_range(total, part, n_parts)
    out = {"nnz": nnz, "total": total, "n_rows": case.n_rows, "scan": scan_form(nnz)}
    out["launch"] = classify_launch(lens, glo, ghi, fan_per_block(ghi - glo))
    dst = np.zeros(nnz + 1, np.int64)
    np.cumsum(lens, out=dst[1:])
    at = np.flatnonzero(dst[:nnz] == glo)
    out["cut"] = {"glo_mod": glo % GROUP, "empty_part": ghi == glo, "on_seg_start": len(at) > 0,
                  "empties_at_cut": bool(len(at) and (lens[at] == 0).any() and (lens[at] > 0).any())}
    cap = small_capacity(nnz, total) if case.n_rows < SMALL_MAX_ROWS else None
    out["small"] = None
    if cap is not None:  # (the launch is sized by the capacity and clamped to the total on the device)
        out["small"] = {"scan": scan_form_small(nnz), "capacity": cap,
                        "launch": classify_launch(lens, 0, total, fan_per_block(cap))}
    return out
