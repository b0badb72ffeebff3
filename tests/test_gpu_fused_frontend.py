"""k_match_fused's front end (gm_match.hip): the lanes' offsets and the block's
two bounding offsets are loaded together at entry, and the block's text goes to
LDS through range-checked 16-byte buffer loads that are all in flight before
the first LDS write (stage_text).

The shapes are the smallest at which that can go wrong: blocks whose text is at
the staging limit and at the unrolled loads' boundary, every start alignment of
a block, batches that end inside a tile or a block, a poisoned pad after the
text, and awkward bytes across block boundaries.  Every row is compared with
the CPU oracle, in both `exact` modes."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# A block's staged extent is toff[end of block] - (toff[first topic] & ~7).
UNIT = 256      # topics per block
LIMIT = 16376   # the largest staged extent: TOK_STAGE - 8
FIRST = 8192    # the unrolled first loads cover this much; the loaded size is round8(extent) + 8
TRIP = 4096     # one load of the block: 256 lanes x 16 bytes


@pytest.fixture(scope="module")
def ctx():
    from emqx_amd import Context
    c = Context(0)
    yield c
    c.close()


def _tok_words():
    """The words of test_tokenizer_alignments_and_bytes: every length 0..19 over
    bytes next to '/' in value, NUL and 0xFF."""
    rng = random.Random(17)
    alphabet = [b".", b"0", b"a", b"\x00", b"\xff", b"\x2e", b"\x30", b"z"]
    return [b"".join(rng.choice(alphabet) for _ in range(k)) for k in range(20) for _ in range(3)]


class World:
    """One index (2,000 seeded mixed filters and the awkward-byte filters), the
    oracle's routers for both modes built once, and a pool of matching topics."""

    def __init__(self, ctx, orc):
        from emqx_amd.engine import gen_filter_codes, render_codes
        self.ctx, self.orc = ctx, orc
        codes = gen_filter_codes(11, 2000)
        fs = set(orc.unpack(*render_codes(codes)))
        self.words = _tok_words()
        for w in self.words:
            fs.update((w + b"/+", b"+/" + w, w + b"/#", w))
        self.filters = sorted(fs)
        self.idx = ctx.build_index(self.filters)
        self.routers = {}
        for mode in (1, 0):
            r = orc.Router(True)
            for f in self.filters:
                if mode == 1:
                    r.add_route(f)
                else:
                    r.trie.insert(f)
            self.routers[mode] = r
        self.ranker = orc.Ranker(self.filters)
        self.pool = orc.unpack(*orc.render_codes(orc.gen_topic_codes(3, 0, 6000, codes)))
        self.short = sorted(self.pool, key=len)[:1500]
        random.Random(1).shuffle(self.short)

    def oracle(self, topics, exact):
        ro, ids, _ = self.routers[1 if exact else 0].match_batch(topics, self.ranker, mode=1 if exact else 0)
        return ro, ids

    def check(self, topics, what=""):
        for exact in (True, False):
            _assert_rows(self.ctx.match(self.idx, topics, exact=exact), self.oracle(topics, exact), topics, (what, exact))

    def match_device(self, data, off, n, exact, shift=0):
        """Match a batch whose text buffer the test lays out itself: `data` (the
        text and whatever follows it) copied `shift` bytes into a device buffer."""
        ctx = self.ctx
        d_tb, d_to = ctx.dev_alloc(len(data) + shift), ctx.dev_alloc(len(off) * 8)
        try:
            ctx.memcpy_h2d(d_tb + shift, data, len(data))
            ctx.memcpy_h2d(d_to, off, len(off) * 8)
            res = ctx.match_device(self.idx, d_tb + shift, d_to, n, exact=exact)
            out = res.to_host()
            res.free()
            return out
        finally:
            ctx.dev_free(d_tb)
            ctx.dev_free(d_to)


@pytest.fixture(scope="module")
def world(ctx, orc):
    w = World(ctx, orc)
    yield w
    w.idx.release()


def _assert_rows(got, want, topics, what):
    (ro, ids), (oro, oids) = got, want
    if np.array_equal(ro, oro) and np.array_equal(ids, oids):
        return
    for i in range(len(topics)):
        g, e = ids[int(ro[i]):int(ro[i + 1])].tolist(), oids[int(oro[i]):int(oro[i + 1])].tolist()
        assert g == e, (what, i, topics[i][:80], g, e)
    raise AssertionError((what, "row offsets differ"))


class Batch:
    """A batch built block by block, tracking the byte offset of the next topic."""

    def __init__(self, world, seed=0):
        self.w, self.t, self.off = world, [], 0
        self.rng = random.Random(seed)

    def add(self, topics):
        for x in topics:
            self.t.append(x)
            self.off += len(x)

    def real(self, k, budget=None, pool=None):
        """k matching topics (of at most `budget` bytes together)."""
        out, used = [], 0
        while len(out) < k:
            x = self.rng.choice(pool or (self.w.short if budget is not None else self.w.pool))
            if budget is not None and used + len(x) > budget:
                x = b""
            out.append(x)
            used += len(x)
        return out

    def block(self, extent, tail=None, filler=b"x"):
        """A whole block of staged extent `extent`: a filler topic first, then
        empties and matching topics, the last of which ends at the extent."""
        assert len(self.t) % UNIT == 0
        text = extent - (self.off & 7)
        tail = sorted(self.real(UNIT - 1, text * 2 // 3), key=len) if tail is None else tail
        assert len(tail) == UNIT - 1 and len(tail[-1]) > 0
        fill = text - sum(map(len, tail))
        assert fill >= 0, (extent, text, fill)
        off0 = self.off
        self.add([(filler * fill)[:fill]] + tail)
        assert self.off - (off0 & ~7) == extent
        return self

    def plain(self, k=UNIT):
        self.add(self.real(k))
        return self


@pytest.mark.parametrize("start", [0, 5], ids=["aligned", "start+5"])
def test_staging_limit(world, start):
    """Blocks exactly at, one byte under and one byte over the staging limit,
    between ordinary blocks (staged and unstaged blocks in one batch), for a
    block start on and off an 8-byte word."""
    b = Batch(world, start)
    b.add([b"s" * start] + b.real(UNIT - 1))
    for extent in (LIMIT, LIMIT - 1, LIMIT + 1, LIMIT - 8, LIMIT + 8, 2 * LIMIT):
        b.block(extent)
        b.add(b.real(63) + [b"p" * ((start - b.off) % 8)] + [b""] * (UNIT - 64))   # the next block starts at `start` mod 8 again
    b.plain(40)
    world.check(b.t, ("limit", start))


def test_empty_and_long_topics(world):
    """A tile and a block of empty topics, one 6 KB topic among empties (it
    fits the block's LDS), one 17 KB topic among empties (it does not: the
    unstaged path), long topics first and last in their blocks."""
    real = world.pool[7]
    long1 = real + b"/" + b"w" * (6000 - len(real) - 1)
    long2 = b"/".join([b"L" * 1500] * 4)
    long3 = real + b"/" + b"/".join([b"M" * 4250] * 4)
    b = Batch(world, 2)
    b.plain(64)
    b.add([b""] * 64)
    b.add([b""] * 20 + [long1] + [b""] * 43)
    b.add([b""] * 63 + [long2])
    b.add([b""] * UNIT)
    b.add([long2] + [b""] * 63)
    b.add([b""] * 100 + [long3] + [b""] * 91)
    b.add([long3] + [b""] * (UNIT - 2) + [long1])
    b.plain(30)
    b.add([b""] * 34)
    b.add([b""] * 7)
    world.check(b.t, "empty/long")


def test_unroll_boundary(world):
    """Block text at the bytes the unrolled loads cover, one byte more and one
    less (the loaded size is round8(extent) + 8, so the second group of loads
    starts at extent 8,185), and at each single load's edge."""
    b = Batch(world, 3)
    for edge in (FIRST, FIRST - 8, TRIP - 8, 3 * TRIP - 8):
        for d in (-1, 0, 1):
            b.block(edge + d)
        b.plain(64)
        b.add([b""] * (UNIT - 64))
    world.check(b.t, "unroll")


@pytest.mark.parametrize("shift", [0, 8], ids=["tb16", "tb8"])
def test_block_start_alignment(world, shift):
    """A block's first topic at every offset 0..15 modulo 16: a filler topic of
    0..15 bytes ends the previous block.  Block 0 starts at the buffer's first
    byte, with the text buffer on a 16-byte and on an 8-byte address."""
    b = Batch(world, 4)
    for a in list(range(16)) + [0]:
        b.add(b.real(63) + [b""] * (UNIT - 64))
        b.add([b"z" * ((a - b.off) % 16)])
        assert b.off % 16 == a
    b.plain(17)
    from emqx_amd.engine import pack
    data, off = pack(b.t)
    for exact in (True, False):
        _assert_rows(world.match_device(data, off, len(b.t), exact, shift), world.oracle(b.t, exact), b.t, ("align", exact))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 255, 256, 257])
def test_partly_filled_blocks(world, n):
    """Batches ending inside a tile and inside a block: the waves wholly past n
    take the block's barriers and leave, the lanes past n load the last
    topic's offsets and nothing else."""
    topics = Batch(world, 5).plain(257).t[:n]
    world.check(topics, ("n", n))


@pytest.mark.parametrize("tail,empty_last", [(0, False), (1, False), (7, False), (0, True), (3, True)],
                         ids=["tail0", "tail1", "tail7", "tail0-empty", "tail3-empty"])
def test_poisoned_pad(world, tail, empty_last):
    """The same device-buffer batch matched with the 64 bytes after the text
    zero and with topic-like garbage there: identical rows, the oracle's.  The
    last topic with text matches filters and ends `tail` bytes past an 8-byte
    word; an empty topic may follow it."""
    from emqx_amd.engine import pack
    b = Batch(world, 6)
    b.plain(256 + 37)
    last = b.rng.choice(world.pool)
    b.add([b"t" * ((tail - b.off - len(last)) % 8), last] + ([b""] if empty_last else []))
    data, off = pack(b.t)
    n, end = len(b.t), int(off[-1])
    assert end % 8 == tail
    assert len(data) == end + 64
    poison = data.copy()
    poison[end:] = np.frombuffer((b"/a/+/#/" + world.pool[1] + b"/" + world.pool[2] + b"/" * 64)[:64], np.uint8)
    for exact in (True, False):
        want = world.oracle(b.t, exact)
        zero = world.match_device(data, off, n, exact)
        bad = world.match_device(poison, off, n, exact)
        _assert_rows(zero, want, b.t, ("zero pad", exact))
        _assert_rows(bad, want, b.t, ("poisoned pad", exact))
        assert np.array_equal(zero[0], bad[0]) and np.array_equal(zero[1], bad[1])


def test_pathological_text_across_edges(world):
    """The awkward words (NUL, 0xFF, bytes next to '/') as the last topics of a
    block and the first of the next, with the block at the staging limit, one
    over it, at the unrolled loads' boundary, and ordinary."""
    rng = random.Random(8)
    ws = world.words

    def odd(k):
        out = []
        for _ in range(k):
            a, c = rng.choice(ws), rng.choice(ws)
            out.append(rng.choice([a + b"/" + c, a, b"/" + a + b"/" + c, a + b"/"]))
        return out

    b = Batch(world, 7)
    for extent in (LIMIT, LIMIT + 1, LIMIT - 1, FIRST, FIRST + 1, 12000, 3000):
        tail = [b""] * (UNIT - 1 - 100) + odd(100)
        while not tail[-1]:
            tail[-1] = rng.choice(ws)
        b.block(extent, tail=tail, filler=rng.choice(ws[30:]) + b"/")
        b.add(odd(64) + [b""] * (UNIT - 64))
    world.check(b.t, "pathological")
