"""The shared-subscription table on the host alone: the compiler
(emqx_amd/csrc/gm_shared.cpp) and the host walk (emqx_gm_shared_pick_host)
against the restatement of emqx_shared_sub:pick/6 (tests/_shared_ref.py).
No device is needed.  All comparisons are exact."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _shared_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRATEGIES = ["hash", "round_robin", "sticky", "random"]


def _table(filters, slots, prev=None):
    from emqx_amd import SharedTable
    return SharedTable.compile_host(filters, slots, prev)


def _pick(t, rows, strategy, hashes=None, seed=0):
    ro, mem, slots = t.pick_host(R.csr_of(rows), strategy, hashes, seed)
    return [int(x) for x in ro], [int(x) for x in mem], [int(x) for x in slots]


def test_build_rules_sort_merge_dedupe_drop():
    filters = [b"b/+", b"a/#", b"c", b"a/#"]  # ids: a/# 0, b/+ 1, c 2
    slots = [(b"c", 5, [9, 9, 8]), (b"a/#", 7, [1]), (b"a/#", 2, [3, 4]), (b"b/+", 0, []), (b"c", 5, [8, 7, 9]),
             (b"a/#", 7, [1, 2])]
    t = _table(filters, slots)
    ref = R.Table(filters, slots)
    assert t.slots() == ref.slot_list() == [(0, 2, [3, 4]), (0, 7, [1, 2]), (2, 5, [9, 8, 7])]
    i = t.info()
    assert (i.n_slots, i.n_members, i.n_filters_with_slots, i.device_bytes) == (3, 7, 2, 0)
    # ids are the ones emqx_gm_index_compile_host assigns
    from emqx_amd import _lib, pack
    fb, fo = pack(filters)
    perm = np.zeros(len(filters), np.uint32)
    info = _lib.IndexInfo()
    assert _lib.lib().emqx_gm_index_compile_host(C.c_void_p(fb.ctypes.data), C.c_void_p(fo.ctypes.data), len(filters),
                                                 None, None, C.c_void_p(perm.ctypes.data), C.byref(info)) == 0
    assert perm.tolist() == [1, 0, 2, 0]
    t.release()
    empty = _table(filters, [])
    assert empty.info().n_slots == 0 and _pick(empty, [[0, 1], []], "round_robin") == ([0, 0, 0], [], [])
    empty.release()


def test_refusals():
    from emqx_amd import GpuMatchError, _lib, pack
    filters = [b"a/#", b"b/+"]
    with pytest.raises(GpuMatchError) as e:
        _table(filters, [(b"a/#", 0, [1]), (b"nope/+", 0, [2])])
    assert e.value.code == _lib.EINVAL and "nope/+" in str(e.value)
    with pytest.raises(GpuMatchError) as e:
        _table(filters, [(b"a/#", 0, [0xFFFFFFFF])])
    assert e.value.code == _lib.EINVAL
    L = _lib.lib()
    ifb, ifo = pack(filters)
    fb, _ = pack([b"a/#", b"b/+"])
    gid = np.zeros(2, np.uint32)
    mi = np.array([1, 2], np.uint32)
    good_mo = np.array([0, 1, 2], np.uint64)
    h = C.c_void_p()

    def compile_(fo, mo):
        fo, mo = np.array(fo, np.uint64), np.array(mo, np.uint64)
        return L.emqx_gm_shared_compile_host(C.c_void_p(ifb.ctypes.data), C.c_void_p(ifo.ctypes.data), 2,
                                             C.c_void_p(fb.ctypes.data), C.c_void_p(fo.ctypes.data),
                                             C.c_void_p(gid.ctypes.data), 2, C.c_void_p(mo.ctypes.data),
                                             C.c_void_p(mi.ctypes.data), None, C.byref(h))
    for fo in ([0, 4, 2], [0, 3, 2**40]):  # descending; an entry far past the buffer
        assert compile_(fo, good_mo) == _lib.EINVAL and not h.value
        assert b"offsets" in L.emqx_gm_last_error(None)
    assert compile_([0, 3, 6], [0, 2, 1]) == _lib.EINVAL and not h.value  # descending member offsets
    assert compile_([0, 3, 6], good_mo) == 0 and h.value
    L.emqx_gm_shared_release(h)
    # the rows of a pick
    t = _table(filters, [(b"a/#", 0, [1, 2])])
    with pytest.raises(GpuMatchError) as e:
        t.pick_host(([0, 1], [2]), "random")  # an id >= n_filters
    assert e.value.code == _lib.EINVAL
    with pytest.raises(GpuMatchError) as e:
        t.pick_host(([0, 2, 1, 2], [0, 0]), "random")  # offsets not ascending
    assert e.value.code == _lib.EINVAL
    with pytest.raises(GpuMatchError) as e:
        t.pick_host(([0, 1], [0]), "hash", None)  # HASH without msg_hash
    assert e.value.code == _lib.EINVAL and "msg_hash" in str(e.value)
    with pytest.raises(GpuMatchError) as e:
        t.pick(([0, 1], [0]), "random")  # a host-only table has no device side
    assert e.value.code == _lib.EUNSUPPORTED
    t.release()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_strategies_on_a_random_set(strategy):
    filters, slots, rows, _ = R.random_case(3)
    t, ref = _table(filters, slots), R.Table(filters, slots)
    assert t.slots() == ref.slot_list()
    hashes = [(r * 2654435761 + 12345) & R.M32 for r in range(len(rows))]
    hits = 0
    for call in range(3):  # state carries from call to call
        seed = 77 + call
        want = ref.pick(rows, strategy, hashes, seed)
        got = _pick(t, rows, strategy, hashes if strategy == "hash" else None, seed)
        assert got[0] == want[0] and got[2] == want[2]
        assert got[1] == want[1]
        hits += len(got[1])
    assert hits > 1000
    t.release()


def test_hash_edges_and_single_member():
    filters = [b"a", b"b", b"c"]
    slots = [(b"a", 0, [10]), (b"b", 0, [20, 21, 22]), (b"b", 1, [30, 31])]
    t, ref = _table(filters, slots), R.Table(filters, slots)
    rows = [[0, 1], [], [1], [2], [0, 1, 2]]
    for h in (0, 1, 2, 3, 2**27 - 1, 2**32 - 1):  # 0, Count - 1, Count (for 2 and 3), large
        hs = [h] * len(rows)
        assert _pick(t, rows, "hash", hs) == tuple(ref.pick(rows, "hash", hs))
    ro, mem, sl = _pick(t, rows, "hash", [2**32 - 1] * 5)
    assert ro == [0, 3, 3, 5, 5, 8] and sl == [0, 1, 2, 1, 2, 0, 1, 2]
    assert mem[:3] == [10, 20 + (2**32 - 1) % 3, 30 + (2**32 - 1) % 2]
    # a slot of one member reads and writes no round-robin state: after the call a second member
    # joins and the start comes from the seed, not from a stored Rem
    _pick(t, [[0]] * 5, "round_robin", seed=1)
    ref.pick([[0]] * 5, "round_robin", seed=1)
    slots2 = slots + [(b"a", 0, [11, 12])]
    t2, ref2 = _table(filters, slots2, t), R.Table(filters, slots2, ref)
    got, want = _pick(t2, [[0]] * 4, "round_robin", seed=5), ref2.pick([[0]] * 4, "round_robin", seed=5)
    assert got == tuple(want) and got[1][0] == [10, 11, 12][R.mix(5, 0) % 3]
    t.release()
    t2.release()


def test_carry_over_with_prev():
    f1 = [b"m/+", b"n/#", b"z"]
    s1 = [(b"m/+", 0, [1, 2, 3, 4, 5]), (b"n/#", 3, [7, 8, 9]), (b"z", 1, [20, 21])]
    t, ref = _table(f1, s1), R.Table(f1, s1)
    rows = [[0, 1, 2], [0], [0, 1], [0]]  # m/+ hit 4 times, n/# twice, z once

    def both(tt, rr, rows_, strategy, seed):
        got, want = _pick(tt, rows_, strategy, seed=seed), rr.pick(rows_, strategy, seed=seed)
        assert got == tuple(want)
        return got
    both(t, ref, rows, "round_robin", 11)
    both(t, ref, rows, "sticky", 12)
    sticky_m = ref.pd[("st", (0, b"m/+"))]
    # (a) a member added to m/+; (b) members removed from it so that rr >= Count; the snapshot gained
    # filters in front, so every id shifted; z's slot dropped
    f2 = [b"a/0", b"a/1"] + f1
    while True:  # drive m/+'s rr to 4, the last index of five
        if ref.pd[("rr", (0, b"m/+"))] == 4:
            break
        both(t, ref, [[0]], "round_robin", 11)
    s2 = [(b"m/+", 0, [1, 2]), (b"n/#", 3, [7, 8, 9, 10])]
    t2, ref2 = _table(f2, s2, t), R.Table(f2, s2, ref)
    assert t2.slots() == ref2.slot_list() == [(2, 0, [1, 2]), (3, 3, [7, 8, 9, 10])]
    rows2 = [[2, 3], [2], [3, 2]]
    got = both(t2, ref2, rows2, "round_robin", 13)
    assert got[1][0] == [1, 2][(4 + 1) % 2]  # (rr + 1) rem Count with the CURRENT Count
    got = both(t2, ref2, rows2, "sticky", 14)
    if sticky_m not in (1, 2):
        assert got[1][0] == [1, 2][R.mix(14, 0) % 2]  # the sticky member left: a new one from the seed
    else:
        assert got[1][0] == sticky_m
    # n/#'s sticky member stayed listed: kept although the filter's id shifted
    assert got[1][1] == ref.pd[("st", (3, b"n/#"))]
    # (c) z re-added: it was absent from t2, so its state starts unset
    s3 = s2 + [(b"z", 1, [20, 21])]
    t3, ref3 = _table(f2, s3, t2), R.Table(f2, s3, ref2)
    got = both(t3, ref3, [[4], [4]], "round_robin", 15)
    assert got[1] == [[20, 21][R.mix(15, 2) % 2], [20, 21][(R.mix(15, 2) + 1) % 2]]
    both(t3, ref3, [[4], [2, 3, 4]], "sticky", 16)
    # prev itself is not modified
    assert _pick(t, [[0]], "round_robin", seed=0)[1] == [1]  # (4 + 1) rem 5
    for x in (t, t2, t3):
        x.release()


def test_sticky_member_removed_is_dropped():
    f = [b"s/#"]
    t, ref = _table(f, [(b"s/#", 0, [5, 6, 7])]), R.Table(f, [(b"s/#", 0, [5, 6, 7])])
    first = _pick(t, [[0], [0]], "sticky", seed=21)[1]
    assert first == ref.pick([[0], [0]], "sticky", seed=21)[1] and first[0] == first[1]
    rest = [m for m in (5, 6, 7) if m != first[0]]
    t2, ref2 = _table(f, [(b"s/#", 0, rest)], t), R.Table(f, [(b"s/#", 0, rest)], ref)
    got = _pick(t2, [[0], [0]], "sticky", seed=22)[1]
    assert got == ref2.pick([[0], [0]], "sticky", seed=22)[1] == [rest[R.mix(22, 0) % 2]] * 2
    t.release()
    t2.release()


def test_compiler_and_host_walk_under_asan():
    """tests/asan/asan_shared.cpp: gm_shared.cpp as host C++ under
    AddressSanitizer + UBSan, run as a plain executable (nothing preloaded)."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "asan-shared"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "asan_shared")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "asan_shared ok" in p.stdout


def test_batcher_shared_argument_with_stand_in_collaborators():
    """PublishBatcher(shared=...): one dispatch_batch per window, the picked member delivered to, the
    rest of subscribers/2 tried when it is down, shared_dispatch for a group the table does not hold;
    without shared= the per-message callback as before.  (Stand-ins for GpuRoutes and SharedSub: the
    device path is tests/test_gpu_shared.py's.)"""
    from emqx_amd.batcher import PublishBatcher

    class Routes:
        other = {b"s/#": 1}
        subs = {}

        def groups_rows(self, topics):
            return [[(b"s/#", [])] for _ in topics], "idx", ([0, 1, 2], [0, 0])

        def groups(self, topics):
            return self.groups_rows(topics)[0]

    class Shared:
        calls = []

        def dispatch_batch(self, index, rows, strategy, hashes=None):
            self.calls.append((index, strategy, hashes))
            return [[(b"g", b"s/#", down)], [(b"g", b"s/#", up)]]

        def subscribers(self, group, f):
            return [down, up]
    down, up, log = "down", "up", []

    def deliver(sub, f, msg):
        log.append((sub, f, msg))
        return sub == "up"
    lookup = lambda f: [(b"g", b"n2"), (b"h", b"n2")]  # noqa: E731
    per_msg = []
    kw = dict(routes=Routes(), timer=False, lookup_routes=lookup, deliver=deliver,
              shared_dispatch=lambda g, f, m: per_msg.append((g, f, m)) or ("ok", 1))
    with pytest.raises(TypeError):
        PublishBatcher(groups_fn=lambda t: [], timer=False, shared=Shared())
    sh = Shared()
    pb = PublishBatcher(shared=sh, shared_strategy="hash_topic", shared_hash=lambda t, m: len(t), **kw)
    out = pb.publish_batch([(b"s/1", "m1"), (b"s/22", "m2")])
    assert sh.calls == [("idx", "hash_topic", [3, 4])]
    assert log == [("down", b"s/#", "m1"), ("up", b"s/#", "m1"), ("up", b"s/#", "m2")]  # FailedSubs: the next member
    assert per_msg == [(b"h", b"s/#", "m1"), (b"h", b"s/#", "m2")]  # no pick for group h: the callback
    assert out[0] == [("share", b"s/#", ("ok", 1)), ("share", b"s/#", ("ok", 1))]
    del log[:], per_msg[:]
    pb = PublishBatcher(**kw)  # absent: exactly the per-message path
    pb.publish_batch([(b"s/1", "m1")])
    assert log == [] and per_msg == [(b"g", b"s/#", "m1"), (b"h", b"s/#", "m1")]
