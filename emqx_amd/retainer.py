"""Retained-message lookup: which stored topics does a subscribe filter match.

``RetainedIndex`` wraps the library's retained-topic index
(emqx_gm_retained_*, include/emqx_gpu_match.h): the stored topics compiled into
a level trie in HBM and batches of filters walked against it by the gfx950
kernels of gm_retained.hip.  ``Retainer`` is the host mirror of the
``emqx_retainer`` storage behaviour (apps/emqx_retainer/src/emqx_retainer.erl:65-73,
emqx_retainer_mnesia.erl:74-165) on top of it.  The reference answers a
subscription with a scan of the whole table (match_messages/1 + condition/1,
emqx_retainer_mnesia.erl:210-244).  There is no '$'-rule on this side: ``#``
matches ``$SYS/...`` topics.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Csr, GpuMatchError, RetainedInfo, check, lib
from .engine import BytesLike, _b, _csr_to_numpy, _ptr, pack


class RetainedIndex:
    """One retained-topic index.  Made by ``Context.build_retained`` (resident
    in HBM) or ``RetainedIndex.compile_host`` (host tables only: ``match_host``
    works, ``match`` and ``expire`` raise)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def compile_host(cls, topics, ids=None, expiry_ms=None) -> "RetainedIndex":
        tb, to, ia, ea = _build_args(topics, ids, expiry_ms)
        h = C.c_void_p()
        rc = lib().emqx_gm_retained_compile_host(_ptr(tb), _ptr(to), len(to) - 1, _ptr(ia), _ptr(ea), C.byref(h))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "retained_compile_host")
        return cls(None, h)

    def match(self, filters, now_ms: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Batch emqx_retainer_mnesia:match_messages/1: CSR (row_off uint64[n+1],
        the caller's ids uint32) of the stored topics each filter matches, each
        row in word-list order of the topics."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "retained match: a host-only index")
        return self._match(filters, now_ms, 0)

    def match_timed(self, filters, now_ms: int = 0):
        """``match`` with its passes timed: (row_off, ids, (count ms, scan ms, fill ms))."""
        ro, ids = self._match(filters, now_ms, _lib.RET_TIMED)
        ms = (C.c_double * 3)()
        check(lib().emqx_gm_retained_last_times(self.h, ms), self.ctx.h, "retained_last_times")
        return ro, ids, tuple(ms)

    def _match(self, filters, now_ms, flags):
        fb, fo = filters if isinstance(filters, tuple) else pack(filters)
        csr = Csr()
        check(lib().emqx_gm_retained_match(self.ctx.h, self.h, _ptr(fb), _ptr(fo), len(fo) - 1, int(now_ms), flags,
                                           C.byref(csr)), self.ctx.h, "retained_match")
        try:
            return _csr_to_numpy(csr)
        finally:
            lib().emqx_gm_csr_free(self.ctx.h, C.byref(csr))

    def match_host(self, filters, now_ms: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The same walk over the host copy of the tables (single thread, no
        device call): test and measurement support."""
        fb, fo = filters if isinstance(filters, tuple) else pack(filters)
        csr = Csr()
        rc = lib().emqx_gm_retained_match_host(self.h, _ptr(fb), _ptr(fo), len(fo) - 1, int(now_ms), C.byref(csr))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "retained_match_host")
        try:
            return _csr_to_numpy(csr)
        finally:
            lib().emqx_gm_retained_csr_free_host(C.byref(csr))

    def expire(self, topics, expiry_ms) -> int:
        """Set the expiry of the stored ones among ``topics`` (in place, in
        stream order with matches); returns how many were stored.
        ``expiry_ms``: one value for all, or one per topic."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "retained expire: a host-only index")
        tb, to = topics if isinstance(topics, tuple) else pack(topics)
        n = len(to) - 1
        ex = np.full(n, expiry_ms, np.uint64) if np.isscalar(expiry_ms) else np.ascontiguousarray(expiry_ms, np.uint64)
        if len(ex) != n:
            raise ValueError("one expiry per topic")
        if len(ex) == 0:
            ex = np.zeros(1, np.uint64)
        found = C.c_uint64()
        check(lib().emqx_gm_retained_expire(self.ctx.h, self.h, _ptr(tb), _ptr(to), n, _ptr(ex), C.byref(found)),
              self.ctx.h, "retained_expire")
        return int(found.value)

    def info(self) -> RetainedInfo:
        info = RetainedInfo()
        check(lib().emqx_gm_retained_info(self.h, C.byref(info)), None, "retained_info")
        return info

    def release(self):
        if self.h:
            lib().emqx_gm_retained_release(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.release()
        except Exception:
            pass


def _build_args(topics, ids, expiry_ms):
    tb, to = topics if isinstance(topics, tuple) else pack(topics)
    n = len(to) - 1
    ia = ea = None
    if ids is not None:
        ia = np.ascontiguousarray(ids, np.uint32)
        if len(ia) != n:
            raise ValueError("one id per topic")
        if n == 0:
            ia = np.zeros(1, np.uint32)
    if expiry_ms is not None:
        ea = np.ascontiguousarray(expiry_ms, np.uint64)
        if len(ea) != n:
            raise ValueError("one expiry per topic")
        if n == 0:
            ea = np.zeros(1, np.uint64)
    return tb, to, ia, ea


def build_retained(ctx, topics, ids=None, expiry_ms=None) -> RetainedIndex:
    """``Context.build_retained``: the table as store_retained/2 leaves it
    (duplicates allowed, the last one's id and expiry kept)."""
    tb, to, ia, ea = _build_args(topics, ids, expiry_ms)
    h = C.c_void_p()
    check(lib().emqx_gm_retained_build(ctx.h, _ptr(tb), _ptr(to), len(to) - 1, _ptr(ia), _ptr(ea), 0, C.byref(h)),
          ctx.h, "retained_build")
    return RetainedIndex(ctx, h)


def _wildcard(topic: bytes) -> bool:
    """emqx_topic:wildcard/1: a '+' or '#' word."""
    return any(w in (b"+", b"#") for w in topic.split(b"/"))


class Retainer:
    """Host mirror of the emqx_retainer storage behaviour over the device
    index: a main index plus a small delta index of the topics stored since the
    main was built.  Every match goes through the device; the host keeps the
    messages and applies no topic algebra of its own.

    A topic keeps its place in its index when its message is deleted or
    replaced: a delete sets its expiry to 1 and a store on a known topic sets
    the new expiry (emqx_gm_retained_expire), so matches run with
    ``now_ms >= 1`` and an expiry of exactly 1 means deleted."""

    DELTA_MIN = 1024

    def __init__(self, ctx):
        self.ctx = ctx
        self._main: Optional[RetainedIndex] = None
        self._delta: Optional[RetainedIndex] = None
        self._topics: List[bytes] = []          # slot -> topic (main slots first, then delta slots)
        self._n_main = 0                        # slots [0, _n_main) are in the main index
        self._slot: Dict[bytes, int] = {}       # topic -> slot (deleted topics keep theirs)
        self._live: Dict[int, Tuple[object, int]] = {}  # slot -> (message, expiry_ms)
        self._delta_dirty = False
        self.compactions = 0

    # -- emqx_retainer_mnesia:store_retained/2 (:74-104)
    def store_retained(self, topic: BytesLike, msg, expiry_ms: int = 0):
        t = _b(topic)
        s = self._slot.get(t)
        if s is None:
            s = len(self._topics)
            self._topics.append(t)
            self._slot[t] = s
            self._delta_dirty = True  # the delta is rebuilt before the next match
        elif s < self._n_main:
            self._main.expire([t], int(expiry_ms))
        elif not self._delta_dirty:
            self._delta.expire([t], int(expiry_ms))
        self._live[s] = (msg, int(expiry_ms))
        if len(self._topics) - self._n_main > max(self.DELTA_MIN, self._n_main // 8):
            self._compact()

    # -- emqx_retainer_mnesia:delete_message/2 (:117-128); a wildcard deletes all it matches
    #    (match_delete_messages/1, :216-222)
    def delete_message(self, topic_or_filter: BytesLike):
        t = _b(topic_or_filter)
        if _wildcard(t):
            self._sync()
            victims = [self._topics[s] for s in self._match_slots([t], 1)[0]]
        else:
            victims = [t] if t in self._slot else []
        main = [v for v in victims if self._slot[v] < self._n_main]
        delta = [v for v in victims if self._slot[v] >= self._n_main]
        if main:
            self._main.expire(main, 1)
        if delta and not self._delta_dirty:
            self._delta.expire(delta, 1)
        for v in victims:
            self._live.pop(self._slot[v], None)

    # -- emqx_retainer_mnesia:read_message/2 (:130-131, read_messages/1 :199-208: a key read, Et >= now)
    def read_message(self, topic: BytesLike, now_ms: int = 0) -> list:
        e = self._live.get(self._slot.get(_b(topic), -1))
        if e is None or not (e[1] == 0 or e[1] >= now_ms):
            return []
        return [e[0]]

    # -- emqx_retainer_mnesia:match_messages/3 (:146-158), batched over filters
    def match_messages(self, filters: Sequence[BytesLike], now_ms: int = 0) -> List[List[Tuple[bytes, object]]]:
        """Per filter, the (topic, message) pairs it matches: the main index's
        part followed by the delta's, each in topic order."""
        self._sync()
        rows = self._match_slots([_b(f) for f in filters], max(int(now_ms), 1))
        return [[(self._topics[s], self._live[s][0]) for s in row] for row in rows]

    def clean(self):
        for ix in (self._main, self._delta):
            if ix is not None:
                ix.release()
        self.__init__(self.ctx)

    def size(self) -> int:
        return len(self._live)

    # -- internals
    def _match_slots(self, filters: List[bytes], now_ms: int) -> List[List[int]]:
        rows: List[List[int]] = [[] for _ in filters]
        packed = pack(filters)
        for ix in (self._main, self._delta):
            if ix is None:
                continue
            ro, ids = ix.match(packed, now_ms)
            for i in range(len(filters)):
                rows[i].extend(int(x) for x in ids[int(ro[i]):int(ro[i + 1])])
        return rows

    def _expiries(self, lo: int, hi: int) -> np.ndarray:
        return np.array([self._live[s][1] if s in self._live else 1 for s in range(lo, hi)], np.uint64)

    def _sync(self):
        """Rebuild the delta index if topics were stored since its last build."""
        if not self._delta_dirty:
            return
        if self._delta is not None:
            self._delta.release()
        lo, hi = self._n_main, len(self._topics)
        self._delta = build_retained(self.ctx, self._topics[lo:hi], np.arange(lo, hi, dtype=np.uint32),
                                     self._expiries(lo, hi))
        self._delta_dirty = False

    def _compact(self):
        """The live set rebuilt into a new main index; the delta starts empty."""
        live = sorted(self._live)
        topics = [self._topics[s] for s in live]
        entries = [self._live[s] for s in live]
        for ix in (self._main, self._delta):
            if ix is not None:
                ix.release()
        self._topics = topics
        self._slot = {t: i for i, t in enumerate(topics)}
        self._live = dict(enumerate(entries))
        self._n_main = len(topics)
        self._main = build_retained(self.ctx, topics, np.arange(len(topics), dtype=np.uint32),
                                    np.array([e[1] for e in entries], np.uint64))
        self._delta = None
        self._delta_dirty = False
        self.compactions += 1
