"""Shared-subscription dispatch: one group member per matched shared filter.

``SharedTable`` wraps the library's shared-subscription table
(emqx_gm_shared_*, include/emqx_gpu_match.h): the ``{Group, Filter}`` slots with
their member lists in HBM, bound to one index snapshot, and the picks of a whole
publish window computed by the gfx950 kernels of gm_shared.hip.  ``SharedSub`` is
the host mirror of ``emqx_shared_sub`` (apps/emqx/src/emqx_shared_sub.erl:
subscribe/3, unsubscribe/3, subscribers/2, dispatch/3) on top of it.  The
reference picks per message and group in the publisher's process (pick/6 ..
do_pick_subscriber/6, :234-288); here every pick goes through the device, in
batch order, bit-equal to that loop.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Csr, GpuMatchError, SharedInfo, check, lib
from .engine import BytesLike, DeviceCsr, _b, _csr_to_numpy, _ptr, pack

STRATEGIES = {"hash": _lib.SHARE_HASH, "hash_clientid": _lib.SHARE_HASH, "hash_topic": _lib.SHARE_HASH,
              "round_robin": _lib.SHARE_ROUND_ROBIN, "sticky": _lib.SHARE_STICKY, "random": _lib.SHARE_RANDOM}


def _strategy(s) -> int:
    return STRATEGIES[s] if isinstance(s, str) else int(s)


def _host_csr(row_off, ids):
    ro = np.ascontiguousarray(row_off, np.uint64)
    ii = np.ascontiguousarray(ids, np.uint32)
    keep = ii if len(ii) else np.zeros(1, np.uint32)
    m = Csr()
    m.n_rows = len(ro) - 1
    m.nnz = len(ii)
    m.row_off = ro.ctypes.data_as(C.POINTER(C.c_uint64))
    m.ids = keep.ctypes.data_as(C.POINTER(C.c_uint32))
    m.on_device = 0
    return m, (ro, keep)


def _slot_args(slots):
    """[(filter, group id, [member ids])] -> the packed build arguments."""
    slots = list(slots)
    fb, fo = pack([f for f, _, _ in slots])
    gids = np.array([g for _, g, _ in slots] or [0], np.uint32)
    mo = np.zeros(len(slots) + 1, np.uint64)
    if slots:
        np.cumsum([len(m) for _, _, m in slots], out=mo[1:])
    mi = np.fromiter((x for _, _, m in slots for x in m), np.uint32, count=int(mo[-1]))
    if len(mi) == 0:
        mi = np.zeros(1, np.uint32)
    return fb, fo, gids, len(slots), mo, mi


class SharedTable:
    """One shared-subscription table.  Made by ``Context.build_shared`` (resident
    in HBM, bound to an index snapshot) or ``SharedTable.compile_host`` (host
    tables only: ``pick_host`` works, ``pick`` raises)."""

    def __init__(self, ctx, handle, index=None):
        self.ctx, self.h, self.index = ctx, handle, index

    @classmethod
    def compile_host(cls, index_filters, slots, prev: Optional["SharedTable"] = None) -> "SharedTable":
        ifb, ifo = index_filters if isinstance(index_filters, tuple) else pack(index_filters)
        fb, fo, gids, n, mo, mi = _slot_args(slots)
        h = C.c_void_p()
        rc = lib().emqx_gm_shared_compile_host(_ptr(ifb), _ptr(ifo), len(ifo) - 1, _ptr(fb), _ptr(fo), _ptr(gids), n,
                                               _ptr(mo), _ptr(mi), prev.h if prev else None, C.byref(h))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "shared_compile_host")
        return cls(None, h)

    # -- emqx_shared_sub:pick/6 for every hit of the rows
    def pick(self, rows, strategy, hashes=None, seed: int = 0, n_chunks: Optional[int] = None):
        """``rows``: (row_off, filter ids) of a match on the bound snapshot.
        Returns (row_off, picked member ids, slot indices), one entry per hit in
        batch order.  ``hashes``: one u32 per row, for the hash strategies.
        ``n_chunks``: force the round-robin chunk count (test support)."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "shared pick: a host-only table")
        m, keep = _host_csr(*rows)
        hs = None if hashes is None else np.ascontiguousarray(hashes, np.uint32)
        if hs is not None and len(hs) != m.n_rows:
            raise ValueError("one hash per row")
        if hs is not None and len(hs) == 0:
            hs = np.zeros(1, np.uint32)
        om, os_ = Csr(), Csr()
        if n_chunks is None:
            rc = lib().emqx_gm_shared_pick(self.ctx.h, self.h, C.byref(m), _strategy(strategy), _ptr(hs),
                                           seed & 0xFFFFFFFF, C.byref(om), C.byref(os_))
        else:
            rc = lib().emqx_gm_shared_pick_chunked(self.ctx.h, self.h, C.byref(m), _strategy(strategy), _ptr(hs),
                                                   seed & 0xFFFFFFFF, n_chunks, C.byref(om), C.byref(os_))
        check(rc, self.ctx.h, "shared_pick")
        try:
            ro, mem = _csr_to_numpy(om)
            ro2, slots = _csr_to_numpy(os_)
            assert np.array_equal(ro, ro2)
            return ro, mem, slots
        finally:
            lib().emqx_gm_csr_free(self.ctx.h, C.byref(om))
            lib().emqx_gm_csr_free(self.ctx.h, C.byref(os_))

    def pick_device(self, matches: DeviceCsr, strategy, d_hashes: Optional[int] = None,
                    seed: int = 0) -> Tuple[DeviceCsr, DeviceCsr]:
        """Rows already in HBM (a DeviceCsr of a match on the bound snapshot;
        ``d_hashes`` a device pointer): (members, slots) stay in HBM."""
        om, os_ = Csr(), Csr()
        check(lib().emqx_gm_shared_pick(self.ctx.h, self.h, C.byref(matches.csr), _strategy(strategy),
                                        C.c_void_p(d_hashes) if d_hashes else None, seed & 0xFFFFFFFF, C.byref(om),
                                        C.byref(os_)), self.ctx.h, "shared_pick")
        return DeviceCsr(self.ctx, om), DeviceCsr(self.ctx, os_)

    def pick_host(self, rows, strategy, hashes=None, seed: int = 0):
        """The same picks by the single-threaded host walk over a host-only
        table and its own state: test and measurement support."""
        m, keep = _host_csr(*rows)
        hs = None if hashes is None else np.ascontiguousarray(hashes, np.uint32)
        if hs is not None and len(hs) == 0:
            hs = np.zeros(1, np.uint32)
        om, os_ = Csr(), Csr()
        rc = lib().emqx_gm_shared_pick_host(self.h, C.byref(m), _strategy(strategy), _ptr(hs), seed & 0xFFFFFFFF,
                                            C.byref(om), C.byref(os_))
        if rc != _lib.OK:
            e = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, e.decode(errors="replace") if e else "shared_pick_host")
        try:
            ro, mem = _csr_to_numpy(om)
            _, slots = _csr_to_numpy(os_)
            return ro, mem, slots
        finally:
            lib().emqx_gm_shared_csr_free_host(C.byref(om))
            lib().emqx_gm_shared_csr_free_host(C.byref(os_))

    def last_times(self) -> Tuple[float, float, float, float]:
        """Device ms of the last pick: enumerate, expand, round-robin passes, whole call."""
        ms = (C.c_double * 4)()
        check(lib().emqx_gm_shared_last_times(self.h, ms), None, "shared_last_times")
        return tuple(ms)

    def slot(self, s: int) -> Tuple[int, int, List[int]]:
        """(filter id, group id, member ids) of slot ``s`` (emqx_gm_shared_slot)."""
        f, g, p, n = C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_uint64()
        check(lib().emqx_gm_shared_slot(self.h, s, C.byref(f), C.byref(g), C.byref(p), C.byref(n)), None,
              "shared_slot")
        mem = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)).tolist() if n.value else []
        return int(f.value), int(g.value), mem

    def slots(self) -> List[Tuple[int, int, List[int]]]:
        return [self.slot(s) for s in range(int(self.info().n_slots))]

    def info(self) -> SharedInfo:
        info = SharedInfo()
        check(lib().emqx_gm_shared_info(self.h, C.byref(info)), None, "shared_info")
        return info

    def release(self):
        if self.h:
            lib().emqx_gm_shared_release(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.release()
        except Exception:
            pass


def build_shared(ctx, index, slots, prev: Optional[SharedTable] = None) -> SharedTable:
    """``Context.build_shared``: ``slots`` is [(filter, group id, [member ids])]
    in any order (equal pairs are merged, duplicate members kept once)."""
    fb, fo, gids, n, mo, mi = _slot_args(slots)
    h = C.c_void_p()
    check(lib().emqx_gm_shared_build(ctx.h, index.h, _ptr(fb), _ptr(fo), _ptr(gids), n, _ptr(mo), _ptr(mi),
                                     prev.h if prev else None, 0, C.byref(h)), ctx.h, "shared_build")
    return SharedTable(ctx, h, index)


class SharedSub:
    """Host mirror of emqx_shared_sub over the device table.  Groups and
    subscribers get u32 ids in order of first appearance; the table is rebuilt,
    with the previous one as ``prev`` so round-robin and sticky state carry
    over, when members or the snapshot changed since the last dispatch.  Every
    filter that has a group member must be a filter of the snapshot (the shared
    route: emqx_router:do_add_route/2 with dest {Group, Node})."""

    def __init__(self, ctx, seed: int = 0):
        self.ctx, self.seed = ctx, seed & 0xFFFFFFFF
        self.group_id: Dict[bytes, int] = {}
        self.groups: List[bytes] = []
        self.sub_id: Dict[object, int] = {}
        self.subs: List[object] = []
        self._members: Dict[Tuple[bytes, bytes], List[int]] = {}  # (group, filter) -> member ids, insertion order
        self._table: Optional[SharedTable] = None
        self._index_h = None
        self._dirty = True
        self._slots: List[Tuple[bytes, bytes, List[int]]] = []    # slot -> (group, filter, member ids)
        self.builds = 0
        self.calls = 0

    # -- emqx_shared_sub:subscribe/3 (:98-99), unsubscribe/3 (:106-108)
    def subscribe(self, group: BytesLike, filt: BytesLike, sub) -> None:
        g, f = _b(group), _b(filt)
        if g not in self.group_id:
            self.group_id[g] = len(self.groups)
            self.groups.append(g)
        sid = self.sub_id.get(sub)
        if sid is None:
            sid = self.sub_id[sub] = len(self.subs)
            self.subs.append(sub)
        mem = self._members.setdefault((g, f), [])
        if sid not in mem:  # an ets bag: an identical object is stored once
            mem.append(sid)
            self._dirty = True

    def unsubscribe(self, group: BytesLike, filt: BytesLike, sub) -> None:
        key = (_b(group), _b(filt))
        sid = self.sub_id.get(sub)
        mem = self._members.get(key)
        if mem is None or sid not in mem:
            return
        mem.remove(sid)
        if not mem:
            del self._members[key]
        self._dirty = True

    # -- subscribers/2 (:287-288)
    def subscribers(self, group: BytesLike, filt: BytesLike) -> list:
        return [self.subs[i] for i in self._members.get((_b(group), _b(filt)), [])]

    def shared_filters(self) -> List[bytes]:
        return sorted({f for _, f in self._members})

    def table(self, index) -> SharedTable:
        """The table for ``index``, rebuilt (with ``prev``) if anything changed."""
        if self._table is None or self._dirty or self._index_h is not index.h:
            slots = [(f, self.group_id[g], mem) for (g, f), mem in self._members.items()]
            new = build_shared(self.ctx, index, slots, self._table)
            if self._table is not None:
                self._table.release()
            self._table, self._index_h, self._dirty = new, index.h, False
            self._slots = [(self.groups[g], index.filter(f), mem) for f, g, mem in new.slots()]
            self.builds += 1
        return self._table

    # -- dispatch/3 (:113-116) for every shared hit of a matched batch
    def dispatch_batch(self, index, rows, strategy, hashes=None, seed: Optional[int] = None):
        """``rows``: (row_off, filter ids) of a match on ``index``.  Per row, in
        batch order, [(group, filter, picked subscriber)].  ``hashes``: one u32
        per row (erlang:phash2 of the client id or source topic) for the hash
        strategies.  ``seed`` defaults to a per-call value derived from the
        constructor's."""
        t = self.table(index)
        auto = self.next_seed()
        ro, mem, slots = t.pick(rows, strategy, hashes, auto if seed is None else seed)
        return self.picks_rows(ro, mem, slots)

    def next_seed(self) -> int:
        """The per-call seed: counts the call and derives its seed from the constructor's."""
        self.calls += 1
        return (self.seed + self.calls * 0x9E3779B9) & 0xFFFFFFFF

    def picks_rows(self, ro, mem, slots):
        """A pick of the current table, per row: [(group, filter, picked subscriber)]."""
        out = []
        for r in range(len(ro) - 1):
            row = []
            for k in range(int(ro[r]), int(ro[r + 1])):
                g, f, _ = self._slots[int(slots[k])]
                row.append((g, f, self.subs[int(mem[k])]))
            out.append(row)
        return out

    def release(self):
        if self._table is not None:
            self._table.release()
            self._table = None
