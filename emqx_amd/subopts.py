"""Subscription options at dispatch: one option byte beside every delivery.

``SubOptTable`` wraps the library's subscription-option table
(emqx_gm_subopts_*, emqx_gm_deliver, include/emqx_gpu_match.h): the options of
``emqx_broker:subscribe/3`` (apps/emqx/src/emqx_broker.erl:126-145) for the
(filter, subscriber) pairs of one index snapshot, in HBM, and the deliveries of
a whole publish window -- subscriber ids as the fan-out gives them, each with
the byte ``emqx_session:enrich_deliver/2`` would compute and the No-Local
verdict of ``ignore_local/4`` (emqx_session.erl:279-291, 560-602) -- computed by
the gfx950 kernels of gm_subopts.hip.
"""

from __future__ import annotations

import ctypes as C
from typing import Iterable, NamedTuple, Optional, Tuple, Union

import numpy as np

from . import _lib
from ._lib import Deliveries, GpuMatchError, SubOptsInfo, check, lib
from .engine import DeviceCsr, _ptr, pack
from .shared import _host_csr

NO_PUBLISHER = _lib.SO_NO_PUBLISHER
OPT_NL, OPT_RAP, OPT_UPGRADE_QOS = 0x04, 0x08, 0x10
MSG_RETAIN, MSG_RETAINED_HEADER = 0x04, 0x08
DOPT_RETAIN, DOPT_NL, DOPT_NO_LOCAL_HIT = 0x04, 0x08, 0x10


def pack_opt(qos: int = 0, nl: int = 0, rap: int = 0, upgrade_qos: bool = False) -> int:
    """The table's option byte: bits 0-1 QoS, 2 nl, 3 rap, 4 the session's upgrade_qos."""
    if qos not in (0, 1, 2):
        raise ValueError("qos")
    return qos | (OPT_NL if nl else 0) | (OPT_RAP if rap else 0) | (OPT_UPGRADE_QOS if upgrade_qos else 0)


def pack_msg(qos: int = 0, retain: bool = False, retained_header: bool = False) -> int:
    """A message's flag byte: bits 0-1 publish QoS, 2 retain, 3 headers.retained =:= true."""
    if qos not in (0, 1, 2):
        raise ValueError("qos")
    return qos | (MSG_RETAIN if retain else 0) | (MSG_RETAINED_HEADER if retained_header else 0)


class DeliveryOpt(NamedTuple):
    qos: int
    retain: bool
    nl: bool
    no_local_hit: bool


def unpack_dopt(b: int) -> DeliveryOpt:
    """A delivery byte: bits 0-1 effective QoS, 2 retain, 3 the nl flag, 4 the No-Local hit (FLAG mode)."""
    b = int(b)
    return DeliveryOpt(b & 3, bool(b & DOPT_RETAIN), bool(b & DOPT_NL), bool(b & DOPT_NO_LOCAL_HIT))


class Delivered(NamedTuple):
    """Row r's deliveries are entries [row_off[r], row_off[r + 1]) of ids / dopt;
    row_dropped (DROP mode, else None) counts the row's No-Local removals."""
    row_off: np.ndarray
    ids: np.ndarray
    dopt: np.ndarray
    row_dropped: Optional[np.ndarray]
    n_dropped: int


def _opt_byte(o) -> int:
    return pack_opt(**o) if isinstance(o, dict) else int(o)


def _entry_args(entries):
    """[(filter, subscriber id, opt byte | pack_opt kwargs)] -> the packed build arguments."""
    entries = list(entries)
    fb, fo = pack([f for f, _, _ in entries])
    subs = np.array([s for _, s, _ in entries] or [0], np.uint32)
    opts = np.array([_opt_byte(o) for _, _, o in entries] or [0], np.uint8)
    return fb, fo, subs, opts, len(entries)


def _msg_args(n: int, msg_flags, msg_from):
    mf = np.zeros(max(n, 1), np.uint8)
    if n:
        mf[:n] = np.asarray(msg_flags, np.uint8)
    fr = np.full(max(n, 1), NO_PUBLISHER, np.uint32)
    if n and msg_from is not None:
        fr[:n] = np.asarray([NO_PUBLISHER if x is None else x for x in msg_from]
                            if not isinstance(msg_from, np.ndarray) else msg_from, np.uint32)
    return mf, fr


def _to_numpy(d: Deliveries, drop: bool) -> Delivered:
    n, nnz = int(d.deliveries.n_rows), int(d.deliveries.nnz)
    ro = np.ctypeslib.as_array(d.deliveries.row_off, shape=(n + 1,)).copy()
    ids = np.ctypeslib.as_array(d.deliveries.ids, shape=(nnz,)).copy() if nnz else np.zeros(0, np.uint32)
    dopt = np.ctypeslib.as_array(d.dopt, shape=(nnz,)).copy() if nnz else np.zeros(0, np.uint8)
    rd = None
    if drop:
        rd = np.ctypeslib.as_array(d.row_dropped, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
    return Delivered(ro, ids, dopt, rd, int(d.n_dropped))


class DeviceDeliveries:
    """Deliveries resident in HBM (owned by the library until free())."""

    def __init__(self, ctx, d: Deliveries, drop: bool):
        self.ctx, self.d, self.drop = ctx, d, drop

    @property
    def nnz(self) -> int:
        return int(self.d.deliveries.nnz)

    def to_host(self) -> Delivered:
        d = self.d
        n, nnz = int(d.deliveries.n_rows), int(d.deliveries.nnz)

        def down(ptr, count, dtype):
            a = np.zeros(max(count, 1), dtype)
            if count:
                self.ctx.memcpy_d2h(a, C.cast(ptr, C.c_void_p).value, count * a.itemsize)
            return a[:count]
        return Delivered(down(d.deliveries.row_off, n + 1, np.uint64), down(d.deliveries.ids, nnz, np.uint32),
                         down(d.dopt, nnz, np.uint8), down(d.row_dropped, n, np.uint32) if self.drop else None,
                         int(d.n_dropped))

    def free(self):
        if self.d.deliveries.row_off:
            check(lib().emqx_gm_deliveries_free(self.ctx.h, C.byref(self.d)), self.ctx.h, "deliveries_free")

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


class SubOptTable:
    """One subscription-option table.  Made by ``build_subopts`` (resident in
    HBM, bound to an index snapshot, which it retains) or
    ``SubOptTable.compile_host`` (host tables only: ``deliver_host`` works,
    ``deliver`` raises)."""

    def __init__(self, ctx, handle, index=None):
        self.ctx, self.h, self.index = ctx, handle, index

    @classmethod
    def compile_host(cls, index_filters, subs, entries, default: int = 0,
                     skip_unknown: bool = False) -> "SubOptTable":
        """``index_filters`` / ``subs`` as ``Context.build_index`` takes them."""
        ifb, ifo = index_filters if isinstance(index_filters, tuple) else pack(index_filters)
        n = len(ifo) - 1
        so = si = None
        if subs is not None:
            if isinstance(subs, tuple):
                so, si = np.ascontiguousarray(subs[0], np.uint64), np.ascontiguousarray(subs[1], np.uint32)
            else:
                so = np.zeros(n + 1, np.uint64)
                np.cumsum([len(s) for s in subs], out=so[1:])
                si = np.fromiter((x for s in subs for x in s), np.uint32, count=int(so[-1]))
            if len(si) == 0:
                si = np.zeros(1, np.uint32)
        fb, fo, es, eo, ne = _entry_args(entries)
        h = C.c_void_p()
        rc = lib().emqx_gm_subopts_compile_host(_ptr(ifb), _ptr(ifo), n, _ptr(so), _ptr(si), _ptr(fb), _ptr(fo),
                                                _ptr(es), _ptr(eo), ne, _opt_byte(default),
                                                _lib.SO_SKIP_UNKNOWN if skip_unknown else 0, C.byref(h))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "subopts_compile_host")
        return cls(None, h)

    def _check_bound(self, index):
        if index is not None and lib().emqx_gm_subopts_index(self.h) != index.h.value:
            raise GpuMatchError(_lib.EINVAL, "deliver: the table is bound to another snapshot than the rows'")

    def deliver(self, rows, msg_flags, msg_from=None, drop: bool = False, index=None) -> Delivered:
        """``rows``: (row_off, filter ids) of a match on the bound snapshot
        (``index``, when given, is checked to be it).  ``msg_flags``: one
        ``pack_msg`` byte per row; ``msg_from``: the publisher's subscriber id
        per row (None: no publisher).  ``drop``: remove the No-Local deliveries
        (EMQX_GM_SO_DROP) instead of flagging them."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "deliver: a host-only table")
        self._check_bound(index)
        m, keep = _host_csr(*rows)
        mf, fr = _msg_args(int(m.n_rows), msg_flags, msg_from)
        d = Deliveries()
        check(lib().emqx_gm_deliver(self.ctx.h, self.h, C.byref(m), _ptr(mf), _ptr(fr),
                                    _lib.SO_DROP if drop else _lib.SO_FLAG, C.byref(d)), self.ctx.h, "deliver")
        try:
            return _to_numpy(d, drop)
        finally:
            lib().emqx_gm_deliveries_free(self.ctx.h, C.byref(d))

    def deliver_device(self, matches: Union[DeviceCsr, "object"], d_msg_flags: int, d_msg_from: int,
                       drop: bool = False, index=None) -> DeviceDeliveries:
        """Rows already in HBM (a DeviceCsr of a match on the bound snapshot, or
        anything with a ``csr`` field) with the messages' bytes and publishers
        at device addresses: the deliveries stay in HBM."""
        self._check_bound(index)
        d = Deliveries()
        check(lib().emqx_gm_deliver(self.ctx.h, self.h, C.byref(matches.csr), C.c_void_p(d_msg_flags),
                                    C.c_void_p(d_msg_from), _lib.SO_DROP if drop else _lib.SO_FLAG, C.byref(d)),
              self.ctx.h, "deliver")
        return DeviceDeliveries(self.ctx, d, drop)

    def deliver_host(self, rows, msg_flags, msg_from=None, drop: bool = False) -> Delivered:
        """The same deliveries by the single-threaded host walk over the table's
        host copy: test and measurement support."""
        m, keep = _host_csr(*rows)
        mf, fr = _msg_args(int(m.n_rows), msg_flags, msg_from)
        d = Deliveries()
        rc = lib().emqx_gm_deliver_host(self.h, C.byref(m), _ptr(mf), _ptr(fr),
                                        _lib.SO_DROP if drop else _lib.SO_FLAG, C.byref(d))
        if rc != _lib.OK:
            e = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, e.decode(errors="replace") if e else "deliver_host")
        try:
            return _to_numpy(d, drop)
        finally:
            lib().emqx_gm_deliveries_free_host(C.byref(d))

    def last_times(self) -> Tuple[float, float, float]:
        """Device ms of the last deliver: lengths + scan + row offsets, the copy kernel, the whole call."""
        ms = (C.c_double * 3)()
        check(lib().emqx_gm_subopts_last_times(self.h, ms), None, "subopts_last_times")
        return tuple(ms)

    def info(self) -> SubOptsInfo:
        info = SubOptsInfo()
        check(lib().emqx_gm_subopts_info(self.h, C.byref(info)), None, "subopts_info")
        return info

    def release(self):
        if self.h:
            lib().emqx_gm_subopts_release(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.release()
        except Exception:
            pass


def build_subopts(ctx, index, entries: Iterable, default: int = 0, skip_unknown: bool = False) -> SubOptTable:
    """A subscription-option table bound to ``index`` (emqx_gm_subopts_build):
    ``entries`` is [(filter, subscriber id, opt)] with opt a ``pack_opt`` byte
    or its keyword dict; a pair of the snapshot without an entry gets
    ``default``; ``skip_unknown`` drops, and counts, entries whose pair the
    snapshot does not hold instead of refusing them."""
    fb, fo, es, eo, ne = _entry_args(entries)
    h = C.c_void_p()
    check(lib().emqx_gm_subopts_build(ctx.h, index.h, _ptr(fb), _ptr(fo), _ptr(es), _ptr(eo), ne, _opt_byte(default),
                                      _lib.SO_SKIP_UNKNOWN if skip_unknown else 0, C.byref(h)), ctx.h, "subopts_build")
    return SubOptTable(ctx, h, index)


# session batches (emqx_gm_deliver_batches): the same deliveries grouped by subscriber, emqx_amd/batches.py
from . import batches as _batches  # noqa: E402
from .batches import DeviceBatches, SessionBatches  # noqa: E402,F401

SubOptTable.deliver_batches = _batches.deliver_batches
SubOptTable.deliver_batches_device = _batches.deliver_batches_device
SubOptTable.deliver_batches_host = _batches.deliver_batches_host
SubOptTable.batches_last_times = _batches.batches_last_times
