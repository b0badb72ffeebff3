"""Session batches: a publish window's deliveries grouped by subscriber.

``SubOptTable.deliver_batches`` (emqx_gm_deliver_batches, include/emqx_gpu_match.h)
gives a window as the lists the reference's connection processes drain from
their mailboxes (``emqx_misc:drain_deliver/1``, apps/emqx/src/emqx_misc.erl:159-173)
and hand to ``emqx_channel:handle_deliver/2`` (emqx_channel.erl:830-842): per
subscriber, ascending by id, its deliveries in window order, each with the
window row, the filter id (the deliver's Topic) and the delivery byte.  Mode
``"lead"`` applies ``emqx_session:ignore_local/4`` (emqx_session.erl:279-291) as
the reference does -- only the leading run of No-Local hits of a batch is
removed.  The grouping is a stable radix partition on the device
(emqx_amd/csrc/gm_batches.hip).
"""

from __future__ import annotations

import ctypes as C
from typing import Iterator, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import Batches, GpuMatchError, check, lib
from .engine import _ptr
from .shared import _host_csr

MODES = {"flag": _lib.SO_FLAG, "drop": _lib.SO_DROP, "lead": _lib.SO_LEAD}


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError("mode: 'flag', 'drop' or 'lead'")
        return MODES[mode]
    return int(mode)


class SessionBatches(NamedTuple):
    """Batch j is subscriber ``subs[j]`` with entries [batch_off[j], batch_off[j + 1])
    of ``rows`` / ``filters`` / ``dopt``; ``batch_dropped`` (None in FLAG mode)
    counts what the mode removed from the batch."""
    subs: np.ndarray
    batch_off: np.ndarray
    rows: np.ndarray
    filters: np.ndarray
    dopt: np.ndarray
    batch_dropped: Optional[np.ndarray]
    n_dropped: int

    def batches(self) -> Iterator[Tuple[int, np.ndarray, np.ndarray, np.ndarray]]:
        """(subscriber, rows, filter ids, bytes) per batch."""
        for j, s in enumerate(self.subs.tolist()):
            a, b = int(self.batch_off[j]), int(self.batch_off[j + 1])
            yield s, self.rows[a:b], self.filters[a:b], self.dopt[a:b]

    def as_lists(self):
        """[(subscriber, [(row, filter id, byte)], removed)] -- test and debugging support."""
        gone = self.batch_dropped.tolist() if self.batch_dropped is not None else [0] * len(self.subs)
        return [(s, list(zip(r.tolist(), f.tolist(), o.tolist())), g) for (s, r, f, o), g in zip(self.batches(), gone)]


def _to_numpy(b: Batches, flag: bool) -> SessionBatches:
    nb, nd = int(b.n_batches), int(b.n_deliveries)

    def arr(ptr, count, dtype):
        return np.ctypeslib.as_array(ptr, shape=(count,)).copy() if count else np.zeros(0, dtype)
    return SessionBatches(arr(b.subs, nb, np.uint32), arr(b.batch_off, nb + 1, np.uint64), arr(b.rows, nd, np.uint32),
                          arr(b.filters, nd, np.uint32), arr(b.dopt, nd, np.uint8),
                          None if flag else arr(b.batch_dropped, nb, np.uint32), int(b.n_dropped))


class DeviceBatches:
    """Session batches resident in HBM (owned by the library until free())."""

    def __init__(self, ctx, b: Batches, flag: bool):
        self.ctx, self.b, self.flag = ctx, b, flag

    @property
    def n_batches(self) -> int:
        return int(self.b.n_batches)

    @property
    def n_deliveries(self) -> int:
        return int(self.b.n_deliveries)

    def to_host(self) -> SessionBatches:
        b = self.b
        nb, nd = int(b.n_batches), int(b.n_deliveries)

        def down(ptr, count, dtype):
            a = np.zeros(max(count, 1), dtype)
            if count:
                self.ctx.memcpy_d2h(a, C.cast(ptr, C.c_void_p).value, count * a.itemsize)
            return a[:count]
        return SessionBatches(down(b.subs, nb, np.uint32), down(b.batch_off, nb + 1, np.uint64),
                              down(b.rows, nd, np.uint32), down(b.filters, nd, np.uint32), down(b.dopt, nd, np.uint8),
                              None if self.flag else down(b.batch_dropped, nb, np.uint32), int(b.n_dropped))

    def free(self):
        if self.b.batch_off:
            check(lib().emqx_gm_batches_free(self.ctx.h, C.byref(self.b)), self.ctx.h, "batches_free")

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


def deliver_batches(self, rows, msg_flags, msg_from=None, mode="flag", index=None, n_chunks: int = 0) -> SessionBatches:
    """``rows``, ``msg_flags``, ``msg_from`` and ``index`` as ``deliver`` takes
    them; ``mode``: "flag" (remove nothing, bit 4 marks a No-Local hit), "drop"
    (remove every hit) or "lead" (remove each batch's leading run of hits, the
    reference's dropwhile; bit 4 cleared).  ``n_chunks`` forces the radix
    partition's chunk count (test support)."""
    from .subopts import _msg_args
    if self.ctx is None:
        raise GpuMatchError(_lib.EUNSUPPORTED, "deliver_batches: a host-only table")
    self._check_bound(index)
    md = _mode(mode)
    m, keep = _host_csr(*rows)
    mf, fr = _msg_args(int(m.n_rows), msg_flags, msg_from)
    b = Batches()
    if n_chunks:
        rc = lib().emqx_gm_deliver_batches_chunked(self.ctx.h, self.h, C.byref(m), _ptr(mf), _ptr(fr), md, n_chunks,
                                                   C.byref(b))
    else:
        rc = lib().emqx_gm_deliver_batches(self.ctx.h, self.h, C.byref(m), _ptr(mf), _ptr(fr), md, C.byref(b))
    check(rc, self.ctx.h, "deliver_batches")
    try:
        return _to_numpy(b, md == _lib.SO_FLAG)
    finally:
        lib().emqx_gm_batches_free(self.ctx.h, C.byref(b))


def deliver_batches_device(self, matches, d_msg_flags: int, d_msg_from: int, mode="flag", index=None,
                           n_chunks: int = 0) -> DeviceBatches:
    """Rows already in HBM (a DeviceCsr, or anything with a ``csr`` field) with
    the messages' bytes and publishers at device addresses: the batches stay in HBM."""
    if self.ctx is None:
        raise GpuMatchError(_lib.EUNSUPPORTED, "deliver_batches: a host-only table")
    self._check_bound(index)
    md = _mode(mode)
    b = Batches()
    check(lib().emqx_gm_deliver_batches_chunked(self.ctx.h, self.h, C.byref(matches.csr), C.c_void_p(d_msg_flags),
                                                C.c_void_p(d_msg_from), md, n_chunks, C.byref(b)),
          self.ctx.h, "deliver_batches")
    return DeviceBatches(self.ctx, b, md == _lib.SO_FLAG)


def deliver_batches_host(self, rows, msg_flags, msg_from=None, mode="flag", index=None) -> SessionBatches:
    """The same batches by the single-threaded host walk over the table's host
    copy (no device): test and measurement support."""
    from .subopts import _msg_args
    self._check_bound(index)
    md = _mode(mode)
    m, keep = _host_csr(*rows)
    mf, fr = _msg_args(int(m.n_rows), msg_flags, msg_from)
    b = Batches()
    rc = lib().emqx_gm_deliver_batches_host(self.h, C.byref(m), _ptr(mf), _ptr(fr), md, C.byref(b))
    if rc != _lib.OK:
        e = lib().emqx_gm_last_error(None)
        raise GpuMatchError(rc, e.decode(errors="replace") if e else "deliver_batches_host")
    try:
        return _to_numpy(b, md == _lib.SO_FLAG)
    finally:
        lib().emqx_gm_batches_free(None, C.byref(b))


def batches_last_times(self):
    """Device ms of the last deliver_batches: count, expand, partition, heads +
    removal + emit, the whole call; its radix passes; and the host-blocking
    waits the last call made."""
    ms = (C.c_double * 7)()
    check(lib().emqx_gm_batches_last_times(self.h, ms), None, "batches_last_times")
    return tuple(ms[:5]) + (int(ms[5]), int(ms[6]))
