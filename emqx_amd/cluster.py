"""Cluster forwards: a publish window's remote routes as one list per node.

``DestTable`` wraps the library's route-destination table (emqx_gm_dests_*,
emqx_gm_forward_plan, include/emqx_gpu_match.h): the node destinations of the
``emqx_route`` bag in HBM, bound to one index snapshot, and the forward plan of a
whole publish window computed by the gfx950 kernels of gm_dests.hip.
``ClusterRoutes`` is the host mirror of the node part of ``emqx_route``
(apps/emqx/src/emqx_router.erl: do_add_route/2, do_delete_route/2,
lookup_routes/1; emqx_router_helper's nodedown purge) on top of it.  The
reference reads the bag per matched filter and forwards per (message, route)
(emqx_broker.erl:245-293); here one call per window gives, per node, the
``(row, filter)`` pairs to forward, in publish order.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, NamedTuple, Optional, Set, Tuple

import numpy as np

from . import _lib
from ._lib import Csr, DestsInfo, Forwards, GpuMatchError, check, lib
from .engine import BytesLike, DeviceCsr, _b, _ptr, pack
from .shared import _host_csr

NO_SKIP = _lib.DESTS_NO_SKIP


class ForwardPlan(NamedTuple):
    """Node k's forwards are entries [node_off[k], node_off[k + 1]) of rows /
    filters, in batch order; row_routes[r] counts the row's node routes,
    the skipped node's included."""
    node_off: np.ndarray
    rows: np.ndarray
    filters: np.ndarray
    row_routes: np.ndarray

    def node(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        a, b = int(self.node_off[k]), int(self.node_off[k + 1])
        return self.rows[a:b], self.filters[a:b]


def _skip(skip_node: Optional[int]) -> int:
    return NO_SKIP if skip_node is None else int(skip_node) & 0xFFFFFFFF


def _plan_to_numpy(fw: Forwards) -> ForwardPlan:
    n, p, N = int(fw.n_rows), int(fw.n_pairs), int(fw.n_nodes)
    u32 = np.zeros(0, np.uint32)
    return ForwardPlan(np.ctypeslib.as_array(fw.node_off, shape=(N + 1,)).copy(),
                       np.ctypeslib.as_array(fw.rows, shape=(p,)).copy() if p else u32,
                       np.ctypeslib.as_array(fw.filters, shape=(p,)).copy() if p else u32,
                       np.ctypeslib.as_array(fw.row_routes, shape=(n,)).copy() if n else u32)


class DeviceForwards:
    """A forward plan resident in HBM (owned by the library until free())."""

    def __init__(self, ctx, fw: Forwards):
        self.ctx, self.fw = ctx, fw

    @property
    def n_pairs(self) -> int:
        return int(self.fw.n_pairs)

    def to_host(self) -> ForwardPlan:
        fw = self.fw
        n, p, N = int(fw.n_rows), int(fw.n_pairs), int(fw.n_nodes)

        def down(ptr, count, dtype):
            a = np.zeros(max(count, 1), dtype)
            if count:
                self.ctx.memcpy_d2h(a, C.cast(ptr, C.c_void_p).value, count * a.itemsize)
            return a[:count]
        return ForwardPlan(down(fw.node_off, N + 1, np.uint64), down(fw.rows, p, np.uint32),
                           down(fw.filters, p, np.uint32), down(fw.row_routes, n, np.uint32))

    def free(self):
        if self.fw.node_off:
            check(lib().emqx_gm_forwards_free(self.ctx.h, C.byref(self.fw)), self.ctx.h, "forwards_free")

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


def _route_args(routes):
    """[(filter, node id)] -> the packed build arguments."""
    routes = list(routes)
    fb, fo = pack([f for f, _ in routes])
    nodes = np.array([n for _, n in routes] or [0], np.uint32)
    return fb, fo, nodes, len(routes)


class DestTable:
    """One route-destination table.  Made by ``build_dests`` (resident in HBM,
    bound to an index snapshot) or ``DestTable.compile_host`` (host tables only:
    ``plan_host`` works, ``plan`` raises)."""

    def __init__(self, ctx, handle, index=None):
        self.ctx, self.h, self.index = ctx, handle, index

    @classmethod
    def compile_host(cls, index_filters, routes, n_nodes: int, skip_unknown: bool = False) -> "DestTable":
        ifb, ifo = index_filters if isinstance(index_filters, tuple) else pack(index_filters)
        fb, fo, nodes, n = _route_args(routes)
        h = C.c_void_p()
        rc = lib().emqx_gm_dests_compile_host(_ptr(ifb), _ptr(ifo), len(ifo) - 1, _ptr(fb), _ptr(fo), _ptr(nodes), n,
                                              n_nodes, _lib.DESTS_SKIP_UNKNOWN if skip_unknown else 0, C.byref(h))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "dests_compile_host")
        return cls(None, h)

    def plan(self, rows, skip_node: Optional[int] = None, n_chunks: Optional[int] = None) -> ForwardPlan:
        """``rows``: (row_off, filter ids) of a match on the bound snapshot.
        ``skip_node``: the caller's own node id (None skips nothing).
        ``n_chunks``: force the partition's chunk count (test support)."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "forward plan: a host-only table")
        m, keep = _host_csr(*rows)
        fw = Forwards()
        if n_chunks is None:
            rc = lib().emqx_gm_forward_plan(self.ctx.h, self.h, C.byref(m), _skip(skip_node), C.byref(fw))
        else:
            rc = lib().emqx_gm_forward_plan_chunked(self.ctx.h, self.h, C.byref(m), _skip(skip_node), n_chunks,
                                                    C.byref(fw))
        check(rc, self.ctx.h, "forward_plan")
        try:
            return _plan_to_numpy(fw)
        finally:
            lib().emqx_gm_forwards_free(self.ctx.h, C.byref(fw))

    def plan_device(self, matches: DeviceCsr, skip_node: Optional[int] = None,
                    n_chunks: Optional[int] = None) -> DeviceForwards:
        """Rows already in HBM (a DeviceCsr of a match on the bound snapshot):
        the plan stays in HBM."""
        fw = Forwards()
        check(lib().emqx_gm_forward_plan_chunked(self.ctx.h, self.h, C.byref(matches.csr), _skip(skip_node),
                                                 n_chunks or 0, C.byref(fw)), self.ctx.h, "forward_plan")
        return DeviceForwards(self.ctx, fw)

    def plan_host(self, rows, skip_node: Optional[int] = None) -> ForwardPlan:
        """The same plan by the single-threaded host walk over the table's host
        copy: test and measurement support."""
        m, keep = _host_csr(*rows)
        fw = Forwards()
        rc = lib().emqx_gm_forward_plan_host(self.h, C.byref(m), _skip(skip_node), C.byref(fw))
        if rc != _lib.OK:
            e = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, e.decode(errors="replace") if e else "forward_plan_host")
        try:
            return _plan_to_numpy(fw)
        finally:
            lib().emqx_gm_forwards_free_host(C.byref(fw))

    def last_times(self) -> Tuple[float, float, float, float]:
        """Device ms of the last plan: enumerate, expand, partition, whole call."""
        ms = (C.c_double * 4)()
        check(lib().emqx_gm_dests_last_times(self.h, ms), None, "dests_last_times")
        return tuple(ms)

    def info(self) -> DestsInfo:
        info = DestsInfo()
        check(lib().emqx_gm_dests_info(self.h, C.byref(info)), None, "dests_info")
        return info

    def release(self):
        if self.h:
            lib().emqx_gm_dests_release(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.release()
        except Exception:
            pass


def build_dests(ctx, index, routes, n_nodes: int, skip_unknown: bool = False) -> DestTable:
    """A route-destination table bound to ``index`` (emqx_gm_dests_build):
    ``routes`` is [(filter, node id)] in any order (a pair given twice is stored
    once); ``skip_unknown`` drops, and counts, routes of filters the snapshot
    does not hold instead of refusing them."""
    fb, fo, nodes, n = _route_args(routes)
    h = C.c_void_p()
    check(lib().emqx_gm_dests_build(ctx.h, index.h, _ptr(fb), _ptr(fo), _ptr(nodes), n, n_nodes,
                                    _lib.DESTS_SKIP_UNKNOWN if skip_unknown else 0, C.byref(h)), ctx.h, "dests_build")
    return DestTable(ctx, h, index)


class ClusterRoutes:
    """Host mirror of the node destinations of emqx_route over the device
    table.  Nodes get dense u32 ids in order of first appearance (a node that
    went down keeps its id: ids index the plan's lists).  The table is rebuilt
    when a route changed or the snapshot is another one since the last plan --
    patching it in place is the follow-up."""

    def __init__(self, ctx, node: BytesLike = b"node"):
        self.ctx, self.node = ctx, _b(node)
        self.node_id: Dict[bytes, int] = {}
        self.nodes: List[bytes] = []
        self._routes: Dict[bytes, Set[int]] = {}  # filter -> node ids
        self._table: Optional[DestTable] = None
        self._index_h = None
        self._dirty = True
        self.builds = 0
        self.self_id = self.id_of(self.node)

    def id_of(self, node: BytesLike) -> int:
        n = _b(node)
        i = self.node_id.get(n)
        if i is None:
            if len(self.nodes) >= _lib.DESTS_MAX_NODES:
                raise GpuMatchError(_lib.EINVAL, "more than %d nodes" % _lib.DESTS_MAX_NODES)
            i = self.node_id[n] = len(self.nodes)
            self.nodes.append(n)
        return i

    # -- emqx_router:do_add_route/2 (:112-116), do_delete_route/2 (:164-172)
    def add_route(self, filt: BytesLike, node: BytesLike) -> None:
        s = self._routes.setdefault(_b(filt), set())
        i = self.id_of(node)
        if i not in s:  # lists:member: a pair is stored once
            s.add(i)
            self._dirty = True

    def delete_route(self, filt: BytesLike, node: BytesLike) -> None:
        f = _b(filt)
        s = self._routes.get(f)
        i = self.node_id.get(_b(node))
        if s is None or i not in s:
            return
        s.discard(i)
        if not s:
            del self._routes[f]
        self._dirty = True

    # -- emqx_router_helper:cleanup_routes/1 (:177-181): every route to a node that went down
    def cleanup_routes(self, node: BytesLike) -> int:
        i = self.node_id.get(_b(node))
        gone = 0
        if i is None:
            return 0
        for f in [f for f, s in self._routes.items() if i in s]:
            self._routes[f].discard(i)
            if not self._routes[f]:
                del self._routes[f]
            gone += 1
        if gone:
            self._dirty = True
        return gone

    # -- lookup_routes/1 (:136), node destinations only
    def lookup_routes(self, filt: BytesLike) -> List[bytes]:
        return [self.nodes[i] for i in sorted(self._routes.get(_b(filt), ()))]

    def routes(self) -> Iterable[Tuple[bytes, int]]:
        return [(f, i) for f, s in self._routes.items() for i in sorted(s)]

    def table(self, index) -> DestTable:
        """The table for ``index``, rebuilt if anything changed.  A route whose
        filter the snapshot does not hold yet (its route mark is still queued)
        is left out of this build: nothing can match it."""
        if self._table is None or self._dirty or self._index_h is not index.h:
            new = build_dests(self.ctx, index, self.routes(), max(len(self.nodes), 1), skip_unknown=True)
            if self._table is not None:
                self._table.release()
            self._table, self._index_h, self._dirty = new, index.h, False
            self.builds += 1
        return self._table

    def plan(self, index, rows) -> ForwardPlan:
        """The window's forwards to every node but this one."""
        return self.table(index).plan(rows, self.self_id)

    def release(self):
        if self._table is not None:
            self._table.release()
            self._table = None
