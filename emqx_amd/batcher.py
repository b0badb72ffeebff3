"""Publish batching aggregator: the host mirror of nif/emqx_gpu_match_batcher.erl.

The reference publishes one message at a time in the publisher's process:
emqx_broker:publish/1 counts 'messages.publish', runs the 'message.publish'
hook, persists the message and then route(aggre(match_routes(Topic))) --
a local route dispatches to the filter's subscribers, a remote one is
forwarded, a shared-group one goes to emqx_shared_sub, and no route at all
runs 'message.dropped' + inc_dropped_cnt (apps/emqx/src/emqx_broker.erl:
204-215, 245-273, 296-322, 506-530).

Here only the MATCH is batched.  ``PublishBatcher`` is the server side: it
collects topics for at most ``window_s`` seconds or ``max_batch`` topics and
answers each with its row -- ``[(filter, subscriber ids)]`` over every matched
route filter -- from ONE groups call (``GpuRoutes.groups``: emqx_gm_match
WITH_EXACT -> emqx_gm_fanout -> each fan-out row cut back into one segment per
filter, the NIF's fanout_batch/2).  ``PublishBatcher.publish`` is the caller
side: it does everything else the reference's publish/1 does, in the caller's
thread, with the local dispatch over the row's subscriber ids and
lookup_routes/1 only for filters that have other destinations (remote nodes,
shared groups).  When the server answers an error (no index, a failed
engine call, a stale snapshot) the caller takes the reference path
(``fallback``: match_routes/1).

``GpuRoutes`` is the server's index maintenance: subscribe / unsubscribe /
subscriber_down / route_add / route_delete queue ops, and the next batch
applies them with ONE emqx_gm_index_update_subs (a new snapshot derived from
the last, never a rebuild by the aggregator).

The window logic takes an injectable clock and groups function, so it is
tested on the CPU; the GPU path is ``GpuRoutes``.
"""

from __future__ import annotations

import threading
import time
import zlib
from concurrent.futures import Future
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

Group = Tuple[bytes, np.ndarray]  # (filter, subscriber ids)
Row = List[Group]
Result = List[Tuple[object, bytes, Tuple[str, object]]]  # publish_result(): [(node | "share", filter, result)]


def _b(s) -> bytes:
    return s.encode() if isinstance(s, str) else bytes(s)


class _Sent:
    """A remote node route whose forward already left with its window's
    forward_batch: the node and the recorded result."""
    __slots__ = ("node", "res")

    def __init__(self, node, res):
        self.node, self.res = node, res


def is_sys(topic: bytes) -> bool:
    """emqx_message:is_sys/1: a $SYS/ topic (not counted in the publish/drop metrics)."""
    return topic.startswith(b"$SYS/")


class _IdsOpts:
    """A filter's segment of a window's deliveries with the option bytes beside
    the ids (``GpuRoutes.groups_opts``); ``dropped``: its No-Local removals."""
    __slots__ = ("ids", "dopt", "dropped")

    def __init__(self, ids, dopt, dropped=0):
        self.ids, self.dopt, self.dropped = ids, dopt, dropped

    def __len__(self):
        return len(self.ids)

    def tolist(self):
        return self.ids.tolist()


class _Counted:
    """A filter's segment of a window whose local deliveries went out by session
    batch (``PublishBatcher(batches=True)``): the subscribers the snapshot lists
    for it, the deliveries the mode kept, and those a ``deliver_batch`` took."""
    __slots__ = ("listed", "kept", "n")

    def __init__(self, listed, kept, n):
        self.listed, self.kept, self.n = listed, kept, n

    def __len__(self):
        return self.listed


def msg_meta(topic, msg):
    """The default ``PublishBatcher(msg_meta=)``: (qos, retain, from[, headers.retained])
    of a message given as a dict with those keys; anything else is (0, False, None)."""
    if isinstance(msg, dict):
        return (msg.get("qos", 0), bool(msg.get("retain")), msg.get("from"), bool(msg.get("retained")))
    return (0, False, None, False)


class GpuRoutes:
    """The aggregator's index over the route filters, with the local
    subscribers' ids as fan-out lists (mirror of the gen_server state of
    nif/emqx_gpu_match_batcher.erl).  A filter is in the index while it has a
    local subscriber or another destination (route_add)."""

    def __init__(self, ctx, node: bytes = b"node", cluster=None, combiner=None):
        self.ctx, self.node = ctx, _b(node)
        self.cluster = cluster                 # a ClusterRoutes: the node destinations, for the window's forward plan
        self.combiner = combiner               # a Combiner of ctx (load-info coalesce): the batch call goes through it
        self.index = ctx.build_index([], subs=[])  # load_index([], []) at init
        self.ops: List[Tuple[bytes, int, str]] = []  # since the snapshot, oldest first
        self.ids: Dict[object, int] = {}       # subscriber -> id
        self._next_id = 0                      # monotonic, as next_id in the Erlang server: a
                                               # subscriber that went down never lends its id
        self.subs: Dict[int, object] = {}      # id -> subscriber (the ?SUBS table)
        self.filters_of: Dict[object, set] = {}
        self.other: Dict[bytes, int] = {}      # filter -> destinations other than node (?OTHER)
        self.updates = 0
        self.builds = 1
        self.stale = False
        self._names: Dict[int, bytes] = {}     # filter id -> bytes of the current snapshot
        self._lock = threading.Lock()
        self.opts: Dict[Tuple[bytes, int], int] = {}  # (filter, subscriber id) -> option byte, where given
        self.subopts_on = False                # a subscription gave options, or a batcher asked for them
        self._so_table = None                  # the SubOptTable of the current snapshot
        self._so_index_h = None
        self._so_dirty = True
        self.subopts_builds = 0

    # ---- maintenance (handle_call subscribe / unsubscribe / route, 'DOWN')
    def subscribe(self, filt, sub, opts=None) -> None:
        """``opts``: the subscription's options (a ``pack_opt`` byte or its keyword
        dict: qos, nl, rap, upgrade_qos); None leaves the pair at the default."""
        f = _b(filt)
        with self._lock:
            sid = self.ids.get(sub)
            if sid is None:
                sid = self.ids[sub] = self._next_id
                self._next_id += 1
                self.subs[sid] = sub
            if opts is not None:
                from .subopts import pack_opt
                self.opts[(f, sid)] = pack_opt(**opts) if isinstance(opts, dict) else int(opts)
                self.subopts_on = self._so_dirty = True
            self.filters_of.setdefault(sub, set()).add(f)
            self.ops.append((f, sid, "subscribe"))

    def unsubscribe(self, filt, sub) -> None:
        f = _b(filt)
        with self._lock:
            sid = self.ids.get(sub)
            if sid is None:
                return
            self.filters_of.get(sub, set()).discard(f)
            if self.opts.pop((f, sid), None) is not None:
                self._so_dirty = True
            self.ops.append((f, sid, "unsubscribe"))

    def subscriber_down(self, sub) -> None:
        """emqx_broker_helper's subscriber_down: every subscription of the subscriber goes."""
        with self._lock:
            sid = self.ids.pop(sub, None)
            if sid is None:
                return
            for f in sorted(self.filters_of.pop(sub, set())):
                if self.opts.pop((f, sid), None) is not None:
                    self._so_dirty = True
                self.ops.append((f, sid, "unsubscribe"))
            self.subs.pop(sid, None)

    def route_add(self, filt, dest) -> None:
        self._route(_b(filt), dest, 1)

    def route_delete(self, filt, dest) -> None:
        self._route(_b(filt), dest, -1)

    def _route(self, f: bytes, dest, d: int) -> None:
        if not isinstance(dest, tuple) and _b(dest) == self.node:  # the local route follows the local subscribers
            return
        with self._lock:
            old = self.other.get(f, 0)
            new = max(0, old + d)
            if new:
                self.other[f] = new
            else:
                self.other.pop(f, None)
            if self.cluster is not None and not isinstance(dest, tuple):
                # the node destination itself, in the critical section that queues the mark
                (self.cluster.add_route if d > 0 else self.cluster.delete_route)(f, dest)
            if old == 0 and new > 0:
                self.ops.append((f, 0, "route_add"))
            elif old > 0 and new == 0:
                self.ops.append((f, 0, "route_delete"))

    def refresh(self) -> None:
        """The queued ops applied to the last snapshot with one update_subs; on
        failure they stay queued and the snapshot is stale until a retry works."""
        with self._lock:
            ops, self.ops = self.ops, []
        if not ops:
            self.stale = False
            self._refresh_subopts()
            return
        try:
            new = self.ctx.update_subs(self.index, ops)
        except Exception:
            with self._lock:
                self.ops = ops + self.ops
            self.stale = True
            return
        self.index, self._names = new, {}
        self.updates += 1
        self.stale = False
        self._refresh_subopts()

    def _refresh_subopts(self) -> None:
        """The option table of the current snapshot, beside the destination table:
        rebuilt when an option changed or the snapshot is another one (the table
        is immutable; an entry whose pair the snapshot does not hold -- its
        subscribe is still queued -- is left out of this build)."""
        if not self.subopts_on or self.stale:
            return
        if self._so_table is not None and not self._so_dirty and self._so_index_h is self.index.h:
            return
        with self._lock:
            entries = [(f, sid, o) for (f, sid), o in self.opts.items()]
            self._so_dirty = False
        new = self.ctx.build_subopts(self.index, entries, default=0, skip_unknown=True)
        if self._so_table is not None:
            self._so_table.release()
        self._so_table, self._so_index_h = new, self.index.h
        self.subopts_builds += 1

    # ---- the batch call (fanout_batch/2)
    def groups(self, topics: Sequence[bytes]) -> List[Row]:
        return self.groups_rows(topics)[0]

    def groups_rows(self, topics: Sequence[bytes]):
        """``groups`` plus what it was cut from: (rows, snapshot, (row_off, filter
        ids)) -- the matched rows a SharedSub.dispatch_batch picks from."""
        self.refresh()
        if self.stale:
            raise RuntimeError("stale_index")
        idx = self.index
        # (the NIF's fanout_batch/2: emqx_gm_match_fanout, the match and its fan-out in one call)
        # (with a combiner: the same call, coalesced with the windows of concurrent callers)
        (ro, ids), (fro, fids) = (self.combiner or self.ctx).match_fanout(idx, list(topics), exact=True)
        return self._cut(idx, ro, ids, fro, fids), idx, (ro, ids)

    def groups_opts(self, topics: Sequence[bytes], msg_flags, msg_from, drop: bool = False) -> List[Row]:
        """``groups`` with the option bytes: each (filter, _IdsOpts) carries the
        segment's ids and their delivery bytes (emqx_gm_deliver, FLAG mode, on
        the window's matched rows); with ``drop`` the marked deliveries are
        removed here and counted in the segment's ``dropped``."""
        self.subopts_on = True
        self.refresh()
        if self.stale:
            raise RuntimeError("stale_index")
        idx, tab = self.index, self._so_table
        ro, ids = self.ctx.match(idx, list(topics), exact=True)
        # FLAG mode: the deliveries are the fan-out's, so a row is cut per filter by the snapshot's own
        # counts; the device's bit 4 is the one verdict on No Local, and `drop` removes what it marks
        d = tab.deliver((ro, ids), msg_flags, msg_from, False, index=idx)
        return self._cut_opts(idx, ro, ids, d, drop)

    def groups_batches(self, topics: Sequence[bytes], msg_flags, msg_from, mode: str = "flag"):
        """The window's session batches next to its groups: one match, one
        emqx_gm_deliver_batches on its rows.  Returns (rows, names, batches):
        rows[k] = [(filter, filter id, subscribers listed)] per matched filter of
        topic k, names = {filter id: filter}, batches the ``SessionBatches`` --
        per subscriber id its (row, filter id, byte) entries in window order.
        ``mode``: "flag", "drop" or "lead" (the reference's dropwhile)."""
        self.subopts_on = True
        self.refresh()
        if self.stale:
            raise RuntimeError("stale_index")
        idx, tab = self.index, self._so_table
        ro, ids = self.ctx.match(idx, list(topics), exact=True)
        sb = tab.deliver_batches((ro, ids), msg_flags, msg_from, mode, index=idx)
        rows, names = [], {}
        for k in range(len(ro) - 1):
            row = []
            for f in ids[ro[k]:ro[k + 1]].tolist():
                name = self._names.get(f)
                if name is None:
                    name = self._names[f] = idx.filter(f)
                names[f] = name
                row.append((name, f, idx.subscriber_count(f)))
            rows.append(row)
        return rows, names, sb

    def _cut_opts(self, idx, ro, ids, d, drop: bool) -> List[Row]:
        """FLAG-mode deliveries (a ``Delivered``) cut into one (filter, _IdsOpts) per matched filter."""
        out = []
        for k in range(len(ro) - 1):
            row, pos = [], int(d.row_off[k])
            for f in ids[ro[k]:ro[k + 1]].tolist():
                c = idx.subscriber_count(f)
                name = self._names.get(f)
                if name is None:
                    name = self._names[f] = idx.filter(f)
                sids, bytes_, gone = d.ids[pos:pos + c], d.dopt[pos:pos + c], 0
                if drop:
                    keep = (bytes_ & 0x10) == 0
                    gone = int(c - keep.sum())
                    if gone:
                        sids, bytes_ = sids[keep], bytes_[keep]
                row.append((name, _IdsOpts(sids, bytes_, gone)))
                pos += c
            if pos != int(d.row_off[k + 1]):
                raise RuntimeError("deliveries do not add up to the snapshot's subscriber counts")
            out.append(row)
        return out

    def _cut(self, idx, ro, ids, fro, fids) -> List[Row]:
        """Each fan-out row cut back into one segment per matched filter."""
        out = []
        for k in range(len(ro) - 1):
            row, pos = [], int(fro[k])
            for f in ids[ro[k]:ro[k + 1]].tolist():
                c = idx.subscriber_count(f)
                name = self._names.get(f)
                if name is None:
                    name = self._names[f] = idx.filter(f)
                row.append((name, fids[pos:pos + c]))
                pos += c
            assert pos == int(fro[k + 1])
            out.append(row)
        return out

    def window(self, topics: Sequence[bytes], shared=None, strategy="round_robin", hashes=None, cluster=None,
               opts=None, drop: bool = False):
        """``groups_rows`` plus the window's shared picks (``shared``, a SharedSub:
        what its ``dispatch_batch`` gives, same per-call seed rule) and forward
        plan (``cluster``, a ClusterRoutes: what its ``plan`` gives) from ONE
        ``Context.publish_window`` call -- one device round trip where the three
        calls make five waits; with a combiner, ``Combiner.publish_window``: the
        same call, coalesced with the whole windows of concurrent callers.  Returns (rows, snapshot, (row_off, filter ids),
        picks per row or None, ForwardPlan or None, stats).

        ``opts = (msg_flags, msg_from)``: the rows carry the option bytes, cut as
        ``groups_opts`` cuts them -- ``(filter, _IdsOpts)``, FLAG mode on the
        device, ``drop`` applied here from bit 4 -- and come from the same one
        call (emqx_gm_publish_window_deliver: the deliveries in place of the plain
        fan-out).  That call runs on the context directly, also when the routes
        were built over a combiner."""
        if opts is not None:
            self.subopts_on = True
        self.refresh()
        if self.stale:
            raise RuntimeError("stale_index")
        idx = self.index
        st = shared.table(idx) if shared is not None else None
        dt = cluster.table(idx) if cluster is not None else None
        if opts is not None:
            (ro, ids), d, picks, plan, stats = self.ctx.publish_window(
                idx, list(topics), exact=True, shared=st, strategy=strategy, hashes=hashes,
                seed=shared.next_seed() if shared is not None else 0, dests=dt,
                skip_node=cluster.self_id if cluster is not None else None,
                subopts=self._so_table, msg_flags=opts[0], msg_from=opts[1], drop=False)
            rows = self._cut_opts(idx, ro, ids, d, drop)
            return rows, idx, (ro, ids), (shared.picks_rows(*picks) if shared is not None else None), plan, stats
        (ro, ids), (fro, fids), picks, plan, stats = (self.combiner or self.ctx).publish_window(
            idx, list(topics), exact=True, shared=st, strategy=strategy, hashes=hashes,
            seed=shared.next_seed() if shared is not None else 0, dests=dt,
            skip_node=cluster.self_id if cluster is not None else None)
        rows = self._cut(idx, ro, ids, fro, fids)
        return rows, idx, (ro, ids), (shared.picks_rows(*picks) if shared is not None else None), plan, stats


class PublishBatcher:
    """Size/time-window aggregator over a groups function (server side) plus the
    caller-side publish/1 around it (see the module doc).

    Caller-side collaborators (defaults: inert): ``subscribers`` maps subscriber
    id -> subscriber for ``deliver(sub, filter, msg) -> bool`` (False: not
    alive); ``lookup_routes(filter) -> [dest]`` with ``others`` the filters that
    have non-local destinations; ``forward(node, filter, msg)``;
    ``shared_dispatch(group, filter, msg)``; ``fallback(topic) -> [(filter,
    dest)]`` (match_routes/1) with ``fallback_dispatch(filter, msg)``;
    ``on_dropped(msg)`` (the 'message.dropped' hook); ``persist(topic, msg)``;
    ``metrics`` counts messages.publish / dropped / dropped.no_subscribers.
    A dest is the node name (bytes or str) or a (group, node) tuple.

    ``routes`` (a GpuRoutes) wires the server's own index in one argument:
    ``groups_fn`` defaults to ``routes.groups``, ``others`` to ``routes.other``
    (the ?OTHER table the Erlang caller reads directly) and ``subscribers`` to
    ``routes.subs``.  A ``groups_fn`` that is a bound ``GpuRoutes.groups`` gets
    its ``others`` the same way, so remote and shared routes cannot be dropped
    by forgetting the second argument.

    ``shared`` (a SharedSub; needs ``routes``): a window's shared deliveries are
    resolved with ONE ``shared.dispatch_batch`` over the window's matched rows
    (strategy ``shared_strategy``; ``shared_hash(topic, msg) -> u32`` stands in
    for erlang:phash2/1 of the client id or source topic, default: CRC-32 of
    the topic) instead of one ``shared_dispatch`` call per message and group.
    The picked member gets ``deliver(sub, filter, msg)``; if that fails the
    caller walks the rest of subscribers/2, as dispatch/4's FailedSubs loop
    does.  A group the table holds no member for goes to ``shared_dispatch``.
    Without ``shared`` nothing changes.

    ``cluster`` (a ClusterRoutes; needs ``routes``): a window's remote node
    routes come from ONE ``cluster.plan`` over the window's matched rows and
    go out with ONE ``forward_batch(node, [(filter, msg), ...])`` per node with
    work -- the node's pairs in publish order -- instead of lookup_routes/1 and
    ``forward`` per (message, route).  What ``forward_batch`` returns (an
    exception: ("error", "badrpc")) is recorded as the result of each of its
    pairs.  ``lookup_routes`` is then consulted for group destinations only.
    A message's forwards leave with its window, so ``submit`` takes the
    message too.  Without ``cluster`` nothing changes.

    ``one_call`` (needs ``routes``; used when ``shared`` or ``cluster`` is
    given): the window's rows, picks and plan come from ONE ``routes.window``
    call (emqx_gm_publish_window: one device round trip) instead of the three
    calls above; the results are the same.  With ``routes`` built over a
    combiner (``GpuRoutes(ctx, combiner=cb)``) that call goes through it
    (emqx_gm_combiner_publish): whole windows of concurrent batchers share one
    device round trip.

    ``subopts`` (needs ``routes``; with ``shared`` / ``cluster`` only together
    with ``one_call``): the window's local deliveries come from
    ``routes.groups_opts`` (one match, one emqx_gm_deliver) with the byte
    emqx_session:enrich_deliver/2 would compute beside every subscriber id, and
    ``deliver`` is called as ``deliver(sub, filter, msg, byte)``
    (``unpack_dopt``).  With ``one_call`` they come from the window call itself
    (``routes.window(..., opts=)``, emqx_gm_publish_window_deliver: the
    deliveries with their bytes in the window's one device round trip, beside
    the picks and the plan); the deliveries and metrics are the same.  ``msg_meta(topic, msg) -> (qos,
    retain, from[, headers.retained])`` reads a message; ``from`` is the
    publishing subscriber as ``routes.ids`` knows it, or None.
    ``drop_no_local`` removes the deliveries the device marked as No-Local hits
    (bit 4) and counts them in ``metrics['delivery.dropped.no_local']``;
    otherwise the bit goes to ``deliver`` and the session drops what
    ignore_local/4 would.  Without
    ``subopts`` nothing changes.

    ``batches`` (needs ``subopts`` and ``deliver_batch``; not with ``one_call``,
    ``shared`` or ``cluster`` for now): the window's local deliveries go out by
    SUBSCRIBER -- ``routes.groups_batches`` (one match, one
    emqx_gm_deliver_batches) and ONE ``deliver_batch(sub, [(filter, msg, byte),
    ...]) -> bool`` per subscriber per window, its deliveries in window order:
    the list emqx_channel:handle_deliver/2 gets from a drained mailbox.
    ``drop_no_local`` then selects the reference's own rule (EMQX_GM_SO_LEAD:
    only the leading run of hits of a batch is removed, bit 4 cleared) and
    ``metrics['delivery.dropped.no_local']`` counts what it removed
    (``batch_dropped``).  A subscriber whose batch was emptied gets no call.
    Without ``batches`` nothing changes."""

    def __init__(self, groups_fn: Optional[Callable[[Sequence[bytes]], List[Row]]] = None, max_batch: int = 4096,
                 window_s: float = 0.001, subscribers: Optional[Dict[int, object]] = None,
                 deliver: Optional[Callable[[object, bytes, object], bool]] = None,
                 clock: Callable[[], float] = time.monotonic, timer: bool = True, node: bytes = b"node",
                 lookup_routes: Optional[Callable[[bytes], List[object]]] = None, others=None,
                 forward: Optional[Callable[[bytes, bytes, object], object]] = None,
                 shared_dispatch: Optional[Callable[[object, bytes, object], object]] = None,
                 fallback: Optional[Callable[[bytes], List[Tuple[bytes, object]]]] = None,
                 fallback_dispatch: Optional[Callable[[bytes, object], object]] = None,
                 on_dropped: Optional[Callable[[object], None]] = None,
                 persist: Optional[Callable[[bytes, object], None]] = None,
                 routes: Optional[GpuRoutes] = None, shared=None, shared_strategy: str = "round_robin",
                 shared_hash: Optional[Callable[[bytes, object], int]] = None, cluster=None,
                 forward_batch: Optional[Callable[[bytes, List[Tuple[bytes, object]]], object]] = None,
                 one_call: bool = False, subopts: bool = False, drop_no_local: bool = False,
                 msg_meta: Callable[[bytes, object], tuple] = msg_meta, batches: bool = False,
                 deliver_batch: Optional[Callable[[object, List[Tuple[bytes, object, int]]], bool]] = None):
        if routes is None and isinstance(getattr(groups_fn, "__self__", None), GpuRoutes):
            routes = groups_fn.__self__
        if groups_fn is None:
            if routes is None:
                raise TypeError("PublishBatcher needs groups_fn or routes")
            groups_fn = routes.groups
        if routes is not None:
            if others is None:
                others = routes.other
            if subscribers is None:
                subscribers = routes.subs
        if shared is not None and routes is None:
            raise TypeError("PublishBatcher(shared=...) needs routes (the window's matched rows)")
        if cluster is not None and routes is None:
            raise TypeError("PublishBatcher(cluster=...) needs routes (the window's matched rows)")
        if one_call and routes is None:
            raise TypeError("PublishBatcher(one_call=True) needs routes (the window call)")
        if subopts and routes is None:
            raise TypeError("PublishBatcher(subopts=True) needs routes")
        if subopts and not one_call and (shared is not None or cluster is not None):
            raise TypeError("PublishBatcher(subopts=True) with shared / cluster needs one_call=True (the window call)")
        if batches and one_call:
            raise TypeError("PublishBatcher(batches=True) with one_call is not supported yet")
        if batches and (not subopts or deliver_batch is None):
            raise TypeError("PublishBatcher(batches=True) needs subopts=True and deliver_batch")
        self.subopts, self.drop_no_local, self.msg_meta = subopts, drop_no_local, msg_meta
        self.by_batch, self.deliver_batch = batches, deliver_batch
        self.one_call = one_call
        self.routes, self.shared, self.shared_strategy = routes, shared, shared_strategy
        self.cluster = cluster
        self.forward_batch = forward_batch or (lambda node, pairs: ("error", "badrpc"))
        self.shared_hash = shared_hash or (lambda topic, msg: zlib.crc32(topic))
        self.groups_fn = groups_fn
        self.max_batch = max_batch
        self.window_s = window_s
        self.subscribers = subscribers if subscribers is not None else {}
        self.deliver = deliver or (lambda sub, filt, msg: sub.append((filt, msg)) or True)
        self.clock = clock
        self.node = _b(node)
        self.lookup_routes = lookup_routes or (lambda f: [])
        self.others = others if others is not None else {}
        self.forward = forward or (lambda node, f, msg: ("error", "badrpc"))
        self.shared_dispatch = shared_dispatch or (lambda group, f, msg: ("error", "no_subscribers"))
        self.fallback = fallback
        self.fallback_dispatch = fallback_dispatch or (lambda f, msg: ("error", "no_subscribers"))
        self.on_dropped = on_dropped or (lambda msg: None)
        self.persist = persist or (lambda topic, msg: None)
        self.metrics = {"messages.publish": 0, "messages.dropped": 0, "messages.dropped.no_subscribers": 0}
        if subopts:
            self.metrics["delivery.dropped.no_local"] = 0
        self.batches = 0
        self.messages = 0
        self._mlock = threading.Lock()
        self._pending: List[Tuple[bytes, Future, object]] = []
        self._deadline: Optional[float] = None
        self._cv = threading.Condition()
        self._closed = False
        self._thread = None
        if timer:
            self._thread = threading.Thread(target=self._run, daemon=True)
            self._thread.start()

    # ---------------------------------------------------------------- server side
    def submit(self, topic, msg=None) -> Future:
        """Queue one topic's match; the future resolves to ("ok", row) or
        ("error", reason) once its batch is matched (at most window_s after the
        batch's first topic)."""
        fut: Future = Future()
        flush = None
        with self._cv:
            self._pending.append((_b(topic), fut, msg))
            if len(self._pending) == 1:
                self._deadline = self.clock() + self.window_s  # the window starts with the batch
                self._cv.notify()
            if len(self._pending) >= self.max_batch:
                flush = self._take()
        if flush:
            self._match(flush)
        return fut

    def poll(self) -> int:
        """Flush if the window has expired (the timer thread's step; tests call it
        with a fake clock).  Returns the number of topics matched."""
        with self._cv:
            due = self._pending and self._deadline is not None and self.clock() >= self._deadline
            batch = self._take() if due else []
        if batch:
            self._match(batch)
        return len(batch)

    def flush(self) -> int:
        with self._cv:
            batch = self._take()
        if batch:
            self._match(batch)
        return len(batch)

    def close(self):
        with self._cv:
            self._closed = True
            self._cv.notify()
        if self._thread:
            self._thread.join()
        self.flush()

    def _take(self):
        batch, self._pending, self._deadline = self._pending, [], None
        return batch

    def _run(self):
        while True:
            with self._cv:
                while not self._closed and not self._pending:
                    self._cv.wait()
                if self._closed:
                    return
                wait = self._deadline - self.clock() if self._deadline is not None else 0.0
                if wait > 0:
                    self._cv.wait(timeout=wait)
            self.poll()

    def _msg_opts(self, topics, msgs):
        """The window's message bytes and publishers: (``pack_msg`` bytes, ``routes.ids`` ids or None)."""
        from .subopts import pack_msg
        meta = [tuple(self.msg_meta(t, m)) + (False,) for t, m in zip(topics, msgs)]
        flags = [pack_msg(q, rt, hdr) for q, rt, _, hdr, *_ in meta]
        froms = [self.routes.ids.get(frm) if frm is not None else None for _, _, frm, *_ in meta]
        return flags, froms

    def _rows(self, topics: Sequence[bytes], msgs: Optional[Sequence[object]] = None):
        try:
            if self.shared is not None or self.cluster is not None or (self.subopts and self.one_call):
                msgs = msgs if msgs is not None else [None] * len(topics)
                hashes = None
                if self.shared is not None and self.shared_strategy.startswith("hash"):
                    hashes = [self.shared_hash(t, m) & 0xFFFFFFFF for t, m in zip(topics, msgs)]
                plan = None
                if self.one_call and self.subopts:  # ... and the deliveries' option bytes, the same one call
                    rows, idx, csr, picks, plan, _ = self.routes.window(
                        list(topics), shared=self.shared, strategy=self.shared_strategy, hashes=hashes,
                        cluster=self.cluster, opts=self._msg_opts(topics, msgs), drop=self.drop_no_local)
                    if picks is None:
                        picks = [None] * len(rows)
                elif self.one_call:  # rows, picks and plan: one device call
                    rows, idx, csr, picks, plan, _ = self.routes.window(
                        list(topics), shared=self.shared, strategy=self.shared_strategy, hashes=hashes,
                        cluster=self.cluster)
                    if picks is None:
                        picks = [None] * len(rows)
                else:
                    rows, idx, csr = self.routes.groups_rows(list(topics))
                    picks = [None] * len(rows)
                    if self.shared is not None:  # the window's shared picks: one device call
                        picks = self.shared.dispatch_batch(idx, csr, self.shared_strategy, hashes)
                if self.cluster is None:
                    return [("ok", r, p) for r, p in zip(rows, picks)]
                return [("ok", r, p, w) for r, p, w in zip(rows, picks, self._forward_window(idx, csr, msgs, plan))]
            if self.by_batch:  # the window's local deliveries by subscriber: one match, one batches call
                msgs = msgs if msgs is not None else [None] * len(topics)
                flags, froms = self._msg_opts(topics, msgs)
                rows, names, sb = self.routes.groups_batches(list(topics), flags, froms,
                                                             "lead" if self.drop_no_local else "flag")
                return [("ok", r) for r in self._deliver_batches(rows, names, sb, msgs)]
            if self.subopts:  # the window's deliveries with their option bytes: one match, one deliver call
                msgs = msgs if msgs is not None else [None] * len(topics)
                flags, froms = self._msg_opts(topics, msgs)
                return [("ok", r) for r in self.routes.groups_opts(list(topics), flags, froms, self.drop_no_local)]
            return [("ok", r) for r in self.groups_fn(list(topics))]
        except Exception as e:  # the NIF's {error, _}: every caller takes the reference path
            return [("error", str(e))] * len(topics)

    def _deliver_batches(self, rows, names, sb, msgs) -> List[Row]:
        """One ``deliver_batch`` per subscriber of the window (handle_deliver/2's
        list); per row, [(filter, _Counted)] for ``route_row``'s bookkeeping.
        The counts are kept per (row, filter id): a matched row lists a filter
        once (the match's rows are sets), so a segment is one key."""
        kept: Dict[Tuple[int, int], int] = {}
        took: Dict[Tuple[int, int], int] = {}
        for sid, rws, fls, bts in sb.batches():
            keys = list(zip(rws.tolist(), fls.tolist()))
            for k in keys:
                kept[k] = kept.get(k, 0) + 1
            sub = self.subscribers.get(int(sid))
            if sub is None or not keys:
                continue
            if self.deliver_batch(sub, [(names[f], msgs[r], b) for (r, f), b in zip(keys, bts.tolist())]):
                for k in keys:
                    took[k] = took.get(k, 0) + 1
        if sb.batch_dropped is not None:
            with self._mlock:
                self.metrics["delivery.dropped.no_local"] += int(sb.batch_dropped.sum())
        return [[(name, _Counted(listed, kept.get((k, f), 0), took.get((k, f), 0))) for name, f, listed in row]
                for k, row in enumerate(rows)]

    def _forward_window(self, idx, csr, msgs, plan=None):
        """The window's remote node routes: one plan call (or the window call's
        ``plan``), one forward_batch per node with work.  Per row, [(node,
        filter, result)]."""
        if plan is None:
            plan = self.cluster.plan(idx, csr)
        names: Dict[int, bytes] = {}
        out: List[list] = [[] for _ in msgs]
        for k in range(len(plan.node_off) - 1):
            rws, fls = plan.node(k)
            if not len(rws):
                continue
            node = self.cluster.nodes[k]
            pairs = []
            for r, f in zip(rws.tolist(), fls.tolist()):
                name = names.get(f)
                if name is None:
                    name = names[f] = idx.filter(f)
                pairs.append((r, name))
            try:
                res = self.forward_batch(node, [(name, msgs[r]) for r, name in pairs])
            except Exception:
                res = ("error", "badrpc")
            for r, name in pairs:
                out[r].append((node, name, res))
        return out

    def _match(self, batch):
        rows = self._rows([t for t, _, _ in batch], [m for _, _, m in batch])
        with self._mlock:
            self.batches += 1
            self.messages += len(batch)
        for (_, fut, _), row in zip(batch, rows):
            fut.set_result(row)

    # ---------------------------------------------------------------- caller side
    def _inc(self, name: str):
        with self._mlock:
            self.metrics[name] += 1

    def prepare(self, topic, msg):
        """publish/1 before the match: the publish metric (not for $SYS) and
        persist_message/1 (the 'message.publish' hook is the caller's own)."""
        t = _b(topic)
        if not is_sys(t):
            self._inc("messages.publish")
        self.persist(t, msg)
        return t

    def publish(self, topic, msg=None) -> Result:
        """emqx_broker:publish/1 with the match batched: blocks until the batch
        holding the topic is matched, then routes in the calling thread."""
        t = self.prepare(topic, msg)
        return self.route_row(self.submit(t, msg).result(), t, msg)

    def publish_batch(self, items: Sequence[Tuple[object, object]]) -> List[Result]:
        """Messages the caller already holds: one groups call, results in order."""
        topics = [self.prepare(t, m) for t, m in items]
        rows = self._rows(topics, [m for _, m in items])
        with self._mlock:
            self.batches += 1
            self.messages += len(topics)
        return [self.route_row(r, t, m) for r, t, (_, m) in zip(rows, topics, items)]

    def route_row(self, row, topic: bytes, msg) -> Result:
        """route(aggre(Routes)) over a matched row (emqx_broker.erl:245-273)."""
        if row[0] == "ok":
            routes: List[tuple] = [(f, self.node, ids) for f, ids in row[1] if len(ids) or getattr(ids, "dropped", 0)]
            sent = row[3] if len(row) > 3 else None  # the window's forwards of this row: [(node, filter, result)]
            other = [(f, d) for f, _ in row[1] if f in self.others for d in self.lookup_routes(f)
                     if isinstance(d, tuple) or (sent is None and _b(d) != self.node)]
            if sent is not None:
                other += [(f, _Sent(node, res)) for node, f, res in sent]
        else:  # the reference path
            routes, other = [], list(self.fallback(topic)) if self.fallback else []
        picks = {(_b(g), f): sub for g, f, sub in row[2]} if len(row) > 2 and row[2] is not None else None
        routes += self.aggre(other)
        if not routes:  # route([], _): no subscribers anywhere
            self.dropped(topic, msg)
            return []
        out: Result = []
        for r in routes:  # lists:foldl prepending, as route/2
            out.insert(0, self.do_route(r, topic, msg, picks))
        return out

    @staticmethod
    def aggre(routes: Sequence[Tuple[bytes, object]]) -> List[tuple]:
        """aggre/1: (filter, node) per node route, one (filter, group) per shared group."""
        nodes = [(f, d if isinstance(d, _Sent) else _b(d)) for f, d in routes if not isinstance(d, tuple)]
        groups = sorted({(f, ("group", d[0])) for f, d in routes if isinstance(d, tuple)})
        return nodes + groups

    def do_route(self, r, topic: bytes, msg, picks=None):
        if len(r) == 3:  # a local route with the GPU fan-out's subscriber ids
            f, node, ids = r
            return (node, f, self.dispatch_ids(f, ids, topic, msg))
        f, d = r
        if isinstance(d, _Sent):  # forwarded with its window's batch: the recorded result
            return (d.node, f, d.res)
        if isinstance(d, tuple):  # ("group", G): emqx_shared_sub:dispatch/3
            if picks is not None and (_b(d[1]), f) in picks:
                return ("share", f, self.deliver_shared(d[1], f, picks[(_b(d[1]), f)], msg))
            return ("share", f, self.shared_dispatch(d[1], f, msg))
        if _b(d) == self.node:
            return (d, f, self.fallback_dispatch(f, msg))
        return (d, f, self.forward(d, f, msg))

    def deliver_shared(self, group, f: bytes, sub, msg):
        """dispatch/4 (emqx_shared_sub.erl:118-130) from the window's pick on: the
        picked member first, then the others of subscribers/2 (FailedSubs)."""
        if self.deliver(sub, f, msg):
            return ("ok", 1)
        for other in self.shared.subscribers(group, f):
            if other is not sub and self.deliver(other, f, msg):
                return ("ok", 1)
        return ("error", "no_subscribers")

    def dispatch_ids(self, f: bytes, ids, topic: bytes, msg):
        """do_dispatch/2,3: one delivery per live subscriber; none live is a drop."""
        n = 0
        if isinstance(ids, _Counted):  # already delivered with its window's session batches
            if ids.n or ids.kept < ids.listed:  # (removed as no_local in its session: not a no_subscribers drop)
                return ("ok", ids.n)
            self.dropped(topic, msg)
            return ("error", "no_subscribers")
        if isinstance(ids, _IdsOpts):  # the option byte goes with the id: deliver(sub, filter, msg, byte)
            for sid, b in zip(ids.ids.tolist(), ids.dopt.tolist()):
                sub = self.subscribers.get(int(sid))
                if sub is not None and self.deliver(sub, f, msg, b):
                    n += 1
            if ids.dropped:  # delivered to its session and dropped there as no_local: not a no_subscribers drop
                with self._mlock:
                    self.metrics["delivery.dropped.no_local"] += ids.dropped
            if n or ids.dropped:
                return ("ok", n)
            self.dropped(topic, msg)
            return ("error", "no_subscribers")
        for sid in (ids.tolist() if hasattr(ids, "tolist") else ids):
            sub = self.subscribers.get(int(sid))
            if sub is not None and self.deliver(sub, f, msg):
                n += 1
        if n:
            return ("ok", n)
        self.dropped(topic, msg)
        return ("error", "no_subscribers")

    def dropped(self, topic: bytes, msg):
        """'message.dropped' hook + inc_dropped_cnt/1 (emqx_broker.erl:245-248, 309-314)."""
        self.on_dropped(msg)
        if not is_sys(topic):
            self._inc("messages.dropped")
            self._inc("messages.dropped.no_subscribers")
