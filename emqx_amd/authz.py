"""Authorization check: the first matching ACL rule per request, on the device.

``AuthzTable`` compiles the reference's rule tuples (a file source,
emqx_authz_rule:compile/1, apps/emqx_authz/src/emqx_authz_rule.erl:55-94) and
the built-in database's records (emqx_authz_mnesia:store_rules/2,
emqx_authz_mnesia.erl:123-132) into the arrays of ``emqx_gm_authz_build``;
``Authz`` is the table resident in HBM, answering windows of requests
``(clientinfo, pubsub, topic)`` with the kernel of gm_authz.hip, bit-equal to
emqx_authz:do_authorize/4 (emqx_authz.erl:307-317) over that chain.  The
library runs no regex: ``AuthzTable.re_mask`` evaluates the table's ``{re, _}``
predicates with Python's ``re`` once per client.  There is no '$'-rule on this
path (emqx_topic:match/2's list clauses): ``#`` authorizes ``$SYS/x``.  There
is no CPU fallback; ``check_host`` is test and measurement support.

Rules are written as the reference writes them, with strings for atoms::

    ("allow", ("username", "dashboard"), "subscribe", ["$SYS/#"])
    ("allow", ("ipaddr", "127.0.0.1"), "all", ["$SYS/#", "#"])
    ("deny", "all", "subscribe", ["$SYS/#", ("eq", "#")])
    ("allow", ("and", [("clientid", ("re", "^test")), ("ipaddrs", ["10.0.0.0/8"])]), "publish", ["t/${clientid}"])
    ("allow", "all")

and a built-in-database record's rules as ``(permission, action, topic)``.
A client is a dict with ``clientid``, ``username`` and ``peerhost`` (missing or
``None``: undefined).
"""

from __future__ import annotations

import ctypes as C
import ipaddress
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import AuthzBatch, AuthzDesc, AuthzInfo, GpuMatchError, check, lib
from .engine import BytesLike, _b, _ptr, pack

GLOBAL, BY_CLIENTID, BY_USERNAME = 0, 1, 2
NOMATCH, ALLOW, DENY = 0, 1, 2
PUBLISH, SUBSCRIBE, ALL = 1, 2, 3
WHO_USERNAME, WHO_CLIENTID, WHO_IPADDR, WHO_REGEX, WHO_AND, WHO_OR = 0, 1, 2, 3, 4, 5
FILTER_PLAIN, FILTER_EQ = 0, 1
F_CLIENTID, F_USERNAME, F_PEERHOST, F_IPV6 = 1, 2, 4, 8
NO_RULE = 0xFFFFFFFF
VERDICTS = {NOMATCH: "nomatch", ALLOW: "allow", DENY: "deny"}

_PERM = {"allow": ALLOW, "deny": DENY}
_ACTION = {"publish": PUBLISH, "subscribe": SUBSCRIBE, "all": ALL}


def cidr_bytes(cidr: str) -> bytes:
    """esockd_cidr:parse(CIDR, true): the family and the inclusive [lo, hi], 33 bytes."""
    net = ipaddress.ip_network(cidr, strict=False)
    lo, hi = net.network_address.packed, net.broadcast_address.packed
    return bytes([net.version]) + lo.ljust(16, b"\0") + hi.ljust(16, b"\0")


class AuthzTable:
    """The ordered segments of one authorization chain, compiled to arrays."""

    def __init__(self):
        self.seg_kind: List[int] = []
        self.seg_ranges: List[List[Tuple[bytes, int, int]]] = []  # per segment: (key, first rule, end rule)
        self.rule_id: List[int] = []
        self.rule_perm: List[int] = []
        self.rule_action: List[int] = []
        self.rule_who_op: List[int] = []
        self.rule_who_off: List[int] = [0]
        self.rule_filter_off: List[int] = [0]
        self.leaf_kind: List[int] = []
        self.leaf_arg: List[bytes] = []
        self.filter_kind: List[int] = []
        self.filter_bytes: List[bytes] = []
        self.regexes: List[Tuple[str, bytes]] = []  # bit k: (field, pattern)
        self._re: List = []

    # ------------------------------------------------------------ sources
    def add_file(self, rules: Sequence, ids: Optional[Sequence[int]] = None) -> List[int]:
        """A file source (emqx_authz_file): one GLOBAL segment.  Returns the rules' ids
        (``ids``, or their positions among all the table's rules)."""
        return self._add_segment(GLOBAL, [(b"", [self._file_rule(r) for r in rules])], ids)

    add_global = add_file

    def add_by_clientid(self, records: Dict[BytesLike, Sequence], ids=None) -> List[int]:
        """The built-in database's clientid records: key -> [(permission, action, topic)]."""
        return self._add_segment(BY_CLIENTID, [(_b(k), [self._db_rule(r) for r in v]) for k, v in records.items()], ids)

    def add_by_username(self, records: Dict[BytesLike, Sequence], ids=None) -> List[int]:
        return self._add_segment(BY_USERNAME, [(_b(k), [self._db_rule(r) for r in v]) for k, v in records.items()], ids)

    def add_builtin_db(self, clientid=None, username=None, all=None) -> List[int]:  # noqa: A002
        """emqx_authz_mnesia:authorize/4 (:95-111): the clientid record's rules, the
        username record's, then the `all` record's."""
        out = self.add_by_clientid(clientid or {})
        out += self.add_by_username(username or {})
        out += self._add_segment(GLOBAL, [(b"", [self._db_rule(r) for r in (all or [])])], None)
        return out

    # ------------------------------------------------------------ compile/1
    def _file_rule(self, rule):
        if len(rule) == 2 and rule[1] == "all":  # compile({Permission, all})
            return (rule[0], ("and", []), "all", ["#"])
        perm, who, action, topics = rule
        return (perm, self._top_who(who), action, list(topics))

    @staticmethod
    def _db_rule(rule):
        perm, action, topic = rule  # do_authorize/4 (:212-218): compile({Permission, all, Action, [TopicFilter]})
        return (perm, ("and", []), action, [topic])

    @staticmethod
    def _top_who(who):
        if who == "all":
            return ("and", [])
        if who[0] in ("and", "or"):
            return (who[0], list(who[1]))
        return ("and", [who])

    def _leaf(self, who) -> Tuple[int, bytes]:
        kind, arg = who
        kind = {"user": "username", "client": "clientid"}.get(kind, kind)
        if kind in ("and", "or"):  # nested: the library refuses it
            return (WHO_AND if kind == "and" else WHO_OR), b""
        if kind in ("username", "clientid"):
            if isinstance(arg, tuple) and arg[0] == "re":
                key = (kind, _b(arg[1]))
                if key not in self.regexes:
                    self.regexes.append(key)
                    self._re.append(re.compile(key[1]))
                return WHO_REGEX, bytes([min(self.regexes.index(key), 255)])
            return (WHO_USERNAME if kind == "username" else WHO_CLIENTID), _b(arg)
        if kind == "ipaddr":
            return WHO_IPADDR, cidr_bytes(arg)
        if kind == "ipaddrs":
            return WHO_IPADDR, b"".join(cidr_bytes(c) for c in arg)
        raise ValueError(f"unknown who: {who!r}")

    @staticmethod
    def _filter(topic) -> Tuple[int, bytes]:
        if isinstance(topic, tuple) and topic[0] == "eq":  # compile_topic({eq, Topic})
            return FILTER_EQ, _b(topic[1])
        t = _b(topic)
        if t.startswith(b"eq "):  # compile_topic(<<"eq ", Topic/binary>>)
            return FILTER_EQ, t[3:]
        return FILTER_PLAIN, t

    def _add_segment(self, kind, ranges, ids) -> List[int]:
        out: List[int] = []
        n_new = sum(len(rs) for _, rs in ranges)
        if ids is not None and len(ids) != n_new:
            raise ValueError("one id per rule")
        seg = []
        for key, rules in ranges:
            lo = len(self.rule_id)
            for perm, (op, leaves), action, topics in rules:
                rid = int(ids[len(out)]) if ids is not None else len(self.rule_id)
                out.append(rid)
                self.rule_id.append(rid)
                self.rule_perm.append(_PERM[perm])
                self.rule_action.append(_ACTION[action] if isinstance(action, str) else int(action))
                self.rule_who_op.append(1 if op == "or" else 0)
                for lf in leaves:
                    k, a = self._leaf(lf)
                    self.leaf_kind.append(k)
                    self.leaf_arg.append(a)
                for t in topics:
                    k, b = self._filter(t)
                    self.filter_kind.append(k)
                    self.filter_bytes.append(b)
                self.rule_who_off.append(len(self.leaf_kind))
                self.rule_filter_off.append(len(self.filter_kind))
            seg.append((key, lo, len(self.rule_id)))
        self.seg_kind.append(kind)
        self.seg_ranges.append(seg)
        return out

    # ------------------------------------------------------------ requests
    def re_mask(self, client: dict) -> int:
        """Bit k: the table's k-th distinct regex matches this client (re:run/2 is
        a search).  Constant per connection, so a caller computes it at connect."""
        m = 0
        for k, ((field, _), rx) in enumerate(zip(self.regexes, self._re)):
            v = client.get(field)
            if v is not None and k < 32 and rx.search(_b(v)):
                m |= 1 << k
        return m

    def desc(self) -> "DescArrays":
        return DescArrays.from_table(self)


class DescArrays:
    """The arrays behind one ``emqx_gm_authz_desc`` (kept alive with it)."""

    def __init__(self, seg_kind, seg_range_off, range_rule_off, keys, rule_id, rule_perm, rule_action, rule_who_op,
                 rule_who_off, rule_filter_off, leaf_kind, leaves, filter_kind, filters):
        u8, u32, u64 = np.uint8, np.uint32, np.uint64

        def arr(a, dt, pad=1):  # never empty: a NULL pointer is refused
            a = np.ascontiguousarray(a, dt)
            return a if len(a) else np.zeros(pad, dt)

        self.n_segments, self.n_ranges = len(seg_kind), len(range_rule_off) - 1
        self.n_rules, self.n_leaves, self.n_filters = len(rule_id), len(leaf_kind), len(filter_kind)
        self.a = [arr(seg_kind, u32), arr(seg_range_off, u64), arr(range_rule_off, u64), keys[0], arr(keys[1], u64),
                  arr(rule_id, u32), arr(rule_perm, u8), arr(rule_action, u8), arr(rule_who_op, u8),
                  arr(rule_who_off, u64), arr(rule_filter_off, u64), arr(leaf_kind, u8), leaves[0],
                  arr(leaves[1], u64), arr(filter_kind, u8), filters[0], arr(filters[1], u64)]

    @classmethod
    def from_table(cls, t: AuthzTable) -> "DescArrays":
        seg_range_off, range_rule_off, keys = [0], [0], []
        for seg in t.seg_ranges:
            for key, _, hi in seg:
                keys.append(key)
                range_rule_off.append(hi)
            seg_range_off.append(len(keys))
        return cls(t.seg_kind, seg_range_off, range_rule_off, pack(keys), t.rule_id, t.rule_perm, t.rule_action,
                   t.rule_who_op, t.rule_who_off, t.rule_filter_off, t.leaf_kind, pack(t.leaf_arg), t.filter_kind,
                   pack(t.filter_bytes))

    def struct(self) -> AuthzDesc:
        p = [a.ctypes.data for a in self.a]
        return AuthzDesc(self.n_segments, p[0], p[1], self.n_ranges, p[2], p[3], p[4], self.n_rules, p[5], p[6], p[7],
                         p[8], p[9], p[10], self.n_leaves, p[11], p[12], p[13], self.n_filters, p[14], p[15], p[16])


class RequestBatch:
    """A window of requests as the arrays of ``emqx_gm_authz_batch``."""

    def __init__(self, topics, clientids, usernames, flags, peerhost, action, re_mask):
        self.n = len(topics[1]) - 1
        z = max(self.n, 1)
        self.a = [topics[0], np.ascontiguousarray(topics[1], np.uint64), clientids[0],
                  np.ascontiguousarray(clientids[1], np.uint64), usernames[0],
                  np.ascontiguousarray(usernames[1], np.uint64),
                  _fit(flags, np.uint8, z), _fit(peerhost, np.uint8, 16 * z), _fit(action, np.uint8, z),
                  _fit(re_mask, np.uint32, z)]

    @classmethod
    def from_requests(cls, requests: Iterable, table: Optional[AuthzTable] = None) -> "RequestBatch":
        """``requests``: (client dict, "publish" | "subscribe", topic); a client's
        ``re_mask`` entry is used when present, else ``table.re_mask(client)``."""
        topics, cids, uns, flags, peers, acts, masks = [], [], [], [], [], [], []
        for client, pubsub, topic in requests:
            cid, un, peer = client.get("clientid"), client.get("username"), client.get("peerhost")
            fl, pb = 0, b"\0" * 16
            if cid is not None:
                fl |= F_CLIENTID
            if un is not None:
                fl |= F_USERNAME
            if peer is not None:
                ip = ipaddress.ip_address(peer)
                fl |= F_PEERHOST | (F_IPV6 if ip.version == 6 else 0)
                pb = ip.packed.ljust(16, b"\0")
            topics.append(topic)
            cids.append(cid if cid is not None else b"")
            uns.append(un if un is not None else b"")
            flags.append(fl)
            peers.append(pb)
            acts.append(_ACTION[pubsub] if isinstance(pubsub, str) else int(pubsub))
            masks.append(client["re_mask"] if "re_mask" in client else (table.re_mask(client) if table else 0))
        return cls(pack(topics), pack(cids), pack(uns), flags, np.frombuffer(b"".join(peers), np.uint8), acts, masks)

    def struct(self) -> AuthzBatch:
        p = [a.ctypes.data for a in self.a]
        return AuthzBatch(self.n, *p)


def _fit(a, dt, n):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return a if len(a) >= n else np.concatenate([a, np.zeros(n - len(a), dt)])


class Authz:
    """One authorization table.  Made by ``Context.build_authz`` (resident in
    HBM) or ``Authz.compile_host`` (host tables only: ``check_host`` works,
    ``authorize`` raises)."""

    def __init__(self, ctx, handle, table: Optional[AuthzTable] = None):
        self.ctx, self.h, self.table = ctx, handle, table

    @classmethod
    def compile_host(cls, table) -> "Authz":
        d = table.desc() if isinstance(table, AuthzTable) else table
        s = d.struct()
        h = C.c_void_p()
        rc = lib().emqx_gm_authz_compile_host(C.byref(s), C.byref(h))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "authz_compile_host")
        return cls(None, h, table if isinstance(table, AuthzTable) else None)

    def _batch(self, requests) -> RequestBatch:
        return requests if isinstance(requests, RequestBatch) else RequestBatch.from_requests(requests, self.table)

    def authorize_batch(self, requests, timed: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """emqx_authz:do_authorize/4 for a window: (verdict uint8[n]: 0 nomatch,
        1 allow, 2 deny; rule uint32[n]: the first matching rule's id, NO_RULE on
        nomatch).  The default for nomatch (authorization.no_match) is the caller's."""
        if self.ctx is None:
            raise GpuMatchError(_lib.EUNSUPPORTED, "authz check: a host-only table")
        b = self._batch(requests)
        verdict, rule = np.zeros(max(b.n, 1), np.uint8), np.full(max(b.n, 1), NO_RULE, np.uint32)
        s = b.struct()
        check(lib().emqx_gm_authz_check(self.ctx.h, self.h, C.byref(s), _lib.AUTHZ_TIMED if timed else 0,
                                        _ptr(verdict), _ptr(rule)), self.ctx.h, "authz_check")
        return verdict[:b.n], rule[:b.n]

    def authorize(self, client: dict, pubsub, topic: BytesLike) -> Tuple[str, Optional[int]]:
        """One request: ("allow" | "deny" | "nomatch", rule id or None)."""
        v, r = self.authorize_batch([(client, pubsub, topic)])
        return VERDICTS[int(v[0])], (None if int(r[0]) == NO_RULE else int(r[0]))

    def check_host(self, requests) -> Tuple[np.ndarray, np.ndarray]:
        """The same walk over the host copy of the tables (single thread, no
        device call): test and measurement support."""
        b = self._batch(requests)
        verdict, rule = np.zeros(max(b.n, 1), np.uint8), np.full(max(b.n, 1), NO_RULE, np.uint32)
        s = b.struct()
        rc = lib().emqx_gm_authz_check_host(self.h, C.byref(s), _ptr(verdict), _ptr(rule))
        if rc != _lib.OK:
            m = lib().emqx_gm_last_error(None)
            raise GpuMatchError(rc, m.decode(errors="replace") if m else "authz_check_host")
        return verdict[:b.n], rule[:b.n]

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        check(lib().emqx_gm_authz_last_kernel_ms(self.h, C.byref(ms)), None, "authz_last_kernel_ms")
        return float(ms.value)

    def info(self) -> AuthzInfo:
        info = AuthzInfo()
        check(lib().emqx_gm_authz_info(self.h, C.byref(info)), None, "authz_info")
        return info

    def release(self):
        if self.h:
            lib().emqx_gm_authz_release(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.release()
        except Exception:
            pass


def build_authz(ctx, table) -> Authz:
    """``Context.build_authz``: an ``AuthzTable`` (or its ``DescArrays``) compiled into HBM."""
    d = table.desc() if isinstance(table, AuthzTable) else table
    s = d.struct()
    h = C.c_void_p()
    check(lib().emqx_gm_authz_build(ctx.h, C.byref(s), 0, C.byref(h)), ctx.h, "authz_build")
    return Authz(ctx, h, table if isinstance(table, AuthzTable) else None)
