"""Plain-Python restatement of the reference's per-delivery subscription-option
path, one branch per Erlang clause (nothing is copied: the clauses are
re-expressed over dicts):

  emqx_session:ignore_local/4   apps/emqx/src/emqx_session.erl:279-291
  emqx_session:get_subopts/2    emqx_session.erl:573-580
  emqx_session:enrich_subopts/3 emqx_session.erl:582-602
  emqx_broker:subscribe/3       apps/emqx/src/emqx_broker.erl:126-138 (the merge over
                                ?DEFAULT_SUBOPTS, include/emqx_mqtt.hrl:193-197)

A message is a dict {qos, retain (flag), retained (headers.retained), from,
nl (flag, set by the walk)}; a session is {subscriptions: {topic: subopts},
upgrade_qos}.  ``World`` holds filters with subscriber lists and the options
per (filter, subscriber), and walks a window the way the library does."""

import random

DEFAULT_SUBOPTS = {"rh": 0, "rap": 0, "nl": 0, "qos": 0}  # emqx_mqtt.hrl:193-197
NONE = 0xFFFFFFFF


def subscribe_opts(subopts0):
    """emqx_broker.erl:128: SubOpts = maps:merge(?DEFAULT_SUBOPTS, SubOpts0)."""
    return {**DEFAULT_SUBOPTS, **subopts0}


def ignore_local_fun(subs, subscriber, deliver):
    """The fun of ignore_local/4 (emqx_session.erl:281-290)."""
    _, topic, msg = deliver
    found = subs.get(topic)                       # :282 maps:find(Topic, Subs)
    if found is not None and found.get("nl") == 1 and subscriber == msg["from"]:  # :283
        return True                               # :287
    return False                                  # :288-289


def ignore_local(delivers, subscriber, session):
    """ignore_local/4 (:279-291): lists:dropwhile -- only the LEADING run is dropped."""
    subs = session["subscriptions"]
    k = 0
    while k < len(delivers) and ignore_local_fun(subs, subscriber, delivers[k]):
        k += 1
    return delivers[k:]


def get_subopts(topic, submap):
    """get_subopts/2 (:573-580)."""
    o = submap.get(topic)
    if o is not None and all(k in o for k in ("nl", "qos", "rap", "subid")):  # :575-576
        return [("nl", o["nl"]), ("qos", o["qos"]), ("rap", o["rap"]), ("subid", o["subid"])]
    if o is not None and all(k in o for k in ("nl", "qos", "rap")):           # :577-578
        return [("nl", o["nl"]), ("qos", o["qos"]), ("rap", o["rap"])]
    return []                                                                   # :579


def enrich_subopts(opts, msg, session):
    """enrich_subopts/3 (:582-602), clause by clause."""
    msg = dict(msg)
    for key, val in opts:
        if key == "nl" and val == 1:                                   # :583-584
            msg["nl"] = True
        elif key == "nl" and val == 0:                                 # :585-586
            pass
        elif key == "qos" and session["upgrade_qos"] is True:          # :587-589
            msg["qos"] = max(val, msg["qos"])
        elif key == "qos" and session["upgrade_qos"] is False:         # :590-592
            msg["qos"] = min(val, msg["qos"])
        elif key == "rap" and val == 1:                                # :593-594
            pass
        elif key == "rap" and val == 0 and msg.get("retained") is True:  # :595-596
            pass
        elif key == "rap" and val == 0:                                # :597-598
            msg["retain"] = False
        elif key == "subid":                                           # :599-602 (not carried by the table)
            msg["subid"] = val
        else:
            raise ValueError((key, val))  # function_clause
    return msg


def enrich_deliver(deliver, session):
    """enrich_deliver/2 (:560-561)."""
    _, topic, msg = deliver
    return enrich_subopts(get_subopts(topic, session["subscriptions"]), msg, session)


def session_deliver(delivers, subscriber, session):
    """What handle_deliver/2 gives a session for one drained batch: ignore_local, then enrich each."""
    return [enrich_deliver(d, session) for d in ignore_local(delivers, subscriber, session)]


# ---- the bytes of include/emqx_gpu_match.h
def opt_byte(o, upgrade_qos=False):
    return o["qos"] | (o["nl"] << 2) | (o["rap"] << 3) | (0x10 if upgrade_qos else 0)


def msg_byte(m):
    return m["qos"] | (4 if m["retain"] else 0) | (8 if m.get("retained") else 0)


def dopt_byte(msg, hit=False):
    return msg["qos"] | (4 if msg["retain"] else 0) | (8 if msg.get("nl") else 0) | (16 if hit else 0)


class World:
    """filters: [bytes] (distinct); lists: per filter its subscriber ids in list
    order; opts: {(filter index, subscriber): subopts dict}; upgrade: {subscriber: bool}."""

    def __init__(self, filters, lists, opts, upgrade=None, default=None):
        self.filters, self.lists, self.opts = filters, lists, opts
        self.upgrade = upgrade or {}
        self.default = default or dict(DEFAULT_SUBOPTS)
        order = sorted(range(len(filters)), key=lambda i: filters[i])
        self.id_of = {i: k for k, i in enumerate(order)}   # input position -> filter id (rank)
        self.by_id = order                                  # filter id -> input position
        self._sessions = None

    def session(self, sub):
        if self._sessions is None:  # every subscriber's subscription map, once
            self._sessions = {}
            for i, lst in enumerate(self.lists):
                for s in lst:
                    self._sessions.setdefault(s, {})[self.filters[i]] = self.opts.get((i, s), self.default)
        return {"subscriptions": self._sessions.get(sub, {}), "upgrade_qos": bool(self.upgrade.get(sub, False))}

    def entries(self):
        return [(self.filters[i], s, opt_byte(o, self.upgrade.get(s, False))) for (i, s), o in self.opts.items()]

    def default_byte(self):
        return opt_byte(self.default)

    def walk_both(self, rows, msgs):
        """rows: per message its matched filter ids in order.  Returns the oracle's
        statement of emqx_gm_deliver in FLAG and in DROP mode, each (row_off, ids,
        dopt, row_dropped), from one pass."""
        f_ro, f_ids, f_opt = [0], [], []
        d_ro, d_ids, d_opt, dropped = [0], [], [], []
        for row, m in zip(rows, msgs):
            nd = 0
            for fid in row:
                i = self.by_id[fid]
                topic = self.filters[i]
                d = ("deliver", topic, dict(m, nl=False))
                for s in self.lists[i]:
                    sess = self.session(s)
                    hit = m["from"] is not None and ignore_local_fun(sess["subscriptions"], s, d)
                    byte = dopt_byte(enrich_deliver(d, sess))
                    f_ids.append(s)
                    f_opt.append(byte | (16 if hit else 0))
                    if hit:
                        nd += 1
                    else:
                        d_ids.append(s)
                        d_opt.append(byte)
            f_ro.append(len(f_ids))
            d_ro.append(len(d_ids))
            dropped.append(nd)
        return (f_ro, f_ids, f_opt, [0] * len(rows)), (d_ro, d_ids, d_opt, dropped)

    def walk(self, rows, msgs, drop):
        return self.walk_both(rows, msgs)[1 if drop else 0]


def csr_of(rows):
    ro, ids = [0], []
    for r in rows:
        ids.extend(r)
        ro.append(len(ids))
    return ro, ids


def random_world(seed=1, n_filters=40, n_subs=60, max_list=12):
    rng = random.Random(seed)
    filters = [b"t/%03d/+" % i for i in range(n_filters)]
    rng.shuffle(filters)
    lists, opts = [], {}
    upgrade = {s: rng.random() < 0.3 for s in range(n_subs)}
    for i in range(n_filters):
        lst = rng.sample(range(n_subs), rng.choice([0, 1, 2, 3, 5, max_list]))
        lists.append(lst)
        for s in lst:
            if upgrade[s] or rng.random() < 0.7:  # (upgrade_qos rides in the entry's byte: such a session gives entries)
                opts[(i, s)] = subscribe_opts({"qos": rng.randrange(3), "nl": rng.randrange(2),
                                               "rap": rng.randrange(2)})
    return World(filters, lists, opts, upgrade)


def random_window(world, seed, n_rows=80):
    rng = random.Random(seed)
    nf = len(world.filters)
    rows, msgs = [], []
    for _ in range(n_rows):
        rows.append([rng.randrange(nf) for _ in range(rng.choice([0, 1, 1, 2, 4]))])
        frm = None
        if rows[-1] and rng.random() < 0.7:  # often a subscriber of a matched filter: No-Local can hit
            lst = world.lists[world.by_id[rng.choice(rows[-1])]]
            frm = rng.choice(lst) if lst and rng.random() < 0.8 else rng.randrange(60)
        msgs.append({"qos": rng.randrange(3), "retain": rng.random() < 0.5, "retained": rng.random() < 0.3,
                     "from": frm})
    return rows, msgs
