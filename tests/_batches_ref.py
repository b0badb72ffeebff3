"""Plain-Python restatement of the session batches over ``_subopts_ref.World``:
what each subscriber's channel gets when a whole publish window reaches its
mailbox before it drains it.

  emqx_broker:dispatch/2        one send per (filter, subscriber), in window order
  emqx_misc:drain_deliver/1     apps/emqx/src/emqx_misc.erl:159-173: the mailbox as one list
  emqx_channel:handle_deliver/2 emqx_channel.erl:830-842: ignore_local, then enrich each
  emqx_session:ignore_local/4   emqx_session.erl:279-291 (lists:dropwhile)

``batches(world, rows, msgs, mode)`` returns [(subscriber, [(row, filter id,
delivery byte)], removed)] by ascending subscriber: the shape of
``SessionBatches.as_lists()``."""

from tests import _subopts_ref as R

FLAG, DROP, LEAD = "flag", "drop", "lead"


def mailboxes(world, rows, msgs):
    """Dispatch the window in order: {subscriber: [(row, filter id, ("deliver", topic, msg))]}."""
    boxes = {}
    for r, (row, m) in enumerate(zip(rows, msgs)):
        for fid in row:
            i = world.by_id[fid]
            d = ("deliver", world.filters[i], dict(m, nl=False))
            for s in world.lists[i]:
                boxes.setdefault(s, []).append((r, fid, d))
    return boxes


def batches(world, rows, msgs, mode):
    out = []
    for s, box in sorted(mailboxes(world, rows, msgs).items()):
        sess = world.session(s)
        delivers = [d for _, _, d in box]
        if mode == LEAD:  # the reference's own path over the drained list
            kept = R.session_deliver(delivers, s, sess)
            gone = len(box) - len(kept)
            entries = [(r, fid, R.dopt_byte(m)) for (r, fid, _), m in zip(box[gone:], kept)]
        else:
            entries, gone = [], 0
            for r, fid, d in box:
                hit = d[2]["from"] is not None and R.ignore_local_fun(sess["subscriptions"], s, d)
                if hit and mode == DROP:
                    gone += 1
                    continue
                entries.append((r, fid, R.dopt_byte(R.enrich_deliver(d, sess), hit)))
        out.append((s, entries, gone))
    return out


def census(world, rows, msgs):
    """(batches with a leading run, batches with a hit dropwhile keeps, batches LEAD empties)."""
    led = mid = emptied = 0
    for s, box in mailboxes(world, rows, msgs).items():
        subs = world.session(s)["subscriptions"]
        hits = [d[2]["from"] is not None and R.ignore_local_fun(subs, s, d) for _, _, d in box]
        lead = 0
        while lead < len(hits) and hits[lead]:
            lead += 1
        led += lead > 0
        mid += any(hits[lead:])
        emptied += lead == len(hits)
    return led, mid, emptied


def map_world(world, fn):
    """The same world with every subscriber id s replaced by fn(s) (fn injective)."""
    lists = [[fn(s) for s in lst] for lst in world.lists]
    opts = {(i, fn(s)): o for (i, s), o in world.opts.items()}
    listed = {s for lst in world.lists for s in lst}  # (a session that subscribes to nothing gets no delivery)
    upgrade = {fn(s): u for s, u in world.upgrade.items() if s in listed}
    return R.World(list(world.filters), lists, opts, upgrade, dict(world.default))


def map_msgs(msgs, fn):
    return [dict(m, **{"from": None if m["from"] is None else fn(m["from"])}) for m in msgs]
