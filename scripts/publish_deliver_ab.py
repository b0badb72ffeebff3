#!/usr/bin/env python3
"""A publish window with its deliveries' option bytes as ONE call
(emqx_gm_publish_window_deliver) against the two calls it replaces
(emqx_gm_publish_window, then emqx_gm_deliver on the returned host rows).

Index: C2's filter set (1M wildcard filters of the bench generator) with the
option recipe of scripts/subopts_ab.py (0 .. 3 subscribers per filter, every
pair its own subscriber, every pair nl = 1 by the table's default; a row's
publisher is its first subscriber, so No Local hits once per row with a
delivery) and the shared / dests recipes of scripts/publish_window_onecall_ab.py.
Two identical sets of tables; the one call runs on one, the two calls on the
other, in the same process, interleaved round by round after a warm-up that
also compares the two sides array by array.  Per window size, caller count and
mode: --rounds rounds, each timing --calls windows per caller; the median and
min - max of the rounds' median window latency, and the device waits per window
with how often each speculation held.  Round robin with 1 caller (the stateful
case), hash with more (stateless windows overlap).

--unchanged: the paths this feature does not touch -- emqx_gm_publish_window
without options and the direct emqx_gm_deliver -- timed from two builds of the
library (--parent-lib: the parent commit's, loaded through EMQX_GM_LIB; this
tree's), each build in processes of its own, alternating; they must agree within
the runs' own spread.

Every measuring step runs in a child process under its own time limit.  One run
on one box: quote the figures that way.
"""

import argparse
import json
import os
import platform
import random
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def host_topics(ctx, codes, seed, start, n):
    d_b, d_o, tot = ctx.gen_topics_device(codes, seed, start, n)
    tb, to = np.zeros(tot + 64, np.uint8), np.zeros(n + 1, np.uint64)
    ctx.memcpy_d2h(tb, d_b, tot)
    ctx.memcpy_d2h(to, d_o, (n + 1) * 8)
    ctx.dev_free(d_b)
    ctx.dev_free(d_o)
    return tb, to


def world(ctx, a, twins):
    """C2's index with subscriber lists, and `twins` sets of (shared, dests, subopts) tables."""
    from emqx_amd import pack_opt
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
    fb, fo = render_codes(codes)
    n = len(fo) - 1
    cnt = (np.arange(n) * 2654435761 >> 7) % 4
    so = np.zeros(n + 1, np.uint64)
    np.cumsum(cnt, out=so[1:])
    si = np.arange(int(so[-1]), dtype=np.uint32)  # (every pair its own subscriber: the default may carry nl)
    index = ctx.build_index((fb, fo), subs=(so, si))
    stb = host_topics(ctx, codes, a.seed, 0, 16384)
    _, ids = ctx.match(index, stb)
    fids, c = np.unique(ids, return_counts=True)
    top = fids[np.argsort(-c, kind="stable")][:max(1, a.slots * 2 // 3)]
    rng = random.Random(a.seed)
    slots, seen = [], set()
    while len(seen) < min(a.slots, 3 * len(top)):
        f, g = int(rng.choice(top)), rng.randrange(3)
        if (f, g) in seen:
            continue
        seen.add((f, g))
        slots.append((index.filter(f), g, [rng.randrange(1_000_000) for _ in range(rng.choice([1, 2, 3, 5, 8, 16, 64]))]))
    rng = random.Random(a.seed * 100 + a.nodes)
    routes = [(index.filter(int(f)), node) for f in fids if rng.random() < 0.75
              for node in rng.sample(range(a.nodes), min(a.nodes, rng.choice([1, 1, 2, 3])))]
    tabs = [(ctx.build_shared(index, slots), ctx.build_dests(index, routes, a.nodes),
             ctx.build_subopts(index, [], default=pack_opt(1, nl=1))) for _ in range(twins)]
    return codes, index, tabs


def messages(ctx, index, w):
    """The window's flag bytes, and per row its first subscriber as the publisher (none for a row without one)."""
    n = len(w[1]) - 1
    (ro, ids), (fro, fids) = ctx.match_fanout(index, w)
    flags = (np.arange(n) % 3 | 4).astype(np.uint8)
    froms = fids[np.minimum(fro[:-1], max(len(fids), 1) - 1).astype(np.int64)] if len(fids) else np.zeros(n, np.uint32)
    return flags, np.where(fro[1:] > fro[:-1], froms, 0xFFFFFFFF).astype(np.uint32)


def same(a, b):
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        if (x is None) != (y is None) or (x is not None and not all(np.array_equal(p, q) for p, q in zip(x, y))):
            return False
    d, e = a[1], b[1]
    rd = (d.row_dropped is None and e.row_dropped is None) or np.array_equal(d.row_dropped, e.row_dropped)
    return all(np.array_equal(p, q) for p, q in zip(d[:3], e[:3])) and rd and d.n_dropped == e.n_dropped


def timed(threads, calls, fn):
    """`calls` calls of fn(thread, call) on each of `threads` callers: (latencies, results, wall seconds)."""
    per = [[] for _ in range(threads)]

    def run(t):
        for c in range(calls):
            t0 = time.perf_counter()
            out = fn(t, c)
            per[t].append((time.perf_counter() - t0, out))
    ts = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    wall = time.perf_counter() - t0
    return [x for p in per for x, _ in p], [o for p in per for _, o in p], wall


def summary(rounds):
    ms = [x["median_ms"] for x in rounds]
    return {"window_ms_median": statistics.median(ms), "window_ms_median_min": min(ms), "window_ms_median_max": max(ms),
            "window_ms_max": max(x["max_ms"] for x in rounds),
            "topics_per_s_median": statistics.median(x["topics_per_s"] for x in rounds)}


def step_device(a):
    from emqx_amd import Context
    res = {"box": platform.node(), "c2_filters": a.c2_filters, "slots_asked": a.slots, "nodes": a.nodes,
           "rounds": a.rounds, "calls_per_round_per_caller": a.calls, "cells": []}
    with Context(0) as ctx:
        codes, index, tabs = world(ctx, a, 2)
        (sh0, dt0, so0), (sh1, dt1, so1) = tabs

        def one(w, mf, fr, drop, strategy, hashes, seed):
            return ctx.publish_window(index, w, shared=sh0, strategy=strategy, hashes=hashes, seed=seed, dests=dt0,
                                      skip_node=0, subopts=so0, msg_flags=mf, msg_from=fr, drop=drop)

        def two(w, mf, fr, drop, strategy, hashes, seed):
            m, _, picks, plan, st = ctx.publish_window(index, w, shared=sh1, strategy=strategy, hashes=hashes,
                                                       seed=seed, dests=dt1, skip_node=0)
            return m, so1.deliver(m, mf, fr, drop, index=index), picks, plan, st

        for n in a.windows:
            wins = [host_topics(ctx, codes, a.seed + 1, k * n, n) for k in range(8)]
            msgs = [messages(ctx, index, w) for w in wins]
            hashes = ((np.arange(n, dtype=np.uint64) * 2654435761 + 7) & 0xFFFFFFFF).astype(np.uint32)
            for threads in a.threads:
                strategy = "round_robin" if threads == 1 else "hash"
                hs = hashes if strategy == "hash" else None
                for mode in a.modes:
                    drop = mode == "drop"
                    for k in range(4):  # warm-up, and the equality of the two sides
                        got = one(wins[k], *msgs[k], drop, strategy, hs, k)
                        want = two(wins[k], *msgs[k], drop, strategy, hs, k)
                        if not same(got, want):
                            raise SystemExit(f"{n} topics, {strategy}, {mode}: the one call != the two calls")
                    cell = {"topics": n, "callers": threads, "strategy": strategy, "mode": mode,
                            "matched_ids": int(got[0][0][-1]), "deliveries": got[4]["n_deliveries"],
                            "dropped": got[4]["n_dropped"], "hits": got[4]["n_hits"], "pairs": got[4]["n_pairs"],
                            "equal": True}
                    lat = {"one": [], "two": []}
                    waits, calls = [], 0
                    held = {"rows_spec": 0, "picks_spec": 0, "forwards_spec": 0, "deliveries_spec": 0}
                    for r in range(a.rounds):
                        for side, fn in (("one", one), ("two", two)):  # interleaved, round by round
                            def call(t, c, fn=fn, r=r):
                                j = (c + 3 * t) % len(wins)
                                return fn(wins[j], *msgs[j], drop, strategy, hs, 1000 * r + c)[4]
                            xs, sts, wall = timed(threads, a.calls, call)
                            lat[side].append({"median_ms": statistics.median(xs) * 1e3, "max_ms": max(xs) * 1e3,
                                              "topics_per_s": n * len(xs) / wall})
                            if side == "one":
                                for st in sts:
                                    calls += 1
                                    waits.append(st["device_waits"])
                                    for key in held:
                                        held[key] += st[key]
                    for side in lat:
                        cell[side] = summary(lat[side])
                    cell["one"]["device_waits_per_window"] = sum(waits) / max(1, len(waits))
                    cell["one"]["held_share"] = {k: v / max(1, calls) for k, v in held.items()}
                    cell["two_over_one_latency"] = cell["two"]["window_ms_median"] / cell["one"]["window_ms_median"]
                    res["cells"].append(cell)
        for t in tabs:
            for x in t:
                x.release()
        index.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def step_unchanged(a):
    """One build (EMQX_GM_LIB, or this tree's): emqx_gm_publish_window without options and the direct emqx_gm_deliver."""
    from emqx_amd import Context
    res = {"lib": os.environ.get("EMQX_GM_LIB") or "this build", "cells": []}
    with Context(0) as ctx:
        codes, index, tabs = world(ctx, a, 1)
        sh, dt, so = tabs[0]
        for n in a.windows:
            wins = [host_topics(ctx, codes, a.seed + 1, k * n, n) for k in range(8)]
            msgs = [messages(ctx, index, w) for w in wins]
            rows = [ctx.match(index, w) for w in wins]

            def window(t, c):
                return ctx.publish_window(index, wins[c % 8], shared=sh, strategy="round_robin", seed=c, dests=dt,
                                          skip_node=0)[4]

            def deliver(t, c):
                return so.deliver(rows[c % 8], *msgs[c % 8], False, index=index)

            for name, fn in (("publish_window", window), ("deliver", deliver)):
                timed(1, 8, fn)
                rounds = []
                for r in range(a.rounds):
                    xs, _, wall = timed(1, a.calls, fn)
                    rounds.append({"median_ms": statistics.median(xs) * 1e3, "max_ms": max(xs) * 1e3,
                                   "topics_per_s": n * len(xs) / wall})
                res["cells"].append(dict(summary(rounds), topics=n, call=name))
        for x in tabs[0]:
            x.release()
        index.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def child(a, step, part, env=None, extra=()):
    fwd = [f"--c2-filters={a.c2_filters}", f"--slots={a.slots}", f"--nodes={a.nodes}", f"--rounds={a.rounds}",
           f"--calls={a.calls}", f"--seed={a.seed}", "--windows"] + [str(x) for x in a.windows] + ["--threads"] + \
        [str(x) for x in a.threads] + ["--modes"] + list(a.modes)
    rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                         "--step", step, "--part", part] + fwd + list(extra), env=env).returncode
    if rc != 0:
        raise SystemExit(f"the measuring step {step} failed (exit {rc}); stopping")
    with open(part) as f:
        out = json.load(f)
    os.remove(part)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--slots", type=int, default=20000)
    p.add_argument("--nodes", type=int, default=8)
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384])
    p.add_argument("--threads", type=int, nargs="+", default=[1, 8])
    p.add_argument("--modes", nargs="+", default=["flag", "drop"])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=40)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for each measuring step")
    p.add_argument("--unchanged", action="store_true", help="also time the untouched paths from both builds")
    p.add_argument("--parent-lib", default=None, help="the parent commit's libemqx_gpu_match.so")
    p.add_argument("--passes", type=int, default=2, help="processes per build for --unchanged, alternating")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_publish_deliver", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    if a.step == "unchanged":
        return step_unchanged(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    res = child(a, "device", part)
    if a.unchanged:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            raise SystemExit("--unchanged needs --parent-lib (the parent commit's library)")
        runs = {"parent": [], "this": []}
        for k in range(a.passes):  # each build in a process of its own, alternating
            for name in ("parent", "this"):
                env = dict(os.environ)
                env.pop("EMQX_GM_LIB", None)
                if name == "parent":
                    env["EMQX_GM_LIB"] = os.path.abspath(a.parent_lib)
                runs[name].append(child(a, "unchanged", part, env)["cells"])
        table = []
        for i, cell in enumerate(runs["this"][0]):
            row = {"topics": cell["topics"], "call": cell["call"]}
            for name in runs:
                ms = [r[i]["window_ms_median"] for r in runs[name]]
                lo = min(r[i]["window_ms_median_min"] for r in runs[name])
                hi = max(r[i]["window_ms_median_max"] for r in runs[name])
                row[name] = {"ms_median_per_process": ms, "ms_rounds_min": lo, "ms_rounds_max": hi}
            # agreement: the builds' ranges of round medians overlap
            row["agree_within_spread"] = (row["parent"]["ms_rounds_min"] <= row["this"]["ms_rounds_max"] and
                                          row["this"]["ms_rounds_min"] <= row["parent"]["ms_rounds_max"])
            table.append(row)
        res["unchanged_paths"] = table
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
