#!/usr/bin/env python3
"""A publish window as ONE call against the three calls it replaces.

Index: C2's filter set (1M wildcard filters of the bench generator), one local
subscriber per filter.  The shared table follows scripts/shared_ab.py's recipe
(the filters a 16K sample hits most carry --slots slots of 1 .. 64 members), the
dests table scripts/forward_ab.py's (3/4 of the filters the sample hits get one
to three of --nodes nodes).  Two identical pairs of tables: emqx_gm_publish_window
runs on one, emqx_gm_match_fanout + emqx_gm_shared_pick + emqx_gm_forward_plan on
the other, in the same process, interleaved round by round; strategy round_robin
with 1 caller thread (the stateful case), hash with --threads callers (stateless
windows overlap).  Per window size and thread count: --rounds rounds after a
warm-up, each timing --calls windows per thread; median and spread of the
rounds' median window latency, the largest single window, topics/s, the waits
per window and how often each speculation held.  The first round's results are
compared array by array.

The measuring step runs in a child process under its own time limit.  One run
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


def same(a, b):
    for x, y in zip(a[:4], b[:4]):
        if (x is None) != (y is None) or (x is not None and not all(np.array_equal(p, q) for p, q in zip(x, y))):
            return False
    return True


def step_device(a):
    from emqx_amd import Context
    from emqx_amd.engine import gen_filter_codes, render_codes
    res = {"box": platform.node(), "c2_filters": a.c2_filters, "slots_asked": a.slots, "nodes": a.nodes,
           "rounds": a.rounds, "calls_per_round_per_thread": a.calls, "cells": []}
    codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
    fb, fo = render_codes(codes)
    with Context(0) as ctx:
        index = ctx.build_index((fb, fo), subs=[[i] for i in range(a.c2_filters)])
        stb = host_topics(ctx, codes, a.seed, 0, 16384)
        _, ids = ctx.match(index, stb)
        fids, cnt = np.unique(ids, return_counts=True)
        top = fids[np.argsort(-cnt, kind="stable")][:max(1, a.slots * 2 // 3)]
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
        sh = [ctx.build_shared(index, slots) for _ in range(2)]
        dt = [ctx.build_dests(index, routes, a.nodes) for _ in range(2)]
        res["shared_table"] = {k: int(getattr(sh[0].info(), k)) for k, _ in sh[0].info()._fields_}
        res["dests_routes"] = int(dt[0].info().n_routes)

        def one(w, strategy, hashes, seed):
            return ctx.publish_window(index, w, shared=sh[0], strategy=strategy, hashes=hashes, seed=seed, dests=dt[0],
                                      skip_node=0)

        def three(w, strategy, hashes, seed):
            m, d = ctx.match_fanout(index, w)
            return m, d, sh[1].pick(m, strategy, hashes, seed), dt[1].plan(m, 0), None

        for n in a.windows:
            wins = [host_topics(ctx, codes, a.seed + 1, k * n, n) for k in range(8)]
            hashes = ((np.arange(n, dtype=np.uint64) * 2654435761 + 7) & 0xFFFFFFFF).astype(np.uint32)
            for threads in a.threads:
                strategy = "round_robin" if threads == 1 else "hash"
                hs = hashes if strategy == "hash" else None
                for k in range(3):  # warm-up, and the equality of the two sides
                    got, want = one(wins[k], strategy, hs, k), three(wins[k], strategy, hs, k)
                    if not same(got, want):
                        raise SystemExit(f"{n} topics, {strategy}: the one call != the three calls")
                cell = {"topics": n, "threads": threads, "strategy": strategy, "matched_ids": int(got[0][0][-1]),
                        "hits": got[4]["n_hits"], "pairs": got[4]["n_pairs"], "equal": True}
                lat = {"one": [], "three": []}
                waits, held = [], {"rows_spec": 0, "fanout_spec": 0, "picks_spec": 0, "forwards_spec": 0}
                calls = 0
                for r in range(a.rounds):
                    for side, fn in (("one", one), ("three", three)):  # interleaved, round by round
                        per = [[] for _ in range(threads)]

                        def run(t):
                            for c in range(a.calls):
                                w = wins[(c + 3 * t) % len(wins)]
                                t0 = time.perf_counter()
                                out = fn(w, strategy, hs, 1000 * r + c)
                                per[t].append((time.perf_counter() - t0, out[4]))
                        ts = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
                        t0 = time.perf_counter()
                        for t in ts:
                            t.start()
                        for t in ts:
                            t.join()
                        wall = time.perf_counter() - t0
                        xs = [x for p in per for x, _ in p]
                        lat[side].append({"median_ms": statistics.median(xs) * 1e3, "max_ms": max(xs) * 1e3,
                                          "topics_per_s": n * len(xs) / wall})
                        if side == "one":
                            for p in per:
                                for _, st in p:
                                    calls += 1
                                    waits.append(st["device_waits"])
                                    for key in held:
                                        held[key] += st[key]
                for side in lat:
                    ms = [x["median_ms"] for x in lat[side]]
                    cell[side] = {"window_ms_median": statistics.median(ms), "window_ms_median_min": min(ms),
                                  "window_ms_median_max": max(ms), "window_ms_max": max(x["max_ms"] for x in lat[side]),
                                  "topics_per_s_median": statistics.median(x["topics_per_s"] for x in lat[side])}
                cell["one"]["device_waits_per_window"] = sum(waits) / max(1, len(waits))
                cell["one"]["held_share"] = {k: v / max(1, calls) for k, v in held.items()}
                cell["one_vs_three_latency"] = cell["three"]["window_ms_median"] / cell["one"]["window_ms_median"]
                res["cells"].append(cell)
        for t in sh + dt:
            t.release()
        index.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--slots", type=int, default=20000)
    p.add_argument("--nodes", type=int, default=8)
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384])
    p.add_argument("--threads", type=int, nargs="+", default=[1, 8])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=40)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_publish_window", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--c2-filters={a.c2_filters}", f"--slots={a.slots}", f"--nodes={a.nodes}", f"--rounds={a.rounds}",
           f"--calls={a.calls}", f"--seed={a.seed}", "--windows"] + [str(x) for x in a.windows] + ["--threads"] + \
        [str(x) for x in a.threads]
    rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                         "--step", "device", "--part", part] + fwd).returncode
    if rc != 0:
        raise SystemExit(f"the measuring step failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
