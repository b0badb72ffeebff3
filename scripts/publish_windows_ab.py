#!/usr/bin/env python3
"""Whole publish windows through the combiner against direct calls.

Index and tables as scripts/publish_window_onecall_ab.py: C2's filter set (1M
wildcard filters of the bench generator), one local subscriber per filter, the
shared table by scripts/shared_ab.py's recipe, the dests table by
scripts/forward_ab.py's.  Two identical pairs of tables.  "direct": N caller
threads each call Context.publish_window on one pair (what a node did before
emqx_gm_combiner_publish); "combined": the same N threads call
Combiner.publish_window, at the combiner's defaults, on the other.  Same
process, interleaved round by round.  Callers 1 / 2 / 4 / 8; round robin with 1
caller, hash with 2, 4 and 8, and round robin with 8 (the case the table's
mutex hurts most).  Per cell: --rounds rounds after a warm-up, each timing
--calls windows per thread; the median and min-max of the rounds' median window
latency, topics/s, the mean group size and the device waits per window.

Round robin through the combiner takes effect in the reported (sequence,
position) order, not the direct side's: the two sides' results are compared
for the stateless cells only (tests/test_gpu_publish_windows.py replays the
order).  The measuring step runs in a child process under its own time limit.
One run on one box: quote the figures that way.
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
           "rounds": a.rounds, "calls_per_round_per_thread": a.calls, "combiner": "defaults", "cells": []}
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
        cb = ctx.combiner()

        def combined(w, strategy, hashes, seed):
            return cb.publish_window(index, w, shared=sh[0], strategy=strategy, hashes=hashes, seed=seed, dests=dt[0],
                                     skip_node=0)

        def direct(w, strategy, hashes, seed):
            return ctx.publish_window(index, w, shared=sh[1], strategy=strategy, hashes=hashes, seed=seed, dests=dt[1],
                                      skip_node=0)

        for n in a.windows:
            wins = [host_topics(ctx, codes, a.seed + 1, k * n, n) for k in range(8)]
            hashes = ((np.arange(n, dtype=np.uint64) * 2654435761 + 7) & 0xFFFFFFFF).astype(np.uint32)
            for threads, strategy in a.cells:
                hs = hashes if strategy == "hash" else None
                equal = None
                for k in range(3):  # warm-up, and (one caller: one order) the equality of the two sides
                    got, want = combined(wins[k], strategy, hs, k), direct(wins[k], strategy, hs, k)
                    if strategy == "hash" or threads == 1:
                        equal = same(got, want)
                        if not equal:
                            raise SystemExit(f"{n} topics, {strategy}: the combiner's window != the direct call")
                cell = {"topics": n, "callers": threads, "strategy": strategy, "matched_ids": int(got[0][0][-1]),
                        "hits": got[4]["n_hits"], "pairs": got[4]["n_pairs"], "equal": equal}
                lat = {"combined": [], "direct": []}
                group_sizes, waits = [], []
                for r in range(a.rounds):
                    for side, fn in (("combined", combined), ("direct", direct)):  # interleaved, round by round
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
                        for p in per:
                            for _, st in p:
                                if side == "combined":
                                    g = st["group"]
                                    group_sizes.append(g["n_windows"])
                                    waits.append(g["device_waits"] / g["n_windows"])
                for side in lat:
                    ms = [x["median_ms"] for x in lat[side]]
                    cell[side] = {"window_ms_median": statistics.median(ms), "window_ms_median_min": min(ms),
                                  "window_ms_median_max": max(ms), "window_ms_max": max(x["max_ms"] for x in lat[side]),
                                  "topics_per_s_median": statistics.median(x["topics_per_s"] for x in lat[side])}
                # (per window: a group of g windows is counted g times, each with 1/g of its waits)
                cell["combined"]["mean_group_size"] = sum(group_sizes) / max(1, len(group_sizes))
                cell["combined"]["device_waits_per_window"] = sum(waits) / max(1, len(waits))
                cell["direct_vs_combined_latency"] = cell["direct"]["window_ms_median"] / cell["combined"]["window_ms_median"]
                cell["combined_vs_direct_throughput"] = (cell["combined"]["topics_per_s_median"] /
                                                         cell["direct"]["topics_per_s_median"])
                res["cells"].append(cell)
        res["combiner_stats"] = cb.stats()
        cb.close()
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
    p.add_argument("--cells", nargs="+", default=["1:round_robin", "2:hash", "4:hash", "8:hash", "8:round_robin"],
                   help="callers:strategy")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=40)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_publish_windows", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    a.cells = [(int(c.split(":")[0]), c.split(":")[1]) for c in a.cells]
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--c2-filters={a.c2_filters}", f"--slots={a.slots}", f"--nodes={a.nodes}", f"--rounds={a.rounds}",
           f"--calls={a.calls}", f"--seed={a.seed}", "--windows"] + [str(x) for x in a.windows] + ["--cells"] + \
        [f"{t}:{s}" for t, s in a.cells]
    rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                         "--step", "device", "--part", part] + fwd).returncode
    if rc != 0:
        raise SystemExit(f"the measuring step failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
