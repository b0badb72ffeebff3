#!/usr/bin/env python3
"""Shared-subscription pick: device call, its passes and the host-walk comparison.

Index: C2's filter set (1M wildcard filters of the bench generator).  A few
thousand slots ({filter, group} pairs, 1..64 members) are laid over the filters
that a 16K-topic sample hits most, so the windows carry shared hits.  Windows of
1,024, 16K and 1M generated topics are matched once on the device; per window
and strategy the script reports the device-row pick (median of --runs after a
warm-up, wall and stream time), its passes from emqx_gm_shared_last_times, the
host-row pick (rows and results cross PCIe), and emqx_gm_shared_pick_host on one
thread over a host-only twin of the table.  For the 1,024-topic window it also
times emqx_gm_match_fanout alone in the same run: the scale a pick sits beside.
The device picks and the host walk must be equal.

Each step runs in a child process under its own time limit; the first failure
stops the script.  One run on one box: quote the figures that way.
"""

import argparse
import json
import os
import platform
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STRATEGIES = ["hash", "round_robin", "sticky", "random"]


def med(xs):
    return statistics.median(xs)


def step_device(a):
    from emqx_amd import Context, SharedTable
    from emqx_amd.engine import gen_filter_codes, render_codes
    res = {"box": platform.node(), "c2_filters": a.c2_filters, "slots_asked": a.slots, "runs": a.runs, "windows": {}}
    codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
    fb, fo = render_codes(codes)
    with Context(0) as ctx:
        index = ctx.build_index((fb, fo))
        # the filters a 16K sample hits most carry the slots
        d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed, 0, 16384)
        m = ctx.match_device(index, d_b, d_o, 16384)
        _, ids = m.to_host()
        m.free()
        ctx.dev_free(d_b)
        ctx.dev_free(d_o)
        fids, cnt = np.unique(ids, return_counts=True)
        top = fids[np.argsort(-cnt, kind="stable")][:max(1, a.slots * 2 // 3)]
        rng = random.Random(a.seed)
        slots, seen = [], set()
        while len(seen) < min(a.slots, 3 * len(top)):
            f, g = int(rng.choice(top)), rng.randrange(3)
            if (f, g) in seen:
                continue
            seen.add((f, g))
            c = rng.choice([1, 2, 3, 5, 8, 16, 64])
            slots.append((index.filter(f), g, [rng.randrange(1_000_000) for _ in range(c)]))
        table = ctx.build_shared(index, slots)
        twin = SharedTable.compile_host((fb, fo), slots)
        info = table.info()
        res["table"] = {k: int(getattr(info, k)) for k, _ in info._fields_}
        for n in a.windows:
            d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed + 1, 0, n)
            rows = ctx.match_device(index, d_b, d_o, n)
            ro, ids = rows.to_host()
            hashes = ((np.arange(n, dtype=np.uint64) * 2654435761 + 7) & 0xFFFFFFFF).astype(np.uint32)
            d_h = ctx.dev_alloc(hashes.nbytes)
            ctx.memcpy_h2d(d_h, hashes, hashes.nbytes)
            w = {"topics": n, "matched_ids": int(ro[-1])}
            for strategy in STRATEGIES:
                hs = hashes if strategy == "hash" else None

                def dev_call(seed):
                    t0 = time.perf_counter()
                    om, os_ = table.pick_device(rows, strategy, d_h if strategy == "hash" else None, seed)
                    dt = time.perf_counter() - t0
                    hits = om.nnz
                    om.free()
                    os_.free()
                    return dt, hits, table.last_times()
                dev_call(1)  # warm-up
                wall, passes = [], []
                for k in range(a.runs):
                    dt, hits, ms = dev_call(2 + k)
                    wall.append(dt)
                    passes.append(ms)
                hwall = []
                table.pick((ro, ids), strategy, hs, 1)
                for k in range(a.runs):
                    t0 = time.perf_counter()
                    got = table.pick((ro, ids), strategy, hs, 100 + k)
                    hwall.append(time.perf_counter() - t0)
                # the host walk, one thread; it and a device pick on fresh, equal state must agree
                cwall = []
                for k in range(a.runs):
                    t0 = time.perf_counter()
                    twin.pick_host((ro, ids), strategy, hs, 100 + k)
                    cwall.append(time.perf_counter() - t0)
                t2 = ctx.build_shared(index, slots)
                w2 = SharedTable.compile_host((fb, fo), slots)
                a_dev, a_host = t2.pick((ro, ids), strategy, hs, 9), w2.pick_host((ro, ids), strategy, hs, 9)
                if not all(np.array_equal(x, y) for x, y in zip(a_dev, a_host)):
                    raise SystemExit(f"{n} topics, {strategy}: device picks != host-walk picks")
                t2.release()
                w2.release()
                w[strategy] = {
                    "hits": int(hits),
                    "device_rows_call_ms_median": med(wall) * 1e3, "device_rows_call_ms_min": min(wall) * 1e3,
                    "enumerate_ms": med(p[0] for p in passes), "expand_ms": med(p[1] for p in passes),
                    "round_robin_passes_ms": med(p[2] for p in passes), "stream_ms": med(p[3] for p in passes),
                    "host_rows_call_ms_median": med(hwall) * 1e3,
                    "pick_host_one_thread_ms_median": med(cwall) * 1e3,
                    "device_rows_vs_pick_host": med(cwall) / med(wall),
                    "host_rows_vs_pick_host": med(cwall) / med(hwall),
                    "equal_to_host_walk": True,
                }
                del got
            if n == a.windows[0]:
                # the window's emqx_gm_match_fanout alone, host buffers, same run
                tb = np.zeros(1, np.uint8)
                tot = np.zeros(n + 1, np.uint64)
                ctx.memcpy_d2h(tot, d_o, (n + 1) * 8)
                tb = np.zeros(int(tot[-1]) + 64, np.uint8)
                ctx.memcpy_d2h(tb, d_b, int(tot[-1]))
                ctx.match_fanout(index, (tb, tot))
                mf = []
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    ctx.match_fanout(index, (tb, tot))
                    mf.append(time.perf_counter() - t0)
                w["match_fanout_call_ms_median"] = med(mf) * 1e3
            rows.free()
            ctx.dev_free(d_h)
            ctx.dev_free(d_b)
            ctx.dev_free(d_o)
            res["windows"][str(n)] = w
        table.release()
        twin.release()
        index.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--slots", type=int, default=4000)
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384, 1_000_000])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_shared", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--c2-filters={a.c2_filters}", f"--slots={a.slots}", f"--runs={a.runs}", f"--seed={a.seed}", "--windows"] + \
        [str(x) for x in a.windows]
    for step, limit in (("device", a.limit),):
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                             "--step", step, "--part", part] + fwd).returncode
        if rc != 0:
            raise SystemExit(f"step {step} failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
