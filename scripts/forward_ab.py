#!/usr/bin/env python3
"""Forward plan: device call, its passes and the host-walk comparison.

Index: C2's filter set (1M wildcard filters of the bench generator).  About 3/4
of the filters that a sample window (--sample topics) hits get node routes, one
to three nodes each, over 8 and over 64 nodes.  Windows of 1,024, 16K and 1M
generated topics are matched once on the device; per node count and window the
script reports the device-row plan (median of --runs after a warm-up, wall time
around a call that ends in a synchronise), its passes from
emqx_gm_dests_last_times (device events), the host-row plan (rows and result
cross PCIe), and emqx_gm_forward_plan_host on one thread over a host-only twin
of the table: the baseline.  The reference's own path (lookup_routes/1 and
forward/3 per route in Erlang) cannot be run here.  The device plan and the
host walk must be equal.

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


def med(xs):
    return statistics.median(xs)


def step_device(a):
    from emqx_amd import Context, DestTable
    from emqx_amd.engine import gen_filter_codes, render_codes
    res = {"box": platform.node(), "c2_filters": a.c2_filters, "sample_topics": a.sample, "runs": a.runs, "nodes": {}}
    codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
    fb, fo = render_codes(codes)
    with Context(0) as ctx:
        index = ctx.build_index((fb, fo))
        d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed, 0, a.sample)
        m = ctx.match_device(index, d_b, d_o, a.sample)
        _, ids = m.to_host()
        m.free()
        ctx.dev_free(d_b)
        ctx.dev_free(d_o)
        hit = np.unique(ids)
        res["sample_filters_hit"] = int(len(hit))
        windows = {}
        for n in a.windows:  # matched once, shared by the node counts
            d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed + 1, 0, n)
            rows = ctx.match_device(index, d_b, d_o, n)
            ctx.dev_free(d_b)
            ctx.dev_free(d_o)
            windows[n] = (rows, rows.to_host())
        for n_nodes in a.nodes:
            rng = random.Random(a.seed * 100 + n_nodes)
            routed = [int(f) for f in hit if rng.random() < 0.75]
            routes = [(index.filter(f), node) for f in routed
                      for node in rng.sample(range(n_nodes), min(n_nodes, rng.choice([1, 1, 2, 3])))]
            table = ctx.build_dests(index, routes, n_nodes)
            twin = DestTable.compile_host((fb, fo), routes, n_nodes)
            info = table.info()
            out = {"table": {k: int(getattr(info, k)) for k, _ in info._fields_ if k != "reserved0"}, "windows": {}}
            for n in a.windows:
                rows, (ro, ids) = windows[n]

                def dev_call():
                    t0 = time.perf_counter()
                    fw = table.plan_device(rows, 0)  # (returns after the call's last synchronise)
                    dt = time.perf_counter() - t0
                    pairs = fw.n_pairs
                    fw.free()
                    return dt, pairs, table.last_times()
                dev_call()  # warm-up
                wall, passes = [], []
                for _ in range(a.runs):
                    dt, pairs, ms = dev_call()
                    wall.append(dt)
                    passes.append(ms)
                table.plan((ro, ids), 0)
                hwall = []
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    got = table.plan((ro, ids), 0)
                    hwall.append(time.perf_counter() - t0)
                twin.plan_host((ro, ids), 0)
                cwall = []
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    want = twin.plan_host((ro, ids), 0)
                    cwall.append(time.perf_counter() - t0)
                if not all(np.array_equal(x, y) for x, y in zip(got, want)):
                    raise SystemExit(f"{n_nodes} nodes, {n} topics: device plan != host-walk plan")
                out["windows"][str(n)] = {
                    "topics": n, "matched_ids": int(ro[-1]), "forwards": int(pairs),
                    "device_rows_call_ms_median": med(wall) * 1e3, "device_rows_call_ms_min": min(wall) * 1e3,
                    "device_rows_call_ms_max": max(wall) * 1e3,
                    "enumerate_ms": med(p[0] for p in passes), "expand_ms": med(p[1] for p in passes),
                    "partition_ms": med(p[2] for p in passes), "stream_ms": med(p[3] for p in passes),
                    "host_rows_call_ms_median": med(hwall) * 1e3,
                    "plan_host_one_thread_ms_median": med(cwall) * 1e3,
                    "plan_host_one_thread_ms_min": min(cwall) * 1e3,
                    "device_rows_vs_plan_host": med(cwall) / med(wall),
                    "host_rows_vs_plan_host": med(cwall) / med(hwall),
                    "equal_to_host_walk": True,
                }
                del got, want
            table.release()
            twin.release()
            res["nodes"][str(n_nodes)] = out
        for rows, _ in windows.values():
            rows.free()
        index.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--sample", type=int, default=1_000_000)
    p.add_argument("--nodes", type=int, nargs="+", default=[8, 64])
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384, 1_000_000])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_forward", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--c2-filters={a.c2_filters}", f"--sample={a.sample}", f"--runs={a.runs}", f"--seed={a.seed}", "--nodes"] + \
        [str(x) for x in a.nodes] + ["--windows"] + [str(x) for x in a.windows]
    for step, limit in (("device", a.limit),):
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                             "--step", step, "--part", part] + fwd).returncode
        if rc != 0:
            raise SystemExit(f"step {step} failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
