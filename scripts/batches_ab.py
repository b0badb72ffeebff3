#!/usr/bin/env python3
"""Session batches: the grouping call against the per-delivery call and the host walk.

Workload: windows of 1,024 and 16,384 generated topics over C2's filter set
with 0-3 subscribers per filter (host rows), every pair with nl = 1 and each
row published by its first subscriber.  After a warm-up the versions alternate
inside one loop; median of --runs with min and max:
  (a) emqx_gm_deliver, FLAG mode, of the same window: the deliveries without
      the grouping, from the same library;
  (b) emqx_gm_deliver_batches in FLAG, DROP and LEAD mode;
  (c) emqx_gm_deliver_batches_host on one thread.
Wall times are around calls that end in a synchronise; the step times are
device events (emqx_gm_batches_last_times: count, expand, partition, heads +
removal + emit, the whole call).  The partition step is every pass's hist,
column, scan and scatter together, so the bytes per second quoted for the
scatter -- 16 B read and written per delivery per pass -- over the partition
step's time is a LOWER bound of the scatter kernel's own.  The device result
must equal the host walk in every mode.

The measuring step runs in a child process under its own time limit.  One run
on one box: quote the figures that way.
"""

import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MODES = ("flag", "drop", "lead")


def stat(xs, scale=1e3):
    xs = [x * scale for x in xs]
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:6], b[:6])) and a[6] == b[6]


def step_device(a):
    from emqx_amd import Context, pack_opt
    from emqx_amd.engine import gen_filter_codes, render_codes
    res = {"box": platform.node(), "runs": a.runs, "windows": {}}
    with Context(0) as ctx:
        codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
        fb, fo = render_codes(codes)
        n = len(fo) - 1
        cnt = (np.arange(n) * 2654435761 >> 7) % 4
        so = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=so[1:])
        si = np.arange(int(so[-1]), dtype=np.uint32)  # (every pair its own subscriber: the default may carry nl)
        idx = ctx.build_index((fb, fo), subs=(so, si))
        table = ctx.build_subopts(idx, [], default=pack_opt(1, nl=1))
        res.update(filters=int(idx.n_filters), pairs=int(so[-1]))
        for nt in a.windows:
            d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed + 1, 0, nt)
            mm = ctx.match_device(idx, d_b, d_o, nt)
            ro, ids = mm.to_host()
            mm.free()
            ctx.dev_free(d_b)
            ctx.dev_free(d_o)
            rows = (ro, ids)
            flags = (np.arange(nt) % 3 | 4).astype(np.uint8)
            d0 = table.deliver(rows, flags, None, False)
            froms = d0.ids[np.minimum(d0.row_off[:-1], max(len(d0.ids) - 1, 0)).astype(np.int64)]
            froms = np.where(d0.row_off[1:] > d0.row_off[:-1], froms, 0xFFFFFFFF).astype(np.uint32)
            for mode in MODES:  # warm-up
                table.deliver_batches(rows, flags, froms, mode)
            table.deliver(rows, flags, froms, False)
            wall = {m: [] for m in MODES}
            steps = {m: [] for m in MODES}
            aw, hw = [], {m: [] for m in MODES}
            got, host = {}, {}
            for _ in range(a.runs):  # the versions alternate
                t0 = time.perf_counter()
                table.deliver(rows, flags, froms, False)
                aw.append(time.perf_counter() - t0)
                for mode in MODES:
                    t0 = time.perf_counter()
                    got[mode] = table.deliver_batches(rows, flags, froms, mode)
                    wall[mode].append(time.perf_counter() - t0)
                    steps[mode].append(table.batches_last_times())
                    t0 = time.perf_counter()
                    host[mode] = table.deliver_batches_host(rows, flags, froms, mode)
                    hw[mode].append(time.perf_counter() - t0)
            for mode in MODES:
                if not same(got[mode], host[mode]):
                    raise SystemExit(f"{nt} topics, {mode}: device batches != host walk")
            total = int(got["flag"].batch_off[-1])
            passes = steps["flag"][-1][5]
            w = {"topics": nt, "matched_ids": int(ro[-1]), "deliveries": total, "batches": int(len(got["flag"].subs)),
                 "radix_passes": passes, "dropped": {m: int(got[m].n_dropped) for m in MODES},
                 "a_deliver_flag_call": stat(aw), "equal_to_host_walk": True}
            for mode in MODES:
                names = ("count", "expand", "partition", "heads_removal_emit", "whole_call_on_stream")
                ev = {k: stat([s[i] for s in steps[mode]], 1.0) for i, k in enumerate(names)}
                part_ms = ev["partition"]["median_ms"]
                w["b_batches_" + mode] = {
                    "call": stat(wall[mode]), "device_steps": ev,
                    "scatter_traffic_bytes": 16 * total * passes,
                    "scatter_traffic_over_partition_step_GBps_lower_bound":
                        (16 * total * passes / (part_ms * 1e-3) / 1e9) if part_ms > 0 else None}
                w["c_batches_host_one_thread_" + mode] = stat(hw[mode])
            res["windows"][str(nt)] = w
        table.release()
        idx.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_batches", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step",
                         "device", "--part", part, f"--c2-filters={a.c2_filters}", f"--runs={a.runs}",
                         f"--seed={a.seed}", "--windows"] + [str(x) for x in a.windows]).returncode
    if rc != 0:
        raise SystemExit(f"the measuring step failed (exit {rc})")
    with open(part) as f:
        res = json.load(f)
    os.remove(part)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
