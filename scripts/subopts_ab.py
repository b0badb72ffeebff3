#!/usr/bin/env python3
"""Subscription options at dispatch: the deliver call against the plain fan-out.

Workloads: the C4 shape (1,000 rows x 1M subscribers, rows in HBM) and windows
of 1,024 and 16,384 generated topics over C2's filter set with 0-3 subscribers
per filter (host rows).  Versions, alternated inside one loop after a warm-up,
median of --runs with min and max:
  (a) emqx_gm_fanout of the same rows: the yardstick (also timed with the
      library given by --parent-lib, when it exists, in a child process of the
      same run: the unchanged path against the parent build);
  (b) emqx_gm_deliver, FLAG mode;
  (c) emqx_gm_deliver, DROP mode, every row's publisher subscribed under nl;
  (d) emqx_gm_deliver_host on one thread over the same table (C4: over the
      first --host-rows rows only; the figure names the rows it covered).
Wall times are around calls that end in a synchronise; the kernel times are
device events (the fan-out's copy kernel from the call's stats, the deliver
call's from emqx_gm_subopts_last_times).  FLAG deliveries must equal the
fan-out's and the host walk must equal the device.

Each step runs in a child process under its own time limit; the first failure
stops the script.  One run on one box: quote the figures that way.
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


def stat(xs):
    xs = [x * 1e3 for x in xs]
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def stat_ms(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def c4_world(ctx):
    K, S = 1000, 1_000_000
    filters = [b"hot/#", b"hot/+/x/#"] + [b"hot/%d/x/y/z" % k for k in range(K)]
    lists = [np.arange(0, 600_000), np.arange(600_000, 999_900)] + [np.arange(999_900, S)] * K
    so = np.zeros(len(lists) + 1, np.uint64)
    so[1:] = np.cumsum([len(x) for x in lists])
    si = np.concatenate(lists).astype(np.uint32)
    idx = ctx.build_index(filters, subs=(so, si))
    from emqx_amd.engine import pack
    tb, to = pack([b"hot/%d/x/y/z" % k for k in range(K)])
    d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
    ctx.memcpy_h2d(d_tb, tb, len(tb))
    ctx.memcpy_h2d(d_to, to, len(to) * 8)
    m = ctx.match_device(idx, d_tb, d_to, K, exact=True)
    ctx.dev_free(d_tb)
    ctx.dev_free(d_to)
    return idx, m, K


def step_fanout_only(a):
    """(a) alone, with whatever library EMQX_GM_LIB names: the parent build's time of the unchanged path."""
    from emqx_amd import Context
    res = {}
    with Context(0) as ctx:
        idx, m, K = c4_world(ctx)
        for _ in range(2):
            ctx.fanout_device(idx, m).free()
        wall, kern = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = ctx.fanout_device(idx, m)
            wall.append(time.perf_counter() - t0)
            kern.append(ctx.stats()["match_kernel_ms"])
            r.free()
        res["c4"] = {"fanout_call": stat(wall), "k_fanout_copy": stat_ms(kern)}
        m.free()
        idx.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def step_device(a):
    from emqx_amd import Context, pack_opt
    from emqx_amd.engine import gen_filter_codes, render_codes
    res = {"box": platform.node(), "runs": a.runs}
    with Context(0) as ctx:
        # ---- C4, rows in HBM
        idx, m, K = c4_world(ctx)
        pubs = [(k * 599) % 600_000 for k in range(K)]  # row k's publisher: a subscriber of hot/#
        entries = [(b"hot/#", s, pack_opt(1, nl=1)) for s in sorted(set(pubs))]
        entries += [(b"hot/+/x/#", 600_000 + 7 * k, pack_opt(2, rap=1, upgrade_qos=True)) for k in range(50_000)]
        table = ctx.build_subopts(idx, entries, default=pack_opt(1))
        flags = (np.arange(K) % 3 | 4).astype(np.uint8)
        froms = np.array(pubs, np.uint32)
        d_f, d_fr = ctx.dev_alloc(K), ctx.dev_alloc(K * 4)
        ctx.memcpy_h2d(d_f, flags, K)
        ctx.memcpy_h2d(d_fr, froms, K * 4)

        def fan():
            t0 = time.perf_counter()
            r = ctx.fanout_device(idx, m)
            dt = time.perf_counter() - t0
            k = ctx.stats()["match_kernel_ms"]
            n = r.nnz
            r.free()
            return dt, k, n

        def deliver(drop):
            t0 = time.perf_counter()
            d = table.deliver_device(m, d_f, d_fr, drop)
            dt = time.perf_counter() - t0
            ms = table.last_times()
            n, nd = d.nnz, int(d.d.n_dropped)
            d.free()
            return dt, ms, n, nd
        fan(), deliver(False), deliver(True)  # warm-up
        fw, fk, bw, bk, bs, cw, ck, cs = [], [], [], [], [], [], [], []
        for _ in range(a.runs):  # the versions alternate
            dt, k, n_fan = fan()
            fw.append(dt), fk.append(k)
            dt, ms, n_flag, _ = deliver(False)
            bw.append(dt), bk.append(ms[1]), bs.append(ms[0])
            dt, ms, n_drop, nd = deliver(True)
            cw.append(dt), ck.append(ms[1]), cs.append(ms[0])
        if n_flag != n_fan or n_drop + nd != n_fan or nd != K:
            raise SystemExit(f"C4: deliveries fan-out {n_fan}, FLAG {n_flag}, DROP {n_drop} + {nd}")
        # (d) the host walk over the first rows, and its equality with the device on them
        ro, ids = m.to_host()
        hr = a.host_rows
        sub = (ro[:hr + 1], ids[:int(ro[hr])])
        t0 = time.perf_counter()
        host = table.deliver_host(sub, flags[:hr], froms[:hr], True)
        hwall = time.perf_counter() - t0
        dev = table.deliver(sub, flags[:hr], froms[:hr], True)
        if not all(np.array_equal(x, y) for x, y in zip(host[:4], dev[:4])):
            raise SystemExit("C4: device deliveries != host walk")
        n_host = len(host.ids)
        del host, dev
        res["c4"] = {
            "rows": K, "deliveries": int(n_fan), "dropped_in_drop_mode": int(nd),
            "a_fanout_call": stat(fw), "a_k_fanout_copy": stat_ms(fk),
            "b_flag_call": stat(bw), "b_k_so_copy": stat_ms(bk), "b_lengths_scan": stat_ms(bs),
            "c_drop_call": stat(cw), "c_k_so_copy": stat_ms(ck), "c_lengths_scan": stat_ms(cs),
            "k_so_copy_over_k_fanout_copy_flag": statistics.median(bk) / statistics.median(fk),
            "k_so_copy_over_k_fanout_copy_drop": statistics.median(ck) / statistics.median(fk),
            "d_deliver_host_one_thread": {"rows": hr, "deliveries": int(n_host), "ms": hwall * 1e3},
        }
        ctx.dev_free(d_f)
        ctx.dev_free(d_fr)
        table.release()
        m.free()
        idx.release()
        ctx.pool_trim()
        if a.c4_only:  # (a profiler run of the C4 kernels alone)
            with open(a.part, "w") as f:
                json.dump(res, f, indent=1)
            return
        # ---- C2's filters, host rows
        codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
        fb, fo = render_codes(codes)
        n = len(fo) - 1
        cnt = (np.arange(n) * 2654435761 >> 7) % 4
        so = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=so[1:])
        si = np.arange(int(so[-1]), dtype=np.uint32)  # (every pair its own subscriber: the default may carry nl)
        idx = ctx.build_index((fb, fo), subs=(so, si))
        table = ctx.build_subopts(idx, [], default=pack_opt(1, nl=1))
        res["c2"] = {"filters": int(idx.n_filters), "pairs": int(so[-1]), "windows": {}}
        for nt in a.windows:
            d_b, d_o, _ = ctx.gen_topics_device(codes, a.seed + 1, 0, nt)
            mm = ctx.match_device(idx, d_b, d_o, nt)
            ro, ids = mm.to_host()
            mm.free()
            ctx.dev_free(d_b)
            ctx.dev_free(d_o)
            fro, fids = ctx.fanout(idx, ro, ids)
            flags = (np.arange(nt) % 3 | 4).astype(np.uint8)
            froms = fids[np.minimum(fro[:-1], len(fids) - 1).astype(np.int64)]  # the row's first subscriber
            froms = np.where(fro[1:] > fro[:-1], froms, 0xFFFFFFFF).astype(np.uint32)
            table.deliver((ro, ids), flags, froms, False), table.deliver((ro, ids), flags, froms, True)
            table.deliver_host((ro, ids), flags, froms, True)
            fw, bw, cw, dw = [], [], [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                ctx.fanout(idx, ro, ids)
                fw.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                flag = table.deliver((ro, ids), flags, froms, False)
                bw.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                drop = table.deliver((ro, ids), flags, froms, True)
                cw.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                host = table.deliver_host((ro, ids), flags, froms, True)
                dw.append(time.perf_counter() - t0)
            if flag.ids.tobytes() != fids.tobytes() or flag.row_off.tobytes() != fro.tobytes():
                raise SystemExit(f"{nt} topics: FLAG deliveries != fan-out")
            if not all(np.array_equal(x, y) for x, y in zip(drop[:4], host[:4])):
                raise SystemExit(f"{nt} topics: device deliveries != host walk")
            res["c2"]["windows"][str(nt)] = {
                "topics": nt, "matched_ids": int(ro[-1]), "deliveries": int(len(fids)), "dropped": int(drop.n_dropped),
                "a_fanout_call": stat(fw), "b_flag_call": stat(bw), "c_drop_call": stat(cw),
                "d_deliver_host_one_thread": stat(dw), "equal_to_fanout_and_host_walk": True}
        table.release()
        idx.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--windows", type=int, nargs="+", default=[1024, 16384])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--host-rows", type=int, default=20)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for each measuring step")
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "emqx_amd", "libemqx_gpu_match_parent.so"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_subopts", "ab.json"))
    p.add_argument("--c4-only", action="store_true", help="step device: stop after C4 (for a kernel trace)")
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    if a.step == "fanout":
        return step_fanout_only(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    fwd = [f"--c2-filters={a.c2_filters}", f"--runs={a.runs}", f"--seed={a.seed}", f"--host-rows={a.host_rows}",
           "--windows"] + [str(x) for x in a.windows]
    steps = [("device", {}, "device")]
    if os.path.exists(a.parent_lib):  # the unchanged fan-out, parent build then this build, back to back
        steps += [("fanout", {"EMQX_GM_LIB": a.parent_lib}, "fanout_parent_build"), ("fanout", {}, "fanout_this_build")]
    out = {}
    for step, env, name in steps:
        part = a.out + "." + name + ".part"
        rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                             "--step", step, "--part", part] + fwd, env=dict(os.environ, **env)).returncode
        if rc != 0:
            raise SystemExit(f"step {name} failed (exit {rc}); stopping")
        with open(part) as f:
            out[name] = json.load(f)
        os.remove(part)
    res = out.pop("device")
    res.update(out)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
