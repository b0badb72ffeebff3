#!/usr/bin/env python3
"""Retained-message lookup: build time, device rate and CPU comparison figures.

Table: 1M retained topics from the bench's topic generator over C2's filter
codes (duplicates collapse).  Filter batches of 100k: (a) the C2 wildcard
filters; (b) literal-heavy ones: a stored topic with one word replaced by '+'.
Reports the build time, filters/s and returned ids/s of the host-to-host
device call (median of --runs after a warm-up), its two walk passes and the
scan timed apart with HIP events, and for 1,000 filters of each batch the
single-thread walk over the host copy of the same tables
(emqx_gm_retained_match_host) and a linear scan of the table per filter -- the
reference's algorithm (emqx_retainer_mnesia:match_messages/1 is a select over
the whole table) -- as a vectorised numpy pass over the topics' word codes.
The device rows and the host-walk rows must be equal on that sample, and the
scan's row lengths too.

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


def workload(a):
    from emqx_amd.engine import gen_filter_codes, render_codes
    from oracle import oracle as orc
    codes = gen_filter_codes(a.seed, a.c2_filters, wildcard_only=True)
    tcodes = orc.gen_topic_codes(a.seed, 0, a.topics, codes)
    topics = orc.render_codes(tcodes)
    fa = codes[:a.filters]
    # (b): stored topics with one present word replaced by '+'
    rng = np.random.default_rng(a.seed)
    fbc = tcodes[rng.integers(0, len(tcodes), a.filters)].copy()
    depth = (fbc != -3).sum(axis=1)
    lvl = (rng.random(a.filters) * depth).astype(np.int64)
    fbc[np.arange(a.filters), lvl] = -1
    return tcodes, topics, {"c2_wildcard": (fa, render_codes(fa)), "literal_heavy": (fbc, render_codes(fbc))}


def scan_counts(tuniq, fcodes):
    """Row lengths by a linear scan of the table per filter, on word codes
    (words of one level are equal iff their codes are)."""
    out = []
    for f in fcodes:
        m = np.ones(len(tuniq), bool)
        for l, c in enumerate(f):
            if c == -2:
                break
            if c == -1:
                m &= tuniq[:, l] != -3
            else:
                m &= tuniq[:, l] == c
        out.append(int(m.sum()))
    return out


def step_device(a):
    from emqx_amd import Context
    res = {"box": platform.node(), "topics_generated": a.topics, "filters_per_batch": a.filters, "runs": a.runs}
    tcodes, topics, batches = workload(a)
    with Context(0) as ctx:
        t0 = time.perf_counter()
        ix = ctx.build_retained(topics)
        res["build_s"] = time.perf_counter() - t0
        info = ix.info()
        res["index"] = {k: int(getattr(info, k)) for k, _ in info._fields_}
        for name, (fc, fp) in batches.items():
            ix.match(fp)  # warm-up
            wall, passes = [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                ro, ids, ms = ix.match_timed(fp)
                wall.append(time.perf_counter() - t0)
                passes.append(ms)
            w = statistics.median(wall)
            nnz = int(ro[-1])
            med = [statistics.median(p[k] for p in passes) for k in range(3)]
            r = {"call_s_median": w, "call_s_min": min(wall), "filters_per_s": a.filters / w, "ids_per_s": nnz / w,
                 "ids_returned": nnz, "count_pass_ms": med[0], "scan_ms": med[1], "fill_pass_ms": med[2],
                 "count_pass_share_of_call": med[0] / 1e3 / w}
            # the CPU figures on a sample of the same filters
            k = a.sample
            sp = (fp[0][:int(fp[1][k]) + 64].copy(), fp[1][:k + 1].copy())
            dro, dids = ix.match(sp)
            t0 = time.perf_counter()
            hro, hids = ix.match_host(sp)
            th = time.perf_counter() - t0
            if not (np.array_equal(dro, hro) and np.array_equal(dids, hids)):
                raise SystemExit(f"{name}: device rows != host-walk rows")
            tuniq = np.unique(tcodes, axis=0)
            t0 = time.perf_counter()
            sc = scan_counts(tuniq, fc[:k])
            ts = time.perf_counter() - t0
            if sc != [int(x) for x in np.diff(hro)]:
                raise SystemExit(f"{name}: linear-scan row lengths != host-walk row lengths")
            r.update({"sample_filters": k, "host_walk_filters_per_s": k / th, "numpy_table_scan_filters_per_s": k / ts,
                      "sample_rows_equal": True})
            res[name] = r
        ix.release()
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--topics", type=int, default=1_000_000)
    p.add_argument("--c2-filters", type=int, default=1_000_000)
    p.add_argument("--filters", type=int, default=100_000)
    p.add_argument("--sample", type=int, default=1000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--limit", type=int, default=420, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_retained", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--{k.replace('_', '-')}={getattr(a, k)}"
           for k in ("topics", "c2_filters", "filters", "sample", "runs", "seed")]
    for step, limit in (("device", a.limit),):
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                             "--step", step, "--part", part] + fwd).returncode
        if rc != 0:
            raise SystemExit(f"step {step} failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
