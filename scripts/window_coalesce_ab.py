"""Publish windows from several callers at once on one context: the direct
emqx_gm_match_fanout calls (each caller its own device round trip) against the
same calls through one emqx_gm_combiner at its defaults (windows that arrive
while earlier groups are on the device run as one group), in the same process
and library, interleaved.  C2's index (1M wildcard filters) with 1-4
subscribers per filter, topics of its stream.  Per (window, callers): topics/s
(the median of --reps runs after a warm-up, with the run-to-run spread), the
window latency (median and maximum over all calls) and the combiner's mean
group size.  The calls go straight through ctypes (no numpy copy of the
results), so the figures are the library's, not the Python layer's.
usage: window_coalesce_ab.py [--reps 5] [--out profiles/r11_windows/ab.json]"""

import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(c, ix, cb, pb, ho, threads, calls, batch):
    """One timed run: (topics/s, [latency_s of every call])."""
    from emqx_amd import _lib
    L = _lib.lib()
    n = len(ho) - 1
    errs, lats = [], [None] * threads
    tbp = C.c_void_p(pb.ctypes.data)

    def one(t):
        m, d = _lib.Csr(), _lib.Csr()
        mine = []
        try:
            for k in range(calls):
                s0 = ((t * calls + k) * batch) % max(1, n - batch)
                top = C.c_void_p(ho.ctypes.data + 8 * s0)
                t0 = time.perf_counter()
                if cb is None:
                    rc = L.emqx_gm_match_fanout(c.h, ix.h, tbp, top, batch, _lib.WITH_EXACT, C.byref(m), C.byref(d))
                else:
                    rc = L.emqx_gm_combiner_match(cb.h, ix.h, tbp, top, batch, _lib.WITH_EXACT, C.byref(m),
                                                  C.byref(d))
                mine.append(time.perf_counter() - t0)
                if rc:
                    raise RuntimeError(f"rc {rc}")
                L.emqx_gm_csr_free(c.h, C.byref(m))
                L.emqx_gm_csr_free(c.h, C.byref(d))
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
        lats[t] = mine

    th = [threading.Thread(target=one, args=(t,)) for t in range(threads)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    if errs:
        raise RuntimeError(errs[0])
    return threads * calls * batch / dt, [x for l in lats for x in l]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_windows", "ab.json"))
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda:0")
    from emqx_amd import Context
    from emqx_amd.engine import gen_filter_codes, render_codes
    c = Context(0)
    codes = gen_filter_codes(1, 1_000_000, wildcard_only=True)
    fb, fo = render_codes(codes)
    nf = len(fo) - 1
    rng = np.random.default_rng(1)
    so = np.zeros(nf + 1, np.uint64)
    so[1:] = np.cumsum(rng.integers(1, 5, size=nf))
    si = rng.integers(0, 1 << 24, size=int(so[-1])).astype(np.uint32)
    ix = c.build_index((fb, fo), subs=(so, si))
    n = 4_000_000
    db, do, tot = c.gen_topics_device(codes, 1, 0, n)
    ho = np.zeros(n + 1, np.uint64)
    c.memcpy_d2h(ho, do, (n + 1) * 8)
    pb = c.host_alloc(tot + 64)
    c.memcpy_d2h(pb, db, tot)
    # "combiner": the defaults, the figures to report; "combiner_in_flight_1": one
    # setting away from them (max_in_flight = 1), to show what the default policy leaves
    via = {"direct": None, "combiner": c.combiner(), "combiner_in_flight_1": c.combiner(max_in_flight=1)}
    rows = []
    for batch, calls in ((1024, 200), (16384, 24)):
        for threads in (1, 2, 4, 8):
            res = {m: [] for m in via}
            lat = {m: [] for m in via}
            for mode in res:  # (warm)
                run(c, ix, via[mode], pb, ho, threads, 4, batch)
            st0 = {m: q.stats() for m, q in via.items() if q}
            for _ in range(a.reps):
                for mode in res:
                    r, l = run(c, ix, via[mode], pb, ho, threads, calls, batch)
                    res[mode].append(r)
                    lat[mode] += l
            st1 = {m: q.stats() for m, q in via.items() if q}
            row = {"window_topics": batch, "callers": threads, "calls_per_caller": calls, "reps": a.reps,
                   "window_bytes_mean": float(ho[batch * 64] - ho[0]) / 64}
            for m in st0:
                row["mean_group" if m == "combiner" else "mean_group_in_flight_1"] = (
                    (st1[m]["windows"] - st0[m]["windows"]) / max(1, st1[m]["groups"] - st0[m]["groups"]))
            for mode in res:
                v = sorted(res[mode])
                med = v[len(v) // 2]
                row[mode] = {"topics_per_s": med, "spread": (v[-1] - v[0]) / med, "runs": res[mode],
                             "latency_us_median": float(np.median(lat[mode])) * 1e6,
                             "latency_us_max": float(np.max(lat[mode])) * 1e6}
            row["combiner_over_direct"] = row["combiner"]["topics_per_s"] / row["direct"]["topics_per_s"]
            rows.append(row)
            row["in_flight_1_over_direct"] = row["combiner_in_flight_1"]["topics_per_s"] / row["direct"]["topics_per_s"]
            d, k, k1 = row["direct"], row["combiner"], row["combiner_in_flight_1"]
            print(f"window {batch:6d} callers {threads}: direct {d['topics_per_s'] / 1e6:8.2f} M topics/s "
                  f"(+-{d['spread'] * 50:4.1f}%, {d['latency_us_median']:7.1f} us median, {d['latency_us_max']:8.1f} max)"
                  f"  combiner {k['topics_per_s'] / 1e6:8.2f} M topics/s (+-{k['spread'] * 50:4.1f}%, "
                  f"{k['latency_us_median']:7.1f} us median, {k['latency_us_max']:8.1f} max, group "
                  f"{row['mean_group']:.2f})  {row['combiner_over_direct']:.2f}x  | max_in_flight=1 "
                  f"{k1['topics_per_s'] / 1e6:8.2f} M topics/s ({k1['latency_us_median']:7.1f} us median, group "
                  f"{row['mean_group_in_flight_1']:.2f})", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"index": "C2: 1M wildcard filters, 1-4 subscribers each", "entry": "emqx_gm_match_fanout",
                   "combiner_opts": "defaults (combiner_in_flight_1: max_in_flight = 1, else defaults)",
                   "rows": rows}, f, indent=1)
        f.write("\n")
    for q in via.values():
        if q:
            q.close()
    c.host_free(pb)
    c.dev_free(db)
    c.dev_free(do)
    ix.release()
    c.close()


if __name__ == "__main__":
    main()
