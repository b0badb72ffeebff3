"""Authorization-check A/B: windows of requests against a built-in-database-shaped
table on the device (k_authz_check) and on the library's own single-threaded
host walk (emqx_gm_authz_check_host) over the same requests, in one run on one
box.  The host walk is this project's C++ restatement on one core, NOT the
reference's Erlang (emqx_authz:authorize/5 was not run here).

Table: a 64-rule file segment in front (who leaves of every kind), then the
built-in database: --clientids clientid records x 4 rules, --usernames username
records x 8 rules, 32 `all` rules.  Requests: 70 % from clients that have a
clientid record (and as many with a username record); windows of 1,024, 16,384,
1M and 16M requests (the 16M window is the 1M window repeated 16 times; its
host-walk time is the 1M window's x 16).  Per window: kernel ms by device events
(median of --runs after a warm-up), host-to-host ms of the whole call, requests/s,
the bytes the kernel must move per request (the request's own inputs and
outputs, one 32-B key slot per keyed segment, and the rule, filter and word
records of the client's own ranges; the shared GLOBAL rules stay in cache) and
the fraction of 8 TB/s that implies, and the host walk's time.

The measuring step runs in a child process under its own time limit; the
script stops at the first failing step.

usage: authz_ab.py [--clientids 1000000] [--usernames 10000] [--out profiles/r08_authz/ab.json]
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(a):
    """The description's arrays, built with numpy (4M rules: no per-rule Python objects)."""
    import numpy as np
    from emqx_amd.authz import BY_CLIENTID, BY_USERNAME, GLOBAL, DescArrays, cidr_bytes
    from emqx_amd.engine import pack
    nc, nu = a.clientids, a.usernames
    # ---- the file segment: 64 rules, one leaf kind after the other
    leaf_kind, leaf_arg, who_off, filters, filt_off = [], [], [0], [], [0]
    perm, action, op = [], [], []
    for j in range(64):
        k = j % 4
        if k == 0:
            leaf_kind.append(2), leaf_arg.append(cidr_bytes("10.%d.0.0/16" % j))
        elif k == 1:
            leaf_kind.append(0), leaf_arg.append(b"admin%d" % j)
        elif k == 3:
            leaf_kind.append(3), leaf_arg.append(bytes([j % 8]))
        who_off.append(len(leaf_kind))
        filters += [b"sys/%d/#" % j, b"ctl/+/%d" % j]
        filt_off.append(len(filters))
        perm.append(1 + j % 2), action.append(1 + j % 3), op.append(0)
    # ---- clientid records x 4, username records x 8, 32 `all` rules: who = all, one filter each
    crules = [b"d/${clientid}/up", b"d/${clientid}/down", b"x/%d/y", b"d/${clientid}/#"]
    cf = [crules[r] if r != 2 else b"x/%d/y" % (i % 1000) for i in range(nc) for r in range(4)]
    uf = [b"t/%d/%d" % (i % 500, r) for i in range(nu) for r in range(8)]
    af = [b"m/%d/#" % r for r in range(32)]
    n_rules = 64 + 4 * nc + 8 * nu + 32
    filters += cf + uf + af
    filt_off = np.concatenate([np.array(filt_off, np.uint64), 128 + np.arange(1, 4 * nc + 8 * nu + 32 + 1, dtype=np.uint64)])
    who_off = np.concatenate([np.array(who_off, np.uint64), np.full(n_rules - 64, len(leaf_kind), np.uint64)])
    perm = np.concatenate([np.array(perm, np.uint8), np.tile(np.array([1, 1, 1, 2], np.uint8), nc),
                           np.tile(np.array([1, 2], np.uint8), 4 * nu), np.tile(np.array([1, 2], np.uint8), 16)])
    action = np.concatenate([np.array(action, np.uint8), np.tile(np.array([1, 2, 3, 3], np.uint8), nc),
                             np.full(8 * nu, 3, np.uint8), np.full(32, 3, np.uint8)])
    op = np.zeros(n_rules, np.uint8)
    keys = [b""] + [b"c%07d" % i for i in range(nc)] + [b"u%05d" % i for i in range(nu)] + [b""]
    range_rule_off = np.concatenate([[0], [64], 64 + 4 * np.arange(1, nc + 1), 64 + 4 * nc + 8 * np.arange(1, nu + 1),
                                     [n_rules]]).astype(np.uint64)
    seg_range_off = [0, 1, 1 + nc, 1 + nc + nu, 2 + nc + nu]
    return DescArrays([GLOBAL, BY_CLIENTID, BY_USERNAME, GLOBAL], seg_range_off, range_rule_off, pack(keys),
                      np.arange(n_rules, dtype=np.uint32), perm, action, op, who_off, filt_off, leaf_kind,
                      pack(leaf_arg), np.zeros(len(filters), np.uint8), pack(filters))


def requests(a, n, seed=1):
    """n requests; 70 % from clients with a clientid record (ids below --clientids)."""
    import numpy as np
    from emqx_amd.authz import F_CLIENTID, F_PEERHOST, F_USERNAME, RequestBatch
    from emqx_amd.engine import pack
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, int(a.clientids / 0.7), n)
    ui = rng.integers(0, int(a.usernames / 0.7), n)
    kind = rng.integers(0, 10, n)
    k = rng.integers(0, 1000, n)
    cids = [b"c%07d" % i for i in ci]
    topics = [(b"d/" + c + b"/up") if t < 4 else (b"d/" + c + b"/zzz") if t < 6 else (b"t/%d/%d" % (x % 500, x % 8))
              if t < 8 else (b"m/%d/q" % (x % 40)) if t < 9 else b"other/%d" % x for c, t, x in zip(cids, kind, k)]
    peer = np.zeros((n, 16), np.uint8)
    peer[:, 0], peer[:, 1], peer[:, 2], peer[:, 3] = 10, rng.integers(64, 200, n), rng.integers(0, 256, n), 1
    return RequestBatch(pack(topics), pack(cids), pack([b"u%05d" % i for i in ui]),
                        np.full(n, F_CLIENTID | F_USERNAME | F_PEERHOST, np.uint8), peer.reshape(-1),
                        rng.integers(1, 3, n).astype(np.uint8), np.zeros(n, np.uint32))


def tile(b, times):
    """The window repeated `times` times."""
    import numpy as np
    from emqx_amd.authz import RequestBatch

    def col(bytes_, off):
        end = int(off[-1])
        return (np.concatenate([np.tile(bytes_[:end], times), np.zeros(64, np.uint8)]),
                np.concatenate([[0], (off[1:][None, :] + (np.arange(times, dtype=np.uint64) * np.uint64(end))[:, None]).reshape(-1)])
                .astype(np.uint64))
    x = b.a
    return RequestBatch(col(x[0], x[1]), col(x[2], x[3]), col(x[4], x[5]), np.tile(x[6], times), np.tile(x[7], times),
                        np.tile(x[8], times), np.tile(x[9], times))


def step_device(a):
    import numpy as np
    from emqx_amd import Context
    t0 = time.perf_counter()
    d = table(a)
    t_arrays = time.perf_counter() - t0
    res = {"clientids": a.clientids, "usernames": a.usernames, "rules": d.n_rules, "runs": a.runs,
           "baseline": "the library's own host walk (emqx_gm_authz_check_host), C++ on one core; not the reference's Erlang",
           "windows": {}}
    with Context(0) as ctx:
        t0 = time.perf_counter()
        tab = ctx.build_authz(d)
        info = tab.info()
        res["build"] = {"build_ms": info.build_ms, "wall_ms": (time.perf_counter() - t0) * 1e3, "arrays_s": t_arrays,
                        "device_bytes": int(info.device_bytes), "n_keys": int(info.n_keys), "n_words": int(info.n_words),
                        "deepest_filter": int(info.deepest_filter), "longest_range": int(info.longest_range)}
        print("build", json.dumps(res["build"]), flush=True)
        base = requests(a, 1 << 20)
        t0 = time.perf_counter()
        hv, hr = tab.check_host(base)
        host_1m = time.perf_counter() - t0
        for n in a.windows:
            if n <= 1 << 20:
                b = requests(a, n) if n < 1 << 20 else base
                t0 = time.perf_counter()
                wv, wr = (hv, hr) if n == 1 << 20 else tab.check_host(b)
                th = host_1m if n == 1 << 20 else time.perf_counter() - t0
            else:
                times = n >> 20
                b = tile(base, times)
                wv, wr, th = np.tile(hv, times), np.tile(hr, times), host_1m * times
            kern, wall = [], []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                v, ru = tab.authorize_batch(b, timed=True)
                w = (time.perf_counter() - t0) * 1e3
                if r:  # (the first is the warm-up)
                    wall.append(w)
                    kern.append(tab.last_kernel_ms())
            if not (np.array_equal(v, wv) and np.array_equal(ru, wr)):
                raise SystemExit(f"window {n}: device answers != host-walk answers")
            x = b.a
            in_bytes = (int(x[1][-1]) + int(x[3][-1]) + int(x[5][-1])) / n + 3 * 4 + 16 + 1 + 1 + 4 + 5
            has_c = float(np.mean(wr != 0xFFFFFFFF))
            table_bytes = 2 * 32 + 0.7 * 4 * (16 + 8 + 3 * 4) + 0.7 * 8 * (16 + 8 + 3 * 4)
            per_req = in_bytes + table_bytes
            km, wm = statistics.median(kern), statistics.median(wall)
            res["windows"][str(n)] = {
                "kernel_ms": km, "host_to_host_ms": wm, "requests_per_s_kernel": n / km * 1e3,
                "requests_per_s_host_to_host": n / wm * 1e3, "bytes_per_request": per_req,
                "fraction_of_8TBps": per_req * n / (km * 1e-3) / 8e12, "host_walk_ms": th * 1e3,
                "host_walk_requests_per_s": n / th, "device_vs_host_walk": th * 1e3 / wm, "matched_fraction": has_c,
                "verdicts": [int(np.sum(wv == k)) for k in range(3)], "answers_equal": True}
            print(n, json.dumps(res["windows"][str(n)]), flush=True)
            with open(a.part, "w") as f:  # (after every window: a later one that runs out of time loses nothing)
                json.dump(res, f, indent=1)
        tab.release()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clientids", type=int, default=1_000_000)
    p.add_argument("--usernames", type=int, default=10_000)
    p.add_argument("--windows", type=lambda s: [int(x) for x in s.split(",")], default=[1024, 16384, 1 << 20, 16 << 20])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--limit", type=int, default=540, help="seconds for the measuring step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_authz", "ab.json"))
    p.add_argument("--step", default=None)
    p.add_argument("--part", default=None)
    a = p.parse_args()
    if a.step == "device":
        return step_device(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    part = a.out + ".part"
    fwd = [f"--clientids={a.clientids}", f"--usernames={a.usernames}", f"--runs={a.runs}",
           "--windows=" + ",".join(map(str, a.windows))]
    for step, limit in (("device", a.limit),):
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                             "--step", step, "--part", part] + fwd).returncode
        if rc != 0:
            raise SystemExit(f"step {step} failed (exit {rc}); stopping")
    os.replace(part, a.out)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
