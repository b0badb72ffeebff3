"""Sharded-update A/B: what a 200-op route update of a prefix-sharded index
costs against the two things the library offered before, on one box in one run
(devices [0, 0], C2's and C3's filter sets, no subscriber lists):

  sharded_update   emqx_gm_index_update on the sharded index (every shard
                   patched or given a new id map, gm_shard.cpp)
  sharded_rebuild  release + emqx_gm_index_build_sharded of the updated set
                   (all a sharded set could do before)
  replicated       the same update of the unsharded index through the same
                   replicated [0, 0] context (each device patches its replica)

Every figure is the median of 5 after one warm-up: wall time of the call and
the call's own device_ms (emqx_gm_last_update_stats).  The update line is
chained (each update applies to the previous result, as a node's subscription
windows do); batches alternate between inserting and deleting the same 200
filters, so the set's size stays put.  bookkeeping_ms = wall - device_ms of
the sharded update: the host plan and the per-shard merge passes.

usage: sharded_update_ab.py [--configs c2,c3] [--ops 200] [--out profiles/r07_sharded_update/ab.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batches(fb, fo, n_ops, unpack, pack):
    """n_ops filters not in the set, under first words the set already has (the
    first n_ops filters with their last word replaced by one the generator never
    makes): the batch that inserts them, the one that deletes them, and the
    packed updated set."""
    import numpy as np
    new = []
    for i, f in enumerate(unpack(fb, fo[:n_ops + 1])):
        g = b"/".join(f.split(b"/")[:-1] + [b"u%d" % i])
        if g not in new:
            new.append(g)
    nb, no = pack(new)
    end = int(fo[-1])
    ub = np.concatenate([fb[:end], nb])
    uo = np.concatenate([fo, no[1:] + np.uint64(end)])
    return [(f, True) for f in new], [(f, False) for f in new], (ub, uo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--ops", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_sharded_update", "ab.json"))
    a = ap.parse_args()
    from emqx_amd import Context
    from emqx_amd.engine import gen_filter_codes, pack, render_codes
    from oracle.oracle import unpack
    res = {"devices": [0, 0], "ops": a.ops, "reps": a.reps, "configs": {}}
    for cfg in a.configs.split(","):
        n_f = {"c2": 1_000_000, "c3": 10_000_000}[cfg]
        fb, fo = render_codes(gen_filter_codes(1, n_f, wildcard_only=cfg == "c2"))
        ins, dele, updated = _batches(fb, fo, a.ops, unpack, pack)
        out = {"n_filters": n_f}
        with Context(devices=[0, 0]) as c:
            def line(ix):
                wall, dev, kinds = [], [], None
                for r in range(a.reps + 1):
                    ops = ins if r % 2 == 0 else dele
                    t = time.perf_counter()
                    nx = c.update_index(ix, ops)
                    w = (time.perf_counter() - t) * 1e3
                    st = c.update_stats()
                    ix.release()
                    ix = nx
                    if r:  # (the first is the warm-up)
                        wall.append(w)
                        dev.append(st["device_ms"])
                        kinds = (st["kind"], c.last_shard_update())
                ix.release()
                return statistics.median(wall), statistics.median(dev), kinds

            w, d, kinds = line(c.build_index_sharded((fb, fo)))
            out["sharded_update"] = {"wall_ms": w, "device_ms": d, "bookkeeping_ms": w - d, "kind": kinds[0],
                                     "shards": kinds[1]}
            w, d, kinds = line(c.build_index((fb, fo)))
            out["replicated"] = {"wall_ms": w, "device_ms": d, "kind": kinds[0]}
            wall = []
            ix = c.build_index_sharded((fb, fo))
            for r in range(a.reps + 1):
                t = time.perf_counter()
                ix.release()
                ix = c.build_index_sharded(updated if r % 2 == 0 else (fb, fo))
                if r:
                    wall.append((time.perf_counter() - t) * 1e3)
            ix.release()
            out["sharded_rebuild"] = {"wall_ms": statistics.median(wall)}
        out["update_vs_rebuild"] = out["sharded_rebuild"]["wall_ms"] / out["sharded_update"]["wall_ms"]
        out["update_vs_replicated"] = out["sharded_update"]["wall_ms"] / out["replicated"]["wall_ms"]
        res["configs"][cfg] = out
        print(cfg, json.dumps(out), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (after every config: a later one that runs out of time loses nothing)
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
