"""The N>1 path of bench.py, rehearsed on one GPU: two ranks under
torch.distributed.run with the rank plumbing over gloo and both ranks pinned to
device 0 (GM_BENCH_BACKEND / GM_BENCH_DEVICE).  The driver's 2/4/8-GPU runs use
the same code with one rank per GPU over RCCL."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(args, world=2):
    env = dict(os.environ, GM_BENCH_BACKEND="gloo", GM_BENCH_DEVICE="0", PYTHONUNBUFFERED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(ROOT, "bench.py"),
           "--gpus", str(world), "--steps", "2", "--warmup", "1", "--full", "--no-cpu"] + args
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-3000:]  # rank 0 prints exactly one line
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_two_ranks_c2():
    one = _run_ranks(["--filters", "20000", "--topics", "1000000"], world=1)
    two = _run_ranks(["--filters", "20000", "--topics", "1000000"], world=2)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["detail"]["ranks_compiled"] == 1 and two["detail"]["replicas_agree"] is True
    # weak scaling: each rank matches its own slice, same per-rank work
    assert two["config"]["topics_per_gpu"] == one["config"]["topics_per_gpu"] == 1_000_000
    assert two["value"] > 0 and two["roofline"]["frac"] > 0
    # the two slices are different windows of the same stream: same matches/topic within noise
    assert abs(two["detail"]["matches_per_topic"] - one["detail"]["matches_per_topic"]) < 0.1
    # the drop-in path's multi-GPU form: rank 0 opens ONE context over the ranks' devices (here
    # device 0 twice), replicates the index in a tree, spreads one host-buffer call over both
    # and applies 200-op updates on both replicas at once
    for out, devs in ((one, [0, 0]), (two, [0, 0])):
        m = out["detail"]["multi_device"]
        assert m["devices"] == devs and m["replica_mode"] == "copied", m
        assert m["host_io_multi_topics_per_s"] > 0 and m["host_io_multi_nnz_matches_device"] is True, m
        u = m["index_update_replicas"]
        assert all(r["replica_mode"] == "patched" and r["replicas"] == 1 for r in u["rounds"]), u
    assert one["detail"]["multi_device"]["index_update_replicas"]["vs_single_device"] > 0
    # the host path against its link: bytes per topic each way and the measured peaks
    link = one["detail"]["host_io_link"]
    assert link["h2d_bytes_per_topic"] > 2 and link["h2d_peak_gbs"] > 0 and 0 < link["h2d_frac_of_peak"] < 1.5
    # the first update says what it did (an index built here keeps its mirror: no download)
    assert one["detail"]["index_update"]["first_includes_mirror_download"] is False


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_two_ranks_c5_exchange():
    out = _run_ranks(["--config", "c5", "--plan", "hash", "--filters", "50000", "--topics", "200000"], world=2)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong"
    assert out["detail"]["exchange_bytes_per_step_rank0"] > 0
    assert out["matches_per_sec"] > 0
    # rank 0's merged rows (slice 0: the shards' pieces merged by global id) = the oracle
    assert out["parity_sample"]["ok"] and out["parity_sample"]["topics"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_two_ranks_c5_replicated():
    """C5's default plan (north_star: replicate while the index fits): the
    unsharded index on every rank, the batch partitioned, weak scaling."""
    out = _run_ranks(["--config", "c5", "--filters", "2000000", "--topics", "200000"], world=2)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    assert out["config"]["topics_per_gpu"] == 200_000 and "replicated" in out["config"]["workload"]
    assert out["parity_sample"]["ok"]
    # the index is compiled ONCE (rank 0) and the other rank imports its image
    d = out["detail"]
    assert d["index_source"] == "built" and d["ranks_compiled"] == 1, d
    assert d["replicas_agree"] is True and d["host_peak_rss_gb_max"] > 0
    # the importing rank neither renders the filter strings nor compiles: less host memory
    rss = d["host_peak_rss_gb_per_rank"]
    assert len(rss) == 2 and rss[1] < rss[0], rss


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_two_ranks_c5_prefix():
    """C5 prefix-sharded: each rank walks about half of the two ranks' topics."""
    out = _run_ranks(["--config", "c5", "--plan", "prefix", "--filters", "200000", "--topics", "200000"], world=2)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    walked = out["detail"]["topics_walked_per_rank"]
    assert sum(walked) == 400_000 and min(walked) > 0.35 * 400_000
    assert out["detail"]["exchange_bytes_per_step_rank0"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_two_ranks_c4():
    out = _run_ranks(["--config", "c4"], world=2)
    assert out["n_gpus"] == 2 and out["config"]["pairs"] == 10**9


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_c5_prefix_one_gpu_device_path():
    """bench.py --config c5 --plan prefix --gpus 1 on its default (nccl) path:
    PrefixShardedMatcher on device tensors, the exchange's copy path at world 1,
    and the oracle parity sample over rank 0's rows."""
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.pop("GM_BENCH_BACKEND", None)
    env.pop("GM_BENCH_DEVICE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c5", "--plan", "prefix", "--gpus", "1",
           "--filters", "4000000", "--topics", "2000000", "--steps", "3", "--warmup", "1", "--full", "--no-cpu"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=380)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith('{"metric"')][-1])
    assert out["detail"]["device_exchange"] is True
    assert out["detail"]["topics_walked_per_rank"] == [2_000_000]
    assert out["parity_sample"]["ok"], out["parity_sample"]


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_replicated_index_rccl_branch_lockstep():
    """bench.replicated_index on its device-tensor (RCCL) branch, 3 ranks as
    threads on one GPU with a lock-step broadcast: rank 0 compiles, ranks 1-2
    import the broadcast image + device tables; every replica's rows equal rank
    0's and the oracle's, and an imported replica takes an in-place update
    (tests/_replicate_worker.py)."""
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "_replicate_worker.py"), "3", "200000",
                        "100000"], cwd=ROOT, capture_output=True, text=True, timeout=380,
                       env={k: v for k, v in os.environ.items() if k not in ("GM_BENCH_BACKEND", "GM_BENCH_DEVICE")})
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "REPLICATE_OK world=3" in p.stdout


DUMP_NAMES = ("shape", "rows", "row_begin", "row_end", "ids")


def _plain_bench_dump(args, out_dir):
    """A plain (no --full) one-GPU bench run with --dump-outputs: (the result line, the arrays)."""
    import numpy as np
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.pop("GM_BENCH_BACKEND", None)
    env.pop("GM_BENCH_DEVICE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args + ["--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-3000:]
    got = {n: np.load(out_dir / f"{n}.npy") for n in DUMP_NAMES}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    return json.loads(lines[0]), got


def _oracle_rows(orc, seed, n_filters, n_topics, wildcard_only):
    """The oracle's match_routes rows (ids = rank among the sorted unique filters)
    of the bench's seeded filters and its first n_topics topics."""
    import bench
    from emqx_amd.engine import gen_filter_codes, render_codes
    codes = gen_filter_codes(seed, n_filters, wildcard_only=wildcard_only)
    fpack = render_codes(codes)
    r = orc.Router(True)
    r.add_routes(fpack)
    topics = orc.render_codes(orc.gen_topic_codes(seed, 0, n_topics, codes))
    oro, oids, _ = r.match_batch(topics, orc.Ranker(bench.sorted_unique(*fpack)), mode=1, nthreads=8)
    return oro, oids


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bench_plain_run_dumps_last_step(tmp_path, orc):
    """A plain run times the steps and prints the headline alone (what --full
    adds is absent), and --dump-outputs writes the last timed step's CSR as
    float64 arrays: here every row of a 100k-topic batch, equal to the oracle's
    rows over the same seeded filters and topics."""
    import numpy as np
    n_filters, n_topics = 20_000, 100_000
    out, got = _plain_bench_dump(["--steps", "3", "--warmup", "1", "--filters", str(n_filters),
                                  "--topics", str(n_topics)], tmp_path / "out")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "topics/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["roofline"]["timed_launches"] == 3 and out["roofline"]["frac"] > 0
    assert not {"cpu_baseline", "vs_cpu", "parity_sample"} & set(out)
    assert not {"host_io_topics_per_s", "index_update", "subs_update", "multi_device"} & set(out["detail"])
    assert got["shape"].tolist() == [n_topics, out["detail"]["nnz_per_step"]]
    assert np.array_equal(got["rows"], np.arange(n_topics))
    oro, oids = _oracle_rows(orc, 1, n_filters, n_topics, wildcard_only=True)
    assert np.array_equal(got["row_begin"], oro[:-1]) and np.array_equal(got["row_end"], oro[1:])
    assert np.array_equal(got["ids"], oids)


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("plan", ["hash", "prefix"])
def test_bench_plain_c5_plans_dump_last_step(tmp_path, orc, plan):
    """The sharded C5 plans' plain runs at one GPU (device tensors): the dumped
    rows of the last step are the oracle's over the whole filter set."""
    import numpy as np
    n_filters, n_topics = 50_000, 100_000
    out, got = _plain_bench_dump(["--config", "c5", "--plan", plan, "--steps", "2", "--warmup", "1",
                                  "--filters", str(n_filters), "--topics", str(n_topics)], tmp_path / "out")
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and "parity_sample" not in out
    oro, oids = _oracle_rows(orc, 1, n_filters, n_topics, wildcard_only=False)
    assert got["shape"].tolist() == [n_topics, len(oids)]
    assert np.array_equal(got["rows"], np.arange(n_topics))
    assert np.array_equal(got["row_begin"], oro[:-1]) and np.array_equal(got["row_end"], oro[1:])
    assert np.array_equal(got["ids"], oids)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bench_plain_c4_dumps_last_step(tmp_path):
    """C4's plain run keeps the last step's part for the dump: every topic's
    row is subscribers 0..999,999 in order (hot/# -> 0..599,999, hot/+/x/# ->
    600,000..999,899, the exact filter -> 999,900..999,999), the row offsets
    are k * 10^6, and the ids stop at the cap (four rows and a half)."""
    import numpy as np
    import bench
    out, got = _plain_bench_dump(["--config", "c4", "--steps", "2", "--warmup", "1"], tmp_path / "out")
    assert out["steps"] == 2 and out["config"]["pairs"] == 10**9 and out["unit"] == "deliveries/s"
    assert got["shape"].tolist() == [1000, 10**9]
    assert np.array_equal(got["rows"], np.arange(1000))
    assert np.array_equal(got["row_begin"], np.arange(1000) * 1e6)
    assert np.array_equal(got["row_end"], np.arange(1, 1001) * 1e6)
    assert len(got["ids"]) == bench.DUMP_MAX_IDS
    assert np.array_equal(got["ids"], np.arange(bench.DUMP_MAX_IDS) % 10**6)


@pytest.mark.gpu
def test_dump_outputs_of_a_device_part_with_a_global_base(tmp_path, orc):
    """dump_outputs on a device result whose ids start at a global offset (a
    later rank's emqx_gm_fanout_part: global row offsets, ids from `first`
    on): part 1 of 3 of the 1/10-scale C4 fan-out begins and ends inside rows,
    and its dump holds exactly its own slice of the whole fan-out's ids."""
    import numpy as np
    import bench
    from emqx_amd import Context
    from emqx_amd.engine import pack
    from tests._fanout_part_worker import c4_small
    filters, subs, topics = c4_small()
    with Context(0) as ctx:
        idx = ctx.build_index(filters, subs=subs)
        tb, to = pack(topics)
        d_tb, d_to = ctx.dev_alloc(len(tb)), ctx.dev_alloc(len(to) * 8)
        ctx.memcpy_h2d(d_tb, tb, len(tb))
        ctx.memcpy_h2d(d_to, to, len(to) * 8)
        m = ctx.match_device(idx, d_tb, d_to, len(topics), exact=True)
        whole = ctx.fanout_device(idx, m)
        w_ro, w_ids = whole.rows(0, len(topics))
        part, first = ctx.fanout_part(idx, m, 1, 3)
        n = part.nnz
        assert 0 < first and first + n < len(w_ids) and n <= bench.DUMP_MAX_IDS
        assert first not in w_ro and first + n not in w_ro  # (both cuts fall inside rows)
        bench.dump_outputs(ctx, part, str(tmp_path), seed=1, base=first)
        for x in (part, whole, m):
            x.free()
        ctx.dev_free(d_tb)
        ctx.dev_free(d_to)
        idx.release()
    got = {k: np.load(tmp_path / f"{k}.npy") for k in DUMP_NAMES}
    assert got["shape"].tolist() == [len(topics), n]
    assert np.array_equal(got["row_begin"], w_ro[:-1]) and np.array_equal(got["row_end"], w_ro[1:])
    assert np.array_equal(got["ids"], w_ids[first:first + n])
