"""bench.py's --dump-outputs writer (dump_outputs) on host CSRs: the whole
result below the row-sample size, the seeded row windows above it, the cap on
the ids written and a part whose ids start at a global offset."""
import numpy as np

import bench

NAMES = ("shape", "rows", "row_begin", "row_end", "ids")


def _csr(n_rows, rng, max_len=4):
    lens = rng.integers(0, max_len + 1, n_rows)
    ro = np.zeros(n_rows + 1, np.uint64)
    ro[1:] = np.cumsum(lens)
    return ro, rng.integers(0, 1 << 32, int(ro[-1]), dtype=np.uint64).astype(np.uint32)


def _load(d):
    got = {n: np.load(d / f"{n}.npy") for n in NAMES}
    assert all(v.dtype == np.float64 and v.ndim == 1 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    return got


def test_small_result_is_written_whole(tmp_path):
    ro, ids = _csr(1000, np.random.default_rng(0))
    bench.dump_outputs(None, (ro, ids), str(tmp_path), seed=1)
    got = _load(tmp_path)
    assert got["shape"].tolist() == [1000, len(ids)]
    assert np.array_equal(got["rows"], np.arange(1000))
    assert np.array_equal(got["row_begin"], ro[:-1]) and np.array_equal(got["row_end"], ro[1:])
    assert np.array_equal(got["ids"], ids)  # (u32 ids are exact in float64)


def test_empty_rows_only(tmp_path):
    ro = np.zeros(8, np.uint64)
    bench.dump_outputs(None, (ro, np.zeros(0, np.uint32)), str(tmp_path), seed=1)
    got = _load(tmp_path)
    assert got["shape"].tolist() == [7, 0] and len(got["ids"]) == 0 and len(got["rows"]) == 7


def test_large_result_is_sampled_in_seeded_windows(tmp_path):
    w, k = bench.DUMP_WINDOW_ROWS, bench.DUMP_WINDOWS
    n = w * k + 3 * w + 5  # one more than fits whole, and no multiple of the window
    ro, ids = _csr(n, np.random.default_rng(1), max_len=3)
    bench.dump_outputs(None, (ro, ids), str(tmp_path / "a"), seed=1)
    bench.dump_outputs(None, (ro, ids), str(tmp_path / "b"), seed=1)
    bench.dump_outputs(None, (ro, ids), str(tmp_path / "c"), seed=2)
    a, b, c = _load(tmp_path / "a"), _load(tmp_path / "b"), _load(tmp_path / "c")
    assert all(np.array_equal(a[x], b[x]) for x in NAMES)  # same arguments, same sample
    assert not np.array_equal(a["rows"], c["rows"])
    rows = a["rows"].astype(np.int64)
    assert len(rows) == w * k and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.all(rows.reshape(k, w)[:, 0] % w == 0) and np.all(np.diff(rows.reshape(k, w), axis=1) == 1)
    assert np.array_equal(a["row_begin"], ro[rows]) and np.array_equal(a["row_end"], ro[rows + 1])
    want = np.concatenate([ids[int(ro[r[0]]):int(ro[r[-1] + 1])] for r in rows.reshape(k, w)])
    assert len(want) < bench.DUMP_MAX_IDS and np.array_equal(a["ids"], want)
    assert a["shape"].tolist() == [n, len(ids)]


def test_ids_stop_at_the_cap_and_parts_start_at_base(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_IDS", 1000)
    # a C4-like part: 10 rows of 500 deliveries, global offsets, this part holding [1200, 3700)
    ro = np.arange(11, dtype=np.uint64) * 500
    held = np.arange(1200, 3700, dtype=np.uint32)
    bench.dump_outputs(None, (ro, held), str(tmp_path / "part"), seed=1, base=1200)
    got = _load(tmp_path / "part")
    assert np.array_equal(got["row_begin"], ro[:-1]) and np.array_equal(got["ids"], held[:1000])
    # ids past what the part holds are never read: a part that ends inside the rows
    bench.dump_outputs(None, (ro, held[:300]), str(tmp_path / "short"), seed=1, base=1200)
    assert np.array_equal(_load(tmp_path / "short")["ids"], held[:300])


def test_plain_run_says_which_options_need_full(monkeypatch, capsys):
    monkeypatch.delenv("GM_BENCH_NO_PIPELINE", raising=False)
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "3", "--subs-update", "--replicas=3", "--no-cpu"])
    a = bench.parse()
    err = capsys.readouterr().err
    assert "--subs-update, --replicas: no effect without --full" in err
    assert a.steps == 3 and not a.subs_update and a.no_multi and a.no_host_io and a.no_parity and a.no_update
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--subs-update", "--no-cpu"])
    a = bench.parse()
    assert capsys.readouterr().err == ""
    assert a.subs_update and a.no_cpu and not (a.no_multi or a.no_host_io or a.no_parity or a.no_update)
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    bench.parse()
    assert capsys.readouterr().err == ""
