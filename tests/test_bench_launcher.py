"""`python bench.py --gpus N` as the driver starts it (no WORLD_SIZE in the environment): the parent must start the
ranks itself, as child processes, and relay their outcome.  On this GPU-less host the ranks meet (gloo) and then each
fails cleanly at `fbs_ctx_create` with FBS_E_DEVICE -- there is no CPU path to fall back to."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_2_launches_its_own_ranks_and_reports_their_failure():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present: the launcher is exercised by the real multi-GPU bench")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                         "--cpu-sample", "0"], env=env, capture_output=True, text=True, timeout=600)
    assert rc.returncode != 0
    assert rc.stdout.strip() == ""                                 # no JSON line is invented
    assert "FBS_E_DEVICE" in rc.stderr and "the 2-rank run failed" in rc.stderr
    assert rc.stderr.count('"rank": ') == 2                         # both ranks got as far as the context


def test_rank_mode_refuses_a_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                        timeout=300)
    assert rc.returncode != 0 and "WORLD_SIZE=4 but --gpus 2" in rc.stderr


def test_plain_run_is_lean_unless_full():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out" and b.steps == 20 and b.warmup == 3


def test_dump_outputs_writes_float64_within_64_mb_and_samples_rows_by_a_fixed_seed(tmp_path):
    import numpy as np
    import bench
    ctw = 1025
    small = np.arange(4 * ctw, dtype=np.uint64).reshape(4, ctw)
    bench.dump_outputs(str(tmp_path / "s"), small, np.array([0, 1, 1, 0]))
    assert np.array_equal(np.load(tmp_path / "s" / "ciphertexts.npy"), small.astype(np.float64))
    assert np.load(tmp_path / "s" / "messages.npy").tolist() == [0, 1, 1, 0]
    assert np.load(tmp_path / "s" / "rows.npy").tolist() == [0, 1, 2, 3]
    big = (np.arange(9000 * ctw, dtype=np.uint64) % ((1 << 46) - 1)).reshape(9000, ctw)     # 74 MB of words
    msgs = np.arange(9000) % 2
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, msgs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["ciphertexts.npy", "messages.npy", "rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    got = np.load(tmp_path / "a" / "ciphertexts.npy")
    assert got.dtype == np.float64 and 8000 < len(rows) < 9000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(got, big[rows].astype(np.float64)) and np.array_equal(np.load(tmp_path / "a" / "messages.npy"), msgs[rows])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
