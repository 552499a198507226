"""bench.py's --dump-outputs writer and its options, without a GPU."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("pengk_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_outputs_are_written_whole_as_float32_or_float64(tmp_path):
    b = load_bench()
    counts = np.arange(4 ** 8, dtype=np.uint32) * np.uint32(65537)
    arrays = {"counts": counts, "scal": np.array([2 ** 40 + 3, 7], np.int64), "z": np.linspace(-3, 3, 4 ** 8, dtype=np.float32),
              "state": np.array([[10, 0], [4, 1]], np.int32)}
    b.write_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(str(tmp_path))) == ["counts.npy", "scal.npy", "state.npy", "z.npy"]
    for name, want in arrays.items():
        got = np.load(str(tmp_path / (name + ".npy")))
        assert got.dtype == (np.float32 if want.dtype == np.float32 else np.float64) and got.shape == want.shape
        assert np.array_equal(got, want.astype(np.float64)), name  # (exact: every value is below 2^53)


def test_outputs_past_the_budget_are_one_fixed_sample(tmp_path):
    """Past 64 MiB in all (a W = 12 table is 4^12 entries) every long array becomes the same seeded sample of its entries:
    at most 64 MiB on disk, short arrays whole, and the same sample from run to run."""
    b = load_bench()
    n = 4 ** 12
    big = np.arange(n, dtype=np.uint32)
    arrays = {"counts": big, "z": np.arange(n, dtype=np.float32) * np.float32(0.5), "pwms": np.full((16, 12, 4), 0.25, np.float32)}
    b.write_outputs(str(tmp_path / "a"), arrays)
    b.write_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name in arrays:
        a, a2 = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.tobytes() == a2.tobytes() and a.dtype in (np.float32, np.float64)
        total += os.path.getsize(str(tmp_path / "a" / (name + ".npy")))
    assert total <= 64 << 20
    counts = np.load(str(tmp_path / "a" / "counts.npy"))
    z = np.load(str(tmp_path / "a" / "z.npy"))
    assert counts.shape == (b.DUMP_SAMPLE,) and np.all(np.diff(counts) > 0) and np.array_equal(z, (counts * 0.5).astype(np.float32))
    assert np.load(str(tmp_path / "a" / "pwms.npy")).shape == (16, 12, 4)


def test_bench_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and b"--full" in r.stdout and b"--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode != 0 and b"--steps" in r.stderr
