"""bench.py's command line and --dump-outputs writer, without a GPU."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def test_help_lists_full_and_dump_outputs():
  p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                     capture_output=True, text=True, timeout=120)
  assert p.returncode == 0, p.stderr
  assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_zero_timed_steps_is_refused_before_any_work():
  p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                     capture_output=True, text=True, timeout=120)
  assert p.returncode == 2 and "--steps" in p.stderr


def test_dump_outputs_small_arrays_whole_in_float64(tmp_path):
  import bench  # (numpy only at module level: no engine, no GPU)
  b = np.arange(24, dtype=np.float64).reshape(4, 6) / 7.0
  nf = np.array([0, 1, 0, 0], dtype=np.int32)
  names = bench.dump_outputs(str(tmp_path / "out"), {"b": b, "nonfinite": nf})
  assert names == ["b", "nonfinite"]
  got = np.load(str(tmp_path / "out" / "b.npy"))
  assert got.dtype == np.float64 and np.array_equal(got, b)
  got = np.load(str(tmp_path / "out" / "nonfinite.npy"))
  assert got.dtype == np.float64 and np.array_equal(got, nf)
  assert not os.path.exists(str(tmp_path / "out" / "member_index.npy"))


def test_dump_outputs_large_arrays_same_seeded_row_sample(tmp_path):
  import bench
  rng = np.random.default_rng(5)
  a, c = rng.standard_normal((1000, 50)), rng.standard_normal((1000, 7))
  limit = 100000
  for d in ("one", "two"):
    names = bench.dump_outputs(str(tmp_path / d), {"a": a, "c": c}, limit=limit)
    assert names == ["a", "c", "member_index"]
  files = [os.path.join(str(tmp_path / "one"), n + ".npy") for n in names]
  assert sum(os.path.getsize(f) for f in files) <= limit + 3 * 128  # (+ the .npy headers)
  idx = np.load(files[2])
  assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and 0 < idx.size < 1000
  rows = idx.astype(int)
  assert np.array_equal(np.load(files[0]), a[rows]) and np.array_equal(np.load(files[1]), c[rows])
  for n in names:  # the sample is fixed: a second dump is identical
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "one"), n + ".npy")),
                          np.load(os.path.join(str(tmp_path / "two"), n + ".npy")))
