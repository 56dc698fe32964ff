"""A plain `bench.py` run (no --full) as a fresh child process: the result line, and what
--dump-outputs writes is what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _bench(args):
  p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                     capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stderr[-2000:]
  return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_dumps_the_headline_state_exactly(gpu, tmp_path):
  """--steps 1 --warmup 0: one fused launch of config 2's whole 1000 steps, the workload of
  fixture G22; the dumped `b` of all 1024 columns has the reference's digests exactly, and its
  sum is the line's checksum.  The plain line holds the headline keys and none of --full's."""
  out = _bench(["--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs",
                str(tmp_path / "dump")])
  for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
    assert k in out, k
  assert out["steps"] == 1 and out["warmup"] == 0 and out["ms_per_step"] > 0
  assert out["value"] > 0 and out["dtype"] == "f64" and out["higher_is_better"] is True
  assert not set(out) & {"contracted", "cpu_baseline", "single_step_us", "hbm_regime", "c3", "c6"}
  assert sorted(os.listdir(str(tmp_path / "dump"))) == ["b.npy"]
  b = np.load(str(tmp_path / "dump" / "b.npy"))
  assert b.dtype == np.float64 and b.shape == (1024, 100)
  assert float(np.sum(b)) == out["checksum"]
  g = load_golden("c2_ensemble_digests")
  assert int(g["nsteps"]) == 1000
  d = np.stack([np.array([np.sum(r), np.sum(r * r)]) for r in b])
  assert np.array_equal(d, g["digest"])


REF_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PM_ROOT"])
import pymoc_amd
from pymoc_amd import configs
ens = pymoc_amd.TwoColEnsemble(configs.config3(N=64), diag_iters=240)
ens.run(ens.M)      # the warm-up interval
ens.run(2 * ens.M)  # the two timed ones
np.savez(os.environ["PM_OUT"], **ens.state())
'''


def test_plain_coupled_run_dumps_the_ensemble_state(gpu, tmp_path):
  """--config 3: the dumped arrays are the state() of the same ensemble run for the same
  (warm-up + timed) model steps by the package directly (in a child process), bit for bit."""
  out = _bench(["--gpus", "1", "--config", "3", "--members", "64", "--steps", "2", "--warmup",
                "1", "--dump-outputs", str(tmp_path / "dump")])
  assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["roofline"] is None
  ref = str(tmp_path / "ref.npz")
  p = subprocess.run([sys.executable, "-c", REF_WORKER], capture_output=True, text=True,
                     timeout=300, env=dict(os.environ, PM_ROOT=ROOT, PM_OUT=ref))
  assert p.returncode == 0, p.stderr[-2000:]
  st = np.load(ref)
  assert sorted(os.listdir(str(tmp_path / "dump"))) == sorted(k + ".npy" for k in st.files)
  for k in st.files:
    got = np.load(str(tmp_path / "dump" / (k + ".npy")))
    assert got.dtype == np.float64 and np.array_equal(got, st[k], equal_nan=True), k
