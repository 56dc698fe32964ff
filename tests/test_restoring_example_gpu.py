"""examples/amoc_early_warning_restoring.py runs end to end at a small size: it prints all four
indicators, finds lam and rho bit-identical to the restatement, and the `lam` group means and tau
medians it prints equal the restatement (tests/restoring_cases.py, tests/stats_cases.py,
tests/windows_cases.py) on the series it saved, exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import restoring_cases as RC
import stats_cases as STC
import windows_cases as WC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_early_warning_restoring_example(gpu, tmp_path):
  saved = str(tmp_path / "series.npz")
  p = subprocess.run([sys.executable, "examples/amoc_early_warning_restoring.py", "--sets", "2",
                      "--realisations", "4", "--years", "60", "--spinup", "4", "--window", "20",
                      "--step", "4", "--significance", "--nsur", "9", "--save-series", saved],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 60 years; warming ramp over years 10-60; noise seed 2018" in out, out
  assert ("years 4-59: 10 windows of 20 years every 4 years, linear trend removed, lag 1; DFA "
          "scales 4 5; restoring rate per year, 10 iterations") in out, out
  assert "restatement on the downloaded series: lam and rho every bit agrees" in out, out
  assert "lambda series exact" in out, out
  for key in ("ac", "var", "dfa", "lam"):
    assert re.search(r"^  set  year  members .*\b%s\b" % key, out, flags=re.M), (key, out)
  rows = re.findall(r"^ +(\d+) +(\d+) +(\d+) +(\S+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  shown = [0, 2, 4, 6, 9]  # five of the 10 windows, evenly spaced
  assert [(int(r[0]), int(r[1]), int(r[2])) for r in rows] == [
      (g, 4 + 19 + 4 * i, 4) for g in range(2) for i in shown], out
  got = np.array([[float(x) for x in r[3:]] for r in rows]).reshape(2, 5, 4)
  taus = re.findall(r"^ +(\d+) +(\S+e\S+) +(\S+e\S+) +(\S+e\S+) +(\S+e\S+)$", out, flags=re.M)
  assert [int(r[0]) for r in taus] == [0, 1], out
  got_tau = np.array([[float(x) for x in r[1:]] for r in taus])
  ps = re.findall(r"^ +(\d+) +(\d\.\d{4}) +(\d\.\d{4}) +(\d\.\d{4}) +(\d\.\d{4})$", out, flags=re.M)
  assert [int(r[0]) for r in ps] == [0, 1] and "AR(1)-surrogate test, 9 surrogates" in out, out
  assert all(0.0 <= float(x) <= 1.0 for r in ps for x in r[1:])
  # the restatement on the series the example saved
  z = np.load(saved)
  v, groups = z["series"], z["groups"]
  assert v.shape == (60, 1, 8) and np.isfinite(v).all() and groups.tolist() == [0] * 4 + [1] * 4
  assert (int(z["k0"]), int(z["k1"]), int(z["window"]), int(z["step"]), int(z["iters"])) == (
      4, 60, 20, 4, 10)
  want = RC.restoring(v, 4, 60, 20, 4, "linear", 10)
  assert want["used"].all() and np.isfinite(want["lam"]).all()
  order, start = STC.order_of(groups)
  wc, ws = STC.group_stats(want["lam"], order, start, (0.05, 0.95), 0, 10)
  assert (wc == 4).all()
  assert np.array_equal(got[:, :, 3], ws[shown, 0, :, 0].T), out
  # ac and var are examples/amoc_early_warning.py's numbers: bit for bit
  wn = WC.windows(v, 4, 60, 20, 4, 1, "linear")
  for j, i in ((0, 3), (1, 2)):
    _, w = STC.group_stats(wn["out"][i], order, start, (0.05, 0.95), 0, 10)
    assert np.array_equal(got[:, :, j], w[shown, 0, :, 0].T), out
  conc, disc, tie, nfin = WC.kendall(want["lam"], 0, 10)
  assert (nfin == 10).all()
  tau = WC.tau_b(conc[0], disc[0], tie[0])
  for g in range(2):
    assert got_tau[g, 3] == float(np.median(tau[groups == g])), out
  assert np.isfinite(got).all() and np.isfinite(got_tau).all()
