"""examples/amoc_early_warning.py runs end to end at a small size, and the group means, bands and
tau medians it prints equal the restatement (tests/windows_cases.py, tests/stats_cases.py) on the
series it downloaded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stats_cases as STC
import windows_cases as WC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_early_warning_example(gpu, tmp_path):
  saved = str(tmp_path / "series.npz")
  p = subprocess.run([sys.executable, "examples/amoc_early_warning.py", "--sets", "2",
                      "--realisations", "4", "--years", "60", "--spinup", "4", "--window", "16",
                      "--step", "4", "--save-series", saved],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 60 years; warming ramp over years 10-60; noise seed 2018" in out, out
  assert "years 4-59: 11 windows of 16 years every 4 years, linear trend removed, lag 1" in out, out
  assert "restatement on the downloaded series: every bit agrees" in out, out
  rows = re.findall(r"^ +(\d+) +(ac|var) +(\d+) +(\d+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  shown = [0, 2, 5, 7, 10]  # five of the 11 windows, evenly spaced
  assert [(int(r[0]), r[1], int(r[2])) for r in rows] == [
      (g, key, 4 + 15 + 4 * i) for g in range(2) for key in ("ac", "var") for i in shown], out
  got = np.array([[float(x) for x in r[3:]] for r in rows]).reshape(2, 2, 5, 4)
  taus = re.findall(r"^ +(\d+) +(ac|var) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), r[1]) for r in taus] == [(g, key) for g in range(2) for key in ("ac", "var")]
  got_tau = np.array([[float(x) for x in r[2:]] for r in taus]).reshape(2, 2, 2)
  # the restatement on the series the example downloaded
  z = np.load(saved)
  v, groups = z["series"], z["groups"]
  assert v.shape == (60, 1, 8) and np.isfinite(v).all() and groups.tolist() == [0] * 4 + [1] * 4
  assert (int(z["k0"]), int(z["k1"]), int(z["window"]), int(z["step"])) == (4, 60, 16, 4)
  want = WC.windows(v, 4, 60, 16, 4, 1, "linear")
  assert (want["nused"] == 11).all()
  order, start = STC.order_of(groups)
  for j, (key, i) in enumerate((("ac", 3), ("var", 2))):
    wc, ws = STC.group_stats(want["out"][i], order, start, (0.05, 0.95), 0, 11)
    assert (got[:, j, :, 0] == 4).all() and np.array_equal(wc[shown, 0, :].T, got[:, j, :, 0])
    assert np.array_equal(got[:, j, :, 1], ws[shown, 0, :, 0].T), out  # printed in full
    assert np.array_equal(got[:, j, :, 2], ws[shown, 0, :, 5].T)
    assert np.array_equal(got[:, j, :, 3], ws[shown, 0, :, 6].T)
    assert (got[:, j, :, 2] <= got[:, j, :, 1]).all() and (got[:, j, :, 1] <= got[:, j, :, 3]).all()
    conc, disc, tie, nfin = WC.kendall(want["out"][i], 0, 11)
    assert (nfin == 11).all()
    tau = WC.tau_b(conc[0], disc[0], tie[0])
    for g in range(2):
      t = tau[groups == g]
      assert got_tau[g, j].tolist() == [float(np.median(t)), float((t > 0).mean())], out
  assert (got[:, 1, :, 1] > 0).all() and (np.abs(got[:, 0, :, 1:]) <= 1).all()  # var, ac
  # the noise acts: the realisations of a set differ
  assert len(set(v[30, 0, :].tolist())) == 8
