"""examples/amoc_spectrum.py runs end to end at a small size, and the group-mean spectrum and band
it prints equal the restatement (tests/spectra_cases.py, tests/stats_cases.py) on the series it
downloaded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spectra_cases as SC
import stats_cases as STC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_spectrum_example(gpu, tmp_path):
  from pymoc_amd.spectra import hann, twiddles
  saved = str(tmp_path / "series.npz")
  p = subprocess.run([sys.executable, "examples/amoc_spectrum.py", "--sets", "2",
                      "--realisations", "4", "--years", "40", "--spinup", "4", "--nperseg", "16",
                      "--save-series", saved],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 40 years; noise seed 2018" in out, out
  assert "Welch spectra of years 4-39: 3 segments of 16 years" in out, out
  assert "restatement on the downloaded series: every bit agrees" in out, out
  rows = re.findall(r"^ +(\d+) +(\S+) +(\d+) +(\S+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), float(r[1])) for r in rows] == [(g, round(f / 16.0, 6)) for g in range(2)
                                                      for f in range(9)], out
  got = np.array([[float(x) for x in r[2:]] for r in rows]).reshape(2, 9, 5)
  # the restatement on the series the example downloaded
  z = np.load(saved)
  v = z["series"]
  assert v.shape == (40, 2, 8) and np.isfinite(v).all()
  assert np.array_equal(z["window"], hann(16)) and (int(z["k0"]), int(z["k1"])) == (4, 40)
  want = SC.spectra(v, 4, 40, 16, 8, z["window"], "constant", ((0, 1),), float(z["scale"]),
                    twiddles(16))
  assert (want["nused"] == 3).all()
  order, start = STC.order_of(z["groups"])
  wc, ws = STC.group_stats(want["psd"], order, start, (0.05, 0.95), 0, 9)
  assert (got[:, :, 0] == 4).all() and np.array_equal(wc[:, 1, :].T, got[:, :, 0])
  assert np.array_equal(got[:, :, 1], ws[:, 1, :, 0].T), out  # the group mean, printed in full
  assert np.array_equal(got[:, :, 2], ws[:, 1, :, 5].T) and np.array_equal(got[:, :, 3], ws[:, 1, :, 6].T)
  assert (got[:, 1:, 1] > 0).all() and (got[:, :, 2] <= got[:, :, 1]).all()
  assert (got[:, :, 1] <= got[:, :, 3]).all()
  assert (got[:, :, 4] >= 0).all() and (got[:, :, 4] <= 1 + 1e-6).all(), out  # a coherence
  # the wind index is the white noise it records: it varies, and differs between realisations
  assert (v[:, 0, :].std(axis=0) > 0).all() and len(set(v[5, 0, :].tolist())) == 8
