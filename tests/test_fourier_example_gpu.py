"""examples/amoc_significance_fourier.py runs end to end at its smallest size and prints, per set
and indicator, a finite fraction of members with p_rising <= the level under both null models."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_significance_fourier_example(gpu):
  p = subprocess.run([sys.executable, "examples/amoc_significance_fourier.py", "--sets", "2",
                      "--realisations", "4", "--years", "60", "--spinup", "4", "--window", "16",
                      "--step", "4", "--nsur", "19", "--level", "0.1"],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 60 years; warming ramp over years 10-60; noise seed 2018" in out, out
  assert ("years 4-59: 11 windows of 16 years every 4 years, linear trend removed, lag 1; 19 "
          "surrogates per member and null model, seed 1955") in out, out
  assert "fraction of the members of a set with p_rising <= 0.1:" in out, out
  rows = re.findall(r"^ +(\d+) +(ac|var) +(\d+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), r[1], int(r[2])) for r in rows] == [
      (g, key, 4) for g in range(2) for key in ("ac", "var")], out
  for r in rows:
    tau, fracs = float(r[3]), (float(r[4]), float(r[5]))
    assert -1.0 <= tau <= 1.0 and all(f in (0.0, 0.25, 0.5, 0.75, 1.0) for f in fracs), r
  assert "every member has a tau and 19 surrogates with one under both null models: True" in out, out
