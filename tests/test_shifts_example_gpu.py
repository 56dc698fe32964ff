"""examples/amoc_tipping_times.py runs end to end at its smallest size, prints per set the detected
fraction, the tipping years and the warnings with and without `until=`, and its self-check against
the restatement passes."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_tipping_times_example(gpu):
  p = subprocess.run([sys.executable, "examples/amoc_tipping_times.py", "--sets", "2",
                      "--realisations", "4", "--years", "60", "--spinup", "4", "--half", "8",
                      "--window", "16", "--step", "4", "--nsur", "19"],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 60 years; warming ramp over years 10-60; noise seed 2018" in out, out
  assert ("years 4-59: drops between two windows of 8 years, detectable from 3 pooled standard "
          "deviations; the trends of 16-year windows every 4 years, linear trend removed, lag 1; "
          "19 AR(1) surrogates per member, seed 1955") in out, out
  tips = re.findall(r"^ +(\d+) +(\d+) +(\S+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), int(r[1])) for r in tips] == [(0, 4), (1, 4)], out
  for r in tips:
    assert float(r[2]) in (0.0, 0.25, 0.5, 0.75, 1.0), r
    if float(r[2]) > 0.0:
      assert 4 + 8 <= float(r[4]) <= float(r[3]) <= float(r[5]) <= 59 - 7, r
  rows = re.findall(r"^ +(\d+) +(ac|var) +(\S+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), r[1]) for r in rows] == [(g, key) for g in range(2) for key in ("ac", "var")], out
  for r in rows:
    assert -1.0 <= float(r[3]) <= 1.0 and float(r[5]) in (0.0, 0.25, 0.5, 0.75, 1.0), r  # plain
  assert "restatement on the downloaded series: every number agrees" in out, out
