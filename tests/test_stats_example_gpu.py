"""examples/ensemble_statistics.py runs end to end at a small size: the statistics it prints come
from SeriesStats, and its own comparison with the restatement on the downloaded series holds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ensemble_statistics_example(gpu):
  p = subprocess.run([sys.executable, "examples/ensemble_statistics.py", "--sets", "3",
                      "--realisations", "5", "--years", "16", "--print-years", "4", "--spinup", "2"],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "3 sets x 5 realisations, 16 years; noise seed 2018" in out, out
  assert "restatement on the downloaded series: every bit agrees" in out, out
  rows = re.findall(r"^ +(\d+) +(\d+) +(\d+) +(\S+) +(\S+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(r[0]), int(r[1])) for r in rows] == [(g, y) for g in range(3)
                                                    for y in (3, 7, 11, 15)], out
  v = np.array([[float(x) for x in r[2:]] for r in rows])
  assert (v[:, 0] == 5).all() and np.isfinite(v).all(), out  # every realisation finite
  assert (v[:, 1] > 0).all() and (v[:, 2] > 0).all(), out   # an AMOC cell, and a spread
  assert (v[:, 3] <= v[:, 4]).all() and (v[:, 4] <= v[:, 5]).all(), out  # 5 % <= 50 % <= 95 %
  members = re.findall(r"^ +(\d+) +(\d+) +(\S+) +(\S+) +(\S+) +(never|\d+)$", out, flags=re.M)
  assert [int(m[1]) for m in members] == list(range(15)), out
  assert all(float(m[2]) > 0 for m in members), out  # every member varies in time
