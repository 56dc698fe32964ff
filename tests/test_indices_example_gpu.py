"""examples/overturning_indices.py runs end to end (tiny settings) and prints finite quantiles."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overturning_indices_example(gpu):
  p = subprocess.run([sys.executable, "examples/overturning_indices.py", "--members", "8",
                      "--years", "4", "--print-years", "2"],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  out = p.stdout
  assert re.search(r"8 members, 4 yearly samples of 5 indices: 1920 bytes on the device", out), out
  rows = re.findall(r"^  year +(\d+) +(\S+) +(\S+) +(\S+)$", out, flags=re.M)
  assert len(rows) == 6 * 3, out  # six series, years 0, 2 and 3: every member has every index
  assert [int(r[0]) for r in rows[:3]] == [0, 2, 3]
  q = np.array([[float(x) for x in r[1:]] for r in rows])
  assert np.isfinite(q).all(), out
  assert (q[:, 0] <= q[:, 1]).all() and (q[:, 1] <= q[:, 2]).all()
  assert (q[:3] > 0).all() and (q[3:9] < 0).all(), out  # an AMOC cell, at depth, above a sign change
  assert "non-finite" not in out
