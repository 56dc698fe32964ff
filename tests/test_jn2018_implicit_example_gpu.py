"""examples/jn2018_implicit.py runs end to end (short settings)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jn2018_implicit_example(gpu):
  p = subprocess.run([sys.executable, "examples/jn2018_implicit.py", "--members", "4", "--years",
                      "4"], cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  out = p.stdout
  m = re.search(r"implicit: (\d+) steps of 30 d, (\d+) non-finite members", out)
  assert m and int(m.group(1)) == 48 and int(m.group(2)) == 0, out
  assert re.search(r"explicit: 144 steps of 10 d, \d+ non-finite members", out), out
  r = re.search(r"kappa dt / dz\^2 = (\d+\.\d+) at 30 d, (\d+\.\d+) at 10 d", out)
  assert r and float(r.group(1)) > 0.5 >= float(r.group(2)), out  # beyond / within the explicit limit
  for f in ("b_basin", "b_north", "bs_SO", "Psi"):
    assert re.search(r"of %s\s+(\d\.\d\de[-+]\d\d|nan)" % f, out), (f, out)
