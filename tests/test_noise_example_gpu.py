"""examples/stochastic_amoc.py runs end to end (tiny settings): identical members are driven apart
by the noise, and the printed rows are reproduced by the seed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
  p = subprocess.run([sys.executable, "examples/stochastic_amoc.py", "--members", "8", "--years", "6",
                      "--print-years", "2"] + list(extra),
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  return p.stdout


def test_stochastic_amoc_example(gpu):
  out = _run()
  assert re.search(r"8 identical members, 6 years; noise seed 2018", out), out
  rows = re.findall(r"^  years +(\d+)- *(\d+) +(\S+) +(\S+)$", out, flags=re.M)
  assert [(int(a), int(b)) for a, b, _, _ in rows] == [(0, 1), (2, 3), (4, 5)], out
  v = np.array([[float(x) for x in r[2:]] for r in rows])
  assert np.isfinite(v).all() and (v[:, 0] > 0).all(), out  # an AMOC cell in every block
  assert (v[1:, 1] > 0).all(), out  # identical members have been driven apart
  assert "non-finite" not in out
  # the seed alone decides the run; another seed gives another one
  assert _run() == out
  assert _run("--seed", "7") != out
