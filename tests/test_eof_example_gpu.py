"""examples/amoc_fingerprint.py runs end to end at its smallest size: it prints the pooled EOF of
every set, the trends of ac and var for pc1 and for the AMOC maximum side by side, the surrogate
test of both, and finds pc1 and the fit bit-identical to the restatement (tests/eof_cases.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amoc_fingerprint_example(gpu):
  p = subprocess.run([sys.executable, "examples/amoc_fingerprint.py", "--sets", "2",
                      "--realisations", "4", "--years", "60", "--spinup", "4", "--window", "20",
                      "--step", "4", "--sigma", "5", "--significance", "--nsur", "9"],
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  out = p.stdout
  assert p.returncode == 0, out + p.stderr
  assert "2 sets x 4 realisations, 60 years; warming ramp over years 10-60; noise seed 2018" in out, out
  assert ("Psi at 300, 600, 1000, 1500, 2000, 2800 m and the AMOC maximum below 500 m, years 4-59, "
          "Gaussian trend of sigma 5 years removed; windows of 20 years every 4 years") in out, out
  assert "restatement on the downloaded residual: pc1 and the fit every bit agrees" in out, out
  eofs = re.findall(r"^ +(\d+) +(\d+) +(\d\.\d{6}) +(\S+e\S+) +((?:[+-]\d\.\d{4} ?){6})$", out,
                    flags=re.M)
  assert [(int(r[0]), int(r[1])) for r in eofs] == [(0, 4 * 56), (1, 4 * 56)], out
  for r in eofs:
    loads = [float(x) for x in r[4].split()]
    assert max(loads) == 1.0 and 0.0 < float(r[2]) <= 1.0 and float(r[3]) >= 0.0, out
  assert re.search(r"^  set +ac pc1 +ac amoc +var pc1 +var amoc$", out, flags=re.M), out
  taus = re.findall(r"^ +(\d+) +(\S+e\S+) +(\S+e\S+) +(\S+e\S+) +(\S+e\S+)$", out, flags=re.M)
  assert [int(r[0]) for r in taus] == [0, 1], out
  assert all(-1.0 <= float(x) <= 1.0 for r in taus for x in r[1:]), out
  ps = re.findall(r"^ +(\d+) +(\d\.\d{4}) +(\d\.\d{4}) +(\d\.\d{4}) +(\d\.\d{4})$", out, flags=re.M)
  assert [int(r[0]) for r in ps] == [0, 1] and "AR(1)-surrogate test, 9 surrogates" in out, out
  assert all(0.0 <= float(x) <= 1.0 for r in ps for x in r[1:])
