"""examples/twobasin_equilibrium.py runs end to end (tiny settings), explicit and implicit."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [(), ("--implicit",)], ids=["explicit", "implicit"])
def test_twobasin_equilibrium_example(gpu, extra):
  p = subprocess.run([sys.executable, "examples/twobasin_equilibrium.py", "--members", "4", "--nz",
                      "17", "--ny", "9", "--steps", "97", "--check-every", "24", "--tol", "1e30",
                      "--consecutive", "1"] + list(extra),
                     cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  out = p.stdout
  m = re.search(r"4 members, (\w+) columns, cap 97 steps .* (\d+) converged, (\d+) non-finite, "
                r"(\d+) capped", out)
  assert m, out
  assert m.group(1) == ("implicit" if extra else "explicit")
  assert [int(m.group(i)) for i in (2, 3, 4)] == [4, 0, 0], out  # tol 1e30: all at the first check
  s = re.search(r"member-steps: (\d+) of (\d+) \(\d+\.\d%\), (\d+) saved", out)
  # (a check's count is read after the next interval is enqueued: one interval past step 25)
  assert s and int(s.group(1)) == 4 * 49 and int(s.group(2)) == 4 * 97, out
  assert int(s.group(3)) == 4 * 97 - 4 * 49
  assert re.search(r"retirement years: min 2  median 2  max 2", out), out
