"""CPU-side checks of the fused Jansen & Nadeau loop with implicit columns: the restatement's own
error (which sets the GPU tolerance), what the case table covers, that the float64 and long-double
restatements take the same decisions, and the kernel's resource usage (cross-compiled)."""
import os
import re
import subprocess

import numpy as np
import pytest

import jn2018_implicit_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_e_coupled_is_the_measured_restatement_error():
  err = J.measure_coupled_error()
  fresh = max(err.values())
  worst = max(err, key=err.get)
  print("E_COUPLED measured %.4e at %r; committed %.4e" % (fresh, worst, J.E_COUPLED))
  assert set(n for n, _ in err) == set(J.CASE_NAMES)
  assert set(k for _, k in err) == set(J.STEP_COUNTS)
  assert fresh <= J.E_COUPLED <= 2.0 * fresh


def test_case_table_covers_shapes_and_branches():
  cases = [J.get_case(n) for n in J.CASE_NAMES]
  assert {c["nz"] for c in cases} == {5, 63, 64, 65, 129, 200, 256}
  assert {c["ny"] for c in cases} == {51, 64, 65}
  assert {c["n"] for c in cases} == {1, 5}
  assert J.STEP_COUNTS == (1, 2, 7, 36)
  assert any((c["area"] != c["area"][:, :1]).any() for c in cases)
  for c in cases:  # beyond the explicit limit somewhere
    dz = np.diff(c["z"])
    r = max(c["kappa"].max(), c["kappaeff"].max()) * c["dt"] / dz.min() ** 2
    assert r > 0.5, (c["name"], r)
  basin, north = set(), set()
  sw_b = sw_n = first_step = 0
  for name in J.CASE_NAMES:
    _, trace = J.run(name)
    for t in trace:
      basin |= {b for b, _ in t["branches"]}
      north |= {n for _, n in t["branches"]}
    b, n = J.switches_after_step_1(name)
    sw_b += len(b)
    sw_n += len(n)
    first_step += int((trace[0]["ksel"] != J.get_case(name)["ksel0"]).sum())
  assert basin == {"south", "north", "none"} and north == {"inflow", "no inflow"}
  assert sw_b >= 1 and sw_n >= 1 and first_step >= 1
  # the launch-splitting test runs on these: every shape class has one
  sw = J.switching_cases()
  assert {J.get_case(c)["n"] for c in sw} == {1, 5}
  assert {(J.get_case(c)["nz"] + 63) // 64 for c in sw} == {1, 2, 3, 4}
  assert {J.get_case(c)["ny"] <= 64 for c in sw} == {True, False}


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_both_precisions_take_the_same_decisions(name):
  (r64, t64), (rld, tld) = J.run(name), J.run(name, np.longdouble)
  assert len(t64) == len(tld) == max(J.STEP_COUNTS)
  for s, (a, b) in enumerate(zip(t64, tld)):
    assert a["branches"] == b["branches"], (name, s)
    assert np.array_equal(a["ksel"], b["ksel"]), (name, s)
    assert np.array_equal(a["conv"], b["conv"]), (name, s)
    assert a["margin"] >= J.TIE_MARGIN and b["margin"] >= J.TIE_MARGIN, (name, s, a["margin"])
  for k in J.STEP_COUNTS:
    assert np.isfinite(r64[k]["b"]).all() and np.isfinite(r64[k]["bs_SO"]).all()
    assert np.array_equal(r64[k]["ksel"], rld[k]["ksel"])


def test_kernel_cross_compiles_without_scratch(tmp_path):
  """Every instantiation of k_jn2018_implicit for gfx950: 0 bytes of scratch (DESIGN.md section
  14 tabulates the registers)."""
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "jn2018_implicit.hip")
  p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "jn2018_implicit.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_jn2018_implicit\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  assert len(set(names)) == 8 and len(scratch) >= 8  # P in {1, 2, 3, 4} x SMALLNY
  assert all(s == 0 for s in scratch), list(zip(names, scratch))


def test_explicit_only_options_are_not_accepted():
  import pymoc_amd
  from pymoc_amd import configs
  assert issubclass(pymoc_amd.JN2018ImplicitEnsemble, pymoc_amd.JN2018Ensemble)
  cfg = configs.config5(N=2, nz=46, dt_days=30.)
  for kw in (dict(arith="contracted"), dict(lanes_per_col=64), dict(use_graph=True),
             dict(shared_coef=True), dict(fused_run=True), dict(split_lanes=True),
             dict(scheme="implicit")):
    with pytest.raises(TypeError):
      pymoc_amd.JN2018ImplicitEnsemble(cfg, **kw)
