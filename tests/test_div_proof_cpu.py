"""pm_div3_proven and pm_div2_proven (the host proofs behind PM_COLS_DIV3_PROVEN and PM_COLS_DIV2_GRID /
PM_COL_DIV2_AREA) against a pure-Python restatement in exact rationals (tests/div_proof_reference.py):
the same candidate numerators and the same verdict per denominator."""
import ctypes as C

import numpy as np

from div_proof_reference import div2_reference, div3_reference
from pymoc_amd import configs
from pymoc_amd._lib import check, lib
from pymoc_amd.columns import div3_proven


def _library(d):
  arr = np.array([float(d)])
  ok, nc = np.full(1, -1, dtype=np.int32), C.c_int64(-1)
  check(lib.pm_div2_proven(arr.ctypes.data, 1, ok.ctypes.data, C.byref(nc)))
  return bool(ok[0]), nc.value


def _grid_denominators(z):
  dz = np.diff(z)
  return list(np.unique(dz)) + list(np.unique(0.5 * (dz[1:] + dz[:-1])))


def test_div2_proof_matches_its_restatement():
  """config2(N=1024)'s grid spacings and Areas, 2000 random mantissas and the mantissas next to 1 and
  2: same candidates, same verdict.  The 2-instruction form has no correction step, so the set holds
  failing denominators as well as passing ones (0 < failures < n), config 2's Areas among them; the
  grid spacings have no candidate at all (>= 3 trailing zero bits of the mantissa)."""
  c = configs.config2(N=1024)
  grid = _grid_denominators(c["z"])
  areas = list(c["Area"][:, 0])
  rng = np.random.default_rng(7)
  rnd = list(rng.uniform(1, 2, 2000) * 2.0**rng.integers(-30, 30, 2000))
  edge = [1.0 + k * 2.0**-52 for k in range(1, 40)] + [2.0 - k * 2.0**-52 for k in range(1, 40)]
  fails = {}
  for name, ds in (("grid", grid), ("areas", areas), ("random", rnd), ("edge", edge)):
    fails[name] = 0
    for d in ds:
      got, ref = _library(d), div2_reference(float(d))
      assert got == ref, (name, float(d).hex(), got, ref)
      fails[name] += not got[0]
      if name == "grid":
        assert got == (True, 0), (float(d).hex(), got)
  print("denominators failing the 2-instruction proof:", fails)
  assert 0 < fails["areas"] < len(areas)
  n = len(grid) + len(areas) + len(rnd) + len(edge)
  assert 0 < sum(fails.values()) < n
  assert fails["grid"] == 0


def test_div2_proof_rejects_what_it_cannot_scale():
  """Zero, subnormal and non-finite denominators are not proven; powers of two are (yl = 0)."""
  for bad in (0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.0**-1060):
    assert _library(bad) == (False, 0)
  for d in (1.0, -4.0, 2.0**-1000, 2.0**1000, 1.5, -3.0):
    assert _library(d) == (True, 0)
  ok = np.zeros(3, dtype=np.int32)
  arr = np.array([1.5, 0.0, 40.0])
  check(lib.pm_div2_proven(arr.ctypes.data, 3, ok.ctypes.data, None))
  assert list(ok) == [1, 0, 1]


def test_div3_proof_matches_its_restatement():
  """pm_div3_proven (host function behind PM_COLS_DIV3_PROVEN): the same candidate numerators and
  the same verdict as an exact-rational restatement, for uniform mantissas, mantissas next to 1 and
  2, mantissas with trailing zeros and the grid spacings of BASELINE's grids; zero, subnormal and
  non-finite denominators are not proven."""
  rng = np.random.default_rng(5)
  ds = list(rng.uniform(1, 2, 150) * 2.0**rng.integers(-30, 30, 150))
  ds += [1.0 + k * 2.0**-52 for k in range(1, 40)] + [2.0 - k * 2.0**-52 for k in range(1, 40)]
  ds += [float((np.float64(x).view(np.uint64) & ~np.uint64(1)).view(np.float64)) for x in rng.uniform(1, 2, 40)]
  ds += [float((np.float64(x).view(np.uint64) & ~np.uint64(3)).view(np.float64)) for x in rng.uniform(1, 2, 40)]
  ds += [3.0, 6e13, 1e-7, 40.0, 0.1, 86400.0 * 30]
  for mk in (configs.config2, configs.config5):
    ds += _grid_denominators(mk(N=2)["z"])
  for d in ds:
    d = float(d)
    ok, nc = C.c_int32(-1), C.c_int64(-1)
    arr = np.array([d])
    check(lib.pm_div3_proven(arr.ctypes.data, 1, C.byref(ok), C.byref(nc)))
    rok, rnc = div3_reference(d)
    assert (bool(ok.value), nc.value) == (rok, rnc), (d, ok.value, nc.value, rok, rnc)
    assert ok.value == 1  # (no denominator is known to fail; the kernels still ask for the proof)
  for bad in (0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.0**-1060):
    assert not div3_proven([1.5, bad])
  assert div3_proven([]) and div3_proven([1.5, -3.0, 2.0**-1000, 2.0**1000])
