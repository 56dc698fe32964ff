"""pm_div2_proven (the host proof behind PM_COLS_DIV2_GRID / PM_COL_DIV2_AREA) against a pure-Python
restatement in exact rationals: the same candidate numerators and the same verdict per denominator."""
import ctypes as C
import math
from fractions import Fraction as F

import numpy as np

from pymoc_amd import configs
from pymoc_amd._lib import check, lib


def _fl(x):
  return float(x)  # (int / int true division rounds a Fraction correctly)


def _div2_reference(d):
  """The candidate numerator mantissas of d (quotient within 4 / (2 D) ulp of a rounding midpoint)
  and whether  yh = RN(1/d); yl = RN((1 - d yh) / d); q = RN(a yh + RN(a yl))  is the correctly
  rounded quotient on every one of them, both signs."""
  m, _ = math.frexp(abs(d))
  D = int(m * 2**53)
  dm = float(D)
  v = (D & -D).bit_length() - 1
  Dp = D >> v
  cands = set()
  if v < 3 and Dp > 1:
    for t in (0, 1):
      sh = 53 + t
      for N in range(-4, 5):
        if N == 0 or N % (1 << v):
          continue
        A0 = ((N >> v) * pow((1 << (sh - v)) % Dp, -1, Dp)) % Dp
        lo, hi = (D, 1 << 53) if t == 0 else (1 << 52, D)
        A = A0 + ((lo - A0 + Dp - 1) // Dp) * Dp
        while A < hi:
          q, r = divmod(A * (1 << sh) - N, D)
          if r == 0 and q % 2 == 1:
            cands.add(A)
          A += Dp
  yh = _fl(F(1) / F(dm))
  e = F(1) - F(dm) * F(yh)
  assert _fl(e) == e  # the residual of the reciprocal is exact in one fma
  yl = _fl(e / F(dm))
  ok = True
  for A in cands:
    for a in (float(A), -float(A)):
      u = _fl(F(a) * F(yl))
      if _fl(F(a) * F(yh) + F(u)) != _fl(F(a) / F(dm)):
        ok = False
  return ok, len(cands)


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
      got, ref = _library(d), _div2_reference(float(d))
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
