"""The constructed Psi_SO members (tests/psi_so_cases.py) and their plain reference are right: the
C oracle is SciPy's brentq on them bit for bit, every branch and style is present where the grid can
hold it, the plain calc_Ekman / calc_GM agree with the oracle, and the derived bound for `linear`
levels holds for the one-solve formula in float64.  No GPU."""
import numpy as np
import pytest
from scipy import optimize

import oracle as O
import psi_so_cases as K

TOL_DIRECT = 1e-13  # tests/test_psi_so_gpu.py


def _oracle_ys(c, m):
  out = np.full(c.nz, np.nan)
  for i, v in enumerate(c.b[m]):
    if c.branches[m][i] != "nan":
      out[i], st = O.psi_so_ys(c.y, c.bs[m], v)
      assert st == 0, (m, i)
  return out


def _relerr(a, ref, keep):
  a, ref = a[keep], ref[keep]
  assert np.isfinite(ref).all() and np.isfinite(a).all()
  scale = np.abs(ref).max()
  return np.abs(a - ref).max() / (scale if scale > 0 else 1.)


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_oracle_is_scipy_brentq_on_these_members(nz, ny):
  c = K.case(nz, ny)
  seen = 0
  for m in range(c.n):
    if c.names[m] == "nan_bs":
      continue
    y, bs = c.y, c.bs[m]
    got = _oracle_ys(c, m)
    for i, v in enumerate(c.b[m]):
      if c.branches[m][i] == "nan":
        continue
      if v < np.min(bs):
        want = y[0] - 1e3
      elif v > bs[-1]:
        want = y[-1]
      else:
        want = optimize.brentq(lambda x: np.interp(x, y, bs) - v, y[np.argmin(bs)], y[-1])
      assert got[i] == want, (m, c.names[m], i, c.branches[m][i], got[i], want)
      seen += 1
  assert seen >= (c.n - 1) * (nz - 1) - nz


def test_every_branch_and_style_is_present():
  small, large = set(), set()
  for nz, ny in K.GRIDS:
    c = K.case(nz, ny)
    assert c.n == len(K.STYLES) + 1 and c.n % 4 != 0
    assert np.all(np.diff(c.y) > 0) and c.y[0] == 0. and np.all(np.diff(c.z) > 0) and c.z[-1] == 0.
    assert np.unique(np.diff(c.y)).size == ny - 1 or ny == 2
    for m, name in enumerate(c.names):
      assert name == (K.MEMBERS[m] if ny >= K.MIN_NY[K.MEMBERS[m]] else "rising")
    (small if ny <= 64 else large).update(c.names)
    have = set(b for row in c.branches if row is not None for b in row)
    want = set(K.BRANCHES) - ({"multi"} if ny < 3 else set())
    assert have == want, (nz, ny, want - have)
    # the styles are what they say
    for m, name in enumerate(c.names):
      bs = c.bs[m]
      if name == "nan_bs":
        assert np.isnan(bs).sum() == 1 and not np.isnan(bs[-1])
        continue
      k = int(np.argmin(bs))
      north = bs[k:]
      mono = K.monotone_north(bs)
      flat = np.nonzero(np.diff(north) == 0)[0]
      if name == "rising":
        assert np.all(np.diff(bs) > 0)
      elif name == "vee":
        assert 0 < k < ny - 2 and np.all(np.diff(north) > 0) and np.all(np.diff(bs[:k + 1]) < 0)
      elif name == "min_last_but_one":
        assert k == ny - 2
      elif name == "min_last":
        assert k == ny - 1
      elif name == "min_tie":
        assert np.count_nonzero(bs == bs[k]) == 2 and bs[k + 1] > bs[k] and bs[k + 2] == bs[k]
        assert not mono
      elif name == "bump":
        assert not mono and (ny <= 64 or np.any(np.diff(north)[:64] < 0))
      elif name == "late_bump":
        d = np.nonzero(np.diff(north) < 0)[0]
        assert d.size == 1 and d[0] >= 64
      elif name == "plateau_in":
        assert mono and flat.size == 2 and flat[0] > 0 and flat[1] == flat[0] + 1 and flat[1] + 1 < north.size - 1
      elif name == "plateau_north":
        assert mono and list(flat) == [north.size - 3, north.size - 2]
      elif name == "plateau_min":
        assert mono and list(flat) == [0, 1] and k > 0
      elif name == "const":
        assert np.all(bs == bs[0])
    assert c.multi() == c.members("min_tie", "bump", "late_bump")
    if nz >= 24:  # every special fits: one NaN and one +inf level in every member
      assert np.all(np.isnan(c.b).sum(axis=1) == 1) and np.all(np.isposinf(c.b).sum(axis=1) == 1)
  assert small == set(K.STYLES) - {"late_bump"} and large == set(K.STYLES)


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_plain_ekman_and_gm_match_the_oracle(nz, ny):
  c = K.case(nz, ny)
  for m in range(c.n):
    if c.names[m] == "nan_bs":
      continue
    ys = _oracle_ys(c, m)
    keep = ~np.isnan(ys)
    for kind in ("scalar", "array"):
      for opts in K.OPTIONS:
        ref = K.solve_at(ys, c, m, kind, opts)
        b = np.where(keep, c.b[m], c.bs[m][-1])  # (a NaN level: every level is on its own here)
        tau = c.tau(kind)[m]
        oPsi, oEk, oGM, st = O.psi_so_solve(c.z, c.y, b, c.bs[m], tau if kind == "array" else float(tau),
                                            KGM=c.KGM[m], **dict(K.PAR, **opts))
        assert st == 0
        what = (nz, ny, m, c.names[m], kind, sorted(opts))
        assert _relerr(ref["Psi_Ek"], oEk, keep) <= TOL_DIRECT, what
        assert _relerr(ref["Psi_GM"], oGM, keep) <= TOL_DIRECT, what
        assert _relerr(ref["Psi"], oPsi, keep) <= TOL_DIRECT, what
        assert ref["Psi"][0] == 0.


def test_derived_bound_holds_for_the_one_solve_formula():
  worst, count = 0., 0
  for nz, ny in K.GRIDS:
    c = K.case(nz, ny)
    for m in range(c.n):
      if c.branches[m] is None:
        continue
      for i, v in enumerate(c.b[m]):
        if c.branches[m][i] != "linear":
          continue
        root, off = K.exact_root(c.y, c.bs[m], v)
        r = K.bound_ratio(K.one_solve(c.y, c.bs[m], v), root, off)
        assert r <= 1., (nz, ny, m, i, r)
        worst = max(worst, r)
        count += 1
  assert count >= 3000 and worst > 0.
