"""The reference side of the K7 launch table (tests/equi_column_cases.py), no device: the
restated Newton loop of `oracle.equi_column.newton_pass` IS `_bvp.solve_newton`, the pass chained
with solve_bvp's mesh refinement IS `solve_bvp`, every row of the table is decisive (so the GPU
file may demand equal iteration and insertion counts), and the entry point's argument checks."""
import ctypes as C

import numpy as np
from scipy.integrate import _bvp

import equi_column_cases as T
from oracle import equi_column as EO
from pymoc_amd import configs


def test_newton_pass_is_solve_newton_bitwise():
  """y, p, singular of the restated loop against SciPy's own, same callbacks, every row."""
  for c in T.CASES + [T.NAN_CASE]:
    fun, bc, col_fun, jac, k = EO.newton_system(c.q, c.x)
    p0 = np.array([c.p]) if k else np.array([])
    y, p, sing = _bvp.solve_newton(4, c.m, np.diff(c.x), col_fun, bc, jac, c.y.copy(), p0, None,
                                   T.TOL, T.TOL)
    r = T.reference(c) if c is not T.NAN_CASE else EO.newton_pass(c.q, c.x, c.y, c.p, T.TOL)
    assert r[2] == sing, c
    assert np.array_equal(r[0], y, equal_nan=True) and np.array_equal(r[1], p, equal_nan=True), c
    rec = r[7]
    assert 1 <= rec["njev"] <= 4 and rec["njev"] <= rec["niter"] <= 8, c
    assert len(rec["alphas"]) == rec["niter"] - (1 if sing else 0), c


def test_chained_passes_are_solve_bvp():
  """newton_pass + `_bvp.modify_mesh` + the spline transfer, looped as solve_bvp loops them:
  the final mesh, solution and depth of `EO.solve`, bitwise, on three golden problems (H unknown
  with scalar and with array profiles, H given with an array kappa)."""
  cases = configs.equi_column_cases()
  for name in ("Hfree_const", "H500_kappa_arr", "Bint1"):
    q = EO.problem(**cases[name])
    r = EO.solve(q)
    x, y, p = T.guess(q, q["nz"])
    hfree = q["H"] is None
    for iteration in range(1, 11):
      y, pp, sing, yp, rms, nadd, info, _ = EO.newton_pass(q, x, y, p if hfree else None, T.TOL)
      p = pp[0] if hfree else None
      assert not sing
      if nadd == 0:
        break
      i1, = np.nonzero((rms > T.TOL) & (rms < 100 * T.TOL))
      i2, = np.nonzero(rms >= 100 * T.TOL)
      xn = _bvp.modify_mesh(x, i1, i2)
      y, x = _bvp.create_spline(y, yp, x, np.diff(x))(xn), xn
    assert r["status"] == 0 and info[1] <= T.TOL and iteration == r["niter"], name
    assert np.array_equal(x, r["x"]) and np.array_equal(y, r["y"]), name
    assert np.array_equal(yp, r["yp"]) and (p if hfree else q["H"]) == r["H"], name


def test_every_row_is_decisive():
  """No row may sit on a decision: every line-search test `cost_new < (1 - 2 alpha sigma) cost`
  is off by >= 1e-6 of cost, every stopping test by >= 1e-6, and every interval's rms is a
  relative 1e-6 or more away from tol and from 100 tol.  (The kernel's rounding differs from
  SciPy's by ~1e-10 at most, so its decisions must then be SciPy's.)  No row is exempt: one that
  fails gets another input in the table."""
  for c in T.CASES:
    rms, rec = T.reference(c)[4], T.reference(c)[7]
    assert np.isfinite(rms).all(), c
    assert min(rec["margins"] + [np.inf]) >= 1e-6, (c, rec["margins"])
    assert min(rec["stop_margins"] + [np.inf]) >= 1e-6, (c, rec["stop_margins"])
    for thr in (T.TOL, 100 * T.TOL):
      assert np.min(np.abs(rms - thr)) >= 1e-6 * thr, (c, thr)


def test_table_reaches_what_it_is_for():
  """The sizes, forms, starts and endings the table exists for are all in it."""
  refs = {c.name: T.reference(c) for c in T.CASES}
  for form in range(4):  # HFREE x HAS_BBOT, each at every size
    ms = {c.m for c in T.CASES if c.flags == form}
    assert set(T.SIZES) <= ms, (form, ms)
  assert {3, 65, 130} <= {c.m for c in T.CASES if c.mmax == c.m}
  for fl in (T.KAPPA_ARRAY, T.PSI_ARRAY, T.KAPPA_ARRAY | T.PSI_ARRAY):
    for nzg in (2, 80):
      assert any(c.flags & 12 == fl and c.q["z"].size == nzg for c in T.CASES if c.flags & 12)
  deep = [c for c in T.CASES if c.flags & 12 and c.hfree and -c.p < c.q["z"][0]]
  assert {c.q["z"].size for c in deep} == {2, 80}
  assert any(np.ptp(np.diff(c.x)) > 1e-3 for c in T.CASES)  # meshes insertion left non-uniform
  ends = {(r[2], r[7]["converged"], r[7]["njev"] == 4, r[7]["niter"] == 8) for r in refs.values()}
  assert (True, False, False, False) in ends    # singular at the first factorisation
  assert (False, True, False, False) in ends    # the stopping rule
  assert (False, False, True, False) in ends    # four Jacobians, unconverged
  assert (False, False, False, True) in ends    # eight iterations on fewer Jacobians
  assert any(r[7]["niter"] == 1 and r[7]["converged"] for r in refs.values())
  assert {a for r in refs.values() for a in r[7]["alphas"]} == {1, 0.5, 0.25, 0.125, 0.0625}
  assert any(r[5] == 0 for r in refs.values()) and any(r[5] > 128 for r in refs.values())
  for name, rows, active, nzg in T.BATCHES:
    cs = [T.batch_case(r) for r in rows]
    assert max(c.m for c in cs) == T.BATCH_MMAX and len({c.m for c in cs}) > 3, name
    assert len({c.flags for c in cs}) > 3 and "singular_m80" in rows, name
    assert all(c.q["z"].size == nzg for c in cs if c.flags & 12), name
  assert 0 in T.BATCHES[1][2] and T.NAN_CASE.name in T.BATCHES[1][1]


def test_newton_entry_rejects_bad_arguments_before_touching_the_device():
  """pm_equi_column_newton's checks: a NULL struct, every required pointer NULL in turn, mmax 2
  and 4097, tol <= 0, a profile grid without zg -- PM_EINVAL each, before any launch (the
  stand-in pointers are never dereferenced); n = 0 is accepted."""
  from pymoc_amd import _lib
  L = _lib.lib
  A = 0x10000
  required = ("m", "x", "y", "yp", "p", "f", "A", "bs", "bb", "kappa", "flags", "scratch")

  def desc(**kw):
    d = _lib.pm_equi_column()
    d.n, d.nzg, d.mmax, d.tol = 2, 0, 64, 1e-3
    for k in required:
      setattr(d, k, A)
    for k, v in kw.items():
      setattr(d, k, v)
    return d

  def refused(d, word):
    rc = L.pm_equi_column_newton(C.byref(d), None)
    return rc == _lib.PM_EINVAL and word in L.pm_last_error().decode()

  assert L.pm_equi_column_newton(None, None) == _lib.PM_EINVAL
  assert "NULL" in L.pm_last_error().decode()
  for k in required:
    assert refused(desc(**{k: None}), "NULL"), k
  assert refused(desc(mmax=2), "mmax") and refused(desc(mmax=4097), "mmax")
  assert refused(desc(n=-1), "n=")
  assert refused(desc(tol=0.0), "tol") and refused(desc(tol=-1e-3), "tol")
  assert refused(desc(tol=float("nan")), "tol")
  assert refused(desc(nzg=80), "zg")
  assert L.pm_equi_column_newton(C.byref(desc(n=0, m=None, scratch=None)), None) == _lib.PM_OK
