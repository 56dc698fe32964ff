"""The launch table of `pm_equi_column_newton` (K7): every row is ONE launch of one member -- a
problem `q` (oracle.equi_column.problem), a mesh `x`, a start `(y, p)` and the row length `mmax`
of the member's buffers -- plus the batches that put several rows into one launch.  The CPU file
(test_equi_column_cpu.py) pins the reference pass on every row and requires every row to be
decisive; the GPU file (test_equi_column_gpu.py) runs every row through the kernel.

Sizes are the smallest that reach the code: m = 3 (N = 12: the 6-row window pre-load meets a
12-row system; the last five pivot columns are half the system), 4, 5; m - 1 = 63 / 64 / 65
intervals (the residual loop's second ballot pass starts at 65) and 128 / 129 (the third);
m = mmax (no padding at all).  Starts: the class's default guess (damped, mostly unconverged
launches), the reference pass's own output (converged launches of one or two iterations) and that
output carried by the spline to the mesh solve_bvp's insertion makes of it (non-uniform)."""
import functools

import numpy as np
from scipy.integrate import _bvp

from oracle import equi_column as EO

TOL = 1e-3
HFREE, HAS_BBOT, KAPPA_ARRAY, PSI_ARRAY = 1, 2, 4, 8  # PM_EQ_* of include/pymoc_hip.h

Z80 = np.linspace(-4000., 0., 80)
Z2 = np.array([-4000., 0.])
PROFILES = {
    80: dict(z=Z80, kappa=np.linspace(1e-5, 4e-5, 80),
             psi_so=3e6 * np.sin(-np.pi * np.maximum(Z80, -2000.) / 2000.)**2),
    2: dict(z=Z2, kappa=np.array([1e-5, 4e-5]), psi_so=np.array([1.5e6, 0.])),
}

# the four forms HFREE x HAS_BBOT (scalar kappa, no psi_so)
FORMS = {
    "free_bint": dict(B_int=3e3, A=2e14, kappa=3e-5),
    "free_bbot": dict(B_int=None, b_bot=-1e-3, A=1e14, kappa=5e-5),
    "given_bint": dict(B_int=3e3, A=2e14, kappa=3e-5, H=800.0),
    "given_bbot": dict(B_int=None, b_bot=2e-3, A=1e14, kappa=5e-5, H=3000.0, b_s=0.02, f=1e-4),
}
SIZES = (3, 4, 5, 64, 65, 66, 129, 130)


class Case(object):
  """One launch of one member."""

  def __init__(self, name, q, x, y, p, mmax=None):
    self.name, self.q = name, q
    self.x, self.y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    self.hfree = q["H"] is None
    self.p = float(p if self.hfree else q["H"])  # the kernel's p: the start of H, or H itself
    self.m = self.x.size
    self.mmax = self.m + 5 if mmax is None else mmax  # 5: rows neither aligned nor a wave multiple
    self.flags = flags(q)

  def __repr__(self):
    return self.name


def flags(q):
  return ((HFREE if q["H"] is None else 0) | (HAS_BBOT if q["b_bot"] is not None else 0) |
          (KAPPA_ARRAY if isinstance(q["kappa"], np.ndarray) else 0) |
          (PSI_ARRAY if isinstance(q["psi_so"], np.ndarray) else 0))


def member(q, nzg):
  """The kernel's per-member inputs as EquiColumnBatch forms them (pymoc_amd/equi_column.py)."""
  f = q["f"]
  d = dict(f=f, A=q["A"], bs=-q["b_s"] / f**2,
           bb=-q["b_bot"] / f**2 if q["b_bot"] is not None else q["B_int"],
           kappa=0.0, kappa_z=np.zeros(nzg), dkappa_z=np.zeros(nzg), psi_z=np.zeros(nzg))
  if isinstance(q["kappa"], np.ndarray):
    d["kappa_z"], d["dkappa_z"] = q["kappa"], np.gradient(q["kappa"], q["z"])
  else:
    d["kappa"] = q["kappa"]
  if isinstance(q["psi_so"], np.ndarray):
    d["psi_z"] = q["psi_so"]
  return d


def guess(q, m):
  """Equi_Column's default initial guess on a uniform mesh of m nodes (equi_column.py:187-213)."""
  bz = EO.functions(q)[4]
  y = np.zeros((4, m))
  y[0] = 1.0
  y[3] = -100.0 if q["b_bot"] is not None else -bz(1500.)
  return np.linspace(-1, 0, m), y, q["H_guess"]


@functools.lru_cache(maxsize=None)
def _reference(name):
  c = BY_NAME[name]
  return EO.newton_pass(c.q, c.x, c.y, c.p if c.hfree else None, TOL)


def reference(case):
  """`EO.newton_pass` of a row: computed once, shared by every test, never written to."""
  return _reference(case.name)


def _from_guess(name, q, m, mmax=None, H0=None):
  x, y, p = guess(q, m)
  return Case(name, q, x, y, p if H0 is None else H0, mmax)


def _after(name, first, refine, mmax=None):
  """The row that starts where the reference pass of `first` ends: on the same mesh, or on the
  mesh solve_bvp makes of it, with the iterate carried there by the spline."""
  y, p, _, yp, rms, nadd = EO.newton_pass(first.q, first.x, first.y,
                                         first.p if first.hfree else None, TOL)[:6]
  x = first.x
  if refine:
    assert nadd > 0, name
    i1, = np.nonzero((rms > TOL) & (rms < 100 * TOL))
    i2, = np.nonzero(rms >= 100 * TOL)
    xn = _bvp.modify_mesh(x, i1, i2)
    y, x = _bvp.create_spline(y, yp, x, np.diff(x))(xn), xn
  return Case(name, first.q, x, y, p[0] if first.hfree else None, mmax)


def _build():
  rows = []
  for form, kw in FORMS.items():
    q = EO.problem(**kw)
    for m in SIZES:
      rows.append(_from_guess("%s_m%d" % (form, m), q, m))
  by = {c.name: c for c in rows}
  # m = mmax: rows without padding (an odd and an even row length)
  rows.append(_from_guess("free_bint_m65_full", EO.problem(**FORMS["free_bint"]), 65, mmax=65))
  rows.append(_from_guess("given_bbot_m130_full", EO.problem(**FORMS["given_bbot"]), 130, mmax=130))
  rows.append(_from_guess("given_bint_m3_full", EO.problem(**FORMS["given_bint"]), 3, mmax=3))
  # array profiles on nzg = 80 / 2 levels; H0 = 6000 starts with z* H below zg[0] = -4000
  for nzg, pr in PROFILES.items():
    both = dict(z=pr["z"], kappa=pr["kappa"], psi_so=pr["psi_so"], A=2e14)
    rows.append(_from_guess("arr%d_free_m5" % nzg, EO.problem(B_int=3e3, **both), 5))
    rows.append(_from_guess("arr%d_free_deep_m66" % nzg, EO.problem(B_int=3e3, **both), 66, H0=6000.))
    rows.append(_from_guess("arr%d_given_bbot_m65" % nzg,
                            EO.problem(B_int=None, b_bot=-1e-3, H=1200., **both), 65))
    rows.append(_from_guess("arr%d_kappa_only_m4" % nzg,
                            EO.problem(B_int=3e3, A=2e14, z=pr["z"], kappa=pr["kappa"], H=5000.), 4))
    rows.append(_from_guess("arr%d_psi_only_m64" % nzg,
                            EO.problem(B_int=3e3, A=2e14, z=pr["z"], kappa=3e-5,
                                       psi_so=pr["psi_so"]), 64))
  # starts at the reference pass's own output, same mesh and refined mesh
  for first in ("free_bint_m3", "free_bint_m65", "free_bbot_m4", "given_bint_m5", "given_bint_m64",
                "given_bbot_m129"):
    rows.append(_after(first + "_again", by[first], False))
  rows.append(_after("arr80_free_m5_again", {c.name: c for c in rows}["arr80_free_m5"], False))
  by = {c.name: c for c in rows}
  for first in ("free_bint_m5", "free_bint_m64", "given_bint_m4", "given_bbot_m66",
                "arr80_given_bbot_m65"):
    rows.append(_after(first + "_refined", by[first], True))
  # the existing singular problem (test_equi_column_failure_modes_match_solve_bvp)
  sing = EO.problem(z=Z80, A=2e14, kappa=3e-5, H=500.0, B_int=None, b_bot=4e3)
  rows.append(_from_guess("singular_m80", sing, 80))
  return rows


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- batches: (name, [row names], active, nzg).  Every member keeps its own mesh; mmax = 130.
# `nan_bint` exists only here: a NaN problem has no path to compare, it must not disturb others.
_nan = EO.problem(**dict(FORMS["free_bint"], B_int=np.nan))
NAN_CASE = _from_guess("nan_bint_m12", _nan, 12)
BATCH_MMAX = 130
BATCHES = [
    ("mixed", ["free_bint_m3", "given_bbot_m130", "arr80_free_deep_m66", "free_bbot_m4",
               "arr80_given_bbot_m65", "given_bint_m129", "singular_m80", "free_bint_m65",
               "arr80_kappa_only_m4", "given_bint_m5_again", "free_bint_m64_refined"],
     [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], 80),
    ("inactive_and_nan", ["given_bint_m66", "free_bint_m5", "nan_bint_m12", "singular_m80",
                          "free_bbot_m130", "arr2_free_m5"],
     [1, 0, 1, 1, 1, 1], 2),
]


def batch_case(name):
  return NAN_CASE if name == NAN_CASE.name else BY_NAME[name]
