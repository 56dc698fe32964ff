"""K6 (`k_column_equi_pass`) one launch at a time: `pm_column_equi_pass` on the table of
tests/equi_pass_cases.py against the NumPy restatement of the kernel, bit for bit.  Every output
buffer is pre-filled with a sentinel NaN pattern, so what a launch leaves alone is visible."""
import ctypes as C

import numpy as np
import pytest

import equi_pass_cases as T
import oracle as O
from oracle import drivers
from pymoc_amd.equilibrium import insert_nodes

pytestmark = pytest.mark.gpu

NADD_SENTINEL = -7
OUTPUTS = ("y", "rms", "nadd", "b", "bz")


def _untouched(a):
  """Every entry still holds the sentinel."""
  a = np.ascontiguousarray(a)
  if a.dtype == np.int32:
    return bool((a == NADD_SENTINEL).all())
  return bool((a.view(np.uint64) == T.SENTINEL).all())


class _Rig(object):

  def __init__(self, gpu):
    from pymoc_amd import _lib
    from pymoc_amd.device import DeviceArray
    self.L, self.DA = _lib, DeviceArray
    self.single = {}

  def launch(self, cases, mmax, path, tol, active=None, ends_only=False, omit=()):
    """One launch.  omit: descriptor fields passed as NULL.  -> host copies of the outputs (those
    that were not omitted), as the launch left the sentinel-filled buffers."""
    L, DA = self.L, self.DA
    h, nz = T.pack(cases, mmax, path, ends_only)
    n = len(cases)
    if active is not None:
      h["active"] = np.asarray(active, np.int32)
    out = dict(y=T.sentinel((n, 2, mmax)), rms=T.sentinel((n, mmax)),
               nadd=np.full(n, NADD_SENTINEL, np.int32), b=T.sentinel((n, nz)),
               bz=T.sentinel((n, nz)))
    dev = {k: DA.from_host(v) for k, v in list(h.items()) + list(out.items())}
    d = L.pm_column_equi()
    d.n, d.nz, d.mmax, d.reserved, d.tol = n, nz, mmax, 0, tol
    for k, v in dev.items():
      setattr(d, k, None if k in omit else v.ptr)
    for k in ("wA", "wA_z", "z", "active"):
      if k not in dev:
        setattr(d, k, None)
    rc = L.lib.pm_column_equi_pass(C.byref(d), None)
    assert rc == L.PM_OK, L.lib.pm_last_error().decode()
    res = {k: dev[k].download() for k in OUTPUTS}
    for k in OUTPUTS:  # an output that was not passed can not have been written
      if k in omit:
        assert _untouched(res[k]), k
    return res

  def alone(self, name, path):
    """The single-member launch of a row at its own mmax and tol, launched once."""
    key = (name, path)
    if key not in self.single:
      c = T.BY_NAME[name]
      self.single[key] = self.launch([c], c.mmax, path, c.tol)
    return self.single[key]


@pytest.fixture(scope="module")
def rig(gpu):
  return _Rig(gpu)


def _member(res, i, m):
  """A member's own part of every output."""
  return dict(y=res["y"][i][:, :m], rms=res["rms"][i][:m - 1], nadd=int(res["nadd"][i]),
              b=res["b"][i], bz=res["bz"][i])


def _padding_untouched(res, i, m):
  return _untouched(res["y"][i][:, m:]) and _untouched(res["rms"][i][m - 1:])


def _check_member(c, o, tol, ref=None):
  """A member's outputs against the restatement: y, v, b, bz bit for bit; rms bit for bit the
  restatement's residual of the device's OWN y; nadd the host rule on the device's own rms."""
  y, rms, nadd, b, bz = c.restate(tol=tol) if ref is None else ref
  assert T.same(o["y"], y), (c, np.nonzero(T.bits(o["y"]) != T.bits(y)))
  with np.errstate(all="ignore"):  # (the non-finite rows)
    own = T.residuals(c.x, c.c4, o["y"][0], o["y"][1])
  assert T.same(o["rms"], own), (c, np.nonzero(T.bits(o["rms"]) != T.bits(own)))
  assert T.same(o["rms"], rms), c  # (follows from the two above; says so if they ever part)
  assert o["nadd"] == int(T.classes(o["rms"], tol).sum()) == nadd, (c, o["nadd"], nadd)
  assert o["nadd"] == insert_nodes(c.x, o["rms"], tol).size - c.m, c


@pytest.mark.parametrize("c", T.CASES, ids=repr)
def test_row_is_the_restatement_bit_for_bit(rig, c):
  """Every row of the table alone in a launch at its own mmax.  A row with a grid is launched
  twice, wA_z interpolated on the device and wA tables of np.interp's values: the two launches
  agree bit for bit.  The padding of y and rms keeps the sentinel."""
  res = rig.alone(c.name, c.path)
  o = _member(res, 0, c.m)
  _check_member(c, o, c.tol, T.reference(c.name))
  assert T.same(o["b"], T.reference(c.name)[3]) and T.same(o["bz"], T.reference(c.name)[4]), c
  assert T.same(o["b"], o["y"][0, c.zidx]) and T.same(o["bz"], o["y"][1, c.zidx]), c
  assert _padding_untouched(res, 0, c.m), c
  if c.path == "interp":
    tab = rig.alone(c.name, "table")
    for k in OUTPUTS:
      assert np.array_equal(res[k], tab[k]) if k == "nadd" else T.same(res[k], tab[k]), (c, k)
    assert _padding_untouched(tab, 0, c.m), c


def test_largest_launch(rig):
  """mmax = 1024 (7 x 1024 doubles = 57344 B of dynamic LDS, the row the driver's default
  max_nodes = 1000 rounds up to) with m = 1024: launches, returns PM_OK, writes every node."""
  c = T.BY_NAME["m1024_full"]
  assert c.m == c.mmax == 1024
  res = rig.alone(c.name, c.path)  # (launch() asserts PM_OK)
  assert np.isfinite(res["y"][0]).all() and np.isfinite(res["rms"][0][:1023]).all()
  assert _untouched(res["rms"][0][1023:])


@pytest.mark.parametrize("name", T.TOL_ROWS)
def test_tol_boundaries_from_the_launch_own_rms(rig, name):
  """tol = rms[k] of a class-1 interval: it now adds 0.  A tol with 100 * tol == rms[k] in
  double: that interval adds 2.  y and rms do not depend on tol."""
  c = T.BY_NAME[name]
  first = _member(rig.alone(name, c.path), 0, c.m)
  b1, b2 = T.tol_boundaries(first["rms"], c.tol)
  assert b1 is not None and b2 is not None, (b1, b2)
  for (k, tol), want in ((b1, 0), (b2, 2)):
    res = rig.launch([c], c.mmax, c.path, tol)
    o = _member(res, 0, c.m)
    assert T.same(o["y"], first["y"]) and T.same(o["rms"], first["rms"]), (c, tol)
    cls = T.classes(o["rms"], tol)
    assert cls[k] == want and o["nadd"] == int(cls.sum()), (c, k, tol, o["nadd"])
    assert o["nadd"] == insert_nodes(c.x, o["rms"], tol).size - c.m
    assert o["nadd"] == c.restate(tol=tol)[2]
  k, tol = b1  # one ulp below, the interval is back in class 1: the boundary is where it is said
  below = _member(rig.launch([c], c.mmax, c.path, np.nextafter(tol, 0.0)), 0, c.m)
  assert below["nadd"] == int(T.classes(first["rms"], np.nextafter(tol, 0.0)).sum())
  assert T.classes(first["rms"], np.nextafter(tol, 0.0))[k] == 1


def test_mixed_batch_isolation(rig):
  """mmax = 1024, members of 2 ... 1024 nodes in one launch, both boundary conditions, the
  overflow member and both NaN members among them, the first and the last member inactive: every
  active member equals its own single launch bit for bit; rows of inactive members, y[:, :, m:]
  and rms[:, m-1:] keep the sentinel in every output."""
  cases = [T.BY_NAME[n] for n in T.BATCH]
  res = rig.launch(cases, T.BATCH_MMAX, "table", 1e-3, active=T.BATCH_ACTIVE, ends_only=True)
  for i, c in enumerate(cases):
    if not T.BATCH_ACTIVE[i]:
      assert all(_untouched(res[k][i]) for k in OUTPUTS), (i, c)
      continue
    o = _member(res, i, c.m)
    alone = _member(rig.alone(c.name, "table"), 0, c.m)
    assert T.same(o["y"], alone["y"]) and T.same(o["rms"], alone["rms"]), (i, c)
    assert o["nadd"] == int(T.classes(alone["rms"], 1e-3).sum()), (i, c)
    if c.tol == 1e-3:
      assert o["nadd"] == alone["nadd"], (i, c)
    assert T.same(o["b"], o["y"][0, [0, c.m - 1]]) and T.same(o["bz"], o["y"][1, [0, c.m - 1]]), c
    assert _padding_untouched(res, i, c.m), (i, c)
    if c.finite:
      assert np.isfinite(o["y"]).all() and np.isfinite(o["rms"]).all(), (i, c)


OPTIONAL = {
    "y": ("y",), "rms": ("rms",), "nadd": ("nadd",), "b_and_zidx": ("b", "zidx"),
    "bz": ("bz",), "flags": ("flags",), "bzbot": ("bzbot",),
}


@pytest.mark.parametrize("which", sorted(OPTIONAL))
def test_optional_pointers(rig, which):
  """One row relaunched with y, rms, nadd, b (+ zidx; bz then has nothing to follow), bz alone,
  flags, or bzbot passed as NULL: the remaining outputs are unchanged bit for bit; without flags
  or without bzbot the answer is the bbot problem's."""
  c = T.BY_NAME[T.POINTER_ROW]
  omit = OPTIONAL[which]
  res = rig.launch([c], c.mmax, c.path, c.tol, omit=omit)
  if which in ("flags", "bzbot"):
    ref = T.restate(c.x, c.c4, c.bs, c.bbot, 0.0, False, c.tol, zidx=c.zidx)
    assert not T.same(ref[0], T.reference(c.name)[0])
    o = _member(res, 0, c.m)
    _check_member(c, o, c.tol, ref)
    assert T.same(o["b"], ref[3]) and T.same(o["bz"], ref[4])
  else:
    full = rig.alone(c.name, c.path)
    for k in OUTPUTS:
      if which == "b_and_zidx" and k == "bz":  # bz is only written beside b
        assert _untouched(res["bz"])
      elif k not in omit:
        assert np.array_equal(np.ascontiguousarray(res[k]).view(np.uint8),
                              np.ascontiguousarray(full[k]).view(np.uint8)), (which, k)
  assert _padding_untouched(res, 0, c.m)


def test_driver_small(gpu):
  """ColumnEquiBatch(max_nodes=40) on four bzbot members that want 41 ... 57 nodes (one gives up
  at the first pass, three at the second): status 1, the node counts and b / bz of
  `oracle.column_solve_equi(max_nodes=40)` member by member -- within the sum of the two
  evaluations' proven bounds against the exact recurrence --, and the kept mesh, its y, b and bz
  bit for bit the restatement's."""
  D = T.DRIVER
  z, wA = D["z"], T.driver_wA()
  n = wA.shape[0]
  eq = gpu.ColumnEquiBatch.from_profiles(z, D["kappa"], D["Area"], D["bs"], D["bbot"],
                                         bzbot=D["bzbot"], n=n, max_nodes=D["max_nodes"])
  eq.solve(wA, keep_mesh=True)
  b, bz = eq.get_b(), eq.get_bz()
  mm, xx, yy = eq.mesh
  assert eq.passes == 2 and (eq.status == 1).all()
  Ak0 = D["Area"] * D["kappa"]
  for i in range(n):
    bo, bzo, x, st = O.column_solve_equi(z, drivers.equi_coef(z, D["kappa"], D["Area"], wA[i]),
                                         D["bs"], D["bbot"], D["bzbot"], max_nodes=D["max_nodes"])
    assert st == 1 and eq.nodes[i] == mm[i] == x.size and np.array_equal(xx[i, :mm[i]], x), i
    pts = T.point_sets(x)
    Ak = [Ak0 + 0. * p for p in pts]
    dAk = [np.gradient(a, p) for a, p in zip(Ak, pts)]  # the driver's: rounding noise, not 0
    c4, _ = T.coefficients(x, Ak, dAk, z=z, wA_z=wA[i])
    zidx = np.searchsorted(x, z)
    y, rms, nadd, br, bzr = T.restate(x, c4, D["bs"], D["bbot"], D["bzbot"], True, 1e-3, zidx=zidx)
    assert x.size + nadd > D["max_nodes"], i
    assert T.same(yy[i][:, :x.size], y), i  # also for the member that stopped a pass earlier
    assert T.same(b[i], br) and T.same(bz[i], bzr), i
    e = T.exact(x, c4, D["bs"], D["bbot"], D["bzbot"], True)
    bV, bY = T.scaled_bounds(e, D["bs"], D["bbot"], D["bzbot"], True)
    assert (np.abs(b[i] - bo) <= 2 * bY[zidx]).all() and (np.abs(bz[i] - bzo) <= 2 * bV[zidx]).all(), i
