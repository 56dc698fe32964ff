"""Equi_Column.solve on the GPU: solve_bvp's Newton iteration and
residual control in `pm_equi_column_newton` against SciPy itself (the oracle restates the
problem and calls scipy.integrate.solve_bvp) and against the reference's outputs (G13); then the
entry point one launch at a time on the table of tests/equi_column_cases.py, against one mesh
iteration of solve_bvp built on SciPy's own blocks (`oracle.equi_column.newton_pass`)."""
import ctypes as C

import numpy as np
import pytest
from scipy.integrate import _bvp

import equi_column_cases as T
from oracle import equi_column as EO
from conftest import load_golden, relerr
from pymoc_amd import configs

pytestmark = pytest.mark.gpu


def test_equi_column_golden_through_the_drop_in_class(gpu):
  """Every G13 problem through `Equi_Column(...).solve()`: the same mesh history as SciPy
  (node counts, iterations, status) and psi / b / H of the reference."""
  g = load_golden("equi_column")
  for name, kw in configs.equi_column_cases().items():
    m = gpu.Equi_Column(**kw)
    m.solve()
    r = EO.solve(EO.problem(**kw))
    eq = m._eq
    assert m.status == r["status"] == 0, name
    assert eq.x[0].size == r["x"].size and eq.niter[0] == r["niter"], (
        name, eq.x[0].size, r["x"].size, eq.niter[0], r["niter"])
    assert relerr(eq.x[0], r["x"]) <= 1e-15, name
    # measured 1e-17 ... 8e-12 (profiles/r01/probe_equi_column.txt); the bound leaves room for
    # the different elimination order of the linear solves (band LU here, SuperLU in SciPy)
    assert relerr(eq.y[0], r["y"]) <= 1e-9, (name, relerr(eq.y[0], r["y"]))
    assert abs(m.H - float(g[name + "_H"])) <= 1e-9 * abs(m.H), name
    assert relerr(m.z, g[name + "_z"]) <= 1e-9, name
    assert relerr(m.psi, g[name + "_psi"]) <= 1e-9, (name, relerr(m.psi, g[name + "_psi"]))
    assert relerr(m.b, g[name + "_b"]) <= 1e-9, (name, relerr(m.b, g[name + "_b"]))


def test_equi_column_batch_of_different_problems(gpu):
  """One batch, 24 members with different B_int / area / diffusivity, H unknown: every
  member against SciPy on that member alone (meshes refine independently)."""
  rng = np.random.default_rng(11)
  n = 24
  B = rng.uniform(2e3, 1.2e4, n)
  A = rng.uniform(6e13, 2e14, n)
  kap = rng.uniform(2e-5, 6e-5, n)
  eq = gpu.EquiColumnBatch(n, B_int=B, A=A, kappa=kap, nz=60).solve()
  nodes = set()
  for i in range(n):
    r = EO.solve(EO.problem(B_int=B[i], A=A[i], kappa=kap[i], nz=60))
    assert eq.status[i] == r["status"] == 0, i
    assert eq.x[i].size == r["x"].size and eq.niter[i] == r["niter"], i
    assert relerr(eq.y[i], r["y"]) <= 1e-9, (i, relerr(eq.y[i], r["y"]))
    assert abs(eq.H[i] - r["H"]) <= 1e-9 * r["H"], i
    nodes.add(eq.x[i].size)
  assert len(nodes) > 4


def test_equi_column_api_contract(gpu):
  """Constructor / helper behaviour the reference's tests pin
  (tests/modules/test_equi_column.py:113-368)."""
  z = np.asarray(np.linspace(-4000, 0, 80))
  with pytest.raises(Exception) as e:
    gpu.Equi_Column(z=z, A=2.0e14, kappa=3e-5, H=500.0, B_int=None, b_bot=None)
  assert str(e.value) == 'You need to specify either b_bot or B_int for bottom boundary condition'
  c = gpu.Equi_Column(z=z, B_int=3e3, A=2.0e14, kappa=3e-5)
  assert c.f == 1.2e-4 and c.A == 2.0e14 and c.H is None and c.H_guess == 1500.
  assert np.array_equal(c.zi, np.linspace(-1, 0, 100))
  assert c.bs == -0.025 / 1.2e-4**2 and c.B_int == 3e3
  assert c.kappa(-0.5, 1000.) == 3e-5 / (1000.**2 * 1.2e-4) and c.dkappa_dz(-0.5, 1000.) == 0
  assert c.psi_so(-0.5, 1000.) == 0
  assert c.alpha(-0.5, 1000.) == 1000.**2 / (2.0e14 * c.kappa(-0.5, 1000.))
  assert c.sol_init.shape == (4, 100) and (c.sol_init[0] == 1).all()
  assert (c.sol_init[3] == -c.bz(1500.)).all()
  ya, yb = np.array([1., 2., 3., 4.]), np.array([5., 6., 7., 8.])
  assert np.array_equal(c.bc(ya, yb, [1200.]),
                        np.array([1., 5., 2., 4. + c.bz(1200.), 7. - c.bs / 1200.]))
  with pytest.raises(TypeError) as e:
    c.bc(ya, yb)
  assert str(e.value) == 'Must provide a p array if column does not have an H value'
  with pytest.raises(TypeError):
    c.ode(c.zi, c.sol_init)
  y = np.vstack([np.linspace(0, 1, 100)] * 4)
  out = c.ode(c.zi, y, [1200.])
  assert np.array_equal(out[:3], y[1:]) and np.array_equal(
      out[3], c.alpha(c.zi, 1200.) * y[3] * (y[0] - 0 - 2.0e14 * 0 / 1200.**2))
  karr = np.linspace(3e-5, 1e-5, 80)
  c2 = gpu.Equi_Column(z=z, B_int=3e3, A=2.0e14, kappa=karr, psi_so=(z + 2000)**2, H=500.0,
                       b_bot=4e3)
  assert c2.b_bot == -4e3 / 1.2e-4**2 and (c2.sol_init[3] == -100.).all()
  assert c2.kappa(-0.5, 500.) == np.interp(-250., z, karr) / (500.**2 * 1.2e-4)
  assert c2.dkappa_dz(-0.5, 500.) == np.interp(-250., z, np.gradient(karr, z)) / (500. * 1.2e-4)
  assert c2.psi_so(-0.5, 500.) == np.interp(-250., z, (z + 2000)**2) / (1.2e-4 * 500.**3)
  assert np.array_equal(c2.bc(ya, yb), np.array([1., 5., 3. - c2.b_bot / 500., 7. - c2.bs / 500.]))


def test_equi_column_callable_profiles_are_tabulated(gpu):
  """examples/example_Equi_Bint.py with its own callables (kappa, dkappa_dz, psi_so): the
  drop-in class samples them on a 65537-level table; same meshes as the reference, depth and
  profiles to 1e-7 (measured: H 4e-10, psi / b 7e-9)."""
  g = load_golden("equi_column")
  for i in range(4):
    m = gpu.Equi_Column(**configs.equi_bint_callable_case(i))
    m.solve()
    name = "Bint_fn%d" % i
    assert m.status == 0
    Href = float(g[name + "_H"])
    assert abs(m.H - Href) <= 1e-7 * Href, (i, m.H, Href)
    zr, pr, br = g[name + "_z"], g[name + "_psi"], g[name + "_b"]
    assert m.z.size == zr.size and relerr(m.z, zr) <= 1e-7
    assert relerr(m.psi, pr) <= 1e-7 and relerr(m.b, br) <= 1e-7, i


def test_equi_column_failure_modes_match_solve_bvp(gpu):
  """A singular Jacobian ends with status 2 like SciPy; NaN or hopeless members of a batch end
  with a status of their own without disturbing their neighbours."""
  z = np.linspace(-4000, 0, 80)
  kw = dict(z=z, A=2e14, kappa=3e-5, H=500.0, B_int=None, b_bot=4e3)
  m = gpu.Equi_Column(**kw)
  m.solve()
  r = EO.solve(EO.problem(**kw))
  assert m.status == r["status"] == 2 and m._eq.x[0].size == r["x"].size
  eq = gpu.EquiColumnBatch(3, B_int=np.array([3e3, np.nan, 3e3]), A=2e14,
                           kappa=np.array([3e-5, 3e-5, 1e-9]), nz=40).solve()
  ref = EO.solve(EO.problem(B_int=3e3, A=2e14, kappa=3e-5, nz=40))
  assert eq.status[0] == 0 and eq.status[1] != 0 and eq.status[2] != 0
  assert abs(eq.H[0] - ref["H"]) <= 1e-9 * ref["H"] and eq.x[0].size == ref["x"].size


# ------------------------------------------------------------------ K7, one launch at a time
SENTINEL = -7  # in nadd / status / niter before a launch


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
  """Bitwise equality (NaN payloads and signed zeros included)."""
  return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class _Rig(object):
  """Buffers the tests own.  One scratch allocation serves every launch, whatever its mmax."""

  def __init__(self, gpu):
    from pymoc_amd import _lib
    from pymoc_amd.device import DeviceArray
    self.lib, self.DA = _lib, DeviceArray
    self.S = int(_lib.lib.pm_equi_column_scratch_doubles(1))
    self.rows = max([len(b[1]) * T.BATCH_MMAX for b in T.BATCHES] + [c.mmax for c in T.CASES])
    self.scratch = DeviceArray.from_host(np.full((self.rows, self.S), np.nan))

  def launch(self, cases, mmax, fill, active=None, nzg=None):
    """One launch of `cases` as members 0 .. n-1 with rows of mmax.  `fill` (NaN, 0.0) goes into
    the scratch and every padding entry of x / y / yp / rms first; fill=None leaves the scratch
    as the previous launch left it (padding NaN).  -> host copies of every output."""
    L, DA = self.lib, self.DA
    n = len(cases)
    assert all(3 <= c.m <= mmax for c in cases) and n * mmax <= self.rows
    assert int(L.lib.pm_equi_column_scratch_doubles(mmax)) == self.S * mmax
    arrs = [c for c in cases if c.flags & 12]
    if nzg is None:
      nzg = arrs[0].q["z"].size if arrs else 0
    zg = arrs[0].q["z"] if arrs else np.zeros(max(nzg, 1))
    assert all(c.q["z"].size == nzg for c in arrs)
    pad = np.nan if fill is None else fill
    if fill is not None:
      self.scratch.view(0, n * mmax).upload(np.full((n * mmax, self.S), fill))
    x = np.full((n, mmax), pad)
    y, yp, rms = np.full((n, 4, mmax), pad), np.full((n, 4, mmax), pad), np.full((n, mmax), pad)
    mem = [T.member(c.q, max(nzg, 1)) for c in cases]
    for i, c in enumerate(cases):
      x[i, :c.m], y[i, :, :c.m] = c.x, c.y
    host = dict(x=x, y=y, yp=yp, rms=rms, p=np.array([c.p for c in cases]),
                m=np.array([c.m for c in cases], np.int32),
                flags=np.array([c.flags for c in cases], np.int32), zg=zg,
                nadd=np.full(n, SENTINEL, np.int32), status=np.full(n, SENTINEL, np.int32),
                niter=np.full(n, SENTINEL, np.int32), info=np.full((n, 2), float(SENTINEL)))
    for k in ("f", "A", "bs", "bb", "kappa", "kappa_z", "dkappa_z", "psi_z"):
      host[k] = np.array([d[k] for d in mem], np.float64)
    if active is not None:
      host["active"] = np.asarray(active, np.int32)
    dev = {k: DA.from_host(v) for k, v in host.items()}
    d = L.pm_equi_column()
    d.n, d.nzg, d.mmax, d.reserved, d.tol = n, nzg, mmax, 0, T.TOL
    for k in dev:
      setattr(d, k, dev[k].ptr)
    if nzg == 0:
      d.zg = d.kappa_z = d.dkappa_z = d.psi_z = None
    d.scratch = self.scratch.ptr
    L.check(L.lib.pm_equi_column_newton(C.byref(d), None))
    out = {k: dev[k].download() for k in ("y", "yp", "rms", "p", "nadd", "status", "niter", "info")}
    out["start"] = host
    return out


def _member(out, i):
  return {k: out[k][i] for k in ("y", "yp", "rms", "p", "nadd", "status", "niter", "info")}


def _equal_members(a, b, m):
  """The outputs of a member of two launches, bitwise, on its own m nodes."""
  return (_same(a["y"][:, :m], b["y"][:, :m]) and _same(a["yp"][:, :m], b["yp"][:, :m]) and
          _same(a["rms"][:m - 1], b["rms"][:m - 1]) and _same(a["p"], b["p"]) and
          _same(a["info"], b["info"]) and
          (a["nadd"], a["status"], a["niter"]) == (b["nadd"], b["status"], b["niter"]))


def _padding_untouched(out, i, m):
  s = out["start"]
  return (_same(out["y"][i][:, m:], s["y"][i][:, m:]) and _same(out["yp"][i][:, m:], s["yp"][i][:, m:])
          and _same(out["rms"][i][m - 1:], s["rms"][i][m - 1:]))


@pytest.fixture(scope="module")
def table(gpu):
  """Every row of the table through the kernel three times on ONE scratch allocation: as the
  previous row (another m, another mmax) left it, filled with NaN, filled with zeros.
  -> {name: [three outputs]}, rig."""
  rig = _Rig(gpu)
  runs = {}
  for c in T.CASES:
    runs[c.name] = [rig.launch([c], c.mmax, fill) for fill in (None, np.nan, 0.0)]
  return runs, rig


def _cmp(a, ref):
  """Largest per-component max-norm error relative to the component's max |ref|."""
  a, ref = np.atleast_2d(a), np.atleast_2d(ref)
  return max(relerr(a[c], ref[c]) for c in range(ref.shape[0]))


def _vs_tol(a, ref):
  """Largest |a - ref| in units of max(|ref|, tol): rms and boundary residuals are only ever
  compared with tol (and 100 tol); below it they are rounding noise of order eps * |y'|."""
  a, ref = np.atleast_1d(a), np.atleast_1d(ref)
  return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref), T.TOL)))


def own_output_deviations(runs):
  """(a): the worst deviation over the table of each secondary output from the same function of
  the kernel's OWN (y, p), formed with the oracle's closures and SciPy's functions."""
  w = dict(yp=0.0, rms=0.0, bc=0.0)
  for c in T.CASES:
    o = _member(runs[c.name][0], 0)
    m, h = c.m, np.diff(c.x)
    y, p = o["y"][:, :m], (np.array([o["p"]]) if c.hfree else np.array([]))
    fun, bc = EO.newton_system(c.q, c.x)[:2]
    f = fun(c.x, y, p)
    col_res, _, _, f_middle = _bvp.collocation_fun(fun, y, p, c.x, h)
    rms = _bvp.estimate_rms_residuals(fun, _bvp.create_spline(y, f, c.x, h), c.x, h, p,
                                      1.5 * col_res / h, f_middle)
    w["yp"] = max(w["yp"], _cmp(o["yp"][:, :m], f))
    w["rms"] = max(w["rms"], _vs_tol(o["rms"][:m - 1], rms))
    w["bc"] = max(w["bc"], _vs_tol(o["info"][1], np.max(np.abs(bc(y[:, 0], y[:, -1], p)))))
  return w


def pass_deviations(runs):
  """(b): the worst deviation of y, p, rms from `newton_pass` from the same start, separately
  for launches that met the stopping rule and for those that ran out of Jacobians / iterations."""
  w = {k + e: 0.0 for k in ("y", "p", "rms") for e in ("_conv", "_unconv")}
  for c in T.CASES:
    y, p, sing, yp, rms, nadd, info, rec = T.reference(c)
    if sing:
      continue
    o = _member(runs[c.name][0], 0)
    e = "_conv" if rec["converged"] else "_unconv"
    w["y" + e] = max(w["y" + e], _cmp(o["y"][:, :c.m], y))
    if c.hfree:
      w["p" + e] = max(w["p" + e], abs(o["p"] - p[0]) / abs(p[0]))
    w["rms" + e] = max(w["rms" + e], _vs_tol(o["rms"][:c.m - 1], rms))
  return w


# Bounds: 10 x the worst value measured over the table on an MI355X (DESIGN section 4, row "K7,
# one launch"); the factor is for the two licensed differences, the elimination order (band LU
# here, SuperLU in SciPy) and the forward-difference Jacobians they are applied to.
# (a) measured: yp, rms and info[1] all exactly SciPy's values on the kernel's own (y, p) -- the
# same operations in the same order -- so they are asserted exactly.
OWN_BOUNDS = dict(yp=0.0, rms=0.0, bc=0.0)
# (b) measured, launches that met the stopping rule: y 2.2e-16, p 0 (given 10 ulp, 2.2e-15, the
# format's floor, not 10 x 0), rms 4.3e-11 of max(rms, tol); launches that ran out of Jacobians
# or iterations (H running to 24000 m, damping down to 1/16: rounding is amplified along the
# path): y 4.2e-5, p 3.0e-6, rms 1.6e-4 of max(rms, tol).
PASS_BOUNDS = dict(y_conv=2.2e-15, p_conv=2.2e-15, rms_conv=4.3e-10, y_unconv=4.2e-4,
                   p_unconv=3.0e-5, rms_unconv=1.6e-3)


def test_launch_secondary_outputs_are_functions_of_its_own_iterate(table):
  """(a) yp = ode(x, y, p), rms = estimate_rms_residuals on create_spline(y, yp), info[1] =
  max |bc(ya, yb, p)| of the kernel's own (y, p); info[0] and nadd formed exactly from the
  kernel's own rms."""
  runs = table[0]
  for c in T.CASES:
    o = _member(runs[c.name][0], 0)
    rms = o["rms"][:c.m - 1]
    assert o["info"][0] == rms.max(), c
    want = int(((rms > T.TOL) & (rms < 100 * T.TOL)).sum() + 2 * (rms >= 100 * T.TOL).sum())
    assert o["nadd"] == want, (c, o["nadd"], want)
  w = own_output_deviations(runs)
  print("K7 one launch, own output:", w)
  for k, bound in OWN_BOUNDS.items():
    assert w[k] <= bound, (k, w[k], bound)


def test_launch_matches_one_mesh_iteration_of_solve_bvp(table):
  """(b) status, Newton iterations and insertion count equal `newton_pass`'s from the same
  start on every row (test_equi_column_cpu.py makes every row decisive); y, p, rms within
  bounds; a launch that is singular at its first factorisation returns its start."""
  runs = table[0]
  for c in T.CASES:
    y, p, sing, yp, rms, nadd, info, rec = T.reference(c)
    o = _member(runs[c.name][0], 0)
    got = (int(o["status"]), int(o["niter"]), int(o["nadd"]))
    assert got == (2 if sing else 0, rec["niter"], nadd), (c, got, sing, rec["niter"], nadd)
    if sing or not c.hfree:
      assert o["p"] == c.p, c
    if sing:
      assert _same(o["y"][:, :c.m], c.y), c
  w = pass_deviations(runs)
  print("K7 one launch, against newton_pass:", w)
  assert max(PASS_BOUNDS["y_conv"], PASS_BOUNDS["p_conv"]) <= 1e-9
  for k, bound in PASS_BOUNDS.items():
    assert w[k] <= bound, (k, w[k], bound)


def test_launch_reads_nothing_it_was_not_given_and_writes_nothing_else(table):
  """(c) a row gives the same bits whether scratch and padding hold the previous row's leftovers,
  NaN or zeros, and leaves the padding of y / yp / rms alone; in the batches every member
  equals its own single launch bitwise (other m, other mmax, other neighbours, a singular and a
  NaN member among them) and the inactive member is not touched."""
  runs, rig = table
  for c in T.CASES:
    a, b, z = runs[c.name]
    assert _equal_members(_member(a, 0), _member(b, 0), c.m), c
    assert _equal_members(_member(a, 0), _member(z, 0), c.m), c
    for o in (a, b, z):
      assert _padding_untouched(o, 0, c.m), c
  nan_alone = _member(rig.launch([T.NAN_CASE], T.NAN_CASE.mmax, np.nan), 0)
  # it ran, and what it reports can not pass for a solution in the outer loop
  assert nan_alone["status"] != SENTINEL and not nan_alone["info"][1] <= T.TOL, nan_alone
  for name, rows, active, nzg in T.BATCHES:
    cs = [T.batch_case(r) for r in rows]
    for fill in (np.nan, 0.0):
      out = rig.launch(cs, T.BATCH_MMAX, fill, active=active, nzg=nzg)
      for i, c in enumerate(cs):
        o = _member(out, i)
        if not active[i]:
          s = out["start"]
          assert _same(o["y"], s["y"][i]) and _same(o["yp"], s["yp"][i]), (name, c)
          assert _same(o["rms"], s["rms"][i]) and o["p"] == c.p, (name, c)
          assert (o["nadd"], o["status"], o["niter"]) == (SENTINEL,) * 3, (name, c)
          assert (o["info"] == SENTINEL).all(), (name, c)
          continue
        alone = nan_alone if c is T.NAN_CASE else _member(runs[c.name][0], 0)
        assert _equal_members(o, alone, c.m), (name, c, fill)
        assert _padding_untouched(out, i, c.m), (name, c)
