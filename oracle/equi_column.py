"""CPU ORACLE for Equi_Column.solve -- TEST INFRASTRUCTURE, NOT PRODUCT.

The reference (src/pymoc/modules/equi_column.py) states a boundary-value problem and hands
it to `scipy.integrate.solve_bvp`, a third-party dependency (scipy 1.15.3 in this image) that
is not part of the reference checkout.  This oracle restates the PROBLEM -- the
non-dimensional profile closures (:116-185), `alpha` (:231-249), `bz` (:251-284), `bc`
(:286-347), `ode` (:349-406), the default initial guess (:187-213) and the output scaling
(:424-435) -- as plain functions of a parameter dict, and calls the same SciPy routine on it.
Pinned against the reference's own outputs (tests/golden/equi_column.npz, set G13).
"""
import numpy as np
from scipy import integrate
from scipy.integrate import _bvp
from scipy.sparse.linalg import splu


def problem(f=1.2e-4, b_s=0.025, b_bot=None, B_int=3e3, A=7e13, nz=100, H_guess=1500.,
            kappa=6e-5, psi_so=None, z=None, H=None, dkappa_dz=None):
  """Parameter dict of one equilibrium column (profiles: numbers, arrays on z or callables)."""
  return dict(f=f, b_s=b_s, b_bot=b_bot, B_int=B_int, A=A, nz=nz, H_guess=H_guess,
              kappa=kappa, psi_so=psi_so, z=z, H=H, dkappa_dz=dkappa_dz)


def _profiles(q):
  f, z = q['f'], q['z']
  kap, pso, dkz = q['kappa'], q['psi_so'], q.get('dkappa_dz')
  if callable(kap):  # equi_column.py:125-128, :146-149
    kappa = lambda x, H: kap(x * H) / (H**2 * f)
    if callable(dkz):
      dkappa = lambda x, H: dkz(x * H) / (H * f)
    else:
      dkappa = lambda x, H: np.gradient(kap(x * H), x * H) / (H * f)
  elif isinstance(kap, np.ndarray):
    dk = np.gradient(kap, z)
    kappa = lambda x, H: np.interp(x * H, z, kap) / (H**2 * f)
    dkappa = lambda x, H: np.interp(x * H, z, dk) / (H * f)
  else:
    kappa = lambda x, H: kap / (H**2 * f)
    dkappa = lambda x, H: 0
  if callable(pso):
    psi = lambda x, H: pso(x * H) / (f * H**3)
  elif isinstance(pso, np.ndarray):
    psi = lambda x, H: np.interp(x * H, z, pso) / (f * H**3)
  else:
    psi = lambda x, H: 0
  return kappa, dkappa, psi


def functions(q):
  """-> (ode, bc, hfree, has_bbot, bz): the problem closures solve_bvp is handed."""
  f, A = q['f'], q['A']
  kappa, dkappa, psi = _profiles(q)
  bs = -q['b_s'] / f**2
  has_bbot = q['b_bot'] is not None
  bbot = -q['b_bot'] / f**2 if has_bbot else None
  bz = lambda H: q['B_int'] / (f**3 * H**2 * A * kappa(-1, H))
  hfree = q['H'] is None

  def depth(p):
    return p[0] if hfree else q['H']

  def ode(x, y, p=None):
    H = depth(p)
    alpha = H**2 / (A * kappa(x, H))
    return np.vstack((y[1], y[2], y[3],
                      alpha * y[3] * (y[0] - psi(x, H) - A * dkappa(x, H) / (H**2))))

  def bc(ya, yb, p=None):
    H = depth(p)
    r = [ya[0], yb[0]] + ([ya[1]] if hfree else [])
    r.append(ya[2] - bbot / H if has_bbot else ya[3] + bz(H))
    r.append(yb[2] - bs / H)
    return np.array(r)

  return ode, bc, hfree, has_bbot, bz


def solve(q, tol=1e-3, max_nodes=1000):
  """-> dict(x, y, H, status, niter, sol): what Equi_Column.solve obtains from solve_bvp."""
  ode, bc, hfree, has_bbot, bz = functions(q)
  nz = q['nz']
  zi = np.linspace(-1, 0, nz)
  y0 = np.zeros((4, nz))
  y0[0] = 1.0
  y0[3] = -100.0 if has_bbot else -bz(1500.)
  res = integrate.solve_bvp(ode, bc, zi, y0, p=[q['H_guess']] if hfree else None, tol=tol,
                            max_nodes=max_nodes)
  H = res.p[0] if hfree else q['H']
  return dict(x=res.x, y=res.y, yp=res.yp, H=H, status=res.status, niter=res.niter,
              sol=res.sol)


def newton_system(q, x):
  """-> (fun, bc, col_fun, jac, k): solve_bvp's wrapped problem functions and the two callbacks
  `_bvp.solve_newton` takes on the mesh x (what `_bvp.prepare_sys` builds, on the same blocks:
  forward-difference Jacobians, `construct_global_jac`)."""
  ode, bc, hfree = functions(q)[:3]
  k, m = (1 if hfree else 0), x.size
  h = np.diff(x)
  fun, bcw = _bvp.wrap_functions(ode, bc, None, None, k, x[0], None, None, float)[:2]
  xm = x[:-1] + 0.5 * h
  i_jac, j_jac = _bvp.compute_jac_indices(4, m, k)

  def col_fun(y, p):
    return _bvp.collocation_fun(fun, y, p, x, h)

  def jac(y, p, y_middle, f, f_middle, bc0):
    df_dy, df_dp = _bvp.estimate_fun_jac(fun, x, y, p, f)
    df_dy_m, df_dp_m = _bvp.estimate_fun_jac(fun, xm, y_middle, p, f_middle)
    dya, dyb, dp = _bvp.estimate_bc_jac(bcw, y[:, 0], y[:, -1], p, bc0)
    return _bvp.construct_global_jac(4, m, k, i_jac, j_jac, h, df_dy, df_dy_m, df_dp, df_dp_m,
                                     dya, dyb, dp)

  return fun, bcw, col_fun, jac, k


def _gap(lhs, rhs, scale):
  """|lhs - rhs| / scale of a comparison `lhs < rhs`; inf where an operand is not finite (a
  comparison with NaN is false, and one with inf is decided, in any arithmetic)."""
  with np.errstate(all='ignore'):
    g = abs(lhs - rhs) / scale
  return float(g) if np.isfinite(g) else np.inf


def newton_pass(q, x, y, p, tol=1e-3):
  """What solve_bvp does between two mesh changes, from the iterate (y [4, m], p = H or None) on
  the mesh x: `_bvp.solve_newton` (restated below, _bvp.py:438-499, so that its path can be
  returned), then the residual estimate and insertion count of solve_bvp's loop (:1086-1104).
  -> (y, p, singular, yp, rms, nadd, info, rec): p as solve_newton returns it ([H] or []),
  info = (max rms, max |bc residual|), rec = dict(niter: iterations entered, njev, alphas: the
  damping factor each iteration ended on, converged: the stopping rule was met, margins:
  |cost_new - rhs| / cost of every line-search test `cost_new < rhs`, stop_margins: distance from 1
  of the largest ratio in every stopping test)."""
  x = np.asarray(x, float)
  y = np.array(y, float)
  fun, bc, col_fun, jac, k = newton_system(q, x)
  p = np.array([p], float) if k else np.array([])
  m, h = x.size, np.diff(x)
  tol_r = 2 / 3 * h * 5e-2 * tol
  max_njev, max_iter, sigma, tau, n_trial = 4, 8, 0.2, 0.5, 4
  col_res, y_middle, f, f_middle = col_fun(y, p)
  bc_res = bc(y[:, 0], y[:, -1], p)
  res = np.hstack((col_res.ravel(order='F'), bc_res))
  rec = dict(niter=0, njev=0, alphas=[], converged=False, margins=[], stop_margins=[])
  singular, recompute_jac = False, True
  for iteration in range(max_iter):
    rec['niter'] += 1
    if recompute_jac:
      J = jac(y, p, y_middle, f, f_middle, bc_res)
      rec['njev'] += 1
      try:
        LU = splu(J)
      except RuntimeError:
        singular = True
        break
      step = LU.solve(res)
      cost = np.dot(step, step)
    y_step = step[:m * 4].reshape((4, m), order='F')
    p_step = step[m * 4:]
    alpha = 1
    for trial in range(n_trial + 1):
      y_new = y - alpha * y_step
      p_new = p - alpha * p_step
      col_res, y_middle, f, f_middle = col_fun(y_new, p_new)
      bc_res = bc(y_new[:, 0], y_new[:, -1], p_new)
      res = np.hstack((col_res.ravel(order='F'), bc_res))
      step_new = LU.solve(res)
      cost_new = np.dot(step_new, step_new)
      rec['margins'].append(_gap(cost_new, (1 - 2 * alpha * sigma) * cost, cost))
      if cost_new < (1 - 2 * alpha * sigma) * cost:
        break
      if trial < n_trial:
        alpha *= tau
    y, p = y_new, p_new
    rec['alphas'].append(alpha)
    if rec['njev'] == max_njev:
      break
    with np.errstate(all='ignore'):
      worst = max(np.max(np.abs(col_res) / (tol_r * (1 + np.abs(f_middle)))),
                  np.max(np.abs(bc_res)) / tol)
    rec['stop_margins'].append(_gap(worst, 1.0, 1.0))
    if (np.all(np.abs(col_res) < tol_r * (1 + np.abs(f_middle))) and
        np.all(np.abs(bc_res) < tol)):
      rec['converged'] = True
      break
    if alpha == 1:
      step, cost, recompute_jac = step_new, cost_new, False
    else:
      recompute_jac = True
  col_res, y_middle, f, f_middle = _bvp.collocation_fun(fun, y, p, x, h)
  bc_res = bc(y[:, 0], y[:, -1], p)
  sol = _bvp.create_spline(y, f, x, h)
  rms = _bvp.estimate_rms_residuals(fun, sol, x, h, p, 1.5 * col_res / h, f_middle)
  with np.errstate(invalid='ignore'):
    nadd = int(((rms > tol) & (rms < 100 * tol)).sum() + 2 * (rms >= 100 * tol).sum())
  info = (np.max(rms), np.max(np.abs(bc_res)))
  return y, p, singular, f, rms, nadd, info, rec


def outputs(q, r):
  """(z, psi, b) as Equi_Column.solve leaves them (equi_column.py:424-435)."""
  f, H = q['f'], r['H']
  if q['z'] is None:
    return r['x'] * H, r['y'][0] * f * H**3 / 1e6, -r['y'][2] * f**2 * H
  z = q['z']
  s = r['sol'](z / H)
  psi = s[0] * f * H**3 / 1e6
  b = -s[2] * f**2 * H
  psi[z < -H] = np.nan
  b[z < -H] = np.nan
  return z, psi, b
