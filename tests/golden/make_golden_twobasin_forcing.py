#!/usr/bin/env python3
"""Generate tests/golden/twobasin_forcing.npz (G27) by RUNNING THE REFERENCE's classes in the
two-basin script's loop under time-dependent forcing.

Run only where the reference checkout is available (read-only), with PYMOC_REFERENCE_SRC naming
its src/ directory:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_twobasin_forcing.py

G27 twobasin_forcing   Column, Psi_Thermwind and Psi_SO of the reference in the loop of
examples/twobasin_NadeauJansen.py:99-122 (make_golden.ref_twobasin's restatement: the script itself
is Python 2), member by member, with a transient experiment's assignments at the top of the loop
body: `Atl.bs = Pac.bs`, `north.bs`, `SO_Atl.tau = SO_Pac.tau` and both `SO_*.bs` set to
np.interp(s * dt, knots, values) at the iterations TwoBasinSweep applies a schedule at (s = 0 and
s = 1 mod MOC_up_iters; tests/twobasin_sweep_cases.py: applied_at) and held in between.  The case,
knots and values are those of tests/twobasin_sweep_cases.py; the fixture holds the seven sampled
fields of both members at steps 1, M + 1 and 3 M + 4, the knots and the knot values, and the
NumPy / SciPy versions.

The final state must differ from the unforced run of the same members by at least 1000 x the
tolerance of the tests (1e-10) in the max-norm relative error of some field, and so must the state
at M + 1 (the ramp has begun by then): a fixture the driver could match without applying the
schedule would be worthless; the generator stops otherwise.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ["PYMOC_REFERENCE_SRC"])

import numpy as np
import scipy

from pymoc.modules import Column, Psi_Thermwind, Psi_SO  # the REFERENCE
from pymoc.utils import make_func
import twobasin_sweep_cases as S

warnings.simplefilter("ignore")  # the reference divides by zero in Psib


def ref_twobasin(m, nsteps, snaps, forcing):
  """make_golden.ref_twobasin with `forcing(s)` -> {target: value} or None at the loop top."""
  z, y = m['z'], m['y']
  kap = m['kappa']
  AMOC = Psi_Thermwind(z=z, b1=m['b_Atl0'].copy(), b2=m['b2_init'].copy(), f=m['f_AMOC'])
  AMOC.solve()
  [Psi_iso_Atl, Psi_iso_N] = AMOC.Psibz()
  ZOC = Psi_Thermwind(z=z, b1=m['b_Atl0'].copy(), b2=m['b_Pac0'].copy(), f=m['f_ZOC'])
  ZOC.solve()
  [Psi_zonal_Atl, Psi_zonal_Pac] = ZOC.Psibz()
  SO_Atl = Psi_SO(z=z, y=y, b=m['b_Atl0'].copy(), bs=m['bs_SO'].copy(), tau=float(m['tau']),
                  L=m['L_Atl'], KGM=float(m['K']))
  SO_Atl.solve()
  SO_Pac = Psi_SO(z=z, y=y, b=m['b_Pac0'].copy(), bs=m['bs_SO'].copy(), tau=float(m['tau']),
                  L=m['L_Pac'], KGM=float(m['K']))
  SO_Pac.solve()
  mk = lambda b, bs, A: Column(z=z, kappa=kap.copy(), b=b.copy(), bs=bs, bbot=m['bbot'],  # noqa
                               Area=float(A), N2min=m['N2min'])
  Atl = mk(m['b_Atl0'], m['bs'], m['A_Atl'])
  north = mk(m['b_north0'], m['bs_north'], m['A_north'])
  Pac = mk(m['b_Pac0'], m['bs'], m['A_Pac'])
  out = {}
  for ii in range(nsteps):
    v = forcing(ii)
    if v is not None:
      Atl.bs = Pac.bs = float(v['bs'])
      north.bs = float(v['bs_north'])
      SO_Atl.tau = make_func(float(v['tau']), y, 'tau')
      SO_Pac.tau = make_func(float(v['tau']), y, 'tau')
      SO_Atl.update(bs=v['bs_SO'].copy())
      SO_Pac.update(bs=v['bs_SO'].copy())
    wA_Atl = (Psi_iso_Atl + Psi_zonal_Atl - SO_Atl.Psi) * 1e6
    wAN = -Psi_iso_N * 1e6
    wA_Pac = (-Psi_zonal_Pac - SO_Pac.Psi) * 1e6
    Atl.timestep(wA=wA_Atl, dt=m['dt'])
    north.timestep(wA=wAN, dt=m['dt'], do_conv=True)
    Pac.timestep(wA=wA_Pac, dt=m['dt'])
    if ii % m['MOC_up_iters'] == 0:
      AMOC.update(b1=Atl.b, b2=north.b)
      AMOC.solve()
      [Psi_iso_Atl, Psi_iso_N] = AMOC.Psibz()
      ZOC.update(b1=Atl.b, b2=Pac.b)
      ZOC.solve()
      [Psi_zonal_Atl, Psi_zonal_Pac] = ZOC.Psibz()
      SO_Atl.update(b=Atl.b)
      SO_Atl.solve()
      SO_Pac.update(b=Pac.b)
      SO_Pac.solve()
    if ii + 1 in snaps:
      out[ii + 1] = dict(b_Atl=Atl.b.copy(), b_north=north.b.copy(), b_Pac=Pac.b.copy(),
                         Psi_AMOC=AMOC.Psi.copy(), Psi_ZOC=ZOC.Psi.copy(),
                         Psi_SO_Atl=SO_Atl.Psi.copy(), Psi_SO_Pac=SO_Pac.Psi.copy())
  return out


def relerr(a, ref):
  return np.max(np.abs(a - ref)) / np.max(np.abs(ref))


def main():
  t, values = S.schedule()
  out = dict(numpy_version=np.__version__, scipy_version=scipy.__version__,
             reference="pymoc 0.0.1rc5", knots=t)
  for k, v in values.items():
    out["values_" + k] = v
  runs = {True: [], False: []}
  for j, m in enumerate(S.members()):
    def forcing(s, j=j, m=m):
      return S.member_values(values, t, s * m['dt'], j) if S.applied_at(s) else None
    runs[True].append(ref_twobasin(m, S.STEPS, set(S.SNAPS), forcing))
    runs[False].append(ref_twobasin(m, S.STEPS, set(S.SNAPS), lambda s: None))
  for s in S.SNAPS:
    for k in S.FIELDS:
      out["s%03d_%s" % (s, k)] = np.stack([r[s][k] for r in runs[True]])
  for s in S.SNAPS[1:]:
    moved = max(relerr(np.stack([r[s][k] for r in runs[True]]),
                       np.stack([r[s][k] for r in runs[False]])) for k in S.FIELDS)
    print("forced vs unforced at step %d: %.3e (needs >= %.1e)" % (s, moved, 1000 * S.TOL))
    assert moved >= 1000 * S.TOL, s
  assert all(np.isfinite(v).all() for k, v in out.items() if k.startswith("s0"))
  path = os.path.join(HERE, "twobasin_forcing.npz")
  np.savez_compressed(path, **out)
  print("twobasin_forcing.npz %.1f KiB" % (os.path.getsize(path) / 1024.))


if __name__ == "__main__":
  main()
