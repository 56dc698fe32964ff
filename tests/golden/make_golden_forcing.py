#!/usr/bin/env python3
"""Generate tests/golden/forcing.npz (G26) by RUNNING THE REFERENCE under time-dependent forcing.

Run only where the reference checkout is available (read-only), with PYMOC_REFERENCE_SRC naming
its src/ directory:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_forcing.py

G26 forcing   The reference's classes in the example scripts' own loops (example_twocol.py:85-96,
example_twocol_plusSO.py:99-115, run_JansenNadeau_2018.py:201-261 -- the loops of make_golden.py's
ref_twocol / ref_jn2018), member by member, with the transient experiments' assignments at the top
of the loop body: `basin.bs`, `north.bs`, `SO.tau` / `SO.bs`, `channel.b_rest` / `.surflux` set to
np.interp(s * dt, knots, values) at the iterations the ensemble drivers apply a schedule at (s = 0
and s = RESTART_PHASE mod MOC_up_iters; tests/forcing_cases.py: applied_at) and held in between.
The cases, knots and values are those of tests/forcing_cases.py; the fixture holds, per case and
snapshot step, the members' state arrays, plus the NumPy / SciPy versions.

Each case's final state must differ from the unforced run of the same cfg by at least 1000 x the
tolerance of the driver's golden test (forcing_cases.TOL) in the max-norm relative error of some
field -- a fixture the drivers could match without applying the schedule would be worthless; the
generator stops otherwise.  The JN2018 case must also be well conditioned in the reference itself:
b_rest scaled by (1 + 4e-16) at the application of step 36 alone -- two roundings -- may move no
field of the final state by more than a tenth of the tolerance (under a strong warming the
reference's mixed layer amplifies such a change to 1e-7 within 36 steps, and no bound of 1e-10
could be asked of anyone).
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

from pymoc.modules import Column, Psi_Thermwind, Psi_SO, SO_ML  # the REFERENCE
from pymoc.utils import make_func
from pymoc_amd import configs  # parameter tables only
import forcing_cases as FC

warnings.simplefilter("ignore")  # the reference divides by zero in Psib


def ref_twocol(m, nsteps, snaps, forcing, so=False):
  """make_golden.ref_twocol with `forcing(s)` -> {target: value} or None at the loop top."""
  z = m['z']
  AMOC = Psi_Thermwind(z=z, b1=m['b_basin0'].copy(), b2=m['b_north0'].copy(), f=m['f'])
  AMOC.solve()
  pib, pin = AMOC.Psibz()
  if so:
    SO = Psi_SO(z=z, y=m['y'], b=m['b_basin0'].copy(), bs=m['bs_SO'].copy(),
                tau=float(m['tau']), f=m['f'], L=m['L'], KGM=float(m['KGM']), c=m['c'],
                bvp_with_Ek=m['bvp_with_Ek'])
    SO.solve()
  kap = m['kappa'] + 0 * z
  basin = Column(z=z, kappa=kap.copy(), Area=float(m['A_basin']), b=m['b_basin0'].copy(),
                 bs=float(m['bs']), bbot=float(m['bbot']))
  north = Column(z=z, kappa=kap.copy(), Area=float(m['A_north']), b=m['b_north0'].copy(),
                 bs=float(m['bs_north']), bbot=float(m['bbot']))
  out = {}
  for ii in range(nsteps):
    v = forcing(ii)
    if v is not None:
      basin.bs = float(v['bs'])
      north.bs = float(v['bs_north']) if 'bs_north' in v else north.bs
      if so:
        SO.tau = make_func(float(v['tau']), m['y'], 'tau')
        SO.update(bs=v['bs_SO'].copy())
    wAb = (pib - SO.Psi) * 1e6 if so else pib * 1e6
    wAN = -pin * 1e6
    basin.timestep(wA=wAb, dt=m['dt'])
    north.timestep(wA=wAN, dt=m['dt'], do_conv=True)
    if ii % m['MOC_up_iters'] == 0:
      AMOC.update(b1=basin.b, b2=north.b)
      AMOC.solve()
      pib, pin = AMOC.Psibz()
      if so:
        SO.update(b=basin.b)
        SO.solve()
    if ii + 1 in snaps:
      out[ii + 1] = dict(b_basin=basin.b.copy(), b_north=north.b.copy(),
                         Psi=AMOC.Psi.copy(), Psi_iso_b=pib.copy(), Psi_iso_n=pin.copy(),
                         Psi_SO=SO.Psi.copy() if so else 0 * z)
  return out


def ref_jn2018(m, nsteps, snaps, forcing):
  """make_golden.ref_jn2018 with `forcing(s)` at the loop top, ahead of the MOC update."""
  z, y = m['z'], m['y']
  kappa, kappaeff = configs.jn2018_kappa, configs.jn2018_kappaeff
  b_basin, b_north, bs_SO = m['b_basin0'].copy(), m['b_north0'].copy(), m['bs_SO_init'].copy()
  AMOC = Psi_Thermwind(z=z, b1=b_basin, b2=b_north, f=m['f'])
  AMOC.solve()
  PsiSO = Psi_SO(z=z, y=y, b=b_basin, bs=bs_SO, tau=float(m['tau']), f=m['f'], L=m['L'],
                 KGM=float(m['KGM']))
  PsiSO.solve()
  bs_SO[-1] = m['bs']
  basin = Column(z=z, kappa=kappaeff, Area=m['A_basin'], b=b_basin, bs=float(m['bs']),
                 bbot=b_basin[0])
  north = Column(z=z, kappa=kappaeff, Area=m['A_north'], b=b_north,
                 bs=float(m['bs_north']), bbot=b_north[0])
  channel = SO_ML(y=y, h=m['h'], L=m['L'], Ks=m['Ks'], surflux=m['surflux'].copy(),
                  rest_mask=m['rest_mask'], b_rest=m['b_rest'].copy(), v_pist=m['v_pist'],
                  bs=bs_SO)
  out = {}
  for ii in range(nsteps):
    v = forcing(ii)
    if v is not None:
      basin.bs, north.bs = float(v['bs']), float(v['bs_north'])
      PsiSO.tau = make_func(float(v['tau']), y, 'tau')
      channel.b_rest, channel.surflux = v['b_rest'].copy(), v['surflux'].copy()
    if ii % m['MOC_up_iters'] == 0:
      AMOC.update(b1=basin.b, b2=north.b)
      AMOC.solve()
      [Psi_res_b, Psi_res_n] = AMOC.Psibz(nb=m['nb'])
      PsiSO.update(b=basin.b, bs=channel.bs)
      PsiSO.solve()
    wAb = (Psi_res_b - PsiSO.Psi) * 1e6
    wAN = -Psi_res_n * 1e6
    if PsiSO.Psi[1] < 0:
      basin.bbot = channel.bs[0]
      basin.kappa = kappaeff
    if Psi_res_b[1] > 0 and north.b[0] < basin.b[1] and north.b[0] < channel.bs[0]:
      basin.bbot = north.b[0]
      basin.kappa = kappaeff
    elif PsiSO.Psi[1] >= 0:
      basin.bbot = basin.b[1]
      basin.kappa = kappa
    if Psi_res_n[1] < 0 and basin.b[0] < north.b[1]:
      north.bbot = basin.b[0]
      north.kappa = kappaeff
    else:
      north.bbot = north.b[1]
      north.kappa = kappa
    basin.timestep(wA=wAb, dt=m['dt'], do_conv=True)
    north.timestep(wA=wAN, dt=m['dt'], do_conv=True)
    channel.timestep(b_basin=basin.b, Psi_b=PsiSO.Psi, dt=m['dt'])
    if ii + 1 in snaps:
      out[ii + 1] = dict(b_basin=basin.b.copy(), b_north=north.b.copy(),
                         bs_SO=channel.bs.copy(), Psi=AMOC.Psi.copy(),
                         Psi_SO=PsiSO.Psi.copy(), Psi_iso_b=Psi_res_b.copy(),
                         Psi_iso_n=Psi_res_n.copy(), Psi_s=channel.Psi_s.copy())
  return out


def relerr(a, ref):
  return np.max(np.abs(a - ref)) / np.max(np.abs(ref))


def main():
  out = dict(numpy_version=np.__version__, scipy_version=scipy.__version__,
             reference="pymoc 0.0.1rc5")
  for name in FC.CASES:
    ms, _, t, values = FC.case(name)
    phase = 0 if name == "jn2018" else 1
    runs = {True: [], False: []}
    for j, m in enumerate(ms):
      def forcing(s, j=j, m=m, nudge=False):
        if not FC.applied_at(s, m['MOC_up_iters'], phase):
          return None
        v = FC.member_values(values, t, s * m['dt'], j)
        if nudge and s == 36:
          v['b_rest'] = v['b_rest'] * (1 + 4e-16)
        return v
      if name == "jn2018":
        a = ref_jn2018(m, FC.STEPS, {FC.STEPS}, forcing)[FC.STEPS]
        b = ref_jn2018(m, FC.STEPS, {FC.STEPS}, lambda s: forcing(s, nudge=True))[FC.STEPS]
        own = max(relerr(b[k], a[k]) for k in a)
        print("jn2018 member %d: two roundings of b_rest at step 36 move the reference by %.1e"
              % (j, own))
        assert own <= 0.1 * FC.TOL[name], (j, own)
      for forced in (True, False):
        f = forcing if forced else (lambda s: None)
        if name == "jn2018":
          runs[forced].append(ref_jn2018(m, FC.STEPS, set(FC.SNAPS), f))
        else:
          runs[forced].append(ref_twocol(m, FC.STEPS, set(FC.SNAPS), f, so=name == "twocol_so"))
    for s in FC.SNAPS:
      for k in FC.FIELDS[name]:
        out["%s_s%03d_%s" % (name, s, k)] = np.stack([r[s][k] for r in runs[True]])
    moved = max(relerr(np.stack([r[FC.STEPS][k] for r in runs[True]]),
                       np.stack([r[FC.STEPS][k] for r in runs[False]]))
                for k in FC.FIELDS[name])
    print("%-10s forced vs unforced at step %d: %.3e (needs >= %.1e)"
          % (name, FC.STEPS, moved, 1000 * FC.TOL[name]))
    assert moved >= 1000 * FC.TOL[name], name
    assert all(np.isfinite(v).all() for k, v in out.items() if k.startswith(name))
  path = os.path.join(HERE, "forcing.npz")
  np.savez_compressed(path, **out)
  print("forcing.npz %.1f KiB" % (os.path.getsize(path) / 1024.))


if __name__ == "__main__":
  main()
