#!/usr/bin/env python3
"""Jansen & Nadeau ensembles with implicit columns: the script's dt = 30 d at nz = 200.

run_JansenNadeau_2018.py steps its columns with forward Euler.  On a 200-level grid that scheme
cannot take the script's own dt = 30 d (kappa dt / dz^2 > 1/2), so JN2018Ensemble runs config 5
at 10 d and takes three times the steps.  JN2018ImplicitEnsemble advances both columns by backward
Euler inside the same fused loop (pm_jn2018_steps_implicit: an extension with no reference
counterpart, a tolerance path) and has no such limit.  This script runs the same members both
ways over the same model time -- implicit at `--dt-days` (default 30), explicit at
`--dt-explicit-days` (default 10) -- and prints how far apart the two end states are.

    python examples/jn2018_implicit.py --members 16 --years 50
    python examples/jn2018_implicit.py --time   # hipEvent medians of 36-step launches, 4096 members
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import Event, synchronize
from pymoc_amd.steady import YEAR

DAY = 86400.0


def run(cls, cfg, years, **kw):
  ens = cls(cfg, **kw)
  nsteps = int(round(years * YEAR / cfg["dt"]))
  synchronize()
  t0 = time.perf_counter()
  ens.run(nsteps)
  synchronize()
  wall = time.perf_counter() - t0
  return ens.state(), nsteps, int(ens.nonfinite_members().size), wall


def time_launches(n, nz, ny, dt_days, dt_explicit_days, nsteps=36, reps=15):
  """Median hipEvent time per step, in us, of `nsteps` steps between two MOC updates: the explicit
  fused loop, the implicit fused loop (one launch each) and the implicit stepwise sequence
  (3 launches per step)."""
  out = {}
  todo = (("explicit fused", pymoc_amd.JN2018Ensemble, dt_explicit_days, {}),
          ("implicit fused", pymoc_amd.JN2018ImplicitEnsemble, dt_days, {}),
          ("implicit stepwise", pymoc_amd.JN2018ImplicitEnsemble, dt_days, dict(fused=False)))
  for name, cls, days, kw in todo:
    ens = cls(configs.config5(N=n, nz=nz, ny=ny, dt_days=days), **kw)
    ens.moc_update()
    ms = []
    for _ in range(reps + 3):
      e0, e1 = Event(), Event()
      e0.record()
      if kw:
        for _ in range(nsteps):
          ens._step()
      else:
        ens._fused_steps(nsteps)
      e1.record()
      e1.sync()
      ms.append(e0.elapsed_ms(e1))
    out[name] = 1e3 * float(np.median(ms[3:])) / nsteps
    bad = int(ens.nonfinite_members().size)
    if bad:
      print("  (%s: %d members non-finite after the timed launches)" % (name, bad))
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--members", type=int, default=16)
  ap.add_argument("--nz", type=int, default=200)
  ap.add_argument("--ny", type=int, default=51)
  ap.add_argument("--years", type=float, default=50.0)
  ap.add_argument("--dt-days", type=float, default=30.0)
  ap.add_argument("--dt-explicit-days", type=float, default=10.0)
  ap.add_argument("--time", action="store_true")
  a = ap.parse_args()

  mk = lambda n, days: configs.config5(N=n, nz=a.nz, ny=a.ny, dt_days=days)  # noqa: E731
  cfg_imp = mk(a.members, a.dt_days)
  imp, n_imp, bad_imp, _ = run(pymoc_amd.JN2018ImplicitEnsemble, cfg_imp, a.years)
  exp, n_exp, bad_exp, _ = run(pymoc_amd.JN2018Ensemble, mk(a.members, a.dt_explicit_days), a.years)
  dz = float(np.min(np.diff(cfg_imp["z"])))
  kmax = max(np.max(cfg_imp["kappa"]), np.max(cfg_imp["kappaeff"]))
  print("nz = %d, dz = %.1f m, max kappa = %.2e: kappa dt / dz^2 = %.2f at %g d, %.2f at %g d"
        % (a.nz, dz, kmax, kmax * a.dt_days * DAY / dz ** 2, a.dt_days,
           kmax * a.dt_explicit_days * DAY / dz ** 2, a.dt_explicit_days))
  print("implicit: %d steps of %g d, %d non-finite members" % (n_imp, a.dt_days, bad_imp))
  print("explicit: %d steps of %g d, %d non-finite members" % (n_exp, a.dt_explicit_days, bad_exp))
  fields = ("b_basin", "b_north", "bs_SO", "Psi")
  ok = np.all([np.isfinite(s[f]).all(axis=1) for s in (imp, exp) for f in fields], axis=0)
  print("compared on the %d of %d members whose state is finite in both runs" % (ok.sum(), ok.size))
  for f in fields:
    d = np.max(np.abs(imp[f][ok] - exp[f][ok])) / np.max(np.abs(exp[f][ok])) if ok.any() else np.nan
    print("  max |implicit - explicit| / max |explicit| of %-8s %.2e" % (f, d))
  if a.time:
    n, nz, ny = 4096, 200, 51
    t = time_launches(n, nz, ny, a.dt_days, a.dt_explicit_days)
    for k in ("explicit fused", "implicit fused", "implicit stepwise"):
      print("%d x nz = %d x ny = %d, 36 steps: %-17s %.3f us / step" % (n, nz, ny, k, t[k]))
    print("  fused implicit / stepwise implicit = %.3f" % (t["implicit fused"] / t["implicit stepwise"]))
    steps = a.dt_days / a.dt_explicit_days
    cost = t["implicit fused"] / t["explicit fused"]
    print("  (explicit steps needed) / (implicit steps needed) = %.2f, (implicit us per step) / "
          "(explicit us per step) = %.2f: pay-off ratio %.2f" % (steps, cost, steps / cost))
    years = 10.0
    for name, cls, days in (("explicit", pymoc_amd.JN2018Ensemble, a.dt_explicit_days),
                            ("implicit", pymoc_amd.JN2018ImplicitEnsemble, a.dt_days)):
      cfg = mk(n, days)
      run(cls, cfg, 1.0)  # warm-up
      _, ns, bad, wall = run(cls, cfg, years)
      print("  run() of %g model years, %d members: %s at %g d: %d steps, %.3f ms, %d non-finite"
            % (years, n, name, days, ns, 1e3 * wall, bad))
  synchronize()


if __name__ == "__main__":
  main()
