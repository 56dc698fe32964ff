#!/usr/bin/env python3
"""Two-column ensembles with the implicit column step: dt = 30 d at nz = 200.

The reference's Column.vertadvdiff is forward Euler: stable for kappa dt / dz^2 <= 1/2 only.  On a
200-level grid (dz = 20.1 m) a diffusivity of 1.2e-4 m^2/s allows dt <= 19 d, so the explicit
scheme cannot take the 30-day step the reference's scripts use at nz = 100.  `scheme="implicit"`
(backward Euler of the same discretisation, pm_column_steps_implicit: an extension with no
reference counterpart, a tolerance path) has no such limit.  This script runs the same members
both ways -- implicit at `--dt-days` (default 30), explicit at its stable `--dt-explicit-days`
(default 10) -- and prints how far apart the two end states are.

    python examples/implicit_columns.py --members 16 --years 50
    python examples/implicit_columns.py --time   # hipEvent medians of both column steps
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import DeviceArray, Event, synchronize
from pymoc_amd.steady import YEAR

DAY = 86400.0


def members(n, nz, dt_days):
  cfg = dict(configs.config3(N=n, nz=nz))
  # a thermocline diffusivity that rules out the 30-day explicit step at nz = 200
  z = cfg["z"]
  cfg["kappa"] = cfg["kappa"] + 1.0e-4 * np.exp(z / 500.0)[None, :]
  cfg["dt"] = dt_days * DAY
  return cfg


def run(cfg, years, scheme):
  ens = pymoc_amd.TwoColEnsemble(cfg, scheme=scheme)
  nsteps = int(round(years * YEAR / cfg["dt"]))
  ens.run(nsteps)
  st = ens.state()
  bad = int(ens.cols.get_nonfinite().reshape(2, -1).any(axis=0).sum())
  return st, nsteps, bad


def time_steps(ncols, nz, nsteps=24, reps=15):
  """Median hipEvent time of one launch of `nsteps` column steps, both schemes, in us per step."""
  rng = np.random.default_rng(7)
  z = np.linspace(-4000.0, 0.0, nz)
  kappa = 2e-5 + 1e-4 * np.exp(z / 500.0)
  b0 = 0.03 * np.exp(z / 300.0)[None, :] * rng.uniform(0.8, 1.0, (ncols, 1))
  wA = 1e6 * np.sin(np.pi * z / 4000.0)[None, :] * rng.uniform(0.5, 1.5, (ncols, 1))
  batch = pymoc_amd.ColumnBatch(z, kappa, 8e13, b0, bs=0.03, bbot=-0.001,
                                do_conv=np.arange(ncols) % 2 == 1)
  wA_d = DeviceArray.from_host(wA)
  dt = 0.4 * (z[1] - z[0]) ** 2 / kappa.max()  # stable for both
  out = {}
  for scheme in ("explicit", "implicit"):
    ms = []
    for _ in range(reps + 3):
      batch.set_b(b0)
      e0, e1 = Event(), Event()
      e0.record()
      batch.steps(wA_d, dt, nsteps, scheme=scheme)
      e1.record()
      e1.sync()
      ms.append(e0.elapsed_ms(e1))
    out[scheme] = 1e3 * float(np.median(ms[3:])) / nsteps
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--members", type=int, default=16)
  ap.add_argument("--nz", type=int, default=200)
  ap.add_argument("--years", type=float, default=50.0)
  ap.add_argument("--dt-days", type=float, default=30.0)
  ap.add_argument("--dt-explicit-days", type=float, default=10.0)
  ap.add_argument("--time", action="store_true")
  a = ap.parse_args()

  cfg_imp = members(a.members, a.nz, a.dt_days)
  imp, n_imp, bad_imp = run(cfg_imp, a.years, "implicit")
  exp, n_exp, bad_exp = run(members(a.members, a.nz, a.dt_explicit_days), a.years, "explicit")
  dz = float(np.min(np.diff(cfg_imp["z"])))
  kmax = cfg_imp["kappa"].max()  # over the members that run
  print("nz = %d, dz = %.1f m, max kappa = %.2e: kappa dt / dz^2 = %.2f at %g d, %.2f at %g d"
        % (a.nz, dz, kmax, kmax * a.dt_days * DAY / dz ** 2, a.dt_days,
           kmax * a.dt_explicit_days * DAY / dz ** 2, a.dt_explicit_days))
  print("implicit: %d steps of %g d, %d non-finite members" % (n_imp, a.dt_days, bad_imp))
  print("explicit: %d steps of %g d, %d non-finite members" % (n_exp, a.dt_explicit_days, bad_exp))
  for f in ("b_basin", "b_north", "Psi"):
    d = np.max(np.abs(imp[f] - exp[f])) / np.max(np.abs(exp[f]))
    print("  max |implicit - explicit| / max |explicit| of %-8s %.2e" % (f, d))
  if a.time:
    for ncols, nz in ((1024, 100), (4096, 200)):
      t = time_steps(ncols, nz)
      print("%d x nz = %d: explicit %.3f us / step (%.3e column-steps/s), implicit %.3f us / step "
            "(%.3e column-steps/s), ratio %.2f"
            % (ncols, nz, t["explicit"], ncols / t["explicit"] * 1e6, t["implicit"],
               ncols / t["implicit"] * 1e6, t["implicit"] / t["explicit"]))
      if nz == 200:
        cost = t["implicit"] / t["explicit"]
        steps = a.dt_days / a.dt_explicit_days
        print("  model years per second of %d columns: explicit at %g d %.1f, implicit at %g d %.1f"
              % (ncols, a.dt_explicit_days, a.dt_explicit_days * DAY / YEAR / (t["explicit"] * 1e-6),
                 a.dt_days, a.dt_days * DAY / YEAR / (t["implicit"] * 1e-6)))
        print("  (explicit steps needed) / (implicit steps needed) = %.2f, "
              "(implicit us per step) / (explicit us per step) = %.2f: the implicit step %s here"
              % (steps, cost, "pays" if steps > cost else "does not pay"))
  synchronize()


if __name__ == "__main__":
  main()
