#!/usr/bin/env python3
"""Two-basin equilibria of a parameter sweep, each member taken when it is reached.

examples/twobasin_NadeauJansen.py's loop is commented "loop to iteratively find equilibrium
solution" and runs a fixed 4000 years, because it has no test for "done".
pymoc_amd.run_to_steady(TwoBasinSweep, ...) checks every member's drift every `--check-every` steps
and retires the members that have settled.  Members are those of configs.config_twobasin (tau, K
and A_Pac swept).

Above about nz = 125 the script's forward-Euler columns cannot take its own dt = 30 d;
`--implicit --nz 200` runs the sweep there with backward-Euler columns (TwoBasinSweep(scheme=
"implicit"): an extension with no reference counterpart, a tolerance path).

    python examples/twobasin_equilibrium.py --members 2048 --tol 1e-7
    python examples/twobasin_equilibrium.py --implicit --nz 200 --members 256
    python examples/twobasin_equilibrium.py --time    # hipEvent medians, one run
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


def make_cfg(n, nz, ny, dt_days):
  return dict(configs.config_twobasin(N=n, nz=nz, ny=ny), dt=DAY * dt_days)


def _median_ms(fn, reps=15, warm=3):
  ms = []
  for _ in range(reps + warm):
    e0, e1 = Event(), Event()
    e0.record()
    fn()
    e1.record()
    e1.sync()
    ms.append(e0.elapsed_ms(e1))
  return float(np.median(ms[warm:]))


def time_intervals(n, nz, ny, dt_days, dt_explicit_days):
  """Median hipEvent time in us of one launch interval -- MOC_up_iters steps and the update they
  end on -- of n members: explicit, implicit with the forcing formed in the kernel, implicit with
  pm_twobasin_forcing and the array kernel."""
  out = {}
  todo = (("explicit", dt_explicit_days, {}, None),
          ("implicit, forcing formed in the kernel", dt_days, dict(scheme="implicit"), True),
          ("implicit, forcing launch + array", dt_days, dict(scheme="implicit"), False))
  for name, days, kw, formed in todo:
    ens = pymoc_amd.TwoBasinSweep(make_cfg(n, nz, ny, days), **kw)
    if formed is not None:
      ens.IMPLICIT_FORMED = formed
    ens.run(1)  # step 0 and its update: whole intervals from here
    out[name] = 1e3 * _median_ms(lambda: ens.run(ens.M))
    bad = int(ens.nonfinite_members().size)
    if bad:
      print("  (%s: %d members non-finite after the timed intervals)" % (name, bad))
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--members", type=int, default=256)
  ap.add_argument("--years", type=float, default=4000., help="cap (the script's run length)")
  ap.add_argument("--steps", type=int, default=None, help="cap in steps instead of --years")
  ap.add_argument("--nz", type=int, default=80)
  ap.add_argument("--ny", type=int, default=51)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--implicit", action="store_true", help="backward-Euler columns")
  ap.add_argument("--tol", type=float, default=1e-7,
                  help="drift tolerance: buoyancy change per 360-day year (m s^-2 / yr)")
  ap.add_argument("--check-every", type=int, default=None,
                  help="steps between checks (default 10 MOC_up_iters = 20 years)")
  ap.add_argument("--consecutive", type=int, default=2)
  ap.add_argument("--time", action="store_true", help="print hipEvent medians as well")
  ap.add_argument("--time-members", type=int, default=2048)
  a = ap.parse_args()

  cfg = make_cfg(a.members, a.nz, a.ny, a.dt_days)
  dz = float(np.min(np.diff(cfg["z"])))
  kmax = float(np.max(cfg["kappa"]))
  r = kmax * cfg["dt"] / dz ** 2
  print("nz = %d, dz = %.1f m, max kappa = %.2e: kappa dt / dz^2 = %.2f at %g d%s"
        % (a.nz, dz, kmax, r, a.dt_days,
           "" if a.implicit or r <= 0.5 else "  (beyond forward Euler: use --implicit)"))
  kw = dict(scheme="implicit") if a.implicit else {}
  max_steps = a.steps if a.steps is not None else int(np.ceil(a.years * YEAR / cfg["dt"]))
  t0 = time.perf_counter()
  res = pymoc_amd.run_to_steady(pymoc_amd.TwoBasinSweep, cfg, a.tol, max_steps,
                                check_every=a.check_every, consecutive=a.consecutive, **kw)
  wall = time.perf_counter() - t0
  c = res.counts()
  cap = a.members * max_steps
  print("%d members, %s columns, cap %d steps (%.0f years), check every %d steps, tol %.1e / yr: "
        "%d converged, %d non-finite, %d capped; %.2f s wall"
        % (a.members, "implicit" if a.implicit else "explicit", max_steps,
           max_steps * cfg["dt"] / YEAR, res.check_every, a.tol, c["converged"], c["nonfinite"],
           c["maxsteps"], wall))
  print("member-steps: %d of %d (%.1f%%), %d saved; %d compactions"
        % (res.member_steps, cap, 100. * res.member_steps / cap, cap - res.member_steps,
           len(res.compactions)))
  conv = res.status == pymoc_amd.steady.CONVERGED
  if conv.any():
    y = res.years[conv]
    print("retirement years: min %.0f  median %.0f  max %.0f" % (y.min(), np.median(y), y.max()))
    amoc = res.fields["Psi_AMOC"][conv].max(axis=1)
    print("equilibrium max AMOC: %.2f .. %.2f Sv over the converged members"
          % (amoc.min(), amoc.max()))
  else:
    print("retirement years: none converged; equilibrium max AMOC: n/a")

  if a.time:
    n, ny = a.time_members, a.ny
    nz_i = max(a.nz, 200)   # the implicit scheme where it is needed: the script's dt at nz = 200
    dt_exp = 4.             # what forward Euler can take there (tests/twobasin_cases.SHAPES)
    t = time_intervals(n, nz_i, ny, a.dt_days, dt_exp)
    for k, v in t.items():
      print("%d members x nz = %d, one interval (24 steps + update): %-40s %8.1f us"
            % (n, nz_i, k, v))
    formed, array = (t["implicit, forcing formed in the kernel"],
                     t["implicit, forcing launch + array"])
    print("  formed / array = %.3f;  per model year: explicit at %g d %.1f us, implicit at %g d "
          "%.1f us" % (formed / array, dt_exp, t["explicit"] * 360. / (24 * dt_exp), a.dt_days,
                       min(formed, array) * 360. / (24 * a.dt_days)))
    # run() for the script's 4000 years against run_to_steady, the main run's shape
    cfg_t = make_cfg(n, a.nz, ny, a.dt_days)
    steps = int(np.ceil(4000. * YEAR / cfg_t["dt"]))
    ens = pymoc_amd.TwoBasinSweep(cfg_t, **kw)
    ens.run(1 + ens.M)  # warm-up
    synchronize()
    t0 = time.perf_counter()
    ens.run(steps - ens.ii)
    synchronize()
    full = time.perf_counter() - t0
    t0 = time.perf_counter()
    rs = pymoc_amd.run_to_steady(pymoc_amd.TwoBasinSweep, cfg_t, a.tol, steps,
                                 check_every=a.check_every, consecutive=a.consecutive, **kw)
    steady = time.perf_counter() - t0
    print("%d members x nz = %d: run() of 4000 years (%d steps) %.2f s;  run_to_steady %.2f s "
          "(%.1f%% of the member-steps, %d converged)"
          % (n, a.nz, steps, full, steady, 100. * rs.member_steps / (n * steps),
             rs.counts()["converged"]))
  synchronize()


if __name__ == "__main__":
  main()
