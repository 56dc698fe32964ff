#!/usr/bin/env python3
"""Jansen & Nadeau (2018) equilibria of a parameter sweep, each member taken when it is reached.

run_JansenNadeau_2018.py steps for 12 000 years (:96-97) because it has no test for "done";
pymoc_amd.run_to_steady checks every member's drift every `--check-every` steps and retires the
members that have settled, so the sweep costs what its members need rather than what the slowest
one (or a guessed length) needs.  Members run at the script's defaults (nz=81, dt=30 d) with
config 5's swept parameters.

    python examples/jn2018_equilibrium.py --members 4096 --tol 1e-6 --out /tmp/eq.npz
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.steady import YEAR


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=4096)
  ap.add_argument("--years", type=float, default=12000., help="cap (the script's run length)")
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--tol", type=float, default=1e-6,
                  help="drift tolerance: buoyancy change per 360-day year (m s^-2 / yr)")
  ap.add_argument("--check-every", type=int, default=None,
                  help="steps between checks (default 10 MOC_up_iters = 10 years)")
  ap.add_argument("--consecutive", type=int, default=2)
  ap.add_argument("--out", default=None, help=".npz file for the result")
  args = ap.parse_args()
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])
  max_steps = int(np.ceil(args.years * YEAR / cfg["dt"]))
  t0 = time.perf_counter()
  res = pymoc_amd.run_to_steady(pymoc_amd.JN2018Ensemble, cfg, args.tol, max_steps,
                                check_every=args.check_every, consecutive=args.consecutive)
  wall = time.perf_counter() - t0
  c = res.counts()
  conv = res.status == pymoc_amd.steady.CONVERGED
  print("%d members, cap %d steps (%.0f years), check every %d steps, tol %.1e / yr: "
        "%d converged, %d non-finite, %d capped; %.2f s wall, %.3g member-steps (%.1f%% of the "
        "cap)" % (args.members, max_steps, max_steps * cfg["dt"] / YEAR, res.check_every,
                  args.tol, c["converged"], c["nonfinite"], c["maxsteps"], wall,
                  res.member_steps, 100. * res.member_steps / (args.members * max_steps)))
  if conv.any():
    y = res.years[conv]
    print("convergence years: min %.0f  median %.0f  max %.0f" % (y.min(), np.median(y), y.max()))
    amoc = res.fields["Psi"][conv].max(axis=1)
    print("equilibrium max AMOC: %.2f .. %.2f Sv over the converged members"
          % (amoc.min(), amoc.max()))
  else:
    print("convergence years: none converged; equilibrium max AMOC: n/a")
  if args.out:
    np.savez(args.out, status=res.status, steps=res.steps, years=res.years, drift=res.drift,
             tol=args.tol, dt=cfg["dt"], MOC_up_iters=M, check_every=res.check_every,
             member_steps=res.member_steps, compactions=np.array(res.compactions).reshape(-1, 3),
             tau=cfg["tau"], KGM=cfg["KGM"], db=cfg["scalars"]["db"], B=cfg["scalars"]["B"],
             **res.fields)


if __name__ == "__main__":
  main()
