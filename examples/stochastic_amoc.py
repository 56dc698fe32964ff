#!/usr/bin/env python3
"""AMOC variability of a Jansen & Nadeau (2018) ensemble under stochastic forcing.

Identical members -- the defaults of run_JansenNadeau_2018.py -- are driven apart by noise that
is generated on the device (pymoc_amd.NoiseForcing, one launch per MOC interval):
  tau       white wind-stress noise over the channel: a new deviate every year
  bs_north  red noise on the surface buoyancy of the northern sinking region, with a decorrelation
            time of `--tau-corr` years
A pymoc_amd.IndexRecorder keeps every member's AMOC maximum below 500 m at every overturning
update (once a year).  Printed: the ensemble mean and spread (standard deviation over the members)
of that index per decade.  Every member has its own deviates (they are counted by the member's
global index), and a run is reproduced by its `--seed` whatever the number of members.

    python examples/stochastic_amoc.py --members 64 --years 200
    python examples/stochastic_amoc.py --time      # what the noise costs
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import Event, LaunchTimer, synchronize
from pymoc_amd.steady import YEAR

SPECS = [("amoc", "max", "Psi", dict(zhi=-500.))]


def identical_members(n, nz, dt_days):
  """n copies of one member (config5 sweeps parameters; here only the noise differs)."""
  one = configs.config5(N=1, nz=nz, dt_days=dt_days)
  cfg = dict(one)
  for key in pymoc_amd.JN2018Ensemble.MEMBER_KEYS:
    a = np.asarray(one[key])
    if a.ndim >= 1 and a.shape[0] == 1:
      cfg[key] = np.repeat(a, n, axis=0)
  return cfg


def noise(args, bs_north=True):
  targets = dict(tau=dict(sigma=args.sigma_tau))
  if bs_north:
    targets["bs_north"] = dict(sigma=args.sigma_bs_north, tau_corr=args.tau_corr * YEAR)
  return pymoc_amd.NoiseForcing(args.seed, **targets)


def _median_ms(spans):
  v = sorted(e0.elapsed_ms(e1) for e0, e1 in spans)
  return v[len(v) // 2]


def _spans(fn, reps):
  out = []
  for _ in range(reps):
    e0, e1 = Event(), Event()
    e0.record()
    fn()
    e1.record()
    out.append((e0, e1))
  synchronize()
  return out


def time_it(args):
  """hipEvent medians at `--members` members: pm_forcing_noise alone (the example's two targets),
  and one MOC interval of run() without noise=, with the example's noise, and with its wind noise
  alone (noise on bs_north makes the columns test every bs operand, and moves the depth the
  northern column convects to: what the step loop does with the values, not the launch)."""
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])
  null = LaunchTimer().null_span_ms()
  out = {}
  for name, kw in (("plain", {}), ("noisy", dict(noise=noise(args))),
                   ("wind", dict(noise=noise(args, bs_north=False)))):
    ens = pymoc_amd.JN2018Ensemble(cfg, **kw)
    ens.run(4 * M)  # warm-up
    out[name] = _median_ms(_spans(lambda: ens.run(M), args.reps)) - null
    if name == "noisy":
      k = [1000]

      def launch():
        k[0] += 1
        ens.noise.apply(k[0], M * ens.dt)
      out["launch"] = _median_ms(_spans(launch, 4 * args.reps)) - null
  us = lambda key: 1e3 * out[key]  # noqa: E731
  print("members %d nz %d ny %d MOC_up_iters %d (empty span %.1f us subtracted)"
        % (args.members, args.nz, cfg["y"].size, M, 1e3 * null))
  print("pm_forcing_noise, tau + bs_north of every member: %.1f us" % us("launch"))
  print("one MOC interval: %.1f us without noise, %.1f us with it (%+.1f us, %.2f %%), %.1f us with "
        "the wind noise alone (%+.1f us, %.2f %%)"
        % (us("plain"), us("noisy"), us("noisy") - us("plain"),
           100. * (out["noisy"] - out["plain"]) / out["plain"], us("wind"),
           us("wind") - us("plain"), 100. * (out["wind"] - out["plain"]) / out["plain"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=None, help="default 64 (4096 with --time)")
  ap.add_argument("--years", type=int, default=200)
  ap.add_argument("--nz", type=int, default=None, help="default 81 (200 with --time)")
  ap.add_argument("--dt-days", type=float, default=None, help="default 30 (10 with --time)")
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--print-years", type=int, default=10, help="years per printed row")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  timing = args.time
  args.members = args.members or (4096 if timing else 64)
  args.nz = args.nz or (200 if timing else 81)
  args.dt_days = args.dt_days or (10. if timing else 30.)
  if timing:
    return time_it(args)
  cfg = identical_members(args.members, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  ens = pymoc_amd.JN2018Ensemble(cfg, noise=noise(args))
  rec = pymoc_amd.IndexRecorder(ens, SPECS, M, args.years)  # a sample at the top of every year
  ens.run(args.years * M)
  amoc = rec.values["amoc"]  # [members, years]
  print("%d identical members, %d years; noise seed %d: tau white, sigma %g N/m2; bs_north red, "
        "sigma %g m/s2, decorrelation %g years" % (ens.n, args.years, args.seed, args.sigma_tau,
                                                   args.sigma_bs_north, args.tau_corr))
  print("AMOC maximum below 500 m [Sv]: ensemble mean and spread per %d years" % args.print_years)
  step = max(args.print_years, 1)
  for y0 in range(0, args.years, step):
    blk = amoc[:, y0:min(y0 + step, args.years)]
    ok = np.isfinite(blk).all(axis=1)
    mean = blk[ok].mean() if ok.any() else np.nan
    spread = blk[ok].mean(axis=1).std() if ok.any() else np.nan
    print("  years %4d-%4d  %10.5f %10.5f%s"
          % (y0, min(y0 + step, args.years) - 1, mean, spread,
             "" if ok.all() else "   (%d members non-finite)" % (~ok).sum()))
  bad = ens.nonfinite_members()
  if bad.size:
    print("%d members went non-finite" % bad.size)


if __name__ == "__main__":
  main()
