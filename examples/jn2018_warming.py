#!/usr/bin/env python3
"""A Jansen & Nadeau (2018) parameter sweep under a ramped surface warming and a wind step.

The reference's transient experiments assign `basin.bs`, `north.bs`, `channel.b_rest` and
`PsiSO.tau` as functions of time at the top of the user loop.  Here the whole ensemble gets them
from one pymoc_amd.ForcingSchedule -- piecewise-linear knots, evaluated on the device at the first
step of every MOC interval -- while JN2018Diagnostics samples the members where the script does.
Every member warms by its own amount between `--ramp-start` and `--ramp-end` years (surface
buoyancy of the basin, the northern column and the channel's restoring profile alike) and its
wind stress steps up by 25 % within one year at `--wind-year`.  Printed: each recorded member's
maximum AMOC at the recorded samples.

    python examples/jn2018_warming.py --members 64 --years 200
    python examples/jn2018_warming.py --time      # what the schedule costs
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import Event, LaunchTimer, synchronize
from pymoc_amd.diagnostics import JN2018Diagnostics
from pymoc_amd.steady import YEAR


def schedule(cfg, ramp=(20., 120.), wind_year=60., warming=None):
  """The five targets of a JN2018Ensemble, every one per member: knots at the ramp's ends and
  around the wind step."""
  n = cfg["b_basin0"].shape[0]
  db = np.linspace(1e-3, 4e-3, n) if warming is None else np.asarray(warming, dtype=np.float64)
  t = np.array([ramp[0], wind_year, wind_year + 1., ramp[1]]) * YEAR
  if not (np.diff(t) > 0).all():
    raise ValueError("the wind step must lie inside the ramp")
  w = (t - t[0]) / (t[-1] - t[0])  # share of the warming reached at each knot
  up = lambda v: np.asarray(v)[None, :] + w[:, None] * db[None, :]  # noqa: E731
  rest = np.asarray(cfg["rest_mask"], dtype=np.float64) * np.ones_like(cfg["b_rest"])
  b_rest = cfg["b_rest"][None] + w[:, None, None] * db[None, :, None] * rest[None]
  tau = np.asarray(cfg["tau"])[None] * np.array([1., 1., 1.25, 1.25])[:, None]
  surflux = np.repeat(np.asarray(cfg["surflux"])[None], t.size, axis=0)
  return pymoc_amd.ForcingSchedule(t, bs=up(cfg["bs"]), bs_north=up(cfg["bs_north"]), tau=tau,
                                   b_rest=b_rest, surflux=surflux)


def _median_ms(spans):
  v = sorted(e0.elapsed_ms(e1) for e0, e1 in spans)
  return v[len(v) // 2]


def time_it(args):
  """hipEvent medians at `--members` members: pm_forcing_apply alone (all five targets per
  member), and one MOC interval of run() with and without the schedule."""
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])
  sched = schedule(cfg, ramp=(0.5, 400.), wind_year=200.)
  null = LaunchTimer().null_span_ms()
  out = {}
  for name, kw in (("plain", {}), ("scheduled", dict(forcing=sched))):
    ens = pymoc_amd.JN2018Ensemble(cfg, **kw)
    ens.run(4 * M)  # warm-up
    spans = []
    for _ in range(args.reps):
      e0, e1 = Event(), Event()
      e0.record()
      ens.run(M)
      e1.record()
      spans.append((e0, e1))
    synchronize()
    out[name] = _median_ms(spans) - null
    if kw:
      spans = []
      for k in range(4 * args.reps):
        e0, e1 = Event(), Event()
        e0.record()
        ens._forcing.apply((7.3 + k) * YEAR)  # between two knots: both slabs are read
        e1.record()
        spans.append((e0, e1))
      synchronize()
      out["apply"] = _median_ms(spans) - null
  ny = cfg["y"].size
  mb = 3 * args.members * (3 + 2 * ny) * 8 / 1e6
  print("members %d nz %d ny %d MOC_up_iters %d (empty span %.1f us subtracted)"
        % (args.members, args.nz, ny, M, 1e3 * null))
  print("pm_forcing_apply, 5 targets per member: %.1f us (%.1f MB moved, %.2f TB/s)"
        % (1e3 * out["apply"], mb, mb / out["apply"] / 1e3 if out["apply"] > 0 else 0.))
  print("one MOC interval: %.1f us without a schedule, %.1f us with one (%+.1f us, %.1f %%)"
        % (1e3 * out["plain"], 1e3 * out["scheduled"], 1e3 * (out["scheduled"] - out["plain"]),
           100. * (out["scheduled"] - out["plain"]) / out["plain"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=None, help="default 64 (4096 with --time)")
  ap.add_argument("--years", type=float, default=200.)
  ap.add_argument("--nz", type=int, default=None, help="default 81 (200 with --time)")
  ap.add_argument("--dt-days", type=float, default=None, help="default 30 (10 with --time)")
  ap.add_argument("--ramp-start", type=float, default=20.)
  ap.add_argument("--ramp-end", type=float, default=120.)
  ap.add_argument("--wind-year", type=float, default=60.)
  ap.add_argument("--diag-years", type=int, default=20, help="years between samples")
  ap.add_argument("--show", type=int, default=4, help="members to print")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--reps", type=int, default=25)
  args = ap.parse_args()
  timing = args.time
  args.members = args.members or (4096 if timing else 64)
  args.nz = args.nz or (200 if timing else 81)
  args.dt_days = args.dt_days or (10. if timing else 30.)
  if timing:
    return time_it(args)
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  total = int(args.years) * M
  ens = pymoc_amd.JN2018Ensemble(
      cfg, forcing=schedule(cfg, (args.ramp_start, args.ramp_end), args.wind_year))
  show = np.unique(np.linspace(0, args.members - 1, min(args.show, args.members)).astype(int))
  ens.recorder = JN2018Diagnostics(ens, args.diag_years * M, total, members=show)
  ens.run(total)
  amoc = ens.recorder.AMOC.max(axis=1)  # [recorded member, sample]
  years = np.arange(amoc.shape[1]) * args.diag_years
  print("max AMOC (Sv) of members %s; warming ramps over years %g-%g, wind +25 %% at year %g"
        % (list(show), args.ramp_start, args.ramp_end, args.wind_year))
  print("  year " + " ".join("%8d" % j for j in show))
  for k, yr in enumerate(years):
    print("%6d " % yr + " ".join("%8.3f" % amoc[i, k] for i in range(show.size)))
  bad = ens.nonfinite_members()
  if bad.size:
    print("%d members went non-finite" % bad.size)


if __name__ == "__main__":
  main()
