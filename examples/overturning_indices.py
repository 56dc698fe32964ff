#!/usr/bin/env python3
"""Overturning indices of a whole warming sweep, recorded on the device while it runs.

The sweep is examples/jn2018_warming.py's: every member of a Jansen & Nadeau (2018) ensemble warms
by its own amount over a ramp and its wind steps up by 25 %.  That script records full profiles of
four members every 20 years and takes `AMOC.max(axis=1)` on the host.  Here a
pymoc_amd.IndexRecorder samples ALL members at EVERY overturning update (once a year) -- one launch
per sample into a device-resident series, a few dozen kilobytes per sample -- and keeps:
  amoc      the AMOC maximum below 500 m, and the depth it sits at
  z_zero    the depth of the sign change beneath it (the top of the abyssal cell; while the AMOC
            cell reaches the bottom, where Psi = 0, this is the bottom)
  abyss     the minimum of Psi below 2500 m (0 until an abyssal cell forms)
  b_1000    the basin's buoyancy at 1000 m
  b_upper   the mean basin buoyancy of the upper 1000 m
Printed: ensemble quantiles (10 / 50 / 90 %) of each, per decade.

    python examples/overturning_indices.py --members 64 --years 200
    python examples/overturning_indices.py --time     # what a sample costs
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import Event, LaunchTimer, synchronize
from pymoc_amd.diagnostics import JN2018Diagnostics
from jn2018_warming import schedule

SPECS = [("amoc", "max", "Psi", dict(zhi=-500.)),
         ("z_zero", "cross", "Psi", dict(level=0., zhi=-1000.)),
         ("abyss", "min", "Psi", dict(zhi=-2500.)),
         ("b_1000", "at", "b_basin", dict(x0=-1000.)),
         ("b_upper", "mean", "b_basin", dict(zlo=-1000.))]
# --time measures a table of 8
MORE = [("so_max", "max", "Psi_SO", {}), ("bn_1000", "at", "b_north", dict(x0=-1000.)),
        ("psi_min", "min", "Psi", {})]


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
  """hipEvent medians at `--members` members and 8 indices: the sample launch alone; one MOC
  interval of run() without a recorder, with an IndexRecorder at every update, and with the only
  other route to the same numbers, JN2018Diagnostics over all members at the same cadence; that
  recorder's own launch and the bytes either stores per sample."""
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])
  n, reps = args.members, args.reps
  warm, nrec = 4, 4 + args.reps + 1
  null = LaunchTimer().null_span_ms()
  out = {}
  for name in ("plain", "indices", "profiles"):
    ens = pymoc_amd.JN2018Ensemble(cfg)
    if name == "indices":
      rec = pymoc_amd.IndexRecorder(ens, SPECS + MORE, M, nrec)
    if name == "profiles":
      ens.recorder = JN2018Diagnostics(ens, M, nrec * M)
    ens.run(warm * M)
    out[name] = _median_ms(_spans(lambda: ens.run(M), reps)) - null
    if name == "indices":
      k = nrec - 1
      dst = (rec._values.ptr + 8 * k * rec._rec, rec._pos.ptr + 4 * k * rec._rec)
      out["sample"] = _median_ms(_spans(lambda: rec.table.sample(out=dst), 4 * reps)) - null
      out["index_bytes"] = 12 * rec._rec
    if name == "profiles":
      ts = ens.recorder.ts
      src = dict(AMOC=ens.tw.Psi, AMOC_b=ens.tw.psib, bgrid=ens.tw.bgrid, b_basin=ens.b_basin,
                 b_north=ens.b_north, bs_SO=ens.ml.bs, Psi_SO=ens.so.Psi)
      out["pack"] = _median_ms(_spans(lambda: ts.append(src, k=nrec - 1), 4 * reps)) - null
      out["profile_bytes"] = 8 * ts.rec
  us = lambda key: 1e3 * out[key]  # noqa: E731
  print("members %d nz %d ny %d nb %d MOC_up_iters %d, %d indices (empty span %.1f us subtracted)"
        % (n, args.nz, cfg["y"].size, int(cfg["nb"]), M, len(SPECS + MORE), 1e3 * null))
  print("pm_row_indices, one sample: %.1f us, %d bytes stored per sample" % (us("sample"), out["index_bytes"]))
  print("one MOC interval: %.1f us without a recorder, %.1f us with an IndexRecorder (%+.1f us, %.2f %%)"
        % (us("plain"), us("indices"), us("indices") - us("plain"),
           100. * (out["indices"] - out["plain"]) / out["plain"]))
  print("JN2018Diagnostics over all members at the same cadence: %.1f us per interval (%+.1f us), its "
        "pm_rows_pack launch %.1f us, %d bytes stored per sample (%.0f x the indices')"
        % (us("profiles"), us("profiles") - us("plain"), us("pack"), out["profile_bytes"],
           out["profile_bytes"] / out["index_bytes"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=None, help="default 64 (4096 with --time)")
  ap.add_argument("--years", type=int, default=200)
  ap.add_argument("--nz", type=int, default=None, help="default 81 (200 with --time)")
  ap.add_argument("--dt-days", type=float, default=None, help="default 30 (10 with --time)")
  ap.add_argument("--ramp-start", type=float, default=20.)
  ap.add_argument("--ramp-end", type=float, default=120.)
  ap.add_argument("--wind-year", type=float, default=60.)
  ap.add_argument("--print-years", type=int, default=10, help="years between printed rows")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  timing = args.time
  args.members = args.members or (4096 if timing else 64)
  args.nz = args.nz or (200 if timing else 81)
  args.dt_days = args.dt_days or (10. if timing else 30.)
  if timing:
    return time_it(args)
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  ens = pymoc_amd.JN2018Ensemble(
      cfg, forcing=schedule(cfg, (args.ramp_start, args.ramp_end), args.wind_year))
  rec = pymoc_amd.IndexRecorder(ens, SPECS, M, args.years)  # a sample at the top of every year
  ens.run(args.years * M)
  series = [("amoc [Sv]", rec.values["amoc"]), ("z(amoc) [m]", rec.depth("amoc")),
            ("z_zero [m]", rec.values["z_zero"]), ("abyss [Sv]", rec.values["abyss"]),
            ("b_1000 [m/s2]", rec.values["b_1000"]), ("b_upper [m/s2]", rec.values["b_upper"])]
  print("%d members, %d yearly samples of %d indices: %d bytes on the device"
        % (ens.n, args.years, len(SPECS), 12 * len(SPECS) * ens.n * args.years))
  print("warming ramps over years %g-%g, wind +25 %% at year %g; ensemble quantiles 10 / 50 / 90 %%"
        % (args.ramp_start, args.ramp_end, args.wind_year))
  years = sorted(set(range(0, args.years, max(args.print_years, 1))) | {args.years - 1})
  for label, a in series:
    print(label)
    for yr in years:
      col = a[:, yr]
      ok = np.isfinite(col)
      q = np.quantile(col[ok], [0.1, 0.5, 0.9]) if ok.any() else [np.nan] * 3
      print("  year %4d  %12.5g %12.5g %12.5g%s"
            % (yr, q[0], q[1], q[2], "" if ok.all() else "   (%d members without one)" % (~ok).sum()))
  bad = ens.nonfinite_members()
  if bad.size:
    print("%d members went non-finite" % bad.size)


if __name__ == "__main__":
  main()
