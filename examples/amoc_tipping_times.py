#!/usr/bin/env python3
"""When does each member's AMOC collapse, and do the early-warning trends warn BEFORE it? -- a
ramped, stochastically forced Jansen & Nadeau (2018) sweep, analysed on the device.

The experiment is the one of examples/amoc_early_warning.py: `--sets` parameter sets x
`--realisations` realisations warm under a ForcingSchedule ramp while NoiseForcing drives the
realisations of a set apart, and an IndexRecorder keeps every member's AMOC maximum below 500 m
once a year.  Every member tips in a year of its own, and some never do, so one record window for
the whole ensemble either throws most records away or lets the collapse itself into the late
windows, where it reads as rising variance and autocorrelation.  pymoc_amd.SeriesShifts finds, per
member, the year of the largest drop between two adjacent windows of `--half` years (`at`) and
the first year from which a drop of `--threshold` pooled standard deviations is detectable
(`first`); SeriesWindows.significance(until=) then runs the surrogate test of the trends on every
member's records before its own `first` (less `--guard` years).  Only results are downloaded.
Printed per set: the fraction of members with a detected drop, the median and the 5-95 % range of
their tipping year, and -- with and without `until=`, side by side -- the median tau and the
fraction of members with p_rising <= 0.05, for `ac` and for `var`.  The script then downloads the
series and checks every printed number against the NumPy restatement (tests/shifts_cases.py,
tests/surrogate_cases.py) run on the device's own surrogate series.  Whether this ramp tips a
member is an outcome, not a claim.

    python examples/amoc_tipping_times.py --sets 2 --realisations 8 --years 120 --half 20
    python examples/amoc_tipping_times.py --time   # the scan, the window launch that feeds it, the
                                                   # censor, the ranged fit and significance() with
                                                   # and without until= at 4096 members x 8 indices
                                                   # x 1200 records, L = 50
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # shifts_cases, surrogate_cases: the restatements
import pymoc_amd
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.series import Ctx, _Plane
from pymoc_amd.shifts import launch_fit_ranged, stt_table
from pymoc_amd.steady import YEAR
from pymoc_amd.surrogates import SeriesSurrogates
from pymoc_amd.windows import launch_windows, win_par
from amoc_early_warning import _median_ms, ramp, same_bits, sweep  # the same experiment
import shifts_cases as SHC
import surrogate_cases as SGC

LEVEL = 0.05
COPY_RATE = 6.29e12  # bytes / s a plain device copy reaches


def tipping(record, first, groups, label):
  """(fraction of the set's members with a detected drop, median, 5 % and 95 % of their tipping
  year); NaN where no member of the set has one."""
  sel = groups == label
  hit = first[sel] >= 0
  years = record[sel][hit].astype(np.float64)
  if not years.size:
    return float(hit.mean()), float("nan"), float("nan"), float("nan")
  return (float(hit.mean()), float(np.median(years)), float(np.quantile(years, 0.05)),
          float(np.quantile(years, 0.95)))


def warning(tau, p, groups, label):
  """(median tau, fraction with p_rising <= LEVEL) over the set's members that have one."""
  t, q = tau[groups == label], p[groups == label]
  t, q = t[~np.isnan(t)], q[~np.isnan(q)]
  return (float(np.median(t)) if t.size else float("nan"),
          float((q <= LEVEL).mean()) if q.size else float("nan"))


def run(args):
  cfg, groups = sweep(args.sets, args.realisations, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  noise = pymoc_amd.NoiseForcing(args.seed, tau=dict(sigma=args.sigma_tau),
                                 bs_north=dict(sigma=args.sigma_bs_north,
                                               tau_corr=args.tau_corr * YEAR))
  sched = ramp(cfg, groups, args.sets, args.ramp_start, args.years if args.ramp_end is None
               else args.ramp_end)
  ens = pymoc_amd.JN2018Ensemble(cfg, forcing=sched, noise=noise)
  rec = pymoc_amd.IndexRecorder(ens, [("amoc", "max", "Psi", dict(zhi=-500.))], M, args.years)
  ens.run((args.years - 1) * M + 1)
  k0, k1 = args.spinup, args.years
  K = k1 - k0
  sh = pymoc_amd.SeriesShifts(rec, args.half, direction=-1, threshold=args.threshold)
  found = sh.detect(k0, k1)
  sh.censored(where="first", guard=args.guard)
  sw = pymoc_amd.SeriesWindows(rec, args.window, step=args.step, detrend="linear", lag=1)
  kw = dict(nsur=args.nsur, seed=args.surrogate_seed)
  plain = sw.significance(k0, k1, **kw)
  until = sw.significance(k0, k1, until=sh, **kw)
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR, args.seed))
  print("AMOC maximum below 500 m, years %d-%d: drops between two windows of %d years, detectable "
        "from %g pooled standard deviations; the trends of %d-year windows every %d years, linear "
        "trend removed, lag 1; %d AR(1) surrogates per member, seed %d"
        % (k0, k1 - 1, args.half, args.threshold, args.window, args.step, args.nsur,
           args.surrogate_seed))
  print("tipping year of the members of a set (the year of the largest drop, where one is "
        "detectable):")
  print("  set  members  detected    median        5%       95%")
  for g in range(args.sets):
    frac, med, lo, hi = tipping(found.record["amoc"], found.first["amoc"], groups, g)
    print("  %3d  %7d  %8.3f  %8.1f  %8.1f  %8.1f" % (g, int((groups == g).sum()), frac, med, lo, hi))
  print("Kendall's tau and the fraction of members with p_rising <= %g, up to every member's own "
        "end (until) and over all years (plain):" % LEVEL)
  print("  set  what  median tau until  median tau plain  fraction until  fraction plain")
  for g in range(args.sets):
    for key in ("ac", "var"):
      u, p = getattr(until, key), getattr(plain, key)
      wu = warning(u.tau["amoc"], u.p_rising["amoc"], groups, g)
      wp = warning(p.tau["amoc"], p.p_rising["amoc"], groups, g)
      print("  %3d  %4s  %16.3f  %16.3f  %14.3f  %14.3f" % (g, key, wu[0], wp[0], wu[1], wp[1]))
  # the host route, for the check: the whole series, the restatement of the definitions, the
  # surrogate series the device generated from its two fits
  series = np.ascontiguousarray(np.stack([rec.values[nm].T for nm in sw.names], axis=1))
  want = SHC.detect(series, k0, k1, args.half, [args.threshold], [-1])
  ok = all(np.array_equal(getattr(found, key)["amoc"], want[key][0])
           for key in ("at", "first", "ncand"))
  ok &= np.array_equal(found.record["amoc"], np.where(want["at"][0] < 0, -1, k0 + want["at"][0]))
  ok &= all(same_bits(getattr(found, key)["amoc"], want["val"][i, 0])
            for i, key in enumerate(("stat", "jump", "before", "after")))
  end = SHC.ends(want["first"], K, args.guard)
  ok &= np.array_equal(sh.end()["amoc"], end[0])
  gen = SeriesSurrogates(rec, seed=args.surrogate_seed)
  sur = gen.generate(k0, k1, 0, args.nsur)[0].download(stream=ens.stream)
  checks = [(plain, SGC.significance(series, k0, k1, args.window, args.step, 1, "linear",
                                     args.nsur, sur=sur))]
  cens, names = sh.censored(where="first", guard=args.guard)
  fit = launch_fit_ranged(cens, (K, 1, series.shape[2]), 0, K, "linear", sh.end, ens.stream, None)
  y = DeviceArray((K, args.nsur, series.shape[2]), np.float64)
  gen._launch(fit, K, 0, args.nsur, y)
  sur = y.download(stream=ens.stream)
  checks.append((until, SHC.significance(series, k0, k1, args.window, args.step, 1, "linear",
                                         args.nsur, end, sur=sur)))
  for got, w in checks:
    for key in ("var", "ac"):
      r = getattr(got, key)
      ok &= all(np.array_equal(getattr(r, f)["amoc"], w[key][f][0]) for f in ("ge", "le", "nvalid"))
      ok &= all(same_bits(getattr(r, f)["amoc"], w[key][f][0]) for f in ("tau", "p_rising"))
      ok &= all(same_bits(warning(r.tau["amoc"], r.p_rising["amoc"], groups, g),
                          warning(w[key]["tau"][0], w[key]["p_rising"][0], groups, g))
                for g in range(args.sets))
  ok &= all(same_bits(tipping(found.record["amoc"], found.first["amoc"], groups, g),
                      tipping(np.where(want["at"][0] < 0, -1, k0 + want["at"][0]), want["first"][0],
                              groups, g)) for g in range(args.sets))
  print("restatement on the downloaded series: %s" % ("every number agrees" if ok else "MISMATCH"))
  return 0 if ok else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the window launch that feeds the scan, the
  scan, the censor (into a copy, and in place on a chunk of surrogates) and the ranged fit, and
  the wall time of significance() with and without `until=`, on a synthetic AR(1) series of
  `--sets` x `--realisations` members, 8 indices and `--records` records in which every second
  member drops by 6 standard deviations in a year of its own."""
  n, nspec, K, L = args.sets * args.realisations, 8, args.records, args.half
  rng = np.random.default_rng(args.seed)
  v = np.empty((K, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(K):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  at = rng.integers(K // 2, K - L, size=n)
  drops = (np.arange(K)[:, None] >= at[None, :]) & (np.arange(n)[None, :] % 2 == 0)
  v -= 6.0 * drops[:, None, :]
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  null = LaunchTimer().null_span_ms()
  sh = pymoc_amd.SeriesShifts((dev, names), L, direction=-1, threshold=args.threshold)
  found = sh.detect()
  hit = np.stack([found.first[nm] >= 0 for nm in names])
  nwin = K - L + 1
  shape = (nwin, nspec, n)
  print("%d members, %d indices, %d records: a series of %.1f MB; L = %d: %d candidates per series, "
        "a window scratch of %.1f MB; a drop detected in %.3f of the series; empty span %.1f us "
        "subtracted" % (n, nspec, K, v.nbytes / 1e6, L, K - 2 * L + 1, 32 * nwin * nspec * n / 1e6,
                        hit.mean(), 1e3 * null))
  feed, ctx = win_par(L, 1, 1, "constant"), Ctx(None, None)
  out = launch_windows(dev, 0, K, feed, ctx)
  scan_out = sh._scan(0, K, _Plane(out[0], 0, shape), _Plane(out[0], 2, shape))
  y, _ = sh.censored()
  fit = launch_fit_ranged(y, (K, nspec, n), 0, K, "linear", sh.end, None, None)
  synchronize()
  plane = 8 * nwin * nspec * n
  t_win = _median_ms(lambda: launch_windows(dev, 0, K, feed, ctx, out=out), args.reps) - null
  t_scan = _median_ms(lambda: sh._scan(0, K, _Plane(out[0], 0, shape), _Plane(out[0], 2, shape),
                                       out=scan_out), args.reps) - null
  t_cens = _median_ms(lambda: sh._censor(dev.ptr, K, 1, y.ptr, None, None), args.reps) - null
  t_inpl = _median_ms(lambda: sh._censor(y.ptr, K, 1, y.ptr, None, None), args.reps) - null
  table = stt_table(K)
  t_fit = _median_ms(lambda: launch_fit_ranged(y, (K, nspec, n), 0, K, "linear", sh.end, None, None,
                                               table=table, out=fit), args.reps) - null
  kept = 8 * int(sh.end.download().astype(np.int64).sum())
  for what, ms, must in (
      ("k_series_windows (W = L, S = 1)", t_win, v.nbytes + 4 * plane),
      ("k_series_shift_scan", t_scan, 2 * plane),
      ("k_series_censor (a copy)", t_cens, kept + v.nbytes),
      ("k_series_censor (in place)", t_inpl, v.nbytes - kept),
      ("k_series_fit_ranged (linear)", t_fit, 2 * kept)):
    print("  %-38s %9.1f us  must move %7.1f MB: %6.1f us at %.2f TB/s"
          % (what + ":", 1e3 * ms, must / 1e6, 1e6 * must / COPY_RATE, COPY_RATE / 1e12))
  sw = pymoc_amd.SeriesWindows((dev, names), args.window, step=args.step)
  kw = dict(nsur=args.nsur, seed=args.surrogate_seed)
  sw.significance(nsur=1)  # warm-up
  synchronize()
  res = {}
  for what, extra in (("plain", {}), ("until", dict(until=sh))):
    t0 = time.perf_counter()
    res[what] = sw.significance(**dict(kw, **extra))
    print("  significance(nsur = %d), %-6s %10.1f ms wall (window %d, step %d)"
          % (args.nsur, what + ":", 1e3 * (time.perf_counter() - t0), args.window, args.step))
  for what in ("plain", "until"):
    p = np.stack([res[what].var.p_rising[nm] for nm in names])
    print("  %s: fraction with var p_rising <= %g among the series that drop %.3f, among the others "
          "%.3f" % (what, LEVEL, np.nanmean(p[hit] <= LEVEL), np.nanmean(p[~hit] <= LEVEL)))
  # (a drop of 6 sd against window means that scatter by 0.9 sd: a few in ten thousand fall short)
  planted = float(hit[:, 0::2].mean())
  ok = planted >= 0.99
  print("a drop is detected in %.4f of the series with one and in %.4f of those without"
        % (planted, float(hit[:, 1::2].mean())))
  return 0 if ok else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 2 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 8 (64 with --time)")
  ap.add_argument("--years", type=int, default=120)
  ap.add_argument("--half", type=int, default=None,
                  help="years of each of the two windows compared; default 20 (50 with --time)")
  ap.add_argument("--threshold", type=float, default=3.0, help="pooled standard deviations")
  ap.add_argument("--guard", type=int, default=0, help="years kept clear before `first`")
  ap.add_argument("--window", type=int, default=None, help="years; default 32 (256 with --time)")
  ap.add_argument("--step", type=int, default=None, help="years between windows; default 4 (8 with --time)")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the analysis")
  ap.add_argument("--nsur", type=int, default=None, help="surrogates; default 200 (100 with --time)")
  ap.add_argument("--surrogate-seed", type=int, default=1955)
  ap.add_argument("--ramp-start", type=float, default=10.)
  ap.add_argument("--ramp-end", type=float, default=None, help="default: the last year")
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 2)
  args.realisations = args.realisations or (64 if args.time else 8)
  args.half = args.half or (50 if args.time else 20)
  args.window = args.window or (256 if args.time else 32)
  args.step = args.step or (8 if args.time else 4)
  args.nsur = args.nsur or (100 if args.time else 200)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < max(args.window, 2 * args.half):
    ap.error("--years less --spinup must be at least --window and twice --half")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
