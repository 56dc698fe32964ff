#!/usr/bin/env python3
"""Lag-1 autocorrelation, variance, the DFA exponent and the restoring rate lambda of the AMOC in a
ramped, stochastically forced sweep, side by side, computed on the device.

The experiment of examples/amoc_early_warning_dfa.py: `--sets` parameter sets x `--realisations`
realisations warm under a pymoc_amd.ForcingSchedule ramp while pymoc_amd.NoiseForcing drives the
realisations apart -- with a red `bs_north` noise, the confound Boers 2021 warns of: `ac` and
`var` also rise when the forcing noise gets redder or stronger, with no loss of stability -- and
an IndexRecorder keeps every member's AMOC maximum below 500 m once a year in a device series.
pymoc_amd.SeriesWindows(..., dfa=True, restoring=True) reads that series where it lives: per
sliding window of `--window` years the three indicators of Lenton et al. 2012 and Boers' own, the
restoring rate lambda (pm_series_restoring): the slope of the regression of the index's yearly
increments on the detrended index, with the regression errors modelled as AR(1) noise and fitted
by ten iterations of generalised least squares.  lambda is per record interval (here: per year)
and rises towards 0 from below as the state loses stability.  Printed per set, side by side:
  across_members   the group means of `ac`, `var`, `dfa` and `lam` per window
  trend            the median Kendall tau of each indicator against time
  --significance   the fraction of members whose AR(1)-surrogate p_rising is at most `--level`,
                   for each of the four
The script then downloads the series and checks, against the NumPy restatement
(tests/restoring_cases.py), lam and rho bit for bit, and the group statistics and Kendall counts
exactly on the device's lambda series.  Whether this ramp shows a rising lambda is an outcome, not
a claim.

    python examples/amoc_early_warning_restoring.py --sets 4 --realisations 16 --years 300 --significance
    python examples/amoc_early_warning_restoring.py --time   # the restoring launch next to the
                                                 # window launch, trend() and significance() with
                                                 # and without restoring, at 4096 members x 8
                                                 # indices x 1200 records, W = 256, S = 8 and S = 1
                                                 # 
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # restoring_cases, windows_cases, stats_cases
sys.path.insert(2, os.path.join(ROOT, "examples"))  # amoc_early_warning: the experiment
import pymoc_amd
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.restoring import launch_restoring
from pymoc_amd.steady import YEAR
import amoc_early_warning as EW
import restoring_cases as RC
import stats_cases as STC
import windows_cases as WC

KEYS = ("ac", "var", "dfa", "lam")
ITERS = 10


def run(args):
  cfg, groups = EW.sweep(args.sets, args.realisations, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  noise = pymoc_amd.NoiseForcing(args.seed, tau=dict(sigma=args.sigma_tau),
                                 bs_north=dict(sigma=args.sigma_bs_north,
                                               tau_corr=args.tau_corr * YEAR))
  sched = EW.ramp(cfg, groups, args.sets, args.ramp_start, args.years)
  ens = pymoc_amd.JN2018Ensemble(cfg, forcing=sched, noise=noise)
  rec = pymoc_amd.IndexRecorder(ens, [("amoc", "max", "Psi", dict(zhi=-500.))], M, args.years)
  ens.run((args.years - 1) * M + 1)
  sw = pymoc_amd.SeriesWindows(rec, args.window, step=args.step, detrend="linear", groups=groups,
                               dfa=True, restoring=True)
  k0, k1 = args.spinup, args.years
  nwin, ends = sw.nwin(k0, k1), sw.record_end(k0, k1)
  across = {key: sw.across_members(key, k0, k1, quantiles=EW.QUANTILES) for key in KEYS}
  trend = sw.trend(k0, k1)
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR,
           args.seed))
  print("AMOC maximum below 500 m, years %d-%d: %d windows of %d years every %d years, linear "
        "trend removed, lag 1; DFA scales %s; restoring rate per year, %d iterations"
        % (k0, k1 - 1, nwin, args.window, args.step, " ".join(map(str, sw.dfa_scales)), ITERS))
  print("group means across the realisations of a set, dated at the end of the window:")
  print("  set  year  members                        ac                       var"
        "                       dfa                       lam")
  shown = np.unique(np.linspace(0, nwin - 1, min(EW.SHOWN, nwin)).astype(int))
  for g in range(args.sets):
    for i in shown:
      print("  %3d  %4d  %7d  %s" % (sw.group_labels[g], ends[i], across["lam"].count["amoc"][g, i],
                                     "  ".join("%24.17e" % across[key].mean["amoc"][g, i]
                                               for key in KEYS)))
  print("Kendall's tau of the indicator against time, median over the members of a set:")
  print("  set                        ac                       var                       dfa"
        "                       lam")
  for g in range(args.sets):
    print("  %3d  %s" % (sw.group_labels[g], "  ".join(
        "%24.17e" % EW.summary(getattr(trend, key).tau["amoc"], groups, sw.group_labels[g])[0]
        for key in KEYS)))
  if args.significance:
    sig = sw.significance(k0, k1, nsur=args.nsur, seed=args.seed + 1)
    print("AR(1)-surrogate test, %d surrogates: fraction of the members of a set with p_rising "
          "<= %g:" % (args.nsur, args.level))
    print("  set        ac       var       dfa       lam")
    for g in range(args.sets):
      fr = []
      for key in KEYS:
        p = getattr(sig, key).p_rising["amoc"][groups == sw.group_labels[g]]
        p = p[~np.isnan(p)]
        fr.append(float((p <= args.level).mean()) if p.size else float("nan"))
      print("  %3d  %8.4f  %8.4f  %8.4f  %8.4f" % ((sw.group_labels[g],) + tuple(fr)))
  # the host route, for the check: the whole series, the restatement of the definition
  r = sw.compute(k0, k1)
  series = np.ascontiguousarray(np.stack([rec.values[nm].T for nm in sw.names], axis=1))
  if args.save_series:
    np.savez(args.save_series, series=series, groups=groups, k0=k0, k1=k1, window=args.window,
             step=args.step, iters=ITERS)
  want = RC.restoring(series, k0, k1, args.window, args.step, "linear", ITERS)
  lam = r.lam["amoc"].T[:, None, :]      # [nwin, 1, n]
  rho = r.lam_rho["amoc"].T[:, None, :]
  ok_bits = EW.same_bits(lam, want["lam"]) and EW.same_bits(rho, want["rho"])
  order, start = STC.order_of(groups)
  wc, ws = STC.group_stats(lam, order, start, EW.QUANTILES, 0, nwin)
  ok = np.array_equal(across["lam"].count["amoc"], wc[:, 0, :].T)
  ok &= EW.same_bits(across["lam"].mean["amoc"], ws[:, 0, :, 0].T)
  conc, disc, tie, nfin = WC.kendall(lam, 0, nwin)
  tr = trend.lam
  ok &= all(np.array_equal(got["amoc"], w[0]) for got, w in
            ((tr.conc, conc), (tr.disc, disc), (tr.tie, tie), (tr.nfin, nfin)))
  ok &= EW.same_bits(tr.tau["amoc"], WC.tau_b(conc[0], disc[0], tie[0]))
  print("restatement on the downloaded series: lam and rho %s; group means and Kendall counts of "
        "the device's lambda series %s"
        % ("every bit agrees" if ok_bits else "MISMATCH", "exact" if ok else "MISMATCH"))
  return 0 if ok and ok_bits else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the restoring launch with and without rho
  stored, of the window launch on the same series in the same run and of trend() whole, for
  `--step` 8 and 1, on a synthetic AR(1) series of `--sets` x `--realisations` members, 8 indices
  and `--records` records; at step 8 the wall time of significance() with `--nsur` surrogates with
  and without restoring; and the device's lam against the restatement on `--host-members`
  members."""
  n, nspec, nrec, W = args.sets * args.realisations, 8, args.records, args.window
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(nrec):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  null = LaunchTimer().null_span_ms()
  hm = min(args.host_members, n)
  ok = True
  for S in (8, 1):
    sw = pymoc_amd.SeriesWindows((dev, names), W, step=S, restoring=True)
    plain = pymoc_amd.SeriesWindows((dev, names), W, step=S)
    nwin, ctx = sw.nwin(), sw._ctx()
    if S == 8:
      print("%d members, %d indices, %d records: a series of %.1f MB; window %d, %d iterations "
            "(empty span %.1f us subtracted)" % (n, nspec, nrec, v.nbytes / 1e6, W, ITERS,
                                                 1e3 * null))
    out = sw._launch(0, nrec, nwin)  # warm-up
    lam, rho = launch_restoring(dev, 0, nrec, sw._par, sw._restoring, ctx, rho=True)
    synchronize()
    t_win = EW._median_ms(lambda: sw._launch(0, nrec, nwin, out=out), args.reps) - null
    t_both = EW._median_ms(lambda: launch_restoring(dev, 0, nrec, sw._par, sw._restoring, ctx,
                                                    lam=lam, rho=rho), args.reps) - null
    t_lam = EW._median_ms(lambda: launch_restoring(dev, 0, nrec, sw._par, sw._restoring, ctx,
                                                   lam=lam), args.reps) - null
    sw.trend(), plain.trend()  # warm-up
    t_tr = EW._median_ms(lambda: sw.trend(), args.reps)
    t_trp = EW._median_ms(lambda: plain.trend(), args.reps)
    print("step %d: %d windows" % (S, nwin))
    print("  k_series_restoring, lam and rho: %9.1f us   lam only: %9.1f us   (2 W = %d LDS reads, "
          "13 products a record, %d divisions a window)"
          % (1e3 * t_both, 1e3 * t_lam, 2 * W, 5 * ITERS))
    print("  k_series_windows:                %9.1f us   (3 W = %d LDS reads and 4 divisions a "
          "window): the restoring launch costs %.1f of it" % (1e3 * t_win, 3 * W, t_lam / t_win))
    print("  trend() whole:                   %9.1f ms with restoring, %9.1f ms without"
          % (t_tr, t_trp))
    res = lam.download()
    want = RC.restoring(v[:, :1, :hm], 0, nrec, W, S, "linear", ITERS)["lam"]
    same = EW.same_bits(res[:, :1, :hm], want)
    ok &= bool(same)
    print("  lam of %d members of index 0 against the restatement: %s"
          % (hm, "every bit agrees" if same else "MISMATCH"))
    if S == 8:
      for obj, what in ((plain, "without restoring"), (sw, "with restoring")):
        obj.significance(nsur=12)  # warm-up: two chunks
        synchronize()
        t0 = time.perf_counter()
        obj.significance(nsur=args.nsur)
        print("  significance(), %d surrogates, %s: %.2f s wall"
              % (args.nsur, what, time.perf_counter() - t0))
  print("restatement and device agree: %s" % ok)
  return 0 if ok else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--years", type=int, default=300)
  ap.add_argument("--window", type=int, default=None, help="years; default 64 (256 with --time)")
  ap.add_argument("--step", type=int, default=4, help="years between windows")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the indicators")
  ap.add_argument("--ramp-start", type=float, default=10.)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--significance", action="store_true", help="the surrogate test of the trends")
  ap.add_argument("--nsur", type=int, default=None, help="default 199 (1000 with --time)")
  ap.add_argument("--level", type=float, default=0.1)
  ap.add_argument("--save-series", default=None,
                  help="write the downloaded series and the settings to this .npz")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--host-members", type=int, default=8, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  args.window = args.window or (256 if args.time else 64)
  args.nsur = args.nsur or (1000 if args.time else 199)
  if args.time:
    return time_it(args)
  if args.window < 20:
    ap.error("--window must be at least 20 for the DFA scales")
  if args.years - args.spinup < args.window:
    ap.error("--years less --spinup must be at least --window")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
