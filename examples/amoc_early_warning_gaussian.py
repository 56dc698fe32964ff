#!/usr/bin/env python3
"""Early-warning trends of the AMOC under the two detrendings, side by side -- computed on the
device.

The ramped, stochastically forced Jansen & Nadeau (2018) sweep of examples/amoc_early_warning.py:
`--sets` parameter sets x `--realisations` realisations warm under a pymoc_amd.ForcingSchedule ramp
while pymoc_amd.NoiseForcing drives the realisations apart, and an IndexRecorder keeps every
member's AMOC maximum below 500 m once a year in a device series.  pymoc_amd.SeriesWindows then
reads that series where it lives, twice:
  detrend="linear"     the least-squares line of every window is removed inside the window
  detrend="gaussian"   a Gaussian-kernel trend of `--sigma` years is removed from the whole record
                       first (pymoc_amd.SeriesSmooth's kernel, pm_series_smooth), then each
                       window's mean: the estimator of Dakos et al. 2008, Lenton et al. 2012 and
                       Boers 2021
and for each the script prints, per set, the median Kendall tau of `ac` and of `var` and the
fraction of members whose AR(1)-surrogate p_rising is at most `--level`.  Under "gaussian" every
surrogate goes through the same smoother as the record.  Under a ramp the index curves; what a
per-window line leaves of that curvature raises both indicators towards the end of the record, so
the two columns may differ -- by how much is an outcome, not a claim.  The script then downloads
the series and checks the "gaussian" indicators and counts, bit for bit, against the NumPy
restatement (tests/smooth_cases.py).

    python examples/amoc_early_warning_gaussian.py --sets 4 --realisations 16 --years 300
    python examples/amoc_early_warning_gaussian.py --time   # the smoother launch, compute(),
                                                            # significance() and the host route at
                                                            # 4096 members x 8 indices x 1200
                                                            # records, W = 256, S = 8, sigma = 50
                                                            # 
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # smooth_cases: the restatement
sys.path.insert(2, os.path.join(ROOT, "examples"))  # amoc_early_warning: the experiment
import pymoc_amd
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.series import Ctx
from pymoc_amd.steady import YEAR
from pymoc_amd.windows import launch_windows
import amoc_early_warning as EW
import smooth_cases as SC

COPY_RATE = EW.COPY_RATE  # bytes / s a plain device copy reaches


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
  k0, k1 = args.spinup, args.years
  kw = dict(step=args.step, lag=1, groups=groups)
  sws = dict(linear=pymoc_amd.SeriesWindows(rec, args.window, detrend="linear", **kw),
             gaussian=pymoc_amd.SeriesWindows(rec, args.window, detrend="gaussian",
                                              sigma=args.sigma, truncate=args.truncate, **kw))
  sig = {det: sw.significance(k0, k1, nsur=args.nsur, seed=args.surrogate_seed)
         for det, sw in sws.items()}
  trend = sws["gaussian"].trend(k0, k1)
  win = sws["gaussian"].compute(k0, k1)
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR, args.seed))
  print("AMOC maximum below 500 m, years %d-%d: %d windows of %d years every %d years, lag 1; %d "
        "AR(1) surrogates per member, seed %d; gaussian: sigma %g years, cut at %g sigma (H = %d)"
        % (k0, k1 - 1, sws["linear"].nwin(k0, k1), args.window, args.step, args.nsur,
           args.surrogate_seed, args.sigma, args.truncate, SC.half_of(args.sigma, args.truncate)))
  print("per set: the median tau over its members and the fraction with p_rising <= %g:" % args.level)
  print("  set  what  members        tau linear  p<=level linear      tau gaussian  p<=level gaussian")
  ok = True
  for g in np.unique(groups):
    sel = groups == g
    for key in ("ac", "var"):
      row = []
      for det in ("linear", "gaussian"):
        r = getattr(sig[det], key)
        tau, p = r.tau["amoc"][sel], r.p_rising["amoc"][sel]
        row += [float(np.median(tau)), float((p <= args.level).mean())]
        ok &= bool(np.isfinite(row).all()) and bool((r.nvalid["amoc"][sel] == args.nsur).all())
      print("  %3d  %4s  %7d  %16.9f  %15.4f  %16.9f  %17.4f" % (g, key, int(sel.sum()), *row))
  print("every member has a tau and %d surrogates with one under both detrendings: %s"
        % (args.nsur, ok))
  # the host route, for the check: the whole series, the restatement of the definitions
  series = np.ascontiguousarray(np.stack([rec.values[nm].T for nm in sws["linear"].names], axis=1))
  want = SC.windows(series, k0, k1, args.window, args.step, 1, args.sigma, args.truncate)
  wt = SC.trend(series, k0, k1, args.window, args.step, 1, args.sigma, args.truncate)
  same = True
  for i, key in enumerate(("mean", "slope", "var", "ac")):
    same &= EW.same_bits(getattr(win, key)["amoc"], want["out"][i, :, 0, :].T)
  for key in ("var", "ac"):
    tr = getattr(trend, key)
    same &= all(np.array_equal(got["amoc"], w[0]) for got, w in
                zip((tr.conc, tr.disc, tr.tie, tr.nfin), wt[key]))
    same &= EW.same_bits(getattr(sig["gaussian"], key).tau["amoc"], tr.tau["amoc"])
  print("restatement of the gaussian pipeline on the downloaded series: %s"
        % ("every bit agrees" if same else "MISMATCH"))
  return 0 if ok and same else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the smoother launch alone, with the bytes it
  must move and its rate against a plain copy; of compute() and wall time of significance() under
  both detrendings; next to them the host route: the download of the series and the smoothing on
  one core (the restatement and scipy.ndimage.gaussian_filter1d on `--host-members` members,
  scaled to all).  A synthetic AR(1) series of `--sets` x `--realisations` members, 8 indices and
  `--records` records."""
  from scipy.ndimage import gaussian_filter1d
  n, nspec, nrec, W, S = args.sets * args.realisations, 8, args.records, args.window, args.step
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(nrec):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  null = LaunchTimer().null_span_ms()
  t0 = time.perf_counter()
  host = dev.download()
  t_down = time.perf_counter() - t0
  H = SC.half_of(args.sigma, args.truncate)
  print("%d members, %d indices, %d records: a series of %.1f MB; window %d, step %d, sigma %g "
        "(H = %d) (empty span %.1f us subtracted); download of the series %.1f ms"
        % (n, nspec, nrec, v.nbytes / 1e6, W, S, args.sigma, H, 1e3 * null, 1e3 * t_down))
  sm = pymoc_amd.SeriesSmooth((dev, names), args.sigma, truncate=args.truncate)
  resid, trend = sm._alloc(nrec), sm._alloc(nrec)
  nbad = sm._launch(0, nrec, resid=resid)  # warm-up
  synchronize()
  t_res = EW._median_ms(lambda: sm._launch(0, nrec, resid=resid, nbad=nbad), args.reps) - null
  t_both = EW._median_ms(lambda: sm._launch(0, nrec, trend=trend, resid=resid, nbad=nbad),
                         args.reps) - null
  must = 2 * v.nbytes + 4 * nspec * n
  taps = float(sum(min(nrec - 1, j + H) - max(0, j - H) + 1 for j in range(nrec))) * nspec * n
  print("  k_series_smooth (resid):         %9.1f us  must read %.1f MB and write %.1f MB: %.1f us "
        "at %.2f TB/s, %.1f %% of the copy rate reached; %.3g taps, %.2f ps per tap"
        % (1e3 * t_res, v.nbytes / 1e6, (v.nbytes + 4 * nspec * n) / 1e6, 1e6 * must / COPY_RATE,
           COPY_RATE / 1e12, 100. * must / COPY_RATE / (1e-3 * t_res), taps, 1e9 * t_res / taps))
  print("  k_series_smooth (trend + resid): %9.1f us" % (1e3 * t_both))
  times = {}
  for det, kw in (("linear", {}), ("gaussian", dict(sigma=args.sigma, truncate=args.truncate))):
    sw = pymoc_amd.SeriesWindows((dev, names), W, step=S, detrend=det, **kw)
    nwin = sw.nwin()
    sw.compute()  # warm-up
    out = sw._alloc(nwin)
    # the launches compute() issues, into preallocated arrays: no allocation inside the span
    # (compute() itself allocates its residual and its outputs per call: that is in its wall time)
    def launches():
      if det == "gaussian":
        sm._launch(0, nrec, resid=resid, nbad=nbad)
        launch_windows(resid, 0, nrec, sw._par, Ctx(None, None), out=out)
      else:
        sw._launch(0, nrec, nwin, out=out)
    launches()
    synchronize()
    t_launch = EW._median_ms(launches, args.reps) - null
    t0 = time.perf_counter()
    sw.compute()
    t_compute = time.perf_counter() - t0
    sw.significance(nsur=min(args.nsur, 12), seed=args.surrogate_seed)  # warm-up
    synchronize()
    t0 = time.perf_counter()
    sig = sw.significance(nsur=args.nsur, seed=args.surrogate_seed)
    t_sig = time.perf_counter() - t0
    times[det] = t_sig
    ok = all((getattr(sig, key).nvalid[nm] == args.nsur).all() for key in ("var", "ac") for nm in names)
    print("  %-8s the launches of compute() %9.1f us (%d windows); compute() with its download "
          "%.1f ms wall; significance(nsur = %d) %.1f ms wall; every surrogate counted: %s"
          % (det, 1e3 * t_launch, nwin, 1e3 * t_compute, args.nsur, 1e3 * t_sig, ok))
  print("  significance under gaussian costs %.2f times the linear one" % (times["gaussian"] / times["linear"]))
  # the host route on one core, on the first members
  hm = min(args.host_members, n)
  t0 = time.perf_counter()
  want = SC.smooth(host[:, :, :hm], 0, nrec, sm.weights)
  t_host = (time.perf_counter() - t0) * n / hm
  t0 = time.perf_counter()
  gaussian_filter1d(host[:, :, :hm], args.sigma, axis=0, truncate=args.truncate)
  t_scipy = (time.perf_counter() - t0) * n / hm
  same = EW.same_bits(resid.download()[:, :, :hm], want["resid"]) and \
      EW.same_bits(trend.download()[:, :, :hm], want["trend"])
  print("  host, one core (%d members, scaled to %d): the restatement %.1f s, "
        "scipy.ndimage.gaussian_filter1d %.2f s, next to the download and the upload of the "
        "residual" % (hm, n, t_host, t_scipy))
  print("host and device agree bit for bit: %s" % same)
  return 0 if same else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--years", type=int, default=300)
  ap.add_argument("--window", type=int, default=None, help="years; default 64 (256 with --time)")
  ap.add_argument("--step", type=int, default=None, help="years between windows; default 4 (8 with --time)")
  ap.add_argument("--sigma", type=float, default=None,
                  help="of the Gaussian kernel, years; default 25 (50 with --time)")
  ap.add_argument("--truncate", type=float, default=4.0)
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the indicators")
  ap.add_argument("--ramp-start", type=float, default=10.)
  ap.add_argument("--nsur", type=int, default=None, help="surrogates; default 200 (1000 with --time)")
  ap.add_argument("--surrogate-seed", type=int, default=1955)
  ap.add_argument("--level", type=float, default=0.1)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--host-members", type=int, default=16, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  args.window = args.window or (256 if args.time else 64)
  args.step = args.step or (8 if args.time else 4)
  args.sigma = args.sigma or (50. if args.time else 25.)
  args.nsur = args.nsur or (1000 if args.time else 200)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < args.window:
    ap.error("--years less --spinup must be at least --window")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
