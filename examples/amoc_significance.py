#!/usr/bin/env python3
"""Surrogate significance of the early-warning trends of the AMOC in a ramped, stochastically
forced Jansen & Nadeau (2018) sweep -- computed on the device.

The experiment is the one of examples/amoc_early_warning.py at a small default size: `--sets`
parameter sets x `--realisations` realisations warm under a ForcingSchedule ramp while NoiseForcing
drives the realisations of a set apart, and an IndexRecorder keeps every member's AMOC maximum
below 500 m once a year.  Kendall's tau of the sliding-window variance and lag-1 autocorrelation
means nothing by itself -- overlapping windows make any red noise trend -- so
pymoc_amd.SeriesWindows.significance fits a stationary AR(1) model to every member's detrended
series, generates `--nsur` surrogate series of it ON THE DEVICE, runs the identical window +
Kendall pipeline on each and counts the surrogates whose tau reaches the observed one:
p_rising = (1 + ge) / (1 + nvalid).  Only the counts are downloaded.  Printed per set: the fraction
of members with p_rising <= `--level` for `ac` and for `var`.  Under the null model that fraction
is `--level` on average; whether this ramp shows more is an outcome, not a claim.

    python examples/amoc_significance.py --sets 2 --realisations 8 --years 120 --window 32
    python examples/amoc_significance.py --time   # the generator, window, Kendall and counting
                                                  # launches and the whole significance() at 4096
                                                  # members x 8 indices x 1200 records, W = 256,
                                                  # S = 8, next to the host route (DESIGN.md
                                                  # section 23)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # windows_cases: the restatement, for the host route
import pymoc_amd
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.series import Ctx, _Plane
from pymoc_amd.steady import YEAR
from pymoc_amd.surrogates import SeriesSurrogates, chunk_size, launch_exceed
from pymoc_amd.windows import launch_kendall, launch_windows
from amoc_early_warning import _median_ms, ramp, sweep  # the same experiment
import windows_cases as WC


def fraction(p, groups, label, level):
  """The fraction of the set's members with p <= level; members without a p are left out."""
  q = p[groups == label]
  q = q[~np.isnan(q)]
  return float((q <= level).mean()) if q.size else float("nan")


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
  sw = pymoc_amd.SeriesWindows(rec, args.window, step=args.step, detrend="linear", lag=1)
  k0, k1 = args.spinup, args.years
  sig = sw.significance(k0, k1, nsur=args.nsur, seed=args.surrogate_seed)
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR, args.seed))
  print("AMOC maximum below 500 m, years %d-%d: %d windows of %d years every %d years, linear "
        "trend removed, lag 1; %d AR(1) surrogates per member, seed %d"
        % (k0, k1 - 1, sw.nwin(k0, k1), args.window, args.step, args.nsur, args.surrogate_seed))
  print("fraction of the members of a set with p_rising <= %g:" % args.level)
  print("  set  what  members  median tau  fraction")
  ok = True
  for g in range(args.sets):
    for key in ("ac", "var"):
      r = getattr(sig, key)
      frac = fraction(r.p_rising["amoc"], groups, g, args.level)
      tau = r.tau["amoc"][groups == g]
      ok &= bool(np.isfinite(frac)) and bool((r.nvalid["amoc"][groups == g] == args.nsur).all())
      print("  %3d  %4s  %7d  %10.3f  %8.3f"
            % (g, key, int((groups == g).sum()), float(np.nanmedian(tau)), frac))
  print("every member has a tau and %d surrogates with one: %s" % (args.nsur, ok))
  return 0 if ok else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the four launches of one chunk -- the
  generator, the windows, one Kendall, one exceed -- and the wall time of the whole
  significance(), on a synthetic AR(1) series of `--sets` x `--realisations` members, 8 indices and
  `--records` records; next to them the same pipeline on the host on one core for ONE surrogate of
  `--host-members` members (NumPy's generator, the restatement, scipy.stats.kendalltau), scaled
  to all members and `--nsur` surrogates."""
  import scipy.stats
  n, nspec, K, W, S = args.sets * args.realisations, 8, args.records, args.window, args.step
  rng = np.random.default_rng(args.seed)
  v = np.empty((K, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(K):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  null = LaunchTimer().null_span_ms()
  sw = pymoc_amd.SeriesWindows((dev, names), W, step=S)
  nwin = sw.nwin()
  nb = chunk_size(args.nsur, args.max_bytes, K, nspec, n)
  planes = nb * nspec
  print("%d members, %d indices, %d records: a series of %.1f MB; window %d, step %d: %d windows; "
        "chunks of %d surrogates (%.1f MB); empty span %.1f us subtracted"
        % (n, nspec, K, v.nbytes / 1e6, W, S, nwin, nb, nb * v.nbytes / 1e6, 1e3 * null))
  gen = SeriesSurrogates((dev, names), seed=args.surrogate_seed)
  fit = gen.fit()
  y = DeviceArray((K, planes, n), np.float64)
  ctx = Ctx(None, None)
  gen._launch(fit, K, 0, nb, y)  # warm-up
  wout = launch_windows(y, 0, K, sw._par, ctx)
  wshape = (nwin, planes, n)
  cnt = launch_kendall(_Plane(wout[0], 3, wshape), wshape, 0, nwin, None, None)
  obs = launch_kendall(_Plane(sw._launch(0, K, nwin)[0], 3, (nwin, nspec, n)), (nwin, nspec, n), 0,
                       nwin, None, None)
  acc = [DeviceArray.zeros((nspec, n), np.int32) for _ in range(3)]
  synchronize()
  t = dict(
      gen=_median_ms(lambda: gen._launch(fit, K, 0, nb, y), args.reps) - null,
      win=_median_ms(lambda: launch_windows(y, 0, K, sw._par, ctx, out=wout), args.reps) - null,
      kd=_median_ms(lambda: launch_kendall(_Plane(wout[0], 3, wshape), wshape, 0, nwin, None, None,
                                           out=cnt), args.reps) - null,
      ex=_median_ms(lambda: launch_exceed(obs, cnt, (nb, nspec, n), acc, None, None), args.reps) - null)
  chunk_ms = t["gen"] + t["win"] + 2 * (t["kd"] + t["ex"])
  for key, what in (("gen", "k_series_surrogates"), ("win", "k_series_windows"),
                    ("kd", "k_series_kendall (one of two)"), ("ex", "k_series_exceed (one of two)")):
    print("  %-32s %10.1f us per chunk of %d surrogates" % (what + ":", 1e3 * t[key], nb))
  print("  one chunk, the six launches:     %10.1f us; the generator writes %.1f MB and the window "
        "launch reads them again" % (1e3 * chunk_ms, nb * v.nbytes / 1e6))
  del y, wout, cnt
  synchronize()
  t0 = time.perf_counter()
  sig = sw.significance(nsur=args.nsur, seed=args.surrogate_seed, max_bytes=args.max_bytes)
  t_sig = time.perf_counter() - t0
  nchunks = -(-args.nsur // nb)
  print("  significance(nsur = %d):         %10.1f ms wall, %d chunks (%.1f ms of launches by the "
        "medians above)" % (args.nsur, 1e3 * t_sig, nchunks, nchunks * chunk_ms))
  # the host route on one core: ONE surrogate of the first members, scaled
  hm = min(args.host_members, n)
  host = v[:, :, :hm]
  t0 = time.perf_counter()
  f = WC.windows(host, 0, K, K, 1, 1, "linear")["out"]
  sd, phi = np.sqrt(f[2, 0]), f[3, 0]
  e = np.random.default_rng(1).standard_normal((K, nspec, hm))
  ys = np.empty_like(e)
  ys[0] = sd * e[0]
  for j in range(1, K):
    ys[j] = phi * ys[j - 1] + sd * np.sqrt(1 - phi * phi) * e[j]
  t_gen = time.perf_counter() - t0
  t0 = time.perf_counter()
  w = WC.windows(ys, 0, K, W, S, 1, "linear")["out"]
  t_win = time.perf_counter() - t0
  t0 = time.perf_counter()
  for s in range(nspec):
    for m in range(hm):
      scipy.stats.kendalltau(np.arange(nwin), w[2][:, s, m])
      scipy.stats.kendalltau(np.arange(nwin), w[3][:, s, m])
  t_kd = time.perf_counter() - t0
  scale = n / hm * args.nsur
  print("  host, one core (one surrogate of %d members, scaled to %d members x %d surrogates): "
        "generation %.0f s, the indicators %.0f s, kendalltau %.0f s"
        % (hm, n, args.nsur, t_gen * scale, t_win * scale, t_kd * scale))
  ok = all((getattr(sig, key).nvalid[nm] == args.nsur).all() for key in ("var", "ac") for nm in names)
  frac = np.mean([(sig.ac.p_rising[nm] <= 0.05).mean() for nm in names])
  print("every series has %d surrogates with a tau: %s; fraction with ac p_rising <= 0.05 on this "
        "stationary series: %.3f" % (args.nsur, ok, frac))
  return 0 if ok else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 2 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 8 (64 with --time)")
  ap.add_argument("--years", type=int, default=120)
  ap.add_argument("--window", type=int, default=None, help="years; default 32 (256 with --time)")
  ap.add_argument("--step", type=int, default=None, help="years between windows; default 4 (8 with --time)")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the indicators")
  ap.add_argument("--nsur", type=int, default=None, help="surrogates; default 200 (1000 with --time)")
  ap.add_argument("--level", type=float, default=0.05)
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
  ap.add_argument("--host-members", type=int, default=16, help="with --time")
  ap.add_argument("--max-bytes", type=int, default=2 << 30, help="with --time: of a chunk's series")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 2)
  args.realisations = args.realisations or (64 if args.time else 8)
  args.window = args.window or (256 if args.time else 32)
  args.step = args.step or (8 if args.time else 4)
  args.nsur = args.nsur or (1000 if args.time else 200)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < args.window:
    ap.error("--years less --spinup must be at least --window")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
