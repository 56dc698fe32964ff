#!/usr/bin/env python3
"""The surrogate significance of the AMOC's early-warning trends under two null models: AR(1) and
Fourier phase-randomised surrogates -- both computed on the device.

The experiment is the one of examples/amoc_significance.py: `--sets` parameter sets x
`--realisations` realisations warm under a ForcingSchedule ramp while NoiseForcing drives the
realisations of a set apart, and an IndexRecorder keeps every member's AMOC maximum below 500 m
once a year.  pymoc_amd.SeriesWindows.significance tests Kendall's tau of the sliding-window
variance and lag-1 autocorrelation against `--nsur` surrogates of every member's detrended series.
With method="ar1" a surrogate is a stationary AR(1) series with the record's variance and lag-1
autocorrelation; with method="fourier" it keeps the record's whole periodogram and only its
phases are drawn anew -- the null model where the index is not AR(1) (a decadal spectral peak, the
band-limited response of the column model to white wind noise: examples/amoc_spectrum.py).
Printed per set: the fraction of members with p_rising <= `--level` under either null.

    python examples/amoc_significance_fourier.py --sets 2 --realisations 8 --years 120 --window 32
    python examples/amoc_significance_fourier.py --time   # the coefficient launch, one synthesis
                                                  # launch per chunk and the whole significance()
                                                  # under both nulls at 4096 members x 8 indices x
                                                  # 1200 records, W = 256, S = 8, next to the host
                                                  # route
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
from pymoc_amd import fourier
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.series import Ctx
from pymoc_amd.steady import YEAR
from pymoc_amd.surrogates import SeriesSurrogates, chunk_size
from pymoc_amd.windows import stt_of
from amoc_early_warning import _median_ms, ramp, sweep  # the same experiment
from amoc_significance import fraction
import windows_cases as WC

METHODS = (("ar1", "AR(1)"), ("fourier", "Fourier"))


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
  sig = {m: sw.significance(k0, k1, nsur=args.nsur, seed=args.surrogate_seed, method=m)
         for m, _ in METHODS}
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR, args.seed))
  print("AMOC maximum below 500 m, years %d-%d: %d windows of %d years every %d years, linear "
        "trend removed, lag 1; %d surrogates per member and null model, seed %d"
        % (k0, k1 - 1, sw.nwin(k0, k1), args.window, args.step, args.nsur, args.surrogate_seed))
  print("fraction of the members of a set with p_rising <= %g:" % args.level)
  print("  set  what  members  median tau    AR(1)  Fourier")
  ok = True
  for g in range(args.sets):
    for key in ("ac", "var"):
      r = {m: getattr(sig[m], key) for m, _ in METHODS}
      frac = [fraction(r[m].p_rising["amoc"], groups, g, args.level) for m, _ in METHODS]
      tau = r["ar1"].tau["amoc"][groups == g]
      ok &= all(bool(np.isfinite(f)) for f in frac)
      ok &= all(bool((r[m].nvalid["amoc"][groups == g] == args.nsur).all()) for m, _ in METHODS)
      ok &= bool(np.array_equal(r["ar1"].tau["amoc"], r["fourier"].tau["amoc"], equal_nan=True))
      print("  %3d  %4s  %7d  %10.3f  %7.3f  %7.3f"
            % (g, key, int((groups == g).sum()), float(np.nanmedian(tau)), frac[0], frac[1]))
  print("every member has a tau and %d surrogates with one under both null models: %s"
        % (args.nsur, ok))
  return 0 if ok else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the coefficient launch and of one synthesis
  launch per chunk, and the wall time of the whole significance() under either null, on a
  synthetic AR(1) series of `--sets` x `--realisations` members, 8 indices and `--records` records;
  next to them the host route on one core for ONE surrogate of `--host-members` members (NumPy's
  rfft / irfft and generator, then the restated windows), scaled to all members and `--nsur`
  surrogates."""
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
  two = fourier.wants_scratch(K)  # the synthesis stores through a second array and transposes
  nb = chunk_size(args.nsur, args.max_bytes, K, nspec, n, per=16 if two else 8)
  nb_ar1 = chunk_size(args.nsur, args.max_bytes, K, nspec, n)
  planes = nb * nspec
  print("%d members, %d indices, %d records (M = %d): a series of %.1f MB; window %d, step %d: %d "
        "windows; chunks of %d surrogates (%.1f MB); empty span %.1f us subtracted"
        % (n, nspec, K, fourier.m_of(K), v.nbytes / 1e6, W, S, sw.nwin(), nb, nb * v.nbytes / 1e6,
           1e3 * null))
  gen = SeriesSurrogates((dev, names), seed=args.surrogate_seed, method="fourier")
  tab, ctx = gen.tables(K), Ctx(None, None)
  coef = gen._coefficients(0, K, K)  # warm-up, and the tables' upload
  y = DeviceArray((K, planes, n), np.float64)
  scratch = DeviceArray((K, planes, n), np.float64)
  direct = lambda: fourier.launch_synthesis(y, coef, nspec, 0, gen.seed, gen.member0, tab, ctx)
  through = lambda: fourier.launch_synthesis(y, coef, nspec, 0, gen.seed, gen.member0, tab, ctx,
                                             scratch)
  direct()
  through()
  synchronize()
  t_coef = _median_ms(lambda: fourier.launch_coef(dev, 0, K, sw._par.detrend, stt_of(K), tab, ctx,
                                                  out=coef), args.reps) - null
  t_syn = {False: _median_ms(direct, args.reps) - null, True: _median_ms(through, args.reps) - null}
  print("  k_series_fourier_coef:           %10.1f us, once per significance()" % (1e3 * t_coef))
  for route, what in ((False, "stored directly"), (True, "through a scratch array, transposed")):
    print("  k_series_surrogates_fourier, %s: %10.1f us per chunk of %d surrogates: %.3f us a "
          "series, %.1f MB written%s" % (what, 1e3 * t_syn[route], nb, 1e3 * t_syn[route] / (planes * n),
                                        nb * v.nbytes / 1e6, " (the route taken)" if route == two else ""))
  del y, scratch
  synchronize()
  wall = {}
  for method, label in METHODS:
    t0 = time.perf_counter()
    sig = sw.significance(nsur=args.nsur, seed=args.surrogate_seed, max_bytes=args.max_bytes,
                          method=method)
    wall[method] = time.perf_counter() - t0
    ok = all((getattr(sig, key).nvalid[nm] == args.nsur).all() for key in ("var", "ac") for nm in names)
    frac = np.mean([(sig.ac.p_rising[nm] <= 0.05).mean() for nm in names])
    print("  significance(nsur = %d, method = \"%s\"): %10.1f ms wall, %d chunks; every series has "
          "%d surrogates with a tau: %s; fraction with ac p_rising <= 0.05 on this stationary "
          "series: %.3f" % (args.nsur, method, 1e3 * wall[method],
                            -(-args.nsur // (nb if method == "fourier" else nb_ar1)), args.nsur,
                            ok, frac))
    if not ok:
      return 1
  # the host route on one core: ONE surrogate of the first members, scaled
  hm = min(args.host_members, n)
  host = v[:, :, :hm]
  t0 = time.perf_counter()
  t = np.arange(K) - 0.5 * (K - 1)
  r = host - host.mean(axis=0) - (t[:, None, None] * host).sum(axis=0) / (t * t).sum() * t[:, None, None]
  R = np.fft.rfft(r, axis=0)
  ph = np.exp(2j * np.pi * np.random.default_rng(1).random(R.shape))
  ph[0] = 1.0
  if K % 2 == 0:
    ph[-1] = 1.0
  ys = np.fft.irfft(R * ph, n=K, axis=0)
  t_gen = time.perf_counter() - t0
  t0 = time.perf_counter()
  WC.windows(ys, 0, K, W, S, 1, "linear")
  t_win = time.perf_counter() - t0
  scale = n / hm * args.nsur
  print("  host, one core (one surrogate of %d members, scaled to %d members x %d surrogates): "
        "rfft / irfft %.0f s, the indicators %.0f s (and kendalltau as in amoc_significance.py)"
        % (hm, n, args.nsur, t_gen * scale, t_win * scale))
  return 0


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
  ap.add_argument("--reps", type=int, default=7)
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
