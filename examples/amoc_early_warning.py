#!/usr/bin/env python3
"""Early-warning indicators of the AMOC in a ramped, stochastically forced Jansen & Nadeau (2018)
sweep -- computed on the device.

`--sets` parameter sets x `--realisations` realisations (`--members` = their product, set
directly: one set) warm under a pymoc_amd.ForcingSchedule ramp (the surface buoyancy of the basin,
the northern column and the channel's restoring profile alike, every set by its own amount) while
pymoc_amd.NoiseForcing drives the realisations of a set apart.  An IndexRecorder keeps every
member's AMOC maximum below 500 m once a year in a device series.  pymoc_amd.SeriesWindows reads
that series where it lives: the lag-1 autocorrelation and the variance of the linearly detrended
index in a sliding window of `--window` years, every `--step` years, and Kendall's tau of each
indicator against time -- critical slowing down shows as both rising.  Only results are downloaded:
  across_members   per set and window: the group mean of `ac` and of `var` and their 5-95 % band
                   over the realisations -- no per-member indicator leaves the device
  trend            per member: the Kendall counts of `var` and `ac`; printed per set: the median
                   tau and the fraction of members with tau > 0
The script then downloads the series and checks every printed number, bit for bit (the integers
exactly), against the NumPy restatement of the definitions (tests/windows_cases.py,
tests/stats_cases.py).  Whether this ramp shows a rising `ac` is an outcome, not a claim.

    python examples/amoc_early_warning.py --sets 4 --realisations 16 --years 300 --window 64
    python examples/amoc_early_warning.py --time   # the window launch, the Kendall launch,
                                                   # across_members and the host route at 4096
                                                   # members x 8 indices x 1200 records, W = 256,
                                                   # S = 8 and S = 1
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # windows_cases, stats_cases: the restatements
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import DeviceArray, Event, LaunchTimer, synchronize
from pymoc_amd.series import _Plane
from pymoc_amd.steady import YEAR
from pymoc_amd.windows import launch_kendall
import stats_cases as STC
import windows_cases as WC

QUANTILES = (0.05, 0.95)
COPY_RATE = 6.29e12  # bytes / s a plain device copy reaches
SHOWN = 5            # window ends printed per set


def sweep(sets, realisations, nz, dt_days):
  """`sets` config5 members, each repeated `realisations` times; the labels of the sets."""
  one = configs.config5(N=sets, nz=nz, dt_days=dt_days)
  cfg = dict(one)
  for key in pymoc_amd.JN2018Ensemble.MEMBER_KEYS:
    a = np.asarray(one.get(key, 0.0))
    if a.ndim >= 1 and a.shape[0] == sets:
      cfg[key] = np.repeat(a, realisations, axis=0)
  return cfg, np.repeat(np.arange(sets), realisations)


def ramp(cfg, groups, sets, start, end):
  """The warming of examples/jn2018_warming.py without its wind step: two knots, set g warming
  by 1e-3 .. 4e-3 m/s2 between them."""
  db = np.linspace(1e-3, 4e-3, sets)[groups]
  t = np.array([start, end]) * YEAR
  w = np.array([0.0, 1.0])
  up = lambda v: np.asarray(v)[None, :] + w[:, None] * db[None, :]  # noqa: E731
  rest = np.asarray(cfg["rest_mask"], dtype=np.float64) * np.ones_like(cfg["b_rest"])
  b_rest = cfg["b_rest"][None] + w[:, None, None] * db[None, :, None] * rest[None]
  same = lambda v: np.repeat(np.asarray(v)[None], 2, axis=0)  # noqa: E731
  return pymoc_amd.ForcingSchedule(t, bs=up(cfg["bs"]), bs_north=up(cfg["bs_north"]),
                                   tau=same(cfg["tau"]), b_rest=b_rest,
                                   surflux=same(cfg["surflux"]))


def same_bits(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  nan = np.isnan(a) & np.isnan(b)
  return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def summary(tau, groups, label):
  """(median tau, fraction of members with tau > 0) of a set; members without a tau are left out
  of both."""
  t = tau[groups == label]
  t = t[~np.isnan(t)]
  return (float(np.median(t)), float((t > 0).mean())) if t.size else (float("nan"), float("nan"))


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
  sw = pymoc_amd.SeriesWindows(rec, args.window, step=args.step, detrend="linear", lag=1,
                               groups=groups)
  k0, k1 = args.spinup, args.years
  nwin, ends = sw.nwin(k0, k1), sw.record_end(k0, k1)
  across = {key: sw.across_members(key, k0, k1, quantiles=QUANTILES) for key in ("ac", "var")}
  trend = sw.trend(k0, k1)
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d: tau "
        "white, sigma %g N/m2; bs_north red, sigma %g m/s2, decorrelation %g years"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR,
           args.seed, args.sigma_tau, args.sigma_bs_north, args.tau_corr))
  print("AMOC maximum below 500 m, years %d-%d: %d windows of %d years every %d years, linear "
        "trend removed, lag 1" % (k0, k1 - 1, nwin, args.window, args.step))
  print("across the realisations of a set, dated at the end of the window:")
  print("  set  what  year  members                group mean                        5%"
        "                       95%")
  shown = np.unique(np.linspace(0, nwin - 1, min(SHOWN, nwin)).astype(int))
  for g in range(args.sets):
    for key in ("ac", "var"):
      a = across[key]
      for i in shown:
        print("  %3d  %4s  %4d  %7d  %24.17e  %24.17e  %24.17e"
              % (sw.group_labels[g], key, ends[i], a.count["amoc"][g, i], a.mean["amoc"][g, i],
                 a.quantile["amoc"][0, g, i], a.quantile["amoc"][1, g, i]))
  print("Kendall's tau of the indicator against time, over the members of a set:")
  print("  set  what               median tau            fraction tau > 0")
  for g in range(args.sets):
    for key in ("ac", "var"):
      med, frac = summary(getattr(trend, key).tau["amoc"], groups, sw.group_labels[g])
      print("  %3d  %4s  %24.17e  %24.17e" % (sw.group_labels[g], key, med, frac))
  # the host route, for the check: the whole series, the restatement of the definitions
  series = np.ascontiguousarray(np.stack([rec.values[nm].T for nm in sw.names], axis=1))
  if args.save_series:
    np.savez(args.save_series, series=series, groups=groups, k0=k0, k1=k1, window=args.window,
             step=args.step)
  want = WC.windows(series, k0, k1, args.window, args.step, 1, "linear")
  order, start = STC.order_of(groups)
  ok = True
  for key, i in (("var", 2), ("ac", 3)):
    wc, ws = STC.group_stats(want["out"][i], order, start, QUANTILES, 0, nwin)
    a = across[key]
    ok &= np.array_equal(a.count["amoc"], wc[:, 0, :].T) and same_bits(a.mean["amoc"], ws[:, 0, :, 0].T)
    ok &= same_bits(a.quantile["amoc"], ws[:, 0, :, 5:].transpose(2, 1, 0))
    conc, disc, tie, nfin = WC.kendall(want["out"][i], 0, nwin)
    tr = getattr(trend, key)
    ok &= all(np.array_equal(got["amoc"], w[0]) for got, w in
              ((tr.conc, conc), (tr.disc, disc), (tr.tie, tie), (tr.nfin, nfin)))
    tau = WC.tau_b(conc[0], disc[0], tie[0])
    ok &= same_bits(tr.tau["amoc"], tau)
    ok &= all(same_bits(summary(tr.tau["amoc"], groups, g), summary(tau, groups, g))
              for g in sw.group_labels)
  print("restatement on the downloaded series: %s" % ("every bit agrees" if ok else "MISMATCH"))
  return 0 if ok else 1


# ------------------------------------------------------------------ --time
def _median_ms(fn, reps):
  spans = []
  for _ in range(reps):
    e0, e1 = Event(), Event()
    e0.record()
    fn()
    e1.record()
    spans.append((e0, e1))
  synchronize()
  v = sorted(e0.elapsed_ms(e1) for e0, e1 in spans)
  return v[len(v) // 2]


def time_it(args):
  """hipEvent medians (the empty span subtracted) of the window launch, of the Kendall launch over
  its `ac` series and of across_members' two launches, for `--step` 8 and 1, on a synthetic AR(1)
  series of `--sets` x `--realisations` members, 8 indices and `--records` records; next to them
  the download of the series and the same numbers on the host on one core (the restatement and
  scipy.stats.kendalltau on `--host-members` members, scaled to all)."""
  import scipy.stats
  n, nspec, nrec, W = args.sets * args.realisations, 8, args.records, args.window
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(nrec):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  groups = np.repeat(np.arange(args.sets), args.realisations)
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  null = LaunchTimer().null_span_ms()
  t0 = time.perf_counter()
  host = dev.download()
  t_down = time.perf_counter() - t0
  print("%d members (%d sets x %d), %d indices, %d records: a series of %.1f MB; window %d "
        "(empty span %.1f us subtracted); download of the series %.1f ms"
        % (n, args.sets, args.realisations, nspec, nrec, v.nbytes / 1e6, W, 1e3 * null,
           1e3 * t_down))
  hm = min(args.host_members, n)
  ok = True
  for S in (8, 1):
    sw = pymoc_amd.SeriesWindows((dev, names), W, step=S, groups=groups)
    nwin = sw.nwin()
    shape = (nwin, nspec, n)
    out = sw._launch(0, nrec, nwin)  # warm-up
    st = pymoc_amd.SeriesStats((_Plane(out[0], 3, shape), names), groups=groups,
                               quantiles=QUANTILES)
    og = st._launch_group(0, nwin)
    synchronize()
    t_win = _median_ms(lambda: sw._launch(0, nrec, nwin, out=out), args.reps) - null
    counts = launch_kendall(_Plane(out[0], 3, shape), shape, 0, nwin, None, None)
    kd = lambda: launch_kendall(_Plane(out[0], 3, shape), shape, 0, nwin, None, None,  # noqa: E731
                                out=counts)
    t_kd = _median_ms(kd, args.reps) - null

    def across():
      sw._launch(0, nrec, nwin, out=out)
      st._launch_group(0, nwin, out=og)
    t_across = _median_ms(across, args.reps) - null
    used = (W + (nwin - 1) * S) * nspec * n * 8  # the records that lie in a window
    wrote = (4 * nwin * 8 + 4) * nspec * n
    must = used + wrote
    res = out[0].download()
    # the host route on one core, on the first members
    t0 = time.perf_counter()
    want = WC.windows(host[:, :, :hm], 0, nrec, W, S, 1, "linear")
    t_host = (time.perf_counter() - t0) * n / hm
    t0 = time.perf_counter()
    for m in range(hm):
      scipy.stats.kendalltau(np.arange(nwin), want["out"][3][:, 0, m])
    t_hk = (time.perf_counter() - t0) * nspec * n / hm
    ok &= same_bits(res[..., :hm], want["out"])
    print("step %d: %d windows" % (S, nwin))
    print("  k_series_windows:      %9.1f us  must read %.1f MB and write %.1f MB: %.1f us at "
          "%.2f TB/s, %.1f %% of the copy rate reached"
          % (1e3 * t_win, used / 1e6, wrote / 1e6, 1e6 * must / COPY_RATE, COPY_RATE / 1e12,
             100. * must / COPY_RATE / (1e-3 * t_win)))
    print("  k_series_kendall (ac): %9.1f us  %.3g comparisons; must read %.1f MB: %.1f us at "
          "%.2f TB/s" % (1e3 * t_kd, 0.5 * nwin * (nwin - 1) * nspec * n,
                         nwin * nspec * n * 8 / 1e6, 1e6 * nwin * nspec * n * 8 / COPY_RATE,
                         COPY_RATE / 1e12))
    print("  across_members(ac):    %9.1f us  (the launch, then k_series_group_stats over %d "
          "windows)" % (1e3 * t_across, nwin))
    print("  host, one core (%d members, scaled to %d): the indicators %.1f s, kendalltau %.1f s"
          % (hm, n, t_host, t_hk))
  print("host and device agree bit for bit: %s" % ok)
  return 0 if ok else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--members", type=int, default=None,
                  help="one set of so many realisations (instead of --sets / --realisations)")
  ap.add_argument("--years", type=int, default=300)
  ap.add_argument("--window", type=int, default=None, help="years; default 64 (256 with --time)")
  ap.add_argument("--step", type=int, default=4, help="years between windows")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the indicators")
  ap.add_argument("--ramp-start", type=float, default=10.)
  ap.add_argument("--ramp-end", type=float, default=None, help="default: the last year")
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--save-series", default=None,
                  help="write the downloaded series and the settings to this .npz")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--host-members", type=int, default=16, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  if args.members:
    args.sets, args.realisations = 1, args.members
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  args.window = args.window or (256 if args.time else 64)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < args.window:
    ap.error("--years less --spinup must be at least --window")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
