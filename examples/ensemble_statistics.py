#!/usr/bin/env python3
"""Ensemble statistics of a stochastically forced Jansen & Nadeau (2018) sweep, reduced on the
device.

The experiment of examples/stochastic_amoc.py as `--sets` parameter sets x `--realisations`
realisations: the members of a set are copies of one config5 member, driven apart by wind and
northern-buoyancy noise that is generated on the device (pymoc_amd.NoiseForcing).  An
IndexRecorder keeps every member's AMOC maximum below 500 m once a year in a device series;
pymoc_amd.SeriesStats reduces that series where it lives, and only the results are downloaded:
  across_members   per set and year: the ensemble mean, the spread and the 5 / 50 / 95 % quantiles
                   (printed at the last year of every `--print-years` block)
  along_time       per member: the variance in time, the lag-1 and lag-10 autocovariance, the first
                   year the index falls below `--threshold` times its initial value
The script then downloads the series and checks every printed number, bit for bit, against the
NumPy restatement of the definitions (tests/stats_cases.py).

    python examples/ensemble_statistics.py --sets 4 --realisations 16 --years 60
    python examples/ensemble_statistics.py --time   # both launches and the host route at 4096
                                                    # members x 8 indices x 1200 records
                                                    # 
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # stats_cases: the restatement
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import DeviceArray, Event, LaunchTimer, synchronize
from pymoc_amd.steady import YEAR
import stats_cases as SC

SPECS = [("amoc", "max", "Psi", dict(zhi=-500.))]
QUANTILES = (0.05, 0.5, 0.95)
LAGS = (1, 10)


def sweep(sets, realisations, nz, dt_days):
  """`sets` config5 members, each repeated `realisations` times; the labels of the sets."""
  one = configs.config5(N=sets, nz=nz, dt_days=dt_days)
  cfg = dict(one)
  for key in pymoc_amd.JN2018Ensemble.MEMBER_KEYS:
    a = np.asarray(one.get(key, 0.0))
    if a.ndim >= 1 and a.shape[0] == sets:
      cfg[key] = np.repeat(a, realisations, axis=0)
  return cfg, np.repeat(np.arange(sets), realisations)


def same_bits(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  nan = np.isnan(a) & np.isnan(b)
  return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def check(st, across, along, series, groups, k_along, thr):
  """Every result against the restatement on the downloaded series [years, 1, members]."""
  order, start = SC.order_of(groups)
  K = series.shape[0]
  wc, ws = SC.group_stats(series, order, start, st.quantiles, 0, K)
  mc, mf, mx, ms = SC.member_stats(series, tuple(st.lags), [thr], [-1], k_along, K)
  ok = np.array_equal(across.count["amoc"], wc[:, 0, :].T)
  for i, key in enumerate(("mean", "var", "min", "max", "sum")):
    ok &= same_bits(getattr(across, key)["amoc"], ws[:, 0, :, i].T)
  ok &= same_bits(across.quantile["amoc"], ws[:, 0, :, 5:].transpose(2, 1, 0))
  ok &= np.array_equal(along.count["amoc"], mc[0]) and np.array_equal(along.first["amoc"], mf[0])
  ok &= np.array_equal(along.ncross["amoc"], mx[0])
  for i, key in enumerate(("mean", "var", "min", "max", "sum", "frac")):
    ok &= same_bits(getattr(along, key)["amoc"], ms[0, :, i])
  ok &= same_bits(along.autocov["amoc"], ms[0, :, 6:].T)
  return bool(ok)


def run(args):
  cfg, groups = sweep(args.sets, args.realisations, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  noise = pymoc_amd.NoiseForcing(args.seed, tau=dict(sigma=args.sigma_tau),
                                 bs_north=dict(sigma=args.sigma_bs_north,
                                               tau_corr=args.tau_corr * YEAR))
  ens = pymoc_amd.JN2018Ensemble(cfg, noise=noise)
  rec = pymoc_amd.IndexRecorder(ens, SPECS, M, args.years)  # a sample at the top of every year
  ens.run((args.years - 1) * M + 1)
  # the threshold: a fraction of the sweep's mean initial index (one small reduction on the device)
  first = pymoc_amd.SeriesStats(rec, groups=groups).across_members(0, 1)
  level = args.threshold * float(first.mean["amoc"][:, 0].mean())
  st = pymoc_amd.SeriesStats(rec, groups=groups, quantiles=QUANTILES, lags=LAGS,
                             thresholds=dict(amoc=(level, "below")))
  across = st.across_members()
  k_along = min(args.spinup, args.years - 11)
  along = st.along_time(k_along, args.years)
  print("%d sets x %d realisations, %d years; noise seed %d: tau white, sigma %g N/m2; bs_north "
        "red, sigma %g m/s2, decorrelation %g years"
        % (args.sets, args.realisations, args.years, args.seed, args.sigma_tau,
           args.sigma_bs_north, args.tau_corr))
  print("AMOC maximum below 500 m [Sv] across the realisations of a set, at the last year of every "
        "%d years:" % args.print_years)
  print("  set  year  finite       mean     spread         5%        50%        95%")
  mean, var, q = across.mean["amoc"], across.var["amoc"], across.quantile["amoc"]
  for g in range(args.sets):
    for y in range(args.print_years - 1, args.years, args.print_years):
      print("  %3d  %4d  %6d %10.5f %10.5f %10.5f %10.5f %10.5f"
            % (st.group_labels[g], y, across.count["amoc"][g, y], mean[g, y], np.sqrt(var[g, y]),
               q[0, g, y], q[1, g, y], q[2, g, y]))
  print("In time, years %d-%d, per member (threshold %.5f Sv = %g x the initial mean):"
        % (k_along, args.years - 1, level, args.threshold))
  print("  set  member   variance  autocov(1) autocov(10)  first year below")
  shown = range(ens.n) if ens.n <= 16 else range(0, ens.n, args.realisations)
  for m in shown:
    f = along.first["amoc"][m]
    print("  %3d  %6d %10.6f %11.6f %11.6f  %s"
          % (groups[m], m, along.var["amoc"][m], along.autocov["amoc"][0, m],
             along.autocov["amoc"][1, m], "never" if f < 0 else "%d" % f))
  if ens.n > 16:
    print("  (the first member of every set; %d members in all, %d of them fall below)"
          % (ens.n, int((along.first["amoc"] >= 0).sum())))
  series = rec.values["amoc"].T[:, None, :]  # the host route: the whole series, for the check
  ok = check(st, across, along, np.ascontiguousarray(series), groups, k_along, level)
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


def _host_route(dev, groups, k_along, level):
  """The download of the series, then the same statistics in NumPy: seconds for each."""
  t0 = time.perf_counter()
  v = dev.download()
  t1 = time.perf_counter()
  nrec, nspec, n = v.shape
  sets = v.reshape(nrec, nspec, groups.max() + 1, -1)  # (contiguous sets of equal size)
  out = [sets.mean(axis=3), sets.var(axis=3, ddof=1), sets.min(axis=3), sets.max(axis=3),
         np.quantile(sets, QUANTILES, axis=3)]
  w = v[k_along:]
  d = w - w.mean(axis=0)
  out += [w.var(axis=0, ddof=1), w.min(axis=0), w.max(axis=0)]
  out += [(d[:-L] * d[L:]).mean(axis=0) for L in LAGS]
  hit = w < level
  out += [hit.mean(axis=0), hit.argmax(axis=0), (hit[1:] != hit[:-1]).sum(axis=0)]
  return t1 - t0, time.perf_counter() - t1, out


def time_it(args):
  """hipEvent medians of the two launches alone (the empty span subtracted) on a synthetic AR(1)
  series of `--sets` x `--realisations` members, 8 indices and `--records` records, and the host
  route next to them."""
  n, nspec, nrec = args.sets * args.realisations, 8, args.records
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(nrec):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  groups = np.repeat(np.arange(args.sets), args.realisations)
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  level, k_along = 13.0, 0
  st = pymoc_amd.SeriesStats((dev, names), groups=groups, quantiles=QUANTILES, lags=LAGS,
                             thresholds={nm: (level, "below") for nm in names})
  # warm-up (and the uploads); the timed launches write the same result arrays again
  og, om = st._launch_group(0, nrec), st._launch_member(k_along, nrec)
  synchronize()
  null = LaunchTimer().null_span_ms()
  t_group = _median_ms(lambda: st._launch_group(0, nrec, out=og), args.reps) - null
  t_member = _median_ms(lambda: st._launch_member(k_along, nrec, out=om), args.reps) - null
  t0 = time.perf_counter()
  across, along = st.across_members(), st.along_time(k_along, nrec)
  t_calls = time.perf_counter() - t0
  t_down, t_numpy, host = _host_route(dev, groups, k_along, level)
  close = (np.allclose(across.mean["index0"], host[0][:, 0].T, rtol=1e-12) and
           np.allclose(along.var["index3"], host[5][3], rtol=1e-10) and
           np.array_equal(across.quantile["index7"], host[4][:, :, 7].transpose(0, 2, 1)))
  series = v.nbytes
  print("%d members (%d sets x %d), %d indices, %d records: a series of %.1f MB (empty span "
        "%.1f us subtracted)" % (n, args.sets, args.realisations, nspec, nrec, series / 1e6,
                                 1e3 * null))
  print("k_series_group_stats:  %8.1f us  reads the series once: %.1f MB, %.2f TB/s"
        % (1e3 * t_group, series / 1e6, series / (1e-3 * t_group) / 1e12))
  print("k_series_member_stats: %8.1f us  two passes over the series and one per lag: %.1f MB "
        "of loads, %.1f MB distinct, %.2f TB/s of loads"
        % (1e3 * t_member, (2 + len(LAGS)) * series / 1e6, series / 1e6,
           (2 + len(LAGS)) * series / (1e-3 * t_member) / 1e12))
  print("both calls with their result downloads: %.1f ms" % (1e3 * t_calls))
  print("host route: download of the series %.1f ms, the statistics in NumPy %.1f ms"
        % (1e3 * t_down, 1e3 * t_numpy))
  print("host and device agree (tolerance; the quantiles bit for bit): %s" % close)
  return 0 if close else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--years", type=int, default=60)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--print-years", type=int, default=10, help="years per printed row")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the time statistics")
  ap.add_argument("--threshold", type=float, default=0.9,
                  help="the level members are timed against, as a fraction of the initial mean")
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  if args.time:
    return time_it(args)
  if args.years < 12:
    ap.error("--years must be at least 12 (the lag-10 autocovariance needs 11 records)")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
