#!/usr/bin/env python3
"""Variability spectrum of the AMOC, and its coherence with the wind, in a stochastically forced
Jansen & Nadeau (2018) sweep -- computed on the device.

The experiment of examples/stochastic_amoc.py as `--sets` parameter sets x `--realisations`
realisations (`--members` = their product, set directly: one set).  An IndexRecorder keeps, once a
year, every member's wind stress (the forcing index) and its AMOC maximum below 500 m in a device
series.  pymoc_amd.SeriesSpectra transforms that series where it lives (Welch: segments of
`--nperseg` years, half overlapping, Hann window, mean removed) and only results are downloaded:
  across_members   per set and frequency: the group-mean AMOC spectrum and its 5-95 % band over
                   the realisations -- no per-member spectrum leaves the device
  compute          per member: the wind-AMOC cross spectrum; printed: the coherence, averaged
                   over the realisations of a set
The script then downloads the series and checks the printed spectra, bit for bit, against the
NumPy restatement of the definitions (tests/spectra_cases.py, tests/stats_cases.py).

    python examples/amoc_spectrum.py --sets 4 --realisations 16 --years 300 --nperseg 64
    python examples/amoc_spectrum.py --time   # the launch, with pairs, across_members, compute()
                                              # and the host route at 4096 members x 8 indices x
                                              # 1200 records
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # spectra_cases, stats_cases: the restatements
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import DeviceArray, Event, LaunchTimer, synchronize
from pymoc_amd.spectra import twiddles
from pymoc_amd.steady import YEAR
import spectra_cases as SC
import stats_cases as STC

QUANTILES = (0.05, 0.95)
PAIR = ("wind", "amoc")
COPY_RATE = 6.29e12  # bytes / s a plain device copy reaches


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


def run(args):
  cfg, groups = sweep(args.sets, args.realisations, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  noise = pymoc_amd.NoiseForcing(args.seed, tau=dict(sigma=args.sigma_tau),
                                 bs_north=dict(sigma=args.sigma_bs_north,
                                               tau_corr=args.tau_corr * YEAR))
  ens = pymoc_amd.JN2018Ensemble(cfg, noise=noise)
  tau = ens.so.tau  # one wind stress per member, or a profile on y: its maximum is the index
  wind = (tau, ens.so.y_host) if len(tau.shape) == 2 else (tau, np.zeros(1), 1)
  specs = [("wind", "max", "tau", {}), ("amoc", "max", "Psi", dict(zhi=-500.))]
  rec = pymoc_amd.IndexRecorder(ens, specs, M, args.years, sources=dict(tau=wind))
  ens.run((args.years - 1) * M + 1)
  sp = pymoc_amd.SeriesSpectra(rec, args.nperseg, pairs=[PAIR], dt_record=1.0, groups=groups)
  k0 = args.spinup
  across = sp.across_members(k0, args.years, quantiles=QUANTILES)
  res = sp.compute(k0, args.years)
  print("%d sets x %d realisations, %d years; noise seed %d: tau white, sigma %g N/m2; bs_north "
        "red, sigma %g m/s2, decorrelation %g years"
        % (args.sets, args.realisations, args.years, args.seed, args.sigma_tau,
           args.sigma_bs_north, args.tau_corr))
  print("Welch spectra of years %d-%d: %d segments of %d years, half overlapping, Hann window, "
        "mean removed" % (k0, args.years - 1, sp.nseg(k0, args.years), args.nperseg))
  print("AMOC maximum below 500 m: power spectral density [Sv^2 year] across the realisations of "
        "a set, and the wind-AMOC coherence averaged over them:")
  print("  set  cycles/year  members                group mean                        5%"
        "                       95%  coherence")
  mean, q, count = across.mean["amoc"], across.quantile["amoc"], across.count["amoc"]
  coh = res.coherence[PAIR]
  for g in range(args.sets):
    cg = np.nanmean(coh[groups == sp.group_labels[g]], axis=0)
    for f in range(sp.nf):
      print("  %3d  %11.6f  %7d  %24.17e  %24.17e  %24.17e  %9.6f"
            % (sp.group_labels[g], sp.freq[f], count[g, f], mean[g, f], q[0, g, f], q[1, g, f],
               cg[f]))
  # the host route, for the check: the whole series, the restatement of the definitions
  series = np.ascontiguousarray(np.stack([rec.values[nm].T for nm in sp.names], axis=1))
  if args.save_series:
    np.savez(args.save_series, series=series, groups=groups, k0=k0, k1=args.years,
             nperseg=args.nperseg, window=sp.window, scale=sp.scale)
  want = SC.spectra(series, k0, args.years, args.nperseg, sp.noverlap, sp.window, "constant",
                    ((0, 1),), sp.scale, twiddles(args.nperseg))
  order, start = STC.order_of(groups)
  wc, ws = STC.group_stats(want["psd"], order, start, QUANTILES, 0, sp.nf)
  ok = all(same_bits(res.psd[nm], want["psd"][:, s].T) for s, nm in enumerate(sp.names))
  ok &= same_bits(res.csd[PAIR].real + 0.0, want["csd"][:, 0].T + 0.0)  # (the sign of a zero)
  ok &= same_bits(res.csd[PAIR].imag + 0.0, want["csd"][:, 1].T + 0.0)
  ok &= np.array_equal(count, wc[:, 1, :].T) and same_bits(mean, ws[:, 1, :, 0].T)
  ok &= same_bits(q, ws[:, 1, :, 5:].transpose(2, 1, 0))
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
  """hipEvent medians of the launch alone (the empty span subtracted), without and with 4 pairs,
  and with across_members' reduction behind it, on a synthetic AR(1) series of `--sets` x
  `--realisations` members, 8 indices and `--records` records; compute() with its downloads and
  the host route (the download of the series, scipy.signal.welch on one core) next to them."""
  import scipy.signal
  n, nspec, nrec, L = args.sets * args.realisations, 8, args.records, args.nperseg
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, nspec, n))
  x = rng.standard_normal((nspec, n))
  for k in range(nrec):  # red noise about 15 Sv, decorrelation ten records
    x = 0.9 * x + np.sqrt(1 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = 15.0 + x
  groups = np.repeat(np.arange(args.sets), args.realisations)
  dev = DeviceArray.from_host(v)
  names = ["index%d" % i for i in range(nspec)]
  pairs = [(names[0], names[i]) for i in range(1, 5)]
  sp = pymoc_amd.SeriesSpectra((dev, names), L, pairs=pairs, groups=groups)
  nseg, nf = sp.nseg(), sp.nf
  o0, o4 = sp._launch(0, nrec, npairs=0), sp._launch(0, nrec)  # warm-up and the uploads
  st = pymoc_amd.SeriesStats((o0[1], names), groups=groups, quantiles=QUANTILES)
  og = st._launch_group(0, nf)
  synchronize()
  null = LaunchTimer().null_span_ms()
  t0p = _median_ms(lambda: sp._launch(0, nrec, out=o0, npairs=0), args.reps) - null
  t4p = _median_ms(lambda: sp._launch(0, nrec, out=o4), args.reps) - null

  def across():
    sp._launch(0, nrec, out=o0, npairs=0)
    st._launch_group(0, nf, out=og)
  t_across = _median_ms(across, args.reps) - null
  walls = []
  for _ in range(args.reps):
    t0 = time.perf_counter()
    res = sp.compute()
    walls.append(time.perf_counter() - t0)
  t_compute = sorted(walls)[len(walls) // 2]
  used = (L + (nseg - 1) * sp.step) * nspec * n * 8       # the records that lie in a segment
  wrote = (nf * 8 + 4) * nspec * n
  must = used + wrote
  t0 = time.perf_counter()
  host = dev.download()
  t_down = time.perf_counter() - t0
  t0 = time.perf_counter()
  _, pw = scipy.signal.welch(host, fs=1.0, window="hann", nperseg=L, noverlap=L // 2,
                             detrend="constant", scaling="density", axis=0)
  t_scipy = time.perf_counter() - t0
  close = np.allclose(res.psd[names[3]], pw[:, 3, :].T, rtol=1e-9, atol=1e-12 * pw.max())
  print("%d members (%d sets x %d), %d indices, %d records: a series of %.1f MB; nperseg %d, %d "
        "segments (empty span %.1f us subtracted)"
        % (n, args.sets, args.realisations, nspec, nrec, v.nbytes / 1e6, L, nseg, 1e3 * null))
  print("k_series_spectra, no pairs:  %8.1f us  must read %.1f MB and write %.1f MB: %.1f us at "
        "%.2f TB/s, %.1f %% of the copy rate reached"
        % (1e3 * t0p, used / 1e6, wrote / 1e6, 1e6 * must / COPY_RATE, COPY_RATE / 1e12,
           100. * must / COPY_RATE / (1e-3 * t0p)))
  print("k_series_spectra, 4 pairs:   %8.1f us  (16 transforms of a tile and segment against 8)"
        % (1e3 * t4p))
  print("across_members on top:       %8.1f us  (the launch, then k_series_group_stats over %d "
        "frequencies)" % (1e3 * t_across, nf))
  print("compute() with its downloads (4 pairs): %.1f ms" % (1e3 * t_compute))
  print("host route: download of the series %.1f ms, scipy.signal.welch on one core %.1f ms"
        % (1e3 * t_down, 1e3 * t_scipy))
  print("host and device agree (tolerance): %s" % close)
  return 0 if close else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--members", type=int, default=None,
                  help="one set of so many realisations (instead of --sets / --realisations)")
  ap.add_argument("--years", type=int, default=300)
  ap.add_argument("--nperseg", type=int, default=None, help="default 64 (256 with --time)")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the spectra")
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
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  if args.members:
    args.sets, args.realisations = 1, args.members
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  args.nperseg = args.nperseg or (256 if args.time else 64)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < args.nperseg:
    ap.error("--years less --spinup must be at least --nperseg")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
