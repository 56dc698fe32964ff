#!/usr/bin/env python3
"""Degenerate fingerprinting (Held & Kleinen 2004) of the overturning in a ramped, stochastically
forced sweep, next to the AMOC maximum alone, computed on the device.

The experiment of examples/amoc_early_warning.py: `--sets` parameter sets x `--realisations`
realisations warm under a pymoc_amd.ForcingSchedule ramp while pymoc_amd.NoiseForcing drives the
realisations apart.  The IndexRecorder keeps, once a year, the AMOC maximum below 500 m AND the
streamfunction Psi at `--depths` (kind "at"): a coarse profile of the overturning.  Then, all
where the series lives:
  SeriesSmooth.residual()   the Gaussian-detrended series of every index
  SeriesEOF.pc()            its leading EOF -- one per parameter set from the pooled scatter of
                            the set's realisations, on the indices scaled to unit variance -- and
                            the principal component pc1, a device series of its own
  SeriesWindows             ac and var of pc1 per sliding window, their Kendall trends and, with
                            --significance, the AR(1)-surrogate test of the trends
and the same SeriesWindows calls on the residual of the AMOC maximum alone, side by side.  The
script then downloads the residual and checks pc1 and the fit against the NumPy restatement
(tests/eof_cases.py) bit for bit.  Whether the fingerprint shows more than the single index in
this ramp is an outcome, not a claim.

    python examples/amoc_fingerprint.py --sets 4 --realisations 16 --years 300 --significance
    python examples/amoc_fingerprint.py --time   # hipEvent medians of the three launches at 4096
                                                 # members x 8 indices x 1200 records against the
                                                 # copy rate, and the host route
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # eof_cases: the restatement
sys.path.insert(2, os.path.join(ROOT, "examples"))  # amoc_early_warning: the experiment
import pymoc_amd
from pymoc_amd.device import DeviceArray, LaunchTimer, synchronize
from pymoc_amd.eof import launch_eof, launch_project, launch_scatter, std_weights
from pymoc_amd.series import Ctx
from pymoc_amd.steady import YEAR
import amoc_early_warning as EW
import eof_cases as EC

KEYS = ("ac", "var")
ITERS = 64


def run(args):
  cfg, groups = EW.sweep(args.sets, args.realisations, args.nz, args.dt_days)
  M = int(cfg["MOC_up_iters"])  # one year
  noise = pymoc_amd.NoiseForcing(args.seed, tau=dict(sigma=args.sigma_tau),
                                 bs_north=dict(sigma=args.sigma_bs_north,
                                               tau_corr=args.tau_corr * YEAR))
  sched = EW.ramp(cfg, groups, args.sets, args.ramp_start, args.years)
  ens = pymoc_amd.JN2018Ensemble(cfg, forcing=sched, noise=noise)
  depths = [float(d) for d in args.depths.split(",")]
  profile = ["psi%d" % d for d in depths]
  specs = [("amoc", "max", "Psi", dict(zhi=-500.))] + [
      (nm, "at", "Psi", dict(x0=-d)) for nm, d in zip(profile, depths)]
  rec = pymoc_amd.IndexRecorder(ens, specs, M, args.years)
  ens.run((args.years - 1) * M + 1)
  k0, k1 = args.spinup, args.years
  K = k1 - k0
  stream = ens.stream
  resid = pymoc_amd.SeriesSmooth(rec, args.sigma).residual(k0, k1)   # (device [K, nspec, n], names)
  se = pymoc_amd.SeriesEOF(resid, indices=profile, scale="std", groups=groups, pooled=True,
                           iters=ITERS, stream=stream)
  fit = se.fit()
  pc = se.pc()
  kw = dict(step=args.step, detrend="constant", groups=groups, stream=stream)
  both = (("pc1", "pc1", pymoc_amd.SeriesWindows(pc, args.window, **kw)),
          ("amoc", "amoc", pymoc_amd.SeriesWindows(resid, args.window, **kw)))
  print("%d sets x %d realisations, %d years; warming ramp over years %g-%g; noise seed %d"
        % (args.sets, args.realisations, args.years, args.ramp_start, sched.t[-1] / YEAR,
           args.seed))
  print("Psi at %s m and the AMOC maximum below 500 m, years %d-%d, Gaussian trend of sigma %g "
        "years removed; windows of %d years every %d years"
        % (", ".join("%g" % d for d in depths), k0, k1 - 1, args.sigma, args.window, args.step))
  print("leading EOF of the scaled profile, pooled over the realisations of a set (%d power "
        "iterations):" % ITERS)
  print("  set  records  variance held     residual  loadings (%s)" % " ".join(profile))
  for g in range(args.sets):
    print("  %3d  %7d  %13.6f  %11.3e  %s" % (fit.labels[g], fit.ntot[g], fit.frac[g], fit.resid[g],
                                              " ".join("%+.4f" % fit.eof[nm][g] for nm in profile)))
  trends = {what: sw.trend() for what, _, sw in both}
  print("Kendall's tau of the indicator against time, median over the members of a set:")
  print("  set                    ac pc1                   ac amoc                   var pc1"
        "                  var amoc")
  for g in range(args.sets):
    print("  %3d  %s" % (fit.labels[g], "  ".join(
        "%24.17e" % EW.summary(getattr(trends[what], key).tau[name], groups, fit.labels[g])[0]
        for key in KEYS for what, name, _ in both)))
  if args.significance:
    sigs = {what: sw.significance(nsur=args.nsur, seed=args.seed + 1) for what, _, sw in both}
    print("AR(1)-surrogate test, %d surrogates: fraction of the members of a set with p_rising "
          "<= %g:" % (args.nsur, args.level))
    print("  set    ac pc1   ac amoc   var pc1  var amoc")
    for g in range(args.sets):
      fr = []
      for key in KEYS:
        for what, name, _ in both:
          p = getattr(sigs[what], key).p_rising[name][groups == fit.labels[g]]
          p = p[~np.isnan(p)]
          fr.append(float((p <= args.level).mean()) if p.size else float("nan"))
      print("  %3d  %8.4f  %8.4f  %8.4f  %8.4f" % ((fit.labels[g],) + tuple(fr)))
  # the host route, for the check: the residual series, the restatement of the definition
  host = resid[0].download(stream=stream)
  names = resid[1]
  sel = np.array([names.index(nm) for nm in profile], dtype=np.int32)
  st = pymoc_amd.SeriesStats(resid, stream=stream).along_time()
  order, start = EC.order_of(groups)
  w = std_weights(np.stack([st.var[nm] for nm in profile]), order, start)
  want = EC.restate(dict(v=host, k0=0, k1=K, sel=sel, w=w, iters=ITERS, order=order, start=start))
  got = pc[0]._parent.download(stream=stream)
  ok = EW.same_bits(got, want["pc"]) and EW.same_bits(fit.lam, want["lam"])
  ok &= all(EW.same_bits(fit.eof[nm], want["eof"][j]) for j, nm in enumerate(profile))
  ok &= np.array_equal(fit.ntot, want["ntot"]) and EW.same_bits(fit.resid, want["resid"])
  print("restatement on the downloaded residual: pc1 and the fit %s"
        % ("every bit agrees" if ok else "MISMATCH"))
  return 0 if ok else 1


# ------------------------------------------------------------------ --time
def time_it(args):
  """hipEvent medians (the empty span subtracted) of the three launches on a synthetic series of
  `--sets` x `--realisations` members, 8 indices and `--records` records -- one shared AR(1) mode
  plus independent noise per index -- per member and pooled per set, each next to the bytes the
  launch must move at the copy rate; and the host route: the download of the series, then per
  member its covariance, np.linalg.eigh and the projection on one core, `--host-members` members
  timed and scaled to all."""
  n, q, nrec = args.sets * args.realisations, 8, args.records
  rng = np.random.default_rng(args.seed)
  v = np.empty((nrec, q, n))
  z, e = rng.standard_normal(n), rng.standard_normal((q, n))
  for k in range(nrec):
    z = 0.9 * z + np.sqrt(1 - 0.81) * rng.standard_normal(n)
    e = 0.3 * e + np.sqrt(1 - 0.09) * rng.standard_normal((q, n))
    v[k] = z[None, :] + 1.5 * e
  groups = np.repeat(np.arange(args.sets), args.realisations)
  dev = DeviceArray.from_host(v)
  sel = list(range(q))
  ctx = Ctx(None, None)
  null = LaunchTimer().null_span_ms()
  t0 = time.perf_counter()
  host = dev.download()
  t_down = time.perf_counter() - t0
  series = nrec * q * n * 8
  print("%d members (%d sets x %d), %d indices, %d records: a series of %.1f MB; %d power "
        "iterations (empty span %.1f us subtracted); download of the series %.1f ms"
        % (n, args.sets, args.realisations, q, nrec, series / 1e6, ITERS, 1e3 * null, 1e3 * t_down))

  def line(what, t, must, note=""):
    print("  %-18s %9.1f us  must move %7.2f MB: %6.1f us at %.2f TB/s, %5.1f %% of the copy rate "
          "reached%s" % (what, 1e3 * t, must / 1e6, 1e6 * must / EW.COPY_RATE, EW.COPY_RATE / 1e12,
                         100. * must / EW.COPY_RATE / (1e-3 * t), note))

  tri = q * (q + 1) // 2
  sc = launch_scatter(dev, 0, nrec, sel, None, ctx)  # warm-up
  synchronize()
  t_sc = EW._median_ms(lambda: launch_scatter(dev, 0, nrec, sel, None, ctx, out=sc), args.reps) - null
  line("k_series_scatter", t_sc, series + (4 + 8 * q + 8 * tri) * n, " (the series is walked twice)")
  order, start = EC.order_of(groups)
  od, sd = DeviceArray.from_host(order, dtype=np.int32), DeviceArray.from_host(start, dtype=np.int32)
  unit = DeviceArray.from_host(EC.unit_of(order, start, n), dtype=np.int32)
  res = {}
  for what, okw, u in (("per member", {}, None),
                       ("pooled", dict(order=od, start=start, start_dev=sd), unit)):
    ef = launch_eof(sc[0], sc[2], q, ITERS, ctx, **okw)
    pcs = launch_project(dev, 0, nrec, sel, None, sc[0], sc[1], ef[0], ctx, unit=u)
    synchronize()
    t_ef = EW._median_ms(lambda: launch_eof(sc[0], sc[2], q, ITERS, ctx, out=ef, **okw),
                         args.reps) - null
    t_pj = EW._median_ms(lambda: launch_project(dev, 0, nrec, sel, None, sc[0], sc[1], ef[0], ctx,
                                                unit=u, pc=pcs), args.reps) - null
    nu = ef[0].shape[1]
    print("%s: %d units" % (what, nu))
    line("k_series_eof", t_ef, (4 + 8 * tri) * n + (8 * q + 36) * nu)
    line("k_series_project", t_pj, series + nrec * n * 8 + (4 + 8 * q) * n + 8 * q * nu)
    res[what] = (ef[0].download(), pcs.download())
  # the host route on one core, on the first members: covariance, eigh, projection
  hm = min(args.host_members, n)
  t0 = time.perf_counter()
  worst = 0.0
  for m in range(hm):
    x = host[:, :, m] - host[:, :, m].mean(axis=0)
    lam, vec = np.linalg.eigh(x.T @ x / nrec)
    lead = vec[:, -1] / vec[np.argmax(np.abs(vec[:, -1])), -1]
    p = x @ lead
    worst = max(worst, float(np.abs(p - res["per member"][1][:, 0, m]).max() / np.abs(p).max()))
  t_host = (time.perf_counter() - t0) * n / hm
  print("host, one core (%d members, scaled to %d): covariance, np.linalg.eigh and projection "
        "%.1f ms, after the download of %.1f ms; largest |pc1 - host| / max |host| %.2e"
        % (hm, n, 1e3 * t_host, 1e3 * t_down, worst))
  want = EC.restate(dict(v=host[:, :, :hm], k0=0, k1=nrec, sel=np.arange(q), w=None, iters=ITERS,
                         order=None, start=None))
  ok = EW.same_bits(res["per member"][1][:, :, :hm], want["pc"])
  ok &= EW.same_bits(res["per member"][0][:, :hm], want["eof"])
  print("restatement and device agree bit for bit: %s" % bool(ok))
  return 0 if ok else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sets", type=int, default=None, help="default 4 (64 with --time)")
  ap.add_argument("--realisations", type=int, default=None, help="default 16 (64 with --time)")
  ap.add_argument("--years", type=int, default=300)
  ap.add_argument("--depths", default="300,600,1000,1500,2000,2800",
                  help="metres below the surface at which Psi is recorded")
  ap.add_argument("--sigma", type=float, default=20., help="years, of the Gaussian detrending")
  ap.add_argument("--window", type=int, default=64, help="years")
  ap.add_argument("--step", type=int, default=4, help="years between windows")
  ap.add_argument("--spinup", type=int, default=10, help="years left out of the analysis")
  ap.add_argument("--ramp-start", type=float, default=10.)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--seed", type=int, default=2018)
  ap.add_argument("--sigma-tau", type=float, default=0.02, help="N/m2, white")
  ap.add_argument("--sigma-bs-north", type=float, default=2e-4, help="m/s2, red")
  ap.add_argument("--tau-corr", type=float, default=10., help="years, of bs_north")
  ap.add_argument("--significance", action="store_true", help="the surrogate test of the trends")
  ap.add_argument("--nsur", type=int, default=199)
  ap.add_argument("--level", type=float, default=0.1)
  ap.add_argument("--time", action="store_true")
  ap.add_argument("--records", type=int, default=1200, help="with --time")
  ap.add_argument("--host-members", type=int, default=16, help="with --time")
  ap.add_argument("--reps", type=int, default=15)
  args = ap.parse_args()
  args.sets = args.sets or (64 if args.time else 4)
  args.realisations = args.realisations or (64 if args.time else 16)
  if args.time:
    return time_it(args)
  if args.years - args.spinup < args.window:
    ap.error("--years less --spinup must be at least --window")
  return run(args)


if __name__ == "__main__":
  sys.exit(main())
