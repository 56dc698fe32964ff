#!/usr/bin/env python3
"""What twobasin_NadeauJansen.py (PyMOC's two-basin script) builds after its loop, :157-262 -- the
depth-space, isopycnal and residual overturning of the globe, the Atlantic and the Pacific on the
section channel + basin + northern transition + northern sinking region -- for EVERY member of a
two-basin ensemble, built on the GPU from the ensemble's device state, and each basin's cell
strengths.

The ensemble is time-stepped (TwoBasinEnsemble); TwoBasinOverturningSections.from_ensemble then
reads its rows in place: the preparation launch, two SectionBatch launches, two thermal-wind and
two Southern-Ocean solves into private buffers, and one launch of the kernel -- no round trip
through the host, and the ensemble's own diagnostics stay untouched.

    python examples/twobasin_overturning.py --members 64 --steps 121
    python examples/twobasin_overturning.py --time     # 2048 members, nz = 80, hipEvent timing
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.twobasin_overturning import FIELDS, STORE, twobasin_section_rows


def host_fields(y, k, n_basin=60, n_trans=20, n_north=20):
  """One member's eight fields in NumPy on the host (what the device computes, row block by row
  block), k the member's rows by name: -> {name: [nrows][nz]}."""
  r, itp = twobasin_section_rows(y), np.interp
  ny, t0 = y.size, y.size + n_basin
  c1, c2, c3 = (r[key][:, None] for key in ("c1", "c2", "c3"))
  c1, c2, c3, lb, ln = c1[ny:t0], c2[ny:t0], c3[t0 + n_trans:], r["lbasin"], r["lnorth"]
  bb = (k["A_Atl"] * k["b_Atl"] + k["A_Pac"] * k["b_Pac"]) / (k["A_Atl"] + k["A_Pac"])
  soA, soP, am, zo = k["Psi_SO_Atl"], k["Psi_SO_Pac"], k["Psi_AMOC"], k["Psi_ZOC"]
  iA, iP = itp(bb, k["b_Atl"], soA), itp(bb, k["b_Pac"], soP)
  PsiSO, Ab, Zb = iA + iP, itp(bb, k["bgrid_AMOC"], k["psib_AMOC"]), itp(bb, k["bgrid_ZOC"], k["psib_ZOC"])
  zero, south = np.zeros((1, bb.size)), k["bsouth"][1:]
  nan = np.full((n_trans + n_north, bb.size), np.nan)
  chan_z = np.array([itp(row, bb, soA + soP) for row in south])
  chan_b = np.where(bb < k["bs_SO"][1:, None], PsiSO, 0.)
  chan_r = np.array([itp(row, bb, PsiSO) for row in south])
  tops = np.concatenate((k["btrans"][:, -1:], np.full((n_north, 1), k["bn"][-1])))
  north_z = np.concatenate((np.tile(am, (n_trans, 1)), (c3 * am) / ln))
  north_b = np.where(bb < tops, np.concatenate((np.tile(Ab, (n_trans, 1)), (c3 * Ab) / ln)), 0.)
  north_r = np.concatenate(([itp(row, k["bgrid_AMOC"], k["psib_AMOC"]) for row in k["btrans"]],
                            (c3 * k["psibz_AMOC2"]) / ln))
  cat = lambda *parts: np.concatenate(parts)  # noqa: E731
  return {
      "psiarray_z": cat(zero, chan_z, (c1 * am + c2 * (soA + soP)) / lb, north_z),
      "psiarray_z_Atl": cat(zero, chan_z, (c1 * am + c2 * (soA - zo)) / lb, north_z),
      "psiarray_z_Pac": cat(zero, chan_z, (c2 * (soP + zo)) / lb, nan),
      "psiarray_b": cat(zero, chan_b, (c1 * Ab + c2 * PsiSO) / lb, north_b),
      "psiarray_b_Atl": cat(zero, chan_b, (c1 * Ab + c2 * (iA - Zb)) / lb, north_b),
      "psiarray_b_Pac": cat(zero, chan_b, (c2 * (iP + Zb)) / lb, nan),
      "psiarray_Atl": cat(zero, chan_r, (c1 * k["psibz_AMOC1"] + c2 * (soA - k["psibz_ZOC1"])) / lb, north_r),
      "psiarray_Pac": cat(zero, chan_r, (c2 * (soP + k["psibz_ZOC2"])) / lb, nan)}


def timed(fn, stream, reps):
  """Median and spread (ms) of `reps` hipEvent-timed calls, after two warm-up calls."""
  fn()
  fn()
  pymoc_amd.synchronize()
  ts = []
  for _ in range(reps):
    e0, e1 = pymoc_amd.Event(), pymoc_amd.Event()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.sync()
    ts.append(e0.elapsed_ms(e1))
  ts.sort()
  return ts[len(ts) // 2], ts[0], ts[-1]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=64)
  ap.add_argument("--steps", type=int, default=121)
  ap.add_argument("--time", action="store_true",
                  help="2048 members (unless given): hipEvent time of the preparation launch, of the "
                       "kernel alone (storing all eleven arrays / extrema only) and of the whole "
                       "compute(), next to the host time of the same fields for one member")
  ap.add_argument("--reps", type=int, default=20)
  args = ap.parse_args()
  if args.time and "--members" not in sys.argv:
    args.members = 2048
  pymoc_amd._lib.require_device()
  cfg = configs.config_twobasin(N=args.members)
  ens = pymoc_amd.TwoBasinEnsemble(cfg)
  M = int(cfg["MOC_up_iters"])
  steps = max(args.steps - (args.steps - 1) % M, 1)  # end right after an update, as the script's fields do
  ens.run(steps)
  y, z, nz, n = cfg["y"], cfg["z"], cfg["z"].size, args.members
  TBO = pymoc_amd.TwoBasinOverturningSections
  ovt = TBO.from_ensemble(ens, cfg, store=STORE).compute()
  ext, status = ovt.extrema(), ovt.status()
  ok = np.flatnonzero(status == 0)
  print("%d members, %d steps: eight fields and three buoyancy sections %s per member; %d members "
        "flagged (%d with a failing section point)"
        % (n, steps, ovt.psiarray_z.shape[1:], int((status != 0).sum()), int((status & 1 != 0).sum())))
  print("strongest cells [Sv] at (y km, z m):  member  residual Atlantic max        residual Pacific min"
        "         depth-space global max")
  where = lambda i: (ovt.ynew[i // nz], z[i % nz])  # noqa: E731
  for m in ok[:8]:
    cells = []
    for col, key in ((6, "max"), (7, "min"), (0, "max")):
      cells.append("%8.3f at (%7.0f, %6.0f)" % ((ext[key][m, col],) + where(ext["arg" + key][m, col])))
    print("  %42d  %s  %s  %s" % ((m,) + tuple(cells)))
  # one member against the explicit route fed with the downloaded rows, and against NumPy
  m = int(ok[0])
  dl = lambda a: a.download(stream=ens.stream)  # noqa: E731
  b = dl(ens.cols.b)
  rows = dict(b_Atl=b[:n], b_Pac=b[2 * n:], A_Atl=cfg["A_Atl"], A_Pac=cfg["A_Pac"], bs_SO=dl(ens.bs_SO),
              Psi_SO_Atl=dl(ovt.so_atl.Psi), Psi_SO_Pac=dl(ovt.so_pac.Psi), Psi_AMOC=dl(ovt.amoc.Psi),
              Psi_ZOC=dl(ovt.zoc.Psi), psibz_AMOC1=dl(ovt.amoc.psibz)[:n], psibz_AMOC2=dl(ovt.amoc.psibz)[n:],
              psibz_ZOC1=dl(ovt.zoc.psibz)[:n], psibz_ZOC2=dl(ovt.zoc.psibz)[n:],
              bgrid_AMOC=dl(ovt.amoc.bgrid), psib_AMOC=dl(ovt.amoc.psib), bgrid_ZOC=dl(ovt.zoc.bgrid),
              psib_ZOC=dl(ovt.zoc.psib), bsouth=dl(ovt.channel.out), btrans=dl(ovt.trans.out), bn=dl(ovt.bn))
  one = TBO(y, z, int(cfg["nb"]), store=STORE, **{k: v[m:m + 1] for k, v in rows.items()}).compute()
  got = {name: ovt.download(name)[m] for name in STORE}
  same = all(np.array_equal(got[name], one.download(name)[0], equal_nan=True) for name in STORE)
  print("member %d equals the explicit route on the downloaded rows: %s" % (m, same))
  a = {k: v[m] for k, v in rows.items()}
  t0 = time.perf_counter()
  host = host_fields(y, a)
  t_host = time.perf_counter() - t0
  same_host = all(np.array_equal(got[name], host[name], equal_nan=True) for name in FIELDS)
  print("member %d equals NumPy on the host: %s" % (m, same_host))
  if not (same and same_host):
    sys.exit(1)
  if args.time:
    st, nrows = ens.stream, ovt.nrows
    dev = {k: pymoc_amd.DeviceArray.from_host(np.ascontiguousarray(v)) for k, v in rows.items()}
    alone = TBO(y, z, int(cfg["nb"]), n=n, stream=st, store=STORE, **dev)
    lean = TBO(y, z, int(cfg["nb"]), n=n, stream=st, store=(), **dict(alone.inputs))
    t_prep = timed(lambda: TBO.profiles(ovt.inputs["b_Atl"], ovt.inputs["b_Pac"], (ens.cols.b, n * nz, nz),
                                        ovt.inputs["A_Atl"], ovt.inputs["A_Pac"], n, nz, ovt.b_basin,
                                        ovt.bn, stream=st), st, args.reps)
    t_store = timed(alone.launch, st, args.reps)
    t_lean = timed(lean.launch, st, args.reps)
    t_all = timed(ovt.compute, st, args.reps)
    stored = n * 8 * len(STORE) * nrows * nz
    print("time (median [min, max] of %d, ms): %d members, %d x %d points each\n"
          "  preparation (b_basin, bn)              %.3f [%.3f, %.3f]\n"
          "  kernel alone, all eleven arrays stored %.3f [%.3f, %.3f]  %.2f GB stored, %.2f TB/s of stores\n"
          "  kernel alone, extrema only             %.3f [%.3f, %.3f]\n"
          "  compute(): preparation + sections + solves + kernel  %.3f [%.3f, %.3f]  (%.2f us per member)\n"
          "  host, the same eight fields of ONE member in NumPy (sections and solves given): %.2f ms"
          % ((args.reps, n, nrows, nz) + t_prep + t_store + (stored / 1e9, stored / t_store[0] / 1e9) +
             t_lean + t_all + (1e3 * t_all[0] / n, 1e3 * t_host)))


if __name__ == "__main__":
  main()
