#!/usr/bin/env python3
"""The overturning streamfunction sections of Plot_overturning.py (PyMOC's figure script) -- the
depth-space, isopycnal and residual overturning it plots, :73-92 -- for EVERY member of a Jansen &
Nadeau (2018) ensemble, built on the GPU from the ensemble's device state, and each member's
strongest cells.

The ensemble is time-stepped (JN2018Ensemble); OverturningSections.from_ensemble then reads its
rows in place: two SectionBatch launches (the buoyancy sections), a thermal-wind and a
Southern-Ocean solve into private buffers, and one launch of the overturning kernel -- no round
trip through the host, and the ensemble's own diagnostics stay untouched.

    python examples/overturning_streamfunctions.py --members 64 --steps 360
    python examples/overturning_streamfunctions.py --time     # 4096 members, nz = 200, hipEvent timing
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.overturning import section_rows


def host_fields(y, b_basin, bs_SO, Psi, Psi_SO, bgrid, psib, psibz1, bsouth, bnorth):
  """One member's three fields in NumPy on the host (what the device computes, row block by row
  block): -> psi_z, psi_b, psi_res [nrows][nz]."""
  r = section_rows(y)
  ny, nn = y.size, bnorth.shape[0]
  c1, c2, c3 = (r[k][:, None] for k in ("c1", "c2", "c3"))
  chan = np.array([np.interp(row, b_basin, Psi_SO) for row in bsouth[1:]])
  blend_b = (c1[ny:-nn] * psibz1 + c2[ny:-nn] * Psi_SO) / r["lbasin"]
  blend_z = (c1[ny:-nn] * Psi + c2[ny:-nn] * Psi_SO) / r["lbasin"]
  top = np.zeros((1, b_basin.size))
  psi_res = np.concatenate((top, chan, blend_b, [np.interp(row, bgrid, psib) for row in bnorth]))
  psi_res[-1] = 0.
  psi_z = np.concatenate((top, chan, blend_z, (c3[-nn:] * Psi) / r["lnorth"]))
  psi_b = np.concatenate((top, np.where(b_basin < bs_SO[1:, None], Psi_SO, 0.), blend_b,
                          np.where(b_basin < bnorth[:, -1:], psibz1, 0.)))
  return psi_z, psi_b, psi_res


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
  ap.add_argument("--steps", type=int, default=360)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--time", action="store_true",
                  help="4096 members at nz = 200 (unless given): hipEvent time of the kernel alone "
                       "(storing the three fields / extrema only) and of the whole compute(), "
                       "next to the host time of the same fields for one member")
  ap.add_argument("--reps", type=int, default=20)
  args = ap.parse_args()
  if args.time:
    if "--members" not in sys.argv:
      args.members = 4096
    if "--nz" not in sys.argv:
      args.nz, args.dt_days, args.steps = 200, 10., 72
  pymoc_amd._lib.require_device()
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  cfg["rest_mask"] = np.repeat(cfg["rest_mask"][None], args.members, axis=0)
  ens = pymoc_amd.JN2018Ensemble(cfg)
  steps = args.steps - args.steps % cfg["MOC_up_iters"]
  ens.run(steps)
  y, z, nz = cfg["y"], cfg["z"], args.nz
  ovt = pymoc_amd.OverturningSections.from_ensemble(ens, cfg).compute()
  ext, status = ovt.extrema(), ovt.status()
  ok = np.flatnonzero(status == 0)
  print("%d members, %d steps: three fields %s per member; %d members flagged (%d with a failing "
        "section point, %d with a non-monotone or non-finite basin profile)"
        % (args.members, steps, ovt.psi_res.shape[1:], int((status != 0).sum()),
           int((status & 1 != 0).sum()), int((status & 2 != 0).sum())))
  print("residual overturning, strongest cells:  member  max [Sv] at (y km, z m)   min [Sv] at (y km, z m)")
  for m in ok[:8]:
    imax, imin = ext["argmax"][m, 2], ext["argmin"][m, 2]
    print("  %38d  %8.3f at (%7.0f, %6.0f)  %8.3f at (%7.0f, %6.0f)"
          % (m, ext["max"][m, 2], ovt.ynew[imax // nz], z[imax % nz],
             ext["min"][m, 2], ovt.ynew[imin // nz], z[imin % nz]))
  # one member against the explicit route fed with the downloaded rows, and against NumPy
  m = int(ok[0])
  dl = lambda a: a.download(stream=ens.stream)
  st = ens.state()
  rows = dict(b_basin=st["b_basin"], bs_SO=st["bs_SO"], Psi=dl(ovt.tw.Psi), Psi_SO=dl(ovt.so.Psi),
              bgrid=dl(ovt.tw.bgrid), psib=dl(ovt.tw.psib), psibz=dl(ovt.tw.psibz1),
              bsouth=dl(ovt.channel.out), bnorth=dl(ovt.north.out))
  one = pymoc_amd.OverturningSections(y, z, int(cfg["nb"]),
                                      **{k: v[m:m + 1] for k, v in rows.items()}).compute()
  got = [dl(a)[m] for a in (ovt.psi_z, ovt.psi_b, ovt.psi_res)]
  same = all(np.array_equal(g, a.download()[0]) for g, a in zip(got, (one.psi_z, one.psi_b, one.psi_res)))
  print("member %d equals the explicit route on the downloaded rows: %s" % (m, same))
  a = {k: v[m] for k, v in rows.items()}
  t0 = time.perf_counter()
  host = host_fields(y, a["b_basin"], a["bs_SO"], a["Psi"], a["Psi_SO"], a["bgrid"], a["psib"],
                     a["psibz"], a["bsouth"], a["bnorth"])
  t_host = time.perf_counter() - t0
  same_host = all(np.array_equal(g, h) for g, h in zip(got, host))
  print("member %d equals NumPy on the host: %s" % (m, same_host))
  if not (same and same_host):
    sys.exit(1)
  if args.time:
    n, nrows = args.members, ovt.nrows
    alone = pymoc_amd.OverturningSections(y, z, int(cfg["nb"]), n=n, stream=ens.stream,
                                          **{k: pymoc_amd.DeviceArray.from_host(v) for k, v in rows.items()})
    lean = pymoc_amd.OverturningSections(y, z, int(cfg["nb"]), n=n, stream=ens.stream, store=(),
                                         **alone_inputs(alone))
    t_store = timed(alone.launch, ens.stream, args.reps)
    t_lean = timed(lean.launch, ens.stream, args.reps)
    t_all = timed(ovt.compute, ens.stream, args.reps)
    # what the storing launch moves: the two buoyancy sections and the profile rows in, three
    # fields out
    nb, ny = int(cfg["nb"]), y.size
    moved = n * 8 * ((ny + ovt.n_north) * nz + 4 * nz + ny + 2 * nb + 3 * nrows * nz)
    print("time (median [min, max] of %d, ms): %d members, %d x %d points each\n"
          "  kernel alone, three fields stored  %.3f [%.3f, %.3f]  %.1f MB moved, %.2f TB/s\n"
          "  kernel alone, extrema only         %.3f [%.3f, %.3f]\n"
          "  compute(): sections + solves + kernel  %.3f [%.3f, %.3f]  (%.2f us per member)\n"
          "  host, the same three fields of ONE member in NumPy (sections and solves given): %.2f ms"
          % ((args.reps, n, nrows, nz) + t_store + (moved / 1e6, moved / t_store[0] / 1e9) + t_lean +
             t_all + (1e3 * t_all[0] / n, 1e3 * t_host)))


def alone_inputs(o):
  """The device rows of an OverturningSections, to build another one on the same memory."""
  return {name: o.inputs[name] for name in o.inputs}


if __name__ == "__main__":
  main()
