#!/usr/bin/env python3
"""The 2-D buoyancy sections of Plot_overturning.py (PyMOC's figure script) for EVERY member of a
Jansen & Nadeau (2018) ensemble, built on the GPU from the ensemble's device state.

The ensemble is time-stepped (JN2018Ensemble), then two SectionBatch launches read its rows in
place -- no round trip through the host -- with the script's fix-ups (fixups='plot_overturning',
Plot_overturning.py:42-50 and :63-64):
  channel: Interpolate_channel(y, z, bs=bs_SO, bn=b_basin).gridit()          (:53)
  north:   Interpolate_twocol(ynorth, z, bs=b_basin, bn=b_north).gridit()    (:67)

    python examples/overturning_sections.py --members 64 --steps 360
    python examples/overturning_sections.py --time        # 4096 members, hipEvent timing
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol


def sections(ens, y, z, fixups="plot_overturning"):
  """The channel and northern SectionBatch of an ensemble, reading its device rows in place."""
  n, nz = ens.n, ens.nz
  # Plot_overturning.py:58-66: ynorth in km, the interpolator's y from 0
  ynorth = np.linspace(1000. / 10., 1000., 10) + y[-1] / 1e3 + 12000.
  channel = pymoc_amd.SectionBatch("channel", y, z, bs=ens.ml.bs, bn=ens.cols.b, n=n,
                                   fixups=fixups, stream=ens.stream)
  north = pymoc_amd.SectionBatch("twocol", ynorth * 1000. - ynorth[0] * 1000., z, bs=ens.cols.b,
                                 bn=ens.cols.b, bn_offset=n * nz, n=n, fixups=fixups,
                                 stream=ens.stream)
  return channel, north


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--members", type=int, default=64)
  ap.add_argument("--steps", type=int, default=360)
  ap.add_argument("--nz", type=int, default=81)
  ap.add_argument("--dt-days", type=float, default=30.)
  ap.add_argument("--time", action="store_true",
                  help="4096 members (unless --members is given); hipEvent time of the two "
                       "section launches next to the host time of the reference's algorithm")
  ap.add_argument("--reps", type=int, default=5)
  args = ap.parse_args()
  if args.time and "--members" not in sys.argv:
    args.members = 4096
  pymoc_amd._lib.require_device()
  cfg = configs.config5(N=args.members, nz=args.nz, dt_days=args.dt_days)
  cfg["rest_mask"] = np.repeat(cfg["rest_mask"][None], args.members, axis=0)
  ens = pymoc_amd.JN2018Ensemble(cfg)
  steps = args.steps - args.steps % cfg["MOC_up_iters"]
  ens.run(steps)
  y, z = cfg["y"], cfg["z"]
  channel, north = sections(ens, y, z)
  bsouth = channel.grid()
  bnorth = north.grid()
  pymoc_amd.synchronize()
  bad = set(ens.nonfinite_members().tolist())
  fail_c, fail_n = channel.failed_points(), north.failed_points()
  ok = [m for m in range(args.members) if m not in bad]
  print("%d members, %d steps: channel %s and north %s sections; %d non-finite members, "
        "%d / %d finite members with a failing point (channel / north)"
        % (args.members, steps, bsouth.shape[1:], bnorth.shape[1:], len(bad),
           int((fail_c[ok] >= 0).sum()), int((fail_n[ok] >= 0).sum())))
  # member 0 against the drop-in classes on the downloaded state (the script's own calls)
  st = ens.state()
  m = ok[0]
  bs, bn = st["bs_SO"][m].copy(), st["b_basin"][m].copy()
  if bs[0] > bs[1]:
    bs[0] = bs[1]
  if bs[0] < bn[0]:
    bn[0] = bs[0]
  ref_c = Interpolate_channel(y=y, z=z, bs=bs, bn=bn).gridit()
  got_c = bsouth.download()[m]
  bnn = st["b_north"][m].copy()
  bnn[0] = st["b_basin"][m][0]
  ynorth = np.linspace(100., 1000., 10) + y[-1] / 1e3 + 12000.
  yn = ynorth * 1000. - ynorth[0] * 1000.
  ref_n = Interpolate_twocol(y=yn, z=z, bs=st["b_basin"][m], bn=bnn).gridit()
  got_n = bnorth.download()[m]
  same = np.array_equal(got_c, ref_c) and np.array_equal(got_n, ref_n)
  print("member %d equals the drop-in classes on the downloaded state: %s" % (m, same))
  if not same:
    sys.exit(1)
  if args.time:
    ev = [pymoc_amd.Event() for _ in range(3)]
    channel.grid()
    north.grid()
    pymoc_amd.synchronize()
    tc = tn = 0.
    for _ in range(args.reps):
      ev[0].record(ens.stream)
      channel.grid()
      ev[1].record(ens.stream)
      north.grid()
      ev[2].record(ens.stream)
      ev[2].sync()
      tc += ev[0].elapsed_ms(ev[1]) / args.reps
      tn += ev[1].elapsed_ms(ev[2]) / args.reps
    # the reference's algorithm on the host (pymoc_amd.utils.brenth + np.interp), one member
    from pymoc_amd.utils import gridit
    ic = Interpolate_channel(y=y, z=z, bs=bs, bn=bn)
    it = Interpolate_twocol(y=yn, z=z, bs=st["b_basin"][m], bn=bnn)
    t0 = time.perf_counter()
    gridit(ic.y, ic.z, ic._host_call)
    t1 = time.perf_counter()
    gridit(it.y, it.z, it._host_call)
    t2 = time.perf_counter()
    print("time: %d members, channel %s + north %s: %.2f + %.2f ms on the device "
          "(%.2f us per member); host, one member with the reference's algorithm: "
          "%.3f + %.3f s" % (args.members, bsouth.shape[1:], bnorth.shape[1:], tc, tn,
                             1e3 * (tc + tn) / args.members, t1 - t0, t2 - t1))


if __name__ == "__main__":
  main()
