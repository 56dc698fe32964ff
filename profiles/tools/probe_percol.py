#!/usr/bin/env python3
"""usage: [PYMOC_HIP_LIB=other/libpymoc_hip.so] probe_percol.py OUT.txt [STRIDE=1]
Which columns of config 2 are the slow waves?  A launch of one wave per column lasts as long as its
slowest wave, and the averaged counters do not say which that is.  Every STRIDE-th column of
config 2 (1024 columns, nz = 100) is run on its own: 64 copies of it in one batch, 5 launches of
1000 steps to warm up, 5 timed between two events.  Writes "column  us-per-launch  do_conv" lines
(profiles/r08/percol_*.txt).  With 64 waves on the device a launch is ~15 % shorter than the same
column's wave in the full batch; the comparison is between columns and between builds."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import pymoc_amd
from pymoc_amd import configs
from pymoc_amd.device import DeviceArray, Event, Stream

N, REP = 1024, 64
cfg = configs.config2(N=N)
stream = Stream()
stride = int(sys.argv[2]) if len(sys.argv) > 2 else 1


def rep(a, j):
  a = np.asarray(a)
  if a.ndim >= 1 and a.shape[0] == N:
    return np.repeat(a[j:j + 1], REP, axis=0)
  return a


out = open(sys.argv[1], "w")
for j in range(0, N, stride):
  batch = pymoc_amd.ColumnBatch(cfg["z"], rep(cfg["kappa"], j), rep(cfg["Area"], j), rep(cfg["b0"], j),
                                bs=rep(cfg["bs"], j), bbot=rep(cfg["bbot"], j), N2min=rep(cfg["N2min"], j),
                                do_conv=rep(cfg["do_conv"], j), stream=stream)
  wA = DeviceArray.from_host(rep(cfg["wA"], j), stream=stream)
  for _ in range(5):
    batch.steps(wA, cfg["dt"], 1000)
  e0, e1 = Event(), Event()
  e0.record(stream)
  for _ in range(5):
    batch.steps(wA, cfg["dt"], 1000)
  e1.record(stream)
  stream.sync()
  us = e0.elapsed_ms(e1) * 1e3 / 5
  out.write("%d %.2f %d\n" % (j, us, int(np.asarray(cfg["do_conv"])[j])))
  out.flush()
out.close()
