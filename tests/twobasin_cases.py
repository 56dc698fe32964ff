"""Shapes of the two-basin driver's edge tests (helper module, no tests): tests/test_twobasin_gpu.py
runs them on the device, tests/test_twobasin_cpu.py checks that the oracle stays finite."""
import functools

import numpy as np

from pymoc_amd import configs

DAY = 86400.0
# (nz, ny, dt in days): the time steps keep kappa dt / dz^2 where nz = 80 at 30 days has it.
# nz > 256: the driver issues separate Psi_SO and thermal-wind launches and the columns hold more
# than four levels per lane
SHAPES = ((17, 9, 30), (46, 51, 30), (81, 33, 30), (129, 51, 11), (200, 51, 4), (300, 65, 2))
N = 10
M = 24  # MOC_up_iters of the config
# launches of 1-2 steps take the forcing as an array, longer ones form it in the column kernel: the
# splits make the two alternate, stop on both sides of an update and cross one
SPLITS = (1, M - 1, 1, 2, 3, M - 2)
SNAPS = (1, M + 1, 2 * M + 4)  # steps at which members are compared with the oracle
MEMBERS = (0, 5)
assert set(SNAPS) <= set(np.cumsum(SPLITS)) and sum(SPLITS) == SNAPS[-1]


def label(shape):
  return "nz%d-ny%d-dt%dd" % shape


def cfg(shape):
  nz, ny, days = shape
  c = configs.config_twobasin(N=N, nz=nz, ny=ny)
  assert c["MOC_up_iters"] == M
  return dict(c, dt=DAY * days)


@functools.lru_cache(maxsize=None)
def oracle_snaps(shape, m):
  """{step: fields} of member m by the CPU oracle's driver at SNAPS."""
  from oracle import drivers
  return drivers.run_twobasin(configs.member(cfg(shape), m, 6), SNAPS[-1], set(SNAPS))
