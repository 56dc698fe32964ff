"""Columns for the super-block tier of the column twin kernel (csrc/column.hip.h: conv_spec_run,
its ROLLED tier -- in entries with at least 256 steps to go a speculative block is 64 steps, the
16-fold body rolled four times, begun and checked once) -- helper module, no tests, no device code.

A case is one batch of 8 columns (MEMBERS) at one nz, one Area and one JOIN STEP.  The launches
that tests/test_column_superblock_gpu.py runs do step 0 on their own, so their super-blocks are
the steps 1 ... 64, 65 ... 128, ...; the join steps lie in the second one: its first step, one step
in each of its four 16-step quarters, its last step.  A join there makes the kernel redo 64 steps
and report the end of that super-block, step 129, to its dispatch.

The joining columns are built, not searched.  The column is flat at bs - eps under a convecting
surface that holds its adjusted value adj, and the diffusivity is R dz^2 / dt at every level, so the
time scale does not depend on nz.  While the surface alone convects the step is affine in the
state: level nz - 2 stands at (bs - eps) + (adj - bs + eps) g(k) after k steps, with g the response
of that level to a unit step at the surface -- read from ONE run of the oracle with a large eps.  The
level first exceeds bs at the convect of step k for eps between A g(k-1)/(1 - g(k-1)) and
A g(k)/(1 - g(k)), A = adj - bs; the column takes the middle.  bs has a low dword of 16, so only
values within 16 ulps below bs share its high dword: the integer filter's alarm and the join are
the same step.  tests/test_column_superblock_gpu.py asserts all of this on the oracle's single
steps before anything runs on the device."""
import functools

import numpy as np

import column_cls_churn_cases as T

DT = T.DT
AREAS = T.AREAS                      # (at nz = 100: form 8, form 7)
NZS = (6, 7, 65, 66, 99, 100)        # P = 1 even / odd; P = 2 odd / even (IF = 1 / IF = 2) twice
# one launch each: 254, 255, 256, 318, 319 and 338 steps behind step 0 -- no super-block; exactly
# four; four and a rest that ends in the tiers of 4 and 1; 16, 4 and 1; five and 16, 1
LAUNCHES = (255, 256, 257, 319, 320, 339)
BLOCK = 64
SECOND = 1 + BLOCK                   # first step of the second super-block
JOIN_STEPS = {"first": SECOND, "q1": SECOND + 8, "q2": SECOND + 24, "q3": SECOND + 40,
              "q4": SECOND + 56, "last": SECOND + BLOCK - 1}
R = 0.01                             # kappa dt / dz^2 of the joining columns
ABOVE = 1e-4                         # N2min dz of the joining columns
BS, BBOT, N2MIN = 0.025, -0.003, 1e-7
MEMBERS = ("quiet", "surface", "join", "join bs<0", "false alarm", "ieee", "all", "quiet bs<0")
JOINING = (2, 3)                     # rows of MEMBERS


def _bs_low16(x):
  """x with the low dword of its pattern set to 16."""
  bits = np.array([x], dtype=np.float64).view(np.uint64)
  bits[0] = (bits[0] & np.uint64(0xffffffff00000000)) | np.uint64(16)
  return float(bits.view(np.float64)[0])


BS_JOIN = {"join": _bs_low16(BS), "join bs<0": -0.001}


def _grid(nz):
  return np.linspace(-4000., 0., nz)


def _kappa(z):
  return 2e-5 + 2e-4 * np.exp(-z / 1000 - 4)


def _base(z, bs=BS, bbot=BBOT):
  """config 2's initial profile, strictly below bs in the interior"""
  return (bs - bbot) * np.exp(z / 300.) + bbot


def _batch(z, area, rows):
  """rows: dicts with b0, bs, bbot, N2min, kappa, w0 -> the arrays T.steps takes."""
  n, nz = len(rows), z.size
  return dict(z=z, kappa=np.stack([r["kappa"] for r in rows]), area=np.full((n, nz), area),
              b0=np.stack([r["b0"] for r in rows]), bs=np.array([r["bs"] for r in rows]),
              bbot=np.array([r["bbot"] for r in rows]), N2min=np.array([r["N2min"] for r in rows]),
              wA=np.stack([area * r["w0"] * np.sin(np.pi * z / 4000.) for r in rows]))


def _join_row(z, bs, eps):
  nz, dz = z.size, z[1] - z[0]
  b0 = np.full(nz, bs - eps)
  b0[-1] = bs + 0.01
  return dict(b0=b0, bs=bs, bbot=bs - eps, N2min=ABOVE / dz, kappa=np.full(nz, R * dz * dz / DT), w0=-3e-8)


@functools.lru_cache(maxsize=None)
def _response(nz, area, bs):
  """(A, g): the surface's adjusted value less bs, and g[k], the rise of level nz - 2 after k
  steps as a fraction of the step between the flat column and the surface (one oracle run)."""
  z = _grid(nz)
  eps0 = 100 * ABOVE  # far below bs: level nz - 2 does not get there in these steps
  c = _batch(z, area, [_join_row(z, bs, eps0)])
  last = max(JOIN_STEPS.values())
  g, b = [0.0], c["b0"]
  for k in range(1, last + 1):
    b = T.steps(c, 1, b)
    assert not (b[0, :-1] > bs).any(), (nz, k)
    if k == 1:
      A = b[0, -1] - bs
      assert A > 0
    assert b[0, -1] - bs == A
    g.append((b[0, -2] - (bs - eps0)) / (A + eps0))
  g = np.array(g)
  assert (np.diff(g[1:]) > 0).all() and g[-1] < 0.75
  return float(A), g


def join_row(nz, area, kind, step):
  """The joining column of `kind` ("join", "join bs<0") whose level nz - 2 first exceeds bs at the
  convect of step `step`."""
  bs = BS_JOIN[kind]
  A, g = _response(nz, area, bs)
  e0, e1 = (A * g[k] / (1 - g[k]) for k in (step - 1, step))
  return _join_row(_grid(nz), bs, 0.5 * (e0 + e1))


@functools.lru_cache(maxsize=None)
def case(nz, area, where):
  """Inputs of the batch with the join at JOIN_STEPS[where], and the oracle's states after every
  launch length; computed once, shared, read-only."""
  z = _grid(nz)
  step = JOIN_STEPS[where]
  quiet = dict(b0=_base(z), bs=BS, bbot=BBOT, N2min=N2MIN, kappa=_kappa(z), w0=1e-8)
  surf = dict(quiet, b0=_base(z))
  surf["b0"][-1] = BS + 0.01
  near = BS * (1 - 2.0**-22)  # in bs's 2^-20 bucket, below bs
  flat = np.full(nz, near)
  flat[-1] = BS
  alarm = dict(quiet, b0=flat, bbot=near, w0=0.0)
  s = 2.0**-1000  # outside the exact-division window: the wave steps in the IEEE form
  ieee = dict(surf, b0=surf["b0"] * s, bs=BS * s, bbot=BBOT * s, N2min=N2MIN * s)
  hot = dict(quiet, b0=BS + 0.01 + 1e-3 * np.linspace(0., 1., nz))
  cold = dict(quiet, b0=_base(z, -0.001, BBOT), bs=-0.001)
  rows = [quiet, surf, join_row(nz, area, "join", step), join_row(nz, area, "join bs<0", step), alarm,
          ieee, hot, cold]
  assert len(rows) == len(MEMBERS) <= 8
  c = _batch(z, area, rows)
  c["step"] = step
  c["ref"] = {n: T.steps(c, n) for n in LAUNCHES}
  for v in list(c.values()) + list(c["ref"].values()):
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return c


def convecting(c, nsteps):
  """Per step k < nsteps and column: the set of levels with b > bs at the convect of step k (the
  oracle's single steps), and whether a level below the surface shares bs's high dword or lies above
  it without convecting (what the integer filter takes for an alarm)."""
  sets, near = [], []
  b = c["b0"]
  bs = c["bs"]
  for _ in range(nsteps):
    with np.errstate(invalid="ignore"):
      conv = b > bs[:, None]
      hit = (b[:, :-1] > 0) & (T._hi32(b[:, :-1]) >= T._hi32(bs)[:, None]) & ~conv[:, :-1]
    sets.append([frozenset(np.nonzero(row)[0].tolist()) for row in conv])
    near.append(hit.any(axis=1))
    b = T.steps(c, 1, b)
  return sets, np.array(near)
