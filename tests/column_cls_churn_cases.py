"""Random near-surface columns whose convecting pattern enters and leaves the class loops of the
column twin kernel (csrc/column.hip.h: conv_class, conv_spec_run, k_column_steps_cls) many times
per launch -- generator, classification of the oracle's single steps, coverage accounting (helper
module, no tests, no device code).

tests/test_column_conv_classes_gpu.py builds columns with ONE event each, always in block 2 of the
16-step tier.  Here the top 2 ... 6 interior levels of a column get a diffusivity near the explicit
scheme's bound, so they oscillate about bs: a column goes surface-only -> joined -> surface-only,
or nothing -> interior -> nothing, over and over, in every tier and after every re-dispatch.  A
planted group sits flat in bs's 2^-20 bucket (false alarms of the integer filter), another creeps
across bs inside that bucket (a true alarm at equal high dwords), and the whole batch exists
again scaled by 2^-150 and 2^150 (the filter compares exponents).

tests/test_column_cls_churn_cpu.py asserts on the oracle alone that these inputs hold the events;
tests/test_column_cls_churn_gpu.py runs them on the device.
"""
import functools

import numpy as np

import oracle as O

DAY = 86400.
DT = 30 * DAY
AREA_PROVEN = 8e13                  # (the 2-instruction proof accepts it)
AREA_REJECTED = 138681915977248.73  # (the 2-instruction proof rejects it: the Area leg takes 3)
AREAS = (AREA_PROVEN, AREA_REJECTED)
# P = 1; P = 1 full wave; P = 2 odd and even; nz = 100; the surface in the last lane (127: alone
# with padding, 128: with level 126); 65: the surface as first level of lane 32
NZS = (9, 64, 65, 66, 100, 127, 128)
N = 96
N_BUCKET = 16
N_CREEP = 8
TOTAL = 140
# launches of one run; the last one is the control: the same columns on k_column_steps
SPLITS = ((64,), (65,), (79,), (140,), (70, 70), (64, 64, 12), (100, 40), (63, 63, 14))
CONTROL = (63, 63, 14)
SCALES = (-150, 150)

NOTHING, SURFACE, JOINED, INTERIOR = 0, 1, 2, 3
CLASS_NAMES = ("nothing", "surface-only", "surface+others", "others")
KINDS = {"surf->joined": (SURFACE, JOINED), "joined->surf": (JOINED, SURFACE),
         "nothing->interior": (NOTHING, INTERIOR), "interior->nothing": (INTERIOR, NOTHING)}


def gen(nz, n, seed, area):
  """n columns of nz levels; the last N_BUCKET of them are the planted bucket group, the N_CREEP
  before them the creeping group."""
  rng = np.random.default_rng(seed)
  z = np.linspace(-4000., 0., nz)
  dz = z[1] - z[0]
  kappa = (2e-5 + 2e-4 * np.exp(-z / 1000 - 4))[None, :] * (1 + 0.3 * rng.random((n, nz)))
  u = rng.random(n)
  bs = np.where(u < 0.75, rng.uniform(0.005, 0.03, n),
                np.where(u < 0.87, 0.0, -rng.uniform(0.001, 0.01, n)))
  kind = np.where(u < 0.75, "bs>0", np.where(u < 0.87, "bs=0", "bs<0")).astype(object)
  neg0 = int(np.nonzero(bs[:n - N_BUCKET - N_CREEP] == 0.0)[0][0])  # one column with bs = -0.0
  bs[neg0] = -0.0
  kind[neg0] = "bs=-0"
  hot_bottom = rng.random(n) < 0.10  # level 0 convects forever; the integer filter is invalid
  bbot = np.where(hot_bottom, bs + 0.005, bs - rng.uniform(0.005, 0.03, n))
  N2min = np.where(rng.random(n) < 0.15, 0.0, 10**rng.uniform(-7, -5, n))
  b0 = (bs - bbot)[:, None] * np.exp(z / 300.)[None, :] + bbot[:, None]
  amp = 10**rng.uniform(-6, -3, n)
  top = min(7, nz - 2)  # the levels under the surface (not level 0)
  b0[:, nz - 1 - top:nz - 1] = (bs[:, None] - amp[:, None] * 3 * rng.random((n, top)) +
                                amp[:, None] * rng.standard_normal((n, top)))
  b0[:, -1] = np.where(rng.random(n) < 0.70, bs + 0.01, bs)
  for i in range(n):
    k = int(rng.integers(2, min(6, nz - 2) + 1))
    kappa[i, nz - 1 - k:nz - 1] = rng.uniform(0.40, 0.56, k) * dz * dz / DT
  w0 = rng.uniform(-3e-8, 3e-8, n)
  for i in range(n):
    if hot_bottom[i]:
      kind[i] += ",bbot>bs"
    if N2min[i] == 0.0:
      kind[i] += ",N2min=0"
  # the planted bucket group: flat in bs's 2^-20 bucket below bs, where the integer filter alarms
  # and nothing convects
  for j, i in enumerate(range(n - N_BUCKET, n)):
    while True:
      bs[i] = rng.uniform(0.005, 0.03)
      near = bs[i] * (1 - 2.0**-22)
      if _hi32(np.array([near]))[0] == _hi32(np.array([bs[i]]))[0]:
        break
    flat = nz // 2
    b0[i, :flat] = near
    b0[i, flat:] = np.linspace(near, bs[i] * (1 - 1e-3), nz - flat)  # a ramp away from bs
    b0[i, -1] = bs[i] + 0.01 if j % 2 == 0 else bs[i]
    bbot[i] = near
    N2min[i] = 10**rng.uniform(-7, -5)
    kappa[i] = (2e-5 + 2e-4 * np.exp(-z / 1000 - 4)) * (1 + 0.3 * rng.random(nz))
    kind[i] = "bucket"
  # the creeping group: a TRUE alarm at hi32(b) == hi32(bs).  The column is flat in bs's bucket
  # below bs under a convecting surface whose adjusted value bs + N2min dz lies in the same bucket
  # above bs, so level nz - 2 diffuses up across bs and joins without leaving the bucket.
  creep = np.arange(n - N_BUCKET - N_CREEP, n - N_BUCKET)
  for i in creep:
    e = np.floor(np.log2(rng.uniform(0.005, 0.03)))
    width = 2.0**(e - 20)  # of the bucket
    bs[i] = 2.0**e * (1 + int(rng.integers(0, 1 << 20)) / 2.0**20) + 0.3 * width
    near = bs[i] - 0.15 * width
    assert _hi32(np.array([near]))[0] == _hi32(np.array([bs[i]]))[0] and near < bs[i]
    N2min[i] = rng.uniform(0.3, 0.6) * width / dz
    kappa[i] = rng.uniform(0.02, 0.15) * dz * dz / DT
    b0[i] = near
    b0[i, -1] = bs[i] + 0.01
    bbot[i] = near
    kind[i] = "creep"
  wA = area * w0[:, None] * np.sin(np.pi * z / 4000.)[None, :]
  return dict(z=z, kappa=kappa, area=np.full((n, nz), area), b0=b0, bs=bs, bbot=bbot, N2min=N2min,
              wA=wA, kind=[str(k) for k in kind], bucket=np.arange(n - N_BUCKET, n), creep=creep)


def scaled(case, k):
  """The same batch at another exponent: b0, bs, bbot, N2min times 2^k (the step is linear in
  them, so every result is 2^k times the unscaled one, bit for bit)."""
  s = 2.0**k
  out = dict(case)
  for key in ("b0", "bs", "bbot", "N2min"):
    out[key] = case[key] * s
  for key in ("b0", "bs", "bbot", "N2min", "wA", "kappa"):
    a = np.abs(np.asarray(out[key]))
    a = a[a != 0]
    assert a.size == 0 or (a.min() >= 2.0**-200 and a.max() <= 2.0**200), key  # the operand window
  return out


def _hi32(x):
  """High dword of each double, as the signed integer the filter compares."""
  return (np.ascontiguousarray(x, dtype=np.float64).view(np.int64) >> 32).astype(np.int64)


def steps(case, nsteps, b=None):
  n = case["b0"].shape[0]
  with np.errstate(all="ignore"):
    return O.column_ensemble_steps(case["z"], case["kappa"], case["area"],
                                   case["b0"] if b is None else b, case["wA"], DT,
                                   np.ones(n, dtype=np.int32), case["bs"], case["bbot"],
                                   case["N2min"], nsteps)


def trace(case, nsteps, keep=None):
  """The oracle's single steps, classified.  Returns a dict:
  cls [nsteps, n]: what convects at the convect of each step -- NOTHING, SURFACE (level nz - 1
    alone), JOINED (the surface and others), INTERIOR (others without the surface);
  trans: the class changes, as (column, step, class before, class at `step`), by column and step;
  alarm [nsteps, n]: false alarms of the integer filter -- bs > 0, class NOTHING or SURFACE, and a
    level below the surface with b > 0, hi32(b) >= hi32(bs) and not b > bs;
  b: {steps done: state} for the step counts in `keep` (None: all of them)."""
  n, nz = case["b0"].shape
  bs = case["bs"]
  cls = np.zeros((nsteps, n), dtype=np.int8)
  alarm = np.zeros((nsteps, n), dtype=bool)
  snaps = {0: case["b0"]}
  b = case["b0"]
  for s in range(nsteps):
    with np.errstate(invalid="ignore"):
      conv = b > bs[:, None]
      surf, rest = conv[:, -1], conv[:, :-1].any(axis=1)
      cls[s] = np.where(surf, np.where(rest, JOINED, SURFACE), np.where(rest, INTERIOR, NOTHING))
      near = (b[:, :-1] > 0) & (_hi32(b[:, :-1]) >= _hi32(bs)[:, None]) & ~conv[:, :-1]
    alarm[s] = (bs > 0) & ((cls[s] == NOTHING) | (cls[s] == SURFACE)) & near.any(axis=1)
    b = steps(case, 1, b)
    if keep is None or s + 1 in keep:
      snaps[s + 1] = b
  ss, cc = np.nonzero(cls[1:] != cls[:-1])
  trans = sorted((int(c), int(s) + 1, int(cls[s, c]), int(cls[s + 1, c])) for s, c in zip(ss, cc))
  return dict(cls=cls, trans=trans, alarm=alarm, b=snaps)


def count(trans, kind, lo=0, hi=1 << 30):
  a, b = KINDS[kind]
  return sum(1 for (_, s, x, y) in trans if (x, y) == (a, b) and lo <= s < hi)


def named(trans):
  """Only the four named kinds of transition."""
  named_pairs = set(KINDS.values())
  return [t for t in trans if (t[2], t[3]) in named_pairs]


def launch_parts(split):
  """The three parts of each launch of a split, as global step ranges: {"first16": [...],
  "tier4": [...], "tail": [...]} -- the first 16 steps of a launch of L steps, its steps
  L - L % 16 ... L - L % 4 - 1 (the tier of 4), and its last L % 4 steps."""
  parts = {"first16": [], "tier4": [], "tail": []}
  o = 0
  for L in split:
    parts["first16"].append((o, o + min(16, L)))
    parts["tier4"].append((o + L - L % 16, o + L - L % 4))
    parts["tail"].append((o + L - L % 4, o + L))
    o += L
  return parts


def seed(nz, area):
  return 7000 + 10 * nz + AREAS.index(area)


@functools.lru_cache(maxsize=None)
def case(nz, area, scale=0):
  """Inputs, the oracle's trace (scale = 0) and its states after every step count a split ends
  at; computed once, shared, read-only."""
  c = gen(nz, N, seed(nz, area), area)
  totals = sorted(set(sum(s) for s in SPLITS))
  if scale:
    c = scaled(c, scale)
    c["ref"] = {t: steps(c, t) for t in totals}
  else:
    c["trace"] = trace(c, TOTAL, keep=totals)
    c["ref"] = {t: c["trace"]["b"][t] for t in totals}
  for v in list(c.values()) + list(c["ref"].values()):
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return c


def describe(c, col, bad_levels, trans):
  """One failing column for an assertion message: index, kind, first transitions, bad levels."""
  mine = [(s, CLASS_NAMES[x], CLASS_NAMES[y]) for (cc, s, x, y) in trans if cc == col][:4]
  return (col, c["kind"][col], mine, bad_levels[:6])
