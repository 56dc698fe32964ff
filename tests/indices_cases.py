"""The index definitions of pm_row_indices restated in NumPy, and the case table of its tests
(helper module, no tests).  Shared by tests/test_indices_cpu.py and tests/test_indices_gpu.py.

`restate(row, axis, kind, lo, hi, param)` -> (value, pos) is the table of include/pymoc_hip.h
written out level by level; the CPU test holds its "max" / "min" to np.argmax / np.argmin and its
"at" to np.interp.  "mean" sums with math.fsum, so it is the exactly rounded trapezoid sum the
kernel is allowed `mean_bound` around.

A case is (id, kind, row [nlev], lo, hi, param) on `axis_for(nlev)`; `member_rows` makes the rows
of the other members from it.
"""
import functools
import math

import numpy as np

KINDS = ("max", "min", "at", "cross", "mean")
NLEVS = (1, 2, 3, 63, 64, 65, 129, 200, 257)
MEMBERS = (1, 3, 5)


def _before(bv, bi, av, ai, is_max):
  """Does (bv, bi) come before (av, ai): a NaN first, then the value, then the lower level."""
  bn, an = bv != bv, av != av
  if bn or an:
    return bn and (not an or bi < ai)
  if bv != av:
    return bv > av if is_max else bv < av
  return bi < ai


def restate(row, axis, kind, lo, hi, param=0.0):
  row, axis = np.asarray(row, dtype=np.float64), np.asarray(axis, dtype=np.float64)
  if kind in ("max", "min"):
    pos = lo
    for i in range(lo + 1, hi + 1):
      if _before(row[i], i, row[pos], pos, kind == "max"):
        pos = i
    return row[pos], pos
  if kind == "at":
    with np.errstate(invalid="ignore"):
      return np.float64(np.interp(param, axis, row)), -1
  if kind == "cross":
    c = np.float64(param)
    if row[hi] == c:
      return axis[hi], hi
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
      for i in range(hi - 1, lo - 1, -1):
        d0, d1 = row[i] - c, row[i + 1] - c
        if (d0 <= 0 < d1) or (d0 >= 0 > d1):
          t = (c - row[i]) / (row[i + 1] - row[i])
          return axis[i] + t * (axis[i + 1] - axis[i]), i
    return np.float64(np.nan), -1
  if kind == "mean":
    if hi == lo:
      return row[lo], -1
    return np.float64(math.fsum(_terms(row, axis, lo, hi)) / (axis[hi] - axis[lo])), -1
  raise KeyError(kind)


def _terms(row, axis, lo, hi):
  return [0.5 * (row[i] + row[i + 1]) * (axis[i + 1] - axis[i]) for i in range(lo, hi)]


def mean_bound(row, axis, lo, hi):
  """What the kernel's own summation order may differ from the fsum restatement by:
  (m + 4) * 2**-53 * sum|term_i| / |axis[hi] - axis[lo]|, m = the number of terms.  Each term
  carries three roundings, a sum of m terms in any order m - 1, the quotient one."""
  if hi == lo:
    return 0.0
  t = _terms(np.asarray(row, dtype=np.float64), np.asarray(axis, dtype=np.float64), lo, hi)
  return (len(t) + 4) * 2.0**-53 * math.fsum(abs(x) for x in t) / abs(axis[hi] - axis[lo])


@functools.lru_cache(maxsize=None)
def axis_for(nlev):
  """Strictly increasing, non-uniform, ending at 0 (a depth axis)."""
  dz = 1.3 + 0.37 * (np.arange(nlev) % 7) + 0.011 * np.arange(nlev)
  z = np.cumsum(dz)
  return z - z[-1]


def member_rows(row, n):
  """[n, nlev]: member 0 is the case's row, member j the row rotated by 7 j levels and scaled."""
  row = np.asarray(row, dtype=np.float64)
  return np.stack([row] + [np.roll(row, 7 * j) * (1.0 + 0.25 * j) for j in range(1, n)])


def _base(nlev, seed):
  rng = np.random.default_rng(1000 * nlev + seed)
  return rng.standard_normal(nlev) * 10.0**rng.integers(-2, 3, nlev)


def _inner(nlev):
  """A window that leaves a level outside on either side where the row is long enough."""
  return (1, nlev - 2) if nlev >= 3 else (0, nlev - 1)


def extremum_cases(nlev):
  """(id, "max", row, lo, hi, 0.0); the "min" cases are these with the row negated."""
  out = []
  full = (0, nlev - 1)

  def add(name, row, win):
    row = np.asarray(row, dtype=np.float64)
    out.append((name + "-max", "max", row, win[0], win[1], 0.0))
    out.append((name + "-min", "min", -row, win[0], win[1], 0.0))

  def peak(seed, where, val=1e4):
    r = _base(nlev, seed)
    for p in np.atleast_1d(where):
      r[p] = val
    return r

  lo, hi = _inner(nlev)
  add("at-lo", peak(1, lo), (lo, hi))
  add("at-hi", peak(2, hi), (lo, hi))
  for p in (63, 64):  # either side of the lane wrap
    if p < nlev:
      add("at-%d" % p, peak(3, p), full)
  if nlev <= 3:
    for p in range(nlev):
      add("short-%d" % p, peak(4, p), full)
  add("constant", np.full(nlev, 2.5), (lo, hi))
  if hi - lo >= 6:
    add("tie-lanes", peak(5, [lo + 1, lo + 6]), (lo, hi))
    add("tie-lanes-rev", peak(6, [hi - 6, hi]), (lo, hi))
  if nlev > 66:
    add("tie-same-lane", peak(7, [2, 66]), full)
    add("tie-wrap", peak(8, [63, 64]), full)
  mid = nlev // 2
  add("one-level", _base(nlev, 9), (mid, mid))
  if nlev >= 3:
    r = _base(nlev, 10)
    r[lo - 1] = r[hi + 1] = 1e6  # larger, and outside the window
    add("excluded", r, (lo, hi))
  for name, where in (("nan-first", [lo]), ("nan-mid", [(lo + hi) // 2]), ("nan-last", [hi])):
    add(name, peak(11, where, np.nan), (lo, hi))
  if hi > lo:
    add("two-nans", peak(12, [lo + (hi - lo) // 3, hi], np.nan), (lo, hi))
    r = peak(13, [lo], np.inf)
    r[hi] = -np.inf
    add("infs", r, (lo, hi))
    r = peak(14, [lo, hi], np.inf)
    add("two-infs", r, (lo, hi))
    for name, pair in (("zeros-mp", (-0.0, 0.0)), ("zeros-pm", (0.0, -0.0))):
      for kind, fill in (("max", -5.0), ("min", 5.0)):  # the two zeros are the extremum
        r = np.full(nlev, fill)
        r[lo], r[lo + 1] = pair
        out.append(("%s-%s" % (name, kind), kind, r, lo, hi, 0.0))
  return out


def at_cases(nlev):
  z = axis_for(nlev)
  out = []
  full = (0, nlev - 1)

  def add(name, row, x0):
    out.append((name, "at", np.asarray(row, dtype=np.float64), full[0], full[1], float(x0)))

  r = _base(nlev, 20)
  add("below", r, z[0] - 3.0)
  add("above", r, z[-1] + 3.0)
  add("first-node", r, z[0])
  add("last-node", r, z[-1])
  add("nan", r, np.nan)
  if nlev >= 2:
    k = nlev // 2
    add("node", r, z[k])
    add("between", r, 0.3 * z[k - 1] + 0.7 * z[k])
    add("between-first", r, 0.5 * (z[0] + z[1]))
    add("just-below-node", r, np.nextafter(z[k], -np.inf))
    add("just-above-node", r, np.nextafter(z[k - 1], np.inf))
    ri = r.copy()
    ri[k] = np.inf  # slope inf: (x - x0) * inf, never NaN unless x == x0
    add("inf-right", ri, 0.5 * (z[k - 1] + z[k]))
    if k + 1 < nlev:
      add("inf-left", ri, 0.5 * (z[k] + z[k + 1]))  # slope -inf, f0 = inf: NaN, then the fallbacks
      rr = ri.copy()
      rr[k + 1] = np.inf  # inf - inf: NaN slope, f0 == f1
      add("inf-both", rr, 0.5 * (z[k] + z[k + 1]))
      rr = ri.copy()
      rr[k + 1] = -np.inf
      add("inf-opposite", rr, 0.5 * (z[k] + z[k + 1]))
  return out


def cross_cases(nlev):
  out = []
  lo, hi = _inner(nlev)

  def add(name, row, c, win=None):
    w = (lo, hi) if win is None else win
    out.append((name, "cross", np.asarray(row, dtype=np.float64), w[0], w[1], float(c)))

  pos = np.abs(_base(nlev, 30)) + 1.0
  add("none", pos, 0.0)
  add("none-level", pos, -2.5)
  eq = pos.copy()
  eq[hi] = 0.75
  add("equal-at-hi", eq, 0.75)
  add("one-level-equal", eq, 0.75, (hi, hi))
  add("one-level-none", pos, 0.0, (hi, hi))
  if hi > lo:
    k = (lo + hi) // 2
    one = pos.copy()
    one[:k + 1] *= -1.0  # negative up to k, positive above: the pair (k, k + 1)
    add("one", one, 0.0)
    add("one-level", one, 0.3)
    down = -one
    add("one-downward", down, 0.0)
    node = one.copy()
    node[k] = 0.0  # equality exactly at an interior node
    add("equal-interior", node, 0.0)
    node2 = one.copy()
    node2[k + 1] = 0.0
    add("equal-interior-upper", node2, 0.0)
    if hi - lo >= 2:
      nb = one.copy()
      nb[k - 1 if k > lo else k + 2 if k + 2 <= hi else lo] = np.nan  # a NaN beside the crossing
      add("nan-beside", nb, 0.0)
      nk = one.copy()
      nk[k] = np.nan  # a NaN in the crossing pair: no crossing there any more
      add("nan-in-pair", nk, 0.0)
  if hi - lo >= 6:
    three = pos.copy()
    a, b, c = lo + 1, (lo + hi) // 2, hi - 2
    three[:a + 1] *= -1.0
    three[b + 1:c + 1] *= -1.0  # sign changes at (a, a+1), (b, b+1), (c, c+1): the topmost wins
    add("three", three, 0.0)
  if nlev >= 3:
    outside = pos.copy()
    outside[hi + 1] = -1.0  # the pair (hi, hi + 1) crosses, one level outside the window
    add("outside-above", outside, 0.0)
    outside = pos.copy()
    outside[lo - 1] = -1.0
    add("outside-below", outside, 0.0)
  return out


def mean_cases(nlev):
  out = []
  lo, hi = _inner(nlev)
  r = _base(nlev, 40)
  out.append(("full", "mean", r, 0, nlev - 1, 0.0))
  out.append(("inner", "mean", r, lo, hi, 0.0))
  out.append(("one-level", "mean", r, nlev // 2, nlev // 2, 0.0))
  out.append(("cancelling", "mean", np.where(np.arange(nlev) % 2, 1e8, -1e8) + r, 0, nlev - 1, 0.0))
  if hi > lo:
    out.append(("two-levels", "mean", r, lo, lo + 1, 0.0))
  return out


@functools.lru_cache(maxsize=None)
def cases(nlev):
  """Every case of one row length, ids unique."""
  out = extremum_cases(nlev) + at_cases(nlev) + cross_cases(nlev) + mean_cases(nlev)
  out = [("%s-%s" % (kind, name) if not name.endswith(kind) else name, kind, row, lo, hi, p)
         for name, kind, row, lo, hi, p in out]
  assert len({c[0] for c in out}) == len(out)
  return out


@functools.lru_cache(maxsize=None)
def expected(nlev, n):
  """[(value [n], pos [n], bound [n])] of `cases(nlev)` for the rows of `member_rows`: computed
  once, shared by the tests."""
  z = axis_for(nlev)
  out = []
  for _, kind, row, lo, hi, p in cases(nlev):
    rows = member_rows(row, n)
    vp = [restate(r, z, kind, lo, hi, p) for r in rows]
    bound = [mean_bound(r, z, lo, hi) if kind == "mean" else 0.0 for r in rows]
    out.append((np.array([v for v, _ in vp], dtype=np.float64),
                np.array([q for _, q in vp], dtype=np.int32), np.array(bound)))
  return out
