"""The NumPy restatement of pm_series_group_stats and pm_series_member_stats, and the case table.

The restatement follows the orders include/pymoc_hip.h states literally (Python floats and NumPy
float64 scalars are IEEE doubles, every operation rounded on its own); it is the authority the
device results are compared with bit for bit.  Shared by tests/test_stats_cpu.py (which checks the
restatement against np.quantile, math.fsum, np.var) and tests/test_stats_gpu.py.
"""
import numpy as np

Q_MAX, LAG_MAX, GROUP_MAX, CHUNK = 8, 4, 8192, 256
PROBS = np.array([0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0])
NAN = float("nan")


# ------------------------------------------------------------------ across members
def tree_sum(terms):
  """The member tree over `terms` [..., G] (already +0.0 where a value is excluded): p[l] = the
  sequential sum in ascending j of the terms with j = l (mod 64), from +0.0; then strides 32 .. 1.
  (Rows are padded with +0.0 to a multiple of 64: p + 0.0 is p, bit for bit, because a sum that
  starts from +0.0 is never -0.0.)"""
  terms = np.asarray(terms, dtype=np.float64)
  G = terms.shape[-1]
  rows = -(-G // 64)
  pad = np.zeros(terms.shape[:-1] + (rows * 64,))
  pad[..., :G] = terms
  pad = pad.reshape(terms.shape[:-1] + (rows, 64))
  p = np.zeros(terms.shape[:-1] + (64,))
  for r in range(rows):
    p = p + pad[..., r, :]
  stride = 32
  while stride >= 1:
    p = p.copy()
    p[..., :stride] = p[..., :stride] + p[..., stride:2 * stride]
    stride //= 2
  return p[..., 0]


def sort_finite(x):
  """The finite values of x ascending, -0.0 before +0.0."""
  f = np.asarray(x, dtype=np.float64)
  f = f[np.isfinite(f)]
  return f[np.lexsort((~np.signbit(f), f))]


def quantile(srt, q):
  """NumPy's method="linear" on the sorted values, as the header states it."""
  m = srt.size
  vi = np.float64(q) * np.float64(m - 1)
  fl = np.floor(vi)
  lo = int(fl)
  hi = min(lo + 1, m - 1)
  g = vi - fl
  a, b = srt[lo], srt[hi]
  with np.errstate(all="ignore"):
    return b - (b - a) * (np.float64(1.0) - g) if g >= 0.5 else a + (b - a) * g


def group_one(x, probs):
  """(count, [mean, var, min, max, sum, q...]) of one group's values x in `order`."""
  x = np.asarray(x, dtype=np.float64)
  out = np.full(5 + len(probs), NAN)
  fin = np.isfinite(x)
  count = int(fin.sum())
  if count == 0:
    return 0, out
  with np.errstate(all="ignore"):
    s = tree_sum(np.where(fin, x, 0.0))
    mean = s / np.float64(count)
    d = np.where(fin, x - mean, 0.0)
    Q = tree_sum(d * d)
    var = Q / np.float64(count - 1) if count >= 2 else NAN
  srt = sort_finite(x)
  out[:5] = mean, var, srt[0], srt[-1], s
  for i, q in enumerate(probs):
    out[5 + i] = quantile(srt, q)
  return count, out


def group_stats(v, order, start, probs, k0, k1):
  """count [K, nspec, ngroups] int32 and stat [K, nspec, ngroups, 5 + nq] of records [k0, k1)."""
  v = np.asarray(v, dtype=np.float64)
  ng, nspec = len(start) - 1, v.shape[1]
  count = np.zeros((k1 - k0, nspec, ng), dtype=np.int32)
  stat = np.full((k1 - k0, nspec, ng, 5 + len(probs)), NAN)
  for k in range(k0, k1):
    for s in range(nspec):
      for g in range(ng):
        members = order[start[g]:start[g + 1]]
        count[k - k0, s, g], stat[k - k0, s, g] = group_one(v[k, s, members], probs)
  return count, stat


# ------------------------------------------------------------------ along the records
def chunk_sum(terms):
  """The time sum over `terms` [K, ...]: per chunk of 256 records the sequential sum in ascending
  k from +0.0; the total is the sequential sum of the chunk partials, from +0.0."""
  terms = np.asarray(terms, dtype=np.float64)
  total = np.zeros(terms.shape[1:])
  for c0 in range(0, terms.shape[0], CHUNK):
    acc = np.zeros(terms.shape[1:])
    for k in range(c0, min(c0 + CHUNK, terms.shape[0])):
      acc = acc + terms[k]
    total = total + acc
  return total


def _signed_extreme(w, fin, take_min):
  """min / max over the finite records; of -0.0 and +0.0, min takes -0.0 and max +0.0."""
  fill = np.inf if take_min else -np.inf
  e = np.where(fin, w, fill)
  e = e.min(axis=0) if take_min else e.max(axis=0)
  zero = fin & (w == 0.0) & (np.signbit(w) == take_min)
  e = np.where((e == 0.0) & zero.any(axis=0), -0.0 if take_min else 0.0, e)
  return np.where(fin.any(axis=0), e, NAN)


def member_stats(v, lags, thr, dirs, k0, k1):
  """(count, first, ncross) [nspec, n] int32 and stat [nspec, n, 6 + nlag] of records [k0, k1)."""
  w = np.asarray(v, dtype=np.float64)[k0:k1]
  K, nspec, n = w.shape
  fin = np.isfinite(w)
  count = fin.sum(axis=0).astype(np.int32)
  stat = np.full((nspec, n, 6 + len(lags)), NAN)
  with np.errstate(all="ignore"):
    total = chunk_sum(np.where(fin, w, 0.0))
    mean = total / count.astype(np.float64)
    d = np.where(fin, w - mean, 0.0)
    var = np.where(count >= 2, chunk_sum(d * d) / (count - 1).astype(np.float64), NAN)
    stat[..., 0], stat[..., 1], stat[..., 4] = mean, var, total
    stat[..., 2], stat[..., 3] = _signed_extreme(w, fin, True), _signed_extreme(w, fin, False)
    for i, L in enumerate(lags):
      ok = np.zeros_like(fin)
      ok[:K - L] = fin[:K - L] & fin[L:]
      prod = np.zeros_like(w)
      prod[:K - L] = (w[:K - L] - mean) * (w[L:] - mean)
      npair = ok.sum(axis=0)
      c = chunk_sum(np.where(ok, prod, 0.0)) / npair.astype(np.float64)
      stat[..., 6 + i] = np.where(npair > 0, c, NAN)
    t = np.asarray(thr, dtype=np.float64)[None, :, None]
    below = (np.asarray(dirs) < 0)[None, :, None]
    hit = fin & np.where(below, w < t, w > t)  # (a NaN threshold compares false: no hit)
    has = ~np.isnan(t[0])
    hits = hit.sum(axis=0)
    stat[..., 5] = np.where(has, hits.astype(np.float64) / count.astype(np.float64), NAN)
  first = np.where(hit.any(axis=0), k0 + hit.argmax(axis=0), -1).astype(np.int32)
  cross = fin[:-1] & fin[1:] & (hit[:-1] != hit[1:])
  return count, first, cross.sum(axis=0).astype(np.int32), stat


# ------------------------------------------------------------------ the case table
def order_of(groups):
  """(order, start) of integer labels: the stable sort pymoc_amd.stats.group_order restates."""
  groups = np.asarray(groups)
  labels, counts = np.unique(groups, return_counts=True)
  order = np.argsort(groups, kind="stable").astype(np.int32)
  return order, np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


STYLES = ("noisy", "ties", "span", "equal", "one", "none")


def _fill(rng, style, n, order, start):
  """One (record, index) row of n members in the given style."""
  if style == "noisy":      # NaN and +-inf sprinkled in
    x = rng.standard_normal(n)
    bad = rng.random(n) < 0.1
    x[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    return x
  if style == "ties":       # few distinct values, -0.0 / +0.0 pairs: zero is the minimum of the
    x = np.zeros(n)         # even groups and the maximum of the odd ones
    for g in range(len(start) - 1):
      members = order[start[g]:start[g + 1]]
      x[members] = rng.integers(0, 3, size=members.size) * (1.0 if g % 2 == 0 else -1.0)
    zero = x == 0.0
    x[zero] = np.where(rng.random(int(zero.sum())) < 0.5, -0.0, 0.0)
    return x
  if style == "span":       # magnitudes 1e-300 .. 1e300, both signs
    return np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-300, 300, size=n)
  if style == "equal":      # every group all-equal (0.1 is not a dyadic fraction: sums round)
    return np.full(n, 0.1)
  x = np.full(n, np.nan)
  x[rng.random(n) < 0.5] = np.inf
  if style == "one":        # exactly one finite member per group, not the first of the group
    for g in range(len(start) - 1):
      G = start[g + 1] - start[g]
      if G:
        x[order[start[g] + (G * 2) // 3]] = rng.standard_normal()
  return x                  # "none": no finite member anywhere


def group_case(name, sizes=None, interleaved=None, seed=0):
  """A series [5, 2, n] whose window [1, 4) holds one (record, index) pair of every style; records
  0 and 4 are ordinary numbers that would change every result if they were read.
    sizes        contiguous groups of these sizes (identity order); a size 0 is an empty group
    interleaved  (n, ngroups): groups = m % ngroups"""
  rng = np.random.default_rng(1000 + seed)
  if sizes is not None:
    start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    n = int(start[-1])
    order = np.arange(n, dtype=np.int32)
    groups = None
  else:
    n, ng = interleaved
    groups = np.arange(n) % ng
    order, start = order_of(groups)
  v = rng.standard_normal((5, 2, n)) * 100.0
  for i, style in enumerate(STYLES):
    v[1 + i // 2, i % 2] = _fill(rng, style, n, order, start)
  return dict(name=name, v=v, order=order, start=start, groups=groups, probs=PROBS, k0=1, k1=4)


def group_cases():
  return [
      group_case("small sizes", sizes=[0, 1, 2, 3, 63, 64], seed=1),
      group_case("both sides of 64", sizes=[65, 3, 128, 0, 64, 129], seed=2),
      group_case("1000 and 5", sizes=[1000, 5], seed=3),
      group_case("8192", sizes=[GROUP_MAX], seed=4),
      group_case("interleaved small", interleaved=(64, 5), seed=5),
      group_case("interleaved large", interleaved=(200, 3), seed=6),
      group_case("one member", sizes=[1], seed=7),
  ]


THR = np.array([-1.0, 1.0, np.nan])
DIRS = np.array([-1, 1, -1], dtype=np.int32)
LAGS = (1, 2, 10, 255)


def _zeros(count):
  return np.where(np.arange(count) % 2 == 1, -0.0, 0.0)


def member_case(K, n, k0=2, tail=3, seed=0):
  """A series [k0 + K + tail, 3, n], window [k0, k0 + K): index 0 with the threshold "below -1",
  index 1 with "above 1", index 2 with none.  Member by member (those that exist):
    0  a hit at the first and at the last record of the window
    1  never hits (all values inside (-0.5, 0.5))
    2  goes non-finite half-way and stays so
    3  non-finite at isolated records only
    4  values exactly equal to the threshold (no hit); -0.0 / +0.0 pairs under positive values in
       index 2
    5  no finite record at all
    6  -0.0 / +0.0 pairs on top of negative values in index 2"""
  rng = np.random.default_rng(2000 + 7 * K + n + seed)
  nrec, k1 = k0 + K + tail, k0 + K
  v = rng.standard_normal((nrec, 3, n)) * 1.5
  hitv = np.array([-2.0, 2.0, 0.0])
  v[k0, :, 0] = hitv
  v[k1 - 1, :, 0] = hitv
  if n > 1:
    v[:, :, 1] = np.clip(v[:, :, 1], -0.4, 0.4)
  if n > 2:
    v[k0 + K // 2:, :, 2] = np.nan
  if n > 3:
    v[k0 + K // 3, :, 3] = np.inf
    v[k0 + (2 * K) // 3, :, 3] = np.nan
  if n > 4:
    v[k0:k1:3, 0, 4], v[k0:k1:3, 1, 4] = THR[0], THR[1]
    v[:, 2, 4] = np.abs(v[:, 2, 4])  # positive values and signed zeros: the minimum is -0.0
    v[k0:k1:3, 2, 4] = _zeros(len(range(k0, k1, 3)))
  if n > 5:
    v[:, :, 5] = -np.inf
  if n > 6:
    v[:, 2, 6] = -np.abs(v[:, 2, 6])  # negative values and signed zeros: the maximum is +0.0
    v[k0:k1:3, 2, 6] = _zeros(len(range(k0, k1, 3)))
  lags = tuple(L for L in LAGS if L < K)
  return dict(name="K %d n %d k0 %d" % (K, n, k0), v=v, lags=lags, thr=THR, dirs=DIRS, k0=k0,
              k1=k1)


def member_cases():
  return [member_case(1, 5), member_case(2, 1), member_case(255, 5), member_case(256, 64),
          member_case(257, 65), member_case(600, 65), member_case(600, 5, k0=0, tail=0),
          member_case(257, 1, k0=1, tail=1)]
