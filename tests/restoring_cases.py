"""The NumPy restatement of pm_series_restoring, its forward bound, an independent evaluation and
the case table.

The restatement follows include/pymoc_hip.h literally: per sliding window pass 1 of
pm_series_windows, then the one pass over the pairs that forms the fourteen sums, then the scalar
iterations, every expression parenthesised as the header parenthesises it -- loops over records,
vectorised over windows, indices and members, every NumPy product, sum and quotient an IEEE
operation of the array's type rounded on its own.  In float64 it is the authority the device's lam
and rho are compared with bit for bit.

`fit` is written once, on operands that are either arrays or `Tracked` values: a Tracked value
carries, next to the float64 value the restatement computes, a running bound on its distance from
the exact-arithmetic value of the same expression.  `direct` evaluates one
iteration in np.longdouble by whitened passes -- no lagged sums, no polynomials in rho -- and is
what the bound is tested against, iteration by iteration with the restatement's own rho fed in.
Shared by tests/test_restoring_cpu.py and the GPU tests.  Pure NumPy; nothing here imports the
product.
"""
import numpy as np

import dfa_cases as DC
import windows_cases as WC

WIN_MIN, ITERS_MAX, DEFAULT_ITERS = 8, 64, 10
NAN = float("nan")
U = 2.0 ** -53
DETRENDS = WC.DETRENDS
stt_of = DC.stt_of


# ------------------------------------------------------------------ values with a running bound
class Tracked(object):
  """A float64 value v computed as the restatement computes it, and e >= |v - the exact-arithmetic
  value of the same expression of the same inputs|.  With u = 2^-53 and round to nearest,
  |fl(z) - z| <= u |fl(z)| for every normal result, so (operands a, b with bounds ea, eb):
    a +- b   e = ea + eb + u |v|
    a * b    e = |a| eb + |b| ea + ea eb + u |v|
    a / b    e = (ea + |v| eb) / (|b| - eb) + u |v|,  inf where eb >= |b|
  An array or a number as the other operand is exact (e = 0).  Nothing is dropped to first order,
  so e is a bound, not an estimate, up to the rounding of e's own evaluation and results below
  the normal range (`slack` covers the first; the table's smallest squares are near 1e-300)."""
  __array_ufunc__ = None  # (an array or a NumPy scalar on the left defers to the methods below)

  def __init__(self, v, e=None):
    self.v = np.asarray(v, dtype=np.float64)
    self.e = np.zeros(self.v.shape) if e is None else np.asarray(e, dtype=np.float64)

  @staticmethod
  def _of(o):
    return o if isinstance(o, Tracked) else Tracked(o)

  def __getitem__(self, i):
    return Tracked(self.v[i], self.e[i])

  @property
  def shape(self):
    return self.v.shape

  def __add__(self, o):
    o = self._of(o)
    v = self.v + o.v
    return Tracked(v, self.e + o.e + U * np.abs(v))

  def __sub__(self, o):
    o = self._of(o)
    v = self.v - o.v
    return Tracked(v, self.e + o.e + U * np.abs(v))

  def __rsub__(self, o):
    return self._of(o) - self

  def __mul__(self, o):
    o = self._of(o)
    v = self.v * o.v
    return Tracked(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

  __rmul__ = __mul__
  __radd__ = __add__

  def __truediv__(self, o):
    o = self._of(o)
    v = self.v / o.v
    den = np.abs(o.v) - o.e
    e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
    return Tracked(v, e + U * np.abs(v))

  def __rtruediv__(self, o):
    return self._of(o) / self


def twice(a):
  """2.0 * a, which is exact (and a + a bit for bit)."""
  return Tracked(a.v + a.v, a.e + a.e) if isinstance(a, Tracked) else a + a


# ------------------------------------------------------------------ the definition, once
def sums(x, W, detrend, T):
  """Pass 1 and pass 2 of the header on x [..., W] (an array of type T, or Tracked): the dict of
  the fourteen sums, Sxy2, Sy2, Sx2, x0, y0 and Mf."""
  lead = x.shape[:-1]
  tracked = isinstance(x, Tracked)
  zero = (lambda: Tracked(np.zeros(lead))) if tracked else (lambda: np.zeros(lead, dtype=T))
  half = T(0.5) * T(W - 1)
  t = np.arange(W).astype(T) - half
  s_, st = zero(), zero()
  for j in range(W):
    s_ = s_ + x[..., j]
    if detrend == "linear":
      st = st + t[j] * x[..., j]
  mean = s_ / T(W)
  slope = st / T(stt_of(W)) if detrend == "linear" else None

  def d(j):
    if detrend == "linear":
      return (x[..., j] - mean) - slope * t[j]
    return x[..., j] - mean  # "constant", and "none": lambda does not depend on an offset

  d0, dl = d(0), d(1)
  x0, y0 = d0, dl - d0
  xp, yp = x0, y0
  names = ("xc", "xp", "yc", "yp", "xcxc", "xcxp", "xpxp", "xcyc", "xcyp", "xpyc", "xpyp", "ycyc",
           "ycyp", "ypyp")
  S = {k: zero() for k in names}
  for j in range(2, W):
    dj = d(j)
    xc, yc = dl, dj - dl
    S["xc"] = S["xc"] + xc
    S["xp"] = S["xp"] + xp
    S["yc"] = S["yc"] + yc
    S["yp"] = S["yp"] + yp
    S["xcxc"] = S["xcxc"] + xc * xc
    S["xcxp"] = S["xcxp"] + xc * xp
    S["xpxp"] = S["xpxp"] + xp * xp
    S["xcyc"] = S["xcyc"] + xc * yc
    S["xcyp"] = S["xcyp"] + xc * yp
    S["xpyc"] = S["xpyc"] + xp * yc
    S["xpyp"] = S["xpyp"] + xp * yp
    S["ycyc"] = S["ycyc"] + yc * yc
    S["ycyp"] = S["ycyp"] + yc * yp
    S["ypyp"] = S["ypyp"] + yp * yp  # (formed as the header lists it; nothing reads it)
    xp, yp, dl = xc, yc, dj
  S["xy2"] = S["xcyp"] + S["xpyc"]
  S["y2"] = S["yc"] + S["yp"]
  S["x2"] = S["xc"] + S["xp"]
  S["x0"], S["y0"], S["Mf"] = x0, y0, T(W - 2)
  return S


def fit(S, r, T):
  """lambda_i and a of the header from the sums S and r = rho_i (an exact array of type T)."""
  Mf = S["Mf"]
  r2 = r * r
  SX = S["xc"] - r * S["xp"]
  SY = S["yc"] - r * S["yp"]
  SXX = (S["xcxc"] - twice(r) * S["xcxp"]) + r2 * S["xpxp"]
  SXY = (S["xcyc"] - r * S["xy2"]) + r2 * S["xpyp"]
  mx, my = SX / Mf, SY / Mf
  lam = (SXY - SX * my) / (SXX - SX * mx)
  a = (my - lam * mx) / (T(1.0) - r)
  return lam, a


def next_rho(S, lam, a):
  """rho_{i+1} of the header from the sums, lambda_i and a."""
  Mf = S["Mf"]
  e0 = (S["y0"] - a) - lam * S["x0"]
  l2, al, a2m = lam * lam, a * lam, Mf * (a * a)
  q = (((((S["ycyc"] - twice(a) * S["yc"]) - twice(lam) * S["xcyc"]) + twice(al) * S["xc"])
        + l2 * S["xcxc"]) + a2m) + e0 * e0
  c = ((((S["ycyp"] - a * S["y2"]) - lam * S["xy2"]) + al * S["x2"]) + l2 * S["xcxp"]) + a2m
  return c / q


def restoring(v, k0, k1, W, S, detrend, iters, dtype=np.float64, trace=False):
  """dict(lam, rho [nwin, nspec, n], used) of the series v [nrec, nspec, n], every operation in
  `dtype`; with trace=True also lams and rhos, the lists of lambda_i and rho_i over i < iters
  (before the NaN rule), and sums, the dict of `sums`."""
  T = dtype
  x = WC.window_values(v, k0, k1, W, S)
  used = np.isfinite(x).all(axis=-1)
  with np.errstate(all="ignore"):
    sm = sums(x.astype(T), W, detrend, T)
    r = np.zeros(x.shape[:-1], dtype=T)
    lams, rhos = [], []
    for i in range(iters):
      lam, a = fit(sm, r, T)
      lams.append(lam)
      rhos.append(r)
      if i + 1 < iters:
        r = next_rho(sm, lam, a)
    ok = used & np.isfinite(lam.astype(np.float64)) & np.isfinite(r.astype(np.float64))
  res = dict(lam=np.where(ok, lam, T(NAN)), rho=np.where(ok, r, T(NAN)), used=used)
  if trace:
    res.update(lams=lams, rhos=rhos, sums=sm)
  return res


# ------------------------------------------------------------------ the independent evaluation
def direct(v, k0, k1, W, S, detrend, r):
  """One iteration in np.longdouble by whitened passes, with r = rho_i [nwin, nspec, n] given:
  (lambda_i, rho_{i+1}).  The residual by NumPy's reductions, the pairs and the whitened variables
  as arrays, the regression from their sums, the unwhitened residuals e_t as an array: none of
  the restatement's lagged sums or polynomials."""
  L = np.longdouble
  x = WC.window_values(v, k0, k1, W, S).astype(L)
  r = np.asarray(r).astype(L)[..., None]
  with np.errstate(all="ignore"):
    t = np.arange(W).astype(L) - L(W - 1) / L(2)
    d = x - x.sum(axis=-1, keepdims=True) / L(W)
    if detrend == "linear":
      d = d - ((x * t).sum(axis=-1, keepdims=True) / (t * t).sum()) * t
    xs, ys = d[..., :-1], d[..., 1:] - d[..., :-1]
    X, Y = xs[..., 1:] - r * xs[..., :-1], ys[..., 1:] - r * ys[..., :-1]
    M = L(W - 2)
    sx, sy = X.sum(axis=-1), Y.sum(axis=-1)
    lam = ((X * Y).sum(axis=-1) - sx * sy / M) / ((X * X).sum(axis=-1) - sx * sx / M)
    a = (sy / M - lam * sx / M) / (L(1) - r[..., 0])
    e = ys - a[..., None] - lam[..., None] * xs
    rho = (e[..., 1:] * e[..., :-1]).sum(axis=-1) / (e * e).sum(axis=-1)
  return lam, rho


def direct_iterated(v, k0, k1, W, S, detrend, iters):
  """`direct` iterated from rho = 0 in np.longdouble throughout: (lam, rho) of the last iteration,
  for the end-to-end difference DESIGN.md section 28 reports (not a bound: the iteration map may
  expand a difference)."""
  x = WC.window_values(v, k0, k1, W, S)
  r = np.zeros(x.shape[:-1], dtype=np.longdouble)
  for i in range(iters):
    lam, nxt = direct(v, k0, k1, W, S, detrend, r)
    if i + 1 < iters:
      r = nxt
  return lam, r


SLACK = 1.0 + 2.0 ** -9


def bounds(v, k0, k1, W, S, detrend, rhos):
  """The forward bound of DESIGN.md section 28, iteration by iteration: for every rho_i of `rhos`
  (the restatement's own, taken as exact inputs) the pair of Tracked (lambda_i, rho_{i+1}) --
  values that equal the restatement's bit for bit, and bounds on their distance from the exact
  lambda and next rho of that rho_i.  The bounds are multiplied by 1 + 2^-9, which covers the
  roundings of the bound's own evaluation (a few hundred u relative) and of the np.longdouble
  reference (2^-11 of float64's at every operation)."""
  x = WC.window_values(v, k0, k1, W, S)
  with np.errstate(all="ignore"):
    sm = sums(Tracked(x), W, detrend, np.float64)
    out = []
    for r in rhos:
      lam, a = fit(sm, np.asarray(r, dtype=np.float64), np.float64)
      nxt = next_rho(sm, lam, a)
      out.append((Tracked(lam.v, lam.e * SLACK), Tracked(nxt.v, nxt.e * SLACK)))
  return out


# ------------------------------------------------------------------ the case table
# offset and huge as in dfa_cases (1e6 + AR(1), which matters under "none"; AR(1) * 1e154, whose
# squares overflow); persist: AR(1) with coefficient 0.99, the regime the lagged sums cancel most
# in; geom: x_t = 2^(40 - t) from the record window's start, an exactly geometric decay -- the line
# lambda = -1/2 fits its increments exactly, so where every operation is exact (W = 8, "none" and
# "constant") q = 0 and rho = 0 / 0
STYLES = DC.STYLES + ("persist", "geom")
K0, AFTER = WC.K0, WC.AFTER


def style_of(s, m):
  return STYLES[(m + 3 * s) % len(STYLES)]


def case(W, S, nwin, n, nspec, detrend, iters, seed=0):
  """As windows_cases.case: a series [K0 + K + AFTER, nspec, n] whose record window [K0, K0 + K)
  holds nwin whole windows and a tail of min(S - 1, 3) records that fits none, between records that
  would change every result if they were read.  Member m of index s has the style
  STYLES[(m + 3 s) % 13]."""
  rng = np.random.default_rng(9000 + 17 * W + seed)
  tail = min(S - 1, 3)
  K = W + (nwin - 1) * S + tail
  nrec = K0 + K + AFTER
  v = np.empty((nrec, nspec, n))
  a = rng.standard_normal((nspec, n))
  p = rng.standard_normal((nspec, n)) / np.sqrt(1.0 - 0.99 ** 2)
  slow = np.empty((nrec, nspec, n))
  for k in range(nrec):
    a = 0.9 * a + np.sqrt(1.0 - 0.81) * rng.standard_normal((nspec, n))
    p = 0.99 * p + rng.standard_normal((nspec, n))
    v[k], slow[k] = a, p
  for s in range(nspec):
    for m in range(n):
      style = style_of(s, m)
      if style == "offset":
        v[:, s, m] = 1e6 + v[:, s, m]
      elif style == "huge":
        v[:, s, m] = 1e154 * v[:, s, m]
      elif style == "persist":
        v[:, s, m] = slow[:, s, m]
      elif style == "geom":
        v[:, s, m] = 2.0 ** (40.0 - (np.arange(nrec) - K0))
      else:
        v[:, s, m] = WC._series(rng, style, v[:, s, m].copy(), K0, W, S, nwin)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  return dict(name="W %d S %d nwin %d n %d nspec %d %s iters %d"
              % (W, S, nwin, n, nspec, detrend, iters),
              v=v, k0=K0, k1=K0 + K, W=W, S=S, nwin=nwin, detrend=detrend, iters=iters)


MANY = 300  # windows of the case whose second chunk is partial (W 20, S 1: a block takes 288)


def cases():
  """The smallest shapes at which the kernel can go wrong: the minimum W = 8 with one window of one
  member and one iteration; W = 8 where the geometric decay is exact; W = 9; W = 20, S = 1 with 300
  windows (a full and a partial chunk) of 37 members (no multiple of a tile) and 10 iterations;
  W = 64 at 1, 2, 10 and 64 iterations; W = 256; one window of 4096 records of three members (the
  tile of 4).  nspec = 1 to 3, the three detrends, k0 = 3 with records behind k1 (every case)."""
  out = [case(8, 8, 1, 1, 1, "linear", 1, 1),
         case(8, 8, 3, 37, 2, "none", 3, 2),
         case(8, 2, 4, 37, 2, "constant", 2, 3)]
  seed = 3
  for det in DETRENDS:
    seed += 1
    out.append(case(9, 3, 4, 33, 3, det, 10, seed))
  out.append(case(20, 1, MANY, 37, 1, "linear", 10, 7))
  for det, iters in (("linear", 1), ("constant", 2), ("none", 10), ("linear", 64), ("linear", 10)):
    seed += 10
    out.append(case(64, 3, 4, 37, 2, det, iters, seed))
  for det in DETRENDS:
    seed += 1
    out.append(case(256, 8, 4, 37, 3, det, 10, seed))
  out.append(case(4096, 4096, 1, 3, 1, "linear", 10, 90))
  return out


def restate(c, v=None, **kw):
  """The restatement of a case (or of another series under the case's settings)."""
  return restoring(c["v"] if v is None else v, c["k0"], c["k1"], c["W"], c["S"], c["detrend"],
                   c["iters"], **kw)


# ------------------------------------------------------------------ the restated surrogate test
def significance(v, k0, k1, W, S, detrend, iters, nsur, seed=0, nb=None, sur=None):
  """surrogate_cases.significance for lambda: dict(tau, ge, le, nvalid, p_rising, p_falling), each
  [nspec, n], of the trend of the restated lambda series; AR(1) surrogates of the restated fit
  unless `sur` [K, nsur * nspec, n] gives the surrogate series."""
  import surrogate_cases as SGC
  v = np.asarray(v, dtype=np.float64)
  nspec, n = v.shape[1:]
  K = k1 - k0
  obs = restoring(v, k0, k1, W, S, detrend, iters)["lam"]
  nwin = obs.shape[0]
  var, ac = SGC.fit(v, k0, k1, detrend) if sur is None else (None, None)
  counts = WC.kendall(obs, 0, nwin)
  acc = [np.zeros((nspec, n), dtype=np.int32) for _ in range(3)]
  for b0, m in SGC.chunks(nsur, nb or nsur):
    if sur is None:
      y = SGC.surrogates(var, ac, K, b0, m, seed, np.arange(n))
    else:
      y = np.asarray(sur)[:, b0 * nspec:(b0 + m) * nspec]
    lam = restoring(y, 0, K, W, S, detrend, iters)["lam"]
    for a, add in zip(acc, SGC.exceed(counts, WC.kendall(lam, 0, nwin))):
      a += add
  return DC.of_counts(counts, acc)
