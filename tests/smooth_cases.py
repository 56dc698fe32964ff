"""The NumPy restatement of pm_series_smooth and of the "gaussian" pipeline built on it, and the
case table.

The definition (include/pymoc_hip.h), restated.  The series is v[k][s][m], the record window
[k0, k1), K = k1 - k0 <= 4096, x_j = v[k0 + j][s][m].  The caller passes a half-width H in
[1, 4095] and a table w[0 .. H], w[0] == 1, every w[d] finite and > 0, w[d + 1] <= w[d].  Per record
j, with lo = max(0, j - H) and hi = min(K - 1, j + H), every product and sum rounded on its own,
both sums sequential in ascending i from +0.0 over the i in [lo, hi] with isfinite(x_i) only:

  num     = sum w[|i - j|] * x_i
  den     = sum w[|i - j|]
  trend_j = num / den                      (NaN when no record in reach is finite)
  resid_j = x_j - trend_j if isfinite(x_j), else NaN
  nbad    = the number of non-finite records of the record window

`smooth` below walks the offsets d = i - j from -H to H -- ascending i for every j at once --
vectorised over records, indices and members, every NumPy product and sum an IEEE double operation
rounded on its own.  It is the authority the device results are compared with bit for bit.  Shared
by tests/test_smooth_cpu.py (which pins it to an extended-precision evaluation and to
scipy.ndimage.gaussian_filter1d) and the GPU tests.  Pure NumPy; nothing here imports the product.
"""
import numpy as np

import surrogate_cases as SGC
import windows_cases as WC

K_MAX, HALF_MAX = 4096, 4095
NAN = float("nan")
MUTANTS = ("descending", "den_all", "reflect", "h_minus")


def half_of(sigma, truncate=4.0):
  """SciPy's gaussian_filter1d radius."""
  return int(truncate * sigma + 0.5)


def weights(sigma, truncate=4.0):
  """w[d] = exp(-0.5 (d / sigma)^2), d = 0 .. H."""
  return np.exp(-0.5 * (np.arange(half_of(sigma, truncate) + 1, dtype=np.float64) / sigma) ** 2)


def smooth(v, k0, k1, w, mutant=None):
  """dict(trend [K, nspec, n], resid [K, nspec, n], nbad [nspec, n]) of the records [k0, k1) of the
  series v [nrec, nspec, n] under the table w [H + 1].  mutant: one of MUTANTS -- a wrong
  definition the tests must tell from the right one."""
  x = np.asarray(v, dtype=np.float64)[k0:k1]
  w = np.asarray(w, dtype=np.float64)
  K, H = x.shape[0], w.size - 1
  if mutant == "h_minus":
    H -= 1
  fin = np.isfinite(x)
  allfin = bool(fin.all())
  num, den = np.zeros(x.shape), np.zeros(x.shape)
  reach = H if mutant == "reflect" else min(H, K - 1)
  offsets = range(-reach, reach + 1)
  if mutant == "descending":
    offsets = reversed(offsets)
  with np.errstate(all="ignore"):
    for d in offsets:
      if mutant == "reflect":  # (scipy's "reflect": .. 1 0 | 0 1 .. K-1 | K-1 K-2 ..)
        i = (np.arange(K) + d) % (2 * K)
        i = np.where(i < K, i, 2 * K - 1 - i)
        ja, xi, fi = slice(0, K), x[i], fin[i]
      else:
        ja = slice(max(0, -d), min(K, K - d))          # the j with 0 <= j + d < K
        ia = slice(ja.start + d, ja.stop + d)
        xi, fi = x[ia], fin[ia]
      wd = w[abs(d)]
      if allfin:  # (the same sums without the selections: what a large all-finite batch costs)
        num[ja] = num[ja] + wd * xi
        den[ja] = den[ja] + wd
        continue
      num[ja] = np.where(fi, num[ja] + wd * xi, num[ja])
      den[ja] = den[ja] + wd if mutant == "den_all" else np.where(fi, den[ja] + wd, den[ja])
    trend = num / den
    resid = np.where(fin, x - trend, NAN)
  return dict(trend=trend, resid=resid, nbad=(~fin).sum(axis=0).astype(np.int32))


# ------------------------------------------------------------------ the "gaussian" pipeline
def windows(v, k0, k1, W, S, Lg, sigma, truncate=4.0):
  """SeriesWindows(detrend="gaussian"): the smoother over [k0, k1), then the windows of the
  records [0, K) of its residual with their means removed (windows_cases.windows)."""
  resid = smooth(v, k0, k1, weights(sigma, truncate))["resid"]
  return WC.windows(resid, 0, k1 - k0, W, S, Lg, "constant")


def trend(v, k0, k1, W, S, Lg, sigma, truncate=4.0):
  """{"var" / "ac": (conc, disc, tie, nfin)} of the gaussian pipeline."""
  out = windows(v, k0, k1, W, S, Lg, sigma, truncate)["out"]
  return {key: WC.kendall(out[i], 0, out.shape[1]) for key, i in (("var", 2), ("ac", 3))}


def fit(v, k0, k1, sigma, truncate=4.0):
  """SeriesSurrogates(detrend="gaussian").fit: (var, ac) [nspec, n], the one-window "constant" fit
  of the residual."""
  resid = smooth(v, k0, k1, weights(sigma, truncate))["resid"]
  return SGC.fit(resid, 0, k1 - k0, "constant")


def significance(v, k0, k1, W, S, Lg, sigma, truncate, nsur, seed=0, ids=None, nb=None, sur=None):
  """SeriesWindows(detrend="gaussian").significance, as surrogate_cases.significance restates the
  other detrends: the observed trends and the fit from the residual, AR(1) surrogates of the
  residual, every chunk through the same smoother and then windows ("constant"), Kendall and the
  counting.  `sur` [K, nsur * nspec, n]: the surrogate series (before smoothing) to use instead of
  generating them."""
  v = np.asarray(v, dtype=np.float64)
  nspec, n = v.shape[1:]
  K = k1 - k0
  w = weights(sigma, truncate)
  ids = np.arange(n) if ids is None else ids
  resid = smooth(v, k0, k1, w)["resid"]
  obs = WC.windows(resid, 0, K, W, S, Lg, "constant")["out"]
  nwin = obs.shape[1]
  var, ac = SGC.fit(resid, 0, K, "constant") if sur is None else (None, None)
  acc = {key: [np.zeros((nspec, n), dtype=np.int32) for _ in range(3)] for key in ("var", "ac")}
  counts = {key: WC.kendall(obs[i], 0, nwin) for key, i in (("var", 2), ("ac", 3))}
  for b0, m in SGC.chunks(nsur, nb or nsur):
    if sur is None:
      y = SGC.surrogates(var, ac, K, b0, m, seed, ids)
    else:
      y = np.asarray(sur)[:, b0 * nspec:(b0 + m) * nspec]
    out = WC.windows(smooth(y, 0, K, w)["resid"], 0, K, W, S, Lg, "constant")["out"]
    for key, i in (("var", 2), ("ac", 3)):
      for a, add in zip(acc[key], SGC.exceed(counts[key], WC.kendall(out[i], 0, nwin))):
        a += add
  res = {}
  for key in ("var", "ac"):
    ge, le, nvalid = acc[key]
    t = SGC.tau(*counts[key][:3])
    none = np.isnan(t) | (nvalid == 0)
    with np.errstate(all="ignore"):
      pr = np.where(none, np.nan, (1.0 + ge) / (1.0 + nvalid))
      pf = np.where(none, np.nan, (1.0 + le) / (1.0 + nvalid))
    res[key] = dict(tau=t, ge=ge, le=le, nvalid=nvalid, p_rising=pr, p_falling=pf)
  return res


# ------------------------------------------------------------------ the case table
STYLES = WC.STYLES + ("allnan", "gap", "edge_nan")
FINITE_STYLES = WC.FINITE_STYLES
K0, AFTER = 3, 2
CHUNK_H, CHUNK = 80, 128  # the records one block takes at H = 80 (pm_series_smooth_geometry)

# n, nspec, K, sigma, truncate
GEOMETRIES = (
    (5, 2, 37, 2.0, 4.0),        # H 8: a ragged tile
    (70, 1, 64, 0.3, 4.0),       # H 1, the minimum; three tiles of 32
    (33, 3, 200, 20.0, 4.0),     # H 80: two chunks of 128 records
    (9, 2, 12, 10.0, 4.0),       # H 40 > K - 1: every reach is the whole window
    (4, 1, 4096, 1023.75, 4.0),  # H 4095, K 4096: both maxima (tiles of 2 members)
    (1, 1, 5, 1.0, 1.0),         # H 1
    (7, 2, CHUNK + 1, 20.0, 4.0),  # one record more than a block's chunk
    (7, 1, CHUNK, 20.0, 4.0),      # and exactly the chunk
    # the tiles of 16, 8 and 4 members
    (17, 1, 700, 75.0, 4.0),     # H 300
    (9, 1, 1300, 150.0, 4.0),    # H 600
    (5, 1, 2500, 300.0, 4.0),    # H 1200
    # blocks that ask for (nearly) all of a CU's LDS: K at least the rows one block stages
    (3, 1, 700, 43.25, 4.0),     # H 173, tiles of 32: 163 828 bytes
    (3, 1, 700, 55.0, 4.0),      # H 220, tiles of 32: 163 692
    (3, 1, 1300, 69.75, 4.0),    # H 279, tiles of 16
    (3, 1, 1300, 77.5, 4.0),     # H 310, tiles of 16: 163 836 of the 163 840
    (3, 1, 2500, 150.5, 4.0),    # H 602, tiles of 8: 163 836
    (3, 1, 4096, 1023.0, 4.0),   # H 4092, tiles of 4: 163 836
)
FULL_LDS = {173: 163828, 220: 163692, 310: 163836, 602: 163836, 4092: 163836}  # H: bytes at that K


def style_of(s, m, off=0):
  return STYLES[(m + 5 * s + off) % len(STYLES)]


def _series(rng, style, red, k0, K, H):
  """One (index, member) series of nrec records in the given style; its record window is
  [k0, k0 + K)."""
  if style == "allnan":    # den = 0 everywhere: the trend is 0 / 0
    return np.full(red.size, np.nan)
  W = min(7, K)
  x = WC._series(rng, style if style in WC.STYLES else "ar1", red, k0, W, 1, K - W + 1)
  if style == "gap":       # a run of NaN longer than 2 H + 1 (where K has room for one): the
    run = min(2 * H + 2, K - 2)  # trend is NaN in its middle, gap-filled near its ends
    x[k0 + 1:k0 + 1 + run] = np.nan
  if style == "edge_nan":  # the first and the last record
    x[k0] = x[k0 + K - 1] = np.nan
  return x


def case(n, nspec, K, sigma, truncate, seed=0):
  """A series [K0 + K + AFTER, nspec, n] with the record window [K0, K0 + K); NaN and 1e300 in the
  records before and behind it, which would change every result if they were read.  Member m of
  index s has the style STYLES[(m + 5 s + seed) % 12]."""
  rng = np.random.default_rng(9000 + 31 * K + seed)
  H = half_of(sigma, truncate)
  nrec = K0 + K + AFTER
  v = np.empty((nrec, nspec, n))
  a = rng.standard_normal((nspec, n))
  for k in range(nrec):
    a = 0.9 * a + np.sqrt(1.0 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = a
  for s in range(nspec):
    for m in range(n):
      v[:, s, m] = _series(rng, style_of(s, m, seed), v[:, s, m].copy(), K0, K, H)
  v[:K0] = np.nan
  v[1:K0:2] = 1e300
  v[K0 + K:] = 1e300
  v[K0 + K + 1::2] = np.nan
  return dict(name="n %d nspec %d K %d sigma %g truncate %g" % (n, nspec, K, sigma, truncate),
              v=v, k0=K0, k1=K0 + K, n=n, nspec=nspec, K=K, sigma=sigma, truncate=truncate, H=H,
              w=weights(sigma, truncate), off=seed)


def cases():
  return [case(*g, seed=i) for i, g in enumerate(GEOMETRIES)]


def restate(c, v=None, k0=None, k1=None):
  """The restatement of a case (or of another series or record window under the case's table)."""
  return smooth(c["v"] if v is None else v, c["k0"] if k0 is None else k0,
                c["k1"] if k1 is None else k1, c["w"])
