"""The NumPy restatement of pm_series_windows and pm_series_kendall, and the case tables.

The restatement follows include/pymoc_hip.h literally: per sliding window the two passes in
ascending j -- vectorised over windows, indices and members, every NumPy product and sum an IEEE
double operation rounded on its own -- and the pair counts of the trend by direct comparison.  It
is the authority the device results are compared with bit for bit.  Shared by
tests/test_windows_cpu.py (which pins it to an extended-precision evaluation, to
scipy.signal.detrend and to scipy.stats.kendalltau) and the GPU tests.
"""
import numpy as np

WIN_MIN, WIN_MAX, KENDALL_MAX = 4, 4096, 4096
NAN = float("nan")
DETRENDS = ("none", "constant", "linear")  # PM_WIN_DETREND_NONE, _CONSTANT, _LINEAR = 0, 1, 2


def nwin_of(K, W, S):
  return (K - W) // S + 1


def stt_of(W):
  return float(W * (W * W - 1) // 12)


def window_values(v, k0, k1, W, S):
  """x [nwin, nspec, n, W]: x[i, s, m, j] = v[k0 + i S + j, s, m]."""
  v = np.asarray(v, dtype=np.float64)
  nwin = nwin_of(k1 - k0, W, S)
  x = np.stack([v[k0 + i * S:k0 + i * S + W] for i in range(nwin)])  # [nwin, W, nspec, n]
  return np.moveaxis(x, 1, -1)


def windows(v, k0, k1, W, S, Lg, detrend):
  """dict(out [4, nwin, nspec, n] (mean, slope, var, ac), nused [nspec, n], used [nwin, nspec, n])
  of the series v [nrec, nspec, n]."""
  x = window_values(v, k0, k1, W, S)
  used = np.isfinite(x).all(axis=-1)
  half = np.float64(0.5) * np.float64(W - 1)
  t = np.arange(W, dtype=np.float64) - half
  lead = x.shape[:-1]
  with np.errstate(all="ignore"):
    s, st = np.zeros(lead), np.zeros(lead)
    for j in range(W):
      s = s + x[..., j]
      st = st + t[j] * x[..., j]
    mean = s / np.float64(W)
    slope = st / np.float64(stt_of(W)) if detrend == "linear" else np.zeros(lead)

    def resid(j):
      if detrend == "linear":
        return (x[..., j] - mean) - slope * t[j]
      if detrend == "constant":
        return x[..., j] - mean
      return x[..., j]

    q, c = np.zeros(lead), np.zeros(lead)
    for j in range(W):
      r = resid(j)
      q = q + r * r
      if j < W - Lg:
        c = c + r * resid(j + Lg)
    var = q / np.float64(W - 1)
    ac = c / q
  out = np.where(used[None], np.stack([mean, slope, var, ac]), NAN)
  return dict(out=out, nused=used.sum(axis=0).astype(np.int32), used=used)


def kendall(v, k0, k1):
  """(conc, disc, tie, nfin) int32 [nspec, n] of the records [k0, k1) of v [nrec, nspec, n]."""
  w = np.asarray(v, dtype=np.float64)[k0:k1]
  K = w.shape[0]
  fin = np.isfinite(w)
  conc, disc, tie = (np.zeros(w.shape[1:], dtype=np.int64) for _ in range(3))
  for a in range(K - 1):
    both = fin[a + 1:] & fin[a]
    with np.errstate(invalid="ignore"):
      conc += (both & (w[a + 1:] > w[a])).sum(axis=0)
      disc += (both & (w[a + 1:] < w[a])).sum(axis=0)
      tie += (both & (w[a + 1:] == w[a])).sum(axis=0)
  return tuple(a.astype(np.int32) for a in (conc, disc, tie, fin.sum(axis=0)))


def tau_b(conc, disc, tie):
  """(conc - disc) / sqrt(n0 (n0 - tie)), n0 = conc + disc + tie, in float64; NaN for n0 == tie."""
  conc, disc, tie = (np.asarray(a, dtype=np.float64) for a in (conc, disc, tie))
  n0 = conc + disc + tie
  with np.errstate(all="ignore"):
    return (conc - disc) / np.sqrt(n0 * (n0 - tie))


# ------------------------------------------------------------------ the case table
STYLES = ("ar1", "ramp", "const", "big", "small", "zeros", "nan1", "inf1", "spoiled")
FINITE_STYLES = STYLES[:6]
K0, AFTER = 3, 2


def style_of(s, m):
  return STYLES[(m + 3 * s) % len(STYLES)]


def _series(rng, style, red, k0, W, S, nwin):
  """One (index, member) series in the given style, from its AR(1) noise (variance 1); its record
  window starts at k0."""
  nrec = red.size
  t = np.arange(nrec) - k0
  if style == "ramp":   # an exact linear ramp (quarters: every value and partial sum is exact)
    return 2.0 + 0.25 * t
  if style == "const":  # q == 0 once a mean is removed: var +0.0, ac NaN
    return np.full(nrec, 3.0)
  if style == "big":    # (without an offset: the square of a sum of 4096 offsets would overflow)
    return red * 1e150
  if style == "small":
    return red * 1e-150
  if style == "zeros":  # signed zeros: q == 0 with and without detrending
    return np.where(np.arange(nrec) % 3 == 1, -0.0, 0.0)
  x = (15.0 if style != "ar1" else 1e3 * (W % 2)) + red  # AR(1) on an offset
  if style == "nan1":   # the first record of the record window lies in window 0 alone
    x[k0] = np.nan
  if style == "inf1":   # the last record of the last window lies in that window alone
    x[k0 + (nwin - 1) * S + W - 1] = np.inf if rng.random() < 0.5 else -np.inf
  if style == "spoiled":  # every W consecutive records hold one of these
    x[(t % W) == W - 1] = np.nan
  return x


def case(W, S, nwin, Lg, n, nspec, detrend, seed=0):
  """A series [K0 + K + AFTER, nspec, n]: the record window [K0, K0 + K) holds nwin whole windows
  and a tail of min(S - 1, 3) records that fits none; the records before and behind it are numbers
  that would change every result if they were read.  Member m of index s has the style
  STYLES[(m + 3 s) % 9]."""
  rng = np.random.default_rng(4000 + 17 * W + seed)
  tail = min(S - 1, 3)
  K = W + (nwin - 1) * S + tail
  nrec = K0 + K + AFTER
  v = np.empty((nrec, nspec, n))
  a = rng.standard_normal((nspec, n))
  for k in range(nrec):
    a = 0.9 * a + np.sqrt(1.0 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = a
  for s in range(nspec):
    for m in range(n):
      v[:, s, m] = _series(rng, style_of(s, m), v[:, s, m].copy(), K0, W, S, nwin)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  return dict(name="W %d S %d nwin %d lag %d n %d nspec %d %s" % (W, S, nwin, Lg, n, nspec, detrend),
              v=v, k0=K0, k1=K0 + K, W=W, S=S, nwin=nwin, Lg=Lg, detrend=detrend)


MANY = 300  # windows of the case that gives a block more windows than it takes (W 64, S 1: 256)
LONG = 400  # and of the one whose blocks stage nearly a whole CU's LDS (W 257, S 1: 624 records)


def cases():
  return [
      case(4, 1, 5, 1, 7, 3, "linear", 1),
      case(4, 2, 2, 2, 65, 3, "constant", 2),
      case(4, 4, 1, 1, 1, 1, "none", 3),
      case(5, 1, 2, 3, 64, 3, "linear", 4),
      case(5, 2, 5, 1, 65, 1, "none", 5),
      case(5, 5, 5, 3, 7, 3, "constant", 6),
      case(64, 1, MANY, 1, 7, 3, "linear", 7),
      case(64, 32, 5, 3, 65, 3, "constant", 8),
      case(64, 64, 2, 62, 64, 1, "linear", 9),
      case(65, 1, 5, 63, 65, 3, "none", 10),
      case(65, 33, 2, 1, 7, 3, "linear", 11),
      case(65, 65, 5, 3, 64, 3, "constant", 12),
      case(257, 1, 2, 3, 65, 3, "linear", 13),
      case(257, 128, 5, 255, 7, 3, "none", 14),
      case(257, 257, 1, 1, 65, 1, "constant", 15),
      case(4096, 1, 5, 1, 7, 3, "linear", 16),
      case(4096, 2048, 2, 4094, 65, 1, "constant", 17),
      case(4096, 4096, 2, 3, 1, 3, "linear", 18),
      # the tiles of 16 and of 8 members, and the largest tile of 32
      case(1024, 1, 2, 3, 7, 3, "linear", 19),
      case(2048, 1, 2, 1, 7, 1, "none", 20),
      case(257, 1, LONG, 1, 7, 1, "constant", 21),
  ]


def restate(c, v=None):
  """The restatement of a case (or of another series under the case's settings)."""
  return windows(c["v"] if v is None else v, c["k0"], c["k1"], c["W"], c["S"], c["Lg"],
                 c["detrend"])


# ------------------------------------------------------------------ the Kendall cases
K_STYLES = ("noise", "ties", "holes", "equal", "rising", "none")


def k_style_of(s, m):
  return K_STYLES[(m + 2 * s) % len(K_STYLES)]


def kendall_case(K, n, nspec, seed=0):
  """A series [K0 + K + AFTER, nspec, n], record window [K0, K0 + K).  Member m of index s:
    noise   distinct values;  ties: values rounded to a few levels;  holes: NaN and +-inf
    sprinkled into tied values;  equal: one value throughout;  rising: strictly increasing
    (tau = 1);  none: no finite record."""
  rng = np.random.default_rng(5000 + 13 * K + seed)
  nrec = K0 + K + AFTER
  v = rng.standard_normal((nrec, nspec, n))
  for s in range(nspec):
    for m in range(n):
      st, x = k_style_of(s, m), v[:, s, m]
      if st == "ties":
        x[:] = np.round(2.0 * x) * 0.5 + 0.0
      elif st == "holes":
        x[:] = np.round(3.0 * x)
        bad = rng.random(nrec) < 0.2
        x[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
      elif st == "equal":
        x[:] = -0.0 if m % 2 else 2.5
      elif st == "rising":
        x[:] = np.cumsum(rng.uniform(0.1, 1.0, size=nrec))
      elif st == "none":
        x[:] = rng.choice([np.nan, np.inf, -np.inf], size=nrec)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  return dict(name="K %d n %d nspec %d" % (K, n, nspec), v=v, k0=K0, k1=K0 + K)


def kendall_cases():
  return [kendall_case(1, 7, 3, 1), kendall_case(2, 65, 1, 2), kendall_case(64, 64, 3, 3),
          kendall_case(65, 65, 3, 4), kendall_case(300, 7, 3, 5), kendall_case(300, 1, 1, 6),
          # the tiles of 8 and of 4 members; 4096 records: 128 KiB of LDS, counts near 2^23
          kendall_case(1000, 9, 1, 7), kendall_case(4096, 6, 1, 8)]
