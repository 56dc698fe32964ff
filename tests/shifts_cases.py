"""The NumPy restatement of pm_series_shift_scan, pm_series_censor and pm_series_fit_ranged, of
SeriesShifts and of SeriesWindows.significance(until=), and the case tables (include/pymoc_hip.h
states the definitions).

The detector is defined on the mean and the var plane of pm_series_windows, so its restatement
starts from windows_cases.windows (window = L, step 1, "constant", lag 1); the ranged fit is ONE
window of that definition per member, of the member's own length.  Every NumPy product and sum is
an IEEE double operation rounded on its own, division and sqrt are IEEE: each double is the
device's bit for bit, the integers are exact.  Pure NumPy; nothing here imports the product."""
import numpy as np

import smooth_cases as SMC
import surrogate_cases as SGC
import windows_cases as WC

HALF_MAX = 2048
NAN = float("nan")


# ------------------------------------------------------------------ the three definitions
def planes(v, k0, k1, L, chunk=1 << 22):
  """(mean, var), each [nwin, nspec, n], nwin = K - L + 1: out[0] and out[2] of
  windows_cases.windows(v, k0, k1, L, 1, 1, "constant") -- taken a range of windows at a time
  (windows are independent), so that the [.., L] intermediate stays below `chunk` doubles."""
  v = np.asarray(v, dtype=np.float64)
  nwin = k1 - k0 - L + 1
  per = max(1, chunk // (L * v.shape[1] * v.shape[2]))
  mean, var = [], []
  for i0 in range(0, nwin, per):
    cnt = min(per, nwin - i0)
    out = WC.windows(v, k0 + i0, k0 + i0 + cnt - 1 + L, L, 1, 1, "constant")["out"]
    mean.append(out[0])
    var.append(out[2])
  return np.concatenate(mean), np.concatenate(var)


def scan(mean, var, L, thr, direction):
  """dict(at, first, ncand int32 [nspec, n]; val [4, nspec, n]: stat, jump, before, after at `at`;
  score, counts [ncand_max, nspec, n]) from the planes [nwin, nspec, n]; candidate c = L + i."""
  mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
  nwin, nspec, n = mean.shape
  nc = nwin - L  # c = L .. K - L, K = nwin + L - 1
  thr = np.asarray(thr, dtype=np.float64).reshape(nspec, 1)
  direction = np.asarray(direction).reshape(nspec, 1)
  before, after = mean[:nc], mean[L:L + nc]
  with np.errstate(all="ignore"):
    jump = after - before
    pooled = np.float64(0.5) * (var[:nc] + var[L:L + nc])
    stat = jump / np.sqrt(pooled)
    score = np.where(direction < 0, -stat, np.where(direction > 0, stat, np.fabs(stat)))
    counts = ~np.isnan(before) & ~np.isnan(after) & ~np.isnan(score)
    reach = counts & (score >= thr)
  at = np.full((nspec, n), -1, dtype=np.int32)
  first = np.full((nspec, n), -1, dtype=np.int32)
  val = np.full((4, nspec, n), NAN)
  for s in range(nspec):
    for m in range(n):
      idx = np.nonzero(counts[:, s, m])[0]
      if idx.size:
        sc = score[idx, s, m]
        i = idx[np.nonzero(sc == sc.max())[0][0]]  # the first of the largest (-0.0 == +0.0)
        at[s, m] = L + i
        val[:, s, m] = stat[i, s, m], jump[i, s, m], before[i, s, m], after[i, s, m]
      hit = np.nonzero(reach[:, s, m])[0]
      if hit.size:
        first[s, m] = L + hit[0]
  return dict(at=at, first=first, ncand=counts.sum(axis=0).astype(np.int32), val=val, score=score,
              counts=counts)


def detect(v, k0, k1, L, thr, direction):
  """SeriesShifts.detect: the planes, then the scan."""
  mean, var = planes(v, k0, k1, L)
  return scan(mean, var, L, thr, direction)


def ends(where, K, guard=0, src=None):
  """end [nspec, n] int32: w = where[src[s]][m]; end = K if w < 0 else max(0, w - guard) (at most
  K)."""
  where = np.asarray(where, dtype=np.int64)
  src = np.arange(where.shape[0]) if src is None else np.asarray(src)
  w = where[src]
  return np.where(w < 0, K, np.minimum(K, np.maximum(0, w - guard))).astype(np.int32)


def censor(x, where, guard=0, src=None, nb=1):
  """(y, end): y[j][i * nspec + s][m] = x[..] if j < end[s][m] else NaN, the kept values the very
  bits."""
  x = np.asarray(x, dtype=np.float64)
  K, planes_, n = x.shape
  nspec = planes_ // nb
  end = ends(where, K, guard, src)
  keep = np.arange(K)[:, None, None, None] < end[None, None]
  y = np.where(keep, x.reshape(K, nb, nspec, n).view(np.uint64), np.uint64(0x7ff8000000000000))
  return y.astype(np.uint64).view(np.float64).reshape(K, planes_, n), end


def stt_of(W):
  """W (W^2 - 1) / 12 exactly (a multiple of a half; windows_cases.stt_of floors it)."""
  return float(W * (W * W - 1)) / 12.0


def one_window(x, detrend):
  """(var, ac) of ONE window x [W, ...] at lag 1: the two passes of pm_series_windows, with the
  exact stt for every W; NaN where a record is not finite."""
  x = np.asarray(x, dtype=np.float64)
  W = x.shape[0]
  used = np.isfinite(x).all(axis=0)
  half = np.float64(0.5) * np.float64(W - 1)
  t = np.arange(W, dtype=np.float64) - half
  with np.errstate(all="ignore"):
    s, st = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for j in range(W):
      s = s + x[j]
      st = st + t[j] * x[j]
    mean = s / np.float64(W)
    slope = st / np.float64(stt_of(W))

    def resid(j):
      if detrend == "linear":
        return (x[j] - mean) - slope * t[j]
      return x[j] - mean if detrend == "constant" else x[j]

    q, c = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for j in range(W):
      r = resid(j)
      q = q + r * r
      if j < W - 1:
        c = c + r * resid(j + 1)
    var, ac = q / np.float64(W - 1), c / q
  return np.where(used, var, NAN), np.where(used, ac, NAN)


def fit_ranged(v, k0, k1, end, detrend):
  """(var, ac) [nspec, n]: per member the one-window fit over [k0, k0 + end[s][m]); NaN for an end
  below 4 or above K."""
  v = np.asarray(v, dtype=np.float64)
  end = np.asarray(end)
  var, ac = np.full(end.shape, NAN), np.full(end.shape, NAN)
  for e in np.unique(end):
    if WC.WIN_MIN <= e <= k1 - k0:
      sel = end == e
      var[sel], ac[sel] = one_window(v[k0:k0 + e][:, sel], detrend)
  return var, ac


# ------------------------------------------------------------------ the composition
def significance(v, k0, k1, W, S, Lg, detrend, nsur, end, seed=0, ids=None, nb=None, sur=None,
                 sigma=None, truncate=4.0):
  """SeriesWindows.significance(until=): `end` [nspec, n] the ends `until.censored()` left.  The
  observed series is the censored record window (under "gaussian" smoothed afterwards), the fit
  the ranged one (of its residual, "constant", under "gaussian"), and every surrogate is censored
  with the same ends before the record's own pipeline.  `sur` [K, nsur * nspec, n]: the surrogate
  series (before censoring) to use instead of generating them.  Returns surrogate_cases'
  dict, plus "fit": (var, ac)."""
  v = np.asarray(v, dtype=np.float64)
  nspec, n = v.shape[1:]
  K = k1 - k0
  where = np.where(end >= K, -1, end)  # (censor() by the ends themselves)
  gauss = detrend == "gaussian"
  w = SMC.weights(sigma, truncate) if gauss else None
  inner = "constant" if gauss else detrend

  def pipeline(y, nb_):
    y = censor(y, where, nb=nb_)[0]
    if gauss:
      y = SMC.smooth(y, 0, K, w)["resid"]
    return y, WC.windows(y, 0, K, W, S, Lg, inner)["out"]

  ids = np.arange(n) if ids is None else ids
  series, obs = pipeline(v[k0:k1], 1)
  nwin = obs.shape[1]
  var, ac = fit_ranged(series, 0, K, end, inner)
  acc = {key: [np.zeros((nspec, n), dtype=np.int32) for _ in range(3)] for key in ("var", "ac")}
  counts = {key: WC.kendall(obs[i], 0, nwin) for key, i in (("var", 2), ("ac", 3))}
  for b0, m in SGC.chunks(nsur, nb or nsur):
    if sur is None:
      y = SGC.surrogates(var, ac, K, b0, m, seed, ids)
    else:
      y = np.asarray(sur)[:, b0 * nspec:(b0 + m) * nspec]
    out = pipeline(y, m)[1]
    for key, i in (("var", 2), ("ac", 3)):
      for a, add in zip(acc[key], SGC.exceed(counts[key], WC.kendall(out[i], 0, nwin))):
        a += add
  res = dict(fit=(var, ac))
  for key in ("var", "ac"):
    ge, le, nvalid = acc[key]
    t = SGC.tau(*counts[key][:3])
    none = np.isnan(t) | (nvalid == 0)
    with np.errstate(all="ignore"):
      pr = np.where(none, np.nan, (1.0 + ge) / (1.0 + nvalid))
      pf = np.where(none, np.nan, (1.0 + le) / (1.0 + nvalid))
    res[key] = dict(tau=t, ge=ge, le=le, nvalid=nvalid, p_rising=pr, p_falling=pf)
  return res


# ------------------------------------------------------------------ the scan cases
STYLES = ("drop", "noise", "nan_some", "nan_all", "const", "stairs", "zeros", "alt", "rise", "inf1")
K0, AFTER = 3, 2
THR3, DIR3 = (3.0, 1e9, NAN), (-1, 0, 1)  # per index: reached, not reached, none; every dir


def style_of(s, m):
  return STYLES[(m + 3 * s) % len(STYLES)]


def _series(rng, style, K, L):
  """One series of K records (numbered from the record window's start)."""
  j = np.arange(K)
  x = rng.standard_normal(K)
  p = L + int(rng.integers(0, K - 2 * L + 1))  # a candidate
  if style == "drop":
    x[p:] -= 6.0
  elif style == "rise":
    x[p:] += 6.0
  elif style == "nan_some":  # window 0 alone holds record 0: candidate L is left out
    x[0] = NAN
    x[K // 2:] -= 4.0
  elif style == "nan_all":   # every L consecutive records hold one
    x[L - 1::L] = NAN
  elif style == "inf1":      # not finite: the windows that hold it have no mean
    x[p] = np.inf if rng.random() < 0.5 else -np.inf
  elif style == "const":     # jump 0 and pooled 0: every score NaN
    x[:] = 3.0
  elif style == "stairs":    # constant levels L records long: an infinite score at every step
    x[:] = -(j // L).astype(np.float64)
  elif style == "zeros":     # signed zeros: NaN scores again
    x[:] = np.where(j % 3 == 1, -0.0, 0.0)
  elif style == "alt":       # +1, -1, ..: every mean +0.0 (L even) over a positive variance, so
    x[:] = np.where(j % 2 == 0, 1.0, -1.0)  # every score is a zero: the first candidate wins
  return x


def case(K, L, n, nspec, seed=0, trail=0):
  """A series [K0 + K + AFTER, nspec, n] with the record window [K0, K0 + K); the records before
  and behind it are numbers that would change every result if they were read.  Member m of index
  s has the style STYLES[(m + 3 s) % 10]; thr and dir per index from THR3 and DIR3, rotated by
  `seed`."""
  rng = np.random.default_rng(9000 + 31 * K + L + seed)
  v = np.empty((K0 + K + AFTER, nspec, n))
  for s in range(nspec):
    for m in range(n):
      v[K0:K0 + K, s, m] = _series(rng, style_of(s, m + seed), K, L)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  thr = [THR3[(s + seed) % 3] for s in range(nspec)]
  direction = [DIR3[(s + seed) % 3] for s in range(nspec)]
  return dict(name="K %d L %d n %d nspec %d" % (K, L, n, nspec), v=v, k0=K0, k1=K0 + K, K=K, L=L,
              n=n, nspec=nspec, thr=np.array(thr), dir=np.array(direction, dtype=np.int32))


def cases():
  return [case(8, 4, 1, 1, 0), case(8, 4, 63, 3, 1), case(9, 4, 65, 1, 2), case(9, 4, 130, 3, 3),
          case(4096, 2048, 1, 1, 0), case(4096, 4, 130, 3, 4), case(300, 40, 65, 3, 5),
          case(301, 41, 63, 1, 7)]


def restate(c):
  return detect(c["v"], c["k0"], c["k1"], c["L"], c["thr"], c["dir"])


# ------------------------------------------------------------------ the censor and the fit cases
def censor_case(K, n, nspec, nb, seed=0):
  """x [K, nb * nspec, n] with non-finite values and NaN payloads among the kept records, and a
  `where` [nspec, n] that holds -1, 0, 1, K - 1, K and records between."""
  rng = np.random.default_rng(9500 + seed)
  x = rng.standard_normal((K, nb * nspec, n))
  bits = x.view(np.uint64)
  bits[rng.random(x.shape) < 0.05] = 0x7ff8dead0000beef   # a NaN with a payload
  bits[rng.random(x.shape) < 0.02] = 0xfff0000000000000   # -inf
  x[rng.random(x.shape) < 0.02] = -0.0
  where = rng.integers(-1, K + 1, size=(nspec, n)).astype(np.int32)
  special = [-1, 0, 1, K - 1, K, 2]
  where.ravel()[:len(special)] = special[:where.size]
  return dict(x=x, where=where, K=K, n=n, nspec=nspec, nb=nb)


def fit_case(K, n, nspec, seed=0):
  """A windows_cases series (every style, the non-finite ones too) with the record window [K0,
  K0 + K) and ends [nspec, n] mixing 0, 3, 4, K and records between; member (0, 1) holds a NaN at
  record 6 with end 10 (inside: no fit), member (0, 2) at record 12 with end 10 (outside)."""
  c = WC.case(K, 1, 1, 1, n, nspec, "linear", 60 + seed)
  rng = np.random.default_rng(9700 + seed)
  end = rng.integers(0, K + 1, size=(nspec, n)).astype(np.int32)
  special = [5, 6, 7, K - 1, 0, 3, 4, K][-end.size:]
  end.ravel()[-len(special):] = special
  v = c["v"]
  if n >= 3 and K >= 13:
    for m, rec in ((1, 6), (2, 12)):
      v[:, 0, m] = np.arange(v.shape[0]) * 0.5 + rng.standard_normal(v.shape[0])
      v[c["k0"] + rec, 0, m] = NAN
      end[0, m] = 10
  return dict(v=v, k0=c["k0"], k1=c["k1"], K=K, n=n, nspec=nspec, end=end)
