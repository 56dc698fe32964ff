"""The NumPy restatement of pm_series_surrogates, pm_series_exceed and of the whole of
SeriesWindows.significance, and the case table (include/pymoc_hip.h states the definitions).

The deviate is tests/noise_cases.py: deviate -- the one host restatement of it -- called with the
counter packing of the header: xi_j = xi(seed, id, b, (s << 12) | j).  Windows and Kendall counts
come from tests/windows_cases.py.  Every NumPy product and sum is an IEEE double operation rounded
on its own, so with the deviates given the series is the device's bit for bit; the counts are exact
integers.  Pure NumPy; nothing here imports the product."""
import numpy as np

import noise_cases as NC
import windows_cases as WC

K_MAX, PLANES_MAX = 4096, 65535


def deviates(K, b0, nb, nspec, seed, ids):
  """(xi, R), each [K, nb * nspec, n], of the surrogates b0 .. b0 + nb - 1: plane i * nspec + s; R
  the radius the deviate's tolerance is stated in."""
  ids = np.asarray(ids, dtype=np.uint64)
  b = np.arange(b0, b0 + nb, dtype=np.uint64)
  xi, R = np.empty((K, nb, nspec, ids.size)), np.empty((K, nb, nspec, ids.size))
  for s in range(nspec):
    for j in range(K):  # (noise_cases takes the last counter word as one integer)
      xi[j, :, s, :], R[j, :, s, :] = NC.deviate(seed, ids[None, :], b[:, None], (s << 12) | j)
  return xi.reshape(K, nb * nspec, ids.size), R.reshape(K, nb * nspec, ids.size)


def surrogates(var, ac, K, b0, nb, seed, ids, xi=None):
  """y [K, nb * nspec, n] from the fit values var, ac [nspec, n]; `xi` [K, nb * nspec, n]: the
  deviates to use instead of noise_cases.deviate's."""
  var, ac = np.asarray(var, dtype=np.float64), np.asarray(ac, dtype=np.float64)
  nspec, n = var.shape
  if xi is None:
    xi = deviates(K, b0, nb, nspec, seed, ids)[0]
  xi = np.asarray(xi, dtype=np.float64).reshape(K, nb, nspec, n)
  with np.errstate(all="ignore"):
    phi, sd = ac, np.sqrt(var)
    g = sd * np.sqrt(np.fmax(0.0, 1.0 - phi * phi))
    ok = np.isfinite(phi) & np.isfinite(sd)
    y = np.empty((K, nb, nspec, n))
    y[0] = sd * xi[0]
    for j in range(1, K):
      y[j] = phi * y[j - 1] + g * xi[j]
  return np.where(ok, y, np.nan).reshape(K, nb * nspec, n)


def tau(c, d, t):
  """(double)(c - d) / sqrt((double)n0 * (double)(n0 - t)), n0 = c + d + t; NaN for n0 == t."""
  c, d, t = (np.asarray(a, dtype=np.int64) for a in (c, d, t))
  n0 = c + d + t
  with np.errstate(all="ignore"):
    return (c - d).astype(np.float64) / np.sqrt(n0.astype(np.float64) * (n0 - t).astype(np.float64))


def exceed(obs, sur):
  """(ge, le, nvalid) int32 [nspec, n] that one call adds: obs = (conc, disc, tie) [nspec, n],
  sur = (conc, disc, tie) [nb * nspec, n]."""
  to = tau(*obs[:3])
  nspec, n = to.shape
  ts = tau(*sur[:3]).reshape(-1, nspec, n)
  live = ~np.isnan(to)
  with np.errstate(invalid="ignore"):
    ge = ((ts >= to) & live).sum(axis=0)
    le = ((ts <= to) & live).sum(axis=0)
  nvalid = (~np.isnan(ts) & live).sum(axis=0)
  return tuple(a.astype(np.int32) for a in (ge, le, nvalid))


def fit(v, k0, k1, detrend):
  """(var, ac) [nspec, n]: one window over the whole record window, lag 1.  (windows_cases.stt_of
  floors W (W^2 - 1) / 12, which ends in .5 for W = 2 mod 4: its linear slope is not the
  definition's there, so such a K is refused here, not restated wrongly.)"""
  K = k1 - k0
  assert detrend != "linear" or K % 4 != 2, "windows_cases restates no linear fit of K = 2 mod 4"
  out = WC.windows(v, k0, k1, K, 1, 1, detrend)["out"]
  return out[2, 0], out[3, 0]


def chunks(nsur, nb):
  return [(b0, min(nb, nsur - b0)) for b0 in range(0, nsur, nb)]


def significance(v, k0, k1, W, S, Lg, detrend, nsur, seed=0, ids=None, nb=None, sur=None):
  """The whole pipeline on the series v [nrec, nspec, n]: {"var" / "ac": dict(tau, ge, le, nvalid,
  p_rising, p_falling), each [nspec, n]}.  `ids`: the global member numbers (default 0 .. n - 1);
  `nb`: the surrogates of a chunk (default all at once); `sur` [K, nsur * nspec, n]: the surrogate
  series to use instead of generating them."""
  v = np.asarray(v, dtype=np.float64)
  nspec, n = v.shape[1:]
  K = k1 - k0
  ids = np.arange(n) if ids is None else ids
  obs = WC.windows(v, k0, k1, W, S, Lg, detrend)["out"]
  nwin = obs.shape[1]
  var, ac = fit(v, k0, k1, detrend) if sur is None else (None, None)
  res = {}
  acc = {key: [np.zeros((nspec, n), dtype=np.int32) for _ in range(3)] for key in ("var", "ac")}
  counts = {key: WC.kendall(obs[i], 0, nwin) for key, i in (("var", 2), ("ac", 3))}
  for b0, m in chunks(nsur, nb or nsur):
    if sur is None:
      y = surrogates(var, ac, K, b0, m, seed, ids)
    else:
      y = np.asarray(sur)[:, b0 * nspec:(b0 + m) * nspec]
    w = WC.windows(y, 0, K, W, S, Lg, detrend)["out"]
    for key, i in (("var", 2), ("ac", 3)):
      for a, add in zip(acc[key], exceed(counts[key], WC.kendall(w[i], 0, nwin))):
        a += add
  for key in ("var", "ac"):
    ge, le, nvalid = acc[key]
    t = tau(*counts[key][:3])
    none = np.isnan(t) | (nvalid == 0)
    with np.errstate(all="ignore"):
      pr = np.where(none, np.nan, (1.0 + ge) / (1.0 + nvalid))
      pf = np.where(none, np.nan, (1.0 + le) / (1.0 + nvalid))
    res[key] = dict(tau=t, ge=ge, le=le, nvalid=nvalid, p_rising=pr, p_falling=pf)
  return res


# ------------------------------------------------------------------ the case table
GEOMETRIES = ((5, 2, 37, 3), (70, 1, 64, 2), (33, 3, 9, 1), (4, 1, 4096, 2))  # n, nspec, K, nb
B0S = (0, 5)
MEMBER0S = (0, 2**32 - 3)  # the second: the id carries into the high word inside the batch
# (phi, var): what the table's first series hold, in this order; the others are drawn
SPECIAL = ((0.0, 1.0), (-0.7, 2.5), (1.0, 1.0), (-1.0, 4.0), (np.nan, 1.0), (0.5, 0.0),
           (0.5, np.inf), (0.3, np.nan), (np.inf, 1.0), (0.9, 1e300), (0.9, 1e-300))
NAN_SERIES = (4, 6, 7, 8)  # of SPECIAL: phi or sqrt(var) not finite


def fit_values(n, nspec, seed):
  """(var, ac) [nspec, n]: flat series q = s * n + m holds SPECIAL[q] while they last, then
  phi uniform in (-0.95, 0.95) and var log-uniform over six decades."""
  rng = np.random.default_rng(7100 + seed)
  ac = rng.uniform(-0.95, 0.95, size=nspec * n)
  var = 10.0 ** rng.uniform(-3, 3, size=nspec * n)
  for q, (p, v) in enumerate(SPECIAL[:nspec * n]):
    ac[q], var[q] = p, v
  return var.reshape(nspec, n), ac.reshape(nspec, n)


def cases():
  out = []
  for gi, (n, nspec, K, nb) in enumerate(GEOMETRIES):
    b0, member0 = B0S[gi % 2], MEMBER0S[(gi // 2) % 2]
    var, ac = fit_values(n, nspec, gi)
    out.append(dict(name="n %d nspec %d K %d nb %d b0 %d member0 %d" % (n, nspec, K, nb, b0, member0),
                    n=n, nspec=nspec, K=K, nb=nb, b0=b0, member0=member0, seed=0x9E3779B97F4A7C15 + gi,
                    var=var, ac=ac))
  # both b0 and both member0 at the geometry with the most special series
  n, nspec, K, nb = GEOMETRIES[0]
  var, ac = fit_values(n, nspec, 0)
  out.append(dict(name="n 5 nspec 2 K 37 nb 3 b0 5 member0 %d" % MEMBER0S[1], n=n, nspec=nspec, K=K,
                  nb=nb, b0=5, member0=MEMBER0S[1], seed=3, var=var, ac=ac))
  return out


def exceed_case():
  """Constructed counts: obs (conc, disc, tie) [2, 6] and sur [4 * 2, 6].  Observed column by
  column: 1/3 as (2, 1, 0); 1/3 as (4, 2, 0); ties (3, 1, 2); n0 == tie (0, 0, 6): NaN; no pair
  (0, 0, 0): NaN; -1 as (0, 10, 0).  The surrogates hold equal taus from other counts, ties,
  n0 == tie and taus either side."""
  obs_row = [(2, 1, 0), (4, 2, 0), (3, 1, 2), (0, 0, 6), (0, 0, 0), (0, 10, 0)]
  sur_rows = [
      [(4, 2, 0), (2, 1, 0), (6, 2, 4), (1, 0, 0), (1, 0, 0), (0, 3, 0)],
      [(0, 0, 3), (0, 0, 0), (2, 2, 0), (0, 0, 3), (2, 1, 0), (0, 0, 1)],
      [(1, 2, 0), (3, 0, 0), (3, 1, 1), (0, 1, 0), (0, 0, 0), (1, 9, 0)],
      [(6, 3, 0), (8, 4, 3), (1, 3, 2), (5, 5, 0), (3, 3, 3), (0, 0, 0)],
  ]
  obs = np.array([obs_row, obs_row[::-1]], dtype=np.int32)             # [2, 6, 3]
  sur = np.array([[r, r[::-1]] for r in sur_rows], dtype=np.int32)     # [4, 2, 6, 3]
  sur[1, 1], sur[2, 1] = sur[2, 1].copy(), sur[1, 1].copy()            # (index 1: another order)
  return (tuple(np.ascontiguousarray(obs[..., i]) for i in range(3)),
          tuple(np.ascontiguousarray(sur[..., i].reshape(8, 6)) for i in range(3)))
