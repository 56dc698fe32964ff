"""The NumPy restatement of pm_series_dfa, its forward bounds, and the case table.

The restatement follows include/pymoc_hip.h literally: per sliding window pass 1 of
pm_series_windows, then per scale the profile box by box, pass A and pass B of every box in
ascending record order -- loops over records, vectorised over windows, indices and members, every
NumPy product, sum and quotient an IEEE operation of the array's type rounded on its own.  In
float64 it is the authority the device's F2 is compared with bit for bit; in np.longdouble it is
the reference of the forward bound (`f2_bound`).  alpha goes through a
logarithm, so it is compared within `alpha_bound` of `alpha_of` in np.longdouble.  Shared by
tests/test_dfa_cpu.py and the GPU tests.  Pure NumPy; nothing here imports the product.
"""
import numpy as np

import windows_cases as WC

SCALES_MAX, SCALE_MIN = 16, 4
NAN = float("nan")
U = 2.0 ** -53
DETRENDS = WC.DETRENDS


def stt_of(W):
  """W (W^2 - 1) / 12: exact (a multiple of a half)."""
  return float(W * (W * W - 1)) / 12.0


def suu_of(s):
  return float(s * (s * s - 1)) / 12.0


def weights_of(scales):
  """The table of nq doubles the entry takes: w_q = 0.5 (L_q - Lbar) / sum (L_q - Lbar)^2."""
  L = np.log(np.asarray(scales, dtype=np.float64))
  dev = L - L.mean()
  return 0.5 * dev / (dev * dev).sum()


def default_scales(W):
  """The definition of pymoc_amd.dfa.default_scales, restated."""
  if W < 32:
    return (4, W // 4)
  return tuple(sorted({min(int(round(4.0 * (W / 16.0) ** (i / 7.0))), W // 4) for i in range(8)}))


def dfa(v, k0, k1, W, S, detrend, scales, dtype=np.float64, weights=None):
  """dict(f2 [nq, nwin, nspec, n], alpha [nwin, nspec, n], used [nwin, nspec, n], ymax, xdev, xmax
  [nq or 1, nwin, nspec, n]) of the series v [nrec, nspec, n], every operation in `dtype`.  ymax =
  max |y_j| over the boxes of a scale, xdev = max |x_j - mean|, xmax = max |x_j|: what `f2_bound`
  is stated in."""
  T = dtype
  x = WC.window_values(v, k0, k1, W, S)
  used = np.isfinite(x).all(axis=-1)
  x = x.astype(T)
  half = T(0.5) * T(W - 1)
  t = np.arange(W).astype(T) - half
  lead = x.shape[:-1]
  f2, ymax = [], []
  with np.errstate(all="ignore"):
    s_, st = np.zeros(lead, dtype=T), np.zeros(lead, dtype=T)
    for j in range(W):
      s_ = s_ + x[..., j]
      st = st + t[j] * x[..., j]
    mean = s_ / T(W)
    slope = st / T(stt_of(W)) if detrend == "linear" else np.zeros(lead, dtype=T)

    def d(j):
      if detrend == "linear":
        return (x[..., j] - mean) - slope * t[j]
      return x[..., j] - mean  # "constant", and "none": the profile is the mean-removed series'

    for s in scales:
      nb, suu, ds = W // s, T(suu_of(s)), T(s)
      u = np.arange(s).astype(T) - T(0.5) * T(s - 1)
      y, f, ym = np.zeros(lead, dtype=T), np.zeros(lead, dtype=T), np.zeros(lead, dtype=T)
      for b in range(nb):
        y0 = y
        sy, su = np.zeros(lead, dtype=T), np.zeros(lead, dtype=T)
        for i in range(s):
          y = y + d(b * s + i)
          sy = sy + y
          su = su + u[i] * y
          ym = np.fmax(ym, np.abs(y))
        a, c = sy / ds, su / suu
        y = y0
        for i in range(s):
          y = y + d(b * s + i)
          e = (y - a) - c * u[i]
          f = f + e * e
      f2.append(f / T(nb * s))
      ymax.append(ym)
    f2 = np.where(used[None], np.stack(f2), T(NAN))
    alpha = alpha_of(f2, scales, dtype=T, weights=weights)
    xdev = np.abs(x - mean[..., None]).max(axis=-1)
    xmax = np.abs(x).max(axis=-1)
  return dict(f2=f2, alpha=alpha, used=used, ymax=np.stack(ymax), xdev=xdev[None], xmax=xmax[None])


def alpha_of(f2, scales, dtype=np.float64, weights=None):
  """alpha = sum_q w_q * log(F2_q), sequential in q from +0.0, in `dtype`, from f2 [nq, ...]; NaN
  unless every F2_q is finite and > 0.  The weights are the float64 table."""
  w = weights_of(scales) if weights is None else np.asarray(weights, dtype=np.float64)
  f2 = np.asarray(f2)
  with np.errstate(all="ignore"):
    ok = (np.isfinite(f2) & (f2 > 0)).all(axis=0)
    al = np.zeros(f2.shape[1:], dtype=dtype)
    for q in range(len(scales)):
      al = al + dtype(w[q]) * np.log(f2[q].astype(dtype))
  return np.where(ok, al, dtype(NAN))


def alpha_terms(f2, scales, weights=None):
  """sum_q |w_q ln F2_q| (float64), what `alpha_bound` scales with."""
  w = weights_of(scales) if weights is None else np.asarray(weights, dtype=np.float64)
  with np.errstate(all="ignore"):
    return sum(np.abs(w[q] * np.log(np.asarray(f2[q], dtype=np.float64)))
               for q in range(len(scales)))


def alpha_c(nq):
  """c(nq) of the alpha bound c(nq) 2^-53 sum_q |w_q ln F2_q|: the device
  library's fp64 log is documented to 1 ulp, at most 2 * 2^-53 relative; the product w_q * log adds
  one rounding, 2^-53; a term then goes through at most nq - 1 roundings of the sequential sum
  (0.0 + the first term is exact); and 1 more covers the second-order terms and the 2^-64 roundings
  of the np.longdouble reference.  2 + 1 + (nq - 1) + 1 = nq + 3."""
  return nq + 3


def alpha_bound(f2, scales, weights=None):
  return alpha_c(len(scales)) * U * alpha_terms(f2, scales, weights)


def f2_bound(r, W, scales, detrend):
  """The forward bound on |F2_q(float64) - F2_q(exact)| of DESIGN.md section 27, [nq, ...], from the
  float64 restatement's result r (its f2, ymax, xdev, xmax).  With Y = ymax, X' = xdev, X = xmax,
  u = 2^-53, to first order in u:
    de  = u [(10.5 W + 2.5 s + 11) Y + LINEAR (14 W X' + s^2 X / 3)]       (the error of a residual e)
    |dF2| <= 2 sqrt(F2) de + de^2 + (nb s + 2) u F2."""
  lin = 1.0 if detrend == "linear" else 0.0
  out = []
  with np.errstate(all="ignore"):
    for q, s in enumerate(scales):
      Y, Xd, X = r["ymax"][q], r["xdev"][0], r["xmax"][0]
      de = U * ((10.5 * W + 2.5 * s + 11.0) * Y + lin * (14.0 * W * Xd + s * s * X / 3.0))
      F = np.asarray(r["f2"][q], dtype=np.float64)
      out.append(2.0 * np.sqrt(F) * de + de * de + ((W // s) * s + 2.0) * U * F)
  return np.stack(out)


def dfa_fast(v, k0, k1, W, S, detrend, scales):
  """An independent vectorised evaluation of the same quantity (f2 [nq, nwin, nspec, n], float64):
  np.cumsum for the profile, a reshape into boxes, the normal equations of the line per box.  Not
  the definition's operation order: it agrees within rounding (`f2_bound`), not bit for bit.  Also
  the host route the example times."""
  x = WC.window_values(v, k0, k1, W, S)
  used = np.isfinite(x).all(axis=-1)
  t = np.arange(W) - 0.5 * (W - 1)
  with np.errstate(all="ignore"):
    r = x - x.mean(axis=-1, keepdims=True)
    if detrend == "linear":
      r = r - ((r * t).sum(axis=-1) / (t * t).sum())[..., None] * t
    y = np.cumsum(r, axis=-1)
    out = []
    for s in scales:
      nb = W // s
      z = y[..., :nb * s].reshape(y.shape[:-1] + (nb, s))
      u = np.arange(s) - 0.5 * (s - 1)
      a = z.mean(axis=-1, keepdims=True)
      c = ((z * u).sum(axis=-1) / (u * u).sum())[..., None]
      e = z - a - c * u
      out.append((e * e).sum(axis=(-1, -2)) / (nb * s))
  return np.where(used[None], np.stack(out), NAN)


# ------------------------------------------------------------------ the case table
# offset: 1e6 + AR(1), which matters under "none"; huge: AR(1) * 1e154, whose squared residuals
# overflow (inf in F2, NaN in alpha), which `big` (1e150) does not reach here
STYLES = WC.STYLES + ("offset", "huge")
K0, AFTER = WC.K0, WC.AFTER


def style_of(s, m):
  return STYLES[(m + 3 * s) % len(STYLES)]


def case(W, S, nwin, n, nspec, detrend, scales, seed=0):
  """As windows_cases.case: a series [K0 + K + AFTER, nspec, n] whose record window [K0, K0 + K)
  holds nwin whole windows and a tail of min(S - 1, 3) records that fits none, between records that
  would change every result if they were read.  Member m of index s has the style
  STYLES[(m + 3 s) % 11]."""
  rng = np.random.default_rng(7000 + 17 * W + seed)
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
      style = style_of(s, m)
      if style == "offset":
        v[:, s, m] = 1e6 + v[:, s, m]
      elif style == "huge":
        v[:, s, m] = 1e154 * v[:, s, m]
      else:
        v[:, s, m] = WC._series(rng, style, v[:, s, m].copy(), K0, W, S, nwin)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  scales = tuple(scales)
  return dict(name="W %d S %d nwin %d n %d nspec %d %s scales %d..%d (%d)"
              % (W, S, nwin, n, nspec, detrend, scales[0], scales[-1], len(scales)),
              v=v, k0=K0, k1=K0 + K, W=W, S=S, nwin=nwin, detrend=detrend, scales=scales)


MANY = 300  # windows of the case whose second chunk is partial (W 20, S 1: a block takes 288)


def cases():
  """The smallest shapes at which the kernel can go wrong, each geometry under the three detrends
  unless said: the minimum W = 20; a trailing record in no box (W 21: one at both scales; W 23:
  three and three); 16 scales; s_max = W / 4 exactly; the default scales of W = 256; one window of
  4096 records with the largest box (the tile of 4 members); S = 1, 3 and W; a full and a partial
  chunk of windows; n = 1, 33, 37; nspec = 1 and 3; k0 = 3 with records behind k1 (every case)."""
  out, seed = [], 0
  for det in DETRENDS:
    for W, S, nwin, n, nspec, scales in (
        (20, 1, 5, 37, 3, (4, 5)),
        (21, 3, 4, 33, 1, (4, 5)),
        (23, 23, 3, 1, 3, (4, 5)),
        (76, 1, 3, 37, 1, tuple(range(4, 20))),
        (64, 3, 4, 33, 3, (4, 16)),
        (256, 8, 4, 37, 3, default_scales(256))):
      seed += 1
      out.append(case(W, S, nwin, n, nspec, det, scales, seed))
  out.append(case(20, 1, MANY, 37, 1, "linear", (4, 5), 40))
  out.append(case(4096, 4096, 1, 11, 1, "linear", (4, 1024), 41))
  return out


def restate(c, v=None, **kw):
  """The restatement of a case (or of another series under the case's settings)."""
  return dfa(c["v"] if v is None else v, c["k0"], c["k1"], c["W"], c["S"], c["detrend"],
             c["scales"], **kw)


# ------------------------------------------------------------------ the restated surrogate test
def significance(v, k0, k1, W, S, detrend, scales, nsur, seed=0, nb=None, sur=None):
  """surrogate_cases.significance for the third indicator: dict(tau, ge, le, nvalid, p_rising,
  p_falling), each [nspec, n], of the trend of the restated alpha series; AR(1) surrogates of the
  restated fit unless `sur` [K, nsur * nspec, n] gives the surrogate series."""
  import surrogate_cases as SGC
  v = np.asarray(v, dtype=np.float64)
  nspec, n = v.shape[1:]
  K = k1 - k0
  obs = dfa(v, k0, k1, W, S, detrend, scales)["alpha"]
  nwin = obs.shape[0]
  var, ac = SGC.fit(v, k0, k1, detrend) if sur is None else (None, None)
  counts = WC.kendall(obs, 0, nwin)
  acc = [np.zeros((nspec, n), dtype=np.int32) for _ in range(3)]
  for b0, m in SGC.chunks(nsur, nb or nsur):
    if sur is None:
      y = SGC.surrogates(var, ac, K, b0, m, seed, np.arange(n))
    else:
      y = np.asarray(sur)[:, b0 * nspec:(b0 + m) * nspec]
    al = dfa(y, 0, K, W, S, detrend, scales)["alpha"]
    for a, add in zip(acc, SGC.exceed(counts, WC.kendall(al, 0, nwin))):
      a += add
  return of_counts(counts, acc)


def of_counts(counts, acc):
  """The result dict from the observed counts and the accumulated (ge, le, nvalid)."""
  import surrogate_cases as SGC
  ge, le, nvalid = acc
  t = SGC.tau(*counts[:3])
  none = np.isnan(t) | (nvalid == 0)
  with np.errstate(all="ignore"):
    pr = np.where(none, np.nan, (1.0 + ge) / (1.0 + nvalid))
    pf = np.where(none, np.nan, (1.0 + le) / (1.0 + nvalid))
  return dict(tau=t, ge=ge, le=le, nvalid=nvalid, p_rising=pr, p_falling=pf)
