"""The NumPy restatement of pm_series_fourier_coef, pm_series_surrogates_fourier and of
SeriesWindows.significance(method="fourier"), and the case table (include/pymoc_hip.h states the
definitions).

The restatement follows the header literally on the tables of pymoc_amd.fourier -- the very
arrays the device reads: the pass-1 sums and the residual of ONE window of K records, Bluestein's
chirp-z (BLU) with the iterative radix-2 decimation-in-time transform of spectra_cases.fft_dit
carried to a complex input, the Philox phase index from the words of noise_cases, the rotation,
the inverse BLU.  Every NumPy product and sum is an IEEE double operation rounded on its own, in
the header's order, so it is the authority the device results are compared with bit for bit.  The
tables themselves are restated here too (`m_of`, `chirp_index`, `filt_of`), for
tests/test_fourier_cpu.py to pin the product's against.  The significance pipeline is composed
from surrogate_cases.significance and smooth_cases.significance, which take the surrogate series.
"""
import numpy as np

import noise_cases as NC
import smooth_cases as SMC
import spectra_cases as SC
import surrogate_cases as SGC

K_MIN, K_MAX = 4, 4096
NAN = float("nan")
U = 2.0**-53


def m_of(K):
  """The smallest power of two M with M >= 2K - 1 and M >= 8."""
  M = 8
  while M < 2 * K - 1:
    M *= 2
  return M


def chirp_index(K):
  """q_j = j^2 mod 2K in Python integers."""
  return np.array([(j * j) % (2 * K) for j in range(K)], dtype=np.int64)


_TABLES = {}


def tables(K):
  """The product's tables of K (pymoc_amd.fourier.Tables), one object per K."""
  if K not in _TABLES:
    from pymoc_amd.fourier import Tables
    _TABLES[K] = Tables(K)
  return _TABLES[K]


def fft_c(re, im, tw):
  """(re, im) [..., M] of DFT(re + i im) with the header's rounding: spectra_cases.fft_dit with an
  imaginary part to start from (with im = 0 it is that function, bit for bit)."""
  M = re.shape[-1]
  lead = re.shape[:-1]
  rev = SC.bitrev(M)
  re = np.ascontiguousarray(re[..., rev], dtype=np.float64)
  im = np.ascontiguousarray(im[..., rev], dtype=np.float64)
  h = 1
  with np.errstate(all="ignore"):
    while h < M:
      W = tw[np.arange(h) * (M // (2 * h))]
      wr, wi = W[:, 0], W[:, 1]
      re = re.reshape(lead + (M // (2 * h), 2 * h))
      im = im.reshape(lead + (M // (2 * h), 2 * h))
      ur, ui, vr, vi = re[..., :h], im[..., :h], re[..., h:], im[..., h:]
      tr = wr * vr - wi * vi
      ti = wr * vi + wi * vr
      re = np.concatenate([ur + tr, ur - tr], axis=-1)
      im = np.concatenate([ui + ti, ui - ti], axis=-1)
      h *= 2
  return re.reshape(lead + (M,)), im.reshape(lead + (M,))


def extension(K, chirp):
  """b [M] (re, im): b_j = conj(chirp_j), j < K; b_{M - j} = b_j, 1 <= j < K; +0 elsewhere."""
  M = m_of(K)
  br, bi = np.zeros(M), np.zeros(M)
  for j in range(K):
    br[j], bi[j] = chirp[j, 0], 0.0 - chirp[j, 1]
  for j in range(1, K):
    br[M - j], bi[M - j] = br[j], bi[j]
  return br, bi


def filt_of(K, tw, chirp):
  """filt [M, 2] restated: fft_c of the extension."""
  fr, fi = fft_c(*extension(K, chirp), tw)
  return np.stack([fr, fi], axis=1)


def cmul(xr, xi, cr, ci):
  """x * c: re = x.re*c.re - x.im*c.im, im = x.re*c.im + x.im*c.re."""
  with np.errstate(all="ignore"):
    return xr * cr - xi * ci, xr * ci + xi * cr


def blu(xr, xi, K, sign, tab=None):
  """BLU(x, sigma) of the header: (re, im) [..., K] of the DFT of length K of x [..., K] with the
  sign `sign` (-1 forward, +1 inverse)."""
  tab = tables(K) if tab is None else tab
  M = tab.M
  s = -1.0 if sign > 0 else 1.0  # (conjugation: an exact sign flip)
  cr, ci = tab.chirp[:, 0], s * tab.chirp[:, 1]
  br, bi = tab.filt[:, 0], s * tab.filt[:, 1]
  lead = xr.shape[:-1]
  ar, ai = np.zeros(lead + (M,)), np.zeros(lead + (M,))
  ar[..., :K], ai[..., :K] = cmul(xr, xi, cr, ci)
  Ar, Ai = fft_c(ar, ai, tab.tw)
  Cr, Ci = cmul(Ar, Ai, br, bi)
  Fr, Fi = fft_c(Cr, -Ci, tab.tw)
  inv_m = 1.0 / np.float64(M)
  with np.errstate(all="ignore"):
    c_re, c_im = Fr * inv_m, (-Fi) * inv_m
  return cmul(c_re[..., :K], c_im[..., :K], cr, ci)


def residual(v, k0, k1, detrend):
  """(r [nspec, n, K], finite [nspec, n]): the r_j of pm_series_windows for ONE window of K records
  (stt = K (K^2 - 1) / 12 as the entry forms it, a multiple of a half), and which series hold
  finite records only."""
  x = np.moveaxis(np.asarray(v, dtype=np.float64)[k0:k1], 0, -1)  # [nspec, n, K]
  K = k1 - k0
  half = np.float64(0.5) * np.float64(K - 1)
  t = np.arange(K, dtype=np.float64) - half
  stt = np.float64(K) * (np.float64(K) * np.float64(K) - 1.0) / 12.0
  lead = x.shape[:-1]
  with np.errstate(all="ignore"):
    s, st = np.zeros(lead), np.zeros(lead)
    for j in range(K):
      s = s + x[..., j]
      st = st + t[j] * x[..., j]
    mean = s / np.float64(K)
    if detrend == "linear":
      slope = st / stt
      r = (x - mean[..., None]) - slope[..., None] * t
    elif detrend == "constant":
      r = x - mean[..., None]
    else:
      r = x.copy()
  return r, np.isfinite(x).all(axis=-1)


def coefficients(v, k0, k1, detrend, tab=None):
  """coef [2, K / 2 + 1, nspec, n] of the series v [nrec, nspec, n]."""
  K = k1 - k0
  r, fin = residual(v, k0, k1, detrend)
  Rr, Ri = blu(r, np.zeros_like(r), K, -1, tab)
  nf = K // 2 + 1
  coef = np.stack([np.moveaxis(Rr[..., :nf], -1, 0), np.moveaxis(Ri[..., :nf], -1, 0)])
  return np.where(fin[None, None], coef, NAN)


def phase_index(K, b0, nb, nspec, seed, ids):
  """q [(K - 1) / 2, nb, nspec, n] (row f - 1: frequency f): the top 16 bits of output word 0 of
  Philox4x32-10 on the counter {id_lo, id_hi, b, (s << 12) | f} -- noise_cases.words with the
  surrogate number in the slot of `j` and (index, frequency) in the slot of `stream`."""
  ids = np.asarray(ids, dtype=np.uint64)
  half = (K - 1) // 2
  f = np.arange(1, half + 1, dtype=np.uint64)[:, None, None, None]
  b = np.arange(b0, b0 + nb, dtype=np.uint64)[None, :, None, None]
  s = np.arange(nspec, dtype=np.uint64)[None, None, :, None]
  i = ids[None, None, None, :]
  seed = int(seed)
  w = NC.philox4x32_10((i & NC.MASK, i >> NC.S32, b, (s << np.uint64(12)) | f),
                       (seed & 0xffffffff, seed >> 32))
  return (np.broadcast_to(w[0], (half, nb, nspec, ids.size)) >> np.uint64(16)).astype(np.int64)


def rotation(q, tab):
  """E = ph_hi[q >> 8] * ph_lo[q & 255]: (re, im) of q's shape."""
  hi, lo = tab.ph_hi[q >> 8], tab.ph_lo[q & 255]
  return cmul(hi[..., 0], hi[..., 1], lo[..., 0], lo[..., 1])


def spectrum(coef, K, b0, nb, seed, ids, tab=None):
  """(Zr, Zi) [nb, nspec, n, K]: the rotated, mirrored coefficients the synthesis transforms."""
  tab = tables(K) if tab is None else tab
  coef = np.asarray(coef, dtype=np.float64)
  nspec, n = coef.shape[2:]
  half = (K - 1) // 2
  Zr, Zi = np.zeros((nb, nspec, n, K)), np.zeros((nb, nspec, n, K))
  Zr[..., 0] = coef[0, 0]
  if K % 2 == 0:
    Zr[..., K // 2] = coef[0, K // 2]
  Er, Ei = rotation(phase_index(K, b0, nb, nspec, seed, ids), tab)  # [half, nb, nspec, n]
  zr, zi = cmul(coef[0, 1:half + 1, None], coef[1, 1:half + 1, None], Er, Ei)
  for f in range(1, half + 1):
    Zr[..., f], Zi[..., f] = zr[f - 1], zi[f - 1]
    Zr[..., K - f], Zi[..., K - f] = zr[f - 1], -zi[f - 1]
  return Zr, Zi


def synthesis(coef, K, b0, nb, seed, ids, tab=None, imag=False):
  """y [K, nb * nspec, n] of the surrogates b0 .. b0 + nb - 1 (plane i * nspec + s) from coef
  [2, K / 2 + 1, nspec, n]; imag=True: (y, the imaginary part the device does not keep, / K)."""
  tab = tables(K) if tab is None else tab
  Zr, Zi = spectrum(coef, K, b0, nb, seed, ids, tab)
  nspec, n = Zr.shape[1:3]
  yr, yi = blu(Zr, Zi, K, +1, tab)
  with np.errstate(all="ignore"):
    yr, yi = yr / np.float64(K), yi / np.float64(K)
  yr = np.ascontiguousarray(np.moveaxis(yr, -1, 0)).reshape(K, nb * nspec, n)
  if imag:
    return yr, np.ascontiguousarray(np.moveaxis(yi, -1, 0)).reshape(K, nb * nspec, n)
  return yr


def surrogates(v, k0, k1, detrend, b0, nb, seed, ids, sigma=None, truncate=4.0):
  """SeriesSurrogates(method="fourier").generate: under "gaussian" the "constant" coefficients of
  the smoother's residual."""
  K = k1 - k0
  if detrend == "gaussian":
    v = SMC.smooth(v, k0, k1, SMC.weights(sigma, truncate))["resid"]
    k0, k1, detrend = 0, K, "constant"
  return synthesis(coefficients(v, k0, k1, detrend), K, b0, nb, seed, ids)


def significance(v, k0, k1, W, S, Lg, detrend, nsur, seed=0, ids=None, nb=None, sigma=None,
                 truncate=4.0):
  """SeriesWindows.significance(method="fourier"): the pipeline of surrogate_cases.significance
  (smooth_cases.significance under "gaussian") fed the Fourier surrogates of the record window."""
  v = np.asarray(v, dtype=np.float64)
  ids = np.arange(v.shape[2]) if ids is None else ids
  sur = np.concatenate([surrogates(v, k0, k1, detrend, b0, m, seed, ids, sigma, truncate)
                        for b0, m in SGC.chunks(nsur, nb or nsur)], axis=1)
  if detrend == "gaussian":
    return SMC.significance(v, k0, k1, W, S, Lg, sigma, truncate, nsur, nb=nb, sur=sur)
  return SGC.significance(v, k0, k1, W, S, Lg, detrend, nsur, nb=nb, sur=sur)


# ------------------------------------------------------------------ the accuracy bound
def bound(K, norm2):
  """The bound on |BLU(x)_k - DFT(x)_k| for every k, ||x||_2 = norm2 (DESIGN.md section 26 has the
  derivation, from Higham, Accuracy and Stability, Thm 24.2): 12 (2K - 1) (2 log2 M + 2) 2^-53
  ||x||_2."""
  L = m_of(K).bit_length() - 1
  return 12.0 * (2 * K - 1) * (2 * L + 2) * U * norm2


def dft_long(xr, xi, sign):
  """The direct O(K^2) DFT in np.longdouble of x [..., K], sign -1 forward / +1 inverse (not
  divided by K); the angles reduced in integers."""
  K = xr.shape[-1]
  j = np.arange(K)
  jk = (j[:, None] * j[None, :]) % K
  ang = np.longdouble(2.0) * np.arccos(np.longdouble(-1.0)) * jk.astype(np.longdouble) / np.longdouble(K)
  c, s = np.cos(ang), sign * np.sin(ang)
  xr, xi = xr.astype(np.longdouble), xi.astype(np.longdouble)
  return xr @ c - xi @ s, xr @ s + xi @ c


# ------------------------------------------------------------------ the case table
K0, AFTER = 3, 2
RECORDS = (4, 5, 8, 9, 17, 96, 257, 1200, 2048, 2049, 4096)
M_OF = {4: 8, 5: 16, 8: 16, 9: 32, 17: 64, 96: 256, 257: 1024, 1200: 4096, 2048: 4096, 2049: 8192,
        4096: 8192}
BIG = 1200  # from here on a case runs at n <= 3, nspec = 1
DETRENDS = ("none", "constant", "linear")
STYLES = ("red", "nan1", "inf1", "const", "zeros", "big", "small", "tone")
B0S = (0, 5, 2**32 - 3)
MEMBER0S = (0, 2**33 + 7)


def _series(style, red, K, rng):
  """One series of K0 + K + AFTER records in the given style, from its red noise; its record
  window starts at K0."""
  nrec = red.size
  t = np.arange(nrec) - K0
  if style == "const":  # every partial sum exact: zero coefficients once a mean is removed
    return np.full(nrec, 3.0)
  if style == "zeros":  # signed zeros
    return np.where(np.arange(nrec) % 3 == 1, -0.0, 0.0)
  if style == "big":
    return red * 1e150
  if style == "small":
    return red * 1e-150
  if style == "tone":  # a pure sinusoid at the DFT frequency K // 4 (at least 1)
    return 2.0 * np.cos(2.0 * np.pi * max(1, K // 4) * t / K + 0.3)
  x = 15.0 + red
  if style == "nan1":
    x[K0 + int(rng.integers(K))] = np.nan
  if style == "inf1":
    x[K0 + K - 1] = np.inf if rng.random() < 0.5 else -np.inf
  return x


def style_of(s, m, n):
  return STYLES[(m + 3 * s) % len(STYLES)] if n > 3 else ("red", "zeros", "big")[(m + s) % 3]


def case(K, n, nspec, detrend, nb, b0, member0, seed=0):
  """A series [K0 + K + AFTER, nspec, n] whose record window [K0, K0 + K) is what the entries read;
  the records before and behind it are numbers that would change every result if they were read.
  With n > 3, member m of index s has the style STYLES[(m + 3 s) % 8]; a case of n <= 3 holds
  red, zeros and big in turn: the special series run at n = 65."""
  rng = np.random.default_rng(9000 + 31 * K + seed)
  nrec = K0 + K + AFTER
  v = np.empty((nrec, nspec, n))
  a = rng.standard_normal((nspec, n))
  for k in range(nrec):
    a = 0.9 * a + np.sqrt(1.0 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = a
  for s in range(nspec):
    for m in range(n):
      v[:, s, m] = _series(style_of(s, m, n), v[:, s, m].copy(), K, rng)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  return dict(name="K %d n %d nspec %d %s nb %d b0 %d member0 %d" % (K, n, nspec, detrend, nb, b0,
                                                                   member0),
              v=v, k0=K0, k1=K0 + K, K=K, n=n, nspec=nspec, detrend=detrend, nb=nb, b0=b0,
              member0=member0, seed=0xD1B54A32D192ED03 + seed)


def cases():
  """Every K crossed with every detrend; n in {1, 3, 65}, nspec in {1, 3}, nb in {1, 3}, b0 and
  member0 rotate through their values.  K >= 1200 runs at n <= 3, nspec = 1."""
  out = []
  for ki, K in enumerate(RECORDS):
    for di, detrend in enumerate(DETRENDS):
      i = ki + di
      if K >= BIG:
        n, nspec = (1, 3, 2)[i % 3], 1
      else:
        n, nspec = (1, 3, 65)[i % 3], (1, 3)[(ki + 2 * di) % 2 if K < 257 else 0]
      out.append(case(K, n, nspec, detrend, (1, 3)[(ki // 2 + di) % 2], B0S[(ki + 2 * di) % 3],
                      MEMBER0S[(ki + di // 2) % 2], 3 * ki + di))
  # every style at the smallest K, at an odd K and at the workload's shape of M
  for K in (4, 17, 96):
    out.append(case(K, 65, 3, "linear", 3, 5, MEMBER0S[1], 100 + K))
  return out


def ids_of(c, n=None):
  return np.uint64(c["member0"]) + np.arange(c["n"] if n is None else n, dtype=np.uint64)


def restate(c, **kw):
  """dict(coef [2, nf, nspec, n], y [K, nb * nspec, n]) of a case (with the edits kw)."""
  c = dict(c, **kw)
  coef = coefficients(c["v"], c["k0"], c["k1"], c["detrend"])
  ids = np.uint64(c["member0"]) + np.arange(c["v"].shape[2], dtype=np.uint64)
  return dict(coef=coef, y=synthesis(coef, c["K"], c["b0"], c["nb"], c["seed"], ids))
