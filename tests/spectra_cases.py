"""The NumPy restatement of pm_series_spectra, and the case table.

The restatement follows include/pymoc_hip.h literally: the segments, the sequential mean, the
iterative radix-2 decimation-in-time transform on the table of pymoc_amd.spectra.twiddles --
vectorised per stage, every NumPy product and sum an IEEE double operation rounded on its own, in
the order the header states -- the periodogram and the sequential sum over the used segments.  It
is the authority the device results are compared with bit for bit.  Shared by
tests/test_spectra_cpu.py (which pins it to an extended-precision direct DFT and to
scipy.signal.welch / csd) and the GPU tests.
"""
import numpy as np

NPERSEG_MIN, NPERSEG_MAX, PAIRS_MAX = 8, 1024, 8
NAN = float("nan")


def bitrev(L):
  """bitrev(j) for j < L, L a power of two."""
  bits = L.bit_length() - 1
  j = np.arange(L)
  r = np.zeros(L, dtype=np.int64)
  for b in range(bits):
    r |= ((j >> b) & 1) << (bits - 1 - b)
  return r


def fft_dit(y, tw):
  """(re, im) [..., L] of DFT(y + 0i), y [..., L] real, with the header's rounding."""
  L = y.shape[-1]
  lead = y.shape[:-1]
  re = np.ascontiguousarray(y[..., bitrev(L)], dtype=np.float64)
  im = np.zeros_like(re)
  h = 1
  with np.errstate(all="ignore"):
    while h < L:
      W = tw[np.arange(h) * (L // (2 * h))]
      wr, wi = W[:, 0], W[:, 1]
      re = re.reshape(lead + (L // (2 * h), 2 * h))
      im = im.reshape(lead + (L // (2 * h), 2 * h))
      ur, ui, vr, vi = re[..., :h], im[..., :h], re[..., h:], im[..., h:]
      tr = wr * vr - wi * vi
      ti = wr * vi + wi * vr
      re = np.concatenate([ur + tr, ur - tr], axis=-1)
      im = np.concatenate([ui + ti, ui - ti], axis=-1)
      h *= 2
  return re.reshape(lead + (L,)), im.reshape(lead + (L,))


def nseg_of(K, L, noverlap):
  return (K - L) // (L - noverlap) + 1


def segments(v, k0, k1, L, noverlap, w, detrend, with_mean=False):
  """(y [nseg, nspec, n, L], used [nseg, nspec, n]): the detrended, windowed segments of the
  window [k0, k1) and which of them are used (all L values finite); with_mean: also the mean that
  was removed [nseg, nspec, n] (zeros without detrending)."""
  v = np.asarray(v, dtype=np.float64)
  S = L - noverlap
  nseg = nseg_of(k1 - k0, L, noverlap)
  x = np.stack([v[k0 + i * S:k0 + i * S + L] for i in range(nseg)])  # [nseg, L, nspec, n]
  x = np.moveaxis(x, 1, -1)
  used = np.isfinite(x).all(axis=-1)
  with np.errstate(all="ignore"):
    if detrend == "constant":
      s = np.zeros(x.shape[:-1])
      for j in range(L):
        s = s + x[..., j]
      mu = s / np.float64(L)
      y = (x - mu[..., None]) * w
    else:
      mu = np.zeros(x.shape[:-1])
      y = x * w
  return (y, used, mu) if with_mean else (y, used)


def _average(terms, used, scale, L):
  """((acc / nused) * scale) * c of terms [nseg, ..., nf] over the used segments, and nused."""
  acc = np.zeros(terms.shape[1:])
  with np.errstate(all="ignore"):
    for i in range(terms.shape[0]):
      acc = np.where(used[i][..., None], acc + terms[i], acc)
    nused = used.sum(axis=0).astype(np.int32)
    c = np.full(L // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    out = ((acc / nused[..., None].astype(np.float64)) * np.float64(scale)) * c
  return np.where(nused[..., None] > 0, out, NAN), nused


def spectra(v, k0, k1, L, noverlap, w, detrend, pairs, scale, tw):
  """dict(nused [nspec, n], psd [nf, nspec, n], nused_pair [npairs, n], csd [nf, 2 npairs, n]) of
  the series v [nrec, nspec, n]; pairs are index pairs (a, b): conj(Za) * Zb."""
  y, used = segments(v, k0, k1, L, noverlap, w, detrend)
  re, im = fft_dit(y, tw)
  nf = L // 2 + 1
  re, im = re[..., :nf], im[..., :nf]
  n = y.shape[2]
  with np.errstate(all="ignore"):
    psd, nused = _average(re * re + im * im, used, scale, L)
    csd = np.zeros((nf, 2 * len(pairs), n))
    nused_pair = np.zeros((len(pairs), n), dtype=np.int32)
    for p, (a, b) in enumerate(pairs):
      both = used[:, a] & used[:, b]
      cr = re[:, a] * re[:, b] + im[:, a] * im[:, b]
      ci = re[:, a] * im[:, b] - im[:, a] * re[:, b]
      r, nused_pair[p] = _average(cr, both, scale, L)
      i, _ = _average(ci, both, scale, L)
      csd[:, 2 * p], csd[:, 2 * p + 1] = r.T, i.T
  return dict(nused=nused, psd=np.ascontiguousarray(np.moveaxis(psd, -1, 0)),
              nused_pair=nused_pair, csd=csd)


# ------------------------------------------------------------------ the case table
STYLES = ("red", "tone", "const", "big", "small", "nan1", "inf1", "spoiled")
FINITE_STYLES = STYLES[:5]
PAIRS3 = ((0, 2), (2, 0), (1, 1))
K0, AFTER = 3, 2


def style_of(s, m):
  return STYLES[(m + 3 * s) % len(STYLES)]


def window_of(kind, L, seed):
  from pymoc_amd.spectra import hann
  if kind == "hann":
    return hann(L)
  if kind == "boxcar":
    return np.ones(L)
  return np.random.default_rng(50 + seed).uniform(0.2, 1.7, size=L)  # random, positive


def _series(rng, style, red, k0, L, S, nseg):
  """One (index, member) series in the given style, from its red noise (variance 1, decorrelation
  ten records); its window starts at k0."""
  nrec = red.size
  t = np.arange(nrec) - k0
  if style == "tone":  # a pure tone on bin L / 4, on an offset
    return 3.0 + 2.0 * np.cos(2.0 * np.pi * (L // 4) * t / L + 0.3)
  if style == "const":  # (0.1 is not a dyadic fraction: the sequential mean rounds)
    return np.full(nrec, 0.1)
  if style == "big":  # (without an offset: at L = 1024 the square of its sum would overflow)
    return red * 1e150
  if style == "small":
    return red * 1e-150
  x = 15.0 + red  # red noise on an offset
  if style == "nan1":  # the first record of the window lies in segment 0 alone
    x[k0] = np.nan
  if style == "inf1":  # the last record of the last segment lies in that segment alone
    x[k0 + (nseg - 1) * S + L - 1] = np.inf if rng.random() < 0.5 else -np.inf
  if style == "spoiled":  # every L consecutive records hold one of these
    x[(t % L) == L - 1] = np.nan
  return x


def case(L, noverlap, nseg, n, nspec, detrend, window, seed=0):
  """A series [K0 + K + AFTER, nspec, n]: the window [K0, K0 + K) holds nseg whole segments and a
  tail of records that fits none (as long as the step leaves room for one); the records before and
  behind the window are numbers that would change every result if they were read.  Member m of
  index s has the style STYLES[(m + 3 s) % 8]."""
  rng = np.random.default_rng(3000 + 17 * L + seed)
  S = L - noverlap
  tail = min(S - 1, 3)
  K = L + (nseg - 1) * S + tail
  nrec = K0 + K + AFTER
  v = np.empty((nrec, nspec, n))
  a = rng.standard_normal((nspec, n))
  for k in range(nrec):
    a = 0.9 * a + np.sqrt(1.0 - 0.81) * rng.standard_normal((nspec, n))
    v[k] = a
  for s in range(nspec):
    for m in range(n):
      v[:, s, m] = _series(rng, style_of(s, m), v[:, s, m].copy(), K0, L, S, nseg)
  v[:K0] = 7e30
  v[K0 + K:] = -3e30
  w = window_of(window, L, seed)
  return dict(name="L %d noverlap %d nseg %d n %d nspec %d %s %s"
              % (L, noverlap, nseg, n, nspec, detrend, window),
              v=v, k0=K0, k1=K0 + K, L=L, noverlap=noverlap, nseg=nseg, detrend=detrend,
              window=window, w=w, pairs=PAIRS3 if nspec == 3 else (), dt=0.5,
              scale=float(np.float64(1.0) / (np.float64(2.0) * (w * w).sum())))


def cases():
  return [
      case(8, 0, 1, 1, 1, "constant", "hann", 1),
      case(8, 4, 5, 7, 3, "none", "boxcar", 2),
      case(8, 7, 2, 65, 3, "constant", "random", 3),
      case(16, 8, 2, 65, 3, "constant", "hann", 4),
      case(32, 31, 5, 7, 3, "none", "random", 5),
      case(64, 0, 2, 64, 3, "constant", "hann", 6),
      case(64, 32, 5, 65, 1, "none", "random", 7),
      case(64, 63, 5, 7, 3, "constant", "boxcar", 8),
      case(128, 0, 5, 7, 3, "none", "hann", 9),
      case(128, 64, 2, 65, 3, "constant", "random", 10),
      case(128, 127, 1, 64, 1, "constant", "boxcar", 11),
      case(256, 128, 5, 65, 3, "constant", "hann", 12),
      case(512, 256, 2, 7, 3, "none", "random", 13),
      case(1024, 512, 2, 65, 3, "constant", "hann", 14),
      case(1024, 1023, 5, 7, 3, "none", "random", 15),
      case(1024, 0, 1, 1, 3, "constant", "boxcar", 16),
  ]


def restate(c, v=None, pairs=None):
  """The restatement of a case (or of another series / other pairs under the case's settings)."""
  from pymoc_amd.spectra import twiddles
  return spectra(c["v"] if v is None else v, c["k0"], c["k1"], c["L"], c["noverlap"], c["w"],
                 c["detrend"], c["pairs"] if pairs is None else pairs, c["scale"],
                 twiddles(c["L"]))
