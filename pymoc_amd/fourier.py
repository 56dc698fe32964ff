"""The host side of the Fourier phase-randomised surrogates (surrogates.py, method="fourier"): the
tables the two entries of csrc/fourier.hip read, and the two launches.

The device calls no sin, cos, exp or sqrt: every trigonometric value comes from the tables made
here, once per record count K, in float64.  include/pymoc_hip.h states what they hold and what the
entries compute from them; tests/fourier_cases.py restates both on these very arrays, which is
what makes every double reproducible bit for bit.

  m_of(K)        M, the transform length of Bluestein's chirp-z: the smallest power of two with
                 M >= 2K - 1 and M >= 8
  chirp_index(K) q = j^2 mod 2K, in integers: the chirp's argument pi q / K never exceeds 2 pi
  chirp(K)       (cos(pi q / K), -sin(pi q / K)) [K, 2]
  filt(K)        the transform of the even extension of conj(chirp) [M, 2], by `fft_dit`
  phases()       ph_hi = e^{2 pi i a / 256}, ph_lo = e^{2 pi i c / 65536}, each [256, 2]
  fft_dit        the header's radix-2 decimation-in-time transform of a complex series, vectorised
                 per stage, every product and sum rounded on its own
  Tables(K)      all of them with their device copies; `tables_of(cache, K)` makes one per K

  wants_scratch(K)  whether the synthesis is given a second array to store series-contiguously
                 and transpose from: where a block holds one series, M >= 2048

`launch_coef` and `launch_synthesis` are the launches alone, over any device view (series.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .spectra import twiddles

M_MIN, M_MAX = 8, 8192
SCRATCH_FROM_M = 2048


def m_of(K):
  K = int(K)
  M = M_MIN
  while M < 2 * K - 1:
    M *= 2
  return M


def chirp_index(K):
  """q[j] = j^2 mod 2K, j < K, in integer arithmetic."""
  K = int(K)
  j = np.arange(K, dtype=np.int64)
  return (j * j) % (2 * K)


def chirp(K):
  """chirp[j] = (cos(pi q / K), -sin(pi q / K)), q = chirp_index(K)[j]: e^{-i pi j^2 / K}."""
  K = int(K)
  q = chirp_index(K)
  # the angle pi q / K folded, in integers, into the first octant, where sin / cos are at their
  # most accurate: past pi by 2 pi - t, past pi / 2 by pi - t, past pi / 4 by pi / 2 - t
  low = q > K
  q = np.where(low, 2 * K - q, q)           # sin changes sign
  left = 2 * q > K
  q = np.where(left, K - q, q)              # cos changes sign
  swap = 4 * q > K
  num = np.where(swap, K - 2 * q, 2 * q)    # the angle is pi num / (2K), num <= K / 2
  ang = np.pi * (num.astype(np.float64) / np.float64(2 * K))
  c, s = np.cos(ang), np.sin(ang)
  c, s = np.where(swap, s, c), np.where(swap, c, s)
  c, s = np.where(left, 0.0 - c, c), np.where(low, 0.0 - s, s)
  return np.ascontiguousarray(np.stack([c + 0.0, 0.0 - s], axis=1))


def phases():
  """(ph_hi, ph_lo), each [256, 2]: e^{2 pi i a / 256} and e^{2 pi i c / 65536}."""
  a = np.arange(256, dtype=np.float64)
  hi, lo = 2.0 * np.pi * (a / 256.0), 2.0 * np.pi * (a / 65536.0)
  return (np.ascontiguousarray(np.stack([np.cos(hi), np.sin(hi)], axis=1)),
          np.ascontiguousarray(np.stack([np.cos(lo), np.sin(lo)], axis=1)))


def bitrev(M):
  bits = M.bit_length() - 1
  j = np.arange(M)
  r = np.zeros(M, dtype=np.int64)
  for b in range(bits):
    r |= ((j >> b) & 1) << (bits - 1 - b)
  return r


def fft_dit(re, im, tw):
  """(re, im) [..., M] of the DFT of the complex series (re, im) [..., M] with the header's
  rounding: a[j] = x[bitrev(j)], then the stages h = 1 .. M / 2 with W = tw[q * (M / (2h))]."""
  M = re.shape[-1]
  lead = re.shape[:-1]
  rev = bitrev(M)
  re = np.ascontiguousarray(np.asarray(re, dtype=np.float64)[..., rev])
  im = np.ascontiguousarray(np.asarray(im, dtype=np.float64)[..., rev])
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


def filt(K, tw=None, ch=None):
  """filt [M, 2]: fft_dit of b, b_j = conj(chirp_j) for j < K, b_{M - j} = b_j for 1 <= j < K, +0
  elsewhere."""
  M = m_of(K)
  tw = twiddles(M) if tw is None else tw
  ch = chirp(K) if ch is None else ch
  br, bi = np.zeros(M), np.zeros(M)
  br[:K], bi[:K] = ch[:, 0], 0.0 - ch[:, 1]
  br[M - K + 1:], bi[M - K + 1:] = br[1:K][::-1], bi[1:K][::-1]
  fr, fi = fft_dit(br, bi, tw)
  return np.ascontiguousarray(np.stack([fr, fi], axis=1))


class Tables(object):
  """The tables of one K: `K`, `M`, the host arrays `tw`, `chirp`, `filt`, `ph_hi`, `ph_lo` (the
  entries check these) and, from the first launch on, their device copies."""
  KEYS = ("tw", "chirp", "filt", "ph_hi", "ph_lo")

  def __init__(self, K):
    self.K, self.M = int(K), m_of(K)
    self.tw, self.chirp = twiddles(self.M), chirp(K)
    self.filt = filt(K, self.tw, self.chirp)
    self.ph_hi, self.ph_lo = phases()
    self._dev = None

  def dev(self, stream=None):
    if self._dev is None:
      self._dev = {key: DeviceArray.from_host(getattr(self, key), dtype=np.float64, stream=stream)
                   for key in self.KEYS}
    return self._dev

  def fill(self, d, keys, stream=None):
    """The host and device addresses of the tables `keys` into the descriptor `d`."""
    dev = self.dev(stream)
    for key in keys:
      setattr(d, key, getattr(self, key).ctypes.data)
      setattr(d, key + "_dev", dev[key].ptr)


def launch_coef(x, k0, k1, detrend, stt, tab, ctx, out=None):
  """pm_series_fourier_coef over the records [k0, k1) of the device view `x` under the entry's
  `detrend` (PM_WIN_DETREND_*): coef [2, K / 2 + 1, nspec, n] on the device, nothing
  synchronised.  `out`: the array of an earlier call, written again."""
  d = _lib.pm_series_fourier_coef()
  (d.nrec, d.nspec, d.n), d.k0, d.k1 = x.shape, k0, k1
  d.detrend, d.M, d.stt, d.v = detrend, tab.M, stt, x.ptr
  tab.fill(d, ("tw", "chirp", "filt"), ctx.stream)
  if out is None:
    out = DeviceArray((2, (k1 - k0) // 2 + 1) + tuple(x.shape[1:]), np.float64)
  with launch_span(ctx.timer, "k_series_fourier_coef", ctx.stream):
    check(lib.pm_series_fourier_coef(C.byref(d), out.ptr, _sh(ctx.stream)))
  return out


def wants_scratch(K):
  """Whether the synthesis of K records is given a scratch array: from M = 2048 on, where a block
  holds a single series and would store 8 bytes per record (csrc/fourier.hip)."""
  return m_of(K) >= SCRATCH_FROM_M


def tables_of(cache, K):
  """The `Tables` of K out of the dict `cache`, made at the first call."""
  if K not in cache:
    cache[K] = Tables(K)
  return cache[K]


def launch_synthesis(y, coef, nspec, b0, seed, member0, tab, ctx, scratch=None):
  """pm_series_surrogates_fourier: the surrogates b0 .. b0 + nb - 1 of the coefficients `coef`
  [2, K / 2 + 1, nspec, n] into the device view `y` [K, nb * nspec, n]; nothing synchronised.
  `scratch`: a device array of at least y's size (not y), through which the entry stores
  series-contiguously and transposes: the same values."""
  d = _lib.pm_series_surrogates_fourier()
  d.K, d.nspec, d.n, d.b0 = y.shape[0], nspec, y.shape[2], b0
  d.nb = y.shape[1] // nspec
  d.member0, d.seed, d.M, d.coef = member0, seed, tab.M, coef.ptr
  d.scratch = None if scratch is None else scratch.ptr
  tab.fill(d, Tables.KEYS, ctx.stream)
  with launch_span(ctx.timer, "k_series_surrogates_fourier", ctx.stream):
    check(lib.pm_series_surrogates_fourier(C.byref(d), y.ptr, _sh(ctx.stream)))
