"""SeriesSpectra: Welch power and cross spectra of a recorded index series, on the device.

A stochastic overturning experiment is read in the frequency domain: the variability spectrum of
the AMOC under white or red forcing, the coherence and phase between a forcing index and the
response.  `SeriesSpectra` computes the Welch power spectral density of every (index, member)
series an `IndexRecorder` keeps on the device ([n_samples][nspec][n]) and the cross spectral
density of up to 8 pairs of indices per member, in ONE launch where the series lives
(pm_series_spectra, csrc/spectra.hip); only the results are downloaded.

  compute(k0, k1)          freq, psd[name] [n, nf], nused[name] [n], csd[(a, b)] (complex, SciPy's
                           conj(Za) * Zb), nused_pair, coherence and phase [n, nf]
  across_members(k0, k1)   the launch, then the device spectra as a series [nf][nspec][n] through
                           SeriesStats.across_members: the group-mean spectrum and its quantile
                           bands per frequency, no per-member spectrum downloaded

A segment with a non-finite value is excluded and counted (`nused`), never propagated.  The
transform is the iterative radix-2 decimation-in-time FFT with the op order include/pymoc_hip.h
states, on a twiddle table made by `twiddles` alone, so every double equals the NumPy restatement
(tests/spectra_cases.py) bit for bit; the restatement is pinned to scipy.signal.welch / csd
(scaling="density", one-sided, detrend="constant" or False).  What a source and a record window
[k0, k1) are: series.py.

`coherence[(a, b)]` = |csd|^2 / (psd_a * psd_b) and `phase` = angle(csd) are formed on the host.
The coherence needs the spectra of the pair's own segments; those are psd_a and psd_b exactly when
every segment used for one of the two series is used for the other (nused[a] = nused[b] =
nused_pair > 0) -- for the other members the coherence is NaN.

Out of scope:
  * linear detrending;
  * zero padding (nfft > nperseg);
  * median averaging of the segments;
  * spectra across ranks: every rank transforms its own members;
  * spectra of `pos` (the positions an IndexRecorder keeps next to the values);
  * anything online: a spectrum is computed from the recorded series, after the samples.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Series, as_int, by_name
from .stats import SeriesStats

_DETREND = dict(constant=_lib.PM_SPEC_DETREND_CONSTANT, none=_lib.PM_SPEC_DETREND_NONE)


def twiddles(L):
  """tw[j] = (cos(2 pi j / L), -sin(2 pi j / L)), j < L / 2, as float64 [L / 2, 2]: the one table
  the kernel and the restatement transform with.  The entries at j = 0 and j = L / 4 are exact:
  (1, 0) and (0, -1)."""
  L = int(L)
  j = np.arange(L // 2)
  # every angle folded into the first octant, where 2 k / L is exact and sin / cos are at their
  # most accurate: cos(pi - t) = -cos(t), then cos(pi / 2 - t) = sin(t)
  second = j > L // 4
  jj = np.where(second, L // 2 - j, j)
  swap = jj > L // 8
  k = np.where(swap, L // 4 - jj, jj)
  ang = np.pi * (2.0 * k / np.float64(L))
  c, s = np.cos(ang), np.sin(ang)
  c, s = np.where(swap, s, c), np.where(swap, c, s)
  tw = np.stack([np.where(second, -c, c), -s], axis=1)
  tw[0] = (1.0, 0.0)
  tw[L // 4] = (0.0, -1.0)
  return np.ascontiguousarray(tw)


def hann(L):
  """The periodic Hann window scipy.signal.get_window("hann", L) returns: the symmetric window of
  L + 1 points without its last."""
  fac = np.linspace(-np.pi, np.pi, L + 1)
  w = np.zeros(L + 1)
  for k, a in enumerate((0.5, 0.5)):
    w += a * np.cos(k * fac)
  return np.ascontiguousarray(w[:-1])


class Spectra(object):
  """What `compute` returns.  freq [nf]; psd[name] [n, nf] and nused[name] [n]; per pair (a, b) of
  names csd (complex), coherence, phase [n, nf] and nused_pair [n]."""

  def __init__(self, names, pairs, freq, nused, psd, nused_pair, csd):
    # psd [nf, nspec, n], csd [nf, 2 npairs, n]
    self.names, self.pairs, self.freq = list(names), list(pairs), freq
    self.nused, self.psd = by_name(names, nused), by_name(names, psd.transpose(1, 2, 0))
    self.nused_pair = by_name(pairs, nused_pair)
    self.csd = by_name(pairs, [(csd[:, 2 * p, :] + 1j * csd[:, 2 * p + 1, :]).T
                               for p in range(len(pairs))])
    coherence = []
    for p, (a, b) in enumerate(pairs):
      same = (nused_pair[p] > 0) & (self.nused[a] == nused_pair[p]) & (self.nused[b] == nused_pair[p])
      with np.errstate(all="ignore"):
        # (two ratios of order one: spectra of 1e+-300 neither overflow nor vanish)
        mod = np.abs(self.csd[(a, b)])
        coh = (mod / self.psd[a]) * (mod / self.psd[b])
      coherence.append(np.where(same[:, None], coh, np.nan))
    self.coherence = by_name(pairs, coherence)
    self.phase = by_name(pairs, [np.angle(self.csd[pr]) for pr in pairs])


class SeriesSpectra(Series):
  """`SeriesSpectra(source, nperseg, noverlap=None, window="hann", detrend="constant", pairs=(),
  dt_record=1.0, groups=None, stream=None)`.

  source      an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  nperseg     L, a power of two in [8, 1024]
  noverlap    records two consecutive segments share, in [0, L - 1]; None: L // 2
  window      "hann" (periodic, as scipy.signal.get_window), "boxcar" or an array [L]
  detrend     "constant" (the segment's mean is removed) or "none"
  pairs       up to 8 tuples (name_a, name_b): cross spectra conj(Za) * Zb
  dt_record   the time between two records: freq = f / (L * dt_record), density per unit frequency
  groups      int array [n] of labels, for `across_members` (as SeriesStats)

  Each call of `compute` / `across_members` is one launch of pm_series_spectra on the source's
  stream.  [k0, k1) is a record window (series.py) of at least nperseg records."""

  def __init__(self, source, nperseg, noverlap=None, window="hann", detrend="constant", pairs=(),
               dt_record=1.0, groups=None, stream=None):
    Series.__init__(self, source, stream)
    L = as_int("nperseg", nperseg)
    if not _lib.PM_SPEC_NPERSEG_MIN <= L <= _lib.PM_SPEC_NPERSEG_MAX or L & (L - 1):
      raise ValueError("nperseg must be a power of two in [%d, %d] (%d here)"
                       % (_lib.PM_SPEC_NPERSEG_MIN, _lib.PM_SPEC_NPERSEG_MAX, L))
    noverlap = L // 2 if noverlap is None else as_int("noverlap", noverlap)
    if not 0 <= noverlap <= L - 1:
      raise ValueError("noverlap must lie in [0, nperseg - 1 = %d] (%d here)" % (L - 1, noverlap))
    self.nperseg, self.noverlap, self.step, self.nf = L, noverlap, L - noverlap, L // 2 + 1
    if isinstance(window, str):
      if window not in ("hann", "boxcar"):
        raise ValueError("unknown window %r (one of hann, boxcar, or an array [nperseg])"
                         % (window,))
      w = hann(L) if window == "hann" else np.ones(L)
    else:
      w = np.ascontiguousarray(window, dtype=np.float64)
      if w.shape != (L,):
        raise ValueError("a window array must have shape (nperseg,) = (%d,) (%r here)"
                         % (L, w.shape))
    if not np.isfinite(w).all():
      bad = int(np.nonzero(~np.isfinite(w))[0][0])
      raise ValueError("every window value must be finite (window[%d] = %r here)"
                       % (bad, float(w[bad])))
    if detrend not in _DETREND:
      raise ValueError("unknown detrend %r (one of constant, none)" % (detrend,))
    try:
      dt = float(dt_record)
    except (TypeError, ValueError):
      raise ValueError("dt_record must be a positive number (%r here)" % (dt_record,))
    if not (np.isfinite(dt) and dt > 0.0):
      raise ValueError("dt_record must be finite and positive (%r here)" % (dt_record,))
    fs = 1.0 / dt
    with np.errstate(all="ignore"):
      scale = np.float64(1.0) / (np.float64(fs) * (w * w).sum())
    if not np.isfinite(scale):
      raise ValueError("the scale 1 / (fs * sum w^2) = %r is not finite: the window is all zero "
                       "or dt_record is out of range" % (float(scale),))
    pairs = list(pairs)
    if len(pairs) > _lib.PM_SPEC_PAIRS_MAX:
      raise ValueError("at most %d pairs (%d here)" % (_lib.PM_SPEC_PAIRS_MAX, len(pairs)))
    idx = np.zeros((max(len(pairs), 1), 2), dtype=np.int32)
    for p, pr in enumerate(pairs):
      if not isinstance(pr, tuple) or len(pr) != 2:
        raise ValueError("pair %r: give a tuple (name_a, name_b)" % (pr,))
      for c, name in enumerate(pr):
        if name not in self.names:
          raise ValueError("pair %r: unknown index %r (one of %s)"
                           % (pr, name, ", ".join(self.names)))
        idx[p, c] = self.names.index(name)
    if self.nf * self.nspec >= 1 << 30:
      raise ValueError("nf * nspec = %d is not below 2^30" % (self.nf * self.nspec))
    if self.nspec + len(pairs) > 65535:
      raise ValueError("nspec + the number of pairs = %d is above 65535"
                       % (self.nspec + len(pairs)))
    self.pairs, self.detrend, self.dt_record = pairs, detrend, dt
    self.freq = np.arange(self.nf, dtype=np.float64) / (L * dt)
    self._set_groups(groups)  # checked now, used by across_members
    # host mirrors (the entry checks these) and, from the first launch on, device copies
    self._w, self._pair, self._scale = w, idx, float(scale)
    self._host = dict(w=w, tw=twiddles(L), pair=idx)
    self.window, self.scale = w.copy(), float(scale)

  # ------------------------------------------------------------------ device side
  def _window(self, k0, k1):
    k0, k1 = self._record_window(k0, k1)
    if k1 - k0 < self.nperseg:
      raise ValueError("window [%d, %d) holds %d records, fewer than nperseg = %d"
                       % (k0, k1, k1 - k0, self.nperseg))
    return k0, k1

  def nseg(self, k0=0, k1=None):
    """The number of whole segments the window [k0, k1) holds."""
    k0, k1 = self._window(k0, k1)
    return (k1 - k0 - self.nperseg) // self.step + 1

  def _alloc(self, npairs):
    """The outputs of a launch with `npairs` pairs: (nused, psd, nused_pair, csd), the last two
    None without pairs."""
    return (DeviceArray((self.nspec, self.n), np.int32),
            DeviceArray((self.nf, self.nspec, self.n), np.float64),
            DeviceArray((npairs, self.n), np.int32) if npairs else None,
            DeviceArray((self.nf, 2 * npairs, self.n), np.float64) if npairs else None)

  def _launch(self, k0, k1, out=None, npairs=None):
    """The launch alone: (nused, psd, nused_pair, csd) on the device, nothing synchronised.  `out`:
    the arrays of an earlier call, written again; `npairs`: only the first so many pairs."""
    dev = self._upload()
    npairs = len(self.pairs) if npairs is None else npairs
    d = _lib.pm_series_spectra()
    d.n, d.nspec, d.nrec, d.k0, d.k1 = self.n, self.nspec, self.nrec, k0, k1
    d.nperseg, d.step, d.detrend, d.npairs = self.nperseg, self.step, _DETREND[self.detrend], npairs
    d.v, d.window, d.window_dev, d.twiddle = (self._series.ptr, self._w.ctypes.data, dev["w"].ptr,
                                              dev["tw"].ptr)
    d.pair, d.pair_dev, d.scale = self._pair.ctypes.data, dev["pair"].ptr, self._scale
    if out is None:
      out = self._alloc(npairs)
    with launch_span(self._timer(), "k_series_spectra", self.stream):
      check(lib.pm_series_spectra(C.byref(d), out[0].ptr, out[1].ptr,
                                  out[2].ptr if npairs else None, out[3].ptr if npairs else None,
                                  _sh(self.stream)))
    return out

  def compute(self, k0=0, k1=None):
    k0, k1 = self._window(k0, k1)
    nused, psd, nused_pair, csd = self._launch(k0, k1)
    get = lambda a: a.download(stream=self.stream)  # noqa: E731
    if self.pairs:
      nused_pair, csd = get(nused_pair), get(csd)
    return Spectra(self.names, self.pairs, self.freq.copy(), get(nused), get(psd), nused_pair, csd)

  def across_members(self, k0=0, k1=None, quantiles=()):
    """The statistics, across the members of every group, of the power spectra as a series with
    the frequency for its record: a `stats.GroupStats` whose arrays are [ngroups, nf] (quantile:
    [nq, ngroups, nf]).  A member with no used segment has a NaN spectrum: SeriesStats excludes
    and counts it."""
    k0, k1 = self._window(k0, k1)
    out = self._alloc(0)
    # (its argument checks come before the launch)
    st = SeriesStats((out[1], self.names), groups=self.groups, quantiles=quantiles,
                     stream=self.stream)
    self.group_labels = st.group_labels
    self._launch(k0, k1, out=out, npairs=0)
    return st.across_members()
