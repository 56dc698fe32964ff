"""SeriesSmooth: Gaussian-kernel detrending of a recorded index series, on the device.

The early-warning method as published (Dakos et al. 2008, Lenton et al. 2012, Boers 2021; R's
earlywarnings::generic_ews) removes a kernel-smoothed trend from the WHOLE record before any
window is cut; it does not remove a straight line inside each window.  Under a ramp towards a
transition the index curves, a per-window line leaves that curvature in the residual, and the
curvature inflates variance and lag-1 autocorrelation towards the end of the record -- the very
signal one is looking for.  `SeriesSmooth` computes, for every (index, member) series an
`IndexRecorder` keeps on the device ([n_samples][nspec][n]), the smoothed trend and the residual
of a record window in ONE launch where the series lives (pm_series_smooth, csrc/smooth.hip), each
a device series [K, nspec, n] that `SeriesWindows`, `SeriesStats`, `SeriesSpectra` and
`SeriesSurrogates` take as a source unchanged.

  trend(k0, k1)      (DeviceArray [K, nspec, n], names): the smoothed series, one launch
  residual(k0, k1)   (DeviceArray [K, nspec, n], names): the series less its trend, one launch
  compute(k0, k1)    trend, resid [name] -> [n, K] and nbad [name] -> [n], downloaded

The weights are w[d] = exp(-0.5 (d / sigma)^2), d <= H = int(truncate * sigma + 0.5) -- SciPy's
gaussian_filter1d radius -- formed on the host; the device evaluates no exp.  The edges are
renormalised by the weights in reach (Nadaraya-Watson, as R's ksmooth; `sigma_of_ksmooth` converts
its bandwidth), not reflected.  A non-finite record is left out and counted (`nbad`), never
propagated: the trend there is the gap-filled value from its neighbours, the residual NaN, which
every later stage excludes and counts by its own rule.  The definition is two sequential sums per
record with the op order include/pymoc_hip.h states, so every double equals the NumPy restatement
(tests/smooth_cases.py) bit for bit.  What a source and a record window [k0, k1) are: series.py.

Out of scope:
  * skewness and higher moments;
  * other kernels (Epanechnikov, loess) -- the entry takes any non-increasing positive table, this
    class forms the Gaussian one;
  * ARMA orders above 1;
  * record windows of more than 4096 records;
  * smoothing across ranks: every rank treats its own members;
  * online smoothing: the series is smoothed after the samples;
  * smoothing of `pos` (the positions an IndexRecorder keeps next to the values);
  * any change to `SeriesSpectra`'s own detrending: hand it a residual source.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Series, by_name

TRUNCATE_MIN, TRUNCATE_MAX = 1.0, 8.0


def sigma_of_ksmooth(bandwidth):
  """The sigma of R's ksmooth(kernel = "normal", bandwidth): its kernel's quartiles lie at
  +-0.25 bandwidth, so sigma = 0.25 bandwidth / qnorm(0.75)."""
  return 0.25 * float(bandwidth) / 0.6744897501960817


def half_width(sigma, truncate=4.0):
  """(sigma, truncate, H) checked: sigma a number > 0, truncate in [1, 8], H = int(truncate *
  sigma + 0.5) in [1, 4095]."""
  for what, val in (("sigma", sigma), ("truncate", truncate)):
    if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)):
      raise ValueError("%s must be a number (%r here)" % (what, val))
  sigma, truncate = float(sigma), float(truncate)
  if not (np.isfinite(sigma) and sigma > 0.0):
    raise ValueError("sigma must be finite and > 0 (%r here)" % sigma)
  if not TRUNCATE_MIN <= truncate <= TRUNCATE_MAX:
    raise ValueError("truncate must lie in [%g, %g] (%r here)"
                     % (TRUNCATE_MIN, TRUNCATE_MAX, truncate))
  H = int(truncate * sigma + 0.5)
  if not 1 <= H <= _lib.PM_SMOOTH_HALF_MAX:
    raise ValueError("the half-width int(truncate * sigma + 0.5) = %d is outside [1, %d]"
                     % (H, _lib.PM_SMOOTH_HALF_MAX))
  return sigma, truncate, H


def gaussian_weights(sigma, H):
  """w[d] = exp(-0.5 (d / sigma)^2), d = 0 .. H."""
  return np.exp(-0.5 * (np.arange(H + 1, dtype=np.float64) / sigma) ** 2)


class Weights(object):
  """What a smoother launch takes besides the series: `half`, the table w[0 .. half] on the `host`
  (the entry checks it there) and its device copy, uploaded once, at the first launch."""

  def __init__(self, sigma, half):
    self.half, self.host, self._dev = half, gaussian_weights(sigma, half), None

  def dev(self, stream):
    if self._dev is None:
      self._dev = DeviceArray.from_host(self.host, dtype=np.float64, stream=stream)
    return self._dev


def launch_smooth(x, k0, k1, w, ctx, trend=None, resid=None, nbad=None):
  """pm_series_smooth over the records [k0, k1) of the device view `x` with the `Weights` w, into
  the given device arrays (trend or resid may be None): nbad [nspec, n] on the device (allocated
  here unless given), nothing synchronised."""
  d = _lib.pm_series_smooth()
  (d.nrec, d.nspec, d.n), d.k0, d.k1, d.half = x.shape, k0, k1, w.half
  d.v, d.w, d.w_dev = x.ptr, w.host.ctypes.data, w.dev(ctx.stream).ptr
  if nbad is None:
    nbad = DeviceArray(x.shape[1:], np.int32)
  with launch_span(ctx.timer, "k_series_smooth", ctx.stream):
    check(lib.pm_series_smooth(C.byref(d), None if trend is None else trend.ptr,
                               None if resid is None else resid.ptr, nbad.ptr, _sh(ctx.stream)))
  return nbad


class Smoothed(object):
  """What `compute` returns: trend, resid `[name] -> [n, K]` and nbad `[name] -> [n]`."""

  def __init__(self, names, trend, resid, nbad):
    self.names = list(names)
    self.trend, self.resid = (by_name(self.names, a.transpose(1, 2, 0)) for a in (trend, resid))
    self.nbad = by_name(self.names, nbad)


class SeriesSmooth(Series):
  """`SeriesSmooth(source, sigma, truncate=4.0, stream=None)`.

  source    an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  sigma     the Gaussian's standard deviation in records, a float > 0
  truncate  the half-width in sigmas, in [1, 8]; H = int(truncate * sigma + 0.5) in [1, 4095]

  A record window [k0, k1) holds at most 4096 records."""

  def __init__(self, source, sigma, truncate=4.0, stream=None):
    Series.__init__(self, source, stream)
    if self.nspec > 65535:
      raise ValueError("nspec = %d is above 65535" % self.nspec)
    self.sigma, self.truncate, self.half = half_width(sigma, truncate)
    self._w = Weights(self.sigma, self.half)
    self.weights = self._w.host

  def _window(self, k0, k1):
    k0, k1 = self._record_window(k0, k1)
    if k1 - k0 > _lib.PM_SMOOTH_MAX:
      raise ValueError("window [%d, %d) holds %d records, more than %d"
                       % (k0, k1, k1 - k0, _lib.PM_SMOOTH_MAX))
    return k0, k1

  def _launch(self, k0, k1, trend=None, resid=None, nbad=None):
    """The launch alone into the given device arrays (trend or resid may be None): nbad on the
    device, nothing synchronised."""
    return launch_smooth(self._series, k0, k1, self._w, self._ctx(), trend, resid, nbad)

  def _alloc(self, K):
    return DeviceArray((K, self.nspec, self.n), np.float64)

  def trend(self, k0=0, k1=None):
    """The smoothed series of the record window: (DeviceArray [K, nspec, n], names), a source of
    its own (pass `stream=` this object's stream with it); one launch, nothing synchronised."""
    k0, k1 = self._window(k0, k1)
    out = self._alloc(k1 - k0)
    self._launch(k0, k1, trend=out)
    return out, list(self.names)

  def residual(self, k0=0, k1=None):
    """The series less its smoothed trend, NaN at a non-finite record: as `trend`."""
    k0, k1 = self._window(k0, k1)
    out = self._alloc(k1 - k0)
    self._launch(k0, k1, resid=out)
    return out, list(self.names)

  def compute(self, k0=0, k1=None):
    """One launch, then the download of all three: a `Smoothed`."""
    k0, k1 = self._window(k0, k1)
    trend, resid = self._alloc(k1 - k0), self._alloc(k1 - k0)
    nbad = self._launch(k0, k1, trend=trend, resid=resid)
    return Smoothed(self.names, trend.download(stream=self.stream),
                    resid.download(stream=self.stream), nbad.download(stream=self.stream))
