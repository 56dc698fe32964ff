"""SeriesWindows: sliding-window early-warning indicators of a recorded index series, on the device.

A ramped noise ensemble is run to see whether the fluctuations of an index slow down and grow as
a transition comes near: critical slowing down, read from the lag-1 autocorrelation and the
variance of the detrended index in a sliding window, each followed through time and summarised by
Kendall's tau of the indicator against time.  `SeriesWindows` computes, for every (index, member)
series an `IndexRecorder` keeps on the device ([n_samples][nspec][n]), the mean, the linear slope,
the variance and the lagged autocorrelation of every sliding window in ONE launch where the series
lives (pm_series_windows, csrc/windows.hip), and the Kendall counts of a series against its record
number in one more (pm_series_kendall); only the results are downloaded.

  compute(k0, k1)          mean, slope, var, ac [name] -> [n, nwin] and nused[name] -> [n]
  across_members(which)    the launch, then the indicator as a device series [nwin][nspec][n]
                           through SeriesStats.across_members: the group mean and the quantile
                           bands per window, no per-member indicator downloaded
  trend(k0, k1)            the launch, then pm_series_kendall over the var and the ac series on the
                           device: tau, conc, disc, tie, nfin [name] -> [n]; only the counts are
                           downloaded
  kendall(source, k0, k1)  the same counts and tau of any device series
  significance(k0, k1, nsur)
                           the surrogate test of `trend`: AR(1) surrogates (or, method="fourier",
                           Fourier phase-randomised ones) generated on the device
                           (surrogates.py), each through the same two launches, and a counting
                           launch; p_rising, p_falling and the three counts [name] -> [n];
                           `until=`: up to every member's own end (shifts.py)

A window with a non-finite value is excluded and counted (`nused`), never propagated: its four
indicators are NaN, which `across_members` and `trend` exclude and count in turn.  The definition
is per window, two sequential passes with the op order include/pymoc_hip.h states, so every double
equals the NumPy restatement (tests/windows_cases.py) bit for bit; the Kendall counts are exact
integers.  `ac` is the biased autocorrelation estimate (R's acf, statsmodels), not the Pearson
correlation of the shifted pair (pandas.Series.autocorr).  An indicator is dated at the END of its
window (`record_end`), the early-warning convention.  What a source and a record window [k0, k1)
are: series.py.

`detrend="gaussian"` is the published estimator: a Gaussian-kernel trend is removed from the whole
record window first (pm_series_smooth, smooth.py: one more launch, into a residual series of K
records allocated per call), and the windows are cut from the residual with only their mean
removed.  A record that is not finite has a NaN residual, so the windows that hold it are excluded
as before.

`dfa=True` (or a sequence of scales) adds the third indicator of Lenton et al. 2012, the exponent
alpha of detrended fluctuation analysis (Livina & Lenton 2007) of every window: one more launch
(pm_series_dfa, csrc/dfa.hip; dfa.py states what it is) on the same windows of the same series.
`compute` then also returns `dfa` [name] -> [n, nwin], `dfa_f2` [name] -> [n, nwin, nq] (the mean
squared fluctuation F2 at every scale) and `dfa_scales`; across_members("dfa") works as for the
four others; `trend()` and `significance()` gain `.dfa`.  Every F2 equals the restatement
(tests/dfa_cases.py) bit for bit; alpha goes through the device library's log and is held to a
bound.  Without `dfa` every method issues the launches it issued before.

`restoring=True` (or a number of iterations) adds Boers' own indicator, the restoring rate lambda of
every window: the increments of the detrended index regressed on the index with AR(1)-correlated
errors, by iterated generalised least squares -- one more launch (pm_series_restoring,
csrc/restoring.hip; restoring.py states what it is) on the same windows of the same series, after
the DFA launch.  lambda is per record interval (phi - 1 of an AR(1) state, -dt / tau of a
relaxation time tau) and rises towards 0 as stability is lost; unlike `ac` and `var` it does not
rise when the forcing noise merely gets redder.  `compute` then also returns `lam` and `lam_rho`
(the errors' lag-1 coefficient the stored lambda was fitted with) [name] -> [n, nwin];
across_members("lam") works as for the others; `trend()` and `significance()` gain `.lam`, after
`var`, `ac` and `dfa`.  Both equal the restatement (tests/restoring_cases.py) bit for bit.  Without
`restoring` every method issues the launches it issued before.

Every method goes through `indicators`, the one path from a device series to its indicator planes
(censor, smooth, the window launch, the DFA launch, the restoring launch), and `significance` sends the record and every
chunk of surrogates through it; `launch_windows` and `launch_kendall` are the launches alone, over any
device view (series.py).

Out of scope:
  * skewness and higher moments;
  * of DFA: backward boxes, orders above 1, overlapping boxes, rescaling alpha to Lenton's
    "propagator", DFA of `pos`;
  * of the restoring rate: AR orders of the errors above 1, online updating, the rate of `pos`,
    and identifiability where the noise is more persistent than the state (restoring.py);
  * of the surrogate test: ARMA orders above 1 (the parametric null model is AR(1)), `until=`
    with Fourier surrogates, amplitude-adjusted (AAFT / IAAFT) surrogates, and surrogates of
    `pos`;
  * anything across ranks: every rank treats its own members;
  * anything online: the indicators are computed from the recorded series, after the samples;
  * indicators of `pos` (the positions an IndexRecorder keeps next to the values);
  * linear detrending inside `SeriesSpectra`, which stays as it is.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .dfa import dfa_par, launch_dfa
from .restoring import launch_restoring, restoring_par
from .series import Series, _Plane, as_int, by_name, records
from .smooth import Weights, half_width, launch_smooth
from .stats import SeriesStats

_DETREND = dict(linear=_lib.PM_WIN_DETREND_LINEAR, constant=_lib.PM_WIN_DETREND_CONSTANT,
                none=_lib.PM_WIN_DETREND_NONE)
GAUSSIAN = "gaussian"  # a detrend of the classes, not of the entry: the smoother, then "constant"
INDICATORS = ("mean", "slope", "var", "ac")


def check_detrend(detrend, sigma, truncate):
  """A class's `detrend` with its `sigma` and `truncate`: (sigma, truncate, H) under "gaussian",
  None under the in-window detrends, which take no sigma."""
  if detrend != GAUSSIAN and detrend not in _DETREND:
    raise ValueError("unknown detrend %r (one of linear, constant, none, gaussian)" % (detrend,))
  if detrend != GAUSSIAN:
    if sigma is not None:
      raise ValueError("sigma is given (%r) but detrend is %r, not \"gaussian\"" % (sigma, detrend))
    return None
  if sigma is None:
    raise ValueError("detrend \"gaussian\" needs sigma, the kernel's width in records")
  return half_width(sigma, truncate)


def stt_of(W):
  """sum t_j^2 = W (W^2 - 1) / 12 of t_j = j - (W - 1) / 2: a multiple of a half below 2^53 (a
  whole number unless W = 2 mod 4), so exact -- the value the entry forms and checks."""
  W = int(W)
  return float(W * (W * W - 1)) / 12.0


def tau_b(conc, disc, tie):
  """Kendall's tau-b against time, which has no ties, from the pair counts: (conc - disc) /
  sqrt(n0 * (n0 - tie)), n0 = conc + disc + tie; NaN for n0 == tie (no pair, or all equal)."""
  conc, disc, tie = (np.asarray(a, dtype=np.float64) for a in (conc, disc, tie))
  n0 = conc + disc + tie
  with np.errstate(all="ignore"):
    return (conc - disc) / np.sqrt(n0 * (n0 - tie))


class _Source(Series):
  """A source as the two kernels of this module take it: at most 65535 indices."""

  def __init__(self, source, stream=None):
    Series.__init__(self, source, stream)
    if self.nspec > 65535:
      raise ValueError("nspec = %d is above 65535" % self.nspec)


def launch_kendall(arr, shape, k0, k1, stream, timer, out=None):
  """pm_series_kendall over the records [k0, k1) of a device series: the four int32 [nspec, n]
  count arrays on the device, nothing synchronised.  `out`: the arrays of an earlier call, written
  again."""
  nrec, nspec, n = shape
  d = _lib.pm_series_kendall()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.v = n, nspec, nrec, k0, k1, arr.ptr
  if out is None:
    out = [DeviceArray((nspec, n), np.int32) for _ in range(4)]
  with launch_span(timer, "k_series_kendall", stream):
    check(lib.pm_series_kendall(C.byref(d), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                _sh(stream)))
  return out


WinPar = collections.namedtuple("WinPar", "window step lag detrend stt")


def win_par(window, step, lag, detrend):
  """What a window launch takes besides the series; "gaussian" is "constant" here, after the
  smoother."""
  return WinPar(window, step, lag, _DETREND["constant" if detrend == GAUSSIAN else detrend],
                stt_of(window))


def alloc_windows(nwin, nspec, n):
  """The outputs of a launch over `nwin` windows: (out [4, nwin, nspec, n], nused [nspec, n])."""
  return DeviceArray((4, nwin, nspec, n), np.float64), DeviceArray((nspec, n), np.int32)


def launch_windows(x, k0, k1, par, ctx, out=None):
  """pm_series_windows over the records [k0, k1) of the device view `x` with the `WinPar` par:
  (out [4, nwin, nspec, n], nused [nspec, n]) on the device, nothing synchronised.  `out`: the
  arrays of an earlier call (of at least this size), written again."""
  d = _lib.pm_series_windows()
  (d.nrec, d.nspec, d.n), d.k0, d.k1 = x.shape, k0, k1
  d.window, d.step, d.lag, d.detrend, d.stt = par
  d.v = x.ptr
  if out is None:
    out = alloc_windows((k1 - k0 - par.window) // par.step + 1, *x.shape[1:])
  with launch_span(ctx.timer, "k_series_windows", ctx.stream):
    check(lib.pm_series_windows(C.byref(d), out[0].ptr, out[1].ptr, _sh(ctx.stream)))
  return out


def indicators(x, k0, k1, par, ctx, cens=None, into=None, weights=None, resid=None, nbad=None,
               out=None, dfa=None, alpha=None, f2=None, restoring=None, lam=None, rho=None):
  """The one path from a device series to its indicator planes, for the record and for a chunk of
  surrogates alike: over the records [k0, k1) of the view `x` (K records, any number of planes)
    1. pm_series_censor with the `shifts.Censor` cens, when one is given: into `into` (x itself:
       in place; None: a copy of K records allocated here);
    2. pm_series_smooth with the `smooth.Weights` weights, when they are given: the residual into
       `resid` (None: allocated here), the count into `nbad`;
    3. pm_series_windows with `par` into `out` (as `launch_windows`);
    4. pm_series_dfa with `par` and the `dfa.DfaPar` dfa, when one is given, on the view step 3
       reads: into `alpha` and `f2` (as `dfa.launch_dfa`);
    5. pm_series_restoring with `par` and the `restoring.RestoringPar` restoring, when one is
       given, on the same view: into `lam` and `rho` (as `restoring.launch_restoring`).
  Returns ((out, nused), (series, r0, r1)): the planes, and the records the windows were cut from,
  which a null-model fit reads; with `dfa`, (alpha, f2) as a third; with `restoring`, (lam, rho)
  as the last.  Nothing is synchronised."""
  K, planes = k1 - k0, tuple(x.shape[1:])
  if cens is not None:
    from .shifts import launch_censor  # (shifts derives from this module)
    into = DeviceArray((K,) + planes, np.float64) if into is None else into
    launch_censor(records(x, k0, k1), into, cens, ctx)
    x, k0, k1 = into, 0, K
  if weights is not None:
    resid = DeviceArray((K,) + planes, np.float64) if resid is None else resid
    launch_smooth(x, k0, k1, weights, ctx, resid=resid, nbad=nbad)
    x, k0, k1 = resid, 0, K
  res = launch_windows(x, k0, k1, par, ctx, out=out), (x, k0, k1)
  if dfa is not None:
    res += (launch_dfa(x, k0, k1, par, dfa, ctx, alpha=alpha, f2=f2),)
  if restoring is not None:
    res += (launch_restoring(x, k0, k1, par, restoring, ctx, lam=lam, rho=rho),)
  return res


class Trend(object):
  """Kendall's tau of a series against its record number and the counts it is formed from: tau,
  conc, disc, tie, nfin, each `[name] -> [n]`."""

  def __init__(self, names, conc, disc, tie, nfin):
    self.names = list(names)
    self.conc, self.disc, self.tie, self.nfin = (by_name(self.names, a)
                                                 for a in (conc, disc, tie, nfin))
    self.tau = by_name(self.names, tau_b(conc, disc, tie))


def kendall(source, k0=0, k1=None, stream=None):
  """The `Trend` of any device series over the records [k0, k1) (at most 4096 of them): one launch
  of pm_series_kendall and the download of the counts.  `source` as for `SeriesWindows`."""
  src = _Source(source, stream)
  k0, k1 = src._record_window(k0, k1)
  if k1 - k0 > _lib.PM_KENDALL_MAX:
    raise ValueError("window [%d, %d) holds %d records, more than %d"
                     % (k0, k1, k1 - k0, _lib.PM_KENDALL_MAX))
  out = launch_kendall(src._series, (src.nrec, src.nspec, src.n), k0, k1, src.stream, src._timer())
  return Trend(src.names, *(a.download(stream=src.stream) for a in out))


class Windows(object):
  """What `compute` returns: mean, slope, var, ac `[name] -> [n, nwin]`, nused `[name] -> [n]` and
  record_end [nwin]; with `dfa`, also dfa `[name] -> [n, nwin]`, dfa_f2 `[name] -> [n, nwin, nq]`
  and dfa_scales; with `restoring`, also lam and lam_rho `[name] -> [n, nwin]`."""

  def __init__(self, names, record_end, out, nused, dfa=None, restoring=None):
    # out [4, nwin, nspec, n]; dfa = (scales, alpha [nwin, nspec, n], f2 [nq, nwin, nspec, n]);
    # restoring = (lam, rho), each [nwin, nspec, n]
    self.names, self.record_end = list(names), record_end
    for i, key in enumerate(INDICATORS):
      setattr(self, key, by_name(self.names, out[i].transpose(1, 2, 0)))
    self.nused = by_name(self.names, nused)
    if dfa is not None:
      self.dfa_scales = tuple(dfa[0])
      self.dfa = by_name(self.names, dfa[1].transpose(1, 2, 0))
      self.dfa_f2 = by_name(self.names, dfa[2].transpose(2, 3, 1, 0))
    if restoring is not None:
      self.lam = by_name(self.names, restoring[0].transpose(1, 2, 0))
      self.lam_rho = by_name(self.names, restoring[1].transpose(1, 2, 0))


class WindowTrend(object):
  """What `trend` returns: `.var` and `.ac`, a `Trend` each; with `dfa`, also `.dfa`; with
  `restoring`, also `.lam`."""

  def __init__(self, var, ac, dfa=None, lam=None):
    self.var, self.ac = var, ac
    if dfa is not None:
      self.dfa = dfa
    if lam is not None:
      self.lam = lam


class SeriesWindows(_Source):
  """`SeriesWindows(source, window, step=1, detrend="linear", lag=1, groups=None, stream=None,
  sigma=None, truncate=4.0, dfa=None, restoring=None)`.

  source    an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  window    W, the records of a window, in [4, 4096]; any integer
  step      S, the records between the starts of two consecutive windows, in [1, W]
  detrend   "linear" (the window's least-squares line is removed), "constant" (its mean), "none",
            or "gaussian": a Gaussian-kernel trend is removed from the whole record window before
            the windows are cut, then each window's mean
  sigma     under "gaussian" (and only there): the kernel's standard deviation in records
  truncate  its half-width in sigmas, in [1, 8] (smooth.py); K <= 4096 under "gaussian"
  lag       Lg of the autocorrelation, in [1, W - 2]
  groups    int array [n] of labels, for `across_members` (as SeriesStats)
  dfa       None, True (the scales `dfa.default_scales(W)`) or a sequence of 2 to 16 strictly
            ascending integer scales, 4 <= s and 4 s <= W: the DFA exponent of every window as a
            fifth indicator, "dfa" -- one more launch (pm_series_dfa) per call
  restoring None, True (10 iterations, the published setting) or the number of iterations, 1 to
            64; W >= 8: the restoring rate lambda of every window under AR(1)-correlated errors
            (restoring.py), per record interval, as a further indicator, "lam" -- one more launch
            (pm_series_restoring) per call

  Each call of `compute` / `across_members` / `trend` is one launch of pm_series_windows on the
  source's stream (and what follows it on the device), after one of pm_series_smooth under
  "gaussian".  [k0, k1) is a record window (series.py)
  of at least W records."""

  def __init__(self, source, window, step=1, detrend="linear", lag=1, groups=None, stream=None,
               sigma=None, truncate=4.0, dfa=None, restoring=None):
    _Source.__init__(self, source, stream)
    W, S, Lg = as_int("window", window), as_int("step", step), as_int("lag", lag)
    if not _lib.PM_WIN_MIN <= W <= _lib.PM_WIN_MAX:
      raise ValueError("window must lie in [%d, %d] (%d here)"
                       % (_lib.PM_WIN_MIN, _lib.PM_WIN_MAX, W))
    if not 1 <= S <= W:
      raise ValueError("step must lie in [1, window = %d] (%d here)" % (W, S))
    if not 1 <= Lg <= W - 2:
      raise ValueError("lag must lie in [1, window - 2 = %d] (%d here)" % (W - 2, Lg))
    self._smooth = check_detrend(detrend, sigma, truncate)
    self._weights = Weights(self._smooth[0], self._smooth[2]) if self._smooth else None
    self._par = win_par(W, S, Lg, detrend)
    self._dfa = None if dfa is None else dfa_par(W, dfa)
    self.dfa_scales = None if dfa is None else self._dfa.scales
    self._restoring = None if restoring is None else restoring_par(W, restoring)
    self._fourier_tables = {}  # per K, for significance(method="fourier")
    self.window, self.step, self.lag, self.detrend, self.stt = W, S, Lg, detrend, self._par.stt
    self._set_groups(groups)  # checked now, used by across_members

  def _window(self, k0, k1):
    k0, k1 = self._record_window(k0, k1)
    if k1 - k0 < self.window:
      raise ValueError("window [%d, %d) holds %d records, fewer than the window length %d"
                       % (k0, k1, k1 - k0, self.window))
    if self._smooth and k1 - k0 > _lib.PM_SMOOTH_MAX:
      raise ValueError("window [%d, %d) holds %d records, more than the %d \"gaussian\" takes"
                       % (k0, k1, k1 - k0, _lib.PM_SMOOTH_MAX))
    nwin = (k1 - k0 - self.window) // self.step + 1
    if nwin * self.nspec >= 1 << 30:
      raise ValueError("nwin * nspec = %d is not below 2^30" % (nwin * self.nspec))
    return k0, k1, nwin

  def nwin(self, k0=0, k1=None):
    """The number of whole windows the record window [k0, k1) holds."""
    return self._window(k0, k1)[2]

  def record_end(self, k0=0, k1=None):
    """The absolute record number of every window's last record [nwin]."""
    k0, k1, nwin = self._window(k0, k1)
    return k0 + np.arange(nwin) * self.step + self.window - 1

  def _trend_window(self, k0, k1):
    """`_window` where the indicator series goes through pm_series_kendall."""
    k0, k1, nwin = self._window(k0, k1)
    if nwin > _lib.PM_KENDALL_MAX:
      raise ValueError("the record window [%d, %d) holds %d windows, more than %d"
                       % (k0, k1, nwin, _lib.PM_KENDALL_MAX))
    return k0, k1, nwin

  def _alloc(self, nwin):
    return alloc_windows(nwin, self.nspec, self.n)

  def _launch(self, k0, k1, nwin, out=None):
    """The window launch alone on the source series, nothing synchronised: `launch_windows`."""
    return launch_windows(self._series, k0, k1, self._par, self._ctx(), out=out)

  def _indicators(self, k0, k1, **kw):
    """`indicators` of the source series with this object's settings (its `dfa` among them: a
    third result then; and its `restoring`: a last one)."""
    return indicators(self._series, k0, k1, self._par, self._ctx(), weights=self._weights,
                      dfa=self._dfa, restoring=self._restoring, **kw)

  def compute(self, k0=0, k1=None):
    k0, k1, nwin = self._window(k0, k1)
    res = self._indicators(k0, k1, f2=True if self._dfa else None,
                           rho=True if self._restoring else None)
    out, nused = res[0]
    dfa = restoring = None
    if self._dfa:
      dfa = (self._dfa.scales,) + tuple(a.download(stream=self.stream) for a in res[2])
    if self._restoring:
      restoring = tuple(a.download(stream=self.stream) for a in res[-1])
    return Windows(self.names, k0 + np.arange(nwin) * self.step + self.window - 1,
                   out.download(stream=self.stream), nused.download(stream=self.stream), dfa,
                   restoring)

  def across_members(self, which, k0=0, k1=None, quantiles=()):
    """The statistics, across the members of every group, of the indicator `which` ("mean",
    "slope", "var", "ac", with `dfa` "dfa", with `restoring` "lam") as a series with the window for its record: a `stats.GroupStats` whose
    arrays are [ngroups, nwin] (quantile: [nq, ngroups, nwin]).  A member's unused window is NaN:
    SeriesStats excludes and counts it."""
    known = (INDICATORS + (("dfa",) if self._dfa else ())
             + (("lam",) if self._restoring else ()))
    if which not in known:
      raise ValueError("unknown indicator %r (one of %s)" % (which, ", ".join(known)))
    k0, k1, nwin = self._window(k0, k1)
    out = self._alloc(nwin)
    # (its argument checks come before the launch)
    kw, shape = dict(out=out), (nwin, self.nspec, self.n)
    if which == "dfa":
      kw["alpha"] = DeviceArray(shape, np.float64)
      view = _Plane(kw["alpha"], 0, shape)
    elif which == "lam":
      kw["lam"] = DeviceArray(shape, np.float64)
      view = _Plane(kw["lam"], 0, shape)
    else:
      view = _Plane(out[0], INDICATORS.index(which), shape)
    st = SeriesStats((view, self.names), groups=self.groups, quantiles=quantiles,
                     stream=self.stream)
    self.group_labels = st.group_labels
    self._indicators(k0, k1, **kw)
    return st.across_members()

  def trend(self, k0=0, k1=None):
    """Kendall's tau against time of the var and of the ac series of every (index, member): the
    launch, then pm_series_kendall over out[2] and out[3] on the device.  NaN windows (unused, or
    ac of a window without variance) are left out of the pairs and show in nfin."""
    k0, k1, nwin = self._trend_window(k0, k1)
    got = self._indicators(k0, k1)
    out = got[0][0]
    shape = (nwin, self.nspec, self.n)
    series = [_Plane(out, i, shape) for i in (2, 3)]
    if self._dfa:  # the alpha series, after the two others
      series.append(_Plane(got[2][0], 0, shape))
    if self._restoring:  # and the lambda series, after them
      series.append(_Plane(got[-1][0], 0, shape))
    res = []
    for view in series:
      cnt = launch_kendall(view, shape, 0, nwin, self.stream, self._timer())
      res.append(Trend(self.names, *(a.download(stream=self.stream) for a in cnt)))
    return WindowTrend(res[0], res[1], dfa=res[2] if self._dfa else None,
                       lam=res[-1] if self._restoring else None)

  def significance(self, k0=0, k1=None, nsur=1000, seed=0, member0=None, max_bytes=2 << 30,
                   until=None, method="ar1"):
    """The surrogate test of `trend()`: `nsur` stationary AR(1) surrogates of every series, fitted
    to the record window under this object's detrend (surrogates.py), each through the identical
    window + Kendall pipeline, all on the device.  Returns a `surrogates.Significance`: `.var` and
    `.ac`, each with tau (observed), ge, le, nvalid, p_rising = (1 + ge) / (1 + nvalid) and
    p_falling = (1 + le) / (1 + nvalid) `[name] -> [n]`; p is NaN where the observed tau is NaN
    or no surrogate has one.

    The observed `trend` launches come first, then the fit; then, per chunk of
    min(remaining, max_bytes // (8 K nspec n), 65535 // nspec) surrogates, pm_series_surrogates,
    pm_series_windows, and pm_series_kendall + pm_series_exceed over the var and the ac planes, on
    the chunk's device arrays, which every chunk reuses; nothing is synchronised inside the loop
    and only the counts are downloaded.  The counts do not depend on the chunking.  `seed` and
    `member0` as for `SeriesSurrogates`; K = k1 - k0 <= 4096.

    Under "gaussian" the pipeline applied to a surrogate is literally the one applied to the
    record: the record window is smoothed once, the observed trends and the fit (one window,
    "constant") come from its residual, the surrogates are AR(1) surrogates of the residual, and
    every chunk goes through pm_series_smooth between pm_series_surrogates and pm_series_windows.
    A surrogate then counts 16 K nspec n bytes against max_bytes, the series plus its residual.

    `until`: a `SeriesShifts` (shifts.py) on which `detect()` and `censored()` have been called
    over the same record window -- the test of every member up to its own end.  The observed series
    is then the censored one (pm_series_censor; under "gaussian" smoothed afterwards), the fit is
    pm_series_fit_ranged over every member's records [k0, k0 + end) (of the censored series, or of
    its residual with "constant"), and every chunk goes through pm_series_censor in place, with
    the same ends, between pm_series_surrogates and what follows: a surrogate is cut where the
    record is.  Without `until` the launches are the ones listed above.

    `method`: "ar1" (the default: everything above) or "fourier", the nonparametric null: the fit
    is replaced by one launch of pm_series_fourier_coef on the same records (the DFT of their
    residual under the same inner detrend) and pm_series_surrogates by
    pm_series_surrogates_fourier, which rotates every coefficient's phase and transforms back
    (surrogates.py); every chunk then goes through the same launches with the same chunking --
    but that a surrogate of more than 512 records (M >= 2048) counts 16 K nspec n bytes against max_bytes as
    under "gaussian": the synthesis stores series-contiguously into a second array and transposes
    (under "gaussian" that array is the residual's).
    "fourier" together with `until=` is a ValueError: every member would be cut at its own end, so
    the transform length would be each member's own -- out of scope.

    With `dfa` the result also has `.dfa`, the same test of the trend of the DFA exponent: the
    observed alpha series and its Kendall counts next to the two others, and per chunk one more
    launch each of pm_series_dfa (alpha only: F2 is not stored), pm_series_kendall and
    pm_series_exceed, into a third triple of accumulators -- under either method, `until=` and
    "gaussian" alike, because it reads the series the window launch reads.  A surrogate costs what
    it cost against max_bytes (the chunk's window planes do not count, so neither does its alpha
    plane, 8 nwin nspec n bytes per surrogate next to their 32 nwin nspec n), and on the device
    one more pass over its windows: about 2 nq W / S reads of LDS per record, against 3 W / S
    for the var and ac planes.

    With `restoring` the result also has `.lam`, the same test of the trend of the restoring rate
    (per record interval), after the others: the observed lambda series and its Kendall counts,
    and per chunk one more launch each of pm_series_restoring (lam only: rho is not stored),
    pm_series_kendall and pm_series_exceed -- under either method, `until=` and "gaussian" alike,
    for the same reason.  Its plane, 8 nwin nspec n bytes per surrogate, does not count against
    max_bytes either; on the device it costs one more pass of 2 W / S reads of LDS per record."""
    from .surrogates import significance  # (surrogates derives from this module)
    return significance(self, k0, k1, nsur, seed, member0, max_bytes, until, method)

