"""SeriesSurrogates: stationary AR(1) surrogates, or Fourier phase-randomised surrogates, of a
recorded index series, generated on the device, and the counting behind
`SeriesWindows.significance`.

Kendall's tau of a sliding-window indicator means nothing by itself: overlapping windows make the
indicator series strongly serially correlated, and stationary red noise routinely gives |tau| of
0.5 and more.  The standard significance statement (Dakos et al. 2008, 2012; Boers 2021) is a
surrogate test: fit a stationary null model to the detrended series, generate many surrogate
series from it, run the identical window + Kendall pipeline on each, and report the fraction of
surrogates whose tau reaches the observed one.  Here the null model is AR(1): the fit is
pm_series_windows itself with ONE window spanning the record window (its `var` and lag-1 `ac` under
the class's `detrend`), and pm_series_surrogates (csrc/surrogates.hip) writes the surrogates as a
device series [K, nb * nspec, n] -- a source every `Series*` class accepts, so spectra or statistics
of surrogates can be taken too.  The surrogate series never exist on the host.

  fit(k0, k1)               the device `var` and `ac` [1, nspec, n] of the record window
  generate(k0, k1, b0, nb)  (DeviceArray [K, nb * nspec, n], names): the surrogates b0 .. b0 + nb - 1
                            of every series, named "%s#%d" % (name, b)

A surrogate depends on nothing but (seed, global member, b, index, record) and the two fit values:
not on n, the shard or the chunk [b0, b0 + nb) -- include/pymoc_hip.h states the definition,
tests/surrogate_cases.py restates it.  A series whose fit is not finite (a record window with a
non-finite value, a constant series) has NaN surrogates, which every later stage excludes and
counts by its own rule.  Under detrend "gaussian" the fit is the smoother (smooth.py) followed by
the one-window "constant" fit of its residual, and the surrogates are surrogates of that residual;
`significance` then sends every chunk through the same smoother.  With `until=` (shifts.py) the
test runs up to every member's own end: the record window censored, the fit per member over its
own records (pm_series_fit_ranged), every chunk censored in place.  The record and a chunk of
surrogates go through the same function, `windows.indicators`.  The deviates come from the
generator `NoiseForcing` uses; give the surrogates a seed of their own (the header says which
coordinates would coincide).

`method="fourier"` is the nonparametric null of the same papers: a surrogate keeps the whole
periodogram of the detrended record window and randomises only the phases, the null model of
choice where the index is not AR(1) (a spectral peak, a band-limited response).  In place of the
fit, pm_series_fourier_coef (csrc/fourier.hip) takes the DFT of the window's residual -- any K,
by Bluestein's chirp-z held in LDS -- and pm_series_surrogates_fourier rotates every coefficient
by a phase drawn from the same Philox generator and transforms back, into the same layout
[K, nb * nspec, n]; everything downstream is unchanged.  From 513 records on (M >= 2048, where a
block of the synthesis holds one series) the entry is given a scratch array of the chunk's size to
store series-contiguously and transpose from; `significance` counts it against max_bytes.

  coefficients(k0, k1)      the device planes (re, im), each [K / 2 + 1, nspec, n], of the DFT of
                            the record window's residual
  generate(k0, k1, b0, nb)  as above; `fit()` raises

The phase of a coefficient is one of 65536 values (the product of two table entries: the device
evaluates no sin or cos, so tests/fourier_cases.py restates every double bit for bit on the
tables of fourier.py, which are cached per K on the object).  Under "gaussian" the coefficients
are the "constant" coefficients of the smoother's residual, the composition the AR(1) fit uses.
A series with a non-finite record has NaN coefficients and NaN surrogates; a constant series has
zero coefficients and zero surrogates, whose indicators have no trend to count.

Out of scope for method="fourier": `until=` (the transform length would be each member's own),
amplitude-adjusted (AAFT / IAAFT) surrogates, packing two surrogates into one complex transform,
K > 4096, anything across ranks or online, and surrogates of `pos`.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import fourier
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Series, View, _Plane, as_int, by_name
from .shifts import launch_fit_ranged
from .smooth import Weights, launch_smooth
from .windows import (alloc_windows, check_detrend, indicators, launch_kendall, tau_b, win_par)

PLANES_MAX = 65535  # nb * nspec: the planes are the indices of the entries that read the series
METHODS = ("ar1", "fourier")


def check_method(method, until=None):
  """A null model's name; "fourier" takes no `until`."""
  if method not in METHODS:
    raise ValueError("unknown method %r (one of %s)" % (method, ", ".join(METHODS)))
  if method == "fourier" and until is not None:
    raise ValueError("method \"fourier\" does not take until=: every member would be cut at an "
                     "end of its own, so the transform length would be each member's own")
  return method


def as_seed(seed):
  seed = as_int("seed", seed)
  if not 0 <= seed < 1 << 64:
    raise ValueError("seed must lie in [0, 2^64) (%d here)" % seed)
  return seed


def as_member0(member0, rec):
  """`member0`, or for None the recorder's ensemble's first global member (0 without one)."""
  if member0 is None:
    return int(rec.ens._member0) if rec is not None else 0
  member0 = as_int("member0", member0)
  if member0 < 0:
    raise ValueError("member0 must not be negative (%d here)" % member0)
  return member0


def launch_exceed(obs, sur, shape, acc, stream, timer):
  """pm_series_exceed: the observed counts `obs` (conc, disc, tie [nspec, n]) against those of
  shape = (nb, nspec, n) surrogates, `sur`, added into acc = (ge, le, nvalid); nothing
  synchronised."""
  d = _lib.pm_series_exceed()
  d.nb, d.nspec, d.n = shape
  d.obs_conc, d.obs_disc, d.obs_tie = (a.ptr for a in obs[:3])
  d.sur_conc, d.sur_disc, d.sur_tie = (a.ptr for a in sur[:3])
  with launch_span(timer, "k_series_exceed", stream):
    check(lib.pm_series_exceed(C.byref(d), acc[0].ptr, acc[1].ptr, acc[2].ptr, _sh(stream)))


def launch_fit(x, k0, k1, detrend, ctx, weights=None, out=None):
  """The null model of the records [k0, k1) of the device view `x`: (var, ac), each a device
  series [1, nspec, n] -- `windows.indicators` with ONE window of K records, lag 1 (under `weights`
  the smoother's launch first, then the "constant" fit of its residual), nothing synchronised.
  `out`: the window outputs of an earlier call, written again."""
  (out, _), on = indicators(x, k0, k1, win_par(k1 - k0, 1, 1, detrend), ctx, weights=weights,
                            out=out)
  shape = (1,) + tuple(x.shape[1:])
  return _Plane(out, 2, shape, keep=on[:1]), _Plane(out, 3, shape, keep=on[:1])


def launch_surrogates(y, fit, b0, seed, member0, ctx, xi=None):
  """pm_series_surrogates: the surrogates b0 .. b0 + nb - 1 of the fit = (var, ac) [1, nspec, n]
  into the device view `y` [K, nb * nspec, n] (the deviates into `xi` when given); nothing
  synchronised."""
  d = _lib.pm_series_surrogates()
  d.K, d.nspec, d.n, d.b0 = y.shape[0], fit[0].shape[1], y.shape[2], b0
  d.nb = y.shape[1] // d.nspec
  d.member0, d.seed, d.var, d.ac = member0, seed, fit[0].ptr, fit[1].ptr
  with launch_span(ctx.timer, "k_series_surrogates", ctx.stream):
    check(lib.pm_series_surrogates(C.byref(d), y.ptr, None if xi is None else xi.ptr,
                                   _sh(ctx.stream)))


def launch_coefficients(x, k0, k1, detrend, tab, ctx, weights=None, out=None):
  """The Fourier coefficients of the records [k0, k1) of the device view `x` under the class
  detrend `detrend`: the device array [2, K / 2 + 1, nspec, n] of pm_series_fourier_coef (under
  `weights` the smoother's launch first, then the "constant" coefficients of its residual),
  nothing synchronised.  `out`: the array of an earlier call, written again."""
  K = k1 - k0
  if weights is not None:
    resid = DeviceArray((K,) + tuple(x.shape[1:]), np.float64)
    launch_smooth(x, k0, k1, weights, ctx, resid=resid)
    x, k0, k1 = resid, 0, K
  par = win_par(K, 1, 1, detrend)
  return fourier.launch_coef(x, k0, k1, par.detrend, par.stt, tab, ctx, out=out)


class SeriesSurrogates(Series):
  """`SeriesSurrogates(source, detrend="linear", seed=0, member0=None, stream=None, sigma=None,
  truncate=4.0, method="ar1")`.

  source    an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  detrend   what the fit removes from the record window first: "linear", "constant", "none", or
            "gaussian" (a Gaussian-kernel trend of `sigma` records, cut at `truncate` sigmas:
            smooth.py; then the mean) -- the surrogates are then surrogates of the residual
  seed      of the deviates, in [0, 2^64)
  member0   the global number of member 0; None: the recorder's ensemble's (what its NoiseForcing
            is bound with), 0 for a tuple source
  method    "ar1": stationary AR(1) surrogates of the fit; "fourier": phase-randomised surrogates
            of the residual's DFT (the phase one of 65536 values)

  A record window [k0, k1) holds K records, 4 <= K <= 4096."""

  def __init__(self, source, detrend="linear", seed=0, member0=None, stream=None, sigma=None,
               truncate=4.0, method="ar1"):
    Series.__init__(self, source, stream)
    self.method, self._tables = check_method(method), {}
    if self.nspec > PLANES_MAX:
      raise ValueError("nspec = %d is above %d" % (self.nspec, PLANES_MAX))
    self._smooth = check_detrend(detrend, sigma, truncate)
    self._weights = Weights(self._smooth[0], self._smooth[2]) if self._smooth else None
    self.detrend, self.seed = detrend, as_seed(seed)
    self.member0 = as_member0(member0, self._rec)

  def _window(self, k0, k1):
    k0, k1 = self._record_window(k0, k1)
    K = k1 - k0
    if not _lib.PM_WIN_MIN <= K <= _lib.PM_SURROGATE_MAX:
      raise ValueError("window [%d, %d) holds %d records: the fit takes %d to %d"
                       % (k0, k1, K, _lib.PM_WIN_MIN, _lib.PM_SURROGATE_MAX))
    return k0, k1, K

  def _chunk(self, b0, nb):
    b0, nb = as_int("b0", b0), as_int("nb", nb)
    if b0 < 0 or nb < 1 or b0 + nb > 1 << 32:
      raise ValueError("surrogates [%d, %d) are not a range inside [0, 2^32)" % (b0, b0 + nb))
    if nb * self.nspec > PLANES_MAX:
      raise ValueError("nb * nspec = %d is above %d" % (nb * self.nspec, PLANES_MAX))
    if nb * self.nspec * self.n >= 1 << 31:
      raise ValueError("nb * nspec * n = %d is not below 2^31" % (nb * self.nspec * self.n))
    return b0, nb

  def names_of(self, b0, nb):
    return ["%s#%d" % (nm, b) for b in range(b0, b0 + nb) for nm in self.names]

  def fit(self, k0=0, k1=None, out=None):
    """The null model of the record window: (var, ac), each a device series [1, nspec, n] -- one
    launch of pm_series_windows with one window of K records, lag 1, nothing synchronised.  Under
    "gaussian" the smoother's launch first, then the "constant" fit of its residual."""
    if self.method != "ar1":
      raise ValueError("method %r has no fit: see coefficients()" % (self.method,))
    k0, k1, K = self._window(k0, k1)
    return launch_fit(self._series, k0, k1, self.detrend, self._ctx(), self._weights, out)

  def tables(self, K):
    """The `fourier.Tables` of K records, made once per K."""
    return fourier.tables_of(self._tables, K)

  def _coefficients(self, k0, k1, K):
    return launch_coefficients(self._series, k0, k1, self.detrend, self.tables(K), self._ctx(),
                               self._weights)

  def coefficients(self, k0=0, k1=None):
    """method="fourier": the DFT of the record window's residual, (re, im), each a device series
    [K / 2 + 1, nspec, n] -- one launch of pm_series_fourier_coef, nothing synchronised.  Under
    "gaussian" the smoother's launch first, then the "constant" coefficients of its residual."""
    if self.method != "fourier":
      raise ValueError("method %r has no coefficients: see fit()" % (self.method,))
    k0, k1, K = self._window(k0, k1)
    coef = self._coefficients(k0, k1, K)
    shape = (K // 2 + 1, self.nspec, self.n)
    return _Plane(coef, 0, shape), _Plane(coef, 1, shape)

  def _launch(self, fit, K, b0, nb, y, xi=None):
    launch_surrogates(View(y.ptr, (K, nb * self.nspec, self.n)), fit, b0, self.seed, self.member0,
                      self._ctx(), xi)

  def generate(self, k0=0, k1=None, b0=0, nb=1):
    """The surrogates b0 .. b0 + nb - 1 of the record window [k0, k1): the fit, then one launch of
    pm_series_surrogates (method="fourier": the coefficients, then one launch of
    pm_series_surrogates_fourier).  Returns (DeviceArray [K, nb * nspec, n], names), a source of
    its own (pass `stream=` this object's stream with it)."""
    k0, k1, K = self._window(k0, k1)
    b0, nb = self._chunk(b0, nb)
    y = DeviceArray((K, nb * self.nspec, self.n), np.float64)
    if self.method == "fourier":
      scratch = DeviceArray(y.shape, np.float64) if fourier.wants_scratch(K) else None
      fourier.launch_synthesis(y, self._coefficients(k0, k1, K), self.nspec, b0, self.seed,
                               self.member0, self.tables(K), self._ctx(), scratch)
      return y, self.names_of(b0, nb)
    fit = self.fit(k0, k1)
    self._launch(fit, K, b0, nb, y)
    return y, self.names_of(b0, nb)


class TrendSignificance(object):
  """The surrogate test of one indicator's trend, each `[name] -> [n]`: the observed `tau`; among
  the `nvalid` surrogates with a tau, `ge` have tau >= the observed one and `le` tau <= it;
  `p_rising = (1 + ge) / (1 + nvalid)` and `p_falling = (1 + le) / (1 + nvalid)`, NaN where the
  observed tau is NaN or nvalid is 0."""

  def __init__(self, names, obs, ge, le, nvalid):
    self.names = list(names)
    tau = tau_b(*obs)
    none = np.isnan(tau) | (nvalid == 0)
    with np.errstate(all="ignore"):
      p = [np.where(none, np.nan, (1.0 + c) / (1.0 + nvalid)) for c in (ge, le)]
    self.tau, self.ge, self.le, self.nvalid, self.p_rising, self.p_falling = (
        by_name(self.names, a) for a in (tau, ge, le, nvalid, p[0], p[1]))


class Significance(object):
  """What `SeriesWindows.significance` returns: `.var` and `.ac`, a `TrendSignificance` each, and
  `nsur`; with the windows' `dfa`, also `.dfa`; with their `restoring`, also `.lam`."""

  def __init__(self, var, ac, nsur, dfa=None, lam=None):
    self.var, self.ac, self.nsur = var, ac, nsur
    if dfa is not None:
      self.dfa = dfa
    if lam is not None:
      self.lam = lam


def chunk_size(nsur, max_bytes, K, nspec, n, per=8):
  """The surrogates of one chunk: what max_bytes holds of per K nspec n bytes each (8; 16 under
  "gaussian", the series plus its residual), at most 65535 // nspec and nsur."""
  nb = min(nsur, max_bytes // (per * K * nspec * n), PLANES_MAX // nspec,
           ((1 << 31) - 1) // (nspec * n))
  if nb < 1:
    raise ValueError("max_bytes = %d does not hold one surrogate of %d bytes (or nspec * n = %d "
                     "is not below 2^31)" % (max_bytes, per * K * nspec * n, nspec * n))
  return nb


def significance(sw, k0, k1, nsur, seed, member0, max_bytes, until=None, method="ar1"):
  """`SeriesWindows.significance` (windows.py states what it does)."""
  check_method(method, until)
  nsur, max_bytes = as_int("nsur", nsur), as_int("max_bytes", max_bytes)
  seed, member0 = as_seed(seed), as_member0(member0, sw._rec)
  k0, k1, nwin = sw._trend_window(k0, k1)
  K = k1 - k0
  if K > _lib.PM_SURROGATE_MAX:
    raise ValueError("the record window [%d, %d) holds %d records, more than %d"
                     % (k0, k1, K, _lib.PM_SURROGATE_MAX))
  if nsur < 1:
    raise ValueError("nsur must be at least 1 (%d here)" % nsur)
  nspec, n, gauss, cens = sw.nspec, sw.n, sw._weights, None
  ctx = stream, timer = sw._ctx()
  if until is not None:  # the same test of the censored record window
    until._until(sw, k0, k1)
    cens = until._cens
  # (a Fourier chunk of more than 512 records holds a second array to transpose from: under
  # "gaussian" the residual's, which the smoother writes afterwards)
  two = method == "fourier" and fourier.wants_scratch(K)
  nbmax = chunk_size(nsur, max_bytes, K, nspec, n, per=16 if gauss or two else 8)
  # 1. the observed trends: `indicators` of the record window (censored into a copy)
  got = sw._indicators(k0, k1, cens=cens)
  (out, _), on = got[:2]
  shape = (nwin, nspec, n)
  series = [_Plane(out, i, shape) for i in (2, 3)]
  if sw._dfa:  # the observed alpha series, after the two others
    series.append(_Plane(got[2][0], 0, shape))
  if sw._restoring:  # and the observed lambda series, after them
    series.append(_Plane(got[-1][0], 0, shape))
  obs = [launch_kendall(view, shape, 0, nwin, stream, timer) for view in series]
  # 2. the fit of what the windows were cut from (`on`), and the zeroed accumulators
  inner = "constant" if gauss else sw.detrend  # (under "gaussian" `on` is the residual)
  if method == "fourier":  # in place of the fit: the coefficients of the same records
    tab = fourier.tables_of(sw._fourier_tables, K)  # (K >= W >= PM_WIN_MIN)
    coef = launch_coefficients(on[0], on[1], on[2], inner, tab, ctx)
  elif until is None:
    fit = launch_fit(on[0], on[1], on[2], inner, ctx)
  else:  # per member, over its records before its end
    fit = launch_fit_ranged(on[0], on[0].shape, on[1], on[2], inner, until.end, stream, timer)
  acc = [[DeviceArray.zeros((nspec, n), np.int32, stream=stream) for _ in range(3)]
         for _ in obs]
  # 3. chunk by chunk on arrays allocated once for the largest: `indicators` of the surrogates
  y =DeviceArray((K, nbmax * nspec, n), np.float64)
  yres = DeviceArray((K, nbmax * nspec, n), np.float64) if gauss or two else None
  nbad = DeviceArray((nbmax * nspec, n), np.int32) if gauss else None
  wout = alloc_windows(nwin, nbmax * nspec, n)
  walpha = DeviceArray((nwin, nbmax * nspec, n), np.float64) if sw._dfa else None
  wlam = DeviceArray((nwin, nbmax * nspec, n), np.float64) if sw._restoring else None
  cnt = [DeviceArray((nbmax * nspec, n), np.int32) for _ in range(4)]
  for b0 in range(0, nsur, nbmax):
    nb = min(nbmax, nsur - b0)
    planes = nb * nspec
    ych = _Plane(y, 0, (K, planes, n))
    if method == "fourier":
      fourier.launch_synthesis(ych, coef, nspec, b0, seed, member0, tab, ctx, yres if two else None)
    else:
      launch_surrogates(ych, fit, b0, seed, member0, ctx)
    # (cut where the record is, in place; the same smoother the record went through)
    indicators(ych, 0, K, sw._par, ctx, cens=cens, into=ych, weights=gauss,
               resid=_Plane(yres, 0, ych.shape) if gauss else None, nbad=nbad, out=wout,
               dfa=sw._dfa, alpha=walpha, restoring=sw._restoring, lam=wlam)
    wshape = (nwin, planes, n)
    series = [_Plane(wout[0], which, wshape) for which in (2, 3)]
    if sw._dfa:
      series.append(_Plane(walpha, 0, wshape))
    if sw._restoring:
      series.append(_Plane(wlam, 0, wshape))
    for i, view in enumerate(series):
      launch_kendall(view, wshape, 0, nwin, stream, timer, out=cnt)
      launch_exceed(obs[i], cnt, (nb, nspec, n), acc[i], stream, timer)
  # 4. the counts, and nothing else
  res = []
  for i in range(len(obs)):
    o = [a.download(stream=stream) for a in obs[i][:3]]
    ge, le, nvalid = (a.download(stream=stream) for a in acc[i])
    res.append(TrendSignificance(sw.names, o, ge, le, nvalid))
  return Significance(res[0], res[1], nsur, dfa=res[2] if sw._dfa else None,
                      lam=res[-1] if sw._restoring else None)
