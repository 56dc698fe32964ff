"""SeriesShifts: where a recorded index series shifts abruptly, per member, and the series cut at
that record -- on the device.

In a ramped, noise-driven sweep every member's AMOC collapses in a year of its own, and some never
do.  The early-warning chain (SeriesSmooth, SeriesWindows, Kendall, the surrogate test) takes one
record window for all members, and the published method (Dakos et al. 2008, Boers 2021) computes
the indicators on the part BEFORE the transition only: a window, a smoother kernel or a Kendall pair
that straddles the shift puts the jump into the variance and the autocorrelation, and the
"warning" it reports is the collapse itself.  `SeriesShifts` finds the record of the largest shift
and the record from which a shift is detectable, per (index, member), and hands every `Series*`
class a copy of the series with NaN from the member's own end on -- which each of them already
excludes and counts by its stated rule (for the smoother: an edge renormalised at the transition).

  detect(k0, k1)            one launch of pm_series_windows (windows of L records, step 1, their
                            means and variances) and one of pm_series_shift_scan (csrc/shifts.hip):
                            a `Shifts` with at, first, ncand, record `[name] -> [n]` (int32) and
                            stat, jump, before, after `[name] -> [n]`; the device arrays stay on
                            this object
  censored(where, guard, by)
                            (DeviceArray [K, nspec, n], names): the record window with NaN from
                            end = max(0, where - guard) on (pm_series_censor), a source of its
                            own; `.end` on the device, `end()` downloaded
  SeriesWindows.significance(..., until=this)
                            the surrogate test up to every member's own end: the observed series
                            censored, the null model fitted per member over [k0, k0 + end)
                            (pm_series_fit_ranged), every surrogate censored like the record

The statistic compares two adjacent windows of L = `half` records: for a candidate record c,
jump = mean[c, c + L) - mean[c - L, c) and stat = jump / sqrt of the mean of the two windows'
variances -- the jump in pooled standard deviations.  `at` is the candidate with the largest score
(-stat for drops, +stat for rises, |stat| for either), the first among equals; `first` the first
candidate whose score reaches `threshold`.  Both are numbered from k0; `record` is k0 + at.  -1:
no candidate counts (a window with a non-finite record has no mean), or none reaches the
threshold.  include/pymoc_hip.h states the definitions; tests/shifts_cases.py restates them.

Out of scope: change-point models beyond the two-window statistic; more than one shift per
series; anything across ranks, online, or on `pos`.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Ctx, View, _Plane, as_int, by_name, records
from .windows import _DETREND, _Source, launch_windows, stt_of, win_par

WHERE = ("first", "at")
VALUES = ("stat", "jump", "before", "after")


def _per_name(what, val, names, default, conv):
  """[nspec] values of a scalar or a {name: value} argument (a name left out takes `default`)."""
  if isinstance(val, dict):
    unknown = [nm for nm in val if nm not in names]
    if unknown:
      raise ValueError("%s names unknown indices %r (one of %s)"
                       % (what, unknown, ", ".join(map(str, names))))
    return [conv(what, val.get(nm, default)) for nm in names]
  return [conv(what, val)] * len(names)


def _as_direction(what, val):
  val = as_int(what, val)
  if val not in (-1, 0, 1):
    raise ValueError("%s must be -1 (drops), 0 (either) or +1 (rises) (%d here)" % (what, val))
  return val


def _as_threshold(what, val):
  if val is None:
    return float("nan")
  if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)):
    raise ValueError("%s must be a number or None (%r here)" % (what, val))
  val = float(val)
  if np.isinf(val):
    raise ValueError("%s must not be infinite" % what)
  return val


def stt_table(K, stream=None):
  """(host, device) table stt_tab[0 .. K] of pm_series_fit_ranged: `stt_of(W)` of every W."""
  tab = np.array([stt_of(W) for W in range(K + 1)], dtype=np.float64)
  return tab, DeviceArray.from_host(tab, dtype=np.float64, stream=stream)


def launch_fit_ranged(arr, shape, k0, k1, detrend, end, stream, timer, table=None, out=None):
  """pm_series_fit_ranged over the records [k0, k1) of a device series of `shape` = (nrec, nspec,
  n): (var, ac), each a device series [1, nspec, n] as `SeriesSurrogates.fit` gives them, fitted
  per member over [k0, k0 + end[s][m]); nothing synchronised.  `table`: a `stt_table(k1 - k0)`
  made earlier; `out`: the fit of an earlier call, written again."""
  nrec, nspec, n = shape
  tab, tab_dev = table or stt_table(k1 - k0, stream)
  if out is None:
    parent = DeviceArray((2, 1, nspec, n), np.float64)
    out = _Plane(parent, 0, (1, nspec, n)), _Plane(parent, 1, (1, nspec, n))
  d = _lib.pm_series_fit_ranged()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.detrend = n, nspec, nrec, k0, k1, _DETREND[detrend]
  d.v, d.end, d.stt_tab, d.stt_tab_dev = arr.ptr, end.ptr, tab.ctypes.data, tab_dev.ptr
  with launch_span(timer, "k_series_fit_ranged", stream):
    check(lib.pm_series_fit_ranged(C.byref(d), out[0].ptr, out[1].ptr, _sh(stream)))
  out[0].keep = (arr, end, tab_dev)  # (they live as long as the fit read from them)
  return out


Censor = collections.namedtuple("Censor", "where guard src src_dev")


def launch_censor(x, y, cens, ctx, end_out=None):
  """pm_series_censor with the `Censor` cens (where [nspec, n] on the device, guard, src [nspec] on
  the host and on the device) from the device view `x` [K, nb * nspec, n] into `y` (x itself: in
  place); the ends into `end_out` when given; nothing synchronised."""
  d = _lib.pm_series_censor()
  d.K, d.nspec, d.n, d.guard = x.shape[0], len(cens.src), x.shape[2], cens.guard
  d.nb = x.shape[1] // d.nspec
  d.x, d.where, d.src, d.src_dev = x.ptr, cens.where.ptr, cens.src.ctypes.data, cens.src_dev.ptr
  with launch_span(ctx.timer, "k_series_censor", ctx.stream):
    check(lib.pm_series_censor(C.byref(d), y.ptr, None if end_out is None else end_out.ptr,
                               _sh(ctx.stream)))


def launch_shift_scan(mean, var, nrec, k0, k1, half, thr, dirs, ctx, out=None):
  """pm_series_shift_scan on the mean and the var plane of windows of `half` records, step 1, over
  the records [k0, k1) of a series of nrec; thr and dirs: (host, device) [nspec].  (at, first,
  ncand [nspec, n] int32, val [4, nspec, n]) on the device, nothing synchronised."""
  nspec, n = mean.shape[1:]
  d = _lib.pm_series_shift_scan()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.half = n, nspec, nrec, k0, k1, half
  d.mean, d.var = mean.ptr, var.ptr
  d.thr, d.thr_dev, d.dir, d.dir_dev = (thr[0].ctypes.data, thr[1].ptr, dirs[0].ctypes.data,
                                        dirs[1].ptr)
  if out is None:
    out = [DeviceArray((nspec, n), np.int32) for _ in range(3)]
    out.append(DeviceArray((4, nspec, n), np.float64))
  with launch_span(ctx.timer, "k_series_shift_scan", ctx.stream):
    check(lib.pm_series_shift_scan(C.byref(d), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                   _sh(ctx.stream)))
  return out


class _Ends(DeviceArray):
  """`SeriesShifts.end`: the ends on the device (int32 [nspec, n]); called, `end()`, it downloads
  them as `[name] -> [n]`."""

  def __call__(self):
    return by_name(self._names, self.download(stream=self._stream))


class Shifts(object):
  """What `detect` returns, each `[name] -> [n]`: at, first, ncand (int32; records numbered from
  k0, -1: none), record (the absolute k0 + at, -1 where at is), and stat, jump, before, after at
  `at` (NaN where at is -1)."""

  def __init__(self, names, k0, at, first, ncand, val):
    self.names, self.k0 = list(names), k0
    self.at, self.first, self.ncand = (by_name(self.names, a) for a in (at, first, ncand))
    self.record = by_name(self.names, np.where(at < 0, -1, k0 + at).astype(np.int32))
    for i, key in enumerate(VALUES):
      setattr(self, key, by_name(self.names, val[i]))


class SeriesShifts(_Source):
  """`SeriesShifts(source, half, direction=-1, threshold=None, stream=None)`.

  source     an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  half       L, the records of each of the two windows compared, in [4, 2048]; 2 L <= K
  direction  -1: drops, +1: rises, 0: either; one value or {name: value} (a name left out: -1)
  threshold  the score from which a shift is detectable (`first`), in pooled standard deviations;
             None: no threshold (`first` is -1); one value or {name: value}

  `detect` first; `censored` and `SeriesWindows.significance(until=)` use what it left on the
  device."""

  def __init__(self, source, half, direction=-1, threshold=None, stream=None):
    _Source.__init__(self, source, stream)
    L = as_int("half", half)
    if not _lib.PM_WIN_MIN <= L <= _lib.PM_SHIFT_HALF_MAX:
      raise ValueError("half must lie in [%d, %d] (%d here)"
                       % (_lib.PM_WIN_MIN, _lib.PM_SHIFT_HALF_MAX, L))
    self.half = L
    self.direction = np.array(_per_name("direction", direction, self.names, -1, _as_direction),
                              dtype=np.int32)
    self.threshold = np.array(_per_name("threshold", threshold, self.names, None, _as_threshold),
                              dtype=np.float64)
    self._host = dict(thr=self.threshold, dir=self.direction)
    self._found = self._cens = self.end = None

  def _window(self, k0, k1):
    k0, k1 = self._record_window(k0, k1)
    K = k1 - k0
    if K < 2 * self.half:
      raise ValueError("window [%d, %d) holds %d records, fewer than 2 * half = %d"
                       % (k0, k1, K, 2 * self.half))
    nwin = K - self.half + 1
    if nwin * self.nspec >= 1 << 30:
      raise ValueError("nwin * nspec = %d is not below 2^30" % (nwin * self.nspec))
    return k0, k1, nwin

  def _scan(self, k0, k1, mean, var, out=None):
    """pm_series_shift_scan on the two planes: (at, first, ncand [nspec, n] int32, val [4, nspec,
    n]) on the device, nothing synchronised."""
    dev = self._upload()
    return launch_shift_scan(mean, var, self.nrec, k0, k1, self.half,
                             (self.threshold, dev["thr"]), (self.direction, dev["dir"]),
                             self._ctx(), out=out)

  def detect(self, k0=0, k1=None, max_bytes=2 << 30):
    """The shifts of the record window [k0, k1): one launch of pm_series_windows (window = half,
    step 1, "constant", lag 1) into a scratch [4, nwin, nspec, n] of 32 nwin nspec n bytes, which
    must not exceed `max_bytes`, then the scan; a `Shifts`."""
    max_bytes = as_int("max_bytes", max_bytes)
    k0, k1, nwin = self._window(k0, k1)
    need = 32 * nwin * self.nspec * self.n
    if need > max_bytes:
      raise ValueError("the window scratch of %d bytes (32 nwin nspec n, nwin = %d) exceeds "
                       "max_bytes = %d" % (need, nwin, max_bytes))
    out, _ = launch_windows(self._series, k0, k1, win_par(self.half, 1, 1, "constant"),
                            self._ctx())
    shape = (nwin, self.nspec, self.n)
    found = self._scan(k0, k1, _Plane(out, 0, shape), _Plane(out, 2, shape))
    self.at_dev, self.first_dev, self.ncand_dev, self.val_dev = found
    self._found, self._cens, self.end = (k0, k1), None, None
    return Shifts(self.names, k0, *(a.download(stream=self.stream) for a in found))

  def _censor(self, x_ptr, K, nb, y_ptr, stream, timer, end_out=None):
    """pm_series_censor with the arguments of the last `censored` call on nb * nspec planes, on
    the caller's stream, its span where the caller's spans go."""
    shape = (K, nb * self.nspec, self.n)
    launch_censor(View(x_ptr, shape), View(y_ptr, shape), self._cens, Ctx(stream, timer), end_out)

  def censored(self, where="first", guard=0, by=None):
    """The record window of the last `detect` with NaN from every member's end on: (DeviceArray
    [K, nspec, n], names), a source every `Series*` class takes (its records are numbered from
    k0; pass `stream=` this object's stream with it).

    where   "first" (the first record the shift is detectable from) or "at" (its largest score)
    guard   records kept clear before it: end = max(0, where - guard); where = -1: end = K
    by      a name: that index's shift governs every index of the member (censor all indices at
            the AMOC's transition); None: every index by its own

    `.end` holds the ends on the device (int32 [nspec, n]) and `end()` downloads them `[name] ->
    [n]`; one launch, nothing synchronised."""
    if self._found is None:
      raise ValueError("censored() needs detect() first")
    if where not in WHERE:
      raise ValueError("unknown where %r (one of %s)" % (where, ", ".join(WHERE)))
    guard = as_int("guard", guard)
    if guard < 0:
      raise ValueError("guard must not be negative (%d here)" % guard)
    if by is not None and by not in self.names:
      raise ValueError("by names an unknown index %r (one of %s)"
                       % (by, ", ".join(map(str, self.names))))
    src = np.arange(self.nspec, dtype=np.int32)
    if by is not None:
      src[:] = self.names.index(by)
    k0, k1 = self._found
    K = k1 - k0
    if self.nspec * K >= 1 << 31 or self.nspec * self.n >= 1 << 31:
      raise ValueError("K * nspec = %d or nspec * n = %d is not below 2^31"
                       % (self.nspec * K, self.nspec * self.n))
    self._cens = Censor(self.first_dev if where == "first" else self.at_dev, guard, src,
                        DeviceArray.from_host(src, dtype=np.int32, stream=self.stream))
    y = DeviceArray((K, self.nspec, self.n), np.float64)
    self.end = _Ends((self.nspec, self.n), np.int32)
    self.end._names, self.end._stream = self.names, self.stream
    launch_censor(records(self._series, k0, k1), y, self._cens, self._ctx(), self.end)
    return y, list(self.names)

  def _until(self, sw, k0, k1):
    """Checked as the `until` of `sw.significance(k0, k1)`."""
    if self._found is None or self._cens is None:
      raise ValueError("until needs detect() and censored() called on it first")
    if (self.nspec, self.n) != (sw.nspec, sw.n) or self.names != sw.names:
      raise ValueError("until was made for another series (%d indices x %d members, here %d x %d)"
                       % (self.nspec, self.n, sw.nspec, sw.n))
    if self._found != (k0, k1):
      raise ValueError("until detected over the record window [%d, %d), not [%d, %d)"
                       % (self._found + (k0, k1)))
