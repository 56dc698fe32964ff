"""SeriesStats: statistics of a recorded index series, reduced on the device.

A noise ensemble is looked at through statistics over the series an `IndexRecorder` keeps on the
device ([n_samples][nspec][n]): the ensemble mean and spread over time, quantiles across the
realisations of a parameter set, every member's variance and autocovariance in time, the record
at which a member leaves a state.  `SeriesStats` computes them where the series lives -- one launch
per call (csrc/stats.hip) -- and downloads the results only; the series is never downloaded.

  across_members(k0, k1)   pm_series_group_stats: per (record, index, group of members) the count
                           of finite members, mean, var (ddof = 1), min, max, sum and up to 8
                           quantiles (np.quantile's method="linear")
  along_time(k0, k1)       pm_series_member_stats: per (index, member) the count of finite
                           records, mean, var, min, max, sum, up to 4 lagged autocovariances and,
                           against a threshold, the fraction of records beyond it, the first such
                           record and the number of crossings

Non-finite values (members that blew up) are excluded and counted, never propagated.  Every sum
has one order, stated in include/pymoc_hip.h and independent of the launch geometry, so each
double equals its NumPy restatement (tests/stats_cases.py) bit for bit.  What a source and a record
window [k0, k1) are: series.py.

Out of scope:
  * statistics across ranks: every rank reduces its own members, so a group must lie on one rank.
    A shard then gives bitwise the whole ensemble's result for its groups, because the order inside
    a group is by member index;
  * statistics updated online while the ensemble runs;
  * statistics of `pos` (the positions an IndexRecorder keeps next to the values).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Series, by_name

_DIRS = dict(below=-1, above=1)


def group_order(groups, n):
  """(labels, order, start) of the group labels `groups` [n] (None: one group): `labels` ascending,
  `order` the members sorted by label with a STABLE sort (ascending member index inside a group),
  group g = order[start[g]:start[g + 1]]."""
  if groups is None:
    if n > _lib.PM_STATS_GROUP_MAX:
      raise ValueError("groups=None makes one group of all %d members, more than %d"
                       % (n, _lib.PM_STATS_GROUP_MAX))
    return (np.zeros(1, dtype=np.int64), np.arange(n, dtype=np.int32),
            np.array([0, n], dtype=np.int32))
  g = np.asarray(groups)
  if g.ndim != 1 or g.size != n:
    raise ValueError("groups must be a 1-D array of %d labels, one per member (shape %r here)"
                     % (n, g.shape))
  if g.dtype.kind not in "iu":
    raise ValueError("groups must hold integer labels (dtype %s here)" % g.dtype)
  labels, counts = np.unique(g, return_counts=True)
  if counts.max() > _lib.PM_STATS_GROUP_MAX:
    raise ValueError("group %r has %d members, more than %d"
                     % (labels[counts.argmax()].item(), counts.max(), _lib.PM_STATS_GROUP_MAX))
  order = np.argsort(g, kind="stable").astype(np.int32)
  start = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
  return labels, order, start


class GroupStats(object):
  """What `across_members` returns: count, mean, var, min, max, sum [ngroups, k1 - k0] and
  quantile [nq, ngroups, k1 - k0], each indexed by index name."""

  def __init__(self, names, count, stat, nq):
    # count [K, nspec, ngroups], stat [K, nspec, ngroups, 5 + nq]
    self.names = list(names)
    self.count = by_name(self.names, count.transpose(1, 2, 0))
    for i, key in enumerate(("mean", "var", "min", "max", "sum")):
      setattr(self, key, by_name(self.names, stat[..., i].transpose(1, 2, 0)))
    self.quantile = by_name(self.names, stat[..., 5:5 + nq].transpose(1, 3, 2, 0))


class MemberStats(object):
  """What `along_time` returns: count, mean, var, min, max, sum, frac, first, ncross [n] and
  autocov [nlag, n], each indexed by index name."""

  def __init__(self, names, count, first, ncross, stat, nlag):
    self.names = list(names)
    self.count, self.first = by_name(self.names, count), by_name(self.names, first)
    self.ncross = by_name(self.names, ncross)
    for i, key in enumerate(("mean", "var", "min", "max", "sum", "frac")):
      setattr(self, key, by_name(self.names, stat[..., i]))
    self.autocov = by_name(self.names, stat[..., 6:6 + nlag].transpose(0, 2, 1))


class SeriesStats(Series):
  """`SeriesStats(source, groups=None, quantiles=(), lags=(), thresholds=None)`.

  source      an `IndexRecorder` or `(DeviceArray [nrec, nspec, n], names)` (series.py)
  groups      int array [n] of arbitrary labels (`group_labels`: ascending); None: one group
  quantiles   up to 8 probabilities in [0, 1]
  lags        up to 4 lags >= 1, in records
  thresholds  {name: (value, "below" | "above")}

  Each call of `across_members` / `along_time` is one launch on the source's stream, behind the
  recorder's samples, and the download of the results.  [k0, k1) is a record window (series.py)."""

  def __init__(self, source, groups=None, quantiles=(), lags=(), thresholds=None, stream=None):
    Series.__init__(self, source, stream)
    self.group_labels, order, start = group_order(groups, self.n)
    self.ngroups = start.size - 1
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if q.ndim != 1 or q.size > _lib.PM_STATS_Q_MAX:
      raise ValueError("at most %d quantiles (%d here)" % (_lib.PM_STATS_Q_MAX, q.size))
    if not ((q >= 0.0) & (q <= 1.0)).all():
      raise ValueError("every quantile must lie in [0, 1] (%r here)" % (q.tolist(),))
    lg = np.atleast_1d(np.asarray(lags))
    if lg.size and lg.dtype.kind not in "iu":
      raise ValueError("lags must be integers (dtype %s here)" % lg.dtype)
    if lg.ndim != 1 or lg.size > _lib.PM_STATS_LAG_MAX:
      raise ValueError("at most %d lags (%d here)" % (_lib.PM_STATS_LAG_MAX, lg.size))
    if lg.size and lg.min() < 1:
      raise ValueError("every lag must be at least 1 (%r here)" % (lg.tolist(),))
    thr = np.full(self.nspec, np.nan)
    dirs = np.full(self.nspec, -1, dtype=np.int32)
    for name, spec in (thresholds or {}).items():
      if name not in self.names:
        raise ValueError("threshold %r: unknown index (one of %s)" % (name, ", ".join(self.names)))
      try:
        value, side = spec
      except (TypeError, ValueError):
        raise ValueError("threshold %r: give (value, 'below' | 'above')" % (name,))
      if side not in _DIRS:
        raise ValueError("threshold %r: unknown direction %r (one of below, above)" % (name, side))
      if not np.isfinite(value):
        raise ValueError("threshold %r: the value must be finite (%r here)" % (name, value))
      thr[self.names.index(name)], dirs[self.names.index(name)] = float(value), _DIRS[side]
    # host mirrors (the entries check these) and, from the first launch on, device copies
    self._q, self._lag = q, lg.astype(np.int32)
    self._start, self._order, self._thr, self._dir = start, order, thr, dirs
    self.quantiles, self.lags = q.copy(), self._lag.copy()
    one = np.zeros(1)
    self._host = dict(order=order, start=start, q=q if q.size else one,
                      lag=self._lag if lg.size else one.astype(np.int32), thr=thr, dir=dirs)

  # ------------------------------------------------------------------ device side
  def _launch_group(self, k0, k1, out=None):
    """The launch of `across_members` alone: (count, stat) on the device, nothing synchronised.
    `out`: the pair of an earlier call on the same window, written again."""
    dev, K, nq = self._upload(), k1 - k0, self._q.size
    d = _lib.pm_series_group_stats()
    d.n, d.nspec, d.nrec, d.k0, d.k1, d.ngroups, d.nq = (self.n, self.nspec, K, 0, K,
                                                         self.ngroups, nq)
    # the window as a series of its own: only its results are allocated
    d.v = self._series.ptr + 8 * k0 * self.nspec * self.n
    d.order, d.start, d.start_dev = dev["order"].ptr, self._start.ctypes.data, dev["start"].ptr
    d.q, d.q_dev = self._q.ctypes.data, dev["q"].ptr
    count, stat = out or (DeviceArray((K, self.nspec, self.ngroups), np.int32),
                          DeviceArray((K, self.nspec, self.ngroups, 5 + nq), np.float64))
    with launch_span(self._timer(), "k_series_group_stats", self.stream):
      check(lib.pm_series_group_stats(C.byref(d), count.ptr, stat.ptr, _sh(self.stream)))
    return count, stat

  def across_members(self, k0=0, k1=None):
    k0, k1 = self._record_window(k0, k1)
    count, stat = self._launch_group(k0, k1)
    return GroupStats(self.names, count.download(stream=self.stream),
                      stat.download(stream=self.stream), self._q.size)

  def _launch_member(self, k0, k1, out=None):
    """The launch of `along_time` alone: ([count, first, ncross], stat) on the device; `out` as for
    `_launch_group`."""
    dev, nlag = self._upload(), self._lag.size
    d = _lib.pm_series_member_stats()
    d.n, d.nspec, d.nrec, d.k0, d.k1, d.nlag = self.n, self.nspec, self.nrec, k0, k1, nlag
    d.v = self._series.ptr
    d.lag, d.lag_dev = self._lag.ctypes.data, dev["lag"].ptr
    d.thr, d.thr_dev = self._thr.ctypes.data, dev["thr"].ptr
    d.dir, d.dir_dev = self._dir.ctypes.data, dev["dir"].ptr
    ints, stat = out or ([DeviceArray((self.nspec, self.n), np.int32) for _ in range(3)],
                         DeviceArray((self.nspec, self.n, 6 + nlag), np.float64))
    with launch_span(self._timer(), "k_series_member_stats", self.stream):
      check(lib.pm_series_member_stats(C.byref(d), ints[0].ptr, ints[1].ptr, ints[2].ptr, stat.ptr,
                                       _sh(self.stream)))
    return ints, stat

  def along_time(self, k0=0, k1=None):
    k0, k1 = self._record_window(k0, k1)
    if self._lag.size and self._lag.max() >= k1 - k0:
      raise ValueError("lag %d does not fit a window of %d records" % (self._lag.max(), k1 - k0))
    ints, stat = self._launch_member(k0, k1)
    count, first, ncross = (a.download(stream=self.stream) for a in ints)
    return MemberStats(self.names, count, first, ncross, stat.download(stream=self.stream),
                       self._lag.size)
