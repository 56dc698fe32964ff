"""SeriesEOF: the leading EOF of several recorded indices and its principal component, on the
device.

Every other link of the early-warning chain (SeriesStats, SeriesSpectra, SeriesWindows, the
surrogates, SeriesSmooth, SeriesShifts) reads one index of one member at a time.  The method that
opened the field for the thermohaline circulation does not: Held & Kleinen 2004 ("degenerate
fingerprinting") project the detrended field onto its leading EOF and read critical slowing down
from that principal component -- the critical mode gathers signal from every index while
independent noise averages out.  An `IndexRecorder` holds up to 32 indices per member, and its
`at` specification samples Psi or b at a depth, so the indices can be a coarse profile of the
overturning itself.  `SeriesEOF` computes, for q chosen indices of every member, the scatter
matrix of the record window, its leading eigenvector by a fixed number of power iterations and
the projection of the series onto it, in three launches where the series lives
(pm_series_scatter, pm_series_eof, pm_series_project; csrc/eof.hip).  The principal component is
itself a device series [K, 1, n] named "pc1" that `SeriesWindows`, `SeriesStats`, `SeriesSpectra`,
`SeriesSurrogates` and `SeriesShifts` take as a source unchanged, so this one class gives the
whole chain -- surrogate significance and per-member ends included -- its multivariate form.

  fit(k0, k1)       entries 1 and 2; downloads eof [name] -> [nu], lam, trace, frac = lam / trace,
                    resid, vv, ntot [nu] and nused [n]: an `EOFFit`
  pc(k0, k1)        all three entries, nothing downloaded: (device series [K, 1, n], ["pc1"])
  compute(k0, k1)   `fit` plus the downloaded pc [n, K]

  launch_scatter, launch_eof, launch_project    the launches alone, over any device view

A record is used iff all q indices are finite there; a source censored by
`SeriesShifts.censored()` therefore needs nothing more: every member's EOF is fitted over its own
pre-transition records.  The EOF is normalised to a largest loading of exactly 1 -- which also
fixes its sign -- not to unit length: that would take a square root, and the device calls none, so
that every double equals the NumPy restatement (tests/eof_cases.py) bit for bit.  ac, the DFA
exponent, the restoring rate and Kendall's tau do not see the scale; var scales by the constant
`vv` = |eof|^2, which `fit` returns.  The iteration count is fixed, with no early exit, so that a
result is a pure function of its input; `resid` = max |C v - lam v| / |lam| tells whether it
sufficed.  include/pymoc_hip.h states the definition operation by operation.

scale="std" forms the weights 1 / sqrt(var) on the host from one `SeriesStats.along_time` launch
(var of the finite records of each index on its own, which is not exactly the variance over the
used records where indices are missing at different records).

Out of scope:
  * further modes (EOF 2 and beyond);
  * MAF / min-max autocorrelation factors;
  * sliding-window EOFs: one pattern per record window;
  * unit-norm EOFs (see above);
  * removing the ensemble mean: the source is expected detrended (`SeriesSmooth.residual()`);
  * EOFs of `pos` (the positions an IndexRecorder keeps next to the values);
  * anything across ranks: a pooled group must lie on one rank;
  * anything online: the series is analysed after the samples.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import Series, _Plane, as_int, by_name
from .stats import SeriesStats, group_order

PC_NAME = "pc1"


def _ptr(a):
  return None if a is None else a.ptr


def launch_scatter(x, k0, k1, sel, w, ctx, out=None):
  """pm_series_scatter over the records [k0, k1) of the device view `x` for the indices `sel`
  (ints) with the device weights `w` [q, n] (None: 1.0): (nused [n] int32, mean [q, n], scat
  [q (q + 1) / 2, n]) on the device, nothing synchronised.  `out`: the triple of an earlier call
  of the same q and n, written again."""
  d = _lib.pm_series_scatter()
  (d.nrec, d.nspec, d.n), d.k0, d.k1, d.q = x.shape, k0, k1, len(sel)
  d.v, d.w = x.ptr, _ptr(w)
  for j, s in enumerate(sel):
    d.sel[j] = s
  q, n = len(sel), x.shape[2]
  nused, mean, scat = out or (DeviceArray((n,), np.int32), DeviceArray((q, n), np.float64),
                              DeviceArray((q * (q + 1) // 2, n), np.float64))
  with launch_span(ctx.timer, "k_series_scatter", ctx.stream):
    check(lib.pm_series_scatter(C.byref(d), nused.ptr, mean.ptr, scat.ptr, _sh(ctx.stream)))
  return nused, mean, scat


def launch_eof(nused, scat, q, iters, ctx, order=None, start=None, start_dev=None, out=None):
  """pm_series_eof over the scatters of `launch_scatter`; units: every member (order None) or the
  groups (order: device [n], start: host int32 [nu + 1], start_dev its device copy).  (eof [q, nu],
  [lam, trace, resid, vv] each [nu], ntot [nu] int32) on the device, nothing synchronised.  `out`:
  the triple of an earlier call, written again."""
  n = nused.shape[0]
  nu = n if order is None else start.size - 1
  d = _lib.pm_series_eof()
  d.n, d.q, d.nu, d.iters = n, q, nu, iters
  d.nused, d.scat, d.order, d.start_dev = nused.ptr, scat.ptr, _ptr(order), _ptr(start_dev)
  d.start = None if start is None else start.ctypes.data
  eof, vals, ntot = out or (DeviceArray((q, nu), np.float64),
                            [DeviceArray((nu,), np.float64) for _ in range(4)],
                            DeviceArray((nu,), np.int32))
  with launch_span(ctx.timer, "k_series_eof", ctx.stream):
    check(lib.pm_series_eof(C.byref(d), eof.ptr, *([a.ptr for a in vals]
                                                   + [ntot.ptr, _sh(ctx.stream)])))
  return eof, vals, ntot


def launch_project(x, k0, k1, sel, w, nused, mean, eof, ctx, unit=None, pc=None):
  """pm_series_project over the records [k0, k1) of the device view `x`: the device series pc
  [K, 1, n], nothing synchronised.  `unit`: device int32 [n] (None: every member its own); `pc`:
  the array of an earlier call, written again."""
  d = _lib.pm_series_project()
  (d.nrec, d.nspec, d.n), d.k0, d.k1, d.q, d.nu = x.shape, k0, k1, len(sel), eof.shape[1]
  d.v, d.w, d.nused, d.mean = x.ptr, _ptr(w), nused.ptr, mean.ptr
  d.eof, d.unit = eof.ptr, _ptr(unit)
  for j, s in enumerate(sel):
    d.sel[j] = s
  if pc is None:
    pc = DeviceArray((k1 - k0, 1, x.shape[2]), np.float64)
  with launch_span(ctx.timer, "k_series_project", ctx.stream):
    check(lib.pm_series_project(C.byref(d), pc.ptr, _sh(ctx.stream)))
  return pc


def std_weights(var, order=None, start=None):
  """The weights of scale="std" from var [q, n]: 1 / sqrt(var), 0 where var is zero or not finite;
  with (order, start) the var of a unit is the mean of its members' finite variances, and its
  members share one weight per index."""
  var = np.array(var, dtype=np.float64)
  if order is not None:
    for u in range(start.size - 1):
      mem = order[start[u]:start[u + 1]]
      for j in range(var.shape[0]):
        fin = var[j, mem][np.isfinite(var[j, mem])]
        var[j, mem] = fin.mean() if fin.size else np.nan
  w = np.zeros_like(var)
  ok = np.isfinite(var) & (var > 0.0)
  w[ok] = 1.0 / np.sqrt(var[ok])
  return np.where(np.isfinite(w), w, 0.0)


class EOFFit(object):
  """What `fit` returns: eof `[name] -> [nu]` (the loadings, the largest exactly 1), lam, trace,
  frac = lam / trace, resid, vv and ntot `[nu]`, nused `[n]`, `unit` [n] (the unit of a member)
  and `labels` [nu] (the group labels, or the member numbers); `compute` adds pc [n, K]."""

  def __init__(self, names, labels, unit, eof, vals, ntot, nused, pc=None):
    self.names, self.labels, self.unit = list(names), labels, unit
    self.eof = by_name(self.names, eof)
    self.lam, self.trace, self.resid, self.vv = vals
    with np.errstate(all="ignore"):
      self.frac = self.lam / self.trace
    self.ntot, self.nused = ntot, nused
    if pc is not None:
      self.pc = pc


class SeriesEOF(Series):
  """`SeriesEOF(source, indices=None, scale="none", groups=None, pooled=False, iters=64,
  stream=None)`.

  source    an `IndexRecorder` or `(device series [nrec, nspec, n], names)` (series.py)
  indices   the names of 1 to 32 distinct indices (None: all of the source's)
  scale     "none"; "std" (weights 1 / sqrt(var) of the record window, see the module); or finite
            weights [q] or [q, n]
  groups    int labels [n]; with pooled=True one EOF per group from the pooled scatter -- the
            realisations of one parameter set share the pattern; otherwise one EOF per member
  iters     the number of power iterations, 1 .. 1024

  Every refusal is a ValueError here, before any device array exists."""

  def __init__(self, source, indices=None, scale="none", groups=None, pooled=False, iters=64,
               stream=None):
    Series.__init__(self, source, stream)
    names = list(self.names) if indices is None else (
        [indices] if isinstance(indices, str) else list(indices))
    if not 1 <= len(names) <= _lib.PM_EOF_Q_MAX:
      raise ValueError("an EOF takes 1 to %d indices (%d here)" % (_lib.PM_EOF_Q_MAX, len(names)))
    for nm in names:
      if nm not in self.names:
        raise ValueError("unknown index %r (one of %s)" % (nm, ", ".join(map(str, self.names))))
    if len(set(names)) != len(names):
      raise ValueError("the indices must be distinct (%r here)" % (names,))
    self.indices, self._sel = names, [self.names.index(nm) for nm in names]
    self.q = len(names)
    self.iters = as_int("iters", iters)
    if not 1 <= self.iters <= _lib.PM_EOF_ITERS_MAX:
      raise ValueError("iters must lie in [1, %d] (%d here)" % (_lib.PM_EOF_ITERS_MAX, self.iters))
    if not isinstance(pooled, (bool, np.bool_)):
      raise ValueError("pooled must be True or False (%r here)" % (pooled,))
    self.pooled = bool(pooled)
    if self.pooled and groups is None:
      raise ValueError("pooled=True needs groups: the members that share an EOF")
    if groups is not None and not self.pooled:
      raise ValueError("groups are read by pooled=True only; without it every member has its "
                       "own EOF")
    self._order = self._start = None
    self.labels, self.unit = np.arange(self.n), np.arange(self.n, dtype=np.int32)
    if self.pooled:
      self.labels, self._order, self._start = group_order(groups, self.n)
      self.unit = np.empty(self.n, dtype=np.int32)
      for u in range(self._start.size - 1):
        self.unit[self._order[self._start[u]:self._start[u + 1]]] = u
      self._host = dict(order=self._order, start=self._start, unit=self.unit)
    self.nu = self.labels.size
    self._w_host, self._w_dev, self._stats = None, None, None
    if isinstance(scale, str):
      if scale not in ("none", "std"):
        raise ValueError("scale must be 'none', 'std' or an array of weights (%r here)" % (scale,))
      if scale == "std":
        self._stats = SeriesStats(source, stream=stream)
    else:
      try:
        w = np.asarray(scale, dtype=np.float64)
      except (TypeError, ValueError):
        raise ValueError("scale must be 'none', 'std' or an array of weights (%r here)" % (scale,))
      if w.shape not in ((self.q,), (self.q, self.n)):
        raise ValueError("the weights must have the shape (%d,) or (%d, %d) (%r here)"
                         % (self.q, self.q, self.n, w.shape))
      if not np.isfinite(w).all():
        raise ValueError("every weight must be finite")
      self._w_host = np.ascontiguousarray(np.broadcast_to(w.reshape(self.q, -1), (self.q, self.n)))
    self.scale = scale if isinstance(scale, str) else "weights"

  # ------------------------------------------------------------------ device side
  def _weights(self, k0, k1):
    """The device weights [q, n] of the record window, or None."""
    if self._stats is not None:
      _, stat = self._stats._launch_member(k0, k1)
      var = stat.download(stream=self.stream)[self._sel, :, 1]
      return DeviceArray.from_host(std_weights(var, self._order, self._start), dtype=np.float64,
                                   stream=self.stream)
    if self._w_host is not None and self._w_dev is None:
      self._w_dev = DeviceArray.from_host(self._w_host, dtype=np.float64, stream=self.stream)
    return self._w_dev

  def _fit(self, k0, k1):
    """Entries 1 and 2 on the device: (w, nused, mean, eof, vals, ntot)."""
    k0, k1 = self._record_window(k0, k1)
    if k1 - k0 < 2:
      raise ValueError("window [%d, %d) holds fewer than 2 records" % (k0, k1))
    ctx, w = self._ctx(), self._weights(k0, k1)
    nused, mean, scat = launch_scatter(self._series, k0, k1, self._sel, w, ctx)
    dev = self._upload() if self.pooled else {}
    eof, vals, ntot = launch_eof(nused, scat, self.q, self.iters, ctx, dev.get("order"),
                                 self._start, dev.get("start"))
    return (k0, k1), (w, nused, mean, eof, vals, ntot)

  def _project(self, win, fitted):
    w, nused, mean, eof = fitted[:4]
    dev = self._upload() if self.pooled else {}
    pc = launch_project(self._series, win[0], win[1], self._sel, w, nused, mean, eof, self._ctx(),
                        dev.get("unit"))
    return _Plane(pc, 0, pc.shape, keep=(self._series, w, nused, mean, eof, dev.get("unit")))

  def _download(self, fitted, pc=None):
    _, nused, _, eof, vals, ntot = fitted
    get = lambda a: a.download(stream=self.stream)
    return EOFFit(self.indices, self.labels, self.unit, get(eof), [get(a) for a in vals],
                  get(ntot), get(nused), pc)

  def fit(self, k0=0, k1=None):
    """Two launches (three with scale="std"), then the download of the fit alone: an `EOFFit`."""
    _, fitted = self._fit(k0, k1)
    return self._download(fitted)

  def pc(self, k0=0, k1=None):
    """The principal component of the record window: (device series [K, 1, n], ["pc1"]), a source
    of its own (pass `stream=` this object's stream with it); three launches, nothing downloaded.
    The series keeps what it was computed from alive."""
    win, fitted = self._fit(k0, k1)
    return self._project(win, fitted), [PC_NAME]

  def compute(self, k0=0, k1=None):
    """`fit` and the downloaded pc [n, K]: an `EOFFit` with `pc`."""
    win, fitted = self._fit(k0, k1)
    plane = self._project(win, fitted)
    pc = plane._parent.download(stream=self.stream)[:, 0, :].T
    return self._download(fitted, np.ascontiguousarray(pc))
