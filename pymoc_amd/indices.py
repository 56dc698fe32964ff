"""RowIndices and IndexRecorder: per-member overturning indices, evaluated on the device.

A sweep is not looked at as profiles but as a handful of scalars per member over time: the
strength of the AMOC cell, the depth of its maximum, the depth where the streamfunction changes
sign, the buoyancy at a fixed depth, the abyssal cell's minimum.  `RowIndices` evaluates up to 32
such indices for every member in ONE launch (pm_row_indices, csrc/indices.hip); `IndexRecorder`
attaches to a coupled ensemble and takes that launch where the driver tests for a diagnostic
gather -- right after the overturning update -- straight into record k of a device-resident series,
so a sample costs one launch, no packing launch, no copy, no synchronisation.

An index is `(name, kind, source_name, params)`:
  kind "max" / "min"   the extremum of the window and the level it sits at (np.argmax / np.argmin:
                       first occurrence, a NaN wins)
  kind "at"            np.interp(x0, axis, row) over the whole row:            params x0=
  kind "cross"         the axis position where the row crosses `level` (default 0), the crossing
                       nearest the top of the window:                           params level=
  kind "mean"          the trapezoid mean over the window
  params zlo=, zhi=    the window: the levels with zlo <= axis <= zhi (default: the whole axis),
                       resolved on the host
include/pymoc_hip.h states the definitions in full.  All are bit-identical to their NumPy
restatement except "mean", whose summation order is the kernel's own (a tolerance index).

Out of scope: gathering indices across ranks (every rank records its own members), and recording
inside `run_to_steady`, which builds its own ensembles.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span

KINDS = dict(max=_lib.PM_IDX_MAX, min=_lib.PM_IDX_MIN, at=_lib.PM_IDX_AT,
             cross=_lib.PM_IDX_CROSS, mean=_lib.PM_IDX_MEAN)
_NEEDS_INCREASING = ("at", "cross", "mean")
_PARAMS = dict(max=("zlo", "zhi"), min=("zlo", "zhi"), mean=("zlo", "zhi"),
               cross=("zlo", "zhi", "level"), at=("x0",))


def window(axis, zlo=None, zhi=None):
  """(lo, hi): the levels with zlo <= axis <= zhi, inclusive; None = unbounded on that side.
  ValueError when no level qualifies or when those that do are not one run of levels."""
  axis = np.asarray(axis, dtype=np.float64)
  ok = np.ones(axis.size, dtype=bool)
  if zlo is not None:
    ok &= axis >= float(zlo)
  if zhi is not None:
    ok &= axis <= float(zhi)
  idx = np.nonzero(ok)[0]
  if idx.size == 0:
    raise ValueError("empty window: no level of the axis lies in [%r, %r]" % (zlo, zhi))
  if idx[-1] - idx[0] + 1 != idx.size:
    raise ValueError("the levels in [%r, %r] are not one run of levels" % (zlo, zhi))
  return int(idx[0]), int(idx[-1])


def resolve(specs, axes):
  """The host half of a table: `specs` against `axes` {source_name: axis}.  Returns
  [(name, kind, source_name, lo, hi, param)] with the windows resolved; ValueError for an empty
  window, an axis that is not strictly increasing under "at" / "cross" / "mean", an unknown kind,
  source or parameter, a duplicate name, a missing x0, no spec or more than 32 of them."""
  specs = list(specs)
  if not 1 <= len(specs) <= _lib.PM_INDICES_MAX:
    raise ValueError("a table holds 1 to %d index specifications (%d here)"
                     % (_lib.PM_INDICES_MAX, len(specs)))
  out, seen = [], set()
  for name, kind, source, params in specs:
    params = dict(params or {})
    if name in seen:
      raise ValueError("duplicate index name %r" % (name,))
    seen.add(name)
    if kind not in KINDS:
      raise ValueError("index %r: unknown kind %r (one of %s)" % (name, kind, ", ".join(KINDS)))
    if source not in axes:
      raise ValueError("index %r: unknown source %r (one of %s)"
                       % (name, source, ", ".join(sorted(axes))))
    extra = set(params) - set(_PARAMS[kind])
    if extra:
      raise ValueError("index %r: kind %r takes %s, not %s"
                       % (name, kind, ", ".join(_PARAMS[kind]), ", ".join(sorted(extra))))
    axis = np.asarray(axes[source], dtype=np.float64)
    if axis.ndim != 1 or axis.size < 1:
      raise ValueError("source %r: the axis must be a 1-D array of at least one level" % (source,))
    if kind in _NEEDS_INCREASING and not (np.diff(axis) > 0).all():
      raise ValueError("index %r: kind %r needs a strictly increasing axis" % (name, kind))
    if kind == "at":
      if "x0" not in params:
        raise ValueError("index %r: kind 'at' needs x0=" % (name,))
      lo, hi, param = 0, axis.size - 1, float(params["x0"])
    else:
      lo, hi = window(axis, params.get("zlo"), params.get("zhi"))
      param = float(params.get("level", 0.0)) if kind == "cross" else 0.0
    out.append((name, kind, source, lo, hi, param))
  return out


def _source(src, n):
  """(DeviceArray, axis, row stride in doubles) of a `sources` entry: (array, axis) or
  (array, axis, stride); the stride defaults to the array's row length."""
  if len(src) == 2:
    arr, axis = src
    stride = arr.shape[-1] if len(arr.shape) > 1 else np.asarray(axis).size
  else:
    arr, axis, stride = src
  axis = np.ascontiguousarray(axis, dtype=np.float64)
  stride = int(stride)
  if arr.dtype != np.float64:
    raise ValueError("an index source must be a float64 array")
  if stride < axis.size or ((n - 1) * stride + axis.size) * 8 > arr.nbytes:
    raise ValueError("an index source of %d bytes does not hold %d rows of %d levels, %d doubles "
                     "apart" % (arr.nbytes, n, axis.size, stride))
  return arr, axis, stride


class RowIndices(object):
  """`RowIndices(n, specs, sources)`: the table of `specs` (the module docstring's tuples) over
  `sources` {source_name: (DeviceArray or row view, axis as a host array[, row stride])} for n
  members, checked on the host (`resolve`) and uploaded once.

  `sample()` launches and returns host arrays (values [nspec, n] float64, pos [nspec, n] int32;
  pos is -1 where the kind has none).  `sample(out=(value address, pos address))` launches into
  the caller's device memory ([nspec][n] each) and returns nothing: no copy, no synchronisation.
  `depth(name)`: axis[pos] of the last host sample, NaN where pos is -1."""

  def __init__(self, n, specs, sources, stream=None):
    self.n, self.stream = int(n), stream
    if self.n < 1:
      raise ValueError("n must be at least 1")
    srcs = {k: _source(v, self.n) for k, v in sources.items()}
    self.table = resolve(specs, {k: v[1] for k, v in srcs.items()})
    self.names = [t[0] for t in self.table]
    self.nspec = len(self.table)
    self.axes = {}      # source_name -> host axis
    self._keep = []     # what the device table points to
    axis_dev = {}
    self._host = (_lib.pm_index_spec * self.nspec)()
    for e, (name, kind, source, lo, hi, param) in zip(self._host, self.table):
      arr, axis, stride = srcs[source]
      if source not in axis_dev:
        axis_dev[source] = DeviceArray.from_host(axis, stream=stream)
        self.axes[source] = axis
        self._keep.append((arr, axis_dev[source]))
      e.src, e.axis, e.stride, e.nlev = arr.ptr, axis_dev[source].ptr, stride, axis.size
      e.kind, e.lo, e.hi, e.param = KINDS[kind], lo, hi, param
    nbytes = C.sizeof(self._host)
    self._dev = DeviceArray((nbytes // 8,), np.float64)
    check(lib.pm_memcpy_h2d(self._dev.ptr, C.addressof(self._host), nbytes, _sh(stream)))
    d = self.desc = _lib.pm_row_indices()
    d.n, d.nspec, d.spec, d.spec_dev = self.n, self.nspec, C.addressof(self._host), self._dev.ptr
    self._value = self._pos = None
    self.values = self.pos = None

  def index(self, name):
    return self.names.index(name)

  def launch(self, value_ptr, pos_ptr, stream=None):
    check(lib.pm_row_indices(C.byref(self.desc), value_ptr, pos_ptr,
                             _sh(self.stream if stream is None else stream)))

  def sample(self, out=None):
    if out is not None:
      self.launch(int(out[0]), int(out[1]))
      return None
    if self._value is None:
      self._value = DeviceArray((self.nspec, self.n), np.float64)
      self._pos = DeviceArray((self.nspec, self.n), np.int32)
    self.launch(self._value.ptr, self._pos.ptr)
    self.values = self._value.download(stream=self.stream)
    self.pos = self._pos.download(stream=self.stream)
    return self.values, self.pos

  def axis_of(self, name):
    return self.axes[self.table[self.index(name)][2]]

  def depth_of(self, name, pos):
    """axis[pos] for positions of index `name` (any shape), NaN where pos is -1."""
    axis, pos = self.axis_of(name), np.asarray(pos)
    return np.where(pos >= 0, axis[np.clip(pos, 0, axis.size - 1)], np.nan)

  def depth(self, name):
    if self.pos is None:
      raise ValueError("depth() follows a sample()")
    return self.depth_of(name, self.pos[self.index(name)])


class _ByName(object):
  """`recorder.values[name]` / `recorder.pos[name]`: [n, n_samples] of one index."""

  def __init__(self, rec, which):
    self._rec, self._which = rec, which

  def __getitem__(self, name):
    return self._rec._series()[self._which][:, self._rec.table.index(name), :].T

  def keys(self):
    return list(self._rec.table.names)


class IndexRecorder(object):
  """`IndexRecorder(ens, specs, every, n_samples)` attaches itself to a coupled ensemble
  (`ens.indices`): TwoColEnsemble, JN2018Ensemble, JN2018ImplicitEnsemble, TwoBasinEnsemble,
  TwoBasinSweep.  The sources default to `ens.fields()` on the driver's z axis; `sources=` adds
  further device rows by name, each a DeviceArray on z or a `RowIndices` source tuple (for example
  `dict(Psi_iso_b=ens.tw.psibz1)`).

  Sample k = step // every is taken when step % every == 0, at the driver's diagnostic-gather
  site: right after the overturning update at `step`, the instant JN2018Diagnostics samples at.
  `every` must be a multiple of MOC_up_iters; samples with k >= n_samples are dropped.  A sample
  is one launch into record k of the device series [n_samples][nspec][n] (values) and its int32
  twin (positions); nothing leaves the device until the series is read:
    values[name], pos[name]   [n, n_samples]; records never written read 0 and -1
    depth(name)               axis[pos], NaN where pos is -1
    steps                     [n_samples] the step of every record, -1 where never written
  downloaded once on first access after the last sample.  Not with `fused_run=True` (ValueError:
  a persistent launch spans the steps the samples are taken at), and JN2018Ensemble's captured
  graph is replayed only while no recorder is attached."""

  def __init__(self, ens, specs, every, n_samples, sources=None):
    every, n_samples = int(every), int(n_samples)
    if every < 1 or every % ens.M != 0:
      raise ValueError("every must be a positive multiple of MOC_up_iters (%d)" % ens.M)
    if n_samples < 1:
      raise ValueError("n_samples must be at least 1")
    if getattr(ens, "_fused_run", False):
      raise ValueError("an IndexRecorder does not go with fused_run=True: a persistent launch "
                       "spans the steps the samples are taken at")
    z = ens.cols.z_host
    srcs = {k: (a, z) for k, a in ens.fields().items() if a is not None}
    for k, a in (sources or {}).items():
      srcs[k] = a if isinstance(a, tuple) else (a, z)
    self.ens, self.every, self.n_samples = ens, every, n_samples
    self.table = RowIndices(ens.n, specs, srcs, stream=ens.stream)
    rec = self.table.nspec * ens.n
    self._rec = rec
    self._values = DeviceArray.zeros((n_samples, self.table.nspec, ens.n), stream=ens.stream)
    self._pos = DeviceArray((n_samples, self.table.nspec, ens.n), np.int32)
    check(lib.pm_memset(self._pos.ptr, 0xff, self._pos.nbytes, _sh(ens.stream)))  # every pos -1
    check(lib.pm_stream_sync(_sh(ens.stream)))
    self._steps = np.full(n_samples, -1, dtype=np.int64)
    self._host = None
    self.values, self.pos = _ByName(self, 0), _ByName(self, 1)
    ens.indices = self

  def maybe_sample(self, step):
    if step % self.every != 0:
      return
    k = step // self.every
    if not 0 <= k < self.n_samples:
      return
    e = self.ens
    with launch_span(e.timer, "k_row_indices", e.stream):
      self.table.sample(out=(self._values.ptr + 8 * k * self._rec,
                             self._pos.ptr + 4 * k * self._rec))
    self._steps[k] = step
    self._host = None

  def _series(self):
    if self._host is None:
      s = self.ens.stream
      self._host = (self._values.download(stream=s), self._pos.download(stream=s))
    return self._host

  @property
  def steps(self):
    return self._steps.copy()

  def depth(self, name):
    return self.table.depth_of(name, self.pos[name])
