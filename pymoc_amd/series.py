"""Series: what the Series* classes (stats, spectra, windows, smooth, surrogates, shifts) share --
the recorded series itself.

A series is an `IndexRecorder`'s device layout v[record][index][member], float64 [nrec, nspec, n].
This module is the one place that knows

  the source         an `IndexRecorder` (its values, its table's names, its ensemble's stream and
                     timer), or `(DeviceArray [nrec, nspec, n], names)` for any device series, with
                     `stream=` the stream that series is written on; the names are distinct, one
                     per index
  the record window  [k0, k1) inside the nrec records (k1 = None: nrec); with a recorder as source
                     a window that holds a record never written (`rec.steps == -1`) is a ValueError
  a device view      anything with `.ptr` and `.shape` = (nrec, nspec, n): a DeviceArray, a `View`
                     (`records`: a record window of one), a `_Plane` (out[i] of a device array,
                     with `keep`, what it was computed from and must outlive it)
  the launch context `Ctx` = (stream, timer): where a launch function (launch_*: a view, plain
                     parameters, a context) enqueues its kernel and records its span
  indexing by name   `by_name`: `result.mean[name]`, one dict for every result class

and the small pieces around a launch: the lazy upload of host mirrors, the check of an integer
argument and of group labels.  A limit one kernel has (nspec <= 65535, say) stays with its class.
"""
import collections

import numpy as np

from .device import DeviceArray


def as_int(what, val):
  """int(val) of an integer argument; a bool, a float or a string is a ValueError."""
  if not isinstance(val, (int, np.integer)) or isinstance(val, bool):
    raise ValueError("%s must be an integer (%r here)" % (what, val))
  return int(val)


class _Named(dict):
  """{name: the rows of one index}; an unknown name is a KeyError that lists the known ones."""

  def __missing__(self, name):
    raise KeyError("unknown index %r (one of %s)" % (name, ", ".join(map(str, self))))


def by_name(names, arr):
  """`result.mean[name]`: {names[s]: arr[s]}, every entry an array of its own."""
  return _Named((nm, np.ascontiguousarray(arr[s])) for s, nm in enumerate(names))


Ctx = collections.namedtuple("Ctx", "stream timer")
View = collections.namedtuple("View", "ptr shape")


def records(x, k0, k1):
  """The records [k0, k1) of the device view `x` as a view of their own (x owns the memory)."""
  return View(x.ptr + 8 * k0 * int(np.prod(x.shape[1:])), (k1 - k0,) + tuple(x.shape[1:]))


class _Plane(object):
  """out[i] of a device array out[..][nrec][nspec][n] as a device series of its own, `shape` =
  (nrec, nspec, n): an address, a shape and a dtype.  The parent owns the memory and is kept
  alive, and so is `keep`: the device arrays the plane was computed from by a launch that may not
  have run yet."""

  def __init__(self, parent, i, shape, keep=()):
    self._parent, self.shape, self.dtype = parent, tuple(shape), np.dtype(np.float64)
    self.ptr = parent.ptr + 8 * i * int(np.prod(shape))
    self.keep = tuple(keep)


class Series(object):
  """A checked source: `_rec` (the recorder or None), `_series`, `names`, `stream`, `nrec`, `nspec`,
  `n`.  The base of the Series* classes."""

  def __init__(self, source, stream=None):
    self._rec = None
    if isinstance(source, tuple):
      if len(source) != 2:
        raise ValueError("a source is an IndexRecorder or (DeviceArray [nrec, nspec, n], names)")
      arr, names = source
      self.stream = stream
    else:
      self._rec = source
      arr, names = source._values, source.table.names
      self.stream = source.ens.stream
    shape = tuple(getattr(arr, "shape", ()))
    if len(shape) != 3 or min(shape) < 1 or np.dtype(getattr(arr, "dtype", None)) != np.float64:
      raise ValueError("the series must be a float64 device array [nrec, nspec, n] (shape %r here)"
                       % (shape,))
    self.nrec, self.nspec, self.n = shape
    self.names = list(names)
    if len(self.names) != self.nspec or len(set(self.names)) != self.nspec:
      raise ValueError("the series has %d indices but %d distinct names are given"
                       % (self.nspec, len(set(self.names))))
    self._series = arr
    self._host, self._dev = {}, None

  def _set_groups(self, groups):
    """`groups` for a later `across_members`, checked now as SeriesStats will check it."""
    from .stats import group_order  # (stats derives from this module)
    if groups is not None:
      group_order(groups, self.n)
    self.groups = groups

  def _record_window(self, k0, k1):
    k0 = int(k0)
    k1 = self.nrec if k1 is None else int(k1)
    if not 0 <= k0 < k1 <= self.nrec:
      raise ValueError("window [%d, %d) is not inside the %d records" % (k0, k1, self.nrec))
    if self._rec is not None:
      missing = np.nonzero(self._rec.steps[k0:k1] < 0)[0]
      if missing.size:
        raise ValueError("window [%d, %d) holds record %d, which was never written"
                         % (k0, k1, k0 + missing[0]))
    return k0, k1

  def _timer(self):
    return self._rec.ens.timer if self._rec is not None else None

  def _ctx(self):
    return Ctx(self.stream, self._timer())

  def _upload(self):
    """{key: device copy} of the host mirrors `_host` (the entries check the host side), made on
    the source's stream at the first launch."""
    if self._dev is None:
      self._dev = {key: DeviceArray.from_host(a, dtype=a.dtype, stream=self.stream)
                   for key, a in self._host.items()}
    return self._dev
