"""What Interpolate_channel and Interpolate_twocol share: the device path (one launch of
pm_sections_grid through SectionBatch) and the decision whether a profile can take it."""
import numpy as np

from ..utils.gridit import gridit as _gridit
from ..utils.coerce import make_func


def _device_profile(fn, axis):
  """The float / float64 array behind a make_func closure, read NOW (the reference's closures see
  in-place edits of the caller's array), or None when only the host can evaluate `fn`."""
  src = getattr(fn, "_pm_source", None)
  if src is None:
    return None
  if isinstance(src, float):
    return float(src)
  if (isinstance(src, np.ndarray) and src.ndim == 1 and src.size == axis.size and
      src.dtype.kind in "fiub"):
    return np.ascontiguousarray(src, dtype=np.float64)
  return None  # np.interp itself raises on this: the host path reproduces its error


def _sorted_axis(a):
  return isinstance(a, np.ndarray) and a.ndim == 1 and a.size >= 2 and bool(np.all(a[1:] >= a[:-1]))


class _Section(object):
  _kind = None

  def __init__(self, y=None, z=None, bs=None, bn=None):
    if isinstance(y, np.ndarray):
      self.y = y
    else:
      raise TypeError('y needs to be numpy array providing grid levels')
    if isinstance(z, np.ndarray):
      self.z = z
    else:
      raise TypeError('z needs to be numpy array providing grid levels')
    self.bs = self.make_func(bs, 'bs', self._bs_axis())
    self.bn = self.make_func(bn, 'bn', self.z)

  def make_func(self, myst, name, xin):
    return make_func(myst, xin, name)

  def _bs_axis(self):
    raise NotImplementedError

  def _batch(self, yq, zq):
    """A one-member SectionBatch of the current profiles on the query grid, or None when a
    profile is a callable (or otherwise something only the host evaluates)."""
    if not (_sorted_axis(self.y) and _sorted_axis(self.z)):
      return None
    bs = _device_profile(self.bs, np.asarray(self._bs_axis()))
    bn = _device_profile(self.bn, np.asarray(self.z))
    if bs is None or bn is None:
      return None
    from ..sections import SectionBatch
    return SectionBatch(self._kind, self.y, self.z, bs, bn, n=1, yq=yq, zq=zq)

  def _device(self, batch):
    """Run `batch`; on a failing point raise what the reference raises there (the host twin
    recomputes that one point, which raises brenth's exception with its message)."""
    out = batch.grid().download()[0]
    first = int(batch.failed_points()[0])
    if first >= 0:
      i, j = divmod(first, batch.nzq)
      self._host_call(batch.yq_host[i], batch.zq_host[j])
      raise RuntimeError("the device reports a failing point (%d, %d) that the host twin "
                         "evaluates without error" % (i, j))
    return out

  def __call__(self, y, z):
    if np.ndim(y) == 0 and np.ndim(z) == 0 and np.isrealobj(y) and np.isrealobj(z):
      batch = self._batch(np.array([y], dtype=np.float64), np.array([z], dtype=np.float64))
      if batch is not None:
        return np.float64(self._device(batch)[0, 0])
    return self._host_call(y, z)

  def gridit(self):
    batch = self._batch(None, None)
    if batch is None:
      return _gridit(self.y, self.z, self)
    return self._device(batch)
