"""SectionBatch: pymoc.plotting's section interpolators for every member of an ensemble, on the GPU.

Arithmetic contract: Interpolate_channel.__call__ / Interpolate_twocol.__call__ of the reference
(src/pymoc/plotting/interp_channel.py:40-62, interp_twocol.py:37-73) at every point of a query
grid, laid out as gridit lays it out (src/pymoc/utils/gridit.py:24-30).  Array and float profiles
give sections bit-identical to the reference's; one launch of pm_sections_grid
(pymoc_amd/csrc/sections.hip) fills all members.
"""
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import check, lib, pm_sections
from .device import DeviceArray, _sh

KINDS = {"channel": _lib.PM_SEC_CHANNEL, "twocol": _lib.PM_SEC_TWOCOL}
FIXUPS = {None: 0, "plot_overturning": _lib.PM_SEC_FIX_PLOT_OVERTURNING,
          "twobasin": _lib.PM_SEC_FIX_TWOBASIN}
STATUS_TEXT = {_lib.PM_SEC_OK: "ok", _lib.PM_SEC_ESIGN: "f(a) and f(b) must have different signs",
               _lib.PM_SEC_ECONV: "Failed to converge after 100 iterations.",
               _lib.PM_SEC_ENAN: "function value is NaN"}


def _axis(a, name):
  a = np.ascontiguousarray(a, dtype=np.float64)
  if a.ndim != 1:
    raise ValueError("%s must be a 1-D grid" % name)
  return a


class SectionBatch(object):
  """n members' sections on shared grids.

  kind    'channel' (Interpolate_channel: bs on y, bn on z) or 'twocol' (Interpolate_twocol:
          bs and bn on z).
  y, z    the classes' grids (1-D, ascending, 2..1024 points): l = y[-1], z[0] is the bottom.
  bs, bn  per profile one of
            - a float: make_func's float profile (value + 0*x), shared by every member;
            - a host array [n][len] (or [len], shared by every member);
            - a DeviceArray holding the rows in place, e.g. an ensemble's `cols.b`: member m's
              row starts `offset + m * stride` doubles into it (`bs_offset` / `bs_stride`,
              `bn_offset` / `bn_stride`; stride defaults to the row length).
  n       member count (needed when no profile is a host array).
  yq, zq  query grid (default: y, z -- the grid gridit uses), 1..1024 points each.
  fixups  the adjustments a reference script makes before it interpolates, applied to each
          member's copy while it is staged (the inputs are never changed):
            None               none (example_twocol_plusSO.py:138);
            'plot_overturning' channel: Plot_overturning.py:42-50 (bs[0] = bs[1] if
                               bs[0] > bs[1], then bn[0] = bs[0] if bs[0] < bn[0]);
                               twocol: :63-64 (bn[0] = bs[0], bs being the basin profile);
            'twobasin'         channel: twobasin_NadeauJansen.py:176 (bs[-1] = bn[-1]).  Its
                               two-column fix-up (:192-193, bn[0] = the mean basin profile's
                               bottom value) needs a third profile and stays with the caller.

  grid() returns the device array [n][nyq][nzq]; a point where the reference's brenth raises
  is NaN there, and status() / failed_points() say why and where.
  """

  def __init__(self, kind, y, z, bs, bn, n=None, yq=None, zq=None, fixups=None, bs_offset=0,
               bs_stride=None, bn_offset=0, bn_stride=None, stream=None):
    _lib.require_device()
    if kind not in KINDS:
      raise ValueError("kind must be 'channel' or 'twocol'")
    if fixups not in FIXUPS:
      raise ValueError("fixups must be None, 'plot_overturning' or 'twobasin'")
    if kind == "twocol" and fixups == "twobasin":
      raise ValueError("fixups='twobasin' is a channel fix-up: the two-column one of "
                       "twobasin_NadeauJansen.py:192-193 needs a third profile (do it on bn first)")
    self.kind, self.fixups, self.stream = kind, fixups, stream
    self.y_host, self.z_host = _axis(y, "y"), _axis(z, "z")
    self.yq_host = self.y_host if yq is None else _axis(yq, "yq")
    self.zq_host = self.z_host if zq is None else _axis(zq, "zq")
    ny, nz = self.y_host.size, self.z_host.size
    self.nyq, self.nzq = self.yq_host.size, self.zq_host.size
    nbs = nz if kind == "twocol" else ny
    self._keep = []
    self.flags = 0
    counts = []
    bs_p = self._profile(bs, "bs", nbs, bs_offset, bs_stride, _lib.PM_SEC_BS_SCALAR, counts)
    bn_p = self._profile(bn, "bn", nz, bn_offset, bn_stride, _lib.PM_SEC_BN_SCALAR, counts)
    if n is None:
      if not counts:
        raise ValueError("n is needed when no profile is a host array [n][len]")
      n = counts[0]
    self.n = int(n)
    for c in counts:
      if c != self.n:
        raise ValueError("profiles hold %d rows, n is %d" % (c, self.n))
    for p, name, length in ((bs_p, "bs", nbs), (bn_p, "bn", nz)):
      dev, off, stride, scalar = p
      if isinstance(dev, DeviceArray) and self.n > 0:
        last = off + (self.n - 1) * stride + (1 if scalar else length)
        if last * dev.dtype.itemsize > dev.nbytes:
          raise ValueError("%s: member rows run past the end of the device array" % name)
    if self.fixups and self.flags:
      raise ValueError("fix-ups need array profiles")
    self._bs, self._bn = bs_p, bn_p
    self.y = DeviceArray.from_host(self.y_host, stream=stream)
    self.z = DeviceArray.from_host(self.z_host, stream=stream)
    self.yq = DeviceArray.from_host(self.yq_host, stream=stream)
    self.zq = DeviceArray.from_host(self.zq_host, stream=stream)
    npts = self.nyq * self.nzq
    self.out = DeviceArray((max(self.n, 1), self.nyq, self.nzq))
    self._status = DeviceArray((max(self.n, 1) * npts,), np.uint8)
    self._first = DeviceArray((max(self.n, 1),), np.int32)

  def _profile(self, p, name, length, offset, stride, scalar_flag, counts):
    """-> (device array, offset, stride, scalar) in doubles."""
    if isinstance(p, DeviceArray):
      if p.dtype != np.float64:
        raise ValueError("%s must hold float64" % name)
      return (p, int(offset), length if stride is None else int(stride), False)
    if isinstance(p, float) or (isinstance(p, numbers.Real) and not isinstance(p, numbers.Integral)):
      self.flags |= scalar_flag
      d = DeviceArray.from_host(np.array([float(p)]), stream=self.stream)
      self._keep.append(d)
      return (d, 0, 0, True)
    if isinstance(p, np.ndarray):
      a = np.ascontiguousarray(p, dtype=np.float64)
      if a.ndim == 1:
        a = a[None, :]
        stride_rows = 0
      elif a.ndim == 2:
        counts.append(a.shape[0])
        stride_rows = length
      else:
        raise ValueError("%s must be [len] or [n][len]" % name)
      if a.shape[1] != length:
        raise ValueError("%s rows hold %d levels, the grid %d" % (name, a.shape[1], length))
      d = DeviceArray.from_host(a, stream=self.stream)
      self._keep.append(d)
      return (d, 0, stride_rows, False)
    raise TypeError(name, "needs to be a float, a numpy array or a DeviceArray")

  def descriptor(self):
    d = pm_sections()
    d.n, d.kind = self.n, KINDS[self.kind]
    d.ny, d.nz, d.nyq, d.nzq = self.y_host.size, self.z_host.size, self.nyq, self.nzq
    d.flags, d.fixups = self.flags, FIXUPS[self.fixups]
    d.y, d.z, d.yq, d.zq = self.y.ptr, self.z.ptr, self.yq.ptr, self.zq.ptr
    d.bs, d.bs_offset, d.bs_stride = self._bs[0].ptr, self._bs[1], self._bs[2]
    d.bn, d.bn_offset, d.bn_stride = self._bn[0].ptr, self._bn[1], self._bn[2]
    d.out, d.status, d.first = self.out.ptr, self._status.ptr, self._first.ptr
    return d

  def grid(self, stream=None):
    """One launch: the sections of all members, device array [n][nyq][nzq]."""
    s = self.stream if stream is None else stream
    d = self.descriptor()
    check(lib.pm_sections_grid(C.byref(d), _sh(s)))
    self._last_stream = s
    return self.out

  def status(self):
    """[n][nyq][nzq] uint8: 0 ok, 1 brenth's sign ValueError, 2 its RuntimeError (no
    convergence), 3 its NaN-value ValueError -- of the last grid()."""
    st = self._status.download(stream=getattr(self, "_last_stream", None))
    return st[:self.n * self.nyq * self.nzq].reshape(self.n, self.nyq, self.nzq)

  def failed_points(self):
    """[n] int32: each member's first failing point i * nzq + j in gridit's order, -1 none."""
    return self._first.download(stream=getattr(self, "_last_stream", None))[:self.n]
