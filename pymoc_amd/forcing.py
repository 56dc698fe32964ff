"""ForcingSchedule: time-dependent forcing of a coupled ensemble, evaluated on the device.

The reference's transient experiments assign `basin.bs`, `north.bs`, `PsiSO.tau`, `channel.b_rest`
as functions of time at the top of the user loop.  A schedule states such functions for a whole
ensemble as piecewise-linear knots; `TwoColEnsemble(cfg, forcing=...)` and
`JN2018Ensemble(cfg, forcing=...)` evaluate it with one launch of pm_forcing_apply at the first
step of every launch interval (CoupledEnsemble._apply_forcing states the rule) into the device
arrays their kernels re-read at every launch -- no host interpolation, no upload, no
synchronisation while the ensemble runs.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh


class ForcingSchedule(object):
  """`ForcingSchedule(t, bs=..., tau=..., ...)`: K strictly increasing finite knot times `t`
  (seconds; model time is step * dt) and, per target, the values at the knots, knot axis first:
    a per-member scalar target (bs, bs_north, a scalar tau)   [K] shared or [K, n]
    a profile target (bs_SO, b_rest, surflux, a tau profile)   [K, ny] shared or [K, n, ny]
  Between knots a value is np.interp's, bit for bit; before the first and after the last knot it
  is held.  The target names are the driver's (its FORCING_TARGETS); the driver checks names and
  shapes against its cfg when it is built, on the host, and uploads the values once."""

  def __init__(self, t, **targets):
    t = np.array(t, dtype=np.float64, ndmin=1)
    if t.ndim != 1 or t.size < 1:
      raise ValueError("t must be a 1-D array of at least one knot time")
    if not np.isfinite(t).all():
      raise ValueError("t must be finite")
    if not (np.diff(t) > 0).all():
      raise ValueError("t must be strictly increasing")
    if not targets:
      raise ValueError("a ForcingSchedule needs at least one target")
    self.t = np.ascontiguousarray(t)
    self.values = {}
    for key, v in targets.items():
      a = np.ascontiguousarray(v, dtype=np.float64)
      if a.ndim < 1 or a.ndim > 3 or a.shape[0] != t.size:
        raise ValueError("forcing target %r: shape %r does not carry the %d knots on its first "
                         "axis ([K], [K, n], [K, ny] or [K, n, ny])" % (key, a.shape, t.size))
      self.values[key] = a

  @property
  def K(self):
    return self.t.size

  def check(self, lengths, n):
    """Names and shapes against a driver's targets {name: row length} for n members -- host only.
    Returns {name: is it per member?}."""
    K, out = self.K, {}
    for key, a in self.values.items():
      if key not in lengths:
        raise ValueError("unknown forcing target %r: this ensemble takes %s"
                         % (key, ", ".join(sorted(lengths))))
      ln = lengths[key]
      shared, per = ((K,), (K, n)) if ln == 1 else ((K, ln), (K, n, ln))
      if a.shape == per:
        out[key] = True
      elif a.shape == shared:
        out[key] = False
      else:
        raise ValueError("forcing target %r: shape %r, but its rows have %d value%s here: %r "
                         "(shared) or %r (per member)"
                         % (key, a.shape, ln, "" if ln == 1 else "s", shared, per))
    if len(out) > _lib.PM_FORCING_MAX_TARGETS:
      raise ValueError("a schedule holds at most %d targets" % _lib.PM_FORCING_MAX_TARGETS)
    return out

  def bind(self, n, targets, stream=None):
    """Upload the values and return the BoundForcing that writes them: `targets` maps each name
    of this schedule to (DeviceArray, first row, row length), or to a list of such destinations
    of one row length (a value the driver keeps in more than one place)."""
    targets = {k: [d] if isinstance(d, tuple) else list(d) for k, d in targets.items()}
    for k, dests in targets.items():
      if len({ln for _, _, ln in dests}) != 1:
        raise ValueError("forcing target %r: its destinations differ in row length" % k)
    per = self.check({k: dests[0][2] for k, dests in targets.items()}, n)
    return BoundForcing(self, n, targets, per, stream)


class BoundForcing(object):
  """A schedule's values in HBM and the pm_forcing that writes them into one ensemble's arrays."""

  def __init__(self, schedule, n, targets, per_member, stream=None):
    self.schedule, self.n = schedule, int(n)
    self.knots = schedule.t  # host array the descriptor points to: kept alive here
    d = self.desc = _lib.pm_forcing()
    ndest = sum(len(targets[key]) for key in per_member)
    if ndest > _lib.PM_FORCING_MAX_TARGETS:
      raise ValueError("a schedule writes at most %d destinations (%d here)"
                       % (_lib.PM_FORCING_MAX_TARGETS, ndest))
    d.n, d.K, d.ntargets, d.reserved = self.n, schedule.K, ndest, 0
    d.knots = self.knots.ctypes.data
    self.arrays = []
    i = 0
    for key, per in per_member.items():
      vals = DeviceArray.from_host(schedule.values[key], stream=stream)  # one upload per name
      for dst, row0, ln in targets[key]:
        if (row0 + self.n) * ln * 8 > dst.nbytes or dst.dtype != np.float64:
          raise ValueError("forcing target %r: rows [%d, %d) of %d values lie outside its array"
                           % (key, row0, row0 + self.n, ln))
        self.arrays.append((dst, vals))  # (the targets must outlive the descriptor)
        g = d.target[i]
        g.dst, g.row0, g.values, g.len, g.per_member = (dst.ptr, int(row0), vals.ptr, int(ln),
                                                        int(per))
        i += 1

  def apply(self, t, stream=None):
    check(lib.pm_forcing_apply(C.byref(self.desc), float(t), _sh(stream)))
