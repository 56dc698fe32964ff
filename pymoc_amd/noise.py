"""NoiseForcing: stochastic forcing of a coupled ensemble, generated on the device.

The other classic use of a thousands-member column model next to a deterministic sweep: AMOC
variability under fluctuating surface buoyancy or wind, noise-induced transitions, spread around a
forced trajectory.  `TwoColEnsemble(cfg, noise=NoiseForcing(seed, tau=dict(sigma=0.02)))` perturbs
the driver's forcing arrays with one red-noise state per (target, member):

  x <- a x + (sigma b) xi,   a = exp(-dt / tau_corr),  b = sqrt(1 - a a)
  value = base + x pattern

at the instants a ForcingSchedule is applied at (CoupledEnsemble._apply_forcing states the rule),
with ONE launch of pm_forcing_noise -- no host work, no upload and no synchronisation while the
ensemble runs.  xi is a standard normal deviate of a counter-based generator: it depends on the
seed, the member's GLOBAL index, the application index and the target only, so a run is
reproducible whatever the batch size, the shard and the other perturbed targets
(include/pymoc_hip.h states the definition).  `base` is the cfg's value of the target, or what a
ForcingSchedule on the same target writes.  The noise is constant within a launch interval.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh

# a target's position here is the `stream` word of its deviates' counter
STREAMS = ("bs", "bs_north", "tau", "b_rest", "surflux", "bs_SO")


def application(s, M, phase, dt):
  """THE rule of the application index: (j, model time since the previous application) when
  forcing is applied at the top of loop iteration s -- s = 0 and every s = phase (mod M), the
  instants of CoupledEnsemble._apply_forcing -- else None.  j counts those instants from 0 at
  s = 0; the time is (s_j - s_{j-1}) * dt, and 0.0 at j = 0."""
  s, M = int(s), int(M)
  p = int(phase) % M
  if s < 0 or not (s == 0 or s % M == p):
    return None
  if s == 0:
    return 0, 0.0
  if p == 0:
    return s // M, M * float(dt)
  j = 1 + (s - p) // M
  return j, (p if j == 1 else M) * float(dt)


def ar1(tau_corr, elapsed):
  """(a, b) of one application `elapsed` seconds after the previous one, in float64:
  a = exp(-elapsed / tau_corr), b = sqrt(1 - a * a); tau_corr = 0 is white noise (0, 1),
  tau_corr = inf a frozen state (1, 0)."""
  tau = np.float64(tau_corr)
  if tau == 0.0:
    return 0.0, 1.0
  if np.isinf(tau):
    return 1.0, 0.0
  a = np.exp(-np.float64(elapsed) / tau)
  return float(a), float(np.sqrt(1.0 - a * a))


class NoiseForcing(object):
  """`NoiseForcing(seed, bs=dict(sigma=...), tau=dict(sigma=..., tau_corr=..., pattern=...))`:
    seed      an integer in [0, 2^64): the generator's key
    sigma     the stationary standard deviation of the target's noise state, >= 0 and finite: a
              scalar or one value per member [n]
    tau_corr  its decorrelation time in seconds: 0 (default) white -- a new deviate at every
              application --, inf frozen at its first value
    pattern   for a profile target, what the state multiplies: [len] or per member [n, len]
              (default: 1 at every point).  A one-value target takes none.
  The target names are the driver's FORCING_TARGETS; the driver checks names and shapes against
  its cfg when it is built, on the host."""

  def __init__(self, seed, **targets):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
      raise ValueError("seed must be an integer in [0, 2**64)")
    if not 0 <= int(seed) < 2**64:
      raise ValueError("seed %d outside [0, 2**64)" % int(seed))
    if not targets:
      raise ValueError("a NoiseForcing needs at least one target")
    self.seed = int(seed)
    self.targets = {}
    for key, spec in targets.items():
      if key not in STREAMS:
        raise ValueError("unknown noise target %r: one of %s" % (key, ", ".join(STREAMS)))
      if not isinstance(spec, dict) or "sigma" not in spec:
        raise ValueError("noise target %r: a dict(sigma=..., tau_corr=0.0, pattern=None)" % key)
      extra = set(spec) - {"sigma", "tau_corr", "pattern"}
      if extra:
        raise ValueError("noise target %r: unknown entries %s" % (key, ", ".join(sorted(extra))))
      sigma = np.asarray(spec["sigma"], dtype=np.float64)
      if sigma.ndim > 1 or not np.isfinite(sigma).all() or (sigma < 0).any():
        raise ValueError("noise target %r: sigma must be finite and >= 0, a scalar or [n]" % key)
      tau = float(spec.get("tau_corr", 0.0))
      if not tau >= 0.0:  # (a NaN too)
        raise ValueError("noise target %r: tau_corr %r is negative or NaN" % (key, tau))
      pattern = spec.get("pattern")
      if pattern is not None:
        pattern = np.asarray(pattern, dtype=np.float64)
        if pattern.ndim not in (1, 2):
          raise ValueError("noise target %r: pattern must be [len] or [n, len]" % key)
      self.targets[key] = dict(sigma=sigma, tau_corr=tau, pattern=pattern)

  def check(self, lengths, n):
    """Names and shapes against a driver's targets {name: row length} for n members -- host only.
    Returns {name: is the pattern per member? (None: no pattern)}."""
    out = {}
    for key, spec in self.targets.items():
      if key not in lengths:
        raise ValueError("unknown noise target %r: this ensemble takes %s"
                         % (key, ", ".join(sorted(lengths))))
      ln, sigma, pattern = lengths[key], spec["sigma"], spec["pattern"]
      if sigma.ndim == 1 and sigma.shape[0] != n:
        raise ValueError("noise target %r: sigma of length %d for %d members"
                         % (key, sigma.shape[0], n))
      out[key] = None
      if pattern is not None:
        if ln == 1:
          raise ValueError("noise target %r: its rows have 1 value here, it takes no pattern" % key)
        if pattern.shape not in ((ln,), (n, ln)):
          raise ValueError("noise target %r: pattern of shape %r, but its rows have %d values "
                           "here: %r or %r" % (key, pattern.shape, ln, (ln,), (n, ln)))
        out[key] = pattern.ndim == 2
    if len(out) > _lib.PM_NOISE_MAX_TARGETS:
      raise ValueError("a NoiseForcing holds at most %d targets" % _lib.PM_NOISE_MAX_TARGETS)
    return out

  def bind(self, n, targets, member0=0, stream=None):
    """Upload sigma and the patterns, copy the destinations' current values as `base` and return
    the BoundNoise that perturbs them: `targets` maps each name of this object to (DeviceArray,
    first row, row length), or to a list of such destinations of one row length (a value the
    driver keeps in more than one place: they share one noise state)."""
    targets = {k: [d] if isinstance(d, tuple) else list(d) for k, d in targets.items()}
    for k, dests in targets.items():
      if len({ln for _, _, ln in dests}) != 1:
        raise ValueError("noise target %r: its destinations differ in row length" % k)
    per = self.check({k: dests[0][2] for k, dests in targets.items()}, n)
    return BoundNoise(self, n, targets, per, member0, stream)


class BoundNoise(object):
  """A NoiseForcing's device state for one ensemble -- per name `base` [n, len], the two state
  buffers [n] the applications alternate between, sigma [n], the pattern -- and the pm_noise that
  perturbs the ensemble's arrays.  `base[name]` is what a ForcingSchedule on the same target
  writes instead of the destination."""

  def __init__(self, noise, n, targets, per_member, member0=0, stream=None):
    self.noise, self.n, self.stream = noise, int(n), stream
    if int(member0) < 0:
      raise ValueError("member0 %d < 0" % member0)
    ndest = sum(len(targets[key]) for key in per_member)
    if ndest > _lib.PM_NOISE_MAX_TARGETS:
      raise ValueError("a NoiseForcing writes at most %d destinations (%d here)"
                       % (_lib.PM_NOISE_MAX_TARGETS, ndest))
    d = self.desc = _lib.pm_noise()
    d.n, d.ntargets, d.j, d.reserved = self.n, ndest, 0, 0
    d.seed, d.member0 = noise.seed, int(member0)
    self.names = list(per_member)
    self.base, self.tau_corr = {}, {}
    self._x = {}       # name -> [the buffer the next application reads, the one it writes]
    self._live = {}    # name -> has its state been set (by an application or by set_state)?
    self._entries = {}  # name -> the descriptor entries of its destinations
    self._keep = []
    i = 0
    for key, per in per_member.items():
      spec = noise.targets[key]
      ln = int(targets[key][0][2])
      for dst, row0, _ in targets[key]:
        if (row0 + self.n) * ln * 8 > dst.nbytes or dst.dtype != np.float64:
          raise ValueError("noise target %r: rows [%d, %d) of %d values lie outside its array"
                           % (key, row0, row0 + self.n, ln))
      first, row0, _ = targets[key][0]
      base = DeviceArray((self.n, ln))
      check(lib.pm_memcpy_d2d(base.ptr, first.ptr + 8 * int(row0) * ln, base.nbytes, _sh(stream)))
      sigma = DeviceArray.from_host(np.broadcast_to(spec["sigma"], (self.n,)), stream=stream)
      pattern = (None if spec["pattern"] is None
                 else DeviceArray.from_host(spec["pattern"], stream=stream))
      self.base[key], self.tau_corr[key] = base, spec["tau_corr"]
      self._x[key] = [DeviceArray.zeros((self.n,), stream=stream) for _ in range(2)]
      self._live[key] = False
      self._entries[key] = []
      for dst, row0, _ in targets[key]:
        g = d.target[i]
        g.dst, g.row0, g.base, g.sigma = dst.ptr, int(row0), base.ptr, sigma.ptr
        g.pattern = None if pattern is None else pattern.ptr
        g.len, g.pattern_per_member, g.stream = ln, int(bool(per)), STREAMS.index(key)
        g.xi_out, g.reserved = None, 0
        self._entries[key].append(g)
        self._keep.append((dst, sigma, pattern))  # (the targets must outlive the descriptor)
        i += 1

  def apply(self, j, elapsed, stream=None):
    """Application j, `elapsed` seconds of model time after the previous one (`application`):
    one launch; a state that has never been set starts stationary, x = sigma * xi."""
    d = self.desc
    d.j = int(j)
    for key in self.names:
      a, b = ar1(self.tau_corr[key], elapsed) if self._live[key] else (0.0, 1.0)
      x_in, x_out = self._x[key]
      for k, g in enumerate(self._entries[key]):
        g.a, g.b, g.x_in = a, b, x_in.ptr
        g.x_out = x_out.ptr if k == 0 else None
    check(lib.pm_forcing_noise(C.byref(d), _sh(stream)))
    for key in self.names:
      self._x[key].reverse()
      self._live[key] = True

  def get_state(self):
    """{name: x [n]}: the noise states after the last application, as host arrays."""
    return {key: self._x[key][0].download(stream=self.stream) for key in self.names}

  def set_state(self, state):
    """Take {name: x [n]} as the states the next application advances (every name of this
    object, or some): a run continues another's noise.  A state set ahead of the first
    application is advanced like any other -- at s = 0 no model time has passed, so a red state
    is written as it is and a white one is drawn anew."""
    for key, x in state.items():
      if key not in self._x:
        raise ValueError("unknown noise target %r: this object holds %s"
                         % (key, ", ".join(self.names)))
      x = np.ascontiguousarray(x, dtype=np.float64)
      if x.shape != (self.n,):
        raise ValueError("noise target %r: a state of shape %r for %d members"
                         % (key, x.shape, self.n))
      self._x[key][0].upload(x, self.stream)
      self._live[key] = True
