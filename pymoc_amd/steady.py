"""Run a coupled ensemble to steady state, retiring members as they converge.

The reference's equilibrium experiments step for a fixed, long time (run_JansenNadeau_2018.py:96-97
12 000 years, example_twocol.py:32 4 000 years) because they have no test for "done".
`run_to_steady` steps a JN2018Ensemble, TwoColEnsemble or TwoBasinSweep and, every `check_every` steps, measures
each member's drift -- the largest change of its prognostic profiles since the last check, in
buoyancy units per 360-day year -- with one launch of pm_steady_check.  A member whose drift stays
at or below its tolerance for `consecutive` checks is retired: its state and overturning at that
check are captured, and it no longer changes.  When few enough members are left running, the
ensemble is rebuilt from them alone (compaction), so retired members stop costing anything.

Checks fall only on states the loop can be restarted from exactly:
  JN2018Ensemble  at s = 0 (mod MOC_up_iters), after that step's MOC update, before the step
                  (run_JansenNadeau_2018.py:204-217);
  TwoColEnsemble  at s = 1 (mod MOC_up_iters), after the update that follows step s - 1
                  (example_twocol.py:85-96);
  TwoBasinSweep   likewise at s = 1 (mod MOC_up_iters) (twobasin_NadeauJansen.py:99-122).
Members never interact and every path through the kernels is bit-identical, so a member's
captured state equals a plain run's after the same number of steps, compacted or not.
"""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, Event, PinnedArray, download_async, rows_pack, _sh
from .ensembles import CoupledEnsemble

YEAR = 360 * 86400.  # the scripts' year (run_JansenNadeau_2018.py:39)

RUNNING = _lib.PM_STEADY_RUNNING
CONVERGED = _lib.PM_STEADY_CONVERGED
NONFINITE = _lib.PM_STEADY_NONFINITE
MAXSTEPS = _lib.PM_STEADY_MAXSTEPS


def _restartable(cls):
  """`cls` if it states how its cfg is read per member and where it can be restarted
  (CoupledEnsemble.MEMBER_KEYS, RESTART_PHASE)."""
  if not (isinstance(cls, type) and issubclass(cls, CoupledEnsemble) and cls.MEMBER_KEYS):
    raise ValueError("run_to_steady supports JN2018Ensemble and TwoColEnsemble (and their "
                     "subclasses) and TwoBasinSweep, not %r" % getattr(cls, "__name__", cls))
  return cls


def restrict_cfg(cls, cfg, keep):
  """`cfg` restricted to members `keep` (indices into its current members), by the rule the
  constructor of `cls` reads each key with (CoupledEnsemble.restrict)."""
  return _restartable(cls).restrict(cfg, keep)


def check_schedule(cls, moc_up_iters, check_every, max_steps):
  """(s0, [check steps]): the first snapshot at s0, then a check every `check_every` steps; the
  last check falls on the last restartable step <= max_steps (it finalizes)."""
  s0 = _restartable(cls).RESTART_PHASE
  M, E, S = int(moc_up_iters), int(check_every), int(max_steps)
  if M < 1:
    raise ValueError("MOC_up_iters must be >= 1")
  if E < 1 or E % M:
    raise ValueError("check_every=%d is not a positive multiple of MOC_up_iters=%d" % (E, M))
  last = s0 + ((S - s0) // M) * M if S >= s0 else s0
  if last <= s0:
    raise ValueError("max_steps=%d leaves no check after the first snapshot at step %d"
                     % (S, s0))
  return s0, list(range(s0 + E, last, E)) + [last]


def _validate(cls, cfg, kw, check_every):
  _restartable(cls)
  if kw.get("arith", "exact") != "exact":
    raise ValueError("run_to_steady needs arith='exact' (its results are bit-identical to a "
                     "plain run)")
  if kw.get("fused_run"):
    raise ValueError("run_to_steady does not drive the persistent fused_run kernels")
  if kw.get("forcing") is not None:
    raise ValueError("run_to_steady does not take forcing: an ensemble under a time-dependent "
                     "schedule has no steady state to run to")
  if kw.get("noise") is not None:
    raise ValueError("run_to_steady does not take noise: an ensemble under a time-dependent "
                     "schedule has no steady state to run to")
  if kw.get("comm") is not None or kw.get("keep_history"):
    raise ValueError("run_to_steady does not take comm or keep_history: call it per rank and "
                     "gather the results")
  M = int(cfg["MOC_up_iters"])
  if check_every is None:
    check_every = cfg.get("Diag_iters") or 10 * M
  return M, int(check_every)


class SteadyResult(object):
  """What run_to_steady returns, member order as in `cfg`:
    status        int32[n]  RUNNING never appears: CONVERGED, NONFINITE or MAXSTEPS
    steps         int64[n]  steps taken when the member retired
    drift         float64[n] its drift at that check (buoyancy per 360-day year; NaN if NONFINITE)
    fields        name -> [n, len]: the captured rows (drift fields, Psi, Psi_SO; for
                  TwoBasinSweep the three columns and the four overturnings)
    compactions   [(step, rows_before, rows_after)]
    member_steps  rows x steps actually stepped"""

  def __init__(self, status, steps, drift, fields, compactions, member_steps, dt, check_every):
    self.status, self.steps, self.drift, self.fields = status, steps, drift, fields
    self.compactions, self.member_steps = compactions, int(member_steps)
    self.dt, self.check_every = float(dt), int(check_every)

  @property
  def years(self):
    """Retirement time of each member in 360-day years."""
    return self.steps * self.dt / YEAR

  def counts(self):
    return {name: int(np.sum(self.status == v)) for name, v in
            (("converged", CONVERGED), ("nonfinite", NONFINITE), ("maxsteps", MAXSTEPS))}


class _Run(object):
  """The device side of one run_to_steady: snapshot, capture and per-member arrays, the current
  ensemble and its rows' original member numbers."""

  def __init__(self, cls, cfg, kw, tol, consecutive):
    self.cfg, self.kw = cfg, kw
    self.stream = kw.get("stream")
    self.ens = cls(cfg, **kw)
    self.n0 = self.rows = self.ens.n
    self.consecutive = consecutive
    d = self.ens.capture_fields()
    self.drift_names = [f[0] for f in self.ens.drift_fields()]
    self.capture_names = [f[0] for f in d]
    self.lens = {f[0]: f[3] for f in d}
    st = self.stream
    self.snap = {k: DeviceArray((self.n0, self.lens[k])) for k in self.drift_names}
    self.cap = {k: DeviceArray.zeros((self.n0, self.lens[k]), stream=st)
                for k in self.capture_names}
    self.orig_h = np.arange(self.n0, dtype=np.int32)
    self.orig = DeviceArray.from_host(self.orig_h, stream=st)
    self.tol = DeviceArray.from_host(tol, dtype=np.float64, stream=st)
    self.streak = DeviceArray.zeros((self.n0,), np.int32, stream=st)
    self.status = DeviceArray.zeros((self.n0,), np.int32, stream=st)
    self.drift = DeviceArray.zeros((self.n0,), np.float64, stream=st)
    self.step_out = DeviceArray.zeros((self.n0,), np.int64, stream=st)
    self.n_running = DeviceArray.zeros((1,), np.int32, stream=st)
    self.pinned = PinnedArray((2,), np.int32)
    self.events = [Event(), Event()]

  def snapshot(self):
    """The first snapshot: every drift field's rows, identity selection."""
    rows_pack([(src.ptr, self.snap[k].ptr, ln, stride) for k, src, stride, ln in
               self.ens.drift_fields()], self.rows, None, self.stream)

  def check(self, step, interval, finalize, slot):
    c = _lib.pm_steady_check()
    c.n, c.n0 = self.rows, self.n0
    fields = self.ens.capture_fields()  # the drift fields first
    c.ndrift, c.ncapture = len(self.drift_names), len(fields)
    c.consecutive, c.finalize, c.step = self.consecutive, int(bool(finalize)), int(step)
    c.scale = YEAR / (interval * self.ens.dt)
    c.orig, c.tol, c.streak, c.status = (self.orig.ptr, self.tol.ptr, self.streak.ptr,
                                         self.status.ptr)
    c.drift_out, c.step_out, c.n_running = self.drift.ptr, self.step_out.ptr, self.n_running.ptr
    for i, (k, src, stride, ln) in enumerate(fields):
      if i < c.ndrift:
        c.drift[i].src, c.drift[i].src_stride, c.drift[i].buf, c.drift[i].len = (
            src.ptr, stride, self.snap[k].ptr, ln)
      c.capture[i].src, c.capture[i].src_stride, c.capture[i].buf, c.capture[i].len = (
          src.ptr, stride, self.cap[k].ptr, ln)
    _lib.check(_lib.lib.pm_steady_check(C.byref(c), _sh(self.stream)))
    download_async(self.n_running.ptr, 4, self.pinned, self.stream, offset=4 * slot)
    self.events[slot].record(self.stream)

  def count(self, slot):
    self.events[slot].sync()
    return int(self.pinned.array[slot])

  def sync(self):
    _lib.check(_lib.lib.pm_stream_sync(_sh(self.stream)))

  def compact(self):
    """Rebuild the ensemble from its running rows (one synchronisation).  Returns the number of
    rows left."""
    self.sync()
    status = self.status.download(stream=self.stream)
    keep = np.nonzero(status[self.orig_h] == RUNNING)[0]
    if keep.size == 0 or keep.size == self.rows:
      return keep.size
    st = self.stream
    new = self.ens.subset(keep, self.cfg, self.kw)
    cfg = type(new).restrict(self.cfg, keep)  # (its state keys are replaced at the next subset)
    sel = DeviceArray.from_host(keep.astype(np.int32), stream=st)
    snap = {k: DeviceArray((keep.size, self.lens[k])) for k in self.drift_names}
    rows_pack([(self.snap[k].ptr, snap[k].ptr, self.lens[k], self.lens[k])
               for k in self.drift_names], keep.size, sel, st)
    self.orig_h = self.orig_h[keep]
    self.orig = DeviceArray.from_host(self.orig_h, stream=st)
    self.sync()  # the gather has read the old snapshot before it is freed
    self.snap, self.ens, self.cfg, self.rows = snap, new, cfg, int(keep.size)
    return self.rows


def run_to_steady(cls, cfg, tol, max_steps, check_every=None, consecutive=1, compact_below=0.5,
                  **ensemble_kwargs):
  """Step `cls(cfg, **ensemble_kwargs)` (JN2018Ensemble, TwoColEnsemble with or without the
  SO channel, or TwoBasinSweep) until every member has converged, gone non-finite or reached `max_steps`.

  tol           drift tolerance, buoyancy units per 360-day year: a scalar or one per member
  max_steps     cap; the last check is on the last restartable step <= max_steps
  check_every   steps between checks, a multiple of MOC_up_iters (default cfg['Diag_iters'], else
                10 MOC_up_iters)
  consecutive   checks in a row at or below tol that make a member converged
  compact_below rebuild the ensemble from its running members once at most this share of the rows
                is still running (0: never, 1: at every check that retired a member)
Returns a SteadyResult.  Refused (ValueError): other classes, arith != 'exact', fused_run, comm,
keep_history, forcing (a ForcingSchedule), noise (a NoiseForcing), a check_every that is not a multiple of MOC_up_iters."""
  M, check_every = _validate(cls, cfg, ensemble_kwargs, check_every)
  s0, checks = check_schedule(cls, M, check_every, max_steps)
  if int(consecutive) < 1:
    raise ValueError("consecutive must be >= 1")
  if not 0. <= float(compact_below) <= 1.:
    raise ValueError("compact_below must lie in [0, 1]")
  n0 = cls.members(cfg)
  tol = np.asarray(tol, dtype=np.float64)
  tol = np.full(n0, tol) if tol.ndim == 0 else tol
  if tol.shape != (n0,) or np.isnan(tol).any():
    raise ValueError("tol must be a scalar or one non-NaN value per member (%d)" % n0)

  r = _Run(cls, cfg, dict(ensemble_kwargs), tol, int(consecutive))
  compactions, member_steps = [], 0
  if s0:
    r.ens.run(s0)  # TwoColEnsemble: step 0 and the update that follows it
    member_steps += r.rows * s0
  r.snapshot()
  prev, pending = s0, None
  for j, s in enumerate(checks):
    final = j == len(checks) - 1
    nsteps = s - r.ens.ii
    r.ens.run(nsteps)
    member_steps += r.rows * nsteps
    r.ens.at_restart_point()
    slot = j % 2
    r.check(s, s - prev, final, slot)
    prev = s
    if final:
      break
    if pending is not None:  # the previous check's count, read after this interval is enqueued
      left = r.count(pending)
      if left == 0:
        break
      pending = slot
      if left <= compact_below * r.rows:
        before = r.rows
        left = r.compact()
        if left == 0:
          break
        if left < before:
          compactions.append((s, before, left))
          pending = None  # this check's count is known: it is r.rows
    else:
      pending = slot
  r.sync()
  st = r.stream
  fields = {k: r.cap[k].download(stream=st) for k in r.capture_names}
  return SteadyResult(r.status.download(stream=st), r.step_out.download(stream=st),
                      r.drift.download(stream=st), fields, compactions, member_steps, r.ens.dt,
                      check_every)
