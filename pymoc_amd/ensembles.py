"""Batched drivers: the coupled time loops of the reference's example scripts, run for a
whole parameter-sweep ensemble with all state resident in HBM.

The reference has no driver class: the loops live in examples/*.py.  The
classes here reproduce those loops' order of operations and cadence exactly:
  JN2018Ensemble           examples/run_JansenNadeau_2018.py:201-261 (config 5)
  TwoBasinEnsemble         examples/twobasin_NadeauJansen.py:99-122
  TwoBasinSweep            the same loop with per-member cfg reading, steady runs, forcing
                           schedules and an implicit column step
  ColumnThermwindEnsemble  examples/example_timestepping.py:73-80   (BASELINE config 1)
  EquiIterationEnsemble    examples/example_iteration.py:59-68      
  TwoColEnsemble           examples/example_twocol.py:85-96         (config 3)
                           examples/example_twocol_plusSO.py:99-115 (config 4, with_so)
Each member is independent; `cfg` is a dict from `pymoc_amd.configs`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .columns import ColumnBatch, _HINT_DIV3_OFF, check_scheme, div3_licensed
from .device import DeviceArray, Event, Graph, Stream, _sh, launch_span
from .equilibrium import ColumnEquiBatch
from .noise import application as noise_application
from .psi_so import PsiSOBatch
from .sharding import DiagnosticGather, member_range
from .so_ml import SOMLBatch
from .thermwind import ThermwindBatch

_TW_ALL = _lib.PM_TW_SOLVE | _lib.PM_TW_PSIB | _lib.PM_TW_PSIBZ


def _rows(v, n, nz):
  a = np.asarray(v, dtype=np.float64)
  if a.ndim == 0:
    return np.full((n, nz), a)
  if a.ndim == 1 and a.shape[0] == n and n != nz:
    return np.repeat(a[:, None], nz, axis=1)
  if a.ndim == 1:
    return np.broadcast_to(a, (n, nz)).copy()
  return a


def _run_fits(kind, nz, nb, ny):
  """Do the phases of a persistent run kernel (kind 0: pm_twocol_run, 1: pm_jn2018_run) fit the
  160 KB of LDS of a CU at 16 members per block?"""
  nbytes = C.c_size_t(0)
  check(lib.pm_run_lds_bytes(int(kind), int(nz), int(nb), int(ny), C.byref(nbytes)))
  return 0 < nbytes.value <= 160 * 1024


def _vec(v, n):
  a = np.asarray(v, dtype=np.float64)
  return np.full(n, a) if a.ndim == 0 else a


class ColumnThermwindEnsemble(object):
  """One column per member, thermal wind against b2 = 0 re-solved after EVERY step and
  applied in z-space: wA = Psi * 1e6 (example_timestepping.py:73-80).

  Every model step is two launches (the column step, the thermal-wind solve), so a small
  ensemble is bound by the host's launch rate: `use_graph` (default) captures GRAPH_STEPS steps
  once into a hipGraph and replays it -- one host call per GRAPH_STEPS model steps; the kernels
  and their order are the same, so are the results."""
  GRAPH_STEPS = 32

  def __init__(self, cfg, n=None, stream=None, lanes_per_col=0, use_graph=True):
    z = cfg['z']
    nz = z.size
    b0 = np.atleast_2d(cfg['b0'])
    n = b0.shape[0] if n is None else n
    self.n, self.nz, self.dt = n, nz, float(cfg['dt'])
    self.lanes, self.stream = lanes_per_col, stream
    self.cols = ColumnBatch(z, _rows(cfg['kappa'], n, nz), _rows(cfg['Area'], n, nz),
                            _rows(b0, n, nz), bs=_vec(cfg['bs'], n), bbot=_vec(cfg['bbot'], n),
                            stream=stream)
    self.tw = ThermwindBatch(z, n, f=cfg['f'], nb=1, stream=stream, z_dev=self.cols.z)
    self.b2 = DeviceArray.zeros((n, nz), stream=stream)
    self.wA = DeviceArray.zeros((n, nz), stream=stream)
    self._use_graph, self._graph = bool(use_graph), None
    self._solve()

  def _solve(self):
    self.tw.update(self.cols.b, self.b2, ops=_lib.PM_TW_SOLVE | _lib.PM_TW_WA_PSI,
                   wA1=self.wA, nb=1)

  def _step(self):
    self.cols.steps(self.wA, self.dt, 1, lanes_per_col=self.lanes)
    self._solve()

  def run(self, nsteps):
    remaining = int(nsteps)
    while self._use_graph and remaining >= self.GRAPH_STEPS:
      if self._graph is None:
        with Graph.capture(self.stream) as cap:
          for _ in range(self.GRAPH_STEPS):
            self._step()
        self._graph = cap.graph
      self._graph.launch(self.stream)
      remaining -= self.GRAPH_STEPS
    for _ in range(remaining):
      self._step()

  def state(self):
    return dict(b=self.cols.get_b(), Psi=self.tw.Psi.download(stream=self.stream))


class EquiIterationEnsemble(object):
  """One basin column per member: its equilibrium profile for the current overturning
  (`Column.solve_equi`) and the thermal-wind overturning against b_N = 0 for the relaxed
  profile, iterated (example_iteration.py:59-68):
      wA = AMOC.Psi*1e6;  basin.solve_equi(wA);
      AMOC.update(b1 = keep*AMOC.b1(z) + relax*basin.b);  AMOC.solve()"""

  def __init__(self, cfg, stream=None):
    z = cfg['z']
    nz = z.size
    b0 = np.atleast_2d(cfg['b_basin0'])
    self.n, self.nz = n, _ = b0.shape[0], nz
    self.keep, self.relax = float(cfg['keep']), float(cfg['relax'])
    self.stream = stream
    self.tw = ThermwindBatch(z, n, f=cfg['f'], nb=1, stream=stream)
    self.b1 = DeviceArray.from_host(_rows(b0, n, nz), stream=stream)
    self.b2 = DeviceArray.zeros((n, nz), stream=stream)
    self.wA = DeviceArray.zeros((n, nz), stream=stream)
    self.eq = ColumnEquiBatch.from_profiles(
        z, _rows(cfg['kappa'], n, nz), _rows(cfg['A_basin'], n, nz), _vec(cfg['bs'], n),
        _vec(cfg['bbot'], n), n=n, stream=stream, z_dev=self.tw.z)
    self._solve()

  def _solve(self):
    self.tw.update(self.b1, self.b2, ops=_lib.PM_TW_SOLVE | _lib.PM_TW_WA_PSI, wA1=self.wA,
                   nb=1)

  def iterate(self, niter=1):
    for _ in range(int(niter)):
      self.eq.solve(self.wA)
      check(lib.pm_axpby(self.n * self.nz, self.keep, self.b1.ptr, self.relax, self.eq.b.ptr,
                         self.b1.ptr, _sh(self.stream)))
      self._solve()

  def state(self):
    return dict(b=self.eq.get_b(), bz=self.eq.get_bz(), b1=self.b1.download(stream=self.stream),
                Psi=self.tw.Psi.download(stream=self.stream))


class CoupledEnsemble(object):
  """What TwoColEnsemble, JN2018Ensemble and TwoBasinEnsemble share: the diagnostic gather, the
  downloads of `state()`, two launches side by side, the cadence of the loop, how a per-member
  `cfg` key is read, and the restart protocol `run_to_steady` drives.

  A driver's columns are stacked in NGROUPS groups of n rows (`cols.b`, `wA`); its constructor
  makes the views of those groups once (`b_basin`, `wA_north`, ...: DeviceArray.view) and every
  launch, gather and check takes them from there.

  MEMBER_KEYS is the single statement of how a per-member `cfg` key is read -- by the
  constructor (`read`), by a restriction to some members (`restrict`) and by the tests:
    ("vec",)       a scalar is shared; an array has the member axis first ((n,) or (n, ...))
    ("rows", axis) a profile on cfg[axis]: 2-D is per member; 1-D of length n is one value per
                   member, repeated along the axis -- unless n equals the axis length, when it is
                   the shared profile; a scalar or any other 1-D array is shared
    ("2d", axis)   a profile on cfg[axis]: 2-D is per member, anything else is shared
  None: the driver's constructor reads its cfg by itself and cannot be restarted on a subset.

  FORCING_TARGETS is the single statement of what a `forcing=ForcingSchedule(...)` may set:
    name -> a tuple of destinations, each (the device array, as an attribute path from the
            driver; the group of n rows its first row starts; the row length: None = one value per
            member, "y" = a profile on cfg['y'], "tau" = whichever of the two the batch's tau is).
            A value the driver keeps in more than one place has one destination for each (all of
            one row length); the schedule's values are uploaded once per name.
  None: the driver takes no schedule."""

  NGROUPS = 2
  FIELDS = ("b_basin", "b_north", "Psi", "Psi_SO")
  MEMBER_KEYS = None
  FORCING_TARGETS = None
  RESTART_PHASE = None  # the steps s = RESTART_PHASE (mod MOC_up_iters) can be restarted from
  # optional indices.IndexRecorder (it attaches itself): sampled at the `_gather_if_due` sites,
  # right after the overturning update at that step; None: no launch is added anywhere
  indices = None
  _noise = None  # the BoundNoise of `noise=`, where a driver takes one

  @classmethod
  def members(cls, cfg):
    return np.atleast_2d(cfg['b_basin0']).shape[0]

  @classmethod
  def _rule(cls, cfg, key, n):
    """(the value as float64, the length of its rows or None, is its first axis the members?)"""
    rule = cls.MEMBER_KEYS[key]
    a = np.asarray(cfg[key], dtype=np.float64)
    if rule[0] == "vec":
      return a, None, a.ndim >= 1
    nlev = np.asarray(cfg[rule[1]]).size
    return a, nlev, a.ndim == 2 or (rule[0] == "rows" and a.ndim == 1 and a.shape[0] == n and
                                    n != nlev)

  @classmethod
  def read(cls, cfg, key, n):
    """cfg[key] of an n-member cfg as an explicit [n, ...] array, by the key's rule."""
    a, nlev, per_member = cls._rule(cfg, key, n)
    if nlev is None:
      return a if per_member else np.full(n, a)
    if per_member:
      return a if a.ndim == 2 else np.repeat(a[:, None], nlev, axis=1)
    return np.broadcast_to(a, (n, nlev)).copy()

  @classmethod
  def restrict(cls, cfg, keep):
    """`cfg` restricted to members `keep` (indices into its current members): a per-member key is
    expanded to explicit [n, ...] at the current n, then indexed -- so a 1-D per-member array never
    comes back as a length-nz vector that would be read as a profile.  Shared keys, and keys the
    constructor does not read per member, are passed on unchanged."""
    n = cls.members(cfg)
    keep = np.asarray(keep, dtype=np.int64)
    out = dict(cfg)
    for key in cls.MEMBER_KEYS:
      if key in cfg and cls._rule(cfg, key, n)[2]:
        out[key] = cls.read(cfg, key, n)[keep]
    return out

  @classmethod
  def _has_channel(cls, cfg):
    return 'y' in cfg

  @classmethod
  def forcing_lengths(cls, cfg, n):
    """name -> row length of the targets a schedule may name for this cfg (host only)."""
    out = {}
    for name, dests in cls.FORCING_TARGETS.items():
      axis = dests[0][2]  # (one row length per name)
      if axis is None:
        out[name] = 1
      elif cls._has_channel(cfg):
        profile = axis == "y" or cls.read(cfg, 'tau', n).ndim == 2
        out[name] = np.asarray(cfg['y']).size if profile else 1
    return out

  def _check_forcing(self, forcing, cfg, n, noise=None, comm=None, n_total=None, **excluded):
    """A constructor's first act, before any device state: refuse what a schedule or a
    NoiseForcing cannot go with, and their names and shapes against this cfg.  `comm`, `n_total`:
    the shard this rank holds -- the noise counts members by their global index."""
    self._forcing, self._forced_at = None, -1
    self._noise, self._noise_spec = None, noise
    for what, given in (("forcing", forcing), ("noise", noise)):
      if given is None:
        continue
      for kw, on in excluded.items():
        if on:
          raise ValueError("%s does not go with %s=True: a captured or persistent launch "
                           "spans the steps the schedule is applied at" % (what, kw))
      given.check(self.forcing_lengths(cfg, n), n)
    self._member0 = 0
    if noise is not None and comm is not None:
      self._member0 = member_range(n if n_total is None else n_total, comm.world, comm.rank)[0]

  @property
  def noise(self):
    """The BoundNoise of `noise=NoiseForcing(...)` (its get_state / set_state carry the noise
    states across runs); None without one."""
    return self._noise

  def _bind_forcing(self, forcing, cfg):
    """A constructor's last act ahead of its own first update (which uses the cfg's values)."""
    n, lengths = self.n, self.forcing_lengths(cfg, self.n)

    def destinations(names):
      targets = {}
      for name in names:
        targets[name] = []
        for path, group, _ in self.FORCING_TARGETS[name]:
          a = self
          for attr in path.split("."):
            a = getattr(a, attr)
          targets[name].append((a, group * n, lengths[name]))
      return targets

    noise = self._noise_spec
    if noise is not None:
      # the noise keeps a copy of the cfg's values as its base and writes every real destination;
      # a schedule on the same target writes that base instead (once, whatever the destinations)
      self._noise = noise.bind(n, destinations(noise.targets), member0=self._member0,
                               stream=self.stream)
      # a Gaussian deviate has no bound: the columns test every bs operand (bit-identical
      # results), as under a schedule with knots outside the window below
      if "bs" in noise.targets or "bs_north" in noise.targets:
        self.cols._par_ok["bs"] = np.zeros(self.cols.ncols, dtype=bool)
        self.cols._upload_flags()
    if forcing is None:
      return
    targets = destinations(forcing.values)
    if self._noise is not None:
      for name in targets:
        if name in self._noise.base:
          targets[name] = [(self._noise.base[name], 0, lengths[name])]
    self._forcing = forcing.bind(n, targets, stream=self.stream)
    # PM_COL_STATIC_IN_RANGE was derived from the cfg's bs; it stays only where every value the
    # schedule can write is zero or inside the exact-division window [2^-200, 2^200]: knots that
    # are zero or within [2^-100, 2^100] guarantee that (an interpolated value is a rounded sum of
    # terms no smaller than 2^-153 next to such knots).  Otherwise the columns test every operand
    # (bit-identical results, include/pymoc_hip.h).
    bs = [np.abs(forcing.values[k]) for k in ("bs", "bs_north") if k in forcing.values]
    if any(not ((v == 0) | ((v >= 2.0**-100) & (v <= 2.0**100))).all() for v in bs):
      self.cols._par_ok["bs"] = np.zeros(self.cols.ncols, dtype=bool)
      self.cols._upload_flags()

  def _apply_forcing(self):
    """THE rule of when a schedule is evaluated: at the top of loop iteration s = self.ii, before
    anything else that iteration does, for s = 0 and every s = RESTART_PHASE (mod MOC_up_iters),
    at t = s * dt; the values are held until the next such iteration.  Those are exactly the first
    steps of the launch intervals, so the forcing is constant within a launch, and it is where a
    reference user loop that assigns at the top of the loop body puts it: ahead of the MOC update
    of iteration s for JN2018Ensemble, behind the update that follows step s - 1 for
    TwoColEnsemble."""
    if (self._forcing is None and self._noise is None) or self._forced_at == self.ii:
      return
    s = self.ii
    if s == 0 or s % self.M == self.RESTART_PHASE % self.M:
      if self._forcing is not None:
        with launch_span(self.timer, "k_forcing_apply", self.stream):
          self._forcing.apply(s * self.dt, self.stream)
      if self._noise is not None:
        # right behind the schedule's launch, which wrote the base of the targets they share
        j, elapsed = noise_application(s, self.M, self.RESTART_PHASE, self.dt)
        with launch_span(self.timer, "k_forcing_noise", self.stream):
          self._noise.apply(j, elapsed, self.stream)
      self._forced_at = s

  @staticmethod
  def _check_arith(arith):
    if arith not in ("exact", "contracted"):
      raise ValueError("arith must be 'exact' or 'contracted'")
    return arith

  def _init_gather(self, comm, n_total, keep_history, gather, gather_overlap):
    self.diag = None
    if comm is not None or keep_history:
      self.diag = DiagnosticGather(comm, self.n, self.n if n_total is None else n_total,
                                   [(k, self.nz) for k in self.FIELDS], stream=self.stream,
                                   keep_history=keep_history, mode=gather, overlap=gather_overlap)

  def fields(self):
    """name -> DeviceArray of the entries of FIELDS (the two-column layout; without an SO channel
    Psi_SO is a zero array)."""
    return dict(b_basin=self.b_basin, b_north=self.b_north, Psi=self.tw.Psi,
                Psi_SO=self.so.Psi if self.so is not None else self._zero_so)

  def gather_diagnostics(self, step=None):
    """Gather FIELDS of every rank's members (device buffers, one collective);
    `self.diag.last()` returns the assembled host arrays."""
    self.diag.gather(self.fields(), step=self.ii if step is None else step)

  def _gather_if_due(self, step):
    if self.indices is not None:
      self.indices.maybe_sample(step)
    if self.diag is not None and self.diag.due(step, self.diag_iters):
      self.gather_diagnostics(step)

  def _no_indices_in_fused_run(self):
    if self.indices is not None:
      raise ValueError("an IndexRecorder does not go with fused_run=True: a persistent launch "
                       "spans the steps the samples are taken at")

  def nonfinite_members(self):
    nf = self.cols.get_nonfinite().reshape(self.NGROUPS, self.n)
    return np.nonzero(np.bitwise_or.reduce(nf, axis=0))[0]

  def _download(self, **arrays):
    return {k: a.download(stream=self.stream) for k, a in arrays.items()}

  def _side_by_side(self, side_fn, main_fn):
    """side_fn(self._side) beside main_fn(self.stream): the side stream starts behind what
    self.stream holds so far, and self.stream goes on only when both are done."""
    self._ev_fork.record(self.stream)
    self._side.wait(self._ev_fork)
    side_fn(self._side)
    self._ev_join.record(self._side)
    main_fn(self.stream)
    check(lib.pm_stream_wait_event(_sh(self.stream), self._ev_join.handle))

  def _interval(self, remaining):
    """The steps up to and including the next one an update follows (ii % M == 0), at most
    `remaining`: they share one forcing, so they are one launch."""
    nxt = self.ii if self.ii % self.M == 0 else (self.ii // self.M + 1) * self.M
    return min(nxt - self.ii + 1, remaining)

  def drift_fields(self):
    """[(name, DeviceArray, row stride, len)] of the prognostic state: what drifts, and what a
    restart carries over as the cfg's initial profiles `<name>0`."""
    nz = self.nz
    return [("b_basin", self.b_basin, nz, nz), ("b_north", self.b_north, nz, nz)]

  def capture_fields(self):
    """The drift fields, then the overturnings of the update at the restart point."""
    nz = self.nz
    f = self.drift_fields() + [("Psi", self.tw.Psi, nz, nz)]
    return f + [("Psi_SO", self.so.Psi, nz, nz)] if self.so is not None else f

  def at_restart_point(self):
    """Bring the diagnostics to the state a restart at this step (= RESTART_PHASE mod M) has."""

  def subset(self, keep, cfg, kw):
    """A new ensemble of this class from members `keep` of this one (built from `cfg`, **kw) at
    the same step, at a restart point: it continues bit-identically to these members here."""
    keep = np.asarray(keep, dtype=np.int64)
    cfg = self.restrict(cfg, keep)
    for name, a, _, _ in self.drift_fields():
      cfg[name + "0"] = a.download(stream=self.stream)[keep]
    new = type(self)(cfg, **kw)
    new.ii = self.ii
    new.at_restart_point()
    return new


class TwoColEnsemble(CoupledEnsemble):
  """Basin + northern sinking column per member, coupled by the thermal-wind overturning
  mapped to isopycnal space every MOC_up_iters steps."""

  # every key is read through `read`; tau / KGM go on to PsiSOBatch, which reads a 1-D array of
  # length n as one value per member and a 2-D one as profiles on y: the "vec" rule
  MEMBER_KEYS = dict(kappa=("rows", "z"), A_basin=("rows", "z"), A_north=("rows", "z"),
                     bs=("vec",), bs_north=("vec",), bbot=("vec",), tau=("vec",), KGM=("vec",),
                     bs_SO=("rows", "y"), b_basin0=("rows", "z"), b_north0=("rows", "z"))
  # after the update that follows step s - 1 (example_twocol.py:85-96): the constructor's own
  # update is the one at a restart
  RESTART_PHASE = 1
  FORCING_TARGETS = dict(bs=(("cols.bs", 0, None),), bs_north=(("cols.bs", 1, None),),
                         tau=(("so.tau", 0, "tau"),), bs_SO=(("bs_SO", 0, "y"),))

  @classmethod
  def _has_channel(cls, cfg):
    return 'y' in cfg and 'bs_SO' in cfg

  def __init__(self, cfg, stream=None, lanes_per_col=0, comm=None, n_total=None,
               diag_iters=None, keep_history=False, arith="exact", overlap_updates=False,
               fused_run=None, gather="all", gather_overlap=True, forcing=None,
               scheme="explicit", noise=None):
    """`scheme="implicit"`: the columns step with backward Euler (ColumnBatch.steps(scheme=
    "implicit"), pm_column_steps_implicit) -- stable at any dt, an extension with no reference
    counterpart (a tolerance path); the forcing reaches them as an array (the thermal wind's wA
    outputs or pm_twocol_forcing, as for launches of 1-2 steps), everything else is unchanged.
    Not with fused_run, arith="contracted" or a non-zero lanes_per_col (ValueError: the implicit
    kernel always gives a column one wavefront).  Works with `forcing=` and under
    run_to_steady.  (This driver captures no hipGraph -- it has no `use_graph` -- so there is
    nothing to capture or refuse.)
    `fused_run`: carry the members through whole stretches of the loop -- many [refresh the
    overturning, MOC_up_iters steps] intervals -- in ONE launch of the persistent per-member
    kernel (pm_twocol_run), ending a launch only where the diagnostics are gathered.  Same device
    functions as the launch sequence, bit-identical results; needs: no SO channel, exact
    arithmetic, Area constant in z, the phases' LDS within 160 KB.  None = off (measured slower
    than the launch sequence on config 3: DESIGN.md section 6).
    `overlap_updates=True`: with an SO channel, Psi_SO.solve and the thermal wind of an update run
    side by side on two streams (bit-identical results; see `_update`).  Round 3's default; since
    the round-5 thermal wind (37 us beside a Psi_SO.solve of 113) the fork / join events cost what
    the overlap gives: config 4 203-204 us per interval side by side, 194-204 one after the other
    (profiles/r05/c4_modes.log).
    `comm` (a pymoc_amd.sharding communicator) makes this rank's members one shard of an
    `n_total`-member ensemble: stepping is unchanged (members never interact) and
    {b_basin, b_north, Psi, Psi_SO} are all-gathered on device buffers every `diag_iters`
    steps (default cfg['Diag_iters']) and by `gather_diagnostics()` at the end of a run;
    `gather="root"` sends them to rank 0 only, `gather_overlap` runs the exchange on a
    communication stream of its own beside the stepping (sharding.DiagnosticGather).
    `arith="contracted"`: the columns step in the opt-in tolerance mode (ColumnBatch.steps).
    `forcing`: a ForcingSchedule for bs, bs_north and, with an SO channel, tau (in the form of the
    batch's tau: one value per member or a profile on y) and bs_SO, applied by the rule of
    `_apply_forcing`; the constructor's own update uses the cfg's values.  Not with fused_run.
    `noise`: a NoiseForcing on the same targets, applied at the same instants right behind the
    schedule (pymoc_amd.noise); with `comm`, members are counted by their global index.  Not with
    fused_run."""
    z = cfg['z']
    nz = z.size
    n = self.members(cfg)
    self._check_forcing(forcing, cfg, n, noise=noise, comm=comm, n_total=n_total,
                        fused_run=fused_run)
    check_scheme(scheme, arith=arith, lanes_per_col=lanes_per_col)
    if scheme == "implicit" and fused_run:
      raise ValueError("scheme='implicit' excludes fused_run")
    self.scheme = scheme
    rd = lambda key: self.read(cfg, key, n)  # noqa: E731
    self.n, self.nz = n, nz
    self.dt, self.M, self.nb = float(cfg['dt']), int(cfg['MOC_up_iters']), int(cfg['nb'])
    self.lanes, self.arith, self.stream = lanes_per_col, arith, stream
    self.diag_iters = cfg.get('Diag_iters') if diag_iters is None else diag_iters
    self.timer = None  # optional device.LaunchTimer: events around every launch of run()
    self._init_gather(comm, n_total, keep_history, gather, gather_overlap)
    kap = rd('kappa')
    # rows [0, n): basin columns, rows [n, 2n): northern columns
    self.cols = ColumnBatch(
        z, np.concatenate([kap, kap]), np.concatenate([rd('A_basin'), rd('A_north')]),
        np.concatenate([rd('b_basin0'), rd('b_north0')]),
        bs=np.concatenate([rd('bs'), rd('bs_north')]), bbot=np.tile(rd('bbot'), 2),
        do_conv=np.concatenate([np.zeros(n, bool), np.ones(n, bool)]), stream=stream)
    self.tw = ThermwindBatch(z, n, f=cfg['f'], nb=self.nb, stream=stream, z_dev=self.cols.z)
    self.wA = DeviceArray.zeros((2 * n, nz), stream=stream)
    self.b_basin, self.b_north = self.cols.b.view(0, n), self.cols.b.view(n, n)
    self.wA_basin, self.wA_north = self.wA.view(0, n), self.wA.view(n, n)
    self.ii = 0
    self.so = None
    if 'y' in cfg and 'bs_SO' in cfg:  # example_twocol_plusSO.py:69-81
      self.so = PsiSOBatch(z, cfg['y'], n, tau=rd('tau'), KGM=rd('KGM'), f=cfg['f'],
                           L=cfg['L'], c=cfg.get('c'), bvp_with_Ek=cfg.get('bvp_with_Ek', False),
                           bvp_refine=cfg.get('bvp_refine', 0), stream=stream,
                           z_dev=self.cols.z)
      self.bs_SO = DeviceArray.from_host(rd('bs_SO'), stream=stream)
    self._zero_so = (DeviceArray.zeros((n, nz), stream=stream)
                     if self.so is None and self.diag is not None else None)
    self._overlap = self.so is not None and bool(overlap_updates)
    if self._overlap:
      self._side, self._ev_fork, self._ev_join = Stream(), Event(), Event()
    can_fuse = (self.so is None and arith == "exact" and self.cols.uniform_area and
                not self.cols.has_bzbot and _run_fits(0, nz, self.nb, 0))
    if fused_run and not can_fuse:
      raise ValueError("fused_run needs: no SO channel, exact arithmetic, Area constant in z, no "
                       "bzbot, 4 <= nz <= 256 and the phases' LDS within 160 KB")
    self._fused_run = False if fused_run is None else bool(fused_run)
    self.run_status = (DeviceArray.zeros((n,), np.int32, stream=stream) if self._fused_run
                       else None)
    self._bind_forcing(forcing, cfg)
    self._update()  # AMOC.solve(); AMOC.Psibz() [; SO.solve()] on the initial profiles

  def _solve_so(self, stream):
    self.so.stream = stream
    with launch_span(self.timer, "k_psi_so", stream):
      self.so.update(self.b_basin, self.bs_SO)
    self.so.stream = self.stream

  def _update(self):
    # SO.solve() and AMOC.solve() both read basin.b only.  With the SO channel the two launches
    # run SIDE BY SIDE on two streams (each leaves the machine partly idle: together 174 us
    # instead of 200 us per update of 8192 members) and the columns form
    # wAb = (Psi_iso_b - SO.Psi)*1e6, wAN = -Psi_iso_n*1e6 themselves (PM_OP_WA_PSI) once both
    # are done -- the same operations as the thermal-wind launch's wA1 / wA2 epilogue.
    if self.so is not None and self._overlap:
      def thermwind(stream):
        with launch_span(self.timer, "k_thermwind", stream):
          self.tw.update(self.b_basin, self.b_north, ops=_TW_ALL, store_psib=False)
      self._side_by_side(self._solve_so, thermwind)
      return
    if self.so is not None:
      self._solve_so(self.stream)
    with launch_span(self.timer, "k_thermwind", self.stream):
      self.tw.update(self.b_basin, self.b_north, ops=_TW_ALL, store_psib=False,
                     Psi_SO=self.so.Psi if self.so is not None else None,
                     wA1=self.wA_basin, wA2=self.wA_north)

  def _steps(self, n):
    name = ("k_column_implicit" if self.scheme == "implicit" else
            "k_column_steps" if n >= 3 else "k_column_steps_short")
    with launch_span(self.timer, name, self.stream):
      self._steps_launch(n)

  def _steps_launch(self, n):
    implicit = self.scheme == "implicit"
    if self.so is not None and self._overlap and n >= 3 and not implicit:
      self.cols.steps(None, self.dt, n, lanes_per_col=self.lanes, arith=self.arith,
                      psi_forcing=(self.tw.psibz, self.so.Psi))
      return
    # a launch of 1-2 steps, or the implicit scheme: the forcing as an array
    if self.so is not None and self._overlap:
      check(lib.pm_twocol_forcing(self.n, self.nz, self.tw.psibz.ptr, self.so.Psi.ptr,
                                  self.wA.ptr, _sh(self.stream)))
    if implicit:
      self.cols.steps(self.wA, self.dt, n, scheme="implicit")
      return
    self.cols.steps(self.wA, self.dt, n, lanes_per_col=self.lanes, arith=self.arith)

  def _run_fused(self, nsteps):
    """The same loop through pm_twocol_run: one launch per stretch that ends at a diagnostic
    gather (or at the end of the run)."""
    self._no_indices_in_fused_run()
    M, remaining = self.M, int(nsteps)
    while remaining > 0:
      ii = self.ii
      k0 = ii if ii % M == 0 else (ii // M + 1) * M  # the next step followed by an update
      last = ii + remaining - 1                       # last step of this run
      sch = _lib.pm_run_schedule()
      sch.m_steps = M
      gather_at = None
      if k0 > last:
        sch.n_first, sch.n_updates, sch.n_last = remaining, 0, 0
        end = last + 1
      else:
        sch.n_first = k0 - ii + 1
        nu, k = 0, k0
        while True:
          nu += 1
          if self.diag is not None and self.diag.due(k, self.diag_iters):
            gather_at, tail = k, 0
            break
          if k + M > last:  # no further update inside this run
            tail = last - k
            break
          k += M
        sch.n_updates = nu
        sch.n_last = tail
        end = k + 1 + sch.n_last
      d = _lib.pm_twocol_loop()
      d.cols = self.cols.descriptor()
      d.tw = self.tw.descriptor(self.b_basin, self.b_north, wA1=self.wA_basin,
                                wA2=self.wA_north, store_psib=False)
      d.wA, d.dt, d.sched, d.status = self.wA.ptr, self.dt, sch, self.run_status.ptr
      with launch_span(self.timer, "k_twocol_run", self.stream):
        check(lib.pm_twocol_run(C.byref(d), _sh(self.stream)))
      remaining -= end - ii
      self.ii = end
      if gather_at is not None:
        self.gather_diagnostics(gather_at)

  def run(self, nsteps):
    """`for ii in range(nsteps): step both columns; if ii % MOC_up_iters == 0: update`,
    with the steps between two updates fused into one launch (wA is constant there)."""
    if self._fused_run:
      return self._run_fused(nsteps)
    remaining = int(nsteps)
    while remaining > 0:
      self._apply_forcing()
      n = self._interval(remaining)
      self._steps(n)
      self.ii += n
      remaining -= n
      if (self.ii - 1) % self.M == 0:
        self._update()
        self._gather_if_due(self.ii - 1)

  def state(self):
    out = self._download(b_basin=self.b_basin, b_north=self.b_north, Psi=self.tw.Psi,
                         Psi_iso_b=self.tw.psibz1, Psi_iso_n=self.tw.psibz2)
    if self.so is not None:
      out.update(self._download(Psi_SO=self.so.Psi, Psi_Ek=self.so.Psi_Ek,
                                Psi_GM=self.so.Psi_GM))
    return out


class JN2018Ensemble(CoupledEnsemble):
  """run_JansenNadeau_2018.py with default flags: basin + north columns, thermal wind,
  SO channel overturning (no BVP smoother) and the SO mixed layer, with the script's
  per-step bottom-BC / bottom-boundary-layer diffusivity switching.

  Per step: BC switch -> both columns (convective adjustment on) -> mixed layer; every
  MOC_up_iters steps (before the step) the three diagnostics are refreshed.  With
  `use_graph` a whole MOC block is captured once into a hipGraph and replayed."""

  # every key is read through `read`; tau / KGM go on to PsiSOBatch ("vec": as for
  # TwoColEnsemble) and surflux / rest_mask / b_rest to SOMLBatch, which reads a 1-D array as the
  # shared profile on y whatever its length: the "2d" rule, as np.broadcast_to does for the
  # diffusivity profiles
  MEMBER_KEYS = dict(kappa=("2d", "z"), kappaeff=("2d", "z"), A_basin=("rows", "z"),
                     A_north=("rows", "z"), bs=("vec",), bs_north=("vec",), tau=("vec",),
                     KGM=("vec",), surflux=("2d", "y"), rest_mask=("2d", "y"),
                     b_rest=("2d", "y"), b_basin0=("rows", "z"), b_north0=("rows", "z"),
                     bs_SO0=("rows", "y"))
  # after step s's MOC update, before the step (run_JansenNadeau_2018.py:204-217)
  RESTART_PHASE = 0
  FORCING_TARGETS = dict(bs=(("cols.bs", 0, None),), bs_north=(("cols.bs", 1, None),),
                         tau=(("so.tau", 0, "tau"),), b_rest=(("ml.b_rest", 0, "y"),),
                         surflux=(("ml.surflux", 0, "y"),))

  def __init__(self, cfg, stream=None, lanes_per_col=0, use_graph=False, fused=None,
               comm=None, n_total=None, diag_iters=None, keep_history=False, arith="exact",
               shared_coef=True, fused_run=None, gather="all", gather_overlap=True,
               split_lanes=False, forcing=None, noise=None):
    """`fused_run`: whole stretches of the loop -- many [PsiSO.solve, AMOC.solve / Psibz,
    MOC_up_iters steps] intervals -- in ONE launch of the persistent per-member kernel
    (pm_jn2018_run), ending a launch only where diagnostics are sampled or gathered;
    bit-identical to the launch sequence; needs the fused step loop's conditions and the phases'
    LDS within 160 KB.  None = off (measured slower than the launch sequence: DESIGN.md section 6).
    `comm`, `n_total`, `diag_iters`, `gather`, `gather_overlap`: as for TwoColEnsemble; the gather happens where the
    script samples its diagnostics (`if ii % Diag_iters == 0`, right after the MOC update,
    run_JansenNadeau_2018.py:218-226; default Diag_iters = 10 MOC_up_iters, :99).
    `arith="contracted"`: the columns of the fused loop step in the opt-in tolerance mode
    (PM_JN_CONTRACTED; uniform-Area ensembles with ny <= 64 -- others stay exact).
    `shared_coef`: let the fused loop read ONE copy of kappa / d(A kappa)/dz / Area per column
    kind when all members' profiles are identical (checked here on the host arrays;
    PM_JN_SHARED_COEF); results are bit-identical either way.
    `split_lanes`: the fused loop steps both columns of a member together, one per half of the
    wavefront (PM_JN_SPLIT_LANES; bit-identical; measured a tie on config 5, hence opt-in).
    `forcing`: a ForcingSchedule for bs, bs_north, tau (in the form of the batch's tau), b_rest
    and surflux, applied by the rule of `_apply_forcing` -- ahead of the MOC update of the step,
    in run() on every path and in moc_update().  Not with use_graph or fused_run.
    `noise`: a NoiseForcing on the same targets, applied at the same instants right behind the
    schedule (pymoc_amd.noise).  Not with use_graph or fused_run: base + x * pattern replaces the
    cfg's values at every application even where sigma is zero, so no captured block is replayed
    while noise is attached."""
    self._check_forcing(forcing, cfg, self.members(cfg), noise=noise, comm=comm, n_total=n_total,
                        use_graph=use_graph, fused_run=fused_run)
    self.arith = self._check_arith(arith)
    self.shared_coef = bool(shared_coef)
    self.split_lanes = bool(split_lanes)
    z, y = cfg['z'], cfg['y']
    nz, ny = z.size, y.size
    n = self.members(cfg)
    rd = lambda key: self.read(cfg, key, n)  # noqa: E731
    self.n, self.nz, self.ny = n, nz, ny
    self.dt, self.M, self.nb = float(cfg['dt']), int(cfg['MOC_up_iters']), int(cfg['nb'])
    self.lanes, self.stream = lanes_per_col, stream
    bb0, bn0 = rd('b_basin0'), rd('b_north0')
    kap, kapeff = rd('kappa'), rd('kappaeff')
    # Column(kappa=kappaeff, bbot=b[0]) (:159-171); coefficient set 0 = kappa, 1 = kappaeff
    self.cols = ColumnBatch(
        z, np.concatenate([kap, kap]), np.concatenate([rd('A_basin'), rd('A_north')]),
        np.concatenate([bb0, bn0]), bs=np.concatenate([rd('bs'), rd('bs_north')]),
        bbot=np.concatenate([bb0[:, 0], bn0[:, 0]]), do_conv=True,
        kappa_alt=np.concatenate([kapeff, kapeff]), stream=stream)
    self.cols.set_ksel(np.ones(2 * n, dtype=np.int32))
    self.tw = ThermwindBatch(z, n, f=cfg['f'], nb=self.nb, stream=stream, z_dev=self.cols.z)
    self.so = PsiSOBatch(z, y, n, tau=rd('tau'), KGM=rd('KGM'), f=cfg['f'], L=cfg['L'],
                         stream=stream, z_dev=self.cols.z)
    self.ml = SOMLBatch(y, nz, rd('bs_SO0'), surflux=rd('surflux'), rest_mask=rd('rest_mask'),
                        b_rest=rd('b_rest'), Ks=cfg['Ks'], h=cfg['h'], L=cfg['L'],
                        v_pist=cfg['v_pist'], stream=stream)
    self.wA = DeviceArray.zeros((2 * n, nz), stream=stream)
    self.b_basin, self.b_north = self.cols.b.view(0, n), self.cols.b.view(n, n)
    self.wA_basin, self.wA_north = self.wA.view(0, n), self.wA.view(n, n)
    self._bc = _lib.pm_jn2018_bc()
    d = self._bc
    d.n, d.nz, d.ny, d.reserved = n, nz, ny, 0
    d.Psi_SO, d.Psi_res_b, d.Psi_res_n = self.so.Psi.ptr, self.tw.psibz1.ptr, self.tw.psibz2.ptr
    d.b_basin, d.b_north = self.b_basin.ptr, self.b_north.ptr
    d.bs_SO, d.bbot, d.ksel = self.ml.bs.ptr, self.cols.bbot.ptr, self.cols.ksel.ptr
    self.ii = 0
    self._graph = None
    self._use_graph = use_graph
    # fused: one launch per MOC block for the whole [BC switch, 2 columns, mixed layer] loop
    self._fused = (nz <= 256) if fused is None else bool(fused)
    self.recorder = None  # optional diagnostics.JN2018Diagnostics
    self.timer = None     # optional device.LaunchTimer
    can_fuse = (self._fused and self.cols.uniform_area and ny <= 64 and
                _run_fits(1, nz, self.nb, ny))
    if fused_run and not can_fuse:
      raise ValueError("fused_run needs the fused step loop (Area constant in z, ny <= 64, "
                       "4 <= nz <= 256) and the phases' LDS within 160 KB")
    self._fused_run = False if fused_run is None else bool(fused_run)
    self._updated_at = -1  # iteration whose MOC update has been done already (fused_run)
    # the two diagnostic launches of an update as one (pm_so_tw_update): scalar tau only? no --
    # any Psi_SO without the boundary-value smoother on nz <= 256
    self._one_update_launch = bool(cfg.get('one_update_launch', True)) and nz <= 256
    self.diag_iters = (cfg.get('Diag_iters', 10 * self.M) if diag_iters is None
                       else diag_iters)
    self._init_gather(comm, n_total, keep_history, gather, gather_overlap)
    self._bind_forcing(forcing, cfg)

  def _after_update(self):
    if self.recorder is not None:
      self.recorder.maybe_record(self.ii)
    self._gather_if_due(self.ii)

  def _update(self):
    # psib / bgrid go to HBM only in the updates a diagnostics recorder samples right after (every
    # Diag_iters steps, run_JansenNadeau_2018.py:218-226); all the other updates sum only the
    # classes Psibz reads (thermwind.hip.h)
    rec = self.recorder
    store = rec is not None and self.ii % rec.Diag_iters == 0
    if self._one_update_launch:
      # PsiSO.solve + AMOC.solve / Psibz of a member by one wave, ONE launch (pm_so_tw_update)
      ds = self.so.descriptor(self.b_basin, self.ml.bs)
      dw = self.tw.descriptor(self.b_basin, self.b_north, Psi_SO=self.so.Psi, wA1=self.wA_basin,
                              wA2=self.wA_north, store_psib=store)
      with launch_span(self.timer, "k_so_tw_update", self.stream):
        check(lib.pm_so_tw_update(C.byref(ds), C.byref(dw), _TW_ALL, _sh(self.stream)))
      return
    with launch_span(self.timer, "k_psi_so", self.stream):
      self.so.update(self.b_basin, self.ml.bs)
    with launch_span(self.timer, "k_thermwind", self.stream):
      self.tw.update(self.b_basin, self.b_north, ops=_TW_ALL, store_psib=store,
                     Psi_SO=self.so.Psi, wA1=self.wA_basin, wA2=self.wA_north)

  def _step(self):
    check(lib.pm_jn2018_bc_switch(C.byref(self._bc), _sh(self.stream)))
    self.cols.steps(self.wA, self.dt, 1, lanes_per_col=self.lanes)
    self.ml.step(self.b_basin, self.so.Psi, self.dt)

  def _block(self):
    self._update()
    for _ in range(self.M):
      self._step()

  def _fused_steps(self, nsteps):
    d = self._jn_descriptor()
    with launch_span(self.timer, "k_jn2018_steps", self.stream):
      check(lib.pm_jn2018_steps(C.byref(d), self.dt, int(nsteps), _sh(self.stream)))

  def _div3(self):
    """PM_JN_DIV3_PROVEN: the columns' static denominators (ColumnBatch.div3_proven) and the
    mixed layer's h, L and y[1] - y[0] admit the 3-instruction exact quotient.  Decided per
    descriptor from the columns' present state -- `cols.set_static` re-derives their proof and
    `cols.use_hints(div3=False)` withdraws it -- only the mixed layer's part is kept, for as long
    as its three denominators stay what they were."""
    t = self.ml
    den = (float(t.h), float(t.L), float(t.y_host[1] - t.y_host[0]))
    if getattr(self, "_ml_div3", (None, False))[0] != den:
      a = np.abs(np.array(den, dtype=np.float64))
      self._ml_div3 = (den, bool(((a >= 2.0**-200) & (a <= 2.0**200)).all() and
                                 div3_licensed(np.array(den, dtype=np.float64))))
    c = self.cols
    return bool(c.uniform_area and c.div3_proven and
                not (c.__dict__.get("_hints_off", 0) & _HINT_DIV3_OFF) and self._ml_div3[1])

  def _jn_descriptor(self):
    d = _lib.pm_jn2018()
    d.n = self.n
    d.hints = _lib.PM_JN_UNIFORM_AREA if self.cols.uniform_area else 0
    if self.arith == "contracted":
      d.hints |= _lib.PM_JN_CONTRACTED
    if self.shared_coef and self.cols.uniform_area and self.cols.shared_halves:
      d.hints |= _lib.PM_JN_SHARED_COEF
    if self.split_lanes:
      d.hints |= _lib.PM_JN_SPLIT_LANES
    if self._div3():
      d.hints |= _lib.PM_JN_DIV3_PROVEN
    d.cols = self.cols.descriptor()
    d.wA, d.Psi_SO = self.wA.ptr, self.so.Psi.ptr
    d.Psi_res_b, d.Psi_res_n = self.tw.psibz1.ptr, self.tw.psibz2.ptr
    ml, t = _lib.pm_so_ml(), self.ml
    ml.n, ml.nz, ml.ny, ml.reserved = t.n, t.nz, t.ny, 0
    ml.y, ml.bs, ml.Psi_s = t.y.ptr, t.bs.ptr, t.Psi_s.ptr
    ml.b_basin, ml.Psi_b = None, None
    ml.surflux, ml.rest_mask, ml.b_rest = t.surflux.ptr, t.rest_mask.ptr, t.b_rest.ptr
    ml.Ks, ml.h, ml.L, ml.v_pist = t.Ks, t.h, t.L, t.v_pist
    ml.status = t.status.ptr
    d.ml = ml
    return d

  def _stops_after_update(self, ii):
    return ((self.recorder is not None and ii % self.recorder.Diag_iters == 0) or
            (self.diag is not None and self.diag.due(ii, self.diag_iters)))

  def _run_fused(self, nsteps):
    """The loop through pm_jn2018_run: one launch per stretch that ends where the script samples
    its diagnostics (right after a MOC update) or at the end of the run."""
    self._no_indices_in_fused_run()
    M, remaining = self.M, int(nsteps)
    while remaining > 0:
      ii = self.ii
      sch = _lib.pm_run_schedule()
      sch.m_steps = M
      fresh = self._updated_at == ii  # this iteration's update is behind us
      sch.n_first = 0 if (ii % M == 0 and not fresh) else min(M - ii % M, remaining)
      pos, rem = ii + sch.n_first, remaining - sch.n_first
      blocks, stopped = [], False
      while rem > 0:
        if self._stops_after_update(pos):
          blocks.append(0)
          stopped = True
          break
        ns = min(M, rem)
        blocks.append(ns)
        pos += ns
        rem -= ns
      sch.n_updates, sch.n_last = len(blocks), (blocks[-1] if blocks else 0)
      d = _lib.pm_jn2018_loop()
      d.jn = self._jn_descriptor()
      d.so = self.so.descriptor(self.b_basin, self.ml.bs)
      d.tw = self.tw.descriptor(self.b_basin, self.b_north, Psi_SO=self.so.Psi,
                                wA1=self.wA_basin, wA2=self.wA_north,
                                store_psib=self.recorder is not None)
      d.dt, d.sched = self.dt, sch
      check(lib.pm_memset(self.ml.status.ptr, 0, self.ml.status.nbytes, _sh(self.stream)))
      with launch_span(self.timer, "k_jn2018_run", self.stream):
        check(lib.pm_jn2018_run(C.byref(d), _sh(self.stream)))
      remaining -= pos - ii
      self.ii = pos
      if stopped:
        self._updated_at = pos
        self._after_update()

  def run(self, nsteps):
    if self._fused_run:
      return self._run_fused(nsteps)
    remaining = int(nsteps)
    while remaining > 0 and self._fused:
      self._apply_forcing()
      if self.ii % self.M == 0 and self._updated_at != self.ii:
        self._update()
        self._after_update()
      n = min(self.M - self.ii % self.M, remaining)
      self._fused_steps(n)
      self.ii += n
      remaining -= n
    while remaining > 0:
      if (self._use_graph and self.recorder is None and self.diag is None and
          self.indices is None and self.ii % self.M == 0 and remaining >= self.M):
        if self._graph is None:
          with Graph.capture(self.stream) as cap:
            self._block()
          self._graph = cap.graph
        self._graph.launch(self.stream)
        self.ii += self.M
        remaining -= self.M
        continue
      self._apply_forcing()
      if self.ii % self.M == 0 and self._updated_at != self.ii:
        self._update()
        self._after_update()
      self._step()
      self.ii += 1
      remaining -= 1

  def moc_update(self):
    """The MOC update of the current step (run_JansenNadeau_2018.py:204-217) ahead of run(), so
    that Psi / Psi_SO of this step can be read before it is taken; run() does not repeat it.
    Only at a step the script updates at (ii % MOC_up_iters == 0)."""
    if self.ii % self.M:
      raise ValueError("step %d is not a MOC update step (MOC_up_iters=%d)" % (self.ii, self.M))
    self._apply_forcing()
    if self._updated_at != self.ii:
      self._update()
      self._after_update()
      self._updated_at = self.ii

  at_restart_point = moc_update

  def drift_fields(self):
    return CoupledEnsemble.drift_fields(self) + [("bs_SO", self.ml.bs, self.ny, self.ny)]

  def state(self):
    return self._download(b_basin=self.b_basin, b_north=self.b_north, bs_SO=self.ml.bs,
                          Psi=self.tw.Psi, Psi_SO=self.so.Psi, Psi_iso_b=self.tw.psibz1,
                          Psi_iso_n=self.tw.psibz2, Psi_s=self.ml.Psi_s)


class JN2018ImplicitEnsemble(JN2018Ensemble):
  """JN2018Ensemble with both columns advanced by backward Euler (pm_jn2018_steps_implicit): an
  extension with no reference counterpart -- run_JansenNadeau_2018.py's columns are forward Euler,
  which at its own nz = 200 cannot take its dt = 30 d (kappa dt / dz^2 > 1/2).  Stable at any dt;
  a tolerance path against the explicit class, which stays the bit-identical one.

  The loop, the MOC update, the recorder, the gather, `state()`, `drift_fields()`, MEMBER_KEYS,
  RESTART_PHASE and FORCING_TARGETS are JN2018Ensemble's; only the step differs: BC switch -> both
  columns by ColumnBatch.steps(scheme="implicit") -> mixed layer, fused over the steps between two
  MOC updates into one launch.  The options of the explicit kernels (lanes_per_col, use_graph,
  arith, shared_coef, fused_run, split_lanes) are not accepted."""

  def __init__(self, cfg, stream=None, fused=None, comm=None, n_total=None, diag_iters=None,
               keep_history=False, gather="all", gather_overlap=True, forcing=None, noise=None):
    """`fused`: None = the fused kernel where it applies (nz <= 256), else one step at a time
    (pm_jn2018_bc_switch, pm_column_steps_implicit, pm_so_ml_step); False forces the latter;
    True where the kernel does not apply is a ValueError.  The two are bit-identical.  The other
    arguments as for JN2018Ensemble."""
    if fused and cfg['z'].size > 256:
      raise ValueError("fused=True needs nz <= 256 (nz=%d)" % cfg['z'].size)
    JN2018Ensemble.__init__(self, cfg, stream=stream, fused=fused, comm=comm, n_total=n_total,
                            diag_iters=diag_iters, keep_history=keep_history, gather=gather,
                            gather_overlap=gather_overlap, forcing=forcing, noise=noise)

  def _step(self):
    check(lib.pm_jn2018_bc_switch(C.byref(self._bc), _sh(self.stream)))
    self.cols.steps(self.wA, self.dt, 1, scheme="implicit")
    self.ml.step(self.b_basin, self.so.Psi, self.dt)

  def _jn_descriptor(self):
    d = JN2018Ensemble._jn_descriptor(self)
    d.hints = 0  # (the hints vouch for what the explicit kernels use)
    return d

  def _fused_steps(self, nsteps):
    d = self._jn_descriptor()
    with launch_span(self.timer, "k_jn2018_implicit", self.stream):
      check(lib.pm_jn2018_steps_implicit(C.byref(d), self.dt, int(nsteps), _sh(self.stream)))


class TwoBasinEnsemble(CoupledEnsemble):
  """twobasin_NadeauJansen.py: Atlantic, northern-sinking and Pacific columns; AMOC
  (Atl vs north) and zonal (Atl vs Pac) thermal-wind overturnings mapped to isopycnal space;
  one Southern-Ocean overturning per basin sector.  Columns are stored Atl rows [0,n),
  north rows [n,2n), Pac rows [2n,3n).

  An update (:111-122) is four independent solves of the columns' current profiles:
  {SO_Atl.solve, AMOC.solve / Psibz} and {SO_Pac.solve, ZOC.solve / Psibz}.  Each pair is ONE
  launch (pm_so_tw_update: Psi_SO.solve and the thermal wind of a member by one wavefront) and
  the two pairs run one after the other, or SIDE BY SIDE on two streams (`overlap_updates=True`),
  joined by an event; the forcing of the columns (:103-105) is formed by the column kernel itself
  from the overturnings (PM_OP_WA_TWOBASIN) -- the same device functions and operations as four
  separate launches and a forcing kernel, bit-identical results.
  `comm`, `n_total`, `diag_iters`, `keep_history`, `gather`, `gather_overlap`: as for
  TwoColEnsemble; the exchanged fields are what the script samples every `plot_iters` steps
  (:124-133): the three columns' b and the four overturnings.  `arith="contracted"`: the columns
  step in the opt-in tolerance mode."""

  NGROUPS = 3
  FIELDS = ("b_Atl", "b_north", "b_Pac", "Psi_AMOC", "Psi_ZOC", "Psi_SO_Atl", "Psi_SO_Pac")

  @classmethod
  def members(cls, cfg):
    return np.size(cfg['tau']) if np.ndim(cfg['tau']) else 1

  def __init__(self, cfg, stream=None, lanes_per_col=0, comm=None, n_total=None,
               diag_iters=None, keep_history=False, arith="exact", overlap_updates=False,
               gather="all", gather_overlap=True, use_graph=True):
    # Measured at 2048 members (profiles/r05/probe_c6_modes.py, us per interval of 24 steps):
    #   the two update pairs one after the other on ONE stream, the forcing formed by the column
    #   kernel (PM_OP_WA_TWOBASIN): 58.2 -- the default;  ... with pm_twobasin_forcing: 63.8;
    #   the pairs side by side on two streams (`overlap_updates=True`; fork / join events):
    #   66-78, 64-70 replayed from a hipGraph (`use_graph`: a whole interval captured once; only
    #   with overlap_updates, off while a LaunchTimer is attached).  With the round-5 thermal wind
    #   a pair is 17 us: the events cost more than the overlap gives.  (Both pairs as the halves
    #   of ONE launch: 33 us against 2 x 17 -- not kept.)
    self.arith = self._check_arith(arith)
    self._use_graph, self._graph = bool(use_graph), None
    z, y = cfg['z'], cfg['y']
    nz, ny = z.size, y.size
    n = self.members(cfg)
    self.n, self.nz, self.ny = n, nz, ny
    self.dt, self.M, self.nb = float(cfg['dt']), int(cfg['MOC_up_iters']), int(cfg['nb'])
    self.lanes, self.stream = lanes_per_col, stream
    self.timer = None  # optional device.LaunchTimer
    kap = _rows(cfg['kappa'], n, nz)
    rows = lambda v: _rows(v, n, nz)  # noqa: E731
    self.cols = ColumnBatch(
        z, np.concatenate([kap, kap, kap]),
        np.concatenate([rows(cfg['A_Atl']), rows(cfg['A_north']), rows(cfg['A_Pac'])]),
        np.concatenate([rows(cfg['b_Atl0']), rows(cfg['b_north0']), rows(cfg['b_Pac0'])]),
        bs=np.concatenate([_vec(cfg['bs'], n), _vec(cfg['bs_north'], n), _vec(cfg['bs'], n)]),
        bbot=np.full(3 * n, float(cfg['bbot'])), N2min=float(cfg['N2min']),
        do_conv=np.concatenate([np.zeros(n, bool), np.ones(n, bool), np.zeros(n, bool)]),
        stream=stream)
    zd = self.cols.z
    self.amoc = ThermwindBatch(z, n, f=cfg['f_AMOC'], nb=self.nb, stream=stream, z_dev=zd)
    self.zoc = ThermwindBatch(z, n, f=cfg['f_ZOC'], nb=self.nb, stream=stream, z_dev=zd)
    so = dict(tau=cfg['tau'], KGM=cfg['K'], f=cfg['f_SO'], stream=stream, z_dev=zd)
    self.so_atl = PsiSOBatch(z, y, n, L=cfg['L_Atl'], **so)
    self.so_pac = PsiSOBatch(z, y, n, L=cfg['L_Pac'], **so)
    # the two sectors' Psi_SO in ONE array (rows [0, n) Atlantic, [n, 2n) Pacific): with the two
    # thermal winds' psibz arrays that is what the column kernel forms its forcing from
    # (PM_OP_WA_TWOBASIN) -- no forcing launch between an update and the steps that follow it
    self._so_psi = DeviceArray.zeros((2 * n, nz), stream=stream)
    self.so_atl.Psi, self.so_pac.Psi = self._so_psi.view(0, n), self._so_psi.view(n, n)
    self._forcing_in_k1 = True
    self._wA_fresh = False  # does self.wA hold the forcing of the last update?
    self.bs_SO = DeviceArray.from_host(_rows(cfg['bs_SO'], n, ny) if np.ndim(cfg['bs_SO']) == 1
                                       else cfg['bs_SO'], stream=stream)
    self.wA = DeviceArray.zeros((3 * n, nz), stream=stream)
    b, w = self.cols.b, self.wA
    self.b_Atl, self.b_north, self.b_Pac = b.view(0, n), b.view(n, n), b.view(2 * n, n)
    self.wA_Atl, self.wA_north, self.wA_Pac = w.view(0, n), w.view(n, n), w.view(2 * n, n)
    self.ii = 0
    self.diag_iters = (cfg.get('plot_iters', cfg.get('Diag_iters', 10 * self.M))
                       if diag_iters is None else diag_iters)
    self._init_gather(comm, n_total, keep_history, gather, gather_overlap)
    self._pairs = nz <= 256   # pm_so_tw_update covers the shape
    self._overlap = bool(overlap_updates)
    if self._overlap:
      self._side, self._ev_fork, self._ev_join = Stream(), Event(), Event()
    # initial diagnostics (:58-79): AMOC against b2 = 0.01*b_Atl, the rest on the initial columns
    b2 = DeviceArray.from_host(rows(cfg['b2_init']), stream=stream)
    self._update(b_north=b2)
    check(lib.pm_stream_sync(_sh(stream)))  # b2 is released on return

  def _solve_pair(self, so, tw, b_so, b1, b2, stream):
    """{Psi_SO.solve on b_so, thermal wind of (b1, b2)} on `stream`: one launch when the shape
    allows, else two."""
    if self._pairs:
      ds = so.descriptor(b_so, self.bs_SO)
      dw = tw.descriptor(b1, b2, store_psib=False)
      with launch_span(self.timer, "k_so_tw_update", stream):
        check(lib.pm_so_tw_update(C.byref(ds), C.byref(dw), _TW_ALL, _sh(stream)))
      return
    keep_so, keep_tw = so.stream, tw.stream
    so.stream = tw.stream = stream
    try:
      with launch_span(self.timer, "k_psi_so", stream):
        so.update(b_so, self.bs_SO)
      with launch_span(self.timer, "k_thermwind", stream):
        tw.update(b1, b2, ops=_TW_ALL, store_psib=False)
    finally:
      so.stream, tw.stream = keep_so, keep_tw

  def _update(self, b_north=None):
    bA, bP = self.b_Atl, self.b_Pac
    bN = self.b_north if b_north is None else b_north
    atl = lambda st: self._solve_pair(self.so_atl, self.amoc, bA, bA, bN, st)  # noqa: E731
    pac = lambda st: self._solve_pair(self.so_pac, self.zoc, bP, bA, bP, st)   # noqa: E731
    if self._overlap:
      self._side_by_side(pac, atl)
    else:
      atl(self.stream)
      pac(self.stream)
    self._wA_fresh = False
    if not self._forcing_in_k1:
      self._form_forcing()

  def _form_forcing(self):
    """wA of the three columns as an array (:103-105; launches of 1-2 steps, and
    `_forcing_in_k1 = False`): pm_twobasin_forcing."""
    check(lib.pm_twobasin_forcing(self.n, self.nz, self.amoc.psibz1.ptr, self.zoc.psibz1.ptr,
                                  self.so_atl.Psi.ptr, self.amoc.psibz2.ptr,
                                  self.zoc.psibz2.ptr, self.so_pac.Psi.ptr, self.wA_Atl.ptr,
                                  self.wA_north.ptr, self.wA_Pac.ptr, _sh(self.stream)))
    self._wA_fresh = True

  def _steps(self, n):
    """n column steps under the forcing of the last update: formed by the column kernel itself
    (>= 3 steps per launch) or taken from the array."""
    if self._forcing_in_k1 and n >= 3:
      self.cols.steps(None, self.dt, n, lanes_per_col=self.lanes, arith=self.arith,
                      twobasin_forcing=(self.amoc.psibz, self.zoc.psibz, self._so_psi))
      return
    if not self._wA_fresh:
      self._form_forcing()
    self.cols.steps(self.wA, self.dt, n, lanes_per_col=self.lanes, arith=self.arith)

  def run(self, nsteps):
    remaining = int(nsteps)
    while remaining > 0:
      n = self._interval(remaining)
      if (self._use_graph and self.timer is None and self._overlap and n == self.M and
          self.ii % self.M == 1 and self.M >= 3):
        # a full interval: M steps, then the update they end on
        if self._graph is None:
          with Graph.capture(self.stream) as cap:
            self._steps(n)
            self._update()
          self._graph = cap.graph
        self._graph.launch(self.stream)
        self.ii += n
        remaining -= n
        self._gather_if_due(self.ii - 1)
        continue
      with launch_span(self.timer, "k_column_steps" if n >= 3 else "k_column_steps_short",
                       self.stream):
        self._steps(n)
      self.ii += n
      remaining -= n
      if (self.ii - 1) % self.M == 0:
        self._update()
        self._gather_if_due(self.ii - 1)

  def fields(self):
    """The seven fields the script samples every plot_iters steps (:124-133)."""
    return dict(b_Atl=self.b_Atl, b_north=self.b_north, b_Pac=self.b_Pac,
                Psi_AMOC=self.amoc.Psi, Psi_ZOC=self.zoc.Psi, Psi_SO_Atl=self.so_atl.Psi,
                Psi_SO_Pac=self.so_pac.Psi)

  def state(self):
    return self._download(**self.fields())


class TwoBasinSweep(TwoBasinEnsemble):
  """TwoBasinEnsemble with what the other coupled drivers have: the cfg read per member by a
  stated rule (MEMBER_KEYS, so `restrict` / `subset` / `run_to_steady` work), a restart point, a
  `forcing=ForcingSchedule(...)` and `scheme="implicit"`.  With neither `forcing` nor `scheme` it
  IS the parent: the same launches in the same order, bit-identical `fields()` / `state()`.

  Restart point (RESTART_PHASE = 1): the loop is `step; if ii % M == 0: update`
  (twobasin_NadeauJansen.py:99-122), the two-column shape, so a member can be restarted at
  s = 1 (mod MOC_up_iters), after the update that follows step s - 1.  The parent's constructor
  forms its first AMOC against cfg['b2_init'] (the script's :64), not against the northern column;
  `subset` therefore hands the new ensemble its members' CURRENT northern rows as `b2_init`, so the
  constructor's own update is the update after step s - 1 on the carried-over columns, and the
  subset comes back with the overturnings of its own three columns.  (`bbot` and `N2min` stay
  shared scalars, as in the parent.)

  `forcing`: bs (the Atlantic and Pacific columns share it, :41-47: two destinations), bs_north,
  tau (both sectors' Psi_SO: two destinations) and bs_SO (the one array both sectors read), applied
  by the rule of `_apply_forcing`: at s = 0 and s = 1 (mod MOC_up_iters), ahead of the steps;
  the constructor's own update uses the cfg's values.  `noise=NoiseForcing(...)` perturbs the same
  targets at the same instants (bs and tau: one noise state for both destinations).  While a
  schedule or a noise is bound the loop runs launch by launch: no hipGraph is captured
  (`use_graph` with `overlap_updates` is the slower option anyway, see the parent's constructor).

  `scheme="implicit"`: the three column groups step with backward Euler (pm_twobasin_forcing and
  pm_column_steps_implicit on the array -- the default, measured no slower -- or
  pm_column_steps_implicit_twobasin, the forcing formed in the kernel, bit-identical:
  IMPLICIT_FORMED chooses).  Updates,
  gather, forcing and steady runs are unchanged.  Like the other implicit paths this is an
  EXTENSION with no reference counterpart -- the script's columns are forward Euler, which above
  about nz = 125 cannot take its own dt = 30 d -- and a tolerance path; the default stays explicit
  and bit-identical.  Not with arith="contracted" or a non-zero lanes_per_col (ValueError)."""

  MEMBER_KEYS = dict(kappa=("rows", "z"), A_Atl=("rows", "z"), A_north=("rows", "z"),
                     A_Pac=("rows", "z"), b_Atl0=("rows", "z"), b_north0=("rows", "z"),
                     b_Pac0=("rows", "z"), b2_init=("rows", "z"), bs=("vec",), bs_north=("vec",),
                     tau=("vec",), K=("vec",), bs_SO=("rows", "y"))
  RESTART_PHASE = 1
  FORCING_TARGETS = dict(bs=(("cols.bs", 0, None), ("cols.bs", 2, None)),
                         bs_north=(("cols.bs", 1, None),),
                         tau=(("so_atl.tau", 0, "tau"), ("so_pac.tau", 0, "tau")),
                         bs_SO=(("bs_SO", 0, "y"),))
  # the implicit step forms its forcing in the kernel (True) or reads it from pm_twobasin_forcing's
  # array (False): bit-identical.  Measured per interval at 2048 x nz = 200: formed 171.6 us, array
  # 167.8 us -- formed is not faster, so the driver takes the array path
  IMPLICIT_FORMED = False

  def __init__(self, cfg, stream=None, lanes_per_col=0, comm=None, n_total=None,
               diag_iters=None, keep_history=False, arith="exact", overlap_updates=False,
               gather="all", gather_overlap=True, use_graph=True, forcing=None,
               scheme="explicit", noise=None):
    n = self.members(cfg)
    self._check_forcing(forcing, cfg, n, noise=noise, comm=comm, n_total=n_total)
    check_scheme(scheme, arith=arith, lanes_per_col=lanes_per_col)
    self.scheme = scheme
    # every per-member key as an explicit [n, ...] array by its rule: the parent's own reading of
    # such arrays is the identity
    cfg = dict(cfg, **{key: self.read(cfg, key, n) for key in self.MEMBER_KEYS})
    TwoBasinEnsemble.__init__(self, cfg, stream=stream, lanes_per_col=lanes_per_col, comm=comm,
                              n_total=n_total, diag_iters=diag_iters, keep_history=keep_history,
                              arith=arith, overlap_updates=overlap_updates, gather=gather,
                              gather_overlap=gather_overlap, use_graph=use_graph)
    self._bind_forcing(forcing, cfg)  # (behind the constructor's update: it used the cfg's values)

  def drift_fields(self):
    nz = self.nz
    return [("b_Atl", self.b_Atl, nz, nz), ("b_north", self.b_north, nz, nz),
            ("b_Pac", self.b_Pac, nz, nz)]

  def capture_fields(self):
    nz = self.nz
    return self.drift_fields() + [
        ("Psi_AMOC", self.amoc.Psi, nz, nz), ("Psi_ZOC", self.zoc.Psi, nz, nz),
        ("Psi_SO_Atl", self.so_atl.Psi, nz, nz), ("Psi_SO_Pac", self.so_pac.Psi, nz, nz)]

  def subset(self, keep, cfg, kw):
    # the constructor's first AMOC is formed against b2_init: at a restart point that is the
    # current northern column (the class docstring's restart rule)
    cfg = dict(cfg, b2_init=self.b_north.download(stream=self.stream))
    return CoupledEnsemble.subset(self, keep, cfg, kw)

  def _steps(self, n):
    if self.scheme != "implicit":
      return TwoBasinEnsemble._steps(self, n)
    if self.IMPLICIT_FORMED:
      self.cols.steps_implicit_twobasin(self.dt, n, self.amoc.psibz, self.zoc.psibz, self._so_psi)
      return
    if not self._wA_fresh:
      self._form_forcing()
    self.cols.steps(self.wA, self.dt, n, scheme="implicit")

  def _span(self, n):
    if self.scheme == "implicit":
      return "k_column_implicit_twobasin" if self.IMPLICIT_FORMED else "k_column_implicit"
    return "k_column_steps" if n >= 3 else "k_column_steps_short"

  def run(self, nsteps):
    if self._forcing is None and self._noise is None and self.scheme == "explicit":
      return TwoBasinEnsemble.run(self, nsteps)
    remaining = int(nsteps)
    while remaining > 0:
      self._apply_forcing()
      n = self._interval(remaining)
      with launch_span(self.timer, self._span(n), self.stream):
        self._steps(n)
      self.ii += n
      remaining -= n
      if (self.ii - 1) % self.M == 0:
        self._update()
        self._gather_if_due(self.ii - 1)
