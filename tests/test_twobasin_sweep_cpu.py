"""TwoBasinSweep and pm_column_steps_implicit_twobasin without a device: the class tables, the cfg
reading against the parent's, every refusal raised before device state exists, the C-ABI
declaration and refusals, and fixture G27 against the oracle restatement of the forced loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import twobasin_sweep_cases as S
from conftest import load_golden, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_Z = ("kappa", "A_Atl", "A_north", "A_Pac", "b_Atl0", "b_north0", "b_Pac0", "b2_init")
VEC = ("bs", "bs_north", "tau", "K")


def test_class_tables():
  from pymoc_amd import TwoBasinEnsemble, TwoBasinSweep
  assert issubclass(TwoBasinSweep, TwoBasinEnsemble)
  want = {k: ("rows", "z") for k in ROWS_Z}
  want.update({k: ("vec",) for k in VEC})
  want["bs_SO"] = ("rows", "y")
  assert TwoBasinSweep.MEMBER_KEYS == want
  assert TwoBasinSweep.RESTART_PHASE == 1
  assert TwoBasinEnsemble.MEMBER_KEYS is None and TwoBasinEnsemble.RESTART_PHASE is None
  assert TwoBasinSweep.FORCING_TARGETS == dict(
      bs=(("cols.bs", 0, None), ("cols.bs", 2, None)), bs_north=(("cols.bs", 1, None),),
      tau=(("so_atl.tau", 0, "tau"), ("so_pac.tau", 0, "tau")), bs_SO=(("bs_SO", 0, "y"),))
  # 6 descriptor targets of the 8
  from pymoc_amd import _lib
  assert sum(len(d) for d in TwoBasinSweep.FORCING_TARGETS.values()) == 6 <= _lib.PM_FORCING_MAX_TARGETS
  assert TwoBasinSweep.FIELDS == TwoBasinEnsemble.FIELDS and TwoBasinSweep.NGROUPS == 3


@pytest.mark.parametrize("N,nz", [(5, 5), (4, 17)])  # the first has n == nz: a length-n 1-D array
def test_read_equals_the_parents_reading(N, nz):    # is then the shared profile, for both
  from pymoc_amd import TwoBasinSweep, configs
  from pymoc_amd.ensembles import _rows, _vec
  cfg = configs.config_twobasin(N=N, nz=nz, ny=9)
  n = TwoBasinSweep.members(cfg)
  assert n == N
  for k in ROWS_Z:
    got = TwoBasinSweep.read(cfg, k, n)
    assert got.shape == (n, nz) and np.array_equal(got, _rows(cfg[k], n, nz)), k
  for k in ("bs", "bs_north"):
    assert np.array_equal(TwoBasinSweep.read(cfg, k, n), _vec(cfg[k], n)), k
  for k in ("tau", "K"):  # the parent hands these to PsiSOBatch as they are: (n,) arrays
    assert np.array_equal(TwoBasinSweep.read(cfg, k, n), np.asarray(cfg[k], dtype=np.float64)), k
  ny = cfg["y"].size
  parent = _rows(cfg["bs_SO"], n, ny) if np.ndim(cfg["bs_SO"]) == 1 else cfg["bs_SO"]
  assert np.array_equal(TwoBasinSweep.read(cfg, "bs_SO", n), parent)
  # a per-member bs_SO (1-D of length n != ny: one value per member; 2-D: rows)
  for v in (np.arange(1., n + 1.), np.arange(1. * n * ny).reshape(n, ny)):
    c2 = dict(cfg, bs_SO=v)
    parent = _rows(v, n, ny) if v.ndim == 1 else v
    assert np.array_equal(TwoBasinSweep.read(c2, "bs_SO", n), parent)


@pytest.mark.parametrize("N,nz", [(5, 5), (4, 17)])
def test_restrict_then_read_round_trips(N, nz):
  from pymoc_amd import TwoBasinSweep, configs
  cfg = configs.config_twobasin(N=N, nz=nz, ny=9)
  rng = np.random.RandomState(3)
  cfg = dict(cfg, b2_init=rng.rand(N, nz), b_north0=rng.rand(N, nz), bs_north=rng.rand(N),
             bs_SO=rng.rand(N, 9))
  keep = np.array([N - 1, 0, 2])
  sub = TwoBasinSweep.restrict(cfg, keep)
  assert TwoBasinSweep.members(sub) == 3
  for k in TwoBasinSweep.MEMBER_KEYS:
    full = TwoBasinSweep.read(cfg, k, N)
    assert np.array_equal(TwoBasinSweep.read(sub, k, 3), full[keep]), k
  assert sub["bbot"] == cfg["bbot"] and sub["N2min"] == cfg["N2min"]  # shared scalars, untouched
  # and once more, on the restricted cfg (3 members: again unlike nz)
  sub2 = TwoBasinSweep.restrict(sub, np.array([2, 1]))
  for k in TwoBasinSweep.MEMBER_KEYS:
    assert np.array_equal(TwoBasinSweep.read(sub2, k, 2), TwoBasinSweep.read(cfg, k, N)[keep][[2, 1]]), k


def test_forcing_names_shapes_and_scheme_refusals_on_the_host():
  """All raised before any device state exists: ValueError, not a missing-device error."""
  from pymoc_amd import ForcingSchedule, TwoBasinSweep, configs
  cfg = configs.config_twobasin(N=4, nz=17, ny=9)
  assert TwoBasinSweep.forcing_lengths(cfg, 4) == dict(bs=1, bs_north=1, tau=1, bs_SO=9)
  one = configs.twobasin_member(nz=17, ny=9)  # scalar tau: one member
  assert TwoBasinSweep.members(one) == 1
  assert TwoBasinSweep.forcing_lengths(one, 1)["tau"] == 1
  t = [0., 1e6, 5e6]
  with pytest.raises(ValueError, match=r"'b_rest'.*bs, bs_SO, bs_north, tau"):
    TwoBasinSweep(cfg, forcing=ForcingSchedule(t, b_rest=np.zeros((3, 9))))
  for kw in (dict(bs=np.zeros((3, 5))), dict(bs_north=np.zeros((3, 4, 1))),
             dict(bs_SO=np.zeros(3)), dict(bs_SO=np.zeros((3, 4, 8))), dict(tau=np.zeros((3, 9))),
             dict(tau=np.zeros((3, 3)))):
    with pytest.raises(ValueError, match="%r: shape" % sorted(kw)[0]):
      TwoBasinSweep(cfg, forcing=ForcingSchedule(t, **kw))
  for kw in (dict(scheme="implicit", arith="contracted"), dict(scheme="implicit", lanes_per_col=32),
             dict(scheme="leapfrog")):
    with pytest.raises(ValueError):
      TwoBasinSweep(cfg, **kw)


def test_bind_rejects_destinations_of_unlike_row_length():
  from pymoc_amd import ForcingSchedule
  f = ForcingSchedule([0., 1.], bs=[0.02, 0.03])
  with pytest.raises(ValueError, match="row length"):
    f.bind(4, dict(bs=[(None, 0, 1), (None, 8, 2)]))


def test_run_to_steady_on_the_host():
  import pymoc_amd
  from pymoc_amd import ForcingSchedule, TwoBasinEnsemble, TwoBasinSweep, configs
  from pymoc_amd.steady import check_schedule
  s0, checks = check_schedule(TwoBasinSweep, 24, 48, 200)
  assert s0 == 1 and checks == [49, 97, 145, 193]
  cfg = configs.config_twobasin(N=4, nz=17, ny=9)
  f = ForcingSchedule([0., 1e6], bs=[0.02, 0.03])
  with pytest.raises(ValueError, match="forcing"):
    pymoc_amd.run_to_steady(TwoBasinSweep, cfg, 1e-6, 200, forcing=f)
  with pytest.raises(ValueError, match="multiple of MOC_up_iters"):
    pymoc_amd.run_to_steady(TwoBasinSweep, cfg, 1e-6, 200, check_every=25)
  with pytest.raises(ValueError, match="JN2018Ensemble and TwoColEnsemble.*TwoBasinSweep"):
    pymoc_amd.run_to_steady(TwoBasinEnsemble, cfg, 1e-6, 200)


def test_c_abi_declaration_and_refusals():
  from pymoc_amd import _lib
  L = _lib.lib
  hdr = open(os.path.join(ROOT, "include", "pymoc_hip.h")).read()
  m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int pm_column_steps_implicit_twobasin\(([^;]*)\);", hdr,
                re.S)
  assert m, "pm_column_steps_implicit_twobasin is not declared in the header"
  args = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
  assert args == ["const pm_columns *cols", "const double *iso", "const double *zon",
                  "const double *so", "double dt", "int32_t nsteps", "int32_t ops",
                  "pm_stream_t stream"]
  assert "twobasin_NadeauJansen.py:103-105" in m.group(1) and "TOLERANCE path" in m.group(1)
  res, argtypes = _lib.SIGNATURES["pm_column_steps_implicit_twobasin"]
  c_dp = _lib.SIGNATURES["pm_column_steps_implicit"][1][1]
  assert res is ctypes.c_int
  assert argtypes == [ctypes.POINTER(_lib.pm_columns), c_dp, c_dp, c_dp, ctypes.c_double,
                      ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]

  FAKE = 0x10000  # never dereferenced: every call below ends in a host-side check
  fn = L.pm_column_steps_implicit_twobasin

  def call(ops=3, nsteps=1, dt=1.0, arrays=(None, None, None), **shape):
    c = _lib.pm_columns()
    c.ncols, c.nz, c.nsel = 0, 10, 1
    for k, v in shape.items():
      setattr(c, k, v)
    rc = fn(ctypes.byref(c), arrays[0], arrays[1], arrays[2], dt, nsteps, ops, None)
    return rc, L.pm_last_error().decode()

  assert call()[0] == _lib.PM_OK          # empty batch: nothing to do
  assert call(nsteps=0)[0] == _lib.PM_OK
  assert call(ops=3 | _lib.PM_OP_WA_TWOBASIN)[0] == _lib.PM_OK  # implied, may be given
  for ops, word in ((3 | _lib.PM_OP_WEFF, "PM_OP_WEFF"), (3 | _lib.PM_OP_HORADV, "PM_OP_HORADV"),
                    (3 | _lib.PM_OP_CONTRACTED, "PM_OP_CONTRACTED"),
                    (3 | _lib.PM_OP_WA_PSI, "PM_OP_WA_PSI"), (3 | 128, "unknown op bits")):
    rc, msg = call(ops=ops)
    assert rc == _lib.PM_EINVAL and word in msg, (ops, msg)
  rc, msg = call(nsteps=-1)
  assert rc == _lib.PM_EINVAL and "nsteps" in msg
  for dt in (0.0, -1.0, float("inf"), float("nan")):
    rc, msg = call(dt=dt)
    assert rc == _lib.PM_EINVAL and "dt" in msg, dt
  for shape in (dict(nz=1), dict(nz=1025), dict(ncols=-3)):
    rc, msg = call(**shape)
    assert rc == _lib.PM_EINVAL and "nz" in msg, shape
  for ncols in (1, 2, 4, 3001):
    rc, msg = call(ncols=ncols, arrays=(FAKE, FAKE, FAKE))
    assert rc == _lib.PM_EINVAL and "multiple of 3" in msg, ncols
  for arrays in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
    rc, msg = call(ncols=3, arrays=arrays)
    assert rc == _lib.PM_EINVAL and "NULL" in msg and "iso, zon, so" in msg, arrays
  assert call(ncols=0, arrays=(None, None, None))[0] == _lib.PM_OK
  rc, msg = call(ncols=3, arrays=(FAKE, FAKE, FAKE))  # rows of a non-empty batch not given
  assert rc == _lib.PM_EINVAL and "pm_columns" in msg
  assert fn(None, None, None, None, 1.0, 1, 3, None) == _lib.PM_EINVAL
  # the sibling keeps its refusal
  c = _lib.pm_columns()
  c.ncols, c.nz, c.nsel = 0, 10, 1
  assert L.pm_column_steps_implicit(ctypes.byref(c), None, 1.0, 1, 3 | _lib.PM_OP_WA_TWOBASIN,
                                    None) == _lib.PM_EINVAL


def test_columnbatch_binding_exists_and_steps_keeps_its_refusals():
  from pymoc_amd.columns import ColumnBatch
  assert callable(ColumnBatch.steps_implicit_twobasin)
  x = np.zeros(4)
  bare = object.__new__(ColumnBatch)
  with pytest.raises(ValueError):
    ColumnBatch.steps(bare, None, 1.0, 1, scheme="implicit", twobasin_forcing=(x, x, x))
  with pytest.raises(TypeError, match="DeviceArray"):  # host data is not taken
    ColumnBatch.steps_implicit_twobasin(bare, 1.0, 1, x, x, x)


def test_g27_holds_what_the_cases_state():
  g = load_golden("twobasin_forcing")
  t, values = S.schedule()
  assert np.array_equal(g["knots"], t)
  for k, v in values.items():
    assert np.array_equal(g["values_" + k], v), k
  assert set(g.files) == ({"knots", "numpy_version", "scipy_version", "reference"} |
                          {"values_" + k for k in values} |
                          {"s%03d_%s" % (s, k) for s in S.SNAPS for k in S.FIELDS})
  assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "twobasin_forcing.npz")) < (
      os.path.getsize(os.path.join(ROOT, "tests", "golden", "twobasin.npz")) // 2)
  # the values change inside the run: every application sees another bs, tau steps once
  applied = [s for s in range(S.STEPS) if S.applied_at(s)]
  assert applied == [0, 1, 25, 49, 73]
  dt = S.members()[0]["dt"]
  bs = [S.member_values(values, t, s * dt, 0)["bs"] for s in applied]
  tau = [S.member_values(values, t, s * dt, 0)["tau"] for s in applied]
  assert len(set(bs[1:])) == 4 and bs[0] == values["bs"][0]
  assert tau[:3] == [0.12] * 3 and tau[3:] == [0.16] * 2


def test_oracle_restatement_of_the_forced_loop_agrees_with_g27():
  """The rule itself -- when an assigned value takes effect -- pinned to the reference,
  independent of the engine: the oracle's functions in run_twobasin's loop with the schedule
  applied at s = 0 and s = 1 (mod M) agree with the reference's classes to 1e-10 at the three
  stored steps; without the schedule they do not."""
  g = load_golden("twobasin_forcing")
  worst = 0.0
  for j in range(S.N):
    got = S.oracle_snaps(j)
    for s in S.SNAPS:
      for k in S.FIELDS:
        worst = max(worst, relerr(got[s][k], g["s%03d_%s" % (s, k)][j]))
  print("oracle restatement vs G27: worst %.3g" % worst)
  assert worst <= S.TOL
  plain = S.oracle_snaps(0, forced=False)
  assert max(relerr(plain[S.STEPS][k], g["s%03d_%s" % (S.STEPS, k)][0]) for k in S.FIELDS) > 1e-4
