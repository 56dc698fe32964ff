"""The fused Jansen & Nadeau loop with implicit columns on the GPU (pm_jn2018_steps_implicit,
JN2018ImplicitEnsemble): bit for bit against the launch sequence it replaces, within
8 x E_COUPLED of the host restatement (tests/jn2018_implicit_cases.py), and through the ensemble
class with forcing, steady runs and the recorder."""
import ctypes as C

import numpy as np
import pytest

import jn2018_implicit_cases as J
from jn2018_members import OUTPUTS, Members

pytestmark = pytest.mark.gpu
TOL = J.GPU_TOL_FACTOR * J.E_COUPLED
_members = {}


@pytest.fixture
def members(gpu):
  def get(name):
    if name not in _members:
      _members[name] = Members(gpu, J.get_case(name), "pm_jn2018_steps_implicit")
    _members[name].reset()
    return _members[name]
  return get


def _bitwise(a, b, what):
  assert set(a) == set(b) == set(OUTPUTS)
  for k in OUTPUTS:
    assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_fused_equals_the_launch_sequence_bitwise(gpu, members, name):
  from pymoc_amd import _lib
  m = members(name)
  for k in J.STEP_COUNTS:
    m.reset()
    _lib.check(m.fused(k))
    got = m.outputs()
    m.reset()
    m.sequence(k, "implicit")
    want = m.outputs()
    _bitwise(got, want, (name, k))
    assert np.isfinite(got["b"]).all() and np.isfinite(got["bs_SO"]).all()
    assert not got["nonfinite"].any() and not got["status"].any()
    assert (got["b"] != m.case["b0"]).any()


@pytest.mark.parametrize("name", J.switching_cases())
def test_launch_splitting(gpu, members, name):
  from pymoc_amd import _lib
  m = members(name)
  _lib.check(m.fused(36))
  one = m.outputs()
  m.reset()
  for _ in range(36):
    _lib.check(m.fused(1))
  _bitwise(m.outputs(), one, (name, "36 x 1"))
  m.reset()
  _lib.check(m.fused(7))
  _lib.check(m.fused(29))
  _bitwise(m.outputs(), one, (name, "7 + 29"))


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_against_the_restatement(gpu, members, name):
  from pymoc_amd import _lib
  m = members(name)
  ref, _ = J.run(name)
  worst = 0.0
  for k in J.STEP_COUNTS:
    m.reset()
    _lib.check(m.fused(k))
    got = m.outputs()
    scale = np.max(np.abs(ref[k]["b"]))
    eb = float(np.max(np.abs(got["b"] - ref[k]["b"])) / scale)
    es = float(np.max(np.abs(got["bs_SO"] - ref[k]["bs_SO"])) / scale)
    print("%s nsteps=%d: columns %.3e, bs_SO %.3e of max|b| (%.3f, %.3f E_COUPLED)"
          % (name, k, eb, es, eb / J.E_COUPLED, es / J.E_COUPLED))
    worst = max(worst, eb, es)
    assert np.array_equal(got["ksel"].ravel(), ref[k]["ksel"]), (name, k)
    # the same CHOICE of bottom value: the restatement's is the same profile entry, to rounding
    assert np.max(np.abs(got["bbot"].ravel() - ref[k]["bbot"])) <= TOL * scale, (name, k)
    assert eb <= TOL and es <= TOL, (name, k, eb, es)
  print("%s: worst %.3e = %.3f E_COUPLED" % (name, worst, worst / J.E_COUPLED))


@pytest.mark.parametrize("name", ["nz63", "nz200"])  # n = 1, 5
def test_rows_that_are_not_the_launchs_own_stay_untouched(gpu, members, name):
  from pymoc_amd import _lib
  m = members(name)
  assert m.n in (1, 5)
  for k in (1, 7):
    _lib.check(m.fused(k))
    out = m.outputs()  # asserts every guard row, of every array the launch writes
  assert np.isfinite(out["b"]).all() and not out["status"].any() and not out["nonfinite"].any()
  # and the inputs the launch only reads
  c = m.case
  for dev, host in ((m.wA, c["wA"]), (m.Psi_SO, c["Psi_SO"]), (m.Pb, c["Psi_res_b"]),
                    (m.Pn, c["Psi_res_n"]), (m.cols.bs, c["bs"]), (m.ml.b_rest, c["b_rest"])):
    assert np.array_equal(dev.download().reshape(host.shape), host)


def test_refusals_and_trivial_launches(gpu, members):
  from pymoc_amd import _lib
  from pymoc_amd.device import synchronize
  m = members("nz65")
  before = m.outputs()

  def refused(rc, word):
    assert rc == _lib.PM_EINVAL
    msg = _lib.lib.pm_last_error().decode()
    assert word in msg, msg

  refused(m.fused(1, hints=_lib.PM_JN_CONTRACTED), "PM_JN_CONTRACTED")
  refused(m.fused(1, hints=_lib.PM_JN_SPLIT_LANES), "PM_JN_SPLIT_LANES")
  refused(m.fused(-1), "nsteps")
  for dt in (0.0, -1.0, np.inf, np.nan):
    refused(m.fused(1, dt=dt), "dt")
  d = m.descriptor()
  d.cols.nz = d.ml.nz = 257
  refused(_lib.lib.pm_jn2018_steps_implicit(C.byref(d), m.case["dt"], 1, None), "nz=257")
  # nothing to do: PM_OK, nothing written
  assert m.fused(0) == _lib.PM_OK
  d = m.descriptor()
  d.n = d.cols.ncols = d.ml.n = 0
  assert _lib.lib.pm_jn2018_steps_implicit(C.byref(d), m.case["dt"], 3, None) == _lib.PM_OK
  synchronize()
  _bitwise(m.outputs(), before, "refusals")
  # the hints of the explicit kernels are ignored
  ign = _lib.PM_JN_UNIFORM_AREA | _lib.PM_JN_SHARED_COEF | _lib.PM_JN_DIV3_PROVEN
  _lib.check(m.fused(2, hints=ign))
  a = m.outputs()
  m.reset()
  _lib.check(m.fused(2))
  _bitwise(a, m.outputs(), "hints")
  with pytest.raises(TypeError):
    gpu.JN2018ImplicitEnsemble(gpu.configs.config5(N=2, nz=46, dt_days=30.), arith="contracted")


def _same(sa, sb, what):
  assert set(sa) == set(sb)
  for k in sa:
    assert np.array_equal(sa[k].view(np.uint64), sb[k].view(np.uint64)), (what, k)


def _hand_loop(ens, nsteps):
  from pymoc_amd._lib import check, lib
  from pymoc_amd.device import _sh
  for ii in range(nsteps):
    if ii % ens.M == 0:
      ens._update()
    check(lib.pm_jn2018_bc_switch(C.byref(ens._bc), _sh(ens.stream)))
    ens.cols.steps(ens.wA, ens.dt, 1, scheme="implicit")
    ens.ml.step(ens.b_basin, ens.so.Psi, ens.dt)


@pytest.mark.parametrize("ny", [51, 65])
def test_ensemble_is_the_hand_written_loop(gpu, ny):
  from pymoc_amd import JN2018Ensemble, JN2018ImplicitEnsemble, configs
  cfg = configs.config5(N=3, nz=46, ny=ny, dt_days=30.)
  total = 2 * int(cfg["MOC_up_iters"]) + 5
  hand = JN2018ImplicitEnsemble(cfg)
  _hand_loop(hand, total)
  want = hand.state()
  for fused in (None, False):
    ens = JN2018ImplicitEnsemble(cfg, fused=fused)
    assert ens._fused is (fused is None)
    ens.run(total)
    got = ens.state()
    _same(got, want, fused)
    assert all(np.isfinite(v).all() for v in got.values())
    assert ens.nonfinite_members().size == 0
  exp = JN2018Ensemble(cfg)
  exp.run(total)
  assert not np.array_equal(exp.state()["b_basin"], want["b_basin"])


# config-5 physics at nz = 200 and the script's dt = 30 d (kappa dt / dz^2 = 0.77): the step after
# which the oracle's explicit run_jn2018 first holds a non-finite value, the same for each of the 4
# members (measured on the CPU)
EXPLICIT_FIRST_NONFINITE = 49


def test_stays_finite_where_explicit_does_not(gpu):
  from pymoc_amd import JN2018Ensemble, JN2018ImplicitEnsemble, configs
  cfg = configs.config5(N=4, nz=200, dt_days=30.)
  exp = JN2018Ensemble(cfg)
  exp.run(EXPLICIT_FIRST_NONFINITE)
  assert exp.nonfinite_members().size > 0
  imp = JN2018ImplicitEnsemble(cfg)
  imp.run(EXPLICIT_FIRST_NONFINITE)
  assert imp.nonfinite_members().size == 0
  st = imp.state()
  assert all(np.isfinite(st[k]).all() for k in ("b_basin", "b_north", "bs_SO"))
  assert not imp.ml.status.download().any()


def _forcing_case(gpu):
  from pymoc_amd import configs
  n = 3
  cfg = configs.config5(N=n, nz=46, dt_days=30.)
  cfg["MOC_up_iters"] = 6
  dt = cfg["dt"]
  t = dt * np.array([3., 12., 20.5])
  bs_north = np.stack([cfg["bs_north"], cfg["bs_north"] + 2e-4, cfg["bs_north"] + 5e-4])  # [K, n]
  tau = np.array([0.12, 0.14, 0.17])                                                      # [K]
  return cfg, t, dict(bs_north=bs_north, tau=tau)


def test_forcing_schedule_fused_stepwise_and_host_set(gpu):
  from pymoc_amd import JN2018ImplicitEnsemble
  cfg, t, values = _forcing_case(gpu)
  M, n = int(cfg["MOC_up_iters"]), 3
  total = 4 * M + 3
  sched = gpu.ForcingSchedule(t, **values)
  a = JN2018ImplicitEnsemble(cfg, forcing=sched)
  a.run(total)
  sa = a.state()
  b = JN2018ImplicitEnsemble(cfg, forcing=sched, fused=False)
  b.run(total)
  _same(sa, b.state(), "fused=False")
  # the forcing set from the host ahead of every interval (s = 0 mod M)
  c = JN2018ImplicitEnsemble(cfg)
  for s in range(0, total, M):
    assert c.ii == s
    north = np.array([np.interp(s * c.dt, t, values["bs_north"][:, j]) for j in range(n)])
    c.cols.bs.upload(np.concatenate([JN2018ImplicitEnsemble.read(cfg, "bs", n), north]), c.stream)
    c.so.set_tau(np.full(n, np.interp(s * c.dt, t, values["tau"])))
    c.run(min(M, total - s))
  _same(sa, c.state(), "host-set")
  plain = JN2018ImplicitEnsemble(cfg)
  plain.run(total)
  assert not np.array_equal(plain.state()["b_north"], sa["b_north"])  # the schedule acts


def test_run_to_steady_equals_plain_runs(gpu):
  import pymoc_amd
  from pymoc_amd import JN2018ImplicitEnsemble, configs
  cfg = configs.config5(N=5, nz=46, dt_days=30.)
  cfg["MOC_up_iters"] = 3
  tol = np.array([0., 1., 0., 1., 0.])
  runs = [pymoc_amd.run_to_steady(JN2018ImplicitEnsemble, cfg, tol, 13, check_every=3,
                                  compact_below=cb) for cb in (0., 1.)]
  assert runs[0].compactions == [] and len(runs[1].compactions) >= 1
  plain = JN2018ImplicitEnsemble(cfg)
  for s in sorted(set(runs[0].steps.tolist())):
    plain.run(s - plain.ii)
    plain.moc_update()
    st = plain.state()
    for res in runs:
      assert np.array_equal(res.steps, runs[0].steps)
      for k in np.nonzero(res.steps == s)[0]:
        for f in ("b_basin", "b_north", "bs_SO", "Psi"):
          assert np.array_equal(res.fields[f][k], st[f][k], equal_nan=True), (f, k, s)
  assert len(set(runs[0].steps.tolist())) >= 2


def test_recorder_series_are_the_states_of_a_plain_run(gpu):
  from pymoc_amd import JN2018ImplicitEnsemble, configs, diagnostics
  cfg = configs.config5(N=3, nz=46, dt_days=30.)
  cfg["MOC_up_iters"] = 4
  Diag, total = 8, 8 * 3 + 2
  for fused in (None, False):
    ens = JN2018ImplicitEnsemble(cfg, fused=fused)
    ens.recorder = diagnostics.JN2018Diagnostics(ens, Diag, total)
    ens.run(total)
    assert ens.recorder.nd == 3
    plain = JN2018ImplicitEnsemble(cfg, fused=fused)
    for j in range(3):
      plain.run(j * Diag - plain.ii)
      plain.moc_update()  # the sample is taken after the step's MOC update, before the step
      st = plain.state()
      for k in ("b_basin", "b_north", "bs_SO", "Psi_SO"):
        assert np.array_equal(getattr(ens.recorder, k)[:, :, j], st[k]), (fused, k, j)
      assert np.array_equal(ens.recorder.AMOC[:, :, j], st["Psi"]), (fused, j)
