"""TwoBasinSweep on the GPU: identity with its parent, pm_column_steps_implicit_twobasin against the
forcing launch plus the array kernel, the implicit driver, forcing schedules (fixture G27) and
steady runs with compaction."""
import ctypes as C

import numpy as np
import pytest

import implicit_column_cases as I
import twobasin_cases as B
import twobasin_sweep_cases as S
from conftest import load_golden, relerr
from pymoc_amd import configs

pytestmark = pytest.mark.gpu

FIELDS = S.FIELDS
M = B.M
SMALL = (17, 9, 30)
OPS = 3  # PM_OP_CONVECT | PM_OP_VERTADVDIFF


def _same(sa, sb, what=()):
  for k in FIELDS:
    assert np.array_equal(sa[k], sb[k]), what + (k,)


def _run_splits(ens):
  out = []
  for n in B.SPLITS:
    ens.run(n)
    out.append(ens.state())
  return out


# ------------------------------------------------------------------ 1. the subclass changes nothing
@pytest.mark.parametrize("shape", [SMALL, (81, 33, 30)], ids=B.label)
def test_sweep_without_its_keywords_is_the_parent(gpu, shape):
  c = B.cfg(shape)
  a, b = gpu.TwoBasinEnsemble(c), gpu.TwoBasinSweep(c)
  assert b.scheme == "explicit" and b._forcing is None and b._forcing_in_k1
  _same(a.state(), b.state(), ("initial",))
  sa, sb = _run_splits(a), _run_splits(b)
  for i in range(len(B.SPLITS)):
    _same(sa[i], sb[i], (i,))
  assert set(b.fields()) == set(a.fields()) == set(FIELDS)


# ------------------------------------------- 2. formed kernel == forcing launch + array kernel
def _column_case(nz, n, seed):
  """3 n columns built directly (northern group do_conv) and three overturning arrays [2 n, nz]
  of both signs, so that the upwind branches mix within a column."""
  rng = np.random.RandomState(seed)
  z = np.linspace(-4000., 0., nz)
  ncols = 3 * n
  kap = configs.twobasin_kappaeff(z)[None, :] * (1. + 0.3 * rng.rand(ncols, 1))
  area = np.repeat(np.array([7e13, 5.5e12, 1.7e14]), n)[:, None] * (1. + 0.2 * rng.rand(ncols, 1))
  area = np.broadcast_to(area, (ncols, nz)).copy()
  bs = np.concatenate([np.full(n, 0.02), np.full(n, 0.00036), np.full(n, 0.02)])
  b0 = 0.02 * np.exp(z / 300.)[None, :] + (z / z[0] * -0.0011)[None, :]
  b0 = b0 * (1. + 1e-3 * rng.randn(ncols, nz))
  do_conv = np.concatenate([np.zeros(n, bool), np.ones(n, bool), np.zeros(n, bool)])
  psi = [8. * rng.randn(2 * n, nz) for _ in range(3)]  # Sv
  return dict(z=z, kappa=kap, area=area, b0=b0, bs=bs, do_conv=do_conv, psi=psi)


def _batch(gpu, c):
  return gpu.ColumnBatch(c["z"], c["kappa"], c["area"], c["b0"], bs=c["bs"], bbot=-0.0011,
                         N2min=2e-7, do_conv=c["do_conv"])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nz", [4, 64, 65, 200, 300, 1024])
def test_formed_forcing_equals_forcing_launch_plus_array_kernel(gpu, nz, n):
  """nz covers P = 1 on both sides of the lane boundary (4, 64) and P = 2, 4, 6, 16; n = 3 is a batch
  of 9 columns, whose last block of 4 waves is partly filled."""
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray
  c = _column_case(nz, n, seed=nz + n)
  dt = 30. * B.DAY
  iso, zon, so = (DeviceArray.from_host(p) for p in c["psi"])
  wA = DeviceArray.zeros((3 * n, nz))
  _lib.check(_lib.lib.pm_twobasin_forcing(
      n, nz, iso.view(0, n).ptr, zon.view(0, n).ptr, so.view(0, n).ptr, iso.view(n, n).ptr,
      zon.view(n, n).ptr, so.view(n, n).ptr, wA.view(0, n).ptr, wA.view(n, n).ptr,
      wA.view(2 * n, n).ptr, None))
  # the forcing the array holds is the script's, :103-105, in float64
  A, Z, P = c["psi"]
  want = np.concatenate([(A[:n] + Z[:n] - P[:n]) * 1e6, (-A[n:]) * 1e6, (-Z[n:] - P[n:]) * 1e6])
  assert np.array_equal(wA.download(), want)
  w = want[:, 1:-1]  # the interior levels' forcing: both upwind branches, in every column at nz >= 64
  assert (w > 0).any() and (w < 0).any()
  assert nz < 64 or ((w > 0).any(axis=1).all() and (w < 0).any(axis=1).all())
  for nsteps in (1, 2, 5):
    f, a = _batch(gpu, c), _batch(gpu, c)
    f.steps_implicit_twobasin(dt, nsteps, iso, zon, so)
    a.steps(wA, dt, nsteps, scheme="implicit")
    bf = f.get_b()
    assert np.isfinite(bf).all() and not np.array_equal(bf, c["b0"])
    assert np.array_equal(bf, a.get_b()), nsteps
    assert np.array_equal(f.get_nonfinite(), a.get_nonfinite())
    assert not f.get_nonfinite().any()
  one = _batch(gpu, c)  # 5 launches of 1 step == 1 launch of 5
  for _ in range(5):
    one.steps_implicit_twobasin(dt, 1, iso, zon, so)
  assert np.array_equal(one.get_b(), bf)
  # a column that holds an inf: the flags of the two paths agree, and only that column is flagged
  bad = dict(c, b0=c["b0"].copy())
  bad["b0"][3 * n - 1, nz // 2] = np.inf
  f, a = _batch(gpu, bad), _batch(gpu, bad)
  f.steps_implicit_twobasin(dt, 2, iso, zon, so)
  a.steps(wA, dt, 2, scheme="implicit")
  assert np.array_equal(f.get_nonfinite(), a.get_nonfinite())
  assert f.get_nonfinite().tolist() == [0] * (3 * n - 1) + [1]
  assert np.array_equal(f.get_b().view(np.uint64), a.get_b().view(np.uint64))


# ------------------------------------------------------------------------- 3. the implicit driver
def _hand_issued(gpu, c, nsteps):
  """pm_twobasin_forcing, pm_column_steps_implicit and the parent's _update, issued by hand in
  the loop's order."""
  from pymoc_amd import _lib
  e = gpu.TwoBasinSweep(c, scheme="implicit")
  remaining = nsteps
  while remaining > 0:
    n = e._interval(remaining)
    gpu.TwoBasinEnsemble._form_forcing(e)
    d = e.cols.descriptor()
    _lib.check(_lib.lib.pm_column_steps_implicit(C.byref(d), e.wA.ptr, e.dt, n, OPS, None))
    e.ii += n
    remaining -= n
    if (e.ii - 1) % e.M == 0:
      gpu.TwoBasinEnsemble._update(e)
  return e.state()


def _cfg(shape, n):
  nz, ny, days = shape
  return dict(configs.config_twobasin(N=n, nz=nz, ny=ny), dt=B.DAY * days)


@pytest.mark.parametrize("shape", [SMALL, (200, 51, 30)], ids=B.label)
def test_implicit_driver_splits_and_hand_issued_sequence(gpu, shape):
  from pymoc_amd.device import LaunchTimer
  c = _cfg(shape, 4)
  total = 2 * M + 4
  assert sum(B.SPLITS) == total and c["MOC_up_iters"] == M
  one = gpu.TwoBasinSweep(c, scheme="implicit")
  assert one.n == 4
  one.timer = LaunchTimer()
  one.run(total)
  ref = one.state()
  names = {name for name, _, _ in one.timer.spans}
  assert ("k_column_implicit_twobasin" if one.IMPLICIT_FORMED else "k_column_implicit") in names
  assert not names & {"k_column_steps", "k_column_steps_short"}
  sp = gpu.TwoBasinSweep(c, scheme="implicit")
  for n in B.SPLITS:
    sp.run(n)
  _same(ref, sp.state(), ("splits",))
  other = gpu.TwoBasinSweep(c, scheme="implicit")
  other.IMPLICIT_FORMED = not one.IMPLICIT_FORMED  # the other of the two bit-identical paths
  other.run(total)
  _same(ref, other.state(), ("other path",))
  _same(ref, _hand_issued(gpu, c, total), ("hand issued",))
  assert one.nonfinite_members().size == 0


def test_implicit_driver_at_nz200_dt30_finite_maxprinciple_and_tolerance(gpu):
  """nz = 200 at the script's dt = 30 d (kappa dt / dz^2 = 1.29: beyond forward Euler).  After 3 M
  steps everything is finite and the Atlantic and Pacific columns (no convection) lie within the
  range of their initial profile and boundary values.  One launch interval of one member, rebuilt
  with implicit_column_cases' restatement in float64 and in longdouble: the engine's distance from
  the longdouble result is at most 8 x the float64 restatement's own."""
  n = 4
  c = _cfg((200, 51, 30), n)
  z = c["z"]
  nz = z.size
  r = np.max(c["kappa"]) * c["dt"] / np.min(np.diff(z)) ** 2
  assert r > 1.0
  e = gpu.TwoBasinSweep(c, scheme="implicit")
  e.run(1)  # step 0 and its update: the first step of a launch interval comes next
  b_before = e.cols.get_b()
  iso, zon, so = (a.download() for a in (e.amoc.psibz, e.zoc.psibz, e._so_psi))
  e.run(M)
  b_after = e.cols.get_b()
  e.run(3 * M - M - 1)
  st = e.state()
  assert e.ii == 3 * M
  for k in FIELDS:
    assert np.isfinite(st[k]).all(), k
  assert e.nonfinite_members().size == 0
  rows = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n, nz))  # noqa: E731
  two = lambda a, b: np.concatenate([a, b])  # noqa: E731
  case = dict(do_conv=np.zeros(2 * n, bool), use_bzbot=np.zeros(2 * n, bool),
              b0=two(rows(c["b_Atl0"]), rows(c["b_Pac0"])), bbot=np.full(2 * n, c["bbot"]),
              bs=np.full(2 * n, c["bs"]))
  excess = I.maxprinciple_excess(case, two(st["b_Atl"], st["b_Pac"]))
  print("maximum-principle excess %.3g (<= 1 passes)" % excess)
  assert excess <= 1.0

  # one interval of member j: its three columns as a case of the restatement
  j = 1
  idx = np.array([j, n + j, 2 * n + j])
  wA = np.stack([(iso[j] + zon[j] - so[j]) * 1e6, (-iso[n + j]) * 1e6,
                 (-zon[n + j] - so[n + j]) * 1e6])
  area = np.stack([rows(c["A_Atl"][j])[0], rows(c["A_north"][j])[0], rows(c["A_Pac"][j])[0]])
  kap = np.broadcast_to(c["kappa"], (3, nz)).copy()
  one = dict(z=z, b0=b_before[idx], ksel=np.zeros(3, np.int32), kappa_sets=kap[None],
             area=area, weff_given=False, forcing=wA,
             dAk_sets=np.gradient(area * kap, z, axis=-1)[None], dt=c["dt"],
             bs=np.array([c["bs"], c["bs_north"], c["bs"]], dtype=np.float64),
             bbot=np.full(3, c["bbot"]), bzbot=np.zeros(3), N2min=np.full(3, c["N2min"]),
             use_bzbot=np.zeros(3, bool), do_conv=np.array([False, True, False]))
  r64 = I.restatement(one, [M], np.float64)[M]
  rld = I.restatement(one, [M], np.longdouble)[M]
  scale = float(np.max(np.abs(rld)))
  own = float(np.max(np.abs(r64.astype(np.longdouble) - rld))) / scale
  eng = float(np.max(np.abs(b_after[idx].astype(np.longdouble) - rld))) / scale
  print("one interval of %d steps at nz = 200: engine %.3e, float64 restatement %.3e from the "
        "longdouble result: ratio %.2f (bound %.0f)" % (M, eng, own, eng / own, I.GPU_TOL_FACTOR))
  assert own > 0.0
  assert eng <= I.GPU_TOL_FACTOR * own


# ------------------------------------------------------------------------------------ 4. forcing
def _small_schedule(c, n):
  ny = c["y"].size
  i = np.arange(n)
  t = c["dt"] * np.array([0.5, 20., 30.5, 70.])
  ramp = np.array([0., 0.3, 0.45, 1.])
  return t, dict(
      bs=c["bs"] * (1. + 0.1 * ramp),                                              # [K] shared
      bs_north=c["bs_north"] + 3e-4 * ramp[:, None] * (1. + i)[None, :],           # [K, n]
      tau=np.asarray(c["tau"])[None, :] * (1. + 0.2 * ramp[:, None] * (1. + i)[None, :]),
      bs_SO=c["bs_SO"][None, None, :] * (1. + 0.04 * ramp[:, None, None] * (1. + i)[None, :, None])
      + np.zeros((4, n, ny)))                                                      # [K, n, ny]


def _interp(t, v, time):
  """np.interp of knot values v [K, ...] at `time`, along the knot axis."""
  flat = v.reshape(v.shape[0], -1)
  out = np.array([np.interp(time, t, flat[:, q]) for q in range(flat.shape[1])])
  return out.reshape(v.shape[1:])


def _upload(e, t, values, time):
  """What the schedule writes at `time`, uploaded by hand into the arrays the kernels read."""
  n = e.n
  bs = np.full(n, _interp(t, values["bs"], time))
  e.cols.bs.upload(np.concatenate([bs, _interp(t, values["bs_north"], time), bs]), e.stream)
  tau = _interp(t, values["tau"], time)
  e.so_atl.tau.upload(tau, e.stream)
  e.so_pac.tau.upload(tau, e.stream)
  e.bs_SO.upload(_interp(t, values["bs_SO"], time), e.stream)


def test_forcing_equals_uploads_by_hand_and_lands_in_both_destinations(gpu):
  n = 3
  c = _cfg(SMALL, n)
  t, values = _small_schedule(c, n)
  f = gpu.TwoBasinSweep(c, forcing=gpu.ForcingSchedule(t, **values), overlap_updates=True)
  assert f._use_graph and f._overlap  # the parent would capture whole intervals; a schedule must not
  h = gpu.TwoBasinSweep(c, overlap_updates=True, use_graph=False)
  _same(f.state(), h.state(), ("initial",))  # the constructor's update uses the cfg's values
  for s, nsteps in ((0, 1), (1, M)):
    _upload(h, t, values, s * c["dt"])
    h.run(nsteps)
  f.run(3)
  f.run(M - 2)
  assert f.ii == h.ii == M + 1
  _same(f.state(), h.state(), (M + 1,))
  for s, nsteps in ((M + 1, M), (2 * M + 1, M), (3 * M + 1, 3)):
    _upload(h, t, values, s * c["dt"])
    h.run(nsteps)
  f.run(30)
  f.run(3 * M + 4 - f.ii)
  assert f.ii == h.ii == 3 * M + 4 and f._graph is None
  _same(f.state(), h.state(), ("end",))
  # (c) the arrays after the run hold np.interp at the last applied time, in every destination
  last = (3 * M + 1) * c["dt"]
  assert f._forced_at == 3 * M + 1
  bs = f.cols.bs.download()
  assert np.array_equal(bs[:n], bs[2 * n:])
  assert np.array_equal(bs[:n], np.full(n, np.interp(last, t, values["bs"])))
  assert np.array_equal(bs[n:2 * n], _interp(t, values["bs_north"], last))
  ta, tp = f.so_atl.tau.download(), f.so_pac.tau.download()
  assert np.array_equal(ta, tp) and np.array_equal(ta, _interp(t, values["tau"], last))
  assert np.array_equal(f.bs_SO.download(), _interp(t, values["bs_SO"], last))
  # and the schedule did something: an unforced run ends elsewhere
  u = gpu.TwoBasinSweep(c)
  u.run(3 * M + 4)
  assert relerr(f.state()["b_Atl"], u.state()["b_Atl"]) > 1e-6


def test_forcing_against_the_reference_g27(gpu):
  g = load_golden("twobasin_forcing")
  values = {k[len("values_"):]: g[k] for k in g.files if k.startswith("values_")}
  e = gpu.TwoBasinSweep(S.cfg(), forcing=gpu.ForcingSchedule(g["knots"], **values))
  assert e.n == S.N
  worst, done = 0.0, 0
  for s in S.SNAPS:
    e.run(s - done)
    done = s
    st = e.state()
    for k in FIELDS:
      worst = max(worst, relerr(st[k], g["s%03d_%s" % (s, k)]))
  print("TwoBasinSweep under G27's schedule: worst distance to the reference %.3g" % worst)
  assert worst <= S.TOL
  assert e.nonfinite_members().size == 0


# ------------------------------------------------------------------------------------- 5. steady
def test_run_to_steady_counts_compaction_and_plain_run_equality(gpu):
  c = B.cfg(SMALL)
  n = B.N
  tol = np.zeros(n)
  tol[[0, 3, 4, 7, 8, 9]] = np.inf
  kw = dict(max_steps=1 + 6 * M, check_every=2 * M)
  res = {cb: gpu.run_to_steady(gpu.TwoBasinSweep, c, tol, compact_below=cb, **kw) for cb in (1, 0)}
  plain = gpu.TwoBasinEnsemble(c)
  at, done = {}, 0
  for s in (1 + 2 * M, 1 + 6 * M):
    plain.run(s - done)
    done = s
    at[s] = plain.state()
  for cb, r in res.items():
    assert r.counts() == dict(converged=6, nonfinite=0, maxsteps=4), cb
    assert set(r.fields) == set(FIELDS)
    want_steps = np.where(np.isinf(tol), 1 + 2 * M, 1 + 6 * M)
    assert np.array_equal(r.steps, want_steps), cb
    for m in range(n):
      for k in FIELDS:
        assert np.array_equal(r.fields[k][m], at[int(r.steps[m])][k][m]), (cb, m, k)
  assert len(res[1].compactions) >= 1 and res[1].compactions[0][1:] == (n, 4)
  assert res[0].compactions == []
  assert res[1].member_steps < res[0].member_steps
  for k in FIELDS:
    assert np.array_equal(res[1].fields[k], res[0].fields[k]), k
  assert np.array_equal(res[1].drift, res[0].drift)
