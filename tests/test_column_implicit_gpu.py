"""The implicit column step on the GPU (pm_column_steps_implicit, scheme="implicit") against the
NumPy restatement of the scheme (tests/implicit_column_cases.py), within 8 x E_REF of max|b|.
The scheme has no reference counterpart; what is bit-exact here is what the kernel shares with the
explicit path (convect) and its own invariances."""
import ctypes as C

import numpy as np
import pytest

import implicit_column_cases as I
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = I.GPU_TOL_FACTOR * I.E_REF


def _batch(gpu, case, b_dev=None):
  from pymoc_amd import _lib
  ks = case["kappa_sets"]
  bz = case["use_bzbot"]
  batch = gpu.ColumnBatch(case["z"], ks[0], case["area"], case["b0"], bs=case["bs"],
                          bbot=case["bbot"], bzbot=case["bzbot"] if bz.any() else None,
                          N2min=case["N2min"], do_conv=case["do_conv"],
                          kappa_alt=ks[1] if case["nsel"] == 2 else None)
  if bz.any():  # columns mixing bbot and bzbot: the flag is per column
    batch._flags_host[~bz] &= ~np.int32(_lib.PM_COL_BZBOT)
    batch._upload_flags()
  batch.set_ksel(case["ksel"])
  if b_dev is not None:
    batch.b = b_dev
    batch.set_b(case["b0"])
  return batch


def _implicit(batch, case, nsteps, **kw):
  batch.steps(case["forcing"], case["dt"], nsteps, scheme="implicit",
              precombined=case["weff_given"], **kw)


def _err(a, ref):
  return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("name", I.CASE_NAMES)
def test_every_case_matches_the_restatement(gpu, name):
  from pymoc_amd import _lib
  case, ref = I.get_case(name), I.reference(name)
  batch = _batch(gpu, case)
  for k in case["steps"]:
    batch.set_b(case["b0"])
    _implicit(batch, case, k)
    b = batch.get_b()
    e = _err(b, ref[k])
    print("%s nsteps=%d: max|gpu - restatement| / max|b| = %.3e = %.3f E_REF" % (name, k, e, e / I.E_REF))
    assert np.isfinite(b).all() and not batch.get_nonfinite().any()
    assert e <= TOL, (name, k, e)
  if case["do_conv"].any():
    # convect alone, one launch on each entry: the same device function, the same bits
    batch.set_b(case["b0"])
    _implicit(batch, case, 1, ops=_lib.PM_OP_CONVECT)
    imp = batch.get_b()
    batch.set_b(case["b0"])
    wA = np.zeros_like(case["b0"])
    batch.steps(wA, case["dt"], 1, ops=_lib.PM_OP_CONVECT)
    exp = batch.get_b()
    assert np.array_equal(imp, exp)
    host = case["b0"].copy()
    I.convect(host, case["z"], case["bs"], case["N2min"], case["do_conv"])
    assert np.array_equal(imp, host)
    assert (imp != case["b0"]).any()


@pytest.mark.parametrize("name", ["nz5", "nz65", "nz200", "nz257"])
def test_launch_splitting_and_forcing_forms(gpu, name):
  case = I.get_case(name)
  batch = _batch(gpu, case)
  _implicit(batch, case, 7)
  fused = batch.get_b()
  batch.set_b(case["b0"])
  for _ in range(7):
    _implicit(batch, case, 1)
  assert np.array_equal(batch.get_b(), fused)
  # precombined forcing (PM_OP_WEFF) from combine_forcing against wA itself
  assert not case["weff_given"]
  weff = batch.combine_forcing(case["forcing"])
  batch.set_b(case["b0"])
  batch.steps(weff, case["dt"], 7, scheme="implicit", precombined=True)
  pre = batch.get_b()
  assert _err(pre, fused) <= TOL
  assert _err(pre, I.reference(name)[7]) <= TOL


def test_a_callers_own_horadv_bit_is_refused_not_dropped(gpu):
  """The default `ops` means convect + vertadvdiff; PM_OP_HORADV asked for by the caller reaches
  the library, which refuses it (PM_EINVAL before any launch) and leaves b as it was."""
  from pymoc_amd import _lib
  case = I.get_case("nz5")
  batch = _batch(gpu, case)
  for ops in (_lib.PM_OP_HORADV, _lib.PM_OP_VERTADVDIFF | _lib.PM_OP_HORADV):
    with pytest.raises(_lib.PmError, match="PM_OP_HORADV") as e:
      _implicit(batch, case, 1, ops=ops)
    assert e.value.code == _lib.PM_EINVAL
  assert np.array_equal(batch.get_b(), case["b0"])
  _implicit(batch, case, 1)  # the default still steps
  assert _err(batch.get_b(), I.reference("nz5")[1]) <= TOL


@pytest.mark.parametrize("name", [n for n in I.CASE_NAMES if 100 in I.get_case(n)["steps"]])
def test_maximum_principle(gpu, name):
  case = I.get_case(name)
  if not I.maxprinciple_columns(case).any():
    pytest.fail("case %s has no column under the maximum principle" % name)
  batch = _batch(gpu, case)
  _implicit(batch, case, 100)
  x = I.maxprinciple_excess(case, batch.get_b())
  print("%s: excess %.3f of nz 2^-52 max|b|" % (name, x))
  assert x <= 1.0


def test_explicit_blows_up_where_implicit_holds(gpu):
  """nz = 33, uniform grid, constant kappa, r = kappa dt / dz^2 = 2: forward Euler amplifies the
  grid mode by |1 - 4 r| = 7 per step (NaN arithmetic, not a fault); backward Euler does not."""
  case = I.get_case("nz33_r2")
  dz = np.diff(case["z"])
  assert np.allclose(case["kappa_sets"][0] * case["dt"] / dz[0] ** 2, 2.0)
  batch = _batch(gpu, case)
  batch.steps(np.zeros_like(case["b0"]), case["dt"], 400)
  assert batch.get_nonfinite().all()
  batch.set_b(case["b0"])
  _implicit(batch, case, 400)
  assert not batch.get_nonfinite().any() and np.isfinite(batch.get_b()).all()
  assert I.maxprinciple_excess(case, batch.get_b()) <= 1.0


def test_consistency_with_the_explicit_step(gpu):
  """One step from a smooth state at dt and at dt / 2: implicit - explicit is O(dt^2), so the two
  differences stand 4 : 1.  The restatement against the oracle's explicit step gives
  I.CONSISTENCY_CPU_RATIO = 3.9257 on the CPU (test_column_implicit_cpu re-checks it)."""
  case = I.consistency_case()
  batch = _batch(gpu, case)
  diffs = []
  for dt in (case["dt"], 0.5 * case["dt"]):
    batch.set_b(case["b0"])
    batch.steps(case["forcing"], dt, 1, scheme="implicit")
    imp = batch.get_b()
    batch.set_b(case["b0"])
    batch.steps(case["forcing"], dt, 1)
    diffs.append(np.max(np.abs(imp - batch.get_b())))
  ratio = diffs[0] / diffs[1]
  print("implicit - explicit: %.3e at dt, %.3e at dt/2, ratio %.4f" % (diffs[0], diffs[1], ratio))
  assert diffs[1] > 1e4 * 2.0 ** -52 * np.max(np.abs(case["b0"]))  # far above rounding
  assert 3.5 <= ratio <= 4.5


@pytest.mark.parametrize("name", ["nz127", "nz65"])  # ncols = 1, 65
def test_neighbouring_rows_are_untouched(gpu, name):
  from pymoc_amd.device import DeviceArray
  case = I.get_case(name)
  ncols, nz = case["b0"].shape
  assert ncols in (1, 65)
  guard = np.full((ncols + 2, nz), -7.25e300)
  guard[0, ::2] = np.nan
  arena = DeviceArray.from_host(guard)
  batch = _batch(gpu, case, b_dev=arena.view(1, ncols))
  for k in (1, 7):
    _implicit(batch, case, k)
  after = arena.download()
  for row in (0, ncols + 1):
    assert after[row].tobytes() == guard[row].tobytes()
  assert np.isfinite(after[1:ncols + 1]).all()


def _twocol_cfg(so, n):
  from pymoc_amd import configs
  cfg = configs.config4(N=n, nz=20) if so else configs.config3(N=n, nz=20)
  cfg = dict(cfg)
  cfg["MOC_up_iters"] = 3
  cfg["dt"] = 120 * I.DAY  # kappa dt / dz^2 ~ 0.3 .. 3 at nz = 20: beyond the explicit limit
  return cfg


@pytest.mark.parametrize("so,overlap", [(False, False), (True, False), (True, True)])
def test_twocol_ensemble_is_the_hand_written_loop(gpu, so, overlap):
  from pymoc_amd import TwoColEnsemble
  from pymoc_amd._lib import check, lib
  from pymoc_amd.device import _sh
  cfg = _twocol_cfg(so, 3)
  ens = TwoColEnsemble(cfg, scheme="implicit", overlap_updates=overlap)
  ens.run(7)
  got = ens.state()
  hand = TwoColEnsemble(cfg, scheme="implicit", overlap_updates=overlap)
  for ii in range(7):
    if so and overlap:
      check(lib.pm_twocol_forcing(hand.n, hand.nz, hand.tw.psibz.ptr, hand.so.Psi.ptr,
                                  hand.wA.ptr, _sh(hand.stream)))
    hand.cols.steps(hand.wA, hand.dt, 1, scheme="implicit")
    if ii % hand.M == 0:
      hand._update()
  want = hand.state()
  assert set(got) == set(want)
  for k in got:
    assert np.array_equal(got[k], want[k], equal_nan=True), k
  assert np.isfinite(got["b_basin"]).all() and np.isfinite(got["b_north"]).all()
  # and it is not the explicit scheme
  exp = TwoColEnsemble(cfg, overlap_updates=overlap)
  exp.run(7)
  assert not np.array_equal(exp.state()["b_basin"], got["b_basin"])


@pytest.mark.parametrize("so", [False, True])
def test_run_to_steady_implicit_equals_plain_runs(gpu, so):
  import pymoc_amd
  from pymoc_amd import TwoColEnsemble
  cfg = _twocol_cfg(so, 5)
  tol = np.array([0., 1., 0., 1., 0.])
  runs = [pymoc_amd.run_to_steady(TwoColEnsemble, cfg, tol, 13, check_every=3, compact_below=cb,
                                  scheme="implicit") for cb in (0., 1.)]
  assert runs[0].compactions == [] and len(runs[1].compactions) >= 1
  plain = TwoColEnsemble(cfg, scheme="implicit")
  for s in sorted(set(runs[0].steps.tolist())):
    plain.run(s - plain.ii)
    st = plain.state()
    for res in runs:
      assert np.array_equal(res.steps, runs[0].steps)
      for k in np.nonzero(res.steps == s)[0]:
        for f in ("b_basin", "b_north", "Psi"):
          assert np.array_equal(res.fields[f][k], st[f][k], equal_nan=True), (f, k, s)
  assert len(set(runs[0].steps.tolist())) >= 2


def test_jn2018_does_not_take_the_keyword(gpu):
  from pymoc_amd import JN2018Ensemble, configs
  with pytest.raises(TypeError):
    JN2018Ensemble(configs.config5(N=2, nz=46, dt_days=30.), scheme="implicit")


def _column(gpu, case, j=0):
  return gpu.Column(z=case["z"], kappa=case["kappa_sets"][0, j], Area=case["area"][j],
                    b=case["b0"][j].copy(), bs=case["bs"][j], bbot=case["bbot"][j],
                    N2min=case["N2min"][j])


def test_dropin_column_queue_and_default(gpu):
  from pymoc_amd.modules import column as colmod
  case = I.get_case("nz63")
  wA, dt = case["forcing"][0], case["dt"]
  lazy = _column(gpu, case)
  for _ in range(3):
    lazy.timestep(wA=wA, dt=dt, scheme="implicit")
  assert lazy._q is not None and lazy._q[0] == 3 and lazy._q[6] == "implicit"
  was = colmod.LAZY
  colmod.LAZY = False
  try:
    eager = _column(gpu, case)
    for _ in range(3):
      eager.timestep(wA=wA, dt=dt, scheme="implicit")
    assert eager._q is None
  finally:
    colmod.LAZY = was
  assert np.array_equal(lazy.b, eager.b)
  assert _err(lazy.b, I.restatement(case, [3])[3][0]) <= TOL
  # a change of scheme flushes the queue
  col = _column(gpu, case)
  col.timestep(wA=wA, dt=dt, scheme="implicit")
  col.timestep(wA=wA, dt=dt, scheme="implicit")
  col.timestep(wA=wA, dt=dt)
  assert col._q[0] == 1 and col._q[6] == "explicit"
  col.timestep(wA=wA, dt=dt, scheme="implicit")
  assert col._q[0] == 1 and col._q[6] == "implicit"
  mixed = col.b.copy()
  ref = _column(gpu, case)
  colmod.LAZY = False
  try:
    for sch in ("implicit", "implicit", "explicit", "implicit"):
      ref.timestep(wA=wA, dt=dt, scheme=sch)
  finally:
    colmod.LAZY = was
  assert np.array_equal(mixed, ref.b)
  with pytest.raises(ValueError):
    col.timestep(wA=wA, dt=dt, vdx_in=wA, b_in=wA, scheme="implicit")
  with pytest.raises(ValueError):
    col.timestep(wA=wA, dt=dt, scheme="leapfrog")


def test_dropin_column_default_is_still_fixture_g1(gpu):
  g = load_golden("column_steps")
  for k in range(int(g["ncases"])):
    p = "c%02d_" % k
    dt, do_conv, bzbot, hor, bs, bbot, N2min = g[p + "par"]
    z = g[p + "z"]
    col = gpu.Column(z=z, kappa=g[p + "kappa"] + 0 * z, Area=g[p + "Area"] + 0 * z, b=g[p + "b0"].copy(),
                     bs=bs, bbot=bbot, bzbot=None if np.isnan(bzbot) else bzbot, N2min=N2min)
    kw = dict(vdx_in=g[p + "vdx"], b_in=g[p + "b_in"]) if hor else {}
    col.timestep(wA=g[p + "wA"], dt=dt, do_conv=bool(do_conv), **kw)
    assert np.array_equal(col.b, g[p + "b1"]), k
    for _ in range(2):
      col.timestep(wA=g[p + "wA"], dt=dt, do_conv=bool(do_conv), **kw)
    assert np.array_equal(col.b, g[p + "b3"]), k
