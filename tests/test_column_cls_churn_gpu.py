"""The class loops of the column twin kernel (csrc/column.hip.h: k_column_steps_cls -- the
surface-only class and the integer filter of conv_spec_run) against the CPU oracle, bit for bit,
on columns that enter and leave those loops again and again (tests/column_cls_churn_cases.py;
tests/test_column_cls_churn_cpu.py asserts on the oracle alone that the events are there: joins
and first crossings in every tier and after every re-dispatch, false alarms of the filter, the
same batch at 2^-150 and 2^150).

Every case asserts on the host, before it runs, which launch-plan row and which of the two kernels
each of its launches takes (ColumnBatch.kernel_name / kernel_twin): both twin rows -- the
proven-quotient one in its forms 8, 7 and 6 and the plain one (fast = 2) -- and the unvouched entry
meet the twin at every launch of at least 64 steps; the 63 + 63 + 14 split, 16 and 32 lanes per
column and a batch without the uniform-Area hint run the same columns on k_column_steps."""
import numpy as np
import pytest

import column_cls_churn_cases as T
import column_forcing_cases as F

pytestmark = pytest.mark.gpu

# the batch's hints, and the Area that gives the form its name
VARIANTS = {"form8": (T.AREA_PROVEN, {}), "form7": (T.AREA_REJECTED, {}),
            "form6": (T.AREA_PROVEN, dict(div2=False)), "fast2": (T.AREA_PROVEN, dict(div3=False)),
            "unvouched": (T.AREA_PROVEN, dict(static_in_range=False))}


def _label(split):
  return "+".join(str(n) for n in split)


def _batch(gpu, c, variant):
  batch = gpu.ColumnBatch(c["z"], c["kappa"], c["area"], c["b0"], bs=c["bs"], bbot=c["bbot"],
                          N2min=c["N2min"], do_conv=True)
  hints = VARIANTS[variant][1]
  if hints:
    batch.use_hints(**hints)
  return batch


def _assert_row(batch, nz, variant, nsteps):
  """The launch-plan row, by the name pm_column_kernel_name reports for it."""
  P = 1 if nz <= 64 else 2
  assert batch.kernel_shape(64) == (64, P)
  if nz == 100:  # the headline's grid: each form really is the one the case names
    assert batch.div3_proven and batch.div2_grid_proven
    assert batch.div2_area_proven.all() == (variant != "form7")
    assert not batch.div2_area_proven.any() or variant != "form7"
  fast = 6 if batch.div3_proven and variant != "fast2" else 2  # CK_STEPS_DIV3_UA / CK_STEPS_PLAIN_UA
  assert batch.kernel_name(nsteps, lanes_per_col=64) == "k_column_steps<64,%d,%d,true,true>" % (P, fast)


def _compare(got, ref, c, trans):
  bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
  rows = np.nonzero(bad.any(axis=1))[0]
  assert rows.size == 0, (rows.size, [T.describe(c, int(i), np.nonzero(bad[i])[0].tolist(), trans)
                                      for i in rows[:8]])


def _run(gpu, nz, variant, split, scale=0):
  area = VARIANTS[variant][0]
  c = T.case(nz, area, scale)
  batch = _batch(gpu, c, variant)
  for n in split:
    _assert_row(batch, nz, variant, n)
    assert batch.kernel_twin(n, lanes_per_col=64) == (n >= 64)
  assert any(batch.kernel_twin(n, lanes_per_col=64) for n in split) == (split != T.CONTROL)
  for n in split:
    batch.steps(c["wA"], T.DT, n, lanes_per_col=64)
  _compare(batch.get_b(), c["ref"][sum(split)], c, T.case(nz, area)["trace"]["trans"])


def test_twin_threshold_and_eligibility(gpu):
  """kernel_twin: 64 steps and more of the one-wave-per-column uniform-Area rows, nothing else."""
  for nz in (9, 100, 128):
    c = T.case(nz, T.AREA_PROVEN)
    batch = _batch(gpu, c, "form8")
    assert [batch.kernel_twin(n, 64) for n in (1, 3, 63, 64, 65, 140)] == [False] * 3 + [True] * 3
    assert batch.kernel_twin(64) and not batch.kernel_twin(63)  # (the library's own choice of lanes)
    assert not batch.kernel_twin(140, 16) and not batch.kernel_twin(140, 32)
    assert not batch.kernel_twin(140, 64, horadv=True) and not batch.kernel_twin(140, 64, arith="contracted")
    batch.use_hints(div3=False)
    assert batch.kernel_twin(64, 64) and not batch.kernel_twin(63, 64)
    batch.use_hints(uniform_area=False)
    assert not batch.kernel_twin(140, 64)
  z = np.linspace(-4000., 0., 256)  # four levels per lane: a uniform-Area row without a twin
  wide = gpu.ColumnBatch(z, 1e-4, T.AREA_PROVEN, np.zeros((4, 256)), do_conv=True)
  assert wide.kernel_shape(64) == (64, 4) and not wide.kernel_twin(140, 64)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("split", T.SPLITS, ids=_label)
@pytest.mark.parametrize("nz", T.NZS)
def test_churning_columns_vs_oracle(gpu, nz, split, variant):
  _run(gpu, nz, variant, split)


@pytest.mark.parametrize("variant", ["form8", "fast2"])
@pytest.mark.parametrize("k", T.SCALES)
@pytest.mark.parametrize("split", [(140,), (70, 70), (64, 64, 12), T.CONTROL], ids=_label)
@pytest.mark.parametrize("nz", T.NZS)
def test_scaled_twins_vs_oracle(gpu, nz, split, k, variant):
  """The same batch at 2^-150 and 2^150: the integer filter compares exponents."""
  _run(gpu, nz, variant, split, scale=k)


@pytest.mark.parametrize("other", ["lanes16", "lanes32", "no-uniform-area-hint"])
@pytest.mark.parametrize("nz", T.NZS)
def test_same_columns_on_the_rows_without_a_twin(gpu, nz, other):
  """16 and 32 lanes per column, and 64 without the uniform-Area hint: not twin rows, same bits."""
  c = T.case(nz, T.AREA_PROVEN)
  lanes = {"lanes16": 16, "lanes32": 32}.get(other, 64)
  for split in ((140,), (70, 70)):
    batch = _batch(gpu, c, "form8")
    if lanes == 64:
      batch.use_hints(uniform_area=False)
      assert batch.kernel_name(split[0], 64).endswith(",2,true,false>")
    else:
      assert batch.kernel_shape(lanes)[0] == lanes
    for n in split:
      assert not batch.kernel_twin(n, lanes_per_col=lanes)
      batch.steps(c["wA"], T.DT, n, lanes_per_col=lanes)
    _compare(batch.get_b(), c["ref"][140], c, c["trace"]["trans"])


@pytest.mark.parametrize("nsteps", [70, 140])
def test_psi_forcing_formed_in_the_twin_bitwise(gpu, nsteps):
  """PM_OP_WA_PSI in launches long enough for the twin: test_column_gpu.py's
  test_forcing_formed_from_the_overturning_bitwise construction (config 2's columns, random
  overturning rows), with and without Psi_SO, against the array-forcing launch and the oracle."""
  import oracle as O
  from pymoc_amd import _lib, configs
  n = 48
  c = configs.config2(N=2 * n)
  nz = c["z"].size
  rng = np.random.default_rng(11)
  psi_iso = rng.standard_normal((2 * n, nz)) * 3.0
  psi_so = rng.standard_normal((n, nz))
  psi_iso[:, 0] = psi_iso[:, -1] = 0.0

  def make():
    return gpu.ColumnBatch(c["z"], c["kappa"], c["Area"], c["b0"], bs=c["bs"], bbot=c["bbot"],
                           N2min=c["N2min"], do_conv=c["do_conv"])
  d_iso, d_so = gpu.DeviceArray.from_host(psi_iso), gpu.DeviceArray.from_host(psi_so)
  for so_h, so_d in ((psi_so, d_so), (None, None)):
    wA = F.form_twocol(psi_iso, so_h)
    ref = O.column_ensemble_steps(c["z"], c["kappa"], c["Area"], c["b0"], wA, c["dt"], c["do_conv"],
                                  c["bs"], c["bbot"], c["N2min"], nsteps)
    a, b = make(), make()
    assert a.kernel_shape(64) == (64, 2)
    assert a.kernel_twin(nsteps, 64, ops=_lib.PM_OP_TIMESTEP | _lib.PM_OP_WA_PSI)
    assert b.kernel_twin(nsteps, 64)
    a.steps(None, c["dt"], nsteps, lanes_per_col=64, psi_forcing=(d_iso, so_d))
    b.steps(gpu.DeviceArray.from_host(wA), c["dt"], nsteps, lanes_per_col=64)
    assert np.array_equal(a.get_b(), b.get_b(), equal_nan=True)
    assert np.array_equal(a.get_b(), ref, equal_nan=True), np.nonzero((a.get_b() != ref).any(axis=1))[0]
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("nsteps", [70, 140])
@pytest.mark.parametrize("nz", [64, 100])
@pytest.mark.parametrize("mod", ["twobasin", "twocol"])
def test_formed_forcing_in_the_twin_vs_oracle(gpu, mod, nz, nsteps):
  """PM_OP_WA_TWOBASIN / PM_OP_WA_PSI on the inputs of tests/column_forcing_cases.py (convection on
  the northern rows from the first step on), 70 and 140 steps: the kernel-formed forcing, the
  array-forcing launch and the oracle agree bit for bit."""
  inp = F.inputs(mod, nz, 21)
  wA = F.forcing(mod, inp)
  ref = F.step(inp, wA, nsteps)
  dev = F.DeviceCase(gpu, mod, inp)
  formed, array = dev.batch(), dev.batch()
  assert formed.div3_proven
  assert dev.kernel_name(formed, nsteps, 64) == "k_column_steps<64,%d,6,true,true>" % (1 if nz <= 64 else 2)
  assert formed.kernel_twin(nsteps, 64, ops=dev.op | 7) and array.kernel_twin(nsteps, 64)
  dev.steps_formed(formed, nsteps, 64)
  got = formed.get_b()
  assert np.array_equal(got, ref, equal_nan=True), np.nonzero((got != ref).any(axis=1))[0]
  dev.steps_array(array, dev.forcing_array(), nsteps, 64)
  assert np.array_equal(array.get_b(), got, equal_nan=True)
  assert np.isfinite(ref).all()
