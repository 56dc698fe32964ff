"""Every row of the column launch plan (csrc/column.hip.h, PM_COLUMN_KERNELS) on the device: each
entry of tests/column_plan_cases.py launches the instantiation it names, and EVERY column of its
batch is compared with the CPU oracle -- bit for bit, the opt-in contracted arithmetic within its
tolerance -- together with every column's non-finite flag.  The expected values come from host
copies of the inputs alone, never from another kernel."""
import numpy as np
import pytest

from column_plan_cases import (CASES, DeviceCall, columns_per_wave, host_inputs, label,
                               oracle_result)

pytestmark = pytest.mark.gpu

CONTRACTED_RTOL = 1e-12  # max-norm per column, relative to max|reference| (test_column_gpu.py)


def _mismatch(case, inp, got, ref):
  """Which columns, which slot of their wave, which levels: the pattern names the fault."""
  bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
  cols = np.nonzero(bad.any(axis=1))[0]
  cpw = columns_per_wave(case)
  lv = np.nonzero(bad.any(axis=0))[0]
  return ("%s: %d of %d columns differ; first %s; slots col %% %d: %s; kinds %s; levels %d..%d (%d)" % (
      label(case), cols.size, got.shape[0], cols[:8].tolist(), cpw,
      sorted(set((cols % cpw).tolist())), sorted(set(inp["kinds"][cols].tolist())),
      lv.min() if lv.size else -1, lv.max() if lv.size else -1, lv.size))


def _run(gpu, case, inp, chunks):
  call = DeviceCall(gpu, case, inp)
  try:
    for n in chunks:
      assert call.kernel_name(n) == case.name
      call.steps(n)
    weff = call.forcing_row(inp["ordinary"]) if case.precombined else None
    return call.get_b(), call.get_nonfinite(), weff
  finally:
    call.free()


@pytest.mark.parametrize("case", CASES, ids=label)
def test_plan_row_every_column_vs_oracle(gpu, case):
  inp = host_inputs(case)
  ref = oracle_result(case, inp)  # (before any launch)
  bad_ref = ~np.isfinite(ref).all(axis=1)
  assert bad_ref.any() and not bad_ref.all()
  # a two-step entry runs as one launch of two steps and, on a second batch, as two launches
  runs = [[case.nsteps]] + ([[1, 1]] if case.nsteps == 2 else [])
  for chunks in runs:
    got, nf, weff = _run(gpu, case, inp, chunks)
    if case.arith == "contracted":
      # another arithmetic in the exact-division window (1e-12); a column outside it steps in the
      # IEEE form and stays bit-identical: every non-finite column is such a column
      with np.errstate(all="ignore"):
        scale = np.max(np.abs(ref), axis=1)
        err = np.max(np.abs(got - ref), axis=1) / scale
      fin = ~bad_ref
      print("contracted: worst finite column %.3e" % err[fin].max())
      assert (err[fin] <= CONTRACTED_RTOL).all(), (label(case), chunks, float(err[fin].max()))
      assert np.array_equal(got[bad_ref], ref[bad_ref], equal_nan=True), (label(case), chunks)
    elif not np.array_equal(got, ref, equal_nan=True):
      pytest.fail(_mismatch(case, inp, got, ref) + " (launches %s)" % chunks)
    bad = ~np.isfinite(got).all(axis=1)
    assert np.array_equal(nf != 0, bad), (label(case), chunks, np.nonzero((nf != 0) != bad)[0][:16].tolist())
    assert bad.any() and not bad.all()
    if weff is not None:
      assert np.isfinite(weff).all()
