"""PM_OP_WA_TWOBASIN / PM_OP_WA_PSI on the device: the column kernel forms its forcing from
overturning rows -- every launch of tests/column_forcing_cases.py against NumPy and the CPU oracle,
bit for bit (the contracted instantiation within its tolerance), with the overturning arrays sized
exactly as the drivers allocate them."""
import numpy as np
import pytest

import column_forcing_cases as T
from test_column_gpu import CONTRACTED_RTOL, _rel

pytestmark = pytest.mark.gpu


def _flags(ref):
  return (~np.isfinite(ref).all(axis=1)).astype(np.int32)


def _same_bits(a, b):
  """Equal as bit patterns (-0.0 is not +0.0: the forcing of a northern row at the zeroed top and
  bottom level is -0.0); NaNs need only coincide, their payloads are not compared."""
  a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  nan = np.isnan(a)
  return (a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and
          np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]))


@pytest.mark.parametrize("case", T.CASES, ids=T.label)
def test_formed_forcing_vs_oracle(gpu, case):
  """The launch selects the instantiation the table names; b and the non-finite flags of EVERY
  column equal the oracle's under the NumPy-formed forcing; the library's forcing entry gives
  NumPy's array bit for bit, and stepping with that array gives the same bits as forming the
  forcing in the kernel."""
  inp = T.inputs(case.mod, case.nz, case.n, case.variant == "areaz")
  wA, ref = T.reference(case)
  dev = T.DeviceCase(gpu, case.mod, inp, case.variant)
  formed, array = dev.batch(), dev.batch()
  if case.kernel == "CK_STEPS_DIV3_UA":
    assert formed.div3_proven
  name = dev.kernel_name(formed, case.nsteps, case.lanes)
  print("%s: %s" % (T.label(case), name))
  assert name == T.kernel_name(case)
  dev.steps_formed(formed, case.nsteps, case.lanes)
  got = formed.get_b()
  if case.kernel == "CK_STEPS_CONTRACTED":
    err = _rel(got, ref)
    print("contracted: %.3g of max|b|" % err)
    assert err <= CONTRACTED_RTOL, err
    assert np.isfinite(ref).all()
  else:
    assert np.array_equal(got, ref, equal_nan=True), np.nonzero((got != ref).any(axis=1))[0]
  assert np.array_equal(formed.get_nonfinite(), _flags(ref))
  wA_dev = dev.forcing_array()
  assert _same_bits(wA_dev.download(), wA)
  dev.steps_array(array, wA_dev, case.nsteps, case.lanes)
  assert np.array_equal(array.get_b(), got, equal_nan=True)
  assert np.array_equal(array.get_nonfinite(), _flags(ref))


@pytest.mark.parametrize("lanes", T.LANES)
@pytest.mark.parametrize("mod", T.MODS)
def test_formed_forcing_enters_the_ieee_leg(gpu, mod, lanes):
  """Members whose FORMED forcing leaves the exact-division window -- a row at 2^300, an inf level
  in a Psi_SO row, a NaN level in an iso row -- and columns of the last group scaled by 2^-1000:
  they and their untouched neighbours (same wave on 16 and 32 lanes, same block on 64) equal the
  oracle bit for bit, flags included."""
  nz, n, nsteps = 100, 21, 4
  inp, cols = T.planted(mod, T.inputs(mod, nz, n))
  wA = T.forcing(mod, inp)
  assert np.isfinite(wA[3]).all() and np.abs(wA[3]).max() > 2.0**300  # (finite after * 1e6)
  ref = T.step(inp, wA, nsteps)
  clean = T.reference(T.Case(mod, None, lanes, nz, n, nsteps, "default"))[1]
  rest = np.setdiff1d(np.arange(inp["ncols"]), cols)
  assert np.array_equal(ref[rest], clean[rest]) and np.isfinite(ref[rest]).all()
  assert all(not np.array_equal(ref[m], clean[m], equal_nan=True) for m in cols)
  assert (~np.isfinite(ref).all(axis=1)).sum() >= 4
  dev = T.DeviceCase(gpu, mod, inp)
  formed, array = dev.batch(), dev.batch()
  want = "CK_STEPS_DIV3_UA" if lanes == 64 else "CK_STEPS_PLAIN"
  assert dev.kernel_name(formed, nsteps, lanes) == T.kernel_name(
      T.Case(mod, want, lanes, nz, n, nsteps, "default"))
  dev.steps_formed(formed, nsteps, lanes)
  got = formed.get_b()
  assert np.array_equal(got, ref, equal_nan=True), np.nonzero((got != ref).any(axis=1))[0]
  assert np.array_equal(formed.get_nonfinite(), _flags(ref))
  wA_dev = dev.forcing_array()
  assert _same_bits(wA_dev.download(), wA)
  dev.steps_array(array, wA_dev, nsteps, lanes)
  assert np.array_equal(array.get_b(), got, equal_nan=True)
