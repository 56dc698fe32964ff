"""The shapes of the two-basin driver's edge tests (tests/twobasin_cases.py, run on the device by
tests/test_twobasin_gpu.py), checked without a GPU."""
import numpy as np
import pytest

import twobasin_cases as B


def test_twobasin_splits_alternate_and_reach_the_compared_steps():
  assert np.cumsum(B.SPLITS)[-1] == B.SNAPS[-1] == 2 * B.M + 4
  assert {n >= 3 for n in B.SPLITS} == {True, False}


@pytest.mark.parametrize("shape", B.SHAPES, ids=B.label)
def test_twobasin_shapes_stay_finite_in_the_oracle(shape):
  """The members tests/test_twobasin_gpu.py compares with the oracle stay finite over its 52 steps
  (a run that blew up would agree with anything that blew up)."""
  c = B.cfg(shape)
  assert c["z"].size == shape[0] and c["y"].size == shape[1] and np.size(c["tau"]) == B.N
  for m in B.MEMBERS:
    out = B.oracle_snaps(shape, m)
    assert set(out) == set(B.SNAPS)
    for s in B.SNAPS:
      for k, v in out[s].items():
        assert np.isfinite(v).all(), (m, s, k)
    assert np.abs(out[B.SNAPS[-1]]["Psi_AMOC"]).max() > 0
