"""The NumPy restatement of the index definitions against NumPy's own functions on every case of
the table, and the host half of RowIndices: window resolution and every ValueError (no device)."""
import numpy as np
import pytest

import indices_cases as IC


def _same_bits(a, b):
  a, b = np.float64(a), np.float64(b)
  return (np.isnan(a) and np.isnan(b)) or a.view(np.uint64) == b.view(np.uint64)


@pytest.mark.parametrize("nlev", IC.NLEVS)
def test_restated_extrema_are_numpys(nlev):
  """value == np.max(r) under `==` (or both NaN), pos == lo + np.argmax(r), and value is row[pos]
  to the bit -- NaN and signed-zero rows included; for every member's row."""
  z = IC.axis_for(nlev)
  seen = 0
  for name, kind, row, lo, hi, p in IC.cases(nlev):
    if kind not in ("max", "min"):
      continue
    for r in IC.member_rows(row, 3):
      v, pos = IC.restate(r, z, kind, lo, hi, p)
      w = r[lo:hi + 1]
      ref, arg = (np.max(w), np.argmax(w)) if kind == "max" else (np.min(w), np.argmin(w))
      assert pos == lo + arg, name
      assert (np.isnan(v) and np.isnan(ref)) or v == ref, name
      assert _same_bits(v, r[pos]), name
      seen += 1
  assert seen >= 3 * 16  # (nlev = 1 has the fewest: 8 shapes of row, max and min)


@pytest.mark.parametrize("nlev", IC.NLEVS)
def test_restated_at_is_np_interp(nlev):
  z = IC.axis_for(nlev)
  seen = 0
  for name, kind, row, lo, hi, p in IC.cases(nlev):
    if kind != "at":
      continue
    v, pos = IC.restate(row, z, kind, lo, hi, p)
    with np.errstate(invalid="ignore"):
      assert _same_bits(v, np.interp(p, z, row)), name
    assert pos == -1
    seen += 1
  assert seen >= 5


def test_restated_cross_and_mean_on_known_rows():
  z = np.array([-4., -3., -1., 0.])
  row = np.array([-2., 2., 1., -1.])
  v, pos = IC.restate(row, z, "cross", 0, 3, 0.0)
  assert (v, pos) == (-0.5, 2)            # the topmost of the two crossings
  assert IC.restate(row, z, "cross", 0, 1, 0.0) == (-3.5, 0)
  v, pos = IC.restate(np.abs(row), z, "cross", 0, 3, 0.0)
  assert np.isnan(v) and pos == -1
  assert IC.restate(row, z, "cross", 0, 3, -1.0) == (0.0, 3)  # row[hi] == level
  v, pos = IC.restate(row, z, "mean", 0, 3, 0.0)
  assert (v, pos) == ((0.0 * 1 + 1.5 * 2 + 0.0 * 1) / 4.0, -1)
  assert IC.restate(row, z, "mean", 1, 1, 0.0) == (2.0, -1)
  assert IC.mean_bound(row, z, 1, 1) == 0.0
  assert IC.mean_bound(row, z, 0, 3) == 7 * 2.0**-53 * 3.0 / 4.0


def test_every_case_table_is_complete():
  for nlev in IC.NLEVS:
    kinds = {c[1] for c in IC.cases(nlev)}
    assert kinds == set(IC.KINDS), nlev
    for _, _, row, lo, hi, _ in IC.cases(nlev):
      assert row.shape == (nlev,) and 0 <= lo <= hi < nlev


# ------------------------------------------------------------------ host half of RowIndices
Z = np.linspace(-4000., 0., 41)  # 100 m apart


def _resolve(specs, axes=None):
  from pymoc_amd import indices
  return indices.resolve(specs, dict(Psi=Z, b=Z) if axes is None else axes)


def test_window_resolution():
  from pymoc_amd import indices
  assert indices.window(Z) == (0, 40)
  assert indices.window(Z, zhi=-500.) == (0, 35)
  assert indices.window(Z, zlo=-1000.) == (30, 40)
  assert indices.window(Z, zlo=-1000., zhi=-500.) == (30, 35)
  assert indices.window(Z, zlo=-1049., zhi=-951.) == (30, 30)   # inclusive, one level
  assert indices.window(Z, zlo=-1000., zhi=-1000.) == (30, 30)
  t = _resolve([("a", "max", "Psi", dict(zhi=-500.)), ("b", "at", "b", dict(x0=-1000.)),
                ("c", "cross", "Psi", dict(level=0.5, zlo=-3000., zhi=-500.)),
                ("d", "mean", "b", dict(zlo=-1000.)), ("e", "min", "Psi", None),
                ("f", "cross", "Psi", {})])
  assert t == [("a", "max", "Psi", 0, 35, 0.0), ("b", "at", "b", 0, 40, -1000.0),
               ("c", "cross", "Psi", 10, 35, 0.5), ("d", "mean", "b", 30, 40, 0.0),
               ("e", "min", "Psi", 0, 40, 0.0), ("f", "cross", "Psi", 0, 40, 0.0)]


@pytest.mark.parametrize("specs,axes,match", [
    ([("a", "max", "Psi", dict(zlo=-950., zhi=-910.))], None, "empty window"),
    ([("a", "max", "Psi", dict(zlo=10.))], None, "empty window"),
    ([("a", "at", "Psi", dict(x0=1.))], dict(Psi=np.array([0., 1., 1., 2.])), "strictly increasing"),
    ([("a", "cross", "Psi", {})], dict(Psi=np.array([0., 2., 1.])), "strictly increasing"),
    ([("a", "mean", "Psi", {})], dict(Psi=Z[::-1]), "strictly increasing"),
    ([("a", "median", "Psi", {})], None, "unknown kind"),
    ([("a", "max", "psi", {})], None, "unknown source"),
    ([("a", "max", "Psi", {}), ("a", "min", "Psi", {})], None, "duplicate"),
    ([("i%d" % i, "max", "Psi", {}) for i in range(33)], None, "1 to 32"),
    ([], None, "1 to 32"),
    ([("a", "at", "Psi", {})], None, "needs x0"),
    ([("a", "max", "Psi", dict(x0=1.))], None, "takes zlo, zhi"),
    ([("a", "max", "Psi", dict(zlo=-1.5, zhi=0.5))], dict(Psi=np.array([0., -3., 0.2])), "one run"),
])
def test_resolve_refuses(specs, axes, match):
  with pytest.raises(ValueError, match=match):
    _resolve(specs, axes)


def test_extrema_take_any_axis_and_32_specs_pass():
  t = _resolve([("a", "max", "Psi", {})], dict(Psi=Z[::-1]))  # max / min do not read the axis
  assert t == [("a", "max", "Psi", 0, 40, 0.0)]
  assert len(_resolve([("i%d" % i, "min", "Psi", {}) for i in range(32)])) == 32
