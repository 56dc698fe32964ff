"""The table behind tests/test_column_forcing_gpu.py, checked without a GPU: its coverage, its
shape rule against the library's, and that the inputs can tell a kernel that is wrong from one that
is right."""
import ctypes as C

import numpy as np
import pytest

import column_forcing_cases as T


def test_forcing_table_covers_every_axis_value_and_kernel():
  from pymoc_amd import _lib
  assert len({T.label(c) for c in T.CASES}) == len(T.CASES)
  # the shape rule is the library's: it refuses none of the 24 (lanes, nz) pairs, so none is skipped
  g, p = C.c_int32(0), C.c_int32(0)
  for lanes in T.LANES:
    for nz in T.NZS:
      assert _lib.lib.pm_column_kernel_shape(6, nz, lanes, C.byref(g), C.byref(p)) == _lib.PM_OK
      assert g.value == T.lanes_used(lanes, nz) and p.value == T.levels_per_lane(nz, g.value)
  assert {nz for nz in T.NZS if T.lanes_used(16, nz) != 16} == {129, 257}
  for mod in ("twobasin", "twocol"):
    cases = [c for c in T.CASES if c.mod == mod]
    assert {(c.lanes, c.nz) for c in cases} == {(g, nz) for g in T.LANES for nz in T.NZS}
    assert {c.n for c in cases} == set(T.MEMBERS) and {c.nsteps for c in cases} == set(T.NSTEPS)
    for nz in (17, 100):
      assert {(c.lanes, c.n) for c in cases if c.nz == nz} >= {(g, n) for g in T.LANES for n in T.MEMBERS}
    assert {c.kernel for c in cases} == {"CK_STEPS_DIV3_UA", "CK_STEPS_PLAIN_UA", "CK_STEPS_PLAIN",
                                         "CK_STEPS_CONTRACTED"}
    # CK_STEPS_PLAIN both ways: an Area that varies in z, and more than four levels per lane
    plain = [c for c in cases if c.kernel == "CK_STEPS_PLAIN" and c.lanes == 64]
    assert any(c.variant == "areaz" and c.nz <= 256 for c in plain) and any(c.nz > 256 for c in plain)
    # the forcing entries at counts that are no multiple of 256
    assert {(1, 3), (5, 17), (21, 129)} <= {(c.n, c.nz) for c in cases}
    assert all((n * nz) % 256 for n, nz in ((1, 3), (5, 17), (21, 129)))
  noso = [c for c in T.CASES if c.mod == "twocol_noso"]
  assert {(c.lanes, c.n) for c in noso} == {(g, n) for g in T.LANES for n in T.MEMBERS}
  assert {c.kernel for c in noso} == {"CK_STEPS_DIV3_UA", "CK_STEPS_PLAIN_UA", "CK_STEPS_PLAIN",
                                      "CK_STEPS_CONTRACTED"}


def test_forcing_table_names_the_kernel_the_call_selects():
  """pm_column_kernel_name on a stand-in descriptor with the hints the case's batch will carry
  (the stand-in pointers are never dereferenced)."""
  from pymoc_amd import _lib
  A = 0x10000
  for c in T.CASES:
    d = _lib.pm_columns()
    d.ncols, d.nz, d.nsel = T.groups(c.mod) * c.n, c.nz, 1
    if c.variant != "areaz":
      d.reserved = _lib.PM_COLS_ALL_UNIFORM_AREA | (0 if c.variant == "nodiv3" else _lib.PM_COLS_DIV3_PROVEN)
    d.z = d.b = d.kappa = d.area = d.dAkappa = d.bs = d.bbot = d.bzbot = d.N2min = A
    d.flags = d.ksel = d.nonfinite = A
    two = c.mod == "twobasin"
    ops = _lib.PM_OP_TIMESTEP | (_lib.PM_OP_WA_TWOBASIN if two else _lib.PM_OP_WA_PSI)
    if c.variant == "contracted":
      ops |= _lib.PM_OP_CONTRACTED
    buf = C.create_string_buffer(96)
    rc = _lib.lib.pm_column_kernel_name(C.byref(d), A, A if two else None, c.nsteps, ops, c.lanes, buf, 96)
    assert rc == _lib.PM_OK, _lib.lib.pm_last_error()
    assert buf.value.decode() == T.kernel_name(c), T.label(c)


def test_forcing_inputs_carry_the_proofs_and_properties_the_cases_need():
  from pymoc_amd.columns import div3_proven
  seen = set()
  for c in T.CASES:
    key = (c.mod, c.nz, c.n, c.variant == "areaz")
    if key in seen:
      continue
    seen.add(key)
    inp = T.inputs(*key)
    n, nz, z = c.n, c.nz, inp["z"]
    assert inp["ncols"] == T.groups(c.mod) * n
    assert nz == 2 or np.ptp(np.diff(z)) > 0.1 * np.diff(z).min()  # non-uniform
    assert inp["iso"].shape == (2 * n, nz)
    if c.mod == "twobasin":
      assert inp["zon"].shape == inp["so"].shape == (2 * n, nz)
    elif c.mod == "twocol":
      assert inp["so"].shape == (n, nz)
    else:
      assert "so" not in inp
    for k in ("iso", "zon", "so"):
      if k in inp:
        assert (inp[k][:, 0] == 0).all() and (inp[k][:, -1] == 0).all()
        assert nz == 2 or (np.abs(inp[k][:, 1:-1]) > 0).all()
    assert (inp["do_conv"] == ((np.arange(inp["ncols"]) // n) == 1)).all()
    # the host half of PM_COLS_DIV3_PROVEN (the device half, its reciprocals, is asserted on the GPU)
    if c.variant != "areaz":
      dz = np.diff(z)
      den = np.concatenate([dz, 0.5 * (dz[1:] + dz[:-1]), inp["Area"][:, 0]])
      assert div3_proven(den), key
    assert np.isfinite(T.reference(c)[1]).all()
  # convective adjustment acts in the northern columns of the larger cases
  inp = T.inputs("twobasin", 100, 21)
  quiet = dict(inp, do_conv=np.zeros(inp["ncols"], dtype=bool))
  wA = T.forcing("twobasin", inp)
  a, b = T.step(inp, wA, 4), T.step(quiet, wA, 4)
  assert np.array_equal(a[:21], b[:21]) and (a[21:42] != b[21:42]).any(axis=1).all()


SENSITIVE = [c for c in T.CASES if c.nz >= 3]  # (nz = 2 has no interior level: see below)


def test_sensitivity_cases_cover_every_modifier_and_member_count():
  assert {(c.mod, c.n) for c in SENSITIVE} == {(m, n) for m in T.MODS for n in T.MEMBERS}


@pytest.mark.parametrize("c", SENSITIVE, ids=T.label)
def test_forcing_references_tell_wrong_rows_and_boundaries_apart(c):
  """A kernel that took the Pacific rows from rows [0, n) of the zonal and Psi_SO arrays instead of
  [n, 2n), or that had a group boundary off by one in either direction, gives another result than
  the reference in exactly the columns it gets wrong -- in every case of the table with an interior
  level (the forcing at the top and bottom level never enters a step: nz = 2 cannot tell).  Rows
  [2n, 3n) do not exist in arrays of the drivers' size, so that mistake has no variant of its own
  here: it is the out-of-bounds read the exactly sized device arrays are there for."""
  inp = T.inputs(c.mod, c.nz, c.n, c.variant == "areaz")
  n, ncols = c.n, inp["ncols"]
  wA, ref = T.reference(c)
  right = (n, 2 * n, n) if c.mod == "twobasin" else (n,)
  assert np.array_equal(T.form_by_column(c.mod, inp, *right), wA)
  wrong = {}
  if c.mod == "twobasin":
    wrong["pac_rows"] = ((n, 2 * n, 0), range(2 * n, 3 * n))
    wrong["north_early"] = ((n - 1, 2 * n, n), [n - 1])
    wrong["north_late"] = ((n + 1, 2 * n, n), [n])
    wrong["pac_early"] = ((n, 2 * n - 1, n - 1), [2 * n - 1])
    wrong["pac_late"] = ((n, 2 * n + 1, n + 1), [2 * n])
  else:
    wrong["north_early"] = ((n - 1,), [n - 1])
    wrong["north_late"] = ((n + 1,), [n])
  for name, (args, cols) in wrong.items():
    got = T.step(inp, T.form_by_column(c.mod, inp, *args), c.nsteps)
    cols = list(cols)
    rest = np.setdiff1d(np.arange(ncols), cols)
    assert np.array_equal(got[rest], ref[rest]), name
    assert (got[cols] != ref[cols]).any(axis=1).all(), name


def test_planted_members_leave_the_window_through_the_forcing():
  for mod in T.MODS:
    base = T.inputs(mod, 100, 21)
    inp, cols = T.planted(mod, base)
    wA = T.forcing(mod, inp)
    a = np.abs(wA)
    with np.errstate(invalid="ignore"):
      outside = ~((a == 0) | ((a >= 2.0**-200) & (a <= 2.0**200)))
    hit = np.nonzero(outside.any(axis=1))[0]
    assert set(hit) <= set(cols) and len(hit) >= len(cols) - 2
    assert np.isfinite(wA[3]).all() and np.isinf(wA).any() == (mod != "twocol_noso") and np.isnan(wA).any()
    # the state alone is inside the window but for the two scaled columns
    b = np.abs(inp["b0"])
    small = np.nonzero((b < 2.0**-200).any(axis=1))[0]
    assert len(small) == 2 and set(small) <= set(cols) and not set(small) & set(hit)
    assert np.isfinite(inp["b0"]).all()
