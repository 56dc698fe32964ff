"""Overturning sections without a GPU: fixture G24's integrity, the host helper that builds the
section's rows, and pm_overturning_sections' argument checks (none reaches a launch)."""
import ctypes

import numpy as np
import pytest

import overturning_cases as OC


@pytest.fixture(scope="module")
def G():
  return OC.load()


def test_fixture_integrity(G):
  names = OC.names(G)
  assert len(names) == len(set(names)) == 16
  assert names[:2] == ["g7_nz81", "g7_nz200"]
  assert sum(c.startswith("c5_long_") for c in names) == 6
  assert sum(c.startswith("c5_") and not c.startswith("c5_long_") for c in names) == 8
  assert str(G["numpy_version"]) and str(G["scipy_version"])
  assert [str(f) for f in G["section_fields"]] == ["psiarray_z", "psiarray_res", "psiarray_b", "bnew"]
  nonzero = total = 0
  for c in names:
    k = OC.case(G, c)
    nz, ny, lev = k["nz"], k["ny"], k["levels"]
    nrows = ny + OC.N_BASIN + OC.N_NORTH
    assert k["full"] == c.startswith("g7_")
    assert lev[0] == 0 and lev[-1] == nz - 1 and np.all(np.diff(lev) > 0) and np.diff(lev).max() <= 10
    assert np.isfinite(k["b_basin"]).all() and np.all(np.diff(k["b_basin"]) >= 0), c
    for f in ("psiarray_z", "psiarray_b", "psiarray_res", "bnew"):
      assert k[f].shape == (nrows, lev.size) and np.isfinite(k[f]).all(), (c, f)
    for f in ("Psi", "Psi_SO", "psibz1", "b_basin", "b_north"):
      assert k[f].shape == (nz,) and np.isfinite(k[f]).all(), (c, f)
    assert k["bgrid"].shape == k["psib"].shape == (k["nb"],) and k["nb"] == 500
    assert k["bs_SO"].shape == (ny,) and k["ynew"].shape == (nrows,)
    # what the script fixes by construction
    assert not k["psiarray_z"][0].any() and not k["psiarray_b"][0].any()
    assert not k["psiarray_res"][0].any() and not k["psiarray_res"][-1].any()
    assert np.array_equal(k["psiarray_z"][1:ny], k["psiarray_res"][1:ny])
    assert np.array_equal(k["psiarray_b"][ny:ny + 60], k["psiarray_res"][ny:ny + 60])
    assert np.array_equal(k["bnew"][ny:ny + 60], np.tile(k["b_basin"][lev], (60, 1)))
    if k["full"]:
      nonzero += np.count_nonzero(k["psiarray_b"])
      total += k["psiarray_b"].size
  assert nonzero > 0.8 * total  # the isopycnal masks are exercised


def test_row_helper_equals_the_scripts_rows(G):
  from pymoc_amd.overturning import section_rows
  for c in OC.names(G):
    k = OC.case(G, c)
    r = section_rows(k["y"])
    assert np.array_equal(r["ynew"], k["ynew"]), c
    lchannel, lbasin, lnorth = k["lengths"]
    assert (r["lchannel"], r["lbasin"], r["lnorth"]) == (lchannel, lbasin, lnorth)
    assert np.array_equal(r["c1"], k["ynew"] - lchannel)
    assert np.array_equal(r["c2"], lchannel + lbasin - k["ynew"])
    assert np.array_equal(r["c3"], lchannel + lbasin + lnorth - k["ynew"])
    for a in (r["c1"], r["c2"], r["c3"]):
      assert a.dtype == np.float64 and a.shape == k["ynew"].shape
    ynorth = k["ynew"][-10:]
    assert np.array_equal(r["y_north"], ynorth * 1000. - ynorth[0] * 1000.)


def test_default_row_count():
  from pymoc_amd.overturning import section_rows
  y = np.linspace(0., 2e6, 51)
  assert section_rows(y)["ynew"].size == 51 + 60 + 10
  r = section_rows(y, lbasin_km=8000., lnorth_km=500., n_basin=7, n_north=3)
  assert r["ynew"].size == 51 + 7 + 3
  assert r["ynew"][-1] == 2000. + 8000. + 500. and r["c3"][-1] == 0.


def test_cabi_rejects_bad_descriptors_before_touching_the_device():
  """pm_overturning_sections against descriptors wrong in exactly one way; the stand-in pointers
  are never dereferenced (a row is refused, or returns before any launch on an empty batch)."""
  from pymoc_amd import _lib
  L = _lib.lib
  A = 0x10000
  ROWS = "b_basin bs_SO Psi Psi_SO bgrid psib psibz1 bsouth bnorth".split()

  def desc(**kw):
    d = _lib.pm_overturning()
    d.n, d.nz, d.ny, d.nb, d.n_basin, d.n_north = 2, 200, 51, 500, 60, 10
    for r in ROWS:
      getattr(d, r).ptr = A
    d.c1 = d.c2 = d.c3 = A
    d.lbasin, d.lnorth = 12000., 1000.
    for k, v in kw.items():
      obj, leaf = d, k
      if "__" in k:
        head, leaf = k.split("__")
        obj = getattr(d, head)
      setattr(obj, leaf, v)
    return d

  def call(d):
    rc = L.pm_overturning_sections(ctypes.byref(d), None)
    return rc, L.pm_last_error().decode()

  bad = [(dict(n=-1), "n=-1"), (dict(nz=1), "nz=1"), (dict(nz=1025), "nz=1025"),
         (dict(ny=1), "ny=1"), (dict(ny=1025), "ny=1025"), (dict(nb=0), "nb=0"),
         (dict(nb=2049), "nb=2049"), (dict(n_basin=0), "n_basin=0"), (dict(n_north=0), "n_north=0"),
         (dict(n_basin=1000, n_north=25), "n_basin=1000"), (dict(n=0, nb=2049), "nb=2049"),
         (dict(b_basin__offset=-1), "negative"), (dict(bnorth__stride=-8), "negative"),
         (dict(c2=None), "NULL")] + [({r + "__ptr": None}, "NULL") for r in ROWS]
  for kw, word in bad:
    rc, msg = call(desc(**kw))
    assert rc == _lib.PM_EINVAL and word in msg, (kw, rc, msg)
  assert L.pm_overturning_sections(None, None) == _lib.PM_EINVAL
  # an empty batch is fine at the limits, pointers may be NULL
  empty = desc(n=0, nz=1024, ny=1024, nb=2048, n_basin=1000, n_north=24, c1=None)
  for r in ROWS:
    getattr(empty, r).ptr = None
  assert call(empty)[0] == _lib.PM_OK
