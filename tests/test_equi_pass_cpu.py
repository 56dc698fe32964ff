"""K6 (`k_column_equi_pass`) without a GPU: the NumPy restatement of tests/equi_pass_cases.py
against the C oracle and against an exact (mpmath) evaluation of the recurrence, the reach of
the launch table, mutants of the restatement, and the refusals of `pm_column_equi_pass`."""
import ctypes as C

import numpy as np
import pytest

import equi_pass_cases as T
import oracle as O


def _oracle(c):
  return O.column_equi_pass(c.x, *c.c4, c.bs, c.bbot, c.bzbot if c.use_bzbot else None)


@pytest.mark.parametrize("c", T.CASES, ids=repr)
def test_one_chunk_restatement_is_the_oracle_bitwise(c):
  """K forced to ni: lane 0 composes every interval, the scan has nothing to do, and the
  restatement is the sequential recurrence of `orc_column_equi_pass`: equal bit for bit (y, v,
  rms), on the non-finite rows too (NaN at the same places)."""
  y, rms, nadd, b, bz = c.restate(K=c.ni)
  yo, ro = _oracle(c)
  assert T.same(y, yo) and T.same(rms, ro), c
  assert nadd == int(T.classes(ro, c.tol).sum())
  assert T.same(b, yo[0, c.zidx]) and T.same(bz, yo[1, c.zidx])


@pytest.mark.parametrize("c", T.FINITE, ids=repr)
def test_error_bound_against_exact(c):
  """Every node of every finite row, for the restatement with the kernel's chunking, with one
  chunk, and for the oracle: the association-free bound of equi_pass_cases' docstring on the raw
  (v, S) and, after the boundary conditions, on (Y, V).  The constants are counted, not fitted;
  the measured worst ratios error / bound are in DESIGN.md."""
  e = c.exact()
  g, w = T.elements(c.x, c.c4[0], c.c4[1])
  raw = [T.raw_ratios(e, *T.sweeps(g, w, K)) for K in (None, c.ni)]
  y = T.reference(c.name)[0]
  sc = [T.bound_ratios(e, yy, c.bs, c.bbot, c.bzbot, c.use_bzbot) for yy in (y, _oracle(c)[0])]
  print("K6 bound", c.name, "rho %.3g" % float(e["rho"]), "raw (v, S): chunked %.3g %.3g one chunk "
        "%.3g %.3g; scaled (V, Y): chunked %.3g %.3g oracle %.3g %.3g" % (raw[0] + raw[1] + sc[0] + sc[1]))
  assert max(raw[0] + raw[1] + sc[0] + sc[1]) <= 1.0, (c, raw, sc)


def test_the_table_reaches_what_it_claims():
  by = T.BY_NAME
  nis = {c.ni for c in T.CASES}
  assert {1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 999, 1022, 1023} <= nis
  Ks, empty, full = set(), 0, 0
  for c in T.CASES:
    K, i0, i1 = T.chunks(c.ni)
    Ks.add(K)
    empty += bool((i0 == i1).any())
    full += bool((i0 < i1).all())
    # exactly one lane writes the last node, every node is written once
    assert ((i1 == c.ni) & (i0 < i1)).sum() == 1 and (i1 - i0).sum() == c.ni
  assert {1, 2, 3, 16} <= Ks and empty and full
  K, i0, i1 = T.chunks(65)  # lane 32 holds one interval, lanes 33 .. 63 none
  assert K == 2 and i1[32] - i0[32] == 1 and (i1[33:] == i0[33:]).all()
  # mmax: m itself for m = 67 and 1024 (nz = m, zidx the identity), larger otherwise, not all x 64
  for name in ("m67_full", "m130_full", "m1024_full"):
    c = by[name]
    assert c.nz == c.m and np.array_equal(c.zidx, np.arange(c.m))
  assert by["m67_full"].mmax == 67 and by["m1024_full"].mmax == 1024
  assert all(c.mmax > c.m for c in T.CASES if c.m not in (67, 130, 1024))
  assert by["m130_full"].mmax == 130 and sum(c.mmax % 64 != 0 for c in T.CASES) >= 5
  assert by["m2"].nz == 2 and all(2 <= c.nz <= c.mmax <= 1024 for c in T.CASES)
  # meshes: nested ones reach h_max / h_min >= 2^12; stiffness c h from 1e-6 to O(1)
  for name in ("m65_nested", "m129_nested", "m1023_nested"):
    h = np.diff(by[name].x)
    assert h.max() >= 2.0**12 * h.min()
  ch = {c.name: np.abs(c.c4[0][:-1] * np.diff(c.x)).max() for c in T.FINITE}
  assert ch["m4"] < 2e-6 and ch["m128_uni"] < 2e-6 and 1e-3 < ch["m67_full"] < 5e-2
  assert ch["m130_full"] > 1 and ch["m1024_full"] > 1 and ch["refining"] > 1
  # the g < 0 row: the denominator changes sign, v alternates, S cancels
  c = by["g_negative"]
  g, w = T.elements(c.x, c.c4[0], c.c4[1])
  assert 0 < (g < 0).sum() < g.size
  e = c.exact()
  assert float(abs(e["S"][-1]) / e["A"][-1]) < 0.9 and float(e["rho"]) > 2
  # degenerate rows
  y, rms, nadd, _, _ = T.reference("bs_is_bbot")
  assert (y[1] == 0).all() and (rms == 0).all() and nadd == 0
  assert (y[0][:-1] == by["bs_is_bbot"].bbot).all()
  y = T.reference("overflow")[0]
  k = int(np.argmax(~np.isfinite(y[1])))
  assert 64 < k < by["overflow"].m - 64 and np.isfinite(y[1][:k]).all()
  assert not np.isfinite(y[1][k:]).any() and np.isinf(y[1][k])
  for name in ("nan_wA_z", "nan_table"):
    y, rms, nadd, _, _ = T.reference(name)
    assert np.isnan(y).any() and np.isnan(rms).any(), name
  assert np.isnan(by["nan_wA_z"].wA_z).sum() == 1 and np.isnan(by["nan_table"].wA[1]).sum() == 1
  assert sum(np.isnan(t).sum() for t in by["nan_table"].wA) == 1
  # rows for nadd
  for name, want in (("three_classes", (1, 1, 1)), ("refining", (0, 1, 1)), ("all_class_2", (0, 0, 1))):
    c = by[name]
    cls = T.classes(T.reference(name)[1], c.tol)
    n = np.bincount(cls, minlength=3)
    assert tuple(int(v > 0) for v in n) == want and c.ni > 64, (name, n)
    last = cls[c.ni // 64 * 64:]
    assert 0 < last.size < 64 and (last > 0).any(), name  # a partly filled last ballot trip counts
  assert T.reference("all_class_2")[2] == 2 * by["all_class_2"].ni
  # the batch: 2 ... 1024 nodes, both conditions, both degenerate kinds, inactive first and last
  B = [by[n] for n in T.BATCH]
  assert {2, 3, 4, 1023, 1024} <= {c.m for c in B} and {c.use_bzbot for c in B} == {True, False}
  assert {"overflow", "nan_table", "nan_wA_z"} <= set(T.BATCH) and len(T.BATCH_ACTIVE) == len(B)
  assert T.BATCH_ACTIVE[0] == T.BATCH_ACTIVE[-1] == 0 and sum(T.BATCH_ACTIVE) == len(B) - 2
  assert by[T.POINTER_ROW].use_bzbot and by[T.POINTER_ROW].path == "interp"


@pytest.mark.parametrize("name", T.TOL_ROWS)
def test_tol_rows_have_both_boundaries(name):
  """The rows the GPU file relaunches at tol = rms[k] and 100 tol = rms[k] have such intervals,
  and the restatement moves exactly that interval's class."""
  c = T.BY_NAME[name]
  rms = T.reference(name)[1]
  first, second = T.tol_boundaries(rms, c.tol)
  assert first is not None and second is not None
  k, t = first
  assert T.classes(rms, c.tol)[k] == 1 and T.classes(rms, t)[k] == 0
  assert T.classes(rms, np.nextafter(t, 0.0))[k] == 1
  k, t = second
  assert 100 * t == rms[k] and T.classes(rms, t)[k] == 2
  assert T.classes(rms, t * (1 + 1e-9))[k] == 1
  assert c.restate(tol=t)[2] == int(T.classes(rms, t).sum())


def _catches(mutant):
  """-> {detector: [rows]}: `oracle` (the one-chunk restatement no longer equals the oracle
  bitwise), `bound` (the chunked restatement breaks the bound against exact), `rms` / `nadd` (they
  differ from the unmutated restatement's), `nadd@tol` (they differ at tol = rms[k])."""
  hit = dict(oracle=[], bound=[], rms=[], nadd=[])
  hit["nadd@tol"] = []
  for c in T.CASES:
    y, rms, nadd, _, _ = T.reference(c.name)
    ym, rm, nm, _, _ = c.restate(mutant=mutant)
    y1, r1, _, _, _ = c.restate(K=c.ni, mutant=mutant)
    yo, ro = _oracle(c)
    if not (T.same(y1, yo) and T.same(r1, ro)):
      hit["oracle"].append(c.name)
    if not T.same(rm, rms):
      hit["rms"].append(c.name)
    if nm != nadd:
      hit["nadd"].append(c.name)
    if c.finite and mutant in ("be_cn_i", "scan_gt"):
      e = c.exact()
      g, w = T.elements(c.x, c.c4[0], c.c4[1], mutant)
      if max(T.raw_ratios(e, *T.sweeps(g, w, None, mutant))) > 1.0:
        hit["bound"].append(c.name)
    if c.name in T.TOL_ROWS:
      k, t = T.tol_boundaries(rms, c.tol)[0]
      if c.restate(tol=t, mutant=mutant)[2] != c.restate(tol=t)[2]:
        hit["nadd@tol"].append(c.name)
  return hit


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutants_of_the_restatement_are_caught(mutant):
  """c[2] <-> c[3], `be` from cn[i], the scan guard `lane > d`, 49/90 -> 32/45, `rms >= tol`:
  each breaks an assertion of this file or changes rms / nadd on a row of the table (the GPU
  file holds the device to the unmutated restatement bit for bit)."""
  hit = _catches(mutant)
  print("K6 mutant", mutant, {k: v for k, v in hit.items() if v})
  finite = {c.name for c in T.FINITE}
  if mutant == "scan_gt":  # one chunk has no scan: only the chunked restatement shows it
    # with ni <= 2 lane 1 needs lane 0's map alone, which no scan step has to form
    assert not hit["oracle"] and set(hit["bound"]) == finite - {"m2", "m3"}
  elif mutant == "be_cn_i":  # (bs == bbot: v0 = 0 hides g after the boundary conditions, not before)
    assert set(hit["oracle"]) >= finite - {"bs_is_bbot"} and set(hit["bound"]) == finite
  elif mutant == "swap_c23":
    assert not hit["bound"] and len(hit["oracle"]) >= 10 and hit["rms"] == hit["oracle"]
    assert "three_classes" in hit["nadd"]
  elif mutant == "w_49_90":
    assert len(hit["oracle"]) >= 10 and hit["rms"] == hit["oracle"] and hit["nadd"]
  else:  # rms >= tol: visible only where an rms equals tol
    assert not hit["oracle"] and not hit["rms"] and not hit["nadd"]
    assert hit["nadd@tol"] == list(T.TOL_ROWS)


def test_coefficient_paths_agree():
  """`coefficients` from tables of np.interp values and from wA_z + z: the same four sets (what
  the GPU file asks of the device's own interpolation), and (3/7)**0.5 is the kernel's constant."""
  from pymoc_amd import equilibrium
  assert equilibrium._S37 == T.SQRT_3_7
  for c in T.CASES:
    if c.path == "interp":
      a, w = T.coefficients(c.x, c.Ak, c.dAk, wA=c.wA)
      assert all(T.same(a[s], c.c4[s]) for s in range(4)), c


# ------------------------------------------------------------------ the entry's refusals
def test_entry_refusals():
  """pm_column_equi_pass on descriptors that are wrong in exactly one way: PM_EINVAL and the
  message's key words, before anything is launched (the stand-in pointers are never
  dereferenced); n = 0 is PM_OK with every pointer NULL."""
  from pymoc_amd import _lib
  L = _lib.lib
  A = 0x10000
  PTRS = "m x Ak dAk wA wA_z z bs bbot bzbot flags zidx y rms nadd b bz active".split()

  def desc(**kw):
    d = _lib.pm_column_equi()
    d.n, d.nz, d.mmax, d.reserved, d.tol = 2, 10, 64, 0, 1e-3
    for f in PTRS:
      setattr(d, f, A)
    for k, v in kw.items():
      setattr(d, k, v)
    return d

  def refused(words, **kw):
    d = desc(**kw)
    rc = L.pm_column_equi_pass(C.byref(d), None)
    msg = L.pm_last_error().decode()
    assert rc == _lib.PM_EINVAL and all(w in msg for w in words), (kw, rc, msg)

  assert L.pm_column_equi_pass(None, None) == _lib.PM_EINVAL
  assert "NULL" in L.pm_last_error().decode()
  refused(("shape", "nz=1"), nz=1)
  refused(("shape", "mmax=9"), mmax=9)          # mmax < nz
  refused(("shape", "mmax=1025"), mmax=1025)
  refused(("shape", "n=-1"), n=-1)
  refused(("tol", "positive"), tol=0.0)
  refused(("tol", "positive"), tol=-1e-3)
  refused(("tol", "positive"), tol=float("nan"))
  refused(("b", "zidx"), zidx=None)
  refused(("wA", "wA_z"), wA=None, wA_z=None)
  refused(("wA", "wA_z"), wA=None, wA_z=None, z=None)
  refused(("wA", "wA_z"), wA=None, z=None)      # wA_z without z
  for f in ("m", "x", "Ak", "dAk", "bs", "bbot"):
    refused(("NULL",), **{f: None})
  # nothing to do: no pointer is looked at
  d = _lib.pm_column_equi()
  d.n, d.nz, d.mmax, d.tol = 0, 2, 2, 1e-3
  assert L.pm_column_equi_pass(C.byref(d), None) == _lib.PM_OK
  d.mmax = 1024
  assert L.pm_column_equi_pass(C.byref(d), None) == _lib.PM_OK
