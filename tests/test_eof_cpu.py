"""pm_series_scatter / pm_series_eof / pm_series_project and SeriesEOF without a device: the
restatement (tests/eof_cases.py) against an extended-precision power iteration and against
np.linalg.eigh within a derived bound; what the principal component gains over the best single
index; the header mirrors, every argument check of the entries and of the class, and the kernels'
scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eof_cases as EC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

CASES = EC.cases()
U = 2.0 ** -53
C_BOUND = 8.0


def test_table_holds_what_it_must():
  """Every shape, content and unit the definition can go wrong at is in the table."""
  ns, qs, Ks, its = (set(f(c) for c in CASES) for f in (
      lambda c: c["v"].shape[2], lambda c: len(c["sel"]), lambda c: c["k1"] - c["k0"],
      lambda c: c["iters"]))
  assert ns == {1, 5, 33, 37, 70} and qs == {1, 2, 7, 32} and Ks == {2, 3, 65, 257}
  assert its == {1, 64, 1024}
  for c in CASES:
    assert c["v"].shape[1] == len(c["sel"]) + 3 and len(set(c["sel"].tolist())) == len(c["sel"])
    assert (c["sel"] != np.sort(c["sel"])).any() or len(c["sel"]) == 1
    assert c["k0"] > 0 and c["k1"] < c["v"].shape[0]
  c = CASES[0]
  r = EC.restate(c)
  by = {EC.style_of(m): m for m in range(len(EC.STYLES))}
  assert r["nused"][by["zero_used"]] == 0 and r["nused"][by["one_used"]] == 1
  assert r["nused"][by["all_nan"]] == 0 and 2 <= r["nused"][by["scattered"]] < 65
  assert 2 <= r["nused"][by["one_index"]] < 65
  assert r["trace"][by["constant"]] == 0.0 and np.isnan(r["lam"][by["constant"]])
  assert r["trace"][by["zeros"]] == 0.0 and np.signbit(c["v"][c["k0"]:c["k1"], c["sel"], by["zeros"]]).any()
  assert np.isinf(r["trace"][by["huge"]]) and np.isnan(r["eof"][:, by["huge"]]).all()
  assert 0.0 < r["lam"][by["tiny"]] < 1e-290 and 1e290 < r["lam"][by["big"]] < np.inf
  assert r["resid"][by["degenerate"]] > 1e-6 > r["resid"][by["modes"]]
  cp = by["copies"]
  assert r["eof"][0, cp] == r["eof"][1, cp] and np.isfinite(r["lam"][cp])
  assert np.isnan(r["pc"][:, 0, by["one_used"]]).all() and np.isnan(r["mean"][:, by["one_used"]]).all()
  assert (r["eof"].max(axis=0)[np.isfinite(r["lam"])] == 1.0).all()
  g = [c for c in CASES if c["order"] is not None][0]
  rg = EC.restate(g)
  assert sorted(np.diff(g["start"]).tolist()) == [1, 2, 27, 40] and (rg["ntot"] == 0).sum() == 1
  assert len(set(g["labels"].tolist())) == 4 and (np.diff(g["labels"]) != 0).sum() > 10
  z = [c for c in CASES if c["w"] is not None and (c["w"] == 0.0).any()]
  assert z and all((EC.restate(c)["eof"][min(1, len(c["sel"]) - 1)][np.isfinite(EC.restate(c)["lam"])] == 0.0).all()
                   for c in z[:1])


# ------------------------------------------------------------------ the bound
def bound(Cm, iters):
  """C_BOUND q 2^-53 lambda1 / (lambda1 - lambda2) + (lambda2 / lambda1)^iters for the symmetric
  matrix Cm (DESIGN.md section 29 derives C_BOUND = 8), for the largest-loading-1 eigenvector in
  the max norm and for lam relative to lambda1."""
  ev = np.linalg.eigvalsh(Cm)
  l1, l2 = ev[-1], max(ev[-2], 0.0) if ev.size > 1 else 0.0
  return C_BOUND * Cm.shape[0] * U * l1 / (l1 - l2) + (l2 / l1) ** iters


def _matrices():
  """Covariances with lambda2 / lambda1 <= 0.5 through the restated scatter: q = 2, 7, 8, 32, one
  shared mode with mixed-sign loadings plus weaker independent noise, 12 members each."""
  out = []
  for q, seed in ((2, 0), (7, 1), (8, 2), (32, 3)):
    rng = np.random.default_rng(seed)
    K, n = 200, 12
    load = np.linspace(1.0, 0.3, q) * np.where(np.arange(q) % 3 == 2, -1.0, 1.0)
    v = (rng.standard_normal((K, 1, n)) * 2.0 * load[None, :, None]
         + 0.5 * rng.standard_normal((K, q, n)))
    sc = EC.scatter(v, 0, K, range(q))
    out.append((q, sc))
  return out


def _ld_power(Cm, iters=4096):
  """The largest-loading-1 eigenvector and the Rayleigh quotient of Cm by power iteration in
  np.longdouble from the definition's start."""
  L = np.longdouble
  A = Cm.astype(L)
  y = A[:, int(np.argmax(np.diag(Cm)))].copy()
  for _ in range(iters + 1):
    vec = y / y[int(np.argmax(np.abs(y)))]
    y = A @ vec
  return vec, (vec @ y) / (vec @ vec)


def test_restatement_against_extended_precision_and_eigh():
  """The restated eof (64 iterations) lies within bound() of the np.longdouble power iteration of
  4096 iterations on the same float64 covariance, in the max norm; lam within bound() of both its
  Rayleigh quotient and np.linalg.eigh's largest eigenvalue, relative to it.  The premises of the
  derivation are asserted per matrix: lambda2 / lambda1 <= 0.5 and ||C||_inf <= 2 lambda1.
  Observed (one run): the largest fraction of the bound 0.041 (eof), 0.10 (lam)."""
  worst_v = worst_l = 0.0
  seen = 0
  for q, sc in _matrices():
    r = EC.eof(sc["nused"], sc["scat"], q, 64)
    I_, J_ = EC.tri(q)
    for m in range(sc["nused"].size):
      Cm = np.zeros((q, q))
      Cm[I_, J_] = Cm[J_, I_] = sc["scat"][:, m] / np.float64(sc["nused"][m])
      ev = np.linalg.eigvalsh(Cm)
      assert ev[-2] / ev[-1] <= 0.5 and np.abs(Cm).sum(axis=1).max() <= 2.0 * ev[-1]
      b = bound(Cm, 64)
      vec, ray = _ld_power(Cm)
      fv = float(np.abs(r["eof"][:, m].astype(np.longdouble) - vec).max()) / b
      fl = max(abs(float((np.longdouble(r["lam"][m]) - ray) / ray)),
               abs(r["lam"][m] - ev[-1]) / ev[-1]) / b
      assert fv <= 1.0 and fl <= 1.0, (q, m, fv, fl)
      assert r["resid"][m] <= b
      worst_v, worst_l, seen = max(worst_v, fv), max(worst_l, fl), seen + 1
  assert seen == 48
  print("largest fraction of the bound: eof %.3g, lam %.3g" % (worst_v, worst_l))


# ------------------------------------------------------------------ the gain
def _ramped(rng, K, q, n):
  """[K, q, n]: one shared mode of unit variance whose AR coefficient ramps 0.1 -> 0.9, loading 1
  on every index, plus independent AR(0.3) noise of 1.5 sd per index."""
  phi = np.linspace(0.1, 0.9, K)
  z = rng.standard_normal(n)
  e = 1.5 * rng.standard_normal((q, n))
  v = np.empty((K, q, n))
  for k in range(K):
    z = phi[k] * z + np.sqrt(1.0 - phi[k] ** 2) * rng.standard_normal(n)
    e = 0.3 * e + 1.5 * np.sqrt(1.0 - 0.09) * rng.standard_normal((q, n))
    v[k] = z[None, :] + e
  return v


def test_the_principal_component_is_no_worse_than_the_best_index():
  """100 series of 600 records x 8 indices, seed 0 (chosen before looking), ac at W = 150, S = 10,
  linear detrending: the number of series with Kendall tau of ac above 0.5 is no smaller for pc1
  than for the index with the largest loading of the same series.  Observed: 97 (pc1) against 52
  (best index)."""
  K, q, n, W, S = 600, 8, 100, 150, 10
  v = _ramped(np.random.default_rng(0), K, q, n)
  c = dict(v=v, k0=0, k1=K, sel=np.arange(q), w=None, iters=64, order=None, start=None)
  r = EC.restate(c)
  assert np.isfinite(r["pc"]).all()
  best = r["eof"].argmax(axis=0)
  single = v[np.arange(K)[:, None], best[None, :], np.arange(n)[None, :]][:, None, :]
  counts = []
  for series in (r["pc"], single):
    ac = WC.windows(series, 0, K, W, S, 1, "linear")["out"][3]
    k = WC.kendall(ac, 0, ac.shape[0])
    counts.append(int((WC.tau_b(k[0][0], k[1][0], k[2][0]) > 0.5).sum()))
  print("tau(ac) > 0.5: %d of %d for pc1, %d for the best single index" % (counts[0], n, counts[1]))
  assert counts[0] >= counts[1], counts


# ------------------------------------------------------------------ the C-ABI
def test_layouts_match_the_header(tmp_path):
  from pymoc_amd import _lib
  for name in ("pm_series_scatter", "pm_series_eof", "pm_series_project"):
    cls = getattr(_lib, name)
    vals = _layout(tmp_path, name, cls._fields_)
    assert vals[0] == C.sizeof(cls), name
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_], name
    assert _lib.SIGNATURES[name][1][0] is C.POINTER(cls)
  assert (_lib.PM_EOF_Q_MAX, _lib.PM_EOF_ITERS_MAX) == (EC.Q_MAX, EC.ITERS_MAX)
  assert _lib.PM_EOF_Q_MAX == _lib.PM_INDICES_MAX
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  for name in ("PM_EOF_Q_MAX", "PM_EOF_ITERS_MAX"):
    assert re.search(r"#define %s %d\b" % (name, getattr(_lib, name)), text), name


def _set(d, kw):
  for k, val in kw.items():
    if k == "sel":
      for j, s in enumerate(val):
        d.sel[j] = s
    else:
      setattr(d, k, val)
  return d


def sdesc(**kw):
  """A valid pm_series_scatter descriptor (the device addresses are stand-ins) with the edits."""
  from pymoc_amd import _lib
  d = _lib.pm_series_scatter()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.q, d.v, d.w = 10, 6, 60, 1, 50, 3, FAKE, FAKE + 8
  return _set(_set(d, dict(sel=(4, 0, 2))), kw)


START = np.array([0, 4, 4, 10], dtype=np.int32)


def edesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_eof()
  d.n, d.q, d.nu, d.iters, d.nused, d.scat = 10, 3, 3, 64, FAKE, FAKE + 8
  d.order, d.start, d.start_dev = FAKE + 16, START.ctypes.data, FAKE + 24
  return _set(d, kw)


def pdesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_project()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.q, d.nu = 10, 6, 60, 1, 50, 3, 3
  d.v, d.w, d.nused, d.mean, d.eof, d.unit = (FAKE + 8 * i for i in range(6))
  return _set(_set(d, dict(sel=(4, 0, 2))), kw)


def _common():
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)),
          ("k0 > k1", dict(k0=40, k1=20)), ("k1 > nrec", dict(k1=61)), ("K 1", dict(k0=49)),
          ("q 0", dict(q=0)), ("q -1", dict(q=-1)), ("q 33", dict(q=33, nspec=40)),
          ("sel -1", dict(sel=(4, -1, 2))), ("sel nspec", dict(sel=(4, 6, 2))),
          ("sel twice", dict(sel=(4, 0, 4))), ("sel twice adjacent", dict(sel=(2, 2, 0))),
          ("v", dict(v=None))]


def bad_scatter():
  return _common()


def bad_eof():
  bad = lambda *a: np.array(a, dtype=np.int32)
  starts = [("start[0]", bad(1, 4, 4, 10)), ("start[nu]", bad(0, 4, 4, 9)),
            ("start falls", bad(0, 5, 4, 10)), ("start beyond n", bad(0, 4, 11, 10))]
  edesc.keep = [s for _, s in starts] + [np.array([0, 9000], dtype=np.int32)]
  return ([("n 0", dict(n=0)), ("nu 0", dict(nu=0)), ("nu > n", dict(nu=11)), ("q 0", dict(q=0)),
           ("q 33", dict(q=33)), ("iters 0", dict(iters=0)), ("iters -1", dict(iters=-1)),
           ("iters 1025", dict(iters=1025)), ("nused", dict(nused=None)), ("scat", dict(scat=None)),
           ("order alone NULL", dict(order=None)), ("start alone NULL", dict(start=None)),
           ("start_dev alone NULL", dict(start_dev=None)),
           ("no units but nu != n", dict(order=None, start=None, start_dev=None)),
           ("a unit of 9000", dict(n=9000, nu=1, start=edesc.keep[-1].ctypes.data))]
          + [(label, dict(start=s.ctypes.data)) for label, s in starts])


def bad_project():
  return _common() + [("nu 0", dict(nu=0)), ("nu > n", dict(nu=11)),
                      ("unit NULL but nu != n", dict(unit=None)), ("nused", dict(nused=None)),
                      ("mean", dict(mean=None)), ("eof", dict(eof=None)),
                      ("tiles * chunks", dict(n=2**31 - 1, nrec=2**29, k0=0, k1=2**29))]


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  o = [FAKE + 64 * i for i in range(1, 8)]
  assert L.pm_series_scatter(None, *o[:3], None) == _lib.PM_EINVAL
  assert L.pm_series_eof(None, *o[:6], None) == _lib.PM_EINVAL
  assert L.pm_series_project(None, o[0], None) == _lib.PM_EINVAL
  for label, kw in bad_scatter():
    assert L.pm_series_scatter(C.byref(sdesc(**kw)), *o[:3], None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  for label, kw in bad_eof():
    assert L.pm_series_eof(C.byref(edesc(**kw)), *o[:6], None) == _lib.PM_EINVAL, label
  for label, kw in bad_project():
    assert L.pm_series_project(C.byref(pdesc(**kw)), o[0], None) == _lib.PM_EINVAL, label
  for i in range(3):
    args = list(o[:3])
    args[i] = None
    assert L.pm_series_scatter(C.byref(sdesc()), *args, None) == _lib.PM_EINVAL
  for i in range(6):
    args = list(o[:6])
    args[i] = None
    assert L.pm_series_eof(C.byref(edesc()), *args, None) == _lib.PM_EINVAL
  assert L.pm_series_project(C.byref(pdesc()), None, None) == _lib.PM_EINVAL
  assert "pc is NULL" in L.pm_last_error().decode()
  for fn, d, args, word in (
      (L.pm_series_scatter, sdesc(sel=(4, 0, 4)), o[:3], "sel[0] = sel[2] = 4"),
      (L.pm_series_scatter, sdesc(k0=49), o[:3], "fewer than 2 records"),
      (L.pm_series_eof, edesc(iters=1025), o[:6], "iters 1025 outside [1, 1024]"),
      (L.pm_series_project, pdesc(**dict(bad_project())["tiles * chunks"]), o[:1],
       "member tiles * record chunks")):
    assert fn(C.byref(d), *args, None) == _lib.PM_EINVAL
    assert word in L.pm_last_error().decode(), (word, L.pm_last_error())


def test_kernels_cross_compile_without_scratch(tmp_path):
  """All nine instantiations of csrc/eof.hip for gfx950: 0 bytes of scratch, no static LDS
  (DESIGN.md section 29 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "eof.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "eof.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = set(re.findall(r"Function Name: (\S*k_series_(?:scatter|eof|project)\S*)", p.stdout))
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout)]
  assert len(names) == 9 and len(scratch) >= 9
  assert all(x == 0 for x in scratch + lds), list(zip(sorted(names), scratch, lds))


# ------------------------------------------------------------------ the class
def test_series_eof_validates_before_any_device_array():
  """Every refusal is a ValueError raised on the host at construction: none reaches a device
  call, which on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesEOF
  names = ["i%d" % s for s in range(6)]
  src = (_Series((400, 6, 10)), names)
  labels = np.arange(10) % 3
  se = SeriesEOF(src)
  assert se.indices == names and se.q == 6 and se.nu == 10 and se.iters == 64 and not se.pooled
  se = SeriesEOF(src, indices=["i4", "i0"], scale=[1.0, -2.0], groups=labels * 7, pooled=True,
                 iters=np.int64(1024))
  assert se._sel == [4, 0] and se.nu == 3 and se.labels.tolist() == [0, 7, 14]
  assert se.unit.tolist() == labels.tolist() and se._w_host.shape == (2, 10)
  assert SeriesEOF(src, indices="i3").q == 1
  assert SeriesEOF(src, indices=["i1", "i2"], scale=np.ones((2, 10))).scale == "weights"
  assert SeriesEOF(src, scale="std").scale == "std"
  many = (_Series((40, 33, 4)), ["j%d" % s for s in range(33)])
  assert SeriesEOF(many, indices=many[1][:32]).q == 32
  for kw, word in ((dict(indices=[]), "1 to 32 indices"), (dict(indices=["i1", "nope"]), "unknown index"),
                   (dict(indices=["i1", "i1"]), "distinct"), (dict(iters=0), r"\[1, 1024\]"),
                   (dict(iters=1025), r"\[1, 1024\]"), (dict(iters=64.0), "integer"),
                   (dict(iters=True), "integer"), (dict(scale="unit"), "'none', 'std'"),
                   (dict(scale=[1.0, 2.0]), "shape"), (dict(scale=np.ones((6, 9))), "shape"),
                   (dict(scale=[1.0, np.nan, 1.0, 1.0, 1.0, 1.0]), "finite"),
                   (dict(scale=[1.0, np.inf, 1.0, 1.0, 1.0, 1.0]), "finite"),
                   (dict(scale=["a"] * 6), "array of weights"),
                   (dict(pooled=True), "needs groups"), (dict(pooled=1), "True or False"),
                   (dict(groups=labels), "pooled=True only"),
                   (dict(groups=labels[:9], pooled=True), "one per member"),
                   (dict(groups=labels * 0.5, pooled=True), "integer labels")):
    with pytest.raises(ValueError, match=word):
      SeriesEOF(src, **kw)
  with pytest.raises(ValueError, match="1 to 32 indices"):
    SeriesEOF(many)
  with pytest.raises(ValueError, match="float64 device array"):
    SeriesEOF((_Series((400, 6)), names))
  with pytest.raises(ValueError, match="not inside"):
    SeriesEOF(src).fit(0, 401)
  with pytest.raises(ValueError, match="fewer than 2 records"):
    SeriesEOF(src).pc(5, 6)


def test_std_weights():
  from pymoc_amd.eof import std_weights
  var = np.array([[4.0, 0.0, np.nan, 16.0, np.inf], [1.0, 1.0, 1.0, 0.25, 4.0]])
  w = std_weights(var)
  assert w.tolist() == [[0.5, 0.0, 0.0, 0.25, 0.0], [1.0, 1.0, 1.0, 2.0, 0.5]]
  order, start = EC.order_of([1, 0, 1, 0, 0])
  wp = std_weights(var, order, start)
  # unit 0 = members 1, 3, 4 (finite vars 0, 16 -> 8), unit 1 = members 0, 2 (4 alone)
  assert wp[0].tolist() == [0.5, 1.0 / np.sqrt(8.0), 0.5, 1.0 / np.sqrt(8.0), 1.0 / np.sqrt(8.0)]
  assert wp[1].tolist() == [1.0, 1.0 / np.sqrt(1.75), 1.0, 1.0 / np.sqrt(1.75), 1.0 / np.sqrt(1.75)]
