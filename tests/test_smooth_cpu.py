"""SeriesSmooth, the "gaussian" detrend of SeriesWindows and SeriesSurrogates, and pm_series_smooth
without a device: the restatement (tests/smooth_cases.py) against an extended-precision evaluation
within the bound DESIGN.md section 24 derives, against scipy.ndimage.gaussian_filter1d, its
properties and invariances, mutants of it, the header mirror, every argument check of the entry
and of the classes, the kernel's scratch, the tile rule, and the calibration and the power of the
restated pipeline."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import smooth_cases as SC
import surrogate_cases as SGC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

U = 2.0 ** -53
CASES = SC.cases()
IDS = [c["name"] for c in CASES]


def _finite_max(a, axis=0):
  """max |a| over the finite values along `axis`; 0 where there is none."""
  a = np.where(np.isfinite(a), np.abs(a), 0.0)
  return a.max(axis=axis)


def reference(v, k0, k1, w):
  """The definition in np.longdouble, record by record, written without the restatement's walk:
  dict(trend, resid, B [K, nspec, n]) -- B = b (1 + b) X with b = (2 n_t + 2) u, n_t = hi - lo + 1
  and X = max |x_i| over the finite records in reach: the bound on |trend - reference| and on
  |resid - reference|."""
  x = np.asarray(v, dtype=np.float64)[k0:k1]
  K, H = x.shape[0], len(w) - 1
  fin = np.isfinite(x)
  xl = np.where(fin, x, 0.0).astype(np.longdouble)
  wl = np.asarray(w, dtype=np.longdouble)
  trend, B = np.empty(x.shape, dtype=np.longdouble), np.empty(x.shape)
  with np.errstate(all="ignore"):
    for j in range(K):
      lo, hi = max(0, j - H), min(K - 1, j + H)
      wj = wl[np.abs(np.arange(lo, hi + 1) - j)][:, None, None]
      num = (wj * xl[lo:hi + 1]).sum(axis=0)
      den = (wj * fin[lo:hi + 1]).sum(axis=0)
      trend[j] = num / den
      b = (2.0 * (hi - lo + 1) + 2.0) * U
      B[j] = b * (1.0 + b) * _finite_max(x[lo:hi + 1])
    resid = np.where(fin, xl - trend, np.nan)
  return dict(trend=trend, resid=resid, B=B)


def _fraction(got, ref, B):
  """The largest |got - ref| / B over the entries where the reference is a number; the NaN
  patterns agree; B == 0 (nothing but zeros in reach): equal."""
  nan = np.isnan(ref.astype(np.float64))
  if not np.array_equal(np.isnan(got), nan):
    return np.inf
  err = np.abs(got.astype(np.longdouble) - ref)[~nan].astype(np.float64)
  B = B[~nan]
  if (err[B == 0] != 0).any():
    return np.inf
  return float((err[B > 0] / B[B > 0]).max()) if (B > 0).any() else 0.0


def _within_bound(c, mutant=None):
  got = SC.smooth(c["v"], c["k0"], c["k1"], c["w"], mutant=mutant)
  ref = reference(c["v"], c["k0"], c["k1"], c["w"])
  return max(_fraction(got[key], ref[key], ref["B"]) for key in ("trend", "resid"))


@pytest.fixture(scope="module")
def fractions():
  """name -> the largest observed fraction of the bound: computed once per case."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = _within_bound(c)
    return cache[c["name"]]
  return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_within_the_derived_bound_of_longdouble(fractions, case):
  """|trend - reference| and |resid - reference| <= b (1 + b) X, b = (2 n_t + 2) u.  The largest
  observed fraction over the table is 0.40 (at H = 1, where n_t = 3); it falls with n_t, as the
  rounding errors of a long sum do not all point one way."""
  assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps  # (an extended type is needed)
  frac = fractions(case)
  print("%s: largest |restatement - longdouble| / bound = %.4f" % (case["name"], frac))
  assert frac <= 1.0, frac


INTERIOR = [c for c in CASES if c["K"] > 2 * c["H"]]


@pytest.mark.parametrize("case", INTERIOR, ids=[c["name"] for c in INTERIOR])
def test_interior_records_agree_with_scipy(case):
  """H <= j < K - H of the finite styles: within twice the bound of gaussian_filter1d (whose
  weights are normalised first and summed in another order)."""
  from scipy.ndimage import gaussian_filter1d
  c = case
  K, H = c["K"], c["H"]
  got = SC.restate(c)["trend"]
  ref = reference(c["v"], c["k0"], c["k1"], c["w"])
  worst, seen = 0.0, 0
  for s in range(c["nspec"]):
    for m in range(c["n"]):
      if SC.style_of(s, m, c["off"]) not in SC.FINITE_STYLES:
        continue
      x = c["v"][c["k0"]:c["k1"], s, m]
      want = gaussian_filter1d(x, c["sigma"], truncate=c["truncate"])[H:K - H]
      err, B = np.abs(got[H:K - H, s, m] - want), 2.0 * ref["B"][H:K - H, s, m]
      assert (err[B == 0] == 0).all()
      if (B > 0).any():
        worst = max(worst, float((err[B > 0] / B[B > 0]).max()))
      seen += 1
  print("%s: %d finite series, largest |restatement - scipy| / (2 bound) = %.4f"
        % (c["name"], seen, worst))
  assert worst <= 1.0, worst


def test_table_holds_what_it_must():
  assert [SC.half_of(g[3], g[4]) for g in SC.GEOMETRIES[:6]] == [8, 1, 80, 40, 4095, 1]
  assert SC.GEOMETRIES[:6] == ((5, 2, 37, 2.0, 4.0), (70, 1, 64, 0.3, 4.0), (33, 3, 200, 20.0, 4.0),
                               (9, 2, 12, 10.0, 4.0), (4, 1, 4096, 1023.75, 4.0), (1, 1, 5, 1.0, 1.0))
  assert SC.STYLES[:9] == WC.STYLES and SC.STYLES[9:] == ("allnan", "gap", "edge_nan")
  seen, gap_nan = set(), False
  for c in CASES:
    assert c["k0"] > 0 and c["k1"] < c["v"].shape[0]
    out = c["v"][np.r_[0:c["k0"], c["k1"]:c["v"].shape[0]]]
    assert np.isnan(out).any() and (out == 1e300).any() and (np.isnan(out) | (out == 1e300)).all()
    assert c["w"][0] == 1.0 and (np.diff(c["w"]) <= 0).all() and (c["w"] > 0).all()
    r = SC.restate(c)
    for s in range(c["nspec"]):
      for m in range(c["n"]):
        st = SC.style_of(s, m, c["off"])
        seen.add(st)
        x = c["v"][c["k0"]:c["k1"], s, m]
        assert r["nbad"][s, m] == (~np.isfinite(x)).sum()
        assert np.array_equal(np.isnan(r["resid"][:, s, m]), ~np.isfinite(x))
        if st == "allnan":
          assert np.isnan(r["trend"][:, s, m]).all() and r["nbad"][s, m] == c["K"]
        if st == "gap" and c["K"] > 2 * c["H"] + 4:
          t = r["trend"][:, s, m]
          gap_nan |= bool(np.isnan(t[c["H"] + 1]) and np.isfinite(t[1]))
        if st == "edge_nan":
          assert np.isfinite(r["trend"][[0, -1], s, m]).all()  # gap-filled from the neighbours
          assert np.isnan(r["resid"][[0, -1], s, m]).all()
  assert seen == set(SC.STYLES) and gap_nan


# ------------------------------------------------------------------ properties
def test_a_constant_and_a_ramp_are_reproduced():
  """A constant series: trend equals it within the bound, so resid is rounding alone.  A linear
  ramp: reproduced in the interior (the kernel is symmetric there) within the bound."""
  K, sigma = 120, 6.0
  w, H = SC.weights(sigma), SC.half_of(sigma)
  v = np.empty((K, 1, 3))
  v[:, 0, 0] = 3.7
  v[:, 0, 1] = 2.0 + 0.3 * np.arange(K)
  v[:, 0, 2] = -1e-3
  got, ref = SC.smooth(v, 0, K, w), reference(v, 0, K, w)
  for m in (0, 2):
    assert (np.abs(got["trend"][:, 0, m] - v[:, 0, m]) <= ref["B"][:, 0, m]).all()
    assert (np.abs(got["resid"][:, 0, m]) <= ref["B"][:, 0, m]).all()
  inner = slice(H, K - H)
  assert (np.abs(got["trend"][inner, 0, 1] - v[inner, 0, 1]) <= ref["B"][inner, 0, 1]).all()
  assert (np.abs(got["resid"][inner, 0, 1]) <= ref["B"][inner, 0, 1]).all()
  # at the edges the renormalised kernel is one-sided: the ramp is NOT reproduced there
  assert abs(got["resid"][0, 0, 1]) > 1.0


@pytest.mark.parametrize("case", CASES[:4] + CASES[5:8], ids=IDS[:4] + IDS[5:8])
def test_resid_plus_trend_gives_the_series_back(case):
  """Within 1 ulp of X (the largest finite |x| in reach) at the finite records."""
  c = case
  r = SC.restate(c)
  x = c["v"][c["k0"]:c["k1"]]
  fin = np.isfinite(x) & np.isfinite(r["trend"])
  H, K = c["H"], c["K"]
  X = np.stack([_finite_max(x[max(0, j - H):min(K, j + H + 1)]) for j in range(K)])
  with np.errstate(all="ignore"):
    err = np.abs((r["resid"] + r["trend"]) - x)
  assert (err[fin] <= np.spacing(X[fin])).all()


def test_the_order_of_the_sum_is_the_definition():
  """x = (2^54, 1, -2^54), w = (1, 1/2): ascending, num at j = 1 is (2^53 + 1) - 2^53 with the 1
  lost to the tie; descending it survives."""
  v = np.array([2.0 ** 54, 1.0, -2.0 ** 54]).reshape(3, 1, 1)
  w = np.array([1.0, 0.5])
  assert SC.smooth(v, 0, 3, w)["trend"][1, 0, 0] == 0.0
  assert SC.smooth(v, 0, 3, w, mutant="descending")["trend"][1, 0, 0] == 0.5
  # signed zeros: a sum from +0.0 is never -0.0
  z = SC.smooth(np.full((4, 1, 1), -0.0), 0, 4, w)
  assert not np.signbit(z["trend"]).any() and np.signbit(z["resid"]).all()


# ------------------------------------------------------------------ invariances
def _same(a, b, what):
  for key in ("trend", "resid"):
    assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
    num = ~np.isnan(a[key])
    assert np.array_equal(np.signbit(a[key][num]), np.signbit(b[key][num])), (what, key, "zeros")
  assert np.array_equal(a["nbad"], b["nbad"]), what


def test_restatement_invariances():
  c = CASES[2]  # n 33, nspec 3, K 200, H 80
  whole = SC.restate(c)
  # a member alone, a shard
  one = SC.restate(c, v=c["v"][:, 1:2, 7:8])
  _same(one, {k: (a[:, 1:2, 7:8] if a.ndim == 3 else a[1:2, 7:8]) for k, a in whole.items()}, "member")
  shard = SC.restate(c, v=c["v"][:, :, 10:25])
  _same(shard, {k: a[..., 10:25] for k, a in whole.items()}, "shard")
  # a sub-window copied out: the records outside it are never read
  k0, k1 = c["k0"] + 17, c["k1"] - 30
  sub = SC.restate(c, k0=k0, k1=k1)
  copied = SC.restate(c, v=np.ascontiguousarray(c["v"][k0:k1]), k0=0, k1=k1 - k0)
  _same(sub, copied, "sub-window")
  assert not np.array_equal(sub["trend"], whole["trend"][17:170], equal_nan=True)  # (other edges)


# ------------------------------------------------------------------ mutants
@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_mutants_of_the_restatement_are_caught(fractions, mutant):
  """A wrong definition leaves the bound, or (the order of the sum) misses the constructed bits."""
  if mutant == "descending":
    v = np.array([2.0 ** 54, 1.0, -2.0 ** 54]).reshape(3, 1, 1)
    right, wrong = (SC.smooth(v, 0, 3, np.array([1.0, 0.5]), mutant=mu)["trend"][1, 0, 0]
                    for mu in (None, mutant))
    assert right == 0.0 and wrong != right
    return
  c = CASES[0]  # n 5, nspec 2, K 37, H 8: NaN styles and edges inside one small case
  assert fractions(c) <= 1.0
  frac = _within_bound(c, mutant=mutant)
  print("%s: %.3g times the bound" % (mutant, frac))
  assert frac > 1.0, (mutant, frac)


# ------------------------------------------------------------------ the C-ABI
def test_smooth_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  cls = _lib.pm_series_smooth
  vals = _layout(tmp_path, cls.__name__, cls._fields_)
  assert vals[0] == C.sizeof(cls)
  assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_series_smooth"][1][0] is C.POINTER(cls)
  assert (_lib.PM_SMOOTH_MAX, _lib.PM_SMOOTH_HALF_MAX) == (SC.K_MAX, SC.HALF_MAX) == (4096, 4095)
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  assert re.search(r"#define PM_SMOOTH_MAX %d\b" % _lib.PM_SMOOTH_MAX, text)
  assert re.search(r"#define PM_SMOOTH_HALF_MAX %d\b" % _lib.PM_SMOOTH_HALF_MAX, text)
  assert "num     = sum w[|i - j|] * x_i" in text and "den     = sum w[|i - j|]" in text


_TABLES = {}


def _table(key, H):
  """The host address of a kept weight table of H + 1 values: `key` names an edit of the valid
  one."""
  w = np.exp(-0.5 * (np.arange(H + 1, dtype=np.float64) / (0.25 * H + 1.0)) ** 2)
  edit = dict(valid=lambda: None, w0=lambda: w.__setitem__(0, 1.0 + 2.0 ** -52),
              w0_nan=lambda: w.__setitem__(0, np.nan), nan=lambda: w.__setitem__(H, np.nan),
              inf=lambda: w.__setitem__(1, np.inf), zero=lambda: w.__setitem__(H, 0.0),
              negative=lambda: w.__setitem__(H, -1e-9),
              rising=lambda: w.__setitem__(H, w[H - 1] * (1.0 + 2.0 ** -52)))[key]
  edit()
  _TABLES[(key, H)] = w
  return w.ctypes.data


def desc(table="valid", **kw):
  """A valid pm_series_smooth descriptor (the device addresses are stand-ins) with the edits."""
  from pymoc_amd import _lib
  d = _lib.pm_series_smooth()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.half, d.v, d.w_dev = 10, 2, 60, 1, 50, 8, FAKE, FAKE
  for k, v in kw.items():
    setattr(d, k, v)
  if "w" not in kw:
    d.w = _table(table, max(2, min(int(d.half), 4095)))
  return d


def bad_descriptors():
  return [("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("nspec 0", dict(nspec=0)),
          ("nrec 0", dict(nrec=0)), ("k0 -1", dict(k0=-1)), ("k0 == k1", dict(k0=50)),
          ("k1 < k0", dict(k0=55)), ("k1 > nrec", dict(k1=61)),
          ("K 4097", dict(nrec=5000, k0=3, k1=4100)),
          ("half 0", dict(half=0)), ("half -1", dict(half=-1)), ("half 4096", dict(half=4096)),
          ("nspec 65536", dict(nspec=65536)), ("v", dict(v=None)), ("w", dict(w=None)),
          ("w_dev", dict(w_dev=None)),
          ("w[0] != 1", dict(table="w0")), ("w[0] NaN", dict(table="w0_nan")),
          ("w NaN", dict(table="nan")), ("w inf", dict(table="inf")), ("w 0", dict(table="zero")),
          ("w < 0", dict(table="negative")), ("w rising", dict(table="rising")),
          ("tiles * chunks 2^31", dict(n=2**31 - 1, nrec=4096, k0=0, k1=4096, half=80))]


def test_entry_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  out = (FAKE + 64, FAKE + 128, FAKE + 192)
  assert L.pm_series_smooth(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(**kw)
    assert L.pm_series_smooth(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc()
  assert L.pm_series_smooth(C.byref(d), None, None, out[2], None) == _lib.PM_EINVAL
  assert "trend and resid are both NULL" in L.pm_last_error().decode()
  assert L.pm_series_smooth(C.byref(d), out[0], out[1], None, None) == _lib.PM_EINVAL
  assert "nbad is NULL" in L.pm_last_error().decode()
  d = desc(k0=50)
  assert L.pm_series_smooth(C.byref(d), *out, None) == _lib.PM_EINVAL
  assert "window [50, 50) is not inside the 60 records" in L.pm_last_error().decode()  # the shared check
  d = desc(table="rising")
  assert L.pm_series_smooth(C.byref(d), *out, None) == _lib.PM_EINVAL
  assert "w[8]" in L.pm_last_error().decode() and "is above w[7]" in L.pm_last_error().decode()


def _geometry(H):
  from pymoc_amd import _lib
  tm, nr = C.c_int32(0), C.c_int32(0)
  assert _lib.lib.pm_series_smooth_geometry(H, C.byref(tm), C.byref(nr)) == _lib.PM_OK
  return tm.value, nr.value


def _lds_bytes(H, K):
  """The dynamic LDS one block of a launch (H, K) asks for, as the launcher itself forms it."""
  from pymoc_amd import _lib
  b = C.c_size_t(0)
  assert _lib.lib.pm_series_smooth_lds_bytes(H, K, C.byref(b)) == _lib.PM_OK
  return b.value


_USAGE = {}


def _resource_usage(tmp_path):
  """What the compiler reports for the three instantiations of k_series_smooth on gfx950:
  dict(names, scratch, spills, vgprs, lds) -- lds the STATIC LDS bytes per block, which a block
  holds on top of what the launcher asks for.  Compiled once."""
  if not _USAGE:
    from conftest import ROOT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "pymoc_amd", "csrc", "smooth.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                        "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                        "-c", "-o", str(tmp_path / "smooth.o"), src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:]
    found = lambda pat: [int(x) for x in re.findall(pat, p.stdout)]  # noqa: E731
    _USAGE.update(names=re.findall(r"Function Name: (\S*k_series_smooth\S*)", p.stdout),
                  scratch=found(r"ScratchSize \[bytes/lane\]: (\d+)"),
                  spills=found(r"[SV]GPRs Spill: (\d+)"), vgprs=found(r" VGPRs: (\d+)"),
                  lds=found(r"LDS Size \[bytes/block\]: (\d+)"))
  return _USAGE


def test_the_tile_rule(tmp_path):
  """Widest rows first, half a CU's LDS before the whole; for EVERY H and the K that asks for the
  most, what a block holds -- the launcher's own dynamic request (the rows it stages, at most the
  4096 records of a window, the table, the counts and the flag) PLUS the static LDS the compiler
  reports for the kernel -- fits the 160 KiB; the chunk holds a record; the table's chunk cases sit
  on the boundary and its full-LDS cases ask for what they say."""
  from pymoc_amd import _lib
  static = _resource_usage(tmp_path)["lds"]
  assert len(static) == 3
  assert _geometry(SC.CHUNK_H) == (32, SC.CHUNK)
  assert [_geometry(H)[0] for H in (1, 8, 40, 80, 300, 600, 1200, 4095)] == [32, 32, 32, 32, 16, 8, 4, 2]
  assert _geometry(4095) == (2, 4096) and _geometry(1200) == (4, 4096)
  most = 0
  for H in range(1, 4096):
    tm, nr = _geometry(H)
    rows = min(4096, nr + 2 * H)
    assert tm in (2, 4, 8, 16, 32) and 1 <= nr <= 4096, H
    asked = _lds_bytes(H, 4096)  # (the request grows with K up to the rows a block stages)
    assert asked == 8 * rows * tm + 8 * (H + 1) + 4 * (tm + 1), (H, tm, nr, asked)
    assert asked + max(static) <= 160 * 1024, (H, tm, nr, asked, static)
    assert _lds_bytes(H, min(rows, 4096)) == asked and _lds_bytes(H, 1) <= asked, H
    most = max(most, asked)
    assert nr == 4096 or nr < 1024 // tm or nr % (1024 // tm) == 0, (H, tm, nr)
  assert most == max(SC.FULL_LDS.values()) == 163836  # (4 bytes to spare at H = 310, 602, 4092)
  for c in CASES:
    if c["H"] in SC.FULL_LDS:
      assert _lds_bytes(c["H"], c["K"]) == SC.FULL_LDS[c["H"]], c["name"]
  assert {c["H"] for c in CASES} >= set(SC.FULL_LDS) | {279}
  for bad in (0, -1, 4096):
    assert _lib.lib.pm_series_smooth_geometry(bad, C.byref(C.c_int32()), C.byref(C.c_int32())) == _lib.PM_EINVAL
  assert _lib.lib.pm_series_smooth_geometry(8, None, None) == _lib.PM_EINVAL
  for H, K in ((0, 10), (4096, 10), (8, 0), (8, 4097)):
    assert _lib.lib.pm_series_smooth_lds_bytes(H, K, C.byref(C.c_size_t())) == _lib.PM_EINVAL
  assert _lib.lib.pm_series_smooth_lds_bytes(8, 10, None) == _lib.PM_EINVAL


def test_kernel_cross_compiles_without_scratch(tmp_path):
  """k_series_smooth (trend and resid, trend only, resid only) for gfx950: 0 bytes of scratch, no
  spills, and 0 bytes of static LDS -- the tile rule fills a CU's LDS to within 4 bytes, so a
  block-wide reduction of the device library with a buffer of its own would push a launch over
  (DESIGN.md section 24 records the registers)."""
  u = _resource_usage(tmp_path)
  assert len(set(u["names"])) == 3 and len(u["scratch"]) == 3 and len(u["spills"]) == 6
  assert len(u["lds"]) == 3
  assert all(x == 0 for x in u["scratch"] + u["spills"] + u["lds"]), u
  assert max(u["vgprs"]) <= 64, u["vgprs"]  # 1024 threads to a block: 8 waves to a SIMD stay possible


# ------------------------------------------------------------------ the classes
class _Recorder(object):
  """A stand-in for an IndexRecorder whose last record was never written."""

  class _T(object):
    names = ["wind", "amoc"]

  class _E(object):
    stream = timer = None
    _member0 = 0

  def __init__(self, nrec):
    self._values, self.table, self.ens = _Series((nrec, 2, 6)), self._T(), self._E()
    self.steps = np.arange(nrec) * 12
    self.steps[-1] = -1


def test_classes_validate_their_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call."""
  import pymoc_amd
  from pymoc_amd import SeriesSmooth, SeriesSurrogates, SeriesWindows
  from pymoc_amd.smooth import sigma_of_ksmooth
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  ok = SeriesSmooth(src, 2.5)
  assert (ok.sigma, ok.truncate, ok.half) == (2.5, 4.0, 10) and ok.weights.shape == (11,)
  assert np.array_equal(ok.weights, SC.weights(2.5)) and ok.weights[0] == 1.0
  assert SeriesSmooth(src, 1023.75).half == 4095 and SeriesSmooth(src, 0.3).half == 1
  assert SeriesSmooth(src, 20, truncate=1).half == 20 and SeriesSmooth(src, np.float64(3.0)).half == 12
  assert sigma_of_ksmooth(10.0) == 0.25 * 10.0 / 0.6744897501960817
  assert pymoc_amd.SeriesSmooth is SeriesSmooth
  for sigma in (0.0, -1.0, np.nan, np.inf, "2", None, True):
    with pytest.raises(ValueError, match="sigma"):
      SeriesSmooth(src, sigma)
  for tr in (0.99, 8.01, np.nan, "4", None, False):
    with pytest.raises(ValueError, match="truncate"):
      SeriesSmooth(src, 2.0, truncate=tr)
  for sigma, tr in ((0.1, 4.0), (1023.9, 4.0), (600.0, 8.0), (0.49, 1.0)):
    with pytest.raises(ValueError, match=r"half-width .* is outside \[1, 4095\]"):
      SeriesSmooth(src, sigma, truncate=tr)
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"])):
    with pytest.raises(ValueError, match="series"):
      SeriesSmooth(bad, 2.0)
  with pytest.raises(ValueError, match="nspec = 65536 is above 65535"):
    SeriesSmooth((_Series((100, 65536, 1)), range(65536)), 2.0)
  for k0, k1 in ((-1, 40), (40, 40), (50, 20), (0, 101)):
    for call in (ok.trend, ok.residual, ok.compute):
      with pytest.raises(ValueError, match="window"):
        call(k0, k1)
  long = SeriesSmooth((_Series((5000, 1, 1)), ["amoc"]), 2.0)
  for call in (long.trend, long.residual, long.compute):
    with pytest.raises(ValueError, match="holds 4097 records, more than 4096"):
      call(3, 4100)
  with pytest.raises(ValueError, match=r"window \[0, 50\) holds record 49, which was never written"):
    SeriesSmooth(_Recorder(50), 2.0).residual()
  # the keyword of the two classes built on it
  for cls, args in ((SeriesWindows, (src, 16)), (SeriesSurrogates, (src,))):
    g = cls(*args, detrend="gaussian", sigma=5.0)
    assert g.detrend == "gaussian" and g._smooth == (5.0, 4.0, 20)
    assert cls(*args, detrend="gaussian", sigma=5, truncate=2)._smooth == (5.0, 2.0, 10)
    assert cls(*args)._smooth is None
    for det in ("linear", "constant", "none"):
      with pytest.raises(ValueError, match="sigma is given"):
        cls(*args, detrend=det, sigma=5.0)
    with pytest.raises(ValueError, match="needs sigma"):
      cls(*args, detrend="gaussian")
    with pytest.raises(ValueError, match="unknown detrend"):
      cls(*args, detrend="loess", sigma=5.0)
    with pytest.raises(ValueError, match="sigma"):
      cls(*args, detrend="gaussian", sigma=-1.0)
    with pytest.raises(ValueError, match="truncate"):
      cls(*args, detrend="gaussian", sigma=5.0, truncate=9)
    with pytest.raises(ValueError, match="half-width"):
      cls(*args, detrend="gaussian", sigma=2000.0)
  big = SeriesWindows((_Series((5000, 1, 1)), ["amoc"]), 64, step=64, detrend="gaussian", sigma=9.0)
  for call in (big.compute, big.trend, big.significance, lambda a, b: big.across_members("var", a, b)):
    with pytest.raises(ValueError, match="holds 4097 records, more than the 4096"):
      call(3, 4100)
  assert SeriesWindows((_Series((5000, 1, 1)), ["amoc"]), 64, step=64).nwin(3, 4100) == 64  # (no such limit)
  with pytest.raises(ValueError, match="holds 4097 records"):
    SeriesSurrogates((_Series((5000, 1, 1)), ["amoc"]), detrend="gaussian", sigma=9.0).fit(3, 4100)
  rec = SeriesWindows(_Recorder(50), 8, detrend="gaussian", sigma=3.0)
  for call in (rec.compute, rec.trend, rec.significance):
    with pytest.raises(ValueError, match="holds record 49, which was never written"):
      call()
  # a surrogate counts 16 K nspec n bytes under "gaussian"
  from pymoc_amd.surrogates import chunk_size
  assert chunk_size(1000, 2 << 30, 1200, 8, 4096) == 6
  assert chunk_size(1000, 2 << 30, 1200, 8, 4096, per=16) == 3
  g = SeriesWindows(src, 32, step=4, detrend="gaussian", sigma=5.0)
  per = 16 * 100 * 2 * 6
  with pytest.raises(ValueError, match="max_bytes = %d does not hold one surrogate of %d bytes" % (per - 1, per)):
    g.significance(max_bytes=per - 1)


# ------------------------------------------------------------------ calibration and power
N, K, W, S, NSUR, SIGMA, TRUNCATE = 400, 200, 50, 5, 199, 20.0, 4.0


def _stationary(rng, phi):
  """[K, 1, N]: stationary AR(1) series of unit marginal variance; phi a number or [K]."""
  phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))
  v = np.empty((K, 1, N))
  x = rng.standard_normal(N)
  for k in range(K):
    x = phi[k] * x + np.sqrt(1.0 - phi[k] * phi[k]) * rng.standard_normal(N)
    v[k, 0] = x
  return v


def _curved():
  t = np.arange(K) / float(K)
  return (3.0 + 4.0 * t * t - 2.0 * np.sin(3.0 * t))[:, None, None]


def _count(res, key, which="p_rising", level=0.1):
  p = res[key][which]
  assert np.isfinite(p).all()
  return int((p <= level).sum())


def test_the_gaussian_test_is_calibrated():
  """400 stationary AR(1) series (phi = 0.5, K = 200) on the curved trend 3 + 4 t^2 - 2 sin(3 t),
  t = k / K; W = 50, S = 5, sigma = 20, truncate = 4, 199 re-smoothed surrogates from the restated
  Philox stream.  Under the null model the number of series with p_rising <= 0.1 is
  Binomial(400, 0.1) -- mean 40, sd 6; asserted within 5 sd, [10, 70], for var and for ac.
  Observed: var 42, ac 49."""
  rng = np.random.default_rng(20241)
  v = _stationary(rng, 0.5) + _curved()
  res = SC.significance(v, 0, K, W, S, 1, SIGMA, TRUNCATE, NSUR, seed=177, nb=25)
  for key in ("var", "ac"):
    got = _count(res, key)
    print("%s: %d of %d series with p_rising <= 0.1" % (key, got, N))
    assert 10 <= got <= 70, (key, got)
    assert (res[key]["nvalid"] == NSUR).all()


def test_the_gaussian_test_has_power():
  """400 series whose AR coefficient ramps 0.1 -> 0.9 on the same curved trend: at least 200 have
  ac.p_rising <= 0.1.  Observed: 356 (var: 11)."""
  rng = np.random.default_rng(20242)
  v = _stationary(rng, np.linspace(0.1, 0.9, K)) + _curved()
  res = SC.significance(v, 0, K, W, S, 1, SIGMA, TRUNCATE, NSUR, seed=178, nb=25)
  got = _count(res, "ac")
  print("ac: %d of %d series with p_rising <= 0.1; var: %d" % (got, N, _count(res, "var")))
  assert got >= 200, got
