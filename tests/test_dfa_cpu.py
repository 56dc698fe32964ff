"""pm_series_dfa and SeriesWindows(dfa=...) without a device: the restatement (tests/dfa_cases.py)
against an extended-precision evaluation of the same definition within a derived forward bound,
against an independent vectorised evaluation, its invariances, the indicator on white noise and on
a random walk, the calibration and the power of the restated surrogate test, the header mirror,
every argument check of the entry and of the class, and the kernel's scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dfa_cases as DC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

CASES = DC.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def restated():
  """name -> the float64 restatement of the case: computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = DC.restate(c)
    return cache[c["name"]]
  return get


def _fraction(got, ref, bound, ok):
  """The largest |got - ref| / bound over the entries `ok`; 0 where the bound and the error are
  both 0 (a constant window: every operand is exact)."""
  with np.errstate(all="ignore"):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref).astype(np.float64)
    frac = np.where(err == 0.0, 0.0, err / bound)
  return float(frac[ok].max()) if ok.any() else 0.0


def test_restatement_against_extended_precision(restated):
  """(a) F2 of the float64 restatement lies within `dfa_cases.f2_bound` (a
  derived forward bound in W, s, max |y|, and under "linear" max |x - mean| and max |x|) of the
  np.longdouble evaluation of the same definition, on every case of the table and every F2 that
  is finite in both.  Observed (one run): the largest fraction of the bound is 0.018 (W = 20, "linear"),
  5e-4 to 1.4e-3 under "none" and "constant"."""
  worst = 0.0
  for c in CASES:
    r = restated(c)
    ref = DC.restate(c, dtype=np.longdouble)
    ok = np.isfinite(r["f2"]) & np.isfinite(ref["f2"].astype(np.float64))
    assert ok.any(), c["name"]
    frac = _fraction(r["f2"], ref["f2"], DC.f2_bound(r, c["W"], c["scales"], c["detrend"]), ok)
    print("%-60s largest |dF2| / bound %.3g" % (c["name"], frac))
    assert frac <= 1.0, (c["name"], frac)
    worst = max(worst, frac)
    # alpha of the restatement against alpha_of in extended precision from the same F2: the
    # bound of the device's alpha holds for NumPy's log as well
    fin = np.isfinite(r["alpha"])
    al = DC.alpha_of(r["f2"], c["scales"], dtype=np.longdouble)
    assert np.array_equal(fin, np.isfinite(al.astype(np.float64)))
    assert _fraction(r["alpha"], al, DC.alpha_bound(r["f2"], c["scales"]), fin) <= 1.0, c["name"]
  print("largest observed fraction of the F2 bound: %.3g" % worst)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_an_independent_evaluation(restated, case):
  """(b) np.cumsum, a reshape into boxes and the normal equations, within twice the bound."""
  c, r = case, restated(case)
  fast = DC.dfa_fast(c["v"], c["k0"], c["k1"], c["W"], c["S"], c["detrend"], c["scales"])
  assert np.isnan(fast[:, ~r["used"]]).all() and np.isnan(r["f2"][:, ~r["used"]]).all()
  ok = np.isfinite(r["f2"]) & np.isfinite(fast)
  bound = 2.0 * DC.f2_bound(r, c["W"], c["scales"], c["detrend"])
  assert _fraction(r["f2"], fast.astype(np.longdouble), bound, ok) <= 1.0, c["name"]


def test_table_holds_what_it_must(restated):
  """Every style in the table; unused windows, F2 == 0 (alpha NaN), overflow (F2 inf, alpha NaN);
  and the one case with more windows than a block takes has a full and a partial chunk."""
  from pymoc_amd import _lib
  seen = set()
  for c in CASES:
    nspec, n = c["v"].shape[1:]
    seen |= {DC.style_of(s, m) for s in range(nspec) for m in range(n)}
    assert len(c["scales"]) >= 2 and c["scales"][0] >= 4 and 4 * c["scales"][-1] <= c["W"]
  assert seen == set(DC.STYLES)
  c = CASES[0]
  r = restated(c)
  assert (~r["used"]).any() and r["used"].any()
  assert (r["f2"] == 0).any() and np.isinf(r["f2"]).any()
  assert np.isnan(r["alpha"][r["used"] & (r["f2"] == 0).any(axis=0)]).all()
  assert np.isnan(r["alpha"][np.isinf(r["f2"]).any(axis=0)]).all()
  assert np.isfinite(r["alpha"]).any()
  tm, nwb = C.c_int32(0), C.c_int32(0)
  many = next(c for c in CASES if c["nwin"] == DC.MANY)
  assert _lib.lib.pm_series_windows_geometry(many["W"], many["S"], C.byref(tm), C.byref(nwb)) == 0
  assert nwb.value < DC.MANY < 2 * nwb.value and 37 % tm.value
  big = next(c for c in CASES if c["W"] == 4096)
  assert _lib.lib.pm_series_windows_geometry(4096, 4096, C.byref(tm), C.byref(nwb)) == 0
  assert tm.value == 4 and big["v"].shape[2] % 4
  assert {c["S"] for c in CASES} >= {1, 3} and any(c["S"] == c["W"] for c in CASES)
  assert {c["v"].shape[2] for c in CASES} >= {1, 33, 37}


def test_restatement_invariances():
  """(c) Adding a constant to x changes F2 by no more than the two evaluations' bounds under any
  detrend; scaling x by 2^k scales F2 by 4^k exactly, and alpha's operands' logs then differ by
  2 k ln 2 within the logarithm's own rounding."""
  rng = np.random.default_rng(11)
  v = np.cumsum(rng.standard_normal((70, 2, 5)), axis=0) * 0.3 + rng.standard_normal((70, 2, 5))
  v = np.round(v * 2.0 ** 20) * 2.0 ** -20  # (so that v + off below is exact: the same data, moved)
  scales = (4, 6, 9, 13)
  for det in DC.DETRENDS:
    base = DC.dfa(v, 2, 68, 54, 4, det, scales)
    assert np.isfinite(base["alpha"]).all()
    for off in (1.0, -37.5, 2.0 ** 20):
      moved = DC.dfa(v + off, 2, 68, 54, 4, det, scales)
      bound = DC.f2_bound(base, 54, scales, det) + DC.f2_bound(moved, 54, scales, det)
      assert (np.abs(moved["f2"] - base["f2"]) <= bound).all(), (det, off)
    for k in (1, -3, 40):
      scaled = DC.dfa(v * 2.0 ** k, 2, 68, 54, 4, det, scales)
      assert np.array_equal(scaled["f2"], base["f2"] * 4.0 ** k), (det, k)
      shift = np.log(scaled["f2"]) - np.log(base["f2"])
      assert (np.abs(shift - 2 * k * np.log(2.0))
              <= 4 * DC.U * (np.abs(np.log(scaled["f2"])) + np.abs(np.log(base["f2"])))).all()
      # the weights sum to zero, so alpha moves only by rounding
      assert (np.abs(scaled["alpha"] - base["alpha"])
              <= DC.alpha_bound(scaled["f2"], scales) + DC.alpha_bound(base["f2"], scales)
              + abs(2 * k * np.log(2.0)) * 8 * DC.U).all(), (det, k)
  # "none" is "constant": the profile is the mean-removed series' by definition
  a, b = DC.dfa(v, 2, 68, 54, 4, "none", scales), DC.dfa(v, 2, 68, 54, 4, "constant", scales)
  assert np.array_equal(a["f2"], b["f2"])


def test_the_indicator_reads_memory():
  """(d) 400 series of white noise and 400 random walks, W = 256, the default scales, the window's
  mean removed (plain DFA, "constant": what the prototype's numbers were taken with; "linear" gives
  1.447 for the walks, the line taking some of their memory with it): the ensemble mean of alpha is 0.5 +- 0.1 and 1.5 +- 0.1, and within three standard
  errors of the prototype's 0.53 (spread 0.06) and 1.47 (spread 0.09) with those spreads.
  Observed with this seed: 0.538 (sd 0.057) and 1.473 (sd 0.095)."""
  rng = np.random.default_rng(1)
  v = rng.standard_normal((256, 1, 400))
  scales = DC.default_scales(256)
  for series, centre, target, spread in ((v, 0.5, 0.53, 0.06),
                                         (np.cumsum(v, axis=0), 1.5, 1.47, 0.09)):
    al = DC.dfa(series, 0, 256, 256, 256, "constant", scales)["alpha"]
    assert np.isfinite(al).all()
    print("alpha: mean %.4f sd %.4f (prototype %.2f +- %.2f)" % (al.mean(), al.std(), target, spread))
    assert abs(al.mean() - centre) <= 0.1
    assert abs(al.mean() - target) <= 3 * spread / np.sqrt(400.0)


# ------------------------------------------------------------------ the restated surrogate test
N, K, W, S, NSUR = 200, 300, 100, 10, 99
SCALES = (4, 6, 9, 13, 18, 25)


def _stationary(rng, phi):
  """[K, 1, N]: stationary AR(1) series of unit marginal variance; phi a number or [K]."""
  phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))
  v = np.empty((K, 1, N))
  x = rng.standard_normal(N)
  for k in range(K):
    x = phi[k] * x + np.sqrt(1.0 - phi[k] * phi[k]) * rng.standard_normal(N)
    v[k, 0] = x
  return v


def _count(res, level=0.1):
  assert np.isfinite(res["p_rising"]).all() and (res["nvalid"] == NSUR).all()
  return int((res["p_rising"] <= level).sum())


def test_the_test_is_calibrated():
  """(e) 200 stationary AR(1) series (phi = 0.5, K = 300), W = 100, S = 10, six scales 4 .. 25,
  linear detrending, 99 AR(1) surrogates of the restated fit: under the null model p_rising is
  uniform, so the number of series with dfa p_rising <= 0.1 is Binomial(200, 0.1), mean 20, sd
  4.24; asserted within 3 sd, [8, 32].  Observed with this seed: 18."""
  rng = np.random.default_rng(20121)
  res = DC.significance(_stationary(rng, 0.5), 0, K, W, S, "linear", SCALES, NSUR, seed=91, nb=33)
  got = _count(res)
  print("dfa: %d of %d stationary series with p_rising <= 0.1" % (got, N))
  sd = np.sqrt(N * 0.1 * 0.9)
  assert abs(got - 0.1 * N) <= 3 * sd, got


def test_the_test_has_power():
  """(e) The AR coefficient ramping 0.1 -> 0.9: more than half of the 200 series have dfa
  p_rising <= 0.1.  Observed with this seed: 168."""
  rng = np.random.default_rng(20122)
  res = DC.significance(_stationary(rng, np.linspace(0.1, 0.9, K)), 0, K, W, S, "linear", SCALES,
                        NSUR, seed=92, nb=33)
  got = _count(res)
  print("dfa: %d of %d ramped series with p_rising <= 0.1" % (got, N))
  assert got > N // 2, got


# ------------------------------------------------------------------ the C-ABI
def test_dfa_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  cls = _lib.pm_series_dfa
  vals = _layout(tmp_path, cls.__name__, cls._fields_)
  assert vals[0] == C.sizeof(cls)
  assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_series_dfa"][1][0] is C.POINTER(cls)
  assert (_lib.PM_DFA_SCALES_MAX, _lib.PM_DFA_SCALE_MIN) == (DC.SCALES_MAX, DC.SCALE_MIN)
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  for name in ("PM_DFA_SCALES_MAX", "PM_DFA_SCALE_MIN"):
    assert re.search(r"#define %s %d\b" % (name, getattr(_lib, name)), text), name


def desc(scales=(4, 6, 8), **kw):
  """A valid pm_series_dfa descriptor (the device address is a stand-in) with the edits `kw`; stt
  and the two tables follow the window length and the scales unless they are given.  An edit may
  be a function of the descriptor."""
  from pymoc_amd import _lib
  d = _lib.pm_series_dfa()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = 10, 2, 60, 1, 50
  d.window, d.step, d.detrend, d.v, d.nq = 32, 8, _lib.PM_WIN_DETREND_LINEAR, FAKE, len(scales)
  with np.errstate(all="ignore"):  # (a scale below 1 has no weights: the entry stops before them)
    w = DC.weights_of(scales) if len(scales) >= 2 else [0.0]
  for q, s in enumerate(scales[:16]):
    d.scale[q], d.suu[q], d.weight[q] = s, DC.suu_of(s), w[q]
  for k, v in kw.items():
    if callable(v):
      v(d)
    else:
      setattr(d, k, v)
  if "stt" not in kw:
    d.stt = DC.stt_of(d.window) if d.window > 0 else 0.0
  return d


def _item(field, q, value):
  return lambda d: getattr(d, field).__setitem__(q, value)


def bad_descriptors():
  nan = float("nan")
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)),
          ("k0 > k1", dict(k0=40, k1=20)), ("k1 > nrec", dict(k1=61)),
          ("W 19", dict(window=19, step=1, scales=(4, 5))), ("W 0", dict(window=0)),
          ("W -32", dict(window=-32)), ("W 4097", dict(window=4097, nrec=9000, k1=8000)),
          ("K < W", dict(k0=30)), ("K = W - 1", dict(k0=19)),
          ("step 0", dict(step=0)), ("step -1", dict(step=-1)), ("step W + 1", dict(step=33)),
          ("detrend 3", dict(detrend=3)), ("detrend -1", dict(detrend=-1)),
          ("stt 0", dict(stt=0.0)), ("stt nan", dict(stt=nan)),
          ("stt off by an ulp", dict(stt=float(np.nextafter(DC.stt_of(32), np.inf)))),
          ("stt of another W", dict(stt=DC.stt_of(33))),
          ("nq 1", dict(nq=1)), ("nq 0", dict(nq=0)), ("nq -1", dict(nq=-1)), ("nq 17", dict(nq=17)),
          ("scale 3", dict(scales=(3, 6, 8))), ("scale 0", dict(scales=(0, 6, 8))),
          ("scale -4", dict(scales=(-4, 6, 8))),
          ("scales equal", dict(scales=(4, 6, 6))), ("scales descending", dict(scales=(4, 8, 6))),
          ("4 s above W", dict(scales=(4, 6, 9))), ("s above W", dict(scales=(4, 6, 40))),
          ("suu 0", dict(e=_item("suu", 1, 0.0))), ("suu nan", dict(e=_item("suu", 0, nan))),
          ("suu off by an ulp", dict(e=_item("suu", 2, float(np.nextafter(DC.suu_of(8), 0.0))))),
          ("suu of another scale", dict(e=_item("suu", 1, DC.suu_of(5)))),
          ("weight nan", dict(e=_item("weight", 0, nan))),
          ("weight inf", dict(e=_item("weight", 2, float("inf")))),
          ("weights not summing to 0", dict(e=_item("weight", 1, 0.25))),
          ("weights all 0", dict(e=lambda d: [d.weight.__setitem__(q, 0.0) for q in range(3)])),
          ("v", dict(v=None)),
          ("nwin * nspec", dict(nspec=60000, nrec=1 << 15, k1=1 << 15, step=1)),
          ("nspec 65536", dict(nspec=65536)),
          # 2^29 tiles of 4 members x 4 chunks of one window each
          ("tiles * chunks", dict(n=2**31 - 1, window=4096, step=4096, nrec=20000, k1=20000))]


def test_entry_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  out = (FAKE + 64, FAKE + 128)
  assert L.pm_series_dfa(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(**kw)
    assert L.pm_series_dfa(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc()
  assert L.pm_series_dfa(C.byref(d), None, out[1], None) == _lib.PM_EINVAL
  assert "alpha is NULL" in L.pm_last_error().decode()
  for kw, word in ((dict(stt=5.0), "stt"), (dict(e=_item("suu", 1, 17.0)), "suu[1]"),
                   (dict(e=_item("weight", 1, 0.25)), "weights sum"),
                   (dict(scales=(4, 6, 9)), "4 * scale[2]"), (dict(scales=(4, 6, 6)), "scale[2] = 6"),
                   (dict(bad_descriptors())["tiles * chunks"],
                    "member tiles * window chunks = 2147483648")):
    assert L.pm_series_dfa(C.byref(desc(**kw)), *out, None) == _lib.PM_EINVAL
    assert word in L.pm_last_error().decode(), (word, L.pm_last_error())


def test_kernel_cross_compiles_without_scratch(tmp_path):
  """Both instantiations of k_series_dfa for gfx950: 0 bytes of scratch, no static LDS (DESIGN.md
  section 27 tabulates the registers); windows.hip still compiles against the shared tile rule."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "dfa.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "dfa.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_dfa\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout)]
  assert len(set(names)) == 2 and len(scratch) >= 2
  assert all(x == 0 for x in scratch + lds), list(zip(names, scratch, lds))


# ------------------------------------------------------------------ the class and the scales
def test_default_scales_satisfy_the_limits_for_every_window():
  """(f) default_scales(W) for every W in [20, 4096]: 2 to 8 strictly ascending integers from 4 to
  at most W // 4, the ones the restatement states; below 20 a ValueError."""
  from pymoc_amd.dfa import default_scales, dfa_par, suu_of
  for Wn in range(20, 4097):
    sc = default_scales(Wn)
    assert sc == DC.default_scales(Wn), Wn
    assert 2 <= len(sc) <= 8 and sc[0] == 4 and 4 * sc[-1] <= Wn, (Wn, sc)
    assert all(isinstance(s, int) for s in sc) and all(b > a for a, b in zip(sc, sc[1:])), (Wn, sc)
    assert Wn < 32 or sc[-1] == Wn // 4
  assert default_scales(256) == (4, 6, 9, 13, 20, 29, 43, 64)
  for Wn in (19, 4, 0, -5):
    with pytest.raises(ValueError, match="at least 20"):
      default_scales(Wn)
  par = dfa_par(256, True)
  assert par.scales == default_scales(256) and par.suu == tuple(DC.suu_of(s) for s in par.scales)
  assert np.array_equal(par.weights, DC.weights_of(par.scales))
  from fractions import Fraction
  for s in list(range(4, 70)) + [1023, 1024]:
    assert Fraction(suu_of(s)) == sum(Fraction(2 * i - (s - 1), 2) ** 2 for i in range(s)), s


def test_series_windows_validates_dfa_before_any_device_array():
  """Every refusal is a ValueError raised on the host at construction."""
  from pymoc_amd import SeriesWindows
  src = (_Series((400, 2, 6)), ["wind", "amoc"])
  none = SeriesWindows(src, 64)
  assert none._dfa is None and none.dfa_scales is None
  assert SeriesWindows(src, 64, dfa=True).dfa_scales == (4, 5, 6, 7, 9, 11, 13, 16)
  assert SeriesWindows(src, 20, dfa=True).dfa_scales == (4, 5)
  assert SeriesWindows(src, 64, dfa=[4, 16]).dfa_scales == (4, 16)
  assert SeriesWindows(src, 76, dfa=np.arange(4, 20)).dfa_scales == tuple(range(4, 20))
  assert SeriesWindows(src, 64, dfa=(4, 8), detrend="gaussian", sigma=5.0).dfa_scales == (4, 8)
  for W_, bad, word in ((19, True, "at least 20"), (16, True, "at least 20"),
                        (64, (4,), "2 to 16 scales"), (64, (), "2 to 16 scales"),
                        (200, tuple(range(4, 21)), "2 to 16 scales"),
                        (64, (3, 8), "at least 4"), (64, (0, 8), "at least 4"),
                        (64, (4, 4), "strictly ascending"), (64, (8, 4), "strictly ascending"),
                        (64, (4, 17), "four boxes"), (64, (4, 8, 100), "four boxes"),
                        (64, (4.0, 8), "integer"), (64, (4, "8"), "integer"),
                        (64, (4, True), "integer"), (64, False, "True or a sequence"),
                        (64, 8, "True or a sequence"), (64, "48", "True or a sequence")):
    with pytest.raises(ValueError, match=word):
      SeriesWindows(src, W_, dfa=bad)
  with pytest.raises(ValueError, match="unknown indicator 'dfa'"):
    none.across_members("dfa")
  with pytest.raises(ValueError, match="one of mean, slope, var, ac, dfa"):
    SeriesWindows(src, 64, dfa=True).across_members("skew")
