"""pm_series_restoring and SeriesWindows(restoring=...) without a device: the restatement
(tests/restoring_cases.py) against an extended-precision evaluation by whitened passes within a
derived forward bound, iteration by iteration; one iteration against np.polyfit; what the indicator
separates; the calibration and the power of the restated surrogate test; the header mirror, every
argument check of the entry and of the class, and the kernel's scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import restoring_cases as RC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

CASES = RC.cases()
IDS = [c["name"] for c in CASES]
NOISE = ("ar1", "big", "small", "offset", "persist")  # the styles with a lambda to speak of


@pytest.fixture(scope="module")
def restated():
  """name -> the float64 restatement of the case with its trace: computed once, shared, left
  unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = RC.restate(c, trace=True)
    return cache[c["name"]]
  return get


def _args(c):
  return c["v"], c["k0"], c["k1"], c["W"], c["S"], c["detrend"]


def _fraction(got, ref, ok):
  """The largest |got.v - ref| / got.e over the entries `ok` of a Tracked `got`; 0 where the error
  is 0 (a window of exact operands)."""
  with np.errstate(all="ignore"):
    err = np.abs(got.v.astype(np.longdouble) - ref).astype(np.float64)
    frac = np.where(err == 0.0, 0.0, err / got.e)
  return float(frac[ok].max()) if ok.any() else 0.0


def _noise_mask(c, shape):
  nspec, n = c["v"].shape[1:]
  m = np.array([[RC.style_of(s, j) in NOISE for j in range(n)] for s in range(nspec)])
  return np.broadcast_to(m, shape)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_extended_precision(restated, case):
  """Every lambda_i and every rho_{i+1} of the float64 restatement lies within the running bound
  (`restoring_cases.bounds`) of the np.longdouble evaluation by whitened
  passes of the same iteration, with the restatement's own rho_i fed into both -- on every case,
  every iteration and every window where both values and the bound are finite.  The Tracked
  values are the restatement's bit for bit.  The end-to-end difference from the iteration run in
  np.longdouble throughout is printed, not asserted: the iteration map may expand a difference.
  Observed (one run): the largest fraction of the bound over the table is 0.12 (W = 9,
  "constant"); the largest end-to-end relative difference of lambda over the noise styles is
  3.3e-14 (W = 9) under "none" and "constant" and, `offset` aside, 1.4e-14 under "linear"; the
  `offset` members (1e6 + AR(1)) reach 1.1e-9 under "linear" (W = 20), where the rounding of the
  slope of 1e6-sized values enters d_j as a line no intercept absorbs -- pass 1 is
  pm_series_windows' by definition."""
  c, r = case, restated(case)
  worst, seen = 0.0, 0
  both = RC.bounds(*_args(c), r["rhos"])
  for i, (lt, nt) in enumerate(both):
    assert np.array_equal(lt.v[r["used"]].view(np.uint64), r["lams"][i][r["used"]].view(np.uint64))
    if i + 1 < c["iters"]:
      assert np.array_equal(nt.v[r["used"]].view(np.uint64),
                            r["rhos"][i + 1][r["used"]].view(np.uint64))
    lam, nxt = RC.direct(*_args(c), r["rhos"][i])
    for got, ref in ((lt, lam), (nt, nxt)):
      ok = (r["used"] & np.isfinite(got.v) & np.isfinite(got.e)
            & np.isfinite(ref.astype(np.float64)))
      seen += int(ok.sum())
      frac = _fraction(got, ref, ok)
      assert frac <= 1.0, (c["name"], i, frac)
      worst = max(worst, frac)
  assert seen or c["v"].shape[2] == 1, c["name"]
  lam, _ = RC.direct_iterated(*_args(c), c["iters"])
  fin = np.isfinite(r["lam"]) & _noise_mask(c, r["lam"].shape)
  with np.errstate(all="ignore"):
    rel = np.abs((r["lam"] - lam.astype(np.float64)) / r["lam"])[fin]
  print("%-52s largest fraction of the bound %.3g, end to end |d lam / lam| %.3g"
        % (c["name"], worst, rel.max() if rel.size else 0.0))


def test_one_iteration_is_ordinary_least_squares(restated):
  """iters = 1 (rho = +0.0): lambda is the slope of the intercept regression of the increments
  d_{t+1} - d_t on d_t over t = 1 .. N - 1 -- np.polyfit on the residual formed in np.longdouble
  -- within the bound of iteration 0, on the noise members of the W = 8, 9, 64 and 256 cases."""
  L = np.longdouble
  checked = 0
  for c in CASES:
    if c["W"] not in (8, 9, 64, 256) or c["v"].shape[2] < 33:
      continue
    r = restated(c)
    lt = RC.bounds(*_args(c), r["rhos"][:1])[0][0]
    x = WC.window_values(*_args(c)[:5]).astype(L)
    W = c["W"]
    t = np.arange(W).astype(L) - L(W - 1) / L(2)
    with np.errstate(all="ignore"):
      d = x - x.sum(axis=-1, keepdims=True) / L(W)
      if c["detrend"] == "linear":
        d = d - ((x * t).sum(axis=-1, keepdims=True) / (t * t).sum()) * t
    d = d.astype(np.float64)
    ok = r["used"] & np.isfinite(lt.v) & np.isfinite(lt.e) & _noise_mask(c, r["used"].shape)
    for idx in np.argwhere(ok)[::7]:
      di = d[tuple(idx)]
      if not np.isfinite(di * di).all():
        continue
      xs, ys = di[:-1], np.diff(di)
      slope = np.polyfit(xs[1:], ys[1:], 1)[0]
      assert abs(lt.v[tuple(idx)] - slope) <= lt.e[tuple(idx)], (c["name"], idx)
      checked += 1
  assert checked > 50


def test_table_holds_what_it_must(restated):
  """Every style and every detrend in the table; the shapes the issue's table sets; unused
  windows; the exactly geometric decay gives q = 0 and NaN; overflow gives NaN; the one case with
  more windows than a block takes has a full and a partial chunk."""
  from pymoc_amd import _lib
  seen = set()
  for c in CASES:
    nspec, n = c["v"].shape[1:]
    seen |= {RC.style_of(s, m) for s in range(nspec) for m in range(n)}
    assert 1 <= nspec <= 3 and c["k0"] > 0 and RC.WIN_MIN <= c["W"] <= 4096
  assert seen == set(RC.STYLES)
  assert {c["detrend"] for c in CASES} == set(RC.DETRENDS)
  assert {c["W"] for c in CASES} == {8, 9, 20, 64, 256, 4096}
  assert {c["iters"] for c in CASES if c["W"] == 64} == {1, 2, 10, 64}
  first = CASES[0]
  assert (first["W"], first["nwin"], first["iters"]) == (8, 1, 1) and first["v"].shape[1:] == (1, 1)
  big = next(c for c in CASES if c["W"] == 4096)
  assert big["nwin"] == 1 and big["v"].shape[2] == 3
  many = next(c for c in CASES if c["nwin"] == RC.MANY)
  assert (many["W"], many["S"], many["iters"]) == (20, 1, 10) and many["v"].shape[2] == 37
  tm, nwb = C.c_int32(0), C.c_int32(0)
  assert _lib.lib.pm_series_windows_geometry(20, 1, C.byref(tm), C.byref(nwb)) == 0
  assert nwb.value < RC.MANY < 2 * nwb.value and 37 % tm.value
  assert _lib.lib.pm_series_windows_geometry(4096, 4096, C.byref(tm), C.byref(nwb)) == 0
  assert tm.value == 4
  # the geometric decay where every operation is exact: lambda = -1/2, then rho = 0 / 0
  c = CASES[1]
  assert (c["W"], c["detrend"], c["iters"]) == (8, "none", 3)
  r = restated(c)
  geom = [(s, m) for s in range(2) for m in range(37) if RC.style_of(s, m) == "geom"]
  assert geom
  for s, m in geom:
    assert (r["lams"][0][:, s, m] == -0.5).all() and np.isnan(r["rhos"][1][:, s, m]).all()
    assert np.isnan(r["lam"][:, s, m]).all() and np.isnan(r["rho"][:, s, m]).all()
  assert (~r["used"]).any() and r["used"].any() and np.isfinite(r["lam"]).any()
  assert np.array_equal(np.isnan(r["lam"]), np.isnan(r["rho"]))
  assert np.isnan(r["lam"][~r["used"]]).all()
  # 254 squares near 1e308: the sums overflow, and lam is NaN
  c = next(c for c in CASES if c["W"] == 256)
  r = restated(c)
  huge = [(s, m) for s in range(3) for m in range(37) if RC.style_of(s, m) == "huge"]
  assert huge
  for s, m in huge:
    assert r["used"][:, s, m].all() and np.isinf(r["sums"]["xcxc"][:, s, m]).all()
    assert np.isnan(r["lam"][:, s, m]).all()


def test_restatement_invariances():
  """Adding a constant moves lambda by no more than the two evaluations' bounds under any detrend
  ("none" included: the residual is x - mean); scaling x by 2^k changes neither lam nor rho by a
  bit; "none" is "constant"."""
  rng = np.random.default_rng(12)
  v = np.cumsum(rng.standard_normal((70, 2, 5)), axis=0) * 0.3 + rng.standard_normal((70, 2, 5))
  v = np.round(v * 2.0 ** 20) * 2.0 ** -20  # (so that v + off below is exact: the same data, moved)
  for det in RC.DETRENDS:
    base = RC.restoring(v, 2, 68, 54, 4, det, 1, trace=True)
    eb = RC.bounds(v, 2, 68, 54, 4, det, base["rhos"])[0][0].e
    assert np.isfinite(base["lam"]).all()
    for off in (1.0, -37.5, 2.0 ** 20):
      moved = RC.restoring(v + off, 2, 68, 54, 4, det, 1, trace=True)
      em = RC.bounds(v + off, 2, 68, 54, 4, det, moved["rhos"])[0][0].e
      assert (np.abs(moved["lam"] - base["lam"]) <= eb + em).all(), (det, off)
    ten = RC.restoring(v, 2, 68, 54, 4, det, 10)
    for k in (1, -3, 40):
      scaled = RC.restoring(v * 2.0 ** k, 2, 68, 54, 4, det, 10)
      assert np.array_equal(scaled["lam"], ten["lam"]) and np.array_equal(scaled["rho"], ten["rho"])
    assert (np.abs(ten["rho"]) <= 1.0).all()
  a, b = (RC.restoring(v, 2, 68, 54, 4, det, 10) for det in ("none", "constant"))
  assert np.array_equal(a["lam"], b["lam"]) and np.array_equal(a["rho"], b["rho"])


def _coloured(rng, phi, rho, K, n):
  """[K, 1, n]: x_{t+1} = phi x_t + eta_t with eta an AR(1) noise of coefficient rho, after a
  spin-up of 200 records."""
  x, eta = np.zeros(n), rng.standard_normal(n)
  v = np.empty((K, 1, n))
  for k in range(-200, K):
    eta = rho * eta + np.sqrt(1.0 - rho * rho) * rng.standard_normal(n)
    x = phi * x + eta
    if k >= 0:
      v[k, 0] = x
  return v


def test_lambda_separates_the_state_from_the_noise():
  """100 series of 256 records with the state coefficient 0.9 (true lambda -0.1) driven by AR(1)
  noise of coefficient 0.3, one window, the mean removed, 10 iterations: the ensemble mean of the
  restated lambda is nearer -0.1 than the mean of ac - 1 is.  Observed with this seed: lambda
  -0.115, ac - 1 -0.066, the errors' rho 0.31."""
  rng = np.random.default_rng(2021)
  v = _coloured(rng, 0.9, 0.3, 256, 100)
  r = RC.restoring(v, 0, 256, 256, 256, "constant", 10)
  ac = WC.windows(v, 0, 256, 256, 256, 1, "constant")["out"][3]
  assert np.isfinite(r["lam"]).all() and (np.abs(r["rho"]) <= 1.0).all()
  lam, naive = float(r["lam"].mean()), float(ac.mean() - 1.0)
  print("lambda: mean %.4f; ac - 1: mean %.4f; rho: mean %.4f (true -0.1, 0.3)"
        % (lam, naive, r["rho"].mean()))
  assert abs(lam + 0.1) < abs(naive + 0.1)
  # with white noise the two agree: one iteration is ac - 1 up to the ends of the window
  w = _coloured(rng, 0.9, 0.0, 256, 100)
  r = RC.restoring(w, 0, 256, 256, 256, "constant", 10)
  ac = WC.windows(w, 0, 256, 256, 256, 1, "constant")["out"][3]
  assert abs(float(r["lam"].mean()) - float(ac.mean() - 1.0)) < 0.02


# ------------------------------------------------------------------ the restated surrogate test
N, K, W, S, NSUR, ITERS = 200, 300, 100, 10, 199, 10


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
  """200 stationary AR(1) series (phi = 0.5, K = 300), W = 100, S = 10, linear detrending, 10
  iterations, 199 AR(1) surrogates of the restated fit, seed 0 throughout (chosen before looking):
  under the null model p_rising is uniform, so the number of series with lam p_rising <= 0.1 is
  Binomial(200, 0.1), mean 20, sd 4.2; asserted within 20 +- 3 * 4.2.  Observed: 17."""
  rng = np.random.default_rng(0)
  res = RC.significance(_stationary(rng, 0.5), 0, K, W, S, "linear", ITERS, NSUR, seed=0, nb=67)
  got = _count(res)
  print("lam: %d of %d stationary series with p_rising <= 0.1" % (got, N))
  assert abs(got - 20) <= 3 * 4.2, got


def test_the_test_has_power():
  """The AR coefficient ramping 0.1 -> 0.9 (lambda rising from -0.9 to -0.1): more than half of
  the 200 series have lam p_rising <= 0.1.  Observed with seed 0: 147."""
  rng = np.random.default_rng(0)
  res = RC.significance(_stationary(rng, np.linspace(0.1, 0.9, K)), 0, K, W, S, "linear", ITERS,
                        NSUR, seed=0, nb=67)
  got = _count(res)
  print("lam: %d of %d ramped series with p_rising <= 0.1" % (got, N))
  assert got > N // 2, got


# ------------------------------------------------------------------ the C-ABI
def test_restoring_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  cls = _lib.pm_series_restoring
  vals = _layout(tmp_path, cls.__name__, cls._fields_)
  assert vals[0] == C.sizeof(cls)
  assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_series_restoring"][1][0] is C.POINTER(cls)
  assert (_lib.PM_RESTORE_WIN_MIN, _lib.PM_RESTORE_ITERS_MAX) == (RC.WIN_MIN, RC.ITERS_MAX)
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  for name in ("PM_RESTORE_WIN_MIN", "PM_RESTORE_ITERS_MAX"):
    assert re.search(r"#define %s %d\b" % (name, getattr(_lib, name)), text), name


def desc(**kw):
  """A valid pm_series_restoring descriptor (the device address is a stand-in) with the edits
  `kw`; stt follows the window length unless it is given."""
  from pymoc_amd import _lib
  d = _lib.pm_series_restoring()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = 10, 2, 60, 1, 50
  d.window, d.step, d.detrend, d.v, d.iters = 32, 8, _lib.PM_WIN_DETREND_LINEAR, FAKE, 10
  for k, v in kw.items():
    setattr(d, k, v)
  if "stt" not in kw:
    d.stt = RC.stt_of(d.window) if d.window > 0 else 0.0
  return d


def bad_descriptors():
  nan = float("nan")
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)),
          ("k0 > k1", dict(k0=40, k1=20)), ("k1 > nrec", dict(k1=61)),
          ("W 7", dict(window=7, step=1)), ("W 4", dict(window=4, step=1)), ("W 0", dict(window=0)),
          ("W -32", dict(window=-32)), ("W 4097", dict(window=4097, nrec=9000, k1=8000)),
          ("K < W", dict(k0=30)), ("K = W - 1", dict(k0=19)),
          ("step 0", dict(step=0)), ("step -1", dict(step=-1)), ("step W + 1", dict(step=33)),
          ("iters 0", dict(iters=0)), ("iters -1", dict(iters=-1)), ("iters 65", dict(iters=65)),
          ("detrend 3", dict(detrend=3)), ("detrend -1", dict(detrend=-1)),
          ("stt 0", dict(stt=0.0)), ("stt nan", dict(stt=nan)),
          ("stt off by an ulp", dict(stt=float(np.nextafter(RC.stt_of(32), np.inf)))),
          ("stt of another W", dict(stt=RC.stt_of(33))),
          ("v", dict(v=None)),
          ("nwin * nspec", dict(nspec=60000, nrec=1 << 15, k1=1 << 15, step=1)),
          ("nspec 65536", dict(nspec=65536)),
          # 2^29 tiles of 4 members x 4 chunks of one window each
          ("tiles * chunks", dict(n=2**31 - 1, window=4096, step=4096, nrec=20000, k1=20000))]


def test_entry_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  out = (FAKE + 64, FAKE + 128)
  assert L.pm_series_restoring(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(**kw)
    assert L.pm_series_restoring(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc()
  assert L.pm_series_restoring(C.byref(d), None, out[1], None) == _lib.PM_EINVAL
  assert "lam is NULL" in L.pm_last_error().decode()
  for kw, word in ((dict(stt=5.0), "stt"), (dict(window=7, step=1), "window length 7 outside [8"),
                   (dict(iters=65), "iters 65 outside [1, 64]"),
                   (dict(bad_descriptors())["tiles * chunks"],
                    "member tiles * window chunks = 2147483648")):
    assert L.pm_series_restoring(C.byref(desc(**kw)), *out, None) == _lib.PM_EINVAL
    assert word in L.pm_last_error().decode(), (word, L.pm_last_error())


def test_kernel_cross_compiles_without_scratch(tmp_path):
  """Both instantiations of k_series_restoring for gfx950: 0 bytes of scratch, no static LDS
  (DESIGN.md section 28 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "restoring.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "restoring.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_restoring\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout)]
  assert len(set(names)) == 2 and len(scratch) >= 2
  assert all(x == 0 for x in scratch + lds), list(zip(names, scratch, lds))


# ------------------------------------------------------------------ the class
def test_restoring_par_and_series_windows_validate_before_any_device_array():
  """Every refusal is a ValueError raised on the host at construction."""
  from pymoc_amd import SeriesWindows, restoring_par
  from pymoc_amd.restoring import RestoringPar
  assert restoring_par(64, True) == RestoringPar(10) and restoring_par(8, 1) == RestoringPar(1)
  assert restoring_par(4096, np.int64(64)).iters == 64
  src = (_Series((400, 2, 6)), ["wind", "amoc"])
  none = SeriesWindows(src, 64)
  assert none._restoring is None
  assert SeriesWindows(src, 64, restoring=True)._restoring.iters == 10
  assert SeriesWindows(src, 8, restoring=3)._restoring.iters == 3
  both = SeriesWindows(src, 64, restoring=64, dfa=True, detrend="gaussian", sigma=5.0)
  assert both._restoring.iters == 64 and both.dfa_scales
  for W_, bad, word in ((7, True, "at least 8"), (4, 10, "at least 8"),
                        (64, 0, "1 to 64 iterations"), (64, -1, "1 to 64 iterations"),
                        (64, 65, "1 to 64 iterations"), (64, False, "True or a number"),
                        (64, 10.0, "integer"), (64, "10", "integer"), (64, (10,), "integer")):
    with pytest.raises(ValueError, match=word):
      restoring_par(W_, bad)
    with pytest.raises(ValueError, match=word):
      SeriesWindows(src, W_, restoring=bad)
  with pytest.raises(ValueError, match="unknown indicator 'lam'"):
    none.across_members("lam")
  with pytest.raises(ValueError, match="one of mean, slope, var, ac, lam"):
    SeriesWindows(src, 64, restoring=True).across_members("skew")
  with pytest.raises(ValueError, match="one of mean, slope, var, ac, dfa, lam"):
    both.across_members("skew")
