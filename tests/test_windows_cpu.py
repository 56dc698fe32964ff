"""SeriesWindows, pm_series_windows and pm_series_kendall without a device: the case tables; the
restatement (tests/windows_cases.py) against an extended-precision evaluation of the same
definitions, against scipy.signal.detrend and against scipy.stats.kendalltau; the header mirror;
every argument check of the entries and of SeriesWindows; the kernels' scratch."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import windows_cases as WC
from test_steady_cpu import _layout

U = 2.0**-53
LD = np.longdouble
CASES = WC.cases()
IDS = [c["name"] for c in CASES]
KCASES = WC.kendall_cases()


def test_table_holds_what_it_must():
  from pymoc_amd import _lib
  assert {c["W"] for c in CASES} >= {4, 5, 64, 65, 257, 4096}
  for W in (4, 5, 64, 65, 257, 4096):
    steps = sorted({c["S"] for c in CASES if c["W"] == W})
    assert steps[0] == 1 and steps[2] == W and abs(steps[1] - W / 2) <= 1, (W, steps)
  assert {c["nwin"] for c in CASES} == {1, 2, 5, WC.MANY, WC.LONG}
  assert {c["v"].shape[2] for c in CASES} == {1, 7, 64, 65}
  assert {c["v"].shape[1] for c in CASES} == {1, 3}
  assert {c["detrend"] for c in CASES} == {"linear", "constant", "none"}
  assert {c["Lg"] for c in CASES} >= {1, 3} and {c["Lg"] == c["W"] - 2 for c in CASES} == {True, False}
  # the tiles: every width, one case that gives a block more windows than it takes, and one whose
  # blocks stage nearly all of a CU's LDS
  tm, nwb, tiles = C.c_int32(0), C.c_int32(0), {}
  for c in CASES:
    assert _lib.lib.pm_series_windows_geometry(c["W"], c["S"], C.byref(tm), C.byref(nwb)) == 0
    tiles[c["name"]] = (tm.value, nwb.value, c["W"] + (min(nwb.value, c["nwin"]) - 1) * c["S"])
  assert {t[0] for t in tiles.values()} == {32, 16, 8, 4}
  many = [tiles[c["name"]] for c in CASES if c["nwin"] == WC.MANY]
  assert many and all(t[0] == 32 and t[1] < WC.MANY < 2 * t[1] for t in many)
  assert max(8 * t[2] * t[0] for t in tiles.values()) > 150 * 1024
  for c in CASES:
    K, W, S = c["k1"] - c["k0"], c["W"], c["S"]
    assert c["k0"] > 0 and c["k1"] < c["v"].shape[0]
    assert WC.nwin_of(K, W, S) == c["nwin"] and 1 <= c["Lg"] <= W - 2
    assert K - (W + (c["nwin"] - 1) * S) == min(S - 1, 3)  # the tail that fits no window
    assert c["v"].shape[1] * c["v"].shape[2] <= 195
    # the styles: one NaN / inf inside exactly one window, members with every window spoiled
    r = WC.restate(c)
    used, (mean, slope, var, ac) = r["used"], r["out"]
    for s in range(c["v"].shape[1]):
      for m in range(c["v"].shape[2]):
        st, x = WC.style_of(s, m), c["v"][c["k0"]:c["k1"], s, m]
        if st in WC.FINITE_STYLES:
          assert used[:, s, m].all() and np.isfinite(x).all()
          assert np.isfinite(mean[:, s, m]).all() and np.isfinite(var[:, s, m]).all()
        elif st == "nan1":
          assert np.isnan(x).sum() == 1 and used[:, s, m].tolist() == [False] + [True] * (c["nwin"] - 1)
        elif st == "inf1":
          assert np.isinf(x).sum() == 1 and used[:, s, m].tolist() == [True] * (c["nwin"] - 1) + [False]
        else:
          assert not used[:, s, m].any() and r["nused"][s, m] == 0
        assert np.array_equal(np.isnan(mean[:, s, m]), ~used[:, s, m])
        if st == "big":
          assert 1e149 < np.abs(x).max() < 1e152
        if st == "small":
          assert 1e-151 < np.abs(x).max() < 1e-149
        if st == "zeros" or (st == "const" and c["detrend"] != "none"):  # q == 0
          assert np.isnan(ac[:, s, m]).all()
          assert (var[:, s, m] == 0.0).all() and not np.signbit(var[:, s, m]).any()
        if st == "zeros":
          assert np.signbit(x).any() and not np.signbit(x).all() and not x.any()
        if st == "ramp" and c["detrend"] == "linear":
          assert np.abs(slope[:, s, m] - 0.25).max() <= 1e-12
  assert any(c["nwin"] > 1 and c["v"].shape[2] >= 9 for c in CASES)
  # the Kendall table
  assert {c["k1"] - c["k0"] for c in KCASES} == {1, 2, 64, 65, 300, 1000, 4096}
  for c in KCASES:
    assert c["k0"] > 0 and c["k1"] < c["v"].shape[0]
    conc, disc, tie, nfin = WC.kendall(c["v"], c["k0"], c["k1"])
    K = c["k1"] - c["k0"]
    assert (conc + disc + tie == nfin.astype(np.int64) * (nfin - 1) // 2).all()
    for s in range(c["v"].shape[1]):
      for m in range(c["v"].shape[2]):
        st, got = WC.k_style_of(s, m), (conc[s, m], disc[s, m], tie[s, m], nfin[s, m])
        if st == "equal":
          assert got == (0, 0, K * (K - 1) // 2, K)
        elif st == "rising":
          assert got == (K * (K - 1) // 2, 0, 0, K)
        elif st == "none":
          assert got == (0, 0, 0, 0)
        elif st == "noise":
          assert tie[s, m] == 0 and nfin[s, m] == K
        elif K >= 64:
          assert tie[s, m] > 0 and (st == "ties" or 0 < nfin[s, m] < K)


def test_restatement_on_windows_worked_by_hand():
  v = np.array([1.0, 2.0, 4.0, 8.0, 16.0]).reshape(5, 1, 1)
  r = WC.windows(v, 0, 5, 4, 1, 1, "linear")["out"][:, :, 0, 0]
  # window 0: x = 1 2 4 8, t = -1.5 -.5 .5 1.5, mean 3.75, st = 11.5, stt = 5, slope 2.3
  assert r[0].tolist() == [3.75, 7.5] and r[1].tolist() == [11.5 / 5.0, 23.0 / 5.0]
  res = np.array([1.0, 2.0, 4.0, 8.0]) - 3.75 - 2.3 * np.array([-1.5, -0.5, 0.5, 1.5])
  assert abs(r[2, 0] - (res * res).sum() / 3.0) < 1e-15
  assert abs(r[3, 0] - (res[:-1] * res[1:]).sum() / (res * res).sum()) < 1e-15
  c = WC.windows(v, 0, 5, 4, 1, 2, "constant")["out"][:, 0, 0, 0]
  d = np.array([1.0, 2.0, 4.0, 8.0]) - 3.75
  assert c.tolist() == [3.75, 0.0, (d * d).sum() / 3.0, (d[0] * d[2] + d[1] * d[3]) / (d * d).sum()]
  n = WC.windows(v, 1, 5, 4, 4, 1, "none")["out"][:, 0, 0, 0]
  assert n.tolist() == [7.5, 0.0, 340.0 / 3.0, (8.0 + 32.0 + 128.0) / 340.0]
  assert WC.stt_of(4) == 5.0 and WC.stt_of(4096) == float(sum((2 * j - 4095) ** 2 for j in range(4096)) // 4)
  # 43 windows with 641 concordant and 262 discordant pairs
  assert abs(WC.tau_b(641, 262, 0) - 0.41971207087486) < 1e-14


# ------------------------------------------------------------------ the two authorities
def c_var(W):
  """|var' - var| / var <= c_var(W) u (1 + kappa), to first order."""
  return 5 * W + 18


def c_ac(W):
  """|ac' - ac| <= c_ac(W) u (1 + kappa), to first order."""
  return 10 * W + 34


def _ld_windows(x, Lg, detrend):
  """(mean, slope, q, c, rms(r), max |x|) of the windows x [..., W] in longdouble (pairwise sums)."""
  W = x.shape[-1]
  xl = x.astype(LD)
  t = np.arange(W).astype(LD) - LD(W - 1) / 2
  mean = xl.sum(axis=-1) / W
  slope = (xl * t).sum(axis=-1) / (t * t).sum() if detrend == "linear" else np.zeros_like(mean)
  if detrend == "none":
    r = xl
  else:
    r = (xl - mean[..., None]) - slope[..., None] * t
  q = (r * r).sum(axis=-1)
  c = (r[..., :W - Lg] * r[..., Lg:]).sum(axis=-1)
  return mean, slope, q, c, np.sqrt(q / W), np.abs(xl).max(axis=-1)


def _degenerate(st, detrend):
  """Styles whose exact residual is zero: kappa is infinite and var, ac are pure rounding."""
  return st == "zeros" or (st == "const" and detrend != "none") or (st == "ramp" and detrend == "linear")


@functools.lru_cache(maxsize=None)
def _ratios(ci, scipy_route):
  """The largest error of the restatement over the case, each as a multiple of its bound: mean and
  slope against their own forward bounds, var (relative) and ac (absolute) against
  c(W) u (1 + kappa) (1 + the same): the quadratic term of the derivation.  scipy_route: the
  distance to scipy.signal.detrend plus the direct formulas instead, against twice the bound."""
  import scipy.signal
  c = CASES[ci]
  W, Lg, det = c["W"], c["Lg"], c["detrend"]
  x = WC.window_values(c["v"], c["k0"], c["k1"], W, c["S"])
  r = WC.restate(c)
  mean, slope, var, ac = r["out"]
  worst = dict(mean=0.0, slope=0.0, var=0.0, ac=0.0)
  t = np.arange(W) - 0.5 * (W - 1)
  for s in range(x.shape[1]):
    for m in range(x.shape[2]):
      st = WC.style_of(s, m)
      use = r["used"][:, s, m]
      if not use.any():
        continue
      xs = x[use, s, m]
      lm, ls, lq, lc, rms, top = _ld_windows(xs, Lg, det)
      gm, gs, gv, ga = (a[use, s, m] for a in (mean, slope, var, ac))
      if not scipy_route and st != "zeros":
        # s: (W - 1) u sum |x|, the division one more u: W u max |x|; st alike over t_j x_j
        worst["mean"] = max(worst["mean"], float((np.abs(gm - lm) / (W * U * top)).max()))
        if det == "linear":
          bs = (W + 2) * U * top * LD(np.abs(t).sum()) / LD(WC.stt_of(W))
          worst["slope"] = max(worst["slope"], float((np.abs(gs - ls) / bs).max()))
      if _degenerate(st, det):
        continue
      kappa = top / rms
      bv, ba = (cw * U * (1 + kappa) for cw in (c_var(W), c_ac(W)))
      bv, ba = bv * (1 + bv), ba * (1 + ba)
      if scipy_route:
        res = xs if det == "none" else scipy.signal.detrend(xs, axis=-1, type=det)
        q = (res * res).sum(axis=-1)
        ev = np.abs(gv - q / (W - 1)) / (q / (W - 1)) / (2 * bv)
        ea = np.abs(ga - (res[:, :W - Lg] * res[:, Lg:]).sum(axis=-1) / q) / (2 * ba)
      else:
        ev = np.abs(gv - lq / (W - 1)) / (lq / (W - 1)) / bv
        ea = np.abs(ga - lc / lq) / ba
      worst["var"] = max(worst["var"], float(ev.max()))
      worst["ac"] = max(worst["ac"], float(ea.max()))
  return worst


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_restatement_against_the_longdouble_evaluation(ci):
  """Every error within its derived bound: mean W u max|x|, slope
  (W + 2) u max|x| sum|t| / stt, var (relative) (5 W + 18) u (1 + kappa), ac (absolute)
  (10 W + 34) u (1 + kappa), kappa = max|x| / rms(r) of the window.  Largest observed fraction of
  the bound over the table: mean 0.45, slope 0.16, var 0.021, ac 0.012 (all at W = 4 or 5, where
  the bound is tightest); at W = 4096 var 0.00035, ac 0.00026 -- the bound grows with W, the error
  of a sum of terms of either sign hardly does."""
  w = _ratios(ci, False)
  print("%s: fractions of the bound: %s" % (CASES[ci]["name"], w))
  for key, val in w.items():
    assert val <= 1.0, (key, val)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_restatement_against_scipy_detrend(ci):
  """scipy.signal.detrend(type="linear" / "constant") and the direct formulas on its residuals:
  both routes lie within the bound of the exact value, so within twice the bound of each other."""
  w = _ratios(ci, True)
  print("%s: fractions of twice the bound: %s" % (CASES[ci]["name"], w))
  assert w["var"] <= 1.0 and w["ac"] <= 1.0, w


@pytest.mark.parametrize("case", KCASES, ids=[c["name"] for c in KCASES])
def test_tau_against_scipy_kendalltau(case):
  import scipy.stats
  from pymoc_amd.windows import tau_b
  c = case
  conc, disc, tie, nfin = WC.kendall(c["v"], c["k0"], c["k1"])
  tau = tau_b(conc, disc, tie)
  assert np.array_equal(tau, WC.tau_b(conc, disc, tie), equal_nan=True)
  for s in range(c["v"].shape[1]):
    for m in range(c["v"].shape[2]):
      x = c["v"][c["k0"]:c["k1"], s, m]
      x = x[np.isfinite(x)]
      assert x.size == nfin[s, m]
      n0 = x.size * (x.size - 1) // 2
      if n0 == tie[s, m]:
        assert np.isnan(tau[s, m])
        continue
      want = scipy.stats.kendalltau(np.arange(x.size), x).statistic
      assert abs(tau[s, m] - want) <= 4 * U, (c["name"], s, m, tau[s, m], want)


# ------------------------------------------------------------------ the C-ABI
def test_windows_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls, entry in ((_lib.pm_series_windows, "pm_series_windows"),
                     (_lib.pm_series_kendall, "pm_series_kendall")):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert _lib.SIGNATURES[entry][1][0] is C.POINTER(cls)
  assert (_lib.PM_WIN_MIN, _lib.PM_WIN_MAX, _lib.PM_KENDALL_MAX) == (WC.WIN_MIN, WC.WIN_MAX,
                                                                    WC.KENDALL_MAX)
  assert (_lib.PM_WIN_DETREND_NONE, _lib.PM_WIN_DETREND_CONSTANT, _lib.PM_WIN_DETREND_LINEAR) == (
      0, 1, 2)
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  for name in ("PM_WIN_MIN", "PM_WIN_MAX", "PM_KENDALL_MAX", "PM_WIN_DETREND_NONE",
               "PM_WIN_DETREND_CONSTANT", "PM_WIN_DETREND_LINEAR"):
    assert re.search(r"#define %s %d\b" % (name, getattr(_lib, name)), text), name


def test_geometry_of_a_block():
  """The tile pm_series_windows_geometry reports fits the LDS of a CU, whatever (W, S)."""
  from pymoc_amd import _lib
  tm, nwb = C.c_int32(0), C.c_int32(0)
  for W in (4, 5, 64, 255, 256, 257, 1024, 1025, 2048, 2049, 4096):
    for S in sorted({1, 2, max(W // 2, 1), W - 1, W}):
      assert _lib.lib.pm_series_windows_geometry(W, S, C.byref(tm), C.byref(nwb)) == _lib.PM_OK
      assert tm.value in (4, 8, 16, 32) and nwb.value >= 1
      span = W + (nwb.value - 1) * S
      assert 8 * span * tm.value + 4 * tm.value <= 160 * 1024, (W, S)
      assert nwb.value % (1024 // tm.value) == 0 or nwb.value < 1024 // tm.value, (W, S)
      if nwb.value >= 1024 // tm.value:  # every thread busy: a byte is fetched at most 6 times
        assert span <= 6 * nwb.value * S, (W, S)
  for W, S in ((3, 1), (4097, 1), (8, 0), (8, 9)):
    assert _lib.lib.pm_series_windows_geometry(W, S, C.byref(tm), C.byref(nwb)) == _lib.PM_EINVAL
  assert _lib.lib.pm_series_windows_geometry(8, 1, None, C.byref(nwb)) == _lib.PM_EINVAL


def test_kernels_cross_compile_without_scratch(tmp_path):
  """Every instantiation of k_series_windows (3 detrends x lag 1 or any) and k_series_kendall for
  gfx950: 0 bytes of scratch (DESIGN.md section 21 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "windows.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "windows.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_(?:windows|kendall)\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  assert len(set(names)) == 7 and len(scratch) >= 7
  assert all(x == 0 for x in scratch), list(zip(names, scratch))


FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first


def desc(**kw):
  """A valid pm_series_windows descriptor (the device address is a stand-in) with the edits `kw`;
  stt follows the window length unless it is given."""
  from pymoc_amd import _lib
  d = _lib.pm_series_windows()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = 10, 2, 60, 1, 50
  d.window, d.step, d.lag, d.detrend, d.v = 16, 8, 1, _lib.PM_WIN_DETREND_LINEAR, FAKE
  for k, v in kw.items():
    setattr(d, k, v)
  if "stt" not in kw:
    d.stt = WC.stt_of(d.window) if d.window > 0 else 0.0
  return d


def bad_descriptors():
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)),
          ("k0 > k1", dict(k0=40, k1=20)), ("k1 > nrec", dict(k1=61)),
          ("W 3", dict(window=3, step=1)), ("W 0", dict(window=0)), ("W -16", dict(window=-16)),
          ("W 4097", dict(window=4097, nrec=9000, k1=8000)),
          ("K < W", dict(k0=40)), ("K = W - 1", dict(k0=35)),
          ("step 0", dict(step=0)), ("step -1", dict(step=-1)), ("step W + 1", dict(step=17)),
          ("lag 0", dict(lag=0)), ("lag -1", dict(lag=-1)), ("lag W - 1", dict(lag=15)),
          ("lag W", dict(lag=16)),
          ("detrend 3", dict(detrend=3)), ("detrend -1", dict(detrend=-1)),
          ("stt 0", dict(stt=0.0)), ("stt nan", dict(stt=float("nan"))),
          ("stt off by an ulp", dict(stt=float(np.nextafter(WC.stt_of(16), np.inf)))),
          ("stt of another W", dict(stt=WC.stt_of(17))),
          ("v", dict(v=None)),
          ("nwin * nspec", dict(nspec=60000, nrec=1 << 15, k1=1 << 15, step=1)),
          ("nspec 65536", dict(nspec=65536)),
          # 2^29 tiles of 4 members x 4 chunks of one window each
          ("tiles * chunks", dict(n=2**31 - 1, window=4096, step=4096, nrec=20000, k1=20000))]


def kdesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_kendall()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.v = 10, 2, 60, 1, 50, FAKE
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_kendall_descriptors():
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)), ("k0 > k1", dict(k0=40, k1=20)),
          ("k1 > nrec", dict(k1=61)), ("K 4097", dict(nrec=5000, k0=3, k1=4100)),
          ("nspec 65536", dict(nspec=65536)), ("v", dict(v=None))]


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  out = (FAKE + 64, FAKE + 128)
  assert L.pm_series_windows(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(**kw)
    assert L.pm_series_windows(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc()
  for args in ((None, out[1]), (out[0], None)):
    assert L.pm_series_windows(C.byref(d), *args, None) == _lib.PM_EINVAL
  d = desc(stt=5.0)
  assert L.pm_series_windows(C.byref(d), *out, None) == _lib.PM_EINVAL
  assert "stt" in L.pm_last_error().decode()
  d = desc(**dict(bad_descriptors())["tiles * chunks"])
  assert L.pm_series_windows(C.byref(d), *out, None) == _lib.PM_EINVAL
  assert "member tiles * window chunks = 2147483648" in L.pm_last_error().decode()
  kout = (FAKE + 64, FAKE + 128, FAKE + 192, FAKE + 256)
  assert L.pm_series_kendall(None, *kout, None) == _lib.PM_EINVAL
  for label, kw in bad_kendall_descriptors():
    d = kdesc(**kw)
    assert L.pm_series_kendall(C.byref(d), *kout, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = kdesc()
  for i in range(4):
    args = list(kout)
    args[i] = None
    assert L.pm_series_kendall(C.byref(d), *args, None) == _lib.PM_EINVAL, i


# ------------------------------------------------------------------ SeriesWindows
class _Series(object):
  """A stand-in for a device series: a shape and a dtype, no memory."""

  def __init__(self, shape, dtype=np.float64):
    self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), 0


class _Recorder(object):
  """A stand-in for an IndexRecorder: what SeriesWindows reads off one."""

  class _T(object):
    names = ["wind", "amoc"]

  class _E(object):
    stream = timer = None

  def __init__(self, written):
    self._values, self.table, self.ens = _Series((len(written), 2, 6)), self._T(), self._E()
    self.steps = np.where(written, np.arange(len(written)) * 12, -1)


def test_series_windows_validates_its_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call, which
  on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesWindows
  from pymoc_amd import windows as W
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  ok = SeriesWindows(src, 32, step=4, groups=[5, 5, 9, 9, 5, 1])
  assert (ok.window, ok.step, ok.lag, ok.detrend, ok.stt) == (32, 4, 1, "linear", WC.stt_of(32))
  assert ok.nwin() == 18 and ok.nwin(3, 50) == 4 and ok.nwin(0, 32) == 1
  assert ok.record_end(3, 50).tolist() == [34, 38, 42, 46]
  assert SeriesWindows(src, 4, step=4, detrend="none", lag=2).nwin() == 25
  assert SeriesWindows(src, 5, detrend="constant", lag=3).nwin(1) == 95
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"]),
              (_Series((10, 0, 6)), []), (_Series((10, 2, 6)),)):
    with pytest.raises(ValueError, match="series|source"):
      SeriesWindows(bad, 8)
    with pytest.raises(ValueError, match="series|source"):
      W.kendall(bad)
  for names in (["amoc"], ["amoc", "amoc"], ["a", "b", "c"]):
    with pytest.raises(ValueError, match="names"):
      SeriesWindows((_Series((10, 2, 6)), names), 8)
  with pytest.raises(ValueError, match="nspec = 65536 is above 65535"):
    SeriesWindows((_Series((100, 65536, 1)), range(65536)), 8)
  for w in (3, 0, -8, 4097, 8.0, "8", True, None):
    with pytest.raises(ValueError, match="window"):
      SeriesWindows(src, w)
  for st in (0, -1, 33, 1.5, "1", False):
    with pytest.raises(ValueError, match="step"):
      SeriesWindows(src, 32, step=st)
  for lg in (0, -1, 31, 32, 1.0, None):
    with pytest.raises(ValueError, match="lag"):
      SeriesWindows(src, 32, lag=lg)
  for det in ("quadratic", None, True, 2):
    with pytest.raises(ValueError, match="detrend"):
      SeriesWindows(src, 32, detrend=det)
  for groups in (np.zeros(5, int), np.zeros(6), 3):
    with pytest.raises(ValueError, match="groups"):
      SeriesWindows(src, 32, groups=groups)
  calls = (ok.compute, ok.trend, ok.nwin, ok.record_end,
           lambda *a: ok.across_members("ac", *a))
  for k0, k1 in ((-1, 40), (40, 40), (50, 20), (0, 101), (100, None)):
    for call in calls:
      with pytest.raises(ValueError, match="window"):
        call(k0, k1)
    with pytest.raises(ValueError, match="window"):
      W.kendall(src, k0, k1)
  with pytest.raises(ValueError, match=r"window \[70, 100\) holds 30 records, fewer than the window length 32"):
    ok.compute(70)
  for call in calls:
    with pytest.raises(ValueError, match="fewer than the window length"):
      call(0, 31)
  with pytest.raises(ValueError, match="unknown indicator 'skew'"):
    ok.across_members("skew")
  big = SeriesWindows((_Series((5000, 1, 1)), ["amoc"]), 4)
  assert big.nwin() == 4997 and big.nwin(0, 4099) == 4096
  with pytest.raises(ValueError, match="holds 4997 windows, more than 4096"):
    big.trend()
  with pytest.raises(ValueError, match="holds 4097 records, more than 4096"):
    W.kendall((_Series((5000, 1, 1)), ["amoc"]), 3, 4100)
  nspec = 40000
  wide = SeriesWindows((_Series((1 << 15, nspec, 1)), range(nspec)), 4)
  with pytest.raises(ValueError, match=r"nwin \* nspec = %d is not below 2\^30" % (((1 << 15) - 3) * nspec)):
    wide.compute()
  # a recorder: the records never written
  rec = _Recorder(np.arange(40) < 36)
  sw = SeriesWindows(rec, 16)
  assert sw.names == ["wind", "amoc"] and (sw.nrec, sw.nspec, sw.n) == (40, 2, 6)
  for call in (sw.compute, sw.trend, lambda *a: sw.across_members("var", *a),
               lambda *a: W.kendall(rec, *a)):
    with pytest.raises(ValueError, match=r"window \[0, 40\) holds record 36, which was never written"):
      call()
    with pytest.raises(ValueError, match="record 36"):
      call(10, 37)
  assert sw.nwin(0, 36) == 21
