"""SeriesShifts, SeriesWindows.significance(until=), pm_series_shift_scan, pm_series_censor and
pm_series_fit_ranged without a device: the restatement (tests/shifts_cases.py) finds a planted
step and nothing in noise; the censored surrogate test stays calibrated where the plain one sees
the step; the restatement's own invariants; the header mirror; every argument check of the
entries and of the classes; the kernels' scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shifts_cases as SHC
import surrogate_cases as SGC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

N = 400


# ------------------------------------------------------------------ detection
def _white(seed, K, step_at=None, size=6.0):
  v = np.random.default_rng(seed).standard_normal((K, 1, N))
  if step_at is not None:
    v[step_at:] -= size
  return v


def test_a_planted_step_is_found_where_it_is():
  """400 white-noise series (sd 1, K = 300, L = 40, drops) with a -6 sd step at record 150: at
  least 390 have |at - 150| <= 3, and with threshold 3 every member has a `first`, at or before
  150.  (A two-pass NumPy check gave 400 and 400; the restatement gives 400 of 400, `at` in
  [149, 150] and `first` in [143, 148].)"""
  r = SHC.detect(_white(31001, 300, 150), 0, 300, 40, [3.0], [-1])
  at, first = r["at"][0], r["first"][0]
  near = int((np.abs(at - 150) <= 3).sum())
  print("|at - 150| <= 3: %d of %d; first in [%d, %d]; at in [%d, %d]"
        % (near, N, first.min(), first.max(), at.min(), at.max()))
  assert near >= 390, near
  assert (first != -1).all() and (first <= 150).all()
  assert (first >= 40).all() and (first <= at).all()
  assert (r["ncand"] == 300 - 2 * 40 + 1).all()
  # the four values at `at`: stat = -score there, jump near -6, the two means either side
  stat, jump, before, after = r["val"][:, 0]
  assert (stat < -3.0).all() and (np.abs(jump + 6.0) < 1.5).all()
  assert np.array_equal(jump, after - before)


def test_noise_alone_reaches_no_threshold():
  """The same without a step: no member reaches threshold 3 (a two-pass NumPy check gave 0 of 400,
  the 95 % quantile of the largest score 0.73; the restatement: maximum 0.910, quantile 0.719)."""
  r = SHC.detect(_white(31002, 300), 0, 300, 40, [3.0], [-1])
  best = -r["val"][0, 0]
  print("largest score: max %.3f, 95 %% quantile %.3f" % (best.max(), np.quantile(best, 0.95)))
  assert (r["first"] == -1).all()
  assert (r["at"] >= 40).all() and (best < 3.0).all()


# ------------------------------------------------------------------ the censored surrogate test
K, W, S, NSUR, STEP_AT, L = 300, 64, 4, 199, 220, 40


def _count(res, key, level=0.1):
  p = res[key]["p_rising"]
  assert np.isfinite(p).all()
  return int((p <= level).sum())


def test_the_censored_test_stays_calibrated():
  """400 stationary AR(1) series (phi = 0.5, unit variance, K = 300) with a -6 sd step at record
  220; L = 40, threshold 3, where = "first"; W = 64, S = 4, linear detrending, 199 surrogates.
  The step is detected in every member, so the censored test sees stationary records only:
  the number of series with p_rising <= 0.1 is Binomial(400, 0.1), asserted in 40 +- 18 (three
  standard deviations) for var and for ac.  The uncensored counts are printed next to them
  (DESIGN.md section 25 records them): the step itself reads as a warning.  Observed: 28 (var) and
  39 (ac) censored, 109 and 124 uncensored."""
  rng = np.random.default_rng(31003)
  v = np.empty((K, 1, N))
  x = rng.standard_normal(N)
  for k in range(K):
    x = 0.5 * x + np.sqrt(0.75) * rng.standard_normal(N)
    v[k, 0] = x
  v[STEP_AT:] -= 6.0
  found = SHC.detect(v, 0, K, L, [3.0], [-1])
  assert (found["first"] != -1).all() and (found["first"] <= STEP_AT).all()
  end = SHC.ends(found["first"], K)
  assert (end >= W).all()
  res = SHC.significance(v, 0, K, W, S, 1, "linear", NSUR, end, seed=79, nb=25)
  plain = SGC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=79, nb=25)
  for key in ("var", "ac"):
    got, unc = _count(res, key), _count(plain, key)
    print("%s: %d of %d series with p_rising <= 0.1 censored, %d uncensored" % (key, got, N, unc))
    assert 22 <= got <= 58, (key, got)
    assert (res[key]["nvalid"] == NSUR).all()


# ------------------------------------------------------------------ the restatement itself
def test_restated_scan_by_hand():
  """Six windows of L = 2 would be below PM_WIN_MIN for the entry; the restatement takes any L.
  Planes by hand: candidates c = 2, 3, 4."""
  mean = np.array([0.0, 1.0, 5.0, 1.0, -3.0, np.nan, 2.0]).reshape(7, 1, 1)
  var = np.array([1.0, 4.0, 1.0, 0.0, 3.0, 1.0, 1.0]).reshape(7, 1, 1)
  # c = 2: jump 5, pooled 1 -> 5;  c = 3: jump 0, pooled 2 -> 0;  c = 4: jump -8, pooled 2;
  # c = 5: mean NaN, left out (7 windows of 2: K = 8, c <= 6: c = 5 and 6 read windows 3..6)
  r = SHC.scan(mean, var, 2, [4.0], [0])
  assert r["ncand"][0, 0] == 4 and r["at"][0, 0] == 4 and r["first"][0, 0] == 2
  assert r["val"][:, 0, 0].tolist() == [-8.0 / np.sqrt(2.0), -8.0, 5.0, -3.0]
  assert SHC.scan(mean, var, 2, [4.0], [1])["at"][0, 0] == 2
  down = SHC.scan(mean, var, 2, [6.0], [-1])
  assert down["at"][0, 0] == 4 and down["first"][0, 0] == -1
  assert SHC.scan(mean, var, 2, [np.nan], [-1])["first"][0, 0] == -1


def test_the_table_holds_what_it_must():
  """Every style in the larger cases; what each style must give."""
  seen = set()
  for c in SHC.cases():
    if c["K"] > 1000 and c["L"] > 1000:
      continue  # (restated on the device side of the suite only: seconds)
    r = SHC.restate(c)
    ncmax = c["K"] - 2 * c["L"] + 1
    for s in range(c["nspec"]):
      for m in range(c["n"]):
        at, nc = r["at"][s, m], r["ncand"][s, m]
        assert (at == -1) == (nc == 0) == bool(np.isnan(r["val"][:, s, m]).all())
        assert nc <= ncmax and (at == -1 or c["L"] <= at <= c["K"] - c["L"])
        if np.isnan(c["thr"][s]):
          assert r["first"][s, m] == -1
    seen |= {SHC.style_of(s, m) for s in range(c["nspec"]) for m in range(c["n"])}
  assert seen == set(SHC.STYLES)
  c = SHC.case(300, 40, 10, 1, 0)  # member m has style m; dir -1, thr 3
  r = SHC.restate(c)
  style = {st: m for m, st in enumerate(SHC.STYLES)}
  assert r["first"][0, style["drop"]] != -1 and r["first"][0, style["noise"]] == -1
  assert 0 < r["ncand"][0, style["nan_some"]] < 221 and r["ncand"][0, style["nan_all"]] == 0
  assert 0 < r["ncand"][0, style["inf1"]] < 221
  for st in ("const", "zeros", "nan_all"):
    assert r["at"][0, style[st]] == -1 and np.isnan(r["val"][:, 0, style[st]]).all()
  m = style["stairs"]   # infinite scores at c = 40, 80, .., 240: the first wins
  assert np.isinf(r["score"][:, 0, m]).sum() == 6 and r["at"][0, m] == 40 == r["first"][0, m]
  assert r["val"][0, 0, m] == -np.inf and r["val"][1, 0, m] == -1.0
  m = style["alt"]      # every score a zero: the first candidate
  assert (r["score"][:, 0, m] == 0.0).all() and r["at"][0, m] == 40 and r["ncand"][0, m] == 221


def test_restated_censor_and_ends():
  c = SHC.censor_case(12, 7, 2, 3, 1)
  assert SHC.ends(np.array([[-1, 0, 5, 12]]), 12).tolist() == [[12, 0, 5, 12]]
  assert SHC.ends(np.array([[-1, 0, 5, 12]]), 12, guard=3).tolist() == [[12, 0, 2, 9]]
  assert SHC.ends(np.array([[1, 2], [-1, 7]]), 9, src=[1, 1]).tolist() == [[9, 7], [9, 7]]
  y, end = SHC.censor(c["x"], c["where"], nb=3)
  xb, yb = c["x"].view(np.uint64), y.view(np.uint64)
  for s in range(2):
    for m in range(7):
      for i in range(3):
        e = end[s, m]
        assert np.array_equal(yb[:e, i * 2 + s, m], xb[:e, i * 2 + s, m])
        assert (yb[e:, i * 2 + s, m] == 0x7ff8000000000000).all()
  assert (xb == 0x7ff8dead0000beef).any() and (yb == 0x7ff8dead0000beef).any()
  none = SHC.censor(c["x"], np.full((2, 7), -1), nb=3)[0]
  assert np.array_equal(none.view(np.uint64), xb)
  gone = SHC.censor(c["x"], np.maximum(c["where"], 0), guard=10**6, nb=3)[0]
  assert np.isnan(gone).all()


def test_restated_ranged_fit_is_the_window_restatement():
  """Per distinct end e the ranged fit equals windows_cases.windows with one window over [k0,
  k0 + e) (for "linear": where windows_cases.stt_of does not floor, e != 2 mod 4)."""
  c = SHC.fit_case(40, 9, 2, 0)
  ends_seen = set(np.unique(c["end"]).tolist())
  assert {0, 3, 4, 40} <= ends_seen
  for det in WC.DETRENDS:
    var, ac = SHC.fit_ranged(c["v"], c["k0"], c["k1"], c["end"], det)
    assert np.isnan(var[c["end"] < 4]).all() and np.isfinite(var).any()
    for e in ends_seen:
      if e < 4 or (det == "linear" and e % 4 == 2):
        continue
      out = WC.windows(c["v"], c["k0"], c["k0"] + e, e, 1, 1, det)["out"]
      sel = c["end"] == e
      assert np.array_equal(var[sel], out[2, 0][sel], equal_nan=True), (det, e)
      assert np.array_equal(ac[sel], out[3, 0][sel], equal_nan=True), (det, e)
    assert np.isnan(var[0, 1]) and np.isfinite(var[0, 2])  # the NaN inside and outside the range
  assert SHC.stt_of(6) == 17.5 and SHC.stt_of(22) == 885.5


def test_restated_composition_without_a_shift_is_the_plain_one():
  """Ends all K: the ranged fit is the one-window fit, the censor keeps everything, and the
  composition is surrogate_cases.significance (K = 36: not 2 mod 4)."""
  c = WC.case(10, 3, 9, 1, 9, 2, "linear", 31)
  K = 36
  kw = dict(v=c["v"], k0=c["k0"], k1=c["k0"] + K, W=10, S=3, Lg=1, detrend="linear", nsur=5, seed=5)
  plain = SGC.significance(**kw)
  same = SHC.significance(end=np.full((2, 9), K, dtype=np.int32), **kw)
  for key in ("var", "ac"):
    for f in ("ge", "le", "nvalid", "tau", "p_rising"):
      assert np.array_equal(same[key][f], plain[key][f], equal_nan=True), (key, f)


# ------------------------------------------------------------------ the C-ABI
def test_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls in (_lib.pm_series_shift_scan, _lib.pm_series_censor, _lib.pm_series_fit_ranged):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert _lib.SIGNATURES[cls.__name__][1][0] is C.POINTER(cls)
  assert _lib.PM_SHIFT_HALF_MAX == SHC.HALF_MAX
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  assert re.search(r"#define PM_SHIFT_HALF_MAX %d\b" % _lib.PM_SHIFT_HALF_MAX, text)


NSPEC = 2
THR = (C.c_double * NSPEC)(3.0, float("nan"))
DIR = (C.c_int32 * NSPEC)(-1, 1)
SRC = (C.c_int32 * NSPEC)(0, 1)
TAB = np.array([SHC.stt_of(w) for w in range(4097)])


def _arr(ctype, *vals):
  return C.addressof((ctype * len(vals))(*vals))


def sdesc(**kw):
  """A valid pm_series_shift_scan descriptor (the device addresses are stand-ins) with the edits."""
  from pymoc_amd import _lib
  d = _lib.pm_series_shift_scan()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.half = 10, NSPEC, 60, 1, 50, 8
  d.mean = d.var = d.thr_dev = d.dir_dev = FAKE
  d.thr, d.dir = C.addressof(THR), C.addressof(DIR)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_scans():
  keep = []  # (the arrays behind the addresses live as long as the list)
  def arr(ctype, *vals):
    keep.append((ctype * len(vals))(*vals))
    return C.addressof(keep[-1])
  out = [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
         ("k0 -1", dict(k0=-1)), ("k0 == k1", dict(k0=50)), ("k1 > nrec", dict(k1=61)),
         ("half 3", dict(half=3)), ("half 2049", dict(half=2049, nrec=9000, k1=9000)),
         ("half 0", dict(half=0)), ("2 half > K", dict(half=25)),
         ("nspec 65536", dict(nspec=65536)),
         ("mean", dict(mean=None)), ("var", dict(var=None)), ("thr", dict(thr=None)),
         ("thr_dev", dict(thr_dev=None)), ("dir", dict(dir=None)), ("dir_dev", dict(dir_dev=None)),
         ("dir 2", dict(dir=arr(C.c_int32, -1, 2))), ("dir -2", dict(dir=arr(C.c_int32, -2, 0))),
         ("thr inf", dict(thr=arr(C.c_double, 1.0, float("inf")))),
         ("thr -inf", dict(thr=arr(C.c_double, float("-inf"), 1.0)))]
  return out, keep


def cdesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_censor()
  d.n, d.nspec, d.K, d.nb, d.guard = 10, NSPEC, 60, 3, 0
  d.x = d.where = d.src_dev = FAKE
  d.src = C.addressof(SRC)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_censors():
  keep = [(C.c_int32 * 2)(0, 2), (C.c_int32 * 2)(-1, 0)]
  out = [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nb 0", dict(nb=0)), ("K 0", dict(K=0)),
         ("K -1", dict(K=-1)), ("guard -1", dict(guard=-1)),
         ("nb * nspec 65536", dict(nb=32768)),
         ("K * nb * nspec 2^31", dict(nb=32767, K=32770)),
         ("nb * nspec * n 2^31", dict(nb=1, nspec=32768, n=65536)),
         ("x", dict(x=None)), ("where", dict(where=None)), ("src", dict(src=None)),
         ("src_dev", dict(src_dev=None)),
         ("src 2", dict(src=C.addressof(keep[0]))), ("src -1", dict(src=C.addressof(keep[1])))]
  return out, keep


def fdesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_fit_ranged()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.detrend = 10, NSPEC, 60, 1, 50, _lib.PM_WIN_DETREND_LINEAR
  d.v = d.end = d.stt_tab_dev = FAKE
  d.stt_tab = TAB.ctypes.data
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_fits():
  floored = np.floor(TAB)   # wrong at W = 2 mod 4
  wrong = TAB.copy()
  wrong[49] += 1.0          # the last entry a window of 49 records reads
  out = [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
         ("k0 -1", dict(k0=-1)), ("k0 == k1", dict(k0=50)), ("k1 > nrec", dict(k1=61)),
         ("K 4097", dict(nrec=5000, k0=0, k1=4097)), ("detrend 3", dict(detrend=3)),
         ("detrend -1", dict(detrend=-1)), ("nspec * n 2^31", dict(nspec=32768, n=65536)),
         ("v", dict(v=None)), ("end", dict(end=None)), ("stt_tab", dict(stt_tab=None)),
         ("stt_tab_dev", dict(stt_tab_dev=None)),
         ("stt floored", dict(stt_tab=floored.ctypes.data)),
         ("stt_tab[49]", dict(stt_tab=wrong.ctypes.data))]
  return out, (floored, wrong)


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  Lb = _lib.lib
  err = lambda: Lb.pm_last_error().decode()
  outs = (FAKE + 64, FAKE + 128, FAKE + 192, FAKE + 256)
  assert Lb.pm_series_shift_scan(None, *outs, None) == _lib.PM_EINVAL
  cases, keep = bad_scans()
  for label, kw in cases:
    d = sdesc(**kw)
    assert Lb.pm_series_shift_scan(C.byref(d), *outs, None) == _lib.PM_EINVAL, label
    assert err(), label
  for i in range(4):
    args = list(outs)
    args[i] = None
    d = sdesc()
    assert Lb.pm_series_shift_scan(C.byref(d), *args, None) == _lib.PM_EINVAL, i
    assert "at, first, ncand or val is NULL" in err()
  d = sdesc(half=25)
  assert Lb.pm_series_shift_scan(C.byref(d), *outs, None) == _lib.PM_EINVAL
  assert "holds 49 records, fewer than 2 * 25" in err()
  # the censor
  assert Lb.pm_series_censor(None, FAKE, FAKE, None) == _lib.PM_EINVAL
  cases, keep = bad_censors()
  for label, kw in cases:
    d = cdesc(**kw)
    assert Lb.pm_series_censor(C.byref(d), FAKE, None, None) == _lib.PM_EINVAL, label
    assert err(), label
  d = cdesc()
  assert Lb.pm_series_censor(C.byref(d), None, FAKE, None) == _lib.PM_EINVAL
  assert "y is NULL" in err()
  d = cdesc(src=C.addressof(keep[0]))
  assert Lb.pm_series_censor(C.byref(d), FAKE, FAKE, None) == _lib.PM_EINVAL
  assert "src[1] = 2 is outside [0, 2)" in err()
  # the ranged fit
  assert Lb.pm_series_fit_ranged(None, FAKE, FAKE, None) == _lib.PM_EINVAL
  cases, keep = bad_fits()
  for label, kw in cases:
    d = fdesc(**kw)
    assert Lb.pm_series_fit_ranged(C.byref(d), FAKE, FAKE + 64, None) == _lib.PM_EINVAL, label
    assert err(), label
  assert "stt_tab[49]" in err()
  d = fdesc(stt_tab=keep[0].ctypes.data)
  assert Lb.pm_series_fit_ranged(C.byref(d), FAKE, FAKE + 64, None) == _lib.PM_EINVAL
  assert "stt_tab[6] = 17 is not" in err()
  for args in ((None, FAKE), (FAKE, None)):
    d = fdesc()
    assert Lb.pm_series_fit_ranged(C.byref(d), *args, None) == _lib.PM_EINVAL
    assert "var or ac is NULL" in err()


def test_kernels_cross_compile_without_scratch(tmp_path):
  """k_series_shift_scan, k_series_censor and the three k_series_fit_ranged for gfx950: 0 bytes of
  scratch, no spill; LDS in the scan alone (DESIGN.md section 25 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "shifts.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "shifts.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_(?:shift_scan|censor|fit_ranged)\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  spills = [int(x) for x in re.findall(r"[SV]GPRs Spill: (\d+)", p.stdout)]
  lds = dict(zip(names, (int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout))))
  assert len(set(names)) == 5 and len(scratch) == 5 and len(spills) == 10
  assert all(x == 0 for x in scratch + spills), list(zip(names, scratch))
  assert all((b == 5120) if "shift_scan" in nm else (b == 0) for nm, b in lds.items()), lds


# ------------------------------------------------------------------ the classes
def test_classes_validate_their_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call, which
  on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesShifts, SeriesWindows
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  ok = SeriesShifts(src, 10)
  assert ok.half == 10 and ok.direction.tolist() == [-1, -1] and np.isnan(ok.threshold).all()
  sh = SeriesShifts(src, 10, direction=dict(wind=1), threshold=dict(amoc=3))
  assert sh.direction.tolist() == [1, -1] and sh.direction.dtype == np.int32
  assert np.isnan(sh.threshold[0]) and sh.threshold[1] == 3.0
  assert SeriesShifts(src, 4, direction=0, threshold=2.5).threshold.tolist() == [2.5, 2.5]
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"])):
    with pytest.raises(ValueError, match="series"):
      SeriesShifts(bad, 4)
  with pytest.raises(ValueError, match="nspec = 65536 is above 65535"):
    SeriesShifts((_Series((100, 65536, 1)), range(65536)), 4)
  for half in (3, 2049, 0, -4, 8.0, "8", True, None):
    with pytest.raises(ValueError, match="half"):
      SeriesShifts(src, half)
  for d in (2, -2, 1.0, "down", None, True, dict(wind=5), dict(gulf=1)):
    with pytest.raises(ValueError, match="direction"):
      SeriesShifts(src, 10, direction=d)
  for t in (float("inf"), -float("inf"), "3", True, dict(amoc=float("inf")), dict(gulf=1.0)):
    with pytest.raises(ValueError, match="threshold"):
      SeriesShifts(src, 10, threshold=t)
  for k0, k1 in ((-1, 40), (40, 40), (50, 20), (0, 101)):
    with pytest.raises(ValueError, match="window"):
      ok.detect(k0, k1)
  with pytest.raises(ValueError, match=r"window \[10, 29\) holds 19 records, fewer than 2 \* half = 20"):
    ok.detect(10, 29)
  need = 32 * 91 * 2 * 6
  with pytest.raises(ValueError, match="scratch of %d bytes .* exceeds max_bytes = %d" % (need, need - 1)):
    ok.detect(max_bytes=need - 1)
  for mb in (1e9, None, "1"):
    with pytest.raises(ValueError, match="max_bytes"):
      ok.detect(max_bytes=mb)
  with pytest.raises(ValueError, match=r"censored\(\) needs detect\(\) first"):
    ok.censored()
  sw = SeriesWindows(src, 32, step=4)
  with pytest.raises(ValueError, match=r"until needs detect\(\) and censored\(\)"):
    sw.significance(until=ok)
  ok._found, ok.first_dev, ok.at_dev = (0, 100), _Series((2, 6), np.int32), _Series((2, 6), np.int32)
  for kw in (dict(where="last"), dict(where=None), dict(guard=-1), dict(guard=1.0), dict(guard=True),
             dict(by="gulf"), dict(by=0)):
    with pytest.raises(ValueError, match="|".join(kw)):
      ok.censored(**kw)
  with pytest.raises(ValueError, match=r"until needs detect\(\) and censored\(\)"):
    sw.significance(until=ok)
  ok._cens = ok.end = object()
  with pytest.raises(ValueError, match=r"until detected over the record window \[0, 100\), not \[5, 100\)"):
    sw.significance(5, 100, until=ok)
  other = SeriesWindows((_Series((100, 2, 7)), ["wind", "amoc"]), 32, step=4)
  with pytest.raises(ValueError, match="until was made for another series"):
    other.significance(until=ok)
  renamed = SeriesWindows((_Series((100, 2, 6)), ["wind", "gulf"]), 32, step=4)
  with pytest.raises(ValueError, match="until was made for another series"):
    renamed.significance(until=ok)
  # the checks of the plain call come first, as without `until`
  with pytest.raises(ValueError, match="nsur"):
    sw.significance(nsur=0, until=ok)
