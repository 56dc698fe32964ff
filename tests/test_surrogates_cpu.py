"""SeriesSurrogates, SeriesWindows.significance, pm_series_surrogates and pm_series_exceed without a
device: the restatement (tests/surrogate_cases.py) is calibrated under its null model and has
power against a rising autocorrelation; its invariances; the header mirror; every argument check
of the entries and of the classes; the kernels' scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surrogate_cases as SGC
import windows_cases as WC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

N, K, W, S, NSUR = 400, 200, 50, 5, 199


def _stationary(rng, phi):
  """[K, 1, N]: stationary AR(1) series of unit marginal variance; phi a number or [K]."""
  phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))
  v = np.empty((K, 1, N))
  x = rng.standard_normal(N)
  for k in range(K):
    x = phi[k] * x + np.sqrt(1.0 - phi[k] * phi[k]) * rng.standard_normal(N)
    v[k, 0] = x
  return v


def _count(res, key, which="p_rising", level=0.1):
  p = res[key][which]
  assert np.isfinite(p).all()
  return int((p <= level).sum())


def test_the_test_is_calibrated():
  """400 stationary AR(1) series (phi = 0.5, K = 200) plus a constant and a linear trend, W = 50,
  S = 5, linear detrending, 199 surrogates: under the null model p_rising is uniform, so the
  number of series with p_rising <= 0.1 is Binomial(400, 0.1) -- mean 40, sd 6; asserted within
  5 sd, [10, 70], for var and for ac.  (A NumPy stand-in with NumPy's own generator gave 32 to 48
  over three seeds; this test draws the surrogates' deviates from the restated Philox stream.)"""
  rng = np.random.default_rng(20081)
  v = _stationary(rng, 0.5) + 3.0 + 0.01 * np.arange(K)[:, None, None]
  res = SGC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=77, nb=25)
  for key in ("var", "ac"):
    got = _count(res, key)
    print("%s: %d of %d series with p_rising <= 0.1" % (key, got, N))
    assert 10 <= got <= 70, (key, got)
    assert (res[key]["nvalid"] == NSUR).all()


def test_the_test_has_power():
  """400 series whose AR coefficient ramps linearly 0.1 -> 0.9 at unit marginal variance: at least
  200 have ac.p_rising <= 0.1 (a NumPy stand-in gave 342 to 350).  var is flat by construction and
  not asserted."""
  rng = np.random.default_rng(20082)
  v = _stationary(rng, np.linspace(0.1, 0.9, K))
  res = SGC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=78, nb=25)
  got = _count(res, "ac")
  print("ac: %d of %d series with p_rising <= 0.1; var: %d" % (got, N, _count(res, "var")))
  assert got >= 200, got


# ------------------------------------------------------------------ invariances of the restatement
def _small():
  c = WC.case(10, 3, 9, 1, 9, 2, "linear", 31)  # every style of windows_cases, nan1 and const too
  return c, dict(v=c["v"], k0=c["k0"], k1=c["k1"], W=10, S=3, Lg=1, detrend="linear", nsur=9, seed=5)


def _same(a, b, what):
  for key in ("var", "ac"):
    for f in ("ge", "le", "nvalid"):
      assert np.array_equal(a[key][f], b[key][f]), (what, key, f)
    for f in ("tau", "p_rising", "p_falling"):
      assert np.array_equal(a[key][f], b[key][f], equal_nan=True), (what, key, f)


def test_restatement_invariances():
  c, kw = _small()
  whole = SGC.significance(**kw)
  for nb in (1, 4):
    _same(SGC.significance(nb=nb, **kw), whole, "chunks of %d" % nb)
  # a member subset with its ids gives the same rows
  part = SGC.significance(**dict(kw, v=c["v"][:, :, 3:7], ids=np.arange(3, 7)))
  for key in ("var", "ac"):
    for f in ("tau", "ge", "le", "nvalid", "p_rising"):
      assert np.array_equal(part[key][f], whole[key][f][:, 3:7], equal_nan=True), (key, f)
  other = SGC.significance(**dict(kw, v=c["v"][:, :, 3:7]))  # (ids 0 .. 3: other deviates)
  assert not np.array_equal(other["ac"]["ge"], part["ac"]["ge"])
  seen = set()
  for key in ("var", "ac"):
    r = whole[key]
    none = np.isnan(r["tau"]) | (r["nvalid"] == 0)
    seen |= {bool(x) for x in none.ravel()}
    assert none.any() and not none.all()
    for f in ("p_rising", "p_falling"):
      assert np.array_equal(np.isnan(r[f]), none), (key, f)
      p = r[f][~none]
      assert (p >= 1.0 / (kw["nsur"] + 1)).all() and (p <= 1.0).all()
    assert (r["nvalid"][np.isnan(r["tau"])] == 0).all() and (r["nvalid"] <= kw["nsur"]).all()
    assert (r["ge"] + r["le"] >= r["nvalid"]).all()
    assert np.array_equal(r["p_rising"][~none], ((1.0 + r["ge"]) / (1.0 + r["nvalid"]))[~none])
  # a series with a NaN in its record window: a NaN fit, NaN surrogates, nvalid 0
  var, ac = SGC.fit(c["v"], c["k0"], c["k1"], "linear")
  for s in range(2):
    for m in range(9):
      if WC.style_of(s, m) in ("nan1", "inf1", "spoiled", "const", "zeros"):
        assert np.isnan(ac[s, m]) and whole["ac"]["nvalid"][s, m] == 0
      elif WC.style_of(s, m) in ("ar1", "big", "small"):
        assert whole["ac"]["nvalid"][s, m] == kw["nsur"]


def test_restated_surrogates():
  """The recurrence by hand on given deviates; the NaN series; a surrogate depends on (seed, id, b,
  s, j) alone; the moments of the Philox-driven series."""
  var, ac = np.array([[4.0, 1.0, np.nan, 0.0]]), np.array([[0.5, -1.0, 0.2, 0.3]])
  xi = np.arange(1.0, 13.0).reshape(3, 1, 4)
  y = SGC.surrogates(var, ac, 3, 0, 1, 0, np.arange(4), xi=xi)
  g = 2.0 * np.sqrt(0.75)
  assert y[:, 0, 0].tolist() == [2.0, 0.5 * 2.0 + g * 5.0, 0.5 * (0.5 * 2.0 + g * 5.0) + g * 9.0]
  assert y[:, 0, 1].tolist() == [2.0, -2.0, 2.0] and np.isnan(y[:, 0, 2]).all()
  assert not y[:, 0, 3].any()
  var, ac = SGC.fit_values(6, 2, 3)
  whole = SGC.surrogates(var, ac, 12, 0, 7, 9, 2**32 - 3 + np.arange(6, dtype=np.uint64))
  one = SGC.surrogates(var, ac, 12, 5, 1, 9, 2**32 - 3 + np.arange(6, dtype=np.uint64))
  assert np.array_equal(one, whole[:, 10:12], equal_nan=True)
  part = SGC.surrogates(var[:, 3:5], ac[:, 3:5], 12, 0, 7, 9, 2**32 + np.arange(2, dtype=np.uint64))
  assert np.array_equal(part, whole[:, :, 3:5], equal_nan=True)
  # 64 surrogates x 500 members of one long series: the marginal variance and the lag-1 coefficient
  y = SGC.surrogates(np.full((1, 500), 2.0), np.full((1, 500), 0.6), 100, 0, 64, 1, np.arange(500))
  assert abs(y.var() / 2.0 - 1.0) < 0.01 and abs(y.mean()) < 0.01
  assert abs((y[1:] * y[:-1]).mean() / y.var() - 0.6) < 0.01
  assert abs(np.corrcoef(y[:, 0, :].ravel(), y[:, 1, :].ravel())[0, 1]) < 0.02  # surrogates differ


def test_restated_exceed_on_constructed_counts():
  obs, sur = SGC.exceed_case()
  to = SGC.tau(*obs)
  assert to[0, 0] == to[0, 1] == 1.0 / 3.0 and np.isnan(to[0, 3]) and np.isnan(to[0, 4])
  assert np.array_equal(to, WC.tau_b(*obs), equal_nan=True)
  ge, le, nvalid = SGC.exceed(obs, sur)
  # column 0: taus 1/3, NaN, -1/3, 1/3 against 1/3
  assert (ge[0, 0], le[0, 0], nvalid[0, 0]) == (2, 3, 3)
  assert (ge[0, 3], le[0, 3], nvalid[0, 3]) == (0, 0, 0) == (ge[0, 4], le[0, 4], nvalid[0, 4])
  assert (ge[0, 5], le[0, 5], nvalid[0, 5]) == (2, 1, 2)  # -1 against -1, NaN, -0.8, NaN
  # accumulation over two calls equals one call
  two =[a + b for a, b in zip(SGC.exceed(obs, tuple(x[:4] for x in sur)),
                               SGC.exceed(obs, tuple(x[4:] for x in sur)))]
  for a, b in zip(two, (ge, le, nvalid)):
    assert np.array_equal(a, b)


def test_table_holds_what_it_must():
  cases = SGC.cases()
  assert {(c["n"], c["nspec"], c["K"], c["nb"]) for c in cases} == set(SGC.GEOMETRIES)
  assert {c["b0"] for c in cases} == {0, 5} and {c["member0"] for c in cases} == {0, 2**32 - 3}
  assert {(c["b0"], c["member0"]) for c in cases if c["n"] == 5} == {(0, 0), (5, 2**32 - 3)}
  first = cases[0]
  phi, var = first["ac"].ravel(), first["var"].ravel()
  assert 0.0 in phi and (phi < 0).any() and 1.0 in phi and -1.0 in phi and np.isnan(phi).any()
  assert 0.0 in var and np.isinf(var).any()
  with np.errstate(all="ignore"):
    bad = ~(np.isfinite(phi) & np.isfinite(np.sqrt(var)))
  assert np.nonzero(bad)[0].tolist() == list(SGC.NAN_SERIES)
  for c in cases:
    assert (c["member0"] + c["n"] > 2**32) == (c["member0"] > 0)


# ------------------------------------------------------------------ the C-ABI
def test_surrogates_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls, entry in ((_lib.pm_series_surrogates, "pm_series_surrogates"),
                     (_lib.pm_series_exceed, "pm_series_exceed")):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert _lib.SIGNATURES[entry][1][0] is C.POINTER(cls)
  assert _lib.PM_SURROGATE_MAX == SGC.K_MAX == _lib.PM_WIN_MAX
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  assert re.search(r"#define PM_SURROGATE_MAX %d\b" % _lib.PM_SURROGATE_MAX, text)
  assert "{ id_lo, id_hi, b, (s << 12) | j }" in text  # the reuse of the j and stream slots


def desc(**kw):
  """A valid pm_series_surrogates descriptor (the device addresses are stand-ins) with the edits."""
  from pymoc_amd import _lib
  d = _lib.pm_series_surrogates()
  d.n, d.nspec, d.K, d.nb, d.b0, d.member0, d.seed, d.var, d.ac = 10, 2, 60, 3, 0, 0, 1, FAKE, FAKE
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_descriptors():
  """(K * nb * nspec < 2^31 follows from the two limits before it: no descriptor reaches it.)"""
  return [("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("nspec 0", dict(nspec=0)), ("nb 0", dict(nb=0)),
          ("nb -2", dict(nb=-2)), ("K 0", dict(K=0)), ("K -1", dict(K=-1)), ("K 4097", dict(K=4097)),
          ("b0 -1", dict(b0=-1)), ("b0 + nb > 2^32", dict(b0=2**32 - 2)),
          ("b0 2^32", dict(b0=2**32)), ("member0 -1", dict(member0=-1)),
          ("nb * nspec 65536", dict(nb=32768)), ("nspec 65536", dict(nspec=65536, nb=1)),
          ("nb * nspec * n 2^31", dict(nb=1, nspec=32768, n=65536)),
          ("var", dict(var=None)), ("ac", dict(ac=None))]


def edesc(**kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_exceed()
  d.n, d.nspec, d.nb = 10, 2, 3
  for f in ("obs_conc", "obs_disc", "obs_tie", "sur_conc", "sur_disc", "sur_tie"):
    setattr(d, f, FAKE)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_exceed_descriptors():
  return ([("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nb 0", dict(nb=0)), ("nb -1", dict(nb=-1)),
           ("nb * nspec 65536", dict(nb=32768)), ("nb * nspec * n 2^31", dict(nb=1, nspec=32768, n=65536))] +
          [(f, {f: None}) for f in ("obs_conc", "obs_disc", "obs_tie", "sur_conc", "sur_disc", "sur_tie")])


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  assert L.pm_series_surrogates(None, FAKE, FAKE, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(**kw)
    assert L.pm_series_surrogates(C.byref(d), FAKE, FAKE, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc()
  assert L.pm_series_surrogates(C.byref(d), None, FAKE, None) == _lib.PM_EINVAL
  assert "y is NULL" in L.pm_last_error().decode()
  d = desc(b0=2**32 - 2)
  assert L.pm_series_surrogates(C.byref(d), FAKE, None, None) == _lib.PM_EINVAL
  assert "[4294967294, 4294967297)" in L.pm_last_error().decode()
  out = (FAKE + 64, FAKE + 128, FAKE + 192)
  assert L.pm_series_exceed(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_exceed_descriptors():
    d = edesc(**kw)
    assert L.pm_series_exceed(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = edesc()
  for i in range(3):
    args = list(out)
    args[i] = None
    assert L.pm_series_exceed(C.byref(d), *args, None) == _lib.PM_EINVAL, i


def test_stt_of_any_window_length_is_the_value_the_entry_checks():
  """The fit is one window of K records, any K in [4, 4096]: W (W^2 - 1) / 12 ends in .5 for
  W = 2 mod 4, and `windows.stt_of` must give that, not its floor, or pm_series_windows refuses the
  launch."""
  from fractions import Fraction
  from pymoc_amd import _lib
  from pymoc_amd.windows import stt_of
  import test_windows_cpu as TW
  for W in list(range(4, 131)) + [4094, 4095, 4096]:
    exact = sum(Fraction(2 * j - (W - 1), 2) ** 2 for j in range(W))
    assert Fraction(stt_of(W)) == exact, W
  assert stt_of(22) == 885.5 and stt_of(6) == 17.5
  for W in (6, 10, 22, 46, 4094):
    d = TW.desc(window=W, step=1, nrec=9000, k1=8000, stt=stt_of(W))
    assert _lib.lib.pm_series_windows(C.byref(d), None, None, None) == _lib.PM_EINVAL
    assert "out or nused is NULL" in _lib.lib.pm_last_error().decode(), W  # (not stt)


def test_kernels_cross_compile_without_scratch_or_lds(tmp_path):
  """k_series_surrogates (with and without xi_out) and k_series_exceed for gfx950: 0 bytes of
  scratch, no LDS (DESIGN.md section 23 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "surrogates.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "surrogates.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_(?:surrogates|exceed)\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout)]
  assert len(set(names)) == 3 and len(scratch) >= 3 and len(lds) >= 3
  assert all(x == 0 for x in scratch + lds), list(zip(names, scratch, lds))


# ------------------------------------------------------------------ the classes
class _Recorder(object):
  """A stand-in for an IndexRecorder on an ensemble whose first global member is 12."""

  class _T(object):
    names = ["wind", "amoc"]

  class _E(object):
    stream = timer = None
    _member0 = 12

  def __init__(self, nrec):
    self._values, self.table, self.ens = _Series((nrec, 2, 6)), self._T(), self._E()
    self.steps = np.arange(nrec) * 12


def test_classes_validate_their_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call, which
  on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesSurrogates, SeriesWindows
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  ok = SeriesSurrogates(src, seed=2**64 - 1)
  assert (ok.detrend, ok.seed, ok.member0) == ("linear", 2**64 - 1, 0)
  assert SeriesSurrogates(src, member0=7).member0 == 7
  assert SeriesSurrogates(_Recorder(50)).member0 == 12
  assert SeriesSurrogates(_Recorder(50), member0=0).member0 == 0
  assert ok.names_of(5, 2) == ["wind#5", "amoc#5", "wind#6", "amoc#6"]
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"])):
    with pytest.raises(ValueError, match="series"):
      SeriesSurrogates(bad)
  with pytest.raises(ValueError, match="nspec = 65536 is above 65535"):
    SeriesSurrogates((_Series((100, 65536, 1)), range(65536)))
  for det in ("quadratic", None, 2):
    with pytest.raises(ValueError, match="detrend"):
      SeriesSurrogates(src, detrend=det)
  for seed in (-1, 2**64, 1.0, "1", True, None):
    with pytest.raises(ValueError, match="seed"):
      SeriesSurrogates(src, seed=seed)
  for m0 in (-1, 1.5, "0", False):
    with pytest.raises(ValueError, match="member0"):
      SeriesSurrogates(src, member0=m0)
  for k0, k1 in ((-1, 40), (40, 40), (50, 20), (0, 101)):
    for call in (ok.fit, ok.generate):
      with pytest.raises(ValueError, match="window"):
        call(k0, k1)
  with pytest.raises(ValueError, match=r"window \[10, 13\) holds 3 records: the fit takes 4 to 4096"):
    ok.fit(10, 13)
  long = SeriesSurrogates((_Series((5000, 1, 1)), ["amoc"]))
  with pytest.raises(ValueError, match="holds 4097 records"):
    long.generate(3, 4100)
  for b0, nb in ((-1, 1), (0, 0), (0, -3), (2**32 - 1, 2), (1.0, 1), (0, "1"), (0, True)):
    with pytest.raises(ValueError, match="surrogates|b0|nb"):
      ok.generate(0, 50, b0, nb)
  with pytest.raises(ValueError, match=r"nb \* nspec = 65536 is above 65535"):
    ok.generate(0, 50, 0, 32768)
  wide = SeriesSurrogates((_Series((100, 1, 2**20)), ["amoc"]))
  with pytest.raises(ValueError, match=r"nb \* nspec \* n = 2147483648 is not below 2\^31"):
    wide.generate(0, 50, 0, 2048)
  # significance
  sw = SeriesWindows(src, 32, step=4)
  for kw in (dict(nsur=0), dict(nsur=-5), dict(nsur=10.0), dict(nsur="10"), dict(nsur=True),
             dict(seed=-1), dict(seed=1.5), dict(member0=-1), dict(member0=2.0),
             dict(max_bytes=1e9), dict(max_bytes=None)):
    with pytest.raises(ValueError, match="|".join(kw)):
      sw.significance(**kw)
  per = 8 * 100 * 2 * 6
  for mb in (per - 1, 0, -1):
    with pytest.raises(ValueError, match="max_bytes = %d does not hold one surrogate of %d bytes" % (mb, per)):
      sw.significance(max_bytes=mb)
  with pytest.raises(ValueError, match="fewer than the window length"):
    sw.significance(0, 31)
  with pytest.raises(ValueError, match="window"):
    sw.significance(0, 101)
  big = SeriesWindows((_Series((5000, 1, 1)), ["amoc"]), 4)
  with pytest.raises(ValueError, match="holds 4997 windows, more than 4096"):
    big.significance()
  with pytest.raises(ValueError, match="holds 4097 records, more than 4096"):
    SeriesWindows((_Series((5000, 1, 1)), ["amoc"]), 64, step=64).significance(3, 4100)
  from pymoc_amd.surrogates import chunk_size
  assert chunk_size(1000, 2 << 30, 1200, 8, 4096) == 6     # floor(2^31 / 314572800)
  assert chunk_size(1000, 1 << 40, 1200, 8, 4096) == 1000  # all of them
  assert chunk_size(100000, 1 << 50, 10, 8, 4) == 65535 // 8
  assert chunk_size(5, 8 * 10 * 8 * 4, 10, 8, 4) == 1
