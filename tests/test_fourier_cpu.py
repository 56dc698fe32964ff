"""The Fourier phase-randomised surrogates without a device: the restatement
(tests/fourier_cases.py) against an extended-precision direct DFT within a derived bound, its
properties (the periodogram is kept, the imaginary part vanishes, the mean and the Nyquist term
pass through, the phases belong to the surrogate number alone), its calibration and power, the
tables, the header mirror, every argument check of the entries and of the classes, and the
kernels' scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fourier_cases as FC
import noise_cases as NC
import spectra_cases as SC
import surrogate_cases as SGC
from test_steady_cpu import _layout
from test_windows_cpu import FAKE, _Series

CASES = FC.cases()
SMALL = [c for c in CASES if c["K"] <= 1200]


def _finite(c):
  """The (index, member) series of a case whose K records are all finite: [nspec, n] bool."""
  return np.isfinite(c["v"][c["k0"]:c["k1"]]).all(axis=0)


# ------------------------------------------------------------------ 1. the accuracy bound
def _norm2(*parts):
  """The 2-norm over the last axis of the vector with the given real parts, in np.longdouble."""
  return np.sqrt(sum((p.astype(np.longdouble) ** 2).sum(axis=-1) for p in parts))


def _frac(err, lim):
  """The largest err / lim (0 where both vanish: a zero series is reproduced exactly)."""
  assert (err[lim == 0] == 0).all()
  return float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0.0)))


def _parts(c):
  """Of the finite series of a case: the residual r [series, K], coef [2, nf, series], the rotated
  spectrum Z and the synthesis with its imaginary part, each (re, im) [nb, series, K]."""
  K, ok = c["K"], _finite(c)
  r, _ = FC.residual(c["v"], c["k0"], c["k1"], c["detrend"])
  coef = FC.coefficients(c["v"], c["k0"], c["k1"], c["detrend"])
  ids = FC.ids_of(c)
  Zr, Zi = FC.spectrum(coef, K, c["b0"], c["nb"], c["seed"], ids)
  yr, yi = FC.synthesis(coef, K, c["b0"], c["nb"], c["seed"], ids, imag=True)
  yr, yi = (np.moveaxis(a.reshape(K, c["nb"], c["nspec"], c["n"]), 0, -1)[:, ok] for a in (yr, yi))
  return r[ok], coef[:, :, ok], (Zr[:, ok], Zi[:, ok]), (yr, yi)


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_restatement_within_the_bound_of_an_extended_precision_dft(case):
  """||BLU(x) - DFT(x)||_2 <= 12 (2K - 1) (2 log2 M + 2) 2^-53 ||x||_2 (DESIGN.md section 26 derives
  it), the DFT a direct O(K^2) sum in np.longdouble: for the coefficients, x the residual (the
  error over the K / 2 + 1 stored ones); for the synthesis, x the rotated spectrum the restatement
  transforms, the bound and the result both divided by K, the imaginary part included.  Largest
  observed fraction of the bound over the table: 0.0068 (coefficients), 0.0084 (synthesis), both at
  K = 4; 0.0001 and 0.0002 at K = 1200."""
  c, K = case, case["K"]
  r, coef, (Zr, Zi), (yr, yi) = _parts(c)
  nf = K // 2 + 1
  Rr, Ri = FC.dft_long(r, np.zeros_like(r), -1)
  err = _norm2(coef[0].T - Rr[:, :nf], coef[1].T - Ri[:, :nf])
  frac = [_frac(err, FC.bound(K, _norm2(r)))]
  Yr, Yi = FC.dft_long(Zr, Zi, +1)
  err = _norm2(yr - Yr / K, yi - Yi / K)
  frac.append(_frac(err, FC.bound(K, _norm2(Zr, Zi)) / K))
  print("%s: largest fraction of the bound: coefficients %.5f, synthesis %.5f"
        % ((c["name"],) + tuple(frac)))
  assert max(frac) <= 1.0, (c["name"], frac)


# ------------------------------------------------------------------ 2. properties
@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_a_surrogate_keeps_the_periodogram_and_is_real(case):
  """Per finite series: |rfft(surrogate)_f| equals |DFT(residual)_f| to within twice the bound at
  every f (once for the coefficients, once for the synthesis: an error of y of 2-norm e moves a
  DFT value by at most sqrt(K) e); the imaginary part of BLU(Z, +1) / K, which the restatement
  keeps, is within the bound / K of zero; Z_0 and, for even K, Z_{K/2} are the coefficients' real
  parts, unrotated."""
  c, K = case, case["K"]
  r, coef, (Zr, Zi), (yr, yi) = _parts(c)
  lim = FC.bound(K, _norm2(r)).astype(np.float64)
  Rr, Ri = FC.dft_long(r, np.zeros_like(r), -1)
  amp = np.sqrt(Rr * Rr + Ri * Ri)[:, :K // 2 + 1].astype(np.float64)
  # (numpy's own transform adds its rounding, a few 2^-53 log2 K ||y||_2: inside the slack the
  # bound's constant keeps; scaled per series so that 1e+-150 neither overflows nor vanishes)
  scale = np.abs(yr).max(axis=-1, keepdims=True)
  scale = np.where(scale > 0, scale, 1.0)
  got = np.abs(np.fft.rfft(yr / scale, axis=-1)) * scale
  assert (np.abs(got - amp) <= 2.0 * lim[:, None]).all(), c["name"]
  limz = (FC.bound(K, _norm2(Zr, Zi)) / K).astype(np.float64)
  assert (np.abs(yi) <= limz[..., None]).all(), c["name"]
  assert np.array_equal(Zr[..., 0], np.broadcast_to(coef[0, 0], Zr[..., 0].shape))
  assert (Zi[..., 0] == 0).all() and not np.signbit(Zi[..., 0]).any()
  if K % 2 == 0:
    assert np.array_equal(Zr[..., K // 2], np.broadcast_to(coef[0, K // 2], Zr[..., 0].shape))
    assert (Zi[..., K // 2] == 0).all() and not np.signbit(Zi[..., K // 2]).any()


def test_phases_belong_to_the_surrogate_number_alone():
  """Two different b give different phases; the same b gives the same phases whatever the chunk,
  the batch or the shard; the index is the top 16 bits of word 0 of noise_cases.words."""
  K, nspec, seed = 17, 3, 12345
  ids = np.uint64(2**33 + 7) + np.arange(4, dtype=np.uint64)
  q = FC.phase_index(K, 5, 4, nspec, seed, ids)
  assert q.shape == (8, 4, nspec, 4) and q.min() >= 0 and q.max() < 65536
  assert not np.array_equal(q[:, 0], q[:, 1])
  assert np.array_equal(FC.phase_index(K, 6, 2, nspec, seed, ids), q[:, 1:3])
  assert np.array_equal(FC.phase_index(K, 5, 4, nspec, seed, ids[2:]), q[..., 2:])
  assert not np.array_equal(FC.phase_index(K, 5, 4, nspec, seed + 1, ids), q)
  for f, b, s, m in ((1, 5, 0, 0), (8, 8, 2, 3), (3, 6, 1, 2)):
    w0 = NC.words(seed, ids[m], b, (s << 12) | f)[0]
    assert int(w0) >> 16 == q[f - 1, b - 5, s, m]
  # the rotation has modulus one to rounding, for every one of the 65536 phases
  Er, Ei = FC.rotation(np.arange(65536), FC.tables(K))
  assert np.abs(Er * Er + Ei * Ei - 1.0).max() <= 8 * FC.U
  ang = np.unwrap(np.arctan2(Ei, Er))
  assert np.abs(ang - 2.0 * np.pi * np.arange(65536) / 65536.0).max() < 1e-12


def test_a_sinusoid_at_a_dft_frequency_keeps_its_line():
  """The "tone" series (frequency K // 4): the surrogate is a sinusoid of the same frequency and
  amplitude at another phase; the constant series has zero coefficients and zero surrogates."""
  c = next(k for k in CASES if k["K"] == 96 and k["n"] == 65 and k["detrend"] == "linear")
  coef = FC.coefficients(c["v"], c["k0"], c["k1"], "constant")
  y = FC.synthesis(coef, 96, 0, 2, 7, FC.ids_of(c)).reshape(96, 2, c["nspec"], 65)
  tone = [(s, m) for s in range(c["nspec"]) for m in range(65) if FC.style_of(s, m, 65) == "tone"]
  const = [(s, m) for s in range(c["nspec"]) for m in range(65) if FC.style_of(s, m, 65) == "const"]
  assert tone and const
  for s, m in tone:
    spec = np.abs(np.fft.rfft(y[:, 1, s, m]))
    assert abs(spec[24] - 96.0) < 1e-9 and np.delete(spec, 24).max() < 1e-9
  for s, m in const:
    assert (coef[:, :, s, m] == 0.0).all() and (y[:, :, s, m] == 0.0).all()


# ------------------------------------------------------------------ 3. calibration and power
N, K, W, S, NSUR = 400, 200, 50, 5, 199


def _ar(rng, phi, phi2=0.0, scale=1.0):
  """[K, 1, N]: AR(2) series x_k = phi_k x_{k-1} + phi2 x_{k-2} + e_k after a spin-up; phi a number
  or [K]; with phi2 = 0 the innovations keep the marginal variance at one."""
  phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))
  v = np.empty((K, 1, N))
  x1, x2 = rng.standard_normal(N), rng.standard_normal(N)
  for k in range(-100, K):
    p = phi[max(k, 0)]
    e = rng.standard_normal(N) * (np.sqrt(1.0 - p * p) if phi2 == 0.0 else scale)
    x1, x2 = p * x1 + phi2 * x2 + e, x1
    if k >= 0:
      v[k, 0] = x1
  return v


def _count(res, key, which="p_rising", level=0.1):
  p = res[key][which]
  assert np.isfinite(p).all()
  return int((p <= level).sum())


def test_the_fourier_test_is_calibrated():
  """400 stationary AR(1) series (phi = 0.5, K = 200) plus a constant and a linear trend, W = 50,
  S = 5, linear detrending, 199 Fourier surrogates: the number of series with p_rising <= 0.1 is
  Binomial(400, 0.1) under the null -- mean 40, sd 6; asserted within three sd, [22, 58], for var
  and for ac.  Observed with these seeds: var 39, ac 44."""
  rng = np.random.default_rng(20261)
  v = _ar(rng, 0.5) + 3.0 + 0.01 * np.arange(K)[:, None, None]
  res = FC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=77, nb=25)
  for key in ("var", "ac"):
    got = _count(res, key)
    print("%s: %d of %d series with p_rising <= 0.1" % (key, got, N))
    assert 22 <= got <= 58, (key, got)
    assert (res[key]["nvalid"] == NSUR).all()


def test_the_fourier_test_has_power():
  """400 series whose AR coefficient ramps linearly 0.1 -> 0.9 at unit marginal variance: at least
  200 have ac.p_rising <= 0.1 (observed with these seeds: 349; var: 8).  var is flat by construction and
  not asserted."""
  rng = np.random.default_rng(20262)
  v = _ar(rng, np.linspace(0.1, 0.9, K))
  res = FC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=78, nb=25)
  got = _count(res, "ac")
  print("ac: %d of %d series with p_rising <= 0.1; var: %d" % (got, N, _count(res, "var")))
  assert got >= 200, got


def test_the_two_nulls_side_by_side_on_a_peaked_spectrum():
  """Reported, not asserted beyond its format: 400 stationary AR(2) series with a spectral peak
  (phi1 = 1.2, phi2 = -0.72: a period of about eight records), the case the Fourier null exists
  for -- the count of p_rising <= 0.1 under either null, 40 expected of a calibrated test.  Observed
  with these seeds: var 42 under AR(1) and 30 under Fourier, ac 36 and 43."""
  rng = np.random.default_rng(20263)
  v = _ar(rng, 1.2, phi2=-0.72)
  four = FC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=79, nb=25)
  ar1 = SGC.significance(v, 0, K, W, S, 1, "linear", NSUR, seed=79, nb=25)
  for key in ("var", "ac"):
    a, f = _count(ar1, key), _count(four, key)
    print("AR(2) null series, %s: p_rising <= 0.1 in %d of %d under AR(1), %d under Fourier"
          % (key, a, N, f))
    assert 0 <= a <= N and 0 <= f <= N


# ------------------------------------------------------------------ 4. host logic
def test_tables_are_what_the_header_states():
  from pymoc_amd import fourier
  from pymoc_amd.spectra import twiddles
  for K, M in FC.M_OF.items():
    assert fourier.m_of(K) == FC.m_of(K) == M
  for K in range(4, 200):
    M = fourier.m_of(K)
    assert M >= 2 * K - 1 and M >= 8 and M & (M - 1) == 0 and (M == 8 or M // 2 < 2 * K - 1)
  assert fourier.m_of(4096) == 8192 and fourier.m_of(2048) == 4096 and fourier.m_of(2049) == 8192
  for K in (4, 5, 17, 96, 1200, 4096):
    q = fourier.chirp_index(K)
    assert np.array_equal(q, FC.chirp_index(K)) and q.min() >= 0 and q.max() < 2 * K
    assert q.dtype == np.int64 and q[-1] == ((K - 1) ** 2) % (2 * K)
    ch = fourier.chirp(K)
    assert ch.shape == (K, 2) and tuple(ch[0]) == (1.0, 0.0) and not np.signbit(ch).all(axis=0).any()
    assert not (np.signbit(ch) & (ch == 0)).any()  # no negative zero
    # (taken mod 2K the argument stays below 2 pi; j^2 itself would reach 1.7e7 at K = 4096); every
    # entry within 3 * 2^-53 of the exact value, which the error bound's derivation relies on
    pi = np.longdouble(2.0) * np.arccos(np.longdouble(0.0))
    ang = pi * q.astype(np.longdouble) / np.longdouble(K)
    assert np.abs(ch[:, 0] - np.cos(ang)).max() <= 3 * FC.U
    assert np.abs(ch[:, 1] + np.sin(ang)).max() <= 3 * FC.U
  for K in (4, 5, 96, 257):
    tab = fourier.Tables(K)
    assert np.array_equal(tab.tw, twiddles(tab.M))
    got = FC.filt_of(K, tab.tw, tab.chirp)
    assert np.array_equal(got.view(np.uint64), tab.filt.view(np.uint64))
    # b is even, so its transform is even: conjugating B^ is all the inverse needs
    br, bi = FC.extension(K, tab.chirp)
    ref = np.fft.fft(br + 1j * bi)
    assert np.abs((tab.filt[:, 0] + 1j * tab.filt[:, 1]) - ref).max() < 1e-11 * K
    assert np.isfinite(tab.filt).all() and tab.filt.shape == (tab.M, 2)
  hi, lo = fourier.phases()
  a = np.arange(256)
  assert hi.shape == lo.shape == (256, 2) and tuple(hi[0]) == tuple(lo[0]) == (1.0, 0.0)
  assert np.abs(hi[:, 0] + 1j * hi[:, 1] - np.exp(2j * np.pi * a / 256)).max() < 1e-15
  assert np.abs(lo[:, 0] + 1j * lo[:, 1] - np.exp(2j * np.pi * a / 65536)).max() < 1e-15
  # the complex transform restated here is spectra_cases.fft_dit when the input is real
  rng = np.random.default_rng(5)
  y = rng.standard_normal((3, 64))
  for got, want in zip(FC.fft_c(y, np.zeros_like(y), twiddles(64)), SC.fft_dit(y, twiddles(64))):
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
  for got, want in zip(fourier.fft_dit(y, y[::-1].copy(), twiddles(64)),
                       FC.fft_c(y, y[::-1].copy(), twiddles(64))):
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_table_holds_what_it_must():
  ks = {c["K"] for c in CASES}
  assert ks == set(FC.RECORDS) == set(FC.M_OF)
  for K in FC.RECORDS:
    assert {c["detrend"] for c in CASES if c["K"] == K} >= set(FC.DETRENDS)
  assert {c["n"] for c in CASES if c["K"] < FC.BIG} == {1, 3, 65}
  assert {c["nspec"] for c in CASES} == {1, 3} and {c["nb"] for c in CASES} == {1, 3}
  assert {c["b0"] for c in CASES} == set(FC.B0S) and {c["member0"] for c in CASES} == set(FC.MEMBER0S)
  assert all(c["n"] <= 3 and c["nspec"] == 1 for c in CASES if c["K"] >= FC.BIG)
  assert all(c["b0"] + c["nb"] <= 2**32 for c in CASES)
  wide = [c for c in CASES if c["n"] == 65 and c["nspec"] == 3]
  assert {FC.style_of(s, m, 65) for s in range(3) for m in range(65)} == set(FC.STYLES) and wide


def test_fourier_layouts_match_header(tmp_path):
  from pymoc_amd import _lib
  for cls, entry in ((_lib.pm_series_fourier_coef, "pm_series_fourier_coef"),
                     (_lib.pm_series_surrogates_fourier, "pm_series_surrogates_fourier")):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert _lib.SIGNATURES[entry][1][0] is C.POINTER(cls)
  text = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pymoc_hip.h")).read()
  assert "{ id_lo, id_hi, b, (s << 12) | f }" in text
  assert "one of\n * 65536 values" in text or "one of 65536 values" in text


def _with_tables(d, K, keys, nan_in=None):
  """The host tables of K (a copy with a NaN in `nan_in`) and stand-in device addresses into d."""
  tab = FC.tables(K)
  d._keep = []
  for key in keys:
    a = getattr(tab, key)
    if key == nan_in:
      a = a.copy()
      a[-1, 1] = np.nan
    d._keep.append(a)
    setattr(d, key, a.ctypes.data)
    setattr(d, key + "_dev", FAKE)


def coef_desc(nan_in=None, **kw):
  """A valid pm_series_fourier_coef descriptor of K = 60 (the device addresses are stand-ins) with
  the edits."""
  from pymoc_amd import _lib
  from pymoc_amd.windows import stt_of
  d = _lib.pm_series_fourier_coef()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = 10, 2, 70, 5, 65
  d.detrend, d.M, d.stt, d.v = _lib.PM_WIN_DETREND_LINEAR, 128, stt_of(60), FAKE
  _with_tables(d, 60, ("tw", "chirp", "filt"), nan_in)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_coef_descriptors():
  return ([("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
           ("k0 -1", dict(k0=-1)), ("k1 > nrec", dict(k1=71)), ("k0 == k1", dict(k0=65)),
           ("K 3", dict(k0=62)), ("K 4097", dict(nrec=5000, k0=0, k1=4097, M=8192)),
           ("M 256", dict(M=256)), ("M 64", dict(M=64)), ("M 0", dict(M=0)),
           ("detrend 3", dict(detrend=3)), ("detrend -1", dict(detrend=-1)),
           ("stt", dict(stt=17995.0 + 1.0)), ("stt nan", dict(stt=float("nan"))),
           ("nspec 65536", dict(nspec=65536, n=1)), ("nspec * n 2^31", dict(nspec=32768, n=65536))] +
          [(f, {f: None}) for f in ("v", "tw", "chirp", "filt", "tw_dev", "chirp_dev", "filt_dev")] +
          [("%s not finite" % f, dict(nan_in=f)) for f in ("tw", "chirp", "filt")])


def synthesis_desc(nan_in=None, **kw):
  """A valid pm_series_surrogates_fourier descriptor of K = 60 with the edits."""
  from pymoc_amd import _lib
  d = _lib.pm_series_surrogates_fourier()
  d.n, d.nspec, d.K, d.nb, d.b0, d.member0, d.seed, d.M, d.coef = 10, 2, 60, 3, 0, 0, 1, 128, FAKE
  _with_tables(d, 60, ("tw", "chirp", "filt", "ph_hi", "ph_lo"), nan_in)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_synthesis_descriptors():
  keys = ("tw", "chirp", "filt", "ph_hi", "ph_lo")
  return ([("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("nspec 0", dict(nspec=0)), ("nb 0", dict(nb=0)),
           ("K 3", dict(K=3, M=8)), ("K 0", dict(K=0)), ("K 4097", dict(K=4097, M=8192)),
           ("M 256", dict(M=256)), ("M 64", dict(M=64)),
           ("b0 -1", dict(b0=-1)), ("b0 + nb > 2^32", dict(b0=2**32 - 2)), ("b0 2^32", dict(b0=2**32)),
           ("member0 -1", dict(member0=-1)), ("nb * nspec 65536", dict(nb=32768)),
           ("nspec 65536", dict(nspec=65536, nb=1)),
           ("nb * nspec * n 2^31", dict(nb=1, nspec=32768, n=65536)), ("coef", dict(coef=None))] +
          [(f, {f: None}) for f in keys] + [(f + "_dev", {f + "_dev": None}) for f in keys] +
          [("%s not finite" % f, dict(nan_in=f)) for f in keys])


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  assert L.pm_series_fourier_coef(None, FAKE, None) == _lib.PM_EINVAL
  assert L.pm_series_surrogates_fourier(None, FAKE, None) == _lib.PM_EINVAL
  for label, kw in bad_coef_descriptors():
    d = coef_desc(**kw)
    assert L.pm_series_fourier_coef(C.byref(d), FAKE, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  for label, kw in bad_synthesis_descriptors():
    d = synthesis_desc(**kw)
    assert L.pm_series_surrogates_fourier(C.byref(d), FAKE, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = coef_desc()
  assert L.pm_series_fourier_coef(C.byref(d), None, None) == _lib.PM_EINVAL
  assert "coef is NULL" in L.pm_last_error().decode()
  d = coef_desc(M=256)
  assert L.pm_series_fourier_coef(C.byref(d), FAKE, None) == _lib.PM_EINVAL
  assert "M 256 is not 128" in L.pm_last_error().decode()
  d = coef_desc(nan_in="filt")
  assert L.pm_series_fourier_coef(C.byref(d), FAKE, None) == _lib.PM_EINVAL
  assert "filt[255] = nan is not finite" in L.pm_last_error().decode()
  d = synthesis_desc()
  assert L.pm_series_surrogates_fourier(C.byref(d), None, None) == _lib.PM_EINVAL
  assert "y is NULL" in L.pm_last_error().decode()
  d = synthesis_desc(nan_in="ph_lo")
  assert L.pm_series_surrogates_fourier(C.byref(d), FAKE, None) == _lib.PM_EINVAL
  assert "ph_lo[511] = nan is not finite" in L.pm_last_error().decode()


def test_kernels_cross_compile_without_scratch(tmp_path):
  """k_series_fourier_coef, both k_series_surrogates_fourier and k_series_fourier_transpose for
  gfx950: 0 bytes of scratch; no static LDS (all of it is dynamic) but the transpose's tile of
  32 x 33 doubles; DESIGN.md section 26 tabulates the registers."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "fourier.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "fourier.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_(?:fourier_coef|surrogates_fourier|fourier_transpose)\S*)",
                     p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stdout)]
  assert len(set(names)) == 4 and len(scratch) >= 4 and len(lds) >= 4
  assert all(x == 0 for x in scratch), list(zip(names, scratch))
  assert sorted(lds)[:-1] == [0] * (len(lds) - 1) and max(lds) == 8 * 32 * 33, list(zip(names, lds))


def test_classes_validate_method_before_any_device_array():
  """Every refusal is a ValueError raised on the host; the chunk arithmetic is what it was."""
  from pymoc_amd import SeriesSurrogates, SeriesWindows
  from pymoc_amd.surrogates import METHODS, check_method, chunk_size
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  assert METHODS == ("ar1", "fourier")
  assert SeriesSurrogates(src).method == "ar1"
  gen = SeriesSurrogates(src, method="fourier", seed=3)
  assert gen.method == "fourier"
  for bad in ("iaaft", "AR1", None, 1, ""):
    with pytest.raises(ValueError, match="unknown method"):
      SeriesSurrogates(src, method=bad)
    with pytest.raises(ValueError, match="unknown method"):
      SeriesWindows(src, 32, step=4).significance(method=bad)
  with pytest.raises(ValueError, match="has no fit"):
    gen.fit()
  with pytest.raises(ValueError, match="has no coefficients"):
    SeriesSurrogates(src).coefficients()
  for k0, k1 in ((-1, 40), (40, 40), (0, 101)):
    for call in (gen.coefficients, gen.generate):
      with pytest.raises(ValueError, match="window"):
        call(k0, k1)
  with pytest.raises(ValueError, match=r"window \[10, 13\) holds 3 records"):
    gen.coefficients(10, 13)
  with pytest.raises(ValueError, match=r"nb \* nspec = 65536 is above 65535"):
    gen.generate(0, 50, 0, 32768)
  tab = gen.tables(60)
  assert gen.tables(60) is tab and (tab.K, tab.M) == (60, 128) and gen.tables(61) is not tab
  # fourier + until: refused with the reason, before `until` is looked at
  sw = SeriesWindows(src, 32, step=4)
  with pytest.raises(ValueError, match="does not take until=.*transform length would be each member's own"):
    sw.significance(method="fourier", until=object())
  check_method("fourier")
  check_method("ar1", until=object())
  for kw in (dict(nsur=0), dict(seed=-1), dict(member0=-1), dict(max_bytes=None)):
    with pytest.raises(ValueError, match="|".join(kw)):
      sw.significance(method="fourier", **kw)
  with pytest.raises(ValueError, match="max_bytes = 9599 does not hold one surrogate of 9600 bytes"):
    sw.significance(method="fourier", max_bytes=9599)
  # a block holds one series from M = 2048 on, K >= 513: there the synthesis is given a scratch
  from pymoc_amd import fourier
  assert [K for K in range(4, 4097) if fourier.wants_scratch(K)] == list(range(513, 4097))
  assert SeriesWindows(src, 32, step=4)._fourier_tables == {}
  assert chunk_size(1000, 2 << 30, 1200, 8, 4096) == 6
  assert chunk_size(1000, 2 << 30, 1200, 8, 4096, per=16) == 3
  assert chunk_size(100000, 1 << 50, 10, 8, 4) == 65535 // 8
  assert chunk_size(5, 8 * 10 * 8 * 4, 10, 8, 4) == 1
