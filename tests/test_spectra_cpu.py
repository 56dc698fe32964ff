"""SeriesSpectra and pm_series_spectra without a device: the case table; the restatement
(tests/spectra_cases.py) against an extended-precision direct DFT and against scipy.signal.welch /
csd; the twiddle table and the Hann window; the header mirror; every argument check of the entry
and of SeriesSpectra."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import spectra_cases as SC
from test_steady_cpu import _layout

U = 2.0**-53
LD = np.longdouble
CASES = SC.cases()
IDS = [c["name"] for c in CASES]
MEMBERS = 8  # the members of a case the authorities are run on: one of every style per index


def test_table_holds_what_it_must():
  assert {c["L"] for c in CASES} >= {8, 64, 128, 1024}
  for L in (8, 64, 128, 1024):
    assert {c["noverlap"] for c in CASES if c["L"] == L} == {0, L // 2, L - 1}, L
  assert {c["nseg"] for c in CASES} == {1, 2, 5}
  assert {c["v"].shape[2] for c in CASES} >= {1, 7, 64, 65}
  assert {c["v"].shape[1] for c in CASES} == {1, 3}
  assert {c["detrend"] for c in CASES} == {"constant", "none"}
  assert {c["window"] for c in CASES} == {"hann", "boxcar", "random"}
  for c in CASES:
    K = c["k1"] - c["k0"]
    assert c["k0"] > 0 and c["k1"] < c["v"].shape[0]
    assert SC.nseg_of(K, c["L"], c["noverlap"]) == c["nseg"]
    S = c["L"] - c["noverlap"]
    assert K - (c["L"] + (c["nseg"] - 1) * S) == min(S - 1, 3)  # the tail that fits no segment
    assert c["v"].shape[1] * c["v"].shape[2] <= 65 * 3
    assert (c["w"] > 0).all() or c["window"] == "hann"
    if c["v"].shape[1] == 3:
      assert tuple(c["pairs"]) == ((0, 2), (2, 0), (1, 1))
    # the styles: one NaN / inf inside exactly one segment, members with every segment spoiled
    y, used = SC.segments(c["v"], c["k0"], c["k1"], c["L"], c["noverlap"], c["w"], c["detrend"])
    for s in range(c["v"].shape[1]):
      for m in range(c["v"].shape[2]):
        st, x = SC.style_of(s, m), c["v"][c["k0"]:c["k1"], s, m]
        if st in SC.FINITE_STYLES:
          assert used[:, s, m].all() and np.isfinite(x).all()
        elif st == "nan1":
          assert np.isnan(x).sum() == 1 and used[:, s, m].tolist() == [False] + [True] * (c["nseg"] - 1)
        elif st == "inf1":
          assert np.isinf(x).sum() == 1 and used[:, s, m].tolist() == [True] * (c["nseg"] - 1) + [False]
        else:
          assert not used[:, s, m].any()
        if st == "big":
          assert 1e149 < np.abs(x).max() < 1e152
        if st == "small":
          assert 1e-151 < np.abs(x).max() < 1e-149
  assert any(c["nseg"] > 1 and c["v"].shape[2] >= 8 for c in CASES)


def test_twiddles_and_hann():
  import scipy.signal
  from pymoc_amd.spectra import hann, twiddles
  for L in (8, 16, 32, 64, 128, 256, 512, 1024):
    tw = twiddles(L)
    assert tw.shape == (L // 2, 2) and tw.dtype == np.float64 and tw.flags.c_contiguous
    assert tw[0].tolist() == [1.0, 0.0] and tw[L // 4].tolist() == [0.0, -1.0]
    j = np.arange(L // 2)
    pi = 4 * np.arctan(LD(1))
    want = np.stack([np.cos(2 * pi * j / L), -np.sin(2 * pi * j / L)], axis=1)
    # the folded angle is at most pi / 4 with a relative error of 2 u (pi's own, one product):
    # 1.6 u; sin / cos add an ulp of a value below 1: 2 u
    assert np.abs(tw - want).max() <= 4 * U
    w = hann(L)
    assert w.shape == (L,) and w[0] == 0.0
    assert np.abs(w - scipy.signal.get_window("hann", L)).max() <= U


def test_restatement_on_a_transform_worked_by_hand():
  """L = 8, boxcar, no detrending: an impulse gives a flat spectrum, a constant only bin 0."""
  from pymoc_amd.spectra import twiddles
  tw = twiddles(8)
  x = np.zeros(8)
  x[0] = 3.0
  re, im = SC.fft_dit(x, tw)
  assert re.tolist() == [3.0] * 8 and not im.any()
  re, im = SC.fft_dit(np.full(8, 2.0), tw)
  assert re.tolist() == [16.0] + [0.0] * 7 and not im.any()
  x = np.arange(8.0)
  re, im = SC.fft_dit(x, tw)
  want = np.fft.fft(x)
  assert np.abs(re - want.real).max() < 1e-14 and np.abs(im - want.imag).max() < 1e-14
  v = np.arange(8.0).reshape(8, 1, 1)
  r = SC.spectra(v, 0, 8, 8, 0, np.ones(8), "none", ((0, 0),), 0.125, tw)
  c = np.array([1, 2, 2, 2, 1.0])
  p = (re[:5] * re[:5] + im[:5] * im[:5]) / 1.0 * 0.125 * c
  assert np.array_equal(r["psd"][:, 0, 0], p) and r["nused"][0, 0] == 1
  assert np.array_equal(r["csd"][:, 0, 0], p) and not r["csd"][:, 1, 0].any()


# ------------------------------------------------------------------ the two authorities
@functools.lru_cache(maxsize=None)
def _ld_tables(L):
  """cos and sin [L, nf] of 2 pi (f j mod L) / L as longdouble: the phase index is reduced in
  integers before it is scaled."""
  pi = 4 * np.arctan(LD(1))
  ang = 2 * pi * np.arange(L).astype(LD) / LD(L)
  idx = (np.arange(L)[:, None] * np.arange(L // 2 + 1)[None, :]) % L
  return np.cos(ang)[idx], np.sin(ang)[idx]


def _ld_dft(y):
  """Z [nseg, nf] (re, im as longdouble) of the segments y [nseg, L] by the direct sum."""
  cos, sin = _ld_tables(y.shape[-1])
  yl = y.astype(LD)
  return yl @ cos, -(yl @ sin)


def _one_sided(L):
  c = np.full(L // 2 + 1, LD(2))
  c[0] = c[-1] = 1
  return c


def _run(used):
  """(i0, i1): the used segments, which are one run in every style of the table."""
  i = np.nonzero(used)[0]
  assert i.size and i[-1] - i[0] + 1 == i.size
  return int(i[0]), int(i[-1])


@functools.lru_cache(maxsize=None)
def _errors(ci, whole):
  """Per case: (err_ours, err_scipy, the largest of each as a multiple of 2^-53 * max psd), every
  error divided by its own series' max psd (the styles differ by 300 orders of magnitude), a cross
  spectrum's by sqrt(max psd_a * max psd_b).
  The authority is the longdouble DFT of the restatement's own detrended, windowed segments.
  whole = False: SciPy gets those same segments one by one (detrend=False; the restatement's mean
  already removed), their periodograms summed in ascending order -- SciPy's transform and scaling
  against ours.  whole = True: scipy.signal.welch / csd on the records of the used segments with
  detrend="constant" or False, as a user calls them (SciPy's own mean enters its error)."""
  import scipy.signal
  c = CASES[ci]
  L, S, fs = c["L"], c["L"] - c["noverlap"], 1.0 / c["dt"]
  y, used, mu = SC.segments(c["v"], c["k0"], c["k1"], L, c["noverlap"], c["w"], c["detrend"], True)
  r = SC.restate(c)
  nspec, n = c["v"].shape[1:]
  members = range(min(n, MEMBERS))
  one = _one_sided(L)
  sp_det = "constant" if c["detrend"] == "constant" else False
  kw = dict(fs=fs, window=c["w"], nperseg=L, scaling="density", return_onesided=True)
  Z, runs, tops = {}, {}, {}
  err_ours = err_scipy = 0.0

  def scipy_of(a, b, i0, i1):
    xa, xb = (c["v"][c["k0"] + i0 * S:c["k0"] + i1 * S + L, s, m] for s, m in (a, b))
    if whole:
      return scipy.signal.csd(xa, xb, noverlap=c["noverlap"], detrend=sp_det, **kw)[1]
    acc = 0.0
    for i in range(i0, i1 + 1):  # the detrended segment before the window
      sa, sb = ((c["v"][c["k0"] + i * S:c["k0"] + i * S + L, s, m] - mu[i, s, m]) for s, m in (a, b))
      acc = acc + scipy.signal.csd(sa, sb, noverlap=0, detrend=False, **kw)[1]
    return acc / (i1 - i0 + 1)

  for s in range(nspec):
    for m in members:
      if not used[:, s, m].any():
        assert np.isnan(r["psd"][:, s, m]).all() and r["nused"][s, m] == 0
        continue
      i0, i1 = runs[s, m] = _run(used[:, s, m])
      Z[s, m] = _ld_dft(y[i0:i1 + 1, s, m])
  with np.errstate(all="ignore"):
    for (s, m), (zr, zi) in Z.items():
      i0, i1 = runs[s, m]
      ref = (zr * zr + zi * zi).mean(axis=0) * LD(c["scale"]) * one
      top = tops[s, m] = float(ref.max())
      assert r["nused"][s, m] == i1 - i0 + 1
      if top == 0.0:
        assert not r["psd"][:, s, m].any()
        continue
      err_ours = max(err_ours, float(np.abs(r["psd"][:, s, m] - ref).max()) / top)
      if SC.style_of(s, m) != "const":  # (about a constant SciPy's own mean is all there is)
        sp = scipy_of((s, m), (s, m), i0, i1).real
        err_scipy = max(err_scipy, float(np.abs(sp - ref).max()) / top)
    for p, (a, b) in enumerate(c["pairs"]):
      for m in members:
        both = used[:, a, m] & used[:, b, m]
        if not both.any():
          assert np.isnan(r["csd"][:, 2 * p:2 * p + 2, m]).all() and r["nused_pair"][p, m] == 0
          continue
        i0, i1 = _run(both)
        (ar, ai), (br, bi) = (tuple(z[i0 - runs[s, m][0]:i1 - runs[s, m][0] + 1] for z in Z[s, m])
                              for s in (a, b))
        cr = (ar * br + ai * bi).mean(axis=0) * LD(c["scale"]) * one
        cim = (ar * bi - ai * br).mean(axis=0) * LD(c["scale"]) * one
        # a bin's error follows |Za| |Zb|, not the cross spectrum left after cancellation
        top = float(np.sqrt(LD(tops[a, m]) * LD(tops[b, m])))
        assert r["nused_pair"][p, m] == i1 - i0 + 1
        if top == 0.0:
          continue
        d = np.hypot(r["csd"][:, 2 * p, m] - cr, r["csd"][:, 2 * p + 1, m] - cim)
        err_ours = max(err_ours, float(d.max()) / top)
        if "const" not in (SC.style_of(a, m), SC.style_of(b, m)):
          sp = scipy_of((a, m), (b, m), i0, i1)
          d = np.hypot(sp.real - cr, sp.imag - cim)
          err_scipy = max(err_scipy, float(d.max()) / top)
  return err_ours, err_scipy


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_restatement_against_the_longdouble_dft(ci):
  """err_ours <= 8 * max(err_scipy, 2^-53 * max psd) per case, errors relative to each series' own
  max psd; SciPy is given the restatement's own segments.  Largest err_ours / 2^-53 observed over
  the table: 3.23 (L = 1024, half overlap, Hann); SciPy's: 3.79."""
  err_ours, err_scipy = _errors(ci, False)
  print("%s: err_ours %.2f u, err_scipy %.2f u (u = 2^-53 max psd)"
        % (CASES[ci]["name"], err_ours / U, err_scipy / U))
  assert err_ours <= 8 * max(err_scipy, U), (err_ours / U, err_scipy / U)


@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if c["L"] <= 256],
                         ids=[c["name"] for c in CASES if c["L"] <= 256])
def test_restatement_against_scipy_welch_and_csd(ci):
  """scipy.signal.welch / csd as a user calls them (detrend="constant" or False,
  scaling="density"): the same bound, SciPy's error now holding its own mean."""
  err_ours, err_scipy = _errors(ci, True)
  print("%s: err_ours %.2f u, err_scipy %.2f u" % (CASES[ci]["name"], err_ours / U, err_scipy / U))
  assert err_ours <= 8 * max(err_scipy, U), (err_ours / U, err_scipy / U)


# ------------------------------------------------------------------ the C-ABI
def test_spectra_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  cls = _lib.pm_series_spectra
  vals = _layout(tmp_path, cls.__name__, cls._fields_)
  assert vals[0] == C.sizeof(cls)
  assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_series_spectra"][1][0] is C.POINTER(cls)
  assert (_lib.PM_SPEC_NPERSEG_MIN, _lib.PM_SPEC_NPERSEG_MAX, _lib.PM_SPEC_PAIRS_MAX) == (
      SC.NPERSEG_MIN, SC.NPERSEG_MAX, SC.PAIRS_MAX)
  assert (_lib.PM_SPEC_DETREND_NONE, _lib.PM_SPEC_DETREND_CONSTANT) == (0, 1)


def test_kernel_cross_compiles_without_scratch(tmp_path):
  """Every instantiation of k_series_spectra for gfx950 (L = 8 .. 1024): 0 bytes of scratch
  (DESIGN.md section 20 tabulates the registers)."""
  from conftest import ROOT
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  src = os.path.join(ROOT, "pymoc_amd", "csrc", "spectra.hip")
  p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC",
                      "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                      "-c", "-o", str(tmp_path / "spectra.o"), src],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
  assert p.returncode == 0, p.stdout[-2000:]
  names = re.findall(r"Function Name: (\S*k_series_spectra\S*)", p.stdout)
  scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stdout)]
  assert len(set(names)) == 8 and len(scratch) >= 8
  assert all(x == 0 for x in scratch), list(zip(names, scratch))


FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first


def desc(keep, **kw):
  """A valid descriptor (device addresses are stand-ins) with the edits `kw`; `keep` holds the host
  mirrors alive; window_values= and pair_values= fill the mirrors, every other keyword sets a
  field."""
  from pymoc_amd import _lib
  d = _lib.pm_series_spectra()
  w = np.asarray(kw.pop("window_values", np.ones(16)), dtype=np.float64)
  pair = np.asarray(kw.pop("pair_values", [[0, 1], [1, 1]]), dtype=np.int32).reshape(-1, 2)
  keep += [w, pair]
  d.n, d.nspec, d.nrec, d.k0, d.k1 = 10, 2, 60, 1, 50
  d.nperseg, d.step, d.detrend, d.npairs = 16, 8, 1, pair.shape[0]
  d.v, d.window_dev, d.twiddle, d.pair_dev = FAKE, FAKE + 4096, FAKE + 8192, FAKE + 12288
  d.window, d.pair, d.scale = w.ctypes.data, pair.ctypes.data, 0.25
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_descriptors():
  w = np.ones(16)
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=50)),
          ("k0 > k1", dict(k0=40, k1=20)), ("k1 > nrec", dict(k1=61)),
          ("L 12", dict(nperseg=12)), ("L 4", dict(nperseg=4)), ("L 0", dict(nperseg=0)),
          ("L -16", dict(nperseg=-16)), ("L 2048", dict(nperseg=2048, nrec=4000, k1=3000)),
          ("K < L", dict(k0=40)), ("K = L - 1", dict(k0=35)),
          ("step 0", dict(step=0)), ("step -1", dict(step=-1)), ("step L + 1", dict(step=17)),
          ("detrend 2", dict(detrend=2)), ("detrend -1", dict(detrend=-1)),
          ("npairs 9", dict(npairs=9)), ("npairs -1", dict(npairs=-1)),
          ("pair = nspec", dict(pair_values=[[0, 2]])), ("pair -1", dict(pair_values=[[0, 1], [-1, 0]])),
          ("v", dict(v=None)), ("window", dict(window=None)), ("window_dev", dict(window_dev=None)),
          ("twiddle", dict(twiddle=None)), ("pair", dict(pair=None)),
          ("pair_dev", dict(pair_dev=None)),
          ("window nan", dict(window_values=np.where(np.arange(16) == 5, np.nan, w))),
          ("window inf", dict(window_values=np.where(np.arange(16) == 15, np.inf, w))),
          ("scale nan", dict(scale=float("nan"))), ("scale inf", dict(scale=float("inf"))),
          ("nf * nspec", dict(nspec=(1 << 30) // 9 + 1)),
          ("jobs", dict(nspec=65534))]


def test_entry_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  keep = []
  out = (FAKE + 64, FAKE + 128, FAKE + 192, FAKE + 256)
  assert L.pm_series_spectra(None, *out, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    d = desc(keep, **kw)
    assert L.pm_series_spectra(C.byref(d), *out, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = desc(keep)
  for i in range(4):
    args = list(out)
    args[i] = None
    assert L.pm_series_spectra(C.byref(d), *args, None) == _lib.PM_EINVAL, i
  # pair, nused_pair and csd may be NULL with no pair -- then it is the next check that refuses
  d = desc(keep, pair_values=[], scale=float("inf"))
  d.pair = d.pair_dev = None
  assert L.pm_series_spectra(C.byref(d), out[0], out[1], None, None, None) == _lib.PM_EINVAL
  assert "scale" in L.pm_last_error().decode()


# ------------------------------------------------------------------ SeriesSpectra
class _Series(object):
  """A stand-in for a device series: a shape and a dtype, no memory."""

  def __init__(self, shape, dtype=np.float64):
    self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), 0


class _Recorder(object):
  """A stand-in for an IndexRecorder: what SeriesSpectra reads off one."""

  class _T(object):
    names = ["wind", "amoc"]

  class _E(object):
    stream = timer = None

  def __init__(self, written):
    self._values, self.table, self.ens = _Series((len(written), 2, 6)), self._T(), self._E()
    self.steps = np.where(written, np.arange(len(written)) * 12, -1)


def test_series_spectra_validates_its_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call, which
  on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesSpectra
  from pymoc_amd.spectra import hann
  src = (_Series((100, 2, 6)), ["wind", "amoc"])
  ok = SeriesSpectra(src, 32, pairs=[("wind", "amoc"), ("amoc", "amoc")], dt_record=0.5,
                     groups=[5, 5, 9, 9, 5, 1])
  assert (ok.nperseg, ok.noverlap, ok.step, ok.nf) == (32, 16, 16, 17)
  assert np.array_equal(ok.window, hann(32)) and ok.detrend == "constant"
  assert ok.scale == 1.0 / (2.0 * (hann(32) * hann(32)).sum())
  assert np.array_equal(ok.freq, np.arange(17) / (32 * 0.5))
  assert ok._pair.tolist() == [[0, 1], [1, 1]] and ok.nseg() == 5 and ok.nseg(3, 50) == 1
  assert SeriesSpectra(src, 8, noverlap=7, window="boxcar", detrend="none").step == 1
  assert SeriesSpectra(src, 8, noverlap=0, window=np.arange(8.0)).step == 8
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"]),
              (_Series((10, 0, 6)), []), (_Series((10, 2, 6)),)):
    with pytest.raises(ValueError, match="series|source"):
      SeriesSpectra(bad, 8)
  for names in (["amoc"], ["amoc", "amoc"], ["a", "b", "c"]):
    with pytest.raises(ValueError, match="names"):
      SeriesSpectra((_Series((10, 2, 6)), names), 8)
  for L in (4, 12, 0, -8, 2048, 8.0, "8", True):
    with pytest.raises(ValueError, match="nperseg"):
      SeriesSpectra(src, L)
  for nov in (-1, 32, 40, 1.5):
    with pytest.raises(ValueError, match="noverlap"):
      SeriesSpectra(src, 32, noverlap=nov)
  for w in ("hamming", np.ones(31), np.ones((32, 1)), np.where(np.arange(32) == 3, np.nan, 1.0),
            np.where(np.arange(32) == 3, np.inf, 1.0)):
    with pytest.raises(ValueError, match="window"):
      SeriesSpectra(src, 32, window=w)
  with pytest.raises(ValueError, match=r"window\[3\] = nan here"):
    SeriesSpectra(src, 32, window=np.where(np.arange(32) == 3, np.nan, 1.0))
  with pytest.raises(ValueError, match="scale"):
    SeriesSpectra(src, 32, window=np.zeros(32))
  for det in ("linear", None, True, 1):
    with pytest.raises(ValueError, match="detrend"):
      SeriesSpectra(src, 32, detrend=det)
  for dt in (0.0, -1.0, np.nan, np.inf, "year"):
    with pytest.raises(ValueError, match="dt_record"):
      SeriesSpectra(src, 32, dt_record=dt)
  with pytest.raises(ValueError, match="at most 8 pairs"):
    SeriesSpectra(src, 32, pairs=[("wind", "amoc")] * 9)
  for pr, word in ((("wind", "psi"), "unknown index 'psi'"), (("wind",), "give a tuple"),
                   ("wind", "give a tuple"), (("wind", "amoc", "amoc"), "give a tuple")):
    with pytest.raises(ValueError, match=word):
      SeriesSpectra(src, 32, pairs=[pr])
  for groups in (np.zeros(5, int), np.zeros(6), 3):
    with pytest.raises(ValueError, match="groups"):
      SeriesSpectra(src, 32, groups=groups)
  nspec = (1 << 30) // 513 + 1  # (integers serve as names)
  with pytest.raises(ValueError, match="nf \\* nspec = %d is not below 2\\^30" % (513 * nspec)):
    SeriesSpectra((_Series((2000, nspec, 1)), range(nspec)), 1024)
  with pytest.raises(ValueError, match="= 65536 is above 65535"):
    SeriesSpectra((_Series((100, 65535, 1)), range(65535)), 8, pairs=[(0, 1)])
  for k0, k1 in ((-1, 40), (40, 40), (50, 20), (0, 101), (100, None)):
    with pytest.raises(ValueError, match="window"):
      ok.compute(k0, k1)
    with pytest.raises(ValueError, match="window"):
      ok.across_members(k0, k1)
  with pytest.raises(ValueError, match=r"window \[70, 100\) holds 30 records, fewer than nperseg = 32"):
    ok.compute(70)
  with pytest.raises(ValueError, match="fewer than nperseg"):
    ok.across_members(0, 31)
  # a recorder: the records never written
  rec = _Recorder(np.arange(40) < 36)
  sp = SeriesSpectra(rec, 16, pairs=[("wind", "amoc")])
  assert sp.names == ["wind", "amoc"] and (sp.nrec, sp.nspec, sp.n) == (40, 2, 6)
  for call in (sp.compute, sp.across_members):
    with pytest.raises(ValueError, match=r"window \[0, 40\) holds record 36, which was never written"):
      call()
    with pytest.raises(ValueError, match="record 36"):
      call(10, 37)
