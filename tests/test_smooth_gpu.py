"""pm_series_smooth, SeriesSmooth and the "gaussian" detrend of SeriesWindows and SeriesSurrogates on
the device: every double bit for bit against the restatement (tests/smooth_cases.py), what a
launch leaves alone, independence of a member from the batch and of a record window from the
records around it, the whole "gaussian" pipeline exactly against the restated composition, the
launches each method issues, and a recorder source."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, PAD, SPARE, V_SENTINEL, _bits, _padded, _up
import smooth_cases as SC
import surrogate_cases as SGC
import windows_cases as WC

pytestmark = pytest.mark.gpu


def _guarded(gpu, size, dtype, fill):
  """A device output of `size` elements inside an allocation filled with `fill`, PAD elements
  before it and SPARE behind: (allocation, address of element 0)."""
  dev = _up(gpu, np.full(PAD + size + SPARE, fill, dtype=dtype))
  return dev, dev.ptr + np.dtype(dtype).itemsize * PAD


def _taken(dev, size, shape, fill, what):
  """The output out of its allocation; nothing before or behind it is touched."""
  flat = dev.download().ravel()
  assert (flat[:PAD] == fill).all(), (what, "before the output")
  assert (flat[PAD + size:] == fill).all(), (what, "behind the output")
  return flat[PAD:PAD + size].reshape(shape)


def run(gpu, c, trend=True, resid=True, v=None, k0=None, k1=None):
  """One launch of the case (or of another series or record window under its table): dict(trend,
  resid [K, nspec, n], nbad [nspec, n]); an output that is not asked for is passed as NULL and its
  arena comes back untouched."""
  from pymoc_amd import _lib
  v = c["v"] if v is None else v
  k0, k1 = c["k0"] if k0 is None else k0, c["k1"] if k1 is None else k1
  nrec, nspec, n = v.shape
  K = k1 - k0
  series, v_ptr = _padded(gpu, v)
  w = np.ascontiguousarray(c["w"])
  w_dev, w_ptr = _padded(gpu, w)
  size = K * nspec * n
  tr, tr_ptr = _guarded(gpu, size, np.float64, V_SENTINEL)
  re, re_ptr = _guarded(gpu, size, np.float64, V_SENTINEL)
  nb, nb_ptr = _guarded(gpu, nspec * n, np.int32, I_SENTINEL)
  d = _lib.pm_series_smooth()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.half = n, nspec, nrec, k0, k1, c["H"]
  d.v, d.w, d.w_dev = v_ptr, w.ctypes.data, w_ptr
  _lib.check(_lib.lib.pm_series_smooth(C.byref(d), tr_ptr if trend else None,
                                       re_ptr if resid else None, nb_ptr, None))
  gpu.synchronize()
  got = dict(nbad=_taken(nb, nspec * n, (nspec, n), I_SENTINEL, c["name"]))
  for key, on, dev in (("trend", trend, tr), ("resid", resid, re)):
    if on:
      got[key] = _taken(dev, size, (K, nspec, n), V_SENTINEL, (c["name"], key))
    else:
      assert (dev.download() == V_SENTINEL).all(), (c["name"], key, "not asked for")
  return got


CASES = SC.cases()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bits_and_optional_outputs(gpu, case):
  c, want = case, SC.restate(case)
  got = run(gpu, c)
  for key in ("trend", "resid"):
    _bits(got[key], want[key], (c["name"], key))
  assert got["nbad"].dtype == np.int32 and np.array_equal(got["nbad"], want["nbad"]), c["name"]
  only = run(gpu, c, resid=False)
  _bits(only["trend"], want["trend"], (c["name"], "trend only"))
  assert np.array_equal(only["nbad"], want["nbad"])
  only = run(gpu, c, trend=False)
  _bits(only["resid"], want["resid"], (c["name"], "resid only"))
  assert np.array_equal(only["nbad"], want["nbad"])


ALL_FINITE = [(3, 1, 1.0), (3, 2, 1.0), (3, 3, 0.3), (40, 37, 2.0), (5, 129, 20.0), (5, 300, 20.0),
              (5, 257, 75.0), (2, 700, 75.0)]


@pytest.mark.parametrize("n,K,sigma", ALL_FINITE, ids=["n %d K %d sigma %g" % p for p in ALL_FINITE])
def test_all_finite_blocks_walk_two_records_at_once_to_the_same_bits(gpu, n, K, sigma):
  """A block that staged no non-finite value forms its records in pairs: K = 1 (no pair), even and
  odd K, reaches cut at either end, at both or at neither, chunks of odd and even length, H above
  K - 1."""
  rng = np.random.default_rng(300 + K)
  v = np.full((3 + K + 2, 2, n), np.nan)
  v[3:3 + K] = 15.0 + rng.standard_normal((K, 2, n)) * np.array([1.0, 1e150])[None, :, None]
  v[3:3 + K, 0] += 0.01 * np.arange(K)[:, None] ** 2
  c = dict(name="all finite n %d K %d" % (n, K), v=v, k0=3, k1=3 + K, H=SC.half_of(sigma),
           w=SC.weights(sigma))
  got, want = run(gpu, c), SC.restate(c)
  for key in ("trend", "resid"):
    _bits(got[key], want[key], (c["name"], key))
  assert not got["nbad"].any() and np.isfinite(got["resid"]).all()


def test_a_member_does_not_depend_on_the_batch_nor_a_window_on_its_surroundings(gpu):
  for c in (CASES[0], CASES[2]):  # H 8 in one chunk; H 80, K 200 in two chunks, two tiles
    whole = run(gpu, c)
    n = c["n"]
    lo, hi = n // 3, n // 3 + max(2, n // 2)
    shard = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, lo:hi]))
    one = run(gpu, c, v=np.ascontiguousarray(c["v"][:, -1:, n - 1:]))
    for key in ("trend", "resid"):
      _bits(shard[key], whole[key][:, :, lo:hi], (c["name"], key, "shard"))
      _bits(one[key], whole[key][:, -1:, n - 1:], (c["name"], key, "one member"))
    assert np.array_equal(shard["nbad"], whole["nbad"][:, lo:hi])
    assert np.array_equal(one["nbad"], whole["nbad"][-1:, n - 1:])
    # a sub-window equals the copied-out sub-series
    k0, k1 = c["k0"] + 5, c["k1"] - 9
    sub = run(gpu, c, k0=k0, k1=k1)
    copied = run(gpu, c, v=np.ascontiguousarray(c["v"][k0:k1]), k0=0, k1=k1 - k0)
    want = SC.restate(c, k0=k0, k1=k1)
    for key in ("trend", "resid"):
      _bits(sub[key], copied[key], (c["name"], key, "sub-window"))
      _bits(sub[key], want[key], (c["name"], key, "sub-window, restated"))
    assert np.array_equal(sub["nbad"], copied["nbad"]) and np.array_equal(sub["nbad"], want["nbad"])


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_smooth_cpu as TC
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(2)]
  nbad = _up(gpu, np.full(4096, I_SENTINEL, dtype=np.int32))
  for label, kw in TC.bad_descriptors():
    d = TC.desc(**kw)
    rc = _lib.lib.pm_series_smooth(C.byref(d), out[0].ptr, out[1].ptr, nbad.ptr, None)
    assert rc == _lib.PM_EINVAL, label
  d = TC.desc()
  assert _lib.lib.pm_series_smooth(C.byref(d), None, None, nbad.ptr, None) == _lib.PM_EINVAL
  assert _lib.lib.pm_series_smooth(C.byref(d), out[0].ptr, out[1].ptr, None, None) == _lib.PM_EINVAL
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()
  assert (nbad.download() == I_SENTINEL).all()


# ------------------------------------------------------------------ SeriesSmooth
def test_series_smooth_on_a_plain_device_series(gpu):
  c = CASES[2]
  names = ["wind", "amoc", "depth"]
  dev = gpu.DeviceArray.from_host(c["v"])
  sm = gpu.SeriesSmooth((dev, names), c["sigma"], truncate=c["truncate"])
  assert sm.half == c["H"] and np.array_equal(sm.weights, c["w"])
  want = SC.restate(c)
  r = sm.compute(c["k0"], c["k1"])
  for s, nm in enumerate(names):
    assert r.trend[nm].shape == (c["n"], c["K"])
    _bits(r.trend[nm], want["trend"][:, s, :].T, (nm, "trend"))
    _bits(r.resid[nm], want["resid"][:, s, :].T, (nm, "resid"))
    assert np.array_equal(r.nbad[nm], want["nbad"][s])
  for call, key in ((sm.trend, "trend"), (sm.residual, "resid")):
    arr, nms = call(c["k0"], c["k1"])
    assert arr.shape == (c["K"], 3, c["n"]) and nms == names
    _bits(arr.download(), want[key], key)
  # the residual is a source of its own
  arr, nms = sm.residual(c["k0"], c["k1"])
  got = gpu.SeriesWindows((arr, nms), 50, step=10, detrend="constant").compute()
  ww = WC.windows(want["resid"], 0, c["K"], 50, 10, 1, "constant")
  for s, nm in enumerate(names):
    _bits(got.var[nm], ww["out"][2, :, s, :].T, (nm, "windows of the residual"))


# ------------------------------------------------------------------ the pipeline
NSUR, KP, WP, SP, SIGMA, TRUNC = 7, 60, 12, 4, 3.0, 2.0
PIPE = [(n, lag) for n in (5, 70) for lag in (1, 2)]


@pytest.mark.parametrize("n,lag", PIPE, ids=["n %d lag %d" % p for p in PIPE])
def test_gaussian_pipeline_equals_the_restated_composition(gpu, n, lag):
  """nspec = 2, K = 60, W = 12, S = 4, sigma = 3, truncate = 2 (H = 6): compute, across_members and
  trend equal smooth -> windows("constant") -> Kendall restated, bit for bit and count for count;
  the fit bit for bit; significance, given the device's surrogate series, EXACTLY, and the same
  under two max_bytes."""
  import stats_cases as STC
  c = WC.case(WP, SP, (KP - WP) // SP + 1, lag, n, 2, "constant", 60 + n + lag)
  v, k0, k1 = c["v"], c["k0"], c["k0"] + KP
  names, seed, member0 = ["wind", "amoc"], 2**63 + 12, 2**32 - 2
  labels = np.arange(n) % 2
  dev = gpu.DeviceArray.from_host(v)
  kw = dict(step=SP, detrend="gaussian", lag=lag, sigma=SIGMA, truncate=TRUNC)
  sw = gpu.SeriesWindows((dev, names), WP, groups=labels, **kw)
  want = SC.windows(v, k0, k1, WP, SP, lag, SIGMA, TRUNC)
  nwin = want["out"].shape[1]
  r = sw.compute(k0, k1)
  assert r.record_end.tolist() == [k0 + WP - 1 + SP * i for i in range(nwin)]  # absolute
  for s, nm in enumerate(names):
    assert np.array_equal(r.nused[nm], want["nused"][s])
    for i, key in enumerate(("mean", "slope", "var", "ac")):
      _bits(getattr(r, key)[nm], want["out"][i, :, s, :].T, (nm, key))
  assert (want["nused"] < nwin).any() and (want["nused"] == nwin).any()
  order, start = STC.order_of(labels)
  across = sw.across_members("var", k0, k1, quantiles=(0.5,))
  wc, ws = STC.group_stats(want["out"][2], order, start, (0.5,), 0, nwin)
  for s, nm in enumerate(names):
    assert np.array_equal(across.count[nm], wc[:, s, :].T), nm
    _bits(across.mean[nm], ws[:, s, :, 0].T, (nm, "group mean"))
    _bits(across.quantile[nm], ws[:, s, :, 5:].transpose(2, 1, 0), (nm, "median"))
  tr = sw.trend(k0, k1)
  wt = SC.trend(v, k0, k1, WP, SP, lag, SIGMA, TRUNC)
  for key in ("var", "ac"):
    for s, nm in enumerate(names):
      for f, w in zip(("conc", "disc", "tie", "nfin"), wt[key]):
        assert np.array_equal(getattr(getattr(tr, key), f)[nm], w[s]), (key, nm, f)
  # the fit
  gen = gpu.SeriesSurrogates((dev, names), detrend="gaussian", seed=seed, member0=member0,
                             sigma=SIGMA, truncate=TRUNC)
  var, ac = gen.fit(k0, k1)
  wvar, wac = SC.fit(v, k0, k1, SIGMA, TRUNC)
  fit = var._parent.download()
  _bits(fit[2, 0], wvar, "fit var")
  _bits(fit[3, 0], wac, "fit ac")
  # significance on the device's own surrogate series
  y, ynames = gen.generate(k0, k1, 0, NSUR)
  sur = y.download()
  assert sur.shape == (KP, NSUR * 2, n) and ynames[1] == "amoc#0"
  wsig = SC.significance(v, k0, k1, WP, SP, lag, SIGMA, TRUNC, NSUR, sur=sur)
  per = 16 * KP * 2 * n
  from pymoc_amd.surrogates import chunk_size
  for nb, max_bytes in ((1, 2 * per - 1), (3, 3 * per), (NSUR, 2 << 30)):
    assert chunk_size(NSUR, max_bytes, KP, 2, n, per=16) == nb
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes)
    for key in ("var", "ac"):
      g, w = getattr(sig, key), wsig[key]
      for s, nm in enumerate(names):
        what = (key, nm, "chunks of %d" % nb)
        for f in ("ge", "le", "nvalid"):
          assert np.array_equal(getattr(g, f)[nm], w[f][s]), what + (f,)
        _bits(g.tau[nm], w["tau"][s], what + ("tau",))
        _bits(g.tau[nm], getattr(tr, key).tau[nm], what + ("trend()",))
        _bits(g.p_rising[nm], w["p_rising"][s], what + ("p_rising",))
        _bits(g.p_falling[nm], w["p_falling"][s], what + ("p_falling",))
  nv = np.stack([sig.ac.nvalid[nm] for nm in names])
  assert (nv == NSUR).any() and (nv == 0).any()


# ------------------------------------------------------------------ launches and a recorder
def test_launches_and_a_recorder_source(gpu):
  """On a 16-member recorded JN2018Ensemble: with "linear" every method issues the launches it
  issued before there was a smoother; with "gaussian" the same and k_series_smooth -- once ahead
  of the window launch, and once per chunk of surrogates between the generator and the windows.
  A record window holding an unwritten record is refused in the shared words."""
  import test_stats_gpu as TG
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  names = list(rec.table.names)
  k0, k1 = 2, TG.N_SAMPLES
  K = k1 - k0
  one = 8 * K * len(names) * 16

  def spans(call):
    before = len(ens.timer.spans)
    res = call()
    return res, [name for name, _, _ in ens.timer.spans[before:]]

  lin = gpu.SeriesWindows(rec, 8, step=2)
  gau = gpu.SeriesWindows(rec, 8, step=2, detrend="gaussian", sigma=2.0)
  chunk = ["k_series_surrogates", "k_series_windows"] + ["k_series_kendall", "k_series_exceed"] * 2
  gchunk = ["k_series_surrogates", "k_series_smooth", "k_series_windows"] + chunk[2:]
  head = ["k_series_windows"] + ["k_series_kendall"] * 2
  assert spans(lambda: lin.compute(k0, k1))[1] == ["k_series_windows"]
  assert spans(lambda: lin.across_members("ac", k0, k1))[1] == ["k_series_windows"]
  assert spans(lambda: lin.trend(k0, k1))[1] == head
  assert spans(lambda: lin.significance(k0, k1, nsur=5, seed=9, max_bytes=2 * one))[1] == \
      head + ["k_series_windows"] + chunk * 3
  r, got = spans(lambda: gau.compute(k0, k1))
  assert got == ["k_series_smooth", "k_series_windows"]
  assert spans(lambda: gau.across_members("ac", k0, k1))[1] == ["k_series_smooth", "k_series_windows"]
  tr, got = spans(lambda: gau.trend(k0, k1))
  assert got == ["k_series_smooth"] + head
  sig, got = spans(lambda: gau.significance(k0, k1, nsur=5, seed=9, max_bytes=4 * one))
  assert got == ["k_series_smooth"] + head + ["k_series_windows"] + gchunk * 3
  gen = gpu.SeriesSurrogates(rec, detrend="gaussian", sigma=2.0, seed=9)
  assert spans(lambda: gen.fit(k0, k1))[1] == ["k_series_smooth", "k_series_windows"]
  assert spans(lambda: gpu.SeriesSurrogates(rec, seed=9).fit(k0, k1))[1] == ["k_series_windows"]
  assert spans(lambda: gpu.SeriesSmooth(rec, 2.0).compute(k0, k1))[1] == ["k_series_smooth"]
  # the values: the restated composition on the recorder's host view
  v = TG._series_of(rec)
  want = SC.windows(v, k0, k1, 8, 2, 1, 2.0)
  for s, nm in enumerate(names):
    _bits(r.var[nm], want["out"][2, :, s, :].T, (nm, "var"))
    _bits(sig.ac.tau[nm], tr.ac.tau[nm], (nm, "tau"))
    assert (sig.ac.nvalid[nm] == 5).all()
  assert r.record_end[0] == k0 + 7
  # an unwritten record
  words = "record %d, which was never written" % TG.N_SAMPLES
  for call in (gau.compute, gau.trend, gau.significance, gen.fit, gpu.SeriesSmooth(rec, 2.0).residual):
    with pytest.raises(ValueError, match=words):
      call()
