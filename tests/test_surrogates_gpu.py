"""pm_series_surrogates, pm_series_exceed, SeriesSurrogates and SeriesWindows.significance on the
device: the deviates to the bound include/pymoc_hip.h states, the recurrence bit for bit on the
device's own deviates, what the launches leave alone, independence of a surrogate from the chunk
and the batch, the counting kernel exactly, the whole pipeline exactly against the restatement
(tests/surrogate_cases.py) on the device's surrogate series, and a recorded noise ensemble."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, PAD, SPARE, V_SENTINEL, _bits, _padded, _up
import noise_cases as NC
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


def run(gpu, c, with_xi=True, **kw):
  """One launch of the case (with the edits `kw`): dict(y, xi), each [K, nb * nspec, n]."""
  from pymoc_amd import _lib
  c = dict(c, **kw)
  n, nspec, K, nb = c["n"], c["nspec"], c["K"], c["nb"]
  fits = [_padded(gpu, c[key]) for key in ("var", "ac")]
  shape = (K, nb * nspec, n)
  size = int(np.prod(shape))
  y, y_ptr = _guarded(gpu, size, np.float64, V_SENTINEL)
  xi, xi_ptr = _guarded(gpu, size, np.float64, V_SENTINEL)
  d = _lib.pm_series_surrogates()
  d.n, d.nspec, d.K, d.nb, d.b0, d.member0, d.seed = n, nspec, K, nb, c["b0"], c["member0"], c["seed"]
  d.var, d.ac = fits[0][1], fits[1][1]
  _lib.check(_lib.lib.pm_series_surrogates(C.byref(d), y_ptr, xi_ptr if with_xi else None, None))
  gpu.synchronize()
  got = dict(y=_taken(y, size, shape, V_SENTINEL, c["name"]))
  if with_xi:
    got["xi"] = _taken(xi, size, shape, V_SENTINEL, c["name"])
  else:
    assert (xi.download() == V_SENTINEL).all()
  return got


CASES = SGC.cases()
IDS = [c["name"] for c in CASES]


def _ids(c, n=None):
  return np.uint64(c["member0"]) + np.arange(c["n"] if n is None else n, dtype=np.uint64)


@pytest.fixture(scope="module")
def results(gpu):
  """name -> the device result of the case: computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = run(gpu, c)
    return cache[c["name"]]
  return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deviates_within_the_stated_bound(gpu, results, case):
  """|xi - noise_cases.deviate| <= 16 * 2^-53 * R, R from the host's uniforms; R == 0: equal."""
  c, xi = case, results(case)["xi"]
  ref, R = SGC.deviates(c["K"], c["b0"], c["nb"], c["nspec"], c["seed"], _ids(c))
  zero = R == 0
  assert np.array_equal(xi[zero], ref[zero])
  ratio = float(np.max(np.abs(xi - ref)[~zero] / (16.0 * NC.EPS * R[~zero])))
  print("%s: largest |xi - restatement| / (16 * 2^-53 * R) = %.3f" % (c["name"], ratio))
  assert ratio <= 1.0, ratio
  assert np.isfinite(xi).all() and abs(xi.mean()) < 5.0 / np.sqrt(xi.size)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recurrence_bit_for_bit_on_the_device_deviates(gpu, results, case):
  c, got = case, results(case)
  want = SGC.surrogates(c["var"], c["ac"], c["K"], c["b0"], c["nb"], c["seed"], _ids(c), xi=got["xi"])
  _bits(got["y"], want, (c["name"], "y"))
  # the NaN series: all K values, in every surrogate; no other series holds one
  with np.errstate(all="ignore"):
    bad = ~(np.isfinite(c["ac"]) & np.isfinite(np.sqrt(c["var"])))
  y = got["y"].reshape(c["K"], c["nb"], c["nspec"], c["n"])
  assert np.array_equal(np.isnan(y), np.broadcast_to(bad, y.shape)), c["name"]
  if c["n"] == 5:
    assert np.nonzero(bad.ravel())[0].tolist() == list(SGC.NAN_SERIES)
  # the same without xi_out
  _bits(run(gpu, c, with_xi=False)["y"], got["y"], (c["name"], "xi_out NULL"))


def test_a_surrogate_does_not_depend_on_the_chunk_or_the_batch(gpu, results):
  for c in (CASES[0], CASES[-1]):  # n 5, nspec 2, K 37; member0 0 and 2^32 - 3
    nspec = c["nspec"]
    whole = run(gpu, c, b0=0, nb=7)
    one = run(gpu, c, b0=5, nb=1)
    part = run(gpu, c, b0=0, nb=7, n=2, member0=c["member0"] + 3,
               var=np.ascontiguousarray(c["var"][:, 3:5]), ac=np.ascontiguousarray(c["ac"][:, 3:5]))
    for key in ("y", "xi"):
      # the chunk (b0 = 5, nb = 1) is plane 5 of (b0 = 0, nb = 7)
      _bits(one[key], whole[key][:, 5 * nspec:6 * nspec], (c["name"], key, "chunk"))
      # the case's own chunk inside it
      if c["b0"] + c["nb"] <= 7:
        _bits(results(c)[key], whole[key][:, c["b0"] * nspec:(c["b0"] + c["nb"]) * nspec],
              (c["name"], key, "the case"))
      # members [3, 5) with member0 + 3
      _bits(part[key], whole[key][:, :, 3:5], (c["name"], key, "members [3, 5)"))
  # another seed: other deviates
  other = run(gpu, CASES[0], seed=CASES[0]["seed"] + 1)
  assert not np.array_equal(other["xi"], results(CASES[0])["xi"])


# ------------------------------------------------------------------ pm_series_exceed
def run_exceed(gpu, obs, sur, start, calls=None):
  """The accumulators after the calls (row ranges of the surrogate planes; default: one call over
  all) on accumulators that hold `start`."""
  from pymoc_amd import _lib
  nspec, n = obs[0].shape
  size = nspec * n
  acc = [_guarded(gpu, size, np.int32, I_SENTINEL) for _ in range(3)]
  for dev, _ in acc:
    host = dev.download()
    host[PAD:PAD + size] = start
    dev.upload(host)
  dobs = [_up(gpu, a) for a in obs]
  nb_all = sur[0].shape[0] // nspec
  for i0, i1 in calls or [(0, nb_all)]:
    dsur = [_up(gpu, np.ascontiguousarray(a[i0 * nspec:i1 * nspec])) for a in sur]
    d = _lib.pm_series_exceed()
    d.n, d.nspec, d.nb = n, nspec, i1 - i0
    d.obs_conc, d.obs_disc, d.obs_tie = (a.ptr for a in dobs)
    d.sur_conc, d.sur_disc, d.sur_tie = (a.ptr for a in dsur)
    _lib.check(_lib.lib.pm_series_exceed(C.byref(d), acc[0][1], acc[1][1], acc[2][1], None))
    gpu.synchronize()
  return [_taken(dev, size, (nspec, n), I_SENTINEL, "exceed") for dev, _ in acc]


def test_exceed_is_exact_on_constructed_counts(gpu):
  obs, sur = SGC.exceed_case()
  want = SGC.exceed(obs, sur)
  assert want[2].max() == 4 and want[2].min() == 0  # (n0 == tie on either side is in the table)
  for got, w in zip(run_exceed(gpu, obs, sur, 0), want):
    assert np.array_equal(got, w)
  # added to what the accumulators hold; two calls equal one
  for got, w in zip(run_exceed(gpu, obs, sur, 11), want):
    assert np.array_equal(got, w + 11)
  for got, w in zip(run_exceed(gpu, obs, sur, 0, calls=[(0, 1), (1, 4)]), want):
    assert np.array_equal(got, w)
  # the counts of a Kendall case, wide enough for several blocks: index 0 against all three
  c = next(k for k in WC.kendall_cases() if k["v"].shape[1:] == (3, 65) and k["k1"] - k["k0"] == 65)
  cnt = WC.kendall(c["v"], c["k0"], c["k1"])
  obs = tuple(np.ascontiguousarray(np.repeat(a[:1], 5, axis=0)[:, :60].reshape(1, 300)) for a in cnt[:3])
  sur = tuple(np.ascontiguousarray(np.tile(a, (1, 5))[:, :300]) for a in cnt[:3])
  want = SGC.exceed(obs, sur)
  assert 0 < want[0].max() <= 3 and (want[2] == 0).any() and (want[2] == 3).any()
  for got, w in zip(run_exceed(gpu, obs, sur, 0), want):
    assert np.array_equal(got, w)


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_surrogates_cpu as TC
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(2)]
  for label, kw in TC.bad_descriptors():
    d = TC.desc(**kw)
    assert _lib.lib.pm_series_surrogates(C.byref(d), out[0].ptr, out[1].ptr, None) == _lib.PM_EINVAL, label
  acc = [_up(gpu, np.full(4096, I_SENTINEL, dtype=np.int32)) for _ in range(3)]
  for label, kw in TC.bad_exceed_descriptors():
    d = TC.edesc(**kw)
    assert _lib.lib.pm_series_exceed(C.byref(d), *(a.ptr for a in acc), None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()
  for a in acc:
    assert (a.download() == I_SENTINEL).all()


# ------------------------------------------------------------------ the pipeline
NSUR, KP, WP, SP = 7, 60, 12, 4
PIPE = [(n, lag, det) for n in (5, 70) for lag in (1, 2) for det in WC.DETRENDS]


@pytest.mark.parametrize("n,lag,detrend", PIPE, ids=["n %d lag %d %s" % p for p in PIPE])
def test_significance_equals_the_restatement_on_the_device_surrogates(gpu, n, lag, detrend):
  """nspec = 2, K = 60, W = 12, S = 4, 7 surrogates in chunks of 1, 3 and all: the counts, the
  observed tau and the p-values equal the restatement's pipeline run on the surrogate series
  SeriesSurrogates.generate gives for the same arguments, EXACTLY; the fit bit for bit."""
  c = WC.case(WP, SP, (KP - WP) // SP + 1, lag, n, 2, detrend, 40 + n + lag)
  v, k0, k1 = c["v"], c["k0"], c["k0"] + KP
  styles = {WC.style_of(s, m) for s in range(2) for m in range(n)}
  assert {"nan1", "const", "ar1"} <= styles
  names, seed, member0 = ["wind", "amoc"], 2**63 + 11, 2**32 - 2
  dev = gpu.DeviceArray.from_host(v)
  gen = gpu.SeriesSurrogates((dev, names), detrend=detrend, seed=seed, member0=member0)
  # the fit
  var, ac = gen.fit(k0, k1)
  assert var.shape == ac.shape == (1, 2, n)
  fit = var._parent.download()
  want_fit = WC.windows(v, k0, k1, KP, 1, 1, detrend)["out"]
  _bits(fit, want_fit, ("fit", detrend))
  # the surrogate series, as a source of its own
  y, ynames = gen.generate(k0, k1, 0, NSUR)
  assert y.shape == (KP, NSUR * 2, n) and ynames[:3] == ["wind#0", "amoc#0", "wind#1"]
  assert len(ynames) == 2 * NSUR and ynames[-1] == "amoc#6"
  sur = y.download()
  with np.errstate(all="ignore"):
    bad = ~(np.isfinite(want_fit[3, 0]) & np.isfinite(np.sqrt(want_fit[2, 0])))
  assert bad.any() and not bad.all()
  assert np.array_equal(np.isnan(sur), np.broadcast_to(np.tile(bad, (NSUR, 1)), sur.shape))
  part, _ = gen.generate(k0, k1, 4, 2)
  _bits(part.download(), sur[:, 8:12], "generate(b0 = 4, nb = 2)")
  sub = gpu.SeriesWindows((y, ynames), WP, step=SP, detrend=detrend, lag=lag).trend()
  want = SGC.significance(v, k0, k1, WP, SP, lag, detrend, NSUR, sur=sur)
  per = 8 * KP * 2 * n
  sw = gpu.SeriesWindows((dev, names), WP, step=SP, detrend=detrend, lag=lag)
  tr = sw.trend(k0, k1)
  from pymoc_amd.surrogates import chunk_size
  for nb, max_bytes in ((1, per), (1, 2 * per - 1), (3, 3 * per), (NSUR, NSUR * per), (NSUR, 2 << 30)):
    assert chunk_size(NSUR, max_bytes, KP, 2, n) == nb
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes)
    for key in ("var", "ac"):
      r, w = getattr(sig, key), want[key]
      for s, nm in enumerate(names):
        what = (key, nm, "chunks of %d" % nb)
        for f in ("ge", "le", "nvalid"):
          assert getattr(r, f)[nm].dtype == np.int32
          assert np.array_equal(getattr(r, f)[nm], w[f][s]), what + (f,)
        _bits(r.tau[nm], w["tau"][s], what + ("tau",))
        _bits(r.tau[nm], getattr(tr, key).tau[nm], what + ("trend()",))
        ge, le, nv = (getattr(r, f)[nm].astype(np.float64) for f in ("ge", "le", "nvalid"))
        none = np.isnan(r.tau[nm]) | (nv == 0)
        _bits(r.p_rising[nm], np.where(none, np.nan, (1.0 + ge) / (1.0 + nv)), what + ("p_rising",))
        _bits(r.p_falling[nm], np.where(none, np.nan, (1.0 + le) / (1.0 + nv)), what + ("p_falling",))
        _bits(r.p_rising[nm], w["p_rising"][s], what)
  # the surrogates' own trends through the public route are what the restatement counted against
  for key, i in (("var", 2), ("ac", 3)):
    ws = WC.windows(sur, 0, KP, WP, SP, lag, detrend)["out"][i]
    cnt = WC.kendall(ws, 0, ws.shape[0])
    for p, nm in enumerate(ynames):
      assert np.array_equal(getattr(sub, key).conc[nm], cnt[0][p]), (key, nm)
  # every kind of series took part: some with all surrogates counted, some with none
  nv = np.stack([sig.ac.nvalid[nm] for nm in names])
  assert (nv == NSUR).any() and (nv == 0).any()
  assert (nv[bad] == 0).all()
  # other seeds and member numbers give other surrogates
  for kw in (dict(seed=seed + 1), dict(member0=member0 + 1)):
    o = gpu.SeriesSurrogates((dev, names), **dict(dict(detrend=detrend, seed=seed, member0=member0), **kw))
    assert not np.array_equal(o.generate(k0, k1, 0, 1)[0].download(), sur[:, :2], equal_nan=True)


def test_fit_of_a_record_window_of_2_mod_4_records(gpu):
  """K = 22: W (W^2 - 1) / 12 = 885.5.  Under constant detrending (where the restatement forms no
  slope) the fit is the restatement's bit for bit; under linear detrending it runs and removes
  the trend."""
  c = WC.case(WP, SP, 13, 1, 5, 2, "constant", 3)
  v, k0, k1 = c["v"], c["k0"], c["k0"] + 22
  dev = gpu.DeviceArray.from_host(v)
  var, _ = gpu.SeriesSurrogates((dev, ["wind", "amoc"]), detrend="constant").fit(k0, k1)
  _bits(var._parent.download(), WC.windows(v, k0, k1, 22, 1, 1, "constant")["out"], "constant")
  lin, _ = gpu.SeriesSurrogates((dev, ["wind", "amoc"]), detrend="linear").fit(k0, k1)
  lin, con = lin._parent.download(), var._parent.download()
  assert np.array_equal(np.isnan(lin[0]), np.isnan(con[0]))
  assert lin[2, 0, 0, 1] == 0.0 and con[2, 0, 0, 1] > 0.0  # the exact ramp
  fin = np.isfinite(con[2, 0])
  assert (lin[2, 0][fin] <= con[2, 0][fin]).all()


def test_significance_on_a_recorded_noise_ensemble(gpu):
  """An IndexRecorder on a 16-member JN2018Ensemble under NoiseForcing: significance runs, its
  observed taus are trend()'s, member0 defaults to the ensemble's, the recorder route and the
  (array, names) route agree, and the launches are the ones windows.py lists."""
  import test_stats_gpu as TG
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  names = list(rec.table.names)
  sw = gpu.SeriesWindows(rec, 8, step=2)
  with pytest.raises(ValueError, match="record %d, which was never written" % TG.N_SAMPLES):
    sw.significance()
  tr = sw.trend(2, TG.N_SAMPLES)
  before = len(ens.timer.spans)
  sig = sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, max_bytes=8 * 22 * len(names) * 16 * 2)
  spans = [name for name, _, _ in ens.timer.spans[before:]]
  chunk = ["k_series_surrogates", "k_series_windows"] + ["k_series_kendall", "k_series_exceed"] * 2
  assert spans == ["k_series_windows"] + ["k_series_kendall"] * 2 + ["k_series_windows"] + chunk * 3
  assert sig.nsur == 5
  gen = gpu.SeriesSurrogates(rec, seed=99)
  assert gen.member0 == ens._member0 == 0 and gen.stream is ens.stream
  v = TG._series_of(rec)
  sur = gen.generate(2, TG.N_SAMPLES, 0, 5)[0].download()
  assert np.isfinite(sur).all()
  want = SGC.significance(v, 2, TG.N_SAMPLES, 8, 2, 1, "linear", 5, sur=sur)
  explicit = sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, member0=ens._member0)
  shifted = sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, member0=3)
  plain = gpu.SeriesWindows((gpu.DeviceArray.from_host(v), names), 8, step=2).significance(
      2, TG.N_SAMPLES, nsur=5, seed=99)
  differs = False
  for key in ("var", "ac"):
    r = getattr(sig, key)
    for s, nm in enumerate(names):
      _bits(r.tau[nm], getattr(tr, key).tau[nm], (key, nm, "tau"))
      assert (r.nvalid[nm] == 5).all() and np.isfinite(r.p_rising[nm]).all()
      assert (r.p_rising[nm] >= 1.0 / 6.0).all() and (r.p_rising[nm] <= 1.0).all()
      for f in ("ge", "le", "nvalid"):
        assert np.array_equal(getattr(r, f)[nm], want[key][f][s]), (key, nm, f)
        assert np.array_equal(getattr(r, f)[nm], getattr(getattr(explicit, key), f)[nm])
        assert np.array_equal(getattr(r, f)[nm], getattr(getattr(plain, key), f)[nm])
      differs |= not np.array_equal(r.ge[nm], getattr(shifted, key).ge[nm])
  assert differs  # (member0 = 3: other deviates)
