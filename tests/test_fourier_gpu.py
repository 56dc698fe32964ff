"""pm_series_fourier_coef, pm_series_surrogates_fourier, SeriesSurrogates(method="fourier") and
SeriesWindows.significance(method="fourier") on the device: every case of tests/fourier_cases.py
through the C-ABI bit for bit against the restatement, with the series inside a padded allocation
and sentinel outputs; independence of a surrogate from the shard, the batch and the chunk; the
whole pipeline exactly against the restated composition; every refusal of the entries; and the
launches of the default method, which are the ones issued without `method`."""
import ctypes as C

import numpy as np
import pytest

from series_harness import PAD, SPARE, V_SENTINEL, _bits, _padded, _up
import fourier_cases as FC
import windows_cases as WC

pytestmark = pytest.mark.gpu


def _guarded(gpu, size):
  """A sentinel-filled device output of `size` doubles, PAD before it and SPARE behind:
  (allocation, address of element 0)."""
  dev = _up(gpu, np.full(PAD + size + SPARE, V_SENTINEL))
  return dev, dev.ptr + 8 * PAD


def _taken(dev, shape, what):
  """The output out of its allocation; nothing before or behind it is touched."""
  size = int(np.prod(shape))
  flat = dev.download().ravel()
  assert (flat[:PAD] == V_SENTINEL).all(), (what, "before the output")
  assert (flat[PAD + size:] == V_SENTINEL).all(), (what, "behind the output")
  return flat[PAD:PAD + size].reshape(shape)


def run_coef(gpu, c, v=None):
  """pm_series_fourier_coef of the case (or of another series under its settings): coef
  [2, nf, nspec, n]."""
  from pymoc_amd import _lib
  from pymoc_amd.windows import _DETREND, stt_of
  v = c["v"] if v is None else v
  nrec, nspec, n = v.shape
  K, tab = c["K"], FC.tables(c["K"])
  keep, ptr = _padded(gpu, v)
  shape = (2, K // 2 + 1, nspec, n)
  out, out_ptr = _guarded(gpu, int(np.prod(shape)))
  d = _lib.pm_series_fourier_coef()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, c["k0"], c["k1"]
  d.detrend, d.M, d.stt, d.v = _DETREND[c["detrend"]], tab.M, stt_of(K), ptr
  tab.fill(d, ("tw", "chirp", "filt"))
  _lib.check(_lib.lib.pm_series_fourier_coef(C.byref(d), out_ptr, None))
  gpu.synchronize()
  return _taken(out, shape, (c["name"], "coef"))


def run_synthesis(gpu, c, coef, **kw):
  """pm_series_surrogates_fourier from the coefficients `coef` [2, nf, nspec, n] (inside a padded
  allocation) with the case's b0, nb, member0 and seed (edits in kw): y [K, nb * nspec, n]."""
  from pymoc_amd import _lib
  c = dict(c, **kw)
  nspec, n = coef.shape[2:]
  K, nb, tab = c["K"], c["nb"], FC.tables(c["K"])
  keep, ptr = _padded(gpu, coef)
  shape = (K, nb * nspec, n)
  out, out_ptr = _guarded(gpu, int(np.prod(shape)))
  scr, scr_ptr = _guarded(gpu, int(np.prod(shape))) if c.get("scratch") else (None, None)
  d = _lib.pm_series_surrogates_fourier()
  d.n, d.nspec, d.K, d.nb, d.b0, d.member0, d.seed = n, nspec, K, nb, c["b0"], c["member0"], c["seed"]
  d.M, d.coef, d.scratch = tab.M, ptr, scr_ptr
  tab.fill(d, tab.KEYS)
  _lib.check(_lib.lib.pm_series_surrogates_fourier(C.byref(d), out_ptr, None))
  gpu.synchronize()
  if scr is not None:  # (what it holds is unspecified; what lies around it is not touched)
    _taken(scr, shape, (c["name"], "scratch"))
  return _taken(out, shape, (c["name"], "y"))


CASES = FC.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def restated():
  """name -> the restatement of the case: computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = FC.restate(c)
    return cache[c["name"]]
  return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_entries_bit_for_bit(gpu, restated, case):
  """The coefficients, and the surrogates synthesised from the device's own coefficients, equal the
  restatement's bit for bit; a series with a non-finite record has NaN coefficients and K NaN
  records in every surrogate, no other series holds one."""
  c, want = case, restated(case)
  coef = run_coef(gpu, c)
  _bits(coef, want["coef"], (c["name"], "coef"))
  y = run_synthesis(gpu, c, coef)
  _bits(y, want["y"], (c["name"], "y"))
  # through a scratch array -- series-contiguous, then transposed -- the same bits
  _bits(run_synthesis(gpu, c, coef, scratch=True), want["y"], (c["name"], "y through scratch"))
  bad = ~np.isfinite(c["v"][c["k0"]:c["k1"]]).all(axis=0)  # [nspec, n]
  assert np.array_equal(np.isnan(coef), np.broadcast_to(bad, coef.shape)), c["name"]
  yy = y.reshape(c["K"], c["nb"], c["nspec"], c["n"])
  assert np.array_equal(np.isnan(yy), np.broadcast_to(bad, yy.shape)), c["name"]
  if c["n"] == 65:  # every style took part
    assert bad.any() and not bad.all()
    const = [(s, m) for s in range(c["nspec"]) for m in range(65) if FC.style_of(s, m, 65) == "const"]
    if c["detrend"] != "none":  # zero coefficients, zero surrogates
      for s, m in const:
        assert (coef[:, :, s, m] == 0.0).all() and (yy[:, :, s, m] == 0.0).all()


def test_a_surrogate_depends_on_its_own_series_alone(gpu, restated):
  """A shard (members [a, b) with member0 + a), a single member and a chunk [b0, b0 + nb) split as
  1 + 2 give the bits they have in the whole; another seed gives other phases."""
  for c in (CASES[-1], CASES[-2], next(k for k in CASES if k["K"] == 257 and k["n"] == 65)):
    nspec = c["nspec"]
    whole_coef = run_coef(gpu, c)
    whole = run_synthesis(gpu, c, whole_coef, nb=3)
    for a, b in ((3, 44), (64, 65), (17, 18)):
      part_coef = run_coef(gpu, c, v=np.ascontiguousarray(c["v"][:, :, a:b]))
      _bits(part_coef, whole_coef[:, :, :, a:b], (c["name"], "coef", a, b))
      part = run_synthesis(gpu, c, part_coef, nb=3, member0=c["member0"] + a)
      _bits(part, whole[:, :, a:b], (c["name"], "y", a, b))
    one = run_synthesis(gpu, c, whole_coef, nb=1)
    two = run_synthesis(gpu, c, whole_coef, nb=2, b0=c["b0"] + 1)
    _bits(one, whole[:, :nspec], (c["name"], "chunk of 1"))
    _bits(two, whole[:, nspec:], (c["name"], "chunk of 2"))
    other = run_synthesis(gpu, c, whole_coef, nb=3, seed=c["seed"] + 1)
    assert not np.array_equal(other, whole, equal_nan=True)


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_fourier_cpu as TC
  out = _up(gpu, np.full(4096, V_SENTINEL))
  for label, kw in TC.bad_coef_descriptors():
    d = TC.coef_desc(**kw)
    assert _lib.lib.pm_series_fourier_coef(C.byref(d), out.ptr, None) == _lib.PM_EINVAL, label
  for label, kw in TC.bad_synthesis_descriptors():
    d = TC.synthesis_desc(**kw)
    assert _lib.lib.pm_series_surrogates_fourier(C.byref(d), out.ptr, None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  assert (out.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ the pipeline
NSUR, KP, WP, SP, SIGMA = 7, 96, 24, 4, 6.0


@pytest.mark.parametrize("detrend", ["linear", "gaussian"])
def test_significance_equals_the_restated_composition(gpu, detrend):
  """n = 5, nspec = 2, K = 96, W = 24, S = 4, 7 surrogates: ge, le, nvalid, tau and both p-values of
  significance(method="fourier") equal the restated composition EXACTLY, in chunks of 3, of 1 and
  all at once (the counts do not depend on max_bytes); the coefficients and the surrogate series of
  SeriesSurrogates(method="fourier") equal the restatement bit for bit."""
  c = WC.case(WP, SP, (KP - WP) // SP + 1, 1, 5, 2, "linear", 61)
  v, k0, k1 = c["v"], c["k0"], c["k0"] + KP
  names, seed, member0 = ["wind", "amoc"], 2**63 + 29, 2**33 + 7
  kw = dict(sigma=SIGMA) if detrend == "gaussian" else {}
  ids = np.uint64(member0) + np.arange(5, dtype=np.uint64)
  dev = gpu.DeviceArray.from_host(v)
  gen = gpu.SeriesSurrogates((dev, names), detrend=detrend, seed=seed, member0=member0,
                             method="fourier", **kw)
  with pytest.raises(ValueError, match="has no fit"):
    gen.fit(k0, k1)
  re, im = gen.coefficients(k0, k1)
  assert re.shape == im.shape == (KP // 2 + 1, 2, 5)
  if detrend == "gaussian":
    import smooth_cases as SMC
    resid = SMC.smooth(v, k0, k1, SMC.weights(SIGMA))["resid"]
    want_coef = FC.coefficients(resid, 0, KP, "constant")
  else:
    want_coef = FC.coefficients(v, k0, k1, detrend)
  _bits(re._parent.download(), want_coef, ("coefficients", detrend))
  y, ynames = gen.generate(k0, k1, 0, NSUR)
  assert y.shape == (KP, NSUR * 2, 5) and ynames[:3] == ["wind#0", "amoc#0", "wind#1"]
  sur = y.download()
  _bits(sur, FC.surrogates(v, k0, k1, detrend, 0, NSUR, seed, ids, **kw), ("generate", detrend))
  part, _ = gen.generate(k0, k1, 4, 2)
  _bits(part.download(), sur[:, 8:12], "generate(b0 = 4, nb = 2)")
  assert np.isnan(sur).any() and not np.isnan(sur).all()

  want = FC.significance(v, k0, k1, WP, SP, 1, detrend, NSUR, seed=seed, ids=ids, nb=3, **kw)
  sw = gpu.SeriesWindows((dev, names), WP, step=SP, detrend=detrend, **kw)
  tr = sw.trend(k0, k1)
  per = (16 if detrend == "gaussian" else 8) * KP * 2 * 5
  from pymoc_amd.surrogates import chunk_size
  for nb, max_bytes in ((3, 3 * per), (1, per), (NSUR, 2 << 30)):
    assert chunk_size(NSUR, max_bytes, KP, 2, 5, per=per // (KP * 2 * 5)) == nb
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes,
                          method="fourier")
    assert sig.nsur == NSUR
    for key in ("var", "ac"):
      r, w = getattr(sig, key), want[key]
      for s, nm in enumerate(names):
        what = (detrend, key, nm, "chunks of %d" % nb)
        for f in ("ge", "le", "nvalid"):
          assert getattr(r, f)[nm].dtype == np.int32
          assert np.array_equal(getattr(r, f)[nm], w[f][s]), what + (f,)
        _bits(r.tau[nm], w["tau"][s], what + ("tau",))
        _bits(r.tau[nm], getattr(tr, key).tau[nm], what + ("trend()",))
        _bits(r.p_rising[nm], w["p_rising"][s], what + ("p_rising",))
        _bits(r.p_falling[nm], w["p_falling"][s], what + ("p_falling",))
  nv = np.stack([sig.ac.nvalid[nm] for nm in names])
  assert (nv == NSUR).any() and (nv == 0).any()


def test_the_classes_take_the_scratch_route_from_513_records(gpu):
  """K = 520 (M = 2048, one series a block): `generate` and `significance(method="fourier")` go
  through the scratch array and give the restatement's bits and counts, in chunks of 1 and of 3 (a
  surrogate counts 16 K nspec n bytes there)."""
  from pymoc_amd import fourier
  from pymoc_amd.surrogates import chunk_size
  K, W, S, n = 520, 130, 26, 3
  assert fourier.wants_scratch(K) and not fourier.wants_scratch(512)
  c = WC.case(W, S, (K - W) // S + 1, 1, n, 1, "linear", 77)
  v, k0, k1 = c["v"], c["k0"], c["k0"] + K
  seed, ids = 4242, np.arange(n, dtype=np.uint64)
  dev = gpu.DeviceArray.from_host(v)
  gen = gpu.SeriesSurrogates((dev, ["amoc"]), seed=seed, method="fourier")
  _bits(gen.generate(k0, k1, 1, 2)[0].download(),
        FC.surrogates(v, k0, k1, "linear", 1, 2, seed, ids), "generate")
  want = FC.significance(v, k0, k1, W, S, 1, "linear", 3, seed=seed, ids=ids)
  sw = gpu.SeriesWindows((dev, ["amoc"]), W, step=S)
  per = 16 * K * n
  for nb, max_bytes in ((1, per), (1, 2 * per - 1), (3, 3 * per)):
    assert chunk_size(3, max_bytes, K, 1, n, per=16) == nb
    sig = sw.significance(k0, k1, nsur=3, seed=seed, max_bytes=max_bytes, method="fourier")
    for key in ("var", "ac"):
      for f in ("ge", "le", "nvalid"):
        assert np.array_equal(getattr(getattr(sig, key), f)["amoc"], want[key][f][0]), (key, f, nb)
      _bits(getattr(sig, key).p_rising["amoc"], want[key]["p_rising"][0], (key, "p_rising", nb))
  with pytest.raises(ValueError, match="max_bytes = %d does not hold one surrogate of %d bytes"
                     % (per - 1, per)):
    sw.significance(k0, k1, nsur=3, seed=seed, max_bytes=per - 1, method="fourier")


def test_the_default_method_issues_the_launches_it_issued(gpu):
  """With method="ar1" the launch names a timer records for generate() and significance() are
  exactly those of a call that does not pass `method`; neither list holds a fourier kernel, and
  method="fourier" issues the coefficient launch once and one synthesis launch per chunk."""
  import test_stats_gpu as TG
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  names = list(rec.table.names)
  mb = 8 * 22 * len(names) * 16 * 2

  def spans(fn):
    before = len(ens.timer.spans)
    fn()
    return [name for name, _, _ in ens.timer.spans[before:]]

  sw = gpu.SeriesWindows(rec, 8, step=2)
  plain = spans(lambda: sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, max_bytes=mb))
  ar1 = spans(lambda: sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, max_bytes=mb, method="ar1"))
  assert plain == ar1 and not [nm for nm in plain if "fourier" in nm]
  chunk = ["k_series_surrogates", "k_series_windows"] + ["k_series_kendall", "k_series_exceed"] * 2
  assert plain == ["k_series_windows"] + ["k_series_kendall"] * 2 + ["k_series_windows"] + chunk * 3
  gplain = spans(lambda: gpu.SeriesSurrogates(rec, seed=99).generate(2, TG.N_SAMPLES, 0, 5))
  gar1 = spans(lambda: gpu.SeriesSurrogates(rec, seed=99, method="ar1").generate(2, TG.N_SAMPLES, 0, 5))
  assert gplain == gar1 == ["k_series_windows", "k_series_surrogates"]
  four = spans(lambda: sw.significance(2, TG.N_SAMPLES, nsur=5, seed=99, max_bytes=mb,
                                       method="fourier"))
  fchunk = ["k_series_surrogates_fourier"] + chunk[1:]
  assert four == (["k_series_windows"] + ["k_series_kendall"] * 2 + ["k_series_fourier_coef"]
                  + fchunk * 3)
  gfour = spans(lambda: gpu.SeriesSurrogates(rec, seed=99, method="fourier").generate(
      2, TG.N_SAMPLES, 0, 5))
  assert gfour == ["k_series_fourier_coef", "k_series_surrogates_fourier"]
