"""pm_series_dfa and SeriesWindows(dfa=...) on the device: every case of tests/dfa_cases.py through
the C-ABI -- F2 bit for bit against the restatement, alpha within the derived bound of its
extended-precision evaluation from the device's own F2 -- what the launch leaves alone,
independence of a member from the batch and of a record window from the series around it, the
class against the restated composition on the device's alpha series, and the launches of a
SeriesWindows without `dfa`."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _collect, _out, _padded, _up
import dfa_cases as DC
import surrogate_cases as SGC
import windows_cases as WC

pytestmark = pytest.mark.gpu


def run(gpu, c, v=None, k0=None, k1=None, with_f2=True):
  """One launch of the case's settings (on another series / record window if given) into
  sentinel-filled outputs; nothing behind an output's last element is touched."""
  from pymoc_amd import _lib
  v = c["v"] if v is None else v
  k0, k1 = (c["k0"], c["k1"]) if k0 is None else (k0, k1)
  nrec, nspec, n = v.shape
  nwin, nq = WC.nwin_of(k1 - k0, c["W"], c["S"]), len(c["scales"])
  series, v_ptr = _padded(gpu, v)
  shapes = dict(alpha=((nwin, nspec, n), np.float64, V_SENTINEL))
  if with_f2:
    shapes["f2"] = ((nq, nwin, nspec, n), np.float64, V_SENTINEL)
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  d = _lib.pm_series_dfa()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, k0, k1
  d.window, d.step, d.detrend = c["W"], c["S"], DC.DETRENDS.index(c["detrend"])
  d.v, d.stt, d.nq = v_ptr, DC.stt_of(c["W"]), nq
  w = DC.weights_of(c["scales"])
  for q, s in enumerate(c["scales"]):
    d.scale[q], d.suu[q], d.weight[q] = s, DC.suu_of(s), w[q]
  _lib.check(_lib.lib.pm_series_dfa(C.byref(d), out["alpha"][0].ptr,
                                    out["f2"][0].ptr if with_f2 else None, None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


CASES = DC.cases()
IDS = [c["name"] for c in CASES]
WIDE = [c for c in CASES if c["v"].shape[2] == 37]


@pytest.fixture(scope="module")
def results(gpu):
  """name -> the device result of the case: computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = run(gpu, c)
    return cache[c["name"]]
  return get


def _alpha_fraction(alpha, f2, scales, what):
  """alpha against alpha_of in np.longdouble from the same F2: the NaN pattern exactly, and the
  largest |difference| / alpha_bound (<= 1 asserted by the caller)."""
  ref = DC.alpha_of(f2, scales, dtype=np.longdouble)
  fin = ~np.isnan(ref.astype(np.float64))
  assert np.array_equal(~np.isnan(alpha), fin), (what, "alpha's NaN pattern")
  assert np.isfinite(alpha[fin]).all(), what
  if not fin.any():
    return 0.0
  err = np.abs(alpha.astype(np.longdouble) - ref).astype(np.float64)[fin]
  bound = DC.alpha_bound(f2, scales)[fin]
  with np.errstate(all="ignore"):
    return float(np.where(err == 0.0, 0.0, err / bound).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_f2_bit_for_bit_and_alpha_within_its_bound(gpu, results, case):
  """F2 equals the restatement bit for bit (the NaN pattern, signed zeros, inf where the squares
  overflow, the denormal-near `small`); alpha is NaN exactly where the restatement's is, finite
  elsewhere, and within c(nq) 2^-53 sum |w_q ln F2_q| of its extended-precision value; alpha
  without F2 stored and a copied-out record window give the same bits; pm_series_windows marks the
  same windows unused.  Observed on an MI355X (one run): the largest fraction of the alpha bound
  over the table is 0.41 (W = 64, scales 4 and 16); DESIGN.md section 27 lists it per case."""
  import test_windows_gpu as TW
  c, got, want = case, results(case), DC.restate(case)
  _bits(got["f2"], want["f2"], (c["name"], "f2"))
  assert np.array_equal(np.isnan(got["alpha"]), np.isnan(want["alpha"])), c["name"]
  assert np.array_equal(np.isnan(got["f2"][0]), ~want["used"]), c["name"]
  frac = _alpha_fraction(got["alpha"], got["f2"], c["scales"], c["name"])
  print("\n%-62s largest |d alpha| / bound %.3g" % (c["name"], frac))
  assert frac <= 1.0, (c["name"], frac)
  # alpha alone: the same bits
  alone = run(gpu, c, with_f2=False)
  _bits(alone["alpha"], got["alpha"], (c["name"], "alpha with f2 = NULL"))
  # the same records as a series of their own: the same bits
  own = run(gpu, c, v=np.ascontiguousarray(c["v"][c["k0"]:c["k1"]]), k0=0, k1=c["k1"] - c["k0"])
  for k in ("alpha", "f2"):
    _bits(own[k], got[k], (c["name"], k, "own series"))
  # pm_series_windows on the same series: unchanged, and the same windows used
  wn = TW.run(gpu, dict(c, Lg=1))
  assert np.array_equal(np.isnan(wn["out"][0]), np.isnan(got["f2"][0])), c["name"]
  assert c["W"] % 4 != 2  # (windows_cases states stt for such W only)
  _bits(wn["out"], WC.windows(c["v"], c["k0"], c["k1"], c["W"], c["S"], 1, c["detrend"])["out"],
        (c["name"], "pm_series_windows"))


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_a_member_does_not_depend_on_the_batch(gpu, results, case):
  """A shard (members 5 .. 20 of 37) and a single member give the bits they have in the batch."""
  c, whole = case, results(case)
  for m0, m1 in ((5, 21), (9, 10)):
    part = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, m0:m1]))
    for k in ("alpha", "f2"):
      _bits(part[k], whole[k][..., m0:m1], (c["name"], k, "members [%d, %d)" % (m0, m1)))


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_dfa_cpu as TC
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(2)]
  for label, kw in TC.bad_descriptors():
    d = TC.desc(**kw)
    assert _lib.lib.pm_series_dfa(C.byref(d), out[0].ptr, out[1].ptr, None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ SeriesWindows(dfa=...)
NSUR, KP, WP, SP = 3, 96, 20, 4
SCALES = (4, 5)
NAMES = ["wind", "amoc"]


def _ensemble(n=5):
  """A dfa_cases series of 2 indices (every kind of member for n >= 11; AR(1), ramps, constants,
  a NaN in the first window for n = 5) with the record window [3, 3 + 96)."""
  c = DC.case(WP, SP, (KP - WP) // SP + 1, n, 2, "linear", SCALES, 70 + n)
  assert c["k1"] - c["k0"] == KP + 3
  return c["v"], c["k0"], c["k0"] + KP


def _check_trend(tr, series, what):
  want = WC.kendall(series, 0, series.shape[0])
  for s, nm in enumerate(NAMES):
    for key, w in zip(("conc", "disc", "tie", "nfin"), want):
      assert np.array_equal(getattr(tr, key)[nm], w[s]), (what, nm, key)
    _bits(tr.tau[nm], WC.tau_b(want[0][s], want[1][s], want[2][s]), (what, nm, "tau"))


def _alpha_series(r):
  """[nwin, nspec, n] from a `Windows`' dfa [name] -> [n, nwin]."""
  return np.stack([r.dfa[nm].T for nm in r.names], axis=1)


def _check_sig(sig, obs, sur_alpha, nspec, what):
  """`sig` (a TrendSignificance) against the restated composition: Kendall of the observed alpha
  series [nwin, nspec, n], of the surrogates' [nwin, nsur * nspec, n], the exceedance counts and
  the p-values -- exactly."""
  nwin = obs.shape[0]
  counts = WC.kendall(obs, 0, nwin)
  acc = SGC.exceed(counts, WC.kendall(sur_alpha, 0, nwin))
  want = DC.of_counts(counts, acc)
  for s, nm in enumerate(NAMES):
    for f in ("ge", "le", "nvalid"):
      assert np.array_equal(getattr(sig, f)[nm], want[f][s]), (what, nm, f)
    for f in ("tau", "p_rising", "p_falling"):
      _bits(getattr(sig, f)[nm], want[f][s], (what, nm, f))
  return want


def test_compute_across_members_and_trend(gpu):
  """compute() returns the C-ABI's bits in the documented shapes; across_members("dfa") is
  SeriesStats of the device's alpha series; trend().dfa its Kendall counts; the four other
  indicators are what they are without dfa."""
  import stats_cases as SC
  v, k0, k1 = _ensemble(37)
  n, nwin = 37, (KP - WP) // SP + 1
  labels = np.array([40, -3, 7])[np.arange(n) % 3]
  dev = gpu.DeviceArray.from_host(v)
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, dfa=SCALES, groups=labels)
  plain = gpu.SeriesWindows((dev, NAMES), WP, step=SP, groups=labels)
  r, p = sw.compute(k0, k1), plain.compute(k0, k1)
  c = dict(v=v, k0=k0, k1=k1, W=WP, S=SP, detrend="linear", scales=SCALES, name="class")
  raw = run(gpu, c)
  assert r.dfa_scales == SCALES and sw.dfa_scales == SCALES
  for s, nm in enumerate(NAMES):
    assert r.dfa[nm].shape == (n, nwin) and r.dfa_f2[nm].shape == (n, nwin, 2)
    _bits(r.dfa[nm], raw["alpha"][:, s, :].T, (nm, "dfa"))
    _bits(r.dfa_f2[nm], raw["f2"][:, :, s, :].transpose(2, 1, 0), (nm, "dfa_f2"))
    for key in ("mean", "slope", "var", "ac"):
      _bits(getattr(r, key)[nm], getattr(p, key)[nm], (nm, key))
    assert np.array_equal(r.nused[nm], p.nused[nm])
  want = DC.restate(c)
  _bits(raw["f2"], want["f2"], "f2")
  assert np.isfinite(raw["alpha"]).any() and np.isnan(raw["alpha"]).any()
  alpha = _alpha_series(r)
  _bits(alpha, raw["alpha"], "alpha series")
  # True: the default scales
  assert gpu.SeriesWindows((dev, NAMES), WP, step=SP, dfa=True).compute(k0, k1).dfa_scales == (4, 5)
  q = (0.05, 0.5, 0.95)
  order, start = SC.order_of(labels)
  across = sw.across_members("dfa", k0, k1, quantiles=q)
  assert sw.group_labels.tolist() == [-3, 7, 40]
  wc, ws = SC.group_stats(alpha, order, start, q, 0, nwin)
  for s, nm in enumerate(NAMES):
    assert across.mean[nm].shape == (3, nwin) and across.quantile[nm].shape == (3, 3, nwin)
    assert np.array_equal(across.count[nm], wc[:, s, :].T), nm
    for j, stat in enumerate(("mean", "var", "min", "max", "sum")):
      _bits(getattr(across, stat)[nm], ws[:, s, :, j].T, (nm, stat))
    _bits(across.quantile[nm], ws[:, s, :, 5:].transpose(2, 1, 0), (nm, "quantile"))
  tr, trp = sw.trend(k0, k1), plain.trend(k0, k1)
  _check_trend(tr.dfa, alpha, "dfa")
  for key in ("var", "ac"):
    for nm in NAMES:
      assert np.array_equal(getattr(tr, key).conc[nm], getattr(trp, key).conc[nm])
  assert (tr.dfa.nfin["wind"] == nwin).any() and (tr.dfa.nfin["wind"] < nwin).any()


SIG = [("linear", "ar1"), ("linear", "fourier"), ("gaussian", "ar1"), ("gaussian", "fourier")]


@pytest.mark.parametrize("detrend,method", SIG, ids=["%s %s" % p for p in SIG])
def test_significance_equals_the_restated_composition(gpu, detrend, method):
  """significance().dfa: counts, taus and p-values equal the restated Kendall + exceedance
  composition on the device's alpha series -- the record's from compute(), the surrogates' from
  SeriesWindows(dfa=...) on the series SeriesSurrogates.generate gives for the same arguments --
  exactly, whole and with max_bytes forcing chunks of 2 + 1 surrogates; var and ac are what they
  are without dfa."""
  v, k0, k1 = _ensemble(5)
  dev = gpu.DeviceArray.from_host(v)
  kw = dict(sigma=5.0) if detrend == "gaussian" else {}
  seed, member0 = 2**63 + 7, 2**32 - 2
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, detrend=detrend, dfa=SCALES, **kw)
  plain = gpu.SeriesWindows((dev, NAMES), WP, step=SP, detrend=detrend, **kw)
  obs = _alpha_series(sw.compute(k0, k1))
  gen = gpu.SeriesSurrogates((dev, NAMES), detrend=detrend, seed=seed, member0=member0,
                             method=method, **kw)
  y, ynames = gen.generate(k0, k1, 0, NSUR)
  sub = gpu.SeriesWindows((y, ynames), WP, step=SP, detrend=detrend, dfa=SCALES, **kw).compute()
  sur_alpha = np.stack([sub.dfa[nm].T for nm in ynames], axis=1)
  assert sur_alpha.shape == (obs.shape[0], NSUR * 2, 5) and np.isfinite(sur_alpha).any()
  per = 16 * KP * 2 * 5 if detrend == "gaussian" else 8 * KP * 2 * 5
  ref = plain.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, method=method)
  for max_bytes in (2 << 30, 2 * per):
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes,
                          method=method)
    want = _check_sig(sig.dfa, obs, sur_alpha, 2, (detrend, method, max_bytes))
    for key in ("var", "ac"):
      for nm in NAMES:
        for f in ("ge", "le", "nvalid"):
          assert np.array_equal(getattr(getattr(sig, key), f)[nm], getattr(getattr(ref, key), f)[nm])
  assert sig.nsur == NSUR and (want["nvalid"] == NSUR).any() and (want["nvalid"] == 0).any()
  tr = sw.trend(k0, k1)
  for nm in NAMES:
    _bits(sig.dfa.tau[nm], tr.dfa.tau[nm], (nm, "trend()"))


def test_significance_until(gpu):
  """significance(until=).dfa, linear detrending: the record censored at the amoc's first
  detectable record, the surrogates of the ranged fit censored where the record is; the restated
  composition on the device's alpha series of both, exactly."""
  import shifts_cases as SHC
  import test_shifts_gpu as TS
  from pymoc_amd.shifts import launch_fit_ranged
  v, k0, k1 = TS._ensemble()
  K = k1 - k0
  dev = gpu.DeviceArray.from_host(v)
  sh = gpu.SeriesShifts((dev, NAMES), TS.LP, direction=dict(wind=1, amoc=-1), threshold=5.0)
  sh.detect(k0, k1)
  y, _ = sh.censored(by="amoc")
  end = sh.end.download()
  assert (end < K).any() and (end == K).any()
  seed, member0 = 2**63 + 5, 2**32 - 2
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, dfa=SCALES)
  obs = _alpha_series(gpu.SeriesWindows((y, NAMES), WP, step=SP, dfa=SCALES).compute())
  fit = launch_fit_ranged(y, (K, 2, 5), 0, K, "linear", sh.end, None, None)
  gen = gpu.SeriesSurrogates((dev, NAMES), detrend="linear", seed=seed, member0=member0)
  ysur = gpu.DeviceArray((K, NSUR * 2, 5), np.float64)
  gen._launch(fit, K, 0, NSUR, ysur)
  cut = SHC.censor(ysur.download(), np.where(end >= K, -1, end), nb=NSUR)[0]
  ynames = gen.names_of(0, NSUR)
  sub = gpu.SeriesWindows((gpu.DeviceArray.from_host(cut), ynames), WP, step=SP, dfa=SCALES).compute()
  sur_alpha = np.stack([sub.dfa[nm].T for nm in ynames], axis=1)
  sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, until=sh)
  want = _check_sig(sig.dfa, obs, sur_alpha, 2, "until")
  assert (want["nvalid"] == NSUR).any()
  whole = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0)
  assert not np.array_equal(whole.dfa.tau["amoc"], sig.dfa.tau["amoc"], equal_nan=True)


class _Recorder(object):
  """What SeriesWindows reads off an IndexRecorder, around a plain device series: a launch timer
  without an ensemble run."""

  class _T(object):
    names = NAMES

  class _E(object):
    stream = None
    _member0 = 0

  def __init__(self, values, timer):
    self._values, self.table, self.ens = values, self._T(), self._E()
    self.ens.timer = timer
    self.steps = np.arange(values.shape[0]) * 12


def test_without_dfa_the_launches_and_results_are_what_they_were(gpu):
  """dfa=None: the span names of compute, trend and significance are the lists of the commit
  before this indicator, written out here, and no result has a `dfa` attribute; with dfa the DFA
  launch follows the window launch, and every trend gains one Kendall (and exceedance) launch."""
  from pymoc_amd.device import LaunchTimer
  v, k0, k1 = _ensemble(5)
  per = 8 * KP * 2 * 5
  timer = LaunchTimer()
  rec = _Recorder(gpu.DeviceArray.from_host(v), timer)

  def spans_of(call):
    before = len(timer.spans)
    res = call()
    return res, [name for name, _, _ in timer.spans[before:]]

  sw = gpu.SeriesWindows(rec, WP, step=SP)
  r, spans = spans_of(lambda: sw.compute(k0, k1))
  assert spans == ["k_series_windows"]
  assert not [a for a in vars(r) if "dfa" in a]
  tr, spans = spans_of(lambda: sw.trend(k0, k1))
  assert spans == ["k_series_windows", "k_series_kendall", "k_series_kendall"]
  assert not hasattr(tr, "dfa")
  sig, spans = spans_of(lambda: sw.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=2 * per))
  assert spans == (["k_series_windows", "k_series_kendall", "k_series_kendall", "k_series_windows"]
                   + ["k_series_surrogates", "k_series_windows", "k_series_kendall",
                      "k_series_exceed", "k_series_kendall", "k_series_exceed"] * 2)
  assert not hasattr(sig, "dfa")
  _, spans = spans_of(lambda: sw.across_members("ac", k0, k1))
  assert spans[0] == "k_series_windows" and "k_series_dfa" not in spans
  with pytest.raises(ValueError, match="unknown indicator 'dfa'"):
    sw.across_members("dfa", k0, k1)
  # with dfa
  sd = gpu.SeriesWindows(rec, WP, step=SP, dfa=SCALES)
  r, spans = spans_of(lambda: sd.compute(k0, k1))
  assert spans == ["k_series_windows", "k_series_dfa"]
  tr, spans = spans_of(lambda: sd.trend(k0, k1))
  assert spans == ["k_series_windows", "k_series_dfa"] + ["k_series_kendall"] * 3
  sig, spans = spans_of(lambda: sd.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=2 * per))
  assert spans == (["k_series_windows", "k_series_dfa"] + ["k_series_kendall"] * 3
                   + ["k_series_windows"]
                   + ["k_series_surrogates", "k_series_windows", "k_series_dfa"]
                   + ["k_series_kendall", "k_series_exceed"] * 3
                   + ["k_series_surrogates", "k_series_windows", "k_series_dfa"]
                   + ["k_series_kendall", "k_series_exceed"] * 3)
  assert hasattr(r, "dfa") and hasattr(tr, "dfa") and hasattr(sig, "dfa")
