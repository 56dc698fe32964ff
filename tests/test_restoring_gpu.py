"""pm_series_restoring and SeriesWindows(restoring=...) on the device: every case of
tests/restoring_cases.py through the C-ABI -- lam and rho bit for bit against the restatement --
what the launch leaves alone, independence of a member from the batch and of a record window from
the series around it, the class against the restated composition on the device's lambda series,
and the launches of a SeriesWindows with and without `restoring`."""
import ctypes as C

import numpy as np
import pytest

from series_harness import V_SENTINEL, _bits, _collect, _out, _padded, _up
import restoring_cases as RC
import dfa_cases as DC
import surrogate_cases as SGC
import windows_cases as WC

pytestmark = pytest.mark.gpu


def run(gpu, c, v=None, k0=None, k1=None, with_rho=True):
  """One launch of the case's settings (on another series / record window if given) into
  sentinel-filled outputs; nothing behind an output's last element is touched."""
  from pymoc_amd import _lib
  v = c["v"] if v is None else v
  k0, k1 = (c["k0"], c["k1"]) if k0 is None else (k0, k1)
  nrec, nspec, n = v.shape
  nwin = WC.nwin_of(k1 - k0, c["W"], c["S"])
  series, v_ptr = _padded(gpu, v)
  shapes = dict(lam=((nwin, nspec, n), np.float64, V_SENTINEL))
  if with_rho:
    shapes["rho"] = ((nwin, nspec, n), np.float64, V_SENTINEL)
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  d = _lib.pm_series_restoring()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, k0, k1
  d.window, d.step, d.detrend = c["W"], c["S"], RC.DETRENDS.index(c["detrend"])
  d.v, d.stt, d.iters = v_ptr, RC.stt_of(c["W"]), c["iters"]
  _lib.check(_lib.lib.pm_series_restoring(C.byref(d), out["lam"][0].ptr,
                                          out["rho"][0].ptr if with_rho else None, None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


CASES = RC.cases()
IDS = [c["name"] for c in CASES]
WIDE = [c for c in CASES if c["v"].shape[2] == 37 and c["nwin"] < RC.MANY]


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
def test_lam_and_rho_bit_for_bit(gpu, results, case):
  """lam and rho equal the restatement bit for bit (the NaN pattern, signed zeros, the overflow
  of `huge`, the exact geometric decay); lam without rho stored and a copied-out record window
  give the same bits; pm_series_windows marks the same windows unused."""
  import test_windows_gpu as TW
  c, got, want = case, results(case), RC.restate(case)
  for k in ("lam", "rho"):
    _bits(got[k], want[k], (c["name"], k))
  assert np.isnan(got["lam"][~want["used"]]).all() and np.isnan(got["rho"][~want["used"]]).all()
  # lam alone: the same bits
  alone = run(gpu, c, with_rho=False)
  _bits(alone["lam"], got["lam"], (c["name"], "lam with rho = NULL"))
  # the same records as a series of their own: the same bits
  own = run(gpu, c, v=np.ascontiguousarray(c["v"][c["k0"]:c["k1"]]), k0=0, k1=c["k1"] - c["k0"])
  for k in ("lam", "rho"):
    _bits(own[k], got[k], (c["name"], k, "own series"))
  # pm_series_windows on the same series: the unused windows are the ones it marks
  wn = TW.run(gpu, dict(c, Lg=1))
  assert np.array_equal(np.isnan(wn["out"][0]), ~want["used"]), c["name"]
  assert np.array_equal(wn["nused"], want["used"].sum(axis=0)), c["name"]


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_a_member_does_not_depend_on_the_batch(gpu, results, case):
  """A shard (members 5 .. 20 of 37) and a single member give the bits they have in the batch."""
  c, whole = case, results(case)
  for m0, m1 in ((5, 21), (9, 10)):
    part = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, m0:m1]))
    for k in ("lam", "rho"):
      _bits(part[k], whole[k][..., m0:m1], (c["name"], k, "members [%d, %d)" % (m0, m1)))


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_restoring_cpu as TC
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(2)]
  for label, kw in TC.bad_descriptors():
    d = TC.desc(**kw)
    assert (_lib.lib.pm_series_restoring(C.byref(d), out[0].ptr, out[1].ptr, None)
            == _lib.PM_EINVAL), label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ SeriesWindows(restoring=...)
NSUR, KP, WP, SP, ITERS = 7, 120, 40, 4, 10
NAMES = ["wind", "amoc"]
NWIN = (KP - WP) // SP + 1


def _ensemble(n=5):
  """A restoring_cases series of 2 indices (every kind of member for n >= 13; AR(1), ramps,
  constants, a NaN in the first window for n = 5) with the record window [3, 3 + 120)."""
  c = RC.case(WP, SP, NWIN, n, 2, "linear", ITERS, 70 + n)
  assert c["k1"] - c["k0"] == KP + 3
  return c["v"], c["k0"], c["k0"] + KP


def _check_trend(tr, series, what):
  want = WC.kendall(series, 0, series.shape[0])
  for s, nm in enumerate(NAMES):
    for key, w in zip(("conc", "disc", "tie", "nfin"), want):
      assert np.array_equal(getattr(tr, key)[nm], w[s]), (what, nm, key)
    _bits(tr.tau[nm], WC.tau_b(want[0][s], want[1][s], want[2][s]), (what, nm, "tau"))


def _lam_series(r, names=None):
  """[nwin, nspec, n] from a `Windows`' lam [name] -> [n, nwin]."""
  return np.stack([r.lam[nm].T for nm in (names or r.names)], axis=1)


def _check_sig(sig, obs, sur_lam, what):
  """`sig` (a TrendSignificance) against the restated composition: Kendall of the observed lambda
  series [nwin, nspec, n], of the surrogates' [nwin, nsur * nspec, n], the exceedance counts and
  the p-values -- exactly."""
  nwin = obs.shape[0]
  counts = WC.kendall(obs, 0, nwin)
  acc = SGC.exceed(counts, WC.kendall(sur_lam, 0, nwin))
  want = DC.of_counts(counts, acc)
  for s, nm in enumerate(NAMES):
    for f in ("ge", "le", "nvalid"):
      assert np.array_equal(getattr(sig, f)[nm], want[f][s]), (what, nm, f)
    for f in ("tau", "p_rising", "p_falling"):
      _bits(getattr(sig, f)[nm], want[f][s], (what, nm, f))
  return want


def test_compute_across_members_and_trend(gpu):
  """compute() returns the C-ABI's bits in the documented shapes; across_members("lam") is
  SeriesStats of the device's lambda series; trend().lam its Kendall counts; the other indicators
  are what they are without restoring, with dfa next to it too."""
  import stats_cases as SC
  v, k0, k1 = _ensemble(37)
  n = 37
  labels = np.array([40, -3, 7])[np.arange(n) % 3]
  dev = gpu.DeviceArray.from_host(v)
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, restoring=True, groups=labels)
  plain = gpu.SeriesWindows((dev, NAMES), WP, step=SP, groups=labels)
  r, p = sw.compute(k0, k1), plain.compute(k0, k1)
  c = dict(v=v, k0=k0, k1=k1, W=WP, S=SP, detrend="linear", iters=ITERS, name="class")
  raw = run(gpu, c)
  want = RC.restate(c)
  for k in ("lam", "rho"):
    _bits(raw[k], want[k], k)
  assert np.isfinite(raw["lam"]).any() and np.isnan(raw["lam"]).any()
  for s, nm in enumerate(NAMES):
    assert r.lam[nm].shape == (n, NWIN) and r.lam_rho[nm].shape == (n, NWIN)
    _bits(r.lam[nm], raw["lam"][:, s, :].T, (nm, "lam"))
    _bits(r.lam_rho[nm], raw["rho"][:, s, :].T, (nm, "lam_rho"))
    for key in ("mean", "slope", "var", "ac"):
      _bits(getattr(r, key)[nm], getattr(p, key)[nm], (nm, key))
    assert np.array_equal(r.nused[nm], p.nused[nm])
  lam = _lam_series(r)
  _bits(lam, raw["lam"], "lam series")
  # an int: that many iterations; with dfa next to it both are what they are alone
  two = gpu.SeriesWindows((dev, NAMES), WP, step=SP, restoring=2, dfa=(4, 5)).compute(k0, k1)
  _bits(_lam_series(two), RC.restate(dict(c, iters=2))["lam"], "2 iterations")
  alone = gpu.SeriesWindows((dev, NAMES), WP, step=SP, dfa=(4, 5)).compute(k0, k1)
  for nm in NAMES:
    _bits(two.dfa[nm], alone.dfa[nm], (nm, "dfa"))
  q = (0.05, 0.5, 0.95)
  order, start = SC.order_of(labels)
  across = sw.across_members("lam", k0, k1, quantiles=q)
  assert sw.group_labels.tolist() == [-3, 7, 40]
  wc, ws = SC.group_stats(lam, order, start, q, 0, NWIN)
  for s, nm in enumerate(NAMES):
    assert across.mean[nm].shape == (3, NWIN) and across.quantile[nm].shape == (3, 3, NWIN)
    assert np.array_equal(across.count[nm], wc[:, s, :].T), nm
    for j, stat in enumerate(("mean", "var", "min", "max", "sum")):
      _bits(getattr(across, stat)[nm], ws[:, s, :, j].T, (nm, stat))
    _bits(across.quantile[nm], ws[:, s, :, 5:].transpose(2, 1, 0), (nm, "quantile"))
  tr, trp = sw.trend(k0, k1), plain.trend(k0, k1)
  _check_trend(tr.lam, lam, "lam")
  for key in ("var", "ac"):
    for nm in NAMES:
      assert np.array_equal(getattr(tr, key).conc[nm], getattr(trp, key).conc[nm])
  assert (tr.lam.nfin["wind"] == NWIN).any() and (tr.lam.nfin["wind"] < NWIN).any()


SIG = [("linear", "ar1"), ("linear", "fourier"), ("gaussian", "ar1"), ("gaussian", "fourier")]


@pytest.mark.parametrize("detrend,method", SIG, ids=["%s %s" % p for p in SIG])
def test_significance_equals_the_restated_composition(gpu, detrend, method):
  """significance().lam: counts, taus and p-values equal the restated Kendall + exceedance
  composition on the device's lambda series -- the record's from compute(), the surrogates' from
  SeriesWindows(restoring=...) on the series SeriesSurrogates.generate gives for the same
  arguments -- exactly, whole and with max_bytes forcing chunks of 3 + 3 + 1 surrogates; var and
  ac are what they are without restoring."""
  v, k0, k1 = _ensemble(5)
  dev = gpu.DeviceArray.from_host(v)
  kw = dict(sigma=5.0) if detrend == "gaussian" else {}
  seed, member0 = 2**63 + 7, 2**32 - 2
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, detrend=detrend, restoring=True, **kw)
  plain = gpu.SeriesWindows((dev, NAMES), WP, step=SP, detrend=detrend, **kw)
  obs = _lam_series(sw.compute(k0, k1))
  gen = gpu.SeriesSurrogates((dev, NAMES), detrend=detrend, seed=seed, member0=member0,
                             method=method, **kw)
  y, ynames = gen.generate(k0, k1, 0, NSUR)
  sub = gpu.SeriesWindows((y, ynames), WP, step=SP, detrend=detrend, restoring=True,
                          **kw).compute()
  sur_lam = _lam_series(sub, ynames)
  assert sur_lam.shape == (NWIN, NSUR * 2, 5) and np.isfinite(sur_lam).any()
  per = 16 * KP * 2 * 5 if detrend == "gaussian" else 8 * KP * 2 * 5
  ref = plain.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, method=method)
  for max_bytes in (2 << 30, 3 * per):
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes,
                          method=method)
    want = _check_sig(sig.lam, obs, sur_lam, (detrend, method, max_bytes))
    for key in ("var", "ac"):
      for nm in NAMES:
        for f in ("ge", "le", "nvalid"):
          assert np.array_equal(getattr(getattr(sig, key), f)[nm], getattr(getattr(ref, key), f)[nm])
  assert sig.nsur == NSUR and (want["nvalid"] == NSUR).any() and (want["nvalid"] == 0).any()
  tr = sw.trend(k0, k1)
  for nm in NAMES:
    _bits(sig.lam.tau[nm], tr.lam.tau[nm], (nm, "trend()"))


def _shifting():
  """test_shifts_gpu._ensemble at 120 records: 2 indices x 5 members x (3 + 120 + 2) records:
  member 0 drops at record 50, 1 at 90, 2 never (noise), 3 holds a NaN before its drop at 75, 4 is
  constant; "wind" rises where "amoc" drops."""
  rng = np.random.default_rng(9400)
  v = np.empty((3 + KP + 2, 2, 5))
  a = rng.standard_normal((2, 5))
  for k in range(v.shape[0]):
    a = 0.6 * a + 0.8 * rng.standard_normal((2, 5))
    v[k] = a
  v[3 + 50:, 1, 0] -= 9.0
  v[3 + 90:, 1, 1] -= 9.0
  v[3 + 75:, 1, 3] -= 9.0
  v[3 + 20, 1, 3] = np.nan
  v[:, 1, 4] = 2.5
  v[3 + 65:, 0, :3] += 9.0
  v[:3], v[3 + KP:] = 7e30, -3e30
  return v, 3, 3 + KP


def test_significance_until(gpu):
  """significance(until=).lam, linear detrending: the record censored at the amoc's first
  detectable record, the surrogates of the ranged fit censored where the record is; the restated
  composition on the device's lambda series of both, exactly."""
  import shifts_cases as SHC
  import test_shifts_gpu as TS
  from pymoc_amd.shifts import launch_fit_ranged
  v, k0, k1 = _shifting()
  K = k1 - k0
  nspec, n = v.shape[1:]
  dev = gpu.DeviceArray.from_host(v)
  sh = gpu.SeriesShifts((dev, NAMES), TS.LP, direction=dict(wind=1, amoc=-1), threshold=5.0)
  sh.detect(k0, k1)
  y, _ = sh.censored(by="amoc")
  end = sh.end.download()
  assert (end < K).any() and (end == K).any()
  seed, member0 = 2**63 + 5, 2**32 - 2
  W_, S_ = WP, SP
  sw = gpu.SeriesWindows((dev, NAMES), W_, step=S_, restoring=True)
  obs = _lam_series(gpu.SeriesWindows((y, NAMES), W_, step=S_, restoring=True).compute())
  fit = launch_fit_ranged(y, (K, nspec, n), 0, K, "linear", sh.end, None, None)
  gen = gpu.SeriesSurrogates((dev, NAMES), detrend="linear", seed=seed, member0=member0)
  ysur = gpu.DeviceArray((K, NSUR * nspec, n), np.float64)
  gen._launch(fit, K, 0, NSUR, ysur)
  cut = SHC.censor(ysur.download(), np.where(end >= K, -1, end), nb=NSUR)[0]
  ynames = gen.names_of(0, NSUR)
  sub = gpu.SeriesWindows((gpu.DeviceArray.from_host(cut), ynames), W_, step=S_,
                          restoring=True).compute()
  sur_lam = _lam_series(sub, ynames)
  sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, until=sh)
  want = _check_sig(sig.lam, obs, sur_lam, "until")
  assert (want["nvalid"] == NSUR).any()
  whole = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0)
  assert not np.array_equal(whole.lam.tau["amoc"], sig.lam.tau["amoc"], equal_nan=True)


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


def test_the_launches_with_and_without_restoring(gpu):
  """restoring=None: the span names of compute, trend and significance are the lists of the
  commit before this indicator, written out here (with and without dfa), and no result has a `lam`
  attribute; with restoring the restoring launch follows the window (and the DFA) launch, and
  every trend gains one Kendall (and exceedance) launch, last."""
  from pymoc_amd.device import LaunchTimer
  v, k0, k1 = _ensemble(5)
  per = 8 * KP * 2 * 5
  timer = LaunchTimer()
  rec = _Recorder(gpu.DeviceArray.from_host(v), timer)

  def spans_of(call):
    before = len(timer.spans)
    res = call()
    return res, [name for name, _, _ in timer.spans[before:]]

  KE = ["k_series_kendall", "k_series_exceed"]
  sw = gpu.SeriesWindows(rec, WP, step=SP)
  r, spans = spans_of(lambda: sw.compute(k0, k1))
  assert spans == ["k_series_windows"]
  assert not [a for a in vars(r) if "lam" in a]
  tr, spans = spans_of(lambda: sw.trend(k0, k1))
  assert spans == ["k_series_windows", "k_series_kendall", "k_series_kendall"]
  assert not hasattr(tr, "lam")
  sig, spans = spans_of(lambda: sw.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=3 * per))
  assert spans == (["k_series_windows", "k_series_kendall", "k_series_kendall", "k_series_windows"]
                   + (["k_series_surrogates", "k_series_windows"] + KE * 2) * 3)
  assert not hasattr(sig, "lam")
  _, spans = spans_of(lambda: sw.across_members("ac", k0, k1))
  assert spans[0] == "k_series_windows" and "k_series_restoring" not in spans
  with pytest.raises(ValueError, match="unknown indicator 'lam'"):
    sw.across_members("lam", k0, k1)
  # dfa alone: as before
  sd = gpu.SeriesWindows(rec, WP, step=SP, dfa=(4, 5))
  sig, spans = spans_of(lambda: sd.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=3 * per))
  assert spans == (["k_series_windows", "k_series_dfa"] + ["k_series_kendall"] * 3
                   + ["k_series_windows"]
                   + (["k_series_surrogates", "k_series_windows", "k_series_dfa"] + KE * 3) * 3)
  assert hasattr(sig, "dfa") and not hasattr(sig, "lam")
  # with restoring
  sr = gpu.SeriesWindows(rec, WP, step=SP, restoring=True)
  r, spans = spans_of(lambda: sr.compute(k0, k1))
  assert spans == ["k_series_windows", "k_series_restoring"]
  tr, spans = spans_of(lambda: sr.trend(k0, k1))
  assert spans == ["k_series_windows", "k_series_restoring"] + ["k_series_kendall"] * 3
  sig, spans = spans_of(lambda: sr.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=3 * per))
  assert spans == (["k_series_windows", "k_series_restoring"] + ["k_series_kendall"] * 3
                   + ["k_series_windows"]
                   + (["k_series_surrogates", "k_series_windows", "k_series_restoring"] + KE * 3) * 3)
  assert hasattr(r, "lam") and hasattr(tr, "lam") and hasattr(sig, "lam")
  assert not hasattr(sig, "dfa")
  _, spans = spans_of(lambda: sr.across_members("lam", k0, k1))
  assert spans[:2] == ["k_series_windows", "k_series_restoring"]
  # with both: dfa, then restoring
  sb = gpu.SeriesWindows(rec, WP, step=SP, dfa=(4, 5), restoring=3)
  tr, spans = spans_of(lambda: sb.trend(k0, k1))
  assert spans == (["k_series_windows", "k_series_dfa", "k_series_restoring"]
                   + ["k_series_kendall"] * 4)
  sig, spans = spans_of(lambda: sb.significance(k0, k1, nsur=NSUR, seed=3, max_bytes=3 * per))
  assert spans == (["k_series_windows", "k_series_dfa", "k_series_restoring"]
                   + ["k_series_kendall"] * 4 + ["k_series_windows"]
                   + (["k_series_surrogates", "k_series_windows", "k_series_dfa",
                       "k_series_restoring"] + KE * 4) * 3)
  assert hasattr(tr, "dfa") and hasattr(tr, "lam") and hasattr(sig, "dfa") and hasattr(sig, "lam")
  for nm in NAMES:
    _bits(sig.dfa.tau[nm], tr.dfa.tau[nm], (nm, "dfa tau"))
    _bits(sig.lam.tau[nm], tr.lam.tau[nm], (nm, "lam tau"))
