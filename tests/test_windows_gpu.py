"""pm_series_windows, pm_series_kendall and SeriesWindows on the device: every case of
tests/windows_cases.py through the C-ABI bit for bit against the restatement, what the launches
leave alone, independence of a member from its neighbours and from the batch, the Kendall counts,
a recorded noise ensemble, and the launches of a run without SeriesWindows."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _collect, _out, _padded, _up
import windows_cases as WC

pytestmark = pytest.mark.gpu

def run(gpu, c, v=None, k0=None, k1=None):
  """One launch of the case's settings (on another series / record window if given) into
  sentinel-filled outputs; nothing behind an output's last element is touched."""
  from pymoc_amd import _lib
  v = c["v"] if v is None else v
  k0, k1 = (c["k0"], c["k1"]) if k0 is None else (k0, k1)
  nrec, nspec, n = v.shape
  nwin = WC.nwin_of(k1 - k0, c["W"], c["S"])
  series, v_ptr = _padded(gpu, v)
  shapes = dict(out=((4, nwin, nspec, n), np.float64, V_SENTINEL),
                nused=((nspec, n), np.int32, I_SENTINEL))
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  d = _lib.pm_series_windows()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, k0, k1
  d.window, d.step, d.lag, d.detrend = c["W"], c["S"], c["Lg"], WC.DETRENDS.index(c["detrend"])
  d.v, d.stt = v_ptr, WC.stt_of(c["W"])
  _lib.check(_lib.lib.pm_series_windows(C.byref(d), out["out"][0].ptr, out["nused"][0].ptr, None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


def run_kendall(gpu, v, k0, k1):
  from pymoc_amd import _lib
  nrec, nspec, n = v.shape
  series, v_ptr = _padded(gpu, v)
  keys = ("conc", "disc", "tie", "nfin")
  shapes = {k: ((nspec, n), np.int32, I_SENTINEL) for k in keys}
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  d = _lib.pm_series_kendall()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.v = n, nspec, nrec, k0, k1, v_ptr
  _lib.check(_lib.lib.pm_series_kendall(C.byref(d), *(out[k][0].ptr for k in keys), None))
  gpu.synchronize()
  res = _collect(out, shapes, "kendall")
  return tuple(res[k] for k in keys)


def _same(got, want, what):
  assert np.array_equal(got["nused"], want["nused"]), (what, "nused")
  _bits(got["out"], want["out"], (what, "out"))


CASES = WC.cases()
IDS = [c["name"] for c in CASES]
WIDE = [c for c in CASES if c["v"].shape[2] == 65]
KCASES = WC.kendall_cases()


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
def test_windows_bit_for_bit(gpu, results, case):
  c, got, want = case, results(case), WC.restate(case)
  _same(got, want, c["name"])
  assert np.array_equal(np.isnan(got["out"][0]), ~want["used"])
  # the styles did what they are for: some windows excluded, some members without any
  if c["v"].shape[1] * c["v"].shape[2] >= 9 and c["nwin"] > 1:  # (every style is there)
    nu = got["nused"]
    assert (nu == c["nwin"]).any() and (nu == c["nwin"] - 1).any() and (nu == 0).any()
  # the same records as a series of their own: the same bits
  own = run(gpu, c, v=np.ascontiguousarray(c["v"][c["k0"]:c["k1"]]), k0=0, k1=c["k1"] - c["k0"])
  _same(own, got, (c["name"], "own series"))


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_a_member_does_not_depend_on_its_neighbours_or_the_batch(gpu, results, case):
  c, whole = case, results(case)
  # the same series in every member: the same bits in every member
  v = np.repeat(c["v"][:, :, 6:7], 65, axis=2)  # (member 6: styles nan1, ar1, big)
  r = run(gpu, c, v=v)
  assert (r["nused"] == r["nused"][..., :1]).all(), c["name"]
  _bits(r["out"], np.repeat(r["out"][..., :1], 65, axis=-1), (c["name"], "copies"))
  for k in ("nused", "out"):
    _bits(r[k][..., 0], whole[k][..., 6], (c["name"], k, "member 6 among others"))
  # a member alone, and a shard: members [9, 41) as a series of their own
  for m0, m1 in ((6, 7), (9, 41)):
    part = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, m0:m1]))
    for k in ("nused", "out"):
      _bits(part[k], whole[k][..., m0:m1], (c["name"], k, "members [%d, %d)" % (m0, m1)))


@pytest.mark.parametrize("case", KCASES, ids=[c["name"] for c in KCASES])
def test_kendall_counts_are_exact(gpu, case):
  c = case
  got = run_kendall(gpu, c["v"], c["k0"], c["k1"])
  want = WC.kendall(c["v"], c["k0"], c["k1"])
  for g, w, key in zip(got, want, ("conc", "disc", "tie", "nfin")):
    assert np.array_equal(g, w), (c["name"], key)
  own = run_kendall(gpu, np.ascontiguousarray(c["v"][c["k0"]:c["k1"]]), 0, c["k1"] - c["k0"])
  for g, w in zip(own, got):
    assert np.array_equal(g, w), (c["name"], "own series")


def test_kendall_of_an_indicator_series(gpu, results):
  """The ac output of a window case -- 300 windows, NaN where a window is unused or has no
  variance -- as the series whose trend is counted."""
  c = next(c for c in CASES if c["nwin"] == WC.MANY)
  ac = np.ascontiguousarray(results(c)["out"][3])
  assert np.isnan(ac).any() and np.isfinite(ac).any()
  got = run_kendall(gpu, ac, 0, c["nwin"])
  want = WC.kendall(WC.restate(c)["out"][3], 0, c["nwin"])
  for g, w, key in zip(got, want, ("conc", "disc", "tie", "nfin")):
    assert np.array_equal(g, w), key
  part = run_kendall(gpu, ac, 7, 250)
  for g, w in zip(part, WC.kendall(ac, 7, 250)):
    assert np.array_equal(g, w)


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_windows_cpu as TC
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(4)]
  for label, kw in TC.bad_descriptors():
    d = TC.desc(**kw)
    assert _lib.lib.pm_series_windows(C.byref(d), out[0].ptr, out[1].ptr, None) == _lib.PM_EINVAL, label
  for label, kw in TC.bad_kendall_descriptors():
    d = TC.kdesc(**kw)
    assert _lib.lib.pm_series_kendall(C.byref(d), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                      None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ SeriesWindows
def _check_trend(tr, series, names, what):
  """A `Trend` against the restatement's counts of `series` [nwin, nspec, n]."""
  want = WC.kendall(series, 0, series.shape[0])
  for s, nm in enumerate(names):
    for key, w in zip(("conc", "disc", "tie", "nfin"), want):
      assert np.array_equal(getattr(tr, key)[nm], w[s]), (what, nm, key)
    assert np.array_equal(tr.tau[nm], WC.tau_b(want[0][s], want[1][s], want[2][s]), equal_nan=True)


def test_series_windows_on_a_plain_device_series(gpu):
  """(DeviceArray, names) as source: compute(), across_members against the restated indicator
  series through stats_cases.group_stats, trend and kendall against the restated counts."""
  import stats_cases as SC
  from pymoc_amd.windows import kendall
  c = next(c for c in CASES if c["W"] == 64 and c["S"] == 32)
  v, names = c["v"], ["wind", "amoc", "depth"]
  labels = np.array([40, -3, 7])[np.arange(65) % 3]
  sw = gpu.SeriesWindows((gpu.DeviceArray.from_host(v), names), 64, step=32, detrend=c["detrend"],
                         lag=c["Lg"], groups=labels)
  assert sw.nwin(c["k0"], c["k1"]) == c["nwin"]
  r, want = sw.compute(c["k0"], c["k1"]), WC.restate(c)
  assert r.record_end.tolist() == [c["k0"] + 63 + 32 * i for i in range(5)]
  assert np.array_equal(r.record_end, sw.record_end(c["k0"], c["k1"]))
  for s, nm in enumerate(names):
    assert np.array_equal(r.nused[nm], want["nused"][s])
    for i, key in enumerate(("mean", "slope", "var", "ac")):
      assert getattr(r, key)[nm].shape == (65, 5)
      _bits(getattr(r, key)[nm], want["out"][i, :, s, :].T, (nm, key))
  q = (0.05, 0.5, 0.95)
  order, start = SC.order_of(labels)
  for i, key in enumerate(("mean", "slope", "var", "ac")):
    across = sw.across_members(key, c["k0"], c["k1"], quantiles=q)
    assert sw.group_labels.tolist() == [-3, 7, 40]
    wc, ws = SC.group_stats(want["out"][i], order, start, q, 0, c["nwin"])
    for s, nm in enumerate(names):
      assert across.mean[nm].shape == (3, 5) and across.quantile[nm].shape == (3, 3, 5)
      assert np.array_equal(across.count[nm], wc[:, s, :].T), (key, nm)
      for j, stat in enumerate(("mean", "var", "min", "max", "sum")):
        _bits(getattr(across, stat)[nm], ws[:, s, :, j].T, (key, nm, stat))
      _bits(across.quantile[nm], ws[:, s, :, 5:].transpose(2, 1, 0), (key, nm, "quantile"))
    # members whose window is unused are excluded and counted
    assert (across.count["wind"] < np.bincount(np.searchsorted([-3, 7, 40], labels))[:, None]).any()
  tr = sw.trend(c["k0"], c["k1"])
  _check_trend(tr.var, want["out"][2], names, "var")
  _check_trend(tr.ac, want["out"][3], names, "ac")
  _check_trend(kendall((gpu.DeviceArray.from_host(v), names), c["k0"], c["k1"]),
               v[c["k0"]:c["k1"]], names, "kendall")


def test_series_windows_on_a_recorded_noise_ensemble(gpu):
  """An IndexRecorder on a 16-member JN2018Ensemble under NoiseForcing: the recorder route, the
  (array, names) route on its series and the restatement on the downloaded series agree bit for
  bit; the run issued no launch of this module before compute(), and each call adds its own."""
  import stats_cases as SC
  import test_stats_gpu as TG
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  before = [name for name, _, _ in ens.timer.spans]
  assert before.count("k_row_indices") == TG.N_SAMPLES
  assert not [name for name in before if "windows" in name or "kendall" in name or "series" in name]
  names = list(rec.table.names)
  sw = gpu.SeriesWindows(rec, 8, step=2, groups=TG.GROUPS)
  with pytest.raises(ValueError, match="record %d, which was never written" % TG.N_SAMPLES):
    sw.compute()
  r = sw.compute(2, TG.N_SAMPLES)
  spans = [name for name, _, _ in ens.timer.spans]
  assert spans[:len(before)] == before and spans[len(before):] == ["k_series_windows"]
  v = TG._series_of(rec)
  assert np.isfinite(v[:TG.N_SAMPLES]).all()
  want = WC.windows(v, 2, TG.N_SAMPLES, 8, 2, 1, "linear")
  nwin = (TG.N_SAMPLES - 2 - 8) // 2 + 1
  assert r.record_end.tolist() == [2 + 7 + 2 * i for i in range(nwin)]
  plain = gpu.SeriesWindows((gpu.DeviceArray.from_host(v), names), 8, step=2).compute(2, TG.N_SAMPLES)
  for s, nm in enumerate(names):
    assert (r.nused[nm] == nwin).all() and np.array_equal(plain.nused[nm], r.nused[nm])
    for i, key in enumerate(("mean", "slope", "var", "ac")):
      _bits(getattr(r, key)[nm], want["out"][i, :, s, :].T, (nm, key))
      _bits(getattr(plain, key)[nm], getattr(r, key)[nm], (nm, key, "plain"))
    assert (r.var[nm] > 0).all() and (np.abs(r.ac[nm]) <= 1).all()  # the noise acts
  order, start = SC.order_of(TG.GROUPS)
  across = sw.across_members("ac", 2, TG.N_SAMPLES, quantiles=(0.05, 0.95))
  wc, ws = SC.group_stats(want["out"][3], order, start, (0.05, 0.95), 0, nwin)
  for s, nm in enumerate(names):
    assert (across.count[nm] == 4).all() and across.mean[nm].shape == (4, nwin)
    _bits(across.mean[nm], ws[:, s, :, 0].T, (nm, "group mean"))
    _bits(across.quantile[nm], ws[:, s, :, 5:].transpose(2, 1, 0), (nm, "band"))
  tr = sw.trend(2, TG.N_SAMPLES)
  _check_trend(tr.var, want["out"][2], names, "var")
  _check_trend(tr.ac, want["out"][3], names, "ac")
  assert (tr.ac.nfin["amoc"] == nwin).all() and np.isfinite(tr.var.tau["amoc"]).all()
  spans = [name for name, _, _ in ens.timer.spans]
  assert spans[:len(before)] == before
  assert spans[len(before):] == ["k_series_windows"] * 3 + ["k_series_kendall"] * 2
