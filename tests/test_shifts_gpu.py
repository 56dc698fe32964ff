"""pm_series_shift_scan, pm_series_censor, pm_series_fit_ranged, SeriesShifts and
SeriesWindows.significance(until=) on the device: every double bit for bit and every integer exact
against the restatement (tests/shifts_cases.py), what the launches leave alone, independence of a
member from the batch, the ranged fit against the existing window kernel, the whole composition
exactly on the device's surrogate series, and that nothing changes without `until`."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _collect, _out, _padded, _up
import shifts_cases as SHC
import smooth_cases as SMC
import surrogate_cases as SGC
import windows_cases as WC

pytestmark = pytest.mark.gpu

CASES = SHC.cases()
IDS = [c["name"] for c in CASES]


def _scan_shapes(nspec, n):
  return dict(at=((nspec, n), np.int32, I_SENTINEL), first=((nspec, n), np.int32, I_SENTINEL),
              ncand=((nspec, n), np.int32, I_SENTINEL), val=((4, nspec, n), np.float64, V_SENTINEL))


def run_scan(gpu, mean_ptr, var_ptr, c, n=None, **kw):
  """One launch of the scan on two device planes: dict(at, first, ncand, val)."""
  from pymoc_amd import _lib
  n = c["n"] if n is None else n
  nspec = c["nspec"]
  thr = np.ascontiguousarray(kw.get("thr", c["thr"]), dtype=np.float64)
  dirs = np.ascontiguousarray(kw.get("dir", c["dir"]), dtype=np.int32)
  dthr, ddir = _up(gpu, thr), _up(gpu, dirs)
  shapes = _scan_shapes(nspec, n)
  out = {k: _out(gpu, *shapes[k]) for k in shapes}
  d = _lib.pm_series_shift_scan()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.half = n, nspec, c["v"].shape[0], c["k0"], c["k1"], c["L"]
  d.mean, d.var = mean_ptr, var_ptr
  d.thr, d.thr_dev, d.dir, d.dir_dev = thr.ctypes.data, dthr.ptr, dirs.ctypes.data, ddir.ptr
  _lib.check(_lib.lib.pm_series_shift_scan(C.byref(d), out["at"][0].ptr, out["first"][0].ptr,
                                           out["ncand"][0].ptr, out["val"][0].ptr, None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


def device_planes(gpu, v, k0, k1, L):
  """pm_series_windows (window L, step 1, "constant", lag 1) on the padded series: (the output
  array [4, nwin, nspec, n], nwin)."""
  from pymoc_amd import _lib
  nrec, nspec, n = v.shape
  nwin = k1 - k0 - L + 1
  dev, ptr = _padded(gpu, v)
  out = gpu.DeviceArray((4, nwin, nspec, n), np.float64)
  nused = gpu.DeviceArray((nspec, n), np.int32)
  d = _lib.pm_series_windows()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, k0, k1
  d.window, d.step, d.lag, d.detrend = L, 1, 1, _lib.PM_WIN_DETREND_CONSTANT
  d.v, d.stt = ptr, SHC.stt_of(L)
  _lib.check(_lib.lib.pm_series_windows(C.byref(d), out.ptr, nused.ptr, None))
  gpu.synchronize()
  return out, nwin


def _same_scan(got, want, what):
  for key in ("at", "first", "ncand"):
    assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key)
  _bits(got["val"], want["val"], (what, "val"))


@pytest.fixture(scope="module")
def restated():
  """name -> (mean, var, the restated scan): computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      mean, var = SHC.planes(c["v"], c["k0"], c["k1"], c["L"])
      cache[c["name"]] = (mean, var, SHC.scan(mean, var, c["L"], c["thr"], c["dir"]))
    return cache[c["name"]]
  return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scan_on_uploaded_planes_and_end_to_end(gpu, restated, case):
  c = case
  mean, var, want = restated(c)
  pm, pv = _padded(gpu, mean), _padded(gpu, var)
  _same_scan(run_scan(gpu, pm[1], pv[1], c), want, (c["name"], "uploaded planes"))
  out, nwin = device_planes(gpu, c["v"], c["k0"], c["k1"], c["L"])
  size = 8 * nwin * c["nspec"] * c["n"]
  _same_scan(run_scan(gpu, out.ptr, out.ptr + 2 * size, c), want, (c["name"], "end to end"))
  if c["n"] > 1:  # every kind of result is in the case
    assert (want["at"] == -1).any() and (want["at"] >= c["L"]).any()


def test_scan_every_direction_and_threshold(gpu, restated):
  """Every index under every dir, with a threshold reached, not reached and NaN; infinite scores
  and ties of zeros among the members."""
  c = next(k for k in CASES if (k["K"], k["L"]) == (300, 40))
  mean, var, _ = restated(c)
  pm, pv = _padded(gpu, mean), _padded(gpu, var)
  infinite = False
  for dirs in ((-1, -1, -1), (0, 0, 0), (1, 1, 1), (1, -1, 0)):
    for thr in ((3.0, 3.0, 3.0), (1e9, np.nan, -1e9), (0.0, -0.0, np.nan)):
      want = SHC.scan(mean, var, c["L"], thr, dirs)
      _same_scan(run_scan(gpu, pm[1], pv[1], c, thr=thr, dir=dirs), want, (dirs, thr))
      if thr[0] == 1e9:  # reached by an infinite score alone, none, reached by whatever counts
        assert np.array_equal(want["first"][0] >= 0, (want["score"][:, 0] == np.inf).any(axis=0))
        assert (want["first"][1] == -1).all()
        assert np.array_equal(want["first"][2] >= 0, want["ncand"][2] > 0)
      infinite |= bool(np.isinf(want["val"][0]).any())
  assert infinite


def test_scan_on_wide_planes_of_the_largest_half_width(gpu):
  """K = 4096, L = 2048 at n = 65, nspec = 3 on drawn planes (the restated windows of such a
  series would take minutes; the scan reads planes, whatever wrote them): NaN means, zero and
  infinite variances, equal scores."""
  rng = np.random.default_rng(9100)
  K, L, n, nspec = 4096, 2048, 65, 3
  nwin = K - L + 1
  mean = np.round(rng.standard_normal((nwin, nspec, n)) * 4.0) / 4.0  # (quarters: equal scores)
  var = rng.choice([0.0, 0.25, 1.0, 4.0, np.inf, np.nan], size=(nwin, nspec, n),
                   p=[0.1, 0.3, 0.3, 0.2, 0.05, 0.05])
  mean[rng.random(mean.shape) < 0.1] = np.nan
  mean[:, 1, 3] = np.nan
  c = dict(name="drawn planes", v=np.empty((K + 5, 1, 1)), k0=2, k1=K + 2, K=K, L=L, n=n,
           nspec=nspec, thr=np.array([2.0, np.nan, 1e9]), dir=np.array([-1, 0, 1], dtype=np.int32))
  want = SHC.scan(mean, var, L, c["thr"], c["dir"])
  assert want["at"][1, 3] == -1 and (want["ncand"] > 0).any()
  pm, pv = _padded(gpu, mean), _padded(gpu, var)
  _same_scan(run_scan(gpu, pm[1], pv[1], c), want, "drawn planes")


def test_scan_of_a_shard_or_a_single_member(gpu, restated):
  c = next(k for k in CASES if (k["K"], k["L"], k["n"]) == (9, 4, 130))
  mean, var, want = restated(c)
  for lo, hi in ((0, 1), (37, 38), (31, 97), (129, 130)):
    pm = _padded(gpu, np.ascontiguousarray(mean[:, :, lo:hi]))
    pv = _padded(gpu, np.ascontiguousarray(var[:, :, lo:hi]))
    got = run_scan(gpu, pm[1], pv[1], c, n=hi - lo)
    _same_scan(got, {k: want[k][..., lo:hi] for k in ("at", "first", "ncand", "val")}, (lo, hi))


# ------------------------------------------------------------------ pm_series_censor
def run_censor(gpu, c, guard=0, src=None, in_place=False, with_end=True, x=None, where=None):
  """One launch: (y [K, nb * nspec, n], end [nspec, n] or None)."""
  from pymoc_amd import _lib
  x = c["x"] if x is None else x
  where = c["where"] if where is None else where
  K, planes, n = x.shape
  nspec, nb = c["nspec"], c["nb"]
  src = np.arange(nspec, dtype=np.int32) if src is None else np.asarray(src, dtype=np.int32)
  dsrc, dwhere = _up(gpu, src), _up(gpu, np.ascontiguousarray(where, dtype=np.int32))
  xdev, xptr = _padded(gpu, x)
  shapes = dict(y=((K, planes, n), np.float64, V_SENTINEL), end=((nspec, n), np.int32, I_SENTINEL))
  out = {k: _out(gpu, *shapes[k]) for k in shapes}
  d = _lib.pm_series_censor()
  d.n, d.nspec, d.K, d.nb, d.guard = n, nspec, K, nb, guard
  d.x, d.where, d.src, d.src_dev = xptr, dwhere.ptr, src.ctypes.data, dsrc.ptr
  yptr = xptr if in_place else out["y"][0].ptr
  _lib.check(_lib.lib.pm_series_censor(C.byref(d), yptr, out["end"][0].ptr if with_end else None,
                                       None))
  gpu.synchronize()
  res = _collect(out, shapes, "censor")
  if in_place:
    from series_harness import PAD
    flat = xdev.download()
    assert (res["y"] == V_SENTINEL).all()
    pad = np.full(PAD, np.nan)
    pad[0:PAD:2] = 7e30
    assert np.array_equal(flat[:PAD], pad, equal_nan=True), "before the series"
    assert np.array_equal(np.isnan(flat[PAD + x.size:]), np.arange(PAD) % 2 == 1), "behind it"
    res["y"] = flat[PAD:PAD + x.size].reshape(x.shape)
  if not with_end:
    assert (res["end"] == I_SENTINEL).all()
  return res["y"], (res["end"] if with_end else None)


def _same_bits(got, want, what):
  assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


CENSORS = [(12, 7, 2, 3), (37, 65, 3, 1), (5, 130, 1, 3), (300, 63, 2, 2)]


@pytest.mark.parametrize("K,n,nspec,nb", CENSORS, ids=["K %d n %d nspec %d nb %d" % p for p in CENSORS])
def test_censor_bit_for_bit(gpu, K, n, nspec, nb):
  c = SHC.censor_case(K, n, nspec, nb, K)
  payload = (c["x"].view(np.uint64) == 0x7ff8dead0000beef)
  assert payload.any()
  rot = (np.arange(nspec) + 1) % nspec
  for guard, src in ((0, None), (2, None), (10**6, None), (1, rot)):
    want, wend = SHC.censor(c["x"], c["where"], guard, src, nb)
    for in_place in (False, True):
      for with_end in (True, False):
        y, end = run_censor(gpu, c, guard, src, in_place, with_end)
        _same_bits(y, want, (guard, in_place, with_end))  # payloads and all
        if with_end:
          assert np.array_equal(end, wend), (guard, in_place)
    if guard == 10**6:  # beyond every `where`: nothing is kept but the members without a shift
      assert np.isnan(want[:, :, np.nonzero((c["where"] >= 0).all(axis=0))[0]]).all()
  # where = -1 throughout: the bits are untouched
  none = np.full((nspec, n), -1, dtype=np.int32)
  for in_place in (False, True):
    y, end = run_censor(gpu, c, 3, None, in_place, True, where=none)
    _same_bits(y, c["x"], ("where -1", in_place))
    assert (end == K).all()
  # a shard or a single member gives the bits it has in the batch
  want, wend = SHC.censor(c["x"], c["where"], 1, None, nb)
  for lo, hi in ((0, 1), (n // 2, n // 2 + 1), (n // 3, n)):
    y, end = run_censor(gpu, c, 1, x=np.ascontiguousarray(c["x"][:, :, lo:hi]),
                        where=np.ascontiguousarray(c["where"][:, lo:hi]))
    _same_bits(y, want[:, :, lo:hi], (lo, hi))
    assert np.array_equal(end, wend[:, lo:hi])


# ------------------------------------------------------------------ pm_series_fit_ranged
def run_fit(gpu, v, k0, k1, end, detrend, tab=None):
  from pymoc_amd import _lib
  nrec, nspec, n = v.shape
  K = k1 - k0
  tab = np.array([SHC.stt_of(W) for W in range(K + 1)]) if tab is None else tab
  dtab, dend = _up(gpu, tab), _up(gpu, np.ascontiguousarray(end, dtype=np.int32))
  vdev, vptr = _padded(gpu, v)
  shapes = dict(var=((nspec, n), np.float64, V_SENTINEL), ac=((nspec, n), np.float64, V_SENTINEL))
  out = {k: _out(gpu, *shapes[k]) for k in shapes}
  d = _lib.pm_series_fit_ranged()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.detrend = n, nspec, nrec, k0, k1, WC.DETRENDS.index(detrend)
  d.v, d.end, d.stt_tab, d.stt_tab_dev = vptr, dend.ptr, tab.ctypes.data, dtab.ptr
  _lib.check(_lib.lib.pm_series_fit_ranged(C.byref(d), out["var"][0].ptr, out["ac"][0].ptr, None))
  gpu.synchronize()
  return _collect(out, shapes, "fit")


FITS = [(40, 9, 2), (22, 65, 3), (300, 130, 1), (64, 1, 1)]


@pytest.mark.parametrize("detrend", WC.DETRENDS)
@pytest.mark.parametrize("K,n,nspec", FITS, ids=["K %d n %d nspec %d" % p for p in FITS])
def test_ranged_fit_is_the_restatement_and_the_window_kernel(gpu, K, n, nspec, detrend):
  """Ends 0, 3, 4, K and between, mixed across the members, with interior NaNs: bit-identical to
  the restatement, and per distinct end e to the EXISTING pm_series_windows run with one window
  over [k0, k0 + e)."""
  from pymoc_amd import _lib
  c = SHC.fit_case(K, n, nspec, K)
  v, k0, k1, end = c["v"], c["k0"], c["k1"], c["end"]
  got = run_fit(gpu, v, k0, k1, end, detrend)
  var, ac = SHC.fit_ranged(v, k0, k1, end, detrend)
  _bits(got["var"], var, (detrend, "var"))
  _bits(got["ac"], ac, (detrend, "ac"))
  assert np.isnan(var[(end < 4)]).all() and (np.isfinite(var).any() or n == 1)
  if n >= 3 and K >= 13:
    assert np.isnan(var[0, 1]) and np.isfinite(var[0, 2])
  dev = gpu.DeviceArray.from_host(v)
  for e in np.unique(end):
    if e < 4:
      continue
    out = gpu.DeviceArray((4, 1, nspec, n), np.float64)
    nused = gpu.DeviceArray((nspec, n), np.int32)
    d = _lib.pm_series_windows()
    d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, v.shape[0], k0, k0 + int(e)
    d.window, d.step, d.lag, d.detrend = int(e), 1, 1, WC.DETRENDS.index(detrend)
    d.v, d.stt = dev.ptr, SHC.stt_of(int(e))
    _lib.check(_lib.lib.pm_series_windows(C.byref(d), out.ptr, nused.ptr, None))
    gpu.synchronize()
    w = out.download()
    sel = end == e
    _bits(got["var"][sel], w[2, 0][sel], (detrend, int(e), "var against the window kernel"))
    _bits(got["ac"][sel], w[3, 0][sel], (detrend, int(e), "ac against the window kernel"))
  # a shard or a single member gives the bits it has in the batch
  for lo, hi in ((0, 1), (n - 1, n), (n // 3, n)):
    part = run_fit(gpu, np.ascontiguousarray(v[:, :, lo:hi]), k0, k1, end[:, lo:hi], detrend)
    _bits(part["var"], got["var"][:, lo:hi], (detrend, lo, hi))
    _bits(part["ac"], got["ac"][:, lo:hi], (detrend, lo, hi))
  # an end beyond the record window is no fit, and reads nothing
  over = run_fit(gpu, v, k0, k1, np.full_like(end, K + 1), detrend)
  assert np.isnan(over["var"]).all() and np.isnan(over["ac"]).all()


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_shifts_cpu as TC
  ints = [_up(gpu, np.full(4096, I_SENTINEL, dtype=np.int32)) for _ in range(3)]
  vals = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(2)]
  cases, keep = TC.bad_scans()
  for label, kw in cases:
    d = TC.sdesc(**kw)
    assert _lib.lib.pm_series_shift_scan(C.byref(d), ints[0].ptr, ints[1].ptr, ints[2].ptr,
                                         vals[0].ptr, None) == _lib.PM_EINVAL, label
  cases, keep = TC.bad_censors()
  for label, kw in cases:
    d = TC.cdesc(**kw)
    assert _lib.lib.pm_series_censor(C.byref(d), vals[0].ptr, ints[0].ptr, None) == _lib.PM_EINVAL, label
  cases, keep = TC.bad_fits()
  for label, kw in cases:
    d = TC.fdesc(**kw)
    assert _lib.lib.pm_series_fit_ranged(C.byref(d), vals[0].ptr, vals[1].ptr, None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in ints:
    assert (a.download() == I_SENTINEL).all()
  for a in vals:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ the classes and the composition
NSUR, KP, WP, SP, LP = 7, 96, 16, 4, 8
NAMES = ["wind", "amoc"]


def _ensemble():
  """2 indices x 5 members x (3 + 96 + 2) records: member 0 drops early, 1 late, 2 never (noise),
  3 holds a NaN before its drop, 4 is constant; "wind" rises where "amoc" drops."""
  rng = np.random.default_rng(9300)
  v = np.empty((3 + KP + 2, 2, 5))
  a = rng.standard_normal((2, 5))
  for k in range(v.shape[0]):
    a = 0.6 * a + 0.8 * rng.standard_normal((2, 5))
    v[k] = a
  v[3 + 40:, 1, 0] -= 9.0
  v[3 + 70:, 1, 1] -= 9.0
  v[3 + 60:, 1, 3] -= 9.0
  v[3 + 20, 1, 3] = np.nan
  v[:, 1, 4] = 2.5
  v[3 + 55:, 0, :3] += 9.0
  v[:3], v[3 + KP:] = 7e30, -3e30
  return v, 3, 3 + KP


def _same_sig(sig, want, what):
  for key in ("var", "ac"):
    r, w = getattr(sig, key), want[key]
    for s, nm in enumerate(NAMES):
      for f in ("ge", "le", "nvalid"):
        assert np.array_equal(getattr(r, f)[nm], w[f][s]), what + (key, nm, f)
      for f in ("tau", "p_rising", "p_falling"):
        _bits(getattr(r, f)[nm], w[f][s], what + (key, nm, f))


@pytest.mark.parametrize("detrend", ["linear", "gaussian"])
def test_detect_censored_and_significance_until_equal_the_restated_composition(gpu, detrend):
  """detect, censored and significance(until=) against shifts_cases on the device's own surrogate
  series: the integers and the counts exactly, every double bit for bit; chunks of 3 and all."""
  from pymoc_amd.shifts import launch_fit_ranged
  v, k0, k1 = _ensemble()
  dev = gpu.DeviceArray.from_host(v)
  dirs, thr = dict(wind=1, amoc=-1), 5.0
  sh = gpu.SeriesShifts((dev, NAMES), LP, direction=dirs, threshold=thr)
  found = sh.detect(k0, k1)
  want = SHC.detect(v, k0, k1, LP, [thr, thr], [1, -1])
  for s, nm in enumerate(NAMES):
    for key in ("at", "first", "ncand"):
      assert np.array_equal(getattr(found, key)[nm], want[key][s]), (nm, key)
    assert np.array_equal(found.record[nm], np.where(want["at"][s] < 0, -1, k0 + want["at"][s]))
    for i, key in enumerate(("stat", "jump", "before", "after")):
      _bits(getattr(found, key)[nm], want["val"][i, s], (nm, key))
  assert want["first"][1].tolist()[2] == -1 and want["at"][1, 4] == -1
  assert (want["first"][1, [0, 1]] > 0).all() and want["ncand"][1, 3] < KP - 2 * LP + 1
  # censored: by its own index, and all by the amoc
  for kw, src in ((dict(), None), (dict(where="at", guard=2), None), (dict(by="amoc"), [1, 1])):
    y, names = sh.censored(**kw)
    wy, wend = SHC.censor(v[k0:k1], want[kw.get("where", "first")], kw.get("guard", 0), src)
    assert names == NAMES and y.shape == (KP, 2, 5)
    assert np.array_equal(y.download().view(np.uint64), wy.view(np.uint64)), kw
    assert np.array_equal(sh.end.download(), wend)
    assert np.array_equal(sh.end()["amoc"], wend[1])
  # the significance, up to the amoc's first detectable record
  y, _ = sh.censored(by="amoc")
  end = sh.end.download()
  assert sorted(set(end[1].tolist())) != [KP] and (end == KP).any()
  kw = dict(sigma=5.0) if detrend == "gaussian" else {}
  sw = gpu.SeriesWindows((dev, NAMES), WP, step=SP, detrend=detrend, **kw)
  seed, member0 = 2**63 + 5, 2**32 - 2
  # the device's fit and its surrogates, from the censored series as significance forms them
  cens = v[k0:k1].copy()
  cens = SHC.censor(cens, np.where(end >= KP, -1, end))[0]
  inner = "constant" if detrend == "gaussian" else detrend
  series = SMC.smooth(cens, 0, KP, SMC.weights(5.0))["resid"] if detrend == "gaussian" else cens
  fit = launch_fit_ranged(gpu.DeviceArray.from_host(series), (KP, 2, 5), 0, KP, inner, sh.end, None, None)
  wfit = SHC.fit_ranged(series, 0, KP, end, inner)
  fitted = fit[0]._parent.download()
  _bits(fitted[0, 0], wfit[0], "var of the ranged fit")
  _bits(fitted[1, 0], wfit[1], "ac of the ranged fit")
  gen = gpu.SeriesSurrogates((dev, NAMES), detrend=inner, seed=seed, member0=member0)
  ysur = gpu.DeviceArray((KP, NSUR * 2, 5), np.float64)
  gen._launch(fit, KP, 0, NSUR, ysur)
  sur = ysur.download()
  want_sig = SHC.significance(v, k0, k1, WP, SP, 1, detrend, NSUR, end, sur=sur, sigma=5.0)
  per = (16 if detrend == "gaussian" else 8) * KP * 2 * 5
  for max_bytes in (3 * per, 2 << 30):
    sig = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0, max_bytes=max_bytes, until=sh)
    _same_sig(sig, want_sig, (detrend, max_bytes))
  nv = np.stack([sig.ac.nvalid[nm] for nm in NAMES])
  assert (nv == NSUR).any() and (nv == 0).any()
  # the observed taus are trend() of the censored source
  tr = gpu.SeriesWindows((y, NAMES), WP, step=SP, detrend=detrend, **kw).trend()
  for nm in NAMES:
    _bits(sig.var.tau[nm], tr.var.tau[nm], (nm, "trend of the censored source"))
  # and the plain test of the same record window differs: it sees the drop
  plain = sw.significance(k0, k1, nsur=NSUR, seed=seed, member0=member0)
  assert not np.array_equal(plain.var.tau["amoc"], sig.var.tau["amoc"], equal_nan=True)


def test_without_until_nothing_changes(gpu):
  """The launch spans and every result of significance() without `until` are what they were (the
  restatement of surrogate_cases on the surrogates of the one-window fit); with `until` the three
  new spans appear where windows.py says; a censored source with no shift anywhere gives trend()
  bitwise that of the uncensored one."""
  import test_stats_gpu as TG
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  names = list(rec.table.names)
  k0, k1 = 2, TG.N_SAMPLES
  sw = gpu.SeriesWindows(rec, 8, step=2)
  before = len(ens.timer.spans)
  sig = sw.significance(k0, k1, nsur=5, seed=99, max_bytes=8 * (k1 - k0) * len(names) * 16 * 2)
  spans = [name for name, _, _ in ens.timer.spans[before:]]
  chunk = ["k_series_surrogates", "k_series_windows"] + ["k_series_kendall", "k_series_exceed"] * 2
  assert spans == ["k_series_windows"] + ["k_series_kendall"] * 2 + ["k_series_windows"] + chunk * 3
  v = TG._series_of(rec)
  sur = gpu.SeriesSurrogates(rec, seed=99).generate(k0, k1, 0, 5)[0].download()
  want = SGC.significance(v, k0, k1, 8, 2, 1, "linear", 5, sur=sur)
  for key in ("var", "ac"):
    for s, nm in enumerate(names):
      for f in ("ge", "le", "nvalid"):
        assert np.array_equal(getattr(getattr(sig, key), f)[nm], want[key][f][s]), (key, nm, f)
      for f in ("tau", "p_rising", "p_falling"):
        _bits(getattr(getattr(sig, key), f)[nm], want[key][f][s], (key, nm, f))
  # with `until`: a threshold nothing reaches, so every end is K
  sh = gpu.SeriesShifts(rec, 4, threshold=1e9)
  before = len(ens.timer.spans)
  found = sh.detect(k0, k1)
  y, ynames = sh.censored()
  spans = [name for name, _, _ in ens.timer.spans[before:]]
  assert spans == ["k_series_windows", "k_series_shift_scan", "k_series_censor"]
  assert all((found.first[nm] == -1).all() for nm in names) and (sh.end.download() == k1 - k0).all()
  assert np.array_equal(y.download().view(np.uint64), v[k0:k1].view(np.uint64))
  tr, trc = sw.trend(k0, k1), gpu.SeriesWindows((y, ynames), 8, step=2, stream=ens.stream).trend()
  for key in ("var", "ac"):
    for nm in names:
      for f in ("conc", "disc", "tie", "nfin"):
        assert np.array_equal(getattr(getattr(tr, key), f)[nm], getattr(getattr(trc, key), f)[nm])
      _bits(getattr(tr, key).tau[nm], getattr(trc, key).tau[nm], (key, nm))
  before = len(ens.timer.spans)
  until = sw.significance(k0, k1, nsur=5, seed=99, until=sh,
                          max_bytes=8 * (k1 - k0) * len(names) * 16 * 2)
  spans = [name for name, _, _ in ens.timer.spans[before:]]
  chunk = (["k_series_surrogates", "k_series_censor", "k_series_windows"]
           + ["k_series_kendall", "k_series_exceed"] * 2)
  assert spans == (["k_series_censor", "k_series_windows"] + ["k_series_kendall"] * 2
                   + ["k_series_fit_ranged"] + chunk * 3)
  # every end is K: the ranged fit is the one-window fit, and the test is the plain one
  for key in ("var", "ac"):
    for nm in names:
      for f in ("ge", "le", "nvalid"):
        assert np.array_equal(getattr(getattr(until, key), f)[nm], getattr(getattr(sig, key), f)[nm])
      _bits(getattr(until, key).p_rising[nm], getattr(sig, key).p_rising[nm], (key, nm))
