"""The launch orders of the recorded-series chain, without a device: `windows.indicators`, the one
path of the record and of a chunk of surrogates, with recording stand-ins for the launch functions,
and the whole `significance` with a recording timer over entries that do nothing.  The orders are
the ones the GPU span tests pin (test_windows_gpu, test_smooth_gpu, test_surrogates_gpu,
test_shifts_gpu), copied from there."""
import contextlib

import numpy as np
import pytest

from test_windows_cpu import FAKE, _Recorder

K0, K1, NSUR = 2, 40, 5
HEAD = ["k_series_windows"] + ["k_series_kendall"] * 2
COUNT = ["k_series_kendall", "k_series_exceed"] * 2
# (observed part, one chunk) by (gaussian, until); three chunks follow the observed part
ORDERS = {
    (False, False): (HEAD + ["k_series_windows"], ["k_series_surrogates", "k_series_windows"] + COUNT),
    (True, False): (["k_series_smooth"] + HEAD + ["k_series_windows"],
                    ["k_series_surrogates", "k_series_smooth", "k_series_windows"] + COUNT),
    (False, True): (["k_series_censor"] + HEAD + ["k_series_fit_ranged"],
                    ["k_series_surrogates", "k_series_censor", "k_series_windows"] + COUNT),
    (True, True): (["k_series_censor", "k_series_smooth"] + HEAD + ["k_series_fit_ranged"],
                   ["k_series_surrogates", "k_series_censor", "k_series_smooth", "k_series_windows"]
                   + COUNT),
}


class _Dev(object):
  """A stand-in for a DeviceArray: a shape, a dtype and an address nothing dereferences."""

  def __init__(self, shape, dtype=np.float64):
    self.shape = tuple(int(s) for s in np.atleast_1d(shape))
    self.dtype, self.ptr = np.dtype(dtype), FAKE

  @classmethod
  def from_host(cls, arr, dtype=None, stream=None):
    return cls(np.shape(arr), dtype or np.float64)

  @classmethod
  def zeros(cls, shape, dtype=np.float64, stream=None):
    return cls(shape, dtype)

  def download(self, out=None, stream=None):
    return np.zeros(self.shape, self.dtype)


class _Timer(object):
  """A stand-in for a LaunchTimer: the names of the spans, in order."""

  def __init__(self):
    self.names = []

  @contextlib.contextmanager
  def span(self, name, stream=None):
    self.names.append(name)
    yield


class _Entries(object):
  """A stand-in for the library: every pm_series_* entry returns PM_OK and launches nothing."""

  def __getattr__(self, name):
    assert name.startswith("pm_series_"), name
    return lambda *args: 0


@pytest.fixture
def no_device(monkeypatch):
  from pymoc_amd import shifts, smooth, surrogates, windows
  for mod in (shifts, smooth, surrogates, windows):
    monkeypatch.setattr(mod, "DeviceArray", _Dev)
    monkeypatch.setattr(mod, "lib", _Entries())


@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("until", [False, True])
def test_indicators_issues_censor_smooth_windows_for_the_record_and_for_a_chunk(monkeypatch, gaussian,
                                                                              until):
  """`indicators` with recording launch functions: censor (with `until`), smooth (under
  "gaussian"), windows, each reading what the one before wrote -- into a copy for the record, in
  place and into the given arrays for a chunk."""
  from pymoc_amd import shifts, windows as W
  from pymoc_amd.series import Ctx
  calls = []

  def censor(x, y, cens, ctx, end_out=None):
    calls.append(("k_series_censor", x.ptr, x.shape, y))

  def smooth(x, k0, k1, w, ctx, trend=None, resid=None, nbad=None):
    calls.append(("k_series_smooth", x, k0, k1, resid, nbad))

  def wins(x, k0, k1, par, ctx, out=None):
    calls.append(("k_series_windows", x, k0, k1, par, out))
    return out

  monkeypatch.setattr(shifts, "launch_censor", censor)
  monkeypatch.setattr(W, "launch_smooth", smooth)
  monkeypatch.setattr(W, "launch_windows", wins)
  monkeypatch.setattr(W, "DeviceArray", _Dev)
  par, ctx = W.win_par(8, 2, 1, "gaussian" if gaussian else "linear"), Ctx(None, None)
  kw = dict(cens=object() if until else None, weights=object() if gaussian else None)
  want = [nm for nm, on in (("k_series_censor", until), ("k_series_smooth", gaussian),
                            ("k_series_windows", True)) if on]
  # the record: records [K0, K1) of 50, everything allocated by the chain
  x = _Dev((50, 2, 6))
  x.ptr = 8 * 4096
  out, on = W.indicators(x, K0, K1, par, ctx, **kw)
  assert [c[0] for c in calls] == want
  K, shape = K1 - K0, (K1 - K0, 2, 6)
  series, r0, r1 = x, K0, K1
  if until:
    _, ptr, shp, copy = calls.pop(0)
    assert (ptr, shp) == (x.ptr + 8 * K0 * 12, shape) and copy is not x and copy.shape == shape
    series, r0, r1 = copy, 0, K
  if gaussian:
    _, src, a, b, resid, nbad = calls.pop(0)
    assert (src, a, b) == (series, r0, r1) and resid.shape == shape and nbad is None
    series, r0, r1 = resid, 0, K
  assert calls.pop() == ("k_series_windows", series, r0, r1, par, None)
  assert on == (series, r0, r1)
  # a chunk: all K records of the planes, censored in place, the arrays given
  y, yres, nbad, wout = _Dev((K, 4, 6)), _Dev((K, 4, 6)), _Dev((4, 6), np.int32), (_Dev(1), _Dev(1))
  got, on = W.indicators(y, 0, K, par, ctx, into=y, resid=yres, nbad=nbad, out=wout, **kw)
  assert [c[0] for c in calls] == want and got is wout
  if until:
    assert calls.pop(0) == ("k_series_censor", y.ptr, (K, 4, 6), y)
  if gaussian:
    assert calls.pop(0) == ("k_series_smooth", y, 0, K, yres, nbad)
  assert calls == [("k_series_windows", yres if gaussian else y, 0, K, par, wout)]
  assert on == (yres if gaussian else y, 0, K)


@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("until", [False, True])
def test_the_classes_issue_the_launch_orders_the_gpu_span_tests_pin(no_device, gaussian, until):
  """compute, trend, SeriesSurrogates.fit and significance (three chunks of 2, 2 and 1 surrogates)
  on a recorder stand-in whose timer records the spans: plain, "gaussian", `until`, and both."""
  from pymoc_amd import SeriesShifts, SeriesSurrogates, SeriesWindows
  from pymoc_amd.shifts import Censor
  rec = _Recorder(np.ones(K1, dtype=bool))
  rec.ens.timer, rec.ens._member0 = _Timer(), 0
  timer = rec.ens.timer
  kw = dict(detrend="gaussian", sigma=2.0) if gaussian else {}
  sw = SeriesWindows(rec, 8, step=2, **kw)
  lead = ["k_series_smooth"] if gaussian else []

  def spans(call):
    del timer.names[:]
    call()
    return list(timer.names)

  assert spans(lambda: sw.compute(K0, K1)) == lead + ["k_series_windows"]
  assert spans(lambda: sw.trend(K0, K1)) == lead + HEAD
  assert spans(lambda: SeriesSurrogates(rec, seed=9, **kw).fit(K0, K1)) == lead + ["k_series_windows"]
  sh = None
  if until:
    sh = SeriesShifts(rec, 4)
    sh._found, sh.end = (K0, K1), _Dev((2, 6), np.int32)
    sh._cens = Censor(_Dev((2, 6), np.int32), 0, np.arange(2, dtype=np.int32), _Dev(2, np.int32))
  one = (16 if gaussian else 8) * (K1 - K0) * 2 * 6
  observed, chunk = ORDERS[gaussian, until]
  got = spans(lambda: sw.significance(K0, K1, nsur=NSUR, seed=9, max_bytes=2 * one, until=sh))
  assert got == observed + chunk * 3
