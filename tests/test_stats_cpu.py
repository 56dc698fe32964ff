"""SeriesStats and the two pm_series_* entries without a device: the restatement
(tests/stats_cases.py) against np.quantile, np.min / np.max, math.fsum and np.var on the case
table; the host's group permutation; the header mirrors; every argument check of the entries and
of SeriesStats."""
import ctypes as C
import math

import numpy as np
import pytest

import stats_cases as SC
from test_steady_cpu import _layout

U = 2.0**-53


# ------------------------------------------------------------------ the restatement
def _group_rows():
  """(case name, k, s, g, x): every (record, index, group) of every group case's window."""
  for c in SC.group_cases():
    for k in range(c["k0"], c["k1"]):
      for s in range(c["v"].shape[1]):
        for g in range(len(c["start"]) - 1):
          yield c["name"], k, s, g, c["v"][k, s, c["order"][c["start"][g]:c["start"][g + 1]]]


def test_table_holds_what_it_must():
  sizes = set()
  for c in SC.group_cases():
    sizes |= set(np.diff(c["start"]).tolist())
  assert {0, 1, 2, 3, 63, 64, 65, 128, 129, 1000, 8192} <= sizes
  both = [np.diff(c["start"]) for c in SC.group_cases()]
  assert any((d > 64).any() and ((d > 0) & (d <= 64)).any() for d in both)
  assert any(c["groups"] is not None for c in SC.group_cases())
  assert sorted(SC.PROBS.tolist()) == sorted([0, 0.05, 0.25, 0.5, 0.75, 0.95, 1, 1 / 3])
  lens = {c["k1"] - c["k0"] for c in SC.member_cases()}
  assert {1, 2, 255, 256, 257, 600} <= lens
  assert {c["v"].shape[2] for c in SC.member_cases()} >= {1, 5, 64, 65}
  assert any(c["k0"] != 0 and c["k1"] < c["v"].shape[0] for c in SC.member_cases())
  assert any(c["lags"] == (1, 2, 10, 255) for c in SC.member_cases())


def test_quantiles_min_max_equal_numpy():
  rows = 0
  for name, k, s, g, x in _group_rows():
    count, st = SC.group_one(x, SC.PROBS)
    f = x[np.isfinite(x)]
    assert count == f.size
    if count == 0:
      assert np.isnan(st).all(), (name, k, s, g)
      continue
    with np.errstate(all="ignore"):
      want = np.quantile(f, SC.PROBS)
    # bit for bit -- except the sign of a result that IS zero: np.quantile partitions with <, which
    # leaves -0.0 and +0.0 in either order, while the definition sorts -0.0 first
    nz = want != 0.0
    assert st[5:][nz].tobytes() == want[nz].tobytes(), (name, k, s, g, st[5:], want)
    assert np.array_equal(st[5:], want), (name, k, s, g, st[5:], want)
    assert st[2] == np.min(f) and st[3] == np.max(f), (name, k, s, g)
    srt = SC.sort_finite(x)
    assert st[2].tobytes() == srt[0].tobytes() and st[3].tobytes() == srt[-1].tobytes()
    rows += 1
  assert rows > 100


def _check_sum_and_var(terms_x, got_sum, got_var, got_mean, depth, what):
  """|sum - fsum| <= (depth + 1) 2^-53 sum|x|, and var against np.var(ddof=1) with the same bound
  applied to sum d^2.  np.var is given the restatement's mean (NumPy >= 2.0: `mean=`), so that the
  two differ in the order of summing the SAME d^2 and not through deviations about two roundings
  of the mean -- about an all-equal group those differ by 100 % of a variance of 1e-34, which no
  bound on a summation order covers.  Returns the two error / bound ratios."""
  f = terms_x[np.isfinite(terms_x)]
  bound = (depth + 1) * U * math.fsum(np.abs(f))
  err = abs(float(got_sum) - math.fsum(f))
  assert err <= bound, (what, err, bound)
  r_sum = err / bound if bound > 0 else 0.0
  r_var = 0.0
  if f.size >= 2:
    with np.errstate(all="ignore"):
      d2 = (f - got_mean) * (f - got_mean)
      want = np.var(f, ddof=1, mean=np.float64(got_mean))
    if np.isfinite(d2).all() and np.isfinite(math.fsum(d2)):
      vbound = (depth + 1) * U * math.fsum(d2) / (f.size - 1)
      verr = abs(float(got_var) - float(want))
      assert verr <= vbound, (what, verr, vbound)
      r_var = verr / vbound if vbound > 0 else 0.0
    else:  # magnitudes of 1e300: the squares overflow in both
      assert got_var == want or (np.isnan(got_var) and np.isnan(want)), (what, got_var, want)
  else:
    assert np.isnan(got_var), what
  return r_sum, r_var


def test_member_tree_sum_and_var_within_the_derived_bound():
  """d = ceil(G / 64) + 5: the additions an element passes through (its residue sum, then six
  strides, less one for the first element of a residue class, which is added to +0.0 exactly)."""
  worst = [0.0, 0.0]
  for name, k, s, g, x in _group_rows():
    count, st = SC.group_one(x, SC.PROBS)
    if count == 0:
      continue
    d = -(-x.size // 64) + 5
    r = _check_sum_and_var(x, st[4], st[1], st[0], d, (name, k, s, g))
    worst = [max(a, b) for a, b in zip(worst, r)]
  print("member tree: largest |sum - fsum| / bound %.3f, |var - np.var| / bound %.3f"
        % tuple(worst))


def test_time_sum_and_var_within_the_derived_bound():
  """d = 255 + ceil(K / 256): inside a chunk, then across the chunk partials."""
  worst = [0.0, 0.0]
  for c in SC.member_cases():
    count, first, ncross, st = SC.member_stats(c["v"], c["lags"], c["thr"], c["dirs"], c["k0"],
                                               c["k1"])
    K = c["k1"] - c["k0"]
    d = 255 + -(-K // 256)
    for s in range(c["v"].shape[1]):
      for m in range(c["v"].shape[2]):
        x = c["v"][c["k0"]:c["k1"], s, m]
        f = x[np.isfinite(x)]
        assert count[s, m] == f.size
        if f.size == 0:
          assert np.isnan(st[s, m, :4]).all() and st[s, m, 4] == 0.0
          assert not np.signbit(st[s, m, 4])
          continue
        assert st[s, m, 2] == f.min() and st[s, m, 3] == f.max()
        r = _check_sum_and_var(x, st[s, m, 4], st[s, m, 1], st[s, m, 0], d, (c["name"], s, m))
        worst = [max(a, b) for a, b in zip(worst, r)]
  print("time sum: largest |sum - fsum| / bound %.3f, |var - np.var| / bound %.3f" % tuple(worst))


def test_member_restatement_on_a_series_worked_by_hand():
  """One member, threshold "below 0": hits, first, crossings, signed zeros, a lag-1 product."""
  x = np.array([9.0, 1.0, -1.0, np.nan, -2.0, 0.0, -0.0, 3.0, 9.0])
  v = x.reshape(-1, 1, 1)
  count, first, ncross, st = SC.member_stats(v, (1,), [0.0], [-1], 1, 8)
  # window: 1, -1, NaN, -2, 0, -0, 3 -> finite 6, hits -1 and -2; crossings 1|-1 and -2|0
  assert (count[0, 0], first[0, 0], ncross[0, 0]) == (6, 2, 2)
  mean = (1.0 - 1.0 - 2.0 + 0.0 - 0.0 + 3.0) / 6.0
  assert st[0, 0, 0] == mean and st[0, 0, 4] == 1.0 and st[0, 0, 5] == 2.0 / 6.0
  assert st[0, 0, 2] == -2.0 and st[0, 0, 3] == 3.0
  pairs = [(1.0, -1.0), (-2.0, 0.0), (0.0, -0.0), (-0.0, 3.0)]
  acc = 0.0
  for a, b in pairs:
    acc = acc + (a - mean) * (b - mean)
  assert st[0, 0, 6] == acc / 4.0
  # signed zeros alone: min -0.0, max +0.0
  z = np.array([0.0, -0.0, 0.0]).reshape(-1, 1, 1)
  _, first, ncross, st = SC.member_stats(z, (), [np.nan], [1], 0, 3)
  assert np.signbit(st[0, 0, 2]) and not np.signbit(st[0, 0, 3])
  assert np.isnan(st[0, 0, 5]) and first[0, 0] == -1 and ncross[0, 0] == 0


# ------------------------------------------------------------------ the host's permutation
def test_group_order_is_a_stable_sort():
  from pymoc_amd.stats import group_order
  rng = np.random.default_rng(5)
  labels_in = rng.choice([-7, 3, 2**40, 11], size=300)
  labels, order, start = group_order(labels_in, 300)
  assert labels.tolist() == [-7, 3, 11, 2**40]
  assert sorted(order.tolist()) == list(range(300)) and order.dtype == np.int32
  assert start[0] == 0 and start[-1] == 300 and start.dtype == np.int32
  for g, lab in enumerate(labels):
    members = order[start[g]:start[g + 1]]
    assert (labels_in[members] == lab).all() and (np.diff(members) > 0).all()
  o2, s2 = SC.order_of(labels_in)
  assert np.array_equal(order, o2) and np.array_equal(start, s2)
  labels, order, start = group_order(None, 7)
  assert order.tolist() == list(range(7)) and start.tolist() == [0, 7] and labels.size == 1
  labels, order, start = group_order(np.arange(12) % 4, 12)
  assert order.tolist() == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]


# ------------------------------------------------------------------ the C-ABI
def test_stats_layouts_match_header(tmp_path):
  from pymoc_amd import _lib
  for cls in (_lib.pm_series_group_stats, _lib.pm_series_member_stats):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_series_group_stats"][1][0] is C.POINTER(_lib.pm_series_group_stats)
  assert _lib.SIGNATURES["pm_series_member_stats"][1][0] is C.POINTER(_lib.pm_series_member_stats)
  assert (_lib.PM_STATS_Q_MAX, _lib.PM_STATS_LAG_MAX, _lib.PM_STATS_GROUP_MAX,
          _lib.PM_STATS_CHUNK) == (SC.Q_MAX, SC.LAG_MAX, SC.GROUP_MAX, SC.CHUNK)


FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first


def group_desc(keep, **kw):
  """A valid descriptor (device addresses are stand-ins) with the edits `kw`; `keep` holds the host
  mirrors alive; start_values= and q_values= fill the mirrors, every other keyword sets a field."""
  from pymoc_amd import _lib
  d = _lib.pm_series_group_stats()
  start = np.asarray(kw.pop("start_values", [0, 3, 3, 10]), dtype=np.int32)
  q = np.asarray(kw.pop("q_values", [0.0, 0.5, 1.0]), dtype=np.float64)
  keep += [start, q]
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.ngroups, d.nq = 10, 2, 6, 1, 5, start.size - 1, q.size
  d.v, d.order, d.start_dev, d.q_dev = FAKE, FAKE + 4096, FAKE + 8192, FAKE + 12288
  d.start, d.q = start.ctypes.data, q.ctypes.data
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_group_descriptors():
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("n -1", dict(n=-1)), ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=5)),
          ("k0 > k1", dict(k0=4, k1=2)), ("k1 > nrec", dict(k1=7)), ("ngroups 0", dict(ngroups=0)),
          ("ngroups -2", dict(ngroups=-2)), ("nq 9", dict(nq=9)), ("nq -1", dict(nq=-1)),
          ("v", dict(v=None)), ("order", dict(order=None)), ("start", dict(start=None)),
          ("start_dev", dict(start_dev=None)), ("q", dict(q=None)), ("q_dev", dict(q_dev=None)),
          ("q > 1", dict(q_values=[0.5, 1.0000001])), ("q < 0", dict(q_values=[-1e-9])),
          ("q nan", dict(q_values=[0.25, np.nan])), ("start falls", dict(start_values=[0, 5, 3, 10])),
          ("start[0]", dict(start_values=[1, 3, 3, 10])), ("start ends early", dict(start_values=[0, 3, 3, 9])),
          ("start ends late", dict(start_values=[0, 3, 3, 11])),
          ("group too large", dict(n=8200, start_values=[0, 8193, 8200]))]


def member_desc(keep, **kw):
  from pymoc_amd import _lib
  d = _lib.pm_series_member_stats()
  lag = np.asarray(kw.pop("lag_values", [1, 3]), dtype=np.int32)
  thr = np.asarray(kw.pop("thr_values", [np.nan, 0.5]), dtype=np.float64)
  dirs = np.asarray(kw.pop("dir_values", [-1, 1]), dtype=np.int32)
  keep += [lag, thr, dirs]
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.nlag = 10, 2, 6, 1, 5, lag.size
  d.v, d.lag_dev, d.thr_dev, d.dir_dev = FAKE, FAKE + 4096, FAKE + 8192, FAKE + 12288
  d.lag, d.thr, d.dir = lag.ctypes.data, thr.ctypes.data, dirs.ctypes.data
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def bad_member_descriptors():
  return [("n 0", dict(n=0)), ("nspec 0", dict(nspec=0)), ("nrec 0", dict(nrec=0)),
          ("k0 -1", dict(k0=-1)), ("k0 = k1", dict(k0=5)), ("k1 > nrec", dict(k1=7)),
          ("nlag 5", dict(nlag=5)), ("nlag -1", dict(nlag=-1)), ("v", dict(v=None)),
          ("lag", dict(lag=None)), ("lag_dev", dict(lag_dev=None)), ("thr", dict(thr=None)),
          ("thr_dev", dict(thr_dev=None)), ("dir", dict(dir=None)), ("dir_dev", dict(dir_dev=None)),
          ("lag 0", dict(lag_values=[0])), ("lag -1", dict(lag_values=[1, -1])),
          ("lag = window", dict(lag_values=[4])), ("lag > window", dict(lag_values=[2, 100])),
          ("dir 0", dict(dir_values=[0, 1])), ("dir 2", dict(dir_values=[-1, 2]))]


def test_entries_reject_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  keep = []
  assert L.pm_series_group_stats(None, FAKE, FAKE, None) == _lib.PM_EINVAL
  assert L.pm_series_member_stats(None, FAKE, FAKE, FAKE, FAKE, None) == _lib.PM_EINVAL
  for label, kw in bad_group_descriptors():
    d = group_desc(keep, **kw)
    assert L.pm_series_group_stats(C.byref(d), FAKE + 64, FAKE + 128, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = group_desc(keep)
  for out in ((None, FAKE), (FAKE, None)):
    assert L.pm_series_group_stats(C.byref(d), out[0], out[1], None) == _lib.PM_EINVAL
  for label, kw in bad_member_descriptors():
    d = member_desc(keep, **kw)
    args = (FAKE + 64, FAKE + 128, FAKE + 192, FAKE + 256)
    assert L.pm_series_member_stats(C.byref(d), *args, None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  d = member_desc(keep)
  for i in range(4):
    args = [FAKE + 64, FAKE + 128, FAKE + 192, FAKE + 256]
    args[i] = None
    assert L.pm_series_member_stats(C.byref(d), *args, None) == _lib.PM_EINVAL
  # q and lag may be NULL when none is asked for -- then it is the next check that refuses
  d = group_desc(keep, q_values=[], k0=9)
  d.q = d.q_dev = None
  assert L.pm_series_group_stats(C.byref(d), FAKE, FAKE, None) == _lib.PM_EINVAL
  assert "window" in L.pm_last_error().decode()


# ------------------------------------------------------------------ SeriesStats
class _Series(object):
  """A stand-in for a device series: a shape and a dtype, no memory."""

  def __init__(self, shape, dtype=np.float64):
    self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), 0


class _Recorder(object):
  """A stand-in for an IndexRecorder: what SeriesStats reads off one."""

  class _T(object):
    names = ["amoc", "depth"]

  class _E(object):
    stream = timer = None

  def __init__(self, written):
    self._values, self.table, self.ens = _Series((len(written), 2, 6)), self._T(), self._E()
    self.steps = np.where(written, np.arange(len(written)) * 12, -1)


def test_series_stats_validates_its_arguments_before_any_device_array():
  """Every refusal is a ValueError raised on the host: none of these reaches a device call, which
  on a machine without a GPU would raise a PmError instead."""
  from pymoc_amd import SeriesStats
  src = (_Series((10, 2, 6)), ["amoc", "depth"])
  ok = SeriesStats(src, groups=[5, 5, 9, 9, 5, 1], quantiles=(0.05, 0.5), lags=(1, 3),
                   thresholds=dict(amoc=(12.5, "below")))
  assert ok.group_labels.tolist() == [1, 5, 9] and ok.ngroups == 3
  assert ok._order.tolist() == [5, 0, 1, 4, 2, 3] and ok._start.tolist() == [0, 1, 4, 6]
  assert np.isnan(ok._thr[1]) and ok._thr[0] == 12.5 and ok._dir.tolist() == [-1, -1]
  assert SeriesStats(src).ngroups == 1
  for bad in ((_Series((10, 2)), ["a", "b"]), (_Series((10, 2, 6), np.float32), ["a", "b"]),
              (_Series((10, 0, 6)), []), (_Series((10, 2, 6)),)):
    with pytest.raises(ValueError, match="series|source"):
      SeriesStats(bad)
  for names in (["amoc"], ["amoc", "amoc"], ["a", "b", "c"]):
    with pytest.raises(ValueError, match="names"):
      SeriesStats((_Series((10, 2, 6)), names))
  for groups in (np.zeros(5, int), np.zeros((6, 1), int), np.zeros(6), 3):
    with pytest.raises(ValueError, match="groups"):
      SeriesStats(src, groups=groups)
  big = (_Series((2, 1, 8193)), ["a"])
  with pytest.raises(ValueError, match="more than 8192"):
    SeriesStats(big)
  with pytest.raises(ValueError, match="group 4 has 8193 members, more than 8192"):
    SeriesStats((_Series((2, 1, 8200)), ["a"]), groups=np.r_[np.full(8193, 4), 10 + np.arange(7)])
  for q in ((-0.1,), (1.5,), (0.5, np.nan), np.linspace(0, 1, 9), np.zeros((2, 2))):
    with pytest.raises(ValueError, match="quantile"):
      SeriesStats(src, quantiles=q)
  for lags in ((0,), (1, -2), (1.5,), (1, 2, 3, 4, 5), np.ones((2, 2), int)):
    with pytest.raises(ValueError, match="lag"):
      SeriesStats(src, lags=lags)
  for thr, word in ((dict(psi=(1., "below")), "unknown index"), (dict(amoc=(1., "under")), "direction"),
                    (dict(amoc=1.0), "give"), (dict(amoc=(np.nan, "above")), "finite"),
                    (dict(amoc=(np.inf, "above")), "finite"), (dict(amoc=(1., "below", 3)), "give")):
    with pytest.raises(ValueError, match=word):
      SeriesStats(src, thresholds=thr)
  for k0, k1 in ((-1, 4), (4, 4), (5, 2), (0, 11), (10, None)):
    with pytest.raises(ValueError, match="window"):
      ok.across_members(k0, k1)
    with pytest.raises(ValueError, match="window"):
      ok.along_time(k0, k1)
  with pytest.raises(ValueError, match="lag 3 does not fit a window of 3 records"):
    ok.along_time(2, 5)
  # a recorder: the records never written
  rec = _Recorder(np.array([True, True, True, False, False]))
  st = SeriesStats(rec, groups=[0, 0, 0, 1, 1, 1])
  assert st.names == ["amoc", "depth"] and (st.nrec, st.nspec, st.n) == (5, 2, 6)
  for call in (st.across_members, st.along_time):
    with pytest.raises(ValueError, match=r"window \[0, 5\) holds record 3, which was never written"):
      call()
    with pytest.raises(ValueError, match="record 3"):
      call(2, 4)
