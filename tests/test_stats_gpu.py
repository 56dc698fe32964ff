"""pm_series_group_stats, pm_series_member_stats and SeriesStats on the device: every case of
tests/stats_cases.py through the C-ABI bit for bit against the restatement, what the launches leave
alone, windows, a recorded noise ensemble, its shards, and the launches of a run without
SeriesStats."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _padded, _up
import stats_cases as SC

pytestmark = pytest.mark.gpu

def run_group(gpu, v, order, start, probs, k0, k1):
  """One launch into sentinel-filled outputs [nrec][nspec][ngroups]; returns (count, stat)."""
  from pymoc_amd import _lib
  nrec, nspec, n = v.shape
  ng, nq = len(start) - 1, len(probs)
  series, v_ptr = _padded(gpu, v)
  start = np.ascontiguousarray(start, dtype=np.int32)
  probs = np.ascontiguousarray(probs, dtype=np.float64)
  d_order, d_start = _up(gpu, np.ascontiguousarray(order, dtype=np.int32)), _up(gpu, start)
  d_q = _up(gpu, probs if nq else np.zeros(1))
  count = _up(gpu, np.full((nrec, nspec, ng), I_SENTINEL, dtype=np.int32))
  stat = _up(gpu, np.full((nrec, nspec, ng, 5 + nq), V_SENTINEL))
  d = _lib.pm_series_group_stats()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.ngroups, d.nq = n, nspec, nrec, k0, k1, ng, nq
  d.v, d.order, d.start, d.start_dev = v_ptr, d_order.ptr, start.ctypes.data, d_start.ptr
  d.q, d.q_dev = probs.ctypes.data, d_q.ptr
  _lib.check(_lib.lib.pm_series_group_stats(C.byref(d), count.ptr, stat.ptr, None))
  gpu.synchronize()
  return count.download(), stat.download()


def run_member(gpu, v, lags, thr, dirs, k0, k1):
  from pymoc_amd import _lib
  nrec, nspec, n = v.shape
  series, v_ptr = _padded(gpu, v)
  lags = np.ascontiguousarray(lags, dtype=np.int32)
  thr = np.ascontiguousarray(thr, dtype=np.float64)
  dirs = np.ascontiguousarray(dirs, dtype=np.int32)
  d_lag = _up(gpu, lags if lags.size else np.zeros(1, dtype=np.int32))
  d_thr, d_dir = _up(gpu, thr), _up(gpu, dirs)
  ints = [_up(gpu, np.full((nspec, n), I_SENTINEL, dtype=np.int32)) for _ in range(3)]
  stat = _up(gpu, np.full((nspec, n, 6 + lags.size + 1), V_SENTINEL))  # (one double to spare)
  d = _lib.pm_series_member_stats()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.nlag = n, nspec, nrec, k0, k1, lags.size
  d.v, d.lag, d.lag_dev = v_ptr, lags.ctypes.data, d_lag.ptr
  d.thr, d.thr_dev, d.dir, d.dir_dev = thr.ctypes.data, d_thr.ptr, dirs.ctypes.data, d_dir.ptr
  _lib.check(_lib.lib.pm_series_member_stats(C.byref(d), ints[0].ptr, ints[1].ptr, ints[2].ptr,
                                             stat.ptr, None))
  gpu.synchronize()
  flat = stat.download().ravel()
  used = nspec * n * (6 + lags.size)
  assert (flat[used:] == V_SENTINEL).all()  # nothing behind the last member's row
  return [a.download() for a in ints], flat[:used].reshape(nspec, n, 6 + lags.size)


GROUP_CASES = SC.group_cases()
MEMBER_CASES = SC.member_cases()


@pytest.mark.parametrize("case", GROUP_CASES, ids=[c["name"] for c in GROUP_CASES])
def test_group_stats_bit_for_bit(gpu, case):
  c = case
  k0, k1 = c["k0"], c["k1"]
  count, stat = run_group(gpu, c["v"], c["order"], c["start"], c["probs"], k0, k1)
  want_count, want_stat = SC.group_stats(c["v"], c["order"], c["start"], c["probs"], k0, k1)
  assert np.array_equal(count[k0:k1], want_count), c["name"]
  _bits(stat[k0:k1], want_stat, c["name"])
  # records outside the window still hold the sentinel
  for a, sent in ((count, I_SENTINEL), (stat, V_SENTINEL)):
    assert (a[:k0] == sent).all() and (a[k1:] == sent).all(), c["name"]
  # the same records as a series of their own: the same bits
  c2, s2 = run_group(gpu, c["v"][k0:k1], c["order"], c["start"], c["probs"], 0, k1 - k0)
  assert np.array_equal(c2, count[k0:k1])
  _bits(s2, stat[k0:k1], (c["name"], "own series"))
  # fewer probabilities: the leading columns do not move
  c3, s3 = run_group(gpu, c["v"], c["order"], c["start"], c["probs"][:2], k0, k1)
  _bits(s3[k0:k1], stat[k0:k1, ..., :7], (c["name"], "nq 2"))
  c4, s4 = run_group(gpu, c["v"], c["order"], c["start"], c["probs"][:0], k0, k1)
  _bits(s4[k0:k1], stat[k0:k1, ..., :5], (c["name"], "nq 0"))


@pytest.mark.parametrize("case", MEMBER_CASES, ids=[c["name"] for c in MEMBER_CASES])
def test_member_stats_bit_for_bit(gpu, case):
  c = case
  k0, k1 = c["k0"], c["k1"]
  ints, stat = run_member(gpu, c["v"], c["lags"], c["thr"], c["dirs"], k0, k1)
  wc, wf, wx, wstat = SC.member_stats(c["v"], c["lags"], c["thr"], c["dirs"], k0, k1)
  for got, want, what in zip(ints, (wc, wf, wx), ("count", "first", "ncross")):
    assert np.array_equal(got, want), (c["name"], what, np.argwhere(got != want)[:5])
  _bits(stat, wstat, c["name"])
  # the same records as a series of their own: `first` moves by k0, nothing else does
  i2, s2 = run_member(gpu, c["v"][k0:k1], c["lags"], c["thr"], c["dirs"], 0, k1 - k0)
  assert np.array_equal(i2[0], ints[0]) and np.array_equal(i2[2], ints[2])
  assert np.array_equal(np.where(i2[1] >= 0, i2[1] + k0, -1), ints[1])
  _bits(s2, stat, (c["name"], "own series"))
  # without lags: the leading columns do not move
  i3, s3 = run_member(gpu, c["v"], (), c["thr"], c["dirs"], k0, k1)
  _bits(s3, stat[..., :6], (c["name"], "no lag"))


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_stats_cpu as TC
  keep = []
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(4)]
  for label, kw in TC.bad_group_descriptors():
    d = TC.group_desc(keep, **kw)
    assert _lib.lib.pm_series_group_stats(C.byref(d), out[0].ptr, out[1].ptr,
                                          None) == _lib.PM_EINVAL, label
  for label, kw in TC.bad_member_descriptors():
    d = TC.member_desc(keep, **kw)
    assert _lib.lib.pm_series_member_stats(C.byref(d), out[0].ptr, out[1].ptr, out[2].ptr,
                                           out[3].ptr, None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ a recorded noise ensemble
SPECS = [("amoc", "max", "Psi", dict(zhi=-500.)), ("b_1000", "at", "b_basin", dict(x0=-1000.))]
GROUPS = np.repeat(np.arange(4), 4)
N_SAMPLES = 24
KW = dict(quantiles=(0.05, 0.5, 0.95), lags=(1, 10), thresholds=dict(amoc=(0.0, "above")))


class _Shard(object):
  """What a driver reads off a communicator to place its members: rank and world."""

  def __init__(self, rank, world):
    self.rank, self.world = rank, world


def _cfg16():
  """4 parameter sets (config5's db, B, kapGM, tau) x 4 realisations, nz = 81, a sample a year:
  members 4 g .. 4 g + 3 are copies of set g, driven apart by the noise alone."""
  import pymoc_amd
  from pymoc_amd import configs
  one = configs.config5(N=4, nz=81, dt_days=30.)
  cfg = dict(one)
  for key in pymoc_amd.JN2018Ensemble.MEMBER_KEYS:
    a = np.asarray(one.get(key, 0.0))
    if a.ndim >= 1 and a.shape[0] == 4:
      cfg[key] = np.repeat(a, 4, axis=0)
  return cfg


def _noise(gpu):
  return gpu.NoiseForcing(2018, tau=dict(sigma=0.02),
                          bs_north=dict(sigma=2e-4, tau_corr=10 * 360 * 86400.))


def _recorded(gpu, cfg, timer=False, **kw):
  from pymoc_amd.device import LaunchTimer
  ens = gpu.JN2018Ensemble(cfg, noise=_noise(gpu), **kw)
  M = int(cfg["MOC_up_iters"])
  rec = gpu.IndexRecorder(ens, SPECS, M, N_SAMPLES + 2)  # two records are never written
  if timer:
    ens.timer = LaunchTimer()
  ens.run((N_SAMPLES - 1) * M + 1)
  assert (rec.steps[:N_SAMPLES] >= 0).all() and (rec.steps[N_SAMPLES:] == -1).all()
  return ens, rec


@pytest.fixture(scope="module")
def whole(gpu):
  """The 16-member run, its SeriesStats results and its launch-span names before SeriesStats."""
  ens, rec = _recorded(gpu, _cfg16(), timer=True)
  names_before = [name for name, _, _ in ens.timer.spans]
  st = gpu.SeriesStats(rec, groups=GROUPS, **KW)
  across, along = st.across_members(0, N_SAMPLES), st.along_time(2, N_SAMPLES)
  names_after = [name for name, _, _ in ens.timer.spans]
  return dict(ens=ens, rec=rec, st=st, across=across, along=along, before=names_before,
              after=names_after)


def _series_of(rec):
  """[n_samples, nspec, n] from the recorder's host view."""
  return np.stack([rec.values[name].T for name in rec.table.names], axis=1)


def _check_against_restatement(st, across, along, v, groups, k_across, k_along):
  order, start = SC.order_of(groups)
  wc, ws = SC.group_stats(v, order, start, st.quantiles, *k_across)
  thr, dirs = np.array([0.0, np.nan]), np.array([1, -1], dtype=np.int32)
  mc, mf, mx, ms = SC.member_stats(v, tuple(st.lags), thr, dirs, *k_along)
  for s, name in enumerate(st.names):
    assert np.array_equal(across.count[name], wc[:, s, :].T), name
    for i, key in enumerate(("mean", "var", "min", "max", "sum")):
      _bits(getattr(across, key)[name], ws[:, s, :, i].T, (name, key))
    _bits(across.quantile[name], ws[:, s, :, 5:].transpose(2, 1, 0), (name, "quantile"))
    assert np.array_equal(along.count[name], mc[s]) and np.array_equal(along.first[name], mf[s])
    assert np.array_equal(along.ncross[name], mx[s]), name
    for i, key in enumerate(("mean", "var", "min", "max", "sum", "frac")):
      _bits(getattr(along, key)[name], ms[s, :, i], (name, key))
    _bits(along.autocov[name], ms[s, :, 6:].T, (name, "autocov"))


def test_series_stats_on_a_recorded_noise_ensemble(gpu, whole):
  st, rec = whole["st"], whole["rec"]
  v = _series_of(rec)
  assert v.shape == (N_SAMPLES + 2, 2, 16) and np.isfinite(v[:N_SAMPLES]).all()
  assert st.group_labels.tolist() == [0, 1, 2, 3]
  assert whole["across"].mean["amoc"].shape == (4, N_SAMPLES)
  assert whole["across"].quantile["amoc"].shape == (3, 4, N_SAMPLES)
  assert whole["along"].autocov["amoc"].shape == (2, 16)
  _check_against_restatement(st, whole["across"], whole["along"], v, GROUPS, (0, N_SAMPLES),
                             (2, N_SAMPLES))
  # the noise acts: the realisations of a set differ, and the sets differ
  assert (whole["across"].var["amoc"][:, 2:] > 0).all()
  assert len(set(whole["across"].mean["amoc"][:, -1].tolist())) == 4
  assert (whole["along"].frac["amoc"] == 1.0).all() and (whole["along"].first["amoc"] == 2).all()
  # a window that reaches a record never written is refused, on the host
  for call in (st.across_members, st.along_time):
    with pytest.raises(ValueError, match="record %d, which was never written" % N_SAMPLES):
      call()
    with pytest.raises(ValueError, match="never written"):
      call(N_SAMPLES - 3, N_SAMPLES + 1)


def test_launches_without_series_stats_are_the_ones_of_today(gpu, whole):
  """A recorder run issues no launch of this module; a SeriesStats call adds exactly its one."""
  before, after = whole["before"], whole["after"]
  assert "k_row_indices" in before and before.count("k_row_indices") == N_SAMPLES
  assert not [name for name in before if "series" in name]
  assert after[:len(before)] == before
  assert after[len(before):] == ["k_series_group_stats", "k_series_member_stats"]


@pytest.mark.parametrize("rank", [0, 1])
def test_a_shard_gives_the_whole_ensembles_rows_for_its_groups(gpu, whole, rank):
  cls = gpu.JN2018Ensemble
  sl = slice(8 * rank, 8 * rank + 8)
  part = cls.restrict(_cfg16(), np.arange(16)[sl])
  ens, rec = _recorded(gpu, part, comm=_Shard(rank, 2), n_total=16, diag_iters=0)
  assert ens.noise.desc.member0 == 8 * rank
  _bits(_series_of(rec)[:N_SAMPLES], _series_of(whole["rec"])[:N_SAMPLES, :, sl], rank)
  st = gpu.SeriesStats(rec, groups=GROUPS[sl], **KW)
  assert st.group_labels.tolist() == [2 * rank, 2 * rank + 1]
  across, along = st.across_members(0, N_SAMPLES), st.along_time(2, N_SAMPLES)
  gs = slice(2 * rank, 2 * rank + 2)
  for name in st.names:
    assert np.array_equal(across.count[name], whole["across"].count[name][gs])
    for key in ("mean", "var", "min", "max", "sum"):
      _bits(getattr(across, key)[name], getattr(whole["across"], key)[name][gs], (name, key))
    _bits(across.quantile[name], whole["across"].quantile[name][:, gs], (name, "quantile"))
    for key in ("count", "first", "ncross"):
      assert np.array_equal(getattr(along, key)[name], getattr(whole["along"], key)[name][sl])
    for key in ("mean", "var", "min", "max", "sum", "frac"):
      _bits(getattr(along, key)[name], getattr(whole["along"], key)[name][sl], (name, key))
    _bits(along.autocov[name], whole["along"].autocov[name][:, sl], (name, "autocov"))


def test_series_stats_on_a_plain_device_series(gpu):
  """(DeviceArray, names) as source, interleaved labels that are no 0 .. ngroups - 1."""
  c = SC.member_case(257, 65)
  v = c["v"]
  labels = np.array([40, -3, 7])[np.arange(65) % 3]
  dev = gpu.DeviceArray.from_host(v)
  st = gpu.SeriesStats((dev, ["a", "b", "c"]), groups=labels, quantiles=SC.PROBS, lags=(1, 255),
                       thresholds=dict(a=(-1.0, "below"), b=(1.0, "above")))
  assert st.group_labels.tolist() == [-3, 7, 40]
  k0, k1 = c["k0"], c["k1"]
  across, along = st.across_members(k0, k1), st.along_time(k0, k1)
  order, start = SC.order_of(labels)
  wc, ws = SC.group_stats(v, order, start, SC.PROBS, k0, k1)
  mc, mf, mx, ms = SC.member_stats(v, (1, 255), c["thr"], c["dirs"], k0, k1)
  for s, name in enumerate(st.names):
    assert np.array_equal(across.count[name], wc[:, s, :].T)
    _bits(across.mean[name], ws[:, s, :, 0].T, name)
    _bits(across.quantile[name], ws[:, s, :, 5:].transpose(2, 1, 0), name)
    assert np.array_equal(along.first[name], mf[s]) and np.array_equal(along.ncross[name], mx[s])
    _bits(along.var[name], ms[s, :, 1], name)
    _bits(along.autocov[name], ms[s, :, 6:].T, name)
