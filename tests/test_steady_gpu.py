"""GPU checks of the run to steady state: pm_steady_check against a NumPy model (bitwise), and
run_to_steady on JN2018Ensemble / TwoColEnsemble against plain runs of the same members."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

YEAR = 360 * 86400.


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and np.array_equal(_bits(a), _bits(b.astype(a.dtype)))


# ------------------------------------------------------------------------------------ kernel

def _model(drift_src, snap, cap_src, cap, orig, tol, streak, status, drift_out, step_out,
           consecutive, finalize, step, scale):
  """pm_steady_check in NumPy (arrays updated in place); returns the running count."""
  running = 0
  for m, k in enumerate(orig):
    if status[k] != 0:
      continue
    cur = np.concatenate([s[m] for s in drift_src])
    ref = np.concatenate([s[m] for s in snap])
    bad = not (np.isfinite(cur).all() and np.isfinite(ref).all())
    with np.errstate(invalid="ignore"):
      d = np.max(np.abs(cur - ref)) * scale
    for s, src in zip(snap, drift_src):
      s[m] = src[m]
    if bad:
      status[k], drift_out[k] = 2, np.nan
    else:
      drift_out[k] = d
      streak[k] = streak[k] + 1 if d <= tol[k] else 0
      status[k] = 1 if streak[k] >= consecutive else (3 if finalize else 0)
    if status[k]:
      for c, src in zip(cap, cap_src):
        c[k] = src[m]
      step_out[k] = step
    else:
      running += 1
  return running


def test_steady_check_kernel_matches_numpy_bitwise(gpu):
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray
  rng = np.random.default_rng(2024)
  n0, n = 45, 37
  orig = rng.permutation(n0)[:n].astype(np.int32)
  dlens, dstrides = [81, 7, 130], [96, 7, 131]
  clens, cstrides = dlens + [64, 3], dstrides + [70, 5]
  # live state: strided rows; snapshot: dense rows close to it
  srcs = [rng.normal(size=(n, st)) * 1e-2 for st in cstrides]
  snaps = [s[:, :ln] + rng.normal(size=(n, ln)) * 10.0**rng.integers(-12, -4, size=(n, 1))
           for s, ln in zip(srcs, dlens)]
  for m in range(n):  # rows identical to the snapshot: drift exactly 0
    if m % 11 == 3:
      for s, sn, ln in zip(srcs, snaps, dlens):
        sn[m] = s[m, :ln]
  srcs[0][2, 40] = np.nan
  srcs[1][5, 6] = np.inf
  snaps[2][9, 129] = -np.inf
  srcs[2][13, 0] = np.nan  # and in a row whose member has already retired (below)
  status = np.zeros(n0, np.int32)
  status[orig[13]] = 1
  status[orig[[20, 21]]] = [3, 2]
  streak = rng.integers(0, 2, n0).astype(np.int32)
  drift_out = rng.normal(size=n0)
  step_out = rng.integers(0, 1000, n0).astype(np.int64)
  caps = [np.full((n0, ln), -7.25) for ln in clens]
  scale = YEAR / (120 * 30 * 86400.)
  # tolerances around the model's drift: equal (converges, `<=`), just below, far above
  dsrc = [s[:, :ln] for s, ln in zip(srcs, dlens)]
  d = np.array([np.max(np.abs(np.concatenate([s[m] for s in dsrc]) -
                              np.concatenate([s[m] for s in snaps]))) * scale for m in range(n)])
  tol = np.full(n0, 1e-30)
  for m, k in enumerate(orig):
    tol[k] = [d[m], np.nextafter(d[m], -1.), 1e3][m % 3] if np.isfinite(d[m]) else 1.

  dev = dict(orig=DeviceArray.from_host(orig), tol=DeviceArray.from_host(tol),
             streak=DeviceArray.from_host(streak), status=DeviceArray.from_host(status),
             drift=DeviceArray.from_host(drift_out), step=DeviceArray.from_host(step_out,
                                                                                   dtype=np.int64),
             nrun=DeviceArray.zeros((1,), np.int32))
  dsrcs = [DeviceArray.from_host(s) for s in srcs]
  dsnaps = [DeviceArray.from_host(s) for s in snaps]
  dcaps = [DeviceArray.from_host(c) for c in caps]

  def launch(step, finalize, consecutive):
    c = _lib.pm_steady_check()
    c.n, c.n0, c.ndrift, c.ncapture = n, n0, len(dlens), len(clens)
    c.consecutive, c.finalize, c.step, c.scale = consecutive, finalize, step, scale
    c.orig, c.tol, c.streak, c.status = (dev["orig"].ptr, dev["tol"].ptr, dev["streak"].ptr,
                                         dev["status"].ptr)
    c.drift_out, c.step_out, c.n_running = dev["drift"].ptr, dev["step"].ptr, dev["nrun"].ptr
    for i in range(len(dlens)):
      c.drift[i].src, c.drift[i].src_stride = dsrcs[i].ptr, dstrides[i]
      c.drift[i].buf, c.drift[i].len = dsnaps[i].ptr, dlens[i]
    for i in range(len(clens)):
      c.capture[i].src, c.capture[i].src_stride = dsrcs[i].ptr, cstrides[i]
      c.capture[i].buf, c.capture[i].len = dcaps[i].ptr, clens[i]
    _lib.check(_lib.lib.pm_steady_check(C.byref(c), None))
    return int(dev["nrun"].download()[0])

  def compare(nrun_dev, nrun_ref):
    assert nrun_dev == nrun_ref
    assert _same(dev["status"].download(), status)
    assert _same(dev["streak"].download(), streak)
    assert _same(dev["drift"].download(), drift_out)
    assert _same(dev["step"].download(), step_out)
    for a, b in zip(dsnaps, snaps):
      assert _same(a.download(), b)
    for a, b in zip(dcaps, caps):
      assert _same(a.download(), b)

  # check 1: consecutive = 2 -- members with streak 1 and drift <= tol converge
  model_args = lambda: (dsrc, snaps, [s[:, :ln] for s, ln in zip(srcs, clens)], caps,  # noqa
                        orig, tol, streak, status, drift_out, step_out)
  ref = _model(*model_args(), 2, 0, 120, scale)
  compare(launch(120, 0, 2), ref)
  assert set(status.tolist()) == {0, 1, 2, 3} and 0 < ref < n
  assert (status[orig[[2, 5, 9]]] == 2).all() and status[orig[13]] == 1
  # check 2: a second look at an unchanged state (drift 0 for every running member) with a
  # fresh live state for some rows, then the finalizing check
  for s in srcs:
    s[::4] += 1e-9
  for a, s in zip(dsrcs, srcs):
    a.upload(s)
  dsrc = [s[:, :ln] for s, ln in zip(srcs, dlens)]
  ref = _model(*model_args(), 2, 0, 240, scale)
  compare(launch(240, 0, 2), ref)
  ref = _model(*model_args(), 2, 1, 360, scale)
  compare(launch(360, 1, 2), ref)
  assert ref == 0 and not (status[orig] == 0).any()  # members without a row stay running
  # every member retired: a further check touches nothing and counts nobody
  compare(launch(480, 1, 2), 0)


# ------------------------------------------------------------------------------ drivers

def _plain_series(cls, cfg, s0, checks):
  """A plain run of `cfg` stepped to s0 and every check step: the drift fields' rows and the
  overturning of the update at that step."""
  import pymoc_amd
  ens = cls(cfg)
  jn = cls is pymoc_amd.JN2018Ensemble
  out = []
  for s in [s0] + list(checks):
    ens.run(s - ens.ii)
    if jn:
      ens.moc_update()
    st = ens.state()
    rec = dict(b_basin=st["b_basin"], b_north=st["b_north"], Psi=st["Psi"])
    if jn:
      rec["bs_SO"] = st["bs_SO"]
    if "Psi_SO" in st:
      rec["Psi_SO"] = st["Psi_SO"]
    out.append(rec)
  return out


def _expected(series, drift_names, checks, s0, dt, tol, consecutive):
  """Per member: (status, retirement check index, drift) of the NumPy model of the run."""
  n = series[0]["b_basin"].shape[0]
  status, jret = np.zeros(n, np.int32), np.full(n, -1)
  drift, streak = np.zeros(n), np.zeros(n, np.int64)
  steps = [s0] + list(checks)
  for j in range(1, len(steps)):
    scale = YEAR / ((steps[j] - steps[j - 1]) * dt)
    for k in range(n):
      if status[k]:
        continue
      cur = np.concatenate([series[j][f][k] for f in drift_names])
      ref = np.concatenate([series[j - 1][f][k] for f in drift_names])
      if not (np.isfinite(cur).all() and np.isfinite(ref).all()):
        status[k], jret[k], drift[k] = 2, j, np.nan
        continue
      drift[k] = np.max(np.abs(cur - ref)) * scale
      streak[k] = streak[k] + 1 if drift[k] <= tol[k] else 0
      if streak[k] >= consecutive:
        status[k], jret[k] = 1, j
      elif j == len(steps) - 1:
        status[k], jret[k] = 3, j
  return status, jret, drift


def _drift_series(series, drift_names, steps, dt):
  n = series[0]["b_basin"].shape[0]
  D = np.zeros((len(steps) - 1, n))
  for j in range(1, len(steps)):
    cur = np.concatenate([series[j][f] for f in drift_names], axis=1)
    ref = np.concatenate([series[j - 1][f] for f in drift_names], axis=1)
    with np.errstate(invalid="ignore"):
      D[j - 1] = np.max(np.abs(cur - ref), axis=1) * YEAR / ((steps[j] - steps[j - 1]) * dt)
  return D


def _check_driver(cls, cfg, drift_names, capture_names, check_every, max_steps, consecutive):
  import pymoc_amd
  from pymoc_amd.steady import check_schedule, restrict_cfg
  n = np.atleast_2d(cfg["b_basin0"]).shape[0]
  M, dt = int(cfg["MOC_up_iters"]), float(cfg["dt"])
  s0, checks = check_schedule(cls, M, check_every, max_steps)
  steps = [s0] + checks
  series = _plain_series(cls, cfg, s0, checks)
  D = _drift_series(series, drift_names, steps, dt)
  assert np.isfinite(D).all()
  # tolerances from the plain run's drift: retirements spread over many checks, some capped
  tol = np.empty(n)
  for k in range(n):
    t = 2 + (k * 5) % (len(checks) - 2)
    tol[k] = 0. if k % 6 == 1 else D[t, k]
  # one more member: a copy of member 0 with a NaN in its initial profile
  big = restrict_cfg(cls, cfg, np.r_[np.arange(n), 0])
  b0 = np.array(big["b_basin0"], dtype=np.float64)
  b0[n, cfg["z"].size // 2] = np.nan
  big["b_basin0"] = b0
  tol_big = np.r_[tol, 1.]
  status, jret, drift = _expected(series, drift_names, checks, s0, dt, tol, consecutive)
  assert (status == 1).sum() >= 3 and (status == 3).any()
  assert len(set(jret[status == 1].tolist())) >= 3

  runs = [pymoc_amd.run_to_steady(cls, big, tol_big, max_steps, check_every=check_every,
                                  consecutive=consecutive, compact_below=cb) for cb in (0., 1.)]
  never, always = runs
  assert never.compactions == [] and len(always.compactions) >= 2
  for a, b in zip(always.compactions, always.compactions[1:]):
    assert a[2] == b[1] and a[2] < a[1]
  assert _same(never.status, always.status) and _same(never.steps, always.steps)
  assert _same(never.drift, always.drift)
  assert set(never.fields) == set(capture_names) == set(always.fields)
  for f in capture_names:
    assert _same(never.fields[f], always.fields[f]), f
  assert always.member_steps < never.member_steps <= (n + 1) * max_steps
  for res in runs:
    # the NaN member retires at the first check; nobody else is affected
    assert res.status[n] == 2 and res.steps[n] == checks[0] and np.isnan(res.drift[n])
    assert _same(res.status[:n], status)
    assert _same(res.steps[:n], np.array([steps[j] for j in jret], np.int64))
    assert _same(res.drift[:n], drift)
    for k in range(n):
      rec = series[jret[k]]
      for f in capture_names:
        assert _same(res.fields[f][k], rec[f][k]), (f, k, jret[k])
    assert (res.years[:n] == res.steps[:n] * dt / YEAR).all()
  assert always.member_steps < n * max_steps
  return never


def test_run_to_steady_jn2018(gpu):
  from pymoc_amd import JN2018Ensemble, configs
  cfg = configs.config5(N=64, nz=81, dt_days=30.)
  _check_driver(JN2018Ensemble, cfg, ["b_basin", "b_north", "bs_SO"],
                ["b_basin", "b_north", "bs_SO", "Psi", "Psi_SO"], 120, 3600, 1)


def test_run_to_steady_twocol(gpu):
  from pymoc_amd import TwoColEnsemble, configs
  _check_driver(TwoColEnsemble, configs.config3(N=64), ["b_basin", "b_north"],
                ["b_basin", "b_north", "Psi"], 240, 2401, 2)


def test_run_to_steady_twocol_so(gpu):
  from pymoc_amd import TwoColEnsemble, configs
  _check_driver(TwoColEnsemble, configs.config4(N=32), ["b_basin", "b_north"],
                ["b_basin", "b_north", "Psi", "Psi_SO"], 240, 2401, 1)


def test_jn2018_equilibrium_example_runs(gpu, tmp_path):
  out = tmp_path / "eq.npz"
  p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "jn2018_equilibrium.py"),
                      "--members", "24", "--years", "150", "--tol", "1e-4", "--out", str(out)],
                     cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert p.returncode == 0, p.stdout + p.stderr
  assert "converged" in p.stdout and "max AMOC" in p.stdout
  z = np.load(out)
  assert z["status"].shape == (24,) and set(np.unique(z["status"])) <= {1, 2, 3}
  assert z["Psi"].shape == (24, 81)


# ---------------------------------------------------------------- the base class's protocol

# The config builders take any nz, so the grids are the smallest ones this suite runs each driver
# on elsewhere (test_fused_run_gpu.py: config 3 at nz = 65, config 5 at nz = 46 with dt = 30 d;
# config 4's channel solve at nz = 100): the checks below are about how a cfg is read and where a
# run restarts, not about kernel shapes nothing else vouches for.
def _case(name, N):
  from pymoc_amd import JN2018Ensemble, TwoColEnsemble, configs
  if name == "config3":
    return TwoColEnsemble, configs.config3(N=N, nz=65)
  if name == "config4":
    return TwoColEnsemble, configs.config4(N=N, nz=100)
  return JN2018Ensemble, configs.config5(N=N, nz=46, dt_days=30)


_CASE_NZ = {"config3": 65, "config4": 100, "config5": 46}


@pytest.mark.parametrize("shape", ["n3", "n_is_nz"])
@pytest.mark.parametrize("name", ["config3", "config4", "config5"])
def test_constructor_reads_member_keys_like_read(gpu, name, shape):
  """An ensemble built from a cfg as its builder returns it, and one from a cfg whose MEMBER_KEYS
  entries are replaced by `cls.read(cfg, key, n)`, are bitwise equal after one MOC interval.  At
  N == nz a 1-D per-member array and a profile have the same shape: a constructor that read a key
  by another rule than `read` would diverge there."""
  N = 3 if shape == "n3" else _CASE_NZ[name]
  cls, cfg = _case(name, N)
  assert cls.members(cfg) == N
  explicit = dict(cfg)
  for key in cls.MEMBER_KEYS:
    if key in cfg:
      explicit[key] = cls.read(cfg, key, N)
      assert explicit[key].shape[0] == N
  a, b = cls(cfg), cls(explicit)
  for e in (a, b):
    e.run(cls.RESTART_PHASE + e.M)
  sa, sb = a.state(), b.state()
  assert list(sa) == list(sb)
  for f in sa:
    assert _same(sa[f], sb[f]), f
  assert np.array_equal(a.nonfinite_members(), b.nonfinite_members())


@pytest.mark.parametrize("name", ["config3", "config4", "config5"])
def test_subset_continues_bit_identically(gpu, name):
  """`subset` at a restart point: members 0, 2, 4 on their own continue bitwise as they do inside
  the full ensemble, in every field of state()."""
  cls, cfg = _case(name, 5)
  keep = [0, 2, 4]
  full = cls(cfg)
  full.run(cls.RESTART_PHASE + 2 * full.M)
  full.at_restart_point()
  sub = full.subset(keep, cfg, {})
  assert type(sub) is cls and sub.n == 3 and sub.ii == full.ii
  for e in (full, sub):
    e.run(2 * e.M)
  sf, ss = full.state(), sub.state()
  assert list(sf) == list(ss)
  for f in sf:
    assert _same(sf[f][keep], ss[f]), f
