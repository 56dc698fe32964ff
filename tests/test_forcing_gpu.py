"""Time-dependent forcing on the device: pm_forcing_apply against np.interp bit for bit, an
ensemble under a ForcingSchedule against the same ensemble whose forcing the test sets from the
host (pre-existing code only), and against the reference run under the same schedule (G26)."""
import ctypes as C

import numpy as np
import pytest

import forcing_cases as FC
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _knots(K):
  return np.array([3.5, 4.0, 9.25, 9.5, 40.0])[:K] if K > 1 else np.array([2.0])


def _times(x):
  """Below the first knot, on it, between knots, on an inner knot, on the last, beyond; NaN."""
  t = [x[0] - 1.5, x[0], x[-1], x[-1] + 3.0, np.nan, np.inf]
  if x.size > 1:
    t += [0.5 * (x[0] + x[1]), np.nextafter(x[1], 0.), x[0] + 0.3 * (x[-1] - x[0])]
  if x.size > 2:
    t += [x[2], np.nextafter(x[2], 1e9)]
  return t


def _values(rng, shape):
  """Knot values of mixed magnitude and sign with equal neighbours, zeros of both signs and,
  in one column, an infinity (np.interp's NaN fallbacks)."""
  v = rng.standard_normal(shape) * 10.0**rng.integers(-8, 8, shape)
  flat = v.reshape(shape[0], -1)
  ncol = flat.shape[1]
  if shape[0] > 1:
    flat[1, ::3] = flat[0, ::3]        # f0 == f1
    flat[:, ncol // 2] = np.inf        # inf - inf: NaN slope, both fallbacks
    flat[0, ncol - 1] = -np.inf        # one infinite knot
  flat[0, 0] = -0.0
  return v


def _interp_rows(t, x, vals, per_member, n, ln):
  """[n, ln] by np.interp itself, one call per element."""
  cols = vals.reshape(x.size, -1)
  with np.errstate(invalid="ignore"):
    out = np.array([np.interp(t, x, cols[:, q]) for q in range(cols.shape[1])])
  return out.reshape(n, ln) if per_member else np.broadcast_to(out, (n, ln))


def _bits_equal(got, want, what):
  """Bit for bit, signed zeros and infinities included; a NaN must be a NaN (its payload is the
  arithmetic unit's, not np.interp's)."""
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), what
  assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), what


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 67])
def test_forcing_apply_is_np_interp_bit_for_bit(gpu, n, K):
  """8 targets in one launch: len 1 / 2 / 51 with shared and per-member values, each a row view at
  a non-zero row offset inside a larger array whose other rows must stay untouched; one per-member
  target that fills its array; one whose destination and values both start 8 bytes off a 16-byte
  boundary (the 16-byte path with a scalar head).  Every time of `_times`."""
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray, synchronize
  rng = np.random.default_rng(100 * n + K)
  x = _knots(K)
  specs = [(ln, per, row0) for ln, row0 in ((1, 3), (2, 3), (51, 2)) for per in (0, 1)]
  specs += [(51, 1, 0), (2, 1, 0)]
  f = _lib.pm_forcing()
  f.n, f.K, f.ntargets, f.knots = n, K, len(specs), x.ctypes.data
  assert f.ntargets == _lib.PM_FORCING_MAX_TARGETS
  keep = []
  for i, (ln, per, row0) in enumerate(specs):
    vals = _values(rng, (K, n, ln) if per else (K, ln))
    off = 1 if i == 7 else 0  # target 7: one double into both arrays
    rows = n if i == 6 else row0 + n + 2
    host = np.full(rows * ln + off, SENTINEL)
    dst = DeviceArray.from_host(host)
    dv = DeviceArray.from_host(np.concatenate([np.zeros(off), vals.ravel()]))
    g = f.target[i]
    g.dst, g.row0, g.values = dst.ptr + 8 * off, row0, dv.ptr + 8 * off
    g.len, g.per_member = ln, per
    keep.append((dst, dv, vals, host.size, off))
  for t in _times(x):
    for dst, _, _, size, _ in keep:
      dst.upload(np.full(size, SENTINEL))
    _lib.check(_lib.lib.pm_forcing_apply(C.byref(f), float(t), None))
    synchronize()
    for i, ((ln, per, row0), (dst, _, vals, size, off)) in enumerate(zip(specs, keep)):
      got = dst.download()
      lo, hi = off + row0 * ln, off + (row0 + n) * ln
      want = _interp_rows(t, x, vals, per, n, ln)
      _bits_equal(got[lo:hi], want.ravel(), (i, t))
      rest = np.concatenate([got[:lo], got[hi:]])
      assert np.array_equal(rest, np.full(rest.size, SENTINEL)), (i, t)


# ------------------------------------------------------------------ ensembles
def _ensemble(gpu, name, **kw):
  cls = gpu.JN2018Ensemble if name == "jn2018" else gpu.TwoColEnsemble
  _, cfg, t, values = FC.case(name)
  return cls, cfg, t, values, kw


def _host_set(ens, name, cfg, t, values, time):
  """The forcing of every member at `time`, by np.interp on the host, uploaded with the arrays'
  own pre-existing setters (a target the schedule leaves out keeps the cfg's value)."""
  n = ens.n
  v = [FC.member_values(values, t, time, j) for j in range(n)]
  col = lambda k: np.array([m[k] for m in v])  # noqa: E731
  north = col("bs_north") if "bs_north" in values else type(ens).read(cfg, "bs_north", n)
  ens.cols.bs.upload(np.concatenate([col("bs"), north]), ens.stream)
  if name == "twocol_so":
    ens.so.set_tau(col("tau"))
    ens.bs_SO.upload(col("bs_SO"), ens.stream)
  if name == "jn2018":
    ens.so.set_tau(col("tau"))
    ens.ml.b_rest.upload(col("b_rest"), ens.stream)
    ens.ml.surflux.upload(col("surflux"), ens.stream)


def _same(sa, sb, what):
  assert set(sa) == set(sb)
  for k in sa:
    assert np.array_equal(sa[k].view(np.uint64), sb[k].view(np.uint64)), (what, k)


@pytest.mark.parametrize("name,kw", [("twocol", {}), ("twocol_so", {}), ("jn2018", dict(fused=True)),
                                     ("jn2018", dict(fused=False))])
def test_schedule_equals_forcing_set_from_the_host(gpu, name, kw):
  """A: built with forcing=.  B: built without; the test uploads np.interp(s * dt, ...) ahead of
  every interval and runs to the next application step.  Bitwise equal after 5 intervals and a
  part of the sixth; one run() equals the same run split at a non-restart step (and, for JN2018,
  with moc_update() called ahead of run())."""
  cls, cfg, t, values, kw = _ensemble(gpu, name, **kw)
  M, phase = int(cfg["MOC_up_iters"]), cls.RESTART_PHASE
  total = 5 * M + phase + 3
  apps = [s for s in range(total) if FC.applied_at(s, M, phase)]
  sched = gpu.ForcingSchedule(t, **values)
  a = cls(cfg, forcing=sched, **kw)
  a.run(total)
  b = cls(cfg, **kw)
  for s, nxt in zip(apps, apps[1:] + [total]):
    assert b.ii == s
    _host_set(b, name, cfg, t, values, s * b.dt)
    b.run(nxt - s)
  sa = a.state()
  _same(sa, b.state(), "host-set")
  unforced = cls(cfg, **kw)
  unforced.run(total)
  assert not np.array_equal(sa["b_basin"], unforced.state()["b_basin"])  # the schedule acts
  c = cls(cfg, forcing=sched, **kw)
  if name == "jn2018":
    c.moc_update()
  c.run(2 * M + phase + 2)  # ends inside an interval, not on a restart step
  assert not FC.applied_at(c.ii, M, phase)
  if name == "jn2018":
    c.run(M - c.ii % M)  # on to a MOC step
    c.moc_update()
  c.run(total - c.ii)
  _same(sa, c.state(), "split")


@pytest.mark.parametrize("name", FC.CASES)
def test_schedule_against_the_reference(gpu, name):
  """G26: the reference's classes in the scripts' loops with np.interp assignments at the loop
  tops the rule names -- within the bound of the driver's own golden test."""
  cls, cfg, t, values, _ = _ensemble(gpu, name)
  g = load_golden("forcing")
  ens = cls(cfg, forcing=gpu.ForcingSchedule(t, **values))
  done = 0
  for s in FC.SNAPS:
    ens.run(s - done)
    done = s
    st = ens.state()
    for k in FC.FIELDS[name]:
      ref = g["%s_s%03d_%s" % (name, s, k)]
      for j in range(FC.N):
        err = relerr(st[k][j], ref[j])
        print(name, s, k, j, "relerr %.3e" % err)
        assert err <= FC.TOL[name], (s, k, j, err)


@pytest.mark.parametrize("name", FC.CASES)
def test_constant_schedule_equals_the_unforced_ensemble(gpu, name):
  """Knot values that repeat the cfg's forcing at every knot: bitwise the ensemble without a
  schedule."""
  cls, cfg, t, values, _ = _ensemble(gpu, name)
  n, K = FC.N, t.size
  rd = lambda key: cls.read(cfg, key, n)  # noqa: E731
  const = dict(bs=np.tile(rd("bs"), (K, 1)), bs_north=np.full(K, float(np.asarray(cfg["bs_north"]))))
  if name == "twocol_so":
    const.update(tau=np.tile(rd("tau"), (K, 1)), bs_SO=np.tile(rd("bs_SO"), (K, 1, 1)))
  if name == "jn2018":
    const.update(tau=np.tile(rd("tau"), (K, 1)), b_rest=np.tile(rd("b_rest"), (K, 1, 1)),
                 surflux=np.tile(rd("surflux")[0], (K, 1)))
  a = cls(cfg, forcing=gpu.ForcingSchedule(t, **const))
  b = cls(cfg)
  steps = 3 * int(cfg["MOC_up_iters"]) + 2
  a.run(steps)
  b.run(steps)
  assert a._forced_at > 0
  _same(a.state(), b.state(), "constant")
