"""Stochastic forcing on the device: pm_forcing_noise against the NumPy restatement
(tests/noise_cases.py) through the C-ABI -- the deviates to their bound, the AR(1) and store stages
bit for bit given the deviates the launch stored, guards intact -- and ensembles under a
NoiseForcing against the restated series and against a twin whose forcing arrays the test sets from
the host (pre-existing code only)."""
import ctypes as C

import numpy as np
import pytest

import forcing_cases as FC
import noise_cases as NC
import test_noise_cpu as TC

pytestmark = pytest.mark.gpu

PAD = 3  # guard elements on either side of a state buffer, guard rows around a destination


def _bits(got, want, what):
  assert got.shape == want.shape, what
  assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


# ------------------------------------------------------------------ C-ABI cases
class _Guarded(object):
  """A device array whose inner [lo, lo + size) is `inner` (or NaN) between NaN guards."""

  def __init__(self, size, inner=None, lo=PAD, hi=PAD):
    from pymoc_amd.device import DeviceArray
    host = np.full(lo + size + hi, np.nan)
    if inner is not None:
      host[lo:lo + size] = np.asarray(inner, dtype=np.float64).ravel()
    self.lo, self.size, self.host0 = lo, size, host
    self.dev = DeviceArray.from_host(host)
    self.ptr = self.dev.ptr + 8 * lo

  def read(self):
    """The inner part, after asserting that the guards are still NaN."""
    got = self.dev.download()
    assert np.isnan(got[:self.lo]).all() and np.isnan(got[self.lo + self.size:]).all()
    return got[self.lo:self.lo + self.size]

  def untouched(self):
    return np.array_equal(self.dev.download(), self.host0, equal_nan=True)


def _spec(rng, n, ln, stream, a=0.625, b=0.75, row0=2, pattern="none", sigma=None, share=None,
          outputs=True):
  """The host side of one descriptor entry."""
  if pattern == "shared":
    pat = rng.standard_normal(ln)
    pat[0], pat[-1] = 0.0, -abs(pat[-1]) - 0.5  # a zero and a negative entry
  elif pattern == "member":
    pat = rng.standard_normal((n, ln))
    pat[0, 0], pat[-1, -1] = 0.0, -1.5
  else:
    pat = None
  return dict(len=ln, stream=stream, a=a, b=b, row0=row0, pattern=pat, share=share,
              outputs=outputs, sigma=rng.uniform(0.5, 2.0, n) if sigma is None else sigma,
              x_in=rng.standard_normal(n), base=rng.standard_normal((n, ln)) * 10.0)


def _launch(n, specs, seed=2018, member0=0, j=3):
  """One launch of pm_forcing_noise on guarded arrays; returns per entry
  dict(dst [n, len], x_out [n] or None, xi [n] or None) after checking every guard."""
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray, synchronize
  f = _lib.pm_noise()
  f.n, f.ntargets, f.j, f.seed, f.member0 = n, len(specs), j, seed, member0
  bufs = []
  for g, s in zip(f.target, specs):
    ln = s["len"]
    b = dict(dst=_Guarded(n * ln, lo=s["row0"] * ln, hi=2 * ln),
             base=DeviceArray.from_host(s["base"]), sigma=DeviceArray.from_host(s["sigma"]),
             x_in=(bufs[s["share"]]["x_in"] if s["share"] is not None
                   else _Guarded(n, s["x_in"])),
             x_out=_Guarded(n) if s["outputs"] else None,
             xi=_Guarded(n) if s["outputs"] else None,
             pattern=None if s["pattern"] is None else DeviceArray.from_host(s["pattern"]))
    bufs.append(b)
    g.dst, g.row0, g.base, g.sigma = b["dst"].dev.ptr, s["row0"], b["base"].ptr, b["sigma"].ptr
    g.x_in = b["x_in"].ptr
    g.x_out = b["x_out"].ptr if s["outputs"] else None
    g.xi_out = b["xi"].ptr if s["outputs"] else None
    g.pattern = None if b["pattern"] is None else b["pattern"].ptr
    g.a, g.b, g.len, g.stream = s["a"], s["b"], ln, s["stream"]
    g.pattern_per_member = int(s["pattern"] is not None and s["pattern"].ndim == 2)
  _lib.check(_lib.lib.pm_forcing_noise(C.byref(f), None))
  synchronize()
  out = []
  for s, b in zip(specs, bufs):
    if s["share"] is None:
      assert np.array_equal(b["x_in"].read(), s["x_in"])  # the input is not written
    out.append(dict(dst=b["dst"].read().reshape(n, s["len"]),
                    x_out=b["x_out"].read() if s["outputs"] else None,
                    xi=b["xi"].read() if s["outputs"] else None))
  return out


def _xi_ratio(xi, seed, ids, j, stream):
  """max |xi - restatement| / (16 * 2^-53 * R); R == 0 must be equal under ==."""
  ref, R = NC.deviate(seed, ids, j, stream)
  zero = R == 0
  assert np.array_equal(xi[zero], ref[zero])
  if zero.all():
    return 0.0
  return float(np.max(np.abs(xi - ref)[~zero] / (16.0 * NC.EPS * R[~zero])))


def _check_entry(s, r, x_out, xi, n, seed, member0, j, what):
  """The deviates to the bound, the two identities bit for bit.  x_out / xi: this entry's, or
  those of the entry it shares its state with."""
  ids = np.uint64(member0) + np.arange(n, dtype=np.uint64)
  ratio = _xi_ratio(xi, seed, ids, j, s["stream"])
  assert ratio <= 1.0, (what, ratio)
  _bits(x_out, s["a"] * s["x_in"] + (s["sigma"] * s["b"]) * xi, what)
  _bits(r["dst"], NC.written(s["base"], x_out, s["pattern"]), what)
  return ratio


@pytest.mark.parametrize("ln", [1, 2, 51])
@pytest.mark.parametrize("n", [1, 3, 67, 130])
def test_layout_deviates_and_identities(gpu, n, ln):
  """Three entries of one row length in a launch -- no pattern, a shared and a per-member pattern
  (each with a zero and a negative entry) -- as row views at a non-zero row0 inside NaN arrays,
  the state buffers between NaN guards."""
  rng = np.random.default_rng(1000 * n + ln)
  specs = [_spec(rng, n, ln, 0), _spec(rng, n, ln, 3, pattern="shared", row0=1),
           _spec(rng, n, ln, 5, pattern="member", row0=4)]
  res = _launch(n, specs, seed=2018, member0=7, j=3)
  worst = max(_check_entry(s, r, r["x_out"], r["xi"], n, 2018, 7, 3, (n, ln, k))
              for k, (s, r) in enumerate(zip(specs, res)))
  print("n %d len %d: largest |xi - restatement| / bound %.3f" % (n, ln, worst))
  assert not np.array_equal(res[0]["xi"], res[1]["xi"])  # another stream: other deviates


def test_deviates_do_not_depend_on_the_batch_the_shard_or_the_other_targets(gpu):
  rng = np.random.default_rng(5)
  whole = _launch(5, [_spec(rng, 5, 2, 2)], member0=0)[0]["xi"]
  parts = [_launch(3, [_spec(rng, 3, 2, 2)], member0=0)[0]["xi"],
           _launch(2, [_spec(rng, 2, 2, 2)], member0=3)[0]["xi"]]
  _bits(np.concatenate(parts), whole, "one launch of 5 against 3 + 2")
  # the same target (stream 2) alone and as the sixth of 8 entries of other lengths and streams
  others = [_spec(rng, 5, ln, st) for ln, st in ((1, 0), (51, 1), (2, 3), (1, 4), (51, 5))]
  among = _launch(5, others + [_spec(rng, 5, 2, 2)] + [_spec(rng, 5, 3, 0), _spec(rng, 5, 1, 1)])
  assert len(among) == 8
  _bits(among[5]["xi"], whole, "alone against among 8")
  # ids above 2^32: the high word counts
  m0 = 2**32 - 2
  high = _launch(5, [_spec(rng, 5, 2, 2)], member0=m0)[0]["xi"]
  parts = [_launch(2, [_spec(rng, 2, 2, 2)], member0=m0)[0]["xi"],
           _launch(3, [_spec(rng, 3, 2, 2)], member0=2**32)[0]["xi"]]
  _bits(np.concatenate(parts), high, "across 2^32")
  assert _xi_ratio(high, 2018, np.uint64(m0) + np.arange(5, dtype=np.uint64), 3, 2) <= 1.0
  low = _launch(3, [_spec(rng, 3, 2, 2)], member0=0)[0]["xi"]
  assert not np.array_equal(high[2:], low)  # ids 2^32 + k are not ids k
  far = _launch(3, [_spec(rng, 3, 2, 2)], member0=2**62 + 11, seed=2**64 - 1)[0]["xi"]
  assert _xi_ratio(far, 2**64 - 1, np.uint64(2**62 + 11) + np.arange(3, dtype=np.uint64), 3, 2) <= 1.0


@pytest.mark.parametrize("j", [0, 1, 2**32 - 1])
def test_edge_values(gpu, j):
  """a = 0 (white / first application), a = 1 (frozen), sigma = 0 and a mixed sigma, against every
  j; patterns with zero and negative entries, shared and per member."""
  rng = np.random.default_rng(j % 1000)
  n = 67
  some = rng.uniform(0.5, 2.0, n)
  some[::3] = 0.0
  specs = [_spec(rng, n, 2, 0, a=0.0, b=1.0, pattern="shared"),
           _spec(rng, n, 51, 1, a=1.0, b=0.0, pattern="member"),
           _spec(rng, n, 1, 2, sigma=np.zeros(n)),
           _spec(rng, n, 2, 4, a=0.0, b=1.0, sigma=np.zeros(n), pattern="shared"),
           _spec(rng, n, 1, 5, sigma=some)]
  res = _launch(n, specs, seed=0, member0=0, j=j)
  for k, (s, r) in enumerate(zip(specs, res)):
    _check_entry(s, r, r["x_out"], r["xi"], n, 0, 0, j, (j, k))
  _bits(res[1]["x_out"], 1.0 * specs[1]["x_in"] + 0.0 * res[1]["xi"], "frozen")
  assert np.array_equal(res[1]["x_out"], specs[1]["x_in"])
  assert np.array_equal(res[2]["x_out"], 0.625 * specs[2]["x_in"])   # sigma = 0: decay only
  assert np.array_equal(res[3]["x_out"], np.zeros(n))                # sigma = 0, a = 0
  assert np.array_equal(res[3]["dst"], specs[3]["base"] + 0.0 * specs[3]["pattern"])
  if j:
    other = _launch(n, specs[:1], seed=0, member0=0, j=j - 1)[0]["xi"]
    assert not np.array_equal(other, res[0]["xi"])


def test_two_destinations_share_one_state(gpu):
  """The two-basin layout: two entries of one name (same stream, same x_in), the second without
  outputs -- both destinations are written from the same x."""
  rng = np.random.default_rng(11)
  n = 67
  first = _spec(rng, n, 1, 0)
  second = dict(_spec(rng, n, 1, 0, row0=5, share=0, outputs=False), a=first["a"], b=first["b"],
                sigma=first["sigma"], x_in=first["x_in"])
  tau1 = _spec(rng, n, 51, 2, pattern="shared")
  tau2 = dict(_spec(rng, n, 51, 2, row0=0, share=2, outputs=False, pattern="shared"),
              a=tau1["a"], b=tau1["b"], sigma=tau1["sigma"], x_in=tau1["x_in"])
  specs = [first, second, tau1, tau2]
  res = _launch(n, specs)
  for k, own in ((0, 0), (1, 0), (2, 2), (3, 2)):
    _check_entry(specs[k], res[k], res[own]["x_out"], res[own]["xi"], n, 2018, 0, 3, k)


def test_every_einval_leaves_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray, synchronize
  n = 4
  outs, entries = [], []
  for i in range(8):
    b = dict(dst=_Guarded(n * 3), x_out=_Guarded(n), xi=_Guarded(n))
    outs += list(b.values())
    ins = dict(base=DeviceArray.from_host(np.ones((n, 3))), sigma=DeviceArray.from_host(np.ones(n)),
               x_in=DeviceArray.from_host(np.ones(n)))
    outs.append(ins)
    entries.append(dict(dst=b["dst"].ptr, base=ins["base"].ptr, sigma=ins["sigma"].ptr,
                        x_in=ins["x_in"].ptr, x_out=b["x_out"].ptr, xi_out=b["xi"].ptr,
                        pattern=None))
  for label, kw in TC.bad_descriptors():
    top = {k: kw.pop(k) for k in ("n", "ntargets", "member0") if k in kw}
    f = TC.fill(_lib.pm_noise(), entries, **dict(top, **kw))
    assert _lib.lib.pm_forcing_noise(C.byref(f), None) == _lib.PM_EINVAL, label
  f = TC.fill(_lib.pm_noise(), entries)
  f.target[1].x_out = f.target[0].x_in
  assert _lib.lib.pm_forcing_noise(C.byref(f), None) == _lib.PM_EINVAL
  synchronize()
  for o in outs:
    if isinstance(o, _Guarded):
      assert o.untouched()
  # and the descriptor the bad ones derive from is accepted and writes
  f = TC.fill(_lib.pm_noise(), entries)
  _lib.check(_lib.lib.pm_forcing_noise(C.byref(f), None))
  synchronize()
  assert np.isfinite(outs[0].read()).all() and np.isfinite(outs[1].read()).all()


# ------------------------------------------------------------------ driver cases
KINDS = ("twocol", "twocol_so", "jn2018", "jn2018_implicit", "twobasin")
SEED = 2018


def _kind(gpu, kind, n6=False):
  """(cls, cfg, kw, noise targets): the sizes of tests/forcing_cases.case for the first three,
  the smallest existing test shapes of JN2018ImplicitEnsemble (test_jn2018_implicit_gpu's forcing
  case) and TwoBasinSweep (test_twobasin_sweep_gpu's SMALL).  The sigmas are a percent or so of
  the cfg's values; between the kinds every target, a per-member sigma, white, red and frozen
  states and shared and per-member patterns occur."""
  from pymoc_amd import configs
  DAY = 86400.0
  if kind in FC.CASES:
    cls = gpu.JN2018Ensemble if kind == "jn2018" else gpu.TwoColEnsemble
    cfg, kw = FC.case(kind)[1], {}
  elif kind == "jn2018_implicit":
    cls, kw = gpu.JN2018ImplicitEnsemble, {}
    cfg = dict(configs.config5(N=3, nz=46, dt_days=30.), MOC_up_iters=6)
  else:
    cls, kw = gpu.TwoBasinSweep, {}
    cfg = dict(configs.config_twobasin(N=3, nz=17, ny=9), dt=DAY * 30)
  n = cls.members(cfg)
  dt, year = float(cfg["dt"]), 360 * DAY
  if kind == "twocol":
    t = dict(bs=dict(sigma=3e-4 * (1. + np.arange(n)), tau_corr=0.5 * year),
             bs_north=dict(sigma=1e-5))
  elif kind == "twocol_so":
    y = np.asarray(cfg["y"])
    pat = ((y / y[-1])**2 - 0.25)[None, :] * (1. + 0.5 * np.arange(n))[:, None]
    pat[:, 3] = 0.0
    t = dict(bs=dict(sigma=3e-4), tau=dict(sigma=2e-3, tau_corr=2 * year),
             bs_SO=dict(sigma=2e-4, tau_corr=np.inf, pattern=pat))
  elif kind == "jn2018":
    y = np.asarray(cfg["y"])
    pat = np.cos(np.pi * y / y[-1])
    pat[0] = 0.0
    t = dict(bs_north=dict(sigma=2e-5, tau_corr=3 * dt), tau=dict(sigma=2e-3 * (1. + np.arange(n))),
             b_rest=dict(sigma=1e-4, tau_corr=10 * dt, pattern=pat),
             surflux=dict(sigma=0.01 * float(np.abs(cfg["surflux"]).max())))
  elif kind == "jn2018_implicit":
    t = dict(tau=dict(sigma=2e-3, tau_corr=4 * dt), bs_north=dict(sigma=2e-5), bs=dict(sigma=1e-4))
  else:
    y = np.asarray(cfg["y"])
    t = dict(bs=dict(sigma=2e-4), tau=dict(sigma=2e-3 * (1. + np.arange(n)), tau_corr=30 * dt),
             bs_north=dict(sigma=1e-5, tau_corr=np.inf),
             bs_SO=dict(sigma=1e-4, tau_corr=10 * dt, pattern=(y / y[-1]) - 0.5))
  return cls, cfg, kw, t


def _apps(cls, cfg, total):
  M, phase = int(cfg["MOC_up_iters"]), cls.RESTART_PHASE
  return [s for s in range(total) if FC.applied_at(s, M, phase)]


def _total(cls, cfg):
  return 3 * int(cfg["MOC_up_iters"]) + cls.RESTART_PHASE + 2


def _dests(ens, name):
  """[(DeviceArray, first row, row length)] of a target, off the driver's FORCING_TARGETS."""
  ln = type(ens).forcing_lengths(ens._cfg_for_tests, ens.n)[name]
  out = []
  for path, group, _ in ens.FORCING_TARGETS[name]:
    a = ens
    for attr in path.split("."):
      a = getattr(a, attr)
    out.append((a, group * ens.n, ln))
  return out


def _read(ens, name):
  """The target's current values [n, len], off every destination (they must agree)."""
  vals = []
  for a, row0, ln in _dests(ens, name):
    vals.append(a.download(stream=ens.stream).reshape(-1, ln)[row0:row0 + ens.n].copy())
  for v in vals[1:]:
    _bits(v, vals[0], name)
  return vals[0]


def _host_set(ens, name, values):
  """Upload [n, len] into every destination of a target with the arrays' own uploads."""
  for a, row0, ln in _dests(ens, name):
    full = a.download(stream=ens.stream)
    full.reshape(-1, ln)[row0:row0 + ens.n] = values
    a.upload(full, ens.stream)


def _build(cls, cfg, kw, **more):
  ens = cls(cfg, **dict(kw, **more))
  ens._cfg_for_tests = cfg
  return ens


def _same(sa, sb, what):
  assert set(sa) == set(sb)
  for k in sa:
    assert np.array_equal(sa[k].view(np.uint64), sb[k].view(np.uint64)), (what, k)


def _run_recording(ens, names, total):
  """Run to `total` one application interval at a time; {name: [values written at application j]}
  and the noise states [{name: x}] after every application."""
  apps = _apps(type(ens), ens._cfg_for_tests, total)
  written, states = {k: [] for k in names}, []
  for s, nxt in zip(apps, apps[1:] + [total]):
    assert ens.ii == s
    ens.run(nxt - s)
    for k in names:
      written[k].append(_read(ens, k))
    if ens.noise is not None:
      states.append(ens.noise.get_state())
  return apps, written, states


def _restated(cls, cfg, targets, name, ids, apps, x0=None):
  spec = targets[name]
  return NC.series(SEED, name, spec["sigma"], spec.get("tau_corr", 0.0), ids, apps,
                   int(cfg["MOC_up_iters"]), cls.RESTART_PHASE, float(cfg["dt"]), x0=x0)


def _check_series(cls, cfg, targets, name, apps, written, states, base, ids=None, what=""):
  """The state series within E_j of the restatement; the written values bit for bit
  base + x * pattern of the device's own x, and within E_j max|pattern| + 2 * 2^-53 max|value|
  of the restated values (a state that differs in its last bits can move the rounding of the sum
  at the base's magnitude by one ulp of the value; where base and pattern leave x as it is, that
  term is below E_j's own 4 X*)."""
  n = cls.members(cfg)
  ids = np.arange(n) if ids is None else ids
  x_ref, R = _restated(cls, cfg, targets, name, ids, apps)
  sigma = float(np.max(targets[name]["sigma"]))
  pattern = targets[name].get("pattern")
  pmax = 1.0 if pattern is None else float(np.abs(pattern).max())
  Rmax, Xmax = float(R.max()), float(np.abs(x_ref).max())
  worst = 0.0
  for j in range(len(apps)):
    E = NC.series_bound(j, sigma, Rmax, Xmax)
    x_dev = states[j][name]
    err = float(np.abs(x_dev - x_ref[j]).max())
    worst = max(worst, err / E)
    assert err <= E, (what, name, j, err, E)
    base_j = base[j] if isinstance(base, list) else base
    _bits(written[name][j], NC.written(base_j, x_dev, pattern), (what, name, j))
    want = NC.written(base_j, x_ref[j], pattern)
    werr = float(np.abs(written[name][j] - want).max())
    assert werr <= E * pmax + 2.0 * NC.EPS * float(np.abs(want).max()), (what, name, j, werr)
  print("%s %s: largest |x - restatement| / E_j %.3f over %d applications"
        % (what, name, worst, len(apps)))
  assert Xmax > 0 or sigma == 0
  return worst


@pytest.mark.parametrize("kind", KINDS)
def test_zero_sigma_noise_is_the_ensemble_without_noise(gpu, kind):
  cls, cfg, kw, targets = _kind(gpu, kind)
  zero = {k: dict(v, sigma=0.0) for k, v in targets.items()}
  total = _total(cls, cfg)
  a = _build(cls, cfg, kw, noise=gpu.NoiseForcing(SEED, **zero))
  b = _build(cls, cfg, kw)
  a.run(total)
  b.run(total)
  assert a._forced_at > 0 and a.noise is not None and b.noise is None
  _same(a.state(), b.state(), kind)


@pytest.mark.parametrize("kind", KINDS)
def test_noise_against_the_restatement_and_the_host_set_twin(gpu, kind):
  """A: built with noise=, run one application interval at a time; the values every application
  wrote and the noise states are downloaded.  B: built without; the test uploads A's values ahead
  of every interval.  C: A's run in one call."""
  cls, cfg, kw, targets = _kind(gpu, kind)
  n, total = cls.members(cfg), _total(cls, cfg)
  noise = gpu.NoiseForcing(SEED, **targets)
  a = _build(cls, cfg, kw, noise=noise)
  base = {k: _read(a, k) for k in targets}  # the cfg's values: nothing is applied yet
  for k in targets:
    _bits(base[k], np.asarray(cls.read(cfg, k, n), dtype=np.float64).reshape(n, -1), k)
  apps, written, states = _run_recording(a, list(targets), total)
  assert len(apps) >= 4
  for k in targets:
    _check_series(cls, cfg, targets, k, apps, written, states, base[k], what=kind)
  b = _build(cls, cfg, kw)
  for j, (s, nxt) in enumerate(zip(apps, apps[1:] + [total])):
    assert b.ii == s
    for k in targets:
      _host_set(b, k, written[k][j])
    b.run(nxt - s)
  sa = a.state()
  _same(sa, b.state(), (kind, "host-set"))
  c = _build(cls, cfg, kw, noise=noise)
  c.run(total)
  _same(sa, c.state(), (kind, "one run"))
  plain = _build(cls, cfg, kw)
  plain.run(total)
  assert not np.array_equal(sa["b_north"], plain.state()["b_north"])  # the noise acts


def test_noise_on_top_of_a_schedule(gpu):
  """twocol_so under FC's schedule of bs, tau and bs_SO with noise on tau (shared with the
  schedule), bs_SO (shared, with a pattern) and bs_north (the noise's alone): a shared target is
  the restated np.interp base + x * pattern, the schedule's other target is np.interp bit for
  bit."""
  cls, cfg, kw, targets = _kind(gpu, "twocol_so")
  _, _, t, values = FC.case("twocol_so")
  targets = dict(tau=targets["tau"], bs_SO=targets["bs_SO"], bs_north=dict(sigma=1e-5))
  n, total = FC.N, _total(cls, cfg)
  ens = _build(cls, cfg, kw, forcing=gpu.ForcingSchedule(t, **values),
               noise=gpu.NoiseForcing(SEED, **targets))
  apps, written, states = _run_recording(ens, ["bs", "bs_north", "tau", "bs_SO"], total)
  interp = [[FC.member_values(values, t, s * ens.dt, m) for m in range(n)] for s in apps]
  col = lambda j, k: np.array([mv[k] for mv in interp[j]]).reshape(n, -1)  # noqa: E731
  for j in range(len(apps)):
    _bits(written["bs"][j], col(j, "bs"), ("bs", j))
  for k in ("tau", "bs_SO"):
    _check_series(cls, cfg, targets, k, apps, written, states,
                  [col(j, k) for j in range(len(apps))], what="scheduled")
  north = np.asarray(cls.read(cfg, "bs_north", n), dtype=np.float64).reshape(n, 1)
  _check_series(cls, cfg, targets, "bs_north", apps, written, states, north, what="scheduled")
  assert not np.array_equal(col(0, "tau"), col(len(apps) - 1, "tau"))  # the schedule moves


class _Shard(object):
  """What a driver reads off a communicator to place its members: rank and world."""

  def __init__(self, rank, world):
    self.rank, self.world = rank, world


def test_shards_write_the_series_of_the_whole_ensemble(gpu):
  """6 members in one ensemble against ranks 0 and 1 of a world of 2 (members 0-2 and 3-5):
  the written series and the final states are bitwise the whole ensemble's rows."""
  from pymoc_amd import configs
  cls = gpu.TwoColEnsemble
  ms = [dict(configs.twocol_member(nz=30, kappa_4k=k4), MOC_up_iters=8)
        for k4 in (2e-4, 2.2e-4, 2.4e-4, 2.6e-4, 2.8e-4, 3e-4)]
  cfg = FC._stack(ms, ("kappa", "b_basin0", "b_north0"))
  sig = 3e-4 * (1. + np.arange(6))
  targets = lambda sl: dict(bs=dict(sigma=sig[sl], tau_corr=180 * 86400.),  # noqa: E731
                            bs_north=dict(sigma=1e-5))
  total = _total(cls, cfg)
  whole = _build(cls, cfg, {}, noise=gpu.NoiseForcing(SEED, **targets(slice(None))))
  apps, w_all, x_all = _run_recording(whole, ["bs", "bs_north"], total)
  s_all = whole.state()
  for rank, sl in ((0, slice(0, 3)), (1, slice(3, 6))):
    part = cls.restrict(cfg, np.arange(6)[sl])
    ens = _build(cls, part, {}, noise=gpu.NoiseForcing(SEED, **targets(sl)),
                 comm=_Shard(rank, 2), n_total=6, diag_iters=0)
    assert ens.noise.desc.member0 == 3 * rank
    _, w, x = _run_recording(ens, ["bs", "bs_north"], total)
    for k in w:
      for j in range(len(apps)):
        _bits(w[k][j], w_all[k][j][sl], (rank, k, j))
        _bits(x[j][k], x_all[j][k][sl], (rank, k, j))
    _same(ens.state(), {k: v[sl] for k, v in s_all.items()}, rank)
  # without a communicator the same three members are members 0-2: other deviates
  alone = _build(cls, cls.restrict(cfg, np.arange(3, 6)), {},
                 noise=gpu.NoiseForcing(SEED, **targets(slice(3, 6))))
  alone.run(1)
  assert not np.array_equal(_read(alone, "bs"), w_all["bs"][0][3:])


def test_state_round_trip_and_continuation(gpu):
  cls, cfg, kw, targets = _kind(gpu, "jn2018")
  n, total = cls.members(cfg), _total(cls, cfg)
  M = int(cfg["MOC_up_iters"])
  noise = gpu.NoiseForcing(SEED, **targets)
  a = _build(cls, cfg, kw, noise=noise)
  a.run(total)
  b = _build(cls, cfg, kw, noise=noise)
  b.run(2 * M)
  st = b.noise.get_state()
  assert set(st) == set(targets) and all(v.shape == (n,) for v in st.values())
  junk = {k: np.full(n, 7.5) + np.arange(n) for k in st}
  b.noise.set_state(junk)
  _same(b.noise.get_state(), junk, "round trip")
  b.noise.set_state(st)
  _same(b.noise.get_state(), st, "round trip back")
  b.run(total - 2 * M)
  _same(a.state(), b.state(), "continued")
  _same(a.noise.get_state(), b.noise.get_state(), "continued noise")
  # a state set ahead of the first application is advanced, not replaced: at s = 0 no time has
  # passed, so the red states are written as they are and the white ones are drawn anew
  x0 = {k: 1e-5 * (1. + np.arange(n)) for k in ("bs_north", "b_rest")}
  c = _build(cls, cfg, kw, noise=noise)
  base = {k: _read(c, k) for k in x0}
  c.noise.set_state(x0)
  apps, written, states = _run_recording(c, list(x0), M + 1)
  for k in x0:
    _bits(states[0][k], x0[k], k)
    _bits(written[k][0], NC.written(base[k], x0[k], targets[k].get("pattern")), k)
    x_ref, _ = _restated(cls, cfg, targets, k, np.arange(n), apps, x0=x0[k])
    assert np.allclose(states[1][k], x_ref[1], rtol=0, atol=NC.series_bound(
        1, targets[k]["sigma"], 10.0, float(np.abs(x_ref).max())))
  with pytest.raises(ValueError, match="unknown noise target"):
    c.noise.set_state(dict(bs_SO=np.zeros(n)))
  with pytest.raises(ValueError, match="shape"):
    c.noise.set_state(dict(tau=np.zeros(n + 1)))


def test_refusals_with_a_device_present(gpu):
  TC.test_drivers_check_noise_on_the_host_and_refuse_what_it_does_not_go_with()
  TC.test_check_names_and_shapes_against_a_driver()


def test_index_recorder_on_a_noisy_ensemble(gpu):
  """The recorder needs no change: its series on a noisy JN2018Ensemble are np.max(Psi) and
  np.interp(-1000, z, b_basin) of the host-set twin's profiles right after each update."""
  cls, cfg, kw, targets = _kind(gpu, "jn2018")
  M, z = int(cfg["MOC_up_iters"]), np.asarray(cfg["z"])
  total = 3 * M
  a = _build(cls, cfg, kw, noise=gpu.NoiseForcing(SEED, **targets))
  rec = gpu.IndexRecorder(a, [("amoc", "max", "Psi", {}), ("b_1000", "at", "b_basin",
                                                           dict(x0=-1000.))], M, 3)
  apps, written, _ = _run_recording(a, list(targets), total)
  assert list(rec.steps) == [0, M, 2 * M]
  b = _build(cls, cfg, kw)
  quiet = _build(cls, cfg, kw)
  for j, s in enumerate(apps):
    for k in targets:
      _host_set(b, k, written[k][j])
    b.moc_update()  # the update at step s: what the recorder samples right after
    quiet.moc_update()
    psi, bb = b.tw.Psi.download(), b.b_basin.download()
    _bits(rec.values["amoc"][:, j].copy(), psi.max(axis=1), ("amoc", j))
    _bits(rec.values["b_1000"][:, j].copy(), np.array([np.interp(-1000., z, r) for r in bb]),
          ("b_1000", j))
    assert np.array_equal(rec.pos["amoc"][:, j], psi.argmax(axis=1))
    if j == len(apps) - 1:
      assert not np.array_equal(psi, quiet.tw.Psi.download())  # the noise reached the overturning
    b.run(M)
    quiet.run(M)
