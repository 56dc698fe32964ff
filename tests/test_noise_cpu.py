"""NoiseForcing and pm_forcing_noise without a device: the generator's known answers and moments
through the NumPy restatement (tests/noise_cases.py), the application rule, the AR(1)
coefficients, the header mirror, the entry's argument checks and every host-side refusal."""
import ctypes as C

import numpy as np
import pytest

import noise_cases as NC
from test_steady_cpu import _layout


# ------------------------------------------------------------------ the restatement
def test_philox_known_answers():
  zero = NC.philox4x32_10((0, 0, 0, 0), (0, 0))
  assert [int(w) for w in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
  f = 0xffffffff
  ones = NC.philox4x32_10((f, f, f, f), (f, f))
  assert [int(w) for w in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
  # the words of a deviate: key from the seed's halves, counter (id lo, id hi, j, stream)
  seed, ident = 0x0123456789abcdef, (5 << 32) | 7
  got = NC.words(seed, ident, 9, 3)
  want = NC.philox4x32_10((7, 5, 9, 3), (0x89abcdef, 0x01234567))
  assert [int(w) for w in got] == [int(w) for w in want]


def test_uniforms_are_exact_multiples_inside_the_unit_interval():
  ids = np.arange(4096, dtype=np.uint64)[:, None]
  j = np.arange(16, dtype=np.uint64)[None, :]
  for d in NC.uniforms(2018, ids, j, 2):
    assert d.min() >= 0.0 and d.max() < 1.0
    assert np.array_equal(d * 2.0**53, np.floor(d * 2.0**53))
    assert np.array_equal((1.0 - d) + d, np.ones_like(d))  # 1 - d is exact
    assert (1.0 - d).min() > 0.0 and (1.0 - d).max() <= 1.0
  # the extreme words: d = 0 and d = 1 - 2^-53
  lo = ((0 >> 5) * 67108864.0 + (0 >> 6)) * NC.EPS
  hi = ((0xffffffff >> 5) * 67108864.0 + (0xffffffff >> 6)) * NC.EPS
  assert lo == 0.0 and hi == 1.0 - 2.0**-53 and 1.0 - hi == 2.0**-53


@pytest.mark.parametrize("seed,stream", [(2018, 0), (2018, 2), (0, 0), (0, 2)])
def test_moments_of_the_restatement(seed, stream):
  """ids 0..4095 x j 0..63: mean, variance and the lag-1 products along j and along id within 4
  standard errors of 0, 1, 0, 0 (for N independent standard normals: 1/sqrt(N), sqrt(2/N),
  1/sqrt(N'), N' the number of products)."""
  ids = np.arange(4096, dtype=np.uint64)[:, None]
  j = np.arange(64, dtype=np.uint64)[None, :]
  xi, R = NC.deviate(seed, ids, j, stream)
  N = xi.size
  assert np.isfinite(xi).all() and (R >= 0).all()
  mean, var = xi.mean(), xi.var()
  lag_j = (xi[:, 1:] * xi[:, :-1]).mean()
  lag_id = (xi[1:, :] * xi[:-1, :]).mean()
  z = [mean * np.sqrt(N), (var - 1.0) / np.sqrt(2.0 / N),
       lag_j * np.sqrt(xi[:, 1:].size), lag_id * np.sqrt(xi[1:, :].size)]
  print(seed, stream, "z-scores (mean, var, lag j, lag id): %.2f %.2f %.2f %.2f" % tuple(z))
  assert np.abs(z).max() <= 4.0, z


# ------------------------------------------------------------------ the host rules
@pytest.mark.parametrize("M,phase", [(8, 1), (6, 0), (1, 0), (1, 1), (5, 1)])
def test_application_rule(M, phase):
  """j and the elapsed time for RESTART_PHASE 0 and 1, s = 0 included: the product's closed form
  against the restatement's enumeration."""
  from pymoc_amd.noise import application
  dt = 86400.0 * 30
  seen = []
  for s in range(4 * M + 3):
    got, want = application(s, M, phase, dt), NC.application(s, M, phase, dt)
    assert got == want, (s, got, want)
    if got is not None:
      seen.append((s,) + got)
  assert seen[0] == (0, 0, 0.0)
  assert [j for _, j, _ in seen] == list(range(len(seen)))
  if (M, phase) == (8, 1):
    assert seen[:4] == [(0, 0, 0.0), (1, 1, dt), (9, 2, 8 * dt), (17, 3, 8 * dt)]
  if (M, phase) == (6, 0):
    assert seen[:3] == [(0, 0, 0.0), (6, 1, 6 * dt), (12, 2, 6 * dt)]
  assert application(-1, M, phase, dt) is None


def test_ar1_coefficients():
  from pymoc_amd.noise import ar1
  assert ar1(0.0, 5.0) == (0.0, 1.0) and ar1(0.0, 0.0) == (0.0, 1.0)
  assert ar1(np.inf, 5.0) == (1.0, 0.0)
  a, b = ar1(10.0, 5.0)
  assert a == float(np.exp(np.float64(-0.5))) and b == float(np.sqrt(1.0 - a * a))
  assert abs(a * a + b * b - 1.0) < 4 * NC.EPS
  assert ar1(10.0, 0.0) == (1.0, 0.0)        # no time has passed: the state is carried
  a, b = ar1(1.0, 1e6)                        # long after: white
  assert (a, b) == (0.0, 1.0)
  for tau, el in ((10.0, 5.0), (3e7, 2.6e6), (1e-3, 7.0)):
    assert ar1(tau, el) == NC.ar1(tau, el)
    assert all(0.0 <= v <= 1.0 for v in ar1(tau, el))


# ------------------------------------------------------------------ the C-ABI
def test_pm_noise_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls in (_lib.pm_noise_target, _lib.pm_noise):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_forcing_noise"][1][0] is C.POINTER(_lib.pm_noise)
  assert _lib.PM_NOISE_MAX_TARGETS == 8 and _lib.PM_NOISE_STREAMS == len(NC.STREAMS)
  from pymoc_amd import noise
  assert noise.STREAMS == NC.STREAMS


def bad_descriptors():
  """[(label, keyword edits)]: descriptors that are wrong in exactly one way.  Shared with the
  GPU test, which shows that the outputs stay untouched."""
  return [("ntargets 0", dict(ntargets=0)), ("ntargets 9", dict(ntargets=9)),
          ("ntargets -1", dict(ntargets=-1)), ("n 0", dict(n=0)), ("n -3", dict(n=-3)),
          ("member0", dict(member0=-1)), ("dst", dict(dst=None)), ("base", dict(base=None)),
          ("sigma", dict(sigma=None)), ("x_in", dict(x_in=None)), ("len 0", dict(len=0)),
          ("len -5", dict(len=-5)), ("row0", dict(row0=-1)), ("x_out is x_in", dict(x_out="x_in")),
          ("a nan", dict(a=np.nan)), ("a inf", dict(a=np.inf)), ("a > 1", dict(a=1.5)),
          ("a < 0", dict(a=-0.25)), ("b nan", dict(b=np.nan)), ("b > 1", dict(b=1.0000001)),
          ("b < 0", dict(b=-1e-9)), ("stream -1", dict(stream=-1)),
          ("stream 6", dict(stream=6)), ("pattern_per_member", dict(pattern_per_member=2)),
          ("too many elements", dict(n=2**20, len=2**11))]


def fill(f, entries, n=4, ntargets=2, member0=0, **target0):
  """`entries`: per target a dict of addresses dst, base, sigma, x_in, x_out, xi_out, pattern."""
  f.n, f.ntargets, f.j, f.seed, f.member0 = n, ntargets, 3, 2018, member0
  for g, e in zip(f.target, entries):
    g.dst, g.row0, g.base, g.sigma = e["dst"], 0, e["base"], e["sigma"]
    g.x_in, g.x_out, g.xi_out, g.pattern = e["x_in"], e["x_out"], e["xi_out"], e["pattern"]
    g.a, g.b, g.len, g.pattern_per_member, g.stream = 0.5, 0.75, 3, 0, 1
  for k, v in target0.items():
    setattr(f.target[0], k, f.target[0].x_in if isinstance(v, str) else v)
  return f


def test_pm_forcing_noise_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first
  entries = [dict(dst=FAKE, base=FAKE + 64, sigma=FAKE + 128, x_in=FAKE + 192 + 64 * i,
                  x_out=FAKE + 1024 + 64 * i, xi_out=None, pattern=None) for i in range(8)]
  assert L.pm_forcing_noise(None, None) == _lib.PM_EINVAL
  for label, kw in bad_descriptors():
    top = {k: kw.pop(k) for k in ("n", "ntargets", "member0") if k in kw}
    f = fill(_lib.pm_noise(), entries, **dict(top, **kw))
    assert L.pm_forcing_noise(C.byref(f), None) == _lib.PM_EINVAL, label
    assert L.pm_last_error(), label
  # one entry's x_out is another's x_in: a launch would read what it writes
  f = fill(_lib.pm_noise(), entries)
  f.target[1].x_out = f.target[0].x_in
  assert L.pm_forcing_noise(C.byref(f), None) == _lib.PM_EINVAL
  assert "x_out" in L.pm_last_error().decode()
  # only the first `ntargets` entries are looked at
  f = fill(_lib.pm_noise(), entries, ntargets=1)
  f.target[1].dst = None
  f.target[0].sigma = None
  assert L.pm_forcing_noise(C.byref(f), None) == _lib.PM_EINVAL
  assert "target 0" in L.pm_last_error().decode()


# ------------------------------------------------------------------ NoiseForcing
def test_noise_forcing_validates_its_arguments():
  from pymoc_amd import NoiseForcing
  ok = NoiseForcing(2018, bs=dict(sigma=1e-3), tau=dict(sigma=[0.1, 0.2], tau_corr=np.inf))
  assert ok.seed == 2018 and set(ok.targets) == {"bs", "tau"}
  assert ok.targets["bs"]["tau_corr"] == 0.0 and ok.targets["bs"]["pattern"] is None
  assert NoiseForcing(2**64 - 1, bs=dict(sigma=0.0)).seed == 2**64 - 1
  assert NoiseForcing(np.int64(7), bs=dict(sigma=0.0)).seed == 7
  for seed in (-1, 2**64, 1.5, "7", None, True):
    with pytest.raises(ValueError, match="seed"):
      NoiseForcing(seed, bs=dict(sigma=1.0))
  with pytest.raises(ValueError, match="at least one target"):
    NoiseForcing(1)
  with pytest.raises(ValueError, match="unknown noise target 'kappa'"):
    NoiseForcing(1, kappa=dict(sigma=1.0))
  for spec in (1.0, dict(tau_corr=1.0), dict(sigma=1.0, colour="red")):
    with pytest.raises(ValueError, match="'bs'"):
      NoiseForcing(1, bs=spec)
  for sigma in (-1e-9, np.nan, np.inf, [0.1, -0.1], [0.1, np.nan], np.zeros((2, 2))):
    with pytest.raises(ValueError, match="sigma"):
      NoiseForcing(1, bs=dict(sigma=sigma))
  for tau in (-1.0, np.nan, -np.inf):
    with pytest.raises(ValueError, match="tau_corr"):
      NoiseForcing(1, bs=dict(sigma=1.0, tau_corr=tau))
  with pytest.raises(ValueError, match="pattern"):
    NoiseForcing(1, b_rest=dict(sigma=1.0, pattern=np.zeros((2, 2, 2))))
  with pytest.raises(ValueError, match="pattern"):
    NoiseForcing(1, b_rest=dict(sigma=1.0, pattern=3.0))


def test_check_names_and_shapes_against_a_driver():
  from pymoc_amd import NoiseForcing
  lengths, n = dict(bs=1, bs_north=1, tau=1, b_rest=21, surflux=21), 4
  ok = NoiseForcing(3, bs=dict(sigma=np.full(4, 0.1)), b_rest=dict(sigma=1., pattern=np.ones(21)),
                    surflux=dict(sigma=1., pattern=np.ones((4, 21))), tau=dict(sigma=0.))
  assert ok.check(lengths, n) == dict(bs=None, b_rest=False, surflux=True, tau=None)
  with pytest.raises(ValueError, match=r"'bs_SO'.*b_rest, bs, bs_north, surflux, tau"):
    NoiseForcing(3, bs_SO=dict(sigma=1.)).check(lengths, n)
  with pytest.raises(ValueError, match="'bs': sigma of length 3 for 4 members"):
    NoiseForcing(3, bs=dict(sigma=np.ones(3))).check(lengths, n)
  with pytest.raises(ValueError, match="'tau'.*no pattern"):
    NoiseForcing(3, tau=dict(sigma=1., pattern=np.ones(1))).check(lengths, n)
  for pattern in (np.ones(20), np.ones((3, 21)), np.ones((4, 20)), np.ones((21, 4))):
    with pytest.raises(ValueError, match="'b_rest': pattern of shape"):
      NoiseForcing(3, b_rest=dict(sigma=1., pattern=pattern)).check(lengths, n)
  # more than 8 destinations: refused before any device array is made (the stand-ins are never
  # looked at)
  nine = {"bs": [(None, 0, 1)] * 9}
  with pytest.raises(ValueError, match="at most 8 destinations"):
    NoiseForcing(3, bs=dict(sigma=1.)).bind(4, nine)
  with pytest.raises(ValueError, match="differ in row length"):
    NoiseForcing(3, bs=dict(sigma=1.)).bind(4, {"bs": [(None, 0, 1), (None, 0, 2)]})
  with pytest.raises(ValueError, match="member0"):
    NoiseForcing(3, bs=dict(sigma=1.)).bind(4, {"bs": [(None, 0, 1)]}, member0=-1)


def _tc(n=4, so=False):
  from pymoc_amd import configs
  return configs.config4(N=n, nz=30, ny=20) if so else configs.config3(N=n, nz=30)


def _jn(n=4):
  from pymoc_amd import configs
  return configs.config5(N=n, nz=40, ny=21)


def test_drivers_check_noise_on_the_host_and_refuse_what_it_does_not_go_with():
  """Before any device state exists: these raise ValueError (not a missing-device error) on a
  machine without a GPU."""
  import pymoc_amd
  from pymoc_amd import (JN2018Ensemble, JN2018ImplicitEnsemble, NoiseForcing, TwoBasinSweep,
                         TwoColEnsemble)
  nz = NoiseForcing(1, bs=dict(sigma=1e-4))
  with pytest.raises(ValueError, match=r"'b_rest'.*bs, bs_SO, bs_north, tau"):
    TwoColEnsemble(_tc(so=True), noise=NoiseForcing(1, b_rest=dict(sigma=1.)))
  with pytest.raises(ValueError, match=r"'tau'.*takes bs, bs_north$"):  # no SO channel
    TwoColEnsemble(_tc(), noise=NoiseForcing(1, tau=dict(sigma=1.)))
  with pytest.raises(ValueError, match=r"'bs_SO'.*b_rest, bs, bs_north, surflux, tau"):
    JN2018Ensemble(_jn(), noise=NoiseForcing(1, bs_SO=dict(sigma=1.)))
  with pytest.raises(ValueError, match="sigma of length 3"):
    JN2018ImplicitEnsemble(_jn(), noise=NoiseForcing(1, bs=dict(sigma=np.ones(3))))
  with pytest.raises(ValueError, match="'b_rest': pattern"):
    JN2018Ensemble(_jn(), noise=NoiseForcing(1, b_rest=dict(sigma=1., pattern=np.ones(20))))
  with pytest.raises(ValueError, match="'tau'.*no pattern"):
    JN2018Ensemble(_jn(), noise=NoiseForcing(1, tau=dict(sigma=1., pattern=np.ones(21))))
  import twobasin_sweep_cases as TS
  with pytest.raises(ValueError, match=r"'surflux'.*bs, bs_SO, bs_north, tau"):
    TwoBasinSweep(TS.cfg(), noise=NoiseForcing(1, surflux=dict(sigma=1.)))
  # the refusals: the wording of forcing's
  with pytest.raises(ValueError, match="noise does not go with use_graph=True: a captured"):
    JN2018Ensemble(_jn(), noise=nz, use_graph=True)
  with pytest.raises(ValueError, match="noise does not go with fused_run=True"):
    JN2018Ensemble(_jn(), noise=nz, fused_run=True)
  with pytest.raises(ValueError, match="noise does not go with fused_run=True"):
    TwoColEnsemble(_tc(), noise=nz, fused_run=True)
  for cls, cfg in ((JN2018Ensemble, _jn()), (TwoColEnsemble, _tc())):
    with pytest.raises(ValueError, match="run_to_steady does not take noise"):
      pymoc_amd.run_to_steady(cls, cfg, 1e-6, 1200, noise=nz)
  with pytest.raises(TypeError):  # out of scope: no keyword
    pymoc_amd.TwoBasinEnsemble({}, noise=nz)
