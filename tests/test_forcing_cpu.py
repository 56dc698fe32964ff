"""ForcingSchedule and pm_forcing_apply without a device: the header mirror, the entry's structural
checks, the schedule's own validation, and every refusal that is raised before a driver touches
the device."""
import ctypes as C

import numpy as np
import pytest

from test_steady_cpu import _layout


def test_pm_forcing_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls in (_lib.pm_forcing_target, _lib.pm_forcing):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_forcing_apply"][1][0] is C.POINTER(_lib.pm_forcing)
  assert _lib.PM_FORCING_MAX_TARGETS == 8


def test_pm_forcing_apply_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first
  knots = np.array([0., 1., 2.5])

  def rc(n=4, K=3, ntargets=2, knots=knots, **target0):
    f = _lib.pm_forcing()
    f.n, f.K, f.ntargets = n, K, ntargets
    f.knots = None if knots is None else knots.ctypes.data
    for g in f.target:
      g.dst, g.row0, g.values, g.len, g.per_member = FAKE, 0, FAKE, 3, 1
    for k, v in target0.items():
      setattr(f.target[0], k, v)
    return L.pm_forcing_apply(C.byref(f), 0.5, None), L.pm_last_error().decode()

  assert L.pm_forcing_apply(None, 0.5, None) == _lib.PM_EINVAL
  cases = [dict(ntargets=0), dict(ntargets=9), dict(ntargets=-1), dict(K=0), dict(K=-2),
           dict(n=0), dict(knots=None), dict(dst=None), dict(values=None), dict(len=0),
           dict(len=-5), dict(row0=-1), dict(per_member=2),
           dict(knots=np.array([0., 1., 1.])), dict(knots=np.array([0., np.nan, 2.])),
           dict(knots=np.array([0., 1., np.inf]))]
  for kw in cases:
    code, text = rc(**kw)
    assert code == _lib.PM_EINVAL, (kw, code, text)
  assert "ntargets 9" in rc(ntargets=9)[1]
  assert "K 0" in rc(K=0)[1]
  assert "NULL" in rc(values=None)[1]
  assert "len 0" in rc(len=0)[1]
  # only the first `ntargets` entries are looked at
  f = _lib.pm_forcing()
  f.n, f.K, f.ntargets, f.knots = 4, 3, 1, knots.ctypes.data
  f.target[0].dst, f.target[0].values, f.target[0].len = FAKE, None, 1
  assert L.pm_forcing_apply(C.byref(f), 0.5, None) == _lib.PM_EINVAL


def test_schedule_validates_its_knots_and_the_knot_axis():
  from pymoc_amd import ForcingSchedule
  ok = ForcingSchedule([0., 1., 3.], bs=[1., 2., 3.], tau=np.zeros((3, 4)))
  assert ok.K == 3 and set(ok.values) == {"bs", "tau"}
  assert ForcingSchedule(5., bs=[0.02]).K == 1  # one knot: the value is held for all times
  for t in ([0., 1., 1.], [0., 2., 1.], [1., 0.]):
    with pytest.raises(ValueError, match="strictly increasing"):
      ForcingSchedule(t, bs=np.zeros(len(t)))
  for t in ([0., np.nan, 2.], [0., 1., np.inf], [-np.inf, 0., 1.]):
    with pytest.raises(ValueError, match="finite"):
      ForcingSchedule(t, bs=np.zeros(3))
  with pytest.raises(ValueError, match="1-D"):
    ForcingSchedule(np.zeros((2, 2)), bs=np.zeros(2))
  with pytest.raises(ValueError, match="at least one target"):
    ForcingSchedule([0., 1.])
  for bad in (np.zeros(3), np.zeros((3, 2)), 0.5, np.zeros((2, 1, 1, 1))):
    with pytest.raises(ValueError, match="'bs_north'.*2 knots"):
      ForcingSchedule([0., 1.], bs=np.zeros(2), bs_north=bad)


def _tc(n=4, so=False):
  from pymoc_amd import configs
  return configs.config4(N=n, nz=30, ny=20) if so else configs.config3(N=n, nz=30)


def _jn(n=4, tau_profile=False):
  from pymoc_amd import configs
  c = configs.config5(N=n, nz=40, ny=21)
  if tau_profile:
    c = dict(c, tau=np.asarray(c["tau"])[:, None] * np.ones((1, 21)))
  return c


def test_drivers_name_their_targets_and_check_shapes_on_the_host():
  """Names and shapes are checked against the cfg before any device state exists: these raise
  ValueError (not a missing-device error) on a machine without a GPU."""
  import pymoc_amd
  from pymoc_amd import ForcingSchedule, JN2018Ensemble, TwoColEnsemble
  t = [0., 1e6, 5e6]
  assert TwoColEnsemble.forcing_lengths(_tc(), 4) == dict(bs=1, bs_north=1)
  assert TwoColEnsemble.forcing_lengths(_tc(so=True), 4) == dict(bs=1, bs_north=1, tau=1,
                                                                 bs_SO=20)
  assert JN2018Ensemble.forcing_lengths(_jn(), 4) == dict(bs=1, bs_north=1, tau=1, b_rest=21,
                                                          surflux=21)
  assert JN2018Ensemble.forcing_lengths(_jn(tau_profile=True), 4)["tau"] == 21
  assert set(TwoColEnsemble.FORCING_TARGETS) == {"bs", "bs_north", "tau", "bs_SO"}
  assert set(JN2018Ensemble.FORCING_TARGETS) == {"bs", "bs_north", "tau", "b_rest", "surflux"}
  assert pymoc_amd.TwoBasinEnsemble.FORCING_TARGETS is None

  # unknown names: the message names the key and lists what the driver takes
  with pytest.raises(ValueError, match=r"'b_rest'.*bs, bs_SO, bs_north, tau"):
    TwoColEnsemble(_tc(so=True), forcing=ForcingSchedule(t, b_rest=np.zeros((3, 20))))
  with pytest.raises(ValueError, match=r"'tau'.*takes bs, bs_north$"):  # no SO channel
    TwoColEnsemble(_tc(), forcing=ForcingSchedule(t, tau=np.zeros(3)))
  with pytest.raises(ValueError, match=r"'bs_SO'.*b_rest, bs, bs_north, surflux, tau"):
    JN2018Ensemble(_jn(), forcing=ForcingSchedule(t, bs_SO=np.zeros((3, 21))))
  with pytest.raises(ValueError, match="'kappa'"):
    JN2018Ensemble(_jn(), forcing=ForcingSchedule(t, bs=np.zeros(3), kappa=np.zeros(3)))

  # wrong shapes: a profile for a scalar target, the wrong member count, the wrong row length
  for cls, cfg, kw in (
      (TwoColEnsemble, _tc(), dict(bs=np.zeros((3, 5)))),
      (TwoColEnsemble, _tc(), dict(bs_north=np.zeros((3, 4, 1)))),
      (TwoColEnsemble, _tc(so=True), dict(bs_SO=np.zeros(3))),
      (TwoColEnsemble, _tc(so=True), dict(bs_SO=np.zeros((3, 4, 19)))),
      (JN2018Ensemble, _jn(), dict(b_rest=np.zeros((3, 4)))),
      (JN2018Ensemble, _jn(), dict(surflux=np.zeros((3, 5, 21)))),
      (JN2018Ensemble, _jn(), dict(bs=np.zeros((3, 4)), b_rest=np.zeros((3, 22))))):
    key = sorted(kw)[0] if len(kw) == 1 else "b_rest"
    with pytest.raises(ValueError, match="%r: shape" % key):
      cls(cfg, forcing=ForcingSchedule(t, **kw))

  # tau follows the form of the batch's tau
  with pytest.raises(ValueError, match=r"'tau': shape \(3, 21\).*1 value"):
    JN2018Ensemble(_jn(), forcing=ForcingSchedule(t, tau=np.zeros((3, 21))))
  with pytest.raises(ValueError, match=r"'tau': shape \(3, 4\).*21 values"):
    JN2018Ensemble(_jn(tau_profile=True), forcing=ForcingSchedule(t, tau=np.zeros((3, 4))))
  with pytest.raises(ValueError, match=r"'tau': shape \(3, 20\).*1 value"):
    TwoColEnsemble(_tc(so=True), forcing=ForcingSchedule(t, tau=np.zeros((3, 20))))


def test_what_a_schedule_does_not_go_with_is_refused():
  import pymoc_amd
  from pymoc_amd import ForcingSchedule, JN2018Ensemble, TwoColEnsemble
  f = ForcingSchedule([0., 1e6], bs=[0.02, 0.03])
  with pytest.raises(ValueError, match="use_graph"):
    JN2018Ensemble(_jn(), forcing=f, use_graph=True)
  with pytest.raises(ValueError, match="fused_run"):
    JN2018Ensemble(_jn(), forcing=f, fused_run=True)
  with pytest.raises(ValueError, match="fused_run"):
    TwoColEnsemble(_tc(), forcing=f, fused_run=True)
  for cls, cfg in ((JN2018Ensemble, _jn()), (TwoColEnsemble, _tc())):
    with pytest.raises(ValueError, match="forcing"):
      pymoc_amd.run_to_steady(cls, cfg, 1e-6, 1200, forcing=f)
  with pytest.raises(TypeError):  # out of scope: no keyword
    pymoc_amd.TwoBasinEnsemble({}, forcing=f)
