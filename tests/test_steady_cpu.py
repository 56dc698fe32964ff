"""CPU checks of the run to steady state (pymoc_amd.steady): the pm_steady_check ABI and its
argument checks, the restriction of a config to a subset of members, the check schedule and the
driver's refusals -- all before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _layout(tmp_path, struct, fields):
  src = tmp_path / ("%s.c" % struct)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pymoc_hip.h"\n'
                 'int main(void) {\n  printf("%%zu", sizeof(struct %s));\n' % struct +
                 "".join('  printf(" %%zu", offsetof(struct %s, %s));\n' % (struct, f[0])
                         for f in fields) + "  return 0;\n}\n")
  exe = tmp_path / struct
  subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
  return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]


def test_pm_steady_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  for cls in (_lib.pm_steady_field, _lib.pm_steady_check):
    vals = _layout(tmp_path, cls.__name__, cls._fields_)
    assert vals[0] == C.sizeof(cls)
    assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]
  assert _lib.SIGNATURES["pm_steady_check"][1][0] is C.POINTER(_lib.pm_steady_check)
  assert (_lib.PM_STEADY_RUNNING, _lib.PM_STEADY_CONVERGED, _lib.PM_STEADY_NONFINITE,
          _lib.PM_STEADY_MAXSTEPS) == (0, 1, 2, 3)


def test_pm_steady_check_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib
  FAKE = 0x10000  # never dereferenced: every case below fails a host-side check first

  def rc(**kw):
    c = _lib.pm_steady_check()
    c.n, c.n0, c.ndrift, c.ncapture, c.consecutive, c.finalize, c.step = 8, 8, 2, 3, 1, 0, 10
    c.scale = 1.
    for name in ("orig", "tol", "streak", "status", "drift_out", "step_out", "n_running"):
      setattr(c, name, FAKE)
    for f in list(c.drift) + list(c.capture):
      f.src, f.buf, f.len, f.src_stride = FAKE, FAKE, 16, 16
    for k, v in kw.items():
      if callable(v):
        v(c)
      else:
        setattr(c, k, v)
    return L.pm_steady_check(C.byref(c), None), L.pm_last_error().decode()

  assert L.pm_steady_check(None, None) == _lib.PM_EINVAL
  cases = [dict(n=-1), dict(n=9), dict(n0=-1, n=0), dict(ndrift=0), dict(ndrift=5),
           dict(ncapture=-1), dict(ncapture=9), dict(consecutive=0), dict(consecutive=-3),
           dict(finalize=2), dict(step=-1)]
  cases += [{name: 0} for name in ("orig", "tol", "streak", "status", "drift_out", "step_out",
                                   "n_running")]
  cases += [dict(f=lambda c: setattr(c.drift[1], "src", 0)),
            dict(f=lambda c: setattr(c.drift[0], "buf", 0)),
            dict(f=lambda c: setattr(c.drift[0], "len", 0)),
            dict(f=lambda c: setattr(c.drift[1], "src_stride", 15)),
            dict(f=lambda c: setattr(c.capture[2], "src", 0)),
            dict(f=lambda c: setattr(c.capture[0], "len", 0))]
  for kw in cases:
    code, text = rc(**kw)
    assert code == _lib.PM_EINVAL, (kw, code, text)
  assert "NULL" in rc(tol=0)[1]
  assert "ndrift 5" in rc(ndrift=5)[1]
  assert "consecutive 0" in rc(consecutive=0)[1]


def _jn_cfg(N, nz=81, rest_mask_2d=False):
  from pymoc_amd import configs
  cfg = configs.config5(N=N, nz=nz, dt_days=30.)
  if rest_mask_2d:
    cfg["rest_mask"] = np.repeat(cfg["rest_mask"][None], N, axis=0)
  return cfg


@pytest.mark.parametrize("case", ["jn_new_n_is_nz", "jn_rest_mask_2d", "twocol_new_n_is_nz",
                                  "twocol_so"])
def test_restrict_cfg_reads_like_the_constructor(case):
  from pymoc_amd import JN2018Ensemble, TwoColEnsemble, configs
  from pymoc_amd.steady import restrict_cfg
  rng = np.random.default_rng(7)
  if case.startswith("jn"):
    cls, nz = JN2018Ensemble, 81
    cfg = _jn_cfg(120, nz=nz, rest_mask_2d=case == "jn_rest_mask_2d")
    n = 120
  elif case == "twocol_new_n_is_nz":
    cls, nz = TwoColEnsemble, 100
    cfg = configs.config3(N=130, nz=nz)
    n = 130
  else:
    cls, nz = TwoColEnsemble, 100
    cfg = configs.config4(N=120, nz=nz)
    n = 120
  # the new n equals nz: a 1-D per-member key restricted to length nz would be read as a profile
  keep = np.sort(rng.choice(n, nz if case != "jn_rest_mask_2d" else 17, replace=False))
  out = restrict_cfg(cls, cfg, keep)
  for key in cls.MEMBER_KEYS:
    if key not in cfg:
      continue
    got = np.asarray(cls.read(out, key, keep.size), dtype=np.float64)
    want = np.asarray(cls.read(cfg, key, n), dtype=np.float64)
    if want.shape[:1] == (n,):
      want = want[keep]
    assert np.array_equal(np.broadcast_to(got, want.shape), want), key
  if case == "jn_rest_mask_2d":
    assert out["rest_mask"].shape == (17, cfg["y"].size)
    assert np.array_equal(out["rest_mask"], cfg["rest_mask"][keep])
  if case == "twocol_new_n_is_nz":
    # A_basin is 1-D per member in config3; at the new n = nz it must come out 2-D
    assert np.ndim(out["A_basin"]) == 2 and np.ndim(out["bs"]) == 1
  # keys the constructors do not read, and shared ones, are passed on untouched
  assert out["z"] is cfg["z"] and out["dt"] == cfg["dt"]
  # restriction composes: a subset of a subset is the subset
  sub = np.array([0, 3, 5])
  twice = restrict_cfg(cls, out, sub)
  once = restrict_cfg(cls, cfg, keep[sub])
  for key in cls.MEMBER_KEYS:
    if key in cfg:
      a = cls.read(twice, key, 3)
      b = cls.read(once, key, 3)
      assert np.array_equal(np.broadcast_to(a, np.shape(b)), b), key


def test_check_schedule_both_classes():
  from pymoc_amd import JN2018Ensemble, TwoColEnsemble
  from pymoc_amd.steady import check_schedule
  s0, ch = check_schedule(JN2018Ensemble, 12, 120, 3600)
  assert s0 == 0 and ch == list(range(120, 3601, 120))
  s0, ch = check_schedule(JN2018Ensemble, 12, 120, 3650)  # last boundary <= 3650 is 3648
  assert ch[-2:] == [3600, 3648]
  s0, ch = check_schedule(JN2018Ensemble, 12, 24, 23)
  assert ch == [12]
  s0, ch = check_schedule(TwoColEnsemble, 24, 240, 3601)
  assert s0 == 1 and ch == list(range(241, 3602, 240))
  s0, ch = check_schedule(TwoColEnsemble, 24, 240, 3600)  # s = 1 (mod 24) grid: 3577
  assert ch[-2:] == [3361, 3577]
  for s in ch:
    assert s % 24 == 1
  with pytest.raises(ValueError, match="multiple of MOC_up_iters"):
    check_schedule(JN2018Ensemble, 12, 100, 3600)
  with pytest.raises(ValueError, match="multiple of MOC_up_iters"):
    check_schedule(TwoColEnsemble, 24, 0, 3600)
  with pytest.raises(ValueError, match="no check"):
    check_schedule(TwoColEnsemble, 24, 240, 24)
  with pytest.raises(ValueError, match="no check"):
    check_schedule(JN2018Ensemble, 12, 120, 11)


def test_run_to_steady_refusals():
  import pymoc_amd
  from pymoc_amd import configs
  jn = _jn_cfg(4)
  tc = configs.config3(N=4)
  run = pymoc_amd.run_to_steady
  for cls, cfg in ((pymoc_amd.TwoBasinEnsemble, configs.config_twobasin(N=4)),
                   (pymoc_amd.ColumnThermwindEnsemble, configs.config2(N=4)),
                   (pymoc_amd.EquiIterationEnsemble, jn), (dict, jn)):
    with pytest.raises(ValueError, match="JN2018Ensemble and TwoColEnsemble"):
      run(cls, cfg, 1e-6, 1200)
  for cls, cfg in ((pymoc_amd.JN2018Ensemble, jn), (pymoc_amd.TwoColEnsemble, tc)):
    with pytest.raises(ValueError, match="arith"):
      run(cls, cfg, 1e-6, 1200, arith="contracted")
    with pytest.raises(ValueError, match="fused_run"):
      run(cls, cfg, 1e-6, 1200, fused_run=True)
    with pytest.raises(ValueError, match="comm"):
      run(cls, cfg, 1e-6, 1200, comm=object())
    with pytest.raises(ValueError, match="keep_history"):
      run(cls, cfg, 1e-6, 1200, keep_history=True)
    with pytest.raises(ValueError, match="multiple of MOC_up_iters"):
      run(cls, cfg, 1e-6, 1200, check_every=int(cfg["MOC_up_iters"]) * 5 + 1)
  # the default check_every (cfg['Diag_iters'], else 10 MOC_up_iters) must fit the grid too
  bad = dict(tc, Diag_iters=100)
  with pytest.raises(ValueError, match="multiple of MOC_up_iters"):
    run(pymoc_amd.TwoColEnsemble, bad, 1e-6, 1200)
  with pytest.raises(ValueError, match="consecutive"):
    run(pymoc_amd.TwoColEnsemble, tc, 1e-6, 1201, consecutive=0)
  with pytest.raises(ValueError, match="compact_below"):
    run(pymoc_amd.TwoColEnsemble, tc, 1e-6, 1201, compact_below=1.5)
  with pytest.raises(ValueError, match="tol"):
    run(pymoc_amd.TwoColEnsemble, tc, np.zeros(3), 1201)
