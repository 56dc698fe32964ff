"""CPU checks of the section interpolators (pymoc_amd.plotting, pymoc_amd.sections): the host
brenth twin against SciPy, gridit, the drop-in classes with CALLABLE profiles (the host path)
against the reference's recorded sections (G23), constructor errors, the pm_sections ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden


def _outcome(fn, *args):
  try:
    return ("ok", fn(*args))
  except (ValueError, RuntimeError) as e:
    return (type(e).__name__, str(e))


def test_brenth_twin_equals_scipy_bitwise():
  from scipy import optimize
  from pymoc_amd.utils.brenth import brenth
  rng = np.random.default_rng(23)
  kinds = {"ok": 0, "ValueError": 0, "RuntimeError": 0}
  for k in range(2500):
    xp = np.sort(rng.uniform(-3., 3., rng.integers(2, 24)))
    fp = rng.normal(size=xp.size)
    if k % 50 == 0:
      fp[rng.integers(0, xp.size)] = np.nan  # the NaN-value ValueError
    t = rng.normal(scale=0.5)
    f = lambda x: np.interp(x, xp, fp) - t
    a, b = rng.uniform(-4., 0.), rng.uniform(0., 4.)
    ref, got = _outcome(optimize.brenth, f, a, b), _outcome(brenth, f, a, b)
    assert ref == got, (k, ref, got)
    kinds[ref[0]] += 1
  for k in range(300):  # analytic functions
    c = rng.uniform(-2., 2.)
    f = [lambda x: x ** 3 - c, lambda x: np.tanh(x - c) + 1e-3 * x, lambda x: np.exp(x) - 2. - c][k % 3]
    ref, got = _outcome(optimize.brenth, f, -3., 3.), _outcome(brenth, f, -3., 3.)
    assert ref == got, (k, ref, got)
    kinds[ref[0]] += 1
  # no convergence: a step function over more iterations than maxiter allows
  f = lambda x: -1. if x < 1. / 3. else 1.
  for it in (3, 5, 100):
    ref = _outcome(lambda a, b: optimize.brenth(f, a, b, maxiter=it), 0., 1.)
    assert ref == _outcome(lambda a, b: brenth(f, a, b, maxiter=it), 0., 1.)
  assert ref[0] == "ok"
  with pytest.raises(RuntimeError, match="Failed to converge after 5 iterations."):
    brenth(f, 0., 1., maxiter=5)
  with pytest.raises(ValueError, match="f\\(a\\) and f\\(b\\) must have different signs"):
    brenth(lambda x: 1. + x * x, -1., 1.)
  assert kinds["ok"] > 1000 and kinds["ValueError"] > 50


def test_gridit_semantics():
  from pymoc_amd.utils import gridit
  calls = []

  def f(a, b):
    calls.append((a, b))
    return 10. * a + b
  x1, x2 = np.array([1., 2., 3.]), np.array([0.5, 0.25])
  g = gridit(x1, x2, f)
  assert g.shape == (3, 2) and g.dtype == np.float64
  assert np.array_equal(g, 10. * x1[:, None] + x2[None, :])
  assert calls == [(a, b) for a in x1 for b in x2]  # row-major

  def boom(a, b):
    if a == 2. and b == 0.25:
      raise ValueError("first")
    if a == 3.:
      raise RuntimeError("never reached")
    return 0.
  with pytest.raises(ValueError, match="first"):
    gridit(x1, x2, boom)


def _callables(G, c):
  """The case's (fixed-up) profiles as Python callables: make_func's closures, unnamed."""
  kind = str(G[c + "_kind"])
  bs, bn = G[c + "_bs_fixed"], G[c + "_bn_fixed"]
  y, z = G[c + "_y"], G[c + "_z"]
  bs_axis = z if kind == "twocol" else y

  def wrap(v, axis, is_float):
    if is_float:
      val = float(v)
      return lambda x: val + 0 * x
    return lambda x: np.interp(x, axis, v)
  return (wrap(bs, bs_axis, bool(G[c + "_bs_float"])), wrap(bn, z, bool(G[c + "_bn_float"])))


HOST_CASES = ["g7_nz81_channel", "g7_nz81_north", "g9_trans", "reftest_twocol_fix",
              "float_bs_channel", "float_both_twocol", "nonuniform_twocol", "failing_twocol",
              "nonfinite_channel", "nonfinite_twocol"]


@pytest.mark.parametrize("case", HOST_CASES)
def test_callable_profiles_match_reference_bitwise(case):
  """Callable profiles take the host path: every point and every exception as the reference."""
  from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol
  G = load_golden("sections")
  cls = Interpolate_twocol if str(G[case + "_kind"]) == "twocol" else Interpolate_channel
  bs, bn = _callables(G, case)
  obj = cls(y=G[case + "_y"], z=G[case + "_z"], bs=bs, bn=bn)
  yq, zq = G[case + "_yq"], G[case + "_zq"]
  ref, err = G[case + "_grid"], G[case + "_err"]
  msgs = dict(zip(G[case + "_fail_idx"].tolist(),
                  zip(G[case + "_fail_type"].tolist(), G[case + "_fail_msg"].tolist())))
  for i in range(yq.size):
    for j in range(zq.size):
      out = _outcome(obj, yq[i], zq[j])
      k = i * zq.size + j
      if err[i, j] == 0:
        assert out[0] == "ok" and np.array_equal(out[1], ref[i, j], equal_nan=True), (i, j)
      else:
        assert out[0] != "ok", (i, j)
        if k in msgs:
          assert out == msgs[k], (i, j)
  if (err != 0).any():
    k = int(np.flatnonzero(err.ravel())[0])
    with pytest.raises((ValueError, RuntimeError)) as ei:
      obj.gridit()
    assert (type(ei.value).__name__, str(ei.value)) == msgs[k]
  else:
    assert np.array_equal(obj.gridit(), ref, equal_nan=True)


def test_constructor_errors_match_reference():
  from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol
  G = load_golden("sections")
  z81, y51 = np.linspace(-4.0e3, 0, 81), np.linspace(0, 2.0e6, 51)
  got = []
  for cls in (Interpolate_channel, Interpolate_twocol):
    for kw in ({}, {"z": z81}, {"y": y51}, {"z": z81, "y": 1e6}, {"z": z81, "y": y51},
               {"z": z81, "y": y51, "bs": np.linspace(0.02, 0.01, 51)}):
      try:
        cls(**kw)
        got.append("")
      except TypeError as e:
        got.append(str(e))
  assert got == G["ctor_errors"].tolist()
  with pytest.raises(TypeError) as ei:
    Interpolate_twocol(y=y51, z=z81, bs=1, bn=0.1)
  assert ei.value.args == ('bs', 'needs to be either function, numpy array, or float')
  ic = Interpolate_channel(y=y51, z=z81, bs=0.01, bn=np.linspace(0., 0.01, 81))
  f = ic.make_func(np.arange(81.), 'q', ic.z)
  assert f(-2000.) == np.interp(-2000., ic.z, np.arange(81.))
  assert ic.make_func(6.0, 'q', ic.y)(1e5) == 6.0


def test_pm_sections_layout_matches_header(tmp_path):
  from pymoc_amd import _lib
  src = tmp_path / "sizes.c"
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pymoc_hip.h"\n'
                 'int main(void) {\n  printf("%zu", sizeof(pm_sections));\n' +
                 "".join('  printf(" %%zu", offsetof(pm_sections, %s));\n' % f[0]
                         for f in _lib.pm_sections._fields_) + "  return 0;\n}\n")
  exe = tmp_path / "sizes"
  subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
  vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
  assert vals[0] == C.sizeof(_lib.pm_sections)
  assert vals[1:] == [getattr(_lib.pm_sections, f[0]).offset for f in _lib.pm_sections._fields_]
  assert _lib.SIGNATURES["pm_sections_grid"][1][0] is C.POINTER(_lib.pm_sections)


def test_pm_sections_rejects_bad_arguments_before_touching_the_device():
  from pymoc_amd import _lib
  L = _lib.lib

  def rc(**kw):
    d = _lib.pm_sections()
    d.n, d.kind, d.ny, d.nz, d.nyq, d.nzq = 4, _lib.PM_SEC_CHANNEL, 51, 81, 51, 81
    for k, v in kw.items():
      setattr(d, k, v)
    return L.pm_sections_grid(C.byref(d), None), L.pm_last_error().decode()

  assert L.pm_sections_grid(None, None) == _lib.PM_EINVAL
  assert rc(kind=2) == (_lib.PM_EINVAL, "bad kind 2")
  code, text = rc(nz=1025)
  assert code == _lib.PM_EINVAL and "1024" in text
  assert rc(ny=1)[0] == _lib.PM_EINVAL
  assert rc(nyq=0)[0] == _lib.PM_EINVAL
  assert rc(nzq=1025)[0] == _lib.PM_EINVAL
  assert rc(n=-1)[0] == _lib.PM_EINVAL
  assert rc(flags=4)[0] == _lib.PM_EINVAL
  assert rc(fixups=4)[0] == _lib.PM_EINVAL
  code, text = rc(kind=_lib.PM_SEC_TWOCOL, fixups=_lib.PM_SEC_FIX_TWOBASIN)
  assert code == _lib.PM_EINVAL and "third profile" in text
  assert rc(fixups=1, flags=_lib.PM_SEC_BS_SCALAR)[0] == _lib.PM_EINVAL
  assert rc(bs_stride=-1)[0] == _lib.PM_EINVAL
  code, text = rc()  # every pointer NULL
  assert code == _lib.PM_EINVAL and "NULL" in text
  assert rc(n=0) == (_lib.PM_OK, rc(n=0)[1])  # nothing to do


def test_fixture_records_versions():
  G = load_golden("sections")
  assert str(G["reference"]) == "pymoc 0.0.1rc5"
  assert str(G["numpy_version"]) and str(G["scipy_version"])
  assert len(G["cases"]) >= 40
