"""The section interpolators on the GPU (pymoc_amd.plotting, pymoc_amd.SectionBatch): every G23
array / float case bit-identical to the reference, the reference's exceptions, ensemble batches,
device-row input, fix-ups, non-finite members, size limits, the example script."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
  return load_golden("sections")


def _cases(G):
  return [str(c) for c in G["cases"]]


def _profiles(G, c, fixed=True):
  tag = "_fixed" if fixed else ""
  out = []
  for nm in ("bs", "bn"):
    v = G[c + "_" + nm + tag]
    out.append(float(v) if bool(G[c + "_" + nm + "_float"]) else v.copy())
  return out


def _dropin(G, c):
  from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol
  cls = Interpolate_twocol if str(G[c + "_kind"]) == "twocol" else Interpolate_channel
  bs, bn = _profiles(G, c)
  return cls(y=G[c + "_y"], z=G[c + "_z"], bs=bs, bn=bn)


def _msgs(G, c, pre=""):
  return dict(zip(G[c + "_%sfail_idx" % pre].tolist(),
                  zip(G[c + "_%sfail_type" % pre].tolist(), G[c + "_%sfail_msg" % pre].tolist())))


def test_every_case_gridit_and_call_bitwise(gpu, G):
  """gridit (one launch) and __call__ (one-point launches) against the reference, every case."""
  ncheck = 0
  for c in _cases(G):
    obj = _dropin(G, c)
    ref, err = G[c + "_grid"], G[c + "_err"]
    full = G[c + "_yq"].size == G[c + "_y"].size and np.array_equal(G[c + "_yq"], G[c + "_y"]) \
        and np.array_equal(G[c + "_zq"], G[c + "_z"])
    if full:
      if (err != 0).any():
        k = int(np.flatnonzero(err.ravel())[0])
        with pytest.raises((ValueError, RuntimeError)) as ei:
          obj.gridit()
        assert (type(ei.value).__name__, str(ei.value)) == _msgs(G, c)[k], c
      else:
        got = obj.gridit()
        assert np.array_equal(got, ref, equal_nan=True), c
      ncheck += 1
    if c + "_cy" in G.files:
      cm = _msgs(G, c, "c")
      for k, (y, z) in enumerate(zip(G[c + "_cy"], G[c + "_cz"])):
        if G[c + "_cerr"][k] == 0:
          v = obj(y, z)
          assert np.array_equal(v, G[c + "_cval"][k], equal_nan=True), (c, k, y, z)
        else:
          with pytest.raises((ValueError, RuntimeError)) as ei:
            obj(y, z)
          assert (type(ei.value).__name__, str(ei.value)) == cm[k], (c, k)
  assert ncheck >= 20


def test_every_point_status_matches_reference(gpu, G):
  """SectionBatch on every case's own query grid: values bitwise, NaN + the reference's error
  code at every failing point, the first failing point in gridit order."""
  import pymoc_amd
  for c in _cases(G):
    bs, bn = _profiles(G, c)
    sb = pymoc_amd.SectionBatch(str(G[c + "_kind"]), G[c + "_y"], G[c + "_z"], bs, bn, n=1,
                                yq=G[c + "_yq"], zq=G[c + "_zq"])
    got = sb.grid().download()[0]
    ref, err = G[c + "_grid"], G[c + "_err"]
    assert np.array_equal(got, ref, equal_nan=True), c
    assert np.array_equal(sb.status()[0], err.astype(np.uint8)), c
    first = np.flatnonzero(err.ravel())
    assert sb.failed_points()[0] == (first[0] if first.size else -1), c


def _replicated(G, cases, n, rng):
  """n members cycling over `cases` (same kind and grids), every other one perturbed."""
  bss, bns, src = [], [], []
  for m in range(n):
    c = cases[m % len(cases)]
    bs, bn = G[c + "_bs_fixed"].copy(), G[c + "_bn_fixed"].copy()
    if m >= len(cases) and m % 2:  # one factor per member keeps the fix-ups' relations
      f = 1. + 1e-3 * rng.standard_normal()
      bs *= f
      bn *= f
    bss.append(bs)
    bns.append(bn)
    src.append(c if m < len(cases) else None)
  return np.array(bss), np.array(bns), src


@pytest.mark.parametrize("kind", ["channel", "north"])
def test_batch_of_4096_members(gpu, G, kind):
  import pymoc_amd
  from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol
  cases = [c for c in _cases(G) if c.startswith("sweep_") and c.endswith("_" + kind)]
  assert len(cases) >= 10
  c0 = cases[0]
  k = "twocol" if kind == "north" else "channel"
  y, z, yq, zq = G[c0 + "_y"], G[c0 + "_z"], G[c0 + "_yq"], G[c0 + "_zq"]
  rng = np.random.default_rng(4096)
  bs, bn, src = _replicated(G, cases, 4096, rng)
  sb = pymoc_amd.SectionBatch(k, y, z, bs, bn, yq=yq, zq=zq)
  out = sb.grid().download()
  assert out.shape == (4096, yq.size, zq.size)
  for m, c in enumerate(src):  # the G23 members themselves
    if c is not None:
      assert np.array_equal(out[m], G[c + "_grid"], equal_nan=True), (m, c)
  cls = Interpolate_twocol if k == "twocol" else Interpolate_channel
  for m in rng.choice(4096, 12, replace=False):  # perturbed members against the host twin
    obj = cls(y=y, z=z, bs=lambda x, p=bs[m]: np.interp(x, z if k == "twocol" else y, p),
              bn=lambda x, p=bn[m]: np.interp(x, z, p))
    host = np.array([[obj(a, b) for b in zq] for a in yq])
    assert np.array_equal(out[m], host), m
  assert (sb.failed_points() == -1).all()


@pytest.fixture(scope="module")
def ensemble(gpu):
  import pymoc_amd
  from pymoc_amd import configs
  n = 16
  cfg = configs.config5(N=n, nz=81, dt_days=30.)
  cfg["rest_mask"] = np.repeat(cfg["rest_mask"][None], n, axis=0)
  ens = pymoc_amd.JN2018Ensemble(cfg)
  ens.run(240)
  return ens, cfg


def _fixed_host(kind, mode, bs, bn):
  bs, bn = bs.copy(), bn.copy()
  if mode == "plot_overturning" and kind == "channel":
    if bs[0] > bs[1]:
      bs[0] = bs[1]
    if bs[0] < bn[0]:
      bn[0] = bs[0]
  elif mode == "plot_overturning":
    bn[0] = bs[0]
  elif mode == "twobasin":
    bs[-1] = bn[-1]
  return bs, bn


def test_device_rows_of_a_live_ensemble(ensemble):
  """DeviceArray rows read in place equal the drop-in classes on the downloaded state."""
  from pymoc_amd.plotting import Interpolate_channel, Interpolate_twocol
  sys.path.insert(0, os.path.join(ROOT, "examples"))
  import overturning_sections as ex
  ens, cfg = ensemble
  y, z = cfg["y"], cfg["z"]
  channel, north = ex.sections(ens, y, z)
  oc, on = channel.grid().download(), north.grid().download()
  st = ens.state()
  yn = north.y_host
  for m in range(ens.n):
    bs, bn = _fixed_host("channel", "plot_overturning", st["bs_SO"][m], st["b_basin"][m])
    assert np.array_equal(oc[m], Interpolate_channel(y=y, z=z, bs=bs, bn=bn).gridit()), m
    bs, bn = _fixed_host("twocol", "plot_overturning", st["b_basin"][m], st["b_north"][m])
    assert np.array_equal(on[m], Interpolate_twocol(y=yn, z=z, bs=bs, bn=bn).gridit()), m


@pytest.mark.parametrize("kind,mode", [("channel", "plot_overturning"), ("twocol", "plot_overturning"),
                                       ("channel", "twobasin")])
def test_fixups_equal_host_fixups(gpu, G, kind, mode):
  import pymoc_amd
  rng = np.random.default_rng(7)
  c = "g7_nz81_channel" if kind == "channel" else "g7_nz81_north"
  y, z = G[c + "_y"], G[c + "_z"]
  # raw inputs; for the twobasin fix-up the Plot_overturning-fixed ones (raw G7 profiles have
  # no bottom slope: every point off y == l raises, whatever bs[-1] is)
  tag = "_fixed" if mode == "twobasin" else ""
  bs0, bn0 = G[c + "_bs" + tag], G[c + "_bn" + tag]
  n = 8
  bs = np.repeat(bs0[None], n, axis=0)
  bn = np.repeat(bn0[None], n, axis=0)
  # members where each branch of the fix-ups is taken
  bs[1, 0] = bs[1, 1] + 1e-4
  bn[2, 0] = bs[2, 0] + 1e-4
  bn[3, -1] += 1e-5
  bs[4] *= 1. + 1e-3 * rng.standard_normal()
  if kind == "channel":
    bs[5, -1] = bn[5, -1] + 1e-3  # a warmer surface end (twobasin_NadeauJansen.py:176's case)
  fixed = [_fixed_host(kind, mode, bs[m], bn[m]) for m in range(n)]
  # on the class grid a channel point never reads bs between y[-2] and l: query inside it too
  yq = np.sort(np.concatenate([y, [0.25 * y[-2] + 0.75 * y[-1], 0.5 * (y[-2] + y[-1])]]))
  got = pymoc_amd.SectionBatch(kind, y, z, bs, bn, yq=yq, fixups=mode).grid().download()
  want = pymoc_amd.SectionBatch(kind, y, z, np.array([f[0] for f in fixed]),
                                np.array([f[1] for f in fixed]), yq=yq).grid().download()
  assert np.array_equal(got, want, equal_nan=True)
  unfixed = pymoc_amd.SectionBatch(kind, y, z, bs, bn, yq=yq).grid().download()
  assert not np.array_equal(unfixed, got, equal_nan=True)
  with pytest.raises(ValueError):
    pymoc_amd.SectionBatch("twocol", y, z, bs, bn, fixups="twobasin")


def test_nonfinite_member_is_isolated(gpu, G):
  import pymoc_amd
  c = "g7_nz81_channel"
  y, z = G[c + "_y"], G[c + "_z"]
  bs = np.repeat(G[c + "_bs_fixed"][None], 4, axis=0)
  bn = np.repeat(G[c + "_bn_fixed"][None], 4, axis=0)
  bn[2, 40] = np.nan
  bs[3, 10] = np.nan
  sb = pymoc_amd.SectionBatch("channel", y, z, bs, bn)
  out = sb.grid().download()
  st = sb.status()
  for m in (0, 1):
    assert np.array_equal(out[m], G[c + "_grid"]) and not st[m].any()
  for m in (2, 3):
    assert np.isnan(out[m]).any() and st[m].any() and sb.failed_points()[m] >= 0
    assert np.isnan(out[m][st[m] != 0]).all()
  assert (sb.failed_points()[:2] == -1).all()


def test_size_limits(gpu):
  import pymoc_amd
  from pymoc_amd.plotting import Interpolate_channel
  z = np.linspace(-4000., 0., 1024)
  y = np.linspace(0., 2e6, 64)
  bs = 0.02 * (y / y[-1]) ** 2 - 0.001
  bn = 0.02 * np.exp(z / 700.) - 0.0015
  sb = pymoc_amd.SectionBatch("channel", y, z, bs, bn, n=1, yq=y[::8], zq=z)
  out = sb.grid().download()[0]
  obj = Interpolate_channel(y=y, z=z, bs=lambda x: np.interp(x, y, bs),
                            bn=lambda x: np.interp(x, z, bn))
  for i in (0, 3, 7):
    for j in (0, 1, 511, 1023):
      assert np.array_equal(out[i, j], obj(y[8 * i], z[j]))
  big = np.linspace(-4000., 0., 1025)
  with pytest.raises(pymoc_amd._lib.PmError, match="1024"):
    pymoc_amd.SectionBatch("channel", y, big, bs, np.interp(big, z, bn), n=1).grid()


def test_example_script(gpu):
  p = subprocess.run([sys.executable, "examples/overturning_sections.py", "--members", "32",
                      "--steps", "240"], cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  assert "equals the drop-in classes on the downloaded state: True" in p.stdout
