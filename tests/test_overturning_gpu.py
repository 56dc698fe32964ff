"""The overturning streamfunction sections on the GPU (pymoc_amd.OverturningSections,
pm_overturning_sections): fixture G24 -- the reference's Plot_overturning.py run on 16 states --
bitwise, batches of 4096 from host arrays and from strided device rows, the extrema, the route
from a live ensemble, status bits and isolation, host validation."""
import ctypes

import numpy as np
import pytest

import overturning_cases as OC
from conftest import load_golden

pytestmark = pytest.mark.gpu

FIELDS = (("z", "psiarray_z"), ("b", "psiarray_b"), ("res", "psiarray_res"))
ALL = ("z", "b", "res", "bnew")


@pytest.fixture(scope="module")
def G():
  return OC.load()


@pytest.fixture(scope="module")
def cases(gpu, G):
  """Every case with the FULL buoyancy sections the kernel needs: the fixture's own bnew where it
  is stored in full, else SectionBatch's (checked bitwise against the stored levels first)."""
  import pymoc_amd
  from pymoc_amd.overturning import section_rows
  out = {}
  for c in OC.names(G):
    k = OC.case(G, c)
    ny, lev = k["ny"], k["levels"]
    if k["full"]:
      k["bsouth"], k["bnorth"] = k["bnew"][:ny].copy(), k["bnew"][ny + OC.N_BASIN:].copy()
    else:
      ch = pymoc_amd.SectionBatch("channel", k["y"], k["z"], bs=k["bs_SO"][None], bn=k["b_basin"][None],
                                  fixups="plot_overturning")
      no = pymoc_amd.SectionBatch("twocol", section_rows(k["y"])["y_north"], k["z"],
                                  bs=k["b_basin"][None], bn=k["b_north"][None],
                                  fixups="plot_overturning")
      k["bsouth"], k["bnorth"] = ch.grid().download()[0], no.grid().download()[0]
      assert (ch.failed_points() == -1).all() and (no.failed_points() == -1).all(), c
      assert np.array_equal(k["bsouth"][:, lev], k["bnew"][:ny]), c
      assert np.array_equal(k["bnorth"][:, lev], k["bnew"][ny + OC.N_BASIN:]), c
    out[c] = k
  return out


def _inputs(ks):
  """Host arrays [n][...] of the explicit route for a list of cases on one grid."""
  kw = {name: np.array([k[name] for k in ks]) for name in
        ("b_basin", "bs_SO", "Psi", "Psi_SO", "bgrid", "psib", "bsouth", "bnorth")}
  kw["psibz"] = np.array([k["psibz1"] for k in ks])
  return kw


def _explicit(ks, store=ALL, **kw):
  import pymoc_amd
  k0 = ks[0]
  args = _inputs(ks)
  args.update(kw)
  return pymoc_amd.OverturningSections(k0["y"], k0["z"], k0["nb"], store=store, **args).compute()


def _fields(o):
  return {"z": o.psi_z.download()[:o.n], "b": o.psi_b.download()[:o.n],
          "res": o.psi_res.download()[:o.n]}


def test_explicit_route_every_case_bitwise(cases):
  """The fixture's inputs -- the reference's own Psi, psib, ... -- give the reference's three fields
  and bnew bit for bit at every stored level, all 16 cases."""
  for c, k in cases.items():
    o = _explicit([k])
    lev = k["levels"]
    assert np.array_equal(o.ynew, k["ynew"]), c
    assert np.array_equal(o.b.download()[0][:, lev], k["bnew"]), c
    got = _fields(o)
    for f, name in FIELDS:
      assert np.array_equal(got[f][0][:, lev], k[name]), (c, name)
    assert o.status()[0] == 0, c


@pytest.fixture(scope="module")
def nz200(cases):
  """The 15 cases on the 200-level grid, their fields from one 15-member launch."""
  ks = [k for k in cases.values() if k["nz"] == 200]
  assert len(ks) == 15
  o = _explicit(ks)
  ref = _fields(o)
  ref["bnew"] = o.b.download()
  for j, k in enumerate(ks):
    for f, name in FIELDS + (("bnew", "bnew"),):
      assert np.array_equal(ref[f][j][:, k["levels"]], k[name]), (k["name"], name)
  return ks, ref, o.extrema()


def _check_batch(o, idx, ref, ext):
  for f, arr in (("z", o.psi_z), ("b", o.psi_b), ("res", o.psi_res), ("bnew", o.b)):
    got = arr.download()
    for m0 in range(0, idx.size, 512):
      sl = slice(m0, m0 + 512)
      assert np.array_equal(got[sl], ref[f][idx[sl]]), (f, m0)
    del got
  e = o.extrema()
  for key in ("max", "min", "argmax", "argmin"):
    assert np.array_equal(e[key], ext[key][idx]), key
  assert not o.status().any()


def test_batch_of_4096_from_host_arrays(nz200):
  ks, ref, ext = nz200
  idx = np.random.default_rng(4096).permutation(np.arange(4096) % len(ks))
  o = _explicit([ks[i] for i in idx])
  assert o.n == 4096 and o.psi_z.shape == (4096, 121, 200)
  _check_batch(o, idx, ref, ext)


def test_batch_of_4096_from_strided_device_rows(nz200):
  """Every input read in place from a device array whose rows are further apart than they are
  long and start at an offset."""
  import pymoc_amd
  from pymoc_amd import DeviceArray
  ks, ref, ext = nz200
  n = 4096
  idx = np.random.default_rng(77).permutation(np.arange(n) % len(ks))
  host = _inputs(ks)
  dev = {}
  for j, (name, a) in enumerate(host.items()):
    length = int(np.prod(a.shape[1:]))
    off, stride = 3 + j, length + 8 + 2 * j
    buf = np.full(off + n * stride, np.nan)
    rows = buf[off:].reshape(n, stride)  # (buf is exactly off + n * stride long)
    rows[:, :length] = a.reshape(len(ks), length)[idx]
    dev[name] = (DeviceArray.from_host(buf), off, stride)
  k0 = ks[0]
  o = pymoc_amd.OverturningSections(k0["y"], k0["z"], k0["nb"], n=n, store=ALL, **dev).compute()
  _check_batch(o, idx, ref, ext)


def _np_extrema(fields):
  """np.max / np.argmax / np.min / np.argmin of [n][nrows][nz] fields, columns z, b, res."""
  flat = [fields[f].reshape(fields[f].shape[0], -1) for f in ("z", "b", "res")]
  return {"max": np.stack([a.max(axis=1) for a in flat], axis=1),
          "min": np.stack([a.min(axis=1) for a in flat], axis=1),
          "argmax": np.stack([a.argmax(axis=1) for a in flat], axis=1).astype(np.int32),
          "argmin": np.stack([a.argmin(axis=1) for a in flat], axis=1).astype(np.int32)}


def _same_extrema(a, b):
  return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("max", "min", "argmax", "argmin"))


def test_extrema(cases, nz200):
  # the fixture's full arrays (G7)
  for c in ("g7_nz81", "g7_nz200"):
    k = cases[c]
    assert k["full"]
    e = _explicit([k]).extrema()
    want = _np_extrema({f: k[name][None] for f, name in FIELDS})
    assert _same_extrema(e, want), (c, e, want)
  # every case: the downloaded fields
  ks, ref, ext = nz200
  assert _same_extrema(ext, _np_extrema(ref))
  o = _explicit([cases["g7_nz81"]])
  assert _same_extrema(o.extrema(), _np_extrema(_fields(o)))
  # nothing stored: the same numbers
  o = _explicit(ks, store=())
  assert o.psi_z is None and o.psi_b is None and o.psi_res is None and o.b is None
  assert _same_extrema(o.extrema(), ext)
  # planted NaNs: NaN and the first NaN's index, as NumPy gives; the neighbours unchanged
  args = _inputs(ks[:4])
  args["Psi_SO"][1, 57] = np.nan
  args["psib"][2, :] = np.nan
  o = _explicit(ks[:4], **args)
  got, e = _fields(o), o.extrema()
  assert np.isnan(got["z"][1]).any() and np.isnan(got["b"][1]).any() and np.isnan(got["res"][2]).any()
  assert _same_extrema(e, _np_extrema(got))
  assert np.isnan(e["max"][1]).all() and np.isnan(e["min"][1]).all()
  assert np.isnan(e["max"][2, 2]) and not np.isnan(e["max"][2, :2]).any()
  for m in (0, 3):
    for key in e:
      assert np.array_equal(e[key][m], ext[key][m])
    for f in got:
      assert np.array_equal(got[f][m], ref[f][m])


@pytest.fixture(scope="module")
def config5(gpu):
  from pymoc_amd import configs
  n = 256
  cfg = configs.config5(N=n)
  cfg["rest_mask"] = np.repeat(cfg["rest_mask"][None], n, axis=0)
  return cfg


def test_ensemble_route_equals_explicit_route(config5):
  """from_ensemble on a live config-5 ensemble against the explicit route fed with the downloaded
  rows of its private solvers and sections."""
  import pymoc_amd
  cfg = config5
  ens = pymoc_amd.JN2018Ensemble(cfg)
  ens.run(72)
  o = pymoc_amd.OverturningSections.from_ensemble(ens, cfg, store=ALL).compute()
  st = ens.state()
  dl = lambda a: a.download(stream=ens.stream)
  x = pymoc_amd.OverturningSections(
      cfg["y"], cfg["z"], int(cfg["nb"]), b_basin=st["b_basin"], bs_SO=st["bs_SO"], Psi=dl(o.tw.Psi),
      Psi_SO=dl(o.so.Psi), bgrid=dl(o.tw.bgrid), psib=dl(o.tw.psib), psibz=dl(o.tw.psibz1),
      bsouth=dl(o.channel.out), bnorth=dl(o.north.out), store=ALL).compute()
  assert o.n == x.n == ens.n == 256 and o.nrows == 121
  for a, b in ((o.psi_z, x.psi_z), (o.psi_b, x.psi_b), (o.psi_res, x.psi_res), (o.b, x.b)):
    assert np.array_equal(dl(a), b.download(), equal_nan=True)
  assert _same_extrema(o.extrema(), x.extrema())
  assert np.array_equal(o.status(), x.status())
  ok = o.status() == 0  # (members whose section has a failing point are reported, not compared)
  assert ok.any() and np.isfinite(o.extrema()["max"][ok]).all()
  # the private thermal-wind solve is a solve of the current state
  tw = pymoc_amd.ThermwindBatch(cfg["z"], ens.n, f=cfg["f"], nb=int(cfg["nb"]))
  b1, b2 = pymoc_amd.DeviceArray.from_host(st["b_basin"]), pymoc_amd.DeviceArray.from_host(st["b_north"])
  tw.update(b1, b2)
  assert np.array_equal(tw.psibz1.download(), dl(o.tw.psibz1), equal_nan=True)
  assert np.array_equal(tw.psib.download(), dl(o.tw.psib), equal_nan=True)


def test_sections_between_runs_leave_the_trajectory_alone(config5):
  import pymoc_amd
  cfg = config5
  a, b = pymoc_amd.JN2018Ensemble(cfg), pymoc_amd.JN2018Ensemble(cfg)
  a.run(54)
  b.run(54)
  o = pymoc_amd.OverturningSections.from_ensemble(a, cfg)
  before = a.state()
  o.compute()
  o.extrema()
  mid = a.state()
  for k in before:
    assert np.array_equal(before[k], mid[k], equal_nan=True), k
  a.run(90)
  b.run(90)
  sa, sb = a.state(), b.state()
  for k in sa:
    assert np.array_equal(sa[k], sb[k], equal_nan=True), k
  assert np.array_equal(a.wA.download(), b.wA.download(), equal_nan=True)


def test_status_bits_and_isolation(cases):
  k = cases["g7_nz81"]
  ks = [k] * 7
  clean = _explicit(ks)
  want = _fields(clean)
  args = _inputs(ks)
  args["bnorth"][1, 3, 5] = np.nan                  # a section point where brenth raised
  args["bsouth"][2, 17, 40] = np.nan
  args["b_basin"][3, [60, 61]] = args["b_basin"][3, [61, 60]]  # decreasing
  assert args["b_basin"][3, 61] < args["b_basin"][3, 60]
  args["b_basin"][4, 12] = np.nan
  args["b_basin"][5, 80] = np.inf
  o = _explicit(ks, **args)
  st = o.status()
  assert st.tolist()[:3] == [0, 1, 1] and st[3] == 2 and st[4] & 2 and st[5] & 2 and st[6] == 0
  got, e, ec = _fields(o), o.extrema(), clean.extrema()
  for m in (0, 6):  # the neighbours of all of them
    for f in got:
      assert np.array_equal(got[f][m], want[f][m]), (f, m)
    for key in e:
      assert np.array_equal(e[key][m], ec[key][m])
  assert np.isnan(o.b.download()[1, 51 + 60 + 3, 5])
  # G23's failing profiles through SectionBatch: the member's section holds NaNs, bit 1
  import pymoc_amd
  S = pymoc_amd.SectionBatch
  G23 = load_golden("sections")
  c = "failing_channel"
  y, z = G23[c + "_y"], G23[c + "_z"]
  sec = S("channel", y, z, G23[c + "_bs"][None], G23[c + "_bn"][None]).grid().download()
  assert np.isnan(sec).any()
  nz, ny = z.size, y.size
  rng = np.random.default_rng(3)
  prof = lambda n: np.sort(rng.uniform(-1e-3, 2e-2, n))
  one = dict(b_basin=prof(nz), bs_SO=prof(ny), Psi=rng.normal(size=nz), Psi_SO=rng.normal(size=nz),
             bgrid=prof(50), psib=rng.normal(size=50), psibz=rng.normal(size=nz),
             bnorth=np.tile(prof(nz), (10, 1)))
  bsouth = np.stack([np.tile(prof(nz), (ny, 1)), sec[0], np.tile(prof(nz), (ny, 1))])
  o = pymoc_amd.OverturningSections(y, z, 50, bsouth=bsouth, **one).compute()
  assert o.status().tolist() == [0, 1, 0]
  alone = pymoc_amd.OverturningSections(y, z, 50, bsouth=bsouth[[0, 2]], **one).compute()
  for f, arr in _fields(alone).items():
    assert np.array_equal(arr, _fields(o)[f][[0, 2]]), f


def test_host_validation_and_limits(gpu, cases):
  import pymoc_amd
  from pymoc_amd import _lib, DeviceArray
  k = cases["g7_nz81"]
  y, z, nb = k["y"], k["z"], k["nb"]
  good = _inputs([k, k])
  OS = pymoc_amd.OverturningSections
  OS(y, z, nb, **good).compute()
  for name, bad in (("b_basin", good["b_basin"][:, :-1]), ("bs_SO", good["bs_SO"][:, 1:]),
                    ("bgrid", good["bgrid"][:, :499]), ("bsouth", good["bsouth"][:, :, :-1]),
                    ("bnorth", good["bnorth"][:, :9]), ("Psi", good["Psi"][:1].repeat(3, axis=0)),
                    ("psibz", good["psibz"].astype(np.float32)[None])):
    with pytest.raises(ValueError):
      OS(y, z, nb, **dict(good, **{name: bad}))
  with pytest.raises(ValueError):
    OS(y, z, nb, **dict(good, Psi=None))
  with pytest.raises(TypeError):
    OS(y, z, nb, **dict(good, Psi=[1., 2.]))
  with pytest.raises(ValueError, match="store"):
    OS(y, z, nb, store=("psi",), **good)
  # rows running past the end of a device array
  dev = DeviceArray.from_host(good["Psi"])
  OS(y, z, nb, **dict(good, Psi=dev))
  OS(y, z, nb, **dict(good, Psi=(dev, z.size, 0)))
  for tup in ((dev, 1, z.size), (dev, 0, z.size + 1), (dev, 2 * z.size, 0)):
    with pytest.raises(ValueError, match="past the end"):
      OS(y, z, nb, **dict(good, Psi=tup))
  with pytest.raises(ValueError, match="n is needed"):
    OS(y, z, nb, **{a: DeviceArray.from_host(b) for a, b in good.items()})
  # limits
  with pytest.raises(ValueError, match="2048"):
    OS(y, z, 2049, **good)
  with pytest.raises(ValueError, match="1024"):
    OS(y, np.linspace(-4000., 0., 1025), nb, **good)
  with pytest.raises(ValueError):
    OS(y, z, nb, n_basin=1000, n_north=25, **good)
  # ... and through the raw C-ABI
  o = OS(y, z, nb, **good)  # (owns the device memory the descriptors point to)
  d = o.descriptor()
  assert _lib.lib.pm_overturning_sections(ctypes.byref(d), None) == _lib.PM_OK
  for field, v in (("nb", 2049), ("nz", 1025), ("ny", 1), ("n_basin", 1020), ("c1", None)):
    d = o.descriptor()
    setattr(d, field, v)
    assert _lib.lib.pm_overturning_sections(ctypes.byref(d), None) == _lib.PM_EINVAL, field
  pymoc_amd.synchronize()
  # the largest shapes run: nz = ny = 1024, nb = 2048 (73.5 KB of LDS per workgroup)
  rng = np.random.default_rng(11)
  zb, yb = np.linspace(-4000., 0., 1024), np.linspace(0., 2e6, 1024)
  prof = lambda n: np.sort(rng.uniform(-1e-3, 2e-2, n))
  big = dict(b_basin=prof(1024), bs_SO=prof(1024), Psi=rng.normal(size=1024),
             Psi_SO=rng.normal(size=1024), bgrid=prof(2048), psib=rng.normal(size=2048),
             psibz=rng.normal(size=1024), bsouth=rng.uniform(-1e-3, 2e-2, (1024, 1024)),
             bnorth=rng.uniform(-1e-3, 2e-2, (3, 1024)))
  o = OS(yb, zb, 2048, n=2, n_basin=2, n_north=3, store=("res", "b"), **big).compute()
  res, pb = o.psi_res.download(), o.psi_b.download()
  assert np.array_equal(res[0], res[1]) and o.nrows == 1029
  for iy in (1, 500, 1023):
    assert np.array_equal(res[0, iy], np.interp(big["bsouth"][iy], big["b_basin"], big["Psi_SO"]))
    want = np.where(big["b_basin"] < big["bs_SO"][iy], big["Psi_SO"], 0.)
    assert np.array_equal(pb[0, iy], want)
  assert np.array_equal(res[0, 1027], np.interp(big["bnorth"][1], big["bgrid"], big["psib"]))
  assert not res[0, 1028].any() and not res[0, 0].any()


def test_example_script(gpu):
  import os
  import subprocess
  import sys
  from conftest import ROOT
  p = subprocess.run([sys.executable, os.path.join("examples", "overturning_streamfunctions.py"),
                      "--members", "32", "--steps", "240"], cwd=ROOT, capture_output=True, text=True,
                     timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  assert "equals the explicit route on the downloaded rows: True" in p.stdout
  assert "equals NumPy on the host: True" in p.stdout
