"""The two-basin overturning sections on the GPU (pymoc_amd.TwoBasinOverturningSections,
pm_twobasin_profiles, pm_twobasin_overturning_sections): fixture G25 -- lines 157-262 of the
reference's twobasin_NadeauJansen.py run on 10 states -- bitwise, a batch of 300 from strided
device rows, the extrema, a tiny shape against NumPy, the route from a live ensemble, status bits
and isolation, host validation."""
import ctypes

import numpy as np
import pytest

import twobasin_overturning_cases as TC

pytestmark = pytest.mark.gpu

def _mod():
  from pymoc_amd import twobasin_overturning as T
  return T


@pytest.fixture(scope="module")
def G():
  return TC.load()


def _dev(a, stride=None):
  from pymoc_amd import DeviceArray
  a = np.ascontiguousarray(a, dtype=np.float64)
  return (DeviceArray.from_host(a), 0, a.shape[-1] if stride is None else stride)


@pytest.fixture(scope="module")
def cases(gpu, G):
  """Every case with the FULL sections the kernel needs: pm_twobasin_profiles' bn and
  SectionBatch's channel and transition sections, each checked bitwise against the stored levels
  of the fixture's bnew first."""
  import pymoc_amd
  T = _mod()
  out = {}
  for c in TC.names(G):
    k = TC.case(G, c)
    ny, nz, lev = k["ny"], k["nz"], k["levels"]
    A = [_dev(np.array([k[a]]), 0) for a in ("A_Atl", "A_Pac")]
    bb, bn = T.TwoBasinOverturningSections.profiles(_dev(k["b_Atl"]), _dev(k["b_Pac"]),
                                                    _dev(k["b_north"]), A[0], A[1], 1, nz)
    k["b_basin"], k["bn"] = bb.download()[0], bn.download()[0]
    want = (k["A_Atl"] * k["b_Atl"] + k["A_Pac"] * k["b_Pac"]) / (k["A_Atl"] + k["A_Pac"])
    assert np.array_equal(k["b_basin"], want), c
    assert np.array_equal(k["bn"][1:], k["b_north"][1:]) and k["bn"][0] == want[0], c
    ch = pymoc_amd.SectionBatch("channel", k["y"], k["z"], bs=k["bs_SO"][None], bn=k["b_basin"][None],
                                fixups="twobasin")
    tr = pymoc_amd.SectionBatch("twocol", T.twobasin_section_rows(k["y"])["y_trans"], k["z"],
                                bs=k["b_Atl"][None], bn=k["bn"][None])
    k["bsouth"], k["btrans"] = ch.grid().download()[0], tr.grid().download()[0]
    assert (ch.failed_points() == -1).all() and (tr.failed_points() == -1).all(), c
    assert np.array_equal(k["bsouth"][:, lev], k["bnew"][:ny]), c
    assert np.array_equal(k["btrans"][:, lev], k["bnew"][ny + 60:ny + 80]), c
    assert np.array_equal(np.tile(k["bn"][lev], (20, 1)), k["bnew"][ny + 80:]), c
    out[c] = k
  return out


def _inputs(ks):
  """Host arrays [n][...] of the explicit route for a list of cases."""
  return {name: np.array([k[name] for k in ks]) for name in _mod().TwoBasinOverturningSections.ROWS}


def _explicit(ks, store=None, **kw):
  T = _mod()
  k0 = ks[0]
  args = _inputs(ks)
  args.update(kw)
  return T.TwoBasinOverturningSections(k0["y"], k0["z"], k0["nb"],
                                       store=T.STORE if store is None else store, **args).compute()


def _all(o):
  return {name: o.download(name) for name in o.store}


def _same_extrema(a, b):
  return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("max", "min", "argmax", "argmin"))


def _np_extrema(fields, pac_rows):
  """np.max / argmax / min / argmin of {name: [n][nrows][nz]}, the Pacific fields over
  [:pac_rows]."""
  T = _mod()
  flat = []
  for name in T.FIELDS:
    a = fields[name][:, :pac_rows] if name in TC.PACIFIC else fields[name]
    flat.append(a.reshape(a.shape[0], -1))
  return {"max": np.stack([a.max(axis=1) for a in flat], axis=1),
          "min": np.stack([a.min(axis=1) for a in flat], axis=1),
          "argmax": np.stack([a.argmax(axis=1) for a in flat], axis=1).astype(np.int32),
          "argmin": np.stack([a.argmin(axis=1) for a in flat], axis=1).astype(np.int32)}


@pytest.fixture(scope="module")
def singles(cases):
  """Each case launched alone: its eleven arrays and its extrema, every stored level checked
  against the fixture."""
  T = _mod()
  ks = list(cases.values())
  ref = {name: [] for name in T.STORE}
  ext = {key: [] for key in ("max", "min", "argmax", "argmin")}
  for k in ks:
    o = _explicit([k])
    assert np.array_equal(o.ynew, k["ynew"]), k["name"]
    assert o.nrows == k["ny"] + 100
    got = _all(o)
    for name in T.STORE:
      assert np.array_equal(got[name][0][:, k["levels"]], k[name], equal_nan=True), (k["name"], name)
      ref[name].append(got[name][0])
    assert o.status()[0] == 0, k["name"]
    e = o.extrema()
    for key in ext:
      ext[key].append(e[key][0])
  return (ks, {name: np.array(v) for name, v in ref.items()}, {key: np.array(v) for key, v in ext.items()})


def test_explicit_route_every_case_bitwise(singles):
  """The fixture's inputs -- the reference's own Psi, Psib, Psibz ... -- give the script's eight
  fields and three buoyancy sections bit for bit at every stored level, all 10 cases, the one
  with overturnings older than its columns included (the checks are in the fixture above)."""
  ks, ref, ext = singles
  assert len(ks) == 10 and ref["psiarray_b_Pac"].shape == (10, 151, 80)
  assert np.isnan(ref["psiarray_Pac"][:, 111:]).all() and np.isnan(ref["bnew_Pac"][:, 111:]).all()
  assert np.isfinite(ext["max"]).all() and np.isfinite(ext["min"]).all()


def test_batch_of_300_from_strided_device_rows(singles):
  """More workgroups than CUs, 151 * 80 points (no multiple of 256) each; every input read in
  place from a device array whose rows are further apart than they are long and start at an
  offset."""
  from pymoc_amd import DeviceArray
  T = _mod()
  ks, ref, ext = singles
  n = 300
  idx = np.random.default_rng(300).permutation(np.arange(n) % len(ks))
  dev = {}
  for j, (name, a) in enumerate(_inputs(ks).items()):
    length = int(np.prod(a.shape[1:]))
    off, stride = 3 + j, length + 8 + 2 * j
    buf = np.full(off + n * stride, np.nan)
    buf[off:].reshape(n, stride)[:, :length] = a.reshape(len(ks), length)[idx]
    dev[name] = (DeviceArray.from_host(buf), off, stride)
  k0 = ks[0]
  o = T.TwoBasinOverturningSections(k0["y"], k0["z"], k0["nb"], n=n, store=T.STORE, **dev).compute()
  for name in T.STORE:
    assert np.array_equal(o.download(name), ref[name][idx], equal_nan=True), name
  e = o.extrema()
  for key in e:
    assert np.array_equal(e[key], ext[key][idx]), key
  assert not o.status().any()


def test_extrema(singles):
  T = _mod()
  ks, ref, ext = singles
  assert _same_extrema(ext, _np_extrema(ref, 111))
  # the fixture's full arrays
  k = ks[0]
  assert k["full"]
  want = _np_extrema({name: k[name][None] for name in T.FIELDS}, 111)
  assert _same_extrema({key: v[:1] for key, v in ext.items()}, want)
  # nothing stored: the same numbers
  o = _explicit(ks, store=())
  assert all(getattr(o, name) is None for name in T.STORE)
  assert _same_extrema(o.extrema(), ext)
  # a planted NaN: NaN and the first NaN's index, as NumPy gives; the neighbours unchanged
  args = _inputs(ks[:3])
  args["Psi_SO_Pac"][1, 57] = np.nan
  o = _explicit(ks[:3], **args)
  got, e = _all(o), o.extrema()
  assert np.isnan(got["psiarray_z"][1]).any() and np.isnan(got["psiarray_b_Pac"][1, :111]).any()
  assert _same_extrema(e, _np_extrema(got, 111))
  nan_cols = np.isnan(e["max"][1])
  assert nan_cols[[0, 2, 5, 7]].all() and np.array_equal(nan_cols, np.isnan(e["min"][1]))
  assert (e["argmax"][1][nan_cols] == e["argmin"][1][nan_cols]).all()
  for m in (0, 2):
    for key in e:
      assert np.array_equal(e[key][m], ext[key][m])
    for name in got:
      assert np.array_equal(got[name][m], ref[name][m], equal_nan=True)


def _host_fields(r, k, ny, nb_, nt, nn):
  """One member's eight fields in NumPy (:207-262 on arrays), rows r = twobasin_section_rows."""
  itp = np.interp
  bb = (k["A_Atl"] * k["b_Atl"] + k["A_Pac"] * k["b_Pac"]) / (k["A_Atl"] + k["A_Pac"])
  bnew = np.concatenate((k["bsouth"], np.tile(bb, (nb_, 1)), k["btrans"], np.tile(k["bn"], (nn, 1))))
  soA, soP, am, zo = k["Psi_SO_Atl"], k["Psi_SO_Pac"], k["Psi_AMOC"], k["Psi_ZOC"]
  iA, iP = itp(bb, k["b_Atl"], soA), itp(bb, k["b_Pac"], soP)
  PsiSO, Ab, Zb = iA + iP, itp(bb, k["bgrid_AMOC"], k["psib_AMOC"]), itp(bb, k["bgrid_ZOC"], k["psib_ZOC"])
  f = {name: np.zeros_like(bnew) for name in _mod().FIELDS}
  for iy in range(1, bnew.shape[0]):
    c1, c2, c3, x = r["c1"][iy], r["c2"][iy], r["c3"][iy], bnew[iy]
    if iy < ny:
      z = zA = zP = itp(x, bb, soA + soP)
      b = bA = bP = np.where(bb < k["bs_SO"][iy], PsiSO, 0.)
      A = P = itp(x, bb, PsiSO)
    elif iy < ny + nb_:
      z, zA, zP = (c1 * am + c2 * (soA + soP)) / r["lbasin"], (c1 * am + c2 * (soA - zo)) / r["lbasin"], \
          (c2 * (soP + zo)) / r["lbasin"]
      b, bA, bP = (c1 * Ab + c2 * PsiSO) / r["lbasin"], (c1 * Ab + c2 * (iA - Zb)) / r["lbasin"], \
          (c2 * (iP + Zb)) / r["lbasin"]
      A = (c1 * k["psibz_AMOC1"] + c2 * (soA - k["psibz_ZOC1"])) / r["lbasin"]
      P = (c2 * (soP + k["psibz_ZOC2"])) / r["lbasin"]
    else:
      zP = bP = P = np.full_like(x, np.nan)
      if iy < ny + nb_ + nt:
        z, b, A = am, Ab, itp(x, k["bgrid_AMOC"], k["psib_AMOC"])
      else:
        z, b, A = (c3 * am) / r["lnorth"], (c3 * Ab) / r["lnorth"], (c3 * k["psibz_AMOC2"]) / r["lnorth"]
      zA, b = z, np.where(bb < x[-1], b, 0.)
      bA = b
    for name, v in zip(_mod().FIELDS, (z, zA, zP, b, bA, bP, A, P)):
      f[name][iy] = v
  return f, bnew


def test_tiny_shape_and_empty(gpu):
  """nz = 3, ny = 2, nb = 1, one row per region, two members, against NumPy; n = 0 is PM_OK."""
  from pymoc_amd import _lib
  T = _mod()
  rng = np.random.default_rng(5)
  y, z = np.array([0., 2e6]), np.array([-4000., -1000., 0.])
  prof = lambda n: np.sort(rng.uniform(-1e-3, 2e-2, n))  # noqa: E731
  ms = []
  for _ in range(2):
    k = {name: rng.normal(size=3) for name in ("Psi_SO_Atl", "Psi_SO_Pac", "Psi_AMOC", "Psi_ZOC",
                                               "psibz_AMOC1", "psibz_AMOC2", "psibz_ZOC1", "psibz_ZOC2")}
    k.update(b_Atl=prof(3), b_Pac=prof(3), bn=prof(3), bs_SO=prof(2), A_Atl=rng.uniform(5e13, 9e13),
             A_Pac=rng.uniform(1e14, 2e14), bgrid_AMOC=prof(1), psib_AMOC=rng.normal(size=1),
             bgrid_ZOC=prof(1), psib_ZOC=rng.normal(size=1), bsouth=rng.uniform(-1e-3, 2e-2, (2, 3)),
             btrans=rng.uniform(-1e-3, 2e-2, (1, 3)))
    ms.append(k)
  geo = dict(n_basin=1, n_trans=1, n_north=1)
  o = T.TwoBasinOverturningSections(y, z, 1, store=T.STORE, **geo, **_inputs(ms)).compute()
  assert o.nrows == 5 and not o.status().any()
  got = _all(o)
  r = T.twobasin_section_rows(y, **geo)
  for m, k in enumerate(ms):
    want, bnew = _host_fields(r, k, 2, 1, 1, 1)
    for name in T.FIELDS:
      assert np.array_equal(got[name][m], want[name], equal_nan=True), (m, name)
    assert np.array_equal(got["bnew"][m], bnew)
    assert np.array_equal(got["bnew_Atl"][m][2], k["b_Atl"]) and np.array_equal(got["bnew_Pac"][m][2], k["b_Pac"])
    assert np.isnan(got["bnew_Pac"][m][3:]).all() and np.array_equal(got["bnew_Atl"][m][3:], bnew[3:])
  assert _same_extrema(o.extrema(), _np_extrema(got, 3))
  d = o.descriptor()
  d.n = 0
  assert _lib.lib.pm_twobasin_overturning_sections(ctypes.byref(d), None) == _lib.PM_OK
  p = _lib.pm_twobasin_rows()
  p.nz = 3
  assert _lib.lib.pm_twobasin_profiles(ctypes.byref(p), None) == _lib.PM_OK


def _state(ens):
  dl = lambda a: a.download(stream=ens.stream)  # noqa: E731
  return {"b": dl(ens.cols.b), "Psi_AMOC": dl(ens.amoc.Psi), "Psi_ZOC": dl(ens.zoc.Psi),
          "psibz_AMOC": dl(ens.amoc.psibz), "psibz_ZOC": dl(ens.zoc.psibz),
          "Psi_SO_Atl": dl(ens.so_atl.Psi), "Psi_SO_Pac": dl(ens.so_pac.Psi), "wA": dl(ens.wA)}


def test_ensemble_route(gpu):
  """from_ensemble on a live two-basin ensemble: equal to the explicit route fed with the
  downloaded private rows; the preparation kernel against NumPy; the ensemble left alone."""
  import pymoc_amd
  from pymoc_amd import configs
  T = _mod()
  cfg = configs.config_twobasin(N=64)
  a, b = pymoc_amd.TwoBasinEnsemble(cfg), pymoc_amd.TwoBasinEnsemble(cfg)
  a.run(49)
  b.run(49)
  assert a.ii % a.M == 1  # right after an update: the fresh solve is the script's
  before = _state(a)
  o = T.TwoBasinOverturningSections.from_ensemble(a, cfg, store=T.STORE).compute()
  dl = lambda x: x.download(stream=a.stream)  # noqa: E731
  n, nz = a.n, a.nz
  rows = dict(b_Atl=before["b"][:n], b_Pac=before["b"][2 * n:], A_Atl=cfg["A_Atl"], A_Pac=cfg["A_Pac"],
              bs_SO=dl(a.bs_SO), Psi_SO_Atl=dl(o.so_atl.Psi), Psi_SO_Pac=dl(o.so_pac.Psi),
              Psi_AMOC=dl(o.amoc.Psi), Psi_ZOC=dl(o.zoc.Psi), psibz_AMOC1=dl(o.amoc.psibz)[:n],
              psibz_AMOC2=dl(o.amoc.psibz)[n:], psibz_ZOC1=dl(o.zoc.psibz)[:n],
              psibz_ZOC2=dl(o.zoc.psibz)[n:], bgrid_AMOC=dl(o.amoc.bgrid), psib_AMOC=dl(o.amoc.psib),
              bgrid_ZOC=dl(o.zoc.bgrid), psib_ZOC=dl(o.zoc.psib), bsouth=dl(o.channel.out),
              btrans=dl(o.trans.out), bn=dl(o.bn))
  x = T.TwoBasinOverturningSections(cfg["y"], cfg["z"], int(cfg["nb"]), store=T.STORE, **rows).compute()
  assert o.n == x.n == 64 and o.nrows == 151
  for name in T.STORE:
    assert np.array_equal(o.download(name), x.download(name), equal_nan=True), name
  assert _same_extrema(o.extrema(), x.extrema())
  assert np.array_equal(o.status(), x.status())
  ok = o.status() == 0  # (members whose section has a failing point are reported, not compared)
  assert ok.any() and np.isfinite(o.extrema()["max"][ok]).all()
  # the preparation kernel
  A_Atl, A_Pac = cfg["A_Atl"][:, None], cfg["A_Pac"][:, None]
  want = (A_Atl * rows["b_Atl"] + A_Pac * rows["b_Pac"]) / (A_Atl + A_Pac)
  assert np.array_equal(dl(o.b_basin), want)
  assert np.array_equal(rows["bn"][:, 1:], before["b"][n:2 * n, 1:]) and np.array_equal(rows["bn"][:, 0], want[:, 0])
  # right after an update the private solves are the ensemble's own
  assert np.array_equal(rows["Psi_AMOC"], before["Psi_AMOC"], equal_nan=True)
  assert np.array_equal(dl(o.zoc.psibz), before["psibz_ZOC"], equal_nan=True)
  assert np.array_equal(rows["Psi_SO_Pac"], before["Psi_SO_Pac"], equal_nan=True)
  # the ensemble was left alone, and goes on as its undisturbed twin
  mid = _state(a)
  for key in before:
    assert np.array_equal(before[key], mid[key], equal_nan=True), key
  a.run(30)
  o.compute()
  a.run(17)
  b.run(47)
  sa, sb = _state(a), _state(b)
  for key in sa:
    assert np.array_equal(sa[key], sb[key], equal_nan=True), key


def test_status_bits_and_isolation(cases):
  from pymoc_amd import _lib
  k = cases["nominal_s0121"]
  ks = [k] * 10
  clean = _explicit(ks)
  want, ec = _all(clean), clean.extrema()
  args = _inputs(ks)
  args["btrans"][1, 3, 5] = np.nan                   # a section point where brenth raised
  args["bsouth"][2, 17, 40] = np.nan
  args["bn"][3, 79] = np.nan
  args["b_Atl"][4, [60, 61]] = args["b_Atl"][4, [61, 60]]  # decreasing
  assert args["b_Atl"][4, 61] < args["b_Atl"][4, 60]
  args["b_Pac"][5, 12] = np.inf
  args["bgrid_AMOC"][6, 100] = args["bgrid_AMOC"][6, 98]
  args["bgrid_ZOC"][7, 499] = np.nan
  args["A_Pac"][8] = np.nan                          # b_basin alone
  o = _explicit(ks, **args)
  st = o.status()
  B = _lib
  assert st.tolist()[:4] == [0, 1, 1, 1] and st[9] == 0
  assert st[4] & B.PM_TBO_BAD_ATL and not st[4] & (B.PM_TBO_BAD_PAC | B.PM_TBO_NAN_SECTION)
  assert st[5] & B.PM_TBO_BAD_PAC and st[5] & B.PM_TBO_BAD_BASIN and not st[5] & B.PM_TBO_BAD_ATL
  assert st[6] == B.PM_TBO_BAD_BGRID_AMOC and st[7] == B.PM_TBO_BAD_BGRID_ZOC
  assert st[8] == B.PM_TBO_BAD_BASIN
  got, e = _all(o), o.extrema()
  for m in (0, 9):  # the clean neighbours
    for name in got:
      assert np.array_equal(got[name][m], want[name][m], equal_nan=True), (name, m)
    for key in e:
      assert np.array_equal(e[key][m], ec[key][m])
  assert np.isnan(got["bnew"][1, 51 + 60 + 3, 5]) and np.isnan(got["bnew_Atl"][3, 131:, 79]).all()


def test_host_validation_and_limits(gpu, cases):
  from pymoc_amd import _lib, DeviceArray
  import pymoc_amd
  T = _mod()
  k = cases["nominal_s0121"]
  y, z, nb = k["y"], k["z"], k["nb"]
  good = _inputs([k, k])
  OS = T.TwoBasinOverturningSections
  OS(y, z, nb, **good).compute()
  OS(y, z, nb, **dict(good, A_Atl=7e13, A_Pac=np.float64(1.7e14))).compute()
  for name, bad in (("b_Atl", good["b_Atl"][:, :-1]), ("bs_SO", good["bs_SO"][:, 1:]),
                    ("bgrid_ZOC", good["bgrid_ZOC"][:, :499]), ("bsouth", good["bsouth"][:, :, :-1]),
                    ("btrans", good["btrans"][:, :19]), ("Psi_ZOC", good["Psi_ZOC"][:1].repeat(3, axis=0)),
                    ("A_Pac", good["A_Pac"][:, None]), ("psibz_ZOC2", good["psibz_ZOC2"].astype(np.float32)[None])):
    with pytest.raises(ValueError):
      OS(y, z, nb, **dict(good, **{name: bad}))
  with pytest.raises(ValueError, match="required"):
    OS(y, z, nb, **dict(good, bn=None))
  with pytest.raises(TypeError):
    OS(y, z, nb, **dict(good, Psi_AMOC=[1., 2.]))
  with pytest.raises(TypeError, match="unknown"):
    OS(y, z, nb, b_basin=good["b_Atl"], **good)
  with pytest.raises(ValueError, match="store"):
    OS(y, z, nb, store=("psiarray_res",), **good)
  # rows running past the end of a device array
  dev = DeviceArray.from_host(good["Psi_AMOC"])
  OS(y, z, nb, **dict(good, Psi_AMOC=dev))
  OS(y, z, nb, **dict(good, Psi_AMOC=(dev, z.size, 0)))
  for tup in ((dev, 1, z.size), (dev, 0, z.size + 1), (dev, 2 * z.size, 0)):
    with pytest.raises(ValueError, match="past the end"):
      OS(y, z, nb, **dict(good, Psi_AMOC=tup))
  with pytest.raises(ValueError, match="n is needed"):
    OS(y, z, nb, **{a: DeviceArray.from_host(b) for a, b in good.items()})
  # limits
  with pytest.raises(ValueError, match="2048"):
    OS(y, z, 2049, **good)
  with pytest.raises(ValueError, match="1024"):
    OS(y, np.linspace(-4000., 0., 1025), nb, **good)
  with pytest.raises(ValueError, match="LDS"):
    OS(y, np.linspace(-4000., 0., 1024), 2048, **good)
  with pytest.raises(ValueError):
    OS(y, z, nb, n_basin=1000, n_trans=20, n_north=5, **good)
  # ... and through the raw C-ABI
  o = OS(y, z, nb, **good)  # (owns the device memory the descriptors point to)
  d = o.descriptor()
  assert _lib.lib.pm_twobasin_overturning_sections(ctypes.byref(d), None) == _lib.PM_OK
  for field, v in (("nb", 2049), ("nz", 1025), ("ny", 1), ("n_basin", 1020), ("n_trans", 0), ("c3", None)):
    d = o.descriptor()
    setattr(d, field, v)
    assert _lib.lib.pm_twobasin_overturning_sections(ctypes.byref(d), None) == _lib.PM_EINVAL, field
  d = o.descriptor()
  d.nz, d.nb = 1024, 2048  # 177 KB of LDS
  assert _lib.lib.pm_twobasin_overturning_sections(ctypes.byref(d), None) == _lib.PM_EINVAL
  assert "LDS" in _lib.lib.pm_last_error().decode()
  d = o.descriptor()
  d.bn.ptr = None
  assert _lib.lib.pm_twobasin_overturning_sections(ctypes.byref(d), None) == _lib.PM_EINVAL
  need = ctypes.c_size_t(0)
  assert _lib.lib.pm_twobasin_overturning_lds_bytes(512, 512, 2048, ctypes.byref(need)) == _lib.PM_OK
  assert 104 * 1024 < need.value <= 106 * 1024
  pymoc_amd.synchronize()
  # the largest shape the issue asks for runs: nz = ny = 512, nb = 2048 (105 KB of LDS)
  rng = np.random.default_rng(11)
  zb, yb = np.linspace(-4000., 0., 512), np.linspace(0., 2e6, 512)
  prof = lambda n: np.sort(rng.uniform(-1e-3, 2e-2, n))  # noqa: E731
  big = {name: rng.normal(size=512) for name in ("Psi_SO_Atl", "Psi_SO_Pac", "Psi_AMOC", "Psi_ZOC",
                                                 "psibz_AMOC1", "psibz_AMOC2", "psibz_ZOC1", "psibz_ZOC2")}
  big.update(b_Atl=prof(512), b_Pac=prof(512), bn=prof(512), bs_SO=prof(512), A_Atl=7e13, A_Pac=1.7e14,
             bgrid_AMOC=prof(2048), psib_AMOC=rng.normal(size=2048), bgrid_ZOC=prof(2048),
             psib_ZOC=rng.normal(size=2048), bsouth=rng.uniform(-1e-3, 2e-2, (512, 512)),
             btrans=rng.uniform(-1e-3, 2e-2, (3, 512)))
  geo = dict(n_basin=2, n_trans=3, n_north=2)
  o = OS(yb, zb, 2048, n=2, store=("psiarray_Atl", "psiarray_b_Pac", "psiarray_z"), **geo, **big).compute()
  assert o.nrows == 519 and not o.status().any()
  want, _ = _host_fields(T.twobasin_section_rows(yb, **geo), big, 512, 2, 3, 2)
  for name in o.store:
    got = o.download(name)
    assert np.array_equal(got[0], got[1], equal_nan=True), name
    for iy in (0, 1, 300, 511, 512, 513, 514, 516, 517, 518):
      assert np.array_equal(got[0, iy], want[name][iy], equal_nan=True), (name, iy)


def test_example_script(gpu):
  import os
  import subprocess
  import sys
  from conftest import ROOT
  p = subprocess.run([sys.executable, os.path.join("examples", "twobasin_overturning.py"),
                      "--members", "32", "--steps", "49"], cwd=ROOT, capture_output=True, text=True,
                     timeout=300)
  assert p.returncode == 0, p.stdout + p.stderr
  assert "equals the explicit route on the downloaded rows: True" in p.stdout
  assert "equals NumPy on the host: True" in p.stdout
