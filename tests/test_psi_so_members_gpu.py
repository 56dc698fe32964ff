"""`so_member` (the body of k_psi_so, compiled into k_so_tw_update and the persistent run kernels
too) on the constructed members of tests/psi_so_cases.py: the outcrop latitudes branch by branch,
the status bits member by member, the wind average and the slope form of calc_GM at the device's
own ys, independence of the batch, the single ops and the caller-supplied ys / tau_ave, and the
one-launch update against the two-launch one.

ys: `south`, `north`, `hit`, `plateau` levels and every level of a `multi` member are the oracle's
bit for bit (the oracle is SciPy's brentq bit for bit on these members:
tests/test_psi_so_cases_cpu.py); a `linear` level lies within the derived bound of the exact root
(psi_so_cases: 8 eps |offset| + eps |exact|) -- brentq's own answer is up to 164 (xtol + rtol |x|)
from that root, which is the reference's conditioning, so no tolerance against it is set there.

Status bit 0 is compared with the definition (bs descends somewhere north of its first minimum):
`bump` and `late_bump`, and `min_tie` as well -- between two separate nodes that hold the minimum
bs rises and comes down again, so a tie with the first node counting is always such a member."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import psi_so_cases as K
from conftest import relerr
from pymoc_amd import configs

pytestmark = pytest.mark.gpu

TOL_DIRECT = 1e-13  # tests/test_psi_so_gpu.py: everything but the GM boundary-value problem
FIELDS = ("ys", "Ek_raw", "GM_raw", "Psi", "Psi_Ek", "Psi_GM")
KINDS = ("scalar", "array")


def _batch(gpu, c, rows, kind, opts, tau=None):
  rows = list(rows)
  return gpu.PsiSOBatch(c.z, c.y, len(rows), tau=c.tau(kind)[rows] if tau is None else tau,
                        KGM=c.KGM[rows], diagnostics=True, **dict(K.PAR, **opts))


def _update(t, b, bs, ops=3, ys_in=None, tau_ave_in=None):
  from pymoc_amd._lib import check, lib
  from pymoc_amd.device import _sh
  d = t.descriptor(b, bs)
  d.ys_in = ys_in.ptr if ys_in is not None else None
  d.tau_ave_in = tau_ave_in.ptr if tau_ave_in is not None else None
  check(lib.pm_psi_so_update(C.byref(d), int(ops), _sh(t.stream)))


def _download(t):
  out = {k: getattr(t, k).download() for k in FIELDS}
  out["status"] = t.status.download()
  return out


def _run(gpu, c, rows, kind, opts, b=None, bs=None, tau=None):
  from pymoc_amd.device import DeviceArray
  rows = list(rows)
  t = _batch(gpu, c, rows, kind, opts, tau=tau)
  t.update(DeviceArray.from_host(c.b[rows] if b is None else b),
           DeviceArray.from_host(c.bs[rows] if bs is None else bs))
  return _download(t)


@functools.lru_cache(maxsize=None)
def _whole(gpu, nz, ny, kind, oi):
  """The whole batch of a grid, launched once per (tau kind, option set)."""
  c = K.case(nz, ny)
  return _run(gpu, c, range(c.n), kind, K.OPTIONS[oi])


@functools.lru_cache(maxsize=None)
def _oracle_ys(nz, ny):
  """[n][nz]; NaN for `nan` levels and the nan_bs member."""
  c = K.case(nz, ny)
  out = np.full((c.n, nz), np.nan)
  for m in range(c.n):
    if c.branches[m] is None:
      continue
    for i, v in enumerate(c.b[m]):
      if c.branches[m][i] != "nan":
        out[m, i], st = O.psi_so_ys(c.y, c.bs[m], v)
        assert st == 0
  return out


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_ys_level_by_level_by_branch(gpu, nz, ny):
  c = K.case(nz, ny)
  ys = _whole(gpu, nz, ny, "scalar", 0)["ys"]
  for kind in KINDS:  # ys depends on neither tau nor the tapers
    for oi in range(len(K.OPTIONS)):
      assert K.same(_whole(gpu, nz, ny, kind, oi)["ys"], ys), (kind, oi)
  want = _oracle_ys(nz, ny)
  wrong, worst, nlin = {}, 0., 0
  for m in range(c.n):
    if c.branches[m] is None:
      continue
    for i, v in enumerate(c.b[m]):
      br = c.branches[m][i]
      if br == "nan":
        ok = np.isnan(ys[m, i])
      elif br == "linear":
        r = K.bound_ratio(ys[m, i], *K.exact_root(c.y, c.bs[m], v)) if np.isfinite(ys[m, i]) else np.inf
        worst, nlin = max(worst, r), nlin + 1
        ok = r <= 1.
      else:
        ok = ys[m, i] == want[m, i]
      if not ok:
        wrong.setdefault((c.names[m], br), []).append((m, i, float(ys[m, i]), float(want[m, i])))
  print("nz=%d ny=%d: %d linear levels, worst error / bound %.3f; off: %s" % (
      nz, ny, nlin, worst, {k: (len(v), max(abs(a - b) for _, _, a, b in v)) for k, v in wrong.items()}))
  assert not wrong, {k: v[:3] for k, v in wrong.items()}


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_status_bits_member_by_member(gpu, nz, ny):
  c = K.case(nz, ny)
  assert set(c.members("bump", "late_bump")) <= set(c.multi())
  for kind in KINDS:
    for oi in range(len(K.OPTIONS)):
      r = _whole(gpu, nz, ny, kind, oi)
      st = r["status"]
      print("nz=%d ny=%d %s %d: status %s" % (nz, ny, kind, oi, st.tolist()))
      assert [m for m in range(c.n) if st[m] & 1] == c.multi()
      assert [m for m in range(c.n) if st[m] & 4] == c.members("nan_bs")
      assert [m for m in range(c.n) if st[m] & 2] == [m for m in range(c.n)
                                                      if not np.isfinite(r["Psi"][m]).all()]
      assert np.all(st & 8 == 0) and np.all(st & ~15 == 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_transports_at_the_device_ys(gpu, nz, ny, kind):
  c = K.case(nz, ny)
  for oi, opts in enumerate(K.OPTIONS):
    r = _whole(gpu, nz, ny, kind, oi)
    assert np.all(r["Psi"][:, 0] == 0.)
    for m in range(c.n):
      if c.names[m] == "nan_bs":
        continue
      ys = r["ys"][m]
      assert np.all(np.isnan(r["Ek_raw"][m][np.isnan(ys)]))
      ref = K.solve_at(ys, c, m, kind, opts)
      for k in ("Ek_raw", "Psi_Ek", "GM_raw", "Psi_GM", "Psi"):
        e = relerr(r[k][m], ref[k])
        assert e <= TOL_DIRECT, (nz, ny, kind, oi, m, c.names[m], k, e)


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_a_member_does_not_depend_on_its_batch(gpu, nz, ny):
  c = K.case(nz, ny)
  keys = FIELDS + ("status",)
  for kind, oi in (("array", 1), ("scalar", 0)):
    whole = _whole(gpu, nz, ny, kind, oi)
    opts = K.OPTIONS[oi]
    for m in (5, 8):  # the same member in every row
      r = _run(gpu, c, [m] * c.n, kind, opts)
      for k in keys:
        for row in range(c.n):
          assert K.same(r[k][row], whole[k][m]), (kind, m, k, row)
    for rows in ([6], list(range(3, 9))):  # one member alone; six members as a batch of their own
      r = _run(gpu, c, rows, kind, opts)
      for k in keys:
        assert K.same(r[k], whole[k][rows]), (kind, rows, k)


@pytest.mark.parametrize("nz,ny", K.GRIDS)
def test_single_ops_and_caller_supplied_ys_and_wind_average(gpu, nz, ny):
  from pymoc_amd import _lib
  from pymoc_amd.device import DeviceArray
  c = K.case(nz, ny)
  rng = np.random.default_rng(nz + ny)
  b, bs = DeviceArray.from_host(c.b), DeviceArray.from_host(c.bs)
  for kind, oi in (("array", 1), ("scalar", 0)):
    opts = K.OPTIONS[oi]
    whole = _whole(gpu, nz, ny, kind, oi)
    ok = [m for m in range(c.n) if c.names[m] != "nan_bs"]
    # calc_Ekman() alone: Psi_Ek and Ek_raw (and ys); Psi, Psi_GM and GM_raw are not touched
    t = _batch(gpu, c, range(c.n), kind, opts)
    for k in ("Psi", "Psi_GM", "GM_raw", "Psi_Ek", "Ek_raw"):
      getattr(t, k).upload(K.sentinel((c.n, nz)))
    _update(t, b, bs, ops=_lib.PM_SO_OP_EKMAN)
    r = _download(t)
    for k in ("Psi", "Psi_GM", "GM_raw"):
      assert K.is_sentinel(r[k]), (kind, k)
    for k in ("Psi_Ek", "Ek_raw", "ys"):
      assert K.same(r[k], whole[k]), (kind, k)
    # calc_GM() alone reads the caller's Psi_Ek: the limit of :329-330 is taken against it
    ek_in = rng.uniform(-5., 25., (c.n, nz))
    t = _batch(gpu, c, range(c.n), kind, opts)
    t.Psi_Ek.upload(ek_in)
    t.Ek_raw.upload(K.sentinel((c.n, nz)))
    _update(t, b, bs, ops=_lib.PM_SO_OP_GM)
    r = _download(t)
    assert K.is_sentinel(r["Ek_raw"]) and K.same(r["Psi_Ek"], ek_in) and K.same(r["ys"], whole["ys"])
    limited = 0
    for m in ok:
      gm = K.gm_raw_noc(r["ys"][m], c.z, c.y, c.KGM[m], Psi_Ek=ek_in[m], **dict(K.PAR, **opts))
      free = K.gm_raw_noc(r["ys"][m], c.z, c.y, c.KGM[m], Psi_Ek=np.full(nz, np.inf), **dict(K.PAR, **opts))
      limited += int(np.count_nonzero(gm != free))
      psi = ek_in[m] + gm / 1e6
      psi[0] = 0.
      assert relerr(r["GM_raw"][m], gm) <= TOL_DIRECT, (kind, m)
      assert relerr(r["Psi_GM"][m], gm / 1e6) <= TOL_DIRECT, (kind, m)
      assert relerr(r["Psi"][m], psi) <= TOL_DIRECT, (kind, m)
    assert limited > 0 or nz < 24
    # ys_in = the ys of the whole launch: every output again, bit for bit
    ys_in = DeviceArray.from_host(whole["ys"])
    t = _batch(gpu, c, range(c.n), kind, opts)
    _update(t, b, bs, ys_in=ys_in)
    r = _download(t)
    for k in FIELDS:
      assert K.same(r[k][ok], whole[k][ok]), (kind, k)
    assert np.array_equal(r["status"], whole["status"])
    # ... and with tau_ave_in = the wind average over 100 points north of those ys, which the device
    # does not store: NumPy's own (the kernel restates np.linspace, np.interp and np.mean's
    # pairwise sum operation by operation)
    tau = c.tau(kind)
    ave = np.array([K.wind_average(whole["ys"][m], c.y, tau[m] if kind == "array" else float(tau[m]))
                    for m in range(c.n)])
    t = _batch(gpu, c, range(c.n), kind, opts)
    _update(t, b, bs, ys_in=ys_in, tau_ave_in=DeviceArray.from_host(ave))
    r = _download(t)
    for k in FIELDS:
      assert K.same(r[k][ok], whole[k][ok]), (kind, k, "tau_ave_in")


@pytest.mark.parametrize("nz,ny", [(65, 65), (200, 51)])
def test_shared_body_one_update_launch_on_these_members(gpu, nz, ny):
  """pm_so_tw_update compiles so_member in: a JN2018Ensemble whose b_basin and bs_SO are the case's
  arrays, one MOC update, in one launch and in two; and the stand-alone launch on the same data."""
  from pymoc_amd.device import DeviceArray
  c = K.case(nz, ny)
  cfg = dict(configs.config5(N=c.n, nz=nz, ny=ny, dt_days=10.), y=c.y)
  got = []
  for one in (True, False):
    e = gpu.JN2018Ensemble(dict(cfg, one_update_launch=one), fused_run=False)
    assert e._one_update_launch == one
    e.b_basin.upload(c.b)
    e.ml.bs.upload(c.bs)
    e.moc_update()
    got.append(dict(Psi=e.so.Psi.download(), Psi_Ek=e.so.Psi_Ek.download(),
                    Psi_GM=e.so.Psi_GM.download(), status=e.so.status.download(),
                    Psi_SO=e.state()["Psi_SO"]))
  for k in got[0]:
    assert K.same(got[0][k], got[1][k]), k
  t = gpu.PsiSOBatch(cfg["z"], c.y, c.n, tau=cfg["tau"], KGM=cfg["KGM"], f=cfg["f"], L=cfg["L"])
  t.update(DeviceArray.from_host(c.b), DeviceArray.from_host(c.bs))
  assert K.same(got[0]["Psi_SO"], t.Psi.download())
  assert K.same(got[0]["Psi_Ek"], t.Psi_Ek.download()) and K.same(got[0]["Psi_GM"], t.Psi_GM.download())
  st = t.status.download()
  assert np.array_equal(got[0]["status"], st)
  assert [m for m in range(c.n) if st[m] & 1] == c.multi()
