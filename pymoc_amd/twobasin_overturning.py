"""TwoBasinOverturningSections: what the reference's two-basin script builds after its loop, for
every member of an ensemble, on the GPU.

Arithmetic contract: examples/twobasin_NadeauJansen.py:157-262 of the reference -- the eight
overturning fields psiarray_z / _z_Atl / _z_Pac (depth space), psiarray_b / _b_Atl / _b_Pac
(isopycnal), psiarray_Atl / _Pac (residual) and the buoyancy sections bnew / bnew_Atl / bnew_Pac on
the section channel + basin + northern transition + northern sinking region that :173-205
assemble -- bit-identical: one launch of pm_twobasin_overturning_sections
(pymoc_amd/csrc/twobasin_overturning.hip) for all members, after pm_twobasin_profiles (:161,
:192-193) and two SectionBatch launches, plus each member's extrema of the eight fields.
"""
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import check, lib, pm_twobasin_overturning, pm_twobasin_rows
from .device import DeviceArray, _sh
from .overturning import OverturningSections

# PM_TBO_Z .. PM_TBO_PAC: the order of extrema()'s columns
FIELDS = ("psiarray_z", "psiarray_z_Atl", "psiarray_z_Pac", "psiarray_b", "psiarray_b_Atl",
          "psiarray_b_Pac", "psiarray_Atl", "psiarray_Pac")
SECTIONS = ("bnew", "bnew_Atl", "bnew_Pac")
STORE = FIELDS + SECTIONS
STATUS_BITS = {"nan_section": _lib.PM_TBO_NAN_SECTION, "b_basin": _lib.PM_TBO_BAD_BASIN,
               "b_Atl": _lib.PM_TBO_BAD_ATL, "b_Pac": _lib.PM_TBO_BAD_PAC,
               "bgrid_AMOC": _lib.PM_TBO_BAD_BGRID_AMOC, "bgrid_ZOC": _lib.PM_TBO_BAD_BGRID_ZOC}


def twobasin_section_rows(y, lbasin_km=11000., ltrans_km=1500., lnorth_km=400., n_basin=60,
                          n_trans=20, n_north=20):
  """The section's row coordinate and what the script forms from it, in NumPy float64 and the
  script's own order (twobasin_NadeauJansen.py:173-202, :228-259; lengths in km):
    ynew         concatenate(y/1e3, ybasin, ytrans, ynorth); ybasin starts AT the channel's end
                 (linspace(0, lbasin, n_basin): Plot_overturning.py starts one step further north)
    c1, c2, c3   ynew - lchannel, lchannel + lbasin - ynew, lchannel + lbasin + ltrans + lnorth - ynew
    y_trans      the transition interpolator's own axis, ytrans*1000. - ytrans[0]*1000.
  """
  y = np.ascontiguousarray(y, dtype=np.float64)
  lbasin, ltrans, lnorth = float(lbasin_km), float(ltrans_km), float(lnorth_km)
  lchannel = y[-1] / 1e3
  ybasin = np.linspace(0, lbasin, int(n_basin)) + lchannel
  ytrans = np.linspace(ltrans / float(n_trans), ltrans, int(n_trans)) + lchannel + lbasin
  ynorth = np.linspace(lnorth / float(n_north), lnorth, int(n_north)) + lchannel + lbasin + ltrans
  ynew = np.concatenate((y / 1e3, ybasin, ytrans, ynorth))
  return dict(ynew=ynew, c1=ynew - lchannel, c2=lchannel + lbasin - ynew,
              c3=lchannel + lbasin + ltrans + lnorth - ynew,
              y_trans=ytrans * 1000. - ytrans[0] * 1000., lchannel=lchannel, lbasin=lbasin,
              ltrans=ltrans, lnorth=lnorth)


class TwoBasinOverturningSections(object):
  """n members' two-basin overturning sections on shared grids.

  y, z      the channel's meridional grid (m) and the vertical grid, 2..1024 points each.
  nb        isopycnal classes of both thermal winds' bgrid / psib (<= 2048).
  n         member count (needed when no input is a host array with a member axis).
  Inputs, per member (objects as in the script):
    b_Atl, b_Pac [nz]            Atl.b, Pac.b;       A_Atl, A_Pac   the basins' areas (one number);
    bs_SO [ny]                   the RAW channel surface buoyancy (not the copy :176 fixes up);
    Psi_SO_Atl, Psi_SO_Pac, Psi_AMOC, Psi_ZOC [nz]   SO_Atl.Psi, SO_Pac.Psi, AMOC.Psi, ZOC.Psi;
    psibz_AMOC1, psibz_AMOC2 [nz]   AMOC.Psibz(nb)[0], [1];   psibz_ZOC1, psibz_ZOC2   ZOC.Psibz()[0], [1];
    bgrid_AMOC, psib_AMOC, bgrid_ZOC, psib_ZOC [nb]  AMOC.bgrid, AMOC.Psib(nb), ZOC.bgrid, ZOC.Psib();
    bsouth [ny][nz], btrans [n_trans][nz]   the channel and transition sections (SectionBatch);
    bn [nz]                      b_north with bn[0] = b_basin[0] (profiles() forms it).
  Each is a host array with or without a leading member axis, a DeviceArray holding the rows in
  place, or a tuple (DeviceArray, offset, stride) in doubles, as for OverturningSections; the areas
  may be plain numbers.  The inputs are taken as they are: overturnings that are older than the
  columns (the script's, up to MOC_up_iters - 1 steps) give the script's fields.
  lbasin_km, ltrans_km, lnorth_km, n_basin, n_trans, n_north   the script's 11000., 1500., 400.,
            60, 20 and 20.
  store     which of FIELDS and 'bnew', 'bnew_Atl', 'bnew_Pac' go to device memory, each
            [n][nrows][nz] and an attribute of that name (None when not stored); the extrema and
            the status are always computed.
  The member's rows are staged in one workgroup's LDS: nz = ny = 512 with nb = 2048 fits, nz = 1024
  with nb = 2048 does not (ValueError).

  compute() is one launch; ynew is the row coordinate in km, extrema() and status() the
  per-member numbers.
  """

  ROWS = pm_twobasin_overturning.ROWS

  def __init__(self, y, z, nb, n=None, lbasin_km=11000., ltrans_km=1500., lnorth_km=400.,
               n_basin=60, n_trans=20, n_north=20, store=FIELDS, stream=None, **inputs):
    _lib.require_device()
    self.stream = stream
    self.y_host = np.ascontiguousarray(y, dtype=np.float64)
    self.z_host = np.ascontiguousarray(z, dtype=np.float64)
    if self.y_host.ndim != 1 or self.z_host.ndim != 1:
      raise ValueError("y and z must be 1-D grids")
    ny, nz = self.y_host.size, self.z_host.size
    self.ny, self.nz, self.nb = ny, nz, int(nb)
    self.n_basin, self.n_trans, self.n_north = int(n_basin), int(n_trans), int(n_north)
    lim = _lib.PM_TBO_MAX_LEVELS
    if not (2 <= ny <= lim and 2 <= nz <= lim):
      raise ValueError("y and z hold 2..%d points (got %d, %d)" % (lim, ny, nz))
    if not 1 <= self.nb <= _lib.PM_TBO_MAX_NB:
      raise ValueError("nb must be 1..%d (got %d)" % (_lib.PM_TBO_MAX_NB, self.nb))
    if min(self.n_basin, self.n_trans, self.n_north) < 1 or \
        self.n_basin + self.n_trans + self.n_north > lim:
      raise ValueError("n_basin, n_trans and n_north must be >= 1 and together <= %d" % lim)
    need = C.c_size_t(0)
    check(lib.pm_twobasin_overturning_lds_bytes(nz, ny, self.nb, C.byref(need)))
    if need.value > _lib.LDS_PER_CU:
      raise ValueError("nz = %d, ny = %d, nb = %d need %d bytes of LDS per member, a workgroup "
                       "has %d" % (nz, ny, self.nb, need.value, _lib.LDS_PER_CU))
    store = tuple(store)
    for s in store:
      if s not in STORE:
        raise ValueError("store holds names of %s, not %r" % (", ".join(STORE), s))
    self.store = store
    self.rows = twobasin_section_rows(self.y_host, lbasin_km, ltrans_km, lnorth_km, self.n_basin,
                                      self.n_trans, self.n_north)
    self.ynew = self.rows["ynew"]
    self.nrows = self.ynew.size
    unknown = sorted(set(inputs) - set(self.ROWS))
    if unknown:
      raise TypeError("unknown inputs: %s" % ", ".join(unknown))
    shapes = {"A_Atl": (), "A_Pac": (), "bs_SO": (ny,), "bsouth": (ny, nz),
              "btrans": (self.n_trans, nz)}
    for name in ("bgrid_AMOC", "psib_AMOC", "bgrid_ZOC", "psib_ZOC"):
      shapes[name] = (self.nb,)
    self._keep, counts = [], []
    self.inputs, self._shapes = {}, {}
    for name in self.ROWS:
      self._shapes[name] = shapes.get(name, (nz,))
      self.inputs[name] = self._rows(inputs.get(name), name, self._shapes[name], counts)
    if n is None:
      if not counts:
        raise ValueError("n is needed when no input is a host array with a member axis")
      n = counts[0]
    self.n = int(n)
    for c in counts:
      if c != self.n:
        raise ValueError("inputs hold %d rows, n is %d" % (c, self.n))
    for name in self.ROWS:
      dev, off, stride = self.inputs[name]
      last = off + (self.n - 1) * stride + int(np.prod(self._shapes[name]))
      if self.n > 0 and last * dev.dtype.itemsize > dev.nbytes:
        raise ValueError("%s: member rows run past the end of the device array" % name)
    self._c = [DeviceArray.from_host(self.rows[k], stream=stream) for k in ("c1", "c2", "c3")]
    m = max(self.n, 1)
    for name in STORE:
      setattr(self, name, DeviceArray((m, self.nrows, nz)) if name in store else None)
    self._extrema = DeviceArray((m, len(FIELDS), 2))
    self._extrema_at = DeviceArray((m, len(FIELDS), 2), np.int32)
    self._status = DeviceArray((m,), np.int32)
    self._sources = None  # from_ensemble: what compute() launches first

  def _rows(self, v, name, shape, counts):
    """-> (device array, offset, stride) in doubles: OverturningSections' rule, and plain numbers
    for the per-member scalars."""
    if shape == () and isinstance(v, (numbers.Real, np.ndarray)) and np.ndim(v) == 0:
      d = DeviceArray.from_host(np.array([float(v)]), stream=self.stream)  # shared by every member
      self._keep.append(d)
      return (d, 0, 0)
    return OverturningSections._rows(self, v, name, shape, counts)

  @staticmethod
  def profiles(b_Atl, b_Pac, b_north, A_Atl, A_Pac, n, nz, b_basin=None, bn=None, stream=None):
    """pm_twobasin_profiles: b_basin = (A_Atl*b_Atl + A_Pac*b_Pac)/(A_Atl + A_Pac) (:161) and
    bn = b_north with bn[0] = b_basin[0] (:192-193) of n members, device arrays [n][nz].  Each
    input is (DeviceArray, offset, stride) in doubles."""
    b_basin = DeviceArray((max(n, 1), nz)) if b_basin is None else b_basin
    bn = DeviceArray((max(n, 1), nz)) if bn is None else bn
    d = pm_twobasin_rows()
    d.n, d.nz = n, nz
    for field, (dev, off, stride) in (("b_Atl", b_Atl), ("b_Pac", b_Pac), ("b_north", b_north),
                                      ("A_Atl", A_Atl), ("A_Pac", A_Pac)):
      r = getattr(d, field)
      r.ptr, r.offset, r.stride = dev.ptr, int(off), int(stride)
    d.b_basin, d.bn = b_basin.ptr, bn.ptr
    check(lib.pm_twobasin_profiles(C.byref(d), _sh(stream)))
    return b_basin, bn

  @classmethod
  def from_ensemble(cls, ens, cfg, nb=None, **kw):
    """The sections of a TwoBasinEnsemble's CURRENT state, everything device-resident on the
    ensemble's stream: compute() issues pm_twobasin_profiles, SectionBatch('channel', bs=ens.bs_SO,
    bn=b_basin, fixups='twobasin'), SectionBatch('twocol', y_trans, z, bs=b_Atl, bn=bn), two
    private ThermwindBatch (AMOC, ZOC; store_psib=True) and two private PsiSOBatch solves of the
    current columns into private buffers, and the kernel, with no host round trip.  The
    ensemble's own amoc / zoc / so_atl / so_pac / wA buffers are never written, so taking
    sections between two run() calls leaves the trajectory as it was.

    One difference from the script: the script plots the overturnings of its last update, which
    are up to MOC_up_iters - 1 steps older than the columns; this route solves afresh on the
    current columns.  The two coincide when ens.ii % MOC_up_iters == 1 (right after an update).
    The explicit route takes whatever it is given and reproduces the script in both situations."""
    from .psi_so import PsiSOBatch
    from .sections import SectionBatch
    from .thermwind import ThermwindBatch
    n, nz, ny = ens.n, ens.nz, ens.ny
    y, z = np.asarray(cfg["y"], dtype=np.float64), np.asarray(cfg["z"], dtype=np.float64)
    nb = int(cfg["nb"] if nb is None else nb)
    geo = {k: kw[k] for k in ("lbasin_km", "ltrans_km", "lnorth_km", "n_basin", "n_trans", "n_north")
           if k in kw}
    rows = twobasin_section_rows(y, **geo)
    st, b, zd = ens.stream, ens.cols.b, ens.cols.z
    vec = lambda v: DeviceArray.from_host(  # noqa: E731
        np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))), stream=st)
    A_Atl, A_Pac = vec(cfg["A_Atl"]), vec(cfg["A_Pac"])
    b_basin, bn = DeviceArray((max(n, 1), nz)), DeviceArray((max(n, 1), nz))
    channel = SectionBatch("channel", y, z, bs=ens.bs_SO, bn=b_basin, n=n, fixups="twobasin",
                           stream=st)
    trans = SectionBatch("twocol", rows["y_trans"], z, bs=b, bn=bn, n=n, stream=st)
    amoc = ThermwindBatch(z, n, f=cfg["f_AMOC"], nb=nb, stream=st, z_dev=zd)
    zoc = ThermwindBatch(z, n, f=cfg["f_ZOC"], nb=nb, stream=st, z_dev=zd)
    so = dict(tau=cfg["tau"], KGM=cfg["K"], f=cfg["f_SO"], stream=st, z_dev=zd)
    so_atl = PsiSOBatch(z, y, n, L=cfg["L_Atl"], **so)
    so_pac = PsiSOBatch(z, y, n, L=cfg["L_Pac"], **so)
    self = cls(y, z, nb, n=n, stream=st, b_Atl=(b, 0, nz), b_Pac=(b, 2 * n * nz, nz),
               A_Atl=(A_Atl, 0, 1), A_Pac=(A_Pac, 0, 1), bs_SO=(ens.bs_SO, 0, ny),
               Psi_SO_Atl=so_atl.Psi, Psi_SO_Pac=so_pac.Psi, Psi_AMOC=amoc.Psi, Psi_ZOC=zoc.Psi,
               psibz_AMOC1=(amoc.psibz, 0, nz), psibz_AMOC2=(amoc.psibz, n * nz, nz),
               psibz_ZOC1=(zoc.psibz, 0, nz), psibz_ZOC2=(zoc.psibz, n * nz, nz),
               bgrid_AMOC=amoc.bgrid, psib_AMOC=amoc.psib, bgrid_ZOC=zoc.bgrid, psib_ZOC=zoc.psib,
               bsouth=channel.out, btrans=trans.out, bn=bn, **kw)
    self.b_basin, self.bn = b_basin, bn
    self.channel, self.trans = channel, trans
    self.amoc, self.zoc, self.so_atl, self.so_pac = amoc, zoc, so_atl, so_pac
    self._sources = ens
    return self

  def descriptor(self):
    d = pm_twobasin_overturning()
    d.n, d.nz, d.ny, d.nb = self.n, self.nz, self.ny, self.nb
    d.n_basin, d.n_trans, d.n_north = self.n_basin, self.n_trans, self.n_north
    for name in self.ROWS:
      dev, off, stride = self.inputs[name]
      r = getattr(d, name)
      r.ptr, r.offset, r.stride = dev.ptr, off, stride
    d.c1, d.c2, d.c3 = (c.ptr for c in self._c)
    d.lbasin, d.lnorth = self.rows["lbasin"], self.rows["lnorth"]
    ptr = lambda a: a.ptr if a is not None else None  # noqa: E731
    for f, name in enumerate(FIELDS):
      d.psi[f] = ptr(getattr(self, name))
    d.bnew, d.bnew_Atl, d.bnew_Pac = ptr(self.bnew), ptr(self.bnew_Atl), ptr(self.bnew_Pac)
    d.extrema, d.extrema_at, d.status = self._extrema.ptr, self._extrema_at.ptr, self._status.ptr
    return d

  def prepare(self):
    """from_ensemble only: everything compute() launches before the kernel."""
    ens = self._sources
    n, nz, st = self.n, self.nz, ens.stream
    self.profiles(self.inputs["b_Atl"], self.inputs["b_Pac"], (ens.cols.b, n * nz, nz),
                  self.inputs["A_Atl"], self.inputs["A_Pac"], n, nz, self.b_basin, self.bn, stream=st)
    self.channel.grid()
    self.trans.grid()
    self.so_atl.update(ens.b_Atl, ens.bs_SO)
    self.amoc.update(ens.b_Atl, ens.b_north, store_psib=True)
    self.so_pac.update(ens.b_Pac, ens.bs_SO)
    self.zoc.update(ens.b_Atl, ens.b_Pac, store_psib=True)

  def compute(self, stream=None):
    """The fields, extrema and status of all members: one launch (after the preparation, the
    sections and the four solves, on the same stream, when built with from_ensemble)."""
    if self._sources is not None:
      stream = None  # the private solvers launch on the ensemble's stream, and so does the kernel
      self.prepare()
    return self.launch(stream)

  def launch(self, stream=None):
    """pm_twobasin_overturning_sections alone, on the inputs as they are in device memory."""
    s = self.stream if stream is None else stream
    d = self.descriptor()
    check(lib.pm_twobasin_overturning_sections(C.byref(d), _sh(s)))
    self._last_stream = s
    return self

  def _download(self, arr):
    return arr.download(stream=getattr(self, "_last_stream", self.stream))[:self.n]

  def download(self, name):
    """The stored field or section `name` of the last compute(), host array [n][nrows][nz]."""
    arr = getattr(self, name) if name in STORE else None
    if arr is None:
      raise ValueError("%r is not stored (store=%r)" % (name, self.store))
    return self._download(arr)

  def extrema(self):
    """{'max', 'min': [n][8] float64, 'argmax', 'argmin': [n][8] int32} of the last compute(),
    columns in the order of FIELDS: np.max / np.min over a member's section and np.argmax /
    np.argmin's flat index iy * nz + k (first occurrence; a field with a NaN gives NaN and the
    first NaN's index).  The three Pacific fields over the rows the script defines,
    field[:ny + n_basin]."""
    v, at = self._download(self._extrema), self._download(self._extrema_at)
    return {"max": v[:, :, 0].copy(), "min": v[:, :, 1].copy(),
            "argmax": at[:, :, 0].copy(), "argmin": at[:, :, 1].copy()}

  def status(self):
    """[n] int32 of the last compute(), bits STATUS_BITS: 1 bsouth / btrans / bn hold a NaN (a
    point where the reference's brenth raises: the script would have stopped); 2, 4, 8 b_basin,
    b_Atl, b_Pac non-finite or not non-decreasing; 16, 32 AMOC's, ZOC's bgrid not non-decreasing
    (np.interp's result then depends on its search order)."""
    return self._download(self._status)
