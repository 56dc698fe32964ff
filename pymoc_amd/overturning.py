"""OverturningSections: the three overturning streamfunction sections of the reference's figure
script for every member of an ensemble, on the GPU.

Arithmetic contract: examples/Plot_overturning.py:73-92 of the reference -- psiarray_z (depth
space), psiarray_b (isopycnal) and psiarray_res (residual) on the section channel + basin + north
that :52-71 assemble -- bit-identical, one launch of pm_overturning_sections
(pymoc_amd/csrc/overturning.hip) for all members, plus each member's extrema of the three fields
(how strong and where each cell is).

Out of scope here: the eight fields of the two-basin script (twobasin_NadeauJansen.py:207-262:
two basins' z / b / residual sections and their sums over a transition region) are built by
TwoBasinOverturningSections (pymoc_amd/twobasin_overturning.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, pm_overturning
from .device import DeviceArray, _sh

FIELDS = ("z", "b", "res")  # PM_OVT_Z, PM_OVT_B, PM_OVT_RES: the order of extrema()'s columns
STORE = FIELDS + ("bnew",)


def section_rows(y, lbasin_km=12000., lnorth_km=1000., n_basin=60, n_north=10):
  """The section's row coordinate and what the script forms from it, in NumPy float64 and the
  script's own order (Plot_overturning.py:56-70, :84-90; lengths in km):
    ynew                 concatenate(y/1e3, ybasin, ynorth)
    c1, c2, c3           ynew - lchannel, lchannel + lbasin - ynew, lchannel + lbasin + lnorth - ynew
    y_north              the northern interpolator's own axis, ynorth*1000. - ynorth[0]*1000.
  """
  y = np.ascontiguousarray(y, dtype=np.float64)
  lbasin, lnorth = float(lbasin_km), float(lnorth_km)
  lchannel = y[-1] / 1e3
  ybasin = np.linspace(lbasin / float(n_basin), lbasin, int(n_basin)) + lchannel
  ynorth = np.linspace(lnorth / float(n_north), lnorth, int(n_north)) + lchannel + lbasin
  ynew = np.concatenate((y / 1e3, ybasin, ynorth))
  return dict(ynew=ynew, c1=ynew - lchannel, c2=lchannel + lbasin - ynew,
              c3=lchannel + lbasin + lnorth - ynew, y_north=ynorth * 1000. - ynorth[0] * 1000.,
              lchannel=lchannel, lbasin=lbasin, lnorth=lnorth)


class OverturningSections(object):
  """n members' overturning sections on shared grids.

  y, z      the channel's meridional grid (m) and the vertical grid, 2..1024 points each.
  nb        isopycnal classes of bgrid / psib (<= 2048).
  n         member count (needed when no input is a host array with a member axis).
  Inputs, per member (names as in the script):
    b_basin [nz], bs_SO [ny]   the RAW state rows (not the copies the script fixes up);
    Psi [nz], bgrid [nb], psib [nb], psibz [nz]   AMOC.Psi, AMOC.bgrid, AMOC.Psib(nb), AMOC.Psibz(nb)[0];
    Psi_SO [nz]                PsiSO.Psi;
    bsouth [ny][nz], bnorth [n_north][nz]   the channel and northern buoyancy sections (SectionBatch).
  Each is one of
    - a host array with a leading member axis ([n][len], sections [n][rows][nz]) or without one
      (shared by every member);
    - a DeviceArray holding the rows in place, member m's row starting m * len doubles into it;
    - a tuple (DeviceArray, offset, stride) in doubles: member m's row starts offset + m * stride.
  lbasin_km, lnorth_km, n_basin, n_north   the script's 12000., 1000., 60 and 10.
  store     which of 'z', 'b', 'res' (psi_z, psi_b, psi_res) and 'bnew' (the assembled buoyancy
            section, attribute `b`) go to device memory, each [n][nrows][nz]; the extrema and the
            status are always computed.

  compute() is one launch; psi_z / psi_b / psi_res / b are the device arrays (None when not
  stored), ynew the row coordinate in km, extrema() and status() the per-member numbers.
  The two-basin script's fields (twobasin_NadeauJansen.py:207-262) are out of scope here:
  TwoBasinOverturningSections builds them.
  """

  def __init__(self, y, z, nb, n=None, b_basin=None, bs_SO=None, Psi=None, Psi_SO=None,
               bgrid=None, psib=None, psibz=None, bsouth=None, bnorth=None, lbasin_km=12000.,
               lnorth_km=1000., n_basin=60, n_north=10, store=("z", "b", "res"), stream=None):
    _lib.require_device()
    self.stream = stream
    self.y_host = np.ascontiguousarray(y, dtype=np.float64)
    self.z_host = np.ascontiguousarray(z, dtype=np.float64)
    if self.y_host.ndim != 1 or self.z_host.ndim != 1:
      raise ValueError("y and z must be 1-D grids")
    ny, nz = self.y_host.size, self.z_host.size
    self.ny, self.nz, self.nb = ny, nz, int(nb)
    self.n_basin, self.n_north = int(n_basin), int(n_north)
    lim = _lib.PM_OVT_MAX_LEVELS
    if not (2 <= ny <= lim and 2 <= nz <= lim):
      raise ValueError("y and z hold 2..%d points (got %d, %d)" % (lim, ny, nz))
    if not 1 <= self.nb <= _lib.PM_OVT_MAX_NB:
      raise ValueError("nb must be 1..%d (got %d)" % (_lib.PM_OVT_MAX_NB, self.nb))
    if self.n_basin < 1 or self.n_north < 1 or self.n_basin + self.n_north > lim:
      raise ValueError("n_basin and n_north must be >= 1 and together <= %d" % lim)
    store = tuple(store)
    for s in store:
      if s not in STORE:
        raise ValueError("store holds 'z', 'b', 'res' and 'bnew', not %r" % (s,))
    self.store = store
    self.rows = section_rows(self.y_host, lbasin_km, lnorth_km, self.n_basin, self.n_north)
    self.ynew = self.rows["ynew"]
    self.nrows = self.ynew.size
    self._keep, counts = [], []
    shapes = (("b_basin", b_basin, (nz,)), ("bs_SO", bs_SO, (ny,)), ("Psi", Psi, (nz,)),
              ("Psi_SO", Psi_SO, (nz,)), ("bgrid", bgrid, (self.nb,)), ("psib", psib, (self.nb,)),
              ("psibz", psibz, (nz,)), ("bsouth", bsouth, (ny, nz)),
              ("bnorth", bnorth, (self.n_north, nz)))
    self.inputs = {name: self._rows(v, name, shape, counts) for name, v, shape in shapes}
    if n is None:
      if not counts:
        raise ValueError("n is needed when no input is a host array with a member axis")
      n = counts[0]
    self.n = int(n)
    for c in counts:
      if c != self.n:
        raise ValueError("inputs hold %d rows, n is %d" % (c, self.n))
    for name, _, shape in shapes:
      dev, off, stride = self.inputs[name]
      last = off + (self.n - 1) * stride + int(np.prod(shape))
      if self.n > 0 and last * dev.dtype.itemsize > dev.nbytes:
        raise ValueError("%s: member rows run past the end of the device array" % name)
    self._c = [DeviceArray.from_host(self.rows[k], stream=stream) for k in ("c1", "c2", "c3")]
    m = max(self.n, 1)
    out = lambda key: DeviceArray((m, self.nrows, nz)) if key in store else None
    self.psi_z, self.psi_b, self.psi_res, self.b = out("z"), out("b"), out("res"), out("bnew")
    self._extrema = DeviceArray((m, 3, 2))
    self._extrema_at = DeviceArray((m, 3, 2), np.int32)
    self._status = DeviceArray((m,), np.int32)
    self._sources = None  # from_ensemble: what compute() launches first

  def _rows(self, v, name, shape, counts):
    """-> (device array, offset, stride) in doubles."""
    length = int(np.prod(shape))
    if v is None:
      raise ValueError("%s is required" % name)
    if isinstance(v, tuple):
      dev, off, stride = v
      if not isinstance(dev, DeviceArray):
        raise TypeError(name, "a tuple input is (DeviceArray, offset, stride)")
      v, off, stride = dev, int(off), int(stride)
      if off < 0 or stride < 0:
        raise ValueError("%s: negative offset or stride" % name)
    elif isinstance(v, DeviceArray):
      off, stride = 0, length
    elif isinstance(v, np.ndarray):
      a = np.ascontiguousarray(v, dtype=np.float64)
      if a.shape == shape:
        stride = 0
      elif a.shape[1:] == shape and a.ndim == len(shape) + 1:
        counts.append(a.shape[0])
        stride = length
      else:
        raise ValueError("%s must have shape %s or [n] + %s, not %s" %
                         (name, list(shape), list(shape), list(a.shape)))
      d = DeviceArray.from_host(a, stream=self.stream)
      self._keep.append(d)
      return (d, 0, stride)
    else:
      raise TypeError(name, "needs to be a numpy array, a DeviceArray or (DeviceArray, offset, stride)")
    if v.dtype != np.float64:
      raise ValueError("%s must hold float64" % name)
    return (v, off, stride)

  @classmethod
  def from_ensemble(cls, ens, cfg, nb=None, L=None, **kw):
    """The sections of a JN2018Ensemble's CURRENT state, everything device-resident: two
    SectionBatch objects with the script's fix-ups read the ensemble's rows in place, and a
    ThermwindBatch and a PsiSOBatch of this object's own solve on those rows into private
    buffers (the script, too, solves afresh: Plot_overturning.py:32-35).  The ensemble's own
    tw / so / wA buffers are never written, so taking sections between two run() calls leaves
    the trajectory as it was.  compute() issues the sections, the solves and the kernel on the
    ensemble's stream, with no host round trip.  `L`: the channel's zonal length for Psi_SO
    (default cfg['L'], the run's own; the script hard-codes its 2e7)."""
    from .psi_so import PsiSOBatch
    from .sections import SectionBatch
    from .thermwind import ThermwindBatch
    n, nz, ny = ens.n, ens.nz, ens.ny
    y, z = np.asarray(cfg["y"], dtype=np.float64), np.asarray(cfg["z"], dtype=np.float64)
    nb = int(cfg["nb"] if nb is None else nb)
    geo = {k: kw[k] for k in ("lbasin_km", "lnorth_km", "n_basin", "n_north") if k in kw}
    rows = section_rows(y, **geo)
    st = ens.stream
    channel = SectionBatch("channel", y, z, bs=ens.ml.bs, bn=ens.cols.b, n=n,
                           fixups="plot_overturning", stream=st)
    north = SectionBatch("twocol", rows["y_north"], z, bs=ens.cols.b, bn=ens.cols.b,
                         bn_offset=n * nz, n=n, fixups="plot_overturning", stream=st)
    tw = ThermwindBatch(z, n, f=cfg["f"], nb=nb, stream=st, z_dev=ens.cols.z)
    so = PsiSOBatch(z, y, n, tau=cfg["tau"], KGM=cfg["KGM"], f=cfg["f"],
                    L=cfg["L"] if L is None else L, stream=st, z_dev=ens.cols.z)
    self = cls(y, z, nb, n=n, b_basin=(ens.cols.b, 0, nz), bs_SO=(ens.ml.bs, 0, ny), Psi=tw.Psi,
               Psi_SO=so.Psi, bgrid=tw.bgrid, psib=tw.psib, psibz=(tw.psibz, 0, nz),
               bsouth=channel.out, bnorth=north.out, stream=st, **kw)
    self.channel, self.north, self.tw, self.so = channel, north, tw, so
    self._sources = ens
    return self

  def descriptor(self):
    d = pm_overturning()
    d.n, d.nz, d.ny, d.nb = self.n, self.nz, self.ny, self.nb
    d.n_basin, d.n_north = self.n_basin, self.n_north
    for field, name in (("b_basin", "b_basin"), ("bs_SO", "bs_SO"), ("Psi", "Psi"),
                        ("Psi_SO", "Psi_SO"), ("bgrid", "bgrid"), ("psib", "psib"),
                        ("psibz1", "psibz"), ("bsouth", "bsouth"), ("bnorth", "bnorth")):
      dev, off, stride = self.inputs[name]
      r = getattr(d, field)
      r.ptr, r.offset, r.stride = dev.ptr, off, stride
    d.c1, d.c2, d.c3 = (c.ptr for c in self._c)
    d.lbasin, d.lnorth = self.rows["lbasin"], self.rows["lnorth"]
    ptr = lambda a: a.ptr if a is not None else None
    d.psi_z, d.psi_b, d.psi_res, d.bnew = ptr(self.psi_z), ptr(self.psi_b), ptr(self.psi_res), ptr(self.b)
    d.extrema, d.extrema_at, d.status = self._extrema.ptr, self._extrema_at.ptr, self._status.ptr
    return d

  def compute(self, stream=None):
    """The fields, extrema and status of all members: one launch (after the sections and the two
    solves, on the same stream, when built with from_ensemble)."""
    if self._sources is not None:
      ens = self._sources
      stream = None  # the private solvers launch on the ensemble's stream, and so does the kernel
      self.channel.grid()
      self.north.grid()
      self.so.update(ens.b_basin, ens.ml.bs)
      self.tw.update(ens.b_basin, ens.b_north, store_psib=True)
    return self.launch(stream)

  def launch(self, stream=None):
    """pm_overturning_sections alone, on the inputs as they are in device memory."""
    s = self.stream if stream is None else stream
    d = self.descriptor()
    check(lib.pm_overturning_sections(C.byref(d), _sh(s)))
    self._last_stream = s
    return self

  def _download(self, arr):
    return arr.download(stream=getattr(self, "_last_stream", self.stream))[:self.n]

  def extrema(self):
    """{'max', 'min': [n][3] float64, 'argmax', 'argmin': [n][3] int32} of the last compute(),
    columns in the order of FIELDS (psi_z, psi_b, psi_res): np.max / np.min over a member's
    section and np.argmax / np.argmin's flat index iy * nz + k (first occurrence; a field with a
    NaN gives NaN and the first NaN's index)."""
    v, at = self._download(self._extrema), self._download(self._extrema_at)
    return {"max": v[:, :, 0].copy(), "min": v[:, :, 1].copy(),
            "argmax": at[:, :, 0].copy(), "argmin": at[:, :, 1].copy()}

  def status(self):
    """[n] int32 of the last compute(): bit 1 the buoyancy section holds a NaN (a point where the
    reference's brenth raises: the script would have stopped), bit 2 b_basin is non-finite or not
    non-decreasing (np.interp's result then depends on its search order)."""
    return self._download(self._status)
