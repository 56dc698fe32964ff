"""A case of the fused Jansen & Nadeau loops on the device, driven through the C-ABI descriptor
(pm_jn2018_steps or pm_jn2018_steps_implicit): every array a launch writes sits inside an arena
with guard rows that `outputs` checks.  Shared by test_jn2018_implicit_gpu.py and
test_jn2018_fused_gpu.py; the cases come from jn2018_implicit_cases.make_case."""
import ctypes as C

import numpy as np

SENTINEL = -7.25e300
OUTPUTS = ("b", "bs_SO", "Psi_s", "bbot", "ksel", "nonfinite", "status")


def _shifted(parent, nbytes, shape):
  """`shape` doubles starting `nbytes` into `parent`, as an array that does not own the memory."""
  from pymoc_amd.device import DeviceArray
  v = object.__new__(DeviceArray)
  v.shape, v.dtype = tuple(shape), parent.dtype
  v.nbytes = int(np.prod(shape)) * parent.dtype.itemsize
  assert nbytes + v.nbytes <= parent.nbytes
  v.ptr = parent.ptr + nbytes
  v._parent = parent
  return v


class Members(object):
  """A case on the device.  Every array a launch writes sits inside an arena with one guard
  member (row) before and after it, filled with a sentinel.
  entry: "pm_jn2018_steps" or "pm_jn2018_steps_implicit".
  status=False: the descriptor's ml.status is NULL (and `outputs` has no "status").
  b_off8=True: cols.b -- the descriptor's pointer and every row of an even nz -- lies 8 bytes off
  a 16-byte boundary (the arena starts one double into a larger allocation)."""

  def __init__(self, gpu, case, entry="pm_jn2018_steps_implicit", status=True, b_off8=False):
    from pymoc_amd import _lib
    from pymoc_amd.device import DeviceArray
    self.case, self.n, self.entry = case, case["n"], entry
    n, nz, ny = case["n"], case["nz"], case["ny"]
    two = lambda a: np.concatenate([a, a])  # noqa: E731
    self.cols = gpu.ColumnBatch(case["z"], two(case["kappa"]), case["area"], case["b0"],
                                bs=case["bs"], bbot=case["bbot0"], N2min=case["N2min"],
                                do_conv=True, kappa_alt=two(case["kappaeff"]))
    self.ml = gpu.SOMLBatch(case["y"], nz, case["bs_SO0"], surflux=case["surflux"],
                            rest_mask=case["rest_mask"], b_rest=case["b_rest"], Ks=case["Ks"],
                            h=case["h"], L=case["L"], v_pist=case["v_pist"])
    self.arenas = {}
    self._pad = None

    def arena(name, rows, length, dtype=np.float64, off8=False):
      host = np.full((rows + 2, length), SENTINEL if dtype == np.float64 else -77, dtype=dtype)
      if off8:  # one sentinel double before the arena and one after it
        self._pad = DeviceArray.from_host(np.full(host.size + 2, SENTINEL))
        a = _shifted(self._pad, 8, host.shape)
      else:
        a = DeviceArray.from_host(host)
      self.arenas[name] = (a, host, rows)
      return a.view(1, rows)

    self.cols.b = arena("b", 2 * n, nz, off8=b_off8)
    if b_off8:
      assert nz % 2 == 0 and self.cols.b.ptr % 16 == 8
    self.ml.bs = arena("bs_SO", n, ny)
    self.ml.Psi_s = arena("Psi_s", n, ny)
    # (per-column scalars: the guard "member" is one element)
    self.cols.bbot = arena("bbot", 2 * n, 1)
    self.cols.ksel = arena("ksel", 2 * n, 1, np.int32)
    self.cols.nonfinite = arena("nonfinite", 2 * n, 1, np.int32)
    self.status_given = bool(status)
    if status:
      self.ml.status = arena("status", n, 1, np.int32)
    self.wA = DeviceArray.from_host(case["wA"])
    self.Psi_SO = DeviceArray.from_host(case["Psi_SO"])
    self.Pb = DeviceArray.from_host(case["Psi_res_b"])
    self.Pn = DeviceArray.from_host(case["Psi_res_n"])
    self.b_basin, self.b_north = self.cols.b.view(0, n), self.cols.b.view(n, n)
    self.reset()
    bc = self.bc = _lib.pm_jn2018_bc()
    bc.n, bc.nz, bc.ny, bc.reserved = n, nz, ny, 0
    bc.Psi_SO, bc.Psi_res_b, bc.Psi_res_n = self.Psi_SO.ptr, self.Pb.ptr, self.Pn.ptr
    bc.b_basin, bc.b_north, bc.bs_SO = self.b_basin.ptr, self.b_north.ptr, self.ml.bs.ptr
    bc.bbot, bc.ksel = self.cols.bbot.ptr, self.cols.ksel.ptr

  def reset(self):
    c, n = self.case, self.n
    self.cols.b.upload(c["b0"])
    self.ml.bs.upload(c["bs_SO0"])
    self.ml.Psi_s.upload(c.get("Psi_s0", np.zeros((n, c["ny"]))))
    self.cols.bbot.upload(c["bbot0"].reshape(-1, 1))
    self.cols.ksel.upload(c["ksel0"].reshape(-1, 1))
    self.cols.nonfinite.upload(np.full((2 * n, 1), 5, dtype=np.int32))
    self.ml.status.upload(np.full(self.ml.status.shape, 5, dtype=np.int32))

  def descriptor(self, hints=0):
    from pymoc_amd import _lib
    d = _lib.pm_jn2018()
    d.n, d.hints = self.n, hints
    d.cols = self.cols.descriptor()
    d.wA, d.Psi_SO, d.Psi_res_b, d.Psi_res_n = self.wA.ptr, self.Psi_SO.ptr, self.Pb.ptr, self.Pn.ptr
    ml, t = _lib.pm_so_ml(), self.ml
    ml.n, ml.nz, ml.ny, ml.reserved = t.n, t.nz, t.ny, 0
    ml.y, ml.bs, ml.Psi_s = t.y.ptr, t.bs.ptr, t.Psi_s.ptr
    ml.b_basin, ml.Psi_b = None, None
    ml.surflux, ml.rest_mask, ml.b_rest = t.surflux.ptr, t.rest_mask.ptr, t.b_rest.ptr
    ml.Ks, ml.h, ml.L, ml.v_pist = t.Ks, t.h, t.L, t.v_pist
    ml.status = t.status.ptr if self.status_given else None
    d.ml = ml
    return d

  def fused(self, nsteps, dt=None, hints=0):
    from pymoc_amd._lib import lib
    d = self.descriptor(hints)
    return getattr(lib, self.entry)(C.byref(d), self.case["dt"] if dt is None else dt,
                                    int(nsteps), None)

  def sequence(self, nsteps, scheme):
    """The launches the fused loop replaces, per step: the switch, both columns by `scheme`
    ("explicit" or "implicit"), the mixed layer."""
    from pymoc_amd._lib import check, lib
    for _ in range(nsteps):
      check(lib.pm_jn2018_bc_switch(C.byref(self.bc), None))
      self.cols.steps(self.wA, self.case["dt"], 1, scheme=scheme)
      self.ml.step(self.b_basin, self.Psi_SO, self.case["dt"])

  def outputs(self):
    """name -> the launch's own rows; asserts that the guard rows still hold the sentinel."""
    out = {}
    for name, (a, host, rows) in self.arenas.items():
      got = a.download()
      for g in (0, rows + 1):
        assert got[g].tobytes() == host[g].tobytes(), "guard row of %s overwritten" % name
      out[name] = got[1:rows + 1]
    if self._pad is not None:
      pad = self._pad.download()
      assert pad[0] == SENTINEL and pad[-1] == SENTINEL, "a double next to the arena of b overwritten"
    return out
