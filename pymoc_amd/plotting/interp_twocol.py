"""Interpolate_twocol (src/pymoc/plotting/interp_twocol.py): the buoyancy section between the
basin and the northern column, interpolated along isopycnals of constant slope (figure
post-processing).

Array and float profiles run on the GPU (pymoc_amd/csrc/sections.hip): `gridit()` is one launch,
`__call__` a one-point launch, both bit-identical to the reference.  Arrays are read at call time,
as the reference's closures read them.  CALLABLE profiles can only be evaluated by Python, so with
one of them the reference's algorithm runs on the host with pymoc_amd.utils.brenth (SciPy's
brenth restated), as Psi_SO does for a callable surface buoyancy.  Where brenth fails, both paths
raise the reference's exception (gridit: that of the first failing point)."""
import numpy as np

from ..utils.brenth import brenth
from ._section import _Section


class Interpolate_twocol(_Section):
  _kind = "twocol"

  def __init__(
      self,
      y=None,    # y-grid
      z=None,    # z-grid
      bs=None,    # buoyancy profile in the south
      bn=None,    # buoyancy profile in the north
  ):
    super(Interpolate_twocol, self).__init__(y=y, z=z, bs=bs, bn=bn)

  def _bs_axis(self):
    return self.z

  def _host_call(self, y, z):
    """interp_twocol.py:37-73 as written, with the brenth twin."""
    l = self.y[-1]
    bsurf = self.make_func(
        self.y / l * self.bn(0) + (1 - self.y / l) * self.bs(0), 'bsurf',
        self.y
    )
    if z == 0 and y == 0:
      z = -0.01
    if z == self.z[0]:
      z = 0.9999 * self.z[0]

    def fint(x):
      return self.bn(0) - self.bs(-x * l)

    def fup(x):
      return self.bs(z - x*y) - bsurf(y - z/x)

    def fdeep(x):
      return self.bs(z - x*y) - self.bn(z + x * (l-y))

    sbot = brenth(fint, 0., 1.)
    if z > -sbot * (l-y):
      s = brenth(fup, 1e-10, 1.0)
    else:
      s = brenth(fdeep, -1.0, 1.0)
    return self.bs(z - s*y)
