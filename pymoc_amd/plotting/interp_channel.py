"""Interpolate_channel (src/pymoc/plotting/interp_channel.py): the buoyancy section of the
Southern Ocean channel, interpolated along isopycnals of constant slope (figure post-processing).

Array and float profiles run on the GPU (pymoc_amd/csrc/sections.hip): `gridit()` is one launch,
`__call__` a one-point launch, both bit-identical to the reference.  Arrays are read at call time,
as the reference's closures read them.  CALLABLE profiles can only be evaluated by Python, so with
one of them the reference's algorithm runs on the host with pymoc_amd.utils.brenth (SciPy's
brenth restated), as Psi_SO does for a callable surface buoyancy.  Where brenth fails, both paths
raise the reference's exception (gridit: that of the first failing point)."""
import numpy as np

from ..utils.brenth import brenth
from ._section import _Section


class Interpolate_channel(_Section):
  _kind = "channel"

  def __init__(
      self,
      y=None,    # y-grid
      z=None,    # z-grid
      bs=None,    # surface buoyancy
      bn=None,    # buoyancy profile in the north
  ):
    super(Interpolate_channel, self).__init__(y=y, z=z, bs=bs, bn=bn)

  def _bs_axis(self):
    return self.y

  def _host_call(self, y, z):
    """interp_channel.py:40-62 as written, with the brenth twin."""
    l = self.y[-1]
    if y == l:
      return self.bn(z)

    def f2(x):
      return self.bn(x) - self.bs(0)

    def f(x):
      return self.bn(z - x * (l-y)) - self.bs(y + z/x)

    sbot = -brenth(f2, self.z[0], 0.)/l
    if -z > sbot*y:
      s = sbot
    else:
      s = brenth(f, 1.e-12, 1.0)
    return self.bn(z - s * (l-y))
