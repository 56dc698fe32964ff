"""pymoc.plotting (src/pymoc/plotting/__init__.py): the section interpolators of the reference's
figure scripts, with array and float profiles evaluated on the GPU."""
from .interp_channel import Interpolate_channel
from .interp_twocol import Interpolate_twocol
