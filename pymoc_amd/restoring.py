"""The restoring rate of every sliding window of a recorded index series, on the device: the host
side of pm_series_restoring (csrc/restoring.hip), which `SeriesWindows(..., restoring=...)` uses.

Boers 2021 reads the loss of stability of an index from its restoring rate lambda: inside a window
the increments of the detrended index are regressed on the index itself, dx_t = lambda x_t + a +
e_t, with the regression errors e modelled as AR(1) noise and fitted by iterated generalised least
squares (fit lambda, estimate the errors' lag-1 coefficient rho from the residuals, whiten with it,
fit again).  The variance and the lag-1 autocorrelation also rise when the *forcing noise* gets
redder or stronger, with no loss of stability; lambda separates the state's own memory from the
noise's, and lambda rising towards 0 from below is the statement "the state is losing stability".
lambda is per record interval: phi - 1 for an AR(1) state with coefficient phi, -dt / tau for a
relaxation time tau sampled every dt.  include/pymoc_hip.h states the definition operation by
operation.

  restoring_par(W, restoring)   the checked `RestoringPar` (iters) of a class's `restoring` argument
  launch_restoring(...)         the launch alone, over any device view: the sibling of
                                `windows.launch_windows` and `dfa.launch_dfa`

rho is the biased lag-1 estimate of the residuals (as this project's `ac`), not statsmodels'
demeaned, adjusted Yule-Walker estimate, and the iteration count is fixed, with no early exit, so
that a result is a pure function of its window.

Out of scope: AR orders of the errors above 1; online updating; the restoring rate of `pos`;
anything across ranks.  Where the noise is more persistent than the state the two are not
identifiable from one window: the iteration settles on the wrong pair (a prototype at state
coefficient 0.3 and noise coefficient 0.7 settled near lambda -0.32, rho 0.31 against the true
-0.7, 0.7).  That belongs to the method, not to this code.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import as_int

RestoringPar = collections.namedtuple("RestoringPar", "iters")
DEFAULT_ITERS = 10  # the published setting


def restoring_par(W, restoring):
  """The `RestoringPar` of a window of W records: `restoring` True (10 iterations, the published
  setting) or the number of iterations, checked as the entry checks them."""
  W = as_int("window", W)
  if W < _lib.PM_RESTORE_WIN_MIN:
    raise ValueError("restoring needs a window of at least %d records (%d here)"
                     % (_lib.PM_RESTORE_WIN_MIN, W))
  if restoring is True:
    iters = DEFAULT_ITERS
  else:
    if isinstance(restoring, bool):
      raise ValueError("restoring must be True or a number of iterations (%r here)" % (restoring,))
    iters = as_int("restoring", restoring)
  if not 1 <= iters <= _lib.PM_RESTORE_ITERS_MAX:
    raise ValueError("restoring takes 1 to %d iterations (%d here)"
                     % (_lib.PM_RESTORE_ITERS_MAX, iters))
  return RestoringPar(iters)


def launch_restoring(x, k0, k1, par, rpar, ctx, lam=None, rho=None):
  """pm_series_restoring over the records [k0, k1) of the device view `x` with the `WinPar` par
  (its lag is not read) and the `RestoringPar` rpar: (lam [nwin, nspec, n], rho) on the device,
  nothing synchronised.  `lam`: the array of an earlier call (of at least this size), written
  again.  `rho`: None -- not stored; True -- [nwin, nspec, n] allocated here; or an earlier
  call's."""
  d = _lib.pm_series_restoring()
  (d.nrec, d.nspec, d.n), d.k0, d.k1 = x.shape, k0, k1
  d.window, d.step, d.detrend, d.stt, d.v = par.window, par.step, par.detrend, par.stt, x.ptr
  d.iters = rpar.iters
  shape = ((k1 - k0 - par.window) // par.step + 1,) + tuple(x.shape[1:])
  if lam is None:
    lam = DeviceArray(shape, np.float64)
  if rho is True:
    rho = DeviceArray(shape, np.float64)
  with launch_span(ctx.timer, "k_series_restoring", ctx.stream):
    check(lib.pm_series_restoring(C.byref(d), lam.ptr, None if rho is None else rho.ptr,
                                  _sh(ctx.stream)))
  return lam, rho
