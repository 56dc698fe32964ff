"""The DFA exponent of every sliding window of a recorded index series, on the device: the host
side of pm_series_dfa (csrc/dfa.hip), which `SeriesWindows(..., dfa=...)` uses.

Detrended fluctuation analysis (Livina & Lenton 2007; the third indicator of Lenton et al. 2012,
next to the lag-1 autocorrelation and the variance): inside a window the mean-removed series is
summed into a profile, the profile is cut into boxes of s records, each box's least-squares line is
removed, and the mean square of what is left, F2(s), is followed over a range of scales s; alpha is
half the least-squares slope of ln F2 against ln s -- 0.5 for white noise, 1.5 for a random walk.
It reads the memory of the fluctuations over a range of time scales, not at one lag, so it stays
meaningful where the sampling interval is short against the decorrelation time or where the index
has a spectral peak.  include/pymoc_hip.h states the definition operation by operation.

  default_scales(W)   the scales a window of W records gets with `dfa=True`
  dfa_par(W, dfa)     the checked `DfaPar` (scales, suu, weights) of a class's `dfa` argument
  launch_dfa(...)     the launch alone, over any device view: the sibling of
                      `windows.launch_windows`

Out of scope: backward boxes (the boxes run from the window's start only; the trailing W mod s
records belong to none), DFA orders above 1 (a line per box), overlapping boxes, rescaling alpha to
Lenton's "propagator", DFA of `pos`, anything across ranks or online.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .device import DeviceArray, _sh, launch_span
from .series import as_int

DfaPar = collections.namedtuple("DfaPar", "scales suu weights")


def default_scales(W):
  """The scales of `dfa=True`: for W >= 32 the distinct integers round(4 (W / 16)^(i / 7)),
  i = 0 .. 7 -- at most eight, log-spaced from 4 to W / 4, none above W // 4 -- and (4, W // 4)
  for 20 <= W < 32."""
  W = as_int("window", W)
  if W < 4 * _lib.PM_DFA_SCALE_MIN + 4:
    raise ValueError("dfa needs a window of at least %d records (%d here)"
                     % (4 * _lib.PM_DFA_SCALE_MIN + 4, W))
  if W < 32:
    return (4, W // 4)
  return tuple(sorted({min(int(round(4.0 * (W / 16.0) ** (i / 7.0))), W // 4) for i in range(8)}))


def suu_of(s):
  """sum u_i^2 = s (s^2 - 1) / 12 of u_i = i - (s - 1) / 2: exact, the value the entry checks."""
  s = int(s)
  return float(s * (s * s - 1)) / 12.0


def weights_of(scales):
  """w_q = 0.5 (L_q - Lbar) / sum (L_q - Lbar)^2, L_q = ln s_q: alpha = sum w_q ln F2_q is the
  least-squares slope of ln F against ln s."""
  L = np.log(np.asarray(scales, dtype=np.float64))
  dev = L - L.mean()
  return 0.5 * dev / (dev * dev).sum()


def dfa_par(W, dfa):
  """The `DfaPar` of a window of W records: `dfa` True (default_scales) or a sequence of scales,
  checked as the entry checks them."""
  if dfa is True:
    scales = default_scales(W)
  else:
    if isinstance(dfa, (str, bytes, bool)) or not hasattr(dfa, "__iter__"):
      raise ValueError("dfa must be True or a sequence of scales (%r here)" % (dfa,))
    scales = tuple(as_int("a dfa scale", s) for s in dfa)
  nq = len(scales)
  if not 2 <= nq <= _lib.PM_DFA_SCALES_MAX:
    raise ValueError("dfa takes 2 to %d scales (%d here)" % (_lib.PM_DFA_SCALES_MAX, nq))
  if scales[0] < _lib.PM_DFA_SCALE_MIN:
    raise ValueError("the smallest dfa scale must be at least %d (%d here)"
                     % (_lib.PM_DFA_SCALE_MIN, scales[0]))
  if any(b <= a for a, b in zip(scales, scales[1:])):
    raise ValueError("the dfa scales must be strictly ascending (%r here)" % (scales,))
  if 4 * scales[-1] > W:
    raise ValueError("the largest dfa scale must leave four boxes: 4 * %d is above window = %d"
                     % (scales[-1], W))
  return DfaPar(scales, tuple(suu_of(s) for s in scales), tuple(weights_of(scales).tolist()))


def launch_dfa(x, k0, k1, par, dfa_par, ctx, alpha=None, f2=None):
  """pm_series_dfa over the records [k0, k1) of the device view `x` with the `WinPar` par (its lag
  is not read) and the `DfaPar` dfa_par: (alpha [nwin, nspec, n], f2) on the device, nothing
  synchronised.  `alpha`: the array of an earlier call (of at least this size), written again.
  `f2`: None -- not stored; True -- [nq, nwin, nspec, n] allocated here; or an earlier call's."""
  d = _lib.pm_series_dfa()
  (d.nrec, d.nspec, d.n), d.k0, d.k1 = x.shape, k0, k1
  d.window, d.step, d.detrend, d.stt, d.v = par.window, par.step, par.detrend, par.stt, x.ptr
  d.nq = len(dfa_par.scales)
  for q in range(d.nq):
    d.scale[q], d.suu[q], d.weight[q] = dfa_par.scales[q], dfa_par.suu[q], dfa_par.weights[q]
  shape = ((k1 - k0 - par.window) // par.step + 1,) + tuple(x.shape[1:])
  if alpha is None:
    alpha = DeviceArray(shape, np.float64)
  if f2 is True:
    f2 = DeviceArray((d.nq,) + shape, np.float64)
  with launch_span(ctx.timer, "k_series_dfa", ctx.stream):
    check(lib.pm_series_dfa(C.byref(d), alpha.ptr, None if f2 is None else f2.ptr,
                            _sh(ctx.stream)))
  return alpha, f2
