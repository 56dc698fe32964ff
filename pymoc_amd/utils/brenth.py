"""scipy.optimize.brenth(f, a, b) with SciPy's defaults (xtol = 2e-12, rtol = 4 eps,
maxiter = 100), restated from scipy/optimize/Zeros/brenth.c (SciPy 1.15.3) decision for
decision, with the Python wrapper's NaN guard (optimize/_zeros_py.py:_wrap_nan_raise).  The
twin of utils/brentq.py: it differs only in the hyperbolic extrapolation step.

Used where the section interpolators must run ON THE HOST: Interpolate_channel /
Interpolate_twocol with a CALLABLE profile, which only Python can evaluate.  Array and float
profiles never come here: the kernel (pymoc_amd/csrc/sections.hip, `brenth`) is the device twin
of this function.  tests/test_sections_cpu.py checks it against SciPy's own brenth."""
import math


def _value(f, x):
  fx = f(x)
  if math.isnan(fx):
    raise ValueError(f'The function value at x={x} is NaN; solver cannot continue.')
  return float(fx)


def brenth(f, xa, xb, xtol=2e-12, rtol=8.881784197001252e-16, maxiter=100):
  xpre, xcur = float(xa), float(xb)
  xblk = fblk = spre = scur = 0.0
  fpre = _value(f, xpre)
  fcur = _value(f, xcur)
  if fpre == 0:
    return xpre
  if fcur == 0:
    return xcur
  if math.copysign(1.0, fpre) == math.copysign(1.0, fcur):
    raise ValueError("f(a) and f(b) must have different signs")
  for _ in range(maxiter):
    if fpre != 0 and fcur != 0 and math.copysign(1.0, fpre) != math.copysign(1.0, fcur):
      xblk, fblk = xpre, fpre
      spre = scur = xcur - xpre
    if abs(fblk) < abs(fcur):
      xpre, xcur, xblk = xcur, xblk, xcur
      fpre, fcur, fblk = fcur, fblk, fcur
    delta = (xtol + rtol * abs(xcur)) / 2
    sbis = (xblk - xcur) / 2
    if fcur == 0 or abs(sbis) < delta:
      return xcur
    if abs(spre) > delta and abs(fcur) < abs(fpre):
      if xpre == xblk:  # interpolate
        stry = -fcur * (xcur - xpre) / (fcur - fpre)
      else:  # extrapolate (hyperbolic)
        dpre = (fpre - fcur) / (xpre - xcur)
        dblk = (fblk - fcur) / (xblk - xcur)
        stry = -fcur * (fblk - fpre) / (fblk * dpre - fpre * dblk)
      if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):
        spre, scur = scur, stry
      else:
        spre = scur = sbis
    else:
      spre = scur = sbis
    xpre, fpre = xcur, fcur
    if abs(scur) > delta:
      xcur += scur
    else:
      xcur += delta if sbis > 0 else -delta
    fcur = _value(f, xcur)
  raise RuntimeError("Failed to converge after %d iterations." % maxiter)
