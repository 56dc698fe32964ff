"""Pure-Python restatement, in exact rationals, of the host proofs behind the kernels' 3- and
2-instruction quotients (csrc/div_proof.h): the candidate numerators of a denominator and the verdict
of each sequence on them."""
import math
from fractions import Fraction as F


def _fl(x):
  return float(x)  # (int / int true division rounds a Fraction correctly)


def candidates(d, nmax):
  """(dm, A's): d's 53-bit mantissa D as a float, and the numerator mantissas A whose quotient A / D
  lies within nmax / (2 D) ulp of a rounding midpoint without being one (0 < |N| <= nmax)."""
  m, _ = math.frexp(abs(d))
  D = int(m * 2**53)
  v = (D & -D).bit_length() - 1
  Dp = D >> v
  cands = set()
  if v < 3 and Dp > 1:
    for t in (0, 1):
      sh = 53 + t
      for N in range(-nmax, nmax + 1):
        if N == 0 or N % (1 << v):
          continue
        A0 = ((N >> v) * pow((1 << (sh - v)) % Dp, -1, Dp)) % Dp
        lo, hi = (D, 1 << 53) if t == 0 else (1 << 52, D)
        A = A0 + ((lo - A0 + Dp - 1) // Dp) * Dp
        while A < hi:
          q, r = divmod(A * (1 << sh) - N, D)
          if r == 0 and q % 2 == 1:
            cands.add(A)
          A += Dp
  return float(D), cands


def _verdict(dm, cands, quotient):
  ok = True
  for A in cands:
    for a in (float(A), -float(A)):
      if quotient(a) != _fl(F(a) / F(dm)):
        ok = False
  return ok, len(cands)


def div3_reference(d):
  """pm_div3_proven for one denominator: the candidates (within 6 / (2 D) ulp of a midpoint) and
  whether  y = RN(1/d); q0 = RN(a y); r = fma(-d, q0, a); q = fma(r, y, q0)  is the correctly rounded
  quotient on every one of them, both signs."""
  dm, cands = candidates(d, 6)
  y = 1.0 / dm

  def quotient(a):
    q0 = _fl(F(a) * F(y))
    r = _fl(F(-dm) * F(q0) + F(a))
    return _fl(F(r) * F(y) + F(q0))

  return _verdict(dm, cands, quotient)


def div2_reference(d):
  """pm_div2_proven for one denominator: the candidates (within 4 / (2 D) ulp of a midpoint) and
  whether  yh = RN(1/d); yl = RN((1 - d yh) / d); q = RN(a yh + RN(a yl))  is the correctly rounded
  quotient on every one of them, both signs."""
  dm, cands = candidates(d, 4)
  yh = _fl(F(1) / F(dm))
  e = F(1) - F(dm) * F(yh)
  assert _fl(e) == e  # the residual of the reciprocal is exact in one fma
  yl = _fl(e / F(dm))

  def quotient(a):
    return _fl(F(a) * F(yh) + F(_fl(F(a) * F(yl))))

  return _verdict(dm, cands, quotient)
