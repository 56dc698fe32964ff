"""Constructed members for the first third of `so_member` (K4, pymoc_amd/csrc/psi_so.hip.h): the
outcrop latitudes ys, the 100-point wind average, the slope form of calc_GM and the status word --
and a plain reference of each, NumPy and `fractions.Fraction` only (the C oracle is never called
here; tests/test_psi_so_cases_cpu.py pins the oracle and this module to each other and to SciPy).

A case is one batch on one grid pair: z[nz], y[ny], b[n][nz], bs[n][ny], tau (one scalar per
member, or a profile on y per member) and KGM[n].  Every batch holds every surface-profile style
of `STYLES` once and `rising` a second time, so neighbouring waves run different branches and
n = 13 is no multiple of the four waves of a block.  Where ny is too small for a style, the member
is a `rising` one (`Case.names` says what each member is).

The levels b of a member are sorted uniform values around [min(bs), bs[-1]], overwritten at fixed
positions with the member's `specials`: node values of its own bs (plateau values, the node next to
the minimum, one SOUTH of the minimum, min(bs), bs[-1]), values below min(bs) and above bs[-1], one
NaN and one +inf.  Grids with fewer than 24 levels hold as many specials as half their levels,
taken from a list rotated by the member's index.

The definition the reference gives a level (psi_SO.py:106-140), as `branch_of` names it:
  nan      b is NaN
  south    b < min(bs): y[0] - 1e3
  north    b > bs[-1]: y[-1]
  multi    bs descends somewhere north of its (first) minimum: several crossings, the reference
           returns whichever brentq's iteration ends on
  hit      b equals the value of a node (north of the minimum) that no adjacent node shares
  plateau  b equals a value that adjacent nodes share
  linear   bs[j] < b < bs[j+1] for exactly one j north of the minimum: one linear solve

The bound for `linear` levels (derived, not measured)
-----------------------------------------------------
The kernel returns  y[j] + (b - bs[j]) / ((bs[j+1] - bs[j]) / (y[j+1] - y[j])).  With u = eps / 2
the unit roundoff, the offset term carries the roundings of three differences and two quotients:
(1 + u)^5 - 1 < 3 eps, rounded up to 8 eps to stay clear of second-order terms; the final sum
rounds once more, u |ys| < eps |exact| (1 + ...).  Hence
  |ys - exact| <= 8 eps |offset| + eps |exact|,
`exact` and `offset` from `exact_root` in rational arithmetic on the double inputs.
"""
import functools
from fractions import Fraction

import numpy as np

EPS = float(np.finfo(np.float64).eps)
# (nz, ny): smallest legal; small odd; one staging trip; P = 2 and the second staging trip; the
# third trip; P = 4; P = 8 and the fourth trip
GRIDS = ((2, 2), (5, 3), (64, 64), (65, 65), (100, 130), (200, 51), (512, 200))
STYLES = ("rising", "vee", "min_last_but_one", "min_last", "min_tie", "bump", "late_bump",
          "plateau_in", "plateau_north", "plateau_min", "const", "nan_bs")
MEMBERS = STYLES + ("rising",)
N = len(MEMBERS)
MIN_NY = dict(rising=2, vee=5, min_last_but_one=3, min_last=2, min_tie=3, bump=3, late_bump=67,
              plateau_in=5, plateau_north=4, plateau_min=5, const=2, nan_bs=2)
BRANCHES = ("south", "north", "nan", "hit", "plateau", "linear", "multi")
PAR = dict(f=1e-4, rho=1030., L=5e6, smax=0.01)
OPTIONS = (dict(), dict(Hsill=500., HEk=100., Htapertop=200., Htaperbot=300.))
SENTINEL = np.uint64(0x7FF4DEADBEEF0001)  # a NaN no arithmetic returns


# ------------------------------------------------------------------ the surface profiles
def _rising(rng, ny):
  return np.sort(rng.uniform(0., 0.03, ny)) + 1e-6 * np.arange(ny)


def _vee(r, k):
  """Minimum r[k] at node k, descending south of it, r's own rise north of it."""
  bs = r.copy()
  bs[:k] = 2. * r[k] - r[:k] + 1e-5
  return bs


def surface(style, rng, ny):
  """-> (bs[ny], marks): marks are node values of this profile that its levels must hit."""
  r = _rising(rng, ny)
  if style == "rising":
    return r, []
  if style == "vee":
    k = ny // 3
    bs = _vee(r, k)
    return bs, [bs[k - 1]]
  if style == "min_last_but_one":
    bs = r[::-1].copy()
    bs[-1] = bs[-2] + 0.01
    return bs, []
  if style == "min_last":
    return r[::-1].copy(), []
  if style == "min_tie":
    k = ny // 3 if ny >= 5 else 0
    bs = _vee(r, k)
    bs[k + 2] = bs[k]
    return bs, [bs[k + 1]]
  if style in ("bump", "late_bump"):
    # bump: the descent is found by the first trip of the kernel's monotonicity loop (64 nodes a
    # trip); late_bump: by the second at the earliest
    d = max(2, min((2 * ny) // 3, 41)) if style == "bump" else 65 + (ny - 66) // 2
    bs = r.copy()
    bs[d] = bs[d - 2] + 0.3 * (bs[d - 1] - bs[d - 2])
    return bs, [bs[d], bs[d - 1]]
  if style == "plateau_in":
    k = max(1, ny // 2 - 1)
    bs = r.copy()
    bs[k + 1] = bs[k + 2] = bs[k]
    return bs, [bs[k]]
  if style == "plateau_north":
    bs = r.copy()
    bs[-2] = bs[-1] = bs[-3]
    return bs, [bs[-1]]
  if style == "plateau_min":
    k = ny // 3
    bs = _vee(r, k)
    bs[k + 1] = bs[k + 2] = bs[k]
    return bs, [bs[k]]
  if style == "const":
    return np.full(ny, 0.0123), [0.0123]
  if style == "nan_bs":
    r[(ny - 1) // 2] = np.nan  # never the last node
    return r, []
  raise KeyError(style)


def levels(rng, nz, bs, marks, m):
  """b[nz] of member m and the specials it holds."""
  fin = bs[~np.isnan(bs)]
  lo, hi = fin.min(), bs[-1]
  k = int(np.nanargmin(bs))
  ny = bs.size
  span = max(hi - lo, 0.01)
  b = np.sort(rng.uniform(lo - 0.15 * span, hi + 0.15 * span, nz))
  nodes = [bs[j] for j in sorted({min(k + 1, ny - 1), (k + ny - 1) // 2, max(ny - 2, 0)})
           if not np.isnan(bs[j])]
  rest = nodes + [lo, lo - 1e-3, hi, np.nan, hi + 1e-3, np.inf]
  rest = rest[m % len(rest):] + rest[:m % len(rest)]
  specials = [v for v in list(marks) + rest]
  cnt = len(specials) if nz >= 24 else max(1, nz // 2)
  specials = specials[:cnt]
  pos = np.rint(np.linspace(0, nz - 1, cnt + 2)[1:-1]).astype(int)
  assert np.unique(pos).size == cnt
  b[pos] = specials
  return b, specials


class Case(object):
  def __init__(self, nz, ny):
    rng = np.random.default_rng(1000 * nz + ny)
    self.nz, self.ny, self.n = nz, ny, N
    z = np.sort(rng.uniform(-4000., 0., nz))
    z[-1] = 0.
    y = np.sort(rng.uniform(0., 2e6, ny))
    y[0] = 0.
    self.z, self.y = z, y
    self.names, bs, b = [], [], []
    for m, style in enumerate(MEMBERS):
      name = style if ny >= MIN_NY[style] else "rising"
      row, marks = surface(name, rng, ny)
      lev, _ = levels(rng, nz, row, marks, m)
      self.names.append(name)
      bs.append(row)
      b.append(lev)
    self.bs, self.b = np.array(bs), np.array(b)
    self.tau_scalar = rng.uniform(0.05, 0.2, N)
    # a profile with a sign change inside the grid, so that the 100-point average is not flat
    self.tau_array = (rng.uniform(0.08, 0.2, (N, 1)) * np.cos(1.3 * np.pi * y / y[-1])[None, :] +
                      0.01 * rng.standard_normal((N, ny)))
    self.KGM = rng.uniform(500., 1500., N)
    self.branches = [None if name == "nan_bs" else [branch_of(y, self.bs[m], v) for v in self.b[m]]
                     for m, name in enumerate(self.names)]

  def tau(self, kind):
    return self.tau_scalar if kind == "scalar" else self.tau_array

  def members(self, *names):
    return [m for m, name in enumerate(self.names) if name in names]

  def multi(self):
    """Members whose bs descends somewhere north of its first minimum, by the definition."""
    return [m for m in range(self.n) if self.names[m] != "nan_bs" and not monotone_north(self.bs[m])]


@functools.lru_cache(maxsize=None)
def case(nz, ny):
  return Case(nz, ny)


# ------------------------------------------------------------------ the plain reference
def monotone_north(bs):
  k = int(np.argmin(bs))
  return not np.any(np.diff(bs[k:]) < 0)


def branch_of(y, bs, b):
  """The branch the reference's definition puts level b of a member (no NaN in bs) in."""
  assert not np.isnan(bs).any()
  if np.isnan(b):
    return "nan"
  if b < np.min(bs):
    return "south"
  if b > bs[-1]:
    return "north"
  if not monotone_north(bs):
    return "multi"
  north = bs[int(np.argmin(bs)):]
  hits = int(np.count_nonzero(north == b))
  if hits:  # (north is non-decreasing: equal nodes are adjacent)
    return "plateau" if hits > 1 else "hit"
  return "linear"


def exact_root(y, bs, b):
  """A `linear` level: (root, offset) with root = y_j + offset,
  offset = (b - bs_j) (y_j+1 - y_j) / (bs_j+1 - bs_j), in rational arithmetic."""
  k = int(np.argmin(bs))
  j = k + int(np.nonzero(bs[k + 1:] > b)[0][0])
  assert bs[j] < b < bs[j + 1]
  F = lambda v: Fraction(float(v))
  off = (F(b) - F(bs[j])) * (F(y[j + 1]) - F(y[j])) / (F(bs[j + 1]) - F(bs[j]))
  return F(y[j]) + off, off


def one_solve(y, bs, b):
  """The kernel's formula for a `linear` level in float64 NumPy."""
  k = int(np.argmin(bs))
  j = k + int(np.nonzero(bs[k + 1:] > b)[0][0])
  return y[j] + (b - bs[j]) / ((bs[j + 1] - bs[j]) / (y[j + 1] - y[j]))


def bound_ratio(ys, root, off):
  """|ys - exact| / (8 eps |offset| + eps |exact|)."""
  err = abs(Fraction(float(ys)) - root)
  return float(err / (8 * Fraction(EPS) * abs(off) + Fraction(EPS) * abs(root)))


def _bottom_taper(H, z):
  return 1. if H is None else 1. - np.maximum(z[0] + H - z, 0.)**2. / H**2.


def _top_taper(H, z, scalar):
  if H is not None:
    return 1 - np.maximum(z + H, 0)**2. / H**2.
  if scalar:
    return 1.
  t = np.ones(z.size)
  t[-1] = 0.
  return t


def ekman_raw(ys, z, y, tau, f, rho, L, Hsill=None, HEk=None, **unused):
  """calc_Ekman (psi_SO.py:236-243) at the outcrop latitudes it is handed; m^3/s.  tau: a scalar
  (the reference's closure is then tau + 0 * y) or a profile on y (np.interp)."""
  with np.errstate(all="ignore"):
    return wind_average(ys, y, tau) / f / rho * L * _bottom_taper(Hsill, z) * _top_taper(HEk, z, False)


def wind_average(ys, y, tau):
  """The mean of tau over 100 points from each ys to y[-1] (psi_SO.py:238-239)."""
  tau_ave = np.empty(len(ys))
  with np.errstate(all="ignore"):
    for ii in range(len(ys)):
      pts = np.linspace(ys[ii], y[-1], 100)
      tau_ave[ii] = np.mean(np.interp(pts, y, tau) if np.ndim(tau) else tau + 0 * pts)
  return tau_ave


def gm_raw_noc(ys, z, y, KGM, L, smax, Psi_Ek, Htapertop=None, Htaperbot=None, **unused):
  """calc_GM without the boundary-value smoother (psi_SO.py:302-307, 325-331) at the outcrop
  latitudes it is handed; m^3/s.  Psi_Ek in Sv, as the class holds it."""
  dy_atz = 0 * z
  for ii in range(z.size):
    dy_atz[ii] = max(y[-1] - ys[ii], 0.1)
  with np.errstate(all="ignore"):
    temp = KGM * np.maximum(z / dy_atz, -smax) * L * _top_taper(Htapertop, z, True) * \
        _bottom_taper(Htaperbot, z)
    idx = dy_atz > y[-1] - y[0]
    temp[idx] = np.maximum(temp[idx], -Psi_Ek[idx] * 1e6)
  return temp


def solve_at(ys, c, m, kind, opts):
  """Ek_raw, Psi_Ek, GM_raw, Psi_GM, Psi of member m of case c at the ys handed in."""
  tau = c.tau(kind)[m]
  kw = dict(PAR, **opts)
  ek = ekman_raw(ys, c.z, c.y, tau if kind == "array" else float(tau), **kw)
  gm = gm_raw_noc(ys, c.z, c.y, c.KGM[m], Psi_Ek=ek / 1e6, **kw)
  psi = ek / 1e6 + gm / 1e6
  psi[0] = 0.
  return dict(Ek_raw=ek, Psi_Ek=ek / 1e6, GM_raw=gm, Psi_GM=gm / 1e6, Psi=psi)


# ------------------------------------------------------------------ comparing
def bits(a):
  """uint64 view with every NaN mapped to one pattern (payload and sign of a computed NaN are the
  machine's); everything else compares bitwise, signed zeros and infinities included."""
  a = np.ascontiguousarray(a, np.float64)
  return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def same(a, b):
  return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def sentinel(shape):
  return np.full(shape, SENTINEL, np.uint64).view(np.float64)


def is_sentinel(a):
  return bool(np.all(np.ascontiguousarray(a, np.float64).view(np.uint64) == SENTINEL))
