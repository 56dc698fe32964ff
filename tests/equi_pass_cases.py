"""The NumPy restatement of `k_column_equi_pass` (K6, pymoc_amd/csrc/equi.hip), an exact
evaluation of the same recurrence, and the launch table of `pm_column_equi_pass`.

`restate` follows the kernel literally -- `equi_elem` per interval, the chunk bounds, sweep 1, the
six `__shfl_up` steps, sweep 2, the last-node writer, the two boundary-condition branches, the
residual of every interval, the insertion count and the `zidx` gather -- with every NumPy product,
quotient and sum an IEEE double operation rounded on its own.  The kernel is built with
`-ffp-contract=off` and its only reassociation is the scan, whose order `restate` repeats, so it
is the authority the device is compared with bit for bit (tests/test_equi_pass_gpu.py).
tests/test_equi_pass_cpu.py pins it to the C oracle (bitwise with one chunk) and to `exact`.

The error bound (asserted for `restate` and for the sequential oracle against `exact`)
---------------------------------------------------------------------------------------
u = 2^-53; every double operation returns its exact result times (1 + d), |d| <= u; first order
in u, made rigorous by the factor 1 / (1 - n C u) (`gamma`).  `exact` starts from the double x
and c, so the first rounding counted is h = x[i+1] - x[i].

A sum whose terms cancel amplifies the errors of its terms.  For the three sums of `equi_elem`
  N = 1 + h c[i]/6 + k4 al,   D = 1 - h c[i+1]/6 - k4 be,   P = 1 + g + 4 (al + be g)
(al = 1/2 + h c[i]/8, be = 1/2 - h c[i+1]/8, k4 = 4h/6 c_m) let rho >= 1 be the largest of
(sum of |terms|) / |sum| over the intervals of a row, al and be expanded into their own two terms:
  (1 + |h c[i]/6| + |k4| (1/2 + |h c[i]/8|)) / |N|, the same for D, and
  (1 + |g| + 4 ((1/2 + |h c[i]/8|) + (1/2 + |h c[i+1]/8|) |g|)) / |P|.
`exact` returns it from the inputs alone (1 + 1e-6 on the mildest rows of the table, 74 on the
stiffest); the constants below are functions of it and of nothing that was measured.

  N: h = x[i+1] - x[i] 1 rounding; h c[i] 1; /6 1: the term h c[i]/6 carries 3.  al: h c[i]/8 carries
     2 (the division by 8 is exact), al's own sum 1: |d al| <= 3 u (1/2 + |h c[i]/8|).  k4 = (4h)/6 c_m:
     4h exact, h 1, /6 1, the product 1: 3.  k4 al: 3 + 3 + 1 for the product = 7 on
     |k4| (1/2 + |h c[i]/8|).  The first sum 1 + h c[i]/6 adds 1 to both of its terms (1 and 4 in all),
     the last sum 1 on N itself:  |dN| <= (1 + 7 rho) u |N|.
  D: the same count.
  g = N / D: 1 more.                        c_g = 3 + 14 rho            (17 at rho = 1)
  P: g carries c_g, and 1 more from 1 + g; be 3 like al; be g: c_g + 3 + 1; al + be g adds 1 to both
     (al 4, be g c_g + 5); 4 (.) is exact; the last sum 1 on P itself.  The term 4 be g carries the
     most:  |dP| <= ((c_g + 5) rho + 1) u |P|.
  w = (h/6) P: h 1, /6 1, the product 1.    c_w = (c_g + 5) rho + 4     (26 at rho = 1)

One composition step of the affine maps (v, S) -> (G v, S + T v), earlier map (G1, T1) first:
  G = G2 G1 (1 rounding),  T = T1 + T2 G1 (2 roundings).
Claim, for a map composed of n intervals in ANY association: |dG| <= (C_v n - 1) u |G| and
|dT| <= (C_S n - 1) u A, with A = sum_j |w_j prod_{k<j} g_k| over its intervals (|T| <= A).  One
interval: c_g <= C_v - 1 and c_w <= C_S - 1.  Step, with n1 and n2 intervals: dG carries
(C_v n1 - 1) + (C_v n2 - 1) + 1 = C_v (n1 + n2) - 1;  dT <= (C_S n1 - 1) u A1 + ((C_S n2 - 1) +
(C_v n1 - 1) + 1) u A2 |G1| + u (A1 + A2 |G1|) = C_S n1 u A1 + (C_S n2 + C_v n1) u A2 |G1|, which is
<= (C_S (n1 + n2) - 1) u (A1 + A2 |G1|) when C_S >= C_v + 1.  So
  C_v = c_g + 1 = 4 + 14 rho,   C_S = max(c_w, C_v) + 1 = (8 + 14 rho) rho + 5
(18 and 27 at rho = 1), and for node i, reached by a map of i intervals applied to (1, 0):
  |v_i - v^_i| <= C_v i u |v^_i|,   |S_i - S^_i| <= C_S i u A_i,   A_i = sum_{j<i} |w_j v_j|.
Sweep 1, the scan steps and sweep 2 are all such steps (a chunk extended by one interval is a
step with n2 = 1; an empty lane's (1, 0) composes exactly), so the bound holds for the kernel's
chunking, for one chunk (the oracle) and for any other.

After the boundary conditions (n = m - 1, S_n the end value, |S_i| <= A_i):
  bzbot:  V_i = bzbot v_i: one multiply,  (C_v i + 1) u |V^_i|;
          Y_i = bs - bzbot (S_n - S_i): |dY_i| <= u (|bzbot| (C_S n A_n + C_S i A_i + 2 |S^_n - S^_i|)
          + |Y^_i|)  (the inner difference, the multiply, the outer difference).
  bbot:   v0 = (bs - bbot) / S_n: the difference, one division, and S_n's own error
          e_n = C_S n A_n / |S^_n|;  V_i = v0 v_i: one multiply, (C_v i + 3 + e_n) u |V^_i|;
          Y_i = bbot + v0 S_i: |dY_i| <= u (|v0^| (C_S i A_i + (3 + e_n) |S^_i|) + |Y^_i|);
          Y_{m-1} = bs exactly.
"""
import functools

import numpy as np

from pymoc_amd.equilibrium import insert_nodes, point_sets

WAVE = 64
SQRT_3_7 = 0.6546536707079771  # equi.hip
U = 2.0**-53
MUTANTS = ("swap_c23", "be_cn_i", "scan_gt", "w_49_90", "ge_tol")


# ------------------------------------------------------------------ the restatement
def elements(x, cn, cm, mutant=None):
  """`equi_elem` of every interval -> g[m-1], w[m-1]."""
  h = x[1:] - x[:-1]
  c0, c1 = cn[:-1], cn[1:]
  al = 0.5 + h * c0 / 8.0
  be = 0.5 - h * (c0 if mutant == "be_cn_i" else c1) / 8.0
  k4 = 4.0 * h / 6.0 * cm
  g = (1.0 + h * c0 / 6.0 + k4 * al) / (1.0 - h * c1 / 6.0 - k4 * be)
  w = h / 6.0 * (1.0 + g + 4.0 * (al + be * g))
  return g, w


def chunks(ni, K=None):
  """K and the lanes' chunk bounds i0[64], i1[64] for ni intervals."""
  K = (ni + WAVE - 1) // WAVE if K is None else K
  lane = np.arange(WAVE)
  i0 = np.minimum(lane * K, ni)
  i1 = np.minimum(i0 + K, ni)
  return K, i0, i1


def sweeps(g, w, K=None, mutant=None):
  """Sweep 1, the wave scan, sweep 2 and the last-node writer -> v[m], S[m] for v[0] = 1,
  S[0] = 0.  Nodes no lane writes stay NaN (there are none)."""
  ni = g.size
  K, i0, i1 = chunks(ni, K)
  lane = np.arange(WAVE)
  G, T = np.ones(WAVE), np.zeros(WAVE)
  for k in range(K):
    i = i0 + k
    on = i < i1
    j = np.where(on, i, 0)
    T = np.where(on, T + w[j] * G, T)
    G = np.where(on, g[j] * G, G)
  d = 1
  while d < WAVE:
    Gp, Tp = np.roll(G, d), np.roll(T, d)
    on = lane > d if mutant == "scan_gt" else lane >= d
    T = np.where(on, Tp + T * Gp, T)
    G = np.where(on, G * Gp, G)
    d <<= 1
  v, S = np.roll(G, 1), np.roll(T, 1)
  v[0], S[0] = 1.0, 0.0
  V, Y = np.full(ni + 1, np.nan), np.full(ni + 1, np.nan)
  for k in range(K):
    i = i0 + k
    on = i < i1
    j = i[on]
    V[j], Y[j] = v[on], S[on]
    S = np.where(on, S + w[np.where(on, i, 0)] * v, S)
    v = np.where(on, g[np.where(on, i, 0)] * v, v)
  last = (i1 == ni) & (i0 < i1)
  assert last.sum() == 1
  V[ni], Y[ni] = v[last][0], S[last][0]
  return V, Y


def residuals(x, c4, Y, V, mutant=None):
  """The rms residual of every interval from the nodal values Y, V (equi.hip:144-185)."""
  c0, c1, c2, c3 = c4
  if mutant == "swap_c23":
    c2, c3 = c3, c2
  h = x[1:] - x[:-1]
  xl = x[:-1]
  ya, yb = (Y[:-1], V[:-1]), (Y[1:], V[1:])
  fa, fb = (V[:-1], c0[:-1] * V[:-1]), (V[1:], c0[1:] * V[1:])
  ymid = [0.5 * (yb[k] + ya[k]) - 0.125 * h * (fb[k] - fa[k]) for k in range(2)]
  fmid = (ymid[1], c1 * ymid[1])
  xm = xl + 0.5 * h
  sh = 0.5 * h * SQRT_3_7
  t1, t2 = (xm + sh) - xl, (xm - sh) - xl
  y1, y2, d1, d2 = [None] * 2, [None] * 2, [None] * 2, [None] * 2
  r_mid = 0.
  for k in range(2):
    slope = (yb[k] - ya[k]) / h
    t = (fa[k] + fb[k] - 2 * slope) / h
    q0, q1, q2, q3 = t / h, (slope - fa[k]) / h - t, fa[k], ya[k]
    y1[k] = q3 + q2 * t1 + q1 * (t1 * t1) + q0 * (t1 * t1 * t1)
    y2[k] = q3 + q2 * t2 + q1 * (t2 * t2) + q0 * (t2 * t2 * t2)
    d1[k] = q2 + q1 * t1 * 2.0 + q0 * (t1 * t1) * 3.0
    d2[k] = q2 + q1 * t2 * 2.0 + q0 * (t2 * t2) * 3.0
    col = yb[k] - ya[k] - h / 6 * (fa[k] + fb[k] + 4 * fmid[k])
    rm = 1.5 * col / h / (1 + np.abs(fmid[k]))
    r_mid = r_mid + rm * rm
  f1, f2 = (y1[1], c2 * y1[1]), (y2[1], c3 * y2[1])
  r1 = r2 = 0.
  for k in range(2):
    ra = (d1[k] - f1[k]) / (1 + np.abs(f1[k]))
    rb = (d2[k] - f2[k]) / (1 + np.abs(f2[k]))
    r1 = r1 + ra * ra
    r2 = r2 + rb * rb
  wl = 32.0 / 45.0 if mutant == "w_49_90" else 49.0 / 90.0
  return np.sqrt(0.5 * (32.0 / 45.0 * r_mid + wl * (r1 + r2)))


def classes(rms, tol, mutant=None):
  """`add` of every interval: 0, 1 or 2 new nodes."""
  over = rms >= tol if mutant == "ge_tol" else rms > tol
  return np.where(over & (rms < 100 * tol), 1, np.where(rms >= 100 * tol, 2, 0))


def restate(x, c4, bs, bbot, bzbot, use_bzbot, tol, zidx=None, K=None, mutant=None):
  """One member of one launch -> y[2, m], rms[m-1], nadd, b, bz (the gather at `zidx`, every
  node when it is None).  K: another chunk length than the kernel's (K = m - 1: one chunk, the
  sequential recurrence).  mutant: one of MUTANTS."""
  x = np.ascontiguousarray(x, np.float64)
  c4 = [np.ascontiguousarray(c, np.float64) for c in c4]
  m = x.size
  with np.errstate(all="ignore"):
    g, w = elements(x, c4[0], c4[1], mutant)
    V, Y = sweeps(g, w, K, mutant)
    Send = Y[m - 1]
    if not use_bzbot:
      v0 = (np.float64(bs) - np.float64(bbot)) / Send
      Y = bbot + v0 * Y
      Y[m - 1] = bs
      V = v0 * V
    else:
      Y = bs - bzbot * (Send - Y)
      V = bzbot * V
    rms = residuals(x, c4, Y, V, mutant)
    nadd = int(classes(rms, tol, mutant).sum())
  zidx = np.arange(m) if zidx is None else np.asarray(zidx)
  return np.stack([Y, V]), rms, nadd, Y[zidx], V[zidx]


def coefficients(x, Ak, dAk, wA=None, z=None, wA_z=None):
  """The four coefficient sets c = (w - dAk) / Ak on the point sets of mesh x.  Ak, dAk, wA: four
  arrays each (m, m-1, m-1, m-1 values); with wA = None, w = np.interp of wA_z on the grid z at
  `point_sets(x)`.  -> c4, w4."""
  if wA is None:
    wA = [np.interp(p, z, wA_z) for p in point_sets(x)]
  with np.errstate(all="ignore"):
    return [(np.asarray(wA[s]) - dAk[s]) / Ak[s] for s in range(4)], list(wA)


# ------------------------------------------------------------------ the exact recurrence
def exact(x, c4, bs, bbot, bzbot, use_bzbot):
  """The recurrence evaluated sequentially with mpmath at 60 digits from the double x and c.
  -> dict: v, S (for v[0] = 1, S[0] = 0), A (A_i = sum_{j<i} |w_j v_j|), Y, V (after the
  boundary conditions), rho (the cancellation ratio of the docstring); lists of mpf."""
  import mpmath
  mp = mpmath.mp.clone()
  mp.dps = 60
  f = lambda a: mp.mpf(float(a))
  m = len(x)
  cn, cm = c4[0], c4[1]
  v, S, A, rho = [mp.mpf(1)], [mp.mpf(0)], [mp.mpf(0)], mp.mpf(1)
  for i in range(m - 1):
    h = f(x[i + 1]) - f(x[i])
    a0, a1 = h * f(cn[i]), h * f(cn[i + 1])
    al, be = mp.mpf(1) / 2 + a0 / 8, mp.mpf(1) / 2 - a1 / 8
    k4 = 4 * h / 6 * f(cm[i])
    N, D = 1 + a0 / 6 + k4 * al, 1 - a1 / 6 - k4 * be
    g = N / D
    P = 1 + g + 4 * (al + be * g)
    w = h / 6 * P
    aal, abe = mp.mpf(1) / 2 + abs(a0 / 8), mp.mpf(1) / 2 + abs(a1 / 8)  # al, be with |terms|
    rho = max(rho, (1 + abs(a0 / 6) + abs(k4) * aal) / abs(N), (1 + abs(a1 / 6) + abs(k4) * abe) / abs(D),
              (1 + abs(g) + 4 * (aal + abe * abs(g))) / abs(P))
    A.append(A[i] + abs(w * v[i]))
    S.append(S[i] + w * v[i])
    v.append(g * v[i])
  Sn = S[m - 1]
  if use_bzbot:
    Y = [f(bs) - f(bzbot) * (Sn - s) for s in S]
    V = [f(bzbot) * a for a in v]
  else:
    v0 = (f(bs) - f(bbot)) / Sn
    Y = [f(bbot) + v0 * s for s in S]
    V = [v0 * a for a in v]
  return dict(v=v, S=S, A=A, Y=Y, V=V, rho=rho, mp=mp)


def constants(rho):
  """C_v, C_S of the docstring for a row's cancellation ratio rho."""
  rho = float(rho) * (1 + 1e-15)
  return 4 + 14 * rho, (8 + 14 * rho) * rho + 5


def gamma(n, C):
  """n C u / (1 - n C u)."""
  return n * C * U / (1.0 - n * C * U)


def scaled_bounds(e, bs, bbot, bzbot, use_bzbot):
  """The docstring's bounds after the boundary conditions for every node -> bV[m], bY[m] (float,
  rounded up by 1e-15 relative)."""
  mp = e["mp"]
  f = lambda a: mp.mpf(float(a))
  Cv, CS = constants(e["rho"])
  m = len(e["v"])
  n = m - 1
  S, A, Sn = e["S"], e["A"], e["S"][n]
  bV, bY = np.zeros(m), np.zeros(m)
  for i in range(m):
    if use_bzbot:
      bV[i] = (gamma(i, Cv) + U) * abs(e["V"][i])
      bY[i] = abs(f(bzbot)) * (gamma(n, CS) * A[n] + gamma(i, CS) * A[i] + 2 * U * abs(Sn - S[i])) + \
          U * abs(e["Y"][i])
    else:
      en = gamma(n, CS) * A[n] / abs(Sn)
      v0 = abs((f(bs) - f(bbot)) / Sn)
      bV[i] = (gamma(i, Cv) + 3 * U + en) * abs(e["V"][i])
      bY[i] = 0 if i == n else v0 * (gamma(i, CS) * A[i] + (3 * U + en) * abs(S[i])) + U * abs(e["Y"][i])
  return bV * (1 + 1e-15), bY * (1 + 1e-15)


def scaled_errors(e, y):
  """|V - V^|, |Y - Y^| of y[2, m] against `exact`'s dict -> float arrays."""
  f = lambda a: e["mp"].mpf(float(a))
  m = len(e["v"])
  return (np.array([float(abs(f(y[1][i]) - e["V"][i])) for i in range(m)]),
          np.array([float(abs(f(y[0][i]) - e["Y"][i])) for i in range(m)]))


def bound_ratios(e, y, bs, bbot, bzbot, use_bzbot):
  """The worst error / bound over the nodes of a finite row for the scaled outputs y[2, m]
  against `exact`'s dict e -> (ratio of V, ratio of Y).  The raw (v, S) bound is `raw_ratios`."""
  bV, bY = scaled_bounds(e, bs, bbot, bzbot, use_bzbot)
  dV, dY = scaled_errors(e, y)
  if not use_bzbot:  # the surface value is assigned, not computed
    assert y[0][-1] == bs
    dY[-1] = 0.0
  with np.errstate(all="ignore"):
    rv = np.where(dV == 0, 0.0, dV / bV)
    ry = np.where(dY == 0, 0.0, dY / bY)
  return float(rv.max()), float(ry.max())


def raw_ratios(e, V, Y):
  """The worst |v_i - v^_i| / (C_v i u |v^_i|) and |S_i - S^_i| / (C_S i u A_i) over the nodes
  i >= 1 (node 0 is (1, 0) exactly) for the unscaled nodal values V, Y of `sweeps`."""
  mp = e["mp"]
  f = lambda a: mp.mpf(float(a))
  Cv, CS = constants(e["rho"])
  assert V[0] == 1.0 and Y[0] == 0.0
  rv = rs = 0.0
  for i in range(1, len(e["v"])):
    rv = max(rv, float(abs(f(V[i]) - e["v"][i]) / (gamma(i, Cv) * abs(e["v"][i]))))
    rs = max(rs, float(abs(f(Y[i]) - e["S"][i]) / (gamma(i, CS) * e["A"][i])))
  return rv, rs


# ------------------------------------------------------------------ the table
H0 = 4000.0
SENTINEL = np.uint64(0x7FF4DEADBEEF0001)  # a signalling-looking NaN: no arithmetic returns it


def ak_fn(p):
  """A kappa, linear in depth: np.interp of wA_z between grid levels then leaves c of the size the
  row asks for (a curved A kappa on a 3-level grid would add c h = O(1) of its own)."""
  return 1.6e9 * (1.0 + 0.3 * p / H0)


def dak_fn(p):
  return 1.6e9 * 0.3 / H0 + 0.0 * p


def grid(nz):
  return np.linspace(-H0, 0.0, nz)


def mesh_uniform(m, nz):
  """m nodes, uniform, containing the nz grid levels ((m - 1) a multiple of (nz - 1))."""
  assert (m - 1) % (nz - 1) == 0
  x = np.linspace(-H0, 0.0, m)
  x[::(m - 1) // (nz - 1)] = grid(nz)
  return x


def mesh_random(m, nz, seed):
  rng = np.random.default_rng(seed)
  z = grid(nz)
  x = np.unique(np.concatenate([z, rng.uniform(-H0, 0.0, m - nz)]))
  assert x.size == m
  return x


def mesh_nested(m, nz, seed):
  """solve_bvp-like: the column grid refined by `insert_nodes` again and again, each time in the
  smallest interval still wider than H0 2^-16 (and halving its upper neighbour), so halves and
  thirds nest down to that width before the next interval is taken up."""
  rng = np.random.default_rng(seed)
  x = grid(nz)
  while x.size < m:
    h = np.diff(x)
    k = int(np.argmin(np.where(h > H0 * 2.0**-16, h, np.inf)))
    rms = np.zeros(h.size)
    room = m - x.size
    rms[k] = 1.0 if room >= 2 and rng.random() < 0.7 else 0.05  # 2 nodes (thirds) or 1 (half)
    if room >= 3 and k + 1 < h.size and h[k + 1] > H0 * 2.0**-16:
      rms[k + 1] = 0.05
    x = insert_nodes(x, rms, 1e-3)
  assert x.size == m and np.diff(x).max() >= 2.0**12 * np.diff(x).min()
  return x


class Case(object):
  """One member: mesh x, grid z (levels are mesh nodes), the tables Ak / dAk / wA on the four
  point sets, wA_z on the grid (None: a row the table path alone can express), the boundary
  condition, tol, the row length mmax.  `path`: the forcing path of the row's own launch."""

  def __init__(self, name, x, z, cz, bs=0.03, bbot=-4e-4, bzbot=None, tol=1e-3, mmax=None,
               path="interp", edit=None, finite=True):
    self.name, self.x = name, np.ascontiguousarray(x, np.float64)
    self.z = z = self.x.copy() if z is None else z  # z = None: every node is a grid level
    self.m, self.nz, self.ni = self.x.size, z.size, self.x.size - 1
    self.mmax = self.m if mmax is None else mmax
    self.zidx = np.searchsorted(self.x, z).astype(np.int32)
    assert np.array_equal(self.x[self.zidx], z) and np.all(np.diff(self.x) > 0)
    self.bs, self.bbot, self.tol, self.path, self.finite = bs, bbot, tol, path, finite
    self.use_bzbot, self.bzbot = bzbot is not None, 0.0 if bzbot is None else bzbot
    pts = point_sets(self.x)
    self.Ak = [ak_fn(p) for p in pts]
    self.dAk = [dak_fn(p) for p in pts]
    # wA on the grid such that c(z) = cz(z) there
    self.wA_z = np.asarray(cz(z), np.float64) * ak_fn(z) + dak_fn(z)
    self.wA = None
    if edit is not None:
      edit(self)  # may change wA_z, or set tables self.wA
    if path == "table" and self.wA is None:
      self.wA = [np.interp(p, z, self.wA_z) for p in pts]
    if path == "table":
      self.c4, self.wA = coefficients(self.x, self.Ak, self.dAk, wA=self.wA)
    else:
      self.c4, self.wA = coefficients(self.x, self.Ak, self.dAk, z=z, wA_z=self.wA_z)

  def __repr__(self):
    return self.name

  def restate(self, **kw):
    tol = kw.pop("tol", self.tol)
    zidx = kw.pop("zidx", self.zidx)
    return restate(self.x, self.c4, self.bs, self.bbot, self.bzbot, self.use_bzbot, tol,
                   zidx=zidx, **kw)

  def exact(self):
    return _exact(self.name)


def _osc(s, hmean, waves=3.0):
  """c(z): amplitude s / hmean (so c h ~ s), changing sign so that v stays bounded."""
  return lambda z: s / hmean * (np.cos(waves * np.pi * z / H0) + 0.2)


def _grow(s, hmean):
  """c(z) > 0, growing towards the surface: the bzbot problems that refine."""
  return lambda z: s / hmean * (0.3 + 1.4 * (1 + z / H0))


def _rough_middles(c):
  """Tables no profile gives: c at the interval middles is large on every third interval, so the
  denominator 1 - h c[i+1]/6 - k4 be changes sign there, g < 0 and S cancels."""
  pts = point_sets(c.x)
  h = np.diff(c.x)
  c.wA = [np.interp(p, c.z, c.wA_z) for p in pts]
  big = np.arange(c.ni) % 3 == 1
  c.wA[1] = np.where(big, (4.5 / h) * c.Ak[1] + c.dAk[1], c.wA[1])


def _nan_in_wA_z(c):
  c.wA_z = c.wA_z.copy()
  c.wA_z[c.nz // 2] = np.nan


def _nan_in_table(c):
  c.wA = [np.interp(p, c.z, c.wA_z) for p in point_sets(c.x)]
  c.wA[1][c.ni // 3] = np.nan


def _jumps(c):
  """Tables with c of the Lobatto points off the profile on chosen intervals: residuals of every
  size, so all three classes of `add` appear."""
  pts = point_sets(c.x)
  c.wA = [np.interp(p, c.z, c.wA_z) for p in pts]
  k = np.arange(c.ni)
  amp = np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, 3e-2, 30.0))
  c.wA[2] = c.wA[2] + amp * c.Ak[2] / np.diff(c.x)
  c.wA[3] = c.wA[3] - 0.5 * amp * c.Ak[3] / np.diff(c.x)


def _build():
  T = []
  add = lambda *a, **k: T.append(Case(*a, **k))
  hm = lambda m: H0 / (m - 1)
  # node counts, uniform / random / nested meshes, c h = 1e-6, 1e-2, O(1); both conditions
  add("m2", grid(2), grid(2), _osc(1e-2, hm(2)), mmax=7)
  add("m3", mesh_uniform(3, 3), grid(3), _osc(1e-2, hm(3)), mmax=5, bzbot=2e-5)
  add("m4", mesh_random(4, 3, 1), grid(3), _osc(1e-6, hm(4)), mmax=64)
  add("m64_rand", mesh_random(64, 5, 2), grid(5), _osc(1e-2, hm(64)), mmax=100)
  add("m65_nested", mesh_nested(65, 5, 3), grid(5), _osc(0.5, hm(5)), mmax=128, bzbot=1e-4)
  add("m66_rand", mesh_random(66, 9, 4), grid(9), _osc(1.0, hm(66)), mmax=66 + 5)
  add("m67_full", mesh_random(67, 2, 5), None, _osc(1e-2, hm(67)), bzbot=3e-5)
  add("m128_uni", mesh_uniform(128, 2), grid(2), _osc(1e-6, hm(128)), mmax=192, bzbot=1e-5)
  add("m129_nested", mesh_nested(129, 3, 6), grid(3), _osc(1e-2, hm(3)), mmax=130)
  add("m130_full", mesh_random(130, 2, 7), None, _osc(1.0, hm(130)), bzbot=1e-4)
  add("m1000_rand", mesh_random(1000, 7, 8), grid(7), _osc(1e-2, hm(1000), 5.0), mmax=1024)
  add("m1023_nested", mesh_nested(1023, 9, 9), grid(9), _osc(0.7, hm(9), 9.0), mmax=1024,
      bzbot=1e-4)
  add("m1024_full", mesh_random(1024, 2, 10), None, _osc(1.0, hm(1024), 31.0))
  # the denominator changes sign: g < 0 on a third of the intervals, S cancels
  add("g_negative", mesh_random(97, 4, 11), grid(4), _osc(1e-2, hm(97)), mmax=128, path="table",
      edit=_rough_middles)
  # degenerate members
  add("bs_is_bbot", mesh_random(70, 4, 12), grid(4), _osc(0.5, hm(70)), bs=0.01, bbot=0.01,
      mmax=96)
  add("overflow", mesh_uniform(701, 8), grid(8), _grow(4.0, hm(701)), bzbot=1e-3, mmax=704,
      finite=False)
  add("nan_wA_z", mesh_random(80, 6, 13), grid(6), _osc(1e-2, hm(80)), mmax=96, edit=_nan_in_wA_z,
      finite=False)
  add("nan_table", mesh_random(80, 6, 13), grid(6), _osc(1e-2, hm(80)), mmax=96, path="table",
      edit=_nan_in_table, bzbot=1e-4, finite=False)
  # rows for nadd: the physical bzbot problem that wants more nodes (classes 0, 1, 2 side by
  # side, the last ballot trip partly filled), every class on chosen intervals, all of class 2
  add("refining", mesh_uniform(101, 5), grid(5), _grow(1.3, hm(101)), bzbot=1e-3, mmax=128)
  add("three_classes", mesh_random(150, 5, 14), grid(5), _osc(0.3, hm(150)), bs=40.0, bbot=-30.0,
      mmax=160, path="table", edit=_jumps)
  add("all_class_2", mesh_uniform(71, 8), grid(8), _grow(9.0, hm(71)), bzbot=1.0, mmax=80)
  return T


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FINITE = [c for c in CASES if c.finite]
# the row relaunched with each optional pointer missing, and with the other forcing path
POINTER_ROW = "m65_nested"
# rows whose own rms has an interval in class 1 / an rms[k] that some tol sends to 100 tol exactly
TOL_ROWS = ("refining", "three_classes")
# the mixed batch at mmax = 1024: members of 2 ... 1024 nodes, both conditions, both degenerate
# kinds, the first and the last member inactive
BATCH_MMAX = 1024
BATCH = ("m66_rand", "m2", "m1024_full", "nan_table", "m3", "m1023_nested", "overflow", "m65_nested",
         "g_negative", "nan_wA_z", "m1000_rand", "bs_is_bbot", "refining", "m129_nested", "m4")
BATCH_ACTIVE = (0,) + (1,) * (len(BATCH) - 2) + (0,)
# the driver's four bzbot members that want more nodes than max_nodes = 40 allows
# (the third stops at the first pass, the others at the second: 41, 44, 48 and 57 nodes wanted)
DRIVER = dict(z=np.linspace(-3500., 0., 20), max_nodes=40, bs=0.03, bbot=-4e-4, bzbot=1e-3,
              kappa=2e-5, Area=7e13, amp=(1.4, 2.0, 2.5, 1.6))


def driver_wA():
  z = DRIVER["z"]
  return np.array([a * 8e6 * np.sin(-np.pi * z / 3500.0) for a in DRIVER["amp"]])


@functools.lru_cache(maxsize=None)
def _exact(name):
  c = BY_NAME[name]
  return exact(c.x, c.c4, c.bs, c.bbot, c.bzbot, c.use_bzbot)


@functools.lru_cache(maxsize=None)
def reference(name):
  """`restate` of a row with the kernel's chunking, computed once."""
  return BY_NAME[name].restate()


def tol_boundaries(rms, tol):
  """From a launch's own rms: (k1, tol1) with interval k1 in class 1 and tol1 = rms[k1] (it now
  adds 0), and (k2, tol2) with 100 * tol2 == rms[k2] in double (it adds 2), or None where there
  is none.  tol2 is searched among rms[k] / 100 and its two neighbours over all k."""
  cls = classes(rms, tol)
  one = np.nonzero(cls == 1)[0]
  first = (int(one[0]), float(rms[one[0]])) if one.size else None
  second = None
  for k in range(rms.size):
    if not np.isfinite(rms[k]) or rms[k] <= 0:
      continue
    t = rms[k] / 100
    for cand in (t, np.nextafter(t, 0.0), np.nextafter(t, np.inf)):
      if 100 * cand == rms[k]:
        second = (k, float(cand))
        break
    if second:
      break
  return first, second


def sentinel(shape):
  """float64 array of the sentinel bit pattern."""
  return np.full(shape, SENTINEL, np.uint64).view(np.float64)


def bits(a):
  """uint64 view with every NaN mapped to one pattern: a NaN the arithmetic produced has the
  payload and sign of the machine that produced it (x86 and gfx950 differ for inf - inf), so
  `NaN at the same positions` is all that can be asked; everything else is compared bitwise,
  signed zeros and infinities included."""
  a = np.ascontiguousarray(a, np.float64)
  return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def same(a, b):
  return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def pack(cases, mmax, path, ends_only=False):
  """The host arrays of ONE launch of `cases` as members 0 .. n-1 with rows of mmax.  path
  "interp": wA_z + z (every member on the grid of the first), "table": wA tables.  ends_only: the
  launch's column grid is the two ends of every member's mesh (nz = 2; members of any grids in
  one launch).  Padding of every input row is NaN (zidx, m: none)."""
  n = len(cases)
  nz = 2 if ends_only else cases[0].nz
  assert all(c.m <= mmax and 2 <= nz <= mmax for c in cases)
  h = dict(m=np.array([c.m for c in cases], np.int32), x=np.full((n, mmax), np.nan),
           Ak=np.full((4, n, mmax), np.nan), dAk=np.full((4, n, mmax), np.nan),
           bs=np.array([c.bs for c in cases]), bbot=np.array([c.bbot for c in cases]),
           bzbot=np.array([c.bzbot for c in cases]),
           flags=np.array([2 if c.use_bzbot else 0 for c in cases], np.int32),
           zidx=np.zeros((n, nz), np.int32))
  if path == "table":
    h["wA"] = np.full((4, n, mmax), np.nan)
  else:
    assert not ends_only and all(np.array_equal(c.z, cases[0].z) for c in cases)
    h["z"] = cases[0].z.copy()
    h["wA_z"] = np.stack([c.wA_z for c in cases])
  for i, c in enumerate(cases):
    h["x"][i, :c.m] = c.x
    h["zidx"][i] = [0, c.m - 1] if ends_only else c.zidx
    for s in range(4):
      k = c.m if s == 0 else c.m - 1
      h["Ak"][s, i, :k], h["dAk"][s, i, :k] = c.Ak[s], c.dAk[s]
      if path == "table":
        h["wA"][s, i, :k] = c.wA[s]
  return h, nz
