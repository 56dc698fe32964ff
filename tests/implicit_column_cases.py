"""The implicit (backward Euler) column step: a NumPy restatement, the case table of its tests and
the measured error of the restatement itself.

The scheme has no reference counterpart (the reference's Column.vertadvdiff, column.py:210-249, is
forward Euler), so the tests compare the kernel with this restatement of the scheme as
include/pymoc_hip.h states it: the reference's own discretisation, one tridiagonal system per
column and step, solved here by a sequential Thomas sweep.  `dtype` is a parameter: float64 is the
comparison value, np.longdouble measures how far float64 itself is from the exact solution of the
scheme (`measure_reference_error`), which sets the tolerance of the GPU tests.
"""
import numpy as np

DAY = 86400.0
STEP_COUNTS = (1, 2, 7, 100)

# max over the case table and its step counts of max|b64 - b_longdouble| / max|b|, measured with
# measure_reference_error() on the CPU (x86-64, 80-bit long double).  test_column_implicit_cpu
# re-measures it and requires  fresh <= E_REF <= 2 * fresh.
E_REF = 1.9e-13
# The GPU tolerance, relative to max|b| of the case: cyclic reduction passes a row through up to
# ceil(log2 64) + 2 = 8 elimination levels where the sequential sweep has one.
GPU_TOL_FACTOR = 8.0


def _f(a, dtype):
  return np.asarray(a, dtype=np.float64).astype(dtype)


class Factored(object):
  """Coefficients and Thomas factors of the columns' systems (static over the steps)."""

  def __init__(self, z, kappa, area, weff, dt, use_bzbot, bzbot, dtype):
    nz = z.size
    self.m = m = nz - 2
    self.dz = dz = z[1:] - z[:-1]
    if m <= 0:
      return
    dzm, dzp = dz[:-1], dz[1:]                      # dz[i-1], dz[i] at i = 1 .. nz-2
    dzc = dtype(0.5) * (dzp + dzm)
    with np.errstate(all="ignore"):
      w = weff[:, 1:-1] / area[:, 1:-1]
      neg = w < 0                                   # the reference's own test (column.py:243)
      k = kappa[:, 1:-1]
      cl = np.where(neg, dtype(0), w / dzm) + k / (dzc * dzm)
      cu = np.where(neg, -w / dzp, dtype(0)) + k / (dzc * dzp)
      fold = np.asarray(use_bzbot, dtype=bool)
      a = -(dt * cl)
      c = -(dt * cu)
      cl_eff = cl.copy()
      cl_eff[fold, 0] = 0
      d = dtype(1) + dt * (cl_eff + cu)
      self.q = np.where(fold, -(dt * cl[:, 0]) * (bzbot * dz[0]), dtype(0))
      a[fold, 0] = 0
      self.a, self.c = a, c
      self.l = np.zeros_like(d)
      self.dp = np.empty_like(d)
      self.dp[:, 0] = d[:, 0]
      for j in range(1, m):
        self.l[:, j] = a[:, j] / self.dp[:, j - 1]
        self.dp[:, j] = d[:, j] - self.l[:, j] * c[:, j - 1]
    self.fold = fold

  def solve(self, rhs):
    m = self.m
    with np.errstate(all="ignore"):
      y = np.empty_like(rhs)
      y[:, 0] = rhs[:, 0]
      for j in range(1, m):
        y[:, j] = rhs[:, j] - self.l[:, j] * y[:, j - 1]
      x = np.empty_like(rhs)
      x[:, m - 1] = y[:, m - 1] / self.dp[:, m - 1]
      for j in range(m - 2, -1, -1):
        x[:, j] = (y[:, j] - self.c[:, j] * x[:, j + 1]) / self.dp[:, j]
    return x


def convect(b, z, bs, N2min, do_conv):
  """Column.convect (column.py:251-271) on the columns flagged do_conv, in b's dtype."""
  for j in np.nonzero(do_conv)[0]:
    ind = b[j] > bs[j]
    if ind.any():
      zconv = np.max(z[~ind]) if (~ind).any() else z[0]
      b[j, ind] = bs[j] + N2min[j] * (z[ind] - zconv)
    else:
      b[j, -1] = bs[j]


def restatement(case, nsteps_list, dtype=np.float64, convect_on=True):
  """{nsteps: b [ncols, nz] in `dtype`} after each of the step counts (one run, snapshots)."""
  z = _f(case["z"], dtype)
  ncols, nz = case["b0"].shape
  sel = case["ksel"]
  kap = _f(case["kappa_sets"][sel, np.arange(ncols)], dtype)
  area = _f(case["area"], dtype)
  if case["weff_given"]:
    weff = _f(case["forcing"], dtype)
  else:
    wA = np.zeros((ncols, nz)) if case["forcing"] is None else case["forcing"]
    weff = _f(wA, dtype) - _f(case["dAk_sets"][sel, np.arange(ncols)], dtype)
  dt = dtype(case["dt"])
  bs, bbot, bzbot, N2min = (_f(case[k], dtype) for k in ("bs", "bbot", "bzbot", "N2min"))
  use_bz, do_conv = case["use_bzbot"], case["do_conv"]
  F = Factored(z, kap, area, weff, dt, use_bz, bzbot, dtype)
  b = _f(case["b0"], dtype).copy()
  out, done = {}, 0
  for target in sorted(nsteps_list):
    for _ in range(target - done):
      if convect_on:
        convect(b, z, bs, N2min, do_conv)
      b[~do_conv, -1] = bs[~do_conv]
      b[~use_bz, 0] = bbot[~use_bz]
      if F.m > 0:
        with np.errstate(all="ignore"):
          rhs = b[:, 1:-1].copy()
          rhs[use_bz, 0] = rhs[use_bz, 0] + F.q[use_bz]
          nb = ~use_bz
          rhs[nb, 0] = rhs[nb, 0] - F.a[nb, 0] * b[nb, 0]
          rhs[:, -1] = rhs[:, -1] - F.c[:, -1] * b[:, -1]
        b[:, 1:-1] = F.solve(rhs)
      b[use_bz, 0] = b[use_bz, 1] - bzbot[use_bz] * F.dz[0]
    done = target
    out[target] = b.copy()
  return out


# ---------------------------------------------------------------------------------- cases
def _grid(nz, kind, H=4000.0):
  if kind == "uniform" or nz < 4:
    return np.linspace(-H, 0.0, nz)
  # strongly non-uniform: spacings fall geometrically by 1e3 towards the surface
  dz = 1e3 ** (-np.arange(nz - 1) / float(nz - 2))
  z = np.concatenate([[0.0], np.cumsum(dz)])
  return (z / z[-1] - 1.0) * H


def make_case(name, nz, ncols, grid="uniform", r=1.0, area="const", forcing="sign", mix_bc=False,
              mix_conv=False, nsel=1, const_kappa=False, k_spread=True, rough=1e-3, steps=STEP_COUNTS,
              seed=0):
  """One batch.  r = max(kappa) dt / min(dz)^2 fixes dt.  mix_bc: columns 1, 4, 7, .. use bzbot;
  mix_conv: odd columns are flagged do_conv, with profiles that convect from the top (j % 6 == 1),
  down to the bottom (j % 6 == 3) or not at all (j % 6 == 5)."""
  rng = np.random.RandomState(1000 + seed)
  H = 4000.0
  z = _grid(nz, grid, H)
  j = np.arange(ncols)
  zz = z[None, :]
  k0 = 2e-5 * (1.0 + (0.5 if k_spread else 0.0) * (j % 4))[:, None]
  if const_kappa:
    kap0 = np.broadcast_to(k0, (ncols, nz)).copy()
  else:
    kap0 = k0 * (1.0 + 4.0 * np.exp(zz / 700.0)) + 1e-4 * np.exp(-(zz + H) / 300.0)
  kap1 = 3.0 * k0 * (1.0 + np.exp(-(zz + H) / 900.0))
  kappa_sets = np.stack([kap0, kap1][:nsel])
  ksel = (j % 2 if nsel == 2 else np.zeros(ncols, dtype=np.int64)).astype(np.int32)
  A0 = 1e14 * (1.0 + 0.25 * (j % 3))[:, None]
  if area == "const":
    A = np.broadcast_to(A0, (ncols, nz)).copy()
  else:
    A = A0 * (0.3 + 0.7 * (1.0 + zz / H) ** 2)
  dAk_sets = np.stack([np.gradient(A * k, z, axis=-1) for k in kappa_sets])
  dzmin = np.min(np.diff(z))
  dt = float(r * dzmin ** 2 / kappa_sets.max())
  weff_given = False
  if forcing == "sign":        # changes sign inside the column
    f = 1e-6 * A * np.sin(2.0 * np.pi * (zz / H) * (1 + j[:, None] % 3)) * (0.5 + rng.rand(ncols, 1))
  elif forcing == "zeros":     # weff handed over, exactly +0 / -0 at some levels
    f = 2e-7 * A * np.cos(3.0 * np.pi * zz / H) * (0.5 + rng.rand(ncols, 1))
    f[:, ::3] = 0.0
    f[:, 1::6] = -0.0
    weff_given = True
  elif forcing == "cancel":    # wA == d(A kappa)/dz at some levels: weff = +0 there
    f = 1e-6 * A * np.sin(np.pi * zz / H)
    f[:, ::4] = dAk_sets[ksel, j][:, ::4]
  elif forcing == "none":      # wA = None (0)
    f = None
  else:
    raise ValueError(forcing)
  bs = 0.02 + 0.005 * (j % 5)
  bbot = -0.001 * (j % 3) + 0.0005
  use_bz = (j % 3 == 1) if mix_bc else np.zeros(ncols, dtype=bool)
  bzbot = np.where(use_bz, 2e-7 * (1 + j % 2), 0.0)
  do_conv = (j % 2 == 1) if mix_conv else np.zeros(ncols, dtype=bool)
  N2min = 1e-7 * (1.0 + (j % 2))
  # a smooth stratified profile below bs, plus a little roughness
  b0 = bbot[:, None] + (0.9 * bs - bbot)[:, None] * np.exp(zz / (300.0 + 100.0 * (j[:, None] % 4)))
  b0 = b0 * (1.0 + rough * rng.randn(ncols, nz))
  for c in np.nonzero(do_conv)[0]:
    kind = c % 6
    if kind == 1:    # convects from the top: the upper fifth is denser than the surface value
      top = z > -0.2 * H
      b0[c, top] = bs[c] * (1.0 + 0.05 * (1.0 + z[top] / H))
    elif kind == 3:  # convects down to the bottom
      b0[c] = bs[c] * (1.02 + 0.01 * np.sin(5.0 * zz[0] / H))
  return dict(name=name, z=z, b0=b0, kappa_sets=kappa_sets, ksel=ksel, area=A, dAk_sets=dAk_sets,
              forcing=f, weff_given=weff_given, dt=dt, r=r, bs=bs, bbot=bbot, bzbot=bzbot,
              use_bzbot=use_bz, do_conv=do_conv, N2min=N2min, steps=tuple(steps), nsel=nsel)


# name, nz, ncols, then keywords.  The issue's nz list (2: no interior; 3: one row; <= 64: cyclic
# reduction alone; 65..: the partition; 257: past the register-tuned range; 1024: the largest) and
# both ends of every levels-per-lane instantiation above it (P = 6: 257, 384; 8: 385, 512;
# 12: 513, 768; 16: 769, 1024); ncols not a multiple of the four columns of a block.
CASE_SPECS = [
    ("nz2", 2, 3, dict(r=1.0, mix_bc=True, mix_conv=True, steps=(1, 2, 7))),
    ("nz3", 3, 5, dict(r=2.0, mix_bc=True, mix_conv=True)),
    ("nz4", 4, 1, dict(grid="stretched", r=30.0, steps=(1, 7))),
    ("nz5", 5, 65, dict(r=1e4, mix_bc=True, mix_conv=True, nsel=2, area="varying")),
    ("nz33_r2", 33, 5, dict(r=2.0, const_kappa=True, k_spread=False, forcing="none",
                          steps=(1, 100))),
    ("nz63", 63, 3, dict(grid="stretched", r=1e2, area="varying", steps=(1, 7, 100))),
    ("nz64", 64, 5, dict(r=1e-3)),
    ("nz65", 65, 65, dict(grid="stretched", r=1e4, mix_bc=True, mix_conv=True, nsel=2,
                          steps=(1, 7))),
    ("nz127", 127, 1, dict(r=0.4, forcing="cancel", steps=(1, 100))),
    ("nz128", 128, 3, dict(grid="stretched", r=30.0, forcing="zeros", steps=(1, 2, 7))),
    ("nz129", 129, 5, dict(r=1e4, forcing="none", const_kappa=True, steps=(1, 7, 100))),
    ("nz200", 200, 65, dict(grid="stretched", r=1e2, mix_bc=True, mix_conv=True, nsel=2,
                            area="varying", steps=(1, 7, 100))),
    ("nz200_none", 200, 3, dict(r=0.77, forcing="none", mix_conv=True, steps=(1, 100))),
    ("nz256", 256, 5, dict(r=1e4, area="varying", steps=(1, 7))),
    ("nz257", 257, 3, dict(grid="stretched", r=1e2, mix_bc=True, mix_conv=True, steps=(1, 7))),
    ("nz1024", 1024, 3, dict(grid="stretched", r=1e4, mix_bc=True, mix_conv=True, steps=(1, 7))),
    ("nz1024_u", 1024, 1, dict(r=0.05, steps=(1, 2))),
    # (appended: a case's position seeds its random numbers)
    ("nz384", 384, 1, dict(r=30.0, mix_conv=False, steps=(1, 2))),
    ("nz385", 385, 3, dict(grid="stretched", r=1e2, mix_bc=True, mix_conv=True, steps=(1, 7))),
    ("nz512", 512, 1, dict(r=30.0, area="varying", steps=(1, 2))),
    ("nz513", 513, 5, dict(r=1e4, mix_bc=True, mix_conv=True, nsel=2, steps=(1, 7))),
    ("nz768", 768, 1, dict(grid="stretched", r=1.0, steps=(1, 2))),
    ("nz769", 769, 3, dict(grid="stretched", r=1e2, mix_bc=True, mix_conv=True, steps=(1, 7))),
]
CASE_NAMES = [s[0] for s in CASE_SPECS]
_cases, _refs = {}, {}


def get_case(name):
  if name not in _cases:
    for k, (n, nz, ncols, kw) in enumerate(CASE_SPECS):
      if n == name:
        _cases[name] = make_case(n, nz, ncols, seed=k, **kw)
  return _cases[name]


def reference(name, dtype=np.float64):
  """The restatement's results of a case at its step counts; computed once and shared."""
  key = (name, np.dtype(dtype).name)
  if key not in _refs:
    c = get_case(name)
    _refs[key] = restatement(c, c["steps"], dtype)
  return _refs[key]


# max|restatement - oracle explicit step| at dt over the same at dt / 2 on consistency_case(),
# measured on the CPU (test_column_implicit_cpu re-checks it within [3.8, 4.2])
CONSISTENCY_CPU_RATIO = 3.9257


def consistency_case():
  """A smooth profile at r = 0.02 (no roughness, boundary values that continue the profile): one
  implicit and one explicit step from it differ by O(dt^2)."""
  c = make_case("consistency", 100, 3, r=0.02, rough=0.0, steps=(1,), seed=99)
  zz = c["z"][None, :]
  c["b0"] = c["bbot"][:, None] + (c["bs"] - c["bbot"])[:, None] * np.exp(zz / 400.0)
  c["b0"][:, 0] = c["bbot"]
  return c


def measure_reference_error():
  """{(case, nsteps): max|b64 - b_longdouble| / max|b|} over the case table."""
  out = {}
  for name in CASE_NAMES:
    r64, rld = reference(name, np.float64), reference(name, np.longdouble)
    for k in r64:
      scale = float(np.max(np.abs(rld[k])))
      out[(name, k)] = float(np.max(np.abs(r64[k].astype(np.longdouble) - rld[k]))) / scale
  return out


def maxprinciple_columns(case):
  """Columns the discrete maximum principle covers: they neither convect nor prescribe a bottom
  gradient (bzbot is a flux source; the solution is then no convex combination of the data)."""
  return ~case["do_conv"] & ~case["use_bzbot"]


def maxprinciple_excess(case, b):
  """Largest excursion of b [ncols, nz] outside [min, max](b0, bbot, bs) per covered column,
  in units of nz 2^-52 max|b| (<= 1 passes)."""
  cols = maxprinciple_columns(case)
  if not cols.any():
    return 0.0
  b0 = case["b0"][cols]
  lo = np.minimum(np.minimum(b0.min(axis=1), case["bbot"][cols]), case["bs"][cols])
  hi = np.maximum(np.maximum(b0.max(axis=1), case["bbot"][cols]), case["bs"][cols])
  x = np.asarray(b, dtype=np.float64)[cols]
  scale = b0.shape[1] * 2.0 ** -52 * np.max(np.abs(x), axis=1)
  over = np.maximum(x.max(axis=1) - hi, lo - x.min(axis=1))
  with np.errstate(invalid="ignore", divide="ignore"):
    return float(np.max(np.where(over > 0, over / scale, 0.0)))
