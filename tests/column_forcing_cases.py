"""The forcing modifiers of `pm_column_steps` as a table of whole-batch oracle cases (helper module,
no tests).

With PM_OP_WA_TWOBASIN / PM_OP_WA_PSI the column kernel forms its forcing `wA` itself from
overturning rows (csrc/column.hip.h, k_column_steps).  CASES holds the launches
tests/test_column_forcing_gpu.py makes: the modifier, the launch-plan row the call must select,
lanes per column, levels, members per group and steps per launch.  tests/test_column_forcing_cpu.py
checks the table against the library's shape rule and checks that the inputs can tell a wrong row
or a wrong group boundary from the right one.

Reference (`reference`): the forcing formed in NumPy in the scripts' operation order
(twobasin_NadeauJansen.py:103-105, example_twocol_plusSO.py:105-106), then
`oracle.column_ensemble_steps`.

Inputs (`inputs`): a stratified, slightly noisy `b0` on a stretched and jittered grid, convective
adjustment on the northern rows only (as in the drivers), every row of every overturning array
drawn independently, a few Sv, zero at the top and bottom level.  The overturning arrays have
exactly the rows the drivers allocate: [2n][nz] each for the two-basin modifier; Psi_iso [2n][nz]
and Psi_SO [n][nz] for the two-column one.
"""
import collections
import functools

import numpy as np

from column_plan_cases import _STEPS_ARGS, levels_per_lane

Case = collections.namedtuple("Case", "mod kernel lanes nz n nsteps variant")

MODS = ("twobasin", "twocol", "twocol_noso")  # (twocol_noso: PM_OP_WA_PSI with Psi_SO = NULL)
LANES = (16, 32, 64)
NZS = (2, 3, 17, 64, 65, 100, 129, 257)
MEMBERS = (1, 5, 21, 64)
NSTEPS = (3, 4, 25)  # the minimum, one 4-fold block, a remainder
# default hints / use_hints(div3=False) / an Area that varies in z / arith="contracted"
VARIANTS = ("default", "nodiv3", "areaz", "contracted")


def groups(mod):
  return 3 if mod == "twobasin" else 2


def lanes_used(lanes, nz):
  """pm_column_kernel_shape's rule: at most 8 levels per lane on 16 and 32 lanes -- a column that
  does not fit the lanes asked for takes twice as many (no (lanes, nz) pair of the table is
  refused)."""
  while lanes < 64 and nz > 8 * lanes:
    lanes *= 2
  return lanes


def plan_row(lanes, nz, variant):
  """The launch-plan row (column_plan) of a launch of >= 3 plain timesteps of such a batch."""
  lanes = lanes_used(lanes, nz)
  wave_per_col = lanes == 64 and levels_per_lane(nz, lanes) <= 4
  if not wave_per_col or variant == "areaz":
    return "CK_STEPS_PLAIN"
  return {"default": "CK_STEPS_DIV3_UA", "nodiv3": "CK_STEPS_PLAIN_UA",
          "contracted": "CK_STEPS_CONTRACTED"}[variant]


def kernel_name(c):
  g = lanes_used(c.lanes, c.nz)
  return "k_column_steps<%d,%d,%s>" % (g, levels_per_lane(c.nz, g), _STEPS_ARGS[c.kernel])


def _table():
  t = []
  k = 0

  def add(mod, lanes, nz, n, variant="default", nsteps=None):
    nonlocal k
    if nsteps is None:
      nsteps = NSTEPS[k % 3]
      k += 1
    c = Case(mod, plan_row(lanes, nz, variant), lanes, nz, n, nsteps, variant)
    if c not in t:
      t.append(c)

  for mod in MODS:
    # every (lanes, members) pair at nz = 17 and nz = 100
    for nz in (17, 100) if mod != "twocol_noso" else (17,):
      for lanes in LANES:
        for n in MEMBERS:
          add(mod, lanes, nz, n)
    # every other (lanes, nz) pair
    if mod != "twocol_noso":
      for j, nz in enumerate(z for z in NZS if z not in (17, 100)):
        for i, lanes in enumerate(LANES):
          add(mod, lanes, nz, MEMBERS[(i + j + 1) % 4])
    # the other three instantiations (one wave per column), and Area(z) on 16 and 32 lanes
    for variant in VARIANTS[1:]:
      for j, nz in enumerate((17, 100, 129, 2) if mod != "twocol_noso" else (100,)):
        add(mod, 64, nz, (5, 21, 64, 1)[j], variant)
    add(mod, 16, 17, 5, "areaz")
    add(mod, 32, 100, 21, "areaz")
    add(mod, 64, 257, 5, "contracted")  # (five levels per lane: the plain kernel, exact)
    # the forcing entries at counts n * nz that are no multiple of 256
    add(mod, 64, 3, 1)
    add(mod, 64, 17, 5)
    add(mod, 64, 129, 21)
    # every step count on the headline instantiation
    for nsteps in NSTEPS:
      add(mod, 64, 100, 21, nsteps=nsteps)
  return t


CASES = _table()


def label(c):
  s = "%s-%s-g%d-nz%d-n%d-s%d" % (c.mod, c.kernel, c.lanes, c.nz, c.n, c.nsteps)
  return s if c.variant in ("default", "nodiv3") else s + "-" + c.variant


# ------------------------------------------------------------------ inputs
def grid(nz):
  """A stretched grid (fine at the top) with every interior level moved by up to a fifth of its
  spacing."""
  rng = np.random.default_rng(7000 + nz)
  s = np.linspace(0.0, 1.0, nz)
  z = -4000.0 * (1.0 - s)**1.3
  if nz > 2:
    dz = np.minimum(np.diff(z)[1:], np.diff(z)[:-1])
    z[1:-1] += 0.2 * dz * rng.uniform(-1, 1, nz - 2)
  z[-1] = 0.0
  assert (np.diff(z) > 0).all()
  return z


@functools.lru_cache(maxsize=None)
def inputs(mod, nz, n, areaz=False):
  """Host arrays of a batch of `groups(mod) * n` columns and of its overturning rows."""
  G = groups(mod)
  ncols = G * n
  rng = np.random.default_rng([MODS.index(mod), nz, n])
  z = grid(nz)
  north = np.zeros(ncols, dtype=bool)
  north[n:2 * n] = True
  inp = dict(z=z, n=n, ncols=ncols, do_conv=north, N2min=np.full(ncols, 2e-7))
  amp = rng.uniform(0.5, 2.0, ncols)
  inp["kappa"] = amp[:, None] * (2e-5 + 1e-4 * np.exp(z / 1000.0) + 2e-4 * np.exp(-z / 1000.0 - 4.0))[None, :]
  # Areas: the drivers' magnitudes, one number per column ...
  area = np.concatenate([rng.uniform(6e13, 9e13, n), rng.uniform(5e12, 7e12, n),
                         rng.uniform(1.2e14, 2.2e14, n)])[:ncols]
  area = np.repeat(area[:, None], nz, axis=1)
  if areaz:  # ... or narrowing with depth
    area = area * (1.0 + 0.25 * z / 4000.0)[None, :]
  inp["Area"] = area
  bs = rng.uniform(0.01, 0.03, ncols)
  bbot = rng.uniform(-0.003, -0.0005, ncols)
  scale = rng.uniform(200.0, 400.0, ncols)
  b0 = bs[:, None] * np.exp(z[None, :] / scale[:, None]) + (z / z[0])[None, :] * bbot[:, None]
  # (the drivers' start: the northern columns hold the basin's profile under dense surface water,
  # so they convect from the first step on)
  bs[north] = rng.uniform(2e-4, 1e-3, n)
  b0 += 1e-4 * rng.standard_normal((ncols, nz))
  inp.update(bs=bs, bbot=bbot, b0=b0)

  def rows(m, sv):
    a = sv * rng.standard_normal((m, nz))
    a[:, 0] = a[:, -1] = 0.0
    return a

  inp["iso"] = rows(2 * n, 3.0)
  if mod == "twobasin":
    inp["zon"] = rows(2 * n, 2.0)
    inp["so"] = rows(2 * n, 1.0)
  elif mod == "twocol":
    inp["so"] = rows(n, 1.0)
  # the explicit scheme's limits: diffusion, and the largest vertical velocity the rows can form
  dzmin = np.diff(z).min()
  psimax = sum(np.abs(inp[k]).max() for k in ("iso", "zon", "so") if k in inp) * 1e6
  inp["dt"] = min(0.3 * dzmin**2 / inp["kappa"].max(), 0.4 * dzmin * area.min() / max(psimax, 1.0),
                  30 * 86400.0)
  return inp


def planted(mod, inp):
  """A copy of `inp` whose forcing, once formed, takes members out of the kernels' exact-division
  window (2^-200 <= |x| <= 2^200 or 0): an overturning row at 2^300 (finite after * 1e6), an inf
  level in a Psi_SO row, a NaN level in an iso row, and columns of the last group scaled by
  2^-1000.  Returns (inputs, the edited columns)."""
  n, nz = inp["n"], inp["z"].size
  assert n >= 21 and nz >= 8
  out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
  cols = []
  big = np.full(nz, 2.0**300)
  big[0] = big[-1] = 0.0
  out["iso"][3] = big           # a basin / Atlantic column
  out["iso"][n + 6] = -big      # a northern column
  out["iso"][n + 9, nz // 3] = np.nan
  out["iso"][2, nz - 2] = np.nan
  cols += [3, n + 6, n + 9, 2]
  if mod == "twobasin":
    out["zon"][n + 4] = big     # a Pacific column
    out["so"][12, nz // 2] = np.inf       # Atlantic
    out["so"][n + 13, 1] = -np.inf        # Pacific
    cols += [2 * n + 4, 12, 2 * n + 13]
  elif mod == "twocol":
    out["so"][12, nz // 2] = np.inf
    cols += [12]
  last = groups(mod) - 1  # Pacific columns (northern ones of a two-column batch)
  for m in (last * n + 8, last * n + n - 1):
    s = 2.0**-1000
    out["b0"][m] *= s
    out["bs"][m] *= s
    out["bbot"][m] *= s
    cols.append(m)
  assert len(set(cols)) == len(cols)
  return out, sorted(cols)


# ------------------------------------------------------------------ reference
def form_twobasin(iso, zon, so):
  """wA [3n][nz] of the two-basin driver (twobasin_NadeauJansen.py:103-105)."""
  n = iso.shape[0] // 2
  with np.errstate(all="ignore"):
    return np.concatenate([(iso[:n] + zon[:n] - so[:n]) * 1e6, (-iso[n:]) * 1e6,
                           (-zon[n:] - so[n:]) * 1e6])


def form_twocol(iso, so):
  """wA [2n][nz] of the two-column drivers (example_twocol_plusSO.py:105-106; Psi_SO may be None)."""
  n = iso.shape[0] // 2
  with np.errstate(all="ignore"):
    return np.concatenate([(iso[:n] - so) * 1e6 if so is not None else iso[:n] * 1e6,
                           (-iso[n:]) * 1e6])


def forcing(mod, inp):
  if mod == "twobasin":
    return form_twobasin(inp["iso"], inp["zon"], inp["so"])
  return form_twocol(inp["iso"], inp.get("so"))


def form_by_column(mod, inp, first_north, first_pac=None, pac_row0=None):
  """The same forcing column by column, as a kernel indexes it: columns below `first_north` take
  the basin (Atlantic) expression on their own row, columns below `first_pac` the northern one,
  the others the Pacific one on rows `pac_row0`, ... of the zonal and Psi_SO arrays.  With
  (n, 2n, n) this is `forcing`; anything else is a kernel that is wrong in that way.  Rows past an
  array's end wrap around (a kernel would read out of bounds there)."""
  ncols, nz = inp["ncols"], inp["z"].size
  iso, zon, so = inp["iso"], inp.get("zon"), inp.get("so")
  wA = np.empty((ncols, nz))
  for col in range(ncols):
    if col < first_north:
      if mod == "twobasin":
        wA[col] = (iso[col] + zon[col] - so[col]) * 1e6
      else:
        wA[col] = (iso[col] - so[col % so.shape[0]]) * 1e6 if so is not None else iso[col] * 1e6
    elif first_pac is None or col < first_pac:
      wA[col] = (-iso[col % iso.shape[0]]) * 1e6
    else:
      r = (pac_row0 + col - first_pac) % zon.shape[0]
      wA[col] = (-zon[r] - so[r]) * 1e6
  return wA


def step(inp, wA, nsteps):
  import oracle as O
  with np.errstate(all="ignore"):
    return O.column_ensemble_steps(inp["z"], inp["kappa"], inp["Area"], inp["b0"], wA, inp["dt"],
                                   inp["do_conv"], inp["bs"], inp["bbot"], inp["N2min"], nsteps)


@functools.lru_cache(maxsize=None)
def _reference(mod, nz, n, areaz, nsteps):
  inp = inputs(mod, nz, n, areaz)
  wA = forcing(mod, inp)
  ref = step(inp, wA, nsteps)
  wA.setflags(write=False)
  ref.setflags(write=False)
  return wA, ref


def reference(c):
  """(wA, b after c.nsteps steps) of the case by NumPy and the CPU oracle; shared, read-only."""
  return _reference(c.mod, c.nz, c.n, c.variant == "areaz", c.nsteps)


# ------------------------------------------------------------------ the call
class DeviceCase(object):
  """The inputs on the device: ColumnBatches of them and the overturning rows in arrays of
  exactly the drivers' sizes."""

  def __init__(self, gpu, mod, inp, variant="default"):
    from pymoc_amd import _lib
    self.gpu, self.mod, self.inp, self.variant = gpu, mod, inp, variant
    self.n, self.nz = inp["n"], inp["z"].size
    n, nz = self.n, self.nz
    self.iso = gpu.DeviceArray.from_host(inp["iso"])
    assert self.iso.shape == (2 * n, nz)
    self.zon = self.so = None
    if mod == "twobasin":
      self.zon, self.so = gpu.DeviceArray.from_host(inp["zon"]), gpu.DeviceArray.from_host(inp["so"])
      assert self.zon.shape == self.so.shape == (2 * n, nz)
      self.op = _lib.PM_OP_WA_TWOBASIN
    else:
      if mod == "twocol":
        self.so = gpu.DeviceArray.from_host(inp["so"])
        assert self.so.shape == (n, nz)
      self.op = _lib.PM_OP_WA_PSI
    self.arith = "contracted" if variant == "contracted" else "exact"

  def batch(self):
    inp = self.inp
    b = self.gpu.ColumnBatch(inp["z"], inp["kappa"], inp["Area"], inp["b0"], bs=inp["bs"],
                             bbot=inp["bbot"], N2min=inp["N2min"], do_conv=inp["do_conv"])
    if self.variant == "nodiv3":
      b.use_hints(div3=False)
    b.nonfinite.upload(np.full(b.ncols, 2, dtype=np.int32))  # stale marks: every flag must be written
    return b

  def kernel_name(self, batch, nsteps, lanes):
    return batch.kernel_name(nsteps, lanes, ops=self.op | 7, arith=self.arith)

  def steps_formed(self, batch, nsteps, lanes):
    """The launch under test: the kernel forms the forcing from the overturning rows."""
    kw = dict(lanes_per_col=lanes, arith=self.arith)
    if self.mod == "twobasin":
      batch.steps(None, self.inp["dt"], nsteps, twobasin_forcing=(self.iso, self.zon, self.so), **kw)
    else:
      batch.steps(None, self.inp["dt"], nsteps, psi_forcing=(self.iso, self.so), **kw)

  def forcing_array(self):
    """The forcing as an array by the library's forcing entry (pm_twobasin_forcing /
    pm_twocol_forcing)."""
    from pymoc_amd._lib import check, lib
    n, nz = self.n, self.nz
    wA = self.gpu.DeviceArray((groups(self.mod) * n, nz))
    if self.mod == "twobasin":
      i, z, s = self.iso, self.zon, self.so
      check(lib.pm_twobasin_forcing(n, nz, i.view(0, n).ptr, z.view(0, n).ptr, s.view(0, n).ptr,
                                    i.view(n, n).ptr, z.view(n, n).ptr, s.view(n, n).ptr,
                                    wA.view(0, n).ptr, wA.view(n, n).ptr, wA.view(2 * n, n).ptr, None))
    else:
      check(lib.pm_twocol_forcing(n, nz, self.iso.ptr, self.so.ptr if self.so is not None else None, wA.ptr, None))
    return wA

  def steps_array(self, batch, wA, nsteps, lanes):
    batch.steps(wA, self.inp["dt"], nsteps, lanes_per_col=lanes, arith=self.arith)
