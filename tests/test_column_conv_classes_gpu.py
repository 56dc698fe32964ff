"""The verification classes of the speculative convective loop (csrc/column.hip.h: conv_class,
conv_spec_run) on constructed columns: the surface-only pattern, whose loop tests the surface
once per block, and the integer filter of the "still nothing convects" test, with every way out
of either -- a second level joining, N2min = 0, a non-finite neighbour, a near-miss level that
raises a false alarm, a first crossing in every part of the wave, a column that convects
everywhere.  Every result is compared bit for bit with the CPU oracle's column_ensemble_steps;
what a construction is meant to do (which levels convect at which step) is asserted on the
oracle's own single steps first, without the device.  (Launches of at least 64 steps run the twin
kernel that has the two mechanisms, k_column_steps_cls: the 70-step launches in its tiers of 16, 4
and 1, the 70 + 70 split entering it again from the state the first launch left.  The 24-step and
33 + 37 launches run k_column_steps, the loops as they were: the same columns, the other kernel.)
Not covered in isolation: the block check's comparison of the surface's bit pattern.  A neighbour
can only turn non-finite inside a speculative block by way of huge finite values, and a huge
positive one convects first, which ends the block through the other test; with a non-finite
level in the initial state the whole wave takes the IEEE form (case d).  (A kernel without that
comparison also passes tests/test_column_cls_churn_gpu.py: DESIGN.md, the mutants of the block check.)"""
import numpy as np
import pytest

import oracle as O

DAY = 86400.
DT = 30 * DAY
BS, BBOT, N2MIN = 0.025, -0.003, 1e-7
AREA_PROVEN = 8e13                 # (the 2-instruction proof accepts it: asserted at nz = 100)
AREA_REJECTED = 138681915977248.73  # (the 2-instruction proof rejects it: the Area leg takes 3)
NZS = (9, 64, 65, 100, 128)         # P = 1, 1, 2, 2, 2 at 64 lanes per column
LAUNCHES = {"70": (70,), "24": (24,), "33+37": (33, 37), "70+70": (70, 70)}
LAUNCH_TWIN = {"70": True, "24": False, "33+37": False, "70+70": True}  # k_column_steps_cls runs it
FORMS = ("form8", "form7", "form6")


def _grid(nz):
  return np.linspace(-4000., 0., nz)


def _kappa(z):
  return 2e-5 + 2e-4 * np.exp(-z / 1000 - 4)


class Col(object):
  """One constructed column: initial state, coefficients, parameters."""

  def __init__(self, kind, z, b0, bs=BS, bbot=BBOT, N2min=N2MIN, kappa=None, w0=1e-8):
    self.kind, self.b0, self.bs, self.bbot, self.N2min = kind, np.array(b0, dtype=float), bs, bbot, N2min
    self.kappa = _kappa(z) if kappa is None else kappa
    self.w0 = w0


def _base(z, bs=BS, bbot=BBOT):
  """config 2's initial profile, strictly below bs in the interior"""
  return (bs - bbot) * np.exp(z / 300.) + bbot


def _trace(z, col, area, nsteps):
  """Levels with b > bs at the convect of each step (the oracle's single steps), as sets."""
  wA = (area * col.w0 * np.sin(np.pi * z / 4000.))[None, :]
  b = col.b0[None, :].copy()
  out = []
  for _ in range(nsteps):
    with np.errstate(invalid="ignore"):
      out.append(frozenset(np.nonzero(b[0] > col.bs)[0].tolist()))
    b = O.column_ensemble_steps(z, col.kappa[None, :], np.full((1, z.size), area), b, wA, DT, [1],
                                [col.bs], [col.bbot], [col.N2min], 1)
  return out


def _joining(z, area, step, bs=BS, bbot=BBOT, alarm=False):
  """(b): surface-only until level nz - 2 crosses bs at the convect of step `step`.  N2min is
  large enough for the surface's adjusted value to stand well above bs, the column downwells, and
  level nz - 2 starts `eps` below bs: bisection on eps for the wanted step.
  alarm (bs > 0): the bottom levels sit flat in bs's 2^-20 bucket, below bs, where they stay for the
  first blocks and do not convect before the joining level does: a false alarm of the integer filter in the first block, so the
  joining level is met in the v_max_f64 loops."""
  nz = z.size
  above = 1e-5 * (z[1] - z[0])  # the surface's adjusted value stands that far above bs

  def make(eps):
    near = bs * (1 - 2.0 ** -22)
    b0 = _base(z, bs, bbot)
    flat = nz // 2 if alarm else 0  # (what disturbs the flat part travels one level per step)
    b0[:flat] = near
    b0[-1] = bs + 0.01
    for k in range(3, min(30, nz - flat)):  # a gentle slope below the surface, then config 2's profile
      b0[-k] = bs - (k - 2) * 0.05 * above
    if nz >= 3:
      b0[-2] = bs - eps
    return Col("join@%d" % step, z, b0, bs=bs, bbot=near if alarm else bbot, N2min=1e-5, w0=-3e-8)

  def first(eps):
    tr = _trace(z, make(eps), area, step + 2)
    for k, s in enumerate(tr):
      if (nz - 2) in s:
        return k
    return len(tr) + 1

  lo, hi = 0.0, 50 * above  # first(lo) is early, first(hi) late
  for _ in range(60):
    mid = 0.5 * (lo + hi)
    if first(mid) <= step:
      lo = mid
    else:
      hi = mid
  col = make(lo)
  return col, first(lo)


def _crossing(z, level):
  """(g): nothing convects at step 0; level `level` alone overshoots bs in the first step (a
  local diffusivity beyond the explicit scheme's bound, under a flat profile), so the first
  speculative block sees the first crossing there."""
  flat, low = 0.9 * BS, 0.5 * BS
  b0 = np.full(z.size, flat)
  b0[-1] = BS
  b0[level] = low
  kappa = _kappa(z).copy()
  dz = z[1] - z[0]
  kappa[level] = 0.75 * dz * dz / DT
  return Col("cross@%d" % level, z, b0, bbot=flat, kappa=kappa, w0=0.0)


def _columns(nz, group, area):
  z = _grid(nz)
  P = 1 if nz <= 64 else 2
  cols = []
  if group == "A":
    b0 = _base(z)
    b0[-1] = BS + 0.01
    cols.append(Col("surface", z, b0))                                   # (a)
    for step in (17, 24, 32):                                            # (b) first / middle / last of block 2
      col, got = _joining(z, area, step)
      assert got == step or nz == 9, (nz, step, got)  # (nz = 9: the coarse grid may not allow it)
      cols.append(col)
    cols.append(Col("N2min=0", z, b0, N2min=0.0))                         # (c)
    for bad in (np.inf, np.nan):                                         # (d)
      bb = b0.copy()
      bb[-2] = bad
      cols.append(Col("neighbour %r" % bad, z, bb))
    hot = BS + 0.01 + 1e-3 * np.linspace(0., 1., nz)                      # (h)
    cols.append(Col("all", z, hot))
  elif group == "C":
    # (b) again where the integer filter is not in use: bs < 0, bs = 0 (never valid), and bs > 0
    # after a forced false alarm -- the surface-only class in the v_max_f64 loops, where level
    # nz - 2 shares the surface's lane at P = 2 and even nz
    for kw in (dict(bs=-0.001), dict(bs=0.0), dict(alarm=True)):
      for step in (17, 24, 32):
        col, got = _joining(z, area, step, **kw)
        assert got == step or nz == 9, (nz, step, got, kw)
        cols.append(col)
  else:
    cols.append(Col("quiet bs>0, b both signs", z, _base(z)))            # (e)
    cols.append(Col("quiet bs>0, b>0", z, _base(z, BS, 0.001), bbot=0.001))
    cols.append(Col("quiet bs<0", z, _base(z, -0.001, BBOT), bs=-0.001))
    cols.append(Col("quiet bs=0", z, _base(z, 0.0, BBOT), bs=0.0))
    near = BS * (1 - 2.0 ** -22)                                         # (f): level 0 holds bbot
    b0 = np.full(nz, near)
    b0[-1] = BS
    cols.append(Col("near miss", z, b0, bbot=near, w0=0.0))
    for lane in (0, 31, 32, 49, 63):                                     # (g)
      for slot in range(P):
        lev = lane * P + slot
        if 1 <= lev <= nz - 2:
          cols.append(_crossing(z, lev))
  assert len(cols) <= 16
  return z, cols


_cases = {}


def _case(nz, group, form):
  """Inputs and the oracle's results (70 and 24 steps), computed once and shared."""
  area = AREA_REJECTED if form == "form7" else AREA_PROVEN
  key = (nz, group, area)
  if key not in _cases:
    z, cols = _columns(nz, group, area)
    n = len(cols)
    inp = dict(z=z, cols=cols, kappa=np.stack([c.kappa for c in cols]), area=np.full((n, nz), area),
               b0=np.stack([c.b0 for c in cols]), bs=np.array([c.bs for c in cols]),
               bbot=np.array([c.bbot for c in cols]), N2min=np.array([c.N2min for c in cols]),
               wA=np.stack([area * c.w0 * np.sin(np.pi * z / 4000.) for c in cols]))
    # what the constructions are meant to do, on the oracle's own single steps
    for c in cols:
      tr = _trace(z, c, area, 70)
      if c.kind == "surface":
        assert all(s == frozenset([nz - 1]) for s in tr), (nz, c.kind)
      elif c.kind.startswith("join@") and nz > 9:
        k = int(c.kind[5:])
        assert all(s == frozenset([nz - 1]) for s in tr[:k]) and (nz - 2) in tr[k], (nz, c.kind)
      elif c.kind == "N2min=0":
        assert tr[0] == frozenset([nz - 1]) and tr[1] == frozenset(), (nz, c.kind)
      elif c.kind.startswith("quiet") or c.kind == "near miss":
        assert all(s == frozenset() for s in tr), (nz, c.kind)
      elif c.kind.startswith("cross@"):
        lev = int(c.kind[6:])
        assert tr[0] == frozenset() and tr[1] == frozenset([lev]), (nz, c.kind, sorted(tr[1]))
      elif c.kind == "all":
        assert tr[0] == frozenset(range(nz)), (nz, c.kind)
    ref = {}
    for nsteps in (70, 24, 140):
      ref[nsteps] = O.column_ensemble_steps(z, inp["kappa"], inp["area"], inp["b0"], inp["wA"], DT,
                                            np.ones(n, dtype=np.int32), inp["bs"], inp["bbot"],
                                            inp["N2min"], nsteps)
    inp["ref"] = ref
    _cases[key] = inp
  return _cases[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("group", ["A", "B", "C"])
@pytest.mark.parametrize("nz", NZS)
def test_constructed_columns_vs_oracle(gpu, nz, group, launch, form):
  inp = _case(nz, group, form)
  chunks = LAUNCHES[launch]
  batch = gpu.ColumnBatch(inp["z"], inp["kappa"], inp["area"], inp["b0"], bs=inp["bs"],
                          bbot=inp["bbot"], N2min=inp["N2min"], do_conv=True)
  if form == "form6":
    batch.use_hints(div2=False)
  P = 1 if nz <= 64 else 2
  assert batch.kernel_shape(64) == (64, P)
  if nz == 100:  # the headline's grid: each form really is the one the case names
    assert batch.div3_proven and batch.div2_grid_proven
    assert batch.div2_area_proven.all() == (form != "form7")
    assert not batch.div2_area_proven.any() or form != "form7"
  if batch.div3_proven:
    assert "k_column_steps<64" in batch.kernel_name(chunks[0], lanes_per_col=64)
  for n in chunks:  # which of the two kernels the launch runs (the module's docstring)
    assert batch.kernel_twin(n, lanes_per_col=64) == LAUNCH_TWIN[launch]
    batch.steps(inp["wA"], DT, n, lanes_per_col=64)
  got = batch.get_b()
  ref = inp["ref"][sum(chunks)]
  bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
  rows = np.nonzero(bad.any(axis=1))[0]
  assert rows.size == 0, [(inp["cols"][i].kind, np.nonzero(bad[i])[0][:6].tolist()) for i in rows]
