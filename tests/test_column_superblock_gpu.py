"""The super-block tier of the column twin kernel (csrc/column.hip.h: conv_spec_run, its ROLLED tier --
entries with at least 256 steps to go check their speculative blocks once per 64 steps, the 16-fold
body rolled four times) against the CPU oracle, bit for bit, on the constructed columns of
tests/column_superblock_cases.py: at most 8 columns per batch, nz = 6, 7, 65, 66, 99 and 100 (one and
two levels per lane, odd and even nz: both operand choices of the integer filter), launches of 255,
256, 257, 319, 320 and 339 steps (no super-block; exactly four; a rest that ends in each lower
tier), on both Areas (at nz = 100: form 8 and form 7).  Every launch first asserts on the host that
it runs the twin (ColumnBatch.kernel_twin), and its result is also compared with the same number of
steps taken as 16-step launches, which run k_column_steps.

Members: a column that never convects (bs > 0: the filter loops; bs < 0: the v_max_f64 loops); a
surface-only column; two columns whose level nz - 2 joins the convecting surface at a chosen step of
the second super-block -- its first step, one step in each 16-step quarter, its last step -- in the
filter loops (bs > 0) and in the v_max_f64 loops (bs < 0): the kernel redoes 64 steps and leaves at
step 129; a persistent false alarm of the filter (a column flat in bs's 2^-20 bucket, below bs); a
column scaled by 2^-1000 (the IEEE leg); a column that convects at every level and sheds levels
one at a time: bad blocks after which the loop goes on in the same class, inside super-blocks and
in the 16-step blocks behind them.

What the constructions are meant to do is asserted on the oracle's own single steps, without the
device, in the unmarked tests at the top."""
import numpy as np
import pytest

import column_cls_churn_cases as T
import column_superblock_cases as S

WHERES = sorted(S.JOIN_STEPS, key=S.JOIN_STEPS.get)


# ------------------------------------------------------------------ the oracle alone
@pytest.mark.parametrize("area", S.AREAS, ids=["proven", "rejected"])
@pytest.mark.parametrize("nz", S.NZS)
def test_join_steps_are_the_first_pattern_changes(nz, area):
  """For each joining case the chosen step is the first step at which the pattern changes: the
  surface alone convects before it, level nz - 2 with it from there; and nothing below the
  surface shares bs's high dword before the join (the filter's alarm is the join, not earlier)."""
  for where in WHERES:
    c = S.case(nz, area, where)
    k = c["step"]
    assert S.SECOND <= k < S.SECOND + S.BLOCK
    sets, near = S.convecting(c, k + 1)
    for m in S.JOINING:
      kind = S.MEMBERS[m]
      assert all(sets[j][m] == frozenset([nz - 1]) for j in range(k)), (nz, where, kind)
      assert sets[k][m] == frozenset([nz - 2, nz - 1]), (nz, where, kind, sorted(sets[k][m]))
      if c["bs"][m] > 0:
        assert not near[:k, m].any(), (nz, where, kind)


@pytest.mark.parametrize("nz", S.NZS)
def test_the_other_members_do_what_they_are_named_for(nz):
  c = S.case(nz, S.AREAS[0], "first")
  last = max(S.LAUNCHES)
  sets, near = S.convecting(c, last)
  row = {name: i for i, name in enumerate(S.MEMBERS)}
  for name in ("quiet", "quiet bs<0", "false alarm"):
    assert all(s[row[name]] == frozenset() for s in sets), (nz, name)
  assert all(s[row["surface"]] == frozenset([nz - 1]) for s in sets), nz
  assert all(s[row["ieee"]] == frozenset([nz - 1]) for s in sets), nz
  assert sets[0][row["all"]] == frozenset(range(nz)), nz
  # the false alarm persists: at every step a level shares bs's high dword without convecting
  assert near[:, row["false alarm"]].all(), nz
  assert not near[:, row["quiet"]].any() and not near[:, row["surface"]].any(), nz
  # the scaled column lies outside the exact-division window (2^-200 ... 2^200)
  assert 0 < np.abs(c["b0"][row["ieee"]]).max() < 2.0**-200
  assert all(np.isfinite(c["ref"][n]).all() for n in S.LAUNCHES), nz


@pytest.mark.parametrize("area", S.AREAS, ids=["proven", "rejected"])
@pytest.mark.parametrize("nz", [n for n in S.NZS if n > 64])
def test_the_all_member_keeps_its_class_through_bad_blocks(nz, area):
  """The column that convects at every level sheds levels from the bottom, one at a time, and
  keeps lanes convecting in both slots: each change makes a block bad WITHOUT leaving the loop (the
  redo re-establishes the cache, set_adj() takes the new zconv, the tier goes on).  There are such
  changes inside super-blocks behind the first, and inside the 16-step blocks that follow the
  super-blocks of the 320-step launch (steps 257 ... 304)."""
  row = S.MEMBERS.index("all")
  sets, _ = S.convecting(S.case(nz, area, "first"), 320)
  slots = lambda s: frozenset(l % 2 for l in s)
  kept = [k for k in range(1, 320) if sets[k][row] != sets[k - 1][row] and
          slots(sets[k][row]) == slots(sets[k - 1][row]) == frozenset([0, 1]) and
          sets[k][row] != frozenset([nz - 1])]
  assert any(S.SECOND <= k < 257 for k in kept), (nz, kept)
  assert any(257 <= k < 305 for k in kept), (nz, kept)


def test_launch_lengths_meet_every_tier():
  """Behind step 0: no super-block below 256 steps, then as many as fit, the rest in blocks of 16
  (at most three), 4 and 1."""
  shape = {}
  for n in S.LAUNCHES:
    togo = n - 1
    sup = togo // 64 if togo >= 256 else 0
    rest = togo - 64 * sup
    shape[n] = (sup, rest // 16, rest % 16 // 4, rest % 4)
  assert shape == {255: (0, 15, 3, 2), 256: (0, 15, 3, 3), 257: (4, 0, 0, 0), 319: (4, 3, 3, 2),
                   320: (4, 3, 3, 3), 339: (5, 1, 0, 2)}


# ------------------------------------------------------------------ the device
def _batch(gpu, c):
  return gpu.ColumnBatch(c["z"], c["kappa"], c["area"], c["b0"], bs=c["bs"], bbot=c["bbot"],
                         N2min=c["N2min"], do_conv=True)


def _same(a, b):
  return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.gpu
@pytest.mark.parametrize("where", WHERES)
@pytest.mark.parametrize("nsteps", S.LAUNCHES)
@pytest.mark.parametrize("nz", S.NZS)
def test_superblock_launches_vs_oracle(gpu, nz, nsteps, where):
  P = 1 if nz <= 64 else 2
  for area in S.AREAS:
    c = S.case(nz, area, where)
    one = _batch(gpu, c)
    assert one.kernel_shape(64) == (64, P)
    if nz == 100:  # the headline's grid: the two Areas really are form 8 and form 7
      assert one.div3_proven and one.div2_grid_proven
      assert one.div2_area_proven.all() == (area == T.AREA_PROVEN)
      assert not one.div2_area_proven.any() or area == T.AREA_PROVEN
    assert one.kernel_twin(nsteps, lanes_per_col=64)
    one.steps(c["wA"], S.DT, nsteps, lanes_per_col=64)
    got = one.get_b()
    bad = ~_same(got, c["ref"][nsteps])
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (area, [(S.MEMBERS[i], np.nonzero(bad[i])[0][:6].tolist()) for i in rows])
    # the same steps as 16-step launches (and a shorter last one): k_column_steps
    many = _batch(gpu, c)
    left = nsteps
    while left > 0:
      n = min(16, left)
      assert not many.kernel_twin(n, lanes_per_col=64)
      many.steps(c["wA"], S.DT, n, lanes_per_col=64)
      left -= n
    short = many.get_b()
    rows = np.nonzero((~_same(got, short)).any(axis=1))[0]
    assert rows.size == 0, (area, [S.MEMBERS[i] for i in rows])
