"""The inputs of tests/test_column_cls_churn_gpu.py do what that test needs -- asserted on the CPU
oracle's single steps, without a device (tests/column_cls_churn_cases.py: generator, trace).  The
floors below are conditions on the inputs, not measurements: a seed that misses one needs more
columns or another seed, never a lower floor."""
import numpy as np
import pytest

import column_cls_churn_cases as T

BIG = [nz for nz in T.NZS if nz >= 64]
FLOOR_BIG, FLOOR_SMALL = 40, 10  # transitions of each kind over the 140 steps
FLOOR_PART = 5                   # per part of a launch, over the whole table
FLOOR_BUSY = 10                  # columns with >= 3 transitions inside one 70-step window
FLOOR_BUCKET = 5                 # bucket columns alarming in their first block, nothing else going on


def test_table_shapes():
  assert T.NZS == (9, 64, 65, 66, 100, 127, 128) and T.N <= 96
  assert set(T.SPLITS) == {(64,), (65,), (79,), (140,), (70, 70), (64, 64, 12), (100, 40), (63, 63, 14)}
  assert all(n < 64 for n in T.CONTROL) and T.CONTROL in T.SPLITS
  assert all(sum(s) <= T.TOTAL for s in T.SPLITS)


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", T.NZS)
def test_inputs_are_what_the_generator_promises(nz, area):
  c = T.case(nz, area)
  bs, bbot, n = c["bs"], c["bbot"], T.N
  assert np.array_equal(c["z"], np.linspace(-4000., 0., nz)) and (c["area"] == area).all()
  assert 0.6 * n <= (bs > 0).sum() <= 0.9 * n and (bs < 0).sum() >= 3
  assert ((bs == 0) & ~np.signbit(bs)).sum() >= 3 and ((bs == 0) & np.signbit(bs)).sum() == 1
  assert 3 <= (bbot > bs).sum() <= 0.2 * n
  assert 5 <= (c["N2min"] == 0).sum() <= 0.3 * n
  assert 0.5 * n <= (c["b0"][:, -1] > bs).sum() <= 0.85 * n
  bk = c["bucket"]
  assert bk.size >= 16 and (bs[bk] > 0).all() and all(c["kind"][i] == "bucket" for i in bk)
  near = bs[bk] * (1 - 2.0**-22)
  assert np.array_equal(bbot[bk], near) and (c["b0"][bk, :nz // 2] == near[:, None]).all()
  assert (T._hi32(near) == T._hi32(bs[bk])).all() and (near < bs[bk]).all()


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", T.NZS)
def test_every_result_is_finite(nz, area):
  for scale in (0,) + T.SCALES:
    c = T.case(nz, area, scale)
    assert all(np.isfinite(b).all() for b in c["ref"].values()), (nz, area, scale)


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", T.NZS)
def test_transitions_of_every_kind(nz, area):
  tr = T.case(nz, area)["trace"]
  got = {k: T.count(tr["trans"], k) for k in T.KINDS}
  print(nz, area, got)
  floor = FLOOR_BIG if nz >= 64 else FLOOR_SMALL
  assert all(v >= floor for v in got.values()), got


def test_joins_and_first_crossings_in_every_part_of_a_launch():
  """surface-only -> joined and nothing -> interior in the first 16 steps of a launch, in its tier
  of 4 and among its last L % 4 steps, summed over the table."""
  got = {}
  for nz in T.NZS:
    for area in T.AREAS:
      trans = T.case(nz, area)["trace"]["trans"]
      for split in T.SPLITS:
        if split == T.CONTROL:
          continue
        for part, ranges in T.launch_parts(split).items():
          for kind in ("surf->joined", "nothing->interior"):
            got[part, kind] = got.get((part, kind), 0) + sum(T.count(trans, kind, lo, hi) for lo, hi in ranges)
  print(got)
  assert len(got) == 6 and all(v >= FLOOR_PART for v in got.values()), got
  # the lengths of the table leave no part empty
  lengths = [L for s in T.SPLITS if s != T.CONTROL for L in s]
  assert any(L % 4 for L in lengths) and any(L % 16 >= 4 for L in lengths)


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", BIG)
def test_columns_that_change_class_again_and_again(nz, area):
  trans = T.named(T.case(nz, area)["trace"]["trans"])
  busy = 0
  for col in range(T.N):
    steps = [s for (c, s, _, _) in trans if c == col]
    busy += max(sum(1 for s in steps if lo <= s < lo + 70) for lo in (0, 70)) >= 3
  print(nz, area, busy)
  assert busy >= FLOOR_BUSY


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", BIG)
def test_bucket_group_raises_false_alarms(nz, area):
  """A level in bs's 2^-20 bucket, below bs, while nothing convects below the surface: over the
  first block of the time loop (steps 1 ... 16; step 0 establishes the pattern)."""
  c = T.case(nz, area)
  tr, bk = c["trace"], c["bucket"]
  quiet = (tr["cls"][:17, bk] <= T.SURFACE).all(axis=0)
  alarms = tr["alarm"][1:17, bk].any(axis=0)
  print(nz, area, int((quiet & alarms).sum()), int(tr["alarm"].sum()))
  assert (quiet & alarms).sum() >= FLOOR_BUCKET
  # both starting classes are among them
  assert set(tr["cls"][0, bk[quiet & alarms]].tolist()) == {T.NOTHING, T.SURFACE}


@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", T.NZS)
def test_creeping_group_joins_inside_the_bucket(nz, area):
  """The filter's equality case: the column is surface-only and the filter valid (bs > 0, bbot not
  above bs) until level nz - 2 joins with hi32(b) == hi32(bs) -- a true alarm that `>` instead of
  `>=` would miss."""
  c = T.case(nz, area)
  cls, cr = c["trace"]["cls"], c["creep"]
  assert cr.size >= 8 and (c["bs"][cr] > 0).all() and (c["bbot"][cr] <= c["bs"][cr]).all()
  first = [int(np.nonzero(cls[:, i] != T.SURFACE)[0][0]) for i in cr]
  print(nz, area, first)
  assert all(1 <= s <= 60 for s in first) and len(set(first)) >= 3, first
  for i, s in zip(cr, first):
    assert cls[s, i] == T.JOINED
    b = T.steps(c, s)[i]
    assert b[nz - 2] > c["bs"][i] and (b[:nz - 2] <= c["bs"][i]).all()
    assert T._hi32(b[nz - 2:nz - 1])[0] == T._hi32(c["bs"][i:i + 1])[0]


@pytest.mark.parametrize("k", T.SCALES)
@pytest.mark.parametrize("area", T.AREAS)
@pytest.mark.parametrize("nz", T.NZS)
def test_scaled_twins_are_the_same_computation(nz, area, k):
  c, cs = T.case(nz, area), T.case(nz, area, k)
  for t, ref in c["ref"].items():
    want = ref * 2.0**k
    assert np.array_equal(cs["ref"][t].view(np.int64), want.view(np.int64)), (nz, area, k, t)
