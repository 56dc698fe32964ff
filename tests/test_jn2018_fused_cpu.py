"""Conditions on the row table of the fused Jansen & Nadeau step loop (jn2018_fused_cases.py),
computed from the oracle-side trace: what test_jn2018_fused_gpu.py compares bit for bit reaches
every kernel variant and every out-of-line path of the loop, with no member left out."""
import numpy as np
import pytest

import jn2018_fused_cases as F

FAMILIES = ("fast", "split", "general")
BASIN_OUTCOMES, NORTH_OUTCOMES = {"south", "north", "none"}, {"inflow", "no inflow"}  # the five
NSTEPS = max(F.STEP_COUNTS)


def _rows_of(fam):
  return [n for n in F.ROW_NAMES if F.family(F.row(n)["kernel"]) == fam]


def _ordinary(name):
  """members compared with the oracle: all but the one whose basin is unsorted on purpose"""
  r = F.row(name)
  return [m for m in range(r["n"]) if m != r["unsorted"]]


def test_every_member_is_finite_and_none_is_left_out():
  for name in F.ROW_NAMES:
    ref, trace = F.run(name)
    assert len(trace) == NSTEPS and set(ref) == set(F.STEP_COUNTS)
    for k in F.STEP_COUNTS:
      assert np.isfinite(ref[k]["b"]).all() and np.isfinite(ref[k]["bs_SO"]).all(), (name, k)
      assert not ref[k]["nonfinite"].any() and not (ref[k]["status"] & 2).any(), (name, k)
    assert len(_ordinary(name)) >= F.row(name)["n"] - 1
  assert sum(F.row(n)["unsorted"] is not None for n in F.ROW_NAMES) == 1


def test_the_table_holds_the_shapes_the_dispatch_turns_on():
  rows = [F.row(n) for n in F.ROW_NAMES]

  def nzs(pred):
    return {r["nz"] for r in rows if pred(r)}

  fast = lambda r: r["kernel"].startswith("fast")  # noqa: E731
  assert nzs(lambda r: fast(r) and "P=2" in r["kernel"]) >= {4, 5, 63, 64, 65, 127, 128}
  assert nzs(lambda r: fast(r) and "P=4" in r["kernel"]) >= {129, 130, 200, 255, 256}
  assert nzs(lambda r: r["kernel"].startswith("split")) >= {65, 96, 97, 128, 193, 224}
  assert any(r["nz"] % 2 for r in rows if r["kernel"].startswith("split"))
  assert nzs(lambda r: fast(r) and r["hints"] & F.SPLIT) == {64, 129, 192, 225}
  off = [r for r in rows if r["b_off8"]]
  assert all(r["nz"] % 2 == 0 and "novec" in r["kernel"] for r in off)
  assert {r["kernel"].split()[1] for r in off if fast(r)} == {"P=2", "P=4"}
  gen = [r for r in rows if r["kernel"].startswith("general")]
  assert {r["kernel"] for r in gen} == {"general P=%d" % p for p in (1, 2, 3, 4)}
  assert {r["nz"] for r in gen if r["nz"] < 4 and r["hints"] & F.UA} == {2, 3}
  assert {r["nz"] for r in gen if r["ny"] == 65 and r["zero_psi"] is None} == {64, 65, 129, 200}
  assert any(r["nz"] == 200 and not r["hints"] & F.UA for r in gen)
  assert {r["nz"] for r in gen if not r["status"]} == {64, 200}
  assert {r["ny"] for r in rows} >= {3, 51, 63, 64}
  assert {r["n"] for r in rows} >= {1, 5, 17}
  for p in ("P=2", "P=4"):
    assert any(r["zero_psi"] is not None and fast(r) and p in r["kernel"] for r in rows)
    assert any(r["shared"] and fast(r) and p in r["kernel"] for r in rows)
  h1 = F.row("h1")
  assert h1["n"] == 130 and h1["tiny"] == (0, 63, 64, 129) and h1["n"] > 2 * 64  # 3 blocks of the IEEE leg
  assert {F.row(n)["kernel"] for n in F.ROW_NAMES if F.row(n)["h2"] is not None} == {
      "fast P=2 vec", "fast P=4 vec", "split PS=3 vec"}
  for r in rows:  # forward Euler is stable: r <= 0.3
    c = F.get_case(r["name"])
    dz = np.diff(c["z"]).min()
    assert max(c["kappa"].max(), c["kappaeff"].max()) * c["dt"] / dz ** 2 <= 0.3 * (1 + 1e-12)


@pytest.mark.parametrize("name", F.ROW_NAMES)
def test_kernel_column_is_what_the_dispatch_does(name):
  r = F.row(name)
  assert F.dispatch(r["nz"], r["ny"], r["hints"], not r["b_off8"], r["status"]) == r["kernel"]
  # the hints the GPU test may add leave the row where it is
  for extra in (F.DIV3, F.SHARED, F.DIV3 | F.SHARED):
    assert F.dispatch(r["nz"], r["ny"], r["hints"] | extra, not r["b_off8"], r["status"]) == r["kernel"]
  c = F.get_case(name)
  uniform = bool((c["area"] == c["area"][:, :1]).all())
  assert uniform or not r["hints"] & F.UA  # (the wrong-hint refusal has its own test)
  if r["shared"]:
    n = r["n"]
    for a in (c["kappa"], c["kappaeff"], c["area"][:n], c["area"][n:]):
      assert (a == a[:1]).all()


def test_dispatch_edges():
  d = F.dispatch
  assert d(3, 51, F.UA, True, True) == "general P=1" and d(4, 51, F.UA, True, True) == "fast P=2 vec"
  assert d(128, 64, F.UA, True, True) == "fast P=2 vec" and d(129, 64, F.UA, True, True) == "fast P=4 novec"
  assert d(128, 65, F.UA, True, True) == "general P=2" and d(256, 65, F.UA, True, True) == "general P=4"
  assert d(64, 51, 0, True, True) == d(64, 51, F.UA, True, False) == "general P=1"
  for nz, k in ((64, "fast P=2 vec"), (65, "split PS=3 novec"), (128, "split PS=4 vec"),
                (129, "fast P=4 novec"), (192, "fast P=4 vec"), (193, "split PS=7 novec"),
                (224, "split PS=7 vec"), (225, "fast P=4 novec")):
    assert d(nz, 51, F.UA | F.SPLIT, True, True) == k
  assert d(96, 51, F.UA | F.SPLIT, False, True) == "split PS=3 novec"


@pytest.mark.parametrize("fam", FAMILIES)
def test_family_takes_every_switch_outcome_and_every_rare_path(fam):
  seen = set()
  outcomes = set()
  for name in _rows_of(fam):
    _, trace = F.run(name)
    n = F.row(name)["n"]
    members = _ordinary(name)
    for s, t in enumerate(trace):
      outcomes |= {t["branches"][m] for m in members}
      prev = trace[s - 1] if s else None
      for m in members:
        cb, cn = t["conv"][m], t["conv"][n + m]
        for c in (cb, cn):
          seen.add("no level convects" if not c.any() else "every level convects" if c.all() else "some")
        if t["argmin"][m] != 0:
          seen.add("argmin != 0")
        if t["below"][m].any():
          seen.add("below the first node")
        if t["above"][m].any():
          seen.add("at or above the last node")
        if t["stepped"][m]:
          seen.add("upwelling on" if t["upwell"][m] else "upwelling off")
        if s >= 1:
          kb = t["ksel"][m] != prev["ksel"][m]
          kn = t["ksel"][n + m] != prev["ksel"][n + m]
          if kb:
            seen.add("basin set change after step 1")
          if kn:
            seen.add("northern set change after step 1")
          if kb and kn:
            seen.add("both in one step")
          if (cb != prev["conv"][m]).any() or (cn != prev["conv"][n + m]).any():
            seen.add("convective pattern changes after step 1")
          if (np.abs(t["interval"][m] - prev["interval"][m]) >= 2).any():
            seen.add("a point moves two or more intervals after step 1")
  print(fam, sorted(outcomes), sorted(seen))
  assert {b for b, _ in outcomes} == BASIN_OUTCOMES and {n for _, n in outcomes} == NORTH_OUTCOMES
  want = {"basin set change after step 1", "northern set change after step 1", "both in one step",
          "convective pattern changes after step 1", "no level convects", "every level convects",
          "argmin != 0", "a point moves two or more intervals after step 1", "below the first node",
          "at or above the last node", "upwelling on", "upwelling off"}
  assert want <= seen, (fam, sorted(want - seen))


def test_basin_profiles_are_sorted_but_the_one_made_otherwise():
  for name in F.ROW_NAMES:
    _, trace = F.run(name)
    u = F.row(name)["unsorted"]
    for s, t in enumerate(trace):
      for m in range(F.row(name)["n"]):
        if m != u:
          assert t["sorted"][m], (name, s, m)
    if u is not None:
      c = F.get_case(name)
      assert c["kinds"][u] == 0 and c["bs_SO0"][u, 0] > c["b0"][u, 1]
      assert not trace[0]["sorted"][u]
      ref = F.run(name)[0]
      assert ref[1]["b"][u, 0] > ref[1]["b"][u, 1]  # levels 0 and 1, inverted by the imposed value


def test_zero_psi_members_freeze_the_mixed_layer_only():
  for name in F.ROW_NAMES:
    m = F.row(name)["zero_psi"]
    ref, trace = F.run(name)
    if m is None:
      assert all(t["stepped"].all() for t in trace) and not any(ref[k]["status"].any() for k in ref)
      continue
    c = F.get_case(name)
    assert not c["Psi_SO"][m].any()
    for k in F.STEP_COUNTS:
      assert ref[k]["status"][m] == 1 and ref[k]["status"].sum() == 1
      assert np.array_equal(ref[k]["bs_SO"][m], c["bs_SO0"][m])
      assert (ref[k]["Psi_s"][m] == F.PSI_S0).all() and (ref[k]["Psi_s"][m - 1] != F.PSI_S0).any()
    assert (ref[36]["b"][m] != ref[7]["b"][m]).any()


def test_hand_over_rows_flag_whom_and_when_the_gpu_test_expects():
  f = F.flagged("h1", 0, 36)
  assert np.array_equal(np.nonzero(f)[0], [0, 63, 64, 129])
  first = 0
  for k in F.LAUNCHES:  # their state is outside the window where every launch starts
    assert np.array_equal(F.flagged("h1", first, k), f)
    b = F.run("h1")[0][first]["b"] if first else F.get_case("h1")["b0"]
    assert (~F.in_window(b[[0, 63, 64, 129]])).any(axis=1).all()
    assert F.in_window(np.delete(b[:130], [0, 63, 64, 129], axis=0)).all()
    first += k
  for name in F.ROW_NAMES:
    r, c = F.row(name), F.get_case(name)
    if r["h2"] is None:
      if not r["tiny"]:
        assert not F.sets_outside_window(c).any() and not F.flagged(name, 0, 36).any(), name
      continue
    m, n = r["h2"], r["n"]
    _, trace = F.run(name)
    assert c["kinds"][m] == 1 and c["ksel0"][m] == 0 and c["ksel0"][n + m] == 0
    bad = F.sets_outside_window(c)
    assert bad[1, m] and bad[1, n + m] and bad.sum() == 2
    kb = [t["ksel"][m] for t in trace]
    assert kb[:F.H2_STEP + 1] == [0] * F.H2_STEP + [1], (name, kb)
    assert not any(t["ksel"][n + m] for t in trace)  # its northern column never loads the set
    only = np.zeros(n, dtype=bool)
    only[m] = True
    assert not F.flagged(name, 0, 2).any()
    assert np.array_equal(F.flagged(name, 0, 3), only) and np.array_equal(F.flagged(name, 0, 36), only)
    assert F.H2_NSTEPS == (F.H2_STEP, F.H2_STEP + 1, 36)
    # in the launches (b): 1 and 1 step unflagged, then stopped at step 0 of the third
    assert [bool(F.flagged(name, a, k)[m]) for a, k in ((0, 1), (1, 1), (2, 5))] == [False, False, True]
