"""Every variant of the fused Jansen & Nadeau step loop (pm_jn2018_steps) on constructed members,
through the C-ABI descriptor inside guard-banded arenas: bit for bit against the oracle-side
restatement (tests/jn2018_fused_cases.py) in one launch and in launches continuing from each
other, bit for bit against the launch sequence the call replaces, the hand-over of members to the
IEEE follow-up launch at step 0 and at a later step, and the PM_JN_DIV3_PROVEN hint of
JN2018Ensemble following use_hints / set_static.  No tolerance appears: the exact kernels promise
bits.  test_jn2018_fused_cpu.py shows from the trace which out-of-line path each row takes."""
import numpy as np
import pytest

import jn2018_fused_cases as F
from jn2018_members import Members

pytestmark = pytest.mark.gpu
_members, _div3_rows = {}, {}


@pytest.fixture
def members(gpu):
  def get(name):
    if name not in _members:
      r = F.row(name)
      _members[name] = Members(gpu, F.get_case(name), "pm_jn2018_steps", status=r["status"],
                               b_off8=r["b_off8"])
    _members[name].reset()
    return _members[name]
  return get


def _div3_holds(m):
  """The host proof behind PM_JN_DIV3_PROVEN, as JN2018Ensemble._div3 decides it."""
  from pymoc_amd.columns import div3_licensed
  t = m.ml
  den = np.array([t.h, t.L, t.y_host[1] - t.y_host[0]], dtype=np.float64)
  return bool(m.cols.uniform_area and m.cols.div3_proven and F.in_window(den).all() and
              (den != 0).all() and div3_licensed(den))


def _hint_sets(m, r):
  """PM_JN_DIV3_PROVEN off, and on where the proof holds (uniform-Area kernels);
  PM_JN_SHARED_COEF on and off where the rows are shared."""
  sets = [r["hints"]]
  if r["shared"]:
    sets.append(r["hints"] | F.SHARED)
  if F.family(r["kernel"]) != "general":
    _div3_rows[r["name"]] = _div3_holds(m)
    if _div3_rows[r["name"]]:
      sets += [h | F.DIV3 for h in sets]
  return sets


def _equals_oracle(got, ref, flagged, r, what):
  """Every output the launch has, bit for bit; status: the mixed layer's, bit 5 for exactly the
  members handed over, nothing at or above bit 8.  The member whose basin is unsorted on purpose
  is left out (np.interp leaves an unsorted table undefined)."""
  n = r["n"]
  keep = np.ones(n, dtype=bool)
  if r["unsorted"] is not None:
    keep[r["unsorted"]] = False
  assert set(got) == set(ref) - (set() if r["status"] else {"status"})
  for k, g in got.items():
    want = ref[k] | np.where(flagged, 32, 0).astype(np.int32) if k == "status" else ref[k]
    want = np.ascontiguousarray(want).reshape(g.shape).astype(g.dtype)
    rows = np.concatenate([keep, keep]) if g.shape[0] == 2 * n else keep
    assert g[rows].tobytes() == want[rows].tobytes(), (what, k, np.nonzero(
        (g[rows].view(np.uint8).reshape(rows.sum(), -1) != want[rows].view(np.uint8).reshape(rows.sum(), -1))
        .any(axis=1))[0])
  if r["status"]:
    assert not (got["status"] >> 8).any(), what


@pytest.mark.parametrize("name", F.ROW_NAMES)
def test_row_equals_the_oracle_bitwise(gpu, members, name):
  from pymoc_amd._lib import check
  r, m = F.row(name), members(name)
  ref, _ = F.run(name)
  total = max(F.STEP_COUNTS)
  for hints in _hint_sets(m, r):
    m.reset()  # (a) one launch
    check(m.fused(total, hints=hints))
    _equals_oracle(m.outputs(), ref[total], F.flagged(name, 0, total), r, (name, hints, "a"))
    m.reset()  # (b) launches continuing from each other: bbot and ksel carry across
    first = 0
    for k in F.LAUNCHES:
      check(m.fused(k, hints=hints))
      _equals_oracle(m.outputs(), ref[first + k], F.flagged(name, first, k), r,
                     (name, hints, "b", first, k))
      first += k
    assert first == total
  z = r["zero_psi"]
  if z is not None:  # the mixed layer frozen, Psi_s never written, the columns stepping
    out = m.outputs()
    assert np.array_equal(out["bs_SO"][z], m.case["bs_SO0"][z]) and (out["Psi_s"][z] == F.PSI_S0).all()
    assert (out["b"][z] != m.case["b0"][z]).any() and (out["Psi_s"][z - 1] != F.PSI_S0).any()
    assert not r["status"] or out["status"][z, 0] == 1


def test_div3_hint_ran_in_both_lane_shapes(gpu, members):
  """The proof holds on the rows' grids, so PM_JN_DIV3_PROVEN did run above (or runs here)."""
  for name in ("f64", "f200"):
    if name not in _div3_rows:
      _div3_rows[name] = _div3_holds(members(name))
    assert _div3_rows[name], name


@pytest.mark.parametrize("name", [n for n in F.ROW_NAMES if F.row(n)["h2"] is not None])
def test_hand_over_after_s_steps(gpu, members, name):
  """H2: the member's basin column selects a coefficient set outside the window in step index 2.
  nsteps = 2: not reached, bit 5 clear; 3: reached in the last step; 36: the IEEE launch takes 34."""
  from pymoc_amd._lib import check
  r, m = F.row(name), members(name)
  ref, _ = F.restatement(F.get_case(name), F.H2_NSTEPS)
  for k in F.H2_NSTEPS:
    fl = F.flagged(name, 0, k)
    assert fl[r["h2"]] == (k > F.H2_STEP) and fl.sum() == int(k > F.H2_STEP)
    for hints in (r["hints"], r["hints"] | F.DIV3) if _div3_holds(m) else (r["hints"],):
      m.reset()
      check(m.fused(k, hints=hints))
      got = m.outputs()
      _equals_oracle(got, ref[k], fl, r, (name, k, hints))
      assert np.array_equal((got["status"].ravel() & 32) != 0, fl)


@pytest.mark.parametrize("name", [n for n in F.ROW_NAMES if F.row(n)["sequence"]])
def test_fused_equals_the_launch_sequence_bitwise(gpu, members, name):
  """pm_jn2018_bc_switch + ColumnBatch.steps(..., 1) + SOMLBatch.step per step, against one fused
  launch of as many steps: every member, the unsorted one and the handed-over ones included.
  (Bit 5 of status is the fused call's own; the sequence has no such bit.)"""
  from pymoc_amd._lib import check
  r, m = F.row(name), members(name)
  fused = {}
  for k in F.STEP_COUNTS:
    m.reset()
    check(m.fused(k, hints=r["hints"]))
    fused[k] = m.outputs()
  m.reset()
  done = 0
  for k in F.STEP_COUNTS:
    m.sequence(k - done, "explicit")
    done = k
    want = m.outputs()
    for key, w in want.items():
      g = fused[k][key] & ~np.int32(32) if key == "status" else fused[k][key]
      assert g.tobytes() == w.tobytes(), (name, k, key)
    fl = F.flagged(name, 0, k)
    assert np.array_equal((fused[k]["status"].ravel() & 32) != 0, fl), (name, k)
  assert np.isfinite(want["b"]).all() and (want["b"] != m.case["b0"]).any()


def test_div3_hint_follows_use_hints_and_set_static(gpu):
  """JN2018Ensemble sends PM_JN_DIV3_PROVEN on the columns' PRESENT proof: use_hints(div3=False)
  and a set_static whose Area is not proven (a subnormal) withdraw it, and it comes back."""
  from pymoc_amd import _lib, configs
  n = 2
  cfg = configs.config5(N=n, nz=46, dt_days=30.)
  ens = gpu.JN2018Ensemble(cfg)
  hint = lambda: bool(ens._jn_descriptor().hints & _lib.PM_JN_DIV3_PROVEN)  # noqa: E731
  assert ens.cols.div3_proven and hint()
  ens.cols.use_hints(div3=False)
  assert not hint()
  ens.cols.use_hints()
  assert hint()
  rd = lambda k: ens.read(cfg, k, n)  # noqa: E731
  kap, kapeff = np.concatenate([rd("kappa")] * 2), np.concatenate([rd("kappaeff")] * 2)
  area = np.concatenate([rd("A_basin"), rd("A_north")])
  area = area if area.ndim == 2 else np.repeat(area[:, None], ens.nz, axis=1)
  unproven = area.copy()
  unproven[1] = 2.0 ** -1060
  ens.cols.set_static(kap, unproven, kapeff)
  assert ens.cols.uniform_area and not ens.cols.div3_proven
  d = ens._jn_descriptor()
  assert d.hints & _lib.PM_JN_UNIFORM_AREA and not d.hints & _lib.PM_JN_DIV3_PROVEN
  ens.cols.set_static(kap, area, kapeff)
  assert hint()
