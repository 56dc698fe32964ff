"""the two-basin topology (examples/twobasin_NadeauJansen.py) on the GPU."""
import numpy as np
import pytest

import twobasin_cases as B
from oracle import drivers
from conftest import load_golden, relerr
from pymoc_amd import configs

pytestmark = pytest.mark.gpu

FIELDS = ("b_Atl", "b_north", "b_Pac", "Psi_AMOC", "Psi_ZOC", "Psi_SO_Atl", "Psi_SO_Pac")


def test_twobasin_trajectory_golden(gpu):
  g = load_golden("twobasin")
  m = configs.twobasin_member(nz=80)
  ens = gpu.TwoBasinEnsemble(m)
  snaps = (1, 24, 25, 26, 1200)
  orc = drivers.run_twobasin(m, 1200, set(snaps))
  done = 0
  for s in snaps:
    ens.run(s - done)
    done = s
    st = ens.state()
    for k in FIELDS:
      assert relerr(st[k][0], g["s%05d_%s" % (s, k)]) <= 1e-10, (s, k)
      assert relerr(st[k][0], orc[s][k]) <= 1e-10, (s, k)


def test_twobasin_sweep_members_vs_reference(gpu):
  g = load_golden("twobasin")
  c = configs.config_twobasin(N=2048)
  ens = gpu.TwoBasinEnsemble(c)
  n = int(g["sweep_nsteps"])
  ens.run(n)
  st = ens.state()
  idx = g["sweep_members"]
  for k in ("b_Atl", "b_north", "b_Pac", "Psi_AMOC", "Psi_ZOC", "Psi_SO_Atl"):
    assert relerr(st[k][idx], g["sweep_" + k]) <= 1e-10, k
  assert ens.nonfinite_members().size == 0


def test_twobasin_update_pairs_side_by_side_equal_four_launches(gpu):
  """Round 5: an update is two one-launch pairs {Psi_SO.solve, thermal wind} on two streams; the
  result equals four separate launches in the script's order bit for bit, and so do the gathers
  of the seven sampled fields at the driver's cadence."""
  c = configs.config_twobasin(N=96)
  s = gpu.Stream()
  # default: the pairs one after the other, the forcing formed by the column kernel
  a = gpu.TwoBasinEnsemble(c, stream=s, keep_history=True, diag_iters=48)
  assert a._forcing_in_k1 and not a._overlap
  # the pairs on two streams, whole intervals replayed from a hipGraph
  a2 = gpu.TwoBasinEnsemble(c, stream=s, keep_history=True, diag_iters=48, overlap_updates=True)
  # ... eagerly, and the forcing by pm_twobasin_forcing (round 5's first form)
  b = gpu.TwoBasinEnsemble(c, stream=s, keep_history=True, diag_iters=48, overlap_updates=True,
                           use_graph=False)
  b._forcing_in_k1 = False
  d = gpu.TwoBasinEnsemble(c, keep_history=True, diag_iters=48, overlap_updates=False)
  d._pairs = False  # four separate launches (what round 4 ran)
  d._forcing_in_k1 = False
  for e in (a, a2, b, d):
    e.run(130)
    e.gather_diagnostics()
  assert a2._graph is not None and a._graph is None and b._graph is None
  sa = a.state()
  for e in (a2, b, d):
    st = e.state()
    for k in FIELDS:
      assert np.array_equal(sa[k], st[k]), k
    assert [x for x, _ in e.diag.history] == [x for x, _ in a.diag.history] == [0, 48, 96, 130]
    for (_, ha), (_, hb) in zip(a.diag.history, e.diag.history):
      for k in FIELDS:
        assert np.array_equal(ha[k], hb[k]), k
  for k in FIELDS:
    assert np.array_equal(a.diag.history[-1][1][k], sa[k]), k


def _run_splits(ens):
  """The seven fields after each of B.SPLITS."""
  out = []
  for n in B.SPLITS:
    ens.run(n)
    out.append(ens.state())
  return out


@pytest.mark.parametrize("shape", B.SHAPES, ids=B.label)
def test_twobasin_other_shapes_internal_equalities_and_oracle(gpu, shape):
  """The driver away from nz = 80, ny = 51 (twobasin_cases.SHAPES; nz = 300 takes the separate
  Psi_SO / thermal-wind launches and columns of five levels per lane), run in splits that make
  launches with the forcing as an array (1-2 steps) and formed by the column kernel (>= 3)
  alternate: the default ensemble, one with the forcing always from pm_twobasin_forcing and one
  with four separate update launches agree bit for bit in all seven fields after every split, and
  two members agree with the oracle's driver to 1e-10 at steps 1, M + 1 and 2 M + 4.

  The worst distance to the oracle per shape (max-norm relative to max|ref|, all seven fields,
  members 0 and 5, the three steps) is printed before it is asserted.  Measured on an MI355X:
    nz =  17, ny =  9: 5.02e-16      nz = 129, ny = 51: 8.17e-16
    nz =  46, ny = 51: 5.53e-16      nz = 200, ny = 51: 6.33e-16
    nz =  81, ny = 33: 4.58e-16      nz = 300, ny = 65: 1.69e-15"""
  nz = shape[0]
  c = B.cfg(shape)
  a = gpu.TwoBasinEnsemble(c)
  assert a._forcing_in_k1 and a._pairs == (nz <= 256)
  b = gpu.TwoBasinEnsemble(c)
  b._forcing_in_k1 = False
  d = gpu.TwoBasinEnsemble(c)
  d._pairs = False
  sa, sb, sd = _run_splits(a), _run_splits(b), _run_splits(d)
  for i in range(len(B.SPLITS)):
    for k in FIELDS:
      assert np.array_equal(sa[i][k], sb[i][k]), (i, k)
      assert np.array_equal(sa[i][k], sd[i][k]), (i, k)
  assert a.nonfinite_members().size == 0
  worst = 0.0
  steps = list(np.cumsum(B.SPLITS))
  for m in B.MEMBERS:
    orc = B.oracle_snaps(shape, m)
    for s in B.SNAPS:
      st = sa[steps.index(s)]
      for k in FIELDS:
        worst = max(worst, relerr(st[k][m], orc[s][k]))
  print("%s: worst distance to the oracle %.3g" % (B.label(shape), worst))
  assert worst <= 1e-10, worst


@pytest.mark.parametrize("lanes", [16, 32])
def test_twobasin_lane_choice_changes_no_bit(gpu, lanes):
  shape = (81, 33, 30)
  c = B.cfg(shape)
  ref = _run_splits(gpu.TwoBasinEnsemble(c))
  got = _run_splits(gpu.TwoBasinEnsemble(c, lanes_per_col=lanes))
  for i in range(len(B.SPLITS)):
    for k in FIELDS:
      assert np.array_equal(ref[i][k], got[i][k]), (i, k)


def test_twobasin_contracted_columns_within_tolerance(gpu):
  c = configs.config_twobasin(N=64)
  a, b = gpu.TwoBasinEnsemble(c), gpu.TwoBasinEnsemble(c, arith="contracted")
  a.run(600)
  b.run(600)
  sa, sb = a.state(), b.state()
  for k in FIELDS:
    assert relerr(sb[k], sa[k]) <= 1e-11, k
