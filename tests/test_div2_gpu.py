"""The 2-instruction exact quotients of k_column_steps<64,P,6,...> (PM_COLS_DIV2_GRID /
PM_COL_DIV2_AREA): the device's sequence on the proof's candidate numerators, and bit identity of
the fused launches with the other quotient forms and with the oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from pymoc_amd import _lib, configs

pytestmark = pytest.mark.gpu


def _batch(gpu, c, **kw):
  return gpu.ColumnBatch(c["z"], c["kappa"], c["Area"], c["b0"], bs=c["bs"], bbot=c["bbot"],
                         N2min=c["N2min"], do_conv=c["do_conv"], **kw)


def _oracle(c, nsteps, dt=None):
  return O.column_ensemble_steps(c["z"], c["kappa"], c["Area"], c["b0"], c["wA"],
                                 c["dt"] if dt is None else dt, c["do_conv"], c["bs"], c["bbot"],
                                 c["N2min"], nsteps)


def _host_proven(d):
  d = np.ascontiguousarray(d, dtype=np.float64)
  ok, nc = np.zeros(d.size, dtype=np.int32), C.c_int64(0)
  _lib.check(_lib.lib.pm_div2_proven(d.ctypes.data, d.size, ok.ctypes.data, C.byref(nc)))
  return ok.astype(bool), nc.value


def _grid_denominators(z):
  dz = np.diff(z)
  return np.concatenate([np.unique(dz), np.unique(0.5 * (dz[1:] + dz[:-1]))])


def test_device_two_instruction_quotient_on_the_candidates(gpu):
  """pm_selftest_div2: the DEVICE's 2-instruction sequence (reciprocal pair formed on the device) on
  the candidate numerators of 2^16 denominators against the host's `/`: no difference on any
  denominator the host proof accepts.  The proof does reject some, and their candidates do differ."""
  tested, bad, unproven, ubad = (C.c_uint64(0) for _ in range(4))
  _lib.check(_lib.lib.pm_selftest_div2(20246, 1 << 16, C.byref(tested), C.byref(bad),
                                       C.byref(unproven), C.byref(ubad)))
  print("pairs", tested.value, "mismatches on proven", bad.value, "unproven denominators",
        unproven.value, "mismatches on unproven", ubad.value)
  assert tested.value > (1 << 16)
  assert bad.value == 0
  assert 0 < unproven.value < (1 << 16) and ubad.value > 0


def test_device_reciprocal_pair_matches_the_hosts(gpu):
  """pm_recip2_check on config 2's denominators: the device forms the pair the proof assumed."""
  c = configs.config2(N=1024)
  d = np.concatenate([_grid_denominators(c["z"]), c["Area"][:, 0]])
  ok = np.zeros(d.size, dtype=np.int32)
  _lib.check(_lib.lib.pm_recip2_check(d.ctypes.data, d.size, ok.ctypes.data))
  assert ok.all()


@pytest.fixture(scope="module")
def c2_four_classes(gpu):
  """config2(N=128) with the four classes (Area div2-proven or not) x (do_conv or not) present:
  where N = 128 lacks an unproven class, Areas of config2(N=1024) that fail the proof replace the
  first members' (their forcing rescaled with the Area, as the config forms it)."""
  c = configs.config2(N=128)
  c = dict(c, Area=c["Area"].copy(), wA=c["wA"].copy())
  proven, _ = _host_proven(c["Area"][:, 0])
  big = configs.config2(N=1024)["Area"][:, 0]
  failing = list(big[~_host_proven(big)[0]])
  assert failing
  for conv in (False, True):
    if not np.any(~proven & (c["do_conv"] == conv)):
      m = int(np.flatnonzero(c["do_conv"] == conv)[0])
      a = failing.pop()
      c["wA"][m] *= a / c["Area"][m, 0]
      c["Area"][m, :] = a
      proven[m] = False
  return c, proven


@pytest.mark.parametrize("nsteps", [3, 24, 250])
def test_two_instruction_quotients_bitwise(gpu, c2_four_classes, nsteps):
  """Hints on (2-instruction quotients where proven), use_hints(div2=False) (3-instruction) and
  use_hints(div3=False) (4-instruction): the same bits, and the oracle's, for every member -- among
  them all four of (Area proven or not) x (do_conv or not), taken from the stored verdicts.  250
  steps run the 16-, 4- and 1-step blocks of the speculative convective loop.  The kernel keeps its
  name: the form is chosen inside the instantiation."""
  c, host_verdict = c2_four_classes
  full, d3, d4 = _batch(gpu, c), _batch(gpu, c), _batch(gpu, c)
  d3.use_hints(div2=False)
  d4.use_hints(div3=False)
  assert full.div3_proven and full.div2_grid_proven
  assert np.array_equal(full.div2_area_proven, host_verdict)
  for conv in (False, True):
    for ok in (False, True):
      assert np.any((full.div2_area_proven == ok) & (c["do_conv"] == conv)), (conv, ok)
  r = full.descriptor().reserved
  assert r & _lib.PM_COLS_DIV3_PROVEN and r & _lib.PM_COLS_DIV2_GRID
  assert d3.descriptor().reserved & _lib.PM_COLS_DIV3_PROVEN
  assert not d3.descriptor().reserved & _lib.PM_COLS_DIV2_GRID
  assert not d4.descriptor().reserved & (_lib.PM_COLS_DIV3_PROVEN | _lib.PM_COLS_DIV2_GRID)
  flags = full.flags.download()
  assert np.array_equal((flags & _lib.PM_COL_DIV2_AREA) != 0, host_verdict)
  assert not (d3.flags.download() & _lib.PM_COL_DIV2_AREA).any()
  assert not (d4.flags.download() & _lib.PM_COL_DIV2_AREA).any()
  assert full.kernel_name(nsteps) == "k_column_steps<64,2,6,true,true>"
  assert d3.kernel_name(nsteps) == "k_column_steps<64,2,6,true,true>"
  assert d4.kernel_name(nsteps) == "k_column_steps<64,2,2,true,true>"
  wA = gpu.DeviceArray.from_host(c["wA"])
  for b in (full, d3, d4):
    b.steps(wA, c["dt"], nsteps)
  got = full.get_b()
  assert np.array_equal(got, d3.get_b())
  assert np.array_equal(got, d4.get_b())
  assert np.array_equal(got, _oracle(c, nsteps))
  assert full.get_nonfinite().sum() == 0


def test_proven_batch_with_four_levels_per_lane(gpu):
  """nz = 256: P = 4.  The choice among the step forms exists for P <= 2 only (at P = 3 and 4 its three
  legs cost a resident wave per SIMD), so this batch -- grid proven, Areas proven and not -- carries
  both hints and `<64,4,6,...>` must ignore them: the oracle's bits from the 3-instruction form."""
  c = configs.config2(N=24, nz=256)
  dt = c["dt"] / 8  # (the explicit scheme's limit at this spacing)
  batch = _batch(gpu, c)
  assert batch.div3_proven and batch.kernel_name(9) == "k_column_steps<64,4,6,true,true>"
  assert batch.div2_grid_proven and 0 < batch.div2_area_proven.sum() < 24
  assert batch.descriptor().reserved & _lib.PM_COLS_DIV2_GRID
  batch.steps(c["wA"], dt, 9)
  assert np.array_equal(batch.get_b(), _oracle(c, 9, dt))


def test_two_instruction_quotients_with_bottom_gradient(gpu):
  """bzbot set (column.py:232-233): the loops that re-impose the boundary values every step (they
  still read dz[0]), with and without convection."""
  c = configs.config2(N=16)
  bzbot = 1e-7
  batch = _batch(gpu, c, bzbot=bzbot)
  assert batch.has_bzbot and batch.div2_grid_proven and batch.div2_area_proven.any()
  assert batch.kernel_name(7) == "k_column_steps<64,2,6,true,true>"
  batch.steps(c["wA"], c["dt"], 7)
  got = batch.get_b()
  for m in range(16):
    ref = c["b0"][m].copy()
    for _ in range(7):
      ref = O.column_timestep(c["z"], c["kappa"][m], c["Area"][m], ref, c["wA"][m], c["dt"],
                              do_conv=bool(c["do_conv"][m]), bs=c["bs"][m], bbot=c["bbot"][m],
                              bzbot=bzbot, N2min=c["N2min"][m])
    assert np.array_equal(got[m], ref), m


@pytest.mark.parametrize("want_proven", [True, False])
def test_grid_hint_follows_the_proof(gpu, want_proven):
  """A grid with a spacing of fewer than three trailing zero bits in its mantissa (the level below
  the surface moved: the top spacing is then that level's depth, any mantissa at all) has candidate
  numerators, and the grid hint is what the proof says about them: one such grid that passes, one
  that fails (and keeps the 3-instruction form throughout).  Bitwise against the oracle."""
  c = configs.config2(N=16)
  z0 = c["z"]
  found = None
  for k in range(1, 4000):
    z = z0.copy()
    z[-2] = -(40.25 + (2 * k + 1) * 2.0**-47)  # odd mantissa: no trailing zero bit
    d = _grid_denominators(z)
    ok, ncand = _host_proven(d)
    if ncand > 0 and bool(ok.all()) == want_proven:
      found = z
      break
  assert found is not None
  mant = np.frexp(d)[0] * 2.0**53
  assert min((int(m) & -int(m)).bit_length() - 1 for m in mant) < 3
  c = dict(c, z=found)
  batch = _batch(gpu, c)
  assert batch.div3_proven
  assert batch.div2_grid_proven == want_proven
  assert bool(batch.descriptor().reserved & _lib.PM_COLS_DIV2_GRID) == want_proven
  if not want_proven:
    assert not batch.div2_area_proven.any()
  assert batch.kernel_name(24) == "k_column_steps<64,2,6,true,true>"
  batch.steps(c["wA"], c["dt"], 24)
  assert np.array_equal(batch.get_b(), _oracle(c, 24))
