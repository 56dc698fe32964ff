#!/usr/bin/env python3
"""Generate tests/golden/twobasin_overturning.npz (G25) by RUNNING THE REFERENCE's two-basin
script's own section code on states stepped with the reference's classes.

Run only where the reference checkout is available (read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_twobasin_overturning.py

G25 two-basin overturning   examples/twobasin_NadeauJansen.py of the reference (pymoc 0.0.1rc5).
The script's time loop holds a Python-2 `print`, so runpy cannot run the file.  This generator
builds the script's objects (Atl, north, Pac, AMOC, ZOC, SO_Atl, SO_Pac) from a parameter table
and steps them with the reference's classes exactly as `ref_twobasin` of make_golden.py does
(:101-122 of the script); then it READS THE SCRIPT FILE and `exec`s its lines from `blevs=` up to
the comment `# plot z-coordinate overturning` (:157-262) in a namespace that holds those objects.
The script's text runs and is never restated, and none of it is stored.  The slice spells NaN
`np.NaN`, an alias NumPy >= 2 dropped: the generator sets `np.NaN = np.nan` when it is absent.

The fixture holds the inputs -- the three columns' b, bs_SO, the areas, the four overturnings,
both thermal winds' bgrid / Psib and all four Psibz rows -- and what the script's namespace holds
afterwards: ynew, the eight psiarray_* fields and bnew (bnew_Atl / bnew_Pac differ from bnew by
tiled input rows and NaN only; they are checked here and rebuilt by the tests), plus the NumPy /
SciPy versions.

Cases: the nominal configs.twobasin_member(nz=80) at step 121 (overturnings fresh: 121 % 24 = 1),
stored in full, and at step 1200 (overturnings 23 steps older than the columns); the eight
config_twobasin(N=2048) members arange(0, 2048, 256) of G9 at step 121.  All but the first keep
every 10th level plus the top one.  Every case must give finite non-Pacific fields, exactly
(n_trans + n_north) * nz NaNs in each Pacific field, non-decreasing b_basin / b_Atl / b_Pac and
bgrids, and exercise the isopycnal masks; the generator stops otherwise.

Storage: as make_golden_overturning.py -- a case's nine section arrays as ONE array
`<case>_sections`, interleaved per row ([nrows][9][levels], order in `section_fields`), split
into eight byte planes, LZMA.  tests/twobasin_overturning_cases.py undoes the packing.
"""
import io
import os
import sys
import warnings
import zipfile

sys.dont_write_bytecode = True
os.environ["MPLBACKEND"] = "Agg"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("PYMOC_REFERENCE_SRC", "/root/reference/src")
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(REF_SRC)), "examples",
                      "twobasin_NadeauJansen.py")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF_SRC)

import numpy as np
import scipy

if not hasattr(np, "NaN"):
  np.NaN = np.nan  # the script's spelling (:246-262)

from pymoc.modules import Psi_Thermwind, Psi_SO, Column
from pymoc.plotting import Interpolate_channel, Interpolate_twocol

from pymoc_amd import configs  # parameter tables only

warnings.simplefilter("ignore")
OUT = dict(numpy_version=np.__version__, scipy_version=scipy.__version__,
           reference="pymoc 0.0.1rc5")
NAMES = []
LEVEL_STEP = 10
N_BASIN, N_TRANS, N_NORTH = 60, 20, 20
SECTION_FIELDS = ("psiarray_z", "psiarray_z_Atl", "psiarray_z_Pac", "psiarray_b", "psiarray_b_Atl",
                  "psiarray_b_Pac", "psiarray_Atl", "psiarray_Pac", "bnew")
PACIFIC = ("psiarray_z_Pac", "psiarray_b_Pac", "psiarray_Pac")


def script_slice():
  """The text of :157-262, read from the reference's file."""
  lines = open(SCRIPT).read().split("\n")
  first = [i for i, ln in enumerate(lines) if ln.startswith("blevs=")]
  last = [i for i, ln in enumerate(lines) if ln.startswith("# plot z-coordinate overturning")]
  assert len(first) == 1 and len(last) == 1 and first[0] < last[0], (first, last)
  return compile("\n".join(lines[first[0]:last[0]]), SCRIPT + ":slice", "exec")


def pack(a):
  """float64 array -> its eight byte planes, uint8 [8][a.size]."""
  return np.ascontiguousarray(np.ascontiguousarray(a, dtype="<f8").reshape(-1).view(np.uint8)
                              .reshape(-1, 8).T)


class Model(object):
  """The script's objects for one member (:64-90) and its loop body (:102-122)."""

  def __init__(self, m):
    z, y = m['z'], m['y']
    self.m, self.ii = m, 0
    self.AMOC = Psi_Thermwind(z=z, b1=m['b_Atl0'].copy(), b2=m['b2_init'].copy(), f=m['f_AMOC'])
    self.AMOC.solve()
    [self.Psi_iso_Atl, self.Psi_iso_N] = self.AMOC.Psibz()
    self.ZOC = Psi_Thermwind(z=z, b1=m['b_Atl0'].copy(), b2=m['b_Pac0'].copy(), f=m['f_ZOC'])
    self.ZOC.solve()
    [self.Psi_zonal_Atl, self.Psi_zonal_Pac] = self.ZOC.Psibz()
    so = lambda b, L: Psi_SO(z=z, y=y, b=b.copy(), bs=m['bs_SO'].copy(), tau=float(m['tau']),  # noqa
                             L=L, KGM=float(m['K']))
    self.SO_Atl, self.SO_Pac = so(m['b_Atl0'], m['L_Atl']), so(m['b_Pac0'], m['L_Pac'])
    self.SO_Atl.solve()
    self.SO_Pac.solve()
    mk = lambda b, bs, A: Column(z=z, kappa=m['kappa'].copy(), b=b.copy(), bs=bs,  # noqa
                                 bbot=m['bbot'], Area=float(A), N2min=m['N2min'])
    self.Atl = mk(m['b_Atl0'], m['bs'], m['A_Atl'])
    self.north = mk(m['b_north0'], m['bs_north'], m['A_north'])
    self.Pac = mk(m['b_Pac0'], m['bs'], m['A_Pac'])

  def run_to(self, nsteps):
    m = self.m
    AMOC, ZOC, SO_Atl, SO_Pac = self.AMOC, self.ZOC, self.SO_Atl, self.SO_Pac
    Atl, north, Pac = self.Atl, self.north, self.Pac
    for ii in range(self.ii, nsteps):
      wA_Atl = (self.Psi_iso_Atl + self.Psi_zonal_Atl - SO_Atl.Psi) * 1e6
      wAN = -self.Psi_iso_N * 1e6
      wA_Pac = (-self.Psi_zonal_Pac - SO_Pac.Psi) * 1e6
      Atl.timestep(wA=wA_Atl, dt=m['dt'])
      north.timestep(wA=wAN, dt=m['dt'], do_conv=True)
      Pac.timestep(wA=wA_Pac, dt=m['dt'])
      if ii % m['MOC_up_iters'] == 0:
        AMOC.update(b1=Atl.b, b2=north.b)
        AMOC.solve()
        [self.Psi_iso_Atl, self.Psi_iso_N] = AMOC.Psibz()
        ZOC.update(b1=Atl.b, b2=Pac.b)
        ZOC.solve()
        [self.Psi_zonal_Atl, self.Psi_zonal_Pac] = ZOC.Psibz()
        SO_Atl.update(b=Atl.b)
        SO_Atl.solve()
        SO_Pac.update(b=Pac.b)
        SO_Pac.solve()
    self.ii = nsteps

  def namespace(self):
    """What the script's globals hold when its loop is done, as far as :157-262 read them."""
    m = self.m
    return dict(np=np, Interpolate_channel=Interpolate_channel,
                Interpolate_twocol=Interpolate_twocol, y=m['y'], z=m['z'],
                bs_SO=m['bs_SO'].copy(), A_Atl=float(m['A_Atl']), A_Pac=float(m['A_Pac']),
                Atl=self.Atl, north=self.north, Pac=self.Pac, AMOC=self.AMOC, ZOC=self.ZOC,
                SO_Atl=self.SO_Atl, SO_Pac=self.SO_Pac)


def nondecreasing(a):
  return bool(np.isfinite(a).all() and np.all(np.diff(a) >= 0))


def case(name, model, code, full):
  m = model.m
  z, y = m['z'], m['y']
  nz, ny = z.size, y.size
  inputs = dict(b_Atl=model.Atl.b.copy(), b_Pac=model.Pac.b.copy(), b_north=model.north.b.copy(),
                bs_SO=m['bs_SO'].copy())
  g = model.namespace()
  exec(code, g)
  nb = int(g["nb"])
  assert nb == int(m['nb']), nb
  for k, v in inputs.items():  # the slice changes none of its inputs
    ref = dict(b_Atl=model.Atl.b, b_Pac=model.Pac.b, b_north=model.north.b, bs_SO=m['bs_SO'])[k]
    assert np.array_equal(v, ref), (name, k)
  fields = {k: np.array(g[k]) for k in SECTION_FIELDS}
  nrows = ny + N_BASIN + N_TRANS + N_NORTH
  for k, v in fields.items():
    assert v.shape == (nrows, nz), (name, k, v.shape)
    if k in PACIFIC:
      assert int(np.isnan(v).sum()) == (N_TRANS + N_NORTH) * nz, (name, k)
      assert np.isfinite(v[:ny + N_BASIN]).all(), (name, k)
    else:
      assert np.isfinite(v).all(), (name, k)
  AMOC, ZOC = g["AMOC"], g["ZOC"]
  for k in ("b_basin",):
    assert nondecreasing(g[k]), (name, k)
  assert nondecreasing(inputs["b_Atl"]) and nondecreasing(inputs["b_Pac"]), name
  nonzero = int(np.count_nonzero(fields["psiarray_b"]))
  assert 0.5 * nrows * nz < nonzero < nrows * nz, (name, nonzero)
  # bnew_Atl / bnew_Pac: bnew with the basin rows replaced by a tiled input row, and NaN
  basin, north0 = slice(ny, ny + N_BASIN), ny + N_BASIN
  want = fields["bnew"].copy()
  want[basin] = np.tile(inputs["b_Atl"], (N_BASIN, 1))
  assert np.array_equal(np.array(g["bnew_Atl"]), want), name
  want[basin] = np.tile(inputs["b_Pac"], (N_BASIN, 1))
  want[north0:] = np.nan
  assert np.array_equal(np.array(g["bnew_Pac"]), want, equal_nan=True), name
  levels = np.arange(nz) if full else \
      np.unique(np.concatenate([np.arange(0, nz, LEVEL_STEP), [nz - 1]]))
  p = name + "_"
  OUT[p + "levels"] = levels.astype(np.int32)
  OUT[p + "sections"] = pack(np.stack([fields[k][:, levels] for k in SECTION_FIELDS], axis=1))
  OUT[p + "ynew"] = np.array(g["ynew"])
  for key, grid in (("z_%d" % nz, z), ("y_%d" % ny, y)):  # shared grids, stored once
    assert key not in OUT or np.array_equal(OUT[key], grid), key
    OUT[key] = grid
  OUT[p + "nz"], OUT[p + "ny"], OUT[p + "nb"] = np.int32(nz), np.int32(ny), np.int32(nb)
  OUT[p + "step"] = np.int32(model.ii)
  for k, v in inputs.items():
    OUT[p + k] = v
  OUT[p + "A_Atl"], OUT[p + "A_Pac"] = np.float64(m['A_Atl']), np.float64(m['A_Pac'])
  OUT[p + "lengths"] = np.array([g["lchannel"], g["lbasin"], g["ltrans"], g["lnorth"]], dtype=float)
  OUT[p + "Psi_SO_Atl"], OUT[p + "Psi_SO_Pac"] = np.array(g["SO_Atl"].Psi), np.array(g["SO_Pac"].Psi)
  OUT[p + "Psi_AMOC"], OUT[p + "Psi_ZOC"] = np.array(AMOC.Psi), np.array(ZOC.Psi)
  OUT[p + "psib_AMOC"] = np.array(AMOC.Psib(nb=nb))
  OUT[p + "bgrid_AMOC"] = np.array(AMOC.bgrid)
  OUT[p + "psib_ZOC"] = np.array(ZOC.Psib())
  OUT[p + "bgrid_ZOC"] = np.array(ZOC.bgrid)
  OUT[p + "psibz_AMOC"] = np.array(AMOC.Psibz(nb=nb))
  OUT[p + "psibz_ZOC"] = np.array(ZOC.Psibz())
  assert nondecreasing(OUT[p + "bgrid_AMOC"]) and nondecreasing(OUT[p + "bgrid_ZOC"]), name
  assert OUT[p + "bgrid_AMOC"].shape == OUT[p + "psib_AMOC"].shape == (nb,), name
  assert OUT[p + "bgrid_ZOC"].shape == OUT[p + "psib_ZOC"].shape == (nb,), name
  assert OUT[p + "psibz_AMOC"].shape == OUT[p + "psibz_ZOC"].shape == (2, nz), name
  for k in ("Psi_SO_Atl", "Psi_SO_Pac", "Psi_AMOC", "Psi_ZOC", "psibz_AMOC", "psibz_ZOC"):
    assert np.isfinite(OUT[p + k]).all(), (name, k)
  NAMES.append(name)
  print("%-14s step %4d  levels kept %3d  Pacific NaNs %4d  psiarray_b non-zero %5d / %5d" %
        (name, model.ii, levels.size, int(np.isnan(fields["psiarray_Pac"]).sum()), nonzero,
         nrows * nz), flush=True)


def main():
  code = script_slice()
  model = Model(configs.twobasin_member(nz=80))
  model.run_to(121)
  case("nominal_s0121", model, code, full=True)
  model.run_to(1200)
  case("nominal_s1200", model, code, full=False)
  c = configs.config_twobasin(N=2048)
  for i in np.arange(0, 2048, 256):
    mm = dict(c)
    for k in ('tau', 'K', 'A_Pac', 'A_Atl', 'A_north'):
      mm[k] = c[k][i]
    model = Model(mm)
    model.run_to(121)
    case("sweep_%04d" % i, model, code, full=False)
  assert len(NAMES) == 10, NAMES
  OUT["cases"] = np.array(NAMES)
  OUT["section_fields"] = np.array(SECTION_FIELDS)
  OUT["n_rows"] = np.array([N_BASIN, N_TRANS, N_NORTH], dtype=np.int32)
  path = os.path.join(HERE, "twobasin_overturning.npz")
  with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as zf:
    for k, v in OUT.items():
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
      zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                  compress_type=zipfile.ZIP_LZMA)
  size = os.path.getsize(path)
  print("wrote", path, size, "bytes")
  assert size < (1 << 20), size


if __name__ == "__main__":
  main()
