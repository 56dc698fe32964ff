#!/usr/bin/env python3
"""Generate tests/golden/overturning.npz (G24) by RUNNING THE REFERENCE's figure script.

Run only where the reference checkout is available (read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_overturning.py

G24 overturning   examples/Plot_overturning.py of the reference (pymoc 0.0.1rc5), executed with
runpy on a `diags.npz` written in the positional layout JN2018Diagnostics.save_member uses (only
the last time column is read).  The script is run, never restated: the fixture holds the inputs
and what the script's own globals hold afterwards --
  psiarray_z / psiarray_b / psiarray_res, bnew, ynew     (the three plotted fields, :73-92)
  AMOC.Psi, AMOC.bgrid, AMOC.Psib(nb), AMOC.Psibz(nb)[0], PsiSO.Psi
-- plus the NumPy / SciPy versions (solve_bvp, brenth and np.interp are third-party arithmetic
under the script).  The reference's src/ directory is found as the other generators find it
(PYMOC_REFERENCE_SRC); the script lies next to it.

Cases: the two G7 states (jn2018_nz81 / jn2018_nz200, step 1200), stored in full, and all 14
config-5 members of sweep.npz (c5, c5_long), which keep all 121 rows and every 10th level plus
the top one.  Every case must complete, give finite fields and a non-decreasing b_basin, and
exercise the isopycnal masks; the generator stops otherwise.

Storage: the four section arrays of a case are kept as ONE array `<case>_sections`, the fields
interleaved per row ([nrows][4][levels], order in `section_fields`) and the doubles split into
their eight byte planes (uint8 [8][nrows * 4 * levels], little-endian), and the archive is written
with LZMA.  Rows that the script makes equal (psi_z = psi_res in the channel, psi_b = psi_res and
the tiled b_basin in the basin, the masked copies of one profile in psi_b) then lie within the
compressor's reach: 1.0 MB instead of 1.5 MB, lossless.  np.load reads the archive as any other;
tests/overturning_cases.py undoes the packing.
"""
import os
import runpy
import sys
import io
import tempfile
import warnings
import zipfile

sys.dont_write_bytecode = True
os.environ["MPLBACKEND"] = "Agg"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("PYMOC_REFERENCE_SRC", "/root/reference/src")
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(REF_SRC)), "examples", "Plot_overturning.py")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF_SRC)

import numpy as np
import scipy

from pymoc_amd import configs  # parameter tables only

warnings.simplefilter("ignore")
OUT = dict(numpy_version=np.__version__, scipy_version=scipy.__version__,
           reference="pymoc 0.0.1rc5")
NAMES = []
LEVEL_STEP = 10
SECTION_FIELDS = ("psiarray_z", "psiarray_res", "psiarray_b", "bnew")


def pack(a):
  """float64 array -> its eight byte planes, uint8 [8][a.size]."""
  return np.ascontiguousarray(np.ascontiguousarray(a, dtype="<f8").reshape(-1).view(np.uint8)
                              .reshape(-1, 8).T)


def run_script(z, y, b_basin, b_north, bs_SO, tau, kapGM):
  """The script's globals after it ran on one state."""
  col = lambda v: np.asarray(v, dtype=float)[:, None]
  nz, nb = z.size, 500
  with tempfile.TemporaryDirectory() as tmp:
    # arr_0..arr_10: AMOC, AMOC_b, b_basin, b_north, bs_SO, z, bgrid, y, Psi_SO, tau, kapGM
    np.savez(os.path.join(tmp, "diags.npz"), np.zeros((nz, 1)), np.zeros((nb, 1)), col(b_basin),
             col(b_north), col(bs_SO), z, np.zeros((nb, 1)), y, np.zeros((nz, 1)), tau, kapGM)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
      g = runpy.run_path(SCRIPT)
    finally:
      os.chdir(cwd)
  g["plt"].close("all")
  return g


def case(name, z, y, b_basin, b_north, bs_SO, tau, kapGM, full):
  g = run_script(z, y, b_basin, b_north, bs_SO, tau, kapGM)
  nb = int(g["nb"])
  fields = {k: np.array(g[k]) for k in ("psiarray_z", "psiarray_b", "psiarray_res", "bnew")}
  nrows = y.size + 60 + 10
  for k, v in fields.items():
    assert v.shape == (nrows, z.size), (name, k, v.shape)
    assert np.isfinite(v).all(), (name, k)
  assert np.all(np.diff(b_basin) >= 0) and np.isfinite(b_basin).all(), name
  nonzero = int(np.count_nonzero(fields["psiarray_b"]))
  assert 0.5 * nrows * z.size < nonzero < nrows * z.size, (name, nonzero)
  levels = np.arange(z.size) if full else \
      np.unique(np.concatenate([np.arange(0, z.size, LEVEL_STEP), [z.size - 1]]))
  p = name + "_"
  OUT[p + "levels"] = levels.astype(np.int32)
  OUT[p + "sections"] = pack(np.stack([fields[k][:, levels] for k in SECTION_FIELDS], axis=1))
  OUT[p + "ynew"] = np.array(g["ynew"])
  for key, grid in (("z_%d" % z.size, z), ("y_%d" % y.size, y)):  # shared grids, stored once
    assert key not in OUT or np.array_equal(OUT[key], grid), key
    OUT[key] = grid
  OUT[p + "nz"], OUT[p + "ny"] = np.int32(z.size), np.int32(y.size)
  OUT[p + "b_basin"], OUT[p + "b_north"], OUT[p + "bs_SO"] = b_basin, b_north, bs_SO
  OUT[p + "tau"], OUT[p + "kapGM"] = np.float64(tau), np.float64(kapGM)
  OUT[p + "nb"] = np.int32(nb)
  OUT[p + "lengths"] = np.array([g["lchannel"], g["lbasin"], g["lnorth"]], dtype=float)
  OUT[p + "Psi"] = np.array(g["AMOC"].Psi)
  OUT[p + "bgrid"] = np.array(g["AMOC"].bgrid)
  OUT[p + "psib"] = np.array(g["AMOC"].Psib(nb=nb))
  OUT[p + "psibz1"] = np.array(g["AMOC"].Psibz(nb=nb)[0])
  OUT[p + "Psi_SO"] = np.array(g["PsiSO"].Psi)
  for k in ("Psi", "psibz1", "Psi_SO"):
    assert OUT[p + k].shape == (z.size,) and np.isfinite(OUT[p + k]).all(), (name, k)
  assert OUT[p + "bgrid"].shape == OUT[p + "psib"].shape == (nb,), name
  NAMES.append(name)
  print("%-12s nz %3d  levels kept %3d  psiarray_b non-zero %5d / %5d" %
        (name, z.size, levels.size, nonzero, nrows * z.size), flush=True)


def main():
  g = lambda n: np.load(os.path.join(HERE, n + ".npz"))
  for nz in (81, 200):
    st = g("jn2018_nz%d" % nz)
    m = configs.jn2018_member(nz=nz)
    case("g7_nz%d" % nz, m["z"], m["y"], st["s01200_b_basin"], st["s01200_b_north"],
         st["s01200_bs_SO"], m["tau"], m["KGM"], full=True)
  sw = g("sweep")
  c5 = configs.config5(N=4096)
  for tag in ("c5", "c5_long"):
    for j, i in enumerate(sw[tag + "_members"]):
      case("%s_%d" % (tag, j), c5["z"], c5["y"], sw[tag + "_b_basin"][j], sw[tag + "_b_north"][j],
           sw[tag + "_bs_SO"][j], c5["tau"][i], c5["KGM"][i], full=False)
  assert len(NAMES) == 16, NAMES
  OUT["cases"] = np.array(NAMES)
  OUT["section_fields"] = np.array(SECTION_FIELDS)
  path = os.path.join(HERE, "overturning.npz")
  with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as zf:
    for k, v in OUT.items():
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
      zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                  compress_type=zipfile.ZIP_LZMA)
  size = os.path.getsize(path)
  print("wrote", path, size, "bytes")
  assert size < min(1 << 20, os.path.getsize(os.path.join(HERE, "sweep_full.npz"))), size


if __name__ == "__main__":
  main()
