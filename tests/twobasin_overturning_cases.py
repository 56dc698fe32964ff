"""Access to fixture G25 (tests/golden/twobasin_overturning.npz, made by
make_golden_twobasin_overturning.py): lines 157-262 of the reference's twobasin_NadeauJansen.py
run on 10 states.  Shared by the CPU and GPU tests."""
import numpy as np

from conftest import load_golden

PROFILES = ("b_Atl", "b_Pac", "b_north", "bs_SO", "Psi_SO_Atl", "Psi_SO_Pac", "Psi_AMOC", "Psi_ZOC",
            "bgrid_AMOC", "psib_AMOC", "bgrid_ZOC", "psib_ZOC")
PACIFIC = ("psiarray_z_Pac", "psiarray_b_Pac", "psiarray_Pac")


def load():
  return load_golden("twobasin_overturning")


def names(G):
  return [str(c) for c in G["cases"]]


def sections(G, c):
  """{psiarray_*, bnew: [nrows][stored levels]} of case c (the fixture keeps them interleaved per
  row and split into byte planes)."""
  nlev = G[c + "_levels"].size
  fields = [str(f) for f in G["section_fields"]]
  a = np.ascontiguousarray(G[c + "_sections"].T).view("<f8").reshape(-1, len(fields), nlev)
  return {f: np.ascontiguousarray(a[:, i]) for i, f in enumerate(fields)}


def case(G, c):
  """Everything of case c: grids, inputs, the reference's rows and its section arrays, and the
  expected bnew_Atl / bnew_Pac (bnew with tiled input rows in the basin, and NaN: :204-205)."""
  nz, ny = int(G[c + "_nz"]), int(G[c + "_ny"])
  n_basin, n_trans, n_north = (int(v) for v in G["n_rows"])
  out = dict(name=c, nz=nz, ny=ny, z=G["z_%d" % nz], y=G["y_%d" % ny], nb=int(G[c + "_nb"]),
             levels=G[c + "_levels"], ynew=G[c + "_ynew"], step=int(G[c + "_step"]),
             A_Atl=float(G[c + "_A_Atl"]), A_Pac=float(G[c + "_A_Pac"]), lengths=G[c + "_lengths"],
             n_basin=n_basin, n_trans=n_trans, n_north=n_north)
  for k in PROFILES:
    out[k] = G[c + "_" + k]
  for k in ("psibz_AMOC", "psibz_ZOC"):
    out[k + "1"], out[k + "2"] = G[c + "_" + k]
  out.update(sections(G, c))
  lev = out["levels"]
  out["full"] = lev.size == nz
  basin, north0 = slice(ny, ny + n_basin), ny + n_basin
  out["bnew_Atl"] = out["bnew"].copy()
  out["bnew_Atl"][basin] = np.tile(out["b_Atl"][lev], (n_basin, 1))
  out["bnew_Pac"] = out["bnew"].copy()
  out["bnew_Pac"][basin] = np.tile(out["b_Pac"][lev], (n_basin, 1))
  out["bnew_Pac"][north0:] = np.nan
  return out
