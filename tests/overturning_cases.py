"""Access to fixture G24 (tests/golden/overturning.npz, made by make_golden_overturning.py): the
reference's Plot_overturning.py run on 16 states.  Shared by the CPU and GPU tests."""
import numpy as np

from conftest import load_golden

N_BASIN, N_NORTH = 60, 10
PROFILES = ("b_basin", "bs_SO", "Psi", "Psi_SO", "bgrid", "psib", "psibz1")


def load():
  return load_golden("overturning")


def names(G):
  return [str(c) for c in G["cases"]]


def sections(G, c):
  """{psiarray_z, psiarray_res, psiarray_b, bnew: [nrows][stored levels]} of case c (the fixture
  keeps them interleaved per row and split into byte planes)."""
  nlev = G[c + "_levels"].size
  fields = [str(f) for f in G["section_fields"]]
  a = np.ascontiguousarray(G[c + "_sections"].T).view("<f8").reshape(-1, len(fields), nlev)
  return {f: np.ascontiguousarray(a[:, i]) for i, f in enumerate(fields)}


def case(G, c):
  """Everything of case c: grids, inputs, the reference's rows and its section arrays."""
  nz, ny = int(G[c + "_nz"]), int(G[c + "_ny"])
  out = dict(name=c, nz=nz, ny=ny, z=G["z_%d" % nz], y=G["y_%d" % ny], nb=int(G[c + "_nb"]),
             levels=G[c + "_levels"], ynew=G[c + "_ynew"], b_north=G[c + "_b_north"],
             tau=float(G[c + "_tau"]), kapGM=float(G[c + "_kapGM"]), lengths=G[c + "_lengths"])
  for k in PROFILES:
    out[k] = G[c + "_" + k]
  out.update(sections(G, c))
  out["full"] = out["levels"].size == nz
  return out
