"""The fused Jansen & Nadeau loop with implicit columns (pm_jn2018_steps_implicit): the case table
of its tests, a host restatement of one launch and the measured error of the restatement itself.

A launch is nsteps x [bottom-BC switch, both columns by backward Euler, mixed layer] with wA,
Psi_SO, Psi_res_b and Psi_res_n held fixed (include/pymoc_hip.h).  The members here are
CONSTRUCTED: those four arrays are chosen, not solved for, so that between them the members take
every branch of the switch (run_JansenNadeau_2018.py:233-254) and some change a column's
coefficient set in a later step of a launch:

  kind 0  bottom water from the south (Psi_SO[1] < 0), none from the north (Psi_res_b[1] <= 0);
          the northern column takes inflow from the basin only once the basin's bottom has
          taken the mixed layer's value: its coefficient set changes in steps 1 AND 2
  kind 1  no bottom water at first (Psi_SO[1] >= 0, northern bottom lighter than the basin's);
          the northern column convects, its bottom value decays step by step and crosses the
          basin's: the BASIN's coefficient set changes in step 1 and again a few steps later
  kind 2  bottom water from the north and inflow into the northern column from the first step
  kind 3  south and north at once (the north wins), no inflow
  kind 4  south, the northern condition open (Psi_res_b[1] > 0) but not met, no inflow

The restatement: the switch as in oracle/drivers.py:95-104, the columns through
implicit_column_cases.Factored / convect in `dtype`, the mixed layer through
oracle.so_ml_advdiff.  The switch and the mixed layer always work in float64 on the rounded
profiles; only the column solve changes precision.
"""
import numpy as np

import implicit_column_cases as I

DAY = 86400.0
STEP_COUNTS = (1, 2, 7, 36)
KINDS = 5

# max over the case table and its step counts of max|b64 - b_longdouble| / max|b| over both columns,
# measured with measure_coupled_error() on the CPU (x86-64, 80-bit long double).
# test_jn2018_implicit_cpu re-measures it and requires  fresh <= E_COUPLED <= 2 * fresh.
E_COUPLED = 1.8e-14
GPU_TOL_FACTOR = I.GPU_TOL_FACTOR  # DESIGN.md section 13's argument: up to 8 elimination levels
# the comparisons of the switch stay this far (x max|b|) from a tie in every step of every case
TIE_MARGIN = 1e-6


def make_case(name, nz, ny, n, r=0.77, area="const", kind0=0, dt_days=30.0, shared=False,
              ksel0=None, kappaeff_entries=None, Psi_SO_rows=None, bs_SO0_south=None):
  """n members of kinds kind0, kind0 + 1, ... (mod KINDS).  r = max(kappa) dt / dz^2.
  shared: every member gets member 0's kappa, kappaeff and Area rows (PM_JN_SHARED_COEF).
  Per-member overrides, each a dict: ksel0 {column: set}, kappaeff_entries {(member, level):
  value}, Psi_SO_rows {member: row [nz]} (wA follows), bs_SO0_south {member: bs_SO0[member, 0]}."""
  H = 4000.0
  z = np.linspace(-H, 0.0, nz)
  y = np.linspace(0.0, 2.0e6, ny)
  dt = dt_days * DAY
  dz = z[1] - z[0]
  kinds = (kind0 + np.arange(n)) % KINDS
  m = np.arange(n)
  mc = np.zeros(n, dtype=m.dtype) if shared else m  # whose coefficients a member takes
  shape = 1.0 + 2.0 * np.exp(z / 800.0)                        # max 3 at the surface
  kbase = r * dz * dz / (3.0 * dt) * (1.0 - 0.05 * (mc % 3))  # max over members: r exactly-ish
  kap = kbase[:, None] * shape[None, :]
  taper = 0.2 + 0.8 * np.minimum(1.0, (z + H) / 1200.0)        # bottom boundary layer
  kapeff = kap * taper[None, :]
  for (mm, lev), v in (kappaeff_entries or {}).items():
    kapeff[mm, lev] = v
  A_b = 8e13 * (1.0 + 0.1 * (mc % 2))
  A_n = A_b / 50.0
  if area == "const":
    prof = np.ones(nz)
  else:
    prof = 0.3 + 0.7 * (1.0 + z / H) ** 2
  area_rows = np.concatenate([A_b[:, None] * prof[None, :], A_n[:, None] * prof[None, :]])
  bs = 0.02 + 1e-4 * m
  bs_north = -0.001 + 2e-5 * m

  south = np.isin(kinds, (0, 3, 4))
  sinp = np.sin(np.pi * (z + H) / H)
  Psi_SO = 2.0 * sinp[None, :] * (1.0 + 0.1 * m[:, None])
  Psi_SO[:, 0] = 0.0
  Psi_SO[:, 1] = np.where(south, -0.4, 0.5)
  for mm, row in (Psi_SO_rows or {}).items():
    Psi_SO[mm] = row
  Pb = 1.5 * sinp[None, :] * np.ones((n, 1))
  Pb[:, 1] = np.where(np.isin(kinds, (1, 2, 3, 4)), 0.3, -0.2)
  Pn = 1.0 * sinp[None, :] * np.ones((n, 1))
  Pn[:, 1] = np.where(np.isin(kinds, (0, 2)), -0.3, 0.2)
  wA = np.concatenate([(Pb - Psi_SO) * 1e6, -Pn * 1e6])

  # basin: stably stratified below bs, the two bottom levels set per kind
  b_basin = bs[:, None] * np.exp(z[None, :] / 300.0) + 0.004 * (1.0 + z[None, :] / H)
  b_basin[:, -1] = bs
  bb0 = np.choose(kinds, [0.001, 0.0025, -0.002, 0.001, 0.0005])
  bb1 = np.choose(kinds, [0.0015, 0.003, 0.001, 0.002, 0.001])
  b_basin[:, 0], b_basin[:, 1] = bb0, bb1
  b_basin[:, 2:] = np.maximum(b_basin[:, 2:], bb1[:, None] + 1e-4 * (1.0 + np.arange(nz - 2))[None, :] / nz)
  b_basin[:, -1] = bs
  # north: kinds 0, 2, 3: the script's cold profile; 1: light everywhere (convects to the
  # bottom, the bottom value decays from 0.01); 4: bottom lighter than the basin's level 1
  b_north = bs_north[:, None] * (z[None, :] / z[0]) ** 2
  b_north[kinds == 1] = 0.01
  b_north[kinds == 4] = 0.0015 * (z[None, :] / z[0]) ** 2 + 0.0005
  b0 = np.concatenate([b_basin, b_north])

  # mixed layer of run_JansenNadeau_2018.py, its southern end at a value chosen per kind
  bs0 = np.choose(kinds, [-0.002, 0.002, 0.0015, 0.0005, 0.0002])
  b_rest = np.repeat(bs0[:, None], ny, axis=1)
  j6 = min(6, ny - 2)
  alpha = 1.0 - np.cos(np.pi * (y[-1] - y[j6 - 1]) / 7.4e6)
  b_rest[:, j6:] = ((bs - bs0)[:, None] * (1.0 - np.cos(np.pi * (y[j6:] - y[j6 - 1]) / 7.4e6))[None, :]
                    / alpha + bs0[:, None])
  bs_SO = b_rest.copy()
  bs_SO[:, -1] = bs
  for mm, v in (bs_SO0_south or {}).items():
    bs_SO[mm, 0] = v
  surflux = np.zeros((n, ny))
  surflux[:, 1:j6] = -(5.9e3 / 4e6 / 2e5) * (1.0 + 0.2 * m[:, None])
  rest_mask = np.zeros((n, ny))
  rest_mask[:, j6:-1] = 1.0
  sel0 = np.ones(2 * n, dtype=np.int32)
  for col, v in (ksel0 or {}).items():
    sel0[col] = v
  return dict(name=name, nz=nz, ny=ny, n=n, z=z, y=y, dt=dt, r=r, kinds=kinds, kappa=kap,
              kappaeff=kapeff, area=area_rows, b0=b0, bs=np.concatenate([bs, bs_north]),
              N2min=np.full(2 * n, 1e-7), Psi_SO=Psi_SO, Psi_res_b=Pb, Psi_res_n=Pn, wA=wA,
              bs_SO0=bs_SO, surflux=surflux, rest_mask=rest_mask, b_rest=b_rest, Ks=400.0, h=50.0,
              L=4e6, v_pist=1.5 / DAY, bbot0=b0[:, 0].copy(), ksel0=sel0)


# name, nz, ny, n, keywords.  nz: both sides of every levels-per-lane boundary (64 | 65, 128 | 129,
# 192 | 200, 256), the last level in lane 63 (63: P = 1, 256: P = 4), a column of 5 levels; ny: the
# register / LDS boundary of the mixed layer (64 | 65) and the script's 51; n = 5 is no multiple of
# the 4 waves of a block; one case with Area varying in z.
CASE_SPECS = [
    ("nz5", 5, 51, 5, dict(r=3.0)),
    ("nz63", 63, 64, 1, dict(r=30.0, kind0=0)),
    ("nz64", 64, 65, 5, dict(r=0.77)),
    ("nz65", 65, 51, 1, dict(r=3.0, kind0=1)),
    ("nz129", 129, 65, 1, dict(r=100.0, kind0=0)),
    ("nz200", 200, 51, 5, dict(r=0.77)),
    ("nz200_area", 200, 64, 5, dict(r=3.0, area="varying", kind0=2)),
    ("nz256", 256, 65, 5, dict(r=30.0, kind0=1)),
    ("nz256_one", 256, 51, 1, dict(r=0.77, kind0=1)),
]
CASE_NAMES = [s[0] for s in CASE_SPECS]
_cases, _runs = {}, {}


def get_case(name):
  if name not in _cases:
    for n_, nz, ny, n, kw in CASE_SPECS:
      if n_ == name:
        _cases[name] = make_case(n_, nz, ny, n, **kw)
  return _cases[name]


def bc_switch(PsiSO1, Pb1, Pn1, bb0, bb1, bn0, bn1, bs0, st):
  """One member's switch (oracle/drivers.py:95-104).  st = [bbot_b, ksel_b, bbot_n, ksel_n] is
  updated; returns (branch of the basin column, branch of the northern column, the distance of
  the data-dependent comparisons from a tie)."""
  basin, margin = "kept", np.inf
  if PsiSO1 < 0:
    st[0], st[1], basin = bs0, 1, "south"
  if Pb1 > 0:
    margin = min(margin, abs(bn0 - bb1), abs(bn0 - bs0))
  if Pb1 > 0 and bn0 < bb1 and bn0 < bs0:
    st[0], st[1], basin = bn0, 1, "north"
  elif PsiSO1 >= 0:
    st[0], st[1], basin = bb1, 0, "none"
  if Pn1 < 0:
    margin = min(margin, abs(bb0 - bn1))
  if Pn1 < 0 and bb0 < bn1:
    st[2], st[3], north = bb0, 1, "inflow"
  else:
    st[2], st[3], north = bn1, 0, "no inflow"
  return basin, north, margin


def restatement(case, nsteps_list=STEP_COUNTS, dtype=np.float64):
  """One launch on the host.  Returns {nsteps: dict(b, bs_SO, Psi_s, bbot, ksel)} snapshots and a
  trace: per step the branches of every member, the columns' coefficient sets after the switch,
  the convecting sets, and the smallest tie margin (relative to max|b|)."""
  import oracle as O
  n, nz = case["n"], case["nz"]
  z = I._f(case["z"], dtype)
  cols = np.arange(2 * n)
  kap_sets = np.stack([np.concatenate([case["kappa"]] * 2), np.concatenate([case["kappaeff"]] * 2)])
  dAk_sets = np.stack([np.gradient(case["area"] * k, case["z"], axis=-1) for k in kap_sets])
  area = I._f(case["area"], dtype)
  dt = dtype(case["dt"])
  bs, N2min = I._f(case["bs"], dtype), I._f(case["N2min"], dtype)
  no = np.zeros(2 * n, dtype=bool)
  yes = np.ones(2 * n, dtype=bool)
  b = I._f(case["b0"], dtype).copy()
  bsSO = case["bs_SO0"].copy()
  Psi_s = np.zeros_like(bsSO)
  bbot, ksel = case["bbot0"].copy(), case["ksel0"].copy()
  F, F_sel = None, None
  out, trace, done = {}, [], 0
  for target in sorted(nsteps_list):
    for _ in range(target - done):
      b64 = b.astype(np.float64)
      scale = float(np.max(np.abs(b64)))
      branches, margin = [], np.inf
      for m in range(n):
        st = [bbot[m], ksel[m], bbot[n + m], ksel[n + m]]
        bas, nor, mg = bc_switch(case["Psi_SO"][m, 1], case["Psi_res_b"][m, 1],
                                 case["Psi_res_n"][m, 1], b64[m, 0], b64[m, 1], b64[n + m, 0],
                                 b64[n + m, 1], bsSO[m, 0], st)
        bbot[m], ksel[m], bbot[n + m], ksel[n + m] = st
        branches.append((bas, nor))
        margin = min(margin, mg / scale)
      if F is None or not np.array_equal(F_sel, ksel):
        weff = I._f(case["wA"], dtype) - I._f(dAk_sets[ksel, cols], dtype)
        F = I.Factored(z, I._f(kap_sets[ksel, cols], dtype), area, weff, dt, no, I._f(no, dtype),
                       dtype)
        F_sel = ksel.copy()
      conv = b > bs[:, None]
      I.convect(b, z, bs, N2min, yes)
      b[:, 0] = I._f(bbot, dtype)
      rhs = b[:, 1:-1].copy()
      rhs[:, 0] = rhs[:, 0] - F.a[:, 0] * b[:, 0]
      rhs[:, -1] = rhs[:, -1] - F.c[:, -1] * b[:, -1]
      b[:, 1:-1] = F.solve(rhs)
      b64 = b.astype(np.float64)
      for m in range(n):
        bsSO[m], Psi_s[m] = O.so_ml_advdiff(case["y"], case["surflux"][m], case["rest_mask"][m],
                                            case["b_rest"][m], bsSO[m], b64[m], case["Psi_SO"][m],
                                            case["dt"], Ks=case["Ks"], h=case["h"], L=case["L"],
                                            v_pist=case["v_pist"])
      trace.append(dict(branches=branches, ksel=ksel.copy(), conv=conv, margin=margin))
    done = target
    out[target] = dict(b=b.copy(), bs_SO=bsSO.copy(), Psi_s=Psi_s.copy(), bbot=bbot.copy(),
                       ksel=ksel.copy())
  return out, trace


def run(name, dtype=np.float64):
  """restatement(get_case(name)) at STEP_COUNTS; computed once and shared."""
  key = (name, np.dtype(dtype).name)
  if key not in _runs:
    _runs[key] = restatement(get_case(name), STEP_COUNTS, dtype)
  return _runs[key]


def switches_after_step_1(name):
  """(members whose basin column, members whose northern column) changes its coefficient set in
  a step after the first."""
  _, trace = run(name)
  n = get_case(name)["n"]
  k = np.stack([t["ksel"] for t in trace])
  ch = (k[1:] != k[:-1]).any(axis=0)
  return np.nonzero(ch[:n])[0], np.nonzero(ch[n:])[0]


def switching_cases():
  return [c for c in CASE_NAMES if any(len(s) for s in switches_after_step_1(c))]


def measure_coupled_error():
  """{(case, nsteps): max|b64 - b_longdouble| / max|b|} over the case table."""
  out = {}
  for name in CASE_NAMES:
    r64, rld = run(name)[0], run(name, np.longdouble)[0]
    for k in r64:
      scale = float(np.max(np.abs(rld[k]["b"])))
      out[(name, k)] = float(np.max(np.abs(r64[k]["b"].astype(np.longdouble) - rld[k]["b"]))) / scale
  return out
