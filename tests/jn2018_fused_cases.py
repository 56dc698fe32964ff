"""The fused Jansen & Nadeau loop with explicit columns (pm_jn2018_steps): the row table of its
tests, the restatement of one launch through the oracle, the trace of what every member does in
every step, and a restatement of the two dispatch sites.

Members are the CONSTRUCTED ones of jn2018_implicit_cases.make_case (wA, Psi_SO, Psi_res_b and
Psi_res_n chosen, not solved for) at r = max(kappa) dt / dz^2 = 0.3, where forward Euler is
stable.  The restatement is exact arithmetic in the reference's operation order: the switch
(jn2018_implicit_cases.bc_switch), oracle.column_timestep(do_conv=True) per column and
oracle.so_ml_advdiff.  The kernels promise its bits, so no tolerance appears anywhere.

A row's `kernel` names where pm_jn2018_steps sends it; `dispatch` below restates the two sites
(pymoc_hip.hip: pm_jn2018_steps, jn2018_fast.hip: jn2018_fast_applies / launch_fast) and
test_jn2018_fused_cpu.py holds every row against it.
"""
import numpy as np

import jn2018_implicit_cases as J

STEP_COUNTS = J.STEP_COUNTS          # snapshots after 1, 2, 7 and 36 steps
LAUNCHES = (1, 1, 5, 29)             # (b): launches continuing from each other, ending at the snapshots
R = 0.3
UA, CONTRACTED, SHARED, SPLIT, DIV3 = 1, 2, 4, 8, 16   # PM_JN_* (include/pymoc_hip.h)
JF_WAVES = 16                        # members (waves) per block of the uniform-Area kernels
PSI_S0 = 3.5                         # Psi_s before a launch: shows where a launch never writes it


def in_window(a):
  """The operand window of the kernels' 4-instruction division: 0 or 2^-200 <= |a| <= 2^200."""
  a = np.abs(np.asarray(a, dtype=np.float64))
  return (a == 0) | ((a >= 2.0 ** -200) & (a <= 2.0 ** 200))


def dispatch(nz, ny, hints, b_aligned16, status_given):
  """The kernel pm_jn2018_steps launches, as "fast P=2 vec", "split PS=3 novec" or "general P=4".
  vec: the 16-byte row accessors (every row 16-byte aligned and a whole number of P-level groups;
  every array but cols.b is a device allocation of its own, so only b's address can refuse)."""
  fast = bool(hints & UA) and ny <= 64 and 4 <= nz <= 256 and status_given
  if not fast:
    return "general P=%d" % ((nz + 63) // 64)
  P, PS = (2 if nz <= 128 else 4), (nz + 31) // 32
  if hints & SPLIT and PS in (3, 4, 7):
    return "split PS=%d %s" % (PS, "vec" if nz % 2 == 0 and b_aligned16 else "novec")
  return "fast P=%d %s" % (P, "vec" if nz % P == 0 and b_aligned16 else "novec")


def family(kernel):
  return kernel.split()[0]


# name, nz, ny, n, kernel, options.  Options: make_case keywords, and
#   hints      PM_JN_* the row's launches carry (default PM_JN_UNIFORM_AREA); PM_JN_DIV3_PROVEN is
#              added by the GPU test where the host proof holds, PM_JN_SHARED_COEF is run on and off
#   status     False: ml.status = NULL
#   b_off8     cols.b 8 bytes off a 16-byte boundary
#   zero_psi   member whose Psi_SO row is all zero
#   tiny       members whose basin state is scaled by 2^-1000 (flagged at step 0 of every launch)
#   sequence   also held against the launch sequence, step by step
#   unsorted   member whose basin profile is inverted on purpose (no oracle comparison)
ROWS = [
    # ---- uniform-Area kernel, P = 2 levels per lane (4 <= nz <= 128); odd nz: 8-byte row accessors
    ("f4", 4, 51, 5, "fast P=2 vec", {}),
    ("f5", 5, 51, 5, "fast P=2 novec", {}),
    ("f63", 63, 63, 1, "fast P=2 novec", dict(kind0=2)),
    ("f64", 64, 64, 5, "fast P=2 vec", dict(sequence=True)),
    ("f65", 65, 51, 1, "fast P=2 novec", dict(kind0=1)),
    ("f127", 127, 3, 3, "fast P=2 novec", dict(kind0=1)),  # ny = 3: the smallest check_so_ml takes
    ("f128", 128, 51, 17, "fast P=2 vec", {}),          # n = 17: a block with 15 idle waves
    # ---- P = 4 (129 <= nz <= 256); nz = 130 is even, but nz % 4 != 0: no 16-byte accessors
    ("f129", 129, 51, 1, "fast P=4 novec", dict(kind0=3)),
    ("f130", 130, 63, 5, "fast P=4 novec", {}),
    ("f200", 200, 51, 5, "fast P=4 vec", {}),
    ("f255", 255, 51, 1, "fast P=4 novec", dict(kind0=4)),
    ("f256", 256, 64, 17, "fast P=4 vec", {}),
    # ---- 16-byte accessors refused by the address of cols.b alone
    ("f64_off8", 64, 51, 5, "fast P=2 novec", dict(b_off8=True)),
    ("f200_off8", 200, 51, 5, "fast P=4 novec", dict(b_off8=True)),
    # ---- PM_JN_SPLIT_LANES: both ends of PS = 3, 4 and 7
    ("s65", 65, 51, 5, "split PS=3 novec", dict(hints=UA | SPLIT)),
    ("s96", 96, 64, 5, "split PS=3 vec", dict(hints=UA | SPLIT, sequence=True)),
    ("s97", 97, 51, 1, "split PS=4 novec", dict(hints=UA | SPLIT, kind0=1)),
    ("s128", 128, 63, 17, "split PS=4 vec", dict(hints=UA | SPLIT)),
    ("s193", 193, 51, 5, "split PS=7 novec", dict(hints=UA | SPLIT)),
    ("s224", 224, 51, 5, "split PS=7 vec", dict(hints=UA | SPLIT)),
    ("s96_off8", 96, 51, 5, "split PS=3 novec", dict(hints=UA | SPLIT, b_off8=True)),
    # ---- the hint is ignored at PS = 2, 5, 6 and 8
    ("i64", 64, 51, 5, "fast P=2 vec", dict(hints=UA | SPLIT)),
    ("i129", 129, 51, 5, "fast P=4 novec", dict(hints=UA | SPLIT)),
    ("i192", 192, 51, 5, "fast P=4 vec", dict(hints=UA | SPLIT)),
    ("i225", 225, 51, 5, "fast P=4 novec", dict(hints=UA | SPLIT)),
    # ---- k_jn2018_steps<1...4>: each condition that refuses the uniform-Area kernel on its own
    ("g2", 2, 51, 5, "general P=1", {}),                                  # nz < 4
    ("g3", 3, 51, 5, "general P=1", {}),
    ("g64_ny65", 64, 65, 5, "general P=1", dict(sequence=True)),          # ny > 64
    ("g65_ny65", 65, 65, 5, "general P=2", {}),
    ("g129_ny65", 129, 65, 5, "general P=3", {}),
    ("g200_ny65", 200, 65, 5, "general P=4", {}),
    ("g200_area", 200, 51, 5, "general P=4", dict(hints=0, area="varying")),  # Area varies in z
    ("g64_nostatus", 64, 51, 5, "general P=1", dict(status=False)),       # ml.status = NULL
    ("g200_nostatus", 200, 64, 5, "general P=4", dict(status=False)),
    # ---- PM_JN_SHARED_COEF (run with the hint and without)
    ("sh64", 64, 51, 5, "fast P=2 vec", dict(shared=True)),
    ("sh200", 200, 51, 5, "fast P=4 vec", dict(shared=True)),
    ("sh96", 96, 51, 5, "split PS=3 vec", dict(shared=True, hints=UA | SPLIT)),
    # ---- Psi_SO all zero: status 1, the mixed layer frozen, the columns stepping
    ("z64", 64, 51, 5, "fast P=2 vec", dict(zero_psi=2)),
    ("z200", 200, 51, 5, "fast P=4 vec", dict(zero_psi=3)),
    ("z65_ny65", 65, 65, 5, "general P=2", dict(zero_psi=1)),
    # ---- H1: flagged members in both ballot groups of FlagScan::take and in three blocks of the
    # IEEE follow-up launch
    # IEEE follow-up launch.  (kind0 = 2 makes them kinds 2, 0, 1, 1: the bottom value the switch
    # imposes on their tiny basin is negative or the basin's own, so the profile stays sorted)
    ("h1", 64, 51, 130, "fast P=2 vec", dict(tiny=(0, 63, 64, 129), kind0=2, sequence=True)),
    # ---- H2: member 1 (kind 1) starts on set 0; one entry of its kappaeff row is 2^-300, and its
    # basin column selects that set in step index 2: stopped there, finished by the IEEE launch
    ("h2_p2", 64, 51, 5, "fast P=2 vec", dict(h2=1, sequence=True)),
    ("h2_p4", 200, 51, 5, "fast P=4 vec", dict(h2=1, sequence=True)),
    ("h2_split", 96, 51, 5, "split PS=3 vec", dict(h2=1, hints=UA | SPLIT, sequence=True)),
    # ---- the imposed bottom value inverts levels 0 and 1 of member 0's basin
    ("u64", 64, 51, 5, "fast P=2 vec", dict(unsorted=0, sequence=True)),
]
ROW_NAMES = [r[0] for r in ROWS]
H2_STEP = 2           # the step index at which an H2 member's basin column selects set 1
H2_NSTEPS = (2, 3, 36)  # not reached (bit 5 clear), reached in the last step, reached early
_OWN = ("hints", "status", "b_off8", "zero_psi", "tiny", "sequence", "unsorted", "h2")
_rows, _cases, _runs = {r[0]: r for r in ROWS}, {}, {}


def row(name):
  """dict(name, nz, ny, n, kernel, hints, status, b_off8, zero_psi, tiny, sequence, unsorted, h2)"""
  _, nz, ny, n, kernel, opt = _rows[name]
  d = dict(name=name, nz=nz, ny=ny, n=n, kernel=kernel, hints=UA, status=True, b_off8=False,
           zero_psi=None, tiny=(), sequence=False, unsorted=None, h2=None, shared=False)
  d.update({k: v for k, v in opt.items() if k in _OWN or k == "shared"})
  return d


def get_case(name):
  if name not in _cases:
    _, nz, ny, n, _, opt = _rows[name]
    kw = {k: v for k, v in opt.items() if k not in _OWN}
    r = row(name)
    if r["zero_psi"] is not None:
      kw["Psi_SO_rows"] = {r["zero_psi"]: np.zeros(nz)}
    if r["h2"] is not None:
      m = r["h2"]
      kw["ksel0"] = {m: 0, n + m: 0}  # (the northern column too: a launch tests the sets it loads)
      kw["kappaeff_entries"] = {(m, nz // 2): 2.0 ** -300}
    if r["unsorted"] is not None:
      kw["bs_SO0_south"] = {r["unsorted"]: 0.002}  # above the basin's level 1 (0.0015) of a kind-0 member
    c = J.make_case(name, nz, ny, n, r=R, **kw)
    for m in r["tiny"]:
      c["b0"][m] *= 2.0 ** -1000
      c["bbot0"][m] = c["b0"][m, 0]
    c["Psi_s0"] = np.full((n, ny), PSI_S0)
    _cases[name] = c
  return _cases[name]


def restatement(case, snapshots=STEP_COUNTS):
  """One launch on the host.  Returns ({nsteps: dict(b, bs_SO, Psi_s, bbot, ksel, nonfinite,
  status)}, trace); trace[step] holds, per member or per column:
    branches  (basin, north) outcome of the switch        margin  its distance from a tie / max|b|
    ksel      [2n] coefficient sets after the switch       conv    [2n, nz] levels that convect
    argmin    [n] argmin(bs_SO)                            sorted  [n] basin profile non-decreasing
    interval  [n, ny] interval of the basin profile a mixed-layer point falls into
    below     [n, ny] point below the first node           above   [n, ny] at or above the last
    upwell    [n] point 1 upwells                          stepped [n] the mixed layer stepped"""
  import oracle as O
  n, nz, ny = case["n"], case["nz"], case["ny"]
  z, dt = case["z"], case["dt"]
  sets = [np.concatenate([case["kappa"]] * 2), np.concatenate([case["kappaeff"]] * 2)]
  b, bsSO = case["b0"].copy(), case["bs_SO0"].copy()
  Psi_s = case["Psi_s0"].copy()
  bbot, ksel = case["bbot0"].copy(), case["ksel0"].copy()
  status = np.zeros(n, dtype=np.int32)
  out, trace, done = {}, [], 0
  for target in sorted(snapshots):
    for _ in range(target - done):
      scale = float(np.max(np.abs(b)))
      branches, margin = [], np.zeros(n)
      for m in range(n):
        st = [bbot[m], ksel[m], bbot[n + m], ksel[n + m]]
        bas, nor, mg = J.bc_switch(case["Psi_SO"][m, 1], case["Psi_res_b"][m, 1],
                                   case["Psi_res_n"][m, 1], b[m, 0], b[m, 1], b[n + m, 0],
                                   b[n + m, 1], bsSO[m, 0], st)
        bbot[m], ksel[m], bbot[n + m], ksel[n + m] = st
        branches.append((bas, nor))
        margin[m] = mg / scale
      conv = b > case["bs"][:, None]
      for c in range(2 * n):
        b[c] = O.column_timestep(z, sets[ksel[c]][c], case["area"][c], b[c], case["wA"][c], dt,
                                 do_conv=True, bs=case["bs"][c], bbot=bbot[c], N2min=case["N2min"][c])
      t = dict(branches=branches, margin=margin, ksel=ksel.copy(), conv=conv,
               argmin=np.argmin(bsSO, axis=1), sorted=(np.diff(b[:n], axis=1) >= 0).all(axis=1),
               interval=np.stack([np.searchsorted(b[m], bsSO[m], side="right") - 1 for m in range(n)]),
               below=bsSO < b[:n, :1], above=bsSO >= b[:n, -1:],
               upwell=np.zeros(n, dtype=bool), stepped=np.zeros(n, dtype=bool))
      for m in range(n):
        try:
          bsSO[m], Psi_s[m] = O.so_ml_advdiff(case["y"], case["surflux"][m], case["rest_mask"][m],
                                              case["b_rest"][m], bsSO[m], b[m], case["Psi_SO"][m],
                                              dt, Ks=case["Ks"], h=case["h"], L=case["L"],
                                              v_pist=case["v_pist"])
          status[m] = 0 if np.isfinite(bsSO[m]).all() else 2
          t["stepped"][m], t["upwell"][m] = True, Psi_s[m, 1] > 0
        except IndexError:  # the header: status 1, bs and Psi_s left alone
          status[m] = 1
      trace.append(t)
    done = target
    bad = ~(np.isfinite(b[:n]).all(axis=1) & np.isfinite(b[n:]).all(axis=1) & np.isfinite(bsSO).all(axis=1))
    out[target] = dict(b=b.copy(), bs_SO=bsSO.copy(), Psi_s=Psi_s.copy(), bbot=bbot.copy(),
                       ksel=ksel.copy(), nonfinite=np.concatenate([bad, bad]).astype(np.int32),
                       status=status | np.where(bad, 2, 0).astype(np.int32))
  return out, trace


def run(name):
  """restatement(get_case(name)) at STEP_COUNTS; computed once and shared."""
  if name not in _runs:
    _runs[name] = restatement(get_case(name))
  return _runs[name]


def sets_outside_window(case):
  """[2 sets, 2n columns]: the set holds an operand outside the exact-division window (kappa, or
  weff = wA - dAkappa at an interior level, as the kernel's load tests them)."""
  area = case["area"]
  bad = []
  for k in (case["kappa"], case["kappaeff"]):
    k2 = np.concatenate([k, k])
    dAk = np.gradient(area * k2, case["z"], axis=-1)
    weff = (case["wA"] - dAk)[:, 1:-1]
    bad.append(~(in_window(k2).all(axis=1) & in_window(weff).all(axis=1)))
  return np.stack(bad)


def flagged(name, first, nsteps):
  """[n] members a launch of steps [first, first + nsteps) hands to its IEEE follow-up launch
  (status bit 5): those whose state lies outside the window (the `tiny` members, from step 0 of
  every launch) and those one of whose columns loads a coefficient set outside it -- the set the
  launch starts with (ksel as carried in) or one a switch of these steps selects."""
  case, (_, trace) = get_case(name), run(name)
  n = case["n"]
  bad = sets_outside_window(case)
  used = [case["ksel0"] if first == 0 else trace[first - 1]["ksel"]]
  used += [trace[s]["ksel"] for s in range(first, first + nsteps)]
  cols = np.arange(2 * n)
  hit = np.zeros(2 * n, dtype=bool)
  for k in used:
    hit |= bad[k, cols]
  f = hit[:n] | hit[n:]
  f[list(row(name)["tiny"])] = True
  return f
