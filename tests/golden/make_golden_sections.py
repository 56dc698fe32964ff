#!/usr/bin/env python3
"""Generate tests/golden/sections.npz (G23) by RUNNING THE REFERENCE's section interpolators.

Run only where the reference checkout is available (read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sections.py

The reference (pymoc 0.0.1rc5, its src/ directory on sys.path as make_golden.py puts it) is
imported, never copied; the fixture holds inputs and the reference's outputs only, and records
the NumPy / SciPy versions (scipy.optimize.brenth is third-party arithmetic under the reference).

G23 sections   pymoc.plotting.Interpolate_channel / Interpolate_twocol:
  - script cases: the G6, G7 (nz = 81, 200) and G9 states through the scripts' own calls, grids
    and fix-ups (example_twocol_plusSO.py:138, Plot_overturning.py:42-67,
    twobasin_NadeauJansen.py:173-196); raw inputs + the fix-up mode, and the fixed-up inputs;
  - the configurations of the reference's (commented-out) plotting tests;
  - float profiles, non-uniform grids, inputs on which brenth raises (sign / NaN), a non-finite
    profile;
  - config-5 sweep members (sweep.npz) on a sub-sampled query grid, with the
    Plot_overturning fix-ups.
Per case: every grid point evaluated on its own (value, or NaN + error code + the exception's
type and message for the first 48 failures), the same for off-grid __call__ points and the special points y == l,
z == z[0], (0, 0); gridit order = row-major, so gridit's exception is the first failing point's.
Error codes: 0 ok, 1 ValueError (sign), 2 RuntimeError (no convergence), 3 ValueError (NaN).
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("PYMOC_REFERENCE_SRC", "/root/reference/src"))

import numpy as np
import scipy

from pymoc.plotting import Interpolate_channel, Interpolate_twocol  # the REFERENCE
from pymoc_amd import configs  # parameter tables only

warnings.simplefilter("ignore")
META = dict(numpy_version=np.__version__, scipy_version=scipy.__version__,
            reference="pymoc 0.0.1rc5")
CLASSES = {"channel": Interpolate_channel, "twocol": Interpolate_twocol}


def code_of(e):
  if isinstance(e, RuntimeError):
    return 2
  if isinstance(e, ValueError):
    return 3 if "is NaN" in str(e) else 1
  raise e


def evaluate(obj, ys, zs):
  """obj(y, z) for every pair: values (NaN where raised), codes, and the failures' text."""
  val = np.full(len(ys), np.nan)
  err = np.zeros(len(ys), np.int8)
  fails = []
  for k, (y, z) in enumerate(zip(ys, zs)):
    try:
      val[k] = obj(y, z)
    except (ValueError, RuntimeError) as e:
      err[k] = code_of(e)
      fails.append((k, type(e).__name__, str(e)))
  return val, err, fails


def fix(kind, mode, bs, bn):
  """The scripts' fix-ups on copies (Plot_overturning.py:42-50, :63-64; twobasin:176)."""
  bs, bn = np.array(bs, dtype=float), np.array(bn, dtype=float)
  if mode == "plot_overturning" and kind == "channel":
    if bs[0] > bs[1]:
      bs[0] = bs[1]
    if bs[0] < bn[0]:
      bn[0] = bs[0]
  elif mode == "plot_overturning":
    bn[0] = bs[0]
  elif mode == "twobasin":
    bs[-1] = 1. * bn[-1]
  return bs, bn


OUT = dict(META)
MAX_FAILS = 48  # exception text kept for the first failing grid points of a case (codes: all)
NAMES = []


def case(name, kind, y, z, bs, bn, fixups="", yq=None, zq=None, calls=()):
  """Record one case; `bs` / `bn` are the RAW inputs (arrays or floats), fix-ups applied here."""
  NAMES.append(name)
  p = "%s_" % name
  OUT[p + "kind"] = kind
  OUT[p + "fixups"] = fixups
  OUT[p + "y"], OUT[p + "z"] = y, z
  for nm, v in (("bs", bs), ("bn", bn)):
    OUT[p + nm] = np.asarray(v, dtype=float)
    OUT[p + nm + "_float"] = isinstance(v, float)
  if fixups:
    fbs, fbn = fix(kind, fixups, bs, bn)
  else:
    fbs, fbn = bs, bn
  OUT[p + "bs_fixed"], OUT[p + "bn_fixed"] = np.asarray(fbs, float), np.asarray(fbn, float)
  obj = CLASSES[kind](y=y, z=z, bs=fbs, bn=fbn)
  yq = y if yq is None else yq
  zq = z if zq is None else zq
  OUT[p + "yq"], OUT[p + "zq"] = yq, zq
  Y, Z = np.meshgrid(yq, zq, indexing="ij")
  val, err, fails = evaluate(obj, Y.ravel(), Z.ravel())
  OUT[p + "grid"] = val.reshape(Y.shape)
  OUT[p + "err"] = err.reshape(Y.shape)
  fails = fails[:MAX_FAILS]
  OUT[p + "fail_idx"] = np.array([f[0] for f in fails], np.int32)
  OUT[p + "fail_type"] = np.array([f[1] for f in fails] or [""])
  OUT[p + "fail_msg"] = np.array([f[2] for f in fails] or [""])
  if calls:
    cy = np.array([c[0] for c in calls], float)
    cz = np.array([c[1] for c in calls], float)
    cval, cerr, cfails = evaluate(obj, cy, cz)
    OUT[p + "cy"], OUT[p + "cz"], OUT[p + "cval"], OUT[p + "cerr"] = cy, cz, cval, cerr
    OUT[p + "cfail_idx"] = np.array([f[0] for f in cfails], np.int32)
    OUT[p + "cfail_type"] = np.array([f[1] for f in cfails] or [""])
    OUT[p + "cfail_msg"] = np.array([f[2] for f in cfails] or [""])
  nfail = int((err != 0).sum())
  print("%-22s %-7s %4d x %4d  failing %d" % (name, kind, len(yq), len(zq), nfail))


def special_calls(y, z, rng, k=12):
  """Off-grid points inside and beyond the grid plus y == l, z == z[0], (0, 0)."""
  l, d = y[-1], z[0]
  pts = [(l, 0.5 * d), (l, d), (0.5 * l, d), (0., 0.), (0., d), (l, 0.), (0.3 * l, 0.)]
  for _ in range(k):
    pts.append((float(rng.uniform(-0.1 * l, 1.1 * l)), float(rng.uniform(1.05 * d, 0.))))
  return pts


def main():
  rng = np.random.default_rng(2323)
  g = lambda n: np.load(os.path.join(HERE, n + ".npz"))

  # G7 (run_JansenNadeau_2018 states) through Plot_overturning.py:38-67
  for nz in (81, 200):
    st = g("jn2018_nz%d" % nz)
    m = configs.jn2018_member(nz=nz)
    y, z = m["y"], m["z"]
    bb, bn, bsso = st["s01200_b_basin"], st["s01200_b_north"], st["s01200_bs_SO"]
    case("g7_nz%d_channel" % nz, "channel", y, z, bsso, bb, "plot_overturning",
         calls=special_calls(y, z, rng))
    lchannel = y[-1] / 1e3
    ynorth = np.linspace(1000. / 10., 1000., 10) + lchannel + 12000.
    case("g7_nz%d_north" % nz, "twocol", ynorth * 1000. - ynorth[0] * 1000., z, bb, bn,
         "plot_overturning", calls=special_calls(ynorth * 1000. - ynorth[0] * 1000., z, rng))
  # G6 (example_twocol_plusSO state) through example_twocol_plusSO.py:138
  st = g("twocol_so")
  m = configs.twocol_so_member()
  case("g6_channel", "channel", m["y"], m["z"], m["bs_SO"], st["s02400_b_basin"],
       calls=special_calls(m["y"], m["z"], rng))
  # G9 (twobasin_NadeauJansen state) through twobasin_NadeauJansen.py:170-196
  st = g("twobasin")
  m = configs.twobasin_member()
  y, z = m["y"], m["z"]
  Atl, Pac = st["s01200_b_Atl"], st["s01200_b_Pac"]
  b_basin = (m["A_Atl"] * Atl + m["A_Pac"] * Pac) / (m["A_Atl"] + m["A_Pac"])
  case("g9_channel", "channel", y, z, m["bs_SO"], b_basin, "twobasin",
       calls=special_calls(y, z, rng))
  ytrans = np.linspace(1500. / 20., 1500., 20) + y[-1] / 1e3 + 11000.
  bn = st["s01200_b_north"].copy()
  bn[0] = b_basin[0]  # :192-193 (the caller's fix-up: it needs the mean basin profile)
  yt = ytrans * 1000. - ytrans[0] * 1000.
  case("g9_trans", "twocol", yt, z, Atl, bn, calls=special_calls(yt, z, rng))

  # the reference's plotting tests (src/pymoc/plotting/tests/*.py): complete configurations
  y51, y81 = np.asarray(np.linspace(0, 2.0e6, 51)), np.asarray(np.linspace(0, 2.0e6, 81))
  z81 = np.asarray(np.linspace(-4.0e3, 0, 81))
  case("reftest_channel_cfg", "channel", y51, z81, np.linspace(0.02, 0.01, 51),
       np.linspace(0.03, -0.01, 81), calls=special_calls(y51, z81, rng))
  case("reftest_channel_fix", "channel", y51, z81, np.linspace(0.02, 0.01, 51),
       np.linspace(0.03, 0.01, 81), calls=special_calls(y51, z81, rng))
  case("reftest_twocol_cfg", "twocol", y81, z81, np.linspace(0.02, 0.01, 81),
       np.linspace(0.03, -0.01, 81), calls=special_calls(y81, z81, rng))
  case("reftest_twocol_fix", "twocol", y81, z81, np.linspace(0.02, -0.01, 81),
       np.linspace(0.03, 0.01, 81), calls=special_calls(y81, z81, rng))
  # the constructor TypeErrors of the same tests (messages)
  errs = []
  for kind, cls in CLASSES.items():
    for kw in ({}, {"z": z81}, {"y": y51}, {"z": z81, "y": 1e6}, {"z": z81, "y": y51},
               {"z": z81, "y": y51, "bs": np.linspace(0.02, 0.01, 51)}):
      try:
        cls(**kw)
        errs.append("")
      except TypeError as e:
        errs.append(str(e))
  OUT["ctor_errors"] = np.array(errs)

  # float profiles
  ys, zs = np.linspace(0., 1.5e6, 7), np.linspace(-3000., 0., 9)
  case("float_bs_channel", "channel", ys, zs, 0.012, 0.02 * np.exp(zs / 800.) - 0.002,
       calls=special_calls(ys, zs, rng, 4))
  case("float_bn_channel", "channel", ys, zs, np.linspace(-0.001, 0.02, 7), 0.004,
       calls=special_calls(ys, zs, rng, 4))
  case("float_both_twocol", "twocol", ys, zs, 0.01, 0.005, calls=special_calls(ys, zs, rng, 4))
  case("float_bn_twocol", "twocol", ys, zs, 0.02 * np.exp(zs / 800.) - 0.001, 0.003,
       calls=special_calls(ys, zs, rng, 4))
  # non-uniform grids
  yn = 2e6 * np.linspace(0., 1., 17) ** 1.7
  zn = -4000. * (1. - np.linspace(0., 1., 23)) ** 1.5
  case("nonuniform_channel", "channel", yn, zn, 0.02 * (yn / yn[-1]) ** 2 - 0.001,
       0.02 * np.exp(zn / 700.) - 0.0015, calls=special_calls(yn, zn, rng))
  case("nonuniform_twocol", "twocol", yn, zn, 0.02 * np.exp(zn / 700.) - 0.0015,
       0.004 * np.exp(zn / 500.) - 0.0015, calls=special_calls(yn, zn, rng))
  # inputs on which brenth raises: made-up profiles (sign errors), a NaN level
  yb, zb = np.linspace(0., 1e6, 20), np.linspace(-4000., 0., 40)
  bsb = 0.01 * np.exp(zb / 600.) + 0.002 * np.sin(zb / 300.)
  bnb = 0.012 * np.exp(zb / 400.) - 0.001
  bnb[0] = bsb[0]
  case("failing_twocol", "twocol", yb, zb, bsb, bnb, calls=special_calls(yb, zb, rng))
  case("failing_channel", "channel", yb, zb, np.linspace(-0.002, 0.015, 20),
       0.01 * np.exp(zb / 600.), calls=special_calls(yb, zb, rng))
  bnan = 0.02 * np.exp(zb / 800.) - 0.002
  bnan[17] = np.nan
  case("nonfinite_channel", "channel", yb, zb, np.linspace(-0.002, 0.015, 20), bnan)
  case("nonfinite_twocol", "twocol", yb, zb, 0.02 * np.exp(zb / 800.) - 0.002, bnan)

  # config-5 sweep members (sweep.npz), Plot_overturning's grids and fix-ups, sub-sampled
  sw = g("sweep")
  m = configs.jn2018_member(nz=200)
  y, z = m["y"], m["z"]
  ynorth = np.linspace(100., 1000., 10) + y[-1] / 1e3 + 12000.
  yt = ynorth * 1000. - ynorth[0] * 1000.
  members = [("c5", j) for j in range(sw["c5_b_basin"].shape[0])] + \
            [("c5_long", j) for j in range(sw["c5_long_b_basin"].shape[0])]
  for tag, j in members:
    bb, bn, bsso = sw[tag + "_b_basin"][j], sw[tag + "_b_north"][j], sw[tag + "_bs_SO"][j]
    if not (np.isfinite(bb).all() and np.isfinite(bn).all() and np.isfinite(bsso).all()):
      continue
    case("sweep_%s_%d_channel" % (tag, j), "channel", y, z, bsso, bb, "plot_overturning",
         yq=y[::5], zq=z[::5])
    case("sweep_%s_%d_north" % (tag, j), "twocol", yt, z, bb, bn, "plot_overturning",
         zq=z[::5])

  OUT["cases"] = np.array(NAMES)
  path = os.path.join(HERE, "sections.npz")
  np.savez_compressed(path, **OUT)
  print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
  main()
