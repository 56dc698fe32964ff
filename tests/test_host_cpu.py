"""CPU-only checks: the C-ABI library loads and exports every symbol the header
declares, host-side coercion and error text match the reference's contract, config
generators are shard-invariant.  No compute call is made (there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header_symbols():
  text = open(os.path.join(ROOT, "include", "pymoc_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
  from pymoc_amd import _lib
  names = _header_symbols()
  assert len(names) >= 20
  for n in names:
    assert hasattr(_lib.lib, n), "libpymoc_hip.so does not export %s" % n
    assert n in _lib.SIGNATURES, "no ctypes signature for %s" % n
  assert set(_lib.SIGNATURES) == set(names)
  assert b"gfx950" in _lib.lib.pm_version()


def test_struct_layout_matches_header(tmp_path):
  """sizeof of every struct of include/pymoc_hip.h as gcc sees it against its ctypes mirror."""
  import subprocess
  from conftest import ROOT
  from pymoc_amd import _lib
  names = ["pm_columns", "pm_thermwind", "pm_psi_so", "pm_so_ml", "pm_jn2018_bc", "pm_jn2018",
           "pm_run_schedule", "pm_twocol_loop", "pm_jn2018_loop", "pm_column_equi",
           "pm_equi_column"]
  src = tmp_path / "sizes.c"
  src.write_text('#include <stdio.h>\n#include "pymoc_hip.h"\nint main(void) {\n' +
                 "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                 "  return 0;\n}\n")
  exe = tmp_path / "sizes"
  subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
  out = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
  for n in names:
    assert ctypes.sizeof(getattr(_lib, n)) == int(out[n]), n
  assert ctypes.sizeof(_lib.pm_columns) == 16 + 14 * 8  # 4 int32 + 14 pointers


def test_no_device_fails_loudly():
  from pymoc_amd import _lib
  n = ctypes.c_int(-1)
  rc = _lib.lib.pm_device_count(ctypes.byref(n))
  if rc == 0 and n.value > 0:
    pytest.skip("a GPU is visible here")
  with pytest.raises(_lib.PmError):
    _lib.require_device()
  import pymoc_amd
  col = pymoc_amd.Column(z=np.linspace(-4000., 0., 10), kappa=1e-5, Area=1e14, b=0.01)
  with pytest.raises(_lib.PmError):
    col.timestep(wA=0., dt=1.)


def test_cabi_rejects_bad_arguments_before_touching_the_device():
  """Every compute entry validates shapes / pointers first and reports through
  pm_last_error; none of these calls reaches a launch, so they run without a GPU."""
  from pymoc_amd import _lib
  L, C = _lib.lib, ctypes

  def err():
    return L.pm_last_error().decode()

  c = _lib.pm_columns()
  c.ncols, c.nz, c.nsel = 4, 1, 1
  assert L.pm_column_steps(C.byref(c), None, None, None, 1., 1, 7, 0, None) == _lib.PM_EINVAL
  assert "nz" in err()
  c.nz = 10
  assert L.pm_column_steps(C.byref(c), None, None, None, 1., 1, 7, 0, None) == _lib.PM_EINVAL
  assert "NULL" in err()
  assert L.pm_column_steps(None, None, None, None, 1., 1, 7, 0, None) == _lib.PM_EINVAL
  c.ncols = 0  # an empty batch is fine, pointers may be NULL
  assert L.pm_column_steps(C.byref(c), None, None, None, 1., 1, 7, 0, None) == _lib.PM_OK
  t = _lib.pm_thermwind()
  t.n, t.nz, t.nb = 2, 1, 10
  assert L.pm_thermwind_update(C.byref(t), 1, None) == _lib.PM_EINVAL
  so = _lib.pm_psi_so()
  so.n, so.nz, so.ny = 2, 1, 10
  assert L.pm_psi_so_update(C.byref(so), 1, None) == _lib.PM_EINVAL
  ml = _lib.pm_so_ml()
  ml.n, ml.nz, ml.ny = 2, 10, 2
  assert L.pm_so_ml_step(C.byref(ml), 1., None) == _lib.PM_EINVAL
  eq = _lib.pm_column_equi()
  eq.n, eq.nz, eq.mmax, eq.tol = 2, 10, 2000, 1e-3
  assert L.pm_column_equi_pass(C.byref(eq), None) == _lib.PM_EINVAL
  assert "mmax" in err()
  ec = _lib.pm_equi_column()
  ec.n, ec.mmax, ec.tol = 2, 64, 1e-3
  assert L.pm_equi_column_newton(C.byref(ec), None) == _lib.PM_EINVAL
  assert "NULL" in err()
  assert L.pm_axpby(4, 1., None, 1., None, None, None) == _lib.PM_EINVAL
  assert L.pm_equi_column_scratch_doubles(64) >= 64 * 100


def test_cabi_rejects_bad_forcing_modifier_calls():
  """pm_column_steps with PM_OP_WA_TWOBASIN / PM_OP_WA_PSI on calls that are wrong in exactly one
  way: PM_EINVAL and the modifier's name in the message, before anything is launched (the stand-in
  pointers are never dereferenced).  The call they are all derived from is accepted
  (pm_column_kernel_name: the same checks, no launch)."""
  from pymoc_amd import _lib
  L, C = _lib.lib, ctypes
  A = 0x10000
  T, WEFF, CT = _lib.PM_OP_TIMESTEP, _lib.PM_OP_WEFF, _lib.PM_OP_CONTRACTED
  PSI, TWO = _lib.PM_OP_WA_PSI, _lib.PM_OP_WA_TWOBASIN

  def cols(ncols):
    c = _lib.pm_columns()
    c.ncols, c.nz, c.nsel = ncols, 10, 1
    c.z = c.b = c.kappa = c.area = c.dAkappa = c.bs = c.bbot = c.N2min = c.flags = A
    return c

  def accepted(ncols, vdx, nsteps, ops):
    buf = C.create_string_buffer(96)
    c = cols(ncols)
    return L.pm_column_kernel_name(C.byref(c), A, vdx, nsteps, ops, 0, buf, 96) == _lib.PM_OK and buf.value != b""

  def refused(ncols, vdx, nsteps, ops, word, wA=A, b_in=A):
    c = cols(ncols)
    rc = L.pm_column_steps(C.byref(c), wA, vdx, b_in, 1., nsteps, ops, 0, None)
    return rc == _lib.PM_EINVAL and word in L.pm_last_error().decode()

  # the two-basin modifier: a three-column ensemble, >= 3 plain steps, three arrays
  assert accepted(6, A, 3, T | TWO) and accepted(6, A, 3, T | TWO | CT)
  assert refused(7, A, 3, T | TWO, "PM_OP_WA_TWOBASIN")   # ncols % 3 != 0
  assert refused(8, A, 3, T | TWO, "PM_OP_WA_TWOBASIN")
  assert refused(6, A, 2, T | TWO, "PM_OP_WA_TWOBASIN")   # nsteps < 3
  assert refused(6, A, 1, T | TWO, "PM_OP_WA_TWOBASIN")
  assert refused(6, None, 3, T | TWO, "PM_OP_WA_TWOBASIN")  # vdx_in = NULL
  assert refused(6, A, 3, T | TWO | WEFF, "PM_OP_WA_TWOBASIN")
  assert refused(6, A, 3, T | TWO | PSI, "PM_OP_WA_TWOBASIN")
  assert refused(6, A, 3, _lib.PM_OP_VERTADVDIFF | TWO, "PM_OP_WA_TWOBASIN")  # not a whole timestep
  assert refused(6, A, 3, T | TWO, "wA", wA=None)
  assert refused(6, A, 3, T | TWO, "b_in", b_in=None)
  # the two-column modifier: an even number of columns, >= 3 plain steps, no horadv slot
  assert accepted(6, None, 3, T | PSI) and accepted(6, None, 3, T | PSI | CT)
  assert refused(7, None, 3, T | PSI, "PM_OP_WA_PSI")     # odd ncols
  assert refused(6, A, 3, T | PSI, "PM_OP_WA_PSI")        # vdx_in given
  assert refused(6, None, 2, T | PSI, "PM_OP_WA_PSI")
  assert refused(6, None, 3, T | PSI | WEFF, "PM_OP_WA_PSI")
  assert refused(6, None, 3, T | PSI, "wA", wA=None)


def test_cabi_bad_argument_table_of_the_per_member_entries():
  """Every per-member entry point against descriptors that are wrong in exactly one way (each
  shape limit from both sides, each required pointer NULL, bad ops, sizes that disagree between
  descriptors, a bad schedule, PM_SO_HAS_C where it is refused) and against batches with nothing
  to do: the return code and a word of the message.  The stand-in pointers are never
  dereferenced: a row is either refused or returns before any launch (an accepted shape limit is
  shown on an empty batch)."""
  from pymoc_amd import _lib
  L, C = _lib.lib, ctypes
  A = 0x10000
  OK, EINVAL = _lib.PM_OK, _lib.PM_EINVAL

  def fill(obj, names, **kw):
    for f in names.split():
      setattr(obj, f, A)
    for k, v in kw.items():
      setattr(obj, k, v)
    return obj

  def cols(ncols, nsel):
    return fill(_lib.pm_columns(), "z b kappa area dAkappa bs bbot N2min flags ksel",
                ncols=ncols, nz=100, nsel=nsel)

  def tw():
    return fill(_lib.pm_thermwind(), "z b1 b2 f Psi", n=2, nz=100, nb=50)

  def so():
    return fill(_lib.pm_psi_so(), "z y b bs tau KGM Psi Psi_Ek Psi_GM", n=2, nz=100, ny=40)

  def ml():
    return fill(_lib.pm_so_ml(), "y bs b_basin Psi_b surflux rest_mask b_rest status", n=2, nz=100,
                ny=40)

  def jn():
    j = fill(_lib.pm_jn2018(), "wA Psi_SO Psi_res_b Psi_res_n", n=2, hints=_lib.PM_JN_UNIFORM_AREA)
    j.cols, j.ml = cols(4, 2), ml()
    return j

  def sched():
    return _lib.pm_run_schedule(1, 1, 1, 1)

  def twocol():
    r = fill(_lib.pm_twocol_loop(), "wA", dt=1.)
    r.cols, r.tw, r.sched = cols(4, 1), fill(tw(), "wA1 wA2"), sched()
    return r

  def jnrun():
    r = _lib.pm_jn2018_loop()
    r.jn, r.tw, r.so, r.dt, r.sched = jn(), tw(), so(), 1., sched()
    return r

  # entry -> (the valid descriptors, the call); "@name" edits replace a call argument
  entries = {
      "tw": (lambda: dict(tw=tw()), dict(ops=7),
             lambda d, a: L.pm_thermwind_update(C.byref(d["tw"]), a["ops"], None)),
      "so": (lambda: dict(so=so()), dict(ops=3),
             lambda d, a: L.pm_psi_so_update(C.byref(d["so"]), a["ops"], None)),
      "ml": (lambda: dict(ml=ml()), dict(),
             lambda d, a: L.pm_so_ml_step(C.byref(d["ml"]), 1., None)),
      "so_tw": (lambda: dict(so=so(), tw=tw()), dict(ops=7),
                lambda d, a: L.pm_so_tw_update(C.byref(d["so"]), C.byref(d["tw"]), a["ops"], None)),
      "steps": (lambda: dict(jn=jn()), dict(nsteps=5),
                lambda d, a: L.pm_jn2018_steps(C.byref(d["jn"]), 1., a["nsteps"], None)),
      "run": (lambda: dict(r=jnrun()), dict(),
              lambda d, a: L.pm_jn2018_run(C.byref(d["r"]), None)),
      "twocol": (lambda: dict(r=twocol()), dict(),
                 lambda d, a: L.pm_twocol_run(C.byref(d["r"]), None)),
  }

  def call(entry, edits):
    make, args, fn = entries[entry]
    d, args = make(), dict(args)
    for path, v in edits.items():
      if path.startswith("@"):
        args[path[1:]] = v
        continue
      *head, leaf = path.split(".")
      obj = d[head[0]]
      for h in head[1:]:
        obj = getattr(obj, h)
      setattr(obj, leaf, v)
    rc = fn(d, args)
    return rc, L.pm_last_error().decode()

  def empty(prefix, n_fields, **more):  # the batch with no members (and what follows from it)
    e = {prefix + f: 0 for f in n_fields.split()}
    e.update({prefix + k: v for k, v in more.items()})
    return e

  E_JN = empty("jn.", "n cols.ncols ml.n")
  E_RUN = dict(empty("r.jn.", "n cols.ncols ml.n"), **{"r.tw.n": 0, "r.so.n": 0})
  E_TWOCOL = empty("r.", "tw.n cols.ncols")
  rows = [
      # ---- pm_thermwind_update
      ("tw", {"tw.n": -1}, EINVAL, "shape"),
      ("tw", {"tw.nz": 1}, EINVAL, "nz=1"),
      ("tw", {"tw.nz": 1025}, EINVAL, "nz=1025"),
      ("tw", {"tw.n": 0, "tw.nz": 1025}, EINVAL, "nz=1025"),
      ("tw", {"tw.n": 0, "tw.nz": 2}, OK, ""),
      ("tw", {"tw.n": 0, "tw.nz": 1024}, OK, ""),
      ("tw", {"tw.n": 0, "tw.z": None, "tw.b1": None, "tw.b2": None, "tw.f": None, "tw.Psi": None}, OK, ""),
      ("tw", {"@ops": 0}, EINVAL, "ops"),
      ("tw", {"@ops": 16}, EINVAL, "ops"),
      ("tw", {"@ops": 4}, EINVAL, "PM_TW_PSIB"),
      ("tw", {"tw.nb": 0}, EINVAL, "nb"),
      ("tw", {"tw.n": 0, "tw.nb": 0}, EINVAL, "nb"),
      ("tw", {"tw.n": 0, "tw.nb": 0, "@ops": 1}, OK, ""),
      ("tw", {"tw.z": None}, EINVAL, "NULL"),
      ("tw", {"tw.b1": None}, EINVAL, "NULL"),
      ("tw", {"tw.b2": None}, EINVAL, "NULL"),
      ("tw", {"tw.Psi": None}, EINVAL, "NULL"),
      ("tw", {"tw.f": None}, EINVAL, "NULL"),
      # ---- pm_psi_so_update
      ("so", {"so.n": -1}, EINVAL, "shape"),
      ("so", {"so.nz": 1}, EINVAL, "nz=1"),
      ("so", {"so.nz": 513}, EINVAL, "nz=513"),
      ("so", {"so.ny": 1}, EINVAL, "ny=1"),
      ("so", {"so.ny": 2049}, EINVAL, "ny=2049"),
      ("so", {"so.n": 0, "so.nz": 2, "so.ny": 2}, OK, ""),
      ("so", {"so.n": 0, "so.nz": 512, "so.ny": 2048}, OK, ""),
      ("so", {"so.n": 0, "so.nz": 513}, EINVAL, "nz=513"),
      ("so", {"so.n": 0, "so.z": None, "so.Psi": None, "so.bvp_refine": 1000}, OK, ""),
      ("so", {"@ops": 0}, EINVAL, "ops"),
      ("so", {"@ops": 4}, EINVAL, "ops"),
      ("so", {"so.bvp_refine": -2}, EINVAL, "bvp_refine"),
      ("so", {"so.bvp_refine": 257}, EINVAL, "bvp_refine"),
      ("so", {"so.Psi": None}, EINVAL, "Psi"),
      ("so", {"so.Psi_GM": None}, EINVAL, "Psi_GM"),
  ] + [("so", {"so." + f: None}, EINVAL, "NULL") for f in "z y b bs tau KGM Psi_Ek".split()] + [
      # ---- pm_so_ml_step
      ("ml", {"ml.n": -1}, EINVAL, "shape"),
      ("ml", {"ml.nz": 1}, EINVAL, "nz=1"),
      ("ml", {"ml.nz": 4097}, EINVAL, "nz=4097"),
      ("ml", {"ml.ny": 2}, EINVAL, "ny=2"),
      ("ml", {"ml.ny": 2049}, EINVAL, "ny=2049"),
      ("ml", {"ml.n": 0, "ml.nz": 2, "ml.ny": 3}, OK, ""),
      ("ml", {"ml.n": 0, "ml.nz": 4096, "ml.ny": 2048}, OK, ""),
      ("ml", {"ml.n": 0, "ml.ny": 2}, EINVAL, "ny=2"),
      ("ml", {"ml.n": 0, "ml.y": None, "ml.bs": None}, OK, ""),
  ] + [("ml", {"ml." + f: None}, EINVAL, "NULL")
       for f in "y bs b_basin Psi_b surflux rest_mask b_rest".split()] + [
      # ---- pm_so_tw_update
      ("so_tw", {"so.n": 3}, EINVAL, "inconsistent"),
      ("so_tw", {"tw.n": 3}, EINVAL, "inconsistent"),
      ("so_tw", {"so.nz": 99}, EINVAL, "inconsistent"),
      ("so_tw", {"so.n": -1, "tw.n": -1}, EINVAL, "inconsistent"),
      ("so_tw", {"so.nz": 1, "tw.nz": 1}, EINVAL, "pm_so_tw_update"),
      ("so_tw", {"so.nz": 257, "tw.nz": 257}, EINVAL, "nz"),
      ("so_tw", {"so.ny": 1}, EINVAL, "pm_so_tw_update"),
      ("so_tw", {"so.ny": 2049}, EINVAL, "pm_so_tw_update"),
      ("so_tw", {"tw.nb": 0}, EINVAL, "pm_so_tw_update"),
      ("so_tw", {"tw.nb": 0, "@ops": 1}, EINVAL, "pm_so_tw_update"),
      ("so_tw", {"so.flags": _lib.PM_SO_HAS_C}, EINVAL, "smoother"),
      ("so_tw", {"@ops": 0}, EINVAL, "ops"),
      ("so_tw", {"@ops": 16}, EINVAL, "ops"),
      ("so_tw", {"@ops": 4}, EINVAL, "ops"),
      ("so_tw", {"so.n": 0, "tw.n": 0, "so.nz": 2, "tw.nz": 2, "so.ny": 2, "tw.nb": 1}, OK, ""),
      ("so_tw", {"so.n": 0, "tw.n": 0, "so.nz": 256, "tw.nz": 256, "so.ny": 2048}, OK, ""),
      ("so_tw", {"so.n": 0, "tw.n": 0, "so.bvp_refine": 1000, "so.z": None, "tw.z": None}, OK, ""),
      ("so_tw", {"so.n": 0, "tw.n": 0, "so.flags": _lib.PM_SO_HAS_C}, EINVAL, "smoother"),
      ("so_tw", {"tw.f": None}, EINVAL, "pm_thermwind"),
  ] + [("so_tw", {"so." + f: None}, EINVAL, "pm_psi_so")
       for f in "z y b bs tau KGM Psi Psi_Ek Psi_GM".split()] + [
      ("so_tw", {"tw." + f: None}, EINVAL, "pm_thermwind") for f in "z b1 b2 Psi".split()] + [
      # ---- pm_jn2018_steps (an empty batch still names its arrays)
      ("steps", {"jn.n": -1}, EINVAL, "inconsistent"),
      ("steps", {"jn.n": 3}, EINVAL, "inconsistent"),
      ("steps", {"jn.cols.ncols": 5}, EINVAL, "inconsistent"),
      ("steps", {"jn.ml.n": 3}, EINVAL, "inconsistent"),
      ("steps", {"jn.ml.nz": 99}, EINVAL, "inconsistent"),
      ("steps", {"jn.cols.nz": 1, "jn.ml.nz": 1}, EINVAL, "nz=1"),
      ("steps", {"jn.cols.nz": 257, "jn.ml.nz": 257}, EINVAL, "nz=257"),
      ("steps", {"jn.ml.ny": 2}, EINVAL, "ny=2"),
      ("steps", {"jn.ml.ny": 2049}, EINVAL, "ny=2049"),
      ("steps", {"jn.cols.nsel": 1}, EINVAL, "nsel"),
      ("steps", {"jn.cols.ksel": None}, EINVAL, ".cols has a NULL"),
      ("steps", {"@nsteps": -1}, EINVAL, "nsteps"),
      ("steps", {"@nsteps": 0}, OK, ""),
      ("steps", dict(E_JN), OK, ""),
      ("steps", dict(E_JN, **{"jn.cols.nz": 2, "jn.ml.nz": 2, "jn.ml.ny": 3}), OK, ""),
      ("steps", dict(E_JN, **{"jn.cols.nz": 256, "jn.ml.nz": 256, "jn.ml.ny": 2048}), OK, ""),
      ("steps", dict(E_JN, **{"jn.wA": None}), EINVAL, "NULL"),
  ] + [("steps", {"jn.cols." + f: None}, EINVAL, ".cols has a NULL")
       for f in "z b kappa area dAkappa bs bbot N2min".split()] + [
      ("steps", {"jn." + f: None}, EINVAL, "NULL") for f in "wA Psi_SO Psi_res_b Psi_res_n".split()] + [
      ("steps", {"jn.ml." + f: None}, EINVAL, ".ml has a NULL")
      for f in "y bs surflux rest_mask b_rest".split()] + [
      # ---- pm_jn2018_run
      ("run", {"r.jn.n": -1}, EINVAL, "inconsistent"),
      ("run", {"r.jn.cols.ncols": 5}, EINVAL, "inconsistent"),
      ("run", {"r.jn.ml.n": 3}, EINVAL, "inconsistent"),
      ("run", {"r.jn.ml.nz": 99}, EINVAL, "inconsistent"),
      ("run", {"r.tw.n": 3}, EINVAL, "inconsistent"),
      ("run", {"r.tw.nz": 99}, EINVAL, "inconsistent"),
      ("run", {"r.so.n": 3}, EINVAL, "inconsistent"),
      ("run", {"r.so.nz": 99}, EINVAL, "inconsistent"),
      ("run", {"r.so.ny": 39}, EINVAL, "inconsistent"),
      ("run", {"r.jn.hints": 0}, EINVAL, "PM_JN_UNIFORM_AREA"),
      ("run", {"r.jn.ml.status": None}, EINVAL, "ml.status"),
      ("run", {"r.jn.ml.ny": 65, "r.so.ny": 65}, EINVAL, "ny"),
      ("run", {"r.jn.ml.ny": 2, "r.so.ny": 2}, EINVAL, "ml"),
      ("run", {"r.jn.cols.nz": 3, "r.jn.ml.nz": 3, "r.tw.nz": 3, "r.so.nz": 3}, EINVAL, "nz"),
      ("run", {"r.jn.cols.nz": 257, "r.jn.ml.nz": 257, "r.tw.nz": 257, "r.so.nz": 257}, EINVAL, "nz"),
      ("run", {"r.jn.cols.nz": 50, "r.jn.ml.nz": 50, "r.tw.nz": 50, "r.so.nz": 50}, EINVAL,
       "not supported"),
      ("run", {"r.jn.cols.nsel": 1}, EINVAL, "nsel"),
      ("run", {"r.tw.nb": 0}, EINVAL, "tw"),
      ("run", {"r.tw.b1_mid": A}, EINVAL, "tw"),
      ("run", {"r.tw.b2_mid": A}, EINVAL, "tw"),
      ("run", {"r.so.flags": _lib.PM_SO_HAS_C}, EINVAL, "smoother"),
      ("run", {"r.sched.n_first": -1}, EINVAL, "schedule"),
      ("run", {"r.sched.n_updates": -1}, EINVAL, "schedule"),
      ("run", {"r.sched.m_steps": -1}, EINVAL, "schedule"),
      ("run", {"r.sched.n_last": -1}, EINVAL, "schedule"),
      ("run", {"r.sched.n_first": 0, "r.sched.n_updates": 0}, OK, ""),
      ("run", {"r.sched.n_first": 0, "r.sched.n_updates": 0, "r.tw.z": None}, EINVAL, "tw"),
      ("run", dict(E_RUN), OK, ""),
      ("run", dict(E_RUN, **{"r.so.Psi": None}), EINVAL, "so"),
      ("run", dict(E_RUN, **{"r.jn.cols.nz": 4, "r.jn.ml.nz": 4, "r.tw.nz": 4, "r.so.nz": 4,
                             "r.jn.ml.ny": 3, "r.so.ny": 3, "r.tw.nb": 1}), OK, ""),
      ("run", dict(E_RUN, **{"r.jn.cols.nz": 256, "r.jn.ml.nz": 256, "r.tw.nz": 256, "r.so.nz": 256,
                             "r.jn.ml.ny": 64, "r.so.ny": 64}), OK, ""),
  ] + [("run", {"r.jn.cols." + f: None}, EINVAL, "jn.cols has a NULL")
       for f in "z b kappa area dAkappa bs bbot N2min ksel".split()] + [
      ("run", {"r.jn." + f: None}, EINVAL, "jn has a NULL") for f in "wA Psi_SO Psi_res_b Psi_res_n".split()] + [
      ("run", {"r.jn.ml." + f: None}, EINVAL, "jn.ml has a NULL")
      for f in "y bs surflux rest_mask b_rest".split()] + [
      ("run", {"r.tw." + f: None}, EINVAL, "tw has a NULL") for f in "z b1 b2 f Psi".split()] + [
      ("run", {"r.so." + f: None}, EINVAL, "so has a NULL")
      for f in "z y b bs tau KGM Psi Psi_Ek Psi_GM".split()] + [
      # ---- pm_twocol_run
      ("twocol", {"r.tw.n": -1}, EINVAL, "inconsistent"),
      ("twocol", {"r.tw.n": 3}, EINVAL, "inconsistent"),
      ("twocol", {"r.cols.ncols": 5}, EINVAL, "inconsistent"),
      ("twocol", {"r.tw.nz": 99}, EINVAL, "inconsistent"),
      ("twocol", {"r.cols.nz": 3, "r.tw.nz": 3}, EINVAL, "nz"),
      ("twocol", {"r.cols.nz": 257, "r.tw.nz": 257}, EINVAL, "nz"),
      ("twocol", {"r.cols.nz": 50, "r.tw.nz": 50}, EINVAL, "not supported"),
      ("twocol", {"r.tw.nb": 0}, EINVAL, "pm_twocol_run"),
      ("twocol", {"r.cols.nsel": 0}, EINVAL, "nsel"),
      ("twocol", {"r.cols.nsel": 3}, EINVAL, "nsel"),
      ("twocol", {"r.cols.nsel": 2, "r.cols.ksel": None}, EINVAL, "ksel"),
      ("twocol", {"r.sched.n_first": -1}, EINVAL, "schedule"),
      ("twocol", {"r.sched.n_updates": -1}, EINVAL, "schedule"),
      ("twocol", {"r.sched.m_steps": -1}, EINVAL, "schedule"),
      ("twocol", {"r.sched.n_last": -1}, EINVAL, "schedule"),
      ("twocol", {"r.sched.n_first": 0, "r.sched.n_updates": 0, "r.tw.z": None, "r.cols.z": None,
                  "r.wA": None}, OK, ""),
      ("twocol", dict(E_TWOCOL, **{"r.tw.z": None, "r.cols.z": None, "r.wA": None}), OK, ""),
      ("twocol", dict(E_TWOCOL, **{"r.cols.nz": 4, "r.tw.nz": 4, "r.tw.nb": 1}), OK, ""),
      ("twocol", dict(E_TWOCOL, **{"r.cols.nz": 256, "r.tw.nz": 256, "r.cols.nsel": 2}), OK, ""),
      ("twocol", dict(E_TWOCOL, **{"r.cols.nz": 257, "r.tw.nz": 257}), EINVAL, "nz"),
      ("twocol", {"r.tw.b1_mid": A}, EINVAL, "pm_twocol_run"),
      ("twocol", {"r.tw.b2_mid": A}, EINVAL, "pm_twocol_run"),
      ("twocol", {"r.tw.Psi_SO": A}, EINVAL, "pm_twocol_run"),
      ("twocol", {"r.wA": None}, EINVAL, "tw has a NULL"),
  ] + [("twocol", {"r.cols." + f: None}, EINVAL, "cols has a NULL")
       for f in "z b kappa area dAkappa bs bbot N2min flags".split()] + [
      ("twocol", {"r.tw." + f: None}, EINVAL, "tw has a NULL")
      for f in "z b1 b2 f Psi wA1 wA2".split()]
  bad = []
  for entry, edits, want, word in rows:
    rc, msg = call(entry, edits)
    if rc != want or (want != OK and word not in msg):
      bad.append((entry, edits, want, word, rc, msg))
  assert not bad, bad

  # the descriptor itself missing
  t, s = tw(), so()
  assert L.pm_thermwind_update(None, 7, None) == EINVAL
  assert L.pm_psi_so_update(None, 3, None) == EINVAL
  assert L.pm_so_ml_step(None, 1., None) == EINVAL
  assert L.pm_so_tw_update(None, C.byref(t), 7, None) == EINVAL
  assert L.pm_so_tw_update(C.byref(s), None, 7, None) == EINVAL
  assert L.pm_jn2018_steps(None, 1., 1, None) == EINVAL
  assert L.pm_jn2018_run(None, None) == EINVAL
  assert L.pm_twocol_run(None, None) == EINVAL

  # pm_run_lds_bytes: bad arguments are refused, an unsupported shape is reported as 0 bytes
  nbytes = C.c_size_t(7)
  assert L.pm_run_lds_bytes(0, 100, 50, 0, None) == EINVAL
  assert L.pm_run_lds_bytes(2, 100, 50, 0, C.byref(nbytes)) == EINVAL
  assert L.pm_run_lds_bytes(-1, 100, 50, 0, C.byref(nbytes)) == EINVAL
  for kind, nz, nb, ny, some in [(0, 100, 50, 0, True), (0, 65, 1, 0, True), (0, 128, 50, 0, True),
                                 (0, 193, 50, 0, True), (0, 256, 50, 0, True), (0, 64, 50, 0, False),
                                 (0, 129, 50, 0, False), (0, 192, 50, 0, False), (0, 257, 50, 0, False),
                                 (0, 100, 0, 0, False), (1, 100, 50, 40, True), (1, 100, 50, 3, True),
                                 (1, 100, 50, 64, True), (1, 100, 50, 2, False), (1, 100, 50, 65, False),
                                 (1, 64, 50, 40, False), (1, 100, 0, 40, False)]:
    assert L.pm_run_lds_bytes(kind, nz, nb, ny, C.byref(nbytes)) == OK
    assert (nbytes.value > 0) == some, (kind, nz, nb, ny, nbytes.value)


def test_column_kernel_name_follows_the_launch_plan():
  """pm_column_kernel_name names the instantiation pm_column_steps launches, read off the call
  alone: one case per row of the launch plan (column.hip.h, column_plan) and both sides of each
  gate, spelled as rocprofv3 reports it.  The stand-in pointers are never dereferenced."""
  from pymoc_amd import _lib
  L, C = _lib.lib, ctypes
  A, M = 0x10000, 0x10008  # 16-byte aligned / misaligned addresses
  T, WEFF, CT = _lib.PM_OP_TIMESTEP, _lib.PM_OP_WEFF, _lib.PM_OP_CONTRACTED
  PSI, TWO = _lib.PM_OP_WA_PSI, _lib.PM_OP_WA_TWOBASIN

  def name(ncols=32768, nz=100, nsteps=1, ops=T, ua=False, d3=False, aff=False, b=A, wA=A,
           vdx=None, lanes=0):
    c = _lib.pm_columns()
    c.ncols, c.nz, c.nsel = ncols, nz, 1
    c.reserved = (_lib.PM_COLS_ALL_UNIFORM_AREA if ua else 0) | (_lib.PM_COLS_DIV3_PROVEN if d3 else 0)
    c.z = c.kappa = c.area = c.dAkappa = c.bs = c.bbot = c.N2min = A
    c.b = b
    if aff:
      c.kappa_base = c.kappa_profile = A
    buf = C.create_string_buffer(96)
    rc = L.pm_column_kernel_name(C.byref(c), wA, vdx, nsteps, ops, lanes, buf, 96)
    assert rc == _lib.PM_OK, L.pm_last_error()
    return buf.value.decode()

  lean = dict(ops=T | WEFF, aff=True, ua=True)
  S = "k_column_stream<%s>"
  cases = [
      # one wave per column, P <= 4, 1-2 plain steps, >= 16384 columns: the streaming kernel;
      # lean (PM_OP_WEFF, affine kappa, every Area one number) with 16-byte accesses
      (dict(lean, d3=True), S % "2,5,true,true,true,true,8,-1,-1"),
      (dict(lean, nsteps=2), S % "2,5,true,true,true,false,8,-1,-1"),
      (dict(lean, d3=True, ncols=32760), S % "2,5,true,true,true,true,0,-1,-1"),
      (dict(lean, ncols=32772), S % "2,5,true,true,true,false,0,-1,-1"),
      (dict(lean, ncols=16384), S % "2,5,true,true,true,false,0,-1,-1"),
      (dict(lean, ncols=16383), "k_column_steps<64,2,0,false,false>"),
      (dict(lean, nsteps=3), "k_column_steps<64,2,2,true,true>"),
      # ... without them: nz odd, b or the forcing misaligned, P != 2 (PM_COLS_DIV3_PROVEN unused)
      (dict(lean, d3=True, nz=99), S % "2,5,true,true,false,false,0,-1,-1"),
      (dict(lean, d3=True, b=M), S % "2,5,true,true,false,false,0,-1,-1"),
      (dict(lean, d3=True, wA=M), S % "2,5,true,true,false,false,0,-1,-1"),
      (dict(lean, d3=True, nz=64), S % "1,5,true,true,false,false,0,-1,-1"),
      (dict(lean, nz=150), S % "3,5,true,true,false,false,0,-1,-1"),
      (dict(lean, nz=256), S % "4,5,true,true,false,false,0,-1,-1"),
      (dict(lean, nz=257), "k_column_steps<64,5,0,false,false>"),
      (dict(lean, lanes=32), "k_column_steps<32,4,0,false,false>"),
      # straight-line forms: P = 2, no affine kappa, 8 | ncols >= 32768, PM_OP_WEFF == every Area one number
      (dict(), S % "2,2,false,false,false,false,8,0,0"),
      (dict(b=M, wA=M), S % "2,2,false,false,false,false,8,0,0"),
      (dict(ops=T | WEFF, ua=True), S % "2,3,false,false,false,false,8,1,1"),
      (dict(ops=T | WEFF, ua=True, d3=True), S % "2,3,false,false,false,false,8,1,1"),
      (dict(ncols=32760), S % "2,2,false,false,false,false,0,-1,-1"),
      (dict(ncols=32772), S % "2,2,false,false,false,false,0,-1,-1"),
      (dict(nz=64), S % "1,2,false,false,false,false,0,-1,-1"),
      # the other streaming forms
      (dict(ua=True), S % "2,2,false,false,false,false,0,-1,-1"),
      (dict(ops=T | WEFF), S % "2,3,false,false,false,false,0,-1,-1"),
      (dict(aff=True), S % "2,3,true,false,false,false,0,-1,-1"),
      (dict(aff=True, ua=True), S % "2,3,true,false,false,false,0,-1,-1"),
      (dict(ops=T | WEFF, aff=True), S % "2,4,true,false,false,false,0,-1,-1"),
      (dict(ops=T | CT, ncols=16384), S % "2,2,false,false,false,false,0,-1,-1"),
      (dict(ops=T | WEFF, ncols=16384, nz=200), S % "4,3,false,false,false,false,0,-1,-1"),
      # not a plain timestep: horadv, part of the step
      (dict(vdx=A), "k_column_steps<64,2,0,false,false>"),
      (dict(ops=_lib.PM_OP_CONVECT | _lib.PM_OP_VERTADVDIFF), "k_column_steps<64,2,0,false,false>"),
      # >= 3 steps: the fused kernel
      (dict(nsteps=3, ops=T | CT), "k_column_steps<64,2,4,true,false>"),
      (dict(nsteps=3, ops=T | CT, ua=True, d3=True), "k_column_steps<64,2,4,true,false>"),
      (dict(nsteps=3, ops=T | CT, lanes=32), "k_column_steps<32,4,2,true,false>"),
      (dict(nsteps=3, ops=T | CT, nz=300), "k_column_steps<64,5,2,true,false>"),
      (dict(nsteps=3, ops=T | CT, vdx=A), "k_column_steps<64,2,1,false,false>"),
      (dict(nsteps=3, ua=True, d3=True), "k_column_steps<64,2,6,true,true>"),
      (dict(nsteps=3, ua=True), "k_column_steps<64,2,2,true,true>"),
      (dict(nsteps=3, d3=True), "k_column_steps<64,2,2,true,false>"),
      (dict(nsteps=3, ua=True, d3=True, nz=256), "k_column_steps<64,4,6,true,true>"),
      (dict(nsteps=3, ua=True, nz=300), "k_column_steps<64,5,2,true,false>"),
      (dict(nsteps=3, ua=True, lanes=16), "k_column_steps<16,7,2,true,false>"),
      (dict(nsteps=3, ops=T | WEFF, aff=True, ua=True), "k_column_steps<64,2,2,true,true>"),
      (dict(nsteps=3), "k_column_steps<64,2,2,true,false>"),
      (dict(nsteps=3, ops=T | PSI, ua=True, d3=True), "k_column_steps<64,2,6,true,true>"),
      (dict(nsteps=3, ops=T | PSI, lanes=16), "k_column_steps<16,7,2,true,false>"),
      (dict(nsteps=3, ops=T | TWO, ncols=3000, vdx=A), "k_column_steps<64,2,2,true,false>"),
      (dict(nsteps=3, ops=T | TWO, ncols=3000, vdx=A, ua=True), "k_column_steps<64,2,2,true,true>"),
      (dict(nsteps=3, vdx=A), "k_column_steps<64,2,1,false,false>"),
      (dict(nsteps=3, vdx=A, ua=True), "k_column_steps<64,2,1,false,false>"),
      (dict(nsteps=3, ops=_lib.PM_OP_VERTADVDIFF, lanes=32), "k_column_steps<32,4,1,false,false>"),
      (dict(nsteps=2, ncols=1000, ua=True, d3=True), "k_column_steps<64,2,0,false,false>"),
      (dict(nsteps=1, ncols=100, lanes=16, nz=10), "k_column_steps<16,1,0,false,false>"),
      # nothing to launch
      (dict(nsteps=0), ""),
      (dict(ncols=0), ""),
      (dict(ops=WEFF), ""),
  ]
  for kw, want in cases:
    assert name(**kw) == want, kw

  # the checks are pm_column_steps'
  c = _lib.pm_columns()
  c.ncols, c.nz, c.nsel = 4, 10, 1
  buf = C.create_string_buffer(96)
  assert L.pm_column_kernel_name(None, A, None, 1, T, 0, buf, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T, 0, buf, 96) == _lib.PM_EINVAL
  assert "NULL" in L.pm_last_error().decode()
  c.z = c.b = c.kappa = c.area = c.dAkappa = c.bs = c.bbot = c.N2min = A
  assert L.pm_column_kernel_name(C.byref(c), None, None, 1, T, 0, buf, 96) == _lib.PM_EINVAL
  assert "wA" in L.pm_last_error().decode()
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, 128, 0, buf, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T | PSI, 0, buf, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 3, T | TWO, 0, buf, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T, 8, buf, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T, 0, None, 96) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T, 0, buf, 8) == _lib.PM_EINVAL
  assert L.pm_column_kernel_name(C.byref(c), A, None, 1, T, 0, buf, 96) == _lib.PM_OK
  assert buf.value == b"k_column_steps<64,1,0,false,false>"


def test_column_kernel_twin_follows_the_launch():
  """pm_column_kernel_twin: launches of at least 64 steps of the one-wave-per-column uniform-Area
  rows with at most 2 levels per lane run k_column_steps_cls (launch_column_kernel asks the same
  predicate); every other launch, and a call that launches nothing, does not.  The row's name stays
  the one pm_column_kernel_name reports either way."""
  from pymoc_amd import _lib
  L, C = _lib.lib, ctypes
  A = 0x10000
  T, CT, PSI, TWO = _lib.PM_OP_TIMESTEP, _lib.PM_OP_CONTRACTED, _lib.PM_OP_WA_PSI, _lib.PM_OP_WA_TWOBASIN

  def twin(ncols=1024, nz=100, nsteps=64, ops=T, ua=True, d3=True, vdx=None, lanes=0):
    c = _lib.pm_columns()
    c.ncols, c.nz, c.nsel = ncols, nz, 1
    c.reserved = (_lib.PM_COLS_ALL_UNIFORM_AREA if ua else 0) | (_lib.PM_COLS_DIV3_PROVEN if d3 else 0)
    c.z = c.b = c.kappa = c.area = c.dAkappa = c.bs = c.bbot = c.N2min = A
    out, buf = C.c_int32(-1), C.create_string_buffer(96)
    assert L.pm_column_kernel_twin(C.byref(c), A, vdx, nsteps, ops, lanes, C.byref(out)) == _lib.PM_OK
    assert L.pm_column_kernel_name(C.byref(c), A, vdx, nsteps, ops, lanes, buf, 96) == _lib.PM_OK
    assert "_cls" not in buf.value.decode()
    return out.value

  for kw, want in [
      (dict(), 1), (dict(nsteps=63), 0), (dict(nsteps=65), 1), (dict(nsteps=1000, d3=False), 1),
      (dict(nz=9), 1), (dict(nz=64), 1), (dict(nz=65), 1), (dict(nz=128), 1), (dict(nz=129), 0),
      (dict(nz=256), 0), (dict(ua=False), 0), (dict(lanes=16), 0), (dict(lanes=32), 0),
      (dict(lanes=64), 1), (dict(ops=T | CT), 0), (dict(vdx=A), 0), (dict(ops=T | PSI), 1),
      (dict(ops=T | PSI, nsteps=24), 0), (dict(ops=T | TWO, ncols=3000, vdx=A), 1),
      (dict(ops=T | TWO, ncols=3000, vdx=A, ua=False), 0), (dict(nsteps=2), 0),
      (dict(nsteps=1, ncols=32768), 0), (dict(nsteps=0), 0), (dict(ncols=0), 0),
      (dict(ops=_lib.PM_OP_VERTADVDIFF), 0)]:
    assert twin(**kw) == want, kw
  c = _lib.pm_columns()
  c.ncols, c.nz, c.nsel = 4, 10, 1
  out = C.c_int32(-1)
  assert L.pm_column_kernel_twin(C.byref(c), A, None, 64, T, 0, C.byref(out)) == _lib.PM_EINVAL
  c.z = c.b = c.kappa = c.area = c.dAkappa = c.bs = c.bbot = c.N2min = A
  assert L.pm_column_kernel_twin(C.byref(c), A, None, 64, T, 0, None) == _lib.PM_EINVAL
  assert L.pm_column_kernel_twin(C.byref(c), A, None, 64, T, 8, C.byref(out)) == _lib.PM_EINVAL


def test_every_launch_plan_row_has_a_whole_batch_oracle_case():
  """tests/column_plan_cases.py, the table tests/test_column_plan_gpu.py runs on the device, holds
  every row of PM_COLUMN_KERNELS (a row added without a numeric case fails here), each entry's
  call selects the instantiation the entry names, and the rows differ in the template arguments
  behind the shape.  The planted columns cover every kind at every slot of a wave."""
  from pymoc_amd import _lib
  import column_plan_cases as T
  text = open(os.path.join(ROOT, "pymoc_amd", "csrc", "column.hip.h")).read()
  rows = re.findall(r"X\((CK_[A-Z0-9_]+),", text)
  assert len(rows) == len(set(rows)) >= 17
  assert {c.id for c in T.CASES} == set(rows)
  assert len({T.label(c) for c in T.CASES}) == len(T.CASES)
  args = {}
  for c in T.CASES:
    d, wA, vdx = T.stand_in_call(c)
    buf = ctypes.create_string_buffer(96)
    for n in ((2, 1) if c.nsteps == 2 else (c.nsteps,)):  # (two steps also run as 1 + 1)
      rc = _lib.lib.pm_column_kernel_name(ctypes.byref(d), wA, vdx, n, T.op_bits(c), c.lanes, buf, 96)
      assert rc == _lib.PM_OK, _lib.lib.pm_last_error()
      assert buf.value.decode() == c.name, T.label(c)
    kernel, targs = re.fullmatch(r"(k_column_\w+)<(.*)>", c.name).groups()
    shape = 1 if kernel == "k_column_stream" else 2  # <P, ...> / <G, P, ...>
    args.setdefault(c.id, set()).add((kernel, ",".join(targs.split(",")[shape:])))
  assert all(len(v) == 1 for v in args.values()), args
  assert len({next(iter(v)) for v in args.values()}) == len(rows), args
  for ncols in {c.ncols for c in T.CASES}:
    cols, kinds, period = T.planted_columns(ncols)
    assert period % 8 == 0 and kinds[cols == 0] == 3 and kinds[cols == ncols - 1] == 4
    for k in range(8):
      assert set(cols[kinds == k] % 8) == set(range(8)), (ncols, k)


def test_product_does_not_import_oracle():
  pkg = os.path.join(ROOT, "pymoc_amd")
  for dirpath, _, files in os.walk(pkg):
    for f in files:
      if f.endswith((".py", ".h", ".hip")):
        src = open(os.path.join(dirpath, f)).read()
        assert "import oracle" not in src and "from oracle" not in src, f
        assert "pymoc_oracle" not in src, f
        assert "import torch" not in src, f


# ---- utils contract (reference tests/utils/test_make_func.py, test_make_array.py)
def test_make_func_contract():
  from pymoc_amd.utils import make_func
  z = np.linspace(-10., 0., 5)
  f = lambda x: 2 * x  # noqa: E731
  assert make_func(f, z, 'f') is f
  arr = np.arange(5.)
  g = make_func(arr, z, 'g')
  assert np.array_equal(g(z), arr)
  arr[2] = 99.  # closure aliases the caller's array (make_func.py:32-37)
  assert g(z[2]) == 99.
  h = make_func(3.0, z, 'h')
  assert np.array_equal(h(z), 3.0 + 0 * z)
  with pytest.raises(TypeError) as e:
    make_func(1, z, 'myst')
  assert str(e.value) == "('myst', 'needs to be either function, numpy array, or float')"


def test_make_array_contract():
  from pymoc_amd.utils import make_array
  z = np.linspace(-10., 0., 5)
  arr = np.arange(5.)
  assert make_array(arr, z, 'a') is arr
  assert np.array_equal(make_array(lambda x: x**2, z, 'a'), z**2)
  assert np.array_equal(make_array(1.5, z, 'a'), 1.5 + 0 * z)
  with pytest.raises(TypeError) as e:
    make_array(1, z, 'myst')
  assert str(e.value) == "('myst', 'needs to be either function, numpy array, or float')"


def test_column_constructor_contract():
  from pymoc_amd import Column
  z = np.linspace(-4000., 0., 20)
  with pytest.raises(TypeError) as e:
    Column(z=1, kappa=1e-5, Area=1e14)
  assert str(e.value) == 'z needs to be numpy array providing grid levels'
  with pytest.raises(TypeError) as e:
    Column(z=np.array([]), kappa=1e-5, Area=1e14)
  assert str(e.value) == 'z needs to be numpy array providing grid levels'
  with pytest.raises(TypeError) as e:
    Column(z=z, kappa=1, Area=1e14)
  assert str(e.value) == "('kappa', 'needs to be either function, numpy array, or float')"
  with pytest.raises(TypeError) as e:
    Column(z=z, kappa=1e-5, Area=1e14, b=1)
  assert str(e.value) == "('b', 'needs to be either function, numpy array, or float')"
  b = 0.02 * np.exp(z / 300.)
  c = Column(z=z, kappa=lambda x: 1e-5 + 0 * x, Area=8e13, b=b, bs=0.02, bbot=0.001,
             bzbot=None, N2min=2e-7)
  assert c.z is z and c.b is b  # arrays are aliased, not copied (column.py:54,67)
  assert (c.bs, c.bbot, c.bzbot, c.N2min) == (0.02, 0.001, None, 2e-7)
  assert np.array_equal(c.bz, np.gradient(b, z))
  assert np.array_equal(c.Akappa(z), 8e13 * (1e-5 + 0 * z))
  assert np.array_equal(c.dAkappa_dz(z), np.gradient(8e13 * (1e-5 + 0 * z), z))


def test_configs_are_shard_invariant():
  from pymoc_amd import configs
  full = configs.config2(N=64)
  part = configs.config2(N=64, members=(16, 48))
  for k in ("kappa", "Area", "wA", "b0", "bs", "do_conv"):
    assert np.array_equal(full[k][16:48], part[k])
  full = configs.config3(N=32)
  part = configs.config3(N=32, members=(8, 9))
  assert np.array_equal(full["kappa"][8:9], part["kappa"])
  full = configs.config4(N=32)
  part = configs.config4(N=32, members=(30, 32))
  assert np.array_equal(full["tau"][30:32], part["tau"])
  full = configs.config5(N=8)
  part = configs.config5(N=8, members=(2, 5))
  assert np.array_equal(full["b_basin0"][2:5], part["b_basin0"])


def test_explicit_scheme_limits_hold_for_the_bench_configs():
  from pymoc_amd import configs
  for c in (configs.config2(N=256), configs.config3(N=256), configs.config4(N=256)):
    dz = np.diff(c["z"]).min()
    assert (c["kappa"].max() * c["dt"] / dz**2) < 0.5


def test_brentq_restatement_equals_scipy():
  """pymoc_amd.utils.brentq (host root-finding for CALLABLE bs in Psi_SO.ys) is SciPy's brentq
  decision for decision: bit-identical roots on random smooth functions."""
  from scipy import optimize
  from pymoc_amd.utils.brentq import brentq
  rng = np.random.default_rng(5)
  seen = 0
  for k in range(600):
    a, b, c = rng.uniform(0.5, 3), rng.uniform(-2, 2), rng.uniform(-1, 1)
    f = lambda y: np.tanh(a * y + b) + 0.3 * np.sin(3 * y) + 0.2 * c - 0.1 * k / 600
    if f(-4.) * f(4.) > 0:
      continue
    seen += 1
    assert optimize.brentq(f, -4., 4.) == brentq(f, -4., 4.)
  assert seen > 200
  with pytest.raises(ValueError):
    brentq(lambda y: 1. + y * y, -1., 1.)
