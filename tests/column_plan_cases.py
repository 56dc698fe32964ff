"""The column launch plan as a table of whole-batch oracle cases (helper module, no tests).

`pm_column_steps` picks one instantiation per call through `column_plan` (csrc/column.hip.h,
PM_COLUMN_KERNELS).  CASES holds one entry or more per row of that list: the row id, the full
kernel name the call must launch, and the recipe of the call -- ensemble size, levels, steps per
launch, lanes per column, the hints that are on, the number of coefficient sets and the alignment
of `b` and of the forcing.  tests/test_host_cpu.py checks the table against the header and the
names against `pm_column_kernel_name`; tests/test_column_plan_gpu.py runs every entry on the
device and compares EVERY column with the oracle.

Inputs (`host_inputs`): a config-2 ensemble in which what a column carries depends on its place
in its wave -- convective adjustment on a random half, the bottom-stratification condition on a
random 30 %, bbot above bs on a few, and the columns of `_extreme_cases` (operands outside the
exact-division window, inf / NaN levels) planted so that every kind sits at every position
`col % 16` (`col % 8` in the small batches of the fused kernels), an inf column in the first wave
and a NaN column in the last.
"""
import collections
import ctypes as C
import functools

import numpy as np

from pymoc_amd import configs

Case = collections.namedtuple(
    "Case", "id name ncols nz nsteps lanes precombined affine ua div3 nsel b_shift w_shift horadv arith")

# template arguments behind the shape (k_column_stream<P, ...> / k_column_steps<G, P, ...>), written
# out per row as profilers report them
_STREAM_ARGS = {
    "CK_STREAM": "2,false,false,false,false,0,-1,-1",
    "CK_STREAM_WEFF": "3,false,false,false,false,0,-1,-1",
    "CK_STREAM_AFF": "3,true,false,false,false,0,-1,-1",
    "CK_STREAM_WEFF_AFF": "4,true,false,false,false,0,-1,-1",
    "CK_STREAM_LEAN": "5,true,true,false,false,0,-1,-1",
    "CK_STREAM_LEAN_VEC": "5,true,true,true,false,0,-1,-1",
    "CK_STREAM_LEAN_VEC_D3": "5,true,true,true,true,0,-1,-1",
    "CK_STREAM_LEAN_VEC_U8": "5,true,true,true,false,8,-1,-1",
    "CK_STREAM_LEAN_VEC_D3_U8": "5,true,true,true,true,8,-1,-1",
    "CK_STREAM_U8": "2,false,false,false,false,8,0,0",
    "CK_STREAM_WEFF_UA_U8": "3,false,false,false,false,8,1,1",
}
_STEPS_ARGS = {
    "CK_STEPS_IEEE": "0,false,false",
    "CK_STEPS_RECIP": "1,false,false",
    "CK_STEPS_PLAIN": "2,true,false",
    "CK_STEPS_PLAIN_UA": "2,true,true",
    "CK_STEPS_DIV3_UA": "6,true,true",
    "CK_STEPS_CONTRACTED": "4,true,false",
}


def levels_per_lane(nz, lanes):
  """Levels per lane of a column of nz levels on `lanes` lanes (pm_column_kernel_shape)."""
  need = -(-nz // lanes)
  sup = (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16) if lanes == 64 else (1, 2, 3, 4, 5, 6, 7, 8)
  return min(v for v in sup if v >= need)


def _case(id, ncols, nz=100, nsteps=1, lanes=0, precombined=False, affine=False, ua=True, div3=True,
          nsel=1, b_shift=False, w_shift=False, horadv=False, arith="exact"):
  G = lanes or 64
  P = levels_per_lane(nz, G)
  if id in _STREAM_ARGS:
    name = "k_column_stream<%d,%s>" % (P, _STREAM_ARGS[id])
  else:
    name = "k_column_steps<%d,%d,%s>" % (G, P, _STEPS_ARGS[id])
  return Case(id, name, ncols, nz, nsteps, lanes, precombined, affine, ua, div3, nsel, b_shift,
              w_shift, horadv, arith)


def _table():
  t = []
  lean = dict(precombined=True, affine=True)
  # the straight-line lean forms: at the gate (8 * 4096 columns) and the bench's workload
  for id, d3 in (("CK_STREAM_LEAN_VEC_D3_U8", True), ("CK_STREAM_LEAN_VEC_U8", False)):
    for ncols in (32768, 262144):
      for nz in (66, 100, 128):
        for nsteps in (1, 2):
          t.append(_case(id, ncols, nz, nsteps, div3=d3, **lean))
  # the lean ring: 2, 2, 2, 5 and 16 (the clamp) columns per wave, ragged last waves
  ragged = (16384, 32760, 32771, 16384 * 5 + 3, 16384 * 16 + 5)
  for id, d3 in (("CK_STREAM_LEAN_VEC_D3", True), ("CK_STREAM_LEAN_VEC", False)):
    for i, ncols in enumerate(ragged):
      for j, nz in enumerate((66, 100, 128)):
        t.append(_case(id, ncols, nz, 1 + (i + j) % 2, div3=d3, **lean))
  for i, ncols in enumerate(ragged):
    t.append(_case("CK_STREAM_LEAN", ncols, 99, 1 + i % 2, **lean))  # nz odd
  for i, nz in enumerate((64, 150, 256)):  # one, three and four levels per lane
    t.append(_case("CK_STREAM_LEAN", 32771, nz, 1 + i % 2, **lean))
    t.append(_case("CK_STREAM_LEAN", 16384 * 5 + 3, nz, 2 - i % 2, **lean))
  for nsteps in (1, 2):  # nz even, but b or the forcing not 16-byte aligned
    t.append(_case("CK_STREAM_LEAN", 32771, 100, nsteps, b_shift=True, **lean))
    t.append(_case("CK_STREAM_LEAN", 32768, 100, nsteps, w_shift=True, **lean))
  # the straight-line forms with every array in the ring: two coefficient sets
  for i, nz in enumerate((65, 66, 100, 127, 128)):
    for nsteps in (1, 2):
      t.append(_case("CK_STREAM_U8", 32768, nz, nsteps, ua=False, nsel=2))
      t.append(_case("CK_STREAM_WEFF_UA_U8", 32768, nz, nsteps, precombined=True, nsel=2))
  for nsteps in (1, 2):  # ... b and the forcing misaligned: the per-level stores
    t.append(_case("CK_STREAM_U8", 32768, 100, nsteps, ua=False, nsel=2, b_shift=True, w_shift=True))
  # the other streaming forms: ragged under the straight-line gate, not a multiple of 8, four
  # levels per lane
  for id, kw in (("CK_STREAM", dict()), ("CK_STREAM_WEFF", dict(precombined=True)),
                 ("CK_STREAM_AFF", dict(affine=True)),
                 ("CK_STREAM_WEFF_AFF", dict(precombined=True, affine=True, ua=False))):
    t.append(_case(id, 32760, 100, 1, **kw))
    t.append(_case(id, 32772, 100, 2, **kw))
    t.append(_case(id, 16384, 200, 2, **kw))
    t.append(_case(id, 32772, 128, 1, **kw))
  # the fused kernel
  for lanes in (0, 16, 32):
    for nsteps in (1, 2):
      t.append(_case("CK_STEPS_IEEE", 304, 100, nsteps, lanes))
    t.append(_case("CK_STEPS_RECIP", 304, 100, 5, lanes, horadv=True))
    t.append(_case("CK_STEPS_PLAIN", 304, 100, 5, lanes, ua=False))
  t.append(_case("CK_STEPS_PLAIN_UA", 304, 100, 5, div3=False))
  t.append(_case("CK_STEPS_DIV3_UA", 304, 100, 5))
  t.append(_case("CK_STEPS_CONTRACTED", 304, 100, 5, arith="contracted"))
  # entries that share their inputs are neighbours (host_inputs / oracle_result keep the last ones)
  t.sort(key=lambda c: (c.ncols, c.nz, c.nsel, c.horadv, c.nsteps))
  return t


CASES = _table()


def label(c):
  s = "%s-n%d-nz%d-s%d" % (c.id, c.ncols, c.nz, c.nsteps)
  if c.lanes:
    s += "-g%d" % c.lanes
  if c.b_shift:
    s += "-b+8"
  if c.w_shift:
    s += "-w+8"
  return s


def columns_per_wave(c):
  """Columns a wave of the entry's streaming kernel walks through (column_plan); 1 when fused."""
  if c.id not in _STREAM_ARGS:
    return 1
  if c.id.endswith("_U8"):
    return 8
  if c.id.startswith("CK_STREAM_LEAN"):
    return min(max(c.ncols // 16384, 2), 16)
  return min(max(c.ncols // 8192, 1), 32)


# ------------------------------------------------------------------ inputs
def _extreme_cases(c, N):
  """Per-column edits of a config-2 ensemble that leave the window of the exact-division
  shortcuts (common.hip.h: 2^-200 <= |x| <= 2^200 or 0): returns (b0, wA, bs, bbot, kinds)."""
  rng = np.random.default_rng(17)
  b0, wA, bs, bbot = c["b0"].copy(), c["wA"].copy(), c["bs"].copy(), np.array(c["bbot"], dtype=float) + np.zeros(N)
  kinds = rng.integers(0, 8, N)
  nz = b0.shape[1]
  for m in range(N):
    k = kinds[m]
    if k == 1:    # the whole column scaled down by 2^-1000 (forcing too: CFL unchanged)
      s = 2.0**-1000
      b0[m] *= s; bs[m] *= s; bbot[m] *= s
    elif k == 2:  # ... scaled up by 2^+900
      s = 2.0**900
      b0[m] *= s; bs[m] *= s; bbot[m] *= s
    elif k == 3:  # an infinite interior level
      b0[m, nz // 2] = np.inf
    elif k == 4:  # a NaN next to the top, a -inf next to the bottom
      b0[m, nz - 2] = np.nan
      b0[m, 1] = -np.inf
    elif k == 5:  # subnormal forcing
      wA[m] *= 2.0**-1060
    elif k == 6:  # buoyancy differences that round into the subnormal range
      b0[m] = b0[m] * 2.0**-1015
      bs[m] *= 2.0**-1015; bbot[m] *= 2.0**-1015
  return b0, wA, bs, bbot, kinds


@functools.lru_cache(maxsize=None)
def planted_columns(ncols):
  """(columns, kinds, period): the columns of a batch that `_extreme_cases` edits, in the order it
  takes them, and the kind it gives each.  Every kind 0..7 lands on every residue `col % period`
  (the i-th column of a kind takes residue i % period; the columns of one residue are spread over
  the whole batch), column 0 carries an inf level (kind 3) and the last column a NaN (kind 4), so
  that the first and the last wave of a launch both hold a non-finite column."""
  period, n = (16, 448) if ncols >= 16384 else (8, 160)
  nblk = ncols // period
  zero = dict(b0=np.zeros((n, 4)), wA=np.zeros((n, 4)), bs=np.zeros(n), bbot=0.0)
  kinds = _extreme_cases(zero, n)[4]  # (the kinds depend on n alone)
  seen = collections.Counter()
  res = np.empty(n, dtype=int)
  for j, k in enumerate(kinds):
    res[j] = seen[k] % period
    seen[k] += 1
  cols = np.empty(n, dtype=int)
  for r in range(period):
    js = np.nonzero(res == r)[0]
    assert js.size <= nblk
    cols[js] = np.linspace(0, nblk - 1, js.size).astype(int) * period + r
  def swap_to(col, kind):  # put a column of `kind` at `col` without touching the residues' coverage
    js = np.nonzero((kinds == kind) & (res == col % period))[0]
    assert js.size >= 2
    at = np.nonzero(cols == col)[0]
    if at.size:
      cols[js[-1]], cols[at[0]] = cols[at[0]], cols[js[-1]]
    else:
      cols[js[-1]] = col
  swap_to(0, 3)
  swap_to(ncols - 1, 4)
  assert np.unique(cols).size == n and cols.min() == 0 and cols.max() == ncols - 1
  assert kinds[cols == 0] == 3 and kinds[cols == ncols - 1] == 4
  for k in range(8):
    assert set(cols[kinds == k] % period) == set(range(period)), k
  return cols, kinds, period


_cache = {}


def _keep_last(slot, key, make):
  """One value per slot: the big ensembles are a gigabyte each."""
  if _cache.get(slot, (None,))[0] != key:
    _cache.pop(slot, None)
    _cache[slot] = (key, make())
  return _cache[slot][1]


def host_inputs(case):
  """The entry's inputs as host arrays; they do not depend on the kernel the entry selects."""
  key = (case.ncols, case.nz, case.nsel, case.horadv)
  return _keep_last("inputs", key, lambda: _make_inputs(*key))


def _make_inputs(N, nz, nsel, horadv):
  c = configs.config2(N=N, nz=nz)
  rng = np.random.default_rng(100003 * nz + N)
  inp = dict(z=c["z"], kappa=c["kappa"], Area=c["Area"], N2min=c["N2min"],
             kappa_back=c["kappa_back"], kappa_profile=c["kappa_profile"])
  # config 2's 30 days are the explicit scheme's limit at nz = 100: finer grids take less
  inp["dt"] = c["dt"] * min(1.0, (99.0 / (nz - 1))**2)
  inp["do_conv"] = rng.random(N) < 0.5
  has_bz = rng.random(N) < 0.3
  inp["has_bzbot"] = has_bz
  inp["bzbot"] = np.where(has_bz, 1e-7, 0.0)
  b0, wA, bs = c["b0"], c["wA"], c["bs"]
  bbot = np.array(c["bbot"], dtype=float) + np.zeros(N)
  hot = rng.random(N) < 0.04
  bbot[hot] = bs[hot] + 0.005  # bbot above bs
  sel, kinds, _ = planted_columns(N)
  sub = dict(b0=b0[sel], wA=wA[sel], bs=bs[sel], bbot=bbot[sel])
  with np.errstate(all="ignore"):
    b0[sel], wA[sel], bs[sel], bbot[sel], kinds2 = _extreme_cases(sub, sel.size)
  assert np.array_equal(kinds, kinds2)
  inp.update(b0=b0, wA=wA, bs=bs, bbot=bbot)
  inp["kinds"] = np.zeros(N, dtype=int)
  inp["kinds"][sel] = kinds
  inp["ordinary"] = int(np.nonzero(inp["kinds"] == 0)[0][1])  # (an unedited column)
  if nsel == 2:
    inp["kappa_alt"] = c["kappa"] * 1.7
    inp["ksel"] = (rng.random(N) < 0.4).astype(np.int32)
  if horadv:
    inp["vdx"] = c["Area"] * 2e-9 * rng.standard_normal((N, nz))
    inp["b_in"] = 0.02 * rng.random((N, nz))
  return inp


def oracle_result(case, inp):
  """`case.nsteps` timesteps of EVERY column by the CPU oracle, from the host inputs alone."""
  key = (case.ncols, case.nz, case.nsel, case.horadv, case.nsteps)
  return _keep_last("oracle", key, lambda: _oracle(inp, case.nsteps))


def _oracle(inp, nsteps):
  import oracle as O
  kap = inp["kappa"]
  if "ksel" in inp:
    kap = np.where(inp["ksel"][:, None] == 1, inp["kappa_alt"], kap)
  z, area, wA, dt = inp["z"], inp["Area"], inp["wA"], inp["dt"]
  horadv = "vdx" in inp
  if horadv:
    ref = inp["b0"].copy()
    rows = range(ref.shape[0])
  else:  # one C call for the columns with the bbot condition ...
    ref = O.column_ensemble_steps(z, kap, area, inp["b0"], wA, dt, inp["do_conv"], inp["bs"],
                                  inp["bbot"], inp["N2min"], nsteps)
    rows = np.nonzero(inp["has_bzbot"])[0]
  for m in rows:  # ... and column by column where the bottom stratification is prescribed
    b = inp["b0"][m]
    kw = dict(do_conv=bool(inp["do_conv"][m]), bs=inp["bs"][m], bbot=inp["bbot"][m],
              bzbot=inp["bzbot"][m] if inp["has_bzbot"][m] else None, N2min=inp["N2min"][m])
    if horadv:
      kw.update(vdx_in=inp["vdx"][m], b_in=inp["b_in"][m])
    for _ in range(nsteps):
      b = O.column_timestep(z, kap[m], area[m], b, wA[m], dt, **kw)
    ref[m] = b
  return ref


# ------------------------------------------------------------------ the call
ALIGNED, SHIFTED = 0x10000, 0x10008  # stand-in addresses: 16-byte aligned / 8 bytes further


def op_bits(case):
  from pymoc_amd import _lib
  return (_lib.PM_OP_TIMESTEP | (_lib.PM_OP_WEFF if case.precombined else 0) |
          (_lib.PM_OP_CONTRACTED if case.arith == "contracted" else 0))


def stand_in_call(case):
  """(descriptor, wA, vdx_in) of the entry's call with stand-in addresses, for
  pm_column_kernel_name (never dereferenced)."""
  from pymoc_amd import _lib
  d = _lib.pm_columns()
  d.ncols, d.nz, d.nsel = case.ncols, case.nz, case.nsel
  d.reserved = _lib.PM_COLS_ALL_UNIFORM_AREA if case.ua else 0
  if case.ua and case.div3:
    d.reserved |= _lib.PM_COLS_DIV3_PROVEN
  d.z = d.kappa = d.area = d.dAkappa = d.bs = d.bbot = d.bzbot = d.N2min = ALIGNED
  d.flags = d.ksel = d.nonfinite = ALIGNED
  d.b = SHIFTED if case.b_shift else ALIGNED
  if case.affine:
    d.kappa_base = d.kappa_profile = ALIGNED
  return d, (SHIFTED if case.w_shift else ALIGNED), (ALIGNED if case.horadv else None)


class _Rows(object):
  """ncols x nz doubles on the device, 16-byte aligned or starting 8 bytes behind such an
  address (one element more is allocated)."""

  def __init__(self, gpu, ncols, nz, shifted, host=None):
    self.shape = (ncols, nz)
    self.mem = gpu.DeviceArray((ncols * nz + (1 if shifted else 0),))
    self.ptr = self.mem.ptr + (8 if shifted else 0)
    self.nbytes = ncols * nz * 8
    assert self.ptr % 16 == (8 if shifted else 0)
    if host is not None:
      from pymoc_amd._lib import check, lib
      host = np.ascontiguousarray(host, dtype=np.float64)
      assert host.shape == self.shape
      check(lib.pm_memcpy_h2d(self.ptr, host.ctypes.data, self.nbytes, None))

  def download(self, first_row=0, nrows=None):
    from pymoc_amd._lib import check, lib
    nrows = self.shape[0] - first_row if nrows is None else nrows
    out = np.empty((nrows, self.shape[1]))
    check(lib.pm_memcpy_d2h(out.ctypes.data, self.ptr + first_row * self.shape[1] * 8, out.nbytes, None))
    return out

  def free(self):
    self.mem.free()


class DeviceCall(object):
  """A table entry on the device: a ColumnBatch of the entry's inputs with its hints, `b` and
  the forcing at the entry's alignment, and the raw pm_column_steps call on the batch's
  descriptor."""

  def __init__(self, gpu, case, inp):
    from pymoc_amd import _lib
    self.case, self.dt = case, float(inp["dt"])
    N, nz = case.ncols, case.nz
    kw = dict(bs=inp["bs"], bbot=inp["bbot"], N2min=inp["N2min"], do_conv=inp["do_conv"])
    if case.nsel == 2:
      kw["kappa_alt"] = inp["kappa_alt"]
    if case.affine:
      kw["kappa_affine"] = (inp["kappa_back"], inp["kappa_profile"])
    self.batch = batch = gpu.ColumnBatch(inp["z"], inp["kappa"], inp["Area"], inp["b0"], **kw)
    self.owned = []
    if case.nsel == 2:
      batch.set_ksel(inp["ksel"])
    # per-column bottom-stratification flags: the other columns keep the bbot condition
    batch.bzbot.upload(inp["bzbot"])
    batch._flags_host |= np.where(inp["has_bzbot"], _lib.PM_COL_BZBOT, 0).astype(np.int32)
    batch.use_hints(uniform_area=case.ua, div3=case.div3)  # (uploads the flags)
    assert batch.uniform_area and (batch.div3_proven or not (case.ua and case.div3))
    batch.nonfinite.upload(np.full(N, 2, dtype=np.int32))  # stale marks: every flag must be written
    self.b = batch.b
    if case.b_shift:
      self.b = _Rows(gpu, N, nz, True, inp["b0"])
      self.owned.append(self.b)
    self.desc = batch.descriptor()
    self.desc.b = self.b.ptr
    wA = _Rows(gpu, N, nz, case.w_shift and not case.precombined, inp["wA"])
    self.owned.append(wA)
    self.forcing = wA
    if case.precombined:
      self.forcing = _Rows(gpu, N, nz, case.w_shift)
      self.owned.append(self.forcing)
      batch.combine_forcing(wA.mem, out=self.forcing)
    self.vdx = self.b_in = None
    if case.horadv:
      self.vdx, self.b_in = _Rows(gpu, N, nz, False, inp["vdx"]), _Rows(gpu, N, nz, False, inp["b_in"])
      self.owned += [self.vdx, self.b_in]
    self.ops = op_bits(case)

  def _args(self):
    return (C.byref(self.desc), self.forcing.ptr, self.vdx.ptr if self.vdx else None)

  def kernel_name(self, nsteps):
    from pymoc_amd._lib import check, lib
    buf = C.create_string_buffer(96)
    check(lib.pm_column_kernel_name(*self._args(), int(nsteps), self.ops, self.case.lanes, buf, 96))
    return buf.value.decode()

  def steps(self, nsteps):
    from pymoc_amd._lib import check, lib
    check(lib.pm_column_steps(*self._args(), self.b_in.ptr if self.b_in else None, self.dt,
                              int(nsteps), self.ops, self.case.lanes, None))

  def get_b(self):
    if self.b is self.batch.b:
      return self.batch.get_b()
    return self.b.download()

  def get_nonfinite(self):
    return self.batch.get_nonfinite()

  def forcing_row(self, m):
    return self.forcing.download(m, 1)[0]

  def free(self):
    for a in self.owned:
      a.free()
    for a in list(vars(self.batch).values()):
      if hasattr(a, "free") and hasattr(a, "ptr"):
        a.free()
    self.owned, self.batch = [], None
