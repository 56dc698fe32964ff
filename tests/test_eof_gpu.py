"""pm_series_scatter, pm_series_eof, pm_series_project and SeriesEOF on the device: every case of
tests/eof_cases.py through the C-ABI -- all outputs of the three entries bit for bit against the
restatement -- what the launches leave alone, independence of a member from the batch, of a record
window from the series around it and of the fit from the order of `sel`, a pooled unit against the
host sum of the device's scatters, the class against the entries, SeriesWindows on the principal
component, and the launches."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _collect, _out, _padded, _up
import eof_cases as EC
import windows_cases as WC

pytestmark = pytest.mark.gpu

F, I = (np.float64, V_SENTINEL), (np.int32, I_SENTINEL)


def run(gpu, c, v=None, k0=None, k1=None, sel=None, w="case"):
  """The three entries of the case's settings (on another series / record window / sel / weights
  if given), each into sentinel-filled outputs and each reading the device outputs of the one
  before; nothing behind an output's last element is touched."""
  from pymoc_amd import _lib
  v = c["v"] if v is None else v
  k0, k1 = (c["k0"], c["k1"]) if k0 is None else (k0, k1)
  sel = c["sel"] if sel is None else sel
  w = c["w"] if isinstance(w, str) else w
  nrec, nspec, n = v.shape
  q, K = len(sel), k1 - k0
  grouped = c["order"] is not None and n == c["v"].shape[2]
  nu = len(c["start"]) - 1 if grouped else n
  series, v_ptr = _padded(gpu, v)
  w_dev = None if w is None else _up(gpu, np.ascontiguousarray(w, dtype=np.float64))
  shapes = dict(nused=((n,),) + I, mean=((q, n),) + F, scat=((q * (q + 1) // 2, n),) + F,
                eof=((q, nu),) + F, lam=((nu,),) + F, trace=((nu,),) + F, resid=((nu,),) + F,
                vv=((nu,),) + F, ntot=((nu,),) + I, pc=((K, 1, n),) + F)
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  p = {k: a[0].ptr for k, a in out.items()}
  d = _lib.pm_series_scatter()
  d.n, d.nspec, d.nrec, d.k0, d.k1, d.q = n, nspec, nrec, k0, k1, q
  d.v, d.w = v_ptr, None if w_dev is None else w_dev.ptr
  d.sel[:q] = [int(s) for s in sel]
  _lib.check(_lib.lib.pm_series_scatter(C.byref(d), p["nused"], p["mean"], p["scat"], None))
  e = _lib.pm_series_eof()
  e.n, e.q, e.nu, e.iters, e.nused, e.scat = n, q, nu, c["iters"], p["nused"], p["scat"]
  keep = []
  if grouped:
    keep = [_up(gpu, c["order"]), _up(gpu, c["start"]),
            _up(gpu, EC.unit_of(c["order"], c["start"], n))]
    e.order, e.start, e.start_dev = keep[0].ptr, c["start"].ctypes.data, keep[1].ptr
  _lib.check(_lib.lib.pm_series_eof(C.byref(e), p["eof"], p["lam"], p["trace"], p["resid"],
                                    p["vv"], p["ntot"], None))
  j = _lib.pm_series_project()
  j.n, j.nspec, j.nrec, j.k0, j.k1, j.q, j.nu = n, nspec, nrec, k0, k1, q, nu
  j.v, j.w, j.nused, j.mean, j.eof = v_ptr, d.w, p["nused"], p["mean"], p["eof"]
  j.unit = keep[2].ptr if grouped else None
  j.sel[:q] = [int(s) for s in sel]
  _lib.check(_lib.lib.pm_series_project(C.byref(j), p["pc"], None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


CASES = EC.cases()
IDS = [c["name"] for c in CASES]
KEYS = ("nused", "mean", "scat", "eof", "lam", "trace", "resid", "vv", "ntot", "pc")
WIDE = [c for c in CASES if c["v"].shape[2] == 37]


@pytest.fixture(scope="module")
def results(gpu):
  """name -> (the device result, the restatement) of the case: computed once, shared, left
  unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = (run(gpu, c), EC.restate(c))
    return cache[c["name"]]
  return get


def _same(got, want, what, keys=KEYS):
  for k in keys:
    if np.asarray(want[k]).dtype.kind == "i":
      assert np.array_equal(got[k], want[k]), (what, k)
    else:
      _bits(got[k], want[k], (what, k))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_output_bit_for_bit(gpu, results, case):
  """All ten outputs of the three entries equal the restatement bit for bit: the NaN patterns (an
  unused record, a member with fewer than 2 used records, a unit of skipped members, a trace of 0,
  the overflow of `huge`), signed zeros, the near-degenerate pair.  The series sits inside a
  padded allocation between records of 7e30 and -3e30 that belong to it but not to the window: a
  read outside the window would show.  The window copied out as a series of its own gives the
  same bits."""
  c = case
  got, want = results(c)
  _same(got, want, c["name"])
  own = run(gpu, c, v=np.ascontiguousarray(c["v"][c["k0"]:c["k1"]]), k0=0, k1=c["k1"] - c["k0"])
  _same(own, got, (c["name"], "own series"))


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_a_member_does_not_depend_on_the_batch(gpu, results, case):
  """Per-member units: a shard (members 5 .. 20 of 37) and a single member give the bits they have
  in the batch."""
  c, (whole, _) = case, results(case)
  assert c["order"] is None
  for m0, m1 in ((5, 21), (9, 10)):
    w = None if c["w"] is None else c["w"][:, m0:m1]
    part = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, m0:m1]), w=w)
    for k in KEYS:
      _bits(part[k], whole[k][..., m0:m1], (c["name"], k, "members [%d, %d)" % (m0, m1)))


def test_sel_permuted(gpu, results):
  """sel permuted: nused is bitwise the same, mean and scat are bitwise the correspondingly
  permuted ones (a product commutes, and every sum runs over the records), and the fit equals the
  restatement of the permuted case bit for bit.  The eof itself is the permuted one up to the
  rounding of its matrix-vector sums, which run in another order: on the `modes` members within
  the bound of test_eof_cpu."""
  import test_eof_cpu as TC
  c = CASES[0]
  got, _ = results(c)
  q, n = len(c["sel"]), c["v"].shape[2]
  perm = np.random.default_rng(5).permutation(q)
  assert (perm != np.arange(q)).any()
  pc = dict(c, sel=c["sel"][perm], name="permuted")
  other = run(gpu, pc)
  _same(other, EC.restate(pc), "permuted")
  assert np.array_equal(other["nused"], got["nused"])
  _bits(other["mean"], got["mean"][perm], "mean")
  I_, J_ = EC.tri(q)
  entry = {(i, j): e for e, (i, j) in enumerate(zip(I_, J_))}
  src = [entry[(max(perm[i], perm[j]), min(perm[i], perm[j]))] for i, j in zip(I_, J_)]
  _bits(other["scat"], got["scat"][src], "scat")
  checked = 0
  for m in range(n):
    if EC.style_of(m) != "modes":
      continue
    Cm = np.zeros((q, q))
    Cm[I_, J_] = Cm[J_, I_] = got["scat"][:, m] / got["nused"][m]
    bound = TC.bound(Cm, c["iters"])
    assert np.abs(other["eof"][:, m] - got["eof"][perm, m]).max() <= 2.0 * bound, m
    checked += 1
  assert checked >= 5


def test_a_pooled_unit_is_the_host_sum_of_the_scatters(gpu, results):
  """A pooled unit equals the device's per-member scatters summed on the host in the stated order
  and then solved by the restatement."""
  for c in (c for c in CASES if c["order"] is not None):
    got, _ = results(c)
    want = EC.solve(*EC.pool(got["nused"], got["scat"], c["order"], c["start"]), len(c["sel"]),
                    c["iters"])
    _same(got, want, c["name"], ("eof", "lam", "trace", "resid", "vv", "ntot"))
    sizes = np.diff(c["start"]).tolist()
    assert sorted(sizes) == [1, 2, 27, 40] and (got["ntot"] == 0).any()


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_eof_cpu as TC
  fl = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(5)]
  it = [_up(gpu, np.full(4096, I_SENTINEL, dtype=np.int32)) for _ in range(2)]
  L = _lib.lib
  for label, kw in TC.bad_scatter():
    d = TC.sdesc(**kw)
    assert L.pm_series_scatter(C.byref(d), it[0].ptr, fl[0].ptr, fl[1].ptr, None) == _lib.PM_EINVAL, label
  for label, kw in TC.bad_eof():
    d = TC.edesc(**kw)
    assert (L.pm_series_eof(C.byref(d), *([a.ptr for a in fl] + [it[1].ptr, None]))
            == _lib.PM_EINVAL), label
  for label, kw in TC.bad_project():
    d = TC.pdesc(**kw)
    assert L.pm_series_project(C.byref(d), fl[0].ptr, None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in fl:
    assert (a.download() == V_SENTINEL).all()
  for a in it:
    assert (a.download() == I_SENTINEL).all()


# ------------------------------------------------------------------ SeriesEOF
def _names(nspec):
  return ["i%d" % s for s in range(nspec)]


@pytest.mark.parametrize("ci", (1, 7, 8), ids=lambda ci: IDS[ci])
def test_the_class_equals_the_entries(gpu, results, ci):
  """compute() of the class -- weights as an array, per member and pooled -- returns the bits of
  the entries composed, in the documented shapes; fit() the same without pc; pc() the device
  series."""
  c = CASES[ci]
  got, _ = results(c)
  nrec, nspec, n = c["v"].shape
  names = _names(nspec)
  dev = gpu.DeviceArray.from_host(c["v"])
  kw = dict(groups=c["labels"], pooled=True) if c["order"] is not None else {}
  se = gpu.SeriesEOF((dev, names), indices=[names[s] for s in c["sel"]], iters=c["iters"],
                     scale="none" if c["w"] is None else c["w"], **kw)
  r = se.compute(c["k0"], c["k1"])
  K = c["k1"] - c["k0"]
  assert r.pc.shape == (n, K) and r.lam.shape == (se.nu,)
  _bits(r.pc, got["pc"][:, 0, :].T, "pc")
  for j, s in enumerate(c["sel"]):
    _bits(r.eof[names[s]], got["eof"][j], ("eof", j))
  for k in ("lam", "trace", "resid", "vv"):
    _bits(getattr(r, k), got[k], k)
  with np.errstate(all="ignore"):
    _bits(r.frac, got["lam"] / got["trace"], "frac")
  assert np.array_equal(r.nused, got["nused"]) and np.array_equal(r.ntot, got["ntot"])
  if c["order"] is not None:
    assert np.array_equal(r.unit, EC.unit_of(c["order"], c["start"], n))
    assert r.labels.tolist() == sorted(set(c["labels"].tolist()))
  f = se.fit(c["k0"], c["k1"])
  assert not hasattr(f, "pc")
  _bits(f.lam, got["lam"], "fit lam")
  y, ynames = se.pc(c["k0"], c["k1"])
  assert ynames == ["pc1"] and y.shape == (K, 1, n)
  _bits(gpu.DeviceArray.download(y._parent), got["pc"], "pc()")


def test_scale_std(gpu):
  """scale="std": the weights are 1 / sqrt(var) of SeriesStats.along_time, 0 for a var that is 0
  or not finite, shared by a pooled unit as the mean of its finite variances; the fit is the
  entries' with those weights."""
  from pymoc_amd.eof import std_weights
  c = CASES[7]
  nrec, nspec, n = c["v"].shape
  names = _names(nspec)
  dev = gpu.DeviceArray.from_host(c["v"])
  ind = [names[s] for s in c["sel"]]
  st = gpu.SeriesStats((dev, names)).along_time(c["k0"], c["k1"])
  var = np.stack([st.var[nm] for nm in ind])
  for kw, w in ((dict(), std_weights(var)),
                (dict(groups=c["labels"], pooled=True), std_weights(var, c["order"], c["start"]))):
    assert np.isfinite(w).all() and (w == 0.0).any() and (w > 0.0).any()
    r = gpu.SeriesEOF((dev, names), indices=ind, scale="std", **kw).compute(c["k0"], c["k1"])
    raw = run(gpu, dict(c, order=c["order"] if kw else None), w=w)
    _bits(r.pc, raw["pc"][:, 0, :].T, "pc")
    _bits(r.lam, raw["lam"], "lam")
  for u in range(len(c["start"]) - 1):
    mem = c["order"][c["start"][u]:c["start"][u + 1]]
    assert (w[:, mem] == w[:, mem[:1]]).all()


WP, SP = 24, 3


class _Recorder(object):
  """What a Series* class reads off an IndexRecorder, around a plain device series: a launch timer
  without an ensemble run."""

  class _E(object):
    stream = None
    _member0 = 0

  def __init__(self, values, names, timer):
    self._values, self.ens = values, self._E()
    self.table = type("T", (), dict(names=names))()
    self.ens.timer = timer
    self.steps = np.arange(values.shape[0]) * 12


def test_series_windows_on_the_principal_component_and_the_launches(gpu):
  """SeriesWindows(SeriesEOF(...).pc(), W).compute() and .trend() equal the restated composition
  (windows_cases) on the device's pc series exactly.  The launch spans the timer records are the
  three new kernels and nothing else new; a SeriesWindows on the original source records the spans
  it recorded before."""
  from pymoc_amd.device import LaunchTimer
  c = CASES[0]
  nrec, nspec, n = c["v"].shape
  names = _names(nspec)
  timer = LaunchTimer()
  rec = _Recorder(gpu.DeviceArray.from_host(c["v"]), names, timer)

  def spans_of(call):
    before = len(timer.spans)
    res = call()
    return res, [name for name, _, _ in timer.spans[before:]]

  se = gpu.SeriesEOF(rec, indices=[names[s] for s in c["sel"]], iters=c["iters"])
  _, spans = spans_of(lambda: se.fit(c["k0"], c["k1"]))
  assert spans == ["k_series_scatter", "k_series_eof"]
  src, spans = spans_of(lambda: se.pc(c["k0"], c["k1"]))
  assert spans == ["k_series_scatter", "k_series_eof", "k_series_project"]
  r, spans = spans_of(lambda: se.compute(c["k0"], c["k1"]))
  assert spans == ["k_series_scatter", "k_series_eof", "k_series_project"]
  _, spans = spans_of(lambda: gpu.SeriesEOF(rec, indices=names[:2], scale="std").fit(c["k0"], c["k1"]))
  assert spans == ["k_series_member_stats", "k_series_scatter", "k_series_eof"]
  sw = gpu.SeriesWindows(rec, WP, step=SP)
  _, spans = spans_of(lambda: sw.compute(c["k0"], c["k1"]))
  assert spans == ["k_series_windows"]
  _, spans = spans_of(lambda: sw.trend(c["k0"], c["k1"]))
  assert spans == ["k_series_windows", "k_series_kendall", "k_series_kendall"]

  pcs = r.pc.T[:, None, :]                         # the device's pc series [K, 1, n]
  K = pcs.shape[0]
  assert np.isfinite(pcs).any() and np.isnan(pcs).any()
  on = gpu.SeriesWindows(src, WP, step=SP, detrend="linear")
  wr, tr = on.compute(), on.trend()
  want = WC.windows(pcs, 0, K, WP, SP, 1, "linear")
  for i, key in enumerate(("mean", "slope", "var", "ac")):
    _bits(getattr(wr, key)["pc1"], want["out"][i][:, 0, :].T, key)
  assert np.array_equal(wr.nused["pc1"], want["nused"][0])
  nwin = want["out"].shape[1]
  for key, plane in (("var", 2), ("ac", 3)):
    k = WC.kendall(want["out"][plane], 0, nwin)
    t = getattr(tr, key)
    for f, w in zip(("conc", "disc", "tie", "nfin"), k):
      assert np.array_equal(getattr(t, f)["pc1"], w[0]), (key, f)
    _bits(t.tau["pc1"], WC.tau_b(k[0][0], k[1][0], k[2][0]), (key, "tau"))
