"""pm_series_spectra and SeriesSpectra on the device: every case of tests/spectra_cases.py through
the C-ABI bit for bit against the restatement, what the launch leaves alone, independence of a
member from its neighbours and from the batch, the pair jobs against the auto spectra,
across_members against SeriesStats, a recorded noise ensemble, and the launches of a run without
SeriesSpectra."""
import ctypes as C

import numpy as np
import pytest

from series_harness import I_SENTINEL, V_SENTINEL, _bits, _collect, _out, _padded, _up
import spectra_cases as SC

pytestmark = pytest.mark.gpu

def run(gpu, c, v=None, pairs=None):
  """One launch of the case's settings (on another series / other pairs if given) into
  sentinel-filled outputs; nothing behind an output's last element is touched."""
  from pymoc_amd import _lib
  from pymoc_amd.spectra import twiddles
  v = c["v"] if v is None else v
  pairs = c["pairs"] if pairs is None else pairs
  nrec, nspec, n = v.shape
  L, nf, npairs = c["L"], c["L"] // 2 + 1, len(pairs)
  series, v_ptr = _padded(gpu, v)
  w = np.ascontiguousarray(c["w"], dtype=np.float64)
  pr = np.ascontiguousarray(pairs if npairs else [[0, 0]], dtype=np.int32)
  d_w, d_tw, d_pr = _up(gpu, w), _up(gpu, twiddles(L)), _up(gpu, pr)
  shapes = dict(nused=((nspec, n), np.int32, I_SENTINEL), psd=((nf, nspec, n), np.float64, V_SENTINEL),
                nused_pair=((npairs, n), np.int32, I_SENTINEL),
                csd=((nf, 2 * npairs, n), np.float64, V_SENTINEL))
  out = {k: _out(gpu, *a) for k, a in shapes.items()}
  d = _lib.pm_series_spectra()
  d.n, d.nspec, d.nrec, d.k0, d.k1 = n, nspec, nrec, c["k0"], c["k1"]
  d.nperseg, d.step, d.npairs = L, L - c["noverlap"], npairs
  d.detrend = dict(constant=_lib.PM_SPEC_DETREND_CONSTANT, none=_lib.PM_SPEC_DETREND_NONE)[c["detrend"]]
  d.v, d.window, d.window_dev, d.twiddle = v_ptr, w.ctypes.data, d_w.ptr, d_tw.ptr
  d.pair, d.pair_dev, d.scale = pr.ctypes.data, d_pr.ptr, c["scale"]
  ptr = lambda k: out[k][0].ptr if (npairs or k in ("nused", "psd")) else None  # noqa: E731
  _lib.check(_lib.lib.pm_series_spectra(C.byref(d), ptr("nused"), ptr("psd"), ptr("nused_pair"),
                                        ptr("csd"), None))
  gpu.synchronize()
  return _collect(out, shapes, c["name"])


def _same(got, want, what):
  assert np.array_equal(got["nused"], want["nused"]), (what, "nused")
  assert np.array_equal(got["nused_pair"], want["nused_pair"]), (what, "nused_pair")
  _bits(got["psd"], want["psd"], (what, "psd"))
  _bits(got["csd"], want["csd"], (what, "csd"), zero_sign=False)


CASES = SC.cases()
IDS = [c["name"] for c in CASES]
WIDE = [c for c in CASES if c["v"].shape[2] == 65]


@pytest.fixture(scope="module")
def results(gpu):
  """name -> the device result of the case: computed once, shared, left unchanged."""
  cache = {}

  def get(c):
    if c["name"] not in cache:
      cache[c["name"]] = run(gpu, c)
    return cache[c["name"]]
  return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spectra_bit_for_bit(gpu, results, case):
  got, want = results(case), SC.restate(case)
  _same(got, want, case["name"])
  assert np.array_equal(np.isnan(got["psd"][0]), want["nused"] == 0)
  # the styles did what they are for: some segments excluded, some members without any
  if case["v"].shape[2] >= 7 and case["nseg"] > 1:
    nu = got["nused"]
    assert (nu == case["nseg"]).any() and (nu == case["nseg"] - 1).any() and (nu == 0).any()


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_a_member_does_not_depend_on_its_neighbours_or_the_batch(gpu, results, case):
  c, whole = case, results(case)
  # the same series in every member: the same bits in every member
  v = np.repeat(c["v"][:, :, 5:6], 65, axis=2)  # (member 5: styles nan1, red, big)
  r = run(gpu, c, v=v)
  for k in ("nused", "nused_pair"):
    assert (r[k] == r[k][..., :1]).all(), (c["name"], k)
  for k in ("psd", "csd"):
    _bits(r[k], np.repeat(r[k][..., :1], 65, axis=2), (c["name"], k, "copies"))
  for k in ("nused", "nused_pair", "psd", "csd"):
    _bits(r[k][..., 0], whole[k][..., 5], (c["name"], k, "member 5 among others"))
  # a shard: members [9, 41) as a series of their own
  part = run(gpu, c, v=np.ascontiguousarray(c["v"][:, :, 9:41]))
  for k in ("nused", "nused_pair", "psd", "csd"):
    _bits(part[k], whole[k][..., 9:41], (c["name"], k, "shard"))
  # without pairs, and with one: the spectra do not move
  r0 = run(gpu, c, pairs=())
  assert np.array_equal(r0["nused"], whole["nused"])
  _bits(r0["psd"], whole["psd"], (c["name"], "no pairs"))
  if c["pairs"]:
    r1 = run(gpu, c, pairs=((2, 0),))
    _bits(r1["psd"], whole["psd"], (c["name"], "one pair"))
    _bits(r1["csd"], whole["csd"][:, 2:4], (c["name"], "the pair alone"))


@pytest.mark.parametrize("case", [c for c in CASES if c["pairs"]],
                         ids=[c["name"] for c in CASES if c["pairs"]])
def test_a_pair_job_transforms_as_the_auto_spectra_do(gpu, results, case):
  """csd[(1, 1)] is conj(Z1) * Z1 of the pair job's own transforms: its real part is psd[1] bit for
  bit -- the one-sided factor (1 or 2, exact) on both -- and its imaginary part exactly 0.
  (0, 2) and (2, 0) are conjugates."""
  r = results(case)
  assert tuple(case["pairs"]) == ((0, 2), (2, 0), (1, 1))
  assert np.array_equal(r["nused_pair"][2], r["nused"][1])
  _bits(r["csd"][:, 4], r["psd"][:, 1], (case["name"], "re (1, 1)"))
  c = np.full(case["L"] // 2 + 1, 2.0)
  c[0] = c[-1] = 1.0
  _bits(r["csd"][:, 4] / c[:, None], r["psd"][:, 1] / c[:, None], (case["name"], "before c"))
  im = r["csd"][:, 5]
  assert ((im == 0.0) | np.isnan(im)).all() and np.array_equal(np.isnan(im), np.isnan(r["csd"][:, 4]))
  assert np.array_equal(r["nused_pair"][0], r["nused_pair"][1])
  _bits(r["csd"][:, 2], r["csd"][:, 0], (case["name"], "re (2, 0)"), zero_sign=False)
  _bits(r["csd"][:, 3], -r["csd"][:, 1], (case["name"], "im (2, 0)"), zero_sign=False)


def test_bad_descriptors_leave_the_outputs_untouched(gpu):
  from pymoc_amd import _lib
  import test_spectra_cpu as TC
  keep = []
  out = [_up(gpu, np.full(4096, V_SENTINEL)) for _ in range(4)]
  for label, kw in TC.bad_descriptors():
    d = TC.desc(keep, **kw)
    assert _lib.lib.pm_series_spectra(C.byref(d), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                      None) == _lib.PM_EINVAL, label
  gpu.synchronize()
  for a in out:
    assert (a.download() == V_SENTINEL).all()


# ------------------------------------------------------------------ SeriesSpectra
def test_series_spectra_on_a_plain_device_series(gpu):
  """(DeviceArray, names) as source: compute() against the restatement, coherence and phase, and
  across_members against SeriesStats on an uploaded copy of the downloaded spectra."""
  c = next(c for c in CASES if c["L"] == 256)
  v, names = c["v"], ["wind", "amoc", "depth"]
  pairs = [("wind", "depth"), ("depth", "wind"), ("amoc", "amoc")]
  labels = np.array([40, -3, 7])[np.arange(65) % 3]
  sp = gpu.SeriesSpectra((gpu.DeviceArray.from_host(v), names), 256, window="hann", pairs=pairs,
                         dt_record=c["dt"], groups=labels)
  assert sp.scale == c["scale"] and sp.nseg(c["k0"], c["k1"]) == c["nseg"]
  r, want = sp.compute(c["k0"], c["k1"]), SC.restate(c)
  assert np.array_equal(r.freq, np.arange(129) / (256 * c["dt"]))
  for s, nm in enumerate(names):
    assert r.psd[nm].shape == (65, 129) and np.array_equal(r.nused[nm], want["nused"][s])
    _bits(r.psd[nm], want["psd"][:, s].T, nm)
  for p, pr in enumerate(pairs):
    assert np.array_equal(r.nused_pair[pr], want["nused_pair"][p])
    _bits(r.csd[pr].real, want["csd"][:, 2 * p].T, pr, zero_sign=False)
    _bits(r.csd[pr].imag, want["csd"][:, 2 * p + 1].T, pr, zero_sign=False)
    a, b = (names.index(x) for x in pr)
    same = (want["nused_pair"][p] > 0) & (want["nused"][a] == want["nused_pair"][p]) & (
        want["nused"][b] == want["nused_pair"][p])
    # (a constant series has a spectrum of rounding residue or exactly 0: no coherence to speak of)
    live = same & np.array([SC.style_of(a, m) != "const" and SC.style_of(b, m) != "const"
                            for m in range(65)])
    coh = r.coherence[pr]
    assert np.isnan(coh[~same]).all() and np.isfinite(coh[live]).all(), pr
    assert live.any() and (~same).any()
    assert (coh[live] >= 0).all() and (coh[live] <= 1 + 1e-12).all(), pr
    assert np.array_equal(r.phase[pr][live], np.angle(r.csd[pr])[live])
    if a == b:
      assert np.allclose(coh[live], 1.0, rtol=1e-14, atol=0) and not r.phase[pr][live].any()
  # across members: the device spectra as a series [nf][nspec][n] through SeriesStats
  q = (0.05, 0.5, 0.95)
  across = sp.across_members(c["k0"], c["k1"], quantiles=q)
  assert sp.group_labels.tolist() == [-3, 7, 40]
  host = gpu.SeriesStats((gpu.DeviceArray.from_host(want["psd"]), names), groups=labels,
                         quantiles=q).across_members()
  for nm in names:
    assert across.mean[nm].shape == (3, 129) and across.quantile[nm].shape == (3, 3, 129)
    assert np.array_equal(across.count[nm], host.count[nm])
    for key in ("mean", "var", "min", "max", "sum", "quantile"):
      _bits(getattr(across, key)[nm], getattr(host, key)[nm], (nm, key))
  # members without a used segment are excluded and counted
  groups_of = [np.nonzero(labels == g)[0] for g in (-3, 7, 40)]
  for s, nm in enumerate(names):
    cnt = [int((want["nused"][s][g] > 0).sum()) for g in groups_of]
    assert (across.count[nm] == np.array(cnt)[:, None]).all() and min(cnt) < min(map(len, groups_of))


def test_series_spectra_on_a_recorded_noise_ensemble(gpu):
  """An IndexRecorder on a 16-member JN2018Ensemble under NoiseForcing: the recorder route, the
  (array, names) route on its series and the restatement on the downloaded series agree bit for
  bit; the run issued no launch of this module before compute(), and compute() adds its one."""
  import test_stats_gpu as TG
  from pymoc_amd.spectra import twiddles
  ens, rec = TG._recorded(gpu, TG._cfg16(), timer=True)
  before = [name for name, _, _ in ens.timer.spans]
  assert before.count("k_row_indices") == TG.N_SAMPLES
  assert not [name for name in before if "spectra" in name or "series" in name]
  pairs = [("amoc", "b_1000")]
  sp = gpu.SeriesSpectra(rec, 8, pairs=pairs, dt_record=1.0, groups=TG.GROUPS)
  with pytest.raises(ValueError, match="record %d, which was never written" % TG.N_SAMPLES):
    sp.compute()
  r = sp.compute(2, TG.N_SAMPLES)
  after = [name for name, _, _ in ens.timer.spans]
  assert after[:len(before)] == before and after[len(before):] == ["k_series_spectra"]
  v = TG._series_of(rec)
  assert np.isfinite(v[:TG.N_SAMPLES]).all()
  want = SC.spectra(v, 2, TG.N_SAMPLES, 8, 4, sp.window, "constant", ((0, 1),), sp.scale,
                    twiddles(8))
  nseg = (TG.N_SAMPLES - 2 - 8) // 4 + 1
  plain = gpu.SeriesSpectra((gpu.DeviceArray.from_host(v), list(rec.table.names)), 8, pairs=pairs,
                            groups=TG.GROUPS).compute(2, TG.N_SAMPLES)
  for s, nm in enumerate(rec.table.names):
    assert (r.nused[nm] == nseg).all() and np.array_equal(plain.nused[nm], r.nused[nm])
    _bits(r.psd[nm], want["psd"][:, s].T, nm)
    _bits(plain.psd[nm], r.psd[nm], (nm, "plain"))
    assert (r.psd[nm][:, 1:] > 0).all()  # the noise acts: every member varies
  _bits(r.csd[pairs[0]].real, want["csd"][:, 0].T, "csd re", zero_sign=False)
  _bits(r.csd[pairs[0]].imag, want["csd"][:, 1].T, "csd im", zero_sign=False)
  _bits(plain.csd[pairs[0]].real, r.csd[pairs[0]].real, "plain csd re")
  _bits(plain.csd[pairs[0]].imag, r.csd[pairs[0]].imag, "plain csd im")
  coh = r.coherence[pairs[0]]
  assert np.isfinite(coh).all() and (coh >= 0).all() and (coh <= 1 + 1e-12).all()
  across = sp.across_members(2, TG.N_SAMPLES, quantiles=(0.05, 0.95))
  assert (across.count["amoc"] == 4).all() and across.mean["amoc"].shape == (4, 5)
  assert (across.quantile["amoc"][0] <= across.mean["amoc"]).all()
  assert (across.mean["amoc"] <= across.quantile["amoc"][1]).all()
