"""What the GPU tests of the three series modules (test_stats_gpu, test_spectra_gpu,
test_windows_gpu) share: the bit-for-bit comparison, a series inside a larger allocation,
sentinel-filled outputs with elements to spare behind them."""
import numpy as np

V_SENTINEL, I_SENTINEL = -7.25, -77
PAD = 97    # doubles on either side of the series inside its allocation
SPARE = 33  # elements behind every output


def _bits(got, want, what, zero_sign=True):
  """Bit for bit, NaN <-> NaN (any payload), signed zeros as they are; zero_sign=False: -0.0 and
  +0.0 are the same."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  gn, wn = np.isnan(got), np.isnan(want)
  assert np.array_equal(gn, wn), (what, "NaN pattern", np.argwhere(gn != wn)[:5])
  same = got.view(np.uint64) == want.view(np.uint64)
  if not zero_sign:
    same |= (got == 0.0) & (want == 0.0)
  bad = np.argwhere(~(same | gn))
  assert bad.size == 0, (what, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def _up(gpu, a):
  return gpu.DeviceArray.from_host(a, dtype=a.dtype)


def _padded(gpu, v):
  """(allocation, address of the series' first value): the series inside a larger allocation.  The
  padding alternates NaN with 7e30: every series kernel skips a NaN by definition (a member, a
  segment or a window that holds one is excluded), so of a read outside the series it is the
  finite half that shows."""
  v = np.ascontiguousarray(v, dtype=np.float64)
  buf = np.full(v.size + 2 * PAD, np.nan)
  buf[0:PAD:2] = 7e30
  buf[PAD + v.size::2] = 7e30
  buf[PAD:PAD + v.size] = v.ravel()
  dev = gpu.DeviceArray.from_host(buf)
  return dev, dev.ptr + 8 * PAD


def _out(gpu, shape, dtype, sentinel):
  """A sentinel-filled device output of `shape` with SPARE elements behind it, and its size."""
  size = int(np.prod(shape))
  return _up(gpu, np.full(size + SPARE, sentinel, dtype=dtype)), size


def _collect(out, shapes, what):
  """{key: the downloaded output in its shape} of out = {key: _out(...)}, shapes = {key: (shape,
  dtype, sentinel)}; nothing behind an output's last element is touched."""
  res = {}
  for k, (dev, size) in out.items():
    flat = dev.download().ravel()
    assert (flat[size:] == shapes[k][2]).all(), (what, k, "behind the output")
    res[k] = flat[:size].reshape(shapes[k][0])
  return res
