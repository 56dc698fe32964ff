"""The NumPy restatement of pymoc_amd.NoiseForcing (include/pymoc_hip.h states the definition):
the authority tests/test_noise_cpu.py and tests/test_noise_gpu.py check the device against.
Pure NumPy; nothing here imports the product."""
import numpy as np

STREAMS = ("bs", "bs_north", "tau", "b_rest", "surflux", "bs_SO")
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
S32 = np.uint64(32)
EPS = 2.0**-53


def philox4x32_10(counter, key):
  """Philox4x32-10: `counter` four and `key` two uint32 words (scalars or arrays that broadcast);
  returns the four output words as uint64 arrays holding 32-bit values."""
  c = [np.asarray(w, dtype=np.uint64) & MASK for w in np.broadcast_arrays(*counter)]
  k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
  for _ in range(10):
    p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow
    c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1),
         p0 & MASK]
    k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
  return c


def words(seed, ids, j, stream):
  """r0..r3 of (seed, id, j, stream); ids / j may be arrays that broadcast."""
  seed = int(seed)
  ids = np.asarray(ids, dtype=np.uint64)
  return philox4x32_10((ids & MASK, ids >> S32, np.asarray(j, dtype=np.uint64),
                        np.uint64(int(stream))), (seed & 0xffffffff, seed >> 32))


def uniforms(seed, ids, j, stream):
  """(d1, d2), multiples of 2^-53 in [0, 1): exact."""
  r = words(seed, ids, j, stream)
  S5, S6 = np.uint64(5), np.uint64(6)
  d1 = ((r[0] >> S5).astype(np.float64) * 67108864.0 + (r[1] >> S6).astype(np.float64)) * EPS
  d2 = ((r[2] >> S5).astype(np.float64) * 67108864.0 + (r[3] >> S6).astype(np.float64)) * EPS
  return d1, d2


def deviate(seed, ids, j, stream):
  """(xi, R): the standard normal deviate and its radius."""
  d1, d2 = uniforms(seed, ids, j, stream)
  R = np.sqrt(-2.0 * np.log(1.0 - d1))
  return R * np.cos(6.283185307179586 * d2), R


def application(s, M, phase, dt):
  """(j, model time since the previous application) at loop iteration s, or None when forcing is
  not applied there: applied at s = 0 and at s = phase (mod M); j counts those instants."""
  instants = [q for q in range(s + 1) if q == 0 or q % M == phase % M]
  if not instants or instants[-1] != s:
    return None
  j = len(instants) - 1
  return j, (float(s - instants[-2]) * dt if j else 0.0)


def ar1(tau_corr, elapsed):
  if tau_corr == 0:
    return 0.0, 1.0
  if np.isinf(tau_corr):
    return 1.0, 0.0
  a = np.exp(-np.float64(elapsed) / np.float64(tau_corr))
  return float(a), float(np.sqrt(1.0 - a * a))


def series(seed, name, sigma, tau_corr, ids, steps, M, phase, dt, x0=None):
  """The noise state of target `name` at every application among loop iterations `steps`
  (increasing): (x [J, n], R [J, n]).  The first application starts stationary, x = sigma * xi,
  unless `x0` gives the state it advances."""
  ids = np.asarray(ids, dtype=np.uint64)
  sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), ids.shape)
  x = np.zeros(ids.size) if x0 is None else np.asarray(x0, dtype=np.float64)
  live = x0 is not None
  xs, Rs = [], []
  for s in steps:
    j, elapsed = application(s, M, phase, dt)
    a, b = ar1(tau_corr, elapsed) if live else (0.0, 1.0)
    xi, R = deviate(seed, ids, j, STREAMS.index(name))
    x = a * x + (sigma * b) * xi
    live = True
    xs.append(x)
    Rs.append(R)
  return np.array(xs), np.array(Rs)


def written(base, x, pattern=None):
  """base [n, len] + x [n] * pattern ([len], [n, len] or None), uncontracted."""
  base = np.asarray(base, dtype=np.float64)
  if base.ndim == 1:
    base = base[:, None]
  if pattern is None:
    return base + x[:, None]
  return base + x[:, None] * np.asarray(pattern, dtype=np.float64)


def series_bound(j, sigma, Rmax, Xmax):
  """E_j = (j + 1) * 2^-53 * (16 sigma R* + 4 X*): one deviate error (16 * 2^-53 * R, scaled by
  sigma b <= sigma) and two roundings (<= 2 half-ulps of |x| each way, 4 * 2^-53 X* with room) per
  application, damped by a <= 1 from one application to the next."""
  return (j + 1) * EPS * (16.0 * sigma * Rmax + 4.0 * Xmax)
