// exact_div.hip -- what licenses the kernels' short exact quotients: the host proofs per
// denominator (div_proof.h) behind pm_div3_proven / pm_div2_proven, the checks that the device
// forms the reciprocals those proofs assume, and the device self tests of every division form of
// common.hip.h against IEEE `/`.
#include <initializer_list>
#include <vector>
#include "common.hip.h"
#include "div_proof.h"

namespace pm {

// ---- fast exact division self test -----------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long &x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double random_double(unsigned long long &st, int emax) {
  const unsigned long long r = splitmix64(st);
  unsigned long long mant = r & 0xFFFFFFFFFFFFFull;
  const unsigned kind = (unsigned)(r >> 60) & 7u;  // 3/8 of the draws: edge mantissas
  if (kind == 0) mant = 0xFFFFFFFFFFFFFull - ((r >> 52) & 15ull);
  if (kind == 1) mant = (r >> 52) & 15ull;
  if (kind == 2) mant = 0x8000000000000ull + ((r >> 52) & 15ull) - 8ull;
  const unsigned long long r2 = splitmix64(st);
  const int e = (int)(r2 % (unsigned long long)(2 * emax + 1)) - emax;
  const unsigned long long bits = ((r2 >> 63) << 63) | ((unsigned long long)(1023 + e) << 52) | mant;
  return __longlong_as_double((long long)bits);
}
__global__ void k_selftest_fastdiv(unsigned long long seed, int per_thread, int emax,
                                   unsigned long long *mismatch) {
  unsigned long long st = seed + 0x1234567ull * (blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x);
  unsigned long long bad = 0;
  for (int i = 0; i < per_thread; ++i) {
    const double d = random_double(st, emax);
    const double y = 1.0 / d;
    const double yl = recip_lo(d, y);
    // several numerators per denominator, as in the kernels (static d, changing a); both
    // reciprocal forms (5 instructions from RN(1/d), 4 from the double-double reciprocal)
    for (int k = 0; k < 4; ++k) {
      const double a = random_double(st, emax);
      const double q_ref = a / d;
      const double q_fast = div_by_recip(a, d, y);
      const double q_fast2 = div_by_recip2(a, d, y, yl);
      bad += (__double_as_longlong(q_ref) != __double_as_longlong(q_fast)) ? 1ull : 0ull;
      bad += (__double_as_longlong(q_ref) != __double_as_longlong(q_fast2)) ? 1ull : 0ull;
    }
  }
  if (bad) atomicAdd(mismatch, bad);
}

// the 3-instruction quotient (col_vertadvdiff's DIV == 6) and the device's own `/` of n operand
// pairs (the host compares both with ITS IEEE quotient)
__global__ void k_selftest_div3(const double *__restrict__ a, const double *__restrict__ d, size_t n,
                                double *__restrict__ q3, double *__restrict__ qd) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const double y = 1.0 / d[i];
    double q = a[i] * y;
    const double r = __builtin_fma(-d[i], q, a[i]);
    q3[i] = __builtin_fma(r, y, q);
    qd[i] = a[i] / d[i];
  }
}
// y[i] = 1.0 / d[i] as every kernel's prologue forms its reciprocals
__global__ void k_recip(const double *__restrict__ d, size_t n, double *__restrict__ y) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    y[i] = 1.0 / d[i];
}

// yh[i] = 1.0 / d[i] and yl[i] = recip_lo_div(d[i], yh[i]) as k_column_steps' prologue forms the
// pair for its 2-instruction quotients
__global__ void k_recip2(const double *__restrict__ d, size_t n, double *__restrict__ yh,
                         double *__restrict__ yl) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const double y = 1.0 / d[i];
    yh[i] = y;
    yl[i] = recip_lo_div(d[i], y);
  }
}
// the 2-instruction quotient (col_vertadvdiff's DIV == 7 / 8) of n operand pairs, reciprocal pair
// formed as in k_recip2
__global__ void k_selftest_div2(const double *__restrict__ a, const double *__restrict__ d, size_t n,
                                double *__restrict__ q2) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const double y = 1.0 / d[i];
    q2[i] = div_by_recip2x(a[i], y, recip_lo_div(d[i], y));
  }
}

// Upload the host columns `in` (n doubles each; on the device one after the other), run
// launch(din, dout, stream) and download the `nout` columns of n doubles it wrote to dout.
template <class Launch>
static int device_round_trip(std::initializer_list<const double *> in, size_t n, size_t nout,
                             std::vector<double> *out, Launch launch) {
  DeviceScratch<double> din, dout;
  if (const int rc = din.alloc(in.size() * n)) return rc;
  if (const int rc = dout.alloc(nout * n)) return rc;
  hipStream_t s = resolve_stream(nullptr);
  size_t k = 0;
  for (const double *col : in)
    PM_HIP(hipMemcpyAsync(din.p + n * k++, col, n * sizeof(double), hipMemcpyHostToDevice, s));
  launch(din.p, dout.p, s);
  PM_HIP(hipGetLastError());
  out->resize(nout * n);
  PM_HIP(hipMemcpyAsync(out->data(), dout.p, nout * n * sizeof(double), hipMemcpyDeviceToHost, s));
  PM_HIP(hipStreamSynchronize(s));
  return PM_OK;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

// ok[i] = the device's 1.0 / d[i] -- and with `lo` its low part recip_lo_div -- is the host's
// correctly rounded quotient (div2_proof's pair), bit for bit
static int recip_matches_host(const double *d, size_t n, bool lo, int32_t *ok) {
  std::vector<double> y;
  const int rc = device_round_trip({d}, n, lo ? 2 : 1, &y, [&](double *dd, double *dy, hipStream_t s) {
    if (lo)
      hipLaunchKernelGGL(k_recip2, dim3(256), dim3(256), 0, s, dd, n, dy, dy + n);
    else
      hipLaunchKernelGGL(k_recip, dim3(256), dim3(256), 0, s, dd, n, dy);
  });
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    const double yh = 1.0 / d[i];
    ok[i] = same_bits(yh, y[i]) && (!lo || same_bits(recip_lo_div_host(d[i], yh), y[n + i]));
  }
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_selftest_fastdiv(uint64_t seed, int32_t blocks, int32_t per_thread, int32_t emax,
                        uint64_t *tested, uint64_t *mismatches) {
  PM_REQUIRE(tested && mismatches, "NULL output");
  PM_REQUIRE(blocks > 0 && per_thread > 0 && emax >= 0 && emax <= 400, "bad sizes");
  DeviceScratch<unsigned long long> d;
  if (const int rc = d.alloc(1)) return rc;
  hipStream_t st = resolve_stream(nullptr);
  PM_HIP(hipMemsetAsync(d.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_selftest_fastdiv, dim3(blocks), dim3(256), 0, st,
                     (unsigned long long)seed, per_thread, emax, d.p);
  PM_HIP(hipGetLastError());
  unsigned long long h = 0;
  PM_HIP(hipMemcpyAsync(&h, d.p, sizeof(h), hipMemcpyDeviceToHost, st));
  PM_HIP(hipStreamSynchronize(st));
  *mismatches = h;
  *tested = 4ull * (unsigned long long)per_thread * 256ull * (unsigned long long)blocks;
  return PM_OK;
}

int pm_div3_proven(const double *d, int64_t n, int32_t *proven, int64_t *candidates) {
  PM_REQUIRE(proven, "proven is NULL");
  PM_REQUIRE(n == 0 || d, "d is NULL");
  long long nc = 0;
  int ok = 1;
  for (int64_t i = 0; i < n && ok; ++i) ok = div3_proof(d[i], nullptr, &nc);
  *proven = ok;
  if (candidates) *candidates = nc;
  return PM_OK;
}

int pm_div2_proven(const double *d, int64_t n, int32_t *proven, int64_t *candidates) {
  PM_REQUIRE(n == 0 || (d && proven), "d or proven is NULL");
  long long nc = 0;
  for (int64_t i = 0; i < n; ++i) proven[i] = div2_proof(d[i], nullptr, &nc);
  if (candidates) *candidates = nc;
  return PM_OK;
}

int pm_recip_check(const double *d, int64_t n, int32_t *ok) {
  PM_REQUIRE(ok, "ok is NULL");
  PM_REQUIRE(n == 0 || d, "d is NULL");
  *ok = 1;
  if (n == 0) return PM_OK;
  std::vector<int32_t> each((size_t)n);
  if (const int rc = recip_matches_host(d, (size_t)n, false, each.data())) return rc;
  for (int32_t e : each) *ok &= e;
  return PM_OK;
}

int pm_recip2_check(const double *d, int64_t n, int32_t *ok) {
  PM_REQUIRE(n == 0 || (d && ok), "d or ok is NULL");
  if (n == 0) return PM_OK;
  return recip_matches_host(d, (size_t)n, true, ok);
}

int pm_selftest_div2(uint64_t seed, int32_t ndenoms, uint64_t *tested, uint64_t *mismatches,
                     uint64_t *unproven, uint64_t *unproven_mismatches) {
  PM_REQUIRE(tested && mismatches && unproven && unproven_mismatches, "NULL output");
  PM_REQUIRE(ndenoms >= 1 && ndenoms <= (1 << 22), "ndenoms must be in [1, 2^22]");
  const DivPairs p = selftest_div_pairs(seed, ndenoms, div2_proof, true);
  const size_t n = p.a.size();
  std::vector<double> hq;
  const int rc = device_round_trip({p.a.data(), p.d.data()}, n, 1, &hq,
                                   [&](double *in, double *dq, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_div2, dim3(256), dim3(256), 0, s, in, in + n, n, dq);
  });
  if (rc) return rc;
  unsigned long long bad = 0, ubad = 0;
  for (size_t i = 0; i < n; ++i)  // against the host's IEEE quotient: the reference
    if (!same_bits(p.a[i] / p.d[i], hq[i])) ++(p.proven[i] ? bad : ubad);
  *tested = n;
  *mismatches = bad;
  *unproven = p.unproven;
  *unproven_mismatches = ubad;
  return PM_OK;
}

int pm_selftest_div3(uint64_t seed, int32_t ndenoms, uint64_t *tested, uint64_t *mismatches,
                     uint64_t *unproven, uint64_t *device_div_off, double *one_bad_pair) {
  PM_REQUIRE(tested && mismatches && unproven && device_div_off, "NULL output");
  PM_REQUIRE(ndenoms >= 1 && ndenoms <= (1 << 22), "ndenoms must be in [1, 2^22]");
  const DivPairs p = selftest_div_pairs(seed, ndenoms, div3_proof, false);
  const size_t n = p.a.size();
  std::vector<double> hq;
  const int rc = device_round_trip({p.a.data(), p.d.data()}, n, 2, &hq,
                                   [&](double *in, double *dq, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_div3, dim3(256), dim3(256), 0, s, in, in + n, n, dq, dq + n);
  });
  if (rc) return rc;
  unsigned long long bad = 0, off = 0;
  for (size_t i = 0; i < n; ++i) {
    const double q = p.a[i] / p.d[i];  // the host's IEEE quotient: the reference
    if (!same_bits(q, hq[i])) {        // (proven or not: `unproven` must be 0 as well)
      if (one_bad_pair && !bad) {
        one_bad_pair[0] = p.a[i];
        one_bad_pair[1] = p.d[i];
      }
      ++bad;
    }
    if (!same_bits(q, hq[n + i])) ++off;
  }
  *tested = n;
  *mismatches = bad;
  *unproven = p.unproven;
  *device_div_off = off;
  return PM_OK;
}

}  // extern "C"
