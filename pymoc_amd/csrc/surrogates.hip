// surrogates.hip -- AR(1) surrogates of a recorded index series, generated as a device series, and
// the count of the surrogate trends that reach an observed one (pymoc_amd.SeriesSurrogates,
// SeriesWindows.significance).
//
// (no counterpart: what a user does with a random generator and a loop over the downloaded series.)
// include/pymoc_hip.h states the two definitions; this file follows them operation by operation and
// is built with -ffp-contract=off.  The deviate is the one of philox.hip.h, shared with noise.hip.
//
// K24 k_series_surrogates.  The output y[j][p][m] (record, plane = surrogate * nspec + index,
// member) has (p, m) contiguous, so a thread owns the flat series i = p * n + m: adjacent lanes are
// adjacent members (and run on into the next plane), and every record's store is one coalesced row
// of 512 bytes per wavefront whatever n is.  The thread reads its two fit values once, then walks
// the K records: ten Philox rounds, one log, one cos and one sqrt per deviate, registers only; the
// deviates do not depend on the recurrence, so of a record only `phi * y + g * xi` sits on the
// dependent chain and the loop is unrolled by two to let deviate j + 1 issue under it.  No LDS.
//
// K25 k_series_exceed.  A thread owns one (index, member) and walks the nb surrogate planes, its
// loads coalesced rows of int32; three int32 read-modify-writes at the end.
#include <cmath>
#include "common.hip.h"
#include "philox.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int SG_BLOCK = 256;

template <bool XI>
__global__ __launch_bounds__(SG_BLOCK) void k_series_surrogates(
    const double *__restrict__ var, const double *__restrict__ ac, uint32_t n, uint32_t nspec,
    uint32_t total, int K, uint32_t b0, uint32_t key0, uint32_t key1, uint32_t id_lo,
    uint32_t id_hi, double *__restrict__ y, double *__restrict__ xi_out) {
  // (total = nb * nspec * n < 2^31: no product below wraps)
  const uint32_t i = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (i >= total) return;
  const uint32_t p = i / n, m = i - p * n;
  const uint32_t ib = p / nspec, s = p - ib * nspec;
  const uint32_t b = b0 + ib;  // (b0 + nb <= 2^32)
  const uint64_t id = (((uint64_t)id_hi << 32) | id_lo) + m;
  const size_t f = (size_t)s * n + m;
  const double phi = ac[f];
  const double sd = sqrt(var[f]);
  const bool ok = series_finite(phi) && series_finite(sd);
  const double g = sd * sqrt(fmax(0.0, 1.0 - phi * phi));
  const double nan = __builtin_nan("");
  const uint32_t st = s << 12;
  size_t o = i;
  double xi = noise_deviate(key0, key1, id, b, st);
  double yj = sd * xi;
  y[o] = ok ? yj : nan;
  if (XI) xi_out[o] = xi;
#pragma unroll 2
  for (int j = 1; j < K; ++j) {
    xi = noise_deviate(key0, key1, id, b, st | (uint32_t)j);
    yj = phi * yj + g * xi;
    o += total;
    y[o] = ok ? yj : nan;
    if (XI) xi_out[o] = xi;
  }
}

// tau-b against time of include/pymoc_hip.h: NaN for n0 == tie (then conc == disc == 0: 0 / 0)
__device__ __forceinline__ double exceed_tau(int c, int d, int t) {
  const int n0 = c + d + t;
  return (double)(c - d) / sqrt((double)n0 * (double)(n0 - t));
}

__global__ __launch_bounds__(SG_BLOCK) void k_series_exceed(
    const int32_t *__restrict__ oc, const int32_t *__restrict__ od, const int32_t *__restrict__ ot,
    const int32_t *__restrict__ sc, const int32_t *__restrict__ sd, const int32_t *__restrict__ st,
    uint32_t plane, int nb, int32_t *__restrict__ ge, int32_t *__restrict__ le,
    int32_t *__restrict__ nvalid) {
  const uint32_t i = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (i >= plane) return;
  const double obs = exceed_tau(oc[i], od[i], ot[i]);
  if (obs != obs) return;
  int g = 0, l = 0, v = 0;
  size_t o = i;
#pragma unroll 4
  for (int ib = 0; ib < nb; ++ib, o += plane) {
    const double t = exceed_tau(sc[o], sd[o], st[o]);
    // (every comparison with a NaN is false)
    v += t == t ? 1 : 0;
    g += t >= obs ? 1 : 0;
    l += t <= obs ? 1 : 0;
  }
  ge[i] += g;
  le[i] += l;
  nvalid[i] += v;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_surrogates(const struct pm_series_surrogates *dp, double *y, double *xi_out,
                         pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_surrogates &d = *dp;
  PM_PLANES_REQUIRE_DIMS(d);
  PM_REQUIRE(d.K >= 1 && d.K <= PM_SURROGATE_MAX, "K %d outside [1, %d]", d.K, PM_SURROGATE_MAX);
  PM_REQUIRE(d.b0 >= 0 && d.b0 + (int64_t)d.nb <= (1ll << 32),
             "surrogates [%lld, %lld) are not inside [0, 2^32)", (long long)d.b0,
             (long long)d.b0 + d.nb);
  PM_REQUIRE(d.member0 >= 0, "member0 %lld < 0", (long long)d.member0);
  PM_PLANES_REQUIRE(d, d.K);
  PM_REQUIRE(d.var && d.ac, "var or ac is NULL");
  PM_REQUIRE(y, "y is NULL");
  hipStream_t st = resolve_stream(stream);
  const uint32_t total = (uint32_t)(planes * d.n);
  const dim3 grid((total + SG_BLOCK - 1) / SG_BLOCK);
  const uint32_t key0 = (uint32_t)d.seed, key1 = (uint32_t)(d.seed >> 32);
  const uint32_t id_lo = (uint32_t)(uint64_t)d.member0;
  const uint32_t id_hi = (uint32_t)((uint64_t)d.member0 >> 32);
  if (xi_out)
    hipLaunchKernelGGL(k_series_surrogates<true>, grid, dim3(SG_BLOCK), 0, st, d.var, d.ac,
                       (uint32_t)d.n, (uint32_t)d.nspec, total, (int)d.K, (uint32_t)d.b0, key0,
                       key1, id_lo, id_hi, y, xi_out);
  else
    hipLaunchKernelGGL(k_series_surrogates<false>, grid, dim3(SG_BLOCK), 0, st, d.var, d.ac,
                       (uint32_t)d.n, (uint32_t)d.nspec, total, (int)d.K, (uint32_t)d.b0, key0,
                       key1, id_lo, id_hi, y, xi_out);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

int pm_series_exceed(const struct pm_series_exceed *dp, int32_t *ge, int32_t *le, int32_t *nvalid,
                     pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_exceed &d = *dp;
  PM_PLANES_REQUIRE_DIMS(d);
  PM_PLANES_REQUIRE(d, 1);  // (K = 1: the counts have no records)
  PM_REQUIRE(d.obs_conc && d.obs_disc && d.obs_tie, "an observed count array is NULL");
  PM_REQUIRE(d.sur_conc && d.sur_disc && d.sur_tie, "a surrogate count array is NULL");
  PM_REQUIRE(ge && le && nvalid, "ge, le or nvalid is NULL");
  hipStream_t st = resolve_stream(stream);
  const uint32_t plane = (uint32_t)d.nspec * (uint32_t)d.n;
  hipLaunchKernelGGL(k_series_exceed, dim3((plane + SG_BLOCK - 1) / SG_BLOCK), dim3(SG_BLOCK), 0,
                     st, d.obs_conc, d.obs_disc, d.obs_tie, d.sur_conc, d.sur_disc, d.sur_tie,
                     plane, (int)d.nb, ge, le, nvalid);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
