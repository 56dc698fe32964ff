// series.hip.h -- what the six series units (stats.hip, spectra.hip, windows.hip, smooth.hip,
// surrogates.hip, shifts.hip) share: a series is v[k][s][m] (record, index, member; an
// IndexRecorder's device layout) with a record window [k0, k1), or y[j][p][m] with p = surrogate *
// nspec + index over nb surrogates.  The entries' opening checks, the finiteness test, the staged
// row of members, and the in-window detrend: its residual, its sum of squared times, its dispatch.
#pragma once
#include <cmath>
#include <type_traits>
#include "common.hip.h"

// The opening check of every series entry on its descriptor d: the dims, then the record window.
// (Whatever else an entry requires, v included, it checks itself, in its own order.)
#define PM_SERIES_REQUIRE(d)                                                              \
  do {                                                                                    \
    PM_REQUIRE((d).n >= 1 && (d).nspec >= 1 && (d).nrec >= 1,                             \
               "n %d, nspec %d or nrec %d < 1", (d).n, (d).nspec, (d).nrec);              \
    PM_REQUIRE(0 <= (d).k0 && (d).k0 < (d).k1 && (d).k1 <= (d).nrec,                      \
               "window [%d, %d) is not inside the %d records", (d).k0, (d).k1, (d).nrec); \
  } while (0)

// The same of an entry over nb * nspec planes, in the two places every such entry has them: the
// dims first, and after the entry's own scalars `planes` = nb * nspec (declared here) against the
// limits -- with K, the records a plane holds (1 where the entry has none: then that check holds).
#define PM_PLANES_REQUIRE_DIMS(d)                                                              \
  PM_REQUIRE((d).n >= 1 && (d).nspec >= 1 && (d).nb >= 1, "n %d, nspec %d or nb %d < 1", (d).n, \
             (d).nspec, (d).nb)
#define PM_PLANES_REQUIRE(d, K)                                                                \
  const long long planes = (long long)(d).nb * (d).nspec;                                      \
  PM_REQUIRE(planes <= 65535, "nb * nspec = %lld > 65535", planes);                            \
  PM_REQUIRE(planes * (K) < (1ll << 31), "K * nb * nspec = %lld is not below 2^31",            \
             planes * (K));                                                                    \
  PM_REQUIRE(planes * (d).n < (1ll << 31), "nb * nspec * n = %lld is not below 2^31",          \
             planes * (d).n)

namespace pm {

__device__ __forceinline__ bool series_finite(double x) {
  return fabs(x) <= 1.7976931348623157e308;  // false for NaN and +-inf
}

// Record k, index s, member m0 + mi of a tile of adjacent members that starts at m0; rs = the
// doubles between records.  A member past the end reads the last one's values: they are in
// bounds, and nothing of it is stored.
__device__ __forceinline__ const double *series_row(const double *__restrict__ v, size_t rs, int n,
                                                    int k, int s, int m0, int mi) {
  const int mc = m0 + mi < n ? m0 + mi : n - 1;
  return v + (size_t)k * rs + (size_t)s * n + mc;
}

// The residual of a window's record under the in-window detrend DET (PM_WIN_DETREND_*), as
// include/pymoc_hip.h defines it.
template <int DET>
__device__ __forceinline__ double series_resid(double x, double mean, double slope, double t) {
  if (DET == PM_WIN_DETREND_LINEAR) return (x - mean) - slope * t;
  if (DET == PM_WIN_DETREND_CONSTANT) return x - mean;
  return x;
}

// sum t_j^2 = W (W^2 - 1) / 12 of a window of W records: a multiple of a half, so exact.
inline double series_stt(int W) { return (double)W * ((double)W * (double)W - 1.0) / 12.0; }

// An entry's `detrend`, checked where the entry calls this, and the rest of the entry f(det), det
// = std::integral_constant<int, DET>: compiled once per DET.
template <class F>
int series_by_detrend(int detrend, F &&f) {
  switch (detrend) {
    case PM_WIN_DETREND_LINEAR:
      return f(std::integral_constant<int, PM_WIN_DETREND_LINEAR>());
    case PM_WIN_DETREND_CONSTANT:
      return f(std::integral_constant<int, PM_WIN_DETREND_CONSTANT>());
    case PM_WIN_DETREND_NONE:
      return f(std::integral_constant<int, PM_WIN_DETREND_NONE>());
  }
  return fail(PM_EINVAL, "unknown detrend %d", detrend);
}

}  // namespace pm
