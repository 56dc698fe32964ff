// series.hip.h -- what the three series units (stats.hip, spectra.hip, windows.hip) share: a
// series is v[k][s][m] (record, index, member; an IndexRecorder's device layout) with a record
// window [k0, k1).  The entries' opening check, the finiteness test, the staged row of members.
#pragma once
#include <cmath>
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

}  // namespace pm
