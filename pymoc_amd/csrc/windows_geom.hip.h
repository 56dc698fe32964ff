// windows_geom.hip.h -- the tile of the three kernels that stage sliding windows in LDS, K22
// k_series_windows (windows.hip), K33 k_series_dfa (dfa.hip) and K34 k_series_restoring
// (restoring.hip): host inline functions, one rule for the units, which
// pm_series_windows_geometry reports.
#pragma once
#include "launch.hip.h"

namespace pm {

constexpr int WN_THREADS = 1024;

// The tile of a launch: TM adjacent members (32, 16, 8 or 4) and at most R records of LDS -- half
// a CU's LDS (two blocks to a CU) or all of it.  nwb = the windows a block takes: what fits R, a
// multiple of the WN_THREADS / TM windows in flight where it exceeds them.  Of the candidates,
// widest rows first and the half before the whole, the first is taken that holds W records, keeps
// every thread busy (nwb >= the windows in flight) and fetches a byte of the series at most six
// times (span / (nwb * S)); failing that, the widest rows that hold W records in a whole CU's LDS.
struct WnGeom {
  int tm, ltm, R, nwb;
};
inline WnGeom wn_candidate(int W, int S, int ltm, size_t bytes) {
  WnGeom g;
  g.ltm = ltm;
  g.tm = 1 << ltm;
  g.R = (int)((bytes - sizeof(int) * g.tm) / (sizeof(double) * g.tm));  // (room for the counts)
  g.nwb = 0;
  if (g.R < W) return g;
  const int slots = WN_THREADS / g.tm;
  int nwb = (g.R - W) / S + 1;
  if (nwb > slots) nwb -= nwb % slots;
  g.nwb = nwb;
  return g;
}
inline WnGeom wn_geometry(int W, int S) {
  for (int ltm = 5; ltm >= 2; --ltm)
    for (size_t bytes : {LDS_PER_CU / 2, LDS_PER_CU}) {
      const WnGeom g = wn_candidate(W, S, ltm, bytes);
      const long long span = W + (long long)(g.nwb - 1) * S;
      if (g.nwb >= WN_THREADS / g.tm && span <= 6ll * g.nwb * S) return g;
    }
  for (int ltm = 5; ltm > 2; --ltm) {
    const WnGeom g = wn_candidate(W, S, ltm, LDS_PER_CU);
    if (g.nwb) return g;
  }
  return wn_candidate(W, S, 2, LDS_PER_CU);  // W <= 4096 < 5119: it fits
}
inline size_t wn_lds(const WnGeom &g, int span) {
  return sizeof(double) * (size_t)span * g.tm + sizeof(int) * g.tm;
}

}  // namespace pm
