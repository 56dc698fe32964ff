// overturning.hip.h -- what the overturning-section kernels share (overturning.hip,
// twobasin_overturning.hip): the workgroup shape, the 16-byte LDS carve, member rows of a pm_rows
// input, and the extrema reduction -- every lane keeps the extrema of its own points (first
// occurrence: its points come in rising order); they meet in a DPP wave reduction and then over
// the block's waves, the lowest index winning a tie.
#pragma once
#include <limits.h>
#include "launch.hip.h"

namespace pm {

constexpr int OVT_BLOCK = 256;
constexpr int OVT_WAVES = OVT_BLOCK / WAVE;
constexpr int OVT_NONE = INT_MAX;

// 16-byte carve of the dynamic LDS: doubles rounded up to an even count
__host__ __device__ __forceinline__ int ovt_pad(int n) { return (n + 1) & ~1; }

__device__ __forceinline__ const double *ovt_row(const pm_rows &r, int m) {
  return r.ptr + r.offset + (int64_t)m * r.stride;
}

// a candidate extremum: value and the row-major index of its first occurrence (OVT_NONE: none)
struct OvtExt {
  double v;
  int at;
};

// `o` replaces `e` when it is the better extremum, or an equal one met earlier
template <bool MAX>
__device__ __forceinline__ OvtExt ovt_better(const OvtExt &o, const OvtExt &e) {
  const bool take = o.at != OVT_NONE &&
                    (e.at == OVT_NONE || (MAX ? o.v > e.v : o.v < e.v) || (o.v == e.v && o.at < e.at));
  return OvtExt{take ? o.v : e.v, take ? o.at : e.at};
}

// GFX9 DPP controls as in psi_so.hip.h: row_shr:d = 0x110 + d, row_bcast:15 = 0x142, row_bcast:31 =
// 0x143; lanes without a source receive 0 and are not merged
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ OvtExt ovt_dpp(const OvtExt &e) {
  OvtExt o;
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(e.v), CTRL, ROWS, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(e.v), CTRL, ROWS, 0xf, true);
  o.v = __hiloint2double(hi, lo);
  o.at = __builtin_amdgcn_update_dpp(0, e.at, CTRL, ROWS, 0xf, true);
  return o;
}

// the wave's extremum, valid in lane 63: rows of 16 by doubling, then the row totals
template <bool MAX>
__device__ __forceinline__ OvtExt ovt_wave_reduce(OvtExt e, int lane) {
  const int li = lane & 15;
  OvtExt o = ovt_dpp<0x111>(e);
  if (li >= 1) e = ovt_better<MAX>(o, e);
  o = ovt_dpp<0x112>(e);
  if (li >= 2) e = ovt_better<MAX>(o, e);
  o = ovt_dpp<0x114>(e);
  if (li >= 4) e = ovt_better<MAX>(o, e);
  o = ovt_dpp<0x118>(e);
  if (li >= 8) e = ovt_better<MAX>(o, e);
  o = ovt_dpp<0x142, 0xa>(e);
  if (lane & 16) e = ovt_better<MAX>(o, e);
  o = ovt_dpp<0x143, 0xc>(e);
  if (lane >= 32) e = ovt_better<MAX>(o, e);
  return e;
}

// one more point of a lane's running extrema (its points come in rising order: `>` and `<` keep
// the first occurrence) and of its first NaN
__device__ __forceinline__ void ovt_track(double x, int p, OvtExt &mx, OvtExt &mn, int &nan_at) {
  if (x != x) {
    if (nan_at == OVT_NONE) nan_at = p;
  } else {
    if (mx.at == OVT_NONE || x > mx.v) mx = OvtExt{x, p};
    if (mn.at == OVT_NONE || x < mn.v) mn = OvtExt{x, p};
  }
}

}  // namespace pm
