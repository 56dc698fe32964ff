// indices.hip -- per-member overturning indices (pymoc_amd.RowIndices / IndexRecorder).
//
// (no counterpart: what a user computes from the profiles after the loop -- `np.max(AMOC.Psi)`,
// the depth of that maximum, the depth where Psi changes sign, `np.interp(-1000, z, basin.b)`.)
// A sweep is looked at as a handful of scalars per member over time; one launch here evaluates up
// to PM_INDICES_MAX index specifications for every member and writes value[spec][member] and
// pos[spec][member] at the caller's address -- record k of a recorder's device series, so a sample
// is this launch and nothing else.
//
// The specification table lives in DEVICE memory (uploaded once by the owner of the table): a wave
// walks it with a uniform index, which from memory is a scalar load per entry; the same table as a
// kernel argument indexed at run time would be copied to scratch (forcing.hip, k_forcing_apply).
//
// Layout: one wavefront per member, four members per block (column_implicit.hip's).  For every
// entry the wave's lanes stride the entry's level window, so a window is read by coalesced 512-byte
// accesses; what a lane keeps -- a (value, level) pair, a level, a partial sum, a count -- is reduced
// across the lanes by xor shuffles.  No LDS, no barrier, registers only.
//
// Definitions (include/pymoc_hip.h states them in full; r = row[lo .. hi]):
//   max / min  row[pos] with pos = lo + np.argmax(r) / np.argmin(r): the pair is ordered "a NaN
//              first, then the value, then the lower level", per lane and across lanes alike
//   at         np.interp(x0, axis, row): pm::interp_sorted's case analysis (common.hip.h) with its
//              bisection replaced by a count of the nodes <= x0 across the lanes
//   cross      the highest level pair of the window that brackets `level`, interpolated to it
//   mean       the trapezoid mean over the window (the summation order is this kernel's own: the
//              one index that is a tolerance path)
// Built with -ffp-contract=off: every product and sum below is rounded on its own.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"

namespace pm {

constexpr int IDX_WPB = 4;  // members (waves) per block

// does candidate (bv, bi) come before (av, ai)?  A level < 0 is "no candidate yet".
template <bool MAX>
__device__ __forceinline__ bool idx_before(double bv, int bi, double av, int ai) {
  if (bi < 0) return false;
  if (ai < 0) return true;
  const bool bn = bv != bv, an = av != av;
  if (bn || an) return bn && (!an || bi < ai);
  if (bv != av) return MAX ? bv > av : bv < av;
  return bi < ai;  // (-0.0 == +0.0: the lower level)
}

template <bool MAX>
__device__ __forceinline__ void idx_extremum(const double *__restrict__ row, int lo, int hi,
                                             int lane, double &val, int &pos) {
  double v = 0.0;
  int at = -1;
#pragma unroll 4
  for (int i = lo + lane; i <= hi; i += WAVE) {
    const double x = row[i];
    if (idx_before<MAX>(x, i, v, at)) {
      v = x;
      at = i;
    }
  }
  // the order is total (levels are distinct), so every lane ends with the same pair
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, WAVE);
    const int oi = __shfl_xor(at, o, WAVE);
    if (idx_before<MAX>(ov, oi, v, at)) {
      v = ov;
      at = oi;
    }
  }
  val = v;  // the row's own bits: a shuffle moves the two halves unchanged
  pos = at;
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
  return x;
}

__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o, WAVE);
    x = y > x ? y : x;
  }
  return x;
}

// np.interp(x, xp, fp) for increasing xp: pm::interp_sorted, the upper bound (first node > x) as
// the number of nodes <= x.  Whatever xp holds, every read stays inside the n levels.
__device__ __forceinline__ double idx_at(const double *__restrict__ xp,
                                         const double *__restrict__ fp, int n, double x,
                                         int lane) {
  int cnt = 0;
#pragma unroll 4
  for (int i = lane; i < n; i += WAVE) cnt += (x >= xp[i]) ? 1 : 0;
  cnt = wave_sum(cnt);
  if (n == 1) return fp[0];  // np.interp's one-node form compares only: a NaN x gets the node's value too
  if (x != x) return x;
  if (x > xp[n - 1]) return fp[n - 1];
  if (x < xp[0]) return fp[0];
  const int j = cnt > 0 ? cnt - 1 : 0;
  if (j >= n - 1) return fp[n - 1];
  const double x0 = xp[j], x1 = xp[j + 1], f0 = fp[j], f1 = fp[j + 1];
  if (x0 == x) return f0;
  const double slope = (f1 - f0) / (x1 - x0);
  double r = slope * (x - x0) + f0;
  if (r != r) {
    r = slope * (x - x1) + f1;
    if (r != r && f0 == f1) r = f0;
  }
  return r;
}

__device__ __forceinline__ void idx_cross(const double *__restrict__ row,
                                          const double *__restrict__ axis, int lo, int hi,
                                          double c, int lane, double &val, int &pos) {
  int at = -1;
#pragma unroll 4
  for (int i = lo + lane; i < hi; i += WAVE) {
    const double d0 = row[i] - c, d1 = row[i + 1] - c;
    if ((d0 <= 0.0 && 0.0 < d1) || (d0 >= 0.0 && 0.0 > d1)) at = i;  // (i rises: the highest stays)
  }
  at = wave_max(at);
  if (row[hi] == c) {
    val = axis[hi];
    pos = hi;
    return;
  }
  if (at < 0) {
    val = __builtin_nan("");
    pos = -1;
    return;
  }
  const double r0 = row[at], r1 = row[at + 1], z0 = axis[at], z1 = axis[at + 1];
  const double t = (c - r0) / (r1 - r0);
  val = z0 + t * (z1 - z0);
  pos = at;
}

__device__ __forceinline__ double idx_mean(const double *__restrict__ row,
                                           const double *__restrict__ axis, int lo, int hi,
                                           int lane) {
  if (hi == lo) return row[lo];
  double s = 0.0;
#pragma unroll 4
  for (int i = lo + lane; i < hi; i += WAVE)
    s += 0.5 * (row[i] + row[i + 1]) * (axis[i + 1] - axis[i]);
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
  return s / (axis[hi] - axis[lo]);
}

__global__ __launch_bounds__(IDX_WPB * WAVE) void k_row_indices(
    const pm_index_spec *__restrict__ table, int nspec, int n, double *__restrict__ value,
    int32_t *__restrict__ pos) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int m = __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) / WAVE));
  if (m >= n) return;  // (whole waves; the kernel has no barrier)
  for (int s = 0; s < nspec; ++s) {
    const pm_index_spec e = table[s];  // uniform address: scalar loads
    const double *row = e.src + (size_t)m * (size_t)e.stride;
    double v = 0.0;
    int at = -1;
    switch (e.kind) {
      case PM_IDX_MAX:
        idx_extremum<true>(row, e.lo, e.hi, lane, v, at);
        break;
      case PM_IDX_MIN:
        idx_extremum<false>(row, e.lo, e.hi, lane, v, at);
        break;
      case PM_IDX_AT:
        v = idx_at(e.axis, row, e.nlev, e.param, lane);
        break;
      case PM_IDX_CROSS:
        idx_cross(row, e.axis, e.lo, e.hi, e.param, lane, v, at);
        break;
      default:  // PM_IDX_MEAN (the entry refuses any other kind)
        v = idx_mean(row, e.axis, e.lo, e.hi, lane);
        break;
    }
    if (lane == 0) {
      const size_t o = (size_t)s * (size_t)n + (size_t)m;
      value[o] = v;
      pos[o] = at;
    }
  }
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_row_indices(const struct pm_row_indices *dp, double *value, int32_t *pos,
                   pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_row_indices &d = *dp;
  PM_REQUIRE(d.n >= 1, "n %d < 1", d.n);
  PM_REQUIRE(d.nspec >= 1 && d.nspec <= PM_INDICES_MAX, "nspec %d outside [1, %d]", d.nspec,
             PM_INDICES_MAX);
  PM_REQUIRE(d.spec && d.spec_dev, "the table is NULL (host or device)");
  PM_REQUIRE(value && pos, "value or pos is NULL");
  for (int i = 0; i < d.nspec; ++i) {
    const pm_index_spec &e = d.spec[i];
    PM_REQUIRE(e.src && e.axis, "spec %d: NULL pointer", i);
    PM_REQUIRE(e.kind >= PM_IDX_MAX && e.kind <= PM_IDX_MEAN, "spec %d: unknown kind %d", i,
               e.kind);
    PM_REQUIRE(e.nlev >= 1 && e.nlev <= (1 << 30), "spec %d: nlev %d outside [1, 2^30]", i,
               e.nlev);
    PM_REQUIRE(e.lo >= 0 && e.lo <= e.hi && e.hi < e.nlev,
               "spec %d: window [%d, %d] is not inside the %d levels", i, e.lo, e.hi, e.nlev);
    PM_REQUIRE(e.stride >= e.nlev, "spec %d: row stride %lld < nlev %d", i, (long long)e.stride,
               e.nlev);
  }
  const unsigned grid = (unsigned)((d.n + IDX_WPB - 1) / IDX_WPB);
  return launch_dyn(k_row_indices, grid, IDX_WPB * WAVE, 0, resolve_stream(stream), d.spec_dev,
                    (int)d.nspec, (int)d.n, value, pos);
}

}  // extern "C"
