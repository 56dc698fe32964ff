// forcing.hip -- time-dependent forcing of an ensemble (pymoc_amd.ForcingSchedule).
//
// (no counterpart: the user loop's assignments `basin.bs = ...`, `PsiSO.tau = ...` ahead of a
// step.)  The reference's transient experiments assign the forcing of each member as a function
// of time at the top of the loop body; the ensemble drivers keep that forcing in device arrays
// every launch re-reads (cols.bs, so.tau, bs_SO, ml.b_rest, ml.surflux).  One launch here
// evaluates a piecewise-linear schedule at time t into up to 8 of them.
//
// The bracket of t in the knots depends on t alone: pm_forcing_apply finds it on the host (the
// knots are a host array) with np.interp's own case analysis, and the kernel gets the case as
// arguments -- copy one knot's values (t outside the knots, on a knot, K = 1), interpolate
// between two knots, or write t (NaN).  What is left is a streaming kernel: the rows of a target
// are contiguous, so a target is ONE flat range of n * len doubles, and with per-member values a
// knot's slab has the same layout.  blockIdx.y is the target, the blocks of a target stride over
// its range; where destination and slabs share their alignment modulo 16 bytes the range is
// covered by 16-byte accesses between a scalar head and tail (8-byte accesses stream at 0.54-0.70
// of the 16-byte rate on this device), else element by element (ny = 51 rows of an odd number of
// members, shared values).
// Traffic per call: 2 knot slabs read, 1 target written -- 3 x 8 B per element (per-member
// values); DESIGN.md section 12 has the measured time.
#include <cmath>
#include "common.hip.h"

namespace pm {

constexpr int FORCING_BLOCK = 256;
enum { FORCING_COPY = 0, FORCING_LERP = 1, FORCING_NAN = 2 };

struct forcing_item {
  double *dst;          // first written element
  const double *lo, *hi;  // the two knots' values (hi == lo when copying)
  int64_t total;        // n * len
  int32_t len;          // > 0: values shared by the members, element i reads lo[i % len]; 0: lo[i]
  int32_t head;         // 16-byte path: scalar elements ahead of the first aligned pair; -1: none
};

struct forcing_args {
  forcing_item item[PM_FORCING_MAX_TARGETS];
  double t, x0, x1;
  int32_t mode, ntargets;
};

// np.interp between two knots: the arithmetic of pm::interp_sorted (common.hip.h) for xp[j] < x <
// xp[j + 1], in its order -- the file is built with -ffp-contract=off
__device__ __forceinline__ double forcing_lerp(double f0, double f1, double t, double x0,
                                               double x1) {
  const double slope = (f1 - f0) / (x1 - x0);
  double r = slope * (t - x0) + f0;
  if (r != r) {
    r = slope * (t - x1) + f1;
    if (r != r && f0 == f1) r = f0;
  }
  return r;
}

template <int MODE>
__device__ __forceinline__ void forcing_range(const forcing_item &it, double t, double x0,
                                              double x1) {
  const int64_t tid = (int64_t)blockIdx.x * FORCING_BLOCK + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * FORCING_BLOCK;
  auto value = [&](double f0, double f1) {
    return MODE == FORCING_LERP ? forcing_lerp(f0, f1, t, x0, x1) : (MODE == FORCING_NAN ? t : f0);
  };
  if (it.head >= 0) {
    // [0, head) scalar, pairs from head, one scalar tail element when the rest is odd
    const int64_t head = it.head, npairs = (it.total - head) >> 1;
    const double2 *lo2 = reinterpret_cast<const double2 *>(it.lo + head);
    const double2 *hi2 = reinterpret_cast<const double2 *>(it.hi + head);
    double2 *dst2 = reinterpret_cast<double2 *>(it.dst + head);
    for (int64_t p = tid; p < npairs; p += nthreads) {
      double2 a = make_double2(0., 0.), b = a;
      if (MODE != FORCING_NAN) a = lo2[p];
      if (MODE == FORCING_LERP) b = hi2[p];
      dst2[p] = make_double2(value(a.x, b.x), value(a.y, b.y));
    }
    if (tid < 2) {
      const int64_t i = tid == 0 ? 0 : head + 2 * npairs;
      if (tid == 0 ? head == 1 : i < it.total) {
        const double a = MODE != FORCING_NAN ? it.lo[i] : 0.;
        const double b = MODE == FORCING_LERP ? it.hi[i] : 0.;
        it.dst[i] = value(a, b);
      }
    }
    return;
  }
  for (int64_t i = tid; i < it.total; i += nthreads) {
    const int64_t k = it.len > 0 ? i % it.len : i;
    const double a = MODE != FORCING_NAN ? it.lo[k] : 0.;
    const double b = MODE == FORCING_LERP ? it.hi[k] : 0.;
    it.dst[i] = value(a, b);
  }
}

// the item is selected over the constant capacity so that a.item[f] is read from the kernel
// arguments at constant offsets (a runtime index would copy the table to scratch)
__global__ void __launch_bounds__(FORCING_BLOCK) k_forcing_apply(forcing_args a) {
  forcing_item it = a.item[0];
#pragma unroll
  for (int f = 1; f < PM_FORCING_MAX_TARGETS; ++f)
    if (f == (int)blockIdx.y) it = a.item[f];
  if ((int64_t)blockIdx.x * FORCING_BLOCK >= it.total) return;  // a shorter target than the widest
  if (a.mode == FORCING_LERP)
    forcing_range<FORCING_LERP>(it, a.t, a.x0, a.x1);
  else if (a.mode == FORCING_COPY)
    forcing_range<FORCING_COPY>(it, a.t, a.x0, a.x1);
  else
    forcing_range<FORCING_NAN>(it, a.t, a.x0, a.x1);
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_forcing_apply(const struct pm_forcing *fp, double t, pm_stream_t stream) {
  PM_REQUIRE(fp, "f is NULL");
  const struct pm_forcing &f = *fp;
  PM_REQUIRE(f.ntargets >= 1 && f.ntargets <= PM_FORCING_MAX_TARGETS,
             "ntargets %d outside [1, %d]", f.ntargets, PM_FORCING_MAX_TARGETS);
  PM_REQUIRE(f.K >= 1, "K %d < 1", f.K);
  PM_REQUIRE(f.n >= 1, "n %d < 1", f.n);
  PM_REQUIRE(f.knots, "knots is NULL");
  for (int k = 0; k < f.K; ++k)
    PM_REQUIRE(std::isfinite(f.knots[k]) && (k == 0 || f.knots[k] > f.knots[k - 1]),
               "knots[%d] is not finite or not above knots[%d]", k, k - 1);
  for (int i = 0; i < f.ntargets; ++i) {
    const pm_forcing_target &g = f.target[i];
    PM_REQUIRE(g.dst && g.values, "target %d: NULL pointer", i);
    PM_REQUIRE(g.len >= 1 && g.row0 >= 0, "target %d: len %d < 1 or row0 %lld < 0", i, g.len,
               (long long)g.row0);
    PM_REQUIRE(g.per_member == 0 || g.per_member == 1, "target %d: per_member %d is not 0 or 1",
               i, g.per_member);
  }
  // np.interp's cases (pm::interp_sorted, common.hip.h): knot j's values, or knots j and j + 1
  forcing_args a;
  memset(&a, 0, sizeof(a));
  const double *xp = f.knots;
  const int K = f.K;
  int j = 0;
  a.mode = FORCING_COPY;
  a.t = t;
  if (K == 1) {
    j = 0;  // np.interp's one-knot form compares only: a NaN t gets the knot's value too
  } else if (t != t) {
    a.mode = FORCING_NAN;
  } else if (t < xp[0]) {
    j = 0;
  } else if (t > xp[K - 1]) {
    j = K - 1;
  } else {
    while (j + 1 < K && t >= xp[j + 1]) ++j;  // the last knot at or below t
    if (j < K - 1 && xp[j] != t) {
      a.mode = FORCING_LERP;
      a.x0 = xp[j];
      a.x1 = xp[j + 1];
    }
  }
  a.ntargets = f.ntargets;
  int64_t widest = 0;
  for (int i = 0; i < PM_FORCING_MAX_TARGETS; ++i) {
    // (unused entries repeat target 0: never selected, never dereferenced)
    const pm_forcing_target &g = f.target[i < f.ntargets ? i : 0];
    forcing_item &it = a.item[i];
    const int64_t slab = g.per_member ? (int64_t)f.n * g.len : (int64_t)g.len;
    it.dst = g.dst + g.row0 * g.len;
    it.lo = g.values + (int64_t)j * slab;
    it.hi = a.mode == FORCING_LERP ? it.lo + slab : it.lo;
    it.total = (int64_t)f.n * g.len;
    it.len = g.per_member ? 0 : g.len;
    const uintptr_t d = (uintptr_t)it.dst, l = (uintptr_t)it.lo, h = (uintptr_t)it.hi;
    const bool same = g.per_member && d % 8 == 0 && ((d ^ l) & 15) == 0 && ((d ^ h) & 15) == 0;
    it.head = same ? (int32_t)((d & 15) != 0) : -1;
    if (i < f.ntargets && it.total > widest) widest = it.total;
  }
  // a thread of the 16-byte path takes two elements, so the grid covers the widest target in one
  // pass of pairs; the scalar path strides the same grid twice
  const int64_t bx = (widest + 2 * FORCING_BLOCK - 1) / (2 * FORCING_BLOCK);
  PM_REQUIRE(bx <= INT32_MAX, "a target of %lld elements is too large", (long long)widest);
  hipStream_t st = resolve_stream(stream);
  hipLaunchKernelGGL(k_forcing_apply, dim3((unsigned)bx, (unsigned)f.ntargets), dim3(FORCING_BLOCK),
                     0, st, a);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
