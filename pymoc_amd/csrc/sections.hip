// sections.hip -- pymoc.plotting's section interpolators for a whole ensemble:
// Interpolate_channel.__call__ (src/pymoc/plotting/interp_channel.py:40-62) and
// Interpolate_twocol.__call__ (src/pymoc/plotting/interp_twocol.py:37-73) at every point of a
// query grid, in gridit's layout (src/pymoc/utils/gridit.py:24-30).
//
// Every point is one scipy.optimize.brenth root find (two with the bottom slope) over np.interp'ed
// profiles; the points are independent.  One workgroup owns one member and a block of 256
// consecutive points of its [nyq][nzq] grid (z fastest, so the f64 stores coalesce): it stages the
// member's profiles and axes in LDS (applying the scripts' fix-ups there), every lane finds the
// member's bottom slope sbot (same inputs in every lane, so the root find runs wave-uniformly and
// costs one lane's time), then each lane solves its own point.  Lanes take different numbers of
// iterations; DESIGN.md section 8 has the measured cost.
//
// Arithmetic: IEEE fp64 in the reference's order, correctly rounded `/` (no reciprocal quotients),
// no contraction (-ffp-contract=off), np.interp as pm::interp_sorted -- bit-identical sections.
#include "common.hip.h"

namespace pm {

constexpr int SEC_BLOCK = 256;

// make_func's closure (src/pymoc/utils/make_func.py:31-44): np.interp on the axis, or a float
struct SecProf {
  const double *xp, *fp;
  int n;
  double c;
  bool scalar;
  __device__ __forceinline__ double operator()(double x) const {
    return scalar ? c + 0. * x : interp_sorted(x, xp, fp, n);
  }
};

// scipy.optimize.brenth(f, xa, xb) with SciPy 1.15.3's defaults: brentq's decisions (see
// brentq_interp, psi_so.hip.h) with the hyperbolic extrapolation step of Zeros/brenth.c, and the
// Python wrapper's NaN guard (every evaluation, in order).  `st` = PM_SEC_* (NaN returned).
template <class F>
__device__ __forceinline__ double brenth(const F &f, double xa, double xb, int &st) {
  const double xtol = 2e-12, rtol = 8.881784197001252e-16;
  double xpre = xa, xcur = xb, xblk = 0., fblk = 0., spre = 0., scur = 0.;
  st = PM_SEC_OK;
  double fpre = f(xpre);
  if (fpre != fpre) { st = PM_SEC_ENAN; return __builtin_nan(""); }
  double fcur = f(xcur);
  if (fcur != fcur) { st = PM_SEC_ENAN; return __builtin_nan(""); }
  if (fpre == 0) return xpre;
  if (fcur == 0) return xcur;
  if (__builtin_signbit(fpre) == __builtin_signbit(fcur)) {
    st = PM_SEC_ESIGN;
    return __builtin_nan("");
  }
  for (int it = 0; it < 100; ++it) {
    if (fpre != 0 && fcur != 0 && (__builtin_signbit(fpre) != __builtin_signbit(fcur))) {
      xblk = xpre;
      fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (fabs(fblk) < fabs(fcur)) {
      xpre = xcur;
      xcur = xblk;
      xblk = xpre;
      fpre = fcur;
      fcur = fblk;
      fblk = fpre;
    }
    const double delta = (xtol + rtol * fabs(xcur)) / 2;
    const double sbis = (xblk - xcur) / 2;
    if (fcur == 0 || fabs(sbis) < delta) return xcur;
    if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
      double stry;
      if (xpre == xblk) {  // interpolate
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {  // extrapolate (hyperbolic)
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk - fpre) / (fblk * dpre - fpre * dblk);
      }
      const double lim1 = fabs(spre), lim2 = 3 * fabs(sbis) - delta;
      if (2 * fabs(stry) < (lim1 < lim2 ? lim1 : lim2)) {
        spre = scur;
        scur = stry;
      } else {
        spre = sbis;
        scur = sbis;
      }
    } else {
      spre = sbis;
      scur = sbis;
    }
    xpre = xcur;
    fpre = fcur;
    if (fabs(scur) > delta)
      xcur += scur;
    else
      xcur += (sbis > 0 ? delta : -delta);
    fcur = f(xcur);
    if (fcur != fcur) { st = PM_SEC_ENAN; return __builtin_nan(""); }
  }
  st = PM_SEC_ECONV;
  return __builtin_nan("");
}

// 16-byte carve of the dynamic LDS (Guideline 17): doubles rounded up to an even count
__host__ __device__ __forceinline__ int sec_pad(int n) { return (n + 1) & ~1; }

__host__ __device__ __forceinline__ size_t sec_lds_bytes(const pm_sections &a) {
  // y, z, bs, bn (+ bsurf on y for the two-column kind)
  int d = 2 * sec_pad(a.ny) + 2 * sec_pad(a.nz);
  d += (a.kind == PM_SEC_TWOCOL) ? sec_pad(a.nz) + sec_pad(a.ny) : sec_pad(a.ny);
  return (size_t)d * sizeof(double);
}

__global__ void __launch_bounds__(SEC_BLOCK) k_sections(pm_sections a) {
  extern __shared__ __attribute__((aligned(16))) double sec_lds[];
  const int m = blockIdx.x;
  const int ny = a.ny, nz = a.nz;
  const bool twocol = a.kind == PM_SEC_TWOCOL;
  const int nbs = twocol ? nz : ny;
  double *ly = sec_lds;
  double *lz = ly + sec_pad(ny);
  double *lbs = lz + sec_pad(nz);
  double *lbn = lbs + sec_pad(twocol ? nz : ny);
  double *lsurf = lbn + sec_pad(nz);
  const bool bs_scalar = a.flags & PM_SEC_BS_SCALAR, bn_scalar = a.flags & PM_SEC_BN_SCALAR;
  const double *gbs = a.bs + a.bs_offset + (int64_t)m * a.bs_stride;
  const double *gbn = a.bn + a.bn_offset + (int64_t)m * a.bn_stride;
  for (int i = threadIdx.x; i < ny; i += SEC_BLOCK) ly[i] = a.y[i];
  for (int i = threadIdx.x; i < nz; i += SEC_BLOCK) lz[i] = a.z[i];
  if (!bs_scalar)
    for (int i = threadIdx.x; i < nbs; i += SEC_BLOCK) lbs[i] = gbs[i];
  if (!bn_scalar)
    for (int i = threadIdx.x; i < nz; i += SEC_BLOCK) lbn[i] = gbn[i];
  __syncthreads();
  if (a.fixups && threadIdx.x == 0) {  // host checked: array profiles only
    if (!twocol && (a.fixups & PM_SEC_FIX_PLOT_OVERTURNING)) {
      if (lbs[0] > lbs[1]) lbs[0] = lbs[1];  // Plot_overturning.py:42-45
      if (lbs[0] < lbn[0]) lbn[0] = lbs[0];  // :46-50
    }
    if (twocol && (a.fixups & PM_SEC_FIX_PLOT_OVERTURNING)) lbn[0] = lbs[0];  // :63-64
    if (!twocol && (a.fixups & PM_SEC_FIX_TWOBASIN)) lbs[ny - 1] = lbn[nz - 1];  // :176
  }
  __syncthreads();
  const SecProf bs{twocol ? lz : ly, lbs, nbs, bs_scalar ? gbs[0] : 0., bs_scalar};
  const SecProf bn{lz, lbn, nz, bn_scalar ? gbn[0] : 0., bn_scalar};
  const double l = ly[ny - 1], z0 = lz[0];
  int sst;
  double sbot;
  if (twocol) {
    // bsurf = make_func(self.y / l * self.bn(0) + (1 - self.y / l) * self.bs(0)) (interp_twocol.py:39-42)
    const double bn0 = bn(0.), bs0 = bs(0.);
    for (int i = threadIdx.x; i < ny; i += SEC_BLOCK) {
      const double t = ly[i] / l;
      lsurf[i] = t * bn0 + (1 - t) * bs0;
    }
    __syncthreads();
    // sbot = brenth(fint, 0., 1.), fint(x) = bn(0) - bs(-x*l)  (:50-52, :64)
    sbot = brenth([&](double x) { return bn0 - bs(-x * l); }, 0., 1., sst);
  } else {
    // sbot = -brenth(f2, self.z[0], 0.)/l, f2(x) = bn(x) - bs(0)  (interp_channel.py:47-49, :56)
    const double bs0 = bs(0.);
    sbot = -brenth([&](double x) { return bn(x) - bs0; }, z0, 0., sst) / l;
  }
  const SecProf bsurf{ly, lsurf, ny, 0., false};

  const int npts = a.nyq * a.nzq;
  const int p = blockIdx.y * SEC_BLOCK + threadIdx.x;
  if (p >= npts) return;
  const int iy = p / a.nzq, iz = p - iy * a.nzq;
  const double y = a.yq[iy];
  double z = a.zq[iz];
  int st = PM_SEC_OK;
  double r = 0.;
  if (!twocol) {
    if (y == l) {
      r = bn(z);  // :42-44
    } else if (sst != PM_SEC_OK) {
      st = sst;
    } else {
      double s = sbot;
      if (!(-z > sbot * y))  // :58-61
        s = brenth([&](double x) { return bn(z - x * (l - y)) - bs(y + z / x); }, 1.e-12, 1.0, st);
      if (st == PM_SEC_OK) r = bn(z - s * (l - y));
    }
  } else {
    if (z == 0 && y == 0) z = -0.01;  // :43-45
    if (z == z0) z = 0.9999 * z0;     // :46-48
    if (sst != PM_SEC_OK) {
      st = sst;
    } else {
      double s;
      if (z > -sbot * (l - y))  // :66-69
        s = brenth([&](double x) { return bs(z - x * y) - bsurf(y - z / x); }, 1e-10, 1.0, st);
      else
        s = brenth([&](double x) { return bs(z - x * y) - bn(z + x * (l - y)); }, -1.0, 1.0, st);
      if (st == PM_SEC_OK) r = bs(z - s * y);
    }
  }
  const size_t o = (size_t)m * (size_t)npts + (size_t)p;
  a.out[o] = (st == PM_SEC_OK) ? r : __builtin_nan("");
  if (a.status) a.status[o] = (uint8_t)st;
  if (a.first && st != PM_SEC_OK) atomicMin((unsigned int *)(a.first + m), (unsigned int)p);
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_sections_grid(const pm_sections *sec, pm_stream_t stream) {
  PM_REQUIRE(sec, "sec is NULL");
  const pm_sections &a = *sec;
  PM_REQUIRE(a.kind == PM_SEC_CHANNEL || a.kind == PM_SEC_TWOCOL, "bad kind %d", a.kind);
  PM_REQUIRE(a.n >= 0, "bad member count n=%d", a.n);
  PM_REQUIRE(a.ny >= 2 && a.ny <= PM_SEC_MAX_LEVELS && a.nz >= 2 && a.nz <= PM_SEC_MAX_LEVELS,
             "bad profile grid ny=%d nz=%d (2..%d levels each: the profiles are staged in LDS)",
             a.ny, a.nz, PM_SEC_MAX_LEVELS);
  PM_REQUIRE(a.nyq >= 1 && a.nyq <= PM_SEC_MAX_LEVELS && a.nzq >= 1 && a.nzq <= PM_SEC_MAX_LEVELS,
             "bad query grid nyq=%d nzq=%d (1..%d points each)", a.nyq, a.nzq, PM_SEC_MAX_LEVELS);
  PM_REQUIRE(!(a.flags & ~(PM_SEC_BS_SCALAR | PM_SEC_BN_SCALAR)), "bad flags %d", a.flags);
  PM_REQUIRE(!(a.fixups & ~(PM_SEC_FIX_PLOT_OVERTURNING | PM_SEC_FIX_TWOBASIN)), "bad fixups %d",
             a.fixups);
  PM_REQUIRE(!(a.kind == PM_SEC_TWOCOL && (a.fixups & PM_SEC_FIX_TWOBASIN)),
             "PM_SEC_FIX_TWOBASIN is a channel fix-up (the two-column one needs a third profile)");
  PM_REQUIRE(!a.fixups || !(a.flags & (PM_SEC_BS_SCALAR | PM_SEC_BN_SCALAR)),
             "fix-ups need array profiles");
  PM_REQUIRE(a.bs_offset >= 0 && a.bn_offset >= 0 && a.bs_stride >= 0 && a.bn_stride >= 0,
             "negative offset or stride");
  if (a.n == 0) return PM_OK;
  PM_REQUIRE(a.y && a.z && a.yq && a.zq && a.bs && a.bn && a.out,
             "pm_sections has a NULL required pointer");
  hipStream_t st = resolve_stream(stream);
  if (a.first) PM_HIP(hipMemsetAsync(a.first, 0xff, (size_t)a.n * sizeof(int32_t), st));
  const int npts = a.nyq * a.nzq;
  hipLaunchKernelGGL(k_sections, dim3(a.n, (npts + SEC_BLOCK - 1) / SEC_BLOCK), dim3(SEC_BLOCK),
                     sec_lds_bytes(a), st, a);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
