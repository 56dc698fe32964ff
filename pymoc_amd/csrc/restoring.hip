// restoring.hip -- the restoring rate lambda of every sliding window of a recorded index series
// under AR(1)-correlated regression errors (Boers 2021), computed where the series lives
// (pymoc_amd.SeriesWindows(restoring=...)).
//
// (no counterpart: a rolling statsmodels GLSAR fit over the downloaded series.)  One entry over a
// series v[k][s][m] and a record window [k0, k1), with pm_series_windows' windows.
// include/pymoc_hip.h states the definition: per used window the mean and slope of
// pm_series_windows, then ONE pass over the pairs (x_t, y_t) = (d_t, d_{t+1} - d_t) that forms the
// lagged sums of the current and the previous pair, then `iters` scalar iterations of generalised
// least squares on those sums alone, every product and sum rounded on its own
// (-ffp-contract=off).  No sqrt, log or exp: lam and rho are reproduced bit for bit by the NumPy
// restatement (tests/restoring_cases.py).
//
// K34 k_series_restoring<DET>.  Staged exactly as K22 (windows.hip) and K33 (dfa.hip), with their
// tile rule (windows_geom.hip.h): block x = (tile of TM adjacent members, chunk of NWB consecutive
// windows), block y = the index; the rows the block's windows span are staged in LDS once,
// x[r][mi], members fastest, and a thread owns one (member, window) at a time: lane = mi + TM *
// slot.
//
// The walk: ONE thread per (member, window), twice over its W rows in ascending j.  The second
// walk keeps the last residual and the previous pair in registers, so each d_j is formed from one
// LDS read, and adds into 13 accumulators (the definition's fourteenth sum, of yp * yp, enters no
// expression and is not formed).  Whitening with rho needs no further walk: every whitened sum and
// both residual sums of an iteration are polynomials in rho, lambda and a of the 13 sums and the
// first pair, so an iteration is about 40 scalar fp64 operations and 5 divisions in registers
// whatever W is.  `iters` is uniform across the grid; the loop has no early exit.  Under
// PM_WIN_DETREND_NONE the definition's residual is x_j - mean with slope +0.0, which is
// PM_WIN_DETREND_CONSTANT's: the two detrends share one instantiation, as in K33.
//
// Per window: 2 W LDS reads, 13 products and 14 sums per record of the second walk, then the
// iterations.  The compiler's resource report (hipcc -O3 -ffp-contract=off, gfx950):
//   k_series_restoring<LINEAR>     70 VGPRs, 62 SGPRs, 0 bytes of scratch
//   k_series_restoring<CONSTANT>   70 VGPRs, 58 SGPRs, 0 bytes of scratch
// no static LDS; the rows are dynamic LDS (wn_lds), so the 1024-thread block -- 4 waves a SIMD, far
// below the 128 VGPRs that allows -- is bounded by LDS, as K22 is.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"
#include "windows_geom.hip.h"

namespace pm {

template <int DET>
__global__ __launch_bounds__(WN_THREADS) void k_series_restoring(
    const double *__restrict__ v, int n, int nspec, int k0, int W, int S, int nwin, int nwb,
    int nchunks, int ltm, double stt, int iters, double *__restrict__ lam_out,
    double *__restrict__ rho_out) {
  extern __shared__ double rs_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int s = blockIdx.y;
  const int m0 = tile << ltm;
  const int i0 = chunk * nwb;                             // the block's first window
  const int nw = nwin - i0 < nwb ? nwin - i0 : nwb;       // and how many it takes (>= 1)
  const int span = W + (nw - 1) * S;                      // records staged: all inside [k0, k1)
  double *x = rs_lds_;
  const size_t rs = (size_t)nspec * (size_t)n;            // doubles between records
  const int mi = tid & (TM - 1), slot = tid >> ltm, slots = WN_THREADS >> ltm;

  {
    const double *base = series_row(v, rs, n, k0 + i0 * S, s, m0, mi);
#pragma unroll 4
    for (int r = slot; r < span; r += slots) x[(r << ltm) + mi] = base[(size_t)r * rs];
  }
  __syncthreads();

  const double nan = __builtin_nan("");
  const double half = 0.5 * (double)(W - 1);
  const double Mf = (double)(W - 2);                      // M = N - 1, N = W - 1
  const bool live = m0 + mi < n;
  for (int wl = slot; wl < nw; wl += slots) {
    const double *xw = x + (((size_t)wl * S) << ltm) + mi;
    // pass 1 of pm_series_windows: the sums of x_j and of t_j * x_j, in its order
    double sum = 0.0, st = 0.0, t = 0.0 - half;
    bool fin = true;
#pragma unroll 4
    for (int j = 0; j < W; ++j) {
      const double xj = xw[j << ltm];
      fin = fin && series_finite(xj);
      sum = sum + xj;
      if (DET == PM_WIN_DETREND_LINEAR) {
        st = st + t * xj;
        t = t + 1.0;
      }
    }
    const size_t o = ((size_t)(i0 + wl) * nspec + s) * n + m0 + mi;
    if (!fin) {
      if (live) {
        lam_out[o] = nan;
        if (rho_out) rho_out[o] = nan;
      }
      continue;
    }
    const double mean = sum / (double)W;
    const double slope = DET == PM_WIN_DETREND_LINEAR ? st / stt : 0.0;
    // pass 2: the sums of the current pair (xc, yc) = (x_t, y_t) and the previous pair (xp, yp),
    // t = 1 .. N - 1; record j = t + 1 is the one read at step t
    t = 0.0 - half;
    const double d0 = series_resid<DET>(xw[0], mean, slope, t);
    t = t + 1.0;
    double dl = series_resid<DET>(xw[1 << ltm], mean, slope, t);
    const double x0 = d0, y0 = dl - d0;
    double xp = x0, yp = y0;
    double sxc = 0.0, sxp = 0.0, syc = 0.0, syp = 0.0, sxcxc = 0.0, sxcxp = 0.0, sxpxp = 0.0,
           sxcyc = 0.0, sxcyp = 0.0, sxpyc = 0.0, sxpyp = 0.0, sycyc = 0.0, sycyp = 0.0;
#pragma unroll 2
    for (int j = 2; j < W; ++j) {
      t = t + 1.0;
      const double dj = series_resid<DET>(xw[j << ltm], mean, slope, t);
      const double xc = dl, yc = dj - dl;
      sxc = sxc + xc;
      sxp = sxp + xp;
      syc = syc + yc;
      syp = syp + yp;
      sxcxc = sxcxc + xc * xc;
      sxcxp = sxcxp + xc * xp;
      sxpxp = sxpxp + xp * xp;
      sxcyc = sxcyc + xc * yc;
      sxcyp = sxcyp + xc * yp;
      sxpyc = sxpyc + xp * yc;
      sxpyp = sxpyp + xp * yp;
      sycyc = sycyc + yc * yc;
      sycyp = sycyp + yc * yp;
      xp = xc;
      yp = yc;
      dl = dj;
    }
    // the iterations: rho^(0) = +0.0; lambda and a from the whitened sums, then (but after the
    // last lambda) the next rho from the residuals of the unwhitened model
    const double sxy2 = sxcyp + sxpyc, sy2 = syc + syp, sx2 = sxc + sxp;
    double r = 0.0, lam = 0.0;
    for (int i = 0;; ++i) {
      const double r2 = r * r;
      const double SX = sxc - r * sxp;
      const double SY = syc - r * syp;
      const double SXX = (sxcxc - (2.0 * r) * sxcxp) + r2 * sxpxp;
      const double SXY = (sxcyc - r * sxy2) + r2 * sxpyp;
      const double mx = SX / Mf, my = SY / Mf;
      lam = (SXY - SX * my) / (SXX - SX * mx);
      if (i + 1 >= iters) break;
      const double a = (my - lam * mx) / (1.0 - r);
      const double e0 = (y0 - a) - lam * x0;
      const double l2 = lam * lam, al = a * lam, a2m = Mf * (a * a);
      const double see = ((((sycyc - (2.0 * a) * syc) - (2.0 * lam) * sxcyc) + (2.0 * al) * sxc) +
                          l2 * sxcxc) + a2m;
      const double q = see + e0 * e0;
      const double c = ((((sycyp - a * sy2) - lam * sxy2) + al * sx2) + l2 * sxcxp) + a2m;
      r = c / q;
    }
    if (live) {
      const bool ok = series_finite(lam) && series_finite(r);
      lam_out[o] = ok ? lam : nan;
      if (rho_out) rho_out[o] = ok ? r : nan;
    }
  }
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_restoring(const struct pm_series_restoring *dp, double *lam, double *rho,
                        pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_restoring &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int W = d.window;
  PM_REQUIRE(W >= PM_RESTORE_WIN_MIN && W <= PM_WIN_MAX, "window length %d outside [%d, %d]", W,
             PM_RESTORE_WIN_MIN, PM_WIN_MAX);
  PM_REQUIRE(d.step >= 1 && d.step <= W, "step %d outside [1, window = %d]", d.step, W);
  PM_REQUIRE(d.k1 - d.k0 >= W, "the record window [%d, %d) is shorter than the window length %d",
             d.k0, d.k1, W);
  PM_REQUIRE(d.iters >= 1 && d.iters <= PM_RESTORE_ITERS_MAX, "iters %d outside [1, %d]", d.iters,
             PM_RESTORE_ITERS_MAX);
  return series_by_detrend(d.detrend, [&](auto det) -> int {
    PM_REQUIRE(d.stt == series_stt(W), "stt %.17g is not W (W^2 - 1) / 12 = %.17g", d.stt,
               series_stt(W));
    const int nwin = (d.k1 - d.k0 - W) / d.step + 1;
    PM_REQUIRE((long long)nwin * d.nspec < (1ll << 30), "nwin * nspec = %lld is not below 2^30",
               (long long)nwin * d.nspec);
    PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
    PM_REQUIRE(d.v, "v is NULL");
    PM_REQUIRE(lam, "lam is NULL");
    const WnGeom g = wn_geometry(W, d.step);
    const int nchunks = (nwin + g.nwb - 1) / g.nwb;
    const long long ntiles = ((long long)d.n + g.tm - 1) / g.tm;
    PM_REQUIRE(ntiles * nchunks < (1ll << 31),
               "member tiles * window chunks = %lld is not below 2^31", ntiles * nchunks);
    hipStream_t st = resolve_stream(stream);
    const int nw = nwin < g.nwb ? nwin : g.nwb;
    const size_t lds = wn_lds(g, W + (nw - 1) * d.step);
    const dim3 grid((unsigned)(ntiles * nchunks), (unsigned)d.nspec);
    // (the residual under _NONE is _CONSTANT's: x_j - mean, slope +0.0)
    constexpr int DET = decltype(det)::value == PM_WIN_DETREND_LINEAR ? PM_WIN_DETREND_LINEAR
                                                                      : PM_WIN_DETREND_CONSTANT;
    return launch_dyn(k_series_restoring<DET>, grid, WN_THREADS, lds, st, d.v, (int)d.n,
                      (int)d.nspec, (int)d.k0, W, (int)d.step, nwin, g.nwb, nchunks, g.ltm, d.stt,
                      (int)d.iters, lam, rho);
  });
}

}  // extern "C"
