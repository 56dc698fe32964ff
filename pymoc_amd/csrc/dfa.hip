// dfa.hip -- the detrended-fluctuation-analysis exponent of every sliding window of a recorded
// index series, computed where the series lives (pymoc_amd.SeriesWindows(dfa=...)).
//
// (no counterpart: a rolling Python loop over the downloaded series.)  One entry over a series
// v[k][s][m] and a record window [k0, k1), with pm_series_windows' windows.  include/pymoc_hip.h
// states the definition: per used window the mean and slope of pm_series_windows, then per scale
// the profile box by box, two passes per box (the box's least-squares line, then the squared
// residuals), every product and sum rounded on its own (-ffp-contract=off).  Each F2 is reproduced
// bit for bit by the NumPy restatement (tests/dfa_cases.py); alpha goes through the device
// library's log and is held to a bound.
//
// K33 k_series_dfa<DET>.  Staged exactly as K22 (windows.hip), with K22's tile rule
// (windows_geom.hip.h): block x = (tile of TM adjacent members, chunk of NWB consecutive windows),
// block y = the index; the rows the block's windows span are staged in LDS once, x[r][mi], members
// fastest, and a thread owns one (member, window) at a time: lane = mi + TM * slot.
//
// The walk: ONE thread per (member, window), looping over the scales, and per scale over the boxes,
// pass A then pass B of a box back to back.  The reasons:
//   * the definition is a chain: y, sy, su and f_q are sequential sums, so a window and scale is
//     one dependent walk whatever is done; splitting (member, window, scale) over threads would
//     give each thread the same walk with nq times the pass-1 work (mean and slope are per window)
//     and leave lanes idle at the short scales' tails -- the scales differ in nb * s;
//   * sharing one LDS read among several scales in pass A needs a y, sy, su, u and a box counter
//     per scale in registers and a box end at a different record for each: with up to 16 scales
//     that is an indexed register file, which the compiler places in scratch.  One scale at a time
//     keeps 0 bytes of scratch and 1024 / TM windows in flight per block, as in K22;
//   * pass B re-reads the s rows pass A has just read: the same LDS addresses, no new staging.
// The scales and the two tables are a by-value kernel argument: uniform across the grid, read with
// scalar loads into SGPRs once per scale.  d_j is formed again from x_j, mean, slope and t_j on
// every read (two or three fp64 operations), which is cheaper than a second LDS array of residuals
// and would not fit next to the rows at W = 4096.  Under PM_WIN_DETREND_NONE the definition's
// increment is x_j - mean with slope +0.0, which is PM_WIN_DETREND_CONSTANT's: the two detrends
// share one instantiation.
//
// Per window: W LDS reads for pass 1, then per scale 2 nb s reads, 2 nb fp64 divisions and one more
// for F2, and one log.  The compiler's resource report (hipcc -O3 -ffp-contract=off, gfx950):
//   k_series_dfa<LINEAR>     62 VGPRs, 90 SGPRs, 0 bytes of scratch
//   k_series_dfa<CONSTANT>   58 VGPRs, 86 SGPRs, 0 bytes of scratch
// no static LDS; the rows are dynamic LDS (wn_lds: half a CU's 160 KiB or all of it, by the tile
// rule), so the 1024-thread block -- 4 waves a SIMD, far below the 128 VGPRs that allows -- is
// bounded by LDS, as K22 is.
#include <cfloat>
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"
#include "windows_geom.hip.h"

namespace pm {

// The scales and the host-made tables of a launch, a kernel argument (scalar registers).
struct DfaTab {
  int scale[PM_DFA_SCALES_MAX];
  double suu[PM_DFA_SCALES_MAX];
  double weight[PM_DFA_SCALES_MAX];
};

template <int DET>
__global__ __launch_bounds__(WN_THREADS) void k_series_dfa(
    const double *__restrict__ v, int n, int nspec, int k0, int W, int S, int nwin, int nwb,
    int nchunks, int ltm, double stt, int nq, const DfaTab tab, double *__restrict__ alpha,
    double *__restrict__ f2) {
  extern __shared__ double dfa_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int s = blockIdx.y;
  const int m0 = tile << ltm;
  const int i0 = chunk * nwb;                             // the block's first window
  const int nw = nwin - i0 < nwb ? nwin - i0 : nwb;       // and how many it takes (>= 1)
  const int span = W + (nw - 1) * S;                      // records staged: all inside [k0, k1)
  double *x = dfa_lds_;
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
  const bool live = m0 + mi < n;
  const size_t plane = (size_t)nwin * rs;
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
    double *oa = alpha + ((size_t)(i0 + wl) * nspec + s) * n + m0 + mi;
    double *of = f2 ? f2 + ((size_t)(i0 + wl) * nspec + s) * n + m0 + mi : nullptr;
    if (!fin) {
      if (live) {
        oa[0] = nan;
        if (of)
          for (int q = 0; q < nq; ++q) of[(size_t)q * plane] = nan;
      }
      continue;
    }
    const double mean = sum / (double)W;
    const double slope = DET == PM_WIN_DETREND_LINEAR ? st / stt : 0.0;
    double al = 0.0;
    bool ok = true;
    for (int q = 0; q < nq; ++q) {
      const int sc = tab.scale[q];
      const double suu = tab.suu[q], ds = (double)sc, uh = 0.5 * (double)(sc - 1);
      const int nb = W / sc;
      const double *xb = xw;                              // the box's first record
      double y = 0.0, f = 0.0, t0 = 0.0 - half;           // t_j of the box's first record (exact)
      for (int b = 0; b < nb; ++b) {
        // pass A: the profile over the box, its sum and its sum against u
        const double y0 = y;
        double sy = 0.0, su = 0.0, u = 0.0 - uh;
        t = t0;
#pragma unroll 4
        for (int i = 0; i < sc; ++i) {
          y = y + series_resid<DET>(xb[i << ltm], mean, slope, t);
          sy = sy + y;
          su = su + u * y;
          u = u + 1.0;
          t = t + 1.0;
        }
        const double a = sy / ds, c = su / suu;
        // pass B: the same profile again, less the box's line
        y = y0;
        u = 0.0 - uh;
        t = t0;
#pragma unroll 4
        for (int i = 0; i < sc; ++i) {
          y = y + series_resid<DET>(xb[i << ltm], mean, slope, t);
          const double e = (y - a) - c * u;
          f = f + e * e;
          u = u + 1.0;
          t = t + 1.0;
        }
        xb += (size_t)sc << ltm;
        t0 = t0 + ds;                                     // (whole numbers below 2^13: exact)
      }
      const double F2 = f / (double)(nb * sc);
      if (live && of) of[(size_t)q * plane] = F2;
      ok = ok && series_finite(F2) && F2 > 0.0;
      al = al + tab.weight[q] * log(F2);
    }
    if (live) oa[0] = ok ? al : nan;
  }
}

// s (s^2 - 1) / 12 of a scale: the form of series_stt, so exact.
inline double dfa_suu(int s) { return series_stt(s); }

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_dfa(const struct pm_series_dfa *dp, double *alpha, double *f2, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_dfa &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int W = d.window;
  PM_REQUIRE(W >= 4 * PM_DFA_SCALE_MIN + 4 && W <= PM_WIN_MAX, "window length %d outside [%d, %d]",
             W, 4 * PM_DFA_SCALE_MIN + 4, PM_WIN_MAX);
  PM_REQUIRE(d.step >= 1 && d.step <= W, "step %d outside [1, window = %d]", d.step, W);
  PM_REQUIRE(d.k1 - d.k0 >= W, "the record window [%d, %d) is shorter than the window length %d",
             d.k0, d.k1, W);
  PM_REQUIRE(d.nq >= 2 && d.nq <= PM_DFA_SCALES_MAX, "nq %d outside [2, %d]", d.nq,
             PM_DFA_SCALES_MAX);
  PM_REQUIRE(d.scale[0] >= PM_DFA_SCALE_MIN, "scale[0] = %d is below %d", d.scale[0],
             PM_DFA_SCALE_MIN);
  for (int q = 1; q < d.nq; ++q)
    PM_REQUIRE(d.scale[q] > d.scale[q - 1], "scale[%d] = %d is not above scale[%d] = %d", q,
               d.scale[q], q - 1, d.scale[q - 1]);
  PM_REQUIRE(d.scale[d.nq - 1] <= W / 4, "4 * scale[%d] = 4 * %d is above the window length %d",
             d.nq - 1, d.scale[d.nq - 1], W);
  double wsum = 0.0, wabs = 0.0;
  for (int q = 0; q < d.nq; ++q) {
    PM_REQUIRE(d.suu[q] == dfa_suu(d.scale[q]), "suu[%d] %.17g is not s (s^2 - 1) / 12 = %.17g", q,
               d.suu[q], dfa_suu(d.scale[q]));
    PM_REQUIRE(std::isfinite(d.weight[q]), "weight[%d] is not finite", q);
    wsum += d.weight[q];
    wabs += std::fabs(d.weight[q]);
  }
  PM_REQUIRE(wabs > 0.0 && std::fabs(wsum) <= 0x1p-40 * wabs,
             "the weights sum to %.17g, not to zero within rounding (sum |w| = %.17g)", wsum, wabs);
  return series_by_detrend(d.detrend, [&](auto det) -> int {
    PM_REQUIRE(d.stt == series_stt(W), "stt %.17g is not W (W^2 - 1) / 12 = %.17g", d.stt,
               series_stt(W));
    const int nwin = (d.k1 - d.k0 - W) / d.step + 1;
    PM_REQUIRE((long long)nwin * d.nspec < (1ll << 30), "nwin * nspec = %lld is not below 2^30",
               (long long)nwin * d.nspec);
    PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
    PM_REQUIRE(d.v, "v is NULL");
    PM_REQUIRE(alpha, "alpha is NULL");
    const WnGeom g = wn_geometry(W, d.step);
    const int nchunks = (nwin + g.nwb - 1) / g.nwb;
    const long long ntiles = ((long long)d.n + g.tm - 1) / g.tm;
    PM_REQUIRE(ntiles * nchunks < (1ll << 31),
               "member tiles * window chunks = %lld is not below 2^31", ntiles * nchunks);
    hipStream_t st = resolve_stream(stream);
    DfaTab tab = {};
    for (int q = 0; q < d.nq; ++q) {
      tab.scale[q] = d.scale[q];
      tab.suu[q] = d.suu[q];
      tab.weight[q] = d.weight[q];
    }
    const int nw = nwin < g.nwb ? nwin : g.nwb;
    const size_t lds = wn_lds(g, W + (nw - 1) * d.step);
    const dim3 grid((unsigned)(ntiles * nchunks), (unsigned)d.nspec);
    // (the increment under _NONE is _CONSTANT's: x_j - mean, slope +0.0)
    constexpr int DET = decltype(det)::value == PM_WIN_DETREND_LINEAR ? PM_WIN_DETREND_LINEAR
                                                                      : PM_WIN_DETREND_CONSTANT;
    return launch_dyn(k_series_dfa<DET>, grid, WN_THREADS, lds, st, d.v, (int)d.n, (int)d.nspec,
                      (int)d.k0, W, (int)d.step, nwin, g.nwb, nchunks, g.ltm, d.stt, (int)d.nq,
                      tab, alpha, f2);
  });
}

}  // extern "C"
