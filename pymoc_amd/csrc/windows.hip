// windows.hip -- sliding-window early-warning indicators of a recorded index series and the
// Kendall trend of a series against its record number, computed where the series lives
// (pymoc_amd.SeriesWindows).
//
// (no counterpart: what a user computes with a rolling apply over the downloaded series.)
// Two entries over a series v[k][s][m] (record, index, member; an IndexRecorder's device layout)
// and a record window [k0, k1).  include/pymoc_hip.h states the definitions: per sliding window the
// two sequential passes (mean and slope, then the residual sums) with every product and sum
// rounded on its own (-ffp-contract=off), and the pair counts of the trend.  Each double is
// reproduced bit for bit by the NumPy restatement (tests/windows_cases.py); the counts are exact.
//
// K22 k_series_windows.  Windows are independent by definition, so a block takes a RANGE of them:
// block x = (tile of TM adjacent members, chunk of NWB consecutive windows), block y = the index.
// The block (1024 threads) stages the records its windows span -- W + (nw - 1) * S rows of TM
// adjacent members, TM * 8 >= 32 contiguous bytes per row, 256 bytes up to W = 639 -- in LDS once:
//   x[r][mi]     r < span, mi < TM
// and a thread owns one (member, window) at a time: lane = mi + TM * slot, 1024 / TM windows in
// flight, slot + p * (1024 / TM) in pass p.  It walks its window's W rows twice in ascending j,
// the sums in registers; both walks read LDS only, members fastest over the lanes, so a 32-lane
// half reads 32 / TM rows of TM consecutive doubles.  A byte of the series is fetched from global
// memory span / (nw * S) times (wn_geometry: at most 6 where every thread can be kept busy, 5 at
// W = 256, S = 1), and read from LDS about 3 W / S times.  nused is summed in LDS per block and
// added to the zeroed output with one integer atomic per (member, block): integers, so no order
// to speak of.
//
// K23 k_series_kendall.  block x = a tile of TM adjacent members, block y = the index.  The K
// records of the tile are staged in LDS, a non-finite value as NaN -- every comparison with a NaN
// is false, so such a pair counts nowhere without a branch.  A thread owns (member, a = slot,
// slot + 1024 / TM, ..) and walks b = a + 1 .. K - 1 counting the concordant and the tied pairs in
// int32 registers (K (K - 1) / 2 < 2^23); the counts are summed over the slots in LDS, and the
// discordant pairs are the finite pairs, nfin (nfin - 1) / 2, less those two.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"
#include "windows_geom.hip.h"

namespace pm {

template <int DET, bool LAG1>
__global__ __launch_bounds__(WN_THREADS) void k_series_windows(
    const double *__restrict__ v, int n, int nspec, int k0, int W, int S, int Lg, int nwin,
    int nwb, int nchunks, int ltm, double stt, double *__restrict__ out,
    int32_t *__restrict__ nused) {
  extern __shared__ double wn_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int s = blockIdx.y;
  const int m0 = tile << ltm;
  const int i0 = chunk * nwb;                             // the block's first window
  const int nw = nwin - i0 < nwb ? nwin - i0 : nwb;       // and how many it takes (>= 1)
  const int span = W + (nw - 1) * S;                      // records staged: all inside [k0, k1)
  double *x = wn_lds_;
  int *cnt = (int *)(x + ((size_t)span << ltm));
  const size_t rs = (size_t)nspec * (size_t)n;            // doubles between records
  const int mi = tid & (TM - 1), slot = tid >> ltm, slots = WN_THREADS >> ltm;

  // rows of TM adjacent members: series_row(v, rs, n, k0 + i0 * S, s, m0, mi), written out -- with
  // the record formed before the clamp the compiler schedules this kernel differently
  {
    const int mc = m0 + mi < n ? m0 + mi : n - 1;
    const double *base = v + (size_t)(k0 + i0 * S) * rs + (size_t)s * n + mc;
#pragma unroll 4
    for (int r = slot; r < span; r += slots) x[(r << ltm) + mi] = base[(size_t)r * rs];
  }
  if (tid < TM) cnt[tid] = 0;
  __syncthreads();

  const double nan = __builtin_nan("");
  const double half = 0.5 * (double)(W - 1);
  const bool live = m0 + mi < n;
  int used = 0;
  for (int wl = slot; wl < nw; wl += slots) {
    const double *xw = x + (((size_t)wl * S) << ltm) + mi;
    // pass 1: the sums of x_j and of t_j * x_j
    // (t_j = (double)j - half is formed by adding 1.0: multiples of a half below 2^12, so exact)
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
    double mean = nan, slope = nan, var = nan, ac = nan;
    if (fin) {
      mean = sum / (double)W;
      slope = DET == PM_WIN_DETREND_LINEAR ? st / stt : 0.0;
      // pass 2: q = sum r_j r_j, c = sum_{j < W - Lg} r_j r_{j + Lg}
      double q = 0.0, c = 0.0;
      t = 0.0 - half;
      if (LAG1) {
        double prev = series_resid<DET>(xw[0], mean, slope, t);
        q = q + prev * prev;
#pragma unroll 4
        for (int j = 1; j < W; ++j) {
          t = t + 1.0;
          const double r = series_resid<DET>(xw[j << ltm], mean, slope, t);
          c = c + prev * r;
          q = q + r * r;
          prev = r;
        }
      } else {
        const int nl = W - Lg;
        const double dl = (double)Lg;
#pragma unroll 2
        for (int j = 0; j < nl; ++j) {
          const double r = series_resid<DET>(xw[j << ltm], mean, slope, t);
          const double r2 = series_resid<DET>(xw[(j + Lg) << ltm], mean, slope, t + dl);
          q = q + r * r;
          c = c + r * r2;
          t = t + 1.0;
        }
#pragma unroll 2
        for (int j = nl; j < W; ++j) {
          const double r = series_resid<DET>(xw[j << ltm], mean, slope, t);
          q = q + r * r;
          t = t + 1.0;
        }
      }
      var = q / (double)(W - 1);
      ac = c / q;
      ++used;
    }
    if (live) {
      const size_t plane = (size_t)nwin * rs;
      double *o = out + ((size_t)(i0 + wl) * nspec + s) * n + m0 + mi;
      o[0] = mean;
      o[plane] = slope;
      o[2 * plane] = var;
      o[3 * plane] = ac;
    }
  }
  if (used) atomicAdd(&cnt[mi], used);
  __syncthreads();
  if (tid < TM && m0 + tid < n && cnt[tid]) atomicAdd(&nused[(size_t)s * n + m0 + tid], cnt[tid]);
}

template <int DET, bool LAG1>
int wn_launch(const struct pm_series_windows &d, int nwin, hipStream_t st, double *out,
              int32_t *nused) {
  const WnGeom g = wn_geometry(d.window, d.step);
  const int nchunks = (nwin + g.nwb - 1) / g.nwb;
  const long long ntiles = ((long long)d.n + g.tm - 1) / g.tm;
  PM_REQUIRE(ntiles * nchunks < (1ll << 31),
             "member tiles * window chunks = %lld is not below 2^31", ntiles * nchunks);
  const int nw = nwin < g.nwb ? nwin : g.nwb;
  const size_t lds = wn_lds(g, d.window + (nw - 1) * d.step);
  PM_HIP(hipMemsetAsync(nused, 0, sizeof(int32_t) * (size_t)d.nspec * (size_t)d.n, st));
  return launch_dyn(k_series_windows<DET, LAG1>,
                    dim3((unsigned)(ntiles * nchunks), (unsigned)d.nspec), WN_THREADS, lds, st,
                    d.v, (int)d.n, (int)d.nspec, (int)d.k0, (int)d.window, (int)d.step, (int)d.lag,
                    nwin, g.nwb, nchunks, g.ltm, d.stt, out, nused);
}

// ------------------------------------------------------------------ K23
// TM members by K records of LDS: at most 64 KiB up to K = 2048, 128 KiB above.
inline int kd_ltm(int K) { return K <= 256 ? 5 : K <= 512 ? 4 : K <= 1024 ? 3 : 2; }

__global__ __launch_bounds__(WN_THREADS) void k_series_kendall(
    const double *__restrict__ v, int n, int nspec, int k0, int K, int ltm,
    int32_t *__restrict__ conc_out, int32_t *__restrict__ disc_out, int32_t *__restrict__ tie_out,
    int32_t *__restrict__ nfin_out) {
  extern __shared__ double wn_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int s = blockIdx.y, m0 = blockIdx.x << ltm;
  double *x = wn_lds_;
  int *cnt = (int *)(x + ((size_t)K << ltm));  // [3][TM]: conc, tie, nfin
  const size_t rs = (size_t)nspec * (size_t)n;
  const int mi = tid & (TM - 1), slot = tid >> ltm, slots = WN_THREADS >> ltm;
  const double nan = __builtin_nan("");
  if (tid < 3 * TM) cnt[tid] = 0;
  int nfin = 0;
  {
    const double *base = series_row(v, rs, n, k0, s, m0, mi);
#pragma unroll 4
    for (int r = slot; r < K; r += slots) {
      const double xr = base[(size_t)r * rs];
      const bool fin = series_finite(xr);
      nfin += fin ? 1 : 0;
      x[(r << ltm) + mi] = fin ? xr : nan;
    }
  }
  __syncthreads();
  // two of the three counts: a pair of finite values that is neither concordant nor tied is
  // discordant, and the finite pairs are nfin (nfin - 1) / 2 -- integers, so exact
  int conc = 0, tie = 0;
  for (int a = slot; a < K - 1; a += slots) {
    const double xa = x[(a << ltm) + mi];
#pragma unroll 4
    for (int b = a + 1; b < K; ++b) {
      const double xb = x[(b << ltm) + mi];
      conc += xb > xa ? 1 : 0;
      tie += xb == xa ? 1 : 0;
    }
  }
  atomicAdd(&cnt[mi], conc);
  atomicAdd(&cnt[TM + mi], tie);
  atomicAdd(&cnt[2 * TM + mi], nfin);
  __syncthreads();
  if (tid < TM && m0 + tid < n) {
    const size_t o = (size_t)s * n + m0 + tid;
    const int nf = cnt[2 * TM + tid], c = cnt[tid], t = cnt[TM + tid];
    conc_out[o] = c;
    disc_out[o] = nf * (nf - 1) / 2 - c - t;
    tie_out[o] = t;
    nfin_out[o] = nf;
  }
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_windows_geometry(int32_t window, int32_t step, int32_t *members, int32_t *windows) {
  PM_REQUIRE(members && windows, "members or windows is NULL");
  PM_REQUIRE(window >= PM_WIN_MIN && window <= PM_WIN_MAX, "window %d outside [%d, %d]", window,
             PM_WIN_MIN, PM_WIN_MAX);
  PM_REQUIRE(step >= 1 && step <= window, "step %d outside [1, window = %d]", step, window);
  const WnGeom g = wn_geometry(window, step);
  *members = g.tm;
  *windows = g.nwb;
  return PM_OK;
}

int pm_series_windows(const struct pm_series_windows *dp, double *out, int32_t *nused,
                      pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_windows &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int W = d.window;
  PM_REQUIRE(W >= PM_WIN_MIN && W <= PM_WIN_MAX, "window length %d outside [%d, %d]", W,
             PM_WIN_MIN, PM_WIN_MAX);
  PM_REQUIRE(d.step >= 1 && d.step <= W, "step %d outside [1, window = %d]", d.step, W);
  PM_REQUIRE(d.lag >= 1 && d.lag <= W - 2, "lag %d outside [1, window - 2 = %d]", d.lag, W - 2);
  PM_REQUIRE(d.k1 - d.k0 >= W, "the record window [%d, %d) is shorter than the window length %d",
             d.k0, d.k1, W);
  return series_by_detrend(d.detrend, [&](auto det) -> int {
    PM_REQUIRE(d.stt == series_stt(W), "stt %.17g is not W (W^2 - 1) / 12 = %.17g", d.stt,
               series_stt(W));
    const int nwin = (d.k1 - d.k0 - W) / d.step + 1;
    PM_REQUIRE((long long)nwin * d.nspec < (1ll << 30), "nwin * nspec = %lld is not below 2^30",
               (long long)nwin * d.nspec);
    PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
    PM_REQUIRE(d.v, "v is NULL");
    PM_REQUIRE(out && nused, "out or nused is NULL");
    hipStream_t st = resolve_stream(stream);
    constexpr int DET = decltype(det)::value;
    return d.lag == 1 ? wn_launch<DET, true>(d, nwin, st, out, nused)
                      : wn_launch<DET, false>(d, nwin, st, out, nused);
  });
}

int pm_series_kendall(const struct pm_series_kendall *dp, int32_t *conc, int32_t *disc,
                      int32_t *tie, int32_t *nfin, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_kendall &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int K = d.k1 - d.k0;
  PM_REQUIRE(K <= PM_KENDALL_MAX, "the window [%d, %d) holds %d records, more than %d", d.k0, d.k1,
             K, PM_KENDALL_MAX);
  PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
  PM_REQUIRE(d.v, "v is NULL");
  PM_REQUIRE(conc && disc && tie && nfin, "conc, disc, tie or nfin is NULL");
  hipStream_t st = resolve_stream(stream);
  const int ltm = kd_ltm(K), tm = 1 << ltm;
  const size_t lds = sizeof(double) * (size_t)K * tm + sizeof(int) * 3 * tm;
  return launch_dyn(k_series_kendall,
                    dim3((unsigned)(((long long)d.n + tm - 1) / tm), (unsigned)d.nspec),
                    WN_THREADS, lds, st, d.v, (int)d.n, (int)d.nspec, (int)d.k0, K, ltm, conc,
                    disc, tie, nfin);
}

}  // extern "C"
