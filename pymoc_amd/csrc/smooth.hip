// smooth.hip -- Gaussian-kernel (any table-kernel) detrending of a recorded index series, computed
// where the series lives (pymoc_amd.SeriesSmooth, SeriesWindows(detrend="gaussian")).
//
// (no counterpart: what a user computes with scipy.ndimage.gaussian_filter1d or R's ksmooth over the
// downloaded series.)  One entry over a series v[k][s][m] (record, index, member; an
// IndexRecorder's device layout) and a record window [k0, k1).  include/pymoc_hip.h states the
// definition: per record j the two sequential sums num and den over the finite records in reach,
// in ascending i from +0.0, every product and sum rounded on its own (-ffp-contract=off), the
// weights read from the caller's table (no exp here).  Each double is reproduced bit for bit by the
// NumPy restatement (tests/smooth_cases.py).
//
// K26 k_series_smooth.  Records are independent by definition, so a block takes a RANGE of them:
// block x = (tile of TM adjacent members, chunk of NR consecutive records), block y = the index.
// The block (1024 threads) stages the records in reach of its chunk -- [j0 - H, j0 + nr + H) cut to
// [0, K), rows of TM adjacent members, a non-finite value as NaN -- and the weight table in LDS
// once:
//   x[r][mi]   r < rows, mi < TM          w[d]   d <= H
// and a thread owns one (member, record) at a time: lane = mi + TM * slot, 1024 / TM records in
// flight, slot + p * (1024 / TM) in pass p.  It walks its reach in ascending i, num and den in
// registers: up to j with the table index falling, behind j with it rising, so no |i - j| is
// formed.  Both walks read LDS only, members fastest over the lanes; the lanes of one record read
// one w[d] (a broadcast).  A staged NaN fails x == x, and the tap keeps num and den as they are by
// a select: left out, never added as zero times something.  A block that staged no such record
// (a flag in the LDS arena, behind the counts; no static LDS) walks without the selections: the
// same sums, bit for bit.  nbad is counted while staging, by the block whose chunk holds the
// record, summed in LDS per block and added to the zeroed output with one integer atomic per
// (member, block): integers, so no order to speak of.
//
// Decided: in an all-finite block a thread forms TWO consecutive records
// per walk from one LDS read of x_i and one of the table; den is formed per record even where
// interior records of an all-finite tile would share it.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int SM_THREADS = 1024;

// The tile of a launch, a function of H alone: TM adjacent members (32 .. 2) and NR consecutive
// records.  A candidate (TM, bytes of LDS -- half a CU's, two blocks to a CU, or all of it) holds
// R rows next to the table, the counts and the block's flag; a block never stages more than
// PM_SMOOTH_MAX rows (its reach is cut to the record window), so R >= PM_SMOOTH_MAX takes every
// record, and otherwise
// NR = R - 2 H, a multiple of the SM_THREADS / TM records in flight where it exceeds them.  Of the
// candidates, widest rows first and the half before the whole, the first is taken that keeps every
// thread busy (NR >= the records in flight) and fetches a byte of the series at most six times
// ((NR + 2 H) / NR); failing that, the widest rows with NR >= 1 in a whole CU's LDS.
struct SmGeom {
  int tm, ltm, nr;
};
inline SmGeom sm_candidate(int H, int ltm, size_t bytes) {
  SmGeom g;
  g.ltm = ltm;
  g.tm = 1 << ltm;
  g.nr = 0;
  const size_t fixed = sizeof(double) * (size_t)(H + 1) + sizeof(int) * (g.tm + 1);
  if (bytes <= fixed) return g;
  const long long R = (long long)((bytes - fixed) / (sizeof(double) * g.tm));
  if (R >= PM_SMOOTH_MAX) {
    g.nr = PM_SMOOTH_MAX;
    return g;
  }
  const int slots = SM_THREADS / g.tm;
  long long nr = R - 2ll * H;
  if (nr < 1) return g;
  if (nr > slots) nr -= nr % slots;
  g.nr = (int)nr;
  return g;
}
inline SmGeom sm_geometry(int H) {
  for (int ltm = 5; ltm >= 2; --ltm)
    for (size_t bytes : {LDS_PER_CU / 2, LDS_PER_CU}) {
      const SmGeom g = sm_candidate(H, ltm, bytes);
      if (g.nr == PM_SMOOTH_MAX) return g;
      if (g.nr >= SM_THREADS / g.tm && g.nr + 2ll * H <= 6ll * g.nr) return g;
    }
  for (int ltm = 5; ltm > 1; --ltm) {
    const SmGeom g = sm_candidate(H, ltm, LDS_PER_CU);
    if (g.nr) return g;
  }
  return sm_candidate(H, 1, LDS_PER_CU);  // 8191 rows of 2 beside 4096 weights: it fits
}
// The rows a block of a launch over K records stages at most, and its LDS: the rows, the table
// w[0 .. Hc], TM counts and the flag.  The kernel has no static LDS (the cross-compile test reads
// it off the compiler's report), so this is all a block asks for.
inline int sm_rows(const SmGeom &g, int K, int H) {
  const long long reach = (long long)g.nr + 2ll * H;
  return reach < K ? (int)reach : K;
}
inline size_t sm_lds(const SmGeom &g, int rows, int Hc) {
  return sizeof(double) * ((size_t)rows * g.tm + (size_t)(Hc + 1)) + sizeof(int) * (g.tm + 1);
}

// One tap of the definition: a record that is not finite (staged as NaN) is left out.  ALLFIN: the
// block staged no such record, and the selections -- half of a tap's vector instructions -- go.
template <bool ALLFIN>
__device__ __forceinline__ void sm_tap(double xi, double wd, double &num, double &den) {
  const double n1 = num + wd * xi, d1 = den + wd;
  if (ALLFIN) {
    num = n1;
    den = d1;
  } else {
    const bool ok = xi == xi;
    num = ok ? n1 : num;
    den = ok ? d1 : den;
  }
}

// trend_j of the record whose reach starts at xp (stride 1 << ltm): nl records before it, nh behind.
template <bool ALLFIN>
__device__ __forceinline__ double sm_trend(const double *xp, const double *w, int nl, int nh,
                                           int ltm) {
  double num = 0.0, den = 0.0;
  // i = lo .. j: the table index j - i falls to 0
#pragma unroll 4
  for (int q = 0; q <= nl; ++q) sm_tap<ALLFIN>(xp[q << ltm], w[nl - q], num, den);
  // i = j + 1 .. hi: it rises from 1
  const double *xq = xp + ((size_t)nl << ltm);
#pragma unroll 4
  for (int q = 1; q <= nh; ++q) sm_tap<ALLFIN>(xq[q << ltm], w[q], num, den);
  return num / den;  // 0 / 0 where no record in reach is finite
}

// H here is min(H, K - 1): no reach goes further, and lo, hi and every table index are the same.
template <bool TREND, bool RESID>
__global__ __launch_bounds__(SM_THREADS) void k_series_smooth(
    const double *__restrict__ v, int n, int nspec, int k0, int K, int H, int nr, int nchunks,
    int ltm, int rows, const double *__restrict__ wtab, double *__restrict__ trend,
    double *__restrict__ resid, int32_t *__restrict__ nbad) {
  extern __shared__ double sm_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int s = blockIdx.y;
  const int m0 = tile << ltm;
  const int j0 = chunk * nr;                              // the block's first record
  const int nrb = K - j0 < nr ? K - j0 : nr;              // and how many it takes (>= 1)
  const int r0 = j0 - H > 0 ? j0 - H : 0;                 // records staged: [r0, r1) inside [0, K)
  const int r1 = j0 + nrb + H < K ? j0 + nrb + H : K;     // (r1 - r0 <= rows)
  double *x = sm_lds_;
  double *w = x + ((size_t)rows << ltm);
  int *cnt = (int *)(w + (H + 1));
  int *flag = cnt + TM;                                   // set where a non-finite value is staged
  const size_t rs = (size_t)nspec * (size_t)n;            // doubles between records
  const int mi = tid & (TM - 1), slot = tid >> ltm, slots = SM_THREADS >> ltm;
  const double nan = __builtin_nan("");

  if (tid < TM) cnt[tid] = 0;
  if (tid == 0) *flag = 0;
  __syncthreads();
  int bad = 0, seen = 0;
  {
    const double *base = series_row(v, rs, n, k0 + r0, s, m0, mi);
    const int span = r1 - r0;
#pragma unroll 4
    for (int r = slot; r < span; r += slots) {
      const double xr = base[(size_t)r * rs];
      const bool fin = series_finite(xr);
      const int j = r0 + r;
      bad += (!fin && j >= j0 && j < j0 + nrb) ? 1 : 0;
      seen |= fin ? 0 : 1;
      x[(r << ltm) + mi] = fin ? xr : nan;
    }
  }
  for (int d = tid; d <= H; d += SM_THREADS) w[d] = wtab[d];
  if (seen) *flag = 1;  // (every writer stores the same value)
  __syncthreads();
  const bool allfin = *flag == 0;  // one answer for the block

  const bool live = m0 + mi < n;
  auto put = [&](int j, double xj, double tr) {
    if (live) {
      const size_t o = ((size_t)j * nspec + s) * n + m0 + mi;
      if (TREND) trend[o] = tr;
      if (RESID) resid[o] = xj - tr;  // xj is NaN where the record is not finite: so is this
    }
  };
  // records one at a time: every record of a block that staged a non-finite value, the odd last
  // one of a block that did not
  const int first = allfin ? (nrb & ~1) + slot : slot;
  for (int rl = first; rl < nrb; rl += slots) {
    const int j = j0 + rl;
    const int lo = j - H > 0 ? j - H : 0;
    const int hi = j + H < K - 1 ? j + H : K - 1;
    const double *xp = x + ((size_t)(lo - r0) << ltm) + mi;
    const int nl = j - lo, nh = hi - j;
    const double tr = allfin ? sm_trend<true>(xp, w, nl, nh, ltm) : sm_trend<false>(xp, w, nl, nh, ltm);
    put(j, xp[nl << ltm], tr);
  }
  // an all-finite block: the records a = ja and b = ja + 1 in ONE walk over [lo_a, hi_b].  Each of
  // the four sums takes its own terms in ascending i, as the definition has them; the weight of b
  // at i is that of a at i - 1 (|i - ja - 1| = |(i - 1) - ja|), so one read of x_i and one of the
  // table serve both.  The reaches differ by at most their first and their last record.
  if (allfin)
    for (int p = slot; p < (nrb >> 1); p += slots) {
      const int ja = j0 + 2 * p;
      const int lo_a = ja - H > 0 ? ja - H : 0, lo_b = ja + 1 - H > 0 ? ja + 1 - H : 0;
      const int hi_a = ja + H < K - 1 ? ja + H : K - 1, hi_b = ja + 1 + H < K - 1 ? ja + 1 + H : K - 1;
      const double *xp = x + ((size_t)(lo_a - r0) << ltm) + mi;
      const int nl = ja - lo_a, nh = hi_a - ja;
      double na = 0.0, da = 0.0, nb = 0.0, db = 0.0, wprev;
      int q = 0;
      if (lo_b > lo_a) {  // a alone takes i = lo_a
        wprev = w[nl];
        na = na + wprev * xp[0];
        da = da + wprev;
        q = 1;
      } else {            // both start at record 0: b's weight there is w[jb] = w[nl + 1], jb <= H
        wprev = w[nl + 1];
      }
#pragma unroll 4
      for (; q <= nl; ++q) {  // i <= ja: a's table index falls to 0
        const double xi = xp[q << ltm], wa = w[nl - q];
        na = na + wa * xi;
        da = da + wa;
        nb = nb + wprev * xi;
        db = db + wprev;
        wprev = wa;
      }
      const double *xq = xp + ((size_t)nl << ltm);
#pragma unroll 4
      for (int r = 1; r <= nh; ++r) {  // ja < i <= hi_a: it rises from 1
        const double xi = xq[r << ltm], wa = w[r];
        na = na + wa * xi;
        da = da + wa;
        nb = nb + wprev * xi;
        db = db + wprev;
        wprev = wa;
      }
      if (hi_b > hi_a) {  // b alone takes i = hi_b
        nb = nb + wprev * xq[(nh + 1) << ltm];
        db = db + wprev;
      }
      put(ja, xq[0], na / da);
      put(ja + 1, xq[1 << ltm], nb / db);
    }
  if (bad) atomicAdd(&cnt[mi], bad);
  __syncthreads();
  if (tid < TM && m0 + tid < n && cnt[tid]) atomicAdd(&nbad[(size_t)s * n + m0 + tid], cnt[tid]);
}

template <bool TREND, bool RESID>
int sm_launch(const struct pm_series_smooth &d, const SmGeom &g, int nchunks, long long ntiles,
              hipStream_t st, double *trend, double *resid, int32_t *nbad) {
  const int K = d.k1 - d.k0;
  const int Hc = d.half < K - 1 ? d.half : K - 1;
  const int rows = sm_rows(g, K, d.half);
  const size_t lds = sm_lds(g, rows, Hc);  // (what pm_series_smooth_lds_bytes reports)
  PM_REQUIRE(lds <= LDS_PER_CU, "a block would need %zu bytes of LDS, more than %zu", lds,
             (size_t)LDS_PER_CU);
  PM_HIP(hipMemsetAsync(nbad, 0, sizeof(int32_t) * (size_t)d.nspec * (size_t)d.n, st));
  return launch_dyn(k_series_smooth<TREND, RESID>,
                    dim3((unsigned)(ntiles * nchunks), (unsigned)d.nspec), SM_THREADS,
                    lds, st, d.v, (int)d.n, (int)d.nspec, (int)d.k0, K, Hc, g.nr,
                    nchunks, g.ltm, rows, d.w_dev, trend, resid, nbad);
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_smooth_geometry(int32_t half, int32_t *members, int32_t *records) {
  PM_REQUIRE(members && records, "members or records is NULL");
  PM_REQUIRE(half >= 1 && half <= PM_SMOOTH_HALF_MAX, "half-width %d outside [1, %d]", half,
             PM_SMOOTH_HALF_MAX);
  const SmGeom g = sm_geometry(half);
  *members = g.tm;
  *records = g.nr;
  return PM_OK;
}

int pm_series_smooth_lds_bytes(int32_t half, int32_t nrecords, size_t *bytes) {
  PM_REQUIRE(bytes, "bytes is NULL");
  PM_REQUIRE(half >= 1 && half <= PM_SMOOTH_HALF_MAX, "half-width %d outside [1, %d]", half,
             PM_SMOOTH_HALF_MAX);
  PM_REQUIRE(nrecords >= 1 && nrecords <= PM_SMOOTH_MAX, "%d records outside [1, %d]", nrecords,
             PM_SMOOTH_MAX);
  const SmGeom g = sm_geometry(half);
  *bytes = sm_lds(g, sm_rows(g, nrecords, half), half < nrecords - 1 ? half : nrecords - 1);
  return PM_OK;
}

int pm_series_smooth(const struct pm_series_smooth *dp, double *trend, double *resid,
                     int32_t *nbad, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_smooth &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int K = d.k1 - d.k0, H = d.half;
  PM_REQUIRE(K <= PM_SMOOTH_MAX, "the window [%d, %d) holds %d records, more than %d", d.k0, d.k1,
             K, PM_SMOOTH_MAX);
  PM_REQUIRE(H >= 1 && H <= PM_SMOOTH_HALF_MAX, "half-width %d outside [1, %d]", H,
             PM_SMOOTH_HALF_MAX);
  PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
  PM_REQUIRE(d.v && d.w && d.w_dev, "v or w (host or device) is NULL");
  PM_REQUIRE(trend || resid, "trend and resid are both NULL");
  PM_REQUIRE(nbad, "nbad is NULL");
  PM_REQUIRE(d.w[0] == 1.0, "w[0] = %.17g is not 1", d.w[0]);
  for (int i = 1; i <= H; ++i) {
    PM_REQUIRE(std::isfinite(d.w[i]) && d.w[i] > 0.0, "w[%d] = %g is not finite and > 0", i,
               d.w[i]);
    PM_REQUIRE(d.w[i] <= d.w[i - 1], "w[%d] = %.17g is above w[%d] = %.17g", i, d.w[i], i - 1,
               d.w[i - 1]);
  }
  const SmGeom g = sm_geometry(H);
  const int nchunks = (K + g.nr - 1) / g.nr;
  const long long ntiles = ((long long)d.n + g.tm - 1) / g.tm;
  PM_REQUIRE(ntiles * nchunks < (1ll << 31),
             "member tiles * record chunks = %lld is not below 2^31", ntiles * nchunks);
  hipStream_t st = resolve_stream(stream);
  if (trend && resid) return sm_launch<true, true>(d, g, nchunks, ntiles, st, trend, resid, nbad);
  if (trend) return sm_launch<true, false>(d, g, nchunks, ntiles, st, trend, resid, nbad);
  return sm_launch<false, true>(d, g, nchunks, ntiles, st, trend, resid, nbad);
}

}  // extern "C"
