// shifts.hip -- the largest abrupt shift of a recorded index series, the series censored from a
// per-member end on, and the null-model fit of every member up to its own end, computed where the
// series lives (pymoc_amd.SeriesShifts, SeriesWindows.significance(until=)).
//
// (no counterpart: what a user does with a rolling two-window statistic and a per-member slice of
// the downloaded series.)  include/pymoc_hip.h states the three definitions; this file follows
// them operation by operation and is built with -ffp-contract=off.  Each double is reproduced bit
// for bit by the NumPy restatement (tests/shifts_cases.py); the integers are exact.
//
// K27 k_series_shift_scan.  The detector reads what k_series_windows wrote (the mean and the var
// plane of windows of L records, step 1), so no sum gets a second order here: a candidate costs
// four loads, a subtraction, an addition, a product, a sqrt and a division.  block x = a tile of
// 32 adjacent members, block y = the index; lane = mi + 32 * slot, and a thread takes the
// candidates L + slot, L + slot + 8, ..: every load is a row of 32 consecutive doubles.  The
// selection (largest score, the smallest record among equals; the smallest record at or above the
// threshold; the count) is order-independent under the tie rule, so the eight slots are reduced
// in LDS (static, 5 KiB); the member's first slot then forms the four values at `at` again from
// the planes -- the same operations, so the same bits.
//
// K28 k_series_censor.  y[j][p][m] has (p, m) contiguous: block x = the flat series i = p * n + m
// (the layout of k_series_surrogates: every record's load and store a coalesced row per wavefront
// whatever n is), block y = a chunk of 64 consecutive records.  A thread reads its series' end,
// copies its kept records as 64-bit words, four loads ahead of their stores, and stores NaN from
// `end` on; in place only the NaNs are stored.  Records are independent, so the chunking does not
// show.  No LDS.
//
// K29 k_series_fit_ranged.  A thread owns one (index, member), reads its end e and walks the
// records [k0, k0 + e) twice in ascending j -- the two passes of k_series_windows for ONE window of
// W = e records at lag 1, the sums in registers, every load a coalesced row.  No LDS.
#include <cmath>
#include "common.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int SH_TM = 32, SH_SLOTS = 8, SH_THREADS = SH_TM * SH_SLOTS;
constexpr int SH_BLOCK = 256;  // K28
constexpr int SH_RECORDS = 64; // K28: consecutive records of a series one thread takes
constexpr int FR_BLOCK = 64;   // K29: one wavefront, so that few series still spread over the CUs

// One candidate of the definition: the four values it reads, and what it forms from them.
struct ShCand {
  double stat, jump, before, after, score;
  bool counts;
};
// (mean and var: the member's window 0 in either plane, rs doubles between windows)
__device__ __forceinline__ ShCand sh_candidate(const double *__restrict__ mean,
                                               const double *__restrict__ var, size_t rs, int c,
                                               int L, int dir) {
  ShCand r;
  const size_t oa = (size_t)(c - L) * rs, ob = (size_t)c * rs;
  r.before = mean[oa];
  r.after = mean[ob];
  r.jump = r.after - r.before;
  const double pooled = 0.5 * (var[oa] + var[ob]);
  r.stat = r.jump / sqrt(pooled);
  r.score = dir < 0 ? -r.stat : dir > 0 ? r.stat : fabs(r.stat);
  r.counts = r.before == r.before && r.after == r.after && r.score == r.score;
  return r;
}

__global__ __launch_bounds__(SH_THREADS) void k_series_shift_scan(
    const double *__restrict__ mean_p, const double *__restrict__ var_p, int n, int nspec, int K,
    int L, const double *__restrict__ thr, const int32_t *__restrict__ dirs, int32_t *__restrict__ at_out,
    int32_t *__restrict__ first_out, int32_t *__restrict__ ncand_out, double *__restrict__ val) {
  __shared__ double l_score[SH_SLOTS][SH_TM];
  __shared__ int l_at[SH_SLOTS][SH_TM], l_first[SH_SLOTS][SH_TM], l_cnt[SH_SLOTS][SH_TM];
  const int tid = threadIdx.x;
  const int mi = tid & (SH_TM - 1), slot = tid / SH_TM;
  const int s = blockIdx.y, m0 = blockIdx.x * SH_TM;
  const size_t rs = (size_t)nspec * (size_t)n;  // doubles between windows
  const double *mean = series_row(mean_p, rs, n, 0, s, m0, mi);
  const double *var = series_row(var_p, rs, n, 0, s, m0, mi);
  const double t = thr[s];
  const int dir = dirs[s];
  double best = 0.0;
  int at = -1, first = 0x7fffffff, cnt = 0;
#pragma unroll 2
  for (int c = L + slot; c <= K - L; c += SH_SLOTS) {
    const ShCand r = sh_candidate(mean, var, rs, c, L, dir);
    if (r.counts) {
      ++cnt;
      if (at < 0 || r.score > best) {  // (ascending c: an equal score does not replace)
        best = r.score;
        at = c;
      }
      if (r.score >= t && c < first) first = c;  // (a NaN threshold compares false)
    }
  }
  l_score[slot][mi] = best;
  l_at[slot][mi] = at;
  l_first[slot][mi] = first;
  l_cnt[slot][mi] = cnt;
  __syncthreads();
  if (slot == 0 && m0 + mi < n) {
    for (int q = 1; q < SH_SLOTS; ++q) {
      const int a = l_at[q][mi];
      const double sc = l_score[q][mi];
      if (a >= 0 && (at < 0 || sc > best || (sc == best && a < at))) {
        best = sc;
        at = a;
      }
      first = l_first[q][mi] < first ? l_first[q][mi] : first;
      cnt += l_cnt[q][mi];
    }
    const size_t o = (size_t)s * n + m0 + mi;
    at_out[o] = at;
    first_out[o] = first == 0x7fffffff ? -1 : first;
    ncand_out[o] = cnt;
    const double nan = __builtin_nan("");
    ShCand r;
    r.stat = r.jump = r.before = r.after = nan;
    if (at >= 0) r = sh_candidate(mean, var, rs, at, L, dir);
    val[o] = r.stat;
    val[rs + o] = r.jump;
    val[2 * rs + o] = r.before;
    val[3 * rs + o] = r.after;
  }
}

// end of the definition, from where[src[s]][m]
__device__ __forceinline__ int censor_end(int w, int K, int guard) {
  if (w < 0) return K;
  const long long e = (long long)w - guard;
  return e < 0 ? 0 : e > K ? K : (int)e;
}

// (x and y may be the same array: no __restrict__ on either; the loads of a batch of four records
// are issued before its stores, since the compiler must take every store for a possible alias)
__global__ __launch_bounds__(SH_BLOCK) void k_series_censor(
    const unsigned long long *x, uint32_t n, uint32_t nspec, uint32_t total, int K, int rc,
    int guard, const int32_t *__restrict__ where, const int32_t *__restrict__ src,
    unsigned long long *y, int32_t *__restrict__ end_out) {
  // (total = nb * nspec * n < 2^31: no product below wraps)
  const uint32_t i = blockIdx.x * SH_BLOCK + threadIdx.x;
  if (i >= total) return;
  const uint32_t p = i / n, m = i - p * n;
  const uint32_t ib = p / nspec, s = p - ib * nspec;
  const int end = censor_end(where[(size_t)src[s] * n + m], K, guard);
  if (end_out && ib == 0 && blockIdx.y == 0) end_out[(size_t)s * n + m] = end;
  // the thread's records [j0, j1): kept below `end`, NaN from there on
  const long long jl = (long long)blockIdx.y * rc;
  const int j0 = (int)jl, j1 = jl + rc < K ? (int)(jl + rc) : K;
  const int je = end < j0 ? j0 : end < j1 ? end : j1;
  const unsigned long long nan = 0x7ff8000000000000ull;
  const size_t t = total;
  if (x != y) {
    size_t o = (size_t)i + (size_t)j0 * t;
    int j = j0;
    for (; j + 4 <= je; j += 4, o += 4 * t) {
      const unsigned long long a0 = x[o], a1 = x[o + t], a2 = x[o + 2 * t], a3 = x[o + 3 * t];
      y[o] = a0;
      y[o + t] = a1;
      y[o + 2 * t] = a2;
      y[o + 3 * t] = a3;
    }
    for (; j < je; ++j, o += t) y[o] = x[o];
  }
  size_t o = (size_t)i + (size_t)je * t;
#pragma unroll 4
  for (int j = je; j < j1; ++j, o += t) y[o] = nan;
}

template <int DET>
__global__ __launch_bounds__(FR_BLOCK) void k_series_fit_ranged(
    const double *__restrict__ v, uint32_t plane, size_t rs, int k0, int K,
    const int32_t *__restrict__ end, const double *__restrict__ stt_tab,
    double *__restrict__ var_out, double *__restrict__ ac_out) {
  const uint32_t i = blockIdx.x * FR_BLOCK + threadIdx.x;
  if (i >= plane) return;
  const int W = end[i];
  const double nan = __builtin_nan("");
  double var = nan, ac = nan;
  if (W >= PM_WIN_MIN && W <= K) {
    const double *xw = v + (size_t)k0 * rs + i;
    const double half = 0.5 * (double)(W - 1);
    // pass 1: the sums of x_j and of t_j * x_j
    double sum = 0.0, st = 0.0, t = 0.0 - half;
    bool fin = true;
#pragma unroll 4
    for (int j = 0; j < W; ++j) {
      const double xj = xw[(size_t)j * rs];
      fin = fin && series_finite(xj);
      sum = sum + xj;
      if (DET == PM_WIN_DETREND_LINEAR) {
        st = st + t * xj;
        t = t + 1.0;
      }
    }
    if (fin) {
      const double mean = sum / (double)W;
      const double slope = DET == PM_WIN_DETREND_LINEAR ? st / stt_tab[W] : 0.0;
      // pass 2: q = sum r_j r_j, c = sum_{j < W - 1} r_j r_{j + 1}
      double q = 0.0, c = 0.0;
      t = 0.0 - half;
      double prev = series_resid<DET>(xw[0], mean, slope, t);
      q = q + prev * prev;
#pragma unroll 4
      for (int j = 1; j < W; ++j) {
        t = t + 1.0;
        const double r = series_resid<DET>(xw[(size_t)j * rs], mean, slope, t);
        c = c + prev * r;
        q = q + r * r;
        prev = r;
      }
      var = q / (double)(W - 1);
      ac = c / q;
    }
  }
  var_out[i] = var;
  ac_out[i] = ac;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_shift_scan(const struct pm_series_shift_scan *dp, int32_t *at, int32_t *first,
                         int32_t *ncand, double *val, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_shift_scan &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int K = d.k1 - d.k0, L = d.half;
  PM_REQUIRE(L >= PM_WIN_MIN && L <= PM_SHIFT_HALF_MAX, "half-width %d outside [%d, %d]", L,
             PM_WIN_MIN, PM_SHIFT_HALF_MAX);
  PM_REQUIRE(2ll * L <= K, "the record window [%d, %d) holds %d records, fewer than 2 * %d", d.k0,
             d.k1, K, L);
  PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
  PM_REQUIRE((long long)(K - L + 1) * d.nspec < (1ll << 30),
             "nwin * nspec = %lld is not below 2^30", (long long)(K - L + 1) * d.nspec);
  PM_REQUIRE(d.mean && d.var, "mean or var is NULL");
  PM_REQUIRE(d.thr && d.thr_dev && d.dir && d.dir_dev, "thr or dir (host or device) is NULL");
  PM_REQUIRE(at && first && ncand && val, "at, first, ncand or val is NULL");
  for (int s = 0; s < d.nspec; ++s) {
    PM_REQUIRE(d.dir[s] >= -1 && d.dir[s] <= 1, "dir[%d] = %d is not -1, 0 or +1", s, d.dir[s]);
    PM_REQUIRE(!std::isinf(d.thr[s]), "thr[%d] is infinite", s);
  }
  hipStream_t st = resolve_stream(stream);
  const dim3 grid((unsigned)(((long long)d.n + SH_TM - 1) / SH_TM), (unsigned)d.nspec);
  hipLaunchKernelGGL(k_series_shift_scan, grid, dim3(SH_THREADS), 0, st, d.mean, d.var, (int)d.n,
                     (int)d.nspec, K, L, d.thr_dev, d.dir_dev, at, first, ncand, val);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

int pm_series_censor(const struct pm_series_censor *dp, double *y, int32_t *end_out,
                     pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_censor &d = *dp;
  PM_PLANES_REQUIRE_DIMS(d);
  PM_REQUIRE(d.K >= 1, "K %d < 1", d.K);
  PM_REQUIRE(d.guard >= 0, "guard %d < 0", d.guard);
  PM_PLANES_REQUIRE(d, d.K);
  PM_REQUIRE(d.x && d.where, "x or where is NULL");
  PM_REQUIRE(d.src && d.src_dev, "src (host or device) is NULL");
  PM_REQUIRE(y, "y is NULL");
  for (int s = 0; s < d.nspec; ++s)
    PM_REQUIRE(d.src[s] >= 0 && d.src[s] < d.nspec, "src[%d] = %d is outside [0, %d)", s, d.src[s],
               d.nspec);
  hipStream_t st = resolve_stream(stream);
  const uint32_t total = (uint32_t)(planes * d.n);
  // a thread takes SH_RECORDS consecutive records of its series (more where K / 65535 exceeds them)
  const int most = (int)(((long long)d.K + 65534) / 65535);
  const int rc = most > SH_RECORDS ? most : SH_RECORDS;
  const dim3 grid((total + SH_BLOCK - 1) / SH_BLOCK, (unsigned)((d.K + rc - 1) / rc));
  hipLaunchKernelGGL(k_series_censor, grid, dim3(SH_BLOCK), 0, st,
                     (const unsigned long long *)d.x, (uint32_t)d.n, (uint32_t)d.nspec, total,
                     (int)d.K, rc, (int)d.guard, d.where, d.src_dev, (unsigned long long *)y,
                     end_out);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

int pm_series_fit_ranged(const struct pm_series_fit_ranged *dp, double *var, double *ac,
                         pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_fit_ranged &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int K = d.k1 - d.k0;
  PM_REQUIRE(K <= PM_WIN_MAX, "the window [%d, %d) holds %d records, more than %d", d.k0, d.k1, K,
             PM_WIN_MAX);
  return series_by_detrend(d.detrend, [&](auto det) -> int {
    PM_REQUIRE((long long)d.nspec * d.n < (1ll << 31), "nspec * n = %lld is not below 2^31",
               (long long)d.nspec * d.n);
    PM_REQUIRE(d.v && d.end, "v or end is NULL");
    PM_REQUIRE(d.stt_tab && d.stt_tab_dev, "stt_tab (host or device) is NULL");
    PM_REQUIRE(var && ac, "var or ac is NULL");
    for (int W = PM_WIN_MIN; W <= K; ++W)
      PM_REQUIRE(d.stt_tab[W] == series_stt(W),
                 "stt_tab[%d] = %.17g is not W (W^2 - 1) / 12 = %.17g", W, d.stt_tab[W],
                 series_stt(W));
    hipStream_t st = resolve_stream(stream);
    const uint32_t plane = (uint32_t)d.nspec * (uint32_t)d.n;
    const size_t rs = (size_t)plane;
    hipLaunchKernelGGL(k_series_fit_ranged<decltype(det)::value>,
                       dim3((plane + FR_BLOCK - 1) / FR_BLOCK), dim3(FR_BLOCK), 0, st, d.v, plane,
                       rs, (int)d.k0, K, d.end, d.stt_tab_dev, var, ac);
    PM_HIP(hipGetLastError());
    return PM_OK;
  });
}

}  // extern "C"
