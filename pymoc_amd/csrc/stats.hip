// stats.hip -- statistics of a recorded index series, reduced where the series lives
// (pymoc_amd.SeriesStats).
//
// (no counterpart: what a user computes in NumPy from the downloaded series -- the ensemble mean
// and spread over time, quantiles across realisations, a member's variance and autocovariance, the
// first record at which it leaves a state.)  Two entries over a series v[k][s][m] (record, index,
// member; an IndexRecorder's device layout) and a record window [k0, k1):
//   pm_series_group_stats   across the members of a group, per (record, index, group)
//   pm_series_member_stats  along the records, per (index, member)
// Every sum has ONE order, stated in include/pymoc_hip.h and independent of the launch geometry;
// with -ffp-contract=off every product and sum below is rounded on its own, so each double is
// reproduced bit for bit by the NumPy restatement (tests/stats_cases.py).
//
// Group statistics, one launch: block x = group, blocks y stride the (record, index) pairs.
//   G <= 64   one WAVEFRONT per (pair, group), four waves per block and up to eight pairs per wave
//             (the next pair's value is loaded ahead): lane j holds x_j; the sum tree
//             is an xor butterfly (p[l] + p[l ^ stride] is p[l] + p[l + stride] for l < stride, and
//             an addition commutes, so every lane ends with p[0]); the sort is a bitonic network on
//             64-bit keys through cross-lane exchanges (DPP for partners 1, 2 and 8 lanes away,
//             ds_bpermute for the others).  Registers only: no LDS allocation, no barrier.
//   G > 64    the BLOCK per (pair, group): the values go to LDS once; wave 0 forms the 64 residue
//             sums sequentially and runs the same butterfly; all 256 threads then sort the keys in
//             LDS (bitonic, the group size rounded up to a power of two, at most 64 KiB).
// The branch is uniform per block (a group has one size), so the barriers of the second form are
// reached by every thread.  Keys: the value's bits with the sign bit flipped (positive) or all
// bits flipped (negative) order as the values do with -0.0 before +0.0, and give the very bits
// back; a non-finite value gets the all-ones key, which sorts behind every finite one.
//
// Member statistics, one launch: a block is 32 members x 8 chunk slots for one index.  A chunk is
// PM_STATS_CHUNK = 256 consecutive records; a slot sums its chunk sequentially, eight chunks run at
// a time, and their partials are added to the total in ascending chunk order by every thread alike
// (so every thread of a member holds the same bits and nothing is broadcast).  Two passes: sum,
// count, extrema and threshold statistics, then -- with the mean -- squared deviations and lagged
// products.  Lanes run along the members: every load is a coalesced 256-byte row segment.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / WAVE;
constexpr unsigned long long KEY_LAST = ~0ull;

__device__ __forceinline__ unsigned long long st_key(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double st_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// The value of lane (l ^ J).  Strides 1 and 2 are DPP quad permutations ([1,0,3,2] = 0xB1,
// [2,3,0,1] = 0x4E) and stride 8 a DPP rotation of the 16-lane row by 8 (row_ror:8 = 0x128): moves
// inside the vector ALU.  The other strides go through the LDS crossbar (ds_bpermute), whose rate
// is the slower.  Every lane is active where these are called and every lane has a source, so the
// zero fill (bound_ctrl, which spares the move a preparatory copy) is never seen.
template <int J>
__device__ __forceinline__ int st_xor32(int x) {
  if constexpr (J == 1)
    return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);
  else if constexpr (J == 2)
    return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);
  else if constexpr (J == 8)
    return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, true);
  else
    return __shfl_xor(x, J, WAVE);
}

template <int J>
__device__ __forceinline__ unsigned long long st_xor(unsigned long long x) {
  const unsigned lo = (unsigned)st_xor32<J>((int)(unsigned)x);
  const unsigned hi = (unsigned)st_xor32<J>((int)(unsigned)(x >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

template <int J>
__device__ __forceinline__ double st_xor(double x) {
  return __longlong_as_double((long long)st_xor<J>((unsigned long long)__double_as_longlong(x)));
}

// strides 32 .. 1 of the tree, on the 64 residue sums held one per lane
__device__ __forceinline__ double st_tree(double p) {
  p += st_xor<32>(p);
  p += st_xor<16>(p);
  p += st_xor<8>(p);
  p += st_xor<4>(p);
  p += st_xor<2>(p);
  p += st_xor<1>(p);
  return p;
}

// one compare-exchange stage of the bitonic network: merge width K, partner lane ^ J
template <int K, int J>
__device__ __forceinline__ unsigned long long st_stage(unsigned long long key, int lane) {
  const unsigned long long other = st_xor<J>(key);
  // the lower lane of an ascending pair and the upper lane of a descending one keep the smaller
  // key; one compare decides (of equal keys either is the same bits)
  const bool keep_small = ((lane & K) == 0) == ((lane & J) == 0);
  return ((other < key) == keep_small) ? other : key;
}

template <int K, int J>
__device__ __forceinline__ unsigned long long st_merge(unsigned long long key, int lane) {
  key = st_stage<K, J>(key, lane);
  if constexpr (J > 1) key = st_merge<K, J / 2>(key, lane);
  return key;
}

// the 64 keys of a wavefront ascending by lane
__device__ __forceinline__ unsigned long long st_sort64(unsigned long long key, int lane) {
  key = st_merge<2, 1>(key, lane);
  key = st_merge<4, 2>(key, lane);
  key = st_merge<8, 4>(key, lane);
  key = st_merge<16, 8>(key, lane);
  key = st_merge<32, 16>(key, lane);
  key = st_merge<64, 32>(key, lane);
  return key;
}

// lane i's key, i the same in every lane: two v_readlane, no LDS crossbar
__device__ __forceinline__ unsigned long long st_lane(unsigned long long key, int i) {
  const int u = __builtin_amdgcn_readfirstlane(i);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), u);
  return ((unsigned long long)hi << 32) | lo;
}

// np.quantile's method="linear" on the m sorted finite values; at(i) returns sorted[i]
template <class At>
__device__ __forceinline__ double st_quantile(double q, int m, At at) {
  const double vi = q * (double)(m - 1);
  const double fl = floor(vi);
  const int lo = (int)fl;
  const int hi = lo + 1 < m - 1 ? lo + 1 : m - 1;
  const double g = vi - fl;
  const double a = at(lo), b = at(hi);
  return g >= 0.5 ? b - (b - a) * (1.0 - g) : a + (b - a) * g;
}

__device__ __forceinline__ void st_store_group(double *__restrict__ o, int32_t *__restrict__ cnt,
                                               int count, double sum, double mean, double var,
                                               double mn, double mx) {
  *cnt = count;
  const double nan = __builtin_nan("");
  o[0] = count ? mean : nan;
  o[1] = count >= 2 ? var : nan;
  o[2] = count ? mn : nan;
  o[3] = count ? mx : nan;
  o[4] = count ? sum : nan;
}

__global__ __launch_bounds__(GS_THREADS) void k_series_group_stats(
    const double *__restrict__ v, const int32_t *__restrict__ order,
    const int32_t *__restrict__ start, const double *__restrict__ q, int n, int nspec, int k0,
    int k1, int ngroups, int nq, int32_t *__restrict__ count_out, double *__restrict__ stat_out) {
  extern __shared__ unsigned long long lds[];  // the block form's values, then keys
  __shared__ int s_count;
  const int g = blockIdx.x;
  const int g0 = start[g], G = start[g + 1] - g0;
  const int npairs = (k1 - k0) * nspec;
  const int nst = 5 + nq;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;

  if (G <= WAVE) {
    // ---------------------------------------------------------------- one wavefront per pair
    const bool have = lane < G;
    const int m = have ? order[g0 + lane] : 0;
    // a wave takes several pairs, a grid's stride apart; the next pair's value is loaded before
    // this one's is reduced, so a load's latency is hidden behind a reduction
    const int step = gridDim.y * GS_WAVES;
    int p = blockIdx.y * GS_WAVES + wave;
    const size_t rec0 = (size_t)k0 * nspec;  // (record, index) pair: k * nspec + s
    double xn = (have && p < npairs) ? v[(rec0 + p) * (size_t)n + m] : __builtin_nan("");
    for (; p < npairs; p += step) {
      const size_t rec = rec0 + p;
      const double x = xn;
      xn = (have && p + step < npairs) ? v[(rec + step) * (size_t)n + m] : __builtin_nan("");
      const bool fin = have && series_finite(x);
      const int count = __popcll(__ballot(fin));
      const double sum = st_tree(0.0 + (fin ? x : 0.0));
      const double mean = sum / (double)count;
      const double d = fin ? x - mean : 0.0;
      const double Q = st_tree(0.0 + d * d);
      const double var = Q / (double)(count - 1);
      unsigned long long key = fin ? st_key(x) : KEY_LAST;
      key = st_sort64(key, lane);
      auto at = [&](int i) { return st_unkey(st_lane(key, i)); };
      const double mn = at(0), mx = at(count > 0 ? count - 1 : 0);
      const size_t o = rec * (size_t)ngroups + g;
      double *out = stat_out + o * nst;
      if (lane == 0) st_store_group(out, count_out + o, count, sum, mean, var, mn, mx);
      for (int i = 0; i < nq; ++i) {
        const double r = count ? st_quantile(q[i], count, at) : __builtin_nan("");
        if (lane == 0) out[5 + i] = r;
      }
    }
    return;
  }

  // -------------------------------------------------------------------- the block per pair
  int P2 = 2 * WAVE;
  while (P2 < G) P2 <<= 1;
  for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
    const size_t rec = (size_t)k0 * nspec + p;
    const double *row = v + rec * (size_t)n;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < G; j += GS_THREADS) {
      const double x = row[order[g0 + j]];
      lds[j] = (unsigned long long)__double_as_longlong(x);
      mine += series_finite(x) ? 1 : 0;
    }
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) mine += __shfl_xor(mine, s, WAVE);
    if (lane == 0) atomicAdd(&s_count, mine);
    __syncthreads();
    const int count = s_count;
    const size_t o = rec * (size_t)ngroups + g;
    double *out = stat_out + o * nst;
    if (wave == 0) {
      double pl = 0.0;
      for (int j = lane; j < G; j += WAVE) {
        const double x = __longlong_as_double((long long)lds[j]);
        pl += series_finite(x) ? x : 0.0;
      }
      const double sum = st_tree(pl);
      const double mean = sum / (double)count;
      double ql = 0.0;
      for (int j = lane; j < G; j += WAVE) {
        const double x = __longlong_as_double((long long)lds[j]);
        const double d = series_finite(x) ? x - mean : 0.0;
        ql += d * d;
      }
      const double Q = st_tree(ql);
      if (lane == 0) {
        const double nan = __builtin_nan("");
        count_out[o] = count;
        out[0] = count ? mean : nan;
        out[1] = count >= 2 ? Q / (double)(count - 1) : nan;
        out[4] = count ? sum : nan;
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < P2; j += GS_THREADS) {
      unsigned long long key = KEY_LAST;
      if (j < G) {
        const double x = __longlong_as_double((long long)lds[j]);
        if (series_finite(x)) key = st_key(x);
      }
      lds[j] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < P2; i += GS_THREADS) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const unsigned long long a = lds[i], b = lds[ixj];
            if ((a > b) == ((i & k) == 0)) {
              lds[i] = b;
              lds[ixj] = a;
            }
          }
        }
        __syncthreads();
      }
    }
    auto at = [&](int i) { return st_unkey(lds[i]); };
    if (threadIdx.x == 0) {
      const double nan = __builtin_nan("");
      out[2] = count ? at(0) : nan;
      out[3] = count ? at(count - 1) : nan;
    }
    if ((int)threadIdx.x < nq)
      out[5 + threadIdx.x] = count ? st_quantile(q[threadIdx.x], count, at) : __builtin_nan("");
    __syncthreads();  // the next pair overwrites lds and s_count
  }
}

// ------------------------------------------------------------------------- along the records
constexpr int MS_TM = 32;  // members per block
constexpr int MS_TC = 8;   // chunks in flight per block
constexpr int MS_SUMS = 1 + PM_STATS_LAG_MAX;

__global__ __launch_bounds__(MS_TM * MS_TC) void k_series_member_stats(
    const double *__restrict__ v, const int32_t *__restrict__ lag, const double *__restrict__ thr,
    const int32_t *__restrict__ dir, int n, int nspec, int k0, int k1, int nlag,
    int32_t *__restrict__ count_out, int32_t *__restrict__ first_out,
    int32_t *__restrict__ ncross_out, double *__restrict__ stat_out) {
  __shared__ double part[MS_SUMS][MS_TC][MS_TM];
  __shared__ int ipart[MS_SUMS][MS_TC][MS_TM];
  __shared__ double ext[2][MS_TC][MS_TM];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int s = blockIdx.y;
  const int m = blockIdx.x * MS_TM + tx;
  const bool live = m < n;  // (no early return: the block has barriers)
  const size_t rs = (size_t)nspec * (size_t)n;  // doubles between records
  const double *x0 = v + (size_t)s * n + (live ? m : 0);
  const int nchunks = (k1 - k0 + PM_STATS_CHUNK - 1) / PM_STATS_CHUNK;
  const double t = thr[s];
  const bool has_t = t == t;
  const bool below = dir[s] < 0;
  auto hit = [&](double x) { return has_t && series_finite(x) && (below ? x < t : x > t); };

  // pass 1: sum, count, extrema, threshold statistics
  double total = 0.0;
  int count = 0, hits = 0, first = 0x7fffffff, ncross = 0;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  for (int c0 = 0; c0 < nchunks; c0 += MS_TC) {
    const int c = c0 + ty;
    if (c < nchunks && live) {
      const int ka = k0 + c * PM_STATS_CHUNK;
      const int kb = ka + PM_STATS_CHUNK < k1 ? ka + PM_STATS_CHUNK : k1;
      double acc = 0.0;
      double x = x0[(size_t)ka * rs];
#pragma unroll 4
      for (int k = ka; k < kb; ++k) {
        // (the last record's successor: the record itself, read and discarded)
        const double xl = x0[(size_t)(k + 1 < k1 ? k + 1 : k) * rs];
        const double xn = k + 1 < k1 ? xl : __builtin_nan("");
        const bool fin = series_finite(x);
        acc += fin ? x : 0.0;
        if (fin) {
          ++count;
          if (x < mn || (x == mn && __builtin_signbit(x))) mn = x;
          if (x > mx || (x == mx && !__builtin_signbit(x))) mx = x;
          const bool h = hit(x);
          if (h) {
            ++hits;
            first = k < first ? k : first;
          }
          if (series_finite(xn) && h != hit(xn)) ++ncross;
        }
        x = xn;
      }
      part[0][ty][tx] = acc;
    }
    __syncthreads();
    const int nc = nchunks - c0 < MS_TC ? nchunks - c0 : MS_TC;
    for (int i = 0; i < nc; ++i) total += part[0][i][tx];
    __syncthreads();
  }
  // the order-free partials of the slots, combined by every thread alike
  ipart[0][ty][tx] = count;
  ipart[1][ty][tx] = hits;
  ipart[2][ty][tx] = first;
  ipart[3][ty][tx] = ncross;
  ext[0][ty][tx] = mn;
  ext[1][ty][tx] = mx;
  __syncthreads();
  count = hits = ncross = 0;
  first = 0x7fffffff;
  mn = __builtin_inf();
  mx = -__builtin_inf();
  for (int i = 0; i < MS_TC; ++i) {
    count += ipart[0][i][tx];
    hits += ipart[1][i][tx];
    first = ipart[2][i][tx] < first ? ipart[2][i][tx] : first;
    ncross += ipart[3][i][tx];
    const double a = ext[0][i][tx], b = ext[1][i][tx];
    if (a < mn || (a == mn && __builtin_signbit(a))) mn = a;
    if (b > mx || (b == mx && !__builtin_signbit(b))) mx = b;
  }
  __syncthreads();
  const double mean = total / (double)count;  // 0 / 0 = NaN with no finite record

  // pass 2: squared deviations and lagged products about the mean
  double tot2[MS_SUMS];
  int npair[MS_SUMS];
#pragma unroll
  for (int i = 0; i < MS_SUMS; ++i) {
    tot2[i] = 0.0;
    npair[i] = 0;
  }
  for (int c0 = 0; c0 < nchunks; c0 += MS_TC) {
    const int c = c0 + ty;
    if (c < nchunks && live) {
      const int ka = k0 + c * PM_STATS_CHUNK;
      const int kb = ka + PM_STATS_CHUNK < k1 ? ka + PM_STATS_CHUNK : k1;
      double acc = 0.0;
#pragma unroll 4
      for (int k = ka; k < kb; ++k) {
        const double x = x0[(size_t)k * rs];
        const double d = series_finite(x) ? x - mean : 0.0;
        acc += d * d;
      }
      part[0][ty][tx] = acc;
#pragma unroll
      for (int i = 0; i < PM_STATS_LAG_MAX; ++i) {
        if (i < nlag) {
          const int L = lag[i];
          double a = 0.0;
          int np = 0;
          const int ke = kb < k1 - L ? kb : k1 - L;
#pragma unroll 4
          for (int k = ka; k < ke; ++k) {
            const double x = x0[(size_t)k * rs], y = x0[(size_t)(k + L) * rs];
            const bool ok = series_finite(x) && series_finite(y);
            a += ok ? (x - mean) * (y - mean) : 0.0;
            np += ok ? 1 : 0;
          }
          part[1 + i][ty][tx] = a;
          npair[1 + i] += np;
        }
      }
    }
    __syncthreads();
    const int nc = nchunks - c0 < MS_TC ? nchunks - c0 : MS_TC;
#pragma unroll
    for (int j = 0; j < MS_SUMS; ++j)
      if (j <= nlag)
        for (int i = 0; i < nc; ++i) tot2[j] += part[j][i][tx];
    __syncthreads();
  }
#pragma unroll
  for (int j = 1; j < MS_SUMS; ++j) ipart[j][ty][tx] = npair[j];
  __syncthreads();
  if (ty != 0 || !live) return;  // (no barrier below)
  const size_t o = (size_t)s * n + m;
  const double nan = __builtin_nan("");
  count_out[o] = count;
  first_out[o] = first == 0x7fffffff ? -1 : first;
  ncross_out[o] = ncross;
  double *out = stat_out + o * (size_t)(6 + nlag);
  out[0] = mean;
  out[1] = count >= 2 ? tot2[0] / (double)(count - 1) : nan;
  out[2] = count ? mn : nan;
  out[3] = count ? mx : nan;
  out[4] = total;
  out[5] = has_t ? (double)hits / (double)count : nan;
#pragma unroll
  for (int j = 1; j < MS_SUMS; ++j) {
    if (j <= nlag) {
      int np = 0;
      for (int i = 0; i < MS_TC; ++i) np += ipart[j][i][tx];
      out[5 + j] = np ? tot2[j] / (double)np : nan;
    }
  }
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_group_stats(const struct pm_series_group_stats *dp, int32_t *count, double *stat,
                          pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_group_stats &d = *dp;
  PM_SERIES_REQUIRE(d);
  PM_REQUIRE(d.ngroups >= 1, "ngroups %d < 1", d.ngroups);
  PM_REQUIRE((long long)(d.k1 - d.k0) * d.nspec < (1ll << 30),
             "(k1 - k0) * nspec = %lld is not below 2^30", (long long)(d.k1 - d.k0) * d.nspec);
  PM_REQUIRE(d.nq >= 0 && d.nq <= PM_STATS_Q_MAX, "nq %d outside [0, %d]", d.nq, PM_STATS_Q_MAX);
  PM_REQUIRE(d.v && d.order && d.start && d.start_dev, "v, order or start is NULL");
  PM_REQUIRE(d.nq == 0 || (d.q && d.q_dev), "q is NULL (host or device)");
  PM_REQUIRE(count && stat, "count or stat is NULL");
  for (int i = 0; i < d.nq; ++i)
    PM_REQUIRE(d.q[i] >= 0.0 && d.q[i] <= 1.0, "q[%d] = %g is not in [0, 1]", i, d.q[i]);
  PM_REQUIRE(d.start[0] == 0, "start[0] = %d, not 0", d.start[0]);
  int gmax = 0;
  for (int g = 0; g < d.ngroups; ++g) {
    const int G = d.start[g + 1] - d.start[g];
    PM_REQUIRE(G >= 0, "start is not monotone at group %d", g);
    PM_REQUIRE(G <= PM_STATS_GROUP_MAX, "group %d has %d members, more than %d", g, G,
               PM_STATS_GROUP_MAX);
    gmax = G > gmax ? G : gmax;
  }
  PM_REQUIRE(d.start[d.ngroups] == d.n, "start ends at %d, not at n = %d", d.start[d.ngroups],
             d.n);
  size_t lds_bytes = 0;
  if (gmax > WAVE) {
    size_t p2 = 2 * WAVE;
    while (p2 < (size_t)gmax) p2 <<= 1;
    lds_bytes = p2 * sizeof(unsigned long long);
  }
  const long long npairs = (long long)(d.k1 - d.k0) * d.nspec;
  // blocks y.  Groups in blocks: a pair per block.  Groups in waves: four waves per block and up
  // to eight pairs per wave (loads run ahead of the reductions), fewer while that would leave the
  // device short of waves.  At most 65535; the loops stride on.  (The results do not depend on it.)
  long long gy = npairs;
  if (gmax <= WAVE) {
    long long per = 8;
    gy = (npairs + GS_WAVES * per - 1) / (GS_WAVES * per);
    while (per > 1 && (long long)d.ngroups * gy * GS_WAVES < 16384) {
      per >>= 1;
      gy = (npairs + GS_WAVES * per - 1) / (GS_WAVES * per);
    }
  }
  const long long cap = 1 + (1 << 20) / d.ngroups;  // ~1M blocks are plenty
  if (gy > cap) gy = cap;
  if (gy > 65535) gy = 65535;
  // (the block form also has a few static bytes: with 64 KiB of keys the total is above what a
  // kernel gets without asking)
  if (lds_bytes >= LDS_DYN_UNRAISED)
    PM_HIP(hipFuncSetAttribute((const void *)k_series_group_stats,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(k_series_group_stats, dim3((unsigned)d.ngroups, (unsigned)gy),
                     dim3(GS_THREADS), lds_bytes, resolve_stream(stream), d.v, d.order,
                     d.start_dev, d.q_dev, (int)d.n, (int)d.nspec, (int)d.k0, (int)d.k1,
                     (int)d.ngroups, (int)d.nq, count, stat);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

int pm_series_member_stats(const struct pm_series_member_stats *dp, int32_t *count, int32_t *first,
                           int32_t *ncross, double *stat, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_member_stats &d = *dp;
  PM_SERIES_REQUIRE(d);
  PM_REQUIRE(d.nlag >= 0 && d.nlag <= PM_STATS_LAG_MAX, "nlag %d outside [0, %d]", d.nlag,
             PM_STATS_LAG_MAX);
  PM_REQUIRE(d.nspec <= 65535, "nspec %d > 65535", d.nspec);
  PM_REQUIRE(d.v && d.thr && d.thr_dev && d.dir && d.dir_dev, "v, thr or dir is NULL");
  PM_REQUIRE(d.nlag == 0 || (d.lag && d.lag_dev), "lag is NULL (host or device)");
  PM_REQUIRE(count && first && ncross && stat, "count, first, ncross or stat is NULL");
  for (int i = 0; i < d.nlag; ++i)
    PM_REQUIRE(d.lag[i] >= 1 && d.lag[i] < d.k1 - d.k0, "lag[%d] = %d is not in [1, %d)", i,
               d.lag[i], d.k1 - d.k0);
  for (int s = 0; s < d.nspec; ++s)
    PM_REQUIRE(d.dir[s] == -1 || d.dir[s] == 1, "dir[%d] = %d is neither -1 nor +1", s, d.dir[s]);
  hipLaunchKernelGGL(k_series_member_stats,
                     dim3((unsigned)((d.n + MS_TM - 1) / MS_TM), (unsigned)d.nspec),
                     dim3(MS_TM, MS_TC), 0, resolve_stream(stream), d.v, d.lag_dev, d.thr_dev,
                     d.dir_dev, (int)d.n, (int)d.nspec, (int)d.k0, (int)d.k1, (int)d.nlag, count,
                     first, ncross, stat);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
