// fourier.hip -- Fourier phase-randomised surrogates of a recorded index series: the DFT
// coefficients of the detrended record window and the surrogates synthesised from them, both as
// device series (pymoc_amd.SeriesSurrogates(method="fourier"), SeriesWindows.significance(method=
// "fourier")).
//
// (no counterpart: what a user does with numpy.fft.rfft / irfft and a loop over the downloaded
// series.)  include/pymoc_hip.h states the two definitions; this file follows them operation by
// operation and is built with -ffp-contract=off.  Every double is reproduced bit for bit by the
// NumPy restatement (tests/fourier_cases.py).  The device calls no sin, cos, exp or sqrt: every
// trigonometric value is read from the caller's tables.
//
// A record window holds any K in [4, 4096], so the DFT of length K is Bluestein's chirp-z over a
// radix-2 transform of M points, M the smallest power of two >= 2K - 1 (and >= 8): fr_blu, ONE
// device function over complex series of M points held in LDS, which both kernels call.
//   z[t][pos]   TS series per block, each MP = M + M / 16 interleaved (re, im) pairs: 16 bytes a
//               point, read and written whole (ds_read_b128 / ds_write_b128).  Point i lives at
//               pos = i + (i >> 4): one pair of padding per 16, so that the 16 lanes one b128 LDS
//               cycle serves hit 16 distinct 16-byte slots in the strided passes -- at stride 4
//               (the first two-stage pass) lane l reads slot (4 l + l / 4) mod 16.
// TS = what 36 KiB hold, at least 1 and at most 16: 1 from M = 2048 up, 2 at 1024, 4 at 512, 8 at
// 256, 16 below; the block has a thread per radix-4 butterfly of its series, 64 to 1024 of them.
// Small blocks, several to a CU, so that one block's barrier leaves the LDS to the others: at
// M = 512 four series a block in 512 threads took 1.08 ms where sixteen in 1024 threads took 1.46 ms
// for the same launch, at M = 4096 one series a block 16.9 ms where two took 17.9 ms (DESIGN.md
// section 26).
//
// fr_blu: (a) a_j = x_j * chirp_j to position bitrev(j), +0 behind K.  bitrev is an involution, so
// a thread that owns j <= bitrev(j) reads both points and writes both: in place, no second buffer.
// (b) the log2 M butterfly stages in place, TWO to a pass through LDS as spectra.hip runs them: a
// thread holds the four points of a radix-4 butterfly and runs the four radix-2 butterflies of
// stages h and 2h on them in registers -- the definition's operations, so its bits -- with one
// barrier per pass (an odd log2 M starts with stage 1 alone).  (c) C_k = A_k * filt_k, conjugated,
// to position bitrev(k), pairwise as in (a).  (d) the stages again.  (e) fr_out(k): the conjugate
// scaled by 1 / M, times chirp_k, formed where the kernel stores it.  tw, chirp and filt are read
// from global memory: launch-invariant, 16 M + 16 K + 8 M bytes, resident in L2 -- the LDS is the
// series'.
//
// K30 k_series_fourier_coef.  A block owns TS ADJACENT flat series i = s * n + m: the record loads
// are rows of TS * 8 contiguous bytes -- 8 bytes a record and block from M = 2048 up, where TS = 1
// (the workload's M = 4096 among them).  The raw records go to LDS; one lane per series walks them
// for the sequential pass-1 sums of pm_series_windows (its mean and slope for one window of K
// records); the residual is formed inside (a).  Once per series: not the hot launch.
//
// K31 k_series_surrogates_fourier.  A block owns TS adjacent flat series i = p * n + m of the
// OUTPUT (plane p = surrogate * nspec + index; they run on into the next plane as in K24), reads
// their coefficients, rotates each by its Philox phase (two table reads and two complex
// products), mirrors the conjugate half, runs fr_blu with the conjugate tables and stores re / K.
// The coefficient reads (cs[f * rs]) and, stored directly, the records are rows of TS * 8 contiguous
// bytes: 8 bytes per block from M = 2048 up.  So the entry takes a scratch array of y's size: with
// one, K31<true> stores every series contiguously, scratch[i][j], a block's K records one run, and
// K32 k_series_fourier_transpose turns 32 x 32 tiles through LDS into y[j][i], both sides rows of
// 256 bytes.  Measured at M = 4096 (196608 series): 12.8 + 0.8 ms against 16.9 ms stored directly;
// the caller gives the scratch where a block holds one series (pymoc_amd.fourier.wants_scratch).
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "philox.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int FR_THREADS = 1024;
constexpr int FR_LTS_MAX = 4;
constexpr size_t FR_LDS_SERIES = 36 * 1024;  // of a block's series, where more than one fits

// M of a K: the smallest power of two >= 2K - 1, at least 8
inline int fr_m_of(int K) {
  int M = 8;
  while (M < 2 * K - 1) M <<= 1;
  return M;
}
inline int fr_log2(int M) {
  int l = 0;
  while ((1 << l) < M) ++l;
  return l;
}

struct FrGeom {
  int logm, lts, threads;
  size_t lds;
};
inline FrGeom fr_geometry(int M) {
  FrGeom g;
  g.logm = fr_log2(M);
  const size_t one = sizeof(double2) * (size_t)(M + (M >> 4));
  g.lts = 0;
  while (g.lts < FR_LTS_MAX && (one << (g.lts + 1)) <= FR_LDS_SERIES) ++g.lts;
  const int bfly = (M >> 2) << g.lts;
  g.threads = bfly < 64 ? 64 : (bfly > FR_THREADS ? FR_THREADS : bfly);
  // mean, slope [TS] and the flags [TS] behind the series
  g.lds = (one << g.lts) + (sizeof(double) * 2 + sizeof(int)) * ((size_t)1 << g.lts);
  return g;
}

__device__ __forceinline__ int fr_pad(int i) { return i + (i >> 4); }

// The complex product of the definition: every product and sum rounded on its own.
__device__ __forceinline__ double2 fr_mul(double2 x, double2 c) {
  return make_double2(x.x * c.x - x.y * c.y, x.x * c.y + x.y * c.x);
}

// (u, v) <- (u + W v, u - W v)
__device__ __forceinline__ void fr_bfly(double2 w, double2 &u, double2 &v) {
  const double tr = w.x * v.x - w.y * v.y;
  const double ti = w.x * v.y + w.y * v.x;
  v = make_double2(u.x - tr, u.y - ti);
  u = make_double2(u.x + tr, u.y + ti);
}

// The stages of the transform of M = 2^logm points over the block's 2^lts series, from bit-reversed
// order to natural order, in place.  Every thread of the block calls it; it ends with a barrier.
__device__ __forceinline__ void fr_stages(double2 *z, const double2 *__restrict__ tw, int logm,
                                          int lts, int MP) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int M = 1 << logm;
  int lh = 0;
  if (logm & 1) {
    const double2 w0 = tw[0];
    for (int t = tid; t < (M >> 1) << lts; t += nt) {
      double2 *zs = z + (t >> (logm - 1)) * MP;
      const int j = (t & ((M >> 1) - 1)) << 1;
      const int i0 = fr_pad(j), i1 = fr_pad(j + 1);
      double2 u = zs[i0], v = zs[i1];
      fr_bfly(w0, u, v);
      zs[i0] = u;
      zs[i1] = v;
    }
    __syncthreads();
    lh = 1;
  }
#pragma unroll 1
  for (; lh < logm; lh += 2) {
    const int h = 1 << lh;
    for (int t = tid; t < (M >> 2) << lts; t += nt) {
      double2 *zs = z + (t >> (logm - 2)) * MP;
      const int bt = t & ((M >> 2) - 1);
      const int q = bt & (h - 1);
      const int j0 = ((bt - q) << 2) + q;
      const int i0 = fr_pad(j0), i1 = fr_pad(j0 + h), i2 = fr_pad(j0 + 2 * h),
                i3 = fr_pad(j0 + 3 * h);
      const int ia = q << (logm - 1 - lh);  // stage h:  q * (M / (2h))
      const int ib = q << (logm - 2 - lh);  // stage 2h: q * (M / (4h)), and (q + h) * (M / (4h))
      const double2 wa = tw[ia], wb = tw[ib], wc = tw[ib + (M >> 2)];
      double2 p0 = zs[i0], p1 = zs[i1], p2 = zs[i2], p3 = zs[i3];
      fr_bfly(wa, p0, p1);
      fr_bfly(wa, p2, p3);
      fr_bfly(wb, p0, p2);
      fr_bfly(wc, p1, p3);
      zs[i0] = p0;
      zs[i1] = p1;
      zs[i2] = p2;
      zs[i3] = p3;
    }
    __syncthreads();
  }
}

template <bool INV>
__device__ __forceinline__ double2 fr_conj_if(double2 c) {
  return INV ? make_double2(c.x, -c.y) : c;
}

// BLU(x, sigma) of include/pymoc_hip.h over the block's series, sigma = +1 for INV.  On entry the
// caller's barrier lies behind the writes of the series; point j < K of series t is in(t, j,
// z[t][pad(j)]).  On return (behind a barrier) fr_out reads X_k.
template <bool INV, class IN>
__device__ __forceinline__ void fr_blu(double2 *z, int K, int logm, int lts, int MP,
                                       const double2 *__restrict__ tw,
                                       const double2 *__restrict__ chirp,
                                       const double2 *__restrict__ filt, IN in) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int M = 1 << logm;
  const double2 zero = make_double2(0.0, 0.0);
  for (int e = tid; e < M << lts; e += nt) {
    const int t = e >> logm, j = e & (M - 1);
    const int r = (int)(__brev((unsigned)j) >> (32 - logm));
    if (r < j) continue;
    double2 *zs = z + t * MP;
    const int pj = fr_pad(j), pr = fr_pad(r);
    const double2 aj = j < K ? fr_mul(in(t, j, zs[pj]), fr_conj_if<INV>(chirp[j])) : zero;
    const double2 ar = r < K ? fr_mul(in(t, r, zs[pr]), fr_conj_if<INV>(chirp[r])) : zero;
    zs[pr] = aj;
    zs[pj] = ar;
  }
  __syncthreads();
  fr_stages(z, tw, logm, lts, MP);
  for (int e = tid; e < M << lts; e += nt) {
    const int t = e >> logm, j = e & (M - 1);
    const int r = (int)(__brev((unsigned)j) >> (32 - logm));
    if (r < j) continue;
    double2 *zs = z + t * MP;
    const int pj = fr_pad(j), pr = fr_pad(r);
    const double2 cj = fr_mul(zs[pj], fr_conj_if<INV>(filt[j]));
    const double2 cr = fr_mul(zs[pr], fr_conj_if<INV>(filt[r]));
    zs[pr] = make_double2(cj.x, -cj.y);
    zs[pj] = make_double2(cr.x, -cr.y);
  }
  __syncthreads();
  fr_stages(z, tw, logm, lts, MP);
}

// X_k of the series zs after fr_blu: c_k = conj(F_k) * (1 / M), X_k = c_k * chirp_k
template <bool INV>
__device__ __forceinline__ double2 fr_out(const double2 *zs, int k, double inv_m,
                                          const double2 *__restrict__ chirp) {
  const double2 f = zs[fr_pad(k)];
  return fr_mul(make_double2(f.x * inv_m, (-f.y) * inv_m), fr_conj_if<INV>(chirp[k]));
}

__global__ __launch_bounds__(FR_THREADS) void k_series_fourier_coef(
    const double *__restrict__ v, uint32_t rs, int k0, int K, int logm, int lts, int det,
    double stt, const double2 *__restrict__ tw, const double2 *__restrict__ chirp,
    const double2 *__restrict__ filt, double *__restrict__ coef) {
  // (rs = nspec * n < 2^31: the flat series of the launch)
  extern __shared__ double2 fr_lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int M = 1 << logm, MP = M + (M >> 4), TS = 1 << lts;
  double2 *z = fr_lds;
  double *mean = (double *)(z + (size_t)MP * TS), *slope = mean + TS;
  int *bad = (int *)(slope + TS);
  const uint32_t i0 = blockIdx.x << lts;
  // rows of TS adjacent series; a series past the end reads the last one's records
  for (int e = tid; e < K << lts; e += nt) {
    const int t = e & (TS - 1), j = e >> lts;
    const uint32_t i = i0 + t < rs ? i0 + t : rs - 1;
    z[t * MP + fr_pad(j)] = make_double2(v[(size_t)(k0 + j) * rs + i], 0.0);
  }
  __syncthreads();
  const double half = 0.5 * (double)(K - 1);
  if (tid < TS) {
    // pass 1 of pm_series_windows for ONE window of K records: sequential in ascending j
    const double2 *zs = z + tid * MP;
    double sum = 0.0, st = 0.0, tj = 0.0 - half;
    bool fin = true;
#pragma unroll 8
    for (int j = 0; j < K; ++j) {
      const double xj = zs[fr_pad(j)].x;
      fin = fin && series_finite(xj);
      sum = sum + xj;
      st = st + tj * xj;
      tj = tj + 1.0;
    }
    mean[tid] = sum / (double)K;
    slope[tid] = det == PM_WIN_DETREND_LINEAR ? st / stt : 0.0;
    bad[tid] = fin ? 0 : 1;
  }
  __syncthreads();
  fr_blu<false>(z, K, logm, lts, MP, tw, chirp, filt, [&](int t, int j, double2 x) {
    const double tj = (double)j - half;
    const double r = det == PM_WIN_DETREND_LINEAR     ? (x.x - mean[t]) - slope[t] * tj
                     : det == PM_WIN_DETREND_CONSTANT ? x.x - mean[t]
                                                      : x.x;
    return make_double2(r, 0.0);
  });
  const int nf = K / 2 + 1;
  const double inv_m = 1.0 / (double)M;
  const double nan = __builtin_nan("");
  for (int e = tid; e < nf << lts; e += nt) {
    const int t = e & (TS - 1), f = e >> lts;
    if (i0 + t >= rs) continue;
    const double2 X = fr_out<false>(z + t * MP, f, inv_m, chirp);
    double *o = coef + (size_t)f * rs + i0 + t;
    o[0] = bad[t] ? nan : X.x;
    o[(size_t)nf * rs] = bad[t] ? nan : X.y;
  }
}

// word 0 of Philox4x32-10 keyed by (key0, key1) on the counter {id_lo, id_hi, b, w3}
__device__ __forceinline__ uint32_t fr_word0(uint32_t key0, uint32_t key1, uint64_t id, uint32_t b,
                                             uint32_t w3) {
  uint32_t c[4] = {(uint32_t)id, (uint32_t)(id >> 32), b, w3};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, key0, key1);
    key0 += 0x9E3779B9u;
    key1 += 0xBB67AE85u;
  }
  return c[0];
}

template <bool CONTIG>
__global__ __launch_bounds__(FR_THREADS) void k_series_surrogates_fourier(
    const double *__restrict__ coef, uint32_t n, uint32_t nspec, uint32_t total, int K, int logm,
    int lts, uint32_t b0, uint32_t key0, uint32_t key1, uint32_t id_lo, uint32_t id_hi,
    const double2 *__restrict__ tw, const double2 *__restrict__ chirp,
    const double2 *__restrict__ filt, const double2 *__restrict__ ph_hi,
    const double2 *__restrict__ ph_lo, double *__restrict__ y) {
  // (total = nb * nspec * n < 2^31: no product below wraps)
  extern __shared__ double2 fr_lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int M = 1 << logm, MP = M + (M >> 4), TS = 1 << lts;
  double2 *z = fr_lds;
  const uint32_t i0 = blockIdx.x << lts;
  const int nf = K / 2 + 1;
  {
    // a thread keeps its series (TS divides the block): a series past the end forms the last one's
    const int t = tid & (TS - 1);
    const uint32_t i = i0 + t < total ? i0 + t : total - 1;
    const uint32_t p = i / n, m = i - p * n;
    const uint32_t ib = p / nspec, s = p - ib * nspec;
    const uint32_t b = b0 + ib;  // (b0 + nb <= 2^32)
    const uint64_t id = (((uint64_t)id_hi << 32) | id_lo) + m;
    const size_t rs = (size_t)nspec * n;
    const double *cs = coef + (size_t)s * n + m;
    double2 *zs = z + t * MP;
    for (int f = tid >> lts; f < nf; f += nt >> lts) {
      const double2 R = make_double2(cs[(size_t)f * rs], cs[(size_t)(nf + f) * rs]);
      if (f == 0 || 2 * f == K) {
        zs[fr_pad(f)] = make_double2(R.x, 0.0);
      } else {
        const uint32_t q = fr_word0(key0, key1, id, b, (s << 12) | (uint32_t)f) >> 16;
        const double2 E = fr_mul(ph_hi[q >> 8], ph_lo[q & 255u]);
        const double2 Z = fr_mul(R, E);
        zs[fr_pad(f)] = Z;
        zs[fr_pad(K - f)] = make_double2(Z.x, -Z.y);
      }
    }
  }
  __syncthreads();
  fr_blu<true>(z, K, logm, lts, MP, tw, chirp, filt, [](int, int, double2 x) { return x; });
  const double inv_m = 1.0 / (double)M;
  const double dk = (double)K;
  for (int e = tid; e < K << lts; e += nt) {
    // CONTIG: y is the scratch [total][K], the records of a series running fastest over the lanes
    const int t = CONTIG ? e / K : e & (TS - 1), j = CONTIG ? e - t * K : e >> lts;
    if (i0 + t >= total) continue;
    const double2 X = fr_out<true>(z + t * MP, j, inv_m, chirp);
    y[CONTIG ? (size_t)(i0 + t) * K + j : (size_t)j * total + i0 + t] = X.x / dk;
  }
}

// K32: ys[total][K] -> y[K][total], tiles of 32 x 32 through LDS
constexpr int FR_TILE = 32;
__global__ __launch_bounds__(256) void k_series_fourier_transpose(const double *__restrict__ ys,
                                                                  uint32_t total, int K,
                                                                  double *__restrict__ y) {
  __shared__ double tile[FR_TILE][FR_TILE + 1];
  const uint32_t i0 = blockIdx.x * FR_TILE;
  const int j0 = blockIdx.y * FR_TILE;
  const int tx = threadIdx.x & (FR_TILE - 1), ty = threadIdx.x / FR_TILE;
  for (int r = ty; r < FR_TILE; r += 256 / FR_TILE)
    if (i0 + r < total && j0 + tx < K) tile[r][tx] = ys[(size_t)(i0 + r) * K + j0 + tx];
  __syncthreads();
  for (int r = ty; r < FR_TILE; r += 256 / FR_TILE)
    if (j0 + r < K && i0 + tx < total) y[(size_t)(j0 + r) * total + i0 + tx] = tile[tx][r];
}

// every value of a host table of `count` doubles is finite
inline int fr_table_finite(const double *tab, size_t count, const char *name) {
  for (size_t j = 0; j < count; ++j)
    PM_REQUIRE(std::isfinite(tab[j]), "%s[%zu] = %g is not finite", name, j, tab[j]);
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_fourier_coef(const struct pm_series_fourier_coef *dp, double *coef,
                           pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_fourier_coef &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int K = d.k1 - d.k0;
  PM_REQUIRE(K >= PM_WIN_MIN && K <= PM_SURROGATE_MAX,
             "the record window [%d, %d) holds %d records, outside [%d, %d]", d.k0, d.k1, K,
             PM_WIN_MIN, PM_SURROGATE_MAX);
  PM_REQUIRE(d.M == fr_m_of(K), "M %d is not %d, the smallest power of two >= 2K - 1 = %d", d.M,
             fr_m_of(K), 2 * K - 1);
  return series_by_detrend(d.detrend, [&](auto det) -> int {
    PM_REQUIRE(d.stt == series_stt(K), "stt %.17g is not K (K^2 - 1) / 12 = %.17g", d.stt,
               series_stt(K));
    PM_REQUIRE(d.nspec <= 65535, "nspec = %d > 65535", d.nspec);
    PM_REQUIRE((long long)d.nspec * d.n < (1ll << 31), "nspec * n = %lld is not below 2^31",
               (long long)d.nspec * d.n);
    PM_REQUIRE(d.v, "v is NULL");
    PM_REQUIRE(d.tw && d.chirp && d.filt, "tw, chirp or filt (host) is NULL");
    PM_REQUIRE(d.tw_dev && d.chirp_dev && d.filt_dev, "tw, chirp or filt (device) is NULL");
    PM_REQUIRE(coef, "coef is NULL");
    if (fr_table_finite(d.tw, (size_t)d.M, "tw") || fr_table_finite(d.chirp, 2 * (size_t)K, "chirp") ||
        fr_table_finite(d.filt, 2 * (size_t)d.M, "filt"))
      return PM_EINVAL;
    hipStream_t st = resolve_stream(stream);
    const FrGeom g = fr_geometry(d.M);
    const uint32_t rs = (uint32_t)d.nspec * (uint32_t)d.n;
    const uint32_t ts = 1u << g.lts;
    return launch_dyn(k_series_fourier_coef, dim3((rs + ts - 1) / ts), dim3((unsigned)g.threads),
                      g.lds, st, d.v, rs, (int)d.k0, K, g.logm, g.lts, (int)decltype(det)::value,
                      d.stt, (const double2 *)d.tw_dev, (const double2 *)d.chirp_dev,
                      (const double2 *)d.filt_dev, coef);
  });
}

int pm_series_surrogates_fourier(const struct pm_series_surrogates_fourier *dp, double *y,
                                 pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_surrogates_fourier &d = *dp;
  PM_PLANES_REQUIRE_DIMS(d);
  PM_REQUIRE(d.K >= PM_WIN_MIN && d.K <= PM_SURROGATE_MAX, "K %d outside [%d, %d]", d.K,
             PM_WIN_MIN, PM_SURROGATE_MAX);
  PM_REQUIRE(d.M == fr_m_of(d.K), "M %d is not %d, the smallest power of two >= 2K - 1 = %d", d.M,
             fr_m_of(d.K), 2 * d.K - 1);
  PM_REQUIRE(d.b0 >= 0 && d.b0 + (int64_t)d.nb <= (1ll << 32),
             "surrogates [%lld, %lld) are not inside [0, 2^32)", (long long)d.b0,
             (long long)d.b0 + d.nb);
  PM_REQUIRE(d.member0 >= 0, "member0 %lld < 0", (long long)d.member0);
  PM_PLANES_REQUIRE(d, d.K);
  PM_REQUIRE(d.coef, "coef is NULL");
  PM_REQUIRE(d.tw && d.chirp && d.filt && d.ph_hi && d.ph_lo,
             "tw, chirp, filt, ph_hi or ph_lo (host) is NULL");
  PM_REQUIRE(d.tw_dev && d.chirp_dev && d.filt_dev && d.ph_hi_dev && d.ph_lo_dev,
             "tw, chirp, filt, ph_hi or ph_lo (device) is NULL");
  PM_REQUIRE(y, "y is NULL");
  if (fr_table_finite(d.tw, (size_t)d.M, "tw") || fr_table_finite(d.chirp, 2 * (size_t)d.K, "chirp") ||
      fr_table_finite(d.filt, 2 * (size_t)d.M, "filt") || fr_table_finite(d.ph_hi, 512, "ph_hi") ||
      fr_table_finite(d.ph_lo, 512, "ph_lo"))
    return PM_EINVAL;
  hipStream_t st = resolve_stream(stream);
  const FrGeom g = fr_geometry(d.M);
  const uint32_t total = (uint32_t)(planes * d.n);
  const uint32_t ts = 1u << g.lts;
  const uint32_t key0 = (uint32_t)d.seed, key1 = (uint32_t)(d.seed >> 32);
  const uint32_t id_lo = (uint32_t)(uint64_t)d.member0;
  const uint32_t id_hi = (uint32_t)((uint64_t)d.member0 >> 32);
  const auto launch = [&](auto kernel, double *out) {
    return launch_dyn(kernel, dim3((total + ts - 1) / ts), dim3((unsigned)g.threads), g.lds, st,
                      d.coef, (uint32_t)d.n, (uint32_t)d.nspec, total, (int)d.K, g.logm, g.lts,
                      (uint32_t)d.b0, key0, key1, id_lo, id_hi, (const double2 *)d.tw_dev,
                      (const double2 *)d.chirp_dev, (const double2 *)d.filt_dev,
                      (const double2 *)d.ph_hi_dev, (const double2 *)d.ph_lo_dev, out);
  };
  if (!d.scratch) return launch(k_series_surrogates_fourier<false>, y);
  if (int rc = launch(k_series_surrogates_fourier<true>, d.scratch)) return rc;
  hipLaunchKernelGGL(k_series_fourier_transpose,
                     dim3((total + FR_TILE - 1) / FR_TILE, (unsigned)((d.K + FR_TILE - 1) / FR_TILE)),
                     dim3(256), 0, st, (const double *)d.scratch, total, (int)d.K, y);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
