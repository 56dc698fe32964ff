// spectra.hip -- Welch power and cross spectra of a recorded index series, computed where the
// series lives (pymoc_amd.SeriesSpectra).
//
// (no counterpart: what a user computes with scipy.signal.welch / csd from the downloaded series.)
// One entry, pm_series_spectra, over a series v[k][s][m] (record, index, member; an IndexRecorder's
// device layout) and a record window [k0, k1).  include/pymoc_hip.h states the definition: the
// segments, the detrending, the iterative radix-2 decimation-in-time transform with every product
// and sum rounded on its own (-ffp-contract=off), the periodogram and the order of the sum over the
// used segments.  Each double is reproduced bit for bit by the NumPy restatement
// (tests/spectra_cases.py).
//
// One launch: block x = a tile of TM adjacent members, block y = a JOB -- the auto spectrum of one
// index, or one pair of indices.  A lane that walked one member's records would touch one cache
// line per value (records are nspec * n doubles apart), so the block loads a segment as L rows of
// TM adjacent members -- TM * 8 >= 64 contiguous bytes per row -- and turns it through LDS:
//   re[mi][pos], im[mi][pos]   one complex series of L points per member of the tile, a row
//                              LP = L + PAD doubles long
// The load writes x_j to pos = bitrev(j), the order the transform starts from.  The mean is the
// sequential sum the header states (one lane per member), the window pass forms y in place, and
// the log2 L butterfly stages run in place, TWO to a pass through LDS: a thread holds the four
// points of a radix-4 butterfly and runs the four radix-2 butterflies of stages h and 2h on them
// in registers -- the definition's operations, so its bits -- with one barrier per pass (an odd
// log2 L starts with stage 1 alone).  Consecutive lanes take consecutive butterflies of one
// member's series: from h = 64 on a wavefront reads and writes runs of 64 consecutive doubles,
// below that runs of h doubles, 4h apart.  The periodogram is
// read back with the MEMBER running fastest over the lanes -- the output rows are members
// contiguous -- and PAD = max(1, 32 / TM) puts the TM * (32 / TM) doubles a 32-lane half reads at
// once on distinct banks.  The averages over the segments are accumulated in registers (L is a
// template argument, so every register array has a constant size and nothing goes to scratch); no
// transform is ever stored to global memory.
//
// A pair job runs the same load / detrend / transform for its first series, keeps that spectrum
// in registers, runs it again for the second, and accumulates conj(Za) * Zb.
//
// TM = 2048 / L clamped to [8, 64]: 32 KiB of series per block up to L = 256, 64 KiB at L = 512,
// 128 KiB at L = 1024.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"

namespace pm {

constexpr int SP_THREADS = 256;

template <int L>
struct SpGeom {
  static constexpr int LOG = L == 8 ? 3 : L == 16 ? 4 : L == 32 ? 5 : L == 64 ? 6 : L == 128 ? 7
                             : L == 256 ? 8 : L == 512 ? 9 : 10;
  static constexpr int TM = 2048 / L < 8 ? 8 : (2048 / L > 64 ? 64 : 2048 / L);
  static constexpr int PAD = 32 / TM < 1 ? 1 : 32 / TM;
  static constexpr int LP = L + PAD;
  static constexpr int NF = L / 2 + 1;
  static constexpr int R = (TM * NF + SP_THREADS - 1) / SP_THREADS;  // spectrum values per thread
  // re, im, the twiddle table, the means, then the int flags and counts
  static constexpr size_t LDS = sizeof(double) * (2 * TM * LP + L + TM) + sizeof(int) * 4 * TM;
  // blocks of four waves per CU the registers are to allow: three up to L = 256 (the LDS would hold
  // four, but below 128 VGPRs a thread the compiler spills to scratch)
  static constexpr int WAVES_PER_SIMD = L <= 256 ? 3 : 1;
};

// One butterfly of the definition: (u, v) <- (u + W v, u - W v), every product and sum rounded on
// its own.
__device__ __forceinline__ void sp_bfly(double wr, double wi, double &ur, double &ui, double &vr,
                                        double &vi) {
  const double tr = wr * vr - wi * vi;
  const double ti = wr * vi + wi * vr;
  vr = ur - tr;
  vi = ui - ti;
  ur = ur + tr;
  ui = ui + ti;
}

// One series of the tile, records kb .. kb + L - 1 of index s: load, detrend, window, transform.
// On return re / im hold Z (natural order) and bad[mi] is nonzero where a value was not finite.
// Every thread of the block calls it; it ends with a barrier.
template <int L>
__device__ __forceinline__ void sp_transform(const double *__restrict__ v,
                                             const double *__restrict__ w, size_t rs, int n, int s,
                                             int m0, int kb, bool detrend, double *re, double *im,
                                             const double *twr, const double *twi, double *mu,
                                             int *bad) {
  using G = SpGeom<L>;
  constexpr int TM = G::TM, LP = G::LP;
  const int tid = threadIdx.x;
  // rows of TM adjacent members, turned into one series per member, bit-reversed.  A thread keeps
  // its member (TM divides the block) and takes every (256 / TM)-th record; the loads of a chunk
  // are issued together, free of branches, before the first of them is waited for.
  constexpr int NL = TM * L / SP_THREADS, CH = NL < 8 ? NL : 8;
  const int mi = tid % TM;
  const double *base = series_row(v, rs, n, kb, s, m0, mi);
  bool fin = true;
#pragma unroll 1
  for (int c = 0; c < NL; c += CH) {
    double x[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u)
      x[u] = base[(size_t)(tid / TM + (c + u) * (SP_THREADS / TM)) * rs];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int j = tid / TM + (c + u) * (SP_THREADS / TM);
      re[mi * LP + (int)(__brev((unsigned)j) >> (32 - G::LOG))] = x[u];
      fin = fin && series_finite(x[u]);
    }
  }
  if (!fin) bad[mi] = 1;
  __syncthreads();
  if (detrend) {
    if (tid < TM) {
      double sum = 0.0;
#pragma unroll 8
      for (int j = 0; j < L; ++j)
        sum = sum + re[tid * LP + (int)(__brev((unsigned)j) >> (32 - G::LOG))];
      mu[tid] = sum / (double)L;
    }
    __syncthreads();
  }
#pragma unroll 4
  for (int e = tid; e < TM * L; e += SP_THREADS) {
    const int mi = e / L, pos = e % L;
    const int j = (int)(__brev((unsigned)pos) >> (32 - G::LOG));
    const double x = re[mi * LP + pos];
    re[mi * LP + pos] = detrend ? (x - mu[mi]) * w[j] : x * w[j];
    im[mi * LP + pos] = 0.0;
  }
  __syncthreads();
  // The stages, two at a time: a thread holds the four points b + q + {0, h, 2h, 3h} of a block
  // of 4h, runs the two butterflies of stage h and the two of stage 2h on them in registers -- the
  // very operations of the definition, in its order for every point -- and a pass through LDS and a
  // barrier serve two stages.  An odd number of stages starts with stage h = 1 alone.
  int lh = 0;
  if (G::LOG & 1) {
#pragma unroll 2
    for (int t = tid; t < TM * (L / 2); t += SP_THREADS) {
      const int i0 = (t / (L / 2)) * LP + ((t % (L / 2)) << 1), i1 = i0 + 1;
      double ur = re[i0], ui = im[i0], vr = re[i1], vi = im[i1];
      sp_bfly(twr[0], twi[0], ur, ui, vr, vi);
      re[i0] = ur;
      im[i0] = ui;
      re[i1] = vr;
      im[i1] = vi;
    }
    __syncthreads();
    lh = 1;
  }
#pragma unroll 1
  for (; lh < G::LOG; lh += 2) {
    const int h = 1 << lh;
#pragma unroll 2
    for (int t = tid; t < TM * (L / 4); t += SP_THREADS) {
      const int mi = t / (L / 4), bt = t % (L / 4);
      const int q = bt & (h - 1);
      const int i0 = mi * LP + ((bt - q) << 2) + q, i1 = i0 + h, i2 = i1 + h, i3 = i2 + h;
      const int ia = q << (G::LOG - 1 - lh);  // stage h:  q * (L / (2h))
      const int ib = q << (G::LOG - 2 - lh);  // stage 2h: q * (L / (4h)), and (q + h) * (L / (4h))
      const int ic = ib + L / 4;
      double r0 = re[i0], m0_ = im[i0], r1 = re[i1], m1 = im[i1];
      double r2 = re[i2], m2 = im[i2], r3 = re[i3], m3 = im[i3];
      const double war = twr[ia], wai = twi[ia];
      sp_bfly(war, wai, r0, m0_, r1, m1);
      sp_bfly(war, wai, r2, m2, r3, m3);
      sp_bfly(twr[ib], twi[ib], r0, m0_, r2, m2);
      sp_bfly(twr[ic], twi[ic], r1, m1, r3, m3);
      re[i0] = r0;
      im[i0] = m0_;
      re[i1] = r1;
      im[i1] = m1;
      re[i2] = r2;
      im[i2] = m2;
      re[i3] = r3;
      im[i3] = m3;
    }
    __syncthreads();
  }
}

template <int L>
__global__ __launch_bounds__(SP_THREADS, SpGeom<L>::WAVES_PER_SIMD) void k_series_spectra(
    const double *__restrict__ v, const double *__restrict__ w, const double *__restrict__ tw,
    const int32_t *__restrict__ pair, int n, int nspec, int k0, int nseg, int step, int detrend,
    int npairs, double scale, int32_t *__restrict__ nused_out, double *__restrict__ psd,
    int32_t *__restrict__ nused_pair_out, double *__restrict__ csd) {
  using G = SpGeom<L>;
  constexpr int TM = G::TM, LP = G::LP, NF = G::NF, R = G::R;
  extern __shared__ double sp_lds[];
  double *re = sp_lds, *im = re + TM * LP;
  double *twr = im + TM * LP, *twi = twr + L / 2;
  double *mu = twi + L / 2;
  int *bad = (int *)(mu + TM);  // [parity of the segment][series of the job][TM]
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * TM;
  const int job = blockIdx.y;
  const bool is_pair = job >= nspec;  // the same for every thread of the block
  const int sa = is_pair ? pair[2 * (job - nspec)] : job;
  const int sb = is_pair ? pair[2 * (job - nspec) + 1] : job;
  const size_t rs = (size_t)nspec * (size_t)n;  // doubles between records

  for (int j = tid; j < L / 2; j += SP_THREADS) {
    twr[j] = tw[2 * j];
    twi[j] = tw[2 * j + 1];
  }
  if (tid < 4 * TM) bad[tid] = 0;
  __syncthreads();

  double acc0[R], acc1[R], zar[R], zai[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc0[r] = acc1[r] = zar[r] = zai[r] = 0.0;
  int count = 0;  // of the member tid (tid < TM)

  for (int i = 0; i < nseg; ++i) {
    const int kb = k0 + i * step;
    int *bad_a = bad + (i & 1) * 2 * TM, *bad_b = bad_a + TM;
    int *bad_next = bad + ((i + 1) & 1) * 2 * TM;
    // the other parity's flags: read last in segment i - 1, set next in segment i + 1; barriers
    // of this segment lie on either side
    if (tid < 2 * TM) bad_next[tid] = 0;
    // one instance of the transform serves the auto spectrum and both series of a pair
#pragma unroll 1
    for (int slot = 0; slot < (is_pair ? 2 : 1); ++slot) {
      sp_transform<L>(v, w, rs, n, slot ? sb : sa, m0, kb, detrend != 0, re, im, twr, twi, mu,
                      slot ? bad_b : bad_a);
      if (!is_pair) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int e = tid + r * SP_THREADS;
          if (e < TM * NF) {
            const int mi = e % TM, f = e / TM;
            const double zr = re[mi * LP + f], zi = im[mi * LP + f];
            const double p = zr * zr + zi * zi;
            if (!bad_a[mi]) acc0[r] = acc0[r] + p;
          }
        }
        if (tid < TM) count += bad_a[tid] ? 0 : 1;
      } else if (slot == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int e = tid + r * SP_THREADS;
          if (e < TM * NF) {
            const int mi = e % TM, f = e / TM;
            zar[r] = re[mi * LP + f];
            zai[r] = im[mi * LP + f];
          }
        }
        __syncthreads();  // the second series overwrites re / im
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int e = tid + r * SP_THREADS;
          if (e < TM * NF) {
            const int mi = e % TM, f = e / TM;
            const double zr = re[mi * LP + f], zi = im[mi * LP + f];
            const double cr = zar[r] * zr + zai[r] * zi;
            const double ci = zar[r] * zi - zai[r] * zr;
            if (!bad_a[mi] && !bad_b[mi]) {
              acc0[r] = acc0[r] + cr;
              acc1[r] = acc1[r] + ci;
            }
          }
        }
        if (tid < TM) count += (bad_a[tid] || bad_b[tid]) ? 0 : 1;
      }
    }
    __syncthreads();  // the next segment overwrites re / im
  }

  int *cnt = bad;  // (every read of the flags lies before the barrier above)
  if (tid < TM) cnt[tid] = count;
  __syncthreads();
  const double nan = __builtin_nan("");
  if (tid < TM && m0 + tid < n) {
    if (is_pair)
      nused_pair_out[(size_t)(job - nspec) * n + m0 + tid] = count;
    else
      nused_out[(size_t)job * n + m0 + tid] = count;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = tid + r * SP_THREADS;
    if (e < TM * NF) {
      const int mi = e % TM, f = e / TM;
      const int m = m0 + mi;
      if (m < n) {
        const int nu = cnt[mi];
        const double c = (f == 0 || f == L / 2) ? 1.0 : 2.0;
        if (!is_pair) {
          psd[((size_t)f * nspec + job) * n + m] =
              nu ? ((acc0[r] / (double)nu) * scale) * c : nan;
        } else {
          double *o = csd + ((size_t)f * (2 * npairs) + 2 * (job - nspec)) * n + m;
          o[0] = nu ? ((acc0[r] / (double)nu) * scale) * c : nan;
          o[n] = nu ? ((acc1[r] / (double)nu) * scale) * c : nan;
        }
      }
    }
  }
}

template <int L>
int sp_launch(const struct pm_series_spectra &d, int nseg, hipStream_t st, int32_t *nused, double *psd,
              int32_t *nused_pair, double *csd) {
  using G = SpGeom<L>;
  static_assert(G::LDS <= LDS_PER_CU, "the tile does not fit the CU's LDS");
  static_assert(G::TM * 8 >= 64 && 4 * G::TM <= SP_THREADS, "tile rows of at least 64 bytes");
  return launch_dyn(k_series_spectra<L>,
                    dim3((unsigned)((d.n + G::TM - 1) / G::TM), (unsigned)(d.nspec + d.npairs)),
                    SP_THREADS, G::LDS, st, d.v, d.window_dev, d.twiddle, d.pair_dev, (int)d.n,
                    (int)d.nspec, (int)d.k0, nseg, (int)d.step, (int)d.detrend, (int)d.npairs,
                    d.scale, nused, psd, nused_pair, csd);
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_spectra(const struct pm_series_spectra *dp, int32_t *nused, double *psd,
                      int32_t *nused_pair, double *csd, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_spectra &d = *dp;
  PM_SERIES_REQUIRE(d);
  const int L = d.nperseg;
  PM_REQUIRE(L >= PM_SPEC_NPERSEG_MIN && L <= PM_SPEC_NPERSEG_MAX && (L & (L - 1)) == 0,
             "nperseg %d is not a power of two in [%d, %d]", L, PM_SPEC_NPERSEG_MIN,
             PM_SPEC_NPERSEG_MAX);
  PM_REQUIRE(d.k1 - d.k0 >= L, "the window [%d, %d) is shorter than nperseg = %d", d.k0, d.k1, L);
  PM_REQUIRE(d.step >= 1 && d.step <= L, "step %d outside [1, nperseg = %d]", d.step, L);
  PM_REQUIRE(d.detrend == PM_SPEC_DETREND_NONE || d.detrend == PM_SPEC_DETREND_CONSTANT,
             "unknown detrend %d", d.detrend);
  PM_REQUIRE(d.npairs >= 0 && d.npairs <= PM_SPEC_PAIRS_MAX, "npairs %d outside [0, %d]", d.npairs,
             PM_SPEC_PAIRS_MAX);
  PM_REQUIRE((long long)(L / 2 + 1) * d.nspec < (1ll << 30),
             "nf * nspec = %lld is not below 2^30", (long long)(L / 2 + 1) * d.nspec);
  PM_REQUIRE(d.nspec + d.npairs <= 65535, "nspec + npairs = %d > 65535", d.nspec + d.npairs);
  PM_REQUIRE(d.v && d.window && d.window_dev && d.twiddle,
             "v, window (host or device) or twiddle is NULL");
  PM_REQUIRE(d.npairs == 0 || (d.pair && d.pair_dev), "pair is NULL (host or device)");
  PM_REQUIRE(nused && psd, "nused or psd is NULL");
  PM_REQUIRE(d.npairs == 0 || (nused_pair && csd), "nused_pair or csd is NULL with npairs %d",
             d.npairs);
  for (int p = 0; p < d.npairs; ++p)
    for (int c = 0; c < 2; ++c)
      PM_REQUIRE(d.pair[2 * p + c] >= 0 && d.pair[2 * p + c] < d.nspec,
                 "pair[%d][%d] = %d is not in [0, nspec = %d)", p, c, d.pair[2 * p + c], d.nspec);
  for (int j = 0; j < L; ++j)
    PM_REQUIRE(std::isfinite(d.window[j]), "window[%d] = %g is not finite", j, d.window[j]);
  PM_REQUIRE(std::isfinite(d.scale), "scale %g is not finite", d.scale);
  const int nseg = (d.k1 - d.k0 - L) / d.step + 1;
  hipStream_t st = resolve_stream(stream);
  switch (L) {
    case 8: return sp_launch<8>(d, nseg, st, nused, psd, nused_pair, csd);
    case 16: return sp_launch<16>(d, nseg, st, nused, psd, nused_pair, csd);
    case 32: return sp_launch<32>(d, nseg, st, nused, psd, nused_pair, csd);
    case 64: return sp_launch<64>(d, nseg, st, nused, psd, nused_pair, csd);
    case 128: return sp_launch<128>(d, nseg, st, nused, psd, nused_pair, csd);
    case 256: return sp_launch<256>(d, nseg, st, nused, psd, nused_pair, csd);
    case 512: return sp_launch<512>(d, nseg, st, nused, psd, nused_pair, csd);
    default: return sp_launch<1024>(d, nseg, st, nused, psd, nused_pair, csd);
  }
}

}  // extern "C"
