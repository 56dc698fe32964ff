// eof.hip -- the leading EOF of several indices of a recorded series and its principal component
// (Held & Kleinen 2004), computed where the series lives (pymoc_amd.SeriesEOF).
//
// (no counterpart: the download of the series and one np.linalg.eigh per member.)  Three entries
// over a series v[k][s][m] and a record window [k0, k1); include/pymoc_hip.h states the definition
// operation by operation: every product, sum and quotient rounded on its own (-ffp-contract=off),
// every sum sequential in ascending order from +0.0, the first on ties, no sqrt, log or exp.  Each
// double is reproduced bit for bit by the NumPy restatement (tests/eof_cases.py).
//
// K35 k_series_scatter<Q>, Q = 4 / 8 / 16 / 32 the compile-time bound of q.  A block is a tile of TM
// adjacent members x Q rows of S: lane = mi + TM * i, one thread per (member, row i).  It walks the
// K records in ascending order TWICE, in chunks of NR records staged in LDS, x[r][j][mi], members
// fastest: thread (mi, i) loads index sel[i] of its member (a row of TM adjacent members is
// contiguous; a member past the end reads the last one's), and a record's flag in LDS is cleared by
// whichever thread met a non-finite value.  Walk 1 sums the thread's own index over the used
// records: the mean.  Walk 2 stages a_ki = (x_ki - mean_i) * w_i instead of x and adds a_ki * a_kj
// into S_i0 .. S_ii, held in registers: the loop over j is unrolled over Q and predicated on
// j <= i, so no register array is indexed at run time.  Every sum is one thread's, in the
// definition's order; the lanes read adjacent members, and the rows a wave holds read one a_kj (a
// broadcast).  TM is 32 (16 at Q = 32), halved down to 8 while the launch has fewer than 512
// blocks: the sums do not depend on it.
//
// K36 k_series_eof<Q>: one unit per 32 lanes, two units per (one-wave) block; lane i owns row i of
// C in registers.  The pooled sum over a unit's members is sequential by definition and is the
// lane's own loop.  The iteration keeps y and v in LDS: every lane finds the pivot from y (the
// same loop, the same answer), forms its v_i, and after a barrier its y_i = sum_j C_ij v_j.  The
// count is fixed: a unit that failed a test goes on with whatever it holds and stores NaN.
//
// K37 k_series_project: a block is a tile of 32 adjacent members x a chunk of 64 records, 8 records
// in flight; mean, w and the unit's eof of the tile are staged in LDS once, the series is read
// straight from memory -- every value exactly once, 256-byte rows -- and one thread forms one
// record's sum over j.  (Nothing of the series is read twice, so there is nothing to stage.)
//
// The compiler's resource report (hipcc -O3 -ffp-contract=off, gfx950) is tabulated in DESIGN.md
// section 29: 0 bytes of scratch and no static LDS in all nine instantiations.
#include <cmath>
#include "common.hip.h"
#include "launch.hip.h"
#include "series.hip.h"

namespace pm {

struct EofSel {
  int32_t s[PM_EOF_Q_MAX];
};

constexpr int sc_ltm_max(int Q) { return Q == 32 ? 4 : 5; }
constexpr int SC_LTM_MIN = 3;
constexpr int SC_BLOCKS_WANTED = 512;

// The records a scatter block stages at a time: about 32 KiB of values, 4 .. 64 records.
inline int sc_records(int q, int tm) {
  const int nr = 4096 / (q * tm);
  return nr < 4 ? 4 : nr > 64 ? 64 : nr;
}
inline size_t sc_lds(int q, int tm, int nr) {
  return sizeof(double) * (size_t)nr * q * tm + sizeof(int) * ((size_t)nr * tm + PM_EOF_Q_MAX);
}

// sel into LDS by constant indices (a kernel argument indexed per lane would go to scratch).
__device__ __forceinline__ void eof_stage_sel(const EofSel &sel, int *sl, int tid) {
#pragma unroll
  for (int j = 0; j < PM_EOF_Q_MAX; ++j)
    if (tid == j) sl[j] = sel.s[j];
}

template <int Q>
__global__ __launch_bounds__(Q << sc_ltm_max(Q)) void k_series_scatter(
    const double *__restrict__ v, const double *__restrict__ w, int n, int nspec, int k0, int K,
    int q, int ltm, int nr, EofSel sel, int32_t *__restrict__ nused, double *__restrict__ mean,
    double *__restrict__ scat) {
  extern __shared__ double ef_lds_[];
  const int TM = 1 << ltm;
  const int tid = threadIdx.x;
  const int mi = tid & (TM - 1), i = tid >> ltm;          // member of the tile, row of S
  const int m0 = blockIdx.x << ltm;
  double *x = ef_lds_;                                    // [nr][q][TM]
  int *fl = (int *)(x + ((size_t)nr * q << ltm));         // [nr][TM]: the record is used
  int *sl = fl + ((size_t)nr << ltm);                     // [PM_EOF_Q_MAX]
  eof_stage_sel(sel, sl, tid);
  __syncthreads();
  const bool act = i < q;
  const size_t rs = (size_t)nspec * (size_t)n;            // doubles between records
  const double *base = series_row(v, rs, n, k0, act ? sl[i] : 0, m0, mi);
  const int mc = m0 + mi < n ? m0 + mi : n - 1;
  const double wi = (w && act) ? w[(size_t)i * n + mc] : 1.0;
  const double nan = __builtin_nan("");

  // One walk over the window: PASS 1 stages x and sums the thread's own index, PASS 2 stages a =
  // (x - mu) * wi and sums the row of S.
  double sum = 0.0, mu = 0.0;
  int cnt = 0;
  double acc[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) acc[j] = 0.0;
#pragma unroll 1
  for (int pass = 1; pass <= 2; ++pass) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += nr) {
      const int nrb = K - kc < nr ? K - kc : nr;
      if (i == 0)
        for (int r = 0; r < nrb; ++r) fl[(r << ltm) + mi] = 1;
      __syncthreads();
      if (act) {
        const double *row = base + (size_t)kc * rs;
#pragma unroll 4
        for (int r = 0; r < nrb; ++r) {
          const double xr = row[(size_t)r * rs];
          if (!series_finite(xr)) fl[(r << ltm) + mi] = 0;  // (every writer stores the same value)
          x[((r * q + i) << ltm) + mi] = pass == 1 ? xr : (xr - mu) * wi;
        }
      }
      __syncthreads();
      if (act) {
        if (pass == 1) {
          for (int r = 0; r < nrb; ++r)
            if (fl[(r << ltm) + mi]) {
              sum = sum + x[((r * q + i) << ltm) + mi];
              ++cnt;
            }
        } else {
          for (int r = 0; r < nrb; ++r)
            if (fl[(r << ltm) + mi]) {
              const double *a = x + ((size_t)(r * q) << ltm) + mi;
              const double ai = a[i << ltm];
#pragma unroll
              for (int j = 0; j < Q; ++j)
                if (j <= i) acc[j] = acc[j] + ai * a[j << ltm];
            }
        }
      }
      __syncthreads();
    }
    if (pass == 1) mu = sum / (double)cnt;
  }

  if (act && m0 + mi < n) {
    const size_t m = (size_t)(m0 + mi);
    const bool ok = cnt >= 2;
    if (i == 0) nused[m] = cnt;
    mean[(size_t)i * n + m] = ok ? mu : nan;
    const size_t e0 = (size_t)i * (i + 1) / 2;
#pragma unroll
    for (int j = 0; j < Q; ++j)
      if (j <= i) scat[(e0 + j) * n + m] = ok ? acc[j] : nan;
  }
}

constexpr int EF_LANES = 32;    // of a unit
constexpr int EF_THREADS = 64;  // two units to a block

template <int Q>
__global__ __launch_bounds__(EF_THREADS) void k_series_eof(
    const int32_t *__restrict__ nused, const double *__restrict__ scat,
    const int32_t *__restrict__ order, const int32_t *__restrict__ start, int n, int q, int nu,
    int iters, double *__restrict__ eof, double *__restrict__ lam_out,
    double *__restrict__ trace_out, double *__restrict__ resid_out, double *__restrict__ vv_out,
    int32_t *__restrict__ ntot) {
  extern __shared__ double ef_lds_[];
  const int i = threadIdx.x & (EF_LANES - 1), sub = threadIdx.x / EF_LANES;
  const int ur = blockIdx.x * (EF_THREADS / EF_LANES) + sub;
  const bool has = ur < nu;
  const int u = has ? ur : nu - 1;                        // (a spare half redoes the last unit)
  double *y = ef_lds_ + sub * 2 * EF_LANES, *vl = y + EF_LANES;
  const bool act = i < q;
  const int ic = act ? i : 0;
  const double nan = __builtin_nan("");

  // P: the unit's members in `order`, those with nused < 2 skipped; lane i sums row i
  double row[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) row[j] = 0.0;
  int N = 0;
  const int t0 = order ? start[u] : u, t1 = order ? start[u + 1] : u + 1;
  for (int t = t0; t < t1; ++t) {
    const int m = order ? order[t] : t;
    const int c = nused[m];
    if (c < 2) continue;
    N += c;
#pragma unroll
    for (int j = 0; j < Q; ++j)
      if (j < q) {
        const int e = j <= ic ? ic * (ic + 1) / 2 + j : j * (j + 1) / 2 + ic;
        row[j] = row[j] + scat[(size_t)e * n + m];
      }
  }
  const double Nf = (double)N;
  double cii = 0.0;
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    row[j] = j < q ? row[j] / Nf : 0.0;
    if (j == ic) cii = row[j];
  }
  if (act) y[i] = cii;
  __syncthreads();
  double trace = 0.0, best = y[0];
  int p = 0;
  for (int j = 0; j < q; ++j) {
    const double c = y[j];
    trace = trace + c;
    if (c > best) {
      best = c;
      p = j;
    }
  }
  bool good = N != 0 && series_finite(trace) && trace > 0.0;
  __syncthreads();
  double yi = 0.0, vi = 0.0;
#pragma unroll
  for (int j = 0; j < Q; ++j)
    if (j == p) yi = row[j];                              // column p0 of C (C is symmetric)
  if (act) y[i] = yi;
  __syncthreads();

  // iters normalise-and-multiply steps, and the one more of the definition
#pragma unroll 1
  for (int it = 0; it <= iters; ++it) {
    double yp = y[0], ab = fabs(yp);
    for (int j = 1; j < q; ++j) {
      const double c = y[j], a = fabs(c);
      if (a > ab) {
        ab = a;
        yp = c;
      }
    }
    if (yp == 0.0 || !series_finite(yp)) good = false;
    vi = yi / yp;
    if (act) vl[i] = vi;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < Q; ++j)
      if (j < q) s = s + row[j] * vl[j];
    yi = s;
    if (act) y[i] = yi;
    __syncthreads();
  }

  double vy = 0.0, vv = 0.0;
  for (int j = 0; j < q; ++j) {
    vy = vy + vl[j] * y[j];
    vv = vv + vl[j] * vl[j];
  }
  const double lam = vy / vv;
  double worst = fabs(y[0] - lam * vl[0]);
  for (int j = 1; j < q; ++j) {
    const double r = fabs(y[j] - lam * vl[j]);
    if (r > worst) worst = r;
  }
  const double resid = worst / fabs(lam);
  if (has && act) eof[(size_t)i * nu + u] = good ? vi : nan;
  if (has && i == 0) {
    lam_out[u] = good ? lam : nan;
    trace_out[u] = trace;
    resid_out[u] = good ? resid : nan;
    vv_out[u] = good ? vv : nan;
    ntot[u] = N;
  }
}

constexpr int PJ_LTM = 5, PJ_TM = 1 << PJ_LTM, PJ_THREADS = 256, PJ_NR = 64;

inline size_t pj_lds(int q) {
  return sizeof(double) * 3 * (size_t)q * PJ_TM + sizeof(int) * PM_EOF_Q_MAX;
}

__global__ __launch_bounds__(PJ_THREADS) void k_series_project(
    const double *__restrict__ v, const double *__restrict__ w,
    const int32_t *__restrict__ nused, const double *__restrict__ mean,
    const double *__restrict__ eof, const int32_t *__restrict__ unit, int n, int nspec, int k0,
    int K, int q, int nu, int nchunks, EofSel sel, double *__restrict__ pc) {
  extern __shared__ double ef_lds_[];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int m0 = tile << PJ_LTM;
  const int mi = tid & (PJ_TM - 1), slot = tid >> PJ_LTM, slots = PJ_THREADS >> PJ_LTM;
  double *mu = ef_lds_, *wl = mu + q * PJ_TM, *el = wl + q * PJ_TM;   // [q][TM] each
  int *sl = (int *)(el + q * PJ_TM);
  eof_stage_sel(sel, sl, tid);
  for (int idx = tid; idx < q * PJ_TM; idx += PJ_THREADS) {
    const int j = idx >> PJ_LTM, ml = idx & (PJ_TM - 1);
    const int mc = m0 + ml < n ? m0 + ml : n - 1;
    const int u = unit ? unit[mc] : mc;
    mu[idx] = mean[(size_t)j * n + mc];
    wl[idx] = w ? w[(size_t)j * n + mc] : 1.0;
    el[idx] = eof[(size_t)j * nu + u];
  }
  __syncthreads();
  const int mc = m0 + mi < n ? m0 + mi : n - 1;
  const bool live = m0 + mi < n;
  const bool fitted = nused[mc] >= 2;
  const size_t rs = (size_t)nspec * (size_t)n;
  const int j0 = chunk * PJ_NR;
  const int nrb = K - j0 < PJ_NR ? K - j0 : PJ_NR;
  const double nan = __builtin_nan("");
  for (int r = slot; r < nrb; r += slots) {
    const double *row = v + (size_t)(k0 + j0 + r) * rs + mc;
    double s = 0.0;
    bool fin = true;
#pragma unroll 4
    for (int j = 0; j < q; ++j) {
      const double xj = row[(size_t)sl[j] * n];
      fin = fin && series_finite(xj);
      s = s + ((xj - mu[(j << PJ_LTM) + mi]) * wl[(j << PJ_LTM) + mi]) * el[(j << PJ_LTM) + mi];
    }
    if (live) pc[(size_t)(j0 + r) * n + m0 + mi] = (fin && fitted) ? s : nan;
  }
}

// q's compile-time bound Q and the rest of the entry f(std::integral_constant<int, Q>).
template <class F>
int eof_by_q(int q, F &&f) {
  if (q <= 4) return f(std::integral_constant<int, 4>());
  if (q <= 8) return f(std::integral_constant<int, 8>());
  if (q <= 16) return f(std::integral_constant<int, 16>());
  return f(std::integral_constant<int, 32>());
}

// What entries 1 and 3 check of q, sel and the record window, after PM_SERIES_REQUIRE.
template <class D>
int eof_check_sel(const D &d) {
  PM_REQUIRE(d.q >= 1 && d.q <= PM_EOF_Q_MAX, "q %d outside [1, %d]", d.q, PM_EOF_Q_MAX);
  PM_REQUIRE(d.k1 - d.k0 >= 2, "the record window [%d, %d) holds fewer than 2 records", d.k0,
             d.k1);
  PM_REQUIRE(d.k1 - d.k0 < (1 << 30), "the record window holds %d records, not below 2^30",
             d.k1 - d.k0);
  for (int j = 0; j < d.q; ++j) {
    PM_REQUIRE(d.sel[j] >= 0 && d.sel[j] < d.nspec, "sel[%d] = %d outside [0, nspec = %d)", j,
               d.sel[j], d.nspec);
    for (int l = 0; l < j; ++l)
      PM_REQUIRE(d.sel[l] != d.sel[j], "sel[%d] = sel[%d] = %d", l, j, d.sel[j]);
  }
  return PM_OK;
}

template <class D>
EofSel eof_sel_of(const D &d) {
  EofSel s;
  for (int j = 0; j < PM_EOF_Q_MAX; ++j) s.s[j] = j < d.q ? d.sel[j] : 0;
  return s;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_series_scatter(const struct pm_series_scatter *dp, int32_t *nused, double *mean,
                      double *scat, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_scatter &d = *dp;
  PM_SERIES_REQUIRE(d);
  if (const int rc = eof_check_sel(d)) return rc;
  PM_REQUIRE(d.v, "v is NULL");
  PM_REQUIRE(nused && mean && scat, "nused, mean or scat is NULL");
  hipStream_t st = resolve_stream(stream);
  return eof_by_q(d.q, [&](auto qb) -> int {
    constexpr int Q = decltype(qb)::value;
    int ltm = sc_ltm_max(Q);
    while (ltm > SC_LTM_MIN && (((long long)d.n + (1 << ltm) - 1) >> ltm) < SC_BLOCKS_WANTED) --ltm;
    const int tm = 1 << ltm, nr = sc_records(d.q, tm);
    const long long ntiles = ((long long)d.n + tm - 1) / tm;   // n < 2^31: so is this
    return launch_dyn(k_series_scatter<Q>, dim3((unsigned)ntiles), Q * tm, sc_lds(d.q, tm, nr), st,
                      d.v, d.w, (int)d.n, (int)d.nspec, (int)d.k0, (int)(d.k1 - d.k0), (int)d.q,
                      ltm, nr, eof_sel_of(d), nused, mean, scat);
  });
}

int pm_series_eof(const struct pm_series_eof *dp, double *eof, double *lam, double *trace,
                  double *resid, double *vv, int32_t *ntot, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_eof &d = *dp;
  PM_REQUIRE(d.n >= 1 && d.nu >= 1 && d.nu <= d.n, "n %d < 1 or nu %d outside [1, n]", d.n, d.nu);
  PM_REQUIRE(d.q >= 1 && d.q <= PM_EOF_Q_MAX, "q %d outside [1, %d]", d.q, PM_EOF_Q_MAX);
  PM_REQUIRE(d.iters >= 1 && d.iters <= PM_EOF_ITERS_MAX, "iters %d outside [1, %d]", d.iters,
             PM_EOF_ITERS_MAX);
  PM_REQUIRE(d.nused && d.scat, "nused or scat is NULL");
  PM_REQUIRE(eof && lam && trace && resid && vv && ntot,
             "eof, lam, trace, resid, vv or ntot is NULL");
  const bool grouped = d.order || d.start || d.start_dev;
  if (grouped) {
    PM_REQUIRE(d.order && d.start && d.start_dev, "order, start and start_dev are not NULL together");
    PM_REQUIRE(d.start[0] == 0 && d.start[d.nu] == d.n, "start[0] = %d is not 0 or start[nu] = %d not n = %d",
               d.start[0], d.start[d.nu], d.n);
    for (int u = 0; u < d.nu; ++u) {
      PM_REQUIRE(d.start[u] <= d.start[u + 1], "start[%d] = %d is above start[%d] = %d", u,
                 d.start[u], u + 1, d.start[u + 1]);
      PM_REQUIRE(d.start[u + 1] - d.start[u] <= PM_STATS_GROUP_MAX, "unit %d has %d members, more than %d",
                 u, d.start[u + 1] - d.start[u], PM_STATS_GROUP_MAX);
    }
  } else {
    PM_REQUIRE(d.nu == d.n, "without order every member is a unit, but nu = %d is not n = %d", d.nu,
               d.n);
  }
  hipStream_t st = resolve_stream(stream);
  const unsigned per = EF_THREADS / EF_LANES;
  const unsigned grid = ((unsigned)d.nu + per - 1) / per;
  return eof_by_q(d.q, [&](auto qb) -> int {
    constexpr int Q = decltype(qb)::value;
    return launch_dyn(k_series_eof<Q>, dim3(grid), EF_THREADS, sizeof(double) * 2 * EF_THREADS, st,
                      d.nused, d.scat, d.order, d.start_dev, (int)d.n, (int)d.q, (int)d.nu,
                      (int)d.iters, eof, lam, trace, resid, vv, ntot);
  });
}

int pm_series_project(const struct pm_series_project *dp, double *pc, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_series_project &d = *dp;
  PM_SERIES_REQUIRE(d);
  if (const int rc = eof_check_sel(d)) return rc;
  PM_REQUIRE(d.nu >= 1 && d.nu <= d.n, "nu %d outside [1, n = %d]", d.nu, d.n);
  PM_REQUIRE(d.unit || d.nu == d.n, "without unit every member is a unit, but nu = %d is not n = %d",
             d.nu, d.n);
  PM_REQUIRE(d.v && d.nused && d.mean && d.eof, "v, nused, mean or eof is NULL");
  PM_REQUIRE(pc, "pc is NULL");
  const int K = d.k1 - d.k0;
  const int nchunks = (K + PJ_NR - 1) / PJ_NR;
  const long long ntiles = ((long long)d.n + PJ_TM - 1) / PJ_TM;
  PM_REQUIRE(ntiles * nchunks < (1ll << 31),
             "member tiles * record chunks = %lld is not below 2^31", ntiles * nchunks);
  hipStream_t st = resolve_stream(stream);
  return launch_dyn(k_series_project, dim3((unsigned)(ntiles * nchunks)), PJ_THREADS, pj_lds(d.q),
                    st, d.v, d.w, d.nused, d.mean, d.eof, d.unit, (int)d.n, (int)d.nspec,
                    (int)d.k0, K, (int)d.q, (int)d.nu, nchunks, eof_sel_of(d), pc);
}

}  // extern "C"
