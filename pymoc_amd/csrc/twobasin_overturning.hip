// twobasin_overturning.hip -- what the reference's two-basin script builds after its loop
// (examples/twobasin_NadeauJansen.py:157-262) for a whole ensemble: eight overturning fields
// (depth space, isopycnal and residual; global, Atlantic and Pacific) and three buoyancy sections
// on channel + basin + northern transition + northern sinking region, plus per member the
// extrema of each field and where they are.
//
// k_twobasin_profiles: the two derived rows the section interpolators need first (:161, :192-193).
//
// k_twobasin_overturning: one workgroup owns one member, as in overturning.hip.  It stages the
// member's ten raw nz-rows, bs_SO and -- first -- ZOC's bgrid / psib in LDS; forms b_basin, the
// summed SO overturning, the two interpolated SO sectors and their sum (:166-167) and ZOC's
// overturning on b_basin; then AMOC's bgrid / psib take the place of ZOC's (which nothing reads
// any more) and give AMOC_bbasin (:168).  The walk over the [nrows][nz] section is in blocks of
// 256 consecutive points, z fastest: loads of the buoyancy sections and the up to eleven stores
// coalesce.  Channel rows cost two np.interp per point, transition rows one, basin and north rows
// blends of LDS rows.  Extrema: overturning.hip.h.
//
// Arithmetic: IEEE fp64 in the script's order, `/` for its divisions, no contraction
// (-ffp-contract=off), np.interp as pm::interp_sorted -- bit-identical fields.
#include "overturning.hip.h"

namespace pm {

constexpr int TBO_F = PM_TBO_FIELDS;
constexpr int TBO_NZ_ROWS = 17;  // ten staged + seven derived rows of nz doubles

// static LDS of k_twobasin_overturning next to the carve
struct alignas(16) TboScratch {
  OvtExt ext[OVT_WAVES][TBO_F][2];
  int nan_at[TBO_F];
  int status;
};

// the carve: what the kernel lays out and what the host checks against the CU's LDS
__host__ __device__ __forceinline__ size_t tbo_carve_doubles(int nz, int ny, int nb) {
  return (size_t)TBO_NZ_ROWS * ovt_pad(nz) + ovt_pad(ny) + 2 * (size_t)ovt_pad(nb);
}
__host__ __device__ __forceinline__ size_t tbo_lds_bytes(int nz, int ny, int nb) {
  return tbo_carve_doubles(nz, ny, nb) * sizeof(double) + sizeof(TboScratch);
}

// :161 b_basin=(A_Atl*Atl.b+A_Pac*Pac.b)/(A_Atl+A_Pac)
__device__ __forceinline__ double tbo_b_basin(double A_Atl, double b_Atl, double A_Pac, double b_Pac) {
  return (A_Atl * b_Atl + A_Pac * b_Pac) / (A_Atl + A_Pac);
}

__device__ __forceinline__ bool tbo_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

__global__ void __launch_bounds__(256) k_twobasin_profiles(pm_twobasin_rows a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)a.n * a.nz) return;
  const int m = (int)(e / a.nz), i = (int)(e - (int64_t)m * a.nz);
  const double A_Atl = ovt_row(a.A_Atl, m)[0], A_Pac = ovt_row(a.A_Pac, m)[0];
  const double bb = tbo_b_basin(A_Atl, ovt_row(a.b_Atl, m)[i], A_Pac, ovt_row(a.b_Pac, m)[i]);
  if (a.b_basin) a.b_basin[e] = bb;
  if (a.bn) a.bn[e] = (i == 0) ? bb : ovt_row(a.b_north, m)[i];
}

__global__ void __launch_bounds__(OVT_BLOCK) k_twobasin_overturning(pm_twobasin_overturning a) {
  extern __shared__ __attribute__((aligned(16))) double tbo_lds[];
  __shared__ TboScratch s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nz = a.nz, ny = a.ny, nb = a.nb, pz = ovt_pad(nz);
  // (the rows np.interp searches do not come first: on a NaN xp[0] interp_sorted reads index -1)
  double *lam = tbo_lds;      // AMOC.Psi
  double *lzo = lam + pz;     // ZOC.Psi
  double *lapz1 = lzo + pz;   // AMOC.Psibz(nb)[0]
  double *lapz2 = lapz1 + pz; // AMOC.Psibz(nb)[1]
  double *lzpz1 = lapz2 + pz; // ZOC.Psibz()[0]
  double *lzpz2 = lzpz1 + pz; // ZOC.Psibz()[1]
  double *lbA = lzpz2 + pz;   // Atl.b
  double *lbP = lbA + pz;     // Pac.b
  double *lsoA = lbP + pz;    // SO_Atl.Psi
  double *lsoP = lsoA + pz;   // SO_Pac.Psi
  double *lbb = lsoP + pz;    // b_basin
  double *lsum = lbb + pz;    // SO_Atl.Psi + SO_Pac.Psi
  double *liA = lsum + pz;    // np.interp(b_basin, Atl.b, SO_Atl.Psi)
  double *liP = liA + pz;     // np.interp(b_basin, Pac.b, SO_Pac.Psi)
  double *lso = liP + pz;     // PsiSO = iA + iP
  double *lAb = lso + pz;     // AMOC_bbasin
  double *lZb = lAb + pz;     // np.interp(b_basin, ZOC.bgrid, ZOC.Psib())
  double *lbs = lZb + pz;     // bs_SO
  double *lbg = lbs + ovt_pad(ny);  // ZOC.bgrid, then AMOC.bgrid
  double *lpb = lbg + ovt_pad(nb);  // ZOC.Psib(), then AMOC.Psib(nb)
  {
    const double *g0 = ovt_row(a.b_Atl, m), *g1 = ovt_row(a.b_Pac, m), *g2 = ovt_row(a.Psi_SO_Atl, m),
                 *g3 = ovt_row(a.Psi_SO_Pac, m), *g4 = ovt_row(a.Psi_AMOC, m),
                 *g5 = ovt_row(a.Psi_ZOC, m), *g6 = ovt_row(a.psibz_AMOC1, m),
                 *g7 = ovt_row(a.psibz_AMOC2, m), *g8 = ovt_row(a.psibz_ZOC1, m),
                 *g9 = ovt_row(a.psibz_ZOC2, m), *gbs = ovt_row(a.bs_SO, m),
                 *gbg = ovt_row(a.bgrid_ZOC, m), *gpb = ovt_row(a.psib_ZOC, m);
    for (int i = tid; i < nz; i += OVT_BLOCK) {
      lbA[i] = g0[i];
      lbP[i] = g1[i];
      lsoA[i] = g2[i];
      lsoP[i] = g3[i];
      lam[i] = g4[i];
      lzo[i] = g5[i];
      lapz1[i] = g6[i];
      lapz2[i] = g7[i];
      lzpz1[i] = g8[i];
      lzpz2[i] = g9[i];
    }
    for (int i = tid; i < ny; i += OVT_BLOCK) lbs[i] = gbs[i];
    for (int i = tid; i < nb; i += OVT_BLOCK) {
      lbg[i] = gbg[i];
      lpb[i] = gpb[i];
    }
  }
  if (tid < TBO_F) s.nan_at[tid] = OVT_NONE;
  if (tid == 0) s.status = 0;
  __syncthreads();
  int status = 0;
  {
    const double A_Atl = ovt_row(a.A_Atl, m)[0], A_Pac = ovt_row(a.A_Pac, m)[0];
    for (int i = tid; i < nz; i += OVT_BLOCK) {
      const double bb = tbo_b_basin(A_Atl, lbA[i], A_Pac, lbP[i]);
      const double iA = interp_sorted(bb, lbA, lsoA, nz), iP = interp_sorted(bb, lbP, lsoP, nz);
      lbb[i] = bb;
      lsum[i] = lsoA[i] + lsoP[i];
      liA[i] = iA;
      liP[i] = iP;
      lso[i] = iA + iP;
      lZb[i] = interp_sorted(bb, lbg, lpb, nb);
      if (!tbo_finite(lbA[i]) || (i > 0 && !(lbA[i] >= lbA[i - 1]))) status |= PM_TBO_BAD_ATL;
      if (!tbo_finite(lbP[i]) || (i > 0 && !(lbP[i] >= lbP[i - 1]))) status |= PM_TBO_BAD_PAC;
    }
    for (int i = tid + 1; i < nb; i += OVT_BLOCK)
      if (!(lbg[i] >= lbg[i - 1])) status |= PM_TBO_BAD_BGRID_ZOC;
  }
  __syncthreads();  // ZOC's bgrid / psib are done with: AMOC's take their place
  {
    const double *gbg = ovt_row(a.bgrid_AMOC, m), *gpb = ovt_row(a.psib_AMOC, m);
    for (int i = tid; i < nb; i += OVT_BLOCK) {
      lbg[i] = gbg[i];
      lpb[i] = gpb[i];
    }
  }
  __syncthreads();
  for (int i = tid; i < nz; i += OVT_BLOCK) {
    const double bb = lbb[i];
    lAb[i] = interp_sorted(bb, lbg, lpb, nb);
    if (!tbo_finite(bb) || (i > 0 && !(bb >= lbb[i - 1]))) status |= PM_TBO_BAD_BASIN;
  }
  for (int i = tid + 1; i < nb; i += OVT_BLOCK)
    if (!(lbg[i] >= lbg[i - 1])) status |= PM_TBO_BAD_BGRID_AMOC;
  __syncthreads();

  const int trans0 = ny + a.n_basin, north0 = trans0 + a.n_trans, nrows = north0 + a.n_north;
  const int npts = nrows * nz, pac_end = trans0 * nz;
  const double *gsouth = ovt_row(a.bsouth, m), *gtrans = ovt_row(a.btrans, m), *gbn = ovt_row(a.bn, m);
  const double lbasin = a.lbasin, lnorth = a.lnorth, qnan = __builtin_nan("");
  const size_t base = (size_t)m * (size_t)npts;
  OvtExt mx[TBO_F], mn[TBO_F];
  int nan_at[TBO_F];
#pragma unroll
  for (int f = 0; f < TBO_F; ++f) {
    mx[f] = mn[f] = OvtExt{0., OVT_NONE};
    nan_at[f] = OVT_NONE;
  }
  for (int p = tid; p < npts; p += OVT_BLOCK) {
    const int iy = p / nz, k = p - iy * nz;
    double v[TBO_F];
#pragma unroll
    for (int f = 0; f < TBO_F; ++f) v[f] = 0.;
    double x, xA, xP;  // bnew, bnew_Atl, bnew_Pac
    if (iy < ny) {
      x = xA = xP = gsouth[p];
      if (iy >= 1) {
        v[PM_TBO_Z] = v[PM_TBO_Z_ATL] = v[PM_TBO_Z_PAC] = interp_sorted(x, lbb, lsum, nz);
        v[PM_TBO_B] = v[PM_TBO_B_ATL] = v[PM_TBO_B_PAC] = (lbb[k] < lbs[iy]) ? lso[k] : 0.;
        v[PM_TBO_ATL] = v[PM_TBO_PAC] = interp_sorted(x, lbb, lso, nz);
      }
    } else if (iy < trans0) {
      x = lbb[k];
      xA = lbA[k];
      xP = lbP[k];
      const double c1 = a.c1[iy], c2 = a.c2[iy];
      const double zA = c1 * lam[k], bA = c1 * lAb[k];
      v[PM_TBO_Z] = (zA + c2 * lsum[k]) / lbasin;
      v[PM_TBO_Z_ATL] = (zA + c2 * (lsoA[k] - lzo[k])) / lbasin;
      v[PM_TBO_Z_PAC] = (c2 * (lsoP[k] + lzo[k])) / lbasin;
      v[PM_TBO_B] = (bA + c2 * lso[k]) / lbasin;
      v[PM_TBO_ATL] = (c1 * lapz1[k] + c2 * (lsoA[k] - lzpz1[k])) / lbasin;
      v[PM_TBO_B_ATL] = (bA + c2 * (liA[k] - lZb[k])) / lbasin;
      v[PM_TBO_PAC] = (c2 * (lsoP[k] + lzpz2[k])) / lbasin;
      v[PM_TBO_B_PAC] = (c2 * (liP[k] + lZb[k])) / lbasin;
    } else {
      double top;
      if (iy < north0) {
        const double *row = gtrans + (size_t)(iy - trans0) * nz;
        x = row[k];
        top = row[nz - 1];
        v[PM_TBO_Z] = lam[k];
        v[PM_TBO_B] = lAb[k];
        v[PM_TBO_ATL] = interp_sorted(x, lbg, lpb, nb);
      } else {
        const double c3 = a.c3[iy];
        x = gbn[k];
        top = gbn[nz - 1];
        v[PM_TBO_Z] = (c3 * lam[k]) / lnorth;
        v[PM_TBO_B] = (c3 * lAb[k]) / lnorth;
        v[PM_TBO_ATL] = (c3 * lapz2[k]) / lnorth;
      }
      if (!(lbb[k] < top)) v[PM_TBO_B] = 0.;
      v[PM_TBO_Z_ATL] = v[PM_TBO_Z];
      v[PM_TBO_B_ATL] = v[PM_TBO_B];
      v[PM_TBO_Z_PAC] = v[PM_TBO_B_PAC] = v[PM_TBO_PAC] = qnan;
      xA = x;
      xP = qnan;
    }
    // a NaN of a staged section (the basin rows are b_basin: PM_TBO_BAD_BASIN says that)
    if ((iy < ny || iy >= trans0) && x != x) status |= PM_TBO_NAN_SECTION;
    if (a.bnew) a.bnew[base + p] = x;
    if (a.bnew_Atl) a.bnew_Atl[base + p] = xA;
    if (a.bnew_Pac) a.bnew_Pac[base + p] = xP;
#pragma unroll
    for (int f = 0; f < TBO_F; ++f) {
      if (a.psi[f]) a.psi[f][base + p] = v[f];
      const bool pacific = f == PM_TBO_Z_PAC || f == PM_TBO_B_PAC || f == PM_TBO_PAC;
      if (!pacific || p < pac_end) ovt_track(v[f], p, mx[f], mn[f], nan_at[f]);
    }
  }
  if (status) atomicOr(&s.status, status);
#pragma unroll
  for (int f = 0; f < TBO_F; ++f) {
    if (nan_at[f] != OVT_NONE) atomicMin(&s.nan_at[f], nan_at[f]);
    const OvtExt wx = ovt_wave_reduce<true>(mx[f], lane), wn = ovt_wave_reduce<false>(mn[f], lane);
    if (lane == WAVE - 1) {
      s.ext[wave][f][0] = wx;
      s.ext[wave][f][1] = wn;
    }
  }
  __syncthreads();
  if (tid < 2 * TBO_F) {
    const int f = tid >> 1, which = tid & 1;
    OvtExt e = s.ext[0][f][which];
    for (int w = 1; w < OVT_WAVES; ++w)
      e = which ? ovt_better<false>(s.ext[w][f][which], e) : ovt_better<true>(s.ext[w][f][which], e);
    if (s.nan_at[f] != OVT_NONE) e = OvtExt{qnan, s.nan_at[f]};
    if (a.extrema) a.extrema[(size_t)m * (2 * TBO_F) + tid] = e.v;
    if (a.extrema_at) a.extrema_at[(size_t)m * (2 * TBO_F) + tid] = e.at;
  }
  if (tid == 0 && a.status) a.status[m] = s.status;
}

static int tbo_rows_ok(const pm_rows *const *rows, int count, bool need_ptr) {
  for (int i = 0; i < count; ++i) {
    PM_REQUIRE(rows[i]->offset >= 0 && rows[i]->stride >= 0, "negative offset or stride");
    if (need_ptr) PM_REQUIRE(rows[i]->ptr, "NULL input row pointer");
  }
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_twobasin_profiles(const pm_twobasin_rows *d, pm_stream_t stream) {
  PM_REQUIRE(d, "pm_twobasin_rows is NULL");
  const pm_twobasin_rows &a = *d;
  PM_REQUIRE(a.n >= 0, "bad member count n=%d", a.n);
  PM_REQUIRE(a.nz >= 2 && a.nz <= PM_TBO_MAX_LEVELS, "bad nz=%d (2..%d)", a.nz, PM_TBO_MAX_LEVELS);
  const pm_rows *rows[] = {&a.b_Atl, &a.b_Pac, &a.b_north, &a.A_Atl, &a.A_Pac};
  if (int rc = tbo_rows_ok(rows, 5, a.n > 0)) return rc;
  if (a.n == 0) return PM_OK;
  const int64_t total = (int64_t)a.n * a.nz;
  hipLaunchKernelGGL(k_twobasin_profiles, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     resolve_stream(stream), a);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

int pm_twobasin_overturning_lds_bytes(int32_t nz, int32_t ny, int32_t nb, size_t *bytes) {
  PM_REQUIRE(bytes, "bytes is NULL");
  PM_REQUIRE(nz >= 0 && ny >= 0 && nb >= 0, "negative size");
  *bytes = tbo_lds_bytes(nz, ny, nb);
  return PM_OK;
}

int pm_twobasin_overturning_sections(const pm_twobasin_overturning *d, pm_stream_t stream) {
  PM_REQUIRE(d, "pm_twobasin_overturning is NULL");
  const pm_twobasin_overturning &a = *d;
  PM_REQUIRE(a.n >= 0, "bad member count n=%d", a.n);
  PM_REQUIRE(a.nz >= 2 && a.nz <= PM_TBO_MAX_LEVELS && a.ny >= 2 && a.ny <= PM_TBO_MAX_LEVELS,
             "bad section grid nz=%d ny=%d (2..%d each)", a.nz, a.ny, PM_TBO_MAX_LEVELS);
  PM_REQUIRE(a.nb >= 1 && a.nb <= PM_TBO_MAX_NB, "bad nb=%d (1..%d isopycnal classes)", a.nb,
             PM_TBO_MAX_NB);
  PM_REQUIRE(a.n_basin >= 1 && a.n_trans >= 1 && a.n_north >= 1 &&
                 (int64_t)a.n_basin + a.n_trans + a.n_north <= PM_TBO_MAX_LEVELS,
             "bad rows n_basin=%d n_trans=%d n_north=%d (each >= 1, together <= %d)", a.n_basin,
             a.n_trans, a.n_north, PM_TBO_MAX_LEVELS);
  const size_t lds = tbo_lds_bytes(a.nz, a.ny, a.nb);
  PM_REQUIRE(lds <= LDS_PER_CU,
             "nz=%d ny=%d nb=%d need %zu bytes of LDS per member, a workgroup has %zu", a.nz, a.ny,
             a.nb, lds, LDS_PER_CU);
  const pm_rows *rows[] = {&a.b_Atl,       &a.b_Pac,       &a.A_Atl,      &a.A_Pac,      &a.bs_SO,
                           &a.Psi_SO_Atl,  &a.Psi_SO_Pac,  &a.Psi_AMOC,   &a.Psi_ZOC,    &a.psibz_AMOC1,
                           &a.psibz_AMOC2, &a.psibz_ZOC1,  &a.psibz_ZOC2, &a.bgrid_AMOC, &a.psib_AMOC,
                           &a.bgrid_ZOC,   &a.psib_ZOC,    &a.bsouth,     &a.btrans,     &a.bn};
  if (int rc = tbo_rows_ok(rows, 20, a.n > 0)) return rc;
  if (a.n == 0) return PM_OK;
  PM_REQUIRE(a.c1 && a.c2 && a.c3, "pm_twobasin_overturning has a NULL row coefficient pointer");
  return launch_dyn(k_twobasin_overturning, (unsigned)a.n, OVT_BLOCK,
                    tbo_carve_doubles(a.nz, a.ny, a.nb) * sizeof(double), resolve_stream(stream), a);
}

}  // extern "C"
