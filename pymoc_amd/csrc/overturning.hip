// overturning.hip -- the three overturning streamfunction sections of the reference's figure
// script (examples/Plot_overturning.py:73-92) for a whole ensemble: psi_z (depth space), psi_b
// (isopycnal) and psi_res (residual) on the section channel + basin + north, plus per member the
// extrema of each field and where they are.
//
// One workgroup owns one member: it stages the member's profiles (b_basin, Psi, Psi_SO, psibz1,
// bs_SO) and bgrid / psib in LDS, then walks the [nrows][nz] section in blocks of 256 consecutive
// points (z fastest, so the f64 loads of the buoyancy section and the stores coalesce).  Channel
// and north rows cost one np.interp per point (binary search in LDS), basin rows two blends.
// Every lane keeps the extrema of its own points (first occurrence: its points come in rising
// order); they meet in a DPP wave reduction and then over the block's waves, the lowest index
// winning a tie -- one workgroup per member, so no result depends on the order blocks finish in.
//
// Arithmetic: IEEE fp64 in the script's order, `/` for its divisions, no contraction
// (-ffp-contract=off), np.interp as pm::interp_sorted -- bit-identical fields.
#include "overturning.hip.h"

namespace pm {

__host__ __device__ __forceinline__ size_t ovt_lds_bytes(const pm_overturning &a) {
  return (size_t)(4 * ovt_pad(a.nz) + ovt_pad(a.ny) + 2 * ovt_pad(a.nb)) * sizeof(double);
}

__global__ void __launch_bounds__(OVT_BLOCK) k_overturning(pm_overturning a) {
  extern __shared__ __attribute__((aligned(16))) double ovt_lds[];
  __shared__ OvtExt s_ext[OVT_WAVES][3][2];
  __shared__ int s_nan_at[3];
  __shared__ int s_status;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int nz = a.nz, ny = a.ny, nb = a.nb;
  double *lb = ovt_lds;               // b_basin
  double *lpsi = lb + ovt_pad(nz);    // AMOC.Psi
  double *lso = lpsi + ovt_pad(nz);   // PsiSO.Psi
  double *lpz = lso + ovt_pad(nz);    // AMOC.Psibz(nb)[0]
  double *lbs = lpz + ovt_pad(nz);    // bs_SO
  double *lbg = lbs + ovt_pad(ny);    // AMOC.bgrid
  double *lpb = lbg + ovt_pad(nb);    // AMOC.Psib(nb)
  {
    const double *gb = ovt_row(a.b_basin, m), *gpsi = ovt_row(a.Psi, m), *gso = ovt_row(a.Psi_SO, m),
                 *gpz = ovt_row(a.psibz1, m), *gbs = ovt_row(a.bs_SO, m), *gbg = ovt_row(a.bgrid, m),
                 *gpb = ovt_row(a.psib, m);
    for (int i = tid; i < nz; i += OVT_BLOCK) {
      lb[i] = gb[i];
      lpsi[i] = gpsi[i];
      lso[i] = gso[i];
      lpz[i] = gpz[i];
    }
    for (int i = tid; i < ny; i += OVT_BLOCK) lbs[i] = gbs[i];
    for (int i = tid; i < nb; i += OVT_BLOCK) {
      lbg[i] = gbg[i];
      lpb[i] = gpb[i];
    }
  }
  if (tid < 3) s_nan_at[tid] = OVT_NONE;
  if (tid == 0) s_status = 0;
  __syncthreads();
  int status = 0;
  for (int i = tid; i < nz; i += OVT_BLOCK) {
    const double b = lb[i];
    if (!(fabs(b) <= 1.7976931348623157e308) || (i > 0 && !(b >= lb[i - 1]))) status |= PM_OVT_BAD_BASIN;
  }

  const int nrows = ny + a.n_basin + a.n_north, north0 = ny + a.n_basin;
  const int npts = nrows * nz;
  const double *gsouth = ovt_row(a.bsouth, m), *gnorth = ovt_row(a.bnorth, m);
  const double lbasin = a.lbasin, lnorth = a.lnorth;
  const size_t base = (size_t)m * (size_t)npts;
  OvtExt mx[3], mn[3];
  int nan_at[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    mx[f] = mn[f] = OvtExt{0., OVT_NONE};
    nan_at[f] = OVT_NONE;
  }
  for (int p = tid; p < npts; p += OVT_BLOCK) {
    const int iy = p / nz, k = p - iy * nz;
    double bn, vz = 0., vb = 0., vr = 0.;
    if (iy < ny) {
      bn = gsouth[p];
      if (iy >= 1) {
        vr = vz = interp_sorted(bn, lb, lso, nz);
        vb = (lb[k] < lbs[iy]) ? lso[k] : 0.;
      }
    } else if (iy < north0) {
      bn = lb[k];
      const double c1 = a.c1[iy], c2 = a.c2[iy], so = c2 * lso[k];
      vr = vb = (c1 * lpz[k] + so) / lbasin;
      vz = (c1 * lpsi[k] + so) / lbasin;
    } else {
      const double *row = gnorth + (size_t)(iy - north0) * nz;
      bn = row[k];
      vr = interp_sorted(bn, lbg, lpb, nb);
      vz = (a.c3[iy] * lpsi[k]) / lnorth;
      vb = (lb[k] < row[nz - 1]) ? lpz[k] : 0.;
    }
    if (iy == nrows - 1) vr = 0.;
    if (bn != bn) status |= PM_OVT_NAN_SECTION;
    if (a.bnew) a.bnew[base + p] = bn;
    if (a.psi_z) a.psi_z[base + p] = vz;
    if (a.psi_b) a.psi_b[base + p] = vb;
    if (a.psi_res) a.psi_res[base + p] = vr;
    ovt_track(vz, p, mx[PM_OVT_Z], mn[PM_OVT_Z], nan_at[PM_OVT_Z]);
    ovt_track(vb, p, mx[PM_OVT_B], mn[PM_OVT_B], nan_at[PM_OVT_B]);
    ovt_track(vr, p, mx[PM_OVT_RES], mn[PM_OVT_RES], nan_at[PM_OVT_RES]);
  }
  if (status) atomicOr(&s_status, status);
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    if (nan_at[f] != OVT_NONE) atomicMin(&s_nan_at[f], nan_at[f]);
    const OvtExt wx = ovt_wave_reduce<true>(mx[f], lane), wn = ovt_wave_reduce<false>(mn[f], lane);
    if (lane == WAVE - 1) {
      s_ext[wave][f][0] = wx;
      s_ext[wave][f][1] = wn;
    }
  }
  __syncthreads();
  if (tid < 6) {
    const int f = tid >> 1, which = tid & 1;
    OvtExt e = s_ext[0][f][which];
    for (int w = 1; w < OVT_WAVES; ++w)
      e = which ? ovt_better<false>(s_ext[w][f][which], e) : ovt_better<true>(s_ext[w][f][which], e);
    if (s_nan_at[f] != OVT_NONE) e = OvtExt{__builtin_nan(""), s_nan_at[f]};
    if (a.extrema) a.extrema[(size_t)m * 6 + tid] = e.v;
    if (a.extrema_at) a.extrema_at[(size_t)m * 6 + tid] = e.at;
  }
  if (tid == 0 && a.status) a.status[m] = s_status;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_overturning_sections(const pm_overturning *d, pm_stream_t stream) {
  PM_REQUIRE(d, "pm_overturning is NULL");
  const pm_overturning &a = *d;
  PM_REQUIRE(a.n >= 0, "bad member count n=%d", a.n);
  PM_REQUIRE(a.nz >= 2 && a.nz <= PM_OVT_MAX_LEVELS && a.ny >= 2 && a.ny <= PM_OVT_MAX_LEVELS,
             "bad section grid nz=%d ny=%d (2..%d each: the profiles are staged in LDS)", a.nz, a.ny,
             PM_OVT_MAX_LEVELS);
  PM_REQUIRE(a.nb >= 1 && a.nb <= PM_OVT_MAX_NB, "bad nb=%d (1..%d isopycnal classes)", a.nb,
             PM_OVT_MAX_NB);
  PM_REQUIRE(a.n_basin >= 1 && a.n_north >= 1 && a.n_basin + a.n_north <= PM_OVT_MAX_LEVELS,
             "bad rows n_basin=%d n_north=%d (each >= 1, together <= %d)", a.n_basin, a.n_north,
             PM_OVT_MAX_LEVELS);
  const pm_rows *rows[] = {&a.b_basin, &a.bs_SO, &a.Psi, &a.Psi_SO, &a.bgrid,
                           &a.psib, &a.psibz1, &a.bsouth, &a.bnorth};
  for (const pm_rows *r : rows)
    PM_REQUIRE(r->offset >= 0 && r->stride >= 0, "negative offset or stride");
  if (a.n == 0) return PM_OK;
  for (const pm_rows *r : rows) PM_REQUIRE(r->ptr, "pm_overturning has a NULL input row pointer");
  PM_REQUIRE(a.c1 && a.c2 && a.c3, "pm_overturning has a NULL row coefficient pointer");
  return launch_dyn(k_overturning, (unsigned)a.n, OVT_BLOCK, ovt_lds_bytes(a),
                    resolve_stream(stream), a);
}

}  // extern "C"
