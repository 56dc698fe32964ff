// column_implicit.hip -- backward Euler of the column's vertical advection-diffusion, fused over
// nsteps (pm_column_steps_implicit).  An EXTENSION: the reference's Column.vertadvdiff
// (src/pymoc/modules/column.py:210-249) is forward Euler and has no implicit counterpart, so
// this is a tolerance path -- bit-identical to nothing but itself.
//
// The scheme.  With the reference's own discretisation (column.py:226-249),
//   dz = z[1:] - z[:-1],  dzc_i = 0.5 (dz[i] + dz[i-1]),  w_i = weff_i / Area_i,
//   cl_i = (w_i < 0 ? 0 : w_i / dz[i-1]) + kappa_i / (dzc_i dz[i-1])     (on b[i-1])
//   cu_i = (w_i < 0 ? -w_i / dz[i] : 0)  + kappa_i / (dzc_i dz[i])       (on b[i+1])
// one step solves, for the interior levels i = 1 .. nz-2,
//   (1 + dt (cl_i + cu_i)) x_i - dt cl_i x_{i-1} - dt cu_i x_{i+1} = b_i
// with x_0, x_{nz-1} the boundary values (under PM_COL_BZBOT x_0 = x_1 - bzbot dz[0] is folded
// into row 1).  weff does not depend on b, so the upwind direction is known before the step and
// the system is linear; its matrix is a strictly diagonally dominant M-matrix (off-diagonals <= 0,
// rows sum to 1), so elimination in any order needs no pivoting.  The matrix depends on static
// data, wA and dt only: it is factored ONCE per launch, a step is the right-hand side's passage
// through the stored multipliers.
//
// Layout: one wavefront per column, lane l holds the P = ceil(nz / 64) contiguous levels
// [l P, l P + P) in registers (the explicit kernel's layout: col_convect is shared).  The
// boundary levels and the padding levels >= nz are identity rows of a 64 P-row system.
//   1. partition: each lane solves its rows 0 .. P-2 against the two values that bound them, the
//      last level of the lane before (X') and its own last level (X):
//         x_j = u_j + v_j X' + w_j X,    T u = r,  T v = -a_0 e_0,  T w = -c_{P-2} e_{P-2}
//      (v, w: static; u: a Thomas sweep of P-1 rows per step with the stored factors of T);
//   2. the lanes' last rows then form a 64-row tridiagonal system in X (the Schur complement,
//      diagonally dominant like its parent), solved by parallel cyclic reduction across the lanes:
//      six levels of two lane shifts and two fma each, multipliers stored at factor time;
//   3. back-substitution: x_j from u_j, X', X.
// P = 1 (nz <= 64) is plain PCR.  No LDS, no barrier; registers only (the build reports the
// scratch size of every instantiation: 0 bytes for nz <= 256).
// pm_column_steps_implicit_twobasin launches the same instantiations with PM_OP_WA_TWOBASIN set: the
// rows' forcing is then formed from the two-basin driver's three overturning arrays as the matrix
// is built (imp_twobasin_wa), in pm_twobasin_forcing's operation order -- bit-identical to that
// launch into an array followed by pm_column_steps_implicit on the array.
// The device functions (row construction, factors, solve, the step) live in column_implicit.hip.h,
// which the fused Jansen & Nadeau loop (jn2018_implicit.hip) includes too.
#include "column_implicit.hip.h"
#include "launch.hip.h"

namespace pm {

template <int P>
__global__ __launch_bounds__(256) void k_column_implicit(pm_columns c,
                                                         const double *__restrict__ wA_g,
                                                         const double *__restrict__ zon_g,
                                                         const double *__restrict__ so_g,
                                                         double dt, int nsteps, int ops) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int col = __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) / WAVE));
  if (col >= c.ncols) return;  // (whole waves; the kernel has no barrier)
  const int nz = c.nz;
  const size_t base = (size_t)col * nz;
  const int sel = c.ksel ? c.ksel[col] : 0;
  const int flags = c.flags ? c.flags[col] : 0;
  ImpCol k;
  k.do_conv = (flags & PM_COL_DO_CONV) != 0;
  k.use_bzbot = (flags & PM_COL_BZBOT) != 0 && c.bzbot != nullptr;
  k.bs = c.bs[col];
  k.bzbot = k.use_bzbot ? c.bzbot[col] : 0.0;
  k.N2min = c.N2min[col];
  k.dz0 = c.z[1] - c.z[0];
  const double bbot = c.bbot[col];

  double b[P], z[P];
  load_levels<P>(b, c.b + base, lane, nz);
  load_levels<P>(z, c.z, lane, nz);

  ImpFactors<P> f;
  double q1 = 0.0;  // PM_COL_BZBOT: row 1's right-hand side is b_1 + q1
  if (ops & PM_OP_VERTADVDIFF)
    imp_build<P>(f, q1, c, wA_g, col, sel, dt, ops, k.use_bzbot, k.bzbot, lane, zon_g, so_g);

  for (int s = 0; s < nsteps; ++s) imp_step<P>(f, b, z, k, bbot, q1, ops, lane, nz, c.z);

  bool bad = false;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    if (i < nz) {
      c.b[base + i] = b[p];
      bad |= !isfinite(b[p]);
    }
  }
  if (c.nonfinite) {
    const unsigned long long m = __ballot(bad);
    if (lane == 0) c.nonfinite[col] = (m != 0ull) ? 1 : 0;
  }
}

// wA alone: the forcing as an array; with zon / so (ops carries PM_OP_WA_TWOBASIN): the three
// overturning arrays of a two-basin batch
int column_steps_implicit(const pm_columns &c, const double *wA, const double *zon,
                          const double *so, double dt, int nsteps, int ops, hipStream_t st) {
  constexpr int WPB = 4;  // columns (waves) per block
  const unsigned grid = (unsigned)((c.ncols + WPB - 1) / WPB);
  const int need = (c.nz + WAVE - 1) / WAVE;
#define PM_IMP_CASE(PP)                                                                     \
  if (need <= PP)                                                                           \
    return launch_dyn(k_column_implicit<PP>, grid, WPB * WAVE, 0, st, c, wA, zon, so, dt,    \
                      nsteps, ops);
  PM_IMP_CASE(1)
  PM_IMP_CASE(2)
  PM_IMP_CASE(3)
  PM_IMP_CASE(4)
  PM_IMP_CASE(6)
  PM_IMP_CASE(8)
  PM_IMP_CASE(12)
  PM_IMP_CASE(16)
#undef PM_IMP_CASE
  return fail(PM_EINVAL, "pm_column_steps_implicit: nz=%d does not fit one wave", c.nz);
}

}  // namespace pm
