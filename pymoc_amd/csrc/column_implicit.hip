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
#include "column.hip.h"
#include "launch.hip.h"

namespace pm {

// lane i <- lane i - s / lane i + s; 0.0 where there is no such lane
__device__ __forceinline__ double imp_up(double x, int s, int lane) {
  const double y = __shfl_up(x, (unsigned)s, WAVE);
  return lane >= s ? y : 0.0;
}
__device__ __forceinline__ double imp_dn(double x, int s, int lane) {
  const double y = __shfl_down(x, (unsigned)s, WAVE);
  return lane + s < WAVE ? y : 0.0;
}

constexpr int IMP_PCR_LEVELS = 6;  // log2(WAVE)

template <int P>
struct ImpFactors {
  static constexpr int Q = P > 1 ? P - 1 : 1;  // rows of a lane's inner system T
  double l[Q];     // Thomas multipliers a_j / d'_{j-1} of T (l[0] = 0)
  double cq[Q];    // c_j of T's rows
  double invd[Q];  // 1 / d'_j
  double v[Q], w[Q];
  double aL, cL;   // the lane's last row: a on x_{P-2}, c on the next lane's x_0
  double al[IMP_PCR_LEVELS], ga[IMP_PCR_LEVELS], invD;  // PCR multipliers of the reduced system
};

// T u = r for the lane's rows 0 .. P-2 with the stored factors
template <int P>
__device__ __forceinline__ void imp_inner_solve(const ImpFactors<P> &f, const double *r, double *u) {
  constexpr int Q = P - 1;
  double y[Q];
  y[0] = r[0];
#pragma unroll
  for (int j = 1; j < Q; ++j) y[j] = fma(-f.l[j], y[j - 1], r[j]);
  u[Q - 1] = y[Q - 1] * f.invd[Q - 1];
#pragma unroll
  for (int j = Q - 2; j >= 0; --j) u[j] = fma(-f.cq[j], u[j + 1], y[j]) * f.invd[j];
}

// factor the lane's P rows (a on the level below, d, c on the level above)
template <int P>
__device__ __forceinline__ void imp_factor(ImpFactors<P> &f, const double (&a)[P],
                                           const double (&d)[P], const double (&c)[P], int lane) {
  double A, D, Cc;  // the lane's row of the reduced system
  if constexpr (P > 1) {
    constexpr int Q = P - 1;
    double dp = d[0];
    f.l[0] = 0.0;
    f.cq[0] = c[0];
    f.invd[0] = 1.0 / dp;
#pragma unroll
    for (int j = 1; j < Q; ++j) {
      f.l[j] = a[j] / dp;
      dp = fma(-f.l[j], c[j - 1], d[j]);
      f.cq[j] = c[j];
      f.invd[j] = 1.0 / dp;
    }
    double rv[Q], rw[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) rv[j] = rw[j] = 0.0;
    rv[0] = -a[0];
    rw[Q - 1] = -c[Q - 1];
    imp_inner_solve<P>(f, rv, f.v);
    imp_inner_solve<P>(f, rw, f.w);
    f.aL = a[P - 1];
    f.cL = c[P - 1];
    A = f.aL * f.v[Q - 1];
    D = fma(f.cL, imp_dn(f.v[0], 1, lane), fma(f.aL, f.w[Q - 1], d[P - 1]));
    Cc = f.cL * imp_dn(f.w[0], 1, lane);
  } else {
    f.l[0] = f.cq[0] = f.invd[0] = f.v[0] = f.w[0] = 0.0;
    f.aL = f.cL = 0.0;
    A = a[0];
    D = d[0];
    Cc = c[0];
  }
#pragma unroll
  for (int k = 0; k < IMP_PCR_LEVELS; ++k) {
    const int s = 1 << k;
    const double Du = imp_up(D, s, lane), Dd = imp_dn(D, s, lane);
    const double al = lane >= s ? -A / Du : 0.0;
    const double ga = lane + s < WAVE ? -Cc / Dd : 0.0;
    const double Au = imp_up(A, s, lane), Cu = imp_up(Cc, s, lane);
    const double Ad = imp_dn(A, s, lane), Cd = imp_dn(Cc, s, lane);
    D = fma(ga, Ad, fma(al, Cu, D));
    A = al * Au;
    Cc = ga * Cd;
    f.al[k] = al;
    f.ga[k] = ga;
  }
  f.invD = 1.0 / D;
}

// x = M^-1 r with the stored factors
template <int P>
__device__ __forceinline__ void imp_solve(const ImpFactors<P> &f, const double (&r)[P],
                                          double (&x)[P], int lane) {
  constexpr int Q = ImpFactors<P>::Q;
  double u[Q];
  double R;
  if constexpr (P > 1) {
    imp_inner_solve<P>(f, r, u);
    R = fma(-f.cL, imp_dn(u[0], 1, lane), fma(-f.aL, u[Q - 1], r[P - 1]));
  } else {
    R = r[0];
  }
#pragma unroll
  for (int k = 0; k < IMP_PCR_LEVELS; ++k) {
    const int s = 1 << k;
    const double Ru = imp_up(R, s, lane), Rd = imp_dn(R, s, lane);
    R = fma(f.ga[k], Rd, fma(f.al[k], Ru, R));
  }
  const double X = R * f.invD;
  x[P - 1] = X;
  if constexpr (P > 1) {
    const double Xp = imp_up(X, 1, lane);
#pragma unroll
    for (int j = 0; j < Q; ++j) x[j] = fma(f.w[j], X, fma(f.v[j], Xp, u[j]));
  }
}

template <int P>
__global__ __launch_bounds__(256) void k_column_implicit(pm_columns c,
                                                         const double *__restrict__ wA_g,
                                                         double dt, int nsteps, int ops) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int col = __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) / WAVE));
  if (col >= c.ncols) return;  // (whole waves; the kernel has no barrier)
  const int nz = c.nz;
  const size_t base = (size_t)col * nz;
  const int sel = c.ksel ? c.ksel[col] : 0;
  const int flags = c.flags ? c.flags[col] : 0;
  const bool do_conv = (flags & PM_COL_DO_CONV) != 0;
  const bool use_bzbot = (flags & PM_COL_BZBOT) != 0 && c.bzbot != nullptr;
  const double bs = c.bs[col];
  const double bbot = c.bbot[col];
  const double bzbot = use_bzbot ? c.bzbot[col] : 0.0;
  const double N2min = c.N2min[col];
  const double dz0 = c.z[1] - c.z[0];
  const size_t coef = (size_t)sel * c.ncols * nz + base;

  double b[P], z[P];
  load_levels<P>(b, c.b + base, lane, nz);
  load_levels<P>(z, c.z, lane, nz);

  ImpFactors<P> f;
  double q1 = 0.0;  // PM_COL_BZBOT: row 1's right-hand side is b_1 + q1
  if (ops & PM_OP_VERTADVDIFF) {
    double ra[P], rd[P], rc[P], rq[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      ra[p] = rc[p] = rq[p] = 0.0;
      rd[p] = 1.0;
      if (i >= 1 && i <= nz - 2) {
        const double z0 = c.z[i], dzm = z0 - c.z[i - 1], dzp = c.z[i + 1] - z0;
        const double dzc = 0.5 * (dzp + dzm);
        const double kap = c.kappa[coef + i];
        const double wa = wA_g ? wA_g[base + i] : 0.0;
        const double weff = (ops & PM_OP_WEFF) ? wa : wa - c.dAkappa[coef + i];
        const double w = weff / c.area[base + i];
        const double cl = (w < 0.0 ? 0.0 : w / dzm) + kap / (dzc * dzm);
        const double cu = (w < 0.0 ? -w / dzp : 0.0) + kap / (dzc * dzp);
        const bool fold = use_bzbot && i == 1;
        ra[p] = fold ? 0.0 : -(dt * cl);
        rc[p] = -(dt * cu);
        rd[p] = 1.0 + dt * ((fold ? 0.0 : cl) + cu);
        rq[p] = fold ? -(dt * cl) * (bzbot * dzm) : 0.0;
      }
    }
    imp_factor<P>(f, ra, rd, rc, lane);
    if (use_bzbot) q1 = level_value<P>(rq, 1);
  }

  for (int s = 0; s < nsteps; ++s) {
    if ((ops & PM_OP_CONVECT) && do_conv) {
      col_convect<WAVE, P>(b, z, bs, N2min, lane, lane, nz, c.z);
      col_pin<P>(b);
    }
    if (ops & PM_OP_VERTADVDIFF) {
      double r[P], x[P];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        double v = b[p];
        if (i == nz - 1 && !do_conv) v = bs;     // column.py:230-231
        if (i == 0) v = use_bzbot ? 0.0 : bbot;  // (BZBOT: row 1 does not read level 0)
        if (i == 1 && i <= nz - 2 && use_bzbot) v = v + q1;
        if (i >= nz) v = 0.0;
        r[p] = v;
      }
      imp_solve<P>(f, r, x, lane);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        if (!(i >= 1 && i <= nz - 2)) x[p] = r[p];  // boundary values as imposed
      }
      if (use_bzbot) {
        const double x1 = level_value<P>(x, 1);
        if (lane == 0) x[0] = x1 - bzbot * dz0;  // column.py:233 with the new b[1]
      }
#pragma unroll
      for (int p = 0; p < P; ++p) b[p] = x[p];
    }
  }

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

int column_steps_implicit(const pm_columns &c, const double *wA, double dt, int nsteps, int ops,
                          hipStream_t st) {
  constexpr int WPB = 4;  // columns (waves) per block
  const unsigned grid = (unsigned)((c.ncols + WPB - 1) / WPB);
  const int need = (c.nz + WAVE - 1) / WAVE;
#define PM_IMP_CASE(PP)                                                                     \
  if (need <= PP)                                                                           \
    return launch_dyn(k_column_implicit<PP>, grid, WPB * WAVE, 0, st, c, wA, dt, nsteps, ops);
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
