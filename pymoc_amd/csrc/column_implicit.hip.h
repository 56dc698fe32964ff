// column_implicit.hip.h -- device functions of the backward-Euler column step, shared by
// k_column_implicit (column_implicit.hip) and the fused Jansen & Nadeau loop k_jn2018_implicit
// (jn2018_implicit.hip): both kernels run the SAME instructions on a column, so a fused launch is
// bit-identical to the launches it replaces.  The scheme and the layout are described in
// column_implicit.hip.
#pragma once
#include "column.hip.h"

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

// Level i's forcing of column `col` of a two-basin batch (rows [0, n) Atlantic, [n, 2n) north,
// [2n, 3n) Pacific, n = ncols / 3) from the overturnings, pm_twobasin_forcing's operations in its
// order (twobasin_NadeauJansen.py:103-105): iso / zon / so are [2n][nz].  Every load sits inside its
// row group's branch (`col` is wave-uniform: the branches are scalar): a Pacific column issues no
// load from `iso`, which has no row for it.
__device__ __forceinline__ double imp_twobasin_wa(const double *__restrict__ iso,
                                                  const double *__restrict__ zon,
                                                  const double *__restrict__ so, int col, int third,
                                                  int nz, int i) {
  if (col < third) {
    const size_t k = (size_t)col * nz + i;
    return (iso[k] + zon[k] - so[k]) * 1e6;
  }
  if (col < 2 * third) return (-iso[(size_t)col * nz + i]) * 1e6;
  const size_t k = (size_t)(col - third) * nz + i;
  return (-zon[k] - so[k]) * 1e6;
}

// The rows of column `col`'s system with coefficient set `sel`, factored into f; q1 = what
// PM_COL_BZBOT adds to row 1's right-hand side.  Static data, wA and dt only.  Under
// PM_OP_WA_TWOBASIN (pm_column_steps_implicit_twobasin only) wA_g / zon_g / so_g are the three
// overturning arrays and the forcing is formed here.
template <int P>
__device__ __forceinline__ void imp_build(ImpFactors<P> &f, double &q1, const pm_columns &c,
                                          const double *__restrict__ wA_g, int col, int sel,
                                          double dt, int ops, bool use_bzbot, double bzbot,
                                          int lane, const double *__restrict__ zon_g = nullptr,
                                          const double *__restrict__ so_g = nullptr) {
  const int nz = c.nz;
  const size_t base = (size_t)col * nz;
  const size_t coef = (size_t)sel * c.ncols * nz + base;
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
      const double wa = (ops & PM_OP_WA_TWOBASIN)
                            ? imp_twobasin_wa(wA_g, zon_g, so_g, col, c.ncols / 3, nz, i)
                            : (wA_g ? wA_g[base + i] : 0.0);
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
  q1 = use_bzbot ? level_value<P>(rq, 1) : 0.0;
}

// what a step reads of its column besides the state and the factors
struct ImpCol {
  bool do_conv, use_bzbot;
  double bs, bzbot, N2min, dz0;
};

// One step of a wave-owned column: convect() (column.py:251-271), the right-hand side with the
// boundary values imposed, the solve.  `bbot` and `q1` are arguments: the fused loop's BC switch
// changes them between steps.
template <int P>
__device__ __forceinline__ void imp_step(const ImpFactors<P> &f, double (&b)[P],
                                         const double (&z)[P], const ImpCol &k, double bbot,
                                         double q1, int ops, int lane, int nz,
                                         const double *__restrict__ zg) {
  if ((ops & PM_OP_CONVECT) && k.do_conv) {
    col_convect<WAVE, P>(b, z, k.bs, k.N2min, lane, lane, nz, zg);
    col_pin<P>(b);
  }
  if (ops & PM_OP_VERTADVDIFF) {
    double r[P], x[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      double v = b[p];
      if (i == nz - 1 && !k.do_conv) v = k.bs;   // column.py:230-231
      if (i == 0) v = k.use_bzbot ? 0.0 : bbot;  // (BZBOT: row 1 does not read level 0)
      if (i == 1 && i <= nz - 2 && k.use_bzbot) v = v + q1;
      if (i >= nz) v = 0.0;
      r[p] = v;
    }
    imp_solve<P>(f, r, x, lane);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      if (!(i >= 1 && i <= nz - 2)) x[p] = r[p];  // boundary values as imposed
    }
    if (k.use_bzbot) {
      const double x1 = level_value<P>(x, 1);
      if (lane == 0) x[0] = x1 - k.bzbot * k.dz0;  // column.py:233 with the new b[1]
    }
#pragma unroll
    for (int p = 0; p < P; ++p) b[p] = x[p];
  }
}

}  // namespace pm
