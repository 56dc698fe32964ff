// psi_so.hip.h -- K4: Southern-Ocean residual overturning Psi = Psi_Ek + Psi_GM.
//
// Arithmetic restated from the reference (nothing copied):
//   Psi_SO.ys          src/pymoc/modules/psi_SO.py:106-140
//   Psi_SO.calc_N2     src/pymoc/modules/psi_SO.py:142-162
//   tapers             src/pymoc/modules/psi_SO.py:164-216
//   Psi_SO.calc_Ekman  src/pymoc/modules/psi_SO.py:218-243
//   Psi_SO.calc_GM     src/pymoc/modules/psi_SO.py:277-331 (+bc_GM :245-275)
//   Psi_SO.solve       src/pymoc/modules/psi_SO.py:333-354
//
// One wavefront per member, lane l owns levels [l*P, l*P+P).
//  * ys(b): the reference root-finds bs(y) = b with scipy brentq (xtol 2e-12); bs(y) is an
//    np.interp closure, i.e. piecewise linear, so the root is taken directly: first
//    crossing north of argmin(bs), one linear solve.  Agrees with brentq to ~1e-15
//    relative.  A level that EQUALS a node value of bs north of the minimum and south of the last
//    node is the exception: over a plateau of bs every point is a root and brentq ends where its
//    iteration first meets f == 0 (kilometres from the plateau's southern end), and on a single
//    node it ends within xtol of the node -- such a level runs brentq_interp, so it is the
//    reference's bit for bit (b == min(bs) and b == bs[-1] are brentq's own two ends, returned
//    before its first step: y[argmin] and y[-1]).  Per level, and no work for any other level.
//    Members whose bs is NOT monotone north of its minimum have several
//    crossings and the reference returns whichever one brentq's iteration lands on
//    (examples/run_single_global_basin.py gets there): those members run brentq itself
//    (brentq_interp below, SciPy's iteration step for step) and are flagged in `status`.
//  * GM boundary-value problem (c != None): the reference calls scipy solve_bvp
//    (4th-order Lobatto IIIA collocation, adaptive mesh, tol 1e-3).  Here the same
//    collocation scheme runs on the grid refined R-fold; u' is eliminated interval by
//    interval, each lane condenses its R sub-intervals to one 2x2 element (static
//    condensation), and the remaining nz-point system is solved without a serial sweep: the
//    node elimination `so_merge` is associative, so a prefix and a suffix scan of the
//    elements (in-lane merges + 6 DPP scan steps each) give every node its closing row.
#pragma once
#include "common.hip.h"
#include "launch.hip.h"

namespace pm {

constexpr int SO_WAVES_PER_BLOCK = 4;

// scipy.optimize.brentq(f, xa, xb) for f(x) = np.interp(x, xp, fp) - target with SciPy's
// defaults xtol = 2e-12, rtol = 4 eps, maxiter = 100 (scipy/optimize/Zeros/brentq.c,
// scipy 1.15.3): the same bracketing / secant / inverse-quadratic / bisection decisions in
// the same arithmetic, so a multi-root bracket ends on the root the reference ends on.
__device__ __noinline__ double brentq_interp(const double *xp, const double *fp, int n,
                                             double target, double xa, double xb) {
  const double xtol = 2e-12, rtol = 8.881784197001252e-16;
  double xpre = xa, xcur = xb, xblk = 0., fblk = 0., spre = 0., scur = 0.;
  double fpre = interp_sorted(xpre, xp, fp, n) - target;
  double fcur = interp_sorted(xcur, xp, fp, n) - target;
  if (fpre == 0) return xpre;
  if (fcur == 0) return xcur;
  if (__builtin_signbit(fpre) == __builtin_signbit(fcur)) return __builtin_nan("");
  for (int it = 0; it < 100; ++it) {
    if (fpre != 0 && fcur != 0 && (__builtin_signbit(fpre) != __builtin_signbit(fcur))) {
      xblk = xpre;
      fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (fabs(fblk) < fabs(fcur)) {
      xpre = xcur;
      xcur = xblk;
      xblk = xpre;
      fpre = fcur;
      fcur = fblk;
      fblk = fpre;
    }
    const double delta = (xtol + rtol * fabs(xcur)) / 2;
    const double sbis = (xblk - xcur) / 2;
    if (fcur == 0 || fabs(sbis) < delta) return xcur;
    if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
      double stry;
      if (xpre == xblk) {  // secant
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {  // inverse quadratic
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
      }
      const double lim1 = fabs(spre), lim2 = 3 * fabs(sbis) - delta;
      if (2 * fabs(stry) < (lim1 < lim2 ? lim1 : lim2)) {
        spre = scur;
        scur = stry;
      } else {
        spre = sbis;
        scur = sbis;
      }
    } else {
      spre = sbis;
      scur = sbis;
    }
    xpre = xcur;
    fpre = fcur;
    if (fabs(scur) > delta)
      xcur += scur;
    else
      xcur += (sbis > 0 ? delta : -delta);
    fcur = interp_sorted(xcur, xp, fp, n) - target;
  }
  return xcur;
}

__device__ __forceinline__ double np_maximum(double a, double b) {
  // np.maximum propagates NaN
  if (a != a) return a;
  if (b != b) return b;
  return a > b ? a : b;
}

// 1/x to ~1 ulp: hardware estimate + two Newton steps (5 instructions instead of the ~12 of
// a correctly rounded division).  Only for the GM boundary-value solve, whose parity bar is
// 1e-9 against the oracle and 1e-5 against SciPy's adaptive solve_bvp -- never on a bitwise path.
__device__ __forceinline__ double so_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
  y = __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
  return y;
}

// one Newton step (~1e-14): only for the residual ESTIMATE, which feeds threshold tests
__device__ __forceinline__ double so_rcp1(double x) {
  const double y = __builtin_amdgcn_rcp(x);
  return __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
}

struct SoElem {  // condensed 2x2 element of an interval: rows for its left/right node
  double a11, a12, c1, a21, a22, c2;
};

// Collocation element of one sub-interval [x0, x1] of  u'' = q (u - T), q = N2/c^2:
// S = u'_0 + u'_1 and D = u'_1 - u'_0 as affine functions of (u_0, u_1).
__device__ __forceinline__ SoElem so_sub_element(double h, double q0, double q1, double qm,
                                                 double r0, double r1, double rm) {
#pragma clang fp contract(fast)
  // divisions by the constants 12 and 6 and the repeated 1/h, 1/al are multiplications by
  // reciprocals here (<= 1 ulp each; this solve is compared at 1e-9 / 1e-5, not bitwise)
  const double h2_12 = h * h * (1. / 12.), h_6 = h * (1. / 6.), two_h = 2. * so_rcp(h);
  const double ral = so_rcp(1. + h2_12 * qm);
  const double sA = -two_h * (1. + h2_12 * q0);
  const double sB = two_h * (1. + h2_12 * q1);
  const double sC = -h_6 * (r1 - r0);
  const double dA = h_6 * (q0 + 2. * qm) * ral;
  const double dB = h_6 * (q1 + 2. * qm) * ral;
  const double dC = -h_6 * (r0 + r1 + 4. * rm) * ral;
  SoElem e;
  e.a11 = sA - dA;
  e.a12 = sB - dB;
  e.c1 = -(sC - dC);
  e.a21 = -(sA + dA);
  e.a22 = -(sB + dB);
  e.c2 = sC + dC;
  return e;
}

// eliminate the node shared by E (left) and e (right)
__device__ __forceinline__ SoElem so_merge(const SoElem &E, const SoElem &e) {
#pragma clang fp contract(fast)
  const double rD = so_rcp(E.a22 + e.a11);
  const double w1 = E.a12 * rD, w2 = e.a21 * rD;
  const double cc = E.c2 + e.c1;
  SoElem o;
  o.a11 = E.a11 - w1 * E.a21;
  o.a12 = -w1 * e.a12;
  o.c1 = E.c1 - w1 * cc;
  o.a21 = -w2 * E.a21;
  o.a22 = e.a22 - w2 * e.a12;
  o.c2 = e.c2 - w2 * cc;
  return o;
}

// Lane movement of the scans by DPP (vector-ALU moves) instead of ds_bpermute (LDS pipe, and
// an LDS round trip of latency per scan step).  GFX9 DPP controls: row_shr:d = 0x110 + d
// (lane i <- lane i-d inside its row of 16), row_shl:d = 0x100 + d, row_bcast:15 = 0x142 (lane
// 15 of every row to all of the next row), row_bcast:31 = 0x143 (lane 31 to the upper half);
// lanes without a source, and rows masked out, receive 0.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ double so_dpp(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROWS, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROWS, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ SoElem so_dpp(const SoElem &e) {
  SoElem o;
  o.a11 = so_dpp<CTRL, ROWS>(e.a11);
  o.a12 = so_dpp<CTRL, ROWS>(e.a12);
  o.c1 = so_dpp<CTRL, ROWS>(e.c1);
  o.a21 = so_dpp<CTRL, ROWS>(e.a21);
  o.a22 = so_dpp<CTRL, ROWS>(e.a22);
  o.c2 = so_dpp<CTRL, ROWS>(e.c2);
  return o;
}
__device__ __forceinline__ double so_lane_value(double x, int src_lane) {  // src_lane: constant
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src_lane);
  return __hiloint2double(hi, lo);
}

// Inclusive prefix scan of chunk elements over the wave: on return lane i holds the element of
// [first node of lane 0, last node of lane i].  Lanes with `has` are a prefix of the wave.
// Rows of 16 by doubling, then the row totals: 6 merges per lane like the plain doubling scan,
// associated differently (this solve is compared at 1e-11, never bitwise).
__device__ __forceinline__ SoElem so_prefix_scan(SoElem PL, bool has, int lane) {
  const int li = lane & 15;
  SoElem o = so_dpp<0x111>(PL);
  if (li >= 1 && has) PL = so_merge(o, PL);
  o = so_dpp<0x112>(PL);
  if (li >= 2 && has) PL = so_merge(o, PL);
  o = so_dpp<0x114>(PL);
  if (li >= 4 && has) PL = so_merge(o, PL);
  o = so_dpp<0x118>(PL);
  if (li >= 8 && has) PL = so_merge(o, PL);
  o = so_dpp<0x142, 0xa>(PL);
  if ((lane & 16) && has) PL = so_merge(o, PL);
  o = so_dpp<0x143, 0xc>(PL);
  if (lane >= 32 && has) PL = so_merge(o, PL);
  return PL;
}

// Suffix scan: on return lane i holds the element of [first node of lane i, last node of the
// last lane with `has`]; nhas = number of lanes with `has` (they are a prefix of the wave).
__device__ __forceinline__ SoElem so_lane_value(const SoElem &e, int src_lane) {
  SoElem o;
  o.a11 = so_lane_value(e.a11, src_lane);
  o.a12 = so_lane_value(e.a12, src_lane);
  o.c1 = so_lane_value(e.c1, src_lane);
  o.a21 = so_lane_value(e.a21, src_lane);
  o.a22 = so_lane_value(e.a22, src_lane);
  o.c2 = so_lane_value(e.c2, src_lane);
  return o;
}
__device__ __forceinline__ SoElem so_select(bool first, const SoElem &a, const SoElem &b) {
  SoElem o;
  o.a11 = first ? a.a11 : b.a11;
  o.a12 = first ? a.a12 : b.a12;
  o.c1 = first ? a.c1 : b.c1;
  o.a21 = first ? a.a21 : b.a21;
  o.a22 = first ? a.a22 : b.a22;
  o.c2 = first ? a.c2 : b.c2;
  return o;
}
__device__ __forceinline__ SoElem so_suffix_scan(SoElem PR, int nhas, int lane) {
  const int li = lane & 15;
  SoElem o = so_dpp<0x101>(PR);
  if (li + 1 < 16 && lane + 1 < nhas) PR = so_merge(PR, o);
  o = so_dpp<0x102>(PR);
  if (li + 2 < 16 && lane + 2 < nhas) PR = so_merge(PR, o);
  o = so_dpp<0x104>(PR);
  if (li + 4 < 16 && lane + 4 < nhas) PR = so_merge(PR, o);
  o = so_dpp<0x108>(PR);
  if (li + 8 < 16 && lane + 8 < nhas) PR = so_merge(PR, o);
  {  // rows 0 and 2 continue into rows 1 and 3
    const SoElem o16 = so_lane_value(PR, 16), o48 = so_lane_value(PR, 48);
    o = so_select(lane < 32, o16, o48);
    if (!(lane & 16) && (lane | 15) + 1 < nhas) PR = so_merge(PR, o);
  }
  o = so_lane_value(PR, 32);
  if (lane < 32 && 32 < nhas) PR = so_merge(PR, o);
  return PR;
}

// Suffix scan of affine maps u_i = A_i + B_i u_(i+1): on return A is u_i given that the map of
// the last lane is a constant (B = 0 there).
__device__ __forceinline__ double so_affine_suffix_scan(double A, double B, int lane) {
#pragma clang fp contract(fast)
  const int li = lane & 15;
#define SO_AFFINE_STEP(D)                                                  \
  {                                                                        \
    const double A2 = so_dpp<0x100 + D>(A), B2 = so_dpp<0x100 + D>(B);     \
    if (li + D < 16) {                                                     \
      A = __builtin_fma(B, A2, A);                                         \
      B = B * B2;                                                          \
    }                                                                      \
  }
  SO_AFFINE_STEP(1)
  SO_AFFINE_STEP(2)
  SO_AFFINE_STEP(4)
  SO_AFFINE_STEP(8)
#undef SO_AFFINE_STEP
  {  // rows 0 and 2 continue into rows 1 and 3
    const double A16 = so_lane_value(A, 16), B16 = so_lane_value(B, 16);
    const double A48 = so_lane_value(A, 48), B48 = so_lane_value(B, 48);
    const double A2 = lane < 32 ? A16 : A48, B2 = lane < 32 ? B16 : B48;
    if (!(lane & 16)) {
      A = __builtin_fma(B, A2, A);
      B = B * B2;
    }
  }
  {  // the lower half continues into the upper half
    const double A2 = so_lane_value(A, 32);
    if (lane < 32) A = __builtin_fma(B, A2, A);
  }
  return A;
}

// inclusive prefix sum over the wave
__device__ __forceinline__ int so_prefix_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
  return v;
}

// ---------------------------------------------------------------------------------------
// The GM boundary-value problem on the mesh scipy.integrate.solve_bvp itself ends on
// (a.bvp_refine <= 0, the default; a.bvp_refine = R > 0 selects the fixed R-fold mesh, 2-3x
// faster and ~1e-6 from the reference).
// solve_bvp (scipy 1.15.3 _bvp.py, defaults tol = 1e-3, max_nodes = 1000, as psi_SO.py:319-321
// calls it) loops: Newton on the collocation system of the current mesh -- the ODE is linear,
// Newton lands on that system's exact solution (checked against SciPy: 6e-16) -- then the rms
// residual of every interval (estimate_rms_residuals: 5-point Lobatto rule on the C1 cubic
// spline of (y, f), residuals relative to 1 + |f|; the mid-point term vanishes for a converged
// collocation solution), then modify_mesh: one node into intervals with tol < rms < 100 tol,
// two into those with rms >= 100 tol; until nothing is added.  Original levels stay nodes
// and the spline interpolates its nodes, so res.sol(z) is the nodal solution there.
// Following the same decisions gives SciPy's mesh (node for node on every golden case) and
// 1e-14 agreement with the reference where the fixed 8-fold mesh was 1e-6 away.
//
// One wave per member, mesh in LDS.  A mesh pass:
//   A  every lane condenses its chunk of consecutive intervals into one element (so_merge);
//   B  prefix / suffix scans of the chunk elements across the wave (as in the fixed-mesh path);
//   C  the first node of every chunk closes with its own row; D  a Thomas sweep inside each
//      chunk between the two now-known chunk ends (all chunks in parallel);
//   E  nodal derivatives, F  residuals and insertion counts per interval, G  the new mesh by
//      a prefix sum of the counts.
// Two implementations.  nz <= SO_REG_NZ: `so_gm_adaptive_reg`, every lane keeps its <= 4
// intervals in registers, meshes up to SO_REG_CAP nodes (config 4 and the golden cases end on
// 85-207; a member whose mesh grows further is flagged with status bit 3 and redone by the
// follow-up launch, k_psi_so<.., FIX>).  Larger grids and that follow-up: `so_gm_adaptive`, chunks
// of any length worked through LDS scratch, meshes up to solve_bvp's own max_nodes.
constexpr int SO_REG_NZ = 128, SO_REG_CAP = 256, SO_REG_C = SO_REG_CAP / 64;
constexpr int SO_BIG_CAP = 1000;
// LDS doubles per wave.  reg: x, q, t, u [CAP] + short mark[CAP], and up[CAP] laid over the
// staging area (y, bs, tau, T, N2: dead once the node tables are filled; the result vector
// `out` lies there too, written when up is dead).  big: x[2][CAP], u[CAP], up[CAP], z[nz],
// sN[nz], sT[nz] + shorts seg[2][CAP], cnt[CAP], + out[nz] behind the staging area.
__host__ __device__ inline bool so_reg_path(int nz) { return (nz + 63) / 64 <= SO_REG_NZ / 64; }
__host__ __device__ inline int so_big_doubles(int nz) {
  return 4 * SO_BIG_CAP + 3 * nz + (3 * SO_BIG_CAP * 2 + 7) / 8;
}
__host__ __device__ inline int so_lds_doubles(int nz, int ny, bool has_c, bool adaptive,
                                              bool force_big = false) {
  const int stage = 3 * ny + (has_c ? 2 * nz : 0);
  if (!adaptive) return stage;
  if (so_reg_path(nz) && !force_big)
    return (stage > SO_REG_CAP ? stage : SO_REG_CAP) + 4 * SO_REG_CAP + (SO_REG_CAP * 2 + 7) / 8;
  return stage + so_big_doubles(nz) + nz;
}

struct SoMesh {
  double *x, *xn, *u, *up;
  const double *z, *N2, *T, *sN, *sT;  // sN, sT: slopes of the np.interp closures per interval
  short *seg, *segn, *cnt;
  int nz;
  double rc2;
};

// q = N2(x)/c^2 and r = q T(x) at mesh node i / at a point xe of original interval k
__device__ __forceinline__ void so_coef_at(const SoMesh &w, int k, double xe, double &q,
                                           double &r) {
  // slope * (x - xp[k]) + fp[k] (np.interp); at the upper level the node value itself
  const double zk = w.z[k];
  const bool top = xe == w.z[k + 1];
  const double dx = xe - zk;
  const double n2 = top ? w.N2[k + 1] : w.sN[k] * dx + w.N2[k];
  const double tv = top ? w.T[k + 1] : w.sT[k] * dx + w.T[k];
  q = n2 * w.rc2;
  r = q * tv;
}

__device__ __forceinline__ SoElem so_mesh_element(const SoMesh &w, int i) {
  const int k = w.seg[i];
  const double x0 = w.x[i], x1 = w.x[i + 1], h = x1 - x0;
  double q0, r0, q1, r1, qm, rm;
  so_coef_at(w, k, x0, q0, r0);
  so_coef_at(w, k, x1, q1, r1);
  so_coef_at(w, k, x0 + 0.5 * h, qm, rm);
  return so_sub_element(h, q0, q1, qm, r0, r1, rm);
}

// returns the final number of mesh nodes; u at the original levels is left in w.u[pos] and
// copied to out_lds[k] (an LDS array of nz doubles) by the caller-visible tail below
__device__ __forceinline__ int so_gm_adaptive(SoMesh w, double ua, double ub, int lane,
                                              double *out_lds, int *status_bits) {
  const double tol = 1e-3;
  const int max_nodes = 1000;
  const int nz = w.nz;
  int m = nz;
  for (int i = lane; i < nz; i += 64) {
    w.x[i] = w.z[i];
    w.seg[i] = (short)(i < nz - 1 ? i : nz - 2);
  }
  __builtin_amdgcn_wave_barrier();
  for (int pass = 0; pass < 64; ++pass) {  // SciPy has no cap while nodes are added; 64 >> any run
    const int ne = m - 1;
    const int C = (ne + 63) >> 6;
    const int f = lane * C;                       // first interval / first node of the chunk
    const int l = f + C < ne ? f + C : ne;        // one past the last interval; node l ends it
    const bool has = f < ne;
    // ---- A: chunk element
    SoElem TL = SoElem{0., 0., 0., 0., 0., 0.};
    for (int i = f; i < l; ++i) {
      const SoElem e = so_mesh_element(w, i);
      TL = (i == f) ? e : so_merge(TL, e);
    }
    // ---- B: scans (lanes with an empty chunk carry nothing; non-empty lanes are a prefix)
    const int nhas = __builtin_popcountll(__ballot(has));
    const SoElem PL = so_prefix_scan(TL, has, lane);
    const SoElem PR = so_suffix_scan(TL, nhas, lane);
    const SoElem XL = so_dpp<0x138>(PL);  // everything left of this chunk (lane > 0)
    // PR: everything from this chunk's first node to the end of the mesh
    // ---- C: first node of the chunk
    double uf = ua;
    if (has && lane > 0) uf = (XL.c2 + PR.c1 - XL.a21 * ua - PR.a12 * ub) / (XL.a22 + PR.a11);
    double ul = from_next_lane_z(uf);
    const bool next_has = lane + 1 < nhas;
    if (!next_has) ul = ub;
    // ---- D: Thomas inside the chunk, Dirichlet ends uf (node f) and ul (node l)
    if (has) {
      w.u[f] = uf;
      if (l == ne) w.u[ne] = ub;
      // rows j = f+1 .. l-1:  E[j-1].a21 u[j-1] + (E[j-1].a22 + E[j].a11) u[j] + E[j].a12 u[j+1]
      //                       = E[j-1].c2 + E[j].c1
      SoElem ep = so_mesh_element(w, f);
      double dprev = 1., rprev = uf, uprev_c = 0.;  // row of node f: u[f] = uf
      for (int j = f + 1; j < l; ++j) {
        const SoElem ej = so_mesh_element(w, j);
        const double lo = ep.a21, di = ep.a22 + ej.a11, upc = ej.a12, rh = ep.c2 + ej.c1;
        const double wq = lo / dprev;
        const double d2 = di - wq * uprev_c, r2 = rh - wq * rprev;
        w.up[j] = d2;   // scratch: modified diagonal
        w.u[j] = r2;    // scratch: modified right-hand side
        w.xn[j] = upc;  // scratch: super-diagonal
        dprev = d2;
        rprev = r2;
        uprev_c = upc;
        ep = ej;
      }
      double unext = ul;
      for (int j = l - 1; j > f; --j) {
        const double v = (w.u[j] - w.xn[j] * unext) / w.up[j];
        w.u[j] = v;
        unext = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- E: nodal derivative u' (continuous across nodes by construction)
    for (int i = lane; i < ne; i += 64) {
      const SoElem e = so_mesh_element(w, i);
      w.up[i] = 0.5 * (e.a11 * w.u[i] + e.a12 * w.u[i + 1] - e.c1);
      if (i == ne - 1) w.up[ne] = 0.5 * (-e.a21 * w.u[i] - e.a22 * w.u[i + 1] + e.c2);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- F: rms residual and insertion count of every interval (estimate_rms_residuals)
    int added = 0;
    const double s37 = 0.6546536707079771;  // sqrt(3/7)
    for (int i = lane; i < ne; i += 64) {
      const int k = w.seg[i];
      const double x0 = w.x[i], h = w.x[i + 1] - x0;
      double q0, r0, q1, r1;
      so_coef_at(w, k, x0, q0, r0);
      so_coef_at(w, k, w.x[i + 1], q1, r1);
      const double y0a = w.u[i], y0b = w.u[i + 1], p0a = w.up[i], p0b = w.up[i + 1];
      const double p1a = q0 * y0a - r0, p1b = q1 * y0b - r1;
      const double rh = so_rcp(h);
      const double sl0 = (y0b - y0a) * rh, t0 = (p0a + p0b - 2 * sl0) * rh;
      const double sl1 = (p0b - p0a) * rh, t1 = (p1a + p1b - 2 * sl1) * rh;
      const double c00 = t0 * rh, c01 = (sl0 - p0a) * rh - t0;
      const double c10 = t1 * rh, c11 = (sl1 - p1a) * rh - t1;
      const double xmid = x0 + 0.5 * h, s = 0.5 * h * s37;
      double acc = 0.;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const double xe = side == 0 ? xmid + s : xmid - s;
        const double dx = xe - x0;
        const double Y0 = ((c00 * dx + c01) * dx + p0a) * dx + y0a;
        const double Y1 = ((c10 * dx + c11) * dx + p1a) * dx + p0a;
        const double Y0p = (3 * c00 * dx + 2 * c01) * dx + p0a;
        const double Y1p = (3 * c10 * dx + 2 * c11) * dx + p1a;
        double qe, re;
        so_coef_at(w, k, xe, qe, re);
        const double F0 = Y1, F1 = qe * Y0 - re;
        const double e0 = (Y0p - F0) * so_rcp(1 + __builtin_fabs(F0));
        const double e1 = (Y1p - F1) * so_rcp(1 + __builtin_fabs(F1));
        acc += e0 * e0 + e1 * e1;
      }
      // rms = sqrt(0.5 * 49/90 * acc) compared through its square
      const double ms = 0.5 * (49. / 90. * acc);
      const int c = (ms >= (100 * tol) * (100 * tol)) ? 2 : ((ms > tol * tol) ? 1 : 0);
      w.cnt[i] = (short)c;
      added += c;
    }
    added = __builtin_amdgcn_readlane(so_prefix_sum(added), 63);
    if (added == 0) break;                       // status 0
    static_assert(SO_BIG_CAP >= 1000, "the general solver follows meshes up to max_nodes");
    if (m + added > max_nodes) {
      // solve_bvp stops here with status 1 ("maximum number of mesh nodes is exceeded") and
      // returns the solution of this mesh: so do we, and say so (status bit 3)
      *status_bits |= 8;
      break;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- G: new mesh (modify_mesh); chunk-wise prefix sum of 1 + cnt
    int mine = 0;
    for (int i = f; i < l; ++i) mine += 1 + w.cnt[i];
    const int incl = so_prefix_sum(mine);
    int pos = incl - mine;
    for (int i = f; i < l; ++i) {
      const double xa = w.x[i], xb = w.x[i + 1];
      const short sg = w.seg[i];
      const int c = w.cnt[i];
      w.xn[pos] = xa;
      w.segn[pos++] = sg;
      if (c == 1) {
        w.xn[pos] = 0.5 * (xa + xb);
        w.segn[pos++] = sg;
      } else if (c == 2) {
        w.xn[pos] = (2 * xa + xb) / 3;
        w.segn[pos++] = sg;
        w.xn[pos] = (xa + 2 * xb) / 3;
        w.segn[pos++] = sg;
      }
    }
    if (lane == 0) {
      w.xn[m + added - 1] = w.x[m - 1];
      w.segn[m + added - 1] = w.seg[m - 1];
    }
    m += added;
    double *tx = w.x;
    w.x = w.xn;
    w.xn = tx;
    short *ts = w.seg;
    w.seg = w.segn;
    w.segn = ts;
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_amdgcn_wave_barrier();
  // the original levels are mesh nodes: node i starts original interval seg[i] iff x[i] == z[seg[i]]
  for (int i = lane; i < m; i += 64) {
    const int k = w.seg[i];
    if (w.x[i] == w.z[k]) out_lds[k] = w.u[i];
    if (i == m - 1) out_lds[nz - 1] = w.u[i];
  }
  __builtin_amdgcn_wave_barrier();
  return m;
}

// ---- register-resident variant (nz <= SO_REG_NZ, meshes <= SO_REG_CAP nodes) -------------
// N2 and T are np.interp closures over the column grid and every mesh interval lies inside one
// original interval, so both are LINEAR on it: the tables q = N2/c^2 and t = T are kept per
// mesh NODE; mid-points, inserted nodes and the Lobatto points take linear combinations of
// their interval's end values (1e-16 from the np.interp expression; this solve is compared at
// 1e-11, its mesh decisions are threshold tests).  A pass, per lane (<= SO_REG_C intervals):
//   elements from the node tables -> chunk element -> prefix scan of chunk elements (6 doubles)
//   -> the chunk-end values obey  u_l = A + B u_l(next lane): a suffix scan of AFFINE maps
//   (2 doubles, no division) -> Thomas inside the chunk, derivatives, residuals, counts -- all
//   in registers -> the new mesh is written back in place after one wave barrier.
struct SoRegMesh {
  double *x, *q, *t, *u, *up;
  short *mark;  // original level of a node, -1 for inserted nodes
};

// One collocation solve on the current mesh for chunks of exactly <= RC intervals per lane
// (RC = ceil((m-1)/64), wave-uniform): nodal values to w.u, nodal derivatives to w.up.
template <int RC>
__device__ __forceinline__ void so_reg_solve(const SoRegMesh &w, int m, double ua, double ub,
                                             int lane PM_TICK_PARAM) {
#pragma clang fp contract(fast)  // not a bitwise path: let mul+add pairs fuse
  const int ne = m - 1;
  const int f = lane * RC;
  int nl = ne - f;
  nl = nl < 0 ? 0 : (nl > RC ? RC : nl);
  const bool has = nl > 0;
  PM_TICK(0)
  // ---- elements of the chunk
  SoElem e[RC];
  {
    int i0 = f < m - 1 ? f : m - 1;
    double x0 = w.x[i0], q0 = w.q[i0], t0 = w.t[i0];
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      const int i1 = f + c + 1 < m ? f + c + 1 : m - 1;
      const double x1 = w.x[i1], q1 = w.q[i1], t1 = w.t[i1];
      const double qm = 0.5 * (q0 + q1), tm = 0.5 * (t0 + t1);
      e[c] = so_sub_element(x1 - x0, q0, q1, qm, q0 * t0, q1 * t1, qm * tm);
      x0 = x1;
      q0 = q1;
      t0 = t1;
    }
  }
  SoElem TL = e[0];
#pragma unroll
  for (int c = 1; c < RC; ++c)
    if (c < nl) TL = so_merge(TL, e[c]);
  PM_TICK(1)
  // ---- prefix scan: PL = element of [node 0, this chunk's last node]
  const SoElem PL = so_prefix_scan(TL, has, lane);
  PM_TICK(2)
  // ---- chunk-end values: (PL.a22 + TLn.a11) u_l + TLn.a12 u_l(next) = PL.c2 + TLn.c1 - PL.a21 ua
  const double n11 = from_next_lane_z(TL.a11), n12 = from_next_lane_z(TL.a12),
               nc1 = from_next_lane_z(TL.c1);
  const bool next_has = lane < 63 && f + RC < ne;  // the chunks with intervals are a prefix
  double A = ub, B = 0.;
  if (has && next_has) {
    const double rden = so_rcp(PL.a22 + n11);
    A = (PL.c2 + nc1 - PL.a21 * ua) * rden;
    B = -n12 * rden;
  }
  const double ul = so_affine_suffix_scan(A, B, lane);
  double uf = from_prev_lane_z(ul);
  if (lane == 0) uf = ua;
  PM_TICK(3)
  // ---- Thomas inside the chunk between uf (node f) and ul (node f + nl)
  double us[RC + 1];
  {
    double rd[RC], rr[RC];
    double rdprev = 1., rprev = uf, cprev = 0.;
#pragma unroll
    for (int c = 1; c < RC; ++c) {
      const double wq = e[c - 1].a21 * rdprev;
      const double d2 = (e[c - 1].a22 + e[c].a11) - wq * cprev;
      const double r2 = (e[c - 1].c2 + e[c].c1) - wq * rprev;
      rd[c] = so_rcp(d2);
      rr[c] = r2;
      rdprev = rd[c];
      rprev = r2;
      cprev = e[c].a12;
    }
    double unext = ul;
    us[0] = uf;
#pragma unroll
    for (int c = RC; c >= 1; --c) {
      double v = unext;  // c >= nl: the chunk end (or beyond it: unused)
      if (c < nl) v = (rr[c < RC ? c : RC - 1] - e[c < RC ? c : RC - 1].a12 * unext) * rd[c < RC ? c : RC - 1];
      us[c] = v;
      unext = v;
    }
  }
  // ---- nodal values and derivatives (continuous across nodes by construction) go to LDS;
  // the elements die here
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    if (c < nl) {
      w.u[f + c] = us[c];
      w.up[f + c] = 0.5 * (e[c].a11 * us[c] + e[c].a12 * us[c + 1] - e[c].c1);
      if (c == nl - 1 && !next_has) {
        w.u[ne] = ub;
        w.up[ne] = 0.5 * (-e[c].a21 * us[c] - e[c].a22 * us[c + 1] + e[c].c2);
      }
    }
  }
  PM_TICK(4)
}

__device__ __forceinline__ int so_gm_adaptive_reg(const SoRegMesh &w, int nz, double ua,
                                                  double ub, int lane, double *out_lds,
                                                  int *status_bits PM_TICK_PARAM) {
#pragma clang fp contract(fast)  // not a bitwise path: let mul+add pairs fuse
  const double tol = 1e-3;
  const int max_nodes = 1000;
  constexpr int RC = SO_REG_C;
  int m = nz;
  PM_TICK(8)
  for (int pass = 0; pass < 64; ++pass) {  // SciPy has no cap while nodes are added; 64 >> any run
    const int ne = m - 1;
    const int C = (ne + 63) >> 6;                 // <= RC because m <= SO_REG_CAP
    const int f = lane * C;                       // first interval / first node of the chunk
    int nl = ne - f;                              // intervals of this lane
    nl = nl < 0 ? 0 : (nl > C ? C : nl);
    const bool has = nl > 0;
    switch (C) {  // wave-uniform
      case 1: so_reg_solve<1>(w, m, ua, ub, lane PM_TICK_ARG); break;
      case 2: so_reg_solve<2>(w, m, ua, ub, lane PM_TICK_ARG); break;
      case 3: so_reg_solve<3>(w, m, ua, ub, lane PM_TICK_ARG); break;
      default: so_reg_solve<4>(w, m, ua, ub, lane PM_TICK_ARG); break;
    }
    const bool next_has = lane < 63 && f + C < ne;
    __builtin_amdgcn_wave_barrier();
    // ---- rms residual and insertion count of every interval (estimate_rms_residuals); a real
    // loop (register pressure); the counts of the lane's intervals are packed 2 bits each
    int cntbits = 0, added = 0;
    if (has) {
      const double s37 = 0.6546536707079771;  // sqrt(3/7)
      double x0 = w.x[f], q0 = w.q[f], t0 = w.t[f], y0a = w.u[f], p0a = w.up[f];
#pragma unroll 1
      for (int c = 0; c < nl; ++c) {
        const int i1 = f + c + 1;
        const double x1 = w.x[i1], q1 = w.q[i1], t1 = w.t[i1], y0b = w.u[i1], p0b = w.up[i1];
        const double h = x1 - x0;
        const double p1a = q0 * y0a - q0 * t0, p1b = q1 * y0b - q1 * t1;
        const double rh = so_rcp(h);
        const double sl0 = (y0b - y0a) * rh, t0c = (p0a + p0b - 2 * sl0) * rh;
        const double sl1 = (p0b - p0a) * rh, t1c = (p1a + p1b - 2 * sl1) * rh;
        const double c00 = t0c * rh, c01 = (sl0 - p0a) * rh - t0c;
        const double c10 = t1c * rh, c11 = (sl1 - p1a) * rh - t1c;
        const double sq = (q1 - q0) * rh, st = (t1 - t0) * rh;
        const double hs = 0.5 * h, s = hs * s37;
        double acc = 0.;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          const double dx = side == 0 ? hs + s : hs - s;
          const double Y0 = ((c00 * dx + c01) * dx + p0a) * dx + y0a;
          const double Y1 = ((c10 * dx + c11) * dx + p1a) * dx + p0a;
          const double Y0p = (3 * c00 * dx + 2 * c01) * dx + p0a;
          const double Y1p = (3 * c10 * dx + 2 * c11) * dx + p1a;
          const double qe = sq * dx + q0, te = st * dx + t0;
          const double F0 = Y1, F1 = qe * Y0 - qe * te;
          const double e0 = (Y0p - F0) * so_rcp1(1 + __builtin_fabs(F0));
          const double e1 = (Y1p - F1) * so_rcp1(1 + __builtin_fabs(F1));
          acc += e0 * e0 + e1 * e1;
        }
        // rms = sqrt(0.5 * 49/90 * acc) compared through its square
        const double ms = 0.5 * (49. / 90. * acc);
        const int k = (ms >= (100 * tol) * (100 * tol)) ? 2 : ((ms > tol * tol) ? 1 : 0);
        cntbits |= k << (2 * c);
        added += k;
        x0 = x1;
        q0 = q1;
        t0 = t1;
        y0a = y0b;
        p0a = p0b;
      }
    }
    PM_TICK(5)
    // ---- new mesh (modify_mesh): positions by a prefix sum of the nodes each lane writes; its
    // last entry is the new node count
    const int mine = nl + added;
    const int incl = so_prefix_sum(mine);
    added = __builtin_amdgcn_readlane(incl, 63) - ne;
    const bool grow = added != 0 && m + added <= max_nodes && m + added <= SO_REG_CAP;
    if (!grow) {
      if (added != 0 && m + added <= max_nodes) *status_bits |= 8;  // SciPy would refine further
      // (beyond max_nodes SciPy stops with this solution too)
      break;
    }
    // in place: everything a lane needs is read before the barrier
    int pos = incl - mine;
    double xs[RC + 1], qs[RC + 1], ts[RC + 1];
    short mk[RC + 1];
#pragma unroll
    for (int c = 0; c <= RC; ++c) {
      const int i = f + c < m ? f + c : m - 1;
      xs[c] = w.x[i];
      qs[c] = w.q[i];
      ts[c] = w.t[i];
      mk[c] = w.mark[i];
    }
    __builtin_amdgcn_wave_barrier();
    const double third = 1. / 3.;  // the inserted x differ from SciPy's (2 x_i + x_i+1) / 3 by <= 1 ulp
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      if (c < nl) {
        const double xa = xs[c], xb = xs[c + 1], qa = qs[c], qb = qs[c + 1], ta = ts[c],
                     tb = ts[c + 1];
        const int k = (cntbits >> (2 * c)) & 3;
        const double wa = k == 1 ? 0.5 : 2. * third, wb = k == 1 ? 0.5 : third;
        w.x[pos] = xa;
        w.q[pos] = qa;
        w.t[pos] = ta;
        w.mark[pos] = mk[c];
        if (k >= 1) {
          w.x[pos + 1] = wa * xa + wb * xb;
          w.q[pos + 1] = wa * qa + wb * qb;
          w.t[pos + 1] = wa * ta + wb * tb;
          w.mark[pos + 1] = (short)-1;
        }
        if (k == 2) {
          w.x[pos + 2] = wb * xa + wa * xb;
          w.q[pos + 2] = wb * qa + wa * qb;
          w.t[pos + 2] = wb * ta + wa * tb;
          w.mark[pos + 2] = (short)-1;
        }
        pos += 1 + k;
      }
    }
    if (has && !next_has) {  // the last node of the mesh
#pragma unroll
      for (int c = 1; c <= RC; ++c)
        if (c == nl) {
          w.x[pos] = xs[c];
          w.q[pos] = qs[c];
          w.t[pos] = ts[c];
          w.mark[pos] = mk[c];
        }
    }
    m += added;
    __builtin_amdgcn_wave_barrier();
    PM_TICK(6)
    PM_COUNT(7)
  }
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < m; i += 64) {
    const int k = w.mark[i];
    if (k >= 0 && k < nz) out_lds[k] = w.u[i];
  }
  __builtin_amdgcn_wave_barrier();
  return m;
}

// BVP: the member batch uses the F2010 boundary-value smoother (c is not None).  Without it
// (JN2018, config 5) the kernel is a third of the registers and runs 4+ waves per SIMD.
// FIX: the follow-up launch of the adaptive solve for nz <= SO_REG_NZ.  A small persistent grid
// scans `status` for members whose mesh outgrew the register-resident solver (bit 3) and redoes
// exactly those with the general solver (meshes up to solve_bvp's own 1000 nodes), so that the
// result is solve_bvp's for ANY input; it exits at once when no member is flagged (~2 us).
// One member's Psi_SO.solve: `s_y` = the wave's so_lds_doubles(...) doubles of LDS.  The body of
// k_psi_so, and a diagnostic phase of the persistent run kernels (coupled_run.hip).
template <int P, bool BVP, bool FIX = false>
__device__ __forceinline__ void so_member(const pm_psi_so &a, int ops, int m_raw, double *s_y,
                                          int lane) {
  const bool m_ok = m_raw < a.n;
  const int m = m_ok ? m_raw : a.n - 1;
  const int nz = a.nz, ny = a.ny;
  PM_TICK_INIT
  PM_WAVE_BEGIN
  const bool has_c = BVP;  // == (a.flags & PM_SO_HAS_C) != 0, checked by the launcher
  const bool tau_arr = (a.flags & PM_SO_TAU_ARRAY) != 0;
  const bool adaptive = has_c && a.bvp_refine <= 0;
  double *s_bs = s_y + ny;
  double *s_tau = s_bs + ny;
  double *s_w = s_tau + ny;  // BVP workspace: T and N2 on the column grid
  const size_t base = (size_t)m * nz;

  // ---- every global operand of the member is requested here, before the first use of any:
  // taken where they are used, the loads form five dependent round trips to memory (surface
  // profiles -> levels -> scalars -> the neighbours for N2 -> the grid for the mesh), a
  // quarter of the member's time under load
  double z[P], b[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    const int ic = i < nz ? i : nz - 1;
    z[p] = a.z[ic];
    b[p] = a.b[base + ic];
  }
  const int jf = lane < ny ? lane : ny - 1;
  const double bs_f = a.bs[(size_t)m * ny + jf], y_f = a.y[jf];
  const double tau_f = tau_arr ? a.tau[(size_t)m * ny + jf] : 0.;
  const double tau_s = tau_arr ? 0. : a.tau[m];
  const double KGM = a.KGM[m];  // (non-NULL for every op: checked at the C-ABI)

  // ---- stage the member's surface profiles; min / argmin of bs (np.min, np.argmin)
  double mn = __builtin_inf();
  int mi = 0x7fffffff;
  bool nanv = false;
  for (int j = lane; j < ny; j += 64) {
    const bool first = j == lane;
    const double v = first ? bs_f : a.bs[(size_t)m * ny + j];
    s_y[j] = first ? y_f : a.y[j];
    s_bs[j] = v;
    s_tau[j] = first ? tau_f : (tau_arr ? a.tau[(size_t)m * ny + j] : 0.);
    nanv |= (v != v);
    if (v < mn) {
      mn = v;
      mi = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(mn, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (ov < mn || (ov == mn && oi < mi)) {
      mn = ov;
      mi = oi;
    }
  }
  const bool bs_nan = __ballot(nanv) != 0ull;
  __builtin_amdgcn_wave_barrier();
  const int minind = mi < ny ? mi : 0;
  const double bsmin = mn, bs_last = s_bs[ny - 1];
  const double y0g = s_y[0], yN = s_y[ny - 1];
  bool nonmono = false;
  for (int j = minind + lane; j < ny - 1; j += 64) nonmono |= s_bs[j + 1] < s_bs[j];
  const bool ambiguous = __ballot(nonmono) != 0ull;

  // ---- per level: outcrop latitude ys (psi_SO.py:106-140)
  // The interval search of the unambiguous case, for all of the lane's levels at once: the
  // same probes as a per-level `while (j < hi)` loop, but the levels' LDS round trips overlap
  // (a uniform trip count; a level that has converged repeats nothing).  Lanes on the other
  // branches search as well and ignore the result (indices stay inside [minind, ny-2]).
  int sj[P];
#pragma unroll
  for (int p = 0; p < P; ++p) sj[p] = minind;
  if (a.ys_in == nullptr && !ambiguous && !bs_nan) {  // wave-uniform
    int sh[P];
#pragma unroll
    for (int p = 0; p < P; ++p) sh[p] = ny - 2;
    for (int span = ny - 2 - minind; span > 0; span >>= 1) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int mid = (sj[p] + sh[p]) >> 1;
        const bool open = sj[p] < sh[p];
        const bool ge = s_bs[mid + 1] >= b[p];
        sh[p] = (open && ge) ? mid : sh[p];
        sj[p] = (open && !ge) ? mid + 1 : sj[p];
      }
    }
  }
  double ys[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    const int ic = i < nz ? i : nz - 1;
    double yv;
    if (a.ys_in != nullptr) {  // the caller's own inversion of a callable bs(y)
      yv = a.ys_in[base + ic];
    } else if (b[p] < bsmin) {
      yv = y0g - 1e3;
    } else if (b[p] > bs_last) {
      yv = yN;
    } else if (b[p] != b[p] || bs_nan) {
      yv = __builtin_nan("");
    } else {
      // first crossing north of argmin: bs is non-decreasing there (not `ambiguous`), so the
      // first j with bs[j+1] >= b is a lower bound -- 6 probes instead of a walk over y
      // (`ambiguous`: j = minind, unused)
      const int j = sj[p];
      const double f0 = s_bs[j], f1 = s_bs[j + 1];
      // b on a node value north of the minimum: bs may hold it over a plateau, where brentq ends
      // wherever its iteration first meets f == 0, and on a single node it ends within its
      // tolerance of the node, not on it -- such a level follows the iteration.  The two ends need
      // none: f0 == b only at j = minind (brentq returns its lower end at once), and b == bs[-1]
      // is met at y[-1] before the first step.
      const bool on_node = f1 == b[p] && f0 != b[p] && j + 1 < ny - 1;
      if (ambiguous || on_node)  // several crossings too: the one brentq's iteration finds
        yv = brentq_interp(s_y, s_bs, ny, b[p], s_y[minind], yN);
      else if (f0 == b[p])
        yv = s_y[j];
      else if (f1 == b[p])
        yv = yN;
      else
        yv = s_y[j] + (b[p] - f0) / ((f1 - f0) / (s_y[j + 1] - s_y[j]));
    }
    ys[p] = yv;
    if (a.ys && i < nz && m_ok) a.ys[base + i] = yv;
  }

  // ---- calc_Ekman (psi_SO.py:218-243)
  double tmean_scalar = 0.;
  if (!tau_arr) {
    // np.mean of 100 copies of tau (pairwise: 8 accumulators x 12 rounds, tree, 4 tail)
    double r8 = tau_s;
    for (int k = 1; k < 12; ++k) r8 += tau_s;
    double res = ((r8 + r8) + (r8 + r8)) + ((r8 + r8) + (r8 + r8));
    for (int k = 96; k < 100; ++k) res += tau_s;
    tmean_scalar = res / 100.;
  }
  double ek_sv[P], ekraw[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    double tau_ave;
    if (a.tau_ave_in != nullptr) {  // the caller's own average of a callable tau(y)
      tau_ave = a.tau_ave_in[base + (i < nz ? i : nz - 1)];
    } else if (!tau_arr) {
      // tau + 0*y is tau unless the outcrop latitude is non-finite
      tau_ave = (ys[p] - ys[p] == 0.) ? tmean_scalar : __builtin_nan("");
    } else {
      Linspace lin;
      lin.init(ys[p], yN, 100);
      double r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = interp_sorted(lin.at(k), s_y, s_tau, ny);
      for (int k = 8; k < 96; k += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] += interp_sorted(lin.at(k + q), s_y, s_tau, ny);
      }
      double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (int k = 96; k < 100; ++k) res += interp_sorted(lin.at(k), s_y, s_tau, ny);
      tau_ave = res / 100.;
    }
    double sill = 1., ekt = 1.;
    if (a.flags & PM_SO_HAS_HSILL) {
      double mm = a.z[0] + a.Hsill - z[p];
      mm = mm > 0. ? mm : 0.;
      sill = 1. - (mm * mm) / (a.Hsill * a.Hsill);
    }
    if (a.flags & PM_SO_HAS_HEK) {
      double mm = z[p] + a.HEk;
      mm = mm > 0 ? mm : 0;
      ekt = 1 - (mm * mm) / (a.HEk * a.HEk);
    } else if (i == nz - 1) {
      ekt = 0.;  // taper = ones with last element 0 (psi_SO.py:213-216)
    }
    ekraw[p] = tau_ave / a.f / a.rho * a.L * sill * ekt;  // :243
    ek_sv[p] = ekraw[p] / 1e6;                             // :349
    if (!(ops & PM_SO_OP_EKMAN))  // calc_GM() alone reads the caller's self.Psi_Ek
      ek_sv[p] = a.Psi_Ek[base + (i < nz ? i : nz - 1)];
    else if (a.Ek_raw && i < nz && m_ok)
      a.Ek_raw[base + i] = ekraw[p];
  }
  if (!(ops & PM_SO_OP_GM)) {  // calc_Ekman() alone
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      if (i < nz && m_ok) a.Psi_Ek[base + i] = ek_sv[p];
    }
    return;
  }

  // ---- calc_GM (psi_SO.py:277-331)
  double dy[P], temp[P], bott[P], topt[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const double d = yN - ys[p];
    dy[p] = (0.1 > d) ? 0.1 : d;  // Python max(d, eps): eps only if eps > d (NaN stays)
    bott[p] = 1.;
    topt[p] = 1.;
    if (a.flags & PM_SO_HAS_HTAPERBOT) {
      double mm = a.z[0] + a.Htaperbot - z[p];
      mm = mm > 0. ? mm : 0.;
      bott[p] = 1. - (mm * mm) / (a.Htaperbot * a.Htaperbot);
    }
    if (a.flags & PM_SO_HAS_HTAPERTOP) {
      double mm = z[p] + a.Htapertop;
      mm = mm > 0 ? mm : 0;
      topt[p] = 1 - (mm * mm) / (a.Htapertop * a.Htapertop);
    }
  }
  int gm_status = 0;
  if constexpr (!BVP) {
#pragma unroll
    for (int p = 0; p < P; ++p)
      temp[p] = KGM * np_maximum(z[p] / dy[p], -a.smax) * a.L * topt[p] * bott[p];  // :325
  } else {
    // --- F2010 boundary-value smoother (psi_SO.py:308-323)
    double *s_T = s_w, *s_N2 = s_w + nz;
    const double c2 = a.c * a.c;
    // the levels above and below come from the neighbouring slots / lanes (the same values the
    // arrays hold; level nz-1 never looks up, level 0 never down)
    const double b_nl = from_next_lane_z(b[0]), z_nl = from_next_lane_z(z[0]);
    const double b_pl = from_prev_lane_z(b[P - 1]), z_pl = from_prev_lane_z(z[P - 1]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      const double b_up = p + 1 < P ? b[p + 1 < P ? p + 1 : p] : b_nl;
      const double z_up = p + 1 < P ? z[p + 1 < P ? p + 1 : p] : z_nl;
      const double b_dn = p > 0 ? b[p > 0 ? p - 1 : 0] : b_pl;
      const double z_dn = p > 0 ? z[p > 0 ? p - 1 : 0] : z_pl;
      if (i < nz) {
        s_T[i] = KGM * z[p] / dy[p] * a.L * topt[p] * bott[p];  // :310
        double n2;  // calc_N2, :154-160
        if (i == 0)
          n2 = (b_up - b[p]) / (z_up - z[p]);
        else if (i == nz - 1)
          n2 = (b[p] - b_dn) / (z[p] - z_dn);
        else
          n2 = (b_up - b_dn) / ((z_up - z[p]) + (z[p] - z_dn));
        s_N2[i] = n2;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // boundary values (bc_GM, :270-275); Psi_Ek[0], Psi_Ek[-1] live in lanes 0 / last
    double ua0 = 0., ub0 = 0.;
    if (a.flags & PM_SO_BVP_WITH_EK) {
      const int last_lane = (nz - 1) / P, last_p = (nz - 1) % P;
      double v_last = 0.;
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (p == last_p) v_last = ek_sv[p];
      ua0 = -(__shfl(ek_sv[0], 0, 64) * 1e6);
      ub0 = -(__shfl(v_last, last_lane, 64) * 1e6);
    }
    if (!FIX && P <= SO_REG_NZ / 64 && adaptive) {  // wave-uniform: follow solve_bvp's own mesh
      const int stage = 3 * ny + 2 * nz;
      double *wk = s_y + (stage > SO_REG_CAP ? stage : SO_REG_CAP);
      SoRegMesh ms;
      ms.x = wk;
      ms.q = wk + SO_REG_CAP;
      ms.t = wk + 2 * SO_REG_CAP;
      ms.u = wk + 3 * SO_REG_CAP;
      ms.mark = reinterpret_cast<short *>(wk + 4 * SO_REG_CAP);
      ms.up = s_y;          // over the staging area: written only after the tables are filled
      double *outl = s_y;   // ... and read for the last time before `out` is written
      const double rc2 = 1. / c2;
#pragma unroll
      for (int p = 0; p < P; ++p) {  // (the lane's own entries of s_N2 / s_T)
        const int i = lane * P + p;
        if (i < nz) {
          ms.x[i] = z[p];
          ms.q[i] = s_N2[i] * rc2;
          ms.t[i] = s_T[i];
          ms.mark[i] = (short)i;
        }
      }
      __builtin_amdgcn_wave_barrier();
      so_gm_adaptive_reg(ms, nz, ua0, ub0, lane, outl, &gm_status PM_TICK_ARG);
      PM_TICK(9)
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        temp[p] = outl[i < nz ? i : nz - 1];
      }
    } else if ((FIX || P > SO_REG_NZ / 64) && adaptive) {
      double *wk = s_w + 2 * nz;
      SoMesh ms;
      ms.x = wk;
      ms.xn = wk + SO_BIG_CAP;
      ms.u = wk + 2 * SO_BIG_CAP;
      ms.up = wk + 3 * SO_BIG_CAP;
      double *zl = wk + 4 * SO_BIG_CAP;
      double *sNl = zl + nz, *sTl = zl + 2 * nz;
      ms.seg = reinterpret_cast<short *>(zl + 3 * nz);
      ms.segn = ms.seg + SO_BIG_CAP;
      ms.cnt = ms.segn + SO_BIG_CAP;
      double *outl = wk + so_big_doubles(nz);
      for (int i = lane; i < nz; i += 64) {
        zl[i] = a.z[i];
        if (i < nz - 1) {
          const double hz = a.z[i + 1] - a.z[i];
          sNl[i] = (s_N2[i + 1] - s_N2[i]) / hz;
          sTl[i] = (s_T[i + 1] - s_T[i]) / hz;
        }
      }
      ms.z = zl;
      ms.sN = sNl;
      ms.sT = sTl;
      ms.N2 = s_N2;
      ms.T = s_T;
      ms.nz = nz;
      ms.rc2 = 1. / c2;
      __builtin_amdgcn_wave_barrier();
      so_gm_adaptive(ms, ua0, ub0, lane, outl, &gm_status);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        temp[p] = outl[i < nz ? i : nz - 1];
      }
    } else {
    const int R = a.bvp_refine > 0 ? a.bvp_refine : 8;
    const double rc2 = 1. / c2, rR = 1. / (double)R;
    SoElem Ecl[P];  // condensed element of interval [z_k, z_k+1], k = lane*P + p
#pragma unroll
    for (int p = 0; p < P; ++p) Ecl[p] = SoElem{0., 0., 0., 0., 0., 0.};
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int k = lane * P + p;  // interval [z_k, z_k+1]
      if (k < nz - 1) {
        const double zk = z[p], hz = a.z[k + 1] - zk;
        const double N0 = s_N2[k], N1 = s_N2[k + 1], T0 = s_T[k], T1 = s_T[k + 1];
        const double sN = (N1 - N0) / hz, sT = (T1 - T0) / hz;
        SoElem E = {0., 0., 0., 0., 0., 0.};
        double xl = zk, ql = N0 * rc2, rl = ql * T0;
        for (int j = 0; j < R; ++j) {
          double xr, qr, rr;
          if (j == R - 1) {
            xr = a.z[k + 1];
            qr = N1 * rc2;
            rr = qr * T1;
          } else {
            xr = zk + hz * ((double)(j + 1) * rR);
            qr = (sN * (xr - zk) + N0) * rc2;
            rr = qr * (sT * (xr - zk) + T0);
          }
          const double h = xr - xl, xm = xl + 0.5 * h;
          const double qm = (sN * (xm - zk) + N0) * rc2;
          const double rm = qm * (sT * (xm - zk) + T0);
          const SoElem e = so_sub_element(h, ql, qr, qm, rl, rr, rm);
          E = (j == 0) ? e : so_merge(E, e);
          xl = xr;
          ql = qr;
          rl = rr;
        }
        Ecl[p] = E;
      }
    }
    const double ua = ua0, ub = ub0;
    // The nz-1 condensed elements are combined by the associative node-elimination `so_merge`:
    // a prefix scan gives L_k (the element of [z_0, z_k+1]) and a suffix scan R_k (the element
    // of [z_k, z_nz-1]); interior node i then closes with its own row
    //   L_{i-1}.a21 ua + (L_{i-1}.a22 + R_i.a11) u_i + R_i.a12 ub = L_{i-1}.c2 + R_i.c1.
    // Each scan is P-1 merges inside a lane, 6 DPP scan steps across the wave and P merges to
    // fold the carried element in -- no serial sweep over the rows.
    const int ne = nz - 1;                       // number of elements
    const int nv = ne - lane * P;                // valid elements of this lane (may be <= 0)
    const int cnt = nv < 0 ? 0 : (nv > P ? P : nv);
    SoElem Lp[P], Rp[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Lp[p] = (p == 0) ? Ecl[0] : ((p < cnt) ? so_merge(Lp[p > 0 ? p - 1 : 0], Ecl[p]) : Lp[p > 0 ? p - 1 : 0]);
    }
#pragma unroll
    for (int p = P - 1; p >= 0; --p) {
      if (p == P - 1)
        Rp[p] = Ecl[p];
      else
        Rp[p] = (p + 1 < cnt) ? so_merge(Ecl[p], Rp[p + 1]) : Ecl[p];
    }
    // wave scans of the lane totals (lanes with cnt == 0 carry nothing)
    SoElem TL = Lp[P - 1];  // element of all valid intervals of this lane (Lp saturates at cnt-1)
    SoElem TR = Rp[0];
    const bool has = cnt > 0;
    const int nhas = __builtin_popcountll(__ballot(has));  // lanes to the left of a valid lane are full
    TL = so_prefix_scan(TL, has, lane);
    TR = so_suffix_scan(TR, nhas, lane);
    const SoElem XL = so_dpp<0x138>(TL);  // everything left of this lane
    const SoElem XR = so_dpp<0x130>(TR);  // everything right of this lane
    const bool xr_has = lane + 1 < nhas;
    // L_{i-1} of this lane's first node lives in the previous lane
    SoElem Lfull[P], Rfull[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Lfull[p] = (lane > 0) ? so_merge(XL, Lp[p]) : Lp[p];
      Rfull[p] = xr_has ? so_merge(Rp[p], XR) : Rp[p];
    }
    const SoElem Lprev = so_dpp<0x138>(Lfull[P - 1]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = lane * P + p;
      const SoElem &Lm = (p == 0) ? Lprev : Lfull[p > 0 ? p - 1 : 0];
      const SoElem &Rm = Rfull[p];
      double u = (i == 0) ? ua : ub;
      if (i >= 1 && i <= nz - 2)
        u = (Lm.c2 + Rm.c1 - Lm.a21 * ua - Rm.a12 * ub) / (Lm.a22 + Rm.a11);
      temp[p] = u;
    }
    }  // fixed R-fold mesh
  }
  // limit Psi_GM to -Psi_Ek on isopycnals that do not outcrop (:329-330)
  const double width = yN - y0g;
  bool bad = false;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    if (dy[p] > width) temp[p] = np_maximum(temp[p], -ek_sv[p] * 1e6);
    const double gm = temp[p] / 1e6;        // :350
    double psi = ek_sv[p] + gm;             // :351
    if (i == 0) psi = 0.;                   // :354
    if (i < nz && m_ok) {
      if (ops & PM_SO_OP_EKMAN) a.Psi_Ek[base + i] = ek_sv[p];
      a.Psi_GM[base + i] = gm;
      a.Psi[base + i] = psi;
      if (a.GM_raw) a.GM_raw[base + i] = temp[p];
      bad |= !isfinite(psi);
    }
  }
  if (a.status) {
    const bool anybad = __ballot(bad) != 0ull;
    if (lane == 0 && m_ok)
      a.status[m] = (ambiguous ? 1 : 0) | (anybad ? 2 : 0) | (bs_nan ? 4 : 0) | gm_status;
  }
  PM_TICK(10)
  PM_TICK_FLUSH
  PM_WAVE_END(m_raw)
}

#ifndef PM_DIAG_DEVICE_FUNCTIONS_ONLY  // (coupled_run.hip.h shares so_member only)
template <int P, bool BVP, bool FIX = false>
__global__ __launch_bounds__(64 * SO_WAVES_PER_BLOCK) void k_psi_so(pm_psi_so a, int ops) {
  extern __shared__ double lds_all[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wave_id = blockIdx.x * (blockDim.x >> 6) + wave;
  const int per_wave = so_lds_doubles(a.nz, a.ny, BVP, BVP && a.bvp_refine <= 0, FIX);
  double *s_y = lds_all + (size_t)wave * per_wave;
  // FIX: every lane looks at one member's status, a ballot collects the flagged ones of 64
  int scan_next = wave_id * 64, cur_base = 0;
  unsigned long long pending = 0ull;
  for (;;) {
    int m_raw = wave_id;
    if constexpr (FIX) {
      while (pending == 0ull) {
        if (scan_next >= a.n) return;  // wave-uniform: nothing left for this wave
        cur_base = scan_next;
        scan_next += gridDim.x * (blockDim.x >> 6) * 64;
        const int mm = cur_base + lane;
        pending = __ballot(mm < a.n && (a.status[mm] & 8) != 0);
      }
      m_raw = cur_base + __builtin_ctzll(pending);
      pending &= pending - 1ull;
    }
    so_member<P, BVP, FIX>(a, ops, m_raw, s_y, lane);
    if constexpr (!FIX) break;
    __builtin_amdgcn_wave_barrier();  // the next flagged member reuses the wave's LDS
  }
}

template <int P, bool BVP>
int launch_psi_so_impl(const pm_psi_so &a, int ops, hipStream_t st) {
  const bool adaptive = BVP && a.bvp_refine <= 0;
  const size_t per_wave = (size_t)so_lds_doubles(a.nz, a.ny, BVP, adaptive) * sizeof(double);
  const int wpb = waves_per_block(per_wave, SO_WAVES_PER_BLOCK, 32);
  const size_t lds = per_wave * wpb;
  if (lds > LDS_PER_CU) return fail(PM_EINVAL, "psi_so needs %zu B of LDS per member", lds);
  const unsigned grid = (unsigned)((a.n + wpb - 1) / wpb);
  if (const int rc = launch_dyn(k_psi_so<P, BVP>, grid, 64 * wpb, lds, st, a, ops)) return rc;
  if constexpr (BVP && P <= SO_REG_NZ / 64) {
    if (adaptive && a.status && (ops & PM_SO_OP_GM) && !(a.flags & PM_SO_NO_FIXUP)) {
      // members whose mesh outgrew the register-resident solver: redone by the general one
      const size_t lds_fix = (size_t)so_lds_doubles(a.nz, a.ny, true, true, true) * sizeof(double);
      const unsigned gfix = (unsigned)(a.n < 256 ? a.n : 256);
      return launch_dyn(k_psi_so<P, BVP, true>, gfix, 64, lds_fix, st, a, ops);
    }
  }
  return PM_OK;
}

template <int P>
int launch_psi_so(const pm_psi_so &a, int ops, hipStream_t st) {
  return (a.flags & PM_SO_HAS_C) ? launch_psi_so_impl<P, true>(a, ops, st)
                                 : launch_psi_so_impl<P, false>(a, ops, st);
}

inline int dispatch_psi_so(const pm_psi_so &a, int ops, hipStream_t st) {
  const int P = (a.nz + 63) / 64;
  switch (P) {
#define PM_CASE(PP) \
  case PP:          \
    return launch_psi_so<PP>(a, ops, st);
    PM_CASE(1) PM_CASE(2) PM_CASE(3) PM_CASE(4) PM_CASE(5) PM_CASE(6) PM_CASE(7) PM_CASE(8)
#undef PM_CASE
  }
  return fail(PM_EINVAL, "nz=%d unsupported by psi_so (max 512)", a.nz);
}


#endif  // PM_DIAG_DEVICE_FUNCTIONS_ONLY

}  // namespace pm
