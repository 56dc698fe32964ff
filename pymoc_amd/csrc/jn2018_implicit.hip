// jn2018_implicit.hip -- the fused Jansen & Nadeau time loop with backward-Euler columns
// (pm_jn2018_steps_implicit): nsteps x [bottom-BC switch -> basin column -> northern column ->
// mixed layer] for one member per wavefront (examples/run_JansenNadeau_2018.py:229-261), with
// wA / Psi_SO / Psibz held fixed.  An EXTENSION with no reference counterpart: the reference's
// columns step with forward Euler, which at the script's own nz = 200 cannot take its dt = 30 d.
//
// The kernel is k_jn2018_steps (so_ml.hip.h) with the column step of k_column_implicit
// (column_implicit.hip.h) in place of col_vertadvdiff: lane l holds levels [l P, l P + P) of both
// columns, the mixed layer lives in registers (ny <= 64) or LDS, the BC switch runs on wave
// broadcasts.  Every device function is the stand-alone kernels' own, so a launch is bit-identical
// to nsteps x [pm_jn2018_bc_switch, pm_column_steps_implicit(1), pm_so_ml_step].
//
// Factors.  Each column keeps its ImpFactors<P> in registers for the launch (the matrix depends on
// static data, wA, dt and the coefficient set only).  The BC switch changes bbot every step -- it
// enters the right-hand side only -- and, rarely, a column's coefficient set: only then is that
// column factored again (from global memory, like load_coef of the explicit loop).
#define PM_SO_ML_DEVICE_FUNCTIONS_ONLY
#include "column_implicit.hip.h"
#include "so_ml.hip.h"
#include "launch.hip.h"

namespace pm {

template <int P, bool SMALLNY>
__global__ __launch_bounds__(64 * ML_WAVES_PER_BLOCK) void k_jn2018_implicit(pm_jn2018 a, double dt,
                                                                            int nsteps) {
  extern __shared__ double lds_all[];
  constexpr int OPS = PM_OP_CONVECT | PM_OP_VERTADVDIFF;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m_raw = blockIdx.x * (blockDim.x >> 6) + wave;
  const bool m_ok = m_raw < a.n;
  const int m = m_ok ? m_raw : a.n - 1;  // a tail wave redoes the last member and stores nothing
  const int n = a.n, nz = a.cols.nz, ny = a.ml.ny;
  const pm_columns &c = a.cols;
  MlLds w;
  w.carve(lds_all + (size_t)wave * MlLds::doubles(nz, ny), nz, ny);
  const size_t bz = (size_t)m * nz, by = (size_t)m * ny;
  const int colb = m, coln = n + m;

  BcState st;
  st.bbot_b = c.bbot[colb];
  st.bbot_n = c.bbot[coln];
  st.ksel_b = c.ksel[colb];
  st.ksel_n = c.ksel[coln];
  auto column = [&](ImpCol &k, int col) {
    const int flags = c.flags ? c.flags[col] : 0;
    k.do_conv = (flags & PM_COL_DO_CONV) != 0;
    k.use_bzbot = (flags & PM_COL_BZBOT) != 0 && c.bzbot != nullptr;
    k.bs = c.bs[col];
    k.bzbot = k.use_bzbot ? c.bzbot[col] : 0.0;
    k.N2min = c.N2min[col];
    k.dz0 = c.z[1] - c.z[0];
  };
  ImpCol kb, kn;
  column(kb, colb);
  column(kn, coln);

  double z[P], bb[P], bn[P];
  load_levels<P>(z, c.z, lane, nz);
  load_levels<P>(bb, c.b + (size_t)colb * nz, lane, nz);
  load_levels<P>(bn, c.b + (size_t)coln * nz, lane, nz);

  ImpFactors<P> fb, fn;
  double q1b, q1n;
  imp_build<P>(fb, q1b, c, a.wA, colb, st.ksel_b, dt, OPS, kb.use_bzbot, kb.bzbot, lane);
  imp_build<P>(fn, q1n, c, a.wA, coln, st.ksel_n, dt, OPS, kn.use_bzbot, kn.bzbot, lane);
  const double PsiSO1 = a.Psi_SO[bz + 1], Pb1 = a.Psi_res_b[bz + 1], Pn1 = a.Psi_res_n[bz + 1];

  for (int i = lane; i < nz; i += 64) w.pm[i] = a.Psi_SO[bz + i];
  for (int j = lane; j < ny; j += 64) w.bs[j] = a.ml.bs[by + j];
  __builtin_amdgcn_wave_barrier();
  MlStatic mc;
  mc.surflux = a.ml.surflux + by;
  mc.rest_mask = a.ml.rest_mask + by;
  mc.b_rest = a.ml.b_rest + by;
  mc.h = a.ml.h;
  mc.L = a.ml.L;
  mc.v_pist = a.ml.v_pist;
  mc.dy = a.ml.y[1] - a.ml.y[0];
  mc.s = a.ml.Ks * dt / (mc.dy * mc.dy);
  int first_pos;
  const bool ml_ok = ml_prepare(w, nz, lane, first_pos);
  if constexpr (!SMALLNY) ml_tables(w, ny, mc.s);  // Thomas factors: only the ordered sweep
  if constexpr (SMALLNY) {  // the block's PCR tables of the Crank-Nicolson system
    double *Tw = lds_all + (size_t)(blockDim.x >> 6) * MlLds::doubles(nz, ny);
    if (wave == 0) ml_build_pcr(Tw, ny, mc.s, lane);
    __syncthreads();
  }
  if (ml_ok) ml_flux_tables(w, mc, ny, lane);
  MlReg q;
  q.bs = q.ps = q.f1 = q.f2 = q.br = 0.;
  q.jh = 0;
  if constexpr (SMALLNY) {
    if (lane < ny) {
      q.bs = w.bs[lane];
      if (ml_ok) {
        q.f1 = w.f1[lane];
        q.f2 = w.f2[lane];
        q.br = w.br[lane];
      }
    }
  }
  // pm_so_ml_step of the last step: did it step (else: status 1, state untouched); did any
  bool last_stepped = false, ps_valid = false;

  // lanes / slots holding levels 0 and 1 of a column
  constexpr int L1 = 1 / P, S1 = 1 % P;
  for (int s = 0; s < nsteps; ++s) {
    // ---- bottom-BC switch (run_JansenNadeau_2018.py:233-254) on wave-uniform scalars
    const double bb0 = lane_value(bb[0], 0), bb1 = lane_value(bb[S1], L1);
    const double bn0 = lane_value(bn[0], 0), bn1 = lane_value(bn[S1], L1);
    const int selb = st.ksel_b, seln = st.ksel_n;
    const double bs0 = SMALLNY ? lane_value(q.bs, 0) : w.bs[0];
    jn2018_bc(st, PsiSO1, Pb1, Pn1, bb0, bb1, bn0, bn1, bs0);
    // a changed coefficient set is another matrix (rare)
    if (st.ksel_b != selb)
      imp_build<P>(fb, q1b, c, a.wA, colb, st.ksel_b, dt, OPS, kb.use_bzbot, kb.bzbot, lane);
    if (st.ksel_n != seln)
      imp_build<P>(fn, q1n, c, a.wA, coln, st.ksel_n, dt, OPS, kn.use_bzbot, kn.bzbot, lane);
    // ---- basin.timestep / north.timestep (:257-258), backward Euler
    imp_step<P>(fb, bb, z, kb, st.bbot_b, q1b, OPS, lane, nz, c.z);
    imp_step<P>(fn, bn, z, kn, st.bbot_n, q1n, OPS, lane, nz, c.z);
    // ---- channel.timestep(b_basin=basin.b, Psi_b=PsiSO.Psi) (:261)
    last_stepped = false;
    if (ml_ok) {
      // (the workspace pointers re-derived from an offset the optimiser cannot see through, as in
      // k_jn2018_steps: hoisted LDS addresses would stay live across the column steps)
      int woff = __builtin_amdgcn_readfirstlane(wave) * MlLds::doubles(nz, ny);
      int moff = (blockDim.x >> 6) * MlLds::doubles(nz, ny);
      asm volatile("" : "+s"(woff), "+s"(moff));
      MlLds w;
      w.carve(lds_all + woff, nz, ny);
      const double *T = lds_all + moff;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        if (i < nz) w.bb[i] = bb[p];
      }
      __builtin_amdgcn_wave_barrier();
      if constexpr (SMALLNY)
        last_stepped = ml_step_reg(q, w, mc, nz, ny, lane, first_pos, dt, T);
      else
        last_stepped = ml_step(w, mc, nz, ny, lane, first_pos, dt);
      ps_valid |= last_stepped;
    }
  }

  bool bad_b = false, bad_n = false, bad_s = false;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = lane * P + p;
    if (i < nz) {
      if (m_ok) {
        c.b[(size_t)colb * nz + i] = bb[p];
        c.b[(size_t)coln * nz + i] = bn[p];
      }
      bad_b |= !isfinite(bb[p]);
      bad_n |= !isfinite(bn[p]);
    }
  }
  if constexpr (SMALLNY) {
    if (lane < ny) {
      bad_s |= !isfinite(q.bs);
      if (m_ok && ps_valid) {  // (a step that did not run leaves bs and Psi_s as they were)
        a.ml.bs[by + lane] = q.bs;
        if (a.ml.Psi_s) a.ml.Psi_s[by + lane] = q.ps;
      }
    }
  } else {
    for (int j = lane; j < ny; j += 64) {
      const double v = w.bs[j];
      bad_s |= !isfinite(v);
      if (m_ok && ps_valid) {
        a.ml.bs[by + j] = v;
        if (a.ml.Psi_s) a.ml.Psi_s[by + j] = w.ps[j];
      }
    }
  }
  // as the launches would leave them: each column's own flag; the mixed layer's status of the
  // LAST step (1: it did not step; else 2 where bs is not finite)
  const bool anyb = __ballot(bad_b) != 0ull, anyn = __ballot(bad_n) != 0ull;
  const bool anys = __ballot(bad_s) != 0ull;
  if (lane == 0 && m_ok) {
    const_cast<double *>(c.bbot)[colb] = st.bbot_b;
    const_cast<double *>(c.bbot)[coln] = st.bbot_n;
    const_cast<int32_t *>(c.ksel)[colb] = st.ksel_b;
    const_cast<int32_t *>(c.ksel)[coln] = st.ksel_n;
    if (c.nonfinite) {
      c.nonfinite[colb] = anyb ? 1 : 0;
      c.nonfinite[coln] = anyn ? 1 : 0;
    }
    if (a.ml.status) a.ml.status[m] = last_stepped ? (anys ? 2 : 0) : 1;
  }
}

template <int P>
static int launch_jn2018_implicit_p(const pm_jn2018 &a, double dt, int nsteps, hipStream_t st) {
  const size_t per_wave = ml_lds_bytes(a.cols.nz, a.ml.ny), prop = ml_prop_bytes(a.ml.ny);
  const int wpb = waves_per_block_fitting(per_wave, prop, ML_WAVES_PER_BLOCK);
  const size_t lds = per_wave * wpb + prop;
  if (lds > LDS_PER_CU)
    return fail(PM_EINVAL, "pm_jn2018_steps_implicit needs %zu B of LDS per member", lds);
  const unsigned grid = (unsigned)((a.n + wpb - 1) / wpb);
  return with_bools(
      [&](auto small) {
        return launch_dyn(k_jn2018_implicit<P, decltype(small)::value>, grid, 64 * wpb, lds, st, a,
                          dt, nsteps);
      },
      a.ml.ny <= 64);
}

int launch_jn2018_implicit(const pm_jn2018 &a, double dt, int nsteps, hipStream_t st) {
  switch ((a.cols.nz + WAVE - 1) / WAVE) {
    case 1: return launch_jn2018_implicit_p<1>(a, dt, nsteps, st);
    case 2: return launch_jn2018_implicit_p<2>(a, dt, nsteps, st);
    case 3: return launch_jn2018_implicit_p<3>(a, dt, nsteps, st);
    case 4: return launch_jn2018_implicit_p<4>(a, dt, nsteps, st);
  }
  return fail(PM_EINVAL, "pm_jn2018_steps_implicit: nz=%d does not fit one wave of 4 levels a lane",
              a.cols.nz);
}

}  // namespace pm
