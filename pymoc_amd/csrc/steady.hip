// steady.hip -- the convergence check of a run to steady state (pymoc_amd.run_to_steady).
//
// The reference's equilibrium experiments step for a fixed length (run_JansenNadeau_2018.py:96-97,
// example_twocol.py:32); a run to steady state instead asks, every few MOC intervals, how far each
// member's prognostic profiles moved since the last check, and retires the members that stopped
// moving.  One launch per check covers every row of the current batch:
//   one wave per row, 4 rows per 256-thread block; the 64 lanes stride over the levels of each
//   drift field (coalesced f64 loads), keep a running fmax of |src - snapshot| and a non-finite
//   flag, overwrite the snapshot with src, and meet in a wave64 __shfl_xor butterfly.  fmax of
//   non-negative doubles is exact and does not depend on order, so the drift is bitwise NumPy's
//   np.max(np.abs(cur - ref)) * scale.  A retiring member (rare, and the same decision for the
//   whole wave) copies its capture rows to the result arrays; the running members of a block are
//   counted with one atomic add per block.
// Traffic: the drift fields are read twice (src, snapshot) and written once (snapshot) -- 3x the
// drift-field bytes per check; DESIGN.md section 9 has the measured time.
#include "common.hip.h"

namespace pm {

constexpr int STEADY_BLOCK = 256;
constexpr int STEADY_ROWS = STEADY_BLOCK / WAVE;

__device__ __forceinline__ double steady_wave_max(double x) {
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

__device__ __forceinline__ int steady_wave_or(int x) {
#pragma unroll
  for (int o = WAVE / 2; o >= 1; o >>= 1) x |= __shfl_xor(x, o);
  return x;
}

// the field loops are unrolled over the constant capacity so that a.drift[f] / a.capture[f] are
// read from the kernel arguments at constant offsets (a runtime index would copy them to scratch)
__global__ void __launch_bounds__(STEADY_BLOCK) k_steady_check(struct pm_steady_check a) {
  __shared__ int running[STEADY_ROWS];
  const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int m = blockIdx.x * STEADY_ROWS + w;
  int still = 0;
  const int k = (m < a.n) ? a.orig[m] : -1;
  if (k >= 0 && k < a.n0 && a.status[k] == PM_STEADY_RUNNING) {
    double d = 0.;
    int bad = 0;
#pragma unroll
    for (int f = 0; f < PM_STEADY_MAX_DRIFT; ++f) {
      if (f < a.ndrift) {
        const double *src = a.drift[f].src + (int64_t)m * a.drift[f].src_stride;
        double *snap = a.drift[f].buf + (int64_t)m * a.drift[f].len;
        const int len = a.drift[f].len;
        for (int i = lane; i < len; i += WAVE) {
          const double x = src[i], y = snap[i];
          bad |= (!__builtin_isfinite(x)) | (!__builtin_isfinite(y));
          d = fmax(d, fabs(x - y));
          snap[i] = x;
        }
      }
    }
    d = steady_wave_max(d);
    bad = steady_wave_or(bad);
    const double dd = d * a.scale;
    int st = PM_STEADY_RUNNING;
    if (bad) {
      st = PM_STEADY_NONFINITE;
    } else {
      const int s = (dd <= a.tol[k]) ? a.streak[k] + 1 : 0;
      if (lane == 0) a.streak[k] = s;
      if (s >= a.consecutive)
        st = PM_STEADY_CONVERGED;
      else if (a.finalize)
        st = PM_STEADY_MAXSTEPS;
    }
    if (lane == 0) a.drift_out[k] = bad ? __builtin_nan("") : dd;
    if (st == PM_STEADY_RUNNING) {
      still = 1;
    } else {
      if (lane == 0) {
        a.status[k] = st;
        a.step_out[k] = a.step;
      }
#pragma unroll
      for (int f = 0; f < PM_STEADY_MAX_CAPTURE; ++f) {
        if (f < a.ncapture) {
          const double *src = a.capture[f].src + (int64_t)m * a.capture[f].src_stride;
          double *dst = a.capture[f].buf + (int64_t)k * a.capture[f].len;
          const int len = a.capture[f].len;
          for (int i = lane; i < len; i += WAVE) dst[i] = src[i];
        }
      }
    }
  }
  if (lane == 0) running[w] = still;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < STEADY_ROWS; ++r) c += running[r];
    if (c) atomicAdd(a.n_running, c);
  }
}

static int steady_field_ok(const pm_steady_field &f) {
  return f.src && f.buf && f.len >= 1 && f.src_stride >= f.len;
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_steady_check(const struct pm_steady_check *c, pm_stream_t stream) {
  PM_REQUIRE(c, "c is NULL");
  const struct pm_steady_check &a = *c;
  PM_REQUIRE(a.n >= 0 && a.n <= a.n0, "bad row count n=%d (0 <= n <= n0=%d)", a.n, a.n0);
  PM_REQUIRE(a.ndrift >= 1 && a.ndrift <= PM_STEADY_MAX_DRIFT, "ndrift %d outside [1, %d]",
             a.ndrift, PM_STEADY_MAX_DRIFT);
  PM_REQUIRE(a.ncapture >= 0 && a.ncapture <= PM_STEADY_MAX_CAPTURE,
             "ncapture %d outside [0, %d]", a.ncapture, PM_STEADY_MAX_CAPTURE);
  PM_REQUIRE(a.consecutive >= 1, "consecutive %d < 1", a.consecutive);
  PM_REQUIRE(a.finalize == 0 || a.finalize == 1, "finalize %d is not 0 or 1", a.finalize);
  PM_REQUIRE(a.step >= 0, "step %lld < 0", (long long)a.step);
  PM_REQUIRE(a.orig && a.tol && a.streak && a.status && a.drift_out && a.step_out && a.n_running,
             "pm_steady_check has a NULL required pointer");
  for (int f = 0; f < a.ndrift; ++f)
    PM_REQUIRE(steady_field_ok(a.drift[f]),
               "drift field %d: NULL pointer, len %d < 1 or src_stride %lld < len", f,
               a.drift[f].len, (long long)a.drift[f].src_stride);
  for (int f = 0; f < a.ncapture; ++f)
    PM_REQUIRE(steady_field_ok(a.capture[f]),
               "capture field %d: NULL pointer, len %d < 1 or src_stride %lld < len", f,
               a.capture[f].len, (long long)a.capture[f].src_stride);
  hipStream_t st = resolve_stream(stream);
  PM_HIP(hipMemsetAsync(a.n_running, 0, sizeof(int32_t), st));
  if (a.n == 0) return PM_OK;
  hipLaunchKernelGGL(k_steady_check, dim3((unsigned)((a.n + STEADY_ROWS - 1) / STEADY_ROWS)),
                     dim3(STEADY_BLOCK), 0, st, a);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
