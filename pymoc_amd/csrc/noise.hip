// noise.hip -- stochastic forcing of an ensemble (pymoc_amd.NoiseForcing).
//
// (no counterpart: an extension.)  A noise-driven ensemble perturbs the forcing arrays every
// launch re-reads (cols.bs, so.tau, bs_SO, ml.b_rest, ml.surflux) with one red-noise state per
// (target, member).  The deviates are made where they are consumed: a counter-based generator
// (Philox4x32-10) keyed by the seed and counted by (global member index, application index,
// target) gives every (member, target, application) its own Gaussian deviate, so a deviate
// depends on nothing but those coordinates -- not on the batch size, the shard or the other
// targets of the launch.  include/pymoc_hip.h states the definition; this file follows it
// operation by operation and is built with -ffp-contract=off.
//
// The launch has k_forcing_apply's shape: blockIdx.y is the destination (selected over the
// constant capacity, so the table is read from the kernel arguments at constant offsets), the
// blocks of a destination stride over its flat range of n * len doubles, so base is read and dst
// written coalesced.  Every thread of member m recomputes the deviate and x_out[m] from x_in[m]
// (ten Philox rounds, one log, one cos, one sqrt: registers only, no memory traffic, so the
// threads of a member need not talk to each other); the thread of element 0 stores x_out[m] into
// the buffer the launch does not read.
#include <cmath>
#include "common.hip.h"
#include "philox.hip.h"  // philox_round, noise_deviate: the deviate of include/pymoc_hip.h

namespace pm {

constexpr int NOISE_BLOCK = 256;
constexpr int NOISE_MAX_BLOCKS = 2048;  // per destination: 8 blocks for each of the 256 CUs

struct noise_item {
  double *dst;            // first written element
  const double *base, *pattern, *sigma, *x_in;
  double *x_out, *xi_out;
  double a, b;
  uint32_t total, len;    // n * len < 2^31
  uint32_t per_member, stream;
};

struct noise_args {
  noise_item item[PM_NOISE_MAX_TARGETS];
  uint32_t key0, key1, id_lo, id_hi, j;
};

__global__ void __launch_bounds__(NOISE_BLOCK) k_forcing_noise(noise_args a) {
  noise_item it = a.item[0];
#pragma unroll
  for (int f = 1; f < PM_NOISE_MAX_TARGETS; ++f)
    if (f == (int)blockIdx.y) it = a.item[f];
  const uint32_t nthreads = gridDim.x * NOISE_BLOCK;
  // (i < total < 2^31 and nthreads <= 2^19: i + nthreads does not wrap)
  for (uint32_t i = blockIdx.x * NOISE_BLOCK + threadIdx.x; i < it.total; i += nthreads) {
    const uint32_t m = i / it.len, e = i - m * it.len;
    const uint64_t id = (((uint64_t)a.id_hi << 32) | a.id_lo) + m;
    const double xi = noise_deviate(a.key0, a.key1, id, a.j, it.stream);
    const double x = it.a * it.x_in[m] + (it.sigma[m] * it.b) * xi;
    double v = it.base[i];
    if (it.pattern)
      v += x * it.pattern[it.per_member ? i : e];
    else
      v += x;
    it.dst[i] = v;
    if (e == 0) {
      if (it.x_out) it.x_out[m] = x;
      if (it.xi_out) it.xi_out[m] = xi;
    }
  }
}

}  // namespace pm

using namespace pm;

extern "C" {

int pm_forcing_noise(const struct pm_noise *dp, pm_stream_t stream) {
  PM_REQUIRE(dp, "d is NULL");
  const struct pm_noise &d = *dp;
  PM_REQUIRE(d.ntargets >= 1 && d.ntargets <= PM_NOISE_MAX_TARGETS, "ntargets %d outside [1, %d]",
             d.ntargets, PM_NOISE_MAX_TARGETS);
  PM_REQUIRE(d.n >= 1, "n %d < 1", d.n);
  PM_REQUIRE(d.member0 >= 0, "member0 %lld < 0", (long long)d.member0);
  for (int i = 0; i < d.ntargets; ++i) {
    const pm_noise_target &g = d.target[i];
    PM_REQUIRE(g.dst && g.base && g.sigma && g.x_in, "target %d: NULL pointer", i);
    PM_REQUIRE(g.len >= 1 && g.row0 >= 0, "target %d: len %d < 1 or row0 %lld < 0", i, g.len,
               (long long)g.row0);
    PM_REQUIRE((int64_t)d.n * g.len <= INT32_MAX, "target %d: %lld elements are too many", i,
               (long long)d.n * g.len);
    PM_REQUIRE(std::isfinite(g.a) && g.a >= 0. && g.a <= 1. && std::isfinite(g.b) && g.b >= 0. &&
                   g.b <= 1., "target %d: a %g or b %g is not finite or outside [0, 1]", i, g.a,
               g.b);
    PM_REQUIRE(g.pattern_per_member == 0 || g.pattern_per_member == 1,
               "target %d: pattern_per_member %d is not 0 or 1", i, g.pattern_per_member);
    PM_REQUIRE(g.stream >= 0 && g.stream < PM_NOISE_STREAMS, "target %d: stream %d outside [0, %d)",
               i, g.stream, PM_NOISE_STREAMS);
    for (int k = 0; k < d.ntargets; ++k)
      PM_REQUIRE(!g.x_out || g.x_out != d.target[k].x_in,
                 "target %d: x_out is the x_in of target %d", i, k);
  }
  noise_args a;
  memset(&a, 0, sizeof(a));
  a.key0 = (uint32_t)d.seed;
  a.key1 = (uint32_t)(d.seed >> 32);
  a.id_lo = (uint32_t)(uint64_t)d.member0;
  a.id_hi = (uint32_t)((uint64_t)d.member0 >> 32);
  a.j = d.j;
  uint32_t widest = 0;
  for (int i = 0; i < PM_NOISE_MAX_TARGETS; ++i) {
    // (unused entries repeat target 0: never selected, never dereferenced)
    const pm_noise_target &g = d.target[i < d.ntargets ? i : 0];
    noise_item &it = a.item[i];
    it.dst = g.dst + g.row0 * g.len;
    it.base = g.base;
    it.pattern = g.pattern;
    it.sigma = g.sigma;
    it.x_in = g.x_in;
    it.x_out = g.x_out;
    it.xi_out = g.xi_out;
    it.a = g.a;
    it.b = g.b;
    it.total = (uint32_t)d.n * (uint32_t)g.len;
    it.len = (uint32_t)g.len;
    it.per_member = (uint32_t)g.pattern_per_member;
    it.stream = (uint32_t)g.stream;
    if (it.total > widest) widest = it.total;
  }
  uint32_t bx = (widest + NOISE_BLOCK - 1) / NOISE_BLOCK;
  if (bx > NOISE_MAX_BLOCKS) bx = NOISE_MAX_BLOCKS;
  hipStream_t st = resolve_stream(stream);
  hipLaunchKernelGGL(k_forcing_noise, dim3(bx, (unsigned)d.ntargets), dim3(NOISE_BLOCK), 0, st, a);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

}  // extern "C"
