// launch.hip.h -- the host side of a launch, shared by the launchers of the per-member kernels and
// of the series kernels: block sizing against the CU's LDS, the launch itself, row alignment,
// runtime flags as template arguments.  Host code only, inline / templates throughout (compiled
// into several translation units).
#pragma once
#include <type_traits>
#include "common.hip.h"

namespace pm {

constexpr size_t LDS_PER_CU = 160 * 1024;        // gfx950: what one block can ask for at most
constexpr size_t LDS_DYN_UNRAISED = 64 * 1024;   // dynamic LDS a kernel gets without asking

// Waves per block, of max_wpb, max_wpb / 2, .., 1: the count that keeps the most waves resident
// on a CU when every wave needs per_wave_bytes of LDS (the larger block on a tie); resident_cap =
// the waves per CU the kernel's registers allow.  (Thermal wind at nz = 200, 14 KB per wave:
// blocks of 4 leave room for 8 waves, single waves for 11.)
inline int waves_per_block(size_t per_wave_bytes, int max_wpb, int resident_cap) {
  int wpb = 1, best = 0;
  for (int w = max_wpb; w >= 1; w >>= 1) {
    int resident = (int)(LDS_PER_CU / (per_wave_bytes * w)) * w;
    if (resident > resident_cap) resident = resident_cap;
    if (best < resident) {
      best = resident;
      wpb = w;
    }
  }
  return wpb;
}

// Waves per block of a kernel whose block also holds `shared_bytes` of tables: max_wpb, halved
// until the block fits the CU (1 may still not fit: the caller checks the total).
inline int waves_per_block_fitting(size_t per_wave_bytes, size_t shared_bytes, int max_wpb) {
  int wpb = max_wpb;
  while (wpb > 1 && per_wave_bytes * wpb + shared_bytes > LDS_PER_CU) wpb >>= 1;
  return wpb;
}

// kernel<<<grid, block, lds_bytes, st>>>(args...), its dynamic-LDS limit raised first if need be
// (a 1-D grid or block is given as a plain integer)
template <class... P, class... A>
int launch_dyn(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
               const A &...args) {
  if (lds_bytes > LDS_DYN_UNRAISED)
    PM_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds_bytes));
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
  PM_HIP(hipGetLastError());
  return PM_OK;
}

// The IEEE leg of a fused JN2018 launch: single-wave blocks (lds_one_wave bytes each) that redo
// the members the launch flagged, at most 64 of them; kernel_vec has the 16-byte row accesses.
template <class... P, class... A>
int launch_ieee_leg(void (*kernel_vec)(P...), void (*kernel)(P...), bool vec, int n,
                    size_t lds_one_wave, hipStream_t st, const A &...args) {
  const unsigned g1 = (unsigned)((n + 63) / 64 < 64 ? (n + 63) / 64 : 64);
  return launch_dyn(vec ? kernel_vec : kernel, g1, 64, lds_one_wave, st, args...);
}

template <class... T>
inline bool aligned16(const T *...p) {
  return ((((unsigned long long)p & 15ull) == 0ull) && ...);
}

// 16-byte row accesses of a column batch: every row the step reads or writes starts 16-byte
// aligned and holds whole lanes of P levels
inline bool rows_aligned(const pm_columns &c, const double *wA, int P) {
  return c.nz % P == 0 && aligned16(c.b, c.area, c.kappa, c.dAkappa, wA);
}

// fn(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): runtime flags as template arguments.
// fn is instantiated for EVERY combination; it guards those without a kernel with `if constexpr`.
template <class F>
int with_bools(F &&fn) {
  return fn();
}
template <class F, class... B>
int with_bools(F &&fn, bool b0, B... rest) {
  auto bound = [&](auto c0) { return with_bools([&](auto... cs) { return fn(c0, cs...); }, rest...); };
  return b0 ? bound(std::true_type{}) : bound(std::false_type{});
}

}  // namespace pm
