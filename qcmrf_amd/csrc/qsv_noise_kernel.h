// qsv_noise_kernel.h -- the LDS trajectory kernel template and its launcher (included by qsv_noise.hip, which instantiates
// the kernels without the MEASURE kind, MEAS = false, by qsv_noise_measure.hip, which instantiates those with it in a
// code object of their own, so that the one of qsv_noise.hip holds the kernels it held before the kind existed, and by
// qsv_noise_accept.hip, which instantiates the accept-aware kernels k_noisy_accept in a third).  The body of both kernel templates
// is qsv_noise_lds_shots.inc.
#pragma once
#include "qsv_noise_ops.h"

template <int TPB, int KRAUS, bool MEAS>
__global__ __launch_bounds__(TPB) void k_noisy(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                               int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                               uint64_t* __restrict__ out) {
  constexpr bool ACC = false, K2 = false, DYN = false;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_lds_shots.inc"
}

// k_noisy<TPB, KRAUS, true> over the shots a.first_shot + [0, shots), abandoning at decisive records
template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy_accept(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                      int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                                      uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = false, DYN = false;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_lds_shots.inc"
}

// One launch of an LDS trajectory kernel of tpb threads: as many workgroups as the chip holds at once with 16 << W bytes of
// LDS each, at most l.max_grid (if set) and l.shots; `more` are the arguments the kernel takes behind k_noisy's.
template <class K, class... A>
static hipError_t nz_lds_launch(K kernel, int tpb, const NzLaunch& l, unsigned* grid, A... more) {
  const size_t lds = (size_t)16 << l.W;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  int per_cu = 0;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, tpb, lds);
  if (e != hipSuccess) return e;
  uint64_t g = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(l.n_cu > 0 ? l.n_cu : 1);
  if (l.max_grid > 0 && (uint64_t)l.max_grid < g) g = (uint64_t)l.max_grid;
  if (l.shots < g) g = l.shots;
  *grid = (unsigned)g;
  hipLaunchKernelGGL(kernel, dim3((unsigned)g), dim3(tpb), lds, l.stream, l.d_ops, l.n_ops, l.d_pool, l.W, l.shots, l.seed, l.meas,
                     l.d_out, more...);
  return hipGetLastError();
}

template <int TPB, int KRAUS, bool MEAS = false>
static hipError_t launch_noisy(const NzLaunch& l, unsigned* grid) {
  return nz_lds_launch(k_noisy<TPB, KRAUS, MEAS>, TPB, l, grid);
}
