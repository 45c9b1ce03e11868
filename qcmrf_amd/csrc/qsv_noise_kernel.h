// qsv_noise_kernel.h -- the LDS trajectory kernel template and its launcher (included by qsv_noise.hip, which instantiates
// the kernels without the MEASURE kind, MEAS = false, and by qsv_noise_measure.hip, which instantiates those with it in a
// code object of their own, so that the one of qsv_noise.hip holds the kernels it held before the kind existed).
#pragma once
#include "qsv_noise_ops.h"

template <int TPB, int KRAUS, bool MEAS>
__global__ __launch_bounds__(TPB) void k_noisy(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                               int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                               uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char nz_lds[];
  cplx* st = reinterpret_cast<cplx*>(nz_lds);              // 2^W amplitudes, nothing else
  const uint32_t N = 1u << W;
  const uint32_t tid = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < shots; t += gridDim.x) {
    for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    __syncthreads();
    uint32_t draw = 0;
    uint64_t mword = 0;                                            // the bits MEASURE records wrote (MEAS only)
    for (int k = 0; k < n_ops; ++k) {
      const NzOp o = nz_fetch(ops, k);
      nz_apply<TPB, 1, KRAUS, MEAS>(st, N, o, pool, tid, seed, t, draw, mword);
    }
    // one basis state from |amp|^2: wave 0, lane l owns the contiguous chunk [l C, (l + 1) C)
    if (tid < 64) {
      const uint32_t lane = tid;
      const uint32_t C = N >= 64u ? N >> 6 : 1u;
      const uint32_t lo = lane * C;
      double part = 0.0;
      if (lo < N)
        for (uint32_t k = 0; k < C; ++k) part += norm2(st[lo + k]);
      const double incl = wave_scan(part, lane);
      double excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 0.0;
      const double total = __shfl(incl, 63, 64);
      const double r = philox_u01(seed, t, NZ_STREAM_SAMPLE, 0) * total;
      const unsigned long long hit = __ballot(part > 0.0 && incl > r);
      const unsigned long long nz = __ballot(part > 0.0);
      const int owner = hit ? __builtin_ctzll(hit) : (nz ? 63 - __builtin_clzll(nz) : 0);   // rounding slack -> last mass
      uint32_t idx = 0;
      if ((int)lane == owner && lo < N) {
        double run = excl;
        int found = -1, last = -1;
        for (uint32_t k = 0; k < C; ++k) {
          const double pk = norm2(st[lo + k]);
          run += pk;
          if (pk > 0.0) {
            last = (int)k;
            if (found < 0 && run > r) found = (int)k;
          }
        }
        idx = lo + (uint32_t)(found >= 0 ? found : (last >= 0 ? last : 0));
      }
      idx = __shfl(idx, owner, 64);
      uint64_t word = nz_word(idx, lane, meas, pool, seed, t);
      if constexpr (MEAS) word |= mword;
      if (lane == 0) out[t] = word;
    }
    __syncthreads();                                               // wave 0 is done reading before the next |0..0>
  }
}

template <int TPB, int KRAUS, bool MEAS = false>
static hipError_t launch_noisy(const NzLaunch& l, unsigned* grid) {
  const size_t lds = (size_t)16 << l.W;
  hipError_t e = hipFuncSetAttribute((const void*)k_noisy<TPB, KRAUS, MEAS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  int per_cu = 0;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_noisy<TPB, KRAUS, MEAS>), TPB, lds);
  if (e != hipSuccess) return e;
  uint64_t g = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(l.n_cu > 0 ? l.n_cu : 1);
  if (l.max_grid > 0 && (uint64_t)l.max_grid < g) g = (uint64_t)l.max_grid;
  if (l.shots < g) g = l.shots;
  *grid = (unsigned)g;
  hipLaunchKernelGGL((k_noisy<TPB, KRAUS, MEAS>), dim3((unsigned)g), dim3(TPB), lds, l.stream, l.d_ops, l.n_ops, l.d_pool, l.W, l.shots,
                     l.seed, l.meas, l.d_out);
  return hipGetLastError();
}
