// qsv_noise_hbm_kernel.h -- the slot-path trajectory kernel template (included by qsv_noise_hbm.hip, which instantiates
// the kernel without the MEASURE kind, MEAS = false, by qsv_noise_measure.hip, which instantiates the one with it, and by
// qsv_noise_accept.hip, which instantiates the accept-aware k_noisy_hbm_accept).  The body of both is qsv_noise_hbm_shots.inc.
#pragma once
#include "qsv_noise_hbm.h"
#include "qsv_noise_ops.h"

#define QSV_NZ_HBM_B 4             // loads of a thread in flight in every op loop (amps, pairs, kraus_op)

template <int TPB, bool MEAS>
__global__ __launch_bounds__(TPB) void k_noisy_hbm(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                   int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                   uint64_t* __restrict__ out) {
  constexpr bool ACC = false, K2 = false, DYN = false;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_hbm_shots.inc"
}

// k_noisy_hbm<TPB, true> over the shots a.first_shot + [0, shots), abandoning at decisive records
template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm_accept(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                          int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                          uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = false, DYN = false;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_hbm_shots.inc"
}
