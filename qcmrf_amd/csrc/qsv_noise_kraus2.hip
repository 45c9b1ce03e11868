// qsv_noise_kraus2.hip -- the trajectory kernels that know KRAUS2 records (QSV_OP_KRAUS2, include/qsv.h: a general two-qubit
// Kraus channel), for both paths and for qsv_noisy_sample_accept: the shot loops of qsv_noise_lds_shots.inc and
// qsv_noise_hbm_shots.inc with K2 = true, in a translation unit -- and so a code object -- of their own, as qsv_noise_measure.hip
// and qsv_noise_accept.hip are.  The host comes here only when the re-encoded stream holds a KRAUS2 record; every other program
// runs the kernels of qsv_noise.hip, qsv_noise_hbm.hip, qsv_noise_measure.hip and qsv_noise_accept.hip, whose code objects hold
// what they held before the kind existed.  One instantiation per shape, the one that knows every record kind (the Kraus
// instantiation of the width with the MEASURE kind); what the record does is nz_apply / kraus2_op of qsv_noise_ops.h.
#include "qsv_noise_kernel.h"
#include "qsv_noise_hbm_kernel.h"

template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy_k2(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                  int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                                  uint64_t* __restrict__ out) {
  constexpr bool MEAS = true, ACC = false, K2 = true, DYN = false;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_lds_shots.inc"
}

template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy_k2_accept(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                         int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                                         uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = true, DYN = false;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_lds_shots.inc"
}

template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm_k2(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                      int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                      uint64_t* __restrict__ out) {
  constexpr bool MEAS = true, ACC = false, K2 = true, DYN = false;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_hbm_shots.inc"
}

template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm_k2_accept(const NzOp* __restrict__ ops, int n_ops,
                                                             const double* __restrict__ pool, int W, uint64_t shots, uint64_t seed,
                                                             NzMeas meas, char* slots, uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = true, DYN = false;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_hbm_shots.inc"
}

// the instantiation of the width, as qsv_noise_launch_measure picks it; the caller has checked W and shots
hipError_t qsv_noise_launch_kraus2(const NzLaunch& l, unsigned* grid) {
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return nz_lds_launch(k_noisy_k2<64, 1>, 64, l, grid);
  return l.W <= QSV_NZ_WAVE_MAXW ? nz_lds_launch(k_noisy_k2<64, 8>, 64, l, grid) : nz_lds_launch(k_noisy_k2<256, 1>, 256, l, grid);
}

hipError_t qsv_noise_launch_accept_kraus2(const NzLaunch& l, const NzAccept& a, unsigned* grid) {
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return nz_lds_launch(k_noisy_k2_accept<64, 1>, 64, l, grid, a);
  return l.W <= QSV_NZ_WAVE_MAXW ? nz_lds_launch(k_noisy_k2_accept<64, 8>, 64, l, grid, a)
                                 : nz_lds_launch(k_noisy_k2_accept<256, 1>, 256, l, grid, a);
}

// the launches of qsv_noise_hbm_launch and qsv_noise_hbm_launch_accept, whose checks have passed
hipError_t qsv_noise_hbm_launch_kraus2(const NzHbmLaunch& l) {
  hipLaunchKernelGGL((k_noisy_hbm_k2<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops, l.d_pool,
                     l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out);
  return hipGetLastError();
}

hipError_t qsv_noise_hbm_launch_accept_kraus2(const NzHbmLaunch& l, const NzAccept& a) {
  hipLaunchKernelGGL((k_noisy_hbm_k2_accept<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops,
                     l.d_pool, l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out, a);
  return hipGetLastError();
}
