// qsv_noise_dynamic.hip -- the trajectory kernels that know IF and RESET records (QSV_OP_IF, QSV_OP_RESET, include/qsv.h: a guard
// over the next records on the shot's classical word, and a reset of one qubit), for both paths and for
// qsv_noisy_sample_accept: the shot loops of qsv_noise_lds_shots.inc and qsv_noise_hbm_shots.inc with DYN = true, in a
// translation unit -- and so a code object -- of their own, as qsv_noise_kraus2.hip is.  The host comes here only when the
// re-encoded stream holds an NZ_IF or NZ_RESET record, or when the diagnostic option noisy_dynamic_kernels sends every stream
// here; every other program runs the kernels of the five other units, whose code objects hold what they held before the kinds
// existed.  One instantiation per shape, the one that knows every record kind (the KRAUS2 instantiation of the width with
// DYN); what a RESET record does is nz_apply / kraus_op of qsv_noise_ops.h, an IF record is taken by the shot loops.
#include "qsv_noise_kernel.h"
#include "qsv_noise_hbm_kernel.h"

template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy_dyn(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                   int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                                   uint64_t* __restrict__ out) {
  constexpr bool MEAS = true, ACC = false, K2 = true, DYN = true;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_lds_shots.inc"
}

template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy_dyn_accept(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                          int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                                          uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = true, DYN = true;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_lds_shots.inc"
}

template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm_dyn(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                       int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                       uint64_t* __restrict__ out) {
  constexpr bool MEAS = true, ACC = false, K2 = true, DYN = true;
  constexpr uint64_t first = 0, fix_val = 0;
#include "qsv_noise_hbm_shots.inc"
}

template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm_dyn_accept(const NzOp* __restrict__ ops, int n_ops,
                                                              const double* __restrict__ pool, int W, uint64_t shots, uint64_t seed,
                                                              NzMeas meas, char* slots, uint64_t* __restrict__ out, NzAccept a) {
  constexpr bool MEAS = true, ACC = true, K2 = true, DYN = true;
  const uint64_t first = a.first_shot, fix_val = a.fix_val;
#include "qsv_noise_hbm_shots.inc"
}

// the instantiation of the width, as qsv_noise_launch_kraus2 picks it; the caller has checked W and shots
hipError_t qsv_noise_launch_dynamic(const NzLaunch& l, unsigned* grid) {
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return nz_lds_launch(k_noisy_dyn<64, 1>, 64, l, grid);
  return l.W <= QSV_NZ_WAVE_MAXW ? nz_lds_launch(k_noisy_dyn<64, 8>, 64, l, grid) : nz_lds_launch(k_noisy_dyn<256, 1>, 256, l, grid);
}

hipError_t qsv_noise_launch_accept_dynamic(const NzLaunch& l, const NzAccept& a, unsigned* grid) {
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return nz_lds_launch(k_noisy_dyn_accept<64, 1>, 64, l, grid, a);
  return l.W <= QSV_NZ_WAVE_MAXW ? nz_lds_launch(k_noisy_dyn_accept<64, 8>, 64, l, grid, a)
                                 : nz_lds_launch(k_noisy_dyn_accept<256, 1>, 256, l, grid, a);
}

// the launches of qsv_noise_hbm_launch and qsv_noise_hbm_launch_accept, whose checks have passed
hipError_t qsv_noise_hbm_launch_dynamic(const NzHbmLaunch& l) {
  hipLaunchKernelGGL((k_noisy_hbm_dyn<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops, l.d_pool,
                     l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out);
  return hipGetLastError();
}

hipError_t qsv_noise_hbm_launch_accept_dynamic(const NzHbmLaunch& l, const NzAccept& a) {
  hipLaunchKernelGGL((k_noisy_hbm_dyn_accept<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops,
                     l.d_pool, l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out, a);
  return hipGetLastError();
}
