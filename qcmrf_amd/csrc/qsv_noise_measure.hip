// qsv_noise_measure.hip -- the trajectory kernels that know MEASURE records (QSV_OP_MEASURE, include/qsv.h: a mid-circuit
// measurement taken in place), for both paths: the kernel templates of qsv_noise_kernel.h and qsv_noise_hbm_kernel.h with
// MEAS = true, in a translation unit -- and so a code object -- of their own.  The host comes here only when the re-encoded
// stream holds a MEASURE record; a program without one runs the kernels of qsv_noise.hip and qsv_noise_hbm.hip, whose code
// objects hold what they held before the kind existed.  What the record does is nz_apply / kraus_op / measure_pick of
// qsv_noise_ops.h; KRAUS > 0 always, because the op is built on kraus_op.
#include "qsv_noise_kernel.h"
#include "qsv_noise_hbm_kernel.h"

// the Kraus instantiation of the width (qsv_noise_launch), with the MEASURE kind
hipError_t qsv_noise_launch_measure(const NzLaunch& l, unsigned* grid) {
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return launch_noisy<64, 1, true>(l, grid);
  return l.W <= QSV_NZ_WAVE_MAXW ? launch_noisy<64, 8, true>(l, grid) : launch_noisy<256, 1, true>(l, grid);
}

// the launch of qsv_noise_hbm_launch, whose checks have passed
hipError_t qsv_noise_hbm_launch_measure(const NzHbmLaunch& l) {
  hipLaunchKernelGGL((k_noisy_hbm<QSV_NZ_HBM_TPB, true>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops,
                     l.d_pool, l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out);
  return hipGetLastError();
}
