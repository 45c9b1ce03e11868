// qsv_noise_accept.hip -- the trajectory kernels of qsv_noisy_sample_accept (include/qsv.h: noisy shots kept only when
// fixed bits of their word read given values), for both paths: the shot loops of qsv_noise_kernel.h and
// qsv_noise_hbm_kernel.h with ACC = true, in a translation unit -- and so a code object -- of their own, as
// qsv_noise_measure.hip is: the code objects of qsv_noise.hip, qsv_noise_hbm.hip and qsv_noise_measure.hip hold the kernels
// they held before.  An accept-aware kernel runs the shots first_shot + [0, shots) of qsv_noisy_sample with the same draws
// and, for a shot it runs to its end, the same word; a shot whose word contradicts fix_val behind a decisive MEASURE record
// (NZ_DECISIVE, set by nz_encode) ends there.  Which shots are kept is decided on the host by the predicate alone.
//
// One instantiation per shape, the one that knows every record kind (the Kraus instantiation of the width with the MEASURE
// kind): a call that fixes bits which only the final draw writes has nothing to abandon and runs these kernels as a plain
// call would run its own, at the registers of the Kraus instantiation.
#include "qsv_noise_kernel.h"
#include "qsv_noise_hbm_kernel.h"

hipError_t qsv_noise_launch_accept(const NzLaunch& l, const NzAccept& a, unsigned* grid) {
  *grid = 0;
  if (l.W < 1 || l.W > QSV_NZ_MAXW) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.dynamic) return qsv_noise_launch_accept_dynamic(l, a, grid); // kernels of their own (qsv_noise_dynamic.hip)
  if (l.kraus2) return qsv_noise_launch_accept_kraus2(l, a, grid);  // kernels of their own (qsv_noise_kraus2.hip)
  if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return nz_lds_launch(k_noisy_accept<64, 1>, 64, l, grid, a);
  return l.W <= QSV_NZ_WAVE_MAXW ? nz_lds_launch(k_noisy_accept<64, 8>, 64, l, grid, a) : nz_lds_launch(k_noisy_accept<256, 1>, 256, l, grid, a);
}

hipError_t qsv_noise_hbm_launch_accept(const NzHbmLaunch& l, const NzAccept& a) {
  if (l.W < 1 || l.W > QSV_NZ_HBM_MAXW || !l.d_slots) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.grid < 1 || (uint64_t)l.grid > l.shots) return hipErrorInvalidValue;
  if (l.dynamic) return qsv_noise_hbm_launch_accept_dynamic(l, a);  // a kernel of its own (qsv_noise_dynamic.hip)
  if (l.kraus2) return qsv_noise_hbm_launch_accept_kraus2(l, a);   // a kernel of its own (qsv_noise_kraus2.hip)
  hipLaunchKernelGGL((k_noisy_hbm_accept<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops,
                     l.d_pool, l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out, a);
  return hipGetLastError();
}
