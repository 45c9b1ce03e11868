// qsv_noise_hbm.hip -- noisy shots as per-shot trajectories resident in device memory (qsv_noisy_sample_hbm; host side in
// qsv_exec.inc).
//
// The contract is that of qsv_noise.hip -- the same record stream, the same Philox draws, the same words -- for W <= 24
// qubits: a trajectory's 2^W complex128 amplitudes live in a slot of 16 << W bytes of device memory instead of LDS.
// Workgroups are persistent: workgroup b owns slot b and runs shots b, b + grid, b + 2 grid, ... in it.  A trajectory
// never leaves its workgroup: every access to a slot is a plain 16-byte load or store by the workgroup that owns it, ops
// are separated by a workgroup barrier (which orders the workgroup's global accesses at workgroup scope: its waves share
// one CU), and nothing is handed from one workgroup to another inside the launch -- no flags, no atomics, no cooperative
// launch.  A slot is written (|0..0>) by its workgroup before that workgroup reads it.
//
// Per shot: |0..0> -> every op of the stream (nz_apply of qsv_noise_ops.h, the interpreter of both paths, here with four
// loads of a thread in flight), i = tid + k TPB over amplitudes or pair numbers so that a wave touches contiguous runs ->
// one basis state drawn from |amp|^2 by the whole workgroup -> measured bits, readout flips, out[shot].
// The order of every addition depends on W and TPB only, never on the grid or the number of shots.
// The kernel template is in qsv_noise_hbm_kernel.h; this file instantiates it without the MEASURE kind (MEAS = false), and
// qsv_noise_measure.hip with it, for the programs that hold a mid-circuit measurement.
#include "qsv_noise_hbm_kernel.h"

hipError_t qsv_noise_hbm_resident(int n_cu, uint64_t* workgroups) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_noisy_hbm<QSV_NZ_HBM_TPB, false>), QSV_NZ_HBM_TPB, 0);
  if (e != hipSuccess) return e;
  *workgroups = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(n_cu > 0 ? n_cu : 1);
  return hipSuccess;
}

hipError_t qsv_noise_hbm_launch(const NzHbmLaunch& l) {
  if (l.W < 1 || l.W > QSV_NZ_HBM_MAXW || !l.d_slots) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.grid < 1 || (uint64_t)l.grid > l.shots) return hipErrorInvalidValue;
  if (l.dynamic) return qsv_noise_hbm_launch_dynamic(l);          // a kernel of its own (qsv_noise_dynamic.hip)
  if (l.kraus2) return qsv_noise_hbm_launch_kraus2(l);            // a kernel of its own (qsv_noise_kraus2.hip)
  if (l.measure) return qsv_noise_hbm_launch_measure(l);          // a kernel of its own (qsv_noise_measure.hip)
  hipLaunchKernelGGL((k_noisy_hbm<QSV_NZ_HBM_TPB, false>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops, l.d_pool,
                     l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out);
  return hipGetLastError();
}
