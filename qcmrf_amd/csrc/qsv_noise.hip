// qsv_noise.hip -- noisy shots as per-shot trajectories (qsv_noisy_sample; host side in qsv_exec.inc).
//
// A shot of a Pauli-noise program is its own random trajectory of a small state: W <= 13 qubits, 2^W complex128
// amplitudes = at most 128 KiB, which lives in the LDS of one workgroup for the whole trajectory.  Workgroups are
// persistent: workgroup b runs shots b, b + grid, b + 2 grid, ...  Per shot:
//   |0..0> -> every op of the compact stream (one workgroup barrier after each op that changes the state) ->
//   one basis state drawn from |amp|^2 by a scan over the LDS state against its actual mass ->
//   measured bits mapped as k_remap_bits does, each flipped with its readout probability -> out[shot].
// W <= 10: one wavefront per workgroup (16 KiB of LDS at most), so the "barriers" compile to LDS waits only.
// W 11..13: 256 threads share one trajectory.
//
// What a record does to the state is qsv_noise_ops.h (nz_apply, here with one load of a thread in flight: LDS needs no more),
// shared with the slot path of qsv_noise_hbm.hip.  A Kraus op (NZ_KRAUS) is the one op whose branch depends on the state
// (kraus_op there).  Only k_noisy<TPB, KRAUS > 0> knows the kind; the host launches one of those when the stream holds such
// an op, so every other program runs k_noisy<TPB, 0>, the kernel without the kind.  A mid-circuit measurement (NZ_MEASURE) is
// built on the same op and follows the same rule: k_noisy<TPB, KRAUS > 0, true> (instantiated in qsv_noise_measure.hip) runs only
// when the stream holds one.  The kernel template is in qsv_noise_kernel.h; this file instantiates it with MEAS = false.
//
// Random numbers: Philox-4x32-10 keyed by the 64-bit seed, counter (draw, stream, shot lo, shot hi).  Every lane of a
// workgroup computes the same draw (the branch on the drawn Pauli is uniform), and a shot's draws depend on nothing
// but (seed, shot, stream, draw): not on the grid, the thread count or how many shots the call has.
#include "qsv_noise_kernel.h"

hipError_t qsv_noise_launch(const NzLaunch& l, unsigned* grid) {
  *grid = 0;
  if (l.W < 1 || l.W > QSV_NZ_MAXW) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.dynamic) return qsv_noise_launch_dynamic(l, grid);         // kernels of their own (qsv_noise_dynamic.hip)
  if (l.kraus2) return qsv_noise_launch_kraus2(l, grid);           // kernels of their own (qsv_noise_kraus2.hip)
  if (l.measure) return qsv_noise_launch_measure(l, grid);         // kernels of their own (qsv_noise_measure.hip)
  if (l.kraus) {
    if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return launch_noisy<64, 1>(l, grid);
    return l.W <= QSV_NZ_WAVE_MAXW ? launch_noisy<64, 8>(l, grid) : launch_noisy<256, 1>(l, grid);
  }
  return l.W <= QSV_NZ_WAVE_MAXW ? launch_noisy<64, 0>(l, grid) : launch_noisy<256, 0>(l, grid);
}
