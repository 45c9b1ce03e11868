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
// an op, so every other program runs k_noisy<TPB, 0>, the kernel without the kind.
//
// Random numbers: Philox-4x32-10 keyed by the 64-bit seed, counter (draw, stream, shot lo, shot hi).  Every lane of a
// workgroup computes the same draw (the branch on the drawn Pauli is uniform), and a shot's draws depend on nothing
// but (seed, shot, stream, draw): not on the grid, the thread count or how many shots the call has.
#include "qsv_noise_ops.h"

template <int TPB, int KRAUS>
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
    for (int k = 0; k < n_ops; ++k) {
      const NzOp o = nz_fetch(ops, k);
      nz_apply<TPB, 1, KRAUS>(st, N, o, pool, tid, seed, t, draw);
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
      const uint64_t word = nz_word(idx, lane, meas, pool, seed, t);
      if (lane == 0) out[t] = word;
    }
    __syncthreads();                                               // wave 0 is done reading before the next |0..0>
  }
}

template <int TPB, int KRAUS>
static hipError_t launch_noisy(const NzLaunch& l, unsigned* grid) {
  const size_t lds = (size_t)16 << l.W;
  hipError_t e = hipFuncSetAttribute((const void*)k_noisy<TPB, KRAUS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  int per_cu = 0;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_noisy<TPB, KRAUS>), TPB, lds);
  if (e != hipSuccess) return e;
  uint64_t g = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(l.n_cu > 0 ? l.n_cu : 1);
  if (l.max_grid > 0 && (uint64_t)l.max_grid < g) g = (uint64_t)l.max_grid;
  if (l.shots < g) g = l.shots;
  *grid = (unsigned)g;
  hipLaunchKernelGGL((k_noisy<TPB, KRAUS>), dim3((unsigned)g), dim3(TPB), lds, l.stream, l.d_ops, l.n_ops, l.d_pool, l.W, l.shots,
                     l.seed, l.meas, l.d_out);
  return hipGetLastError();
}

hipError_t qsv_noise_launch(const NzLaunch& l, unsigned* grid) {
  *grid = 0;
  if (l.W < 1 || l.W > QSV_NZ_MAXW) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.kraus) {
    if (l.W <= QSV_NZ_KRAUS_1PAIR_MAXW) return launch_noisy<64, 1>(l, grid);
    return l.W <= QSV_NZ_WAVE_MAXW ? launch_noisy<64, 8>(l, grid) : launch_noisy<256, 1>(l, grid);
  }
  return l.W <= QSV_NZ_WAVE_MAXW ? launch_noisy<64, 0>(l, grid) : launch_noisy<256, 0>(l, grid);
}
