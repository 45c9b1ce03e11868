// qsv_branch.hip -- the device side of the level-wise trajectory walk (qsv_branch_mass, qsv_branch_split; host side in
// qsv_branch.inc, the walk in qcmrf_amd/trajectory.py).
//
// The live branches of one level of the outcome tree sit side by side as the slots of one wide state: slot b is the
// aligned block of 2^w amplitudes from b << w.  One qsv_exec applies a segment to all of them (gates on qubits < w do not
// see the slot number); the two kernels here are what is left per level:
//
//   k_branch_mass   one read pass: per slot the two sums of |amp|^2 by the value of the measured bit.  No atomics.
//   k_branch_split  one gather pass: the next level's slots, each a parent slot projected on an outcome.
//
// Order contract of the sums.  The pair of a slot is a pure function of (w, qubit, the slot's contents): not of the number
// of slots, the slot's position, the width of the state or the grid.  The additions form one fixed tree:
//   - a wave reads an aligned run of 2^10 amplitudes, lane l the amplitudes l, l + 64, ..., l + 960 of the run.  Runs and
//     slots are both aligned, so a run lies inside one slot (w >= 10) or is made of whole slots (w < 10), and where a run
//     starts inside its slot does not depend on where the slot is;
//   - a lane adds the values of ITS amplitudes of one slot in index order (16 of them for w >= 10, 2^(w-6) for
//     6 <= w < 10, one for w < 6), those with the measured bit 0 into one sum and those with 1 into the other (the other
//     sum gets + 0.0, which is exact);
//   - the lanes that share a slot are folded by an xor butterfly over the offsets min(32, 2^(w-1)), ..., 2, 1;
//   - w > 10: the 2^(w-10) run sums of a slot are folded by k_branch_fold: thread t of T adds the run sums t, t + T, ... in
//     that order, the T threads are folded by the butterfly (and, T = 256, the four waves in wave order).  T depends on w
//     alone (64 below QSV_BR_FOLD_WG_W, 256 from it).
// Which wave of which workgroup takes a run is free, and so is the grid.
#include "qsv_branch.h"
#include "qsv_common.h"
#include <algorithm>

#define BR_RUN (1u << QSV_BR_RUN_LOG2)
#define BR_LOADS (BR_RUN / 64u)                 // loads of a lane per run

// GL: log2 of the loads of a lane that fall into one slot (4: the whole run, w >= 10; 0..3: w = 6..9; 0 also for w < 6,
// where a slot is a group of 2^w lanes of one load)
template <int GL>
__global__ __launch_bounds__(QSV_TPB) void k_branch_mass(const cplx* __restrict__ amp, uint64_t n_amps, int w, int qubit,
                                                         uint64_t n_out, double2* __restrict__ out) {
  constexpr int G = 1 << GL;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_runs = (n_amps + BR_RUN - 1) >> QSV_BR_RUN_LOG2;
  const uint64_t nwaves = (uint64_t)gridDim.x * (QSV_TPB / 64);
  const int top = w < 6 ? (1 << (w - 1)) : 32;
  const unsigned writer_mask = w < 6 ? (1u << w) - 1u : 63u;
  for (uint64_t run = (uint64_t)blockIdx.x * (QSV_TPB / 64) + (threadIdx.x >> 6); run < n_runs; run += nwaves) {
    const uint64_t base = (run << QSV_BR_RUN_LOG2) + lane;
    double p[BR_LOADS];
#pragma unroll
    for (unsigned j = 0; j < BR_LOADS; ++j) {
      const uint64_t idx = base + 64u * j;
      p[j] = 0.0;
      if (idx < n_amps) {
        const cplx a = ld(amp + idx);
        p[j] = fma(a.x, a.x, a.y * a.y);
      }
    }
#pragma unroll
    for (unsigned j0 = 0; j0 < BR_LOADS; j0 += G) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (unsigned j = j0; j < j0 + G; ++j) {
        const bool one = ((base + 64u * j) >> qubit) & 1ull;
        s0 += one ? 0.0 : p[j];
        s1 += one ? p[j] : 0.0;
      }
      for (int o = top; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
      }
      if ((lane & writer_mask) == 0u) {
        const uint64_t o = GL == 4 ? run : (base + 64u * j0) >> w;      // w >= 10: one pair per run; else per slot
        if (o < n_out) out[o] = make_double2(s0, s1);
      }
    }
  }
}

// the 2^mlog run sums of every slot -> the slot's pair.  WG: one workgroup per slot, else one wave per slot.
template <bool WG>
__global__ __launch_bounds__(QSV_TPB) void k_branch_fold(const double2* __restrict__ part, int mlog, uint64_t n_slots,
                                                         double2* __restrict__ out) {
  const uint64_t m = 1ull << mlog;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (!WG) {
    const uint64_t stride = (uint64_t)gridDim.x * (QSV_TPB / 64);
    for (uint64_t b = (uint64_t)blockIdx.x * (QSV_TPB / 64) + wave; b < n_slots; b += stride) {
      double s0 = 0.0, s1 = 0.0;
      for (uint64_t i = lane; i < m; i += 64) {
        const double2 v = part[(b << mlog) + i];
        s0 += v.x;
        s1 += v.y;
      }
      s0 = wave_sum(s0);
      s1 = wave_sum(s1);
      if (lane == 0) out[b] = make_double2(s0, s1);
    }
  } else {
    __shared__ double2 sh[QSV_TPB / 64];
    for (uint64_t b = blockIdx.x; b < n_slots; b += gridDim.x) {      // (n_slots is uniform: every thread meets every barrier)
      double s0 = 0.0, s1 = 0.0;
      for (uint64_t i = threadIdx.x; i < m; i += QSV_TPB) {
        const double2 v = part[(b << mlog) + i];
        s0 += v.x;
        s1 += v.y;
      }
      s0 = wave_sum(s0);
      s1 = wave_sum(s1);
      if (lane == 0) sh[wave] = make_double2(s0, s1);
      __syncthreads();
      if (threadIdx.x == 0) {
        double2 t = sh[0];
        for (unsigned k = 1; k < QSV_TPB / 64; ++k) { t.x += sh[k].x; t.y += sh[k].y; }
        out[b] = t;
      }
      __syncthreads();
    }
  }
}

// A workgroup writes 4096 consecutive amplitudes of dst, thread t the amplitudes t, t + 256, ...: a wave stores contiguous
// 1 KiB runs in slot order, and reads the kept half of the parent slot in runs as long as the measured bit allows.  All
// loads of a thread are issued before its first store.
#define BR_SPLIT_PER 16u
__global__ __launch_bounds__(QSV_TPB) void k_branch_split(cplx* __restrict__ dst, uint64_t n_dst, const cplx* __restrict__ src,
                                                          int w, uint64_t n_children, const uint32_t* __restrict__ parent,
                                                          const uint8_t* __restrict__ outcome, int qubit, int release) {
  const uint64_t smask = (1ull << w) - 1ull;
  const uint64_t n_tiles = (n_dst + QSV_TPB * BR_SPLIT_PER - 1) / (QSV_TPB * BR_SPLIT_PER);
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * (QSV_TPB * BR_SPLIT_PER) + threadIdx.x;
    cplx v[BR_SPLIT_PER];
#pragma unroll
    for (unsigned j = 0; j < BR_SPLIT_PER; ++j) {
      const uint64_t g = base + (uint64_t)QSV_TPB * j;
      const uint64_t c = g >> w;
      v[j] = make_double2(0.0, 0.0);
      if (g < n_dst && c < n_children) {
        const uint64_t i = g & smask;
        const uint64_t o = outcome[c];
        const uint64_t keep = release ? 0ull : o;            // the value of the measured bit at which dst holds the kept half
        if (((i >> qubit) & 1ull) == keep) v[j] = ld(src + ((((uint64_t)parent[c]) << w) | (i ^ ((keep ^ o) << qubit))));
      }
    }
#pragma unroll
    for (unsigned j = 0; j < BR_SPLIT_PER; ++j) {
      const uint64_t g = base + (uint64_t)QSV_TPB * j;
      if (g < n_dst) st(dst + g, v[j]);
    }
  }
}

static unsigned br_grid(uint64_t need) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>(need, 1), (1ull << 24) - 1ull);   // gridDim.x * blockDim.x < 2^32; every kernel here strides
}

hipError_t qsv_branch_mass_launch(hipStream_t stream, const double2* amp, int w, uint64_t n_slots, int qubit,
                                  double* d_part, double* d_out, int* launches) {
  const uint64_t n_amps = n_slots << w;
  const uint64_t n_runs = (n_amps + BR_RUN - 1) >> QSV_BR_RUN_LOG2;
  const bool fold = w > QSV_BR_RUN_LOG2;
  double2* out = reinterpret_cast<double2*>(fold ? d_part : d_out);
  const uint64_t n_out = fold ? n_runs : n_slots;
  const dim3 grid(br_grid((n_runs + QSV_TPB / 64 - 1) / (QSV_TPB / 64))), block(QSV_TPB);
#define BR_MASS(GL) hipLaunchKernelGGL((k_branch_mass<GL>), grid, block, 0, stream, amp, n_amps, w, qubit, n_out, out)
  switch (w >= QSV_BR_RUN_LOG2 ? 4 : (w > 6 ? w - 6 : 0)) {
    case 0: BR_MASS(0); break;
    case 1: BR_MASS(1); break;
    case 2: BR_MASS(2); break;
    case 3: BR_MASS(3); break;
    default: BR_MASS(4); break;
  }
#undef BR_MASS
  *launches = 1;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !fold) return e;
  const int mlog = w - QSV_BR_RUN_LOG2;
  if (w >= QSV_BR_FOLD_WG_W)
    hipLaunchKernelGGL((k_branch_fold<true>), dim3(br_grid(n_slots)), block, 0, stream, reinterpret_cast<const double2*>(d_part), mlog, n_slots, reinterpret_cast<double2*>(d_out));
  else
    hipLaunchKernelGGL((k_branch_fold<false>), dim3(br_grid((n_slots + QSV_TPB / 64 - 1) / (QSV_TPB / 64))), block, 0, stream, reinterpret_cast<const double2*>(d_part), mlog, n_slots, reinterpret_cast<double2*>(d_out));
  *launches = 2;
  return hipGetLastError();
}

hipError_t qsv_branch_split_launch(hipStream_t stream, double2* dst, uint64_t n_dst, const double2* src, int w,
                                   uint64_t n_children, const uint32_t* d_parent, const uint8_t* d_outcome, int qubit,
                                   int release) {
  const uint64_t n_tiles = (n_dst + QSV_TPB * BR_SPLIT_PER - 1) / (QSV_TPB * BR_SPLIT_PER);
  hipLaunchKernelGGL(k_branch_split, dim3(br_grid(n_tiles)), dim3(QSV_TPB), 0, stream, dst, n_dst, src, w, n_children,
                     d_parent, d_outcome, qubit, release);
  return hipGetLastError();
}
