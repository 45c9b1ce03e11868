// qsv_branch.h -- the two device primitives of the level-wise trajectory walk (qsv_branch_mass, qsv_branch_split): launchers
// shared by qsv_branch.hip (kernels) and qsv.hip (entry points in qsv_branch.inc).
//
// A slot is an aligned block of 2^w amplitudes of one shard; slot b starts at amplitude b << w.  Every index is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QSV_BR_RUN_LOG2 10        // a wave reads aligned runs of 2^10 amplitudes (16 KiB): 16 loads of 16 bytes per lane
#define QSV_BR_FOLD_WG_W 23       // from this slot width a whole workgroup folds a slot's run sums, below it one wave

// doubles of scratch qsv_branch_mass_launch needs behind d_out (one pair per run; 0 for w <= QSV_BR_RUN_LOG2)
static inline uint64_t qsv_branch_mass_scratch(int w, uint64_t n_slots) {
  return w > QSV_BR_RUN_LOG2 ? 2ull * (n_slots << (w - QSV_BR_RUN_LOG2)) : 0ull;
}

// d_out[2 b + v] = sum |amp|^2 over slot b < n_slots with bit `qubit` == v; d_part: qsv_branch_mass_scratch doubles.
// One or two launches on `stream` (asynchronous); *launches says how many.
hipError_t qsv_branch_mass_launch(hipStream_t stream, const double2* amp, int w, uint64_t n_slots, int qubit,
                                  double* d_part, double* d_out, int* launches);

// dst[0, n_dst): slot c < n_children <- slot parent[c] of src projected on bit `qubit` == outcome[c] (release != 0: an
// outcome 1 lands on bit 0), every other amplitude zero.  The tables are device pointers.  One launch on `stream`.
hipError_t qsv_branch_split_launch(hipStream_t stream, double2* dst, uint64_t n_dst, const double2* src, int w,
                                   uint64_t n_children, const uint32_t* d_parent, const uint8_t* d_outcome, int qubit,
                                   int release);
