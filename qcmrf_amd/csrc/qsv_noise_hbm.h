// qsv_noise_hbm.h -- noisy shots whose trajectories live in device memory (qsv_noisy_sample_hbm): the wide record of the
// compact op stream and the launcher.  Shared by qsv_noise_hbm.hip (kernel) and qsv.hip (entry point in qsv_exec.inc).
// The record kinds (NZ_*), the Philox draws, NzMeas and the meaning of every field are those of qsv_noise.h.
#pragma once
#include "qsv_noise.h"

#define QSV_NZ_HBM_MAXW 24        // 2^24 complex128 = 256 MiB per trajectory; index arithmetic stays in 32 bits
#define QSV_NZ_HBM_TPB 256

// One op of the compact stream for qubits < 256 and masks of 32 bits, 32 bytes like NzOp.
struct NzWideOp {
  uint8_t kind;        // NZ_*
  uint8_t target;      // 1Q, MCX, KRAUS
  uint8_t n;           // DIAG, PAULI: number of qubits in ql; KRAUS: number of operators (1..4)
  uint8_t pad;
  uint32_t cmask;      // control qubits (1Q, MCX, MCPHASE: all its qubits); NZ_INIT: the uniform mask
  uint32_t cval;       // values the control bits must have
  uint32_t off;        // into the pool (doubles), tables as NzOp::off
  uint64_t ql[2];      // DIAG, PAULI: qubit b in bits [8 (b & 7), 8 (b & 7) + 8) of ql[b >> 3]
};
static_assert(sizeof(NzWideOp) == 32, "NzWideOp is 32 bytes");

__host__ __device__ __forceinline__ uint32_t nz_wide_qubit(const NzWideOp& o, uint32_t b) {
  return (uint32_t)(((b < 8u ? o.ql[0] : o.ql[1]) >> (8u * (b & 7u))) & 255u);
}

struct NzHbmLaunch {
  hipStream_t stream;
  int W;
  unsigned grid;            // workgroups = slots; the caller sized `slots` for it
  const NzWideOp* d_ops;    // device copies
  int n_ops;
  const double* d_pool;
  uint64_t shots, seed;
  NzMeas meas;
  char* d_slots;            // grid x (16 << W) bytes: workgroup b owns [b (16 << W), (b + 1) (16 << W))
  uint64_t* d_out;
};

// workgroups of the trajectory kernel the chip holds at once (occupancy API x n_cu), at least 1
hipError_t qsv_noise_hbm_resident(int n_cu, uint64_t* workgroups);
// launches the trajectory kernel on l.stream (asynchronous)
hipError_t qsv_noise_hbm_launch(const NzHbmLaunch& l);
