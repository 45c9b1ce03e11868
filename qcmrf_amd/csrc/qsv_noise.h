// qsv_noise.h -- noisy shots as per-shot trajectories (qsv_noisy_sample): the compact op stream the kernel walks
// and its launcher.  Shared by qsv_noise.hip (kernel) and qsv.hip (entry point, re-encoding of qsv_op records).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QSV_NZ_MAXW 13            // 2^13 complex128 = 128 KiB of LDS per trajectory
#define QSV_NZ_WAVE_MAXW 10       // up to here one wavefront per trajectory (no workgroup barriers)
#define QSV_NZ_KRAUS_1PAIR_MAXW 7 // up to here a lane owns at most one pair of a Kraus op's target (2^6 pairs, 64 lanes)

enum { NZ_INIT = 0, NZ_1Q, NZ_MCX, NZ_DIAG, NZ_MCPHASE, NZ_PAULI, NZ_KRAUS };

// One op of the compact stream, 32 bytes: every trajectory reads the whole list, so a record is a quarter of an
// L2 line instead of the 168 bytes of a qsv_op.  Qubits < 16, so masks are 16 bits.
struct NzOp {
  uint16_t kind;       // NZ_*
  uint16_t target;     // 1Q, MCX, KRAUS
  uint16_t cmask;      // control qubits (1Q, MCX, MCPHASE: all its qubits); NZ_INIT: the uniform mask
  uint16_t cval;       // values the control bits must have
  uint32_t off;        // into the pool (doubles): 1Q 8 = m00 m01 m10 m11; DIAG 2^n complex; MCPHASE (cos, sin);
                       // INIT the amplitude value; PAULI 4^n cumulative probabilities; KRAUS n x 8 = the K_k as 1Q, then
                       // n x 4 = (E00, E11, Re E01, Im E01) of E_k = K_k^dg K_k
  uint32_t n;          // DIAG, PAULI: number of qubits in qlist; KRAUS: number of operators (1..4)
  uint64_t qlist;      // DIAG, PAULI: qubit b in bits [4b, 4b + 4)
  uint64_t pad;
};
static_assert(sizeof(NzOp) == 32, "NzOp is 32 bytes");

// Philox-4x32-10 streams (counter word 1): every random number is a pure function of (seed, shot, stream, draw)
enum { NZ_STREAM_PAULI = 0, NZ_STREAM_SAMPLE = 1, NZ_STREAM_READOUT = 2 };

// the draw itself, in [0, 1): 53 bits of counter (draw, stream, shot lo, shot hi) under the 64-bit seed
__device__ __forceinline__ double philox_u01(uint64_t seed, uint64_t shot, uint32_t stream, uint32_t draw) {
  uint32_t c0 = draw, c1 = stream, c2 = (uint32_t)shot, c3 = (uint32_t)(shot >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  return (double)((((uint64_t)c0 << 32) | c1) >> 11) * 0x1.0p-53;      // 53 bits: [0, 1)
}

struct NzMeas {
  int n;                    // measured bits (<= 64); < 0: out = the full basis index
  int readout;              // pool offset of n x 2 flip probabilities, < 0: none
  const int* pos;           // device: bit j <- qubit pos[j] (< 0: stays 0), n entries
};

struct NzLaunch {
  hipStream_t stream;
  int W;
  int n_cu;
  int max_grid;             // 0: as many workgroups as the chip holds at once
  const NzOp* d_ops;        // device copies
  int n_ops;
  bool kraus;               // the stream holds an NZ_KRAUS op: a kernel instantiation that knows the kind is launched
  const double* d_pool;
  uint64_t shots, seed;
  NzMeas meas;
  uint64_t* d_out;
};

// launches the trajectory kernel on l.stream (asynchronous); the workgroup count used goes to *grid
hipError_t qsv_noise_launch(const NzLaunch& l, unsigned* grid);
