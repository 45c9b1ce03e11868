// qsv_noise.h -- noisy shots as per-shot trajectories (qsv_noisy_sample): the compact op stream the kernel walks
// and its launcher.  Shared by qsv_noise.hip and qsv_noise_hbm.hip (kernels; what a record does is in qsv_noise_ops.h) and
// qsv.hip (entry points, re-encoding of qsv_op records).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QSV_NZ_MAXW 13            // 2^13 complex128 = 128 KiB of LDS per trajectory
#define QSV_NZ_WAVE_MAXW 10       // up to here one wavefront per trajectory (no workgroup barriers)
#define QSV_NZ_KRAUS_1PAIR_MAXW 7 // up to here a lane owns at most one pair of a Kraus op's target (2^6 pairs, 64 lanes)

enum { NZ_INIT = 0, NZ_1Q, NZ_MCX, NZ_DIAG, NZ_MCPHASE, NZ_PAULI, NZ_KRAUS, NZ_MEASURE, NZ_KRAUS2, NZ_IF, NZ_RESET };

// One op of the compact stream, 32 bytes: every trajectory reads the whole list, so a record is a quarter of an
// L2 line instead of the 168 bytes of a qsv_op.  Both paths read this record: qubits < 256, masks of 32 bits (the slot path
// goes to 24 qubits; the 13 of the LDS path fit as well).  What a trajectory waits for at every op is the scalar fetch of
// the record, so everything but a diagonal over more than 8 qubits sits in the first 16 bytes, one s_load_dwordx4
// (nz_fetch): DIAG and PAULI have no controls, and their first 8 listed qubits take the place of cmask and cval.
struct NzOp {
  uint32_t kind : 8;   // NZ_*.  Bit fields of one word: the record's first 16 bytes have no hole and load as one piece
  uint32_t target : 8; // 1Q, MCX, KRAUS, MEASURE; KRAUS2: its qubit 0 (matrix index bit 0)
  uint32_t n : 16;     // DIAG, PAULI: number of listed qubits; KRAUS: number of operators (1..4); KRAUS2: the same (1..16)
  uint32_t cmask;      // control qubits (1Q, MCX, MCPHASE: all its qubits); NZ_INIT: the uniform mask.  DIAG, PAULI: listed
  uint32_t cval;       // qubits 0..3 / values the control bits must have.  DIAG, PAULI: listed qubits 4..7, 8 bits each
                       // MEASURE: cmask = classical bit | release << 8 | decisive << 9 (NZ_DECISIVE, set for
                       // qsv_noisy_sample_accept only), cval = the record's ordinal among the MEASURE records
                       // KRAUS2: cmask = its qubit 1 (matrix index bit 1)
                       // RESET: a MEASURE record that writes no bit: cmask = release << 8 (always set), cval = the record's
                       // ordinal among the MEASURE and RESET records; off is not read
                       // IF: target = negate, cmask = span, (cval, off) = the low and high half of the 64-bit mask -- span
                       // and mask, what the branch waits for, in the first 16 bytes --, ql8 = the 64-bit value
  uint32_t off;        // into the pool (doubles): 1Q 8 = m00 m01 m10 m11; DIAG 2^n complex; MCPHASE (cos, sin);
                       // INIT the amplitude value; PAULI 4^n cumulative probabilities; KRAUS n x 8 = the K_k as 1Q, then
                       // n x 4 = (E00, E11, Re E01, Im E01) of E_k = K_k^dg K_k; MEASURE 2 = P(flip | 0), P(flip | 1);
                       // KRAUS2 n x 32 = the K_k (4 x 4, row-major, re / im), then n x 16 = the packed E_k of QSV_OP_KRAUS2
  uint64_t ql8;        // DIAG: listed qubit b = 8..15 in bits [8 (b - 8), 8 (b - 8) + 8); IF: the value compared
  uint64_t pad2;
};
static_assert(sizeof(NzOp) == 32, "NzOp is 32 bytes");

// A MEASURE record is decisive when it is the last record to write a classical bit that the call fixes (fix_mask of
// qsv_noisy_sample_accept): the bit it leaves in the shot's word is final, so a shot in which it contradicts fix_val can be
// abandoned there.  Only the accept-aware kernels (qsv_noise_accept.hip) read the flag, and only their calls set it.
#define NZ_DECISIVE (1u << 9)

// listed qubit b of a DIAG or PAULI record
__host__ __device__ __forceinline__ uint32_t nz_qubit(const NzOp& o, uint32_t b) {
  const uint32_t w = b < 4u ? o.cmask : b < 8u ? o.cval : (uint32_t)(o.ql8 >> (b < 12u ? 0 : 32));
  return (w >> (8u * (b & 3u))) & 255u;
}

// Philox-4x32-10 streams (counter word 1): every random number is a pure function of (seed, shot, stream, draw)
enum { NZ_STREAM_PAULI = 0, NZ_STREAM_SAMPLE = 1, NZ_STREAM_READOUT = 2, NZ_STREAM_MEASURE = 3 };

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

// what every launch of a trajectory kernel takes
struct NzCall {
  hipStream_t stream;
  int W;
  const NzOp* d_ops;        // device copies
  int n_ops;
  const double* d_pool;
  uint64_t shots, seed;
  NzMeas meas;
  uint64_t* d_out;
  bool measure;             // the stream holds an NZ_MEASURE op: a kernel instantiation that knows the kind is launched
  bool kraus2;              // the stream holds an NZ_KRAUS2 op: the kernels of qsv_noise_kraus2.hip, which know every kind
  bool dynamic;             // the stream holds an NZ_IF or NZ_RESET op (or the option noisy_dynamic_kernels is set): the kernels
                            // of qsv_noise_dynamic.hip, which know those two besides every other kind
};

// what an accept-aware launch takes besides: it runs the shots first_shot + [0, shots) and writes shot first_shot + i to
// d_out[i]; a shot whose word contradicts fix_val at a decisive record ends there (its word as it stands is stored)
struct NzAccept {
  uint64_t first_shot, fix_mask, fix_val;
};

struct NzLaunch : NzCall {
  int n_cu;
  int max_grid;             // 0: as many workgroups as the chip holds at once
  bool kraus;               // the stream holds an NZ_KRAUS op: a kernel instantiation that knows the kind is launched
};

// launches the trajectory kernel on l.stream (asynchronous); the workgroup count used goes to *grid
hipError_t qsv_noise_launch(const NzLaunch& l, unsigned* grid);
// the same for a stream that holds an NZ_MEASURE op (qsv_noise_measure.hip); qsv_noise_launch comes here by itself
hipError_t qsv_noise_launch_measure(const NzLaunch& l, unsigned* grid);
// the accept-aware kernels (qsv_noise_accept.hip), for any stream without an NZ_KRAUS2 op; l.measure and l.kraus are not looked
// at, and a stream with l.kraus2 goes on to qsv_noise_launch_accept_kraus2
hipError_t qsv_noise_launch_accept(const NzLaunch& l, const NzAccept& a, unsigned* grid);
// the same two for a stream that holds an NZ_KRAUS2 op (qsv_noise_kraus2.hip); the launchers above come here by themselves
hipError_t qsv_noise_launch_kraus2(const NzLaunch& l, unsigned* grid);
hipError_t qsv_noise_launch_accept_kraus2(const NzLaunch& l, const NzAccept& a, unsigned* grid);
// the same two for a stream with l.dynamic (qsv_noise_dynamic.hip); qsv_noise_launch and qsv_noise_launch_accept come here by
// themselves, before they look at l.kraus2
hipError_t qsv_noise_launch_dynamic(const NzLaunch& l, unsigned* grid);
hipError_t qsv_noise_launch_accept_dynamic(const NzLaunch& l, const NzAccept& a, unsigned* grid);
