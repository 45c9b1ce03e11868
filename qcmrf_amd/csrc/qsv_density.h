// qsv_density.h -- density-matrix method (qsv_density_*): launchers of the channel, diagonal and sampling kernels.
// Shared by qsv_density.hip (kernels) and qsv.hip (entry points in qsv_density.inc).
//
// A density matrix of W qubits is the vector of a 2W-qubit handle: amplitude v = i | (j << W) holds rho[i, j] (ket bits
// low, bra bits high).  A channel on n error qubits acts inside blocks of 4^n amplitudes: those that differ only in the
// ket and bra bits of the error qubits.  One thread owns whole blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qsv_noise.h"

// Block bit k <-> address bit pos[k]: k < n the ket bit of error qubit k, k >= n the bra bit of error qubit k - n.
// ins[] holds the same 2n positions ascending (zero bits inserted into the block number in that order).
struct DmPos {
  int ins[4];
  int pos[4];
};
// c[x * 2^n + d] = sum_z p(x, z) (-1)^(z . d): out[v] = sum_x c[x][d(v)] in[v ^ m_x], d = ket xor bra bits of the error qubits
struct DmPauli { double c[16]; };
// S[e][f] (row-major, (re, im)) = sum_k K_k[a][a'] conj(K_k[b][b']), e = a | b << 1, f = a' | b' << 1: B <- sum_k K_k B K_k^dg
struct DmKraus { double s[32]; };

struct DmLaunch {
  hipStream_t stream;
  unsigned grid;            // workgroups of QSV_TPB threads (grid-stride over the blocks)
  double2* amp;
  uint64_t nblocks;         // 4^W / 4^n
  bool nt;                  // non-temporal loads and stores
  DmPos pos;
};

hipError_t qsv_dm_pauli_launch(const DmLaunch& l, int n, const DmPauli& c);
hipError_t qsv_dm_kraus_launch(const DmLaunch& l, const DmKraus& s);
// A MEASURE record with its outcome fixed or forgotten: B' = diag(w0 B00, w1 B11) on every 2 x 2 block over the ket and bra
// bit of the measured qubit (n = 1 in DmPos), release != 0: B' = diag(w0 B00 + w1 B11, 0).  2 loads, 4 stores per block.
hipError_t qsv_dm_measure_launch(const DmLaunch& l, int release, double w0, double w1);
// Below this qubit the ket pair (v, v + 2^t) of a block shares one 128-byte line (8 amplitudes), so the entries k_dm_measure does
// not load come in with their lines anyway: nothing is saved, and two half-used loads per line ran 0.5 to 0.9 times as fast as
// k_dm_kraus (t = 0, 1, 2 at W = 13); from qubit 3 up k_dm_measure is 1.3 to 1.4 times faster (profiles/density_measure.log)
#define QSV_DM_MEASURE_MIN_QUBIT 3
// A KRAUS2 record: d_s = the 16 x 16 superoperator in device memory (512 doubles: too large for kernel arguments),
// S[e][f] (row-major, (re, im)) = sum_k K_k[a][a'] conj(K_k[b][b']), e = a | b << 2, f = a' | b' << 2, with a, b, a', b' the
// two-bit indices of the record's operators (bit j on error qubit j): block bits 0, 1 the ket bits, 2, 3 the bra bits (DmPos)
#define QSV_DM_KRAUS2_DOUBLES 512
hipError_t qsv_dm_kraus2_launch(const DmLaunch& l, const double* d_s);

// out[i] = Re rho[i, i], i < 2^W: one strided read
hipError_t qsv_dm_diag_launch(hipStream_t stream, const double2* amp, int W, double* out);

// One thread per shot: u = Philox (seed, shot, stream 1, draw 0); the first i with cum[i] > u cum[n - 1], none: `last`;
// bits mapped and flipped as the trajectory kernel does (meas.readout: offset into `pool`, < 0 none).
hipError_t qsv_dm_sample_launch(hipStream_t stream, const double* cum, uint64_t n, uint64_t last, uint64_t shots, uint64_t seed,
                                NzMeas meas, const double* pool, uint64_t* out);
