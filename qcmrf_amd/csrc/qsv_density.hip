// qsv_density.hip -- density-matrix method: the channel kernels, the diagonal gather and the per-shot search
// (qsv_density_exec / _diagonal / _sample; host side in qsv_density.inc).
//
// rho of W qubits lives in a 2W-qubit shard, rho[i, j] at v = i | (j << W).  Unitary records run as mirrored pairs
// through the engine's own sweeps (qsv_exec); only the two record kinds that are no unitary have kernels here:
//   k_dm_pauli<N>   rho -> sum_p P(p) P rho P^dg on N = 1, 2 error qubits.  P rho P^dg moves rho[i ^ x, j ^ x] to
//                   rho[i, j] with the sign (-1)^(z . (i xor j)); the phases of Y cancel.  Summed over z that is 2^N real
//                   coefficients per element, chosen by d = (i xor j) on the error qubits, and orbits of 2^N elements.
//   k_dm_kraus      rho -> sum_k K_k rho K_k^dg on one qubit: every 2 x 2 block B[a, b] over (i_q, j_q) times the 4 x 4
//                   superoperator S (built once per record on the host).
//   k_dm_kraus2     the same on two qubits: 4 x 4 blocks of 16 amplitudes times the 16 x 16 superoperator, which comes
//                   through device memory.
//   k_dm_measure    an accepted (or forgotten) measurement of one qubit taken in place: of every 2 x 2 block only the two
//                   entries diagonal in the qubit survive, weighted; with RELEASE both land on the |0><0| entry.
// A thread owns whole blocks: the 4^N amplitudes that differ only in the ket and bra bits of the error qubits.  For a low
// error qubit q its loads are adjacent 16-byte pieces of one line (q = 0: v and v + 1); the bra bit q + W is a far stride
// for every W that matters.  Each amplitude is read once and written once: 32 B per amplitude, a pure stream
// (k_dm_measure: two of four read, all four written, 24 B per amplitude).
// Every array index is a compile-time constant after unrolling: no scratch.
#include "qsv_density.h"
#include "qsv_common.h"

template <int NB>
__device__ __forceinline__ uint64_t dm_base(uint64_t t, const DmPos& p) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int b = p.ins[j];
    t = ((t >> b) << (b + 1)) | (t & ((1ull << b) - 1ull));
  }
  return t;
}

template <int NB>
__device__ __forceinline__ uint64_t dm_offset(int e, const DmPos& p) {
  uint64_t o = 0;
#pragma unroll
  for (int k = 0; k < NB; ++k)
    if ((e >> k) & 1) o |= 1ull << p.pos[k];
  return o;
}

template <int N, bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_dm_pauli(cplx* __restrict__ amp, uint64_t nblocks, DmPos p, DmPauli c) {
  constexpr int NB = 2 * N, E = 1 << NB, X = 1 << N;
  uint64_t off[E];
#pragma unroll
  for (int e = 0; e < E; ++e) off[e] = dm_offset<NB>(e, p);
  for (uint64_t t = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; t < nblocks; t += (uint64_t)gridDim.x * QSV_TPB) {
    cplx* b = amp + dm_base<NB>(t, p);
    cplx in[E];
#pragma unroll
    for (int e = 0; e < E; ++e) in[e] = NT ? ld_nt(b + off[e]) : ld(b + off[e]);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int d = (e ^ (e >> N)) & (X - 1);
      double re = c.c[d] * in[e].x, im = c.c[d] * in[e].y;        // x = 0
#pragma unroll
      for (int x = 1; x < X; ++x) {
        const int f = e ^ (x | (x << N));
        re = fma(c.c[x * X + d], in[f].x, re);
        im = fma(c.c[x * X + d], in[f].y, im);
      }
      if (NT) st_nt(b + off[e], make_double2(re, im)); else st(b + off[e], make_double2(re, im));
    }
  }
}

template <bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_dm_kraus(cplx* __restrict__ amp, uint64_t nblocks, DmPos p, DmKraus s) {
  const uint64_t o1 = 1ull << p.pos[0], o2 = 1ull << p.pos[1];
  const uint64_t off[4] = {0, o1, o2, o1 | o2};
  for (uint64_t t = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; t < nblocks; t += (uint64_t)gridDim.x * QSV_TPB) {
    cplx* b = amp + dm_base<2>(t, p);
    cplx in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) in[e] = NT ? ld_nt(b + off[e]) : ld(b + off[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cplx acc = cmul(make_double2(s.s[8 * e], s.s[8 * e + 1]), in[0]);
#pragma unroll
      for (int f = 1; f < 4; ++f) acc = cmad(make_double2(s.s[8 * e + 2 * f], s.s[8 * e + 2 * f + 1]), in[f], acc);
      if (NT) st_nt(b + off[e], acc); else st(b + off[e], acc);
    }
  }
}

// A MEASURE record on qubit t whose outcome is fixed (or forgotten): B = the 2 x 2 block over (ket bit t, bra bit t + W),
// B' = diag(w0 B00, w1 B11), with RELEASE B' = diag(w0 B00 + w1 B11, 0).  The off-diagonal entries are never read and the
// zeros are stored as zeros (not as 0 x input: an inf or nan there must not survive): 2 loads and 4 stores per block.
template <bool NT, bool RELEASE>
__global__ __launch_bounds__(QSV_TPB) void k_dm_measure(cplx* __restrict__ amp, uint64_t nblocks, DmPos p, double w0, double w1) {
  const uint64_t o1 = 1ull << p.pos[0], o2 = 1ull << p.pos[1];
  const cplx zero = make_double2(0.0, 0.0);
  for (uint64_t t = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; t < nblocks; t += (uint64_t)gridDim.x * QSV_TPB) {
    cplx* b = amp + dm_base<2>(t, p);
    const cplx b00 = NT ? ld_nt(b) : ld(b);
    const cplx b11 = NT ? ld_nt(b + (o1 | o2)) : ld(b + (o1 | o2));
    cplx out[4] = {make_double2(w0 * b00.x, w0 * b00.y), zero, zero, make_double2(w1 * b11.x, w1 * b11.y)};
    if (RELEASE) {
      out[0] = make_double2(fma(w1, b11.x, out[0].x), fma(w1, b11.y, out[0].y));
      out[3] = zero;
    }
    const uint64_t off[4] = {0, o1, o2, o1 | o2};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (NT) st_nt(b + off[e], out[e]); else st(b + off[e], out[e]);
    }
  }
}

// rho -> sum_k K_k rho K_k^dg on two qubits: every 4 x 4 block B[a, b] over the ket and bra bits of the two error qubits, 16
// amplitudes, times the 16 x 16 superoperator S.  S is read from device memory at addresses every lane shares (scalar loads
// that stay in the scalar cache: 4 KiB); the 16 amplitudes of a block are all loaded before the first is stored.
template <bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_dm_kraus2(cplx* __restrict__ amp, uint64_t nblocks, DmPos p, const double* __restrict__ S) {
  uint64_t off[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) off[e] = dm_offset<4>(e, p);
  for (uint64_t t = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; t < nblocks; t += (uint64_t)gridDim.x * QSV_TPB) {
    cplx* b = amp + dm_base<4>(t, p);
    cplx in[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) in[e] = NT ? ld_nt(b + off[e]) : ld(b + off[e]);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      cplx acc = cmul(make_double2(S[32 * e], S[32 * e + 1]), in[0]);
#pragma unroll
      for (int f = 1; f < 16; ++f) acc = cmad(make_double2(S[32 * e + 2 * f], S[32 * e + 2 * f + 1]), in[f], acc);
      if (NT) st_nt(b + off[e], acc); else st(b + off[e], acc);
    }
  }
}

__global__ __launch_bounds__(QSV_TPB) void k_dm_diag(const cplx* __restrict__ amp, uint64_t n, int W, double* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * QSV_TPB)
    out[i] = amp[i | (i << W)].x;
}

__global__ __launch_bounds__(QSV_TPB) void k_dm_sample(const double* __restrict__ cum, uint64_t n, uint64_t last, uint64_t shots,
                                                       uint64_t seed, NzMeas meas, const double* __restrict__ pool,
                                                       uint64_t* __restrict__ out) {
  for (uint64_t t = (uint64_t)blockIdx.x * QSV_TPB + threadIdx.x; t < shots; t += (uint64_t)gridDim.x * QSV_TPB) {
    const double r = philox_u01(seed, t, NZ_STREAM_SAMPLE, 0) * cum[n - 1];
    uint64_t lo = 0, hi = n;                                       // first i with cum[i] > r (cum never falls: such an i has P_i > 0)
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (cum[mid] > r) hi = mid; else lo = mid + 1;
    }
    const uint64_t idx = lo < n ? lo : last;                       // rounding at the top boundary: the last i with mass
    uint64_t word = idx;
    if (meas.n >= 0) {
      word = 0;
      for (int j = 0; j < meas.n; ++j) {
        const int q = meas.pos[j];
        if (q < 0) continue;
        uint32_t bit = (uint32_t)(idx >> q) & 1u;
        if (meas.readout >= 0 && philox_u01(seed, t, NZ_STREAM_READOUT, (uint32_t)j) < pool[meas.readout + 2 * j + (int)bit]) bit ^= 1u;
        word |= (uint64_t)bit << j;
      }
    }
    out[t] = word;
  }
}

hipError_t qsv_dm_pauli_launch(const DmLaunch& l, int n, const DmPauli& c) {
  if (n == 1) {
    if (l.nt) hipLaunchKernelGGL((k_dm_pauli<1, true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, c);
    else hipLaunchKernelGGL((k_dm_pauli<1, false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, c);
  } else if (n == 2) {
    if (l.nt) hipLaunchKernelGGL((k_dm_pauli<2, true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, c);
    else hipLaunchKernelGGL((k_dm_pauli<2, false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, c);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t qsv_dm_kraus_launch(const DmLaunch& l, const DmKraus& s) {
  if (l.nt) hipLaunchKernelGGL((k_dm_kraus<true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, s);
  else hipLaunchKernelGGL((k_dm_kraus<false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, s);
  return hipGetLastError();
}

hipError_t qsv_dm_measure_launch(const DmLaunch& l, int release, double w0, double w1) {
  if (release) {
    if (l.nt) hipLaunchKernelGGL((k_dm_measure<true, true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, w0, w1);
    else hipLaunchKernelGGL((k_dm_measure<false, true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, w0, w1);
  } else {
    if (l.nt) hipLaunchKernelGGL((k_dm_measure<true, false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, w0, w1);
    else hipLaunchKernelGGL((k_dm_measure<false, false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, w0, w1);
  }
  return hipGetLastError();
}

hipError_t qsv_dm_kraus2_launch(const DmLaunch& l, const double* d_s) {
  if (!d_s) return hipErrorInvalidValue;
  if (l.nt) hipLaunchKernelGGL((k_dm_kraus2<true>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, d_s);
  else hipLaunchKernelGGL((k_dm_kraus2<false>), dim3(l.grid), dim3(QSV_TPB), 0, l.stream, l.amp, l.nblocks, l.pos, d_s);
  return hipGetLastError();
}

static unsigned dm_small_grid(uint64_t work) {
  const uint64_t g = (work + QSV_TPB - 1) / QSV_TPB;
  return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

hipError_t qsv_dm_diag_launch(hipStream_t stream, const double2* amp, int W, double* out) {
  const uint64_t n = 1ull << W;
  hipLaunchKernelGGL(k_dm_diag, dim3(dm_small_grid(n)), dim3(QSV_TPB), 0, stream, amp, n, W, out);
  return hipGetLastError();
}

hipError_t qsv_dm_sample_launch(hipStream_t stream, const double* cum, uint64_t n, uint64_t last, uint64_t shots, uint64_t seed,
                                NzMeas meas, const double* pool, uint64_t* out) {
  if (shots == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dm_sample, dim3(dm_small_grid(shots)), dim3(QSV_TPB), 0, stream, cum, n, last, shots, seed, meas, pool, out);
  return hipGetLastError();
}
