// qsv_noise_hbm_kernel.h -- the slot-path trajectory kernel template (included by qsv_noise_hbm.hip, which instantiates
// the kernel without the MEASURE kind, MEAS = false, and by qsv_noise_measure.hip, which instantiates the one with it).
#pragma once
#include "qsv_noise_hbm.h"
#include "qsv_noise_ops.h"

#define QSV_NZ_HBM_B 4             // loads of a thread in flight in every op loop (amps, pairs, kraus_op)

template <int TPB, bool MEAS>
__global__ __launch_bounds__(TPB) void k_noisy_hbm(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                   int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                   uint64_t* __restrict__ out) {
  static_assert(TPB % 64 == 0 && TPB >= 64, "whole waves");
  constexpr int NW = TPB / 64;
  __shared__ double fd_wsum[NW];
  __shared__ unsigned long long fd_hit[NW], fd_nz[NW];
  __shared__ double fd_excl;
  cplx* st = reinterpret_cast<cplx*>(slots + (uint64_t)blockIdx.x * ((uint64_t)16 << W));   // 64-bit byte offset
  const uint32_t N = 1u << W;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint64_t t = blockIdx.x; t < shots; t += gridDim.x) {
    for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    __syncthreads();
    uint32_t draw = 0;
    uint64_t mword = 0;                                            // the bits MEASURE records wrote (MEAS only)
    for (int k = 0; k < n_ops; ++k) {
      const NzOp o = nz_fetch(ops, k);
      nz_apply<TPB, QSV_NZ_HBM_B, 1, MEAS>(st, N, o, pool, tid, seed, t, draw, mword);
    }
    // One basis state from |amp|^2, the whole workgroup: thread t owns the contiguous chunk [t C, (t + 1) C).  The chunk
    // sums are scanned inside each wave, the waves' totals cross through LDS and are added in wave order.
    const uint32_t C = N >= (uint32_t)TPB ? N / (uint32_t)TPB : 1u;
    const uint32_t clo = tid * C;
    double part = 0.0;
    if (clo < N) {
#pragma unroll 8
      for (uint32_t k = 0; k < C; ++k) part += norm2(st[clo + k]);                 // added in index order
    }
    const double incl_w = wave_scan(part, lane);
    double excl_w = __shfl_up(incl_w, 1, 64);
    if (lane == 0) excl_w = 0.0;
    if (lane == 63) fd_wsum[wave] = incl_w;
    __syncthreads();
    double before = 0.0, total = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == (int)wave) before = total;
      total += fd_wsum[w];
    }
    const double r = philox_u01(seed, t, NZ_STREAM_SAMPLE, 0) * total;
    {
      const unsigned long long hit = __ballot(part > 0.0 && before + incl_w > r);
      const unsigned long long nz = __ballot(part > 0.0);
      if (lane == 0) { fd_hit[wave] = hit; fd_nz[wave] = nz; }
    }
    __syncthreads();
    int owner = -1, lastnz = -1;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const unsigned long long hit = fd_hit[w], nz = fd_nz[w];
      if (owner < 0 && hit) owner = 64 * w + __builtin_ctzll(hit);
      if (nz) lastnz = 64 * w + 63 - __builtin_clzll(nz);
    }
    if (owner < 0) owner = lastnz >= 0 ? lastnz : 0;               // rounding slack -> the last chunk with mass
    if ((int)tid == owner) fd_excl = before + excl_w;
    __syncthreads();
    // Wave 0 locates the amplitude inside the owner's chunk: the chunk is cut into 64 contiguous pieces, one per lane,
    // scanned as the chunks were, and the piece that holds r is cut again until a piece is one amplitude.  No serial walk
    // longer than a 64th of a chunk (2^10 amplitudes at W = 24).
    if (tid < 64) {
      uint32_t lo = (uint32_t)owner * C, len = C;
      double base = fd_excl;
      while (len > 1u) {
        const uint32_t sub = len >= 64u ? len >> 6 : 1u, pieces = len / sub;
        double p = 0.0;
        if (lane < pieces) {
#pragma unroll 8
          for (uint32_t k = 0; k < sub; ++k) p += norm2(st[lo + lane * sub + k]);
        }
        const double inc = wave_scan(p, lane);
        double exc = __shfl_up(inc, 1, 64);
        if (lane == 0) exc = 0.0;
        const unsigned long long hit = __ballot(p > 0.0 && base + inc > r);
        const unsigned long long nz = __ballot(p > 0.0);
        const int piece = hit ? __builtin_ctzll(hit) : (nz ? 63 - __builtin_clzll(nz) : 0);
        base += __shfl(exc, piece, 64);
        lo += (uint32_t)piece * sub;
        len = sub;
      }
      const uint32_t idx = lo < N ? lo : 0u;
      uint64_t word = nz_word(idx, lane, meas, pool, seed, t);
      if constexpr (MEAS) word |= mword;
      if (lane == 0) out[t] = word;
    }
    __syncthreads();                                               // wave 0 is done reading before the next |0..0>
  }
}
