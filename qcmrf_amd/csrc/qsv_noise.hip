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
// A Kraus op (NZ_KRAUS) is the one op whose branch depends on the state: the workgroup reduces the target's reduced density
// matrix over the trajectory, every lane ending with bitwise the same sums, draws one operator, applies it and rescales
// the state to the mass it had (kraus_op).  Only k_noisy<TPB, KRAUS > 0> knows the kind; the host launches one of those
// when the stream holds such an op, so every other program runs k_noisy<TPB, 0>, the kernel as it was without the kind.
//
// Random numbers: Philox-4x32-10 keyed by the 64-bit seed, counter (draw, stream, shot lo, shot hi).  Every lane of a
// workgroup computes the same draw (the branch on the drawn Pauli is uniform), and a shot's draws depend on nothing
// but (seed, shot, stream, draw): not on the grid, the thread count or how many shots the call has.
#include "qsv_noise.h"
#include "qsv_common.h"

// amplitude times i^ny, negated if neg
__device__ __forceinline__ cplx pauli_phase(cplx a, uint32_t ny, bool neg) {
  cplx r = a;
  switch (ny & 3u) {
    case 1: r = make_double2(-a.y, a.x); break;
    case 2: r = make_double2(-a.x, -a.y); break;
    case 3: r = make_double2(a.y, -a.x); break;
    default: break;
  }
  return neg ? make_double2(-r.x, -r.y) : r;
}

// One Kraus channel on one trajectory (the contract is in include/qsv.h, QSV_OP_KRAUS): r = the reduced density matrix
// of the target summed over all pairs, w_k = tr(E_k r), the first k whose cumulative weight exceeds u total, then every
// pair times K_k sqrt(total / w_k).  TPB 64 (W <= 10): a lane owns at most R pairs and keeps them in registers between
// the reduction and the apply, so the op reads and writes the state once, as a 1Q op does.  R = 8 covers W <= 10 and
// costs 112 VGPRs (4 waves per SIMD); R = 1 covers W <= 7 with 67, the 7 waves per SIMD of the kernel without the kind,
// and small trajectories live on having many in flight.  TPB 256 (R unused): 16 pairs per thread would take 128
// registers, so the pairs are read again; the four waves' sums cross through 128 bytes of static LDS and every thread
// adds them in one order.  The caller's barrier after the op also fences that scratch.
template <int TPB, int R>
__device__ __forceinline__ void kraus_op(cplx* st, const NzOp& o, const double* __restrict__ pool, uint32_t half, uint32_t tid,
                                         double u) {
  const uint32_t tb = 1u << o.target, lo = tb - 1u;
  cplx a0[R], a1[R];
  double r00 = 0.0, r11 = 0.0, rre = 0.0, rim = 0.0;               // r10 = sum a1 conj(a0) = rre + i rim
  if constexpr (TPB == 64) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t p = tid + 64u * (uint32_t)j;
      a0[j] = a1[j] = make_double2(0.0, 0.0);
      if (p < half) {
        const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
        a0[j] = st[i0];
        a1[j] = st[i0 | tb];
      }
      r00 += fma(a0[j].x, a0[j].x, a0[j].y * a0[j].y);
      r11 += fma(a1[j].x, a1[j].x, a1[j].y * a1[j].y);
      rre += fma(a1[j].x, a0[j].x, a1[j].y * a0[j].y);
      rim += fma(a1[j].y, a0[j].x, -(a1[j].x * a0[j].y));
    }
  } else {
    for (uint32_t p = tid; p < half; p += TPB) {
      const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
      const cplx b0 = st[i0], b1 = st[i0 | tb];
      r00 += fma(b0.x, b0.x, b0.y * b0.y);
      r11 += fma(b1.x, b1.x, b1.y * b1.y);
      rre += fma(b1.x, b0.x, b1.y * b0.y);
      rim += fma(b1.y, b0.x, -(b1.x * b0.y));
    }
  }
  r00 = wave_sum(r00);                                             // xor butterfly: the partners of a step add the same two
  r11 = wave_sum(r11);                                             // numbers, so all 64 lanes end with the same bits
  rre = wave_sum(rre);
  rim = wave_sum(rim);
  if constexpr (TPB > 64) {
    static_assert(TPB == 256, "four waves cross their sums");
    __shared__ double part[4][4];
    if ((tid & 63u) == 0) {
      double* mine = part[tid >> 6];
      mine[0] = r00; mine[1] = r11; mine[2] = rre; mine[3] = rim;
    }
    __syncthreads();
    r00 = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
    r11 = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
    rre = ((part[0][2] + part[1][2]) + part[2][2]) + part[3][2];
    rim = ((part[0][3] + part[1][3]) + part[2][3]) + part[3][3];
  }
  const double* K = pool + o.off;
  const double* E = K + 8u * o.n;
  const double total = r00 + r11, r = u * total;
  double cum = 0.0, wk = 0.0, wlast = 0.0;
  int pick = -1, last = -1;
  for (uint32_t k = 0; k < o.n; ++k) {
    const double* e = E + 4u * k;
    const double w = e[0] * r00 + e[1] * r11 + 2.0 * (e[2] * rre - e[3] * rim);
    if (w > 0.0) {
      cum += w;
      last = (int)k;
      wlast = w;
      if (pick < 0 && cum > r) { pick = (int)k; wk = w; }
    }
  }
  if (pick < 0) { pick = last; wk = wlast; }                       // rounding at the top boundary: the last k with weight
  if (pick < 0) return;                                            // a state without mass stays as it is
  pick = __builtin_amdgcn_readfirstlane(pick);                     // every lane holds the same k: say so, the loads go scalar
  const double s = sqrt(total / wk);
  const double* m = K + 8 * pick;
  const cplx m00 = make_double2(m[0] * s, m[1] * s), m01 = make_double2(m[2] * s, m[3] * s);
  const cplx m10 = make_double2(m[4] * s, m[5] * s), m11 = make_double2(m[6] * s, m[7] * s);
  if constexpr (TPB == 64) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t p = tid + 64u * (uint32_t)j;
      if (p < half) {
        const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
        st[i0] = cmad(m00, a0[j], cmul(m01, a1[j]));
        st[i0 | tb] = cmad(m10, a0[j], cmul(m11, a1[j]));
      }
    }
  } else {
    for (uint32_t p = tid; p < half; p += TPB) {
      const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
      const cplx b0 = st[i0], b1 = st[i0 | tb];
      st[i0] = cmad(m00, b0, cmul(m01, b1));
      st[i0 | tb] = cmad(m10, b0, cmul(m11, b1));
    }
  }
}

template <int TPB, int KRAUS>
__global__ __launch_bounds__(TPB) void k_noisy(const NzOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                               int W, uint64_t shots, uint64_t seed, NzMeas meas,
                                               uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char nz_lds[];
  cplx* st = reinterpret_cast<cplx*>(nz_lds);              // 2^W amplitudes, nothing else
  const uint32_t N = 1u << W, half = N >> 1;
  const uint32_t tid = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < shots; t += gridDim.x) {
    for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    __syncthreads();
    uint32_t draw = 0;
    for (int k = 0; k < n_ops; ++k) {
      const NzOp o = ops[k];
      switch (o.kind) {
        case NZ_INIT: {
          const double v = pool[o.off];
          const uint32_t keep = o.cmask;
          for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2((i & ~keep) ? 0.0 : v, 0.0);
          break;
        }
        case NZ_1Q: {
          const double* m = pool + o.off;
          const cplx m00 = make_double2(m[0], m[1]), m01 = make_double2(m[2], m[3]);
          const cplx m10 = make_double2(m[4], m[5]), m11 = make_double2(m[6], m[7]);
          const uint32_t tb = 1u << o.target, lo = tb - 1u;
          for (uint32_t p = tid; p < half; p += TPB) {
            const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
            if ((i0 & o.cmask) != o.cval) continue;
            const cplx a0 = st[i0], a1 = st[i0 | tb];
            st[i0] = cmad(m00, a0, cmul(m01, a1));
            st[i0 | tb] = cmad(m10, a0, cmul(m11, a1));
          }
          break;
        }
        case NZ_MCX: {
          const uint32_t tb = 1u << o.target, lo = tb - 1u;
          for (uint32_t p = tid; p < half; p += TPB) {
            const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
            if ((i0 & o.cmask) != o.cval) continue;
            const cplx a0 = st[i0];
            st[i0] = st[i0 | tb];
            st[i0 | tb] = a0;
          }
          break;
        }
        case NZ_DIAG: {
          const cplx* tab = reinterpret_cast<const cplx*>(pool + o.off);   // even offset: 16-byte aligned
          if (o.n == 1) {
            const cplx t0 = tab[0], t1 = tab[1];
            const uint32_t q = (uint32_t)(o.qlist & 15u);
            for (uint32_t i = tid; i < N; i += TPB) st[i] = cmul(st[i], ((i >> q) & 1u) ? t1 : t0);
          } else {
            for (uint32_t i = tid; i < N; i += TPB) {
              uint32_t j = 0;
              for (uint32_t b = 0; b < o.n; ++b) j |= ((i >> ((o.qlist >> (4u * b)) & 15u)) & 1u) << b;
              st[i] = cmul(st[i], tab[j]);
            }
          }
          break;
        }
        case NZ_MCPHASE: {
          const cplx ph = make_double2(pool[o.off], pool[o.off + 1]);
          for (uint32_t i = tid; i < N; i += TPB)
            if ((i & o.cmask) == o.cval) st[i] = cmul(st[i], ph);
          break;
        }
        case NZ_PAULI: {
          const double u = philox_u01(seed, t, NZ_STREAM_PAULI, draw++);
          const double* cum = pool + o.off;
          const uint32_t np = 1u << (2u * o.n);
          uint32_t p = 0;
          while (p + 1u < np && u >= cum[p]) ++p;
          if (p == 0) continue;                                    // identity: the state is unchanged, no barrier
          uint32_t xm = 0, zm = 0, ny = 0;
          for (uint32_t j = 0; j < o.n; ++j) {
            const uint32_t q = (uint32_t)((o.qlist >> (4u * j)) & 15u);
            const uint32_t x = (p >> (2u * j)) & 1u, z = (p >> (2u * j + 1u)) & 1u;
            xm |= x << q;
            zm |= z << q;
            ny += x & z;
          }
          if (xm == 0) {                                           // Z-type: a sign per amplitude
            for (uint32_t i = tid; i < N; i += TPB)
              if (__popc(i & zm) & 1) st[i] = make_double2(-st[i].x, -st[i].y);
          } else {                                                 // amplitude i -> i ^ xm, times (-1)^|i & zm| i^ny
            const uint32_t lb = xm & (0u - xm), lo = lb - 1u;
            for (uint32_t q = tid; q < half; q += TPB) {
              const uint32_t i = ((q & ~lo) << 1) | (q & lo);
              const uint32_t j = i ^ xm;
              const cplx a = st[i], b = st[j];
              st[j] = pauli_phase(a, ny, __popc(i & zm) & 1);
              st[i] = pauli_phase(b, ny, __popc(j & zm) & 1);
            }
          }
          break;
        }
        case NZ_KRAUS: {
          if constexpr (KRAUS > 0) kraus_op<TPB, KRAUS>(st, o, pool, half, tid, philox_u01(seed, t, NZ_STREAM_PAULI, draw++));
          break;
        }
        default: break;
      }
      __syncthreads();
    }
    // one basis state from |amp|^2: wave 0, lane l owns the contiguous chunk [l C, (l + 1) C)
    if (tid < 64) {
      const uint32_t lane = tid;
      const uint32_t C = N >= 64u ? N >> 6 : 1u;
      const uint32_t lo = lane * C;
      double part = 0.0;
      if (lo < N)
        for (uint32_t k = 0; k < C; ++k) { const cplx a = st[lo + k]; part += fma(a.x, a.x, a.y * a.y); }
      double incl = part;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += v;
      }
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
          const cplx a = st[lo + k];
          const double pk = fma(a.x, a.x, a.y * a.y);
          run += pk;
          if (pk > 0.0) {
            last = (int)k;
            if (found < 0 && run > r) found = (int)k;
          }
        }
        idx = lo + (uint32_t)(found >= 0 ? found : (last >= 0 ? last : 0));
      }
      idx = __shfl(idx, owner, 64);
      uint64_t word = idx;
      if (meas.n >= 0) {
        uint32_t bit = 0;
        if ((int)lane < meas.n) {
          const int q = meas.pos[lane];
          if (q >= 0) {
            bit = (idx >> q) & 1u;
            if (meas.readout >= 0 &&
                philox_u01(seed, t, NZ_STREAM_READOUT, lane) < pool[meas.readout + 2 * (int)lane + (int)bit])
              bit ^= 1u;
          }
        }
        word = __ballot(bit != 0u);
      }
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
