// qsv_noise_hbm.hip -- noisy shots as per-shot trajectories resident in device memory (qsv_noisy_sample_hbm; host side in
// qsv_exec.inc).
//
// The contract is that of qsv_noise.hip -- the same record stream, the same Philox draws, the same words -- for W <= 24
// qubits: a trajectory's 2^W complex128 amplitudes live in a slot of 16 << W bytes of device memory instead of LDS.
// Workgroups are persistent: workgroup b owns slot b and runs shots b, b + grid, b + 2 grid, ... in it.  A trajectory
// never leaves its workgroup: every access to a slot is a plain 16-byte load or store by the workgroup that owns it, ops
// are separated by a workgroup barrier (which orders the workgroup's global accesses at workgroup scope: its waves share
// one CU), and nothing is handed from one workgroup to another inside the launch -- no flags, no atomics, no cooperative
// launch.  A slot is written (|0..0>) by its workgroup before that workgroup reads it.
//
// Per shot: |0..0> -> every op of the stream, i = tid + k TPB over amplitudes or pair numbers so that a wave touches
// contiguous runs -> one basis state drawn from |amp|^2 by the whole workgroup -> measured bits, readout flips, out[shot].
// The order of every addition depends on W and TPB only, never on the grid or the number of shots.
#include "qsv_noise_hbm.h"
#include "qsv_common.h"

// amplitude times i^ny, negated if neg
__device__ __forceinline__ cplx hbm_pauli_phase(cplx a, uint32_t ny, bool neg) {
  cplx r = a;
  switch (ny & 3u) {
    case 1: r = make_double2(-a.y, a.x); break;
    case 2: r = make_double2(-a.x, -a.y); break;
    case 3: r = make_double2(a.y, -a.x); break;
    default: break;
  }
  return neg ? make_double2(-r.x, -r.y) : r;
}

__device__ __forceinline__ double norm2(cplx a) { return fma(a.x, a.x, a.y * a.y); }

// The loops of k_noisy over a slot, QSV_NZ_HBM_B iterations of a thread at a time with every load issued before the first
// store: a workgroup alone has few loads in flight, and the compiler may not move a load of st above a store to st.
// amps: st[i] = f(i, st[i]) for the i = tid + k TPB < N with pred(i).
// pairs: (st[i], st[i ^ xm]) = f(i, i ^ xm, st[i], st[i ^ xm]) for pair number p = tid + k TPB < half with pred(i),
//        i = p with a zero inserted at the lowest bit of xm.
#define QSV_NZ_HBM_B 4
template <int TPB, class P, class F>
__device__ __forceinline__ void amps(cplx* st, uint32_t N, uint32_t tid, P pred, F f) {
  for (uint32_t i0 = tid; i0 < N; i0 += QSV_NZ_HBM_B * TPB) {
    cplx a[QSV_NZ_HBM_B];
    bool on[QSV_NZ_HBM_B];
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j) {
      const uint32_t i = i0 + (uint32_t)j * TPB;
      on[j] = i < N && pred(i);
      if (on[j]) a[j] = st[i];
    }
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j) {
      const uint32_t i = i0 + (uint32_t)j * TPB;
      if (on[j]) st[i] = f(i, a[j]);
    }
  }
}
template <int TPB, class P, class F>
__device__ __forceinline__ void pairs(cplx* st, uint32_t half, uint32_t xm, uint32_t tid, P pred, F f) {
  const uint32_t lo = (xm & (0u - xm)) - 1u;
  for (uint32_t p0 = tid; p0 < half; p0 += QSV_NZ_HBM_B * TPB) {
    cplx a[QSV_NZ_HBM_B], b[QSV_NZ_HBM_B];
    uint32_t i[QSV_NZ_HBM_B];
    bool on[QSV_NZ_HBM_B];
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j) {
      const uint32_t p = p0 + (uint32_t)j * TPB;
      i[j] = ((p & ~lo) << 1) | (p & lo);
      on[j] = p < half && pred(i[j]);
      if (on[j]) { a[j] = st[i[j]]; b[j] = st[i[j] ^ xm]; }
    }
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j)
      if (on[j]) {
        cplx na, nb;
        f(i[j], i[j] ^ xm, a[j], b[j], na, nb);
        st[i[j]] = na;
        st[i[j] ^ xm] = nb;
      }
  }
}

// One Kraus channel on one trajectory (contract: include/qsv.h, QSV_OP_KRAUS), the TPB = 256 scheme of qsv_noise.hip: every
// thread sums its pairs in index order, the xor butterfly leaves every lane of a wave with the same bits, the waves' sums
// cross through static LDS and every thread adds them in one order; then the pairs are read again and K_k sqrt(total / w_k)
// applied.  The caller's barrier after the op also fences the LDS scratch.
template <int TPB>
__device__ __forceinline__ void kraus_hbm(cplx* st, const NzWideOp& o, const double* __restrict__ pool, uint32_t half,
                                          uint32_t tid, double u) {
  constexpr int NW = TPB / 64;
  const uint32_t tb = 1u << o.target, lo = tb - 1u;
  double r00 = 0.0, r11 = 0.0, rre = 0.0, rim = 0.0;               // r10 = sum a1 conj(a0) = rre + i rim
  for (uint32_t p0 = tid; p0 < half; p0 += QSV_NZ_HBM_B * TPB) {   // loads of a batch first, its sums in index order (pairs past the end are zeros)
    cplx b0[QSV_NZ_HBM_B], b1[QSV_NZ_HBM_B];
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j) {
      const uint32_t p = p0 + (uint32_t)j * TPB;
      const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
      b0[j] = b1[j] = make_double2(0.0, 0.0);
      if (p < half) { b0[j] = st[i0]; b1[j] = st[i0 | tb]; }
    }
#pragma unroll
    for (int j = 0; j < QSV_NZ_HBM_B; ++j) {
      r00 += fma(b0[j].x, b0[j].x, b0[j].y * b0[j].y);
      r11 += fma(b1[j].x, b1[j].x, b1[j].y * b1[j].y);
      rre += fma(b1[j].x, b0[j].x, b1[j].y * b0[j].y);
      rim += fma(b1[j].y, b0[j].x, -(b1[j].x * b0[j].y));
    }
  }
  r00 = wave_sum(r00);
  r11 = wave_sum(r11);
  rre = wave_sum(rre);
  rim = wave_sum(rim);
  __shared__ double part[NW][4];
  if ((tid & 63u) == 0) {
    double* mine = part[tid >> 6];
    mine[0] = r00; mine[1] = r11; mine[2] = rre; mine[3] = rim;
  }
  __syncthreads();
  r00 = part[0][0]; r11 = part[0][1]; rre = part[0][2]; rim = part[0][3];
#pragma unroll
  for (int w = 1; w < NW; ++w) { r00 += part[w][0]; r11 += part[w][1]; rre += part[w][2]; rim += part[w][3]; }
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
  pick = __builtin_amdgcn_readfirstlane(pick);                     // every lane holds the same k: the loads go scalar
  const double s = sqrt(total / wk);
  const double* m = K + 8 * pick;
  const cplx m00 = make_double2(m[0] * s, m[1] * s), m01 = make_double2(m[2] * s, m[3] * s);
  const cplx m10 = make_double2(m[4] * s, m[5] * s), m11 = make_double2(m[6] * s, m[7] * s);
  pairs<TPB>(st, half, tb, tid, [](uint32_t) { return true; },
             [&](uint32_t, uint32_t, cplx b0, cplx b1, cplx& n0, cplx& n1) {
               n0 = cmad(m00, b0, cmul(m01, b1));
               n1 = cmad(m10, b0, cmul(m11, b1));
             });
}

// inclusive scan over the 64 lanes of a wave, lane 0 first
__device__ __forceinline__ double wave_scan(double v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double x = __shfl_up(v, o, 64);
    if ((int)lane >= o) v += x;
  }
  return v;
}

template <int TPB>
__global__ __launch_bounds__(TPB) void k_noisy_hbm(const NzWideOp* __restrict__ ops, int n_ops, const double* __restrict__ pool,
                                                   int W, uint64_t shots, uint64_t seed, NzMeas meas, char* slots,
                                                   uint64_t* __restrict__ out) {
  static_assert(TPB % 64 == 0 && TPB >= 64, "whole waves");
  constexpr int NW = TPB / 64;
  __shared__ double fd_wsum[NW];
  __shared__ unsigned long long fd_hit[NW], fd_nz[NW];
  __shared__ double fd_excl;
  cplx* st = reinterpret_cast<cplx*>(slots + (uint64_t)blockIdx.x * ((uint64_t)16 << W));   // 64-bit byte offset
  const uint32_t N = 1u << W, half = N >> 1;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint64_t t = blockIdx.x; t < shots; t += gridDim.x) {
    for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    __syncthreads();
    uint32_t draw = 0;
    for (int k = 0; k < n_ops; ++k) {
      const NzWideOp o = ops[k];
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
          const uint32_t cmask = o.cmask, cval = o.cval;
          pairs<TPB>(st, half, 1u << o.target, tid, [=](uint32_t i0) { return (i0 & cmask) == cval; },
                     [&](uint32_t, uint32_t, cplx a0, cplx a1, cplx& n0, cplx& n1) {
                       n0 = cmad(m00, a0, cmul(m01, a1));
                       n1 = cmad(m10, a0, cmul(m11, a1));
                     });
          break;
        }
        case NZ_MCX: {
          const uint32_t cmask = o.cmask, cval = o.cval;
          pairs<TPB>(st, half, 1u << o.target, tid, [=](uint32_t i0) { return (i0 & cmask) == cval; },
                     [](uint32_t, uint32_t, cplx a0, cplx a1, cplx& n0, cplx& n1) { n0 = a1; n1 = a0; });
          break;
        }
        case NZ_DIAG: {
          const cplx* tab = reinterpret_cast<const cplx*>(pool + o.off);   // even offset: 16-byte aligned
          if (o.n == 1) {
            const cplx t0 = tab[0], t1 = tab[1];
            const uint32_t q = nz_wide_qubit(o, 0);
            amps<TPB>(st, N, tid, [](uint32_t) { return true; },
                      [=](uint32_t i, cplx a) { return cmul(a, ((i >> q) & 1u) ? t1 : t0); });
          } else {
            const uint64_t q0 = o.ql[0], q1 = o.ql[1];
            const uint32_t n = o.n;
            amps<TPB>(st, N, tid, [](uint32_t) { return true; }, [=](uint32_t i, cplx a) {
              uint32_t j = 0;
              for (uint32_t b = 0; b < n; ++b) j |= ((i >> (uint32_t)(((b < 8u ? q0 : q1) >> (8u * (b & 7u))) & 255u)) & 1u) << b;
              return cmul(a, tab[j]);
            });
          }
          break;
        }
        case NZ_MCPHASE: {
          const cplx ph = make_double2(pool[o.off], pool[o.off + 1]);
          const uint32_t cmask = o.cmask, cval = o.cval;
          amps<TPB>(st, N, tid, [=](uint32_t i) { return (i & cmask) == cval; }, [=](uint32_t, cplx a) { return cmul(a, ph); });
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
            const uint32_t q = nz_wide_qubit(o, j);
            const uint32_t x = (p >> (2u * j)) & 1u, z = (p >> (2u * j + 1u)) & 1u;
            xm |= x << q;
            zm |= z << q;
            ny += x & z;
          }
          if (xm == 0) {                                           // Z-type: a sign per amplitude
            amps<TPB>(st, N, tid, [=](uint32_t i) { return (__popc(i & zm) & 1) != 0; },
                      [](uint32_t, cplx a) { return make_double2(-a.x, -a.y); });
          } else {                                                 // amplitude i -> i ^ xm, times (-1)^|i & zm| i^ny
            pairs<TPB>(st, half, xm, tid, [](uint32_t) { return true; },
                       [=](uint32_t i, uint32_t j, cplx a, cplx b, cplx& ni, cplx& nj) {
                         nj = hbm_pauli_phase(a, ny, __popc(i & zm) & 1);
                         ni = hbm_pauli_phase(b, ny, __popc(j & zm) & 1);
                       });
          }
          break;
        }
        case NZ_KRAUS: {
          kraus_hbm<TPB>(st, o, pool, half, tid, philox_u01(seed, t, NZ_STREAM_PAULI, draw++));
          break;
        }
        default: break;
      }
      __syncthreads();
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

hipError_t qsv_noise_hbm_resident(int n_cu, uint64_t* workgroups) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_noisy_hbm<QSV_NZ_HBM_TPB>), QSV_NZ_HBM_TPB, 0);
  if (e != hipSuccess) return e;
  *workgroups = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(n_cu > 0 ? n_cu : 1);
  return hipSuccess;
}

hipError_t qsv_noise_hbm_launch(const NzHbmLaunch& l) {
  if (l.W < 1 || l.W > QSV_NZ_HBM_MAXW || !l.d_slots) return hipErrorInvalidValue;
  if (l.shots == 0) return hipSuccess;
  if (l.grid < 1 || (uint64_t)l.grid > l.shots) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_noisy_hbm<QSV_NZ_HBM_TPB>), dim3(l.grid), dim3(QSV_NZ_HBM_TPB), 0, l.stream, l.d_ops, l.n_ops, l.d_pool,
                     l.W, l.shots, l.seed, l.meas, l.d_slots, l.d_out);
  return hipGetLastError();
}
