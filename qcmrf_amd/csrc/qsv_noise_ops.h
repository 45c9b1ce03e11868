// qsv_noise_ops.h -- what one record of the compact stream (NzOp, qsv_noise.h) does to one trajectory: the interpreter of
// both trajectory kernels (device only).  k_noisy (qsv_noise.hip, the state in LDS) runs it with B = 1, k_noisy_hbm
// (qsv_noise_hbm.hip, the state in a slot of device memory) with B = 4 loads of a thread in flight.  The kernels keep what
// depends on where the state lives: the shot loop, the |0..0> write and the final draw.
#pragma once
#include "qsv_noise.h"
#include "qsv_common.h"

// Record k of the stream.  The first 16 bytes come as one scalar load and are what an op waits for; the load of the second
// half (listed qubits 8..15) is issued with it for DIAG, PAULI and KRAUS records, and only a diagonal over more than 8
// qubits waits for it.
__device__ __forceinline__ NzOp nz_fetch(const NzOp* __restrict__ ops, int k) {
  union { uint4 w[2]; NzOp o; } u;
  const uint4* p = reinterpret_cast<const uint4*>(ops + k);
  u.w[0] = p[0];
  u.w[1] = p[1];
  return u.o;
}

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

__device__ __forceinline__ double norm2(cplx a) { return fma(a.x, a.x, a.y * a.y); }

// inclusive scan over the 64 lanes of a wave, lane 0 first
__device__ __forceinline__ double wave_scan(double v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double x = __shfl_up(v, o, 64);
    if ((int)lane >= o) v += x;
  }
  return v;
}

// The loops over a state, B iterations of a thread at a time with every load issued before the first store: a workgroup
// alone has few global loads in flight, and the compiler may not move a load of st above a store to st.  B = 1 is the
// plain loop, written as one: the two phases of a batch would cost an LDS-resident state a second branch per iteration.
// amps: st[i] = f(i, st[i]) for the i = tid + k TPB < N with pred(i).
// pairs: (st[i], st[i ^ xm]) = f(i, i ^ xm, st[i], st[i ^ xm]) for pair number p = tid + k TPB < half with pred(i),
//        i = p with a zero inserted at the lowest bit of xm.
template <int TPB, int B, class P, class F>
__device__ __forceinline__ void amps(cplx* st, uint32_t N, uint32_t tid, P pred, F f) {
  if constexpr (B == 1) {
    for (uint32_t i = tid; i < N; i += TPB)
      if (pred(i)) st[i] = f(i, st[i]);
    return;
  }
  for (uint32_t i0 = tid; i0 < N; i0 += B * TPB) {
    cplx a[B];
    bool on[B];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const uint32_t i = i0 + (uint32_t)j * TPB;
      on[j] = i < N && pred(i);
      if (on[j]) a[j] = st[i];
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const uint32_t i = i0 + (uint32_t)j * TPB;
      if (on[j]) st[i] = f(i, a[j]);
    }
  }
}
template <int TPB, int B, class P, class F>
__device__ __forceinline__ void pairs(cplx* st, uint32_t half, uint32_t xm, uint32_t tid, P pred, F f) {
  const uint32_t lo = (xm & (0u - xm)) - 1u;
  if constexpr (B == 1) {
    for (uint32_t p = tid; p < half; p += TPB) {
      const uint32_t i = ((p & ~lo) << 1) | (p & lo);
      if (!pred(i)) continue;
      cplx na, nb;
      f(i, i ^ xm, st[i], st[i ^ xm], na, nb);
      st[i] = na;
      st[i ^ xm] = nb;
    }
    return;
  }
  for (uint32_t p0 = tid; p0 < half; p0 += B * TPB) {
    cplx a[B], b[B];
    uint32_t i[B];
    bool on[B];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const uint32_t p = p0 + (uint32_t)j * TPB;
      i[j] = ((p & ~lo) << 1) | (p & lo);
      on[j] = p < half && pred(i[j]);
      if (on[j]) { a[j] = st[i[j]]; b[j] = st[i[j] ^ xm]; }
    }
#pragma unroll
    for (int j = 0; j < B; ++j)
      if (on[j]) {
        cplx na, nb;
        f(i[j], i[j] ^ xm, a[j], b[j], na, nb);
        st[i[j]] = na;
        st[i[j] ^ xm] = nb;
      }
  }
}

// a draw u of a PAULI record -> the Pauli index p (0: identity)
__device__ __forceinline__ uint32_t pauli_draw(double u, const NzOp& o, const double* __restrict__ pool) {
  const double* cum = pool + o.off;
  const uint32_t np = 1u << (2u * o.n);
  uint32_t p = 0;
  while (p + 1u < np && u >= cum[p]) ++p;
  return p;
}
// the Pauli index p of a PAULI record -> its x and z masks over the state's qubits and its number of Y
__device__ __forceinline__ void pauli_masks(uint32_t p, const NzOp& o, uint32_t& xm, uint32_t& zm, uint32_t& ny) {
  xm = zm = ny = 0;
  for (uint32_t j = 0; j < o.n; ++j) {
    const uint32_t q = nz_qubit(o, j);
    const uint32_t x = (p >> (2u * j)) & 1u, z = (p >> (2u * j + 1u)) & 1u;
    xm |= x << q;
    zm |= z << q;
    ny += x & z;
  }
}

// The operator of a KRAUS record for the draw u and the target's reduced density matrix (r00, r11, r10 = rre + i rim), which
// every lane holds with the same bits: w_k = tr(E_k r), the first k whose cumulative weight exceeds u total, and
// m = K_k sqrt(total / w_k).  false: the state has no mass and stays as it is.
__device__ __forceinline__ bool kraus_pick(double r00, double r11, double rre, double rim, double u, const NzOp& o,
                                           const double* __restrict__ pool, cplx& m00, cplx& m01, cplx& m10, cplx& m11) {
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
  if (pick < 0) return false;
  pick = __builtin_amdgcn_readfirstlane(pick);                     // every lane holds the same k: say so, the loads go scalar
  const double s = sqrt(total / wk);
  const double* m = K + 8 * pick;
  m00 = make_double2(m[0] * s, m[1] * s); m01 = make_double2(m[2] * s, m[3] * s);
  m10 = make_double2(m[4] * s, m[5] * s); m11 = make_double2(m[6] * s, m[7] * s);
  return true;
}

// The operator of a MEASURE record (the contract is in include/qsv.h, QSV_OP_MEASURE) for the draw u: the Kraus rule with
// K_0 = |0><0|, K_1 = |1><1| (release: |0><1|), so w_0 = r00 and w_1 = r11.  Returns the outcome b and m = K_b sqrt(total / w_b);
// -1: the state has no mass and stays as it is (the recorded outcome is then 0).  Every lane holds the same r00, r11 and u.
__device__ __forceinline__ int measure_pick(double r00, double r11, double u, bool release, cplx& m00, cplx& m01, cplx& m10,
                                            cplx& m11) {
  const double total = r00 + r11, r = u * total;
  int b = (r00 > 0.0 && r00 > r) ? 0 : (r11 > 0.0 ? 1 : 0);
  const double w = b ? r11 : r00;
  if (!(w > 0.0)) return -1;
  b = __builtin_amdgcn_readfirstlane(b);                           // uniform: the selects below are scalar
  const double s = sqrt(total / w);
  m00 = m01 = m10 = m11 = make_double2(0.0, 0.0);
  if (b == 0) m00.x = s;
  else if (release) m01.x = s;                                     // the kept half moves to the 0 half: the slot is back in |0>
  else m11.x = s;
  return b;
}

// One Kraus channel on one trajectory (the contract is in include/qsv.h, QSV_OP_KRAUS): r = the reduced density matrix
// of the target summed over all pairs, then every pair times the operator kraus_pick draws.  TPB 64 (W <= 10): a lane owns
// at most R pairs and keeps them in registers between the reduction and the apply, so the op reads and writes the state
// once, as a 1Q op does.  R = 8 covers W <= 10 and costs 113 VGPRs (4 waves per SIMD); R = 1 covers W <= 7 with 67, the 7
// waves per SIMD of the kernel without the kind, and small trajectories live on having many in flight.  Wider workgroups (R
// unused): 16 pairs per thread at W = 13 would take 128 registers, so the pairs are read again, B loads in flight; a thread
// sums its pairs in index order (a batch's pairs past the end are zeros), the waves' sums cross through static LDS and every
// thread adds them in wave order.  The caller's barrier after the op also fences that scratch.
// MEAS: the record may also be a MEASURE record, which shares everything but the pick (measure_pick).  Returns the outcome of
// a MEASURE record (0 for a KRAUS record), -1 for a state without mass.
// DYN (with MEAS): a RESET record (QSV_OP_RESET, include/qsv.h) takes the pick of a MEASURE record too; its release flag is set.
template <int TPB, int B, int R, bool MEAS = false, bool DYN = false>
__device__ __forceinline__ int kraus_op(cplx* st, const NzOp& o, const double* __restrict__ pool, uint32_t half, uint32_t tid,
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
      r00 += norm2(a0[j]);
      r11 += norm2(a1[j]);
      rre += fma(a1[j].x, a0[j].x, a1[j].y * a0[j].y);
      rim += fma(a1[j].y, a0[j].x, -(a1[j].x * a0[j].y));
    }
  } else {
    for (uint32_t p0 = tid; p0 < half; p0 += B * TPB) {
      cplx b0[B], b1[B];
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const uint32_t p = p0 + (uint32_t)j * TPB;
        const uint32_t i0 = ((p & ~lo) << 1) | (p & lo);
        b0[j] = b1[j] = make_double2(0.0, 0.0);
        if (p < half) { b0[j] = st[i0]; b1[j] = st[i0 | tb]; }
      }
#pragma unroll
      for (int j = 0; j < B; ++j) {
        r00 += norm2(b0[j]);
        r11 += norm2(b1[j]);
        rre += fma(b1[j].x, b0[j].x, b1[j].y * b0[j].y);
        rim += fma(b1[j].y, b0[j].x, -(b1[j].x * b0[j].y));
      }
    }
  }
  r00 = wave_sum(r00);                                             // xor butterfly: the partners of a step add the same two
  r11 = wave_sum(r11);                                             // numbers, so all 64 lanes end with the same bits
  rre = wave_sum(rre);
  rim = wave_sum(rim);
  if constexpr (TPB > 64) {
    constexpr int NW = TPB / 64;
    __shared__ double part[NW][4];
    if ((tid & 63u) == 0) {
      double* mine = part[tid >> 6];
      mine[0] = r00; mine[1] = r11; mine[2] = rre; mine[3] = rim;
    }
    __syncthreads();
    r00 = part[0][0]; r11 = part[0][1]; rre = part[0][2]; rim = part[0][3];
#pragma unroll
    for (int w = 1; w < NW; ++w) { r00 += part[w][0]; r11 += part[w][1]; rre += part[w][2]; rim += part[w][3]; }
  }
  cplx m00, m01, m10, m11;
  int b = 0;
  if (MEAS && (o.kind == NZ_MEASURE || (DYN && o.kind == NZ_RESET))) {
    b = measure_pick(r00, r11, u, (o.cmask >> 8) & 1u, m00, m01, m10, m11);
    if (b < 0) return -1;
  } else if (!kraus_pick(r00, r11, rre, rim, u, o, pool, m00, m01, m10, m11)) return -1;
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
    pairs<TPB, B>(st, half, tb, tid, [](uint32_t) { return true; },
                  [&](uint32_t, uint32_t, cplx b0, cplx b1, cplx& n0, cplx& n1) {
                    n0 = cmad(m00, b0, cmul(m01, b1));
                    n1 = cmad(m10, b0, cmul(m11, b1));
                  });
  }
  return b;
}

// ---- KRAUS2: a general two-qubit Kraus channel (the contract is in include/qsv.h, QSV_OP_KRAUS2) ---------------------------------
// A quad is the four amplitudes that differ only in the record's two qubits; quad number p is p with a zero bit inserted at
// the lower and then at the higher of the two positions (lom, him: the masks below them), and amplitude x of it has the bit of
// qubit 0 = x & 1 and the bit of qubit 1 = x >> 1.  Only these addresses depend on where the two qubits lie.
__device__ __forceinline__ uint32_t k2_base(uint32_t p, uint32_t lom, uint32_t him) {
  const uint32_t t = ((p & ~lom) << 1) | (p & lom);
  return ((t & ~him) << 1) | (t & him);
}
__device__ __forceinline__ void k2_load(const cplx* st, uint32_t i0, uint32_t b0, uint32_t b1, cplx (&a)[4]) {
  a[0] = st[i0];
  a[1] = st[i0 | b0];
  a[2] = st[i0 | b1];
  a[3] = st[i0 | b0 | b1];
}
// one quad added to rr, the 16 real numbers of r[x][y] = sum a_x conj(a_y) in the packing of the record's E tables: rr[0..4)
// the diagonal, then (re, im) of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  Every index is a constant after unrolling.
__device__ __forceinline__ void k2_accum(double (&rr)[16], const cplx (&a)[4]) {
#pragma unroll
  for (int x = 0; x < 4; ++x) rr[x] += norm2(a[x]);
#pragma unroll
  for (int x = 0; x < 3; ++x) {
#pragma unroll
    for (int y = x + 1; y < 4; ++y) {
      const int n = 4 + 2 * (x == 0 ? y - 1 : x == 1 ? y + 1 : 5);
      rr[n] += fma(a[x].x, a[y].x, a[x].y * a[y].y);
      rr[n + 1] += fma(a[x].y, a[y].x, -(a[x].x * a[y].y));
    }
  }
}
// The operator a KRAUS2 record draws for u and rr, which every lane holds with the same bits: w_k = tr(E_k r) = d + 2 f,
// d over the diagonal and f over the 12 off-diagonal numbers, each in ascending index; the first k whose cumulative weight
// exceeds u total.  Returns k, made uniform so that the operator comes in by scalar loads, and s = sqrt(total / w_k);
// -1: the state has no mass and stays as it is.
__device__ __forceinline__ int kraus2_pick(const double (&rr)[16], double u, const NzOp& o, const double* __restrict__ pool,
                                           double& s) {
  const double* E = pool + o.off + 32u * o.n;
  const double total = ((rr[0] + rr[1]) + rr[2]) + rr[3], r = u * total;
  double cum = 0.0, wk = 0.0, wlast = 0.0;
  int pick = -1, last = -1;
  for (uint32_t k = 0; k < o.n; ++k) {
    const double* e = E + 16u * k;
    double d = e[0] * rr[0], f = e[4] * rr[4];
#pragma unroll
    for (int j = 1; j < 4; ++j) d = fma(e[j], rr[j], d);
#pragma unroll
    for (int j = 5; j < 16; ++j) f = fma(e[j], rr[j], f);
    const double w = fma(2.0, f, d);
    if (w > 0.0) {
      cum += w;
      last = (int)k;
      wlast = w;
      if (pick < 0 && cum > r) { pick = (int)k; wk = w; }
    }
  }
  if (pick < 0) { pick = last; wk = wlast; }                       // rounding at the top boundary: the last k with weight
  if (pick < 0) return -1;
  s = sqrt(total / wk);
  return __builtin_amdgcn_readfirstlane(pick);
}
// n = (m a) s for the 4 x 4 operator m (row-major, re / im: uniform, so its 32 numbers are scalar operands)
__device__ __forceinline__ void k2_apply(const double* __restrict__ m, double s, const cplx (&a)[4], cplx (&n)[4]) {
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    cplx acc = cmul(make_double2(m[8 * x], m[8 * x + 1]), a[0]);
#pragma unroll
    for (int y = 1; y < 4; ++y) acc = cmad(make_double2(m[8 * x + 2 * y], m[8 * x + 2 * y + 1]), a[y], acc);
    n[x] = make_double2(acc.x * s, acc.y * s);
  }
}

// One KRAUS2 record on one trajectory: rr = the 16 numbers of r summed over all quads, then every quad times the operator
// kraus2_pick draws -- kraus_op one size up.  TPB 64 (W <= 10): a lane owns at most R quads (R = 1 up to W = 7, R = 4 up to
// W = 10) and keeps them in registers between the reduction and the apply, so the op reads and writes the state once.  Wider
// workgroups (R unused): the quads are read again, QB of a thread in flight (as many loads as B pairs); a thread sums its
// quads in index order (quads past the end are zeros), the lanes' sums are made equal on every lane by the xor butterfly, the
// waves' sums cross through static LDS (4 x 16 doubles) and every thread adds them in wave order.  The caller's barrier after
// the op also fences that scratch.  false: a state without mass, left as it is.
template <int TPB, int B, int R>
__device__ __forceinline__ bool kraus2_op(cplx* st, const NzOp& o, const double* __restrict__ pool, uint32_t N, uint32_t tid,
                                          double u) {
  constexpr int QB = B > 1 ? B / 2 : 1;
  const uint32_t b0 = 1u << o.target, b1 = 1u << (o.cmask & 255u);
  const uint32_t lom = (b0 < b1 ? b0 : b1) - 1u, him = (b0 < b1 ? b1 : b0) - 1u;
  const uint32_t nquad = N >> 2;
  double rr[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) rr[j] = 0.0;
  cplx q[R][4];
  if constexpr (TPB == 64) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t p = tid + 64u * (uint32_t)j;
#pragma unroll
      for (int x = 0; x < 4; ++x) q[j][x] = make_double2(0.0, 0.0);
      if (p < nquad) k2_load(st, k2_base(p, lom, him), b0, b1, q[j]);
      k2_accum(rr, q[j]);
    }
  } else {
    for (uint32_t p0 = tid; p0 < nquad; p0 += QB * TPB) {
      cplx b[QB][4];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const uint32_t p = p0 + (uint32_t)j * TPB;
#pragma unroll
        for (int x = 0; x < 4; ++x) b[j][x] = make_double2(0.0, 0.0);
        if (p < nquad) k2_load(st, k2_base(p, lom, him), b0, b1, b[j]);
      }
#pragma unroll
      for (int j = 0; j < QB; ++j) k2_accum(rr, b[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) rr[j] = wave_sum(rr[j]);            // xor butterfly: all 64 lanes end with the same bits
  if constexpr (TPB > 64) {
    constexpr int NW = TPB / 64;
    __shared__ double part2[NW][16];
    if ((tid & 63u) == 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j) part2[tid >> 6][j] = rr[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      double v = part2[0][j];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += part2[w][j];
      rr[j] = v;
    }
  }
  double s = 1.0;
  const int pick = kraus2_pick(rr, u, o, pool, s);
  if (pick < 0) return false;
  const double* m = pool + o.off + 32u * (uint32_t)pick;
  if constexpr (TPB == 64) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t p = tid + 64u * (uint32_t)j;
      if (p < nquad) {
        const uint32_t i0 = k2_base(p, lom, him);
        cplx n[4];
        k2_apply(m, s, q[j], n);
        st[i0] = n[0];
        st[i0 | b0] = n[1];
        st[i0 | b1] = n[2];
        st[i0 | b0 | b1] = n[3];
      }
    }
  } else {
    for (uint32_t p0 = tid; p0 < nquad; p0 += QB * TPB) {
      cplx b[QB][4];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const uint32_t p = p0 + (uint32_t)j * TPB;
        if (p < nquad) k2_load(st, k2_base(p, lom, him), b0, b1, b[j]);
      }
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        const uint32_t p = p0 + (uint32_t)j * TPB;
        if (p < nquad) {
          const uint32_t i0 = k2_base(p, lom, him);
          cplx n[4];
          k2_apply(m, s, b[j], n);
          st[i0] = n[0];
          st[i0 | b0] = n[1];
          st[i0 | b1] = n[2];
          st[i0 | b0 | b1] = n[3];
        }
      }
    }
  }
  return true;
}

// One record on one trajectory of N amplitudes, by the TPB threads of its workgroup, and the workgroup barrier that has to
// follow before the state is read again.  PAULI and KRAUS records take the next draw of the shot's stream NZ_STREAM_PAULI
// (draw advances at every one of them, whatever is drawn); an identity Pauli leaves the state as it is and skips the barrier.
// KRAUS > 0: the kind is known, and at TPB 64 a lane holds KRAUS pairs (kraus_op).
// MEAS: MEASURE records are known too (KRAUS > 0 with it: the op is built on kraus_op, and one copy of it serves both kinds).
// A MEASURE record draws from its own stream NZ_STREAM_MEASURE, numbered by the record's ordinal, so `draw` does not advance;
// it writes its bit, flipped by the readout draw nz_word would take for it, into `word`, which every thread holds alike.
// K2: KRAUS2 records are known too (only with MEAS: the kernels that know the kind know every kind).  The record takes the next
// draw of stream NZ_STREAM_PAULI, like a KRAUS record; at TPB 64 a lane holds 1 quad where it holds 1 pair, else 4 (kraus2_op).
// DYN: RESET records are known too (only with K2: the kernels of qsv_noise_dynamic.hip know every kind).  A RESET record is a
// MEASURE record with release set that draws as one -- stream NZ_STREAM_MEASURE, numbered by the record's ordinal among both
// kinds -- and leaves `word` alone.  An IF record never comes here: the shot loops take it, it touches nothing of the state.
template <int TPB, int B, int KRAUS, bool MEAS = false, bool K2 = false, bool DYN = false>
__device__ __forceinline__ void nz_apply(cplx* st, uint32_t N, const NzOp& o, const double* __restrict__ pool, uint32_t tid,
                                         uint64_t seed, uint64_t shot, uint32_t& draw, uint64_t& word) {
  const uint32_t half = N >> 1;
  if constexpr (K2) {
    static_assert(MEAS, "a kernel that knows KRAUS2 records knows MEASURE and KRAUS records");
    static_assert(K2 || !DYN, "a kernel that knows IF and RESET records knows every kind");
    if (o.kind == NZ_KRAUS2) {
      kraus2_op<TPB, B, KRAUS == 1 ? 1 : 4>(st, o, pool, N, tid, philox_u01(seed, shot, NZ_STREAM_PAULI, draw++));
      __syncthreads();
      return;
    }
  }
  if constexpr (MEAS) {
    static_assert(KRAUS > 0, "a kernel that knows MEASURE records knows KRAUS records");
    const bool reset = DYN && o.kind == NZ_RESET;
    if (o.kind == NZ_MEASURE || o.kind == NZ_KRAUS || reset) {
      const bool meas = o.kind == NZ_MEASURE;
      const bool own = meas || reset;                              // a draw of its own stream, not the next of stream 0
      const double u = philox_u01(seed, shot, own ? NZ_STREAM_MEASURE : NZ_STREAM_PAULI, own ? o.cval : draw);
      if (!own) ++draw;
      const int k = kraus_op<TPB, B, KRAUS, true, DYN>(st, o, pool, half, tid, u);
      if (meas) {
        const uint32_t c = o.cmask & 63u;
        uint32_t bit = k > 0 ? 1u : 0u;
        if (philox_u01(seed, shot, NZ_STREAM_READOUT, c) < pool[o.off + bit]) bit ^= 1u;
        word = (word & ~(1ull << c)) | ((uint64_t)bit << c);
      }
      __syncthreads();
      return;
    }
  }
  const auto all = [](uint32_t) { return true; };
  const uint32_t cmask = o.cmask, cval = o.cval;
  const auto ctrl = [=](uint32_t i) { return (i & cmask) == cval; };
  switch (o.kind) {
    case NZ_INIT: {
      const double v = pool[o.off];
      for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2((i & ~cmask) ? 0.0 : v, 0.0);
      break;
    }
    case NZ_1Q: {
      const double* m = pool + o.off;
      const cplx m00 = make_double2(m[0], m[1]), m01 = make_double2(m[2], m[3]);
      const cplx m10 = make_double2(m[4], m[5]), m11 = make_double2(m[6], m[7]);
      pairs<TPB, B>(st, half, 1u << o.target, tid, ctrl, [&](uint32_t, uint32_t, cplx a0, cplx a1, cplx& n0, cplx& n1) {
        n0 = cmad(m00, a0, cmul(m01, a1));
        n1 = cmad(m10, a0, cmul(m11, a1));
      });
      break;
    }
    case NZ_MCX:
      pairs<TPB, B>(st, half, 1u << o.target, tid, ctrl,
                    [](uint32_t, uint32_t, cplx a0, cplx a1, cplx& n0, cplx& n1) { n0 = a1; n1 = a0; });
      break;
    case NZ_DIAG: {
      const cplx* tab = reinterpret_cast<const cplx*>(pool + o.off);   // even offset: 16-byte aligned
      if (o.n == 1) {
        const cplx t0 = tab[0], t1 = tab[1];
        const uint32_t q = nz_qubit(o, 0);
        // LDS state: the table is there before the loop starts.  Scalar loads and LDS reads count on one counter, and a
        // wait for the table placed inside the loop also waits for the iteration's LDS read before the select that could
        // overlap it (measured: DESIGN 5f).  A state in device memory is read on another counter and needs none of this.
        if constexpr (B == 1) asm volatile("" : : "s"(t0.x), "s"(t0.y), "s"(t1.x), "s"(t1.y));
        amps<TPB, B>(st, N, tid, all, [=](uint32_t i, cplx a) { return cmul(a, ((i >> q) & 1u) ? t1 : t0); });
      } else {
        const NzOp l = o;                                          // the list by value, not the caller's record
        amps<TPB, B>(st, N, tid, all, [=](uint32_t i, cplx a) {
          uint32_t j = 0;
          for (uint32_t b = 0; b < l.n; ++b) j |= ((i >> nz_qubit(l, b)) & 1u) << b;
          return cmul(a, tab[j]);
        });
      }
      break;
    }
    case NZ_MCPHASE: {
      const cplx ph = make_double2(pool[o.off], pool[o.off + 1]);
      amps<TPB, B>(st, N, tid, ctrl, [=](uint32_t, cplx a) { return cmul(a, ph); });
      break;
    }
    case NZ_PAULI: {
      const uint32_t p = pauli_draw(philox_u01(seed, shot, NZ_STREAM_PAULI, draw++), o, pool);
      if (p == 0) return;                                      // identity, most draws: no decode, no barrier
      uint32_t xm, zm, ny;
      pauli_masks(p, o, xm, zm, ny);
      if (xm == 0) {                                           // Z-type: a sign per amplitude
        amps<TPB, B>(st, N, tid, [=](uint32_t i) { return (__popc(i & zm) & 1) != 0; },
                     [](uint32_t, cplx a) { return make_double2(-a.x, -a.y); });
      } else {                                                 // amplitude i -> i ^ xm, times (-1)^|i & zm| i^ny
        pairs<TPB, B>(st, half, xm, tid, all, [=](uint32_t i, uint32_t j, cplx a, cplx b, cplx& ni, cplx& nj) {
          nj = pauli_phase(a, ny, __popc(i & zm) & 1);
          ni = pauli_phase(b, ny, __popc(j & zm) & 1);
        });
      }
      break;
    }
    case NZ_KRAUS:
      if constexpr (KRAUS > 0 && !MEAS) kraus_op<TPB, B, KRAUS>(st, o, pool, half, tid, philox_u01(seed, shot, NZ_STREAM_PAULI, draw++));
      break;
    default: break;
  }
  __syncthreads();
}

// The word of a shot that ended in basis state idx, by all 64 lanes of a wave: lane j maps bit j as k_remap_bits does and
// flips it with its readout probability (stream NZ_STREAM_READOUT, draw j); a ballot forms the word.  meas.n < 0: idx itself.
__device__ __forceinline__ uint64_t nz_word(uint32_t idx, uint32_t lane, const NzMeas& meas, const double* __restrict__ pool,
                                            uint64_t seed, uint64_t shot) {
  if (meas.n < 0) return idx;
  uint32_t bit = 0;
  if ((int)lane < meas.n) {
    const int q = meas.pos[lane];
    if (q >= 0) {
      bit = (idx >> q) & 1u;
      if (meas.readout >= 0 && philox_u01(seed, shot, NZ_STREAM_READOUT, lane) < pool[meas.readout + 2 * (int)lane + (int)bit])
        bit ^= 1u;
    }
  }
  return __ballot(bit != 0u);
}
