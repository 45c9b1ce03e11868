// qsv_noise_hbm_shots.inc -- the body of the slot-path trajectory kernels (qsv_noise_hbm_kernel.h includes it once per kernel):
// the shots first + [blockIdx.x, shots) step gridDim.x of one workgroup in its slot, shot first + t to out[t].  The including
// kernel has TPB, MEAS, ACC, K2 (compile-time), first and fix_val in scope besides the arguments of k_noisy_hbm.  Text and not a
// function, so that k_noisy_hbm compiles to the instructions it had before the accept-aware kernel existed (see there).
// ACC (k_noisy_hbm_accept): behind a decisive MEASURE record (NZ_DECISIVE) whose bit in the shot's word differs from fix_val
// the shot is abandoned as qsv_noise_lds_shots.inc abandons it, and for the same reasons: the branch is uniform and
// sits right behind the barrier in which nz_apply ends, which also orders the workgroup's loads of the slot before the stores
// of the next |0..0>.  The scratch of the final draw (fd_*) is touched by the final draw alone, and a shot that runs it leaves
// it behind its own closing barrier, so a shot that skips it finds and leaves nothing pending there.
// DYN (the including kernel has it in scope too): IF records skip as qsv_noise_lds_shots.inc skips them.
  static_assert(TPB % 64 == 0 && TPB >= 64, "whole waves");
  constexpr int NW = TPB / 64;
  __shared__ double fd_wsum[NW];
  __shared__ unsigned long long fd_hit[NW], fd_nz[NW];
  __shared__ double fd_excl;
  cplx* st = reinterpret_cast<cplx*>(slots + (uint64_t)blockIdx.x * ((uint64_t)16 << W));   // 64-bit byte offset
  const uint32_t N = 1u << W;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint64_t t = blockIdx.x; t < shots; t += gridDim.x) {
    const uint64_t shot = first + t;
    for (uint32_t i = tid; i < N; i += TPB) st[i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    __syncthreads();
    uint32_t draw = 0;
    uint64_t mword = 0;                                            // the bits MEASURE records wrote (MEAS only)
    bool dead = false;
    for (int k = 0; k < n_ops; ++k) {
      const NzOp o = nz_fetch(ops, k);
      if constexpr (DYN) {
        if (o.kind == NZ_IF) {                                       // span and mask are in the record's first 16 bytes
          const uint64_t mask = (uint64_t)o.cval | ((uint64_t)o.off << 32);
          const bool hit = ((mword & mask) == o.ql8) != (o.target != 0u);
          k += (int)__builtin_amdgcn_readfirstlane(hit ? 0u : o.cmask);   // every thread holds mword alike: say so, k stays scalar
          continue;
        }
      }
      nz_apply<TPB, QSV_NZ_HBM_B, 1, MEAS, K2, DYN>(st, N, o, pool, tid, seed, shot, draw, mword);
      if constexpr (ACC) {
        if (o.kind == NZ_MEASURE && (o.cmask & NZ_DECISIVE) && (((mword ^ fix_val) >> (o.cmask & 63u)) & 1ull)) {
          dead = true;
          break;
        }
      }
    }
    if constexpr (ACC) {
      if (dead) {
        if (tid == 0) out[t] = mword;
        continue;
      }
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
    const double r = philox_u01(seed, shot, NZ_STREAM_SAMPLE, 0) * total;
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
      uint64_t word = nz_word(idx, lane, meas, pool, seed, shot);
      if constexpr (MEAS) word |= mword;
      if (lane == 0) out[t] = word;
    }
    __syncthreads();                                               // wave 0 is done reading before the next |0..0>
  }
