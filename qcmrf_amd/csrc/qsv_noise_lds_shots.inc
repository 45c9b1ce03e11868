// qsv_noise_lds_shots.inc -- the body of the LDS trajectory kernels (qsv_noise_kernel.h includes it once per kernel): the shots
// first + [blockIdx.x, shots) step gridDim.x of one workgroup, shot first + t to out[t].  The including kernel has TPB, KRAUS,
// MEAS, ACC, K2 (compile-time), first and fix_val in scope besides the arguments of k_noisy.  Text and not a function, so that
// k_noisy compiles to the instructions it had before the accept-aware kernel existed: through a function the arguments lose
// their __restrict__ and the schedule changes (the slot kernel's register allocation too).
// ACC (k_noisy_accept, MEAS only): behind a decisive MEASURE record (NZ_DECISIVE) whose bit in the shot's word differs from
// fix_val the shot is abandoned: thread 0 stores the word as it stands -- it fails (word & fix_mask) == fix_val by that bit,
// which no later record would have written --, the remaining records and the final draw are skipped, and the workgroup goes
// on to its next shot.  Every thread holds the word alike, so the branch is uniform; it is taken right behind the barrier in
// which nz_apply ends, so everything the abandoned shot read of the state (and, at TPB > 64, of kraus_op's scratch) is read
// before any thread writes the next |0..0>.  With one wave per workgroup that barrier is a wait for the wave's own LDS
// accesses, which the LDS serves in order.
// DYN (qsv_noise_dynamic.hip; the including kernel has it in scope too): an IF record (QSV_OP_IF, include/qsv.h) compares the
// word as it stands and, on a miss, adds its span to the record index: the skipped records are not fetched, so they take no
// draw and write no bit, and the ordinals of stream 3 are in the records, which a skip cannot shift.  Every thread holds the
// word alike, so the branch is uniform, and it needs no barrier because nothing of the state is touched.  The abandonment
// check sits behind an executed record, so a decisive record that was skipped abandons nothing.
  static_assert(MEAS || !ACC, "only a MEASURE record ends a shot early");
  extern __shared__ __attribute__((aligned(16))) char nz_lds[];
  cplx* st = reinterpret_cast<cplx*>(nz_lds);              // 2^W amplitudes, nothing else
  const uint32_t N = 1u << W;
  const uint32_t tid = threadIdx.x;
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
      nz_apply<TPB, 1, KRAUS, MEAS, K2, DYN>(st, N, o, pool, tid, seed, shot, draw, mword);
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
    // one basis state from |amp|^2: wave 0, lane l owns the contiguous chunk [l C, (l + 1) C)
    if (tid < 64) {
      const uint32_t lane = tid;
      const uint32_t C = N >= 64u ? N >> 6 : 1u;
      const uint32_t lo = lane * C;
      double part = 0.0;
      if (lo < N)
        for (uint32_t k = 0; k < C; ++k) part += norm2(st[lo + k]);
      const double incl = wave_scan(part, lane);
      double excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 0.0;
      const double total = __shfl(incl, 63, 64);
      const double r = philox_u01(seed, shot, NZ_STREAM_SAMPLE, 0) * total;
      const unsigned long long hit = __ballot(part > 0.0 && incl > r);
      const unsigned long long nz = __ballot(part > 0.0);
      const int owner = hit ? __builtin_ctzll(hit) : (nz ? 63 - __builtin_clzll(nz) : 0);   // rounding slack -> last mass
      uint32_t idx = 0;
      if ((int)lane == owner && lo < N) {
        double run = excl;
        int found = -1, last = -1;
        for (uint32_t k = 0; k < C; ++k) {
          const double pk = norm2(st[lo + k]);
          run += pk;
          if (pk > 0.0) {
            last = (int)k;
            if (found < 0 && run > r) found = (int)k;
          }
        }
        idx = lo + (uint32_t)(found >= 0 ? found : (last >= 0 ? last : 0));
      }
      idx = __shfl(idx, owner, 64);
      uint64_t word = nz_word(idx, lane, meas, pool, seed, shot);
      if constexpr (MEAS) word |= mword;
      if (lane == 0) out[t] = word;
    }
    __syncthreads();                                               // wave 0 is done reading before the next |0..0>
  }
