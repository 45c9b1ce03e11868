// qsv_measure.inc -- block / tile sums, sampling, marginals, amplitude copies (part of qsv.hip)
// ------------------------------------------------------------------------------------------
// measurement
// ------------------------------------------------------------------------------------------
struct SumView {                 // host copy of a shard's block / tile sums, owned by the shard
  const double* p = nullptr;
  size_t n = 0;
  bool super = false;
  size_t size() const { return n; }
  const double* data() const { return p; }
  double operator[](size_t i) const { return p[i]; }
};

// the super sums of a shard's tile sums on the device (d_super), formed once per state: the host copy block_sums
// fetches and the sampler's device walk (sample_chain) share them
static int super_sums(Shard& s, uint64_t nsuper) {
  CHK(shard_set(s));
  if (s.h_tsums_cap < nsuper) {
    if (s.h_tsums) HIPCHK(hipHostFree(s.h_tsums));
    if (s.d_super) HIPCHK(hipFree(s.d_super));
    if (s.d_walk) HIPCHK(hipFree(s.d_walk));
    s.h_tsums = nullptr;
    s.d_super = nullptr;
    s.d_walk = nullptr;
    s.h_tsums_cap = 0;
    s.d_super_valid = 0;
    HIPCHK(hipHostMalloc(&s.h_tsums, nsuper * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMalloc(&s.d_super, nsuper * sizeof(double)));
    HIPCHK(hipMalloc(&s.d_walk, (nsuper + 2) * sizeof(double)));
    s.h_tsums_cap = nsuper;
  }
  if (s.d_super_valid & 1) return QSV_OK;
  hipLaunchKernelGGL(k_supersum, dim3((unsigned)std::min<uint64_t>(nsuper, 65535)), dim3(QSV_TPB), 0, s.stream,
                     s.d_tsums, s.tile_nblocks, s.d_super, nsuper);
  HIPCHK(hipGetLastError());
  s.d_super_valid |= 1;
  return QSV_OK;
}

static int block_sums(qsv_handle* h, Shard& s, SumView& sums) {
  if (s.tile_valid && h->opt_cache_sums) {   // left behind by the last pass of the program: no read pass
    // pinned staging buffer, fetched once per state (norm and sample of one run share it): a
    // 34-qubit shard has 2^21 tiles = 16 MiB of sums, a pageable copy of which costs more than
    // the sampling itself
    const uint64_t nsuper = (s.tile_nblocks + QSV_SUPER - 1) / QSV_SUPER;
    if (!s.h_tsums_valid) {
      CHK(super_sums(s, nsuper));
      HIPCHK(hipMemcpyAsync(s.h_tsums, s.d_super, nsuper * sizeof(double), hipMemcpyDeviceToHost, s.stream));
      HIPCHK(hipStreamSynchronize(s.stream));
      s.h_tsums_valid = true;
    }
    sums.p = s.h_tsums;
    sums.n = nsuper;
    sums.super = true;                    // entries are sums over QSV_SUPER tiles each
    return QSV_OK;
  }
  if (s.sums_valid && h->opt_cache_sums) { sums.p = s.h_sums.data(); sums.n = s.h_sums.size(); return QSV_OK; }
  const uint64_t n = amps_local(h);
  const uint64_t nblk = (n + QSV_SBLOCK - 1) / QSV_SBLOCK;
  CHK(materialize(h, s));                   // the block-sum pass (and k_locate after it) read every amplitude
  CHK(shard_set(s));
  CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)n, [&] {
    const bool nt = h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26);       // a read stream beyond the caches
    // access-pattern experiments (option blocksum_variant): 1 index swizzle (a read-only stream LOSES with it: 0.79 -> 0.67
    // of peak), 2 each wave reads its own contiguous quarter of the block, 4 one workgroup per block instead of a grid-stride loop
    const int bv = h->opt_blocksum_variant;
    const unsigned grid = (unsigned)((bv & 4) ? std::min<uint64_t>(nblk, (1ull << 24) - 1) : std::min<uint64_t>(nblk, (uint64_t)s.n_cu * 16));
    if (nt) hipLaunchKernelGGL(k_blocksum<true>, dim3(grid), dim3(QSV_TPB), 0, s.stream, s.amp, n, s.d_sums, nblk, bv & 3);
    else hipLaunchKernelGGL(k_blocksum<false>, dim3(grid), dim3(QSV_TPB), 0, s.stream, s.amp, n, s.d_sums, nblk, bv & 3);
  }));
  s.h_sums.resize(nblk);
  HIPCHK(hipMemcpyAsync(s.h_sums.data(), s.d_sums, nblk * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  s.sums_valid = true;
  sums.p = s.h_sums.data();
  sums.n = s.h_sums.size();
  return QSV_OK;
}

static double pairwise_sum(const double* x, size_t n) {
  if (n <= 64) { double s = 0; for (size_t i = 0; i < n; ++i) s += x[i]; return s; }
  const size_t m = n / 2;
  return pairwise_sum(x, m) + pairwise_sum(x + m, n - m);
}

extern "C" int qsv_norm(qsv_handle* h, double* out) {
  if (!h || !out) return fail(QSV_E_BADARG, "NULL argument");
  double tot = 0;
  SumView sums;
  for (Shard& s : h->shards) {
    CHK(block_sums(h, s, sums));
    tot += pairwise_sum(sums.data(), sums.size());
  }
  *out = tot;
  return QSV_OK;
}

// qsv_sample on the tile sums of a handle's one shard, without a host round trip (option sample_chain, DESIGN §6): the
// super sums, their walk (k_walk_super) and every later step stay on the device, the host draws the spacings while the
// first two kernels run and waits once, for the words and the total.  A deferred shard's shots are located inside the
// generator (QSV_GEN_LOCATE): no tile is stored.  The arithmetic is that of qsv_sample's host walk, operation for operation:
// the same words come out.  shuffle false (qsv_sample_unordered): the words land in out_bits as the device leaves them,
// ascending in the walk's order; the shuffle's random numbers are not drawn.
static int sample_chain(qsv_handle* h, Shard& sh, uint64_t shots, uint64_t seed, const MeasMap& mm, bool shuffle, uint64_t* out_bits) {
  const uint64_t nsuper = (sh.tile_nblocks + QSV_SUPER - 1) / QSV_SUPER;
  CHK(super_sums(sh, nsuper));
  if (!(sh.d_super_valid & 2)) {
    hipLaunchKernelGGL(k_walk_super, dim3(1), dim3(64), 0, sh.stream, sh.d_super, (int)nsuper, sh.d_walk);
    HIPCHK(hipGetLastError());
    sh.d_super_valid |= 2;
  }
  // one pinned slot: the total the device leaves (first 256 bytes), then the running sums of the spacings, unscaled, which
  // k_walk_shots reads in place
  void* slot = nullptr;
  CHK(arena_slot(sh, 256 + shots * sizeof(double), &slot));
  double* h_total = reinterpret_cast<double*>(slot);
  double* raw = reinterpret_cast<double*>(reinterpret_cast<char*>(slot) + 256);
  *h_total = 0.0;
  std::mt19937_64 rng(seed);
  double run = 0.0;
  for (uint64_t s = 0; s < shots; ++s) {
    run += -std::log((double)((rng() >> 11) + 1ull) * (1.0 / 9007199254740992.0));
    raw[s] = run;
  }
  run += -std::log((double)((rng() >> 11) + 1ull) * (1.0 / 9007199254740992.0));
  if (sh.sample_cap < shots) {
    if (sh.d_sblk) { HIPCHK(hipFree(sh.d_sblk)); HIPCHK(hipFree(sh.d_sres)); HIPCHK(hipFree(sh.d_sout)); }
    sh.d_sblk = nullptr; sh.d_sres = nullptr; sh.d_sout = nullptr;
    sh.sample_cap = 0;
    const size_t cap = std::max<size_t>(shots, 8192);
    HIPCHK(hipMalloc(&sh.d_sblk, cap * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&sh.d_sres, cap * sizeof(double)));
    HIPCHK(hipMalloc(&sh.d_sout, cap * sizeof(uint64_t)));
    sh.sample_cap = cap;
  }
  hipLaunchKernelGGL(k_walk_shots, dim3((unsigned)std::min<uint64_t>((shots + QSV_TPB - 1) / QSV_TPB, 1024)), dim3(QSV_TPB), 0, sh.stream,
                     sh.d_walk, (int)nsuper, raw, run, shots, sh.d_sblk, sh.d_sres, h_total);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_locate_super, dim3((unsigned)std::min<uint64_t>(shots, 65535)), dim3(64), 0, sh.stream,
                     sh.d_tsums, sh.tile_nblocks, sh.d_sblk, sh.d_sres, shots);
  HIPCHK(hipGetLastError());
  if (sh.deferred) {
    CHK(launch_recipe(h, sh, QSV_GEN_LOCATE, sh.d_sblk, shots, sh.d_sres, sh.d_sout));
    HIPCHK(hipGetLastError());
    h->n_listed += 1;
  } else {
    const dim3 g((unsigned)std::min<uint64_t>(shots, 65535));
#define LT(RR) hipLaunchKernelGGL((k_locate_tile<RR>), g, dim3(QSV_TPB), 0, sh.stream, sh.amp, sh.tile_ins, sh.tile_rp, sh.tile_lp, sh.d_sblk, sh.d_sres, sh.d_sout, shots, sh.tile_xor, sh.zmask)
    switch (sh.tile_R) {
      case 0: LT(0); break; case 1: LT(1); break; case 2: LT(2); break; case 3: LT(3); break;
      case 4: LT(4); break; case 5: LT(5); break; default: LT(6); break;
    }
#undef LT
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_remap_bits, dim3((unsigned)((shots + QSV_TPB - 1) / QSV_TPB)), dim3(QSV_TPB), 0, sh.stream,
                     sh.d_sout, shots, (uint64_t)sh.index << h->L, mm);
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> idx(shuffle ? shots : 0);
  HIPCHK(hipMemcpyAsync(shuffle ? idx.data() : out_bits, sh.d_sout, shots * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
  HIPCHK(hipStreamSynchronize(sh.stream));
  const double total = *reinterpret_cast<volatile double*>(h_total);
  if (!(total > 0)) return fail(QSV_E_BADARG, "state has zero norm on this process; nothing to sample");
  if (!shuffle) return QSV_OK;
  for (uint64_t s = shots - 1; s > 0; --s) {
    const uint64_t k = rng() % (s + 1);
    std::swap(idx[s], idx[k]);
  }
  memcpy(out_bits, idx.data(), shots * sizeof(uint64_t));
  return QSV_OK;
}

// The compact index space of a post-selected draw (qsv_sample_cond): the local fixed bits, their values, and the
// number of matching amplitudes of a shard (k_blocksum_cond / k_locate_cond)
struct CondView { BitIns fix; uint64_t val; uint64_t nc; };

// The host walk of qsv_sample and qsv_sample_cond (DESIGN §6): shards, then blocks, then the device inside a block.
// sums[i] / mass[i] are shard i's block, super or compact-block sums and their total (mass 0: the shard is skipped);
// total > 0 is the caller's to check.  cond == NULL: the blocks are those of the state (k_locate / k_locate_tile);
// otherwise compact blocks of the matching sub-cube (k_locate_cond).  shuffle false (the unordered entry points): every
// shard's words are copied straight into out_bits, in the walk's ascending order, and no shuffle is drawn.
static int sample_walk(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                       const std::vector<SumView>& sums, const std::vector<double>& mass, double total,
                       const CondView* cond, bool shuffle, uint64_t* out_bits) {
  const size_t ns = h->shards.size();
  // sorted uniforms in [0,total) WITHOUT a sort: the order statistics of n iid uniforms are the
  // normalised partial sums of n + 1 iid exponentials (a sort of 4096 doubles cost 0.12 ms, a
  // quarter of the whole call at 34 qubits)
  std::mt19937_64 rng(seed);
  std::vector<double> r(shots);
  {
    double run = 0.0;
    for (uint64_t s = 0; s < shots; ++s) {
      run += -std::log((double)((rng() >> 11) + 1ull) * (1.0 / 9007199254740992.0));
      r[s] = run;
    }
    run += -std::log((double)((rng() >> 11) + 1ull) * (1.0 / 9007199254740992.0));
    const double scale = total / run;
    for (uint64_t s = 0; s < shots; ++s) r[s] = std::min(r[s] * scale, std::nextafter(total, 0.0));
  }
  std::vector<uint64_t> idx(shuffle ? shots : 0);
  uint64_t* const words = shuffle ? idx.data() : out_bits;
  MeasMap mm;
  mm.n = meas_qubits ? n_meas : -1;                      // -1: the full basis index
  for (int j = 0; j < 64; ++j) mm.pos[j] = (meas_qubits && j < n_meas) ? (signed char)meas_qubits[j] : (signed char)-1;
  int last_shard = -1;
  for (size_t i = 0; i < ns; ++i) if (mass[i] > 0) last_shard = (int)i;
  uint64_t s0 = 0;
  double base = 0;
  for (size_t i = 0; i < ns && s0 < shots; ++i) {
    if (!(mass[i] > 0)) continue;
    Shard& sh = h->shards[i];
    const double top = ((int)i == last_shard) ? INFINITY : base + mass[i];
    uint64_t s1 = s0;
    while (s1 < shots && r[s1] < top) ++s1;
    const uint64_t cnt = s1 - s0;
    if (cnt) {
      // walk the blocks of this shard; rounding slack is clamped to the last populated block
      std::vector<uint64_t> blk(cnt);
      std::vector<double> res(cnt);
      const SumView& bs = sums[i];
      size_t last_nz = 0;
      for (size_t bb = 0; bb < bs.size(); ++bb) if (bs[bb] > 0) last_nz = bb;
      size_t b = 0;
      double pre = base;                 // mass before block b
      for (uint64_t q = 0; q < cnt; ++q) {
        const double x = r[s0 + q];
        while (b < last_nz && x >= pre + bs[b]) { pre += bs[b]; ++b; }
        blk[q] = b;
        res[q] = std::max(0.0, x - pre);
      }
      CHK(shard_set(sh));
      if (sh.sample_cap < cnt) {
        if (sh.d_sblk) { HIPCHK(hipFree(sh.d_sblk)); HIPCHK(hipFree(sh.d_sres)); HIPCHK(hipFree(sh.d_sout)); }
        sh.sample_cap = std::max<size_t>(cnt, 8192);
        HIPCHK(hipMalloc(&sh.d_sblk, sh.sample_cap * sizeof(uint64_t)));
        HIPCHK(hipMalloc(&sh.d_sres, sh.sample_cap * sizeof(double)));
        HIPCHK(hipMalloc(&sh.d_sout, sh.sample_cap * sizeof(uint64_t)));
      }
      // The shots' (block, residual) pairs go to the device through the pinned arena and a kernel that reads it, not as
      // two copies from pageable memory: those are staged copies on a copy engine, each with a host wait, and the first
      // one after event timing has been switched on stalls for 8-20 ms inside the runtime (profiles/r09_factored_sums.log)
      // -- once per process, but a step is 2.5 ms.  Lists beyond a quarter of the arena take the copies as before.
      if (2 * cnt * sizeof(uint64_t) <= sh.arena_bytes / 4) {
        void* hb = nullptr;
        void* hr = nullptr;
        CHK(arena_stage(sh, blk.data(), cnt * sizeof(uint64_t), &hb));
        CHK(arena_stage(sh, res.data(), cnt * sizeof(double), &hr));
        hipLaunchKernelGGL(k_stage_shots, dim3((unsigned)std::min<uint64_t>((cnt + QSV_TPB - 1) / QSV_TPB, 1024)), dim3(QSV_TPB), 0, sh.stream,
                           reinterpret_cast<const uint64_t*>(hb), reinterpret_cast<const double*>(hr), sh.d_sblk, sh.d_sres, cnt);
        HIPCHK(hipGetLastError());
      } else {
        HIPCHK(hipMemcpyAsync(sh.d_sblk, blk.data(), cnt * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
        HIPCHK(hipMemcpyAsync(sh.d_sres, res.data(), cnt * sizeof(double), hipMemcpyHostToDevice, sh.stream));
      }
      if (bs.super) {                     // (super block, mass) -> (tile, mass) on the device
        hipLaunchKernelGGL(k_locate_super, dim3((unsigned)std::min<uint64_t>(cnt, 65535)), dim3(64), 0, sh.stream,
                           sh.d_tsums, sh.tile_nblocks, sh.d_sblk, sh.d_sres, cnt);
        HIPCHK(hipGetLastError());
      }
      if (bs.super && sh.deferred) {
        // Deferred state: d_sblk now holds each shot's tile.  One launch of the generator's listed form stores exactly
        // those tiles at their real addresses (a tile listed several times once: the list is non-decreasing and an entry
        // equal to its predecessor is skipped); k_locate_tile then reads what the writing form would have stored.  Part
        // of sampling: like k_locate_*, not booked as a sweep.
        CHK(launch_recipe(h, sh, QSV_GEN_LISTED, sh.d_sblk, cnt));
        HIPCHK(hipGetLastError());
        h->n_listed += 1;
      }
      if (cond) {                         // compact blocks of the matching sub-cube; implied zeros are not read
        hipLaunchKernelGGL(k_locate_cond, dim3((unsigned)std::min<uint64_t>(cnt, 65535)), dim3(64), 0, sh.stream,
                           sh.amp, cond->nc, cond->fix, cond->val, sh.zmask, sh.d_sblk, sh.d_sres, sh.d_sout, cnt);
      } else if (bs.super) {              // tile order of the program's last pass
        const dim3 g((unsigned)std::min<uint64_t>(cnt, 65535));
#define LT(RR) hipLaunchKernelGGL((k_locate_tile<RR>), g, dim3(QSV_TPB), 0, sh.stream, sh.amp, sh.tile_ins, sh.tile_rp, sh.tile_lp, sh.d_sblk, sh.d_sres, sh.d_sout, cnt, sh.tile_xor, sh.zmask)
        switch (sh.tile_R) {
          case 0: LT(0); break; case 1: LT(1); break; case 2: LT(2); break; case 3: LT(3); break;
          case 4: LT(4); break; case 5: LT(5); break; default: LT(6); break;
        }
#undef LT
      } else {
        CHK(materialize(h, sh));          // (done by block_sums already; k_locate reads amplitudes, not tile sums)
        hipLaunchKernelGGL(k_locate, dim3((unsigned)std::min<uint64_t>(cnt, 65535)), dim3(64), 0, sh.stream,
                           sh.amp, amps_local(h), sh.d_sblk, sh.d_sres, sh.d_sout, cnt);
      }
      HIPCHK(hipGetLastError());
      // global index -> the caller's bit layout, still on the device (one thread per shot)
      hipLaunchKernelGGL(k_remap_bits, dim3((unsigned)((cnt + QSV_TPB - 1) / QSV_TPB)), dim3(QSV_TPB), 0, sh.stream,
                         sh.d_sout, cnt, (uint64_t)sh.index << h->L, mm);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(words + s0, sh.d_sout, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
      HIPCHK(hipStreamSynchronize(sh.stream));
    }
    base += mass[i];
    s0 = s1;
  }
  if (!shuffle) return QSV_OK;
  // shots come out sorted by index; decorrelate the order with the same generator
  for (uint64_t s = shots - 1; s > 0; --s) {
    const uint64_t k = rng() % (s + 1);
    std::swap(idx[s], idx[k]);
  }
  memcpy(out_bits, idx.data(), shots * sizeof(uint64_t));
  return QSV_OK;
}

static int sample_any(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas, bool shuffle,
                      uint64_t* out_bits) {
  if (!h || (shots && !out_bits)) return fail(QSV_E_BADARG, "NULL argument");
  if (meas_qubits && (n_meas < 0 || n_meas > 64)) return fail(QSV_E_BADARG, "n_meas %d out of range", n_meas);
  if (meas_qubits) for (int i = 0; i < n_meas; ++i) if (meas_qubits[i] >= 0) CHK(check_qubit(h, meas_qubits[i], "measured"));
  if (shots == 0) return QSV_OK;
  if (h->opt_sample_chain && h->shards.size() == 1) {
    // one shard, the tile path, a power-of-two tile count within k_walk_super's reach, the spacings within a quarter of the
    // arena; everything else walks on the host as before
    Shard& sh = h->shards[0];
    const uint64_t nt = sh.tile_nblocks;
    if (sh.tile_valid && h->opt_cache_sums && nt && !(nt & (nt - 1)) && (nt + QSV_SUPER - 1) / QSV_SUPER <= QSV_WALK_MAX &&
        256 + shots * sizeof(double) <= sh.arena_bytes / 4 && (!sh.deferred || sh.zmask == sh.recipe.zskip)) {
      MeasMap cm;
      cm.n = meas_qubits ? n_meas : -1;
      for (int j = 0; j < 64; ++j) cm.pos[j] = (meas_qubits && j < n_meas) ? (signed char)meas_qubits[j] : (signed char)-1;
      return sample_chain(h, sh, shots, seed, cm, shuffle, out_bits);
    }
  }
  const size_t ns = h->shards.size();
  std::vector<SumView> sums(ns);
  std::vector<double> mass(ns);
  double total = 0;
  for (size_t i = 0; i < ns; ++i) {
    CHK(block_sums(h, h->shards[i], sums[i]));
    mass[i] = pairwise_sum(sums[i].data(), sums[i].size());
    total += mass[i];
  }
  if (!(total > 0)) return fail(QSV_E_BADARG, "state has zero norm on this process; nothing to sample");
  return sample_walk(h, shots, seed, meas_qubits, n_meas, sums, mass, total, nullptr, shuffle, out_bits);
}
extern "C" int qsv_sample(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                          uint64_t* out_bits) {
  return sample_any(h, shots, seed, meas_qubits, n_meas, true, out_bits);
}
extern "C" int qsv_sample_unordered(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                                    uint64_t* out_bits) {
  return sample_any(h, shots, seed, meas_qubits, n_meas, false, out_bits);
}

// A deferred shard ahead of a post-selected draw (DESIGN §6): the matching sub-cube lies inside the tiles whose block
// bits agree with the fixed block bits.  Their indices -- ascending, each once: the free tile-index bits counted up, the
// fixed ones deposited -- go to the generator's listed form, which stores exactly those tiles; the shard stays deferred.
// Option post_select_list: -1 lists when the list is at most ntiles >> QSV_PROD_MAXG entries (the listed form walks a whole
// group, up to 2^QSV_PROD_MAXG tiles of arithmetic, per tile stored; a reasoned break-even, not a measured one) and fits
// a quarter of the arena; 1 whenever a block bit is fixed and the list fits; 0 never.  Otherwise the state is realised.
static int cond_prepare_deferred(qsv_handle* h, Shard& s, uint64_t lmask, uint64_t lval) {
  const GenRecipe& rc = s.recipe;
  BitIns tf;                                         // fixed bits of the tile index, ascending
  tf.n = 0;
  uint64_t tval = 0;
  for (int b = 0; (1ull << b) < rc.ntiles; ++b) {
    // tile-index bit b is this address bit (tile_base_blk)
    const uint64_t a = ins_bits(rc.lp.pos[0] < 0 ? (1ull << b) * QSV_TPB : (1ull << b) << 5, rc.ins);
    if (!(a & lmask)) continue;
    tf.pos[tf.n++] = b;
    if (a & lval) tval |= 1ull << b;
  }
  const uint64_t nlist = rc.ntiles >> tf.n;
  const bool fits = nlist * sizeof(uint64_t) <= s.arena_bytes / 4;
  const int pl = h->opt_post_select_list;
  const bool list = tf.n > 0 && fits && s.zmask == rc.zskip && pl != 0 && (pl > 0 || nlist <= (rc.ntiles >> QSV_PROD_MAXG));
  if (h->opt_trace_passes)
    fprintf(stderr, "[qsv] post_select shard %d: %d block bits fixed, %llu of %llu tiles hold the sub-cube: %s\n", s.index, tf.n,
            (unsigned long long)nlist, (unsigned long long)rc.ntiles, list ? "listed" : "realised");
  if (!list) return realize(h, s);
  std::vector<uint64_t> tiles(nlist);
  for (uint64_t j = 0; j < nlist; ++j) tiles[j] = ins_bits(j, tf) | tval;
  void* dl = nullptr;
  CHK(arena_put(s, tiles.data(), nlist * sizeof(uint64_t), &dl));
  CHK(launch_recipe(h, s, QSV_GEN_LISTED, reinterpret_cast<const uint64_t*>(dl), nlist));
  HIPCHK(hipGetLastError());
  h->n_listed += 1;
  return QSV_OK;
}

static int sample_cond_any(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                           uint64_t fix_mask, uint64_t fix_val, bool shuffle, uint64_t* out_bits, double* mass_out) {
  if (!h || (shots && !out_bits)) return fail(QSV_E_BADARG, "NULL argument");
  if (meas_qubits && (n_meas < 0 || n_meas > 64)) return fail(QSV_E_BADARG, "n_meas %d out of range", n_meas);
  if (meas_qubits) for (int i = 0; i < n_meas; ++i) if (meas_qubits[i] >= 0) CHK(check_qubit(h, meas_qubits[i], "measured"));
  if (fix_val & ~fix_mask) return fail(QSV_E_BADARG, "fix_val has bits outside fix_mask");
  if (h->W < 64 && (fix_mask >> h->W)) return fail(QSV_E_BADARG, "fix_mask has bits at or above qubit %d", h->W);
  if (!fix_mask) {                                   // nothing fixed: qsv_sample itself, word for word
    if (mass_out) CHK(qsv_norm(h, mass_out));
    return sample_any(h, shots, seed, meas_qubits, n_meas, shuffle, out_bits);
  }
  const uint64_t n = amps_local(h);
  const uint64_t lmask = fix_mask & (n - 1), lval = fix_val & (n - 1);
  CondView cv;
  cv.fix.n = 0;
  for (int q = 0; q < h->L; ++q)
    if ((lmask >> q) & 1ull) {
      if (cv.fix.n == QSV_MAXB) return fail(QSV_E_UNSUPPORTED, "more than %d fixed bits local to a shard", QSV_MAXB);
      cv.fix.pos[cv.fix.n++] = q;
    }
  cv.val = lval;
  cv.nc = n >> cv.fix.n;
  const uint64_t nblk = (cv.nc + QSV_SBLOCK - 1) / QSV_SBLOCK;
  const size_t ns = h->shards.size();
  std::vector<std::vector<double>> csum(ns);         // not cached: a second call repeats the 2^-f pass
  std::vector<SumView> sums(ns);
  std::vector<double> mass(ns, 0.0);
  double total = 0;
  for (size_t i = 0; i < ns; ++i) {
    Shard& s = h->shards[i];
    // a fixed shard bit does not enter the kernels: a shard whose index disagrees with it has mass 0 and is skipped
    if ((((uint64_t)s.index << h->L) & fix_mask) != (fix_val & ~(n - 1))) continue;
    CHK(shard_set(s));
    if (s.deferred) CHK(cond_prepare_deferred(h, s, lmask, lval));
    CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)cv.nc, [&] {
      // every fixed bit at or above bit 12: a compact block is one contiguous 64 KiB run, streamed as k_blocksum does
      const bool nt = (cv.fix.n == 0 || cv.fix.pos[0] >= 12) && (h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26));
      const unsigned grid = (unsigned)std::min<uint64_t>(nblk, (uint64_t)s.n_cu * 16);
      if (nt) hipLaunchKernelGGL(k_blocksum_cond<true>, dim3(grid), dim3(QSV_TPB), 0, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, s.d_sums, nblk);
      else hipLaunchKernelGGL(k_blocksum_cond<false>, dim3(grid), dim3(QSV_TPB), 0, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, s.d_sums, nblk);
    }));
    csum[i].resize(nblk);
    HIPCHK(hipMemcpyAsync(csum[i].data(), s.d_sums, nblk * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    sums[i].p = csum[i].data();
    sums[i].n = csum[i].size();
    mass[i] = pairwise_sum(sums[i].data(), sums[i].size());
    total += mass[i];
  }
  if (mass_out) *mass_out = total;
  if (shots == 0) return QSV_OK;
  if (!(total > 0)) return fail(QSV_E_BADARG, "post-selected outcome has zero probability");
  return sample_walk(h, shots, seed, meas_qubits, n_meas, sums, mass, total, &cv, shuffle, out_bits);
}
extern "C" int qsv_sample_cond(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                               uint64_t fix_mask, uint64_t fix_val, uint64_t* out_bits, double* mass_out) {
  return sample_cond_any(h, shots, seed, meas_qubits, n_meas, fix_mask, fix_val, true, out_bits, mass_out);
}
extern "C" int qsv_sample_cond_unordered(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                                         uint64_t fix_mask, uint64_t fix_val, uint64_t* out_bits, double* mass_out) {
  return sample_cond_any(h, shots, seed, meas_qubits, n_meas, fix_mask, fix_val, false, out_bits, mass_out);
}

// reduction scratch of a shard: a marginal or an expectation value per branch node of a trajectory run is thousands of
// calls -- no hipMalloc / hipFree (a device-wide synchronisation each) per call
static int red_scratch(Shard& s, size_t n_doubles, double** out, bool* temp) {
  *temp = n_doubles > (1u << 24);                           // (kept up to 128 MiB: the tile sums of a 34-qubit expectation value are 64; a 2^26-entry marginal is not worth keeping 512 MiB for)
  if (*temp) { HIPCHK(hipMalloc(out, n_doubles * sizeof(double))); return QSV_OK; }
  if (s.red_cap < n_doubles) {
    if (s.d_red) HIPCHK(hipFree(s.d_red));
    s.d_red = nullptr;
    s.red_cap = 0;
    const size_t cap = std::max<size_t>(n_doubles, 8192);
    HIPCHK(hipMalloc(&s.d_red, cap * sizeof(double)));
    s.red_cap = cap;
  }
  *out = s.d_red;
  return QSV_OK;
}

extern "C" int qsv_probabilities_cond(qsv_handle* h, const int* qubits, int k, uint64_t fix_mask, uint64_t fix_val,
                                      double* out) {
  if (!h || !out || (k && !qubits)) return fail(QSV_E_BADARG, "NULL argument");
  if (k < 0 || k > 26) return fail(QSV_E_BADARG, "marginal over %d qubits unsupported (max 26)", k);
  for (int i = 0; i < k; ++i) CHK(check_qubit(h, qubits[i], "marginal"));
  const int ntab = 1 << k;
  BitList bl;
  bl.n = k;
  for (int b = 0; b < k; ++b) bl.pos[b] = qubits[b];
  std::vector<double> part(ntab);
  for (int i = 0; i < ntab; ++i) out[i] = 0.0;
  const uint64_t n = amps_local(h);
  CHK(materialize_all(h));
  for (Shard& s : h->shards) {
    CHK(shard_set(s));
    double* d_out = nullptr;
    bool temp = false;
    CHK(red_scratch(s, (size_t)ntab, &d_out, &temp));
    HIPCHK(hipMemsetAsync(d_out, 0, ntab * sizeof(double), s.stream));
    const uint64_t hi = (uint64_t)s.index << h->L;
    const bool lds = k <= 12;
    CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)n, [&] {
      const dim3 g(grid_for(h, s, n, QSV_TPB * 8));
      if (lds) hipLaunchKernelGGL((k_marginal<true>), g, dim3(QSV_TPB), ntab * sizeof(double), s.stream, s.amp, n, hi, bl, fix_mask, fix_val, d_out, ntab);
      else     hipLaunchKernelGGL((k_marginal<false>), g, dim3(QSV_TPB), 0, s.stream, s.amp, n, hi, bl, fix_mask, fix_val, d_out, ntab);
    }));
    HIPCHK(hipMemcpyAsync(part.data(), d_out, ntab * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (temp) HIPCHK(hipFree(d_out));
    for (int i = 0; i < ntab; ++i) out[i] += part[i];
  }
  return QSV_OK;
}
extern "C" int qsv_probabilities(qsv_handle* h, const int* qubits, int k, double* out) {
  return qsv_probabilities_cond(h, qubits, k, 0ull, 0ull, out);
}

#define QSV_ED(LD, N, SH) hipLaunchKernelGGL((k_expect_diag<LD, N>), dim3(nblk), dim3(QSV_TPB), SH, s.stream, s.amp, n, hi, bl, fix_mask, fix_val, d_tab, ntab, d_part, tiled ? 2 : (h->opt_blocksum_variant & 3))
extern "C" int qsv_expect_diag(qsv_handle* h, const int* qubits, int k, const double* table, uint64_t fix_mask,
                               uint64_t fix_val, double* out) {
  if (!h || !out || !table || (k && !qubits)) return fail(QSV_E_BADARG, "NULL argument");
  if (k < 0 || k > 26) return fail(QSV_E_BADARG, "diagonal observable over %d qubits unsupported (max 26)", k);
  CHK(check_distinct(h, k, qubits, -1));
  const int ntab = 1 << k;
  BitList bl;
  bl.n = k;
  for (int b = 0; b < k; ++b) bl.pos[b] = qubits[b];
  const uint64_t n = amps_local(h);
  const size_t tbytes = (size_t)ntab * sizeof(double);
  const bool lds = k <= 12;                                  // 32 KiB of table in LDS; wider ones through L2
  out[0] = out[1] = 0.0;
  CHK(materialize_all(h));
  for (Shard& s : h->shards) {
    CHK(shard_set(s));
    double* d_tab = nullptr;
    bool own_tab = false;
    if (tbytes <= (1u << 20)) {
      void* p = nullptr;
      CHK(arena_put(s, table, tbytes, &p));
      d_tab = reinterpret_cast<double*>(p);
    } else {
      HIPCHK(hipMalloc(&d_tab, tbytes));
      own_tab = true;
      HIPCHK(hipMemcpyAsync(d_tab, table, tbytes, hipMemcpyHostToDevice, s.stream));
    }
    // A read-only stream wants fresh workgroups in launch order, each on its own contiguous 64 KiB (blocksum_variant & 4,
    // profiles/r02_blocksum_variants.log), not a grid-stride loop: one workgroup per 4096 amplitudes, one pair of partial
    // sums each, and a second kernel that folds them -- in a fixed order -- into one pair per folding workgroup.
    const bool tiled = (h->opt_blocksum_variant & 4) && n >= (1ull << 20) && (n >> 12) < (1ull << 31);
    const unsigned nblk = tiled ? (unsigned)(n >> 12)
                                : (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + QSV_TPB * 4 - 1) / (QSV_TPB * 4), (uint64_t)s.n_cu * 8));
    const unsigned nfold = tiled ? 1024u : nblk;
    double* d_part = nullptr;
    bool temp = false;
    CHK(red_scratch(s, 2 * (size_t)nblk + (tiled ? 2 * (size_t)nfold : 0), &d_part, &temp));
    double* d_fold = tiled ? d_part + 2 * (size_t)nblk : d_part;
    const uint64_t hi = (uint64_t)s.index << h->L;
    CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)n, [&] {
      const bool nt = h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26);
      if (lds) { if (nt) QSV_ED(true, true, tbytes); else QSV_ED(true, false, tbytes); }
      else     { if (nt) QSV_ED(false, true, 0); else QSV_ED(false, false, 0); }
      if (tiled) hipLaunchKernelGGL(k_reduce_pairs, dim3(nfold), dim3(QSV_TPB), 0, s.stream, d_part, (uint64_t)nblk, d_fold);
    }));
    std::vector<double> part(2 * (size_t)nfold);
    HIPCHK(hipMemcpyAsync(part.data(), d_fold, part.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (temp) HIPCHK(hipFree(d_part));
    if (own_tab) HIPCHK(hipFree(d_tab));
    std::vector<double> a(nfold), b(nfold);
    for (unsigned i = 0; i < nfold; ++i) { a[i] = part[2 * i]; b[i] = part[2 * i + 1]; }
    out[0] += pairwise_sum(a.data(), a.size());
    out[1] += pairwise_sum(b.data(), b.size());
  }
  return QSV_OK;
}

static int amp_copy(qsv_handle* h, uint64_t start, uint64_t count, double* out, const double* in) {
  if (!h || (count && !out && !in)) return fail(QSV_E_BADARG, "NULL argument");
  const uint64_t n = amps_local(h);
  uint64_t done = 0;
  while (done < count) {
    const uint64_t g = start + done;
    const int si = (int)(g >> h->L);
    Shard* sh = nullptr;
    for (Shard& s : h->shards) if (s.index == si) sh = &s;
    if (!sh) return fail(QSV_E_BADARG, "amplitude %llu lives on shard %d, which this process does not own", (unsigned long long)g, si);
    const uint64_t off = g & (n - 1);
    const uint64_t m = std::min(count - done, n - off);
    CHK(shard_set(*sh));
    if (out) CHK(realize(h, *sh));        // a deferred state is written before it is read (the write path: materialize below)
    HIPCHK(hipStreamSynchronize(sh->stream));
    if (out) {
      HIPCHK(hipMemcpy(out + 2 * done, sh->amp + off, m * sizeof(cplx), hipMemcpyDeviceToHost));
      // implied zeros: the copy of undefined memory is overwritten by the zeros it stands for.  zmask is constant on
      // every aligned run of 2^(lowest zmask bit) amplitudes: one memset per run.  A zero qubit on bit 0 makes that one
      // per amplitude -- a few ns each, the order of the PCIe copy of its 16 bytes, on this debugging read path; cheaper
      // than writing the zero half of a large shard on the device for a read of a few amplitudes.
      if (sh->zmask) {
        const uint64_t run = sh->zmask & (0 - sh->zmask);
        for (uint64_t a = off; a < off + m;) {
          const uint64_t e = std::min(off + m, (a | (run - 1)) + 1);
          if (a & sh->zmask) memset(out + 2 * (done + (a - off)), 0, (e - a) * sizeof(cplx));
          a = e;
        }
      }
    } else {
      CHK(materialize(h, *sh));           // a partial write into the zero region must not be lost
      CHK(shard_set(*sh));
      HIPCHK(hipStreamSynchronize(sh->stream));
      HIPCHK(hipMemcpy(sh->amp + off, in + 2 * done, m * sizeof(cplx), hipMemcpyHostToDevice));
      sh->sums_valid = false; sh->tile_valid = false; sh->h_tsums_valid = false; sh->d_super_valid = 0;
    }
    done += m;
  }
  return QSV_OK;
}
extern "C" int qsv_copy_state(qsv_handle* dst, qsv_handle* src) {
  if (!dst || !src) return fail(QSV_E_BADARG, "NULL handle");
  if (dst->W != src->W || dst->P != src->P || dst->shards.size() != src->shards.size())
    return fail(QSV_E_BADARG, "qsv_copy_state: handles differ in shape (%d/%d qubits, %d/%d shards)", dst->W, src->W, dst->P, src->P);
  const size_t bytes = amps_local(src) * sizeof(cplx);
  for (size_t i = 0; i < src->shards.size(); ++i) {
    Shard& a = src->shards[i];
    Shard& b = dst->shards[i];
    if (a.index != b.index) return fail(QSV_E_BADARG, "qsv_copy_state: shard order differs");
    // destination after source, source after the copy: two events, no host round trip
    CHK(shard_set(a));
    CHK(realize(src, a));                 // the copy reads the whole source shard; the destination's old state, deferred or not, is gone
    b.deferred = false;
    if (!a.ev_ready) HIPCHK(hipEventCreateWithFlags(&a.ev_ready, hipEventDisableTiming));
    HIPCHK(hipEventRecord(a.ev_ready, a.stream));
    CHK(shard_set(b));
    HIPCHK(hipStreamWaitEvent(b.stream, a.ev_ready, 0));
    HIPCHK(hipMemcpyAsync(b.amp, a.amp, bytes, hipMemcpyDeviceToDevice, b.stream));
    // the copy runs on the DESTINATION's stream: whatever the source is asked to do next (a trajectory run projects it on
    // the sibling outcome at once) must not start before its amplitudes have been read
    if (!a.ev_copied) HIPCHK(hipEventCreateWithFlags(&a.ev_copied, hipEventDisableTiming));
    HIPCHK(hipEventRecord(a.ev_copied, b.stream));
    CHK(shard_set(a));
    HIPCHK(hipStreamWaitEvent(a.stream, a.ev_copied, 0));
    b.zmask = a.zmask;
    b.sums_valid = false;
    b.tile_valid = false;
    b.h_tsums_valid = false; b.d_super_valid = 0;
    dst->stats.per_kind[QSV_K_SWAP].launches += 1;
    dst->stats.per_kind[QSV_K_SWAP].algorithmic_bytes += 2.0 * (double)bytes;
  }
  return QSV_OK;
}
extern "C" int qsv_get_amplitudes(qsv_handle* h, uint64_t start, uint64_t count, double* out) { return amp_copy(h, start, count, out, nullptr); }
extern "C" int qsv_set_amplitudes(qsv_handle* h, uint64_t start, uint64_t count, const double* in) { return amp_copy(h, start, count, nullptr, in); }
