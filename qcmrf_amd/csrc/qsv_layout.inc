// qsv_layout.inc -- dense k-qubit gates, local bit swaps, the shard-bit exchange (part of qsv.hip)
template <int K>
static void launch_kq(const qsv_handle* h, const Shard& s, uint64_t ngroups, const BitIns& ins,
                      const KqOffs& offs, const cplx* u) {
  const size_t shm = sizeof(cplx) << (2 * K);
  hipLaunchKernelGGL((k_kq<K>), dim3(grid_for(h, s, ngroups, QSV_TPB)), dim3(QSV_TPB), shm, s.stream,
                     s.amp, ngroups, ins, offs, u);
}

template <int K>
static void launch_kq_mfma(const qsv_handle* h, const Shard& s, uint64_t nbatch, const BitIns& ins,
                           const KqOffs& offs, const double* ur, const double* ui) {
  // every wave keeps U in registers; give each at least ~8 batches to amortise loading it
  // option kq_grid (a diagnostic, 0 = none): no launch below takes more workgroups than that -- which wave gets which batch changes, nothing else
  const uint64_t cap = h->opt_kq_grid > 0 ? (uint64_t)h->opt_kq_grid : ~0ull;
  const uint64_t blocks = std::min(cap, std::max<uint64_t>(1, std::min<uint64_t>((nbatch + 31) / 32, (uint64_t)s.n_cu * (h->opt_kq_blocks_per_cu > 0 ? h->opt_kq_blocks_per_cu : 64))));
  const bool nt = single_nt(h, ins.n ? ins.pos[0] : 0);     // lowest target bit: inside a 128-byte line it loses (kq5 on bits 0..4: 0.60 -> 0.54)
  const dim3 g((unsigned)blocks), b(QSV_TPB);
#define QSV_KQ_GO(KERNEL) hipLaunchKernelGGL(KERNEL, g, b, 0, s.stream, s.amp, nbatch, ins, offs, ur, ui, h->opt_kq_chunked)
  // -1 (default): by K -- the 32-group-wide kernel at K = 4 (63 + 48 registers, four waves per SIMD: 0.75-0.77 against 0.70), the
  // 16-group one with prefetch and LDS fragments at K = 5 (the wide one holds two batches of 32 rows: two waves, no prefetch: 0.63-0.71 either way)
  // ... and at K = 5 the LDS-staged one (8) when a target sits inside a 128-byte line: the operand layout would then ask for pieces
  // of lines (targets 0..4: 0.60-0.64 -> 0.64-0.65; targets 1, 6, 11, 17, 27: 0.71 -> 0.73-0.75); with whole lines either way it loses (0.62-0.65 against 0.66-0.68)
  // (K = 4 -- which K = 3 on low targets is padded to -- with a target inside a line: the LDS-staged one too, 0.65 -> 0.74, r03l_kq_grid.log)
  const bool subline = ins.n && ins.pos[0] < 3;
  const int variant = h->opt_kq_variant >= 0 ? h->opt_kq_variant : (K == 4 ? (subline ? 6 : 5) : (subline ? 8 : 3));
  if (variant >= 6 && variant <= 8) {                       // 6..8: the batch staged through LDS, loads and stores in memory order; 1, 2, 3 batches of loads in flight per wave
    constexpr int D = 1 << K;
    // the K + 4 index bits of a batch element (4 group bits, K row bits), by the address bit each one is
    struct EB { int pos; uint64_t g; uint32_t l; };
    std::vector<EB> eb;
    for (int c = 0; c < 4; ++c) {
      const uint64_t g = ins_bits(1ull << c, ins);
      eb.push_back({__builtin_ctzll(g), g, 16u << c});
    }
    for (int j = 1, a = 0; j < D; j <<= 1, ++a) eb.push_back({__builtin_ctzll(offs.off[j]), offs.off[j], (uint32_t)QSV_KQ_LDS_RS << a});
    std::sort(eb.begin(), eb.end(), [](const EB& x, const EB& y) { return x.pos < y.pos; });
    KqLds lay;
    memset(&lay, 0, sizeof lay);
    lay.swap_lo = -1;
    // the sixth lane bit: address bit 11 where that can be had (a wave access is then two 512-byte runs 32 KiB apart, the
    // shape that streams best on this chip, DESIGN.md 3b) -- as one of the batch's own index bits, or in exchange for the
    // group bit that would have been sixth (a relabelling of the batches: bit 11 of the batch number takes its place)
    if ((h->opt_swz == 2 || (h->opt_swz == 1 && h->L >= 26)) && h->L >= 14 && eb[5].pos < 11) {
      int at11 = -1;
      for (int e = 6; e < K + 4; ++e) if (eb[e].pos == 11) at11 = e;
      bool target11 = false;
      for (int t = 0; t < ins.n; ++t) target11 |= ins.pos[t] == 11;
      if (at11 >= 0) std::swap(eb[5], eb[at11]);
      else if (!target11 && eb[5].l < (uint32_t)QSV_KQ_LDS_RS && eb[5].pos >= 5) {   // (a group bit: its image offset is a column)
        lay.swap_lo = eb[5].pos;
        eb[5].g = 1ull << 11;
      }
      std::sort(eb.begin() + 6, eb.end(), [](const EB& x, const EB& y) { return x.pos < y.pos; });
    }
    for (int n = 0; n < 6; ++n) { lay.lane_goff[n] = eb[n].g; lay.lane_loff[n] = eb[n].l; }
    for (int i = 0; i < D / 4; ++i)
      for (int m = 0; m < K - 2; ++m)
        if ((i >> m) & 1) { lay.goff_i[i] |= eb[6 + m].g; lay.loff_i[i] += eb[6 + m].l; }
    const bool ntl = single_nt(h, 12);                      // whole lines both ways whatever the targets: the size rule alone decides
    const int bpc = h->opt_kq_blocks_per_cu > 0 ? h->opt_kq_blocks_per_cu : (K == 4 ? 64 : 8);   // K = 4: small images, many workgroups per CU: 0.67 -> 0.74 on targets 1..3
#define QSV_KQ_LDS_GO(NW, DBG, PD) do { \
      const size_t shm = (DBG) == 3 ? 0 : (size_t)D / 16 * (D / 4) * 3 * 64 * sizeof(double) + (size_t)(NW) * D * QSV_KQ_LDS_RS; \
      const uint64_t want = (nbatch + (NW) * 16 - 1) / ((NW) * 16); \
      const dim3 gl((unsigned)std::min(cap, std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)s.n_cu * bpc)))); \
      if (shm > 64 * 1024) { \
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kq_lds<K, true, NW, DBG, PD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kq_lds<K, false, NW, DBG, PD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
      } \
      if (ntl) hipLaunchKernelGGL((k_kq_lds<K, true, NW, DBG, PD>), gl, dim3((NW) * 64), shm, s.stream, s.amp, nbatch, ins, lay, ur, ui); \
      else     hipLaunchKernelGGL((k_kq_lds<K, false, NW, DBG, PD>), gl, dim3((NW) * 64), shm, s.stream, s.amp, nbatch, ins, lay, ur, ui); \
    } while (0)
    // measurement only (scripts/kq_variants.py): kq_debug 1 / 2 = the kernel without its products / without its memory traffic
    if (variant == 6) {
      if (h->opt_kq_debug == 1) QSV_KQ_LDS_GO((K == 5 ? 6 : 4), 1, 1);
      else if (h->opt_kq_debug == 2) QSV_KQ_LDS_GO((K == 5 ? 6 : 4), 2, 1);
      else if (h->opt_kq_debug == 3) QSV_KQ_LDS_GO((K == 5 ? 6 : 4), 3, 1);
      else QSV_KQ_LDS_GO((K == 5 ? 6 : 4), 0, 1);
    } else if (variant == 7) {
      if (h->opt_kq_debug == 1) QSV_KQ_LDS_GO(4, 1, 2); else QSV_KQ_LDS_GO(4, 0, 2);
    } else {
      if (h->opt_kq_debug == 1) QSV_KQ_LDS_GO(4, 1, 3); else if (h->opt_kq_debug == 3) QSV_KQ_LDS_GO(4, 3, 3); else QSV_KQ_LDS_GO(4, 0, 3);
    }
#undef QSV_KQ_LDS_GO
    return;
  }
  if (variant == 5 && nbatch % 2 == 0) {                    // 5: two batches per step, 32 groups wide (two 512-byte runs per wave access)
    const size_t shm = (size_t)(1 << K) / 16 * ((1 << K) / 4) * 3 * 64 * sizeof(double);
    const uint64_t nsteps = nbatch / 2;
    const dim3 gw((unsigned)std::min(cap, std::max<uint64_t>(1, std::min<uint64_t>((nsteps + 15) / 16, (uint64_t)s.n_cu * (h->opt_kq_blocks_per_cu > 0 ? h->opt_kq_blocks_per_cu : 64)))));
    if (nt) hipLaunchKernelGGL((k_kq_mfma3w<K, true>), gw, b, shm, s.stream, s.amp, nsteps, ins, offs, ur, ui);
    else    hipLaunchKernelGGL((k_kq_mfma3w<K, false>), gw, b, shm, s.stream, s.amp, nsteps, ins, offs, ur, ui);
    return;
  }
  switch (variant == 5 ? 3 : variant) {                     // 0: four real products per complex one | 1: three (Gauss) | 2: three + next batch prefetched
    case 0:  if (nt) QSV_KQ_GO((k_kq_mfma<K, true>)); else QSV_KQ_GO((k_kq_mfma<K, false>)); break;
    case 1:  if (nt) QSV_KQ_GO((k_kq_mfma3<K, true, false>)); else QSV_KQ_GO((k_kq_mfma3<K, false, false>)); break;
    case 2:  if (nt) QSV_KQ_GO((k_kq_mfma3<K, true, true>)); else QSV_KQ_GO((k_kq_mfma3<K, false, true>)); break;
    default: {                                              // 3: as 2 with the A fragments in LDS (three waves per SIMD at K = 5); 4: as 1 with them in LDS (four)
      const size_t shm = (size_t)(1 << K) / 16 * ((1 << K) / 4) * 3 * 64 * sizeof(double);
#define QSV_KQ_GO_L(KERNEL) hipLaunchKernelGGL(KERNEL, g, b, shm, s.stream, s.amp, nbatch, ins, offs, ur, ui, h->opt_kq_chunked)
      if (variant != 4) { if (nt) QSV_KQ_GO_L((k_kq_mfma3<K, true, true, true>)); else QSV_KQ_GO_L((k_kq_mfma3<K, false, true, true>)); }
      else                        { if (nt) QSV_KQ_GO_L((k_kq_mfma3<K, true, false, true>)); else QSV_KQ_GO_L((k_kq_mfma3<K, false, false, true>)); }
#undef QSV_KQ_GO_L
    }
  }
#undef QSV_KQ_GO
}

template <int K>
static void launch_kq_tile(const qsv_handle* h, const Shard& s, uint64_t ngroups, const BitIns& ins,
                           const KqOffs& offs, const cplx* u, uint64_t special) {
  const size_t shm = sizeof(cplx) << (2 * K);
  const unsigned blocks = (unsigned)((ngroups + QSV_TPB - 1) / QSV_TPB);
  const int swz = skip_swz(h, special);                      // groups are enumerated with the targets left out
  if (single_nt(h, ins.n ? ins.pos[0] : 0))
    hipLaunchKernelGGL((k_kq_tile<K, true>), dim3(blocks), dim3(QSV_TPB), shm, s.stream, s.amp, ngroups, ins, offs, u, swz);
  else
    hipLaunchKernelGGL((k_kq_tile<K, false>), dim3(blocks), dim3(QSV_TPB), shm, s.stream, s.amp, ngroups, ins, offs, u, swz);
}

extern "C" int qsv_apply_kq(qsv_handle* h, int k, const int* qubits, const double* u) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  if (k < 1 || k > QSV_MAX_KQ || !qubits || !u) return fail(QSV_E_BADARG, "kq needs 1..%d qubits and a matrix", QSV_MAX_KQ);
  CHK(check_distinct(h, k, qubits, -1));
  for (int b = 0; b < k; ++b)
    if (qubits[b] >= h->L)
      return fail(QSV_E_UNSUPPORTED, "qubit %d of a dense gate is a shard bit (local qubits: %d); qsv_swap_layout it first", qubits[b], h->L);
  if (h->L < k) return fail(QSV_E_BADARG, "dense %d-qubit gate on %d local qubits", k, h->L);
  CHK(materialize_all(h));
  const uint64_t n = amps_local(h);

  // matrix-core path: K = 4, 5 natively; K = 3 embedded as I (x) U on one extra (free) qubit
  const int km = k >= 4 ? k : 4;
  // K = 3 is 2 flop/B: the vector units carry it as a plain stream (k_kq_tile); the matrix cores take K = 4, 5
  int lowest = 64;
  for (int b = 0; b < k; ++b) lowest = std::min(lowest, qubits[b]);
  // ... when no target sits inside a 128-byte line (a thread's 8 amplitudes would be 16-byte pieces of 8 lines: 0.57 against 0.63)
  const bool tile3 = k == 3 && (h->opt_kq3_tile > 1 || (h->opt_kq3_tile == 1 && lowest >= 3)) && (n >> 3) < (1ull << 40);
  if (h->opt_kq_mfma && k >= 3 && !tile3 && h->L - km >= 4) {
    std::vector<int> q(qubits, qubits + k);
    if (k == 3)                                            // pad with a HIGH free bit: low bits stay batch bits (coalescing)
      for (int b = h->L - 1; b >= 0; --b)
        if (std::find(q.begin(), q.end(), b) == q.end()) { q.push_back(b); break; }
    const int D = 1 << km, d = 1 << k;
    // Which target is index bit 0, 1, ... of the matrix is the kernels' access pattern (the operand layouts put index bits
    // 0 and 1 -- the wide kernel bit 0 -- on the lanes, i.e. decide how far apart the runs of one wave access lie), not
    // the caller's business: kq_order 1 (default) makes a target on address bit 11 index bit 0 (the two runs of a wide wave
    // access then lie 32 KiB apart, DESIGN.md 3b: K = 4 on bits 8..11 0.75 -> 0.81; no other distance gains anything),
    // 2 ascending, 3 descending, 4 nearest bit 11 first, 0 as given; the matrix is re-indexed to match.
    std::vector<int> perm(km);
    for (int b = 0; b < km; ++b) perm[b] = b;
    if (h->opt_kq_order == 1) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return (q[a] == 11) > (q[b] == 11); });
    else if (h->opt_kq_order == 4) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return std::abs(q[a] - 11) < std::abs(q[b] - 11); });
    else if (h->opt_kq_order == 2) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return q[a] < q[b]; });
    else if (h->opt_kq_order == 3) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return q[a] > q[b]; });
    auto old_index = [&](int x) { int y = 0; for (int b = 0; b < km; ++b) if ((x >> b) & 1) y |= 1 << perm[b]; return y; };
    {
      std::vector<int> q2(km);
      for (int b = 0; b < km; ++b) q2[b] = q[perm[b]];
      q = q2;
    }
    std::vector<double> ri(2 * (size_t)D * D, 0.0);       // Ur then Ui, row-major D x D
    for (int r2 = 0; r2 < D; ++r2)
      for (int c2 = 0; c2 < D; ++c2) {
        const int r = old_index(r2), c = old_index(c2);
        if ((r >> k) != (c >> k)) continue;                // block diagonal in the padding bit
        const double* e = u + 2 * ((size_t)(r & (d - 1)) * d + (c & (d - 1)));
        ri[(size_t)r2 * D + c2] = e[0];
        ri[(size_t)D * D + (size_t)r2 * D + c2] = e[1];
      }
    KqOffs offs;
    memset(&offs, 0, sizeof offs);
    for (int j = 0; j < D; ++j)
      for (int b = 0; b < km; ++b)
        if ((j >> b) & 1) offs.off[j] |= 1ull << q[b];
    const BitIns ins = make_ins(q);
    const uint64_t nbatch = (n >> km) / 16;
    for (Shard& s : h->shards) {
      CHK(shard_set(s));
      void* dtab = nullptr;
      CHK(arena_put(s, ri.data(), ri.size() * sizeof(double), &dtab));
      const double* ur = reinterpret_cast<const double*>(dtab);
      const double* ui = ur + (size_t)D * D;
      CHK(launch(h, s, QSV_K_KQ, 32.0 * (double)n, [&] {
        if (km == 4) launch_kq_mfma<4>(h, s, nbatch, ins, offs, ur, ui);
        else         launch_kq_mfma<5>(h, s, nbatch, ins, offs, ur, ui);
      }));
    }
    return QSV_OK;
  }

  const uint64_t ngroups = n >> k;
  KqOffs offs;
  memset(&offs, 0, sizeof offs);
  for (int j = 0; j < (1 << k); ++j)
    for (int b = 0; b < k; ++b)
      if ((j >> b) & 1) offs.off[j] |= 1ull << qubits[b];
  const BitIns ins = make_ins(std::vector<int>(qubits, qubits + k));
  for (Shard& s : h->shards) {
    CHK(shard_set(s));
    void* dtab = nullptr;
    CHK(arena_put(s, u, sizeof(double) * 2 << (2 * k), &dtab));
    const cplx* up = reinterpret_cast<const cplx*>(dtab);
    CHK(launch(h, s, QSV_K_KQ, 32.0 * (double)n, [&] {
      uint64_t special = 0;
      for (int b = 0; b < k; ++b) special |= 1ull << qubits[b];
      switch (k) {
        case 1: launch_kq<1>(h, s, ngroups, ins, offs, up); break;
        case 2: launch_kq<2>(h, s, ngroups, ins, offs, up); break;
        case 3: if (tile3) launch_kq_tile<3>(h, s, ngroups, ins, offs, up, special); else launch_kq<3>(h, s, ngroups, ins, offs, up); break;
        case 4: launch_kq<4>(h, s, ngroups, ins, offs, up); break;
        default: launch_kq<5>(h, s, ngroups, ins, offs, up); break;
      }
    }));
  }
  return QSV_OK;
}

// ------------------------------------------------------------------------------------------
// layout swaps and the shard-bit exchange
// ------------------------------------------------------------------------------------------
static int ensure_xbuf(qsv_handle* h, Shard& s, uint64_t amps) {
  if (s.xbuf_amps >= amps) return QSV_OK;
  CHK(shard_set(s));
  for (int b = 0; b < 2; ++b) {
    if (s.xbuf[b]) { HIPCHK(hipFree(s.xbuf[b])); s.xbuf[b] = nullptr; }
    HIPCHK(hipMalloc(&s.xbuf[b], amps * sizeof(cplx)));
  }
  s.xbuf_amps = amps;
  return QSV_OK;
}

static int swap_local(qsv_handle* h, int a, int b) {
  if (a > b) std::swap(a, b);
  const uint64_t n = amps_local(h);
  const uint64_t nq = n >> 2;
  const BitIns ins = make_ins({a, b});
  for (Shard& s : h->shards) {
    CHK(shard_set(s));
    CHK(launch(h, s, QSV_K_SWAP, 32.0 * (double)(n >> 1), [&] {
      hipLaunchKernelGGL(k_swap_bits, dim3(grid_for(h, s, nq, QSV_TPB * 2)), dim3(QSV_TPB), 0, s.stream,
                         s.amp, nq, ins, 1ull << a, 1ull << b, a >= 6 ? single_swz(h, (1ull << a) | (1ull << b)) : 0);     // (a < b) below bit 6 a wave access is not one run anyway: measured -3 %
    }));
  }
  return QSV_OK;
}

// ------------------------------------------------------------------------------------------
// Batched exchange: k shard bits G[i] <-> k local bits J[i] in one step.  Shard s keeps the block of
// its local index space whose J-bits spell its own G-bit values U(s) and swaps every other block B
// with the shard whose G-bits spell B (which holds it as ITS block U(s)): an all-to-all inside each
// group of 2^k shards -- (2^k - 1) / 2^k of a shard leaves over 2^k - 1 links at once, instead of k
// sequential half-shard exchanges over one link each.  k = 1 is the pairwise half-shard exchange.
// ------------------------------------------------------------------------------------------
struct XferPeer { int shard; uint64_t send_fixed, recv_fixed; };   // blocks as deposits into the J bits

static uint64_t deposit_bits(unsigned v, const std::vector<int>& pos) {
  uint64_t m = 0;
  for (size_t i = 0; i < pos.size(); ++i) if ((v >> i) & 1u) m |= 1ull << pos[i];
  return m;
}
static unsigned shard_group_value(int shard, const std::vector<int>& gb) {
  unsigned u = 0;
  for (size_t i = 0; i < gb.size(); ++i) u |= (unsigned)((shard >> gb[i]) & 1) << i;
  return u;
}
static int shard_with_group_value(int shard, const std::vector<int>& gb, unsigned v) {
  for (size_t i = 0; i < gb.size(); ++i) shard = (shard & ~(1 << gb[i])) | (int)((v >> i) & 1u) << gb[i];
  return shard;
}

static int ensure_xstage(qsv_handle* h, Shard& s, uint64_t amps) {
  CHK(shard_set(s));
  if (!s.xstream) {
    HIPCHK(hipStreamCreateWithFlags(&s.xstream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIPCHK(hipEventCreateWithFlags(&s.ev_packed[b], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&s.ev_sent[b], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&s.ev_unpacked[b], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&s.ev_start, hipEventDisableTiming));
  }
  if (s.xstage_amps >= amps) return QSV_OK;
  for (int b = 0; b < 2; ++b) {
    if (s.xsend[b]) { HIPCHK(hipFree(s.xsend[b])); s.xsend[b] = nullptr; }
    if (s.xrecv[b]) { HIPCHK(hipFree(s.xrecv[b])); s.xrecv[b] = nullptr; }
    HIPCHK(hipMalloc(&s.xsend[b], amps * sizeof(cplx)));
    HIPCHK(hipMalloc(&s.xrecv[b], amps * sizeof(cplx)));
  }
  s.xstage_amps = amps;
  return QSV_OK;
}

// RCCL transport of one shard's side of a batched exchange: per chunk of the block index space,
// pack the chunk of every outgoing block into its peer's segment of a send slot, ONE grouped
// ncclSend/ncclRecv with all peers, unpack.  Double buffered: pack of chunk c + 1 and unpack of
// chunk c - 1 run on the shard's second stream while chunk c is on the wire.
static int rccl_block_exchange(qsv_handle* h, Shard& s, const BitIns& ins, uint64_t nblock, const std::vector<XferPeer>& peers) {
  const size_t np = peers.size();
  uint64_t chunk = std::min<uint64_t>(nblock, h->opt_xchunk);
  // staging = 4 slots x peers x chunk: keep it under an eighth of the shard
  while (chunk > 4096 && 4ull * np * chunk > (amps_local(h) >> 3)) chunk >>= 1;
  CHK(ensure_xstage(h, s, (uint64_t)np * chunk));
  const uint64_t nchunks = (nblock + chunk - 1) / chunk;
  hipStream_t mainst = s.stream, aux = s.xstream;
  auto cnt_of = [&](uint64_t c) { return std::min<uint64_t>(chunk, nblock - c * chunk); };
  auto pack = [&](uint64_t c) -> int {
    const int b = (int)(c & 1);
    if (c >= 2) HIPCHK(hipStreamWaitEvent(aux, s.ev_sent[b], 0));            // send slot b is free again
    const uint64_t cnt = cnt_of(c);
    for (size_t pi = 0; pi < np; ++pi)
      hipLaunchKernelGGL(k_pack_block, dim3(grid_for(h, s, cnt, QSV_TPB * 2)), dim3(QSV_TPB), 0, aux, s.amp,
                         s.xsend[b] + pi * chunk, c * chunk, cnt, ins, peers[pi].send_fixed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev_packed[b], aux));
    return QSV_OK;
  };
  HIPCHK(hipEventRecord(s.ev_start, mainst));                                  // the state is final before anything is packed
  HIPCHK(hipStreamWaitEvent(aux, s.ev_start, 0));
  CHK(pack(0));
  for (uint64_t c = 0; c < nchunks; ++c) {
    const int b = (int)(c & 1);
    const uint64_t cnt = cnt_of(c);
    HIPCHK(hipStreamWaitEvent(mainst, s.ev_packed[b], 0));
    if (c >= 2) HIPCHK(hipStreamWaitEvent(mainst, s.ev_unpacked[b], 0));      // recv slot b has been consumed
    NCCLCHK(g_rccl.GroupStart());
    for (size_t pi = 0; pi < np; ++pi) {
      NCCLCHK(g_rccl.Send(s.xsend[b] + pi * chunk, cnt * 2, ncclDouble, peers[pi].shard, h->comm, mainst));
      NCCLCHK(g_rccl.Recv(s.xrecv[b] + pi * chunk, cnt * 2, ncclDouble, peers[pi].shard, h->comm, mainst));
    }
    NCCLCHK(g_rccl.GroupEnd());
    HIPCHK(hipEventRecord(s.ev_sent[b], mainst));
    if (c + 1 < nchunks) CHK(pack(c + 1));                                    // overlaps the transfer just queued
    HIPCHK(hipStreamWaitEvent(aux, s.ev_sent[b], 0));
    for (size_t pi = 0; pi < np; ++pi)
      hipLaunchKernelGGL(k_unpack_block, dim3(grid_for(h, s, cnt, QSV_TPB * 2)), dim3(QSV_TPB), 0, aux, s.amp,
                         s.xrecv[b] + pi * chunk, c * chunk, cnt, ins, peers[pi].recv_fixed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev_unpacked[b], aux));
    h->stats.exchange_bytes += (double)np * (double)cnt * sizeof(cplx);
  }
  // whatever follows on the main stream sees the exchanged state
  HIPCHK(hipStreamWaitEvent(mainst, s.ev_unpacked[(nchunks - 1) & 1], 0));
  if (nchunks >= 2) HIPCHK(hipStreamWaitEvent(mainst, s.ev_unpacked[(nchunks - 2) & 1], 0));
  return QSV_OK;
}

static int exchange_multi(qsv_handle* h, const std::vector<int>& G, const std::vector<int>& J) {
  // every cached reduction describes the state BEFORE the swap: block sums, the per-tile sums a
  // program's last pass left and their host copy
  for (Shard& s : h->shards) { s.sums_valid = false; s.tile_valid = false; s.h_tsums_valid = false; s.d_super_valid = 0; }
  const int k = (int)G.size();
  std::vector<int> gb(k);
  for (int i = 0; i < k; ++i) gb[i] = G[i] - h->L;
  // `ins` holds the J positions sorted; block values are deposited at the positions in PAIR order
  const BitIns ins = make_ins(J);
  const uint64_t n = amps_local(h);
  const uint64_t nblock = n >> k;
  const unsigned ngroup = 1u << k;
  // in-place block swaps are read+write streams like the gate sweeps: same index swizzle, when every swapped
  // bit is above the lane bits and neither is bit 5 or 11 (the same decision on every rank: it depends on the call only)
  uint64_t jmask = 0;
  int jmin = 64;
  for (int q : J) { jmask |= 1ull << q; jmin = std::min(jmin, q); }
  const int xswz = jmin >= 6 ? single_swz(h, jmask) : 0;
  h->stats.exchanges += 1;
  if (!h->multiproc) {
    // every shard lives in this process: one in-place swap kernel per unordered pair of a group
    bool one_device = true;
    for (Shard& s : h->shards) if (s.device != h->shards[0].device) one_device = false;
    if (!one_device) return fail(QSV_E_UNSUPPORTED, "batched exchange between devices of one process");
    CHK(qsv_sync(h));
    for (Shard& A : h->shards) {
      const unsigned ua = shard_group_value(A.index, gb);
      for (unsigned ub = ua + 1; ub < ngroup; ++ub) {
        Shard& B = h->shards[shard_with_group_value(A.index, gb, ub)];
        CHK(shard_set(A));
        CHK(launch(h, A, QSV_K_EXCHANGE, 32.0 * (double)nblock, [&] {
          hipLaunchKernelGGL(k_swap_blocks, dim3(grid_for(h, A, nblock, QSV_TPB * 2)), dim3(QSV_TPB), 0, A.stream,
                             A.amp, B.amp, 0ull, nblock, ins, deposit_bits(ub, J), deposit_bits(ua, J), xswz);
        }));
      }
    }
    CHK(qsv_sync(h));
    return QSV_OK;
  }
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  const unsigned me = shard_group_value(s.index, gb);
  std::vector<XferPeer> peers;
  std::vector<int> peer_ranks;
  for (unsigned v = 0; v < ngroup; ++v) {
    if (v == me) continue;
    const int p = shard_with_group_value(s.index, gb, v);
    peers.push_back({p, deposit_bits(v, J), deposit_bits(v, J)});      // my block v <-> its block `me`
    peer_ranks.push_back(p);
  }
  if (!h->peer_amp.empty()) {
    // peer-mapped transport: every pair swaps in place, each rank its half of the pair's block.
    // The group synchronises before (all states final, streams idle) and after (all halves written).
    HIPCHK(hipStreamSynchronize(s.stream));
    CHK(ipc_group_barrier(h, peer_ranks));
    const uint64_t half = nblock >> 1;
    double moved = 0;
    for (const XferPeer& xp : peers) {
      const unsigned v = shard_group_value(xp.shard, gb);
      const bool low = me < v;
      const uint64_t p0 = low ? 0 : half, cnt = low ? half : nblock - half;
      if (!cnt) continue;
      cplx* peer = h->peer_amp[xp.shard];
      CHK(launch(h, s, QSV_K_EXCHANGE, 32.0 * (double)cnt, [&] {
        hipLaunchKernelGGL(k_swap_blocks, dim3(grid_for(h, s, cnt, QSV_TPB * 2)), dim3(QSV_TPB), 0, s.stream,
                           s.amp, peer, p0, cnt, ins, deposit_bits(v, J), deposit_bits(me, J), xswz);
      }));
      moved += 32.0 * (double)cnt;
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    CHK(ipc_group_barrier(h, peer_ranks));
    h->stats.exchange_bytes += moved;
    return QSV_OK;
  }
  if (!h->comm) return fail(QSV_E_RCCL, "exchange needs qsv_comm_init (RCCL) or qsv_ipc_attach on every rank first");
  Pending p{QSV_K_EXCHANGE, nullptr, nullptr};
  if (h->profiling) { CHK(get_event(s, &p.e0)); CHK(get_event(s, &p.e1)); HIPCHK(hipEventRecord(p.e0, s.stream)); }
  CHK(rccl_block_exchange(h, s, ins, nblock, peers));
  if (h->profiling) { HIPCHK(hipEventRecord(p.e1, s.stream)); s.pending.push_back(p); }
  h->stats.per_kind[QSV_K_EXCHANGE].launches += 1;
  h->stats.per_kind[QSV_K_EXCHANGE].algorithmic_bytes += 32.0 * (double)nblock * (double)peers.size();
  return QSV_OK;
}

// swap shard bit G (>= L) with local bit j between two DEVICES driven by this one process (peer
// copies through staging buffers); every other configuration goes through exchange_multi
static int exchange_peer_copy(qsv_handle* h, int G, int j) {
  for (Shard& s : h->shards) { s.sums_valid = false; s.tile_valid = false; s.h_tsums_valid = false; s.d_super_valid = 0; }
  const int gb = G - h->L;
  const uint64_t n = amps_local(h);
  const uint64_t nhalf = n >> 1;
  h->stats.exchanges += 1;
  for (Shard& A : h->shards) {
    if ((A.index >> gb) & 1) continue;
    Shard& B = h->shards[A.index | (1 << gb)];
    if (A.device == B.device) {
      CHK(shard_set(A));
      HIPCHK(hipStreamSynchronize(B.stream));
      CHK(launch(h, A, QSV_K_EXCHANGE, 32.0 * (double)n, [&] {
        hipLaunchKernelGGL(k_swap_shards, dim3(grid_for(h, A, nhalf, QSV_TPB * 2)), dim3(QSV_TPB), 0, A.stream,
                           A.amp, B.amp, nhalf, j);
      }));
      HIPCHK(hipStreamSynchronize(A.stream));
      continue;
    }
    const uint64_t chunk = std::min<uint64_t>(nhalf, h->opt_xchunk);
    CHK(ensure_xbuf(h, A, chunk));
    CHK(ensure_xbuf(h, B, chunk));
    for (uint64_t p0 = 0; p0 < nhalf; p0 += chunk) {
      CHK(shard_set(A));
      hipLaunchKernelGGL(k_pack, dim3(grid_for(h, A, chunk, QSV_TPB * 2)), dim3(QSV_TPB), 0, A.stream, A.amp, A.xbuf[0], p0, chunk, j, 1);
      HIPCHK(hipGetLastError());
      CHK(shard_set(B));
      hipLaunchKernelGGL(k_pack, dim3(grid_for(h, B, chunk, QSV_TPB * 2)), dim3(QSV_TPB), 0, B.stream, B.amp, B.xbuf[0], p0, chunk, j, 0);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(B.stream));
      CHK(shard_set(A));
      HIPCHK(hipStreamSynchronize(A.stream));
      HIPCHK(hipMemcpyPeer(B.xbuf[1], B.device, A.xbuf[0], A.device, chunk * sizeof(cplx)));
      HIPCHK(hipMemcpyPeer(A.xbuf[1], A.device, B.xbuf[0], B.device, chunk * sizeof(cplx)));
      hipLaunchKernelGGL(k_unpack, dim3(grid_for(h, A, chunk, QSV_TPB * 2)), dim3(QSV_TPB), 0, A.stream, A.amp, A.xbuf[1], p0, chunk, j, 1);
      HIPCHK(hipGetLastError());
      CHK(shard_set(B));
      hipLaunchKernelGGL(k_unpack, dim3(grid_for(h, B, chunk, QSV_TPB * 2)), dim3(QSV_TPB), 0, B.stream, B.amp, B.xbuf[1], p0, chunk, j, 0);
      HIPCHK(hipGetLastError());
      h->stats.exchange_bytes += 2.0 * (double)chunk * sizeof(cplx);
    }
    HIPCHK(hipStreamSynchronize(B.stream));
    CHK(shard_set(A));
    HIPCHK(hipStreamSynchronize(A.stream));
    h->stats.per_kind[QSV_K_EXCHANGE].launches += 1;
    h->stats.per_kind[QSV_K_EXCHANGE].algorithmic_bytes += 32.0 * (double)n;
  }
  return QSV_OK;
}

static bool one_process_several_devices(const qsv_handle* h) {
  if (h->multiproc) return false;
  for (const Shard& s : h->shards) if (s.device != h->shards[0].device) return true;
  return false;
}

extern "C" int qsv_swap_layout(qsv_handle* h, int npairs, const int* a, const int* b) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  if (npairs < 0 || (npairs && (!a || !b))) return fail(QSV_E_BADARG, "bad swap list");
  uint64_t seen = 0;
  bool disjoint = true;
  for (int i = 0; i < npairs; ++i) {
    CHK(check_qubit(h, a[i], "swap"));
    CHK(check_qubit(h, b[i], "swap"));
    if (a[i] == b[i]) continue;
    if ((seen >> a[i]) & 1ull || (seen >> b[i]) & 1ull) disjoint = false;
    seen |= (1ull << a[i]) | (1ull << b[i]);
    if (std::min(a[i], b[i]) >= h->L)
      return fail(QSV_E_UNSUPPORTED, "swap of two shard bits (%d,%d) is not implemented; route through a local bit", a[i], b[i]);
  }
  // a local swap reads every amplitude, and an exchange partner must never read undefined memory
  CHK(materialize_all(h));
  // pairs that touch distinct qubits commute: the local ones run as permutation sweeps, ALL the
  // shard-bit ones as ONE batched exchange (an all-to-all inside each group of 2^k shards)
  std::vector<int> G, J;
  for (int i = 0; i < npairs; ++i) {
    if (a[i] == b[i]) continue;
    const int lo = std::min(a[i], b[i]), hi = std::max(a[i], b[i]);
    if (hi < h->L) { CHK(swap_local(h, lo, hi)); continue; }
    if (disjoint && !one_process_several_devices(h)) { G.push_back(hi); J.push_back(lo); continue; }
    if (one_process_several_devices(h)) CHK(exchange_peer_copy(h, hi, lo));
    else CHK(exchange_multi(h, std::vector<int>{hi}, std::vector<int>{lo}));
  }
  if (!G.empty()) CHK(exchange_multi(h, G, J));
  return QSV_OK;
}

// Diagnostic for a box with ONE GPU (RCCL refuses two ranks on a device): the complete RCCL side of
// a batched exchange -- staging, the two-stream double-buffered pipeline, grouped ncclSend/ncclRecv
// to several "peers" -- run on a 1-rank communicator with rank 0 as its own peer.  A 2^n_qubits
// shard is filled with amp[i] = (i, -i); blocks of the local bits {3, n_qubits - 2} are shipped
// 1 -> 2 and 2 -> 3 (send and receive blocks differ, so a pack that ran after the unpack of the same
// chunk, or a slot reused too early, shows up as wrong data), in chunks of 2^chunk_log2 amplitudes.
extern "C" int qsv_rccl_exchange_selftest(int device_id, int n_qubits, int chunk_log2) {
  if (n_qubits < 8 || n_qubits > 26) return fail(QSV_E_BADARG, "n_qubits must be 8..26");
  if (chunk_log2 < 4 || chunk_log2 > 30) return fail(QSV_E_BADARG, "chunk_log2 must be 4..30");
  CHK(rccl_load());
  qsv_handle* h = nullptr;
  CHK(qsv_create_rank(n_qubits, 1, 0, device_id, &h));
  int rc = QSV_OK;
  auto body = [&]() -> int {
    Shard& s = h->shards[0];
    CHK(shard_set(s));
    ncclUniqueId uid;
    NCCLCHK(g_rccl.GetUniqueId(&uid));
    StdoutToStderr quiet;
    NCCLCHK(g_rccl.CommInitRank(&h->comm, 1, uid, 0));
    h->opt_xchunk = 1ull << chunk_log2;
    const uint64_t n = amps_local(h);
    std::vector<double> host(2 * n);
    for (uint64_t i = 0; i < n; ++i) { host[2 * i] = (double)i; host[2 * i + 1] = -(double)i; }
    CHK(qsv_set_amplitudes(h, 0, n, host.data()));
    const std::vector<int> J{3, n_qubits - 2};
    const BitIns ins = make_ins(J);
    const std::vector<XferPeer> peers{{0, deposit_bits(1, J), deposit_bits(2, J)}, {0, deposit_bits(2, J), deposit_bits(3, J)}};
    CHK(rccl_block_exchange(h, s, ins, n >> 2, peers));
    HIPCHK(hipStreamSynchronize(s.stream));
    std::vector<double> got(2 * n);
    CHK(qsv_get_amplitudes(h, 0, n, got.data()));
    const uint64_t jm = deposit_bits(3, J);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t blk = i & jm, rest = i & ~jm;
      uint64_t src = i;
      if (blk == deposit_bits(2, J)) src = rest | deposit_bits(1, J);
      else if (blk == deposit_bits(3, J)) src = rest | deposit_bits(2, J);
      if (got[2 * i] != (double)src || got[2 * i + 1] != -(double)src)
        return fail(QSV_E_RCCL, "rccl exchange self-test: amplitude %llu holds (%g, %g), expected the old value of %llu",
                    (unsigned long long)i, got[2 * i], got[2 * i + 1], (unsigned long long)src);
    }
    return QSV_OK;
  };
  rc = body();
  qsv_destroy(h);
  return rc;
}
