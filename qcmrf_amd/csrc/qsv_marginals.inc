// qsv_marginals_cond (DESIGN §6): many marginals of the conditioned state from one load of each matching amplitude.
//
// The index space is the compact one of qsv_sample_cond (CondView): compact index j stands for the local address
// ins_bits(j, F) | val.  A compact block is QSV_SBLOCK = 4096 entries, compact bits 0..11, laid over a workgroup as
//     bits 0..5  lane        bits 6..7  wave        bits 8..11  u, the thread's 16 loads (j = block*4096 + u*256 + thread)
// A group qubit is one of: an "inner" bit (a free local bit whose compact position is below 12), a "block" bit (compact
// position 12 or more: the same for the whole block, taken from the block number), a fixed bit or a shard bit (the same
// for the whole shard: folded into MargGroup::base on the host).  Per block and group the 4096 values p = |amp|^2 are
// summed over the compact bits 0..11 that are NOT inner bits of the group.
//
// The tree of additions, a pure function of (shard contents, shard structure, groups, mask) -- no atomics anywhere:
//   1. registers: for t = 0..3, when u bit t is not in the group: v[u] += v[u | 1 << t] for every u with bit t clear;
//   2. lanes:     for t = 0..5, when lane bit t is not in the group: x += shfl_xor(x, 1 << t) (both partners form the same
//                 sum: addition commutes);
//   3. waves:     the four waves' values go through LDS (the staging area); one thread per inner bin adds the waves that
//                 agree with the bin's wave bits in ascending wave order, ((w0 + w1) + w2) + w3 when no wave bit is in
//                 the group;
//   4. blocks:    that thread adds the result to its bin of the chunk's row in LDS; a chunk is a fixed run of consecutive
//                 blocks (nchunks = min(number of blocks, 4096), blocks per chunk = their quotient: both powers of two),
//                 walked in ascending order.  Workgroup w takes chunks w, w + grid, ...: the grid decides who walks a
//                 chunk, never what is added to what.  A chunk's row is stored to part[chunk][bin];
//   5. chunks:    k_marginals_fold: runs of 64 rows added in ascending order, one thread per (run, bin); then the run
//                 totals added in ascending order by the same kernel, one thread per bin;
//   6. shards:    added on the host in shard order.
// The mass rides along as one more group without qubits.  A bin no matching amplitude falls into (one that contradicts a
// fixed bit) is never added to and stays +0.0.
// Steps 1-3 depend on a group's inner bits alone (smask), so groups with the same smask -- every group that lies on block,
// fixed and shard bits shares smask 0 with the mass -- share one staged result: the host sorts the groups by smask, the
// first group of a class (MARG_LEAD) computes and stages it, and classes are packed into batches whose staged values fit
// the staging area (MARG_BATCH_END closes one): one barrier per batch, not per group.  Which groups share a batch changes
// no addition: every bin still takes the tree above.
enum { MARG_LEAD = 1, MARG_BATCH_END = 2 };
struct MargGroup {
  uint32_t off;            // first bin of the group in a row
  uint32_t base;           // bin bits given by fixed and shard bits
  uint16_t smask;          // inner bits: compact positions below 12
  uint16_t stage_off;      // where the class's 2^n_in values sit in a wave's staging area
  uint8_t n_in, n_ent;     // entries [0, n_in) are inner bits, [n_in, n_ent) block bits; ascending compact position
  uint8_t flags, pad;      // MARG_LEAD | MARG_BATCH_END
  uint8_t cpos[QSV_MARG_MAX_K], bit[QSV_MARG_MAX_K];   // compact position -> bit of the bin number
};

template <bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_marginals_cond(const cplx* __restrict__ amp, uint64_t nc, BitIns fix, uint64_t val,
                                                            uint64_t zmask, const MargGroup* __restrict__ grp, int ngrp, int rowlen,
                                                            uint64_t nchunks, uint64_t bpc, double* __restrict__ part) {
  static_assert(QSV_TPB == 256 && QSV_SBLOCK == 4096, "the block layout above");
  extern __shared__ double row[];                          // rowlen bins of the chunk in hand
  __shared__ double stage[2][QSV_TPB / 64][1 << QSV_MARG_MAX_K];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  int buf = 0;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    for (int i = tid; i < rowlen; i += QSV_TPB) row[i] = 0.0;
    __syncthreads();
    for (uint64_t b = c * bpc; b < (c + 1) * bpc; ++b) {
      double p[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const uint64_t j = b * QSV_SBLOCK + (uint64_t)u * QSV_TPB + tid;
        p[u] = 0.0;
        if (j < nc) {
          const uint64_t i = ins_bits(j, fix) | val;
          if (!(i & zmask)) { const cplx a = NT ? ld_nt(amp + i) : amp[i]; p[u] = fma(a.x, a.x, a.y * a.y); }
        }
      }
      for (int g0 = 0; g0 < ngrp; buf ^= 1) {
        // a batch, first half: every class's sums over the bits outside it, staged per wave
        int g1 = g0;
        for (;; ++g1) {
          const MargGroup& G = grp[g1];
          if (G.flags & MARG_LEAD) {
            const uint32_t sm = G.smask, slane = sm & 63u, su = sm >> 8;
            const int nl = __builtin_popcount(slane);
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = p[u];
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (!((su >> t) & 1u)) {
#pragma unroll
                for (int u = 0; u < 16; ++u) if (!(u & (1 << t))) v[u] += v[u | (1 << t)];
              }
            uint32_t li = 0;                               // the lane's group bits, packed
            for (int t = 0, k = 0; t < 6; ++t) if ((slane >> t) & 1u) { li |= ((lane >> t) & 1u) << k; ++k; }
            const bool writer = (lane & ~slane) == 0;
            double* st = stage[buf][wave] + G.stage_off;
#pragma unroll
            for (int u = 0; u < 16; ++u)
              if (!((uint32_t)u & ~su)) {                  // workgroup-uniform: the u's that hold a sum after step 1
                double x = v[u];
#pragma unroll
                for (int t = 0; t < 6; ++t) if (!((slane >> t) & 1u)) x += __shfl_xor(x, 1 << t, 64);
                uint32_t ui = 0;
                for (int t = 0, k = 0; t < 4; ++t) if ((su >> t) & 1u) { ui |= (((uint32_t)u >> t) & 1u) << k; ++k; }
                if (writer) st[li | (ui << nl)] = x;
              }
          }
          if (G.flags & MARG_BATCH_END) break;
        }
        __syncthreads();
        // Two staging buffers taken in turn, across blocks and chunks too: a buffer is written again two batches later, after
        // the barrier of the batch in between, which every thread reaches only after it has read here.
        // second half: one thread per inner bin of every group of the batch; tid's bits are the entries [0, n_in)
        for (int g = g0; g <= g1; ++g) {
          const MargGroup& G = grp[g];
          if (tid < (1u << G.n_in)) {
            const uint32_t sm = G.smask, slane = sm & 63u, swave = (sm >> 6) & 3u;
            const int nl = __builtin_popcount(slane), nw = __builtin_popcount(swave);
            const uint32_t il = tid & ((1u << nl) - 1u), iw = (tid >> nl) & ((1u << nw) - 1u), iu = tid >> (nl + nw);
            uint32_t wsel = 0;
            for (int t = 0, k = 0; t < 2; ++t) if ((swave >> t) & 1u) { wsel |= ((iw >> k) & 1u) << t; ++k; }
            const uint32_t idx = G.stage_off + (il | (iu << nl));
            double s = 0.0;
            bool first = true;
            for (uint32_t w = 0; w < QSV_TPB / 64; ++w)
              if ((w & swave) == wsel) { s = first ? stage[buf][w][idx] : s + stage[buf][w][idx]; first = false; }
            uint32_t bin = G.base;
            for (int e = 0; e < G.n_in; ++e) bin |= ((tid >> e) & 1u) << G.bit[e];
            for (int e = G.n_in; e < G.n_ent; ++e) bin |= (uint32_t)((b >> (G.cpos[e] - 12)) & 1ull) << G.bit[e];
            row[G.off + bin] += s;                         // bins of one group are distinct per thread, groups do not share bins
          }
        }
        g0 = g1 + 1;
      }
    }
    __syncthreads();
    for (int i = tid; i < rowlen; i += QSV_TPB) part[c * (uint64_t)rowlen + i] = row[i];
    __syncthreads();
  }
}

// step 5 of the tree above: out[r][bin] = rows 64 r .. 64 r + 63 of `in` added in ascending order, r = blockIdx.y; launched
// once over the chunks' rows and, where there are more than 64 of them, once more over the run totals
__global__ __launch_bounds__(QSV_TPB) void k_marginals_fold(const double* __restrict__ in, uint64_t nrows, int rowlen,
                                                            double* __restrict__ out) {
  const int i = blockIdx.x * QSV_TPB + threadIdx.x;
  if (i >= rowlen) return;
  const uint64_t r0 = (uint64_t)blockIdx.y * 64;
  double s = 0.0;
  for (uint64_t r = r0; r < r0 + 64 && r < nrows; ++r) s += in[r * (uint64_t)rowlen + i];
  out[(uint64_t)blockIdx.y * (uint64_t)rowlen + i] = s;
}

extern "C" int qsv_marginals_cond(qsv_handle* h, int n_groups, const int* group_k, const int* qubits, uint64_t fix_mask,
                                  uint64_t fix_val, double* out, double* mass_out) {
  if (!h || !group_k || !out) return fail(QSV_E_BADARG, "NULL argument");
  if (n_groups < 1 || n_groups > QSV_MARG_MAX_GROUPS) return fail(QSV_E_BADARG, "%d groups, 1..%d supported", n_groups, QSV_MARG_MAX_GROUPS);
  int nbins = 0, nq = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (group_k[g] < 0 || group_k[g] > QSV_MARG_MAX_K) return fail(QSV_E_BADARG, "group %d has %d qubits, 0..%d supported", g, group_k[g], QSV_MARG_MAX_K);
    nbins += 1 << group_k[g];
    nq += group_k[g];
  }
  if (nbins > QSV_MARG_MAX_BINS) return fail(QSV_E_BADARG, "%d bins in %d groups, at most %d supported", nbins, n_groups, QSV_MARG_MAX_BINS);
  if (nq && !qubits) return fail(QSV_E_BADARG, "NULL argument");
  for (int g = 0, o = 0; g < n_groups; o += group_k[g], ++g) {
    uint64_t seen = 0;
    for (int b = 0; b < group_k[g]; ++b) {
      const int q = qubits[o + b];
      if (q < 0 || q >= h->W) return fail(QSV_E_BADARG, "group %d: qubit %d not in [0,%d)", g, q, h->W);
      if ((seen >> q) & 1ull) return fail(QSV_E_BADARG, "group %d: qubit %d repeated", g, q);
      seen |= 1ull << q;
    }
  }
  if (fix_val & ~fix_mask) return fail(QSV_E_BADARG, "fix_val has bits outside fix_mask");
  if (h->W < 64 && (fix_mask >> h->W)) return fail(QSV_E_BADARG, "fix_mask has bits at or above qubit %d", h->W);
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
  const uint64_t nblk = (cv.nc + QSV_SBLOCK - 1) / QSV_SBLOCK;     // a power of two
  const uint64_t nchunks = std::min<uint64_t>(nblk, 4096), bpc = nblk / nchunks;
  const int ngrp = n_groups + 1, rowlen = nbins + 1;               // the mass: one more group, without qubits
  std::vector<double> tot((size_t)rowlen, 0.0), got((size_t)rowlen);
  std::vector<MargGroup> mg((size_t)ngrp);
  for (Shard& s : h->shards) {
    // a fixed shard bit does not enter the kernels: a shard whose index disagrees with it holds no matching amplitude
    if ((((uint64_t)s.index << h->L) & fix_mask) != (fix_val & ~(n - 1))) continue;
    CHK(shard_set(s));
    if (s.deferred) {
      if (fix_mask) CHK(cond_prepare_deferred(h, s, lmask, lval));
      else CHK(realize(h, s));
    }
    for (int g = 0, o = 0, off = 0; g < ngrp; ++g) {
      MargGroup& G = mg[(size_t)g];
      const int k = g < n_groups ? group_k[g] : 0;
      memset(&G, 0, sizeof(G));
      G.off = (uint32_t)off;
      std::vector<std::pair<int, int>> ent;                        // (compact position, bit of the bin number)
      for (int b = 0; b < k; ++b) {
        const int q = qubits[o + b];
        if (q >= h->L) G.base |= (uint32_t)shard_bit(h, s, q) << b;
        else if ((lmask >> q) & 1ull) G.base |= (uint32_t)((lval >> q) & 1ull) << b;
        else ent.emplace_back(q - __builtin_popcountll(lmask & ((1ull << q) - 1ull)), b);
      }
      std::sort(ent.begin(), ent.end());
      G.n_ent = (uint8_t)ent.size();
      for (size_t e = 0; e < ent.size(); ++e) {
        G.cpos[e] = (uint8_t)ent[e].first;
        G.bit[e] = (uint8_t)ent[e].second;
        if (ent[e].first < 12) { G.smask |= (uint16_t)(1u << ent[e].first); G.n_in = (uint8_t)(e + 1); }
      }
      o += k;
      off += 1 << k;
    }
    // classes and batches (see above): the order of the groups in the kernel's list is free, G.off says where a group's bins go
    std::stable_sort(mg.begin(), mg.end(), [](const MargGroup& a, const MargGroup& b) { return a.smask < b.smask; });
    for (int g = 0, used = 0, at = 0; g < ngrp; ++g) {
      MargGroup& G = mg[(size_t)g];
      if (g == 0 || G.smask != mg[(size_t)g - 1].smask) {
        const int need = 1 << G.n_in;
        if (used + need > (1 << QSV_MARG_MAX_K)) { mg[(size_t)g - 1].flags |= MARG_BATCH_END; used = 0; }   // a batch ends only where a class does
        G.flags |= MARG_LEAD;
        at = used;
        used += need;
      }
      G.stage_off = (uint16_t)at;
    }
    mg[(size_t)ngrp - 1].flags |= MARG_BATCH_END;
    void* d_grp = nullptr;
    CHK(arena_put(s, mg.data(), mg.size() * sizeof(MargGroup), &d_grp));
    double* d_part = nullptr;
    bool temp = false;
    const uint64_t nruns = (nchunks + 63) / 64;                    // <= 64
    CHK(red_scratch(s, (size_t)(nchunks + nruns + 1) * (size_t)rowlen, &d_part, &temp));
    double* d_runs = d_part + (size_t)nchunks * (size_t)rowlen;
    double* d_row = nruns > 1 ? d_runs + (size_t)nruns * (size_t)rowlen : d_runs;
    CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)cv.nc, [&] {
      // every fixed bit at or above bit 12: a compact block is one contiguous 64 KiB run, streamed as k_blocksum does
      const bool nt = (cv.fix.n == 0 || cv.fix.pos[0] >= 12) && (h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26));
      uint64_t grid = std::min<uint64_t>(nchunks, (uint64_t)s.n_cu * 8);
      if (h->opt_marginals_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_marginals_grid);
      const size_t sh = (size_t)rowlen * sizeof(double);
      const MargGroup* dg = reinterpret_cast<const MargGroup*>(d_grp);
      if (nt) hipLaunchKernelGGL(k_marginals_cond<true>, dim3((unsigned)grid), dim3(QSV_TPB), sh, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, dg, ngrp, rowlen, nchunks, bpc, d_part);
      else hipLaunchKernelGGL(k_marginals_cond<false>, dim3((unsigned)grid), dim3(QSV_TPB), sh, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, dg, ngrp, rowlen, nchunks, bpc, d_part);
      const unsigned fx = (unsigned)((rowlen + QSV_TPB - 1) / QSV_TPB);
      hipLaunchKernelGGL(k_marginals_fold, dim3(fx, (unsigned)nruns), dim3(QSV_TPB), 0, s.stream, d_part, nchunks, rowlen, d_runs);
      if (nruns > 1) hipLaunchKernelGGL(k_marginals_fold, dim3(fx, 1), dim3(QSV_TPB), 0, s.stream, d_runs, nruns, rowlen, d_row);
    }));
    HIPCHK(hipMemcpyAsync(got.data(), d_row, (size_t)rowlen * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (temp) HIPCHK(hipFree(d_part));
    for (int i = 0; i < rowlen; ++i) tot[(size_t)i] += got[(size_t)i];
  }
  memcpy(out, tot.data(), (size_t)nbins * sizeof(double));
  if (mass_out) *mass_out = tot[(size_t)nbins];
  return QSV_OK;
}
