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
  uint8_t flags, n_fix;    // MARG_LEAD | MARG_BATCH_END; entries [n_ent, n_ent + n_fix) are fixed bits (k_marginals_rows alone)
  uint8_t cpos[QSV_MARG_MAX_K], bit[QSV_MARG_MAX_K];   // compact position -> bit of the bin number (a fixed bit: its local position)
};

// Steps 1-4 of the tree above for chunk c of one condition: the chunk's row is formed in `row` (LDS) and stored to dst.
// Shared by k_marginals_cond and k_marginals_rows, so that a chunk takes the same additions whoever walks it.  A fixed
// bit of a group is part of MargGroup::base (k_marginals_cond: the value is the launch's) or an entry past n_ent whose
// bit is read from val (k_marginals_rows: the group list is shared by every row with the same mask).
template <bool NT>
__device__ __forceinline__ void marg_chunk(const cplx* __restrict__ amp, uint64_t nc, const BitIns& fix, uint64_t val, uint64_t zmask,
                                           const MargGroup* __restrict__ grp, int ngrp, int rowlen, uint64_t c, uint64_t bpc,
                                           double* row, double (*stage)[QSV_TPB / 64][1 << QSV_MARG_MAX_K], int& buf,
                                           double* __restrict__ dst) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
          for (int e = G.n_ent; e < G.n_ent + G.n_fix; ++e) bin |= (uint32_t)((val >> G.cpos[e]) & 1ull) << G.bit[e];
          row[G.off + bin] += s;                         // bins of one group are distinct per thread, groups do not share bins
        }
      }
      g0 = g1 + 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < rowlen; i += QSV_TPB) dst[i] = row[i];
  __syncthreads();
}

template <bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_marginals_cond(const cplx* __restrict__ amp, uint64_t nc, BitIns fix, uint64_t val,
                                                            uint64_t zmask, const MargGroup* __restrict__ grp, int ngrp, int rowlen,
                                                            uint64_t nchunks, uint64_t bpc, double* __restrict__ part) {
  static_assert(QSV_TPB == 256 && QSV_SBLOCK == 4096, "the block layout above");
  extern __shared__ double row[];                          // rowlen bins of the chunk in hand
  __shared__ double stage[2][QSV_TPB / 64][1 << QSV_MARG_MAX_K];
  int buf = 0;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x)
    marg_chunk<NT>(amp, nc, fix, val, zmask, grp, ngrp, rowlen, c, bpc, row, stage, buf, part + c * (uint64_t)rowlen);
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

// what qsv_marginals_cond and qsv_marginals_cond_rows refuse about the groups; *nbins_out = the bins of a row
static int marg_check_groups(qsv_handle* h, int n_groups, const int* group_k, const int* qubits, int* nbins_out) {
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
  *nbins_out = nbins;
  return QSV_OK;
}

// The kernels' group list for one local mask on shard s: mg[0 .. n_groups], the mass last before sorting.  A fixed bit of
// a group goes into MargGroup::base with its value from lval (by_row false: the list of one condition), or becomes an
// entry past n_ent that the kernel reads from the row's value (by_row true: the list of every row with this mask).
static void marg_build_groups(const qsv_handle* h, const Shard& s, int n_groups, const int* group_k, const int* qubits,
                              uint64_t lmask, uint64_t lval, bool by_row, MargGroup* mg) {
  const int ngrp = n_groups + 1;
  for (int g = 0, o = 0, off = 0; g < ngrp; ++g) {
    MargGroup& G = mg[g];
    const int k = g < n_groups ? group_k[g] : 0;
    memset(&G, 0, sizeof(G));
    G.off = (uint32_t)off;
    std::pair<int, int> ent[QSV_MARG_MAX_K], fixed[QSV_MARG_MAX_K];   // (compact position, bit of the bin number); (local position, bit)
    int ne = 0, nf = 0;
    for (int b = 0; b < k; ++b) {
      const int q = qubits[o + b];
      if (q >= h->L) G.base |= (uint32_t)shard_bit(h, s, q) << b;
      else if (!((lmask >> q) & 1ull)) ent[ne++] = {q - __builtin_popcountll(lmask & ((1ull << q) - 1ull)), b};
      else if (by_row) fixed[nf++] = {q, b};
      else G.base |= (uint32_t)((lval >> q) & 1ull) << b;
    }
    std::sort(ent, ent + ne);
    G.n_ent = (uint8_t)ne;
    G.n_fix = (uint8_t)nf;
    for (int e = 0; e < ne; ++e) {
      G.cpos[e] = (uint8_t)ent[e].first;
      G.bit[e] = (uint8_t)ent[e].second;
      if (ent[e].first < 12) { G.smask |= (uint16_t)(1u << ent[e].first); G.n_in = (uint8_t)(e + 1); }
    }
    for (int e = 0; e < nf; ++e) { G.cpos[ne + e] = (uint8_t)fixed[e].first; G.bit[ne + e] = (uint8_t)fixed[e].second; }
    o += k;
    off += 1 << k;
  }
  // classes and batches (see above): the order of the groups in the kernel's list is free, G.off says where a group's bins go
  std::stable_sort(mg, mg + ngrp, [](const MargGroup& a, const MargGroup& b) { return a.smask < b.smask; });
  for (int g = 0, used = 0, at = 0; g < ngrp; ++g) {
    MargGroup& G = mg[g];
    if (g == 0 || G.smask != mg[g - 1].smask) {
      const int need = 1 << G.n_in;
      if (used + need > (1 << QSV_MARG_MAX_K)) { mg[g - 1].flags |= MARG_BATCH_END; used = 0; }   // a batch ends only where a class does
      G.flags |= MARG_LEAD;
      at = used;
      used += need;
    }
    G.stage_off = (uint16_t)at;
  }
  mg[ngrp - 1].flags |= MARG_BATCH_END;
}

extern "C" int qsv_marginals_cond(qsv_handle* h, int n_groups, const int* group_k, const int* qubits, uint64_t fix_mask,
                                  uint64_t fix_val, double* out, double* mass_out) {
  if (!h || !group_k || !out) return fail(QSV_E_BADARG, "NULL argument");
  int nbins = 0;
  CHK(marg_check_groups(h, n_groups, group_k, qubits, &nbins));
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
    marg_build_groups(h, s, n_groups, group_k, qubits, lmask, lval, false, mg.data());
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

// qsv_marginals_cond_rows (DESIGN §6c): the same sums for many conditions on one state from one launch group per shard.
//
// A row is one condition; row r of the result is, byte for byte, what qsv_marginals_cond writes for (fix_mask[r],
// fix_val[r]): every row keeps its own compact index space and its own chunking, and every chunk goes through marg_chunk.
// The work is a flat list of (row, chunk) items in row order, item = MargRow::item0 + chunk, walked grid-stride by
// persistent workgroups; item i stores its chunk row to row i of the scratch, so the rows of one condition lie together
// as they do for the single call.  Which workgroup walks an item, and which other rows are in the list, changes nothing
// that is added.  What depends on the local mask alone -- compact positions, smask, classes, batches, stage_off, the
// chunking -- is one MargMask and one group list per distinct mask of the slab, shared by its rows; a row adds its value.
struct MargMask {
  BitIns fix;              // the local fixed bits
  uint32_t grp0;           // first entry of the mask's group list
  uint32_t nt;             // non-temporal loads, by the rule of the single call
  uint64_t nc, bpc;        // matching amplitudes of a shard, blocks per chunk
};
struct MargRow { uint64_t val; uint32_t item0, mask; };
struct MargFold { uint32_t in0, n, out; };                 // rows in0 .. in0 + n - 1 of the scratch added in ascending order into row out

__global__ __launch_bounds__(QSV_TPB) void k_marginals_rows(const cplx* __restrict__ amp, uint64_t zmask, const MargMask* __restrict__ masks,
                                                            const MargRow* __restrict__ rows, uint32_t nrows, uint32_t nitems,
                                                            const MargGroup* __restrict__ grp, int ngrp, int rowlen,
                                                            double* __restrict__ part) {
  extern __shared__ double row[];                          // rowlen bins of the chunk in hand
  __shared__ double stage[2][QSV_TPB / 64][1 << QSV_MARG_MAX_K];
  int buf = 0;
  for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    uint32_t lo = 0, hi = nrows;                           // the row of item it: rows[lo].item0 <= it < rows[hi].item0 (item0 ascends strictly)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (rows[mid].item0 <= it) lo = mid; else hi = mid;
    }
    const MargRow& R = rows[lo];
    const MargMask& M = masks[R.mask];
    double* dst = part + (uint64_t)it * (uint64_t)rowlen;
    if (M.nt) marg_chunk<true>(amp, M.nc, M.fix, R.val, zmask, grp + M.grp0, ngrp, rowlen, it - R.item0, M.bpc, row, stage, buf, dst);
    else marg_chunk<false>(amp, M.nc, M.fix, R.val, zmask, grp + M.grp0, ngrp, rowlen, it - R.item0, M.bpc, row, stage, buf, dst);
  }
}

// step 5 for every row of a slab: what k_marginals_fold does for one condition, a list entry per run of 64 chunk rows
// and, in a second launch, an entry per row that has more than one run
__global__ __launch_bounds__(QSV_TPB) void k_marginals_fold_rows(double* buf, const MargFold* __restrict__ f, uint32_t nf, int rowlen) {
  const int i = blockIdx.x * QSV_TPB + threadIdx.x;
  if (i >= rowlen) return;
  for (uint32_t k = blockIdx.y; k < nf; k += gridDim.y) {
    const MargFold F = f[k];
    double s = 0.0;
    for (uint32_t r = F.in0; r < F.in0 + F.n; ++r) s += buf[(uint64_t)r * (uint64_t)rowlen + i];
    buf[(uint64_t)F.out * (uint64_t)rowlen + i] = s;
  }
}

static inline uint64_t marg_chunks_of(uint64_t nc) { return std::min<uint64_t>((nc + QSV_SBLOCK - 1) / QSV_SBLOCK, 4096); }

extern "C" int qsv_marginals_cond_rows(qsv_handle* h, int n_groups, const int* group_k, const int* qubits, int n_rows,
                                       const uint64_t* fix_mask, const uint64_t* fix_val, double* out, double* mass_out) {
  if (!h || !group_k || !out || !fix_mask || !fix_val) return fail(QSV_E_BADARG, "NULL argument");
  int nbins = 0;
  CHK(marg_check_groups(h, n_groups, group_k, qubits, &nbins));
  if (n_rows < 1 || n_rows > QSV_MARG_MAX_ROWS) return fail(QSV_E_BADARG, "%d rows, 1..%d supported", n_rows, QSV_MARG_MAX_ROWS);
  const uint64_t n = amps_local(h);
  for (int r = 0; r < n_rows; ++r) {
    if (fix_val[r] & ~fix_mask[r]) return fail(QSV_E_BADARG, "row %d: fix_val has bits outside fix_mask", r);
    if (h->W < 64 && (fix_mask[r] >> h->W)) return fail(QSV_E_BADARG, "row %d: fix_mask has bits at or above qubit %d", r, h->W);
    if (__builtin_popcountll(fix_mask[r] & (n - 1)) > QSV_MAXB) return fail(QSV_E_UNSUPPORTED, "row %d: more than %d fixed bits local to a shard", r, QSV_MAXB);
  }
  const int ngrp = n_groups + 1, rowlen = nbins + 1;               // the mass: one more group, without qubits
  // the common condition: the bits every row fixes, to the same value
  uint64_t cmask = ~0ull, differ = 0;
  for (int r = 0; r < n_rows; ++r) { cmask &= fix_mask[r]; differ |= fix_val[r] ^ fix_val[0]; }
  cmask &= ~differ;
  const uint64_t cval = fix_val[0] & cmask;
  auto live = [&](const Shard& s, int r) { return (((uint64_t)s.index << h->L) & fix_mask[r]) == (fix_val[r] & ~(n - 1)); };
  // a deferred shard is prepared once, as the single call with the common condition would prepare it
  for (Shard& s : h->shards) {
    if (!s.deferred) continue;
    bool any = false;
    for (int r = 0; r < n_rows && !any; ++r) any = live(s, r);
    if (!any) continue;
    CHK(shard_set(s));
    if (cmask) CHK(cond_prepare_deferred(h, s, cmask & (n - 1), cval & (n - 1)));
    else CHK(realize(h, s));
  }
  for (size_t i = 0; i < (size_t)n_rows * (size_t)nbins; ++i) out[i] = 0.0;
  std::vector<double> mass((size_t)n_rows, 0.0), got;
  std::vector<char> blob;
  std::vector<int> rows_live;
  std::unordered_map<uint64_t, uint32_t> mask_id;
  // Slabs of consecutive rows: a slab's descriptors are one table of at most half the arena, its chunk rows, run totals
  // and results stay within the scratch that red_scratch keeps (2^24 doubles).  A slab of one row always fits: it asks
  // what the single call asks.  Sized as if every row were live on every shard.
  const size_t desc_cap = h->shards.empty() ? 0 : h->shards[0].arena_bytes / 2 - 256, part_cap = (size_t)1 << 24;
  for (int r0 = 0; r0 < n_rows;) {
    int r1 = r0;
    size_t desc = 0, part = 0;
    mask_id.clear();
    for (; r1 < n_rows; ++r1) {
      if (h->opt_marginals_rows > 0 && r1 - r0 >= h->opt_marginals_rows) break;
      const uint64_t lmask = fix_mask[r1] & (n - 1);
      const uint64_t nch = marg_chunks_of(n >> __builtin_popcountll(lmask)), nruns = (nch + 63) / 64;
      const size_t d = sizeof(MargRow) + (size_t)(nruns + 1) * sizeof(MargFold) +
                       (mask_id.count(lmask) ? 0 : sizeof(MargMask) + (size_t)ngrp * sizeof(MargGroup));
      const size_t p = (size_t)(nch + (nruns > 1 ? nruns : 0) + 1) * (size_t)rowlen;
      if (r1 > r0 && (desc + d > desc_cap || part + p > part_cap)) break;
      mask_id.emplace(lmask, 0u);
      desc += d;
      part += p;
    }
    for (Shard& s : h->shards) {
      rows_live.clear();
      for (int r = r0; r < r1; ++r) if (live(s, r)) rows_live.push_back(r);
      if (rows_live.empty()) continue;
      CHK(shard_set(s));
      const size_t nl = rows_live.size();
      // the table: masks | group lists | rows | fold entries of the first level | of the second
      std::vector<MargMask> masks;
      std::vector<MargGroup> groups;
      std::vector<MargRow> rows(nl);
      std::vector<MargFold> fold1, fold2;
      mask_id.clear();
      uint64_t nitems = 0, nrun_rows = 0, loads = 0;
      for (size_t i = 0; i < nl; ++i) {
        const int r = rows_live[i];
        const uint64_t lmask = fix_mask[r] & (n - 1);
        auto at = mask_id.find(lmask);
        if (at == mask_id.end()) {
          MargMask M;
          memset(&M, 0, sizeof(M));
          for (int q = 0; q < h->L; ++q) if ((lmask >> q) & 1ull) M.fix.pos[M.fix.n++] = q;
          M.nc = n >> M.fix.n;
          M.bpc = (M.nc + QSV_SBLOCK - 1) / QSV_SBLOCK / marg_chunks_of(M.nc);
          // every fixed bit at or above bit 12: a compact block is one contiguous 64 KiB run, streamed as k_blocksum does
          M.nt = (M.fix.n == 0 || M.fix.pos[0] >= 12) && (h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26));
          M.grp0 = (uint32_t)groups.size();
          groups.resize(groups.size() + (size_t)ngrp);
          marg_build_groups(h, s, n_groups, group_k, qubits, lmask, 0, true, groups.data() + M.grp0);
          at = mask_id.emplace(lmask, (uint32_t)masks.size()).first;
          masks.push_back(M);
        }
        const MargMask& M = masks[at->second];
        rows[i].val = fix_val[r] & (n - 1);
        rows[i].item0 = (uint32_t)nitems;
        rows[i].mask = at->second;
        const uint64_t nch = marg_chunks_of(M.nc);
        nitems += nch;
        if (nch > 64) nrun_rows += (nch + 63) / 64;
        loads += M.nc;
      }
      // scratch rows: the items' chunk rows | the run totals of the rows with more than one run | one result per live row
      const uint64_t res0 = nitems + nrun_rows;
      for (size_t i = 0, run0 = nitems; i < nl; ++i) {
        const uint64_t nch = (i + 1 < nl ? rows[i + 1].item0 : nitems) - rows[i].item0, nruns = (nch + 63) / 64;
        for (uint64_t k = 0; k < nruns; ++k)
          fold1.push_back({(uint32_t)(rows[i].item0 + 64 * k), (uint32_t)std::min<uint64_t>(64, nch - 64 * k),
                           (uint32_t)(nruns > 1 ? run0 + k : res0 + i)});
        if (nruns > 1) { fold2.push_back({(uint32_t)run0, (uint32_t)nruns, (uint32_t)(res0 + i)}); run0 += nruns; }
      }
      size_t o_grp, o_row, o_f1, o_f2, total = 0;
      auto place = [&](size_t bytes) { const size_t at = total; total = (total + bytes + 15) & ~(size_t)15; return at; };
      place(masks.size() * sizeof(MargMask));
      o_grp = place(groups.size() * sizeof(MargGroup));
      o_row = place(rows.size() * sizeof(MargRow));
      o_f1 = place(fold1.size() * sizeof(MargFold));
      o_f2 = place(fold2.size() * sizeof(MargFold));
      blob.assign(total, 0);
      memcpy(blob.data(), masks.data(), masks.size() * sizeof(MargMask));
      memcpy(blob.data() + o_grp, groups.data(), groups.size() * sizeof(MargGroup));
      memcpy(blob.data() + o_row, rows.data(), rows.size() * sizeof(MargRow));
      memcpy(blob.data() + o_f1, fold1.data(), fold1.size() * sizeof(MargFold));
      if (!fold2.empty()) memcpy(blob.data() + o_f2, fold2.data(), fold2.size() * sizeof(MargFold));
      void* d_tab = nullptr;
      CHK(arena_put(s, blob.data(), total, &d_tab));
      double* d_part = nullptr;
      bool temp = false;
      CHK(red_scratch(s, (size_t)(res0 + nl) * (size_t)rowlen, &d_part, &temp));
      const char* dt = reinterpret_cast<const char*>(d_tab);
      int rc = launch(h, s, QSV_K_PROB, 16.0 * (double)loads, [&] {
        uint64_t grid = std::min<uint64_t>(nitems, (uint64_t)s.n_cu * 8);
        if (h->opt_marginals_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_marginals_grid);
        hipLaunchKernelGGL(k_marginals_rows, dim3((unsigned)grid), dim3(QSV_TPB), (size_t)rowlen * sizeof(double), s.stream, s.amp, s.zmask,
                           reinterpret_cast<const MargMask*>(dt), reinterpret_cast<const MargRow*>(dt + o_row), (uint32_t)nl, (uint32_t)nitems,
                           reinterpret_cast<const MargGroup*>(dt + o_grp), ngrp, rowlen, d_part);
        const unsigned fx = (unsigned)((rowlen + QSV_TPB - 1) / QSV_TPB);
        hipLaunchKernelGGL(k_marginals_fold_rows, dim3(fx, (unsigned)std::min<size_t>(fold1.size(), 65535)), dim3(QSV_TPB), 0, s.stream, d_part,
                           reinterpret_cast<const MargFold*>(dt + o_f1), (uint32_t)fold1.size(), rowlen);
        if (!fold2.empty())
          hipLaunchKernelGGL(k_marginals_fold_rows, dim3(fx, (unsigned)std::min<size_t>(fold2.size(), 65535)), dim3(QSV_TPB), 0, s.stream, d_part,
                             reinterpret_cast<const MargFold*>(dt + o_f2), (uint32_t)fold2.size(), rowlen);
      });
      got.resize(nl * (size_t)rowlen);
      hipError_t e_copy = rc == QSV_OK ? hipMemcpyAsync(got.data(), d_part + (size_t)res0 * (size_t)rowlen, got.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream) : hipSuccess;
      hipError_t e_sync = hipStreamSynchronize(s.stream);
      if (temp) HIPCHK(hipFree(d_part));                     // before any error returns: a temporary does not outlive the call
      CHK(rc);
      HIPCHK(e_copy);
      HIPCHK(e_sync);
      for (size_t i = 0; i < nl; ++i) {                      // step 6: the shards in shard order
        double* o = out + (size_t)rows_live[i] * (size_t)nbins;
        const double* g = got.data() + i * (size_t)rowlen;
        for (int b = 0; b < nbins; ++b) o[b] += g[b];
        mass[(size_t)rows_live[i]] += g[nbins];
      }
    }
    r0 = r1;
  }
  if (mass_out) memcpy(mass_out, mass.data(), (size_t)n_rows * sizeof(double));
  return QSV_OK;
}
