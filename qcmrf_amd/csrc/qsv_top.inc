// qsv_top_cond (DESIGN §6b): the K most probable basis states of the conditioned state from one load of each matching
// amplitude -- exact MAP / top-k inference on the state a QCMRF circuit prepares.
//
// A candidate is the pair (p, x): x a global index with (x & fix_mask) == fix_val, p = re*re + im*im with each product
// and the sum rounded separately (top_weight: contraction off, NOT the fma of the summing kernels -- numpy's
// a.real*a.real + a.imag*a.imag on the amplitudes read back is then the same bits).  The order is strict and total:
//     (p, x) before (q, y)   iff   p > q, or p == q and x < y
// and only candidates with p > 0 take part (a 0, an implied zero and a NaN fail `p > anything`).  The K first candidates
// of a set under a strict total order are a pure function of the set: whatever the grid, whichever workgroup walks a
// block and in whatever order lists are merged, the result is the same.  No floating-point atomics (the workgroup-wide
// votes are integer ORs in LDS, whose result does not depend on arrival order).
//
// The index space is the compact one of qsv_sample_cond (CondView) in the blocks of k_marginals_cond: block b, thread tid
// and load u read compact index j = b*4096 + u*256 + tid, local address ins_bits(j, F) | val -- ascending in (b, u, tid).
//
// k_top_cond: a workgroup keeps its best K candidates in LDS, sorted, and the weight of the K-th (0 while fewer than K
//   are held) as its threshold thr.  It walks blocks blockIdx.x, + grid, ... in ascending order, and u in ascending order
//   inside a block, so every candidate it meets has a larger index than all it has met: one that ties the threshold
//   comes after the K-th and `p > thr` alone decides.  The common block -- no entrant -- costs the loads, one compare per
//   entry and one workgroup-wide vote (__syncthreads_or).  A block with entrants takes one vote per u and, for every u
//   with entrants, one fold (top_fold).
// top_fold: up to one entrant per thread is folded into the sorted list.  The entrants are compacted in thread order
//   (wave ballots, the waves' counts through LDS); every entrant counts the list entries and entrants before it, every
//   list entry adds the entrants before it to its position: the counts are the places in the merged order (a permutation,
//   the order is strict), and whoever's place is below K stores itself there in the other list buffer.
// k_top_merge: a workgroup reduces a run of lists to one by the same fold, 8 candidates per thread and round, under the
//   full order (lists of different workgroups interleave in index).  One workgroup reduces the lists to the shard's K;
//   above TOP_MERGE_ONE lists a first launch reduces runs of TOP_MERGE_RUN lists, one workgroup each, to one list per
//   run (the rounds of one workgroup are serial) -- which lists meet first changes
//   nothing, the order is total.
// The shards of a process are merged on the host by the same order.
struct TopList {
  double p[2][QSV_TOP_MAX_K];
  uint64_t x[2][QSV_TOP_MAX_K];
  double ep[QSV_TPB];
  uint64_t ex[QSV_TPB];
  uint32_t wcnt[QSV_TPB / 64];
};

__device__ __forceinline__ double top_weight(cplx a) {
#pragma clang fp contract(off)
  const double r = a.x * a.x, i = a.y * a.y;
  return r + i;
}
__device__ __forceinline__ bool top_before(double p, uint64_t x, double q, uint64_t y) { return p > q || (p == q && x < y); }

// Fold the threads' entrants (has: this thread brings (p, x), p > 0, not in the list) into the list of n entries in
// buffer cur; returns the new n, the list then in buffer cur ^ 1.  Every thread of the workgroup calls it (barriers inside).
__device__ __forceinline__ int top_fold(TopList& T, int cur, int n, int K, bool has, double p, uint64_t x) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long vote = __ballot(has);
  if (lane == 0) T.wcnt[wave] = (uint32_t)__popcll(vote);
  __syncthreads();
  uint32_t at = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull)), e = 0;
  for (uint32_t w = 0; w < QSV_TPB / 64; ++w) { if (w < wave) at += T.wcnt[w]; e += T.wcnt[w]; }
  if (has) { T.ep[at] = p; T.ex[at] = x; }
  __syncthreads();
  if (tid < e) {                                           // entrant tid: list entries and entrants before it
    const double q = T.ep[tid];
    const uint64_t y = T.ex[tid];
    int r = 0;
    for (int s = 0; s < n; ++s) r += top_before(T.p[cur][s], T.x[cur][s], q, y) ? 1 : 0;
    for (uint32_t s = 0; s < e; ++s) r += top_before(T.ep[s], T.ex[s], q, y) ? 1 : 0;
    if (r < K) { T.p[cur ^ 1][r] = q; T.x[cur ^ 1][r] = y; }
  }
  if (tid >= QSV_TPB - (uint32_t)n) {                      // list entry s (the last threads: entrants sit on the first ones)
    const int s = (int)(QSV_TPB - 1u - tid);
    const double q = T.p[cur][s];
    const uint64_t y = T.x[cur][s];
    int r = s;
    for (uint32_t t = 0; t < e; ++t) r += top_before(T.ep[t], T.ex[t], q, y) ? 1 : 0;
    if (r < K) { T.p[cur ^ 1][r] = q; T.x[cur ^ 1][r] = y; }
  }
  __syncthreads();
  const int m = n + (int)e;
  return m < K ? m : K;
}

// a workgroup's list goes to lp / lx [blockIdx.x * K ..], its length to ln[blockIdx.x]; hi: the shard's bits of the index
template <bool NT>
__global__ __launch_bounds__(QSV_TPB) void k_top_cond(const cplx* __restrict__ amp, uint64_t nc, BitIns fix, uint64_t val,
                                                      uint64_t zmask, uint64_t hi, int K, uint64_t nblk,
                                                      double* __restrict__ lp, uint64_t* __restrict__ lx, uint32_t* __restrict__ ln) {
  static_assert(QSV_TPB == 256 && QSV_SBLOCK == 4096, "the block layout above");
  __shared__ TopList T;
  const uint32_t tid = threadIdx.x;
  int cur = 0, n = 0;
  double thr = 0.0;
  for (uint64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    double p[16];
    bool mine = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const uint64_t j = b * QSV_SBLOCK + (uint64_t)u * QSV_TPB + tid;
      p[u] = 0.0;
      if (j < nc) {
        const uint64_t i = ins_bits(j, fix) | val;
        if (!(i & zmask)) p[u] = top_weight(NT ? ld_nt(amp + i) : amp[i]);
      }
      mine |= p[u] > thr;
    }
    if (!__syncthreads_or(mine ? 1 : 0)) continue;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const bool has = p[u] > thr;
      if (!__syncthreads_or(has ? 1 : 0)) continue;
      const uint64_t j = b * QSV_SBLOCK + (uint64_t)u * QSV_TPB + tid;
      n = top_fold(T, cur, n, K, has, p[u], hi | ins_bits(j, fix) | val);
      cur ^= 1;
      thr = n == K ? T.p[cur][K - 1] : 0.0;
    }
  }
  __syncthreads();
  if (tid < (uint32_t)n) { lp[(uint64_t)blockIdx.x * K + tid] = T.p[cur][tid]; lx[(uint64_t)blockIdx.x * K + tid] = T.x[cur][tid]; }
  if (tid == 0) ln[blockIdx.x] = (uint32_t)n;
}

// nl lists of up to K entries (list g: ln[g] entries from g * K); workgroup w takes the lists [w * run, (w + 1) * run):
// the first K of their union, sorted, to op / ox [w * K ..], their number to on[w].  The threshold is the K-th entry as a
// pair: lists interleave in index.
enum { TOP_MERGE_ONE = 64, TOP_MERGE_RUN = 32 };
__global__ __launch_bounds__(QSV_TPB) void k_top_merge(const double* __restrict__ lp, const uint64_t* __restrict__ lx,
                                                       const uint32_t* __restrict__ ln, uint32_t nl, uint32_t run, int K,
                                                       double* __restrict__ op, uint64_t* __restrict__ ox, uint32_t* __restrict__ on) {
  __shared__ TopList T;
  const uint32_t tid = threadIdx.x;
  const uint32_t first = blockIdx.x * run * (uint32_t)K;   // (at most 8 lists per CU of 64 entries: far below 2^32)
  const uint32_t tot = (nl < (blockIdx.x + 1) * run ? nl : (blockIdx.x + 1) * run) * (uint32_t)K;
  int cur = 0, n = 0;
  double thr = 0.0;
  uint64_t thx = 0;                                        // with thr == 0 (list not full) a tie at 0 must not enter: x < 0 never holds
  for (uint32_t c0 = first; c0 < tot; c0 += 8 * QSV_TPB) {
    double p[8];
    uint64_t x[8];
    bool mine = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t c = c0 + (uint32_t)r * QSV_TPB + tid;
      p[r] = 0.0;
      x[r] = 0;
      if (c < tot && c % (uint32_t)K < ln[c / (uint32_t)K]) { p[r] = lp[c]; x[r] = lx[c]; }
      mine |= top_before(p[r], x[r], thr, thx);
    }
    if (!__syncthreads_or(mine ? 1 : 0)) continue;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const bool has = top_before(p[r], x[r], thr, thx);
      if (!__syncthreads_or(has ? 1 : 0)) continue;
      n = top_fold(T, cur, n, K, has, p[r], x[r]);
      cur ^= 1;
      thr = n == K ? T.p[cur][K - 1] : 0.0;
      thx = n == K ? T.x[cur][K - 1] : 0;
    }
  }
  __syncthreads();
  if (tid < (uint32_t)n) { op[blockIdx.x * (uint32_t)K + tid] = T.p[cur][tid]; ox[blockIdx.x * (uint32_t)K + tid] = T.x[cur][tid]; }
  if (tid == 0) on[blockIdx.x] = (uint32_t)n;
}

extern "C" int qsv_top_cond(qsv_handle* h, int k, uint64_t fix_mask, uint64_t fix_val, uint64_t* out_index, double* out_p,
                            int* n_found) {
  if (!h || !out_index || !out_p || !n_found) return fail(QSV_E_BADARG, "NULL argument");
  if (k < 1 || k > QSV_TOP_MAX_K) return fail(QSV_E_BADARG, "k = %d, 1..%d supported", k, QSV_TOP_MAX_K);
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
  const uint64_t nblk = (cv.nc + QSV_SBLOCK - 1) / QSV_SBLOCK;
  std::vector<std::pair<double, uint64_t>> best;           // the shards' lists, merged by the same order
  for (Shard& s : h->shards) {
    // a fixed shard bit does not enter the kernels: a shard whose index disagrees with it holds no candidate
    if ((((uint64_t)s.index << h->L) & fix_mask) != (fix_val & ~(n - 1))) continue;
    CHK(shard_set(s));
    if (s.deferred) {
      if (fix_mask) CHK(cond_prepare_deferred(h, s, lmask, lval));
      else CHK(realize(h, s));
    }
    uint64_t grid = std::min<uint64_t>(nblk, (uint64_t)s.n_cu * 8);
    if (h->opt_top_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_top_grid);
    // scratch, in 8-byte words: the workgroups' weights and indices, the shard's K of each and their number, the lists'
    // lengths, and the same three for the lists of the first merge
    const uint32_t nrun = grid > TOP_MERGE_ONE ? (uint32_t)((grid + TOP_MERGE_RUN - 1) / TOP_MERGE_RUN) : 0;
    const size_t nlist = (size_t)grid * (size_t)k, nlen = 1 + ((size_t)grid + 1) / 2, nlist2 = (size_t)nrun * (size_t)k;
    double* d_lp = nullptr;
    bool temp = false;
    CHK(red_scratch(s, 2 * nlist + 2 * (size_t)k + nlen + 2 * nlist2 + ((size_t)nrun + 1) / 2, &d_lp, &temp));
    uint64_t* d_lx = reinterpret_cast<uint64_t*>(d_lp + nlist);
    double* d_op = d_lp + 2 * nlist;
    uint64_t* d_ox = reinterpret_cast<uint64_t*>(d_op + k);
    uint32_t* d_on = reinterpret_cast<uint32_t*>(d_op + 2 * (size_t)k);      // one word of its own: d_op .. d_on come back in one copy
    uint32_t* d_ln = d_on + 2;
    double* d_lp2 = d_op + 2 * (size_t)k + nlen;
    uint64_t* d_lx2 = reinterpret_cast<uint64_t*>(d_lp2 + nlist2);
    uint32_t* d_ln2 = reinterpret_cast<uint32_t*>(d_lp2 + 2 * nlist2);
    const uint64_t hi = (uint64_t)s.index << h->L;
    CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)cv.nc, [&] {
      // every fixed bit at or above bit 12: a compact block is one contiguous 64 KiB run, streamed as k_marginals_cond does
      const bool nt = (cv.fix.n == 0 || cv.fix.pos[0] >= 12) && (h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26));
      if (nt) hipLaunchKernelGGL(k_top_cond<true>, dim3((unsigned)grid), dim3(QSV_TPB), 0, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, hi, k, nblk, d_lp, d_lx, d_ln);
      else hipLaunchKernelGGL(k_top_cond<false>, dim3((unsigned)grid), dim3(QSV_TPB), 0, s.stream, s.amp, cv.nc, cv.fix, cv.val, s.zmask, hi, k, nblk, d_lp, d_lx, d_ln);
      if (nrun) {
        hipLaunchKernelGGL(k_top_merge, dim3(nrun), dim3(QSV_TPB), 0, s.stream, d_lp, d_lx, d_ln, (uint32_t)grid, (uint32_t)TOP_MERGE_RUN, k, d_lp2, d_lx2, d_ln2);
        hipLaunchKernelGGL(k_top_merge, dim3(1), dim3(QSV_TPB), 0, s.stream, d_lp2, d_lx2, d_ln2, nrun, nrun, k, d_op, d_ox, d_on);
      } else {
        hipLaunchKernelGGL(k_top_merge, dim3(1), dim3(QSV_TPB), 0, s.stream, d_lp, d_lx, d_ln, (uint32_t)grid, (uint32_t)grid, k, d_op, d_ox, d_on);
      }
    }));
    uint64_t got[2 * QSV_TOP_MAX_K + 1];                   // k weights, k indices, the count
    hipError_t e_copy = hipMemcpyAsync(got, d_op, (2 * (size_t)k + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
    hipError_t e_sync = hipStreamSynchronize(s.stream);
    if (temp) HIPCHK(hipFree(d_lp));                       // before either error returns: a temporary does not outlive the call
    HIPCHK(e_copy);
    HIPCHK(e_sync);
    uint32_t gn = 0;                                       // the kernel stores 4 bytes at the start of the count's word: read those, not the word
    memcpy(&gn, &got[2 * k], sizeof(gn));
    for (uint32_t i = 0; i < gn && i < (uint32_t)k; ++i) {
      double p;
      memcpy(&p, &got[i], sizeof(p));
      best.emplace_back(p, got[(size_t)k + i]);
    }
  }
  std::sort(best.begin(), best.end(), [](const std::pair<double, uint64_t>& a, const std::pair<double, uint64_t>& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  });
  const size_t m = std::min<size_t>(best.size(), (size_t)k);
  for (size_t i = 0; i < m; ++i) { out_p[i] = best[i].first; out_index[i] = best[i].second; }
  *n_found = (int)m;
  return QSV_OK;
}
