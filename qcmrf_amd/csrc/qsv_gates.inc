// qsv_gates.inc -- per-shard gate resolution and the one-gate-one-kernel launchers (part of qsv.hip)
// ------------------------------------------------------------------------------------------
// gates: every gate is first RESOLVED per shard (shard-bit controls evaluated, tables sliced)
// into a LocalOp on local address bits, then either launched alone (dedicated kernel) or
// grouped with its neighbours into one register-tiled k_multi pass (qsv_exec).
// ------------------------------------------------------------------------------------------
struct LocalOp {
  int type = 0;               // 0 mux table | 1 diag table | 2 controlled 2x2 | 3 controlled phase
  bool is_x = false;          // type 2 that is a plain X: swap kernel when launched alone
  int target = -1;            // local address bit (types 0, 2)
  std::vector<int> list;      // types 0,1: gather list; table index bit e <- address bit list[e]
  std::vector<double> table;  // type 0: 8 doubles per entry; type 1: 2 doubles per entry
  std::vector<int> cq, cv;    // types 2,3: local controls and their values
  double m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// slice a 2^k table (entry = `ent` doubles) over `qubits` down to the local qubits of shard s
static void slice_table(const qsv_handle* h, const Shard& s, int k, const int* qubits, const double* table,
                        int ent, std::vector<int>& lq, std::vector<double>& out) {
  std::vector<int> lpos;
  uint32_t gfix = 0;
  lq.clear();
  for (int b = 0; b < k; ++b) {
    if (qubits[b] >= h->L) { if (shard_bit(h, s, qubits[b])) gfix |= 1u << b; }
    else { lpos.push_back(b); lq.push_back(qubits[b]); }
  }
  const int kl = (int)lpos.size();
  out.resize((size_t)ent << kl);
  for (uint32_t jl = 0; jl < (1u << kl); ++jl) {
    uint32_t j = gfix;
    for (int b = 0; b < kl; ++b) if ((jl >> b) & 1u) j |= 1u << lpos[b];
    memcpy(&out[(size_t)jl * ent], &table[(size_t)j * ent], sizeof(double) * ent);
  }
}

// argument validation shared by the one-gate entry points and qsv_exec
static int validate_gate(const qsv_handle* h, int kind, int n, const int* q, int target, const void* data) {
  switch (kind) {
    case QSV_OP_1Q: case QSV_OP_MCX:
      if (n < 0 || n > QSV_MAX_CTRL || (n && !q)) return fail(QSV_E_BADARG, "n_ctrl %d out of range", n);
      CHK(check_qubit(h, target, "target"));
      CHK(check_distinct(h, n, q, target));
      if (kind == QSV_OP_1Q && !data) return fail(QSV_E_BADARG, "matrix is NULL");
      break;
    case QSV_OP_MUX:
      if (n < 0 || n > 10 || (n && !q) || !data) return fail(QSV_E_BADARG, "mux needs 0..10 controls and matrices");
      CHK(check_qubit(h, target, "target"));
      CHK(check_distinct(h, n, q, target));
      break;
    case QSV_OP_DIAG:
      if (n < 1 || n > QSV_MAX_CTRL || !q || !data) return fail(QSV_E_BADARG, "diag needs 1..%d qubits and a table", QSV_MAX_CTRL);
      CHK(check_distinct(h, n, q, -1));
      return QSV_OK;
    case QSV_OP_MCPHASE:
      if (n < 1 || n > QSV_MAX_CTRL || !q) return fail(QSV_E_BADARG, "mcphase needs 1..%d qubits", QSV_MAX_CTRL);
      CHK(check_distinct(h, n, q, -1));
      return QSV_OK;
    default:
      return fail(QSV_E_BADARG, "not a gate kind: %d", kind);
  }
  if (target >= h->L)
    return fail(QSV_E_UNSUPPORTED, "target qubit %d is a shard bit (local qubits: %d); qsv_swap_layout it first", target, h->L);
  return QSV_OK;
}

// false: this shard is untouched by the gate (a shard-bit control does not match)
static bool resolve_gate(const qsv_handle* h, const Shard& s, int kind, int n, const int* q, const int* vals,
                         int target, const double* data, double angle, LocalOp& lo) {
  lo = LocalOp();
  if (kind == QSV_OP_1Q || kind == QSV_OP_MCX || kind == QSV_OP_MCPHASE) {
    LocalCtrl lc = resolve_ctrl(h, s, n, q, vals);
    if (lc.skip) return false;
    lo.cq = lc.q;
    lo.cv = lc.v;
    if (kind == QSV_OP_MCPHASE) {
      lo.type = 3;
      lo.m[0] = std::cos(angle);
      lo.m[1] = std::sin(angle);
    } else {
      lo.type = 2;
      lo.target = target;
      lo.is_x = kind == QSV_OP_MCX;
      if (lo.is_x) { lo.m[2] = 1.0; lo.m[4] = 1.0; }
      else memcpy(lo.m, data, sizeof lo.m);
    }
    return true;
  }
  if (kind == QSV_OP_MUX) {
    lo.type = 0;
    lo.target = target;
    slice_table(h, s, n, q, data, 8, lo.list, lo.table);
  } else {
    lo.type = 1;
    slice_table(h, s, n, q, data, 2, lo.list, lo.table);
  }
  return true;
}

template <int KIND, bool NT>
static void launch_pair(const qsv_handle* h, const Shard& s, uint64_t npairs, const BitIns& ins,
                        uint64_t fixed, uint64_t tbit, const Mat2& m, int swz) {
  const int U = h->opt_unroll;
  if (U >= 4 && npairs % (QSV_TPB * 4) == 0)
    hipLaunchKernelGGL((k_pair<KIND, 4, false, NT>), dim3(grid_for(h, s, npairs, QSV_TPB * 4)), dim3(QSV_TPB), 0,
                       s.stream, s.amp, npairs, ins, fixed, tbit, m, swz);
  else if (U >= 2 && npairs % (QSV_TPB * 2) == 0)
    hipLaunchKernelGGL((k_pair<KIND, 2, false, NT>), dim3(grid_for(h, s, npairs, QSV_TPB * 2)), dim3(QSV_TPB), 0,
                       s.stream, s.amp, npairs, ins, fixed, tbit, m, swz);
  else
    hipLaunchKernelGGL((k_pair<KIND, 1, true, NT>), dim3(grid_for(h, s, npairs, QSV_TPB)), dim3(QSV_TPB), 0,
                       s.stream, s.amp, npairs, ins, fixed, tbit, m, swz);
}

// one resolved gate, one dedicated kernel
// Non-temporal loads + stores for the one-gate-one-kernel sweeps (option "nontemporal": -1 by shard
// size, 0 never, 1 always).  Measured at 28 qubits (profiles/r02_gates_nt.log): dense 1q / diag / mux
// sweeps +5-6 % (0.66-0.69 -> 0.69-0.73 of peak, target 11/12: 0.82), but a gate whose control or
// target sits inside a 128-byte line (bits 0..2) touches lines only partly and LOSES without the
// cache (ccx with a control on bit 1: 0.31 -> 0.23): those keep the plain form.
// index swizzle of the one-gate kernels (swz_5_11): when neither bit is one the gate singles out
// Returns the address bit that changes places with bit 11 (the kernels' ``swz``), 0 for none.
static int single_swz(const qsv_handle* h, uint64_t special_bits) {
  // from 2^26 amplitudes on (profiles/r02_swizzle_by_size.log: +10-18 % at 28-30 qubits, +3-17 % at 26, nothing or a few
  // percent lost where the state sits in the caches); swizzle = 2 forces it from 2^14 (tests)
  return (h->opt_swz && (h->L >= 26 || (h->opt_swz > 1 && h->L >= 14)) && !(special_bits & ((1ull << 5) | (1ull << 11)))) ? 5 : 0;
}
// ... for a sweep that ENUMERATES the indices with the special bits (controls, target) left out: lane bit 5 of the
// enumeration lands on the sixth free address bit -- bit 5, or the next free one when a control or the target sits on
// bits 0..5 -- and that one trades places with bit 11 (a dense gate on target 5: 0.74 -> 0.80 of the stream; ccx with
// controls on bits 1 and 5: 0.34 -> 0.40, profiles/r03zz_gate_microbench_W28.jsonl)
static int skip_swz(const qsv_handle* h, uint64_t special_bits) {
  if (!(h->opt_swz && (h->L >= 26 || (h->opt_swz > 1 && h->L >= 14))) || ((special_bits >> 11) & 1)) return 0;
  int nfree = 0;
  for (int bit = 0; bit < 11; ++bit) {
    if ((special_bits >> bit) & 1) continue;
    if (nfree++ == 5) return bit;
  }
  return 0;
}
static bool single_nt(const qsv_handle* h, int lowest_bit) {
  if (h->opt_nt >= 0) return h->opt_nt > 0;
  return h->L >= 26 && lowest_bit >= 3;
}

static int run_single(qsv_handle* h, Shard& s, const LocalOp& lo) {
  CHK(shard_set(s));
  const uint64_t n = amps_local(h);
  if (lo.type == 2) {
    const int nc = (int)lo.cq.size(), t = lo.target;
    const uint64_t npairs = n >> (1 + nc);
    const double bytes = 32.0 * (double)(n >> nc);
    const int kind = lo.is_x ? QSV_K_X : QSV_K_1Q;
    Mat2 mm;
    memcpy(mm.v, lo.m, sizeof mm.v);
    // (target 5: the pair sweep with bit 6 in the swizzle's place streams at 0.81, the shuffle form -- one 1 KiB run per wave access -- at 0.76)
    // (an X on such a target is the same stream with the partner's amplitude taken as it is: 0.76 as a pair sweep, 0.83 here)
    if (nc == 0 && (t < 5 || (t == 5 && !skip_swz(h, 1ull << 5))) && h->opt_lowt_shuffle && n % (QSV_TPB * 4) == 0) {
      if (lo.is_x) { memset(mm.v, 0, sizeof mm.v); mm.v[2] = 1.0; mm.v[4] = 1.0; }
      return launch(h, s, kind, bytes, [&] {
        if (single_nt(h, 3))                                  // every line is read and written whole
          hipLaunchKernelGGL((k_lowt<4, true>), dim3(grid_for(h, s, n, QSV_TPB * 4)), dim3(QSV_TPB), 0, s.stream, s.amp, n, t, mm, single_swz(h, 1ull << t));
        else
          hipLaunchKernelGGL((k_lowt<4, false>), dim3(grid_for(h, s, n, QSV_TPB * 4)), dim3(QSV_TPB), 0, s.stream, s.amp, n, t, mm, single_swz(h, 1ull << t));
      });
    }
    // a control inside a 128-byte line: masked full-line sweep (k_pair_m) over the pairs the HIGHER controls select
    if (h->opt_lowctl_mask && nc > 0) {
      std::vector<int> hpos;
      uint64_t hfixed = 0, lmask = 0, lval = 0;
      for (int i = 0; i < nc; ++i) {
        if (lo.cq[i] < 3) { lmask |= 1ull << lo.cq[i]; if (lo.cv[i]) lval |= 1ull << lo.cq[i]; }
        else { hpos.push_back(lo.cq[i]); if (lo.cv[i]) hfixed |= 1ull << lo.cq[i]; }
      }
      const uint64_t np = n >> (1 + hpos.size());
      if (lmask && np % (QSV_TPB * 4) == 0 && np / (QSV_TPB * 4) < (1ull << 31)) {
        hpos.push_back(t);
        const BitIns hins = make_ins(hpos);
        const bool nt = single_nt(h, 3);                       // lines are read and written whole
        uint64_t hspecial = 0;
        for (int p : hpos) hspecial |= 1ull << p;
        const int swa = skip_swz(h, hspecial) ? skip_swz(h, hspecial) : -1;
        const dim3 g((unsigned)(np / (QSV_TPB * 4))), b(QSV_TPB);
        return launch(h, s, kind, bytes, [&] {
          if (lo.is_x) { if (nt) hipLaunchKernelGGL((k_pair_m<1, 4, true>), g, b, 0, s.stream, s.amp, np, hins, hfixed, 1ull << t, mm, lmask, lval, swa);
                         else    hipLaunchKernelGGL((k_pair_m<1, 4, false>), g, b, 0, s.stream, s.amp, np, hins, hfixed, 1ull << t, mm, lmask, lval, swa); }
          else         { if (nt) hipLaunchKernelGGL((k_pair_m<0, 4, true>), g, b, 0, s.stream, s.amp, np, hins, hfixed, 1ull << t, mm, lmask, lval, swa);
                         else    hipLaunchKernelGGL((k_pair_m<0, 4, false>), g, b, 0, s.stream, s.amp, np, hins, hfixed, 1ull << t, mm, lmask, lval, swa); }
        });
      }
    }
    std::vector<int> pos = lo.cq;
    pos.push_back(t);
    const BitIns ins = make_ins(pos);
    uint64_t fixed = 0;
    for (int i = 0; i < nc; ++i) if (lo.cv[i]) fixed |= 1ull << lo.cq[i];
    const uint64_t tbit = 1ull << t;
    if (h->opt_pair_variant && !lo.is_x && npairs % (QSV_TPB * 8 * 8) == 0) {
      const int v = h->opt_pair_variant;
      return launch(h, s, kind, bytes, [&] {
#define PX(U, NL, NS, RM) hipLaunchKernelGGL((k_pair_x<U, NL, NS, RM>), dim3((unsigned)(npairs / (QSV_TPB * U))), dim3(QSV_TPB), 0, s.stream, s.amp, npairs, ins, fixed, tbit, mm)
        switch (v) {
          case 1: PX(4, false, false, false); break;   // baseline shape without the grid-stride loop
          case 2: PX(4, false, true, false); break;    // nt stores only
          case 3: PX(4, true, false, false); break;    // nt loads only
          case 4: PX(4, false, false, true); break;    // XCD remap
          case 5: PX(8, false, false, false); break;   // deeper unroll
          case 6: PX(8, false, false, true); break;
          case 7: PX(2, false, false, false); break;
          case 8: PX(4, false, true, true); break;
          default: PX(8, false, true, false); break;
        }
#undef PX
      });
    }
    int lowest = t;
    for (int q : lo.cq) lowest = std::min(lowest, q);
    const bool nt = single_nt(h, lowest);
    uint64_t special = tbit;
    for (int q : lo.cq) special |= 1ull << q;
    const int swz = skip_swz(h, special);
    return launch(h, s, kind, bytes, [&] {
      if (lo.is_x) { if (nt) launch_pair<1, true>(h, s, npairs, ins, fixed, tbit, mm, swz); else launch_pair<1, false>(h, s, npairs, ins, fixed, tbit, mm, swz); }
      else         { if (nt) launch_pair<0, true>(h, s, npairs, ins, fixed, tbit, mm, swz); else launch_pair<0, false>(h, s, npairs, ins, fixed, tbit, mm, swz); }
    });
  }
  if (lo.type == 3) {
    const int nc = (int)lo.cq.size();
    const uint64_t nsub = n >> nc;
    const BitIns ins = make_ins(lo.cq);
    uint64_t fixed = 0;
    for (int i = 0; i < nc; ++i) if (lo.cv[i]) fixed |= 1ull << lo.cq[i];
    const cplx ph = make_double2(lo.m[0], lo.m[1]);
    uint64_t special = 0;
    for (int q : lo.cq) special |= 1ull << q;
    const int swz = skip_swz(h, special);
    return launch(h, s, QSV_K_MCPHASE, 32.0 * (double)nsub, [&] {
      if (nsub % (QSV_TPB * 4) == 0)
        hipLaunchKernelGGL((k_mcphase<4, false>), dim3(grid_for(h, s, nsub, QSV_TPB * 4)), dim3(QSV_TPB), 0, s.stream, s.amp, nsub, ins, fixed, ph, swz);
      else
        hipLaunchKernelGGL((k_mcphase<1, true>), dim3(grid_for(h, s, nsub, QSV_TPB)), dim3(QSV_TPB), 0, s.stream, s.amp, nsub, ins, fixed, ph, swz);
    });
  }
  const int kl = (int)lo.list.size();
  void* dtab = nullptr;
  CHK(arena_put(s, lo.table.data(), lo.table.size() * sizeof(double), &dtab));
  BitList bl;
  bl.n = kl;
  for (int b = 0; b < kl; ++b) bl.pos[b] = lo.list[b];
  if (lo.type == 1) {
    const int ntab = 1 << kl;
    const bool lds = kl <= 11;
    const size_t shm = lds ? (size_t)ntab * sizeof(cplx) : 0;
    const int swz = single_swz(h, 0);                        // every amplitude on its own: no bit is special
    return launch(h, s, QSV_K_DIAG, 32.0 * (double)n, [&] {
      const cplx* tp = reinterpret_cast<const cplx*>(dtab);
      if (n % (QSV_TPB * 4) == 0) {
        const dim3 g(grid_for(h, s, n, QSV_TPB * 4));
        if (lds) {
          if (single_nt(h, 3)) hipLaunchKernelGGL((k_diag<4, false, true, true>), g, dim3(QSV_TPB), shm, s.stream, s.amp, n, bl, tp, ntab, swz);
          else           hipLaunchKernelGGL((k_diag<4, false, true, false>), g, dim3(QSV_TPB), shm, s.stream, s.amp, n, bl, tp, ntab, swz);
        } else           hipLaunchKernelGGL((k_diag<4, false, false, false>), g, dim3(QSV_TPB), 0, s.stream, s.amp, n, bl, tp, ntab, swz);
      } else {
        const dim3 g(grid_for(h, s, n, QSV_TPB));
        if (lds) hipLaunchKernelGGL((k_diag<1, true, true, false>), g, dim3(QSV_TPB), shm, s.stream, s.amp, n, bl, tp, ntab, swz);
        else     hipLaunchKernelGGL((k_diag<1, true, false, false>), g, dim3(QSV_TPB), 0, s.stream, s.amp, n, bl, tp, ntab, swz);
      }
    });
  }
  // type 0: uniformly controlled 2x2
  const int nmat = 1 << kl, t = lo.target;
  const uint64_t npairs = n >> 1;
  const size_t shm = (size_t)nmat * 64;
  const int swz = skip_swz(h, 1ull << t);                    // the selects are only read off the (swizzled) index
  return launch(h, s, QSV_K_MUX, 32.0 * (double)n, [&] {
    const double* mp = reinterpret_cast<const double*>(dtab);
    if (npairs % (QSV_TPB * 4) == 0 && h->opt_unroll >= 4) {
      const dim3 g(grid_for(h, s, npairs, QSV_TPB * 4));
      if (single_nt(h, 3)) hipLaunchKernelGGL((k_mux<4, false, true>), g, dim3(QSV_TPB), shm, s.stream, s.amp, npairs, t, bl, mp, nmat, swz);
      else           hipLaunchKernelGGL((k_mux<4, false, false>), g, dim3(QSV_TPB), shm, s.stream, s.amp, npairs, t, bl, mp, nmat, swz);
    } else if (npairs % (QSV_TPB * 2) == 0) {
      hipLaunchKernelGGL((k_mux<2, false, false>), dim3(grid_for(h, s, npairs, QSV_TPB * 2)), dim3(QSV_TPB), shm, s.stream, s.amp, npairs, t, bl, mp, nmat, swz);
    } else {
      hipLaunchKernelGGL((k_mux<1, true, false>), dim3(grid_for(h, s, npairs, QSV_TPB)), dim3(QSV_TPB), shm, s.stream, s.amp, npairs, t, bl, mp, nmat, swz);
    }
  });
}

static int apply_gate(qsv_handle* h, int kind, int n, const int* q, const int* vals, int target,
                      const double* data, double angle) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  CHK(validate_gate(h, kind, n, q, target, kind == QSV_OP_MCX || kind == QSV_OP_MCPHASE ? (const void*)h : (const void*)data));
  CHK(materialize_all(h));                         // the one-gate kernels read every amplitude
  LocalOp lo;
  for (Shard& s : h->shards)
    if (resolve_gate(h, s, kind, n, q, vals, target, data, angle, lo)) CHK(run_single(h, s, lo));
  return QSV_OK;
}

extern "C" int qsv_apply_1q(qsv_handle* h, int t, const double m[8]) { return apply_gate(h, QSV_OP_1Q, 0, nullptr, nullptr, t, m, 0); }
extern "C" int qsv_apply_mc1q(qsv_handle* h, int n_ctrl, const int* ctrls, const int* ctrl_vals, int t, const double m[8]) {
  return apply_gate(h, QSV_OP_1Q, n_ctrl, ctrls, ctrl_vals, t, m, 0);
}
extern "C" int qsv_apply_mcx(qsv_handle* h, int n_ctrl, const int* ctrls, const int* ctrl_vals, int t) {
  return apply_gate(h, QSV_OP_MCX, n_ctrl, ctrls, ctrl_vals, t, nullptr, 0);
}
extern "C" int qsv_apply_mcphase(qsv_handle* h, int n_ctrl, const int* ctrls, const int* vals, double angle) {
  return apply_gate(h, QSV_OP_MCPHASE, n_ctrl, ctrls, vals, -1, nullptr, angle);
}
extern "C" int qsv_apply_diag(qsv_handle* h, int k, const int* qubits, const double* table) {
  return apply_gate(h, QSV_OP_DIAG, k, qubits, nullptr, -1, table, 0);
}
extern "C" int qsv_apply_mux_1q(qsv_handle* h, int k, const int* ctrls, int t, const double* mats) {
  return apply_gate(h, QSV_OP_MUX, k, ctrls, nullptr, t, mats, 0);
}
