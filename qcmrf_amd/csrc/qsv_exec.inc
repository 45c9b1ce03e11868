// qsv_exec.inc -- batched execution (qsv_exec), instrumentation and options (part of qsv.hip)
// ------------------------------------------------------------------------------------------
// batched execution: resolve per shard, block consecutive gates into k_multi passes
// ------------------------------------------------------------------------------------------
extern "C" int qsv_exec(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data) {
  if (!h || (n_ops && !ops)) return fail(QSV_E_BADARG, "NULL argument");
  const size_t ns = h->shards.size();
  std::vector<PendingGroup> pend(ns);
  auto flush_all = [&](bool final_pass = false) -> int {          // no pass and no X left pending
    for (size_t i = 0; i < ns; ++i) CHK(flush_group_hard(h, h->shards[i], pend[i], final_pass));
    return QSV_OK;
  };
  for (Shard& s : h->shards) s.tile_fresh = false;
  // An init sets a shard's zmask when it is parsed, before anything is written.  If the program fails before that write
  // (a bad op later on), the shard still holds the previous state: its zmask goes back to the one that describes it.
  std::vector<uint64_t> zheld(ns);
  struct InitGuard {
    qsv_handle* h;
    const std::vector<PendingGroup>& pend;
    const std::vector<uint64_t>& zheld;
    ~InitGuard() { for (size_t k = 0; k < pend.size(); ++k) if (pend[k].init) h->shards[k].zmask = zheld[k]; }
  } init_guard{h, pend, zheld};
  // implied zeros left by the previous program: an init supersedes them, anything else sees the zeros written first
  if (n_ops > 0 && ops[0].kind != QSV_OP_INIT_ZERO && ops[0].kind != QSV_OP_INIT_UNIFORM) CHK(materialize_all(h));
  // An init write is pending and nothing has been applied since: an uncontrolled Hadamard on a qubit that is still |0> is
  // part of that write (|0> -> |+>: the qubit joins the uniform mask) -- the same merge the INIT-fused pass is, one step
  // earlier.  The reference's stream opens with H on every variable qubit (QCMRF.py:204-205): gate by gate they cost a
  // pass of 10 and a pass of 4 masked 2x2 (14 dense targets on a 4 + 6 target tile) before the first clique block.
  bool init_streak = false;
  uint64_t init_mask = 0;
  for (int i = 0; i < n_ops; ++i) {
    const qsv_op& o = ops[i];
    h->exec_ops_left = n_ops - i;
    if (o.kind != QSV_OP_IF && (o.n < 0 || o.n > QSV_MAX_CTRL)) return fail(QSV_E_BADARG, "op %d: n=%d out of range", i, o.n);   // an IF record's n is its span
    const double* d = data ? data + o.data_off : nullptr;
    auto need = [&](uint64_t cnt) -> int {
      if (!data || o.data_off + cnt > n_data) return fail(QSV_E_BADARG, "op %d: data range [%llu,+%llu) outside pool of %llu", i,
                                                          (unsigned long long)o.data_off, (unsigned long long)cnt, (unsigned long long)n_data);
      return QSV_OK;
    };
    switch (o.kind) {
      case QSV_OP_INIT_ZERO:
      case QSV_OP_INIT_UNIFORM: {
        for (size_t k = 0; k < ns; ++k) {             // X gates still pending act on a state that is about to be overwritten
          CHK(flush_group(h, h->shards[k], pend[k]));
          pend[k].xframe = 0;
        }
        const uint64_t mask = o.kind == QSV_OP_INIT_ZERO ? 0ull : o.mask;
        if (h->W < 64 && (mask >> h->W)) return fail(QSV_E_BADARG, "mask has bits beyond qubit %d", h->W - 1);
        if (h->opt_multi_r < 1) { CHK(qsv_init_uniform(h, mask)); break; }
        const double val = std::pow(2.0, -0.5 * __builtin_popcountll(mask));
        for (size_t k = 0; k < ns; ++k) {
          const Shard& s = h->shards[k];
          const uint64_t hi = (uint64_t)s.index << h->L;
          pend[k].init = true;
          pend[k].initval = (hi & ~mask) ? 0.0 : val;
          pend[k].nonmask = ~mask & (amps_local(h) - 1);
          zheld[k] = h->shards[k].zmask;
          h->shards[k].zmask = h->opt_zero_tracking ? pend[k].nonmask : 0ull;
        }
        init_streak = h->opt_fold_init_h != 0;
        init_mask = mask;
        break;
      }
      case QSV_OP_1Q: case QSV_OP_MCX: case QSV_OP_DIAG: case QSV_OP_MCPHASE: case QSV_OP_MUX: {
        if ((o.flags & QSV_OPF_NEW_PASS) && h->opt_pass_hints)
          for (size_t k = 0; k < ns; ++k) if (!pend[k].ops.empty()) CHK(flush_group(h, h->shards[k], pend[k]));
        if (o.kind == QSV_OP_1Q) CHK(need(8));
        if (init_streak && o.kind == QSV_OP_1Q && o.n == 0 && o.target >= 0 && o.target < h->W && !((init_mask >> o.target) & 1ull)) {
          const double r = 0.70710678118654752440;
          const double want[8] = {r, 0, r, 0, r, 0, -r, 0};
          bool is_h = true;
          for (int e = 0; e < 8; ++e) is_h = is_h && std::fabs(d[e] - want[e]) <= 1e-15;
          if (is_h) {
            init_mask |= 1ull << o.target;
            const double val = std::pow(2.0, -0.5 * __builtin_popcountll(init_mask));
            for (size_t k = 0; k < ns; ++k) {
              const uint64_t hi = (uint64_t)h->shards[k].index << h->L;
              pend[k].initval = (hi & ~init_mask) ? 0.0 : val;
              pend[k].nonmask = ~init_mask & (amps_local(h) - 1);
              h->shards[k].zmask = h->opt_zero_tracking ? pend[k].nonmask : 0ull;
            }
            h->stats.fused_gates += 1;
            break;
          }
        }
        init_streak = false;
        if (o.kind == QSV_OP_DIAG) CHK(need(2ull << o.n));
        if (o.kind == QSV_OP_MUX) CHK(need(8ull << o.n));
        CHK(validate_gate(h, o.kind, o.n, o.qubits, o.target, o.kind == QSV_OP_MCX || o.kind == QSV_OP_MCPHASE ? (const void*)h : (const void*)d));
        LocalOp lo;
        for (size_t k = 0; k < ns; ++k) {
          Shard& s = h->shards[k];
          if (!resolve_gate(h, s, o.kind, o.n, o.qubits, o.vals, o.target, d, o.angle, lo)) continue;
          if (!groupable(h, lo)) {
            CHK(flush_group_hard(h, s, pend[k]));
            CHK(materialize(h, s));
            CHK(run_single(h, s, lo));
            continue;
          }
          // X frame: an uncontrolled X inside a pass costs nothing -- later ops of the pass are
          // conjugated by it and the pass stores through the XOR-ed address
          const bool frame_ok = h->opt_xframe && !h->opt_zero_tracking && s.zmask == 0 && h->L >= 8;
          if (frame_ok) conjugate_by_xframe(lo, pend[k].xframe);
          if (frame_ok && lo.type == 2 && lo.is_x && lo.cq.empty()) {
            pend[k].xframe ^= 1ull << lo.target;
            h->stats.fused_gates += 1;
            continue;
          }
          if (!group_fits(h, pend[k], lo)) {
            // the closed pass applies what it safely can of the frame by its own store; the op joins the next
            // pass conjugated by what is still pending
            const uint64_t before = pend[k].xframe;
            CHK(flush_group(h, s, pend[k]));
            const uint64_t applied = before ^ pend[k].xframe;
            if (applied) conjugate_by_xframe(lo, applied);   // undo those: X_A (X_F O X_F) X_A = X_(F^A) O X_(F^A)
          }
          group_add(h, s, pend[k], std::move(lo));
        }
        break;
      }
      case QSV_OP_KQ:
        init_streak = false;
        CHK(flush_all());
        for (Shard& s : h->shards) CHK(materialize(h, s));
        CHK(need(2ull << (2 * o.n)));
        CHK(qsv_apply_kq(h, o.n, o.qubits, d));
        break;
      case QSV_OP_SWAP:
        init_streak = false;
        CHK(flush_all());
        for (Shard& s : h->shards) CHK(materialize(h, s));
        CHK(qsv_swap_layout(h, o.n, o.qubits, o.vals));
        break;
      case QSV_OP_PAULI:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_PAULI (a random Pauli) runs in qsv_noisy_sample only, not in qsv_exec", i);
      case QSV_OP_KRAUS:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS (a Kraus channel) runs in qsv_noisy_sample only, not in qsv_exec", i);
      case QSV_OP_KRAUS2:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 (a two-qubit Kraus channel) runs in qsv_noisy_sample only, not in qsv_exec", i);
      case QSV_OP_MEASURE:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE (a measurement taken in place) runs in qsv_noisy_sample only, not in qsv_exec", i);
      case QSV_OP_IF:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_IF (a guard on the shot's classical bits) runs in qsv_noisy_sample only, not in qsv_exec", i);
      case QSV_OP_RESET:
        return fail(QSV_E_BADARG, "op %d: QSV_OP_RESET (a reset taken in place) runs in qsv_noisy_sample only, not in qsv_exec", i);
      default:
        return fail(QSV_E_BADARG, "op %d: unknown kind %d", i, o.kind);
    }
  }
  h->exec_ops_left = 1 << 30;
  CHK(flush_all(true));
  for (Shard& s : h->shards) {
    if (!h->opt_implied_zeros && !s.deferred) CHK(materialize(h, s));   // else the zero region stays implied (s.zmask, materialize); a deferred state has no implied zeros without the option
    s.tile_valid = s.tile_fresh;
    s.tile_fresh = false;
  }
  return QSV_OK;
}

// ------------------------------------------------------------------------------------------
// noisy shots: one trajectory per shot, in LDS (kernel: qsv_noise.hip) or in a slot of device memory (qsv_noise_hbm.hip)
// ------------------------------------------------------------------------------------------
// The qsv_op records are re-encoded once per call into 32-byte records (NzOp, qsv_noise.h: one format for both paths) and
// a pool in which equal tables are stored once (a lowered circuit repeats a handful of matrices thousands of times): every
// trajectory streams the whole list.  Both entry points are nz_run: the checks, the re-encoding (nz_encode), the staging of
// the device copies (nz_stage), the launch fields the kernels share (NzCall) and the copy back.  An entry point says its
// width limit and how it launches: qsv_noisy_sample picks a k_noisy instantiation and lets the launcher size the grid by LDS
// occupancy; qsv_noisy_sample_hbm sizes the grid by the memory its slots need, allocates them and launches k_noisy_hbm.
// What a record does on the device is written once as well (qsv_noise_ops.h).
static inline void nz_put_ctrl(NzOp& c, int q, bool one) {
  c.cmask |= 1u << q;
  if (one) c.cval |= 1u << q;
}
static inline void nz_put_qubit(NzOp& c, int b, int q) {            // read back by nz_qubit
  if (b < 4) c.cmask |= (uint32_t)q << (8 * b);
  else if (b < 8) c.cval |= (uint32_t)q << (8 * (b - 4));
  else c.ql8 |= (uint64_t)q << (8 * (b - 8));
}

struct NzPool {                                                   // each table once, at an even offset (16-byte aligned)
  std::vector<double> pool;
  std::unordered_map<std::string, uint32_t> seen;
  uint32_t put(const double* v, size_t cnt) {
    std::string key(reinterpret_cast<const char*>(v), cnt * sizeof(double));
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    const uint32_t off = (uint32_t)pool.size();
    pool.insert(pool.end(), v, v + cnt);
    if (pool.size() & 1) pool.push_back(0.0);
    seen.emplace(std::move(key), off);
    return off;
  }
};

// the checks both entry points make on everything but the records
static int nz_check_args(qsv_handle* h, const qsv_op* ops, int n_ops, uint64_t shots, const uint64_t* out_bits) {
  if (!h || n_ops < 0 || (n_ops && !ops) || (shots && !out_bits)) return fail(QSV_E_BADARG, "NULL argument");
  if (h->multiproc || h->shards.size() != 1) return fail(QSV_E_UNSUPPORTED, "noisy shots need a single-shard handle");
  return QSV_OK;
}
static int nz_check_meas(qsv_handle* h, const int* meas_qubits, int n_meas, const double* readout) {
  if (meas_qubits && (n_meas < 0 || n_meas > 64)) return fail(QSV_E_BADARG, "n_meas %d out of range", n_meas);
  if (readout && !meas_qubits) return fail(QSV_E_BADARG, "readout errors need meas_qubits");
  if (meas_qubits) for (int j = 0; j < n_meas; ++j) if (meas_qubits[j] >= 0) CHK(check_qubit(h, meas_qubits[j], "measured"));
  if (readout)
    for (int j = 0; j < 2 * n_meas; ++j)
      if (!(readout[j] >= 0.0 && readout[j] <= 1.0)) return fail(QSV_E_BADARG, "readout probability %d = %g not in [0, 1]", j, readout[j]);
  return QSV_OK;
}

// validates every record and appends its compact form to cops, its tables to pool; a MEASURE record is checked against the
// measurement map it writes beside (meas_qubits, n_meas).  fix_mask (qsv_noisy_sample_accept; 0 elsewhere, and the stream is
// then what it was without the parameter): the last MEASURE record to write a bit of it is marked NZ_DECISIVE -- a bit may be
// written twice, and only its last write may end a shot, wherever the record stands: one inside the span of an IF record may be
// skipped, and then abandons nothing.  *written (may be NULL): the bits MEASURE records write.  *has_dynamic: the stream
// holds an IF or a RESET record; every check of QSV_OP_IF is made here, before anything is staged or launched.
static int nz_encode(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data, const int* meas_qubits,
                     int n_meas, std::vector<NzOp>& cops, NzPool& pool, bool* has_kraus, bool* has_measure, bool* has_kraus2,
                     bool* has_dynamic, uint64_t fix_mask = 0, uint64_t* written = nullptr) {
  cops.reserve(n_ops);
  *has_kraus = false;
  *has_measure = false;
  *has_kraus2 = false;
  *has_dynamic = false;
  uint32_t n_measure = 0;                                  // MEASURE and RESET records so far: the draw numbers of stream 3
  int span_end = 0, span_of = -1;                          // records below span_end lie in the span of IF record span_of
  for (int i = 0; i < n_ops; ++i) {
    const qsv_op& o = ops[i];
    if (o.kind == QSV_OP_IF) {                             // n is the span, not a number of listed qubits
      if (i < span_end) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF inside the span of the QSV_OP_IF record %d (guards do not nest)", i, span_of);
      if (o.n < 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF guards a span of %d records, not at least 1", i, o.n);
      if ((int64_t)i + o.n >= (int64_t)n_ops) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF guards %d records, %d follow it", i, o.n, n_ops - 1 - i);
      if (!meas_qubits) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF reads classical bits and needs meas_qubits (full-index words have none)", i);
      if (o.mask == 0) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF compares no classical bit (mask = 0)", i);
      const uint64_t value = (uint64_t)(uint32_t)o.vals[0] | ((uint64_t)(uint32_t)o.vals[1] << 32);
      if (value & ~o.mask) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF value %#llx has bits outside its mask %#llx", i, (unsigned long long)value, (unsigned long long)o.mask);
      if (n_meas < 64 && (o.mask >> n_meas))
        return fail(QSV_E_BADARG, "op %d: QSV_OP_IF mask %#llx reads a classical bit outside the %d bits of the call", i, (unsigned long long)o.mask, n_meas);
      if (o.target != 0 && o.target != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_IF negate flag %d is not 0 or 1", i, o.target);
      NzOp c;
      memset(&c, 0, sizeof c);
      c.kind = NZ_IF;
      c.target = (uint8_t)o.target;
      c.cmask = (uint32_t)o.n;
      c.cval = (uint32_t)o.mask;
      c.off = (uint32_t)(o.mask >> 32);
      c.ql8 = value;
      cops.push_back(c);
      span_end = i + 1 + o.n;
      span_of = i;
      *has_dynamic = true;
      continue;
    }
    if (i < span_end && (o.kind == QSV_OP_INIT_ZERO || o.kind == QSV_OP_INIT_UNIFORM))
      return fail(QSV_E_BADARG, "op %d: an INIT record inside the span of the QSV_OP_IF record %d", i, span_of);
    if (o.n < 0 || o.n > QSV_MAX_CTRL) return fail(QSV_E_BADARG, "op %d: n=%d out of range", i, o.n);
    const double* d = data ? data + o.data_off : nullptr;
    auto need = [&](uint64_t cnt) -> int {
      if (!data || o.data_off + cnt > n_data) return fail(QSV_E_BADARG, "op %d: data range [%llu,+%llu) outside pool of %llu", i,
                                                          (unsigned long long)o.data_off, (unsigned long long)cnt, (unsigned long long)n_data);
      return QSV_OK;
    };
    auto ctrl_mask = [&](NzOp& c) {
      for (int b = 0; b < o.n; ++b) nz_put_ctrl(c, o.qubits[b], o.vals[b] != 0);
    };
    NzOp c;
    memset(&c, 0, sizeof c);
    switch (o.kind) {
      case QSV_OP_INIT_ZERO:
      case QSV_OP_INIT_UNIFORM: {
        const uint64_t mask = o.kind == QSV_OP_INIT_ZERO ? 0ull : o.mask;
        if (mask >> h->W) return fail(QSV_E_BADARG, "op %d: mask has bits beyond qubit %d", i, h->W - 1);
        const double val = std::pow(2.0, -0.5 * __builtin_popcountll(mask));
        c.kind = NZ_INIT;
        c.cmask = (uint32_t)mask;
        c.off = pool.put(&val, 1);
        break;
      }
      case QSV_OP_1Q:
      case QSV_OP_MCX:
        CHK(check_qubit(h, o.target, "target"));
        CHK(check_distinct(h, o.n, o.qubits, o.target));
        c.kind = o.kind == QSV_OP_1Q ? NZ_1Q : NZ_MCX;
        c.target = (uint8_t)o.target;
        ctrl_mask(c);
        if (o.kind == QSV_OP_1Q) { CHK(need(8)); c.off = pool.put(d, 8); }
        break;
      case QSV_OP_DIAG:
        CHK(check_distinct(h, o.n, o.qubits, -1));
        CHK(need(2ull << o.n));
        c.kind = NZ_DIAG;
        c.n = (uint8_t)o.n;
        for (int b = 0; b < o.n; ++b) nz_put_qubit(c, b, o.qubits[b]);
        c.off = pool.put(d, 2ull << o.n);
        break;
      case QSV_OP_MCPHASE: {
        if (o.n < 1) return fail(QSV_E_BADARG, "op %d: a controlled phase needs at least one qubit", i);
        CHK(check_distinct(h, o.n, o.qubits, -1));
        const double cs[2] = {std::cos(o.angle), std::sin(o.angle)};
        c.kind = NZ_MCPHASE;
        ctrl_mask(c);
        c.off = pool.put(cs, 2);
        break;
      }
      case QSV_OP_PAULI: {
        if (o.n < 1 || o.n > 2) return fail(QSV_E_BADARG, "op %d: a Pauli error acts on 1 or 2 qubits, not %d", i, o.n);
        CHK(check_distinct(h, o.n, o.qubits, -1));
        const uint64_t np = 1ull << (2 * o.n);
        CHK(need(np));
        for (uint64_t p = 0; p < np; ++p)
          if (!(d[p] >= (p ? d[p - 1] : 0.0) && d[p] <= 1.0))
            return fail(QSV_E_BADARG, "op %d: cumulative Pauli probabilities must rise from 0 to 1 (entry %llu = %g)", i,
                        (unsigned long long)p, d[p]);
        if (d[np - 1] != 1.0) return fail(QSV_E_BADARG, "op %d: cumulative Pauli probabilities end at %.17g, not 1", i, d[np - 1]);
        c.kind = NZ_PAULI;
        c.n = (uint8_t)o.n;
        for (int b = 0; b < o.n; ++b) nz_put_qubit(c, b, o.qubits[b]);
        c.off = pool.put(d, np);
        break;
      }
      case QSV_OP_KRAUS: {
        if (o.n != 1) return fail(QSV_E_BADARG, "op %d: a Kraus channel acts on 1 qubit, not %d", i, o.n);
        CHK(check_qubit(h, o.qubits[0], "Kraus"));
        const int m = o.vals[0];
        if (m < 1 || m > 4) return fail(QSV_E_BADARG, "op %d: a Kraus channel has 1 to 4 operators, not %d", i, m);
        CHK(need(12ull * m));
        double e00 = 0.0, e11 = 0.0, e01r = 0.0, e01i = 0.0;
        for (int j = 0; j < 12 * m; ++j)
          if (!std::isfinite(d[j])) return fail(QSV_E_BADARG, "op %d: Kraus entry %d is not finite", i, j);
        for (int k = 0; k < m; ++k) {
          const double* e = d + 8 * m + 4 * k;
          if (e[0] < 0.0 || e[1] < 0.0) return fail(QSV_E_BADARG, "op %d: K^dg K of operator %d has a negative diagonal", i, k);
          e00 += e[0]; e11 += e[1]; e01r += e[2]; e01i += e[3];
        }
        if (std::fabs(e00 - 1.0) > 1e-9 || std::fabs(e11 - 1.0) > 1e-9 || std::fabs(e01r) > 1e-9 || std::fabs(e01i) > 1e-9)
          return fail(QSV_E_BADARG, "op %d: the K^dg K of a Kraus channel must sum to the identity (diagonal %.17g, %.17g)", i, e00, e11);
        c.kind = NZ_KRAUS;
        c.target = (uint8_t)o.qubits[0];
        c.n = (uint8_t)m;
        c.off = pool.put(d, 12 * (size_t)m);
        *has_kraus = true;
        break;
      }
      case QSV_OP_KRAUS2: {
        if (o.n != 2) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 (a two-qubit Kraus channel) acts on 2 qubits, not %d", i, o.n);
        for (int b = 0; b < 2; ++b)
          if (o.qubits[b] < 0 || o.qubits[b] >= h->W)
            return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 qubit %d not in [0,%d)", i, o.qubits[b], h->W);
        if (o.qubits[0] == o.qubits[1]) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 names qubit %d twice", i, o.qubits[0]);
        const int m = o.vals[0];
        if (m < 1 || m > 16) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 has 1 to 16 operators, not %d", i, m);
        CHK(need(48ull * m));
        for (int j = 0; j < 48 * m; ++j)
          if (!std::isfinite(d[j])) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 entry %d is not finite", i, j);
        double sum[16] = {0.0};
        for (int k = 0; k < m; ++k) {
          const double* e = d + 32 * m + 16 * k;
          for (int j = 0; j < 4; ++j)
            if (e[j] < 0.0) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2: K^dg K of operator %d has a negative diagonal", i, k);
          for (int j = 0; j < 16; ++j) sum[j] += e[j];
        }
        for (int j = 0; j < 16; ++j)
          if (std::fabs(sum[j] - (j < 4 ? 1.0 : 0.0)) > 1e-9)
            return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2: the K^dg K of a Kraus channel must sum to the identity (packed entry %d sums to %.17g)", i, j, sum[j]);
        c.kind = NZ_KRAUS2;
        c.target = (uint8_t)o.qubits[0];
        c.cmask = (uint32_t)o.qubits[1];
        c.n = (uint16_t)m;
        c.off = pool.put(d, 48 * (size_t)m);
        *has_kraus2 = true;
        break;
      }
      case QSV_OP_MEASURE: {
        if (o.n != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE measures 1 qubit, not %d", i, o.n);
        CHK(check_qubit(h, o.qubits[0], "QSV_OP_MEASURE"));
        if (!meas_qubits) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE writes a classical bit and needs meas_qubits (full-index words have none)", i);
        const int cb = o.vals[0], release = o.vals[1];
        if (cb < 0 || cb >= 64 || cb >= n_meas)
          return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE writes classical bit %d, outside the %d bits of the call", i, cb, n_meas < 64 ? n_meas : 64);
        if (meas_qubits[cb] >= 0)
          return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE writes classical bit %d, which the final draw writes too (meas_qubits[%d] = %d, not -1)", i, cb, cb, meas_qubits[cb]);
        if (release != 0 && release != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE release flag %d is not 0 or 1", i, release);
        CHK(need(2));
        for (int j = 0; j < 2; ++j)
          if (!(d[j] >= 0.0 && d[j] <= 1.0)) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE flip probability %d = %g not in [0, 1]", i, j, d[j]);
        c.kind = NZ_MEASURE;
        c.target = (uint8_t)o.qubits[0];
        c.cmask = (uint32_t)cb | ((uint32_t)release << 8);
        c.cval = n_measure++;                              // the draw number of stream NZ_STREAM_MEASURE
        c.off = pool.put(d, 2);
        *has_measure = true;
        break;
      }
      case QSV_OP_RESET: {
        if (o.n != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_RESET resets 1 qubit, not %d", i, o.n);
        CHK(check_qubit(h, o.qubits[0], "QSV_OP_RESET"));
        c.kind = NZ_RESET;
        c.target = (uint8_t)o.qubits[0];
        c.cmask = 1u << 8;                                 // release, where a MEASURE record has it
        c.cval = n_measure++;                              // the draw number of stream NZ_STREAM_MEASURE
        *has_dynamic = true;
        break;
      }
      default:
        return fail(QSV_E_UNSUPPORTED, "op %d: kind %d is not supported by noisy shots (INIT, 1Q, MCX, DIAG, MCPHASE, PAULI, KRAUS, KRAUS2, MEASURE, IF, RESET only)", i, o.kind);
    }
    cops.push_back(c);
  }
  uint64_t later = 0;                                      // the bits a MEASURE record behind the current one writes
  for (size_t k = cops.size(); k-- > 0;) {
    if (cops[k].kind != NZ_MEASURE) continue;
    const uint64_t bit = 1ull << (cops[k].cmask & 63u);
    if ((fix_mask & bit) && !(later & bit)) cops[k].cmask |= NZ_DECISIVE;
    later |= bit;
  }
  if (written) *written = later;
  return QSV_OK;
}

// the device copies of one call in the shard's noisy buffer: [ops | pool | pos | out], each part 256-byte aligned
struct NzStaged {
  const NzOp* ops;
  const double* pool;
  const int* pos;
  uint64_t* out;
};
static int nz_stage(Shard& s, const std::vector<NzOp>& cops, const std::vector<double>& pool, const int* meas_qubits, int n_meas,
                    uint64_t shots, NzStaged* st) {
  std::vector<int> pos(64, -1);
  for (int j = 0; meas_qubits && j < n_meas; ++j) pos[j] = meas_qubits[j];
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_ops = up(cops.size() * sizeof(NzOp) + 1), b_pool = up(pool.size() * sizeof(double)), b_pos = up(64 * sizeof(int));
  const size_t bytes = b_ops + b_pool + b_pos + up(shots * sizeof(uint64_t));
  if (s.noisy_cap < bytes) {
    if (s.d_noisy) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(s.d_noisy)); }
    s.d_noisy = nullptr;
    s.noisy_cap = 0;
    HIPCHK(hipMalloc(&s.d_noisy, bytes));
    s.noisy_cap = bytes;
  }
  char* base = s.d_noisy;
  st->ops = reinterpret_cast<const NzOp*>(base);
  st->pool = reinterpret_cast<const double*>(base + b_ops);
  st->pos = reinterpret_cast<const int*>(base + b_ops + b_pool);
  st->out = reinterpret_cast<uint64_t*>(base + b_ops + b_pool + b_pos);
  if (!cops.empty()) HIPCHK(hipMemcpyAsync(base, cops.data(), cops.size() * sizeof(NzOp), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(base + b_ops, pool.data(), pool.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(base + b_ops + b_pool, pos.data(), 64 * sizeof(int), hipMemcpyHostToDevice, s.stream));
  return QSV_OK;
}

// records -> compact records, pool and measurement map of one call
static int nz_prepare(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data, const int* meas_qubits,
                      int n_meas, const double* readout, std::vector<NzOp>& cops, NzPool& pool, bool* has_kraus, bool* has_measure,
                      bool* has_kraus2, bool* has_dynamic, NzMeas* meas, uint64_t fix_mask = 0, uint64_t* written = nullptr) {
  CHK(nz_check_meas(h, meas_qubits, n_meas, readout));
  CHK(nz_encode(h, ops, n_ops, data, n_data, meas_qubits, n_meas, cops, pool, has_kraus, has_measure, has_kraus2, has_dynamic, fix_mask, written));
  meas->n = meas_qubits ? n_meas : -1;
  meas->readout = -1;
  meas->pos = nullptr;
  if (readout && n_meas > 0) meas->readout = (int)pool.put(readout, 2 * (size_t)n_meas);
  if (pool.pool.empty()) pool.pool.push_back(0.0);
  if (pool.pool.size() >= (1ull << 31)) return fail(QSV_E_BADARG, "tables of %zu doubles exceed the noisy op stream's offsets", pool.pool.size());
  return QSV_OK;
}

// One call of either path: everything but the width limit (max_w qubits, kept in `where`) and the launch.  launch(s, c, kraus)
// gets the shard, the fields both kernels take and whether the stream holds a Kraus record; it chooses its grid and starts
// its kernel on s.stream.
template <class Launch>
static int nz_run(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data, uint64_t shots, uint64_t seed,
                  const int* meas_qubits, int n_meas, const double* readout, uint64_t* out_bits, int max_w, const char* where,
                  Launch launch) {
  CHK(nz_check_args(h, ops, n_ops, shots, out_bits));
  if (h->W > max_w) return fail(QSV_E_BADARG, "noisy shots keep one %d-qubit state per trajectory in %s: at most %d qubits", h->W, where, max_w);
  std::vector<NzOp> cops;
  NzPool pool;
  bool has_kraus = false, has_measure = false, has_kraus2 = false, has_dynamic = false;
  NzCall c;
  CHK(nz_prepare(h, ops, n_ops, data, n_data, meas_qubits, n_meas, readout, cops, pool, &has_kraus, &has_measure, &has_kraus2, &has_dynamic, &c.meas));
  if (shots == 0) return QSV_OK;
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  NzStaged st;
  CHK(nz_stage(s, cops, pool.pool, meas_qubits, n_meas, shots, &st));
  c.stream = s.stream;
  c.W = h->W;
  c.d_ops = st.ops;
  c.n_ops = (int)cops.size();
  c.d_pool = st.pool;
  c.shots = shots;
  c.seed = seed;
  c.meas.pos = st.pos;
  c.d_out = st.out;
  c.measure = has_measure;
  c.kraus2 = has_kraus2;
  c.dynamic = has_dynamic || h->opt_noisy_dynamic_kernels;
  const int rc = launch(s, c, has_kraus);
  hipError_t e = hipSuccess;
  if (rc == QSV_OK) e = hipMemcpyAsync(out_bits, c.d_out, shots * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
  // Synchronised on every way out, a failed launch included, so that the stream is idle before a caller frees its slots.
  // (For the LDS path the synchronisation after a failed launch is new: nothing runs then, and the error returned is the same.)
  const hipError_t e2 = hipStreamSynchronize(s.stream);
  CHK(rc);
  HIPCHK(e);
  HIPCHK(e2);
  return QSV_OK;
}

extern "C" int qsv_noisy_sample(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                                uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                                const double* readout, uint64_t* out_bits) {
  return nz_run(h, ops, n_ops, data, n_data, shots, seed, meas_qubits, n_meas, readout, out_bits, QSV_NOISY_MAX_QUBITS, "LDS",
                [&](Shard& s, const NzCall& c, bool kraus) -> int {
                  NzLaunch l;
                  static_cast<NzCall&>(l) = c;
                  l.n_cu = s.n_cu;
                  l.max_grid = h->opt_noisy_grid;
                  l.kraus = kraus;
                  unsigned grid = 0;
                  HIPCHK(qsv_noise_launch(l, &grid));
                  return QSV_OK;
                });
}

// The slot path.  The slots are one allocation per call, sized for the grid and freed on every way out (NzSlots), after
// nz_run has synchronised; nothing of them stays on the handle, so a handle that ran 64 GiB of trajectories holds no more
// memory afterwards than one that did not.
struct NzSlots {
  char* p = nullptr;
  ~NzSlots() { if (p) hipFree(p); }
};
// grid = min(shots, noisy_grid if set, workgroups resident at once, slots that fit into 90 % of the free memory), and the
// slots for it
static int nz_hbm_slots(qsv_handle* h, Shard& s, uint64_t shots, NzSlots& slots, uint64_t* workgroups) {
  const uint64_t slot = (uint64_t)16 << h->W;
  uint64_t grid = 0;
  HIPCHK(qsv_noise_hbm_resident(s.n_cu, &grid));
  if (h->opt_noisy_grid > 0 && (uint64_t)h->opt_noisy_grid < grid) grid = (uint64_t)h->opt_noisy_grid;
  if (shots < grid) grid = shots;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t fit = (uint64_t)((double)free_b * 0.9) / slot;
  if (fit < 1)
    return fail(QSV_E_NOMEM, "noisy shots in device memory: one %d-qubit trajectory needs %llu bytes, %llu bytes are free (qsv_device_memory)",
                h->W, (unsigned long long)slot, (unsigned long long)free_b);
  if (fit < grid) grid = fit;
  if (hipMalloc(&slots.p, grid * slot) != hipSuccess) {
    slots.p = nullptr;
    (void)hipGetLastError();
    return fail(QSV_E_NOMEM, "noisy shots in device memory: %llu slots of %llu bytes need %llu bytes, %llu bytes are free (qsv_device_memory)",
                (unsigned long long)grid, (unsigned long long)slot, (unsigned long long)(grid * slot), (unsigned long long)free_b);
  }
  *workgroups = grid;
  return QSV_OK;
}
extern "C" int qsv_noisy_sample_hbm(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                                    uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                                    const double* readout, uint64_t* out_bits) {
  NzSlots slots;
  return nz_run(h, ops, n_ops, data, n_data, shots, seed, meas_qubits, n_meas, readout, out_bits, QSV_NOISY_HBM_MAX_QUBITS,
                "a slot of device memory", [&](Shard& s, const NzCall& c, bool) -> int {
    uint64_t grid = 0;
    CHK(nz_hbm_slots(h, s, shots, slots, &grid));
    NzHbmLaunch l;
    static_cast<NzCall&>(l) = c;
    l.grid = (unsigned)grid;
    l.d_slots = slots.p;
    HIPCHK(qsv_noise_hbm_launch(l));
    return QSV_OK;
  });
}

// Noisy shots kept only when fixed bits read given values (the contract is in include/qsv.h).  Attempts are launched in rounds
// on the accept-aware kernels; the host keeps the words that satisfy the predicate, in ascending attempt index, until it has
// `shots` of them.  What is returned is a function of the attempts' words alone: the rounds only decide how much work past
// the last accepted attempt is thrown away.
#define QSV_NZ_ACCEPT_ROUND_MIN 64ull            // attempts of a round chosen here at least: below this a launch is all overhead
#define QSV_NZ_ACCEPT_ROUND_MAX (1ull << 20)     // and at most: 8 MiB of words on the device and on the host

// the checks of the fixed bits; `written` = the bits MEASURE records write
static int nz_check_accept(qsv_handle* h, const int* meas_qubits, int n_meas, uint64_t fix_mask, uint64_t fix_val, uint64_t written) {
  for (int b = 0; b < 64; ++b) {
    const uint64_t bit = 1ull << b;
    if ((fix_val & bit) && !(fix_mask & bit)) return fail(QSV_E_BADARG, "fix_val sets bit %d, which fix_mask does not fix", b);
    if (!(fix_mask & bit)) continue;
    if (!meas_qubits) {
      if (b >= h->W) return fail(QSV_E_BADARG, "fix_mask fixes bit %d, beyond the %d qubits of the full-index word", b, h->W);
      continue;
    }
    if (b >= n_meas) return fail(QSV_E_BADARG, "fix_mask fixes bit %d, outside the %d bits of the call", b, n_meas);
    if (meas_qubits[b] < 0 && !(written & bit))
      return fail(QSV_E_BADARG, "fix_mask fixes bit %d, which neither the final draw (meas_qubits[%d] = -1) nor a QSV_OP_MEASURE record writes", b, b);
  }
  return QSV_OK;
}

// attempts of the next round when the library chooses: about `shots` at first, then what the acceptance seen so far asks for
// the shots still missing, a quarter more; four times what was examined while nothing has been accepted yet
static uint64_t nz_accept_round(uint64_t shots, uint64_t accepted, uint64_t examined, uint64_t cap) {
  double want;
  if (examined == 0) want = (double)shots;
  else if (accepted == 0) want = 4.0 * (double)examined;
  else want = 1.25 * (double)(shots - accepted) * (double)examined / (double)accepted;
  uint64_t n = want >= (double)cap ? cap : (uint64_t)want;
  if (n < QSV_NZ_ACCEPT_ROUND_MIN) n = QSV_NZ_ACCEPT_ROUND_MIN;
  return n < cap ? n : cap;
}

extern "C" int qsv_noisy_sample_accept(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                                       uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas, const double* readout,
                                       uint64_t fix_mask, uint64_t fix_val, uint64_t first_shot, uint64_t max_attempts,
                                       uint64_t round, int hbm, uint64_t* out_bits, uint64_t* out_shot, uint64_t* accepted,
                                       uint64_t* attempts) {
  CHK(nz_check_args(h, ops, n_ops, shots, out_bits));
  if (!accepted || !attempts) return fail(QSV_E_BADARG, "NULL argument");
  *accepted = *attempts = 0;
  const int max_w = hbm ? QSV_NOISY_HBM_MAX_QUBITS : QSV_NOISY_MAX_QUBITS;
  if (h->W > max_w)
    return fail(QSV_E_BADARG, "noisy shots keep one %d-qubit state per trajectory in %s: at most %d qubits", h->W,
                hbm ? "a slot of device memory" : "LDS", max_w);
  std::vector<NzOp> cops;
  NzPool pool;
  bool has_kraus = false, has_measure = false, has_kraus2 = false, has_dynamic = false;
  uint64_t written = 0;
  NzCall c;
  CHK(nz_prepare(h, ops, n_ops, data, n_data, meas_qubits, n_meas, readout, cops, pool, &has_kraus, &has_measure, &has_kraus2, &has_dynamic, &c.meas,
                 fix_mask, &written));
  CHK(nz_check_accept(h, meas_qubits, n_meas, fix_mask, fix_val, written));
  if (shots == 0) return QSV_OK;
  if (max_attempts == 0) return fail(QSV_E_BADARG, "max_attempts = 0 with %llu shots to accept", (unsigned long long)shots);
  if (first_shot + max_attempts < first_shot) return fail(QSV_E_BADARG, "first_shot + max_attempts exceeds 64 bits");
  // the words buffer holds the largest round
  uint64_t cap = round ? round : QSV_NZ_ACCEPT_ROUND_MAX;
  if (cap > max_attempts) cap = max_attempts;
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  NzStaged st;
  CHK(nz_stage(s, cops, pool.pool, meas_qubits, n_meas, cap, &st));       // ops, pool and map: once per call
  c.stream = s.stream;
  c.W = h->W;
  c.d_ops = st.ops;
  c.n_ops = (int)cops.size();
  c.d_pool = st.pool;
  c.seed = seed;
  c.meas.pos = st.pos;
  c.d_out = st.out;
  c.measure = has_measure;
  c.kraus2 = has_kraus2;
  c.dynamic = has_dynamic || h->opt_noisy_dynamic_kernels;
  // and the slots: as a plain call of max(64, 4 shots) shots would size them, so that a call for a few shots does not take the
  // memory of a full grid; a round of more attempts runs them in these
  NzSlots slots;
  uint64_t slot_grid = 0;
  const uint64_t slot_shots = shots < 16 ? 64 : shots < (QSV_NZ_ACCEPT_ROUND_MAX >> 2) ? shots << 2 : QSV_NZ_ACCEPT_ROUND_MAX;
  int rc = hbm ? nz_hbm_slots(h, s, slot_shots < cap ? slot_shots : cap, slots, &slot_grid) : QSV_OK;
  std::vector<uint64_t> words;
  uint64_t got = 0, examined = 0;
  hipError_t e = hipSuccess;
  while (rc == QSV_OK && e == hipSuccess && got < shots && examined < max_attempts) {
    uint64_t n = round ? round : nz_accept_round(shots, got, examined, cap);
    if (n > max_attempts - examined) n = max_attempts - examined;
    const NzAccept a = {first_shot + examined, fix_mask, fix_val};
    c.shots = n;
    if (hbm) {
      NzHbmLaunch l;
      static_cast<NzCall&>(l) = c;
      l.grid = (unsigned)(n < slot_grid ? n : slot_grid);
      l.d_slots = slots.p;
      e = qsv_noise_hbm_launch_accept(l, a);
    } else {
      NzLaunch l;
      static_cast<NzCall&>(l) = c;
      l.n_cu = s.n_cu;
      l.max_grid = h->opt_noisy_grid;
      l.kraus = has_kraus;
      unsigned grid = 0;
      e = qsv_noise_launch_accept(l, a, &grid);
    }
    if (e != hipSuccess) break;
    words.resize(n);
    e = hipMemcpyAsync(words.data(), c.d_out, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
    if (e != hipSuccess) break;
    e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) break;
    uint64_t i = 0;
    for (; i < n && got < shots; ++i)
      if ((words[i] & fix_mask) == fix_val) {
        out_bits[got] = words[i];
        if (out_shot) out_shot[got] = a.first_shot + i;
        ++got;
      }
    examined += got == shots ? i : n;                      // up to the last accepted attempt, or the whole round
  }
  // idle on every way out, before the slots are freed
  const hipError_t e2 = hipStreamSynchronize(s.stream);
  CHK(rc);
  HIPCHK(e);
  HIPCHK(e2);
  *accepted = got;
  *attempts = examined;
  return QSV_OK;
}

// ------------------------------------------------------------------------------------------
// instrumentation
// ------------------------------------------------------------------------------------------
extern "C" int qsv_set_profiling(qsv_handle* h, int on) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  if (!on) CHK(drain_pending(h));
  h->profiling = on != 0;
  return QSV_OK;
}
extern "C" int qsv_reset_stats(qsv_handle* h) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  CHK(drain_pending(h));
  memset(&h->stats, 0, sizeof h->stats);
  return QSV_OK;
}
extern "C" int qsv_get_stats(qsv_handle* h, qsv_stats* out) {
  if (!h || !out) return fail(QSV_E_BADARG, "NULL argument");
  CHK(qsv_sync(h));
  CHK(drain_pending(h));
  *out = h->stats;
  return QSV_OK;
}
extern "C" int qsv_state_info(qsv_handle* h, int* deferred, uint64_t* realize_calls, uint64_t* listed_launches) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  int d = 0;
  for (const Shard& s : h->shards) d |= s.deferred ? 1 : 0;
  if (deferred) *deferred = d;
  if (realize_calls) *realize_calls = h->n_realize;
  if (listed_launches) *listed_launches = h->n_listed;
  return QSV_OK;
}
extern "C" int qsv_tile_sums(qsv_handle* h, int shard, double* out, uint64_t cap, uint64_t* n) {
  if (!h || !n) return fail(QSV_E_BADARG, "NULL argument");
  if (shard < 0 || shard >= (int)h->shards.size()) return fail(QSV_E_BADARG, "shard %d of %zu", shard, h->shards.size());
  Shard& s = h->shards[shard];
  if (!s.tile_valid) return fail(QSV_E_BADARG, "the last pass left no tile sums on shard %d", shard);
  *n = s.tile_nblocks;
  if (!out) return QSV_OK;
  if (cap < s.tile_nblocks) return fail(QSV_E_BADARG, "room for %llu tile sums, %llu needed", (unsigned long long)cap, (unsigned long long)s.tile_nblocks);
  CHK(shard_set(s));
  HIPCHK(hipMemcpyAsync(out, s.d_tsums, s.tile_nblocks * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  return QSV_OK;
}
extern "C" int qsv_tile_sums_info(qsv_handle* h, int shard, int* factored, int* d_bits, int* inner_factors, int* uniform_factors) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  if (shard < 0 || shard >= (int)h->shards.size()) return fail(QSV_E_BADARG, "shard %d of %zu", shard, h->shards.size());
  const Shard& s = h->shards[shard];
  if (!s.tile_valid || !s.sums_from_gen) return fail(QSV_E_BADARG, "the last pass on shard %d was no generator leaving tile sums", shard);
  if (factored) *factored = s.sums_info[0];
  if (d_bits) *d_bits = s.sums_info[1];
  if (inner_factors) *inner_factors = s.sums_info[2];
  if (uniform_factors) *uniform_factors = s.sums_info[3];
  return QSV_OK;
}
extern "C" int qsv_timer_begin(qsv_handle* h) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  if (!h->t0) { HIPCHK(hipEventCreate(&h->t0)); HIPCHK(hipEventCreate(&h->t1)); }
  HIPCHK(hipEventRecord(h->t0, s.stream));
  return QSV_OK;
}
extern "C" int qsv_timer_end(qsv_handle* h, double* ms) {
  if (!h || !ms || !h->t0) return fail(QSV_E_BADARG, "timer not started");
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  HIPCHK(hipEventRecord(h->t1, s.stream));
  HIPCHK(hipEventSynchronize(h->t1));
  float f = 0.f;
  HIPCHK(hipEventElapsedTime(&f, h->t0, h->t1));
  *ms = f;
  return QSV_OK;
}
extern "C" int qsv_set_option(qsv_handle* h, const char* name, int value) {
  if (!h || !name) return fail(QSV_E_BADARG, "NULL argument");
  if (!strcmp(name, "blocks_per_cu")) { if (value < 1) return fail(QSV_E_BADARG, "blocks_per_cu < 1"); h->opt_blocks_per_cu = value; }
  else if (!strcmp(name, "unroll")) h->opt_unroll = value;
  else if (!strcmp(name, "lowt_shuffle")) h->opt_lowt_shuffle = value;
  else if (!strcmp(name, "nontemporal")) h->opt_nt = value;
  else if (!strcmp(name, "lane_targets")) h->opt_lane_targets = value != 0;
  else if (!strcmp(name, "cache_sums")) h->opt_cache_sums = value != 0;
  else if (!strcmp(name, "fused_sums")) h->opt_fused_sums = value != 0;
  else if (!strcmp(name, "pair_variant")) h->opt_pair_variant = value;
  else if (!strcmp(name, "kq_mfma")) h->opt_kq_mfma = value != 0;
  else if (!strcmp(name, "zero_tracking")) h->opt_zero_tracking = value != 0;
  else if (!strcmp(name, "implied_zeros")) h->opt_implied_zeros = value != 0;
  else if (!strcmp(name, "lane_map")) h->opt_lane_map = value;
  else if (!strcmp(name, "lane_map_min_l")) h->opt_lane_map_min_l = value;
  else if (!strcmp(name, "init_prod_bit0")) h->opt_init_prod_bit0 = value;
  else if (!strcmp(name, "init_prod_r")) { if (value != 0 && (value < 3 || value > 6)) return fail(QSV_E_BADARG, "init_prod_r must be 0 (auto) or 3..6"); h->opt_init_prod_r = value; }
  else if (!strcmp(name, "init_prod")) h->opt_init_prod = value != 0;
  else if (!strcmp(name, "pass_hints")) h->opt_pass_hints = value != 0;
  else if (!strcmp(name, "dyn_lanes")) { if (value < 0 || value > 3) return fail(QSV_E_BADARG, "dyn_lanes out of range"); h->opt_dyn_lanes = value; }
  else if (!strcmp(name, "xframe")) h->opt_xframe = value != 0;
  else if (!strcmp(name, "multi_nt")) h->opt_multi_nt = value;
  else if (!strcmp(name, "init_prod_nt")) h->opt_init_prod_nt = value;
  else if (!strcmp(name, "init_prod_grid")) { if (value < 0) return fail(QSV_E_BADARG, "init_prod_grid < 0"); h->opt_init_prod_grid = value; }
  else if (!strcmp(name, "sums_factored")) { if (value < -1 || value > 1) return fail(QSV_E_BADARG, "sums_factored must be -1 (auto), 0 or 1"); h->opt_sums_factored = value; }
  else if (!strcmp(name, "defer_state")) { if (value < -1 || value > 1) return fail(QSV_E_BADARG, "defer_state must be -1 (auto), 0 or 1"); h->opt_defer_state = value; }
  else if (!strcmp(name, "sample_chain")) { if (value < 0 || value > 1) return fail(QSV_E_BADARG, "sample_chain must be 0 or 1"); h->opt_sample_chain = value; }
  else if (!strcmp(name, "density_measure_kernel")) { if (value < -1 || value > 1) return fail(QSV_E_BADARG, "density_measure_kernel must be -1 (auto), 0 or 1"); h->opt_density_measure_kernel = value; }
  else if (!strcmp(name, "post_select_list")) { if (value < -1 || value > 1) return fail(QSV_E_BADARG, "post_select_list must be -1 (auto), 0 or 1"); h->opt_post_select_list = value; }
  else if (!strcmp(name, "init_prod_group")) { if (value < -1 || value > QSV_PROD_MAXG) return fail(QSV_E_BADARG, "init_prod_group must be -1 (auto) or 0..4"); h->opt_init_prod_group = value; }
  else if (!strcmp(name, "pass_max_ops")) { if (value < 1 || value > 512) return fail(QSV_E_BADARG, "pass_max_ops out of range"); h->opt_pass_max_ops = value; }
  else if (!strcmp(name, "single_shortcut")) h->opt_single_shortcut = value != 0;
  else if (!strcmp(name, "trace_passes")) h->opt_trace_passes = value != 0;
  else if (!strcmp(name, "noisy_dynamic_kernels")) { if (value < 0 || value > 1) return fail(QSV_E_BADARG, "noisy_dynamic_kernels not 0 or 1"); h->opt_noisy_dynamic_kernels = value; }
  else if (!strcmp(name, "noisy_grid")) { if (value < 0) return fail(QSV_E_BADARG, "noisy_grid < 0"); h->opt_noisy_grid = value; }
  else if (!strcmp(name, "pass_budget")) { if (value < 0) return fail(QSV_E_BADARG, "pass_budget < 0"); h->opt_pass_budget = value; }
  else if (!strcmp(name, "fold_init_h")) h->opt_fold_init_h = value != 0;
  else if (!strcmp(name, "general_combos")) h->opt_general_combos = value != 0;
  else if (!strcmp(name, "lowctl_mask")) h->opt_lowctl_mask = value != 0;
  else if (!strcmp(name, "kq_chunked")) h->opt_kq_chunked = value != 0;
  else if (!strcmp(name, "kq_variant")) h->opt_kq_variant = (int)value;
  else if (!strcmp(name, "kq_debug")) {
    // measurement knob (scripts/kq_variants.py, kq_lds_case.py): the LDS-staged dense-gate kernel with a part of its work
    // left out -- the state it leaves is NOT the gate's result, so it takes an explicit opt-in from the environment
    if (value != 0 && !getenv("QSV_MEASUREMENT_KNOBS")) return fail(QSV_E_BADARG, "kq_debug leaves a wrong state behind; set QSV_MEASUREMENT_KNOBS=1 to time with it");
    h->opt_kq_debug = (int)value;
  }
  else if (!strcmp(name, "kq_order")) { if (value < 0 || value > 4) return fail(QSV_E_BADARG, "kq_order must be 0..4"); h->opt_kq_order = (int)value; }
  else if (!strcmp(name, "kq3_tile")) h->opt_kq3_tile = (int)value;
  else if (!strcmp(name, "kq_blocks_per_cu")) h->opt_kq_blocks_per_cu = (int)value;
  else if (!strcmp(name, "kq_grid")) { if (value < 0) return fail(QSV_E_BADARG, "kq_grid < 0"); h->opt_kq_grid = value; }
  else if (!strcmp(name, "marginals_grid")) { if (value < 0) return fail(QSV_E_BADARG, "marginals_grid < 0"); h->opt_marginals_grid = value; }
  else if (!strcmp(name, "marginals_rows")) { if (value < 0) return fail(QSV_E_BADARG, "marginals_rows < 0"); h->opt_marginals_rows = value; }
  else if (!strcmp(name, "top_grid")) { if (value < 0) return fail(QSV_E_BADARG, "top_grid < 0"); h->opt_top_grid = value; }
  else if (!strcmp(name, "blocksum_variant")) h->opt_blocksum_variant = value & 7;
  else if (!strcmp(name, "swizzle")) h->opt_swz = value < 0 ? 0 : (value > 2 ? 2 : value);
  else if (!strcmp(name, "general_light_r")) { if (value < 1 || value > QSV_GENERAL_MAXR) return fail(QSV_E_BADARG, "general_light_r out of range"); h->opt_general_light_r = value; }
  else if (!strcmp(name, "general_r")) { if (value < 1 || value > QSV_GENERAL_MAXR) return fail(QSV_E_BADARG, "general_r out of range"); h->opt_general_r = value; }
  else if (!strcmp(name, "multi_r")) { if (value < 0 || value > QSV_MULTI_MAXR) return fail(QSV_E_BADARG, "multi_r out of range"); h->opt_multi_r = value; }
  else if (!strcmp(name, "exchange_chunk_log2")) { if (value < 4 || value > 32) return fail(QSV_E_BADARG, "exchange_chunk_log2 out of range"); h->opt_xchunk = 1ull << value; }
  else return fail(QSV_E_BADARG, "unknown option %s", name);
  return QSV_OK;
}
extern "C" const char* qsv_last_error(void) { return g_err.c_str(); }
extern "C" const char* qsv_version(void) { return "qsv 0.1 (gfx950)"; }
