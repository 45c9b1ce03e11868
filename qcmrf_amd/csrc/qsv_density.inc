// qsv_density.inc -- density-matrix method: qsv_density_exec / _diagonal / _sample (part of qsv.hip; kernels in qsv_density.hip)
// ------------------------------------------------------------------------------------------
// rho of W qubits in the shard of a 2W-qubit handle, rho[i, j] at v = i | (j << W).  The program is the record stream of
// qsv_noisy_sample.  A unitary record runs as itself on the ket bits and as its mirror on the bra bits (qubits + W,
// matrix and table conjugated, angle negated); every maximal run of them is ONE qsv_exec program, so ket and bra gates share
// k_multi passes like any other gates.  PAULI, KRAUS and KRAUS2 records close the run and have kernels of their own; so do the
// MEASURE records of qsv_density_exec_accept (an outcome fixed by the caller, or forgotten: one linear map on rho).
// ------------------------------------------------------------------------------------------
static int dm_check_handle(const qsv_handle* h) {
  if (!h) return fail(QSV_E_BADARG, "NULL handle");
  if (h->multiproc || h->shards.size() != 1) return fail(QSV_E_UNSUPPORTED, "the density-matrix method needs a single-shard handle");
  if (h->W & 1) return fail(QSV_E_BADARG, "a density matrix of W qubits takes a handle of 2W qubits, not %d", h->W);
  return QSV_OK;
}

static inline uint32_t dm_pauli_index(uint32_t x, uint32_t z, int n) {
  uint32_t p = 0;
  for (int j = 0; j < n; ++j) p |= (((x >> j) & 1u) << (2 * j)) | (((z >> j) & 1u) << (2 * j + 1));
  return p;
}

// out[x * 2^n + d] = sum_z p(x, z) (-1)^(z . d), p = the differences of the record's cumulative table.  Host only.
extern "C" int qsv_density_pauli_table(int n, const double* cum, double* out) {
  if (n < 1 || n > 2 || !cum || !out) return fail(QSV_E_BADARG, "a Pauli error acts on 1 or 2 qubits (n = %d) and needs its table", n);
  const uint32_t X = 1u << n;
  for (uint32_t x = 0; x < X; ++x)
    for (uint32_t d = 0; d < X; ++d) {
      double c = 0.0;
      for (uint32_t z = 0; z < X; ++z) {
        const uint32_t p = dm_pauli_index(x, z, n);
        const double pr = cum[p] - (p ? cum[p - 1] : 0.0);
        c += (__builtin_popcount(z & d) & 1) ? -pr : pr;
      }
      out[x * X + d] = c;
    }
  return QSV_OK;
}

// the entry protocol of a kernel that reads and writes the shard behind the engine's bookkeeping (as qsv_apply_kq):
// implied zeros written first; launch() drops the cached sums
// kraus2: the 512 doubles of a KRAUS2 record's superoperator on the host; they are staged in the shard's noisy buffer, in stream
// order behind the kernel of an earlier record that may still read its own
// measure: {release, w0, w1} of a MEASURE record (k_dm_measure: 2 loads and 4 stores per block, 24 B per amplitude)
static int dm_channel(qsv_handle* h, int n, const int* qubits, const DmPauli* pauli, const DmKraus* kraus, const double* kraus2 = nullptr,
                      const double* measure = nullptr) {
  CHK(materialize_all(h));
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  const int W = h->W / 2;
  const uint64_t N = amps_local(h);
  DmLaunch l;
  l.stream = s.stream;
  l.amp = s.amp;
  l.nblocks = N >> (2 * n);
  l.grid = grid_for(h, s, l.nblocks, QSV_TPB);
  l.nt = h->opt_nt < 0 ? h->L >= 26 : h->opt_nt != 0;
  for (int k = 0; k < 4; ++k) l.pos.pos[k] = l.pos.ins[k] = 0;
  for (int k = 0; k < n; ++k) {
    l.pos.pos[k] = qubits[k];
    l.pos.pos[n + k] = qubits[k] + W;
  }
  for (int k = 0; k < 2 * n; ++k) l.pos.ins[k] = l.pos.pos[k];
  std::sort(l.pos.ins, l.pos.ins + 2 * n);
  hipError_t e = hipSuccess;
  if (measure) {
    CHK(launch(h, s, QSV_K_KQ, 24.0 * (double)N, [&] { e = qsv_dm_measure_launch(l, measure[0] != 0.0, measure[1], measure[2]); }));
    HIPCHK(e);
    return QSV_OK;
  }
  if (kraus2) {
    const size_t bytes = QSV_DM_KRAUS2_DOUBLES * sizeof(double);
    if (s.noisy_cap < bytes) {
      if (s.d_noisy) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(s.d_noisy)); }
      s.d_noisy = nullptr;
      s.noisy_cap = 0;
      HIPCHK(hipMalloc(&s.d_noisy, bytes));
      s.noisy_cap = bytes;
    }
    HIPCHK(hipMemcpyAsync(s.d_noisy, kraus2, bytes, hipMemcpyHostToDevice, s.stream));
    CHK(launch(h, s, QSV_K_KQ, 32.0 * (double)N, [&] { e = qsv_dm_kraus2_launch(l, reinterpret_cast<const double*>(s.d_noisy)); }));
    HIPCHK(e);
    return QSV_OK;
  }
  CHK(launch(h, s, QSV_K_KQ, 32.0 * (double)N, [&] { e = pauli ? qsv_dm_pauli_launch(l, n, *pauli) : qsv_dm_kraus_launch(l, *kraus); }));
  HIPCHK(e);
  return QSV_OK;
}

// the body of qsv_density_exec and qsv_density_exec_accept; `accept`: MEASURE records are taken (fix_mask, fix_val: the bits
// whose last write conditions), otherwise refused
static int dm_exec(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data, bool accept,
                   uint64_t fix_mask, uint64_t fix_val) {
  CHK(dm_check_handle(h));
  if (n_ops < 0 || (n_ops && !ops)) return fail(QSV_E_BADARG, "NULL argument");
  const int W = h->W / 2;
  if (W > QSV_DENSITY_MAX_QUBITS) return fail(QSV_E_BADARG, "a density matrix of %d qubits exceeds the %d this method holds", W, QSV_DENSITY_MAX_QUBITS);
  if (fix_val & ~fix_mask)
    return fail(QSV_E_BADARG, "fix_val sets bit %d, which fix_mask does not fix", __builtin_ctzll(fix_val & ~fix_mask));
  int last_write[64];                                      // the MEASURE record that writes a bit last: the one that conditions
  for (int c = 0; c < 64; ++c) last_write[c] = -1;
  auto need = [&](int i, const qsv_op& o, uint64_t cnt) -> int {
    if (!data || o.data_off + cnt > n_data) return fail(QSV_E_BADARG, "op %d: data range [%llu,+%llu) outside pool of %llu", i,
                                                        (unsigned long long)o.data_off, (unsigned long long)cnt, (unsigned long long)n_data);
    return QSV_OK;
  };
  auto below_w = [&](int i, int q) -> int {
    if (q < 0 || q >= W) return fail(QSV_E_BADARG, "op %d: qubit %d not in [0,%d) of the density matrix", i, q, W);
    return QSV_OK;
  };
  // every record is checked before anything runs: a refused program leaves the state as it was
  for (int i = 0; i < n_ops; ++i) {
    const qsv_op& o = ops[i];
    if (o.kind == QSV_OP_IF)
      return fail(QSV_E_UNSUPPORTED, "op %d: QSV_OP_IF (a guard on the shot's classical bits) runs in qsv_noisy_sample only; a density matrix cannot follow a measured bit without branching", i);
    if (o.kind == QSV_OP_RESET)
      return fail(QSV_E_UNSUPPORTED, "op %d: QSV_OP_RESET runs in qsv_noisy_sample only; qsv_density_exec_accept takes a reset as a QSV_OP_MEASURE record with release = 1 whose bit is outside fix_mask", i);
    if (o.n < 0 || o.n > QSV_MAX_CTRL) return fail(QSV_E_BADARG, "op %d: n=%d out of range", i, o.n);
    switch (o.kind) {
      case QSV_OP_INIT_ZERO: break;
      case QSV_OP_INIT_UNIFORM:
        if (o.mask >> W) return fail(QSV_E_BADARG, "op %d: mask has bits beyond qubit %d", i, W - 1);
        break;
      case QSV_OP_1Q: case QSV_OP_MCX: case QSV_OP_DIAG: case QSV_OP_MCPHASE:
        if (o.kind == QSV_OP_1Q || o.kind == QSV_OP_MCX) CHK(below_w(i, o.target));
        for (int b = 0; b < o.n; ++b) CHK(below_w(i, o.qubits[b]));
        if (o.kind == QSV_OP_1Q) CHK(need(i, o, 8));
        if (o.kind == QSV_OP_DIAG) CHK(need(i, o, 2ull << o.n));
        break;
      case QSV_OP_PAULI: {
        if (o.n < 1 || o.n > 2) return fail(QSV_E_BADARG, "op %d: a Pauli error acts on 1 or 2 qubits, not %d", i, o.n);
        for (int b = 0; b < o.n; ++b) CHK(below_w(i, o.qubits[b]));
        if (o.n == 2 && o.qubits[0] == o.qubits[1]) return fail(QSV_E_BADARG, "op %d: duplicate qubit %d in a Pauli error", i, o.qubits[0]);
        const uint64_t np = 1ull << (2 * o.n);
        CHK(need(i, o, np));
        const double* d = data + o.data_off;
        for (uint64_t p = 0; p < np; ++p)
          if (!(d[p] >= (p ? d[p - 1] : 0.0) && d[p] <= 1.0))
            return fail(QSV_E_BADARG, "op %d: cumulative Pauli probabilities must rise from 0 to 1 (entry %llu = %g)", i, (unsigned long long)p, d[p]);
        if (d[np - 1] != 1.0) return fail(QSV_E_BADARG, "op %d: cumulative Pauli probabilities end at %.17g, not 1", i, d[np - 1]);
        break;
      }
      case QSV_OP_KRAUS: {
        if (o.n != 1) return fail(QSV_E_BADARG, "op %d: a Kraus channel acts on 1 qubit, not %d", i, o.n);
        CHK(below_w(i, o.qubits[0]));
        const int m = o.vals[0];
        if (m < 1 || m > 4) return fail(QSV_E_BADARG, "op %d: a Kraus channel has 1 to 4 operators, not %d", i, m);
        CHK(need(i, o, 12ull * m));                        // the record carries its E tables; this method does not read them
        for (int j = 0; j < 8 * m; ++j)
          if (!std::isfinite(data[o.data_off + j])) return fail(QSV_E_BADARG, "op %d: Kraus entry %d is not finite", i, j);
        break;
      }
      case QSV_OP_KRAUS2: {
        if (o.n != 2) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 (a two-qubit Kraus channel) acts on 2 qubits, not %d", i, o.n);
        for (int b = 0; b < 2; ++b)
          if (o.qubits[b] < 0 || o.qubits[b] >= W)
            return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 qubit %d not in [0,%d) of the density matrix", i, o.qubits[b], W);
        if (o.qubits[0] == o.qubits[1]) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 names qubit %d twice", i, o.qubits[0]);
        const int m = o.vals[0];
        if (m < 1 || m > 16) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 has 1 to 16 operators, not %d", i, m);
        CHK(need(i, o, 48ull * m));                        // the record carries its E tables; this method does not read them
        for (int j = 0; j < 32 * m; ++j)
          if (!std::isfinite(data[o.data_off + j])) return fail(QSV_E_BADARG, "op %d: QSV_OP_KRAUS2 entry %d is not finite", i, j);
        break;
      }
      case QSV_OP_MEASURE: {
        if (!accept)
          return fail(QSV_E_UNSUPPORTED, "op %d: QSV_OP_MEASURE (a measurement taken in place) runs in qsv_noisy_sample only; the density-matrix method defers every measurement", i);
        if (o.n != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE measures 1 qubit, not %d", i, o.n);
        if (o.qubits[0] < 0 || o.qubits[0] >= W)
          return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE qubit %d not in [0,%d) of the density matrix", i, o.qubits[0], W);
        if (o.vals[0] < 0 || o.vals[0] >= 64) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE writes classical bit %d, not in [0,64)", i, o.vals[0]);
        if (o.vals[1] != 0 && o.vals[1] != 1) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE release flag %d is not 0 or 1", i, o.vals[1]);
        CHK(need(i, o, 2));
        for (int b = 0; b < 2; ++b) {
          const double f = data[o.data_off + b];
          if (!(f >= 0.0 && f <= 1.0)) return fail(QSV_E_BADARG, "op %d: QSV_OP_MEASURE flip probability P(flip | %d) = %g not in [0, 1]", i, b, f);
        }
        last_write[o.vals[0]] = i;
        break;
      }
      case QSV_OP_MUX: case QSV_OP_KQ: case QSV_OP_SWAP:
        return fail(QSV_E_UNSUPPORTED, "op %d: kind %d is not supported by the density-matrix method (INIT, 1Q, MCX, DIAG, MCPHASE, PAULI, KRAUS, KRAUS2 only)", i, o.kind);
      default:
        return fail(QSV_E_BADARG, "op %d: unknown kind %d", i, o.kind);
    }
  }
  std::vector<qsv_op> run;
  std::vector<double> pool;
  auto flush_run = [&]() -> int {
    if (run.empty()) return QSV_OK;
    if (pool.empty()) pool.push_back(0.0);
    CHK(qsv_exec(h, run.data(), (int)run.size(), pool.data(), pool.size()));
    run.clear();
    pool.clear();
    return QSV_OK;
  };
  qsv_op start;
  memset(&start, 0, sizeof start);
  start.kind = QSV_OP_INIT_ZERO;                           // |0..0><0..0|
  run.push_back(start);
  for (int i = 0; i < n_ops; ++i) {
    const qsv_op& o = ops[i];
    const double* d = data ? data + o.data_off : nullptr;
    switch (o.kind) {
      case QSV_OP_INIT_ZERO:
      case QSV_OP_INIT_UNIFORM: {
        qsv_op u = o;
        u.mask = o.kind == QSV_OP_INIT_UNIFORM ? o.mask | (o.mask << W) : 0ull;
        const bool supersedes = !run.empty() && (run.back().kind == QSV_OP_INIT_ZERO || run.back().kind == QSV_OP_INIT_UNIFORM);
        if (supersedes) run.back() = u; else run.push_back(u);     // an init right after an init: the first is never written
        break;
      }
      case QSV_OP_1Q: case QSV_OP_MCX: case QSV_OP_DIAG: case QSV_OP_MCPHASE: {
        const uint64_t cnt = o.kind == QSV_OP_1Q ? 8 : (o.kind == QSV_OP_DIAG ? 2ull << o.n : 0);
        qsv_op ket = o, bra = o;
        ket.data_off = pool.size();
        pool.insert(pool.end(), d, d + cnt);
        bra.flags &= ~QSV_OPF_NEW_PASS;                    // the pair belongs to one pass where it fits
        bra.target = o.target + W;                         // (unused by DIAG and MCPHASE)
        for (int b = 0; b < o.n; ++b) bra.qubits[b] = o.qubits[b] + W;
        bra.angle = -o.angle;
        bra.data_off = pool.size();
        for (uint64_t e = 0; e < cnt; ++e) pool.push_back((e & 1) ? -d[e] : d[e]);
        run.push_back(ket);
        run.push_back(bra);
        break;
      }
      case QSV_OP_PAULI: {
        CHK(flush_run());
        DmPauli c;
        memset(&c, 0, sizeof c);
        CHK(qsv_density_pauli_table(o.n, d, c.c));
        CHK(dm_channel(h, o.n, o.qubits, &c, nullptr));
        break;
      }
      case QSV_OP_KRAUS: {
        CHK(flush_run());
        const int m = o.vals[0];
        DmKraus s;
        memset(&s, 0, sizeof s);
        for (int k = 0; k < m; ++k) {
          const double* K = d + 8 * k;                     // K[a][a'] at 2 (2a + a')
          for (int e = 0; e < 4; ++e)
            for (int f = 0; f < 4; ++f) {
              const double* x = K + 2 * (2 * (e & 1) + (f & 1));      // K[a][a']
              const double* y = K + 2 * (2 * (e >> 1) + (f >> 1));    // K[b][b'], conjugated
              s.s[8 * e + 2 * f] += x[0] * y[0] + x[1] * y[1];
              s.s[8 * e + 2 * f + 1] += x[1] * y[0] - x[0] * y[1];
            }
        }
        CHK(dm_channel(h, 1, o.qubits, nullptr, &s));
        break;
      }
      case QSV_OP_KRAUS2: {
        CHK(flush_run());
        const int m = o.vals[0];
        std::vector<double> s(QSV_DM_KRAUS2_DOUBLES, 0.0);
        for (int k = 0; k < m; ++k) {
          const double* K = d + 32 * k;                    // K[a][a'] at 2 (4a + a')
          for (int e = 0; e < 16; ++e)
            for (int f = 0; f < 16; ++f) {
              const double* x = K + 2 * (4 * (e & 3) + (f & 3));      // K[a][a']
              const double* y = K + 2 * (4 * (e >> 2) + (f >> 2));    // K[b][b'], conjugated
              s[32 * e + 2 * f] += x[0] * y[0] + x[1] * y[1];
              s[32 * e + 2 * f + 1] += x[1] * y[0] - x[0] * y[1];
            }
        }
        CHK(dm_channel(h, 2, o.qubits, nullptr, nullptr, s.data()));
        break;
      }
      case QSV_OP_MEASURE: {
        CHK(flush_run());
        const int c = o.vals[0];
        double m[3] = {(double)o.vals[1], 1.0, 1.0};      // an outcome nobody fixes, or one overwritten later: forgotten
        if (((fix_mask >> c) & 1ull) && last_write[c] == i) {
          const int v = (int)((fix_val >> c) & 1ull);      // acceptance is on the bit as read: w_b = P(read v | true b)
          m[1] = v == 0 ? 1.0 - d[0] : d[0];
          m[2] = v == 1 ? 1.0 - d[1] : d[1];
        }
        const int own = h->opt_density_measure_kernel;
        if (own > 0 || (own < 0 && o.qubits[0] >= QSV_DM_MEASURE_MIN_QUBIT)) {
          CHK(dm_channel(h, 1, o.qubits, nullptr, nullptr, nullptr, m));
        } else {
          // a low qubit: the same map as the superoperator of sqrt(w0) |0><0| and sqrt(w1) |1><1| (release: sqrt(w1) |0><1|)
          DmKraus s;
          memset(&s, 0, sizeof s);
          s.s[0] = m[1];                                   // S[0][0]: B00 -> B00
          s.s[o.vals[1] ? 6 : 30] = m[2];                  // release: S[0][3], B11 -> B00; else S[3][3]
          CHK(dm_channel(h, 1, o.qubits, nullptr, &s));
        }
        break;
      }
      default: break;
    }
  }
  CHK(flush_run());
  return QSV_OK;
}

extern "C" int qsv_density_exec(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data) {
  return dm_exec(h, ops, n_ops, data, n_data, false, 0, 0);
}

extern "C" int qsv_density_exec_accept(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                                       uint64_t fix_mask, uint64_t fix_val) {
  return dm_exec(h, ops, n_ops, data, n_data, true, fix_mask, fix_val);
}

// Re rho_ii for every i, on the host: one strided read on the device, 2^W doubles (1 MiB at W = 17) across
static int dm_diagonal(qsv_handle* h, std::vector<double>& diag) {
  CHK(dm_check_handle(h));
  const int W = h->W / 2;
  if (W > QSV_DENSITY_MAX_QUBITS) return fail(QSV_E_BADARG, "a density matrix of %d qubits exceeds the %d this method holds", W, QSV_DENSITY_MAX_QUBITS);
  CHK(materialize_all(h));
  Shard& s = h->shards[0];
  CHK(shard_set(s));
  const uint64_t n = 1ull << W;
  if (s.red_cap < 2 * n) {
    if (s.d_red) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(s.d_red)); }
    s.d_red = nullptr;
    s.red_cap = 0;
    HIPCHK(hipMalloc(&s.d_red, 2 * n * sizeof(double)));
    s.red_cap = 2 * n;
  }
  hipError_t e = hipSuccess;
  CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)n, [&] { e = qsv_dm_diag_launch(s.stream, s.amp, W, s.d_red); }));
  HIPCHK(e);
  diag.resize(n);
  HIPCHK(hipMemcpyAsync(diag.data(), s.d_red, n * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  return QSV_OK;
}

extern "C" int qsv_density_diagonal(qsv_handle* h, const int* qubits, int k, double* out, double* trace) {
  CHK(dm_check_handle(h));
  const int W = h->W / 2;
  if (k < 0 || k > W || (k && !qubits) || (k >= 0 && !out)) return fail(QSV_E_BADARG, "the diagonal is taken over 0..%d qubits into a buffer (k = %d)", W, k);
  uint64_t seen = 0;
  for (int b = 0; b < k; ++b) {
    if (qubits[b] < 0 || qubits[b] >= W) return fail(QSV_E_BADARG, "qubit %d not in [0,%d) of the density matrix", qubits[b], W);
    if (seen & (1ull << qubits[b])) return fail(QSV_E_BADARG, "duplicate qubit %d", qubits[b]);
    seen |= 1ull << qubits[b];
  }
  std::vector<double> diag;
  CHK(dm_diagonal(h, diag));
  // ascending i, one thread: the same bits every time
  for (uint64_t j = 0; j < (1ull << k); ++j) out[j] = 0.0;
  double tr = 0.0;
  for (uint64_t i = 0; i < diag.size(); ++i) {
    uint64_t j = 0;
    for (int b = 0; b < k; ++b) j |= ((i >> qubits[b]) & 1ull) << b;
    out[j] += diag[i];
    tr += diag[i];
  }
  if (trace) *trace = tr;
  return QSV_OK;
}

extern "C" int qsv_density_sample(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                                  const double* readout, uint64_t* out_bits) {
  CHK(dm_check_handle(h));
  const int W = h->W / 2;
  if (shots && !out_bits) return fail(QSV_E_BADARG, "NULL argument");
  if (meas_qubits && (n_meas < 0 || n_meas > 64)) return fail(QSV_E_BADARG, "n_meas %d out of range", n_meas);
  if (readout && !meas_qubits) return fail(QSV_E_BADARG, "readout errors need meas_qubits");
  if (meas_qubits)
    for (int j = 0; j < n_meas; ++j)
      if (meas_qubits[j] >= W) return fail(QSV_E_BADARG, "measured qubit %d not in [0,%d) of the density matrix", meas_qubits[j], W);
  if (readout)
    for (int j = 0; j < 2 * n_meas; ++j)
      if (!(readout[j] >= 0.0 && readout[j] <= 1.0)) return fail(QSV_E_BADARG, "readout probability %d = %g not in [0, 1]", j, readout[j]);
  if (shots == 0) return QSV_OK;
  // gather once, scan once (ascending, on the host: 2^W <= 131072 terms), then one search per shot on the device
  std::vector<double> cum;
  CHK(dm_diagonal(h, cum));
  const uint64_t n = cum.size();
  uint64_t last = 0;
  double run = 0.0;
  for (uint64_t i = 0; i < n; ++i) {
    const double p = cum[i] > 0.0 ? cum[i] : 0.0;
    if (p > 0.0) last = i;
    run += p;
    cum[i] = run;
  }
  Shard& s = h->shards[0];
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_pos = up(64 * sizeof(int)), b_ro = up(128 * sizeof(double));
  const size_t bytes = b_pos + b_ro + up(shots * sizeof(uint64_t));
  if (s.noisy_cap < bytes) {
    if (s.d_noisy) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(s.d_noisy)); }
    s.d_noisy = nullptr;
    s.noisy_cap = 0;
    HIPCHK(hipMalloc(&s.d_noisy, bytes));
    s.noisy_cap = bytes;
  }
  std::vector<int> pos(64, -1);
  for (int j = 0; meas_qubits && j < n_meas; ++j) pos[j] = meas_qubits[j] < 0 ? -1 : meas_qubits[j];
  std::vector<double> ro(128, 0.0);
  for (int j = 0; readout && j < 2 * n_meas; ++j) ro[j] = readout[j];
  char* base = s.d_noisy;
  NzMeas meas;
  meas.n = meas_qubits ? n_meas : -1;
  meas.readout = readout && n_meas > 0 ? 0 : -1;
  meas.pos = reinterpret_cast<const int*>(base);
  uint64_t* d_out = reinterpret_cast<uint64_t*>(base + b_pos + b_ro);
  double* d_cum = s.d_red + n;                             // second half of the buffer dm_diagonal sized
  HIPCHK(hipMemcpyAsync(d_cum, cum.data(), n * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(base, pos.data(), 64 * sizeof(int), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(base + b_pos, ro.data(), 128 * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(qsv_dm_sample_launch(s.stream, d_cum, n, last, shots, seed, meas, reinterpret_cast<const double*>(base + b_pos), d_out));
  HIPCHK(hipMemcpyAsync(out_bits, d_out, shots * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  return QSV_OK;
}
