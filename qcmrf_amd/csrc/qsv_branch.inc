// qsv_branch.inc -- qsv_branch_mass / qsv_branch_split: the host side of the level-wise trajectory walk (part of qsv.hip;
// kernels and the order contract of the sums in qsv_branch.hip)
static int branch_shard(qsv_handle* h, const char* who, const char* role, int w, Shard** out) {
  if (h->multiproc || h->P != 1 || h->shards.size() != 1)
    return fail(QSV_E_BADARG, "%s: the %s handle has %d shards%s; slots live in a single-shard, single-process handle", who, role,
                h->P, h->multiproc ? " over several ranks" : "");
  if (w < 1 || w > h->W) return fail(QSV_E_BADARG, "%s: slot width %d not in [1, %d] (the %s handle's qubits)", who, w, h->W, role);
  *out = &h->shards[0];
  return QSV_OK;
}

extern "C" int qsv_branch_mass(qsv_handle* h, int w, uint64_t n_slots, int qubit, double* out) {
  if (!h || !out) return fail(QSV_E_BADARG, "NULL argument");
  Shard* sp = nullptr;
  CHK(branch_shard(h, "qsv_branch_mass", "state", w, &sp));
  Shard& s = *sp;
  if (qubit < 0 || qubit >= w) return fail(QSV_E_BADARG, "qsv_branch_mass: measured qubit %d not in [0, %d) (inside a slot)", qubit, w);
  const uint64_t max_slots = 1ull << (h->W - w);
  if (n_slots < 1 || n_slots > max_slots)
    return fail(QSV_E_BADARG, "qsv_branch_mass: %llu slots of 2^%d amplitudes; a state of %d qubits holds 1 .. %llu", (unsigned long long)n_slots, w, h->W, (unsigned long long)max_slots);
  CHK(materialize(h, s));                   // realises a deferred state, writes implied zeros: the pass reads every amplitude of the slots
  CHK(shard_set(s));
  const uint64_t n_part = qsv_branch_mass_scratch(w, n_slots);
  double* d_red = nullptr;
  bool temp = false;
  CHK(red_scratch(s, (size_t)(2 * n_slots + n_part), &d_red, &temp));
  double* d_out = d_red;
  double* d_part = d_red + 2 * n_slots;
  int launches = 0;
  hipError_t err = hipSuccess;
  CHK(launch(h, s, QSV_K_PROB, 16.0 * (double)(n_slots << w), [&] {
    err = qsv_branch_mass_launch(s.stream, s.amp, w, n_slots, qubit, d_part, d_out, &launches);
  }));
  HIPCHK(err);
  if (launches > 1) h->stats.per_kind[QSV_K_PROB].launches += (uint64_t)(launches - 1);
  HIPCHK(hipMemcpyAsync(out, d_out, 2 * n_slots * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  if (temp) HIPCHK(hipFree(d_red));
  return QSV_OK;
}

extern "C" int qsv_branch_split(qsv_handle* dst, qsv_handle* src, int w, uint64_t n_children, const uint32_t* parent,
                                const uint8_t* outcome, int qubit, int release) {
  if (!dst || !src || !parent || !outcome) return fail(QSV_E_BADARG, "NULL argument");
  if (dst == src) return fail(QSV_E_BADARG, "qsv_branch_split: source and destination are the same handle");
  Shard *ap = nullptr, *bp = nullptr;
  CHK(branch_shard(src, "qsv_branch_split", "source", w, &ap));
  CHK(branch_shard(dst, "qsv_branch_split", "destination", w, &bp));
  Shard& a = *ap;
  Shard& b = *bp;
  if (a.device != b.device) return fail(QSV_E_BADARG, "qsv_branch_split: source on device %d, destination on device %d", a.device, b.device);
  if (qubit < 0 || qubit >= w) return fail(QSV_E_BADARG, "qsv_branch_split: measured qubit %d not in [0, %d) (inside a slot)", qubit, w);
  const uint64_t dst_slots = 1ull << (dst->W - w), src_slots = 1ull << (src->W - w);
  if (n_children < 1 || n_children > dst_slots)
    return fail(QSV_E_BADARG, "qsv_branch_split: %llu children of 2^%d amplitudes; the destination of %d qubits holds 1 .. %llu", (unsigned long long)n_children, w, dst->W, (unsigned long long)dst_slots);
  for (uint64_t c = 0; c < n_children; ++c) {
    if ((uint64_t)parent[c] >= src_slots) return fail(QSV_E_BADARG, "qsv_branch_split: child %llu has parent %u; the source holds %llu slots", (unsigned long long)c, parent[c], (unsigned long long)src_slots);
    if (outcome[c] > 1) return fail(QSV_E_BADARG, "qsv_branch_split: child %llu has outcome %u (0 or 1)", (unsigned long long)c, (unsigned)outcome[c]);
  }
  // destination after source, source after the split: the two events of qsv_copy_state, no host round trip
  CHK(shard_set(a));
  CHK(materialize(src, a));                 // a deferred source is written, its implied zeros too: the split reads the kept halves as stored
  if (!a.ev_ready) HIPCHK(hipEventCreateWithFlags(&a.ev_ready, hipEventDisableTiming));
  HIPCHK(hipEventRecord(a.ev_ready, a.stream));
  CHK(shard_set(b));
  HIPCHK(hipStreamWaitEvent(b.stream, a.ev_ready, 0));
  // the tables: [parent | outcome] in one buffer, through the destination's arena, or -- beyond a megabyte -- its reduction scratch
  const size_t pbytes = (size_t)n_children * sizeof(uint32_t), tbytes = pbytes + (size_t)n_children;
  char* d_tab = nullptr;
  bool temp = false;
  if (tbytes <= (1u << 20)) {
    std::vector<char> tab(tbytes);
    memcpy(tab.data(), parent, pbytes);
    memcpy(tab.data() + pbytes, outcome, (size_t)n_children);
    void* p = nullptr;
    CHK(arena_put(b, tab.data(), tbytes, &p));
    d_tab = reinterpret_cast<char*>(p);
  } else {
    double* d = nullptr;
    CHK(red_scratch(b, (tbytes + sizeof(double) - 1) / sizeof(double), &d, &temp));
    d_tab = reinterpret_cast<char*>(d);
    const size_t step = b.arena_bytes / 2;               // staged through the arena's pinned half: the caller's buffers are free on return
    void* p = nullptr;
    for (size_t off = 0; off < pbytes; off += step)
      CHK(arena_put(b, reinterpret_cast<const char*>(parent) + off, std::min(step, pbytes - off), &p, d_tab + off));
    for (size_t off = 0; off < (size_t)n_children; off += step)
      CHK(arena_put(b, outcome + off, std::min(step, (size_t)n_children - off), &p, d_tab + pbytes + off));
  }
  const uint64_t n_dst = amps_local(dst);
  hipError_t err = hipSuccess;
  // the destination's old state, deferred or with implied zeros, is gone: every amplitude is stored (launch clears the caches)
  b.zmask = 0;
  CHK(launch(dst, b, QSV_K_SWAP, 16.0 * ((double)n_dst + 0.5 * (double)(n_children << w)), [&] {
    err = qsv_branch_split_launch(b.stream, b.amp, n_dst, a.amp, w, n_children, reinterpret_cast<const uint32_t*>(d_tab),
                                  reinterpret_cast<const uint8_t*>(d_tab + pbytes), qubit, release);
  }));
  HIPCHK(err);
  // the split runs on the DESTINATION's stream: whatever the source is asked to do next must not start before it has been read
  if (!a.ev_copied) HIPCHK(hipEventCreateWithFlags(&a.ev_copied, hipEventDisableTiming));
  HIPCHK(hipEventRecord(a.ev_copied, b.stream));
  CHK(shard_set(a));
  HIPCHK(hipStreamWaitEvent(a.stream, a.ev_copied, 0));
  if (temp) { CHK(shard_set(b)); HIPCHK(hipStreamSynchronize(b.stream)); HIPCHK(hipFree(d_tab)); }
  return QSV_OK;
}
