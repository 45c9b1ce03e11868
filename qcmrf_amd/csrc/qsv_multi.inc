// qsv_multi.inc -- grouping of consecutive gates into register-tiled k_multi passes, zero tracking (part of qsv.hip)
// ------------------------------------------------------------------------------------------
// k_multi pass: a run of resolved gates on <= opt_multi_r distinct targets, one HBM sweep
// ------------------------------------------------------------------------------------------
struct PendingGroup {
  std::vector<LocalOp> ops;
  std::vector<int> targets;       // distinct target bits, in first-use order
  std::vector<int> selects;       // every table-select bit used by a table op of the group
  std::vector<int> lane_targets;  // targets on address bits < 6, handled by wave shuffles (no register bit)
  std::vector<int> dyn_targets;   // targets >= 6 riding on a borrowed lane bit (3..5) for this pass only
  bool lane_mode = false;         // decided when the group opens: lane bits are really the lane id
  bool opened = false;
  bool simple = true;             // only table ops, and no select bit is a target of the group
  size_t table_cplx = 0;
  bool init = false;              // an init write is waiting to be merged into the pass
  uint64_t nonmask = 0;
  double initval = 0;
  // X frame: local bits on which an uncontrolled X is still pending.  Such a gate is no data
  // movement: every later op is conjugated by it (conjugate_by_xframe) and a pass stores each
  // amplitude at (address XOR frame) -- for the bits where that is race-free (flush_group: the
  // register and lane bits of a read+write pass, every bit of a write-only one).  The other bits
  // stay pending: flush_group hands them to the next group, and the X gates of a +-flag pair
  // (QCMRF.py:224-227) cancel there without ever having moved an amplitude.
  uint64_t xframe = 0;
  double cost = 0;                // arithmetic of the pass so far, in units of pass_budget (group_fits)
};

static bool has_bit(const std::vector<int>& v, int q) { return std::find(v.begin(), v.end(), q) != v.end(); }

// O -> X_F O X_F for the X gates pending on the bits of F: control values and table selects on
// those bits flip, a 2x2 on such a target has rows and columns swapped
static void conjugate_by_xframe(LocalOp& lo, uint64_t F) {
  if (!F) return;
  auto xmx = [](double* m) { for (int i = 0; i < 2; ++i) { std::swap(m[i], m[6 + i]); std::swap(m[2 + i], m[4 + i]); } };
  if (lo.type == 2 || lo.type == 3) {
    for (size_t k = 0; k < lo.cq.size(); ++k) if ((F >> lo.cq[k]) & 1ull) lo.cv[k] ^= 1;
    if (lo.type == 2 && !lo.is_x && ((F >> lo.target) & 1ull)) xmx(lo.m);
    return;
  }
  const size_t ent = lo.type == 0 ? 8 : 2;
  unsigned flip = 0;
  for (size_t e = 0; e < lo.list.size(); ++e) if ((F >> lo.list[e]) & 1ull) flip |= 1u << e;
  if (flip) {
    std::vector<double> t(lo.table.size());
    const size_t nent = lo.table.size() / ent;
    for (size_t j = 0; j < nent; ++j) memcpy(&t[j * ent], &lo.table[(j ^ flip) * ent], ent * sizeof(double));
    lo.table.swap(t);
  }
  if (lo.type == 0 && ((F >> lo.target) & 1ull))
    for (size_t j = 0; j < lo.table.size() / 8; ++j) xmx(&lo.table[j * 8]);
}

// Arithmetic an op adds to a general (MODE 0) pass, in PERCENT of the time one read + write of the
// shard takes -- both scale with the number of amplitudes, so the figures hold at any width.
// Measured on MI355X at R = 4 (scripts/pass_budget.py, profiles/r02w_pass_budget.log; 60 ops of one kind
// in a pass at 28 qubits against 1.6 ms for the bare pass, after the in-place rewrite of the general
// kernel): controlled X 31 us = 1.9 % on a register target and 74 us on a lane target, controlled
// phase 51 us, 2x2 72 us (96 us on a lane target), table ops with a register select 100 / 170 us.
// opt_pass_budget (percent, default 0 = off) cuts a general pass when the sum exceeds it, which
// keeps each pass nearer the HBM roofline -- but measured on the unfused reference stream the TOTAL
// does not fall: arithmetic beyond what the memory time hides costs the same wherever it runs,
// and more passes add memory time (28 qubits: 9 passes = 32.5 ms unlimited, 24 passes = 42.9 ms at
// budget 100, profiles/r02v_pass_budget.log).  Hence an experiment knob, not a default.
static double op_cost(const LocalOp& lo, bool lane_target, const std::vector<int>& reg_targets) {
  auto reg_select = [&]() { for (int q : lo.list) if (has_bit(reg_targets, q)) return true; return false; };
  switch (lo.type) {
    case 0: return reg_select() ? 6.3 : (lane_target ? 6.0 : 4.5);     // table 2x2 per pair
    case 1: return reg_select() ? 10.6 : 2.0;                          // table phase per amplitude
    case 2: return lo.is_x ? (lane_target ? 4.6 : 1.9) : (lane_target ? 6.0 : 4.5);   // masked swap | masked 2x2
    default: return 3.2;                                               // masked phase
  }
}

static size_t table_cplx_of(const LocalOp& lo) {
  if (lo.type == 0) return (size_t)4 << lo.list.size();
  if (lo.type == 1) return (size_t)1 << lo.list.size();
  return 0;
}
// complex table entries one pass may stage: 40 KiB of LDS, less the identity table flush_group appends
#define QSV_MULTI_TABLE_CPLX (2560 - 4)
static bool groupable(const qsv_handle* h, const LocalOp& lo) {
  if (h->opt_multi_r < 1) return false;
  if ((lo.type == 0 || lo.type == 1) && (int)lo.list.size() > QSV_MULTI_MAXLIST) return false;
  // a table no pass can hold (a mux with 10 selects: 4096 entries): group_add would take it into an empty group all
  // the same, and the pass would ask for more dynamic LDS than k_multi may have.  It runs as its dedicated kernel.
  if (table_cplx_of(lo) > QSV_MULTI_TABLE_CPLX) return false;
  return true;
}

// lane bits 3..5 in use: static lane targets sitting there plus borrowed ones
static int high_lanes_used(const PendingGroup& g) {
  int n = (int)g.dyn_targets.size();
  for (int q : g.lane_targets) if (q >= 3) ++n;
  return n;
}

// would the group still be "simple" (table ops only, selects disjoint from register targets)?
// as_reg: lo's target would become a register target (else it rides on a lane bit / has none)
static bool stays_simple(const PendingGroup& g, const LocalOp& lo, bool as_reg) {
  if (!g.simple || lo.type > 1) return false;
  for (int q : lo.list) if (has_bit(g.targets, q) || q == lo.target) return false;
  if (as_reg && lo.target >= 0 && has_bit(g.selects, lo.target)) return false;
  return true;
}

// Where does lo's target go if lo joins group g?
enum Place { PL_NONE, PL_REG_OLD, PL_REG_NEW, PL_LANE_OLD, PL_LANE_NEW, PL_DYN_NEW, PL_REJECT };
static Place place_target(const qsv_handle* h, const PendingGroup& g, const LocalOp& lo) {
  const int t = lo.target;
  if (t < 0) return PL_NONE;
  if (has_bit(g.targets, t)) return PL_REG_OLD;
  if (g.lane_mode && (has_bit(g.lane_targets, t) || has_bit(g.dyn_targets, t))) return PL_LANE_OLD;
  if (g.lane_mode && t < 6) {
    if (g.lane_targets.size() >= 6) return PL_REJECT;
    if (t >= 3 && high_lanes_used(g) >= 3) return PL_REJECT;      // its lane bit is lent out in this pass
    return PL_LANE_NEW;
  }
  // the general kernel (controls / selects on register bits, masked 2x2) holds a smaller tile (opt_general_r)
  const int rmax = stays_simple(g, lo, true) ? h->opt_multi_r : std::min(h->opt_multi_r, h->opt_general_r);
  if ((int)g.targets.size() < rmax) return PL_REG_NEW;
  // registers are full: borrow one of lane bits 3..5 (simple passes, every register bit above the lanes)
  if (g.lane_mode && t < 28 && stays_simple(g, lo, false) && (int)g.dyn_targets.size() < h->opt_dyn_lanes &&
      high_lanes_used(g) < 3) {
    for (int q : g.targets) if (q < 6) return PL_REJECT;
    return PL_DYN_NEW;
  }
  return PL_REJECT;
}

static bool group_fits(const qsv_handle* h, const PendingGroup& g, const LocalOp& lo) {
  const Place pl = place_target(h, g, lo);
  if (pl == PL_REJECT) return false;
  const bool as_reg = pl == PL_REG_NEW || pl == PL_REG_OLD;
  if (!stays_simple(g, lo, as_reg)) {
    // borrowed lane bits exist in the table-op (simple) kernels only; the general kernel holds R <= opt_general_r
    if (!g.dyn_targets.empty() || pl == PL_DYN_NEW) return false;
    if ((int)g.targets.size() + (pl == PL_REG_NEW ? 1 : 0) > std::min(h->opt_multi_r, h->opt_general_r)) return false;
  }
  if (g.table_cplx + table_cplx_of(lo) > QSV_MULTI_TABLE_CPLX) return false;  // 40 KiB of LDS tables
  // keep the pass HBM bound: a general (masked / non-table) pass is cut when its arithmetic outgrows
  // what one read + write of the shard hides; table-only passes of a fused circuit are planned in
  // Python (lane quota) and measured to stay below it
  if (h->opt_pass_budget > 0 && !g.ops.empty() && !stays_simple(g, lo, as_reg) &&
      g.cost + op_cost(lo, pl == PL_LANE_NEW || pl == PL_LANE_OLD, g.targets) > (double)h->opt_pass_budget) return false;
  // the cap is where a pass's arithmetic about equals its memory time; the last few ops of a program ride along all the
  // same: a pass of two ops costs a whole read + write of the shard (the unfused reference stream ended with one)
  const int cap = std::min(h->opt_pass_max_ops, 64 * QSV_COMBO_WORDS - 16);
  return (int)g.ops.size() < cap || (h->exec_ops_left <= cap / 8 && (int)g.ops.size() < 64 * QSV_COMBO_WORDS);
}
static void group_add(const qsv_handle* h, const Shard& s, PendingGroup& g, LocalOp&& lo) {
  if (!g.opened) {
    // lane bits are the lane id only if nothing is inserted below bit 6: no known-zero bit there
    // (zero tracking) and a shard wide enough for 64-lane rows
    g.opened = true;
    g.lane_mode = h->opt_lane_targets && h->L >= 12 && s.zmask == 0;   // full wavefronts, lane id = address bits 0..5
  }
  const Place pl = place_target(h, g, lo);
  g.simple = stays_simple(g, lo, pl == PL_REG_NEW || pl == PL_REG_OLD);
  if (pl == PL_LANE_NEW) g.lane_targets.push_back(lo.target);
  else if (pl == PL_DYN_NEW) g.dyn_targets.push_back(lo.target);
  else if (pl == PL_REG_NEW) g.targets.push_back(lo.target);
  if (lo.type <= 1) for (int q : lo.list) if (!has_bit(g.selects, q)) g.selects.push_back(q);
  g.cost += op_cost(lo, pl == PL_LANE_NEW || pl == PL_LANE_OLD, g.targets);
  g.table_cplx += table_cplx_of(lo);
  g.ops.push_back(std::move(lo));
}

template <int R>
static void launch_multi(const qsv_handle* h, const Shard& s, bool init, int mode, uint64_t nthreads, const BitIns& ins,
                         const RegPos& rp, const LanePos& lp, const MultiOp* dops, const MultiSlot* dslots, int nrounds,
                         const cplx* dtab, int ntab, uint64_t nonmask, double initval, unsigned zreg, double* tsums, uint64_t xmask) {
  const dim3 g((unsigned)((nthreads + QSV_TPB - 1) / QSV_TPB));
  const size_t shm = (size_t)std::max(ntab, 1) * sizeof(cplx);
#define QSV_LM(I, S, N) hipLaunchKernelGGL((k_multi<R, I, S, N>), g, dim3(QSV_TPB), shm, s.stream, s.amp, nthreads, ins, rp, lp, dops, dslots, nrounds, dtab, ntab, nonmask, initval, zreg, tsums, xmask)
  // non-temporal form for shards beyond the caches (option multi_nt: -1 by shard size, 0 never, 1 always);
  // instantiated for the tile widths large states use
  bool nt = false;
  if constexpr (R >= 3) nt = h->opt_multi_nt > 0 || (h->opt_multi_nt < 0 && h->L >= 26);
  if (mode == 0) {                                   // the general kernel exists up to QSV_GENERAL_MAXR (checked by the caller)
    if constexpr (R <= QSV_GENERAL_MAXR) {
      if constexpr (R >= 3) {
        if (nt) { if (init) QSV_LM(true, 0, true); else QSV_LM(false, 0, true); return; }
      }
      if (init) QSV_LM(true, 0, false); else QSV_LM(false, 0, false);
    }
    return;
  }
  if constexpr (R >= 3) {
    if (nt) {
      if (init) { if (mode == 2) QSV_LM(true, 2, true); else QSV_LM(true, 1, true); }
      else      { if (mode == 2) QSV_LM(false, 2, true); else QSV_LM(false, 1, true); }
      return;
    }
  }
  if (init) { if (mode == 2) QSV_LM(true, 2, false); else QSV_LM(true, 1, false); }
  else      { if (mode == 2) QSV_LM(false, 2, false); else QSV_LM(false, 1, false); }
#undef QSV_LM
}

// ------------------------------------------------------------------------------------------
// init + diagonal factors only: k_init_prod (write-only generator, no k_multi machinery)
// ------------------------------------------------------------------------------------------
static bool group_is_init_product(const qsv_handle* h, const PendingGroup& g) {
  if (!h->opt_init_prod || !g.init || g.ops.empty() || h->L < 14 || g.xframe) return false;
  for (const LocalOp& lo : g.ops) if (lo.type != 1) return false;
  return true;
}

#define QSV_GEN_NT_MIN_L 30
#define QSV_DEFER_MIN_L 30        // option defer_state = -1: local qubits from which the final generator leaves sums only (DESIGN §5e)
// option sums_factored = -1: tile-index bits the factored sums launch must remove to be taken.  Measured
// (profiles/r09_factored_sums.log): 4 bits of 22 at 34 qubits 1.65 -> 0.174 ms, 3 of 15 at 28 qubits 0.390 -> 0.379 ms, 2 of 7 at
// 20 qubits 0.0342 -> 0.0375 ms (the second launch costs more than a quarter of 128 tiles saves)
#define QSV_FACTORED_MIN_BITS 3
template <int R, bool NT, int ZR, int FORM>
static int launch_init_prod_k(const qsv_handle* h, const Shard& s, uint64_t ntiles, const BitIns& ins, const RegPos& rp,
                              const LanePos& lp, const ProdFactor* f, const ProdCounts& cnt, const ProdGroup& grp,
                              const cplx* tab, int ntab, uint64_t nonmask, double initval, uint64_t zskip,
                              unsigned zreg, const uint64_t* list, uint64_t nlist, const double* resid, uint64_t* out) {
  // persistent grid: every workgroup the chip holds at once at this kernel's occupancy (option init_prod_grid: fewer)
  const size_t lds = (size_t)ntab * sizeof(cplx) + (size_t)cnt.nfac * (16 + 64 * sizeof(uint16_t)) +
                     (grp.nb ? ((size_t)cnt.nfac << grp.nb) * sizeof(uint16_t) : 0);
  // (asked once per LDS size: the answer depends on nothing else, and the query is host time on every step)
  static thread_local std::unordered_map<size_t, int> occupancy;
  auto it = occupancy.find(lds);
  if (it == occupancy.end()) {
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&k_init_prod<R, NT, ZR, FORM>),
                                                        QSV_TPB, std::max<size_t>(lds, 16)));
    it = occupancy.emplace(lds, per_cu).first;
  }
  const int per_cu = it->second;
  if (per_cu < 1) return fail(QSV_E_UNSUPPORTED, "k_init_prod does not fit a CU (%zu B of LDS)", lds);
  uint64_t grid = (uint64_t)per_cu * (uint64_t)s.n_cu;
  if (h->opt_init_prod_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_init_prod_grid);
  if (FORM == QSV_GEN_LISTED || FORM == QSV_GEN_LOCATE) grid = std::max<uint64_t>(1, std::min(grid, nlist));   // one workgroup per entry, grid-stride beyond
  else grid = std::min(grid, ntiles >> grp.nb);   // one workgroup per group at most
  hipLaunchKernelGGL((k_init_prod<R, NT, ZR, FORM>), dim3((unsigned)grid), dim3(QSV_TPB), std::max<size_t>(lds, 16), s.stream,
                     s.amp, ntiles, ins, rp, lp, f, cnt, grp, tab, ntab, nonmask, initval, zskip, zreg, list, nlist, resid, out);
  return QSV_OK;
}
template <int R>
static int launch_init_prod(const qsv_handle* h, const Shard& s, int form, uint64_t ntiles, const BitIns& ins, const RegPos& rp, const LanePos& lp,
                            const ProdFactor* f, const ProdCounts& cnt, const ProdGroup& grp, const cplx* tab, int ntab,
                            uint64_t nonmask, double initval, uint64_t zskip, unsigned zreg,
                            const uint64_t* list = nullptr, uint64_t nlist = 0, const double* resid = nullptr, uint64_t* out = nullptr) {
  // non-temporal stores pay on big shards (34 qubits: 6.86 -> 7.11 TB/s; 28 qubits: -1 %; profiles/r02_nt_variants.log)
  const bool nt = h->opt_nt > 0 || (h->opt_init_prod_nt < 0 && h->L >= QSV_GEN_NT_MIN_L) || h->opt_init_prod_nt > 0;
  // the top register bit as the only implied-zero register bit (the layout at 34 qubits) is a compile-time case; any
  // other zreg, none included, is read at run time (a compile-time zreg = 0 took 127 registers at R = 4 against 109
  // and wrote the full state 8 % slower)
  constexpr int ZTOP = 1 << (R - 1);
#define QSV_LIP(NT, ZR, FORM) return launch_init_prod_k<R, NT, ZR, FORM>(h, s, ntiles, ins, rp, lp, f, cnt, grp, tab, ntab, nonmask, initval, zskip, zreg, list, nlist, resid, out)
  // the listed form stores a few tiles that k_locate_tile reads next: one instantiation per (R, ZR), whatever the
  // non-temporal choice of the writing form
  if (form == QSV_GEN_LISTED) { if (zreg == ZTOP) QSV_LIP(false, ZTOP, QSV_GEN_LISTED); QSV_LIP(false, -1, QSV_GEN_LISTED); }
  // the locating form stores nothing: one instantiation per (R, ZR) likewise
  if (form == QSV_GEN_LOCATE) { if (zreg == ZTOP) QSV_LIP(false, ZTOP, QSV_GEN_LOCATE); QSV_LIP(false, -1, QSV_GEN_LOCATE); }
  if (nt) { if (zreg == ZTOP) QSV_LIP(true, ZTOP, QSV_GEN_WRITE); QSV_LIP(true, -1, QSV_GEN_WRITE); }
  if (zreg == ZTOP) QSV_LIP(false, ZTOP, QSV_GEN_WRITE);
  QSV_LIP(false, -1, QSV_GEN_WRITE);
#undef QSV_LIP
}

// The tile sums of the state the generator produces (k_prod_sums): the one producer of a generator pass's sums, whether
// the amplitudes are stored by the launch before it or deferred.  Persistent grid like the generator's.
template <int R, bool REGSUM>
static int launch_prod_sums_k(const qsv_handle* h, const Shard& s, uint64_t ntiles, const BitIns& ins, const RegPos& rp,
                              const LanePos& lp, const ProdFactor* f, const ProdCounts& cnt, const ProdGroup& grp,
                              const ProdWalk& walk, const cplx* tab, int ntab, uint64_t nonmask, double initval, double* tsums) {
  const size_t lds = (size_t)((ntab + 1) & ~1) * sizeof(double) + (size_t)cnt.nfac * (16 + 64 * sizeof(uint16_t)) +
                     (grp.nb ? ((size_t)cnt.nfac << grp.nb) * sizeof(uint16_t) : 0);
  static thread_local std::unordered_map<size_t, int> occupancy;
  auto it = occupancy.find(lds);
  if (it == occupancy.end()) {
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&k_prod_sums<R, REGSUM>),
                                                        QSV_TPB, std::max<size_t>(lds, 16)));
    it = occupancy.emplace(lds, per_cu).first;
  }
  const int per_cu = it->second;
  if (per_cu < 1) return fail(QSV_E_UNSUPPORTED, "k_prod_sums does not fit a CU (%zu B of LDS)", lds);
  uint64_t grid = (uint64_t)per_cu * (uint64_t)s.n_cu;
  if (h->opt_init_prod_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_init_prod_grid);
  grid = std::max<uint64_t>(1, std::min(grid, walk.nsum >> grp.nb));   // one workgroup per group at most
  hipLaunchKernelGGL((k_prod_sums<R, REGSUM>), dim3((unsigned)grid), dim3(QSV_TPB), std::max<size_t>(lds, 16), s.stream,
                     ntiles, ins, rp, lp, f, cnt, grp, walk, tab, ntab, nonmask, initval, tsums);
  return QSV_OK;
}
template <int R>
static int launch_prod_sums(const qsv_handle* h, const Shard& s, uint64_t ntiles, const BitIns& ins, const RegPos& rp, const LanePos& lp,
                            const ProdFactor* f, const ProdCounts& cnt, const ProdGroup& grp, const ProdWalk& walk,
                            const cplx* tab, int ntab, uint64_t nonmask, double initval, double* tsums) {
  // only single-register factors on the register bits: the register sum is a product of R two-term sums
  if (cnt.nmulti == 0 && cnt.nmixed == 0)
    return launch_prod_sums_k<R, false>(h, s, ntiles, ins, rp, lp, f, cnt, grp, walk, tab, ntab, nonmask, initval, tsums);
  return launch_prod_sums_k<R, true>(h, s, ntiles, ins, rp, lp, f, cnt, grp, walk, tab, ntab, nonmask, initval, tsums);
}
// every tile's sum from the inner sums of a factored launch: one thread per tile, each workgroup a few runs of 256 tiles
static int launch_tile_sums_expand(const qsv_handle* h, const Shard& s, uint64_t ntiles, uint64_t dmask, uint64_t tnon,
                                   const ExpandFactor* f, int nuni, int nw, const cplx* tab, const double* inner, double* tsums) {
  const size_t lds = (size_t)nw * sizeof(double) + (size_t)nuni * sizeof(ExpandFactor);
  uint64_t grid = std::min<uint64_t>((ntiles + QSV_TPB - 1) / QSV_TPB, (uint64_t)s.n_cu * 8);
  if (h->opt_init_prod_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)h->opt_init_prod_grid);
  hipLaunchKernelGGL(k_tile_sums_expand, dim3((unsigned)std::max<uint64_t>(grid, 1)), dim3(QSV_TPB), std::max<size_t>(lds, 16), s.stream,
                     ntiles, dmask, tnon, f, nuni, nw, tab, inner, tsums);
  return QSV_OK;
}

// the generator from a shard's recipe: the writing form (realize), the listed form or the locating form (qsv_sample)
static int launch_recipe(const qsv_handle* h, const Shard& s, int form, const uint64_t* list, uint64_t nlist,
                         const double* resid = nullptr, uint64_t* out = nullptr) {
  const GenRecipe& rc = s.recipe;
#define QSV_LR(RR) return launch_init_prod<RR>(h, s, form, rc.ntiles, rc.ins, rc.rp, rc.lp, rc.dfac, rc.cnt, rc.grp, rc.dtab, rc.ntab, rc.nonmask, rc.initval, rc.zskip, rc.zreg, list, nlist, resid, out)
  switch (rc.R) {
    case 3: QSV_LR(3);
    case 4: QSV_LR(4);
    case 5: QSV_LR(5);
    case 6: QSV_LR(6);
    default: return fail(QSV_E_HIP, "deferred state without a recipe");
  }
#undef QSV_LR
}

// A deferred shard gets its amplitudes: the writing generator on the recipe the sums launch ran with, the
// instantiation the engine's options choose for a writing launch.  The state does not change, so -- as in materialize --
// the cached sums stay valid.  Booked under init_prod with the 16 B of every amplitude stored; afterwards zmask is what
// a writing final pass leaves (it was set when the state was deferred).
static int realize(qsv_handle* h, Shard& s) {
  if (!s.deferred) return QSV_OK;
  const uint64_t n = amps_local(h);
  CHK(shard_set(s));
  const bool sv = s.sums_valid, tv = s.tile_valid, hv = s.h_tsums_valid;
  const int dv = s.d_super_valid;
  int lr = QSV_OK;
  const int r = launch(h, s, QSV_K_INIT_PROD, 16.0 * (double)(n >> __builtin_popcountll(s.recipe.zskip)), [&] {
    lr = launch_recipe(h, s, QSV_GEN_WRITE, nullptr, 0);
  });
  CHK(lr);
  CHK(r);
  s.deferred = false;
  s.sums_valid = sv;
  s.tile_valid = tv;
  s.h_tsums_valid = hv;
  s.d_super_valid = dv;
  h->n_realize += 1;
  return QSV_OK;
}

template <int R>
static int flush_init_product_r(qsv_handle* h, Shard& s, PendingGroup& g, bool final_pass) {
  const uint64_t n = amps_local(h);
  CHK(shard_set(s));
  // the planner puts qubits that few factors touch on the register bits
  RegPos rp;
  memset(&rp, 0, sizeof rp);
  std::vector<int> inspos;
  // Where the register bits sit is a pure access-pattern choice, measured per shard size
  // (profiles/r01s2_gen_tile_by_size.log, r01s2_gen_tile34.log): shards of >= 2^33 amplitudes
  // stream best with the registers on the TOP bits (each of a lane's stores belongs to its own
  // long linear run: 6.9-7.1 TB/s against 6.6-6.7), smaller ones with registers on bits 6..10
  // and lane bit 5 on bit 11 (6.3-6.5 TB/s against 5.0-5.8).  planner.choose_layout mirrors this.
  int b0 = 6;
  if (h->opt_init_prod_bit0 < 0 || (h->opt_init_prod_bit0 == 0 && h->L >= 33)) b0 = h->L - R;
  else if (h->opt_init_prod_bit0 > 6) b0 = std::min(h->opt_init_prod_bit0, h->L - R);
  for (int c = 0; c < R; ++c) { rp.pos[c] = b0 + c; inspos.push_back(b0 + c); }
  LanePos lp;
  if (b0 == 6) {
    lp.pos[0] = 3; lp.pos[1] = 4; lp.pos[2] = 6 + R;
    for (int k = 0; k < 3; ++k) inspos.push_back(lp.pos[k]);
  } else if (h->opt_lane_map == 1 && b0 > 11 && h->L >= 14) {
    lp.pos[0] = 3; lp.pos[1] = 4; lp.pos[2] = 11;            // lane bit 5 on bit 11 wherever the tile is (flush_group, lane map)
    for (int k = 0; k < 3; ++k) inspos.push_back(lp.pos[k]);
  } else {
    lp.pos[0] = lp.pos[1] = lp.pos[2] = -1;
  }
  const BitIns ins = make_ins(inspos);
  // the class of every address bit for this tile geometry (k_init_prod): register bit, lane bit (varies within a
  // wave), or wave-uniform -- then it is bit t of the wave index tile * 4 + wave, whose bits the tile map places
  // (tile_base_thr / tile_base_blk) like those of the value (wave index << wsh)
  uint32_t lanemask = 0;
  for (uint32_t l = 0; l < 64; ++l) lanemask |= tile_base_thr(l, ins, lp);
  const int wsh = lp.pos[0] < 0 ? 6 : 3;
  int wbit_of[64];
  for (int q = 0; q < 64; ++q) wbit_of[q] = -1;
  for (int t = 0; t < QSV_PROD_NOBIT && t + wsh < 64; ++t) {
    const uint64_t a = ins_bits(1ull << (t + wsh), ins);
    if (a && a < (1ull << h->L)) wbit_of[__builtin_ctzll(a)] = t;
  }
  if ((n >> R) / 64 > (1ull << QSV_PROD_NOBIT)) return fail(QSV_E_UNSUPPORTED, "init product: shard too large for 31-bit wave indices");
  const uint64_t ntiles = (n >> R) / QSV_TPB;
  // Tile groups (k_init_prod): block bits of the tile index whose 2^B tiles a workgroup takes at once.  Option
  // init_prod_group: -1 up to 3 of them, 0 none, 1..4 that many where they exist; never more than the tile index has.
  // Never a nonmask bit: those are the provably-zero qubits, the same with implied zeros on or off, so the choice --
  // and with it the product order of every amplitude -- is too.  First the bits the fewest factors touch, then bits
  // that share no factor with a register bit (such a factor costs a multiply per amplitude), then the lowest.  The
  // choice depends on the tile geometry and the factor list only.
  // classify(): the group bits and the factor classes -- outer, group, register (single / multi), mixed (k_init_prod) --
  // of the factors `which` (indices into g.ops, list order kept), group bits taken among the address bits `cand_bits`.
  // Every op's table keeps its place in the one table array, whichever factors a launch lists.
  int ntb = 0;
  while ((1ull << ntb) < ntiles) ++ntb;
  std::vector<double> tables;
  std::vector<int> tab_of(g.ops.size());
  for (size_t i = 0; i < g.ops.size(); ++i) {
    tab_of[i] = (int)(tables.size() / 2);
    tables.insert(tables.end(), g.ops[i].table.begin(), g.ops[i].table.end());
  }
  if (tables.size() / 2 > 2560) return fail(QSV_E_UNSUPPORTED, "init product tables exceed LDS");
  if (g.ops.size() > QSV_PROD_MAXF) return fail(QSV_E_UNSUPPORTED, "init product of %zu factors (limit %d)", g.ops.size(), QSV_PROD_MAXF);
  struct Classified { ProdGroup grp; ProdCounts cnt; std::vector<ProdFactor> uni; };   // uni: the factor list in kernel order
  auto classify = [&](const std::vector<int>& which, uint64_t cand_bits, Classified& out) -> int {
    ProdGroup& grp = out.grp;
    memset(&grp, 0, sizeof grp);
    int gbit_of[64];                                  // address bit -> group bit index, or -1
    for (int q = 0; q < 64; ++q) gbit_of[q] = -1;
    {
      const int want = std::min(h->opt_init_prod_group < 0 ? 3 : h->opt_init_prod_group, std::min(ntb, QSV_PROD_MAXG));
      int nfq[64] = {0};
      bool regq[64] = {false};
      for (int i : which) {
        const LocalOp& lo = g.ops[i];
        bool reg = false;
        for (int q : lo.list) reg |= q >= b0 && q < b0 + R;
        for (int q : lo.list) { ++nfq[q]; regq[q] |= reg; }
      }
      std::vector<int> cand;                          // block bits: wave-index bits 2.. (the tile index)
      for (int q = 0; q < h->L; ++q)
        if (wbit_of[q] >= 2 && !((g.nonmask >> q) & 1ull) && ((cand_bits >> q) & 1ull)) cand.push_back(q);
      std::sort(cand.begin(), cand.end(), [&](int a, int b) {
        return std::make_tuple(nfq[a], regq[a], a) < std::make_tuple(nfq[b], regq[b], b);
      });
      if ((int)cand.size() > want) cand.resize(std::max(want, 0));
      std::sort(cand.begin(), cand.end());            // the tile map keeps the order of the bits
      grp.nb = (int)cand.size();
      for (int i = 0; i < grp.nb; ++i) { grp.tpos[i] = wbit_of[cand[i]] - 2; gbit_of[cand[i]] = i; }
    }
    std::vector<ProdFactor> outer, grpf, multi, mixed, single[R];
    int nlmax = 0;
    for (int i : which) {
      const LocalOp& lo = g.ops[i];
      ProdFactor pf;
      memset(&pf, 0, sizeof pf);
      pf.nlist = (int)lo.list.size();
      pf.tab = tab_of[i];
      nlmax = std::max(nlmax, pf.nlist);
      int nreg = 0, creg = 0, ngb = 0;
      for (int e = 0; e < QSV_MULTI_MAXLIST; ++e) pf.wbit[e >> 2] |= (uint32_t)QSV_PROD_NOBIT << (8 * (e & 3));
      for (int e = 0; e < pf.nlist; ++e) {
        const int q = lo.list[e];
        pf.pos[e] = -1;
        if (q >= b0 && q < b0 + R) { pf.regw[q - b0] = 1 << e; ++nreg; creg = q - b0; }
        else if (q < 32 && ((lanemask >> q) & 1u)) pf.pos[e] = q;
        else {
          if (wbit_of[q] < 0) return fail(QSV_E_UNSUPPORTED, "init product: address bit %d has no class", q);
          // a group bit is 0 in the wave index of a group's first tile, which is where the kernel gathers
          pf.wbit[e >> 2] = (pf.wbit[e >> 2] & ~(0xffu << (8 * (e & 3)))) | ((uint32_t)wbit_of[q] << (8 * (e & 3)));
          if (gbit_of[q] >= 0) { pf.grpw[gbit_of[q]] = 1 << e; ++ngb; }
        }
      }
      if (nreg == 0) (ngb ? grpf : outer).push_back(pf);
      else if (ngb) mixed.push_back(pf);
      else (nreg == 1 ? single[creg] : multi).push_back(pf);
    }
    ProdCounts& cnt = out.cnt;
    memset(&cnt, 0, sizeof cnt);
    std::vector<ProdFactor>& uni = out.uni;
    uni.clear();
    cnt.nouter = (int)outer.size();
    uni.insert(uni.end(), outer.begin(), outer.end());
    cnt.ngrp = (int)grpf.size();
    uni.insert(uni.end(), grpf.begin(), grpf.end());
    for (int c = 0; c < R; ++c) { cnt.nsingle[c] = (int)single[c].size(); uni.insert(uni.end(), single[c].begin(), single[c].end()); }
    cnt.nmulti = (int)multi.size();
    uni.insert(uni.end(), multi.begin(), multi.end());
    cnt.nmixed = (int)mixed.size();
    uni.insert(uni.end(), mixed.begin(), mixed.end());
    cnt.nfac = (int)uni.size();
    cnt.nlmax = nlmax;
    return QSV_OK;
  };
  std::vector<int> every(g.ops.size());
  for (size_t i = 0; i < every.size(); ++i) every[i] = (int)i;
  Classified all;                                   // what the writing and listed generator run with, and the unfactored sums
  CHK(classify(every, ~0ull, all));
  const ProdGroup& grp = all.grp;
  const ProdCounts& cnt = all.cnt;
  const std::vector<ProdFactor>& uni = all.uni;
  const int ntab = (int)(tables.size() / 2);
  const uint64_t nthreads = n >> R;
  double* tsums = nullptr;
  if (final_pass && h->opt_fused_sums) {
    const uint64_t nb = nthreads / QSV_TPB;
    if (s.tsums_cap < nb) {
      if (s.d_tsums) HIPCHK(hipFree(s.d_tsums));
      HIPCHK(hipMalloc(&s.d_tsums, nb * sizeof(double)));
      s.tsums_cap = nb;
    }
    tsums = s.d_tsums;
    s.tile_R = R;
    s.tile_rp = rp;
    s.tile_lp = lp;
    s.tile_ins = ins;
    s.tile_nblocks = nb;
    s.tile_xor = 0;
  }
  // Factored sums (option sums_factored, DESIGN §5e), the sums launch only.  A factor whose every bit is a block bit is
  // tile-uniform: one weight for all 256 threads of a tile, so it leaves the tile's sum.  The other factors (inner)
  // read the tile index only through D, the block bits they touch: k_prod_sums runs over the 2^|D| tiles with every
  // other tile-index bit held at 0, with group bits and classes of its own taken over the inner factors and D, and
  // k_tile_sums_expand forms every tile's sum from those.  A nonmask bit is never in D: it is 0 wherever the sum is
  // not.  Taken when it removes at least QSV_FACTORED_MIN_BITS tile-index bits (sums_factored = 1: one); a function
  // of the tile geometry and the factor list only.
  Classified in;
  std::vector<ExpandFactor> tuf;
  ProdWalk walk;
  memset(&walk, 0, sizeof walk);
  walk.nsum = ntiles;
  for (int i = 0; i < grp.nb; ++i) walk.cpos[i] = grp.tpos[i];
  uint64_t dmask = 0, tnon = 0;
  int nwexp = 0;
  bool factored = false;
  if (tsums) {
    std::vector<int> inner;
    for (size_t i = 0; i < g.ops.size(); ++i) {
      bool uniform = true;
      for (int q : g.ops[i].list) uniform &= wbit_of[q] >= 2;
      if (!uniform) { inner.push_back((int)i); continue; }
      ExpandFactor ef;
      memset(&ef, 0, sizeof ef);
      ef.nlist = (int)g.ops[i].list.size();
      ef.tab = tab_of[i];
      ef.lds = nwexp;
      for (int e = 0; e < ef.nlist; ++e) ef.tbit[e] = (unsigned char)(wbit_of[g.ops[i].list[e]] - 2);
      nwexp += 1 << ef.nlist;
      tuf.push_back(ef);
    }
    uint64_t dbits = 0;                             // D as address bits
    for (int i : inner)
      for (int q : g.ops[i].list)
        if (wbit_of[q] >= 2 && !((g.nonmask >> q) & 1ull)) { dmask |= 1ull << (wbit_of[q] - 2); dbits |= 1ull << q; }
    for (int q = 0; q < h->L; ++q)
      if (wbit_of[q] >= 2 && ((g.nonmask >> q) & 1ull)) tnon |= 1ull << (wbit_of[q] - 2);
    const int nd = __builtin_popcountll(dmask);
    const int need = h->opt_sums_factored > 0 ? 1 : QSV_FACTORED_MIN_BITS;
    factored = h->opt_sums_factored != 0 && ntb - nd >= need;
    s.sums_info[0] = factored ? 1 : 0;
    s.sums_info[1] = nd;
    s.sums_info[2] = (int)inner.size();
    s.sums_info[3] = (int)tuf.size();
    if (factored) {
      CHK(classify(inner, dbits, in));
      walk.nsum = 1ull << nd;
      walk.tfix = (ntiles - 1ull) & ~dmask;
      for (int i = 0; i < in.grp.nb; ++i) walk.cpos[i] = __builtin_popcountll(dmask & ((1ull << in.grp.tpos[i]) - 1ull));
      if (s.inner_cap < walk.nsum) {
        if (s.d_inner) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(s.d_inner)); }
        s.d_inner = nullptr;
        s.inner_cap = 0;
        HIPCHK(hipMalloc(&s.d_inner, walk.nsum * sizeof(double)));
        s.inner_cap = walk.nsum;
      }
    }
  }
  // implied zeros: as the program's last pass the generator stores only the amplitudes outside the provably-zero
  // region (planner.choose_layout puts such a qubit on the top bit: half the shard); otherwise every amplitude is
  // written, zeros included, so that the passes after it need not know
  const uint64_t nonmask = g.nonmask;
  const uint64_t zskip = final_pass && h->opt_implied_zeros ? nonmask : 0ull;
  unsigned zreg = 0;
  for (int c = 0; c < R; ++c) if ((zskip >> rp.pos[c]) & 1ull) zreg |= 1u << c;
  s.zmask = zskip;
  // Deferred state (option defer_state): as the program's last pass, leaving tile sums, the generator stores nothing:
  // k_prod_sums alone runs.  Not deferred, the writing generator runs and then k_prod_sums, one bracket, one launch booked.
  // The step's result needs the sums and the tiles its shots fall into (qsv_sample stores those); whoever reads the
  // state later calls realize().  The descriptors and tables then go to the shard's recipe buffer, not to the arena.
  const bool defer = tsums != nullptr && (h->opt_defer_state > 0 || (h->opt_defer_state < 0 && h->L >= QSV_DEFER_MIN_L));
  const size_t fbytes = (uni.size() * sizeof(ProdFactor) + 255) & ~size_t(255);
  const size_t tbytes = tables.size() * sizeof(double);
  void* dfac = nullptr;
  void* dtab = nullptr;
  void* dfin = nullptr;                             // a factored sums launch: the inner factors in their own order, the tile-uniform ones
  void* dtuf = nullptr;
  if (defer) {
    // one upload: [factor descriptors | tables | inner factors | tile-uniform factors], each part at a 256-byte offset
    // of one pinned block, sent with one copy into the recipe buffer (the last two parts serve this pass's sums launch
    // only; four copies were four 5 us transfers in a row ahead of k_prod_sums)
    const size_t ibytes = factored ? in.uni.size() * sizeof(ProdFactor) : 0;
    const size_t ubytes = factored ? tuf.size() * sizeof(ExpandFactor) : 0;
    const size_t otab = fbytes, ofin = (otab + tbytes + 255) & ~size_t(255), otuf = (ofin + ibytes + 255) & ~size_t(255);
    const size_t need = otuf + ubytes;
    GenRecipe& rc = s.recipe;
    if (rc.cap < need) {
      if (rc.d_buf) { HIPCHK(hipStreamSynchronize(s.stream)); HIPCHK(hipFree(rc.d_buf)); }
      rc.d_buf = nullptr;
      rc.cap = 0;
      const size_t cap = std::max<size_t>(need, 64u << 10);
      HIPCHK(hipMalloc(&rc.d_buf, cap));
      rc.cap = cap;
    }
    void* hb = nullptr;
    CHK(arena_slot(s, need, &hb));
    char* hp = reinterpret_cast<char*>(hb);
    memcpy(hp, uni.data(), uni.size() * sizeof(ProdFactor));
    memcpy(hp + otab, tables.data(), tbytes);
    if (ibytes) memcpy(hp + ofin, in.uni.data(), ibytes);
    if (ubytes) memcpy(hp + otuf, tuf.data(), ubytes);
    HIPCHK(hipMemcpyAsync(rc.d_buf, hp, need, hipMemcpyHostToDevice, s.stream));
    dfac = rc.d_buf;
    dtab = rc.d_buf + otab;
    if (ibytes) dfin = rc.d_buf + ofin;
    if (ubytes) dtuf = rc.d_buf + otuf;
    rc.R = R; rc.ntiles = ntiles; rc.ins = ins; rc.rp = rp; rc.lp = lp; rc.cnt = cnt; rc.grp = grp; rc.ntab = ntab;
    rc.nonmask = nonmask; rc.zskip = zskip; rc.initval = g.initval; rc.zreg = zreg;
    rc.dfac = reinterpret_cast<const ProdFactor*>(dfac);
    rc.dtab = reinterpret_cast<const cplx*>(dtab);
  } else {
    CHK(arena_put(s, uni.data(), uni.size() * sizeof(ProdFactor), &dfac));
    CHK(arena_put(s, tables.data(), tbytes, &dtab));
    if (factored) {
      if (!in.uni.empty()) CHK(arena_put(s, in.uni.data(), in.uni.size() * sizeof(ProdFactor), &dfin));
      if (!tuf.empty()) CHK(arena_put(s, tuf.data(), tuf.size() * sizeof(ExpandFactor), &dtuf));
    }
  }
  h->stats.fused_gates += g.ops.size();
  const double initval = g.initval;
  int lr = QSV_OK;
  const int r = launch(h, s, QSV_K_INIT_PROD, defer ? 0.0 : 16.0 * (double)(n >> __builtin_popcountll(zskip)), [&] {
    const ProdFactor* df = reinterpret_cast<const ProdFactor*>(dfac);
    const cplx* dt = reinterpret_cast<const cplx*>(dtab);
    if (!defer) lr = launch_init_prod<R>(h, s, QSV_GEN_WRITE, ntiles, ins, rp, lp, df, cnt, grp, dt, ntab, nonmask, initval, zskip, zreg);
    if (lr != QSV_OK || !tsums) return;
    if (!factored) { lr = launch_prod_sums<R>(h, s, ntiles, ins, rp, lp, df, cnt, grp, walk, dt, ntab, nonmask, initval, tsums); return; }
    lr = launch_prod_sums<R>(h, s, ntiles, ins, rp, lp, reinterpret_cast<const ProdFactor*>(dfin), in.cnt, in.grp, walk, dt, ntab,
                             nonmask, initval, s.d_inner);
    if (lr == QSV_OK)
      lr = launch_tile_sums_expand(h, s, ntiles, dmask, tnon, reinterpret_cast<const ExpandFactor*>(dtuf), (int)tuf.size(), nwexp,
                                   dt, s.d_inner, tsums);
  });
  CHK(lr);
  s.deferred = defer && r == QSV_OK;
  s.tile_fresh = tsums != nullptr;
  s.sums_from_gen = tsums != nullptr;
  g = PendingGroup();
  return r;
}

static int flush_init_product(qsv_handle* h, Shard& s, PendingGroup& g, bool final_pass) {
  const int r = h->opt_init_prod_r ? h->opt_init_prod_r
                                   : ((h->opt_init_prod_bit0 < 0 || (h->opt_init_prod_bit0 == 0 && h->L >= 33)) ? 4 : 5);
  switch (r) {
    case 3: return flush_init_product_r<3>(h, s, g, final_pass);
    case 4: return flush_init_product_r<4>(h, s, g, final_pass);
    case 6: return flush_init_product_r<6>(h, s, g, final_pass);
    default: return flush_init_product_r<5>(h, s, g, final_pass);
  }
}

static int flush_group(qsv_handle* h, Shard& s, PendingGroup& g, bool final_pass = false) {
  const uint64_t n = amps_local(h);
  CHK(shard_set(s));
  if (group_is_init_product(h, g)) return flush_init_product(h, s, g, final_pass);
  if (g.ops.empty()) {
    if (g.init) {
      s.zmask = 0;
      CHK(launch(h, s, QSV_K_INIT, 16.0 * (double)n, [&] {
        hipLaunchKernelGGL(k_init, dim3(grid_for(h, s, n, QSV_TPB * 4)), dim3(QSV_TPB), 0, s.stream, s.amp, n, g.nonmask, g.initval);
      }));
    }
    // X gates with no pass to ride in: executed as the swaps they are (each thread of k_pair moves both
    // amplitudes of its pair: safe on any bit)
    for (int b = 0; b < h->L; ++b)
      if ((g.xframe >> b) & 1ull) {
        LocalOp x;
        x.type = 2; x.is_x = true; x.target = b; x.m[2] = 1.0; x.m[4] = 1.0;
        CHK(run_single(h, s, x));
      }
    g = PendingGroup();
    return QSV_OK;
  }
  if (g.ops.size() == 1 && !g.init && !g.xframe && h->opt_single_shortcut) {
    CHK(materialize(h, s));
    const int r = run_single(h, s, g.ops[0]);
    g = PendingGroup();
    return r;
  }
  // register bits: the targets, padded with free bits >= 6 so every lane keeps >= 8 loads in flight
  std::vector<int> reg = g.targets;
  const int want = std::min(h->L, std::max((int)reg.size(), std::min(3, h->opt_multi_r)));
  for (int pass = 0; pass < 2; ++pass) {             // first bits >= 6 that are not table selects, then any
    for (int b = std::min(6, h->L - 1); (int)reg.size() < want && b < h->L; ++b)
      if (!has_bit(reg, b) && (pass == 1 || (!has_bit(g.selects, b) && !((s.zmask >> b) & 1ull)))) reg.push_back(b);
  }
  if (g.lane_targets.empty())
    for (int b = 0; (int)reg.size() < want && b < h->L; ++b)
      if (!has_bit(reg, b)) reg.push_back(b);
  // a simple (table-op) pass streams best at 32 amplitudes per lane (R = 5: 5.5 TB/s and the lane
  // map of bits 6..10, against 5.1-5.2 TB/s at R = 4): pad with bits no op of the pass looks at
  if (g.simple && h->L >= 12) {
    const int want5 = std::min(5, h->opt_multi_r);
    auto clean = [&](int b) {
      return b >= 6 && b < h->L && !has_bit(reg, b) && !has_bit(g.selects, b) && !has_bit(g.dyn_targets, b) && !((s.zmask >> b) & 1ull);
    };
    while ((int)reg.size() < want5 && !reg.empty()) {      // next to the bits already there: a compact tile streams best
      const int hi = *std::max_element(reg.begin(), reg.end()), lo = *std::min_element(reg.begin(), reg.end());
      if (clean(hi + 1)) reg.push_back(hi + 1);
      else if (clean(lo - 1)) reg.push_back(lo - 1);
      else break;
    }
    for (int b = 6; (int)reg.size() < want5 && b < h->L; ++b)
      if (clean(b)) reg.push_back(b);
  }
  // a general pass: pad to its tile size as well (fewer, larger waves: the per-op tests and descriptor
  // loads are paid once per wave), with bits nothing in the pass tests -- neither a table select nor a control
  if (!g.simple && h->L >= 12) {
    uint64_t seen = 0;
    for (const LocalOp& lo : g.ops) { for (int q : lo.list) seen |= 1ull << q; for (int q : lo.cq) seen |= 1ull << q; }
    // ... and a LIGHT one (arithmetic below half of what a sweep hides, op_cost) to the 32-amplitude tile the
    // table-op passes use: it streams 12 % faster (1.40 against 1.61 ms bare at 28 qubits), the general kernel
    // there runs two waves per SIMD and doubles each op's work per wave, which only a heavy pass notices
    // (profiles/r02_general_r_light.log: 16 masked X 1.47 against 1.63 ms, 32 dense 2x2 2.94 against 2.58)
    const int wantg = std::min(g.cost <= 50.0 ? std::max(h->opt_general_r, h->opt_general_light_r) : h->opt_general_r, h->opt_multi_r);
    for (int b = 6; (int)reg.size() < wantg && b < h->L; ++b)
      if (!has_bit(reg, b) && !((seen >> b) & 1ull) && !((s.zmask >> b) & 1ull)) reg.push_back(b);
  }
  const int R = (int)reg.size();
  RegPos rp;
  memset(&rp, 0, sizeof rp);
  for (int c = 0; c < R; ++c) rp.pos[c] = reg[c];
  // zero tracking: register bits still known |0> are not read; known-zero bits outside the tile
  // stay zero, so only the subspace where they are 0 is enumerated at all
  uint64_t regmask = 0;
  for (int q : reg) regmask |= 1ull << q;
  const uint64_t zin = s.zmask, zout = zin & ~regmask;
  unsigned zreg = 0;
  for (int c = 0; c < R; ++c) if ((zin >> reg[c]) & 1ull) zreg |= 1u << c;
  std::vector<int> inspos = reg;
  for (int b = 0; b < h->L; ++b) if ((zout >> b) & 1ull) inspos.push_back(b);
  const int nzout = __builtin_popcountll(zout);
  s.zmask = zout;
  // lane map: lane bits 3..5 keep address bits 3..5 unless lent to a target of this pass
  LanePos lp;
  lp.pos[0] = lp.pos[1] = lp.pos[2] = -1;
  if (!g.dyn_targets.empty()) {
    bool taken[3] = {false, false, false};
    for (int q : g.lane_targets) if (q >= 3) { lp.pos[q - 3] = q; taken[q - 3] = true; }
    size_t d = 0;
    for (int k = 2; k >= 0 && d < g.dyn_targets.size(); --k)
      if (!taken[k]) { lp.pos[k] = g.dyn_targets[d++]; taken[k] = true; }
    for (int k = 0; k < 3; ++k) if (!taken[k]) lp.pos[k] = 3 + k;
    for (int k = 0; k < 3; ++k) inspos.push_back(lp.pos[k]);
  } else if (h->opt_lane_map && g.lane_mode && zin == 0) {
    // No target needs a lane, but the lane map also decides which addresses one wave instruction
    // touches -- a pure access-pattern choice.  lane_map = 1 (default): the one pattern that
    // measurably beats the plain map (scripts/lane_map_sweep2.py, W = 28 / 32 / 34: 5.44 -> 5.89
    // TB/s): registers on bits 6..10, lane bit 5 on bit 11, so a wave load is two 512-byte runs
    // 32 KiB apart and the workgroup still covers one contiguous 128 KiB.  Other values: explicit
    // 5-bit fields for lane bits 3, 4, 5 (experiments).
    bool ok = true;
    for (int q : reg) if (q < 6) ok = false;
    int code = h->opt_lane_map;
    if (code == 1) {
      // whatever the register bits are, as long as bit 11 is not one of them (measured with the tile on
      // bits 6..9 + one target anywhere in 13..27: 1.53-1.74 ms plain, 1.35-1.43 ms with this map, and no
      // other position of the lane bit does it: profiles/r02_lane_map_high_target.log).  lane_map = 2: the
      // round-1 rule (only a tile on exactly bits 6..10).
      ok = ok && h->L >= 14 && !has_bit(g.lane_targets, 5);
      {
        // (the tile on exactly bits 6..10 takes the map from 2^14 amplitudes on, as in round 1; any other tile from 2^26:
        // below that the state sits in the caches and the pattern was not measured to matter)
        std::vector<int> sr = reg;
        std::sort(sr.begin(), sr.end());
        const bool classic = R == 5 && sr[0] == 6 && sr[4] == 10;
        if (!classic && h->L < h->opt_lane_map_min_l) ok = false;
      }
      // ... except in the LAST pass of a program while an X is pending on bit 5 (and none on bit 11): with the
      // plain map that pass can still apply it (flush_group below: only register and lane bits are safe
      // for the X frame); left pending it would cost a swap kernel and the cached tile sums
      if (final_pass && ((g.xframe >> 5) & 1ull) && !((g.xframe >> 11) & 1ull)) ok = false;
      code = 11 << 10;
    } else if (code == 2) {
      std::vector<int> sr = reg;
      std::sort(sr.begin(), sr.end());
      ok = ok && R == 5 && sr[0] == 6 && sr[4] == 10 && h->L >= 14 && !has_bit(g.lane_targets, 5);
      code = 11 << 10;
    } else {
      for (int q : g.lane_targets) if (q >= 3) ok = false;
    }
    int want[3];
    for (int k = 0; k < 3 && ok; ++k) {
      const int f = (code >> (5 * k)) & 31;
      want[k] = f ? f : 3 + k;
      if (want[k] >= 28 || want[k] >= h->L || has_bit(reg, want[k]) || (f && want[k] < 6)) ok = false;
      for (int j = 0; j < k && ok; ++j) if (want[j] == want[k]) ok = false;
    }
    if (ok) {
      for (int k = 0; k < 3; ++k) { lp.pos[k] = want[k]; inspos.push_back(want[k]); }
    }
  }
  auto lane_index = [&](int q) -> int {                    // lane bit that carries address bit q in this pass
    if (lp.pos[0] >= 0) for (int k = 0; k < 3; ++k) if (lp.pos[k] == q) return 3 + k;
    return q;
  };
  const BitIns ins = make_ins(inspos);
  auto reg_index = [&](int q) -> int {
    for (int c = 0; c < R; ++c) if (reg[c] == q) return c;
    return -1;
  };
  std::vector<MultiOp> mops(g.ops.size());
  std::vector<double> tables;
  for (size_t i = 0; i < g.ops.size(); ++i) {
    const LocalOp& lo = g.ops[i];
    MultiOp& mo = mops[i];
    memset(&mo, 0, sizeof mo);
    mo.type = lo.type;
    mo.bit = lo.target >= 0 ? reg_index(lo.target) : 0;
    if (lo.target >= 0 && mo.bit < 0) {                  // a lane target: wave-shuffle form
      mo.type = lo.type == 0 ? 4 : 5;
      mo.bit = lane_index(lo.target);
    }
    mo.uniform = 1;
    if (lo.type == 0 || lo.type == 1) {
      mo.nlist = (int)lo.list.size();
      mo.tab = (int)(tables.size() / 2);
      for (int e = 0; e < mo.nlist; ++e) {
        const int c = reg_index(lo.list[e]);
        if (c >= 0) { mo.pos[e] = -1; mo.regw[c] = (lo.type == 0 ? 1 : 1) << e; mo.uniform = 0; }
        else mo.pos[e] = lo.list[e];
      }
      tables.insert(tables.end(), lo.table.begin(), lo.table.end());
    } else {
      for (size_t k = 0; k < lo.cq.size(); ++k) {
        const int c = reg_index(lo.cq[k]);
        if (c >= 0) { mo.rmask |= 1u << c; if (lo.cv[k]) mo.rval |= 1u << c; }
        else { mo.tmask |= 1ull << lo.cq[k]; if (lo.cv[k]) mo.tval |= 1ull << lo.cq[k]; }
      }
      memcpy(mo.m, lo.m, sizeof mo.m);
      if (lo.type == 2 && lo.is_x) mo.nlist = 1;           // register swap instead of arithmetic
      for (int j = 0; j < (1 << R); ++j) if (((unsigned)j & mo.rmask) == mo.rval) mo.rfire |= 1ull << j;
      mo.uniform = mo.rmask == 0;
    }
    switch (mo.type) {                                     // update shape of the op in a general pass
      case 0: mo.shape = mo.uniform ? GS_TAB_T : GS_TAB_P; break;
      case 1: mo.shape = mo.uniform ? GS_DIAG_T : GS_DIAG_A; break;
      case 2: mo.shape = mo.nlist ? GS_X : GS_MAT; break;
      case 3: mo.shape = GS_PHASE; break;
      case 4: mo.shape = mo.uniform ? GS_LTAB_T : GS_LTAB_A; break;
      default: mo.shape = mo.nlist ? GS_LX : GS_LMAT; break;
    }
  }
  bool simple = true;
  for (const MultiOp& mo : mops) if ((mo.type != 0 && mo.type != 1 && mo.type != 4) || !mo.uniform) simple = false;
  // rounds of 1 + R slots: slot 0 = list of ops without a register target (diag / phase / lane-bit
  // gates), slot 1 + b = optional 2x2 gate on register bit b; a round runs its list first, then the
  // bits in order.  An op joins the current round if program order allows it or if it commutes
  // with what it would overtake (neither op's target lies in the other's support).
  // A GENERAL pass takes its ops as a flat list in program order (no rounds).
  const int NS = R + 1;
  std::vector<MultiSlot> slots;
  std::vector<MultiOp> sorted;
  sorted.reserve(mops.size() + NS);
  std::vector<int> combos;                                 // general pass: see GenCombos in qsv_kmulti.h
  if (!simple) {
    sorted = mops;
    slots.assign(NS, MultiSlot{0, 0, 0, 0});
    if (mops.size() > 64 * QSV_COMBO_WORDS) return fail(QSV_E_UNSUPPORTED, "general k_multi pass of %zu ops (limit %d)", mops.size(), 64 * QSV_COMBO_WORDS);
    // address bits that are the same for a whole workgroup: not a register bit, not supplied by the thread index, not
    // enumerated away as known-zero
    const uint64_t blockmask = (n - 1) & ~regmask & ~zout & ~(uint64_t)tile_base_thr(QSV_TPB - 1, ins, lp);
    std::vector<int> cb;
    if (h->opt_general_combos && !g.init) {
      int freq[64] = {0};
      for (const MultiOp& mo : mops)
        if (mo.type == 2 || mo.type == 3 || mo.type == 5)
          for (int b = 0; b < h->L; ++b) if (((mo.tmask & blockmask) >> b) & 1ull) ++freq[b];
      for (int b = 0; b < h->L; ++b) if (freq[b]) cb.push_back(b);
      std::sort(cb.begin(), cb.end(), [&](int x, int y) { return freq[x] != freq[y] ? freq[x] > freq[y] : x < y; });
      if ((int)cb.size() > QSV_COMBO_MAXBITS) cb.resize(QSV_COMBO_MAXBITS);
    }
    const int nb = (int)cb.size();
    combos.assign(QSV_COMBO_HDR + ((size_t)(2 * QSV_COMBO_WORDS) << nb), 0);
    combos[0] = nb;
    uint64_t chosen = 0;
    for (int e = 0; e < nb; ++e) { combos[1 + e] = cb[e]; chosen |= 1ull << cb[e]; }
    for (int ci = 0; ci < (1 << nb); ++ci) {
      uint64_t val = 0;
      for (int e = 0; e < nb; ++e) if ((ci >> e) & 1) val |= 1ull << cb[e];
      uint64_t words[QSV_COMBO_WORDS] = {0};
      for (size_t i = 0; i < mops.size(); ++i) {
        const MultiOp& mo = mops[i];
        const bool masked = mo.type == 2 || mo.type == 3 || mo.type == 5;
        if (masked && ((val ^ mo.tval) & mo.tmask & chosen)) continue;           // cannot fire in these workgroups
        words[i >> 6] |= 1ull << (i & 63);
      }
      memcpy(&combos[QSV_COMBO_HDR + (size_t)ci * 2 * QSV_COMBO_WORDS], words, sizeof words);
    }
  } else {
    auto support_mask = [&](size_t i) -> uint64_t {          // every address bit op i reads or writes
      const LocalOp& lo = g.ops[i];
      uint64_t m = 0;
      if (lo.target >= 0) m |= 1ull << lo.target;
      for (int q : lo.list) m |= 1ull << q;
      for (int q : lo.cq) m |= 1ull << q;
      return m;
    };
    auto target_mask = [&](size_t i) -> uint64_t { return g.ops[i].target >= 0 ? 1ull << g.ops[i].target : 0ull; };
    auto commute = [&](size_t i, size_t j) -> bool {
      return !(target_mask(i) & support_mask(j)) && !(target_mask(j) & support_mask(i));
    };
    struct Round { std::vector<int> list; std::vector<int> gate; std::vector<int> members; };
    std::vector<Round> rounds(1);
    rounds[0].gate.assign(std::max(R, 1), -1);
    int bp = 0;                                            // gates of the current round occupy bits < bp
    for (size_t i = 0; i < mops.size(); ++i) {
      const MultiOp& mo = mops[i];
      Round* cur = &rounds.back();
      const bool is_list = mo.type == 1 || mo.type >= 3;
      bool fits;
      if (is_list) {
        // the list runs before the round's gates: fine if there are none yet, or if op i commutes
        // with every gate already placed in this round
        fits = true;
        for (int gi : cur->gate) if (gi >= 0 && !commute(i, (size_t)gi)) { fits = false; break; }
      } else {
        fits = cur->gate[mo.bit] < 0;
        if (fits && mo.bit < bp)                           // would run before later-placed higher bits? no: lower bits run first
          for (int gi : cur->gate) if (gi >= 0 && mops[gi].bit > mo.bit && !commute(i, (size_t)gi)) { fits = false; break; }
      }
      if (!fits) {
        rounds.emplace_back();
        cur = &rounds.back();
        cur->gate.assign(std::max(R, 1), -1);
        bp = 0;
      }
      if (is_list) cur->list.push_back((int)i);
      else { cur->gate[mo.bit] = (int)i; bp = std::max(bp, mo.bit + 1); }
    }
    MultiOp ident;                                         // simple passes run a gate in every slot
    memset(&ident, 0, sizeof ident);
    ident.uniform = 1;
    ident.tab = (int)(tables.size() / 2);
    if (simple && R > 0) { const double id4[8] = {1, 0, 0, 0, 0, 0, 1, 0}; tables.insert(tables.end(), id4, id4 + 8); }
    for (const Round& rd : rounds) {
      MultiSlot ls;
      ls.first = (int)sorted.size();
      ls.ndiag = (int)rd.list.size();
      ls.has = 0;
      ls.pad = 0;
      for (int idx : rd.list) sorted.push_back(mops[idx]);
      slots.push_back(ls);
      for (int b = 0; b < R; ++b) {
        MultiSlot gs;
        gs.first = (int)sorted.size();
        gs.ndiag = 0;
        gs.has = rd.gate[b] >= 0;
        gs.pad = 0;
        if (rd.gate[b] >= 0) sorted.push_back(mops[rd.gate[b]]);
        else if (simple) { ident.bit = b; sorted.push_back(ident); }
        slots.push_back(gs);
      }
    }
  }
  const int nrounds = simple ? (int)slots.size() / NS : (int)sorted.size();   // general pass: number of ops
  void* dops = nullptr;
  void* dslots = nullptr;
  void* dtab = nullptr;
  CHK(arena_put(s, sorted.data(), sorted.size() * sizeof(MultiOp), &dops));
  if (!simple) CHK(arena_put(s, combos.data(), combos.size() * sizeof(int), &dslots));
  else CHK(arena_put(s, slots.data(), slots.size() * sizeof(MultiSlot), &dslots));
  if (tables.empty()) tables.assign(2, 0.0);
  CHK(arena_put(s, tables.data(), tables.size() * sizeof(double), &dtab));
  const int ntab = (int)(tables.size() / 2);
  const uint64_t nthreads = n >> (R + nzout);
  if (nthreads >= (1ull << 32)) return fail(QSV_E_UNSUPPORTED, "k_multi pass of 2^%d threads exceeds the launch limit", h->L - R - nzout);
  const double n_written = (double)(n >> nzout);
  const double n_read = g.init ? 0.0 : (double)(n >> (nzout + __builtin_popcount(zreg)));
  const double bytes = 16.0 * (n_written + n_read);
  h->stats.fused_gates += g.ops.size();
  const bool init = g.init;
  const uint64_t nonmask = g.nonmask;
  const double initval = g.initval;
  // X frame: this pass applies the pending X gates on the bits where a store through the XOR-ed address
  // cannot overtake another wave's load: its register bits and the address bits its lane id supplies
  // (the wave that stores there loaded it); a write-only pass reads nothing, so every bit.  The rest
  // stays pending for the next group.
  uint64_t xsafe = regmask;
  for (int lb = 0; lb < 6; ++lb) xsafe |= (uint64_t)tile_base_thr(1u << lb, ins, lp);
  if (g.init) xsafe = ~0ull;
  const uint64_t xmask = g.xframe & xsafe, xleft = g.xframe & ~xsafe;
  // the program's last pass also reduces |amp|^2 per workgroup tile: measurement then needs no read pass
  double* tsums = nullptr;
  if (final_pass && h->opt_fused_sums && nthreads % QSV_TPB == 0 && nthreads >= QSV_TPB) {
    const uint64_t nb = nthreads / QSV_TPB;
    if (s.tsums_cap < nb) {
      if (s.d_tsums) HIPCHK(hipFree(s.d_tsums));
      HIPCHK(hipMalloc(&s.d_tsums, nb * sizeof(double)));
      s.tsums_cap = nb;
    }
    tsums = s.d_tsums;
    s.tile_R = R;
    s.tile_rp = rp;
    s.tile_lp = lp;
    s.tile_ins = ins;
    s.tile_nblocks = nb;
    s.tile_xor = xmask;
  }
  // MODE 2: simple pass whose every 2x2 table entry is RX-like (real diagonal, imaginary off-diagonal)
  int mode = simple ? 1 : 0;
  if (simple) {
    bool rx = true;
    for (const MultiOp& mo : sorted) {
      if (mo.type == 1) { rx = false; break; }           // a complex diagonal does not fit the RX-like form
      if (mo.type != 0 && mo.type != 4) continue;
      const size_t nent = (size_t)1 << mo.nlist;
      for (size_t e = 0; e < nent && rx; ++e) {
        const double* m = &tables[2 * ((size_t)mo.tab + 4 * e)];
        if (m[1] != 0.0 || m[7] != 0.0 || m[2] != 0.0 || m[4] != 0.0) rx = false;
      }
      if (!rx) break;
    }
    if (rx) mode = 2;
  }
  if (h->opt_trace_passes) {
    int hist[11] = {0};
    for (const MultiOp& mo : sorted) ++hist[mo.shape];
    fprintf(stderr, "[qsv pass] shard %d R %d mode %d init %d ops %zu xframe %d | tab %d/%d x %d mat %d | diag %d/%d phase %d | lane tab %d/%d x %d mat %d"
                    " | rounds %d lanes %d/%d/%d tables %d\n",
            (int)(&s - &h->shards[0]), R, mode, (int)init, g.ops.size(), __builtin_popcountll(xmask), hist[GS_TAB_T], hist[GS_TAB_P], hist[GS_X],
            hist[GS_MAT], hist[GS_DIAG_T], hist[GS_DIAG_A], hist[GS_PHASE], hist[GS_LTAB_T], hist[GS_LTAB_A], hist[GS_LX], hist[GS_LMAT],
            nrounds, lp.pos[0], lp.pos[1], lp.pos[2], ntab);
  }
  if (mode == 0 && R > QSV_GENERAL_MAXR) return fail(QSV_E_UNSUPPORTED, "general k_multi pass on %d register bits (limit %d)", R, QSV_GENERAL_MAXR);
  // the init-fused pass (write only) is a different kernel instantiation: accounted on its own
  const int r = launch(h, s, init ? QSV_K_MULTI_INIT : QSV_K_MULTI, bytes, [&] {
    const MultiOp* o = reinterpret_cast<const MultiOp*>(dops);
    const MultiSlot* sl = reinterpret_cast<const MultiSlot*>(dslots);
    const cplx* tp = reinterpret_cast<const cplx*>(dtab);
    switch (R) {
      case 0: launch_multi<0>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      case 1: launch_multi<1>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      case 2: launch_multi<2>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      case 3: launch_multi<3>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      case 4: launch_multi<4>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      case 5: launch_multi<5>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
      default: launch_multi<6>(h, s, init, mode, nthreads, ins, rp, lp, o, sl, nrounds, tp, ntab, nonmask, initval, zreg, tsums, xmask); break;
    }
  });
  s.tile_fresh = tsums != nullptr;
  if (tsums) s.sums_from_gen = false;
  g = PendingGroup();
  g.xframe = xleft;
  return r;
}

// flush, and leave no X pending either (before anything that is not a grouped pass reads the shard)
static int flush_group_hard(qsv_handle* h, Shard& s, PendingGroup& g, bool final_pass = false) {
  CHK(flush_group(h, s, g, final_pass));
  if (g.xframe) {
    CHK(flush_group(h, s, g));                 // no ops left: the pending X gates run as swaps
    s.tile_fresh = false;                      // ... after the pass that left its tile sums behind
  }
  return QSV_OK;
}
