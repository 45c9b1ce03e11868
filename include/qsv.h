/*
 * qsv.h -- C ABI of libqsv.so, the MI355X (gfx950) fp64 statevector engine that replaces
 * the Qiskit-Aer call of the reference's hot path:
 *
 *     simulator = Aer.get_backend('qasm_simulator')            /root/reference/run_experiment.py:54
 *     result    = simulator.run(T, shots=SHOTS).result()       /root/reference/run_experiment.py:56
 *     counts    = result.get_counts()                          /root/reference/run_experiment.py:57
 *
 * The reference's "FFI" for this path is the Python -> Aer C++ extension call hidden inside
 * run(); this header is what a ctypes (or cgo / JNI) binding of that call binds instead.
 * Every entry point names the reference gate / step it executes (file:line into
 * /root/reference).  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *  - amplitude vector: 2^n_qubits complex128, interleaved (re, im); qubit q <-> bit q of the
 *    basis index (Qiskit little-endian).  Qubit numbers here are PHYSICAL positions; the
 *    Python host keeps the logical->physical layout map.
 *  - sharding: P = 2^g shards by the g highest physical qubits; shard s holds indices
 *    [s << L, (s+1) << L), L = n_qubits - g.  Qubits >= L are "shard bits".
 *  - every pointer argument is a caller-owned host buffer, read or filled synchronously;
 *    nothing is retained after return.  No callbacks.
 *  - return 0 on success; <0 on error (QSV_E_*); text via qsv_last_error() (thread local).
 *  - a handle is not thread-safe; distinct handles may be used from distinct threads.
 *  - gate calls are asynchronous on the device stream(s); results are synchronised by
 *    qsv_sync / qsv_probabilities / qsv_sample / qsv_get_amplitudes / qsv_get_stats.
 */
#ifndef QSV_H
#define QSV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qsv_handle qsv_handle;

#define QSV_OK             0
#define QSV_E_BADARG      -1
#define QSV_E_NOMEM       -2
#define QSV_E_HIP         -3
#define QSV_E_RCCL        -4
#define QSV_E_UNSUPPORTED -5

#define QSV_MAX_CTRL      16   /* controls of one gate / qubits of one diagonal        */
#define QSV_MAX_KQ         5   /* dense k-qubit unitary                                */
#define QSV_UNIQUE_ID_BYTES 128

/* kernel kinds, index into qsv_stats.per_kind[] */
enum {
  QSV_K_INIT = 0, QSV_K_1Q, QSV_K_X, QSV_K_DIAG, QSV_K_MCPHASE, QSV_K_MUX, QSV_K_KQ,
  QSV_K_PROB, QSV_K_SWAP, QSV_K_EXCHANGE, QSV_K_MULTI, QSV_K_MULTI_INIT, QSV_K_INIT_PROD, QSV_K_COUNT
};

typedef struct {
  uint64_t launches;          /* kernel launches of this kind                              */
  double   algorithmic_bytes; /* SURVEY.md 8(d) byte model, summed                         */
  double   device_ms;         /* HIP-event time on the launch stream (profiling on only)   */
} qsv_kind_stats;

typedef struct {
  qsv_kind_stats per_kind[QSV_K_COUNT];
  uint64_t exchanges;         /* shard-bit exchanges performed                              */
  double   exchange_bytes;    /* bytes sent over the fabric by this process                 */
  uint64_t fused_gates;       /* gates executed inside multi-gate (QSV_K_MULTI) passes      */
} qsv_stats;

/* ---- life cycle -------------------------------------------------------------------- */

/* number of visible HIP devices (<0 on error) */
int qsv_device_count(void);

/* HBM of one device in bytes (free now / total): lets the caller size a state vector to the
 * card (2^34 complex128 = 256 GiB fits the 288 GiB of one MI355X). */
int qsv_device_memory(int device_id, uint64_t* free_bytes, uint64_t* total_bytes);

/* PCI bus id of a device ("0000:05:00.0"): two ranks that report the same id on the same host
 * share one GPU (RCCL refuses that; the peer-mapped transport below does not mind) */
int qsv_device_bus_id(int device_id, char* out, int len);

/* One process drives n_devices shards (n_devices a power of two).  device_ids[i] is the HIP
 * device of shard i; repeating an id places several ("virtual") shards on one GPU.
 * Replaces: the state allocation inside Aer's run() (run_experiment.py:56). */
int qsv_create(int n_qubits, int n_devices, const int* device_ids, qsv_handle** out);

/* One process per GPU (torchrun-style launch): this process owns shard `rank` of
 * `world_size` (a power of two) on HIP device device_id.  Exchanges go over RCCL once
 * qsv_comm_init has been called on every rank. */
int qsv_create_rank(int n_qubits, int world_size, int rank, int device_id, qsv_handle** out);

/* RCCL bootstrap for qsv_create_rank handles: rank 0 calls qsv_comm_unique_id, the host
 * side broadcasts the 128 bytes, every rank calls qsv_comm_init (collective). */
int qsv_comm_unique_id(uint8_t id[QSV_UNIQUE_ID_BYTES]);
int qsv_comm_init(qsv_handle* h, const uint8_t id[QSV_UNIQUE_ID_BYTES]);

/* Peer-mapped exchange (alternative transport for qsv_create_rank handles on ONE node): every
 * rank exports an IPC handle of its shard, the host side all-gathers the QSV_IPC_HANDLE_BYTES
 * each and every rank attaches the others; `shm_name` names a small POSIX shared-memory segment
 * (created by the rank that passes create != 0, before the others attach) through which a pair
 * of ranks synchronises around an exchange.  With it a shard-bit exchange is ONE kernel per rank
 * that swaps its half of the pairs in place, reading and writing the partner's shard directly
 * (over xGMI between GPUs; plain HBM when two ranks share a device, which RCCL refuses) -- no
 * staging buffers, each amplitude crosses the link once.  RCCL stays the default transport
 * whenever every rank has a device of its own. */
#define QSV_IPC_HANDLE_BYTES 64
int qsv_ipc_export(qsv_handle* h, uint8_t out[QSV_IPC_HANDLE_BYTES]);
int qsv_ipc_attach(qsv_handle* h, const uint8_t* handles /* world x QSV_IPC_HANDLE_BYTES */,
                   const char* shm_name, int create);

/* Diagnostic: bring RCCL up on one device as a 1-rank communicator and push `n_doubles` through
 * the same grouped ncclSend/ncclRecv + stream sequence the shard exchange uses (rank 0 to itself),
 * then compare.  Exercises the dlopen binding, communicator life cycle and call order on a box
 * with a single GPU, where RCCL refuses two ranks on one device.  0 on success. */
int qsv_rccl_selftest(int device_id, uint64_t n_doubles);

/* Diagnostic: the RCCL side of a BATCHED exchange (several shard bits at once = an all-to-all inside a
 * group of shards) on a 1-rank communicator with rank 0 as its own peers: staging buffers, the
 * two-stream double-buffered pack / grouped send+recv / unpack pipeline in chunks of 2^chunk_log2
 * amplitudes over a 2^n_qubits shard, verified element by element.  0 on success. */
int qsv_rccl_exchange_selftest(int device_id, int n_qubits, int chunk_log2);

/* Diagnostic: leave quiet NaNs in the LDS of every compute unit of the handle's devices (LDS is not cleared
 * between kernels).  A kernel that reads a table it never staged then produces NaN deterministically instead
 * of "usually fine" -- used by the GPU tests before the init passes, whose idle workgroups skip the staging. */
int qsv_poison_lds(qsv_handle* h);

int qsv_destroy(qsv_handle* h);
int qsv_sync(qsv_handle* h);

/* ---- state preparation -------------------------------------------------------------- */

/* |0...0>  -- implicit initial state of a QuantumCircuit (QCMRF.py:78). */
int qsv_init_zero(qsv_handle* h);

/* H on every qubit of qubit_mask applied to |0...0>, written directly:
 * amp = 2^{-popcount/2} where (index & ~mask) == 0, else 0.   (QCMRF.py:204-205) */
int qsv_init_uniform(qsv_handle* h, uint64_t qubit_mask);

/* ---- gates -------------------------------------------------------------------------- */

/* dense 2x2 on qubit t; m = row-major {re,im} x 4.   h / sx (QCMRF.py:231,236; basis 'sx'
 * run_experiment.py:52). */
int qsv_apply_1q(qsv_handle* h, int t, const double m[8]);

/* multi-controlled 2x2: fires where bit ctrls[i] == ctrl_vals[i] (NULL = all ones). */
int qsv_apply_mc1q(qsv_handle* h, int n_ctrl, const int* ctrls, const int* ctrl_vals,
                   int t, const double m[8]);

/* X / CX / CCX / MCX(k) with +-control flags: the AND gate of QCMRF.py:224-225,227, the
 * x of QCMRF.py:233,235, basis 'cx','x'. */
int qsv_apply_mcx(qsv_handle* h, int n_ctrl, const int* ctrls, const int* ctrl_vals, int t);

/* k-qubit diagonal: amp[i] *= table[j], j = sum_b bit(i, qubits[b]) << b; table = 2^k x {re,im}.
 * rz / p / merged phase blocks (cU_C of QCMRF.py:218-228 is one such table). */
int qsv_apply_diag(qsv_handle* h, int k, const int* qubits, const double* table);

/* e^{i angle} on the subspace where bit ctrls[i] == ctrl_vals[i] for all i (n_ctrl >= 1).
 * cp(2 gamma, n, anc) of QCMRF.py:226 is n_ctrl = 2. */
int qsv_apply_mcphase(qsv_handle* h, int n_ctrl, const int* ctrls, const int* ctrl_vals,
                      double angle);

/* uniformly controlled 2x2 on t: mats[j] (8 doubles each), j = control bits, ctrls[0] = LSB.
 * The whole real-part-extraction sandwich H cU X cU^dg X H of QCMRF.py:231-236 is one of
 * these. */
int qsv_apply_mux_1q(qsv_handle* h, int k, const int* ctrls, int t, const double* mats);

/* dense 2^k x 2^k unitary (k <= QSV_MAX_KQ), row-major {re,im}; index bit b <-> qubits[b].
 * Fused blocks of a transpiled circuit (run_experiment.py:52). */
int qsv_apply_kq(qsv_handle* h, int k, const int* qubits, const double* u);

/* physically swap the amplitude-index positions a[i] <-> b[i].  Both local: a permutation
 * sweep.  One of them a shard bit: the pairwise half-shard exchange (in-place swap kernel for
 * virtual shards and peer-mapped ranks, peer copy between devices of one process, RCCL
 * send/recv between ranks).  Several such pairs on distinct qubits in ONE call are executed as
 * one batched exchange: an all-to-all inside every group of 2^k shards (each shard sends 1/2^k
 * of itself to each of its 2^k - 1 partners, all links busy at once) instead of k sequential
 * half-shard exchanges.  The RCCL path is chunked and double buffered (pack / unpack on a second
 * stream while the neighbouring chunk is on the wire). */
int qsv_swap_layout(qsv_handle* h, int npairs, const int* a, const int* b);

/* ---- measurement (QCMRF.py:239,243; shots of run_experiment.py:56) -------------------- */

/* marginal distribution over `qubits` (k <= 26): out[j] += sum |amp|^2, j as in qsv_apply_diag.
 * Only amplitudes with (index & fix_mask) == fix_val contribute (fix_mask = 0: all).
 * Multi-process handles return this rank's partial sums. */
int qsv_probabilities(qsv_handle* h, const int* qubits, int k, double* out);
int qsv_probabilities_cond(qsv_handle* h, const int* qubits, int k,
                           uint64_t fix_mask, uint64_t fix_val, double* out);

/* expectation of a real DIAGONAL observable on the resident state: table has 2^k doubles, indexed
 * like qsv_apply_diag's (k <= 26; qubits may include shard bits).  Only amplitudes whose global
 * index g has (g & fix_mask) == fix_val contribute:
 *     out[0] = sum |amp[g]|^2 table[j(g)]      out[1] = sum |amp[g]|^2      (both over those g)
 * so out[0] / out[1] is the expectation in the post-selected state (fix_mask = 0: plain <O>,
 * out[1] = norm).  One read pass over the shard(s), 16 B per amplitude.  Multi-process handles
 * return this rank's partial sums.
 * Replaces: the opflow expectation of QCMRF.Hamiltonian() / sufficient_statistic()
 * (QCMRF.py:159-193): H = -sum theta_{C,y} Phi_{C,y} is diagonal in the computational basis. */
int qsv_expect_diag(qsv_handle* h, const int* qubits, int k, const double* table,
                    uint64_t fix_mask, uint64_t fix_val, double out[2]);

/* sum |amp|^2 over this process's shards */
int qsv_norm(qsv_handle* h, double* out);

/* draw `shots` basis states from |amp|^2 over this process's shards (normalised by their
 * mass); out_bits[s] bit j = value of qubit meas_qubits[j] (n_meas <= 64; an entry of -1 leaves
 * bit j at 0: a classical bit no measurement writes).
 * meas_qubits == NULL: out_bits[s] = the full basis index. */
int qsv_sample(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits,
               int n_meas, uint64_t* out_bits);

/* qsv_sample restricted to the basis states g with (g & fix_mask) == fix_val (global index bits, shard bits allowed):
 * shots are drawn from |amp|^2 over those states, normalised by their mass on this process; *mass receives that
 * mass (not normalised by qsv_norm; mass may be NULL).  shots == 0: the mass only.  fix_mask == 0: the words of
 * qsv_sample, word for word, and mass = qsv_norm.  mass == 0 with shots > 0: QSV_E_BADARG "post-selected outcome has
 * zero probability".  fix_val & ~fix_mask != 0, or a mask bit at or above n_qubits: QSV_E_BADARG.
 * The contract is qsv_sample's, applied to the matching states: std::mt19937_64(seed) draws shots + 1 spacings, the
 * uniforms are scaled to the conditional mass, the inverse-CDF walk runs in ascending global index over the matching
 * states, the same Fisher-Yates shuffle follows.
 * Cost: with f fixed bits local to a shard, the matching amplitudes are a sub-cube of 2^(L-f) entries ("compact index
 * space"); one read pass over them (booked under QSV_K_PROB with 16 B each) and one locating kernel, nothing else of the
 * shard is touched, implied zeros are not read.  The sums of a conditioned call are NOT cached: a second call repeats
 * the 2^-f pass.  At most 28 fixed bits local to a shard (QSV_E_UNSUPPORTED beyond).
 * A deferred shard (qsv_state_info) is not written out when the call fixes a block bit of the generator's tile index:
 * the tiles that hold the sub-cube are listed and stored (one listed_launches), the shard stays deferred; otherwise, and
 * by option post_select_list, it is realised first. */
int qsv_sample_cond(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                    uint64_t fix_mask, uint64_t fix_val, uint64_t* out_bits, double* mass);

/* qsv_sample and qsv_sample_cond for callers that only count outcomes.  Same arguments.  out_bits receives exactly the
 * multiset of words the ordered call returns for the same handle state, shots, seed and measurement map; the ORDER is
 * unspecified (today: ascending in the walk's order, the Fisher-Yates shuffle is neither drawn nor applied, and the words
 * are copied from the device straight into out_bits, one host wait as before).  Everything else is the ordered call's:
 * the errors and their text (zero norm, bad qubit, zero mass; out_bits is then undefined), *mass, and the effects on the
 * handle -- qsv_state_info (deferred, realize_calls, listed_launches), the cached sums, the stats.  Callers that hand
 * shots out one by one, in order, keep the ordered calls. */
int qsv_sample_unordered(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits,
                         int n_meas, uint64_t* out_bits);
int qsv_sample_cond_unordered(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                              uint64_t fix_mask, uint64_t fix_val, uint64_t* out_bits, double* mass);

/* Many marginals of the conditioned state in one pass.  Group g lists group_k[g] distinct qubits (the lists concatenated
 * in `qubits`; groups may overlap, group_k[g] == 0 is allowed); off_g = sum of 2^group_k over the groups before g.
 *   out[off_g + j] = sum |amp[x]|^2 over the global indices x owned by this process with (x & fix_mask) == fix_val whose
 *                    bits qubits_g[b] spell j (bit b of j <-> qubits_g[b], as in qsv_apply_diag);
 *   *mass          = the same sum without the bin condition (mass may be NULL).
 * Not normalised; the shards of a process are summed, handles of several ranks return this rank's part.  A group qubit
 * may be a shard bit (its value is the shard's) or a fixed bit (the bins contradicting fix_val are exactly 0.0; a group
 * without qubits has one bin, the mass); a fixed shard bit skips the shards that disagree, as in qsv_sample_cond.
 * Cost: one pass over the compact index space of qsv_sample_cond, 2^(L-f) loads per shard for f fixed bits local to it
 * (booked under QSV_K_PROB with 16 B each, one launch of that kind per shard); implied zeros are not loaded; nothing is
 * cached between calls.  A deferred shard is prepared exactly as for qsv_sample_cond (the tiles holding the sub-cube
 * listed and stored, one listed_launches, the shard still deferred -- or realised, by the same rule and option
 * post_select_list); with fix_mask == 0 the sub-cube is the shard and a deferred shard is realised.
 * Reproducible: out and *mass are a pure function of (shard contents, shard structure, groups, mask) -- the same bits
 * from call to call, for every number of workgroups (option marginals_grid), for a stored and for a deferred-and-listed
 * shard: a fixed tree of additions (spelled out in qsv_marginals.inc), no floating-point atomics.
 * QSV_E_BADARG, checked before the first launch, with a message naming the group: a NULL argument, n_groups outside
 * 1..QSV_MARG_MAX_GROUPS, a group_k outside 0..QSV_MARG_MAX_K, more than QSV_MARG_MAX_BINS bins, a qubit at or above
 * n_qubits, a qubit repeated within a group, fix_val outside fix_mask, a mask bit at or above n_qubits.  More than 28
 * fixed bits local to a shard: QSV_E_UNSUPPORTED. */
#define QSV_MARG_MAX_GROUPS 64     /* groups of one call                         */
#define QSV_MARG_MAX_K       8     /* qubits of one group                        */
#define QSV_MARG_MAX_BINS 4096     /* sum over the groups of 2^k_g (32 KiB)      */
int qsv_marginals_cond(qsv_handle* h, int n_groups, const int* group_k, const int* qubits,
                       uint64_t fix_mask, uint64_t fix_val, double* out, double* mass);

/* The same marginals for n_rows conditions (fix_mask[r], fix_val[r]) on one state -- one conditional query per data row
 * of a model -- from one launch group and one host wait per shard, not per row.  nbins = sum of 2^group_k.
 * The contract: row r of out (n_rows x nbins, row-major) and mass[r] (mass may be NULL) are, byte for byte, what
 * qsv_marginals_cond(h, n_groups, group_k, qubits, fix_mask[r], fix_val[r], ...) writes on the same handle state -- for
 * every number of workgroups (marginals_grid), every split of the rows over launches (marginals_rows), every order and
 * composition of the batch (a row repeated, alone, the rows reversed), stored and deferred shards.  Every row keeps its
 * own compact index space and its own chunking and takes the tree of additions of qsv_marginals.inc; no floating-point
 * atomics.  A row of zero mass is not an error: its bins and its mass are +0.0.
 * Cost: per shard on which at least one row is live (a row whose fixed shard bits disagree with a shard is skipped
 * there) one table upload, one launch booked under QSV_K_PROB with 16 B times the sum of the live rows' 2^(L-f), and
 * one host wait.  Rows with the same local mask share one descriptor; a row adds 16 bytes.  Where the descriptors exceed
 * half the arena or the partial sums the kept reduction scratch (2^24 doubles), the rows are processed in slabs of
 * consecutive rows, each costing the above once; option marginals_rows caps a slab's rows.
 * A deferred shard is prepared once per call, exactly as qsv_marginals_cond would for the COMMON condition (the bits set
 * in every row's mask with the same value in every row): its tiles listed (one listed_launches, still deferred) or the
 * shard realised, by the same rule and option post_select_list; an empty common condition realises.
 * QSV_E_BADARG before the first launch, the handle usable afterwards: what qsv_marginals_cond refuses about the groups
 * (same messages), n_rows outside 1..QSV_MARG_MAX_ROWS, NULL fix_mask / fix_val / out, and with a message "row %d: ..."
 * a fix_val outside its mask or a mask bit at or above n_qubits.  More than 28 fixed bits local to a shard in some row:
 * QSV_E_UNSUPPORTED, naming the row. */
#define QSV_MARG_MAX_ROWS 65536
int qsv_marginals_cond_rows(qsv_handle* h, int n_groups, const int* group_k, const int* qubits,
                            int n_rows, const uint64_t* fix_mask, const uint64_t* fix_val,
                            double* out  /* n_rows x nbins, row-major */,
                            double* mass /* n_rows, may be NULL */);

/* The k most probable basis states of the conditioned state in one pass: exact MAP (k = 1) and top-k inference.
 * Candidates: the global indices x owned by this process with (x & fix_mask) == fix_val; the weight of x is
 *   p(x) = re*re + im*im, each product and the sum rounded separately, no fused contraction -- deliberately NOT the fma
 *   the summing kernels (qsv_marginals_cond, qsv_expect_diag) use: numpy's a.real*a.real + a.imag*a.imag on the
 *   amplitudes read back gives the same bits.
 * Order: x comes before y iff p(x) > p(y), or p(x) == p(y) and x < y -- strict and total.
 * Output: the first min(k, number of candidates with p > 0) candidates in that order, out_index[i] and out_p[i];
 *   *n_found is that number.  A candidate whose p is not > 0 (a 0, an implied zero, a NaN) is never returned; entries of
 *   out_index / out_p from n_found on are left untouched.
 * The shards of a process are merged on the host by the same order, an index carries its shard's bits; a fixed shard bit
 * skips the shards that disagree, as in qsv_marginals_cond; handles of several ranks return this rank's part.
 * The result is a pure function of the state: selection under a strict total order does not depend on the number of
 * workgroups (option top_grid) or on the order in which candidates are compared; no floating-point atomics.
 * Cost: one pass over the compact index space of qsv_sample_cond, 2^(L-f) loads per shard for f fixed bits local to it
 * (booked under QSV_K_PROB with 16 B each, one launch of that kind per shard); implied zeros are not loaded; nothing is
 * cached between calls.  A deferred shard is prepared exactly as for qsv_marginals_cond (the tiles holding the sub-cube
 * listed and stored, one listed_launches, the shard still deferred -- or realised, by the same rule and option
 * post_select_list); with fix_mask == 0 a deferred shard is realised.
 * QSV_E_BADARG, checked before the first launch, with a message: a NULL argument, k outside 1..QSV_TOP_MAX_K, fix_val
 * outside fix_mask, a mask bit at or above n_qubits.  More than 28 fixed bits local to a shard: QSV_E_UNSUPPORTED.
 * After a refusal the handle is usable. */
#define QSV_TOP_MAX_K 64
int qsv_top_cond(qsv_handle* h, int k, uint64_t fix_mask, uint64_t fix_val,
                 uint64_t* out_index /* k */, double* out_p /* k */, int* n_found);

/* copy amplitudes [start, start+count) of the GLOBAL index space into out (2*count doubles);
 * the range must lie inside shards owned by this process. */
int qsv_get_amplitudes(qsv_handle* h, uint64_t start, uint64_t count, double* out);
int qsv_set_amplitudes(qsv_handle* h, uint64_t start, uint64_t count, const double* in);

/* dst <- src (same n_qubits and shard structure), device to device.  Branch points of the
 * trajectory mode: the mid-circuit measure of QCMRF.py:238-239 taken when it occurs. */
int qsv_copy_state(qsv_handle* dst, qsv_handle* src);

/* ---- slots: the branches of one level of a trajectory run, side by side ------------- */

/* A slot is an aligned block of 2^w amplitudes of a single-shard, single-process handle of W >= w qubits: slot b starts at
 * amplitude b << w (the branch number rides on the qubits >= w, so one qsv_exec of gates on qubits < w evolves every slot
 * alike, and an all-zero slot stays zero).  Handles of several shards or ranks return QSV_E_BADARG.  Both entries realise a
 * deferred state and write implied zeros before they read (qsv_state_info).
 *
 * qsv_branch_mass: out[2b] = sum |amp|^2 over slot b with bit `qubit` = 0, out[2b+1] the same with the bit = 1, for
 * b < n_slots (0 <= qubit < w, 1 <= n_slots <= 2^(W-w); out holds 2 n_slots doubles).  One read pass over n_slots << w
 * amplitudes, no atomics, one copy and one stream synchronisation; the partial sums live in the shard's reduction scratch,
 * which is kept between calls up to 2^24 doubles -- a call that needs more (2 n_slots + 2 (n_slots << w) / 1024 doubles for
 * w > 10, e.g. all 8192 slots of w = 20 in W = 33) allocates and frees its scratch itself.  The two sums of a slot are a pure function of (w, qubit,
 * the slot's contents): the same bits whatever n_slots, the slot's position, W or the grid (the tree of additions is
 * spelled out in qsv_branch.hip).  Booked under QSV_K_PROB. */
int qsv_branch_mass(qsv_handle* h, int w, uint64_t n_slots, int qubit, double* out /* 2 * n_slots */);

/* qsv_branch_split: slot c of dst, c < n_children, becomes slot parent[c] of src projected on bit `qubit` == outcome[c]:
 * the kept amplitudes bit for bit, the other half zero.  With release != 0 a kept half of outcome 1 is stored at bit
 * `qubit` = 0 instead (the projection followed by X: the measured qubit handed back in |0>).  Every further slot of dst, up
 * to 2^(W_dst - w), is written zero.  dst != src, both on one device; W_dst and W_src may differ, each >= w (W_dst = w with
 * one child extracts a branch into an ordinary state); 1 <= n_children <= 2^(W_dst - w), parent[c] < 2^(W_src - w), a parent
 * may occur any number of times.  One pass: reads the kept halves, writes all of dst, which afterwards is a plainly stored
 * state.  Runs on dst's stream, ordered after everything asked of src so far, and src's stream waits for it as in
 * qsv_copy_state: src may be reused at once.  Booked under QSV_K_SWAP of dst. */
int qsv_branch_split(qsv_handle* dst, qsv_handle* src, int w, uint64_t n_children, const uint32_t* parent,
                     const uint8_t* outcome, int qubit, int release);

/* ---- batched execution -------------------------------------------------------------- */

enum {
  QSV_OP_INIT_ZERO = 0, QSV_OP_INIT_UNIFORM, QSV_OP_1Q, QSV_OP_MCX, QSV_OP_DIAG,
  QSV_OP_MCPHASE, QSV_OP_MUX, QSV_OP_KQ, QSV_OP_SWAP,
  QSV_OP_PAULI,     /* random Pauli on qubits[0..n) (n <= 2), qsv_noisy_sample only: data_off points to the 4^n
                       CUMULATIVE probabilities; Pauli index p holds for error qubit j the x bit (p >> 2j) & 1 and
                       the z bit (p >> 2j+1) & 1 -- (x,z) = (0,0) I, (1,0) X, (0,1) Z, (1,1) Y               */
  QSV_OP_KRAUS = 10,/* one-qubit Kraus channel of m = vals[0] operators (1 <= m <= 4) on qubits[0] (n = 1),
                       qsv_noisy_sample only: data_off points to m x 8 doubles, each K_k row-major with (re, im) pairs as
                       for QSV_OP_1Q, followed by m x 4 doubles, E_k = K_k^dg K_k as (E00, E11, Re E01, Im E01).  Per
                       shot one k is drawn with weight <psi|E_k|psi> and K_k applied, the state keeping its mass. */
  QSV_OP_MEASURE = 11,/* measurement of qubits[0] (n = 1) taken when it occurs, qsv_noisy_sample only: vals[0] = the classical
                       bit c it writes (0 <= c < 64), vals[1] = release (0 or 1: hand the qubit back in |0>), data_off points
                       to 2 doubles, P(flip | 0) and P(flip | 1) (always present; zeros: no readout error).  The contract
                       is below, next to the one of QSV_OP_KRAUS. */
  QSV_OP_KRAUS2 = 12,/* two-qubit Kraus channel of m = vals[0] operators (1 <= m <= 16) on the distinct qubits qubits[0] and
                       qubits[1] (n = 2), qsv_noisy_sample only: data_off points to m x 32 doubles, each K_k (4 x 4) row-major
                       with (re, im) pairs, matrix index bit j on qubits[j], followed by m x 16 doubles, E_k = K_k^dg K_k packed
                       as its 4 real diagonal entries E00 E11 E22 E33, then its 6 upper off-diagonal entries (0,1) (0,2) (0,3)
                       (1,2) (1,3) (2,3) as (re, im).  The contract is below, behind the one of QSV_OP_KRAUS. */
  QSV_OP_IF = 13,   /* guard over the next `span` records on the shot's classical word, qsv_noisy_sample only: n = span (>= 1; NOT a
                       number of listed qubits, and not bounded by QSV_MAX_CTRL), mask = the classical bits compared, vals[0] and
                       vals[1] = the low and the high 32 bits of the value they must read, target = negate (0 or 1).  qubits,
                       data_off and angle are not read.  The contract is below, behind the one of QSV_OP_MEASURE. */
  QSV_OP_RESET = 14 /* reset of qubits[0] (n = 1) to |0>, qsv_noisy_sample only: a MEASURE record with release = 1 that writes no
                       classical bit and takes no readout draw.  vals and data_off are not read.  The contract is below. */
};

/* scheduling hint from the planner: close the current multi-gate pass before this gate (the
 * result does not depend on it; it only decides which gates share one sweep of the shard) */
#define QSV_OPF_NEW_PASS 1

typedef struct {
  int32_t  kind;                   /* QSV_OP_*                                             */
  int32_t  target;                 /* target qubit (1Q, MCX, MUX)                          */
  int32_t  n;                      /* number of controls / qubits in qubits[]              */
  int32_t  flags;                  /* QSV_OPF_*                                            */
  int32_t  qubits[QSV_MAX_CTRL];   /* controls, or qubit list (DIAG, KQ), or swap a-list   */
  int32_t  vals[QSV_MAX_CTRL];     /* control values, or swap b-list                       */
  uint64_t data_off;               /* offset in doubles into `data` (matrix / table)       */
  uint64_t mask;                   /* INIT_UNIFORM qubit mask                              */
  double   angle;                  /* MCPHASE                                              */
} qsv_op;

/* run a whole program in one call (one ctypes crossing per circuit); QSV_OP_PAULI, QSV_OP_KRAUS, QSV_OP_KRAUS2, QSV_OP_MEASURE,
 * QSV_OP_IF and QSV_OP_RESET are refused */
int qsv_exec(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data);

/* ---- noisy shots: one trajectory per shot ------------------------------------------------ */

#define QSV_NOISY_MAX_QUBITS 13

/* Every shot s runs the program on its own copy of |0...0> (2^W amplitudes in the LDS of one workgroup; W = the
 * handle's n_qubits <= QSV_NOISY_MAX_QUBITS on a single-shard handle, whose own amplitude vector is not used),
 * drawing one Pauli per QSV_OP_PAULI record and one Kraus operator per QSV_OP_KRAUS record (below), then one basis
 * state from |amp|^2, and records it as qsv_sample does:
 * out_bits[s] bit j = the value of qubit meas_qubits[j] (-1: bit j stays 0; NULL: the full basis index), each
 * measured bit flipped with probability readout[2j + value] (NULL: no readout error).
 * Kinds: INIT_ZERO, INIT_UNIFORM, 1Q, MCX, DIAG, MCPHASE, PAULI, KRAUS, KRAUS2, MEASURE, IF, RESET; anything else returns
 * QSV_E_UNSUPPORTED.
 * A KRAUS record on qubit t: u = the next draw of stream 0 (PAULI and KRAUS records share one draw counter, which
 * advances at every such record, m = 1 included); r00 = sum |a_i0|^2, r11 = sum |a_i1|^2, r10 = sum a_i1 conj(a_i0) over
 * the pairs (a_i0, a_i1) of t, total = r00 + r11; w_k = E00_k r00 + E11_k r11 + 2 Re(E01_k r10); the first k with w_k > 0
 * whose inclusive cumulative sum of the positive w exceeds u total is taken (none: the last k with w_k > 0), and every
 * pair is multiplied by K_k sqrt(total / w_k).
 * A KRAUS2 record on the qubits (t0, t1) is the same rule one size up.  u = the next draw of stream 0: the draw counter is the
 * one PAULI and KRAUS records advance, and it advances at every KRAUS2 record too, m = 1 included.  A quad is the four
 * amplitudes (a_i0, a_i1, a_i2, a_i3) that differ only in the bits t0 and t1, a_ix having bit t0 = x & 1 and bit t1 = x >> 1;
 * r[x][y] = sum_i a_ix conj(a_iy) over all quads, total = ((r[0][0] + r[1][1]) + r[2][2]) + r[3][3].  With the packed entries
 * e[0..16) of E_k and the 16 real numbers of r in the same packing -- rr[0..4) = r[x][x], then (Re r[x][y], Im r[x][y]) for
 * (x, y) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) --, w_k = tr(E_k r) = d + 2 f, d = e[0] rr[0] + ... + e[3] rr[3] and
 * f = e[4] rr[4] + ... + e[15] rr[15], each sum taken in ascending index (Re(E[x][y] r[y][x]) = Re E Re r + Im E Im r).  The
 * first k with w_k > 0 whose inclusive cumulative sum of the positive w exceeds u total is taken (none: the last k with
 * w_k > 0), and every quad is multiplied by K_k and by sqrt(total / w_k).  A state without mass stays as it is.
 * QSV_E_BADARG, with a message that names the op: n != 2, equal qubits, a qubit at or above the width, m outside 1..16, an
 * entry that is not finite, E tables whose sum is not the identity to 1e-9.
 * A MEASURE record on qubit t with classical bit c: the channel K_0 = |0><0|, K_1 = |1><1| (release: |0><1|) plus one recorded
 * bit.  u = the draw (seed, shot, stream 3, d), d = the ordinal of the record among the MEASURE records of the program; the
 * draw counter of stream 0 does NOT advance, so a shot meets the same Pauli and Kraus draws whether its measurements are
 * deferred or taken in place.  r00, r11 and total as for KRAUS.  The outcome b = 0 if r00 > 0 and r00 > u total, otherwise
 * b = 1 if r11 > 0, else b = 0 (the KRAUS rule with w_0 = r00, w_1 = r11); a state without mass stays as it is, with b = 0.
 * The other half of every pair is set to zero and the kept half multiplied by sqrt(total / w_b); with release = 1 and
 * b = 1 the kept half moves to the 0 half, so that the qubit is back in |0>.  Bit c of the shot's word is cleared, then
 * set to b, flipped iff the draw (seed, shot, stream 2, c) -- the draw the final readout takes for bit c, so the readout draw
 * of a bit does not depend on when it was measured -- is below flip[b].  A later MEASURE record may write the same bit
 * again.  The final word is the word of the final draw ORed with these bits.  QSV_E_BADARG, with a message that names the
 * op: meas_qubits == NULL (full-index words) together with a MEASURE record, c >= n_meas, meas_qubits[c] >= 0 for a bit a
 * MEASURE record writes, a flip outside [0, 1], a release flag other than 0 or 1.
 * An IF record with span, mask, value and negate: when the record is reached, hit = ((word & mask) == value) != negate, where
 * word holds the bits that MEASURE records have written so far in this shot, as read (readout flip included: what a classical
 * register of the device would hold); bits not yet written read 0, the bits of the final draw included.  If !hit, the next
 * span records do nothing and take no draw: the draw counter of stream 0 does not advance, a skipped MEASURE record writes no
 * bit, and the stream-3 ordinals of MEASURE and RESET records are positions in the program, which a skip cannot shift.  So a
 * shot's draws behind the span depend on whether the span ran -- as they do on a device, where an error of a gate occurs only
 * when the gate does.  QSV_E_BADARG, with a message that names the op: span < 1 or reaching past the last record, mask == 0,
 * a value bit outside mask, a mask bit at or above n_meas, meas_qubits == NULL, negate other than 0 or 1, an IF or an INIT
 * record inside a span (guards do not nest).  All of it is checked before the first launch.
 * A RESET record on qubit t is the MEASURE contract with release = 1, except that no classical bit is written and no readout
 * draw is taken: u = the draw (seed, shot, stream 3, d), d = the ordinal of the record among the MEASURE AND RESET records of
 * the program (for every program without a RESET record that is the ordinal of MEASURE as it was); outcome, projection,
 * rescaling and the move of the 1 half to the 0 half as there.  QSV_E_BADARG: n != 1, t at or above the width.
 * Programs with an IF or a RESET record run kernels of their own (qsv_noise_dynamic.hip); with the diagnostic option
 * noisy_dynamic_kernels every program does, and no word depends on that.
 * Random numbers are Philox-4x32-10 draws keyed by the seed and counted by (shot, stream, draw): shot s of a call
 * is the same whatever the number of shots or the grid.  Runs on the handle's stream (qsv_timer_* bracket it).
 * Replaces: simulator.run(T, shots=SHOTS, noise_model=...) of an Aer noise model of Pauli, one- and two-qubit Kraus errors. */
int qsv_noisy_sample(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                     uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                     const double* readout /* n_meas x 2: P(flip | 0), P(flip | 1); NULL = none */,
                     uint64_t* out_bits);

#define QSV_NOISY_HBM_MAX_QUBITS 24

/* qsv_noisy_sample for up to QSV_NOISY_HBM_MAX_QUBITS qubits: the same arguments, checks, record kinds, draws and words, with
 * every trajectory's 2^W amplitudes in a slot of 16 x 2^W bytes of device memory instead of LDS.  A persistent workgroup
 * owns one slot and runs shots b, b + grid, ... in it; grid = min(shots, the noisy_grid option if set, the workgroups the
 * chip holds at once, the slots that fit into 90 % of the free device memory).  The slots are one allocation per call,
 * freed before the call returns; if not even one fits, QSV_E_NOMEM names the bytes needed and the bytes free
 * (qsv_device_memory).  Widths up to QSV_NOISY_MAX_QUBITS are accepted too (the two paths can be compared on them):
 * a shot's Pauli, Kraus and readout draws are those of qsv_noisy_sample; sums of |amp|^2 are added in another order, so
 * a draw within rounding distance of a boundary may fall on its other side.  Opt-in: qsv_noisy_sample is unchanged. */
int qsv_noisy_sample_hbm(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                         uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                         const double* readout /* n_meas x 2: P(flip | 0), P(flip | 1); NULL = none */,
                         uint64_t* out_bits);

/* Noisy shots kept only when fixed bits of their word read given values: rejection sampling, reproducible because a shot is a
 * pure function of (program, seed, shot index).  The arguments up to `readout` are those of qsv_noisy_sample, with its checks;
 * hbm = 0 keeps the states in LDS (width limit QSV_NOISY_MAX_QUBITS), hbm = 1 in slots of device memory
 * (QSV_NOISY_HBM_MAX_QUBITS).  Attempt t = first_shot, first_shot + 1, ... is shot t of qsv_noisy_sample (hbm = 1:
 * qsv_noisy_sample_hbm) with the same arguments: the same draws and, where the shot is run to its end, the same word.  Attempt
 * t is accepted iff (word & fix_mask) == fix_val, over the bits of the recorded word.  The call returns the first `shots`
 * accepted attempts in ascending t: their words in out_bits[0, *accepted), their indices t in out_shot (NULL: not wanted).
 * *accepted = how many were found; *attempts = the number of indices examined: the last accepted index - first_shot + 1
 * when *accepted == shots, max_attempts otherwise.  Running out of attempts is QSV_OK with *accepted < shots: the caller
 * decides what that means.
 * A trajectory is abandoned as soon as it can no longer be accepted: behind the last MEASURE record that writes a fixed bit
 * (a bit may be written twice; only its last write may end a shot), if the bit it left in the word -- after the readout flip:
 * acceptance is on what was read -- differs from fix_val, the remaining records and the final draw of that shot are skipped.
 * Attempts that fail only on bits the final draw writes run to their end and are filtered.  The word of an abandoned shot is
 * never returned.  The decisive record is the last one in program order that writes the fixed bit, wherever it stands: the
 * check sits behind an EXECUTED record, so where the span of an IF record skips that last writer nothing is abandoned, the
 * shot runs to its end, and the predicate above, which the host applies to every word, decides.
 * `round` = attempts per launch, 0 = chosen by the library (about `shots` at first, later rounds from the acceptance seen so
 * far, at most 2^20).  Nothing the call returns depends on `round`, on the noisy_grid option or on whether a rejected
 * trajectory was abandoned.  With fix_mask = 0 and first_shot = 0, out_bits is the output of qsv_noisy_sample(_hbm) word for
 * word and *attempts = shots.  The op stream, its tables and the measurement map are encoded and copied to the device once
 * per call, the slots of hbm = 1 allocated once per call (as qsv_noisy_sample_hbm sizes them for max(64, 4 shots) shots) and
 * freed before it returns; the loop over the rounds is inside the call.
 * QSV_E_BADARG, with a message that names the bit: a bit of fix_val outside fix_mask; a bit of fix_mask at or above n_meas
 * (meas_qubits == NULL: at or above the width); a bit of fix_mask that neither the final draw (meas_qubits[bit] >= 0) nor a
 * MEASURE record writes.  Also QSV_E_BADARG: max_attempts = 0 with shots > 0; accepted or attempts NULL. */
int qsv_noisy_sample_accept(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                            uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                            const double* readout /* n_meas x 2: P(flip | 0), P(flip | 1); NULL = none */,
                            uint64_t fix_mask, uint64_t fix_val, uint64_t first_shot, uint64_t max_attempts,
                            uint64_t round, int hbm, uint64_t* out_bits /* shots */, uint64_t* out_shot /* shots, or NULL */,
                            uint64_t* accepted, uint64_t* attempts);

/* ---- density matrix: exact noisy distributions ------------------------------------------- */

#define QSV_DENSITY_MAX_QUBITS 17

/* A density matrix of W qubits is the amplitude vector of a single-shard handle of n_qubits = 2W (W <=
 * QSV_DENSITY_MAX_QUBITS: 16 x 4^W bytes): amplitude v = i | (j << W) holds rho[i, j], ket bits low, bra bits high.
 *
 * qsv_density_exec runs the record stream of qsv_noisy_sample from |0..0><0..0|, exactly: a unitary record U as
 * U rho U^dg (the record on the ket bits and its mirror on the bra bits -- qubits + W, matrix and table conjugated, angle
 * negated -- through the sweeps of qsv_exec), QSV_OP_PAULI as sum_p P(p) P rho P^dg with P(p) the differences of the
 * record's cumulative table, QSV_OP_KRAUS and QSV_OP_KRAUS2 as sum_k K_k rho K_k^dg (their E tables are not read; the
 * 16 x 16 superoperator of a KRAUS2 record is built once per record on the host and read from device memory).
 * Kinds: INIT_ZERO, INIT_UNIFORM, 1Q, MCX, DIAG, MCPHASE, PAULI (n = 1, 2), KRAUS (n = 1, 1..4 operators), KRAUS2 (n = 2, 1..16
 * operators); MUX, KQ, SWAP, MEASURE, IF, RESET and
 * handles of several shards or ranks return QSV_E_UNSUPPORTED; an odd n_qubits or a record qubit >= W QSV_E_BADARG.  Every
 * record is checked before the first one runs.
 * Replaces: simulator.run(T, noise_model=..., method="density_matrix") of Qiskit Aer. */
int qsv_density_exec(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data);

/* qsv_density_exec with the measurements taken in place where their outcome is fixed by the caller: the same stream, body and
 * checks, and in addition QSV_OP_MEASURE records as qsv_noisy_sample documents them (qubits[0] = t < W, vals[0] = the classical
 * bit c < 64, vals[1] = release, data_off -> f0, f1 = P(flip | 0), P(flip | 1)).  A density matrix cannot follow a measured
 * bit without branching, but "bit c read v, qubit handed on" is ONE linear, trace-decreasing map: for every 2 x 2 block B over
 * (ket bit t, bra bit t + W)
 *     release = 0:  B' = [[w0 B00, 0], [0, w1 B11]]        release = 1:  B' = [[w0 B00 + w1 B11, 0], [0, 0]]  (t back in |0>)
 * with w_b = P(read v | true b) -- 1 - f_b if b == v, f_b otherwise: acceptance is on the bit as read, as in
 * qsv_noisy_sample_accept -- when c is in fix_mask and v = bit c of fix_val, and w0 = w1 = 1 when c is not in fix_mask (the
 * outcome is forgotten: the dephasing channel, with release the reset channel; the trace stays).  Of a fixed bit that several
 * MEASURE records write only the LAST write conditions, the earlier ones are forgotten (the rule of
 * qsv_noisy_sample_accept).  The trace is NOT renormalised: after the call it is the probability that every conditioning
 * record read its value.  A fix_mask bit that no MEASURE record writes is allowed and does nothing: the caller conditions
 * it on the diagonal.  A MEASURE record closes the run of mirrored unitary records, as PAULI and KRAUS do, and is one kernel:
 * from qubit 3 up its own (2 loads and 4 stores per block: 24 bytes per amplitude), below that the KRAUS kernel with the
 * superoperator of sqrt(w0) |0><0| and sqrt(w1) |1><1| (release: |0><1|) -- option density_measure_kernel.
 * QSV_E_BADARG, with a message that names the op or the bit: t >= W, c >= 64, release not 0 or 1, a flip outside [0, 1] or
 * not finite, the data range outside the pool, a bit of fix_val outside fix_mask.  Every record is checked before the first
 * one runs.  With fix_mask = 0 and no MEASURE record the vector is bit for bit that of qsv_density_exec.
 * QSV_OP_IF is refused (QSV_E_UNSUPPORTED: it would need branching), and so is QSV_OP_RESET as a kind: a reset comes as the
 * MEASURE record above with release = 1 and a classical bit outside fix_mask, which is the reset channel exactly. */
int qsv_density_exec_accept(qsv_handle* h, const qsv_op* ops, int n_ops, const double* data, uint64_t n_data,
                            uint64_t fix_mask, uint64_t fix_val);

/* the 4^n real coefficients a PAULI record (n = 1, 2) comes to on a density matrix (host only, no device needed):
 * out[x * 2^n + d] = sum_z P(x, z) (-1)^(z . d), with x, z the x and z bits of the Pauli index (QSV_OP_PAULI) and P the
 * differences of `cum`; then rho'[v] = sum_x out[x][d(v)] rho[v ^ m_x], m_x = the x bits on both sides, d(v) = (i xor j)
 * on the error qubits. */
int qsv_density_pauli_table(int n, const double* cum, double* out);

/* out[j] = sum Re rho[i, i] over the i whose bits qubits[b] spell j (k <= W, 2^k doubles, not clipped); *trace = the sum
 * over all i (trace may be NULL).  One strided read of 2^W elements, summed in ascending i: the same bits every time. */
int qsv_density_diagonal(qsv_handle* h, const int* qubits, int k, double* out, double* trace);

/* `shots` basis states of the W qubits from P_i = max(Re rho[i, i], 0), recorded as qsv_noisy_sample records them
 * (meas_qubits, n_meas, readout, out_bits as there).  u = the Philox draw (seed, shot, stream 1, draw 0); the state is the
 * first i whose inclusive cumulative sum (ascending i) exceeds u sum P, none: the last i with P_i > 0; each measured bit j
 * is flipped when the draw (seed, shot, stream 2, draw j) is below readout[2j + value].  A shot depends on (seed, shot)
 * alone. */
int qsv_density_sample(qsv_handle* h, uint64_t shots, uint64_t seed, const int* meas_qubits, int n_meas,
                       const double* readout /* n_meas x 2; NULL = none */, uint64_t* out_bits);

/* ---- instrumentation ---------------------------------------------------------------- */

/* on: bracket every kernel launch with HIP events on its own stream (costs a little) */
int qsv_set_profiling(qsv_handle* h, int on);
int qsv_reset_stats(qsv_handle* h);
int qsv_get_stats(qsv_handle* h, qsv_stats* out);

/* Deferred state (option defer_state).  A program whose last pass is the generator and leaves tile sums may store no
 * amplitude at all: only the sums kernel runs (it forms the sums from the factors' |.|^2 and touches no amplitude; the
 * same kernel follows the writing generator when the state is not deferred, so the sums do not depend on the option),
 * the shard keeps the generator's recipe, qsv_sample stores the tiles its shots fall into, qsv_norm
 * answers from the sums, and every other entry that reads or changes the state first has the generator write it
 * ("realises" it; booked under QSV_K_INIT_PROD with the bytes stored).  Entries that realise: qsv_get_amplitudes,
 * qsv_set_amplitudes, qsv_copy_state (source), qsv_probabilities*, qsv_expect_diag, qsv_apply_*, qsv_swap_layout (and
 * its exchanges), qsv_ipc_export, qsv_density_*, a qsv_exec that does not start with an init, and qsv_norm / qsv_sample
 * when they cannot use the tile sums (cache_sums or fused_sums 0), qsv_sample_cond / qsv_marginals_cond / qsv_top_cond when no block
 * bit of the tile index is fixed (or by option post_select_list; qsv_marginals_cond_rows: by its rows' common condition).  Entries that do not: qsv_sample on the tile path,
 * qsv_sample_cond / qsv_marginals_cond / qsv_top_cond when they list the tiles that hold the sub-cube,
 * qsv_norm from the cached sums, qsv_tile_sums, qsv_noisy_sample* (they keep their own states), stats, timers, options, qsv_sync.
 * Deferred state ends with realisation or with the next init that writes; a program refused before its init writes
 * leaves the deferred state, recipe included, as it was.
 * deferred: 1 if a shard of this process is deferred; realize_calls / listed_launches: generator launches so far that
 * realised a shard / that stored a sampler's tile list or (sample_chain 1) located its shots in it.  Any out pointer may be NULL. */
int qsv_state_info(qsv_handle* h, int* deferred, uint64_t* realize_calls, uint64_t* listed_launches);

/* The per-tile sums of |amp|^2 the last pass of the last program left on local shard `shard` (fused_sums), in
 * tile-index order: *n = their number; out (may be NULL: *n only) receives them when cap >= *n.  Read only: a deferred
 * state stays deferred.  QSV_E_BADARG when that shard holds no valid tile sums (the state changed since, or its last
 * pass left none). */
int qsv_tile_sums(qsv_handle* h, int shard, double* out, uint64_t cap, uint64_t* n);

/* How the generator formed the tile sums local shard `shard` holds (option sums_factored).  A factor that touches block
 * bits only is tile-uniform: one weight for a whole tile.  The other factors (inner) read the tile index through the
 * block bits they touch, the set D.  Factored, the 256-thread sums ran over the 2^|D| tiles that differ in D, and every
 * tile's sum is that sum times its tile-uniform weights.  *factored: 1 if the last sums launch ran that way; *d_bits:
 * |D|; *inner_factors, *uniform_factors: the split of the factor list (reported whichever path ran).  Read only; any
 * out pointer may be NULL.  QSV_E_BADARG when the shard's tile sums are not valid or were not left by the generator. */
int qsv_tile_sums_info(qsv_handle* h, int shard, int* factored, int* d_bits, int* inner_factors, int* uniform_factors);

/* HIP-event stopwatch on shard 0's stream: begin records, end records+synchronises */
int qsv_timer_begin(qsv_handle* h);
int qsv_timer_end(qsv_handle* h, double* ms);

/* Tuning knobs (defaults in brackets; none of them changes a result, only how it is computed).  Unknown
 * name or value out of range: QSV_E_BADARG.
 *   passes      multi_r [5]        register targets of a k_multi pass at most (0: one kernel per gate)
 *               general_r [4]      ... of a GENERAL pass (masked X / 2x2 / phase, register selects); its tile width
 *               general_light_r [5] tile width a general pass with little arithmetic is padded to
 *               pass_max_ops [56]  ops per pass at most        pass_budget [0]   arithmetic cap of a general pass, % of one sweep
 *               lane_targets [1]   targets < 6 ride on lane bits (wave shuffles)   dyn_lanes [3]  lane bits 3..5 lent per pass
 *               lane_map [1]       lane bit 5 on address bit 11 when the tile allows (2: only a tile on bits 6..10; 0: never)    pass_hints [1]  honour QSV_OPF_NEW_PASS
 *               xframe [1]         uncontrolled X = XOR on store addresses / pending across passes (never a data move)
 *               single_shortcut [1] a one-op pass runs as its dedicated kernel     trace_passes [0]  one stderr line per pass
 *               general_combos [1] general pass: controls on workgroup-uniform bits resolved per workgroup on the host (combo table)
 *               fold_init_h [1]    H on a still-|0> qubit right after an init is part of the init write.  The one knob that can
 *                                  decide WHETHER a program runs: folded, an H on a shard-bit qubit needs no data movement; with 0
 *                                  the same record is a dense gate on a shard bit and qsv_exec returns QSV_E_UNSUPPORTED (swap the
 *                                  qubit to a local position first).  Where both run, the results agree.
 *   generator   init_prod [1]      init x diagonal factors in one write-only pass   init_prod_r [0 = by shard size], init_prod_bit0 [0 = by size]
 *                                  init_prod_grid [0 = every workgroup the chip holds at once; else at most this many]
 *                                  init_prod_group [-1 = up to 3 group bits; 0 = one tile per group; 1..4 = that many]
 *                                  defer_state [-1]  the generator as a program's last pass, leaving tile sums, stores nothing (qsv_state_info):
 *                                  -1 from 30 local qubits, 0 never, 1 always
 *                                  sums_factored [-1]  the generator's tile sums from the 2^|D| tiles its inner factors tell apart,
 *                                  times the tile-uniform factors' weights (qsv_tile_sums_info): -1 where that removes at least 3
 *                                  tile-index bits, 1 at least one, 0 never (the sums differ by rounding only, within the same bound)
 *   memory      nontemporal [-1], multi_nt [-1], init_prod_nt [-1]   non-temporal loads/stores: -1 by shard size, 0 never, 1 always
 *   measurement cache_sums [1], fused_sums [1]   keep / produce per-tile |amp|^2 sums in the last pass of a program
 *               sample_chain [1]   qsv_sample on one shard's tile sums: 1 the walk over the super sums on the device, a deferred shard's
 *                                  shots located inside the generator (nothing stored), one host wait; 0 the host walk.  Same words.
 *               post_select_list [-1]  qsv_sample_cond on a deferred shard: -1 the tiles holding the matching amplitudes are listed and
 *                                  stored when they are at most 1/16 of the tiles and the list fits a quarter of the arena, else the
 *                                  state is realised; 0 always realised; 1 listed whenever a block bit is fixed and the list fits.  Same words.
 *               marginals_grid [0] diagnostic: qsv_marginals_cond takes at most this many workgroups, 0 = as many as the chip holds;
 *                                  which workgroup walks a chunk changes, no bit of the result does
 *               marginals_rows [0] diagnostic: qsv_marginals_cond_rows takes at most this many rows per slab, 0 = as many as the arena and
 *                                  the reduction scratch hold; the launches per shard change, no bit of the result does.  Refused below 0.
 *                                  marginals_grid caps the workgroups of the batched kernel too
 *               top_grid [0]       diagnostic: qsv_top_cond takes at most this many workgroups, 0 = as many as the chip holds;
 *                                  which workgroup walks a block changes, no bit of the result does
 *   kernels     unroll [4], lowt_shuffle [1], pair_variant [0], kq_mfma [1], blocks_per_cu [65536]
 *               swizzle [1]        one-gate kernels: lane bit 5 of a wave access carries address bit 11 (two 512-byte runs 32 KiB apart);
 *                                  1 from 2^26 amplitudes per shard, 2 from 2^14, 0 never        lane_map_min_l [26]  same for k_multi tiles other than bits 6..10
 *               kq_grid [0]        diagnostic: the matrix-core dense-gate launches (qsv_apply_kq, QSV_OP_KQ with k >= 3) take at most this
 *                                  many workgroups, 0 = no cap; which wave computes a batch changes, no amplitude does
 *   noisy       noisy_grid [0]     workgroups of qsv_noisy_sample, qsv_noisy_sample_hbm and each round of qsv_noisy_sample_accept: 0 = as many as the
 *                                  chip holds at once, else at most this many
 *               noisy_dynamic_kernels [0]  diagnostic: 1 sends every per-shot stream through the kernels of qsv_noise_dynamic.hip, which
 *                                  streams with an IF or a RESET record run anyway; no word depends on it
 *   density     density_measure_kernel [-1]  a MEASURE record of qsv_density_exec_accept: -1 its own kernel (24 bytes per amplitude) from
 *                                  qubit 3 up, below that -- where the entries it skips share the lines of those it loads -- the same map as
 *                                  a two-operator superoperator through the KRAUS kernel (32); 0 always the latter; 1 always its own.
 *                                  The same map either way.
 *   other      zero_tracking [0]  skip amplitudes known to be zero (opt-in)       exchange_chunk_log2 [24]  amplitudes per exchange chunk
 *               implied_zeros [1]  the generator as a program's last pass (and qsv_exec's end) leaves the provably-zero part
 *                                  of a shard unwritten; every reader honours that or writes the zeros first (0: write them always) */
int qsv_set_option(qsv_handle* h, const char* name, int value);

const char* qsv_last_error(void);
const char* qsv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QSV_H */
