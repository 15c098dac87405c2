/*
 * libqsv -- MI355X (gfx950) statevector + Pauli-expectation backend for the QUEASARS circuit-evaluation path.
 *
 * C ABI.  Plain pointers and sizes only; no Python, torch or C++ types cross this boundary.
 *
 * The reference (DLR-RB/QUEASARS, pure Python) has no FFI for this path: its boundary is the Python protocol
 *     BaseCircuitEvaluator.evaluate_circuits(circuits, parameter_values) -> list[float]   and   .n_qubits
 *     (reference: queasars/circuit_evaluation/circuit_evaluation.py:62-87)
 * whose implementations hand (circuit, operator, parameter values) "pubs" to a Qiskit primitive
 *     OperatorCircuitEvaluator.evaluate_circuits        (circuit_evaluation.py:200-215, estimator branch)
 *     OperatorSamplerCircuitEvaluator.evaluate_circuits (circuit_evaluation.py:147-157, sampler branch)
 *     measure_quasi_distributions                       (circuit_evaluation.py:29-59)
 * Each entry point below says which of those calls it replaces.  INTEGRATION.md shows the ctypes stub a
 * QUEASARS maintainer would add.
 *
 * Conventions
 *   - little endian qubits: qubit q is bit q of a basis-state index (reference: queasars/utility/pauli_strings.py:38-40)
 *   - a Pauli term is (x_mask, z_mask, coeff): factor on qubit q is I/X/Z/Y for (x,z) bit pair 00/10/01/11
 *   - gates: id, u(theta,phi,lam) and cu3(theta,phi,lam) with Qiskit's matrix definitions
 *     (reference: queasars/minimum_eigensolvers/evqe/quantum_circuit/quantum_gate.py:78-79, :96-102, :157-165)
 *   - every function returns 0 on success, a negative QSV_E_* code otherwise; qsv_last_error() gives text
 *   - the caller owns every host array it passes in or receives results in; the library owns all device memory
 *   - a handle may be used from several host threads; calls on one handle are serialised internally
 *   - between qsv_eval_begin and qsv_eval_end the calling thread holds the handle (other threads' calls wait for the end).  From
 *     that thread, every call that takes the handle returns QSV_E_STATE -- "a batch is open on this handle (<function> goes
 *     between batches)" -- and does nothing.  The exceptions are the calls that belong inside a batch: qsv_eval_push,
 *     qsv_eval_push_device, qsv_eval_staging, qsv_eval_set_output, qsv_eval_suggested_pushes and qsv_eval_end; and those that
 *     take no lock: qsv_destroy, qsv_last_error, qsv_n_qubits, qsv_group_size and the functions without a handle.  (A second
 *     qsv_eval_begin is refused in its own words.)
 */
#ifndef QSV_H
#define QSV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qsv_handle qsv_t;

enum { QSV_OP_ID = 0, QSV_OP_U = 1, QSV_OP_CU3 = 2 };
enum { QSV_F64 = 0, QSV_F32 = 1 };
enum { QSV_NO_CONTROL = 0xFF };

enum {
    QSV_OK = 0,
    QSV_E_ARG = -1,      /* bad argument */
    QSV_E_DEVICE = -2,   /* HIP runtime error (no device, out of memory, launch failure) */
    QSV_E_STATE = -3,    /* call order (e.g. expectation requested before an operator was set) */
    QSV_E_UNSUPPORTED = -4
};

/* One decomposed circuit instruction.  An angle is params[p_x] when p_x >= 0, else the literal. 40 bytes. */
typedef struct qsv_op {
    uint8_t kind;    /* QSV_OP_* */
    uint8_t target;  /* qubit the 2x2 matrix acts on */
    uint8_t control; /* control qubit for cu3, QSV_NO_CONTROL otherwise */
    uint8_t flags;   /* reserved, 0 */
    int32_t p_theta, p_phi, p_lambda;
    double theta, phi, lambda;
} qsv_op;

/* Tuning knobs of the pass scheduler (0 = library default). */
typedef struct qsv_plan_config {
    int32_t tile_bits; /* k: qubits resident on chip per pass (per workgroup tile of 2^k amplitudes) */
    int32_t reg_bits;  /* r: qubits held in each thread's registers at a time (2^r amplitudes per thread) */
    int32_t low_bits;  /* c: lowest qubits always kept in the tile so global accesses stay coalesced */
    int32_t group;     /* circuits evaluated per launch group (0 = size the group to the Infinity Cache) */
    int32_t exchange;  /* LDS transpose: 1 whole complex element per access, 2 re/im planes both resident,
                          3 re then im through one plane buffer (half the LDS); fp32 always uses 1 */
} qsv_plan_config;

/* Counters of the most recent qsv_eval_* call (timings need qsv_set_profiling(h, 1)). */
typedef struct qsv_profile {
    uint64_t n_evals;          /* circuit evaluations in the call */
    uint64_t n_pass_launches;  /* launches of the gate-pass kernel */
    uint64_t n_state_passes;   /* sum over launches of states swept (launch x circuits in its group) */
    uint64_t n_gates;          /* non-identity gates applied */
    uint64_t state_bytes;      /* algorithmic state bytes of the gate-pass launches: 16 * 2^n per state and direction a
                                  fused pass design has to move (pass 0 only writes, a fused last pass only reads) */
    double pass_ms;            /* device time of the gate-pass launches, summed over pushes (HIP events on the stream
                                  each push runs on; pushes on the two streams overlap, so this can exceed wall time) */
    double expect_ms;          /* device time of expectation / reduction kernels */
    double total_ms;           /* device time of the whole call, first launch to last */
    double pass_window_ms;     /* wall-clock window from the first gate-pass launch to the end of the last one */
    uint64_t moved_bytes;      /* state bytes the launches really moved: less than state_bytes when a compact first pass
                                  replaced the state round trip between the first two passes by a small table */
    /* The kernels of the hot path; with profiling on, every launch is bracketed by HIP events on the stream it runs
       on.  [0] = the synthesising first pass of the gate-pass kernel (writes only; also the one-tile virtual circuits
       of split evaluations), [1] = every later pass (the last one fuses the diagonal expectation and then only
       reads), [2] = the contraction kernel of split evaluations (reads the diagonal table once, forms the amplitudes
       from two small tables).  bytes = algorithmic state bytes at the pass's own price (16 * 2^n per state and
       direction it has to move; for [2] what the contraction reads per state: the diagonal table, 8 * 2^n, and the two
       side tables), moved = what a launch really moves (compact tables instead of states; = bytes for [2]), flops = 24
       per amplitude pair a pass updates (4 multiplications + 10 fused multiply-adds), for [2] 8 J + 5 per amplitude
       (J product terms). */
    uint64_t kernel_launches[3];
    double kernel_ms[3];
    uint64_t kernel_bytes[3];
    uint64_t kernel_moved_bytes[3];
    double kernel_flops[3];
    uint64_t kernel_states[3]; /* states swept, summed over launches */
} qsv_profile;

/* ---- lifetime ---------------------------------------------------------------------------------- */

/* Create an evaluator for n_qubits on HIP device `device`.  Replaces constructing a Qiskit primitive. */
int qsv_create(int n_qubits, int dtype, int device, const qsv_plan_config* cfg /* may be NULL */, qsv_t** out);
void qsv_destroy(qsv_t* h);
/* Text of the last error on this handle (or of the last failed qsv_create when h is NULL). */
const char* qsv_last_error(const qsv_t* h);
/* Launch on an existing HIP stream (hipStream_t passed as void*); NULL = the library's own stream. */
int qsv_set_stream(qsv_t* h, void* hip_stream);
int qsv_n_qubits(const qsv_t* h);

/* ---- operator ---------------------------------------------------------------------------------- */

/*
 * Set the observable H = sum_k (coeff_re[k] + i coeff_im[k]) P_k.
 * Replaces passing `operator` in each pub (circuit_evaluation.py:204-208).  An operator whose terms are all
 * I/Z takes the diagonal fast path (one table D[i] = sum_k c_k (-1)^popcount(i & z_k) built once on device).
 */
int qsv_set_operator(qsv_t* h, int n_terms, const uint64_t* x_mask, const uint64_t* z_mask,
                     const double* coeff_re, const double* coeff_im);

/* ---- circuits ---------------------------------------------------------------------------------- */

/* Register a circuit structure once; evaluations then send only parameter values. */
int qsv_circuit_create(qsv_t* h, int n_ops, const qsv_op* ops, int n_params, int* out_circuit_id);
/* The same for many structures at once (circuit i = ops[op_offsets[i] .. op_offsets[i+1]), n_params[i] parameters):
 * the pass scheduler runs on several host threads.  What a generation of EVQE needs after topological search or layer
 * removal, when a whole population of new structures arrives together (reference: one fresh QuantumCircuit per
 * individual, queasars/minimum_eigensolvers/evqe/evolutionary_algorithm/selection.py:75-82). */
int qsv_circuits_create(qsv_t* h, int n_circuits, const int64_t* op_offsets, const qsv_op* ops, const int* n_params,
                        int* out_circuit_ids);
int qsv_circuit_destroy(qsv_t* h, int circuit_id);

/*
 * KEPT STATES.  A layer search evaluates one circuit over and over with only one layer's angles changing
 * (reference: optimize_layer_of_individual binds every other layer, mutation.py:57-59,
 * individual.py:288-322 get_partially_parameterized_quantum_circuit): everything in front of that layer is the same state
 * in every evaluation.  qsv_prefix_create runs n_states (circuit, parameter vector) pairs from |0..0> ONCE and keeps their
 * final states resident (2^n amplitudes each); a circuit registered with qsv_circuit(s)_create_on_prefix(es) starts from
 * such a state instead of |0..0> and is evaluated by every qsv_eval_* entry point like any other circuit id (qsv_statevector
 * too; the sampling entry points refuse it).  Unsplittable (deep) individuals then cost the passes of the layers from the
 * searched one on, not of the whole circuit.  A kept state lives until qsv_prefix_destroy AND the last circuit registered on
 * it is destroyed; its memory is reused afterwards.
 */
int qsv_prefix_create(qsv_t* h, int n_states, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                      int* out_prefix_ids);
int qsv_prefix_destroy(qsv_t* h, int n_states, const int* prefix_ids);
/* Kept states alive on the handle (held by the caller or by a circuit). */
int qsv_prefix_count(const qsv_t* h);
int qsv_circuit_create_on_prefix(qsv_t* h, int prefix_id, int n_ops, const qsv_op* ops, int n_params, int* out_circuit_id);
int qsv_circuits_create_on_prefixes(qsv_t* h, int n_circuits, const int64_t* op_offsets, const qsv_op* ops, const int* n_params,
                                    const int* prefix_ids, int* out_circuit_ids);

/*
 * Which way an expectation value of a registered circuit goes under the operator set now, and about what it costs: what a
 * scheduler needs to deal individuals of unequal depth to several GPUs (the reference balances dynamically, one future per
 * individual on a pool: selection.py:75-82, mutation.py:206-216), and what decides whether a layer search is worth a kept
 * state.  microseconds: GPU time per evaluation inside a full launch, from the measured figures of DESIGN.md (an estimate:
 * only ratios matter to its users).
 */
enum { QSV_ROUTE_ONE_TILE = 0, QSV_ROUTE_SPLIT_ONE_LAUNCH = 1, QSV_ROUTE_SPLIT = 2, QSV_ROUTE_PASSES = 3 };
typedef struct qsv_circuit_cost_t {
    int32_t route;         /* QSV_ROUTE_* */
    int32_t n_keys;        /* split routes: cut keys (2^keys product terms) */
    int32_t n_passes;      /* gate passes (split routes: of the longer virtual circuit) */
    int32_t on_kept_state; /* the circuit continues a kept state */
    double microseconds;
} qsv_circuit_cost_t;
int qsv_circuit_cost(qsv_t* h, int circuit_id, qsv_circuit_cost_t* out);

/*
 * How a registered circuit is planned, read back as it is (tests and coverage claims: which form of split evaluation a
 * circuit took).  Computes nothing: route and n_keys are qsv_circuit_cost's; the rest is the circuit's split form, all
 * zero when it has none.  Side x is the side the split block calls X (its states are the outer index of the split
 * sampler's draw: index = deposit(x, mask_x) | deposit(y, mask_y)).
 */
typedef struct qsv_circuit_form_t {
    int32_t route;           /* QSV_ROUTE_*, as qsv_circuit_cost */
    int32_t n_keys;          /* as qsv_circuit_cost */
    int32_t n_virtual[2];    /* virtual qubits of side x, side y (0 if not split) */
    int32_t amps_per_thread; /* of the side plans: 8 (the sides_r3 form) or the handle's own 16 */
    int32_t halves;          /* three-key thirteen-qubit sides on two workgroups each (kEvalHalves) */
    int32_t outer[2];        /* log2 of the tiles a side sweeps: qubits of side x, side y outside its tile */
    int32_t one_launch;      /* the split form may take the one-launch route (both sides one pass, kEvalFused) */
    int32_t split_sampled;   /* qsv_sample_* draw it from its two side tables */
    uint32_t mask_x, mask_y; /* qubits of side x, side y (without the keys) */
} qsv_circuit_form_t;
int qsv_circuit_form(qsv_t* h, int circuit_id, qsv_circuit_form_t* out);
/*
 * The same, but n_virtual, halves and outer describe the side plans the one-launch route RUNS for the circuit under the
 * operator and options set now: those of its reduced form (option "final_controls") where it has one and that route takes it,
 * else qsv_circuit_form's.  mask_x, mask_y and everything else as qsv_circuit_form: every other consumer of the side states
 * runs the full form.
 */
int qsv_circuit_launch_form(qsv_t* h, int circuit_id, qsv_circuit_form_t* out);

/*
 * Expectation values real(<psi_i|H|psi_i>) of n_evals (circuit, parameter vector) pairs, |psi_i> prepared from
 * |0..0>.  params holds the vectors back to back, vector i at params[param_offsets[i] .. param_offsets[i+1]).
 * Replaces `estimator.run(pubs, precision=0).result()` + `real(res.data.evs)` (circuit_evaluation.py:210-215).
 */
int qsv_eval_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                      const double* params, double* out_expectations);

/*
 * ONE evaluation, merged with the evaluations other host threads ask for at the same time: the first caller collects
 * the requests that arrive within `window_us` microseconds (0 = library default; it stops earlier once as many
 * callers as last time have arrived, or nobody new comes), runs them as one batch and every caller gets its value.
 * This is the native form of the reference's BatchingMutexPrimitiveJobRunner (a 0.1 s collection window in front of a
 * primitive that is not thread safe, queasars/circuit_evaluation/mutex_primitives.py:67-199) for its calling pattern:
 * population_size threads, one circuit per call (selection.py:75-82, mutation.py:63-75).
 */
int qsv_eval_coalesced(qsv_t* h, int circuit_id, const double* params, int n_params, double window_us,
                       double* out_expectation);

/*
 * Streaming form of qsv_eval_circuits, for callers whose parameter vectors become available (or are converted)
 * piecemeal: qsv_eval_begin lays the batch out, each qsv_eval_push ships the packed parameter values of evaluations
 * [first, first+count) and launches them asynchronously, qsv_eval_end waits and returns all results.  Pushes must be
 * in order and contiguous; a push of any size is accepted (at most qsv_group_size() of its evaluations run side by
 * side in one launch).  The handle is locked from begin to end; end must be called even after a failed push.
 */
int qsv_eval_begin(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_counts);
int qsv_eval_push(qsv_t* h, int first, int count, const double* values);
/* Where the library keeps the parameter values of evaluations [first, first + count) of the open batch until their kernels
 * have read them (pinned host memory, sum of their param_counts doubles, back to back): a caller that writes them THERE and
 * passes the same pointer to qsv_eval_push saves the library's copy (84 KB per population of the benchmark: 5 us of a 72 us
 * step).  Valid until that push; evaluations must still be pushed in order. */
int qsv_eval_staging(qsv_t* h, int first, int count, double** values);
/* qsv_eval_push for parameter values that ALREADY LIVE IN DEVICE MEMORY (this handle's GPU; an optimiser that runs on the
 * device, a torch tensor): `device_values` points at the first value of evaluation `first`, the values of the push packed
 * back to back by the counts given to qsv_eval_begin -- a row-major matrix of equal rows is such a packing when every
 * evaluation declares the row length as its count (a circuit takes the first n_params values of its row).  Nothing is copied
 * and nothing crosses PCIe: the kernels read the values where they are, so they must stay unchanged until qsv_eval_end has
 * returned (for a batch that does not wait, qsv_eval_set_output: until its work is complete).  `ready_event`: a hipEvent_t
 * after which the values are complete -- every stream of the handle waits for it --, or NULL when they already are (the
 * caller synchronised, or wrote them on the handle's stream, qsv_set_stream).  Pushes of both kinds may be mixed in a batch.
 * (An evaluation that declares more than 1024 values -- rows padded that far -- is prepared without the LDS copy of its vector:
 * the same result to the last bits, not bit for bit.) */
int qsv_eval_push_device(qsv_t* h, int first, int count, const double* device_values, void* ready_event);
int qsv_eval_end(qsv_t* h, double* out_expectations);
/*
 * Results into DEVICE memory (n_evals doubles, this handle's GPU), for a caller that feeds them to something on the
 * device -- the fitness all-gather of a population sharded over several GPUs (one process per GPU; the reference hands
 * every individual to a worker of its own, evolutionary_algorithm/selection.py:75-85).  Call between qsv_eval_begin and
 * the first push.  qsv_eval_end(h, NULL) then returns WITHOUT waiting: the results are complete once the work
 * enqueued so far on the handle's stream (qsv_set_stream) is, so whatever the caller enqueues on that stream next sees
 * them, and one synchronisation at the end of ITS chain replaces the library's.  With a non-NULL pointer qsv_eval_end
 * waits and also copies the results to the host.  The next call on the handle waits for an unfinished batch first.
 */
int qsv_eval_set_output(qsv_t* h, double* device_out);
/*
 * The caller has SEEN every result of the last batch that ended without waiting (qsv_eval_set_output into memory the host can
 * read -- a node's shared fitness table: a result is an evaluation's last store): nothing of that batch is still running,
 * and the next call on the handle need not wait for the streams before it reuses the staging buffers (20 us per step of a
 * caller that hands its parameter values over as host arrays).  Saying so about results that have not all arrived is the
 * caller's error.
 */
int qsv_eval_results_seen(qsv_t* h);
/*
 * The optimiser's share of one iteration of R lock-step SPSA runs as ONE launch on the handle's stream, for a parameter search
 * whose state lives in device memory (evqe/device_search.py; the reference runs one qiskit_algorithms SPSA per individual on a
 * worker thread, mutation.py:28-89): with qsv_eval_push_device and qsv_eval_set_output an iteration is this launch plus the
 * evaluation's, and the host waits for neither.  All pointers are device memory of the handle's GPU, row-major, rows of
 * `width` doubles (a run shorter than the widest is padded with zero signs).
 *   accept  (values != NULL): values[2r], values[2r + 1] = f(x_r + eps delta_r), f(x_r - eps delta_r) measured with
 *           delta_accept; update = (f+ - f-) / (2 eps) * delta, divided by its norm if trust_region and the norm exceeds 1, times
 *           lr; x_r -= update for runs with active[r] != 0; iterations[r] counts them; a run stops (active[r] = 0) at maxiter,
 *           at 2 * iterations >= maxfev (maxfev >= 0), or by the reference's SPSATerminationChecker rule over `window` =
 *           allowed_consecutive_violations + 1 relative changes of 0.5 (f+ + f-) below min_rel (window = 0: no rule;
 *           previous / n_values / changes are its state: zeros, zeros, +inf before the first call).
 *   propose (delta_propose != NULL): points[2r] = x_r + eps delta, points[2r + 1] = x_r - eps delta.
 * Products and sums are rounded one by one as the host's NumPy expressions are; the norm is a fixed-order sum of its own.
 */
typedef struct qsv_spsa_step_args {
    int32_t n_runs, width;
    double* x;                   /* [n_runs][width] */
    uint8_t* active;             /* [n_runs] */
    int64_t* iterations;         /* [n_runs] */
    const double* delta_accept;  /* [n_runs][width], the signs the values were measured with */
    const double* values;        /* [2 n_runs]: f(x + eps delta), f(x - eps delta) per run */
    const double* delta_propose; /* [n_runs][width] */
    double* points;              /* [2 n_runs][width] */
    double eps, lr;
    int32_t trust_region, maxiter;
    int32_t window;              /* termination rule: allowed_consecutive_violations + 1, 0 = no rule */
    int32_t reserved;
    double min_rel;
    int64_t maxfev;              /* < 0: none */
    double* previous;            /* [n_runs] */
    int64_t* n_values;           /* [n_runs] */
    double* changes;             /* [n_runs][window] */
} qsv_spsa_step_args;
int qsv_spsa_step(qsv_t* h, const qsv_spsa_step_args* args);
/*
 * The optimiser's share of one iteration of R lock-step NFT runs (Nakanishi-Fujii-Todo sequential minimisation, Phys. Rev.
 * Research 2, 043158: the optimiser of the reference's own test harness, test/minimum_eigensolvers/evqe/solver.py:28-36) as ONE
 * launch on the handle's stream, for a parameter search whose state lives in device memory (evqe/device_search.py): ACCEPT
 * iteration accept_iteration from the values measured at its points, then PROPOSE the points of iteration propose_iteration.
 * Either half may be left out (accept / propose = 0): a search's first call only proposes, its last only accepts.  Fresh runs of
 * one configuration move in lock-step -- which iterations evaluate the base point and where the search ends depend on no function
 * value --, so the caller knows both iteration numbers and both forms ahead and the device keeps no counters.
 * All pointers are device memory of the handle's GPU; x and points are row-major with rows of `width` doubles.
 *   x         R x width.  Run r searches sizes[r] >= 1 of its row's entries: variable j is column columns[r * columns_stride + j]
 *             (the identity for a run that owns its row; a layer's positions inside the parameter vector of a shared circuit).
 *             The other entries of the row are never written and reach every proposed point as they are.
 *   recycled  R doubles: the fitted minimum of the run's last accepted iteration, f at its new x, which stands in for the base
 *             value of an iteration proposed without one.  Written by every accept; read only by an accept without the base.
 *   accept    with j = accept_iteration % sizes[r], col = column of variable j, and k = 3 (accept_with_base) or 2 values per run:
 *             z0 = values[3r] or recycled[r]; z1, z3 = the run's last two values (f at x[col] + pi/2 and at x[col] - pi/2);
 *             c = 0.5 (z1 + z3); cos_part = z0 - c; sin_part = 0.5 (z3 - z1); a = hypot(cos_part, sin_part);
 *             if a > 0: x[col] = (x[col] - atan2(sin_part, cos_part)) + pi;  recycled[r] = c - a.
 *             Every sum and product is rounded on its own, in this order (no fused multiply-add); hypot and atan2 are the device
 *             math library's, so the new x[col] and recycled[r] can differ from a host's in the last bits.
 *   propose   with col as above for propose_iteration: rows k r .. k r + k - 1 of points are the run's row of x, bit for bit --
 *             in the order base (only if propose_with_base, k = 3), plus, minus -- except that entry col is x[col] + M_PI_2 in
 *             the plus row and x[col] - M_PI_2 in the minus row.  The values of an iteration are expected in the same order.
 * The contents of sizes and columns are the caller's responsibility: sizes[r] in 1 .. columns_stride, columns in 0 .. width - 1.
 * (A run whose size is outside that range is left alone, and a column outside the row moves nothing; neither is reported.)
 * QSV_E_ARG: a null struct; null x / sizes / columns / recycled; n_runs or width < 0; columns_stride < 1; an accept without values;
 * a propose without points; a negative iteration number on a half that is asked for; x or points not aligned to 8 bytes.
 * n_runs == 0 or width == 0 is a successful call that launches nothing.
 */
typedef struct qsv_nft_step_args {
    int32_t n_runs, width;
    int32_t columns_stride;
    int32_t reserved;
    double* x;
    const int32_t* sizes;
    const int32_t* columns;
    double* recycled;
    int32_t accept, accept_with_base;   /* flags: any non-zero value is "yes" */
    int64_t accept_iteration;
    int32_t propose, propose_with_base;
    int64_t propose_iteration;
    const double* values;        /* [3 n_runs] (base, plus, minus per run) or [2 n_runs] */
    double* points;              /* [3 n_runs][width] or [2 n_runs][width], rows in the order of the values */
} qsv_nft_step_args;
int qsv_nft_step(qsv_t* h, const qsv_nft_step_args* args);
/*
 * The optimiser's share of one iteration of R lock-step Adam runs (evqe/solver.py: Adam, _AdamRun.accept_gradient) as ONE launch
 * on the handle's stream, for a search whose state lives in device memory (evqe/device_search.py: minimize_adam_on_device): the
 * moments, the update and the stopping rule from gradients that a qsv_gradient_plan_run queued in front of it left in device
 * memory.  It waits for nothing.  All pointers are device memory of the handle's GPU.
 *   x         R x width, row-major.  Run r searches sizes[r] >= 1 of its row's entries: variable j is column
 *             columns[r * columns_stride + j], as in qsv_nft_step_args.  The other entries of the row are never written.
 *   m, v, gradient   R x grad_width, row-major: entry j of row r belongs to variable j of run r (a row of a gradient plan's output).
 *   For every run r with active[r] != 0 and every j < sizes[r], with col the column of variable j:
 *             g = gradient[r][j]
 *             m = beta_1 * m + one_minus_beta_1 * g
 *             v = beta_2 * v + one_minus_beta_2 * (g * g)
 *             u = lr * (m / bias_1) / (sqrt(v / bias_2) + eps)
 *             x[r][col] = x[r][col] - u
 *             in this association, every product, quotient, square root and sum rounded on its own (no fused multiply-add; fp64
 *             division and square root are correctly rounded): BIT FOR BIT what _AdamRun.accept_gradient computes in NumPy.
 *             Then iterations[r] += 1; active[r] = 0 if iterations[r] >= maxiter; and, if tol > 0, active[r] = 0 also when
 *             sqrt(sum over j of u_j * u_j) < tol, the sum taken in ascending j from 0.0, every product and sum rounded on its own.
 *   A run with active[r] == 0 is not touched: its rows of x, m and v and its count stay as they are.
 *   bias_1, bias_2   1 - beta_1**t and 1 - beta_2**t of THIS iteration t (1 for a run's first), and one_minus_beta_* = 1 - beta_*,
 *             all formed by the caller: the device never calls pow, and the doubles are the ones the host driver would use.
 * The contents of sizes and columns are the caller's responsibility: sizes[r] in 1 .. min(columns_stride, grad_width), columns in
 * 0 .. width - 1.  (A run whose size is outside that range is left alone -- not even counted --, and a column outside the row
 * moves nothing while its moments are still updated; neither is reported.)
 * QSV_E_ARG: a null struct; null x / sizes / columns / m / v / gradient / active / iterations; n_runs, width or grad_width < 0;
 * columns_stride < 1; grad_width < columns_stride (a run may search columns_stride entries: its gradient row must hold them).
 * n_runs == 0 or width == 0 is a successful call that launches nothing.
 */
typedef struct qsv_adam_step_args {
    int32_t n_runs, width;
    int32_t columns_stride, grad_width;
    double* x;
    const int32_t* sizes;
    const int32_t* columns;
    double* m;
    double* v;
    const double* gradient;
    uint8_t* active;
    int64_t* iterations;
    double lr, beta_1, beta_2, one_minus_beta_1, one_minus_beta_2, eps, tol;
    double bias_1, bias_2;
    int64_t maxiter;
} qsv_adam_step_args;
int qsv_adam_step(qsv_t* h, const qsv_adam_step_args* args);
/* How many pushes the open batch is best delivered in (1 or 2): measurement-backed advice, any number works. */
int qsv_eval_suggested_pushes(const qsv_t* h);
/* Launch-group size of the handle (evaluations whose states are resident at the same time). */
int qsv_group_size(const qsv_t* h);

/* Same, with the op lists passed inline (circuit i = ops[op_offsets[i] .. op_offsets[i+1])). */
int qsv_eval_batch(qsv_t* h, int n_evals, const int64_t* op_offsets, const qsv_op* ops,
                   const int64_t* param_offsets, const double* params, double* out_expectations);

/* Final state of one circuit as interleaved (re, im) doubles, 2 * 2^n values (debug / parity checks). */
int qsv_statevector(qsv_t* h, int circuit_id, const double* params, int n_params, double* out_re_im);

/* |amplitude|^2 of every basis state, 2^n doubles.  Exact counterpart of the sampler's distribution. */
int qsv_probabilities(qsv_t* h, int circuit_id, const double* params, int n_params, double* out_probs);

/*
 * Draw `shots` basis states from the circuit's output distribution on the device (seeded inverse-CDF sampling).
 * Replaces `sampler.run(pubs, shots)` + `get_counts()` in measure_quasi_distributions (circuit_evaluation.py:50-59).
 * The draw is a function of (seed, circuit, parameters) on a given handle configuration; a circuit that has a split form
 * is sampled from its two side tables (no 2^n probabilities are formed), which walks the index space in another order
 * than the probabilities-based sampler: same distribution, different samples for the same seed.
 */
int qsv_sample(qsv_t* h, int circuit_id, const double* params, int n_params, int shots, uint64_t seed,
               uint64_t* out_states);

/*
 * The same for a batch: evaluation i draws `shots` samples into out_states[i * shots ..] from its own random stream
 * derived from (seed, i).  When the operator set on the handle is diagonal (I/Z terms only) and out_values is not
 * NULL, out_values[i * shots + s] receives the operator's value on that sample, sum_k c_k (-1)^popcount(state & z_k)
 * -- what `_evaluate_sparsepauli` computes per measured state in get_expectation_with_operator
 * (reference: queasars/circuit_evaluation/expectation_calculation.py:64-66) -- so the host only sorts for the CVaR.
 */
int qsv_sample_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                     int shots, uint64_t seed, uint64_t* out_states, double* out_values /* may be NULL */);

/*
 * Sampling and the CVaR in one call: out_cvar[i] = CVaR_alpha of the operator's values on evaluation i's `shots` samples
 * (the samples qsv_sample_batch draws for the same seed), i.e. the mean of the lowest alpha * shots sample values with
 * the boundary sample weighted fractionally -- what get_expectation_with_operator / _get_expectation compute from the
 * measured distribution (reference: queasars/circuit_evaluation/expectation_calculation.py:14-69; alpha = 1: the plain
 * mean).  Needs a diagonal operator on the handle, 0 < alpha <= 1 and shots <= 4096; the samples are sorted on the
 * device and never cross PCIe.
 */
int qsv_sample_cvar_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          int shots, uint64_t seed, double alpha, double* out_cvar);

/*
 * The sampler branch without sampling noise: out_cvar[i] = CVaR_alpha of the operator's values under the EXACT distribution
 * |amplitude|^2 of evaluation i -- the value get_expectation_with_operator / _get_expectation would return for a measured
 * distribution that equals the exact one (reference: queasars/circuit_evaluation/expectation_calculation.py:14-32, :55-69),
 * including the loop's stopping rule numpy.isclose(gathered, alpha) and, for states of equal value, the index order a stable
 * sort leaves them in.  Needs a diagonal operator on the handle, 0 < alpha <= 1 and at most 28 qubits; deterministic.
 * (For alpha = 1 -- numpy.isclose, as the reference tests it -- this is the expectation value qsv_eval_circuits computes.)  Circuits that have a split form are read from
 * their two side tables, the others from the probabilities their last gate pass writes.
 */
int qsv_exact_cvar_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                         double alpha, double* out_cvar);

/*
 * Both of the above with the parameter values READ FROM and the results LEFT IN device memory (this handle's GPU), queued on the
 * handle's stream (qsv_set_stream) without waiting: the evaluation step of an optimiser that lives on the device
 * (evqe/device_search.py with a sampler evaluator; with qsv_spsa_step an iteration is two chains of launches and the host waits for
 * neither).  Replaces, like they do, measure_quasi_distributions + get_expectation_with_operator of the reference's
 * OperatorSamplerCircuitEvaluator.evaluate_circuits (circuit_evaluation.py:94-161, expectation_calculation.py:14-69).
 *   device_values  row-major matrix of n_evals rows of `width` doubles: evaluation e takes the first n_params of row e, exactly as
 *                  qsv_eval_push_device documents (rows wider than 1024: prepared without the LDS copy, same remark).  They must
 *                  stay unchanged until the call's work is complete.  `ready_event` as in qsv_eval_push_device.
 *   shots > 0      device_out[e] = what qsv_sample_cvar_batch computes for the same circuits, values, shots, seed and alpha, bit
 *                  for bit (evaluation e draws from the stream of (seed, e)); shots <= 4096.
 *   shots == 0     device_out[e] = what qsv_exact_cvar_batch computes, bit for bit, including alpha = 1 (numpy.isclose): the
 *                  expectation value.  At most 28 qubits.
 *   device_active  may be NULL: every evaluation runs.  Otherwise entry e / active_stride (uint8) decides evaluation e: 0 = its
 *                  workgroups return at once in every kernel of the call and device_out[e] is left untouched (stride 2 with
 *                  qsv_spsa_step's own `active` array: a stopped run's plus / minus pair costs nothing and its values are not
 *                  read).  The values of the evaluations that run do not depend on the mask, bit for bit.  The mask is read by
 *                  the kernels, in stream order: what was written to it on the handle's stream before the call is what they see.
 *                  (alpha = 1 with shots == 0: switched-off evaluations still run, only their results are withheld.)
 * Returns without waiting: the results are complete once the work enqueued so far on the handle's stream is.  The next call on
 * the handle that needs the staging or scratch buffers waits for unfinished work first, as after qsv_eval_end(h, NULL) -- except
 * a qsv_cvar_device call with the same circuit_ids, width and kind (shots > 0 or not) as the one before it and nothing else in
 * between: it reuses that call's layout and neither writes a staging buffer nor waits, so the iterations of a search follow each
 * other on the stream.  A call allocates only if its scratch has to grow (more evaluations x shots than any call before) or its
 * batch is laid out afresh; it waits for the handle's streams before it frees anything.
 * Errors as the host forms: no diagonal operator QSV_E_STATE; shots > 4096, alpha outside (0, 1], a pointer that is not this
 * device's memory QSV_E_ARG; more than 28 qubits with shots == 0, and circuits on kept states, QSV_E_UNSUPPORTED.
 */
int qsv_cvar_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                    int shots /* 0: the exact distribution */, uint64_t seed, double alpha,
                    const uint8_t* device_active /* may be NULL */, int active_stride, double* device_out);

/*
 * Exact readout: the k most probable basis states of every evaluation, selected on the device.  For evaluation i,
 * out_states[i * k + j] is the j-th entry of its 2^n exact probabilities |amplitude|^2 under the total order PROBABILITY
 * DESCENDING, BASIS-STATE INDEX ASCENDING (states of equal probability -- the zeros of a shallow circuit -- come in index order;
 * probabilities are compared as doubles), out_probs[i * k + j] that probability, and out_values[i * k + j] (may be NULL) the
 * diagonal operator's value on the state, sum_k c_k (-1)^popcount(state & z_k), as qsv_sample_batch gathers it.  The order is
 * total, so the result is unique and the same bits on every call.  Replaces the last step of the reference's
 * _solve_by_evolution -- measuring the best individual once more for result.eigenstate
 * (evolving_ansatz_minimum_eigensolver.py:442-454) and taking its most probable states on the host -- without sampling noise
 * and without moving 2^n doubles (qsv_probabilities) to sort them there.  Circuits that have a split form are read from their two
 * side tables, the others from the probabilities their last gate pass writes, group by group as qsv_exact_cvar_batch; no sort of
 * 2^n pairs takes place.  1 <= k <= min(1024, 2^n), else QSV_E_ARG; out_values without a diagonal operator on the handle
 * QSV_E_STATE; more than 28 qubits, and circuits on kept states, QSV_E_UNSUPPORTED.  No operator is needed when out_values is NULL.
 */
int qsv_top_states(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                   int k, uint64_t* out_states, double* out_probs, double* out_values /* may be NULL */);

/* ---- sampled values of a host-side scoring function ------------------------------------------------ */

/*
 * VALUE CACHES.  The reference's BitstringCircuitEvaluator scores every measured state through a Python callable str -> float
 * (reference: queasars/circuit_evaluation/circuit_evaluation.py:222-291, bitstring_evaluation.py).  The callable cannot run on the
 * device; everything around it can.  A value cache is an open-addressing hash table basis state -> double in device memory that
 * lives until qsv_value_cache_destroy or the handle: 2^log2_slots slots of a uint64 key (all ones: empty; state 0 is an ordinary
 * key) and a double, home slot splitmix64(state) & (slots - 1), linear probing.  One evaluation step is two calls:
 *
 * qsv_sample_lookup draws, for n_evals (circuit, parameter vector) pairs laid out as in qsv_eval_circuits, exactly the samples
 * qsv_sample_batch draws for the same handle, circuits, values, shots and seed -- they stay in device memory; no operator is
 * needed --, looks every sample up in the table and inserts the states it does not hold.  Only those come back: the distinct
 * never-seen states of the WHOLE batch, *out_n_missing of them at *out_missing_states, in pinned host memory that stays valid and
 * unchanged until the finish (or the clear), in whatever order the device's atomics gave.  Same refusals as qsv_sample_batch.
 *
 * qsv_sample_lookup_finish takes their values, in that same order (n_values != the lookup's count: QSV_E_STATE, the lookup still
 * waits), stores them, gathers every sample's value from the table and returns out_cvar[e] (may be NULL) = CVaR_alpha of
 * evaluation e's values, sorted and summed on the device exactly as qsv_sample_cvar_batch does for an operator's values (so at most
 * 4096 shots and 0 < alpha <= 1, else QSV_E_ARG), and / or out_values[e * shots + s] (may be NULL) = the value of sample s of
 * evaluation e.  A call whose states are all known moves nothing but the results.
 *
 * Growth: before a lookup probes, the table is doubled (its entries rehashed) until 2 * (entries + n_evals * shots) <= slots --
 * the worst case of every sample being new, so a probe never meets a full table.  Where that would pass 2^log2_max_slots the
 * table is cleared first and refilled as the states come again: the scoring function is taken to be pure, so only time is lost.
 * A single call of more than 2^(log2_max_slots - 1) samples is QSV_E_ARG, before anything is launched.  1 <= log2_slots <=
 * log2_max_slots <= 30; 16 bytes of device memory per slot.
 *
 * Between a lookup and its finish only the cache's own buffers are held: other calls on the handle, lookups on other caches
 * included, are allowed.  A second lookup on the same cache is QSV_E_STATE, and so is a finish without a lookup.
 * qsv_value_cache_clear empties the table and cancels a lookup that was never finished (a scoring function that raised): the
 * states such a lookup inserted have no values yet.  An unknown cache id is QSV_E_ARG.
 */
int qsv_value_cache_create(qsv_t* h, int log2_slots, int log2_max_slots, int* out_cache_id);
int qsv_value_cache_destroy(qsv_t* h, int cache_id);
int qsv_value_cache_clear(qsv_t* h, int cache_id);
/* Counters of a cache since it was created: the states it holds and its slots now; the samples looked up, split into those whose
 * state was already there (or was inserted by another sample of the same call) and those that created an entry; how often the
 * table grew and how often it was cleared (at its largest size, or by qsv_value_cache_clear). */
typedef struct qsv_value_cache_stats_t {
    int64_t entries;
    int64_t slots;
    int64_t samples_looked_up;
    int64_t hits;
    int64_t new_entries;
    int64_t rehashes;
    int64_t clears;
} qsv_value_cache_stats_t;
int qsv_value_cache_stats(const qsv_t* h, int cache_id, qsv_value_cache_stats_t* out);
int qsv_sample_lookup(qsv_t* h, int cache_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                      int shots, uint64_t seed, int64_t* out_n_missing, const uint64_t** out_missing_states);
int qsv_sample_lookup_finish(qsv_t* h, int cache_id, int64_t n_values, const double* values, double alpha,
                             double* out_cvar /* may be NULL; needs shots <= 4096 */,
                             double* out_values /* may be NULL; n_evals * shots */);

/* ---- analytic gradients ------------------------------------------------------------------------ */

/*
 * PARAMETER-SHIFT GRADIENTS.  With the gate set id, u(theta, phi, lambda), cu3(theta, phi, lambda) the expectation value is a short
 * trigonometric polynomial in every angle, so its derivative by a parameter is an exact linear combination of the SAME circuit's
 * values at shifted parameter values (the reference hands its circuits to qiskit_algorithms optimisers, whose gradient-based ones
 * fall back to finite differences there).  With
 *     s1 = M_PI_2,  s3 = 3.0 * M_PI_2,  cp = (sqrt(2.0) + 1.0) / (4.0 * sqrt(2.0)),  cm = (sqrt(2.0) - 1.0) / (4.0 * sqrt(2.0))
 * (doubles, formed exactly so) and E(a) the value with the parameter set to a, everything else unchanged:
 *     two terms   every angle of u, phi and lambda of cu3:   dE/da = 0.5 * (E(a + s1) - E(a - s1))
 *     four terms  theta of cu3 (frequencies 1/2 and 1):      dE/da = cp * (E(a + s1) - E(a - s1)) - cm * (E(a + s3) - E(a - s3))
 *     no term     no gate reads the parameter (id gates read nothing): the derivative is 0 and nothing is evaluated
 * in that association, every product and difference rounded on its own.  A parameter's evaluations are ordered +s1, -s1, +s3, -s3;
 * an evaluation's are ordered by its requested parameters.  A parameter that more than one angle slot reads has no such rule
 * (parameter values cannot shift one occurrence): its gradient is refused.
 *
 * qsv_gradient_describe (no handle, no device): out_n_terms[p] = 0, 2 or 4 by the rules above, -1 for a parameter more than one
 * angle slot reads.  QSV_E_ARG for an op kind or a parameter index out of range.
 */
int qsv_gradient_describe(int n_ops, const qsv_op* ops, int n_params, int32_t* out_n_terms);

/*
 * Gradients of the expectation values qsv_eval_circuits computes, under the handle's operator (diagonal or general), for
 * n_evals (circuit, parameter vector) pairs laid out as there -- circuits on kept states included.  Evaluation e is
 * differentiated by its parameters wrt[wrt_offsets[e] .. wrt_offsets[e + 1]) in that order (wrt_offsets NULL: by every parameter,
 * 0 .. n_params - 1); `out` receives the entries of evaluation 0, then those of evaluation 1, and so on.  out_n_shifted (may be
 * NULL) receives the number of circuit evaluations the call ran: what an evaluation budget counts.
 *
 * The base points are uploaded once; a kernel expands them into the shifted rows in device memory, chunk by chunk ("gradient_chunk"
 * rows, qsv_set_option; default 8192), each chunk runs as one batch of the qsv_eval_begin / qsv_eval_push_device /
 * qsv_eval_set_output / qsv_eval_end driver, and a kernel combines the values.  For circuits of at most 1024 parameters every
 * entry is, BIT FOR BIT, the combination above of what qsv_eval_circuits returns at the shifted points -- for any batch, any wrt,
 * any chunk size and either entry point.
 *
 * Errors: no operator set QSV_E_STATE; a wrt index outside the circuit's parameters QSV_E_ARG; a requested parameter that more
 * than one angle slot reads QSV_E_UNSUPPORTED, named in qsv_last_error.
 */
int qsv_gradient_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          const int64_t* wrt_offsets /* NULL: every parameter of each circuit */, const int32_t* wrt,
                          double* out /* host; packed back to back by the wrt counts */, int64_t* out_n_shifted /* may be NULL */);
/*
 * The same with the points READ FROM and the gradients LEFT IN device memory (this handle's GPU): evaluation e takes the first
 * n_params values of row e of the row-major matrix device_values (rows of `width` doubles, `ready_event` as in
 * qsv_eval_push_device), and row e of device_out (rows of out_width doubles) receives its entries, the rest of the row zeros;
 * out_width smaller than an evaluation's number of entries is QSV_E_ARG.  Queued on the handle's stream (qsv_set_stream); returns
 * without waiting, with qsv_cvar_device's contract: the gradients are complete once the work enqueued so far on that stream is,
 * the points must stay unchanged until then, and the next call that needs the staging or scratch buffers waits first.  (A call of
 * more than one chunk waits for each chunk but the last.)  It allocates only when its scratch has to grow (qsv_gradient_stats).
 */
int qsv_gradient_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                        const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out, int64_t* out_n_shifted);
/* Counters of the gradient entry points: the last call's shifted evaluations and chunks, and how often their scratch (device
 * buffers and the pinned table) was allocated or grown since the handle was created, with its present size in device memory. */
typedef struct qsv_gradient_stats_t {
    int64_t n_shifted;
    int64_t n_chunks;
    int64_t n_allocations;
    int64_t scratch_bytes;
} qsv_gradient_stats_t;
int qsv_gradient_stats(const qsv_t* h, qsv_gradient_stats_t* out);

/*
 * GRADIENT PLANS: qsv_gradient_device for a caller that differentiates the SAME circuits by the SAME parameters again and again
 * (a gradient-based optimiser's iterations).  The shift tables depend on the circuits' structure and on wrt alone, so a plan
 * builds them once and keeps them in device memory of its own; its runs then follow each other on the handle's stream.
 *
 * qsv_gradient_plan_create validates exactly as qsv_gradient_device does -- same codes, same messages, QSV_E_UNSUPPORTED for a
 * parameter more than one angle slot reads --, with `width` the row length of the points a run will read and out_width that of
 * the gradients it will write.  It records the ids, both widths and the chunk size in force ("gradient_chunk"), uploads the
 * tables and waits for that upload: create may block.  out_n_shifted (may be NULL): circuit evaluations ONE run queues.
 *
 * qsv_gradient_plan_run queues on the handle's stream what qsv_gradient_device queues for the plan's ids, wrt and widths at the
 * points in device_values (ready_event as there), and row e of device_out receives, BIT FOR BIT, what that call writes -- for any
 * chunk size.  Its contract is qsv_gradient_device's: complete once the work enqueued so far on the stream is, the points
 * unchanged until then.  The ids are looked up on every run (a destroyed circuit: QSV_E_ARG); qsv_set_operator between runs is
 * allowed.  A run of a plan with ONE chunk directly behind a run of the same plan -- nothing else on the handle in between
 * but launches on its stream, qsv_adam_step for one -- writes no staging buffer, reuses the batch layout the run before it
 * left and returns without the host having waited for anything.  A plan's first run, a run behind any other batch and every
 * run of a plan with several chunks may wait where qsv_gradient_device does.
 *
 * qsv_gradient_plan_destroy waits for the handle's stream (a run may still read the tables) and frees them; qsv_destroy frees
 * the plans that are left.  Unknown plan ids are QSV_E_ARG everywhere.
 */
int qsv_gradient_plan_create(qsv_t* h, int n_evals, const int* circuit_ids, int width, const int64_t* wrt_offsets, const int32_t* wrt,
                             int out_width, int* out_plan_id, int64_t* out_n_shifted);
int qsv_gradient_plan_run(qsv_t* h, int plan_id, const double* device_values, void* ready_event, double* device_out);
int qsv_gradient_plan_destroy(qsv_t* h, int plan_id);
/* A plan's counters: shifted evaluations and chunks of one run, runs queued so far, how often the host waited for a stream or an
 * event inside those runs (the first run of a plan usually does; a one-chunk plan run again does not), and the bytes of its
 * tables in device memory. */
typedef struct qsv_gradient_plan_stats_t {
    int64_t n_shifted;
    int64_t n_chunks;
    int64_t n_runs;
    int64_t n_host_waits;
    int64_t table_bytes;
} qsv_gradient_plan_stats_t;
int qsv_gradient_plan_stats(const qsv_t* h, int plan_id, qsv_gradient_plan_stats_t* out);

/*
 * ADJOINT GRADIENTS: the same derivatives from ONE reverse sweep of the state per evaluation instead of two
 * or four circuit evaluations per entry -- for circuits that go through the state (route QSV_ROUTE_PASSES), where a shifted
 * evaluation costs a sweep per gate pass and a gradient thousands of them.  With E = Re<psi|H|psi>, psi = U_G ... U_1 |0..0>
 * and H_h the Hermitian part of H (what qsv_set_operator keeps): psi_G = psi, lambda_G = H_h psi; for g = G .. 1,
 * psi_(g-1) = U_g^dagger psi_g, every angle slot a of gate g that reads a parameter adds 2 Re<lambda_g| dU_g/da |psi_(g-1)> to
 * that parameter's entry (for cu3 the derivative's control-0 block is zero), then lambda_(g-1) = U_g^dagger lambda_g.  id gates
 * and literal angles add nothing; a parameter no gate reads has entry 0.0; a parameter SEVERAL angle slots read gets the sum --
 * what parameter shift refuses.  E = Re<psi|lambda_G> comes as a by-product.
 *
 * qsv_adjoint_describe (no handle, no device): how the sweep of a circuit differentiated by wrt[0 .. n_wrt) (n_wrt < 0: by every
 * parameter) is cut into RUNS -- consecutive gates, walked last to first, whose targets and controls lie among the qubits of one
 * workgroup tile (*out_tile_bits qubits, the lowest *out_low_bits always among them; both may be NULL).  The sweep ends at the
 * earliest gate that reads a requested parameter; gates in front of it are never swept.  Returns the number of runs (the first
 * capacity_runs of them are written: run r's tile qubits out_masks[r], its smallest and largest op index out_first_op[r] /
 * out_last_op[r]; run 0 holds the circuit's last gates) and *out_n_gates, the non-id gates swept; QSV_E_ARG for an op kind, a
 * qubit, a parameter or a wrt index out of range.  A gate's run and that run's mask do not depend on wrt.
 */
int qsv_adjoint_describe(int n_qubits, int n_ops, const qsv_op* ops, int n_params, int n_wrt, const int32_t* wrt, int capacity_runs,
                         uint64_t* out_masks, int32_t* out_first_op, int32_t* out_last_op, int64_t* out_n_gates,
                         int32_t* out_tile_bits, int32_t* out_low_bits);
/*
 * Gradients by the adjoint sweep: arguments, wrt_offsets / wrt and the layout of `out` as qsv_gradient_circuits, plus
 * out_values (may be NULL): E of every evaluation.  Each launch group's circuits run their ordinary plans into state slots (no
 * split route, as qsv_prefix_create runs them), then on the handle's stream: lambda = H_h psi into a scratch buffer of one
 * launch group's states (allocated on first need, grown by need), one launch per run, one combination.  Deterministic: an
 * evaluation's row and value are the same bits in any batch, at any position of a launch group, from either entry point and
 * on every call, and the entries of a wrt subset are, bit for bit, those entries of the full gradient.
 * Errors: no operator set QSV_E_STATE; a wrt index outside the circuit's parameters QSV_E_ARG; a circuit on a kept state
 * QSV_E_UNSUPPORTED.
 */
int qsv_adjoint_gradient_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                                  const int64_t* wrt_offsets /* NULL: every parameter of each circuit */, const int32_t* wrt,
                                  double* out /* host; packed back to back by the wrt counts */, double* out_values /* may be NULL */);
/*
 * The same with the points READ FROM and the gradients LEFT IN device memory, with qsv_gradient_device's layout (rows of `width`
 * / out_width doubles, zeros behind a row's entries, out_width smaller than an evaluation's entries QSV_E_ARG), its ready_event
 * and its stream contract: queued on the handle's stream, not waited for.  device_out_values (may be NULL): n_evals doubles.
 */
int qsv_adjoint_gradient_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                                const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out,
                                double* device_out_values /* may be NULL */);
/* Counters of the last adjoint call: gates swept and states swept (one for H and one per run, summed over its evaluations), launches
 * of the run kernel; the scratch's present size in device memory and how often it was allocated or grown since the handle was created. */
typedef struct qsv_adjoint_stats_t {
    int64_t n_gates;
    int64_t n_runs;
    int64_t n_state_sweeps;
    int64_t scratch_bytes;
    int64_t n_allocations;
} qsv_adjoint_stats_t;
int qsv_adjoint_stats(const qsv_t* h, qsv_adjoint_stats_t* out);

/*
 * DEFLATED COSTS: values and gradients of the variational-deflation cost
 *     C_e = <psi_e|H_h|psi_e> + sum_k betas[k] |<phi_k|psi_e>|^2
 * against n_states kept states phi_k (qsv_prefix_create; prefix_ids in any order, repeats allowed, at most
 * QSV_OVERLAP_MAX_STATES).  The gradient is the adjoint sweep's with another seed: lambda_G = H_h psi_e + sum_k betas[k] c_ek phi_k
 * with c_ek = <phi_k|psi_e>, for which Re<psi_e|lambda_G> = C_e; planner, runs, combination and every contract of the adjoint
 * entry points carry over.  Per launch group, on the handle's stream: lambda = H_h psi, the overlap panels and their
 * ascending-order reduction (qsv_overlap_circuits' kernels; c stays in device memory), one kernel that adds the rank-n_states
 * update to lambda on the fp64 matrix pipe (the sum over k ascending in the position of prefix_ids, fp64 also on an fp32 handle),
 * the runs, the combination, and the penalties added to E in ascending k.  A launch group in which no evaluation has a gate to
 * sweep -- a call whose wrt counts are all 0: the value-only call -- does not run the update.
 *     out          the gradient rows, as qsv_adjoint_gradient_circuits packs them
 *     out_values   (may be NULL) C_e          out_energies (may be NULL) E_e = <psi_e|H_h|psi_e>
 *     out_overlaps (may be NULL) [n_evals][n_states][2]: c_ek (re, im), the bits qsv_overlap_circuits returns
 * Contract: n_states == 0 returns, bit for bit, what qsv_adjoint_gradient_circuits returns; an evaluation's row, value, energy
 * and overlaps are the same bits in any batch, at any position of a launch group, from either entry point and on every call; the
 * entries of a wrt subset are the bits of the full gradient.  Scratch growth is counted in qsv_adjoint_stats, and the update is
 * one more state sweep per evaluation of a group that runs it.
 * Errors: no operator set QSV_E_STATE; prefix_ids or betas NULL with n_states > 0, a non-finite beta, an unknown or released kept
 * state, and the adjoint call's wrt and out_width errors QSV_E_ARG; n_states > QSV_OVERLAP_MAX_STATES, more than 28 qubits, a
 * circuit on a kept state QSV_E_UNSUPPORTED; a batch open on this thread QSV_E_STATE; n_evals == 0 QSV_OK.
 */
int qsv_deflated_gradient_circuits(qsv_t* h, int n_states, const int* prefix_ids, const double* betas /* n_states doubles */,
                                   int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                                   const int64_t* wrt_offsets /* NULL: every parameter of each circuit */, const int32_t* wrt,
                                   double* out, double* out_values /* may be NULL */, double* out_energies /* may be NULL */,
                                   double* out_overlaps /* may be NULL */);
/*
 * The same with the points READ FROM and the rows LEFT IN device memory: qsv_adjoint_gradient_device's layout, ready_event and
 * stream contract (queued on the handle's stream, not waited for; nothing crosses to the host between the forward run and the
 * sweep).  prefix_ids and betas are host memory.  device_out_values / device_out_energies: n_evals doubles; device_out_overlaps:
 * n_evals * n_states * 2 doubles; each may be NULL.
 */
int qsv_deflated_gradient_device(qsv_t* h, int n_states, const int* prefix_ids, const double* betas, int n_evals, const int* circuit_ids,
                                 int width, const double* device_values, void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt,
                                 int out_width, double* device_out, double* device_out_values /* may be NULL */,
                                 double* device_out_energies /* may be NULL */, double* device_out_overlaps /* may be NULL */);

/*
 * EXACT CVAR GRADIENTS: gradients of CVaR_alpha of the diagonal operator under the EXACT output distribution,
 * the quantity qsv_exact_cvar_batch returns.  With the basis states sorted ascending by (value v_i, index), p_i(theta) = |psi_i|^2,
 * target = alpha - (1e-8 + 1e-5 |alpha|), b the first rank whose cumulative mass cum_b reaches target (the last rank where none
 * does) and t = v_b, the rows are the derivative of
 *     t - (1 / alpha) sum_i max(t - v_i, 0) p_i(theta)
 * by theta AT t = v_b(theta) HELD FIXED (Rockafellar-Uryasev): the gradient of the expectation value of the clipped operator
 * diag(w), w_i = -max(t - v_i, 0) / alpha.  That is dCVaR_alpha / dtheta wherever the mass in front of the boundary state and the
 * mass up to and including it straddle alpha.  At a kink -- where the boundary state changes, or where the stopping rule
 * (cum_b within numpy.isclose of alpha, below it) fires -- it is one of the one-sided derivatives.  States tied with t carry
 * weight 0, so the order inside a tie does not matter.  With alpha within numpy.isclose of 1 it is the expectation value's
 * gradient: the call IS the plain adjoint call, rows and values bit for bit qsv_adjoint_gradient_circuits', and the thresholds are
 * the operator's largest value.
 * It is the adjoint sweep's with another seed: per launch group, on the handle's stream behind the forward run into state slots
 * (no split route), the exact CVaR's two-step search with p_i read from the state slot through the sorted order (no table of
 * 2^n probabilities is written; fixed-order sums, no floating-point atomics), one streaming pass that writes
 * lambda_G = diag(w) psi (fp64 arithmetic, rounded to the handle's type) and the workgroups' shares of Re<psi|lambda_G> in H psi's
 * place, the runs, the combination, and one kernel for
 *     out_values[e]     (may be NULL) CVaR_alpha = t (1 - s / alpha) + Re<psi|lambda_G>, s = max(alpha - cum_b, 0) the mass the
 *                       stopping rule leaves out: the reference's accumulation, to rounding what qsv_exact_cvar_batch returns
 *     out_thresholds[e] (may be NULL) t, the value at risk
 * Arguments, wrt_offsets / wrt and `out` as qsv_adjoint_gradient_circuits.  A call whose wrt counts are all 0 is the value-only
 * call: no run is launched.  The first call after qsv_set_operator sorts the operator's values, as the exact CVaR does.
 * Contract: an evaluation's row, value and threshold are the same bits in any batch, at any position of a launch group, from
 * either entry point and on every call; the entries of a wrt subset are the bits of the full gradient.  Scratch growth is counted
 * in qsv_adjoint_stats, where the seed pass is the one state sweep the H application is.
 * Errors: no operator or a non-diagonal one, a batch open on this thread QSV_E_STATE; alpha outside (0, 1], the adjoint call's
 * wrt and out_width errors, a pointer of the device form that is not this device's memory QSV_E_ARG; more than 28 qubits, a
 * circuit on a kept state QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK.
 * Not built: gradients of SAMPLED values, the split route, circuits on kept states, a device_active mask.
 */
int qsv_cvar_gradient_circuits(qsv_t* h, double alpha, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                               const double* params, const int64_t* wrt_offsets /* NULL: every parameter of each circuit */,
                               const int32_t* wrt, double* out, double* out_values /* may be NULL */,
                               double* out_thresholds /* may be NULL */);
/*
 * The same with the points READ FROM and the rows LEFT IN device memory: qsv_adjoint_gradient_device's layout, ready_event and
 * stream contract (queued on the handle's stream, not waited for).  device_out_values / device_out_thresholds: n_evals doubles
 * each; each may be NULL.
 */
int qsv_cvar_gradient_device(qsv_t* h, double alpha, int n_evals, const int* circuit_ids, int width, const double* device_values,
                             void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out,
                             double* device_out_values /* may be NULL */, double* device_out_thresholds /* may be NULL */);

/*
 * FOLDED-SPECTRUM AND VARIANCE COSTS: values and gradients of
 *     F_e = <psi_e| (H_h - c_e)^2 |psi_e>
 * with H_h the Hermitian part of the operator (what qsv_set_operator keeps) and c_e the evaluation's centre:
 *     centre == 0   c_e = target, one double for the call: the folded-spectrum cost, least at the eigenstate whose eigenvalue lies
 *                   nearest the target
 *     centre == 1   c_e = E_e = Re<psi_e|H_h psi_e>, formed on the device (target is not read beyond being finite): the variance
 * With r = H_h psi - c psi the residual, the value is the CENTRED form |r|^2, never negative and free of the eps * E^2
 * cancellation of qsv_variance_circuits' one pass.  The rows are the adjoint sweep's from lambda_G = (H_h - c) r with c HELD
 * FIXED, which under centre == 1 is still the derivative of the variance: d/dc <(H_h - c)^2> = -2 (E - c) vanishes at c = E.
 * The sweep is started from lambda_G - (E - c)^2 psi: a real multiple alpha psi of the state adds alpha d<psi|psi> = 0 to every
 * entry, and this one is most of lambda_G's norm where the target lies far from E -- sweeping it would add only its rounding
 * (single precision: several times the allowance of DESIGN.md 4.21).  Under centre == 1 nothing is subtracted.
 * Per launch group, on the handle's stream behind the forward run into state slots (no split route): the adjoint call's H
 * application (lambda_1 = H_h psi and the shares of E), one wave per evaluation for E and c, one streaming pass for r (fp64
 * arithmetic, rounded to the handle's type into a second buffer of the group's size) with the workgroups' shares of |r|^2 taken
 * before the rounding, one pass that writes the seed row by row from r (and psi) over lambda_1, the runs, the combination, and one kernel for
 *     out_values[e]   (may be NULL) |r|^2       out_energies[e] (may be NULL) E_e
 * An operator without x-mask groups (every diagonal operator) takes both passes in one, r_i = (D_i - c) psi_i and
 * lambda_G,i = (D_i - c) r_i (less (E - c)^2 psi_i), and allocates no second buffer.  A launch group in which no evaluation has a gate to sweep -- a call
 * whose wrt counts are all 0: the value-only call -- stops behind the shares of |r|^2: it stores neither r nor lambda_G and
 * launches no run.  Every sum is fp64 in a fixed order, without floating-point atomics.
 * Arguments, wrt_offsets / wrt and `out` as qsv_adjoint_gradient_circuits.
 * Contract: an evaluation's row, value and energy are the same bits in any batch, at any position of a launch group, from either
 * entry point and on every call; the entries of a wrt subset are the bits of the full gradient.  E agrees with qsv_eval_circuits
 * to rounding.  Scratch growth is counted in qsv_adjoint_stats, where the residual and the seed pass are one state sweep each.
 * Errors: no operator, a batch open on this thread QSV_E_STATE; centre outside {0, 1}, a non-finite target, the adjoint call's
 * wrt and out_width errors, a pointer of the device form that is not this device's memory QSV_E_ARG; more than 28 qubits, a
 * circuit on a kept state QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK.
 * Not built: penalised costs a E + b Var, a target per evaluation, the split route, circuits on kept states, gradient plans and
 * device-resident searches on these costs, Hessians.
 */
int qsv_folded_gradient_circuits(qsv_t* h, int centre /* 0: target, 1: each evaluation's own mean */, double target, int n_evals,
                                 const int* circuit_ids, const int64_t* param_offsets, const double* params,
                                 const int64_t* wrt_offsets /* NULL: every parameter of each circuit */, const int32_t* wrt,
                                 double* out, double* out_values /* may be NULL */, double* out_energies /* may be NULL */);
/*
 * The same with the points READ FROM and the rows LEFT IN device memory: qsv_adjoint_gradient_device's layout, ready_event and
 * stream contract (queued on the handle's stream, not waited for).  device_out_values / device_out_energies: n_evals doubles
 * each; each may be NULL.
 */
int qsv_folded_gradient_device(qsv_t* h, int centre, double target, int n_evals, const int* circuit_ids, int width,
                               const double* device_values, void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt,
                               int out_width, double* device_out, double* device_out_values /* may be NULL */,
                               double* device_out_energies /* may be NULL */);

/*
 * ENERGY VARIANCE: out_variances[e] = <psi_e| H_h^2 |psi_e> - <psi_e| H_h |psi_e>^2 and, where out_values is
 * not NULL, out_values[e] = <psi_e| H_h |psi_e>, for n_evals (circuit, parameter vector) pairs laid out as in qsv_eval_circuits;
 * H_h is the Hermitian part of the operator (what qsv_set_operator keeps).  Zero exactly on eigenstates of H_h; the spread of a
 * diagonal cost over the state's distribution; Var / shots is the squared statistical error of a finite-shot estimator.
 * Each launch group's circuits run their ordinary plans into state slots (no split route, as qsv_prefix_create runs them: the
 * whole state is needed), then on the handle's stream one kernel forms every row lambda_i = (H_h psi)_i from the operator tables
 * -- the diagonal table, and per x-mask group (w_re(i) - i w_im(i)) psi_(i ^ x) -- and reduces m1 = sum Re(conj(psi_i) lambda_i)
 * and m2 = sum |lambda_i|^2 in fp64 without storing lambda, and a second one writes E = m1 and Var = m2 - m1 * m1.  The scratch
 * (two doubles per evaluation and per workgroup of a launch group) is allocated on first need and grown by need.
 * The values are RAW: no division by <psi|psi>, and Var is not clamped -- rounding may leave a tiny negative number.  One pass
 * costs a cancellation of about eps * E^2 where Var << E^2 (fp64: 1e-12 at |E| = 100).
 * Contract: an evaluation's two numbers are the same bits in any batch, at any position of a launch group and on every call
 * (fixed-order sums, no floating-point atomics).  out_values agrees with qsv_eval_circuits to rounding, not bit for bit: it comes
 * from another route.  The call lays a batch out as every batch call does, so a recorded batch ("replay_launches") is dropped
 * and laid out again by the next qsv_eval_* call, which returns the bits it returned before.  Goes between batches.
 * Errors: no operator set QSV_E_STATE; out_variances NULL with n_evals > 0 (or other
 * bad arguments) QSV_E_ARG; a circuit on a kept state QSV_E_UNSUPPORTED; more than 28 qubits QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK.
 */
int qsv_variance_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          double* out_variances, double* out_values /* may be NULL */);

/* ---- several observables per evaluation ---------------------------------------------------------- */

/*
 * OBSERVABLE SETS.  The reference evaluates every aux operator at the best individual and returns the values as
 * result.aux_operators_evaluated (reference: queasars/minimum_eigensolvers/base/evolving_ansatz_minimum_eigensolver.py:177-199,
 * :461-476); an EstimatorV2 pub may hold an array of observables.  A set holds M observables
 *     O_m = sum over k in [term_offsets[m], term_offsets[m+1]) of (coeff_re[k] + i coeff_im[k]) P_k
 * (Pauli conventions as qsv_set_operator; an observable without terms is 0; duplicate strings are allowed, within an
 * observable or across observables).  Its distinct strings are grouped by x mask once, on the device.  At most 65536
 * observables, 65536 distinct strings and 2^24 terms; a term acting on a qubit >= n_qubits, n_observables < 1 or a larger
 * set is QSV_E_ARG.  Sets live until qsv_observables_destroy or the handle.
 *
 * qsv_eval_observables: out[e * n_observables + m] = real(<psi_e| O_m |psi_e>) for n_evals (circuit, parameter vector)
 * pairs laid out as in qsv_eval_circuits, psi_e prepared as qsv_eval_circuits prepares it (from |0..0>, or from the kept state
 * of a circuit registered on one).  Independent of the handle's operator: none needs to be set, no table is rebuilt and no
 * plan invalidated, and qsv_eval_* results after the call are bitwise those before it.  Deterministic: a value depends only on
 * the set, the circuit, its parameters and the handle configuration, never on the batch.  Each evaluation takes one route,
 * fixed by its circuit and the handle: a split form of at most three keys on a handle with side tables runs its two virtual
 * circuits and takes every string's value from the two side tables; everything else runs its gate passes into a state slot,
 * whose strings' values come from one Walsh-Hadamard sweep of the state per x-mask group.
 */
int qsv_observables_create(qsv_t* h, int n_observables, const int64_t* term_offsets, const uint64_t* x_mask,
                           const uint64_t* z_mask, const double* coeff_re, const double* coeff_im, int* out_set_id);
int qsv_observables_destroy(qsv_t* h, int set_id);
int qsv_eval_observables(qsv_t* h, int set_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                         const double* params, double* out);

/*
 * COVARIANCES: the second moments of a set's observables in each evaluation's state.  With lambda_m = O_m psi_e
 * for the Hermitian part O_m of observable m (a set keeps the real parts of the coefficients),
 *     out_values[e * M + m]        = E_m  = Re<psi_e|lambda_m>                     (where out_values is not NULL)
 *     out_cov[(e * M + a) * M + b] = C_ab = Re<lambda_a|lambda_b> - E_a E_b = <{O_a, O_b}> / 2 - <O_a><O_b>,
 * the full symmetric M x M matrix, row-major; C_aa is Var(O_a), and w^T C w the variance of sum_m w_m O_m.  Arguments are laid
 * out as in qsv_eval_observables.  The call runs as qsv_variance_circuits runs: ordinary plans into state slots (no split route),
 * then on the handle's stream one kernel per launch group that forms lambda_m(i) for 64 amplitudes and 16 observables at a time
 * and accumulates Re(Lambda^H Lambda) per pair of 16-observable blocks on the fp64 matrix pipe, and one that adds the workgroups'
 * partial tiles in ascending order, subtracts E_a E_b and mirrors the upper triangle.  Nothing state-sized is written; the scratch
 * is allocated on first need and grown by need, and a launch group is made smaller where its partials would pass 64 MiB.
 * The handle's operator is neither needed nor touched.  The numbers are RAW (no division by <psi|psi>, no clamping: rounding may
 * leave a diagonal entry a tiny bit below zero) and out_cov[a][b] == out_cov[b][a] bit for bit.  Contract: an evaluation's numbers
 * are the same bits in any batch, at any position of a launch group and on every call (fixed-order sums, no floating-point
 * atomics).  out_values agrees with qsv_eval_observables to rounding, not bit for bit.  The call lays a batch out as every batch
 * call does, so a recorded batch is dropped and laid out again by the next qsv_eval_* call, which returns the bits it returned
 * before.  Goes between batches.
 * Errors: unknown set QSV_E_ARG; out_cov NULL with n_evals > 0 (or other bad arguments) QSV_E_ARG; a circuit on a kept state QSV_E_UNSUPPORTED; more than 28 qubits QSV_E_UNSUPPORTED; a set of more than
 * QSV_COVARIANCE_MAX_OBSERVABLES observables QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK.
 */
#define QSV_COVARIANCE_MAX_OBSERVABLES 64
int qsv_observables_covariance(qsv_t* h, int set_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                               const double* params, double* out_values /* n_evals*M, may be NULL */,
                               double* out_cov /* n_evals*M*M */);

/* ---- two states at a time -------------------------------------------------------------------------- */

/*
 * OVERLAPS: the final states psi_e of n_evals (circuit, parameter vector) pairs, laid out as in
 * qsv_eval_circuits, against n_states kept states phi_k (qsv_prefix_create), named by prefix_ids in any order, repeats allowed:
 *     out_overlaps[(e * n_states + k) * 2 + {0, 1}] = S_ek = <phi_k|psi_e> = sum_i conj(phi_k[i]) psi_e[i]   (re, im)
 *     out_elements[(e * n_states + k) * 2 + {0, 1}] = T_ek = <phi_k|H_h|psi_e>                               (with_operator != 0)
 * with H_h the Hermitian part qsv_set_operator keeps; out_elements is required iff with_operator is set and not looked at
 * otherwise, and the handle's operator is read only then.  The call runs as qsv_variance_circuits runs: ordinary plans into state
 * slots (no split route), then on the handle's stream one kernel per launch group that takes 64 amplitudes of 16 kept states and
 * 16 evaluations at a time, forms (H_h psi_e)(i) for them where asked, and accumulates the 16 x 16 complex tiles on the fp64
 * matrix pipe, and one that adds the workgroups' partial tiles in ascending order.  Nothing state-sized is written and the
 * kept-state buffer is only read; the scratch is allocated on first need and grown by need, and a launch group is made smaller
 * where its partial tiles would pass 64 MiB.  The numbers are RAW: no division by norms.  Contract: an evaluation's row is the
 * same bits in any batch, at any position of a launch group and on every call, and a kept state's column the same bits at any
 * position of prefix_ids -- a repeated id gives two identical columns (fixed-order sums, no floating-point atomics).  The call
 * lays a batch out as every batch call does, so a recorded batch is dropped and laid out again by the next qsv_eval_* call, which
 * returns the bits it returned before.  Goes between batches.
 * Errors: out_overlaps NULL, out_elements NULL where with_operator is set, prefix_ids NULL, n_states < 1 (or other bad arguments)
 * QSV_E_ARG; an unknown or released kept state QSV_E_ARG; n_states > QSV_OVERLAP_MAX_STATES QSV_E_UNSUPPORTED; more than 28 qubits
 * QSV_E_UNSUPPORTED; an evaluated circuit on a kept state QSV_E_UNSUPPORTED; with_operator and no operator set QSV_E_STATE;
 * n_evals == 0 QSV_OK.
 */
#define QSV_OVERLAP_MAX_STATES 64
int qsv_overlap_circuits(qsv_t* h, int n_states, const int* prefix_ids, int with_operator, int n_evals, const int* circuit_ids,
                         const int64_t* param_offsets, const double* params, double* out_overlaps /* [n_evals][n_states][2] */,
                         double* out_elements /* the same shape; required iff with_operator */);

/* ---- a few qubits of a state ------------------------------------------------------------------------ */

/*
 * REDUCED DENSITY MATRICES: rho_A = Tr_rest |psi_e><psi_e| of the final states psi_e of n_evals (circuit,
 * parameter vector) pairs, laid out as in qsv_eval_circuits, for n_subsets qubit subsets A_s = subset_qubits[subset_offsets[s] ..
 * subset_offsets[s + 1]) of k_s = 1 .. QSV_RDM_MAX_QUBITS distinct qubits each, in the caller's order: bit j of a row index a is
 * the value of the subset's j-th qubit.
 *     out[e * R + off_s + 2 * (a * 2^k_s + a') + {0, 1}] = rho_s[a][a'] = sum_b psi_e(a, b) conj psi_e(a', b)   (re, im)
 * with off_s the sum of 2 * 4^k over the subsets before s and R that sum over all of them.  The matrices are raw: not divided
 * by |psi|^2.  The call runs as qsv_variance_circuits runs: ordinary plans into state slots (no split route), then on the handle's
 * stream one kernel per launch group and run of subsets that walks each state in blocks of the subset's qubits and the six lowest
 * others and accumulates 16 x 16 tiles on the fp64 matrix pipe, and a second that adds the workgroups' tiles in ascending order.
 * No operator is read: the call works on a handle that has none.  rho is Hermitian to the bit, its diagonal's imaginary parts are
 * 0.0, and the matrix of an (evaluation, subset) is the same bits in any batch, at any position of a launch group and of the
 * subset list, whatever other subsets the call names -- a repeated subset gives two identical blocks (fixed-order sums, no
 * floating-point atomics).  Every sum is fp64, also on an fp32 handle.  The call lays a batch out as every batch call does, so a
 * recorded batch is dropped and laid out again by the next qsv_eval_* call, which returns the bits it returned before.  Goes
 * between batches.
 * Errors: out, subset_offsets or subset_qubits NULL, n_subsets < 1, an empty subset, a qubit out of range or named twice in one
 * subset, n_evals < 0 QSV_E_ARG; more than QSV_RDM_MAX_QUBITS qubits in a subset, more than QSV_RDM_MAX_SUBSETS subsets, more
 * than 28 qubits, an evaluated circuit on a kept state QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK once the subsets were checked.
 */
#define QSV_RDM_MAX_QUBITS 4
#define QSV_RDM_MAX_SUBSETS 1024
int qsv_reduced_density_circuits(qsv_t* h, int n_subsets, const int32_t* subset_offsets /* n_subsets + 1 */,
                                 const int32_t* subset_qubits, int n_evals, const int* circuit_ids,
                                 const int64_t* param_offsets, const double* params, double* out);

/*
 * OPERATOR DENSITY MATRICES: the operator-weighted reduced density matrices W_A = Tr_rest(H_h |psi_e><psi_e|)
 * of the final states psi_e of n_evals (circuit, parameter vector) pairs, laid out as in qsv_eval_circuits, for H_h the Hermitian
 * part of the operator set with qsv_set_operator and n_subsets qubit subsets given as in qsv_reduced_density_circuits (the same
 * limits, the same row convention):
 *     out[e * R + off_s + 2 * (a * 2^k_s + a') + {0, 1}] = W_s[a][a'] = sum_b (H_h psi_e)(a, b) conj psi_e(a', b)   (re, im)
 * in qsv_reduced_density_circuits' layout; out_values[e] (may be NULL) = <psi_e|H_h|psi_e>, which is also Tr W_s of every subset.
 * For a gate V(s) on A with V(0) = 1 and D = dV/ds at 0 appended to the circuit, dE/ds at 0 is 2 Re sum_{a,a'} D[a][a'] conj
 * W_A[a][a'].  W is not Hermitian in general and is raw: not divided by |psi|^2.  The call runs as qsv_reduced_density_circuits
 * runs: ordinary plans into state slots (no split route), then on the handle's stream, per launch group, the adjoint sweep's
 * operator kernel, which writes lambda = H_h psi of the group into its scratch (allocated on first need, grown by need; the only
 * state-sized write) and leaves its shares of <H>, and per run of subsets one kernel that walks psi and lambda in blocks of the
 * subset's qubits and the six lowest others and accumulates four 16 x 16 tiles on the fp64 matrix pipe, and a second that adds the
 * workgroups' tiles in ascending order.  The matrix of an (evaluation, subset) is the same bits in any batch, at any position of
 * a launch group and of the subset list, whatever other subsets the call names, and on every call (fixed-order sums, no
 * floating-point atomics); so is a value.  Every sum is fp64, also on an fp32 handle, whose lambda is fp32.  The call lays a
 * batch out as every batch call does, so a recorded batch is dropped and laid out again by the next qsv_eval_* call, which returns
 * the bits it returned before.  Goes between batches.
 * Errors: everything qsv_reduced_density_circuits refuses, with the same codes; no operator set QSV_E_STATE; n_evals == 0 QSV_OK
 * once the subsets were checked.
 */
int qsv_operator_density_circuits(qsv_t* h, int n_subsets, const int32_t* subset_offsets /* n_subsets + 1 */,
                                  const int32_t* subset_qubits, int n_evals, const int* circuit_ids,
                                  const int64_t* param_offsets, const double* params, double* out,
                                  double* out_values /* may be NULL: <H> per evaluation */);

/* ---- the geometry of a circuit's parameters ---------------------------------------------------------- */

/*
 * FUBINI-STUDY METRIC (a quarter of the quantum Fisher information): for n_evals (circuit, parameter vector)
 * pairs laid out as in qsv_eval_circuits,
 *     out[e * W * W + i * W + j] = G_ij = Re<d_i psi|d_j psi> - <d_i psi|psi><psi|d_j psi>,   W = out_width,
 * over the requested parameters of evaluation e: wrt[wrt_offsets[e] .. wrt_offsets[e + 1]), or every parameter of its circuit
 * where wrt_offsets is NULL (qsv_adjoint_gradient_circuits' rules); zeros behind an evaluation's entries.  A parameter several
 * angle slots read gets the sum over them, a parameter no gate reads a zero row and column; id gates and literal angles add
 * nothing.  The call runs as qsv_adjoint_gradient_circuits runs -- ordinary plans into state slots (no split route), then on the
 * handle's stream the adjoint sweep's runs (qsv_adjoint_describe, over the WHOLE circuit) --, but what it carries backwards
 * beside psi is one derivative state per requested angle slot, born at its gate as dU/d(slot) psi_(g-1); behind the sweep one
 * kernel forms the real Gram matrix of these columns and i psi on the fp64 matrix pipe and a second adds the workgroups' tiles
 * in ascending order, subtracts b b^T (b = Im<psi|xi>) and sums slots into parameters.  No operator is read: the call works on a
 * handle that has none.  Every sum is fp64, also on an fp32 handle.  G is symmetric to the bit; an evaluation's matrix is the
 * same bits in any batch and at any position of a launch group, and the matrix of a wrt subset is, bit for bit, that submatrix of
 * the full one (fixed-order sums, no floating-point atomics; the sweep does not stop early for a subset -- what it would leave
 * un-swept changes the last bits of every sum).  Scratch: (columns + 2) states per evaluation of a launch group, as wide as the
 * call's largest evaluation, allocated on first need, grown by need and bounded by option "metric_scratch_mib": the launch group
 * shrinks to what fits.  Goes between batches.
 * Errors: out NULL with n_evals > 0, a wrt index outside the circuit's parameters, out_width smaller than an evaluation's
 * entries, n_evals < 0 QSV_E_ARG; more than 28 qubits, a circuit on a kept state, one evaluation's columns beyond the scratch
 * bound (qsv_last_error names how many fit) QSV_E_UNSUPPORTED; n_evals == 0 QSV_OK.
 */
int qsv_metric_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                        const int64_t* wrt_offsets /* NULL: every parameter of each circuit */, const int32_t* wrt, int out_width,
                        double* out /* host: [n_evals][out_width][out_width] */);
/* Counters of the last metric call: columns carried (summed over its evaluations), launches of the run kernel and of the Gram
 * kernel; with option "time_moments" on, the device time of those launches in milliseconds (0.0 otherwise); the scratch's present
 * size in device memory and how often it was allocated or grown since the handle was created. */
typedef struct qsv_metric_stats_t {
    int64_t n_columns;
    int64_t n_run_launches;
    int64_t n_gram_launches;
    int64_t scratch_bytes;
    int64_t n_allocations;
    double run_ms;
    double gram_ms;
} qsv_metric_stats_t;
int qsv_metric_stats(const qsv_t* h, qsv_metric_stats_t* out);

/* ---- sharded populations on one node ------------------------------------------------------------- */

/*
 * The waiting part of one step through a node's shared fitness table (queasars_amd/distributed.py, _NodeTable; reference:
 * the executor's futures of selection.py:75-85 -- here every rank's values land in a table all ranks map).  `own`: this rank's
 * slot (count doubles that the rank marked with QSV_TABLE_SENTINEL before it started its evaluation, whose kernels store
 * the values there); `done`: the ranks' step counters, `stride` 64-bit words apart.  Spins until no sentinel is left in the
 * slot, publishes done[rank * stride] = step, spins until every rank's counter has reached `step`.  Needs no handle and no
 * GPU.  Returns 0; 1 / 2 when the slot / the counters were not there after budget_us microseconds (nothing published in
 * case 1): the caller decides how to go on waiting.
 */
#define QSV_TABLE_SENTINEL 0x7FF8C0DEC0DE0001ull
int qsv_fitness_table_wait(const volatile uint64_t* own, int count, volatile int64_t* done, int stride, int world, int rank,
                           int64_t step, int budget_us);

/* ---- measurement support ----------------------------------------------------------------------- */

/*
 * Switches of a handle, for measurements and tests (the defaults are the measured best).  name / value:
 *   "split" 0|1          weakly entangled circuits run as two virtual circuits (csrc/split.hpp); 1 needs a handle that was
 *                        created with splitting on.  Applies to circuits registered afterwards.
 *   "factor" 0|1         split evaluations use the factorised expectation kernels instead of the contraction sweep
 *   "fused_factor" 0|1   ... inside the launch that runs their virtual circuits, where a circuit qualifies (one launch per push)
 *   "fused_lds_table" 0|1 ... and there a side hands its state to its Gram matrices through LDS where it fits (up to twelve
 *                        virtual qubits as the state would lie in memory; three-key sides of thirteen as padded rows read in
 *                        place) instead of through its slot: the same sums in the same order, the same bits
 *   "sides_r3" 0|1       ... at 20 qubits and below (12-qubit tiles, fp64) the sides of that route are planned with EIGHT amplitudes per
 *                        thread instead of the handle's sixteen -- twice the waves per side: a gate phase is one wave's issue time over
 *                        its own amplitudes --, and a side of thirteen virtual qubits runs as TWO workgroups, one per value of its last
 *                        key qubit, that trade half rows through memory (where its plan does not leave that qubit outside the tile:
 *                        as two tiles swept by one workgroup).  Other orders of the sums (1e-10 apart).  Applies to circuits
 *                        registered afterwards.
 *   "final_controls" 0|1 ... and a side simulates no key qubit for a key whose control on it is FINAL (nothing targets the control after
 *                        the key's first gate; qsv_split_describe_reduced): the rows of that key are the two halves of the one state.
 *                        Only on that route; every other consumer of side states keeps the full form.  Other orders of the sums
 *                        (1e-10 apart).  Applies to circuits registered afterwards; QSV_FINAL_CONTROLS=0 in the environment.
 *   "live_entries" 0|1   ... and a THREE-key evaluation with a side on that form hands off and combines only the LIVE entries of its
 *                        sides' Gram tables (qsv_live_entries): an entry whose rows differ in a final-control key is an exact zero on
 *                        the side that projects, and the combination multiplies entry by entry.  64 >> f values a weight instead of
 *                        64, f the final-control keys of both sides; the same terms in the same order, the same bits.  Takes effect
 *                        at the next launch (a recorded launch is dropped); QSV_LIVE_ENTRIES=0 in the environment.
 *   "side_prepare" 0|1   ... and a side whose plan qualifies (one pass, at most two tiles, its angle table, fold index and chain index
 *                        within 4096 plan words) is prepared from ONE staged read of its plan and parameters, and keeps its threads'
 *                        and tiles' factors in registers instead of handing them to itself through memory: the same expressions in
 *                        the same order, the same bits.  Takes effect at the next launch.
 *   "side_diag" 0|1      ... and reads its values of D from a table of its own -- entry x of a side = D[x deposited in the side's
 *                        qubits], one run, filled when the circuit's plan is uploaded -- instead of gathering them from D, one
 *                        cache line per value: the same values, the same bits.  A side on the reduced form ("final_controls")
 *                        always has and reads a table of its own, whatever this option says: with 0 only the sides on the full
 *                        form gather from D itself
 *   "split_max_keys" 0..5 most cut keys of a split form (default 5; four and five: quadratic operators only).  Applies to
 *                        circuits registered afterwards.
 *   "chain_stream" 0|1   in a push that holds split evaluations of both kinds (finished by the launch that runs their
 *                        virtual circuits / with launches of their own) the second kind runs on the second lane's stream
 *   "poll_results" 0|1   a waiting qsv_eval_end watches the (pinned) result buffer instead of the streams: every result is one
 *                        8-byte store, visible about 5 us before the stream's completion signal (diagonal operators)
 *   "repeat_layout" 0|1  a batch with the previous batch's circuit ids and counts, nothing registered or set in between,
 *                        keeps that batch's layout (an optimiser's next iteration)
 *   "replay_launches" 0|1  ... and, where that batch went through in ONE push that made nothing but kernel launches (no mask, no
 *                        profiling, no second chain of launches on another stream), its push queues those launches again as they were
 *                        recorded -- grids, instantiations and argument structs by value, only the call's own pointers set anew
 *                        (parameter values, descriptors, result buffer) -- instead of deriving them from the circuits once more: the
 *                        same launches, the same bits.  Default 1 (QSV_REPLAY=0: off); needs "repeat_layout".
 *   "split_sampling" 0|1 split circuits are sampled from their side tables
 *   "streams" 1..4       HIP streams the pushes of a batch cycle over (at most as many as were created with the handle)
 *   "gradient_chunk" 0..1048576  shifted evaluations a gradient call expands and runs at a time (0: the default, 8192); the same
 *                        bits at any value
 *   "max_grid_y" 0..limit  x-mask groups of a general operator (qsv_set_operator), and rows of an observable set
 *                        (qsv_observables_create), that one launch takes: such a launch has one row of workgroups per group, and an
 *                        operator may hold more groups than the device's largest gridDim.y (hipDeviceAttributeMaxGridDimY, read
 *                        when the handle is created: the default, 0, and the largest value accepted).  More groups go in several
 *                        launches with the partial sums laid out as one launch lays them out: the same bits at any value
 *   "time_moments" 0|1   qsv_variance_circuits and qsv_observables_covariance bracket the two kernels of every launch group by HIP
 *                        events on the handle's stream and leave their summed device time in qsv_get_profile's expect_ms (measurements; the same bits);
 *                        qsv_metric_circuits brackets its run launches and its Gram kernels: qsv_metric_stats' run_ms / gram_ms
 *   "metric_scratch_mib" 1..1048576  most device memory, in MiB, that qsv_metric_circuits' scratch of derivative states may take
 *                        (default 8192); the same bits at any value
 * Returns QSV_E_ARG for an unknown name or a value out of range.
 */
int qsv_set_option(qsv_t* h, const char* name, int value);

/*
 * The LIVE entries of a three-key evaluation's 8 x 8 Hermitian Gram tables on the one-launch route (option "live_entries"),
 * without touching any device.  key_mask: the keys (bits of kappa, 0 .. 7) whose final control a side of the evaluation projects
 * on.  Entry pi < 64 -- the 8 diagonal entries, then the real and the imaginary part of every pair of rows (ja, jb), ja < jb, in
 * lexicographic order -- is live iff ja and jb agree on every key of the mask; every other entry is an exact zero on the side
 * that projects, and adds nothing to the combination.  out_pi[r] receives the entry of live rank r, in ascending order, -1
 * beyond; returns their number, 64 >> popcount(key_mask).  n_keys other than 3, a mask above 7 or a null pointer: QSV_E_ARG.
 * Used by the CPU-side tests; the kernel asks the same function (csrc/kernels.hpp live_entry).
 */
int qsv_live_entries(int n_keys, unsigned key_mask, int* out_pi);

/* Pushes of this handle, since it was created, that queued a kept layout's recorded launches ("replay_launches"). */
long long qsv_replayed_pushes(const qsv_t* h);

int qsv_set_profiling(qsv_t* h, int enabled);
int qsv_get_profile(const qsv_t* h, qsv_profile* out);

/*
 * Roofline microbenchmark: apply one u (control < 0) or cu3 gate with the given angles
 * to the resident 2^n state `reps` times and report the average device time per sweep in milliseconds.
 */
int qsv_bench_gate(qsv_t* h, int target, int control, double theta, double phi, double lambda, int reps,
                   double* out_ms_per_sweep);

/*
 * Same for an arbitrary bound gate list (every angle literal): the ops are scheduled into passes WITHOUT folding
 * and applied read-modify-write to the resident state `reps` times.  Reports milliseconds per repetition and the
 * number of passes one repetition takes.
 */
int qsv_bench_ops(qsv_t* h, int n_ops, const qsv_op* ops, int reps, double* out_ms_per_rep, int* out_n_passes);

/*
 * Build (without touching any device) the pass plan the scheduler produces for a circuit and copy its encoded
 * words out; *n_words receives the size needed.  Used by the CPU-side tests to check the scheduler.
 */
int qsv_plan_build(int n_qubits, int dtype, int n_ops, const qsv_op* ops, const qsv_plan_config* cfg,
                   uint32_t* out_words, size_t capacity_words, size_t* n_words);

/*
 * How the scheduler would split a circuit into two virtual circuits (csrc/split.hpp), without touching any device.
 * Returns the number of cut keys K (>= 0), or -1 when the circuit keeps its ordinary plan; an argument error is
 * QSV_E_ARG - 100.  mask_a receives the qubits of side A (the rest is side B).  The virtual circuits come back as op
 * lists on popcount(side) + K qubits (side qubits in ascending order, then the keys): kind QSV_OP_U / QSV_OP_CU3,
 * angles as in the input, except that p_theta = -2 / -3 / -4 stands for the fixed matrix diag(1, 0) / [[1,0],[1,0]] / X.
 * The final states a_kappa, b_kappa of the two circuits give  psi[i] = sum_kappa a[kappa, i|A] * b[kappa, i|B].
 * Used by the CPU-side tests.
 */
int qsv_split_describe(int n_qubits, int n_ops, const qsv_op* ops, int max_side, uint64_t* mask_a, qsv_op* ops_a,
                       int capacity_a, int* n_ops_a, qsv_op* ops_b, int capacity_b, int* n_ops_b);

/*
 * The REDUCED form of the same partition and keys (csrc/split.hpp, reduce_final_controls), without touching any device.
 * A key whose control c is FINAL -- nothing targets c after the key's first gate -- needs no key qubit on the control's
 * side: a_kappa(x) = a(x) [x_c = kappa_j].  Return value and mask_a as qsv_split_describe.  Per side s (0 = A, 1 = B):
 *   simulated_keys[s]  the keys (bits of kappa) the side still simulates with a key qubit;
 *   final_keys[s]      the keys whose final control lies on the side (the other bits of kappa);
 *   key_bits[s * QSV_SPLIT_MAX_KEYS + j]  key j's bit in the side's index: its key qubit's, or its final control's
 *                      (-1 beyond the K keys);
 *   qubits[s * 32 + p] the register's qubit at position p of the side's index, p < popcount(side) (-1 beyond): the
 *                      qubits that are no final controls in ascending order, then the final controls in key order.
 * The op lists are on popcount(side) + popcount(simulated_keys[s]) qubits: the real qubits as `qubits` orders them, then
 * the simulated keys in ascending order.  With a, b the final states of the two circuits and e_s(kappa, i) the index
 * made of the side's real bits of i and, for each simulated key j, kappa_j at key_bits[s][j]:
 *   psi[i] = sum_kappa  [i_c = kappa_j for every final key j of A] a[e_A(kappa, i)]
 *                     * [i_c = kappa_j for every final key j of B] b[e_B(kappa, i)].
 * Used by the CPU-side tests; the one-launch route runs this form where a side gets smaller (option "final_controls").
 */
#define QSV_SPLIT_MAX_KEYS 8
int qsv_split_describe_reduced(int n_qubits, int n_ops, const qsv_op* ops, int max_side, uint64_t* mask_a, qsv_op* ops_a,
                               int capacity_a, int* n_ops_a, qsv_op* ops_b, int capacity_b, int* n_ops_b,
                               uint32_t* simulated_keys, uint32_t* final_keys, int* key_bits, int* qubits);

/* Library version string. */
const char* qsv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QSV_H */
