// C ABI of libqsv (include/qsv.h): handle, device memory, plan cache, launch sequencing.
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/qsv.h"
#include "adjoint.hpp"
#include "moments.hpp"
#include "covariance.hpp"
#include "overlap.hpp"
#include "operator_density.hpp"
#include "reduced_density.hpp"
#include "metric.hpp"
#include "deflation.hpp"
#include "cvar_gradient.hpp"
#include "folded.hpp"
#include "gradient.hpp"
#include "value_cache.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "split.hpp"

using namespace qsv;

namespace {

// what a result slot holds until its evaluation's kernel writes it: a NaN whose payload no arithmetic produces
constexpr uint64_t kResultSentinel = 0x7ff8dead5e4717e1ull;
constexpr int kPollMicros = 200;

// Error text is kept per calling thread (and per handle it belongs to): the thread that received a failing return code
// is the one that asks for the text, and it must not race with another thread's failure on the same handle.
constexpr size_t kInlineCacheLimit = 4096;  // structures qsv_eval_batch keeps registered between calls

thread_local std::string g_create_error;
thread_local std::string g_handle_error;
thread_local const void* g_handle_error_owner = nullptr;

// A circuit the scheduler could split (split.hpp): the plans of the two virtual circuits and the contraction's index
// maps follow the ordinary plan in `plan.words` (offsets relative to it, like everything in a plan).
struct SplitInfo {
    bool ok = false;
    int n_keys = 0;
    PlanStats stats[2];
    int t[2] = {0, 0};              // thread bits of the two plans
    int outer[2] = {0, 0};          // qubits outside a tile (0: the virtual circuit is one tile)
    int n_virtual[2] = {0, 0};      // qubits of the virtual circuits
    uint32_t off_side[2] = {0, 0};  // word offsets of the side plans
    uint32_t off_block = 0;         // ... and of the split block (kernels.hpp)
    int tile_bits[2] = {0, 0};      // tile of the two plans (a side's tile may be larger than the handle's, see build_circuit)
    bool fused = false;             // both virtual circuits are one pass (kernels.hpp kEvalFused)
    bool halves = false;            // ... three keys, thirteen virtual qubits a side: two workgroups per side (kernels.hpp kEvalHalves)
    int side_r = 0;                 // amplitudes per thread of the side plans, as log2 (the handle's, or 3: build_circuit)
};

struct Circuit {
    int n_params = 0;
    int n_gates = 0;                // non-identity ops
    CircuitPlan plan;               // words: everything of this circuit that lives in the device arena; stats: of the
                                    // ordinary multi-pass plan, once it exists
    SplitInfo split;
    // The form the ONE-LAUNCH route runs instead where a side has final controls (split.hpp, reduce_final_controls; option
    // "final_controls"): plans of the reduced sides and a split block of their own behind the full form's, which every other
    // consumer of side states keeps.  A side that is not reduced shares the full form's plan.  By side X / Y of the block:
    // the side's qubits without its final controls, and the final controls as SideDiagJob::top wants them.
    SplitInfo reduced;
    uint32_t reduced_mask[2] = {0, 0}, reduced_top[2] = {0, 0};
    // The ordinary plan of a circuit that has a split form is scheduled when something first needs it (a general
    // operator, a state read-out, sampling): a population of fresh structures under a diagonal operator never does,
    // and its scheduling was half the cost of registering a structure.
    bool has_plan = false;
    uint32_t off_plan = 0;          // word offset of the ordinary plan inside plan.words
    bool fold = true;
    std::vector<GateIn> gates;      // (kept until the ordinary plan is built)
    std::vector<AngleSource> angles;
    bool uploaded = false;
    bool staged = false;            // scratch flag of upload_plans (a circuit may appear several times in a batch)
    uint32_t plan_base = 0;         // word offset in the device arena
    int prefix_id = -1;             // >= 0: the circuit continues that kept state (qsv_circuit_create_on_prefix) instead of |0..0>
    std::vector<int32_t> grad_terms;  // per parameter: shifted evaluations its derivative takes (gradient.hpp: gradient_plan)
    std::vector<qsv_op> ops;          // the ops as they were registered: what the adjoint sweep plans and differentiates (adjoint.hpp)
};

// A kept state (qsv_prefix_create): one slot of the handle's prefix buffer, alive while the caller holds it or a circuit
// continues it.
struct PrefixState {
    uint32_t slot = 0;
    int refs = 0;          // circuits registered on it
    bool released = false; // the caller has let go (qsv_prefix_destroy): the slot is recycled once refs == 0
};

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// An observable set (qsv_observables_create): its distinct Pauli strings as pauli_terms_kernel and split_term_values_kernel
// read them, and each observable as a list of (string, real coefficient) in the caller's order (kernels.hpp)
struct ObservableSet {
    uint32_t n_obs = 0;
    uint32_t n_terms = 0;  // distinct strings
    int n_rows = 0;
    int nb = 1;            // workgroups per row and state of pauli_terms_kernel
    DeviceBuffer d_rows, d_terms, d_split_terms, d_offsets, d_term_of, d_coef;
    // what covariance_panels_kernel reads (covariance.hpp; sets of up to kCovMaxObservables only): each observable's terms grouped
    // by x mask, in the caller's order within a group
    DeviceBuffer d_cov_first, d_cov_groups, d_cov_terms;
};

}  // namespace

// Persistent host threads for scheduling many circuit structures at once (a generation of EVQE brings up to a
// population of new structures): spawning threads per call would cost more than the plans.
class WorkerPool {
public:
    explicit WorkerPool(unsigned n_threads) {
        for (unsigned i = 0; i < n_threads; ++i) threads_.emplace_back([this]() { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stop_ = true;
        }
        wake_.notify_all();
        for (std::thread& t : threads_) t.join();
    }
    // run fn(0 .. count-1), the calling thread takes part; returns when every index is done
    void run(size_t count, const std::function<void(size_t)>& fn) {
        if (count == 0) return;
        {
            std::lock_guard<std::mutex> lock(mu_);
            fn_ = &fn;
            count_ = count;
            next_.store(0);
            pending_ = count;
            ++generation_;
        }
        wake_.notify_all();
        work();
        std::unique_lock<std::mutex> lock(mu_);
        done_.wait(lock, [this]() { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void work() {
        for (;;) {
            const size_t i = next_.fetch_add(1);
            if (i >= count_) return;
            (*fn_)(i);
            std::lock_guard<std::mutex> lock(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lock(mu_);
                wake_.wait(lock, [&]() { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                if (!fn_) continue;
            }
            work();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable wake_, done_;
    const std::function<void(size_t)>* fn_ = nullptr;
    std::atomic<size_t> count_{0};
    size_t pending_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t generation_ = 0;
    bool stop_ = false;
};

// A value cache (qsv_value_cache_create): the table, what one lookup leaves for its finish -- every sample's slot and the
// slots of the new entries, so that nothing is probed twice and nothing of the handle's scratch is held in between -- and the
// pinned buffers the miss list and its values cross in.
struct ValueCache {
    int log2_slots = 0, log2_max_slots = 0;
    uint64_t* d_keys = nullptr;
    double* d_vals = nullptr;
    DeviceBuffer d_sample_slot, d_miss_slots, d_counters;
    uint64_t* h_miss = nullptr;  // pinned: the miss list's states, written by the probe kernel
    size_t h_miss_bytes = 0;
    double* h_values = nullptr;  // pinned: their values, read by the fill kernel
    size_t h_values_bytes = 0;
    uint32_t* h_counters = nullptr;  // pinned copy of d_counters
    int64_t entries = 0;
    bool pending = false;  // a lookup waits for its finish
    int64_t pending_evals = 0, pending_missing = 0;
    int pending_shots = 0;
    int64_t samples_looked_up = 0, hits = 0, new_entries = 0, rehashes = 0, clears = 0;
};

struct qsv_handle {
    int n = 0, dtype = 0, device = 0;
    PlanConfig cfg;
    Geometry geo;
    int group = 1;
    size_t amp_bytes = 16;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // Second stream for the streaming evaluation: consecutive pushes alternate between the two, so that the
    // compute-bound first pass of one push runs beside the memory-bound later passes of the other.
    std::vector<hipStream_t> side_streams;  // (own, non-blocking); pushes cycle over `stream` and these
    int n_lane_streams = 0;  // the first so many of side_streams are lanes of pushes
    int aux_stream = -1;  // index in side_streams of the stream that is never a push's lane: in a batch that mixes split and
                          // ordinary evaluations the ordinary ones run there, beside the split ones (eval_push).  Created
                          // when a batch first needs it: a process has few hardware queues (four by default), and streams
                          // beyond them share queues -- with two handles alive, a third stream per handle made the two
                          // pushes of a 256-evaluation step run one after the other (262 -> 358 us).
    int chain_stream = -1;  // index in side_streams of the stream that takes, in a push that holds both kinds, the split
                            // evaluations that need launches of their own (virtual circuits, Gram matrices, combination) --
                            // beside the one-launch ones on the push's lane instead of in front of them (eval_push)
    // Counts everything that could make the layout of an earlier batch stale: registrations, operators, options, every full
    // batch_layout, a reallocated staging buffer.  A batch whose ids and counts are the previous batch's, with nothing counted
    // in between, is that batch again (an optimiser's next iteration over the same population): eval_begin keeps its layout.
    uint64_t epoch = 1;
    bool repeat_enabled = true;
    bool replay_enabled = true;   // a repeated whole-push batch queues the kept layout's recorded launches again (replay_push)
    uint64_t replayed_pushes = 0;  // pushes that did (qsv_replayed_pushes)
    // QSV_HOST_TIMING=1 (read when the handle is created): where the host's share of a qsv_eval_begin / push / end call goes,
    // summed over the handle's life and printed when it is destroyed.  Off: one test of `on` per phase.
    struct HostTiming {
        bool on = false, in_push = false;
        uint64_t calls = 0, replays = 0;
        double begin_us = 0, push_us = 0, launch_us = 0, end_us = 0, copy_us = 0;  // (push_us holds launch_us, end_us holds copy_us: reported apart)
    } timing;
    bool chain_enabled = true;
    bool fused_lds_table = true;  // one-launch route: small sides hand their state to the Gram matrices through LDS (kModeFusedLdsTable)
    bool side_prepare = true;     // one-launch route: a side is prepared from one staged read of its plan (kModeSidePrepare); asked at every launch
    int n_cus = 256;
    int max_grid_y = 65535, device_max_grid_y = 65535;  // the device's largest gridDim.y (and what option "max_grid_y" makes of it):
                                                          // launches with one row of workgroups per x-mask group are sliced by it
    bool poll_results = true;  // a waiting end of a batch watches the (pinned) result buffer instead of the streams: the last
                               // workgroups' stores are visible about 5 us before hipStreamSynchronize returns (eval_end)
    hipStream_t work = nullptr;  // stream of the push being issued (null: `stream`)
    hipEvent_t ev_join = nullptr;
    int n_streams = 2;           // streams a batch cycles over (QSV_STREAMS, 1 .. 4)
    bool split_enabled = true;   // weakly entangled circuits run as two virtual circuits + a contraction (split.hpp)
    bool split_sampling = true;  // ... and are sampled from their two side tables (kernels.hpp: launch_split_sample)
    bool factor_enabled = true;  // ... and, under a quadratic diagonal operator, need no sweep over the 2^n indices at all
                                 // (kernels.hpp: launch_factor)
    bool fused_factor = true;    // ... in the launch that runs the virtual circuits, where the circuit qualifies (kEvalFused)
    int split_max_keys = 5;      // most cut keys of a split form: four and five (16 / 32 product terms, quadratic operators
                                 // only) -- their chain of launches (virtual circuits of up to 16 qubits, Gram matrices of up to
                                 // 1024 entries) runs beside the one-launch evaluations of the push on the second lane's stream
                                 // (eval_push).  QSV_SPLIT_MAX_KEYS / qsv_set_option "split_max_keys" = 3: the round-2 limit
    bool quadratic = false;      // the operator is diagonal and every term has at most two Z factors
    DeviceBuffer d_quad;         // its couplings as an n x n matrix
    DeviceBuffer d_fterms;       // a general operator's terms as a plain list (kernels.hpp: launch_factor_terms)
    uint32_t n_fterms = 0;
    DeviceBuffer d_fpart;        // ... and that kernel's partial sums
    DeviceBuffer d_factor;       // launch_factor's partial Gram matrices, one region per side-table slot
    DeviceBuffer d_factor_count; // kModeFusedFactor: one counter per side-table slot (each fused evaluation adds two)
    DeviceBuffer d_factor_big;   // launch_factor_big's partial Gram matrices (four and five keys), allocated on first need
    DeviceBuffer d_factor_big_count;  // ... and their workgroup counters (zeroed once)
    uint32_t stream_mode = 0;    // kModeStreaming when a state is larger than the Infinity Cache (256 MiB), else 0
    mutable std::mutex mu;
    std::atomic<std::thread::id> batch_owner{};  // thread that holds `mu` between qsv_eval_begin and qsv_eval_end

    // operator
    int n_terms = 0;
    bool diagonal = false;        // every term is I/Z: the whole expectation is fused into the last gate pass
    bool has_diag_part = false;   // some terms are I/Z (their diagonal table exists)
    int n_groups = 0;             // x-mask groups of the off-diagonal terms
    DeviceBuffer d_z, d_cre, d_diag, d_term_partials, d_groups, d_term_odd;
    DeviceBuffer d_order, d_sorted;  // the basis states in ascending order of the diagonal operator's value, and the values
    bool order_valid = false;        // (sort.hip; built when the exact-probability CVaR first needs them)
    int pauli_nb = 0;

    // circuits
    std::unordered_map<int, Circuit> circuits;
    int next_circuit_id = 1;
    // kept states (qsv_prefix_create): slots of one buffer that grows by doubling
    std::unordered_map<int, PrefixState> prefixes;
    int next_prefix_id = 1;
    DeviceBuffer d_prefix;
    // the sides' own tables of D (kernels.hpp kSplitSideDiag): filled when a split circuit's plan is uploaded, gone with the arena
    DeviceBuffer d_sdiag;
    size_t sdiag_used = 0;             // doubles handed out
    bool side_diag = true;             // (QSV_SIDE_DIAG=0: the sums gather from D itself, as before round 4)
    bool final_controls = true;        // one-launch route: a side simulates no key qubit for a key whose control on it is final (split.hpp,
                                       // reduce_final_controls); circuits registered afterwards.  QSV_FINAL_CONTROLS=0 / option "final_controls"
    bool live_entries = true;          // one-launch route: a three-key evaluation with a reduced side hands off and combines only the live
                                       // entries of its Gram tables (kernels.hpp kModeFusedLive); the next launch.  QSV_LIVE_ENTRIES=0 /
                                       // option "live_entries"
    bool sides_r3 = true;              // one-launch route at 20 qubits: sides of up to twelve virtual qubits planned with EIGHT amplitudes per thread
                                       // (a gate phase is one wave's issue time over its own amplitudes: twice the waves, half the time),
                                       // three-key sides of thirteen as two workgroups each (kEvalHalves); circuits registered afterwards
    size_t prefix_slots = 0;           // capacity
    std::vector<uint32_t> prefix_free; // recycled slots
    size_t prefix_used = 0;            // slots handed out so far (below capacity)
    std::unordered_map<std::string, int> inline_cache;
    // observable sets (qsv_observables_create) and the scratch of qsv_eval_observables: per-workgroup partial sums of the
    // strings' values, and the values
    std::unordered_map<int, ObservableSet> obs_sets;
    int next_obs_id = 1;
    DeviceBuffer d_obs_partials, d_obs_values;
    std::unique_ptr<WorkerPool> pool;  // created on first use (qsv_circuits_create, qsv_eval_batch)
    std::mutex pool_mu;

    // qsv_eval_coalesced: requests of concurrent callers waiting to be merged into one batch
    struct CoalesceRequest {
        int circuit_id = 0;
        const double* params = nullptr;
        int n_params = 0;
        double value = 0.0;
        int rc = QSV_OK;
        std::string err;
        bool done = false;
    };
    std::mutex cq_mu;
    std::condition_variable cq_cv;
    std::vector<CoalesceRequest*> cq;
    std::atomic<size_t> cq_count{0};   // = cq.size(), readable without the lock (the collecting caller spins on it)
    bool cq_collecting = false;        // some caller is collecting or evaluating a batch
    size_t cq_expected = 0;            // size of recent batches: how many callers to expect
    uint64_t cq_batches = 0;           // batches evaluated so far (diagnostic)

    // device memory
    DeviceBuffer d_arena;  // plans (uint32 words)
    size_t arena_used_words = 0;
    DeviceBuffer d_states;
    DeviceBuffer d_wtab;      // compact tables of pass 0 (plan.hpp COMPACT), one per state slot
    uint64_t wtab_stride = 0; // amplitudes per slot
    DeviceBuffer d_side;      // final states of the virtual circuits of split evaluations (split.hpp): two halves per slot
    uint64_t side_stride = 0; // amplitudes per slot
    int side_slots = 0;       // a split evaluation needs no state, so many more of them than `group` run side by side
    DeviceBuffer d_batch;     // [EvalDesc x B][parameter vectors]
    DeviceBuffer d_mats;      // per evaluation: gate matrices in schedule order + product-state factors
    int tiles_per_block = 1;        // pass 0 (and the only pass of a small circuit)
    int tiles_per_block_later = 1;  // passes 1.. (a multiple of tiles_per_block)
    DeviceBuffer d_partials;  // [B][blocks_per_state]
    DeviceBuffer d_out;       // [B]
    DeviceBuffer d_scratch;   // probabilities / converted state
    void* h_batch = nullptr;  // pinned
    size_t h_batch_bytes = 0;
    // The same bytes in DEVICE memory, written by the host directly over the PCIe BAR (large-BAR systems: every MI355X host):
    // what the kernels read -- descriptors and parameter vectors -- is then a local read instead of a trip over PCIe per
    // dependent load (scripts/ubench/bar_write.hip: 32 KiB written in 0.9 us; one wave reading them back: 28 us against 91
    // from pinned host memory).  batch_ship copies each push's ranges across and fences; kernels get these pointers.
    void* d_ship = nullptr;
    bool bar_ship = false;
    std::vector<char> ship_shadow;  // what d_ship's descriptor regions hold (host copy, for the compare)
    uint32_t* h_stage = nullptr;  // pinned staging buffer for plan uploads
    size_t h_stage_words = 0;
    double* h_out = nullptr;  // pinned
    bool repeat_device_descs = true;  // (QSV_REPEAT_DESCS=0: a repeated batch reads its descriptors from pinned memory again)
    const void* dev_params_checked = nullptr;  // the last qsv_eval_push_device pointer found to be this device's memory
    double* out_target = nullptr;  // qsv_eval_set_output: device memory the open batch's results go to instead of h_out
    bool async_pending = false;    // a batch ended without waiting (qsv_eval_end with a device output): the staging buffers
                                   // may still be read by its kernels
    void* h_samples = nullptr;  // pinned: sampled states (and their operator values) of one qsv_sample_batch call
    size_t h_samples_bytes = 0;
    size_t h_out_count = 0;

    // streaming evaluation (qsv_eval_begin / push / end)
    struct Batch {
        bool open = false;
        std::vector<Circuit*> circs;
        std::vector<uint32_t> param_base;  // per evaluation, in doubles
        std::vector<uint32_t> n_params;
        size_t desc_bytes = 0;
        size_t pushed = 0;                 // evaluations launched so far
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pass_events, exp_events;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> launch_events[3];  // per launch: [0] first pass, [1] later passes, [2] contraction
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        bool split_any = false; // some evaluation of the batch runs split: the descriptor array has a second region
        bool reduced = false;   // ... and those with a reduced form run it (side_form): laid out by the expectation route for its one-launch route
        std::vector<char> split;  // per evaluation
        bool cont_any = false;  // some evaluation continues a kept state (Circuit::prefix_id): a push puts those last
        size_t snap_n_cont = 0;
        std::vector<uint32_t> eval_at;  // descriptor position -> evaluation (a push puts its split evaluations first)
        int ways = 1;           // streams this batch cycles over
        unsigned used_mask = 0; // side streams (bit i = side_streams[i]) with work of this batch in flight
        bool aux_plain = false; // the batch's ordinary evaluations run on the auxiliary stream (eval_begin)
        bool chain_now = false; // this push: the split evaluations with launches of their own go to the chain stream (eval_push)
        bool chain_crossed = false; // some push of this batch put its chain on the other lane's stream (eval_push)
        bool sentinels = false; // the result buffer was filled with kResultSentinel before the first push (eval_begin)
        // the batch as qsv_eval_begin was called (kept for the next call's comparison), and what the last COMPLETED batch left
        // in place: valid while snap_epoch == the handle's epoch
        std::vector<int> cur_ids, snap_ids;
        std::vector<int64_t> cur_counts, snap_counts;
        uint64_t snap_epoch = 0;
        size_t snap_n_split = 0;
        int snap_ways = 0;         // `ways` of the push that laid the kept layout out and slotted its descriptors (eval_push)
        bool pinned_descs = false; // this push repeats that layout over fewer lanes: its kernels read the pinned descriptors (descs_base)
        bool have_ids = false;     // cur_ids / cur_counts describe THIS batch (it came through qsv_eval_begin)
        bool repeat = false;       // this batch reuses the previous batch's layout (descriptors as its one push left them)
        bool whole_push = false;   // this batch was pushed in one piece
        size_t aux_count = 0;   // ... how many of them have been pushed (their state slots cycle over the whole group)

        size_t n_pushes = 0;
        const double* dev_params = nullptr;  // this push's parameter values live in device memory (qsv_eval_push_device):
                                             // where evaluation 0's values would be -- descriptors index it like the staging buffer
        // The launches of the kept layout's one push, as that push made them (eval_push records, replay_push queues them again
        // for a batch that repeats): lives and dies with the kept layout -- dropped wherever a batch is laid out afresh
        // (batch_layout), and usable only while `epoch` is the handle's and the batch is a repeat (snap_epoch == epoch).
        struct LaunchEntry {
            enum Kind : uint8_t { Prepare, Pass, Reduce, Factor, FactorTerms, Contract, PauliGroups, PauliCombine } kind = Pass;
            int stream = -1;  // -1: the handle's own stream; i: side_streams[i]
            // Pass: the kernel's instantiation and launch shape
            int dtype = 0, r = 0, xmode = 0, threads = 0;
            dim3 grid;
            size_t lds = 0;
            PassArgs a{};  // Pass, Factor, FactorTerms, Contract: the argument struct by value
            // patched at every replay (see replay_push): offsets from the descriptor / result bases, -1 where the launch takes none
            int64_t host_evals_off = -1, result_off = -1;
            bool takes_params = false;
            // the other kinds' arguments: functions of the layout alone
            int n = 0, n2 = 0, n3 = 0;          // evaluations (Prepare, Reduce, Factor*, PauliGroups, PauliCombine) / first group, groups (PauliGroups) / most keys (Factor)
            uint32_t blocks = 0;                // Reduce: partial sums per evaluation; Contract: chunks
            const double* partials = nullptr;   // Reduce: where they are
            double* out = nullptr;              // Reduce: a device destination that is not the result buffer (d_out)
            const EvalDesc* evals = nullptr;    // Prepare: the device descriptors written; Reduce, PauliCombine: those read (may be null)
        };
        struct LaunchRecord {
            std::vector<LaunchEntry> entries;
            bool recording = false;  // a push is appending to it
            bool spoiled = false;    // ... and did something that is not a kernel launch on one of the handle's streams
            bool usable = false;     // the push made nothing but kernel launches, and ended well
            uint64_t epoch = 0;      // the handle's when the push ended
            int ways = 0;            // streams the batch cycled over (slots and launch groups follow it)
            bool no_direct_env = false;  // what single_workgroup_path found in the environment
            unsigned used_mask = 0;  // side streams the push left work on
            size_t aux_count = 0;    // ordinary evaluations it put on the auxiliary stream
            qsv_profile prof{};      // what the push added to the handle's counters (they are zero when a batch begins)
        } record;
    } batch;
    std::unique_lock<std::mutex> batch_lock;  // held from begin to end
    // qsv_cvar_device: its device_active for the duration of the call (run_group and batch_ship hand it to their launches) ...
    ActiveMask mask;
    const void* cvar_checked[3] = {nullptr, nullptr, nullptr};  // its values / output / mask pointers last found to be this device's memory
    // ... and the layout its last call left in the staging buffer (descriptors ordered and slotted, batch.eval_at / split /
    // param_base): valid while `epoch` is the handle's, for a call with the same circuits, row width and kind
    struct CvarSnap {
        uint64_t epoch = 0;
        std::vector<int> ids;
        int width = -1;
        bool sampled = false;
        size_t n_split = 0;
        std::vector<std::pair<size_t, size_t>> groups;
    } cvar_snap;

    // parameter-shift gradients (qsv_gradient_circuits / qsv_gradient_device)
    int grad_chunk = kGradientChunkRows;  // shifted evaluations per chunk (qsv_set_option "gradient_chunk")
    DeviceBuffer d_grad_tab;     // [GradRow x shifted][GradEntry x entries][int64 x (evaluations + 1)]
    DeviceBuffer d_grad_rows;    // one chunk's shifted rows; grows by doubling
    DeviceBuffer d_grad_values;  // every shifted evaluation's value
    DeviceBuffer d_grad_base;    // host form: the base rows
    DeviceBuffer d_grad_out;     // host form: the gradient rows
    void* h_grad_tab = nullptr;  // pinned: what d_grad_tab is copied from
    size_t h_grad_tab_bytes = 0;
    hipEvent_t ev_grad = nullptr;  // that copy is complete
    bool grad_copy_pending = false;
    const void* grad_checked[2] = {nullptr, nullptr};  // qsv_gradient_device's values / output last found to be this device's memory
    qsv_gradient_stats_t grad_stats{};
    // gradient plans (qsv_gradient_plan_create): a plan's tables in device memory of its own, and what a run needs of them on the host
    struct GradientPlan {
        std::vector<int> ids;
        int width = 0, out_width = 0;
        size_t chunk = 1;                // shifted evaluations per chunk, as "gradient_chunk" stood when the plan was made
        std::vector<GradRow> rows;       // the host's copy: which evaluation a shifted row belongs to
        size_t n_entries = 0;
        void* d_tab = nullptr;           // [GradRow x shifted][GradEntry x entries][int64 x (evaluations + 1)]
        qsv_gradient_plan_stats_t stats{};
    };
    std::unordered_map<int, GradientPlan> grad_plans;
    int next_grad_plan_id = 1;
    // The layout the last run of a ONE-chunk plan left in the staging buffer, as cvar_snap is qsv_cvar_device's: valid while `epoch`
    // is the handle's, for the next run of the same plan (expectation_to_device)
    struct PlanSnap {
        uint64_t epoch = 0;
        int plan_id = 0;
        size_t n_evals = 0;
    } plan_snap;
    // adjoint gradients (qsv_adjoint_gradient_circuits / qsv_adjoint_gradient_device; adjoint.hpp): lambda of one launch group's
    // states, the call's tables, the group's gate matrices and partial sums; the host form's points, rows and values
    DeviceBuffer d_adj_lambda, d_adj_tab, d_adj_mats, d_adj_partials, d_adj_epart, d_adj_base, d_adj_out, d_adj_values;
    const void* adj_checked[3] = {nullptr, nullptr, nullptr};  // qsv_adjoint_gradient_device's pointers last found to be this device's memory
    qsv_adjoint_stats_t adj_stats{};
    // deflated costs (qsv_deflated_gradient_circuits / qsv_deflated_gradient_device; deflation.hpp): one launch group's overlaps by
    // position | its partial tiles; the host form's energies | overlaps.  Counted with the adjoint scratch (adj_stats).
    DeviceBuffer d_defl, d_defl_out;
    const void* defl_checked[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // qsv_deflated_gradient_device's pointers
    // exact CVaR gradients (qsv_cvar_gradient_circuits / qsv_cvar_gradient_device; cvar_gradient.hpp): one launch group's (t, s) pairs by
    // position | its chunk masses.  The host form's thresholds are d_defl_out.  Counted with the adjoint scratch (adj_stats).
    DeviceBuffer d_cvar_grad;
    const void* cvar_grad_checked[4] = {nullptr, nullptr, nullptr, nullptr};  // qsv_cvar_gradient_device's pointers
    // folded-spectrum and variance costs (qsv_folded_gradient_circuits / qsv_folded_gradient_device; folded.hpp): one launch group's
    // (E, c) pairs by position | its shares of |r|^2, and -- an operator with x-mask groups, a gate to sweep -- the group's residuals.
    // The host form's energies are d_defl_out.  Counted with the adjoint scratch (adj_stats).
    DeviceBuffer d_fold, d_fold_r;
    const void* fold_checked[4] = {nullptr, nullptr, nullptr, nullptr};  // qsv_folded_gradient_device's pointers
    // the operator's moments (qsv_variance_circuits; moments.hpp): the call's (E, Var) pairs by position | one launch group's partials
    DeviceBuffer d_moments;
    // an observable set's second moments (qsv_observables_covariance; covariance.hpp): the call's values | covariances by position |
    // one launch group's partials
    DeviceBuffer d_cov;
    // overlaps against kept states (qsv_overlap_circuits; overlap.hpp): the call's S by position | its T by position | one launch
    // group's partial tiles
    DeviceBuffer d_overlap;
    // reduced density matrices (qsv_reduced_density_circuits; reduced_density.hpp): the call's subset table | its matrices by
    // position | one launch's partial tiles
    DeviceBuffer d_rdm;
    // operator-weighted reduced density matrices (qsv_operator_density_circuits; operator_density.hpp): the call's subset table | its
    // matrices by position | its values by position | one launch's partial tiles.  lambda = H_h psi of a launch group and the
    // operator kernel's shares of <H> are the adjoint sweep's d_adj_lambda and d_adj_epart.
    DeviceBuffer d_opdm;
    // the Fubini-Study metric (qsv_metric_circuits; metric.hpp): one launch group's psi buffers and derivative states | the call's
    // tables | the group's gate matrices | one Gram launch's partial tiles | the points | the call's matrices
    DeviceBuffer d_met_scratch, d_met_tab, d_met_mats, d_met_partials, d_met_base, d_met_out;
    int metric_scratch_mib = 8192;  // option "metric_scratch_mib": the bound of d_met_scratch
    qsv_metric_stats_t met_stats{};
    bool time_moments = false;  // option "time_moments": the device time of the two kernels goes to prof.expect_ms
    uint64_t host_waits = 0;  // times the host waited for a stream or an event (sync_streams and the few direct waits a batch can meet)

    // device-resident value caches (qsv_value_cache_create; value_cache.hpp)
    std::unordered_map<int, ValueCache> value_caches;
    int next_cache_id = 1;

    // profiling
    bool profiling = false;
    bool stamping = false;  // per-launch events are recorded (inside qsv_eval_push of a profiled batch only)
    qsv_profile prof{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
};

namespace {

int fail(qsv_t* h, int code, const std::string& msg) {
    if (h) {
        g_handle_error = msg;
        g_handle_error_owner = h;
    } else {
        g_create_error = msg;
    }
    return code;
}

inline hipStream_t ws(const qsv_t* h) { return h->work ? h->work : h->stream; }

#define QSV_HIP(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail((h), QSV_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

// QSV_HOST_TIMING: adds the time between its construction and its destruction to one of the handle's phase sums (a launch
// call's only inside qsv_eval_push, whose own sum is reported without them)
struct PhaseClock {
    using Timing = qsv_handle::HostTiming;
    double* acc = nullptr;
    std::chrono::steady_clock::time_point t0;
    PhaseClock(qsv_t* h, double Timing::*phase, bool in_push_only = false) {
        if (h->timing.on && (!in_push_only || h->timing.in_push)) {
            acc = &(h->timing.*phase);
            t0 = std::chrono::steady_clock::now();
        }
    }
    ~PhaseClock() {
        if (acc) *acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
};

// a kernel launch of the batch path: QSV_HIP, and timed as a launch call
#define QSV_LAUNCH(h, expr)                                                       \
    do {                                                                          \
        PhaseClock _launch_clock((h), &PhaseClock::Timing::launch_us, true);      \
        QSV_HIP((h), expr);                                                       \
    } while (0)

// ---- the launch record of a kept layout (qsv_handle::Batch::LaunchRecord) ---------------------------------
using LaunchEntry = qsv_handle::Batch::LaunchEntry;

// the push being recorded did something a replay cannot repeat by launching kernels (or launched where a record cannot say)
void record_spoil(qsv_t* h) {
    if (h->batch.record.recording) h->batch.record.spoiled = true;
}

// the entry of a launch on the stream of the push being issued; null when no push is being recorded
LaunchEntry* record_entry(qsv_t* h, LaunchEntry::Kind kind, hipStream_t st) {
    qsv_handle::Batch::LaunchRecord& rec = h->batch.record;
    if (!rec.recording) return nullptr;
    int index = -1;
    if (st != h->stream) {
        for (size_t i = 0; i < h->side_streams.size(); ++i)
            if (h->side_streams[i] == st) index = int(i);
        if (index < 0) rec.spoiled = true;
    }
    rec.entries.emplace_back();
    LaunchEntry& e = rec.entries.back();
    e.kind = kind;
    e.stream = index;
    return &e;
}

// Nothing on either stream may still be using a buffer that is about to be replaced.
hipError_t sync_streams(qsv_t* h) {
    h->host_waits += 1;
    hipError_t e = h->stream ? hipStreamSynchronize(h->stream) : hipSuccess;
    for (hipStream_t st : h->side_streams)
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

int ensure(qsv_t* h, DeviceBuffer& b, size_t bytes) {
    if (b.bytes >= bytes && b.ptr) return QSV_OK;
    if (b.ptr) {
        QSV_HIP(h, sync_streams(h));
        QSV_HIP(h, hipFree(b.ptr));
        b.ptr = nullptr;
        b.bytes = 0;
    }
    size_t want = std::max(bytes, size_t(256));
    QSV_HIP(h, hipMalloc(&b.ptr, want));
    b.bytes = want;
    return QSV_OK;
}

// ... and a reallocation counted where a call reports its own (qsv_gradient_stats, qsv_adjoint_stats)
int ensure_counted(qsv_t* h, DeviceBuffer& b, size_t bytes, int64_t& counter) {
    if (!(b.bytes >= bytes && b.ptr)) counter += 1;
    return ensure(h, b, bytes);
}
// A call's tables (adjoint_plan.hpp: TableBlob) into `b`, grown where it has to: one copy that waits.  TableBlob::at(b.ptr, offset)
// is a part in device memory.
int upload_blob(qsv_t* h, DeviceBuffer& b, const TableBlob& blob, int64_t& counter) {
    if (const int rc = ensure_counted(h, b, blob.bytes.size(), counter)) return rc;
    QSV_HIP(h, hipMemcpy(b.ptr, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice));
    return QSV_OK;
}

// ---- what the entry points have in common (the entry layer) ------------------------------------------------------
// Between qsv_eval_begin and qsv_eval_end the calling thread holds the handle's lock (batch_lock): an entry point that took it
// again from that thread would wait for itself, so it refuses.
int refuse_in_batch(qsv_t* h, const char* name) {
    return fail(h, QSV_E_STATE, std::string("a batch is open on this handle (") + name + " goes between batches)");
}

// The opening: the one way an entry point takes the handle.  A handle, no batch of the calling thread's open on it, its lock
// (held by `lock` until the caller returns) and, for a call that touches the device, its device.  The getters hand in a
// const handle: fail only writes thread-locals, and the lock is mutable.
int open_handle(const qsv_t* handle, const char* name, std::unique_lock<std::mutex>& lock, bool device) {
    qsv_t* h = const_cast<qsv_t*>(handle);
    if (!h) return QSV_E_ARG;
    if (h->batch_owner.load() == std::this_thread::get_id()) return refuse_in_batch(h, name);
    lock = std::unique_lock<std::mutex>(h->mu);
    if (device) QSV_HIP(h, hipSetDevice(h->device));
    return QSV_OK;
}
constexpr bool kHostOnly = false, kDevice = true;
#define QSV_OPEN(h, name, device)                                               \
    std::unique_lock<std::mutex> lock;                                          \
    if (const int _open_rc = open_handle((h), (name), lock, (device))) return _open_rc

// A batch that ended without waiting (async_pending) may still read or write the staging buffers and the scratch: whoever is
// about to write them waits for it first.
int wait_pending(qsv_t* h) {
    if (h->async_pending) {
        QSV_HIP(h, sync_streams(h));
        h->async_pending = false;
    }
    return QSV_OK;
}

// given[i] (null: not looked at) is memory of the handle's device.  A search hands over the same buffers call after call: the
// caller's cache remembers each, so that it is asked about once.
int check_device_pointers(qsv_t* h, const void* const* given, const char* const* names, const void** cache, int count) {
    for (int i = 0; i < count; ++i) {
        if (!given[i] || given[i] == cache[i]) continue;
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, given[i]) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != h->device) {
            (void)hipGetLastError();
            return fail(h, QSV_E_ARG, std::string(names[i]) + " is not memory of this handle's device");
        }
        cache[i] = given[i];
    }
    return QSV_OK;
}

int too_few_values(qsv_t* h, int need, int64_t got) {
    return fail(h, QSV_E_ARG, "circuit needs " + std::to_string(need) + " parameter values, got " + std::to_string(got));
}

// The consumers of whole final states are built up to 28 qubits: `message` is the caller's refusal as far as "... 28 qubits",
// `name_size` adds the handle's own size behind it.
int qubit_guard(qsv_t* h, const char* message, bool name_size = false) {
    if (h->n <= 28) return QSV_OK;
    return fail(h, QSV_E_UNSUPPORTED, name_size ? std::string(message) + ", this handle has " + std::to_string(h->n) : std::string(message));
}

// The kept states prefix_ids[0 .. n_states) as the overlap panels and the deflate kernel address them (n_states <= kOvlMaxStates).
int kept_refs(qsv_t* h, int n_states, const int* prefix_ids, OverlapRefs& refs) {
    for (int k = 0; k < n_states; ++k) {
        const auto it = h->prefixes.find(prefix_ids[k]);
        if (it == h->prefixes.end() || it->second.released) return fail(h, QSV_E_ARG, "unknown kept state " + std::to_string(prefix_ids[k]));
        refs.slot[k] = it->second.slot;
    }
    return QSV_OK;
}

// What evaluation e of a gradient-like call asks for: the parameters wrt[first .. first + count) of its circuit c, or, without
// wrt_offsets, all of them in their order.  Checked: the offsets do not fall, a row of out_width takes the count (`noun`: what
// the call's message counts), and every index names a parameter of c.
struct WrtRequest {
    int64_t first, count;
};
int wrt_request(qsv_t* h, const Circuit& c, int circuit_id, size_t e, const int64_t* wrt_offsets, const int32_t* wrt, int out_width,
                const char* noun, WrtRequest& out) {
    const int64_t first = wrt_offsets ? wrt_offsets[e] : 0, count = wrt_offsets ? wrt_offsets[e + 1] - first : int64_t(c.n_params);
    if (count < 0) return fail(h, QSV_E_ARG, "wrt_offsets must be non-decreasing");
    if (count > out_width)
        return fail(h, QSV_E_ARG, "out_width " + std::to_string(out_width) + " is too small for " + std::to_string(count) + " " + noun);
    if (count > 0 && wrt_offsets && !wrt) return fail(h, QSV_E_ARG, "wrt is null");
    for (int64_t j = 0; wrt_offsets && j < count; ++j)
        if (wrt[first + j] < 0 || wrt[first + j] >= c.n_params)
            return fail(h, QSV_E_ARG, "wrt index " + std::to_string(wrt[first + j]) + " is outside the " + std::to_string(c.n_params) +
                                          " parameters of circuit " + std::to_string(circuit_id));
    out = WrtRequest{first, count};
    return QSV_OK;
}

int validate_ops(qsv_t* h, int n, int n_ops, const qsv_op* ops, int n_params) {
    if (n_ops < 0 || (n_ops > 0 && !ops)) return fail(h, QSV_E_ARG, "ops is null");
    for (int i = 0; i < n_ops; ++i) {
        const qsv_op& o = ops[i];
        if (o.kind > QSV_OP_CU3) return fail(h, QSV_E_ARG, "unknown op kind at op " + std::to_string(i));
        if (o.target >= n) return fail(h, QSV_E_ARG, "target qubit out of range at op " + std::to_string(i));
        if (o.kind == QSV_OP_CU3 && (o.control >= n || o.control == o.target))
            return fail(h, QSV_E_ARG, "bad control qubit at op " + std::to_string(i));
        if (o.kind != QSV_OP_ID)
            for (int32_t p : {o.p_theta, o.p_phi, o.p_lambda})
                if (p >= n_params || p < -1)  // (below -1: the scheduler's own fixed matrices, split.hpp)
                    return fail(h, QSV_E_ARG, "parameter index out of range at op " + std::to_string(i));
    }
    return QSV_OK;
}

std::vector<GateIn> gates_of(const qsv_op* ops, int n_ops, std::vector<AngleSource>* angles) {
    std::vector<GateIn> gates;
    angles->clear();
    for (int i = 0; i < n_ops; ++i) {
        angles->push_back(AngleSource{ops[i].p_theta, ops[i].p_phi, ops[i].p_lambda, ops[i].theta, ops[i].phi,
                                      ops[i].lambda});
        if (ops[i].kind == QSV_OP_ID) continue;
        GateIn g;
        g.target = ops[i].target;
        g.control = ops[i].kind == QSV_OP_CU3 ? int(ops[i].control) : -1;
        g.op = i;
        gates.push_back(g);
    }
    return gates;
}

PlanConfig resolve_config(const qsv_plan_config* cfg, int dtype, int n_qubits) {
    PlanConfig pc;
    pc.amp_bytes = dtype == QSV_F64 ? 16 : 8;
    // Tile geometry by size (fp64; measured on MI355X with the EVQE benchmark family, scripts/geometry_sweep.sh): 16 amplitudes
    // per thread halve the per-amplitude cost of decoding the plan from n = 20 on, and 13 tile qubits save a pass
    // from n = 21 on (n = 24: 3 -> 2.25 passes on average, +33 % evaluations per second).
    // (single precision likewise since its round loop is generated assembly too, round 4: n = 20, L = 8 60 k -> 81 k evals/s with
    // 16 amplitudes per thread, n = 24 3.0 k -> 3.8 k with 13-qubit tiles, profiles/r04_fp32.txt)
    if (n_qubits >= 20) {
        pc.reg_bits = 4;
        pc.tile_bits = n_qubits >= 21 ? 13 : 12;
    }
    // Runs in memory.  The load and store layouts of a multi-gate pass keep only the lowest `lane_bits` tile qubits on the low
    // lanes (everything else goes where the first round's targets want it): a wave's access is 64 / 2^lane_bits separate runs
    // of 2^lane_bits amplitudes.  Two bits are 64-byte runs in double precision -- half an L2 line (128 bytes on this part) --
    // and 32-byte runs in single precision.  Measured in round 4 (profiles/r04_fp32.txt): with THREE the later pass of config
    // 5's genome goes from 0.55 to 0.68 of 8 TB/s at n = 28 (fp64) and from 0.36 to 0.57 (fp32), whole deep evaluations at
    // n = 26 / 28 gain 10 - 20 %; at n <= 24 in double precision the pass gains as much as the lost free qubit costs in
    // passes (n = 24: L = 8 +5 %, L = 4 -5 %).  So: three wherever the state is beyond the Infinity Cache, and in single
    // precision from 20 qubits on.
    if ((size_t(1) << n_qubits) * size_t(pc.amp_bytes) > (size_t(256) << 20) || (dtype != QSV_F64 && n_qubits >= 20))
        pc.low_bits = pc.lane_bits = 3;
    if (dtype != QSV_F64) pc.xmode = 0;  // fp32: one 8-byte complex element per LDS access
    if (const char* e = getenv("QSV_XMODE")) pc.xmode = atoi(e);
    if (const char* e = getenv("QSV_TILE_BITS")) pc.tile_bits = atoi(e);
    if (const char* e = getenv("QSV_REG_BITS")) pc.reg_bits = atoi(e);
    if (const char* e = getenv("QSV_LOW_BITS")) pc.low_bits = atoi(e);
    if (const char* e = getenv("QSV_LANE_BITS")) pc.lane_bits = atoi(e);
    if (const char* e = getenv("QSV_FOLD")) pc.fold = atoi(e) != 0;
    if (const char* e = getenv("QSV_COMPACT")) pc.compact = atoi(e) != 0;
    if (const char* e = getenv("QSV_SWAPS")) pc.swaps = atoi(e) != 0;
    // multiplexed gates (plan.hpp FUSION): the assembly round loops of both precisions take their entries at full speed (fp32
    // since round 4: RoundLoopF32's one body serves products of matrices as well)
    pc.fuse = true;
    if (const char* e = getenv("QSV_FUSE")) pc.fuse = atoi(e) != 0;
    if (const char* e = getenv("QSV_RETRIES")) pc.retries = atoi(e);
    if (cfg) {
        if (cfg->tile_bits > 0) pc.tile_bits = cfg->tile_bits;
        if (cfg->reg_bits > 0) pc.reg_bits = cfg->reg_bits;
        if (cfg->low_bits > 0) pc.low_bits = cfg->low_bits;
        if (cfg->exchange > 0) pc.xmode = cfg->exchange - 1;
    }
    if (dtype != QSV_F64 && pc.xmode != 0) pc.xmode = 0;
    pc.elem_bytes = (dtype == QSV_F64 && pc.xmode == 0) ? 16 : 8;
    return pc;
}

// The ordinary (multi-pass) plan of a circuit.  With THREE low lane bits instead of two a pass over a state runs faster (128-byte
// runs, resolve_config) but has one free tile qubit fewer, which costs some circuits a pass: where the handle's default is two
// (double precision up to 24 qubits) the circuit is scheduled both ways and takes three when that costs no pass -- three in four
// deep individuals (n = 24, L = 8: 24 of 32; L = 4: 31 of 32).  QSV_LOW_BITS / QSV_LANE_BITS / QSV_AUTO_LANE=0 switch it off.
CircuitPlan build_ordinary_plan(const qsv_t* h, const std::vector<GateIn>& gates, const std::vector<AngleSource>& angles, const PlanConfig& pc) {
    CircuitPlan two = build_plan(h->n, gates, angles, pc);
    static const bool automatic = !getenv("QSV_LOW_BITS") && !getenv("QSV_LANE_BITS") && !(getenv("QSV_AUTO_LANE") && atoi(getenv("QSV_AUTO_LANE")) == 0);
    if (!automatic || pc.low_bits != 2 || pc.lane_bits != 2 || h->geo.blocks_per_state < 2 || two.stats.n_passes < 1) return two;
    PlanConfig wide = pc;
    wide.low_bits = wide.lane_bits = 3;
    try {
        CircuitPlan three = build_plan(h->n, gates, angles, wide);
        if (three.stats.n_passes <= two.stats.n_passes) return three;
    } catch (const std::exception&) {
        // (the narrower plan stands)
    }
    return two;
}

// The reduced form of a circuit whose full form takes the one-launch route (Circuit::reduced): a side with final controls is
// planned anew without their keys -- one tile, one pass, the full form's amplitudes per thread, or it keeps the full form --
// and a copy of the split block says which keys are whose (kernels.hpp kSplitReduced).  sx: the side that is X in the block.
// The tail deals its Gram waves out over the 2^F blocks of x (kernels.hip fused_factor_tail): at least one wave per block and 64
// x per block.  Appends to out->plan.words.
void plan_reduced_sides(const qsv_t* h, const PlanConfig& pc, const SplitCircuits& sc, int sx, Circuit* out) {
    const SplitInfo& full = out->split;
    const ReducedSplit rs = reduce_final_controls(sc);
    if (!rs.any || sc.n_keys > 3) return;
    SplitInfo red = full;
    std::vector<uint32_t>& w = out->plan.words;
    const size_t words_before = w.size();
    const int side_tile = std::max(h->geo.k, std::min(h->geo.r + 9, int(kMaxTileBits)));
    uint32_t word[2] = {0, 0}, slots[2][2] = {{0, 0}, {0, 0}};
    bool any = false;
    for (int s = 0; s < 2; ++s) {
        const int xy = s == sx ? 0 : 1;
        out->reduced_mask[xy] = uint32_t(sc.mask[s]);
        out->reduced_top[xy] = 0;
        if (!rs.final_keys[s]) continue;
        const int n_final = __builtin_popcount(rs.final_keys[s]), n_sim = __builtin_popcount(rs.simulated_keys[s]), nv = rs.n_virtual[s];
        PlanConfig side = pc;
        side.reg_bits = full.side_r;
        side.compact = false;
        side.tile_bits = full.side_r == 3 ? std::min(nv, 12) : std::min(nv, side_tile);
        side.lane_bits = 0;  // (one tile, synthesised, its state read back by its own workgroup only: build_circuit)
        if (nv > side.tile_bits || side.tile_bits <= side.reg_bits) continue;
        const int t = side.tile_bits - side.reg_bits, gram_waves = t >= 9 ? 8 : 4;
        if ((1 << n_final) > gram_waves || sc.n_side[s] - n_final < 6) continue;
        const CircuitPlan p = build_plan(nv, rs.gates[s], rs.angles[s], side);
        if (p.stats.n_passes != 1) continue;
        red.stats[s] = p.stats;
        red.t[s] = t;
        red.outer[s] = 0;
        red.tile_bits[s] = side.tile_bits;
        red.n_virtual[s] = nv;
        red.off_side[s] = uint32_t(w.size());
        w.insert(w.end(), p.words.begin(), p.words.end());
        word[xy] = uint32_t(n_final) | uint32_t(n_sim) << 2;
        int row = 0;  // (row bits: the final controls in key order, then the simulated keys)
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < sc.n_keys; ++j)
                if (((rs.final_keys[s] >> j) & 1u) == uint32_t(pass == 0)) word[xy] |= uint32_t(j) << (4 + 2 * row++);
        std::vector<int> qubit;  // the register's qubit of each local qubit of the full form
        for (int q = 0; q < h->n; ++q)
            if (sc.mask[s] >> q & 1u) qubit.push_back(q);
        for (int pos = 0; pos < sc.n_side[s]; ++pos) slots[xy][pos >> 3] |= uint32_t(rs.qubit_of[s][size_t(pos)]) << (4 * (pos & 7));
        uint32_t top = uint32_t(n_final), low_mask = uint32_t(sc.mask[s]);
        for (int f = 0; f < n_final; ++f) {
            const int q = qubit[size_t(rs.qubit_of[s][size_t(sc.n_side[s] - n_final + f)])];
            top |= uint32_t(q) << (2 + 5 * f);
            low_mask &= ~(1u << q);
        }
        out->reduced_mask[xy] = low_mask;
        out->reduced_top[xy] = top;
        any = true;
    }
    if (!any) {
        w.resize(words_before);
        return;
    }
    // (half sides: the thirteen-qubit sides that keep the full form, under the full form's rule)
    red.halves = full.halves && ((word[sx == 0 ? 0 : 1] == 0 && full.n_virtual[0] == kFusedLdsRowsBits) ||
                                 (word[sx == 1 ? 0 : 1] == 0 && full.n_virtual[1] == kFusedLdsRowsBits));
    const std::vector<uint32_t> block(w.begin() + long(full.off_block), w.begin() + long(full.off_block) + long(kSplitBlockWords));
    red.off_block = uint32_t(w.size());
    w.insert(w.end(), block.begin(), block.end());
    uint32_t* blk = w.data() + red.off_block;
    for (int xy = 0; xy < 2; ++xy) {
        blk[kSplitReduced + xy] = word[xy];
        blk[kSplitReducedSlots + 2 * xy] = slots[xy][0];
        blk[kSplitReducedSlots + 2 * xy + 1] = slots[xy][1];
    }
    red.ok = true;
    out->reduced = red;
    if (getenv("QSV_SPLIT_DEBUG"))
        fprintf(stderr, "split: reduced virtual %d/%d (full %d/%d) halves %d\n", red.n_virtual[0], red.n_virtual[1], full.n_virtual[0],
                full.n_virtual[1], int(red.halves));
}

// Validate an op list and schedule it.  Touches only immutable parts of the handle (n, cfg), so it needs no lock and
// several threads may build plans at the same time.
int build_circuit(qsv_t* h, int n_ops, const qsv_op* ops, int n_params, bool fold, Circuit* out, std::string* err) {
    std::string local;
    {
        // validate_ops reports through fail(): keep its text
        int rc = validate_ops(h, h->n, n_ops, ops, n_params);
        if (rc) {
            if (err) *err = g_handle_error;
            return rc;
        }
    }
    out->n_params = n_params;
    out->ops.assign(ops, ops + n_ops);
    out->grad_terms.assign(size_t(n_params), 0);
    (void)gradient_plan(n_ops, ops, n_params, out->grad_terms.data());
    std::vector<AngleSource> angles;
    std::vector<GateIn> gates = gates_of(ops, n_ops, &angles);
    out->n_gates = int(gates.size());
    out->fold = fold;
    try {
        PlanConfig pc = h->cfg;
        pc.fold = pc.fold && fold;
        // (with QSV_FACTOR=0 not under a general operator: every evaluation then needs the state, i.e. the ordinary plan; a
        // circuit registered now and evaluated under a diagonal operator later simply takes the ordinary path)
        const bool state_needed = h->n_terms > 0 && !h->diagonal && !h->factor_enabled;
        if (h->split_enabled && !state_needed && pc.fold && h->n > h->geo.k && h->n <= 28) {  // (28: the contraction's 32-bit byte offsets into D)
            // a virtual circuit may be a few qubits larger than a tile (it then takes the pass kernel a few passes over up
            // to sixteen tiles: nothing next to the 2^n indices of the contraction)
            // ... but one tile each is what to look for first: no second pass, one workgroup per virtual circuit
            // (with 16 amplitudes per thread a side's tile may be one qubit larger than the handle's, below: sides that
            // fit THAT are the second choice)
            const int side_tile = std::max(h->geo.k, std::min(h->geo.r + 9, int(kMaxTileBits)));
            std::vector<int> limits{h->geo.k};
            if (side_tile > h->geo.k && side_tile < h->n) limits.push_back(side_tile);
            // (every size up to tile + 4 is a stage of its own since round 4: the first limit that has a partition wins, and with
            // the stages two qubits apart config 5's genome -- 14 + 14 qubits and two keys under limit 16 -- was taken as 13 + 15
            // under limit 17 on handles with 13-qubit tiles, a quarter more rows for the term kernel)
            for (int extra = 1; extra <= kSideExtraBits; ++extra) {
                const int limit = std::min(h->geo.k + extra, h->n - 1);
                if (limit > limits.back()) limits.push_back(limit);
            }
            SplitCircuits sc = find_split(h->n, gates, angles, limits, h->split_max_keys);
            if (sc.ok && std::max(sc.n_side[0], sc.n_side[1]) > kSideMaxOwnBits) sc.ok = false;
            if (sc.ok) {
                SplitInfo& sp = out->split;
                std::vector<uint32_t>& w = out->plan.words;
                bool fits = true;
                // The one-launch route's sides at 20 qubits, where a gate phase is what ONE WAVE takes to issue a gate over its own
                // amplitudes (HISTORY round 4, item 14): planned with eight amplitudes per thread instead of sixteen -- twice the waves
                // -- if both are at most twelve virtual qubits (one tile of 512 threads) and stay one pass; three keys and thirteen
                // virtual qubits a side: over 12-qubit tiles the scheduler leaves a qubit that is never a target outside the tile --
                // a key qubit; if that is the LAST one on both sides and one pass does, each side runs as two workgroups
                // (kEvalHalves).  Each form is tried and kept only if it holds; else the handle's own geometry, as before.
                const bool r3_handle = h->sides_r3 && h->dtype == QSV_F64 && h->geo.k == 12 && h->geo.r == 4 && sc.n_keys <= 3;
                // (half sides: every thirteen-qubit side of the circuit, if each leaves its LAST key qubit outside the tile)
                bool try_halves = r3_handle && sc.n_keys >= 1 && std::max(sc.n_side[0], sc.n_side[1]) + sc.n_keys == kFusedLdsRowsBits &&
                                  !getenv("QSV_NO_HALF_SIDES");  // (tests: the swept form, which a plan that keeps its last key inside the tile falls back to)
                // (thirteen virtual qubits otherwise: two 12-qubit tiles swept by the side's one workgroup -- as long as there is a key
                // qubit to leave outside the tile and one pass does)
                const int most_virtual = std::max(sc.n_side[0], sc.n_side[1]) + sc.n_keys;
                bool try_r3 = try_halves || (r3_handle && (most_virtual <= 12 || (most_virtual == 13 && sc.n_keys >= 1)));
                const size_t words_before = w.size();
                for (bool planned = false; !planned;) {  // (at most three times: half sides, swept tiles, the handle's own geometry)
                planned = true;
                for (int s = 0; s < 2 && fits && planned; ++s) {
                    PlanConfig side = pc;
                    sp.n_virtual[s] = sc.n_side[s] + sc.n_keys;
                    // (a virtual circuit one qubit larger than the handle's tile still fits ONE workgroup when that may have
                    // 512 threads: n = 20 keeps 12-qubit tiles of 256 threads for its states, but a three-key circuit's
                    // 13-qubit sides then stay one tile and one pass -- and with that in the one-launch path, kEvalFused)
                    side.tile_bits = std::min(sp.n_virtual[s], side_tile);
                    side.reg_bits = try_r3 ? 3 : h->geo.r;
                    side.compact = false;  // (the compact-table buffer is where a side's state lives)
                    fits = side.tile_bits > side.reg_bits;
                    if (!fits) break;
                    // A side of ONE tile is synthesised, not loaded, and its final state goes to LDS or to a small table that only
                    // its own workgroup reads back: no layout of it has to keep the low qubits on the low lanes -- the first round
                    // may target them, and the swaps that brought them home at the end (up to four of a side's ten) are not made
                    // (a zero-key circuit of the benchmark alone: 34.1 -> 32.5 us).
                    if (sp.n_virtual[s] <= side.tile_bits) side.lane_bits = 0;
                    if (try_halves && sp.n_virtual[s] == kFusedLdsRowsBits) {  // (the same goes for a half side: its state stays in LDS)
                        side.tile_bits = 12;
                        side.lane_bits = 0;
                    } else if (try_r3) {
                        side.tile_bits = std::min(sp.n_virtual[s], 12);
                    }
                    if (const char* env = getenv("QSV_SIDE_LANE_BITS")) side.lane_bits = atoi(env);  // (measurements)
                    const CircuitPlan p = build_plan(sp.n_virtual[s], sc.gates[s], sc.angles[s], side);
                    sp.stats[s] = p.stats;
                    sp.t[s] = side.tile_bits - side.reg_bits;
                    sp.outer[s] = sp.n_virtual[s] - side.tile_bits;
                    sp.tile_bits[s] = side.tile_bits;
                    sp.off_side[s] = uint32_t(w.size());
                    w.insert(w.end(), p.words.begin(), p.words.end());
                    if (try_r3) {
                        bool ok = p.stats.n_passes == 1;
                        if (ok && try_halves && sp.n_virtual[s] == kFusedLdsRowsBits) {  // (the tile's qubits are 0 .. 11: the last key qubit, 12, is the tile number)
                            const uint32_t* c0 = p.words.data();
                            const uint32_t* p0 = c0 + c0[kCircuitHeaderWords];
                            bool last_outside = true;
                            for (uint32_t j = 0; j < 12 && last_outside; ++j) last_outside = p0[kPassHeaderWords + j] != uint32_t(kFusedLdsRowsBits - 1);
                            if (!last_outside) {  // (two tiles swept by the side's one workgroup, then: planned anew with that form's lanes)
                                try_halves = false;
                                planned = false;
                            }
                        }
                        if (!ok) {  // (as before: the handle's geometry, one tile)
                            try_halves = try_r3 = false;
                            planned = false;
                        }
                        if (!planned) w.resize(words_before);
                    }
                }
                }
                sp.halves = fits && try_halves;
                sp.side_r = try_r3 ? 3 : h->geo.r;
                // the contraction kernel's view of the circuit (kernels.hpp, split block): ready-made pieces of the two
                // table indices for the lanes, the wave index, a thread's own five bits and the chunk number
                const int wave_bits = h->geo.t > 6 ? h->geo.t - 6 : 0;
                const int loop0 = 6 + wave_bits, chunk0 = loop0 + kSplitLoopBits;
                fits = fits && h->n >= chunk0 && h->n - chunk0 <= 14;
                if (fits) {
                    int own_a = 0;  // how many of a thread's own bits belong to side A
                    for (int b = 0; b < kSplitLoopBits; ++b) own_a += int(sc.mask[0] >> (loop0 + b) & 1u);
                    const bool swap_xy = own_a > kSplitMaxLoopX;  // X = the side with fewer of them
                    const int sx = swap_xy ? 1 : 0;
                    const int loop_x = swap_xy ? kSplitLoopBits - own_a : own_a;
                    // bit of index position p in the table index of the side it belongs to
                    std::vector<uint32_t> colx(size_t(h->n), 0), coly(size_t(h->n), 0);
                    {
                        int cx_ = 0, cy_ = 0;
                        for (int q = 0; q < h->n; ++q) {
                            if (sc.mask[sx] >> q & 1u)
                                colx[size_t(q)] = 1u << cx_++;
                            else
                                coly[size_t(q)] = 1u << cy_++;
                        }
                    }
                    sp.off_block = uint32_t(w.size());
                    w.resize(w.size() + kSplitBlockWords, 0);
                    uint32_t* blk = w.data() + sp.off_block;
                    blk[0] = uint32_t(sc.n_keys);
                    blk[1] = uint32_t(sc.n_side[sx]);
                    blk[2] = uint32_t(sc.n_side[1 - sx]);
                    blk[kSplitFlags] = (swap_xy ? kSplitSwapXY : 0u) | uint32_t(loop_x) << 8;
                    blk[kSplitMaskX] = uint32_t(sc.mask[sx]);
                    blk[kSplitMaskY] = uint32_t(sc.mask[1 - sx]);
                    blk[kSplitSideDiag] = blk[kSplitSideDiag + 1] = kNoSideDiag;  // (upload_plans names the tables)
                    {
                        int at = 0;
                        for (int which = 0; which < 2; ++which)
                            for (int b = 0; b < kSplitLoopBits; ++b) {
                                const int q = loop0 + b;
                                const bool is_x = sc.mask[sx] >> q & 1u;
                                if (is_x != (which == 0)) continue;
                                blk[kSplitLoopCols + at] = is_x ? colx[size_t(q)] : coly[size_t(q)];
                                blk[kSplitLoopPos + at] = 1u << q;
                                ++at;
                            }
                    }
                    // (entry v of a table = entry v without its lowest set bit | that bit's own pieces: one step per entry)
                    auto fill = [&](uint32_t* table, uint32_t entries, int first_bit) {
                        table[0] = table[1] = 0;
                        for (uint32_t v = 1; v < entries; ++v) {
                            const uint32_t low = v & (0u - v), rest = v ^ low;
                            const int q = first_bit + __builtin_ctz(low);
                            table[2 * v] = table[2 * rest] | (q < h->n ? colx[size_t(q)] : 0u);
                            table[2 * v + 1] = table[2 * rest + 1] | (q < h->n ? coly[size_t(q)] : 0u);
                        }
                    };
                    fill(blk + kSplitLaneTable, 64, 0);
                    fill(blk + kSplitWaveTable, 1u << wave_bits, 6);
                    fill(blk + kSplitChunkLow, 128, chunk0);
                    fill(blk + kSplitChunkHigh, 128, chunk0 + 7);
                    sp.n_keys = sc.n_keys;
                    sp.ok = true;
                    // (the one-launch path exists in the 16-amplitudes-per-thread instantiation: its 128 registers hold the
                    // Gram matrices' accumulators, the 80 of the 8-amplitude one do not)
                    // (a side of several tiles is swept by its ONE workgroup, tile after tile, as long as it is one pass)
                    // A property of the circuit and the handle, never of the batch: the two routes add in different orders.
                    // Measured (profiles/r03_fused_factor.txt): the one-launch route wins where a side's Gram matrices are a
                    // few blocks per wave -- 20-qubit registers, every population size -- and loses from 22 qubits on, where
                    // a side's table is 2^11 .. 2^13 rows for the four to eight waves of its one workgroup.
                    sp.fused = h->geo.r == 4 && h->geo.k == 12 && sp.n_keys <= 3 && ((sp.outer[0] == 0 && sp.outer[1] == 0) || sp.halves || (sp.side_r == 3 && sp.outer[0] <= 1 && sp.outer[1] <= 1)) &&
                               sp.stats[0].n_passes == 1 && sp.stats[1].n_passes == 1;
                    if (const char* env = getenv("QSV_FUSED_MAX_KEYS")) sp.fused = sp.fused && sp.n_keys <= atoi(env);  // (measurements)
                    if (getenv("QSV_SPLIT_DEBUG"))
                        fprintf(stderr, "split: keys %d sides %d+%d virtual %d/%d tiles 2^%d/2^%d passes %d/%d fused %d\n", sp.n_keys, sc.n_side[0],
                                sc.n_side[1], sp.n_virtual[0], sp.n_virtual[1], sp.outer[0], sp.outer[1], sp.stats[0].n_passes,
                                sp.stats[1].n_passes, int(sp.fused));
                    // (`blk` is not used below: the words may move)
                    if (sp.fused && h->final_controls) plan_reduced_sides(h, pc, sc, sx, out);
                } else {
                    w.resize(sp.off_side[0] ? sp.off_side[0] : w.size());
                    sp = SplitInfo{};
                }
            }
        }
        if (out->split.ok) {
            out->gates = std::move(gates);
            out->angles = std::move(angles);
        } else {
            const CircuitPlan p = build_ordinary_plan(h, gates, angles, pc);
            out->off_plan = uint32_t(out->plan.words.size());
            out->plan.words.insert(out->plan.words.end(), p.words.begin(), p.words.end());
            out->plan.stats = p.stats;
            out->has_plan = true;
        }
    } catch (const std::exception& e) {
        if (err) *err = std::string("plan: ") + e.what();
        return QSV_E_ARG;
    }
    return QSV_OK;
}

// The ordinary plan of a circuit registered in split form, on first need (caller holds the handle).
int ensure_plan(qsv_t* h, Circuit& c) {
    if (c.has_plan) return QSV_OK;
    try {
        PlanConfig pc = h->cfg;
        pc.fold = pc.fold && c.fold;
        const CircuitPlan p = build_ordinary_plan(h, c.gates, c.angles, pc);
        c.off_plan = uint32_t(c.plan.words.size());
        c.plan.words.insert(c.plan.words.end(), p.words.begin(), p.words.end());
        c.plan.stats = p.stats;
    } catch (const std::exception& e) {
        return fail(h, QSV_E_ARG, std::string("plan: ") + e.what());
    }
    c.has_plan = true;
    c.uploaded = false;  // (the arena copy, if any, lacks the new words)
    c.gates.clear();
    c.gates.shrink_to_fit();
    c.angles.clear();
    c.angles.shrink_to_fit();
    return QSV_OK;
}

// Schedule `count` structures, in parallel when there are several.  build(i) fills circuits[i]; the first failure is
// reported.  Needs no handle lock (build_circuit reads only immutable parts of the handle).
struct BuiltCircuit {
    Circuit circuit;
    std::string err;
    int rc = QSV_OK;
};
void build_many(qsv_t* h, size_t count, const std::function<void(size_t, BuiltCircuit&)>& build, std::vector<BuiltCircuit>& out) {
    out.resize(count);
    if (count < 4) {
        for (size_t i = 0; i < count; ++i) build(i, out[i]);
        return;
    }
    WorkerPool* pool;
    {
        std::lock_guard<std::mutex> lock(h->pool_mu);
        if (!h->pool) {
            unsigned hw = std::max(2u, std::min(16u, std::thread::hardware_concurrency()));
            if (const char* env = getenv("QSV_BUILD_THREADS")) hw = std::max(2u, std::min(64u, unsigned(atoi(env))));
            h->pool.reset(new WorkerPool(hw - 1));
        }
        pool = h->pool.get();
    }
    // one job at a time per pool: callers on several threads take turns
    static std::mutex job_mu;
    std::lock_guard<std::mutex> job(job_mu);
    pool->run(count, [&](size_t i) { build(i, out[i]); });
}

// a circuit that continued kept state `id` is gone (caller holds h->mu)
void prefix_unref(qsv_t* h, int id) {
    auto it = h->prefixes.find(id);
    if (it == h->prefixes.end()) return;
    if (--it->second.refs <= 0 && it->second.released) {
        h->prefix_free.push_back(it->second.slot);
        h->prefixes.erase(it);
    }
}

// (caller holds h->mu)
int insert_circuit(qsv_t* h, Circuit&& c) {
    const int id = h->next_circuit_id++;
    h->circuits.emplace(id, std::move(c));
    return id;
}

int register_circuit(qsv_t* h, int n_ops, const qsv_op* ops, int n_params, int* out_id, bool fold = true) {
    Circuit c;
    std::string err;
    int rc = build_circuit(h, n_ops, ops, n_params, fold, &c, &err);
    if (rc) return fail(h, rc, err);
    *out_id = insert_circuit(h, std::move(c));
    return QSV_OK;
}

// Make the plans of `circs` resident in the device arena.  New plans are staged back to back in one pinned host buffer
// and shipped with ONE copy per batch (a population of fresh structures used to cost one copy + one stream
// synchronisation per circuit).  When the arena is full it is rebuilt from the circuits that are still registered: the
// space of destroyed circuits is reclaimed, and the arena only grows when the live plans really need more room.
int upload_plans(qsv_t* h, const std::vector<Circuit*>& circs) {
    std::vector<Circuit*> fresh;
    size_t need = 0, need_d = 0;
    // (doubles of the two sides' own tables of D: split circuits whose expectation comes from Gram sums -- a quadratic diagonal operator)
    auto side_diag_doubles = [&](const Circuit* c) -> size_t {
        if (!h->d_diag.ptr || !c->split.ok || !(h->diagonal && h->quadratic && h->d_quad.ptr)) return 0;
        const uint32_t* blk = c->plan.words.data() + c->split.off_block;
        // (a reduced form's block names tables of its own, whatever the option says: a reduced side's table is in the order of ITS
        // qubits, which no mask describes -- the same values of D either way, so the option still changes no bit)
        return ((size_t(1) << blk[1]) + (size_t(1) << blk[2])) * ((h->side_diag ? 1 : 0) + (c->reduced.ok ? 1 : 0));
    };
    for (Circuit* c : circs)
        if (!c->uploaded && !c->staged) {
            c->staged = true;
            fresh.push_back(c);
            need += c->plan.words.size();
            need_d += side_diag_doubles(c);
        }
    for (Circuit* c : fresh) c->staged = false;
    if (fresh.empty()) return QSV_OK;
    const size_t cap = h->d_arena.bytes / 4;
    const bool tables_full = h->sdiag_used + need_d > h->d_sdiag.bytes / 8;
    if (h->arena_used_words + need > cap || tables_full) {
        // rebuild: everything still registered that is part of this batch goes in again; plans of other live circuits
        // are re-uploaded when they are next used
        QSV_HIP(h, sync_streams(h));
        for (auto& kv : h->circuits) kv.second.uploaded = false;
        fresh.clear();
        need = need_d = 0;
        for (Circuit* c : circs)
            if (!c->staged) {
                c->staged = true;
                fresh.push_back(c);
                need += c->plan.words.size();
                need_d += side_diag_doubles(c);
            }
        for (Circuit* c : fresh) c->staged = false;
        h->arena_used_words = 0;
        h->sdiag_used = 0;
        if (need_d > h->d_sdiag.bytes / 8 || (tables_full && h->d_sdiag.bytes < (size_t(256) << 20))) {
            // (it was full, or never there: twice the room up to 256 MiB, so that a run that keeps registering structures -- an
            // EVQE run does, every generation -- comes here, and uploads everything again, ever more rarely)
            const size_t new_doubles = std::max(std::max(need_d * 2, h->d_sdiag.bytes / 4), size_t(1) << 19);
            if (h->d_sdiag.ptr) QSV_HIP(h, hipFree(h->d_sdiag.ptr));
            h->d_sdiag = DeviceBuffer{};
            QSV_HIP(h, hipMalloc(&h->d_sdiag.ptr, new_doubles * 8));
            h->d_sdiag.bytes = new_doubles * 8;
        }
        if (getenv("QSV_ARENA_DEBUG"))
            fprintf(stderr, "plan arena: rebuilt for a batch of %zu plans, %zu words of %zu%s\n", fresh.size(), need, cap, need > cap ? " (grows)" : "");
        if (need > cap) {
            const size_t new_cap = std::max(need * 2, size_t(1) << 20);
            if (h->d_arena.ptr) QSV_HIP(h, hipFree(h->d_arena.ptr));
            h->d_arena = DeviceBuffer{};
            QSV_HIP(h, hipMalloc(&h->d_arena.ptr, new_cap * 4));
            h->d_arena.bytes = new_cap * 4;
        }
    }
    if (h->h_stage_words < need) {
        if (h->h_stage) {
            QSV_HIP(h, sync_streams(h));
            QSV_HIP(h, hipHostFree(h->h_stage));
            h->h_stage = nullptr;
            h->h_stage_words = 0;
        }
        const size_t want = std::max(need * 2, size_t(1) << 16);
        QSV_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_stage), want * 4, hipHostMallocDefault));
        h->h_stage_words = want;
    } else {
        // the previous batch's copy out of the staging buffer must be complete before it is overwritten
        h->host_waits += 1;
        QSV_HIP(h, hipStreamSynchronize(h->stream));
    }
    size_t cur = 0;
    std::vector<SideDiagJob> jobs;
    for (Circuit* c : fresh) {
        if (c->split.ok) {
            // the sides' own tables of D: named in the split block, filled behind the copy below
            uint32_t* blk = c->plan.words.data() + c->split.off_block;
            blk[kSplitSideDiag] = blk[kSplitSideDiag + 1] = kNoSideDiag;
            if (h->side_diag && side_diag_doubles(c))
                for (uint32_t xy = 0; xy < 2; ++xy) {
                    blk[kSplitSideDiag + xy] = uint32_t(h->sdiag_used);
                    jobs.push_back(SideDiagJob{uint32_t(h->sdiag_used), blk[kSplitMaskX + xy], blk[1 + xy]});
                    h->sdiag_used += size_t(1) << blk[1 + xy];
                }
            if (c->reduced.ok) {
                uint32_t* rblk = c->plan.words.data() + c->reduced.off_block;
                rblk[kSplitSideDiag] = rblk[kSplitSideDiag + 1] = kNoSideDiag;
                if (side_diag_doubles(c))
                    for (uint32_t xy = 0; xy < 2; ++xy) {
                        rblk[kSplitSideDiag + xy] = uint32_t(h->sdiag_used);
                        jobs.push_back(SideDiagJob{uint32_t(h->sdiag_used), c->reduced_mask[xy], rblk[1 + xy], c->reduced_top[xy]});
                        h->sdiag_used += size_t(1) << rblk[1 + xy];
                    }
            }
        }
        std::memcpy(h->h_stage + cur, c->plan.words.data(), c->plan.words.size() * 4);
        c->plan_base = uint32_t(h->arena_used_words + cur);
        cur += c->plan.words.size();
        c->uploaded = true;
    }
    QSV_HIP(h, hipMemcpyAsync(static_cast<uint32_t*>(h->d_arena.ptr) + h->arena_used_words, h->h_stage, need * 4,
                              hipMemcpyHostToDevice, h->stream));
    h->arena_used_words += need;
    if (getenv("QSV_ARENA_DEBUG"))
        fprintf(stderr, "plan arena: %zu fresh plans, %zu side tables of D (%zu doubles used of %zu), diag %p\n", fresh.size(), jobs.size(), h->sdiag_used,
                h->d_sdiag.bytes / 8, h->d_diag.ptr);
    for (size_t first = 0; first < jobs.size(); first += size_t(kSideDiagJobsPerLaunch)) {
        SideDiagJobs batch{};
        const int n_jobs = int(std::min(jobs.size() - first, size_t(kSideDiagJobsPerLaunch)));
        std::copy(jobs.begin() + long(first), jobs.begin() + long(first) + n_jobs, batch.job);
        QSV_HIP(h, launch_side_diag(static_cast<const double*>(h->d_diag.ptr), static_cast<double*>(h->d_sdiag.ptr), batch, n_jobs, h->stream));
    }
    // launches on the second stream read the arena too: they wait for this copy
    if (!h->side_streams.empty()) {
        QSV_HIP(h, hipEventRecord(h->ev_join, h->stream));
        for (hipStream_t st : h->side_streams) QSV_HIP(h, hipStreamWaitEvent(st, h->ev_join, 0));
    }
    return QSV_OK;
}

int ensure_host_batch(qsv_t* h, size_t bytes) {
    if (h->h_batch_bytes >= bytes) return QSV_OK;
    if (h->h_batch) {
        QSV_HIP(h, sync_streams(h));
        QSV_HIP(h, hipHostFree(h->h_batch));
        h->h_batch = nullptr;
    }
    size_t want = std::max(bytes * 2, size_t(1) << 16);
    h->epoch += 1;
    QSV_HIP(h, hipHostMalloc(&h->h_batch, want, hipHostMallocDefault));
    h->h_batch_bytes = want;
    if (h->bar_ship) {
        if (h->d_ship) QSV_HIP(h, hipFree(h->d_ship));
        h->d_ship = nullptr;
        h->ship_shadow.clear();
        QSV_HIP(h, hipMalloc(&h->d_ship, want));
    }
    return QSV_OK;
}

// where the kernels read a batch's descriptors and parameters from
const void* ship_base(const qsv_t* h) { return h->bar_ship ? h->d_ship : h->h_batch; }
// where the kernels read the descriptors of the current batch from: a batch that repeats the one before it (same layout, kept:
// qsv_eval_begin) finds them in the device copy that batch's kernels left -- one PCIe round trip less at the start of every
// workgroup
// -- unless it runs over FEWER lanes than the push that laid the batch out (qsv_eval_set_output behind a call that waited): the
// device copy's slots are that push's, an evaluation's position modulo its lanes' share of the slots, and a launch group of
// this push, which spans a larger share, would hold two evaluations per slot.  Such a push reads the pinned descriptors, where
// eval_push has just written its own slots.  (Over more lanes the groups are smaller and the kept slots distinct within each.)
const EvalDesc* descs_base(const qsv_t* h) {
    if (h->batch.repeat && !h->bar_ship && h->repeat_device_descs && !h->batch.pinned_descs)
        return static_cast<const EvalDesc*>(h->d_batch.ptr);
    return static_cast<const EvalDesc*>(ship_base(h));
}
// where the kernels of the current push read parameter values from: the pinned staging buffer, or the caller's device memory
const double* params_base(const qsv_t* h) {
    if (h->batch.dev_params) return h->batch.dev_params;
    return reinterpret_cast<const double*>(static_cast<const char*>(h->h_batch) + h->batch.desc_bytes);
}

// where the kernels of the current batch write results: the caller's device buffer (qsv_eval_set_output) or the pinned one
double* result_base(const qsv_t* h) { return h->out_target ? h->out_target : h->h_out; }

// a recorded launch's argument struct, and which of its call-dependent pointers it carries (replay_push sets them anew)
void record_args(qsv_t* h, LaunchEntry& e, const PassArgs& a) {
    e.a = a;
    e.host_evals_off = a.host_evals ? int64_t(a.host_evals - descs_base(h)) : -1;
    e.takes_params = a.host_params != nullptr;
    e.result_off = a.result_out ? int64_t(a.result_out - result_base(h)) : -1;
    if ((a.host_params && a.host_params != params_base(h)) || a.active.flags) record_spoil(h);
}

void record_pass(qsv_t* h, int r, dim3 grid, int threads, size_t lds, const PassArgs& a) {
    LaunchEntry* e = record_entry(h, LaunchEntry::Pass, ws(h));
    if (!e) return;
    record_args(h, *e, a);
    e->dtype = h->dtype;
    e->r = r;
    e->xmode = h->cfg.xmode;
    e->grid = grid;
    e->threads = threads;
    e->lds = lds;
}

int ensure_host_out(qsv_t* h, size_t count) {
    if (h->h_out_count >= count) return QSV_OK;
    if (h->h_out) {
        QSV_HIP(h, sync_streams(h));
        QSV_HIP(h, hipHostFree(h->h_out));
        h->h_out = nullptr;
    }
    size_t want = std::max(count * 2, size_t(256));
    QSV_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_out), want * sizeof(double), hipHostMallocDefault));
    h->h_out_count = want;
    return QSV_OK;
}

// Device time of spans of a stream (option "time_moments"): begin(stream, tag) .. end(stream) bracket one between two events;
// after the caller's synchronise, elapsed(tag, sum) adds the milliseconds of the tag's spans, in their order.  The timer owns its
// events: they are destroyed on every exit path.
struct SpanTimer {
    struct Span {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        int tag = 0;
    };
    std::vector<Span> spans;
    SpanTimer() = default;
    SpanTimer(const SpanTimer&) = delete;
    SpanTimer& operator=(const SpanTimer&) = delete;
    ~SpanTimer() {
        for (Span& s : spans) {
            if (s.t0) (void)hipEventDestroy(s.t0);
            if (s.t1) (void)hipEventDestroy(s.t1);
        }
    }
    hipError_t begin(hipStream_t stream, int tag = 0) {
        spans.emplace_back();
        Span& s = spans.back();
        s.tag = tag;
        hipError_t err = hipEventCreate(&s.t0);
        if (err == hipSuccess) err = hipEventCreate(&s.t1);
        return err == hipSuccess ? hipEventRecord(s.t0, stream) : err;
    }
    hipError_t end(hipStream_t stream) { return hipEventRecord(spans.back().t1, stream); }
    hipError_t elapsed(int tag, double& sum_ms) const {
        for (const Span& s : spans) {
            if (s.tag != tag) continue;
            float ms = 0.0f;
            if (const hipError_t err = hipEventElapsedTime(&ms, s.t0, s.t1)) return err;
            sum_ms += double(ms);
        }
        return hipSuccess;
    }
};

// ---- batches ---------------------------------------------------------------------------------------------
// A batch is laid out once (descriptors, parameter offsets, matrix regions), then evaluations are PUSHED in
// group-aligned slices: each push ships that slice's parameter values, turns them into matrices on the device and
// launches the slice's gate passes, all asynchronously, so the host can prepare the next slice meanwhile.

// doubles of an evaluation's matrix region(s): one for the ordinary plan, or one per virtual circuit when it runs split
// The form of a split circuit the batch laid out now runs: the reduced one (Circuit::reduced) where the batch is the
// expectation route's and that route is the one-launch one (Batch::reduced), else the full form.
const SplitInfo& side_form(const qsv_t* h, const Circuit& c) { return h->batch.reduced && c.reduced.ok ? c.reduced : c.split; }

size_t mat_doubles_of(const qsv_t* h, const Circuit& c, bool split, int side) {
    if (!split)
        return mat_region_doubles(uint32_t(c.plan.stats.n_real_gates), uint32_t(h->n), h->geo.t, h->n - h->geo.k,
                                  c.plan.stats.n_passes);
    const SplitInfo& sp = side_form(h, c);
    return mat_region_doubles(uint32_t(sp.stats[side].n_real_gates), uint32_t(sp.n_virtual[side]), sp.t[side],
                              sp.outer[side], sp.stats[side].n_passes);
}

// The partial sums and the counters of evaluations of four and five keys (launch_factor: factor_big_slot_doubles() doubles and
// factor_big_slot_counters() counters per side-table slot), made when a handle first meets such an evaluation.  The counters
// are zeroed, and waited for, before anything else is enqueued: the counters of EVERY slot are cleared here, and the next
// push's chain -- on the other lane's stream, which does not wait for this one -- adds to those of its own slots.  Left to run
// in stream order, a clear that came late (its stream still busy with this chain's virtual circuits) reset counters that
// other chain had begun to add to: its evaluations of four and five keys were combined from incomplete partial sums, or not
// at all -- a wrong value in the first batch of a handle.  `in_push`: called from inside a push, whose launch record the clear
// (no kernel launch) spoils.
int ensure_factor_big(qsv_t* h, hipStream_t stream, bool in_push) {
    int rc = ensure(h, h->d_factor_big, factor_big_slot_doubles() * sizeof(double) * size_t(h->side_slots));
    if (rc || h->d_factor_big_count.ptr) return rc;
    const size_t cbytes = factor_big_slot_counters() * sizeof(uint32_t) * size_t(h->side_slots);
    if ((rc = ensure(h, h->d_factor_big_count, cbytes))) return rc;
    if (in_push) record_spoil(h);
    QSV_HIP(h, hipMemsetAsync(h->d_factor_big_count.ptr, 0, cbytes, stream));
    h->host_waits += 1;
    QSV_HIP(h, hipStreamSynchronize(stream));
    return QSV_OK;
}

// Whether a circuit runs as the two virtual circuits of its split form (split.hpp) in a call of one kind (split_rule):
// `allow` -- what the virtual circuits leave is all the caller needs of the final state --, and no more cut keys than the
// caller's kernels take (four and five keys: the factorised expectation under a quadratic operator only).  Otherwise the
// circuit runs its ordinary plan.  (A circuit on a kept state has no split form: its plan is unfolded.)
struct SplitRule {
    bool allow = false;
    int max_keys = 3;
    bool reduced = false;  // the one-launch route's reduced forms where circuits have them (the expectation route only: eval_begin)
    bool takes(const Circuit& c) const { return allow && c.split.ok && c.split.n_keys <= max_keys && c.prefix_id < 0; }
    size_t count(const std::vector<Circuit*>& circs) const {
        return size_t(std::count_if(circs.begin(), circs.end(), [&](const Circuit* c) { return takes(*c); }));
    }
};

int batch_layout(qsv_t* h, const std::vector<Circuit*>& circs, const std::vector<int64_t>& n_params, SplitRule rule = {}) {
    auto splits = [&](const Circuit* c) { return rule.takes(*c); };
    qsv_handle::Batch& b = h->batch;
    const size_t n_evals = circs.size();
    int rc;
    h->epoch += 1;  // (whatever an earlier batch left in the staging buffer is overwritten below)
    b.repeat = false;
    b.reduced = rule.reduced;
    b.record.entries.clear();  // (the launches of the layout that goes)
    b.record.usable = false;
    if ((rc = wait_pending(h))) return rc;  // (the staging buffers are written below)
    {
        // ordinary plans that are needed now and do not exist yet (circuits registered in split form): scheduled on the
        // host's worker threads when there are several
        std::vector<Circuit*> missing;
        for (Circuit* c : circs)
            if (!splits(c) && !c->has_plan && std::find(missing.begin(), missing.end(), c) == missing.end())
                missing.push_back(c);
        if (missing.size() >= 4) {
            std::vector<BuiltCircuit> built;
            build_many(h, missing.size(), [&](size_t i, BuiltCircuit& out) {
                Circuit& c = *missing[i];
                try {
                    PlanConfig pc = h->cfg;
                    pc.fold = pc.fold && c.fold;
                    out.circuit.plan = build_ordinary_plan(h, c.gates, c.angles, pc);
                } catch (const std::exception& e) {
                    out.rc = QSV_E_ARG;
                    out.err = std::string("plan: ") + e.what();
                }
            }, built);
            for (size_t i = 0; i < missing.size(); ++i) {
                if (built[i].rc) return fail(h, built[i].rc, built[i].err);
                Circuit& c = *missing[i];
                const CircuitPlan& p = built[i].circuit.plan;
                c.off_plan = uint32_t(c.plan.words.size());
                c.plan.words.insert(c.plan.words.end(), p.words.begin(), p.words.end());
                c.plan.stats = p.stats;
                c.has_plan = true;
                c.uploaded = false;
                c.gates.clear();
                c.angles.clear();
            }
        } else {
            for (Circuit* c : missing)
                if ((rc = ensure_plan(h, *c))) return rc;
        }
    }
    if ((rc = upload_plans(h, circs))) return rc;
    size_t total_params = 0, total_mats = 0;
    b.split.assign(n_evals, 0);
    b.split_any = false;
    b.cont_any = false;
    b.eval_at.resize(n_evals);
    for (size_t i = 0; i < n_evals; ++i) b.eval_at[i] = uint32_t(i);
    for (size_t i = 0; i < n_evals; ++i) {
        if (n_params[i] < circs[i]->n_params) return too_few_values(h, circs[i]->n_params, n_params[i]);
        total_params += size_t(n_params[i]);
        const bool split = splits(circs[i]);
        b.split[i] = split;
        b.split_any |= split;
        total_mats += mat_doubles_of(h, *circs[i], split, 0) + (split ? mat_doubles_of(h, *circs[i], true, 1) : 0);
    }
    if (total_params >= (size_t(1) << 31) || total_mats >= (size_t(1) << 31))
        return fail(h, QSV_E_ARG, "batch too large");
    // The counters of evaluations of four and five keys (run_group, launch_factor) are allocated and cleared here, before the
    // batch's first push.  Left to the push, the clear -- no kernel launch -- spoiled the push's launch record, and a repeated
    // push records nothing: the first batch of a handle that held such a circuit was never replayed while its layout was kept,
    // where the same batch on a handle that had met one before was (tests/test_gpu_operator_walk.py).
    if (b.split_any && !h->d_factor_big_count.ptr && h->side_slots > 0) {
        int most_keys = 0;
        for (size_t i = 0; i < n_evals; ++i)
            if (b.split[i]) most_keys = std::max(most_keys, circs[i]->split.n_keys);
        if (most_keys > 3 && (rc = ensure_factor_big(h, h->stream, false))) return rc;
    }
    b.desc_bytes = ((sizeof(EvalDesc) * n_evals * (b.split_any ? 2 : 1) + 63) / 64) * 64;
    const size_t bytes = b.desc_bytes + (total_params + 1) * sizeof(double);
    if ((rc = ensure_host_batch(h, bytes))) return rc;
    if ((rc = ensure(h, h->d_batch, bytes))) return rc;
    if ((rc = ensure(h, h->d_mats, total_mats * sizeof(double)))) return rc;
    EvalDesc* hd = static_cast<EvalDesc*>(h->h_batch);
    b.circs = circs;
    b.param_base.resize(n_evals);
    b.n_params.resize(n_evals);
    size_t pcur = 0, mcur = 0;
    for (size_t i = 0; i < n_evals; ++i) {
        const Circuit& c = *circs[i];
        const uint32_t slot = uint32_t(i % size_t(h->group));
        if (!b.split[i]) {
            uint32_t flags = 0, kept_slot = 0;
            if (c.prefix_id >= 0) {  // (alive: a circuit registered on a kept state holds it)
                flags = kEvalPrefix;
                kept_slot = h->prefixes.find(c.prefix_id)->second.slot;
                b.cont_any = true;
            }
            hd[i] = EvalDesc{c.plan_base + c.off_plan, uint32_t(mcur), slot, uint32_t(i), uint32_t(pcur), uint32_t(n_params[i]), flags, kept_slot};
            mcur += mat_doubles_of(h, c, false, 0);
            if (b.split_any) hd[n_evals + i] = EvalDesc{0, 0, slot, uint32_t(i), 0, 0, kEvalNull, 0};
        } else {
            // one descriptor per virtual circuit: side A here, side B in the second region
            const SplitInfo& sp = side_form(h, c);
            for (int s = 0; s < 2; ++s) {
                hd[size_t(s) * n_evals + i] =
                    EvalDesc{c.plan_base + sp.off_side[s], uint32_t(mcur), slot, uint32_t(i), uint32_t(pcur),
                             uint32_t(n_params[i]), kEvalSide | (s ? kEvalSideB : 0u) | (sp.fused ? kEvalFused : 0u) | (sp.fused && sp.halves ? kEvalHalves : 0u),
                             c.plan_base + sp.off_block};
                mcur += mat_doubles_of(h, c, true, s);
            }
        }
        b.param_base[i] = uint32_t(pcur);
        b.n_params[i] = uint32_t(n_params[i]);
        pcur += size_t(n_params[i]);
        h->prof.n_gates += uint64_t(c.n_gates);
    }
    // (no copy here: prepare_kernel reads descriptors and parameters from this pinned buffer and writes the device
    // copy of the descriptors itself)
    b.pushed = 0;
    return QSV_OK;
}

const EvalDesc* batch_evals(const qsv_t* h) { return static_cast<const EvalDesc*>(h->d_batch.ptr); }

// Ship the parameter values of evaluations [first, first+count) (packed back to back in `values`) and prepare
// their matrices.
// (The first n_fused evaluations of the range are split evaluations: the pass kernel prepares their virtual circuits
// itself, kModeFusedPrepare.)
int batch_ship(qsv_t* h, size_t first, size_t count, const double* values, size_t n_fused = 0) {
    qsv_handle::Batch& b = h->batch;
    if (count == 0) return QSV_OK;
    const size_t p0 = b.param_base[first];
    const size_t p1 = size_t(b.param_base[first + count - 1]) + b.n_params[first + count - 1];
    double* hp = reinterpret_cast<double*>(static_cast<char*>(h->h_batch) + b.desc_bytes);
    if (p1 > p0 && !b.dev_params && values != hp + p0) std::memcpy(hp + p0, values, (p1 - p0) * sizeof(double));  // (qsv_eval_staging: in place)
    if (h->bar_ship) {
        // the push's descriptors (both regions of a batch with split evaluations) into the device copy: plain stores through
        // the write-combining BAR mapping, fenced before any launch that reads them is queued -- and only what differs from
        // what the copy already holds (a population evaluated again: nothing; the copy costs 0.5 us per 2 KiB, the compare
        // nothing).  The parameters stay in pinned memory: 30 KiB through the BAR cost the host what the kernel saves.
        char* dst = static_cast<char*>(h->d_ship);
        const char* src = static_cast<const char*>(h->h_batch);
        const size_t P = b.circs.size();
        if (h->ship_shadow.size() < b.desc_bytes) h->ship_shadow.assign(b.desc_bytes, char(0xff));
        bool wrote = false;
        for (size_t region = 0; region < (b.split_any ? 2u : 1u); ++region) {
            const size_t at = (region * P + first) * sizeof(EvalDesc), bytes = count * sizeof(EvalDesc);
            if (at + bytes > b.desc_bytes || std::memcmp(h->ship_shadow.data() + at, src + at, bytes) == 0) continue;
            std::memcpy(dst + at, src + at, bytes);
            std::memcpy(h->ship_shadow.data() + at, src + at, bytes);
            wrote = true;
        }
        if (wrote) _mm_sfence();
    }
    const EvalDesc* host_evals = descs_base(h);
    const double* ship_params = params_base(h);
    if (count > n_fused) {
        QSV_LAUNCH(h, launch_prepare(static_cast<const uint32_t*>(h->d_arena.ptr), host_evals + first + n_fused,
                                     static_cast<EvalDesc*>(h->d_batch.ptr) + first + n_fused, ship_params,
                                     static_cast<double*>(h->d_mats.ptr), int(count - n_fused), ws(h), 1, 0, h->dtype, h->mask));
        if (LaunchEntry* e = record_entry(h, LaunchEntry::Prepare, ws(h))) {
            e->host_evals_off = int64_t(first + n_fused);
            e->evals = static_cast<EvalDesc*>(h->d_batch.ptr) + first + n_fused;
            e->takes_params = true;
            e->n = int(count - n_fused);
        }
    }
    return QSV_OK;
}

// One workgroup per evaluation (the register fits one tile) under a diagonal operator: the pass kernel prepares the
// evaluation itself and writes the expectation value straight to the result buffer -- one launch per push instead of three.
bool single_workgroup_path(const qsv_t* h, uint32_t mode) {
    return h->geo.blocks_per_state == 1 && h->diagonal && (mode & kModeFinalDiag) && !(mode & kModeFinalStore) &&
           (mode & kModeSynthFirst) && !getenv("QSV_NO_DIRECT");
}

unsigned chunks_per_state(const qsv_t* h) {
    const unsigned tpb = unsigned(std::min<uint32_t>(uint32_t(h->tiles_per_block), h->geo.blocks_per_state));
    return h->geo.blocks_per_state / tpb;
}

// partial sums the fused last pass leaves per state: one per wave of every workgroup
unsigned partials_per_state(const qsv_t* h) { return chunks_per_state(h) * unsigned(h->geo.threads_launch / 64); }

hipError_t stamp(qsv_t* h, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, bool begin) {
    if (!h->profiling) return hipSuccess;
    if (begin) {
        std::pair<hipEvent_t, hipEvent_t> p{nullptr, nullptr};
        hipError_t e = hipEventCreate(&p.first);
        if (e != hipSuccess) return e;
        e = hipEventCreate(&p.second);
        if (e != hipSuccess) return e;
        list.push_back(p);
        return hipEventRecord(p.first, ws(h));
    }
    return hipEventRecord(list.back().second, ws(h));
}

// Split evaluations need no contraction sweep under a quadratic diagonal operator (kernels.hpp: launch_factor).
bool factor_path(const qsv_t* h) { return h->factor_enabled && h->diagonal && h->quadratic && h->d_quad.ptr != nullptr && h->d_factor.ptr != nullptr; }

// ... and none under a general operator (kernels.hpp: launch_factor_terms).
bool factor_terms_path(const qsv_t* h) { return h->factor_enabled && !h->diagonal && h->n_fterms > 0 && h->d_side.ptr != nullptr; }

// Split evaluations flagged kEvalFused are finished by the launch that runs their virtual circuits (quadratic operator).
bool fused_route(const qsv_t* h) { return factor_path(h) && h->d_factor_count.ptr != nullptr && h->fused_factor; }
// ... with the reduced forms of circuits that have one (Circuit::reduced): a reduced side's values of D come from its own table only
bool reduced_route(const qsv_t* h) { return fused_route(h) && h->final_controls && h->d_diag.ptr != nullptr; }

// The kinds of call that may run circuits split, and what each needs of the final states: the expectation value under the
// operator set now (eval_begin; qsv_circuit_cost also asks before an operator is set), samples or the exact CVaR (read from the
// product of the two side tables, up to three keys), the values of an observable set's Pauli strings (the side tables, at most
// 32 qubits).
enum class SplitUse { Expectation, Sampling, Observables };

SplitRule split_rule(const qsv_t* h, SplitUse use) {
    switch (use) {
    case SplitUse::Expectation:
        return {h->n_terms == 0 || h->diagonal || factor_terms_path(h), (h->n_terms == 0 || factor_path(h)) ? kMaxSplitKeys : 3};
    case SplitUse::Sampling:
        return {h->split_sampling, 3};
    case SplitUse::Observables:
        break;
    }
    return {h->factor_enabled && h->d_side.ptr != nullptr && h->n <= 32, 3};
}

// Workgroups of a one-launch evaluation that do not leave at once: one per side, two for a half side (kernels.hpp kEvalHalves).
size_t working_workgroups(const SplitInfo& sp) {
    return 2u + (sp.halves ? size_t(sp.n_virtual[0] == kFusedLdsRowsBits) + size_t(sp.n_virtual[1] == kFusedLdsRowsBits) : 0u);
}

// Run the gate passes of evaluations [first, first+count) of the current batch (one launch group).
int run_group(qsv_t* h, const std::vector<Circuit*>& circs, size_t first, size_t count, uint32_t mode) {
    const qsv_handle::Batch& b = h->batch;
    const bool batch_split = b.split_any && b.split.size() == circs.size();
    const bool reordered = (b.split_any || b.cont_any) && b.split.size() == circs.size();
    // descriptor position -> evaluation (eval_push put the push's split evaluations first, those on kept states last)
    auto eval_of = [&](size_t pos) { return reordered ? size_t(b.eval_at[pos]) : pos; };
    size_t n_split = 0, n_cont = 0;
    int max_passes = 0;
    for (size_t i = 0; i < count; ++i) {
        const size_t e = eval_of(first + i);
        if (batch_split && b.split[e]) {
            n_split = i + 1;  // (split evaluations lead each push, so also each group of it)
        } else {
            max_passes = std::max(max_passes, circs[e]->plan.stats.n_passes);
            n_cont += circs[e]->prefix_id >= 0 ? 1 : 0;
        }
    }
    // Evaluations that continue a kept state read it in their first pass (the later-pass instantiation of the kernel, no
    // synthesis): a launch group holds only such evaluations, or none
    if (n_cont > 0) {
        if (n_cont != count) return fail(h, QSV_E_STATE, "internal: a launch group mixes evaluations on kept states with others");
        mode &= ~uint32_t(kModeSynthFirst | kModeFusedPrepare | kModeDirectResult);
    }
    const bool any_split = n_split > 0;
    if (b.reduced && (mode & kModeSidesOnly)) return fail(h, QSV_E_STATE, "internal: a batch laid out for reduced sides runs its sides only");
    const size_t n_plain = count - n_split;
    if (h->mask.flags) mode |= kModeMasked;  // (qsv_cvar_device with a mask: every launch below carries the bit and the pointer)
    PassArgs a{};
    a.active = h->mask;
    a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
    a.mats = static_cast<const double*>(h->d_mats.ptr);
    a.evals = batch_evals(h) + first;
    a.states = h->d_states.ptr;
    a.wtab = h->d_wtab.ptr;
    a.wtab_stride = h->wtab_stride;
    a.diag = static_cast<const double*>(h->d_diag.ptr);
    a.partials = static_cast<double*>(h->d_partials.ptr);
    a.state_stride = uint64_t(1) << h->n;
    a.mode = mode | h->stream_mode;
    a.prefix_states = h->d_prefix.ptr;
    a.side_diag = static_cast<const double*>(h->d_sdiag.ptr);
    {
        static const uint32_t dephase = getenv("QSV_DEPHASE") ? uint32_t(atoi(getenv("QSV_DEPHASE"))) : 0u;
        a.dephase = dephase;
    }
    // Pass 0 and the later passes have their own grids (tiles per workgroup): a compact pass 0 has few tiles and wants
    // them spread, a later pass sweeps all of them and amortises its set-up over more.  Which grid an evaluation's
    // LAST pass runs on depends on its own pass count only, so its partial sums are laid out (and added) the same
    // way in any batch.
    const unsigned chunks = chunks_per_state(h);
    const unsigned tpb_later = unsigned(std::min<uint32_t>(uint32_t(h->tiles_per_block_later), h->geo.blocks_per_state));
    const unsigned chunks_later = std::max(1u, std::min(chunks, h->geo.blocks_per_state / std::max(1u, tpb_later)));
    a.partial_chunks = chunks;
    a.region_stride = uint32_t(circs.size());
    const uint64_t sweep = (uint64_t(1) << h->n) * h->amp_bytes;
    // of the split evaluations (they lead the group) the first n_unfused need launches of their own after the virtual
    // circuits; the others are finished by the launch that runs theirs (kEvalFused, under a quadratic operator only)
    size_t n_unfused = n_split;
    const bool fuse_ok = fused_route(h) && !(mode & kModeSidesOnly);
    if (fuse_ok) {
        n_unfused = 0;
        while (n_unfused < n_split && !side_form(h, *circs[eval_of(first + n_unfused)]).fused) ++n_unfused;
    }
    const bool two_chains = b.chain_now && h->chain_stream != -1 && n_unfused > 0 && n_split > n_unfused && factor_path(h);
    // (the chain's stream: the second lane's, or -- for a push on the second lane -- the handle's own, which `work` = null means)
    hipStream_t const chain_st = h->chain_stream >= 0 ? h->side_streams[size_t(h->chain_stream)] : nullptr;
    if (any_split) {
        if (n_plain > 0) return fail(h, QSV_E_STATE, "internal: a launch group mixes split and ordinary evaluations");
        a.wtab = h->d_side.ptr;  // (the side tables' own slots)
        a.wtab_stride = h->side_stride;
        a.quad = static_cast<const double*>(h->d_quad.ptr);
        a.factor_scratch = static_cast<double*>(h->d_factor.ptr);
        a.factor_counters = static_cast<uint32_t*>(h->d_factor_count.ptr);
        a.n_full = uint32_t(h->n);
        a.result_out = h->out_target ? h->out_target : h->h_out;
        a.tiles_per_block = 1;
        a.host_params = params_base(h);
        a.mats_out = static_cast<double*>(h->d_mats.ptr);
        // threads and LDS of a launch over split evaluations [lo, hi) of the group: a side's tile may be larger than the
        // handle's (build_circuit)
        auto shape_of = [&](size_t lo, size_t hi, int* threads, size_t* lds, int* passes, unsigned* tiles) {
            int tile = 0, t = 0;
            *passes = 1;
            *tiles = 1;
            for (size_t i = lo; i < hi; ++i) {
                const SplitInfo& sp = side_form(h, *circs[eval_of(first + i)]);
                for (int s = 0; s < 2; ++s) {
                    tile = std::max(tile, sp.tile_bits[s]);
                    t = std::max(t, sp.t[s]);
                    *passes = std::max(*passes, sp.stats[s].n_passes);
                    *tiles = std::max(*tiles, 1u << sp.outer[s]);
                }
            }
            *threads = std::max(64, 1 << t);
            *lds = (size_t(1) << tile) * h->amp_bytes / (h->cfg.xmode == 2 ? 2 : 1);
        };
        auto at_least_four_waves = [](int threads) { return std::max(256, threads); };  // (the fused factor tail's Gram waves)
        auto launch_sides = [&](size_t lo, size_t hi, uint32_t extra_mode, int r) -> int {
            int threads, passes;
            size_t lds;
            unsigned tiles;
            shape_of(lo, hi, &threads, &lds, &passes, &tiles);
            if (extra_mode & kModeFusedFactor) threads = at_least_four_waves(threads);
            // (fused: ONE workgroup per side, one tile -- or, a half side, one of its two tiles -- then on to the side's Gram matrices)
            bool any_halves = false, any_reduced = false;
            if (extra_mode & kModeFusedFactor)
                for (size_t i = lo; i < hi; ++i) {
                    const Circuit& c = *circs[eval_of(first + i)];
                    any_halves |= side_form(h, c).halves;
                    any_reduced |= &side_form(h, c) == &c.reduced;  // (the launch then needs the tail that knows reduced sides)
                }
            // (a side's one workgroup sweeps its tiles itself, whatever the grid's width: pass_kernel)
            a.tiles_per_block = (extra_mode & kModeFusedFactor) ? tiles : 1u;
            const unsigned grid_x = (extra_mode & kModeFusedFactor) ? (any_halves ? 2u : 1u) : tiles;
            // (pass 0 prepares the virtual circuits' matrices and tables itself: no prepare launch ran for them)
            a.evals = batch_evals(h) + first + lo;
            a.host_evals = descs_base(h) + first + lo;
            a.evals_out = static_cast<EvalDesc*>(h->d_batch.ptr) + first + lo;
            for (int p = 0; p < passes; ++p) {
                a.pass_index = uint32_t(p);
                a.mode = ((p == 0 ? (mode | kModeFusedPrepare | extra_mode) : mode) & ~uint32_t(kModeSidesOnly)) | h->stream_mode;
                const int kind = p == 0 ? 0 : 1;
                size_t need = lds;
                if (p == 0) need = std::max(need, kFusedPrepareLdsBytes);
                if (p == 0 && (extra_mode & kModeFusedFactor)) need = std::max(need, kFusedFactorLdsBytes);
                // at most one workgroup per CU in flight anyway (two per evaluation): room for the sides' states in LDS
                size_t working = 0;
                for (size_t i = lo; i < hi; ++i) working += working_workgroups(side_form(h, *circs[eval_of(first + i)]));
                if (p == 0 && (extra_mode & kModeFusedFactor) && h->dtype == QSV_F64 && (h->fused_lds_table || any_halves) && working <= size_t(h->n_cus)) {
                    a.mode |= kModeFusedLdsTable;
                    need = std::max(need, kFusedLdsTableEnd);
                }
                // (need >= kFusedFactorLdsBytes: room for the staged plan run behind prepare_eval's scratch)
                if (p == 0 && (extra_mode & kModeFusedFactor) && h->side_prepare) a.mode |= kModeSidePrepare;
                if (p == 0 && any_reduced) a.mode |= kModeFusedReduced;
                if (p == 0 && any_reduced && h->live_entries) a.mode |= kModeFusedLive;
                if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[kind], true));
                QSV_LAUNCH(h, launch_pass(h->dtype, r, h->cfg.xmode, dim3(grid_x, unsigned(hi - lo), 2), threads, need, ws(h), a));
                record_pass(h, r, dim3(grid_x, unsigned(hi - lo), 2), threads, need, a);
                if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[kind], false));
                h->prof.n_pass_launches += 1;
                h->prof.kernel_launches[kind] += 1;
            }
            return QSV_OK;
        };
        int rc2;
        // (both kinds in one group: the ones with launches of their own start first, on the chain stream where the push
        // has one -- theirs is the longer chain)
        hipStream_t const lane_of_group = h->work;
        if (two_chains) h->work = chain_st;
        // (a launch is one instantiation of the kernel: within each kind the sides with eight amplitudes per thread come first,
        // order_split_first; half sides need their states in LDS, i.e. at most one workgroup per compute unit: four per evaluation)
        auto launch_sides_by_r = [&](size_t lo, size_t hi, uint32_t extra_mode) -> int {
            // (runs of evaluations whose sides have the same number of amplitudes per thread: order_split_first puts the eight-
            // amplitude ones first within each kind, but a range may hold both kinds -- every split evaluation under an operator
            // that has no one-launch route)
            for (size_t at = lo; at < hi;) {
                const int r = side_form(h, *circs[eval_of(first + at)]).side_r == 3 ? 3 : h->geo.r;
                size_t end = at;
                bool halves_here = false;
                while (end < hi && (side_form(h, *circs[eval_of(first + end)]).side_r == 3 ? 3 : h->geo.r) == r) {
                    halves_here |= side_form(h, *circs[eval_of(first + end)]).halves;
                    ++end;
                }
                // (half sides need the launch's states in LDS: at most one working workgroup per compute unit)
                for (size_t from = at; from < end;) {
                    size_t to = end;
                    if (halves_here && (extra_mode & kModeFusedFactor)) {
                        size_t wg = 0;
                        for (to = from; to < end && wg + working_workgroups(side_form(h, *circs[eval_of(first + to)])) <= size_t(h->n_cus); ++to)
                            wg += working_workgroups(side_form(h, *circs[eval_of(first + to)]));
                        if (to == from) to = from + 1;
                    }
                    const int rc3 = launch_sides(from, to, extra_mode, r);
                    if (rc3) return rc3;
                    from = to;
                }
                at = end;
            }
            return QSV_OK;
        };
        if (n_unfused > 0 && (rc2 = launch_sides_by_r(0, n_unfused, 0u))) return rc2;
        h->work = lane_of_group;
        // (the one-launch kind: as one launch -- unless the group is too large for one with the sides' states in LDS and holds half
        // sides, which lead the range: those go first, to the chain stream where the push has one free, the others follow as before)
        size_t n_halved = 0, all_working = 0;
        while (n_unfused + n_halved < n_split && side_form(h, *circs[eval_of(first + n_unfused + n_halved)]).halves) ++n_halved;
        for (size_t i = n_unfused; i < n_split; ++i) all_working += working_workgroups(side_form(h, *circs[eval_of(first + i)]));
        if (n_halved > 0 && n_unfused + n_halved < n_split && all_working > size_t(h->n_cus)) {
            // (too many for one launch with the sides' states in LDS, which half sides need: those few lead the range and get a
            // launch of their own -- on the chain stream where the push has one free --, the others follow as one launch, their
            // states handed over through their slots as in any launch of that size.  Measured, 128 evaluations with one half-sided
            // circuit: 56 us per step; cut into launches of one working workgroup per compute unit each: 75)
            if (b.chain_now && h->chain_stream != -1 && n_unfused == 0) h->work = chain_st;
            if ((rc2 = launch_sides_by_r(n_unfused, n_unfused + n_halved, kModeFusedFactor))) return rc2;
            h->work = lane_of_group;
            if ((rc2 = launch_sides_by_r(n_unfused + n_halved, n_split, kModeFusedFactor))) return rc2;
        } else if (n_split > n_unfused && (rc2 = launch_sides_by_r(n_unfused, n_split, kModeFusedFactor))) return rc2;
        a.mode = mode | h->stream_mode;
        // what the side circuits move: they synthesise their input and write their final states
        for (size_t i = 0; i < n_split; ++i) {
            const SplitInfo& sp = side_form(h, *circs[eval_of(first + i)]);
            const uint64_t bytes = ((uint64_t(1) << sp.n_virtual[0]) + (uint64_t(1) << sp.n_virtual[1])) * h->amp_bytes;
            h->prof.state_bytes += bytes;
            h->prof.moved_bytes += bytes;
            h->prof.kernel_bytes[0] += bytes;
            h->prof.kernel_moved_bytes[0] += bytes;
        }
        // (the fused ones: what their Gram matrices read and compute is part of that launch)
        for (size_t i = n_unfused; i < n_split; ++i) {
            const SplitInfo& sp = side_form(h, *circs[eval_of(first + i)]);
            for (int s = 0; s < 2; ++s) {
                const int side_bits = sp.n_virtual[s] - sp.n_keys;
                const uint64_t moved = (uint64_t(1) << sp.n_virtual[s]) * h->amp_bytes + (uint64_t(8) << side_bits);
                h->prof.kernel_bytes[0] += moved;
                h->prof.kernel_moved_bytes[0] += moved;
                h->prof.kernel_flops[0] += double(uint64_t(1) << side_bits) * double(1u << (2 * sp.n_keys)) * (side_bits / 2.0 + 5.0) * 2.0;
                h->prof.kernel_states[0] += 1;
                if (!sp.stats[s].pass_pairs.empty()) h->prof.kernel_flops[0] += 24.0 * sp.stats[s].pass_pairs[0];
            }
            h->prof.kernel_states[2] += 1;
        }
    }
    a.evals = batch_evals(h) + first + n_split;
    const bool direct = mode & kModeDirectResult;  // (eval_push decides, for the whole push)
    const bool fused = direct || (mode & kModeFusedPrepare);  // (... or the sampler path, for one-tile registers)
    if (mode & kModeFinalProbs) a.partials = static_cast<double*>(h->d_scratch.ptr);  // [slot][2^n] probabilities
    if (fused) {
        a.mode |= kModeFusedPrepare;
        a.host_evals = descs_base(h) + first + n_split;
        a.evals_out = static_cast<EvalDesc*>(h->d_batch.ptr) + first + n_split;
        a.host_params = params_base(h);
        a.mats_out = static_cast<double*>(h->d_mats.ptr);
        a.result_out = h->out_target ? h->out_target : h->h_out;
    }
    for (int p = 0; p < max_passes && n_plain > 0; ++p) {
        const unsigned chunks_p = p == 0 ? chunks : chunks_later;
        a.tiles_per_block = (h->geo.blocks_per_state + chunks_p - 1) / chunks_p;
        dim3 grid(chunks_p, unsigned(n_plain));
        a.pass_index = uint32_t(p);
        {
            static const bool tile_major = getenv("QSV_TILE_MAJOR") && atoi(getenv("QSV_TILE_MAJOR")) != 0;
            const bool swap = tile_major && !(p == 0 && (mode & kModeSynthFirst)) && n_plain > 1;
            a.mode = swap ? (a.mode | kModeTileMajor) : (a.mode & ~uint32_t(kModeTileMajor));
            if (swap) grid = dim3(unsigned(n_plain), chunks_p);
        }
        const int kind = (p == 0 && (mode & kModeSynthFirst)) ? 0 : 1;  // which instantiation of the kernel runs
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[kind], true));
        QSV_LAUNCH(h, launch_pass(h->dtype, h->geo.r, h->cfg.xmode, grid, h->geo.threads_launch,
                                  std::max(h->geo.lds_bytes, fused ? kFusedPrepareLdsBytes : size_t(0)), ws(h), a));
        record_pass(h, h->geo.r, grid, h->geo.threads_launch, std::max(h->geo.lds_bytes, fused ? kFusedPrepareLdsBytes : size_t(0)), a);
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[kind], false));
        h->prof.n_pass_launches += 1;
        h->prof.n_state_passes += n_plain;
        h->prof.kernel_launches[kind] += 1;
        // Algorithmic state bytes at this pass's own price: every pass reads and writes the state once, except that a
        // synthesising pass 0 does not read and a fused last pass does not write.  What it really moves is less when
        // a compact pass 0 writes, and pass 1 reads, a table of 2^cb tiles instead of the state.
        for (size_t i = n_split; i < count; ++i) {
            const PlanStats& st = circs[eval_of(first + i)]->plan.stats;
            if (p >= st.n_passes) continue;
            const bool reads = !(p == 0 && (mode & kModeSynthFirst));
            const bool writes = !(p + 1 == st.n_passes && !(mode & kModeFinalStore));
            const uint64_t table = (mode & kModeSynthFirst) && st.compact_bits >= 0
                                       ? (uint64_t(1) << (st.compact_bits + h->geo.k)) * h->amp_bytes
                                       : sweep;
            const uint64_t alg = (reads ? sweep : 0) + (writes ? sweep : 0);
            const uint64_t moved = (reads ? (p == 1 ? table : sweep) : 0) + (writes ? (p == 0 ? table : sweep) : 0);
            h->prof.state_bytes += alg;
            h->prof.moved_bytes += moved;
            h->prof.kernel_bytes[kind] += alg;
            h->prof.kernel_moved_bytes[kind] += moved;
            h->prof.kernel_states[kind] += 1;
            if (size_t(p) < st.pass_pairs.size()) h->prof.kernel_flops[kind] += 24.0 * st.pass_pairs[size_t(p)];
        }
    }
    if (any_split && !(mode & kModeSidesOnly) && factor_path(h)) {
      if (n_unfused > 0) {
        hipStream_t const lane_of_group = h->work;
        struct Restore {
            qsv_t* h;
            hipStream_t st;
            ~Restore() { h->work = st; }
        } restore{h, lane_of_group};
        if (two_chains) h->work = chain_st;
        // quadratic operator: the expectation value from the two side tables alone, written straight to the result buffer
        int most_keys = 0;
        for (size_t i = 0; i < n_unfused; ++i) most_keys = std::max(most_keys, circs[eval_of(first + i)]->split.n_keys);
        if (most_keys > 3) {
            // (batch_layout has made these buffers for every batch it laid out: a fallback, which spoils the push's record)
            int rc3 = ensure_factor_big(h, ws(h), true);
            if (rc3) return rc3;
        }
        a.evals = batch_evals(h) + first;
        a.result_out = h->out_target ? h->out_target : h->h_out;
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], true));
        QSV_LAUNCH(h, launch_factor(h->dtype, unsigned(n_unfused), static_cast<double*>(h->d_factor.ptr),
                                    static_cast<const double*>(h->d_quad.ptr), h->n, ws(h), a, static_cast<double*>(h->d_factor_big.ptr),
                                    static_cast<uint32_t*>(h->d_factor_big_count.ptr), most_keys));
        if (LaunchEntry* e = record_entry(h, LaunchEntry::Factor, ws(h))) {
            record_args(h, *e, a);
            e->n = int(n_unfused);
            e->n3 = most_keys;
        }
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], false));
        h->prof.kernel_launches[2] += 1;  // (the launches of the route, timed as one)
      }
        for (size_t i = 0; i < n_unfused; ++i) {
            const SplitInfo& sp = circs[eval_of(first + i)]->split;
            // what the two kernels read per state: the side tables and one value of D per table row
            uint64_t moved = 0;
            double flops = 0.0;
            for (int s = 0; s < 2; ++s) {
                const int side_bits = sp.n_virtual[s] - sp.n_keys;
                moved += (uint64_t(1) << sp.n_virtual[s]) * h->amp_bytes + (uint64_t(8) << side_bits);
                flops += double(uint64_t(1) << side_bits) * double(1u << (2 * sp.n_keys)) * (side_bits / 2.0 + 5.0) * 2.0;
                h->prof.kernel_states[0] += 1;
                if (!sp.stats[s].pass_pairs.empty()) h->prof.kernel_flops[0] += 24.0 * sp.stats[s].pass_pairs[0];
            }
            h->prof.state_bytes += moved;
            h->prof.kernel_bytes[2] += moved;
            h->prof.moved_bytes += moved;
            h->prof.kernel_moved_bytes[2] += moved;
            h->prof.kernel_states[2] += 1;
            h->prof.kernel_flops[2] += flops;
        }
    } else if (any_split && !(mode & kModeSidesOnly) && !h->diagonal) {
        // general operator: every term's two small matrices from the side tables, summed per evaluation into d_out
        a.evals = batch_evals(h) + first;
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], true));
        QSV_LAUNCH(h, launch_factor_terms(h->dtype, unsigned(n_split), static_cast<const FactorTerm*>(h->d_fterms.ptr), h->n_fterms,
                                          static_cast<double*>(h->d_fpart.ptr), ws(h), a));
        if (LaunchEntry* e = record_entry(h, LaunchEntry::FactorTerms, ws(h))) {
            record_args(h, *e, a);
            e->n = int(n_split);
        }
        QSV_LAUNCH(h, launch_reduce_partials(static_cast<const double*>(h->d_fpart.ptr), kFactorTermWaves, int(n_split),
                                             static_cast<double*>(h->d_out.ptr), ws(h), batch_evals(h) + first));
        if (LaunchEntry* e = record_entry(h, LaunchEntry::Reduce, ws(h))) {
            e->partials = static_cast<const double*>(h->d_fpart.ptr);
            e->blocks = kFactorTermWaves;
            e->n = int(n_split);
            e->out = static_cast<double*>(h->d_out.ptr);
            e->evals = batch_evals(h) + first;
        }
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], false));
        h->prof.kernel_launches[2] += 1;
        for (size_t i = 0; i < n_split; ++i) {
            const SplitInfo& sp = circs[eval_of(first + i)]->split;
            for (int s = 0; s < 2; ++s) {
                const uint64_t bytes = (uint64_t(1) << sp.n_virtual[s]) * h->amp_bytes * uint64_t(h->n_fterms);
                h->prof.kernel_bytes[2] += bytes;
                h->prof.kernel_moved_bytes[2] += bytes;
                h->prof.kernel_flops[2] += 8.0 * double(uint64_t(1) << sp.n_virtual[s]) * double(1u << sp.n_keys) * double(h->n_fterms);
                h->prof.kernel_states[0] += 1;
            }
            h->prof.kernel_states[2] += 1;
        }
    } else if (any_split && !(mode & kModeSidesOnly)) {
        // the contraction of the split evaluations
        a.evals = batch_evals(h) + first;
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], true));
        const unsigned contract_chunks = unsigned((uint64_t(1) << h->n) / (uint64_t(h->geo.threads_launch) << kSplitLoopBits));
        QSV_LAUNCH(h, launch_contract(h->dtype, contract_chunks, unsigned(n_split), h->geo.threads_launch, ws(h), a));
        if (LaunchEntry* e = record_entry(h, LaunchEntry::Contract, ws(h))) {
            record_args(h, *e, a);
            e->blocks = contract_chunks;
            e->n = int(n_split);
        }
        if (h->stamping) QSV_HIP(h, stamp(h, h->batch.launch_events[2], false));
        h->prof.kernel_launches[2] += 1;
        for (size_t i = 0; i < n_split; ++i) {
            const SplitInfo& sp = circs[eval_of(first + i)]->split;
            // what the contraction reads per state: D once (8 * 2^n bytes) and the two side tables
            const uint64_t moved = (uint64_t(8) << h->n) + ((uint64_t(1) << sp.n_virtual[0]) + (uint64_t(1) << sp.n_virtual[1])) * h->amp_bytes;
            h->prof.state_bytes += moved;
            h->prof.kernel_bytes[2] += moved;
            h->prof.moved_bytes += moved;
            h->prof.kernel_moved_bytes[2] += moved;
            h->prof.kernel_states[2] += 1;
            h->prof.kernel_flops[2] += double(uint64_t(1) << h->n) * (8.0 * double(1u << sp.n_keys) + 5.0);
            for (int s = 0; s < 2; ++s) {
                h->prof.kernel_states[0] += 1;
                if (!sp.stats[s].pass_pairs.empty()) h->prof.kernel_flops[0] += 24.0 * sp.stats[s].pass_pairs[0];
            }
        }
    }
    return QSV_OK;
}

int eval_begin(qsv_t* h, const std::vector<Circuit*>& circs, const std::vector<int64_t>& n_params) {
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    h->prof = qsv_profile{};
    h->prof.n_evals = uint64_t(circs.size());
    int rc;
    const size_t n_evals = circs.size();
    if ((rc = ensure(h, h->d_partials, std::max<size_t>(1, n_evals) * partials_per_state(h) * sizeof(double)))) return rc;
    if ((rc = ensure(h, h->d_out, std::max<size_t>(1, n_evals) * sizeof(double)))) return rc;
    if ((rc = ensure_host_out(h, std::max<size_t>(1, n_evals)))) return rc;
    if (h->profiling) {
        QSV_HIP(h, hipEventCreate(&h->batch.ev0));
        QSV_HIP(h, hipEventCreate(&h->batch.ev1));
        QSV_HIP(h, hipEventRecord(h->batch.ev0, h->stream));
    }
    SplitRule rule = split_rule(h, SplitUse::Expectation);
    rule.reduced = reduced_route(h);
    if ((rc = batch_layout(h, circs, n_params, rule))) return rc;
    if (factor_terms_path(h) && h->batch.split_any &&
        (rc = ensure(h, h->d_fpart, std::max<size_t>(1, n_evals) * kFactorTermWaves * sizeof(double))))
        return rc;
    qsv_handle::Batch& b = h->batch;
    // Two streams: consecutive pushes alternate between them, so that kernels of different pushes share the chip
    // (+15 % on the benchmark population).  Each stream owns one half of the state slots (eval_push assigns them),
    // so a slot is only ever reused on the stream that used it before and needs no cross-stream ordering.  Only when
    // the expectation is fused into the last pass (no scratch shared between pushes).
    // Measured alternative: pass 0 of every push on one stream and the later passes on the other (compute-bound
    // beside memory-bound by construction) is 10 % slower: two resident kernels mostly take workgroup slots from
    // each other.
    b.ways = 1;
    if (h->diagonal && n_evals >= 2)
        b.ways = std::max(1, std::min({h->n_streams, h->n_lane_streams + 1, h->group}));  // (lanes: not the auxiliary stream)
    // A batch that mixes split evaluations (three short launches, no state) with ordinary ones (passes over resident
    // states): the ordinary ones go to the auxiliary stream, every push's, so that the two kinds run side by side instead
    // of one after the other (n = 14, 64 four-layer circuits of which a third has no split form: 114 -> see DESIGN.md).
    // Only where the split ones leave no partial sums for the push's common reduction (quadratic operator).
    b.aux_plain = false;
    if (h->diagonal && b.split_any && factor_path(h) && h->geo.blocks_per_state > 1)
        for (size_t i = 0; i < n_evals && !b.aux_plain; ++i) b.aux_plain = b.split[i] == 0;
    if (b.aux_plain && h->aux_stream < 0) {
        hipStream_t st = nullptr;
        QSV_HIP(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        h->side_streams.push_back(st);
        h->aux_stream = int(h->side_streams.size()) - 1;
        // (the plans of this batch were uploaded on the handle's stream before this stream existed)
        QSV_HIP(h, hipEventRecord(h->ev_join, h->stream));
        QSV_HIP(h, hipStreamWaitEvent(st, h->ev_join, 0));
    }
    b.aux_count = 0;
    b.used_mask = 0;
    b.n_pushes = 0;
    b.chain_crossed = false;
    // Every evaluation's result is ONE 8-byte store to the pinned result buffer by the kernel that finishes it (diagonal
    // operators): marked with a value no kernel writes, the buffer itself says when the batch is done (eval_end).
    b.sentinels = h->poll_results && h->diagonal && !h->profiling && n_evals > 0;
    if (b.sentinels) {
        uint64_t* v = reinterpret_cast<uint64_t*>(h->h_out);
        for (size_t i = 0; i < n_evals; ++i) v[i] = kResultSentinel;
    }
    return QSV_OK;
}

// Descriptors [first, first + count) of the current batch: split evaluations first, the others behind them (results,
// partial sums and slots go by the descriptor's fields, not by its position), so that the side circuits, the ordinary
// passes and the contraction are each launched over the evaluations they concern -- a workgroup that only finds out that
// it has nothing to do still costs its dispatch, and a mixed launch was mostly such workgroups.  Among the split ones
// those with more keys first: their workgroups of the contraction take longest and should not be the tail of the
// launch.  Returns the number of split evaluations; batch.eval_at maps positions back to evaluations.
// Evaluations that continue a kept state (Circuit::prefix_id) come LAST, behind the ordinary ones: their first pass runs the
// later-pass instantiation of the kernel, so they are launch groups of their own; *n_cont receives their number.
size_t order_split_first(qsv_t* h, size_t first, size_t count, size_t* n_cont = nullptr) {
    qsv_handle::Batch& b = h->batch;
    if (n_cont) *n_cont = 0;
    if (!b.split_any && !b.cont_any) return 0;
    EvalDesc* hd = static_cast<EvalDesc*>(h->h_batch);
    const size_t P = b.circs.size();
    std::vector<EvalDesc> tmp(hd + first, hd + first + count), tmp2;
    if (b.split_any) tmp2.assign(hd + P + first, hd + P + first + count);
    size_t at = first, n_split = 0;
    if (!b.split_any) {
        for (int cont = 0; cont <= 1; ++cont)
            for (size_t j = 0; j < count; ++j) {
                if (int(b.circs[first + j]->prefix_id >= 0) != cont) continue;
                hd[at] = tmp[j];
                b.eval_at[at] = uint32_t(first + j);
                ++at;
                if (cont && n_cont) *n_cont += 1;
            }
        return 0;
    }
    // (among the split ones first those that need launches of their own after the virtual circuits -- kEvalFused ones are
    // finished by the launch that runs theirs --, so that each kind is one contiguous range of every launch group)
    // (... and among the kEvalFused ones first those whose sides have eight amplitudes per thread: a launch is ONE instantiation of
    // the kernel)
    // (... and of those first the ones with half sides: a group too large for one launch with the sides' states in LDS gives them
    // a launch of their own, run_group)
    for (int fused = 0; fused <= 1; ++fused)
      for (int r = 3; r <= 4; ++r)
       for (int halved = 1; halved >= 0; --halved)
        for (int cls = kMaxSplitKeys; cls >= 0; --cls)
            for (size_t j = 0; j < count; ++j) {
                if (!b.split[first + j]) continue;
                const SplitInfo& sp = side_form(h, *b.circs[first + j]);
                if (sp.n_keys != cls || int(sp.fused) != fused || ((sp.side_r == 3) != (r == 3)) || int(sp.halves) != halved) continue;
                hd[at] = tmp[j];
                hd[P + at] = tmp2[j];
                b.eval_at[at] = uint32_t(first + j);
                ++at;
                ++n_split;
            }
    for (int cont = 0; cont <= 1; ++cont)
        for (size_t j = 0; j < count; ++j) {
            if (b.split[first + j] || int(b.circs[first + j]->prefix_id >= 0) != cont) continue;
            hd[at] = tmp[j];
            hd[P + at] = tmp2[j];
            b.eval_at[at] = uint32_t(first + j);
            ++at;
            if (cont && n_cont) *n_cont += 1;
        }
    return n_split;
}

// The expectation kernels of the general-operator path over the gc states of a launch group: x-mask groups [g1, g1 + groups), then
// their combination into d_out (every argument but these is the operator's or the handle's; both run on the handle's own stream)
OperatorView operator_view(const qsv_t* h) {
    return OperatorView{h->has_diag_part ? static_cast<const double*>(h->d_diag.ptr) : nullptr, h->n_groups,
                        static_cast<const PauliGroup*>(h->d_groups.ptr), static_cast<const uint64_t*>(h->d_z.ptr),
                        static_cast<const double*>(h->d_cre.ptr), static_cast<const uint32_t*>(h->d_term_odd.ptr)};
}
hipError_t launch_pauli_groups_of(qsv_t* h, int gc, int g1, int groups) {
    return launch_pauli_groups(h->dtype, h->d_states.ptr, uint64_t(1) << h->n, h->n, gc, operator_view(h), h->pauli_nb,
                               static_cast<double*>(h->d_term_partials.ptr), h->stream, g1, groups);
}
hipError_t launch_pauli_combine_of(qsv_t* h, int gc, const EvalDesc* evals) {
    return launch_pauli_combine(static_cast<const double*>(h->d_term_partials.ptr), uint32_t(h->n_groups) * uint32_t(h->pauli_nb),
                                h->has_diag_part ? static_cast<const double*>(h->d_partials.ptr) : nullptr, partials_per_state(h), gc,
                                evals, static_cast<double*>(h->d_out.ptr), h->stream);
}

// a push's own reduction into the result buffer, as a record entry
LaunchEntry reduce_entry(LaunchEntry e, const double* partials, int n, int64_t result_off, const EvalDesc* evals) {
    e.partials = partials;
    e.n = n;
    e.result_off = result_off;
    e.evals = evals;
    return e;
}

// what a push adds to the handle's counters (they are zero when a batch begins: `from` is the recorded push's total)
void add_push_counters(qsv_profile& to, const qsv_profile& from) {
    to.n_pass_launches += from.n_pass_launches;
    to.n_state_passes += from.n_state_passes;
    to.state_bytes += from.state_bytes;
    to.moved_bytes += from.moved_bytes;
    for (int k = 0; k < 3; ++k) {
        to.kernel_launches[k] += from.kernel_launches[k];
        to.kernel_bytes[k] += from.kernel_bytes[k];
        to.kernel_moved_bytes[k] += from.kernel_moved_bytes[k];
        to.kernel_flops[k] += from.kernel_flops[k];
        to.kernel_states[k] += from.kernel_states[k];
    }
}

// The one push of a batch that repeats the batch before it, whose push was recorded (eval_push: the record is usable, the handle's
// epoch has not moved, the batch cycles over as many streams): the recorded launches again, in their order, each on its stream.
//
// Set anew at every replay -- what may differ from the recording call although the layout is the same:
//   host_evals  (PassArgs; launch_prepare's)  descs_base(h): the pinned descriptors on the recording call, their device copy on a
//               repeat (repeat_device_descs), at the recorded offset
//   host_params (PassArgs; launch_prepare's)  params_base(h): the staging buffer or this call's device memory (qsv_eval_push_device)
//   result_out  (PassArgs; launch_reduce_partials' destination)  result_base(h): the pinned result buffer or this call's device
//               buffer (qsv_eval_set_output), at the recorded offset
//   active      (PassArgs; launch_prepare's)  the empty mask: no record is made or used under a mask
// Every other field is a function of the layout, the operator and the handle, none of which can change without the epoch moving
// (registrations, qsv_set_operator, qsv_set_option, qsv_set_profiling, every batch_layout, a new staging buffer) or the batch
// being laid out afresh: plan, mats / mats_out, evals / evals_out, states, wtab, diag, partials, quad, factor_scratch,
// factor_counters, prefix_states, side_diag are device buffers of the handle that only a batch_layout, an operator or a registration
// replaces; state_stride, wtab_stride, n_full, dephase are the handle's; pass_index, mode, tiles_per_block, region_stride,
// partial_chunks follow the circuits' plans and forms, the options and the number of streams (the record's `ways`).  Grid, block,
// LDS bytes and the kernel's instantiation likewise.  Device buffers a call may replace without a layout (d_partials, d_out,
// d_fpart, the result buffer) are replaced in eval_begin only, which lays the batch out.
int replay_push(qsv_t* h, size_t count, const double* values) {
    qsv_handle::Batch& b = h->batch;
    qsv_handle::Batch::LaunchRecord& rec = b.record;
    const size_t total = size_t(b.param_base[count - 1]) + b.n_params[count - 1];
    double* hp = reinterpret_cast<double*>(static_cast<char*>(h->h_batch) + b.desc_bytes);
    if (total > 0 && !b.dev_params && values != hp) std::memcpy(hp, values, total * sizeof(double));  // (as batch_ship)
    const EvalDesc* descs = descs_base(h);
    const double* params = params_base(h);
    double* result = result_base(h);
    for (LaunchEntry& e : rec.entries) {
        hipStream_t const st = e.stream < 0 ? h->stream : h->side_streams[size_t(e.stream)];
        PassArgs& a = e.a;
        a.host_evals = e.host_evals_off >= 0 ? descs + e.host_evals_off : nullptr;
        a.host_params = e.takes_params ? params : nullptr;
        a.result_out = e.result_off >= 0 ? result + e.result_off : nullptr;
        a.active = ActiveMask{};
        switch (e.kind) {
        case LaunchEntry::Prepare:
            QSV_LAUNCH(h, launch_prepare(static_cast<const uint32_t*>(h->d_arena.ptr), a.host_evals, const_cast<EvalDesc*>(e.evals), params,
                                         static_cast<double*>(h->d_mats.ptr), e.n, st, 1, 0, h->dtype, ActiveMask{}));
            break;
        case LaunchEntry::Pass:
            QSV_LAUNCH(h, launch_pass(e.dtype, e.r, e.xmode, e.grid, e.threads, e.lds, st, a));
            break;
        case LaunchEntry::Reduce:
            QSV_LAUNCH(h, launch_reduce_partials(e.partials, e.blocks, e.n, e.out ? e.out : a.result_out, st, e.evals));
            break;
        case LaunchEntry::Factor:
            QSV_LAUNCH(h, launch_factor(h->dtype, unsigned(e.n), static_cast<double*>(h->d_factor.ptr), static_cast<const double*>(h->d_quad.ptr),
                                        h->n, st, a, static_cast<double*>(h->d_factor_big.ptr),
                                        static_cast<uint32_t*>(h->d_factor_big_count.ptr), e.n3));
            break;
        case LaunchEntry::FactorTerms:
            QSV_LAUNCH(h, launch_factor_terms(h->dtype, unsigned(e.n), static_cast<const FactorTerm*>(h->d_fterms.ptr), h->n_fterms,
                                              static_cast<double*>(h->d_fpart.ptr), st, a));
            break;
        case LaunchEntry::Contract:
            QSV_LAUNCH(h, launch_contract(h->dtype, e.blocks, unsigned(e.n), h->geo.threads_launch, st, a));
            break;
        case LaunchEntry::PauliGroups:
            QSV_LAUNCH(h, launch_pauli_groups_of(h, e.n, e.n2, e.n3));
            break;
        case LaunchEntry::PauliCombine:
            QSV_LAUNCH(h, launch_pauli_combine_of(h, e.n, e.evals));
            break;
        }
    }
    // (what later code goes by, once the launches are queued)
    add_push_counters(h->prof, rec.prof);
    b.pushed = count;
    b.n_pushes = 1;
    b.whole_push = true;
    b.used_mask |= rec.used_mask;
    b.aux_count = rec.aux_count;
    b.chain_now = false;
    h->chain_stream = -1;
    h->replayed_pushes += 1;
    h->timing.replays += 1;
    return QSV_OK;
}

int eval_push(qsv_t* h, size_t first, size_t count, const double* values, const double* device_values = nullptr) {
    qsv_handle::Batch& b = h->batch;
    if (first != b.pushed) return fail(h, QSV_E_STATE, "evaluations must be pushed in order");
    if (first + count > b.circs.size()) return fail(h, QSV_E_ARG, "push exceeds the batch");
    // Launch groups: G evaluations whose states are resident together.  On one stream the slot of an evaluation is its
    // index mod G (batch_layout) and the stream orders every reuse.  With two streams each push takes its stream's
    // half of the slots and is cut into launch groups of G / 2.
    size_t G = size_t(h->group);
    struct WorkGuard {
        qsv_t* h;
        ~WorkGuard() {
            h->work = nullptr;
            h->stamping = false;
            h->batch.dev_params = nullptr;  // (a property of the push: other paths lay batches out and ship them too)
            h->batch.record.recording = false;
            h->batch.pinned_descs = false;
            h->timing.in_push = false;
        }
    } guard{h};
    PhaseClock push_clock(h, &PhaseClock::Timing::push_us);
    h->timing.in_push = h->timing.on;
    h->stamping = h->profiling;
    EvalDesc* hd = static_cast<EvalDesc*>(h->h_batch);  // pinned; prepare_kernel reads it after this point
    if (b.repeat && !(first == 0 && count == b.circs.size())) {
        // (pushed differently than the batch whose layout this one kept: lay it out afresh)
        const std::vector<Circuit*> circs = b.circs;
        const std::vector<int64_t> np(b.cur_counts.begin(), b.cur_counts.end());
        const int rc0 = eval_begin(h, circs, np);
        if (rc0) return rc0;
        if (h->out_target) b.ways = 1;  // (qsv_eval_set_output's choice, made before this push)
    }
    if (!device_values && h->async_pending) {  // (the staging buffer is about to be written: see qsv_eval_begin)
        QSV_HIP(h, sync_streams(h));
        h->async_pending = false;
    }
    // (values in device memory: the descriptors' offsets are those of the staging buffer, so the base is where evaluation 0's
    // values would be)
    b.dev_params = device_values && count > 0 ? device_values - b.param_base[first] : nullptr;
    const bool whole = first == 0 && count == b.circs.size();
    b.pinned_descs = b.repeat && b.ways < b.snap_ways;
    qsv_handle::Batch::LaunchRecord& rec = b.record;
    // (a record is made, and used, only where nothing but the call's own pointers can differ from one call to the next: no mask,
    // no per-launch events, descriptors that the kernels read where the host left them)
    const bool record_ok = whole && h->replay_enabled && h->repeat_enabled && !h->profiling && !h->mask.flags && !h->bar_ship && count > 0;
    const bool no_direct_env = h->geo.blocks_per_state == 1 && h->diagonal && getenv("QSV_NO_DIRECT") != nullptr;
    if (b.repeat && record_ok && rec.usable && rec.epoch == h->epoch && rec.ways == b.ways && rec.no_direct_env == no_direct_env)
        return replay_push(h, count, values);
    b.whole_push = whole;
    rec.recording = !b.repeat && record_ok && b.have_ids;
    if (rec.recording) {
        rec.entries.clear();
        rec.usable = rec.spoiled = false;
    }
    const size_t ways = size_t(std::max(1, b.ways)), lane = ways > 1 ? size_t(b.n_pushes) % ways : 0;
    const size_t P = b.circs.size();
    size_t n_cont = b.snap_n_cont;
    const size_t n_split = b.repeat ? b.snap_n_split : order_split_first(h, first, count, &n_cont);
    if (b.whole_push) {
        b.snap_n_split = n_split;
        b.snap_n_cont = n_cont;
        if (!b.repeat) b.snap_ways = b.ways;
    }
    // Slots.  Ordinary evaluations: G states are resident together; on one stream the slot of an evaluation is its
    // position mod G and the stream orders every reuse; with several streams each push takes its stream's share of the
    // slots.  (The expectation kernels of the general-operator path index states by position in the launch group.)
    // Split evaluations have no state, only two small tables: their own, much larger set of slots.
    if (ways > 1) {
        G = G / ways;
        if (lane) {
            h->work = h->side_streams[lane - 1];
            b.used_mask |= 1u << (lane - 1);
        }
    }
    const size_t SG = h->side_slots > 0 ? std::max<size_t>(1, size_t(h->side_slots) / ways) : 1;
    for (size_t j = 0; j < n_split; ++j) {
        const uint32_t slot = uint32_t(lane * SG + j % SG);
        hd[first + j].state_slot = slot;
        hd[P + first + j].state_slot = slot;
    }
    hipStream_t const lane_stream = h->work;  // (null: the handle's own)
    // Split evaluations of both kinds in this push -- finished by the launch that runs their virtual circuits (kEvalFused) /
    // with launches of their own: the second kind's chain (virtual circuits, Gram matrices, combination) goes to the chain
    // stream and runs beside the first kind's one launch.  Every split evaluation of the push has its own slot then (n_split
    // <= SG), so the two streams share nothing.
    // The chain stream is the OTHER lane's: idle when the push is the whole batch, and in a batch of two pushes (one per lane)
    // each stream then carries one push's single launch and the other push's chain -- 128 five-layer circuits: 230 -> see
    // DESIGN.md 4.2.  (A stream of its own would be the handle's fourth, and a process has four hardware queues by default: it
    // landed on the auxiliary stream's queue and the two chains ran one after the other; L = 6 with five keys: 397 -> 449 us
    // per step.)  A lane's slots are reused by the lane's later pushes in stream order -- which a chain on the other lane's
    // stream is outside of: a push that comes to a lane again after such a chain first joins the two lanes' streams.
    b.chain_now = false;
    h->chain_stream = -1;
    const size_t push_index = b.n_pushes;
    if (b.chain_crossed && push_index >= ways && h->n_lane_streams >= 1) {
        record_spoil(h);
        QSV_HIP(h, hipEventRecord(h->ev_join, h->stream));
        QSV_HIP(h, hipStreamWaitEvent(h->side_streams[0], h->ev_join, 0));
        QSV_HIP(h, hipEventRecord(h->ev_join, h->side_streams[0]));
        QSV_HIP(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
        b.chain_crossed = false;
    }
    if (h->chain_enabled && ways <= 2 && lane <= 1 && h->n_lane_streams >= 1 && n_split > 0 && n_split <= SG && factor_path(h) &&
        fused_route(h)) {
        size_t n_fused = 0;
        for (size_t j = 0; j < n_split; ++j) n_fused += side_form(h, *b.circs[b.eval_at[first + j]]).fused ? 1 : 0;
        b.chain_now = n_fused > 0 && n_fused < n_split;
        // (... or every split evaluation is of the first kind, too many for one launch with the sides' states in LDS, and some have
        // half sides, which need them there: those few get a launch of their own beside the others', run_group)
        size_t n_halved = 0;
        for (size_t j = 0; j < n_split; ++j) n_halved += side_form(h, *b.circs[b.eval_at[first + j]]).halves ? 1 : 0;
        size_t working = 0;
        for (size_t j = 0; j < n_split; ++j) working += working_workgroups(side_form(h, *b.circs[b.eval_at[first + j]]));
        if (n_fused == n_split && n_halved > 0 && working > size_t(h->n_cus)) b.chain_now = true;
    }
    if (b.chain_now) {
        record_spoil(h);  // (two streams, and events between them)
        h->chain_stream = lane == 0 ? 0 : -2;  // (-2: the handle's own stream, lane 0's)
        b.chain_crossed = true;
        if (lane == 0) {
            b.used_mask |= 1u;
            if (h->out_target) {  // (the caller may have work queued on the handle's stream that the results must come after)
                QSV_HIP(h, hipEventRecord(h->ev_join, h->stream));
                QSV_HIP(h, hipStreamWaitEvent(h->side_streams[0], h->ev_join, 0));
            }
        }
    }
    hipStream_t const plain_stream = b.aux_plain ? h->side_streams[size_t(h->aux_stream)] : lane_stream;
    if (b.aux_plain && n_split < count) b.used_mask |= 1u << h->aux_stream;

    for (size_t j = n_split; j < count; ++j) {
        // (on the auxiliary stream every ordinary evaluation of the batch: one stream orders every reuse of a slot)
        const uint32_t slot = b.aux_plain ? uint32_t((b.aux_count + (j - n_split)) % size_t(h->group))
                                          : uint32_t(lane * G + (j - n_split) % G);
        hd[first + j].state_slot = slot;
        if (b.split_any) hd[P + first + j].state_slot = slot;
    }
    if (b.aux_plain) {
        b.aux_count += count - n_split;
        G = size_t(h->group);
    }
    b.n_pushes += 1;
    const uint32_t mode = kModeSynthFirst | (h->diagonal ? kModeFinalDiag : kModeFinalStore) |
                          (h->has_diag_part ? kModeFinalDiag : 0u);
    bool direct = single_workgroup_path(h, mode) && n_cont == 0;  // (an evaluation on a kept state does not synthesise its input)
    for (size_t j = 0; direct && j < count; ++j) direct = b.circs[first + j]->plan.stats.n_passes == 1;
    h->work = plain_stream;  // (the preparation launch concerns the ordinary evaluations only)
    int rc = batch_ship(h, first, count, values, direct ? count : n_split);
    h->work = lane_stream;
    if (rc) return rc;
    const uint32_t group_mode = mode | (direct ? uint32_t(kModeDirectResult) : 0u);
    // launch groups: the split evaluations of the push in groups of SG, then the ordinary ones in groups of G, then -- in
    // groups of their own -- those that continue a kept state
    const size_t cont0 = first + count - n_cont;
    for (size_t g0 = first; g0 < first + count;) {
        const bool in_split = g0 < first + n_split;
        const size_t gc = in_split ? std::min(SG, first + n_split - g0) : std::min(G, (g0 < cont0 ? cont0 : first + count) - g0);
        struct Advance {
            size_t& g0;
            size_t gc;
            ~Advance() { g0 += gc; }
        } advance{g0, gc};
        h->work = in_split ? lane_stream : plain_stream;
        QSV_HIP(h, stamp(h, b.pass_events, true));
        rc = run_group(h, b.circs, g0, gc, group_mode);
        if (!rc) QSV_HIP(h, stamp(h, b.pass_events, false));
        if (rc) return rc;
        if (!h->diagonal && !in_split) {
            QSV_HIP(h, stamp(h, b.exp_events, true));
            // (an operator may have more x-mask groups than gridDim.y can be: slices of the groups, the partial sums where one
            // launch puts them)
            for (int g1 = 0; g1 < h->n_groups; g1 += h->max_grid_y) {
                QSV_LAUNCH(h, launch_pauli_groups_of(h, int(gc), g1, std::min(h->max_grid_y, h->n_groups - g1)));
                if (LaunchEntry* e = record_entry(h, LaunchEntry::PauliGroups, h->stream)) {
                    e->n = int(gc);
                    e->n2 = g1;
                    e->n3 = std::min(h->max_grid_y, h->n_groups - g1);
                }
            }
            QSV_LAUNCH(h, launch_pauli_combine_of(h, int(gc), batch_evals(h) + g0));
            if (LaunchEntry* e = record_entry(h, LaunchEntry::PauliCombine, h->stream)) {
                e->n = int(gc);
                e->evals = batch_evals(h) + g0;
            }
            QSV_HIP(h, stamp(h, b.exp_events, false));
        }
    }
    if (h->diagonal && !direct) {
        // This push's evaluations are reduced on the push's own stream, straight into the pinned result buffer: no
        // cross-stream join in front of one final reduction (the join alone cost 15-30 us at the end of every call).
        QSV_HIP(h, stamp(h, b.exp_events, true));
        // (on the stream that wrote the partial sums it reads: the ordinary evaluations' -- the auxiliary stream in a mixed
        // batch, ALSO in a push of that batch that holds no split evaluation itself; off the factor path the split evaluations
        // leave partial sums too, and then the batch has no auxiliary stream: plain_stream is the lane's)
        h->work = plain_stream;
        LaunchEntry* e = record_entry(h, LaunchEntry::Reduce, ws(h));
        if (n_split > 0 && factor_path(h)) {  // (the split evaluations' results are already there: the others, by descriptor)
            QSV_LAUNCH(h, launch_reduce_partials(static_cast<const double*>(h->d_partials.ptr), partials_per_state(h),
                                                 int(count - n_split), result_base(h), ws(h), batch_evals(h) + first + n_split));
            if (e) *e = reduce_entry(*e, static_cast<const double*>(h->d_partials.ptr), int(count - n_split), 0, batch_evals(h) + first + n_split);
        } else {
            QSV_LAUNCH(h, launch_reduce_partials(static_cast<const double*>(h->d_partials.ptr) + first * size_t(partials_per_state(h)),
                                                 partials_per_state(h), int(count), result_base(h) + first, ws(h)));
            if (e) *e = reduce_entry(*e, static_cast<const double*>(h->d_partials.ptr) + first * size_t(partials_per_state(h)), int(count), int64_t(first), nullptr);
        }
        if (e) e->blocks = partials_per_state(h);
        QSV_HIP(h, stamp(h, b.exp_events, false));
    }
    b.pushed = first + count;
    if (rec.recording) {
        rec.usable = !rec.spoiled;
        rec.epoch = h->epoch;
        rec.ways = b.ways;
        rec.no_direct_env = no_direct_env;
        rec.used_mask = b.used_mask;
        rec.aux_count = b.aux_count;
        rec.prof = h->prof;
    }
    return QSV_OK;
}

int eval_end(qsv_t* h, double* out) {
    qsv_handle::Batch& b = h->batch;
    const size_t n_evals = b.circs.size();
    PhaseClock end_clock(h, &PhaseClock::Timing::end_us);  // (the copy-out inside it is reported apart)
    if (b.pushed != n_evals) return fail(h, QSV_E_STATE, "not every evaluation of the batch was pushed");
    if (n_evals == 0) return QSV_OK;
    const unsigned used_mask = b.used_mask;
    if (h->profiling)  // (only so that ev1 below marks the end of EVERY stream's work)
        for (size_t i = 0; i < h->side_streams.size(); ++i)
            if (used_mask >> i & 1u) {
                QSV_HIP(h, hipEventRecord(h->ev_join, h->side_streams[i]));
                QSV_HIP(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
            }
    b.used_mask = 0;
    if (h->profiling) QSV_HIP(h, hipEventRecord(b.ev1, h->stream));
    // a batch that went through in one push leaves its layout for the next call to find (qsv_eval_begin)
    if (b.have_ids && b.whole_push && h->repeat_enabled && !h->profiling) {
        if (!b.repeat) {
            b.snap_ids = b.cur_ids;
            b.snap_counts = b.cur_counts;
        }
        b.snap_epoch = h->epoch;
    } else {
        b.snap_epoch = 0;
    }
    if (h->out_target && !out && !h->profiling) {
        // Results go to the caller's device buffer: nothing to wait for here.  Whatever the caller enqueues on the
        // handle's stream next (a collective over the results) runs after every push, also those of the other streams.
        for (size_t i = 0; i < h->side_streams.size(); ++i)
            if (used_mask >> i & 1u) {
                QSV_HIP(h, hipEventRecord(h->ev_join, h->side_streams[i]));
                QSV_HIP(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
            }
        if (!h->diagonal)
            // (hipMemcpyDefault: the caller's buffer may be host memory the device can address -- a node's shared fitness table)
            QSV_HIP(h, hipMemcpyAsync(h->out_target, h->d_out.ptr, n_evals * sizeof(double), hipMemcpyDefault, h->stream));
        h->async_pending = true;
        return QSV_OK;
    }
    if (!h->diagonal)
        QSV_HIP(h, hipMemcpyAsync(h->out_target ? h->out_target : h->h_out, h->d_out.ptr, n_evals * sizeof(double),
                                  h->out_target ? hipMemcpyDefault : hipMemcpyDeviceToHost, h->stream));
    // The results themselves say when they are there: every evaluation's is one store to the pinned buffer, visible to the host
    // about 5 us before the stream's completion signal is (scripts/ubench/flag_vs_sync.hip).  Watched for at most kPollMicros
    // -- a step of a shallow population; longer batches wait on the streams as before.  Results that have all arrived ARE the
    // end of the batch's work (every kernel that reads a staging buffer comes before the one that writes its evaluation's
    // result): nothing is left for a later call to wait for, and the runtime retires its own bookkeeping with the next
    // launches (synchronising at the start of the next call instead was measured: 77 -> 84 us per step, worse than not polling).
    bool arrived = false;
    if (b.sentinels && !h->out_target && out) {
        const volatile uint64_t* v = reinterpret_cast<const volatile uint64_t*>(h->h_out);
        const auto t0 = std::chrono::steady_clock::now();
        size_t done = 0;
        for (uint32_t spin = 1;; ++spin) {
            while (done < n_evals && v[done] != kResultSentinel) ++done;
            if (done == n_evals) {
                arrived = true;
                break;
            }
            if ((spin & 31u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kPollMicros)) break;
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!arrived) {
        // (polling hipStreamQuery instead was measured: no faster, and it slowed concurrent callers down threefold)
        h->host_waits += 1;
        QSV_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < h->side_streams.size(); ++i)
            if (used_mask >> i & 1u) QSV_HIP(h, hipStreamSynchronize(h->side_streams[i]));
    }
    {
        PhaseClock copy_clock(h, &PhaseClock::Timing::copy_us);
        if (h->out_target) {  // (a waiting end of a batch with a device output: the caller also gets a host copy)
            if (out) QSV_HIP(h, hipMemcpy(out, h->out_target, n_evals * sizeof(double), hipMemcpyDefault));
        } else {
            std::memcpy(out, h->h_out, n_evals * sizeof(double));
        }
    }

    if (h->profiling) {
        float ms = 0.f;
        QSV_HIP(h, hipEventElapsedTime(&ms, b.ev0, b.ev1));
        h->prof.total_ms = ms;
        for (auto& p : b.pass_events) {
            QSV_HIP(h, hipEventElapsedTime(&ms, p.first, p.second));
            h->prof.pass_ms += ms;
        }
        for (int kind = 0; kind < 3; ++kind)
            for (auto& p : b.launch_events[kind]) {
                QSV_HIP(h, hipEventElapsedTime(&ms, p.first, p.second));
                h->prof.kernel_ms[kind] += ms;
            }
        // wall-clock window of the gate passes: with two streams the per-push intervals above overlap
        for (auto& p : b.pass_events) {
            QSV_HIP(h, hipEventElapsedTime(&ms, b.pass_events.front().first, p.second));
            h->prof.pass_window_ms = std::max(h->prof.pass_window_ms, double(ms));
        }
        for (auto& p : b.exp_events) {
            QSV_HIP(h, hipEventElapsedTime(&ms, p.first, p.second));
            h->prof.expect_ms += ms;
        }
    }
    return QSV_OK;
}

// Releases whatever a batch holds (events) and marks it closed; safe to call on error paths.
void eval_close(qsv_t* h) {
    qsv_handle::Batch& b = h->batch;
    for (auto* list : {&b.pass_events, &b.exp_events, &b.launch_events[0], &b.launch_events[1], &b.launch_events[2]}) {
        for (auto& p : *list) {
            if (p.first) (void)hipEventDestroy(p.first);
            if (p.second) (void)hipEventDestroy(p.second);
        }
        list->clear();
    }
    if (b.ev0) (void)hipEventDestroy(b.ev0);
    if (b.ev1) (void)hipEventDestroy(b.ev1);
    b.ev0 = b.ev1 = nullptr;
    if (b.snap_epoch != h->epoch) b.circs.clear();  // (kept with a layout the next batch may reuse)
    b.have_ids = false;
    b.repeat = false;
    b.open = false;
    h->out_target = nullptr;
    b.ways = 1;
    b.used_mask = 0;
    h->work = nullptr;
}

// where a batch without parameter values reads them from
const double kNoValues[1] = {0.0};

// A batch as the entry points take it: its circuits, each evaluation's parameter count, and the values packed back to back
// (the caller's vectors may have gaps between them).
struct BatchArgs {
    std::vector<Circuit*> circs;
    std::vector<int64_t> n_params;
    std::vector<double> values;
    // the values live in DEVICE memory instead (qsv_cvar_device): evaluation e's are row e of a row-major matrix whose row
    // length every entry of n_params holds, as qsv_eval_push_device documents; `values` is not looked at
    const double* device_values = nullptr;
};

// Looks up circuit_ids[0, n) and packs what each evaluation's param_offsets declare (params == nullptr: an empty array;
// param_offsets == nullptr: the ids only, for a call that runs nothing).  kept_refusal: circuits on kept states are refused
// with this message.
int resolve_batch(qsv_t* h, size_t n, const int* circuit_ids, const int64_t* param_offsets, const double* params, BatchArgs& out,
                  const char* kept_refusal = nullptr) {
    out.circs.assign(n, nullptr);
    out.n_params.assign(n, 0);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        auto it = h->circuits.find(circuit_ids[i]);
        if (it == h->circuits.end()) return fail(h, QSV_E_ARG, "unknown circuit id " + std::to_string(circuit_ids[i]));
        if (kept_refusal && it->second.prefix_id >= 0) return fail(h, QSV_E_UNSUPPORTED, kept_refusal);
        out.circs[i] = &it->second;
        if (!param_offsets) continue;
        out.n_params[i] = param_offsets[i + 1] - param_offsets[i];
        if (out.n_params[i] < 0) return fail(h, QSV_E_ARG, "param_offsets must be non-decreasing");
        total += size_t(out.n_params[i]);
    }
    out.values.assign(total + 1, 0.0);
    for (size_t i = 0, cur = 0; params && i < n; cur += size_t(out.n_params[i]), ++i)
        if (out.n_params[i]) std::memcpy(out.values.data() + cur, params + param_offsets[i], size_t(out.n_params[i]) * sizeof(double));
    return QSV_OK;
}

// The host forms of the gradient entry points hand the driver matrices.  pack_rows: the batch's parameter vectors as the rows
// of one zero-filled row-major matrix `base`, as wide as the longest of them (at least one value; `even`: rounded up to an even
// number of doubles), and out_width, the longest gradient request's -- evaluation e's is wrt_offsets[e + 1] - wrt_offsets[e]
// entries (wrt_offsets null: one per parameter of its circuit).  unpack_rows: the first so many entries of each row of `rows`,
// back to back into `out`.
int pack_rows(qsv_t* h, const BatchArgs& args, const int64_t* wrt_offsets, const double* out, bool even, int64_t& width, int64_t& out_width,
              std::vector<double>& base) {
    const size_t n = args.circs.size();
    auto row = [&](int64_t count) { return even ? (count + 1) / 2 * 2 : count; };
    int64_t total_out = 0;
    width = row(1);
    out_width = 1;
    for (size_t e = 0; e < n; ++e) {
        width = std::max(width, row(args.n_params[e]));
        const int64_t count = wrt_offsets ? wrt_offsets[e + 1] - wrt_offsets[e] : int64_t(args.circs[e]->n_params);
        if (count < 0) return fail(h, QSV_E_ARG, "wrt_offsets must be non-decreasing");
        out_width = std::max(out_width, count);
        total_out += count;
        if (args.n_params[e] < args.circs[e]->n_params) return too_few_values(h, args.circs[e]->n_params, args.n_params[e]);
    }
    if (total_out > 0 && !out) return fail(h, QSV_E_ARG, "out is null");
    if (width > (1 << 24) || out_width > (1 << 24)) return fail(h, QSV_E_ARG, "too many parameters");
    base.assign(n * size_t(width), 0.0);
    for (size_t e = 0, cur = 0; e < n; cur += size_t(args.n_params[e]), ++e)
        if (args.n_params[e]) std::memcpy(base.data() + e * size_t(width), args.values.data() + cur, size_t(args.n_params[e]) * sizeof(double));
    return QSV_OK;
}
void unpack_rows(const BatchArgs& args, const int64_t* wrt_offsets, const std::vector<double>& rows, int64_t out_width, double* out) {
    for (size_t e = 0, cur = 0; e < args.circs.size(); ++e) {
        const size_t count = size_t(wrt_offsets ? wrt_offsets[e + 1] - wrt_offsets[e] : int64_t(args.circs[e]->n_params));
        if (count) std::memcpy(out + cur, rows.data() + e * size_t(out_width), count * sizeof(double));
        cur += count;
    }
}
// The head of a host form that runs on rows in device memory: the points pack_rows packed (`base`, rows of `width`) go to
// `buffer`, and `args` become the forward run's arguments that read them there.
int rows_to_device(qsv_t* h, const BatchArgs& packed, const std::vector<double>& base, int64_t width, DeviceBuffer& buffer, int64_t& allocations,
                   BatchArgs& args) {
    int rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers may still be read or written by a call that did not wait)
    if ((rc = ensure_counted(h, buffer, base.size() * sizeof(double), allocations))) return rc;
    QSV_HIP(h, hipMemcpy(buffer.ptr, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice));
    args.circs = packed.circs;
    args.values.assign(1, 0.0);
    args.n_params.assign(packed.circs.size(), width);
    args.device_values = static_cast<const double*>(buffer.ptr);
    return QSV_OK;
}
// The tail of such a form: the output rows at d_rows (and `also`: further doubles from device memory into the caller's host
// arrays) come back, the streams are waited for, and the rows are unpacked into `out` as the call's wrt_offsets lay them out.
struct ReadBack {
    const void* src;
    double* dst;
    size_t count;
};
int rows_to_host(qsv_t* h, const BatchArgs& packed, const int64_t* wrt_offsets, const void* d_rows, int64_t out_width, double* out,
                 std::initializer_list<ReadBack> also = {}) {
    std::vector<double> rows(packed.circs.size() * size_t(out_width));
    QSV_HIP(h, hipMemcpyAsync(rows.data(), d_rows, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    for (const ReadBack& r : also)
        if (r.count) QSV_HIP(h, hipMemcpyAsync(r.dst, r.src, r.count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    QSV_HIP(h, sync_streams(h));
    h->async_pending = false;
    unpack_rows(packed, wrt_offsets, rows, out_width, out);
    return QSV_OK;
}

// One-shot evaluation: begin + one push + end.
int eval_all(qsv_t* h, const BatchArgs& args, double* out) {
    if (args.circs.empty()) return QSV_OK;
    int rc = eval_begin(h, args.circs, args.n_params);
    if (!rc) rc = eval_push(h, 0, args.circs.size(), args.values.data());
    if (!rc) rc = eval_end(h, out);
    eval_close(h);
    return rc;
}

// How run_to_states runs a batch: which circuits run split, the launch groups of split evaluations (side-table slots) and
// of the others (state slots), whether the pass kernel prepares every evaluation itself (one-tile registers) or the split
// ones only, and the run_group mode of each kind.
struct StateRun {
    SplitRule rule;
    size_t split_group, state_group;
    bool prepare_in_pass;
    uint32_t split_mode, state_mode;
};

// Runs a batch into state slots, for the entry points that need more of the final states than the expectation value: split
// evaluations first (order_split_first), in launch groups of their own, then the ordinary ones, then -- in groups of their
// own, which run_group requires -- those on kept states.  An evaluation's slot is its position in its launch group.  After
// each group, on_split / on_state(first, count) launches the caller's consumer of positions [first, first + count);
// batch.eval_at maps positions back to evaluations, also after the return.
//
// Two halves, so that a caller whose batch repeats (qsv_cvar_device) lays it out once: lay_out_states writes the staging
// buffer -- it waits for a batch that ended without waiting first, batch_layout --, run_laid_out only reads it.  Everything
// run_laid_out enqueues goes to the handle's own stream: run_group leaves it for the second lane or the chain stream only on the
// expectation routes (two_chains needs evaluations the launch of the virtual circuits finishes, which kModeSidesOnly has none of;
// h->work is null outside a push).
using GroupFn = std::function<int(size_t, size_t)>;
struct StateLayout {
    size_t n_split = 0;
    std::vector<std::pair<size_t, size_t>> groups;  // (first position, count) of every launch group
};
struct BatchRelease {  // what a batch run through these two holds: released on every exit path
    qsv_t* h;
    ~BatchRelease() {
        h->batch.circs.clear();
        h->batch.dev_params = nullptr;
        h->batch.repeat = false;
    }
};
int lay_out_states(qsv_t* h, const BatchArgs& args, const StateRun& run, StateLayout& lay) {
    const size_t n = args.circs.size();
    int rc = batch_layout(h, args.circs, args.n_params, run.rule);
    if (rc) return rc;
    size_t n_cont = 0;
    lay.n_split = order_split_first(h, 0, n, &n_cont);
    lay.groups.clear();
    auto cut = [&](size_t lo, size_t hi, size_t size) {
        for (size_t g0 = lo; g0 < hi; g0 += size) lay.groups.emplace_back(g0, std::min(size, hi - g0));
    };
    cut(0, lay.n_split, run.split_group);
    cut(lay.n_split, n - n_cont, run.state_group);
    cut(n - n_cont, n, run.state_group);
    EvalDesc* hd = static_cast<EvalDesc*>(h->h_batch);
    for (const auto& g : lay.groups)
        for (size_t j = g.first; j < g.first + g.second; ++j) {
            hd[j].state_slot = uint32_t(j - g.first);
            if (h->batch.split_any) hd[n + j].state_slot = uint32_t(j - g.first);
        }
    return ensure(h, h->d_partials, std::max<size_t>(1, n) * partials_per_state(h) * sizeof(double));
}
int run_laid_out(qsv_t* h, const BatchArgs& args, const StateRun& run, const StateLayout& lay, const GroupFn& on_split,
                 const GroupFn& on_state) {
    const size_t n = args.circs.size();
    int rc;
    // (rows in device memory: the descriptors' offsets are e * width, so the base is the matrix itself)
    h->batch.dev_params = args.device_values;
    if ((rc = batch_ship(h, 0, n, args.values.data(), run.prepare_in_pass ? n : lay.n_split))) return rc;
    for (const auto& g : lay.groups) {
        const bool split = g.first < lay.n_split;
        if ((rc = run_group(h, args.circs, g.first, g.second, split ? run.split_mode : run.state_mode))) return rc;
        const GroupFn& consume = split ? on_split : on_state;
        if (consume && (rc = consume(g.first, g.second))) return rc;
    }
    return QSV_OK;
}
int run_to_states(qsv_t* h, const BatchArgs& args, const StateRun& run, const GroupFn& on_split, const GroupFn& on_state) {
    BatchRelease release{h};
    StateLayout lay;
    h->prof = qsv_profile{};
    const int rc = lay_out_states(h, args, run, lay);
    return rc ? rc : run_laid_out(h, args, run, lay, on_split, on_state);
}

// The frame of a consumer of WHOLE final states (qsv_variance_circuits, qsv_observables_covariance, qsv_overlap_circuits): ordinary plans into state
// slots, never split (as qsv_prefix_create runs them), in launch groups of G; behind each group `launch`(first, count) queues
// the consumer's kernels on the handle's stream, which leave their results by position in device memory at `results`.  Those
// `count` doubles are in h_out when it returns, and batch.eval_at says whose they are; nothing of a failed call is still
// running.  Option "time_moments": each group's kernels are bracketed by events, and their device time goes to prof.expect_ms.
int run_whole_states(qsv_t* h, const BatchArgs& args, size_t G, const GroupFn& launch, const double* results, size_t count) {
    SpanTimer timer;
    auto group = [&](size_t g0, size_t gc) -> int {
        if (h->time_moments) QSV_HIP(h, timer.begin(h->stream));
        if (const int rc = launch(g0, gc)) return rc;
        if (h->time_moments) QSV_HIP(h, timer.end(h->stream));
        return QSV_OK;
    };
    const int rc = run_to_states(h, args, StateRun{SplitRule{}, 1, G, false, 0, kModeSynthFirst | kModeFinalStore}, {}, group);
    if (rc) {
        (void)sync_streams(h);
        return rc;
    }
    QSV_HIP(h, hipMemcpyAsync(h->h_out, results, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    QSV_HIP(h, sync_streams(h));
    QSV_HIP(h, timer.elapsed(0, h->prof.expect_ms));
    return QSV_OK;
}

// What qsv_cvar_device has and the host forms of the sampler branch do not: the ids and row width its layout is remembered
// by, and device memory for the results.  Such a call does not wait, so the next one that writes the staging buffer must
// (batch_layout, async_pending) -- unless it is the same batch again, the next iteration of a search: then the layout the last
// call left is used as it stands (handle: cvar_snap), the kernels read the descriptors from the device copy that call's kernels
// made (batch.repeat, descs_base), and the host neither writes a staging buffer nor waits.
struct DeviceCall {
    const int* ids;
    int width;
    bool sampled;
    double* out;
};
int run_states(qsv_t* h, const BatchArgs& args, const StateRun& run, const GroupFn& on_split, const GroupFn& on_state,
               const DeviceCall* dev) {
    if (!dev) return run_to_states(h, args, run, on_split, on_state);
    BatchRelease release{h};
    qsv_handle::CvarSnap& snap = h->cvar_snap;
    const size_t n = args.circs.size();
    StateLayout lay;
    h->prof = qsv_profile{};
    if (h->repeat_enabled && snap.epoch == h->epoch && snap.width == dev->width && snap.sampled == dev->sampled && snap.ids.size() == n &&
        std::equal(snap.ids.begin(), snap.ids.end(), dev->ids)) {
        h->batch.circs = args.circs;
        h->batch.repeat = true;
        lay.n_split = snap.n_split;
        lay.groups = snap.groups;
    } else {
        snap.epoch = 0;
        const int rc = lay_out_states(h, args, run, lay);
        if (rc) return rc;
        snap.ids.assign(dev->ids, dev->ids + n);
        snap.width = dev->width;
        snap.sampled = dev->sampled;
        snap.n_split = lay.n_split;
        snap.groups = lay.groups;
    }
    const int rc = run_laid_out(h, args, run, lay, on_split, on_state);
    snap.epoch = rc ? 0 : h->epoch;
    return rc;
}

// The final state of one circuit in slot 0 (statevector / probabilities).
int run_single_to_state(qsv_t* h, int circuit_id, const double* params, int n_params) {
    const int64_t offsets[2] = {0, std::max(0, n_params)};
    BatchArgs args;
    int rc = resolve_batch(h, 1, &circuit_id, offsets, params, args);
    if (!rc && n_params < 0)  // (a count, not offsets: refused as batch_layout refuses too few values)
        rc = too_few_values(h, args.circs[0]->n_params, n_params);
    if (!rc) rc = run_to_states(h, args, StateRun{SplitRule{}, 1, 1, false, 0, kModeSynthFirst | kModeFinalStore}, {}, {});
    return rc;
}

// ---- observable sets ---------------------------------------------------------------------------------------------------
// Largest set qsv_observables_create accepts, and the scratch one launch group of qsv_eval_observables may use for the partial
// sums of its strings (the group is made smaller to stay inside it)
constexpr uint32_t kMaxObsStrings = 1u << 16, kMaxObservables = 1u << 16;
constexpr int64_t kMaxObsEntries = int64_t(1) << 24;
constexpr size_t kObsScratchBytes = size_t(64) << 20;

void free_observable_set(ObservableSet& s) {
    for (DeviceBuffer* b : {&s.d_rows, &s.d_terms, &s.d_split_terms, &s.d_offsets, &s.d_term_of, &s.d_coef, &s.d_cov_first, &s.d_cov_groups,
                            &s.d_cov_terms})
        if (b->ptr) (void)hipFree(b->ptr);
    s = ObservableSet{};
}

void free_value_cache(ValueCache& c) {  // (the caller has waited for the handle's streams)
    if (c.d_keys) (void)hipFree(c.d_keys);
    if (c.d_vals) (void)hipFree(c.d_vals);
    for (DeviceBuffer* b : {&c.d_sample_slot, &c.d_miss_slots, &c.d_counters})
        if (b->ptr) (void)hipFree(b->ptr);
    if (c.h_miss) (void)hipHostFree(c.h_miss);
    if (c.h_values) (void)hipHostFree(c.h_values);
    if (c.h_counters) (void)hipHostFree(c.h_counters);
    c = ValueCache{};
}

int upload_bytes(qsv_t* h, DeviceBuffer& b, const void* src, size_t bytes) {
    int rc = ensure(h, b, bytes);
    if (rc) return rc;
    if (bytes) QSV_HIP(h, hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
    return QSV_OK;
}

// qsv_eval_observables with the lock held and the arguments checked.  An evaluation takes the split route when split_rule
// lets its circuit run split (the side tables); everything else takes the state route.  Each launch group's values land in the
// pinned result buffer at its positions, and the host puts the rows back in the caller's order.
int eval_observables_locked(qsv_t* h, const ObservableSet& set, const BatchArgs& args, double* out) {
    const size_t n_evals = args.circs.size();
    const SplitRule rule = split_rule(h, SplitUse::Observables);
    const size_t n_split = rule.count(args.circs);
    const size_t T = set.n_terms, M = set.n_obs;
    const size_t per_state = std::max<size_t>(1, T * size_t(set.nb)) * sizeof(double);
    const size_t G = std::max<size_t>(1, std::min(size_t(h->group), kObsScratchBytes / per_state));
    const size_t SG = std::max<size_t>(1, std::min(size_t(std::max(1, h->side_slots)), kObsScratchBytes / (std::max<size_t>(1, T) * 8)));
    int rc;
    if ((rc = ensure(h, h->d_obs_partials, G * per_state))) return rc;
    if ((rc = ensure(h, h->d_obs_values, std::max(G, n_split ? std::min(SG, n_split) : size_t(1)) * std::max<size_t>(1, T) * 8))) return rc;
    if ((rc = ensure_host_out(h, n_evals * M))) return rc;
    double* values = static_cast<double*>(h->d_obs_values.ptr);
    double* partials = static_cast<double*>(h->d_obs_partials.ptr);
    auto combine = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_observables_combine(values, uint32_t(T), int(gc), uint32_t(M), static_cast<const int64_t*>(set.d_offsets.ptr),
                                              static_cast<const uint32_t*>(set.d_term_of.ptr), static_cast<const double*>(set.d_coef.ptr),
                                              h->h_out + g0 * M, h->stream));
        return QSV_OK;
    };
    auto on_split = [&](size_t g0, size_t gc) -> int {
        PassArgs a{};
        a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
        a.evals = batch_evals(h) + g0;
        a.wtab = h->d_side.ptr;
        a.wtab_stride = h->side_stride;
        QSV_HIP(h, launch_split_term_values(h->dtype, unsigned(gc), static_cast<const FactorTerm*>(set.d_split_terms.ptr),
                                            uint32_t(T), values, h->stream, a));
        return combine(g0, gc);
    };
    auto on_state = [&](size_t g0, size_t gc) -> int {
        // (a set may have more rows than gridDim.y can be: slices of the rows, each row names its strings' places itself)
        for (int r0 = 0; r0 < set.n_rows; r0 += h->max_grid_y)
            QSV_HIP(h, launch_pauli_terms(h->dtype, h->d_states.ptr, uint64_t(1) << h->n, h->n, int(gc), std::min(h->max_grid_y, set.n_rows - r0),
                                          static_cast<const ObsRow*>(set.d_rows.ptr) + r0, static_cast<const ObsTerm*>(set.d_terms.ptr),
                                          uint32_t(T), set.nb, partials, h->stream));
        QSV_HIP(h, launch_pauli_terms_reduce(partials, set.nb, uint32_t(T), static_cast<const ObsTerm*>(set.d_terms.ptr), int(gc),
                                             values, h->stream));
        return combine(g0, gc);
    };
    const StateRun run{rule, SG, G, false, kModeSynthFirst | kModeFinalStore | kModeSidesOnly, kModeSynthFirst | kModeFinalStore};
    if ((rc = run_to_states(h, args, run, on_split, on_state))) return rc;
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    for (size_t j = 0; j < n_evals; ++j) std::memcpy(out + size_t(h->batch.eval_at[j]) * M, h->h_out + j * M, M * sizeof(double));
    return QSV_OK;
}


}  // namespace

extern "C" {

const char* qsv_version(void) { return "libqsv 0.1.0 (gfx950)"; }

// Not part of include/qsv.h: read-out of the per-phase cycle stamps of a diagnostic (-DQSV_STAMPS) build.
int qsv_debug_stamps(unsigned long long* out, int reset) {
    return qsv::read_stamps(out, reset) == hipSuccess ? QSV_OK : QSV_E_UNSUPPORTED;
}

// Likewise not part of include/qsv.h: the phase timeline of a -DQSV_TIMELINE build (scripts/timeline.py).
int qsv_debug_timeline(unsigned long long* out, size_t max_words, unsigned int* n_records, int reset) {
    return qsv::read_timeline(out, max_words, n_records, reset) == hipSuccess ? QSV_OK : QSV_E_UNSUPPORTED;
}

int qsv_create(int n_qubits, int dtype, int device, const qsv_plan_config* cfg, qsv_t** out) {
    if (!out) return fail(nullptr, QSV_E_ARG, "out is null");
    *out = nullptr;
    if (dtype != QSV_F64 && dtype != QSV_F32) return fail(nullptr, QSV_E_ARG, "dtype must be QSV_F64 or QSV_F32");
    PlanConfig pc;
    Geometry geo;
    try {
        pc = resolve_config(cfg, dtype, n_qubits);
        geo = make_geometry(n_qubits, pc);
    } catch (const std::exception& e) {
        return fail(nullptr, QSV_E_ARG, e.what());
    }
    if (geo.threads_launch > 512) return fail(nullptr, QSV_E_ARG, "tile_bits - reg_bits must be <= 9");
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0)
        return fail(nullptr, QSV_E_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= n_dev) return fail(nullptr, QSV_E_ARG, "device index out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, QSV_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));

    qsv_t* h = new qsv_t();
    h->n = n_qubits;
    h->dtype = dtype;
    h->device = device;
    h->cfg = pc;
    h->geo = geo;
    h->amp_bytes = size_t(pc.amp_bytes);
    const size_t state_bytes = (size_t(1) << n_qubits) * h->amp_bytes;
    int group = cfg && cfg->group > 0 ? cfg->group : 0;
    if (const char* env = getenv("QSV_GROUP")) group = atoi(env);
    if (group <= 0) {
        // Evaluations that run side by side in one launch.  Measured on MI355X (scripts/sweep.sh): the passes are
        // bound by fp64 issue and LDS traffic rather than by HBM, so keeping a group inside the 256 MiB Infinity
        // Cache buys nothing, while larger groups amortise launch ramp-up and tail: 2 GiB of resident states, at
        // most 256 evaluations (n = 16: 256, n = 20: 128, n = 24: 8, n >= 27: 1).
        const size_t budget = size_t(2) << 30;
        group = int(std::max<size_t>(1, std::min<size_t>(256, budget / state_bytes)));
    }
    h->group = group;
    // a workgroup sweeps two consecutive tiles once a launch has plenty of workgroups anyway (>= 4096 tiles)
    {
        const uint64_t tiles_per_launch = uint64_t(geo.blocks_per_state) * uint64_t(group);
        h->tiles_per_block = (tiles_per_launch >= 4096 && geo.blocks_per_state >= 2) ? 2 : 1;
    }
    h->tiles_per_block_later = h->tiles_per_block;
    if (const char* env = getenv("QSV_TILES_PER_BLOCK")) h->tiles_per_block = h->tiles_per_block_later = std::max(1, atoi(env));
    if (const char* env = getenv("QSV_TILES_PER_BLOCK_LATER")) h->tiles_per_block_later = std::max(1, atoi(env));
    auto bail = [&](hipError_t err, const char* what) {
        std::string msg = std::string(what) + ": " + hipGetErrorString(err);
        qsv_destroy(h);
        return fail(nullptr, QSV_E_DEVICE, msg);
    };
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    h->own_stream = true;
    if (const char* env = getenv("QSV_SPLIT")) h->split_enabled = atoi(env) != 0;
    if (const char* env = getenv("QSV_SPLIT_SAMPLE")) h->split_sampling = atoi(env) != 0;
    if (const char* env = getenv("QSV_FACTOR")) h->factor_enabled = atoi(env) != 0;
    if (getenv("QSV_NO_FUSED_FACTOR")) h->fused_factor = false;
    if (const char* env = getenv("QSV_CHAIN_STREAM")) h->chain_enabled = atoi(env) != 0;
    if (const char* env = getenv("QSV_POLL")) h->poll_results = atoi(env) != 0;
    if (const char* env = getenv("QSV_REPEAT")) h->repeat_enabled = atoi(env) != 0;
    if (const char* env = getenv("QSV_REPLAY")) h->replay_enabled = atoi(env) != 0;
    if (const char* env = getenv("QSV_HOST_TIMING")) h->timing.on = atoi(env) != 0;
    if (const char* env = getenv("QSV_REPEAT_DESCS")) h->repeat_device_descs = atoi(env) != 0;
    if (const char* env = getenv("QSV_FUSED_LDS")) h->fused_lds_table = atoi(env) != 0;
    if (const char* env = getenv("QSV_SIDE_PREPARE")) h->side_prepare = atoi(env) != 0;
    if (const char* env = getenv("QSV_SIDE_DIAG")) h->side_diag = atoi(env) != 0;
    if (const char* env = getenv("QSV_SIDES_R3")) h->sides_r3 = atoi(env) != 0;
    if (const char* env = getenv("QSV_FINAL_CONTROLS")) h->final_controls = atoi(env) != 0;
    if (const char* env = getenv("QSV_LIVE_ENTRIES")) h->live_entries = atoi(env) != 0;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_cus = cus;
        int grid_y = 0;
        if (hipDeviceGetAttribute(&grid_y, hipDeviceAttributeMaxGridDimY, device) == hipSuccess && grid_y > 0)
            h->max_grid_y = h->device_max_grid_y = grid_y;
    }
    {
        int large_bar = 0;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess) large_bar = 0;
        // (measured, n = 20, 64 evaluations: the launch is 1.4 us shorter with the descriptors local -- 54.4 -> 53.0 us --, the
        // step is not, 73.8 -> 73.6 us: off unless asked for)
        h->bar_ship = false;
        if (const char* env = getenv("QSV_BAR")) h->bar_ship = large_bar != 0 && atoi(env) != 0;
    }
    if (const char* env = getenv("QSV_SPLIT_MAX_KEYS")) h->split_max_keys = std::max(0, std::min(kMaxSplitKeys, atoi(env)));
    h->stream_mode = state_bytes > (size_t(256) << 20) ? uint32_t(kModeStreaming) : 0u;
    if (const char* env = getenv("QSV_STREAMING")) h->stream_mode = atoi(env) ? uint32_t(kModeStreaming) : 0u;
    if (const char* env = getenv("QSV_STREAMS")) h->n_streams = std::max(1, std::min(4, atoi(env)));
    for (int i = 1; i < std::max(2, h->n_streams); ++i) {  // (the lanes' streams; the auxiliary one on first need)
        hipStream_t st = nullptr;
        if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
        h->side_streams.push_back(st);
    }
    h->n_lane_streams = int(h->side_streams.size());
    if ((e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipMalloc(&h->d_states.ptr, state_bytes * size_t(group))) != hipSuccess) return bail(e, "hipMalloc(states)");
    h->d_states.bytes = state_bytes * size_t(group);
    // compact tables: at most 2^kMaxCompactBits tiles per slot, never more than a state
    h->wtab_stride = std::min<uint64_t>(uint64_t(1) << n_qubits, uint64_t(1) << (geo.k + int(kMaxCompactBits)));
    if ((e = hipMalloc(&h->d_wtab.ptr, size_t(h->wtab_stride) * h->amp_bytes * size_t(group))) != hipSuccess)
        return bail(e, "hipMalloc(compact tables)");
    h->d_wtab.bytes = size_t(h->wtab_stride) * h->amp_bytes * size_t(group);
    if (h->split_enabled && n_qubits > geo.k && n_qubits <= 28) {
        // side tables of split evaluations: two virtual circuits of at most tile + kSideExtraBits qubits per slot
        h->side_stride = uint64_t(2) << (geo.k + kSideExtraBits);
        // (a lane's split evaluations run in launch groups of its share of the slots: with 128 slots config 3's step --
        // 256 evaluations at 24 qubits, two lanes -- was four groups of 64, two chains of launches per lane; with 256 it is
        // one per lane: 0.276 -> 0.211 ms.  4 MiB per slot at 13-qubit tiles.)
        h->side_slots = 256;
        if (const char* env = getenv("QSV_SIDE_SLOTS")) h->side_slots = std::max(8, std::min(1024, atoi(env)));
        if ((e = hipMalloc(&h->d_side.ptr, size_t(h->side_stride) * h->amp_bytes * size_t(h->side_slots))) != hipSuccess)
            return bail(e, "hipMalloc(side tables)");
        h->d_side.bytes = size_t(h->side_stride) * h->amp_bytes * size_t(h->side_slots);
        if (h->factor_enabled) {
            const size_t bytes = factor_slot_doubles() * sizeof(double) * size_t(h->side_slots);
            if ((e = hipMalloc(&h->d_factor.ptr, bytes)) != hipSuccess) return bail(e, "hipMalloc(partial Gram matrices)");
            h->d_factor.bytes = bytes;
            const size_t cbytes = sizeof(uint32_t) * size_t(kFactorCountersPerSlot) * size_t(h->side_slots);
            if ((e = hipMalloc(&h->d_factor_count.ptr, cbytes)) != hipSuccess) return bail(e, "hipMalloc(hand-off counters)");
            h->d_factor_count.bytes = cbytes;
            if ((e = hipMemset(h->d_factor_count.ptr, 0, cbytes)) != hipSuccess) return bail(e, "hipMemset(hand-off counters)");
        }
    }
    {
        // the most dynamic LDS a pass launch of this handle may ask for: the exchange plane of the largest tile (a side of a
        // split circuit may have a tile one qubit larger than the handle's), the fused preparation, the fused factor tail
        const int side_tile = std::max(geo.k, std::min(geo.r + 9, int(kMaxTileBits)));
        const size_t plane = (size_t(1) << side_tile) * h->amp_bytes / (pc.xmode == 2 ? 2 : 1);
        const size_t most = std::max({geo.lds_bytes, plane, kFusedPrepareLdsBytes, kFusedFactorLdsBytes, kFusedLdsTableEnd});
        if ((e = configure_pass_kernels(dtype, geo.r, pc.xmode, most)) != hipSuccess) return bail(e, "hipFuncSetAttribute");
        // (sides of split circuits may run with eight amplitudes per thread whatever the handle's own geometry: build_circuit)
        if (geo.r != 3 && (e = configure_pass_kernels(dtype, 3, pc.xmode, most)) != hipSuccess) return bail(e, "hipFuncSetAttribute");
    }
    *out = h;
    return QSV_OK;
}

void qsv_destroy(qsv_t* h) {
    if (!h) return;
    if (getenv("QSV_COALESCE_DEBUG") && h->cq_batches)
        fprintf(stderr, "qsv_eval_coalesced: %llu batches, last expectation %zu\n", (unsigned long long)h->cq_batches, h->cq_expected);
    if (h->timing.on && h->timing.calls) {
        const qsv_handle::HostTiming& t = h->timing;
        const double per = 1.0 / double(t.calls);
        fprintf(stderr,
                "qsv host timing over %llu qsv_eval_begin calls (%llu replayed pushes), us per call: begin %.2f  push without launch calls %.2f  "
                "launch calls %.2f  end and poll %.2f  copy-out %.2f\n",
                (unsigned long long)t.calls, (unsigned long long)t.replays, t.begin_us * per, (t.push_us - t.launch_us) * per,
                t.launch_us * per, (t.end_us - t.copy_us) * per, t.copy_us * per);
    }
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipStream_t st : h->side_streams) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (DeviceBuffer* b : {&h->d_z, &h->d_cre, &h->d_diag, &h->d_order, &h->d_sorted, &h->d_term_partials, &h->d_groups, &h->d_term_odd, &h->d_arena,
                            &h->d_states, &h->d_wtab, &h->d_side, &h->d_factor, &h->d_factor_count, &h->d_factor_big, &h->d_factor_big_count, &h->d_quad, &h->d_fterms, &h->d_fpart, &h->d_batch, &h->d_mats, &h->d_partials, &h->d_out, &h->d_scratch, &h->d_prefix, &h->d_sdiag,
                            &h->d_obs_partials, &h->d_obs_values, &h->d_grad_tab, &h->d_grad_rows, &h->d_grad_values, &h->d_grad_base,
                            &h->d_grad_out, &h->d_adj_lambda, &h->d_adj_tab, &h->d_adj_mats, &h->d_adj_partials, &h->d_adj_epart, &h->d_adj_base,
                            &h->d_adj_out, &h->d_adj_values, &h->d_defl, &h->d_defl_out, &h->d_cvar_grad, &h->d_fold, &h->d_fold_r, &h->d_moments, &h->d_cov, &h->d_overlap, &h->d_rdm, &h->d_opdm,
                            &h->d_met_scratch, &h->d_met_tab, &h->d_met_mats, &h->d_met_partials, &h->d_met_base, &h->d_met_out})
        if (b->ptr) (void)hipFree(b->ptr);
    for (auto& kv : h->obs_sets) free_observable_set(kv.second);
    for (auto& kv : h->value_caches) free_value_cache(kv.second);
    if (h->h_batch) (void)hipHostFree(h->h_batch);
    if (h->d_ship) (void)hipFree(h->d_ship);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_out) (void)hipHostFree(h->h_out);
    if (h->h_samples) (void)hipHostFree(h->h_samples);
    if (h->h_grad_tab) (void)hipHostFree(h->h_grad_tab);
    for (auto& plan : h->grad_plans)
        if (plan.second.d_tab) (void)hipFree(plan.second.d_tab);
    if (h->ev_grad) (void)hipEventDestroy(h->ev_grad);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* qsv_last_error(const qsv_t* h) {
    if (!h) return g_create_error.c_str();
    return g_handle_error_owner == h ? g_handle_error.c_str() : "";
}

int qsv_set_stream(qsv_t* h, void* hip_stream) {
    QSV_OPEN(h, "qsv_set_stream", kDevice);
    h->epoch += 1;
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    if (h->own_stream) {
        (void)hipStreamDestroy(h->stream);
        h->own_stream = false;
    }
    if (hip_stream) {
        h->stream = static_cast<hipStream_t>(hip_stream);
    } else {
        QSV_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return QSV_OK;
}

int qsv_n_qubits(const qsv_t* h) { return h ? h->n : QSV_E_ARG; }
int qsv_group_size(const qsv_t* h) { return h ? h->group : QSV_E_ARG; }

int qsv_set_operator(qsv_t* h, int n_terms, const uint64_t* x_mask, const uint64_t* z_mask, const double* coeff_re,
                     const double* coeff_im) {
    QSV_OPEN(h, "qsv_set_operator", kDevice);
    h->epoch += 1;
    if (n_terms < 1 || !x_mask || !z_mask || !coeff_re) return fail(h, QSV_E_ARG, "operator needs at least one term");
    (void)coeff_im;  // <P_k> is real for every Pauli string, so real(<H>) only needs the real parts
    const uint64_t limit = (uint64_t(1) << h->n) - 1;
    for (int k = 0; k < n_terms; ++k)
        if ((x_mask[k] | z_mask[k]) & ~limit) return fail(h, QSV_E_ARG, "Pauli term acts on a qubit >= n_qubits");
    // ---- split into the diagonal part (x = 0) and x-mask groups of the rest -------------------------------
    std::vector<uint64_t> diag_z, off_z;
    std::vector<double> diag_c, off_c;
    std::vector<uint32_t> off_odd;
    std::vector<PauliGroup> groups;
    std::vector<int> order;
    for (int k = 0; k < n_terms; ++k) {
        if (x_mask[k] == 0) {
            diag_z.push_back(z_mask[k]);
            diag_c.push_back(coeff_re[k]);
        } else {
            order.push_back(k);
        }
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return x_mask[a] < x_mask[b]; });
    for (int k : order) {
        const uint64_t x = x_mask[k];
        if (groups.empty() || groups.back().x != x) {
            PauliGroup g{};
            g.x = x;
            g.first = uint32_t(off_z.size());
            g.count = 0;
            g.pivot = uint32_t(63 - __builtin_clzll(x));
            groups.push_back(g);
        }
        groups.back().count += 1;
        const int ny = __builtin_popcountll(x & z_mask[k]);
        off_z.push_back(z_mask[k]);
        off_odd.push_back(uint32_t(ny & 1));
        off_c.push_back(((ny >> 1) & 1) ? -coeff_re[k] : coeff_re[k]);  // (-1)^{floor(ny/2)}
    }
    int rc;
    const bool all_diag = groups.empty();
    if (!diag_z.empty()) {
        DeviceBuffer tmp_z, tmp_c;
        const size_t mb = diag_z.size() * 8;
        if ((rc = ensure(h, tmp_z, mb)) || (rc = ensure(h, tmp_c, mb))) return rc;
        QSV_HIP(h, hipMemcpyAsync(tmp_z.ptr, diag_z.data(), mb, hipMemcpyHostToDevice, h->stream));
        QSV_HIP(h, hipMemcpyAsync(tmp_c.ptr, diag_c.data(), mb, hipMemcpyHostToDevice, h->stream));
        if ((rc = ensure(h, h->d_diag, (size_t(1) << h->n) * sizeof(double)))) return rc;
        QSV_HIP(h, launch_diag_table(h->n, int(diag_z.size()), static_cast<const uint64_t*>(tmp_z.ptr),
                                     static_cast<const double*>(tmp_c.ptr), static_cast<double*>(h->d_diag.ptr),
                                     h->stream));
        QSV_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(tmp_z.ptr);
        (void)hipFree(tmp_c.ptr);
    }
    if (!all_diag) {
        const size_t nt = off_z.size();
        if ((rc = ensure(h, h->d_z, nt * 8)) || (rc = ensure(h, h->d_cre, nt * 8)) ||
            (rc = ensure(h, h->d_term_odd, nt * 4)) || (rc = ensure(h, h->d_groups, groups.size() * sizeof(PauliGroup))))
            return rc;
        QSV_HIP(h, hipMemcpyAsync(h->d_z.ptr, off_z.data(), nt * 8, hipMemcpyHostToDevice, h->stream));
        QSV_HIP(h, hipMemcpyAsync(h->d_cre.ptr, off_c.data(), nt * 8, hipMemcpyHostToDevice, h->stream));
        QSV_HIP(h, hipMemcpyAsync(h->d_term_odd.ptr, off_odd.data(), nt * 4, hipMemcpyHostToDevice, h->stream));
        QSV_HIP(h, hipMemcpyAsync(h->d_groups.ptr, groups.data(), groups.size() * sizeof(PauliGroup),
                                  hipMemcpyHostToDevice, h->stream));
        const uint64_t n_pairs = uint64_t(1) << (h->n - 1);
        // enough workgroups per group to fill the chip once the group count is accounted for
        const uint64_t want = std::max<uint64_t>(1, 2048 / std::max<size_t>(1, groups.size()));
        h->pauli_nb = int(std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, 1024), n_pairs / 256 + 1)));
        if ((rc = ensure(h, h->d_term_partials, size_t(h->group) * groups.size() * size_t(h->pauli_nb) * 8))) return rc;
        QSV_HIP(h, hipStreamSynchronize(h->stream));
    }
    // quadratic diagonal operators: the couplings as a dense matrix (split evaluations then factorise, launch_factor)
    h->quadratic = false;
    if (all_diag) {
        bool quadratic = true;
        std::vector<double> quad(size_t(h->n) * size_t(h->n), 0.0);
        for (size_t k = 0; k < diag_z.size() && quadratic; ++k) {
            const int weight = __builtin_popcountll(diag_z[k]);
            if (weight > 2) quadratic = false;
            if (weight == 2) {
                const int a = __builtin_ctzll(diag_z[k]), b = 63 - __builtin_clzll(diag_z[k]);
                quad[size_t(a) * size_t(h->n) + size_t(b)] += diag_c[k];
                quad[size_t(b) * size_t(h->n) + size_t(a)] += diag_c[k];
            }
        }
        if (quadratic) {
            if ((rc = ensure(h, h->d_quad, quad.size() * sizeof(double)))) return rc;
            QSV_HIP(h, hipMemcpyAsync(h->d_quad.ptr, quad.data(), quad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            QSV_HIP(h, hipStreamSynchronize(h->stream));
            h->quadratic = true;
        }
    }
    // general operators: the terms as a plain list (split evaluations then need no state either, launch_factor_terms)
    h->n_fterms = 0;
    if (!all_diag && h->n <= 32) {
        std::vector<FactorTerm> list(size_t(n_terms), FactorTerm{0, 0, 0.0});
        for (int k = 0; k < n_terms; ++k) list[size_t(k)] = FactorTerm{uint32_t(x_mask[k]), uint32_t(z_mask[k]), coeff_re[k]};
        if ((rc = ensure(h, h->d_fterms, list.size() * sizeof(FactorTerm)))) return rc;
        QSV_HIP(h, hipMemcpyAsync(h->d_fterms.ptr, list.data(), list.size() * sizeof(FactorTerm), hipMemcpyHostToDevice, h->stream));
        QSV_HIP(h, hipStreamSynchronize(h->stream));
        h->n_fterms = uint32_t(n_terms);
    }
    // (plans in the arena name tables of the OLD operator's D: everything is uploaded again when it is next used)
    QSV_HIP(h, sync_streams(h));
    for (auto& kv : h->circuits) kv.second.uploaded = false;
    h->sdiag_used = 0;
    h->n_terms = n_terms;
    h->order_valid = false;
    h->diagonal = all_diag;
    h->has_diag_part = !diag_z.empty();
    h->n_groups = int(groups.size());
    return QSV_OK;
}

int qsv_circuit_create(qsv_t* h, int n_ops, const qsv_op* ops, int n_params, int* out_circuit_id) {
    if (!h) return QSV_E_ARG;
    if (!out_circuit_id || n_params < 0) return fail(h, QSV_E_ARG, "bad arguments");
    // the scheduler runs outside the handle lock: callers on several threads register structures side by side
    Circuit c;
    std::string err;
    int rc = build_circuit(h, n_ops, ops, n_params, true, &c, &err);
    if (rc) return fail(h, rc, err);
    QSV_OPEN(h, "qsv_circuit_create", kHostOnly);
    h->epoch += 1;
    *out_circuit_id = insert_circuit(h, std::move(c));
    return QSV_OK;
}

int qsv_circuits_create(qsv_t* h, int n_circuits, const int64_t* op_offsets, const qsv_op* ops, const int* n_params,
                        int* out_circuit_ids) {
    if (!h) return QSV_E_ARG;
    if (n_circuits < 0 || (n_circuits > 0 && (!op_offsets || !n_params || !out_circuit_ids)))
        return fail(h, QSV_E_ARG, "bad arguments");
    for (int i = 0; i < n_circuits; ++i)
        if (op_offsets[i + 1] < op_offsets[i] || n_params[i] < 0) return fail(h, QSV_E_ARG, "bad offsets or parameter counts");
    std::vector<BuiltCircuit> built;
    build_many(h, size_t(n_circuits), [&](size_t i, BuiltCircuit& b) {
        b.rc = build_circuit(h, int(op_offsets[i + 1] - op_offsets[i]), ops + op_offsets[i], n_params[i], true, &b.circuit, &b.err);
    }, built);
    for (int i = 0; i < n_circuits; ++i)
        if (built[size_t(i)].rc) return fail(h, built[size_t(i)].rc, built[size_t(i)].err + " (circuit " + std::to_string(i) + ")");
    QSV_OPEN(h, "qsv_circuits_create", kHostOnly);
    h->epoch += 1;
    for (int i = 0; i < n_circuits; ++i) out_circuit_ids[i] = insert_circuit(h, std::move(built[size_t(i)].circuit));
    return QSV_OK;
}

int qsv_circuit_destroy(qsv_t* h, int circuit_id) {
    QSV_OPEN(h, "qsv_circuit_destroy", kHostOnly);
    h->epoch += 1;
    auto it = h->circuits.find(circuit_id);
    if (it == h->circuits.end()) return fail(h, QSV_E_ARG, "unknown circuit id");
    if (it->second.prefix_id >= 0) prefix_unref(h, it->second.prefix_id);
    h->circuits.erase(it);
    // the arena space is reclaimed when the arena is next rebuilt
    return QSV_OK;
}

// ---- kept states ---------------------------------------------------------------------------------------------------------
// (reference: mutation.py:57-59 -- optimize_layer_of_individual evaluates get_partially_parameterized_quantum_circuit({layer_id})
// over and over: everything in front of that layer is the same state in every evaluation of the search)

int qsv_prefix_create(qsv_t* h, int n_states, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                      int* out_prefix_ids) {
    QSV_OPEN(h, "qsv_prefix_create", kDevice);
    if (n_states < 0 || (n_states > 0 && (!circuit_ids || !param_offsets || !out_prefix_ids))) return fail(h, QSV_E_ARG, "bad arguments");
    if (n_states == 0) return QSV_OK;
    const size_t n = size_t(n_states);
    BatchArgs args;
    int rc = resolve_batch(h, n, circuit_ids, param_offsets, params, args, "a kept state of a circuit that itself continues a kept state");
    if (rc) return rc;
    // room for n more states
    const size_t state_bytes = (size_t(1) << h->n) * h->amp_bytes;
    const size_t fresh_needed = n > h->prefix_free.size() ? n - h->prefix_free.size() : 0;
    if (h->prefix_used + fresh_needed > h->prefix_slots) {
        const size_t want = h->prefix_used + fresh_needed;
        size_t cap = std::max(want, h->prefix_slots * 2);
        void* fresh = nullptr;
        hipError_t e = hipMalloc(&fresh, cap * state_bytes);
        if (e != hipSuccess && cap > want) {
            (void)hipGetLastError();
            cap = want;
            e = hipMalloc(&fresh, cap * state_bytes);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, QSV_E_DEVICE, std::string("hipMalloc(kept states): ") + hipGetErrorString(e));
        }
        if (h->d_prefix.ptr) {
            hipError_t e2 = sync_streams(h);  // (nothing may still read the old buffer)
            if (e2 == hipSuccess && h->prefix_used)
                e2 = hipMemcpy(fresh, h->d_prefix.ptr, h->prefix_used * state_bytes, hipMemcpyDeviceToDevice);
            if (e2 != hipSuccess) {
                (void)hipFree(fresh);
                return fail(h, QSV_E_DEVICE, std::string("moving the kept states: ") + hipGetErrorString(e2));
            }
            (void)hipFree(h->d_prefix.ptr);
        }
        h->d_prefix.ptr = fresh;
        h->d_prefix.bytes = cap * state_bytes;
        h->prefix_slots = cap;
    }
    // (kept slots are taken once the batch is laid out and run: a batch refused before that leaves them as they were)
    std::vector<uint32_t> slots;
    auto give_back = [&]() {
        if (slots.empty()) return;
        for (uint32_t sl : slots) h->prefix_free.push_back(sl);
        (void)sync_streams(h);  // (copies into them may still be queued)
    };
    // the circuits run their ordinary plans (a state is wanted, not an expectation value), a launch group at a time, on the
    // handle's stream; each final state is copied from its slot of the group to its kept slot
    auto keep = [&](size_t g0, size_t gc) -> int {
        for (size_t i = slots.size(); i < n; ++i) {
            if (!h->prefix_free.empty()) {
                slots.push_back(h->prefix_free.back());
                h->prefix_free.pop_back();
            } else {
                slots.push_back(uint32_t(h->prefix_used++));
            }
        }
        for (size_t j = g0; j < g0 + gc; ++j) {
            hipError_t e = hipMemcpyAsync(static_cast<char*>(h->d_prefix.ptr) + size_t(slots[h->batch.eval_at[j]]) * state_bytes,
                                          static_cast<const char*>(h->d_states.ptr) + (j - g0) * state_bytes, state_bytes,
                                          hipMemcpyDeviceToDevice, h->stream);
            if (e != hipSuccess) return fail(h, QSV_E_DEVICE, std::string("hipMemcpyAsync(kept state): ") + hipGetErrorString(e));
        }
        return QSV_OK;
    };
    if ((rc = run_to_states(h, args, StateRun{SplitRule{}, 1, size_t(h->group), false, 0, kModeSynthFirst | kModeFinalStore}, {}, keep))) {
        give_back();
        return rc;
    }
    // (the staging buffers this batch's preparation read are free again, and whatever stream continues a kept state finds it)
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        give_back();
        return fail(h, QSV_E_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    for (size_t i = 0; i < n; ++i) {
        const int id = h->next_prefix_id++;
        h->prefixes.emplace(id, PrefixState{slots[i], 0, false});
        out_prefix_ids[i] = id;
    }
    return QSV_OK;
}

int qsv_prefix_destroy(qsv_t* h, int n_states, const int* prefix_ids) {
    if (!h) return QSV_E_ARG;
    if (n_states < 0 || (n_states > 0 && !prefix_ids)) return fail(h, QSV_E_ARG, "bad arguments");
    // (finalizers of host objects call this: the opening keeps it from waiting for a handle its own thread holds between begin and end)
    QSV_OPEN(h, "qsv_prefix_destroy", kHostOnly);
    int rc = QSV_OK;
    for (int i = 0; i < n_states; ++i) {
        auto it = h->prefixes.find(prefix_ids[i]);
        if (it == h->prefixes.end() || it->second.released) {
            rc = fail(h, QSV_E_ARG, "unknown kept state " + std::to_string(prefix_ids[i]));
            continue;
        }
        it->second.released = true;
        if (it->second.refs == 0) {
            h->prefix_free.push_back(it->second.slot);
            h->prefixes.erase(it);
        }
    }
    return rc;
}

int qsv_prefix_count(const qsv_t* h) {
    QSV_OPEN(h, "qsv_prefix_count", kHostOnly);
    return int(h->prefixes.size());
}

static int create_on_prefixes(qsv_t* h, const char* name, int n_circuits, const int64_t* op_offsets, const qsv_op* ops, const int* n_params,
                              const int* prefix_ids, int* out_circuit_ids) {
    if (!h) return QSV_E_ARG;
    if (n_circuits < 0 || (n_circuits > 0 && (!op_offsets || !n_params || !prefix_ids || !out_circuit_ids)))
        return fail(h, QSV_E_ARG, "bad arguments");
    for (int i = 0; i < n_circuits; ++i)
        if (op_offsets[i + 1] < op_offsets[i] || n_params[i] < 0) return fail(h, QSV_E_ARG, "bad offsets or parameter counts");
    // unfolded plans (the input is an arbitrary state, not a product state), never split
    std::vector<BuiltCircuit> built;
    build_many(h, size_t(n_circuits), [&](size_t i, BuiltCircuit& b) {
        b.rc = build_circuit(h, int(op_offsets[i + 1] - op_offsets[i]), ops + op_offsets[i], n_params[i], false, &b.circuit, &b.err);
    }, built);
    for (int i = 0; i < n_circuits; ++i)
        if (built[size_t(i)].rc) return fail(h, built[size_t(i)].rc, built[size_t(i)].err + " (circuit " + std::to_string(i) + ")");
    QSV_OPEN(h, name, kHostOnly);
    for (int i = 0; i < n_circuits; ++i) {
        auto it = h->prefixes.find(prefix_ids[i]);
        if (it == h->prefixes.end() || it->second.released) return fail(h, QSV_E_ARG, "unknown kept state " + std::to_string(prefix_ids[i]));
    }
    h->epoch += 1;
    for (int i = 0; i < n_circuits; ++i) {
        built[size_t(i)].circuit.prefix_id = prefix_ids[i];
        h->prefixes.find(prefix_ids[i])->second.refs += 1;
        out_circuit_ids[i] = insert_circuit(h, std::move(built[size_t(i)].circuit));
    }
    return QSV_OK;
}

int qsv_circuits_create_on_prefixes(qsv_t* h, int n_circuits, const int64_t* op_offsets, const qsv_op* ops, const int* n_params,
                                    const int* prefix_ids, int* out_circuit_ids) {
    return create_on_prefixes(h, "qsv_circuits_create_on_prefixes", n_circuits, op_offsets, ops, n_params, prefix_ids, out_circuit_ids);
}

int qsv_circuit_create_on_prefix(qsv_t* h, int prefix_id, int n_ops, const qsv_op* ops, int n_params, int* out_circuit_id) {
    const int64_t offsets[2] = {0, n_ops};
    return create_on_prefixes(h, "qsv_circuit_create_on_prefix", 1, offsets, ops, &n_params, &prefix_id, out_circuit_id);
}

// Whether the one-launch route runs `c` on its reduced form under the operator set now: what run_group decides through side_form
// (eval_begin lays a batch out for reduced sides where reduced_route holds); before an operator is set, what it would decide
// under a quadratic one.
static bool runs_reduced(const qsv_t* h, const Circuit& c) {
    return c.split.fused && c.reduced.ok && (h->n_terms == 0 ? h->fused_factor && h->final_controls : reduced_route(h));
}

static int circuit_cost_locked(qsv_t* h, int circuit_id, qsv_circuit_cost_t* out) {
    auto it = h->circuits.find(circuit_id);
    if (it == h->circuits.end()) return fail(h, QSV_E_ARG, "unknown circuit id");
    Circuit& c = it->second;
    *out = qsv_circuit_cost_t{};
    // which way an expectation value of this circuit goes under the operator set now
    const double scale = std::ldexp(1.0, h->n - 20) * (h->dtype == QSV_F64 ? 1.0 : 0.5);
    if (split_rule(h, SplitUse::Expectation).takes(c)) {
        const bool one_launch = c.split.fused && h->fused_factor && (h->n_terms == 0 || factor_path(h));
        // (the one-launch route runs the reduced form of a circuit that has one: its sizes are what the launch costs)
        const SplitInfo& sp = one_launch && runs_reduced(h, c) ? c.reduced : c.split;
        out->route = one_launch ? QSV_ROUTE_SPLIT_ONE_LAUNCH : QSV_ROUTE_SPLIT;
        out->n_keys = sp.n_keys;
        out->n_passes = std::max(sp.stats[0].n_passes, sp.stats[1].n_passes);
        // measured at 20 qubits (profiles/r03_split_by_depth.txt, r03_chain_stream.txt): one launch of 64 evaluations 49 us; own
        // launches 1.2 us per evaluation up to three keys, 16 / 32 product terms 5 / 9 us; sides larger than 2^10 cost in proportion
        const double sides = 0.5 * (std::ldexp(1.0, sp.n_virtual[0] - sp.n_keys - 10) + std::ldexp(1.0, sp.n_virtual[1] - sp.n_keys - 10));
        const double per = one_launch ? 0.8 : (sp.n_keys <= 3 ? 1.2 : (sp.n_keys == 4 ? 5.0 : 9.0));
        out->microseconds = per * std::max(1.0, sides) * double(out->n_passes);
        return QSV_OK;
    }
    int rc = ensure_plan(h, c);
    if (rc) return rc;
    out->n_passes = c.plan.stats.n_passes;
    out->on_kept_state = c.prefix_id >= 0 ? 1 : 0;
    if (h->geo.blocks_per_state == 1) {
        out->route = QSV_ROUTE_ONE_TILE;
        out->microseconds = 1.0;
        return QSV_OK;
    }
    out->route = QSV_ROUTE_PASSES;
    // a pass over a 2^20 state inside a full launch, measured (profiles/r04_prefix_reuse.txt): a deep individual's whole circuit
    // 17.1 us per evaluation at 3.13 passes = 5.5 us per pass (the synthesising, compact first pass included); on a kept state
    // 10.5 - 11 us at 1.89 passes, 18.4 at 2.8: 5.8 - 6.6 us per pass -- few gates, but every pass reads and writes the whole state
    // (HBM bound: 56 MiB per two-pass evaluation at 5.3 TB/s); n = 24: 16 times both
    // ... refitted at the end of round 4 (scripts/prefix_cache_experiment.py after the scheduler's tile search): a pass that
    // moves the state costs 4.2 us at 20 qubits, a scheduled gate entry 0.09 us on top, a synthesising first pass 1 us and no
    // state traffic: whole eight-layer circuit 2.98 passes, 78 entries -> 15 us (14.6 measured); seven layers 13.4 (13.5); a last
    // layer on a kept state 1.89 passes, 15 entries -> 9.3 (9.6); the upper four of eight layers 2.02 passes, 70 entries -> 14.8
    // (14.8: as dear as the whole circuit, which is why a search in the middle keeps it)
    {
        const bool synth = c.prefix_id < 0;
        const double moving = double(out->n_passes) - (synth ? 1.0 : 0.0);
        out->microseconds = (4.2 * std::max(0.0, moving) + 0.09 * double(c.plan.stats.n_real_gates) + (synth ? 1.0 : 0.0)) * scale;
    }
    return QSV_OK;
}

int qsv_circuit_cost(qsv_t* h, int circuit_id, qsv_circuit_cost_t* out) {
    if (!h) return QSV_E_ARG;
    if (!out) return fail(h, QSV_E_ARG, "out is null");
    QSV_OPEN(h, "qsv_circuit_cost", kHostOnly);
    return circuit_cost_locked(h, circuit_id, out);
}

static int circuit_form_of(qsv_t* h, int circuit_id, qsv_circuit_form_t* out, bool launched) {
    if (!h) return QSV_E_ARG;
    if (!out) return fail(h, QSV_E_ARG, "out is null");
    QSV_OPEN(h, launched ? "qsv_circuit_launch_form" : "qsv_circuit_form", kHostOnly);
    qsv_circuit_cost_t cost;
    int rc = circuit_cost_locked(h, circuit_id, &cost);
    if (rc) return rc;
    const Circuit& c = h->circuits.find(circuit_id)->second;
    *out = qsv_circuit_form_t{};
    out->route = cost.route;
    out->n_keys = cost.n_keys;
    // (qsv_circuit_form: the FULL form, also of a circuit the one-launch route runs reduced: mask_x / mask_y and the keys both sides
    // share are what every other consumer of the side states goes by.  qsv_circuit_launch_form: the side plans that route runs)
    if (!c.split.ok) return QSV_OK;
    const SplitInfo& sp = launched && cost.route == QSV_ROUTE_SPLIT_ONE_LAUNCH && runs_reduced(h, c) ? c.reduced : c.split;
    // (the side plans are indexed as find_split left them; the split block names which of them is X -- in either form)
    const uint32_t* blk = c.plan.words.data() + c.split.off_block;
    const int sx = (blk[kSplitFlags] & kSplitSwapXY) ? 1 : 0;
    for (int xy = 0; xy < 2; ++xy) {
        out->n_virtual[xy] = sp.n_virtual[xy == 0 ? sx : 1 - sx];
        out->outer[xy] = sp.outer[xy == 0 ? sx : 1 - sx];
    }
    out->amps_per_thread = 1 << sp.side_r;
    out->halves = sp.fused && sp.halves ? 1 : 0;
    out->one_launch = sp.fused ? 1 : 0;
    out->split_sampled = split_rule(h, SplitUse::Sampling).takes(c) ? 1 : 0;
    out->mask_x = blk[kSplitMaskX];
    out->mask_y = blk[kSplitMaskY];
    return QSV_OK;
}

int qsv_circuit_form(qsv_t* h, int circuit_id, qsv_circuit_form_t* out) { return circuit_form_of(h, circuit_id, out, false); }

int qsv_circuit_launch_form(qsv_t* h, int circuit_id, qsv_circuit_form_t* out) { return circuit_form_of(h, circuit_id, out, true); }

int qsv_eval_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                      double* out) {
    QSV_OPEN(h, "qsv_eval_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out)))
        return fail(h, QSV_E_ARG, "bad arguments");
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args);
    return rc ? rc : eval_all(h, args, out);
}

// Collect the requests of concurrent callers for a moment, evaluate them as ONE batch, hand every caller its value.
// (caller holds h->cq_mu through `lock`; returns with it held)
static void coalesce_lead(qsv_t* h, std::unique_lock<std::mutex>& lock, double window_us) {
    using clock = std::chrono::steady_clock;
    const double window = window_us > 0 ? window_us : 300.0;
    const double quiet = getenv("QSV_COALESCE_QUIET_US") ? atof(getenv("QSV_COALESCE_QUIET_US")) : 60.0;
    // A batch is complete when as many callers as last time have arrived, or nobody new came for `quiet` us, or the
    // window is over.  The collector spins (no timed sleep is shorter than the kernel's timer slack of ~50 us).
    lock.unlock();
    const auto t0 = clock::now();
    auto last_arrival = t0;
    size_t seen = h->cq_count.load();
    for (;;) {
        const auto now = clock::now();
        const size_t count = h->cq_count.load();
        if (count != seen) {
            seen = count;
            last_arrival = now;
        }
        const double since_start = std::chrono::duration<double, std::micro>(now - t0).count();
        const double since_arrival = std::chrono::duration<double, std::micro>(now - last_arrival).count();
        if ((h->cq_expected > 1 && count >= h->cq_expected) || since_arrival >= quiet || since_start >= window) break;
        __builtin_ia32_pause();
    }
    lock.lock();
    std::vector<qsv_handle::CoalesceRequest*> batch;
    batch.swap(h->cq);
    h->cq_count.store(0);
    lock.unlock();
    {
        std::lock_guard<std::mutex> hl(h->mu);
        BatchArgs args;  // (each request is checked on its own: a bad one fails alone)
        std::vector<qsv_handle::CoalesceRequest*> valid;
        for (auto* r : batch) {
            auto it = h->circuits.find(r->circuit_id);
            if (it == h->circuits.end() || r->n_params < it->second.n_params) {
                r->rc = QSV_E_ARG;
                r->err = it == h->circuits.end() ? "unknown circuit id " + std::to_string(r->circuit_id)
                                                 : "circuit needs " + std::to_string(it->second.n_params) + " parameter values";
                continue;
            }
            args.circs.push_back(&it->second);
            args.n_params.push_back(r->n_params);
            args.values.insert(args.values.end(), r->params, r->params + r->n_params);
            valid.push_back(r);
        }
        if (!valid.empty()) {
            std::vector<double> values(valid.size(), 0.0);
            args.values.push_back(0.0);
            int rc = hipSetDevice(h->device) == hipSuccess ? QSV_OK : QSV_E_DEVICE;
            if (!rc) rc = eval_all(h, args, values.data());
            const std::string err = rc ? g_handle_error : std::string();
            for (size_t i = 0; i < valid.size(); ++i) {
                valid[i]->rc = rc;
                valid[i]->err = err;
                valid[i]->value = values[i];
            }
        }
    }
    lock.lock();
    // how many callers to expect next time: a high-water mark that decays slowly (a batch cut short by a pause in the
    // arrivals must not teach the next collector to stop early as well)
    h->cq_expected = std::max(batch.size(), h->cq_expected * 7 / 8);
    h->cq_batches += 1;
    for (auto* r : batch) r->done = true;
    h->cq_collecting = false;
    h->cq_cv.notify_all();
}

int qsv_eval_coalesced(qsv_t* h, int circuit_id, const double* params, int n_params, double window_us, double* out) {
    if (!h) return QSV_E_ARG;
    if (!out || n_params < 0 || (n_params > 0 && !params)) return fail(h, QSV_E_ARG, "bad arguments");
    // (whoever collects the batch takes the handle's lock in coalesce_lead: refused here, before the request is queued)
    if (h->batch_owner.load() == std::this_thread::get_id()) return refuse_in_batch(h, "qsv_eval_coalesced");
    qsv_handle::CoalesceRequest req;
    req.circuit_id = circuit_id;
    req.params = params;
    req.n_params = n_params;
    std::unique_lock<std::mutex> lock(h->cq_mu);
    h->cq.push_back(&req);
    h->cq_count.fetch_add(1);
    while (!req.done) {
        if (!h->cq_collecting) {
            h->cq_collecting = true;  // nobody is collecting: this caller does, for everyone queued with it
            coalesce_lead(h, lock, window_us);
        } else {
            h->cq_cv.wait(lock);
        }
    }
    lock.unlock();
    if (req.rc) return fail(h, req.rc, req.err);
    *out = req.value;
    return QSV_OK;
}

int qsv_eval_begin(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_counts) {
    if (!h) return QSV_E_ARG;
    // a second begin from the thread that already holds the handle (between begin and end) would wait for itself
    if (h->batch_owner.load() == std::this_thread::get_id())
        return fail(h, QSV_E_STATE, "a batch is already open on this handle");
    std::unique_lock<std::mutex> lock(h->mu);
    if (h->batch.open) return fail(h, QSV_E_STATE, "a batch is already open on this handle");
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_counts))) return fail(h, QSV_E_ARG, "bad arguments");
    PhaseClock begin_clock(h, &PhaseClock::Timing::begin_us);
    h->timing.calls += 1;
    QSV_HIP(h, hipSetDevice(h->device));
    {
        // The previous batch again (same circuits, same counts, nothing changed in between -- an optimiser's next iteration):
        // its layout is still in the staging buffer, descriptors ordered and slotted as its one push left them.
        qsv_handle::Batch& b = h->batch;
        b.cur_ids.assign(circuit_ids, circuit_ids + n_evals);
        b.cur_counts.assign(param_counts, param_counts + n_evals);
        b.have_ids = true;
        if (h->repeat_enabled && n_evals > 0 && b.snap_epoch == h->epoch && !h->profiling && b.reduced == reduced_route(h) &&
            b.snap_ids == b.cur_ids && b.snap_counts == b.cur_counts && b.circs.size() == size_t(n_evals)) {
            // (A batch that ended without waiting may still be running.  Its kernels read the staging buffers: whoever WRITES
            // them waits for it first -- qsv_eval_push with host values, qsv_eval_staging --, and a batch whose values come from
            // device memory, qsv_eval_push_device, writes nothing: such batches follow each other on the stream without the
            // host ever waiting, which is what an optimiser that lives on the device needs.)
            h->prof = qsv_profile{};
            h->prof.n_evals = uint64_t(n_evals);
            b.repeat = true;
            b.whole_push = false;
            b.pushed = 0;
            b.n_pushes = 0;
            b.aux_count = 0;
            b.used_mask = 0;
            b.chain_crossed = false;
            b.ways = 1;
            if (h->diagonal && n_evals >= 2) b.ways = std::max(1, std::min({h->n_streams, h->n_lane_streams + 1, h->group}));
            b.sentinels = h->poll_results && h->diagonal;
            if (b.sentinels) {
                uint64_t* v = reinterpret_cast<uint64_t*>(h->h_out);
                for (int i = 0; i < n_evals; ++i) v[i] = kResultSentinel;
            }
            b.open = true;
            h->batch_owner.store(std::this_thread::get_id());
            h->batch_lock = std::move(lock);
            return QSV_OK;
        }
    }
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, nullptr, nullptr, args);
    if (rc) return rc;
    for (int i = 0; i < n_evals; ++i)
        if (param_counts[i] < 0) return fail(h, QSV_E_ARG, "negative parameter count");
    args.n_params.assign(param_counts, param_counts + n_evals);
    rc = eval_begin(h, args.circs, args.n_params);
    if (rc) {
        eval_close(h);
        return rc;
    }
    h->batch.open = true;
    h->batch_owner.store(std::this_thread::get_id());
    h->batch_lock = std::move(lock);  // other threads wait until qsv_eval_end
    return QSV_OK;
}

int qsv_eval_push(qsv_t* h, int first, int count, const double* values) {
    if (!h) return QSV_E_ARG;
    if (!h->batch.open) return fail(h, QSV_E_STATE, "no open batch (call qsv_eval_begin first)");
    if (first < 0 || count < 0) return fail(h, QSV_E_ARG, "bad arguments");
    return eval_push(h, size_t(first), size_t(count), values ? values : kNoValues);
}

int qsv_eval_push_device(qsv_t* h, int first, int count, const double* device_values, void* ready_event) {
    if (!h) return QSV_E_ARG;
    if (!h->batch.open) return fail(h, QSV_E_STATE, "no open batch (call qsv_eval_begin first)");
    if (first < 0 || count < 0) return fail(h, QSV_E_ARG, "bad arguments");
    if (!device_values) return qsv_eval_push(h, first, count, nullptr);  // (only legal for evaluations without parameters)
    const void* const given = device_values;
    static const char* const name = "device_values";
    if (const int rc = check_device_pointers(h, &given, &name, &h->dev_params_checked, 1)) return rc;
    if (ready_event) {
        // whichever of the handle's streams runs a part of this push reads the values: all of them wait
        QSV_HIP(h, hipStreamWaitEvent(h->stream, static_cast<hipEvent_t>(ready_event), 0));
        for (hipStream_t st : h->side_streams) QSV_HIP(h, hipStreamWaitEvent(st, static_cast<hipEvent_t>(ready_event), 0));
    }
    return eval_push(h, size_t(first), size_t(count), kNoValues, device_values);
}

int qsv_eval_staging(qsv_t* h, int first, int count, double** values) {
    if (!h || !values) return QSV_E_ARG;
    if (!h->batch.open) return fail(h, QSV_E_STATE, "no open batch (call qsv_eval_begin first)");
    const qsv_handle::Batch& b = h->batch;
    if (first < 0 || count < 0 || size_t(first) + size_t(count) > b.circs.size()) return fail(h, QSV_E_ARG, "range exceeds the batch");
    if (const int rc = wait_pending(h)) return rc;  // (the caller is about to write the staging buffer)
    double* hp = reinterpret_cast<double*>(static_cast<char*>(h->h_batch) + b.desc_bytes);
    *values = hp + (count > 0 ? size_t(b.param_base[size_t(first)]) : 0);
    return QSV_OK;
}

int qsv_spsa_step(qsv_t* h, const qsv_spsa_step_args* in) {
    if (!h || !in) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_spsa_step", kDevice);
    if (in->n_runs < 0 || in->width < 0 || !in->x || !in->active || !in->iterations) return fail(h, QSV_E_ARG, "bad arguments");
    if (in->values && !in->delta_accept) return fail(h, QSV_E_ARG, "values without the signs they were measured with");
    if (in->delta_propose && !in->points) return fail(h, QSV_E_ARG, "a proposal needs somewhere to go");
    if (in->window < 0 || (in->window > 0 && (!in->previous || !in->n_values || !in->changes)))
        return fail(h, QSV_E_ARG, "the termination rule needs its state");
    if (!(in->eps > 0)) return fail(h, QSV_E_ARG, "eps must be positive");
    QSV_HIP(h, launch_spsa_step(*in, h->stream));
    return QSV_OK;
}

int qsv_nft_step(qsv_t* h, const qsv_nft_step_args* in) {
    if (!h || !in) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_nft_step", kDevice);
    if (in->n_runs < 0 || in->width < 0 || in->columns_stride < 1 || !in->x || !in->sizes || !in->columns || !in->recycled)
        return fail(h, QSV_E_ARG, "bad arguments");
    if (in->accept && !in->values) return fail(h, QSV_E_ARG, "an accept needs the values it fits");
    if (in->propose && !in->points) return fail(h, QSV_E_ARG, "a proposal needs somewhere to go");
    if ((in->accept && in->accept_iteration < 0) || (in->propose && in->propose_iteration < 0))
        return fail(h, QSV_E_ARG, "a negative iteration number");
    if ((reinterpret_cast<uintptr_t>(in->x) & 7u) || (reinterpret_cast<uintptr_t>(in->points) & 7u))
        return fail(h, QSV_E_ARG, "x and points must be aligned as doubles are");
    QSV_HIP(h, launch_nft_step(*in, h->stream));
    return QSV_OK;
}

int qsv_adam_step(qsv_t* h, const qsv_adam_step_args* in) {
    if (!h || !in) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_adam_step", kDevice);
    if (in->n_runs < 0 || in->width < 0 || in->grad_width < 0 || in->columns_stride < 1 || !in->x || !in->sizes || !in->columns || !in->m ||
        !in->v || !in->gradient || !in->active || !in->iterations)
        return fail(h, QSV_E_ARG, "bad arguments");
    if (in->grad_width < in->columns_stride)
        return fail(h, QSV_E_ARG, "grad_width " + std::to_string(in->grad_width) + " is smaller than the " + std::to_string(in->columns_stride) +
                                      " entries a run may search");
    QSV_HIP(h, launch_adam_step(*in, h->stream));
    return QSV_OK;
}

int qsv_eval_suggested_pushes(const qsv_t* h) {
    if (!h || !h->batch.open) return QSV_E_ARG;
    // Two pushes overlap the packing of the second half with the GPU work on the first -- worth it when there is GPU
    // work to speak of.  A batch of split evaluations under a quadratic operator is a chain of three short launches:
    // one push (measured at 20 qubits, 64 evaluations: 87.6 us per call against 90.5).
    const qsv_handle::Batch& b = h->batch;
    bool all_split = b.split_any;
    for (size_t i = 0; all_split && i < b.split.size(); ++i) all_split = b.split[i] != 0;
    // (... up to about a launch group of the side circuits: 256 evaluations at 24 qubits take 0.29 ms in two pushes,
    // 0.42 ms in one)
    // (a mixed batch whose ordinary evaluations run beside the split ones on the auxiliary stream likewise)
    // (128 since a push's split evaluations of both kinds run side by side, eval_push: 128 five-layer circuits at 20 qubits
    // 678 k evals/s in two pushes, 827 k in one; six layers 268 k / 288 k; four layers 1.51 M / 1.48 M; 256: two pushes)
    return ((all_split && factor_path(h)) || b.aux_plain) && b.split.size() <= 128 ? 1 : 2;
}

int qsv_eval_set_output(qsv_t* h, double* device_out) {
    if (!h) return QSV_E_ARG;
    if (!h->batch.open) return fail(h, QSV_E_STATE, "no open batch (call qsv_eval_begin first)");
    if (h->batch.pushed != 0) return fail(h, QSV_E_STATE, "the output must be set before the first push");
    h->out_target = device_out;
    // every push on the handle's own stream: the caller continues on that stream (joining the other streams into it
    // cost 15 us per batch of 64 evaluations at 20 qubits; callers should push such a batch in one go)
    if (device_out) {
        h->batch.ways = 1;
        // The caller may already have queued writes to the output buffer on the handle's stream (a fill of the unused
        // tail of an uneven shard).  The batch's ordinary evaluations can run on the auxiliary stream (mixed batches,
        // eval_begin): whatever stream of ours writes results must come after that work.
        if (h->batch.aux_plain && h->aux_stream >= 0) {
            QSV_HIP(h, hipEventRecord(h->ev_join, h->stream));
            QSV_HIP(h, hipStreamWaitEvent(h->side_streams[size_t(h->aux_stream)], h->ev_join, 0));
        }
    }
    return QSV_OK;
}

int qsv_eval_results_seen(qsv_t* h) {
    QSV_OPEN(h, "qsv_eval_results_seen", kHostOnly);
    if (h->batch.open) return fail(h, QSV_E_STATE, "a batch is open");
    h->async_pending = false;
    return QSV_OK;
}

int qsv_eval_end(qsv_t* h, double* out_expectations) {
    if (!h) return QSV_E_ARG;
    if (!h->batch.open) return fail(h, QSV_E_STATE, "no open batch (call qsv_eval_begin first)");
    int rc = out_expectations || h->batch.circs.empty() || h->out_target ? eval_end(h, out_expectations)
                                                                         : fail(h, QSV_E_ARG, "out is null");
    if (rc) {  // nothing of the failed batch may still be running
        (void)sync_streams(h);
    }
    eval_close(h);
    h->batch_owner.store(std::thread::id());
    std::unique_lock<std::mutex> lock = std::move(h->batch_lock);
    return rc;  // `lock` releases the handle here
}

int qsv_eval_batch(qsv_t* h, int n_evals, const int64_t* op_offsets, const qsv_op* ops, const int64_t* param_offsets,
                   const double* params, double* out) {
    QSV_OPEN(h, "qsv_eval_batch", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!op_offsets || !param_offsets || !out)))
        return fail(h, QSV_E_ARG, "bad arguments");
    // The cache of inline structures is bounded.  It is emptied only HERE, before any circuit of this call has been
    // looked up: evicting inside the loop below would free plans that earlier evaluations of the same call point at.
    if (h->inline_cache.size() > kInlineCacheLimit) {
        QSV_HIP(h, sync_streams(h));
        for (auto& kv : h->inline_cache) h->circuits.erase(kv.second);
        h->inline_cache.clear();
    }
    // pass 1: ids of known structures, list of the new ones (each distinct structure once)
    std::vector<int> ids(size_t(n_evals), 0);
    std::vector<std::string> keys;
    keys.resize(size_t(n_evals));
    struct Fresh {
        int first_eval;
        Circuit circuit;
        std::string err;
        int rc = QSV_OK;
    };
    std::vector<Fresh> fresh;
    std::unordered_map<std::string, int> fresh_index;  // key -> index in `fresh`
    std::vector<int> pending(size_t(n_evals), -1);
    for (int i = 0; i < n_evals; ++i) {
        const int64_t b = op_offsets[i], e = op_offsets[i + 1];
        if (e < b) return fail(h, QSV_E_ARG, "op_offsets must be non-decreasing");
        const int64_t np = param_offsets[i + 1] - param_offsets[i];
        if (np < 0) return fail(h, QSV_E_ARG, "param_offsets must be non-decreasing");
        // structure key: the ops (literal angles are baked into a registered circuit, so they are part of its
        // identity) and the length of the parameter vector
        std::string& key = keys[size_t(i)];
        key.assign(reinterpret_cast<const char*>(ops + b), size_t(e - b) * sizeof(qsv_op));
        key.append(reinterpret_cast<const char*>(&np), sizeof(np));
        auto it = h->inline_cache.find(key);
        if (it != h->inline_cache.end()) {
            ids[size_t(i)] = it->second;
            continue;
        }
        auto fi = fresh_index.find(key);
        if (fi == fresh_index.end()) {
            fi = fresh_index.emplace(key, int(fresh.size())).first;
            fresh.emplace_back();
            fresh.back().first_eval = i;
        }
        pending[size_t(i)] = fi->second;
    }
    // pass 2: schedule the new structures, on several host threads when there are many (a generation of EVQE brings
    // up to a population of new structures at once)
    if (!fresh.empty()) {
        std::vector<BuiltCircuit> built;
        build_many(h, fresh.size(), [&](size_t j, BuiltCircuit& b) {
            const int i = fresh[j].first_eval;
            const int64_t ob = op_offsets[i], oe = op_offsets[i + 1];
            b.rc = build_circuit(h, int(oe - ob), ops + ob, int(param_offsets[i + 1] - param_offsets[i]), true, &b.circuit, &b.err);
        }, built);
        for (size_t j = 0; j < fresh.size(); ++j) {
            fresh[j].rc = built[j].rc;
            fresh[j].err = std::move(built[j].err);
            fresh[j].circuit = std::move(built[j].circuit);
        }
        for (Fresh& f : fresh)
            if (f.rc) return fail(h, f.rc, f.err + " (evaluation " + std::to_string(f.first_eval) + ")");
        std::vector<int> fresh_id(fresh.size());
        for (size_t j = 0; j < fresh.size(); ++j) {
            fresh_id[j] = insert_circuit(h, std::move(fresh[j].circuit));
            h->inline_cache.emplace(keys[size_t(fresh[j].first_eval)], fresh_id[j]);
        }
        for (int i = 0; i < n_evals; ++i)
            if (pending[size_t(i)] >= 0) ids[size_t(i)] = fresh_id[size_t(pending[size_t(i)])];
    }
    // pass 3: only now, with every registration done, take pointers into the circuit table
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), ids.data(), param_offsets, params, args);
    return rc ? rc : eval_all(h, args, out);
}

int qsv_statevector(qsv_t* h, int circuit_id, const double* params, int n_params, double* out_re_im) {
    QSV_OPEN(h, "qsv_statevector", kDevice);
    if (!out_re_im) return fail(h, QSV_E_ARG, "out is null");
    int rc = run_single_to_state(h, circuit_id, params, n_params);
    if (rc) return rc;
    const uint64_t dim = uint64_t(1) << h->n;
    if (h->dtype == QSV_F64) {
        QSV_HIP(h, hipMemcpyAsync(out_re_im, h->d_states.ptr, dim * 16, hipMemcpyDeviceToHost, h->stream));
    } else {
        if ((rc = ensure(h, h->d_scratch, dim * 16))) return rc;
        QSV_HIP(h, launch_state_to_f64(h->dtype, h->d_states.ptr, dim, static_cast<double*>(h->d_scratch.ptr), h->stream));
        QSV_HIP(h, hipMemcpyAsync(out_re_im, h->d_scratch.ptr, dim * 16, hipMemcpyDeviceToHost, h->stream));
    }
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    return QSV_OK;
}

int qsv_probabilities(qsv_t* h, int circuit_id, const double* params, int n_params, double* out_probs) {
    QSV_OPEN(h, "qsv_probabilities", kDevice);
    if (!out_probs) return fail(h, QSV_E_ARG, "out is null");
    int rc = run_single_to_state(h, circuit_id, params, n_params);
    if (rc) return rc;
    const uint64_t dim = uint64_t(1) << h->n;
    if ((rc = ensure(h, h->d_scratch, dim * 8))) return rc;
    QSV_HIP(h, launch_probabilities(h->dtype, h->d_states.ptr, dim, 1, static_cast<double*>(h->d_scratch.ptr), h->stream));
    QSV_HIP(h, hipMemcpyAsync(out_probs, h->d_scratch.ptr, dim * 8, hipMemcpyDeviceToHost, h->stream));
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    return QSV_OK;
}

static const char* const kNotSampled = "circuits on kept states are not sampled (qsv_eval_* only)";

// Sampler branch for a whole batch: run the circuits group by group, turn each resident state into probabilities,
// draw `shots` samples per evaluation on the device and (for a diagonal operator) gather each sample's value D[state].
// out_cvar != null: the samples and their values stay on the device, only CVaR_alpha per evaluation comes back.
// dev != null (qsv_cvar_device): ... and goes to dev->out in device memory, and the call returns without waiting.  Which calls
// can allocate: one whose d_scratch has to grow (more evaluations x shots, or the first call of a handle), and whatever
// batch_layout needs for a batch it has not laid out before; ensure() waits for the handle's streams before it frees.  A search
// that repeats one shape allocates in its first iteration only.
// keep_states != null (qsv_sample_lookup): the samples stay in d_scratch, where the device-side CVaR keeps them, no value is
// gathered and no operator needed; *keep_states points at them and the call returns without waiting.
static int sample_batch_locked(qsv_t* h, const BatchArgs& args, int shots, uint64_t seed, uint64_t* out_states,
                               double* out_values, double alpha = 1.0, double* out_cvar = nullptr, const DeviceCall* dev = nullptr,
                               uint64_t** keep_states = nullptr) {
    const size_t n_evals = args.circs.size();
    if (dev) out_cvar = dev->out;
    if (n_evals == 0 || shots == 0) return QSV_OK;
    if ((out_values || out_cvar) && !(h->has_diag_part && h->diagonal))
        return fail(h, QSV_E_STATE, "sample values need a diagonal operator (call qsv_set_operator with I/Z terms only)");
    // circuits that have a split form are sampled from their two side tables: no state, no 2^n probabilities
    const SplitRule rule = split_rule(h, SplitUse::Sampling);
    const size_t n_split = rule.count(args.circs), n_plain = n_evals - n_split;
    const uint64_t dim = uint64_t(1) << h->n;
    const size_t G = size_t(h->group), SG = size_t(std::max(1, h->side_slots));
    // device scratch: probabilities and chunk sums of a group of ordinary evaluations | tables of a group of split
    // ones | (device-side CVaR) the samples
    const size_t probs_bytes = n_plain ? G * dim * 8 : 0, sums_bytes = n_plain ? G * size_t(sample_chunk_count(dim)) * 8 : 0;
    const size_t split_off = ((probs_bytes + sums_bytes + 63) / 64) * 64;
    const size_t split_bytes = n_split ? std::min(SG, n_split) * split_sample_slot_doubles(h->geo.k + kSideExtraBits) * 8 : 0;
    const size_t out_bytes = n_evals * size_t(shots) * 8;
    const size_t dev_samples_off = ((split_off + split_bytes + 63) / 64) * 64;
    int rc;
    if ((rc = ensure(h, h->d_scratch, dev_samples_off + (out_cvar ? 2 * out_bytes : keep_states ? out_bytes : 0)))) return rc;
    if (out_cvar && !dev && (rc = ensure_host_out(h, n_evals))) return rc;
    // samples (and their operator values) are written by the kernel straight into pinned host memory: no copy operations
    if (!out_cvar && !keep_states && h->h_samples_bytes < 2 * out_bytes) {
        if (h->h_samples) {
            QSV_HIP(h, sync_streams(h));
            QSV_HIP(h, hipHostFree(h->h_samples));
            h->h_samples = nullptr;
            h->h_samples_bytes = 0;
        }
        QSV_HIP(h, hipHostMalloc(&h->h_samples, 4 * out_bytes, hipHostMallocDefault));
        h->h_samples_bytes = 4 * out_bytes;
    }
    double* probs = static_cast<double*>(h->d_scratch.ptr);
    double* sums = probs + (n_plain ? G * dim : 0);
    double* split_scratch = reinterpret_cast<double*>(static_cast<char*>(h->d_scratch.ptr) + split_off);
    uint64_t* d_states = static_cast<uint64_t*>(h->h_samples);
    double* d_values = out_values ? reinterpret_cast<double*>(static_cast<char*>(h->h_samples) + out_bytes) : nullptr;
    if (out_cvar) {  // (device scratch behind the probabilities and chunk sums)
        d_states = reinterpret_cast<uint64_t*>(static_cast<char*>(h->d_scratch.ptr) + dev_samples_off);
        d_values = reinterpret_cast<double*>(static_cast<char*>(h->d_scratch.ptr) + dev_samples_off + out_bytes);
    }
    if (keep_states) d_states = reinterpret_cast<uint64_t*>(static_cast<char*>(h->d_scratch.ptr) + dev_samples_off);
    const double* diag = d_values ? static_cast<const double*>(h->d_diag.ptr) : nullptr;
    // one-tile registers: the pass kernel prepares its evaluation itself; n <= 28: its last pass writes the
    // probabilities, not the state
    const bool fuse = h->geo.blocks_per_state == 1;
    const bool probs_in_pass = h->n <= 28;
    // the split evaluations, a group of side-table slots at a time
    auto on_split = [&](size_t g0, size_t gc) -> int {
        PassArgs a{};
        a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
        a.evals = batch_evals(h) + g0;
        a.wtab = h->d_side.ptr;
        a.wtab_stride = h->side_stride;
        a.active = h->mask;
        QSV_HIP(h, launch_split_tables(h->dtype, h->geo.k + kSideExtraBits, unsigned(gc), split_scratch, h->stream, a));
        uint32_t table_doubles = 64;  // the largest Gram table of the group (whichever side the contraction calls Y)
        for (size_t i = 0; i < gc; ++i) {
            const SplitInfo& sp = args.circs[h->batch.eval_at[g0 + i]]->split;
            for (int side = 0; side < 2; ++side)
                table_doubles = std::max(table_doubles, uint32_t(1) << (2 * sp.n_keys + std::max(0, sp.n_virtual[side] - sp.n_keys - 6)));
        }
        QSV_HIP(h, launch_split_sample(h->dtype, h->geo.k + kSideExtraBits, unsigned(gc), split_scratch, shots, seed, diag, d_states, d_values,
                                       h->stream, a, table_doubles));
        return QSV_OK;
    };
    auto on_state = [&](size_t g0, size_t gc) -> int {
        if (!probs_in_pass) QSV_HIP(h, launch_probabilities(h->dtype, h->d_states.ptr, dim, int(gc), probs, h->stream));
        QSV_HIP(h, launch_sample(probs, dim, int(gc), sums, shots, seed, uint32_t(g0), diag, d_states, d_values, h->stream,
                                 n_split ? batch_evals(h) + g0 : nullptr, h->mask));
        return QSV_OK;
    };
    const StateRun run{rule, SG, G, fuse, kModeSynthFirst | kModeFinalStore | kModeSidesOnly,
                       kModeSynthFirst | (probs_in_pass ? kModeFinalProbs : kModeFinalStore) | (fuse ? kModeFusedPrepare : 0u)};
    if ((rc = run_states(h, args, run, on_split, on_state, dev))) return rc;
    if (keep_states) {
        *keep_states = d_states;
        return QSV_OK;
    }
    // (evaluation e's values are at d_values[e * shots ..] in the caller's numbering -- the sample kernels address by the
    // descriptor's out_index, or by first_eval + slot in a batch nothing reordered --, so workgroup e writes out[e])
    if (out_cvar) QSV_HIP(h, launch_cvar(d_values, int(n_evals), shots, alpha, dev ? dev->out : h->h_out, h->stream, h->mask));
    if (dev) {  // (everything above went to the handle's stream: complete once the work enqueued so far on it is)
        h->async_pending = true;
        return QSV_OK;
    }
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    if (out_cvar) {
        std::memcpy(out_cvar, h->h_out, n_evals * sizeof(double));
        return QSV_OK;
    }
    std::memcpy(out_states, d_states, out_bytes);
    if (out_values) std::memcpy(out_values, d_values, out_bytes);
    return QSV_OK;
}

// Exact-probability CVaR for a whole batch: the circuits group by group as in the sampler branch (split circuits as their
// two virtual circuits, the others with the probabilities written by their last gate pass), then launch_cvar_exact.
// dev != null (qsv_cvar_device): the results go to dev->out in device memory and the call returns without waiting.  It can
// allocate where sample_batch_locked can, and the first call after qsv_set_operator sorts the operator's values, which
// allocates and waits (sort_states_by_value).
static int expectation_to_device(qsv_t* h, const BatchArgs& args, double* device_out, const int* plan_id = nullptr);
// What the exact CVaR and its gradient ask of the operator, of alpha, and of the sorted values (sort.hip).
static int cvar_operator_guard(qsv_t* h) {
    if (h->has_diag_part && h->diagonal) return QSV_OK;
    return fail(h, QSV_E_STATE, "the exact CVaR needs a diagonal operator (call qsv_set_operator with I/Z terms only)");
}
static bool cvar_alpha_is_one(double alpha) { return std::fabs(alpha - 1.0) <= 1e-8 + 1e-5; }  // numpy.isclose(alpha, 1)
static int sorted_values_ready(qsv_t* h) {
    if (h->order_valid) return QSV_OK;
    const uint64_t dim = uint64_t(1) << h->n;
    int rc;
    if ((rc = wait_pending(h))) return rc;  // (it allocates: not beside a batch that ended without waiting)
    if ((rc = ensure(h, h->d_order, dim * sizeof(uint32_t))) || (rc = ensure(h, h->d_sorted, dim * sizeof(double)))) return rc;
    QSV_HIP(h, sort_states_by_value(static_cast<const double*>(h->d_diag.ptr), dim, static_cast<uint32_t*>(h->d_order.ptr),
                                    static_cast<double*>(h->d_sorted.ptr), h->stream));
    h->order_valid = true;
    return QSV_OK;
}
static int exact_cvar_locked(qsv_t* h, const BatchArgs& args, double alpha, double* out_cvar, const DeviceCall* dev = nullptr) {
    const size_t n_evals = args.circs.size();
    if (n_evals == 0) return QSV_OK;
    if (const int rc = cvar_operator_guard(h)) return rc;
    if (const int rc = qubit_guard(h, "the exact CVaR is available up to 28 qubits")) return rc;
    // alpha = 1 (numpy.isclose(alpha, 1), the reference's test): the reference takes the plain mean of the values there
    // (expectation_calculation.py:55-69), not its accumulation loop, whose stopping rule leaves out the last 1e-5 of the mass
    // (5e-4 of an Ising value at 20 qubits): the expectation value, as qsv_eval_circuits computes it
    if (cvar_alpha_is_one(alpha)) return dev ? expectation_to_device(h, args, dev->out) : eval_all(h, args, out_cvar);
    const uint64_t dim = uint64_t(1) << h->n;
    int rc;
    if ((rc = sorted_values_ready(h))) return rc;
    const SplitRule rule = split_rule(h, SplitUse::Sampling);
    const size_t n_split = rule.count(args.circs), n_plain = n_evals - n_split;
    const size_t G = size_t(h->group), SG = size_t(std::max(1, h->side_slots));
    const uint32_t n_chunks = cvar_exact_chunks(dim);
    const size_t probs_bytes = n_plain ? G * dim * 8 : 0;
    const size_t chunk_off = ((probs_bytes + 63) / 64) * 64;
    const size_t chunk_bytes = 2 * std::max(G, std::min(SG, std::max<size_t>(1, n_split))) * size_t(n_chunks) * 8;
    if ((rc = ensure(h, h->d_scratch, chunk_off + chunk_bytes))) return rc;
    if (!dev && (rc = ensure_host_out(h, n_evals))) return rc;
    double* const result = dev ? dev->out : h->h_out;  // (written at out_index, the caller's numbering: nothing to un-permute)
    double* probs = static_cast<double*>(h->d_scratch.ptr);
    double* chunk_scratch = reinterpret_cast<double*>(static_cast<char*>(h->d_scratch.ptr) + chunk_off);
    const bool fuse = h->geo.blocks_per_state == 1;
    const uint32_t* order = static_cast<const uint32_t*>(h->d_order.ptr);
    const double* sorted = static_cast<const double*>(h->d_sorted.ptr);
    // (split evaluations and the others alike: the kernel reads each one's side tables or probabilities by its descriptor)
    auto consume = [&](size_t g0, size_t gc) -> int {
        PassArgs a{};  // (here: the batch's layout may have moved the plan arena)
        a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
        a.wtab = h->d_side.ptr;
        a.wtab_stride = h->side_stride;
        a.evals = batch_evals(h) + g0;
        a.active = h->mask;
        QSV_HIP(h, launch_cvar_exact(h->dtype, probs, dim, unsigned(gc), order, sorted, alpha, chunk_scratch, result, h->stream, a));
        return QSV_OK;
    };
    const StateRun run{rule, SG, G, fuse, kModeSynthFirst | kModeFinalStore | kModeSidesOnly,
                       kModeSynthFirst | kModeFinalProbs | (fuse ? kModeFusedPrepare : 0u)};
    if ((rc = run_states(h, args, run, consume, consume, dev))) return rc;
    if (dev) {
        h->async_pending = true;
        return QSV_OK;
    }
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_cvar, h->h_out, n_evals * sizeof(double));
    return QSV_OK;
}

// alpha = 1 of the exact form with values and results in device memory: the expectation values, as a batch with
// qsv_eval_push_device and qsv_eval_set_output computes them; with a mask they go through d_scratch, and a copy kernel leaves
// plan_id (qsv_gradient_plan_run, the one chunk of a plan): the batch is remembered by it, and the same plan's next run, with
// nothing in between that counts (handle: epoch), is that batch again as qsv_eval_begin knows it -- the layout stands, the
// kernels read the descriptors from the device copy the last run's kernels made (batch.repeat, descs_base), and the host
// neither writes a staging buffer nor waits.  Everything still goes to the handle's stream, in order.
static int expectation_to_device(qsv_t* h, const BatchArgs& args, double* device_out, const int* plan_id) {
    const size_t n = args.circs.size();
    const ActiveMask mask = h->mask;
    h->mask = ActiveMask{};
    int rc = QSV_OK;
    if (mask.flags) rc = ensure(h, h->d_scratch, n * sizeof(double));
    qsv_handle::Batch& b = h->batch;
    const bool remember = plan_id && !mask.flags && args.device_values && n > 0 && h->repeat_enabled && !h->profiling;
    const bool again = remember && h->plan_snap.epoch == h->epoch && h->plan_snap.plan_id == *plan_id && h->plan_snap.n_evals == n;
    h->plan_snap.epoch = 0;
    if (!rc && again) {
        // (what qsv_eval_begin sets for the previous batch again; the buffers eval_begin sizes have their sizes)
        h->prof = qsv_profile{};
        h->prof.n_evals = uint64_t(n);
        b.circs = args.circs;
        b.repeat = true;
        b.whole_push = false;
        b.pushed = 0;
        b.n_pushes = 0;
        b.aux_count = 0;
        b.used_mask = 0;
        b.chain_crossed = false;
        b.sentinels = false;
    } else if (!rc) {
        rc = eval_begin(h, args.circs, args.n_params);
    }
    if (!rc) {
        h->out_target = mask.flags ? static_cast<double*>(h->d_scratch.ptr) : device_out;
        h->batch.ways = 1;  // (every push on the handle's own stream, and the ordinary evaluations of a mixed batch behind whatever
                            // the caller queued there: qsv_eval_set_output)
        if (h->batch.aux_plain && h->aux_stream >= 0) {
            hipError_t e = hipEventRecord(h->ev_join, h->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(h->side_streams[size_t(h->aux_stream)], h->ev_join, 0);
            if (e != hipSuccess) rc = fail(h, QSV_E_DEVICE, std::string("joining the auxiliary stream: ") + hipGetErrorString(e));
        }
    }
    if (!rc) rc = eval_push(h, 0, n, kNoValues, args.device_values);
    if (!rc) rc = eval_end(h, nullptr);
    if (!rc && h->profiling) h->async_pending = true;  // (a profiled batch waits in eval_end; harmless)
    if (!rc && mask.flags) {
        hipError_t e = launch_masked_copy(static_cast<const double*>(h->d_scratch.ptr), device_out, int(n), mask, h->stream);
        if (e != hipSuccess) rc = fail(h, QSV_E_DEVICE, std::string("launch_masked_copy: ") + hipGetErrorString(e));
    }
    if (rc) (void)sync_streams(h);
    eval_close(h);
    if (!rc && remember) h->plan_snap = qsv_handle::PlanSnap{h->epoch, *plan_id, n};
    return rc;
}

int qsv_sample_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                     int shots, uint64_t seed, uint64_t* out_states, double* out_values) {
    QSV_OPEN(h, "qsv_sample_batch", kDevice);
    if (n_evals < 0 || shots < 0 || (n_evals > 0 && shots > 0 && (!circuit_ids || !param_offsets || !out_states)))
        return fail(h, QSV_E_ARG, "bad arguments");
    BatchArgs args;  // (no shots: only the ids are looked at)
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, shots ? param_offsets : nullptr, params, args, shots ? kNotSampled : nullptr);
    return rc ? rc : sample_batch_locked(h, args, shots, seed, out_states, out_values);
}

int qsv_sample_cvar_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          int shots, uint64_t seed, double alpha, double* out_cvar) {
    QSV_OPEN(h, "qsv_sample_cvar_batch", kDevice);
    if (n_evals < 0 || shots < 1 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out_cvar)))
        return fail(h, QSV_E_ARG, "bad arguments");
    if (!(alpha > 0.0) || alpha > 1.0) return fail(h, QSV_E_ARG, "alpha must be in (0, 1]");
    if (shots > kCvarMaxShots) return fail(h, QSV_E_ARG, "the device-side CVaR sorts at most 4096 samples per evaluation");
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args, kNotSampled);
    return rc ? rc : sample_batch_locked(h, args, shots, seed, nullptr, nullptr, alpha, out_cvar);
}

int qsv_exact_cvar_batch(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                         double alpha, double* out_cvar) {
    QSV_OPEN(h, "qsv_exact_cvar_batch", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out_cvar))) return fail(h, QSV_E_ARG, "bad arguments");
    if (!(alpha > 0.0) || alpha > 1.0) return fail(h, QSV_E_ARG, "alpha must be in (0, 1]");
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args, kNotSampled);
    return rc ? rc : exact_cvar_locked(h, args, alpha, out_cvar);
}

// The k most probable basis states of every evaluation of a batch: the circuits group by group as in exact_cvar_locked (split
// circuits as their two virtual circuits, the others with the probabilities written by their last gate pass), then
// launch_top_states, which writes row out_index of the three outputs in pinned host memory (states | probabilities | values).
static int top_states_locked(qsv_t* h, const BatchArgs& args, int k, uint64_t* out_states, double* out_probs, double* out_values) {
    const size_t n_evals = args.circs.size();
    if (n_evals == 0) return QSV_OK;
    if (out_values && !(h->has_diag_part && h->diagonal))
        return fail(h, QSV_E_STATE, "the values of the top states need a diagonal operator (call qsv_set_operator with I/Z terms only)");
    const uint64_t dim = uint64_t(1) << h->n;
    const SplitRule rule = split_rule(h, SplitUse::Sampling);
    const size_t n_split = rule.count(args.circs), n_plain = n_evals - n_split;
    const size_t G = size_t(h->group), SG = size_t(std::max(1, h->side_slots));
    const size_t rows = n_evals * size_t(k);
    // device scratch: the probabilities of a group of ordinary evaluations | the blocks' lists of a group of either kind
    const size_t probs_bytes = std::min(G, n_plain) * dim * 8;
    const size_t lists_off = ((probs_bytes + 63) / 64) * 64;
    const size_t lists_bytes = top_states_scratch_bytes(dim, uint32_t(k), std::max(std::min(G, n_plain), std::min(SG, n_split)));
    int rc;
    if ((rc = ensure(h, h->d_scratch, lists_off + lists_bytes))) return rc;
    if ((rc = ensure_host_out(h, 3 * rows))) return rc;
    uint64_t* const states = reinterpret_cast<uint64_t*>(h->h_out);
    double* const result_probs = h->h_out + rows;
    double* const values = out_values ? h->h_out + 2 * rows : nullptr;
    double* probs = static_cast<double*>(h->d_scratch.ptr);
    void* lists = static_cast<char*>(h->d_scratch.ptr) + lists_off;
    const double* diag = out_values ? static_cast<const double*>(h->d_diag.ptr) : nullptr;
    const bool fuse = h->geo.blocks_per_state == 1;
    auto consume = [&](size_t g0, size_t gc) -> int {
        PassArgs a{};
        a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
        a.wtab = h->d_side.ptr;
        a.wtab_stride = h->side_stride;
        a.evals = batch_evals(h) + g0;
        QSV_HIP(h, launch_top_states(h->dtype, probs, dim, unsigned(gc), uint32_t(k), diag, lists, states, result_probs, values, h->stream, a));
        return QSV_OK;
    };
    const StateRun run{rule, SG, G, fuse, kModeSynthFirst | kModeFinalStore | kModeSidesOnly,
                       kModeSynthFirst | kModeFinalProbs | (fuse ? kModeFusedPrepare : 0u)};
    if ((rc = run_to_states(h, args, run, consume, consume))) return rc;
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_states, states, rows * sizeof(uint64_t));
    std::memcpy(out_probs, result_probs, rows * sizeof(double));
    if (out_values) std::memcpy(out_values, values, rows * sizeof(double));
    return QSV_OK;
}

int qsv_top_states(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params, int k,
                   uint64_t* out_states, double* out_probs, double* out_values) {
    QSV_OPEN(h, "qsv_top_states", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out_states || !out_probs))) return fail(h, QSV_E_ARG, "bad arguments");
    if (const int rc = qubit_guard(h, "the top states are available up to 28 qubits")) return rc;
    if (k < 1 || k > int(kTopMaxStates) || uint64_t(k) > (uint64_t(1) << h->n))
        return fail(h, QSV_E_ARG, "k must be between 1 and min(" + std::to_string(kTopMaxStates) + ", 2^n)");
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args,
                           "circuits on kept states have no top states (qsv_eval_* only)");
    return rc ? rc : top_states_locked(h, args, k, out_states, out_probs, out_values);
}

int qsv_cvar_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                    int shots, uint64_t seed, double alpha, const uint8_t* device_active, int active_stride, double* device_out) {
    QSV_OPEN(h, "qsv_cvar_device", kDevice);
    if (n_evals < 0 || shots < 0 || width < 0 || (n_evals > 0 && (!circuit_ids || !device_out || (width > 0 && !device_values))))
        return fail(h, QSV_E_ARG, "bad arguments");
    if (device_active && active_stride < 1) return fail(h, QSV_E_ARG, "active_stride must be at least 1");
    if (!(alpha > 0.0) || alpha > 1.0) return fail(h, QSV_E_ARG, "alpha must be in (0, 1]");
    if (shots > kCvarMaxShots) return fail(h, QSV_E_ARG, "the device-side CVaR sorts at most 4096 samples per evaluation");
    if (n_evals == 0) return QSV_OK;
    const void* given[3] = {width > 0 ? device_values : nullptr, device_out, device_active};
    static const char* const names[3] = {"device_values", "device_out", "device_active"};
    int rc = check_device_pointers(h, given, names, h->cvar_checked, 3);
    if (rc) return rc;
    BatchArgs args;
    if ((rc = resolve_batch(h, size_t(n_evals), circuit_ids, nullptr, nullptr, args, kNotSampled))) return rc;
    args.n_params.assign(size_t(n_evals), int64_t(width));
    args.device_values = width > 0 ? device_values : nullptr;
    // (all work of the call goes to the handle's stream -- run_laid_out --, so that is the stream that waits for the values)
    if (ready_event) QSV_HIP(h, hipStreamWaitEvent(h->stream, static_cast<hipEvent_t>(ready_event), 0));
    struct Unmask {
        qsv_t* h;
        ~Unmask() { h->mask = ActiveMask{}; }
    } unmask{h};
    if (device_active) h->mask = ActiveMask{device_active, uint32_t(active_stride)};
    const DeviceCall dev{circuit_ids, width, shots > 0, device_out};
    rc = shots > 0 ? sample_batch_locked(h, args, shots, seed, nullptr, nullptr, alpha, nullptr, &dev)
                   : exact_cvar_locked(h, args, alpha, nullptr, &dev);
    if (rc) {  // nothing of a failed call may still be running
        (void)sync_streams(h);
        h->cvar_snap.epoch = 0;
    }
    return rc;
}

// ---- device-resident value cache -------------------------------------------------------------------------------------------

static int ensure_pinned(qsv_t* h, void** ptr, size_t* have, size_t bytes) {
    if (*ptr && *have >= bytes) return QSV_OK;
    if (*ptr) {
        QSV_HIP(h, sync_streams(h));
        QSV_HIP(h, hipHostFree(*ptr));
        *ptr = nullptr;
        *have = 0;
    }
    const size_t want = std::max(2 * bytes, size_t(4096));
    QSV_HIP(h, hipHostMalloc(ptr, want, hipHostMallocDefault));
    *have = want;
    return QSV_OK;
}

// A table of 2^log2_slots empty slots (the keys are set on the handle's stream).
static int cache_table_alloc(qsv_t* h, int log2_slots, uint64_t** keys, double** vals) {
    const size_t bytes = sizeof(uint64_t) << log2_slots;
    *keys = nullptr;
    *vals = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(keys), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(vals), bytes);
    if (e == hipSuccess) e = hipMemsetAsync(*keys, 0xFF, bytes, h->stream);
    if (e != hipSuccess) {
        if (*keys) (void)hipFree(*keys);
        if (*vals) (void)hipFree(*vals);
        *keys = nullptr;
        *vals = nullptr;
        return fail(h, QSV_E_DEVICE, std::string("value cache table of 2^") + std::to_string(log2_slots) + " slots: " + hipGetErrorString(e));
    }
    return QSV_OK;
}

static int cache_clear_locked(qsv_t* h, ValueCache& c) {
    c.pending = false;
    c.entries = 0;
    c.clears += 1;
    QSV_HIP(h, hipMemsetAsync(c.d_keys, 0xFF, sizeof(uint64_t) << c.log2_slots, h->stream));
    return QSV_OK;
}

// The growth rule: after it 2 * (entries + n_samples) <= slots, the worst case of every sample being new, so a probe can never
// meet a full table.  The table doubles (its entries rehashed into the new one, once, whatever the number of doublings) up to
// 2^log2_max_slots; where the entries and the samples together would pass that, the table is cleared instead -- the scoring
// function is pure, only time is lost.  (The caller has refused a call that cannot fit into an empty table.)
static int cache_make_room(qsv_t* h, ValueCache& c, int64_t n_samples) {
    bool cleared = false;
    if (2 * (c.entries + n_samples) > (int64_t(1) << c.log2_max_slots)) {
        cleared = true;
        c.entries = 0;
        c.clears += 1;
    }
    int target = c.log2_slots;
    while (2 * (c.entries + n_samples) > (int64_t(1) << target)) ++target;
    if (target == c.log2_slots) {
        if (cleared) QSV_HIP(h, hipMemsetAsync(c.d_keys, 0xFF, sizeof(uint64_t) << c.log2_slots, h->stream));
        return QSV_OK;
    }
    uint64_t* keys;
    double* vals;
    int rc = cache_table_alloc(h, target, &keys, &vals);
    if (rc) return rc;
    if (!cleared) {
        hipError_t e = launch_cache_rehash(c.d_keys, c.d_vals, uint32_t(c.log2_slots), keys, vals, uint32_t(target),
                                           static_cast<uint32_t*>(c.d_counters.ptr), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipFree(keys);
            (void)hipFree(vals);
            return fail(h, QSV_E_DEVICE, std::string("launch_cache_rehash: ") + hipGetErrorString(e));
        }
        c.rehashes += 1;
    } else {
        QSV_HIP(h, hipStreamSynchronize(h->stream));  // (nothing may still read the table that is freed below)
    }
    (void)hipFree(c.d_keys);
    (void)hipFree(c.d_vals);
    c.d_keys = keys;
    c.d_vals = vals;
    c.log2_slots = target;
    return QSV_OK;
}

static ValueCache* find_cache(qsv_t* h, int cache_id) {
    auto it = h->value_caches.find(cache_id);
    if (it == h->value_caches.end()) {
        (void)fail(h, QSV_E_ARG, "unknown value cache id " + std::to_string(cache_id));
        return nullptr;
    }
    return &it->second;
}

int qsv_value_cache_create(qsv_t* h, int log2_slots, int log2_max_slots, int* out_cache_id) {
    QSV_OPEN(h, "qsv_value_cache_create", kDevice);
    if (!out_cache_id) return fail(h, QSV_E_ARG, "out_cache_id is null");
    if (log2_slots < 1 || log2_max_slots < log2_slots || log2_max_slots > 30)
        return fail(h, QSV_E_ARG, "a value cache needs 1 <= log2_slots <= log2_max_slots <= 30");
    ValueCache c;
    c.log2_slots = log2_slots;
    c.log2_max_slots = log2_max_slots;
    int rc = cache_table_alloc(h, log2_slots, &c.d_keys, &c.d_vals);
    if (!rc) rc = ensure(h, c.d_counters, kCacheCounterWords * sizeof(uint32_t));
    if (!rc) {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c.h_counters), kCacheCounterWords * sizeof(uint32_t), hipHostMallocDefault);
        if (e != hipSuccess) rc = fail(h, QSV_E_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    if (rc) {
        (void)sync_streams(h);
        free_value_cache(c);
        return rc;
    }
    const int id = h->next_cache_id++;
    h->value_caches.emplace(id, c);
    *out_cache_id = id;
    return QSV_OK;
}

int qsv_value_cache_destroy(qsv_t* h, int cache_id) {
    QSV_OPEN(h, "qsv_value_cache_destroy", kDevice);
    ValueCache* c = find_cache(h, cache_id);
    if (!c) return QSV_E_ARG;
    QSV_HIP(h, sync_streams(h));
    free_value_cache(*c);
    h->value_caches.erase(cache_id);
    return QSV_OK;
}

int qsv_value_cache_clear(qsv_t* h, int cache_id) {
    QSV_OPEN(h, "qsv_value_cache_clear", kDevice);
    ValueCache* c = find_cache(h, cache_id);
    if (!c) return QSV_E_ARG;
    return cache_clear_locked(h, *c);
}

int qsv_value_cache_stats(const qsv_t* h, int cache_id, qsv_value_cache_stats_t* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_value_cache_stats", kHostOnly);
    auto it = h->value_caches.find(cache_id);
    if (it == h->value_caches.end()) return QSV_E_ARG;
    const ValueCache& c = it->second;
    out->entries = c.entries;
    out->slots = int64_t(1) << c.log2_slots;
    out->samples_looked_up = c.samples_looked_up;
    out->hits = c.hits;
    out->new_entries = c.new_entries;
    out->rehashes = c.rehashes;
    out->clears = c.clears;
    return QSV_OK;
}

int qsv_sample_lookup(qsv_t* h, int cache_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                      int shots, uint64_t seed, int64_t* out_n_missing, const uint64_t** out_missing_states) {
    QSV_OPEN(h, "qsv_sample_lookup", kDevice);
    if (n_evals < 0 || shots < 0 || !out_n_missing || !out_missing_states ||
        (n_evals > 0 && shots > 0 && (!circuit_ids || !param_offsets)))
        return fail(h, QSV_E_ARG, "bad arguments");
    ValueCache* c = find_cache(h, cache_id);
    if (!c) return QSV_E_ARG;
    if (c->pending) return fail(h, QSV_E_STATE, "a lookup on this value cache waits for qsv_sample_lookup_finish (or qsv_value_cache_clear)");
    const int64_t n_samples = int64_t(n_evals) * shots;
    if (2 * n_samples > (int64_t(1) << c->log2_max_slots))  // (before anything is launched)
        return fail(h, QSV_E_ARG, "one call's " + std::to_string(n_samples) + " samples do not fit into half of the cache's 2^" +
                                      std::to_string(c->log2_max_slots) + " slots");
    if (h->n >= 64) return fail(h, QSV_E_UNSUPPORTED, "value caches key on states of fewer than 64 qubits");
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, shots ? param_offsets : nullptr, params, args, shots ? kNotSampled : nullptr);
    if (rc) return rc;
    *out_n_missing = 0;
    *out_missing_states = c->h_miss;
    if (n_samples == 0) {  // (nothing is drawn, as in qsv_sample_batch; the finish has nothing to do either)
        c->pending = true;
        c->pending_evals = 0;
        c->pending_shots = shots;
        c->pending_missing = 0;
        return QSV_OK;
    }
    // the cache's own buffers first (they may wait for the streams), then the draws, the growth and the probe on the stream
    if ((rc = ensure(h, c->d_sample_slot, size_t(n_samples) * sizeof(uint32_t))) ||
        (rc = ensure(h, c->d_miss_slots, size_t(n_samples) * sizeof(uint32_t))) ||
        (rc = ensure_pinned(h, reinterpret_cast<void**>(&c->h_miss), &c->h_miss_bytes, size_t(n_samples) * sizeof(uint64_t))))
        return rc;
    uint64_t* d_states = nullptr;
    if ((rc = sample_batch_locked(h, args, shots, seed, nullptr, nullptr, 1.0, nullptr, nullptr, &d_states))) {
        (void)sync_streams(h);
        return rc;
    }
    uint32_t* counters = static_cast<uint32_t*>(c->d_counters.ptr);
    hipError_t e = hipMemsetAsync(counters, 0, kCacheCounterWords * sizeof(uint32_t), h->stream);
    if (e == hipSuccess && (rc = cache_make_room(h, *c, n_samples))) {
        (void)sync_streams(h);
        return rc;
    }
    if (e == hipSuccess)
        e = launch_cache_probe(d_states, n_samples, c->d_keys, uint32_t(c->log2_slots), static_cast<uint32_t*>(c->d_sample_slot.ptr),
                               c->h_miss, static_cast<uint32_t*>(c->d_miss_slots.ptr), counters, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_counters, counters, kCacheCounterWords * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)sync_streams(h);
        return fail(h, QSV_E_DEVICE, std::string("qsv_sample_lookup: ") + hipGetErrorString(e));
    }
    if (c->h_counters[1] != 0) {  // (the growth rule rules it out; the table is no longer to be trusted)
        (void)cache_clear_locked(h, *c);
        return fail(h, QSV_E_DEVICE, "a value cache probe walked its whole table (the cache was cleared)");
    }
    const int64_t n_missing = int64_t(c->h_counters[0]);
    c->entries += n_missing;
    c->samples_looked_up += n_samples;
    c->new_entries += n_missing;
    c->hits += n_samples - n_missing;
    c->pending = true;
    c->pending_evals = n_evals;
    c->pending_shots = shots;
    c->pending_missing = n_missing;
    *out_n_missing = n_missing;
    *out_missing_states = c->h_miss;
    return QSV_OK;
}

int qsv_sample_lookup_finish(qsv_t* h, int cache_id, int64_t n_values, const double* values, double alpha, double* out_cvar,
                             double* out_values) {
    QSV_OPEN(h, "qsv_sample_lookup_finish", kDevice);
    ValueCache* c = find_cache(h, cache_id);
    if (!c) return QSV_E_ARG;
    if (!c->pending) return fail(h, QSV_E_STATE, "no lookup on this value cache waits for its values (qsv_sample_lookup comes first)");
    if (n_values != c->pending_missing)
        return fail(h, QSV_E_STATE, "the lookup reported " + std::to_string(c->pending_missing) + " missing states, " +
                                        std::to_string(n_values) + " values were given");
    if (n_values > 0 && !values) return fail(h, QSV_E_ARG, "values is null");
    if (out_cvar && (!(alpha > 0.0) || alpha > 1.0)) return fail(h, QSV_E_ARG, "alpha must be in (0, 1]");
    if (out_cvar && c->pending_shots > kCvarMaxShots)
        return fail(h, QSV_E_ARG, "the device-side CVaR sorts at most 4096 samples per evaluation");
    const int64_t n_evals = c->pending_evals, n_samples = n_evals * c->pending_shots;
    int rc;
    if ((rc = wait_pending(h))) return rc;  // (the scratch and the result buffer are about to be written)
    if (n_values > 0) {
        if ((rc = ensure_pinned(h, reinterpret_cast<void**>(&c->h_values), &c->h_values_bytes, size_t(n_values) * sizeof(double)))) return rc;
        std::memcpy(c->h_values, values, size_t(n_values) * sizeof(double));
        QSV_HIP(h, launch_cache_fill(c->d_vals, static_cast<const uint32_t*>(c->d_miss_slots.ptr), c->h_values, n_values, h->stream));
    }
    if (n_samples > 0 && (out_cvar || out_values)) {
        // every sample's value, evaluation e's at [e * shots ..) as sample_batch_locked leaves its d_values for launch_cvar
        if ((rc = ensure(h, h->d_scratch, size_t(n_samples) * sizeof(double)))) return rc;
        double* d_values = static_cast<double*>(h->d_scratch.ptr);
        QSV_HIP(h, launch_cache_gather(c->d_vals, static_cast<const uint32_t*>(c->d_sample_slot.ptr), n_samples, d_values, h->stream));
        if (out_cvar) {
            if ((rc = ensure_host_out(h, size_t(n_evals)))) return rc;
            QSV_HIP(h, launch_cvar(d_values, int(n_evals), c->pending_shots, alpha, h->h_out, h->stream, ActiveMask{}));
        }
        if (out_values)
            QSV_HIP(h, hipMemcpyAsync(out_values, d_values, size_t(n_samples) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    if (out_cvar && n_samples > 0) std::memcpy(out_cvar, h->h_out, size_t(n_evals) * sizeof(double));
    c->pending = false;
    return QSV_OK;
}

// ---- parameter-shift gradients ---------------------------------------------------------------------------------------------

// A device buffer that grows by doubling (the scratch matrix of the shifted rows: calls of growing size reallocate seldom).
static int ensure_doubling(qsv_t* h, DeviceBuffer& b, size_t bytes, size_t most, int64_t& counter) {
    if (b.bytes >= bytes && b.ptr) return QSV_OK;
    return ensure_counted(h, b, std::max(bytes, std::min(2 * b.bytes, most)), counter);
}

// The base rows and the output of a gradient call, both in device memory.
struct GradCall {
    const double* base;
    int64_t base_stride;
    int base_width;
    double* out;
    int out_width;
};

// The shift tables of a gradient call -- circs[e] by the parameters wrt[wrt_offsets[e] .. wrt_offsets[e + 1]) (wrt_offsets null: by
// every parameter), points in rows of base_width values, gradients in rows of out_width -- and every check such a call makes.
struct GradTables {
    std::vector<GradRow> rows;
    std::vector<GradEntry> entries;
    std::vector<int64_t> offsets;
};
static int gradient_tables(qsv_t* h, const std::vector<Circuit*>& circs, const int* circuit_ids, const int64_t* wrt_offsets,
                           const int32_t* wrt, int base_width, int out_width, GradTables& tab) {
    const size_t n_evals = circs.size();
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    std::vector<GradRow>& rows = tab.rows;
    std::vector<GradEntry>& entries = tab.entries;
    rows.clear();
    entries.clear();
    tab.offsets.assign(n_evals + 1, 0);
    const double shifts[4] = {grad_shift1(), -grad_shift1(), grad_shift3(), -grad_shift3()};
    for (size_t e = 0; e < n_evals; ++e) {
        const Circuit& c = *circs[e];
        if (base_width < c.n_params) return too_few_values(h, c.n_params, base_width);
        WrtRequest asked;
        if (const int rc = wrt_request(h, c, circuit_ids[e], e, wrt_offsets, wrt, out_width, "gradient entries", asked)) return rc;
        for (int64_t j = 0; j < asked.count; ++j) {
            const int64_t p = wrt_offsets ? int64_t(wrt[asked.first + j]) : j;
            const int32_t t = c.grad_terms[size_t(p)];
            if (t < 0)
                return fail(h, QSV_E_UNSUPPORTED, "parameter " + std::to_string(p) + " of circuit " + std::to_string(circuit_ids[e]) +
                                                      " is read by more than one angle slot: no shift rule");
            entries.push_back(GradEntry{int64_t(rows.size()), t, 0});
            for (int32_t k = 0; k < t; ++k) rows.push_back(GradRow{int32_t(e), int32_t(p), shifts[k]});
        }
        tab.offsets[e + 1] = int64_t(entries.size());
    }
    return QSV_OK;
}

// What a gradient call queues once its tables are in device memory: chunk by chunk the expansion kernel and the shifted
// evaluations -- one batch of the ordinary driver each, values from and results into device memory, expectation_to_device --,
// then the combination kernel.  host_rows: the host's copy of the T rows (which evaluation's circuit a shifted row runs).
// Everything on the handle's stream; returns without waiting for the last chunk.  plan_id: a plan's run -- its one chunk, if it
// is one, is remembered under that id (expectation_to_device).
static int gradient_chunks(qsv_t* h, const std::vector<Circuit*>& circs, const GradRow* host_rows, size_t T, size_t chunk, const GradRow* d_rows,
                           const GradEntry* d_entries, const int64_t* d_offsets, const GradCall& call, const int* plan_id) {
    const size_t n_evals = circs.size();
    int rc;
    int64_t& allocations = h->grad_stats.n_allocations;
    if ((rc = ensure_counted(h, h->d_grad_values, std::max<size_t>(1, T) * sizeof(double), allocations))) return rc;
    double* values = static_cast<double*>(h->d_grad_values.ptr);
    // the shifted rows: even width, so that every row starts on 16 bytes (an evaluation takes the first n_params of its row)
    const int width = (std::max(call.base_width, 1) + 1) / 2 * 2;
    const size_t row_bytes = size_t(width) * sizeof(double);
    if (T > 0 && (rc = ensure_doubling(h, h->d_grad_rows, std::min(T, chunk) * row_bytes, chunk * row_bytes, allocations))) return rc;
    double* matrix = static_cast<double*>(h->d_grad_rows.ptr);
    BatchArgs args;
    for (size_t t0 = 0; t0 < T; t0 += chunk) {
        const size_t tc = std::min(chunk, T - t0);
        if (t0 > 0 && (rc = wait_pending(h))) return rc;  // (the chunk before this one may still be reading the rows)
        QSV_HIP(h, launch_gradient_expand(call.base, call.base_stride, call.base_width, d_rows + t0, int64_t(tc), matrix, width, h->stream));
        args.circs.resize(tc);
        for (size_t t = 0; t < tc; ++t) args.circs[t] = circs[size_t(host_rows[t0 + t].base_row)];
        args.n_params.assign(tc, int64_t(width));
        args.device_values = matrix;
        if ((rc = expectation_to_device(h, args, values + t0, T <= chunk ? plan_id : nullptr))) return rc;
        h->grad_stats.n_chunks += 1;
    }
    QSV_HIP(h, launch_gradient_combine(values, d_entries, d_offsets, int64_t(n_evals), call.out_width, grad_cp(), grad_cm(), call.out, h->stream));
    return QSV_OK;
}

// Gradients of circs[e] at row e of call.base by the parameters wrt[wrt_offsets[e] .. wrt_offsets[e + 1]) (wrt_offsets null:
// by every parameter) into row e of call.out: the shift tables, through the handle's pinned table into its device table, then
// gradient_chunks.
static int gradient_locked(qsv_t* h, const std::vector<Circuit*>& circs, const int* circuit_ids, const int64_t* wrt_offsets,
                           const int32_t* wrt, const GradCall& call, int64_t* out_n_shifted) {
    const size_t n_evals = circs.size();
    GradTables tab;
    int rc = gradient_tables(h, circs, circuit_ids, wrt_offsets, wrt, call.base_width, call.out_width, tab);
    if (rc) return rc;
    const std::vector<GradRow>& rows = tab.rows;
    const std::vector<GradEntry>& entries = tab.entries;
    const std::vector<int64_t>& offsets = tab.offsets;
    const size_t T = rows.size();
    if (out_n_shifted) *out_n_shifted = int64_t(T);
    h->grad_stats.n_shifted = int64_t(T);
    h->grad_stats.n_chunks = 0;
    if (n_evals == 0 || call.out_width <= 0) return QSV_OK;
    // the three tables, back to back (each a multiple of 8 bytes), through pinned memory
    const size_t rows_bytes = T * sizeof(GradRow), entries_bytes = entries.size() * sizeof(GradEntry),
                 tab_bytes = rows_bytes + entries_bytes + offsets.size() * sizeof(int64_t);
    if (h->grad_copy_pending) {  // (the pinned table is written below: the last call's copy must have read it)
        h->host_waits += 1;
        QSV_HIP(h, hipEventSynchronize(h->ev_grad));
        h->grad_copy_pending = false;
    }
    if (!h->ev_grad) QSV_HIP(h, hipEventCreateWithFlags(&h->ev_grad, hipEventDisableTiming));
    if (h->h_grad_tab_bytes < tab_bytes) {
        if (h->h_grad_tab) QSV_HIP(h, hipHostFree(h->h_grad_tab));
        const size_t want = std::max(tab_bytes, 2 * h->h_grad_tab_bytes);
        h->h_grad_tab = nullptr;
        h->h_grad_tab_bytes = 0;
        QSV_HIP(h, hipHostMalloc(&h->h_grad_tab, want, hipHostMallocDefault));
        h->h_grad_tab_bytes = want;
        h->grad_stats.n_allocations += 1;
    }
    if ((rc = ensure_doubling(h, h->d_grad_tab, tab_bytes, size_t(-1) / 4, h->grad_stats.n_allocations))) return rc;
    char* ht = static_cast<char*>(h->h_grad_tab);
    if (rows_bytes) std::memcpy(ht, rows.data(), rows_bytes);
    if (entries_bytes) std::memcpy(ht + rows_bytes, entries.data(), entries_bytes);
    std::memcpy(ht + rows_bytes + entries_bytes, offsets.data(), offsets.size() * sizeof(int64_t));
    char* dt = static_cast<char*>(h->d_grad_tab.ptr);
    QSV_HIP(h, hipMemcpyAsync(dt, ht, tab_bytes, hipMemcpyHostToDevice, h->stream));
    QSV_HIP(h, hipEventRecord(h->ev_grad, h->stream));
    h->grad_copy_pending = true;
    return gradient_chunks(h, circs, rows.data(), T, size_t(std::max(1, h->grad_chunk)), reinterpret_cast<const GradRow*>(dt),
                           reinterpret_cast<const GradEntry*>(dt + rows_bytes),
                           reinterpret_cast<const int64_t*>(dt + rows_bytes + entries_bytes), call, nullptr);
}

int qsv_gradient_describe(int n_ops, const qsv_op* ops, int n_params, int32_t* out_n_terms) {
    if (n_ops < 0 || n_params < 0 || (n_ops > 0 && !ops) || (n_params > 0 && !out_n_terms)) return QSV_E_ARG;
    for (int i = 0; i < n_ops; ++i) {
        if (ops[i].kind > QSV_OP_CU3) return QSV_E_ARG;
        if (ops[i].kind != QSV_OP_ID)
            for (int32_t p : {ops[i].p_theta, ops[i].p_phi, ops[i].p_lambda})
                if (p >= n_params || p < -1) return QSV_E_ARG;
    }
    (void)gradient_plan(n_ops, ops, n_params, out_n_terms);
    return QSV_OK;
}

int qsv_gradient_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          const int64_t* wrt_offsets, const int32_t* wrt, double* out, int64_t* out_n_shifted) {
    QSV_OPEN(h, "qsv_gradient_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets))) return fail(h, QSV_E_ARG, "bad arguments");
    if (out_n_shifted) *out_n_shifted = 0;
    if (n_evals == 0) return QSV_OK;
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args);
    if (rc) return rc;
    // the base points as one matrix, a row per evaluation; the gradient rows as wide as the longest request
    int64_t base_width, out_width;
    std::vector<double> base;
    if ((rc = pack_rows(h, args, wrt_offsets, out, false, base_width, out_width, base))) return rc;
    if ((rc = ensure_counted(h, h->d_grad_base, base.size() * sizeof(double), h->grad_stats.n_allocations))) return rc;
    if ((rc = ensure_counted(h, h->d_grad_out, size_t(n_evals) * size_t(out_width) * sizeof(double), h->grad_stats.n_allocations))) return rc;
    // (`base` outlives the copy: every path below waits for the stream before it returns)
    QSV_HIP(h, hipMemcpyAsync(h->d_grad_base.ptr, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const GradCall call{static_cast<const double*>(h->d_grad_base.ptr), base_width, int(base_width), static_cast<double*>(h->d_grad_out.ptr),
                        int(out_width)};
    rc = gradient_locked(h, args.circs, circuit_ids, wrt_offsets, wrt, call, out_n_shifted);
    if (rc) {
        (void)sync_streams(h);
        return rc;
    }
    return rows_to_host(h, args, wrt_offsets, h->d_grad_out.ptr, out_width, out);
}

// The device forms of the gradient-like calls: points in rows of `width` at device_values, gradients into rows of out_width at
// device_out, both device memory, queued behind ready_event (may be null) on the handle's stream and not waited for.
struct DeviceForm {
    int n_evals;
    const int* circuit_ids;
    int width;
    const double* device_values;
    void* ready_event;
    int out_width;
    double* device_out;
};
static int device_form_guard(qsv_t* h, const DeviceForm& f) {
    if (f.n_evals < 0 || f.width < 0 || f.out_width < 0 ||
        (f.n_evals > 0 && (!f.circuit_ids || (f.out_width > 0 && !f.device_out) || (f.width > 0 && !f.device_values))))
        return fail(h, QSV_E_ARG, "bad arguments");
    return QSV_OK;
}
// Opens one of at least one evaluation: its pointers -- the two above and the call's further outputs `more` (name, pointer; null:
// not given), remembered in `cache` -- are memory of the handle's device, its circuits exist (kept_refusal: resolve_batch's), the
// forward run's `args` read the points where they are, and the stream waits for ready_event.
static int device_form_open(qsv_t* h, const DeviceForm& f, std::initializer_list<std::pair<const char*, const void*>> more, const void** cache,
                            const char* kept_refusal, BatchArgs& args) {
    const void* given[8] = {f.width > 0 ? f.device_values : nullptr, f.out_width > 0 ? f.device_out : nullptr};
    const char* names[8] = {"device_values", "device_out"};
    int count = 2;
    for (const auto& m : more) {
        names[count] = m.first;
        given[count++] = m.second;
    }
    int rc = check_device_pointers(h, given, names, cache, count);
    if (rc) return rc;
    if ((rc = resolve_batch(h, size_t(f.n_evals), f.circuit_ids, nullptr, nullptr, args, kept_refusal))) return rc;
    args.n_params.assign(size_t(f.n_evals), int64_t(f.width));
    args.device_values = f.width > 0 ? f.device_values : nullptr;
    if (f.ready_event) QSV_HIP(h, hipStreamWaitEvent(h->stream, static_cast<hipEvent_t>(f.ready_event), 0));
    return QSV_OK;
}
// ... and ends it: nothing of a failed call may still be running; one that queued its work leaves it pending where `pending` says so.
static int device_form_end(qsv_t* h, int rc, bool pending) {
    if (rc)
        (void)sync_streams(h);
    else if (pending)
        h->async_pending = true;
    return rc;
}

int qsv_gradient_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                        const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out, int64_t* out_n_shifted) {
    QSV_OPEN(h, "qsv_gradient_device", kDevice);
    const DeviceForm form{n_evals, circuit_ids, width, device_values, ready_event, out_width, device_out};
    int rc = device_form_guard(h, form);
    if (rc) return rc;
    if (out_n_shifted) *out_n_shifted = 0;
    if (n_evals == 0) return QSV_OK;
    BatchArgs args;
    if ((rc = device_form_open(h, form, {}, h->grad_checked, nullptr, args))) return rc;
    const GradCall call{device_values, int64_t(width), width, device_out, out_width};
    // (the shifted evaluations are batches of the ordinary driver, which keeps async_pending itself)
    return device_form_end(h, gradient_locked(h, args.circs, circuit_ids, wrt_offsets, wrt, call, out_n_shifted), false);
}

int qsv_gradient_stats(const qsv_t* h, qsv_gradient_stats_t* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_gradient_stats", kHostOnly);
    *out = h->grad_stats;
    out->scratch_bytes = int64_t(h->d_grad_tab.bytes + h->d_grad_rows.bytes + h->d_grad_values.bytes + h->d_grad_base.bytes + h->d_grad_out.bytes);
    return QSV_OK;
}

// ---- adjoint gradients (qsv.h: ADJOINT GRADIENTS; adjoint.hpp) -----------------------------------------------------------------

int qsv_adjoint_describe(int n_qubits, int n_ops, const qsv_op* ops, int n_params, int n_wrt, const int32_t* wrt, int capacity_runs,
                         uint64_t* out_masks, int32_t* out_first_op, int32_t* out_last_op, int64_t* out_n_gates,
                         int32_t* out_tile_bits, int32_t* out_low_bits) {
    if (capacity_runs < 0 || (capacity_runs > 0 && (!out_masks || !out_first_op || !out_last_op))) return QSV_E_ARG;
    AdjointPlan plan;
    const int rc = adjoint_plan(n_qubits, n_ops, ops, n_params, n_wrt, wrt, &plan);
    if (rc) return rc;
    for (size_t r = 0; r < plan.runs.size() && r < size_t(capacity_runs); ++r) {
        out_masks[r] = plan.runs[r].mask;
        out_first_op[r] = plan.runs[r].first_op;
        out_last_op[r] = plan.runs[r].last_op;
    }
    if (out_n_gates) *out_n_gates = int64_t(plan.gates.size());
    if (out_tile_bits) *out_tile_bits = kAdjointTileBits;
    if (out_low_bits) *out_low_bits = kAdjointLowBits;
    return int(plan.runs.size());
}

// The points and the output of an adjoint call, all in device memory.
struct AdjCall {
    const double* base;
    int width;
    double* out;
    int out_width;
    double* out_values;
};
// The deflated cost's extension of the sweep's seed: lambda_G = H_h psi + sum_k betas[k] c_k phi_k against the
// kept states `refs`, c_k = <phi_k|psi> from the overlap panels.  With it AdjCall::out_values receives the cost
// E + sum_k betas[k] |c_k|^2; out_energies (E) and out_overlaps ([row][k][2]) are device memory and may be null.  `timer`
// (may be null): under option "time_moments" the deflate kernel of every group is a span of it.
struct AdjSeed {
    uint32_t n_refs = 0;
    OverlapRefs refs{};
    const double* betas = nullptr;  // host memory
    double* out_energies = nullptr;
    double* out_overlaps = nullptr;
    SpanTimer* timer = nullptr;
    // The exact CVaR's seed instead (cvar_seed's): lambda_G = diag(w) psi, w_i = -max(t - v_i, 0) / alpha at the
    // threshold t the search finds in the group's states (`clipped`; not clipped, alpha within numpy.isclose of 1: H_h psi, the plain
    // call).  AdjCall::out_values then receives the CVaR, out_thresholds (device memory, may be null) t.
    bool cvar = false, clipped = false;
    double alpha = 1.0;
    double* out_thresholds = nullptr;
    // The folded cost's seed instead (folded_seed's): lambda_G = (H_h - c) r - (E - c)^2 psi, r = H_h psi - c psi,
    // c the call's `target` or (own_mean) the evaluation's own E.  AdjCall::out_values then receives |r|^2, out_energies E.
    bool folded = false, own_mean = false;
    double target = 0.0;
};

// What both entry points run with the lock held: the call's tables, the forward run group by group, and behind each group the H
// application (a clipped CVaR seed: the threshold search and the seed pass in its place), the runs and the combination on the
// handle's stream.  Returns without waiting.
static int adjoint_locked(qsv_t* h, BatchArgs& args, const int* circuit_ids, const int64_t* wrt_offsets, const int32_t* wrt,
                          const AdjCall& call, const AdjSeed* seed = nullptr) {
    const size_t n_evals = args.circs.size();
    const size_t K = seed ? size_t(seed->n_refs) : 0;
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    h->adj_stats.n_gates = h->adj_stats.n_runs = h->adj_stats.n_state_sweeps = 0;
    // ---- the tables: per distinct circuit its swept gates and runs (adjoint_plan.hpp: sweep_tables_add) and, flattened, the slots
    // that read each parameter; per evaluation its entries
    struct CircuitSlots {
        uint32_t slot_base = 0;
        std::vector<uint32_t> slot_first;  // per parameter: its slots are slots[slot_base + slot_first[p] .. + slot_first[p + 1])
    };
    SweepTables tables;
    std::unordered_map<const SweepCircuit*, CircuitSlots> slots_of;
    std::vector<uint32_t> slots;
    std::vector<AdjEntry> entries;
    std::vector<int64_t> entry_offsets(n_evals + 1, 0);
    std::vector<uint32_t> eval_runs(n_evals, 0), eval_gates(n_evals, 0);
    uint32_t max_gates = 0;
    for (size_t e = 0; e < n_evals; ++e) {
        const Circuit& c = *args.circs[e];
        if (call.width < c.n_params) return too_few_values(h, c.n_params, call.width);
        WrtRequest asked;
        if (const int rc = wrt_request(h, c, circuit_ids[e], e, wrt_offsets, wrt, call.out_width, "gradient entries", asked)) return rc;
        const int64_t first = asked.first, count = asked.count;
        const SweepCircuit* const t = sweep_tables_add(tables, &c, h->n, int(c.ops.size()), c.ops.data(), c.n_params);
        if (!t) return fail(h, QSV_E_ARG, "circuit " + std::to_string(circuit_ids[e]) + " cannot be planned for the adjoint sweep");
        CircuitSlots& s = slots_of[t];
        if (s.slot_first.empty()) {  // (the circuit's first evaluation)
            s.slot_base = uint32_t(slots.size());
            s.slot_first.assign(size_t(c.n_params) + 1, 0);
            for (int p = 0; p < c.n_params; ++p) {
                slots.insert(slots.end(), t->readers[size_t(p)].begin(), t->readers[size_t(p)].end());
                s.slot_first[size_t(p) + 1] = s.slot_first[size_t(p)] + uint32_t(t->readers[size_t(p)].size());
            }
        }
        if (wrt_offsets) {  // (its own sweep: the front part of the circuit's that reaches the earliest gate reading one of ITS parameters)
            AdjointPlan own;
            (void)adjoint_plan(h->n, int(c.ops.size()), c.ops.data(), c.n_params, int(count), wrt + first, &own);
            eval_runs[e] = uint32_t(own.runs.size());
            eval_gates[e] = uint32_t(own.gates.size());
        } else {
            eval_runs[e] = t->n_runs;
            eval_gates[e] = t->n_gates;
        }
        max_gates = std::max(max_gates, eval_gates[e]);
        for (int64_t j = 0; j < count; ++j) {
            const size_t p = size_t(wrt_offsets ? int64_t(wrt[first + j]) : j);
            entries.push_back(AdjEntry{s.slot_base + s.slot_first[p], s.slot_first[p + 1] - s.slot_first[p]});
        }
        entry_offsets[e + 1] = int64_t(entries.size());
        h->adj_stats.n_gates += int64_t(eval_gates[e]);
        h->adj_stats.n_state_sweeps += 1 + int64_t(eval_runs[e]);
    }
    if (n_evals == 0) return QSV_OK;

    // ---- the forward run's layout (ordinary plans into state slots, never split: as qsv_prefix_create runs them)
    // (against kept states the group is the overlap panels' where that is smaller: their partial tiles stay under 64 MiB)
    const size_t G_sweep = std::max<size_t>(1, std::min<size_t>(size_t(h->group), 4096));
    const size_t G = K ? overlap_group(h->n, K, false, std::min(G_sweep, size_t(std::max(1, h->max_grid_y)))) : G_sweep;
    const StateRun run{SplitRule{}, 1, G, false, 0, kModeSynthFirst | kModeFinalStore};
    BatchRelease release{h};
    StateLayout lay;
    h->prof = qsv_profile{};
    int rc = lay_out_states(h, args, run, lay);
    if (rc) return rc;
    std::vector<AdjEval> evals(n_evals);
    for (size_t j = 0; j < n_evals; ++j) {
        const size_t e = h->batch.eval_at[j];
        const SweepCircuit& t = tables.circuits.at(args.circs[e]);
        evals[j] = AdjEval{t.gate_base, t.run_base, eval_runs[e], eval_gates[e], uint32_t(e), 0};
    }
    // one blob: [gates][runs][entries][entry offsets][slots][evaluations by position][the seed's betas]
    TableBlob blob;
    const size_t off_gates = blob.add(tables.gates), off_runs = blob.add(tables.runs), off_entries = blob.add(entries),
                 off_offsets = blob.add(entry_offsets), off_slots = blob.add(slots), off_evals = blob.add(evals),
                 off_betas = blob.add(K ? seed->betas : nullptr, K * sizeof(double));
    const size_t gc_max = std::min(G, n_evals);
    const uint64_t dim = uint64_t(1) << h->n;
    const uint32_t blocks = adjoint_blocks(h->n), op_blocks = adjoint_op_blocks(h->n);
    int64_t& allocations = h->adj_stats.n_allocations;
    // (lay_out_states has waited for whatever an earlier call without a wait left running: nothing reads the old tables)
    if ((rc = upload_blob(h, h->d_adj_tab, blob, allocations)) || (rc = ensure_counted(h, h->d_adj_lambda, gc_max * dim * h->amp_bytes, allocations)) ||
        (rc = ensure_counted(h, h->d_adj_mats, gc_max * std::max<size_t>(1, max_gates) * kAdjointMatDoubles * sizeof(double), allocations)) ||
        (rc = ensure_counted(h, h->d_adj_partials, gc_max * 3 * std::max<size_t>(1, max_gates) * blocks * sizeof(double), allocations)) ||
        (rc = ensure_counted(h, h->d_adj_epart, gc_max * op_blocks * sizeof(double), allocations)))
        return rc;
    // the seed's scratch: the group's overlaps by position | the panels' partial tiles
    const size_t ovl_bytes = (gc_max * K * 2 * sizeof(double) + 63) / 64 * 64;
    if (K && (rc = ensure_counted(h, h->d_defl, ovl_bytes + overlap_partial_bytes(h->n, K, false, gc_max), allocations))) return rc;
    const bool clipped = seed && seed->clipped;
    if (clipped && (rc = ensure_counted(h, h->d_cvar_grad, cvar_gradient_scratch_doubles(h->n, gc_max) * sizeof(double), allocations))) return rc;
    double* const cvar_scratch = static_cast<double*>(h->d_cvar_grad.ptr);
    // the folded seed's scratch; the residuals only where the row gathers (x-mask groups) and some evaluation sweeps a gate
    const bool folded = seed && seed->folded, folded_gathers = folded && h->n_groups > 0;
    const bool any_run = std::any_of(eval_runs.begin(), eval_runs.end(), [](uint32_t r) { return r > 0; });
    if (folded && ((rc = ensure_counted(h, h->d_fold, folded_scratch_doubles(h->n, gc_max) * sizeof(double), allocations)) ||
                   (folded_gathers && any_run && (rc = ensure_counted(h, h->d_fold_r, gc_max * dim * h->amp_bytes, allocations)))))
        return rc;
    double* const fold_scratch = static_cast<double*>(h->d_fold.ptr);
    const double* const sorted = static_cast<const double*>(h->d_sorted.ptr);  // (a CVaR seed's: sorted_values_ready)
    const void* dt = h->d_adj_tab.ptr;
    const AdjGate* d_gates = TableBlob::at<AdjGate>(dt, off_gates);
    const AdjRunDesc* d_runs = TableBlob::at<AdjRunDesc>(dt, off_runs);
    const AdjEntry* d_entries = TableBlob::at<AdjEntry>(dt, off_entries);
    const int64_t* d_offsets = TableBlob::at<int64_t>(dt, off_offsets);
    const uint32_t* d_slots = TableBlob::at<uint32_t>(dt, off_slots);
    const AdjEval* d_evals = TableBlob::at<AdjEval>(dt, off_evals);
    const double* d_betas = TableBlob::at<double>(dt, off_betas);
    double* d_ovl = static_cast<double*>(h->d_defl.ptr);
    double* ovl_partials = K ? reinterpret_cast<double*>(static_cast<char*>(h->d_defl.ptr) + ovl_bytes) : nullptr;
    // E goes where the caller wants it apart from the cost; the cost is written behind it by the seed's finishing kernel
    // (the folded seed's finishing kernel writes both itself)
    double* const d_energies = folded ? nullptr : seed && seed->out_energies ? seed->out_energies : call.out_values;
    double* mats = static_cast<double*>(h->d_adj_mats.ptr);
    double* partials = static_cast<double*>(h->d_adj_partials.ptr);
    double* e_partials = static_cast<double*>(h->d_adj_epart.ptr);
    const bool streaming = h->stream_mode != 0;
    auto sweep = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_adjoint_prepare(d_evals + g0, int(gc), d_gates, max_gates, call.base, call.width, mats, h->stream));
        uint32_t most_runs = 0;
        for (size_t j = g0; j < g0 + gc; ++j) most_runs = std::max(most_runs, evals[j].n_runs);
        if (clipped) {
            // t and s from the amplitudes while the states are still the final ones, then the clipped seed in H psi's place (its
            // lambda is stored where a gate is swept at all)
            QSV_HIP(h, launch_cvar_gradient_threshold(h->dtype, h->d_states.ptr, h->n, int(gc), static_cast<const uint32_t*>(h->d_order.ptr),
                                                      sorted, seed->alpha, cvar_scratch, h->stream));
            QSV_HIP(h, launch_cvar_gradient_seed(h->dtype, h->d_states.ptr, most_runs > 0 ? h->d_adj_lambda.ptr : nullptr, h->n, int(gc),
                                                 static_cast<const double*>(h->d_diag.ptr), cvar_scratch, seed->alpha, streaming, e_partials,
                                                 h->stream));
        } else {
            QSV_HIP(h, launch_adjoint_apply_operator(h->dtype, h->d_states.ptr, h->d_adj_lambda.ptr, h->n, int(gc), operator_view(h), streaming,
                                                     e_partials, h->stream));
        }
        if (folded) {
            // E and the centre from the shares, r = lambda_1 - c psi with the shares of |r|^2, then -- where a gate is swept at all --
            // lambda_G = (H_h - c) r - (E - c)^2 psi over lambda_1; an operator of its diagonal part alone: both in one pass
            const bool sweeps = most_runs > 0;
            QSV_HIP(h, launch_folded_centre(e_partials, op_blocks, int(gc), seed->own_mean, seed->target, fold_scratch, h->stream));
            if (!folded_gathers) {
                QSV_HIP(h, launch_folded_diagonal(h->dtype, h->d_states.ptr, sweeps ? h->d_adj_lambda.ptr : nullptr, h->n, int(gc),
                                                  operator_view(h).diag, fold_scratch, streaming, h->stream));
            } else {
                QSV_HIP(h, launch_folded_residual(h->dtype, h->d_states.ptr, h->d_adj_lambda.ptr, sweeps ? h->d_fold_r.ptr : nullptr, h->n,
                                                  int(gc), fold_scratch, streaming, h->stream));
                if (sweeps)
                    QSV_HIP(h, launch_folded_seed(h->dtype, h->d_states.ptr, h->d_fold_r.ptr, h->d_adj_lambda.ptr, h->n, int(gc), operator_view(h), fold_scratch,
                                                  streaming, h->stream));
            }
            h->adj_stats.n_state_sweeps += int64_t(gc) * (folded_gathers && sweeps ? 2 : 1);
        }
        if (K) {
            // c = Phi^H Psi while the states are still the final ones (the runs rewrite them), then -- where a gate is swept at all --
            // lambda += sum_k beta_k c_k phi_k
            QSV_HIP(h, launch_overlap_panels(h->dtype, h->d_states.ptr, h->d_prefix.ptr, seed->refs, uint32_t(K), h->n, int(gc), kNoOperator,
                                             ovl_partials, h->stream));
            QSV_HIP(h, launch_overlap_combine(ovl_partials, h->n, int(gc), uint32_t(K), d_ovl, nullptr, h->stream));
            if (most_runs > 0) {
                const bool timing = h->time_moments && seed->timer;
                if (timing) QSV_HIP(h, seed->timer->begin(h->stream));
                QSV_HIP(h, launch_deflate(h->dtype, h->d_adj_lambda.ptr, h->d_prefix.ptr, seed->refs, uint32_t(K), h->n, int(gc), d_betas, d_ovl,
                                          streaming, h->stream));
                if (timing) QSV_HIP(h, seed->timer->end(h->stream));
                h->adj_stats.n_state_sweeps += int64_t(gc);
            }
        }
        for (uint32_t r = 0; r < most_runs; ++r) {
            QSV_HIP(h, launch_adjoint_run(h->dtype, h->d_states.ptr, h->d_adj_lambda.ptr, h->n, int(gc), r, d_evals + g0, d_runs, d_gates, mats,
                                          max_gates, streaming, partials, h->stream));
            h->adj_stats.n_runs += 1;
        }
        QSV_HIP(h, launch_adjoint_combine(d_evals + g0, int(gc), d_offsets, d_entries, d_slots, partials, max_gates, blocks, e_partials,
                                          op_blocks, call.out_width, call.out, d_energies, h->stream));
        if (folded)
            QSV_HIP(h, launch_folded_finish(d_evals + g0, int(gc), h->n, fold_scratch, call.out_values, seed->out_energies, h->stream));
        else if (seed && (K || (seed->out_energies && call.out_values)))
            QSV_HIP(h, launch_deflation_finish(d_evals + g0, int(gc), uint32_t(K), d_betas, d_ovl, d_energies, call.out_values,
                                               K ? seed->out_overlaps : nullptr, h->stream));
        if (seed && seed->cvar)
            QSV_HIP(h, launch_cvar_gradient_finish(d_evals + g0, int(gc), clipped ? cvar_scratch : nullptr, seed->alpha, sorted + (dim - 1),
                                                   call.out_values, seed->out_thresholds, h->stream));
        return QSV_OK;
    };
    return run_laid_out(h, args, run, lay, {}, sweep);
}

// The host form of the adjoint call and, with `seed` (deflation_seed's), of the deflated one, whose energies and overlaps then go
// to out_energies / out_overlaps (may be null), or (cvar_seed's) of the CVaR one, whose thresholds go to out_thresholds (may be
// null): the points as one matrix in device memory, a row per evaluation (rows of an even number of doubles), the gradient rows
// as wide as the longest request, everything back after one wait.
static int adjoint_host_form(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                             const int64_t* wrt_offsets, const int32_t* wrt, double* out, double* out_values, const char* kept_refusal,
                             AdjSeed* seed = nullptr, double* out_energies = nullptr, double* out_overlaps = nullptr,
                             double* out_thresholds = nullptr) {
    BatchArgs packed, args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, packed, kept_refusal);
    if (rc) return rc;
    int64_t width, out_width;
    std::vector<double> base;
    if ((rc = pack_rows(h, packed, wrt_offsets, out, true, width, out_width, base))) return rc;
    // (behind the values: the deflated call's energies | overlaps, or the CVaR call's thresholds)
    const size_t n = size_t(n_evals), K = seed ? size_t(seed->n_refs) : 0, n_extra = seed ? n + n * K * 2 : 0;
    int64_t& allocations = h->adj_stats.n_allocations;
    if ((rc = rows_to_device(h, packed, base, width, h->d_adj_base, allocations, args)) ||
        (rc = ensure_counted(h, h->d_adj_out, n * size_t(out_width) * sizeof(double), allocations)) ||
        (rc = ensure_counted(h, h->d_adj_values, n * sizeof(double), allocations)) ||
        (seed && (rc = ensure_counted(h, h->d_defl_out, n_extra * sizeof(double), allocations))))
        return rc;
    const AdjCall call{args.device_values, int(width), static_cast<double*>(h->d_adj_out.ptr), int(out_width), static_cast<double*>(h->d_adj_values.ptr)};
    SpanTimer timer;
    double* const d_energies = static_cast<double*>(h->d_defl_out.ptr);
    if (seed) {
        seed->out_energies = out_energies ? d_energies : nullptr;
        seed->out_overlaps = out_overlaps && K ? d_energies + n : nullptr;
        seed->out_thresholds = out_thresholds ? d_energies : nullptr;
        seed->timer = &timer;
    }
    if ((rc = adjoint_locked(h, args, circuit_ids, wrt_offsets, wrt, call, seed))) {
        (void)sync_streams(h);
        return rc;
    }
    std::vector<double> values(n), extra(n_extra);
    const bool any_extra = seed && (seed->out_energies || seed->out_overlaps || seed->out_thresholds);
    if ((rc = rows_to_host(h, packed, wrt_offsets, h->d_adj_out.ptr, out_width, out,
                           {{h->d_adj_values.ptr, values.data(), n}, {d_energies, extra.data(), any_extra ? n_extra : 0}})))
        return rc;
    QSV_HIP(h, timer.elapsed(0, h->prof.expect_ms));
    if (out_values) std::memcpy(out_values, values.data(), n * sizeof(double));
    if (seed && out_energies) std::memcpy(out_energies, extra.data(), n * sizeof(double));
    if (seed && seed->out_overlaps) std::memcpy(out_overlaps, extra.data() + n, n * K * 2 * sizeof(double));
    if (seed && out_thresholds) std::memcpy(out_thresholds, extra.data(), n * sizeof(double));
    return QSV_OK;
}

int qsv_adjoint_gradient_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                                  const int64_t* wrt_offsets, const int32_t* wrt, double* out, double* out_values) {
    QSV_OPEN(h, "qsv_adjoint_gradient_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets))) return fail(h, QSV_E_ARG, "bad arguments");
    if (n_evals == 0) return QSV_OK;
    return adjoint_host_form(h, n_evals, circuit_ids, param_offsets, params, wrt_offsets, wrt, out, out_values,
                             "adjoint gradients of a circuit on a kept state are not built");
}

int qsv_adjoint_gradient_device(qsv_t* h, int n_evals, const int* circuit_ids, int width, const double* device_values, void* ready_event,
                                const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out, double* device_out_values) {
    QSV_OPEN(h, "qsv_adjoint_gradient_device", kDevice);
    const DeviceForm form{n_evals, circuit_ids, width, device_values, ready_event, out_width, device_out};
    int rc = device_form_guard(h, form);
    if (rc || n_evals == 0) return rc;
    BatchArgs args;
    if ((rc = device_form_open(h, form, {{"device_out_values", device_out_values}}, h->adj_checked,
                               "adjoint gradients of a circuit on a kept state are not built", args)))
        return rc;
    const AdjCall call{device_values, width, device_out, out_width, device_out_values};
    return device_form_end(h, adjoint_locked(h, args, circuit_ids, wrt_offsets, wrt, call), true);
}

// ---- deflated costs against kept states (qsv.h: DEFLATED COSTS; deflation.hpp) -----------------------------------------------------

// The kept states and weights of a deflated call, checked, as adjoint_locked's seed extension.
static int deflation_seed(qsv_t* h, int n_states, const int* prefix_ids, const double* betas, int n_evals, AdjSeed& seed) {
    if (n_states < 0) return fail(h, QSV_E_ARG, "n_states is negative");
    if (n_states > int(kOvlMaxStates)) return fail(h, QSV_E_UNSUPPORTED, "n_states: deflated costs are available against up to 64 kept states per call");
    if (n_states > 0 && !prefix_ids) return fail(h, QSV_E_ARG, "prefix_ids is null");
    if (n_states > 0 && !betas) return fail(h, QSV_E_ARG, "betas is null");
    for (int k = 0; k < n_states; ++k)
        if (!std::isfinite(betas[k])) return fail(h, QSV_E_ARG, "betas[" + std::to_string(k) + "] is not finite");
    // (the register's size is the handle's own: asked before the kept states, which such a handle need not hold)
    if (n_evals > 0)
        if (const int rc = qubit_guard(h, "deflated costs are available up to 28 qubits", true)) return rc;
    seed.n_refs = uint32_t(n_states);
    seed.betas = betas;
    return kept_refs(h, n_states, prefix_ids, seed.refs);
}

int qsv_deflated_gradient_circuits(qsv_t* h, int n_states, const int* prefix_ids, const double* betas, int n_evals, const int* circuit_ids,
                                   const int64_t* param_offsets, const double* params, const int64_t* wrt_offsets, const int32_t* wrt,
                                   double* out, double* out_values, double* out_energies, double* out_overlaps) {
    QSV_OPEN(h, "qsv_deflated_gradient_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets))) return fail(h, QSV_E_ARG, "bad arguments");
    AdjSeed seed;
    int rc = deflation_seed(h, n_states, prefix_ids, betas, n_evals, seed);
    if (rc) return rc;
    if (n_evals == 0) return QSV_OK;
    return adjoint_host_form(h, n_evals, circuit_ids, param_offsets, params, wrt_offsets, wrt, out, out_values,
                             "deflated gradients of a circuit on a kept state are not built", &seed, out_energies, out_overlaps);
}

int qsv_deflated_gradient_device(qsv_t* h, int n_states, const int* prefix_ids, const double* betas, int n_evals, const int* circuit_ids,
                                 int width, const double* device_values, void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt,
                                 int out_width, double* device_out, double* device_out_values, double* device_out_energies,
                                 double* device_out_overlaps) {
    QSV_OPEN(h, "qsv_deflated_gradient_device", kDevice);
    const DeviceForm form{n_evals, circuit_ids, width, device_values, ready_event, out_width, device_out};
    int rc = device_form_guard(h, form);
    if (rc) return rc;
    AdjSeed seed;
    if ((rc = deflation_seed(h, n_states, prefix_ids, betas, n_evals, seed)) || n_evals == 0) return rc;
    seed.out_energies = device_out_energies;
    seed.out_overlaps = n_states > 0 ? device_out_overlaps : nullptr;
    BatchArgs args;
    if ((rc = device_form_open(h, form, {{"device_out_values", device_out_values}, {"device_out_energies", seed.out_energies}, {"device_out_overlaps", seed.out_overlaps}},
                               h->defl_checked, "deflated gradients of a circuit on a kept state are not built", args)))
        return rc;
    const AdjCall call{device_values, width, device_out, out_width, device_out_values};
    return device_form_end(h, adjoint_locked(h, args, circuit_ids, wrt_offsets, wrt, call, &seed), true);
}

// ---- exact CVaR gradients (qsv.h: EXACT CVAR GRADIENTS; cvar_gradient.hpp) ---------------------------------------------------------

// alpha and the operator of a CVaR call, checked, as adjoint_locked's seed; with an evaluation to run, the operator's values sorted.
static int cvar_seed(qsv_t* h, double alpha, int n_evals, AdjSeed& seed) {
    if (!(alpha > 0.0) || alpha > 1.0) return fail(h, QSV_E_ARG, "alpha must be in (0, 1]");
    seed.cvar = true;
    seed.alpha = alpha;
    seed.clipped = !cvar_alpha_is_one(alpha);
    if (n_evals == 0) return QSV_OK;
    int rc;
    if ((rc = cvar_operator_guard(h)) || (rc = qubit_guard(h, "the exact CVaR's gradient is available up to 28 qubits"))) return rc;
    return sorted_values_ready(h);
}

int qsv_cvar_gradient_circuits(qsv_t* h, double alpha, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                               const double* params, const int64_t* wrt_offsets, const int32_t* wrt, double* out, double* out_values,
                               double* out_thresholds) {
    QSV_OPEN(h, "qsv_cvar_gradient_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets))) return fail(h, QSV_E_ARG, "bad arguments");
    AdjSeed seed;
    int rc = cvar_seed(h, alpha, n_evals, seed);
    if (rc || n_evals == 0) return rc;
    return adjoint_host_form(h, n_evals, circuit_ids, param_offsets, params, wrt_offsets, wrt, out, out_values,
                             "CVaR gradients of a circuit on a kept state are not built", &seed, nullptr, nullptr, out_thresholds);
}

int qsv_cvar_gradient_device(qsv_t* h, double alpha, int n_evals, const int* circuit_ids, int width, const double* device_values,
                             void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* device_out,
                             double* device_out_values, double* device_out_thresholds) {
    QSV_OPEN(h, "qsv_cvar_gradient_device", kDevice);
    const DeviceForm form{n_evals, circuit_ids, width, device_values, ready_event, out_width, device_out};
    int rc = device_form_guard(h, form);
    if (rc) return rc;
    AdjSeed seed;
    if ((rc = cvar_seed(h, alpha, n_evals, seed)) || n_evals == 0) return rc;
    seed.out_thresholds = device_out_thresholds;
    BatchArgs args;
    if ((rc = device_form_open(h, form, {{"device_out_values", device_out_values}, {"device_out_thresholds", device_out_thresholds}},
                               h->cvar_grad_checked, "CVaR gradients of a circuit on a kept state are not built", args)))
        return rc;
    const AdjCall call{device_values, width, device_out, out_width, device_out_values};
    return device_form_end(h, adjoint_locked(h, args, circuit_ids, wrt_offsets, wrt, call, &seed), true);
}

// ---- folded-spectrum and variance costs (qsv.h: FOLDED-SPECTRUM AND VARIANCE COSTS; folded.hpp) --------------------------------------

// The centre of a folded call, checked, as adjoint_locked's seed.
static int folded_seed(qsv_t* h, int centre, double target, int n_evals, AdjSeed& seed) {
    if (centre != 0 && centre != 1) return fail(h, QSV_E_ARG, "centre must be 0 (the target) or 1 (each evaluation's own mean)");
    if (!std::isfinite(target)) return fail(h, QSV_E_ARG, "target is not finite");
    seed.folded = true;
    seed.own_mean = centre == 1;
    seed.target = target;
    if (n_evals == 0) return QSV_OK;
    // (the register's size is asked first: such a handle need not hold an operator's tables)
    if (const int rc = qubit_guard(h, "folded-spectrum costs are available up to 28 qubits", true)) return rc;
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    return QSV_OK;
}

int qsv_folded_gradient_circuits(qsv_t* h, int centre, double target, int n_evals, const int* circuit_ids, const int64_t* param_offsets,
                                 const double* params, const int64_t* wrt_offsets, const int32_t* wrt, double* out, double* out_values,
                                 double* out_energies) {
    QSV_OPEN(h, "qsv_folded_gradient_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets))) return fail(h, QSV_E_ARG, "bad arguments");
    AdjSeed seed;
    int rc = folded_seed(h, centre, target, n_evals, seed);
    if (rc || n_evals == 0) return rc;
    return adjoint_host_form(h, n_evals, circuit_ids, param_offsets, params, wrt_offsets, wrt, out, out_values,
                             "folded-spectrum costs of a circuit on a kept state are not built", &seed, out_energies);
}

int qsv_folded_gradient_device(qsv_t* h, int centre, double target, int n_evals, const int* circuit_ids, int width,
                               const double* device_values, void* ready_event, const int64_t* wrt_offsets, const int32_t* wrt, int out_width,
                               double* device_out, double* device_out_values, double* device_out_energies) {
    QSV_OPEN(h, "qsv_folded_gradient_device", kDevice);
    const DeviceForm form{n_evals, circuit_ids, width, device_values, ready_event, out_width, device_out};
    int rc = device_form_guard(h, form);
    if (rc) return rc;
    AdjSeed seed;
    if ((rc = folded_seed(h, centre, target, n_evals, seed)) || n_evals == 0) return rc;
    seed.out_energies = device_out_energies;
    BatchArgs args;
    if ((rc = device_form_open(h, form, {{"device_out_values", device_out_values}, {"device_out_energies", device_out_energies}},
                               h->fold_checked, "folded-spectrum costs of a circuit on a kept state are not built", args)))
        return rc;
    const AdjCall call{device_values, width, device_out, out_width, device_out_values};
    return device_form_end(h, adjoint_locked(h, args, circuit_ids, wrt_offsets, wrt, call, &seed), true);
}

int qsv_adjoint_stats(const qsv_t* h, qsv_adjoint_stats_t* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_adjoint_stats", kHostOnly);
    *out = h->adj_stats;
    out->scratch_bytes = int64_t(h->d_adj_lambda.bytes + h->d_adj_tab.bytes + h->d_adj_mats.bytes + h->d_adj_partials.bytes + h->d_adj_epart.bytes +
                                 h->d_adj_base.bytes + h->d_adj_out.bytes + h->d_adj_values.bytes + h->d_defl.bytes + h->d_defl_out.bytes +
                                 h->d_cvar_grad.bytes + h->d_fold.bytes + h->d_fold_r.bytes);
    return QSV_OK;
}

// ---- the operator's variance (qsv.h: ENERGY VARIANCE; moments.hpp) -------------------------------------------------------------

int qsv_variance_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                          double* out_variances, double* out_values) {
    QSV_OPEN(h, "qsv_variance_circuits", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out_variances))) return fail(h, QSV_E_ARG, "bad arguments");
    if (n_evals == 0) return QSV_OK;
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    if (const int rc = qubit_guard(h, "the variance is available up to 28 qubits")) return rc;
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args,
                           "the variance of a circuit on a kept state is not built");
    if (rc) return rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers below may still be read or written by a call that did not wait)
    const size_t n = size_t(n_evals);
    const size_t G = std::max<size_t>(1, std::min(size_t(h->group), size_t(h->max_grid_y)));
    const uint32_t blocks = moments_blocks(h->n);
    // device scratch: the call's (E, Var) pairs by position | the partials of one launch group
    const size_t out_bytes = (n * 2 * sizeof(double) + 63) / 64 * 64;
    if ((rc = ensure(h, h->d_moments, out_bytes + std::min(G, n) * blocks * 2 * sizeof(double))) || (rc = ensure_host_out(h, 2 * n))) return rc;
    double* const pairs = static_cast<double*>(h->d_moments.ptr);
    double* const partials = reinterpret_cast<double*>(static_cast<char*>(h->d_moments.ptr) + out_bytes);
    auto moments = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_operator_moments(h->dtype, h->d_states.ptr, h->n, int(gc), operator_view(h), partials, h->stream));
        QSV_HIP(h, launch_moments_combine(partials, blocks, int(gc), pairs + 2 * g0, h->stream));
        return QSV_OK;
    };
    if ((rc = run_whole_states(h, args, G, moments, pairs, 2 * n))) return rc;
    for (size_t j = 0; j < n; ++j) {
        const size_t e = h->batch.eval_at[j];
        if (out_values) out_values[e] = h->h_out[2 * j];
        out_variances[e] = h->h_out[2 * j + 1];
    }
    return QSV_OK;
}

int qsv_gradient_plan_create(qsv_t* h, int n_evals, const int* circuit_ids, int width, const int64_t* wrt_offsets, const int32_t* wrt,
                             int out_width, int* out_plan_id, int64_t* out_n_shifted) {
    QSV_OPEN(h, "qsv_gradient_plan_create", kDevice);
    if (n_evals < 0 || width < 0 || out_width < 0 || !out_plan_id || (n_evals > 0 && !circuit_ids)) return fail(h, QSV_E_ARG, "bad arguments");
    if (out_n_shifted) *out_n_shifted = 0;
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, nullptr, nullptr, args);
    if (rc) return rc;
    GradTables tab;
    if ((rc = gradient_tables(h, args.circs, circuit_ids, wrt_offsets, wrt, width, out_width, tab))) return rc;
    qsv_handle::GradientPlan plan;
    plan.ids.assign(circuit_ids, circuit_ids + n_evals);
    plan.width = width;
    plan.out_width = out_width;
    plan.chunk = size_t(std::max(1, h->grad_chunk));
    plan.n_entries = tab.entries.size();
    const size_t T = tab.rows.size();
    const size_t rows_bytes = T * sizeof(GradRow), entries_bytes = tab.entries.size() * sizeof(GradEntry),
                 tab_bytes = rows_bytes + entries_bytes + tab.offsets.size() * sizeof(int64_t);
    QSV_HIP(h, hipMalloc(&plan.d_tab, tab_bytes));
    // (the host vectors outlive the copies: the wait below)
    char* dt = static_cast<char*>(plan.d_tab);
    hipError_t e = hipSuccess;
    if (rows_bytes) e = hipMemcpyAsync(dt, tab.rows.data(), rows_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && entries_bytes) e = hipMemcpyAsync(dt + rows_bytes, tab.entries.data(), entries_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(dt + rows_bytes + entries_bytes, tab.offsets.data(), tab.offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipFree(plan.d_tab);
        return fail(h, QSV_E_DEVICE, std::string("uploading a gradient plan's tables: ") + hipGetErrorString(e));
    }
    plan.rows = std::move(tab.rows);
    plan.stats.n_shifted = int64_t(T);
    plan.stats.n_chunks = int64_t((T + plan.chunk - 1) / plan.chunk);
    plan.stats.table_bytes = int64_t(tab_bytes);
    if (out_n_shifted) *out_n_shifted = int64_t(T);
    const int id = h->next_grad_plan_id++;
    h->grad_plans.emplace(id, std::move(plan));
    *out_plan_id = id;
    return QSV_OK;
}

int qsv_gradient_plan_run(qsv_t* h, int plan_id, const double* device_values, void* ready_event, double* device_out) {
    QSV_OPEN(h, "qsv_gradient_plan_run", kDevice);
    const auto it = h->grad_plans.find(plan_id);
    if (it == h->grad_plans.end()) return fail(h, QSV_E_ARG, "unknown gradient plan " + std::to_string(plan_id));
    qsv_handle::GradientPlan& plan = it->second;
    const size_t n_evals = plan.ids.size();
    if (n_evals > 0 && ((plan.out_width > 0 && !device_out) || (plan.width > 0 && !device_values))) return fail(h, QSV_E_ARG, "bad arguments");
    if (n_evals == 0) return QSV_OK;
    const void* given[2] = {plan.width > 0 ? device_values : nullptr, plan.out_width > 0 ? device_out : nullptr};
    static const char* const names[2] = {"device_values", "device_out"};
    int rc = check_device_pointers(h, given, names, h->grad_checked, 2);  // (the cache of qsv_gradient_device)
    if (rc) return rc;
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    BatchArgs args;
    if ((rc = resolve_batch(h, n_evals, plan.ids.data(), nullptr, nullptr, args))) return rc;
    const uint64_t waits_before = h->host_waits;
    if (ready_event) QSV_HIP(h, hipStreamWaitEvent(h->stream, static_cast<hipEvent_t>(ready_event), 0));
    const size_t T = plan.rows.size();
    h->grad_stats.n_shifted = int64_t(T);
    h->grad_stats.n_chunks = 0;
    if (plan.out_width > 0) {
        const char* dt = static_cast<const char*>(plan.d_tab);
        const size_t rows_bytes = T * sizeof(GradRow), entries_bytes = plan.n_entries * sizeof(GradEntry);
        const GradCall call{device_values, int64_t(plan.width), plan.width, device_out, plan.out_width};
        rc = gradient_chunks(h, args.circs, plan.rows.data(), T, plan.chunk, reinterpret_cast<const GradRow*>(dt),
                             reinterpret_cast<const GradEntry*>(dt + rows_bytes),
                             reinterpret_cast<const int64_t*>(dt + rows_bytes + entries_bytes), call, &plan_id);
        if (rc) (void)sync_streams(h);  // nothing of a failed call may still be running
    }
    plan.stats.n_host_waits += int64_t(h->host_waits - waits_before);
    if (!rc) plan.stats.n_runs += 1;
    return rc;
}

int qsv_gradient_plan_destroy(qsv_t* h, int plan_id) {
    QSV_OPEN(h, "qsv_gradient_plan_destroy", kDevice);
    const auto it = h->grad_plans.find(plan_id);
    if (it == h->grad_plans.end()) return fail(h, QSV_E_ARG, "unknown gradient plan " + std::to_string(plan_id));
    QSV_HIP(h, sync_streams(h));  // (a run's kernels may still read the tables)
    h->async_pending = false;
    if (h->plan_snap.plan_id == plan_id) h->plan_snap.epoch = 0;
    if (it->second.d_tab) (void)hipFree(it->second.d_tab);
    h->grad_plans.erase(it);
    return QSV_OK;
}

int qsv_gradient_plan_stats(const qsv_t* h, int plan_id, qsv_gradient_plan_stats_t* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_gradient_plan_stats", kHostOnly);
    const auto it = h->grad_plans.find(plan_id);
    if (it == h->grad_plans.end()) return QSV_E_ARG;
    *out = it->second.stats;
    return QSV_OK;
}

int qsv_observables_create(qsv_t* h, int n_observables, const int64_t* term_offsets, const uint64_t* x_mask, const uint64_t* z_mask,
                           const double* coeff_re, const double* coeff_im, int* out_set_id) {
    (void)coeff_im;  // <P_k> is real for every Pauli string: real(<O_m>) only needs the real parts (as qsv_set_operator)
    QSV_OPEN(h, "qsv_observables_create", kDevice);
    if (n_observables < 1 || uint32_t(n_observables) > kMaxObservables || !term_offsets || !out_set_id)
        return fail(h, QSV_E_ARG, "an observable set needs 1 .. 65536 observables, their term offsets and an output");
    const int64_t first = term_offsets[0], n_entries = term_offsets[n_observables] - first;
    if (first < 0) return fail(h, QSV_E_ARG, "term offsets must not be negative");
    for (int m = 0; m < n_observables; ++m)
        if (term_offsets[m + 1] < term_offsets[m]) return fail(h, QSV_E_ARG, "term offsets must be non-decreasing");
    if (n_entries > kMaxObsEntries) return fail(h, QSV_E_ARG, "an observable set holds at most 2^24 terms");
    if (n_entries > 0 && (!x_mask || !z_mask || !coeff_re)) return fail(h, QSV_E_ARG, "term arrays are null");
    const uint64_t limit = h->n >= 64 ? ~uint64_t(0) : (uint64_t(1) << h->n) - 1;
    for (int64_t k = first; k < first + n_entries; ++k)
        if ((x_mask[k] | z_mask[k]) & ~limit) return fail(h, QSV_E_ARG, "Pauli term acts on a qubit >= n_qubits");
    // the distinct strings, ordered by (x, z): the diagonal group first, then the groups by x mask
    std::vector<std::pair<uint64_t, uint64_t>> strings;
    strings.reserve(size_t(n_entries));
    for (int64_t k = first; k < first + n_entries; ++k) strings.emplace_back(x_mask[k], z_mask[k]);
    std::sort(strings.begin(), strings.end());
    strings.erase(std::unique(strings.begin(), strings.end()), strings.end());
    if (strings.size() > kMaxObsStrings) return fail(h, QSV_E_ARG, "an observable set holds at most 65536 distinct Pauli strings");
    const uint32_t T = uint32_t(strings.size());
    std::vector<ObsTerm> terms(T);
    std::vector<FactorTerm> split_terms(T);
    std::vector<ObsRow> rows;
    for (uint32_t k = 0; k < T; ++k) {
        const uint64_t x = strings[k].first, z = strings[k].second;
        const uint32_t pivot = x ? uint32_t(63 - __builtin_clzll(x)) : 0u;
        const int ny = __builtin_popcountll(x & z);
        const uint64_t low = (uint64_t(1) << pivot) - 1;
        terms[k].zp = x ? ((z >> (pivot + 1)) << pivot) | (z & low) : z;
        terms[k].odd = uint32_t(ny & 1);
        terms[k].pad = 0;
        terms[k].scale = x ? (((ny >> 1) & 1) ? -2.0 : 2.0) : 1.0;  // (-1)^{floor(ny/2)}, both halves of each pair
        split_terms[k] = FactorTerm{uint32_t(x), uint32_t(z), 1.0};
        if (rows.empty() || rows.back().x != x || rows.back().count == kObsChunk) rows.push_back(ObsRow{x, k, 0, pivot, 0});
        rows.back().count += 1;
        rows.back().parts |= (ny & 1) ? 2u : 1u;
    }
    std::vector<int64_t> offsets(size_t(n_observables) + 1);
    std::vector<uint32_t> term_of(static_cast<size_t>(n_entries));
    std::vector<double> coef(static_cast<size_t>(n_entries));
    for (int m = 0; m <= n_observables; ++m) offsets[size_t(m)] = term_offsets[m] - first;
    for (int64_t k = 0; k < n_entries; ++k) {
        const auto at = std::lower_bound(strings.begin(), strings.end(), std::make_pair(x_mask[first + k], z_mask[first + k]));
        term_of[size_t(k)] = uint32_t(at - strings.begin());
        coef[size_t(k)] = coeff_re[first + k];
    }
    ObservableSet s;
    s.n_obs = uint32_t(n_observables);
    s.n_terms = T;
    s.n_rows = int(rows.size());
    // workgroups (one wave each) per row and state: up to 2048 per state in all, each sweeping at least four blocks of the
    // diagonal group -- a function of the set and the register only, so that the partial sums of a string are laid out, and
    // added, the same way in every batch (measured shapes: DESIGN 4.6)
    const uint64_t blocks = h->n > kObsBlockBits ? uint64_t(1) << (h->n - kObsBlockBits) : 1;
    s.nb = int(std::max<uint64_t>(1, std::min<uint64_t>(blocks / 4, 2048 / std::max<uint64_t>(1, rows.size()))));
    int rc;
    if ((rc = upload_bytes(h, s.d_rows, rows.data(), rows.size() * sizeof(ObsRow))) ||
        (rc = upload_bytes(h, s.d_terms, terms.data(), terms.size() * sizeof(ObsTerm))) ||
        (rc = upload_bytes(h, s.d_split_terms, split_terms.data(), split_terms.size() * sizeof(FactorTerm))) ||
        (rc = upload_bytes(h, s.d_offsets, offsets.data(), offsets.size() * sizeof(int64_t))) ||
        (rc = upload_bytes(h, s.d_term_of, term_of.data(), term_of.size() * sizeof(uint32_t))) ||
        (rc = upload_bytes(h, s.d_coef, coef.data(), coef.size() * sizeof(double)))) {
        free_observable_set(s);
        return rc;
    }
    if (uint32_t(n_observables) <= kCovMaxObservables) {  // qsv_observables_covariance's tables (covariance.hpp)
        std::vector<uint32_t> cov_first(size_t(n_observables) + 1, 0);
        std::vector<PauliGroup> cov_groups;
        std::vector<CovTerm> cov_terms;
        std::vector<int64_t> order;
        for (int m = 0; m < n_observables; ++m) {
            order.clear();
            for (int64_t k = term_offsets[m]; k < term_offsets[m + 1]; ++k) order.push_back(k);
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return x_mask[a] < x_mask[b]; });
            bool any = false;
            for (int64_t k : order) {
                const uint64_t x = x_mask[k];
                if (!any || cov_groups.back().x != x) {
                    PauliGroup g{};
                    g.x = x;
                    g.first = uint32_t(cov_terms.size());
                    g.pivot = x ? uint32_t(63 - __builtin_clzll(x)) : 0u;
                    cov_groups.push_back(g);
                    any = true;
                }
                cov_groups.back().count += 1;
                const int ny = __builtin_popcountll(x & z_mask[k]);
                const double c = ((ny >> 1) & 1) ? -coeff_re[k] : coeff_re[k];  // (-1)^{floor(ny/2)}
                cov_terms.push_back(CovTerm{z_mask[k] | ((ny & 1) ? kCovOddY : uint64_t(0)), c});
            }
            cov_first[size_t(m) + 1] = uint32_t(cov_groups.size());
        }
        if ((rc = upload_bytes(h, s.d_cov_first, cov_first.data(), cov_first.size() * sizeof(uint32_t))) ||
            (rc = upload_bytes(h, s.d_cov_groups, cov_groups.data(), cov_groups.size() * sizeof(PauliGroup))) ||
            (rc = upload_bytes(h, s.d_cov_terms, cov_terms.data(), cov_terms.size() * sizeof(CovTerm)))) {
            free_observable_set(s);
            return rc;
        }
    }
    const int id = h->next_obs_id++;
    h->obs_sets.emplace(id, std::move(s));
    *out_set_id = id;
    return QSV_OK;
}

int qsv_observables_destroy(qsv_t* h, int set_id) {
    QSV_OPEN(h, "qsv_observables_destroy", kDevice);
    auto it = h->obs_sets.find(set_id);
    if (it == h->obs_sets.end()) return fail(h, QSV_E_ARG, "unknown observable set " + std::to_string(set_id));
    QSV_HIP(h, sync_streams(h));
    free_observable_set(it->second);
    h->obs_sets.erase(it);
    return QSV_OK;
}

int qsv_eval_observables(qsv_t* h, int set_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                         double* out) {
    QSV_OPEN(h, "qsv_eval_observables", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out))) return fail(h, QSV_E_ARG, "bad arguments");
    auto set = h->obs_sets.find(set_id);
    if (set == h->obs_sets.end()) return fail(h, QSV_E_ARG, "unknown observable set " + std::to_string(set_id));
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args);
    if (rc || n_evals == 0) return rc;
    return eval_observables_locked(h, set->second, args, out);
}

// ---- an observable set's second moments (qsv.h: COVARIANCES; covariance.hpp) -----------------------------------------------------

int qsv_observables_covariance(qsv_t* h, int set_id, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                               double* out_values, double* out_cov) {
    QSV_OPEN(h, "qsv_observables_covariance", kDevice);
    if (n_evals < 0 || (n_evals > 0 && (!circuit_ids || !param_offsets || !out_cov))) return fail(h, QSV_E_ARG, "bad arguments");
    const auto found = h->obs_sets.find(set_id);
    if (found == h->obs_sets.end()) return fail(h, QSV_E_ARG, "unknown observable set " + std::to_string(set_id));
    const ObservableSet& set = found->second;
    if (set.n_obs > kCovMaxObservables) return fail(h, QSV_E_UNSUPPORTED, "covariances are available for sets of up to 64 observables");
    if (n_evals == 0) return QSV_OK;
    if (const int rc = qubit_guard(h, "covariances are available up to 28 qubits")) return rc;
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args,
                           "the covariances of a circuit on a kept state are not built");
    if (rc) return rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers below may still be read or written by a call that did not wait)
    // (a launch group's partials stay within the scratch limit of qsv_eval_observables)
    const size_t n = size_t(n_evals), M = set.n_obs;
    const size_t per_eval = size_t(covariance_pairs(set.n_obs)) * covariance_blocks(h->n, set.n_obs) * kCovPartial * sizeof(double);
    const size_t G = std::max<size_t>(1, std::min({size_t(h->group), size_t(h->max_grid_y), size_t(65535), kObsScratchBytes / per_eval}));
    // device scratch: the call's values by position | its covariances by position | the partials of one launch group
    const size_t out_count = n * (M + M * M), out_bytes = (out_count * sizeof(double) + 63) / 64 * 64;
    if ((rc = ensure(h, h->d_cov, out_bytes + std::min(G, n) * per_eval)) || (rc = ensure_host_out(h, out_count))) return rc;
    double* const values = static_cast<double*>(h->d_cov.ptr);
    double* const cov = values + n * M;
    double* const partials = reinterpret_cast<double*>(static_cast<char*>(h->d_cov.ptr) + out_bytes);
    auto moments = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_covariance_panels(h->dtype, h->d_states.ptr, h->n, int(gc), set.n_obs, static_cast<const uint32_t*>(set.d_cov_first.ptr),
                                            static_cast<const PauliGroup*>(set.d_cov_groups.ptr),
                                            static_cast<const CovTerm*>(set.d_cov_terms.ptr), partials, h->stream));
        QSV_HIP(h, launch_covariance_combine(partials, h->n, int(gc), set.n_obs, values + g0 * M, cov + g0 * M * M, h->stream));
        return QSV_OK;
    };
    if ((rc = run_whole_states(h, args, G, moments, values, out_count))) return rc;
    const double* const h_cov = h->h_out + n * M;
    for (size_t j = 0; j < n; ++j) {
        const size_t e = h->batch.eval_at[j];
        if (out_values) std::copy(h->h_out + j * M, h->h_out + (j + 1) * M, out_values + e * M);
        std::copy(h_cov + j * M * M, h_cov + (j + 1) * M * M, out_cov + e * M * M);
    }
    return QSV_OK;
}

// ---- overlaps and operator matrix elements against kept states (qsv.h: OVERLAPS; overlap.hpp) -------------------------------------

int qsv_overlap_circuits(qsv_t* h, int n_states, const int* prefix_ids, int with_operator, int n_evals, const int* circuit_ids,
                         const int64_t* param_offsets, const double* params, double* out_overlaps, double* out_elements) {
    QSV_OPEN(h, "qsv_overlap_circuits", kDevice);
    if (n_states < 1) return fail(h, QSV_E_ARG, "n_states must be at least 1");
    if (n_states > int(kOvlMaxStates)) return fail(h, QSV_E_UNSUPPORTED, "n_states: overlaps are available against up to 64 kept states per call");
    if (!prefix_ids) return fail(h, QSV_E_ARG, "prefix_ids is null");
    if (n_evals < 0) return fail(h, QSV_E_ARG, "n_evals is negative");
    if (n_evals > 0 && (!circuit_ids || !param_offsets)) return fail(h, QSV_E_ARG, "circuit_ids or param_offsets is null");
    if (n_evals > 0 && !out_overlaps) return fail(h, QSV_E_ARG, "out_overlaps is null");
    if (n_evals > 0 && with_operator && !out_elements) return fail(h, QSV_E_ARG, "out_elements is null (required with with_operator)");
    // (the register's size is the handle's own: asked before the kept states, which such a handle need not hold)
    if (n_evals > 0)
        if (const int rc = qubit_guard(h, "overlaps are available up to 28 qubits", true)) return rc;
    const size_t K = size_t(n_states);
    OverlapRefs refs{};
    int rc = kept_refs(h, n_states, prefix_ids, refs);
    if (rc || n_evals == 0) return rc;
    if (with_operator && h->n_terms == 0) return fail(h, QSV_E_STATE, "with_operator: no operator set (call qsv_set_operator first)");
    BatchArgs args;
    if ((rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args, "circuit_ids: the overlaps of a circuit on a kept state are not built")))
        return rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers below may still be read or written by a call that did not wait)
    const size_t n = size_t(n_evals);
    const bool op = with_operator != 0;
    const size_t G = overlap_group(h->n, K, op, std::max<size_t>(1, std::min(size_t(h->group), size_t(h->max_grid_y))));
    // device scratch: the call's S by position | its T by position | the partial tiles of one launch group
    const size_t tile_count = n * K * 2, out_count = op ? 2 * tile_count : tile_count, out_bytes = (out_count * sizeof(double) + 63) / 64 * 64;
    if ((rc = ensure(h, h->d_overlap, out_bytes + overlap_partial_bytes(h->n, K, op, std::min(G, n)))) || (rc = ensure_host_out(h, out_count)))
        return rc;
    double* const d_s = static_cast<double*>(h->d_overlap.ptr);
    double* const d_t = op ? d_s + tile_count : nullptr;
    double* const partials = reinterpret_cast<double*>(static_cast<char*>(h->d_overlap.ptr) + out_bytes);
    auto tiles = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_overlap_panels(h->dtype, h->d_states.ptr, h->d_prefix.ptr, refs, uint32_t(K), h->n, int(gc),
                                         op ? operator_view(h) : kNoOperator, partials, h->stream));
        QSV_HIP(h, launch_overlap_combine(partials, h->n, int(gc), uint32_t(K), d_s + g0 * K * 2, op ? d_t + g0 * K * 2 : nullptr, h->stream));
        return QSV_OK;
    };
    if ((rc = run_whole_states(h, args, G, tiles, d_s, out_count))) return rc;
    const size_t row = K * 2;
    for (size_t j = 0; j < n; ++j) {
        const size_t e = h->batch.eval_at[j];
        std::copy(h->h_out + j * row, h->h_out + (j + 1) * row, out_overlaps + e * row);
        if (op) std::copy(h->h_out + tile_count + j * row, h->h_out + tile_count + (j + 1) * row, out_elements + e * row);
    }
    return QSV_OK;
}

// ---- reduced density matrices of qubit subsets (qsv.h: REDUCED DENSITY MATRICES; reduced_density.hpp) ----------------------------

// What qsv_reduced_density_circuits and qsv_operator_density_circuits check alike before anything is built: the pointers, the
// register's size and the subsets (`what`: whose matrices, for the messages).  Fills the subset table and R, the doubles of an
// evaluation's row of the output.
static int rdm_open_subsets(qsv_t* h, const std::string& what, int n_subsets, const int32_t* subset_offsets, const int32_t* subset_qubits,
                            int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* out,
                            std::vector<RdmSubset>& table, size_t& R) {
    if (n_subsets < 1) return fail(h, QSV_E_ARG, "n_subsets must be at least 1");
    if (n_subsets > int(kRdmMaxSubsets)) return fail(h, QSV_E_UNSUPPORTED, "n_subsets: " + what + " are available for up to 1024 subsets per call");
    if (!subset_offsets || !subset_qubits) return fail(h, QSV_E_ARG, "subset_offsets or subset_qubits is null");
    if (n_evals < 0) return fail(h, QSV_E_ARG, "n_evals is negative");
    if (n_evals > 0 && (!circuit_ids || !param_offsets)) return fail(h, QSV_E_ARG, "circuit_ids or param_offsets is null");
    if (n_evals > 0 && !out) return fail(h, QSV_E_ARG, "out is null");
    // (the register's size is asked before anything is built or uploaded)
    if (const int rc = qubit_guard(h, (what + " are available up to 28 qubits").c_str(), true)) return rc;
    const size_t S = size_t(n_subsets);
    table.assign(S, RdmSubset{});
    R = 0;
    for (size_t s = 0; s < S; ++s) {
        const int64_t k = int64_t(subset_offsets[s + 1]) - int64_t(subset_offsets[s]);
        const std::string name = "subset " + std::to_string(s);
        if (subset_offsets[s] < 0 || k < 0) return fail(h, QSV_E_ARG, "subset_offsets must start at or above 0 and not fall (" + name + ")");
        if (k == 0) return fail(h, QSV_E_ARG, name + " is empty");
        if (k > int64_t(kRdmMaxQubits)) return fail(h, QSV_E_UNSUPPORTED, name + " has " + std::to_string(k) + " qubits: " + what + " are available for up to 4");
        const int32_t* q = subset_qubits + subset_offsets[s];
        for (int64_t j = 0; j < k; ++j) {
            if (q[j] < 0 || q[j] >= h->n) return fail(h, QSV_E_ARG, name + ": qubit " + std::to_string(q[j]) + " is out of range");
            for (int64_t i = 0; i < j; ++i)
                if (q[i] == q[j]) return fail(h, QSV_E_ARG, name + " names qubit " + std::to_string(q[j]) + " twice");
        }
        rdm_subset(h->n, q, uint32_t(k), uint32_t(R), table[s]);
        R += size_t(2) << (2 * k);
    }
    return QSV_OK;
}

int qsv_reduced_density_circuits(qsv_t* h, int n_subsets, const int32_t* subset_offsets, const int32_t* subset_qubits, int n_evals,
                                 const int* circuit_ids, const int64_t* param_offsets, const double* params, double* out) {
    QSV_OPEN(h, "qsv_reduced_density_circuits", kDevice);
    std::vector<RdmSubset> table;
    size_t R = 0;  // doubles of an evaluation's row of the output
    if (const int rc = rdm_open_subsets(h, "reduced density matrices", n_subsets, subset_offsets, subset_qubits, n_evals, circuit_ids, param_offsets, out, table, R))
        return rc;
    const size_t S = size_t(n_subsets);
    if (n_evals == 0) return QSV_OK;
    BatchArgs args;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args,
                           "circuit_ids: the reduced density matrices of a circuit on a kept state are not built");
    if (rc) return rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers below may still be read or written by a call that did not wait)
    const size_t n = size_t(n_evals);
    const size_t G = rdm_group(h->n, std::max<size_t>(1, std::min(size_t(h->group), size_t(h->max_grid_y))));
    // device scratch: the subset table | the call's matrices by position | the partial tiles of one launch
    const size_t table_bytes = S * sizeof(RdmSubset), out_count = n * R, out_bytes = (out_count * sizeof(double) + 63) / 64 * 64;
    const size_t most = std::min(G, n), run = std::min(S, rdm_subset_run(h->n, most));
    const size_t partial_bytes = most * run * rdm_blocks(h->n) * kRdmPartial * sizeof(double);
    if ((rc = ensure(h, h->d_rdm, table_bytes + out_bytes + partial_bytes)) || (rc = ensure_host_out(h, out_count))) return rc;
    const RdmSubset* const d_table = static_cast<const RdmSubset*>(h->d_rdm.ptr);
    double* const d_out = reinterpret_cast<double*>(static_cast<char*>(h->d_rdm.ptr) + table_bytes);
    double* const partials = reinterpret_cast<double*>(static_cast<char*>(h->d_rdm.ptr) + table_bytes + out_bytes);
    QSV_HIP(h, hipMemcpy(h->d_rdm.ptr, table.data(), table_bytes, hipMemcpyHostToDevice));
    auto tiles = [&](size_t g0, size_t gc) -> int {
        for (size_t s0 = 0; s0 < S; s0 += run) {
            const uint32_t sc = uint32_t(std::min(run, S - s0));
            QSV_HIP(h, launch_rdm_panels(h->dtype, h->d_states.ptr, h->n, int(gc), d_table + s0, sc, partials, h->stream));
            QSV_HIP(h, launch_rdm_combine(partials, h->n, int(gc), d_table + s0, sc, R, d_out + g0 * R, h->stream));
        }
        return QSV_OK;
    };
    if ((rc = run_whole_states(h, args, G, tiles, d_out, out_count))) return rc;
    for (size_t j = 0; j < n; ++j) std::copy(h->h_out + j * R, h->h_out + (j + 1) * R, out + size_t(h->batch.eval_at[j]) * R);
    return QSV_OK;
}

// ---- operator-weighted reduced density matrices (qsv.h: OPERATOR DENSITY MATRICES; operator_density.hpp) --------------------------

int qsv_operator_density_circuits(qsv_t* h, int n_subsets, const int32_t* subset_offsets, const int32_t* subset_qubits, int n_evals,
                                  const int* circuit_ids, const int64_t* param_offsets, const double* params, double* out,
                                  double* out_values) {
    QSV_OPEN(h, "qsv_operator_density_circuits", kDevice);
    std::vector<RdmSubset> table;
    size_t R = 0;  // doubles of an evaluation's row of the output
    int rc = rdm_open_subsets(h, "operator density matrices", n_subsets, subset_offsets, subset_qubits, n_evals, circuit_ids, param_offsets, out, table, R);
    if (rc || n_evals == 0) return rc;
    if (h->n_terms == 0) return fail(h, QSV_E_STATE, "no operator set (call qsv_set_operator first)");
    BatchArgs args;
    if ((rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, args,
                            "circuit_ids: the operator density matrices of a circuit on a kept state are not built")))
        return rc;
    if ((rc = wait_pending(h))) return rc;  // (the buffers below may still be read or written by a call that did not wait)
    const size_t S = size_t(n_subsets), n = size_t(n_evals);
    const size_t G = rdm_group(h->n, std::max<size_t>(1, std::min(size_t(h->group), size_t(h->max_grid_y))));
    // device scratch: the subset table | the call's matrices by position | its values by position | the partial tiles of one launch
    const size_t table_bytes = S * sizeof(RdmSubset), out_count = n * R + n, out_bytes = (out_count * sizeof(double) + 63) / 64 * 64;
    const size_t most = std::min(G, n), run = std::min(S, rdm_subset_run(h->n, most));
    const size_t partial_bytes = most * run * rdm_blocks(h->n) * kOpdmPartial * sizeof(double);
    const uint32_t op_blocks = adjoint_op_blocks(h->n);
    // (lambda and the operator's shares are the adjoint sweep's buffers, grown by need; qsv_adjoint_stats counts the sweep's own
    // allocations only)
    if ((rc = ensure(h, h->d_opdm, table_bytes + out_bytes + partial_bytes)) || (rc = ensure_host_out(h, out_count)) ||
        (rc = ensure(h, h->d_adj_lambda, (most << h->n) * h->amp_bytes)) || (rc = ensure(h, h->d_adj_epart, most * op_blocks * sizeof(double))))
        return rc;
    const RdmSubset* const d_table = static_cast<const RdmSubset*>(h->d_opdm.ptr);
    double* const d_out = reinterpret_cast<double*>(static_cast<char*>(h->d_opdm.ptr) + table_bytes);
    double* const d_values = d_out + n * R;
    double* const partials = reinterpret_cast<double*>(static_cast<char*>(h->d_opdm.ptr) + table_bytes + out_bytes);
    double* const e_partials = static_cast<double*>(h->d_adj_epart.ptr);
    QSV_HIP(h, hipMemcpy(h->d_opdm.ptr, table.data(), table_bytes, hipMemcpyHostToDevice));
    const bool streaming = h->stream_mode != 0;
    auto tiles = [&](size_t g0, size_t gc) -> int {
        QSV_HIP(h, launch_adjoint_apply_operator(h->dtype, h->d_states.ptr, h->d_adj_lambda.ptr, h->n, int(gc), operator_view(h), streaming,
                                                 e_partials, h->stream));
        QSV_HIP(h, launch_opdm_values(e_partials, op_blocks, int(gc), d_values + g0, h->stream));
        for (size_t s0 = 0; s0 < S; s0 += run) {
            const uint32_t sc = uint32_t(std::min(run, S - s0));
            QSV_HIP(h, launch_opdm_panels(h->dtype, h->d_states.ptr, h->d_adj_lambda.ptr, h->n, int(gc), d_table + s0, sc, partials, h->stream));
            QSV_HIP(h, launch_opdm_combine(partials, h->n, int(gc), d_table + s0, sc, R, d_out + g0 * R, h->stream));
        }
        return QSV_OK;
    };
    if ((rc = run_whole_states(h, args, G, tiles, d_out, out_count))) return rc;
    for (size_t j = 0; j < n; ++j) {
        const size_t e = h->batch.eval_at[j];
        std::copy(h->h_out + j * R, h->h_out + (j + 1) * R, out + e * R);
        if (out_values) out_values[e] = h->h_out[n * R + j];
    }
    return QSV_OK;
}

// ---- the Fubini-Study metric (qsv.h: FUBINI-STUDY METRIC; metric.hpp) --------------------------------------------------------------

int qsv_metric_circuits(qsv_t* h, int n_evals, const int* circuit_ids, const int64_t* param_offsets, const double* params,
                        const int64_t* wrt_offsets, const int32_t* wrt, int out_width, double* out) {
    QSV_OPEN(h, "qsv_metric_circuits", kDevice);
    if (n_evals < 0) return fail(h, QSV_E_ARG, "n_evals is negative");
    if (n_evals == 0) return QSV_OK;
    if (!circuit_ids || !param_offsets) return fail(h, QSV_E_ARG, "circuit_ids or param_offsets is null");
    if (!out) return fail(h, QSV_E_ARG, "out is null");
    if (out_width < 1) return fail(h, QSV_E_ARG, "out_width must be at least 1");
    // (the register's size is asked before anything is built or uploaded)
    if (const int rc = qubit_guard(h, "the metric is available up to 28 qubits", true)) return rc;
    BatchArgs packed;
    int rc = resolve_batch(h, size_t(n_evals), circuit_ids, param_offsets, params, packed, "circuit_ids: the metric of a circuit on a kept state is not built");
    if (rc) return rc;
    int64_t width, longest;
    std::vector<double> base;
    if ((rc = pack_rows(h, packed, wrt_offsets, out, true, width, longest, base))) return rc;
    const size_t n = size_t(n_evals), W = size_t(out_width);
    h->met_stats.n_columns = h->met_stats.n_run_launches = h->met_stats.n_gram_launches = 0;
    h->met_stats.run_ms = h->met_stats.gram_ms = 0.0;

    // ---- the tables: per distinct circuit the adjoint sweep's gates and runs of the WHOLE circuit and the slots that read each
    // parameter (adjoint_plan.hpp: sweep_tables_add); per evaluation its columns (the requested slots in the sweep's order) and
    // its entries
    SweepTables tables;
    std::vector<MetCol> cols;
    std::vector<MetEntry> entries;
    std::vector<uint32_t> entry_cols;
    std::vector<MetEval> by_eval(n);
    uint32_t max_gates = 0, max_cols = 0;
    for (size_t e = 0; e < n; ++e) {
        const Circuit& c = *packed.circs[e];
        WrtRequest asked;
        if ((rc = wrt_request(h, c, circuit_ids[e], e, wrt_offsets, wrt, out_width, "parameters", asked))) return rc;
        const int64_t first = asked.first, count = asked.count;
        const SweepCircuit* const found = sweep_tables_add(tables, &c, h->n, int(c.ops.size()), c.ops.data(), c.n_params);
        if (!found) return fail(h, QSV_E_ARG, "circuit " + std::to_string(circuit_ids[e]) + " cannot be planned for the adjoint sweep");
        const SweepCircuit& t = *found;
        // the columns: every slot that reads a requested parameter, once, in birth order (the sweep's: ascending 3 * gate + slot)
        std::vector<uint32_t> born;
        for (int64_t j = 0; j < count; ++j) {
            const std::vector<uint32_t>& r = t.readers[size_t(wrt_offsets ? int64_t(wrt[first + j]) : j)];
            born.insert(born.end(), r.begin(), r.end());
        }
        std::sort(born.begin(), born.end());
        born.erase(std::unique(born.begin(), born.end()), born.end());
        MetEval& ev = by_eval[e];
        ev = MetEval{t.gate_base, t.run_base, born.empty() ? 0u : t.n_runs, t.n_gates, uint32_t(e), uint32_t(cols.size()), uint32_t(born.size()),
                     uint32_t(entries.size()), uint32_t(count), 0};
        for (uint32_t s : born) cols.push_back(MetCol{s});
        // an entry's columns in ascending (gate, slot) order of the CIRCUIT: the sweep's gates backwards, a gate's slots forwards
        for (int64_t j = 0; j < count; ++j) {
            std::vector<uint32_t> r = t.readers[size_t(wrt_offsets ? int64_t(wrt[first + j]) : j)];
            std::sort(r.begin(), r.end(), [](uint32_t a, uint32_t b) { return a / 3 != b / 3 ? a / 3 > b / 3 : a < b; });
            entries.push_back(MetEntry{uint32_t(entry_cols.size()), uint32_t(r.size())});
            for (uint32_t s : r) entry_cols.push_back(uint32_t(std::lower_bound(born.begin(), born.end(), s) - born.begin()));
        }
        max_gates = std::max(max_gates, t.n_gates);
        max_cols = std::max(max_cols, uint32_t(born.size()));
        h->met_stats.n_columns += int64_t(born.size());
    }
    if (max_cols + 1 > 65535u) return fail(h, QSV_E_UNSUPPORTED, "the metric is available for up to 65534 columns per evaluation");

    // ---- the launch group: what the scratch bound leaves of the handle's
    const uint64_t dim = uint64_t(1) << h->n;
    const size_t stride = size_t(max_cols) + kMetricPsiBuffers, state_bytes = size_t(dim) * h->amp_bytes, eval_bytes = stride * state_bytes;
    const size_t bound = size_t(h->metric_scratch_mib) << 20;
    if (eval_bytes > bound) {
        const size_t fit = bound / state_bytes;
        return fail(h, QSV_E_UNSUPPORTED, "an evaluation of this call has " + std::to_string(max_cols) + " columns; \"metric_scratch_mib\" " +
                                              std::to_string(h->metric_scratch_mib) + " leaves room for " +
                                              std::to_string(fit > kMetricPsiBuffers ? fit - kMetricPsiBuffers : 0) + " at " + std::to_string(h->n) + " qubits");
    }
    const size_t G = std::max<size_t>(1, std::min({size_t(h->group), size_t(65535), bound / eval_bytes}));
    // the Gram kernel's partial tiles: so many evaluations per launch that they stay within 64 MiB (one always runs)
    const uint32_t max_pairs = metric_pairs(max_cols), gram_blocks = metric_gram_blocks(h->n);
    const size_t eval_partials = size_t(max_pairs) * gram_blocks * kMetTile * sizeof(double);
    const size_t gram_group = std::max<size_t>(1, std::min(G, (size_t(64) << 20) / eval_partials));

    int64_t& allocations = h->met_stats.n_allocations;
    BatchArgs args;
    if ((rc = rows_to_device(h, packed, base, width, h->d_met_base, allocations, args)) ||
        (rc = ensure_counted(h, h->d_met_out, n * W * W * sizeof(double), allocations)))
        return rc;

    // ---- the forward run's layout (ordinary plans into state slots, never split: as qsv_adjoint_gradient_circuits runs them)
    const StateRun run{SplitRule{}, 1, G, false, 0, kModeSynthFirst | kModeFinalStore};
    BatchRelease release{h};
    StateLayout lay;
    h->prof = qsv_profile{};
    if ((rc = lay_out_states(h, args, run, lay))) return rc;
    std::vector<MetEval> evals(n);
    std::vector<AdjEval> adj_evals(n);  // what launch_adjoint_prepare reads of an evaluation
    for (size_t j = 0; j < n; ++j) {
        evals[j] = by_eval[h->batch.eval_at[j]];
        adj_evals[j] = AdjEval{evals[j].gate_base, evals[j].run_base, evals[j].n_runs, evals[j].n_runs ? evals[j].n_gates : 0u, evals[j].row, 0};
    }
    // one blob: [gates][runs][evaluations][... as the adjoint sweep's][columns][entries][entry columns]
    TableBlob blob;
    const size_t off_gates = blob.add(tables.gates), off_runs = blob.add(tables.runs), off_evals = blob.add(evals), off_adj = blob.add(adj_evals),
                 off_cols = blob.add(cols), off_entries = blob.add(entries), off_ecols = blob.add(entry_cols);
    const size_t gc_max = std::min(G, n);
    // (lay_out_states has waited for whatever an earlier call without a wait left running: nothing reads the old tables)
    if ((rc = upload_blob(h, h->d_met_tab, blob, allocations)) || (rc = ensure_counted(h, h->d_met_scratch, gc_max * eval_bytes, allocations)) ||
        (rc = ensure_counted(h, h->d_met_mats, gc_max * std::max<size_t>(1, max_gates) * kAdjointMatDoubles * sizeof(double), allocations)) ||
        (rc = ensure_counted(h, h->d_met_partials, std::min(gram_group, gc_max) * eval_partials, allocations)))
        return rc;
    const void* dt = h->d_met_tab.ptr;
    const AdjGate* d_gates = TableBlob::at<AdjGate>(dt, off_gates);
    const AdjRunDesc* d_runs = TableBlob::at<AdjRunDesc>(dt, off_runs);
    const MetEval* d_evals = TableBlob::at<MetEval>(dt, off_evals);
    const AdjEval* d_adj = TableBlob::at<AdjEval>(dt, off_adj);
    const MetCol* d_cols = TableBlob::at<MetCol>(dt, off_cols);
    const MetEntry* d_entries = TableBlob::at<MetEntry>(dt, off_entries);
    const uint32_t* d_ecols = TableBlob::at<uint32_t>(dt, off_ecols);
    double* mats = static_cast<double*>(h->d_met_mats.ptr);
    double* partials = static_cast<double*>(h->d_met_partials.ptr);
    double* d_out = static_cast<double*>(h->d_met_out.ptr);
    char* scratch = static_cast<char*>(h->d_met_scratch.ptr);
    const bool streaming = h->stream_mode != 0;
    // option "time_moments": the run launches and the Gram kernels of every group are spans of their own
    enum { kRunSpan, kGramSpan };
    SpanTimer timer;
    const bool timing = h->time_moments;
    auto sweep = [&](size_t g0, size_t gc) -> int {
        uint32_t most_runs = 0, group_cols = 0;
        for (size_t j = g0; j < g0 + gc; ++j) {
            most_runs = std::max(most_runs, evals[j].n_runs);
            group_cols = std::max(group_cols, evals[j].n_cols);
        }
        if (most_runs > 0) {
            QSV_HIP(h, launch_adjoint_prepare(d_adj + g0, int(gc), d_gates, max_gates, args.device_values, width, mats, h->stream));
            if (timing) QSV_HIP(h, timer.begin(h->stream, kRunSpan));
            for (uint32_t r = 0; r < most_runs; ++r) {
                QSV_HIP(h, launch_metric_run(h->dtype, h->d_states.ptr, scratch, stride, h->n, int(gc), group_cols, r, d_evals + g0, d_runs, d_gates,
                                             d_cols, mats, max_gates, streaming, h->stream));
                h->met_stats.n_run_launches += 1;
            }
            if (timing) {
                QSV_HIP(h, timer.end(h->stream));
                QSV_HIP(h, timer.begin(h->stream, kGramSpan));
            }
        }
        for (size_t c0 = 0; c0 < gc; c0 += gram_group) {
            const size_t cc = std::min(gram_group, gc - c0);
            if (most_runs > 0) {
                // (the pair numbering is the call's -- max_cols --, the grid too: pairs past an evaluation's own leave at once)
                QSV_HIP(h, launch_metric_gram(h->dtype, scratch + c0 * eval_bytes, stride, h->n, int(cc), max_cols, d_evals + g0 + c0, partials, h->stream));
                h->met_stats.n_gram_launches += 1;
            }
            QSV_HIP(h, launch_metric_combine(d_evals + g0 + c0, int(cc), d_entries, d_ecols, partials, max_pairs, gram_blocks, out_width, d_out, h->stream));
        }
        if (most_runs > 0 && timing) QSV_HIP(h, timer.end(h->stream));
        return QSV_OK;
    };
    rc = run_laid_out(h, args, run, lay, {}, sweep);
    if (rc) {
        (void)sync_streams(h);
        return rc;
    }
    QSV_HIP(h, hipMemcpyAsync(out, d_out, n * W * W * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    QSV_HIP(h, sync_streams(h));
    h->async_pending = false;
    QSV_HIP(h, timer.elapsed(kRunSpan, h->met_stats.run_ms));
    QSV_HIP(h, timer.elapsed(kGramSpan, h->met_stats.gram_ms));
    return QSV_OK;
}

int qsv_metric_stats(const qsv_t* h, qsv_metric_stats_t* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_metric_stats", kHostOnly);
    *out = h->met_stats;
    out->scratch_bytes = int64_t(h->d_met_scratch.bytes + h->d_met_tab.bytes + h->d_met_mats.bytes + h->d_met_partials.bytes + h->d_met_base.bytes +
                                 h->d_met_out.bytes);
    return QSV_OK;
}

int qsv_sample(qsv_t* h, int circuit_id, const double* params, int n_params, int shots, uint64_t seed,
               uint64_t* out_states) {
    QSV_OPEN(h, "qsv_sample", kDevice);
    if (shots < 0 || n_params < 0 || (shots > 0 && !out_states)) return fail(h, QSV_E_ARG, "bad arguments");
    const int64_t offsets[2] = {0, n_params};
    BatchArgs args;
    int rc = resolve_batch(h, 1, &circuit_id, offsets, params, args, shots ? kNotSampled : nullptr);
    return rc ? rc : sample_batch_locked(h, args, shots, seed, out_states, nullptr);
}

int qsv_fitness_table_wait(const volatile uint64_t* own, int count, volatile int64_t* done, int stride, int world, int rank,
                           int64_t step, int budget_us) {
    if (!own || !done || count < 0 || world < 1 || rank < 0 || rank >= world || stride < 1) return QSV_E_ARG;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(budget_us);
    auto expired = [&](unsigned& spins) {
        __builtin_ia32_pause();
        return (++spins & 255u) == 0 && std::chrono::steady_clock::now() > deadline;
    };
    unsigned spins = 0;
    for (int i = 0; i < count;) {  // (values arrive in any order: every word is looked at until it is no sentinel)
        if (own[i] != QSV_TABLE_SENTINEL)
            ++i;
        else if (expired(spins))
            return 1;
    }
    // (the values were seen by this core before the counter is published: whoever sees the counter sees them)
    __atomic_store_n(&done[size_t(rank) * size_t(stride)], step, __ATOMIC_RELEASE);
    for (int r = 0; r < world;) {
        if (__atomic_load_n(&done[size_t(r) * size_t(stride)], __ATOMIC_ACQUIRE) >= step)
            ++r;
        else if (expired(spins))
            return 2;
    }
    return 0;
}

int qsv_set_option(qsv_t* h, const char* name, int value) {
    if (!h) return QSV_E_ARG;
    if (!name) return fail(h, QSV_E_ARG, "option name is null");
    QSV_OPEN(h, "qsv_set_option", kHostOnly);
    h->epoch += 1;
    const std::string key(name);
    if (key == "split") {
        if (value != 0 && !h->d_side.ptr && h->n > h->geo.k && h->n <= 28)
            return fail(h, QSV_E_ARG, "this handle was created without side tables (QSV_SPLIT=0): splitting cannot be switched on");
        h->split_enabled = value != 0;
    } else if (key == "factor") {
        if (value != 0 && h->split_enabled && h->d_side.ptr && !h->d_factor.ptr)
            return fail(h, QSV_E_ARG, "this handle was created without the factorised path (QSV_FACTOR=0)");
        h->factor_enabled = value != 0;
    } else if (key == "fused_factor") {
        h->fused_factor = value != 0;
    } else if (key == "chain_stream") {
        h->chain_enabled = value != 0;
    } else if (key == "poll_results") {
        h->poll_results = value != 0;
    } else if (key == "repeat_layout") {
        h->repeat_enabled = value != 0;
    } else if (key == "replay_launches") {  // a repeated whole-push batch queues its recorded launches again (the same launches, the same bits)
        h->replay_enabled = value != 0;
    } else if (key == "split_max_keys") {
        if (value < 0 || value > kMaxSplitKeys) return fail(h, QSV_E_ARG, "split_max_keys must be between 0 and 5");
        h->split_max_keys = value;
    } else if (key == "split_sampling") {
        h->split_sampling = value != 0;
    } else if (key == "fused_lds_table") {  // one-launch route: sides' states handed to their Gram matrices through LDS (same bits either way)
        h->fused_lds_table = value != 0;
    } else if (key == "side_prepare") {  // one-launch route: a side prepared from one staged read of its plan (same bits either way).  The next launch.
        h->side_prepare = value != 0;
    } else if (key == "final_controls") {  // one-launch route: no key qubit for a final control's key on the control's side.  Circuits registered afterwards.
        h->final_controls = value != 0;
        h->epoch += 1;  // (a batch that repeats must be laid out again: which form it runs is decided there)
    } else if (key == "live_entries") {  // one-launch route: three-key evaluations with a reduced side hand off live entries only (same bits either way)
        // (a launch's mode carries it: the epoch moved above, so a recorded launch is dropped and the next push lays its launches out anew)
        h->live_entries = value != 0;
    } else if (key == "sides_r3") {  // one-launch route: sides with eight amplitudes per thread, three-key sides on two workgroups.  Circuits registered afterwards.
        h->sides_r3 = value != 0;
    } else if (key == "side_diag") {  // one-launch route: a side's values of D from a table of its own (one run) instead of gathered from D
        // (same values either way; the plans name the tables: everything is uploaded again when it is next used)
        if (h->side_diag != (value != 0)) {
            QSV_HIP(h, sync_streams(h));
            for (auto& kv : h->circuits) kv.second.uploaded = false;
            h->sdiag_used = 0;
        }
        h->side_diag = value != 0;
    } else if (key == "streams") {
        if (value < 1 || value > h->n_lane_streams + 1) return fail(h, QSV_E_ARG, "streams must be between 1 and the number the handle was created with");
        h->n_streams = value;
    } else if (key == "max_grid_y") {  // x-mask groups / observable rows per launch (0: the device's largest gridDim.y); the same bits at any value
        if (value < 0 || value > h->device_max_grid_y) return fail(h, QSV_E_ARG, "max_grid_y must be between 0 and the device's largest gridDim.y");
        h->max_grid_y = value ? value : h->device_max_grid_y;
    } else if (key == "gradient_chunk") {  // shifted evaluations per chunk of a gradient call (0: the default); the same bits at any value
        if (value < 0 || value > (1 << 20)) return fail(h, QSV_E_ARG, "gradient_chunk must be between 0 and 1048576");
        h->grad_chunk = value ? value : kGradientChunkRows;
    } else if (key == "time_moments") {  // qsv_variance_circuits brackets its two kernels by events: qsv_get_profile's expect_ms (the same bits)
        h->time_moments = value != 0;
    } else if (key == "metric_scratch_mib") {  // the bound of qsv_metric_circuits' scratch of derivative states; the same bits at any value
        if (value < 1 || value > (1 << 20)) return fail(h, QSV_E_ARG, "metric_scratch_mib must be between 1 and 1048576");
        h->metric_scratch_mib = value;
    } else {
        return fail(h, QSV_E_ARG, "unknown option '" + key + "'");
    }
    return QSV_OK;
}

int qsv_set_profiling(qsv_t* h, int enabled) {
    QSV_OPEN(h, "qsv_set_profiling", kHostOnly);
    h->epoch += 1;
    h->profiling = enabled != 0;
    return QSV_OK;
}

int qsv_live_entries(int n_keys, unsigned key_mask, int* out_pi) {
    if (n_keys != 3 || key_mask > 7u || !out_pi) return QSV_E_ARG;
    for (int i = 0; i < 64; ++i) out_pi[i] = -1;
    int count = 0;
    for (uint32_t pi = 0; pi < 64; ++pi) {
        uint32_t rank = 0;
        if (!live_entry(key_mask, pi, &rank)) continue;
        out_pi[rank] = int(pi);  // (the entry's place in the hand-off)
        ++count;
    }
    return count;
}

long long qsv_replayed_pushes(const qsv_t* h) {
    QSV_OPEN(h, "qsv_replayed_pushes", kHostOnly);
    return (long long)h->replayed_pushes;
}

int qsv_get_profile(const qsv_t* h, qsv_profile* out) {
    if (!out) return QSV_E_ARG;
    QSV_OPEN(h, "qsv_get_profile", kHostOnly);
    *out = h->prof;
    return QSV_OK;
}

static int bench_ops_locked(qsv_t* h, int n_ops, const qsv_op* ops, int reps, double* out_ms_per_rep,
                            int* out_n_passes) {
    if (!out_ms_per_rep || reps < 1) return fail(h, QSV_E_ARG, "bad arguments");
    int id = 0;
    // no folding: the gates must really be applied to the resident state
    int rc = register_circuit(h, n_ops, ops, 0, &id, /*fold=*/false);
    if (rc) return rc;
    Circuit& c = h->circuits.find(id)->second;
    auto cleanup = [&]() { h->circuits.erase(id); };
    std::vector<Circuit*> cc{&c};
    if ((rc = batch_layout(h, cc, std::vector<int64_t>{0})) || (rc = batch_ship(h, 0, 1, kNoValues))) {
        h->batch.circs.clear();
        cleanup();
        return rc;
    }
    h->batch.circs.clear();
    PassArgs a{};
    a.plan = static_cast<const uint32_t*>(h->d_arena.ptr);
    a.mats = static_cast<const double*>(h->d_mats.ptr);
    a.evals = batch_evals(h);
    a.states = h->d_states.ptr;
    a.wtab = h->d_wtab.ptr;
    a.wtab_stride = h->wtab_stride;
    a.state_stride = uint64_t(1) << h->n;
    a.mode = kModeFinalStore | h->stream_mode;  // read-modify-write of the resident state, no synthesis
    const unsigned chunks = chunks_per_state(h);
    a.tiles_per_block = (h->geo.blocks_per_state + chunks - 1) / chunks;
    dim3 grid(chunks, 1);
    const int n_passes = c.plan.stats.n_passes;
    auto sweep = [&]() -> hipError_t {
        for (int p = 0; p < n_passes; ++p) {
            a.pass_index = uint32_t(p);
            hipError_t e = launch_pass(h->dtype, h->geo.r, h->cfg.xmode, grid, h->geo.threads_launch, h->geo.lds_bytes, h->stream, a);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    hipEvent_t e0, e1;
    QSV_HIP(h, hipEventCreate(&e0));
    QSV_HIP(h, hipEventCreate(&e1));
    QSV_HIP(h, sweep());  // untimed: code object load, plan in cache
    QSV_HIP(h, hipEventRecord(e0, h->stream));
    for (int i = 0; i < reps; ++i) QSV_HIP(h, sweep());
    QSV_HIP(h, hipEventRecord(e1, h->stream));
    QSV_HIP(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    QSV_HIP(h, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *out_ms_per_rep = double(ms) / reps;
    if (out_n_passes) *out_n_passes = n_passes;
    cleanup();
    return QSV_OK;
}

int qsv_bench_ops(qsv_t* h, int n_ops, const qsv_op* ops, int reps, double* out_ms_per_rep, int* out_n_passes) {
    QSV_OPEN(h, "qsv_bench_ops", kDevice);
    for (int i = 0; i < n_ops; ++i)
        if (ops && ops[i].kind != QSV_OP_ID && (ops[i].p_theta >= 0 || ops[i].p_phi >= 0 || ops[i].p_lambda >= 0))
            return fail(h, QSV_E_ARG, "qsv_bench_ops needs bound (literal) angles");
    return bench_ops_locked(h, n_ops, ops, reps, out_ms_per_rep, out_n_passes);
}

int qsv_bench_gate(qsv_t* h, int target, int control, double theta, double phi, double lambda, int reps,
                   double* out_ms_per_sweep) {
    QSV_OPEN(h, "qsv_bench_gate", kDevice);
    if (target < 0 || target >= h->n || control >= h->n) return fail(h, QSV_E_ARG, "qubit out of range");
    qsv_op op{};
    op.kind = control >= 0 ? QSV_OP_CU3 : QSV_OP_U;
    op.target = uint8_t(target);
    op.control = control >= 0 ? uint8_t(control) : uint8_t(QSV_NO_CONTROL);
    op.p_theta = op.p_phi = op.p_lambda = -1;
    op.theta = theta;
    op.phi = phi;
    op.lambda = lambda;
    return bench_ops_locked(h, 1, &op, reps, out_ms_per_sweep, nullptr);
}

int qsv_split_describe(int n_qubits, int n_ops, const qsv_op* ops, int max_side, uint64_t* mask_a, qsv_op* ops_a,
                       int capacity_a, int* n_ops_a, qsv_op* ops_b, int capacity_b, int* n_ops_b) {
    if (!mask_a || !n_ops_a || !n_ops_b) return fail(nullptr, QSV_E_ARG, "null output") - 100;
    if (n_qubits < 1 || n_qubits > 32) return fail(nullptr, QSV_E_ARG, "n_qubits must be in [1, 32]") - 100;
    if (validate_ops(nullptr, n_qubits, n_ops, ops, 1 << 30)) return QSV_E_ARG - 100;
    std::vector<AngleSource> angles;
    const std::vector<GateIn> gates = gates_of(ops, n_ops, &angles);
    const SplitCircuits sc = find_split(n_qubits, gates, angles, max_side);
    if (!sc.ok) return -1;
    *mask_a = sc.mask[0];
    qsv_op* outs[2] = {ops_a, ops_b};
    const int caps[2] = {capacity_a, capacity_b};
    int* counts[2] = {n_ops_a, n_ops_b};
    for (int s = 0; s < 2; ++s) {
        *counts[s] = int(sc.gates[s].size());
        if (!outs[s] || caps[s] < *counts[s]) continue;
        for (size_t i = 0; i < sc.gates[s].size(); ++i) {
            const GateIn& g = sc.gates[s][i];
            const AngleSource& a = sc.angles[s][size_t(g.op)];
            qsv_op o{};
            o.kind = g.control < 0 ? QSV_OP_U : QSV_OP_CU3;
            o.target = uint8_t(g.target);
            o.control = g.control < 0 ? uint8_t(QSV_NO_CONTROL) : uint8_t(g.control);
            o.p_theta = a.p_theta; o.p_phi = a.p_phi; o.p_lambda = a.p_lambda;
            o.theta = a.theta; o.phi = a.phi; o.lambda = a.lambda;
            outs[s][i] = o;
        }
    }
    return sc.n_keys;
}

int qsv_split_describe_reduced(int n_qubits, int n_ops, const qsv_op* ops, int max_side, uint64_t* mask_a, qsv_op* ops_a,
                               int capacity_a, int* n_ops_a, qsv_op* ops_b, int capacity_b, int* n_ops_b,
                               uint32_t* simulated_keys, uint32_t* final_keys, int* key_bits, int* qubits) {
    if (!mask_a || !n_ops_a || !n_ops_b || !simulated_keys || !final_keys || !key_bits || !qubits)
        return fail(nullptr, QSV_E_ARG, "null output") - 100;
    if (n_qubits < 1 || n_qubits > 32) return fail(nullptr, QSV_E_ARG, "n_qubits must be in [1, 32]") - 100;
    if (validate_ops(nullptr, n_qubits, n_ops, ops, 1 << 30)) return QSV_E_ARG - 100;
    std::vector<AngleSource> angles;
    const std::vector<GateIn> gates = gates_of(ops, n_ops, &angles);
    const SplitCircuits sc = find_split(n_qubits, gates, angles, max_side);
    if (!sc.ok) return -1;
    const ReducedSplit rs = reduce_final_controls(sc);
    *mask_a = sc.mask[0];
    qsv_op* outs[2] = {ops_a, ops_b};
    const int caps[2] = {capacity_a, capacity_b};
    int* counts[2] = {n_ops_a, n_ops_b};
    for (int s = 0; s < 2; ++s) {
        simulated_keys[s] = rs.simulated_keys[s];
        final_keys[s] = rs.final_keys[s];
        for (int j = 0; j < QSV_SPLIT_MAX_KEYS; ++j) key_bits[s * QSV_SPLIT_MAX_KEYS + j] = j < kMaxSplitKeys ? rs.key_bit[s][j] : -1;
        // (the side's qubits in ascending order are the full form's local numbers)
        std::vector<int> global;
        for (int q = 0; q < n_qubits; ++q)
            if (sc.mask[s] >> q & 1u) global.push_back(q);
        for (int p = 0; p < 32; ++p) qubits[s * 32 + p] = p < sc.n_side[s] ? global[size_t(rs.qubit_of[s][size_t(p)])] : -1;
        *counts[s] = int(rs.gates[s].size());
        if (!outs[s] || caps[s] < *counts[s]) continue;
        for (size_t i = 0; i < rs.gates[s].size(); ++i) {
            const GateIn& g = rs.gates[s][i];
            const AngleSource& a = rs.angles[s][size_t(g.op)];
            qsv_op o{};
            o.kind = g.control < 0 ? QSV_OP_U : QSV_OP_CU3;
            o.target = uint8_t(g.target);
            o.control = g.control < 0 ? uint8_t(QSV_NO_CONTROL) : uint8_t(g.control);
            o.p_theta = a.p_theta; o.p_phi = a.p_phi; o.p_lambda = a.p_lambda;
            o.theta = a.theta; o.phi = a.phi; o.lambda = a.lambda;
            outs[s][i] = o;
        }
    }
    return sc.n_keys;
}

int qsv_plan_build(int n_qubits, int dtype, int n_ops, const qsv_op* ops, const qsv_plan_config* cfg,
                   uint32_t* out_words, size_t capacity_words, size_t* n_words) {
    if (!n_words) return fail(nullptr, QSV_E_ARG, "n_words is null");
    if (dtype != QSV_F64 && dtype != QSV_F32) return fail(nullptr, QSV_E_ARG, "bad dtype");
    if (n_qubits < 1 || n_qubits > 32) return fail(nullptr, QSV_E_ARG, "n_qubits must be in [1, 32]");
    int rc = validate_ops(nullptr, n_qubits, n_ops, ops, 1 << 30);
    if (rc) return rc;
    try {
        PlanConfig pc = resolve_config(cfg, dtype, n_qubits);
        std::vector<AngleSource> angles;
        std::vector<GateIn> gates = gates_of(ops, n_ops, &angles);
        CircuitPlan plan = build_plan(n_qubits, gates, angles, pc);
        *n_words = plan.words.size();
        if (out_words && capacity_words >= plan.words.size())
            std::memcpy(out_words, plan.words.data(), plan.words.size() * 4);
    } catch (const std::exception& e) {
        return fail(nullptr, QSV_E_ARG, e.what());
    }
    return QSV_OK;
}

}  // extern "C"
