// Device-resident value cache: the probe, rehash, fill and gather kernels (value_cache.hpp).
#include "value_cache.hpp"

namespace qsv {

namespace {

constexpr int kCacheThreads = 256;

// Walks from `state`'s home slot until it finds the state or claims an empty slot for it.  Returns the slot, or `slots` when
// the whole table was walked in vain; *won: this call created the entry.
//
// The key is read with a PLAIN load.  Other threads of the launch insert while this one reads, their compare-and-swaps are
// performed at the memory side, and neither this CU's L1 nor this XCD's L2 is refreshed by them, so the load can be stale --
// but only in one direction: a key changes once, from empty to a state, and the launch started with clean caches (a kernel
// boundary), so a stale line can show "empty" where a state now is and never anything else.  "Empty" is therefore only ever
// believed from the compare-and-swap's own answer (agent scope, the default of atomicCAS): the winner owns a new entry, a
// loser that reads back its own state has a hit, any other loser goes on.  A non-empty key the load shows is final.  An
// L1-bypassing load would buy nothing here (the other XCDs' inserts are not in this L2 either) and the warm case, where every
// sample is a hit and nobody writes, keeps its cache hits.
__device__ __forceinline__ uint64_t cache_find_or_claim(uint64_t* keys, uint64_t slots, uint64_t state, bool match, bool* won) {
    const uint64_t mask = slots - 1;
    uint64_t pos = cache_hash(state) & mask;
    for (uint64_t step = 0; step < slots; ++step) {  // (bounded: no table, however full, makes a thread spin)
        uint64_t k = keys[pos];
        if (k == kCacheEmptyKey) {
            k = atomicCAS(reinterpret_cast<unsigned long long*>(keys + pos), (unsigned long long)kCacheEmptyKey, (unsigned long long)state);
            if (k == kCacheEmptyKey) {
                *won = true;
                return pos;
            }
        }
        if (match && k == state) return pos;
        pos = (pos + 1) & mask;
    }
    return slots;
}

__global__ void __launch_bounds__(kCacheThreads)
cache_probe_kernel(const uint64_t* __restrict__ states, long long n_samples, uint64_t* keys, uint32_t log2_slots,
                   uint32_t* __restrict__ sample_slot, uint64_t* __restrict__ miss_states, uint32_t* __restrict__ miss_slots,
                   uint32_t* counters) {
    const long long i = (long long)blockIdx.x * kCacheThreads + threadIdx.x;
    const uint64_t slots = uint64_t(1) << log2_slots;
    bool won = false;
    uint64_t state = 0, pos = 0;
    if (i < n_samples) {  // (no early return: every lane of the wave takes part in the ballot below)
        state = states[i];
        pos = cache_find_or_claim(keys, slots, state, true, &won);
        if (pos == slots) {
            counters[1] = 1u;
            pos = 0;
        }
        sample_slot[i] = uint32_t(pos);
    }
    // the winners of a wave append together: one atomic per wave
    const unsigned long long winners = __ballot(won);
    if (winners == 0) return;
    const int lane = int(threadIdx.x & 63u);
    const int leader = __ffsll((long long)winners) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&counters[0], uint32_t(__popcll(winners)));
    base = uint32_t(__shfl(int(base), leader));
    if (won) {
        const uint32_t at = base + uint32_t(__popcll(winners & ((1ull << lane) - 1ull)));
        miss_states[at] = state;
        miss_slots[at] = uint32_t(pos);
    }
}

__global__ void __launch_bounds__(kCacheThreads)
cache_rehash_kernel(const uint64_t* __restrict__ old_keys, const double* __restrict__ old_vals, uint32_t old_log2_slots, uint64_t* keys,
                    double* __restrict__ vals, uint32_t log2_slots, uint32_t* counters) {
    const uint64_t i = uint64_t(blockIdx.x) * kCacheThreads + threadIdx.x;
    if (i >= (uint64_t(1) << old_log2_slots)) return;
    const uint64_t state = old_keys[i];
    if (state == kCacheEmptyKey) return;
    const uint64_t slots = uint64_t(1) << log2_slots;
    bool won = false;
    const uint64_t pos = cache_find_or_claim(keys, slots, state, false, &won);  // (the old table's keys are distinct: no match to look for)
    if (pos == slots) {
        counters[1] = 1u;
        return;
    }
    vals[pos] = old_vals[i];
}

__global__ void __launch_bounds__(kCacheThreads)
cache_fill_kernel(double* __restrict__ vals, const uint32_t* __restrict__ miss_slots, const double* __restrict__ values, long long n) {
    const long long j = (long long)blockIdx.x * kCacheThreads + threadIdx.x;
    if (j < n) vals[miss_slots[j]] = values[j];
}

__global__ void __launch_bounds__(kCacheThreads)
cache_gather_kernel(const double* __restrict__ vals, const uint32_t* __restrict__ sample_slot, long long n_samples, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kCacheThreads + threadIdx.x;
    if (i < n_samples) out[i] = vals[sample_slot[i]];
}

inline unsigned cache_blocks(uint64_t n) { return unsigned((n + kCacheThreads - 1) / kCacheThreads); }

}  // namespace

hipError_t launch_cache_probe(const uint64_t* states, int64_t n_samples, uint64_t* keys, uint32_t log2_slots, uint32_t* sample_slot,
                              uint64_t* miss_states, uint32_t* miss_slots, uint32_t* counters, hipStream_t stream) {
    if (n_samples <= 0) return hipSuccess;
    if (log2_slots > 31 || n_samples > (int64_t(1) << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cache_probe_kernel, dim3(cache_blocks(uint64_t(n_samples))), dim3(kCacheThreads), 0, stream, states,
                       (long long)n_samples, keys, log2_slots, sample_slot, miss_states, miss_slots, counters);
    return hipGetLastError();
}

hipError_t launch_cache_rehash(const uint64_t* old_keys, const double* old_vals, uint32_t old_log2_slots, uint64_t* keys, double* vals,
                               uint32_t log2_slots, uint32_t* counters, hipStream_t stream) {
    if (old_log2_slots > 31 || log2_slots > 31) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cache_rehash_kernel, dim3(cache_blocks(uint64_t(1) << old_log2_slots)), dim3(kCacheThreads), 0, stream, old_keys,
                       old_vals, old_log2_slots, keys, vals, log2_slots, counters);
    return hipGetLastError();
}

hipError_t launch_cache_fill(double* vals, const uint32_t* miss_slots, const double* values, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cache_fill_kernel, dim3(cache_blocks(uint64_t(n))), dim3(kCacheThreads), 0, stream, vals, miss_slots, values,
                       (long long)n);
    return hipGetLastError();
}

hipError_t launch_cache_gather(const double* vals, const uint32_t* sample_slot, int64_t n_samples, double* out, hipStream_t stream) {
    if (n_samples <= 0) return hipSuccess;
    hipLaunchKernelGGL(cache_gather_kernel, dim3(cache_blocks(uint64_t(n_samples))), dim3(kCacheThreads), 0, stream, vals, sample_slot,
                       (long long)n_samples, out);
    return hipGetLastError();
}

}  // namespace qsv
