// Device-resident value cache (qsv.h: qsv_value_cache_*, qsv_sample_lookup, qsv_sample_lookup_finish): an open-addressing
// hash table basis state -> double in device memory, and the four kernels around a host-side scoring function -- which sampled
// states are new, each state's value once the host has supplied it, the gather of a value per sample.
//
// Layout: `slots` (a power of two) keys and as many values, two arrays (a probe reads keys only).  An empty key is
// kCacheEmptyKey; state 0 is an ordinary key.  A state's home slot is splitmix64(state) & (slots - 1), collisions go to the
// next slot (linear probing).  Keys only ever change from empty to a state within a table's lifetime -- a clear or a growth is
// a kernel boundary --, and nothing is ever removed, so a probe that ends at an empty slot has seen every slot the state could
// be in.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace qsv {

constexpr uint64_t kCacheEmptyKey = ~uint64_t(0);

__host__ __device__ inline uint64_t cache_hash(uint64_t x) {  // splitmix64's finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// What a probe leaves behind besides the table: counters[0] = entries of the miss list, counters[1] = nonzero when some thread
// walked the whole table without finding its state or an empty slot (never with the host's growth rule; then the slot indices
// are not valid).  Both are zeroed by the caller on the stream ahead of the launch.
constexpr int kCacheCounterWords = 2;

// For every sample i < n_samples: find or insert states[i] and write its slot to sample_slot[i].  The thread whose insert
// created an entry appends (state, slot) to the miss list: miss_states (may be pinned host memory: written once, never
// read) and miss_slots, capacity n_samples each, in whatever order the atomics give.  The table must have at least one empty
// slot per sample beyond its entries.
hipError_t launch_cache_probe(const uint64_t* states, int64_t n_samples, uint64_t* keys, uint32_t log2_slots, uint32_t* sample_slot,
                              uint64_t* miss_states, uint32_t* miss_slots, uint32_t* counters, hipStream_t stream);

// Every entry of the old table (keys and values) into the new one, which must be all empty and have room; a failed walk
// sets counters[1].
hipError_t launch_cache_rehash(const uint64_t* old_keys, const double* old_vals, uint32_t old_log2_slots, uint64_t* keys, double* vals,
                               uint32_t log2_slots, uint32_t* counters, hipStream_t stream);

// vals[miss_slots[j]] = values[j] for j < n (values may be pinned host memory).
hipError_t launch_cache_fill(double* vals, const uint32_t* miss_slots, const double* values, int64_t n, hipStream_t stream);

// out[i] = vals[sample_slot[i]] for i < n_samples.
hipError_t launch_cache_gather(const double* vals, const uint32_t* sample_slot, int64_t n_samples, double* out, hipStream_t stream);

}  // namespace qsv
