// Exact CVaR gradients (cvar_gradient.hpp): the threshold search from amplitudes, the clipped seed and the
// finishing kernel.  Every sum is fp64 and is formed in a fixed order -- per thread over its ranks or amplitudes in ascending
// order, across a wave by a butterfly, across waves, threads and chunks in index order --, so an evaluation's threshold, seed and
// value depend on nothing but its state, the operator and alpha.  No floating-point atomics.
#include "cvar_gradient.hpp"

namespace qsv {

namespace {

template <typename real>
struct alignas(2 * sizeof(real)) gcx {  // (one access per amplitude)
    real re, im;
};

template <typename real>
__device__ __forceinline__ gcx<real> load_amp(const gcx<real>* p) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = *reinterpret_cast<const vec2*>(p);
    return gcx<real>{v.x, v.y};
}
template <typename real>
__device__ __forceinline__ void store_amp(gcx<real>* p, gcx<real> a, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    vec2 v;
    v.x = a.re;
    v.y = a.im;
    if (streaming)
        __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
    else
        *reinterpret_cast<vec2*>(p) = v;
}
template <typename real>
__device__ __forceinline__ double probability(gcx<real> a) {
    const double re = double(a.re), im = double(a.im);
    return fma(re, re, im * im);
}

constexpr uint32_t kThreads = 256;
constexpr uint32_t kOwn = kCvarChunk / kThreads;  // ranks of a chunk per thread
static_assert(kThreads == uint32_t(kAdjointThreads), "the seed's shares have launch_adjoint_apply_operator's layout");

// every lane receives the sum of the wave's 64 values, added in the butterfly's order
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double block_sum(double v, double* red) {  // red: one double per wave of the 256 threads
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// sh[i] <- sh[0] + .. + sh[i - 1], by thread 0 in index order; returns the total to every thread.  The values are seen by all
// threads after the call.
__device__ double exclusive_scan_256(double* sh, double* total) {
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (uint32_t i = 0; i < kThreads; ++i) {
            const double v = sh[i];
            sh[i] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    return *total;
}

// chunk c of evaluation e: the mass of ranks [c kCvarChunk, (c + 1) kCvarChunk), every thread its strided share in ascending
// order, then the fixed-order block sum.  grid: (chunks, evaluations)
template <typename real>
__global__ void __launch_bounds__(kThreads)
cvar_gradient_chunks_kernel(const gcx<real>* __restrict__ states, unsigned long long dim, const uint32_t* __restrict__ order,
                            uint32_t n_chunks, double* __restrict__ chunk_mass) {
    __shared__ double red[4];
    const uint32_t pos = blockIdx.y;
    const gcx<real>* st = states + size_t(pos) * dim;
    const unsigned long long base = (unsigned long long)blockIdx.x * kCvarChunk;
    double m = 0.0;
#pragma unroll 4
    for (uint32_t k = 0; k < kOwn; ++k) {
        const unsigned long long rank = base + (unsigned long long)k * kThreads + threadIdx.x;
        if (rank < dim) m += probability(load_amp(st + order[rank]));
    }
    const double mass = block_sum(m, red);
    if (threadIdx.x == 0) chunk_mass[size_t(pos) * n_chunks + blockIdx.x] = mass;
}

// One workgroup per evaluation: the chunk in which the gathered mass reaches the target, the rank inside it (thread t owns ranks
// t kOwn .. t kOwn + kOwn - 1 of the chunk), and the pair (t, s) of cvar_gradient.hpp.
template <typename real>
__global__ void __launch_bounds__(kThreads)
cvar_gradient_rank_kernel(const gcx<real>* __restrict__ states, unsigned long long dim, const uint32_t* __restrict__ order,
                          const double* __restrict__ sorted, uint32_t n_chunks, const double* __restrict__ chunk_mass, double alpha,
                          double* __restrict__ pairs) {
    __shared__ double sh_sum[kThreads], sh_at[kThreads];
    __shared__ uint32_t sh_found[kThreads];
    __shared__ double total, chunk_before;
    __shared__ uint32_t chunk_found;
    const uint32_t pos = blockIdx.x, t = threadIdx.x;
    const double* mass = chunk_mass + size_t(pos) * n_chunks;
    const double target = alpha - (1e-8 + 1e-5 * fabs(alpha));  // isclose(gathered, alpha) with gathered <= alpha
    // ---- which chunk ----
    const uint32_t per = (n_chunks + kThreads - 1) / kThreads;
    const uint32_t lo = min(n_chunks, t * per), hi = min(n_chunks, lo + per);
    double local = 0.0;
    for (uint32_t c = lo; c < hi; ++c) local += mass[c];
    sh_sum[t] = local;
    const double all_mass = exclusive_scan_256(sh_sum, &total);
    {
        double cum = sh_sum[t], before = 0.0;
        uint32_t found = n_chunks;
        for (uint32_t c = lo; c < hi; ++c) {
            const double next = cum + mass[c];
            if (found == n_chunks && next >= target) {
                found = c;
                before = cum;
            }
            cum = next;
        }
        sh_found[t] = found;
        sh_at[t] = before;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t chunk = n_chunks;
        double before = 0.0;
        for (uint32_t i = 0; i < kThreads && chunk == n_chunks; ++i)
            if (sh_found[i] < n_chunks) {
                chunk = sh_found[i];
                before = sh_at[i];
            }
        chunk_found = chunk;
        chunk_before = before;
    }
    __syncthreads();
    const uint32_t chunk = chunk_found;
    const double mass_before = chunk_before;
    if (chunk == n_chunks) {  // (the whole distribution carries less than the target: the boundary is the last rank)
        if (t == 0) {
            pairs[size_t(pos) * 2 + 0] = sorted[dim - 1];
            pairs[size_t(pos) * 2 + 1] = fmax(alpha - all_mass, 0.0);
        }
        return;
    }
    // ---- which rank inside the chunk ----
    const gcx<real>* st = states + size_t(pos) * dim;
    const unsigned long long first = (unsigned long long)chunk * kCvarChunk + (unsigned long long)t * kOwn;
    double p[kOwn];
    double own = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < kOwn; ++k) {
        p[k] = first + k < dim ? probability(load_amp(st + order[first + k])) : 0.0;
        own += p[k];
    }
    __syncthreads();  // (thread 0 has read sh_found / sh_at)
    sh_sum[t] = own;
    const double chunk_mass_here = exclusive_scan_256(sh_sum, &total);
    {
        double cum = mass_before + sh_sum[t], at = 0.0;
        uint32_t found = kOwn;
#pragma unroll
        for (uint32_t k = 0; k < kOwn; ++k) {
            const double next = cum + p[k];
            if (found == kOwn && first + k < dim && next >= target) {
                found = k;
                at = next;
            }
            cum = next;
        }
        sh_found[t] = found;
        sh_at[t] = at;
    }
    __syncthreads();
    if (t == 0) {
        // (rounding: where the chunk's ranks one by one fall short of what the chunk scan saw, the boundary is the chunk's last rank)
        const unsigned long long chunk_end = min(dim, ((unsigned long long)chunk + 1) * kCvarChunk);
        unsigned long long rank = chunk_end - 1;
        double cum = mass_before + chunk_mass_here;
        for (uint32_t i = 0; i < kThreads; ++i)
            if (sh_found[i] < kOwn) {
                rank = (unsigned long long)chunk * kCvarChunk + (unsigned long long)i * kOwn + sh_found[i];
                cum = sh_at[i];
                break;
            }
        pairs[size_t(pos) * 2 + 0] = sorted[rank];
        pairs[size_t(pos) * 2 + 1] = fmax(alpha - cum, 0.0);
    }
}

// One streaming pass: consecutive lanes take consecutive amplitudes, so a wave reads and writes whole lines.
// grid: (adjoint_op_blocks(n), evaluations)
template <typename real>
__global__ void __launch_bounds__(kThreads)
cvar_gradient_seed_kernel(const gcx<real>* __restrict__ states, gcx<real>* __restrict__ lambda, unsigned long long dim,
                          const double* __restrict__ diag, const double* __restrict__ pairs, double alpha, bool streaming,
                          double* __restrict__ e_partials) {
    __shared__ double red[4];
    const uint32_t pos = blockIdx.y;
    const gcx<real>* st = states + size_t(pos) * dim;
    gcx<real>* lm = lambda ? lambda + size_t(pos) * dim : nullptr;
    const double t = pairs[size_t(pos) * 2];
    double acc = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < dim; i += stride) {
        const gcx<real> a = load_amp(st + i);
        const double w = -(fmax(t - diag[i], 0.0) / alpha);
        const double l_re = w * double(a.re), l_im = w * double(a.im);
        acc += double(a.re) * l_re + double(a.im) * l_im;
        if (lm) store_amp(lm + i, gcx<real>{real(l_re), real(l_im)}, streaming);
    }
    const double share = block_sum(acc, red);
    if (threadIdx.x == 0) e_partials[size_t(pos) * gridDim.x + blockIdx.x] = share;
}

// One thread per evaluation of the group.
__global__ void __launch_bounds__(64)
cvar_gradient_finish_kernel(const AdjEval* __restrict__ evals, uint32_t n_evals, const double* __restrict__ pairs, double alpha,
                            const double* __restrict__ largest_value, double* values, double* __restrict__ thresholds) {
    const uint32_t pos = blockIdx.x * 64 + threadIdx.x;
    if (pos >= n_evals) return;
    const size_t row = evals[pos].row;
    if (!pairs) {
        if (thresholds) thresholds[row] = *largest_value;
        return;
    }
    const double t = pairs[size_t(pos) * 2 + 0], s = pairs[size_t(pos) * 2 + 1];
    if (values) values[row] = t * (1.0 - s / alpha) + values[row];
    if (thresholds) thresholds[row] = t;
}

}  // namespace

hipError_t launch_cvar_gradient_threshold(int dtype, const void* states, int n_qubits, int n_evals, const uint32_t* order,
                                          const double* sorted_values, double alpha, double* scratch, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (!(alpha > 0.0) || alpha > 1.0 || n_qubits < 1 || n_qubits > 30) return hipErrorInvalidValue;
    const unsigned long long dim = 1ull << n_qubits;
    const uint32_t n_chunks = cvar_exact_chunks(dim);
    double* chunk_mass = scratch + size_t(n_evals) * 2;
    const dim3 grid(n_chunks, unsigned(n_evals));
    if (dtype == QSV_F64) {
        hipLaunchKernelGGL(cvar_gradient_chunks_kernel<double>, grid, dim3(kThreads), 0, stream, static_cast<const gcx<double>*>(states), dim,
                           order, n_chunks, chunk_mass);
        hipLaunchKernelGGL(cvar_gradient_rank_kernel<double>, dim3(unsigned(n_evals)), dim3(kThreads), 0, stream,
                           static_cast<const gcx<double>*>(states), dim, order, sorted_values, n_chunks, chunk_mass, alpha, scratch);
    } else {
        hipLaunchKernelGGL(cvar_gradient_chunks_kernel<float>, grid, dim3(kThreads), 0, stream, static_cast<const gcx<float>*>(states), dim,
                           order, n_chunks, chunk_mass);
        hipLaunchKernelGGL(cvar_gradient_rank_kernel<float>, dim3(unsigned(n_evals)), dim3(kThreads), 0, stream,
                           static_cast<const gcx<float>*>(states), dim, order, sorted_values, n_chunks, chunk_mass, alpha, scratch);
    }
    return hipGetLastError();
}

hipError_t launch_cvar_gradient_seed(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const double* diag,
                                     const double* scratch, double alpha, bool streaming, double* e_partials, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (!diag) return hipErrorInvalidValue;
    const dim3 grid(adjoint_op_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(cvar_gradient_seed_kernel<double>, grid, dim3(kThreads), 0, stream, static_cast<const gcx<double>*>(states),
                           static_cast<gcx<double>*>(lambda), dim, diag, scratch, alpha, streaming, e_partials);
    else
        hipLaunchKernelGGL(cvar_gradient_seed_kernel<float>, grid, dim3(kThreads), 0, stream, static_cast<const gcx<float>*>(states),
                           static_cast<gcx<float>*>(lambda), dim, diag, scratch, alpha, streaming, e_partials);
    return hipGetLastError();
}

hipError_t launch_cvar_gradient_finish(const AdjEval* evals, int n_evals, const double* scratch, double alpha, const double* largest_value,
                                       double* values, double* thresholds, hipStream_t stream) {
    if (n_evals <= 0 || (!thresholds && !(scratch && values))) return hipSuccess;
    hipLaunchKernelGGL(cvar_gradient_finish_kernel, dim3((unsigned(n_evals) + 63) / 64), dim3(64), 0, stream, evals, uint32_t(n_evals),
                       scratch, alpha, largest_value, values, thresholds);
    return hipGetLastError();
}

}  // namespace qsv
