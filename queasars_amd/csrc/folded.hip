// Folded-spectrum and variance costs (folded.hpp): the centre, the residual, the seed and the finishing kernel.
// Every sum is fp64 and is formed in a fixed order -- per thread over its amplitudes in ascending order, across a wave by a
// butterfly, across waves and workgroups in index order --, so an evaluation's centre, cost and seed depend on nothing but its
// state, the operator and the target.  No floating-point atomics.
#include "folded.hpp"
#include "operator_row.hpp"

namespace qsv {

namespace {

template <typename real>
struct alignas(2 * sizeof(real)) fcx {  // (one access per amplitude)
    real re, im;
};

template <typename real>
__device__ __forceinline__ fcx<real> load_amp(const fcx<real>* p) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = *reinterpret_cast<const vec2*>(p);
    return fcx<real>{v.x, v.y};
}
template <typename real>
__device__ __forceinline__ void store_amp(fcx<real>* p, fcx<real> a, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    vec2 v;
    v.x = a.re;
    v.y = a.im;
    if (streaming)
        __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
    else
        *reinterpret_cast<vec2*>(p) = v;
}

constexpr uint32_t kThreads = 256;
static_assert(kThreads == uint32_t(kAdjointThreads), "the passes have launch_adjoint_apply_operator's grid");

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

// One wave per evaluation: adjoint_combine_kernel's sum of the row's e_partials.
__global__ void __launch_bounds__(64)
folded_centre_kernel(const double* __restrict__ e_partials, uint32_t op_blocks, bool own_mean, double target, double* __restrict__ pairs) {
    const uint32_t pos = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (uint32_t b = lane; b < op_blocks; b += 64) acc += e_partials[size_t(pos) * op_blocks + b];
    acc = wave_sum(acc);
    if (lane == 0) {
        pairs[size_t(pos) * 2 + 0] = acc;
        pairs[size_t(pos) * 2 + 1] = own_mean ? acc : target;
    }
}

// One streaming pass: consecutive lanes take consecutive amplitudes, so a wave reads and writes whole lines.
// grid: (folded_blocks(n), evaluations)
template <typename real>
__global__ void __launch_bounds__(kThreads)
folded_residual_kernel(const fcx<real>* __restrict__ states, const fcx<real>* __restrict__ lambda1, fcx<real>* __restrict__ residual,
                       unsigned long long dim, const double* __restrict__ pairs, bool streaming, double* __restrict__ shares) {
    __shared__ double red[4];
    const uint32_t pos = blockIdx.y;
    const fcx<real>* st = states + size_t(pos) * dim;
    const fcx<real>* l1 = lambda1 + size_t(pos) * dim;
    fcx<real>* rs = residual ? residual + size_t(pos) * dim : nullptr;
    const double c = pairs[size_t(pos) * 2 + 1];
    double acc = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < dim; i += stride) {
        const fcx<real> a = load_amp(st + i), l = load_amp(l1 + i);
        const double r_re = double(l.re) - c * double(a.re), r_im = double(l.im) - c * double(a.im);
        acc += fma(r_re, r_re, r_im * r_im);
        if (rs) store_amp(rs + i, fcx<real>{real(r_re), real(r_im)}, streaming);
    }
    const double share = block_sum(acc, red);
    if (threadIdx.x == 0) shares[size_t(pos) * gridDim.x + blockIdx.x] = share;
}

// lambda = (H_h - c) r - (E - c)^2 psi, row by row (operator_row.hpp) over the residual.  grid: (folded_blocks(n), evaluations)
template <typename real>
__global__ void __launch_bounds__(kThreads)
folded_seed_kernel(const fcx<real>* __restrict__ states, const fcx<real>* __restrict__ residual, fcx<real>* __restrict__ lambda,
                   unsigned long long dim, const double* __restrict__ diag, int n_groups, const PauliGroup* __restrict__ groups,
                   const uint64_t* __restrict__ term_z, const double* __restrict__ term_coef, const uint32_t* __restrict__ term_odd,
                   const double* __restrict__ pairs, bool streaming) {
    const uint32_t pos = blockIdx.y;
    const fcx<real>* st = states + size_t(pos) * dim;
    const fcx<real>* rs = residual + size_t(pos) * dim;
    fcx<real>* lm = lambda + size_t(pos) * dim;
    const double c = pairs[size_t(pos) * 2 + 1], off = pairs[size_t(pos) * 2] - c, shift = off * off;
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < dim; i += stride) {
        const fcx<real> r = load_amp(rs + i), a = load_amp(st + i);
        const OperatorRow row = operator_row(rs, i, r, diag, n_groups, groups, term_z, term_coef, term_odd);
        const double l_re = (row.re - c * double(r.re)) - shift * double(a.re), l_im = (row.im - c * double(r.im)) - shift * double(a.im);
        store_amp(lm + i, fcx<real>{real(l_re), real(l_im)}, streaming);
    }
}

// An operator of its diagonal part alone: residual and seed in one streaming pass.  grid: (folded_blocks(n), evaluations)
template <typename real>
__global__ void __launch_bounds__(kThreads)
folded_diagonal_kernel(const fcx<real>* __restrict__ states, fcx<real>* __restrict__ lambda, unsigned long long dim,
                       const double* __restrict__ diag, const double* __restrict__ pairs, bool streaming, double* __restrict__ shares) {
    __shared__ double red[4];
    const uint32_t pos = blockIdx.y;
    const fcx<real>* st = states + size_t(pos) * dim;
    fcx<real>* lm = lambda ? lambda + size_t(pos) * dim : nullptr;
    const double c = pairs[size_t(pos) * 2 + 1], off = pairs[size_t(pos) * 2] - c, shift = off * off;
    double acc = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < dim; i += stride) {
        const fcx<real> a = load_amp(st + i);
        const double w = diag[i] - c;
        const double r_re = w * double(a.re), r_im = w * double(a.im);
        acc += fma(r_re, r_re, r_im * r_im);
        if (lm) store_amp(lm + i, fcx<real>{real(w * r_re - shift * double(a.re)), real(w * r_im - shift * double(a.im))}, streaming);
    }
    const double share = block_sum(acc, red);
    if (threadIdx.x == 0) shares[size_t(pos) * gridDim.x + blockIdx.x] = share;
}

// One thread per evaluation of the group.
__global__ void __launch_bounds__(64)
folded_finish_kernel(const AdjEval* __restrict__ evals, uint32_t n_evals, uint32_t blocks, const double* __restrict__ pairs,
                     const double* __restrict__ shares, double* __restrict__ values, double* __restrict__ energies) {
    const uint32_t pos = blockIdx.x * 64 + threadIdx.x;
    if (pos >= n_evals) return;
    const size_t row = evals[pos].row;
    if (values) {
        double cost = 0.0;
        for (uint32_t b = 0; b < blocks; ++b) cost += shares[size_t(pos) * blocks + b];
        values[row] = cost;
    }
    if (energies) energies[row] = pairs[size_t(pos) * 2];
}

}  // namespace

hipError_t launch_folded_centre(const double* e_partials, uint32_t op_blocks, int n_evals, bool own_mean, double target, double* scratch,
                                hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    hipLaunchKernelGGL(folded_centre_kernel, dim3(unsigned(n_evals)), dim3(64), 0, stream, e_partials, op_blocks, own_mean, target, scratch);
    return hipGetLastError();
}

hipError_t launch_folded_residual(int dtype, const void* states, const void* lambda1, void* residual, int n_qubits, int n_evals,
                                  double* scratch, bool streaming, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (n_qubits < 1 || n_qubits > 30 || residual == lambda1) return hipErrorInvalidValue;
    const dim3 grid(folded_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    double* shares = scratch + size_t(n_evals) * 2;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(folded_residual_kernel<double>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<double>*>(states),
                           static_cast<const fcx<double>*>(lambda1), static_cast<fcx<double>*>(residual), dim, scratch, streaming, shares);
    else
        hipLaunchKernelGGL(folded_residual_kernel<float>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<float>*>(states),
                           static_cast<const fcx<float>*>(lambda1), static_cast<fcx<float>*>(residual), dim, scratch, streaming, shares);
    return hipGetLastError();
}

hipError_t launch_folded_seed(int dtype, const void* states, const void* residual, void* lambda, int n_qubits, int n_evals,
                              const OperatorView& op, const double* scratch, bool streaming, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (n_qubits < 1 || n_qubits > 30 || !states || !residual || !lambda || residual == lambda) return hipErrorInvalidValue;
    const dim3 grid(folded_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(folded_seed_kernel<double>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<double>*>(states),
                           static_cast<const fcx<double>*>(residual), static_cast<fcx<double>*>(lambda), dim, op.diag, op.n_groups, op.groups, op.term_z, op.term_coef, op.term_odd,
                           scratch, streaming);
    else
        hipLaunchKernelGGL(folded_seed_kernel<float>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<float>*>(states),
                           static_cast<const fcx<float>*>(residual), static_cast<fcx<float>*>(lambda), dim, op.diag, op.n_groups, op.groups, op.term_z, op.term_coef, op.term_odd,
                           scratch, streaming);
    return hipGetLastError();
}

hipError_t launch_folded_diagonal(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const double* diag,
                                  double* scratch, bool streaming, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (n_qubits < 1 || n_qubits > 30 || !diag) return hipErrorInvalidValue;
    const dim3 grid(folded_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    double* shares = scratch + size_t(n_evals) * 2;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(folded_diagonal_kernel<double>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<double>*>(states),
                           static_cast<fcx<double>*>(lambda), dim, diag, scratch, streaming, shares);
    else
        hipLaunchKernelGGL(folded_diagonal_kernel<float>, grid, dim3(kThreads), 0, stream, static_cast<const fcx<float>*>(states),
                           static_cast<fcx<float>*>(lambda), dim, diag, scratch, streaming, shares);
    return hipGetLastError();
}

hipError_t launch_folded_finish(const AdjEval* evals, int n_evals, int n_qubits, const double* scratch, double* values, double* energies,
                                hipStream_t stream) {
    if (n_evals <= 0 || (!values && !energies)) return hipSuccess;
    hipLaunchKernelGGL(folded_finish_kernel, dim3((unsigned(n_evals) + 63) / 64), dim3(64), 0, stream, evals, uint32_t(n_evals),
                       folded_blocks(n_qubits), scratch, scratch + size_t(n_evals) * 2, values, energies);
    return hipGetLastError();
}

}  // namespace qsv
