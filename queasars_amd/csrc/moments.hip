// The operator's first two moments (moments.hpp): m1 = Re<psi|H_h psi> and m2 = |H_h psi|^2 from one read of the
// state per x-mask group, no H_h psi stored.  Both sums are fp64 whatever the state's type and are formed in a fixed order -- per
// thread over its rows, across a wave by a butterfly, across the waves in wave order, across workgroups lane-strided in ascending
// order and by the butterfly again --, so an evaluation's numbers depend on nothing but its circuit, its point and the operator.
// No floating-point atomics.
#include "moments.hpp"
#include "operator_row.hpp"

namespace qsv {

namespace {

template <typename real>
struct alignas(2 * sizeof(real)) mcx {  // (one load per amplitude)
    real re, im;
};

// every lane receives the sum of the wave's 64 values, added in the butterfly's order
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// A thread walks the rows i = block * 256 + tid, += blocks * 256 of the state in its slot.  The state is read by plain loads (16
// bytes in fp64, 8 in fp32): every group reads it again, so it should stay in the caches.
template <typename real>
__global__ void __launch_bounds__(kMomentsThreads)
operator_moments_kernel(const mcx<real>* __restrict__ states, unsigned long long dim, const double* __restrict__ diag, int n_groups,
                        const PauliGroup* __restrict__ groups, const uint64_t* __restrict__ term_z,
                        const double* __restrict__ term_coef, const uint32_t* __restrict__ term_odd, double* __restrict__ partials) {
    __shared__ double red[2 * (kMomentsThreads / 64)];
    const uint32_t pos = blockIdx.y;
    const mcx<real>* st = states + size_t(pos) * dim;
    double m1 = 0.0, m2 = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kMomentsThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kMomentsThreads + threadIdx.x; i < dim; i += stride) {
        const mcx<real> a = st[i];
        const OperatorRow row = operator_row(st, i, a, diag, n_groups, groups, term_z, term_coef, term_odd);
        const double l_re = row.re, l_im = row.im;
        m1 += double(a.re) * l_re + double(a.im) * l_im;
        m2 += l_re * l_re + l_im * l_im;
    }
    m1 = wave_sum(m1);
    m2 = wave_sum(m2);
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = m1;
        red[2 * (threadIdx.x >> 6) + 1] = m2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        typedef double vec2 __attribute__((ext_vector_type(2)));
        vec2 v;
        v.x = ((red[0] + red[2]) + red[4]) + red[6];
        v.y = ((red[1] + red[3]) + red[5]) + red[7];
        *reinterpret_cast<vec2*>(partials + (size_t(pos) * gridDim.x + blockIdx.x) * 2) = v;
    }
}

// One wave per evaluation.
__global__ void __launch_bounds__(64)
moments_combine_kernel(const double* __restrict__ partials, uint32_t blocks, double* __restrict__ out) {
    const uint32_t pos = blockIdx.x, lane = threadIdx.x;
    const double* p = partials + size_t(pos) * blocks * 2;
    double m1 = 0.0, m2 = 0.0;
    for (uint32_t b = lane; b < blocks; b += 64) {
        m1 += p[2 * b];
        m2 += p[2 * b + 1];
    }
    m1 = wave_sum(m1);
    m2 = wave_sum(m2);
    if (lane == 0) {
        out[size_t(pos) * 2] = m1;
        out[size_t(pos) * 2 + 1] = m2 - m1 * m1;
    }
}

}  // namespace

hipError_t launch_operator_moments(int dtype, const void* states, int n_qubits, int n_evals, const OperatorView& op, double* partials,
                                   hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    const dim3 grid(moments_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(operator_moments_kernel<double>, grid, dim3(kMomentsThreads), 0, stream, static_cast<const mcx<double>*>(states),
                           dim, op.diag, op.n_groups, op.groups, op.term_z, op.term_coef, op.term_odd, partials);
    else
        hipLaunchKernelGGL(operator_moments_kernel<float>, grid, dim3(kMomentsThreads), 0, stream, static_cast<const mcx<float>*>(states),
                           dim, op.diag, op.n_groups, op.groups, op.term_z, op.term_coef, op.term_odd, partials);
    return hipGetLastError();
}

hipError_t launch_moments_combine(const double* partials, uint32_t blocks, int n_evals, double* out, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    hipLaunchKernelGGL(moments_combine_kernel, dim3(unsigned(n_evals)), dim3(64), 0, stream, partials, blocks, out);
    return hipGetLastError();
}

}  // namespace qsv
