// Operator-weighted reduced density matrices W_A = Tr_rest(H_h |psi><psi|) of qubit subsets A of up to four qubits
// (operator_density.hpp): with psi and lambda = H_h psi written as 2^k x 2^(n-k) matrices M and L, rows indexed
// by A's bits, W_A = L M^H is a GEMM over the 2^n amplitudes of two states.  The walk is reduced_density.hip's, driven by the same
// subset table: a workgroup is one wave, takes one (evaluation, subset) pair and walks blocks of A's qubits and the six lowest
// others, 2^k runs of 64 consecutive amplitudes each, so every load of either state is a full line.  An amplitude goes to its
// state's LDS panels at row a (A's bits) and column b (the other six); the 16 x 16 tiles lr pr^T, li pi^T, li pr^T and lr pi^T are
// accumulated on the fp64 matrix pipe, v_mfma_f64_16x16x4_f64 over four columns per instruction: Re W is the sum of the first
// two, Im W the third minus the fourth.  Every sum is fp64 whatever the states' type and runs in a fixed order: per workgroup over
// its blocks in ascending order, across workgroups in ascending order in the combine kernel.  No floating-point atomics.
#include "operator_density.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) ocx {  // (one load per amplitude)
    real re, im;
};

constexpr uint32_t kPanel = (kRdmSide + 1) * kRdmRow;  // (row 16: the spare row)

// the four registers of an accumulator to their places of a 16 x 16 tile: column = lane & 15, row = (lane >> 4) + 4 * register
__device__ __forceinline__ void store_tile(double* __restrict__ out, v4d acc, uint32_t lane) {
    out[((lane >> 4) + 0) * 16 + (lane & 15)] = acc.x;
    out[((lane >> 4) + 4) * 16 + (lane & 15)] = acc.y;
    out[((lane >> 4) + 8) * 16 + (lane & 15)] = acc.z;
    out[((lane >> 4) + 12) * 16 + (lane & 15)] = acc.w;
}

// grid: (workgroups, subsets, evaluations)
template <typename real>
__global__ void __launch_bounds__(64)
opdm_panels_kernel(const ocx<real>* __restrict__ states, const ocx<real>* __restrict__ lambdas, const RdmSubset* __restrict__ table,
                   unsigned long long dim, double* __restrict__ partials) {
    // (rows past 2^k, columns past 2^(n-k) and row 16 keep the zeros they are given here: no amplitude of a block goes to the
    // first two, and row 16, which is never read, takes what the dead lanes of a register below six qubits write)
    __shared__ double p_re[kPanel], p_im[kPanel], l_re[kPanel], l_im[kPanel];
    const uint32_t lane = threadIdx.x;
    const RdmSubset* __restrict__ sub = table + blockIdx.y;
    for (uint32_t j = 0; j <= kRdmSide; ++j) {
        const uint32_t w = j * kRdmRow + lane;
        p_re[w] = p_im[w] = l_re[w] = l_im[w] = 0.0;
    }
    // Fixed before the walk: where the lane's amplitude of a run goes in the panels, and which amplitude of the run it reads -- a
    // dead lane (n < 6: one run of 2^n) reads amplitude 0, which is there, and writes the spare row.
    const bool live = lane < dim;
    const uint32_t mine = live ? lane : 0u;
    uint32_t to = 0;
#pragma unroll
    for (uint32_t p = 0; p < 6; ++p) to += (lane >> p & 1u) * sub->lane_to[p];
    if (!live) to = kRdmSide * kRdmRow + lane;
    // lane l supplies the operand element (row l & 15, column 4 s + (l >> 4)) of both sides at step s
    const uint32_t at = (lane & 15) * kRdmRow + (lane >> 4);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    v4d rr = zero, ii = zero, ir = zero, ri = zero;
    const ocx<real>* __restrict__ state = states + size_t(blockIdx.z) * dim;
    const ocx<real>* __restrict__ lambda = lambdas + size_t(blockIdx.z) * dim;
    const uint32_t runs = sub->runs, blocks = sub->blocks, n_high = sub->n_high;
    for (uint32_t block = blockIdx.x; block < blocks; block += gridDim.x) {
        // the block's first amplitude: its number's bits at the qubits outside the block
        uint32_t first = block << 6;
        for (uint32_t j = 0; j < n_high; ++j) {
            const uint32_t p = sub->high[j];
            first = ((first >> p) << (p + 1)) | (first & ((1u << p) - 1u));
        }
        for (uint32_t t = 0; t < runs; ++t) {
            const uint32_t from = first + sub->run_at[t] + mine;
            const ocx<real> a = state[from], l = lambda[from];
            const uint32_t w = to + sub->run_to[t];
            p_re[w] = double(a.re);
            p_im[w] = double(a.im);
            l_re[w] = double(l.re);
            l_im[w] = double(l.im);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double pr = p_re[at + 4 * s], pi = p_im[at + 4 * s], lr = l_re[at + 4 * s], li = l_im[at + 4 * s];
            rr = __builtin_amdgcn_mfma_f64_16x16x4f64(lr, pr, rr, 0, 0, 0);
            ii = __builtin_amdgcn_mfma_f64_16x16x4f64(li, pi, ii, 0, 0, 0);
            ir = __builtin_amdgcn_mfma_f64_16x16x4f64(li, pr, ir, 0, 0, 0);
            ri = __builtin_amdgcn_mfma_f64_16x16x4f64(lr, pi, ri, 0, 0, 0);
        }
        __syncthreads();  // (the next block's panels go into the same LDS)
    }
    double* out = partials + ((size_t(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kOpdmPartial;
    store_tile(out, rr + ii, lane);
    store_tile(out + kOpdmPartial / 2, ir - ri, lane);
}

// One workgroup per (evaluation, subset), one thread per entry of the tile: a = t >> 4 the row, a' = t & 15 the column.
__global__ void __launch_bounds__(256)
opdm_combine_kernel(const double* __restrict__ partials, uint32_t blocks, const RdmSubset* __restrict__ table, size_t row,
                    double* __restrict__ out) {
    const uint32_t t = threadIdx.x, a = t >> 4, b = t & 15;
    const RdmSubset* __restrict__ sub = table + blockIdx.x;
    const double* p = partials + (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * blocks * kOpdmPartial;
    double re = 0.0, im = 0.0;
    for (uint32_t w = 0; w < blocks; ++w) {
        const double* q = p + size_t(w) * kOpdmPartial;
        re += q[t];
        im += q[kOpdmPartial / 2 + t];
    }
    const uint32_t side = 1u << sub->k;
    if (a >= side || b >= side) return;
    double* o = out + size_t(blockIdx.y) * row + sub->out_at + 2 * (a * side + b);
    o[0] = re;
    o[1] = im;
}

// One wave per evaluation.
__global__ void __launch_bounds__(64)
opdm_values_kernel(const double* __restrict__ e_partials, uint32_t op_blocks, double* __restrict__ values) {
    const uint32_t pos = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (uint32_t b = lane; b < op_blocks; b += 64) acc += e_partials[size_t(pos) * op_blocks + b];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) values[pos] = acc;
}

}  // namespace

hipError_t launch_opdm_panels(int dtype, const void* states, const void* lambda, int n_qubits, int n_evals, const RdmSubset* table,
                              uint32_t n_subsets, double* partials, hipStream_t stream) {
    if (n_evals <= 0 || n_subsets == 0) return hipSuccess;
    const dim3 grid(rdm_blocks(n_qubits), n_subsets, uint32_t(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL((opdm_panels_kernel<double>), grid, dim3(64), 0, stream, static_cast<const ocx<double>*>(states),
                           static_cast<const ocx<double>*>(lambda), table, dim, partials);
    else
        hipLaunchKernelGGL((opdm_panels_kernel<float>), grid, dim3(64), 0, stream, static_cast<const ocx<float>*>(states),
                           static_cast<const ocx<float>*>(lambda), table, dim, partials);
    return hipGetLastError();
}

hipError_t launch_opdm_combine(const double* partials, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets, size_t row,
                               double* out, hipStream_t stream) {
    if (n_evals <= 0 || n_subsets == 0) return hipSuccess;
    hipLaunchKernelGGL(opdm_combine_kernel, dim3(n_subsets, uint32_t(n_evals)), dim3(256), 0, stream, partials, rdm_blocks(n_qubits), table,
                       row, out);
    return hipGetLastError();
}

hipError_t launch_opdm_values(const double* e_partials, uint32_t op_blocks, int n_evals, double* values, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    hipLaunchKernelGGL(opdm_values_kernel, dim3(uint32_t(n_evals)), dim3(64), 0, stream, e_partials, op_blocks, values);
    return hipGetLastError();
}

}  // namespace qsv
