// Reduced density matrices rho_A = Tr_rest |psi><psi| of qubit subsets A of up to four qubits (reduced_density.hpp, DESIGN.md
// 4.16): with the state written as a 2^k x 2^(n-k) matrix M, rows indexed by A's bits, rho_A = M M^H is a GEMM over the 2^n
// amplitudes.  A workgroup is one wave.  It takes one (evaluation, subset) pair and walks blocks: the 2^(k+6) amplitudes spanned by
// A's qubits and the six lowest qubits outside A.  Such a block always holds qubits 0 .. 5, so it is 2^k runs of 64 consecutive
// amplitudes and every load is a full line whichever qubits A names.  An amplitude goes to the LDS panel at row a (A's bits) and
// column b (the other six); the 16 x 16 tiles Re rho = sum r_a r_a' + i_a i_a' and X = sum i_a r_a' are accumulated on the fp64
// matrix pipe, v_mfma_f64_16x16x4_f64 over four columns per instruction.  Every sum is fp64 whatever the state's type and runs in
// a fixed order: per workgroup over its blocks in ascending order, across workgroups in ascending order in the combine kernel,
// which forms Im rho = X - X^T.  No floating-point atomics.
#include "reduced_density.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) rcx {  // (one load per amplitude)
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
rdm_panels_kernel(const rcx<real>* __restrict__ states, const RdmSubset* __restrict__ table, unsigned long long dim,
                  double* __restrict__ partials) {
    // (rows past 2^k, columns past 2^(n-k) and row 16 keep the zeros they are given here: no amplitude of a block goes to the
    // first two, and row 16, which is never read, takes what the dead lanes of a register below six qubits write)
    __shared__ double m_re[kPanel], m_im[kPanel];
    const uint32_t lane = threadIdx.x;
    const RdmSubset* __restrict__ sub = table + blockIdx.y;
    for (uint32_t j = 0; j <= kRdmSide; ++j) m_re[j * kRdmRow + lane] = m_im[j * kRdmRow + lane] = 0.0;
    // Fixed before the walk: where the lane's amplitude of a run goes in the panel, and which amplitude of the run it reads -- a
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
    v4d rr = zero, ii = zero, x = zero;
    const rcx<real>* __restrict__ state = states + size_t(blockIdx.z) * dim;
    const uint32_t runs = sub->runs, blocks = sub->blocks, n_high = sub->n_high;
    for (uint32_t block = blockIdx.x; block < blocks; block += gridDim.x) {
        // the block's first amplitude: its number's bits at the qubits outside the block
        uint32_t first = block << 6;
        for (uint32_t j = 0; j < n_high; ++j) {
            const uint32_t p = sub->high[j];
            first = ((first >> p) << (p + 1)) | (first & ((1u << p) - 1u));
        }
        for (uint32_t t = 0; t < runs; ++t) {
            const rcx<real> a = state[first + sub->run_at[t] + mine];
            const uint32_t w = to + sub->run_to[t];
            m_re[w] = double(a.re);
            m_im[w] = double(a.im);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double r = m_re[at + 4 * s], i = m_im[at + 4 * s];
            rr = __builtin_amdgcn_mfma_f64_16x16x4f64(r, r, rr, 0, 0, 0);
            ii = __builtin_amdgcn_mfma_f64_16x16x4f64(i, i, ii, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(i, r, x, 0, 0, 0);
        }
        __syncthreads();  // (the next block's panel goes into the same LDS)
    }
    double* out = partials + ((size_t(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kRdmPartial;
    store_tile(out, rr + ii, lane);
    store_tile(out + kRdmPartial / 2, x, lane);
}

// One workgroup per (evaluation, subset), one thread per entry of the tile: a = t >> 4 the row, a' = t & 15 the column.  Re rho
// is summed where it stands above the diagonal, so both triangles hold one sum; X is summed at the entry and at its mirror image
// -- the mirror thread forms the same two sums, so Im rho = X - X^T is antisymmetric and zero on the diagonal to the bit.
__global__ void __launch_bounds__(256)
rdm_combine_kernel(const double* __restrict__ partials, uint32_t blocks, const RdmSubset* __restrict__ table, size_t row,
                   double* __restrict__ out) {
    const uint32_t t = threadIdx.x, a = t >> 4, b = t & 15;
    const RdmSubset* __restrict__ sub = table + blockIdx.x;
    const double* p = partials + (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * blocks * kRdmPartial;
    const uint32_t upper = min(a, b) * 16 + max(a, b), here = kRdmPartial / 2 + a * 16 + b, mirror = kRdmPartial / 2 + b * 16 + a;
    double re = 0.0, x = 0.0, xt = 0.0;
    for (uint32_t w = 0; w < blocks; ++w) {
        const double* q = p + size_t(w) * kRdmPartial;
        re += q[upper];
        x += q[here];
        xt += q[mirror];
    }
    const uint32_t side = 1u << sub->k;
    if (a >= side || b >= side) return;
    double* o = out + size_t(blockIdx.y) * row + sub->out_at + 2 * (a * side + b);
    o[0] = re;
    o[1] = x - xt;
}

}  // namespace

hipError_t launch_rdm_panels(int dtype, const void* states, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets,
                             double* partials, hipStream_t stream) {
    if (n_evals <= 0 || n_subsets == 0) return hipSuccess;
    const dim3 grid(rdm_blocks(n_qubits), n_subsets, uint32_t(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL((rdm_panels_kernel<double>), grid, dim3(64), 0, stream, static_cast<const rcx<double>*>(states), table, dim, partials);
    else
        hipLaunchKernelGGL((rdm_panels_kernel<float>), grid, dim3(64), 0, stream, static_cast<const rcx<float>*>(states), table, dim, partials);
    return hipGetLastError();
}

hipError_t launch_rdm_combine(const double* partials, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets, size_t row,
                              double* out, hipStream_t stream) {
    if (n_evals <= 0 || n_subsets == 0) return hipSuccess;
    hipLaunchKernelGGL(rdm_combine_kernel, dim3(n_subsets, uint32_t(n_evals)), dim3(256), 0, stream, partials, rdm_blocks(n_qubits), table,
                       row, out);
    return hipGetLastError();
}

}  // namespace qsv
