// Overlaps <phi_k|psi_e> and operator matrix elements <phi_k|H_h|psi_e> of a launch group's states psi_e against kept states
// phi_k (overlap.hpp): Phi^H Psi over the 2^n rows is a plain GEMM.  A workgroup is one wave.  It takes one
// (block of 16 kept states, block of 16 evaluations) pair and 64 consecutive amplitudes at a time, writes them -- and, with the
// operator, lambda_e(i) = (H_h psi_e)_i from operator_row -- to LDS panels [state][amplitude] and accumulates the 16 x 16 complex
// tiles on the fp64 matrix pipe: v_mfma_f64_16x16x4_f64 sums over four amplitudes per instruction, real and imaginary parts as
// separate steps.  Every sum is fp64 whatever the state's type and runs in a fixed order: per workgroup over its amplitudes in
// ascending order, across workgroups in ascending order in the combine kernel.  An entry's sum does not depend on its place in
// the tile, nor on what the tile's other rows and columns hold.  No floating-point atomics.
#include "overlap.hpp"
#include "operator_row.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) ocx {  // (one load per amplitude)
    real re, im;
};

constexpr uint32_t kRow = 66;  // doubles per panel row: lanes m = 0 .. 15 read 8-byte words 4 m + 2 k apart, every bank once
constexpr uint32_t kPanel = (kOvlBlock + 1) * kRow;  // (row 16: the spare row)

// the four registers of an accumulator to their places of a 16 x 16 tile: column = lane & 15, row = (lane >> 4) + 4 * register
__device__ __forceinline__ void store_tile(double* __restrict__ out, v4d acc, uint32_t lane) {
    out[((lane >> 4) + 0) * 16 + (lane & 15)] = acc.x;
    out[((lane >> 4) + 4) * 16 + (lane & 15)] = acc.y;
    out[((lane >> 4) + 8) * 16 + (lane & 15)] = acc.z;
    out[((lane >> 4) + 12) * 16 + (lane & 15)] = acc.w;
}

// grid: (workgroups, blocks of kept states, blocks of evaluations)
template <typename real, bool kOperator>
__global__ void __launch_bounds__(64)
overlap_panels_kernel(const ocx<real>* __restrict__ states, const ocx<real>* __restrict__ kept, const OverlapRefs refs, uint32_t n_refs,
                      uint32_t n_evals, unsigned long long dim, const double* __restrict__ diag, int n_groups,
                      const PauliGroup* __restrict__ groups, const uint64_t* __restrict__ term_z, const double* __restrict__ term_coef,
                      const uint32_t* __restrict__ term_odd, double* __restrict__ partials) {
    // (row 16 of a panel is never read: what belongs to no state of the tile is written there, so the rows of unused kept states
    // and evaluations, and the amplitudes past 2^n of a register below six qubits, keep the zeros they are given here)
    __shared__ double f_re[kPanel], f_im[kPanel];  // phi: the block's kept states
    __shared__ double p_re[kPanel], p_im[kPanel];  // psi: the block's evaluations
    __shared__ double l_re[kOperator ? kPanel : 1], l_im[kOperator ? kPanel : 1];  // lambda = H_h psi
    const uint32_t lane = threadIdx.x, rb = blockIdx.y, eb = blockIdx.z;
    for (uint32_t j = 0; j <= kOvlBlock; ++j) {
        f_re[j * kRow + lane] = f_im[j * kRow + lane] = p_re[j * kRow + lane] = p_im[j * kRow + lane] = 0.0;
        if (kOperator) l_re[j * kRow + lane] = l_im[j * kRow + lane] = 0.0;
    }
    // lane l supplies the operand element (state l & 15, amplitude 4 s + (l >> 4) of the 64) of both sides at step s
    const uint32_t at = (lane & 15) * kRow + (lane >> 4);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    // Re S: phi_r psi_r + phi_i psi_i; Im S: phi_r psi_i (plus) - phi_i psi_r (minus, subtracted once at the end); T alike
    v4d s_re = zero, s_plus = zero, s_minus = zero, t_re = zero, t_plus = zero, t_minus = zero;
    // The tile's kept states n_r and evaluations n_e (1 .. 16 each).  A lane is dead where the register has fewer than 64
    // amplitudes (n < 6: one chunk).  Per row j, fixed before the walk: where the lane's amplitude of chunk 0 is in kept state
    // 16 rb + j and in evaluation 16 eb + j, and where it goes in the panel -- an unused row reads the block's first state, which is
    // there, at the lane's own amplitude, a dead lane reads amplitude 0 of its row's state, and both write row 16.  j is never a
    // run-time index.
    const uint32_t n_r = min(kOvlBlock, n_refs - rb * kOvlBlock), n_e = min(kOvlBlock, n_evals - eb * kOvlBlock);
    const bool live = lane < dim;
    const uint32_t spare = kOvlBlock * kRow + lane, mine = live ? lane : 0u;
    unsigned long long ref_at[kOvlBlock], eval_at[kOperator ? 1 : kOvlBlock];
    uint32_t ref_to[kOvlBlock], eval_to[kOperator ? 1 : kOvlBlock];
#pragma unroll
    for (uint32_t j = 0; j < kOvlBlock; ++j) {
        // (the state numbers go to vector registers at once: sixteen products kept in scalar registers are more than there are)
        uint32_t slot = refs.slot[rb * kOvlBlock + (j < n_r ? j : 0u)], e = eb * kOvlBlock + (j < n_e ? j : 0u);
        asm volatile("" : "+v"(slot), "+v"(e));
        ref_at[j] = (unsigned long long)slot * dim + mine;
        ref_to[j] = live && j < n_r ? j * kRow + lane : spare;
        if constexpr (!kOperator) {
            eval_at[j] = (unsigned long long)e * dim + mine;
            eval_to[j] = live && j < n_e ? j * kRow + lane : spare;
        }
    }
    const unsigned long long chunks = (dim + 63) / 64;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
#pragma unroll
        for (uint32_t j = 0; j < kOvlBlock; ++j) {
            const ocx<real> a = kept[ref_at[j] + chunk * 64];
            f_re[ref_to[j]] = double(a.re);
            f_im[ref_to[j]] = double(a.im);
        }
        if constexpr (kOperator) {
            // lambda is formed here, once per (amplitude, evaluation, block of kept states); an unused row is skipped
            for (uint32_t j = 0; j < n_e; ++j) {
                const ocx<real>* st = states + size_t(eb * kOvlBlock + j) * dim;
                const unsigned long long i = chunk * 64 + mine;
                const ocx<real> a = st[i];
                const OperatorRow row = operator_row(st, i, a, diag, n_groups, groups, term_z, term_coef, term_odd);
                const uint32_t w = live ? j * kRow + lane : spare;
                p_re[w] = double(a.re);
                p_im[w] = double(a.im);
                l_re[w] = row.re;
                l_im[w] = row.im;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kOvlBlock; ++j) {
                const ocx<real> a = states[eval_at[j] + chunk * 64];
                p_re[eval_to[j]] = double(a.re);
                p_im[eval_to[j]] = double(a.im);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double fr = f_re[at + 4 * s], fi = f_im[at + 4 * s];
            const double pr = p_re[at + 4 * s], pi = p_im[at + 4 * s];
            s_re = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, pr, s_re, 0, 0, 0);
            s_plus = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, pi, s_plus, 0, 0, 0);
            s_minus = __builtin_amdgcn_mfma_f64_16x16x4f64(fi, pr, s_minus, 0, 0, 0);
            s_re = __builtin_amdgcn_mfma_f64_16x16x4f64(fi, pi, s_re, 0, 0, 0);
            if (kOperator) {
                const double lr = l_re[at + 4 * s], li = l_im[at + 4 * s];
                t_re = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, lr, t_re, 0, 0, 0);
                t_plus = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, li, t_plus, 0, 0, 0);
                t_minus = __builtin_amdgcn_mfma_f64_16x16x4f64(fi, lr, t_minus, 0, 0, 0);
                t_re = __builtin_amdgcn_mfma_f64_16x16x4f64(fi, li, t_re, 0, 0, 0);
            }
        }
        __syncthreads();  // (the next chunk's panels go into the same LDS)
    }
    double* out = partials + ((size_t(eb) * gridDim.y + rb) * gridDim.x + blockIdx.x) * (kOperator ? 2 * kOvlTile : kOvlTile);
    store_tile(out, s_re, lane);
    store_tile(out + kOvlTile / 2, s_plus - s_minus, lane);
    if (kOperator) {
        store_tile(out + kOvlTile, t_re, lane);
        store_tile(out + kOvlTile + kOvlTile / 2, t_plus - t_minus, lane);
    }
}

// One workgroup per pair of blocks, one thread per entry of the tile: r = t >> 4 the kept state, c = t & 15 the evaluation.
__global__ void __launch_bounds__(256)
overlap_combine_kernel(const double* __restrict__ partials, uint32_t blocks, uint32_t partial, uint32_t n_refs, uint32_t n_evals,
                       double* __restrict__ out_s, double* __restrict__ out_t) {
    const uint32_t t = threadIdx.x, rb = blockIdx.x, eb = blockIdx.y;
    const double* p = partials + (size_t(eb) * gridDim.x + rb) * blocks * partial + t;
    double s_re = 0.0, s_im = 0.0, t_re = 0.0, t_im = 0.0;
    for (uint32_t w = 0; w < blocks; ++w) {
        const double* q = p + size_t(w) * partial;
        s_re += q[0];
        s_im += q[kOvlTile / 2];
        if (out_t) {
            t_re += q[kOvlTile];
            t_im += q[kOvlTile + kOvlTile / 2];
        }
    }
    const uint32_t k = rb * kOvlBlock + (t >> 4), e = eb * kOvlBlock + (t & 15);
    if (k >= n_refs || e >= n_evals) return;
    const size_t at = (size_t(e) * n_refs + k) * 2;
    out_s[at] = s_re;
    out_s[at + 1] = s_im;
    if (out_t) {
        out_t[at] = t_re;
        out_t[at + 1] = t_im;
    }
}

template <typename real>
void launch_panels(const void* states, const void* kept, const OverlapRefs& refs, uint32_t n_refs, int n_qubits, int n_evals,
                   const OperatorView& op, double* partials, hipStream_t stream) {
    const dim3 grid(overlap_blocks(n_qubits), overlap_state_blocks(n_refs), overlap_state_blocks(size_t(n_evals)));
    const unsigned long long dim = 1ull << n_qubits;
    const ocx<real>* st = static_cast<const ocx<real>*>(states);
    const ocx<real>* kp = static_cast<const ocx<real>*>(kept);
    if (op.n_groups >= 0)
        hipLaunchKernelGGL((overlap_panels_kernel<real, true>), grid, dim3(64), 0, stream, st, kp, refs, n_refs, uint32_t(n_evals), dim, op.diag,
                           op.n_groups, op.groups, op.term_z, op.term_coef, op.term_odd, partials);
    else
        hipLaunchKernelGGL((overlap_panels_kernel<real, false>), grid, dim3(64), 0, stream, st, kp, refs, n_refs, uint32_t(n_evals), dim,
                           nullptr, 0, nullptr, nullptr, nullptr, nullptr, partials);
}

}  // namespace

hipError_t launch_overlap_panels(int dtype, const void* states, const void* kept, const OverlapRefs& refs, uint32_t n_refs, int n_qubits,
                                 int n_evals, const OperatorView& op, double* partials, hipStream_t stream) {
    if (n_evals <= 0 || n_refs == 0) return hipSuccess;
    if (dtype == QSV_F64)
        launch_panels<double>(states, kept, refs, n_refs, n_qubits, n_evals, op, partials, stream);
    else
        launch_panels<float>(states, kept, refs, n_refs, n_qubits, n_evals, op, partials, stream);
    return hipGetLastError();
}

hipError_t launch_overlap_combine(const double* partials, int n_qubits, int n_evals, uint32_t n_refs, double* out_s, double* out_t,
                                  hipStream_t stream) {
    if (n_evals <= 0 || n_refs == 0) return hipSuccess;
    hipLaunchKernelGGL(overlap_combine_kernel, dim3(overlap_state_blocks(n_refs), overlap_state_blocks(size_t(n_evals))), dim3(256), 0, stream,
                       partials, overlap_blocks(n_qubits), overlap_partial(out_t != nullptr), n_refs, uint32_t(n_evals), out_s, out_t);
    return hipGetLastError();
}

}  // namespace qsv
