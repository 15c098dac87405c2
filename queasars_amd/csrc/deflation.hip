// Deflated (VQD) costs against kept states (deflation.hpp).  The seed of the adjoint sweep under the cost
// C_e = <psi_e|H_h|psi_e> + sum_k beta_k |<phi_k|psi_e>|^2 is lambda_e = H_h psi_e + sum_k (beta_k c_ek) phi_k: a complex product
// (evaluations x K) . (K x amplitudes) added to the lambda that adjoint_apply_operator_kernel has written.  It runs on the fp64
// matrix pipe, v_mfma_f64_16x16x4_f64, with overlap.hip's operand layout: a wave takes 16 evaluations x 64 amplitudes (four
// 16 x 16 tiles) and walks the kept states four at a time, in ascending position of the call's list.  The coefficients are the A
// operand, from LDS; the kept states are the B operand, read straight from memory -- 16 lanes read 16 consecutive amplitudes of
// one kept state, whole lines, once per 16 evaluations --; the C/D map puts 16 consecutive amplitudes of one evaluation in 16
// lanes, so lambda is read and written in whole lines too.  Every sum is fp64 whatever the states' type; an entry of a tile
// depends on its own row of coefficients and its own column of amplitudes only, so an evaluation's lambda does not depend on its
// batch or on its place in the launch group.  No floating-point atomics.
#include "deflation.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) dcx {  // (one access per amplitude)
    real re, im;
};

template <typename real>
__device__ __forceinline__ dcx<real> load_amp(const dcx<real>* p, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = streaming ? __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p)) : *reinterpret_cast<const vec2*>(p);
    return dcx<real>{v.x, v.y};
}
template <typename real>
__device__ __forceinline__ void store_amp(dcx<real>* p, dcx<real> a, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    vec2 v;
    v.x = a.re;
    v.y = a.im;
    if (streaming)
        __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
    else
        *reinterpret_cast<vec2*>(p) = v;
}

constexpr uint32_t kWaves = kDeflateThreads / 64;

// grid: (workgroups, blocks of 16 evaluations)
template <typename real>
__global__ void __launch_bounds__(kDeflateThreads)
deflate_kernel(dcx<real>* __restrict__ lambda, const dcx<real>* __restrict__ kept, const OverlapRefs refs, uint32_t n_refs,
               uint32_t n_evals, unsigned long long dim, const double* __restrict__ betas, const double* __restrict__ overlaps,
               bool streaming) {
    // w[k][evaluation] = beta_k c_ek, zero for the kept states past n_refs (the last step of four) and the rows past the group
    __shared__ double w_re[kOvlMaxStates * kOvlBlock], w_im[kOvlMaxStates * kOvlBlock];
    __shared__ uint32_t s_slot[kOvlMaxStates];  // (a position past n_refs reads the first kept state, which is there, times zero)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, eb = blockIdx.y;
    const uint32_t n_e = min(kOvlBlock, n_evals - eb * kOvlBlock);
    for (uint32_t i = tid; i < kOvlMaxStates * kOvlBlock; i += kDeflateThreads) {
        const uint32_t k = i >> 4, e = i & 15;
        double re = 0.0, im = 0.0;
        if (k < n_refs && e < n_e) {
            const double* c = overlaps + (size_t(eb * kOvlBlock + e) * n_refs + k) * 2;
            const double beta = betas[k];
            re = beta * c[0];
            im = beta * c[1];
        }
        w_re[i] = re;
        w_im[i] = im;
    }
    if (tid < kOvlMaxStates) s_slot[tid] = refs.slot[tid < n_refs ? tid : 0u];
    __syncthreads();
    // operand A[m][k]: lane l supplies m = l & 15 (the evaluation), k = l >> 4; operand B[k][n]: k = l >> 4, n = l & 15 (the
    // amplitude); D[m][n]: n = l & 15, m = (l >> 4) + 4 * register
    const uint32_t col = lane & 15, quad = lane >> 4;
    const uint32_t steps = (n_refs + 3) / 4;
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const unsigned long long chunks = (dim + 63) / 64;
    for (unsigned long long chunk = (unsigned long long)blockIdx.x * kWaves + wave; chunk < chunks;
         chunk += (unsigned long long)gridDim.x * kWaves) {
        // the lane's amplitude of each of the four tiles; past 2^n (a register below six qubits) it reads amplitude 0 and writes nothing
        unsigned long long amp[4];
        bool live[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long a = chunk * 64 + 16 * j + col;
            live[j] = a < dim;
            amp[j] = live[j] ? a : 0ull;
        }
        v4d acc_re[4] = {zero, zero, zero, zero}, acc_im[4] = {zero, zero, zero, zero};
        for (uint32_t s = 0; s < steps; ++s) {
            const uint32_t k = 4 * s + quad;
            const double wr = w_re[k * kOvlBlock + col], wi = w_im[k * kOvlBlock + col], nwi = -wi;
            const dcx<real>* ph = kept + (unsigned long long)s_slot[k] * dim;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const dcx<real> f = load_amp(ph + amp[j], streaming);
                const double fr = double(f.re), fi = double(f.im);
                // (w phi)_re = w_re phi_re - w_im phi_im, (w phi)_im = w_re phi_im + w_im phi_re
                acc_re[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr, fr, acc_re[j], 0, 0, 0);
                acc_re[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nwi, fi, acc_re[j], 0, 0, 0);
                acc_im[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr, fi, acc_im[j], 0, 0, 0);
                acc_im[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wi, fr, acc_im[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t e = quad + 4 * r;
                if (!live[j] || e >= n_e) continue;
                dcx<real>* p = lambda + (unsigned long long)(eb * kOvlBlock + e) * dim + amp[j];
                const dcx<real> l = load_amp(p, streaming);
                store_amp(p, dcx<real>{real(double(l.re) + acc_re[j][r]), real(double(l.im) + acc_im[j][r])}, streaming);
            }
        }
    }
}

// One wave per evaluation of the group.
__global__ void __launch_bounds__(64)
deflation_finish_kernel(const AdjEval* __restrict__ evals, uint32_t n_refs, const double* __restrict__ betas,
                        const double* __restrict__ overlaps, const double* energies, double* out_values,
                        double* __restrict__ out_overlaps) {
    const uint32_t pos = blockIdx.x, lane = threadIdx.x;
    const size_t row = evals[pos].row;
    const double* c = overlaps + size_t(pos) * n_refs * 2;
    if (out_overlaps)
        for (uint32_t i = lane; i < 2 * n_refs; i += 64) out_overlaps[row * n_refs * 2 + i] = c[i];
    if (out_values && lane == 0) {
        double penalty = 0.0;
        for (uint32_t k = 0; k < n_refs; ++k) penalty += betas[k] * (c[2 * k] * c[2 * k] + c[2 * k + 1] * c[2 * k + 1]);
        out_values[row] = energies[row] + penalty;
    }
}

}  // namespace

hipError_t launch_deflate(int dtype, void* lambda, const void* kept, const OverlapRefs& refs, uint32_t n_refs, int n_qubits, int n_evals,
                          const double* betas, const double* overlaps, bool streaming, hipStream_t stream) {
    if (n_evals <= 0 || n_refs == 0) return hipSuccess;
    const dim3 grid(deflate_blocks(n_qubits), overlap_state_blocks(size_t(n_evals)));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(deflate_kernel<double>, grid, dim3(kDeflateThreads), 0, stream, static_cast<dcx<double>*>(lambda),
                           static_cast<const dcx<double>*>(kept), refs, n_refs, uint32_t(n_evals), dim, betas, overlaps, streaming);
    else
        hipLaunchKernelGGL(deflate_kernel<float>, grid, dim3(kDeflateThreads), 0, stream, static_cast<dcx<float>*>(lambda),
                           static_cast<const dcx<float>*>(kept), refs, n_refs, uint32_t(n_evals), dim, betas, overlaps, streaming);
    return hipGetLastError();
}

hipError_t launch_deflation_finish(const AdjEval* evals, int n_evals, uint32_t n_refs, const double* betas, const double* overlaps,
                                   const double* energies, double* out_values, double* out_overlaps, hipStream_t stream) {
    if (n_evals <= 0 || (!out_values && !out_overlaps)) return hipSuccess;
    hipLaunchKernelGGL(deflation_finish_kernel, dim3(unsigned(n_evals)), dim3(64), 0, stream, evals, n_refs, betas, overlaps, energies,
                       out_values, out_overlaps);
    return hipGetLastError();
}

}  // namespace qsv
